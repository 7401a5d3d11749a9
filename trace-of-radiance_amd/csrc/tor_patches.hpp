// tor_patches.hpp -- what tor_api.cpp tells the patch table of a context (tor_patches.hip, include/tor_patches.h).  The table lives
// in tor_patches.hip, keyed by the context: the two events of a context's life that concern it arrive through these calls.
#pragma once

struct TorContext;

namespace tor {

// a tor_scene_upload replaced the scene (the device is idle): the context has no patch table any more
void patches_scene_replaced(TorContext* ctx);
// tor_context_destroy, with the context's device current: the table's device copy is freed and the context forgotten
void patches_context_destroyed(TorContext* ctx);

}  // namespace tor
