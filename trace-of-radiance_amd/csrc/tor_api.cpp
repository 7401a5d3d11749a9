// tor_api.cpp -- the C ABI of libtor_mi355x.so (include/tor_render.h): context, scene
// flattening (AoS HittableVariant -> device SoA), launch orchestration, error reporting.
// There is NO CPU fallback: without a HIP device every rendering entry point fails with
// TOR_ERR_NO_DEVICE.
#include "../../include/tor_render.h"

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "tor_context.hpp"
#include "tor_knobs.hpp"
#include "tor_patches.hpp"
#include "tor_screen.hpp"

// ---- layout guards: the structs must match what Nim's C backend emits --------
static_assert(sizeof(TorVec3) == 24, "Vec3 is 3 x float64 (vec3s.nim:12-14)");
static_assert(sizeof(TorMaterial) == 40 && offsetof(TorMaterial, u) == 8, "Material (core.nim:16-28)");
static_assert(sizeof(TorSphere) == 72, "Sphere (spheres.nim:15-18)");
static_assert(sizeof(TorMovingSphere) == 112, "MovingSphere (moving_spheres.nim:15-20)");
static_assert(sizeof(TorHittableVariant) == 120 && offsetof(TorHittableVariant, u) == 8,
              "HittableVariant (hittables_variants.nim:50-57)");
static_assert(sizeof(TorHittableList) == 16, "HittableList (hittables_lists.nim:20-24)");
static_assert(sizeof(TorCamera) == 192, "Camera (cameras.nim:15-22)");
static_assert(sizeof(TorCanvas) == 24, "Canvas (canvas.nim:20-28)");
static_assert(sizeof(tor::Camera) == sizeof(TorCamera), "device camera mirrors TorCamera");
static_assert(offsetof(TorOptions, device_count) == 32, "the round-1 TorOptions is a prefix of the current one");

namespace {
std::mutex g_handoff_mutex;                    // hand-off launches are chained per device (tor_render_device)
std::map<int, hipEvent_t> g_handoff_event;     // device -> end of the last hand-off launch of this process
thread_local std::string g_last_error = "";
thread_local double g_last_timing[5] = {0, 0, 0, 0, 0};
}  // namespace

namespace tor {

void set_last_error(const std::string& msg) { g_last_error = msg; }  // for the host-only sources (tor_mp4.cpp)

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int fail_hip(hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
    return fail(TOR_ERR_NO_DEVICE, m + " (libtor_mi355x has no CPU fallback)");
  if (e == hipErrorOutOfMemory) return fail(TOR_ERR_OUT_OF_MEMORY, m);
  return fail(TOR_ERR_HIP, m);
}

hipError_t DeviceLayout::put(const HostLayout& lay, const std::vector<double>* cold_override) {
  const std::vector<double>& c = cold_override ? *cold_override : lay.cold;
  struct Part { const void* src; size_t bytes; size_t off; };
  Part parts[13] = {{lay.stat.data(), lay.stat.size() * 8, 0}, {lay.mov.data(), lay.mov.size() * 8, 0},
                   {lay.movy.data(), lay.movy.size() * 8, 0}, {lay.segs.data(), lay.segs.size() * 8, 0},
                   {c.data(), c.size() * 8, 0},               {lay.hot32.data(), lay.hot32.size() * 4, 0},
                   {lay.coop_trips.data(), lay.coop_trips.size() * 8, 0},
                   {lay.xhdr.data(), lay.xhdr.size() * 8, 0}, {lay.xrec.data(), lay.xrec.size() * 8, 0},
                    {lay.xpl.data(), lay.xpl.size() * 8, 0}, {lay.xpl32.data(), lay.xpl32.size() * 4, 0},
                    {lay.xwb.data(), lay.xwb.size() * 4, 0}, {lay.xwb_all.data(), lay.xwb_all.size() * 4, 0}};
  size_t total = 0;
  for (Part& p : parts) {
    p.off = total;
    total += (p.bytes + 255) / 256 * 256 + 256;  // every array keeps a little slack behind it
  }
  std::vector<unsigned char> host(total, 0);
  for (const Part& p : parts)
    if (p.bytes > 0) std::memcpy(host.data() + p.off, p.src, p.bytes);
  hipError_t e = blob.ensure(total);
  if (e == hipSuccess) e = hipMemcpy(blob.ptr, host.data(), total, hipMemcpyHostToDevice);
  const char* b = (const char*)blob.ptr;
  stat = (const double*)(b + parts[0].off);
  mov = (const double*)(b + parts[1].off);
  movy = (const double*)(b + parts[2].off);
  segs = (const double*)(b + parts[3].off);
  cold = (const double*)(b + parts[4].off);
  hot32 = (const float*)(b + parts[5].off);
  coop_trips = (const double*)(b + parts[6].off);
  xhdr = (const double*)(b + parts[7].off);
  xrec = (const double*)(b + parts[8].off);
  xpl = (const double*)(b + parts[9].off);
  xpl32 = (const float*)(b + parts[10].off);
  xwb = (const float*)(b + parts[11].off);
  xwb_all = (const float*)(b + parts[12].off);
  n_segs = lay.n_segs;
  n_sorted = (int)lay.n_sorted;
  any_reach = false;  // bit 2 of a header's gate word (tor_scene.cpp)
  for (int s = 0; s < lay.n_segs; ++s) {
    int32_t ints[8];
    std::memcpy(ints, &lay.xhdr[16 * (size_t)s], sizeof(ints));
    any_reach = any_reach || (ints[7] & 4) != 0;
  }
  n_xrec = (int)lay.xrec.size();
  has_f32 = false;
  for (int s = 0; s < lay.n_segs; ++s) has_f32 = has_f32 || lay.segs[8 * (size_t)s] >= 5.0;
  return e;
}

static bool parse_device_list(const char* e, TorOptions& o) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return false;
  o.device_count = 0;
  if (std::strcmp(e, "all") == 0) {
    for (int d = 0; d < count && d < TOR_MAX_DEVICES; ++d) o.devices[o.device_count++] = d;
    return true;
  }
  const char* p = e;
  while (*p) {
    char* endp = nullptr;
    const long v = std::strtol(p, &endp, 10);
    if (endp == p || v < 0 || v >= count || o.device_count >= TOR_MAX_DEVICES) return false;
    o.devices[o.device_count++] = (int32_t)v;
    p = endp;
    if (*p == ',') ++p;
    else if (*p) return false;
  }
  return o.device_count > 0;
}

// (why the last valid_options() call said no; the callers put it into tor_last_error)
thread_local std::string g_options_why;
const std::string& options_why() { return g_options_why; }

bool valid_options(const TorOptions* opt, TorOptions& o, bool for_drop_in) {
  g_options_why.clear();
  auto no = [](const char* why) { g_options_why = why; return false; };
  o = TorOptions{};
  o.struct_size = sizeof(TorOptions);
  o.seeding = TOR_SEED_PIXEL;
  o.arith = TOR_ARITH_STRICT;
  o.device = -1;
  o.shard_index = 0;
  o.shard_count = 1;
  o.row_tile = 1;
  o.gather = TOR_GATHER_AUTO;
  constexpr uint32_t kV1Size = 32;  // round-1 layout: everything up to and including `accel`
  if (opt) {
    if (opt->struct_size == sizeof(TorOptions)) o = *opt;
    else if (opt->struct_size == kV1Size) std::memcpy(&o, opt, kV1Size);
    else return no("struct_size is neither sizeof(TorOptions) nor the 32-byte round-1 layout");
    o.struct_size = sizeof(TorOptions);
  } else if (for_drop_in) {
    // tor_render() has the reference's signature and no options: a host that cannot pass TorOptions (the Nim
    // shim of INTEGRATION.md) steers the library through the environment.  None of these changes a pixel.
    o.accel = TOR_ACCEL_BLOCKS | TOR_ACCEL_F32;  // exact accelerations on by default for the drop-in
    // (a malformed value is an error, not a silent fall-back to one GPU / the default: ADVICE r2)
    if (const char* e = tor::knob("TOR_DEFAULT_ACCEL")) {
      char* endp = nullptr;
      const long v = std::strtol(e, &endp, 10);
      if (endp != e && *endp == 0 && v >= 0 && v <= (TOR_ACCEL_BLOCKS | TOR_ACCEL_F32)) o.accel = (int32_t)v;
      else return no("TOR_DEFAULT_ACCEL must be 0, 1, 2 or 3");
    }
    // TOR_DEFAULT_SEEDING = pixel | sample: which random streams the drop-in uses.  `pixel` (default) is the reference's
    // render.nim:59-67 -- one stream per pixel, the spp samples in sequence.  `sample` is the counter-based stream of
    // BASELINE.json's north_star, seed(row, col, sample): render.nim:59-60 re-seeds per pixel "to be able to parallelize the
    // outer loops"; this is the same idea one level down, and it is what lets 8 GPUs share a 1080p frame.  It is
    // the one knob of this list that changes pixels (a different, equally valid sample set; oracle mode SAMPLE / QUANTIZED).
    if (const char* e = tor::knob("TOR_DEFAULT_SEEDING")) {
      if (!std::strcmp(e, "sample")) o.seeding = TOR_SEED_SAMPLE;
      else if (!std::strcmp(e, "pixel")) o.seeding = TOR_SEED_PIXEL;
      else return no("TOR_DEFAULT_SEEDING must be pixel or sample");
    }
    if (const char* e = tor::knob("TOR_DEVICES")) {
      TorOptions t = o;
      if (parse_device_list(e, t)) o = t;
      else return no("TOR_DEVICES must be \"all\" or a comma list of HIP device ordinals that exist (at most TOR_MAX_DEVICES)");
    }
    if (const char* e = tor::knob("TOR_GATHER")) {
      if (!std::strcmp(e, "rccl")) o.gather = TOR_GATHER_RCCL;
      else if (!std::strcmp(e, "peer")) o.gather = TOR_GATHER_PEER;
      else if (!std::strcmp(e, "host")) o.gather = TOR_GATHER_HOST;
      else if (!std::strcmp(e, "auto")) o.gather = TOR_GATHER_AUTO;
      else return no("TOR_GATHER must be auto, rccl, peer or host");
    }
  }
  if (o.seeding != TOR_SEED_PIXEL && o.seeding != TOR_SEED_SAMPLE) return no("seeding must be TOR_SEED_PIXEL or TOR_SEED_SAMPLE");
  if (o.arith == TOR_ARITH_FUSED)
    return no("TOR_ARITH_FUSED was removed in round 5: it was not the reference's rounding (README.md:82) and TOR_ARITH_STRICT behind the conservative "
              "FMA screen is faster -- pass TOR_ARITH_STRICT (0)");
  if (o.arith != TOR_ARITH_STRICT) return no("arith must be TOR_ARITH_STRICT");
  if (o.accel < 0 || o.accel > (TOR_ACCEL_BLOCKS | TOR_ACCEL_F32)) return no("accel holds unknown TOR_ACCEL_* bits");
  if (o.shard_count < 1) o.shard_count = 1;  // (0 in a zero-initialised struct: whole image, one row per tile)
  if (o.row_tile == 0) o.row_tile = 1;
  if (o.row_tile < 0) return no("row_tile must be >= 1");
  if (o.shard_index < 0 || o.shard_index >= o.shard_count) return no("shard_index must lie in [0, shard_count)");
  if (o.device_count < 0 || o.device_count > TOR_MAX_DEVICES) return no("device_count must lie in [0, TOR_MAX_DEVICES]");
  if (o.gather < TOR_GATHER_AUTO || o.gather > TOR_GATHER_HOST) return no("gather must be a TOR_GATHER_* value");
  if (o.pixel_kernel < TOR_PIXEL_KERNEL_AUTO || o.pixel_kernel > TOR_PIXEL_KERNEL_WAVE) return no("pixel_kernel must be a TOR_PIXEL_KERNEL_* value");
  if (o.device_count > 1) {
    // the device list IS the sharding and the placement: shard_index / shard_count / device stay at their defaults (tor_render.h)
    if (o.shard_count != 1 || o.shard_index != 0) return no("with a device list, shard_index / shard_count must be left at 0 / 1: entry k renders shard k");
    // (`device` is ignored with a device list -- a zero-initialised TorOptions says 0 there, as it says 0 for shard_count and
    // row_tile, which are tolerated too; only a value that names a device OUTSIDE the list is a contradiction: ADVICE r3)
    if (o.device > 0) {
      bool listed = false;
      for (int k = 0; k < o.device_count; ++k) listed = listed || o.devices[k] == o.device;
      if (!listed) return no("with a device list, `device` must be -1, 0 or one of the listed ordinals (it is ignored)");
    }
    o.device = -1;
    for (int k = 0; k < o.device_count; ++k)
      if (o.devices[k] < 0) return no("negative ordinal in the device list");
  } else if (o.device_count == 1) {
    if (o.devices[0] < 0) return no("negative ordinal in the device list");
    o.device = o.devices[0];
  }
  return true;
}

// ---- lazily built device layouts ---------------------------------------------------------------
int ensure_layouts(TorContext* ctx, int accel) {
  const TorHittableVariant* objs = (const TorHittableVariant*)ctx->scene_bytes.data();
  const int64_t n = ctx->n_objects;
  const bool want_f32 = (accel & TOR_ACCEL_F32) != 0;
  const bool want_blocks = (accel & TOR_ACCEL_BLOCKS) != 0;
  if (want_f32 && !ctx->f32_built) {
    ctx->f32 = f32_options_for(objs, n);
    ctx->f32_built = true;
  }
  auto build_flat = [&](int v) -> int {
    if (ctx->flat_built[v]) return TOR_OK;
    std::vector<int64_t> ids((size_t)n);
    for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = i;
    HostLayout lay;
    std::string err;
    if (!build_layout(objs, ids, lay, err, v == 1 ? &ctx->f32 : nullptr)) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_upload: " + err);
    if (n == 0) lay.n_segs = 0;
    HIP_TRY(ctx->flat[v].put(lay));
    ctx->flat_built[v] = true;
    ctx->n_layouts_built += 1;
    return TOR_OK;
  };
  auto build_blocks = [&](int v) -> int {
    if (ctx->accel_built[v]) return TOR_OK;
    build_accel(objs, n, ctx->accel[v], v == 1 ? &ctx->f32 : nullptr);
    if (!ctx->accel[v].available) {
      ctx->accel_built[v] = true;  // (built: this scene has no culling layout)
      return TOR_OK;
    }
    // the layout counts as built only once every upload below has succeeded: a failed HIP call leaves it unbuilt (the
    // next launch tries again) instead of marked-built with null or stale device pointers
    struct Rollback {
      TorContext* c; int v; bool ok = false;
      ~Rollback() { if (!ok) { c->d_accel[v].release(); c->accel[v] = tor::HostAccel{}; } }
    } rollback{ctx, v};
    auto put = [](DeviceBuffer& b, const void* src, size_t bytes) -> hipError_t {
      hipError_t e = b.ensure(bytes > 0 ? bytes : 8);
      if (e == hipSuccess && bytes > 0) e = hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice);
      return e;
    };
    HIP_TRY(ctx->d_accel[v].always.put(ctx->accel[v].always, &ctx->accel[v].cold));
    HIP_TRY(put(ctx->d_accel[v].hot, ctx->accel[v].hot.data(), ctx->accel[v].hot.size() * 8));
    HIP_TRY(put(ctx->d_accel[v].grp, ctx->accel[v].groups.data(), ctx->accel[v].groups.size() * 8));
    if (ctx->accel[v].sp32) HIP_TRY(put(ctx->d_accel[v].hot32, ctx->accel[v].hot32.data(), ctx->accel[v].hot32.size() * 4));
    const size_t n_bnd_p = (ctx->accel[v].n_blocks + kPad - 1) / kPad * kPad;
    const size_t n_super_p = (n_bnd_p / kPad + kPad - 1) / kPad * kPad;
    // per slot: the float64 boxes, then the same records as float32 (8 floats each)
    const size_t slot_bytes = (8 * (n_bnd_p + 1 + n_super_p + 1)) * (8 + 4);
    if (slot_bytes * TorContext::kRing > ctx->bnd_ring.bytes) {
      // growing the ring frees the old one: no launch may still be reading it
      if (ctx->bnd_ring.ptr) HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(ctx->bnd_ring.ensure(slot_bytes * TorContext::kRing));
    }
    if (slot_bytes > ctx->bnd_slot_bytes) ctx->bnd_slot_bytes = slot_bytes;
    rollback.ok = true;
    ctx->accel_built[v] = true;
    ctx->n_layouts_built += 1;
    return TOR_OK;
  };
  int v32 = want_f32 ? 1 : 0;
  if (want_blocks) {
    int rc = build_blocks(v32);
    if (rc != TOR_OK) return rc;
    // the float32 kernel variant needs float32 block records; otherwise the launch stays on the float64 layouts
    if (v32 && ctx->accel[1].available && !ctx->accel[1].sp32) {
      v32 = 0;
      rc = build_blocks(0);
      if (rc != TOR_OK) return rc;
    }
    if (ctx->accel[v32].available) return TOR_OK;  // the launch uses the always-layout of the accel variant
  }
  return build_flat(v32);
}

int last_render_allows(TorContext* ctx, const void* stream, const char* who, const char* sentence) {
  if (ctx->launches > 0 && ctx->last_stream_valid && ctx->last_stream != stream) {
    const hipError_t q = hipEventQuery(ctx->ev_stop[ctx->last_slot]);
    if (q == hipErrorNotReady) return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + sentence);
    if (q != hipSuccess) return fail_hip(q, "hipEventQuery");
  }
  return TOR_OK;
}

}  // namespace tor

using tor::DeviceBuffer;
using tor::fail;
using tor::fail_hip;
using tor::valid_options;

extern "C" {

const char* tor_last_error(void) { return g_last_error.c_str(); }

const char* tor_version(void) { return "tor_mi355x 0.6 (gfx950)"; }

int32_t tor_knob_count(void) { return tor::kKnobCount; }

int tor_knob_info(int32_t i, const char** name, const char** dflt, const char** range, const char** when, const char** what) {
  if (i < 0 || i >= tor::kKnobCount) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_knob_info: index out of range");
  const tor::Knob& k = tor::kKnobs[i];
  if (name) *name = k.name;
  if (dflt) *dflt = k.dflt;
  if (range) *range = k.range;
  if (when) *when = k.when;
  if (what) *what = k.what;
  return TOR_OK;
}

int tor_last_render_timing(double out[5]) {
  if (!out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_render_timing: out is NULL");
  for (int k = 0; k < 5; ++k) out[k] = g_last_timing[k];
  return TOR_OK;
}

int tor_context_create(int32_t device, TorContext** out) {
  if (!out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_context_create: out is NULL");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(TOR_ERR_NO_DEVICE,
                std::string("no HIP device available (") + hipGetErrorString(e) +
                    "); libtor_mi355x has no CPU fallback");
  if (device < 0) HIP_TRY(hipGetDevice(&device));
  if (device >= count) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_context_create: device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  TorContext* ctx = new (std::nothrow) TorContext();
  if (!ctx) return fail(TOR_ERR_OUT_OF_MEMORY, "tor_context_create: host allocation failed");
  ctx->device = device;
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) {
    delete ctx;
    return fail_hip(e, "hipGetDeviceProperties");
  }
  ctx->num_cus = prop.multiProcessorCount;
  if (const char* w = tor::knob("TOR_WAVES_PER_SIMD")) ctx->waves_override = std::atoi(w);
  if (const char* l = tor::knob("TOR_LPT_MIN_SPP")) ctx->lpt_min_spp = std::atoi(l);
  if (const char* c = tor::knob("TOR_COOP_MAX_PIXELS")) ctx->coop_max_pixels = std::atoll(c);
  if (const char* c = tor::knob("TOR_HOT_FRAC")) ctx->hot_frac = (float)std::atof(c);
  if (const char* c = tor::knob("TOR_PRIO_SHIFT")) ctx->prio_shift = std::atoi(c);
  if (const char* c = tor::knob("TOR_MIGRATE")) ctx->mig_mode = std::atoi(c);
  if (const char* c = tor::knob("TOR_SRV_FRAC")) ctx->srv_frac = (float)std::atof(c);
  if (const char* c = tor::knob("TOR_SRV_PATIENCE_US")) ctx->srv_patience_us = std::atoi(c);
  if (const char* c = tor::knob("TOR_SRV_MIN_FRAC")) ctx->srv_min_frac = (float)std::atof(c);
  if (const char* c = tor::knob("TOR_PUSH_THETA")) ctx->push_theta = (float)std::atof(c);
  if (const char* c = tor::knob("TOR_FLOOR_THETA")) ctx->floor_theta = (float)std::atof(c);
  if (const char* c = tor::knob("TOR_CHAIN_THETA")) ctx->chain_theta = (float)std::atof(c);
  if (const char* c = tor::knob("TOR_TAIL_LANES")) ctx->mig_tail_lanes = std::atoi(c);
  if (const char* c = tor::knob("TOR_SCREEN")) ctx->screen = std::atoi(c) != 0;
  if (const char* c = tor::knob("TOR_PLANE")) ctx->plane_screen = std::atoi(c);  // 0 off, 1 gated (default), 2 on every segment that carries the table, 3 as 1 but the reach pass culls nothing
  if (const char* c = tor::knob("TOR_TAIL_REST")) ctx->mig_tail_rest = std::atoi(c);
  if (const char* c = tor::knob("TOR_MIG_FLAGS")) ctx->mig_flags = (unsigned)std::strtoul(c, nullptr, 0);
  if (const char* b = tor::knob("TOR_BLOCKS_PER_CU"))
    for (int s = 0; s < 2; ++s) ctx->max_blocks_per_cu[s][0] = ctx->max_blocks_per_cu[s][1] = std::atoi(b);
  e = ctx->counters.ensure(TorContext::kRing * TorContext::kSlotWords * sizeof(unsigned long long));
  if (e == hipSuccess) e = ctx->cam_ring.ensure(TorContext::kRing * sizeof(TorCamera));
  for (int i = 0; i < TorContext::kRing && e == hipSuccess; ++i) {
    e = hipEventCreate(&ctx->ev_start[i]);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev_stop[i]);
  }
  if (e != hipSuccess) {
    tor_context_destroy(ctx);
    return fail_hip(e, "tor_context_create");
  }
  *out = ctx;
  return TOR_OK;
}

int tor_context_destroy(TorContext* ctx) {
  if (!ctx) return TOR_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  (void)tor_comm_destroy(ctx);
  tor::patches_context_destroyed(ctx);  // the patch table (tor_patches.hip) lives outside the context
  for (int v = 0; v < 2; ++v) {
    ctx->flat[v].release();
    ctx->d_accel[v].release();
  }
  ctx->bnd_ring.release();
  ctx->counters.release();
  ctx->cam_ring.release();
  ctx->wave_log.release();
  for (int i = 0; i < TorContext::kRing; ++i) {
    ctx->tile_order[i].release();
  }
  ctx->probe_buf.release();
  ctx->mig_rec.release();
  ctx->mig_flag.release();
  ctx->scratch.release();
  ctx->slice.release();
  ctx->gather.release();
  ctx->frame.release();
  ctx->noise.release();
  ctx->adapt.release();
  ctx->staging.release();
  for (hipEvent_t ev : ctx->chunk_events) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : ctx->ev_call) if (ev) (void)hipEventDestroy(ev);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  for (int i = 0; i < TorContext::kRing; ++i) {
    if (ctx->ev_fork[i]) (void)hipEventDestroy(ctx->ev_fork[i]);
    if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
  }
  for (int i = 0; i < TorContext::kRing; ++i) {
    if (ctx->ev_start[i]) (void)hipEventDestroy(ctx->ev_start[i]);
    if (ctx->ev_stop[i]) (void)hipEventDestroy(ctx->ev_stop[i]);
  }
  delete ctx;
  return TOR_OK;
}

int tor_context_set_stats(TorContext* ctx, int32_t enable) {
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_context_set_stats: ctx is NULL");
  ctx->collect_stats = enable != 0;
  return TOR_OK;
}

int tor_debug_last_variant(TorContext* ctx, int32_t out[5]) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_last_variant: NULL argument");
  for (int k = 0; k < 5; ++k) out[k] = ctx->last_variant[k];
  return TOR_OK;
}

int tor_debug_last_split_tiles(TorContext* ctx, int64_t* tiles_out) {
  if (!ctx || !tiles_out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_last_split_tiles: NULL argument");
  *tiles_out = 0;
  if (!ctx->last_split) return TOR_OK;  // the last launch ran one kernel for the whole frame
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
  unsigned long long w = 0;  // slot word 6: the split point tile_order_kernel chose (tiles of the cost order the wave kernel took)
  HIP_TRY(hipMemcpy(&w, (unsigned long long*)ctx->counters.ptr + (size_t)ctx->last_slot * TorContext::kSlotWords + 6, sizeof w, hipMemcpyDeviceToHost));
  *tiles_out = (int64_t)w;
  return TOR_OK;
}

int tor_context_scene_counters(TorContext* ctx, int64_t out[3]) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_context_scene_counters: NULL argument");
  out[0] = ctx->n_uploads;
  out[1] = ctx->n_cache_hits;
  out[2] = ctx->n_layouts_built;
  return TOR_OK;
}

// AoS -> SoA.  Objects are partitioned into one static segment and one segment per distinct
// (time0, time1) pair; closest-hit is order independent (hittables_lists.nim:48-55; ties are
// broken by the original index carried in the cold record), so the reordering is exact.
// The context keeps a byte copy of the list: an identical list is a cache hit, and the device layouts are
// built from the copy when a launch first needs them (ensure_layouts).
int tor_scene_upload(TorContext* ctx, TorHittableList world) {
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_upload: ctx is NULL");
  if (world.len < 0 || (world.len > 0 && !world.objects))
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_upload: bad HittableList");
  if (world.len > (int64_t)1 << 24) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_upload: too many objects");
  ctx->n_uploads += 1;
  const size_t bytes = (size_t)world.len * sizeof(TorHittableVariant);
  if (ctx->scene_ready && ctx->n_objects == world.len && ctx->scene_bytes.size() == bytes &&
      (bytes == 0 || std::memcmp(ctx->scene_bytes.data(), world.objects, bytes) == 0)) {
    ctx->n_cache_hits += 1;
    return TOR_OK;
  }
  for (int64_t i = 0; i < world.len; ++i) {
    const TorHittableVariant& h = world.objects[i];
    if (h.kind != TOR_SPHERE && h.kind != TOR_MOVING_SPHERE) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_upload: unknown HittableVariant kind");
    const uint8_t mk = h.kind == TOR_SPHERE ? h.u.sphere.material.kind : h.u.moving_sphere.material.kind;
    if (mk > TOR_DIELECTRIC) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_upload: unknown Material kind");
  }
  HIP_TRY(hipSetDevice(ctx->device));
  // the scene buffers are about to be overwritten / reallocated: no launch may still be reading them
  if (ctx->scene_ready) HIP_TRY(hipDeviceSynchronize());
  ctx->scene_ready = false;
  ctx->scene_bytes.assign((const unsigned char*)world.objects, (const unsigned char*)world.objects + bytes);
  ctx->n_objects = world.len;
  for (int v = 0; v < 2; ++v) ctx->flat_built[v] = ctx->accel_built[v] = false;
  ctx->f32_built = false;
  ctx->hitq.groups.clear();  // a new scene: every object in every group (tor_scene_groups)
  ctx->hitq.groups_gen += 1;
  ctx->hitq.n_lights = 0;    // ... and no light table (tor_scene_lights)
  ctx->hitq.n_media = 0;     // ... and no media table (tor_scene_media)
  ctx->hitq.drop_grids();    // ... so no density grids (tor_scene_media_grid); the device is idle (above)
  ctx->hitq.n_textures = 0;  // ... and no texture table (tor_scene_textures)
  tor::patches_scene_replaced(ctx);  // ... and no patch table (tor_scene_patches)
  ctx->scene_ready = true;
  return TOR_OK;
}

int32_t tor_shard_rows(int32_t nrows, int32_t row_tile, int32_t shard_index, int32_t shard_count,
                       int32_t* rows_out) {
  if (nrows <= 0) return 0;
  if (shard_count < 1) shard_count = 1;
  if (row_tile < 1) row_tile = 1;
  if (shard_index < 0 || shard_index >= shard_count) return 0;
  int32_t n = 0;
  for (int32_t r = 0; r < nrows; ++r)
    if ((r / row_tile) % shard_count == shard_index) {
      if (rows_out) rows_out[n] = r;
      ++n;
    }
  return n;
}

// tor::launch_integrate, recording the kernel variant it launched (tor_debug_last_variant)
static hipError_t launch_integrate_recorded(TorContext* ctx, const tor::KParams& p, int seeding, int arith, int waves_per_simd, int blocks,
                                            hipStream_t stream) {
  const hipError_t e = tor::launch_integrate(p, seeding, arith, waves_per_simd, blocks, stream);
  if (e == hipSuccess) tor::integrate_variant_key(p, seeding, arith, waves_per_simd, ctx->last_variant);
  return e;
}

#define TOR_TRY(expr) do { const int rc__ = (expr); if (rc__ != TOR_OK) return rc__; } while (0)

// ---- one render launch, phase by phase ("The host side of a launch") ---------------------------------------------
// One call of a render entry.  The entry fills the first ten members; decode_call derives the rest down to n_tiles,
// claim_ring_slot the ring slot's part.
struct RenderCall {
  const char* who;  // the entry's name, for its refusals
  const TorCamera* cam;
  int32_t nrows, ncols, spp;
  float gamma_correction;
  int64_t max_depth;
  double* d_pixels;
  hipStream_t stream;
  // not null: one pass of tor_render_accumulate_device -- samples [acc->first_sample, + spp) added to the raw quantised sums in
  // d_pixels (and, with acc->moments, their second moments), no clearing, no finalize
  const tor::AccumLaunch* acc;
  bool listed;  // ... over a pixel list
  bool resume;  // tor_render_resume_device: a pass on the pixel streams from / into caller-owned state
  bool rlist;   // tor_render_resume_list_device: ... over the listed pixels only
  TorOptions o;  // validated, defaults applied
  int kseed;     // the kernel variant's SEEDING
  int32_t local_rows;
  long long npix, n_values;
  long long work_pix;  // pixels this launch traces
  long long n_tiles;
  int slot;
  unsigned long long* slot_counters;
};

static int refuse(const char* who, const std::string& what) { return fail(TOR_ERR_INVALID_ARGUMENT, who + what); }

// Every refusal of a render entry that does not depend on the context's launches in flight, then what the phases below derive from
// the arguments.
static int decode_call(TorContext* ctx, const TorOptions* opt, RenderCall& c) {
  const char* who = c.who;
  const tor::AccumLaunch* acc = c.acc;
  c.listed = acc && acc->list;
  c.resume = acc && acc->rng;
  c.rlist = c.resume && c.listed;
  if (!ctx || !c.cam || !c.d_pixels) return refuse(who, ": NULL argument");
  if (!ctx->scene_ready) return refuse(who, ": no scene uploaded");
  // The reference divides by (ncols-1) and (nrows-1) (render.nim:64-65) and by spp
  // (canvas.nim:49); degenerate sizes are rejected instead of producing inf/NaN canvases.
  if (c.nrows < 2 || c.ncols < 2 || c.spp < 1) return refuse(who, ": need nrows >= 2, ncols >= 2, samples_per_pixel >= 1");
  if (c.max_depth > 0x7fffffff) c.max_depth = 0x7fffffff;
  TorOptions& o = c.o;
  if (!valid_options(opt, o, false)) return refuse(who, ": bad TorOptions: " + tor::options_why());
  if (o.device_count > 1) return refuse(who, ": one context renders on one device (device lists: tor_render_opt)");
  if (c.resume && o.seeding != TOR_SEED_PIXEL)
    return refuse(who, ": needs TOR_SEED_PIXEL -- it continues the reference's per-pixel streams (render.nim:59-67) from per-pixel "
                       "generator states; passes of TOR_SEED_SAMPLE streams are tor_render_accumulate_device's");
  if (acc && !c.resume && o.seeding != TOR_SEED_SAMPLE)
    return refuse(who, ": needs TOR_SEED_SAMPLE -- a TOR_SEED_PIXEL pixel is one sequential chain of "
                       "samples on one generator (render.nim:59-67); resuming it would need per-pixel RNG state");
  // the kernel variant: SEED_SAMPLE with second moments (3) only for progressive launches that asked for them, over a pixel list (4)
  // for adaptive ones; resume passes on the pixel streams run 5, or 6 with second moments, or 7 over a pixel list (always with moments)
  c.kseed = c.rlist ? 7 : c.resume ? (acc->moments ? 6 : 5) : (c.listed ? 4 : ((acc && acc->moments) ? 3 : o.seeding));
  HIP_TRY(hipSetDevice(ctx->device));

  c.local_rows = tor_shard_rows(c.nrows, o.row_tile, o.shard_index, o.shard_count, nullptr);
  c.npix = (long long)c.local_rows * c.ncols;
  c.n_values = c.npix * 3;
  c.work_pix = c.listed ? (long long)acc->n_list : c.npix;
  c.n_tiles = (c.npix + tor::kTilePixelsHost - 1) / tor::kTilePixelsHost;
  ctx->timing_valid = false;
  ctx->last_samples = 0;
  ctx->last_migrate = false;
  ctx->last_split = false;
  return TOR_OK;
}

// A ring slot (events, camera, bounds, counters, tile schedule) is reused every kRing launches: its previous launch must be
// done.  Then the stream rule, and the slot's counters start at zero.
static int claim_ring_slot(TorContext* ctx, RenderCall& c) {
  c.slot = (int)(ctx->launches % TorContext::kRing);
  if (ctx->launches >= TorContext::kRing) HIP_TRY(hipEventSynchronize(ctx->ev_stop[c.slot]));
  // One stream per context while launches are in flight (tor_render.h): the per-launch state (work counters, tile
  // schedule, probe buffer, hand-off queue) is ordered by the stream.  A launch on ANOTHER stream is accepted only once
  // the previous launch of this context has finished.
  TOR_TRY(tor::last_render_allows(ctx, c.stream, c.who, ": the previous launch of this context is still running on a different stream -- "
                                                        "launches of one context that may overlap must use ONE stream (or use one context per stream)"));
  ctx->last_stream = c.stream;
  ctx->last_stream_valid = true;
  c.slot_counters = (unsigned long long*)ctx->counters.ptr + (size_t)c.slot * TorContext::kSlotWords;
  HIP_TRY(hipMemsetAsync(c.slot_counters, 0, TorContext::kSlotWords * sizeof(unsigned long long), c.stream));
  return TOR_OK;
}

// Split fraction (measured: tools/split_sweep.py, with the tiles ordered by their longest chain): the wave-per-pixel
// kernel saturates at ~285 Msamples/s, the lane kernel (with both exact accelerations) is bound by its longest chains;
// the best share of the probed work for the wave kernel is ~20 000 / pixels, capped at 0.2 (C1 at 100 spp: 16-17 ms for
// anything in 0.15-0.35, at 1000 spp 130 ms at 0.15 against 163 ms at 0.45) and floored at 0.02 (only the glass-sphere
// tiles); from ~1.2 M pixels on the lane kernel keeps everything.
static float split_fraction(const TorContext* ctx, const RenderCall& c) {
  if (ctx->split_frac >= 0.0f) return ctx->split_frac;
  if (c.o.accel != (TOR_ACCEL_BLOCKS | TOR_ACCEL_F32) || c.npix > 1200000) return 0.0f;
  const float f = 20000.0f / (float)c.npix;
  return f > 0.2f ? 0.2f : (f < 0.02f ? 0.02f : f);
}

// the scene part of q that names the device arrays of one layout
static void use_layout(tor::KParams& q, const tor::DeviceLayout& L, const TorContext* ctx, const RenderCall& c, int accel) {
  q.stat = L.stat;
  q.mov = L.mov;
  q.movy = L.movy;
  q.segs = L.segs;
  q.cold = L.cold;
  q.hot32 = L.has_f32 ? L.hot32 : nullptr;
  q.xhdr = L.xhdr;
  q.xrec = L.xrec;
  q.xpl = ctx->plane_screen != 0 ? L.xpl : nullptr;
  q.xpl32 = ctx->plane_screen != 0 ? L.xpl32 : nullptr;
#if TOR_REACH
  // (null: no segment of the layout asks for the reach pass -- the launch takes the kernels without it; TOR_PLANE=2 runs it everywhere)
  q.xwb = (ctx->plane_screen != 0 && (L.any_reach || ctx->plane_screen == 2)) ? (ctx->plane_screen == 3 ? L.xwb_all : L.xwb) : nullptr;
#endif
  q.plane_gate2 = ctx->plane_screen == 2 ? 0.0 : 4.0 * tor::kPlaneGate * tor::kPlaneGate;
  // stage two of the plane-screened segments reads its records per lane: from LDS when the table fits beside the per-wave
  // queues -- and, with sample streams, the camera-ray reservoirs -- at this launch's workgroups per CU (random_scene: 15.9 KB + 18.7 KB
  // + 18.8 KB of 53.3 KB) and inside the 64 KB a launch may
  // ask for without an opt-in, else through the vector cache.  Only the ARITH 2 variants stage it (brute-force layouts
  // behind the screen: tor_kernels.hip dynamic_lds), so the room is only counted there.
  q.xrec_lds_doubles = 0;
  if (q.xpl != nullptr && ctx->screen && accel == 0) {
    const size_t wgs = (size_t)std::max(1, ctx->max_blocks_per_cu[c.o.seeding][0]);
    const size_t need = (size_t)L.n_xrec * 8 + (size_t)tor::integrate_fixed_lds_bytes(0, 0, c.kseed);
    if (need <= (size_t)(160 * 1024) / wgs - 1024 && need <= (size_t)64 * 1024) q.xrec_lds_doubles = L.n_xrec;
  }
  q.n_segs = L.n_segs;
}

static bool fits_lds(size_t bytes, int wgs, size_t fixed) {
  return bytes + fixed <= (size_t)(160 * 1024) / (size_t)wgs - 1024;
}

// LDS staging of the block records next to the per-wave queues (10 KB per workgroup in these variants, 160 KB per CU): the
// float32 pair records (TOR_ACCEL_F32; survivors are re-tested from the cold records -- staging the float64
// records as well measured +2 % at best) or the float64 compact records.  It must fit at this mode's
// workgroups/CU, else global loads (through L2).
// `full` is that count; returns the workgroups per CU the launch may run with what was staged (0: nothing staged).
static int stage_records_in_lds(tor::KParams& q, const tor::HostAccel& hacc, size_t bnd32_stage_floats, int full, int kseed) {
  const size_t hot_bytes = q.shot32 ? hacc.hot32.size() * 4 : hacc.hot.size() * 8;
  const size_t fixed = (size_t)tor::integrate_fixed_lds_bytes(1, q.shot32 != nullptr ? 1 : 0, kseed);
  // Workgroups per CU come first: on the 1601-object animation frames 3 workgroups/CU reading the records through L2
  // render 2339 Msamples/s, 2 workgroups/CU with the records in LDS 1914.  So the launch keeps its full workgroup count
  // and stages what fits beside it: the block boxes of a two-level scene first (6.6 KB there; every lane reads 8 of
  // them per super box it expands), then the block records if there is still room; only a launch whose mode runs at 2
  // workgroups/CU anyway gets the bigger LDS share.
  const bool stage_boxes = q.shot32 && bnd32_stage_floats > 0 && fits_lds(bnd32_stage_floats * 4, full, fixed);
  const size_t box_bytes = stage_boxes ? bnd32_stage_floats * 4 : 0;
  bool stage_hot = fits_lds(hot_bytes + box_bytes, full, fixed);
  int wg = (stage_hot || stage_boxes) ? full : 0;
  if (!q.shot32 && !stage_hot && full > 2 && fits_lds(hot_bytes, full - 1, fixed)) {
    // (the float64 compact records of TOR_ACCEL_BLOCKS alone are read by every lane for every block it enters: there
    // one workgroup fewer with the records in LDS wins, 1212 against 1140 Msamples/s on the same frames)
    stage_hot = true;
    wg = full - 1;
  }
  q.shot_lds_doubles = (stage_hot && !q.shot32) ? (int)hacc.hot.size() : 0;
  q.shot32_lds_floats = (stage_hot && q.shot32) ? (int)hacc.hot32.size() : 0;
  q.bnd32_lds_floats = stage_boxes ? (int)bnd32_stage_floats : 0;
  return wg;
}

// what configure_layout chose beside the scene part of the KParams
struct LayoutChoice {
  bool use_accel = false;  // the launch walks the culling layout
  int stage_wg = 0;        // > 0: compact records staged in LDS, at most this many workgroups per CU
  const tor::HostAccel* hacc = nullptr;
};

// Layout configuration of a launch: which device arrays the kernel walks for `accel`, the per-call block bounds (into bnd_host /
// bnd32_host) and the LDS staging decision.  Two launches of one call may use it: the frame's kernel with the caller's
// accel bits and -- SEED_PIXEL -- the cost probe, which always runs with both exact accelerations when the scene has
// them (it only COUNTS closest-hit queries per pixel; the count does not depend on how the hit is found).
static int configure_layout(TorContext* ctx, const RenderCall& c, int accel, tor::KParams& q, std::vector<double>& bnd_host,
                            std::vector<float>& bnd32_host, LayoutChoice& out) {
  TOR_TRY(tor::ensure_layouts(ctx, accel));
  // TOR_ACCEL_F32 layout variant; with TOR_ACCEL_BLOCKS it needs float32 block records (HostAccel::sp32),
  // otherwise the whole launch stays on the float64 layout
  int v32 = (accel & TOR_ACCEL_F32) ? 1 : 0;
  if (v32 && (accel & TOR_ACCEL_BLOCKS) && ctx->accel[1].available && !ctx->accel[1].sp32) v32 = 0;
  const bool blocks_avail = (accel & TOR_ACCEL_BLOCKS) && ctx->accel_built[v32] && ctx->accel[v32].available;
  if (!blocks_avail) use_layout(q, ctx->flat[v32], ctx, c, accel);
  for (int k = 0; k < 3; ++k) q.org[k] = ctx->f32.origin[k];
  q.bnd = nullptr;
  q.spatial_base = 0;
  q.shot = nullptr;
  q.sgrp = nullptr;
  q.shot_lds_doubles = 0;
  q.shot_stride = 8;
  const tor::HostAccel& hacc = ctx->accel[v32];
  out = LayoutChoice{false, 0, &hacc};
  if (blocks_avail) {
    // rays carry the camera's shutter times, or 0 after a metal / dielectric bounce (rays.nim:19)
    const double t_lo = std::fmin(0.0, std::fmin(c.cam->shutter_open, c.cam->shutter_close));
    const double t_hi = std::fmax(0.0, std::fmax(c.cam->shutter_open, c.cam->shutter_close));
    out.use_accel = tor::compute_block_bounds(hacc, t_lo, t_hi, bnd_host);
    if (!out.use_accel) {  // non-finite ray-time range: brute force over the flat layout
      TOR_TRY(tor::ensure_layouts(ctx, accel & ~TOR_ACCEL_BLOCKS));
      use_layout(q, ctx->flat[v32], ctx, c, accel);
    }
  }
  if (!out.use_accel) return TOR_OK;
  use_layout(q, ctx->d_accel[v32].always, ctx, c, accel);
  q.bnd = (const double*)((char*)ctx->bnd_ring.ptr + (size_t)c.slot * ctx->bnd_slot_bytes);  // filled by the caller (async copy)
  q.spatial_base = (int)hacc.spatial_base;
  q.n_super = (int)(tor::accel_boxes_padded(hacc) / tor::kPad);
  q.two_level = hacc.two_level ? 1 : 0;
  // (the float32 records carry their own guard, the `wild` ray of tor_filter32.hpp; only the float64 block loop reads these)
  q.box_reach2 = -1.0;
  q.box_amin = INFINITY;
  for (int k = 0; k < 3; ++k) q.box_org[k] = 0.0;
  if (!(v32 && hacc.sp32)) tor::block_reach(hacc, bnd_host, q.box_org, &q.box_reach2, &q.box_amin);
  q.shot = (const double*)ctx->d_accel[v32].hot.ptr;
  q.sgrp = (const double*)ctx->d_accel[v32].grp.ptr;
  q.shot_stride = hacc.hot_stride;
  q.shot32 = nullptr;
  size_t bnd32_stage_floats = 0;
  if (v32 && hacc.sp32) {
    q.shot32 = (const float*)ctx->d_accel[v32].hot32.ptr;
    q.shot32_stride = hacc.hot32_stride;
    q.shot32_block_stride = hacc.hot32_block_stride;
    q.sp_mc0max = hacc.sp_mc0max; q.sp_dcmax = hacc.sp_dcmax;
    q.sp_t0 = hacc.sp_t0; q.sp_dt = hacc.sp_dt;
    // float32 boxes for the slab tests; on two-level scenes the lanes read the block boxes themselves: stage them
    q.sp_bmax = tor::block_bounds_f32(bnd_host, ctx->f32.origin, bnd32_host, &q.sp_hmin);
    q.bnd32 = (const float*)((const char*)q.bnd + bnd_host.size() * 8);
    if (hacc.two_level) bnd32_stage_floats = 8 * tor::accel_boxes_padded(hacc);
  }
  out.stage_wg = stage_records_in_lds(q, hacc, bnd32_stage_floats, ctx->max_blocks_per_cu[c.o.seeding][accel != 0], c.kseed);
  return TOR_OK;
}

// Launch configuration of the frame's lane kernel, shared by the hand-off decision and the launch itself.
struct FrameConfig {
  tor::KParams p{};
  LayoutChoice lay;
  // launch shape: workgroups per CU for this mode (fewer when the LDS staging needs the room); the
  // kernel variant's register budget follows it
  int waves_per_simd = 0;
  long long resident_waves = 0;
};

static int configure_frame(TorContext* ctx, const RenderCall& c, FrameConfig& f) {
  TOR_TRY(configure_layout(ctx, c, c.o.accel, f.p, ctx->bnd_host[c.slot], ctx->bnd32_host[c.slot], f.lay));
  int cap = ctx->max_blocks_per_cu[c.o.seeding][c.o.accel != 0];
  if (cap < 1) cap = 4;
  if (f.lay.stage_wg > 0 && f.lay.stage_wg < cap) cap = f.lay.stage_wg;
  f.waves_per_simd = ctx->waves_override > 0 ? ctx->waves_override : ((cap >= 2 && cap <= 4) ? cap : 4);
  int bpc_eff = tor::integrate_blocks_per_cu(f.p, c.kseed, c.o.arith, f.waves_per_simd);
  if (bpc_eff > cap) bpc_eff = cap;
  f.resident_waves = (long long)ctx->num_cus * bpc_eff * (tor::kThreads / 64);
  return TOR_OK;
}

// Chain hand-off (DESIGN 4.7 (HISTORY 4.10)): the lane kernel pushes its long chains to server waves inside the same launch -- it
// replaces both the whole-frame wave kernel and split mode wherever the launch's kernel variant carries the servers
// (both exact accelerations, single-level culling layout with float32 records, <= 128 block boxes) and the probe runs.
// Decided in full -- handoff_candidate, then handoff_runs on the configured frame -- before split mode and the wave-per-pixel
// kernel are ruled out: a frame whose hand-off cannot run after all (non-finite shutter range -> no culling, a variant without
// servers, a tiny machine) keeps those two.
static bool handoff_candidate(const TorContext* ctx, const RenderCall& c) {
  return c.o.seeding == TOR_SEED_PIXEL && c.o.pixel_kernel == TOR_PIXEL_KERNEL_AUTO && ctx->mig_mode != 0 &&
         c.o.accel == (TOR_ACCEL_BLOCKS | TOR_ACCEL_F32) && ctx->lpt_min_spp > 0 && c.spp >= ctx->lpt_min_spp &&
         c.npix > tor::kTilePixelsHost && !ctx->collect_stats && ctx->n_objects > 0 &&
         !c.resume;  // (no hand-off for resume passes: a stalled launch would leave some pixels advanced in place and others not -- DESIGN 4.11)
}

static bool handoff_runs(const TorContext* ctx, const RenderCall& c, const FrameConfig& f) {
  const tor::HostAccel& ha = ctx->accel[1];
  return ctx->accel_built[1] && ha.available && ha.sp32 && !ha.two_level && tor::accel_boxes_padded(ha) <= 128 && f.lay.use_accel &&
         c.n_tiles > 1 && tor::integrate_variant_serves_chains(f.p, c.o.seeding) && f.resident_waves >= 8;
}

static bool split_applies(const TorContext* ctx, const RenderCall& c, float split_frac) {
  return c.o.pixel_kernel == TOR_PIXEL_KERNEL_AUTO && split_frac > 0.0f && ctx->lpt_min_spp > 0 && c.spp >= ctx->lpt_min_spp &&
         c.npix >= ctx->split_min_pixels && c.npix <= ctx->split_max_pixels && !ctx->collect_stats && ctx->n_objects > 0 &&
         !c.rlist;  // (a listed pass has no tile schedule to split: no probe, no order -- see probe_and_schedule)
}

// `elsewhere`: split mode or the hand-off takes the frame
static bool wave_kernel_wanted(const TorContext* ctx, const RenderCall& c, bool elsewhere) {
  // (a listed pass: the list's length stands in for the pixel count -- what decides is how many chains can run side by side -- against
  // three quarters of the threshold: measured at 1080p the two kernels cross at ~95 000 listed pixels, below the whole-frame rule's
  // 114 688, because a listed lane pass has no probe to pay for and no tile order to lose)
  const long long coop_max_listed = ctx->coop_max_pixels / 4 * 3;
  const bool want = c.o.pixel_kernel == TOR_PIXEL_KERNEL_WAVE ||
                    (c.o.pixel_kernel == TOR_PIXEL_KERNEL_AUTO && ctx->coop_max_pixels > 0 &&
                     (c.rlist ? c.work_pix <= coop_max_listed : c.npix <= ctx->coop_max_pixels) && !elsewhere);
  return c.o.seeding == TOR_SEED_PIXEL && !ctx->collect_stats && want && ctx->n_objects > 0;
}

// the call's own part of a render kernel's KParams, the lane kernel's and the wave-per-pixel kernel's alike
static void call_params(tor::KParams& q, const RenderCall& c) {
  q.nrows = c.nrows; q.ncols = c.ncols; q.spp = c.spp; q.max_depth = (int)c.max_depth;
  q.shard_index = c.o.shard_index; q.shard_count = c.o.shard_count; q.row_tile = c.o.row_tile;
  q.n_pixels = (unsigned)c.npix;
  q.work_counter = c.slot_counters;
  q.out = c.d_pixels;
  q.first_sample = c.acc ? c.acc->first_sample : 0;
  q.mom = c.acc ? c.acc->moments : nullptr;
  q.pixel_list = c.listed ? c.acc->list : nullptr;
  q.rstate = c.resume ? c.acc->rng : nullptr;
}

// the wave-per-pixel kernel's view of the float64 flat layout
static void coop_params(tor::KParams& q, const tor::DeviceLayout& L) {
  q.cold = L.cold;
  q.n_cold_slots = L.n_sorted;
  q.coop_slots = (L.n_sorted + 63) / 64 * 64;
  q.coop_trips = L.coop_trips;
}

// the camera travels in its own small device slot (one per in-flight launch)
static int upload_camera(TorContext* ctx, const RenderCall& c, const double*& cam_dev) {
  ctx->cam_host[c.slot] = *c.cam;
  cam_dev = (const double*)((char*)ctx->cam_ring.ptr + (size_t)c.slot * sizeof(TorCamera));
  HIP_TRY(hipMemcpyAsync((void*)cam_dev, &ctx->cam_host[c.slot], sizeof(TorCamera), hipMemcpyHostToDevice, c.stream));
  return TOR_OK;
}

// One timed launch of a call, between the slot's ev_start and ev_stop: the wave-per-pixel kernel (`wave`), the lane kernel
// (`lane`), or -- split mode, both -- the wave kernel on stream2 beside the lane kernel, joined before ev_stop.  `wave_blocks` is
// the wave kernel's grid when it runs alone.
static int launch_bracketed(TorContext* ctx, const RenderCall& c, const tor::KParams* wave, int wave_blocks, const tor::KParams* lane,
                            int waves_per_simd, int lane_blocks) {
  const int slot = c.slot;
  const bool split = wave && lane;
  if (split) {
    if (!ctx->stream2) HIP_TRY(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    if (!ctx->ev_fork[slot]) {
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork[slot], hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join[slot], hipEventDisableTiming));
    }
  }
  HIP_TRY(hipEventRecord(ctx->ev_start[slot], c.stream));
  if (split) {
    HIP_TRY(hipEventRecord(ctx->ev_fork[slot], c.stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork[slot], 0));
  }
  if (split) wave_blocks = ctx->num_cus * tor::coop_blocks_per_cu(*wave, c.o.arith);  // beside the lane kernel it takes what is resident
  if (wave) HIP_TRY(tor::launch_coop(*wave, c.o.arith, wave_blocks, split ? ctx->stream2 : c.stream));
  if (split) HIP_TRY(hipEventRecord(ctx->ev_join[slot], ctx->stream2));
  if (lane) HIP_TRY(launch_integrate_recorded(ctx, *lane, c.kseed, c.o.arith, waves_per_simd, lane_blocks, c.stream));
  if (split) HIP_TRY(hipStreamWaitEvent(c.stream, ctx->ev_join[slot], 0));
  HIP_TRY(hipEventRecord(ctx->ev_stop[slot], c.stream));
  ctx->launches += 1;
  ctx->last_slot = slot;
  ctx->last_split = split;
  ctx->timing_valid = true;
  ctx->last_samples = (int64_t)c.work_pix * c.spp;
  return TOR_OK;
}

// Small SEED_PIXEL frames: one wave per pixel (coop_pixel_kernel) -- the lane-per-pixel kernel would be bound by
// the latency of the longest pixel chain.  Same canvas bit for bit; needs only the float64 flat layout.
// `launched` stays false when the objects do not fit LDS: the lane kernel takes the frame.
// (work_pix: on the pixel streams a listed pass is a resume pass -- decode_call -- so it is the list's length exactly when rlist)
static int launch_wave_frame(TorContext* ctx, const RenderCall& c, bool& launched) {
  launched = false;
  TOR_TRY(tor::ensure_layouts(ctx, 0));
  tor::KParams wp{};
  coop_params(wp, ctx->flat[0]);
  const int bpc = tor::coop_blocks_per_cu(wp, c.o.arith);
  if (bpc <= 0) return TOR_OK;
  call_params(wp, c);
  if (c.rlist) wp.total_work = (unsigned long long)c.work_pix;  // work item k = list slot k
  TOR_TRY(upload_camera(ctx, c, wp.cam_dev));
  long long blocks = (c.work_pix + (tor::kThreads / 64) - 1) / (tor::kThreads / 64);
  const long long resident = (long long)ctx->num_cus * bpc;
  if (blocks > resident) blocks = resident;
  TOR_TRY(launch_bracketed(ctx, c, &wp, (int)blocks, nullptr, 0, 0));
  launched = true;
  return TOR_OK;
}

// The call's part of the lane kernel's KParams, its grid (`blocks`), and the uploads the launch reads: camera and block bounds.
static int prepare_lane_launch(TorContext* ctx, const RenderCall& c, FrameConfig& f, bool migrate, int& blocks) {
  tor::KParams& p = f.p;
  const TorOptions& o = c.o;
  call_params(p, c);
  p.inv_spp = 1.0 / (double)c.spp; p.inv_ncols = 1.0 / (double)c.ncols; p.inv_row_tile = 1.0 / (double)(o.row_tile > 0 ? o.row_tile : 1);
  p.stats = ctx->collect_stats ? c.slot_counters + 1 : nullptr;

  long long waves;
  p.order = nullptr;
  p.pixel_cost = nullptr;
  ctx->last_probe_pixels = 0;
  p.sched = nullptr;
  if (c.rlist) {
    p.total_work = (unsigned long long)c.work_pix;  // list slots, in tiles of 64 consecutive ones (the last may be partial)
    p.chunk = tor::kTilePixelsHost;
    waves = (c.work_pix + tor::kTilePixelsHost - 1) / tor::kTilePixelsHost;
  } else if (o.seeding == TOR_SEED_PIXEL) {
    p.total_work = (unsigned long long)c.n_tiles * tor::kTilePixelsHost;  // tiles of 64 pixels
    p.chunk = tor::kTilePixelsHost;
    waves = c.n_tiles;
  } else {
    p.total_work = (unsigned long long)c.work_pix * (unsigned long long)c.spp;
    long long ch = (long long)(p.total_work / (unsigned long long)(f.resident_waves * 16));
    // largest chunk of the guided schedule: up to 1024 samples, or one whole pixel when a pixel has more (<= 4096)
    const long long cap_c = (c.spp > 1024) ? (c.spp < 4096 ? c.spp : 4096) : 1024;
    if (ch < 64) ch = 64;
    if (ch > cap_c) ch = cap_c;
    p.chunk = (unsigned)((ch >= c.spp) ? ch : ch / 64 * 64);
    waves = (long long)((p.total_work + 63) / 64);
  }
  if (waves > f.resident_waves) waves = f.resident_waves;
  blocks = (int)((waves + (tor::kThreads / 64) - 1) / (tor::kThreads / 64));
  if (blocks < 1) blocks = 1;
  p.screen = ctx->screen ? 1 : 0;
  p.n_boxes = f.lay.use_accel ? (int)tor::accel_boxes_padded(*f.lay.hacc) : 0;
  p.mig = nullptr;
  if (migrate) blocks = (int)(f.resident_waves / (tor::kThreads / 64));  // the whole machine: waves without a tile are servers at once
  p.n_waves = (unsigned)(blocks * (tor::kThreads / 64));
  p.wave_log = nullptr;
  if (ctx->collect_stats) {
    HIP_TRY(ctx->wave_log.ensure((size_t)p.n_waves * 64));
    HIP_TRY(hipMemsetAsync(ctx->wave_log.ptr, 0, (size_t)p.n_waves * 64, c.stream));
    p.wave_log = (unsigned long long*)ctx->wave_log.ptr;
    ctx->last_n_waves = (int64_t)p.n_waves;
  }
  TOR_TRY(upload_camera(ctx, c, p.cam_dev));
  if (f.lay.use_accel) {
    const std::vector<double>& bnd_host = ctx->bnd_host[c.slot];
    HIP_TRY(hipMemcpyAsync((void*)p.bnd, bnd_host.data(), bnd_host.size() * 8, hipMemcpyHostToDevice, c.stream));
    if (p.bnd32)
      HIP_TRY(hipMemcpyAsync((void*)p.bnd32, ctx->bnd32_host[c.slot].data(), ctx->bnd32_host[c.slot].size() * 4, hipMemcpyHostToDevice, c.stream));
  }
  return TOR_OK;
}

// The cost probe: a 2-spp launch on per-sample streams that only counts closest-hit queries per pixel (into tile_cost; it
// never touches the canvas).
static int launch_cost_probe(TorContext* ctx, const RenderCall& c, const tor::KParams& p, DeviceBuffer& tile_cost) {
  const int slot = c.slot;
  tor::KParams pp = p;
  if (ctx->probe_accel && (c.o.accel & TOR_ACCEL_BLOCKS) == 0) {
    // The probe only counts closest-hit queries per pixel -- the count does not depend on how a hit is found -- so a launch
    // without the block culling (whose ring slot of block bounds is free) still probes with both exact accelerations when
    // the scene has them: 2.5 ms instead of 7.7 ms in front of a float64 brute-force 1080p frame.
    tor::KParams pa = p;
    LayoutChoice pl;
    TOR_TRY(configure_layout(ctx, c, TOR_ACCEL_BLOCKS | TOR_ACCEL_F32, pa, ctx->probe_bnd_host[slot], ctx->probe_bnd32_host[slot], pl));
    if (pl.use_accel && pa.shot32 != nullptr && pa.bnd32 != nullptr) {
      HIP_TRY(hipMemcpyAsync((void*)pa.bnd, ctx->probe_bnd_host[slot].data(), ctx->probe_bnd_host[slot].size() * 8, hipMemcpyHostToDevice, c.stream));
      HIP_TRY(hipMemcpyAsync((void*)pa.bnd32, ctx->probe_bnd32_host[slot].data(), ctx->probe_bnd32_host[slot].size() * 4, hipMemcpyHostToDevice, c.stream));
      pp = pa;
    }
  }
  pp.spp = ctx->probe_spp;
  pp.inv_spp = 1.0 / (double)ctx->probe_spp;
  pp.total_work = (unsigned long long)c.npix * (unsigned long long)ctx->probe_spp;
  ctx->last_probe_pixels = c.npix;
  pp.chunk = 256;
  pp.work_counter = c.slot_counters + 5;
  pp.stats = nullptr;
  pp.wave_log = nullptr;
  pp.out = nullptr;
  pp.pixel_cost = (unsigned*)tile_cost.ptr;
  long long pw = (long long)((pp.total_work + 63) / 64);
  const long long pres = (long long)ctx->num_cus * 3 * (tor::kThreads / 64);
  if (pw > pres) pw = pres;
  const int pblocks = (int)((pw + (tor::kThreads / 64) - 1) / (tor::kThreads / 64));
  pp.n_waves = (unsigned)(pblocks * (tor::kThreads / 64));
  HIP_TRY(tor::launch_probe(pp, pblocks, c.stream));
  return TOR_OK;
}

// The hand-off's queue of handed-over chains: 64-byte records + ready flags (zeroed per launch), control words in the ring slot;
// and the part of the tile schedule that sets its thresholds.
static int setup_handoff_queue(TorContext* ctx, const RenderCall& c, tor::KParams& p, tor::MigSchedule& ms, int blocks) {
  const size_t cap = (size_t)(c.npix < (1ll << 20) ? c.npix : (1ll << 20));
  HIP_TRY(ctx->mig_rec.ensure(cap * 64));
  HIP_TRY(ctx->mig_flag.ensure(cap * 4));
  HIP_TRY(hipMemsetAsync(ctx->mig_flag.ptr, 0, cap * 4, c.stream));
  p.mig = c.slot_counters + TorContext::kMigWord0;
  p.mig_rec = (unsigned long long*)ctx->mig_rec.ptr;
  p.mig_flag = (unsigned*)ctx->mig_flag.ptr;
  p.mig_cap = (unsigned)cap;
  p.mig_tail_lanes = ctx->mig_tail_lanes;
  p.mig_flags = ctx->mig_flags;
  p.mig_patience = (unsigned)(ctx->srv_patience_us > 0 ? ctx->srv_patience_us : 0) * 100u;
  p.mig_tail_rest = ctx->mig_tail_rest;
  // (read per launch, not per context: the drop-in's cached contexts outlive any one caller's settings)
  double stall_s = ctx->mig_stall_s;
  if (const char* s = tor::knob("TOR_SRV_STALL_S")) stall_s = std::atof(s);
  p.mig_stall_ticks = stall_s > 0.0 ? (unsigned long long)(stall_s * 1e8) + 2ull : (stall_s < 0.0 ? 1ull : 0ull);  // (< 0, a test setting: every waiting server gives up at its first look)
  ms.mig = p.mig;
  ms.lavg_scale = (float)c.spp / (float)ctx->probe_spp / ((float)blocks * (float)tor::kThreads);
  ms.srv_frac = ctx->srv_frac;
  ms.srv_min_frac = ctx->srv_min_frac;
  ms.push_theta = ctx->push_theta;
  ms.chain_scale = (float)c.spp / (float)ctx->probe_spp / (float)c.npix;
  ms.chain_theta = ctx->chain_theta;
  ms.floor_theta = ctx->floor_theta;
  ms.blocks = blocks;
  ms.spp = c.spp;
  ms.max_depth = (int)c.max_depth;
  return TOR_OK;
}

// Cost-ordered schedule of a SEED_PIXEL frame: a 2-spp probe + a counting sort; ~2/spp of extra work.  With `split_ok` it also
// decides split mode -- `split` says whether it applies, `wk` is then the wave kernel's KParams -- and with `migrate` it sets up
// the hand-off queue.
static int probe_and_schedule(TorContext* ctx, const RenderCall& c, FrameConfig& f, int blocks, bool migrate, bool split_ok, float split_frac,
                              tor::KParams& wk, bool& split) {
  split = false;
  // (a listed pass runs no probe and no tile order: the probe costs 2 samples of EVERY pixel of the shard -- more than a pass of 16 over a
  // list of a few per cent of them -- and its tiles are tiles of pixels, not of list slots)
  if (!(c.o.seeding == TOR_SEED_PIXEL && ctx->lpt_min_spp > 0 && c.spp >= ctx->lpt_min_spp && c.n_tiles > 1 && !c.rlist)) return TOR_OK;
  tor::KParams& p = f.p;
  const long long npix = c.npix, n_tiles = c.n_tiles;
  // (one buffer per context, not per ring slot: only the probe and the two sort kernels touch it, and the launches of a
  // context are ordered on one stream)
  DeviceBuffer& tile_cost = ctx->probe_buf;
  DeviceBuffer& tile_order = ctx->tile_order[c.slot];
  // per-pixel query counts of the probe, then per tile: sort key, probed work
  HIP_TRY(tile_cost.ensure(((size_t)npix + 2 * (size_t)n_tiles) * 4 + tor::kTileSortScratchBytes));
  HIP_TRY(tile_order.ensure((size_t)n_tiles * 4));
  HIP_TRY(hipMemsetAsync(tile_cost.ptr, 0, (size_t)npix * 4, c.stream));
  TOR_TRY(launch_cost_probe(ctx, c, p, tile_cost));
  // Split mode (mid-size frames): the lane kernel is bound by its longest pixel chains, the wave-per-pixel kernel by
  // its throughput -- so the most expensive tiles (split_frac of the probed cost) go to the wave kernel on a second
  // stream while the lane kernel renders the rest.  Disjoint pixels, same arithmetic: same canvas.
  if (split_ok) {
    TOR_TRY(tor::ensure_layouts(ctx, 0));
    wk = p;
    coop_params(wk, ctx->flat[0]);
    wk.order = (const unsigned*)tile_order.ptr;
    wk.split = c.slot_counters + 6;
    wk.work_counter = c.slot_counters + 7;
    wk.stats = nullptr;
    wk.wave_log = nullptr;
    split = tor::coop_blocks_per_cu(wk, c.o.arith) > 0;
  }
  unsigned* const tile_key = (unsigned*)tile_cost.ptr + npix;
  // schedule of the lane kernel (tor_kernels.hip): the hot chains -- a pixel chain is hot when it needs more than hot_frac of the
  // iterations an average wave runs in this frame
  //   average = total probed queries * spp / probe_spp / lanes
  p.prio_shift = ctx->prio_shift;
  p.sched = c.slot_counters + 8;
  tor::MigSchedule ms;
  ms.key_mode = ctx->key_mode;
  ms.probe_spp = ctx->probe_spp;
  if (migrate) TOR_TRY(setup_handoff_queue(ctx, c, p, ms, blocks));
  HIP_TRY(tor::launch_tile_order((const unsigned*)tile_cost.ptr, (unsigned)npix, tile_key, tile_key + n_tiles, (unsigned*)tile_order.ptr,
                                 (int)n_tiles, split ? split_frac : 0.0f, split ? c.slot_counters + 6 : nullptr,
                                 split ? c.slot_counters : nullptr,
                                 ctx->hot_frac > 0.0f ? ctx->hot_frac * (float)c.spp / (float)ctx->probe_spp / (float)(f.resident_waves * 64) : -1.0f,
                                 p.sched, ms, c.stream));
  p.order = (const unsigned*)tile_order.ptr;
  return TOR_OK;
}

// A hand-off launch covers the whole machine and its waves WAIT for each other (servers for lane waves): two of them
// interleaved on one GPU -- two contexts on one device, e.g. a device list that repeats an ordinal -- would each hold part
// of the machine and wait for workgroups that can never start.  So hand-off launches of this process are chained per
// device: each waits (on the device, not the host) for the previous one's end event.  Kernels without
// inter-workgroup waits may still overlap it; they end on their own.
static int launch_handoff(TorContext* ctx, const RenderCall& c, const FrameConfig& f, int blocks) {
  std::lock_guard<std::mutex> lock(g_handoff_mutex);
  hipEvent_t& ev = g_handoff_event[ctx->device];
  if (ev) HIP_TRY(hipStreamWaitEvent(c.stream, ev, 0));
  else HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  TOR_TRY(launch_bracketed(ctx, c, nullptr, 0, &f.p, f.waves_per_simd, blocks));
  HIP_TRY(hipEventRecord(ev, c.stream));
  return TOR_OK;
}

// A pass (acc) leaves raw sums: tor_resolve_device finalizes.  One condition for all three launches: the wave kernel and split
// mode run on TOR_SEED_PIXEL only, where decode_call admits no pass but a resume pass -- there `acc` is `resume`.
static int finish_call(const RenderCall& c) {
  if (c.acc) return TOR_OK;
  // canvas.nim:47-54
  HIP_TRY(tor::launch_finalize(c.d_pixels, c.n_values, 1.0 / (double)c.spp, 1.0 / (double)c.gamma_correction, c.stream));
  return TOR_OK;
}

// All five render entries: the phases above, in order.
static int render_device_impl(TorContext* ctx, const TorOptions* opt, RenderCall& c) {
  TOR_TRY(decode_call(ctx, opt, c));
  if (c.work_pix == 0) return TOR_OK;
  TOR_TRY(claim_ring_slot(ctx, c));
  // (a resume pass takes no shortcut: with max_depth <= 0 the reference still draws every sample's pixel jitter, lens and time
  // samples -- render.nim:63-65, cameras.nim:47-57 -- and the states must advance exactly so; its kernels end such a sample black)
  if (!c.resume && (c.max_depth <= 0 || ctx->n_objects < 0)) {
    if (c.acc) return TOR_OK;  // every sample is black: the pass adds zeros, the sums (and moments) stay as they are
    // render.nim:25: the bounce loop does not run -> every sample is black -> pow(0, g) = 0
    HIP_TRY(hipMemsetAsync(c.d_pixels, 0, (size_t)c.n_values * 8, c.stream));
    return TOR_OK;
  }
  if (c.o.seeding == TOR_SEED_SAMPLE && !c.acc) HIP_TRY(hipMemsetAsync(c.d_pixels, 0, (size_t)c.n_values * 8, c.stream));

  // The frame is configured (layouts built, block bounds computed) where it was always configured: before the hand-off decision
  // for its candidates, else only once the wave-per-pixel kernel -- which needs the float64 flat layout alone -- has not taken it.
  FrameConfig f;
  const float split_frac = split_fraction(ctx, c);
  const bool candidate = handoff_candidate(ctx, c);
  if (candidate) TOR_TRY(configure_frame(ctx, c, f));
  const bool migrate = candidate && handoff_runs(ctx, c, f);
  const bool split_ok = !migrate && split_applies(ctx, c, split_frac);
  if (wave_kernel_wanted(ctx, c, split_ok || migrate)) {
    bool launched = false;
    TOR_TRY(launch_wave_frame(ctx, c, launched));
    if (launched) return finish_call(c);
  }
  if (!candidate) TOR_TRY(configure_frame(ctx, c, f));

  int blocks = 0;
  bool split = false;
  tor::KParams wk{};
  TOR_TRY(prepare_lane_launch(ctx, c, f, migrate, blocks));
  TOR_TRY(probe_and_schedule(ctx, c, f, blocks, migrate, split_ok, split_frac, wk, split));
  ctx->last_migrate = migrate && f.p.mig != nullptr;
  if (split) TOR_TRY(launch_bracketed(ctx, c, &wk, 0, &f.p, f.waves_per_simd, blocks));
  else if (ctx->last_migrate) TOR_TRY(launch_handoff(ctx, c, f, blocks));
  else TOR_TRY(launch_bracketed(ctx, c, nullptr, 0, &f.p, f.waves_per_simd, blocks));
  return finish_call(c);
}

int tor_render_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                      int32_t spp, float gamma_correction, int64_t max_depth, const TorOptions* opt,
                      double* d_pixels, void* hip_stream) {
  RenderCall c{"tor_render_device", cam, nrows, ncols, spp, gamma_correction, max_depth, d_pixels, (hipStream_t)hip_stream, nullptr};
  return render_device_impl(ctx, opt, c);
}

// ---- progressive rendering (TOR_SEED_SAMPLE): passes of samples into raw sums, resolve, noise -------------------------
// Exactness bound: a sample's quantised radiance q is a multiple of 2^-36 in [0, 1] per channel (the sky is at most 1 --
// render.nim:41-45 -- and every bounce multiplies by an albedo of at most 1: scenes.nim's materials, the same assumption the
// one-shot TOR_SEED_SAMPLE mode rests on).  A sum of N such values is k * 2^-36 with k <= N * 2^36; float64 holds every
// integer k <= 2^53 exactly, so every partial sum -- in any order, any split -- is exact for N <= 2^17.  The moments
// quantize36(q * q) lie in [0, 1] too: same bound.
static const int64_t kMaxAccumSamples = (int64_t)1 << 17;

int tor_render_accumulate_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int32_t first_sample,
                                 int32_t n_samples, int64_t max_depth, const TorOptions* opt, double* d_sums, double* d_moments,
                                 void* hip_stream) {
  if (first_sample < 0 || n_samples < 1 || (int64_t)first_sample + n_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_accumulate_device: need first_sample >= 0, n_samples >= 1 and first_sample + n_samples "
                                          "<= 2^17 (131072): beyond that the 2^-36-granular float64 sums are no longer exact");
  if (!ctx || !cam || !d_sums) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_accumulate_device: NULL argument");
  const tor::AccumLaunch acc{first_sample, d_moments};
  RenderCall c{"tor_render_accumulate_device", cam, nrows, ncols, n_samples, 2.2f, max_depth, d_sums, (hipStream_t)hip_stream, &acc};
  return render_device_impl(ctx, opt, c);
}

// ---- resumable rendering on the reference's per-pixel streams (TOR_SEED_PIXEL) -----------------------------------------
// The first k samples of a pixel do not depend on spp (it only enters Canvas.draw's final scale), so a pixel that has run k samples and
// kept {generator state, raw sequential sum} IS the reference's pixel at k spp and goes on being the reference's pixel at any n > k.
// The 2^17 bound is not an exactness bound here (the sums are plain sequential float64 sums in sample order, as render.nim:67 forms
// them): it is the range tor_resolve_device and tor_accum_noise_device accept, so that both serve this mode unchanged.
int tor_render_resume_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int32_t first_sample, int32_t n_samples,
                             int64_t max_depth, const TorOptions* opt, TorRng* d_rng, double* d_sums, double* d_moments, void* hip_stream) {
  if (first_sample < 0 || n_samples < 1 || (int64_t)first_sample + n_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_resume_device: need first_sample >= 0, n_samples >= 1 and first_sample + n_samples <= 2^17 "
                                          "(131072): the range tor_resolve_device and tor_accum_noise_device accept");
  if (!ctx || !cam || !d_rng || !d_sums) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_resume_device: NULL argument");
  tor::AccumLaunch acc{first_sample, d_moments};
  acc.rng = (unsigned long long*)d_rng;
  RenderCall c{"tor_render_resume_device", cam, nrows, ncols, n_samples, 2.2f, max_depth, d_sums, (hipStream_t)hip_stream, &acc};
  return render_device_impl(ctx, opt, c);
}

// ... over a pixel list: adaptive sampling on the reference's streams.  The list rules are tor_render_accumulate_list_device's; the pass
// is tor_render_resume_device's for the listed pixels and leaves every other pixel's state, sums and moments alone.
int tor_render_resume_list_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, const int32_t* d_list, int32_t n_list,
                                  int32_t first_sample, int32_t n_samples, int64_t max_depth, const TorOptions* opt, TorRng* d_rng,
                                  double* d_sums, double* d_moments, void* hip_stream) {
  const char* who = "tor_render_resume_list_device";
  if (first_sample < 0 || n_samples < 1 || (int64_t)first_sample + n_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": need first_sample >= 0, n_samples >= 1 and first_sample + n_samples <= 2^17 "
                                          "(131072): the range tor_adaptive_select_device, tor_resolve_counts_device and tor_accum_noise_device accept");
  if (n_list < 0) return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": n_list < 0");
  {  // (checked before the context is touched: the list may not be longer than the shard)
    TorOptions o;
    if (nrows >= 2 && ncols >= 2 && valid_options(opt, o, false)) {
      const long long npix = (long long)tor_shard_rows(nrows, o.row_tile, o.shard_index, o.shard_count, nullptr) * ncols;
      if ((long long)n_list > npix)
        return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": n_list = " + std::to_string(n_list) + " is above the shard's " +
                                              std::to_string(npix) + " pixels");
    }
  }
  if (!ctx || !cam || !d_rng || !d_sums || !d_moments || (!d_list && n_list > 0))
    return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument (generator states, sums and moments are all required, and the list unless n_list is 0)");
  // (an empty pass takes the common path up to its no-op return, so that it is checked like any other; its list is never read)
  static const int32_t empty_list[1] = {0};
  tor::AccumLaunch acc{first_sample, d_moments, n_list > 0 ? d_list : empty_list, n_list};
  acc.rng = (unsigned long long*)d_rng;
  RenderCall c{"tor_render_resume_list_device", cam, nrows, ncols, n_samples, 2.2f, max_depth, d_sums, (hipStream_t)hip_stream, &acc};
  return render_device_impl(ctx, opt, c);
}

int tor_resolve_device(TorContext* ctx, const double* d_sums, int64_t n_values, int64_t total_samples, float gamma_correction,
                       double* d_pixels, void* hip_stream) {
  if (n_values < 0 || total_samples < 1 || total_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_resolve_device: need n_values >= 0 and 1 <= total_samples <= 2^17");
  if (!ctx || !d_sums || !d_pixels) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_resolve_device: NULL argument");
  HIP_TRY(hipSetDevice(ctx->device));
  // canvas.nim:47-54 with finalize_kernel's operands: a resolved progressive frame is the one-shot frame bit for bit
  HIP_TRY(tor::launch_resolve(d_sums, d_pixels, n_values, 1.0 / (double)total_samples, 1.0 / (double)gamma_correction, (hipStream_t)hip_stream));
  return TOR_OK;
}

int tor_accum_noise_device(TorContext* ctx, const double* d_sums, const double* d_moments, int64_t npix, int64_t total_samples,
                           double* d_err, double out[2], void* hip_stream) {
  if (npix < 1 || total_samples < 2 || total_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_accum_noise_device: need npix >= 1 and 2 <= total_samples <= 2^17 (the variance needs two samples)");
  if (!ctx || !d_sums || !d_moments || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_accum_noise_device: NULL argument");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  HIP_TRY(ctx->noise.ensure(((size_t)tor::kNoiseMaxBlocks + 1) * 2 * sizeof(double)));
  double* partials = (double*)ctx->noise.ptr;
  double* dout = partials + 2 * tor::kNoiseMaxBlocks;
  HIP_TRY(tor::launch_accum_noise(d_sums, d_moments, npix, (double)total_samples, d_err, partials, dout, stream));
  double h[2] = {0.0, 0.0};
  HIP_TRY(hipMemcpyAsync(h, dout, sizeof(h), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  out[0] = h[0] / (double)npix;
  out[1] = h[1];
  return TOR_OK;
}

// ---- adaptive sampling (TOR_SEED_SAMPLE): passes over a shrinking list of pixels, convergence select, per-pixel resolve ---------
int tor_render_accumulate_list_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, const int32_t* d_list,
                                      int32_t n_list, int32_t first_sample, int32_t n_samples, int64_t max_depth, const TorOptions* opt,
                                      double* d_sums, double* d_moments, void* hip_stream) {
  const char* who = "tor_render_accumulate_list_device";
  if (first_sample < 0 || n_samples < 1 || (int64_t)first_sample + n_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": need first_sample >= 0, n_samples >= 1 and first_sample + n_samples "
                                          "<= 2^17 (131072): beyond that the 2^-36-granular float64 sums are no longer exact");
  if (n_list < 0) return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": n_list < 0");
  {  // (checked before the context is touched: the list may not be longer than the shard)
    TorOptions o;
    if (nrows >= 2 && ncols >= 2 && valid_options(opt, o, false)) {
      const long long npix = (long long)tor_shard_rows(nrows, o.row_tile, o.shard_index, o.shard_count, nullptr) * ncols;
      if ((long long)n_list > npix)
        return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": n_list = " + std::to_string(n_list) + " is above the shard's " +
                                              std::to_string(npix) + " pixels");
    }
  }
  if (!ctx || !cam || !d_list || !d_sums || !d_moments) return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument (sums and moments are both required)");
  const tor::AccumLaunch acc{first_sample, d_moments, d_list, n_list};
  RenderCall c{"tor_render_accumulate_list_device", cam, nrows, ncols, n_samples, 2.2f, max_depth, d_sums, (hipStream_t)hip_stream, &acc};
  return render_device_impl(ctx, opt, c);
}

int tor_adaptive_select_device(TorContext* ctx, const double* d_sums, const double* d_moments, const int32_t* d_list_in, int32_t n_in,
                               int64_t total_samples, double abs_tol, double rel_tol, int32_t* d_list_out, int32_t* d_counts, int32_t* n_out,
                               void* hip_stream) {
  const char* who = "tor_adaptive_select_device";
  if (n_in < 0) return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": n_in < 0");
  if (total_samples < 2 || total_samples > kMaxAccumSamples)
    return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": need 2 <= total_samples <= 2^17 (the variance needs two samples)");
  if (!(abs_tol >= 0.0) || !(rel_tol >= 0.0))  // (false for NaN too)
    return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": tolerances must be >= 0 and not NaN");
  if (!ctx || !d_sums || !d_moments || !d_list_in || !d_list_out || !d_counts || !n_out)
    return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": NULL argument");
  if (d_list_out == d_list_in) return fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": d_list_out must not alias d_list_in");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  // [0, 16): the survivor count; then the compaction's scratch
  HIP_TRY(ctx->adapt.ensure(16 + tor::adaptive_select_scratch_bytes(n_in)));
  int32_t* dn = (int32_t*)ctx->adapt.ptr;
  HIP_TRY(tor::launch_adaptive_select(d_sums, d_moments, d_list_in, n_in, (double)total_samples, abs_tol, rel_tol, d_list_out, d_counts,
                                      (char*)ctx->adapt.ptr + 16, dn, stream));
  int32_t h = 0;
  HIP_TRY(hipMemcpyAsync(&h, dn, sizeof(h), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *n_out = h;
  return TOR_OK;
}

int tor_resolve_counts_device(TorContext* ctx, const double* d_sums, const int32_t* d_counts, int64_t npix, float gamma_correction,
                              double* d_pixels, void* hip_stream) {
  if (npix < 0) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_resolve_counts_device: npix < 0");
  if (!ctx || !d_sums || !d_counts || !d_pixels) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_resolve_counts_device: NULL argument");
  HIP_TRY(hipSetDevice(ctx->device));
  // resolve_kernel's operands with scale = 1.0 / (double)counts[pixel], computed on the device exactly as the host computes it
  HIP_TRY(tor::launch_resolve_counts(d_sums, d_counts, d_pixels, npix * 3, 1.0 / (double)gamma_correction, (hipStream_t)hip_stream));
  return TOR_OK;
}

int tor_quantize_rgb8_device(TorContext* ctx, const double* d_pixels, int64_t n_values, uint8_t* d_rgb8,
                             void* hip_stream) {
  if (!ctx || !d_pixels || !d_rgb8 || n_values < 0)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_quantize_rgb8_device: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(tor::launch_quantize(d_pixels, n_values, d_rgb8, (hipStream_t)hip_stream));
  return TOR_OK;
}

// ---- video output stage (io/rgb.nim, io/color_conversions.nim, io/h264.nim) --------------------

int64_t tor_h264_frame_bytes(int32_t width, int32_t height) {
  // 4:2:0: even sizes.  A size that is not a multiple of 16 is coded with its last macroblock row / column padded by edge
  // replication and cropped away again by the SPS (tor_h264_stream_header): the standard's way (H.264 7.4.2.1.1).  The
  // reference has a TODO there (h264.nim:178): its SPS announces ceil(size / 16) macroblocks, its flushFrame writes
  // floor(size / 16) -- at 1920x1080, BASELINE configs[4]'s size, a stream no decoder accepts.
  if (width < 2 || height < 2 || (width & 1) || (height & 1) || width > 65520 || height > 65520) return TOR_ERR_INVALID_ARGUMENT;
  const int64_t n_mb = (int64_t)((width + 15) >> 4) * ((height + 15) >> 4);
  return n_mb * 386 + 8;  // slice header 9 + 384 per macroblock + 2 per macroblock after the first + stop byte
}

// initSPS (h264.nim:90-142) followed by the constant PPS (h264.nim:37), as H264Encoder.init writes
// them (h264.nim:174-176).  Returns the number of bytes written or a negative status.
int tor_h264_stream_header(int32_t width, int32_t height, uint8_t* out, int32_t cap) {
  if (!out || tor_h264_frame_bytes(width, height) < 0) return TOR_ERR_INVALID_ARGUMENT;
  std::vector<uint8_t> b = {0x00, 0x00, 0x00, 0x01};
  unsigned acc = 0;
  int nbits = 0;
  auto put = [&](int n, unsigned v) {  // MSB first
    for (int k = n - 1; k >= 0; --k) {
      acc = (acc << 1) | ((v >> k) & 1u);
      if (++nbits == 8) { b.push_back((uint8_t)acc); acc = 0; nbits = 0; }
    }
  };
  auto ue = [&](unsigned v) {  // putGolomb, h264.nim:73-78
    int size = 1;
    unsigned t = v + 1;
    while ((t >>= 1) != 0) ++size;
    put(2 * size - 1, v + 1);
  };
  put(1, 0); put(2, 3); put(5, 7);        // forbidden_zero_bit, nal_ref_idc, nal_unit_type = SPS
  put(8, 66);                             // baseline profile
  put(1, 0); put(1, 0); put(1, 0); put(1, 0); put(4, 0);  // constraint flags, reserved
  put(8, 10);                             // level_idc
  ue(0); ue(0); ue(0); ue(0);             // sps id, log2_max_frame_num-4, poc type, log2_max_poc_lsb-4
  ue(0); put(1, 0);                       // num_ref_frames, gaps_in_frame_num_value_allowed
  ue((unsigned)(((width + 15) >> 4) - 1));
  ue((unsigned)(((height + 15) >> 4) - 1));
  put(1, 1); put(1, 0);                   // frame_mbs_only, direct_8x8_inference
  const unsigned crop_r = (unsigned)((((width + 15) >> 4) << 4) - width) / 2, crop_b = (unsigned)((((height + 15) >> 4) << 4) - height) / 2;
  if (crop_r == 0 && crop_b == 0) {
    put(1, 0);                            // frame_cropping_flag: the reference never sets it (h264.nim:178 TODO) -- same bytes for multiples of 16
  } else {
    put(1, 1);                            // padded macroblocks are cropped away: offsets in units of 2 luma samples (4:2:0 frames)
    ue(0); ue(crop_r); ue(0); ue(crop_b);  // left, right, top, bottom
  }
  put(1, 0); put(1, 1);                   // vui_parameters_present, stop bit
  if (nbits > 0) b.push_back((uint8_t)(acc << (8 - nbits)));
  const uint8_t pps[8] = {0x00, 0x00, 0x00, 0x01, 0x68, 0xce, 0x38, 0x80};
  b.insert(b.end(), pps, pps + 8);
  if ((int)b.size() > cap) return TOR_ERR_INVALID_ARGUMENT;
  std::memcpy(out, b.data(), b.size());
  return (int)b.size();
}

int tor_encode_frame_device(TorContext* ctx, const double* d_pixels, int32_t nrows, int32_t ncols, uint8_t* d_slice,
                            uint8_t* d_y, uint8_t* d_cb, uint8_t* d_cr, void* hip_stream) {
  if (!ctx || !d_pixels || !d_slice) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_encode_frame_device: NULL argument");
  // h264.nim:178 "TODO cropping for non-multiple of 16": the reference silently drops the partial macroblock rows / columns
  // (flushFrame loops over `div 16`) although its SPS announces them; here they are padded and cropped (tor_h264_frame_bytes).
  if (tor_h264_frame_bytes(ncols, nrows) < 0)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_encode_frame_device: width and height must be even (4:2:0) and at most 65520");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(tor::launch_encode_ipcm(d_pixels, nrows, ncols, d_slice, d_y, d_cb, d_cr, (hipStream_t)hip_stream));
  return TOR_OK;
}

// One turn of the animation driver's loop body (trace_of_radiance_animation.nim:181-196): render the
// frame, convert and pack it on the device, and hand back only the slice NAL unit (1.5 B per pixel
// over PCIe instead of the 24 B per pixel canvas).  Blocking.
int tor_render_frame_h264(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int32_t spp,
                          float gamma_correction, int64_t max_depth, const TorOptions* opt, uint8_t* slice_out,
                          int64_t cap) {
  if (!ctx || !cam || !slice_out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_frame_h264: NULL argument");
  const int64_t n = tor_h264_frame_bytes(ncols, nrows);
  if (n < 0) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_frame_h264: width and height must be even (4:2:0) and at most 65520");
  if (cap < n) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_frame_h264: output buffer too small");
  if (opt && opt->shard_count > 1) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_frame_h264: whole frames only");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(ctx->scratch.ensure((size_t)nrows * ncols * 24));
  HIP_TRY(ctx->slice.ensure((size_t)n));
  int rc = tor_render_device(ctx, cam, nrows, ncols, spp, gamma_correction, max_depth, opt, (double*)ctx->scratch.ptr, nullptr);
  if (rc != TOR_OK) return rc;
  rc = tor::rerender_if_stalled(ctx, cam, nrows, ncols, spp, gamma_correction, max_depth, opt, (double*)ctx->scratch.ptr, nullptr);
  if (rc != TOR_OK) return rc;
  rc = tor_encode_frame_device(ctx, (const double*)ctx->scratch.ptr, nrows, ncols, (uint8_t*)ctx->slice.ptr, nullptr, nullptr,
                               nullptr, nullptr);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipMemcpy(slice_out, ctx->slice.ptr, (size_t)n, hipMemcpyDeviceToHost));
  return TOR_OK;
}

int tor_last_kernel_ms(TorContext* ctx, float* ms_out, int64_t* samples_out) {
  if (!ctx || !ms_out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_kernel_ms: NULL argument");
  if (!ctx->timing_valid) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_kernel_ms: no timed launch");
  HIP_TRY(hipSetDevice(ctx->device));
  const int slot = (int)((ctx->launches - 1) % TorContext::kRing);
  HIP_TRY(hipEventSynchronize(ctx->ev_stop[slot]));
  HIP_TRY(hipEventElapsedTime(ms_out, ctx->ev_start[slot], ctx->ev_stop[slot]));
  if (samples_out) *samples_out = ctx->last_samples;
  // an asynchronous caller that comes here to learn that its launch is over also learns when the frame is NOT whole
  // (ADVICE r4): the hand-off's stall escape leaves holes, and only tor_context_handoff_stalled used to say so
  if (ctx->last_migrate && slot == ctx->last_slot) {
    unsigned long long w = 0;
    HIP_TRY(hipMemcpy(&w, (unsigned long long*)ctx->counters.ptr + (size_t)slot * TorContext::kSlotWords + TorContext::kMigWord0 + tor::kMigStalled,
                      sizeof w, hipMemcpyDeviceToHost));
    if (w != 0)
      return fail(TOR_ERR_INCOMPLETE, "tor_last_kernel_ms: the launch's chain hand-off stalled (not all of its workgroups were resident) and flagged the "
                                      "frame INCOMPLETE -- render it again (tor_context_handoff_stalled; the blocking entry points do so themselves)");
  }
  return TOR_OK;
}

int tor_kernel_ms_mean(TorContext* ctx, int32_t last_n, float* mean_ms_out, int32_t* n_used_out) {
  if (!ctx || !mean_ms_out || last_n < 1) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_kernel_ms_mean: bad argument");
  if (!ctx->timing_valid || ctx->launches < 1) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_kernel_ms_mean: no timed launch");
  HIP_TRY(hipSetDevice(ctx->device));
  int64_t n = last_n;
  if (n > ctx->launches) n = ctx->launches;
  if (n > TorContext::kRing) n = TorContext::kRing;
  double sum = 0.0;
  for (int64_t k = 0; k < n; ++k) {
    const int slot = (int)((ctx->launches - 1 - k) % TorContext::kRing);
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(ctx->ev_stop[slot]));
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_start[slot], ctx->ev_stop[slot]));
    sum += ms;
  }
  *mean_ms_out = (float)(sum / (double)n);
  if (n_used_out) *n_used_out = (int32_t)n;
  return TOR_OK;
}

int tor_last_wave_log(TorContext* ctx, uint64_t* out, int64_t cap_waves) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_wave_log: NULL argument");
  if (!ctx->collect_stats || ctx->last_n_waves <= 0) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_wave_log: stats not enabled");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  const int64_t n = ctx->last_n_waves < cap_waves ? ctx->last_n_waves : cap_waves;
  HIP_TRY(hipMemcpy(out, ctx->wave_log.ptr, (size_t)n * 64, hipMemcpyDeviceToHost));
  return (int)n;
}

int64_t tor_last_pixel_cost(TorContext* ctx, uint32_t* out, int64_t cap_pixels) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_pixel_cost: NULL argument");
  if (ctx->last_probe_pixels <= 0) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_pixel_cost: the last launch ran no cost probe");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  const int64_t n = ctx->last_probe_pixels < cap_pixels ? ctx->last_probe_pixels : cap_pixels;
  HIP_TRY(hipMemcpy(out, ctx->probe_buf.ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
  return n;
}

int tor_last_handoff_counters(TorContext* ctx, uint64_t out[16]) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_handoff_counters: NULL argument");
  if (ctx->launches < 1) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_handoff_counters: no launch yet");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long h[tor::kMigWords];
  HIP_TRY(hipMemcpy(h, (unsigned long long*)ctx->counters.ptr + (size_t)ctx->last_slot * TorContext::kSlotWords + TorContext::kMigWord0, sizeof h,
                    hipMemcpyDeviceToHost));
  const int idx[8] = {tor::kMigHead, tor::kMigTail, tor::kMigLaneWaves, tor::kMigSrvWgs, tor::kMigPush, tor::kMigServed, tor::kMigHotPushes, tor::kMigTailPushes};
  for (int k = 0; k < 8; ++k) out[k] = h[idx[k]];
  // [8..12]: microseconds after the kernel's start: work counter dry, last wave out of the lane loop, last hot chain served, last tail chain served; 0 = never
  const unsigned long long t0 = h[tor::kMigT0];
  auto us = [&](unsigned long long t) { return (t == 0 || t == ~0ull || t < t0) ? 0ull : (t - t0) / 100ull; };
  out[8] = us(h[tor::kMigTCounterDry]); out[9] = us(h[tor::kMigTLaneEnd]); out[10] = us(h[tor::kMigTHotDone]); out[11] = us(h[tor::kMigTTailDone]);
  out[12] = h[tor::kMigItsHot]; out[13] = h[tor::kMigItsTail]; out[14] = h[tor::kMigConverted]; out[15] = h[tor::kMigPushNow];
#ifdef TOR_SERVE_PROF
  // profiling build (make SERVE_PROF=1, tools/server_phases.py): shader-clock ticks per phase of the served bounces
  std::fprintf(stderr, "serve_prof query %llu lambertian %llu metal %llu dielectric %llu miss %llu setup %llu n_lambertian %llu n_metal %llu n_dielectric %llu "
               "n_miss %llu rounds %llu candidates %llu total %llu samples %llu q_slab %llu q_slots %llu q_load %llu q_test %llu q_min %llu\n", h[81], h[82], h[83], h[84], h[85], h[86], h[87], h[88], h[89], h[90], h[91], h[92], h[93], h[94], h[75], h[76], h[77], h[78], h[79]);
#endif
  return TOR_OK;
}

int tor_context_handoff_stalled(TorContext* ctx, int32_t* stalled_out, int64_t* total_out) {
  if (!ctx || !stalled_out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_context_handoff_stalled: NULL argument");
  bool st = false;
  const int rc = tor::handoff_stalled(ctx, (hipStream_t)ctx->last_stream, &st);
  if (rc != TOR_OK) return rc;
  *stalled_out = st ? 1 : 0;
  if (total_out) *total_out = ctx->n_stalled_frames;
  return TOR_OK;
}

int tor_last_stats(TorContext* ctx, TorStats* out) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_stats: NULL argument");
  if (!ctx->collect_stats) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_last_stats: stats not enabled");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long h[12];
  HIP_TRY(hipMemcpy(h, (unsigned long long*)ctx->counters.ptr + (size_t)ctx->last_slot * TorContext::kSlotWords, sizeof h, hipMemcpyDeviceToHost));
  out->hit_queries = h[1];
  out->object_tests = h[1] * (uint64_t)ctx->n_objects;
  out->candidates = h[2];
  out->wave_iterations = h[3];
  out->lane_slots = h[3] * 64;
  out->samples = h[4];
  // word 11 (= KParams.stats + 10): the cooperative variants count the objects their float32 block filter looked at apart from the
  // survivors that reach the exact float64 test; the per-lane block expansion (TOR_ACCEL_BLOCKS alone) runs the exact test on all 8
  out->block_tests = h[11];
  out->exact_tests = h[2] - h[11];
  return TOR_OK;
}

// ---- the drop-in: host canvas in, host canvas out ---------------------------------------

static std::mutex g_ctx_mutex;
static std::map<std::pair<int, int>, TorContext*> g_default_ctx;  // cached contexts per (device, replica)

}  // extern "C"

namespace tor {
// After a hand-off launch (ctx->last_migrate): waits for the stream and reads the launch's kMigStalled word.
int handoff_stalled(TorContext* ctx, hipStream_t stream, bool* stalled) {
  *stalled = false;
  if (!ctx->last_migrate) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(stream));
  unsigned long long w = 0;
  HIP_TRY(hipMemcpy(&w, (unsigned long long*)ctx->counters.ptr + (size_t)ctx->last_slot * TorContext::kSlotWords + TorContext::kMigWord0 + tor::kMigStalled,
                    sizeof w, hipMemcpyDeviceToHost));
  *stalled = w != 0;
  return TOR_OK;
}

int rerender_if_stalled(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int32_t spp, float gamma_correction,
                        int64_t max_depth, const TorOptions* o, double* d_pixels, hipStream_t stream) {
  bool stalled = false;
  int rc = handoff_stalled(ctx, stream, &stalled);
  if (rc != TOR_OK || !stalled) return rc;
  ctx->n_stalled_frames += 1;
  const int saved = ctx->mig_mode;
  ctx->mig_mode = 0;
  rc = tor_render_device(ctx, cam, nrows, ncols, spp, gamma_correction, max_depth, o, d_pixels, stream);
  ctx->mig_mode = saved;
  return rc;
}

int default_context(int device, int replica, TorContext** out) {
  std::lock_guard<std::mutex> lock(g_ctx_mutex);
  TorContext*& ctx = g_default_ctx[{device, replica}];
  if (!ctx) {
    int rc = tor_context_create(device, &ctx);
    if (rc != TOR_OK) { ctx = nullptr; return rc; }
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { tor_context_destroy(ctx); ctx = nullptr; return fail_hip(e, "hipStreamCreate"); }
  }
  *out = ctx;
  return TOR_OK;
}
}  // namespace tor

extern "C" {

static std::mutex g_render_mutex;  // the drop-in is callable from one host thread at a time

int tor_render_opt(TorCanvas* canvas, const TorCamera* cam, TorHittableList world, int64_t max_depth,
                   const TorOptions* opt) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  const clk::time_point t_call = clk::now();
  if (!canvas || !cam || !canvas->pixels) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render: NULL argument");
  TorOptions o;
  if (!valid_options(opt, o, true)) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render: bad options: " + tor::options_why());
  std::lock_guard<std::mutex> lock(g_render_mutex);
  for (double& t : g_last_timing) t = 0.0;
  if (o.device_count > 1) {
    const int rc = tor::render_multi_device(canvas, cam, world, max_depth, o, g_last_timing);
    g_last_timing[3] = ms_since(t_call);
    return rc;
  }
  int device = o.device;
  if (device < 0) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
      return fail(TOR_ERR_NO_DEVICE, std::string("no HIP device available (") + hipGetErrorString(e) +
                                         "); libtor_mi355x has no CPU fallback");
    HIP_TRY(hipGetDevice(&device));
  }
  TorContext* ctx = nullptr;
  int rc = tor::default_context(device, 0, &ctx);
  if (rc != TOR_OK) return rc;
  clk::time_point t0 = clk::now();
  const int64_t hits_before = ctx->n_cache_hits;
  rc = tor_scene_upload(ctx, world);
  if (rc != TOR_OK) return rc;
  g_last_timing[4] = ctx->n_cache_hits > hits_before ? 1.0 : 0.0;
  {
    // layouts are built here (not inside the timed kernel section) so that out[0] is the whole upload cost
    HIP_TRY(hipSetDevice(ctx->device));
    rc = tor::ensure_layouts(ctx, o.accel);
    if (rc != TOR_OK) return rc;
  }
  g_last_timing[0] = ms_since(t0);
  t0 = clk::now();
  const int32_t nrows = canvas->nrows, ncols = canvas->ncols;
  std::vector<int32_t> rows((size_t)(nrows > 0 ? nrows : 0));
  const int32_t local_rows = tor_shard_rows(nrows, o.row_tile, o.shard_index, o.shard_count, rows.data());
  const size_t row_bytes = (size_t)(ncols > 0 ? ncols : 0) * 24;
  HIP_TRY(ctx->scratch.ensure((size_t)(local_rows > 0 ? local_rows : 1) * (row_bytes > 0 ? row_bytes : 24)));
  // out[1] ("launch + kernels until the device is done") is measured on the device: one event in front of the launches, one
  // behind the last kernel; the D2H queues behind them without a host synchronisation in between, and out[2] is the rest
  // of the section (the part of the download that did not overlap nothing: copies + the host-side row placement)
  if (!ctx->ev_call[0]) {
    HIP_TRY(hipEventCreate(&ctx->ev_call[0]));
    HIP_TRY(hipEventCreate(&ctx->ev_call[1]));
  }
  HIP_TRY(hipEventRecord(ctx->ev_call[0], ctx->stream));
  rc = tor_render_device(ctx, cam, nrows, ncols, canvas->samples_per_pixel, canvas->gamma_correction,
                         max_depth, &o, (double*)ctx->scratch.ptr, ctx->stream);
  if (rc != TOR_OK) return rc;
  // (a hand-off launch whose servers gave up -- not all of its workgroups were resident -- left the frame incomplete: render it
  // again without the hand-off before anything reaches the caller's canvas)
  rc = tor::rerender_if_stalled(ctx, cam, nrows, ncols, canvas->samples_per_pixel, canvas->gamma_correction, max_depth, &o,
                                (double*)ctx->scratch.ptr, ctx->stream);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipEventRecord(ctx->ev_call[1], ctx->stream));
  rc = tor::download_rows(ctx, ctx->scratch.ptr, local_rows, row_bytes, o.shard_count > 1 ? rows.data() : nullptr,
                          (char*)canvas->pixels, ctx->stream);
  if (rc != TOR_OK) return rc;
  const double section = ms_since(t0);
  float dev_ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&dev_ms, ctx->ev_call[0], ctx->ev_call[1]));  // (both events are complete: download_rows waited for the stream)
  g_last_timing[1] = (double)dev_ms < section ? (double)dev_ms : section;
  g_last_timing[2] = section - g_last_timing[1];
  g_last_timing[3] = ms_since(t_call);
  return TOR_OK;
}

int tor_render(TorCanvas* canvas, const TorCamera* cam, TorHittableList world, int64_t max_depth) {
  return tor_render_opt(canvas, cam, world, max_depth, nullptr);
}

int tor_render_ptr(TorCanvas* canvas, const TorCamera* cam, const TorHittableList* world, int64_t max_depth) {
  if (!world) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_render_ptr: world is NULL");
  return tor_render_opt(canvas, cam, *world, max_depth, nullptr);
}

// Debug view of the TOR_ACCEL_BLOCKS layout (host only, no device needed): for the given object list and
// ray-time range, writes per spatial slot the original object index (-1 for padding) and per block its
// box {lo xyz, hi xyz}, then the super boxes.  Returns the number of blocks (0: no second level is built),
// or a negative status.  Used by the CPU test that checks the boxes are conservative.
int tor_debug_accel_layout(TorHittableList world, double t_lo, double t_hi, int64_t* slot_object, int64_t slot_cap,
                           double* block_boxes, double* super_boxes, int64_t box_cap, int32_t* two_level_out) {
  if (world.len < 0 || (world.len > 0 && !world.objects)) return TOR_ERR_INVALID_ARGUMENT;
  tor::HostAccel acc;
  tor::build_accel(world.objects, world.len, acc);
  if (!acc.available) return 0;
  std::vector<double> bnd;
  if (!tor::compute_block_bounds(acc, t_lo, t_hi, bnd)) return 0;
  const int64_t n_blocks = (int64_t)acc.n_blocks;
  const int64_t n_bnd_p = (n_blocks + tor::kPad - 1) / tor::kPad * tor::kPad;          // (per block, as this view reports them)
  const int64_t n_box_p = (int64_t)tor::accel_boxes_padded(acc), F = acc.fanout > 0 ? acc.fanout : 1;
  if (slot_cap < n_blocks * tor::kPad || box_cap < n_bnd_p) return TOR_ERR_INVALID_ARGUMENT;
  for (int64_t k = 0; k < n_blocks * tor::kPad; ++k) {
    int64_t orig = -1;
    if (acc.spatial[(size_t)k].valid) std::memcpy(&orig, &acc.cold[16 * (acc.spatial_base + (size_t)k) + 14], 8);
    slot_object[k] = orig;
  }
  // (a culling box stands for `fanout` consecutive blocks: block b is reported with the box that covers it; a super box covers
  // 8 boxes = 8 F blocks, reported per group of 8 BLOCKS as before -- the super box that covers the group's first block)
  for (int64_t b = 0; b < n_bnd_p; ++b)
    for (int c = 0; c < 6; ++c) block_boxes[6 * b + c] = (b / F < n_box_p) ? bnd[8 * (size_t)(b / F) + c] : std::nan("");
  const int64_t n_super = n_bnd_p / tor::kPad;
  for (int64_t sidx = 0; sidx < n_super; ++sidx)
    for (int c = 0; c < 6; ++c) {
      const int64_t sb = (sidx * tor::kPad / F) / tor::kPad;  // super box of the group's first block
      super_boxes[6 * sidx + c] = sb < n_box_p / tor::kPad ? bnd[8 * (size_t)(n_box_p + 1 + sb) + c] : std::nan("");
    }
  if (two_level_out) *two_level_out = acc.two_level ? 1 : 0;
  return (int)n_blocks;
}

// TOR_ACCEL_F32 self test (host build of tor_filter32.hpp, no device needed): ray i against sphere i.
// keep[i] = the float32 pre-filter's decision; need[i] = the float64 condition it must never miss,
// D > 0 and (half_b < 0 or c < 0) evaluated as spheres.nim:30-33 does (bit 1: a root > 0.001 exists).
int tor_selftest_filter32_host(int64_t n, const double* o, const double* d, const double* c0, const double* dc,
                               const int32_t* moving, const double* f, const double* r2, const double* origin,
                               int32_t* keep, int32_t* need) {
  if (n < 0 || !o || !d || !c0 || !dc || !moving || !f || !r2 || !origin || !keep || !need)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_filter32_host: bad argument");
  for (int64_t i = 0; i < n; ++i) {
    const double* oo = o + 3 * i; const double* dd = d + 3 * i; const double* cc0 = c0 + 3 * i; const double* dcc = dc + 3 * i;
    const bool mv = moving[i] != 0;
    keep[i] = (int32_t)tor::filter_one(oo, dd, cc0, dcc, mv, f[i], r2[i], origin);
    double c[3] = {cc0[0], cc0[1], cc0[2]};
    if (mv) for (int k = 0; k < 3; ++k) c[k] = cc0[k] + dcc[k] * f[i];  // moving_spheres.nim:43
    const double ocx = oo[0] - c[0], ocy = oo[1] - c[1], ocz = oo[2] - c[2];
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
    const double hb = ocx * dd[0] + ocy * dd[1] + ocz * dd[2];
    const double cq = (ocx * ocx + ocy * ocy + ocz * ocz) - r2[i];
    const double disc = hb * hb - a * cq;
    int32_t nd = (disc > 0.0 && (hb < 0.0 || cq < 0.0)) ? 1 : 0;
    if (disc > 0.0) {
      const double root = std::sqrt(disc);
      const double s0 = (-hb - root) / a, s1 = (-hb + root) / a;
      if ((0.001 < s0 && s0 < INFINITY) || (0.001 < s1 && s1 < INFINITY)) nd |= 2;
    }
    need[i] = nd;
  }
  return TOR_OK;
}

// The conservative FMA screen of the strict object loop (tor_screen.hpp) on the HOST: ray i against sphere i, with the
// margins the kernel would use for a segment that holds only this object (the smallest margins the host ever hands out).
// keep[i] = the screen keeps the object; need[i] as in tor_selftest_filter32_host.
int tor_selftest_screen_host(int64_t n, const double* o, const double* d, const double* c0, const double* dc,
                             const int32_t* moving, const double* f, const double* r2, int32_t* keep, int32_t* need) {
  if (n < 0 || !o || !d || !c0 || !dc || !moving || !f || !r2 || !keep || !need)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_screen_host: bad argument");
  auto up = [](double x) { return x * (1.0 + 0x1p-40); };
  for (int64_t i = 0; i < n; ++i) {
    const double* oo = o + 3 * i; const double* dd = d + 3 * i; const double* cc0 = c0 + 3 * i; const double* dcc = dc + 3 * i;
    const bool mv = moving[i] != 0;
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
    // tor_scene.cpp build_layout: segs[6], segs[7]
    const double reach = up(std::sqrt(cc0[0] * cc0[0] + cc0[1] * cc0[1] + cc0[2] * cc0[2]) + std::sqrt(std::fabs(r2[i])));
    const double travel = mv ? up(std::sqrt(dcc[0] * dcc[0] + dcc[1] * dcc[1] + dcc[2] * dcc[2])) : 0.0;
    const double s1 = std::fabs(oo[0]) + std::fabs(oo[1]) + std::fabs(oo[2]);
    const double d1 = std::fabs(dd[0]) + std::fabs(dd[1]) + std::fabs(dd[2]);
    double negmu, am;
    tor::screen_margins(s1 + reach + travel * std::fabs(mv ? f[i] : 0.0), d1, a, negmu, am);
    const double nf = -f[i];
    const double sx = mv ? tor::fma_(nf, dcc[0], oo[0] - cc0[0]) : oo[0] - cc0[0];
    const double sy = mv ? tor::fma_(nf, dcc[1], oo[1] - cc0[1]) : oo[1] - cc0[1];
    const double sz = mv ? tor::fma_(nf, dcc[2], oo[2] - cc0[2]) : oo[2] - cc0[2];
    keep[i] = tor::screen_filter(sx, sy, sz, dd[0], dd[1], dd[2], a, negmu, am, r2[i]) < 0 ? 1 : 0;
    double c[3] = {cc0[0], cc0[1], cc0[2]};
    if (mv) for (int k = 0; k < 3; ++k) c[k] = cc0[k] + dcc[k] * f[i];  // moving_spheres.nim:43
    const double ocx = oo[0] - c[0], ocy = oo[1] - c[1], ocz = oo[2] - c[2];
    const double hb = ocx * dd[0] + ocy * dd[1] + ocz * dd[2];
    const double cq = (ocx * ocx + ocy * ocy + ocz * ocz) - r2[i];
    const double disc = hb * hb - a * cq;
    int32_t nd = (disc > 0.0 && (hb < 0.0 || cq < 0.0)) ? 1 : 0;
    if (disc > 0.0) {
      const double root = std::sqrt(disc);
      const double s0 = (-hb - root) / a, s1r = (-hb + root) / a;
      if ((0.001 < s0 && s0 < INFINITY) || (0.001 < s1r && s1r < INFINITY)) nd |= 2;
    }
    need[i] = nd;
  }
  return TOR_OK;
}

// The SECOND form of the screen (tor_screen.hpp: expanded quadratic, normalised direction) on the host, same conventions as
// tor_selftest_screen_host.  variant 0: a static sphere through the general record (kind 10), a mover along y through kind 12,
// any other mover through the first form (as the kernel does); variant 1: static spheres through the common-height record (kind 11);
// variant 2: every pair through the PLANE screen (stage one) alone -- statics and movers along y by {cx, cz}, movers in general
// position by {c0x, c0z, dcx, dcz} (xkind 13).
int tor_selftest_screen2_host(int64_t n, const double* o, const double* d, const double* c0, const double* dc,
                              const int32_t* moving, const double* f, const double* r2, int32_t variant, int32_t* keep, int32_t* need) {
  if (n < 0 || !o || !d || !c0 || !dc || !moving || !f || !r2 || !keep || !need)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_screen2_host: bad argument");
  int rc = tor_selftest_screen_host(n, o, d, c0, dc, moving, f, r2, keep, need);  // `need`, and `keep` of the pairs that stay on the first form
  if (rc != TOR_OK) return rc;
  auto up = [](double x) { return x * (1.0 + 0x1p-40); };
  for (int64_t i = 0; i < n; ++i) {
    const double* oo = o + 3 * i; const double* dd = d + 3 * i; const double* cc0 = c0 + 3 * i; const double* dcc = dc + 3 * i;
    const bool mv = moving[i] != 0;
    const bool general = mv && !(dcc[0] == 0.0 && dcc[2] == 0.0);
    if (general && variant != 2) continue;
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];  // spheres.nim:30
    const double reach = up(std::sqrt(cc0[0] * cc0[0] + cc0[1] * cc0[1] + cc0[2] * cc0[2]) + std::sqrt(std::fabs(r2[i])));
    const double travel = mv ? up(std::sqrt(dcc[0] * dcc[0] + dcc[1] * dcc[1] + dcc[2] * dcc[2])) : 0.0;
    const tor::ScreenRay ray = tor::screen2_ray(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], a);
    int word;
    if (variant == 2) {  // stage one: the plane screen alone (R = this object's radius); a mover in general position through the 4-fma chain of xkind 13
      const tor::PlaneSeg ps = tor::plane_seg(ray, tor::plane_ray(ray), reach, travel, mv ? f[i] : 0.0, r2[i]);
      word = general ? tor::plane_word_mov(ps, cc0[0], cc0[2], dcc[0], dcc[2]) : tor::plane_word(ps, cc0[0], cc0[2]);
    } else if (mv) {
      const tor::ScreenSeg sg = tor::screen2_seg(ray, reach, travel, cc0[1], f[i]);
      word = tor::screen2_movy_y(sg, cc0[0], cc0[2], tor::screen2_Ky(cc0[0], cc0[2], r2[i]), dcc[1]);
    } else if (variant == 1) {
      const tor::ScreenSeg sg = tor::screen2_seg(ray, reach, 0.0, cc0[1], 0.0);
      word = tor::screen2_static_y(sg, cc0[0], cc0[2], tor::screen2_Ky(cc0[0], cc0[2], r2[i]));
    } else {
      const tor::ScreenSeg sg = tor::screen2_seg(ray, reach, 0.0, 0.0, 0.0);
      word = tor::screen2_static(sg, cc0[0], cc0[1], cc0[2], tor::screen2_K(cc0[0], cc0[1], cc0[2], r2[i]));
    }
    keep[i] = word < 0 ? 1 : 0;
  }
  return TOR_OK;
}

// TOR_ACCEL_F32 on the HOST over a whole scene: builds the same layout tor_scene_upload builds and walks its
// float32 segments (kinds 5/6/7) for each ray exactly as integrate_kernel does (same records, same
// tor_filter32.hpp code).  keep[ray * world.len + object] = 1 kept, 0 dropped, 2 object is on the float64
// loop (not eligible for the filter).  No device needed.
int tor_debug_filter32_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d,
                             const double* time, int8_t* keep) {
  if (world.len < 0 || (world.len > 0 && !world.objects) || n_rays < 0 || !o || !d || !time || !keep)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_filter32_scene: bad argument");
  const tor::F32Options f32 = tor::f32_options_for(world.objects, world.len);
  std::vector<int64_t> ids((size_t)world.len);
  for (int64_t i = 0; i < world.len; ++i) ids[(size_t)i] = i;
  tor::HostLayout lay;
  std::string err;
  if (!tor::build_layout(world.objects, ids, lay, err, &f32)) return fail(TOR_ERR_INVALID_ARGUMENT, err);
  using tor::f2v;
  for (int64_t r = 0; r < n_rays; ++r) {
    int8_t* kr = keep + r * world.len;
    for (int64_t i = 0; i < world.len; ++i) kr[i] = 2;
    const double* oo = o + 3 * r; const double* dd = d + 3 * r;
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
    const tor::RayF32 r32 = tor::make_ray_f32(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], a, f32.origin[0], f32.origin[1], f32.origin[2]);
    for (int s = 0; s < lay.n_segs; ++s) {
      const double* sg = &lay.segs[8 * (size_t)s];
      const int kind = (int)sg[0];
      if (kind < 5) continue;
      const int begin = (int)sg[1], count = (int)sg[2] & 0xffffff, block0 = (int)sg[3];
      const double f64 = kind == 5 ? 0.0 : (time[r] - sg[4]) / sg[5];
      const tor::SegF32 s32 = tor::make_seg_f32(r32, f64, (float)sg[6], (float)sg[7]);
      const int stride = kind == 5 ? 10 : (kind == 6 ? 12 : 16);
      for (int i = 0; i < count; i += tor::kPad) {
        unsigned m = 0;
        for (int j = 0; j < tor::kPad / 2; ++j) {
          const float* rec = &lay.hot32[(size_t)begin + (size_t)(i / 2 + j) * stride];
          const f2v cx = {rec[0], rec[1]}, cy = {rec[2], rec[3]}, cz = {rec[4], rec[5]};
          f2v ocx = tor::oc_static32(r32.ox, cx), ocy = tor::oc_static32(r32.oy, cy), ocz = tor::oc_static32(r32.oz, cz);
          if (kind == 6) ocy = tor::oc_moving32(r32.oy, cy, (f2v){rec[10], rec[11]}, s32.nf);
          if (kind == 7) {
            ocx = tor::oc_moving32(r32.ox, cx, (f2v){rec[10], rec[11]}, s32.nf);
            ocy = tor::oc_moving32(r32.oy, cy, (f2v){rec[12], rec[13]}, s32.nf);
            ocz = tor::oc_moving32(r32.oz, cz, (f2v){rec[14], rec[15]}, s32.nf);
          }
          m = tor::filter_pair32(r32, s32, ocx, ocy, ocz, (f2v){rec[6], rec[7]}, (f2v){rec[8], rec[9]}, m);
        }
        m |= s32.wild;
        for (int j = 0; j < tor::kPad; ++j) {
          const size_t slot = (size_t)(block0 + i / tor::kPad) * tor::kPad + (size_t)j;
          int64_t orig;
          std::memcpy(&orig, &lay.cold[16 * slot + 14], 8);
          const bool padding = lay.cold[16 * slot + 15] < 0.0;
          const int bit = (m >> (7 - j)) & 1;
          if (!padding) kr[orig] = (int8_t)bit;
        }
      }
    }
  }
  return TOR_OK;
}

// The strict brute-force layout's SCREENED segments on the HOST over a whole scene: builds the layout tor_scene_upload builds
// (no float32 segments) and walks its xkinds 10-14 for each ray as integrate_kernel's ARITH 2 loop does when stage one runs --
// the plane screen first (the segment's plane table, its largest radius^2), then the segment's own test on the per-lane record:
// the second form for 10 / 11 / 12 (32 bytes), the first form for 13 / 14 (64 bytes).  keep[ray * world.len + object] = 0 dropped
// by the plane screen, 1 dropped by stage two, 2 a candidate of the exact test, 3 the object is on a segment without a table (a
// time group whose fraction is never finite).  kind_out[object] (nullable) = its segment's xkind (0, 10-14);
// pays_out[ray * n_segs_out + segment] (nullable, with n_segs_out) = plane_pays' vote of that ray.  No device needed.
int tor_debug_layout_segments(TorHittableList world, int32_t* out, int64_t max_segs, int64_t* n_segs_out) {
  if (world.len < 0 || (world.len > 0 && !world.objects) || max_segs < 0 || (max_segs > 0 && !out) || !n_segs_out)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_layout_segments: bad argument");
  std::vector<int64_t> ids((size_t)world.len);
  for (int64_t i = 0; i < world.len; ++i) ids[(size_t)i] = i;
  tor::HostLayout lay;
  std::string err;
  if (!tor::build_layout(world.objects, ids, lay, err, nullptr)) return fail(TOR_ERR_INVALID_ARGUMENT, err);
  *n_segs_out = lay.n_segs;
  for (int s = 0; s < lay.n_segs && s < max_segs; ++s) {
    const double* sg = &lay.segs[8 * (size_t)s];
    const int count = (int)sg[2] & 0xffffff, real = count - ((int)sg[2] >> 24);
    out[4 * s + 0] = (int32_t)lay.xsegs[8 * (size_t)s];
    out[4 * s + 1] = real;
    out[4 * s + 2] = count;
    out[4 * s + 3] = (int32_t)sg[3] * (int32_t)tor::kPad;
  }
  return TOR_OK;
}

int tor_debug_screen2_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d, const double* time, int8_t* keep,
                            int32_t* kind_out, int8_t* pays_out, int64_t n_segs_out) {
  if (world.len < 0 || (world.len > 0 && !world.objects) || n_rays < 0 || !o || !d || !time || !keep)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_screen2_scene: bad argument");
  std::vector<int64_t> ids((size_t)world.len);
  for (int64_t i = 0; i < world.len; ++i) ids[(size_t)i] = i;
  tor::HostLayout lay;
  std::string err;
  if (!tor::build_layout(world.objects, ids, lay, err, nullptr)) return fail(TOR_ERR_INVALID_ARGUMENT, err);
  auto orig_of = [&](size_t slot) {
    int64_t v;
    std::memcpy(&v, &lay.cold[16 * slot + 14], 8);
    return v;
  };
  for (int64_t r = 0; r < n_rays; ++r) {
    int8_t* kr = keep + r * world.len;
    for (int64_t i = 0; i < world.len; ++i) kr[i] = 3;
    const double* oo = o + 3 * r; const double* dd = d + 3 * r;
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];  // spheres.nim:30
    const tor::ScreenRay ray = tor::screen2_ray(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], a);
    const tor::PlaneRay pray = tor::plane_ray(ray);
    for (int s = 0; s < lay.n_segs; ++s) {
      const double* sg = &lay.segs[8 * (size_t)s];
      const double* xs = &lay.xsegs[8 * (size_t)s];
      const int xkind = (int)xs[0];
      const int count = (int)sg[2] & 0xffffff, real = count - ((int)sg[2] >> 24), block0 = (int)sg[3];
      if (r == 0 && kind_out)
        for (int i = 0; i < real; ++i) kind_out[orig_of((size_t)block0 * tor::kPad + (size_t)i)] = xkind;
      if (xkind < 10) continue;
      const double f = xkind >= 12 ? (time[r] - sg[4]) / sg[5] : 0.0;  // moving_spheres.nim:42
      const tor::ScreenSeg ss = tor::screen2_seg(ray, sg[6], sg[7], xs[2], f);
      const tor::PlaneSeg ps = tor::plane_seg(ray, pray, sg[6], sg[7], f, xs[4]);
      double negmu = 0.0, am = 0.0;  // first form (13 / 14): integrate_loop_plane.inc / integrate_loop_f64_movers.inc
      tor::screen_margins(ray.s1 + sg[6] + sg[7] * std::fabs(f), std::fabs(dd[0]) + std::fabs(dd[1]) + std::fabs(dd[2]), a, negmu, am);
      const size_t xsz = xkind >= 13 ? 8 : 4, pw = xkind == 13 ? 4 : 2;
      for (int i = 0; i < real; ++i) {
        const double* x = &lay.xrec[(size_t)xs[1] + xsz * (size_t)i];
        const double* pl = &lay.xpl[(size_t)xs[3] + pw * (size_t)i];
        const bool table_ok = xkind == 10   ? (pl[0] == x[0] && pl[1] == x[2])
                              : xkind <= 12 ? (pl[0] == x[0] && pl[1] == x[1])
                              : xkind == 13 ? (pl[0] == x[0] && pl[1] == x[2] && pl[2] == x[4] && pl[3] == x[6])
                                            : (pl[0] == x[0] && pl[1] == x[2] && x[4] == 0.0 && x[6] == 0.0);
        if (!table_ok) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_screen2_scene: the plane table and the records disagree (layout bug)");
        int8_t verdict;
        const int w1 = xkind == 13 ? tor::plane_word_mov(ps, pl[0], pl[1], pl[2], pl[3]) : tor::plane_word(ps, pl[0], pl[1]);
        if (w1 >= 0) {
          verdict = 0;
        } else {
          int w2;
          if (xkind == 10) w2 = tor::screen2_static(ss, x[0], x[1], x[2], x[3]);
          else if (xkind == 11) w2 = tor::screen2_static_y(ss, x[0], x[1], x[2]);
          else if (xkind == 12) w2 = tor::screen2_movy_y(ss, x[0], x[1], x[2], x[3]);
          else w2 = tor::screen_filter(tor::fma_(-f, x[4], oo[0] - x[0]), tor::fma_(-f, x[5], oo[1] - x[1]), tor::fma_(-f, x[6], oo[2] - x[2]), dd[0], dd[1], dd[2], a, negmu, am, x[3]);
          verdict = w2 < 0 ? 2 : 1;
        }
        kr[orig_of((size_t)block0 * tor::kPad + (size_t)i)] = verdict;
      }
      if (pays_out && s < n_segs_out) pays_out[r * n_segs_out + s] = tor::plane_pays(pray, 4.0 * tor::kPlaneGate * tor::kPlaneGate, xs[4], xs[5], xs[6]) ? 1 : 0;
    }
  }
  return TOR_OK;
}

// Stage one in float32 against the float64 plane screen over a whole scene on the HOST (include/tor_render.h): the layout and the
// segment headers tor_scene_upload builds, PlaneSeg32 from the header's slots exactly as kernel/integrate_loop_plane.inc reads them.
int tor_debug_plane32_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d, const double* time, int8_t* keep,
                            int32_t* pad_kept, int64_t* n_pad_out) {
  if (world.len < 0 || (world.len > 0 && !world.objects) || n_rays < 0 || !o || !d || !time || !keep || !pad_kept || !n_pad_out)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_plane32_scene: bad argument");
  std::vector<int64_t> ids((size_t)world.len);
  for (int64_t i = 0; i < world.len; ++i) ids[(size_t)i] = i;
  tor::HostLayout lay;
  std::string err;
  if (!tor::build_layout(world.objects, ids, lay, err, nullptr)) return fail(TOR_ERR_INVALID_ARGUMENT, err);
  auto orig_of = [&](size_t slot) {
    int64_t v;
    std::memcpy(&v, &lay.cold[16 * slot + 14], 8);
    return v;
  };
  *n_pad_out = 0;
  for (int s = 0; s < lay.n_segs; ++s) {
    const double* sg = &lay.segs[8 * (size_t)s];
    const int xkind = (int)lay.xsegs[8 * (size_t)s];
    if (xkind >= 10 && xkind != 13) *n_pad_out += ((int)sg[2] >> 24);
  }
  for (int64_t r = 0; r < n_rays; ++r) {
    int8_t* kr = keep + r * world.len;
    for (int64_t i = 0; i < world.len; ++i) kr[i] = -1;
    pad_kept[r] = 0;
    const double* oo = o + 3 * r; const double* dd = d + 3 * r;
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];  // spheres.nim:30
    const tor::ScreenRay ray = tor::screen2_ray(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], a);
    const tor::PlaneRay pray = tor::plane_ray(ray);
    for (int s = 0; s < lay.n_segs; ++s) {
      const double* sg = &lay.segs[8 * (size_t)s];
      const double* xs = &lay.xsegs[8 * (size_t)s];
      const double* h = &lay.xhdr[16 * (size_t)s];
      const int xkind = (int)xs[0];
      if (xkind < 10 || xkind == 13) continue;
      const int count = (int)sg[2] & 0xffffff, real = count - ((int)sg[2] >> 24), block0 = (int)sg[3];
      const double f = xkind >= 12 ? (time[r] - sg[4]) / sg[5] : 0.0;  // moving_spheres.nim:42
      const tor::PlaneSeg ps = tor::plane_seg(ray, pray, sg[6], sg[7], f, xs[4]);
      float first[2], ec[2];
      std::memcpy(first, &h[12], 8);
      std::memcpy(ec, &h[15], 8);
      const tor::PlaneSeg32 ps32 = tor::plane_seg32(ray, ps, h[13], h[14], (double)ec[0], (double)ec[1]);
      for (int i = 0; i < count; ++i) {
        const float* pl32 = &lay.xpl32[(size_t)xs[3] + 2 * (size_t)i];
        if (i == 0 && !(pl32[0] == first[0] && pl32[1] == first[1]))
          return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_plane32_scene: the header's first record and the table disagree (layout bug)");
        const bool k32 = tor::plane_word32(ps32, pl32[0], pl32[1]) < 0;
        if (i >= real) {
          pad_kept[r] += k32 ? 1 : 0;
          continue;
        }
        const double* pl = &lay.xpl[(size_t)xs[3] + 2 * (size_t)i];
        const bool k64 = tor::plane_word(ps, pl[0], pl[1]) < 0;
        kr[orig_of((size_t)block0 * tor::kPad + (size_t)i)] = (int8_t)((k64 ? 1 : 0) | (k32 ? 2 : 0));
      }
    }
  }
  return TOR_OK;
}

// The reach pass over a whole scene on the HOST (include/tor_reach.h): the layout, the headers and the word records
// tor_scene_upload builds; PlaneSeg32 and ReachRay from them exactly as kernel/integrate_loop_plane.inc makes them.
int tor_debug_reach_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d, const double* time, int8_t* reach,
                          int32_t* word_out, int32_t* slot_out, double* boxes_out, int64_t max_words, int64_t* n_words_out) {
  if (world.len < 0 || (world.len > 0 && !world.objects) || n_rays < 0 || !o || !d || !time || !reach || max_words < 0 || (max_words > 0 && !boxes_out))
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_reach_scene: bad argument");
  std::vector<int64_t> ids((size_t)world.len);
  for (int64_t i = 0; i < world.len; ++i) ids[(size_t)i] = i;
  tor::HostLayout lay;
  std::string err;
  if (!tor::build_layout(world.objects, ids, lay, err, nullptr)) return fail(TOR_ERR_INVALID_ARGUMENT, err);
  auto orig_of = [&](size_t slot) {
    int64_t v;
    std::memcpy(&v, &lay.cold[16 * slot + 14], 8);
    return v;
  };
  const size_t n_words = (lay.n_sorted + 31) / 32;
  if (n_words_out) *n_words_out = (int64_t)n_words;
  // a word's record, and whether it carries a box: (-inf, +inf) in x says it does not
  auto rec_of = [&](size_t w) { return &lay.xwb[w * (size_t)tor::kReachRecFloats]; };
  auto boxed = [&](size_t w) { return !(rec_of(w)[0] == -INFINITY && rec_of(w)[1] == INFINITY); };
  for (int64_t i = 0; i < world.len; ++i) {
    if (word_out) word_out[i] = -1;
    if (slot_out) slot_out[i] = -1;
  }
  for (size_t w = 0; w < n_words && (int64_t)w < max_words; ++w) {
    double* b = boxes_out + 6 * w;
    b[0] = b[2] = b[4] = -INFINITY; b[1] = b[3] = b[5] = INFINITY;
  }
  for (int64_t r = -1; r < n_rays; ++r) {  // (r = -1: the tables that do not depend on the ray)
    const double* oo = o + 3 * (r < 0 ? 0 : r); const double* dd = d + 3 * (r < 0 ? 0 : r);
    tor::ScreenRay ray{};
    tor::PlaneRay pray{};
    if (r >= 0) {
      const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];  // spheres.nim:30
      ray = tor::screen2_ray(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], a);
      pray = tor::plane_ray(ray);
      for (int64_t i = 0; i < world.len; ++i) reach[r * world.len + i] = 1;
    }
    for (int s = 0; s < lay.n_segs; ++s) {
      const double* sg = &lay.segs[8 * (size_t)s];
      const double* xs = &lay.xsegs[8 * (size_t)s];
      const double* h = &lay.xhdr[16 * (size_t)s];
      const int xkind = (int)xs[0];
      if ((int)sg[0] > 2) continue;  // (the float32 pre-filter's segments: not part of the float64 list's screens)
      const int count = (int)sg[2] & 0xffffff, real = count - ((int)sg[2] >> 24), block0 = (int)sg[3];
      const size_t slot0 = (size_t)block0 * tor::kPad;
      if (r < 0) {
        for (int i = 0; i < real; ++i) {
          const size_t slot = slot0 + (size_t)i, w = slot / 32;
          const int64_t obj = orig_of(slot);
          if (slot_out) slot_out[obj] = (int32_t)slot;
          if (word_out && xkind >= 10 && xkind != 13 && boxed(w)) word_out[obj] = (int32_t)w;
        }
        for (size_t w = (slot0 + 31) / 32; xkind >= 10 && xkind != 13 && 32 * (w + 1) <= slot0 + (size_t)count; ++w) {
          if (!boxed(w) || (int64_t)w >= max_words) continue;
          const float* rec = rec_of(w);
          double* b = boxes_out + 6 * w;
          b[0] = (double)rec[0] + h[13]; b[1] = (double)rec[1] + h[13]; b[2] = (double)rec[2] + h[14]; b[3] = (double)rec[3] + h[14];
          std::memcpy(&b[4], rec + 4, 16);
        }
        continue;
      }
      if (xkind < 10 || xkind == 13) continue;
      const double f = xkind >= 12 ? (time[r] - sg[4]) / sg[5] : 0.0;  // moving_spheres.nim:42
      const tor::PlaneSeg ps = tor::plane_seg(ray, pray, sg[6], sg[7], f, xs[4]);
      float ec[2];
      std::memcpy(ec, &h[15], 8);
      const tor::PlaneSeg32 ps32 = tor::plane_seg32(ray, ps, h[13], h[14], (double)ec[0], (double)ec[1]);
      // (every word of a segment carries the segment's slab; the kernel reads it from the first word of a pass)
      for (size_t w = (slot0 + 31) / 32; 32 * (w + 1) <= slot0 + (size_t)count; ++w) {
        const float* rec = rec_of(w);
        double slab[2];
        std::memcpy(slab, rec + 4, 16);
        const tor::ReachRay rr = tor::reach_ray(ray, !(ps32.T < INFINITY), ray.s1 + sg[6] + sg[7] * std::fabs(f), h[13], h[14], slab[0], slab[1], f);
        if (!tor::reach_miss(rr, rec[0], rec[1], rec[2], rec[3])) continue;
        if (!boxed(w)) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_reach_scene: a word without a box was not reached (reach pass bug)");
        for (size_t slot = 32 * w; slot < 32 * (w + 1) && slot < slot0 + (size_t)real; ++slot) reach[r * world.len + orig_of(slot)] = 0;
      }
    }
  }
  return TOR_OK;
}

int tor_debug_last_reach(TorContext* ctx, uint64_t out[2]) {
  if (!ctx || !out) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_last_reach: NULL argument");
  if (!ctx->collect_stats) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_debug_last_reach: stats not enabled");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long h[2];
  // words 12, 13 of the launch's counter slot (= KParams.stats + 11, + 12): kernel/integrate_loop_plane.inc
  HIP_TRY(hipMemcpy(h, (unsigned long long*)ctx->counters.ptr + (size_t)ctx->last_slot * TorContext::kSlotWords + 12, sizeof h, hipMemcpyDeviceToHost));
  out[0] = h[0]; out[1] = h[1];
  return TOR_OK;
}

// Float32 slab test of the culling boxes on the HOST (same source as the kernel): ray i against box i.
// keep[i] = slab_bit32 on the float32 record block_bounds_f32 makes of the box; need[i] = the float64 slab test
// of the kernel's float64 path on the same box.  Correct iff need implies keep.
int tor_selftest_slab32_host(int64_t n, const double* o, const double* d, const double* lo, const double* hi,
                             const double* origin, int32_t* keep, int32_t* need) {
  if (n < 0 || !o || !d || !lo || !hi || !origin || !keep || !need)
    return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_slab32_host: bad argument");
  std::vector<double> bnd((size_t)n * 8, 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) { bnd[8 * i + k] = lo[3 * i + k]; bnd[8 * i + 3 + k] = hi[3 * i + k]; }
  std::vector<float> bnd32;
  float hmin = 0.0f;
  const float bmax = tor::block_bounds_f32(bnd, origin, bnd32, &hmin);
  using tor::f2v;
  for (int64_t i = 0; i < n; ++i) {
    const double* oo = o + 3 * i; const double* dd = d + 3 * i;
    const double a = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2];
    const tor::RayF32 r = tor::make_ray_f32(oo[0], oo[1], oo[2], dd[0], dd[1], dd[2], a, origin[0], origin[1], origin[2]);
    const tor::BoxRay32 b = tor::make_box_ray32(r, bmax, hmin);
    const float* rec = &bnd32[8 * (size_t)i];
    keep[i] = (int32_t)(tor::slab_bit32(b, (f2v){rec[0], rec[1]}, (f2v){rec[2], rec[3]}, (f2v){rec[4], rec[5]}) | (r.wild & 1u));
    const double ix = 1.0 / dd[0], iy = 1.0 / dd[1], iz = 1.0 / dd[2];
    const double* c = &bnd[8 * (size_t)i];
    const double tx0 = (c[0] - oo[0]) * ix, tx1 = (c[3] - oo[0]) * ix;
    const double ty0 = (c[1] - oo[1]) * iy, ty1 = (c[4] - oo[1]) * iy;
    const double tz0 = (c[2] - oo[2]) * iz, tz1 = (c[5] - oo[2]) * iz;
    const double t_in = std::fmax(std::fmax(std::fmin(tx0, tx1), std::fmin(ty0, ty1)), std::fmax(std::fmin(tz0, tz1), 0.0));
    const double t_out = std::fmin(std::fmin(std::fmax(tx0, tx1), std::fmax(ty0, ty1)), std::fmax(tz0, tz1));
    need[i] = (t_in <= t_out) ? 1 : 0;
  }
  return TOR_OK;
}

// ---- self tests -----------------------------------------------------------------------------

int tor_selftest_math_host(int32_t op, const double* x, const double* y, double* out0, double* out1,
                           int64_t n) {
  if (!x || !out0 || n < 0) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_math_host: bad argument");
  for (int64_t i = 0; i < n; ++i) {
    double a = 0, b = 0;
    tor::selftest_math_one(op, x[i], y ? y[i] : 0.0, a, b);
    out0[i] = a;
    if (out1) out1[i] = b;
  }
  return TOR_OK;
}

int tor_selftest_math_device(int32_t op, const double* x, const double* y, double* out0, double* out1,
                             int64_t n, int32_t device) {
  if (!x || !out0 || n < 0) return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_math_device: bad argument");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) return fail(TOR_ERR_NO_DEVICE, "no HIP device available");
  if (device >= 0) HIP_TRY(hipSetDevice(device));
  const size_t bytes = (size_t)n * 8;
  DeviceBuffer bx, by, b0, b1;  // released on every path
  struct Release {
    DeviceBuffer *a, *b, *c, *d;
    ~Release() { a->release(); b->release(); c->release(); d->release(); }
  } release{&bx, &by, &b0, &b1};
  HIP_TRY(bx.ensure(bytes + 8));
  HIP_TRY(by.ensure(bytes + 8));
  HIP_TRY(b0.ensure(bytes + 8));
  HIP_TRY(b1.ensure(bytes + 8));
  HIP_TRY(hipMemcpy(bx.ptr, x, bytes, hipMemcpyHostToDevice));
  if (y) HIP_TRY(hipMemcpy(by.ptr, y, bytes, hipMemcpyHostToDevice));
  else HIP_TRY(hipMemset(by.ptr, 0, bytes));
  HIP_TRY(hipMemset(b0.ptr, 0, bytes));
  HIP_TRY(hipMemset(b1.ptr, 0, bytes));
  HIP_TRY(tor::launch_selftest(op, (const double*)bx.ptr, (const double*)by.ptr, (double*)b0.ptr, (double*)b1.ptr, n, nullptr));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out0, b0.ptr, bytes, hipMemcpyDeviceToHost));
  if (out1) HIP_TRY(hipMemcpy(out1, b1.ptr, bytes, hipMemcpyDeviceToHost));
  return TOR_OK;
}

int tor_selftest_rng_host(int32_t mode, uint64_t a, uint64_t b, uint64_t c, uint64_t state_out[4],
                          uint64_t* draws_out, int64_t n) {
  tor::Rng g{0, 0, 0, 0};
  if (mode == 1) tor::seed1(g, a);
  else if (mode == 2) tor::seed2(g, a, b);
  else if (mode == 3) tor::seed3(g, a, b, c);
  else return fail(TOR_ERR_INVALID_ARGUMENT, "tor_selftest_rng_host: mode must be 1, 2 or 3");
  if (state_out) { state_out[0] = g.s0; state_out[1] = g.s1; state_out[2] = g.s2; state_out[3] = g.s3; }
  for (int64_t i = 0; i < n && draws_out; ++i) draws_out[i] = tor::next(g);
  return TOR_OK;
}

}  // extern "C"
