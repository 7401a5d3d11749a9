// tor_shade.hpp -- what the kernels that scatter a ray share: radiance_kernel (tor_radiance.hip) and the path-step kernels
// bounce_kernel / scatter_kernel (tor_bounce.hip).  The scatter itself is tor_shade_scatter.inc, a textual include (as
// tor_query_descent.inc is: a function call in its place changes radiance_kernel's register allocation).
#pragma once

#include "tor_device.hpp"
#include "tor_query.hpp"

namespace tor {
namespace {

__device__ __forceinline__ void set_ray(QRay& r, V3 o, V3 d) {
  r.ox = o.x; r.oy = o.y; r.oz = o.z;
  r.dx = d.x; r.dy = d.y; r.dz = d.z;
}

}  // namespace
}  // namespace tor
