// tor_query.hip -- batched closest-hit queries against the uploaded scene (tor_hit_device / tor_hit_host, include/tor_render.h):
// the reference's HittableList.hit (hittables_lists.nim:48-55 over spheres.nim:28-49 / moving_spheres.nim:39-67) for rays the
// caller supplies, on gfx950.  Kernels, parameter struct and entry points of their own: nothing here is shared with the integrator
// (tor_kernels.hip, KParams, kernel/*.inc), whose kernels stay as they are.  The exact test, the slab test, the descent and the host
// setup live in tor_query.hpp / tor_query_descent.inc, shared with the radiance queries (tor_radiance.hip).
//
// The sequential `closest_so_far` loop is order independent.  An object replaces the record iff its accepted root in (t_min, t_max)
// -- the first root if it lies in the interval, else the second -- is below the closest so far: the first root is never larger than
// the second, so a root rejected only by closest_so_far can never win.  The result is the smallest accepted root over all objects,
// ties to the lowest ORIGINAL index, whatever order the objects are visited in and whichever objects are skipped because they cannot
// be hit.  The record (p, normal, front_face) is then built once, for the winner, with the reference's operations.
//
//   hit_kernel<false>  brute force: one ray per lane; every cold slot of the flat layout in a wave-uniform loop (scalar loads)
//   hit_kernel<true>   blocks: the culling layout's always-objects in the same loop; then per lane a float64 slab test of the block
//                      boxes (two-level scenes: the super boxes, then the 8 block boxes of each super box entered) and the exact test for
//                      the 8 objects of every block entered.  A ray the boxes cannot answer for walks every spatial slot instead:
//                      its time lies outside the range the boxes were built for (or is NaN), its t_min is not >= 0 (the slab test
//                      clips at 0), or its origin lies beyond the reach of the boxes' margin (below).
//   hit_masked_kernel<>  the same two with visibility groups (tor_scene_groups): object j takes part for ray i iff groups[j] &
//                      mask_i != 0.  The order independence above is what makes this exact: the closest hit over the objects a ray sees
//                      is the sequential loop on the sub-list of those objects, ties to the lowest index among them.  Skipping a box
//                      whose OR-word shares no bit with the ray's mask skips only objects the ray does not see.
//
// Why the boxes' margin needs a reach.  The reference's own test rounds: disc = half_b^2 - a * c carries an absolute error of at most
// ~12 eps |d|^2 (|oc|^2 + r^2) (eps = 2^-53; half_b^2 and a * c each within 5 roundings, then the difference), and the exact value is
// |d|^2 (r^2 - dist^2), dist = the distance from the centre to the ray's line.  So the reference can accept a ray whose line passes up
// to 6 eps (|oc|^2 + r^2) / r OUTSIDE the sphere -- negligible near the scene, but 2.8e-6 for r = 0.2 at |oc| = 1e5.  Such a hit
// lies in the object's box only while that excess stays below the box's inflation (compute_block_bounds: at least 1e-6).  The host
// derives a radius `reach` around the spatial objects' bounding box within which 16 eps (|oc|^2 + r_max^2) / r_min <= 1e-6 / 4
// (hit_reach), and a floor for a = |d|^2 above which no product of the test underflows enough to matter; rays outside either walk.
//
// Float64, unfused (-ffp-contract=off), correctly rounded division and square root: the integrator's exactness contract.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "tor_context.hpp"
#include "tor_query.hpp"

static_assert(sizeof(TorRay) == 56 && offsetof(TorRay, direction) == 24 && offsetof(TorRay, time) == 48,
              "TorRay: origin, direction, time (primitives/rays.nim)");
static_assert(sizeof(TorHit) == 64 && offsetof(TorHit, normal) == 24 && offsetof(TorHit, t) == 48 && offsetof(TorHit, object) == 56 &&
                  offsetof(TorHit, front_face) == 60,
              "TorHit: HitRecord (physics/core.nim:30-36) with the object index in place of the material");

namespace tor {
namespace {

template <bool BLOCKS>
__global__ __launch_bounds__(kHitThreads) void hit_kernel(const QParams p) {
  const long long i = (long long)blockIdx.x * kHitThreads + threadIdx.x;
  const bool live = i < p.n_rays;
  QRay r{};  // (lanes past the end: t_max = 0 accepts nothing)
  if (live) {
    const double* q = p.rays + 7 * i;
    r.ox = q[0]; r.oy = q[1]; r.oz = q[2];
    r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
    r.time = q[6];
    if (p.t_range) {
      r.t_min = p.t_range[2 * i];
      r.t_max = p.t_range[2 * i + 1];
    } else {
      r.t_min = 0.001;  // render.nim:34
      r.t_max = __builtin_inf();
    }
  }
  r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30 r.direction.length_squared()
  QBest b{r.t_max, INT_MAX, -1};
#include "tor_query_descent.inc"
  if (!live) return;
  double* o = p.hits + 8 * i;
  if (b.slot < 0) {  // miss: object -1, every other field 0
    for (int k = 0; k < 7; ++k) o[k] = 0.0;
    o[7] = __longlong_as_double((long long)0xffffffffull);
    return;
  }
  const qgdptr c = (qgdptr)(uintptr_t)(p.cold + 16 * (size_t)b.slot);
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);
  const double t = b.t;
  const double px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t;  // rays.nim:24-25 origin + t * direction
  const double inv_r = c[6];                                                     // vec3s.nim:93-94: `/ radius` is `* (1.0 / radius)`
  double nx = (px - cx) * inv_r, ny = (py - cy) * inv_r, nz = (pz - cz) * inv_r;
  const bool front = (r.dx * nx + r.dy * ny + r.dz * nz) < 0.0;  // core.nim:47-49
  if (!front) {
    nx = -nx; ny = -ny; nz = -nz;
  }
  o[0] = px; o[1] = py; o[2] = pz;
  o[3] = nx; o[4] = ny; o[5] = nz;
  o[6] = t;
  o[7] = __longlong_as_double((long long)(((unsigned long long)(front ? 1u : 0u) << 32) | (unsigned)b.orig));
}

// hit_kernel with visibility groups.  A kernel of its own, statement for statement hit_kernel's but for `vis`: sharing the body
// through a function or a second template parameter changes hit_kernel's name or its register allocation, and the unmasked kernels
// stay byte-identical.
template <bool BLOCKS>
__global__ __launch_bounds__(kHitThreads) void hit_masked_kernel(const QParams p, const MParams mk) {
  const long long i = (long long)blockIdx.x * kHitThreads + threadIdx.x;
  const bool live = i < p.n_rays;
  unsigned r_mask = 0u;  // (lanes past the end see nothing)
  if (live) r_mask = mk.ray_mask ? mk.ray_mask[i] : mk.mask;
  const Sees<true> vis{mk.grp, mk.box_or, r_mask};  // the descent's `vis`
  QRay r{};  // (lanes past the end: t_max = 0 accepts nothing)
  if (live) {
    const double* q = p.rays + 7 * i;
    r.ox = q[0]; r.oy = q[1]; r.oz = q[2];
    r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
    r.time = q[6];
    if (p.t_range) {
      r.t_min = p.t_range[2 * i];
      r.t_max = p.t_range[2 * i + 1];
    } else {
      r.t_min = 0.001;  // render.nim:34
      r.t_max = __builtin_inf();
    }
  }
  r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30 r.direction.length_squared()
  QBest b{r.t_max, INT_MAX, -1};
#include "tor_query_descent.inc"
  if (!live) return;
  double* o = p.hits + 8 * i;
  if (b.slot < 0) {  // miss: object -1, every other field 0
    for (int k = 0; k < 7; ++k) o[k] = 0.0;
    o[7] = __longlong_as_double((long long)0xffffffffull);
    return;
  }
  const qgdptr c = (qgdptr)(uintptr_t)(p.cold + 16 * (size_t)b.slot);
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);
  const double t = b.t;
  const double px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t;  // rays.nim:24-25 origin + t * direction
  const double inv_r = c[6];                                                     // vec3s.nim:93-94: `/ radius` is `* (1.0 / radius)`
  double nx = (px - cx) * inv_r, ny = (py - cy) * inv_r, nz = (pz - cz) * inv_r;
  const bool front = (r.dx * nx + r.dy * ny + r.dz * nz) < 0.0;  // core.nim:47-49
  if (!front) {
    nx = -nx; ny = -ny; nz = -nz;
  }
  o[0] = px; o[1] = py; o[2] = pz;
  o[3] = nx; o[4] = ny; o[5] = nz;
  o[6] = t;
  o[7] = __longlong_as_double((long long)(((unsigned long long)(front ? 1u : 0u) << 32) | (unsigned)b.orig));
}

}  // namespace

HitQueryState::~HitQueryState() {
  bnd.release();
  io.release();
  head.release();
  obj_cold.release();
  sel.release();
  grp[0].release();
  grp[1].release();
  if (ev_done) (void)hipEventDestroy(ev_done);
}

}  // namespace tor

namespace {

constexpr int64_t kMaxHitRays = (int64_t)0x7fffffff * tor::kHitThreads;  // one lane per ray, at most 2^31 - 1 workgroups

// every check that needs no device and does not read *ctx (the CPU suite runs these)
int hit_args(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, double time_lo, double time_hi, int32_t mode,
             const void* hits) {
  using tor::fail;
  const std::string w = who;
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (n_rays < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_rays < 0");
  if (n_rays > kMaxHitRays) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_rays above 2^31 - 1 workgroups of 256 rays");
  if (!std::isfinite(time_lo) || !std::isfinite(time_hi) || time_lo > time_hi)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the time range must be finite with time_lo <= time_hi");
  if (mode < TOR_HIT_AUTO || mode > TOR_HIT_BLOCKS)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": mode must be TOR_HIT_AUTO (0), TOR_HIT_BRUTE (1) or TOR_HIT_BLOCKS (2)");
  if (n_rays > 0 && (!rays || !hits)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays or hits");
  return TOR_OK;
}

// the launch; the arguments are checked and n_rays > 0.  masked: with the visibility groups and d_mask / mask (tor_hit_masked_device)
int hit_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, double time_lo,
               double time_hi, int32_t mode, void* d_hits, hipStream_t stream, bool masked = false, const uint32_t* d_mask = nullptr,
               uint32_t mask = 0) {
  tor::HitQueryState& hq = ctx->hitq;
  tor::QParams p{};
  bool blocks = false;
  std::string why;
  const int rc = tor::query_setup(who, ctx, time_lo, time_hi, mode, stream, p, blocks, why);
  if (rc != TOR_OK) return rc;
  p.rays = (const double*)d_rays;
  p.t_range = d_t_range;
  p.hits = (double*)d_hits;
  p.n_rays = (long long)n_rays;
  const unsigned grid = (unsigned)((n_rays + tor::kHitThreads - 1) / tor::kHitThreads);
  if (masked) {
    tor::MParams mk{};
    const int rm = tor::masked_setup(ctx, blocks, d_mask, mask, stream, mk);
    if (rm != TOR_OK) return rm;
    if (blocks) hipLaunchKernelGGL(tor::hit_masked_kernel<true>, dim3(grid), dim3(tor::kHitThreads), 0, stream, p, mk);
    else hipLaunchKernelGGL(tor::hit_masked_kernel<false>, dim3(grid), dim3(tor::kHitThreads), 0, stream, p, mk);
  } else if (blocks) {
    hipLaunchKernelGGL(tor::hit_kernel<true>, dim3(grid), dim3(tor::kHitThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL(tor::hit_kernel<false>, dim3(grid), dim3(tor::kHitThreads), 0, stream, p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(hq.ev_done, stream));
  hq.launched = true;
  hq.stream = (void*)stream;
  const std::string what = masked ? "hit (masked): " : "hit: ";
  tor::set_last_note(blocks ? what + "blocks" : what + "brute force" + (why.empty() ? std::string() : " (" + why + ")"));
  return TOR_OK;
}

// tor_hit_host / tor_hit_masked_host (masks: nullable host words, staged behind the records)
int hit_host(const char* who, TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo, double time_hi,
             int32_t mode, TorHit* hits, bool masked, const uint32_t* masks, uint32_t mask) {
  int rc = hit_args(who, ctx, n_rays, rays, time_lo, time_hi, mode, hits);
  if (rc != TOR_OK) return rc;
  if (!ctx->scene_ready) return tor::fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": no scene uploaded");
  if (n_rays == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  // copy in, the device query on the default stream, copy out (blocking)
  const size_t ray_bytes = (size_t)n_rays * sizeof(TorRay), range_bytes = t_range ? (size_t)n_rays * 16 : 0;
  const size_t hit_bytes = (size_t)n_rays * sizeof(TorHit), mask_bytes = masked && masks ? (size_t)n_rays * 4 : 0;
  tor::HitQueryState& hq = ctx->hitq;
  // blocking entry: it waits for the context's last render launch and last query, on whatever stream they run, where the
  // asynchronous entry would refuse a different stream (the staging buffer below may be reallocated too)
  if (ctx->launches > 0) HIP_TRY(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));
  HIP_TRY(hq.io.ensure(ray_bytes + range_bytes + hit_bytes + mask_bytes));
  char* base = (char*)hq.io.ptr;
  char* d_masks = base + ray_bytes + range_bytes + hit_bytes;  // (every part before it is a multiple of 8 bytes)
  HIP_TRY(hipMemcpy(base, rays, ray_bytes, hipMemcpyHostToDevice));
  if (t_range) HIP_TRY(hipMemcpy(base + ray_bytes, t_range, range_bytes, hipMemcpyHostToDevice));
  if (mask_bytes) HIP_TRY(hipMemcpy(d_masks, masks, mask_bytes, hipMemcpyHostToDevice));
  rc = hit_launch(who, ctx, n_rays, base, t_range ? (const double*)(base + ray_bytes) : nullptr, time_lo, time_hi, mode,
                  base + ray_bytes + range_bytes, nullptr, masked, mask_bytes ? (const uint32_t*)d_masks : nullptr, mask);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipMemcpy(hits, base + ray_bytes + range_bytes, hit_bytes, hipMemcpyDeviceToHost));
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_hit_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo, double time_hi,
                   int32_t mode, TorHit* d_hits, void* hip_stream) {
  int rc = hit_args("tor_hit_device", ctx, n_rays, d_rays, time_lo, time_hi, mode, d_hits);
  if (rc != TOR_OK) return rc;
  if (!ctx->scene_ready) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_hit_device: no scene uploaded");
  if (n_rays == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  return hit_launch("tor_hit_device", ctx, n_rays, d_rays, d_t_range, time_lo, time_hi, mode, d_hits, (hipStream_t)hip_stream);
}

int tor_hit_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo, double time_hi,
                 int32_t mode, TorHit* hits) {
  return hit_host("tor_hit_host", ctx, n_rays, rays, t_range, time_lo, time_hi, mode, hits, false, nullptr, 0);
}

int tor_hit_masked_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo, double time_hi,
                          int32_t mode, TorHit* d_hits, void* hip_stream, const uint32_t* d_mask, uint32_t mask) {
  int rc = hit_args("tor_hit_masked_device", ctx, n_rays, d_rays, time_lo, time_hi, mode, d_hits);
  if (rc != TOR_OK) return rc;
  if (!ctx->scene_ready) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_hit_masked_device: no scene uploaded");
  if (n_rays == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  return hit_launch("tor_hit_masked_device", ctx, n_rays, d_rays, d_t_range, time_lo, time_hi, mode, d_hits, (hipStream_t)hip_stream,
                    true, d_mask, mask);
}

int tor_hit_masked_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo, double time_hi,
                        int32_t mode, TorHit* hits, const uint32_t* masks, uint32_t mask) {
  return hit_host("tor_hit_masked_host", ctx, n_rays, rays, t_range, time_lo, time_hi, mode, hits, true, masks, mask);
}

int tor_scene_groups(TorContext* ctx, int64_t n_objects, const uint32_t* groups) {
  if (!ctx) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_groups: ctx is NULL");
  if (!ctx->scene_ready) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_groups: no scene uploaded");
  if (n_objects != ctx->n_objects)
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_scene_groups: n_objects must be the uploaded list's length (" +
                                                   std::to_string(ctx->n_objects) + ")");
  tor::HitQueryState& hq = ctx->hitq;
  if (hq.launched) {  // the last query may still read the words on the device and their host copy
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(hq.ev_done));
  }
  if (groups) hq.groups.assign(groups, groups + n_objects);
  else hq.groups.clear();
  hq.groups_gen += 1;  // the per-layout words are built again by the next masked query (masked_setup)
  return TOR_OK;
}

}  // extern "C"
