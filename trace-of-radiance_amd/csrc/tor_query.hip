// tor_query.hip -- batched closest-hit queries against the uploaded scene (tor_hit_device / tor_hit_host, include/tor_render.h):
// the reference's HittableList.hit (hittables_lists.nim:48-55 over spheres.nim:28-49 / moving_spheres.nim:39-67) for rays the
// caller supplies, on gfx950.  Kernels, parameter struct and entry points of their own: nothing here is shared with the integrator
// (tor_kernels.hip, KParams, kernel/*.inc), whose kernels stay as they are.  The exact test, the slab test, the descent, the record
// and the host glue live in tor_query.hpp / tor_query_descent.inc / tor_query_record.inc, shared with the other query families.
//
// The sequential `closest_so_far` loop is order independent.  An object replaces the record iff its accepted root in (t_min, t_max)
// -- the first root if it lies in the interval, else the second -- is below the closest so far: the first root is never larger than
// the second, so a root rejected only by closest_so_far can never win.  The result is the smallest accepted root over all objects,
// ties to the lowest ORIGINAL index, whatever order the objects are visited in and whichever objects are skipped because they cannot
// be hit.  The record (p, normal, front_face) is then built once, for the winner, with the reference's operations.
//
//   hit_kernel<false, MASKED>  brute force: one ray per lane; every cold slot of the flat layout in a wave-uniform loop (scalar loads)
//   hit_kernel<true, MASKED>   blocks: the culling layout's always-objects in the same loop; then per lane a float64 slab test of the
//                      block boxes (two-level scenes: the super boxes, then the 8 block boxes of each super box entered) and the exact
//                      test for the 8 objects of every block entered.  A ray the boxes cannot answer for walks every spatial slot
//                      instead: its time lies outside the range the boxes were built for (or is NaN), its t_min is not >= 0 (the
//                      slab test clips at 0), or its origin lies beyond the reach of the boxes' margin (below).
//   MASKED             with visibility groups (tor_scene_groups): object j takes part for ray i iff groups[j] & mask_i != 0.  The
//                      order independence above is what makes this exact: the closest hit over the objects a ray sees is the
//                      sequential loop on the sub-list of those objects, ties to the lowest index among them.  Skipping a box whose
//                      OR-word shares no bit with the ray's mask skips only objects the ray does not see.  One kernel text for both:
//                      the argument (KArgs, tor_query.hpp) carries the group words only when MASKED, `vis` is a Sees<MASKED>, and
//                      the unmasked instantiations compile to what they were without the parameter.
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

template <bool BLOCKS, bool MASKED>
__global__ __launch_bounds__(kHitThreads) void hit_kernel(const KArgs<QParams, MASKED> A) {
  const QParams& p = A.P;
  const long long i = (long long)blockIdx.x * kHitThreads + threadIdx.x;
  const bool live = i < p.n_rays;
  Sees<MASKED> vis{nullptr, nullptr, 0u};  // the descent's `vis` (lanes past the end see nothing)
  if constexpr (MASKED) {
    if (live) vis.m = A.mk.ray_mask ? A.mk.ray_mask[i] : A.mk.mask;
    vis.grp = A.mk.grp;
    vis.box_or = A.mk.box_or;
  }
  QRay r{};  // (lanes past the end: t_max = 0 accepts nothing)
  if (live) load_ray(r, p.rays, p.t_range, i);
  r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30 r.direction.length_squared()
  QBest b{r.t_max, INT_MAX, -1};
#include "tor_query_descent.inc"
  if (!live) return;
  double* o = p.hits + 8 * i;
  if (b.slot < 0) {
    write_miss_record(o);
    return;
  }
  const qgdptr c = (qgdptr)(uintptr_t)(p.cold + 16 * (size_t)b.slot);
  const double t = b.t;
  const int object = b.orig;
#include "tor_query_record.inc"
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
  absr[0].release();
  absr[1].release();
  lights.release();
  media.release();
  drop_grids();
  env.release();
  ph_cell.release();
  ph_rec.release();
  ph_start.release();
  ph_tmp.release();
  tex_table.release();
  tex_binding.release();
  tex_atlas.release();
  if (ev_done) (void)hipEventDestroy(ev_done);
}

}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx; then the scene
int hit_check(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, double time_lo, double time_hi, int32_t mode,
              const void* hits) {
  const std::string w = who;
  int rc = tor::count_args(w, ctx, n_rays);
  if (rc == TOR_OK) rc = tor::range_args(w, time_lo, time_hi, mode);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && (!rays || !hits)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays or hits");
  return tor::scene_args(who, ctx);
}

// the launch; the arguments are checked and n_rays > 0.  masked: with the visibility groups and d_mask / mask (tor_hit_masked_device)
int hit_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, double time_lo,
               double time_hi, int32_t mode, void* d_hits, hipStream_t stream, bool masked, const uint32_t* d_mask, uint32_t mask) {
  tor::QParams p{};
  tor::MParams mk{};
  bool blocks = false;
  std::string why;
  int rc = tor::query_setup(who, ctx, time_lo, time_hi, mode, stream, p, blocks, why);
  if (rc == TOR_OK && masked) rc = tor::masked_setup(ctx, blocks, d_mask, mask, stream, mk);
  if (rc != TOR_OK) return rc;
  p.rays = (const double*)d_rays;
  p.t_range = d_t_range;
  p.hits = (double*)d_hits;
  p.n_rays = (long long)n_rays;
  const unsigned grid = (unsigned)((n_rays + tor::kHitThreads - 1) / tor::kHitThreads);
  tor::for_variant(blocks, masked, [&](auto B, auto M) {
    hipLaunchKernelGGL((tor::hit_kernel<decltype(B)::value, decltype(M)::value>), dim3(grid), dim3(tor::kHitThreads), 0, stream,
                       tor::kargs<decltype(M)::value>(p, mk));
  });
  return tor::query_finish(ctx, stream, "hit", masked, blocks, why);
}

// tor_hit_device / tor_hit_masked_device
int hit_device(const char* who, TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo,
               double time_hi, int32_t mode, TorHit* d_hits, void* hip_stream, bool masked, const uint32_t* d_mask, uint32_t mask) {
  const int rc = hit_check(who, ctx, n_rays, d_rays, time_lo, time_hi, mode, d_hits);
  if (rc != TOR_OK || n_rays == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return hit_launch(who, ctx, n_rays, d_rays, d_t_range, time_lo, time_hi, mode, d_hits, (hipStream_t)hip_stream, masked, d_mask, mask);
}

// tor_hit_host / tor_hit_masked_host (masks: nullable host words): copy in, the device query on the default stream, copy out
int hit_host(const char* who, TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo, double time_hi,
             int32_t mode, TorHit* hits, bool masked, const uint32_t* masks, uint32_t mask) {
  int rc = hit_check(who, ctx, n_rays, rays, time_lo, time_hi, mode, hits);
  if (rc != TOR_OK || n_rays == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_rays;
  tor::HostPart st[4] = {{rays, n * sizeof(TorRay), true, false},
                         {t_range, t_range ? n * 16 : 0, true, false},
                         {hits, n * sizeof(TorHit), false, true},
                         {masks, masked && masks ? n * 4 : 0, true, false}};
  rc = tor::stage_in(ctx, st, 4);
  if (rc != TOR_OK) return rc;
  rc = hit_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), time_lo, time_hi, mode, st[2].dev, nullptr, masked,
                  st[3].as<const uint32_t>(), mask);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 4);
}

}  // namespace

extern "C" {

int tor_hit_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo, double time_hi,
                   int32_t mode, TorHit* d_hits, void* hip_stream) {
  return hit_device("tor_hit_device", ctx, n_rays, d_rays, d_t_range, time_lo, time_hi, mode, d_hits, hip_stream, false, nullptr, 0);
}

int tor_hit_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo, double time_hi,
                 int32_t mode, TorHit* hits) {
  return hit_host("tor_hit_host", ctx, n_rays, rays, t_range, time_lo, time_hi, mode, hits, false, nullptr, 0);
}

int tor_hit_masked_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo, double time_hi,
                          int32_t mode, TorHit* d_hits, void* hip_stream, const uint32_t* d_mask, uint32_t mask) {
  return hit_device("tor_hit_masked_device", ctx, n_rays, d_rays, d_t_range, time_lo, time_hi, mode, d_hits, hip_stream, true, d_mask,
                    mask);
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
