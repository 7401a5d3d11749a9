// tor_occluded.hip -- batched any-hit (occlusion) queries against the uploaded scene (tor_occluded_device / tor_occluded_host,
// include/tor_render.h): for each listed ray ONE bit, whether world.hit(r, t_min, t_max, rec) of the reference returns true
// (hittables_lists.nim:48-55 over spheres.nim:28-49 / moving_spheres.nim:39-67), on gfx950.  What a host integrator asks for its
// shadow rays.  A kernel of its own: the closest-hit descent (tor_query_descent.inc) must test every candidate; this one stops.
//
// Why the bit is order independent.  HittableList.hit returns hit_anything, and the closest_so_far it shrinks along the way can only
// reject a root of a LATER object once an EARLIER object has been accepted -- by which time hit_anything is already true.  So
//     occluded(r, t_min, t_max) = OR over the list of Sphere.hit / MovingSphere.hit(r, t_min, t_max)
// each with the caller's t_max: the first root if it lies in (t_min, t_max), else the second, both comparisons strict.  An OR holds in
// any visiting order and under any early exit; objects that cannot be hit may be skipped (the head of tor_query.hip says why the
// block boxes, with their margin, `reach` and a_min, skip only those).  WHICH object occludes depends on the order, so it is not
// reported.
//
//   occluded_kernel<false, MASKED>  brute force: one listed ray per lane; the cold slots of the flat layout in a wave-uniform loop (scalar
//                           loads) that the wave leaves once every live lane has its answer
//   occluded_kernel<true, MASKED>   blocks: the culling layout's always-objects first, in the same loop (in random_scene they hold the
//                           ground sphere, which settles most downward rays); then the rays the boxes do not hold for walk the
//                           spatial slots, wave-uniform, until all of them are settled; the others descend the block / super boxes
//                           per lane and leave at every level once their flag is set.  The 8 records of a block are tested
//                           together: their loads go out as one batch, and a branch between them would serialise eight round trips.
//   MASKED                  with visibility groups: the OR over the objects the ray sees (the kernel's comment; KArgs and Sees,
//                           tor_query.hpp)
//
// The slab test's exit is clipped at the ray's t_max (slab_clipped): a box the segment ends in front of is not entered.  Why that
// stays conservative.  Let `sol` be a root the reference accepts for an object of the box, for a ray that uses the boxes
// (0 <= t_min < sol < t_max, time inside the boxes' range, origin within `reach`, a >= a_min), and P = origin + sol * direction.
//  (1) P lies in the box with a margin.  sol = (-half_b +- root) / a with root^2 = disc + rounding, and disc carries the absolute
//      error 12 eps |d|^2 (|oc|^2 + r^2) of the head of tor_query.hip, so |P - centre|^2 = dist^2 + (sol - t_c)^2 |d|^2 <= r^2 +
//      12 eps (|oc|^2 + r^2) up to terms of order eps (|oc| + r): P is at most 6 eps (|oc|^2 + r^2) / r outside the sphere -- the
//      bound that holds for the ray's line, now for the point at the COMPUTED root.  Within `reach` that is below 1e-6 / 4
//      (hit_reach), and every box is inflated by at least 1e-6: along each axis k, lo_k + m <= P_k <= hi_k - m with m >= 0.75e-6.
//  (2) So in exact arithmetic the entry parameter of every axis with d_k != 0, e_k = min((lo_k - o_k) / d_k, (hi_k - o_k) / d_k),
//      is at most sol - m / |d_k|.  The slab test computes e_k as fl(fl(lo_k - o_k) * fl(1 / d_k)): three roundings, a relative error
//      below 4 eps, and an underflowed product is off by less than 2^-1022, far below m / |d_k| (|d_k| < 1e154, or a overflows and
//      nothing is accepted).  The clip compares t_in * (1 - 2^-40): for t_in > 0 that is below max_k e_k <= sol < t_max whatever the
//      distance of the origin, and t_in = 0 (the clip at 0) passes because 0 <= t_min < sol < t_max.
//  (3) An axis with d_k = 0 or 1 / d_k = +-inf gives -inf (no constraint) when o_k lies strictly inside [lo_k, hi_k], which (1)
//      implies when |sol d_k| < m; otherwise e_k is finite in exact arithmetic only for |sol| > m / |d_k| > 1e302, and a >= a_min puts
//      such a point outside every box.  The unclipped test rests on the same cases.
//  (4) t_max = NaN accepts nothing and enters nothing; t_max = +inf leaves the test as it was.
// So a box that holds an accepted root is still entered; boxes entered needlessly cost time only.  tests/test_gpu_occluded_query.py
// steps t_max across the roots of 200 spheres ulp by ulp to guard this.
//
// Float64, unfused (-ffp-contract=off), correctly rounded division and square root: exact_test's arithmetic (tor_query.hpp).
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

static_assert(sizeof(TorRay) == 56, "TorRay: origin, direction, time (primitives/rays.nim)");

namespace tor {
namespace {

struct OParams {
  QParams q;         // the scene and its boxes, rays, t_range, n_rays (hits unused)
  const int* list;   // the rays to answer, or null: entry e is ray e
  long long n_list;
  int* occluded;     // one int32 per ray, indexed by the ray
};

// spheres.nim:29-48 / moving_spheres.nim:47-66 for the object in cold record c: does it accept a root in (t_min, t_max)?
// exact_test's operations in exact_test's order, without the closest-so-far.
template <typename P>
__device__ __forceinline__ bool occludes(P c, const QRay& r) {
  const double r2 = c[15];
  if (r2 == -1.0) return false;  // padding slot
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);
  const double ocx = r.ox - cx, ocy = r.oy - cy, ocz = r.oz - cz;
  const double hb = ocx * r.dx + ocy * r.dy + ocz * r.dz;
  const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
  const double disc = hb * hb - r.a * cc;
  bool ok = false;
  if (disc > 0.0) {
    const double root = __builtin_sqrt(disc);
    double sol = (-hb - root) / r.a;
    ok = (r.t_min < sol) && (sol < r.t_max);
    if (!ok) {
      sol = (-hb + root) / r.a;
      ok = (r.t_min < sol) && (sol < r.t_max);
    }
  }
  return ok;
}

// slab (tor_query.hpp) with the exit clipped at the ray's t_max; the file head says why it stays conservative
template <typename P>
__device__ __forceinline__ bool slab_clipped(P bx, const QRay& r, double ix, double iy, double iz) {
  const double tx0 = (bx[0] - r.ox) * ix, tx1 = (bx[3] - r.ox) * ix;
  const double ty0 = (bx[1] - r.oy) * iy, ty1 = (bx[4] - r.oy) * iy;
  const double tz0 = (bx[2] - r.oz) * iz, tz1 = (bx[5] - r.oz) * iz;
  const double t_in = __builtin_fmax(__builtin_fmax(__builtin_fmin(tx0, tx1), __builtin_fmin(ty0, ty1)),
                                     __builtin_fmax(__builtin_fmin(tz0, tz1), 0.0));
  const double t_out = __builtin_fmin(__builtin_fmin(__builtin_fmax(tx0, tx1), __builtin_fmax(ty0, ty1)), __builtin_fmax(tz0, tz1));
  return (t_in <= t_out) && (t_in * (1.0 - 0x1p-40) <= r.t_max);
}

// MASKED: with visibility groups (tor_occluded_masked_device) only the objects a ray sees can occlude it: the OR of the file head,
// over the sub-list.  Every early exit counts a lane as settled only once it has FOUND an occluder: a lane whose mask rejects a
// slot or a box is simply not tested there and stays unsettled.
template <bool BLOCKS, bool MASKED>
__global__ __launch_bounds__(kHitThreads) void occluded_kernel(const KArgs<OParams, MASKED> A) {
  const OParams& P = A.P;
  const QParams& p = P.q;
  const long long i = listed_ray(P.list, P.n_list, p.n_rays, (long long)blockIdx.x * kHitThreads + threadIdx.x);
  const bool live = i >= 0;
  Sees<MASKED> vis{nullptr, nullptr, 0u};  // (lanes without a ray see nothing)
  if constexpr (MASKED) {
    if (live) vis.m = A.mk.ray_mask ? A.mk.ray_mask[i] : A.mk.mask;
    vis.grp = A.mk.grp;
    vis.box_or = A.mk.box_or;
  }
  QRay r{};  // (lanes without a ray: t_max = 0 accepts nothing)
  if (live) load_ray(r, p.rays, p.t_range, i);
  r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30
  bool found = false;
  // wave-uniform: every unsettled lane that sees the slot tests the same record; the wave leaves when no unsettled lane is left
  for (int s = 0; s < p.n_uniform; ++s) {
    if (__ballot(live && !found) == 0) break;
    if (live && !found && vis.slot_u(s)) found = occludes((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)s), r);
  }
  if constexpr (BLOCKS) {
    const double ex = r.ox - p.org[0], ey = r.oy - p.org[1], ez = r.oz - p.org[2];
    const bool boxed = live && (r.t_min >= 0.0) && (r.time >= p.time_lo) && (r.time <= p.time_hi) &&
                       (ex * ex + ey * ey + ez * ez <= p.reach2) && (r.a >= p.a_min);
    const bool walk = live && !boxed;
    // rays the boxes do not hold for: every spatial slot, wave-uniform, until all of them are settled
    for (int s = 0; s < p.n_spatial; ++s) {
      if (__ballot(walk && !found) == 0) break;
      if (walk && !found && vis.slot_u(p.spatial_base + s)) found = occludes((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)(p.spatial_base + s)), r);
    }
    if (boxed && !found) {
      const double ix = 1.0 / r.dx, iy = 1.0 / r.dy, iz = 1.0 / r.dz;
      auto test_box = [&](int box) {  // the blocks behind block box `box`, 8 objects each
        for (int fk = 0; fk < p.fanout && !found; ++fk) {
          const int slot0 = p.spatial_base + 8 * (box * p.fanout + fk);
          bool any = false;
          for (int k = 0; k < 8; ++k)
            if (vis.slot(slot0 + k)) any |= occludes((qgdptr)(uintptr_t)(p.cold + 16 * (size_t)(slot0 + k)), r);
          found = any;
        }
      };
      const int n_top = p.two_level ? p.n_super : p.n_boxes;
      const int top0 = p.two_level ? p.super0 : 0;
      // the top-level boxes 64 at a time (scalar loads); then the ones the ray's segment enters
      for (int c0 = 0; c0 < n_top && !found; c0 += 64) {
        const int cn = n_top - c0 < 64 ? n_top - c0 : 64;
        unsigned long long m = 0;
        for (int j = 0; j < cn; ++j)
          if (vis.box_u(top0 + c0 + j) && slab_clipped((qcdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + c0 + j)), r, ix, iy, iz)) m |= 1ull << j;
        while (m != 0 && !found) {
          const int top = c0 + __builtin_ctzll(m);
          m &= m - 1;
          if (!p.two_level) {
            test_box(top);
            continue;
          }
          // super box `top`: its 8 block boxes (NaN padding boxes are never entered)
          unsigned m8 = 0;
          for (int k = 0; k < 8; ++k)
            if (vis.box(8 * top + k) && slab_clipped((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(8 * top + k)), r, ix, iy, iz)) m8 |= 1u << k;
          while (m8 != 0 && !found) {
            const int k = __builtin_ctz(m8);
            m8 &= m8 - 1;
            test_box(8 * top + k);
          }
        }
      }
    }
  }
  if (live) P.occluded[i] = found ? 1 : 0;
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: what tor_hit_device refuses, and the path steps' list rules;
// then the scene
int occluded_check(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, const void* list, int64_t n_list, double time_lo,
                   double time_hi, int32_t mode, const void* occluded) {
  const std::string w = who;
  int rc = tor::list_args(w, ctx, n_rays, list, n_list);
  if (rc == TOR_OK) rc = tor::range_args(w, time_lo, time_hi, mode);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && (!rays || !occluded)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays or occluded");
  return tor::scene_args(who, ctx);
}

// the launch; the arguments are checked, n_rays > 0 and n_list > 0
int occluded_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, const int32_t* d_list,
                    int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* d_occluded, hipStream_t stream, bool masked,
                    const uint32_t* d_mask, uint32_t mask) {
  tor::OParams P{};
  tor::MParams mk{};
  bool blocks = false;
  std::string why;
  int rc = tor::query_setup(who, ctx, time_lo, time_hi, mode, stream, P.q, blocks, why);
  if (rc == TOR_OK && masked) rc = tor::masked_setup(ctx, blocks, d_mask, mask, stream, mk);
  if (rc != TOR_OK) return rc;
  P.q.rays = (const double*)d_rays;
  P.q.t_range = d_t_range;
  P.q.n_rays = (long long)n_rays;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.occluded = d_occluded;
  const unsigned grid = (unsigned)((n_list + tor::kHitThreads - 1) / tor::kHitThreads);
  tor::for_variant(blocks, masked, [&](auto B, auto M) {
    hipLaunchKernelGGL((tor::occluded_kernel<decltype(B)::value, decltype(M)::value>), dim3(grid), dim3(tor::kHitThreads), 0, stream,
                       tor::kargs<decltype(M)::value>(P, mk));
  });
  return tor::query_finish(ctx, stream, "occluded", masked, blocks, why);
}

// tor_occluded_device / tor_occluded_masked_device
int occluded_device(const char* who, TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                    int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* d_occluded, void* hip_stream, bool masked,
                    const uint32_t* d_mask, uint32_t mask) {
  const int rc = occluded_check(who, ctx, n_rays, d_rays, d_list, n_list, time_lo, time_hi, mode, d_occluded);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return occluded_launch(who, ctx, n_rays, d_rays, d_t_range, d_list, n_list, time_lo, time_hi, mode, d_occluded, (hipStream_t)hip_stream,
                         masked, d_mask, mask);
}

// tor_occluded_host / tor_occluded_masked_host (masks: nullable host words): every array in -- the output too, rays that are not
// listed keep what the caller holds --, the query on the default stream, the output back
int occluded_host(const char* who, TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                  int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* occluded, bool masked, const uint32_t* masks,
                  uint32_t mask) {
  int rc = occluded_check(who, ctx, n_rays, rays, list, n_list, time_lo, time_hi, mode, occluded);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_rays;
  tor::HostPart st[5] = {{rays, n * sizeof(TorRay), true, false},
                         {t_range, t_range ? n * 16 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {occluded, n * 4, true, true},
                         {masks, masked && masks ? n * 4 : 0, true, false}};
  rc = tor::stage_in(ctx, st, 5);
  if (rc != TOR_OK) return rc;
  rc = occluded_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const int32_t>(), n_list, time_lo, time_hi, mode,
                       st[3].as<int32_t>(), nullptr, masked, st[4].as<const uint32_t>(), mask);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 5);
}

}  // namespace

extern "C" {

int tor_occluded_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                        int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* d_occluded, void* hip_stream) {
  return occluded_device("tor_occluded_device", ctx, n_rays, d_rays, d_t_range, d_list, n_list, time_lo, time_hi, mode, d_occluded,
                         hip_stream, false, nullptr, 0);
}

int tor_occluded_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list, int64_t n_list,
                      double time_lo, double time_hi, int32_t mode, int32_t* occluded) {
  return occluded_host("tor_occluded_host", ctx, n_rays, rays, t_range, list, n_list, time_lo, time_hi, mode, occluded, false, nullptr, 0);
}

int tor_occluded_masked_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                               int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* d_occluded, void* hip_stream,
                               const uint32_t* d_mask, uint32_t mask) {
  return occluded_device("tor_occluded_masked_device", ctx, n_rays, d_rays, d_t_range, d_list, n_list, time_lo, time_hi, mode, d_occluded,
                         hip_stream, true, d_mask, mask);
}

int tor_occluded_masked_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                             int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* occluded, const uint32_t* masks,
                             uint32_t mask) {
  return occluded_host("tor_occluded_masked_host", ctx, n_rays, rays, t_range, list, n_list, time_lo, time_hi, mode, occluded, true, masks,
                       mask);
}

}  // extern "C"
