// tor_crossings.hip -- batched ordered multi-hit queries against the uploaded scene (tor_crossings_device / tor_crossings_host,
// include/tor_render.h): for each listed ray the first K surface crossings in (t_min, t_max), in order, on gfx950.  What a host asks
// for transparent shadows (the surfaces a segment crosses, or the path length inside glass), depth peeling, thickness and inside /
// outside parity, and picking through glass -- in one walk of the scene where K dependent tor_hit_device launches take K.
//
// What a crossing is.  For ray r and object j the reference computes (spheres.nim:29-48 / moving_spheres.nim:39-66)
//     s0 = (-half_b - sqrt(disc)) / a,  s1 = (-half_b + sqrt(disc)) / a     when disc > 0 (strict),
// in float64, unfused, with correctly rounded `/` and sqrt: exact_test's operations in exact_test's order (tor_query.hpp).  Every
// root with t_min < s < t_max (both strict, as in the reference) is a crossing (t, object, which): which = 0 for s0, 1 for s1; BOTH
// roots of one object count.  NaN and infinite roots fail the comparisons; padding slots have none.  The crossings of a ray are
// ordered by the key (t, object, which), ascending, t compared as a double; the query returns the first min(total, K) of them.
//
// Why the answer is order independent.  The crossings of a ray are a SET of keys, each a function of the ray, the range and one
// object alone -- no closest_so_far couples the objects.  No two keys are equal (object and which tell them apart), so "the K
// smallest keys of the set, ascending" is one well-defined list whatever order the objects are visited in.  Inserting the keys one by
// one into a sorted list that keeps its K smallest gives that list for every insertion order: a key among the final K is never
// displaced (at most K - 1 keys are smaller), and a key that is not is displaced by the time the last smaller one has arrived.  For
// the same reason a key may be dropped on sight once K keys that are smaller have been seen, and objects that cannot produce a key
// among the K smallest may be skipped.  Consequences, bit for bit: crossing 0 is tor_hit_device's (t, object) -- per object the first
// root in range is never larger than the second, so the smallest accepted root over the list, ties to the lowest index, is the
// smallest key; count > 0 is tor_occluded_device's bit; and on a ray without equal-t crossings, crossing k + 1 is tor_hit_device's
// answer with t_min := crossing k's t (same ray, same objects, same roots; only the range moves).
//
//   crossings_kernel<false, MASKED, CAP>  brute force: one listed ray per lane; every cold slot of the flat layout in a wave-uniform
//                                         loop (records through the scalar-load view)
//   crossings_kernel<true, MASKED, CAP>   blocks: the culling layout's always-objects in the same loop; the rays the boxes do not hold
//                                         for (time outside the range or NaN, t_min not >= 0, origin beyond `reach`, a < a_min) walk
//                                         every spatial slot, wave-uniform; the others descend the super boxes, block boxes and blocks
//                                         per lane, the records of a block loaded and tested as a batch before any is inserted (all 8
//                                         with CAP = 4; 4 and 4 with CAP = 16, whose list leaves fewer registers)
//   MASKED                                with visibility groups (Sees<true>, masked_setup): object j takes part for ray i iff
//                                         groups[j] & mask_i != 0 -- the same set restricted to the objects the ray sees, `object` in
//                                         the full list's numbering; a box whose OR-word shares no bit with the mask is not entered
//   CAP                                   4 (K <= 4, the transparent-shadow case) or TOR_CROSSINGS_MAX = 16: the sorted list lives in
//                                         registers, per entry t and one packed word object * 2 + which, and an insertion is a fully
//                                         unrolled compare-and-select chain over the CAP entries.  No array is indexed dynamically: the
//                                         K entries in use are the LAST K of the CAP (the ones in front hold -inf and never move), so
//                                         the K-th smallest is always entry CAP - 1, a fixed register.  No variant uses scratch.
//
// The bound shrinks.  While the list holds fewer than K crossings the bound is t_max; once it is full it is the K-th entry's t, and it
// only ever decreases.  A per-object root above the bound is dropped; a root EQUAL to it goes through the full key compare (a lower
// object index at the same t must displace the K-th).  A box is entered iff the slab test passes and t_in * (1 - 2^-40) <= bound --
// non-strict on the keep side for the same reason.
//
// Why the clipped boxes stay exact.  Let `sol` be a root that belongs to the final answer, of a spatial object, for a ray that uses
// the boxes (0 <= t_min < sol < t_max, time inside the boxes' range, origin within `reach`, a >= a_min), and P = origin + sol *
// direction.  The final answer's keys are at or below the final bound, and the bound at any earlier moment is no smaller: sol <=
// bound whenever a box is tested.
//  (1) P lies in the object's box with a margin.  The head of tor_occluded.hip derives it from sol = (-half_b +- root) / a with
//      root^2 = disc + rounding and the discriminant's absolute error 12 eps |d|^2 (|oc|^2 + r^2) (head of tor_query.hip): |P -
//      centre|^2 <= r^2 + 12 eps (|oc|^2 + r^2) up to terms of order eps (|oc| + r), so P is at most 6 eps (|oc|^2 + r^2) / r
//      outside the sphere, below 1e-6 / 4 within `reach` (hit_reach), and every box is inflated by at least 1e-6.  The derivation
//      never uses WHICH sign the root carries or that the other root was rejected: it holds for s0 and for s1 of one object at
//      once, each with its own P, and both points lie in the same box (the box bounds the sphere over the time range, inflated).
//      Here both roots of an object are candidates at the same time, and both are covered.
//  (2) So in exact arithmetic the entry parameter of every axis with d_k != 0 is at most sol - m / |d_k| with m >= 0.75e-6, the
//      computed one is within a relative 4 eps of it (three roundings; an underflowed product is off by less than 2^-1022), and
//      t_in * (1 - 2^-40) < sol <= bound for t_in > 0; t_in = 0 (the clip at 0) passes because 0 <= t_min < sol <= bound.  Axes
//      with d_k = 0 or 1 / d_k = +-inf are case (3) of tor_occluded.hip's head, unchanged, and the unclipped test t_in <= t_out
//      rests on the same cases.
//  (3) t_max = NaN accepts nothing, the bound is NaN and nothing is entered; t_max = +inf leaves the test unclipped until the list is
//      full.
// So a box that holds a crossing of the final answer is entered whenever it is tested -- at the top level against the bound at the
// start of its chunk of 64, at the block boxes of a super box against the bound when the super box is opened, and once more
// against the current bound just before a block box is opened, in one-level and two-level layouts alike -- and boxes entered
// needlessly cost time only.  Boxes are visited in index order, not near to far, so how much the shrinking bound saves depends on
// the scene.  tests/test_gpu_crossings_query.py steps t_max and t_min across the roots of
// 200 spheres ulp by ulp, and places coincident duplicates so that entries K and K + 1 share one t, to guard this.
//
// Results, and the records rebuilt at the end from the by-object cold records (tor_hit_device's formula for that (t, object):
// rays.nim:24-25, vec3s.nim:93-94, core.nim:47-49), go out as ordinary per-lane stores.
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
#include "tor_scene.hpp"

static_assert(sizeof(TorRay) == 56, "TorRay: origin, direction, time (primitives/rays.nim)");
static_assert(sizeof(TorCrossing) == 16 && offsetof(TorCrossing, object) == 8 && offsetof(TorCrossing, which) == 12,
              "TorCrossing: t, object, which");
static_assert(sizeof(TorHit) == 64 && offsetof(TorHit, t) == 48 && offsetof(TorHit, object) == 56 && offsetof(TorHit, front_face) == 60,
              "TorHit: HitRecord (physics/core.nim:30-36) with the object index in place of the material");
static_assert(TOR_CROSSINGS_MAX == 16, "the large capacity variant holds TOR_CROSSINGS_MAX entries");

namespace tor {
namespace {

constexpr int kCapSmall = 4;
constexpr int kCapLarge = TOR_CROSSINGS_MAX;

struct XParams {
  QParams q;               // the scene and its boxes, rays, t_range, n_rays (hits unused)
  const int* list;         // the rays to answer, or null: entry e is ray e
  long long n_list;
  int k;                   // crossings per ray, 1 .. CAP
  double* cross;           // k TorCrossing per ray, 2 float64 words each: t, then object (low word) and which (high word)
  int* count;              // one int32 per ray
  double* records;         // null, or k TorHit per ray, 8 float64 words each
  const double* obj_cold;  // records only: the cold records by ORIGINAL index, 16 float64 per object
};

// spheres.nim:29-48 / moving_spheres.nim:47-66 for the object in cold record c: both roots, whether each lies in (t_min, t_max), and
// the object's key.  exact_test's operations in exact_test's order, without the closest-so-far and without the early choice.
struct XRoots {
  double s0, s1;
  unsigned key;  // object * 2
  bool ok0, ok1;
};

template <typename P>
__device__ __forceinline__ XRoots roots_of(P c, const QRay& r) {
  XRoots x{0.0, 0.0, 0u, false, false};
  const double r2 = c[15];
  if (r2 == -1.0) return x;  // padding slot
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);
  const double ocx = r.ox - cx, ocy = r.oy - cy, ocz = r.oz - cz;
  const double hb = ocx * r.dx + ocy * r.dy + ocz * r.dz;
  const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
  const double disc = hb * hb - r.a * cc;
  if (disc > 0.0) {
    const double root = __builtin_sqrt(disc);
    x.s0 = (-hb - root) / r.a;
    x.s1 = (-hb + root) / r.a;
    x.ok0 = (r.t_min < x.s0) && (x.s0 < r.t_max);
    x.ok1 = (r.t_min < x.s1) && (x.s1 < r.t_max);
    x.key = (unsigned)(int)__double_as_longlong(c[14]) << 1;
  }
  return x;
}

// a root above the bound is dropped; one equal to it goes through the key compare
template <int CAP>
__device__ __forceinline__ void take(XList<CAP>& L, const XRoots& x, const QRay& r) {
  if (x.ok0 && !(x.s0 > L.bound(r.t_max))) L.insert(x.s0, x.key);
  if (x.ok1 && !(x.s1 > L.bound(r.t_max))) L.insert(x.s1, x.key | 1u);
}

// slab (tor_query.hpp) with the entry clipped at the shrinking bound; the file head says why it stays exact
template <typename P>
__device__ __forceinline__ bool slab_bound(P bx, const QRay& r, double ix, double iy, double iz, double bound) {
  const double tx0 = (bx[0] - r.ox) * ix, tx1 = (bx[3] - r.ox) * ix;
  const double ty0 = (bx[1] - r.oy) * iy, ty1 = (bx[4] - r.oy) * iy;
  const double tz0 = (bx[2] - r.oz) * iz, tz1 = (bx[5] - r.oz) * iz;
  const double t_in = __builtin_fmax(__builtin_fmax(__builtin_fmin(tx0, tx1), __builtin_fmin(ty0, ty1)),
                                     __builtin_fmax(__builtin_fmin(tz0, tz1), 0.0));
  const double t_out = __builtin_fmin(__builtin_fmin(__builtin_fmax(tx0, tx1), __builtin_fmax(ty0, ty1)), __builtin_fmax(tz0, tz1));
  return (t_in <= t_out) && (t_in * (1.0 - 0x1p-40) <= bound);
}

// TorHit for the crossing (t, object): tor_hit_device's record for that root of that object, from the by-object cold records
__device__ __forceinline__ void write_record(double* o, const double* obj_cold, const QRay& r, double t, unsigned key) {
  const int object = (int)(key >> 1);
  const qgdptr c = (qgdptr)(uintptr_t)(obj_cold + 16 * (size_t)object);
#include "tor_query_record.inc"
}

template <bool BLOCKS, bool MASKED, int CAP>
__global__ __launch_bounds__(kHitThreads) void crossings_kernel(const XParams P, const MParams mk) {
  const QParams& p = P.q;
  const long long e = (long long)blockIdx.x * kHitThreads + threadIdx.x;
  // listed_ray's rule (tor_query.hpp), spelled out: through the function two instructions of the blocks variants change places
  long long i = -1;  // the ray of list entry e; -1: past the end of the list, or an entry outside [0, n_rays) (skipped)
  if (e < P.n_list) {
    const long long v = P.list ? (long long)P.list[e] : e;
    if (v >= 0 && v < p.n_rays) i = v;
  }
  const bool live = i >= 0;
  unsigned r_mask = 0u;  // (lanes without a ray see nothing)
  if constexpr (MASKED) {
    if (live) r_mask = mk.ray_mask ? mk.ray_mask[i] : mk.mask;
  }
  const Sees<MASKED> vis{mk.grp, mk.box_or, r_mask};
  QRay r{};  // (lanes without a ray: t_max = 0 accepts nothing)
  if (live) load_ray(r, p.rays, p.t_range, i);
  r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30
  const int K = P.k < CAP ? P.k : CAP;
  // records of a block tested per batch: all 8 with the small list; 4 with the large one, whose registers a batch of 8 would push
  // past two waves per SIMD
  constexpr int kBatch = CAP <= kCapSmall ? 8 : 4;
  XList<CAP> L;
  L.init(K);
  // wave-uniform: every live lane that sees the slot tests the same record
  for (int s = 0; s < p.n_uniform; ++s)
    if (live && vis.slot_u(s)) take(L, roots_of((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)s), r), r);
  if constexpr (BLOCKS) {
    const double ex = r.ox - p.org[0], ey = r.oy - p.org[1], ez = r.oz - p.org[2];
    const bool boxed = live && (r.t_min >= 0.0) && (r.time >= p.time_lo) && (r.time <= p.time_hi) &&
                       (ex * ex + ey * ey + ez * ez <= p.reach2) && (r.a >= p.a_min);
    const bool walk = live && !boxed;
    if (__ballot(walk) != 0) {  // rays the boxes do not hold for: every spatial slot, wave-uniform
      for (int s = 0; s < p.n_spatial; ++s) {
        const int slot = p.spatial_base + s;
        if (walk && vis.slot_u(slot)) take(L, roots_of((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)slot), r), r);
      }
    }
    if (boxed) {
      const double ix = 1.0 / r.dx, iy = 1.0 / r.dy, iz = 1.0 / r.dz;
      auto test_box = [&](int box) {  // the blocks behind block box `box`, 8 objects each
        for (int fk = 0; fk < p.fanout; ++fk) {
          const int slot0 = p.spatial_base + 8 * (box * p.fanout + fk);
          // the records' loads go out as one batch: no insertion (a branch) between them
#pragma unroll 1
          for (int k0 = 0; k0 < 8; k0 += kBatch) {
            XRoots x[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
              x[k] = XRoots{0.0, 0.0, 0u, false, false};
              if (vis.slot(slot0 + k0 + k)) x[k] = roots_of((qgdptr)(uintptr_t)(p.cold + 16 * (size_t)(slot0 + k0 + k)), r);
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) take(L, x[k], r);
          }
        }
      };
      const int n_top = p.two_level ? p.n_super : p.n_boxes;
      const int top0 = p.two_level ? p.super0 : 0;
      // the top-level boxes 64 at a time (scalar loads); then the ones the ray's segment enters below the bound
      for (int c0 = 0; c0 < n_top; c0 += 64) {
        const int cn = n_top - c0 < 64 ? n_top - c0 : 64;
        const double b0 = L.bound(r.t_max);
        unsigned long long m = 0;
        for (int j = 0; j < cn; ++j)
          if (vis.box_u(top0 + c0 + j) && slab_bound((qcdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + c0 + j)), r, ix, iy, iz, b0))
            m |= 1ull << j;
        while (m != 0) {
          const int top = c0 + __builtin_ctzll(m);
          m &= m - 1;
          // one level: block box `top` itself.  Two levels: super box `top`, its 8 block boxes (NaN padding boxes are never
          // entered), against the bound as it stands now.  (One call of test_box for both: the insertion chains are long.)
          unsigned m8 = 1u;
          int box0 = top;
          if (p.two_level) {
            const double b1 = L.bound(r.t_max);
            m8 = 0u;
            box0 = 8 * top;
            for (int k = 0; k < 8; ++k)
              if (vis.box(box0 + k) && slab_bound((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(box0 + k)), r, ix, iy, iz, b1)) m8 |= 1u << k;
          }
          // the bound may have shrunk since the box passed its test (b0 is a chunk old, b1 a super box old): a block box is
          // opened only if it still lies at or below the bound as it stands now
          while (m8 != 0) {
            const int k = __builtin_ctz(m8);
            m8 &= m8 - 1;
            if (slab_bound((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(box0 + k)), r, ix, iy, iz, L.bound(r.t_max))) test_box(box0 + k);
          }
        }
      }
    }
  }
  if (!live) return;
  // entries CAP - K .. CAP - 1 are crossings 0 .. K - 1; unused ones hold t = 0, object = -1, which = 0 (and the miss record)
  double* out = P.cross + 2 * (size_t)i * (size_t)P.k;
  double* rec = P.records ? P.records + 8 * (size_t)i * (size_t)P.k : nullptr;
  int count = 0;
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    const int m = j - (CAP - K);
    if (m < 0) continue;
    const bool has = L.t[j] < __builtin_inf();
    count += has ? 1 : 0;
    const unsigned long long w = has ? (((unsigned long long)(L.key[j] & 1u) << 32) | (unsigned long long)(L.key[j] >> 1)) : 0xffffffffull;
    out[2 * m] = has ? L.t[j] : 0.0;
    out[2 * m + 1] = __longlong_as_double((long long)w);
    if (rec) {
      double* o = rec + 8 * m;
      if (has) {
        write_record(o, P.obj_cold, r, L.t[j], L.key[j]);
      } else {  // write_miss_record's stores (tor_query.hpp), spelled out for the same reason
        for (int k = 0; k < 7; ++k) o[k] = 0.0;
        o[7] = __longlong_as_double((long long)0xffffffffull);
      }
    }
  }
  P.count[i] = count;
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: what tor_occluded_device refuses, and k; then the scene
int crossings_check(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, const void* list, int64_t n_list, int32_t k,
                    double time_lo, double time_hi, int32_t mode, const void* cross, const void* count) {
  using tor::fail;
  const std::string w = who;
  int rc = tor::list_args(w, ctx, n_rays, list, n_list);
  if (rc != TOR_OK) return rc;
  if (k < 1 || k > TOR_CROSSINGS_MAX)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": k must be in 1 .. TOR_CROSSINGS_MAX (" + std::to_string(TOR_CROSSINGS_MAX) + ")");
  rc = tor::range_args(w, time_lo, time_hi, mode);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && (!rays || !cross || !count)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays, cross or count");
  return tor::scene_args(who, ctx);
}

template <bool BLOCKS, bool MASKED>
void crossings_dispatch(unsigned grid, hipStream_t stream, const tor::XParams& P, const tor::MParams& mk) {
  if (P.k <= tor::kCapSmall)
    hipLaunchKernelGGL((tor::crossings_kernel<BLOCKS, MASKED, tor::kCapSmall>), dim3(grid), dim3(tor::kHitThreads), 0, stream, P, mk);
  else
    hipLaunchKernelGGL((tor::crossings_kernel<BLOCKS, MASKED, tor::kCapLarge>), dim3(grid), dim3(tor::kHitThreads), 0, stream, P, mk);
}

// the launch; the arguments are checked, n_rays > 0 and n_list > 0.  A call without per-ray masks whose mask is 0xFFFFFFFF sees
// every object whatever the group words hold: it runs the unmasked kernels and neither builds nor reads any group state.
int crossings_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, const int32_t* d_list,
                     int64_t n_list, int32_t k, const uint32_t* d_mask, uint32_t mask, double time_lo, double time_hi, int32_t mode,
                     TorCrossing* d_cross, int32_t* d_count, TorHit* d_records, hipStream_t stream) {
  tor::XParams P{};
  tor::MParams mk{};
  bool blocks = false;
  std::string why;
  const bool masked = d_mask != nullptr || mask != 0xFFFFFFFFu;
  int rc = tor::query_setup(who, ctx, time_lo, time_hi, mode, stream, P.q, blocks, why);
  if (rc == TOR_OK && d_records) rc = tor::ensure_obj_cold(who, ctx, stream);  // the records are rebuilt from the by-object records
  if (rc == TOR_OK && masked) rc = tor::masked_setup(ctx, blocks, d_mask, mask, stream, mk);
  if (rc != TOR_OK) return rc;
  P.q.rays = (const double*)d_rays;
  P.q.t_range = d_t_range;
  P.q.n_rays = (long long)n_rays;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.k = k;
  P.cross = (double*)d_cross;
  P.count = d_count;
  P.records = (double*)d_records;
  if (d_records) P.obj_cold = (const double*)ctx->hitq.obj_cold.ptr;
  const unsigned grid = (unsigned)((n_list + tor::kHitThreads - 1) / tor::kHitThreads);
  tor::for_variant(blocks, masked,
                   [&](auto B, auto M) { crossings_dispatch<decltype(B)::value, decltype(M)::value>(grid, stream, P, mk); });
  return tor::query_finish(ctx, stream, "crossings", masked, blocks, why);
}

}  // namespace

extern "C" {

int tor_crossings_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                         int64_t n_list, int32_t k, const uint32_t* d_mask, uint32_t mask, double time_lo, double time_hi, int32_t mode,
                         TorCrossing* d_cross, int32_t* d_count, TorHit* d_records, void* hip_stream) {
  const int rc = crossings_check("tor_crossings_device", ctx, n_rays, d_rays, d_list, n_list, k, time_lo, time_hi, mode, d_cross, d_count);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return crossings_launch("tor_crossings_device", ctx, n_rays, d_rays, d_t_range, d_list, n_list, k, d_mask, mask, time_lo, time_hi, mode,
                          d_cross, d_count, d_records, (hipStream_t)hip_stream);
}

int tor_crossings_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list, int64_t n_list,
                       int32_t k, const uint32_t* masks, uint32_t mask, double time_lo, double time_hi, int32_t mode, TorCrossing* cross,
                       int32_t* count, TorHit* records) {
  const char* who = "tor_crossings_host";
  int rc = crossings_check(who, ctx, n_rays, rays, list, n_list, k, time_lo, time_hi, mode, cross, count);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too, rays that are not listed keep what the caller holds --, the query on the default stream, the
  // outputs back
  const size_t n = (size_t)n_rays, nk = n * (size_t)k;
  tor::HostPart st[7] = {{rays, n * sizeof(TorRay), true, false},
                         {t_range, t_range ? n * 16 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {masks, masks ? n * 4 : 0, true, false},
                         {cross, nk * sizeof(TorCrossing), true, true},
                         {count, n * 4, true, true},
                         {records, records ? nk * sizeof(TorHit) : 0, true, true}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = crossings_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const int32_t>(), n_list, k,
                        st[3].as<const uint32_t>(), mask, time_lo, time_hi, mode, st[4].as<TorCrossing>(), st[5].as<int32_t>(),
                        st[6].as<TorHit>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

}  // extern "C"
