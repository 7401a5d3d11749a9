// tor_nearest.hip -- batched nearest-surface point queries against the uploaded scene (tor_nearest_device / tor_nearest_host,
// include/tor_render.h): for each listed point (p, time) the K objects whose surfaces lie nearest, in order, on gfx950.  What a host
// integrator asks where no ray can: the emitters within a radius of a shading point (light culling before the shadow rays; the
// visibility groups mark the emitters), a distance field for sphere tracing, proximity and contact shading, a contact test.
//
// What a neighbour is.  For point (p, time) and object j
//     c  = the sphere's centre, or MovingSphere.center(time)          (moving_spheres.nim:39-44: centre_at's operations)
//     oc = p - c
//     d  = sqrt(oc.x * oc.x + oc.y * oc.y + oc.z * oc.z) - abs(radius)    (vec3s.nim:23-27 length)
// in float64, unfused, with a correctly rounded sqrt: the signed distance to the surface, negative inside; a negative radius is a
// surface at abs(radius).  Object j is a neighbour iff d is finite and d < d_max (strict; NaN and +-inf distances are none, d_max =
// NaN accepts nothing).  Neighbours are ordered by the key (d, object) ascending, d compared as a double; the query returns the
// first min(total, K) of them.
//
// Why the answer is order independent.  The neighbours of a point are a SET of keys, each a function of the point, d_max and one
// object alone -- nothing couples the objects.  No two keys are equal (the object tells them apart), so "the K smallest keys of the
// set, ascending" is one well-defined list whatever order the objects are visited in.  Inserting the keys one by one into a sorted
// list that keeps its K smallest gives that list for every insertion order: a key among the final K is never displaced (at most
// K - 1 keys are smaller), and a key that is not is displaced by the time the last smaller one has arrived.  For the same reason a
// key may be dropped on sight once K keys that are smaller have been seen, and objects that cannot produce a key among the K
// smallest may be skipped.  (The argument at the head of tor_crossings.hip, word for word; XList, tor_query.hpp, is that list.)
//
//   nearest_kernel<false, MASKED, CAP>  brute force: one listed point per lane; every cold slot of the flat layout in a wave-uniform
//                                       loop (records and radii through the scalar-load view)
//   nearest_kernel<true, MASKED, CAP>   blocks: the culling layout's always-objects in the same loop; the points the boxes do not hold
//                                       for (time outside the range or NaN, beyond the point reach) walk every spatial slot,
//                                       wave-uniform; the others test the top-level boxes wave-uniformly and descend per lane, the
//                                       records of a block loaded and measured as a batch before any is inserted
//   MASKED                              with visibility groups (Sees<true>, masked_setup): object j takes part for point i iff
//                                       groups[j] & mask_i != 0, `object` in the full list's numbering; a box whose OR-word shares no
//                                       bit with the mask is not entered
//   CAP                                 4 (K <= 4) or TOR_NEAREST_MAX = 16: XList in registers, no dynamic indexing, no scratch
//
// abs(radius) is not in the cold record (it holds 1 / r and r * r; sqrt(r * r) is wrong where the square overflows or underflows):
// it comes from a side array by cold slot, built and cached per scene next to the group words (radii_setup).  A padding slot holds
// NaN there, so its distance is NaN and it is no neighbour, whatever its record holds.
//
// The bound shrinks.  While the list holds fewer than K neighbours the bound is d_max; once it is full it is the K-th entry's d.  A
// distance above the bound is dropped; one EQUAL to it goes through the full key compare (a lower object index at the same distance
// must displace the K-th).
//
// The boxes.  For box record {lo, hi} (compute_block_bounds) q = sqrt(dx^2 + dy^2 + dz^2) with d_k = max(lo_k - p_k, 0, p_k - hi_k)
// is the float64 distance from p to the box.  A box is entered iff q == 0, or q < d_max and q <= bound:
//  (a) q == 0: the point is inside the box (or so close that q rounds to 0).  Distances are signed -- p may be deep inside a sphere
//      of the box, its d far below 0 and below a negative K-th bound -- so such a box gives no lower bound and is always entered.
//  (b) the keep side is non-strict: a box at q == bound is entered, as an element at d == bound is compared by its key.
//
// Why culling is exact.  Take a spatial object of the final answer, d its computed distance, for a point that uses the boxes (time
// inside the boxes' range, |p - org| <= reach), and a box (block box or super box) that bounds it.
//  (1) In exact arithmetic the sphere lies in the box shrunk by its inflation: the box bounds the sphere over [time_lo, time_hi] (the
//      centre moves linearly, the hull of the two end spheres holds it) and is then inflated per axis by pad_k >= 1e-6.  For p
//      outside the box the segment from p to the nearest point of the sphere leaves the box's boundary at least min pad_k from the
//      shrunk box, so d_exact >= q_exact + m with m >= 1e-6.
//  (2) Roundings.  Let M bound every magnitude the two computations meet: |c0| + |f| |dc| + |r| over the spatial objects with f the
//      centre's fraction at either end of the time range (so M also bounds the box coordinates and |org|, up to the inflation), and
//      R = |p - org|.  Then |p| <= M + R and |oc| <= 2 M + R.  The centre carries at most 4 roundings relative to M per axis (7 eps M
//      as a vector); oc one relative to |oc| per axis; the length three (squares, sums, square root); the subtraction one relative to
//      |oc| + |r|: |d - d_exact| <= 19 eps M + 6 eps R.  q: lo - p and p - hi one rounding relative to 2 M + R per axis, the length
//      three: |q - q_exact| <= 5 eps (2 M + R).  Together below 32 eps (M + R).  A product that underflows is off by less than
//      2^-1074 absolutely, far below the margin.
//  (3) The point reach (point_reach below, in the manner of hit_reach): R <= reach with 32 eps (M + reach) <= 1e-6 / 4, a quarter of
//      the margin.  Within it d >= q + 0.75e-6 > q for every q > 0.
//  (4) The final answer's keys are at or below the final bound and below d_max, and the bound at any earlier moment is no smaller.
//      So q < d <= bound and q < d < d_max whenever a box that holds such an object is tested: it is entered -- at the top level
//      against the bound at the start of its chunk of 64, at the block boxes of a super box against the bound when the super box is
//      opened, and once more against the current bound just before a block box is opened.  Boxes entered needlessly cost time only.
//  (5) d_max = NaN accepts nothing: such a point visits nothing at all.  d_max = +inf leaves only the bound.
// A point beyond the reach, with a time outside [time_lo, time_hi] or a NaN time (or NaN coordinates: the reach compare fails) walks
// every spatial slot wave-uniformly, as the ray kernels' rays do; when no point can use the boxes (no layout, no finite bounds, no
// ray reach, no point reach) the launch is the brute force and tor_last_note says why.  The hint never changes a bit of the answer.
// TOR_HIT_AUTO also takes the brute force for k > 4 without d_max on a one-level layout, where it measured faster
// (profiles/nearest_rate.txt: random_scene, K = 16); TOR_HIT_BLOCKS still runs the blocks there.
//
// Visiting order.  Index order, as the ray kernels -- with one addition that stays simple: before the index-order pass a lane opens
// the top-level box NEAREST to its point (the smallest squared box distance, found in one wave-uniform pass without the square
// root), which usually fills the list with near objects and so sets a tight bound for everything after it.  That box is left out of
// the index-order pass (an object must be inserted once).  The choice of the first box is a heuristic; exactness rests on (1)-(4).
//
// Float64, unfused (-ffp-contract=off), correctly rounded square root.
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

static_assert(sizeof(TorPoint) == 32 && offsetof(TorPoint, time) == 24, "TorPoint: p, time");
static_assert(sizeof(TorNear) == 16 && offsetof(TorNear, object) == 8 && offsetof(TorNear, inside) == 12, "TorNear: distance, object, inside");
static_assert(TOR_NEAREST_MAX == 16, "the large capacity variant holds TOR_NEAREST_MAX entries");

namespace tor {
namespace {

constexpr int kNearSmall = 4;
constexpr int kNearLarge = TOR_NEAREST_MAX;

struct NParams {
  QParams q;            // the scene and its boxes; rays = the points (4 float64 each), n_rays = n_points, reach2 = the POINT reach
  const double* d_max;  // one float64 per point, or null: +inf
  const double* absr;   // abs(radius) per cold slot of the layout q.cold belongs to; padding slots NaN
  const int* list;      // the points to answer, or null: entry e is point e
  long long n_list;
  int k;                // neighbours per point, 1 .. CAP
  double* near;         // k TorNear per point, 2 float64 words each: distance, then object (low word) and inside (high word)
  int* count;           // one int32 per point
};

struct NPoint {
  double x, y, z, time, d_max;
};

// the signed distance of the point to the object in cold record c whose abs(radius) is ar (NaN for a padding slot: no distance)
template <typename P>
__device__ __forceinline__ double dist_of(P c, double ar, const NPoint& p) {
  double cx, cy, cz;
  centre_at(c, p.time, cx, cy, cz);
  const double ocx = p.x - cx, ocy = p.y - cy, ocz = p.z - cz;
  return __builtin_sqrt(ocx * ocx + ocy * ocy + ocz * ocz) - ar;
}

template <typename P>
__device__ __forceinline__ unsigned object_of(P c) {
  return (unsigned)(int)__double_as_longlong(c[14]);
}

// a neighbour is finite and below d_max; one above the bound is dropped, one equal to it goes through the key compare
template <int CAP>
__device__ __forceinline__ void take(XList<CAP>& L, double d, unsigned object, const NPoint& p) {
  if ((d < p.d_max) && (__builtin_fabs(d) < __builtin_inf()) && !(d > L.bound(p.d_max))) L.insert(d, object);
}

// squared distance from the point to box record bx (NaN box: 0, see box_enter)
template <typename P>
__device__ __forceinline__ double box_dist2(P bx, const NPoint& p) {
  const double dx = __builtin_fmax(__builtin_fmax(bx[0] - p.x, p.x - bx[3]), 0.0);
  const double dy = __builtin_fmax(__builtin_fmax(bx[1] - p.y, p.y - bx[4]), 0.0);
  const double dz = __builtin_fmax(__builtin_fmax(bx[2] - p.z, p.z - bx[5]), 0.0);
  return dx * dx + dy * dy + dz * dz;
}

// the entry test of the file head; a NaN box (padding, empty) is never entered (its maxima drop the NaN operands)
template <typename P>
__device__ __forceinline__ bool box_enter(P bx, const NPoint& p, double bound) {
  const double q = __builtin_sqrt(box_dist2(bx, p));
  return (bx[0] == bx[0]) && ((q == 0.0) || ((q < p.d_max) && (q <= bound)));
}

template <bool BLOCKS, bool MASKED, int CAP>
__global__ __launch_bounds__(kHitThreads) void nearest_kernel(const NParams P, const MParams mk) {
  const QParams& p = P.q;
  const long long e = (long long)blockIdx.x * kHitThreads + threadIdx.x;
  long long i = -1;  // the point of list entry e; -1: past the end of the list, or an entry outside [0, n_points) (skipped)
  if (e < P.n_list) {
    const long long v = P.list ? (long long)P.list[e] : e;
    if (v >= 0 && v < p.n_rays) i = v;
  }
  const bool live = i >= 0;
  unsigned r_mask = 0u;  // (lanes without a point see nothing)
  if constexpr (MASKED) {
    if (live) r_mask = mk.ray_mask ? mk.ray_mask[i] : mk.mask;
  }
  const Sees<MASKED> vis{mk.grp, mk.box_or, r_mask};
  NPoint q{0.0, 0.0, 0.0, 0.0, __builtin_nan("")};  // (lanes without a point: d_max = NaN accepts nothing)
  if (live) {
    const double* s = p.rays + 4 * i;
    q.x = s[0]; q.y = s[1]; q.z = s[2]; q.time = s[3];
    q.d_max = P.d_max ? P.d_max[i] : __builtin_inf();
  }
  const bool seeks = live && (q.d_max == q.d_max);  // d_max = NaN: nothing to look for
  const int K = P.k < CAP ? P.k : CAP;
  // records of a block measured per batch: all 8 with the small list; 4 with the large one, which leaves fewer registers
  constexpr int kBatch = CAP <= kNearSmall ? 8 : 4;
  const qcdptr absr_u = (qcdptr)(uintptr_t)P.absr;
  XList<CAP> L;
  L.init(K);
  // wave-uniform: every lane that seeks and sees the slot measures the same record
  for (int s = 0; s < p.n_uniform; ++s) {
    if (seeks && vis.slot_u(s)) {
      const qcdptr c = (qcdptr)(uintptr_t)(p.cold + 16 * (size_t)s);
      take(L, dist_of(c, absr_u[s], q), object_of(c), q);
    }
  }
  if constexpr (BLOCKS) {
    const double ex = q.x - p.org[0], ey = q.y - p.org[1], ez = q.z - p.org[2];
    const bool boxed = seeks && (q.time >= p.time_lo) && (q.time <= p.time_hi) && (ex * ex + ey * ey + ez * ez <= p.reach2);
    const bool walk = seeks && !boxed;
    if (__ballot(walk) != 0) {  // points the boxes do not hold for: every spatial slot, wave-uniform
      for (int s = 0; s < p.n_spatial; ++s) {
        const int slot = p.spatial_base + s;
        if (walk && vis.slot_u(slot)) {
          const qcdptr c = (qcdptr)(uintptr_t)(p.cold + 16 * (size_t)slot);
          take(L, dist_of(c, absr_u[slot], q), object_of(c), q);
        }
      }
    }
    const int n_top = p.two_level ? p.n_super : p.n_boxes;
    const int top0 = p.two_level ? p.super0 : 0;
    // the top-level box nearest to the point (the file head: visiting order); -1: none the lane sees
    int seed = -1;
    if (__ballot(boxed) != 0) {
      double best = __builtin_inf();
      for (int j = 0; j < n_top; ++j) {
        const qcdptr bx = (qcdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + j));
        const double q2 = box_dist2(bx, q);
        if (boxed && vis.box_u(top0 + j) && (bx[0] == bx[0]) && q2 < best) {
          best = q2;
          seed = j;
        }
      }
    }
    if (boxed) {
      auto test_box = [&](int box) {  // the blocks behind block box `box`, 8 objects each
        for (int fk = 0; fk < p.fanout; ++fk) {
          const int slot0 = p.spatial_base + 8 * (box * p.fanout + fk);
          // the records' loads go out as one batch: no insertion (a branch) between them
#pragma unroll 1
          for (int k0 = 0; k0 < 8; k0 += kBatch) {
            double d[kBatch];
            unsigned o[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
              const int slot = slot0 + k0 + k;
              d[k] = __builtin_nan("");
              o[k] = 0u;
              if (vis.slot(slot)) {
                const qgdptr c = (qgdptr)(uintptr_t)(p.cold + 16 * (size_t)slot);
                d[k] = dist_of(c, P.absr[slot], q);
                o[k] = object_of(c);
              }
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) take(L, d[k], o[k], q);
          }
        }
      };
      // chunk -64 is the seed box alone; then the top-level boxes 64 at a time (scalar loads) without the seed, and per lane the
      // ones at or below the bound
      for (int c0 = -64; c0 < n_top; c0 += 64) {
        unsigned long long m = 0;
        int base = c0;
        if (c0 < 0) {
          base = seed;
          if (seed >= 0 && box_enter((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + seed)), q, L.bound(q.d_max))) m = 1ull;
        } else {
          const int cn = n_top - c0 < 64 ? n_top - c0 : 64;
          const double b0 = L.bound(q.d_max);
          for (int j = 0; j < cn; ++j)
            if (vis.box_u(top0 + c0 + j) && (c0 + j != seed) &&
                box_enter((qcdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + c0 + j)), q, b0))
              m |= 1ull << j;
        }
        while (m != 0) {
          const int top = base + __builtin_ctzll(m);
          m &= m - 1;
          // one level: block box `top` itself.  Two levels: super box `top`, its 8 block boxes, against the bound as it stands now.
          unsigned m8 = 1u;
          int box0 = top;
          if (p.two_level) {
            const double b1 = L.bound(q.d_max);
            m8 = 0u;
            box0 = 8 * top;
            for (int k = 0; k < 8; ++k)
              if (vis.box(box0 + k) && box_enter((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(box0 + k)), q, b1)) m8 |= 1u << k;
          }
          // the bound may have shrunk since the box passed its test (b0 is a chunk old, b1 a super box old): a block box is
          // opened only if it still lies at or below the bound as it stands now
          while (m8 != 0) {
            const int k = __builtin_ctz(m8);
            m8 &= m8 - 1;
            if (box_enter((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(box0 + k)), q, L.bound(q.d_max))) test_box(box0 + k);
          }
        }
      }
    }
  }
  if (!live) return;
  // entries CAP - K .. CAP - 1 are neighbours 0 .. K - 1; unused ones hold distance = 0, object = -1, inside = 0
  double* out = P.near + 2 * (size_t)i * (size_t)P.k;
  int count = 0;
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    const int m = j - (CAP - K);
    if (m < 0) continue;
    const bool has = L.t[j] < __builtin_inf();
    count += has ? 1 : 0;
    const unsigned long long w = has ? (((unsigned long long)(L.t[j] < 0.0 ? 1u : 0u) << 32) | (unsigned long long)L.key[j]) : 0xffffffffull;
    out[2 * m] = has ? L.t[j] : 0.0;
    out[2 * m + 1] = __longlong_as_double((long long)w);
  }
  P.count[i] = count;
}

// Where a POINT may use the boxes (the file head, (2)-(3)): within `reach` of hq.org with 32 eps (M + reach) <= 1e-6 / 4.  M: the
// largest |c0| + |f| |dc| + |r| over the spatial objects, f the centre's fraction at either end of the time range, with a little on
// top for the boxes' own inflation.  Cached per (scene, time range).
void point_reach(TorContext* ctx, const tor::HostAccel& acc, double time_lo, double time_hi) {
  tor::HitQueryState& hq = ctx->hitq;
  const int64_t gen = ctx->n_uploads - ctx->n_cache_hits;
  uint64_t lo_bits, hi_bits;
  std::memcpy(&lo_bits, &time_lo, 8);
  std::memcpy(&hi_bits, &time_hi, 8);
  if (hq.pt_scene == gen && hq.pt_lo == lo_bits && hq.pt_hi == hi_bits) return;
  hq.pt_scene = gen;
  hq.pt_lo = lo_bits;
  hq.pt_hi = hi_bits;
  hq.pt_reach2 = -1.0;
  double M = 0.0;
  for (const tor::HostAccel::Obj& o : acc.spatial) {
    if (!o.valid) continue;
    double f = 0.0;
    if (o.moving) f = std::fmax(std::fabs((time_lo - o.t0) / o.dt), std::fabs((time_hi - o.t0) / o.dt));
    const double m = std::sqrt(o.c0[0] * o.c0[0] + o.c0[1] * o.c0[1] + o.c0[2] * o.c0[2]) +
                     f * std::sqrt(o.dc[0] * o.dc[0] + o.dc[1] * o.dc[1] + o.dc[2] * o.dc[2]) + o.abs_r;
    if (!std::isfinite(m)) return;
    M = std::fmax(M, m);
  }
  M = M * (1.0 + 1e-5) + 1e-5;
  const double eps = 0x1p-53;
  const double reach = 0.25e-6 / (32.0 * eps) * (1.0 - 1e-9) - M;
  if (!(reach > 0.0)) return;
  hq.pt_reach2 = reach * reach * (1.0 - 1e-9);  // (the kernel's |p - org|^2 carries a few roundings)
}

// abs(radius) per cold slot of the layout a launch reads (`blocks`: the culling layout's, else the flat layout's), NaN for a padding
// slot, into hitq.absr: built and cached per scene the way masked_setup builds the group words.  The culling layout's array covers
// the slots behind the padding boxes too.
int radii_setup(const char* who, TorContext* ctx, bool blocks, hipStream_t stream, const double*& d_absr) {
  tor::HitQueryState& hq = ctx->hitq;
  const int lay = blocks ? 1 : 0;
  const int64_t gen = ctx->n_uploads - ctx->n_cache_hits;
  if (hq.absr_scene[lay] != gen) {
    hq.absr_scene[lay] = -1;
    if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the buffer and its host source
    const int64_t n = ctx->n_objects;
    const TorHittableVariant* objs = (const TorHittableVariant*)ctx->scene_bytes.data();
    auto radius_of = [&](const double* c) -> double {  // of the object in cold record c
      if (c[15] == -1.0) return std::nan("");          // padding slot
      int64_t orig;
      std::memcpy(&orig, &c[14], 8);
      if (orig < 0 || orig >= n) return std::nan("");
      return std::fabs(objs[orig].kind == TOR_SPHERE ? objs[orig].u.sphere.radius : objs[orig].u.moving_sphere.radius);
    };
    std::vector<double>& w = hq.absr_host[lay];
    if (blocks) {
      const tor::HostAccel& acc = ctx->accel[0];
      const size_t fan = acc.fanout > 0 ? (size_t)acc.fanout : 1;
      const size_t n_slots = acc.spatial_base + tor::accel_boxes_padded(acc) * fan * tor::kPad;
      if (acc.cold.size() < 16 * n_slots)
        return tor::fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": the culling layout's cold records are short");
      w.assign(n_slots, std::nan(""));
      for (size_t s = 0; s < n_slots; ++s) w[s] = radius_of(&acc.cold[16 * s]);
    } else {
      tor::HostLayout flat;
      std::string err;
      if (!flat_host_layout(ctx, flat, err)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": " + err);
      const size_t n_slots = (size_t)ctx->flat[0].n_sorted;
      if (flat.n_sorted != n_slots || flat.cold.size() < 16 * n_slots)
        return tor::fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": the flat layout's slots do not match the device's");
      w.assign(n_slots, std::nan(""));
      for (size_t s = 0; s < n_slots; ++s) w[s] = radius_of(&flat.cold[16 * s]);
    }
    HIP_TRY(hq.absr[lay].ensure(w.size() * 8 + 64));
    if (!w.empty()) HIP_TRY(hipMemcpyAsync(hq.absr[lay].ptr, w.data(), w.size() * 8, hipMemcpyHostToDevice, stream));
    hq.absr_scene[lay] = gen;
  }
  d_absr = (const double*)hq.absr[lay].ptr;
  return TOR_OK;
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: what tor_crossings_device refuses; then the scene
int nearest_check(const char* who, TorContext* ctx, int64_t n_points, const void* points, const void* list, int64_t n_list, int32_t k,
                  double time_lo, double time_hi, int32_t mode, const void* near, const void* count) {
  using tor::fail;
  const std::string w = who;
  int rc = tor::list_args(w, ctx, n_points, list, n_list);
  if (rc != TOR_OK) return rc;
  if (k < 1 || k > TOR_NEAREST_MAX)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": k must be in 1 .. TOR_NEAREST_MAX (" + std::to_string(TOR_NEAREST_MAX) + ")");
  rc = tor::range_args(w, time_lo, time_hi, mode);
  if (rc != TOR_OK) return rc;
  if (n_points > 0 && n_list > 0 && (!points || !near || !count)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL points, near or count");
  return tor::scene_args(who, ctx);
}

template <bool BLOCKS, bool MASKED>
void nearest_dispatch(unsigned grid, hipStream_t stream, const tor::NParams& P, const tor::MParams& mk) {
  if (P.k <= tor::kNearSmall)
    hipLaunchKernelGGL((tor::nearest_kernel<BLOCKS, MASKED, tor::kNearSmall>), dim3(grid), dim3(tor::kHitThreads), 0, stream, P, mk);
  else
    hipLaunchKernelGGL((tor::nearest_kernel<BLOCKS, MASKED, tor::kNearLarge>), dim3(grid), dim3(tor::kHitThreads), 0, stream, P, mk);
}

// the launch; the arguments are checked, n_points > 0 and n_list > 0.  A call without per-point masks whose mask is 0xFFFFFFFF sees
// every object whatever the group words hold: it runs the unmasked kernels and neither builds nor reads any group state.
int nearest_launch(const char* who, TorContext* ctx, int64_t n_points, const void* d_points, const double* d_max_dist,
                   const int32_t* d_list, int64_t n_list, int32_t k, const uint32_t* d_mask, uint32_t mask, double time_lo,
                   double time_hi, int32_t mode, TorNear* d_near, int32_t* d_count, hipStream_t stream) {
  tor::NParams P{};
  tor::MParams mk{};
  bool blocks = false;
  std::string why;
  const bool masked = d_mask != nullptr || mask != 0xFFFFFFFFu;
  int rc = tor::query_setup(who, ctx, time_lo, time_hi, mode, stream, P.q, blocks, why);
  if (rc == TOR_OK && blocks) {
    tor::point_reach(ctx, ctx->accel[0], time_lo, time_hi);
    if (!(ctx->hitq.pt_reach2 > 0.0)) {  // no point may use the boxes: the flat layout
      rc = tor::query_setup(who, ctx, time_lo, time_hi, TOR_HIT_BRUTE, stream, P.q, blocks, why);
      why = "the block boxes' margin holds for no point (scene too far from the origin)";
    } else if (mode == TOR_HIT_AUTO && k > tor::kNearSmall && !d_max_dist && !P.q.two_level) {
      // measured (profiles/nearest_rate.txt): the large list without a limit has a loose bound, a point enters most of the few
      // boxes of a one-level layout, and the per-lane record loads then cost more than the flat layout's scalar ones
      rc = tor::query_setup(who, ctx, time_lo, time_hi, TOR_HIT_BRUTE, stream, P.q, blocks, why);
      why = "auto: k > 4 without a limit on a one-level layout";
    }
  }
  if (rc == TOR_OK) rc = tor::radii_setup(who, ctx, blocks, stream, P.absr);
  if (rc == TOR_OK && masked) rc = tor::masked_setup(ctx, blocks, d_mask, mask, stream, mk);
  if (rc != TOR_OK) return rc;
  P.q.rays = (const double*)d_points;
  P.q.n_rays = (long long)n_points;
  if (blocks) P.q.reach2 = ctx->hitq.pt_reach2;
  P.d_max = d_max_dist;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.k = k;
  P.near = (double*)d_near;
  P.count = d_count;
  const unsigned grid = (unsigned)((n_list + tor::kHitThreads - 1) / tor::kHitThreads);
  tor::for_variant(blocks, masked,
                   [&](auto B, auto M) { nearest_dispatch<decltype(B)::value, decltype(M)::value>(grid, stream, P, mk); });
  return tor::query_finish(ctx, stream, "nearest", masked, blocks, why);
}

}  // namespace

extern "C" {

int tor_nearest_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, const double* d_max_dist, const int32_t* d_list,
                       int64_t n_list, int32_t k, const uint32_t* d_mask, uint32_t mask, double time_lo, double time_hi, int32_t mode,
                       TorNear* d_near, int32_t* d_count, void* hip_stream) {
  const int rc = nearest_check("tor_nearest_device", ctx, n_points, d_points, d_list, n_list, k, time_lo, time_hi, mode, d_near, d_count);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return nearest_launch("tor_nearest_device", ctx, n_points, d_points, d_max_dist, d_list, n_list, k, d_mask, mask, time_lo, time_hi, mode,
                        d_near, d_count, (hipStream_t)hip_stream);
}

int tor_nearest_host(TorContext* ctx, int64_t n_points, const TorPoint* points, const double* max_dist, const int32_t* list,
                     int64_t n_list, int32_t k, const uint32_t* masks, uint32_t mask, double time_lo, double time_hi, int32_t mode,
                     TorNear* near, int32_t* count) {
  const char* who = "tor_nearest_host";
  int rc = nearest_check(who, ctx, n_points, points, list, n_list, k, time_lo, time_hi, mode, near, count);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too, points that are not listed keep what the caller holds --, the query on the default stream,
  // the outputs back
  const size_t n = (size_t)n_points, nk = n * (size_t)k;
  tor::HostPart st[6] = {{points, n * sizeof(TorPoint), true, false},
                         {max_dist, max_dist ? n * 8 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {masks, masks ? n * 4 : 0, true, false},
                         {near, nk * sizeof(TorNear), true, true},
                         {count, n * 4, true, true}};
  rc = tor::stage_in(ctx, st, 6);
  if (rc != TOR_OK) return rc;
  rc = nearest_launch(who, ctx, n_points, st[0].dev, st[1].as<const double>(), st[2].as<const int32_t>(), n_list, k,
                      st[3].as<const uint32_t>(), mask, time_lo, time_hi, mode, st[4].as<TorNear>(), st[5].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 6);
}

}  // extern "C"
