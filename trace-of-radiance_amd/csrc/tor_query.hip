// tor_query.hip -- batched closest-hit queries against the uploaded scene (tor_hit_device / tor_hit_host, include/tor_render.h):
// the reference's HittableList.hit (hittables_lists.nim:48-55 over spheres.nim:28-49 / moving_spheres.nim:39-67) for rays the
// caller supplies, on gfx950.  Kernels, parameter struct and entry points of their own: nothing here is shared with the integrator
// (tor_kernels.hip, KParams, kernel/*.inc), whose kernels stay as they are.
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

static_assert(sizeof(TorRay) == 56 && offsetof(TorRay, direction) == 24 && offsetof(TorRay, time) == 48,
              "TorRay: origin, direction, time (primitives/rays.nim)");
static_assert(sizeof(TorHit) == 64 && offsetof(TorHit, normal) == 24 && offsetof(TorHit, t) == 48 && offsetof(TorHit, object) == 56 &&
                  offsetof(TorHit, front_face) == 60,
              "TorHit: HitRecord (physics/core.nim:30-36) with the object index in place of the material");

namespace tor {
namespace {

typedef const double __attribute__((address_space(4))) * qcdptr;  // scalar view: wave-uniform records come through s_load
typedef const double __attribute__((address_space(1))) * qgdptr;  // global: per-lane records

constexpr int kHitThreads = 256;

struct QParams {
  const double* rays;     // 7 float64 per ray (TorRay)
  const double* t_range;  // 2 float64 per ray {t_min, t_max}, or null: render.nim's (0.001, +inf)
  double* hits;           // 8 float64 words per ray (TorHit)
  long long n_rays;
  const double* cold;     // cold records (tor_kernels.hpp), 16 float64 per slot
  int n_uniform;          // slots [0, n_uniform) go through the wave-uniform loop: the whole flat layout, or the always-layout
  // blocks only:
  int spatial_base;       // block b owns cold slots spatial_base + 8 b .. + 8
  int n_spatial;          // spatial slots (8 per block)
  const double* bnd;      // 8 float64 per box record {lo xyz, hi xyz, -, -} (compute_block_bounds)
  int n_boxes;            // block boxes; box b stands for blocks [b fanout, (b + 1) fanout)
  int fanout;
  int two_level;          // the top-level loop tests the super boxes (records super0 + s, s < n_super) instead of the block boxes
  int super0, n_super;
  double time_lo, time_hi;  // the ray-time range the boxes hold for
  double org[3];            // centre of the spatial objects' bounding box ...
  double reach2;            // ... and the squared distance from it within which an origin may use the boxes (< 0: none may)
  double a_min;             // smallest |d|^2 that may use the boxes
};

struct QRay {
  double ox, oy, oz, dx, dy, dz, time, t_min, t_max, a;
};

struct QBest {
  double t;
  int orig;  // original index of the winner (ties: the lowest)
  int slot;  // its cold slot, -1 = no hit
};

// centre of the object in cold record c at the ray's time: moving_spheres.nim:39-44 (center0 + (time - time0) / (time1 - time0) *
// (center1 - center0); the record carries center1 - center0 and time1 - time0), or the sphere's centre
template <typename P>
__device__ __forceinline__ void centre_at(P c, double time, double& cx, double& cy, double& cz) {
  cx = c[0]; cy = c[1]; cz = c[2];
  if ((int)__double_as_longlong(c[13]) & 1) {
    const double f = (time - c[7]) / c[8];
    cx = cx + c[3] * f; cy = cy + c[4] * f; cz = cz + c[5] * f;
  }
}

// spheres.nim:29-48 / moving_spheres.nim:47-66 for the object in cold record c, in the reference's operation order, reduced to the
// order-independent update of the closest hit
template <typename P>
__device__ __forceinline__ void exact_test(P c, int slot, const QRay& r, QBest& b) {
  const double r2 = c[15];
  if (r2 == -1.0) return;  // padding slot (a real record holds radius * radius: >= 0 or NaN)
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);
  const double ocx = r.ox - cx, ocy = r.oy - cy, ocz = r.oz - cz;
  const double hb = ocx * r.dx + ocy * r.dy + ocz * r.dz;
  const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
  const double disc = hb * hb - r.a * cc;
  if (disc > 0.0) {
    const double root = __builtin_sqrt(disc);
    double sol = (-hb - root) / r.a;
    bool ok = (r.t_min < sol) && (sol < r.t_max);
    if (!ok) {
      sol = (-hb + root) / r.a;
      ok = (r.t_min < sol) && (sol < r.t_max);
    }
    if (ok) {
      const int orig = (int)__double_as_longlong(c[14]);
      if (sol < b.t || (sol == b.t && orig < b.orig)) {
        b.t = sol;
        b.orig = orig;
        b.slot = slot;
      }
    }
  }
}

// float64 slab test of box record bx, clipped at t = 0: the integrator's test (integrate_loop_boxes64.inc); conservative for the
// inflated boxes of compute_block_bounds
template <typename P>
__device__ __forceinline__ bool slab(P bx, const QRay& r, double ix, double iy, double iz) {
  const double tx0 = (bx[0] - r.ox) * ix, tx1 = (bx[3] - r.ox) * ix;
  const double ty0 = (bx[1] - r.oy) * iy, ty1 = (bx[4] - r.oy) * iy;
  const double tz0 = (bx[2] - r.oz) * iz, tz1 = (bx[5] - r.oz) * iz;
  const double t_in = __builtin_fmax(__builtin_fmax(__builtin_fmin(tx0, tx1), __builtin_fmin(ty0, ty1)),
                                     __builtin_fmax(__builtin_fmin(tz0, tz1), 0.0));
  const double t_out = __builtin_fmin(__builtin_fmin(__builtin_fmax(tx0, tx1), __builtin_fmax(ty0, ty1)), __builtin_fmax(tz0, tz1));
  return t_in <= t_out;
}

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
  // wave-uniform: every lane tests the same record
  for (int s = 0; s < p.n_uniform; ++s) exact_test((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)s), s, r, b);
  if constexpr (BLOCKS) {
    const double ex = r.ox - p.org[0], ey = r.oy - p.org[1], ez = r.oz - p.org[2];
    const bool boxed = live && (r.t_min >= 0.0) && (r.time >= p.time_lo) && (r.time <= p.time_hi) &&
                       (ex * ex + ey * ey + ez * ez <= p.reach2) && (r.a >= p.a_min);
    const bool walk = live && !boxed;
    if (__ballot(walk) != 0) {  // rays the boxes do not hold for: every spatial slot, wave-uniform
      for (int s = 0; s < p.n_spatial; ++s) {
        const int slot = p.spatial_base + s;
        if (walk) exact_test((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)slot), slot, r, b);
      }
    }
    if (boxed) {
      const double ix = 1.0 / r.dx, iy = 1.0 / r.dy, iz = 1.0 / r.dz;
      auto test_box = [&](int box) {  // the 8 objects of each block behind block box `box`
        for (int fk = 0; fk < p.fanout; ++fk) {
          const int slot0 = p.spatial_base + 8 * (box * p.fanout + fk);
          for (int k = 0; k < 8; ++k) exact_test((qgdptr)(uintptr_t)(p.cold + 16 * (size_t)(slot0 + k)), slot0 + k, r, b);
        }
      };
      const int n_top = p.two_level ? p.n_super : p.n_boxes;
      const int top0 = p.two_level ? p.super0 : 0;
      // the top-level boxes 64 at a time, wave-uniform (scalar loads); then per lane the ones its ray enters
      for (int c0 = 0; c0 < n_top; c0 += 64) {
        const int cn = n_top - c0 < 64 ? n_top - c0 : 64;
        unsigned long long m = 0;
        for (int j = 0; j < cn; ++j)
          if (slab((qcdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + c0 + j)), r, ix, iy, iz)) m |= 1ull << j;
        while (m != 0) {
          const int top = c0 + __builtin_ctzll(m);
          m &= m - 1;
          if (!p.two_level) {
            test_box(top);
            continue;
          }
          // super box `top`: its 8 block boxes (NaN padding boxes are never entered)
          unsigned m8 = 0;
          for (int k = 0; k < 8; ++k)
            if (slab((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(8 * top + k)), r, ix, iy, iz)) m8 |= 1u << k;
          while (m8 != 0) {
            const int k = __builtin_ctz(m8);
            m8 &= m8 - 1;
            test_box(8 * top + k);
          }
        }
      }
    }
  }
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

// Where the boxes of `bnd` (compute_block_bounds for acc) hold for the reference's rounding (the head of this file): a hit the reference
// accepts on a spatial object of radius r from an origin at distance |oc| lies at most 6 eps (|oc|^2 + r^2) / r outside the sphere, and
// every box is inflated by at least 1e-6.  With 16 eps (|oc|^2 + r_max^2) / r_min <= 1e-6 / 4, over 10x margin, the hit lies inside
// its box.  |oc| <= |o - org| + half the diagonal of the boxes' union, so origins within `reach` of org qualify.  a_min keeps the
// test's products clear of the subnormal range (an underflowed product's error is absolute, not relative): a * r_min^2 >= 2^-1000.
void hit_reach(const tor::HostAccel& acc, const std::vector<double>& bnd, tor::HitQueryState& hq) {
  hq.reach2 = -1.0;
  hq.a_min = INFINITY;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t b = 0; b < acc.n_boxes; ++b) {
    const double* c = &bnd[8 * b];
    if (c[0] != c[0]) continue;  // NaN: empty box
    for (int k = 0; k < 3; ++k) { lo[k] = std::fmin(lo[k], c[k]); hi[k] = std::fmax(hi[k], c[3 + k]); }
  }
  double r_min = INFINITY, r_max = 0.0;
  for (const tor::HostAccel::Obj& o : acc.spatial)
    if (o.valid) { r_min = std::fmin(r_min, o.abs_r); r_max = std::fmax(r_max, o.abs_r); }
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) || !(r_min > 0.0) || !std::isfinite(r_max)) return;
  const double eps = 0x1p-53;
  double half_diag = 0.0;
  for (int k = 0; k < 3; ++k) {
    hq.org[k] = 0.5 * lo[k] + 0.5 * hi[k];
    half_diag += (hi[k] - lo[k]) * (hi[k] - lo[k]);
  }
  half_diag = 0.5 * std::sqrt(half_diag) * (1.0 + 1e-9);
  const double oc2 = 0.25e-6 * r_min / (16.0 * eps) - r_max * r_max;  // the largest |oc|^2 the margin covers
  if (!(oc2 > 0.0) || !std::isfinite(oc2)) return;
  const double reach = std::sqrt(oc2) * (1.0 - 1e-9) - half_diag;
  if (!(reach > 0.0)) return;
  hq.reach2 = reach * reach * (1.0 - 1e-9);  // (the kernel's |o - org|^2 carries a few roundings)
  hq.a_min = 0x1p-1000 / (r_min * r_min);
}

// layouts, block bounds and the launch; the arguments are checked and n_rays > 0
int hit_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, double time_lo,
               double time_hi, int32_t mode, void* d_hits, hipStream_t stream) {
  using tor::fail;
  using tor::fail_hip;
  const std::string w = who;
  tor::HitQueryState& hq = ctx->hitq;
  // one stream per context while launches are in flight (tor_render.h): neither the context's last render launch nor its last query
  // may still be running on another stream
  if (ctx->launches > 0 && ctx->last_stream_valid && ctx->last_stream != (void*)stream) {
    const hipError_t q = hipEventQuery(ctx->ev_stop[ctx->last_slot]);
    if (q == hipErrorNotReady)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context's last render launch is still running on a different stream -- launches "
                                                "of one context that may overlap must use ONE stream (or use one context per stream)");
    if (q != hipSuccess) return fail_hip(q, "hipEventQuery");
  }
  if (hq.launched && hq.stream != (void*)stream) {
    const hipError_t q = hipEventQuery(hq.ev_done);
    if (q == hipErrorNotReady)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context's last query is still running on a different stream -- launches of one "
                                                "context that may overlap must use ONE stream (or use one context per stream)");
    if (q != hipSuccess) return fail_hip(q, "hipEventQuery");
  }
  if (!hq.ev_done) HIP_TRY(hipEventCreateWithFlags(&hq.ev_done, hipEventDisableTiming));

  bool blocks = false;
  std::string why;
  if (mode != TOR_HIT_BRUTE) {
    const int rc = tor::ensure_layouts(ctx, TOR_ACCEL_BLOCKS);
    if (rc != TOR_OK) return rc;
    const tor::HostAccel& acc = ctx->accel[0];
    if (!acc.available) {
      why = "the scene has no culling layout";
    } else {
      // block bounds cached per (scene, time range); the render path's bounds ring is not touched
      const int64_t gen = ctx->n_uploads - ctx->n_cache_hits;
      uint64_t lo_bits, hi_bits;
      std::memcpy(&lo_bits, &time_lo, 8);
      std::memcpy(&hi_bits, &time_hi, 8);
      if (hq.bnd_scene != gen || hq.bnd_lo != lo_bits || hq.bnd_hi != hi_bits) {
        hq.bnd_scene = -1;
        if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the buffer and its host source
        hq.bnd_ok = tor::compute_block_bounds(acc, time_lo, time_hi, hq.bnd_host);
        if (hq.bnd_ok) {
          hit_reach(acc, hq.bnd_host, hq);
          const size_t bytes = hq.bnd_host.size() * 8;
          HIP_TRY(hq.bnd.ensure(bytes));
          HIP_TRY(hipMemcpyAsync(hq.bnd.ptr, hq.bnd_host.data(), bytes, hipMemcpyHostToDevice, stream));
        }
        hq.bnd_scene = gen;
        hq.bnd_lo = lo_bits;
        hq.bnd_hi = hi_bits;
      }
      if (!hq.bnd_ok) why = "no finite block bounds for the time range";
      else if (!(hq.reach2 > 0.0)) why = "the block boxes' margin holds for no ray origin (radii too small)";
      else blocks = true;
    }
  }
  if (!blocks) {
    const int rc = tor::ensure_layouts(ctx, 0);
    if (rc != TOR_OK) return rc;
  }

  tor::QParams p{};
  p.rays = (const double*)d_rays;
  p.t_range = d_t_range;
  p.hits = (double*)d_hits;
  p.n_rays = (long long)n_rays;
  if (blocks) {
    const tor::HostAccel& acc = ctx->accel[0];
    const size_t n_bnd_p = tor::accel_boxes_padded(acc);
    p.cold = ctx->d_accel[0].always.cold;
    p.n_uniform = (int)acc.spatial_base;
    p.spatial_base = (int)acc.spatial_base;
    p.n_spatial = (int)(acc.n_blocks * tor::kPad);
    p.bnd = (const double*)hq.bnd.ptr;
    p.n_boxes = (int)acc.n_boxes;
    p.fanout = acc.fanout > 0 ? acc.fanout : 1;
    p.two_level = acc.two_level ? 1 : 0;
    p.super0 = (int)(n_bnd_p + 1);
    p.n_super = (int)(n_bnd_p / tor::kPad);
    p.time_lo = time_lo;
    p.time_hi = time_hi;
    for (int k = 0; k < 3; ++k) p.org[k] = hq.org[k];
    p.reach2 = hq.reach2;
    p.a_min = hq.a_min;
  } else {
    p.cold = ctx->flat[0].cold;
    p.n_uniform = ctx->flat[0].n_sorted;
  }
  const unsigned grid = (unsigned)((n_rays + tor::kHitThreads - 1) / tor::kHitThreads);
  if (blocks) hipLaunchKernelGGL(tor::hit_kernel<true>, dim3(grid), dim3(tor::kHitThreads), 0, stream, p);
  else hipLaunchKernelGGL(tor::hit_kernel<false>, dim3(grid), dim3(tor::kHitThreads), 0, stream, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(hq.ev_done, stream));
  hq.launched = true;
  hq.stream = (void*)stream;
  tor::set_last_note(blocks ? std::string("hit: blocks")
                            : std::string("hit: brute force") + (why.empty() ? std::string() : " (" + why + ")"));
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
  int rc = hit_args("tor_hit_host", ctx, n_rays, rays, time_lo, time_hi, mode, hits);
  if (rc != TOR_OK) return rc;
  if (!ctx->scene_ready) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_hit_host: no scene uploaded");
  if (n_rays == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  // copy in, the device query on the default stream, copy out (blocking)
  const size_t ray_bytes = (size_t)n_rays * sizeof(TorRay), range_bytes = t_range ? (size_t)n_rays * 16 : 0;
  const size_t hit_bytes = (size_t)n_rays * sizeof(TorHit);
  tor::HitQueryState& hq = ctx->hitq;
  // blocking entry: it waits for the context's last render launch and last query, on whatever stream they run, where the
  // asynchronous entry would refuse a different stream (the staging buffer below may be reallocated too)
  if (ctx->launches > 0) HIP_TRY(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));
  HIP_TRY(hq.io.ensure(ray_bytes + range_bytes + hit_bytes));
  char* base = (char*)hq.io.ptr;
  HIP_TRY(hipMemcpy(base, rays, ray_bytes, hipMemcpyHostToDevice));
  if (t_range) HIP_TRY(hipMemcpy(base + ray_bytes, t_range, range_bytes, hipMemcpyHostToDevice));
  rc = hit_launch("tor_hit_host", ctx, n_rays, base, t_range ? (const double*)(base + ray_bytes) : nullptr, time_lo, time_hi, mode,
                  base + ray_bytes + range_bytes, nullptr);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipMemcpy(hits, base + ray_bytes + range_bytes, hit_bytes, hipMemcpyDeviceToHost));
  return TOR_OK;
}

}  // extern "C"
