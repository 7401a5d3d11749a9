// tor_query.hpp -- what the query families (tor_query.hip, tor_radiance.hip, tor_bounce.hip, tor_occluded.hip, tor_crossings.hip,
// tor_nearest.hip) share.  Device: the closest-hit query's exact test and slab test (the head of tor_query.hip says why they are
// exact; the descent itself is tor_query_descent.inc), the visibility test `Sees`, the kernel argument struct with its optional mask
// part, a kernel's prologue (list entry -> ray, the ray's load), the TorHit record's stores and the ordered queries' register-resident
// sorted list `XList`.  Host: the one copy of the glue around a launch --
// argument checks, stream rule, layouts and cached block bounds, group words, by-object records, the
// launch's tail and note, the blocking entries' wait and staging.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "tor_context.hpp"

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

// visibility groups (tor_scene_groups): what a masked kernel gets next to its QParams
struct MParams {
  const unsigned* grp;       // one group word per cold slot of the layout p.cold belongs to (padding slots: 0)
  const unsigned* box_or;    // blocks only: per box record of p.bnd the OR of the words behind it (block box: its fanout * 8 slots)
  const unsigned* ray_mask;  // one mask per ray, or null: every ray uses `mask`
  unsigned mask;
};

typedef const unsigned __attribute__((address_space(4))) * qcuptr;  // scalar view of the group words, as qcdptr is of the records

// What the descent (tor_query_descent.inc) asks before it touches a slot or a box: does this lane's ray see anything there?
// _u: wave-uniform index, read through a scalar load.  Sees<false> answers yes without reading anything.
template <bool MASKED>
struct Sees {
  const unsigned* grp;
  const unsigned* box_or;
  unsigned m;  // the lane's mask
  __device__ __forceinline__ bool slot_u(int s) const {
    if constexpr (MASKED) return (((qcuptr)(uintptr_t)grp)[s] & m) != 0u;
    else return true;
  }
  __device__ __forceinline__ bool slot(int s) const {
    if constexpr (MASKED) return (grp[s] & m) != 0u;
    else return true;
  }
  __device__ __forceinline__ bool box_u(int rec) const {
    if constexpr (MASKED) return (((qcuptr)(uintptr_t)box_or)[rec] & m) != 0u;
    else return true;
  }
  __device__ __forceinline__ bool box(int rec) const {
    if constexpr (MASKED) return (box_or[rec] & m) != 0u;
    else return true;
  }
};

// A kernel's single argument: the family's parameters and, in a masked instantiation only, the group words behind them (so the
// unmasked kernarg segment holds the parameters alone)
template <typename PARAMS, bool MASKED>
struct KArgs {
  PARAMS P;
};
template <typename PARAMS>
struct KArgs<PARAMS, true> {
  PARAMS P;
  MParams mk;
};

struct QRay {
  double ox, oy, oz, dx, dy, dz, time, t_min, t_max, a;
};

struct QBest {
  double t;
  int orig;  // original index of the winner (ties: the lowest)
  int slot;  // its cold slot, -1 = no hit
};

// the ray of list entry `e` (list null: entry e is ray e), or -1: past the end of the list, or an entry outside [0, n_rays) (skipped).
// The fields come by reference so that each is read where it is used, as in the kernels' own text: by value the compiler orders two
// compares the other way round.
__device__ __forceinline__ long long listed_ray(const int* const& list, const long long& n_list, const long long& n_rays, long long e) {
  if (e >= n_list) return -1;
  const long long i = list ? (long long)list[e] : e;
  return (i >= 0 && i < n_rays) ? i : -1;
}

// ray i of `rays` (7 float64 per ray) with its range from t_range, or render.nim:34's (0.001, +inf) without one; r.a stays with the
// caller, who computes it for every lane
__device__ __forceinline__ void load_ray(QRay& r, const double* rays, const double* t_range, long long i) {
  const double* q = rays + 7 * i;
  r.ox = q[0]; r.oy = q[1]; r.oz = q[2];
  r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
  r.time = q[6];
  if (t_range) {
    r.t_min = t_range[2 * i];
    r.t_max = t_range[2 * i + 1];
  } else {
    r.t_min = 0.001;
    r.t_max = __builtin_inf();
  }
}

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

// TorHit for a miss: object -1, every other field 0
__device__ __forceinline__ void write_miss_record(double* o) {
  for (int k = 0; k < 7; ++k) o[k] = 0.0;
  o[7] = __longlong_as_double((long long)0xffffffffull);
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

// The K smallest (t, key) pairs seen so far, ascending, in entries CAP - K .. CAP - 1: the sorted list of the ordered queries
// (tor_crossings.hip: t a root, key = object * 2 + which; tor_nearest.hip: t a distance, key = object).  The entries in front
// hold -inf and are never displaced, unused entries hold +inf (no element has an infinite t).  Every index below is a
// compile-time constant: the list lives in registers.
template <int CAP>
struct XList {
  double t[CAP];
  unsigned key[CAP];  // ascending at equal t: the lower object first (crossings: then which 0 before 1)

  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      t[j] = j < CAP - k ? -__builtin_inf() : __builtin_inf();
      key[j] = 0xffffffffu;
    }
  }
  // t_max while fewer than K elements are held, else the K-th's t (NaN for t_max = NaN: no compare with it holds)
  __device__ __forceinline__ double bound(double t_max) const { return t[CAP - 1] < __builtin_inf() ? t[CAP - 1] : t_max; }
  // one pass of insertion: the new element sinks in where it belongs and carries the displaced ones along; the largest falls off
  __device__ __forceinline__ void insert(double nt, unsigned nk) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      const bool lt = (nt < t[j]) || (nt == t[j] && nk < key[j]);
      const double ot = t[j];
      const unsigned ok = key[j];
      t[j] = lt ? nt : ot;
      key[j] = lt ? nk : ok;
      nt = lt ? ot : nt;
      nk = lt ? ok : nk;
    }
  }
};

// ---- host side ----------------------------------------------------------------------------------------------------------

constexpr int64_t kMaxItems = (int64_t)0x7fffffff * kHitThreads;  // one lane per ray or list entry, at most 2^31 - 1 workgroups

// The argument checks the entries share; none needs a device or reads *ctx (the CPU suite runs these).  Each entry calls them in the
// order its refusals are documented in and adds its own NULL-pointer (and k) check.
int count_args(const std::string& w, TorContext* ctx, int64_t n_rays) {
  using tor::fail;
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (n_rays < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_rays < 0");
  if (n_rays > kMaxItems) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_rays above 2^31 - 1 workgroups of 256 rays");
  return TOR_OK;
}

// count_args and the list rule
int list_args(const std::string& w, TorContext* ctx, int64_t n_rays, const void* list, int64_t n_list) {
  using tor::fail;
  const int rc = count_args(w, ctx, n_rays);
  if (rc != TOR_OK) return rc;
  if (n_list < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_list < 0");
  if (!list && n_list != n_rays) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": without a list n_list must be n_rays");
  if (n_list > kMaxItems) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_list above 2^31 - 1 workgroups of 256 entries");
  return TOR_OK;
}

// the time range and the mode
int range_args(const std::string& w, double time_lo, double time_hi, int32_t mode) {
  using tor::fail;
  if (!std::isfinite(time_lo) || !std::isfinite(time_hi) || time_lo > time_hi)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the time range must be finite with time_lo <= time_hi");
  if (mode < TOR_HIT_AUTO || mode > TOR_HIT_BLOCKS)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": mode must be TOR_HIT_AUTO (0), TOR_HIT_BRUTE (1) or TOR_HIT_BLOCKS (2)");
  return TOR_OK;
}

// the last of an entry's checks: a scene must be uploaded (the entry then returns on an empty call and sets the context's device)
int scene_args(const char* who, TorContext* ctx) {
  if (!ctx->scene_ready) return tor::fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": no scene uploaded");
  return TOR_OK;
}

// Where the boxes of `bnd` (compute_block_bounds for acc) hold for the reference's rounding (the head of tor_query.hip): tor_scene.hpp
// block_reach, shared with the integrator's float64 block loop.
void hit_reach(const tor::HostAccel& acc, const std::vector<double>& bnd, tor::HitQueryState& hq) {
  tor::block_reach(acc, bnd, hq.org, &hq.reach2, &hq.a_min);
}

// The one-stream-per-context rule of a query launch on `stream` (tor_render.h): neither the context's last render launch nor its
// last query may still be running on another stream.  Creates the event the launch records when it is done.
int query_stream_rule(const char* who, TorContext* ctx, hipStream_t stream) {
  using tor::fail;
  using tor::fail_hip;
  const std::string w = who;
  tor::HitQueryState& hq = ctx->hitq;
  {
    const int rc = tor::last_render_allows(ctx, (void*)stream, who, ": the context's last render launch is still running on a different stream -- launches "
                                                                    "of one context that may overlap must use ONE stream (or use one context per stream)");
    if (rc != TOR_OK) return rc;
  }
  if (hq.launched && hq.stream != (void*)stream) {
    const hipError_t q = hipEventQuery(hq.ev_done);
    if (q == hipErrorNotReady)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context's last query is still running on a different stream -- launches of one "
                                                "context that may overlap must use ONE stream (or use one context per stream)");
    if (q != hipSuccess) return fail_hip(q, "hipEventQuery");
  }
  if (!hq.ev_done) HIP_TRY(hipEventCreateWithFlags(&hq.ev_done, hipEventDisableTiming));
  return TOR_OK;
}

// The host side of a query launch on `stream` (the caller has checked its arguments): the one-stream-per-context rule, the layouts
// and the block bounds cached per (scene, time range), and the scene part of p -- the culling layout's (blocks = true) when mode is
// not TOR_HIT_BRUTE and the scene has one with finite bounds and a usable margin, else the flat layout's (`why` says why, if mode
// asked for the blocks).  Used by the hit queries (tor_query.hip), the radiance queries (tor_radiance.hip) and the path steps
// (tor_bounce.hip).
int query_setup(const char* who, TorContext* ctx, double time_lo, double time_hi, int32_t mode, hipStream_t stream, QParams& p,
                bool& blocks, std::string& why) {
  using tor::fail;
  tor::HitQueryState& hq = ctx->hitq;
  {
    const int rc = query_stream_rule(who, ctx, stream);
    if (rc != TOR_OK) return rc;
  }

  blocks = false;
  why.clear();
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
  return TOR_OK;
}

// the flat layout over the whole uploaded list, built on the host: its cold records name the objects
bool flat_host_layout(TorContext* ctx, tor::HostLayout& lay, std::string& err) {
  const int64_t n = ctx->n_objects;
  std::vector<int64_t> ids((size_t)n);
  for (int64_t i = 0; i < n; ++i) ids[(size_t)i] = i;
  return tor::build_layout((const TorHittableVariant*)ctx->scene_bytes.data(), ids, lay, err, nullptr);
}

// The group words of a masked launch, after query_setup (`blocks`: which layout p.cold belongs to), into mk: one word per cold slot
// of that layout -- the object's word (tor_scene_groups; 0xFFFFFFFF without any), 0 for a padding slot -- and, for the culling
// layout, behind them one OR-word per box record of `bnd`: a block box over the fanout * 8 slots it stands for, a super box over its
// 8 block boxes, 0 for padding and slack records.  Cached per layout; rebuilt when the words or the scene change.
int masked_setup(TorContext* ctx, bool blocks, const uint32_t* d_mask, uint32_t mask, hipStream_t stream, MParams& mk) {
  tor::HitQueryState& hq = ctx->hitq;
  const int lay = blocks ? 1 : 0;
  const int64_t gen = ctx->n_uploads - ctx->n_cache_hits;
  const tor::HostAccel& acc = ctx->accel[0];
  const size_t n_slots = blocks ? acc.spatial_base + acc.n_blocks * tor::kPad : (size_t)ctx->flat[0].n_sorted;
  if (hq.grp_scene[lay] != gen || hq.grp_gen[lay] != hq.groups_gen) {
    hq.grp_scene[lay] = -1;
    if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the buffer and its host source
    const int64_t n = ctx->n_objects;
    auto word_of = [&](const double* c) -> uint32_t {  // of the object in cold record c
      if (c[15] == -1.0) return 0u;                    // padding slot
      int64_t orig;
      std::memcpy(&orig, &c[14], 8);
      if (orig < 0 || orig >= n) return 0u;
      return hq.groups.empty() ? 0xFFFFFFFFu : hq.groups[(size_t)orig];
    };
    std::vector<uint32_t>& w = hq.grp_host[lay];
    if (blocks) {
      if (acc.cold.size() < 16 * n_slots) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "masked query: the culling layout's cold records are short");
      const size_t n_bnd_p = tor::accel_boxes_padded(acc), n_super_p = (n_bnd_p / tor::kPad + tor::kPad - 1) / tor::kPad * tor::kPad;
      w.assign(n_slots + n_bnd_p + 1 + n_super_p + 1, 0u);
      for (size_t s = 0; s < n_slots; ++s) w[s] = word_of(&acc.cold[16 * s]);
      uint32_t* box = w.data() + n_slots;
      const size_t fan = acc.fanout > 0 ? (size_t)acc.fanout : 1;
      for (size_t b = 0; b < acc.n_boxes; ++b)
        for (size_t s = b * fan * tor::kPad; s < (b + 1) * fan * tor::kPad && s < acc.n_blocks * tor::kPad; ++s)
          box[b] |= w[acc.spatial_base + s];
      for (size_t b = 0; b < acc.n_boxes; ++b) box[n_bnd_p + 1 + b / tor::kPad] |= box[b];
    } else {
      // the flat layout's slot order: the layout ensure_layouts built, built again on the host
      tor::HostLayout flat;
      std::string err;
      if (!flat_host_layout(ctx, flat, err)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "masked query: " + err);
      if (flat.n_sorted != n_slots || flat.cold.size() < 16 * n_slots)
        return tor::fail(TOR_ERR_INVALID_ARGUMENT, "masked query: the flat layout's slots do not match the device's");
      w.assign(n_slots, 0u);
      for (size_t s = 0; s < n_slots; ++s) w[s] = word_of(&flat.cold[16 * s]);
    }
    HIP_TRY(hq.grp[lay].ensure(w.size() * 4 + 64));
    if (!w.empty()) HIP_TRY(hipMemcpyAsync(hq.grp[lay].ptr, w.data(), w.size() * 4, hipMemcpyHostToDevice, stream));
    hq.grp_scene[lay] = gen;
    hq.grp_gen[lay] = hq.groups_gen;
  }
  mk.grp = (const unsigned*)hq.grp[lay].ptr;
  mk.box_or = mk.grp + n_slots;
  mk.ray_mask = (const unsigned*)d_mask;
  mk.mask = mask;
  return TOR_OK;
}

// The cold records by ORIGINAL index, 16 float64 per object, in hitq.obj_cold: what scatter_kernel looks the material up in by
// TorHit.object and crossings_kernel rebuilds its records from.  Cached per scene; this is its only filler.  `who` prefixes a
// layout error.
int ensure_obj_cold(const char* who, TorContext* ctx, hipStream_t stream) {
  tor::HitQueryState& hq = ctx->hitq;
  const int64_t gen = ctx->n_uploads - ctx->n_cache_hits;
  if (hq.obj_scene == gen) return TOR_OK;
  hq.obj_scene = -1;
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the buffer and its host source
  const int64_t n = ctx->n_objects;
  tor::HostLayout lay;
  std::string err;
  if (!flat_host_layout(ctx, lay, err)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, std::string(who) + ": " + err);
  hq.obj_cold_host.assign((size_t)(n > 0 ? n : 1) * 16, 0.0);
  for (size_t s = 0; s < lay.n_sorted && n > 0; ++s) {
    const double* c = &lay.cold[16 * s];
    if (c[15] == -1.0) continue;  // padding slot
    int64_t orig;
    std::memcpy(&orig, &c[14], 8);
    if (orig >= 0 && orig < n) std::memcpy(&hq.obj_cold_host[16 * (size_t)orig], c, 16 * sizeof(double));
  }
  const size_t bytes = hq.obj_cold_host.size() * sizeof(double);
  HIP_TRY(hq.obj_cold.ensure(bytes));
  HIP_TRY(hipMemcpyAsync(hq.obj_cold.ptr, hq.obj_cold_host.data(), bytes, hipMemcpyHostToDevice, stream));
  hq.obj_scene = gen;
  return TOR_OK;
}

// f(BLOCKS, MASKED) with the two flags as std::bool_constant: a launch picks its kernel's instantiation in one place
template <typename F>
void for_variant(bool blocks, bool masked, F&& f) {
  if (blocks && masked) f(std::true_type{}, std::true_type{});
  else if (blocks) f(std::true_type{}, std::false_type{});
  else if (masked) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}

// the kernel argument of a launch: P and, for a masked instantiation, mk
template <bool MASKED, typename PARAMS>
KArgs<PARAMS, MASKED> kargs(const PARAMS& P, const MParams& mk) {
  if constexpr (MASKED) return {P, mk};
  else return {P};
}

// After a query's launch on `stream`: the launch's error, the event the stream rule and the caches wait for.
int query_done(TorContext* ctx, hipStream_t stream) {
  tor::HitQueryState& hq = ctx->hitq;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(hq.ev_done, stream));
  hq.launched = true;
  hq.stream = (void*)stream;
  return TOR_OK;
}

// query_done and tor_last_note's "<what>[ (masked)]: blocks | brute force[ (<why>)]" (blocks, why: query_setup's)
int query_finish(TorContext* ctx, hipStream_t stream, const char* what, bool masked, bool blocks, const std::string& why) {
  const int rc = query_done(ctx, stream);
  if (rc != TOR_OK) return rc;
  const std::string w = std::string(what) + (masked ? " (masked): " : ": ");
  tor::set_last_note(blocks ? w + "blocks" : w + "brute force" + (why.empty() ? std::string() : " (" + why + ")"));
  return TOR_OK;
}

// A blocking entry waits for the context's last render launch and last query, on whatever stream they run, where the asynchronous
// entry would refuse a different stream (the staging buffer may be reallocated too).
int host_wait(TorContext* ctx) {
  if (ctx->launches > 0) HIP_TRY(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
  if (ctx->hitq.launched) HIP_TRY(hipEventSynchronize(ctx->hitq.ev_done));
  return TOR_OK;
}

// One host array of a blocking entry, staged in hitq.io: `bytes` may be 0 (an absent optional array: dev stays null); `in` copies it
// to the device before the launch (an output is staged in where unlisted rays must keep the caller's values), `out` back after it.
struct HostPart {
  const void* host;
  size_t bytes;
  bool in, out;
  char* dev;
  template <typename T>
  T* as() const { return (T*)dev; }
};

// host_wait, then the parts laid out in hitq.io in order, each padded to 64 bytes, and the `in` parts copied (blocking)
int stage_in(TorContext* ctx, HostPart* parts, int n_parts) {
  const int rc = host_wait(ctx);
  if (rc != TOR_OK) return rc;
  size_t total = 0;
  for (int k = 0; k < n_parts; ++k) total += (parts[k].bytes + 63) / 64 * 64;
  HIP_TRY(ctx->hitq.io.ensure(total));
  char* at = (char*)ctx->hitq.io.ptr;
  for (int k = 0; k < n_parts; ++k) {
    HostPart& h = parts[k];
    h.dev = h.bytes ? at : nullptr;
    if (h.bytes && h.in) HIP_TRY(hipMemcpy(h.dev, h.host, h.bytes, hipMemcpyHostToDevice));
    at += (h.bytes + 63) / 64 * 64;
  }
  return TOR_OK;
}

// the `out` parts back to the host (blocking: it waits for the launch on the default stream)
int stage_out(const HostPart* parts, int n_parts) {
  for (int k = 0; k < n_parts; ++k)
    if (parts[k].bytes && parts[k].out) HIP_TRY(hipMemcpy((void*)parts[k].host, parts[k].dev, parts[k].bytes, hipMemcpyDeviceToHost));
  return TOR_OK;
}

}  // namespace
}  // namespace tor
