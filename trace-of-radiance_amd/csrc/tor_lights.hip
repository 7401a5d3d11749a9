// tor_lights.hip -- direct-light sampling queries for host integrators (tor_scene_lights, tor_light_sample_device /
// tor_light_pdf_device and the blocking _host twins, include/tor_lights.h): for each listed shading point (p, time) one light of
// the context's light table, a direction inside the cone that light's sphere subtends, the solid-angle density of that direction
// and the shadow segment towards the sampled surface point, on gfx950 -- the step of next-event estimation that produces the
// shadow rays tor_occluded_device answers.  include/tor_lights.h holds the definition, operation by operation; this file
// follows it line by line (light_geom, importance_of, the walk, cone_sample).
//
// The light table (tor_scene_lights) is one device record of 16 float64 per light, packed when the table is set:
//     [0..2] center / center0   [3..5] center1 - center0   [6] time0   [7] time1 - time0   [8] 1.0 for a MovingSphere, else 0.0
//     [9] R = abs(radius)   [10] R * R   [11] weight   [12] the running sum of the weights up to and including this light
//     [13] the object's index in the uploaded list (int64 bits)   [14..15] unused
// -- the centre data are the scene's cold record's (tor_kernels.hpp), so the centre is centre_at's (tor_query.hpp) operation
// for operation.  Light j is read at a wave-uniform address through the scalar-load view, so the loops over the lights are
// uniform: a lane without a point runs them with importance 0 and touches no memory.
//
//   light_sample_kernel<false>  TOR_LIGHT_BY_WEIGHT: the importances are the weights -- the same for every point --, so the total
//                               and the running sums are the table's (summed once, sequentially, when it was set) and the walk
//                               compares only; the geometry of the ONE picked light is then computed per lane
//   light_sample_kernel<true>   TOR_LIGHT_BY_SOLID_ANGLE: n_points x n_lights, a `/` and a sqrt per pair, in two passes -- the
//                               total, then the walk to the pick.  Pass 2 computes every importance again instead of storing
//                               it, through the same function: the same instructions in the same order, so its running sums
//                               are pass 1's bits.  The walk keeps the geometry of its candidate in registers (selects), so no
//                               lane ever loads a record at an address of its own
//   light_pdf_kernel<SOLID>     the density the sampler gives the direction towards a given object: the same per-light
//                               arithmetic and the same sequential total, nothing drawn
//
// Float64, unfused (-ffp-contract=off), correctly rounded `/` and sqrt.  Stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tor_lights.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"

static_assert(sizeof(TorPoint) == 32 && sizeof(TorRay) == 56 && sizeof(TorRng) == 32, "TorPoint / TorRay / TorRng as the kernels index them");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");

namespace tor {
namespace {

constexpr int kLightThreads = 256;
constexpr int kLightWords = 16;  // float64 per light record
constexpr double kTwoPi = 2.0 * 3.141592653589793;  // sampling.nim:52: Nim's 2 * PI

struct LParams {
  const double* lights;      // n_lights records of kLightWords float64
  int n_lights;
  const double* points;      // 4 float64 per point (TorPoint)
  unsigned long long* rng;   // 4 u64 per point (TorRng), read and written (the sampler alone)
  const int* object;         // the density query alone: one object index per point
  const int* list;           // the points to answer, or null: entry e is point e
  long long n_list, n_points;
  double* rays;              // 7 float64 per point (TorRay)
  double* pdf;               // one float64 per point
  int* light;                // one int32 per point: the picked light's OBJECT index, -1 for none
  double* dist;              // one float64 per point, or null
};

// what the sampler needs of one (point, light) pair
struct LGeom {
  double wx, wy, wz;  // centre - p
  double d2, R2, m;   // |w|^2, R * R, 1 - cos(theta_max)
  bool inside;
};

// tor_lights.h "per light": the centre at the point's time (centre_at's operations, moving_spheres.nim:39-44), w, d2, inside, m
template <typename P>
__device__ __forceinline__ LGeom light_geom(P r, double px, double py, double pz, double time) {
  double cx = r[0], cy = r[1], cz = r[2];
  if (r[8] != 0.0) {
    const double f = (time - r[6]) / r[7];
    cx = cx + r[3] * f; cy = cy + r[4] * f; cz = cz + r[5] * f;
  }
  LGeom g;
  g.wx = cx - px; g.wy = cy - py; g.wz = cz - pz;
  g.d2 = g.wx * g.wx + g.wy * g.wy + g.wz * g.wz;
  g.R2 = r[10];
  g.inside = !(g.d2 > g.R2);
  const double s2 = g.R2 / g.d2;
  g.m = g.inside ? 2.0 : s2 / (1.0 + __builtin_sqrt(1.0 - s2));
  return g;
}

template <typename P>
__device__ __forceinline__ int light_object(P r) {
  return (int)__double_as_longlong(r[13]);
}

struct LPoint {
  double x, y, z, time;
};

// the point of this lane's list entry, or -1 (listed_ray, tor_query.hpp)
__device__ __forceinline__ long long light_point(const LParams& P, LPoint& q) {
  const long long i = listed_ray(P.list, P.n_list, P.n_points, (long long)blockIdx.x * kLightThreads + threadIdx.x);
  q = LPoint{0.0, 0.0, 0.0, 0.0};
  if (i >= 0) {
    const double* s = P.points + 4 * i;
    q.x = s[0]; q.y = s[1]; q.z = s[2]; q.time = s[3];
  }
  return i;
}

// T > 0 and finite
__device__ __forceinline__ bool usable_total(double T) { return (T > 0.0) && (T < __builtin_inf()); }

template <bool SOLID>
__global__ __launch_bounds__(kLightThreads) void light_sample_kernel(const LParams P) {
  LPoint q;
  const long long i = light_point(P, q);
  const bool live = i >= 0;
  Rng g{0, 0, 0, 0};
  if (live) {
    const unsigned long long* s = P.rng + 4 * i;
    g = Rng{s[0], s[1], s[2], s[3]};
  }
  // exactly three draws, whatever follows
  const double u0 = uniform01(g), u1 = uniform01(g), u2 = uniform01(g);
  const qcdptr L = (qcdptr)(uintptr_t)P.lights;
  const int n = P.n_lights;
  // pass 1: the total
  double T = 0.0;
  if constexpr (SOLID) {
    for (int j = 0; j < n; ++j) {
      const qcdptr r = L + kLightWords * (size_t)j;
      const LGeom gj = light_geom(r, q.x, q.y, q.z, q.time);
      const double I = live ? r[11] * gj.m : 0.0;
      T = T + I;
    }
  } else {
    T = L[kLightWords * (size_t)(n - 1) + 12];
  }
  const bool usable = live && usable_total(T);
  const double x = u0 * T;
  // pass 2, the walk: the candidate is the last light with I > 0 seen so far, frozen at the first whose running sum is above x
  int cand = -1, object = -1;
  bool done = false;
  LGeom pg{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, false};
  double pI = 0.0;
  if constexpr (SOLID) {
    double run = 0.0;
    for (int j = 0; j < n; ++j) {
      const qcdptr r = L + kLightWords * (size_t)j;
      const LGeom gj = light_geom(r, q.x, q.y, q.z, q.time);
      const double I = live ? r[11] * gj.m : 0.0;
      run = run + I;
      if (usable && !done && (I > 0.0)) {
        cand = j;
        object = light_object(r);
        pg = gj;
        pI = I;
        done = run > x;
      }
    }
  } else {
    for (int j = 0; j < n; ++j) {
      const qcdptr r = L + kLightWords * (size_t)j;
      const double I = r[11];
      if (usable && !done && (I > 0.0)) {
        cand = j;
        done = r[12] > x;
      }
    }
    if (cand >= 0) {  // (cand < n_lights: the loop's index)
      const qgdptr r = (qgdptr)(uintptr_t)(P.lights + kLightWords * (size_t)cand);
      pg = light_geom(r, q.x, q.y, q.z, q.time);
      pI = r[11];
      object = light_object(r);
    }
  }
  if (!live) return;
  unsigned long long* s = P.rng + 4 * i;
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
  double* o = P.rays + 7 * i;
  if (cand < 0) {  // no usable total (or, with one, no light of positive importance: cannot happen)
    for (int k = 0; k < 7; ++k) o[k] = 0.0;
    P.pdf[i] = 0.0;
    P.light[i] = -1;
    if (P.dist) P.dist[i] = 0.0;
    return;
  }
  // the cone sample of the picked light
  const double Pj = pI / T;
  const double k = u1 * pg.m;
  const double cos_t = 1.0 - k;
  const double sin2 = k * (2.0 - k);
  const double sin_t = __builtin_sqrt(sin2);
  double sn, cs;
  sincos_2pi(u2 * kTwoPi, sn, cs);
  const double sd = __builtin_sqrt(pg.d2);
  const double inv = 1.0 / sd;
  double ax = pg.wx * inv, ay = pg.wy * inv, az = pg.wz * inv;
  if (pg.d2 == 0.0) { ax = 0.0; ay = 0.0; az = 1.0; }
  // the branchless orthonormal frame around a
  const double sg = __builtin_copysign(1.0, az);
  const double aa = -1.0 / (sg + az);
  const double bb = ax * ay * aa;
  const double b1x = 1.0 + sg * ax * ax * aa, b1y = sg * bb, b1z = -sg * ax;
  const double b2x = bb, b2y = sg + ay * ay * aa, b2z = -ay;
  const double e1 = sin_t * cs, e2 = sin_t * sn;
  const double dx = b1x * e1 + b2x * e2 + ax * cos_t;
  const double dy = b1y * e1 + b2y * e2 + ay * cos_t;
  const double dz = b1z * e1 + b2z * e2 + az * cos_t;
  double h = pg.R2 - pg.d2 * sin2;
  if (!(h > 0.0)) h = 0.0;
  const double rh = __builtin_sqrt(h);
  const double t = pg.inside ? sd * cos_t + rh : sd * cos_t - rh;
  o[0] = q.x; o[1] = q.y; o[2] = q.z;
  o[3] = dx * t; o[4] = dy * t; o[5] = dz * t;
  o[6] = q.time;
  P.pdf[i] = Pj / (kTwoPi * pg.m);
  P.light[i] = object;
  if (P.dist) P.dist[i] = t;
}

template <bool SOLID>
__global__ __launch_bounds__(kLightThreads) void light_pdf_kernel(const LParams P) {
  LPoint q;
  const long long i = light_point(P, q);
  const bool live = i >= 0;
  const int want = live ? P.object[i] : -1;
  const qcdptr L = (qcdptr)(uintptr_t)P.lights;
  const int n = P.n_lights;
  double T = 0.0, pI = 0.0, pm = 0.0;
  bool found = false;
  if constexpr (SOLID) {
    for (int j = 0; j < n; ++j) {
      const qcdptr r = L + kLightWords * (size_t)j;
      const LGeom gj = light_geom(r, q.x, q.y, q.z, q.time);
      const double I = live ? r[11] * gj.m : 0.0;
      T = T + I;
      if (live && light_object(r) == want) {
        found = true;
        pI = I;
        pm = gj.m;
      }
    }
  } else {
    T = L[kLightWords * (size_t)(n - 1) + 12];
    int at = -1;
    for (int j = 0; j < n; ++j)
      if (live && light_object(L + kLightWords * (size_t)j) == want) at = j;
    if (at >= 0) {  // (at < n_lights: the loop's index)
      const qgdptr r = (qgdptr)(uintptr_t)(P.lights + kLightWords * (size_t)at);
      found = true;
      pI = r[11];
      pm = light_geom(r, q.x, q.y, q.z, q.time).m;
    }
  }
  if (!live) return;
  P.pdf[i] = (found && usable_total(T) && (pI > 0.0)) ? (pI / T) / (kTwoPi * pm) : 0.0;
}

}  // namespace
}  // namespace tor

namespace {

const char* strategy_note(int32_t strategy) { return strategy == TOR_LIGHT_BY_WEIGHT ? "by weight" : "by solid angle"; }

// the checks that need no device and do not read *ctx: tor_bounce_device's, then the strategy and the NULL arrays; then the scene
// and its light table
int light_check(const char* who, TorContext* ctx, int64_t n_points, const void* list, int64_t n_list, int32_t strategy, bool nulls) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_points, list, n_list);
  if (rc != TOR_OK) return rc;
  if (strategy != TOR_LIGHT_BY_WEIGHT && strategy != TOR_LIGHT_BY_SOLID_ANGLE)
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": strategy must be TOR_LIGHT_BY_WEIGHT (0) or TOR_LIGHT_BY_SOLID_ANGLE (1)");
  if (n_points > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL points, rng, object, rays, pdf or light");
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  if (ctx->hitq.n_lights <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no light table (tor_scene_lights)");
  return TOR_OK;
}

unsigned light_grid(int64_t n_list) { return (unsigned)((n_list + tor::kLightThreads - 1) / tor::kLightThreads); }

// the launches; the arguments are checked, n_points > 0 and n_list > 0
int light_launch(const char* who, TorContext* ctx, bool pdf_only, int64_t n_points, const void* d_points, void* d_rng, const int32_t* d_object,
                 const int32_t* d_list, int64_t n_list, int32_t strategy, void* d_rays, double* d_pdf, int32_t* d_light, double* d_dist,
                 hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the queries read the light table alone)
  if (rc != TOR_OK) return rc;
  tor::LParams P{};
  P.lights = (const double*)ctx->hitq.lights.ptr;
  P.n_lights = (int)ctx->hitq.n_lights;
  P.points = (const double*)d_points;
  P.rng = (unsigned long long*)d_rng;
  P.object = d_object;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_points = (long long)n_points;
  P.rays = (double*)d_rays;
  P.pdf = d_pdf;
  P.light = d_light;
  P.dist = d_dist;
  const bool solid = strategy == TOR_LIGHT_BY_SOLID_ANGLE;
  const dim3 grid(light_grid(n_list)), block(tor::kLightThreads);
  if (pdf_only) {
    if (solid) hipLaunchKernelGGL(tor::light_pdf_kernel<true>, grid, block, 0, stream, P);
    else hipLaunchKernelGGL(tor::light_pdf_kernel<false>, grid, block, 0, stream, P);
  } else {
    if (solid) hipLaunchKernelGGL(tor::light_sample_kernel<true>, grid, block, 0, stream, P);
    else hipLaunchKernelGGL(tor::light_sample_kernel<false>, grid, block, 0, stream, P);
  }
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note(std::string(pdf_only ? "light pdf: " : "light sample: ") + strategy_note(strategy));
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_scene_lights(TorContext* ctx, int64_t n_lights, const int32_t* objects, const double* weights) {
  using tor::fail;
  const std::string w = "tor_scene_lights";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  const int64_t n = ctx->n_objects;
  if (n_lights < 0 || n_lights > n) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_lights <= the uploaded list's length (" + std::to_string(n) + ")");
  if (n_lights > 0 && !objects) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": objects is NULL");
  std::vector<char> seen((size_t)n, 0);
  bool any = false;
  for (int64_t j = 0; j < n_lights; ++j) {
    const int64_t o = objects[j];
    if (o < 0 || o >= n) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": objects[" + std::to_string(j) + "] is outside the uploaded list");
    if (seen[(size_t)o]) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": object " + std::to_string(o) + " is listed twice");
    seen[(size_t)o] = 1;
    const double wt = weights ? weights[j] : 1.0;
    if (!std::isfinite(wt) || wt < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": weights must be finite and >= 0");
    any = any || wt > 0.0;
  }
  if (n_lights > 0 && !any) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": at least one weight must be > 0");
  // the records, from the scene's cold records (by original index) and the list's radii
  std::vector<double> recs((size_t)n_lights * tor::kLightWords, 0.0);
  double run = 0.0;
  int64_t last_pos = 0;
  if (n_lights > 0) {
    tor::HostLayout lay;
    std::string err;
    if (!tor::flat_host_layout(ctx, lay, err)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": " + err);
    std::vector<int64_t> slot_of((size_t)n, -1);
    for (size_t s = 0; s < lay.n_sorted; ++s) {
      const double* c = &lay.cold[16 * s];
      if (c[15] == -1.0) continue;  // padding slot
      int64_t orig;
      std::memcpy(&orig, &c[14], 8);
      if (orig >= 0 && orig < n) slot_of[(size_t)orig] = (int64_t)s;
    }
    const TorHittableVariant* objs = (const TorHittableVariant*)ctx->scene_bytes.data();
    for (int64_t j = 0; j < n_lights; ++j) {
      const int64_t o = objects[j];
      if (slot_of[(size_t)o] < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the flat layout holds no record of object " + std::to_string(o));
      const double* c = &lay.cold[16 * (size_t)slot_of[(size_t)o]];
      double* r = &recs[(size_t)j * tor::kLightWords];
      int64_t flags;
      std::memcpy(&flags, &c[13], 8);
      for (int k = 0; k < 6; ++k) r[k] = c[k];
      r[6] = c[7];
      r[7] = c[8];
      r[8] = ((int)flags & 1) ? 1.0 : 0.0;
      const double R = std::fabs(objs[o].kind == TOR_SPHERE ? objs[o].u.sphere.radius : objs[o].u.moving_sphere.radius);
      r[9] = R;
      r[10] = R * R;
      const double wt = weights ? weights[j] : 1.0;
      r[11] = wt;
      run = run + wt;
      r[12] = run;
      if (wt > 0.0) last_pos = j;
      std::memcpy(&r[13], &o, 8);
    }
  }
  HIP_TRY(hipSetDevice(ctx->device));
  tor::HitQueryState& hq = ctx->hitq;
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the table
  if (n_lights > 0) {
    HIP_TRY(hq.lights.ensure(recs.size() * 8));
    HIP_TRY(hipMemcpy(hq.lights.ptr, recs.data(), recs.size() * 8, hipMemcpyHostToDevice));
  }
  hq.n_lights = n_lights;
  hq.lights_total = run;
  hq.lights_last_pos = last_pos;
  return TOR_OK;
}

int tor_light_sample_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                            int32_t strategy, TorRay* d_rays, double* d_pdf, int32_t* d_light, double* d_dist, void* hip_stream) {
  const char* who = "tor_light_sample_device";
  const int rc = light_check(who, ctx, n_points, d_list, n_list, strategy, !d_points || !d_rng || !d_rays || !d_pdf || !d_light);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return light_launch(who, ctx, false, n_points, d_points, d_rng, nullptr, d_list, n_list, strategy, d_rays, d_pdf, d_light, d_dist,
                      (hipStream_t)hip_stream);
}

int tor_light_sample_host(TorContext* ctx, int64_t n_points, const TorPoint* points, TorRng* rng, const int32_t* list, int64_t n_list,
                          int32_t strategy, TorRay* rays, double* pdf, int32_t* light, double* dist) {
  const char* who = "tor_light_sample_host";
  int rc = light_check(who, ctx, n_points, list, n_list, strategy, !points || !rng || !rays || !pdf || !light);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too, points that are not listed keep what the caller holds --, the query on the default stream,
  // the outputs back
  const size_t n = (size_t)n_points;
  tor::HostPart st[7] = {{points, n * sizeof(TorPoint), true, false},
                         {rng, n * sizeof(TorRng), true, true},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {rays, n * sizeof(TorRay), true, true},
                         {pdf, n * 8, true, true},
                         {light, n * 4, true, true},
                         {dist, dist ? n * 8 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = light_launch(who, ctx, false, n_points, st[0].dev, st[1].dev, nullptr, st[2].as<const int32_t>(), n_list, strategy, st[3].dev,
                    st[4].as<double>(), st[5].as<int32_t>(), st[6].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

int tor_light_pdf_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, const int32_t* d_object, const int32_t* d_list,
                         int64_t n_list, int32_t strategy, double* d_pdf, void* hip_stream) {
  const char* who = "tor_light_pdf_device";
  const int rc = light_check(who, ctx, n_points, d_list, n_list, strategy, !d_points || !d_object || !d_pdf);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return light_launch(who, ctx, true, n_points, d_points, nullptr, d_object, d_list, n_list, strategy, nullptr, d_pdf, nullptr, nullptr,
                      (hipStream_t)hip_stream);
}

int tor_light_pdf_host(TorContext* ctx, int64_t n_points, const TorPoint* points, const int32_t* object, const int32_t* list, int64_t n_list,
                       int32_t strategy, double* pdf) {
  const char* who = "tor_light_pdf_host";
  int rc = light_check(who, ctx, n_points, list, n_list, strategy, !points || !object || !pdf);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_points;
  tor::HostPart st[4] = {{points, n * sizeof(TorPoint), true, false},
                         {object, n * 4, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {pdf, n * 8, true, true}};
  rc = tor::stage_in(ctx, st, 4);
  if (rc != TOR_OK) return rc;
  rc = light_launch(who, ctx, true, n_points, st[0].dev, nullptr, st[1].as<const int32_t>(), st[2].as<const int32_t>(), n_list, strategy,
                    nullptr, st[3].as<double>(), nullptr, nullptr, nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 4);
}

}  // extern "C"
