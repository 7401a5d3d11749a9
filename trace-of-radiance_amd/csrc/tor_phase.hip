// tor_phase.hip -- phase-function queries for host integrators (tor_scene_media_phase, tor_phase_eval_device,
// tor_phase_sample_device and the blocking _host twins, include/tor_phase.h): the Henyey-Greenstein mixture of the media that are
// active at a collision -- a direction drawn from it, and value and density of a direction that was not drawn --, on gfx950.
// include/tor_phase.h holds the definition, operation by operation; this file follows it line by line (hg, the three walks of the
// sampler, the one walk of the evaluation).
//
// The asymmetry g_m is word [15] of the media record (the head of tor_media.hip); tor_scene_media_phase patches that word of every
// record with one strided copy.  Medium m is read at a wave-uniform address through the scalar-load view, as tor_media.hip reads
// it; the lane's `active` bit is the predicate.
//
//   phase_sample_kernel   one listed ray per lane: three generator outputs; then the wave's union of the lanes' active words
//                         (ballots, so the union lives in scalar registers) and up to three walks over its set bits, ascending:
//                         rho, the selection, the mixture.  A medium outside the union is active for no lane of the wave: skipping
//                         it changes no lane's sums.  Every walk is bounded by n_media <= 64.
//   phase_eval_kernel     one listed item per lane: the union, then one walk (the mixture).
// No LDS, no atomics, no lane waits for another; a wrong compare shows as a wrong answer, never as a hang.
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

#include "../../include/tor_phase.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"

static_assert(sizeof(TorRay) == 56 && sizeof(TorRng) == 32, "TorRay / TorRng as the kernels index them");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");
static_assert(TOR_MEDIA_MAX == 64, "the active set is one 64-bit word");

namespace tor {
namespace {

constexpr int kPhaseThreads = 256;
constexpr int kMediaWords = 16;  // float64 per medium record (tor_media.hip packs it)
constexpr int kSigmaWord = 10, kAlbedoWord = 11, kPhaseWord = 15;
static_assert(kPhaseWord == kMediaWords - 1 && kAlbedoWord + 3 <= kPhaseWord - 1, "g is the record's last word, after albedo and the index");
constexpr double kPi = 3.141592653589793;
constexpr double kFourPi = 4.0 * kPi;
constexpr double kTwoPi = 2.0 * kPi;

struct PhParams {
  const double* media;          // n_media records of kMediaWords float64
  int n_media;
  const double* rays;           // 7 float64 per ray (TorRay): the sampler's rays, the evaluation's d_in
  const double* rays_to;        // the evaluation's d_out
  const double* t_in;           // the sampler: the collision's parameter per ray
  const unsigned long long* active_in;
  unsigned long long* rng;      // the sampler: 4 u64 per ray (TorRng), read and written
  const int* list;
  long long n_list, n_rays;
  double* rays_out;             // the sampler's outputs: 7 float64 per ray
  double* att;                  // ... and 3
  double* value;                // the evaluation's outputs: 3 float64 per item
  double* pdf;                  // one per item (the sampler: or null)
};

// tor_phase.h hg(g, mu)
__device__ __forceinline__ double hg(double g, double mu) {
  const double g2 = g * g;
  const double den = (1.0 + g2) - (2.0 * g) * mu;
  return (1.0 - g2) / (kFourPi * (den * __builtin_sqrt(den)));
}

__device__ __forceinline__ double clamp1(double x) { return x > 1.0 ? 1.0 : (x < -1.0 ? -1.0 : x); }

// the union of the wave's lanes' words over media 0 .. n - 1, in scalar registers
__device__ __forceinline__ unsigned long long wave_union(unsigned long long mine, int n) {
  unsigned long long uni = 0ull;
  for (int m = 0; m < n; ++m)
    if (__ballot((mine >> m) & 1ull) != 0ull) uni |= 1ull << m;
  return ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(uni >> 32)) << 32) |
         (unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)uni);
}

struct PhMix {
  double rho, q, nx, ny, nz;
};

// tor_phase.h mixture(active, mu), over the set bits of the wave's union, ascending; `mine` is the lane's own word
__device__ __forceinline__ PhMix mixture(qcdptr M, unsigned long long uni, unsigned long long mine, double mu) {
  PhMix x{0.0, 0.0, 0.0, 0.0, 0.0};
  for (unsigned long long u = uni; u != 0ull; u &= u - 1ull) {
    const int m = __builtin_ctzll(u);
    const qcdptr r = M + kMediaWords * (size_t)m;
    const double sg = r[kSigmaWord];
    const double p = hg(r[kPhaseWord], mu);
    if ((mine >> m) & 1ull) {
      x.rho = x.rho + sg;
      x.q = x.q + sg * p;
      x.nx = x.nx + (sg * r[kAlbedoWord]) * p;
      x.ny = x.ny + (sg * r[kAlbedoWord + 1]) * p;
      x.nz = x.nz + (sg * r[kAlbedoWord + 2]) * p;
    }
  }
  return x;
}

__global__ __launch_bounds__(kPhaseThreads) void phase_sample_kernel(const PhParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_rays, (long long)blockIdx.x * kPhaseThreads + threadIdx.x);
  const bool live = i >= 0;
  Rng g{0, 0, 0, 0};
  double ray[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double t = 0.0;
  unsigned long long active = 0ull;
  if (live) {
    const unsigned long long* s = P.rng + 4 * i;
    g = Rng{s[0], s[1], s[2], s[3]};
    const double* r = P.rays + 7 * i;
#pragma unroll
    for (int k = 0; k < 7; ++k) ray[k] = r[k];
    t = P.t_in[i];
    active = P.active_in[i];
  }
  // exactly three outputs of the generator, whatever follows
  const double u_sel = uniform01(g), u_cos = uniform01(g), u_phi = uniform01(g);
  const qcdptr M = (qcdptr)(uintptr_t)P.media;
  const int n = P.n_media;
  const bool beyond = n < 64 && (active >> n) != 0ull;  // a bit at or above n_media
  const unsigned long long mine = beyond ? 0ull : active;
  const unsigned long long uni = wave_union(mine, n);
  const double ii = ray[3] * ray[3] + ray[4] * ray[4] + ray[5] * ray[5];
  // walk 1: rho
  double rho = 0.0;
  for (unsigned long long u = uni; u != 0ull; u &= u - 1ull) {
    const int m = __builtin_ctzll(u);
    const double sg = M[kMediaWords * (size_t)m + kSigmaWord];
    if ((mine >> m) & 1ull) rho = rho + sg;
  }
  // walk 2: the selection; the chosen medium's g travels with its index
  const double x = u_sel * rho;
  double acc = 0.0, g_chosen = 0.0, g_last = 0.0;
  int chosen = -1, last = -1;
  for (unsigned long long u = uni; u != 0ull; u &= u - 1ull) {
    const int m = __builtin_ctzll(u);
    const qcdptr r = M + kMediaWords * (size_t)m;
    const double sg = r[kSigmaWord], gm = r[kPhaseWord];
    if ((mine >> m) & 1ull) {
      acc = acc + sg;
      if (sg > 0.0) { last = m; g_last = gm; }
      if (chosen < 0 && x < acc) { chosen = m; g_chosen = gm; }
    }
  }
  if (chosen < 0) { chosen = last; g_chosen = g_last; }
  // the cosine
  double mu;
  if (g_chosen == 0.0) {
    mu = 1.0 - 2.0 * u_cos;
  } else {
    const double gg = g_chosen * g_chosen;
    const double s = (1.0 - gg) / ((1.0 - g_chosen) + (2.0 * g_chosen) * u_cos);
    mu = ((1.0 + gg) - s * s) / (2.0 * g_chosen);
  }
  mu = clamp1(mu);
  double r2 = 1.0 - mu * mu;
  if (!(r2 > 0.0)) r2 = 0.0;
  const double st = __builtin_sqrt(r2);
  // the azimuth
  double sp, cp;
  sincos_2pi(u_phi * kTwoPi, sp, cp);
  // the frame around the incoming direction
  const double inv = 1.0 / __builtin_sqrt(ii);
  const double wx = ray[3] * inv, wy = ray[4] * inv, wz = ray[5] * inv;
  const double sgn = __builtin_copysign(1.0, wz);
  const double a = -1.0 / (sgn + wz);
  const double b = (wx * wy) * a;
  const double b1x = 1.0 + ((sgn * wx) * wx) * a, b1y = sgn * b, b1z = -(sgn * wx);
  const double b2x = b, b2y = sgn + (wy * wy) * a, b2z = -wy;
  const double ec = st * cp, es = st * sp;
  const double vx = (ec * b1x + es * b2x) + mu * wx;
  const double vy = (ec * b1y + es * b2y) + mu * wy;
  const double vz = (ec * b1z + es * b2z) + mu * wz;
  // walk 3: the mixture at the cosine that was drawn
  const PhMix mix = mixture(M, uni, mine, mu);
  if (!live) return;
  unsigned long long* s = P.rng + 4 * i;
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
  double* o = P.rays_out + 7 * i;
  double* at = P.att + 3 * i;
  const bool bad_ii = !(ii > 0.0) || ii == __builtin_inf();
  if (active == 0ull || beyond || !(rho > 0.0) || bad_ii || !(mix.q > 0.0)) {
    for (int k = 0; k < 7; ++k) o[k] = 0.0;
    at[0] = 0.0; at[1] = 0.0; at[2] = 0.0;
    if (P.pdf) P.pdf[i] = 0.0;
    return;
  }
  o[0] = ray[0] + t * ray[3]; o[1] = ray[1] + t * ray[4]; o[2] = ray[2] + t * ray[5];
  o[3] = vx; o[4] = vy; o[5] = vz;
  o[6] = ray[6];
  at[0] = mix.nx / mix.q; at[1] = mix.ny / mix.q; at[2] = mix.nz / mix.q;
  if (P.pdf) P.pdf[i] = mix.q / rho;
}

__global__ __launch_bounds__(kPhaseThreads) void phase_eval_kernel(const PhParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_rays, (long long)blockIdx.x * kPhaseThreads + threadIdx.x);
  const bool live = i >= 0;
  double ix = 0.0, iy = 0.0, iz = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;
  unsigned long long active = 0ull;
  if (live) {
    const double* a = P.rays + 7 * i;
    const double* b = P.rays_to + 7 * i;
    ix = a[3]; iy = a[4]; iz = a[5];
    ox = b[3]; oy = b[4]; oz = b[5];
    active = P.active_in[i];
  }
  const qcdptr M = (qcdptr)(uintptr_t)P.media;
  const int n = P.n_media;
  const bool beyond = n < 64 && (active >> n) != 0ull;
  const unsigned long long mine = beyond ? 0ull : active;
  const unsigned long long uni = wave_union(mine, n);
  const double ii = ix * ix + iy * iy + iz * iz;
  const double oo = ox * ox + oy * oy + oz * oz;
  const double inv_i = 1.0 / __builtin_sqrt(ii), inv_o = 1.0 / __builtin_sqrt(oo);
  const double wx = ix * inv_i, wy = iy * inv_i, wz = iz * inv_i;
  const double vx = ox * inv_o, vy = oy * inv_o, vz = oz * inv_o;
  const double mu = clamp1(wx * vx + wy * vy + wz * vz);
  const PhMix mix = mixture(M, uni, mine, mu);
  if (!live) return;
  double* val = P.value + 3 * i;
  const bool bad = !(ii > 0.0) || ii == __builtin_inf() || !(oo > 0.0) || oo == __builtin_inf();
  if (bad || active == 0ull || beyond || !(mix.rho > 0.0)) {
    val[0] = 0.0; val[1] = 0.0; val[2] = 0.0;
    P.pdf[i] = 0.0;
    return;
  }
  val[0] = mix.nx / mix.rho; val[1] = mix.ny / mix.rho; val[2] = mix.nz / mix.rho;
  P.pdf[i] = mix.q / mix.rho;
}

}  // namespace
}  // namespace tor

namespace {

// media_check's order (tor_media.hip): the list arguments, the NULL arrays, the scene, its media table
int phase_check(const char* who, TorContext* ctx, int64_t n_rays, const void* list, int64_t n_list, bool nulls, const char* names) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_rays, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL " + names);
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  if (ctx->hitq.n_media <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no media table (tor_scene_media)");
  return TOR_OK;
}

// the launches; the arguments are checked, n_rays > 0 and n_list > 0
int phase_launch(const char* who, TorContext* ctx, bool sample, tor::PhParams& P, int64_t n_rays, const int32_t* d_list, int64_t n_list,
                 hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  P.media = (const double*)ctx->hitq.media.ptr;
  P.n_media = (int)ctx->hitq.n_media;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_rays = (long long)n_rays;
  const dim3 grid((unsigned)((n_list + tor::kPhaseThreads - 1) / tor::kPhaseThreads)), block(tor::kPhaseThreads);
  if (sample) hipLaunchKernelGGL(tor::phase_sample_kernel, grid, block, 0, stream, P);
  else hipLaunchKernelGGL(tor::phase_eval_kernel, grid, block, 0, stream, P);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note(std::string(sample ? "phase sample: " : "phase eval: ") + std::to_string(ctx->hitq.n_media) + " media");
  return TOR_OK;
}

int eval_launch(const char* who, TorContext* ctx, int64_t n, const void* d_in, const uint64_t* d_active, const void* d_out,
                const int32_t* d_list, int64_t n_list, double* d_value, double* d_pdf, hipStream_t stream) {
  tor::PhParams P{};
  P.rays = (const double*)d_in;
  P.rays_to = (const double*)d_out;
  P.active_in = (const unsigned long long*)d_active;
  P.value = d_value;
  P.pdf = d_pdf;
  return phase_launch(who, ctx, false, P, n, d_list, n_list, stream);
}

int sample_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t, const uint64_t* d_active,
                  void* d_rng, const int32_t* d_list, int64_t n_list, void* d_rays_out, double* d_att, double* d_pdf, hipStream_t stream) {
  tor::PhParams P{};
  P.rays = (const double*)d_rays;
  P.t_in = d_t;
  P.active_in = (const unsigned long long*)d_active;
  P.rng = (unsigned long long*)d_rng;
  P.rays_out = (double*)d_rays_out;
  P.att = d_att;
  P.pdf = d_pdf;
  return phase_launch(who, ctx, true, P, n_rays, d_list, n_list, stream);
}

}  // namespace

extern "C" {

int tor_scene_media_phase(TorContext* ctx, int64_t n_media, const double* g) {
  using tor::fail;
  const std::string w = "tor_scene_media_phase";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  tor::HitQueryState& hq = ctx->hitq;
  if (hq.n_media <= 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no media table (tor_scene_media)");
  if (n_media != hq.n_media)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_media must be the table's count (" + std::to_string(hq.n_media) + ")");
  for (int64_t j = 0; g && j < n_media; ++j)
    if (!std::isfinite(g[j])) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": g must be finite");
  for (int64_t j = 0; g && j < n_media; ++j)
    if (std::fabs(g[j]) > TOR_PHASE_G_MAX) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": |g| above TOR_PHASE_G_MAX (0.99)");
  for (int64_t j = 0; g && j < n_media; ++j)
    if (g[j] != 0.0 && std::fabs(g[j]) < TOR_PHASE_G_MIN)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": 0 < |g| below TOR_PHASE_G_MIN (2^-20): use 0 for an isotropic medium");
  const std::vector<double> zeros(g ? 0 : (size_t)n_media, 0.0);
  const double* src = g ? g : zeros.data();
  HIP_TRY(hipSetDevice(ctx->device));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the table
  // word [15] of every record: one strided copy
  HIP_TRY(hipMemcpy2D((char*)hq.media.ptr + 8 * tor::kPhaseWord, 8 * tor::kMediaWords, src, 8, 8, (size_t)n_media, hipMemcpyHostToDevice));
  return TOR_OK;
}

int tor_phase_eval_device(TorContext* ctx, int64_t n, const TorRay* d_in, const uint64_t* d_active, const TorRay* d_out, const int32_t* d_list,
                          int64_t n_list, double* d_value, double* d_pdf, void* hip_stream) {
  const char* who = "tor_phase_eval_device";
  const int rc = phase_check(who, ctx, n, d_list, n_list, !d_in || !d_active || !d_out || !d_value || !d_pdf, "in, active, out, value or pdf");
  if (rc != TOR_OK || n == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return eval_launch(who, ctx, n, d_in, d_active, d_out, d_list, n_list, d_value, d_pdf, (hipStream_t)hip_stream);
}

int tor_phase_eval_host(TorContext* ctx, int64_t n, const TorRay* in, const uint64_t* active, const TorRay* out, const int32_t* list,
                        int64_t n_list, double* value, double* pdf) {
  const char* who = "tor_phase_eval_host";
  int rc = phase_check(who, ctx, n, list, n_list, !in || !active || !out || !value || !pdf, "in, active, out, value or pdf");
  if (rc != TOR_OK || n == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t k = (size_t)n;
  tor::HostPart st[6] = {{in, k * sizeof(TorRay), true, false},
                         {active, k * 8, true, false},
                         {out, k * sizeof(TorRay), true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {value, k * 24, true, true},
                         {pdf, k * 8, true, true}};
  rc = tor::stage_in(ctx, st, 6);
  if (rc != TOR_OK) return rc;
  rc = eval_launch(who, ctx, n, st[0].dev, st[1].as<const uint64_t>(), st[2].dev, st[3].as<const int32_t>(), n_list, st[4].as<double>(),
                   st[5].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 6);
}

int tor_phase_sample_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t, const uint64_t* d_active, TorRng* d_rng,
                            const int32_t* d_list, int64_t n_list, TorRay* d_rays_out, double* d_att, double* d_pdf, void* hip_stream) {
  const char* who = "tor_phase_sample_device";
  const int rc = phase_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_t || !d_active || !d_rng || !d_rays_out || !d_att,
                             "rays, t, active, rng, rays_out or att");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return sample_launch(who, ctx, n_rays, d_rays, d_t, d_active, d_rng, d_list, n_list, d_rays_out, d_att, d_pdf, (hipStream_t)hip_stream);
}

int tor_phase_sample_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t, const uint64_t* active, TorRng* rng,
                          const int32_t* list, int64_t n_list, TorRay* rays_out, double* att, double* pdf) {
  const char* who = "tor_phase_sample_host";
  int rc = phase_check(who, ctx, n_rays, list, n_list, !rays || !t || !active || !rng || !rays_out || !att,
                       "rays, t, active, rng, rays_out or att");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_rays;
  const bool alias = (const void*)rays_out == (const void*)rays;  // one staged copy then: read, and written back
  tor::HostPart st[8] = {{rays, n * sizeof(TorRay), true, alias},
                         {t, n * 8, true, false},
                         {active, n * 8, true, false},
                         {rng, n * sizeof(TorRng), true, true},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {rays_out, alias ? 0 : n * sizeof(TorRay), true, true},
                         {att, n * 24, true, true},
                         {pdf, pdf ? n * 8 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 8);
  if (rc != TOR_OK) return rc;
  rc = sample_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const uint64_t>(), st[3].dev,
                     st[4].as<const int32_t>(), n_list, alias ? st[0].dev : st[5].dev, st[6].as<double>(), st[7].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 8);
}

}  // extern "C"
