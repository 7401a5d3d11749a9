// tor_env.hip -- environment-light queries for host integrators (tor_scene_environment, tor_env_sample_device /
// tor_env_eval_device and the blocking _host twins, include/tor_env.h): a context-owned octahedral environment map, for each
// listed shading point one direction drawn in proportion to the map's importance with its solid-angle density and the shadow ray
// tor_occluded_device answers, and for each listed ray the colour and the density of its direction, on gfx950.
// include/tor_env.h holds the definition, operation by operation; this file follows it line by line (env_decode, the encode at the
// head of env_eval_kernel, the two searches, env_density).
//
// The map's tables (tor_scene_environment) are one device allocation, laid out by n alone (EnvLayout), nc = ceil(n / 16):
//     tex      n * n records of 4 float64 {R, G, B, I}: everything the evaluation and the sampler's outputs need of a texel is ONE
//              32-byte load
//     cum      n * n float64: the running sums of the importances within each row
//     ccoarse  n * nc float64: per row every 16th running sum -- entry k is the LAST running sum of the columns [16 k, 16 k + 16)
//     marg     n float64: the marginal running sums M_r;   mcoarse  nc float64: every 16th of them, as ccoarse
//     lastcol  n int32: per row the last column with I > 0 (-1: none), the column search's fallback
// A search is "the first index whose running sum is > x" in a non-decreasing array (running sums of non-negatives never decrease,
// whatever the rounding), in two levels: count_le over the coarse array picks the group of 16, count_le over that group -- one
// 128-byte line -- the element.  The coarse entry of a group is its own last element, so the two-level answer IS the first index
// of the whole array, bit for bit; a plain binary search over n = 1024 would touch about ten lines per lane, this one touches the
// coarse array (at most 1 KiB per row, shared by the wave's lanes that picked the row) and one line.  count_le is a fixed-length
// branch-free lower-bound walk: bit_length(length) steps, the same for every lane, every index clamped into the array before its
// load.  Lanes without a point return before the first load.
//
// Float64, unfused (-ffp-contract=off), correctly rounded `/` and sqrt.  Stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tor_env.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"

static_assert(sizeof(TorPoint) == 32 && sizeof(TorRay) == 56 && sizeof(TorRng) == 32, "TorPoint / TorRay / TorRng as the kernels index them");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");

namespace tor {
namespace {

constexpr int kEnvThreads = 256;
constexpr int kEnvGroup = 16;  // running sums per coarse entry: 16 float64 are one 128-byte line

// where the tables sit in the context's allocation (offsets in float64), from n alone
struct EnvLayout {
  size_t n, nc, tex, cum, ccoarse, marg, mcoarse, lastcol, words;
  explicit EnvLayout(size_t n_) : n(n_), nc((n_ + kEnvGroup - 1) / kEnvGroup) {
    tex = 0;
    cum = tex + 4 * n * n;
    ccoarse = cum + n * n;
    marg = ccoarse + n * nc;
    mcoarse = marg + n;
    lastcol = mcoarse + nc;
    words = lastcol + (n + 1) / 2;
  }
};

int bit_length(int m) {
  int b = 0;
  while (m > 0) { ++b; m >>= 1; }
  return b;
}

struct EParams {
  const double *tex, *cum, *ccoarse, *marg, *mcoarse;
  const int* lastcol;
  int n, nc;
  int steps;                 // bit_length(nc): the trip count of a coarse search
  int last_row;              // the last row with S_r > 0
  double total;              // T
  const double* points;      // 4 float64 per point (TorPoint); the sampler alone
  unsigned long long* rng;   // 4 u64 per point (TorRng), read and written; the sampler alone
  const int* list;           // the points / rays to answer, or null: entry e is point e
  long long n_list, n_items;
  double* rays;              // 7 float64 per point (TorRay): the sampler's output, the evaluation's input
  double* pdf;               // one float64 per point (the evaluation: or null)
  int* texel;                // one int32 per point (the evaluation: or null)
  double* color;             // 3 float64 per point (the sampler: or null)
};

// How many elements of the non-decreasing a[0 .. m) are <= x, m >= 1: the first index whose element is > x, or m if none.  `steps`
// >= bit_length(m) halving steps, branch-free; the index of every load is clamped into [0, m).
__device__ __forceinline__ int count_le(const double* a, int m, int steps, double x) {
  int pos = 0;
  for (int s = steps - 1; s >= 0; --s) {
    const int probe = pos + (1 << s);
    const int at = (probe < m ? probe : m) - 1;
    const double v = a[at];
    pos = (probe <= m && v <= x) ? probe : pos;
  }
  return pos;
}

// the first index of the non-decreasing a[0 .. n) whose element is > x, or n if none: the group through the coarse array co[0 .. nc)
// (entry k = the last element of group k), then the element inside the group's line -- its last element is > x, so the first
// one is among the count of the others that are <= x
__device__ __forceinline__ int first_above(const double* a, const double* co, int n, int nc, int steps, double x) {
  const int k = count_le(co, nc, steps, x);
  const int kk = k < nc ? k : nc - 1;
  const int base = kEnvGroup * kk;
  const int m = (n - base < kEnvGroup ? n - base : kEnvGroup) - 1;  // the group's elements but its last: 0 .. 15
  const int j = m > 0 ? count_le(a + base, m, 4, x) : 0;
  return k < nc ? base + j : n;
}

struct EDir {
  double x, y, z, len;
};

// tor_env.h decode
__device__ __forceinline__ EDir env_decode(double s, double t) {
  const double as = __builtin_fabs(s), at = __builtin_fabs(t);
  const double py = (1.0 - as) - at;
  double px = s, pz = t;
  if (!(py >= 0.0)) {
    px = __builtin_copysign(1.0 - at, s);
    pz = __builtin_copysign(1.0 - as, t);
  }
  EDir d;
  d.len = __builtin_sqrt(px * px + py * py + pz * pz);
  const double inv = 1.0 / d.len;
  d.x = px * inv; d.y = py * inv; d.z = pz * inv;
  return d;
}

__device__ __forceinline__ int env_cell(double s, double nd, int n) {
  const double f = __builtin_floor((s + 1.0) * (0.5 * nd));
  return f > 0.0 ? (f < (double)(n - 1) ? (int)f : n - 1) : 0;
}

// tor_env.h density: P = I / T; A = (n * n) * 0.25; (P * A) * ((len * len) * len)
__device__ __forceinline__ double env_density(double I, double T, double nd, double len) {
  const double P = I / T;
  const double A = (nd * nd) * 0.25;
  return (P * A) * ((len * len) * len);
}

__global__ __launch_bounds__(kEnvThreads) void env_sample_kernel(const EParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_items, (long long)blockIdx.x * kEnvThreads + threadIdx.x);
  if (i < 0) return;  // a lane without a point loads nothing
  const double* q = P.points + 4 * i;
  const double px = q[0], py = q[1], pz = q[2], time = q[3];
  unsigned long long* st = P.rng + 4 * i;
  Rng g{st[0], st[1], st[2], st[3]};
  // exactly four draws
  const double u0 = uniform01(g), u1 = uniform01(g), u2 = uniform01(g), u3 = uniform01(g);
  const int n = P.n, nc = P.nc;
  const double nd = (double)n;
  // the row: the first r with M_r > x, else the last r with S_r > 0
  const double x = u0 * P.total;
  int row = first_above(P.marg, P.mcoarse, n, nc, P.steps, x);
  if (row >= n) row = P.last_row;
  row = row < 0 ? 0 : (row < n ? row : n - 1);
  // the column: the first c with cum[row][c] > y, else the last c with I > 0
  const double* cum = P.cum + (size_t)row * (size_t)n;
  const double y = u1 * cum[n - 1];
  int col = first_above(cum, P.ccoarse + (size_t)row * (size_t)nc, n, nc, P.steps, y);
  if (col >= n) col = P.lastcol[row];
  col = col < 0 ? 0 : (col < n ? col : n - 1);
  const int cell = row * n + col;
  const double* tx = P.tex + 4 * (size_t)cell;
  const double R = tx[0], G = tx[1], B = tx[2], I = tx[3];
  // the direction
  const double h = 2.0 / nd;
  const double s = ((double)col + u2) * h - 1.0;
  const double t = ((double)row + u3) * h - 1.0;
  const EDir d = env_decode(s, t);
  st[0] = g.s0; st[1] = g.s1; st[2] = g.s2; st[3] = g.s3;
  double* o = P.rays + 7 * i;
  o[0] = px; o[1] = py; o[2] = pz;
  o[3] = d.x; o[4] = d.y; o[5] = d.z;
  o[6] = time;
  P.pdf[i] = env_density(I, P.total, nd, d.len);
  P.texel[i] = cell;
  if (P.color) {
    double* c = P.color + 3 * i;
    c[0] = R; c[1] = G; c[2] = B;
  }
}

__global__ __launch_bounds__(kEnvThreads) void env_eval_kernel(const EParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_items, (long long)blockIdx.x * kEnvThreads + threadIdx.x);
  if (i < 0) return;
  const double* q = P.rays + 7 * i;
  const double dx = q[3], dy = q[4], dz = q[5];
  const int n = P.n;
  const double nd = (double)n;
  // tor_env.h encode
  const double L1 = __builtin_fabs(dx) + __builtin_fabs(dy) + __builtin_fabs(dz);
  const bool usable = (L1 > 0.0) && (L1 < __builtin_inf());
  double R = 0.0, G = 0.0, B = 0.0, pdf = 0.0;
  int cell = -1;
  if (usable) {
    const double qx = dx / L1, qy = dy / L1, qz = dz / L1;
    double s = qx, t = qz;
    if (!(dy >= 0.0)) {
      s = __builtin_copysign(1.0 - __builtin_fabs(qz), qx);
      t = __builtin_copysign(1.0 - __builtin_fabs(qx), qz);
    }
    const int c = env_cell(s, nd, n), r = env_cell(t, nd, n);
    const double len = __builtin_sqrt(qx * qx + qy * qy + qz * qz);
    cell = r * n + c;
    const double* tx = P.tex + 4 * (size_t)cell;
    R = tx[0]; G = tx[1]; B = tx[2];
    pdf = env_density(tx[3], P.total, nd, len);
  }
  double* o = P.color + 3 * i;
  o[0] = R; o[1] = G; o[2] = B;
  if (P.pdf) P.pdf[i] = pdf;
  if (P.texel) P.texel[i] = cell;
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: tor_bounce_device's, then the NULL arrays; then the map
int env_check(const char* who, TorContext* ctx, int64_t n_items, const void* list, int64_t n_list, bool nulls, const char* which) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_items, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_items > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL " + which);
  if (ctx->hitq.env_n <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no environment map (tor_scene_environment)");
  return TOR_OK;
}

// the launches; the arguments are checked, n_items > 0 and n_list > 0
int env_launch(const char* who, TorContext* ctx, bool eval, int64_t n_items, const void* d_points, void* d_rng, const int32_t* d_list,
               int64_t n_list, void* d_rays, double* d_pdf, int32_t* d_texel, double* d_color, hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the queries read the map alone)
  if (rc != TOR_OK) return rc;
  const tor::HitQueryState& hq = ctx->hitq;
  const tor::EnvLayout lay((size_t)hq.env_n);
  const double* base = (const double*)hq.env.ptr;
  tor::EParams P{};
  P.tex = base + lay.tex;
  P.cum = base + lay.cum;
  P.ccoarse = base + lay.ccoarse;
  P.marg = base + lay.marg;
  P.mcoarse = base + lay.mcoarse;
  P.lastcol = (const int*)(base + lay.lastcol);
  P.n = (int)lay.n;
  P.nc = (int)lay.nc;
  P.steps = tor::bit_length((int)lay.nc);
  P.last_row = hq.env_last_row;
  P.total = hq.env_total;
  P.points = (const double*)d_points;
  P.rng = (unsigned long long*)d_rng;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_items = (long long)n_items;
  P.rays = (double*)d_rays;
  P.pdf = d_pdf;
  P.texel = d_texel;
  P.color = d_color;
  const dim3 grid((unsigned)((n_list + tor::kEnvThreads - 1) / tor::kEnvThreads)), block(tor::kEnvThreads);
  if (eval) hipLaunchKernelGGL(tor::env_eval_kernel, grid, block, 0, stream, P);
  else hipLaunchKernelGGL(tor::env_sample_kernel, grid, block, 0, stream, P);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note(eval ? "env eval" : "env sample");
  return TOR_OK;
}

// px, py, pz of decode(s, t) squared and summed, then the square root: decode's len (tor_env.h), on the host
double host_decode_len(double s, double t) {
  const double as = std::fabs(s), at = std::fabs(t);
  const double py = (1.0 - as) - at;
  double px = s, pz = t;
  if (!(py >= 0.0)) {
    px = std::copysign(1.0 - at, s);
    pz = std::copysign(1.0 - as, t);
  }
  return std::sqrt(px * px + py * py + pz * pz);
}

}  // namespace

extern "C" {

int tor_scene_environment(TorContext* ctx, int64_t n, const double* rgb, const double* importance) {
  using tor::fail;
  const std::string w = "tor_scene_environment";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (n < 0 || n > TOR_ENV_MAX_SIDE) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n <= " + std::to_string((int)TOR_ENV_MAX_SIDE));
  if (n > 0 && !rgb) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": rgb is NULL");
  tor::HitQueryState& hq = ctx->hitq;
  if (n == 0) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the map
    hq.env_n = 0;
    return TOR_OK;
  }
  const size_t N = (size_t)n, NN = N * N;
  for (size_t k = 0; k < 3 * NN; ++k)
    if (!std::isfinite(rgb[k]) || rgb[k] < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": rgb must be finite and >= 0");
  if (importance)
    for (size_t k = 0; k < NN; ++k)
      if (!std::isfinite(importance[k]) || importance[k] < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": importance must be finite and >= 0");
  // the tables, on the host
  const tor::EnvLayout lay(N);
  std::vector<double> tab(lay.words, 0.0);
  double* tex = &tab[lay.tex];
  double* cum = &tab[lay.cum];
  double* ccoarse = &tab[lay.ccoarse];
  double* marg = &tab[lay.marg];
  double* mcoarse = &tab[lay.mcoarse];
  int32_t* lastcol = (int32_t*)&tab[lay.lastcol];
  const double h = 2.0 / (double)n;
  double total = 0.0;
  int32_t last_row = -1;
  for (size_t r = 0; r < N; ++r) {
    double run = 0.0;
    int32_t last = -1;
    for (size_t c = 0; c < N; ++c) {
      const size_t k = r * N + c;
      const double R = rgb[3 * k], G = rgb[3 * k + 1], B = rgb[3 * k + 2];
      double I;
      if (importance) {
        I = importance[k];
      } else {
        const double lum = (0.2126 * R + 0.7152 * G) + 0.0722 * B;
        const double len = host_decode_len(((double)c + 0.5) * h - 1.0, ((double)r + 0.5) * h - 1.0);
        const double wt = 1.0 / ((len * len) * len);
        I = lum * wt;
      }
      tex[4 * k] = R; tex[4 * k + 1] = G; tex[4 * k + 2] = B; tex[4 * k + 3] = I;
      run = run + I;
      cum[k] = run;
      if (I > 0.0) last = (int32_t)c;
    }
    for (size_t g = 0; g < lay.nc; ++g) ccoarse[r * lay.nc + g] = cum[r * N + std::min(N - 1, tor::kEnvGroup * g + tor::kEnvGroup - 1)];
    lastcol[r] = last;
    total = total + run;
    marg[r] = total;
    if (run > 0.0) last_row = (int32_t)r;
  }
  for (size_t g = 0; g < lay.nc; ++g) mcoarse[g] = marg[std::min(N - 1, tor::kEnvGroup * g + tor::kEnvGroup - 1)];
  if (!(total > 0.0) || !std::isfinite(total) || last_row < 0)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the importances must add up to a finite total > 0");
  HIP_TRY(hipSetDevice(ctx->device));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the map
  hq.env_n = 0;  // (a failed allocation or copy leaves the context without a map, not with half of one)
  HIP_TRY(hq.env.ensure(tab.size() * 8));
  HIP_TRY(hipMemcpy(hq.env.ptr, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  hq.env_n = n;
  hq.env_total = total;
  hq.env_last_row = last_row;
  return TOR_OK;
}

int tor_env_sample_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                          TorRay* d_rays, double* d_pdf, int32_t* d_texel, double* d_color, void* hip_stream) {
  const char* who = "tor_env_sample_device";
  const int rc = env_check(who, ctx, n_points, d_list, n_list, !d_points || !d_rng || !d_rays || !d_pdf || !d_texel,
                           "points, rng, rays, pdf or texel");
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return env_launch(who, ctx, false, n_points, d_points, d_rng, d_list, n_list, d_rays, d_pdf, d_texel, d_color, (hipStream_t)hip_stream);
}

int tor_env_sample_host(TorContext* ctx, int64_t n_points, const TorPoint* points, TorRng* rng, const int32_t* list, int64_t n_list,
                        TorRay* rays, double* pdf, int32_t* texel, double* color) {
  const char* who = "tor_env_sample_host";
  int rc = env_check(who, ctx, n_points, list, n_list, !points || !rng || !rays || !pdf || !texel, "points, rng, rays, pdf or texel");
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
                         {texel, n * 4, true, true},
                         {color, color ? n * 24 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = env_launch(who, ctx, false, n_points, st[0].dev, st[1].dev, st[2].as<const int32_t>(), n_list, st[3].dev, st[4].as<double>(),
                  st[5].as<int32_t>(), st[6].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

int tor_env_eval_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const int32_t* d_list, int64_t n_list, double* d_color,
                        double* d_pdf, int32_t* d_texel, void* hip_stream) {
  const char* who = "tor_env_eval_device";
  const int rc = env_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_color, "rays or color");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return env_launch(who, ctx, true, n_rays, nullptr, nullptr, d_list, n_list, (void*)d_rays, d_pdf, d_texel, d_color, (hipStream_t)hip_stream);
}

int tor_env_eval_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const int32_t* list, int64_t n_list, double* color, double* pdf,
                      int32_t* texel) {
  const char* who = "tor_env_eval_host";
  int rc = env_check(who, ctx, n_rays, list, n_list, !rays || !color, "rays or color");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_rays;
  tor::HostPart st[5] = {{rays, n * sizeof(TorRay), true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {color, n * 24, true, true},
                         {pdf, pdf ? n * 8 : 0, true, true},
                         {texel, texel ? n * 4 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 5);
  if (rc != TOR_OK) return rc;
  rc = env_launch(who, ctx, true, n_rays, nullptr, nullptr, st[1].as<const int32_t>(), n_list, st[0].dev, st[3].as<double>(),
                  st[4].as<int32_t>(), st[2].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 5);
}

}  // extern "C"
