// tor_media.hip -- participating-media queries for host integrators (tor_scene_media, tor_media_march_device,
// tor_media_scatter_device, tor_rng_uniform_device and the blocking _host twins, include/tor_media.h): where along each listed ray
// the optical depth through a table of homogeneous spherical media reaches a budget, the isotropic scatter at that collision, and
// plain uniforms from a path's stream, on gfx950.  include/tor_media.h holds the definition, operation by operation; this file
// follows it line by line (medium_roots, the step loop, the mixture).
//
// The media table (tor_scene_media) is one device record of 16 float64 per medium, packed when the table is set:
//     [0..2] center / center0   [3..5] center1 - center0   [6] time0   [7] time1 - time0   [8] 1.0 for a MovingSphere, else 0.0
//     [9] radius * radius   [10] sigma   [11..13] albedo   [14] the object's index in the uploaded list (int64 bits)   [15] g: 0.0 here;
//     tor_scene_media_phase (tor_phase.hip) sets the asymmetry of the phase function
// -- the centre data and radius * radius are the scene's cold record's (tor_kernels.hpp), so the roots are roots_of's
// (tor_crossings.hip) operation for operation.  Medium m is read at a wave-uniform address through the scalar-load view.
//
//   media_march_kernel    one listed ray per lane.  Pass 1 walks the table once and gives each lane a 64-bit `touch` word: the media
//                         one of whose comparisons in the march can hold for this ray at all (below), and the wave the union of
//                         its lanes' words (ballots, so the union lives in scalar registers).  The step loop is the header's
//                         counted loop; each step walks the set bits of the union, ascending, and computes the roots again --
//                         the roots of 64 media do not fit a lane's registers, and the same operations give the same bits.  A lane
//                         that is done keeps its answer in registers and takes no further part; the loop ends early when the
//                         whole wave is done (a wave-uniform exit: no lane waits for another, and a wrong table or a wrong
//                         compare shows as a wrong answer, never as a hang: the trip count is bounded by 2 * n_media + 1).
//   media_scatter_kernel  one listed ray per lane: two generator outputs, the mixture over the active bits in a wave-uniform loop
//   rng_uniform_kernel    one listed state per lane
//
// The touch word.  Medium m enters the march of a ray only through three comparisons, at some t with t_min <= t < t_max and some
// t_next <= t_max:  (A) s0 <= t && t < s1,  (B) s0 > t && s0 < t_next,  (C) s1 > t && s1 < t_next.  (A) implies s0 < t_max && s1 >
// t_min; (B) implies t_min < s0 < t_max; (C) implies t_min < s1 < t_max.  touch_m = has_m && ((A') || (B') || (C')) with those
// three implied conditions: a medium without the bit can change neither rho, A nor t_next at any step, whatever NaN or infinity
// its roots hold, so skipping it leaves every bit of the answer as the header defines it.  A medium with a density grid
// (include/tor_grid.h; the kernel's grid_mask) never gets the bit: the march answers as if has_m were false for it, and it contributes
// through tor_media_grid_march_device alone.  With no grid the mask is 0 and every bit of every answer is as it was.
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

#include "../../include/tor_media.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"

static_assert(sizeof(TorRay) == 56 && sizeof(TorRng) == 32, "TorRay / TorRng as the kernels index them");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");
static_assert(TOR_MEDIA_MAX == 64, "the active set is one 64-bit word");

namespace tor {
namespace {

constexpr int kMediaThreads = 256;
constexpr int kMediaWords = 16;  // float64 per medium record

struct MdParams {
  const double* media;          // n_media records of kMediaWords float64
  int n_media;
  const double* rays;           // 7 float64 per ray (TorRay)
  const double* t_range;        // 2 float64 per ray, or null: (0.0, +inf)
  const double* tau;            // the march: one budget per ray
  const double* t_in;           // the scatter: the collision's parameter per ray ...
  const unsigned long long* active_in;  // ... and its active set
  unsigned long long* rng;      // the scatter: 4 u64 per ray (TorRng), read and written
  const int* list;              // the rays to answer, or null: entry e is ray e
  long long n_list, n_rays;
  int* status;                  // the march's outputs, one per ray
  double* t;
  double* depth;
  unsigned long long* active;
  double* rho;                  // ... or null
  double* rays_out;             // the scatter's outputs: 7 float64 per ray
  double* att;                  // ... and 3
};

struct MdRoots {
  double s0, s1;
  bool has;
};

// tor_media.h "per medium": roots_of's operations (tor_crossings.hip) on the record's centre data, unclipped
template <typename P>
__device__ __forceinline__ MdRoots medium_roots(P r, const QRay& q) {
  double cx = r[0], cy = r[1], cz = r[2];
  if (r[8] != 0.0) {
    const double f = (q.time - r[6]) / r[7];
    cx = cx + r[3] * f; cy = cy + r[4] * f; cz = cz + r[5] * f;
  }
  const double ocx = q.ox - cx, ocy = q.oy - cy, ocz = q.oz - cz;
  const double hb = ocx * q.dx + ocy * q.dy + ocz * q.dz;
  const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r[9];
  const double disc = hb * hb - q.a * cc;
  MdRoots x{0.0, 0.0, false};
  if (disc > 0.0) {
    const double root = __builtin_sqrt(disc);
    x.s0 = (-hb - root) / q.a;
    x.s1 = (-hb + root) / q.a;
    x.has = true;
  }
  return x;
}

// grid_mask: bit m set: medium m has a density grid (tor_grid.hip) and takes no part here
__global__ __launch_bounds__(kMediaThreads) void media_march_kernel(const MdParams P, const unsigned long long grid_mask) {
  const long long i = listed_ray(P.list, P.n_list, P.n_rays, (long long)blockIdx.x * kMediaThreads + threadIdx.x);
  const bool live = i >= 0;
  QRay q{};
  double tau = 0.0;
  if (live) {
    const double* s = P.rays + 7 * i;
    q.ox = s[0]; q.oy = s[1]; q.oz = s[2];
    q.dx = s[3]; q.dy = s[4]; q.dz = s[5];
    q.time = s[6];
    q.t_min = P.t_range ? P.t_range[2 * i] : 0.0;
    q.t_max = P.t_range ? P.t_range[2 * i + 1] : __builtin_inf();
    tau = P.tau[i];
  }
  q.a = q.dx * q.dx + q.dy * q.dy + q.dz * q.dz;
  const double len = __builtin_sqrt(q.a);
  const bool refused = !(tau >= 0.0) || !(q.t_min < q.t_max);
  bool done = !live || refused;
  const qcdptr M = (qcdptr)(uintptr_t)P.media;
  const int n = P.n_media;
  // pass 1: the lane's touch word and the wave's union
  unsigned long long touch = 0ull, uni = 0ull;
  for (int m = 0; m < n; ++m) {
    const MdRoots x = medium_roots(M + kMediaWords * (size_t)m, q);
    const bool tm = !done && x.has && ((grid_mask >> m) & 1ull) == 0ull &&
                    ((x.s0 < q.t_max && x.s1 > q.t_min) || (x.s0 > q.t_min && x.s0 < q.t_max) || (x.s1 > q.t_min && x.s1 < q.t_max));
    if (tm) touch |= 1ull << m;
    if (__ballot(tm) != 0ull) uni |= 1ull << m;
  }
  uni = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(uni >> 32)) << 32) |
        (unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)uni);
  // the answer of a ray that is refused, and of one that escapes before its first step
  int status = refused ? -1 : 0;
  double out_t = refused ? q.t_min : q.t_max, out_depth = 0.0, out_rho = 0.0;
  unsigned long long out_active = 0ull;
  double t = q.t_min, D = 0.0;
  const int bound = 2 * n + 1;
  for (int it = 0; it < bound; ++it) {
    if (__ballot(!done) == 0ull) break;
    double rho = 0.0, t_next = q.t_max;
    unsigned long long A = 0ull;
    for (unsigned long long u = uni; u != 0ull; u &= u - 1ull) {
      const int m = __builtin_ctzll(u);
      const qcdptr r = M + kMediaWords * (size_t)m;
      const MdRoots x = medium_roots(r, q);
      if ((touch >> m) & 1ull) {
        if (x.s0 <= t && t < x.s1) {
          rho = rho + r[10];
          A |= 1ull << m;
        }
        if (x.s0 > t && x.s0 < t_next) t_next = x.s0;
        if (x.s1 > t && x.s1 < t_next) t_next = x.s1;
      }
    }
    const double step = rho > 0.0 ? rho * ((t_next - t) * len) : 0.0;
    const double rem = tau - D;
    if (!done) {
      if (rho > 0.0 && rem < step) {
        double t_c = t + (rem / rho) / len;
        if (t_next < t_c) t_c = t_next;
        status = 1; out_t = t_c; out_depth = tau; out_active = A; out_rho = rho;
        done = true;
      } else {
        D = D + step;
        out_depth = D;
        if (!(t_next < q.t_max)) done = true;
        else t = t_next;
      }
    }
  }
  if (!live) return;
  P.status[i] = status;
  P.t[i] = out_t;
  P.depth[i] = out_depth;
  P.active[i] = out_active;
  if (P.rho) P.rho[i] = out_rho;
}

__global__ __launch_bounds__(kMediaThreads) void media_scatter_kernel(const MdParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_rays, (long long)blockIdx.x * kMediaThreads + threadIdx.x);
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
  // exactly two outputs of the generator, whatever follows
  const V3 v = random_unit_vector(g);
  const qcdptr M = (qcdptr)(uintptr_t)P.media;
  const int n = P.n_media;
  double rho = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
  for (int m = 0; m < n; ++m) {
    const qcdptr r = M + kMediaWords * (size_t)m;
    if ((active >> m) & 1ull) {
      const double sg = r[10];
      rho = rho + sg;
      nx = nx + sg * r[11]; ny = ny + sg * r[12]; nz = nz + sg * r[13];
    }
  }
  if (!live) return;
  unsigned long long* s = P.rng + 4 * i;
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
  double* o = P.rays_out + 7 * i;
  double* a = P.att + 3 * i;
  const bool beyond = n < 64 && (active >> n) != 0ull;  // a bit at or above n_media
  if (active == 0ull || beyond || !(rho > 0.0)) {
    for (int k = 0; k < 7; ++k) o[k] = 0.0;
    a[0] = 0.0; a[1] = 0.0; a[2] = 0.0;
    return;
  }
  o[0] = ray[0] + t * ray[3]; o[1] = ray[1] + t * ray[4]; o[2] = ray[2] + t * ray[5];
  o[3] = v.x; o[4] = v.y; o[5] = v.z;
  o[6] = ray[6];
  a[0] = nx / rho; a[1] = ny / rho; a[2] = nz / rho;
}

struct UParams {
  unsigned long long* rng;  // 4 u64 per state (TorRng), read and written
  const int* list;
  long long n_list, n_states;
  int n_draws;
  double* out;              // n_draws float64 per state
};

__global__ __launch_bounds__(kMediaThreads) void rng_uniform_kernel(const UParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_states, (long long)blockIdx.x * kMediaThreads + threadIdx.x);
  if (i < 0) return;
  unsigned long long* s = P.rng + 4 * i;
  Rng g{s[0], s[1], s[2], s[3]};
  double* o = P.out + (size_t)i * (size_t)P.n_draws;
  for (int k = 0; k < P.n_draws; ++k) o[k] = uniform01(g);
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: tor_light_sample_device's, then the NULL arrays; then the scene and its
// media table
int media_check(const char* who, TorContext* ctx, int64_t n_rays, const void* list, int64_t n_list, bool nulls, const char* names) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_rays, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL " + names);
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  if (ctx->hitq.n_media <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no media table (tor_scene_media)");
  return TOR_OK;
}

unsigned media_grid(int64_t n_list) { return (unsigned)((n_list + tor::kMediaThreads - 1) / tor::kMediaThreads); }

// the launches; the arguments are checked, n_rays > 0 and n_list > 0
int media_launch(const char* who, TorContext* ctx, bool scatter, tor::MdParams& P, int64_t n_rays, const int32_t* d_list, int64_t n_list,
                 hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the queries read the media table alone)
  if (rc != TOR_OK) return rc;
  P.media = (const double*)ctx->hitq.media.ptr;
  P.n_media = (int)ctx->hitq.n_media;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_rays = (long long)n_rays;
  const dim3 grid(media_grid(n_list)), block(tor::kMediaThreads);
  if (scatter) hipLaunchKernelGGL(tor::media_scatter_kernel, grid, block, 0, stream, P);
  else hipLaunchKernelGGL(tor::media_march_kernel, grid, block, 0, stream, P, (unsigned long long)ctx->hitq.grid_mask);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note(std::string(scatter ? "media scatter: " : "media march: ") + std::to_string(ctx->hitq.n_media) + " media");
  return TOR_OK;
}

int march_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, const double* d_tau,
                 const int32_t* d_list, int64_t n_list, int32_t* d_status, double* d_t, double* d_depth, uint64_t* d_active, double* d_rho,
                 hipStream_t stream) {
  tor::MdParams P{};
  P.rays = (const double*)d_rays;
  P.t_range = d_t_range;
  P.tau = d_tau;
  P.status = d_status;
  P.t = d_t;
  P.depth = d_depth;
  P.active = (unsigned long long*)d_active;
  P.rho = d_rho;
  return media_launch(who, ctx, false, P, n_rays, d_list, n_list, stream);
}

int scatter_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t, const uint64_t* d_active,
                   void* d_rng, const int32_t* d_list, int64_t n_list, void* d_rays_out, double* d_att, hipStream_t stream) {
  tor::MdParams P{};
  P.rays = (const double*)d_rays;
  P.t_in = d_t;
  P.active_in = (const unsigned long long*)d_active;
  P.rng = (unsigned long long*)d_rng;
  P.rays_out = (double*)d_rays_out;
  P.att = d_att;
  return media_launch(who, ctx, true, P, n_rays, d_list, n_list, stream);
}

int uniform_check(const char* who, TorContext* ctx, int64_t n_states, const void* list, int64_t n_list, int32_t n_draws, const void* rng,
                  const void* out) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_states, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_draws < 1 || n_draws > TOR_UNIFORM_MAX_DRAWS)
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_draws must be in 1 .. TOR_UNIFORM_MAX_DRAWS (" + std::to_string(TOR_UNIFORM_MAX_DRAWS) + ")");
  if (n_states > 0 && n_list > 0 && (!rng || !out)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rng or out");
  return TOR_OK;
}

int uniform_launch(const char* who, TorContext* ctx, int64_t n_states, void* d_rng, const int32_t* d_list, int64_t n_list, int32_t n_draws,
                   double* d_out, hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::UParams P{};
  P.rng = (unsigned long long*)d_rng;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_states = (long long)n_states;
  P.n_draws = n_draws;
  P.out = d_out;
  hipLaunchKernelGGL(tor::rng_uniform_kernel, dim3(media_grid(n_list)), dim3(tor::kMediaThreads), 0, stream, P);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note("rng uniform: " + std::to_string(n_draws) + (n_draws == 1 ? " draw" : " draws"));
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_scene_media(TorContext* ctx, int64_t n_media, const int32_t* objects, const double* sigma, const double* albedo) {
  using tor::fail;
  const std::string w = "tor_scene_media";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  const int64_t n = ctx->n_objects;
  if (n_media < 0 || n_media > n) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_media <= the uploaded list's length (" + std::to_string(n) + ")");
  if (n_media > TOR_MEDIA_MAX) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_media above TOR_MEDIA_MAX (" + std::to_string(TOR_MEDIA_MAX) + ")");
  if (n_media > 0 && (!objects || !sigma)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": objects or sigma is NULL");
  std::vector<char> seen((size_t)n, 0);
  for (int64_t j = 0; j < n_media; ++j) {
    const int64_t o = objects[j];
    if (o < 0 || o >= n) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": objects[" + std::to_string(j) + "] is outside the uploaded list");
    if (seen[(size_t)o]) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": object " + std::to_string(o) + " is listed twice");
    seen[(size_t)o] = 1;
    if (!std::isfinite(sigma[j]) || sigma[j] < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": sigma must be finite and >= 0");
    for (int k = 0; albedo && k < 3; ++k)
      if (!std::isfinite(albedo[3 * j + k]) || albedo[3 * j + k] < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": albedo must be finite and >= 0");
  }
  // the records, from the scene's cold records (by original index)
  std::vector<double> recs((size_t)n_media * tor::kMediaWords, 0.0);
  if (n_media > 0) {
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
    for (int64_t j = 0; j < n_media; ++j) {
      const int64_t o = objects[j];
      if (slot_of[(size_t)o] < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the flat layout holds no record of object " + std::to_string(o));
      const double* c = &lay.cold[16 * (size_t)slot_of[(size_t)o]];
      double* r = &recs[(size_t)j * tor::kMediaWords];
      int64_t flags;
      std::memcpy(&flags, &c[13], 8);
      for (int k = 0; k < 6; ++k) r[k] = c[k];
      r[6] = c[7];
      r[7] = c[8];
      r[8] = ((int)flags & 1) ? 1.0 : 0.0;
      r[9] = c[15];
      r[10] = sigma[j];
      for (int k = 0; k < 3; ++k) r[11 + k] = albedo ? albedo[3 * j + k] : 1.0;
      std::memcpy(&r[14], &o, 8);
    }
  }
  HIP_TRY(hipSetDevice(ctx->device));
  tor::HitQueryState& hq = ctx->hitq;
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the table
  if (n_media > 0) {
    HIP_TRY(hq.media.ensure(recs.size() * 8));
    HIP_TRY(hipMemcpy(hq.media.ptr, recs.data(), recs.size() * 8, hipMemcpyHostToDevice));
  }
  hq.n_media = n_media;
  hq.drop_grids();  // a new table: no medium has a density grid (tor_scene_media_grid), as none has a g
  return TOR_OK;
}

int tor_media_march_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const double* d_tau,
                           const int32_t* d_list, int64_t n_list, int32_t* d_status, double* d_t, double* d_depth, uint64_t* d_active,
                           double* d_rho, void* hip_stream) {
  const char* who = "tor_media_march_device";
  const int rc = media_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_tau || !d_status || !d_t || !d_depth || !d_active,
                             "rays, tau, status, t, depth or active");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return march_launch(who, ctx, n_rays, d_rays, d_t_range, d_tau, d_list, n_list, d_status, d_t, d_depth, d_active, d_rho,
                      (hipStream_t)hip_stream);
}

int tor_media_march_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const double* tau, const int32_t* list,
                         int64_t n_list, int32_t* status, double* t, double* depth, uint64_t* active, double* rho) {
  const char* who = "tor_media_march_host";
  int rc = media_check(who, ctx, n_rays, list, n_list, !rays || !tau || !status || !t || !depth || !active,
                       "rays, tau, status, t, depth or active");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too, rays that are not listed keep what the caller holds --, the query on the default stream,
  // the outputs back
  const size_t n = (size_t)n_rays;
  tor::HostPart st[9] = {{rays, n * sizeof(TorRay), true, false},
                         {t_range, t_range ? n * 16 : 0, true, false},
                         {tau, n * 8, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {status, n * 4, true, true},
                         {t, n * 8, true, true},
                         {depth, n * 8, true, true},
                         {active, n * 8, true, true},
                         {rho, rho ? n * 8 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 9);
  if (rc != TOR_OK) return rc;
  rc = march_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const double>(), st[3].as<const int32_t>(), n_list,
                    st[4].as<int32_t>(), st[5].as<double>(), st[6].as<double>(), st[7].as<uint64_t>(), st[8].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 9);
}

int tor_media_scatter_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t, const uint64_t* d_active, TorRng* d_rng,
                             const int32_t* d_list, int64_t n_list, TorRay* d_rays_out, double* d_att, void* hip_stream) {
  const char* who = "tor_media_scatter_device";
  const int rc = media_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_t || !d_active || !d_rng || !d_rays_out || !d_att,
                             "rays, t, active, rng, rays_out or att");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return scatter_launch(who, ctx, n_rays, d_rays, d_t, d_active, d_rng, d_list, n_list, d_rays_out, d_att, (hipStream_t)hip_stream);
}

int tor_media_scatter_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t, const uint64_t* active, TorRng* rng,
                           const int32_t* list, int64_t n_list, TorRay* rays_out, double* att) {
  const char* who = "tor_media_scatter_host";
  int rc = media_check(who, ctx, n_rays, list, n_list, !rays || !t || !active || !rng || !rays_out || !att,
                       "rays, t, active, rng, rays_out or att");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_rays;
  const bool alias = (const void*)rays_out == (const void*)rays;  // one staged copy then: read, and written back
  tor::HostPart st[7] = {{rays, n * sizeof(TorRay), true, alias},
                         {t, n * 8, true, false},
                         {active, n * 8, true, false},
                         {rng, n * sizeof(TorRng), true, true},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {rays_out, alias ? 0 : n * sizeof(TorRay), true, true},
                         {att, n * 24, true, true}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = scatter_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const uint64_t>(), st[3].dev,
                      st[4].as<const int32_t>(), n_list, alias ? st[0].dev : st[5].dev, st[6].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

int tor_rng_uniform_device(TorContext* ctx, int64_t n_states, TorRng* d_rng, const int32_t* d_list, int64_t n_list, int32_t n_draws,
                           double* d_out, void* hip_stream) {
  const char* who = "tor_rng_uniform_device";
  const int rc = uniform_check(who, ctx, n_states, d_list, n_list, n_draws, d_rng, d_out);
  if (rc != TOR_OK || n_states == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return uniform_launch(who, ctx, n_states, d_rng, d_list, n_list, n_draws, d_out, (hipStream_t)hip_stream);
}

int tor_rng_uniform_host(TorContext* ctx, int64_t n_states, TorRng* rng, const int32_t* list, int64_t n_list, int32_t n_draws, double* out) {
  const char* who = "tor_rng_uniform_host";
  int rc = uniform_check(who, ctx, n_states, list, n_list, n_draws, rng, out);
  if (rc != TOR_OK || n_states == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_states;
  tor::HostPart st[3] = {{rng, n * sizeof(TorRng), true, true},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {out, n * 8 * (size_t)n_draws, true, true}};
  rc = tor::stage_in(ctx, st, 3);
  if (rc != TOR_OK) return rc;
  rc = uniform_launch(who, ctx, n_states, st[0].dev, st[1].as<const int32_t>(), n_list, n_draws, st[2].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 3);
}

}  // extern "C"
