// tor_radiance.hip -- batched radiance queries (tor_radiance_device / tor_radiance_host, include/tor_render.h): the reference's
// radiance(ray, world, max_depth, rng) (render.nim:21-47) for rays and xoshiro256+ states the caller supplies, and the library's
// camera rays for listed pixels (tor_camera_rays_device: render.nim:63-65 + cameras.nim:47-57), on gfx950.
//
// Exactness.  A bounce is world.hit(r, 0.001, +inf, rec): the hit query's exact test, slab test and block / super-box descent
// (tor_query.hpp, tor_query_descent.inc), whose result is the sequential closest_so_far loop's whatever the visiting order (the
// head of tor_query.hip).  The shading restates materials.nim:21-96 with tor_device.hpp's helpers, operation for operation and
// draw for draw (tor_shade_scatter.inc, the one text of the scatter, shared with the path steps of tor_bounce.hip), as the
// integrator's integrate_shade.inc and the CPU oracle's scatter do: the same cold records (1 / radius, the material flags, the
// host's eta = 1 / ri and Schlick r0 per side), the portable sin/cos and pow5, float64 unfused.  The state a lane writes back is its
// generator after the path's last draw, so a caller can chain samples on one stream as render.nim:59-67 does.
//
// Persistent waves with refill.  Paths end after 1 .. max_depth bounces (random_scene averages 2.6 queries per path).  A lane whose
// path ended writes its colour and state and takes the next ray index of its wave's batch; a wave takes 64 indices per atomicAdd on
// a head counter (zeroed on the stream before each launch), so the dequeue is paid once per 64 paths and no wave idles while others
// still have work.  The descent runs with every lane of the wave, live or idle (its uniform loops use scalar loads).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_shade.hpp"

static_assert(sizeof(TorRng) == 32 && offsetof(TorRng, s1) == 8 && offsetof(TorRng, s2) == 16 && offsetof(TorRng, s3) == 24,
              "TorRng: Rng (support/rng.nim:18-19)");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");
static_assert(sizeof(TorCamera) == sizeof(tor::Camera), "TorCamera mirrors tor::Camera");

namespace tor {
namespace {

constexpr int kRadThreads = 256;
constexpr int kCamThreads = 256;

struct RParams {
  QParams q;                 // the scene and its boxes (rays, t_range, hits unused)
  const double* rays;        // 7 float64 per ray (TorRay)
  unsigned long long* rng;   // 4 u64 per ray (TorRng), read and written
  double* color;             // 3 float64 per ray
  unsigned long long* head;  // next unclaimed ray index; 0 at launch
  long long n_rays;
  int max_depth;             // >= 1 (max_depth 0 never launches)
};

template <bool BLOCKS>
__global__ __launch_bounds__(kRadThreads) __attribute__((amdgpu_waves_per_eu(4))) void radiance_kernel(const RParams P) {
  const QParams& p = P.q;
  const Sees<false> vis{nullptr, nullptr, 0u};  // the descent's `vis`: no masks here
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long idx = -1;  // this lane's ray, -1: none
  // the lane's ray lives in r (origin, direction, time; t_min = 0.001 as render.nim:28): no second copy for the descent
  QRay r{};
  r.t_min = 0.001;
  V3 att{};
  Rng g{};
  int depth = 0;
  long long bnext = 0;  // wave-uniform: the wave's batch [bnext, bnext + bleft)
  int bleft = 0;
  bool dry = false;     // the counter has passed n_rays
  for (;;) {
    // refill: the lanes without a path take the next indices of the batch, in lane order; a new batch when it runs out
    unsigned long long need = __ballot(idx < 0);
    while (need != 0 && !dry) {
      if (bleft == 0) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(P.head, 64ull);
        base = __shfl(base, 0);
        if (base >= (unsigned long long)P.n_rays) {
          dry = true;
          break;
        }
        bnext = (long long)base;
        bleft = P.n_rays - bnext < 64 ? (int)(P.n_rays - bnext) : 64;
      }
      const int n_need = __popcll(need);
      const int take = n_need < bleft ? n_need : bleft;
      if (idx < 0) {
        const int rank = __popcll(need & below);
        if (rank < take) {
          idx = bnext + rank;
          const double* q = P.rays + 7 * idx;
          r.ox = q[0]; r.oy = q[1]; r.oz = q[2];
          r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
          r.time = q[6];
          const unsigned long long* s = P.rng + 4 * idx;
          g.s0 = s[0]; g.s1 = s[1]; g.s2 = s[2]; g.s3 = s[3];
          att = v3(1.0, 1.0, 1.0);
          depth = 0;
        }
      }
      bnext += take;
      bleft -= take;
      need = __ballot(idx < 0);
    }
    const bool live = idx >= 0;
    if (__ballot(live) == 0) break;

    // world.hit(r, 0.001, +inf, rec) (render.nim:28)
    r.t_max = live ? __builtin_inf() : 0.0;  // (idle lanes: t_max = 0 accepts nothing)
    r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30
    QBest b{r.t_max, INT_MAX, -1};
#include "tor_query_descent.inc"
    if (!live) continue;

    // shade: the sky, or the scatter (materials.nim:21-96) and the depth bookkeeping (render.nim:25,47)
    bool ended = false;
    V3 radiance = v3(0.0, 0.0, 0.0);
    const V3 o = v3(r.ox, r.oy, r.oz), d = v3(r.dx, r.dy, r.dz);
    const V3 ud = unit_vector(d);  // render.nim:42, materials.nim:40,68: one copy serves the sky, Metal and Dielectric
    if (b.slot < 0) {
      radiance = sky_unit(ud, att);  // render.nim:41-45
      ended = true;
    } else {
      const double* c = p.cold + 16 * (size_t)b.slot;
      double cx, cy, cz;
      centre_at(c, r.time, cx, cy, cz);                                 // moving_spheres.nim:39-44
      const V3 hp = o + d * b.t;                                       // rays.nim:24-25
      const V3 outward = (hp - v3(cx, cy, cz)) * c[6];                 // spheres.nim:43 (c[6] = 1.0 / radius)
      const bool front = dot(d, outward) < 0.0;                        // core.nim:47-49
      const V3 n = front ? outward : -outward;
#include "tor_shade_scatter.inc"
      if (!ended) {
        depth += 1;
        if (depth >= P.max_depth) ended = true;  // render.nim:25,47: loop exhausted -> black
      }
    }
    if (ended) {
      double* out = P.color + 3 * idx;
      out[0] = radiance.x; out[1] = radiance.y; out[2] = radiance.z;
      unsigned long long* s = P.rng + 4 * idx;
      s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
      idx = -1;
    }
  }
}

struct CParams {
  Camera cam;
  const int* pixels;      // flat pixel indices, or null: entry e is pixel e
  unsigned long long* rng;  // 4 u64 per (entry, sample)
  double* rays;           // 7 float64 per (entry, sample)
  long long n_items;      // n_pixels * n_samples
  int nrows, ncols, n_samples, first_sample;
  int seeding;            // TOR_SEED_SAMPLE: seed3 per sample; TOR_SEED_PIXEL: the state in rng, read and written
};

// render.nim:63-65 + cameras.nim:47-57 for one (pixel, sample), as the integrator and the CPU oracle's pixel_sample draw them
__global__ __launch_bounds__(kCamThreads) void camera_rays_kernel(const CParams p) {
  const long long i = (long long)blockIdx.x * kCamThreads + threadIdx.x;
  if (i >= p.n_items) return;
  const long long e = i / p.n_samples;
  const int k = (int)(i - e * p.n_samples);
  const long long pix = p.pixels ? (long long)p.pixels[e] : e;
  if (pix < 0 || pix >= (long long)p.nrows * p.ncols) return;  // outside the canvas: skipped
  const int row = (int)(pix / p.ncols), col = (int)(pix % p.ncols);
  unsigned long long* s = p.rng + 4 * i;
  Rng g;
  if (p.seeding == TOR_SEED_SAMPLE) {
    seed3(g, (uint64_t)row, (uint64_t)col, (uint64_t)p.first_sample + (uint64_t)k);
  } else {
    g.s0 = s[0]; g.s1 = s[1]; g.s2 = s[2]; g.s3 = s[3];
  }
  const double u = ((double)col + uniform01(g)) / (double)(p.ncols - 1);
  const double v = ((double)row + uniform01(g)) / (double)(p.nrows - 1);
  const Ray r = camera_ray(p.cam, u, v, g);
  double* o = p.rays + 7 * i;
  o[0] = r.origin.x; o[1] = r.origin.y; o[2] = r.origin.z;
  o[3] = r.direction.x; o[4] = r.direction.y; o[5] = r.direction.z;
  o[6] = r.time;
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
}

}  // namespace
}  // namespace tor

namespace {

constexpr int64_t kMaxItems = (int64_t)0x7fffffff * 256;  // at most 2^31 - 1 workgroups of 256 lanes

int radiance_args(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, const void* rng, int32_t max_depth,
                  double time_lo, double time_hi, int32_t mode, const void* color) {
  using tor::fail;
  const std::string w = who;
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (n_rays < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_rays < 0");
  if (n_rays > kMaxItems) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_rays above 2^31 - 1 workgroups of 256 rays");
  if (max_depth < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": max_depth < 0");
  if (!std::isfinite(time_lo) || !std::isfinite(time_hi) || time_lo > time_hi)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the time range must be finite with time_lo <= time_hi");
  if (mode < TOR_HIT_AUTO || mode > TOR_HIT_BLOCKS)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": mode must be TOR_HIT_AUTO (0), TOR_HIT_BRUTE (1) or TOR_HIT_BLOCKS (2)");
  if (n_rays > 0 && (!rays || !rng || !color)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays, rng or color");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  return TOR_OK;
}

// the launch; the arguments are checked and n_rays > 0
int radiance_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, void* d_rng, int32_t max_depth,
                    double time_lo, double time_hi, int32_t mode, double* d_color, hipStream_t stream) {
  tor::HitQueryState& hq = ctx->hitq;
  // scattered Metal and Dielectric rays carry time 0: the boxes are built for a range that holds it
  const double lo = time_lo < 0.0 ? time_lo : 0.0, hi = time_hi > 0.0 ? time_hi : 0.0;
  tor::RParams P{};
  bool blocks = false;
  std::string why;
  const int rc = tor::query_setup(who, ctx, lo, hi, mode, stream, P.q, blocks, why);
  if (rc != TOR_OK) return rc;
  if (max_depth == 0) {  // render.nim:25: no bounce, black, no draw
    HIP_TRY(hipMemsetAsync(d_color, 0, (size_t)n_rays * 3 * sizeof(double), stream));
  } else {
    HIP_TRY(hq.head.ensure(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(hq.head.ptr, 0, sizeof(unsigned long long), stream));
    P.rays = (const double*)d_rays;
    P.rng = (unsigned long long*)d_rng;
    P.color = d_color;
    P.head = (unsigned long long*)hq.head.ptr;
    P.n_rays = (long long)n_rays;
    P.max_depth = max_depth;
    // persistent waves: enough workgroups to fill the device, never more than the rays need
    const int64_t need = (n_rays + tor::kRadThreads - 1) / tor::kRadThreads;
    const int64_t fill = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
    const unsigned grid = (unsigned)(need < fill ? need : fill);
    if (blocks) hipLaunchKernelGGL(tor::radiance_kernel<true>, dim3(grid), dim3(tor::kRadThreads), 0, stream, P);
    else hipLaunchKernelGGL(tor::radiance_kernel<false>, dim3(grid), dim3(tor::kRadThreads), 0, stream, P);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(hq.ev_done, stream));
  hq.launched = true;
  hq.stream = (void*)stream;
  tor::set_last_note(blocks ? std::string("radiance: blocks")
                            : std::string("radiance: brute force") + (why.empty() ? std::string() : " (" + why + ")"));
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_radiance_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, TorRng* d_rng, int32_t max_depth, double time_lo,
                        double time_hi, int32_t mode, double* d_color, void* hip_stream) {
  const int rc = radiance_args("tor_radiance_device", ctx, n_rays, d_rays, d_rng, max_depth, time_lo, time_hi, mode, d_color);
  if (rc != TOR_OK) return rc;
  if (n_rays == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  return radiance_launch("tor_radiance_device", ctx, n_rays, d_rays, d_rng, max_depth, time_lo, time_hi, mode, d_color,
                         (hipStream_t)hip_stream);
}

int tor_radiance_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, TorRng* rng, int32_t max_depth, double time_lo,
                      double time_hi, int32_t mode, double* color) {
  int rc = radiance_args("tor_radiance_host", ctx, n_rays, rays, rng, max_depth, time_lo, time_hi, mode, color);
  if (rc != TOR_OK) return rc;
  if (n_rays == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t ray_bytes = (size_t)n_rays * sizeof(TorRay), rng_bytes = (size_t)n_rays * sizeof(TorRng);
  const size_t color_bytes = (size_t)n_rays * 3 * sizeof(double);
  tor::HitQueryState& hq = ctx->hitq;
  // blocking entry: it waits for the context's last render launch and last query, on whatever stream they run (tor_hit_host)
  if (ctx->launches > 0) HIP_TRY(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));
  HIP_TRY(hq.io.ensure(ray_bytes + rng_bytes + color_bytes));
  char* base = (char*)hq.io.ptr;
  HIP_TRY(hipMemcpy(base, rays, ray_bytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(base + ray_bytes, rng, rng_bytes, hipMemcpyHostToDevice));
  rc = radiance_launch("tor_radiance_host", ctx, n_rays, base, base + ray_bytes, max_depth, time_lo, time_hi, mode,
                       (double*)(base + ray_bytes + rng_bytes), nullptr);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipMemcpy(color, base + ray_bytes + rng_bytes, color_bytes, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rng, base + ray_bytes, rng_bytes, hipMemcpyDeviceToHost));
  return TOR_OK;
}

int tor_camera_rays_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, const int32_t* d_pixels,
                           int64_t n_pixels, int32_t first_sample, int32_t n_samples, int32_t seeding, TorRng* d_rng, TorRay* d_rays,
                           void* hip_stream) {
  using tor::fail;
  const std::string w = "tor_camera_rays_device";
  if (!ctx || !cam) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx or cam is NULL");
  if (nrows < 2 || ncols < 2) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": nrows and ncols must be >= 2");
  if (n_pixels < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_pixels < 0");
  if (!d_pixels && n_pixels != (int64_t)nrows * ncols)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": without a pixel list n_pixels must be nrows * ncols");
  if (seeding != TOR_SEED_SAMPLE && seeding != TOR_SEED_PIXEL)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": seeding must be TOR_SEED_PIXEL (0) or TOR_SEED_SAMPLE (1)");
  if (seeding == TOR_SEED_PIXEL) {
    if (n_samples != 1) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": TOR_SEED_PIXEL takes n_samples == 1");
    first_sample = 0;
  }
  if (first_sample < 0 || n_samples < 1 || (int64_t)first_sample + n_samples > (int64_t)INT32_MAX)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need first_sample >= 0, n_samples >= 1, first_sample + n_samples <= 2^31 - 1");
  if (n_pixels > kMaxItems / n_samples) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_pixels * n_samples too large");
  if (n_pixels > 0 && (!d_rng || !d_rays)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rng or rays");
  if (n_pixels == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  tor::CParams p{};
  std::memcpy(&p.cam, cam, sizeof(TorCamera));
  p.pixels = d_pixels;
  p.rng = (unsigned long long*)d_rng;
  p.rays = (double*)d_rays;
  p.n_items = (long long)(n_pixels * n_samples);
  p.nrows = nrows;
  p.ncols = ncols;
  p.n_samples = n_samples;
  p.first_sample = first_sample;
  p.seeding = seeding;
  const unsigned grid = (unsigned)((p.n_items + tor::kCamThreads - 1) / tor::kCamThreads);
  hipLaunchKernelGGL(tor::camera_rays_kernel, dim3(grid), dim3(tor::kCamThreads), 0, (hipStream_t)hip_stream, p);
  HIP_TRY(hipGetLastError());
  return TOR_OK;
}

}  // extern "C"
