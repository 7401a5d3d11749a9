// tor_camera.hip -- light-tracing queries for host integrators (tor_camera_connect_device, tor_light_emit_device and the blocking
// _host twins, include/tor_camera.h): a path started ON a lamp of the context's light table, and for a world point the pixel it
// lands in, the lens point and the measurement weight, on gfx950 -- the two endpoints a light tracer needs, whose splats
// tor_deposit_device takes.  include/tor_camera.h holds the definition, operation by operation; this file follows it line by line.
//
//   camera_connect_kernel   one point per lane; the per-camera constants (fd, H . H, V . V, K) are computed once on the host with
//                           the header's operations and come by value with the camera, so they sit in SGPRs.  Streaming: 32 bytes
//                           of point and 32 of state in, 32 of state, 56 of ray, 4 of pixel, 8 of factor (and 16 of lens) out.
//   light_emit_kernel       one path per lane; the pick is a fixed-length, branch-free lower-bound walk over the running sums of
//                           the light table's records (count_le of tor_env.hip, strided by the record), bit_length(n_lights)
//                           probes, so emission is logarithmic in the light count; the picked record is then read per lane.
//                           Streaming: 32 + 32 of state, 56 of ray, 24 of normal, 4 of light, 16 of densities, plus the table.
//
// Lanes without work return before the first load.  No LDS, no scratch.  Float64, unfused (-ffp-contract=off), correctly rounded
// `/` and sqrt.  Stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/tor_camera.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"

static_assert(sizeof(TorPoint) == 32 && sizeof(TorRay) == 56 && sizeof(TorRng) == 32, "TorPoint / TorRay / TorRng as the kernels index them");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");
static_assert(sizeof(TorCamera) == sizeof(tor::Camera), "TorCamera mirrors tor::Camera");

namespace tor {
namespace {

constexpr int kCamQThreads = 256;
constexpr int kLightWords = 16;                      // float64 per light record (tor_lights.hip)
constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 2.0 * 3.141592653589793;   // sampling.nim:52: Nim's 2 * PI

struct CCParams {
  Camera cam;
  double fd, HH, VV, K;      // tor_camera.h "per camera and frame"
  double fcols, frows;       // (double)ncols, (double)nrows
  int nrows, ncols;
  const double* points;      // 4 float64 per point (TorPoint)
  unsigned long long* rng;   // 4 u64 per point (TorRng), read and written
  const int* list;           // the points to answer, or null: entry e is point e
  long long n_list, n_points;
  double* rays;              // 7 float64 per point (TorRay)
  int* pixel;                // one int32 per point: row * ncols + col, -1 for none
  double* factor;            // one float64 per point
  double* lens;              // 2 float64 per point, or null
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(kCamQThreads) void camera_connect_kernel(const CCParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_points, (long long)blockIdx.x * kCamQThreads + threadIdx.x);
  if (i < 0) return;
  const double* pt = P.points + 4 * i;
  const double yx = pt[0], yy = pt[1], yz = pt[2], time = pt[3];
  unsigned long long* s = P.rng + 4 * i;
  Rng g{s[0], s[1], s[2], s[3]};
  // exactly two draws, whatever follows
  const double u0 = uniform01(g), u1 = uniform01(g);
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
  const Camera& c = P.cam;
  // the lens point
  const double r = __builtin_sqrt(u0);
  double sn, cs;
  sincos_2pi(u1 * kTwoPi, sn, cs);
  const double lr = c.lens_radius * r;
  const double rdx = lr * cs, rdy = lr * sn;
  const double xx = c.origin.x + c.u.x * rdx + c.v.x * rdy;
  const double xy = c.origin.y + c.u.y * rdx + c.v.y * rdy;
  const double xz = c.origin.z + c.u.z * rdx + c.v.z * rdy;
  // the geometry
  const double ex = yx - xx, ey = yy - xy, ez = yz - xz;
  const double z = -dot3(ex, ey, ez, c.w.x, c.w.y, c.w.z);
  const double k = P.fd / z;
  const double qx = (xx + ex * k) - c.lower_left_corner.x;
  const double qy = (xy + ey * k) - c.lower_left_corner.y;
  const double qz = (xz + ez * k) - c.lower_left_corner.z;
  const double sc = dot3(qx, qy, qz, c.horizontal.x, c.horizontal.y, c.horizontal.z) / P.HH;
  const double tc = dot3(qx, qy, qz, c.vertical.x, c.vertical.y, c.vertical.z) / P.VV;
  const double a = sc * (P.fcols - 1.0), b = tc * (P.frows - 1.0);   // ((double)(ncols - 1) exactly: ncols < 2^31)
  const double len = __builtin_sqrt(dot3(ex, ey, ez, ex, ey, ez));
  const double z3 = z * z * z;
  const double f = P.K * len / z3;
  const bool valid = (z > 0.0) && (a >= 0.0) && (a < P.fcols) && (b >= 0.0) && (b < P.frows) && (z3 < __builtin_inf()) && (f >= 0.0) &&
                     (f < __builtin_inf());
  double* o = P.rays + 7 * i;
  if (P.lens) {
    P.lens[2 * i] = rdx;
    P.lens[2 * i + 1] = rdy;
  }
  if (!valid) {
    for (int q = 0; q < 7; ++q) o[q] = 0.0;
    P.pixel[i] = -1;
    P.factor[i] = 0.0;
    return;
  }
  const int col = (int)__builtin_floor(a), row = (int)__builtin_floor(b);   // in [0, ncols) and [0, nrows): checked above
  o[0] = yx; o[1] = yy; o[2] = yz;
  o[3] = xx - yx; o[4] = xy - yy; o[5] = xz - yz;
  o[6] = time;
  P.pixel[i] = row * P.ncols + col;
  P.factor[i] = f;
}

struct LEParams {
  const double* lights;      // n_lights records of kLightWords float64 (tor_lights.hip)
  int n_lights, steps;       // steps = bit_length(n_lights): the walk's probes
  int last_pos;              // the last light of weight > 0: the walk's fallback
  double total;              // T: the last light's running sum
  double time_lo, time_hi;
  unsigned long long* rng;   // 4 u64 per path (TorRng), read and written
  const int* list;           // the paths to start, or null: entry e is path e
  long long n_list, n_paths;
  double* rays;              // 7 float64 per path (TorRay)
  double* normal;            // 3 float64 per path
  int* light;                // one int32 per path: the picked light's OBJECT index
  double* pdf;               // 2 float64 per path: per unit area (the pick included), per unit solid angle
};

// How many of the non-decreasing running sums run[0 .. m) (word 12 of each record) are <= x, m >= 1: the first index whose sum is
// > x, or m if none.  `steps` >= bit_length(m) halving steps, branch-free; the index of every load is clamped into [0, m).
__device__ __forceinline__ int count_le_runs(const double* recs, int m, int steps, double x) {
  int pos = 0;
  for (int s = steps - 1; s >= 0; --s) {
    const int probe = pos + (1 << s);
    const int at = (probe < m ? probe : m) - 1;
    const double v = recs[(size_t)at * kLightWords + 12];
    pos = (probe <= m && v <= x) ? probe : pos;
  }
  return pos;
}

__global__ __launch_bounds__(kCamQThreads) void light_emit_kernel(const LEParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_paths, (long long)blockIdx.x * kCamQThreads + threadIdx.x);
  if (i < 0) return;
  unsigned long long* s = P.rng + 4 * i;
  Rng g{s[0], s[1], s[2], s[3]};
  // exactly six draws, in this order
  const double time = uniform_range(g, P.time_lo, P.time_hi);
  const double u0 = uniform01(g), u1 = uniform01(g), u2 = uniform01(g), u3 = uniform01(g), u4 = uniform01(g);
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
  // the pick: the first light whose running sum is > x, else the last of positive weight
  const double x = u0 * P.total;
  int j = count_le_runs(P.lights, P.n_lights, P.steps, x);
  if (j >= P.n_lights) j = P.last_pos;   // (last_pos < n_lights: the host found it in the table)
  const double* r = P.lights + (size_t)j * kLightWords;
  const double Pj = r[11] / P.total;
  // the position: the centre at the drawn time (light_geom's operations, moving_spheres.nim:39-44)
  double cx = r[0], cy = r[1], cz = r[2];
  if (r[8] != 0.0) {
    const double fr = (time - r[6]) / r[7];
    cx = cx + r[3] * fr; cy = cy + r[4] * fr; cz = cz + r[5] * fr;
  }
  const double R = r[9], R2 = r[10];
  const double zc = 1.0 - 2.0 * u1;
  const double rr = __builtin_sqrt(4.0 * u1 * (1.0 - u1));
  double sn, cs;
  sincos_2pi(u2 * kTwoPi, sn, cs);
  const double nx = rr * cs, ny = rr * sn, nz = zc;
  // the direction: cosine-weighted about n, in the branchless frame of tor_lights.h
  const double sin_t = __builtin_sqrt(u3), cos_t = __builtin_sqrt(1.0 - u3);
  double s4, c4;
  sincos_2pi(u4 * kTwoPi, s4, c4);
  const double sg = __builtin_copysign(1.0, nz);
  const double aa = -1.0 / (sg + nz);
  const double bb = nx * ny * aa;
  const double b1x = 1.0 + sg * nx * nx * aa, b1y = sg * bb, b1z = -sg * nx;
  const double b2x = bb, b2y = sg + ny * ny * aa, b2z = -ny;
  const double e1 = sin_t * c4, e2 = sin_t * s4;
  double* o = P.rays + 7 * i;
  o[0] = cx + nx * R; o[1] = cy + ny * R; o[2] = cz + nz * R;
  o[3] = b1x * e1 + b2x * e2 + nx * cos_t;
  o[4] = b1y * e1 + b2y * e2 + ny * cos_t;
  o[5] = b1z * e1 + b2z * e2 + nz * cos_t;
  o[6] = time;
  double* nn = P.normal + 3 * i;
  nn[0] = nx; nn[1] = ny; nn[2] = nz;
  P.light[i] = (int)__double_as_longlong(r[13]);
  P.pdf[2 * i] = Pj / ((4.0 * kPi) * R2);
  P.pdf[2 * i + 1] = cos_t / kPi;
}

}  // namespace
}  // namespace tor

namespace {

unsigned camq_grid(int64_t n_list) { return (unsigned)((n_list + tor::kCamQThreads - 1) / tor::kCamQThreads); }

double hdot(const tor::V3& a, const tor::V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// tor_camera.h's refusals that need no device, in the documented order, and the per-camera constants
int connect_check(const char* who, TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int64_t n_points, const void* list,
                  int64_t n_list, bool nulls, tor::CCParams& P) {
  using tor::fail;
  const std::string w = who;
  if (!ctx || !cam) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx or cam is NULL");
  if (nrows < 2 || ncols < 2) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": nrows and ncols must be >= 2");
  const int rc = tor::list_args(w, ctx, n_points, list, n_list);
  if (rc != TOR_OK) return rc;
  std::memcpy(&P.cam, cam, sizeof(TorCamera));
  const tor::Camera& c = P.cam;
  const tor::V3 ol{c.origin.x - c.lower_left_corner.x, c.origin.y - c.lower_left_corner.y, c.origin.z - c.lower_left_corner.z};
  P.fd = hdot(ol, c.w);
  P.HH = hdot(c.horizontal, c.horizontal);
  P.VV = hdot(c.vertical, c.vertical);
  P.K = P.fd * P.fd * (double)(ncols - 1) * (double)(nrows - 1) / (std::sqrt(P.HH) * std::sqrt(P.VV));
  if (!(P.fd > 0.0) || !std::isfinite(P.fd) || !(P.HH > 0.0) || !std::isfinite(P.HH) || !(P.VV > 0.0) || !std::isfinite(P.VV))
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the camera's focus distance, |horizontal|^2 and |vertical|^2 must be finite and > 0");
  if (!(c.lens_radius >= 0.0) || !std::isfinite(c.lens_radius))
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the camera's lens_radius must be finite and >= 0");
  if (n_points > 0 && n_list > 0 && nulls) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL points, rng, rays, pixel or factor");
  P.nrows = nrows;
  P.ncols = ncols;
  P.fcols = (double)ncols;
  P.frows = (double)nrows;
  return TOR_OK;
}

int connect_launch(tor::CCParams& P, int64_t n_points, const void* d_points, void* d_rng, const int32_t* d_list, int64_t n_list, void* d_rays,
                   int32_t* d_pixel, double* d_factor, double* d_lens, hipStream_t stream) {
  P.points = (const double*)d_points;
  P.rng = (unsigned long long*)d_rng;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_points = (long long)n_points;
  P.rays = (double*)d_rays;
  P.pixel = d_pixel;
  P.factor = d_factor;
  P.lens = d_lens;
  hipLaunchKernelGGL(tor::camera_connect_kernel, dim3(camq_grid(n_list)), dim3(tor::kCamQThreads), 0, stream, P);
  HIP_TRY(hipGetLastError());
  tor::set_last_note(P.cam.lens_radius == 0.0 ? "camera connect: pinhole" : "camera connect: thin lens");
  return TOR_OK;
}

// tor_light_sample_device's checks with the time range where it has the strategy
int emit_check(const char* who, TorContext* ctx, int64_t n_paths, const void* list, int64_t n_list, double time_lo, double time_hi, bool nulls) {
  using tor::fail;
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_paths, list, n_list);
  if (rc != TOR_OK) return rc;
  if (!std::isfinite(time_lo) || !std::isfinite(time_hi) || time_lo > time_hi)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the time range must be finite with time_lo <= time_hi");
  if (n_paths > 0 && n_list > 0 && nulls) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rng, rays, normal, light or pdf");
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  if (ctx->hitq.n_lights <= 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no light table (tor_scene_lights)");
  return TOR_OK;
}

// the launch; the arguments are checked, n_paths > 0 and n_list > 0
int emit_launch(const char* who, TorContext* ctx, int64_t n_paths, void* d_rng, const int32_t* d_list, int64_t n_list, double time_lo,
                double time_hi, void* d_rays, double* d_normal, int32_t* d_light, double* d_pdf, hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::HitQueryState& hq = ctx->hitq;
  tor::LEParams P{};
  P.lights = (const double*)hq.lights.ptr;
  P.n_lights = (int)hq.n_lights;
  P.steps = 0;
  while ((1ll << P.steps) <= hq.n_lights) ++P.steps;
  P.last_pos = (int)hq.lights_last_pos;
  P.total = hq.lights_total;
  P.time_lo = time_lo;
  P.time_hi = time_hi;
  P.rng = (unsigned long long*)d_rng;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_paths = (long long)n_paths;
  P.rays = (double*)d_rays;
  P.normal = d_normal;
  P.light = d_light;
  P.pdf = d_pdf;
  hipLaunchKernelGGL(tor::light_emit_kernel, dim3(camq_grid(n_list)), dim3(tor::kCamQThreads), 0, stream, P);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note("light emit: by weight");
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_camera_connect_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int64_t n_points, const TorPoint* d_points,
                              TorRng* d_rng, const int32_t* d_list, int64_t n_list, TorRay* d_rays, int32_t* d_pixel, double* d_factor,
                              double* d_lens, void* hip_stream) {
  tor::CCParams P{};
  const int rc = connect_check("tor_camera_connect_device", ctx, cam, nrows, ncols, n_points, d_list, n_list,
                               !d_points || !d_rng || !d_rays || !d_pixel || !d_factor, P);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return connect_launch(P, n_points, d_points, d_rng, d_list, n_list, d_rays, d_pixel, d_factor, d_lens, (hipStream_t)hip_stream);
}

int tor_camera_connect_host(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int64_t n_points, const TorPoint* points,
                            TorRng* rng, const int32_t* list, int64_t n_list, TorRay* rays, int32_t* pixel, double* factor, double* lens) {
  tor::CCParams P{};
  int rc = connect_check("tor_camera_connect_host", ctx, cam, nrows, ncols, n_points, list, n_list, !points || !rng || !rays || !pixel || !factor,
                         P);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_points;
  tor::HostPart st[7] = {{points, n * sizeof(TorPoint), true, false},
                         {rng, n * sizeof(TorRng), true, true},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {rays, n * sizeof(TorRay), true, true},
                         {pixel, n * 4, true, true},
                         {factor, n * 8, true, true},
                         {lens, lens ? n * 16 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = connect_launch(P, n_points, st[0].dev, st[1].dev, st[2].as<const int32_t>(), n_list, st[3].dev, st[4].as<int32_t>(),
                      st[5].as<double>(), st[6].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

int tor_light_emit_device(TorContext* ctx, int64_t n_paths, TorRng* d_rng, const int32_t* d_list, int64_t n_list, double time_lo,
                          double time_hi, TorRay* d_rays, double* d_normal, int32_t* d_light, double* d_pdf, void* hip_stream) {
  const char* who = "tor_light_emit_device";
  const int rc = emit_check(who, ctx, n_paths, d_list, n_list, time_lo, time_hi, !d_rng || !d_rays || !d_normal || !d_light || !d_pdf);
  if (rc != TOR_OK || n_paths == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return emit_launch(who, ctx, n_paths, d_rng, d_list, n_list, time_lo, time_hi, d_rays, d_normal, d_light, d_pdf, (hipStream_t)hip_stream);
}

int tor_light_emit_host(TorContext* ctx, int64_t n_paths, TorRng* rng, const int32_t* list, int64_t n_list, double time_lo, double time_hi,
                        TorRay* rays, double* normal, int32_t* light, double* pdf) {
  const char* who = "tor_light_emit_host";
  int rc = emit_check(who, ctx, n_paths, list, n_list, time_lo, time_hi, !rng || !rays || !normal || !light || !pdf);
  if (rc != TOR_OK || n_paths == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_paths;
  tor::HostPart st[6] = {{rng, n * sizeof(TorRng), true, true},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {rays, n * sizeof(TorRay), true, true},
                         {normal, n * 24, true, true},
                         {light, n * 4, true, true},
                         {pdf, n * 16, true, true}};
  rc = tor::stage_in(ctx, st, 6);
  if (rc != TOR_OK) return rc;
  rc = emit_launch(who, ctx, n_paths, st[0].dev, st[1].as<const int32_t>(), n_list, time_lo, time_hi, st[2].dev, st[3].as<double>(),
                   st[4].as<int32_t>(), st[5].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 6);
}

}  // extern "C"
