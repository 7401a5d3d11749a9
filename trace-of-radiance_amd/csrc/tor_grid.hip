// tor_grid.hip -- heterogeneous media for host integrators (tor_scene_media_grid, tor_media_grid_info, tor_media_grid_march_device,
// tor_media_grid_density_device and the blocking _host twins, include/tor_grid.h): a voxel grid of densities attached to one medium
// of the media table, the optical-depth march through it by regular tracking -- an exact 3-D DDA walk through the piecewise-constant
// density -- and the density lookup at a point, on gfx950.  include/tor_grid.h holds the definition, operation by operation; this
// file follows it line by line (sphere_of, the clip, the entry, the walk).
//
// The grid's descriptor (lo, hi, h, n, the density pointer) travels in the kernel arguments, and the medium's record (the head of
// tor_media.hip) is read at a wave-uniform address through the scalar-load view: both stay in scalar registers.  The density load is
// the only per-lane gather.
//
//   media_grid_march_kernel    one listed ray per lane.  The walk is the header's counted loop; the three axes are kept in named
//                              registers and chosen by compares, never by a computed index into an array, so nothing spills to
//                              scratch.  A lane that is done keeps its answer in registers and takes no further part -- it loads no
//                              density --; the loop leaves when the whole wave is done (a ballot: a wave-uniform exit).  No lane
//                              waits for another, and a wrong compare shows as a wrong answer, never as a hang or a fault: the
//                              trip count is bounded by nx + ny + nz, and the load's index is clamped at entry and checked at every
//                              move (the header's two arguments).
//   media_grid_density_kernel  one listed point per lane: the lookup.
// No LDS, no atomics.  Float64, unfused (-ffp-contract=off), correctly rounded `/` and sqrt.  Stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tor_grid.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"

static_assert(sizeof(TorRay) == 56, "TorRay as the kernels index it");
static_assert(TOR_MEDIA_MAX == 64, "the active set is one 64-bit word");
static_assert(TOR_GRID_MAX_CELLS <= INT_MAX && 3 * TOR_GRID_MAX_DIM <= INT_MAX, "a cell index and the loop's bound are ints");

namespace tor {
namespace {

constexpr int kGridThreads = 256;
constexpr int kMediaWords = 16;  // float64 per medium record (tor_media.hip packs it)
constexpr int kSigmaWord = 10;

struct GdParams {
  const double* record;         // the record of the grid's medium: kMediaWords float64
  const double* density;        // nx * ny * nz float64, C order
  double lo[3], hi[3], h[3];    // the box, as offsets from the medium's centre, and the cell size
  int n[3];
  int medium;
  const double* rays;           // the march: 7 float64 per ray (TorRay)
  const double* t_range;        // 2 float64 per ray, or null: (0.0, +inf)
  const double* tau;            // one budget per ray
  const double* points;         // the lookup: 4 float64 per point (p, time)
  const int* list;              // the rays / points to answer, or null: entry e is item e
  long long n_list, n_items;
  int* status;                  // the march's outputs, one per ray
  double* t;
  double* depth;
  unsigned long long* active;
  double* rho;                  // ... or null
  int* cell;                    // ... or null (the lookup: not null)
  double* out_density;          // the lookup's second output
};

// tor_grid.h "sphere" up to oc: the centre of the record at `time`, as tor_media.hip's medium_roots computes it
template <typename R>
__device__ __forceinline__ void centre_of(R r, double time, double& cx, double& cy, double& cz) {
  cx = r[0]; cy = r[1]; cz = r[2];
  if (r[8] != 0.0) {
    const double f = (time - r[6]) / r[7];
    cx = cx + r[3] * f; cy = cy + r[4] * f; cz = cz + r[5] * f;
  }
}

// the entry rule's clamped floor: the index of coordinate q (an offset from the centre) along an axis; in [0, n - 1] whatever q holds
__device__ __forceinline__ int cell_index(double q, double lo, double h, int n) {
  double f = __builtin_floor((q - lo) / h);
  if (!(f >= 0.0)) f = 0.0;
  if (f > (double)(n - 1)) f = (double)(n - 1);
  return (int)f;
}

// the parameter of the plane a ray leaves cell i through along an axis: from the index each time, never accumulated
__device__ __forceinline__ double plane_t(int i, int dir, double lo, double h, double oc, double d) {
  return ((lo + (double)(i + (dir > 0 ? 1 : 0)) * h) - oc) / d;
}

// the clip of one axis: false when the ray is parallel to the slab and outside it
__device__ __forceinline__ bool clip_axis(double oc, double d, double lo, double hi, double& t0, double& t1) {
  if (d == 0.0) return oc >= lo && oc < hi;
  const double ta = (lo - oc) / d, tb = (hi - oc) / d;
  const double near = d > 0.0 ? ta : tb, far = d > 0.0 ? tb : ta;
  if (near > t0) t0 = near;
  if (far < t1) t1 = far;
  return true;
}

__global__ __launch_bounds__(kGridThreads) void media_grid_march_kernel(const GdParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_items, (long long)blockIdx.x * kGridThreads + threadIdx.x);
  const bool live = i >= 0;
  double ox = 0.0, oy = 0.0, oz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, time = 0.0, t_min = 0.0, t_max = 0.0, tau = 0.0;
  if (live) {
    const double* s = P.rays + 7 * i;
    ox = s[0]; oy = s[1]; oz = s[2];
    dx = s[3]; dy = s[4]; dz = s[5];
    time = s[6];
    t_min = P.t_range ? P.t_range[2 * i] : 0.0;
    t_max = P.t_range ? P.t_range[2 * i + 1] : __builtin_inf();
    tau = P.tau[i];
  }
  const double a = dx * dx + dy * dy + dz * dz;
  const double len = __builtin_sqrt(a);
  const bool refused = !(tau >= 0.0) || !(t_min < t_max);
  // sphere: medium_roots' operations (tor_media.hip), keeping oc
  const qcdptr r = (qcdptr)(uintptr_t)P.record;
  double cx, cy, cz;
  centre_of(r, time, cx, cy, cz);
  const double ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
  const double hb = ocx * dx + ocy * dy + ocz * dz;
  const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r[9];
  const double disc = hb * hb - a * cc;
  bool has = false;
  double s0 = 0.0, s1 = 0.0;
  if (disc > 0.0) {
    const double root = __builtin_sqrt(disc);
    s0 = (-hb - root) / a;
    s1 = (-hb + root) / a;
    has = true;
  }
  const double sigma = r[kSigmaWord];
  const double lox = P.lo[0], loy = P.lo[1], loz = P.lo[2], hx = P.h[0], hy = P.h[1], hz = P.h[2];
  const int nx = P.n[0], ny = P.n[1], nz = P.n[2];
  // clip
  double t0 = t_min, t1 = t_max;
  if (s0 > t0) t0 = s0;
  if (s1 < t1) t1 = s1;
  bool empty = !has;
  if (!clip_axis(ocx, dx, lox, P.hi[0], t0, t1)) empty = true;
  if (!clip_axis(ocy, dy, loy, P.hi[1], t0, t1)) empty = true;
  if (!clip_axis(ocz, dz, loz, P.hi[2], t0, t1)) empty = true;
  if (!(t0 < t1)) empty = true;
  // entry (every lane: the clamp holds the indices in range whatever t0 is)
  int ix = cell_index(ocx + t0 * dx, lox, hx, nx), iy = cell_index(ocy + t0 * dy, loy, hy, ny), iz = cell_index(ocz + t0 * dz, loz, hz, nz);
  const int dirx = dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0), diry = dy > 0.0 ? 1 : (dy < 0.0 ? -1 : 0), dirz = dz > 0.0 ? 1 : (dz < 0.0 ? -1 : 0);
  const double inf = __builtin_inf();
  double tkx = dirx == 0 ? inf : plane_t(ix, dirx, lox, hx, ocx, dx);
  double tky = diry == 0 ? inf : plane_t(iy, diry, loy, hy, ocy, dy);
  double tkz = dirz == 0 ? inf : plane_t(iz, dirz, loz, hz, ocz, dz);
  // the answer of a ray that is refused, and of one that meets nothing
  bool done = !live || refused || empty;
  int status = refused ? -1 : 0, out_cell = -1;
  double out_t = refused ? t_min : t_max, out_depth = 0.0, out_rho = 0.0;
  unsigned long long out_active = 0ull;
  double t = t0, D = 0.0;
  const qgdptr dens = (qgdptr)(uintptr_t)P.density;
  const int bound = nx + ny + nz;
  for (int it = 0; it < bound; ++it) {
    if (__ballot(!done) == 0ull) break;
    int ks = 0;
    double tn = tkx;
    if (tky < tn) { ks = 1; tn = tky; }
    if (tkz < tn) { ks = 2; tn = tkz; }
    const bool last = !(tn < t1);
    if (last) tn = t1;
    if (tn < t) tn = t;  // the guard
    const int cell = (ix * ny + iy) * nz + iz;  // in [0, nx * ny * nz): clamped at entry, checked at every move
    if (!done) {
      const double rho = sigma * dens[cell];
      const double step = rho > 0.0 ? rho * ((tn - t) * len) : 0.0;
      const double rem = tau - D;
      if (rho > 0.0 && rem < step) {
        double t_c = t + (rem / rho) / len;
        if (tn < t_c) t_c = tn;
        status = 1; out_t = t_c; out_depth = tau; out_active = 1ull << P.medium; out_rho = rho; out_cell = cell;
        done = true;
      } else {
        D = D + step;
        out_depth = D;
        if (last) {
          done = true;
        } else if (ks == 0) {
          ix += dirx;
          if (ix < 0 || ix >= nx) { done = true; ix -= dirx; }
          else tkx = plane_t(ix, dirx, lox, hx, ocx, dx);
        } else if (ks == 1) {
          iy += diry;
          if (iy < 0 || iy >= ny) { done = true; iy -= diry; }
          else tky = plane_t(iy, diry, loy, hy, ocy, dy);
        } else {
          iz += dirz;
          if (iz < 0 || iz >= nz) { done = true; iz -= dirz; }
          else tkz = plane_t(iz, dirz, loz, hz, ocz, dz);
        }
        t = tn;
      }
    }
  }
  if (!live) return;
  P.status[i] = status;
  P.t[i] = out_t;
  P.depth[i] = out_depth;
  P.active[i] = out_active;
  if (P.rho) P.rho[i] = out_rho;
  if (P.cell) P.cell[i] = out_cell;
}

__global__ __launch_bounds__(kGridThreads) void media_grid_density_kernel(const GdParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n_items, (long long)blockIdx.x * kGridThreads + threadIdx.x);
  if (i < 0) return;
  const double* s = P.points + 4 * i;
  const qcdptr r = (qcdptr)(uintptr_t)P.record;
  double cx, cy, cz;
  centre_of(r, s[3], cx, cy, cz);
  const double qx = s[0] - cx, qy = s[1] - cy, qz = s[2] - cz;
  const bool in_sphere = (qx * qx + qy * qy + qz * qz) - r[9] < 0.0;
  const bool in_box = qx >= P.lo[0] && qx < P.hi[0] && qy >= P.lo[1] && qy < P.hi[1] && qz >= P.lo[2] && qz < P.hi[2];
  int cell = -1;
  double value = 0.0;
  if (in_sphere && in_box) {
    const int ix = cell_index(qx, P.lo[0], P.h[0], P.n[0]), iy = cell_index(qy, P.lo[1], P.h[1], P.n[1]),
              iz = cell_index(qz, P.lo[2], P.h[2], P.n[2]);
    cell = (ix * P.n[1] + iy) * P.n[2] + iz;  // in range: every index is clamped
    value = P.density[cell];
  }
  P.cell[i] = cell;
  P.out_density[i] = value;
}

}  // namespace
}  // namespace tor

namespace {

std::string dims_of(const tor::MediaGrid& g) {
  return std::to_string(g.n[0]) + "x" + std::to_string(g.n[1]) + "x" + std::to_string(g.n[2]);
}

// tor_media_march_device's checks (the list, the NULL arrays, the scene, the table), then the medium and its grid
int grid_check(const char* who, TorContext* ctx, int64_t n_items, const void* list, int64_t n_list, bool nulls, const char* names,
               int32_t medium) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_items, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_items > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL " + names);
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  const tor::HitQueryState& hq = ctx->hitq;
  if (hq.n_media <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no media table (tor_scene_media)");
  if (medium < 0 || medium >= hq.n_media)
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": medium " + std::to_string(medium) + " is outside the media table (" + std::to_string(hq.n_media) + ")");
  if (hq.grids[medium].n[0] <= 0)
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": medium " + std::to_string(medium) + " has no density grid (tor_scene_media_grid)");
  return TOR_OK;
}

// the launches; the arguments are checked, n_items > 0 and n_list > 0
int grid_launch(const char* who, TorContext* ctx, bool lookup, tor::GdParams& P, int32_t medium, int64_t n_items, const int32_t* d_list,
                int64_t n_list, hipStream_t stream) {
  const int rc = tor::query_stream_rule(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  const tor::MediaGrid& g = ctx->hitq.grids[medium];
  P.record = (const double*)ctx->hitq.media.ptr + (size_t)tor::kMediaWords * (size_t)medium;
  P.density = (const double*)g.density.ptr;
  for (int k = 0; k < 3; ++k) {
    P.lo[k] = g.lo[k]; P.hi[k] = g.hi[k]; P.h[k] = g.h[k];
    P.n[k] = g.n[k];
  }
  P.medium = medium;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_items = (long long)n_items;
  const dim3 grid((unsigned)((n_list + tor::kGridThreads - 1) / tor::kGridThreads)), block(tor::kGridThreads);
  if (lookup) hipLaunchKernelGGL(tor::media_grid_density_kernel, grid, block, 0, stream, P);
  else hipLaunchKernelGGL(tor::media_grid_march_kernel, grid, block, 0, stream, P);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note(std::string(lookup ? "media grid density: medium " : "media grid march: medium ") + std::to_string(medium) + ", " + dims_of(g));
  return TOR_OK;
}

int march_launch(const char* who, TorContext* ctx, int64_t n_rays, const void* d_rays, const double* d_t_range, const double* d_tau,
                 int32_t medium, const int32_t* d_list, int64_t n_list, int32_t* d_status, double* d_t, double* d_depth, uint64_t* d_active,
                 double* d_rho, int32_t* d_cell, hipStream_t stream) {
  tor::GdParams P{};
  P.rays = (const double*)d_rays;
  P.t_range = d_t_range;
  P.tau = d_tau;
  P.status = d_status;
  P.t = d_t;
  P.depth = d_depth;
  P.active = (unsigned long long*)d_active;
  P.rho = d_rho;
  P.cell = d_cell;
  return grid_launch(who, ctx, false, P, medium, n_rays, d_list, n_list, stream);
}

int density_launch(const char* who, TorContext* ctx, int64_t n_points, const double* d_points, int32_t medium, const int32_t* d_list,
                   int64_t n_list, int32_t* d_cell, double* d_density, hipStream_t stream) {
  tor::GdParams P{};
  P.points = d_points;
  P.cell = d_cell;
  P.out_density = d_density;
  return grid_launch(who, ctx, true, P, medium, n_points, d_list, n_list, stream);
}

}  // namespace

extern "C" {

int tor_scene_media_grid(TorContext* ctx, int32_t medium, int32_t nx, int32_t ny, int32_t nz, const double* box, const double* density) {
  using tor::fail;
  const std::string w = "tor_scene_media_grid";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  tor::HitQueryState& hq = ctx->hitq;
  if (hq.n_media <= 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no media table (tor_scene_media)");
  if (medium < 0 || medium >= hq.n_media)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": medium " + std::to_string(medium) + " is outside the media table (" + std::to_string(hq.n_media) + ")");
  const bool remove = nx == 0 && ny == 0 && nz == 0;
  size_t cells = 0;
  double lo[3], hi[3];
  if (!remove) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > TOR_GRID_MAX_DIM || ny > TOR_GRID_MAX_DIM || nz > TOR_GRID_MAX_DIM)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": every dimension must be in 1 .. TOR_GRID_MAX_DIM (" + std::to_string(TOR_GRID_MAX_DIM) + ")");
    cells = (size_t)nx * (size_t)ny * (size_t)nz;
    if (cells > (size_t)TOR_GRID_MAX_CELLS)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": more cells than TOR_GRID_MAX_CELLS (" + std::to_string(TOR_GRID_MAX_CELLS) + ")");
    if (!density) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": density is NULL");
    for (int k = 0; box && k < 3; ++k) {
      lo[k] = box[k];
      hi[k] = box[3 + k];
      if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(lo[k] < hi[k]))
        return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the box must be finite with lo < hi on every axis");
    }
    for (size_t c = 0; c < cells; ++c)
      if (!std::isfinite(density[c]) || density[c] < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": density must be finite and >= 0");
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the grid
  tor::MediaGrid& g = hq.grids[medium];
  if (remove) {
    g.density.release();
    g.n[0] = g.n[1] = g.n[2] = 0;
    hq.grid_mask &= ~(1ull << medium);
    return TOR_OK;
  }
  if (!box) {  // the sphere's bounding cube, from the record's radius * radius
    double r2 = 0.0;
    HIP_TRY(hipMemcpy(&r2, (const double*)hq.media.ptr + (size_t)tor::kMediaWords * (size_t)medium + 9, 8, hipMemcpyDeviceToHost));
    const double R = std::sqrt(r2);
    if (!std::isfinite(R) || !(R > 0.0)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the box must be finite with lo < hi on every axis");
    for (int k = 0; k < 3; ++k) { lo[k] = -R; hi[k] = R; }
  }
  tor::DeviceBuffer fresh;  // (so that a failed allocation or copy leaves the medium's old grid as it was)
  HIP_TRY(fresh.ensure(cells * 8));
  const hipError_t e = hipMemcpy(fresh.ptr, density, cells * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    fresh.release();
    return tor::fail_hip(e, "hipMemcpy(density)");
  }
  g.density.release();
  g.density = fresh;
  const int32_t n[3] = {nx, ny, nz};
  for (int k = 0; k < 3; ++k) {
    g.n[k] = n[k];
    g.lo[k] = lo[k];
    g.hi[k] = hi[k];
    g.h[k] = (hi[k] - lo[k]) / (double)n[k];
  }
  hq.grid_mask |= 1ull << medium;
  return TOR_OK;
}

int tor_media_grid_info(TorContext* ctx, int32_t medium, int32_t* dims, double* box, uint64_t* grid_mask) {
  using tor::fail;
  const std::string w = "tor_media_grid_info";
  if (!ctx || !dims) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx or dims is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  const tor::HitQueryState& hq = ctx->hitq;
  if (hq.n_media <= 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no media table (tor_scene_media)");
  if (medium < 0 || medium >= hq.n_media)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": medium " + std::to_string(medium) + " is outside the media table (" + std::to_string(hq.n_media) + ")");
  const tor::MediaGrid& g = hq.grids[medium];
  for (int k = 0; k < 3; ++k) dims[k] = g.n[k];
  if (box && g.n[0] > 0)
    for (int k = 0; k < 3; ++k) { box[k] = g.lo[k]; box[3 + k] = g.hi[k]; }
  if (grid_mask) *grid_mask = hq.grid_mask;
  return TOR_OK;
}

int tor_media_grid_march_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const double* d_tau,
                                int32_t medium, const int32_t* d_list, int64_t n_list, int32_t* d_status, double* d_t, double* d_depth,
                                uint64_t* d_active, double* d_rho, int32_t* d_cell, void* hip_stream) {
  const char* who = "tor_media_grid_march_device";
  const int rc = grid_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_tau || !d_status || !d_t || !d_depth || !d_active,
                            "rays, tau, status, t, depth or active", medium);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return march_launch(who, ctx, n_rays, d_rays, d_t_range, d_tau, medium, d_list, n_list, d_status, d_t, d_depth, d_active, d_rho, d_cell,
                      (hipStream_t)hip_stream);
}

int tor_media_grid_march_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const double* tau, int32_t medium,
                              const int32_t* list, int64_t n_list, int32_t* status, double* t, double* depth, uint64_t* active, double* rho,
                              int32_t* cell) {
  const char* who = "tor_media_grid_march_host";
  int rc = grid_check(who, ctx, n_rays, list, n_list, !rays || !tau || !status || !t || !depth || !active,
                      "rays, tau, status, t, depth or active", medium);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too: rays that are not listed keep what the caller holds --, the query on the default stream, the
  // outputs back
  const size_t n = (size_t)n_rays;
  tor::HostPart st[10] = {{rays, n * sizeof(TorRay), true, false},
                          {t_range, t_range ? n * 16 : 0, true, false},
                          {tau, n * 8, true, false},
                          {list, list ? (size_t)n_list * 4 : 0, true, false},
                          {status, n * 4, true, true},
                          {t, n * 8, true, true},
                          {depth, n * 8, true, true},
                          {active, n * 8, true, true},
                          {rho, rho ? n * 8 : 0, true, true},
                          {cell, cell ? n * 4 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 10);
  if (rc != TOR_OK) return rc;
  rc = march_launch(who, ctx, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const double>(), medium, st[3].as<const int32_t>(),
                    n_list, st[4].as<int32_t>(), st[5].as<double>(), st[6].as<double>(), st[7].as<uint64_t>(), st[8].as<double>(),
                    st[9].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 10);
}

int tor_media_grid_density_device(TorContext* ctx, int64_t n_points, const double* d_points, int32_t medium, const int32_t* d_list,
                                  int64_t n_list, int32_t* d_cell, double* d_density, void* hip_stream) {
  const char* who = "tor_media_grid_density_device";
  const int rc = grid_check(who, ctx, n_points, d_list, n_list, !d_points || !d_cell || !d_density, "points, cell or density", medium);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return density_launch(who, ctx, n_points, d_points, medium, d_list, n_list, d_cell, d_density, (hipStream_t)hip_stream);
}

int tor_media_grid_density_host(TorContext* ctx, int64_t n_points, const double* points, int32_t medium, const int32_t* list, int64_t n_list,
                                int32_t* cell, double* density) {
  const char* who = "tor_media_grid_density_host";
  int rc = grid_check(who, ctx, n_points, list, n_list, !points || !cell || !density, "points, cell or density", medium);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)n_points;
  tor::HostPart st[4] = {{points, n * 32, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {cell, n * 4, true, true},
                         {density, n * 8, true, true}};
  rc = tor::stage_in(ctx, st, 4);
  if (rc != TOR_OK) return rc;
  rc = density_launch(who, ctx, n_points, st[0].as<const double>(), medium, st[1].as<const int32_t>(), n_list, st[2].as<int32_t>(),
                      st[3].as<double>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 4);
}

}  // extern "C"
