// tor_photons.hip -- the photon-map queries for host integrators (tor_photons_build_device, tor_photons_gather_device, their blocking
// _host twins and tor_photons_info, include/tor_photons.h): light-path vertices stored as photons in a context-owned hashed uniform
// grid, and per query point the exact sum of the powers of the photons within a radius, on gfx950.  include/tor_photons.h holds the
// definition -- brute force over the stored photons, operation by operation -- and the proof that the 27 neighbouring cells hold every
// accepted photon; the kernels follow it line by line.
//
// The build is a counting sort of the listed photons by bucket, every stage bounded by the list's length or the bucket count:
//   photon_classify_kernel   one lane per list entry: validity, cell, bucket -> key[e] (kNoKey: skipped or dropped); the dropped
//                            photons counted with one atomic per wave
//   photon_histogram_kernel  one lane per list entry: a 32-bit atomic per valid photon into its bucket's counter
//   the exclusive scan       photon_tile_sums_kernel (a tile of 2048 counters per workgroup: its sum, and the largest counter for
//                            tor_photons_info), photon_scan_top_kernel (one workgroup scans the <= 2^15 tile sums),
//                            photon_scan_apply_kernel (each tile scanned again from its offset -> start[], the counters zeroed: they
//                            become the scatter's cursors; the last tile writes start[n_buckets] = the stored count)
//   photon_scatter_kernel    one lane per list entry: slot = start[bucket] + atomicAdd(cursor[bucket], 1); the record -- position,
//                            power, direction (9 float64) and the exact int32 cell (16 bytes, apart: the walk reads it first) --
//                            stored at the slot.  The order inside a bucket is the atomics'; no answer depends on it.
// The gather, photon_gather_kernel, is one query per lane: for each of the (at most) 27 cells it walks the cell's bucket from
// start[b] to start[b + 1] and takes only records whose stored cell equals the cell asked for, so two neighbour cells that share a
// bucket are not counted twice and strangers are ignored.  Every loop bound is a count read from the map (clipped to the records'
// capacity); no lane waits for another, there is no LDS and no cross-lane step: a wrong hash would show as a wrong answer, never
// as a hang.  The sums are float64 additions of non-negative multiples of 2^-36, exact within the header's bound.
//
// Float64, unfused (-ffp-contract=off), correctly rounded `/`.  Stores are ordinary vector stores and vector atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tor_photons.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"

namespace tor {
namespace {

constexpr int kPhThreads = 256;
constexpr int kPhTile = 2048;              // counters per workgroup of the scan: 8 per thread
constexpr int kPhTopThreads = 1024;
constexpr unsigned kNoKey = 0xffffffffu;   // key of a list entry that stores nothing
constexpr double kCellMax = 1073741824.0;  // 2^30: |cell| <= kCellMax is in range
constexpr double kQueryMax = 1073741827.0; // 2^30 + 3: a query quotient at or beyond it accepts nothing (tor_photons.h, step 5)
constexpr int64_t kMaxPhotons = (int64_t)1 << 30;

struct BParams {
  const double* pos;    // 3 float64 per photon
  const double* pow;    // 3 float64 per photon
  const double* dir;    // 3 float64 per photon, or null
  const int* list;      // the photons to store, or null: entry e is photon e
  long long n_list, n;
  double h;             // the cell size
  unsigned mask;        // n_buckets - 1
  long long n_buckets;
  unsigned* key;        // per list entry: its bucket, or kNoKey
  unsigned* cnt;        // per bucket: the histogram, then the scatter's cursor
  unsigned* tile;       // per tile of kPhTile buckets: its sum, then its exclusive prefix
  long long n_tiles;
  unsigned* start;      // n_buckets + 1
  unsigned long long* info;  // {stored, dropped, n_buckets, largest bucket}
  int4* cell;           // per slot
  double* rec;          // 9 float64 per slot
};

__device__ __forceinline__ bool is_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

__device__ __forceinline__ unsigned bucket_of(int cx, int cy, int cz, unsigned mask) {
  return (((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u) ^ ((unsigned)cz * 83492791u)) & mask;
}

// tor_photons.h "VALID": the photon's cell, or false
__device__ __forceinline__ bool photon_cell(const BParams& P, long long i, int& cx, int& cy, int& cz) {
  const double* p = P.pos + 3 * i;
  const double* w = P.pow + 3 * i;
  const double px = p[0], py = p[1], pz = p[2];
  const double wx = w[0], wy = w[1], wz = w[2];
  bool ok = is_finite(px) && is_finite(py) && is_finite(pz);
  // NaN fails w >= 0; -0.0 passes it; +inf is caught on its own
  ok = ok && (wx >= 0.0) && (wy >= 0.0) && (wz >= 0.0) && (wx < __builtin_inf()) && (wy < __builtin_inf()) && (wz < __builtin_inf());
  if (P.dir) {
    const double* d = P.dir + 3 * i;
    ok = ok && is_finite(d[0]) && is_finite(d[1]) && is_finite(d[2]);
  }
  const double fx = __builtin_floor(px / P.h), fy = __builtin_floor(py / P.h), fz = __builtin_floor(pz / P.h);
  ok = ok && (fx >= -kCellMax) && (fx <= kCellMax) && (fy >= -kCellMax) && (fy <= kCellMax) && (fz >= -kCellMax) && (fz <= kCellMax);
  if (!ok) return false;
  cx = (int)fx; cy = (int)fy; cz = (int)fz;  // |f| <= 2^30: exact
  return true;
}

__global__ __launch_bounds__(kPhThreads) void photon_classify_kernel(const BParams P) {
  const long long e = (long long)blockIdx.x * kPhThreads + threadIdx.x;
  const long long i = listed_ray(P.list, P.n_list, P.n, e);
  bool dropped = false;
  if (i >= 0) {
    int cx, cy, cz;
    const bool ok = photon_cell(P, i, cx, cy, cz);
    dropped = !ok;
    P.key[e] = ok ? bucket_of(cx, cy, cz, P.mask) : kNoKey;
  } else if (e < P.n_list) {
    P.key[e] = kNoKey;  // a listed entry outside [0, n): skipped, not counted
  }
  const unsigned long long m = __ballot(dropped);
  if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(P.info + 1, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kPhThreads) void photon_histogram_kernel(const BParams P) {
  const long long e = (long long)blockIdx.x * kPhThreads + threadIdx.x;
  if (e >= P.n_list) return;
  const unsigned k = P.key[e];
  if (k != kNoKey) atomicAdd(P.cnt + k, 1u);
}

// sum and maximum of a tile of counters
__global__ __launch_bounds__(kPhThreads) void photon_tile_sums_kernel(const BParams P) {
  __shared__ unsigned s_sum[kPhThreads], s_max[kPhThreads];
  const long long base = (long long)blockIdx.x * kPhTile;
  unsigned sum = 0, mx = 0;
#pragma unroll
  for (int k = 0; k < kPhTile / kPhThreads; ++k) {
    const long long b = base + k * kPhThreads + threadIdx.x;
    const unsigned c = b < P.n_buckets ? P.cnt[b] : 0u;
    sum += c;
    mx = c > mx ? c : mx;
  }
  s_sum[threadIdx.x] = sum;
  s_max[threadIdx.x] = mx;
  __syncthreads();
  for (int d = kPhThreads / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
      const unsigned o = s_max[threadIdx.x + d];
      if (o > s_max[threadIdx.x]) s_max[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    P.tile[blockIdx.x] = s_sum[0];
    if (s_max[0] != 0) atomicMax(P.info + 3, (unsigned long long)s_max[0]);
  }
}

// exclusive scan of the tile sums, in place: one workgroup, a contiguous run of tiles per thread
__global__ __launch_bounds__(kPhTopThreads) void photon_scan_top_kernel(const BParams P) {
  __shared__ unsigned s[kPhTopThreads];
  const long long per = (P.n_tiles + kPhTopThreads - 1) / kPhTopThreads;
  const long long lo = (long long)threadIdx.x * per;
  const long long hi = lo + per < P.n_tiles ? lo + per : P.n_tiles;
  unsigned sum = 0;
  for (long long t = lo; t < hi; ++t) sum += P.tile[t];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kPhTopThreads; d <<= 1) {  // inclusive, Hillis-Steele
    const unsigned add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned run = s[threadIdx.x] - sum;
  for (long long t = lo; t < hi; ++t) {
    const unsigned c = P.tile[t];
    P.tile[t] = run;
    run += c;
  }
}

// start[] of a tile from its offset; the counters become the scatter's cursors (0)
__global__ __launch_bounds__(kPhThreads) void photon_scan_apply_kernel(const BParams P) {
  __shared__ unsigned s[kPhThreads];
  constexpr int kPer = kPhTile / kPhThreads;
  const long long base = (long long)blockIdx.x * kPhTile + (long long)threadIdx.x * kPer;
  unsigned c[kPer];
  unsigned sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    c[k] = base + k < P.n_buckets ? P.cnt[base + k] : 0u;
    sum += c[k];
  }
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kPhThreads; d <<= 1) {
    const unsigned add = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  const unsigned incl = P.tile[blockIdx.x] + s[threadIdx.x];
  unsigned run = incl - sum;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    if (base + k < P.n_buckets) {
      P.start[base + k] = run;
      P.cnt[base + k] = 0u;
    }
    run += c[k];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kPhThreads - 1) {  // the last thread of the last tile holds the total
    P.start[P.n_buckets] = incl;
    P.info[0] = (unsigned long long)incl;
    P.info[2] = (unsigned long long)P.n_buckets;
  }
}

__global__ __launch_bounds__(kPhThreads) void photon_scatter_kernel(const BParams P) {
  const long long e = (long long)blockIdx.x * kPhThreads + threadIdx.x;
  if (e >= P.n_list) return;
  const unsigned k = P.key[e];
  if (k == kNoKey) return;
  const long long i = P.list ? (long long)P.list[e] : e;  // in range: the entry has a key
  int cx, cy, cz;
  if (!photon_cell(P, i, cx, cy, cz)) return;  // (it was valid when its key was made)
  const size_t slot = (size_t)P.start[k] + atomicAdd(P.cnt + k, 1u);
  if (slot >= (size_t)P.n_list) return;  // never: the buckets hold as many slots as entries have keys
  P.cell[slot] = make_int4(cx, cy, cz, 0);
  double* r = P.rec + 9 * slot;
  const double* p = P.pos + 3 * i;
  const double* w = P.pow + 3 * i;
  r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
  r[3] = w[0]; r[4] = w[1]; r[5] = w[2];
  if (P.dir) {
    const double* d = P.dir + 3 * i;
    r[6] = d[0]; r[7] = d[1]; r[8] = d[2];
  } else {
    r[6] = 0.0; r[7] = 0.0; r[8] = 0.0;
  }
}

struct GParams {
  const double* point;   // 3 float64 per point
  const double* normal;  // 3 float64 per point, or null
  const double* radius;  // one float64 per point, or null
  const int* list;       // the points to answer, or null: entry e is point e
  long long n_list, n;
  int kernel;            // TOR_PHOTON_KERNEL_*
  double max_value;
  double R, h;
  unsigned mask;         // n_buckets - 1
  unsigned cap;          // slots the record arrays hold
  const unsigned* start; // n_buckets + 1
  const int4* cell;
  const double* rec;
  double* sums;          // 3 float64 per point
  int* count;            // one int32 per point
};

__global__ __launch_bounds__(kPhThreads) void photon_gather_kernel(const GParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n, (long long)blockIdx.x * kPhThreads + threadIdx.x);
  if (i < 0) return;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int count = 0;
  double r = P.radius ? P.radius[i] : P.R;
  if (r >= 0.0) {  // (a negative or NaN radius accepts nothing)
    r = r < P.R ? r : P.R;
    const double r2 = r * r;
    const double* x = P.point + 3 * i;
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    const double q0 = x0 / P.h, q1 = x1 / P.h, q2 = x2 / P.h;
    // tor_photons.h step 5: beyond kQueryMax (NaN and infinities too) nothing can be accepted, and nothing is converted
    if ((__builtin_fabs(q0) < kQueryMax) && (__builtin_fabs(q1) < kQueryMax) && (__builtin_fabs(q2) < kQueryMax)) {
      const int kc = (int)kCellMax;
      const int c0 = (int)__builtin_floor(q0), c1 = (int)__builtin_floor(q1), c2 = (int)__builtin_floor(q2);
      const int lo0 = c0 - 1 > -kc ? c0 - 1 : -kc, hi0 = c0 + 1 < kc ? c0 + 1 : kc;
      const int lo1 = c1 - 1 > -kc ? c1 - 1 : -kc, hi1 = c1 + 1 < kc ? c1 + 1 : kc;
      const int lo2 = c2 - 1 > -kc ? c2 - 1 : -kc, hi2 = c2 + 1 < kc ? c2 + 1 : kc;
      double n0 = 0.0, n1 = 0.0, n2 = 0.0;
      if (P.normal) {
        const double* nn = P.normal + 3 * i;
        n0 = nn[0]; n1 = nn[1]; n2 = nn[2];
      }
      for (int cz = lo2; cz <= hi2; ++cz)
        for (int cy = lo1; cy <= hi1; ++cy)
          for (int cx = lo0; cx <= hi0; ++cx) {
            const unsigned b = bucket_of(cx, cy, cz, P.mask);
            const unsigned s = P.start[b];
            unsigned e = P.start[b + 1];
            e = e < P.cap ? e : P.cap;
            for (unsigned j = s; j < e; ++j) {
              const int4 c = P.cell[j];
              if (c.x != cx || c.y != cy || c.z != cz) continue;  // a stranger, or a neighbour cell's photon: met under its own cell
              const double* rec = P.rec + 9 * (size_t)j;
              const double e0 = rec[0] - x0, e1 = rec[1] - x1, e2 = rec[2] - x2;
              const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
              if (!(d2 < r2)) continue;
              if (P.normal) {
                const double dn = (rec[6] * n0 + rec[7] * n1) + rec[8] * n2;
                if (!(dn < 0.0)) continue;
              }
              const double w = P.kernel == TOR_PHOTON_KERNEL_EPANECHNIKOV ? 1.0 - d2 / r2 : 1.0;
              const double a0 = rec[3] * w, a1 = rec[4] * w, a2 = rec[5] * w;
              sx += quantize36(a0 < P.max_value ? a0 : P.max_value);
              sy += quantize36(a1 < P.max_value ? a1 : P.max_value);
              sz += quantize36(a2 < P.max_value ? a2 : P.max_value);
              ++count;
            }
          }
    }
  }
  double* o = P.sums + 3 * i;
  o[0] = sx; o[1] = sy; o[2] = sz;
  P.count[i] = count;
}

}  // namespace
}  // namespace tor

namespace {

// the map's bucket count for a list of n_list entries
int64_t photon_buckets(int64_t n_list) {
  const int64_t want = 2 * (n_list > 1 ? n_list : 1);
  int64_t nb = 16;
  while (nb < want && nb < ((int64_t)1 << 26)) nb <<= 1;
  return nb;
}

// where the 4 info words sit in ph_start, behind the n_buckets + 1 starts
size_t photon_info_offset(int64_t nb) { return ((size_t)(nb + 1) * 4 + 63) / 64 * 64; }

// the checks of a build that need no device and do not read *ctx; h = the cell size
int build_check(const char* who, TorContext* ctx, int64_t n, const void* list, int64_t n_list, double radius, bool nulls, double& h) {
  using tor::fail;
  const std::string w = who;
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (n < 0 || n_list < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_photons < 0 or n_list < 0");
  if (n > tor::kMaxPhotons || n_list > tor::kMaxPhotons) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_photons or n_list above 2^30");
  if (!list && n_list != n) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": without a list n_list must be n_photons");
  h = radius + radius * 9.5367431640625e-07;  // 2^-20
  if (!std::isfinite(radius) || !(radius > 0.0) || !std::isfinite(h))
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": radius must be finite and > 0, with a finite cell size");
  if (n > 0 && n_list > 0 && nulls) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL position or power");
  return TOR_OK;
}

// the build's launches; the arguments are checked
int build_launch(const char* who, TorContext* ctx, int64_t n, const double* d_pos, const double* d_pow, const double* d_dir,
                 const int32_t* d_list, int64_t n_list, double radius, double h, hipStream_t stream) {
  int rc = tor::query_stream_rule(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::HitQueryState& hq = ctx->hitq;
  const int64_t nb = photon_buckets(n_list);
  const int64_t n_tiles = (nb + tor::kPhTile - 1) / tor::kPhTile;
  const size_t slots = (size_t)(n_list > 0 ? n_list : 1);
  const size_t info_at = photon_info_offset(nb);
  const size_t key_bytes = (slots * 4 + 63) / 64 * 64, cnt_bytes = (size_t)nb * 4, tile_bytes = ((size_t)n_tiles * 4 + 63) / 64 * 64;
  hq.ph_built = false;  // (until the launches below are queued: a failed allocation leaves no half-made map behind)
  HIP_TRY(hq.ph_cell.ensure(slots * 16));
  HIP_TRY(hq.ph_rec.ensure(slots * 72));
  HIP_TRY(hq.ph_start.ensure(info_at + 32));
  HIP_TRY(hq.ph_tmp.ensure(key_bytes + cnt_bytes + tile_bytes));
  tor::BParams P{};
  P.pos = d_pos;
  P.pow = d_pow;
  P.dir = d_dir;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n = (long long)n;
  P.h = h;
  P.mask = (unsigned)(nb - 1);
  P.n_buckets = (long long)nb;
  P.key = (unsigned*)hq.ph_tmp.ptr;
  P.cnt = (unsigned*)((char*)hq.ph_tmp.ptr + key_bytes);
  P.tile = (unsigned*)((char*)hq.ph_tmp.ptr + key_bytes + cnt_bytes);
  P.n_tiles = (long long)n_tiles;
  P.start = (unsigned*)hq.ph_start.ptr;
  P.info = (unsigned long long*)((char*)hq.ph_start.ptr + info_at);
  P.cell = (int4*)hq.ph_cell.ptr;
  P.rec = (double*)hq.ph_rec.ptr;
  HIP_TRY(hipMemsetAsync(P.cnt, 0, cnt_bytes, stream));
  HIP_TRY(hipMemsetAsync(P.info, 0, 32, stream));
  const unsigned grid = (unsigned)((n_list + tor::kPhThreads - 1) / tor::kPhThreads);
  if (n_list > 0) {
    hipLaunchKernelGGL(tor::photon_classify_kernel, dim3(grid), dim3(tor::kPhThreads), 0, stream, P);
    hipLaunchKernelGGL(tor::photon_histogram_kernel, dim3(grid), dim3(tor::kPhThreads), 0, stream, P);
  }
  hipLaunchKernelGGL(tor::photon_tile_sums_kernel, dim3((unsigned)n_tiles), dim3(tor::kPhThreads), 0, stream, P);
  hipLaunchKernelGGL(tor::photon_scan_top_kernel, dim3(1), dim3(tor::kPhTopThreads), 0, stream, P);
  hipLaunchKernelGGL(tor::photon_scan_apply_kernel, dim3((unsigned)n_tiles), dim3(tor::kPhThreads), 0, stream, P);
  if (n_list > 0) hipLaunchKernelGGL(tor::photon_scatter_kernel, dim3(grid), dim3(tor::kPhThreads), 0, stream, P);
  rc = tor::query_done(ctx, stream);
  if (rc != TOR_OK) return rc;
  hq.ph_built = true;
  hq.ph_has_dir = d_dir != nullptr || n == 0 || n_list == 0;  // (a build without a photon array holds nothing that normals could miss)
  hq.ph_radius = radius;
  hq.ph_h = h;
  hq.ph_buckets = nb;
  tor::set_last_note("photons build: " + std::to_string((long long)nb) + " buckets");
  return TOR_OK;
}

// the checks of a gather that need no device; the map's come last and read *ctx
int gather_check(const char* who, TorContext* ctx, int64_t n, const void* list, int64_t n_list, int32_t kernel, double max_value,
                 bool nulls, bool normals) {
  using tor::fail;
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n, list, n_list);
  if (rc != TOR_OK) return rc;
  if (kernel != TOR_PHOTON_KERNEL_CONSTANT && kernel != TOR_PHOTON_KERNEL_EPANECHNIKOV)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": kernel must be TOR_PHOTON_KERNEL_CONSTANT (0) or TOR_PHOTON_KERNEL_EPANECHNIKOV (1)");
  if (!(max_value > 0.0 && max_value <= 128.0))
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": max_value must lie in (0, 128] (the sums must stay within quantize36's exact range)");
  if (n > 0 && n_list > 0 && nulls) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL point, sums or count");
  if (!ctx->hitq.ph_built) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no photon map built");
  if (normals && !ctx->hitq.ph_has_dir) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": normals given, but the map was built without directions");
  return TOR_OK;
}

// the launch; the arguments are checked, n > 0 and n_list > 0
int gather_launch(const char* who, TorContext* ctx, int64_t n, const double* d_point, const double* d_normal, const double* d_radius,
                  const int32_t* d_list, int64_t n_list, int32_t kernel, double max_value, double* d_sums, int32_t* d_count,
                  hipStream_t stream) {
  int rc = tor::query_stream_rule(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  const tor::HitQueryState& hq = ctx->hitq;
  tor::GParams P{};
  P.point = d_point;
  P.normal = d_normal;
  P.radius = d_radius;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n = (long long)n;
  P.kernel = kernel;
  P.max_value = max_value;
  P.R = hq.ph_radius;
  P.h = hq.ph_h;
  P.mask = (unsigned)(hq.ph_buckets - 1);
  const size_t cap = hq.ph_cell.bytes / 16;
  P.cap = (unsigned)(cap < 0xffffffffull ? cap : 0xffffffffull);
  P.start = (const unsigned*)hq.ph_start.ptr;
  P.cell = (const int4*)hq.ph_cell.ptr;
  P.rec = (const double*)hq.ph_rec.ptr;
  P.sums = d_sums;
  P.count = d_count;
  const unsigned grid = (unsigned)((n_list + tor::kPhThreads - 1) / tor::kPhThreads);
  hipLaunchKernelGGL(tor::photon_gather_kernel, dim3(grid), dim3(tor::kPhThreads), 0, stream, P);
  rc = tor::query_done(ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::set_last_note("photons gather");
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_photons_build_device(TorContext* ctx, int64_t n_photons, const double* d_position, const double* d_power, const double* d_direction,
                             const int32_t* d_list, int64_t n_list, double radius, void* hip_stream) {
  const char* who = "tor_photons_build_device";
  double h = 0.0;
  const int rc = build_check(who, ctx, n_photons, d_list, n_list, radius, !d_position || !d_power, h);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return build_launch(who, ctx, n_photons, d_position, d_power, d_direction, d_list, n_list, radius, h, (hipStream_t)hip_stream);
}

int tor_photons_build_host(TorContext* ctx, int64_t n_photons, const double* position, const double* power, const double* direction,
                           const int32_t* list, int64_t n_list, double radius) {
  const char* who = "tor_photons_build_host";
  double h = 0.0;
  int rc = build_check(who, ctx, n_photons, list, n_list, radius, !position || !power, h);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t m = (size_t)n_photons;
  tor::HostPart st[4] = {{position, position ? m * 24 : 0, true, false},
                         {power, power ? m * 24 : 0, true, false},
                         {direction, direction ? m * 24 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false}};
  rc = tor::stage_in(ctx, st, 4);
  if (rc != TOR_OK) return rc;
  // (an empty array stages to a null pointer: a list keeps a non-null one, never dereferenced, so that it stays a list)
  const int32_t* d_list = list ? (st[3].dev ? st[3].as<const int32_t>() : (const int32_t*)16) : nullptr;
  const double* d_dir = direction ? (st[2].dev ? st[2].as<const double>() : (const double*)16) : nullptr;
  rc = build_launch(who, ctx, n_photons, st[0].as<const double>(), st[1].as<const double>(), d_dir, d_list, n_list, radius, h, nullptr);
  if (rc != TOR_OK) return rc;
  HIP_TRY(hipStreamSynchronize(nullptr));  // the map is copied out of the staging buffer before the entry returns
  return TOR_OK;
}

int tor_photons_gather_device(TorContext* ctx, int64_t n_points, const double* d_point, const double* d_normal, const double* d_radius,
                              const int32_t* d_list, int64_t n_list, int32_t kernel, double max_value, double* d_sums, int32_t* d_count,
                              void* hip_stream) {
  const char* who = "tor_photons_gather_device";
  const int rc = gather_check(who, ctx, n_points, d_list, n_list, kernel, max_value, !d_point || !d_sums || !d_count, d_normal != nullptr);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return gather_launch(who, ctx, n_points, d_point, d_normal, d_radius, d_list, n_list, kernel, max_value, d_sums, d_count,
                       (hipStream_t)hip_stream);
}

int tor_photons_gather_host(TorContext* ctx, int64_t n_points, const double* point, const double* normal, const double* radius,
                            const int32_t* list, int64_t n_list, int32_t kernel, double max_value, double* sums, int32_t* count) {
  const char* who = "tor_photons_gather_host";
  int rc = gather_check(who, ctx, n_points, list, n_list, kernel, max_value, !point || !sums || !count, normal != nullptr);
  if (rc != TOR_OK || n_points == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t m = (size_t)n_points;
  tor::HostPart st[6] = {{point, m * 24, true, false},
                         {normal, normal ? m * 24 : 0, true, false},
                         {radius, radius ? m * 8 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {sums, m * 24, true, true},
                         {count, m * 4, true, true}};
  rc = tor::stage_in(ctx, st, 6);
  if (rc != TOR_OK) return rc;
  rc = gather_launch(who, ctx, n_points, st[0].as<const double>(), st[1].as<const double>(), st[2].as<const double>(),
                     st[3].as<const int32_t>(), n_list, kernel, max_value, st[4].as<double>(), st[5].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 6);
}

int tor_photons_info(TorContext* ctx, int64_t out[4]) {
  using tor::fail;
  const std::string w = "tor_photons_info";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!out) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": out is NULL");
  if (!ctx->hitq.ph_built) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no photon map built");
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->hitq.launched) HIP_TRY(hipEventSynchronize(ctx->hitq.ev_done));
  HIP_TRY(hipMemcpy(out, (const char*)ctx->hitq.ph_start.ptr + photon_info_offset(ctx->hitq.ph_buckets), 32, hipMemcpyDeviceToHost));
  return TOR_OK;
}

}  // extern "C"
