// tor_deposit.hip -- exact sample deposits (tor_deposit_device, include/tor_render.h): the deposit of kernel/integrate_deposit.inc on
// its own, for colours and pixel numbers the caller supplies -- the film of a host-written integrator, on gfx950.
//
// What a deposit is.  Entry i (i = 0 .. n - 1, or the listed i = index[j] inside [0, n)) carries a colour c = color[3 i ..] and a
// pixel p = pixel[i].  p outside [0, npix) deposits nothing and is not counted.  A colour with any channel NaN, +-inf or < 0 is
// rejected as a whole (-0.0 passes) and counted once in *rejected.  Otherwise, per channel,
//     q = quantize36(min(c, max_value));   sums[3 p + ch] += q;   moments[3 p + ch] += quantize36(q * q);   counts[p] += 1
// with tor_device.hpp's quantize36, q * q one rounding, nothing fused (-ffp-contract=off) -- SEEDING 3's operations.
//
// Why every order gives the same bits.  Every addend is a non-negative multiple of 2^-36 (q <= max_value <= 2^7 < 2^15, so
// quantize36 is exact in its range; q * q <= 2^14 likewise).  While a pixel has received at most 2^17 / max(max_value, max_value^2)
// accepted samples its sums stay below 2^17, i.e. integers below 2^53 in units of 2^-36: exact in float64.  Addends are never
// negative, so EVERY partial sum -- a run's inside the wave, HBM's at any moment -- is at most the final one and exact too.  Hence
// the wave may combine what shares a pixel in any grouping, and the atomics may arrive in any order.
//
// The kernel.  One entry per lane, grid-stride by workgroup (the loop bound is wave-uniform: every lane takes part in the shuffles).
//   live   the lane holds an accepted sample for a pixel in range; every other lane contributes nothing and belongs to no run
//   head   live, and lane 0 or the lane below is not live or holds another pixel: the first lane of a RUN of adjacent live lanes
//          with one pixel
//   run    the number of heads at or below the lane (prefix count of the head ballot); -1 for a lane that is not live
// {q, quantize36(q * q), 1} are reduced per run by a backward segmented scan: for d = 1, 2, 4 .. 32 a lane adds lane + d's partial
// iff that lane has the SAME RUN NUMBER.  After step d = 2^k lane i holds the sum over [i, min(i + 2^(k+1) - 1, end of i's run)]
// (induction: the partner's partial covers exactly the next 2^k lanes of the run, or the partner is past the run's end, which
// means the run was already complete); runs are contiguous, so the head ends with the whole run.  Comparing pixels instead of run
// numbers would be wrong: with lanes A A A B A lane 0 would add, at d = 4, the partial of lane 4, which lane 4 -- a head too --
// flushes again (and with A B A B, once any run of the wave keeps the scan going to d = 2, lane 0 would add lane 2's sample).
// The scan stops at the first d at which no lane finds a partner (run lengths <= d: none will at 2 d either) and is skipped when
// every live lane is a head, so entries in random order (every run of length 1) pay no reduction step.  Only heads issue atomics:
// in camera order with k samples per pixel that is ceil(64 / k) heads per wave writing adjacent 24-byte records, one head per wave
// from k = 64.  *rejected gets one atomic per wave and pass, of the ballot's population count.
//
// The flush.  With few heads each head adds its three (six) values itself.  With kSpreadHeads or more heads in the wave that shape is
// slow: every atomic instruction has one lane per 24-byte record, 8 bytes each, so each of the 3 (6) instructions touches every
// record of the wave (measured at k = 1 in camera order: 0.35 of torch.index_add_).  The spread flush hands the values
// round instead: the wave's values form a list (lane, channel), and lane l of step t = 0, 1, 2 adds element 64 t + l -- the value
// of lane (64 t + l) / 3, channel (64 t + l) % 3, fetched by shuffle -- iff that lane is a head.  The same atomics, only issued by
// other lanes: three neighbouring lanes now cover one record, and consecutive pixels give contiguous addresses.  Measured: 3.0
// times the plain flush at k = 1 in camera order, 2.4 times in random order, nothing lost where it does not run.
//
// No LDS, no scratch (the cross-lane steps are ds_bpermute: LDS hardware, no LDS allocation).  It reads no scene and no render
// state: the context only names the device and its size.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "tor_context.hpp"
#include "tor_device.hpp"

namespace tor {
namespace {

constexpr int kDepThreads = 256;
constexpr int kSpreadHeads = 32;  // heads per wave from which the spread flush runs (measured at 64 and at <= 4 heads only)

struct DParams {
  const double* color;  // 3 float64 per entry
  const int* pixel;     // one int32 per entry
  const int* index;     // the entries to deposit, or null: list slot j is entry j
  long long n;          // entries
  long long n_list;     // list slots (n without a list)
  long long npix;
  double max_value;
  double* sums;               // 3 float64 per pixel
  double* moments;            // 3 float64 per pixel, or null
  int* counts;                // one int32 per pixel, or null
  unsigned long long* rejected;  // one int64, added to, or null
};

__device__ __forceinline__ double down(double v, int d) { return __shfl_down(v, d, 64); }

__global__ __launch_bounds__(kDepThreads) void deposit_kernel(const DParams P) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * kDepThreads;
  for (long long base = (long long)blockIdx.x * kDepThreads; base < P.n_list; base += stride) {
    const long long j = base + threadIdx.x;
    long long i = -1;  // the entry of list slot j; -1: past the end of the list, or a listed entry outside [0, n) (skipped)
    if (j < P.n_list) {
      const long long v = P.index ? (long long)P.index[j] : j;
      if (v >= 0 && v < P.n) i = v;
    }
    int pix = -1;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    bool live = false, bad = false;
    if (i >= 0) {
      const long long p = (long long)P.pixel[i];
      if (p >= 0 && p < P.npix) {
        const double* c = P.color + 3 * i;
        const double cx = c[0], cy = c[1], cz = c[2];
        // NaN fails c >= 0; -0.0 passes it; -inf and negatives fail it; +inf is caught on its own
        const bool ok = (cx >= 0.0) && (cy >= 0.0) && (cz >= 0.0) && (cx < __builtin_inf()) && (cy < __builtin_inf()) &&
                        (cz < __builtin_inf());
        bad = !ok;
        if (ok) {
          live = true;
          pix = (int)p;
          qx = quantize36(cx < P.max_value ? cx : P.max_value);
          qy = quantize36(cy < P.max_value ? cy : P.max_value);
          qz = quantize36(cz < P.max_value ? cz : P.max_value);
        }
      }
    }
    if (P.rejected) {
      const unsigned long long bad_mask = __ballot(bad);
      if (bad_mask != 0 && lane == 0) atomicAdd(P.rejected, (unsigned long long)__popcll(bad_mask));
    }
    const unsigned long long live_mask = __ballot(live);
    if (live_mask == 0) continue;
    const bool want_mom = P.moments != nullptr;
    double mx = 0.0, my = 0.0, mz = 0.0;
    if (want_mom && live) {  // q * q: one rounding, then rounded to 2^-36 like q itself (SEEDING 3, integrate_deposit.inc)
      mx = quantize36(qx * qx);
      my = quantize36(qy * qy);
      mz = quantize36(qz * qz);
    }
    int cnt = live ? 1 : 0;
    // runs: the lane below is lane - 1 (lane 0 has none)
    const int below_pix = __shfl_up(pix, 1, 64);
    const bool head = live && (lane == 0 || below_pix != pix);  // (a lane that is not live holds pix = -1, which no live lane holds)
    const unsigned long long head_mask = __ballot(head);
    const int run = live ? (int)__popcll(head_mask & ((2ull << lane) - 1ull)) : -1;
    if (head_mask != live_mask) {  // some run is longer than one lane
      for (int d = 1; d < 64; d <<= 1) {
        const int other = __shfl_down(run, d, 64);
        const bool same = live && (lane + d < 64) && (other == run);
        if (__ballot(same) == 0) break;
        const double ax = down(qx, d), ay = down(qy, d), az = down(qz, d);
        const int ac = __shfl_down(cnt, d, 64);
        if (same) {
          qx += ax; qy += ay; qz += az;
          cnt += ac;
        }
        if (want_mom) {
          const double bx = down(mx, d), by = down(my, d), bz = down(mz, d);
          if (same) {
            mx += bx; my += by; mz += bz;
          }
        }
      }
    }
    if (__popcll(head_mask) >= kSpreadHeads) {
      // spread flush (the file head): lane l of step t adds element 64 t + l of the wave's (lane, channel) list, if that lane is a head
      const int hd = head ? 1 : 0;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int e = 64 * t + lane, src = e / 3, ch = e - 3 * src;  // src <= 63
        const int sp = __shfl(pix, src, 64), sh = __shfl(hd, src, 64);
        const double vx = __shfl(qx, src, 64), vy = __shfl(qy, src, 64), vz = __shfl(qz, src, 64);
        if (sh) unsafeAtomicAdd(P.sums + 3 * (size_t)sp + ch, ch == 0 ? vx : ch == 1 ? vy : vz);
        if (want_mom) {
          const double wx = __shfl(mx, src, 64), wy = __shfl(my, src, 64), wz = __shfl(mz, src, 64);
          if (sh) unsafeAtomicAdd(P.moments + 3 * (size_t)sp + ch, ch == 0 ? wx : ch == 1 ? wy : wz);
        }
      }
      if (head && P.counts) atomicAdd(P.counts + pix, cnt);
    } else if (head) {
      double* s = P.sums + 3 * (size_t)pix;
      unsafeAtomicAdd(s + 0, qx);
      unsafeAtomicAdd(s + 1, qy);
      unsafeAtomicAdd(s + 2, qz);
      if (want_mom) {
        double* m = P.moments + 3 * (size_t)pix;
        unsafeAtomicAdd(m + 0, mx);
        unsafeAtomicAdd(m + 1, my);
        unsafeAtomicAdd(m + 2, mz);
      }
      if (P.counts) atomicAdd(P.counts + pix, cnt);
    }
  }
}

}  // namespace
}  // namespace tor

extern "C" {

int tor_deposit_device(TorContext* ctx, int64_t n, const double* d_color, const int32_t* d_pixel, const int32_t* d_index,
                       int64_t n_index, double max_value, int64_t npix, double* d_sums, double* d_moments, int32_t* d_counts,
                       int64_t* d_rejected, void* hip_stream) {
  using tor::fail;
  const std::string w = "tor_deposit_device";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (n < 0 || n_index < 0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n < 0 or n_index < 0");
  const int64_t n_list = d_index ? n_index : n;
  const bool work = n > 0 && n_list > 0;
  if (work && (!d_color || !d_pixel || !d_sums)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL color, pixel or sums");
  if (npix < 1) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": npix < 1");
  if (!(max_value > 0.0 && max_value <= 128.0))
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": max_value must lie in (0, 128] (q * q must stay within quantize36's exact range)");
  if (!work) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  tor::DParams P{};
  P.color = d_color;
  P.pixel = d_pixel;
  P.index = d_index;
  P.n = (long long)n;
  P.n_list = (long long)n_list;
  P.npix = (long long)npix;
  P.max_value = max_value;
  P.sums = d_sums;
  P.moments = d_moments;
  P.counts = d_counts;
  P.rejected = (unsigned long long*)d_rejected;
  // grid-stride: enough workgroups to fill the device, never more than the list needs
  const int64_t need = (n_list + tor::kDepThreads - 1) / tor::kDepThreads;
  const int64_t fill = (int64_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 8;
  const unsigned grid = (unsigned)(need < fill ? need : fill);
  hipLaunchKernelGGL(tor::deposit_kernel, dim3(grid), dim3(tor::kDepThreads), 0, (hipStream_t)hip_stream, P);
  HIP_TRY(hipGetLastError());
  return TOR_OK;
}

}  // extern "C"
