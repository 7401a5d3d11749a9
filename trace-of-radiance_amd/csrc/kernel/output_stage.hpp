// kernel/output_stage.hpp -- the small kernels around the integrator: finalize (canvas.nim:47-54), resolve / accum_noise (progressive rendering), adaptive select / resolve_counts (adaptive sampling), quantize (io/ppm.nim:15-16),
// encode_ipcm (animation output stage), gather_rows (multi-GPU assembly), selftest, spin_until.  Textually included by tor_kernels.hip.
// canvas.nim:47-54
__global__ __launch_bounds__(256) void finalize_kernel(double* pixels, long long n_values, double scale,
                                                        double gamma) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_values) pixels[i] = pow_pos(scale * pixels[i], gamma);
}

// Progressive rendering (tor_resolve_device): finalize_kernel's operations on sums that stay where they are, so a resolved
// progressive frame is the one-shot frame bit for bit and more passes can follow.  pixels == sums is allowed.
__global__ __launch_bounds__(256) void resolve_kernel(const double* sums, double* pixels, long long n_values, double scale,
                                                       double gamma) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_values) pixels[i] = pow_pos(scale * sums[i], gamma);
}

// var / n of the standard error.  (TOR_ACCUM_MUTATE == 2: the mutation check of the oracle tests -- var * (1.0 / n), one rounding more,
// which differs from var / n in the last bit for most n that are not powers of two.)
#if defined(TOR_ACCUM_MUTATE) && TOR_ACCUM_MUTATE == 2
#define TOR_ACCUM_VAR_OVER_N(var, n) ((var) * (1.0 / (n)))
#else
#define TOR_ACCUM_VAR_OVER_N(var, n) ((var) / (n))
#endif

// Progressive rendering (tor_accum_noise_device): per pixel, the largest over the channels of the standard error of the mean,
// sqrt(max(0, (M - S*S/n) / (n - 1)) / n), linear units; err nullable.  Block b sums / maxes pixels b*256 + t + k*gridDim*256
// in a fixed order and a fixed tree: partials[2b] = sum, partials[2b + 1] = max.
// Outside the finite: `var > 0.0 ? var : 0.0` takes a NaN variance to 0, so a channel whose sum is NaN or infinite (S * S / n = inf,
// M - inf = -inf or NaN) reports noise 0; only an infinite moment beside a finite sum reports inf.  No NaN leaves this kernel.
__global__ __launch_bounds__(256) void accum_noise_kernel(const double* sums, const double* moments, long long npix, double n,
                                                           double* err, double* partials) {
  __shared__ double s_sum[256], s_max[256];
  double acc = 0.0, mx = 0.0;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += stride) {
    double e = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double S = sums[i * 3 + c], M = moments[i * 3 + c];
      double var = (M - S * S / n) / (n - 1.0);
      var = var > 0.0 ? var : 0.0;
      const double se = __builtin_sqrt(TOR_ACCUM_VAR_OVER_N(var, n));
      e = se > e ? se : e;
    }
    if (err) err[i] = e;
    acc += e;
    mx = e > mx ? e : mx;
  }
  s_sum[threadIdx.x] = acc;
  s_max[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
      s_max[threadIdx.x] = s_max[threadIdx.x + w] > s_max[threadIdx.x] ? s_max[threadIdx.x + w] : s_max[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = s_sum[0];
    partials[2 * blockIdx.x + 1] = s_max[0];
  }
}

// ... and the partials of its n_blocks blocks, again in a fixed order: out2 = {sum, max}
__global__ __launch_bounds__(256) void accum_noise_finish_kernel(const double* partials, int n_blocks, double* out2) {
  __shared__ double s_sum[256], s_max[256];
  double acc = 0.0, mx = 0.0;
  for (int b = threadIdx.x; b < n_blocks; b += 256) {
    acc += partials[2 * b];
    mx = partials[2 * b + 1] > mx ? partials[2 * b + 1] : mx;
  }
  s_sum[threadIdx.x] = acc;
  s_max[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
      s_max[threadIdx.x] = s_max[threadIdx.x + w] > s_max[threadIdx.x] ? s_max[threadIdx.x + w] : s_max[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out2[0] = s_sum[0];
    out2[1] = s_max[0];
  }
}

// ---- adaptive sampling (tor_adaptive_select_device, tor_resolve_counts_device) ------------------------------------------------
// Convergence of a pixel with sums S, moments M of n samples: per channel, mean = S / n, se = sqrt(max(0, (M - S*S/n) / (n-1)) / n)
// (accum_noise_kernel's operations), converged iff se <= abs_tol + rel_tol * mean in all three channels.  Every operation is one IEEE
// float64 rounding, nothing fused, so a host restatement in float64 reproduces the keep set bit for bit.
// Outside the finite: a channel whose sum is NaN or infinite has se = 0 (as in accum_noise_kernel) and mean = NaN or +-inf.  A NaN
// mean, or rel_tol = 0 beside an infinite one (0 * inf), makes the right-hand side NaN, and a mean of -inf makes it -inf: `<=` is
// false and the pixel never converges.  A sum of +inf with rel_tol > 0 converges (0 <= inf), as does anything under abs_tol = inf
// whose right-hand side is not NaN.
__device__ __forceinline__ bool adaptive_still_active(const double* sums, const double* moments, unsigned pix, double n, double abs_tol,
                                                      double rel_tol) {
#pragma clang fp contract(off)
  bool converged = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double S = sums[(size_t)pix * 3 + c], M = moments[(size_t)pix * 3 + c];
    const double mean = S / n;
    double var = (M - S * S / n) / (n - 1.0);
    var = var > 0.0 ? var : 0.0;
    const double se = __builtin_sqrt(TOR_ACCUM_VAR_OVER_N(var, n));
    converged = converged && se <= abs_tol + rel_tol * mean;
  }
  return !converged;
}

// Ordered compaction of the list, in tiles of kSelTile entries per 256-thread block: entry i of block b is b * kSelTile + k * 256 + t.
constexpr int kSelTile = 1024;

// pass 1: counts[pix] = n for every listed pixel, keep[i] = not converged, block_count[b] = the block's survivors (wave ballots)
__global__ __launch_bounds__(256) void adaptive_count_kernel(const double* sums, const double* moments, const int32_t* list_in, long long n_in,
                                                              double n, double abs_tol, double rel_tol, int32_t* counts, uint8_t* keep,
                                                              unsigned* block_count) {
  __shared__ unsigned s_cnt[4];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  unsigned mine = 0;
  for (int k = 0; k < kSelTile / 256; ++k) {
    const long long i = (long long)blockIdx.x * kSelTile + k * 256 + threadIdx.x;
    bool act = false;
    if (i < n_in) {
      const unsigned pix = (unsigned)list_in[i];
      counts[pix] = (int32_t)n;
      act = adaptive_still_active(sums, moments, pix, n, abs_tol, rel_tol);
      keep[i] = act ? 1 : 0;
    }
    mine += (unsigned)__builtin_popcountll(ballot64(act));
  }
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// pass 2 (one block): block_count -> exclusive offsets in place, the total to *n_out
__global__ __launch_bounds__(1024) void adaptive_scan_kernel(unsigned* block_count, int n_blocks, int32_t* n_out) {
  __shared__ unsigned s[1024];
  const int t = (int)threadIdx.x;
  const int per = (n_blocks + 1023) / 1024;  // thread t owns blocks [t * per, (t + 1) * per)
  const int b0 = t * per;
  const int b1 = (b0 + per < n_blocks) ? b0 + per : n_blocks;
  unsigned sum = 0;
  for (int b = b0; b < b1; ++b) sum += block_count[b];
  s[t] = sum;
  __syncthreads();
  for (int w = 1; w < 1024; w <<= 1) {  // inclusive Hillis-Steele scan of the 1024 thread totals
    const unsigned v = t >= w ? s[t - w] : 0u;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  unsigned run = s[t] - sum;
  for (int b = b0; b < b1; ++b) {
    const unsigned c = block_count[b];
    block_count[b] = run;
    run += c;
  }
  if (t == 1023) *n_out = (int32_t)s[1023];
}

// pass 3: the survivors to list_out at their block's offset + their rank inside the block, in input order
__global__ __launch_bounds__(256) void adaptive_scatter_kernel(const int32_t* list_in, long long n_in, const uint8_t* keep,
                                                                const unsigned* block_offset, int32_t* list_out) {
  __shared__ unsigned s_cnt[kSelTile / 256][4];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  unsigned long long masks[kSelTile / 256];
  for (int k = 0; k < kSelTile / 256; ++k) {
    const long long i = (long long)blockIdx.x * kSelTile + k * 256 + threadIdx.x;
    masks[k] = ballot64(i < n_in && keep[i] != 0);
    if (lane == 0) s_cnt[k][wave] = (unsigned)__builtin_popcountll(masks[k]);
  }
  __syncthreads();
  unsigned run = block_offset[blockIdx.x];
  for (int k = 0; k < kSelTile / 256; ++k) {
    const long long i = (long long)blockIdx.x * kSelTile + k * 256 + threadIdx.x;
    unsigned before = run;
    for (int w = 0; w < wave; ++w) before += s_cnt[k][w];
    if ((masks[k] >> lane) & 1ull) list_out[before + lane_prefix(masks[k])] = list_in[i];
    run += s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
  }
}

// resolve_kernel with each pixel's own sample count: (1.0 / (double)c) is the host's scale of tor_resolve_device at total_samples = c,
// so a pixel's value is that call's, bit for bit.  pixels == sums is allowed.
__global__ __launch_bounds__(256) void resolve_counts_kernel(const double* sums, const int32_t* counts, double* pixels, long long n_values,
                                                              double gamma) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_values) pixels[i] = pow_pos((1.0 / (double)counts[i / 3]) * sums[i], gamma);
}

// io/ppm.nim:15-16 ; safe_math.nim:10-14: int(256 * clamp(c, 0, 0.999)).  A NaN channel is black: `c > 0.0` is tested first, so that
// no NaN reaches the float-to-int conversion (undefined in C++; the reference's int(256 * clamp(NaN)) is undefined too).  The same
// text stands in encode_ipcm_kernel below, in tor_canvas_to_rgb8 (tor_host.cpp) and in the oracle's two quantisers.
__device__ __forceinline__ int quantize_channel(double c) {
  const double cl = (c > 0.0) ? ((c > 0.999) ? 0.999 : c) : 0.0;
  return (int)(256 * cl);
}

__global__ __launch_bounds__(256) void quantize_kernel(const double* pixels, long long n_values, uint8_t* out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_values) out[i] = (uint8_t)quantize_channel(pixels[i]);
}

// ---------------------------------------------------------------------------------------------
// Per-frame output stage of the animation driver (trace_of_radiance_animation.nim:186-196), fused:
//   Canvas -> RGB8        io/rgb.nim:17-31   uint8(256 * clamp(c, 0, 0.999)), top scanline first; a NaN channel is 0.
//                         (rgb.nim:29-31 indexes canvas[nrows - i, j], one row past the end for
//                         i = 0; the intended flip canvas[nrows - 1 - i, j] is implemented here.)
//   RGB8 -> Y'CbCr 4:2:0  io/color_conversions.nim:180-252, BT.601 fixed point:
//                         kr,kg,kb = 77,150,29 (>>8); y_scale = 110 (>>7), y_min = 16; fb = 127, fr = 160 (>>8)
//   planes -> I_PCM slice io/h264.nim:189-259: slice header, per macroblock [0x0d 0x00 except the
//                         first] + 256 Y + 64 Cb + 64 Cr raw bytes, stop byte 0x80.
// One workgroup per 16x16 macroblock, one thread per pixel.  Integer and byte work, HBM-bound:
// 24 B read and 1.5 B written per pixel.
__global__ __launch_bounds__(256) void encode_ipcm_kernel(const double* pixels, int nrows, int ncols, uint8_t* out,
                                                          uint8_t* plane_y, uint8_t* plane_cb, uint8_t* plane_cr) {
  __shared__ short s_u[256], s_v[256];
  const int mb_cols = (ncols + 15) >> 4;
  const int mb = blockIdx.x;
  const int mi = mb / mb_cols, mj = mb - mi * mb_cols;
  const int x = threadIdx.x >> 4, y = threadIdx.x & 15;      // row, column inside the macroblock
  const int vr = mi * 16 + x, vc = mj * 16 + y;              // video row (0 = top), column
  // a size that is not a multiple of 16: the last macroblock row / column is padded by edge replication (the SPS crops it)
  const int sr = vr < nrows ? vr : nrows - 1, sc = vc < ncols ? vc : ncols - 1;
  const bool inside = vr < nrows && vc < ncols;
  const double* px = pixels + ((size_t)(nrows - 1 - sr) * ncols + sc) * 3;
  int rgb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[c] = quantize_channel(px[c]);  // safe_math.nim:10-14; in [0, 255], a NaN channel 0
  const int tY = (77 * rgb[0] + 150 * rgb[1] + 29 * rgb[2]) >> 8;     // color_conversions.nim:218-220
  const uint8_t Y = (uint8_t)(((tY * 110) >> 7) + 16);                // :223
  s_u[threadIdx.x] = (short)(rgb[2] - tY);                            // :221
  s_v[threadIdx.x] = (short)(rgb[0] - tY);                            // :222
  const size_t data = 9 + (size_t)mb * 386;                           // first payload byte of this macroblock
  out[data + threadIdx.x] = Y;
  if (plane_y && inside) plane_y[(size_t)vr * ncols + vc] = Y;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int cx = threadIdx.x >> 3, cy = threadIdx.x & 7;
    const int b0 = (2 * cx) * 16 + 2 * cy;
    const int tU = s_u[b0] + s_u[b0 + 1] + s_u[b0 + 16] + s_u[b0 + 17];
    const int tV = s_v[b0] + s_v[b0 + 1] + s_v[b0 + 16] + s_v[b0 + 17];
    const uint8_t U = (uint8_t)((((tU >> 2) * 127) >> 8) + 128);      // :249
    const uint8_t V = (uint8_t)((((tV >> 2) * 160) >> 8) + 128);      // :250
    out[data + 256 + threadIdx.x] = U;
    out[data + 320 + threadIdx.x] = V;
    const size_t cpos = (size_t)(mi * 8 + cx) * (ncols >> 1) + (mj * 8 + cy);
    const bool cinside = mi * 8 + cx < (nrows >> 1) && mj * 8 + cy < (ncols >> 1);
    if (plane_cb && cinside) plane_cb[cpos] = U;
    if (plane_cr && cinside) plane_cr[cpos] = V;
  }
  if (threadIdx.x == 0) {
    if (mb == 0) {  // h264.nim:38: constant slice header (start code, IDR slice NAL, I_PCM first macroblock)
      const uint8_t hdr[9] = {0x00, 0x00, 0x00, 0x01, 0x05, 0x88, 0x84, 0x21, 0xa0};
      for (int k = 0; k < 9; ++k) out[k] = hdr[k];
    } else {        // h264.nim:39,191-192: mb_type I_PCM for every further macroblock
      out[data - 2] = 0x0d;
      out[data - 1] = 0x00;
    }
    if (mb == (int)gridDim.x - 1) out[data + 384] = 0x80;  // h264.nim:40,259: slice stop bit
  }
}

// Multi-GPU assembly: the shards arrive rank-major and compact; put every row at its image position.
// One thread per float64 value; HBM-bound copy (48 B per pixel).
__global__ __launch_bounds__(256) void gather_rows_kernel(const double* gathered, double* frame, int nrows, int ncols,
                                                          int row_tile, int shard_count, long long shard_stride) {
  const long long row_values = (long long)ncols * 3;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)nrows * row_values) return;
  const int row = (int)(i / row_values);
  const long long within_row = i - (long long)row * row_values;
  const int tile = row / row_tile;
  const int shard = tile % shard_count;
  const int local_row = (tile / shard_count) * row_tile + (row - tile * row_tile);
  frame[i] = gathered[(long long)shard * shard_stride + (long long)local_row * row_values + within_row];
}

// keeps its stream busy until the host sets *flag (or max_ticks pass): the stand-in for a collective that never completes
__global__ void spin_until_kernel(volatile unsigned* flag, unsigned long long max_ticks) {
  const unsigned long long t0 = wall_clock64();
  while (*flag == 0u && wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(127);
}

__global__ void selftest_kernel(int op, const double* x, const double* y, double* out0, double* out1,
                                long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  selftest_math_one(op, x[i], y ? y[i] : 0.0, out0[i], out1 ? out1[i] : out0[i]);
}

