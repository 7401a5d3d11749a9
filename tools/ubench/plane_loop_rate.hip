// plane_loop_rate.hip -- what bounds the float32 stage one of the plane-screened object loop (kernel/integrate_loop_plane.inc, PW == 2)
// now that its arithmetic is 4 vector instructions per object?  The loop alone: float32 records {cx', cz'} (8 bytes per object) through
// the scalar data path into SGPRs, v_fma_f32 + v_fmac_f32 + v_sub_f32 |v| - T + v_alignbit_b32 per object, whole words (32 objects), two
// per trip.  Workgroups of 256 threads (one wave per SIMD), 1, 2 or 3 of them per CU (the dynamic LDS size sets the occupancy the
// kernel's 168 VGPRs and 53.3 KB give it), four rounds of them over the whole machine.  Rows:
//   a  the loop as it is compiled today: plain loads, each s_load_dwordx16 requested one object ahead of the wait that needs it
//   b  each s_load_dwordx16 requested a whole group of 8 objects ahead of its wait (two 16-dword SGPR buffers), written by hand
//   c  two groups ahead (three buffers; the wait is lgkmcnt(1), which presumes that the scalar loads return in order -- the
//      checksum column says whether they did on this run; a measurement only)
//   d  loop-invariant operands, no loads: the floor
//   e  loads + v_alignbit only: the scalar path's own rate at 8 bytes per object
//   f  row b's feed, the two fma and the subtract as v_pk_fma_f32 / v_pk_add_f32 on adjacent object pairs from a {cxA, cxB, czA, czB}
//      record order: 5 issues per 2 objects instead of 8 (the packed add has no |.| modifier: the rate is what is measured
//      here, not the decision; its checksum differs)
//   g, h, i  rows d, a, b with the decision pushed as v_cmp_lt_f32 |v|, T + v_addc_co_u32 m, m, m (the carry shifts in) instead of
//      v_sub_f32 + v_alignbit_b32: the same bit, the same 4 issues
//   p0-p4  one instruction kind alone (four independent registers in turn): pipe cycles per wave64 instruction
// Floors, per object and wave of SIMD time at 2.4 GHz: the vector pipe at 8 cycles per object (4 wave64 float32 instructions of 2
// cycles) 3.33 ns; one wave's issue rate of an instruction per 4 cycles: 16 cycles per object, 6.67 / 3.33 / 2.22 ns at 1 / 2 / 3
// waves; row e is the measured floor of the scalar bytes.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/ubench/plane_loop_rate.hip -o plane_loop_rate && ./plane_loop_rate [out.txt]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

typedef float __attribute__((ext_vector_type(16))) f16v;
typedef float __attribute__((ext_vector_type(2))) f2v;
typedef const float __attribute__((address_space(4))) * cfptr;

// (the running mask goes through every request and wait: the chain of shifts then pins the objects of a group between its two
// statements, so a request keeps the distance it was written at)
#define FEED_REQ(buf, ptr, off) asm volatile("s_load_dwordx16 %0, %2, %3" : "=&s"(buf), "+v"(m) : "s"(ptr), "i"(off))
#define FEED_WAIT(buf, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+s"(buf), "+v"(m))
#define FEED_WAIT_REQ(cur, n, nxt, ptr, off) \
  asm volatile("s_waitcnt lgkmcnt(" #n ")\n\ts_load_dwordx16 %1, %3, %4" : "+s"(cur), "=&s"(nxt), "+v"(m) : "s"(ptr), "i"(off))

template <int PUSH>
__device__ __forceinline__ unsigned obj(unsigned m, float nx, float nz, float c0, float T, float cx, float cz) {
  const float v = __builtin_fmaf(nx, cx, __builtin_fmaf(nz, cz, c0));
  if (PUSH == 0) {
    const float q = __builtin_fabsf(v) - T;
    return __builtin_amdgcn_alignbit(m, __float_as_uint(q), 31);
  } else {
    unsigned long long keep, carry;
    unsigned r;
    asm("v_cmp_lt_f32_e64 %0, |%1|, %2" : "=s"(keep) : "v"(v), "v"(T));
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(carry) : "v"(m), "s"(keep));
    return r;
  }
}
template <int PUSH>
__device__ __forceinline__ unsigned group(unsigned m, float nx, float nz, float c0, float T, const f16v& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) m = obj<PUSH>(m, nx, nz, c0, T, b[2 * j], b[2 * j + 1]);
  return m;
}
__device__ __forceinline__ unsigned group_pk(unsigned m, f2v nx2, f2v nz2, f2v c02, f2v negT2, const f16v& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f2v cx = {b[4 * k], b[4 * k + 1]}, cz = {b[4 * k + 2], b[4 * k + 3]};
    f2v t, v, q;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(t) : "v"(nz2), "s"(cz), "v"(c02));
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(v) : "v"(nx2), "s"(cx), "v"(t));
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(q) : "v"(v), "v"(negT2));
    m = __builtin_amdgcn_alignbit(m, __float_as_uint(q[0]), 31);
    m = __builtin_amdgcn_alignbit(m, __float_as_uint(q[1]), 31);
  }
  return m;
}

// n_obj: a multiple of 192 (whole trips of every row)
template <int MODE, int PUSH>
__global__ __launch_bounds__(256) void k(const float* tab, int n_obj, int iters, const float* rays, unsigned* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const float nx = rays[(t & 1023) * 4 + 0], nz = rays[(t & 1023) * 4 + 1], c0 = rays[(t & 1023) * 4 + 2], T = rays[(t & 1023) * 4 + 3];
  unsigned m = 0, acc = 0;
  cfptr base = (cfptr)(uintptr_t)tab;
  for (int it = 0; it < iters; ++it) {
    cfptr rec = base;
    if (MODE == 3) {  // d, g
      f16v b;
#pragma unroll
      for (int j = 0; j < 16; ++j) b[j] = rec[j];
      for (int i = 0; i < n_obj; i += 32) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float c = c0;
          asm volatile("" : "+v"(c));  // (or the compiler hoists the three float32 instructions out of the loop)
          m = group<PUSH>(m, nx, nz, c, T, b);
        }
        acc += m;
        asm volatile("" : "+v"(m));
      }
    } else if (MODE == 0 || MODE == 4) {  // a, e, h
      float n0 = rec[0], n1 = rec[1];
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
      for (int i = 0; i < n_obj; i += 64) {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
#pragma unroll
          for (int j = 0; j < 32; ++j) {
            const float cx = n0, cz = n1;
            n0 = rec[2 * (j + 1)]; n1 = rec[2 * (j + 1) + 1];
            if (MODE == 4) m = __builtin_amdgcn_alignbit(m, __float_as_uint(cx) ^ __float_as_uint(cz), 31);
            else m = obj<PUSH>(m, nx, nz, c0, T, cx, cz);
            __builtin_amdgcn_sched_barrier(0);  // one object after the other, each request one object ahead: as integrate_kernel's register budget makes the compiler schedule them
          }
          rec += 64;
          acc += m;
          asm volatile("" : "+v"(m));
        }
      }
    } else if (MODE == 1 || MODE == 5) {  // b, f, i
      const f2v nx2 = {nx, nx}, nz2 = {nz, nz}, c02 = {c0, c0}, negT2 = {-T, -T};
      auto grp = [&](const f16v& b) { m = MODE == 5 ? group_pk(m, nx2, nz2, c02, negT2, b) : group<PUSH>(m, nx, nz, c0, T, b); };
      f16v A, B;
      FEED_REQ(A, rec, 0);
#pragma unroll 1
      for (int i = 0; i < n_obj; i += 64) {
        FEED_WAIT_REQ(A, 0, B, rec, 64); grp(A);
        FEED_WAIT_REQ(B, 0, A, rec, 128); grp(B);
        FEED_WAIT_REQ(A, 0, B, rec, 192); grp(A);
        FEED_WAIT_REQ(B, 0, A, rec, 256); grp(B);
        acc += m;
        FEED_WAIT_REQ(A, 0, B, rec, 320); grp(A);
        FEED_WAIT_REQ(B, 0, A, rec, 384); grp(B);
        FEED_WAIT_REQ(A, 0, B, rec, 448); grp(A);
        FEED_WAIT_REQ(B, 0, A, rec, 512); grp(B);
        acc += m;
        rec += 128;
      }
      FEED_WAIT(A, 0);  // the request behind the list: nobody reads it, but its registers are the compiler's again only now
    } else if (MODE == 2) {  // c
      f16v A, B, C;
      FEED_REQ(A, rec, 0);
      FEED_REQ(B, rec, 64);
#pragma unroll 1
      for (int i = 0; i < n_obj; i += 96) {
        FEED_WAIT_REQ(A, 1, C, rec, 128); m = group<PUSH>(m, nx, nz, c0, T, A);
        FEED_WAIT_REQ(B, 1, A, rec, 192); m = group<PUSH>(m, nx, nz, c0, T, B);
        FEED_WAIT_REQ(C, 1, B, rec, 256); m = group<PUSH>(m, nx, nz, c0, T, C);
        FEED_WAIT_REQ(A, 1, C, rec, 320); m = group<PUSH>(m, nx, nz, c0, T, A);
        acc += m;
        FEED_WAIT_REQ(B, 1, A, rec, 384); m = group<PUSH>(m, nx, nz, c0, T, B);
        FEED_WAIT_REQ(C, 1, B, rec, 448); m = group<PUSH>(m, nx, nz, c0, T, C);
        FEED_WAIT_REQ(A, 1, C, rec, 512); m = group<PUSH>(m, nx, nz, c0, T, A);
        FEED_WAIT_REQ(B, 1, A, rec, 576); m = group<PUSH>(m, nx, nz, c0, T, B);
        acc += m;
        FEED_WAIT_REQ(C, 1, B, rec, 640); m = group<PUSH>(m, nx, nz, c0, T, C);
        FEED_WAIT_REQ(A, 1, C, rec, 704); m = group<PUSH>(m, nx, nz, c0, T, A);
        FEED_WAIT_REQ(B, 1, A, rec, 768); m = group<PUSH>(m, nx, nz, c0, T, B);
        FEED_WAIT_REQ(C, 1, B, rec, 832); m = group<PUSH>(m, nx, nz, c0, T, C);
        acc += m;
        rec += 192;
      }
      FEED_WAIT(A, 0);
      FEED_WAIT(B, 0);
    } else {  // p0-p4 (PUSH: the instruction): 4 x 8 x 15 = n_obj instructions per pass
      float a0 = nx, a1 = nz, a2 = c0, a3 = T;
      unsigned u0 = m, u1 = m + 1, u2 = m + 2, u3 = m + 3;
      unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
      for (int i = 0; i < n_obj; i += 32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (PUSH == 0) asm volatile("v_fma_f32 %0, %4, %5, %0\n\tv_fma_f32 %1, %4, %5, %1\n\tv_fma_f32 %2, %4, %5, %2\n\tv_fma_f32 %3, %4, %5, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(nx), "v"(nz));
          if (PUSH == 1) asm volatile("v_sub_f32_e64 %0, |%0|, %4\n\tv_sub_f32_e64 %1, |%1|, %4\n\tv_sub_f32_e64 %2, |%2|, %4\n\tv_sub_f32_e64 %3, |%3|, %4" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(T));
          if (PUSH == 2) asm volatile("v_alignbit_b32 %0, %0, %4, 31\n\tv_alignbit_b32 %1, %1, %4, 31\n\tv_alignbit_b32 %2, %2, %4, 31\n\tv_alignbit_b32 %3, %3, %4, 31" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3) : "v"(nx));
          if (PUSH == 3) asm volatile("v_cmp_lt_f32_e64 %0, |%4|, %5\n\tv_cmp_lt_f32_e64 %1, |%5|, %4\n\tv_cmp_lt_f32_e64 %2, |%4|, %6\n\tv_cmp_lt_f32_e64 %3, |%6|, %4" : "=s"(s0), "=s"(s1), "=s"(s2), "=s"(s3) : "v"(a0), "v"(a1), "v"(a2));
          if (PUSH == 4) asm volatile("v_addc_co_u32_e64 %0, %4, %0, %0, %4\n\tv_addc_co_u32_e64 %1, %5, %1, %1, %5\n\tv_addc_co_u32_e64 %2, %6, %2, %2, %6\n\tv_addc_co_u32_e64 %3, %7, %3, %3, %7"
                                      : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3));
        }
      }
      acc += __float_as_uint(a0 + a1 + a2 + a3) + u0 + u1 + u2 + u3 + (unsigned)(s0 ^ s1 ^ s2 ^ s3);
    }
  }
  out[t] = acc;
}

static const int kNObj = 384;                       // 12 whole words
static const int kSlackFloats = 64;                 // behind the table: row c reads 32 floats past it
static const size_t kLdsBytes[4] = {0, 96 * 1024, 64 * 1024, 48 * 1024};  // 1 / 2 / 3 workgroups fit in a CU's 160 KB

template <int MODE, int PUSH>
void run(const char* name, const float* tab, const float* rays, unsigned* out, int cus, FILE* f) {
  const int iters = 2000, rounds = 4, reps = 3;
  (void)hipFuncSetAttribute((const void*)k<MODE, PUSH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes[1]);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  char line[512];
  int at = snprintf(line, sizeof line, "%-46s", name);
  unsigned sum = 0;
  for (int w = 1; w <= 3; ++w) {
    const int grid = cus * w * rounds;
    hipLaunchKernelGGL((k<MODE, PUSH>), dim3(grid), dim3(256), kLdsBytes[w], 0, tab, kNObj, 50, rays, out);
    if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "launch failed: %s\n", hipGetErrorString(hipGetLastError())); exit(1); }
    float ms[reps];
    for (int r = 0; r < reps; ++r) {
      (void)hipEventRecord(e0);
      hipLaunchKernelGGL((k<MODE, PUSH>), dim3(grid), dim3(256), kLdsBytes[w], 0, tab, kNObj, iters, rays, out);
      (void)hipEventRecord(e1);
      if (hipEventSynchronize(e1) != hipSuccess) { fprintf(stderr, "kernel failed: %s\n", hipGetErrorString(hipGetLastError())); exit(1); }
      (void)hipEventElapsedTime(&ms[r], e0, e1);
    }
    std::sort(ms, ms + reps);
    // a SIMD hosts w waves at a time, `rounds` of them one after the other: SIMD time per object (instruction) and wave
    const double per = 1e6 / ((double)rounds * iters * kNObj * w);
    at += snprintf(line + at, sizeof line - at, "  | %5.2f (%5.2f..%5.2f) %6.2f", ms[1] * per, ms[0] * per, ms[reps - 1] * per, ms[1] * per * w);
    if (w == 3) {
      std::vector<unsigned> h(1024);
      (void)hipMemcpy(h.data(), out, 1024 * 4, hipMemcpyDeviceToHost);
      for (unsigned v : h) sum = sum * 31u + v;
    }
  }
  snprintf(line + at, sizeof line - at, "  | %08x", sum);
  printf("%s\n", line); fflush(stdout);
  if (f) { fprintf(f, "%s\n", line); fflush(f); }
}

int main(int argc, char** argv) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { fprintf(stderr, "no device\n"); return 1; }
  FILE* f = argc > 1 ? fopen(argv[1], "w") : nullptr;
  std::vector<float> tab(2 * kNObj + kSlackFloats, 0x1p100f), tab_pk(2 * kNObj + kSlackFloats, 0x1p100f), rays(4096);
  for (int i = 0; i < kNObj; ++i) {
    const float cx = -11.0f + 22.0f * ((i * 37) % 101) / 101.0f, cz = -11.0f + 22.0f * ((i * 53) % 103) / 103.0f;
    tab[2 * i] = cx; tab[2 * i + 1] = cz;
    tab_pk[4 * (i / 2) + (i & 1)] = cx; tab_pk[4 * (i / 2) + 2 + (i & 1)] = cz;  // {cxA, cxB, czA, czB}
  }
  // (a band of 2.0 around tracks 0.05 apart: a fifth of the objects kept, so that the checksum has something to say)
  for (int i = 0; i < 1024; ++i) { rays[4 * i] = 0.6f; rays[4 * i + 1] = 0.8f; rays[4 * i + 2] = 0.05f * (i - 512); rays[4 * i + 3] = 2.0f; }
  float *d_tab, *d_tab_pk, *d_rays; unsigned* d_out;
  const int cus = prop.multiProcessorCount;
  (void)hipMalloc(&d_tab, tab.size() * 4); (void)hipMalloc(&d_tab_pk, tab.size() * 4); (void)hipMalloc(&d_rays, rays.size() * 4);
  (void)hipMalloc(&d_out, (size_t)cus * 3 * 4 * 256 * 4);
  (void)hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice); (void)hipMemcpy(d_tab_pk, tab_pk.data(), tab.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(d_rays, rays.data(), rays.size() * 4, hipMemcpyHostToDevice);
  char head[640];
  snprintf(head, sizeof head, "%d CUs, %d MHz; ns per object (p rows: per instruction) and wave of SIMD time, median (min..max) of 3, then ns per object as one wave sees it, at 1 | 2 | 3 waves per SIMD; checksum\n"
           "floors: pipe (8 cycles per object) 3.33 | 3.33 | 3.33; one wave's issue rate (16 cycles per object) 6.67 | 3.33 | 2.22; scalar bytes: row e",
           cus, prop.clockRate / 1000);
  printf("%s\n", head); if (f) fprintf(f, "%s\n", head);
  run<0, 0>("a  as compiled (request one object ahead)", d_tab, d_rays, d_out, cus, f);
  run<1, 0>("b  request one group of 8 ahead (2 buffers)", d_tab, d_rays, d_out, cus, f);
  run<2, 0>("c  two groups ahead (3 buffers, lgkmcnt(1))", d_tab, d_rays, d_out, cus, f);
  run<3, 0>("d  loop-invariant operands, no loads", d_tab, d_rays, d_out, cus, f);
  run<4, 0>("e  loads + v_alignbit only", d_tab, d_rays, d_out, cus, f);
  run<5, 0>("f  b's feed, v_pk_fma_f32 on object pairs", d_tab_pk, d_rays, d_out, cus, f);
  run<3, 1>("g  d with v_cmp_lt_f32 + v_addc_co_u32", d_tab, d_rays, d_out, cus, f);
  run<0, 1>("h  a with v_cmp_lt_f32 + v_addc_co_u32", d_tab, d_rays, d_out, cus, f);
  run<1, 1>("i  b with v_cmp_lt_f32 + v_addc_co_u32", d_tab, d_rays, d_out, cus, f);
  run<6, 0>("p0 v_fma_f32 alone", d_tab, d_rays, d_out, cus, f);
  run<6, 1>("p1 v_sub_f32_e64 |v| alone", d_tab, d_rays, d_out, cus, f);
  run<6, 2>("p2 v_alignbit_b32 alone", d_tab, d_rays, d_out, cus, f);
  run<6, 3>("p3 v_cmp_lt_f32_e64 |v| (to an SGPR pair) alone", d_tab, d_rays, d_out, cus, f);
  run<6, 4>("p4 v_addc_co_u32_e64 alone", d_tab, d_rays, d_out, cus, f);
  if (f) fclose(f);
  return 0;
}
