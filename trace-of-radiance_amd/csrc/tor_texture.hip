// tor_texture.hip -- the surface-texture query for host integrators (tor_texture_eval_device and the blocking _host twin,
// tor_scene_textures, tor_texture_info; include/tor_texture.h): for each listed hit record the colour of the surface there -- a
// constant, a 3-D checker in world or normal space, or an octahedral image looked up by the record's outward normal, nearest or
// bilinear with the fold's seam rule -- or, for an object without a texture, the attenuation tor_bounce_device gives a scattered
// ray.  include/tor_texture.h holds the definition, operation by operation; texture_kernel follows it line by line.
//
// One record per lane, 256-thread blocks, no LDS, no scratch, no atomics; a lane without an item returns before its first load.
// Per lane: word 7 of the hit record (object, front_face), the binding, then either the cold record's words 13 and 9..11
// (untextured: the by-ORIGINAL-index buffer bsdf_kernel reads) or the texture record, words 3..5 of the hit record (the normal)
// and, for a WORLD checker alone, words 0..2 (p).  The atlas is the library's own copy, padded to 4 float64 per texel so that a
// texel is two aligned 16-byte loads; the four corners of a bilinear lookup are all requested before the first is used.  Every
// texel index is clamped into [0, n - 1] per axis as the last step before it is formed (texel_at).
//
// Float64, unfused (-ffp-contract=off), correctly rounded `/`.  Stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/tor_texture.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"

static_assert(sizeof(TorTexture) == 96 && offsetof(TorTexture, offset) == 16 && offsetof(TorTexture, a) == 24 &&
                  offsetof(TorTexture, b) == 48 && offsetof(TorTexture, freq) == 72,
              "TorTexture as include/tor_texture.h and the Python binding lay it out");
static_assert(sizeof(TorHit) == 64 && offsetof(TorHit, normal) == 24 && offsetof(TorHit, object) == 56 && offsetof(TorHit, front_face) == 60,
              "p is words 0..2, normal words 3..5, object and front_face the halves of word 7");

namespace tor {
namespace {

constexpr int kTexThreads = 256;
constexpr int kTexelWords = 4;  // float64 per texel of the device atlas: R, G, B, 0

struct TParams {
  const double* hits;      // 8 float64 words per record (TorHit)
  const int* list;         // the records to answer, or null: entry e is record e
  long long n_list, n;
  const double* obj_cold;  // the cold records by ORIGINAL index, 16 float64 per object
  long long n_objects;
  const int* binding;      // n_objects int32: the texture of every object, or -1
  const TorTexture* table; // n_textures records
  int n_textures;
  const double* atlas;     // kTexelWords float64 per texel
  double* color;           // 3 float64 per record
  int* texel;              // one int32 per record, or null
};

struct Texel {
  double r, g, b;
};

__device__ __forceinline__ void write_tex(const TParams& P, long long i, double r, double g, double b, int texel) {
  double* c = P.color + 3 * i;
  c[0] = r; c[1] = g; c[2] = b;
  if (P.texel) P.texel[i] = texel;
}

__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

// the texel (r, c) of the n x n image at `base`: both indices clamped LAST, so the two 16-byte loads are inside the image whatever
// r and c hold
__device__ __forceinline__ Texel texel_at(const double* base, int n, int r, int c) {
  const int rr = clamp_index(r, n), cc = clamp_index(c, n);
  const double2* t = (const double2*)(base + (size_t)kTexelWords * ((size_t)rr * (size_t)n + (size_t)cc));
  const double2 lo = t[0], hi = t[1];
  return Texel{lo.x, lo.y, hi.x};
}

// tor_env.h's clamped floor
__device__ __forceinline__ int tex_cell(double w, double nd, int n) {
  const double f = __builtin_floor((w + 1.0) * (0.5 * nd));
  return f > 0.0 ? (f < (double)(n - 1) ? (int)f : n - 1) : 0;
}

// a bilinear floor as an int in [-1, n - 1]
__device__ __forceinline__ int tex_floor(double f, int n) {
  if (!(f >= -1.0)) return -1;
  if (f > (double)(n - 1)) return n - 1;
  return (int)f;
}

// tor_texture.h's seam rule
__device__ __forceinline__ void seam(int n, int& r, int& c) {
  if (c < 0 || c > n - 1) {
    r = (n - 1) - r;
    c = clamp_index(c, n);
  }
  if (r < 0 || r > n - 1) {
    c = (n - 1) - c;
    r = clamp_index(r, n);
  }
}

__global__ __launch_bounds__(kTexThreads) void texture_kernel(const TParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n, (long long)blockIdx.x * kTexThreads + threadIdx.x);
  if (i < 0) return;
  const double* h = P.hits + 8 * i;
  const unsigned long long w7 = (unsigned long long)__double_as_longlong(h[7]);
  const long long object = (long long)(int)(unsigned)(w7 & 0xffffffffull);
  if (object < 0 || object >= P.n_objects) {  // no such object
    write_tex(P, i, 0.0, 0.0, 0.0, -1);
    return;
  }
  const int bound = P.binding[object];
  if (bound < 0 || bound >= P.n_textures) {  // no texture (the host admits -1 and table indices only): the scatter's attenuation
    const qgdptr c = (qgdptr)(uintptr_t)(P.obj_cold + 16 * (size_t)object);
    const int mat = ((int)__double_as_longlong(c[13]) >> 8) & 0xff;
    if (mat == kLambertian || mat == kMetal) write_tex(P, i, c[9], c[10], c[11], -1);
    else write_tex(P, i, 1.0, 1.0, 1.0, -1);
    return;
  }
  const TorTexture* T = P.table + bound;
  const int kind = T->kind, option = T->option;
  if (kind == TOR_TEXTURE_CONSTANT) {
    write_tex(P, i, T->a[0], T->a[1], T->a[2], 0);
    return;
  }
  const bool front = (unsigned)(w7 >> 32) != 0u;
  double mx = h[3], my = h[4], mz = h[5];
  if (!front) {
    mx = -mx; my = -my; mz = -mz;
  }
  if (kind == TOR_TEXTURE_CHECKER) {
    double x = mx, y = my, z = mz;
    if (option == TOR_TEXTURE_WORLD) {
      x = h[0]; y = h[1]; z = h[2];
    }
    const double fx = __builtin_floor(x * T->freq[0]), fy = __builtin_floor(y * T->freq[1]), fz = __builtin_floor(z * T->freq[2]);
    const double big = 4503599627370496.0;  // 2^52
    if (!(__builtin_fabs(fx) < big) || !(__builtin_fabs(fy) < big) || !(__builtin_fabs(fz) < big)) {
      write_tex(P, i, T->a[0], T->a[1], T->a[2], -1);
      return;
    }
    const double px = fx - 2.0 * __builtin_floor(fx * 0.5), py = fy - 2.0 * __builtin_floor(fy * 0.5),
                 pz = fz - 2.0 * __builtin_floor(fz * 0.5);
    const int odd = ((int)px + (int)py + (int)pz) & 1;
    const double* col = odd ? T->b : T->a;
    write_tex(P, i, col[0], col[1], col[2], odd);
    return;
  }
  // IMAGE: tor_env.h's encode of m
  int n = T->side;
  if (n < 1) n = 1;  // (the host admits 1 .. TOR_TEXTURE_MAX_SIDE)
  const double nd = (double)n;
  const double L1 = __builtin_fabs(mx) + __builtin_fabs(my) + __builtin_fabs(mz);
  if (!((L1 > 0.0) && (L1 < __builtin_inf()))) {
    write_tex(P, i, 0.0, 0.0, 0.0, -1);
    return;
  }
  const double qx = mx / L1, qz = mz / L1;
  double s = qx, t = qz;
  if (!(my >= 0.0)) {
    s = __builtin_copysign(1.0 - __builtin_fabs(qz), qx);
    t = __builtin_copysign(1.0 - __builtin_fabs(qx), qz);
  }
  const int cn = tex_cell(s, nd, n), rn = tex_cell(t, nd, n);
  const double* base = P.atlas + (size_t)kTexelWords * (size_t)T->offset;
  if (option != TOR_TEXTURE_BILINEAR) {
    const Texel x = texel_at(base, n, rn, cn);
    write_tex(P, i, x.r, x.g, x.b, rn * n + cn);
    return;
  }
  const double u = (s + 1.0) * (0.5 * nd) - 0.5, v = (t + 1.0) * (0.5 * nd) - 0.5;
  const double fc = __builtin_floor(u), fr = __builtin_floor(v);
  const double al = u - fc, be = v - fr;
  const int c0 = tex_floor(fc, n), r0 = tex_floor(fr, n);
  int ra = r0, ca = c0, rb = r0, cb = c0 + 1, rc = r0 + 1, cc = c0, rd = r0 + 1, cd = c0 + 1;
  seam(n, ra, ca);
  seam(n, rb, cb);
  seam(n, rc, cc);
  seam(n, rd, cd);
  // the four corners, requested before the first is used
  const Texel t00 = texel_at(base, n, ra, ca), t01 = texel_at(base, n, rb, cb), t10 = texel_at(base, n, rc, cc),
              t11 = texel_at(base, n, rd, cd);
  const double ia = 1.0 - al, ib = 1.0 - be;
  const double R = ((ia * t00.r + al * t01.r) * ib) + ((ia * t10.r + al * t11.r) * be);
  const double G = ((ia * t00.g + al * t01.g) * ib) + ((ia * t10.g + al * t11.g) * be);
  const double B = ((ia * t00.b + al * t01.b) * ib) + ((ia * t10.b + al * t11.b) * be);
  write_tex(P, i, R, G, B, rn * n + cn);
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: tor_bsdf_eval_device's, then the NULL arrays; then the scene and the table
int texture_check(const char* who, TorContext* ctx, int64_t n, const void* list, int64_t n_list, bool nulls) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL hits or color");
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  if (ctx->hitq.n_textures <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no texture table (tor_scene_textures)");
  return TOR_OK;
}

// the launch; the arguments are checked, n > 0 and n_list > 0
int texture_launch(const char* who, TorContext* ctx, int64_t n, const void* d_hits, const int32_t* d_list, int64_t n_list, double* d_color,
                   int32_t* d_texel, hipStream_t stream) {
  int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the query reads the by-object records and the table)
  if (rc == TOR_OK) rc = tor::ensure_obj_cold(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  const tor::HitQueryState& hq = ctx->hitq;
  tor::TParams P{};
  P.hits = (const double*)d_hits;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n = (long long)n;
  P.obj_cold = (const double*)hq.obj_cold.ptr;
  P.n_objects = (long long)ctx->n_objects;
  P.binding = (const int*)hq.tex_binding.ptr;
  P.table = (const TorTexture*)hq.tex_table.ptr;
  P.n_textures = (int)hq.n_textures;
  P.atlas = (const double*)hq.tex_atlas.ptr;
  P.color = d_color;
  P.texel = d_texel;
  const unsigned grid = (unsigned)((n_list + tor::kTexThreads - 1) / tor::kTexThreads);
  hipLaunchKernelGGL(tor::texture_kernel, dim3(grid), dim3(tor::kTexThreads), 0, stream, P);
  rc = tor::query_done(ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::set_last_note("texture eval");
  return TOR_OK;
}

bool bad_colour(const double* c) {
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(c[k]) || c[k] < 0.0) return true;
  return false;
}

}  // namespace

extern "C" {

int tor_scene_textures(TorContext* ctx, int64_t n_textures, const TorTexture* table, int64_t n_objects, const int32_t* binding,
                       int64_t n_texels, const double* texels) {
  using tor::fail;
  const std::string w = "tor_scene_textures";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  if (n_textures < 0 || n_textures > TOR_TEXTURE_MAX)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_textures <= TOR_TEXTURE_MAX (" + std::to_string((int)TOR_TEXTURE_MAX) + ")");
  if (n_objects != ctx->n_objects)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": n_objects must be the uploaded list's length (" + std::to_string(ctx->n_objects) + ")");
  if (n_texels < 0 || n_texels > TOR_TEXTURE_MAX_TEXELS)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_texels <= TOR_TEXTURE_MAX_TEXELS (" + std::to_string((int)TOR_TEXTURE_MAX_TEXELS) + ")");
  tor::HitQueryState& hq = ctx->hitq;
  if (n_textures == 0) {  // clear: the buffers stay for the next table
    HIP_TRY(hipSetDevice(ctx->device));
    if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));
    hq.n_textures = hq.n_texels = hq.tex_bound = 0;
    return TOR_OK;
  }
  if (!table || (n_objects > 0 && !binding)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": table or binding is NULL");
  if (n_texels > 0 && !texels) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": texels is NULL");
  for (int64_t j = 0; j < n_textures; ++j) {
    const TorTexture& t = table[j];
    const std::string at = w + ": table[" + std::to_string(j) + "]";
    if (t.kind != TOR_TEXTURE_CONSTANT && t.kind != TOR_TEXTURE_CHECKER && t.kind != TOR_TEXTURE_IMAGE)
      return fail(TOR_ERR_INVALID_ARGUMENT, at + ": unknown kind");
    if (t.kind != TOR_TEXTURE_CONSTANT && t.option != 0 && t.option != 1) return fail(TOR_ERR_INVALID_ARGUMENT, at + ": unknown option");
    if (t.kind == TOR_TEXTURE_IMAGE) {
      if (t.side < 1 || t.side > TOR_TEXTURE_MAX_SIDE)
        return fail(TOR_ERR_INVALID_ARGUMENT, at + ": side outside [1, " + std::to_string((int)TOR_TEXTURE_MAX_SIDE) + "]");
      if (t.offset < 0 || t.offset > n_texels || (int64_t)t.side * t.side > n_texels - t.offset)
        return fail(TOR_ERR_INVALID_ARGUMENT, at + ": the image does not lie inside the atlas");
      continue;
    }
    if (bad_colour(t.a) || (t.kind == TOR_TEXTURE_CHECKER && bad_colour(t.b)))
      return fail(TOR_ERR_INVALID_ARGUMENT, at + ": colours must be finite and >= 0");
    if (t.kind == TOR_TEXTURE_CHECKER && (!std::isfinite(t.freq[0]) || !std::isfinite(t.freq[1]) || !std::isfinite(t.freq[2])))
      return fail(TOR_ERR_INVALID_ARGUMENT, at + ": freq must be finite");
  }
  int64_t bound = 0;
  for (int64_t j = 0; j < n_objects; ++j) {
    if (binding[j] < -1 || binding[j] >= n_textures)
      return fail(TOR_ERR_INVALID_ARGUMENT, w + ": binding[" + std::to_string(j) + "] is outside [-1, n_textures)");
    bound += binding[j] >= 0 ? 1 : 0;
  }
  for (int64_t k = 0; k < n_texels * 3; ++k)
    if (!std::isfinite(texels[k]) || texels[k] < 0.0) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": texels must be finite and >= 0");
  // the library's copies: the table as given, the atlas padded to 4 float64 per texel
  // (up to 128 MB of host memory: a failed allocation is a status, never an exception across the C ABI)
  std::vector<double> atlas;
  try {
    atlas.assign((size_t)n_texels * tor::kTexelWords, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(TOR_ERR_OUT_OF_MEMORY, w + ": no host memory for the padded atlas");
  }
  for (int64_t k = 0; k < n_texels; ++k)
    for (int ch = 0; ch < 3; ++ch) atlas[(size_t)k * tor::kTexelWords + ch] = texels[(size_t)k * 3 + ch];
  HIP_TRY(hipSetDevice(ctx->device));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the table
  hq.n_textures = 0;  // (a failed allocation or copy leaves no table rather than half of one)
  HIP_TRY(hq.tex_table.ensure((size_t)n_textures * sizeof(TorTexture)));
  HIP_TRY(hq.tex_binding.ensure((size_t)(n_objects > 0 ? n_objects : 1) * 4));
  HIP_TRY(hq.tex_atlas.ensure((atlas.empty() ? (size_t)tor::kTexelWords : atlas.size()) * 8));
  HIP_TRY(hipMemcpy(hq.tex_table.ptr, table, (size_t)n_textures * sizeof(TorTexture), hipMemcpyHostToDevice));
  if (n_objects > 0) HIP_TRY(hipMemcpy(hq.tex_binding.ptr, binding, (size_t)n_objects * 4, hipMemcpyHostToDevice));
  if (!atlas.empty()) HIP_TRY(hipMemcpy(hq.tex_atlas.ptr, atlas.data(), atlas.size() * 8, hipMemcpyHostToDevice));
  hq.n_textures = n_textures;
  hq.n_texels = n_texels;
  hq.tex_bound = bound;
  return TOR_OK;
}

int tor_texture_info(TorContext* ctx, int64_t* out) {
  if (!ctx || !out) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_texture_info: NULL argument");
  const tor::HitQueryState& hq = ctx->hitq;
  const bool any = hq.n_textures > 0;
  out[0] = any ? hq.n_textures : 0;
  out[1] = any ? hq.n_texels : 0;
  out[2] = any ? hq.tex_bound : 0;
  return TOR_OK;
}

int tor_texture_eval_device(TorContext* ctx, int64_t n_hits, const TorHit* d_hits, const int32_t* d_list, int64_t n_list, double* d_color,
                            int32_t* d_texel, void* hip_stream) {
  const char* who = "tor_texture_eval_device";
  const int rc = texture_check(who, ctx, n_hits, d_list, n_list, !d_hits || !d_color);
  if (rc != TOR_OK || n_hits == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return texture_launch(who, ctx, n_hits, d_hits, d_list, n_list, d_color, d_texel, (hipStream_t)hip_stream);
}

int tor_texture_eval_host(TorContext* ctx, int64_t n_hits, const TorHit* hits, const int32_t* list, int64_t n_list, double* color,
                          int32_t* texel) {
  const char* who = "tor_texture_eval_host";
  int rc = texture_check(who, ctx, n_hits, list, n_list, !hits || !color);
  if (rc != TOR_OK || n_hits == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too, records that are not listed keep what the caller holds --, the query on the default stream,
  // the outputs back
  const size_t m = (size_t)n_hits;
  tor::HostPart st[4] = {{hits, m * sizeof(TorHit), true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {color, m * 24, true, true},
                         {texel, texel ? m * 4 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 4);
  if (rc != TOR_OK) return rc;
  rc = texture_launch(who, ctx, n_hits, st[0].dev, st[1].as<const int32_t>(), n_list, st[2].as<double>(), st[3].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 4);
}

}  // extern "C"
