// tor_bsdf.hip -- the BSDF query for host integrators (tor_bsdf_eval_device and the blocking _host twin, include/tor_bsdf.h): for
// each listed item (incoming direction, hit record, outgoing direction) the solid-angle density rec.material.scatter
// (materials.nim:21-96, tor_shade_scatter.inc) gives the outgoing direction, the value albedo * density and the kind of the
// answer, on gfx950 -- what next-event estimation and multiple importance sampling need at a Lambertian or a fuzzy Metal vertex.
// include/tor_bsdf.h holds the definition, operation by operation; bsdf_kernel follows it line by line.
//
// One item per lane, 256-thread blocks, no LDS, no scratch; a lane without an item returns before its first load.  Of the three
// strided records only the words the header names are loaded: direction (words 3..5) of the two rays, normal (3..5) and word 7 of
// the hit record.  The object's cold record (tor_kernels.hpp; by ORIGINAL index, the buffer tor_scatter_device looks the
// material up in) is gathered per lane -- the index is not wave-uniform, so these are vector loads: word 13 (flags), then
// 9..12 (albedo, fuzz) for the kinds that have a density.
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

#include "../../include/tor_bsdf.h"
#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"

static_assert(sizeof(TorRay) == 56 && sizeof(TorHit) == 64, "TorRay / TorHit as the kernel indexes them");
static_assert(offsetof(TorRay, direction) == 24 && offsetof(TorHit, normal) == 24 && offsetof(TorHit, object) == 56,
              "direction and normal are words 3..5, object the low half of word 7");

namespace tor {
namespace {

constexpr int kBsdfThreads = 256;
constexpr double kPi = 3.141592653589793;  // Nim's PI

struct FParams {
  const double* in;        // 7 float64 per item (TorRay): the incoming ray, direction read
  const double* hits;      // 8 float64 words per item (TorHit): normal and object read
  const double* out;       // 7 float64 per item (TorRay): the outgoing ray, direction read
  const int* list;         // the items to answer, or null: entry e is item e
  long long n_list, n;
  const double* obj_cold;  // the cold records by ORIGINAL index, 16 float64 per object
  long long n_objects;
  double* value;           // 3 float64 per item
  double* pdf;             // one float64 per item
  int* kind;               // one int32 per item (TOR_BSDF_*), or null
};

__device__ __forceinline__ void write_eval(const FParams& P, long long i, double vx, double vy, double vz, double pdf, int kind) {
  double* v = P.value + 3 * i;
  v[0] = vx; v[1] = vy; v[2] = vz;
  P.pdf[i] = pdf;
  if (P.kind) P.kind[i] = kind;
}

// tor_bsdf.h "Metal": the density of unit(r + f B) at w, r = reflect(unit(in), n)
__device__ __forceinline__ double metal_density(V3 w, V3 d_in, V3 n, double fuzz) {
  const V3 ud = unit_vector(d_in);  // materials.nim:40
  const V3 r = reflect(ud, n);      // rays.nim:27-28
  const double f = __builtin_fabs(fuzz);
  const double b = dot(w, r);
  const V3 x = v3(w.y * r.z - w.z * r.y, w.z * r.x - w.x * r.z, w.x * r.y - w.y * r.x);  // vec3s.nim:100-104
  const double s2 = dot(x, x);
  const double h = f * f - s2;
  if (!(h > 0.0)) return 0.0;
  const double q = __builtin_sqrt(h);
  const double lo = b - q, hi = b + q;
  const double f3 = f * f * f;
  if (lo > 0.0) return (q * (3.0 * b * b + h)) / (2.0 * kPi * f3);
  if (hi > 0.0) return (hi * hi * hi) / (4.0 * kPi * f3);
  return 0.0;
}

__global__ __launch_bounds__(kBsdfThreads) void bsdf_kernel(const FParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n, (long long)blockIdx.x * kBsdfThreads + threadIdx.x);
  if (i < 0) return;
  const double* h = P.hits + 8 * i;
  const unsigned long long w7 = (unsigned long long)__double_as_longlong(h[7]);
  const long long object = (long long)(int)(unsigned)(w7 & 0xffffffffull);
  if (object < 0 || object >= P.n_objects) {  // no such object: tor_scatter_device's miss
    write_eval(P, i, 0.0, 0.0, 0.0, 0.0, TOR_BSDF_NONE);
    return;
  }
  const qgdptr c = (qgdptr)(uintptr_t)(P.obj_cold + 16 * (size_t)object);
  const int mat = ((int)__double_as_longlong(c[13]) >> 8) & 0xff;
  const double fuzz = c[12];  // (a Dielectric's word 12 is its refraction index: not used)
  if (mat != kLambertian && !(mat == kMetal && fuzz != 0.0)) {  // Dielectric, a mirror: Dirac
    write_eval(P, i, 0.0, 0.0, 0.0, 0.0, TOR_BSDF_DELTA);
    return;
  }
  const V3 albedo = v3(c[9], c[10], c[11]);
  const double* po = P.out + 7 * i;
  const V3 out = v3(po[3], po[4], po[5]);
  const V3 n = v3(h[3], h[4], h[5]);
  const double oo = dot(out, out);
  double pdf = 0.0;
  if ((oo > 0.0) && (oo < __builtin_inf())) {
    const V3 w = out * (1.0 / __builtin_sqrt(oo));  // unit_vector(out), vec3s.nim:106-107
    if (dot(out, n) > 0.0) {  // the scatter's own test, on the unnormalised direction
      if (mat == kLambertian) {
        const double cs = dot(w, n);
        pdf = (cs > 0.0) ? cs / kPi : 0.0;
      } else {
        const double* pin = P.in + 7 * i;
        pdf = metal_density(w, v3(pin[3], pin[4], pin[5]), n, fuzz);
      }
    }
  }
  write_eval(P, i, albedo.x * pdf, albedo.y * pdf, albedo.z * pdf, pdf, TOR_BSDF_DENSITY);
}

}  // namespace
}  // namespace tor

namespace {

// the checks that need no device and do not read *ctx: tor_light_pdf_device's, then the NULL arrays; then the scene
int bsdf_check(const char* who, TorContext* ctx, int64_t n, const void* list, int64_t n_list, bool nulls) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL in, hits, out, value or pdf");
  return tor::scene_args(who, ctx);
}

// the launch; the arguments are checked, n > 0 and n_list > 0
int bsdf_launch(const char* who, TorContext* ctx, int64_t n, const void* d_in, const void* d_hits, const void* d_out, const int32_t* d_list,
                int64_t n_list, double* d_value, double* d_pdf, int32_t* d_kind, hipStream_t stream) {
  int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the query reads the by-object records alone)
  if (rc == TOR_OK) rc = tor::ensure_obj_cold(who, ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::FParams P{};
  P.in = (const double*)d_in;
  P.hits = (const double*)d_hits;
  P.out = (const double*)d_out;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n = (long long)n;
  P.obj_cold = (const double*)ctx->hitq.obj_cold.ptr;
  P.n_objects = (long long)ctx->n_objects;
  P.value = d_value;
  P.pdf = d_pdf;
  P.kind = d_kind;
  const unsigned grid = (unsigned)((n_list + tor::kBsdfThreads - 1) / tor::kBsdfThreads);
  hipLaunchKernelGGL(tor::bsdf_kernel, dim3(grid), dim3(tor::kBsdfThreads), 0, stream, P);
  rc = tor::query_done(ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::set_last_note("bsdf eval");
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_bsdf_eval_device(TorContext* ctx, int64_t n, const TorRay* d_in, const TorHit* d_hits, const TorRay* d_out, const int32_t* d_list,
                         int64_t n_list, double* d_value, double* d_pdf, int32_t* d_kind, void* hip_stream) {
  const char* who = "tor_bsdf_eval_device";
  const int rc = bsdf_check(who, ctx, n, d_list, n_list, !d_in || !d_hits || !d_out || !d_value || !d_pdf);
  if (rc != TOR_OK || n == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return bsdf_launch(who, ctx, n, d_in, d_hits, d_out, d_list, n_list, d_value, d_pdf, d_kind, (hipStream_t)hip_stream);
}

int tor_bsdf_eval_host(TorContext* ctx, int64_t n, const TorRay* in, const TorHit* hits, const TorRay* out, const int32_t* list,
                       int64_t n_list, double* value, double* pdf, int32_t* kind) {
  const char* who = "tor_bsdf_eval_host";
  int rc = bsdf_check(who, ctx, n, list, n_list, !in || !hits || !out || !value || !pdf);
  if (rc != TOR_OK || n == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too, items that are not listed keep what the caller holds --, the query on the default stream,
  // the outputs back
  const size_t m = (size_t)n;
  tor::HostPart st[7] = {{in, m * sizeof(TorRay), true, false},
                         {hits, m * sizeof(TorHit), true, false},
                         {out, m * sizeof(TorRay), true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false},
                         {value, m * 24, true, true},
                         {pdf, m * 8, true, true},
                         {kind, kind ? m * 4 : 0, true, true}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = bsdf_launch(who, ctx, n, st[0].dev, st[1].dev, st[2].dev, st[3].as<const int32_t>(), n_list, st[4].as<double>(), st[5].as<double>(),
                   st[6].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

}  // extern "C"
