// tor_patches.hip -- planar patch queries for host integrators (tor_scene_patches, tor_patch_info, tor_patch_hit_device,
// tor_patch_occluded_device and the blocking _host twins; include/tor_patches.h): a context-owned table of static quads and
// triangles, the closest patch per ray -- alone, or merged into the records tor_hit_device wrote -- and the any-hit bit, alone or
// OR-ed into tor_occluded_device's.  include/tor_patches.h holds the definition, operation by operation; patch_test follows it
// line by line.
//
// patch_kernel<ANY, MASKED>: one ray per lane, 256-thread blocks, a wave-uniform loop over the whole table (brute force), no LDS,
// no scratch, no atomics; a lane without a ray returns before its first load.  The loop's record -- q, u, v and the word that
// holds kind and groups, 80 bytes of the 128-byte device record -- comes through scalar loads from the constant address space, and
// record j + 1 is requested before record j is tested.  Per pair 46 float64 operations and no division: the division, the range
// test and the winner's update sit behind the inside test, which about one patch per ray passes.  ANY stops a lane at its first
// accepted patch and the wave when all its lanes are done (asked once per 16 patches).  The record is built after the loop, for
// the winner alone, from the unit normal the host computed when the table was set (the host code is built with
// -ffp-contract=off: the header's operations, the header's bits); the winner's index is clamped into [0, n_patches) before that
// record is read.
//
// The table's state lives here, keyed by the context (tor_patches.hpp): no other translation unit reads it.
//
// Float64, unfused (-ffp-contract=off), correctly rounded `/` and sqrt.  Stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tor_patches.h"
#include "tor_context.hpp"
#include "tor_patches.hpp"
#include "tor_query.hpp"

static_assert(sizeof(TorPatch) == 88 && offsetof(TorPatch, groups) == 8 && offsetof(TorPatch, q) == 16 && offsetof(TorPatch, u) == 40 &&
                  offsetof(TorPatch, v) == 64,
              "TorPatch as include/tor_patches.h and the Python binding lay it out");
static_assert(sizeof(TorHit) == 64 && offsetof(TorHit, normal) == 24 && offsetof(TorHit, t) == 48 && offsetof(TorHit, object) == 56 &&
                  offsetof(TorHit, front_face) == 60,
              "p is words 0..2, normal words 3..5, t word 6, object and front_face the halves of word 7");

namespace tor {
namespace {

constexpr int kPatchThreads = 256;
// the device record: 16 float64 -- q 0..2, u 3..5, v 6..8, word 9 {kind, groups}, N 10..12 (the unit normal), word 13 {material, 0}
constexpr int kPatchWords = 16;
constexpr int kAnyStride = 16;  // the any-hit walk asks "is the whole wave done?" once per this many patches

struct PParams {
  const double* rays;      // 7 float64 per ray (TorRay)
  const double* t_range;   // 2 float64 per ray, or null: (0.001, +inf)
  const int* list;         // the rays to answer, or null: entry e is ray e
  long long n_list, n;
  const double* table;     // kPatchWords float64 per patch
  int n_patches;
  int merge;
  double* hits;            // 8 float64 words per ray (TorHit); null for ANY
  int* patch;              // one int32 per ray; null for ANY
  double* uv;              // 2 float64 per ray, or null
  int* occluded;           // ANY: one int32 per ray
  const unsigned* ray_mask;  // MASKED: one word per ray, or null: every ray uses `mask`
  unsigned mask;
};

// what the loop reads of a patch: 10 wave-uniform words
struct PRec {
  double qx, qy, qz, ux, uy, uz, vx, vy, vz;
  unsigned kind, groups;
};

__device__ __forceinline__ PRec load_patch(qcdptr T, int j) {
  const qcdptr c = T + (size_t)kPatchWords * (size_t)j;
  const unsigned long long w = (unsigned long long)__double_as_longlong(c[9]);
  return PRec{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], (unsigned)(w & 0xffffffffull), (unsigned)(w >> 32)};
}

struct PRay {
  double ox, oy, oz, dx, dy, dz, t_min, limit;
};

struct PBest {
  double t, an, bn, det;
  int index;  // -1: none
};

// include/tor_patches.h THE TEST for ray r and patch c (index j); true: accepted.  Closest-hit callers pass b, which keeps the
// smallest t (ties: the lower index, the table being walked upwards)
template <bool ANY>
__device__ __forceinline__ bool patch_test(const PRec& c, int j, const PRay& r, PBest& b) {
  const double pvx = r.dy * c.vz - r.dz * c.vy, pvy = r.dz * c.vx - r.dx * c.vz, pvz = r.dx * c.vy - r.dy * c.vx;
  double det = (c.ux * pvx + c.uy * pvy) + c.uz * pvz;
  if (!(__builtin_fabs(det) > 0.0)) return false;
  const double tvx = r.ox - c.qx, tvy = r.oy - c.qy, tvz = r.oz - c.qz;
  double an = (tvx * pvx + tvy * pvy) + tvz * pvz;
  const double qvx = tvy * c.uz - tvz * c.uy, qvy = tvz * c.ux - tvx * c.uz, qvz = tvx * c.uy - tvy * c.ux;
  double bn = (r.dx * qvx + r.dy * qvy) + r.dz * qvz;
  double tn = (c.vx * qvx + c.vy * qvy) + c.vz * qvz;
  if (det < 0.0) {
    det = -det; an = -an; bn = -bn; tn = -tn;
  }
  const bool inside = c.kind == (unsigned)TOR_PATCH_TRIANGLE ? (an >= 0.0 && bn >= 0.0 && (an + bn) <= det)
                                                             : (an >= 0.0 && an <= det && bn >= 0.0 && bn <= det);
  if (!inside) return false;
  const double t = tn / det;
  if (!(r.t_min < t && t < r.limit)) return false;
  if constexpr (!ANY) {
    if (b.index < 0 || t < b.t) {
      b.t = t; b.an = an; b.bn = bn; b.det = det; b.index = j;
    }
  }
  return true;
}

template <bool ANY, bool MASKED>
__global__ __launch_bounds__(kPatchThreads) void patch_kernel(const PParams P) {
  const long long i = listed_ray(P.list, P.n_list, P.n, (long long)blockIdx.x * kPatchThreads + threadIdx.x);
  if (i < 0) return;
  const double* q = P.rays + 7 * i;
  PRay r;
  r.ox = q[0]; r.oy = q[1]; r.oz = q[2];
  r.dx = q[3]; r.dy = q[4]; r.dz = q[5];
  r.t_min = 0.001;
  r.limit = __builtin_inf();
  if (P.t_range) {
    r.t_min = P.t_range[2 * i];
    r.limit = P.t_range[2 * i + 1];
  }
  unsigned m = 0xffffffffu;
  if constexpr (MASKED) m = P.ray_mask ? P.ray_mask[i] : P.mask;
  if constexpr (!ANY) {
    if (P.merge) {  // the sphere's record lowers the limit: a tie stays with the sphere
      const double* h = P.hits + 8 * i;
      const int object = (int)(unsigned)((unsigned long long)__double_as_longlong(h[7]) & 0xffffffffull);
      const double ht = h[6];
      if (object >= 0 && ht < r.limit) r.limit = ht;
    }
  }
  PBest b{0.0, 0.0, 0.0, 1.0, -1};
  bool done = false;
  const int n = P.n_patches;
  const qcdptr T = (qcdptr)(uintptr_t)P.table;
  // wave-uniform: every lane tests the same record; record j + 1 is requested before record j is tested.  ANY asks after every
  // kAnyStride records whether a lane of the wave is still looking (asked after every record, the question costs more than the
  // early exit saves on incoherent rays); the closest hit walks the table in one stretch
  const int stride = ANY ? kAnyStride : n;
  PRec cur = load_patch(T, 0);
  for (int j0 = 0; j0 < n; j0 += stride) {
    const int j1 = n - j0 < stride ? n : j0 + stride;
    for (int j = j0; j < j1; ++j) {
      const PRec nxt = load_patch(T, j + 1 < n ? j + 1 : j);
      bool see = !done;
      if constexpr (MASKED) see = see && (cur.groups & m) != 0u;
      if (see && patch_test<ANY>(cur, j, r, b)) {
        if constexpr (ANY) done = true;
      }
      cur = nxt;
    }
    if constexpr (ANY) {
      if (__ballot(!done) == 0) break;
    }
  }
  if constexpr (ANY) {
    if (done) P.occluded[i] = 1;
    else if (!P.merge) P.occluded[i] = 0;
    return;
  } else {
    double* o = P.hits + 8 * i;
    if (b.index < 0) {
      if (!P.merge) write_miss_record(o);
      P.patch[i] = -1;
      if (P.uv) {
        P.uv[2 * i] = 0.0;
        P.uv[2 * i + 1] = 0.0;
      }
      return;
    }
    const int w = b.index > n - 1 ? n - 1 : b.index;  // in [0, n) whatever the loop left (b.index >= 0 here)
    const qgdptr c = (qgdptr)(uintptr_t)(P.table + (size_t)kPatchWords * (size_t)w);
    double nx = c[10], ny = c[11], nz = c[12];
    const int material = (int)(unsigned)((unsigned long long)__double_as_longlong(c[13]) & 0xffffffffull);
    const double t = b.t;
    const double px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t;
    const bool front = ((r.dx * nx + r.dy * ny) + r.dz * nz) < 0.0;
    if (!front) {
      nx = -nx; ny = -ny; nz = -nz;
    }
    o[0] = px; o[1] = py; o[2] = pz;
    o[3] = nx; o[4] = ny; o[5] = nz;
    o[6] = t;
    o[7] = __longlong_as_double((long long)(((unsigned long long)(front ? 1u : 0u) << 32) | (unsigned)material));
    P.patch[i] = w;
    if (P.uv) {
      P.uv[2 * i] = b.an / b.det;
      P.uv[2 * i + 1] = b.bn / b.det;
    }
  }
}

// ---- the table of a context ---------------------------------------------------------------------------------------------------

struct PatchTable {
  DeviceBuffer dev;            // kPatchWords float64 per patch
  int64_t n = 0;               // 0: no table
  int64_t with_material = 0;   // the patches whose material is >= 0
  bool every_group = false;    // no patch has the group word 0: a launch whose mask is 0xFFFFFFFF for every ray needs no group test
};

std::mutex g_tables_mu;
std::unordered_map<TorContext*, PatchTable> g_tables;

// the context's table, or null when it never had one (the map's nodes do not move: the pointer stays good until the context is
// destroyed; calls on ONE context are the caller's to serialise, as for every other entry)
PatchTable* table_of(TorContext* ctx, bool create) {
  std::lock_guard<std::mutex> lock(g_tables_mu);
  if (create) return &g_tables[ctx];
  const auto it = g_tables.find(ctx);
  return it == g_tables.end() ? nullptr : &it->second;
}

}  // namespace

void patches_scene_replaced(TorContext* ctx) {
  if (PatchTable* t = table_of(ctx, false)) t->n = t->with_material = 0;
}

void patches_context_destroyed(TorContext* ctx) {
  std::lock_guard<std::mutex> lock(g_tables_mu);
  const auto it = g_tables.find(ctx);
  if (it == g_tables.end()) return;
  it->second.dev.release();
  g_tables.erase(it);
}

}  // namespace tor

namespace {

inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rule 5 of tor_scene_patches for one record, in the header's order: why it is refused, or null -- then `unit` holds
// N = cross(u, v) * (1.0 / sqrt(nn)), the header's operations (this file is built with -ffp-contract=off)
const char* patch_refusal(const TorPatch& p, int64_t n_objects, double* unit) {
  if (p.kind != TOR_PATCH_QUAD && p.kind != TOR_PATCH_TRIANGLE) return "unknown kind";
  if (p.material < -1 || p.material >= n_objects) return "material outside [-1, n_objects)";
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(p.q[k]) || !std::isfinite(p.u[k]) || !std::isfinite(p.v[k])) return "q, u and v must be finite";
  double nrm[3];
  cross3(p.u, p.v, nrm);
  if (!std::isfinite(nrm[0]) || !std::isfinite(nrm[1]) || !std::isfinite(nrm[2])) return "cross(u, v) is not finite";
  const double nn = dot3(nrm, nrm);
  if (!(nn > 0.0) || std::isinf(nn)) return "the patch has no area, or |cross(u, v)|^2 overflows";
  const double inv = 1.0 / std::sqrt(nn);
  if (!std::isfinite(inv)) return "1 / |cross(u, v)| is not finite";
  for (int k = 0; k < 3; ++k) unit[k] = nrm[k] * inv;
  return nullptr;
}

// the checks that need no device and do not read *ctx: tor_bsdf_eval_device's, then the NULL arrays; then the scene and the table
int patch_check(const char* who, TorContext* ctx, int64_t n, const void* list, int64_t n_list, bool nulls, const char* arrays) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n > 0 && n_list > 0 && nulls) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL " + arrays);
  const int rs = tor::scene_args(who, ctx);
  if (rs != TOR_OK) return rs;
  const tor::PatchTable* t = tor::table_of(ctx, false);
  if (!t || t->n <= 0) return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": the context has no patch table (tor_scene_patches)");
  return TOR_OK;
}

// the launch of either query; the arguments are checked, n > 0 and n_list > 0
int patch_launch(const char* who, TorContext* ctx, bool any, int64_t n, const void* d_rays, const double* d_t_range, const int32_t* d_list,
                 int64_t n_list, int32_t merge, void* d_hits, int32_t* d_patch, double* d_uv, int32_t* d_occluded, hipStream_t stream,
                 const uint32_t* d_mask, uint32_t mask) {
  const int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the query reads the patch table alone)
  if (rc != TOR_OK) return rc;
  const tor::PatchTable& t = *tor::table_of(ctx, false);
  tor::PParams P{};
  P.rays = (const double*)d_rays;
  P.t_range = d_t_range;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n = (long long)n;
  P.table = (const double*)t.dev.ptr;
  P.n_patches = (int)t.n;
  P.merge = merge != 0 ? 1 : 0;
  P.hits = (double*)d_hits;
  P.patch = d_patch;
  P.uv = d_uv;
  P.occluded = d_occluded;
  P.ray_mask = d_mask;
  P.mask = mask;
  const bool masked = d_mask != nullptr || mask != 0xFFFFFFFFu || !t.every_group;
  const dim3 grid((unsigned)((n_list + tor::kPatchThreads - 1) / tor::kPatchThreads)), block(tor::kPatchThreads);
  if (any && masked) hipLaunchKernelGGL((tor::patch_kernel<true, true>), grid, block, 0, stream, P);
  else if (any) hipLaunchKernelGGL((tor::patch_kernel<true, false>), grid, block, 0, stream, P);
  else if (masked) hipLaunchKernelGGL((tor::patch_kernel<false, true>), grid, block, 0, stream, P);
  else hipLaunchKernelGGL((tor::patch_kernel<false, false>), grid, block, 0, stream, P);
  const int rd = tor::query_done(ctx, stream);
  if (rd != TOR_OK) return rd;
  tor::set_last_note(any ? "patch occluded" : "patch hit");
  return TOR_OK;
}

}  // namespace

extern "C" {

int tor_scene_patches(TorContext* ctx, int64_t n_patches, const TorPatch* table) {
  using tor::fail;
  const std::string w = "tor_scene_patches";
  if (!ctx) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx is NULL");
  if (!ctx->scene_ready) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": no scene uploaded");
  if (n_patches < 0 || n_patches > TOR_PATCH_MAX)
    return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_patches <= TOR_PATCH_MAX (" + std::to_string((int)TOR_PATCH_MAX) + ")");
  if (n_patches > 0 && !table) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": table is NULL");
  for (int64_t j = 0; j < n_patches; ++j) {  // every record is checked before anything is allocated or changed
    double unit[3];
    const char* why = patch_refusal(table[j], ctx->n_objects, unit);
    if (why) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": table[" + std::to_string(j) + "]: " + why);
  }
  // the library's copy: the device records, with the unit normal of every patch
  std::vector<double> rec;
  try {
    rec.assign((size_t)n_patches * tor::kPatchWords, 0.0);
  } catch (const std::bad_alloc&) {
    return fail(TOR_ERR_OUT_OF_MEMORY, w + ": no host memory for the table's copy");
  }
  int64_t with_material = 0;
  bool every_group = true;
  for (int64_t j = 0; j < n_patches; ++j) {
    const TorPatch& p = table[j];
    double* r = &rec[(size_t)j * tor::kPatchWords];
    (void)patch_refusal(p, ctx->n_objects, r + 10);
    for (int k = 0; k < 3; ++k) {
      r[k] = p.q[k];
      r[3 + k] = p.u[k];
      r[6 + k] = p.v[k];
    }
    const uint64_t w9 = (uint64_t)(uint32_t)p.kind | ((uint64_t)p.groups << 32), w13 = (uint64_t)(uint32_t)p.material;
    std::memcpy(&r[9], &w9, 8);
    std::memcpy(&r[13], &w13, 8);
    with_material += p.material >= 0 ? 1 : 0;
    every_group = every_group && p.groups != 0u;
  }
  tor::HitQueryState& hq = ctx->hitq;
  HIP_TRY(hipSetDevice(ctx->device));
  if (hq.launched) HIP_TRY(hipEventSynchronize(hq.ev_done));  // the last query may still read the table
  tor::PatchTable* t = tor::table_of(ctx, n_patches > 0);
  if (n_patches == 0) {  // clear: the buffer stays for the next table
    if (t) t->n = t->with_material = 0;
    return TOR_OK;
  }
  t->n = t->with_material = 0;  // (a failed allocation or copy leaves no table rather than half of one)
  HIP_TRY(t->dev.ensure(rec.size() * 8));
  HIP_TRY(hipMemcpy(t->dev.ptr, rec.data(), rec.size() * 8, hipMemcpyHostToDevice));
  t->n = n_patches;
  t->with_material = with_material;
  t->every_group = every_group;
  return TOR_OK;
}

int tor_patch_info(TorContext* ctx, int64_t* out) {
  if (!ctx || !out) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_patch_info: NULL argument");
  const tor::PatchTable* t = tor::table_of(ctx, false);
  out[0] = t ? t->n : 0;
  out[1] = t && t->n > 0 ? t->with_material : 0;
  return TOR_OK;
}

int tor_patch_hit_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                         int64_t n_list, int32_t merge, TorHit* d_hits, int32_t* d_patch, double* d_uv, void* hip_stream,
                         const uint32_t* d_mask, uint32_t mask) {
  const char* who = "tor_patch_hit_device";
  const int rc = patch_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_hits || !d_patch, "rays, hits or patch");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return patch_launch(who, ctx, false, n_rays, d_rays, d_t_range, d_list, n_list, merge, d_hits, d_patch, d_uv, nullptr,
                      (hipStream_t)hip_stream, d_mask, mask);
}

int tor_patch_hit_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list, int64_t n_list,
                       int32_t merge, TorHit* hits, int32_t* patch, double* uv, const uint32_t* masks, uint32_t mask) {
  const char* who = "tor_patch_hit_host";
  int rc = patch_check(who, ctx, n_rays, list, n_list, !rays || !hits || !patch, "rays, hits or patch");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in -- the outputs too: rays that are not listed, and merged records without a patch, keep what the caller holds
  const size_t m = (size_t)n_rays;
  tor::HostPart st[7] = {{rays, m * sizeof(TorRay), true, false}, {t_range, t_range ? m * 16 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false}, {hits, m * sizeof(TorHit), true, true},
                         {patch, m * 4, true, true}, {uv, uv ? m * 16 : 0, true, true}, {masks, masks ? m * 4 : 0, true, false}};
  rc = tor::stage_in(ctx, st, 7);
  if (rc != TOR_OK) return rc;
  rc = patch_launch(who, ctx, false, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const int32_t>(), n_list, merge, st[3].dev,
                    st[4].as<int32_t>(), st[5].as<double>(), nullptr, nullptr, st[6].as<const uint32_t>(), mask);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 7);
}

int tor_patch_occluded_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                              int64_t n_list, int32_t merge, int32_t* d_occluded, void* hip_stream, const uint32_t* d_mask,
                              uint32_t mask) {
  const char* who = "tor_patch_occluded_device";
  const int rc = patch_check(who, ctx, n_rays, d_list, n_list, !d_rays || !d_occluded, "rays or occluded");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return patch_launch(who, ctx, true, n_rays, d_rays, d_t_range, d_list, n_list, merge, nullptr, nullptr, nullptr, d_occluded,
                      (hipStream_t)hip_stream, d_mask, mask);
}

int tor_patch_occluded_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                            int64_t n_list, int32_t merge, int32_t* occluded, const uint32_t* masks, uint32_t mask) {
  const char* who = "tor_patch_occluded_host";
  int rc = patch_check(who, ctx, n_rays, list, n_list, !rays || !occluded, "rays or occluded");
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t m = (size_t)n_rays;
  tor::HostPart st[5] = {{rays, m * sizeof(TorRay), true, false}, {t_range, t_range ? m * 16 : 0, true, false},
                         {list, list ? (size_t)n_list * 4 : 0, true, false}, {occluded, m * 4, true, true},
                         {masks, masks ? m * 4 : 0, true, false}};
  rc = tor::stage_in(ctx, st, 5);
  if (rc != TOR_OK) return rc;
  rc = patch_launch(who, ctx, true, n_rays, st[0].dev, st[1].as<const double>(), st[2].as<const int32_t>(), n_list, merge, nullptr, nullptr,
                    nullptr, st[3].as<int32_t>(), nullptr, st[4].as<const uint32_t>(), mask);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 5);
}

}  // extern "C"
