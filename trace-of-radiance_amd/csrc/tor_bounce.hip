// tor_bounce.hip -- path steps for host integrators (tor_bounce_device / tor_scatter_device / tor_sky_device /
// tor_bounce_select_device and the blocking _host twins, include/tor_render.h): ONE iteration of radiance()'s loop
// (render.nim:26-38) -- world.hit(ray, 0.001, +inf, rec), then rec.material.scatter(ray, rec, rng, attenuation, scattered)
// (materials.nim:21-96) -- per listed ray, the scatter alone for hit records the caller supplies, the sky gradient of
// render.nim:41-44, and the ordered compaction of the rays that scattered, on gfx950.
//
// Exactness.  The closest hit is the hit query's (tor_query.hpp, tor_query_descent.inc: the head of tor_query.hip says why the
// descent gives the sequential closest_so_far loop's record; bounce_kernel<BLOCKS, MASKED> is hit_kernel's pair of flags), and
// the record is built with hit_kernel's operations, so d_hits is what tor_hit_device writes.  The scatter is
// tor_shade_scatter.inc, the text radiance_kernel (tor_radiance.hip) includes: the same cold records, helpers, draws and
// operation order, float64 unfused.  Driven the reference's way -- att = 1; per step att *= attenuation, a miss ends with sky *
// att, an absorbed ray with black, max_depth steps -- the steps are radiance_kernel's iterations one launch at a time: colours
// and states equal tor_radiance_device's bit for bit.
//
// One ray per lane: every lane does exactly one bounce, so there is no refill queue.  Arrays are indexed by the ray, not by the
// position in the list; the lanes of entries outside [0, n_rays) and past the end of the list take part in the descent with
// t_max = 0 (its uniform loops use scalar loads) and touch no memory.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "tor_context.hpp"
#include "tor_device.hpp"
#include "tor_query.hpp"
#include "tor_scene.hpp"
#include "tor_shade.hpp"

static_assert(sizeof(TorRay) == 56 && sizeof(TorHit) == 64 && sizeof(TorRng) == 32, "TorRay / TorHit / TorRng as the kernels index them");
static_assert(offsetof(TorHit, object) == 56 && offsetof(TorHit, front_face) == 60, "TorHit: object in the low, front_face in the high word of word 7");
static_assert(sizeof(TorRng) == sizeof(tor::Rng), "TorRng mirrors tor::Rng");

namespace tor {
namespace {

constexpr int kStepThreads = 256;
constexpr int kSelTile = 1024;  // entries per 256-thread block of the compaction

struct BParams {
  QParams q;                 // bounce_kernel: the scene and its boxes (rays, t_range, hits, n_rays unused)
  double* rays;              // 7 float64 per ray (TorRay): r_in, overwritten by `scattered` on a hit
  unsigned long long* rng;   // 4 u64 per ray (TorRng), read and written on a hit
  const int* list;           // the rays to step, or null: entry e is ray e
  long long n_list, n_rays;
  double* hits;              // 8 float64 words per ray (TorHit): written by bounce_kernel, read by scatter_kernel
  double* att;               // 3 float64 per ray: the attenuation
  int* status;               // TOR_BOUNCE_*
  const double* obj_cold;    // scatter_kernel: the cold records by ORIGINAL index, 16 float64 per object
  long long n_objects;
};

// the ray of this lane's list entry, or -1 (listed_ray, tor_query.hpp)
__device__ __forceinline__ long long step_ray(const BParams& P) {
  return listed_ray(P.list, P.n_list, P.n_rays, (long long)blockIdx.x * kStepThreads + threadIdx.x);
}

__device__ __forceinline__ void write_miss(const BParams& P, long long i) {
  double* a = P.att + 3 * i;
  a[0] = 0.0; a[1] = 0.0; a[2] = 0.0;
  P.status[i] = TOR_BOUNCE_MISS;
}

// `scattered`, the state after the scatter's last draw, the attenuation (0 for an absorbed ray: the reference leaves it unset) and
// the status of ray i
__device__ __forceinline__ void write_scatter(const BParams& P, long long i, const QRay& r, const Rng& g, V3 att, bool ended) {
  double* q = P.rays + 7 * i;
  q[0] = r.ox; q[1] = r.oy; q[2] = r.oz;
  q[3] = r.dx; q[4] = r.dy; q[5] = r.dz;
  q[6] = r.time;
  unsigned long long* s = P.rng + 4 * i;
  s[0] = g.s0; s[1] = g.s1; s[2] = g.s2; s[3] = g.s3;
  double* a = P.att + 3 * i;
  a[0] = ended ? 0.0 : att.x; a[1] = ended ? 0.0 : att.y; a[2] = ended ? 0.0 : att.z;
  P.status[i] = ended ? TOR_BOUNCE_ABSORBED : TOR_BOUNCE_SCATTERED;
}

// MASKED: with visibility groups (tor_bounce_masked_device) the closest VISIBLE object scatters
template <bool BLOCKS, bool MASKED>
__global__ __launch_bounds__(kStepThreads) void bounce_kernel(const KArgs<BParams, MASKED> A) {
  const BParams& P = A.P;
  const QParams& p = P.q;
  const long long i = step_ray(P);
  const bool live = i >= 0;
  Sees<MASKED> vis{nullptr, nullptr, 0u};  // (lanes without a ray see nothing)
  if constexpr (MASKED) {
    if (live) vis.m = A.mk.ray_mask ? A.mk.ray_mask[i] : A.mk.mask;
    vis.grp = A.mk.grp;
    vis.box_or = A.mk.box_or;
  }
  QRay r{};  // (lanes without a ray: t_max = 0 accepts nothing)
  if (live) load_ray(r, P.rays, nullptr, i);  // render.nim:28: (0.001, +inf)
  r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;  // spheres.nim:30
  QBest b{r.t_max, INT_MAX, -1};
#include "tor_query_descent.inc"
  if (!live) return;
  double* h = P.hits + 8 * i;
  if (b.slot < 0) {  // miss: the record tor_hit_device writes; ray and state untouched, nothing drawn
    write_miss_record(h);
    write_miss(P, i);
    return;
  }
  // the record, with tor_query_record.inc's operations through V3: the scatter goes on with hp, n and front
  const double* c = p.cold + 16 * (size_t)b.slot;
  double cx, cy, cz;
  centre_at(c, r.time, cx, cy, cz);                                 // moving_spheres.nim:39-44
  const V3 o = v3(r.ox, r.oy, r.oz), d = v3(r.dx, r.dy, r.dz);
  const V3 hp = o + d * b.t;                                       // rays.nim:24-25
  const V3 outward = (hp - v3(cx, cy, cz)) * c[6];                 // spheres.nim:43 (c[6] = 1.0 / radius)
  const bool front = dot(d, outward) < 0.0;                        // core.nim:47-49
  const V3 n = front ? outward : -outward;
  h[0] = hp.x; h[1] = hp.y; h[2] = hp.z;
  h[3] = n.x; h[4] = n.y; h[5] = n.z;
  h[6] = b.t;
  h[7] = __longlong_as_double((long long)(((unsigned long long)(front ? 1u : 0u) << 32) | (unsigned)b.orig));
  // the scatter
  const unsigned long long* s = P.rng + 4 * i;
  Rng g{s[0], s[1], s[2], s[3]};
  const V3 ud = unit_vector(d);  // materials.nim:40,68
  V3 att = v3(1.0, 1.0, 1.0);
  bool ended = false;
  {
#include "tor_shade_scatter.inc"
  }
  write_scatter(P, i, r, g, att, ended);
}

// rec.material.scatter for the caller's record: material of hits[i].object, and p, normal, front_face as given
__global__ __launch_bounds__(kStepThreads) void scatter_kernel(const BParams P) {
  const long long i = step_ray(P);
  if (i < 0) return;
  const double* h = P.hits + 8 * i;
  const unsigned long long w7 = (unsigned long long)__double_as_longlong(h[7]);
  const long long object = (long long)(int)(unsigned)(w7 & 0xffffffffull);
  if (object < 0 || object >= P.n_objects) {  // no such object: a miss
    write_miss(P, i);
    return;
  }
  const bool front = (unsigned)(w7 >> 32) != 0u;
  const double* c = P.obj_cold + 16 * (size_t)object;
  const double* q = P.rays + 7 * i;
  QRay r{};
  r.time = q[6];
  const V3 d = v3(q[3], q[4], q[5]);
  const V3 hp = v3(h[0], h[1], h[2]);
  const V3 n = v3(h[3], h[4], h[5]);
  const unsigned long long* s = P.rng + 4 * i;
  Rng g{s[0], s[1], s[2], s[3]};
  const V3 ud = unit_vector(d);
  V3 att = v3(1.0, 1.0, 1.0);
  bool ended = false;
  {
#include "tor_shade_scatter.inc"
  }
  write_scatter(P, i, r, g, att, ended);
}

// render.nim:41-44 without the attenuation (sky()'s product with (1, 1, 1) is exact)
__global__ __launch_bounds__(kStepThreads) void sky_kernel(const BParams P) {
  const long long i = step_ray(P);
  if (i < 0) return;
  const double* q = P.rays + 7 * i;
  const V3 col = sky(v3(q[3], q[4], q[5]), v3(1.0, 1.0, 1.0));
  double* a = P.att + 3 * i;
  a[0] = col.x; a[1] = col.y; a[2] = col.z;
}

// ---- ordered compaction of the scattered rays, in tiles of kSelTile entries per block: entry b * kSelTile + k * 256 + t ----

__device__ __forceinline__ bool select_keeps(const int* status, const int* list_in, long long n_in, long long n_rays, long long e, int& ray) {
  if (e >= n_in) return false;
  const long long i = list_in ? (long long)list_in[e] : e;
  if (i < 0 || i >= n_rays) return false;
  ray = (int)i;
  return status[i] == TOR_BOUNCE_SCATTERED;
}

// pass 1: block_count[b] = the block's survivors (wave ballots)
__global__ __launch_bounds__(256) void select_count_kernel(const int* status, const int* list_in, long long n_in, long long n_rays,
                                                            unsigned* block_count) {
  __shared__ unsigned s_cnt[4];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  unsigned mine = 0;
  for (int k = 0; k < kSelTile / 256; ++k) {
    int ray = 0;
    const bool keep = select_keeps(status, list_in, n_in, n_rays, (long long)blockIdx.x * kSelTile + k * 256 + threadIdx.x, ray);
    mine += (unsigned)__popcll(__ballot(keep));
  }
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// pass 2 (one block): block_count -> exclusive offsets in place, the total to *n_out
__global__ __launch_bounds__(1024) void select_scan_kernel(unsigned* block_count, int n_blocks, long long* n_out) {
  __shared__ unsigned s[1024];
  const int t = (int)threadIdx.x;
  const int per = (n_blocks + 1023) / 1024;  // thread t owns blocks [t * per, (t + 1) * per)
  const int b0 = t * per < n_blocks ? t * per : n_blocks;
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
  if (t == 1023) *n_out = (long long)s[1023];
}

// pass 3: the survivors to list_out at their block's offset + their rank inside the block, in input order
__global__ __launch_bounds__(256) void select_scatter_kernel(const int* status, const int* list_in, long long n_in, long long n_rays,
                                                              const unsigned* block_offset, int* list_out) {
  __shared__ unsigned s_cnt[kSelTile / 256][4];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  unsigned long long masks[kSelTile / 256];
  int rays[kSelTile / 256];
  for (int k = 0; k < kSelTile / 256; ++k) {
    rays[k] = 0;
    masks[k] = __ballot(select_keeps(status, list_in, n_in, n_rays, (long long)blockIdx.x * kSelTile + k * 256 + threadIdx.x, rays[k]));
    if (lane == 0) s_cnt[k][wave] = (unsigned)__popcll(masks[k]);
  }
  __syncthreads();
  unsigned run = block_offset[blockIdx.x];
  for (int k = 0; k < kSelTile / 256; ++k) {
    unsigned before = run;
    for (int w = 0; w < wave; ++w) before += s_cnt[k][w];
    // (before + rank < the number of survivors <= n_in: list_out holds n_in entries)
    if ((masks[k] >> lane) & 1ull) list_out[before + (unsigned)__popcll(masks[k] & ((1ull << lane) - 1ull))] = rays[k];
    run += s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
  }
}

}  // namespace
}  // namespace tor

namespace {

// the checks every step shares (tor::list_args) and a step's own; none needs a device or reads *ctx.  Then the scene.
int bounce_check(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, const void* rng, const void* list, int64_t n_list,
                 double time_lo, double time_hi, int32_t mode, const void* hits, const void* att, const void* status) {
  const std::string w = who;
  int rc = tor::list_args(w, ctx, n_rays, list, n_list);
  if (rc == TOR_OK) rc = tor::range_args(w, time_lo, time_hi, mode);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && (!rays || !rng || !hits || !att || !status))
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays, rng, hits, attenuation or status");
  return tor::scene_args(who, ctx);
}

int scatter_check(const char* who, TorContext* ctx, int64_t n_rays, const void* rays, const void* hits, const void* rng, const void* list,
                  int64_t n_list, const void* att, const void* status) {
  const std::string w = who;
  const int rc = tor::list_args(w, ctx, n_rays, list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && (!rays || !hits || !rng || !att || !status))
    return tor::fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL rays, hits, rng, attenuation or status");
  return tor::scene_args(who, ctx);
}

unsigned step_grid(int64_t n_list) { return (unsigned)((n_list + tor::kStepThreads - 1) / tor::kStepThreads); }

// the launches; the arguments are checked, n_rays > 0 and n_list > 0
int bounce_launch(const char* who, TorContext* ctx, int64_t n_rays, void* d_rays, void* d_rng, const int32_t* d_list, int64_t n_list,
                  double time_lo, double time_hi, int32_t mode, void* d_hits, double* d_att, int32_t* d_status, hipStream_t stream,
                  bool masked = false, const uint32_t* d_mask = nullptr, uint32_t mask = 0) {
  // scattered Metal and Dielectric rays carry time 0: the boxes are built for a range that holds it, as radiance_launch builds
  // them, so a chain of steps called with one range looks up ONE cached set of block bounds
  const double lo = time_lo < 0.0 ? time_lo : 0.0, hi = time_hi > 0.0 ? time_hi : 0.0;
  tor::BParams P{};
  tor::MParams mk{};
  bool blocks = false;
  std::string why;
  int rc = tor::query_setup(who, ctx, lo, hi, mode, stream, P.q, blocks, why);
  if (rc == TOR_OK && masked) rc = tor::masked_setup(ctx, blocks, d_mask, mask, stream, mk);
  if (rc != TOR_OK) return rc;
  P.rays = (double*)d_rays;
  P.rng = (unsigned long long*)d_rng;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_rays = (long long)n_rays;
  P.hits = (double*)d_hits;
  P.att = d_att;
  P.status = d_status;
  tor::for_variant(blocks, masked, [&](auto B, auto M) {
    hipLaunchKernelGGL((tor::bounce_kernel<decltype(B)::value, decltype(M)::value>), dim3(step_grid(n_list)), dim3(tor::kStepThreads), 0,
                       stream, tor::kargs<decltype(M)::value>(P, mk));
  });
  return tor::query_finish(ctx, stream, "bounce", masked, blocks, why);
}

int scatter_launch(const char* who, TorContext* ctx, int64_t n_rays, void* d_rays, const void* d_hits, void* d_rng, const int32_t* d_list,
                   int64_t n_list, double* d_att, int32_t* d_status, hipStream_t stream) {
  tor::BParams P{};
  int rc = tor::query_stream_rule(who, ctx, stream);  // (no layout and no box: the scatter reads the by-object records alone)
  if (rc == TOR_OK) rc = tor::ensure_obj_cold("tor_scatter_device", ctx, stream);
  if (rc != TOR_OK) return rc;
  P.rays = (double*)d_rays;
  P.rng = (unsigned long long*)d_rng;
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_rays = (long long)n_rays;
  P.hits = (double*)d_hits;  // (read only)
  P.att = d_att;
  P.status = d_status;
  P.obj_cold = (const double*)ctx->hitq.obj_cold.ptr;
  P.n_objects = (long long)ctx->n_objects;
  hipLaunchKernelGGL(tor::scatter_kernel, dim3(step_grid(n_list)), dim3(tor::kStepThreads), 0, stream, P);
  rc = tor::query_done(ctx, stream);
  if (rc != TOR_OK) return rc;
  tor::set_last_note("scatter");
  return TOR_OK;
}

// tor_bounce_device / tor_bounce_masked_device
int bounce_device(const char* who, TorContext* ctx, int64_t n_rays, TorRay* d_rays, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                  double time_lo, double time_hi, int32_t mode, TorHit* d_hits, double* d_att, int32_t* d_status, void* hip_stream,
                  bool masked, const uint32_t* d_mask, uint32_t mask) {
  const int rc = bounce_check(who, ctx, n_rays, d_rays, d_rng, d_list, n_list, time_lo, time_hi, mode, d_hits, d_att, d_status);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return bounce_launch(who, ctx, n_rays, d_rays, d_rng, d_list, n_list, time_lo, time_hi, mode, d_hits, d_att, d_status,
                       (hipStream_t)hip_stream, masked, d_mask, mask);
}

// the per-ray arrays the blocking twins stage, in this order: every one goes in (rays that are not listed keep what the caller
// holds); hits_out: tor_bounce_host writes the records, tor_scatter_host only reads them
void step_parts(tor::HostPart* st, int64_t n_rays, int64_t n_list, const void* rays, const void* rng, const void* list, const void* hits,
                bool hits_out, const void* att, const void* status) {
  const size_t n = (size_t)n_rays;
  st[0] = {rays, n * sizeof(TorRay), true, true};
  st[1] = {rng, n * sizeof(TorRng), true, true};
  st[2] = {list, list ? (size_t)n_list * 4 : 0, true, false};
  st[3] = {hits, n * sizeof(TorHit), true, hits_out};
  st[4] = {att, n * 24, true, true};
  st[5] = {status, n * 4, true, true};
}

}  // namespace

extern "C" {

int tor_bounce_device(TorContext* ctx, int64_t n_rays, TorRay* d_rays, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                      double time_lo, double time_hi, int32_t mode, TorHit* d_hits, double* d_attenuation, int32_t* d_status,
                      void* hip_stream) {
  return bounce_device("tor_bounce_device", ctx, n_rays, d_rays, d_rng, d_list, n_list, time_lo, time_hi, mode, d_hits, d_attenuation,
                       d_status, hip_stream, false, nullptr, 0);
}

int tor_bounce_masked_device(TorContext* ctx, int64_t n_rays, TorRay* d_rays, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                             double time_lo, double time_hi, int32_t mode, TorHit* d_hits, double* d_attenuation, int32_t* d_status,
                             void* hip_stream, const uint32_t* d_mask, uint32_t mask) {
  return bounce_device("tor_bounce_masked_device", ctx, n_rays, d_rays, d_rng, d_list, n_list, time_lo, time_hi, mode, d_hits,
                       d_attenuation, d_status, hip_stream, true, d_mask, mask);
}

int tor_scatter_device(TorContext* ctx, int64_t n_rays, TorRay* d_rays, const TorHit* d_hits, TorRng* d_rng, const int32_t* d_list,
                       int64_t n_list, double* d_attenuation, int32_t* d_status, void* hip_stream) {
  const int rc = scatter_check("tor_scatter_device", ctx, n_rays, d_rays, d_hits, d_rng, d_list, n_list, d_attenuation, d_status);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return scatter_launch("tor_scatter_device", ctx, n_rays, d_rays, d_hits, d_rng, d_list, n_list, d_attenuation, d_status,
                        (hipStream_t)hip_stream);
}

int tor_bounce_host(TorContext* ctx, int64_t n_rays, TorRay* rays, TorRng* rng, const int32_t* list, int64_t n_list, double time_lo,
                    double time_hi, int32_t mode, TorHit* hits, double* attenuation, int32_t* status) {
  int rc = bounce_check("tor_bounce_host", ctx, n_rays, rays, rng, list, n_list, time_lo, time_hi, mode, hits, attenuation, status);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // every array in, the step on the default stream, every output back
  tor::HostPart st[6];
  step_parts(st, n_rays, n_list, rays, rng, list, hits, true, attenuation, status);
  rc = tor::stage_in(ctx, st, 6);
  if (rc != TOR_OK) return rc;
  rc = bounce_launch("tor_bounce_host", ctx, n_rays, st[0].dev, st[1].dev, st[2].as<const int32_t>(), n_list, time_lo, time_hi, mode,
                     st[3].dev, st[4].as<double>(), st[5].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 6);
}

int tor_scatter_host(TorContext* ctx, int64_t n_rays, TorRay* rays, const TorHit* hits, TorRng* rng, const int32_t* list, int64_t n_list,
                     double* attenuation, int32_t* status) {
  int rc = scatter_check("tor_scatter_host", ctx, n_rays, rays, hits, rng, list, n_list, attenuation, status);
  if (rc != TOR_OK || n_rays == 0 || n_list == 0) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  tor::HostPart st[6];
  step_parts(st, n_rays, n_list, rays, rng, list, hits, false, attenuation, status);
  rc = tor::stage_in(ctx, st, 6);
  if (rc != TOR_OK) return rc;
  rc = scatter_launch("tor_scatter_host", ctx, n_rays, st[0].dev, st[3].dev, st[1].dev, st[2].as<const int32_t>(), n_list,
                      st[4].as<double>(), st[5].as<int32_t>(), nullptr);
  if (rc != TOR_OK) return rc;
  return tor::stage_out(st, 6);
}

int tor_sky_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const int32_t* d_list, int64_t n_list, double* d_color,
                   void* hip_stream) {
  const int rc = tor::list_args("tor_sky_device", ctx, n_rays, d_list, n_list);
  if (rc != TOR_OK) return rc;
  if (n_rays > 0 && n_list > 0 && (!d_rays || !d_color)) return tor::fail(TOR_ERR_INVALID_ARGUMENT, "tor_sky_device: NULL rays or color");
  if (n_rays == 0 || n_list == 0) return TOR_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  tor::BParams P{};
  P.rays = (double*)d_rays;  // (read only)
  P.list = d_list;
  P.n_list = (long long)n_list;
  P.n_rays = (long long)n_rays;
  P.att = d_color;
  hipLaunchKernelGGL(tor::sky_kernel, dim3(step_grid(n_list)), dim3(tor::kStepThreads), 0, (hipStream_t)hip_stream, P);
  HIP_TRY(hipGetLastError());
  tor::set_last_note("sky");
  return TOR_OK;
}

int tor_bounce_select_device(TorContext* ctx, int64_t n_rays, const int32_t* d_status, const int32_t* d_list_in, int64_t n_in,
                             int32_t* d_list_out, int64_t* n_out, void* hip_stream) {
  using tor::fail;
  const std::string w = "tor_bounce_select_device";
  if (!ctx || !n_out) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": ctx or n_out is NULL");
  if (n_rays < 0 || n_rays > (int64_t)INT32_MAX) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_rays <= 2^31 - 1 (the list holds int32 indices)");
  if (n_in < 0 || n_in > (int64_t)INT32_MAX) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": need 0 <= n_in <= 2^31 - 1");
  if (!d_list_in && n_in != n_rays) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": without a list n_in must be n_rays");
  if (n_in > 0 && n_rays > 0 && (!d_status || !d_list_out)) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": NULL status or list_out");
  if (d_list_out && d_list_out == d_list_in) return fail(TOR_ERR_INVALID_ARGUMENT, w + ": d_list_out must not alias d_list_in");
  if (n_in == 0 || n_rays == 0) {
    *n_out = 0;
    return TOR_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  {  // its scratch belongs to the context: the one-stream rule of the other queries (the call itself ends synchronised)
    const int rc = tor::query_stream_rule("tor_bounce_select_device", ctx, stream);
    if (rc != TOR_OK) return rc;
  }
  // [0, 16): the survivor count; then one offset per block
  const int64_t n_blocks = (n_in + tor::kSelTile - 1) / tor::kSelTile;
  HIP_TRY(ctx->hitq.sel.ensure(16 + (size_t)n_blocks * 4));
  long long* dn = (long long*)ctx->hitq.sel.ptr;
  unsigned* block_count = (unsigned*)((char*)ctx->hitq.sel.ptr + 16);
  hipLaunchKernelGGL(tor::select_count_kernel, dim3((unsigned)n_blocks), dim3(256), 0, stream, d_status, d_list_in, (long long)n_in,
                     (long long)n_rays, block_count);
  hipLaunchKernelGGL(tor::select_scan_kernel, dim3(1), dim3(1024), 0, stream, block_count, (int)n_blocks, dn);
  hipLaunchKernelGGL(tor::select_scatter_kernel, dim3((unsigned)n_blocks), dim3(256), 0, stream, d_status, d_list_in, (long long)n_in,
                     (long long)n_rays, (const unsigned*)block_count, d_list_out);
  HIP_TRY(hipGetLastError());
  long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, dn, sizeof(h), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  *n_out = (int64_t)h;
  tor::set_last_note("bounce select");
  return TOR_OK;
}

}  // extern "C"
