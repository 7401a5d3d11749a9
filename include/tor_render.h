/*
 * tor_render.h -- C ABI of libtor_mi355x.so: the MI355X (gfx950) implementation of the
 * trace-of-radiance integrator hot path
 *     render() -> radiance() -> HittableList.hit -> Material.scatter
 * (reference: trace_of_radiance/render.nim:21-68).  Plain pointers and sizes only; every
 * struct is a bit-for-bit mirror of the value type Nim's C backend emits for the reference
 * type named next to it (x86-64), so a Nim caller passes `unsafeAddr` of its own objects
 * (see INTEGRATION.md for the {.importc.} shim).
 *
 * All arithmetic on the path is IEEE float64 (vec3s.nim:12-14).
 */
#ifndef TOR_RENDER_H
#define TOR_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOR_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------ */
/* POD mirrors of the reference's value types                                            */
/* ------------------------------------------------------------------------------------ */

/* Vec3 / Point3 / Color / Attenuation / UnitVector -- primitives/vec3s.nim:12-14 (24 B) */
typedef struct TorVec3 { double x, y, z; } TorVec3;

/* MaterialKind -- physics/core.nim:25-27 (enum order of registerSubType) */
enum { TOR_LAMBERTIAN = 0, TOR_METAL = 1, TOR_DIELECTRIC = 2 };

/* Material -- physics/core.nim:16-28 (object variant: kind:uint8 @0, union @8; 40 B) */
typedef struct TorMaterial {
  uint8_t kind;
  uint8_t _pad[7];
  union {
    struct { TorVec3 albedo; } lambertian;              /* core.nim:16-17 */
    struct { TorVec3 albedo; double fuzz; } metal;      /* core.nim:18-20 */
    struct { double refraction_index; } dielectric;     /* core.nim:21-22 */
  } u;
} TorMaterial;

/* Sphere -- physics/hittables/spheres.nim:15-18 (72 B) */
typedef struct TorSphere {
  TorVec3 center;
  double radius;
  TorMaterial material;
} TorSphere;

/* MovingSphere -- physics/hittables/moving_spheres.nim:15-20 (112 B) */
typedef struct TorMovingSphere {
  TorVec3 center0, center1;
  double time0, time1;
  double radius;
  TorMaterial material;
} TorMovingSphere;

/* HittableVariantKind -- physics/hittables/hittables_variants.nim:53-54 */
enum { TOR_SPHERE = 0, TOR_MOVING_SPHERE = 1 };

/* HittableVariant -- hittables_variants.nim:50-57 (kind:uint8 @0, union @8; 120 B) */
typedef struct TorHittableVariant {
  uint8_t kind;
  uint8_t _pad[7];
  union {
    TorSphere sphere;
    TorMovingSphere moving_sphere;
  } u;
} TorHittableVariant;

/* HittableList -- physics/hittables/hittables_lists.nim:20-24 (borrowed view; 16 B) */
typedef struct TorHittableList {
  int64_t len;
  const TorHittableVariant* objects;
} TorHittableList;

/* Camera -- physics/cameras.nim:15-22 (24 float64 in declaration order; 192 B) */
typedef struct TorCamera {
  TorVec3 origin, lower_left_corner, horizontal, vertical, u, v, w;
  double lens_radius, shutter_open, shutter_close;
} TorCamera;

/* Canvas -- primitives/canvas.nim:20-28 (24 B).  pixels: nrows*ncols Colors, row-major,
 * row 0 = BOTTOM scanline (io/ppm.nim:20); caller-allocated, fully overwritten. */
typedef struct TorCanvas {
  TorVec3* pixels;
  int32_t nrows, ncols;
  int32_t samples_per_pixel;
  float gamma_correction;
} TorCanvas;

/* ------------------------------------------------------------------------------------ */
/* Options                                                                               */
/* ------------------------------------------------------------------------------------ */

/* How the per-pixel RNG streams are laid out. */
enum {
  /* render.nim:59-67: rng.seed(row,col) once per pixel, the spp samples share one stream.
   * One GPU lane per PIXEL.  This is the reference's behaviour. */
  TOR_SEED_PIXEL = 0,
  /* Counter-based extension (BASELINE.json north_star): the stream is re-seeded per
   * (row,col,sample): sm=pair(row,col); h=splitMix64(sm); seed(h xor sample).
   * One GPU lane per PIXEL-SAMPLE; per-pixel sums use exact (2^-36-quantised) float64
   * addition so the result does not depend on scheduling or device count. */
  TOR_SEED_SAMPLE = 1
};

/* Rounding of the ray/sphere quadratic. */
enum {
  TOR_ARITH_STRICT = 0, /* reference operation order, no FMA (README.md:82) -- the only arithmetic     */
  TOR_ARITH_FUSED = 1   /* REMOVED in round 5 (rounds 1-4: the same formulas with explicit fma(); not the
                           reference's rounding, and slower than STRICT behind the conservative screen).  The value
                           stays reserved: every entry point rejects it with TOR_ERR_INVALID_ARGUMENT and says why. */
};

/* Exact accelerations of the closest-hit query; a bit mask.  They never change a pixel:
 * closest hit is order independent and every kept object goes through the reference's float64 test. */
enum {
  TOR_ACCEL_NONE = 0,   /* the reference's algorithm and arithmetic: every ray against every object in
                           float64 (default)                                                          */
  TOR_ACCEL_BLOCKS = 1, /* objects in spatial blocks of 8 inside conservative boxes; a ray only looks
                           into the blocks whose box it can touch                                     */
  TOR_ACCEL_F32 = 2     /* still every ray against every object, but first through a conservative
                           packed-float32 discriminant with an a-priori error margin; only the objects
                           it cannot rule out get the float64 test                                    */
};

/* How the row shards of a multi-device tor_render_opt() reach the caller's canvas. */
enum {
  TOR_GATHER_AUTO = 0,  /* RCCL when the devices are distinct, librccl loads and the communicator passes its
                           self-check; if that leg fails -- or does not COMPLETE: every wait of the RCCL leg has a
                           deadline (TOR_RCCL_TIMEOUT_MS per transfer, default 10 s + 1 ms / MB; TOR_RCCL_INIT_TIMEOUT_MS
                           for communicator creation + self-check, default 120 s), past it the communicators are
                           aborted -- peer copies; if those fail: HOST (tor_last_note)                           */
  TOR_GATHER_RCCL = 1,  /* single-process RCCL (ncclCommInitAll): every device sends its shard to
                           devices[0] over xGMI, one de-interleave kernel, one D2H (BASELINE north_star) */
  TOR_GATHER_PEER = 2,  /* the same with hipMemcpyPeerAsync instead of RCCL                              */
  TOR_GATHER_HOST = 3   /* no device-side gather: every device copies its rows straight into the
                           canvas over its own PCIe link (SURVEY 8e "alternative")                       */
};

#define TOR_MAX_DEVICES 16

enum { TOR_PIXEL_KERNEL_AUTO = 0, TOR_PIXEL_KERNEL_LANE = 1, TOR_PIXEL_KERNEL_WAVE = 2 };

typedef struct TorOptions {
  uint32_t struct_size; /* = sizeof(TorOptions); the 32-byte round-1 layout (up to `accel`) is accepted too */
  int32_t seeding;      /* TOR_SEED_*  (default TOR_SEED_PIXEL)  */
  int32_t arith;        /* TOR_ARITH_* (default TOR_ARITH_STRICT) */
  int32_t device;       /* HIP device ordinal; -1 = current device */
  /* Row sharding (render.nim:55 `parallelFor row` across GPUs): image rows are cut into
   * tiles of row_tile rows; tile t is rendered by shard (t mod shard_count).  The shard's
   * rows are written compactly, in increasing row order.  shard_count <= 1: whole image. */
  int32_t shard_index, shard_count, row_tile;
  int32_t accel;        /* TOR_ACCEL_* bits (explicit options: default TOR_ACCEL_NONE) */
  /* Multi-GPU behind the drop-in (tor_render / tor_render_opt only): device_count > 1 renders the frame on
   * devices[0 .. device_count) -- one host thread and one HIP stream per entry, entry k renders row shard
   * (k, device_count, row_tile) -- and assembles it in canvas->pixels (`gather`).  An ordinal may appear more
   * than once (several contexts on one GPU: how a 1-GPU box tests the path).  shard_index/shard_count/device
   * must then be left at their defaults.  The canvas is bit-identical for every device list. */
  int32_t device_count;
  int32_t gather;       /* TOR_GATHER_* */
  int32_t devices[TOR_MAX_DEVICES];
  /* TOR_SEED_PIXEL only: which kernel walks the pixel chains (same canvas either way).
   * TOR_PIXEL_KERNEL_AUTO: with both exact accelerations, >= 32 spp and a single-level culling layout (<= 128 block
   * boxes) every frame size runs the one-lane-per-pixel kernel with the CHAIN HAND-OFF -- lanes push their long pixel
   * chains to server waves inside the same launch (DESIGN 4.7 (HISTORY 4.7-4.8); the launch covers the whole GPU and assumes exclusive
   * use of it: tor_context_handoff_stalled; TOR_MIGRATE=0 turns it off).  Where the hand-off cannot run: frames of
   * 16 K pixels and more (per device) with both accelerations and >= 32 spp are SHARED -- the tiles that carry the
   * largest part of a probed cost go to the one-wave-per-pixel kernel on a second stream, the lane kernel renders the
   * rest at the same time (TOR_SPLIT_FRAC overrides the fraction, 0 = off); otherwise one wave per pixel up to 114688
   * pixels (TOR_COOP_MAX_PIXELS), one lane per pixel above.  LANE / WAVE force one kernel for the whole frame, without
   * hand-off (WAVE falls back to LANE when the scene does not fit LDS). */
  int32_t pixel_kernel;
} TorOptions;

/* Status codes (the reference's render() returns void and has no error path; this ABI
 * returns 0 on success and never writes a partial canvas on failure). */
enum {
  TOR_OK = 0,
  TOR_ERR_INVALID_ARGUMENT = -1,
  TOR_ERR_NO_DEVICE = -2,  /* no HIP device / kernels unavailable: there is NO CPU fallback */
  TOR_ERR_HIP = -3,
  TOR_ERR_OUT_OF_MEMORY = -4,
  TOR_ERR_INCOMPLETE = -5  /* tor_last_kernel_ms after an asynchronous tor_render_device whose chain hand-off stalled: the frame
                              has holes and must be rendered again (the blocking entry points and tor_render_gather_device
                              do that themselves)                                                                     */
};

/* ------------------------------------------------------------------------------------ */
/* The drop-in entry point                                                               */
/* ------------------------------------------------------------------------------------ */

/* Replaces `proc render*(canvas: var Canvas, cam: Camera, world: HittableList,
 * max_depth: int)` -- render.nim:49.  Blocking: canvas.pixels is complete on return (the
 * reference's canvas is complete only after exit(Weave)/syncRoot(Weave),
 * trace_of_radiance.nim:61-63).  Reference semantics: TOR_SEED_PIXEL, TOR_ARITH_STRICT.
 *
 * A host that keeps the reference's signature cannot pass TorOptions, so tor_render() takes its speed knobs
 * from the environment -- none of them changes a pixel:
 *   TOR_DEFAULT_ACCEL = 0..3  TOR_ACCEL_* bits.  Unset: 3 -- both exact accelerations are ON for tor_render()
 *                             (bit-identical canvases by construction, parity tests and differential fuzzing);
 *                             0 restores the reference's float64 brute force.
 *   TOR_SCREEN = 0            (float64 brute force only) every ray x object through the reference's unfused discriminant;
 *                             unset: the object loop is a conservative FMA screen of the same quadratic and only its
 *                             candidates see the unfused operations -- same canvas (csrc/tor_screen.hpp), read at context creation
 *   TOR_DEFAULT_SEEDING = pixel | sample   the ONE knob here that selects a different (equally valid) image: `pixel`
 *                             (default) = the reference's streams, one per pixel (render.nim:59-67); `sample` = the
 *                             counter-based per-sample streams of TOR_SEED_SAMPLE -- what lets 8 GPUs share a 1080p frame
 *                             (a pixel stream is a sequential chain) and the mode the headline Msamples/s is quoted on
 *   TOR_DEVICES = "all" | "0,1,2,3"   render on several GPUs (TorOptions.device_count / devices)
 *   TOR_GATHER  = rccl | peer | host  (TorOptions.gather)
 * The device scene is cached: a call whose object list is byte-identical to the previous call's (on that
 * device) uploads nothing (the host pointer is never retained; the library keeps its own copy). */
TOR_API int tor_render(TorCanvas* canvas, const TorCamera* cam, TorHittableList world,
                       int64_t max_depth);

/* tor_render with the HittableList behind a pointer: for FFIs that would rather not pass a 16-byte struct by
 * value (Nim passes small objects by value and large ones by hidden pointer -- README.md:232-235 -- unless the
 * type is marked {.bycopy.}; a pointer leaves nothing to the calling convention). */
TOR_API int tor_render_ptr(TorCanvas* canvas, const TorCamera* cam, const TorHittableList* world, int64_t max_depth);

/* Same with explicit options (NULL = tor_render's defaults).  With shard_count > 1 only this shard's
 * rows of canvas->pixels are written (in place, at their image positions). */
TOR_API int tor_render_opt(TorCanvas* canvas, const TorCamera* cam, TorHittableList world,
                           int64_t max_depth, const TorOptions* opt);

/* Host-side cost of the last tor_render / tor_render_opt call on this thread, in milliseconds:
 * out[0] scene upload (0 on a cache hit), out[1] launch + kernels until the device is done (single device: measured
 * with HIP events on the call's stream, first launch to last kernel), out[2] the rest of the call's device section:
 * D2H / gather into canvas->pixels, out[3] whole call.  out[4] = 1 when the scene came from the cache. */
TOR_API int tor_last_render_timing(double out[5]);

/* The library's environment knobs -- ONE table (csrc/tor_knobs.hpp; KNOBS.md is generated from it): name, default, accepted
 * values, when it is read ("call" | "context" | "upload") and what it does.  Strings are static. */
TOR_API int32_t tor_knob_count(void);
TOR_API int tor_knob_info(int32_t i, const char** name, const char** dflt, const char** range, const char** when, const char** what);

/* Thread-local description of the last failure (never NULL). */
TOR_API const char* tor_last_error(void);

/* Thread-local note of the last successful multi-device tor_render / tor_render_opt on this thread (never NULL): which
 * gather ran ("gather: rccl" | "gather: peer" | "gather: host"), preceded by the legs TOR_GATHER_AUTO tried first and
 * why they failed -- AUTO walks RCCL -> peer copies -> per-device D2H and never returns a wrong canvas.  Not an error. */
TOR_API const char* tor_last_note(void);

/* Facts about the last successful multi-device tor_render / tor_render_opt on this thread (what a scaling log needs):
 * out[0] = the TOR_GATHER_* leg that assembled the frame, out[1] = ranks of the RCCL communicator that carried it
 * (ncclCommCount; 0 when the leg was not RCCL), out[2] = entries of the device list, out[3] = 1 when they were distinct GPUs. */
TOR_API int tor_last_gather_info(int32_t out[4]);
/* Duration of the dominant kernel (integrate_kernel) on every device of that call, in milliseconds: HIP events around the
 * launch on the launch's own stream.  Writes min(cap, n) values, returns n = entries of the device list. */
TOR_API int32_t tor_last_device_kernel_ms(float* out, int32_t cap);

/* ------------------------------------------------------------------------------------ */
/* Resident-context API (frame loops: trace_of_radiance_animation.nim:173-196; benchmarks; */
/* multi-GPU hosts that own device buffers)                                              */
/* ------------------------------------------------------------------------------------ */

typedef struct TorContext TorContext;

TOR_API int tor_context_create(int32_t device, TorContext** out);
TOR_API int tor_context_destroy(TorContext* ctx);

/* Flattens the AoS HittableVariant list (hittables_lists.nim:41-46) into the device SoA
 * scene.  The host pointer is not retained (the context keeps a byte copy: a later upload of an identical
 * list is a no-op, and the layouts a launch does not use -- the float32 and block-culling variants -- are
 * only built when a launch first asks for them). */
TOR_API int tor_scene_upload(TorContext* ctx, TorHittableList world);

/* Number of rows / list of rows shard (index,count,row_tile) owns. rows_out may be NULL. */
TOR_API int32_t tor_shard_rows(int32_t nrows, int32_t row_tile, int32_t shard_index,
                               int32_t shard_count, int32_t* rows_out);

/* Renders this shard's rows into d_pixels, a DEVICE buffer of tor_shard_rows()*ncols*3
 * float64 (rows in increasing order, gamma-corrected exactly like Canvas.draw,
 * canvas.nim:47-54).  Asynchronous on hip_stream (a hipStream_t; NULL = default stream);
 * the buffer is complete when the stream reaches the end of the enqueued work. */
TOR_API int tor_render_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                              int32_t samples_per_pixel, float gamma_correction,
                              int64_t max_depth, const TorOptions* opt, double* d_pixels,
                              void* hip_stream);

/* ---- progressive rendering (TOR_SEED_SAMPLE only): passes of samples into exact sums, resolve, noise -------------------
 * In TOR_SEED_SAMPLE mode a sample's stream depends only on (row, col, sample index) and every sample is rounded to a
 * multiple of 2^-36 before it is added, so every partial sum is exact: samples [0, k) and then [k, n) added into one buffer
 * give the same bits as one n-sample render, and tor_resolve_device turns them into the same canvas as tor_render_device
 * with samples_per_pixel = n.  Buffers written by separate contexts or GPUs (disjoint sample ranges) add exactly too.
 *
 * tor_render_accumulate_device: ADDS samples [first_sample, first_sample + n_samples) of this shard's rows to d_sums, a
 * DEVICE buffer of tor_shard_rows()*ncols*3 float64 (same row layout as tor_render_device) holding raw quantised LINEAR
 * sums.  It never clears the buffer: the caller zeroes it once.  d_moments (nullable, same size) additionally receives
 * the per-channel sums of quantize36(q * q) -- the input of tor_accum_noise_device (a launch without it runs the same
 * kernels as tor_render_device).  Row shards (shard_index / shard_count / row_tile) and every accel value work as in
 * tor_render_device.  Asynchronous on hip_stream, with the same one-stream-per-context rule; tor_last_kernel_ms and the
 * stats calls report this launch.  TOR_ERR_INVALID_ARGUMENT for TOR_SEED_PIXEL (a pixel is one sequential chain of
 * samples on one generator; resuming it would need per-pixel RNG state), first_sample < 0, n_samples < 1 and
 * first_sample + n_samples > 2^17 (131072): per-sample radiance is at most 1 per channel, so up to 2^17 samples the sums
 * stay multiples of 2^-36 below 2^17 -- integers up to 2^53 in units of 2^-36, exact in float64.  max_depth <= 0 and an
 * empty scene add zeros: d_sums / d_moments are left untouched.
 *
 * tor_resolve_device: d_pixels[i] = pow(d_sums[i] / total_samples, 1 / gamma_correction) for n_values float64 (exactly
 * Canvas.draw's operations, canvas.nim:47-54); d_sums is left as it is (d_pixels == d_sums resolves in place).
 * 1 <= total_samples <= 2^17.  Asynchronous on hip_stream.
 *
 * tor_accum_noise_device: from sums S, moments M of total_samples = N >= 2 samples, each channel's standard error of the
 * mean sqrt(max(0, (M - S*S/N) / (N - 1)) / N) in linear (pre-gamma) units; d_err (nullable, npix float64) receives the
 * per-pixel maximum over the three channels, out[0] / out[1] the frame's mean / maximum of it, reduced in a fixed order
 * (repeated calls return the same bits).  A channel whose sum is NaN or infinite reports 0 (max(0, .) takes a NaN variance to
 * 0), an infinite moment beside a finite sum inf; no NaN is reported.  Blocking: returns when out is filled.  (The formula needs S, M and N only: the
 * raw moments of tor_render_resume_device and tor_render_resume_list_device are served as they are.) */
TOR_API int tor_render_accumulate_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                                         int32_t first_sample, int32_t n_samples, int64_t max_depth,
                                         const TorOptions* opt, double* d_sums, double* d_moments, void* hip_stream);
TOR_API int tor_resolve_device(TorContext* ctx, const double* d_sums, int64_t n_values, int64_t total_samples,
                               float gamma_correction, double* d_pixels, void* hip_stream);
TOR_API int tor_accum_noise_device(TorContext* ctx, const double* d_sums, const double* d_moments, int64_t npix,
                                   int64_t total_samples, double* d_err, double out[2], void* hip_stream);

/* ---- resumable rendering on the reference's per-pixel streams (TOR_SEED_PIXEL only) -------------------------------------
 * render.nim:59-67 gives every pixel ONE generator, seeded from (row, col), draws the pixel's spp samples from it one after
 * the other and sums them in float64 in that order.  The first k samples do not depend on spp (it only enters Canvas.draw's
 * final scale), so a pixel that has run k samples and kept {generator state, raw sum} IS the reference's pixel at k spp and
 * goes on being the reference's pixel at any n > k.  tor_render_resume_device makes that state three caller-owned DEVICE
 * buffers in the shard's compact row layout of tor_render_device (shard_index / shard_count / row_tile work as there):
 *   d_rng      one TorRng per pixel: the state the reference's `var Rng` of that pixel has after the samples run so far
 *   d_sums     3 float64 per pixel: the RAW sequential sum ((0 + c0) + c1) + ... of render.nim:67 -- not quantised, not scaled
 *   d_moments  (nullable) 3 float64 per pixel: the sequential float64 sum of c * c per channel (one rounding for the
 *              product, one for the add, nothing fused) -- the input of tor_accum_noise_device, whose formula only needs
 *              S, M and N and serves this mode as it is
 * first_sample == 0 STARTS the pixels: the kernel seeds seed2(row, col) itself and starts the sums at 0 -- none of the three
 * buffers is read, none needs clearing.  first_sample > 0 CONTINUES them: every pixel loads its state and sums, runs
 * n_samples more samples of the same stream and stores both back.  The library cannot check that the buffers really hold
 * first_sample samples of this camera, scene and size: a caller that passes anything else gets a different image, not an error.
 * After any sequence of calls that covers [0, n), d_sums holds the same bits as the raw sums of a one-shot tor_render_device
 * with samples_per_pixel = n before its finalize, and tor_resolve_device(d_sums, ..., total_samples = n, gamma) gives that
 * call's canvas bit for bit (it performs Canvas.draw's operations, canvas.nim:47-54).
 * No draw is ever skipped: with max_depth <= 0 and with an empty scene the reference still draws the pixel jitter and the
 * camera's lens and time samples of every sample (render.nim:63-65, cameras.nim:47-57), the states advance exactly so, and
 * an empty scene's sky colours depend on them.  (tor_render_accumulate_device may leave its buffers untouched in those cases
 * because its streams are stateless; this entry never does.)
 * Every accel value and every pixel_kernel value is accepted and gives the same bits.  LANE runs the one-lane-per-pixel kernel
 * (tor_debug_last_variant: seeding 5, or 6 with d_moments), WAVE the one-wave-per-pixel kernel; AUTO picks as tor_render_device
 * does from the pass's n_samples (cost probe and tile order from 32 samples per pass, shared frames, wave kernel on small
 * frames) with ONE exception: a resume pass never uses the chain hand-off.  A stalled hand-off launch leaves holes
 * (tor_context_handoff_stalled); here the state lives in place, so the holes would be pixels still at first_sample next to
 * pixels already at first_sample + n_samples, and the pass could not be repeated.  Frames that tor_render_device would hand
 * off are shared between the two kernels instead (tor_debug_last_split_tiles says how) or run one lane per pixel; tor_context_handoff_stalled therefore
 * always reports 0 after this entry and no re-render rule applies to it.
 * Asynchronous on hip_stream, with the one-stream-per-context rule of the other render entries; tor_last_kernel_ms and the
 * stats calls report this launch.  TOR_ERR_INVALID_ARGUMENT, nothing written: opt->seeding != TOR_SEED_PIXEL (sample streams:
 * tor_render_accumulate_device), first_sample < 0, n_samples < 1, first_sample + n_samples > 2^17 (131072 -- NOT an exactness
 * bound here: it is the range tor_resolve_device and tor_accum_noise_device accept, so that both serve this mode unchanged),
 * NULL d_rng / d_sums, nrows < 2 or ncols < 2, a context without a scene upload. */
struct TorRng;  /* defined with the radiance queries below: Rng -- support/rng.nim:18-19, 4 x uint64 */
TOR_API int tor_render_resume_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                                     int32_t first_sample, int32_t n_samples, int64_t max_depth, const TorOptions* opt,
                                     struct TorRng* d_rng, double* d_sums, double* d_moments, void* hip_stream);

/* ---- adaptive sampling (TOR_SEED_SAMPLE only): samples where the noise is ------------------------------------------------
 * An adaptive render is a sequence of passes over a shrinking ACTIVE LIST of pixels.  Every listed pixel holds exactly N samples
 * [0, N) before a pass and receives the same range [N, N + k); a select then tests each listed pixel at N + k samples, records
 * counts[p] = N + k and keeps the unconverged ones, in input order, for the next pass.  So each pixel's samples are a prefix
 * [0, counts[p]), and -- every deposit being exact (progressive block above) -- pixel p of an adaptive render is pixel p of a
 * uniform counts[p]-spp render, bit for bit, whatever the schedule.
 *
 * tor_render_accumulate_list_device: tor_render_accumulate_device over the n_list pixels of d_list only (DEVICE int32,
 * shard-local indices in d_sums' layout, strictly ascending, unique -- ascending keeps neighbouring pixels in one wave).  Sums
 * AND moments are required.  n_list == 0 is a no-op.  An entry outside the shard deposits nothing.  The same rejections as
 * tor_render_accumulate_device (TOR_SEED_PIXEL -- listed passes on the reference's streams are tor_render_resume_list_device's,
 * below --, sample ranges, the 2^17 bound), and n_list < 0 or above the shard's pixel count.  Asynchronous on hip_stream.
 *
 * tor_adaptive_select_device: the convergence test at total_samples = n (2 <= n <= 2^17) of every listed pixel.  Per channel
 * c, mean_c = S_c / n and se_c = sqrt(max(0, (M_c - S_c*S_c/n) / (n - 1)) / n) -- tor_accum_noise_device's standard error --
 * each operation one IEEE float64 rounding, nothing fused; the pixel has converged iff se_c <= abs_tol + rel_tol * mean_c for
 * all three channels.  d_counts[p] = n for every listed p (npix int32, the sample map), the unconverged pixels to d_list_out in
 * input order (an ordered compaction: d_list_out must not alias d_list_in), their number to *n_out.  Every entry must be a pixel
 * of d_sums.  abs_tol, rel_tol >= 0, not NaN.  A channel whose sum is NaN or infinite has se_c = 0 there: the pixel never
 * converges when that makes the right-hand side NaN or -inf (a NaN sum; -inf; +inf with rel_tol = 0), and a sum of +inf with
 * rel_tol > 0 counts as converged.  n_in == 0 gives *n_out = 0.  Blocking: returns when *n_out is known.  It reads
 * S, M and n only, so it serves the raw sums and moments of tor_render_resume_list_device (TOR_SEED_PIXEL) as it is.
 *
 * tor_resolve_counts_device: d_pixels[i] = pow(d_sums[i] / counts[i / 3], 1 / gamma_correction) for npix pixels, computed as
 * (1.0 / counts) * sum -- tor_resolve_device's operations with total_samples = counts[i / 3], so the same bits.  Every count
 * must lie in [1, 2^17]; the counts live on the device, so one outside is not rejected and gives what the arithmetic gives: a
 * count of 0 (scale inf) inf for a positive sum and NaN for a sum of 0, a negative count NaN for a positive sum and 0 for a
 * sum of 0.  d_pixels == d_sums resolves in place.  Asynchronous on hip_stream.  On the raw sums of
 * tor_render_resume_list_device it gives, per pixel, the reference's pixel at counts[p] samples per pixel. */
TOR_API int tor_render_accumulate_list_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                                              const int32_t* d_list, int32_t n_list, int32_t first_sample, int32_t n_samples,
                                              int64_t max_depth, const TorOptions* opt, double* d_sums, double* d_moments,
                                              void* hip_stream);
TOR_API int tor_adaptive_select_device(TorContext* ctx, const double* d_sums, const double* d_moments, const int32_t* d_list_in,
                                       int32_t n_in, int64_t total_samples, double abs_tol, double rel_tol, int32_t* d_list_out,
                                       int32_t* d_counts, int32_t* n_out, void* hip_stream);
TOR_API int tor_resolve_counts_device(TorContext* ctx, const double* d_sums, const int32_t* d_counts, int64_t npix,
                                      float gamma_correction, double* d_pixels, void* hip_stream);

/* ---- adaptive sampling on the reference's per-pixel streams (TOR_SEED_PIXEL only) ----------------------------------------
 * tor_render_resume_list_device: tor_render_resume_device over the n_list pixels of d_list only.  The list rules are
 * tor_render_accumulate_list_device's: DEVICE int32, shard-local indices in the compact row layout, strictly ascending and
 * unique; an entry outside the shard is skipped -- nothing read, nothing written, nothing drawn; n_list == 0 is a no-op.
 * first_sample == 0 STARTS the listed pixels (the kernel seeds seed2(row, col) and zeroes the sums itself; the buffers are not
 * read for them), first_sample > 0 CONTINUES them from their stored state.  A pixel that is NOT listed keeps every bit of its
 * d_rng, d_sums and d_moments.  d_rng, d_sums and d_moments are all required (the moments are what the select reads).  No draw
 * is skipped for max_depth <= 0 or an empty scene, exactly as in tor_render_resume_device.
 * The guarantee: after passes over lists such that listed pixel p has received exactly the prefix [0, counts[p]) of its stream,
 * tor_resolve_counts_device(d_sums, d_counts, ...) gives, per pixel, the canvas value of a one-shot tor_render_device with
 * TOR_SEED_PIXEL and samples_per_pixel = counts[p] -- which is also the CPU oracle's value and the unmodified reference
 * program's -- bit for bit, for every accel and every pixel_kernel value.  tor_adaptive_select_device, tor_resolve_counts_device
 * and tor_accum_noise_device serve this mode unchanged.
 * Kernels: LANE runs the one-lane-per-pixel kernel over tiles of 64 consecutive list slots (tor_debug_last_variant: seeding 7),
 * WAVE the one-wave-per-pixel kernel with one list slot per work item (LANE when the scene does not fit LDS); AUTO applies
 * tor_render_device's rule with n_list in place of the pixel count and three quarters of its threshold: the wave kernel up to
 * 3/4 x TOR_COOP_MAX_PIXELS (86 016) listed pixels, the lane kernel above (measured: DESIGN 4.12).  A listed pass runs no cost
 * probe, no tile ordering and no split mode (tor_debug_last_split_tiles gives 0) and, like every resume pass, no chain hand-off:
 * tor_context_handoff_stalled reports 0 afterwards.
 * Asynchronous on hip_stream, with the one-stream-per-context rule of the other render entries (a pass on a second stream while
 * one is in flight is refused before any state moves); tor_last_kernel_ms and the stats calls report this launch.
 * TOR_ERR_INVALID_ARGUMENT, nothing written: everything tor_render_resume_device rejects, NULL d_list with n_list > 0, NULL
 * d_moments, n_list < 0 or above the shard's pixel count. */
TOR_API int tor_render_resume_list_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                                          const int32_t* d_list, int32_t n_list, int32_t first_sample, int32_t n_samples,
                                          int64_t max_depth, const TorOptions* opt, struct TorRng* d_rng, double* d_sums,
                                          double* d_moments, void* hip_stream);

/* ---- closest-hit queries: `hit()` of the uploaded list for the caller's rays ---------------------------------------------
 * Every Hittable provides hit(r, t_min, t_max, rec) (physics/core.nim:38-42); these entries answer batches of rays with the uploaded
 * list's (hittables_lists.nim:48-55 over spheres.nim:28-49 / moving_spheres.nim:39-67), bit for bit: for each ray the record of
 * world.hit(r, t_min, t_max, rec) on the caller's list in list order.
 *   t        the first root (-half_b - sqrt(disc)) / a if it lies in (t_min, t_max), else the second root if that one does; over the
 *            list: the smallest accepted root, ties to the lowest index (the sequential closest_so_far loop, reduced)
 *   p        origin + direction * t (rays.nim:24-25); normal = outward = (p - center(time)) * (1.0 / radius) (vec3s.nim:93-94), negated
 *            when front_face = 0; front_face = dot(direction, outward) < 0 (core.nim:47-49); moving centres as moving_spheres.nim:39-44
 *   object   the winner's index in the uploaded list (the reference's rec.material); a miss: object = -1, every other field 0
 * Float64 throughout, unfused, correctly rounded `/` and sqrt.  Zero directions, NaN times, t_max = +inf, movers with time0 == time1,
 * negative radii and an empty list all go through the reference's arithmetic and give its answer.
 *
 * tor_hit_device: n_rays DEVICE rays (TorRay) -> d_hits (n_rays TorHit, DEVICE).  d_t_range (nullable, DEVICE): 2 float64 per ray
 * {t_min, t_max}; NULL = render.nim's (0.001, +inf).  Asynchronous on hip_stream, with the one-stream-per-context rule of the render
 * entries.  [time_lo, time_hi] is the ray-time range the block bounds are built for (cached per scene and range) -- a speed hint only:
 * a ray whose time lies outside it (or is NaN) is answered by the brute-force walk.  The blocks also need t_min >= 0 (their slab test
 * clips at 0) and an origin within the reach of the boxes' margin: far from the scene the reference's own discriminant rounds by ~eps
 * |origin - centre|^2 and accepts rays that pass outside a sphere by more than its box's inflation (reach = sqrt(r_min * 1e-6 /
 * (64 eps)) minus the objects' extent: ~5300 units for spheres of radius 0.2).  Rays that miss any of these conditions are answered by
 * the brute-force walk, so every result is exact whatever the hint.  mode: TOR_HIT_AUTO (blocks when the scene has a culling layout
 * and the range has finite bounds, else brute force; tor_last_note() says which ran: "hit: blocks" | "hit: brute force (...)"),
 * TOR_HIT_BRUTE, TOR_HIT_BLOCKS (falls back to brute force as AUTO does).  TOR_ERR_INVALID_ARGUMENT for n_rays < 0, a context without a scene, a non-finite or inverted time range and a
 * mode outside 0..2.  n_rays == 0 is a no-op.
 * tor_hit_host: the same on host arrays, blocking (copy in, query, copy out) -- what a Nim host's {.importc.} shim calls.  It first
 * waits for the context's last render launch and last query, on whatever stream they run (it does not refuse another stream). */
typedef struct TorRay { TorVec3 origin, direction; double time; } TorRay;  /* Ray -- primitives/rays.nim (56 B) */
/* HitRecord -- physics/core.nim:30-36; the material is replaced by the object's index in the uploaded list (64 B) */
typedef struct TorHit { TorVec3 p, normal; double t; int32_t object; int32_t front_face; } TorHit;
enum { TOR_HIT_AUTO = 0, TOR_HIT_BRUTE = 1, TOR_HIT_BLOCKS = 2 };
TOR_API int tor_hit_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo,
                           double time_hi, int32_t mode, TorHit* d_hits, void* hip_stream);
TOR_API int tor_hit_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo, double time_hi,
                         int32_t mode, TorHit* hits);

/* ---- radiance queries: render.nim's radiance() and the camera's rays for rays and RNG states the caller supplies ------------------
 * tor_radiance_device: color[i] = radiance(rays[i], world, max_depth, rng[i]) (render.nim:21-47) on the uploaded list, bit for bit, and
 * rng[i] is left where the reference leaves its `var Rng` after the call.  Every bounce is world.hit(r, 0.001, +inf, rec)
 * (render.nim:28) as tor_hit_device answers it, then the material's scatter (materials.nim:21-96) with the reference's draws in the
 * reference's order: Lambertian keeps the ray's time; Metal and Dielectric give the scattered ray time 0 (rays.nim:19's default); an
 * absorbed Metal ray is black; a miss is the sky 0.5 * y + 1.0 (sic, render.nim:42) of the unit direction times the attenuation; a
 * path still bouncing after max_depth hits is black.  The colour is the unquantised float64 in the reference's operation order:
 * unfused, `Vec3 / s` as `* (1.0 / s)`, correctly rounded `/` and sqrt, the portable sin/cos and pow of the GPU integrator.
 * max_depth == 0 gives black and draws nothing; an empty scene gives the sky and draws nothing.  d_rays (n_rays TorRay), d_rng
 * (n_rays TorRng, read and written) and d_color (n_rays * 3 float64) are DEVICE arrays; the states may be any the caller holds
 * (seed1 / seed2 / seed3 of support/rng.nim, or what tor_camera_rays_device left).  mode and [time_lo, time_hi] work as in
 * tor_hit_device, and tor_last_note() says what ran ("radiance: blocks" | "radiance: brute force (...)"); as scattered Metal and
 * Dielectric rays carry time 0, the library widens the range to include 0 before it builds or looks up the cached block bounds.
 * Asynchronous on hip_stream, one stream per context as for the hit queries; a query leaves every render state alone.
 * TOR_ERR_INVALID_ARGUMENT for what tor_hit_device refuses and for max_depth < 0; n_rays == 0 is a no-op.
 * tor_radiance_host: the same on host arrays, blocking (copy in, query, copy out; rng updated in place) -- for a Nim shim, which
 * casts its Rng (whose fields are private) to a TorRng.
 *
 * tor_camera_rays_device: the library's camera rays (render.nim:63-65 + cameras.nim:47-57) for listed pixels: per pixel (row, col)
 * and sample, u = (col + U) / (ncols - 1), v = (row + U) / (nrows - 1), cam.ray(u, v, rng), from the stream below; writes the ray
 * and the state after the camera's draws -- ready for tor_radiance_device.
 *   d_pixels  DEVICE int32 flat pixel indices row * ncols + col (row 0 = bottom), n_pixels of them; NULL = every pixel, row-major
 *             (n_pixels must then be nrows * ncols).  Entries outside [0, nrows * ncols) are skipped: their rays and states are not
 *             written.
 *   TOR_SEED_SAMPLE  seed3(row, col, s) for s in [first_sample, first_sample + n_samples) (the per-sample streams of
 *                    tor_render_accumulate_device); d_rng is output only; entry e, sample s at index e * n_samples + (s - first_sample)
 *                    of d_rng and d_rays.
 *   TOR_SEED_PIXEL   n_samples == 1 (first_sample is ignored); d_rng is read and written per listed pixel: the caller seeds
 *                    seed2(row, col) once and passes the states tor_radiance_device left -- the reference's one stream per pixel.
 * Asynchronous on hip_stream; it reads no scene and no other state of the context.  TOR_ERR_INVALID_ARGUMENT for nrows or ncols
 * below 2, n_pixels < 0, first_sample < 0, n_samples < 1, first_sample + n_samples above 2^31 - 1, another seeding, NULL pointers. */
typedef struct TorRng { uint64_t s0, s1, s2, s3; } TorRng;  /* Rng -- support/rng.nim:18-19, xoshiro256+ (32 B) */
TOR_API int tor_radiance_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, TorRng* d_rng, int32_t max_depth,
                                double time_lo, double time_hi, int32_t mode, double* d_color, void* hip_stream);
TOR_API int tor_radiance_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, TorRng* rng, int32_t max_depth, double time_lo,
                              double time_hi, int32_t mode, double* color);
TOR_API int tor_camera_rays_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, const int32_t* d_pixels,
                                   int64_t n_pixels, int32_t first_sample, int32_t n_samples, int32_t seeding, TorRng* d_rng,
                                   TorRay* d_rays, void* hip_stream);

/* ---- path steps: one iteration of radiance()'s loop, the scatter alone, the sky and the list of the rays that go on ---------------
 * For hosts that write their own integrator (own sky or environment map, emissive objects picked by `object`, feature buffers of
 * any bounce, Russian roulette) and keep the reference's physics and draws.  Arrays are indexed by the RAY, not by the position in
 * the list: a host keeps full-size arrays and a shrinking list and never moves a ray.  d_list (DEVICE int32, n_list entries; NULL:
 * every ray, n_list must be n_rays) names the rays a call works on; entries outside [0, n_rays) are skipped (nothing read, nothing
 * written); entries must be unique (duplicates are the caller's race); rays that are not listed are untouched in every array.
 * n_list == 0 and n_rays == 0 are no-ops.
 *
 * tor_bounce_device: per listed ray i one iteration of render.nim:26-38 -- world.hit(rays[i], 0.001, +inf, rec), then
 * rec.material.scatter(rays[i], rec, rng[i], attenuation, scattered) (materials.nim:21-96) -- bit for bit:
 *   d_hits[i]         what tor_hit_device writes for rays[i] with d_t_range = NULL (a miss: object = -1, the rest 0)
 *   miss              status TOR_BOUNCE_MISS, attenuation 0, ray and state untouched, nothing drawn
 *   hit               the winner's material scatters with the reference's draws in the reference's order (float64 unfused, the
 *                     portable sin/cos and pow5 of tor_radiance_device); d_rays[i] becomes `scattered`: origin rec.p, Lambertian
 *                     keeps r_in.time, Metal and Dielectric write time 0 (rays.nim:19) -- written for an absorbed Metal ray too, as
 *                     materials.nim:41 writes it before the test; d_rng[i] is the state after the scatter's last draw
 *   d_attenuation[i]  3 float64: the albedo (Lambertian, scattered Metal), (1, 1, 1) (Dielectric), 0 (absorbed: the reference
 *                     leaves it unset); status TOR_BOUNCE_SCATTERED | TOR_BOUNCE_ABSORBED
 * Driven as render.nim drives it (att = 1; per step att *= attenuation; a miss ends with tor_sky_device's colour * att, an
 * absorbed ray with black; max_depth steps, then black) the steps give tor_radiance_device's colours and states, bit for bit.
 * mode and [time_lo, time_hi] work as in tor_hit_device (a speed hint only); the library widens the range to include 0 as
 * tor_radiance_device does, so a chain of steps called with one range uses ONE cached set of block bounds.  tor_last_note():
 * "bounce: blocks" | "bounce: brute force (...)".  An empty scene gives all misses and draws nothing.  Asynchronous on hip_stream,
 * one stream per context as for the other queries; a step leaves every render state alone.  TOR_ERR_INVALID_ARGUMENT (nothing
 * written) for what tor_hit_device refuses, n_list < 0, a NULL list with n_list != n_rays, NULL arrays.
 *
 * tor_scatter_device: the second half alone, from the caller's records: the material of d_hits[i].object, and p, normal,
 * front_face as given (a host may have perturbed the normal, or taken the record from geometry of its own); t is not read.  An
 * object outside [0, n_objects) counts as a miss.  tor_bounce_device equals tor_hit_device followed by tor_scatter_device, bit for
 * bit.  tor_last_note(): "scatter".
 * tor_bounce_host / tor_scatter_host: the same on host arrays, blocking (every array copied in, the step, the outputs copied
 * out) -- what a Nim shim's {.importc.} calls; they wait for the context's last render launch and last query as tor_hit_host does.
 *
 * tor_sky_device: d_color[i] (3 float64) = render.nim:41-44 without the attenuation for each listed ray:
 * (1 - t) * white + t * (0.5, 0.7, 1.0) with t = 0.5 * unit_vector(direction).y + 1.0 (sic).  Asynchronous.  It reads no scene
 * and no other state of the context (as tor_camera_rays_device), so the one-stream rule does not apply to it.  Note: "sky".
 *
 * tor_bounce_select_device: ordered compaction -- the entries of d_list_in (NULL: 0 .. n_in - 1, n_in must be n_rays) that lie in
 * [0, n_rays) and whose d_status is TOR_BOUNCE_SCATTERED, in input order, to d_list_out (room for n_in entries, not d_list_in
 * itself); *n_out (HOST) = how many.  Blocking on hip_stream, as tor_adaptive_select_device; its scratch is the context's, so the
 * one-stream rule of the other queries holds for it.  n_rays and n_in at most 2^31 - 1.  Note: "bounce select". */
enum { TOR_BOUNCE_MISS = 0, TOR_BOUNCE_SCATTERED = 1, TOR_BOUNCE_ABSORBED = 2 };
TOR_API int tor_bounce_device(TorContext* ctx, int64_t n_rays, TorRay* d_rays, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                              double time_lo, double time_hi, int32_t mode, TorHit* d_hits, double* d_attenuation,
                              int32_t* d_status, void* hip_stream);
TOR_API int tor_bounce_host(TorContext* ctx, int64_t n_rays, TorRay* rays, TorRng* rng, const int32_t* list, int64_t n_list,
                            double time_lo, double time_hi, int32_t mode, TorHit* hits, double* attenuation, int32_t* status);
TOR_API int tor_scatter_device(TorContext* ctx, int64_t n_rays, TorRay* d_rays, const TorHit* d_hits, TorRng* d_rng,
                               const int32_t* d_list, int64_t n_list, double* d_attenuation, int32_t* d_status, void* hip_stream);
TOR_API int tor_scatter_host(TorContext* ctx, int64_t n_rays, TorRay* rays, const TorHit* hits, TorRng* rng, const int32_t* list,
                             int64_t n_list, double* attenuation, int32_t* status);
TOR_API int tor_sky_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const int32_t* d_list, int64_t n_list,
                           double* d_color, void* hip_stream);
TOR_API int tor_bounce_select_device(TorContext* ctx, int64_t n_rays, const int32_t* d_status, const int32_t* d_list_in, int64_t n_in,
                                     int32_t* d_list_out, int64_t* n_out, void* hip_stream);

/* ---- any-hit queries: is anything in the way?  One bit per shadow ray ----------------------------------------------------------
 * A host that treats objects as emitters casts shadow rays towards them and keeps one bit of each answer.  These entries give
 * that bit without the closest hit's cost: no smallest root, no record, 4 bytes out per ray, and the kernel stops at the first
 * accepted root.  The bit is the reference's, exactly: HittableList.hit (hittables_lists.nim:48-55) returns hit_anything, and the
 * closest_so_far it shrinks on the way only rejects roots of later objects after an earlier one has been accepted, so
 *   occluded(r, t_min, t_max) = OR over the list of Sphere.hit / MovingSphere.hit(r, t_min, t_max)
 * (spheres.nim:28-49, moving_spheres.nim:39-67), in any visiting order and under any early exit.
 *
 * tor_occluded_device: d_occluded[i] (DEVICE int32, one per ray, indexed by the ray) = 1 iff world.hit(rays[i], t_min, t_max, rec)
 * returns true on the uploaded list, else 0.  d_t_range (nullable, DEVICE): 2 float64 per ray {t_min, t_max}, indexed by the ray;
 * NULL = render.nim's (0.001, +inf).  A shadow segment from p to q is origin p, direction q - p, range (0.001, 1.0); both
 * comparisons are strict, as in the reference.  d_list / n_list follow the path steps' rules: NULL = every ray (n_list must be
 * n_rays); entries outside [0, n_rays) are skipped (nothing read, nothing written); entries must be unique; rays that are not
 * listed keep every bit of d_occluded; n_list == 0 and n_rays == 0 are no-ops.  mode and [time_lo, time_hi] work as in
 * tor_hit_device (a speed hint only): a ray whose time lies outside the range (or is NaN), whose t_min is not >= 0, whose origin
 * lies beyond the reach of the boxes' margin or whose |direction|^2 is below its floor walks every spatial slot instead, so every
 * bit is exact whatever the hint.  With the blocks a box the segment ends in front of is not entered, so short segments cost
 * little.  tor_last_note(): "occluded: blocks" | "occluded: brute force (...)".  Asynchronous on hip_stream, one stream per
 * context as for the other queries; a query leaves every render state alone.  TOR_ERR_INVALID_ARGUMENT (nothing written) for
 * what tor_hit_device refuses, n_list < 0, a NULL list with n_list != n_rays, NULL rays or output with work to do.
 * WHICH object occludes a ray is not exposed: with the early exit it depends on the visiting order, so the reference does not
 * define it (tor_hit_device answers that question).
 * tor_occluded_host: the same on host arrays, blocking (every array copied in, the query, the output copied out); it waits for
 * the context's last render launch and last query as tor_hit_host does. */
TOR_API int tor_occluded_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                                int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* d_occluded, void* hip_stream);
TOR_API int tor_occluded_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                              int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* occluded);

/* ---- visibility groups and per-ray masks: the hit, any-hit and step queries on a sub-list of the scene --------------------------
 * Shadow rays that skip glass, shadow segments towards a lamp that ignore the lamp, lamps the camera does not see: every object
 * of the uploaded list carries a 32-bit GROUP word, every ray of a masked query a 32-bit MASK, and
 *   object j takes part for ray i  iff  groups[j] & mask_i != 0.
 * The meaning is exact in the reference's terms: a masked query is world.hit(r, t_min, t_max, rec) (hittables_lists.nim:48-55) on
 * the sub-list of the objects the ray sees, in list order.  Each masked entry equals its unmasked entry on a context that
 * uploaded only those objects, bit for bit, with `object` reported as the index in the FULL list; so ties go to the lowest
 * visible index.  A ray with mask 0 misses (object = -1, the rest 0), is not occluded, and its step has status
 * TOR_BOUNCE_MISS, draws nothing and leaves ray and state untouched.
 *
 * tor_scene_groups: one word per object of the uploaded list, in list order, from a HOST array.  groups == NULL resets every
 * object to 0xFFFFFFFF: the state after every tor_scene_upload that replaces the scene (an upload of a byte-identical list is a
 * no-op and keeps the words).  n_objects must equal the uploaded count: otherwise, and for a context without a scene,
 * TOR_ERR_INVALID_ARGUMENT and nothing changes.  The call waits for the context's last query before it replaces the words.  The
 * render entries and the unmasked queries never read them.
 *
 * tor_hit_masked_device / tor_occluded_masked_device / tor_bounce_masked_device: the arguments of tor_hit_device /
 * tor_occluded_device / tor_bounce_device, then d_mask (nullable, DEVICE: one word per ray, indexed by the ray as every other
 * per-ray array is) and mask (the mask of every ray when d_mask is NULL; ignored otherwise).  tor_bounce_masked_device scatters off
 * the visible winner with the reference's draws; its d_hits is tor_hit_masked_device's.  Lists, d_t_range, mode, the time-range
 * hint, the walk of the rays the boxes do not hold for, the one-stream rule and the refusals are the unmasked entries'.  With the
 * blocks a ray does not enter a box that holds nothing it sees.  tor_last_note(): "hit (masked): blocks" | "hit (masked): brute
 * force (...)", and likewise "occluded (masked): ..." and "bounce (masked): ...".
 * tor_hit_masked_host / tor_occluded_masked_host: the same on host arrays (masks: nullable, HOST), blocking, as tor_hit_host. */
TOR_API int tor_scene_groups(TorContext* ctx, int64_t n_objects, const uint32_t* groups);
TOR_API int tor_hit_masked_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, double time_lo,
                                  double time_hi, int32_t mode, TorHit* d_hits, void* hip_stream, const uint32_t* d_mask, uint32_t mask);
TOR_API int tor_hit_masked_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, double time_lo,
                                double time_hi, int32_t mode, TorHit* hits, const uint32_t* masks, uint32_t mask);
TOR_API int tor_occluded_masked_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range,
                                       const int32_t* d_list, int64_t n_list, double time_lo, double time_hi, int32_t mode,
                                       int32_t* d_occluded, void* hip_stream, const uint32_t* d_mask, uint32_t mask);
TOR_API int tor_occluded_masked_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                                     int64_t n_list, double time_lo, double time_hi, int32_t mode, int32_t* occluded,
                                     const uint32_t* masks, uint32_t mask);
TOR_API int tor_bounce_masked_device(TorContext* ctx, int64_t n_rays, TorRay* d_rays, TorRng* d_rng, const int32_t* d_list,
                                     int64_t n_list, double time_lo, double time_hi, int32_t mode, TorHit* d_hits,
                                     double* d_attenuation, int32_t* d_status, void* hip_stream, const uint32_t* d_mask, uint32_t mask);

/* ---- ordered multi-hit queries: the first K surface crossings of a ray, in order ------------------------------------------------
 * Transparent shadows (which surfaces a segment crosses, how long it runs inside glass), depth peeling and layered feature buffers,
 * thickness and inside / outside parity, picking through glass: one walk of the scene where K chained tor_hit_device launches with
 * a moving t_min take K walks and cannot tell two surfaces at the same t apart.
 * For ray r, range (t_min, t_max) and object j of the uploaded list the roots are the reference's (spheres.nim:29-48,
 * moving_spheres.nim:39-66): s0 = (-half_b - sqrt(disc)) / a and s1 = (-half_b + sqrt(disc)) / a when disc > 0 (strict), float64,
 * unfused, correctly rounded `/` and sqrt -- the arithmetic of tor_hit_device.
 *   crossing  a triple (t, object, which), one for EACH root with t_min < t < t_max (both strict, as in the reference): which = 0
 *             for s0, 1 for s1; both roots of one object count; NaN and infinite roots are no crossings
 *   order     t ascending, compared as doubles; equal t: the lower object first, then which 0 before 1
 *   result    d_cross[i * k + m], m < d_count[i] = min(total, k): the first crossings in that order; entries d_count[i] .. k - 1
 *             hold t = 0, object = -1, which = 0.  A host that must know whether MORE than k crossings exist asks for k + 1.
 *   records   d_records (nullable, DEVICE): one TorHit per stored crossing, d_records[i * k + m]: p = origin + direction * t
 *             (rays.nim:24-25), normal and front_face by tor_hit_device's formula for that (t, object) (vec3s.nim:93-94,
 *             core.nim:47-49; negative radii go through it as they are); unused entries hold the miss record (object = -1, the rest 0)
 * 1 <= k <= TOR_CROSSINGS_MAX.  Bit for bit: crossing 0 and its record are tor_hit_device's answer and d_count[i] == 0 exactly on a
 * miss; d_count[i] > 0 is tor_occluded_device's bit; on a ray without equal-t crossings, crossing m + 1 is what tor_hit_device
 * returns with t_min := crossing m's t.
 * Visibility groups: with d_mask (nullable, DEVICE: one word per ray, indexed by the ray) or mask (the mask of every ray when d_mask
 * is NULL) object j takes part for ray i iff groups[j] & mask_i != 0 (tor_scene_groups); `object` is the index in the FULL list; a
 * ray with mask 0 has no crossings.  d_mask == NULL with mask == 0xFFFFFFFF is the unmasked query: it neither builds nor reads any
 * group state.
 * d_t_range (nullable, DEVICE): 2 float64 per ray {t_min, t_max}; NULL = render.nim's (0.001, +inf).  d_list / n_list follow
 * tor_occluded_device's rules: NULL = every ray (n_list must be n_rays); entries outside [0, n_rays) are skipped; entries must be
 * unique; rays that are not listed keep what d_cross, d_count and d_records hold; n_list == 0 and n_rays == 0 are no-ops.  mode and
 * [time_lo, time_hi] work as in tor_hit_device (a speed hint only): rays the boxes do not hold for walk every spatial slot, so every
 * result is exact whatever the hint.  With the blocks a box is entered only while its entry lies at or below the k-th crossing found
 * so far, so small k costs little.  tor_last_note(): "crossings: blocks" | "crossings: brute force (...)" ("crossings (masked): ..."
 * with masks).  Asynchronous on hip_stream, one stream per context as for the other queries; a query leaves every render state
 * alone.  TOR_ERR_INVALID_ARGUMENT (nothing written) for n_rays < 0, k outside 1 .. TOR_CROSSINGS_MAX, a context without a scene, a
 * non-finite or inverted time range, a mode outside 0..2, n_list < 0, a NULL list with n_list != n_rays, NULL d_rays, d_cross or
 * d_count with work to do.
 * tor_crossings_host: the same on host arrays (masks: nullable, HOST), blocking (every array copied in, the query, the outputs
 * copied out); it waits for the context's last render launch and last query as tor_hit_host does. */
enum { TOR_CROSSINGS_MAX = 16 };
typedef struct TorCrossing { double t; int32_t object; int32_t which; } TorCrossing;  /* 16 B */
TOR_API int tor_crossings_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                                 int64_t n_list, int32_t k, const uint32_t* d_mask, uint32_t mask, double time_lo, double time_hi,
                                 int32_t mode, TorCrossing* d_cross, int32_t* d_count, TorHit* d_records, void* hip_stream);
TOR_API int tor_crossings_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                               int64_t n_list, int32_t k, const uint32_t* masks, uint32_t mask, double time_lo, double time_hi,
                               int32_t mode, TorCrossing* cross, int32_t* count, TorHit* records);

/* ---- nearest-surface point queries: the K closest objects to a point ---------------------------------------------------------------
 * The one question of the query family that starts from a point, not a ray: which objects lie nearest to p at `time`, and how far
 * away are their surfaces -- the emitters within a radius of a shading point (light culling before the shadow rays; visibility
 * groups mark the emitters), a distance field for sphere tracing, proximity and contact shading, a contact test.
 * For point (p, time) and object j of the uploaded list:
 *     c  = the sphere's centre, or MovingSphere.center(time)   (moving_spheres.nim:39-44)
 *     oc = p - c
 *     d  = sqrt(oc.x*oc.x + oc.y*oc.y + oc.z*oc.z) - abs(radius)   (vec3s.nim:23-27 length; unfused float64, correctly rounded sqrt)
 *   distance    d is the signed distance to the surface, negative inside; a negative radius is a surface at abs(radius) (the
 *               hollow-glass idiom)
 *   neighbour   object j is a neighbour of the point iff d is finite and d < d_max (strict, as every range compare of this library);
 *               NaN and +-inf distances are no neighbours; d_max = NaN accepts nothing
 *   order       (d, object) ascending, d compared as a double; equal d: the lower index in the full list first
 *   result      d_near[i * k + m], m < d_count[i] = min(total, k): the first neighbours in that order as TorNear { distance, object,
 *               inside } with inside = d < 0; entries d_count[i] .. k - 1 hold {0, -1, 0}.  A host that must know whether MORE than
 *               k neighbours exist asks for k + 1.
 * Each neighbour is a function of the point and one object alone, so the first k of that set do not depend on the visiting order.
 * 1 <= k <= TOR_NEAREST_MAX.  d_max_dist (nullable, DEVICE): one float64 per point, indexed by the point; NULL = +inf.
 * Visibility groups: with d_mask (nullable, DEVICE: one word per point, indexed by the point) or mask (the mask of every point when
 * d_mask is NULL) object j takes part for point i iff groups[j] & mask_i != 0 (tor_scene_groups); `object` is the index in the FULL
 * list; a point with mask 0 has no neighbours.  d_mask == NULL with mask == 0xFFFFFFFF is the unmasked query: it neither builds nor
 * reads any group state.
 * Everything else follows tor_crossings_device with points in place of rays: d_list / n_list (NULL = every point, n_list must be
 * n_points; entries outside [0, n_points) are skipped; entries must be unique; points that are not listed keep what d_near and
 * d_count hold; n_list == 0 and n_points == 0 are no-ops), mode and [time_lo, time_hi] (a speed hint only: points the boxes do not
 * hold for -- a time outside the range or NaN, a position beyond the reach within which the boxes' margin covers the roundings --
 * walk every spatial slot, so every result is exact whatever the hint), the one-stream rule, and the refusals in the same order
 * (their messages name the point count n_rays).  With the blocks a box is entered only while its distance from the point lies at
 * or below the k-th neighbour found so far and below d_max; a box that holds the point is always entered (distances are signed).
 * TOR_HIT_AUTO runs the brute force where it measured faster: k > 4 without d_max_dist on a scene whose culling layout has one level.
 * tor_last_note(): "nearest: blocks" | "nearest: brute force (...)" ("nearest (masked): ..." with masks).  Asynchronous on hip_stream;
 * a query leaves every render state alone.  TOR_ERR_INVALID_ARGUMENT (nothing written) for n_points < 0, k outside 1 ..
 * TOR_NEAREST_MAX, a context without a scene, a non-finite or inverted time range, a mode outside 0..2, n_list < 0, a NULL list with
 * n_list != n_points, NULL d_points, d_near or d_count with work to do.
 * tor_nearest_host: the same on host arrays (max_dist, masks: nullable, HOST), blocking (every array copied in, the query, the
 * outputs copied out); it waits for the context's last render launch and last query as tor_hit_host does. */
typedef struct TorPoint { TorVec3 p; double time; } TorPoint;  /* 32 B */
enum { TOR_NEAREST_MAX = 16 };
typedef struct TorNear { double distance; int32_t object; int32_t inside; } TorNear;  /* 16 B */
TOR_API int tor_nearest_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, const double* d_max_dist, const int32_t* d_list,
                               int64_t n_list, int32_t k, const uint32_t* d_mask, uint32_t mask, double time_lo, double time_hi,
                               int32_t mode, TorNear* d_near, int32_t* d_count, void* hip_stream);
TOR_API int tor_nearest_host(TorContext* ctx, int64_t n_points, const TorPoint* points, const double* max_dist, const int32_t* list,
                             int64_t n_list, int32_t k, const uint32_t* masks, uint32_t mask, double time_lo, double time_hi,
                             int32_t mode, TorNear* near, int32_t* count);

/* ---- exact sample deposits: the film of a host-written integrator ------------------------------------------------------------------
 * The open pipeline (tor_camera_rays_device, tor_radiance_device, the path steps) ends in per-ray colours; the exact film
 * (tor_render_accumulate_device's sums and moments, tor_resolve_device, tor_accum_noise_device, tor_adaptive_select_device,
 * tor_resolve_counts_device) is otherwise filled by the library's own integrator only.  tor_deposit_device is the deposit of that
 * integrator on its own: it ADDS the caller's samples to the caller's buffers in the progressive block's exact arithmetic, so a
 * host-written integrator gets sums that are reproducible, additive across passes, contexts and GPUs, and served by every entry
 * named above.  Camera rays of samples [a, b), tor_radiance_device and this entry with max_value = 1 give
 * tor_render_accumulate_device's d_sums and d_moments for [a, b), bit for bit.
 *   entries     i = 0 .. n - 1; with d_index (nullable, DEVICE int32) i = d_index[j], j < n_index (n_index is not read
 *               otherwise, but must not be negative).  A listed i outside [0, n) is skipped; a repeated i deposits again.
 *   pixel       p = d_pixel[i] (DEVICE int32), in d_sums' layout: the numbering of tor_render_accumulate_list_device's lists; for
 *               an unsharded frame tor_camera_rays_device's row * ncols + col.  A p outside [0, npix) deposits nothing and is not
 *               counted anywhere -- how a sharded caller drops the pixels of other shards.
 *   rejection   c = d_color[3 i .. 3 i + 2] (DEVICE float64).  The sample is rejected AS A WHOLE if any channel is NaN, +inf,
 *               -inf or < 0 (-0.0 is accepted): it deposits nothing and adds 1 to *d_rejected.
 *   deposit     otherwise per channel q = quantize36(min(c, max_value)) -- rounded to the nearest multiple of 2^-36, ties to
 *               even, as (x + 98304.0) - 98304.0 --; d_sums[3 p + ch] += q; d_moments[3 p + ch] += quantize36(q * q) (q * q one
 *               rounding, nothing fused: the moments of tor_render_accumulate_device); d_counts[p] += 1.
 *   buffers     d_sums (npix * 3 float64), d_moments (nullable, same size), d_counts (nullable, npix int32), d_rejected (nullable,
 *               ONE int64): DEVICE, added to, never cleared -- the caller zeroes them once.
 * 0 < max_value <= 128, not NaN -- derived, not chosen: quantize36 is exact for |x| < 2^15, so q * q <= 2^14 needs q <= 2^7.
 * Exactness, and with it independence of the order of the entries, of the split into calls and of the GPU, holds while every
 * pixel has received at most 2^17 / max(max_value, max_value^2) ACCEPTED samples, the samples the library's own passes put into
 * the same buffers included (max_value = 1: the progressive block's 2^17).  The library cannot check this: a caller that deposits
 * more gets sums that depend on the order, not an error.
 * Asynchronous on hip_stream.  It reads no scene and no other state of the context (as tor_camera_rays_device), so the one-stream
 * rule does not apply to it.  TOR_ERR_INVALID_ARGUMENT, nothing written, tested in this order: n < 0 or n_index < 0; NULL d_color,
 * d_pixel or d_sums with work to do; npix < 1; max_value outside (0, 128] or NaN.  n == 0, and a list with n_index == 0, are no-ops. */
TOR_API int tor_deposit_device(TorContext* ctx, int64_t n, const double* d_color, const int32_t* d_pixel, const int32_t* d_index,
                               int64_t n_index, double max_value, int64_t npix, double* d_sums, double* d_moments, int32_t* d_counts,
                               int64_t* d_rejected, void* hip_stream);

/* ---- multi-process hosts: one process per GPU, the framebuffer gather inside the library (RCCL) ----------
 * rank 0 calls tor_comm_unique_id and hands the 128 bytes to the other ranks by its own means (bench.py:
 * torch.distributed broadcast); every rank then calls tor_comm_init_rank on its context (ncclCommInitRank).
 * tor_render_gather_device = tor_render_device for shard (rank, world, opt->row_tile) + the gather of the row
 * shards over xGMI + a de-interleave kernel: d_frame (nrows*ncols*3 float64, rows in image order, DEVICE memory)
 * is complete on `root` (root >= 0: send/recv gather, each rank's own link to the root) or on every rank
 * (root < 0: ncclAllGather).  Asynchronous on hip_stream.  librccl.so.1 is loaded on first use (dlopen), the
 * library has no link-time dependency on it. */
TOR_API int tor_comm_unique_id(uint8_t id_out[128]);
TOR_API int tor_comm_init_rank(TorContext* ctx, const uint8_t id[128], int32_t rank, int32_t world);
TOR_API int tor_comm_destroy(TorContext* ctx);
/* ncclCommAbort: for a host whose watchdog saw a gather that does not complete (bench.py polls its stream with a deadline);
 * RCCL's kernels leave, the context has no communicator afterwards.  tor_comm_count: ranks of the communicator
 * (ncclCommCount), 0 without one. */
TOR_API int tor_comm_abort(TorContext* ctx);
TOR_API int tor_comm_count(TorContext* ctx, int32_t* ranks_out);
TOR_API int tor_render_gather_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                                     int32_t samples_per_pixel, float gamma_correction, int64_t max_depth,
                                     const TorOptions* opt, int32_t root, double* d_frame, void* hip_stream);

/* Chain hand-off of the last launch of `ctx` (TOR_SEED_PIXEL with both exact accelerations, DESIGN 4.7 (HISTORY 4.7-4.8)): the launch covers
 * the whole GPU and its waves wait for each other, so it assumes exclusive use of the device's compute units (hand-off
 * launches of ONE process are chained per device by the library; TOR_MIGRATE=0 turns the hand-off off).  If some of its
 * workgroups never become resident (another process's persistent kernel, a CU mask) the waiting waves give up after
 * TOR_SRV_STALL_S seconds without progress (default 60, 0 = never) and the frame is INCOMPLETE: tor_render / tor_render_opt /
 * tor_render_frame_h264 notice and render the frame again without the hand-off; a caller of the asynchronous
 * tor_render_device asks here.  Blocks until the last launch's stream is idle.  *stalled_out = 1: render again with
 * TOR_PIXEL_KERNEL_LANE.  total_out (nullable): frames the blocking entry points re-rendered so far. */
TOR_API int tor_context_handoff_stalled(TorContext* ctx, int32_t* stalled_out, int64_t* total_out);

/* Scene-cache counters of a context: out[0] = tor_scene_upload calls, out[1] = calls that found the device
 * scene up to date (nothing rebuilt, nothing copied), out[2] = device layouts built so far. */
TOR_API int tor_context_scene_counters(TorContext* ctx, int64_t out[3]);

/* Device-side output stage (io/ppm.nim:15-16 quantiser int(256*clamp(c,0,0.999))):
 * d_pixels (n_rows*ncols*3 float64) -> d_rgb8 (n_rows*ncols*3 bytes), same row order.  A NaN channel gives byte 0 (black):
 * the reference's int(256 * clamp(NaN)) is undefined, and here no NaN reaches the conversion. */
TOR_API int tor_quantize_rgb8_device(TorContext* ctx, const double* d_pixels, int64_t n_values,
                                     uint8_t* d_rgb8, void* hip_stream);

/* Video output stage of the animation driver (trace_of_radiance_animation.nim:186-196), one fused
 * device kernel per frame: Canvas -> RGB8 (io/rgb.nim:17-31, top scanline first) -> BT.601 Y'CbCr
 * 4:2:0 (io/color_conversions.nim:180-252) -> one I_PCM slice (io/h264.nim:249-259).
 *   tor_h264_stream_header : SPS (h264.nim:90-142) + PPS (h264.nim:37), written once per stream
 *   tor_h264_frame_bytes   : size of one frame's slice NAL unit (width, height even; a size that is not a multiple of 16 --
 *                            1080 rows: BASELINE configs[4] -- is padded to whole macroblocks by edge replication and the SPS
 *                            crops the padding away (H.264 7.4.2.1.1).  The reference has a TODO there (h264.nim:178): its
 *                            SPS announces ceil(size/16) macroblocks, its flushFrame writes floor(size/16).)
 *   tor_encode_frame_device: d_pixels = finished canvas (nrows*ncols*3 float64, row 0 = bottom);
 *                            d_slice receives tor_h264_frame_bytes() bytes; d_y/d_cb/d_cr (nullable)
 *                            receive the planes (H264Encoder.getFrameBuffers, h264.nim:206-224).  A NaN
 *                            channel enters the colour conversion as byte 0, as in tor_quantize_rgb8_device.
 * Concatenating header + slices gives the Annex-B .264 file of main_animation_mp4;
 * tor_mp4_mux_file wraps it into the .mp4 (host side). */
TOR_API int tor_h264_stream_header(int32_t width, int32_t height, uint8_t* out, int32_t cap);
TOR_API int64_t tor_h264_frame_bytes(int32_t width, int32_t height);
/* MP4Muxer.initialize + writeMP4_from + close (io/mp4.nim:113-163, driver trace_of_radiance_animation.nim:
 * 203-210): reads the Annex-B stream src_annexb_path and writes an MP4 file with one avc1 video track --
 * one sample per slice NAL unit, 90 kHz time base, 90000/fps ticks per sample (the reference: fps = 30).
 * Host code, streams file to file.  Returns the number of samples written, or a negative status. */
TOR_API int tor_mp4_mux_file(const char* src_annexb_path, const char* dst_mp4_path, int32_t width,
                             int32_t height, int32_t fps);
TOR_API int tor_encode_frame_device(TorContext* ctx, const double* d_pixels, int32_t nrows, int32_t ncols,
                                    uint8_t* d_slice, uint8_t* d_y, uint8_t* d_cb, uint8_t* d_cr,
                                    void* hip_stream);

/* The animation driver's loop body in one blocking call (trace_of_radiance_animation.nim:181-196):
 * render the frame with the uploaded scene, convert + pack it on the device, copy only the slice NAL
 * unit (tor_h264_frame_bytes() bytes) to slice_out. */
TOR_API int tor_render_frame_h264(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols,
                                  int32_t samples_per_pixel, float gamma_correction, int64_t max_depth,
                                  const TorOptions* opt, uint8_t* slice_out, int64_t cap);

/* Timing of the last tor_render_device call on this context, measured with HIP events
 * recorded on the launch stream around the integrator kernel only (ms; the SEED_PIXEL cost probe and
 * the tile sort run before the start event); blocks until the kernel has finished.  samples_out
 * (nullable) = pixel-samples that launch traced.  All launches of one context that may be in flight
 * together must use ONE stream (per-launch state lives in a ring of 64 slots; with statistics enabled
 * launches must not overlap at all): tor_render_device returns TOR_ERR_INVALID_ARGUMENT for a launch on a different
 * stream while the context's previous launch is still running (use one context per stream for concurrency). */
TOR_API int tor_last_kernel_ms(TorContext* ctx, float* ms_out, int64_t* samples_out);
/* Mean duration (ms) of the integrator kernel over the last `last_n` tor_render_device calls
 * (at most 64 are remembered), from the same per-launch HIP events. */
TOR_API int tor_kernel_ms_mean(TorContext* ctx, int32_t last_n, float* mean_ms_out, int32_t* n_used_out);

/* Workload counters of the last tor_render_device call (only when the context was told to
 * collect them, see tor_context_set_stats): closest-hit queries, candidate resolves. */
typedef struct TorStats {
  uint64_t hit_queries;       /* world.hit() calls (hittables_lists.nim:48-55)          */
  uint64_t object_tests;      /* hit_queries * n_objects                                 */
  uint64_t candidates;        /* objects that went past the wave-uniform object loop: block_tests + exact_tests */
  uint64_t wave_iterations;   /* bounce-loop trips summed over waves                     */
  uint64_t lane_slots;        /* 64 * wave_iterations                                    */
  uint64_t samples;           /* pixel-samples traced                                    */
  uint64_t block_tests;       /* TOR_ACCEL_BLOCKS | TOR_ACCEL_F32: objects the float32 filter looked at in the blocks a ray entered (8 per block) */
  uint64_t exact_tests;       /* candidates - block_tests: objects that reached the reference's own test (spheres.nim:28-49) */
} TorStats;
TOR_API int tor_context_set_stats(TorContext* ctx, int32_t enable);
TOR_API int tor_last_stats(TorContext* ctx, TorStats* out);
/* Debug: 8 x u64 per wave of the last launch (stats enabled): {start, end (100 MHz wall clock), bounce
 * iterations (low 40 bits) | stage two of the plane-screened segments << 43 (a 21-bit field like the six below, part of
 * the object loop's), closest-hit queries | HW_ID << 44, time when the work counter ran dry, iteration count at that
 * time | trips of the resolve loop << 32, and two words of six 21-bit fields in units of 4096 shader cycles:
 * refill + camera ray, object loop, exact resolve | shade, deposit, total}.
 * Returns the number of waves copied (<= cap_waves) or < 0. */
TOR_API int tor_last_wave_log(TorContext* ctx, uint64_t* out, int64_t cap_waves);
/* Debug: chain hand-off of the last TOR_SEED_PIXEL launch on this context (all 0 when the launch ran without it):
 * out[0] tickets taken by server waves, out[1] chains pushed by lanes, out[2] waves still in the lane loop (0 after the
 * launch), out[3] workgroups that were servers from the start, out[4] push threshold (bounce iterations), out[5] chains
 * served, out[6] pushes of hot chains, out[7] pushes in the tail of the frame; out[8..11] microseconds after the
 * kernel's start at which the work counter ran dry, the last wave left the lane loop, the last hot chain and the last
 * tail chain were finished by a server; out[12], out[13] bounce iterations served for hot / tail chains; out[14] dedicated
 * server waves that found nothing to do and turned into lane waves; out[15] the adaptive push threshold at the end. */
TOR_API int tor_last_handoff_counters(TorContext* ctx, uint64_t out[16]);
/* Debug: the cost probe of the last TOR_SEED_PIXEL launch (it runs from 32 spp on): closest-hit queries per pixel over the
 * probe's samples (2 per pixel; per-sample streams, so only statistically what the frame's samples do), in the shard's
 * local pixel order.  Returns the number of pixels copied (<= cap_pixels) or < 0 (no probe ran). */
TOR_API int64_t tor_last_pixel_cost(TorContext* ctx, uint32_t* out, int64_t cap_pixels);

/* ------------------------------------------------------------------------------------ */
/* Host-side mirrors of the reference constructors on either side of the path            */
/* ------------------------------------------------------------------------------------ */

/* camera(...) -- physics/cameras.nim:24-45 */
TOR_API int tor_camera_init(TorCamera* out, const TorVec3* look_from, const TorVec3* look_at,
                            const TorVec3* view_up, double vertical_fov_degrees,
                            double aspect_ratio, double aperture, double focus_distance,
                            double shutter_open, double shutter_close);

/* random_scene(rng) with rng.seed(seed) -- scenes.nim:13-50, trace_of_radiance.nim:34-36.
 * Returns the number of objects written, or a negative status if cap is too small. */
TOR_API int64_t tor_random_scene(uint64_t seed, TorHittableVariant* out, int64_t cap);

/* Animated scene (BASELINE config 5) -- trace_of_radiance/scenes_animated.nim.
 * tor_animation_create = random_moving_spheres (:90-154) with rng.seed(seed);
 * tor_animation_next   = one turn of `iterator scenes(anim, skip)` (:176-225): returns 1 and fills
 *                        (cam, objects[0 .. *n_out)) when a frame is due, 0 once anim.t >= t_max.
 * Frames are independent given (cam, objects): a frame-parallel host gives frame f to GPU f mod N. */
typedef struct TorAnimation TorAnimation;
TOR_API int tor_animation_create(uint64_t seed, int32_t height, int32_t width, float dt, float t_min,
                                 float t_max, TorAnimation** out);
TOR_API void tor_animation_destroy(TorAnimation* anim);
TOR_API int64_t tor_animation_object_count(const TorAnimation* anim);
TOR_API int tor_animation_next(TorAnimation* anim, int32_t skip, TorCamera* cam, TorHittableVariant* objects,
                               int64_t cap, int64_t* n_out, float* t_out);

/* exportToPPM's quantiser on a host canvas -- io/ppm.nim:14-27.  out: nrows*ncols*3 bytes,
 * first row = top scanline. */
TOR_API int tor_canvas_to_rgb8(const TorCanvas* canvas, uint8_t* out);

/* ------------------------------------------------------------------------------------ */
/* Self-test probes (used by the parity tests; no effect on rendering)                   */
/* ------------------------------------------------------------------------------------ */

/* Host-only debug view of the TOR_ACCEL_BLOCKS layout for a ray-time range: slot_object[k] = original index
 * of the object in spatial slot k (block k/8) or -1; block_boxes / super_boxes = 6 float64 {lo xyz, hi xyz}
 * per (padded) block / per group of 8 blocks.  Returns the number of blocks (0 when no culling layout is
 * built for this scene) or a negative status. */
TOR_API int tor_debug_accel_layout(TorHittableList world, double t_lo, double t_hi, int64_t* slot_object,
                                   int64_t slot_cap, double* block_boxes, double* super_boxes, int64_t box_cap,
                                   int32_t* two_level_out);

/* The integrate_kernel variant that the context's last render launch chose (tor_render_device, tor_render_accumulate_device,
 * tor_render_accumulate_list_device, tor_render_resume_device, tor_render_resume_list_device, ...): out = {seeding, arith, w, f32, blocks} -- seeding 0 | 1 | 3
 * (sample streams + second moments) | 4 (... over a pixel list) | 5 (resumable pixel streams) | 6 (... + second moments) | 7 (... over a pixel list); arith 0, or 2 behind the FMA screen; w = 2 (256 VGPRs) or 3 (168 VGPRs); f32 0 | 1; blocks
 * 0 | 1 | 2 (two-level layout).  All -1 until the context has launched one; a launch that traces nothing (an empty list) or runs
 * the wave-per-pixel kernel leaves it as it was.  Host only, no synchronisation. */
TOR_API int tor_debug_last_variant(TorContext* ctx, int32_t out[5]);
/* Split mode of the context's last render launch (TOR_SEED_PIXEL, TOR_PIXEL_KERNEL_AUTO: the frame shared between the lane kernel and
 * the wave-per-pixel kernel on a second stream): *tiles_out = the number of 64-pixel tiles, most expensive first by the probe's
 * count, that the wave-per-pixel kernel rendered; 0 when the launch ran one kernel for the whole frame.  Blocks until that launch
 * has finished. */
TOR_API int tor_debug_last_split_tiles(TorContext* ctx, int64_t* tiles_out);

/* TOR_ACCEL_F32 over a whole scene on the HOST: builds the layout tor_scene_upload builds and walks its float32
 * segments for each ray (origin o, direction d, time) exactly as the kernel does.
 * keep[ray * world.len + object] = 1 kept, 0 dropped, 2 object stays on the float64 loop. */
TOR_API int tor_debug_filter32_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d,
                                     const double* time, int8_t* keep);

/* The strict brute-force layout's screened segments over a whole scene on the HOST (csrc/tor_screen.hpp; the layout
 * tor_scene_upload builds, walked as the ARITH 2 object loop walks it when stage one runs: plane screen, then the segment's own
 * test per object -- second form for xkind 10 / 11 / 12, first form for 13 / 14).
 * keep[ray * world.len + object] = 0 dropped by the plane screen, 1 dropped by stage two, 2 candidate of the exact test,
 * 3 the object sits on a segment without a plane table; kind_out[object] (nullable) = 0 | 10..14, its segment's xkind;
 * pays_out[ray * n_segs_out + segment] (nullable) = 1 when that ray votes for stage one on that segment (plane_pays). */
TOR_API int tor_debug_screen2_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d,
                                    const double* time, int8_t* keep, int32_t* kind_out, int8_t* pays_out, int64_t n_segs_out);

/* Stage one of the strict layout's plane-screened segments in FLOAT32 against the float64 plane screen it stands for, on the
 * HOST (csrc/tor_screen.hpp plane_seg32 / plane_word32; the layout and segment headers tor_scene_upload builds).  For every ray
 * and every object on a segment of xkind 10 / 11 / 12 / 14: keep[ray * world.len + object] = bit 0: the float64 plane screen
 * keeps it, bit 1: the float32 one does; -1 for the other objects.  pad_kept[ray] = the padding slots of those segments the
 * float32 screen keeps for that ray, *n_pad_out = the number of such padding slots. */
TOR_API int tor_debug_plane32_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d, const double* time,
                                    int8_t* keep, int32_t* pad_kept, int64_t* n_pad_out);

/* The float64 layout's segments in the order the kernel walks them (tor_scene.cpp: largest first; a plane-screened segment's long
 * tail padded to a whole word of 32 slots): out[4 * s + {0, 1, 2, 3}] = {xkind, objects, slots, first slot} for the first
 * `max_segs` segments; *n_segs_out = the number of segments.  Host only. */
TOR_API int tor_debug_layout_segments(TorHittableList world, int32_t* out, int64_t max_segs, int64_t* n_segs_out);

/* Float32 slab test of the culling boxes on the HOST (same source as the kernel): ray i against the box [lo_i, hi_i].
 * keep[i] = the float32 test keeps the box, need[i] = the float64 slab test of the float64 path passes.
 * Correct iff need[i] != 0 implies keep[i] != 0. */
TOR_API int tor_selftest_slab32_host(int64_t n, const double* o, const double* d, const double* lo, const double* hi,
                                     const double* origin, int32_t* keep, int32_t* need);

/* TOR_ACCEL_F32 self test on the HOST (same source as the kernel's pre-filter): ray i against sphere i with
 * centre c0 + dc * f (moving != 0) or c0.  keep[i] = pre-filter keeps the object; need[i] bit 0 = the
 * float64 test D > 0 and (half_b < 0 or c < 0) holds, bit 1 = the reference's hit() accepts a root.
 * The filter is correct iff need[i] != 0 implies keep[i] != 0. */
TOR_API int tor_selftest_filter32_host(int64_t n, const double* o, const double* d, const double* c0,
                                       const double* dc, const int32_t* moving, const double* f, const double* r2,
                                       const double* origin, int32_t* keep, int32_t* need);

/* The conservative FMA screen of the strict float64 object loop on the HOST (same source as the kernel, csrc/tor_screen.hpp):
 * ray i against sphere i, margins as for a segment that holds only this object.  keep / need as above; correct iff
 * need[i] != 0 implies keep[i] != 0.  (The screen only selects candidates for the exact test of spheres.nim:29-48.) */
TOR_API int tor_selftest_screen_host(int64_t n, const double* o, const double* d, const double* c0,
                                     const double* dc, const int32_t* moving, const double* f, const double* r2,
                                     int32_t* keep, int32_t* need);
/* The screen's SECOND form (expanded quadratic, direction normalised per ray: csrc/tor_screen.hpp).  variant 0: static
 * spheres through the general record, movers along y through the common-height record, other movers through the first form
 * (as the kernel routes them); variant 1: static spheres through the common-height record; variant 2: static spheres and
 * movers along y through the plane screen alone (stage one of the common-height segments). */
TOR_API int tor_selftest_screen2_host(int64_t n, const double* o, const double* d, const double* c0,
                                      const double* dc, const int32_t* moving, const double* f, const double* r2,
                                      int32_t variant, int32_t* keep, int32_t* need);

/* Runs the kernel's own math on the DEVICE: op 0: sin,cos(a)  1: x^5  2: pow(x,y)
 * 3: sqrt(x)  4: x/y  5: uniform01 of seed(row=x,col=y) first n draws... see tests. */
TOR_API int tor_selftest_math_device(int32_t op, const double* x, const double* y, double* out0,
                                     double* out1, int64_t n, int32_t device);
/* Same routines compiled for the HOST from the same source (no GPU needed). */
TOR_API int tor_selftest_math_host(int32_t op, const double* x, const double* y, double* out0,
                                   double* out1, int64_t n);
/* RNG probes (host build of the kernel's RNG): state after seed, then n draws. */
TOR_API int tor_selftest_rng_host(int32_t mode, uint64_t a, uint64_t b, uint64_t c,
                                  uint64_t state_out[4], uint64_t* draws_out, int64_t n);

TOR_API const char* tor_version(void);

#ifdef __cplusplus
}
#endif

/* ---- direct-light sampling queries: the shadow rays of next-event estimation --------------------------------------------------------
 * tor_scene_lights, tor_light_sample_device / _host, tor_light_pdf_device / _host: per shading point one light of the context's
 * light table, a direction inside the cone its sphere subtends, the shadow segment for tor_occluded_device and the solid-angle
 * density -- defined operation by operation, in the query family's style, in tor_lights.h. */
#include "tor_lights.h"

/* ---- environment-light queries: the sky as an emitter ---------------------------------------------------------------------------------
 * tor_scene_environment, tor_env_sample_device / _host, tor_env_eval_device / _host: a context-owned octahedral environment map,
 * evaluated per ray direction, importance-sampled per shading point, with the solid-angle density of any direction -- defined
 * operation by operation in tor_env.h. */
#include "tor_env.h"

/* ---- light-tracing queries: emit from the lights, connect to the camera ---------------------------------------------------------------
 * tor_light_emit_device / _host, tor_camera_connect_device / _host: a path started ON a lamp of the light table, and for a world
 * point the pixel it lands in, the lens point and the measurement weight -- the splats of a light tracer, defined operation by
 * operation in tor_camera.h. */
#include "tor_camera.h"

/* ---- BSDF queries: value and density of the reference's scatter ----------------------------------------------------------------------
 * tor_bsdf_eval_device / _host: for an incoming direction, a hit record and an outgoing direction the solid-angle density
 * Material.scatter gives that direction and the value albedo * density -- what next-event estimation and multiple importance
 * sampling need at a Lambertian or a fuzzy Metal vertex -- defined operation by operation in tor_bsdf.h. */
#include "tor_bsdf.h"

/* ---- photon-map queries: build a hashed grid, gather by radius, exactly --------------------------------------------------------------
 * tor_photons_build_device / _host, tor_photons_gather_device / _host, tor_photons_info: light-path vertices stored as photons in a
 * context-owned map, and per query point the exact sum of the powers of the photons within a radius -- density estimation for
 * caustics seen through specular vertices -- defined by brute force, operation by operation, in tor_photons.h. */
#include "tor_photons.h"

/* ---- participating-media queries: optical-depth march, isotropic scatter -------------------------------------------------------------
 * tor_scene_media, tor_media_march_device / _host, tor_media_scatter_device / _host, tor_rng_uniform_device / _host: where along a
 * ray the optical depth through a table of homogeneous spherical media reaches a budget, the isotropic scatter at that collision,
 * and plain uniforms from a path's stream -- fog, smoke and haze for host-written integrators, defined operation by operation in
 * tor_media.h. */
#include "tor_media.h"

/* ---- phase-function queries: Henyey-Greenstein sample, value, density ------------------------------------------------------------------
 * tor_scene_media_phase, tor_phase_sample_device / _host, tor_phase_eval_device / _host: an asymmetry per medium of the media table, a
 * direction drawn from the Henyey-Greenstein mixture of the media active at a collision, and value and density of a direction that
 * was not drawn -- what lets a lamp of the light table light the fog --, defined operation by operation in tor_phase.h. */
#include "tor_phase.h"

/* ---- heterogeneous media: density grids marched cell by cell, exactly -------------------------------------------------------------------
 * tor_scene_media_grid, tor_media_grid_info, tor_media_grid_march_device / _host, tor_media_grid_density_device / _host: a voxel grid
 * of densities attached to one medium of the media table, the optical-depth march through it by regular tracking (a 3-D DDA, no
 * log, no exp, no draws) and the density lookup at a point, defined operation by operation in tor_grid.h. */
#include "tor_grid.h"

/* ---- surface-texture queries: checker and octahedral image albedos --------------------------------------------------------------------
 * tor_scene_textures, tor_texture_info, tor_texture_eval_device / _host: a table of textures bound to the objects of the uploaded
 * list, and per hit record the colour of the surface there -- a constant, a 3-D checker, or an octahedral image looked up by the
 * record's outward normal (nearest or bilinear, no atan2 and no acos) -- defined operation by operation in tor_texture.h. */
#include "tor_texture.h"

/* ---- planar patch queries: quads and triangles for host integrators -------------------------------------------------------------------
 * tor_scene_patches, tor_patch_info, tor_patch_hit_device / _host, tor_patch_occluded_device / _host: a context-owned table of
 * static parallelograms and triangles, the closest patch per ray (alone, or merged into the records tor_hit_device wrote) and the
 * any-hit bit (alone, or OR-ed into tor_occluded_device's) -- Moeller-Trumbore in float64, defined operation by operation in
 * tor_patches.h. */
#include "tor_patches.h"

/* ---- debug entries of the reach pass in front of the plane screen's whole words -------------------------------------------------
 * tor_debug_reach_scene, tor_debug_last_reach: which words of the sorted list a ray can be near (host mirror), and how many whole
 * words the last launch walked; described in tor_reach.h. */
#include "tor_reach.h"

#endif /* TOR_RENDER_H */
