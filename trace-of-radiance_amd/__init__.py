"""trace-of-radiance on MI355X: host-side mirror of the reference's render() interface.

The product is ``lib/libtor_mi355x.so`` (hand-written HIP kernels for gfx950 behind the C ABI
declared in ``include/tor_render.h``).  This module is the thin host layer above that ABI; it
mirrors the names of the reference's own interface for the path

    camera(...)                     physics/cameras.nim:24-45
    random_scene(seed)              scenes.nim:13-50 (+ trace_of_radiance.nim:34-36)
    new_canvas / Canvas             primitives/canvas.nim:20-41
    render(canvas, cam, world, max_depth)   render.nim:49
    export_rgb8 (exportToPPM's quantiser)   io/ppm.nim:14-27

so the parity tests read like the reference's ``main()`` (trace_of_radiance.nim:26-71).
There is NO CPU fallback: every rendering call raises ``TorError`` when the HIP extension or a
GPU is missing.  (The package directory name contains a hyphen; import it with
``importlib.import_module("trace-of-radiance_amd")``.)
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtor_mi355x.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

SEED_PIXEL, SEED_SAMPLE = 0, 1
ARITH_STRICT, ARITH_FUSED = 0, 1   # (ARITH_FUSED: removed in round 5; the library rejects it and says why)
ACCEL_NONE, ACCEL_BLOCKS, ACCEL_F32 = 0, 1, 2
GATHER_AUTO, GATHER_RCCL, GATHER_PEER, GATHER_HOST = 0, 1, 2, 3
PIXEL_KERNEL_AUTO, PIXEL_KERNEL_LANE, PIXEL_KERNEL_WAVE = 0, 1, 2
# return codes (include/tor_render.h)
OK, ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_OUT_OF_MEMORY, ERR_INCOMPLETE = 0, -1, -2, -3, -4, -5
MAX_DEVICES = 16
LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2
SPHERE, MOVING_SPHERE = 0, 1


class TorError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"tor_mi355x error {code}: {msg}")
        self.code = code


# --------------------------------------------------------------------------------------
# ABI structs (include/tor_render.h)
# --------------------------------------------------------------------------------------
class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class _Lambertian(C.Structure):
    _fields_ = [("albedo", Vec3)]


class _Metal(C.Structure):
    _fields_ = [("albedo", Vec3), ("fuzz", C.c_double)]


class _Dielectric(C.Structure):
    _fields_ = [("refraction_index", C.c_double)]


class _MaterialU(C.Union):
    _fields_ = [("lambertian", _Lambertian), ("metal", _Metal), ("dielectric", _Dielectric)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("_pad", C.c_uint8 * 7), ("u", _MaterialU)]


class Sphere(C.Structure):
    _fields_ = [("center", Vec3), ("radius", C.c_double), ("material", Material)]


class MovingSphere(C.Structure):
    _fields_ = [("center0", Vec3), ("center1", Vec3), ("time0", C.c_double), ("time1", C.c_double),
                ("radius", C.c_double), ("material", Material)]


class _HittableU(C.Union):
    _fields_ = [("sphere", Sphere), ("moving_sphere", MovingSphere)]


class HittableVariant(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("_pad", C.c_uint8 * 7), ("u", _HittableU)]


class HittableList(C.Structure):
    _fields_ = [("len", C.c_int64), ("objects", C.POINTER(HittableVariant))]


class Camera(C.Structure):
    _fields_ = [("origin", Vec3), ("lower_left_corner", Vec3), ("horizontal", Vec3), ("vertical", Vec3),
                ("u", Vec3), ("v", Vec3), ("w", Vec3), ("lens_radius", C.c_double),
                ("shutter_open", C.c_double), ("shutter_close", C.c_double)]

    def as_array(self) -> np.ndarray:
        return np.frombuffer(bytes(self), dtype=np.float64).copy()


class CanvasStruct(C.Structure):
    _fields_ = [("pixels", C.POINTER(Vec3)), ("nrows", C.c_int32), ("ncols", C.c_int32),
                ("samples_per_pixel", C.c_int32), ("gamma_correction", C.c_float)]


class Options(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("seeding", C.c_int32), ("arith", C.c_int32),
                ("device", C.c_int32), ("shard_index", C.c_int32), ("shard_count", C.c_int32),
                ("row_tile", C.c_int32), ("accel", C.c_int32),
                ("device_count", C.c_int32), ("gather", C.c_int32), ("devices", C.c_int32 * MAX_DEVICES),
                ("pixel_kernel", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("hit_queries", C.c_uint64), ("object_tests", C.c_uint64), ("candidates", C.c_uint64),
                ("wave_iterations", C.c_uint64), ("lane_slots", C.c_uint64), ("samples", C.c_uint64),
                ("block_tests", C.c_uint64), ("exact_tests", C.c_uint64)]


class Ray(C.Structure):
    """TorRay -- primitives/rays.nim (origin, direction, time; 56 B)."""
    _fields_ = [("origin", Vec3), ("direction", Vec3), ("time", C.c_double)]


class Hit(C.Structure):
    """TorHit -- HitRecord, physics/core.nim:30-36, with the object's index in the uploaded list in place of the material (64 B)."""
    _fields_ = [("p", Vec3), ("normal", Vec3), ("t", C.c_double), ("object", C.c_int32), ("front_face", C.c_int32)]


class Rng(C.Structure):
    """TorRng -- Rng, support/rng.nim:18-19: the four xoshiro256+ words (32 B)."""
    _fields_ = [("s0", C.c_uint64), ("s1", C.c_uint64), ("s2", C.c_uint64), ("s3", C.c_uint64)]


assert C.sizeof(Rng) == 32
assert C.sizeof(Ray) == 56 and C.sizeof(Hit) == 64 and Hit.object.offset == 56 and Hit.front_face.offset == 60
assert C.sizeof(Vec3) == 24 and C.sizeof(Material) == 40 and C.sizeof(Sphere) == 72
assert C.sizeof(MovingSphere) == 112 and C.sizeof(HittableVariant) == 120
assert C.sizeof(HittableList) == 16 and C.sizeof(Camera) == 192 and C.sizeof(CanvasStruct) == 24

EXPORTED_SYMBOLS = [
    "tor_render", "tor_render_opt", "tor_last_error", "tor_context_create", "tor_context_destroy",
    "tor_scene_upload", "tor_shard_rows", "tor_render_device", "tor_quantize_rgb8_device",
    "tor_last_kernel_ms", "tor_kernel_ms_mean", "tor_context_set_stats", "tor_last_stats", "tor_last_wave_log", "tor_camera_init",
    "tor_random_scene", "tor_canvas_to_rgb8", "tor_animation_create", "tor_animation_destroy",
    "tor_animation_object_count", "tor_animation_next", "tor_h264_stream_header", "tor_h264_frame_bytes",
    "tor_encode_frame_device", "tor_render_frame_h264", "tor_mp4_mux_file", "tor_debug_accel_layout", "tor_selftest_filter32_host", "tor_selftest_screen_host", "tor_selftest_slab32_host", "tor_debug_filter32_scene", "tor_selftest_math_device", "tor_selftest_math_host",
    "tor_selftest_rng_host", "tor_version",
    "tor_last_render_timing", "tor_comm_unique_id", "tor_comm_init_rank", "tor_comm_destroy", "tor_render_gather_device",
    "tor_context_scene_counters", "tor_render_ptr", "tor_last_pixel_cost", "tor_last_note", "tor_last_handoff_counters",
    "tor_selftest_screen2_host", "tor_debug_screen2_scene", "tor_debug_layout_segments", "tor_debug_plane32_scene", "tor_knob_count", "tor_knob_info", "tor_last_gather_info", "tor_last_device_kernel_ms", "tor_comm_abort", "tor_comm_count", "tor_context_handoff_stalled",
    "tor_render_accumulate_device", "tor_resolve_device", "tor_accum_noise_device",
    "tor_render_accumulate_list_device", "tor_adaptive_select_device", "tor_resolve_counts_device", "tor_debug_last_variant",
    "tor_hit_device", "tor_hit_host", "tor_radiance_device", "tor_radiance_host", "tor_camera_rays_device",
    "tor_bounce_device", "tor_bounce_host", "tor_scatter_device", "tor_scatter_host", "tor_sky_device", "tor_bounce_select_device",
    "tor_render_resume_device", "tor_debug_last_split_tiles", "tor_render_resume_list_device",
    "tor_occluded_device", "tor_occluded_host",
    "tor_scene_groups", "tor_hit_masked_device", "tor_hit_masked_host", "tor_occluded_masked_device", "tor_occluded_masked_host",
    "tor_bounce_masked_device",
    "tor_crossings_device", "tor_crossings_host",
    "tor_nearest_device", "tor_nearest_host",
    "tor_deposit_device",
]
# the direct-light sampling queries (include/tor_lights.h), bound next to the entries of tor_render.h
LIGHT_SYMBOLS = ["tor_scene_lights", "tor_light_sample_device", "tor_light_sample_host", "tor_light_pdf_device", "tor_light_pdf_host"]
LIGHT_BY_WEIGHT, LIGHT_BY_SOLID_ANGLE = 0, 1   # TOR_LIGHT_BY_*: what Context.sample_lights picks a light by
LIGHT_STRATEGIES = {"weight": LIGHT_BY_WEIGHT, "solid_angle": LIGHT_BY_SOLID_ANGLE}
# the environment-light queries (include/tor_env.h), bound as the light entries are
ENV_SYMBOLS = ["tor_scene_environment", "tor_env_sample_device", "tor_env_sample_host", "tor_env_eval_device", "tor_env_eval_host"]
ENV_MAX_SIDE = 2048   # TOR_ENV_MAX_SIDE: the most texels per side of an environment map
# the light-tracing queries (include/tor_camera.h), bound as the light entries are
CAMERA_SYMBOLS = ["tor_camera_connect_device", "tor_camera_connect_host", "tor_light_emit_device", "tor_light_emit_host"]
# the BSDF queries (include/tor_bsdf.h), bound as the light entries are
BSDF_SYMBOLS = ["tor_bsdf_eval_device", "tor_bsdf_eval_host"]
BSDF_NONE, BSDF_DENSITY, BSDF_DELTA = 0, 1, 2   # TOR_BSDF_*: the kind of a Context.bsdf answer
# the photon-map queries (include/tor_photons.h), bound as the light entries are
PHOTON_SYMBOLS = ["tor_photons_build_device", "tor_photons_build_host", "tor_photons_gather_device", "tor_photons_gather_host",
                  "tor_photons_info"]
PHOTON_KERNELS = {"constant": 0, "epanechnikov": 1}   # TOR_PHOTON_KERNEL_*: the weight of a photon inside the gather radius
# the participating-media queries (include/tor_media.h), bound as the light entries are
MEDIA_SYMBOLS = ["tor_scene_media", "tor_media_march_device", "tor_media_march_host", "tor_media_scatter_device",
                 "tor_media_scatter_host", "tor_rng_uniform_device", "tor_rng_uniform_host"]
MEDIA_MAX = 64            # TOR_MEDIA_MAX: the most media of a table (the active set of a march is one 64-bit word)
UNIFORM_MAX_DRAWS = 16    # TOR_UNIFORM_MAX_DRAWS: the most uniforms per state of one Context.uniform call
MEDIA_REFUSED, MEDIA_ESCAPED, MEDIA_COLLIDED = -1, 0, 1   # the status of a Context.march_media answer
# the phase-function queries (include/tor_phase.h): bound in a second step of lib(), after the table _bind gives every library
PHASE_SYMBOLS = ["tor_scene_media_phase", "tor_phase_eval_device", "tor_phase_eval_host", "tor_phase_sample_device",
                 "tor_phase_sample_host"]
# the debug entries of the reach pass (include/tor_reach.h), bound as the phase entries are
REACH_SYMBOLS = ["tor_debug_reach_scene", "tor_debug_last_reach"]
# the density grids of heterogeneous media (include/tor_grid.h), bound as the phase entries are
GRID_SYMBOLS = ["tor_scene_media_grid", "tor_media_grid_info", "tor_media_grid_march_device", "tor_media_grid_march_host",
                "tor_media_grid_density_device", "tor_media_grid_density_host"]
GRID_MAX_DIM = 1024         # TOR_GRID_MAX_DIM: the most cells of a density grid along one axis
GRID_MAX_CELLS = 1 << 24    # TOR_GRID_MAX_CELLS: the most cells of a density grid
# the surface-texture queries (include/tor_texture.h), bound as the phase entries are
TEXTURE_SYMBOLS = ["tor_scene_textures", "tor_texture_info", "tor_texture_eval_device", "tor_texture_eval_host"]
TEXTURE_CONSTANT, TEXTURE_CHECKER, TEXTURE_IMAGE = 0, 1, 2   # TOR_TEXTURE_*: the kind of a Texture
TEXTURE_SPACES = {"world": 0, "normal": 1}                   # TOR_TEXTURE_WORLD / _NORMAL: what a checker reads
TEXTURE_FILTERS = {"nearest": 0, "bilinear": 1}              # TOR_TEXTURE_NEAREST / _BILINEAR: how an image is looked up
TEXTURE_MAX, TEXTURE_MAX_SIDE, TEXTURE_MAX_TEXELS = 4096, 2048, 1 << 22   # TOR_TEXTURE_MAX*
# the planar patch queries (include/tor_patches.h), bound as the texture entries are
PATCH_SYMBOLS = ["tor_scene_patches", "tor_patch_info", "tor_patch_hit_device", "tor_patch_hit_host", "tor_patch_occluded_device",
                 "tor_patch_occluded_host"]
PATCH_QUAD, PATCH_TRIANGLE = 0, 1   # TOR_PATCH_*: the kind of a Patch
PATCH_MAX = 16384                   # TOR_PATCH_MAX: the most patches of a table
PHASE_G_MAX = 0.99          # TOR_PHASE_G_MAX: the largest |g| of Context.set_media_phase
PHASE_G_MIN = 2.0 ** -20    # TOR_PHASE_G_MIN: the smallest |g| that is not 0
HIT_AUTO, HIT_BRUTE, HIT_BLOCKS = 0, 1, 2
HIT_MODES = {"auto": HIT_AUTO, "brute": HIT_BRUTE, "blocks": HIT_BLOCKS}
BOUNCE_MISS, BOUNCE_SCATTERED, BOUNCE_ABSORBED = 0, 1, 2
CROSSINGS_MAX = 16   # TOR_CROSSINGS_MAX: the most crossings per ray Context.crossings keeps
NEAREST_MAX = 16     # TOR_NEAREST_MAX: the most neighbours per point Context.nearest keeps
DEPOSIT_MAX_VALUE = 128.0   # tor_deposit_device: the largest clamp (q * q must stay within quantize36's exact range)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2   # Material kinds (TOR_LAMBERTIAN ..): groups_by_material gives 1 << kind

_lib = None


def build(force: bool = False) -> str:
    """Compile libtor_mi355x.so for gfx950 in-tree (hipcc cross-compiles without a GPU).  Serialised by a
    file lock: the ranks of a multi-GPU launch may all find the library missing at the same time."""
    import fcntl
    src_dir = os.path.join(_HERE, "csrc")
    lock_path = os.path.join(src_dir, ".build.lock")
    if not os.access(src_dir, os.W_OK):  # read-only install: serialise through the temp dir instead
        import hashlib
        import tempfile
        lock_path = os.path.join(tempfile.gettempdir(), "tor_mi355x_" + hashlib.sha1(src_dir.encode()).hexdigest()[:12] + ".lock")
    with open(lock_path, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            cmd = ["make", "-C", src_dir] + (["-B"] if force or not os.path.exists(LIB_PATH) else []) + ["all"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:  # show the compiler's own words
                raise TorError(-3, f"building libtor_mi355x.so failed ({' '.join(cmd)}):\n{r.stdout[-4000:]}\n{r.stderr[-8000:]}")
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


def ensure_built() -> str:
    """Build the HIP extension if the in-tree library is missing (a fresh checkout); never a fallback --
    without hipcc this raises."""
    if not os.path.exists(LIB_PATH):
        build()
    return LIB_PATH


def lib():
    """Load the HIP extension; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TorError(-2, f"HIP extension missing: {LIB_PATH} (run __graft_entry__.build()); "
                           "there is no CPU fallback")
    # PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  Two HIP/HSA
    # runtimes in one process cannot both open the GPU, so when torch is installed it must be
    # loaded FIRST: the dynamic loader then binds this library's NEEDED libamdhip64.so.7 to the
    # already-loaded copy and device pointers / streams are shared with torch.
    if os.environ.get("TOR_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    # (harness-side A/B switch of the tools: TOR_AB_LIB = another build of THIS library -- e.g. last round's kernels -- to measure
    # against in the same gpurun call; never a fallback: unset, the in-tree library above is the only one there is)
    ab = os.environ.get("TOR_AB_LIB")
    if ab:  # never silent: every consumer of this process measures / validates ANOTHER binary
        print(f"trace-of-radiance_amd: TOR_AB_LIB set -- loading {ab} instead of the in-tree library", file=sys.stderr, flush=True)
    L = C.CDLL(ab or LIB_PATH)
    _bind(L, skip_missing=bool(ab))   # (an A/B build may be older than an entry; the in-tree library has them all, or this raises)
    _bind(L, PHASE_SYMBOLS, skip_missing=bool(ab), table=_PHASE_SIGNATURES)
    _bind(L, REACH_SYMBOLS, skip_missing=bool(ab), table=_REACH_SIGNATURES)
    _bind(L, GRID_SYMBOLS, skip_missing=bool(ab), table=_GRID_SIGNATURES)
    _bind(L, TEXTURE_SYMBOLS, skip_missing=bool(ab), table=_TEXTURE_SIGNATURES)
    _bind(L, PATCH_SYMBOLS, skip_missing=bool(ab), table=_PATCH_SIGNATURES)
    _lib = L
    return L


def _signatures() -> dict:
    """The ctypes signature of every entry this module calls: symbol -> argtypes, or (argtypes, restype) where the restype is not
    int; argtypes None: none are set."""
    v, i32, i64, u32, u64, d, f, P = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double, C.c_float, C.POINTER
    dp, cam, opt, obj = P(d), P(Camera), P(Options), P(HittableVariant)
    frame = [v, cam, i32, i32, i32, f, i64, opt]              # ctx, camera, rows, cols, spp, gamma, depth, options
    passes = [v, cam, i32, i32, i32, i32, i64, opt]           # ... first sample and samples where spp and gamma are
    listed = [v, cam, i32, i32, v, i32, i32, i32, i64, opt]   # ... and the pixel list and its length before them
    return {
        "tor_last_error": (None, C.c_char_p),
        "tor_version": (None, C.c_char_p),
        "tor_last_note": (None, C.c_char_p),
        "tor_render": [P(CanvasStruct), cam, HittableList, i64],
        "tor_render_ptr": [P(CanvasStruct), cam, P(HittableList), i64],
        "tor_render_opt": [P(CanvasStruct), cam, HittableList, i64, opt],
        "tor_context_create": [i32, P(v)],
        "tor_context_destroy": [v],
        "tor_scene_upload": [v, HittableList],
        "tor_shard_rows": [i32, i32, i32, i32, P(i32)],
        "tor_render_device": frame + [v, v],
        "tor_quantize_rgb8_device": [v, v, i64, v, v],
        "tor_last_kernel_ms": [v, P(f), P(i64)],
        "tor_kernel_ms_mean": [v, i32, P(f), P(i32)],
        "tor_context_set_stats": [v, i32],
        "tor_last_stats": [v, P(Stats)],
        "tor_last_wave_log": [v, P(u64), i64],
        "tor_last_pixel_cost": ([v, P(u32), i64], i64),
        "tor_last_handoff_counters": [v, P(u64)],
        "tor_camera_init": [cam, P(Vec3), P(Vec3), P(Vec3)] + [d] * 6,
        "tor_random_scene": ([u64, obj, i64], i64),
        "tor_canvas_to_rgb8": [P(CanvasStruct), P(C.c_uint8)],
        "tor_animation_create": [u64, i32, i32, f, f, f, P(v)],
        "tor_animation_destroy": ([v], None),
        "tor_animation_object_count": ([v], i64),
        "tor_animation_next": [v, i32, cam, obj, i64, P(i64), P(f)],
        "tor_h264_stream_header": [i32, i32, P(C.c_uint8), i32],
        "tor_h264_frame_bytes": ([i32, i32], i64),
        "tor_encode_frame_device": [v, v, i32, i32, v, v, v, v, v],
        "tor_render_frame_h264": frame + [P(C.c_uint8), i64],
        "tor_mp4_mux_file": [C.c_char_p, C.c_char_p, i32, i32, i32],
        "tor_debug_accel_layout": [HittableList, d, d, P(i64), i64, dp, dp, i64, P(i32)],
        "tor_selftest_filter32_host": [i64] + [dp] * 4 + [P(i32)] + [dp] * 3 + [P(i32)] * 2,
        "tor_selftest_screen_host": [i64] + [dp] * 4 + [P(i32)] + [dp] * 2 + [P(i32)] * 2,
        "tor_selftest_screen2_host": [i64] + [dp] * 4 + [P(i32)] + [dp] * 2 + [i32] + [P(i32)] * 2,
        "tor_selftest_slab32_host": [i64] + [dp] * 5 + [P(i32)] * 2,
        "tor_debug_filter32_scene": [HittableList, i64] + [dp] * 3 + [P(C.c_int8)],
        "tor_debug_screen2_scene": [HittableList, i64] + [dp] * 3 + [P(C.c_int8), P(i32), P(C.c_int8), i64],
        "tor_debug_plane32_scene": [HittableList, i64] + [dp] * 3 + [P(C.c_int8), P(i32), P(i64)],
        "tor_debug_layout_segments": [HittableList, P(i32), i64, P(i64)],
        "tor_selftest_math_device": [i32, dp, dp, dp, dp, i64, i32],
        "tor_selftest_math_host": [i32, dp, dp, dp, dp, i64],
        "tor_selftest_rng_host": [i32, u64, u64, u64, P(u64), P(u64), i64],
        "tor_last_render_timing": [dp],
        "tor_comm_unique_id": [P(C.c_uint8)],
        "tor_comm_init_rank": [v, P(C.c_uint8), i32, i32],
        "tor_comm_destroy": [v],
        "tor_render_gather_device": frame + [i32, v, v],
        "tor_context_scene_counters": [v, P(i64)],
        "tor_knob_count": (None, i32),
        "tor_knob_info": [i32] + [P(C.c_char_p)] * 5,
        "tor_last_gather_info": [P(i32)],
        "tor_last_device_kernel_ms": [P(f), i32],
        "tor_comm_abort": [v],
        "tor_comm_count": [v, P(i32)],
        "tor_context_handoff_stalled": [v, P(i32), P(i64)],
        # progressive and adaptive rendering, on the sample streams and on the reference's pixel streams
        "tor_render_accumulate_device": passes + [v, v, v],
        "tor_resolve_device": [v, v, i64, i64, f, v, v],
        "tor_accum_noise_device": [v, v, v, i64, i64, v, dp, v],
        "tor_render_accumulate_list_device": listed + [v, v, v],
        "tor_adaptive_select_device": [v, v, v, v, i32, i64, d, d, v, v, P(i32), v],
        "tor_resolve_counts_device": [v, v, v, i64, f, v, v],
        "tor_debug_last_variant": [v, P(i32)],
        "tor_render_resume_device": passes + [v, v, v, v],
        "tor_debug_last_split_tiles": [v, P(i64)],
        "tor_render_resume_list_device": listed + [v, v, v, v],
        # the queries: ctx, n, the arrays ...; a _device entry ends in the stream -- and a _masked_ one in the mask after it
        "tor_hit_device": [v, i64, v, v, d, d, i32, v, v],
        "tor_hit_host": [v, i64, v, v, d, d, i32, v],
        "tor_hit_masked_device": [v, i64, v, v, d, d, i32, v, v, v, u32],
        "tor_hit_masked_host": [v, i64, v, v, d, d, i32, v, v, u32],
        "tor_radiance_device": [v, i64, v, v, i32, d, d, i32, v, v],
        "tor_radiance_host": [v, i64, v, v, i32, d, d, i32, v],
        "tor_camera_rays_device": [v, cam, i32, i32, v, i64, i32, i32, i32, v, v, v],
        "tor_bounce_device": [v, i64, v, v, v, i64, d, d, i32, v, v, v, v],
        "tor_bounce_host": [v, i64, v, v, v, i64, d, d, i32, v, v, v],
        "tor_bounce_masked_device": [v, i64, v, v, v, i64, d, d, i32, v, v, v, v, v, u32],
        "tor_scatter_device": [v, i64, v, v, v, v, i64, v, v, v],
        "tor_scatter_host": [v, i64, v, v, v, v, i64, v, v],
        "tor_sky_device": [v, i64, v, v, i64, v, v],
        "tor_bounce_select_device": [v, i64, v, v, i64, v, P(i64), v],
        "tor_occluded_device": [v, i64, v, v, v, i64, d, d, i32, v, v],
        "tor_occluded_host": [v, i64, v, v, v, i64, d, d, i32, v],
        "tor_occluded_masked_device": [v, i64, v, v, v, i64, d, d, i32, v, v, v, u32],
        "tor_occluded_masked_host": [v, i64, v, v, v, i64, d, d, i32, v, v, u32],
        "tor_scene_groups": [v, i64, v],
        "tor_crossings_device": [v, i64, v, v, v, i64, i32, v, u32, d, d, i32, v, v, v, v],
        "tor_crossings_host": [v, i64, v, v, v, i64, i32, v, u32, d, d, i32, v, v, v],
        "tor_nearest_device": [v, i64, v, v, v, i64, i32, v, u32, d, d, i32, v, v, v],
        "tor_nearest_host": [v, i64, v, v, v, i64, i32, v, u32, d, d, i32, v, v],
        "tor_deposit_device": [v, i64, v, v, v, i64, d, i64, v, v, v, v, v],
        # include/tor_lights.h
        "tor_scene_lights": [v, i64, v, v],
        "tor_light_sample_device": [v, i64, v, v, v, i64, i32, v, v, v, v, v],
        "tor_light_sample_host": [v, i64, v, v, v, i64, i32, v, v, v, v],
        "tor_light_pdf_device": [v, i64, v, v, v, i64, i32, v, v],
        "tor_light_pdf_host": [v, i64, v, v, v, i64, i32, v],
        # include/tor_env.h
        "tor_scene_environment": [v, i64, v, v],
        "tor_env_sample_device": [v, i64, v, v, v, i64, v, v, v, v, v],
        "tor_env_sample_host": [v, i64, v, v, v, i64, v, v, v, v],
        "tor_env_eval_device": [v, i64, v, v, i64, v, v, v, v],
        "tor_env_eval_host": [v, i64, v, v, i64, v, v, v],
        # include/tor_camera.h
        "tor_camera_connect_device": [v, cam, i32, i32, i64, v, v, v, i64, v, v, v, v, v],
        "tor_camera_connect_host": [v, cam, i32, i32, i64, v, v, v, i64, v, v, v, v],
        "tor_light_emit_device": [v, i64, v, v, i64, d, d, v, v, v, v, v],
        "tor_light_emit_host": [v, i64, v, v, i64, d, d, v, v, v, v],
        # include/tor_bsdf.h
        "tor_bsdf_eval_device": [v, i64, v, v, v, v, i64, v, v, v, v],
        "tor_bsdf_eval_host": [v, i64, v, v, v, v, i64, v, v, v],
        # include/tor_photons.h
        "tor_photons_build_device": [v, i64, v, v, v, v, i64, d, v],
        "tor_photons_build_host": [v, i64, v, v, v, v, i64, d],
        "tor_photons_gather_device": [v, i64, v, v, v, v, i64, i32, d, v, v, v],
        "tor_photons_gather_host": [v, i64, v, v, v, v, i64, i32, d, v, v],
        "tor_photons_info": [v, v],
        # include/tor_media.h
        "tor_scene_media": [v, i64, v, v, v],
        "tor_media_march_device": [v, i64, v, v, v, v, i64, v, v, v, v, v, v],
        "tor_media_march_host": [v, i64, v, v, v, v, i64, v, v, v, v, v],
        "tor_media_scatter_device": [v, i64, v, v, v, v, v, i64, v, v, v],
        "tor_media_scatter_host": [v, i64, v, v, v, v, v, i64, v, v],
        "tor_rng_uniform_device": [v, i64, v, v, i64, i32, v, v],
        "tor_rng_uniform_host": [v, i64, v, v, i64, i32, v],
    }


_SIGNATURES = _signatures()


def _phase_signatures() -> dict:
    """The entries of include/tor_phase.h, in a table of their own: lib() binds them after _signatures()'s."""
    v, i64 = C.c_void_p, C.c_int64
    return {
        "tor_scene_media_phase": [v, i64, v],
        "tor_phase_eval_device": [v, i64, v, v, v, v, i64, v, v, v],
        "tor_phase_eval_host": [v, i64, v, v, v, v, i64, v, v],
        "tor_phase_sample_device": [v, i64, v, v, v, v, v, i64, v, v, v, v],
        "tor_phase_sample_host": [v, i64, v, v, v, v, v, i64, v, v, v],
    }


_PHASE_SIGNATURES = _phase_signatures()


def _reach_signatures() -> dict:
    """The entries of include/tor_reach.h, in a table of their own like the phase entries."""
    v, i32, i64, d, P = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.POINTER
    return {
        "tor_debug_reach_scene": [HittableList, i64] + [P(d)] * 3 + [P(C.c_int8), P(i32), P(i32), P(d), i64, P(i64)],
        "tor_debug_last_reach": [v, P(C.c_uint64)],
    }


_REACH_SIGNATURES = _reach_signatures()


def _grid_signatures() -> dict:
    """The entries of include/tor_grid.h, in a table of their own like the phase entries."""
    v, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    return {
        "tor_scene_media_grid": [v, i32, i32, i32, i32, v, v],
        "tor_media_grid_info": [v, i32, v, v, v],
        "tor_media_grid_march_device": [v, i64, v, v, v, i32, v, i64, v, v, v, v, v, v, v],
        "tor_media_grid_march_host": [v, i64, v, v, v, i32, v, i64, v, v, v, v, v, v],
        "tor_media_grid_density_device": [v, i64, v, i32, v, i64, v, v, v],
        "tor_media_grid_density_host": [v, i64, v, i32, v, i64, v, v],
    }


_GRID_SIGNATURES = _grid_signatures()


def _texture_signatures() -> dict:
    """The entries of include/tor_texture.h, in a table of their own like the phase entries."""
    v, i64 = C.c_void_p, C.c_int64
    return {
        "tor_scene_textures": [v, i64, v, i64, v, i64, v],
        "tor_texture_info": [v, v],
        "tor_texture_eval_device": [v, i64, v, v, i64, v, v, v],
        "tor_texture_eval_host": [v, i64, v, v, i64, v, v],
    }


_TEXTURE_SIGNATURES = _texture_signatures()


def _patch_signatures() -> dict:
    """The entries of include/tor_patches.h, in a table of their own like the texture entries."""
    v, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    return {
        "tor_scene_patches": [v, i64, v],
        "tor_patch_info": [v, v],
        "tor_patch_hit_device": [v, i64, v, v, v, i64, i32, v, v, v, v, v, u32],
        "tor_patch_hit_host": [v, i64, v, v, v, i64, i32, v, v, v, v, u32],
        "tor_patch_occluded_device": [v, i64, v, v, v, i64, i32, v, v, v, u32],
        "tor_patch_occluded_host": [v, i64, v, v, v, i64, i32, v, v, u32],
    }


_PATCH_SIGNATURES = _patch_signatures()


def _bind(L, names=None, skip_missing=False, table=None) -> None:
    """Give the named entries of the CDLL `L` (default: every entry of the table) their signatures.  A symbol `L` lacks raises,
    unless skip_missing (another build of the library, which may be older than the entry).  table: _SIGNATURES, or another."""
    table = _SIGNATURES if table is None else table
    for name in table if names is None else names:
        if skip_missing and not hasattr(L, name):
            continue
        sig = table[name]
        argtypes, *restype = sig if isinstance(sig, tuple) else (sig,)
        fn = getattr(L, name)
        if argtypes is not None:
            fn.argtypes = argtypes
        if restype:
            fn.restype = restype[0]


def _check(rc: int) -> None:
    if rc != 0:
        raise TorError(rc, lib().tor_last_error().decode("utf-8", "replace"))


# --------------------------------------------------------------------------------------
# Reference-interface mirrors
# --------------------------------------------------------------------------------------
# ---- host mirrors of support/rng.nim's seeding (splitmix64, rng.nim:22-53), vectorised: (n, 4) uint64 TorRng states ----------
_GOLDEN, _MIX = np.uint64(0x9e3779b97f4a7c15), np.uint64(0xbf58476d1ce4e5b9)


def _u64(x) -> np.ndarray:
    """x as a flat uint64 array: the two's-complement bits of negative integers, as the C ABI's uint64_t sees them."""
    a = np.asarray(x)
    if a.dtype.kind == "u":
        return a.astype(np.uint64).reshape(-1)
    if a.dtype.kind == "i":
        return a.astype(np.int64).view(np.uint64).reshape(-1)
    return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in a.reshape(-1)], dtype=np.uint64)


def _splitmix64(state: np.ndarray):
    """rng.nim:31-36: (next state, output)."""
    with np.errstate(over="ignore"):
        state = state + _GOLDEN
        r = (state ^ (state >> np.uint64(30))) * _MIX
        r = (r ^ (r >> np.uint64(27))) * _MIX
    return state, r ^ (r >> np.uint64(31))


def rng_seed1(x) -> np.ndarray:
    """rng.nim:38-44 seed(x) for every x: (n, 4) uint64."""
    sm = _u64(x)
    out = np.empty((sm.shape[0], 4), dtype=np.uint64)
    for k in range(4):
        sm, out[:, k] = _splitmix64(sm)
    return out


def rng_seed2(x, y) -> np.ndarray:
    """rng.nim:46-53 seed(x, y) = seed((x shl 32) xor y) -- render.nim:60's per-pixel stream seed(row, col)."""
    x, y = np.broadcast_arrays(_u64(x), _u64(y))
    return rng_seed1((x << np.uint64(32)) ^ y)


def rng_seed3(row, col, sample) -> np.ndarray:
    """TOR_SEED_SAMPLE's per-sample stream: h = splitmix64 output of the state (row shl 32) xor col, then seed(h xor sample)."""
    row, col, sample = np.broadcast_arrays(_u64(row), _u64(col), _u64(sample))
    _, h = _splitmix64((row << np.uint64(32)) ^ col)
    return rng_seed1(h ^ sample)


def vec3(x, y, z) -> Vec3:
    return Vec3(float(x), float(y), float(z))


def camera(look_from=(13, 2, 3), look_at=(0, 0, 0), view_up=(0, 1, 0), vertical_field_of_view=20.0,
           aspect_ratio=16.0 / 9.0, aperture=0.1, focus_distance=10.0, shutter_open=0.0,
           shutter_close=1.0) -> Camera:
    """camera() -- physics/cameras.nim:24-45; defaults = trace_of_radiance.nim:38-51."""
    cam = Camera()
    a, b, c = vec3(*look_from), vec3(*look_at), vec3(*view_up)
    _check(lib().tor_camera_init(C.byref(cam), C.byref(a), C.byref(b), C.byref(c),
                                 vertical_field_of_view, aspect_ratio, aperture, focus_distance,
                                 shutter_open, shutter_close))
    return cam


class Scene:
    """Scene / HittableList -- physics/hittables/hittables_lists.nim:15-46 (owner + borrowed view)."""

    def __init__(self, objects=None, n: int = 0):
        self.objects = objects if objects is not None else (HittableVariant * 1)()
        self.n = n

    def list(self) -> HittableList:
        return HittableList(self.n, C.cast(self.objects, C.POINTER(HittableVariant)))

    def __len__(self):
        return self.n

    @staticmethod
    def from_records(recs: np.ndarray) -> "Scene":
        """Build from flat (n,16) float64 records {kind, c0 xyz, c1 xyz, t0, t1, radius, material, albedo rgb, fuzz, ri}
        (the interchange format of the parity tests)."""
        n = int(recs.shape[0])
        arr = (HittableVariant * max(n, 1))()
        for i in range(n):
            r = recs[i]
            h = arr[i]
            mat = Material()
            mat.kind = int(r[10])
            if mat.kind == LAMBERTIAN:
                mat.u.lambertian.albedo = vec3(r[11], r[12], r[13])
            elif mat.kind == METAL:
                mat.u.metal.albedo = vec3(r[11], r[12], r[13])
                mat.u.metal.fuzz = float(r[14])
            else:
                mat.u.dielectric.refraction_index = float(r[15])
            if int(r[0]) == SPHERE:
                h.kind = SPHERE
                h.u.sphere.center = vec3(r[1], r[2], r[3])
                h.u.sphere.radius = float(r[9])
                h.u.sphere.material = mat
            else:
                h.kind = MOVING_SPHERE
                h.u.moving_sphere.center0 = vec3(r[1], r[2], r[3])
                h.u.moving_sphere.center1 = vec3(r[4], r[5], r[6])
                h.u.moving_sphere.time0 = float(r[7])
                h.u.moving_sphere.time1 = float(r[8])
                h.u.moving_sphere.radius = float(r[9])
                h.u.moving_sphere.material = mat
        return Scene(arr, n)

    def to_records(self) -> np.ndarray:
        """The scene as flat (n,16) float64 records (see from_records)."""
        out = np.zeros((self.n, 16), dtype=np.float64)
        for i in range(self.n):
            h = self.objects[i]
            if h.kind == SPHERE:
                s = h.u.sphere
                c0 = c1 = s.center
                t0, t1, rad, m = 0.0, 1.0, s.radius, s.material
            else:
                s = h.u.moving_sphere
                c0, c1, t0, t1, rad, m = s.center0, s.center1, s.time0, s.time1, s.radius, s.material
            out[i, 0] = h.kind
            out[i, 1:4] = (c0.x, c0.y, c0.z)
            out[i, 4:7] = (c1.x, c1.y, c1.z)
            out[i, 7:10] = (t0, t1, rad)
            out[i, 10] = m.kind
            if m.kind == LAMBERTIAN:
                a = m.u.lambertian.albedo
                out[i, 11:14] = (a.x, a.y, a.z)
            elif m.kind == METAL:
                a = m.u.metal.albedo
                out[i, 11:14] = (a.x, a.y, a.z)
                out[i, 14] = m.u.metal.fuzz
            else:
                out[i, 15] = m.u.dielectric.refraction_index
        return out


def random_scene(seed: int = 0xFACADE) -> Scene:
    """random_scene(rng) with rng.seed(seed) -- scenes.nim:13-50."""
    cap = 2048
    arr = (HittableVariant * cap)()
    n = lib().tor_random_scene(seed, arr, cap)
    if n < 0:
        raise TorError(int(n), "tor_random_scene failed")
    return Scene(arr, int(n))


class Animation:
    """random_moving_spheres + `iterator scenes` -- trace_of_radiance/scenes_animated.nim:90-225.

    ``for cam, scene, t in Animation(h, w, dt, t_min, t_max).scenes(skip=6): render(canvas, cam, scene.list(), depth)``
    mirrors trace_of_radiance_animation.nim:84-97."""

    def __init__(self, height: int, width: int, dt: float = 0.005, t_min: float = 0.0, t_max: float = 2.0,
                 seed: int = 0xFACADE):
        self._h = C.c_void_p()
        _check(lib().tor_animation_create(seed, height, width, dt, t_min, t_max, C.byref(self._h)))
        self.n_objects = int(lib().tor_animation_object_count(self._h))

    def scenes(self, skip: int = 6):
        while True:
            cam = Camera()
            arr = (HittableVariant * self.n_objects)()
            n = C.c_int64(0)
            t = C.c_float(0)
            rc = lib().tor_animation_next(self._h, skip, C.byref(cam), arr, self.n_objects, C.byref(n), C.byref(t))
            if rc == 0:
                return
            if rc < 0:
                raise TorError(rc, "tor_animation_next failed")
            yield cam, Scene(arr, int(n.value)), float(t.value)

    def close(self):
        if self._h:
            lib().tor_animation_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frames_of_rank(n_frames: int, rank: int, world: int):
    """Frame-parallel split of an animation: frame f is rendered by GPU f mod world."""
    return list(range(rank, n_frames, max(world, 1)))


class Canvas:
    """Canvas -- primitives/canvas.nim:20-41: row-major float64 RGB, row 0 = bottom scanline."""

    def __init__(self, height: int, width: int, samples_per_pixel: int, gamma_correction: float = 2.2):
        self.pixels = np.zeros((height, width, 3), dtype=np.float64)
        self.nrows, self.ncols = int(height), int(width)
        self.samples_per_pixel = int(samples_per_pixel)
        self.gamma_correction = float(gamma_correction)

    def struct(self) -> CanvasStruct:
        return CanvasStruct(self.pixels.ctypes.data_as(C.POINTER(Vec3)), self.nrows, self.ncols,
                            self.samples_per_pixel, self.gamma_correction)


def new_canvas(height, width, samples_per_pixel, gamma_correction=2.2) -> Canvas:
    return Canvas(height, width, samples_per_pixel, gamma_correction)


def make_options(seeding=SEED_PIXEL, arith=ARITH_STRICT, device=-1, shard_index=0, shard_count=1,
                 row_tile=1, accel=0, devices=None, gather=GATHER_AUTO, pixel_kernel=PIXEL_KERNEL_AUTO) -> Options:
    """TorOptions.  devices: a list of HIP ordinals -> tor_render_opt renders row shard k on devices[k] and
    assembles the frame in the canvas (`gather`)."""
    o = Options(C.sizeof(Options), seeding, arith, device, shard_index, shard_count, row_tile, accel)
    if devices:
        o.device_count = len(devices)
        for k, d in enumerate(devices):
            o.devices[k] = int(d)
    o.gather = gather
    o.pixel_kernel = pixel_kernel
    return o


def last_render_timing() -> dict:
    """Host-side cost of this thread's last render(): ms for upload, launch+kernels, download/gather, whole call."""
    t = (C.c_double * 5)()
    _check(lib().tor_last_render_timing(t))
    return {"upload_ms": t[0], "render_ms": t[1], "download_ms": t[2], "total_ms": t[3], "scene_cache_hit": bool(t[4])}


def last_note() -> str:
    """What the last multi-device render() on this thread chose / fell back to (tor_last_note)."""
    return lib().tor_last_note().decode("utf-8", "replace")


def knobs() -> list:
    """The library's environment knobs (csrc/tor_knobs.hpp): dicts {name, default, range, when, what}."""
    out = []
    for i in range(int(lib().tor_knob_count())):
        f = [C.c_char_p() for _ in range(5)]
        _check(lib().tor_knob_info(i, *[C.byref(x) for x in f]))
        out.append(dict(zip(("name", "default", "range", "when", "what"), (x.value.decode() for x in f))))
    return out


def last_gather_info() -> dict:
    """Facts about this thread's last multi-device render(): the gather leg, the RCCL communicator's rank count (0: not
    RCCL), entries of the device list, whether they were distinct GPUs (tor_last_gather_info)."""
    out = (C.c_int32 * 4)()
    _check(lib().tor_last_gather_info(out))
    return {"leg": {GATHER_RCCL: "rccl", GATHER_PEER: "peer", GATHER_HOST: "host"}.get(int(out[0]), "none"),
            "rccl_ranks": int(out[1]), "devices": int(out[2]), "distinct_devices": bool(out[3])}


def last_device_kernel_ms() -> list:
    """integrate_kernel's duration on every device of this thread's last multi-device render() (HIP events on each launch stream)."""
    buf = (C.c_float * 64)()
    n = int(lib().tor_last_device_kernel_ms(buf, 64))
    return [float(buf[k]) for k in range(min(n, 64))]


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * 128)()
    _check(lib().tor_comm_unique_id(buf))
    return bytes(buf)


def render(canvas: Canvas, cam: Camera, world: HittableList, max_depth: int, options: Options | None = None):
    """render(canvas, cam, world, max_depth) -- render.nim:49.  Blocking."""
    cs = canvas.struct()
    if options is None:
        _check(lib().tor_render(C.byref(cs), C.byref(cam), world, int(max_depth)))
    else:
        _check(lib().tor_render_opt(C.byref(cs), C.byref(cam), world, int(max_depth), C.byref(options)))


def export_rgb8(canvas: Canvas) -> np.ndarray:
    """exportToPPM's quantiser (io/ppm.nim:14-27): uint8 (nrows, ncols, 3), first row = top."""
    out = np.zeros((canvas.nrows, canvas.ncols, 3), dtype=np.uint8)
    cs = canvas.struct()
    _check(lib().tor_canvas_to_rgb8(C.byref(cs), out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def export_ppm(canvas: Canvas, f) -> None:
    """exportToPPM(canvas, f) -- io/ppm.nim:14-27 (ASCII P3)."""
    rgb = export_rgb8(canvas)
    f.write(f"P3\n{canvas.ncols} {canvas.nrows}\n255\n")
    for r, g, b in rgb.reshape(-1, 3):
        f.write(f"{r} {g} {b}\n")


def h264_stream_header(width: int, height: int) -> bytes:
    """SPS + PPS as H264Encoder.init writes them (io/h264.nim:90-142,37,174-176)."""
    buf = (C.c_uint8 * 64)()
    n = lib().tor_h264_stream_header(width, height, buf, 64)
    if n < 0:
        raise TorError(n, "tor_h264_stream_header failed")
    return bytes(buf[:n])


def h264_frame_bytes(width: int, height: int) -> int:
    n = int(lib().tor_h264_frame_bytes(width, height))
    if n < 0:
        raise TorError(n, "width and height must be multiples of 16")
    return n


def shard_rows(nrows: int, row_tile: int, shard_index: int, shard_count: int) -> np.ndarray:
    buf = (C.c_int32 * max(nrows, 1))()
    n = lib().tor_shard_rows(nrows, row_tile, shard_index, shard_count, buf)
    return np.array(buf[:n], dtype=np.int32)


# --------------------------------------------------------------------------------------
# The operand layer of the queries: everything a query does differently for CUDA tensors and for numpy arrays
# --------------------------------------------------------------------------------------
def _is_tensor(x) -> bool:
    """The module's one tensor-or-array decision (by the type's module: torch is never imported for a numpy caller)."""
    return type(x).__module__.startswith("torch")


def _shape(tail) -> str:
    return "(n, " + ", ".join(str(s) for s in tail) + ")" if tail else "(n,)"


class _Operands:
    """The operands of one query call, of the kind of its leading operand (_operands picks the subclass): `lead` is that operand,
    (n, cols) float64 and contiguous, `n` its rows.  A subclass checks and allocates arrays of its kind, gives their addresses
    and enters the library.  It knows nothing of the query but its name `who`, which words the refusals and names the entries
    tor_<who>_* and their note."""
    __slots__ = ("who", "name", "h", "lead", "n")

    def bad(self, what, must):
        raise ValueError(f"Context.{self.who}: {what} must be {must}")

    def words(self, buf):
        """The int32 words of a float64 buffer (object, front_face, which, inside)."""
        return buf.view(self.xp.int32)

    def times(self, col, time_range):
        """The time range of a call: the caller's, or the finite min / max of the leading operand's column col ((0, 0): none)."""
        if time_range is not None:
            return float(time_range[0]), float(time_range[1])
        return self._finite_range(self.lead[:, col])

    def mask(self, mask):
        """A mask that is not None: (what to keep alive, (the address of the per-row words or 0, the scalar word))."""
        if isinstance(mask, (int, np.integer)):
            return None, (0, int(mask) & 0xFFFFFFFF)
        words, address = self._per_row_mask(mask)
        return words, (address or 16, 0)

    def note(self, n_list) -> str:
        """tor_last_note of a listed query; one with no row to answer never reaches the code that writes it."""
        return last_note() if self.n and n_list else f"{self.who}: nothing to do"

    def call(self, *args, masked=None, after=()):
        """tor_<who>_device(ctx, n, *args, stream) or tor_<who>_host(ctx, n, *args); with masked = mask()'s pair the
        _masked_ twin, which takes the pair last.  after: what an entry without a twin takes behind the stream (the patch
        queries' mask pair)."""
        name = f"tor_{self.who}{'' if masked is None else '_masked'}{self.suffix}"
        _check(getattr(lib(), name)(self.h, self.n, *args, *self.tail, *(masked or ()), *after))


class _Tensors(_Operands):
    """CUDA tensors, zero-copy and asynchronous on torch's current stream: a contiguous tensor is the caller's own (what a query
    updates, it updates in place), another one is copied and the copy is what the result carries."""
    __slots__ = ("dev", "xp", "tail")
    suffix = "_device"

    def __init__(self, ctx, who, lead, name, cols, copy=False):
        import torch
        if not isinstance(lead, torch.Tensor) or lead.dtype != torch.float64 or lead.dim() != 2 or lead.shape[1] != cols \
                or not lead.is_cuda:
            raise ValueError(f"Context.{who}: {name} must be an (n, {cols}) float64 CUDA tensor")
        dev = getattr(ctx, "_device", None)
        if dev is not None and lead.device.index != dev:
            raise ValueError(f"Context.{who}: the {name} are on {lead.device}, the context on cuda:{dev}")
        self.who, self.name, self.h, self.xp = who, name, ctx._h, torch
        self.lead, self.n, self.dev = lead.contiguous(), int(lead.shape[0]), lead.device
        # what a _device entry takes after the arrays: the handle of torch's current stream on the device, read as
        # torch.cuda.current_stream(device).cuda_stream reads it but without building the Stream object (1 - 2 us of a small call)
        self.tail = (torch._C._cuda_getCurrentRawStream(lead.device.index),)

    def rows(self, x, what, *tail, dtype="float64", or_number=False):
        """A secondary operand: None, or an (n, *tail) tensor of dtype on the leading operand's device (or_number: or a number,
        one value for every row); contiguous."""
        if x is None:
            return None
        torch = self.xp
        if or_number and isinstance(x, (int, float, np.floating, np.integer)):
            x = torch.full((self.n,), float(x), dtype=torch.float64, device=self.dev)
        elif not isinstance(x, torch.Tensor) or x.dtype != getattr(torch, dtype) or tuple(x.shape) != (self.n, *tail) \
                or x.device != self.dev:
            self.bad(what, f"{'a number or ' if or_number else ''}an {_shape(tail)} {dtype} tensor on the {self.name}' device")
        return x.contiguous()

    def states(self, rng):
        """(n, 4) generator states, int64 holding the u64 bits."""
        torch = self.xp
        if not isinstance(rng, torch.Tensor) or rng.dtype not in (torch.int64, torch.uint64) or tuple(rng.shape) != (self.n, 4) \
                or rng.device != self.dev:
            self.bad("rng", f"an (n, 4) int64 tensor on the {self.name}' device")
        return rng.contiguous()

    def new(self, *shape, dtype="float64", unused=None, zero=True):
        """An output buffer, zeroed (zero=False: uninitialised), the int32 word `unused` of every entry -1."""
        torch = self.xp
        buf = (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, dtype), device=self.dev)
        if unused is not None:
            buf.view(torch.int32)[..., unused] = -1
        return buf

    def fits(self, buf, *shape, dtype="float64") -> bool:
        """Can a caller's `out` buffer be written again by this call?"""
        torch = self.xp
        return isinstance(buf, torch.Tensor) and buf.dtype == getattr(torch, dtype) and tuple(buf.shape) == shape \
            and buf.device == self.dev and buf.is_contiguous()

    def holds(self, buf) -> bool:
        """Is buf a tensor of n rows on this device (what a step asks of the `out` it writes again)?"""
        return isinstance(buf, self.xp.Tensor) and int(buf.shape[0]) == self.n and buf.device == self.dev

    def index(self, index):
        return _tensor_list(index, self.n, self.dev)

    def as_bool(self, buf):
        """The low byte of every int32 as a bool view."""
        return buf.view(self.xp.bool).view(self.n, 4)[:, 0]

    def ptr(self, x) -> int:
        return 0 if x is None else x.data_ptr()

    def keep(self, *refs):
        """What a result must keep alive while the query may still run: contiguous copies nobody else holds."""
        return refs

    def _finite_range(self, t):
        torch = self.xp
        t = t[torch.isfinite(t)]
        return (0.0, 0.0) if t.numel() == 0 else tuple(float(v) for v in torch.aminmax(t))

    def _per_row_mask(self, mask):
        torch = self.xp
        if not _is_tensor(mask):
            mask = torch.from_numpy(_mask_words(np.asarray(mask).reshape(-1)).view(np.int32))
        if mask.dtype not in (torch.int32, torch.uint32) or tuple(mask.shape) != (self.n,):
            self.bad("a per-ray mask", "an (n,) uint32 / int32 tensor or array")
        mask = mask.to(self.dev).contiguous()
        return mask, mask.data_ptr()


class _Arrays(_Operands):
    """Anything numpy takes, through the blocking _host entries: a read-only query may alias a contiguous float64 input, what a
    query updates is copied first (copy=True for the leading operand, always for the states), so the caller's arrays are never
    written.  n == 0 passes NULL for every array."""
    __slots__ = ()
    suffix, xp, dev, tail = "_host", np, None, ()

    def __init__(self, ctx, who, lead, name, cols, copy=False):
        lead = np.array(lead, dtype=np.float64, order="C") if copy else np.ascontiguousarray(lead, dtype=np.float64)
        if lead.ndim != 2 or lead.shape[1] != cols:
            raise ValueError(f"Context.{who}: {name} must be an (n, {cols}) float64 array")
        self.who, self.name, self.h = who, name, ctx._h
        self.lead, self.n = lead, int(lead.shape[0])

    def rows(self, x, what, *tail, dtype="float64", or_number=False):
        """A secondary operand: None, or anything numpy makes an (n, *tail) array of dtype from (or_number: or a number, one value
        for every row); contiguous."""
        if x is None:
            return None
        if or_number and np.ndim(x) == 0:
            x = np.full((self.n,), float(x), dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.shape != (self.n, *tail):
            self.bad(what, f"{'a number or ' if or_number else ''}an {_shape(tail)} {dtype} array")
        return x

    def states(self, rng):
        """(n, 4) generator states as uint64: a copy."""
        st = np.asarray(rng)
        if st.shape != (self.n, 4) or st.dtype.kind not in "iu" or st.dtype.itemsize != 8:
            self.bad("rng", "an (n, 4) array of 64-bit integers")
        return np.ascontiguousarray(st).view(np.uint64).copy()

    def new(self, *shape, dtype="float64", unused=None, zero=True):
        """An output buffer, zeroed (always: a host entry's caller reads it at once), the int32 word `unused` of every entry -1."""
        buf = np.zeros(shape, dtype=dtype)
        if unused is not None:
            buf.view(np.int32)[..., unused] = -1
        return buf

    def fits(self, buf, *shape, dtype="float64") -> bool:
        """Can a caller's `out` buffer be written again by this call?"""
        return isinstance(buf, np.ndarray) and buf.dtype == dtype and buf.shape == shape and buf.flags.c_contiguous

    def holds(self, buf) -> bool:
        """Is buf an array of n rows (what a step asks of the `out` it writes again)?"""
        return isinstance(buf, np.ndarray) and buf.shape[0] == self.n

    def index(self, index):
        if index is None:
            return None, self.n, 0
        index = np.ascontiguousarray(np.asarray(index).reshape(-1), dtype=np.int32)
        return index, int(index.size), index.ctypes.data or 16   # (an empty list is a list: never dereferenced)

    def as_bool(self, buf):
        """The low byte of every int32 as a bool view."""
        return buf.view(np.bool_).reshape(self.n, 4)[:, 0]

    def ptr(self, x) -> int:
        return x.ctypes.data if x is not None and self.n else 0

    def keep(self, *refs):
        """Nothing: a host entry has returned before the result exists."""
        return None

    def _finite_range(self, t):
        t = t[np.isfinite(t)]
        return (0.0, 0.0) if t.size == 0 else (float(t.min()), float(t.max()))

    def _per_row_mask(self, mask):
        words = _mask_words(mask.cpu().numpy() if _is_tensor(mask) else np.asarray(mask))
        if words.shape != (self.n,):
            self.bad("a per-ray mask", "an (n,) uint32 / int32 tensor or array")
        return words, words.ctypes.data


def _operands(ctx, who, lead, name, cols, copy=False) -> _Operands:
    return (_Tensors if _is_tensor(lead) else _Arrays)(ctx, who, lead, name, cols, copy)


def _tensor_list(index, n, device):
    """The list of a listed query as a device tensor: (contiguous int32 tensor or None, n_list, its address -- 0 for None: every row)."""
    if index is None:
        return None, n, 0
    import torch
    index = torch.as_tensor(index).to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    return index, int(index.numel()), index.data_ptr() or 16   # (an empty list is a list: never dereferenced)


class Context:
    """Resident device context (tor_context_* / tor_scene_upload / tor_render_device)."""

    def __init__(self, device: int = -1):
        self._h = C.c_void_p()
        self.last_incomplete = False   # set by last_kernel_ms(): the last launch's hand-off stalled, its frame is not whole
        _check(lib().tor_context_create(device, C.byref(self._h)))
        # the context's device ordinal (-1: the current device, as the library resolves it) -- hit() checks tensors against it
        torch = sys.modules.get("torch")
        self._device = device if device >= 0 else (torch.cuda.current_device() if torch is not None else None)

    def close(self):
        if self._h:
            lib().tor_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, world: HittableList):
        _check(lib().tor_scene_upload(self._h, world))
        self._n_uploaded = int(world.len)

    def set_stats(self, enable: bool):
        _check(lib().tor_context_set_stats(self._h, int(enable)))

    def render_device(self, cam: Camera, nrows: int, ncols: int, spp: int, gamma: float, max_depth: int,
                      options: Options, d_pixels_ptr: int, stream_ptr: int = 0):
        """Asynchronous on the given hipStream_t; d_pixels_ptr is a device pointer."""
        _check(lib().tor_render_device(self._h, C.byref(cam), nrows, ncols, spp, gamma, int(max_depth),
                                       C.byref(options), C.c_void_p(d_pixels_ptr), C.c_void_p(stream_ptr)))

    def accumulate_device(self, cam: Camera, nrows: int, ncols: int, first_sample: int, n_samples: int, max_depth: int,
                          options: Options, d_sums_ptr: int, d_moments_ptr: int = 0, stream_ptr: int = 0):
        """Adds samples [first_sample, first_sample + n_samples) of this shard's rows to the raw sums at d_sums_ptr (and their second
        moments at d_moments_ptr, 0 = none); never clears them.  TOR_SEED_SAMPLE only.  Asynchronous on the given hipStream_t."""
        _check(lib().tor_render_accumulate_device(self._h, C.byref(cam), nrows, ncols, first_sample, n_samples, int(max_depth),
                                                  C.byref(options), C.c_void_p(d_sums_ptr), C.c_void_p(d_moments_ptr),
                                                  C.c_void_p(stream_ptr)))

    def resume_device(self, cam: Camera, nrows: int, ncols: int, first_sample: int, n_samples: int, max_depth: int,
                      options: Options, d_rng_ptr: int, d_sums_ptr: int, d_moments_ptr: int = 0, stream_ptr: int = 0):
        """Runs samples [first_sample, first_sample + n_samples) of every pixel's own stream (TOR_SEED_PIXEL only): first_sample == 0
        seeds the pixels and starts the sums, > 0 continues from the generator states at d_rng_ptr (one TorRng per pixel) and the raw
        sequential sums at d_sums_ptr (and the sums of c * c at d_moments_ptr, 0 = none); all three are stored back.  Asynchronous on
        the given hipStream_t."""
        _check(lib().tor_render_resume_device(self._h, C.byref(cam), nrows, ncols, first_sample, n_samples, int(max_depth),
                                              C.byref(options), C.c_void_p(d_rng_ptr), C.c_void_p(d_sums_ptr),
                                              C.c_void_p(d_moments_ptr), C.c_void_p(stream_ptr)))

    def resolve_device(self, d_sums_ptr: int, n_values: int, total_samples: int, gamma: float, d_pixels_ptr: int,
                       stream_ptr: int = 0):
        """pixels = pow(sums / total_samples, 1 / gamma), the sums left as they are.  Asynchronous on the given hipStream_t."""
        _check(lib().tor_resolve_device(self._h, C.c_void_p(d_sums_ptr), n_values, total_samples, gamma,
                                        C.c_void_p(d_pixels_ptr), C.c_void_p(stream_ptr)))

    def accum_noise_device(self, d_sums_ptr: int, d_moments_ptr: int, npix: int, total_samples: int, d_err_ptr: int = 0,
                           stream_ptr: int = 0):
        """(mean, max) over the pixels of the largest per-channel standard error of the mean; d_err_ptr (0 = none) receives it per
        pixel.  Blocking."""
        out = (C.c_double * 2)()
        _check(lib().tor_accum_noise_device(self._h, C.c_void_p(d_sums_ptr), C.c_void_p(d_moments_ptr), npix, total_samples,
                                            C.c_void_p(d_err_ptr), out, C.c_void_p(stream_ptr)))
        return float(out[0]), float(out[1])

    def accumulate_list_device(self, cam: Camera, nrows: int, ncols: int, d_list_ptr: int, n_list: int, first_sample: int,
                               n_samples: int, max_depth: int, options: Options, d_sums_ptr: int, d_moments_ptr: int, stream_ptr: int = 0):
        """accumulate_device over the n_list pixels of the device int32 list at d_list_ptr (shard-local, strictly ascending, unique);
        sums and moments both required.  Asynchronous on the given hipStream_t."""
        _check(lib().tor_render_accumulate_list_device(self._h, C.byref(cam), nrows, ncols, C.c_void_p(d_list_ptr), int(n_list),
                                                       int(first_sample), int(n_samples), int(max_depth), C.byref(options),
                                                       C.c_void_p(d_sums_ptr), C.c_void_p(d_moments_ptr), C.c_void_p(stream_ptr)))

    def resume_list_device(self, cam: Camera, nrows: int, ncols: int, d_list_ptr: int, n_list: int, first_sample: int, n_samples: int,
                           max_depth: int, options: Options, d_rng_ptr: int, d_sums_ptr: int, d_moments_ptr: int, stream_ptr: int = 0):
        """resume_device over the n_list pixels of the device int32 list at d_list_ptr (shard-local, strictly ascending, unique):
        generator states, sums and moments all required; a pixel that is not listed keeps every bit of the three.  TOR_SEED_PIXEL
        only.  Asynchronous on the given hipStream_t."""
        _check(lib().tor_render_resume_list_device(self._h, C.byref(cam), nrows, ncols, C.c_void_p(d_list_ptr), int(n_list),
                                                   int(first_sample), int(n_samples), int(max_depth), C.byref(options),
                                                   C.c_void_p(d_rng_ptr), C.c_void_p(d_sums_ptr), C.c_void_p(d_moments_ptr),
                                                   C.c_void_p(stream_ptr)))

    def adaptive_select_device(self, d_sums_ptr: int, d_moments_ptr: int, d_list_in_ptr: int, n_in: int, total_samples: int,
                               abs_tol: float, rel_tol: float, d_list_out_ptr: int, d_counts_ptr: int, stream_ptr: int = 0) -> int:
        """Convergence test at total_samples of every listed pixel: counts[p] = total_samples, the unconverged pixels to the output
        list in input order.  Returns their number.  Blocking."""
        n = C.c_int32(0)
        _check(lib().tor_adaptive_select_device(self._h, C.c_void_p(d_sums_ptr), C.c_void_p(d_moments_ptr), C.c_void_p(d_list_in_ptr),
                                                int(n_in), int(total_samples), float(abs_tol), float(rel_tol), C.c_void_p(d_list_out_ptr),
                                                C.c_void_p(d_counts_ptr), C.byref(n), C.c_void_p(stream_ptr)))
        return int(n.value)

    def resolve_counts_device(self, d_sums_ptr: int, d_counts_ptr: int, npix: int, gamma: float, d_pixels_ptr: int, stream_ptr: int = 0):
        """pixels = pow(sums / counts[pixel], 1 / gamma), each pixel resolved at its own sample count.  Asynchronous."""
        _check(lib().tor_resolve_counts_device(self._h, C.c_void_p(d_sums_ptr), C.c_void_p(d_counts_ptr), int(npix), gamma,
                                               C.c_void_p(d_pixels_ptr), C.c_void_p(stream_ptr)))

    def quantize_rgb8_device(self, d_pixels_ptr: int, n_values: int, d_rgb8_ptr: int, stream_ptr: int = 0):
        _check(lib().tor_quantize_rgb8_device(self._h, C.c_void_p(d_pixels_ptr), n_values,
                                              C.c_void_p(d_rgb8_ptr), C.c_void_p(stream_ptr)))

    def encode_frame_device(self, d_pixels_ptr: int, nrows: int, ncols: int, d_slice_ptr: int, d_y_ptr: int = 0,
                            d_cb_ptr: int = 0, d_cr_ptr: int = 0, stream_ptr: int = 0):
        """canvas -> RGB8 -> Y'CbCr 4:2:0 -> I_PCM slice bytes (io/rgb.nim, color_conversions.nim, h264.nim)."""
        _check(lib().tor_encode_frame_device(self._h, C.c_void_p(d_pixels_ptr), nrows, ncols, C.c_void_p(d_slice_ptr),
                                             C.c_void_p(d_y_ptr), C.c_void_p(d_cb_ptr), C.c_void_p(d_cr_ptr),
                                             C.c_void_p(stream_ptr)))

    def render_frame_h264(self, cam: Camera, nrows: int, ncols: int, spp: int, gamma: float, max_depth: int,
                          options: Options | None = None) -> bytes:
        """Render the uploaded scene and return the frame's I_PCM slice (animation driver loop body)."""
        n = h264_frame_bytes(ncols, nrows)
        buf = (C.c_uint8 * n)()
        _check(lib().tor_render_frame_h264(self._h, C.byref(cam), nrows, ncols, spp, gamma, int(max_depth),
                                           C.byref(options) if options is not None else None, buf, n))
        return bytes(buf)

    def scene_counters(self):
        """(uploads, cache hits, device layouts built)"""
        out = (C.c_int64 * 3)()
        _check(lib().tor_context_scene_counters(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def comm_init_rank(self, unique_id: bytes, rank: int, world: int):
        """ncclCommInitRank inside the library (one process per GPU; id from comm_unique_id() of rank 0)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(lib().tor_comm_init_rank(self._h, buf, rank, world))

    def comm_destroy(self):
        _check(lib().tor_comm_destroy(self._h))

    def comm_abort(self):
        """ncclCommAbort (a gather that does not complete: RCCL's kernels leave)."""
        _check(lib().tor_comm_abort(self._h))

    def comm_count(self) -> int:
        """Ranks of the context's RCCL communicator (ncclCommCount); 0 without one."""
        n = C.c_int32(0)
        _check(lib().tor_comm_count(self._h, C.byref(n)))
        return int(n.value)

    def handoff_stalled(self):
        """(stalled, frames re-rendered so far) of the last launch's chain hand-off (tor_context_handoff_stalled); blocks."""
        st = C.c_int32(0)
        tot = C.c_int64(0)
        _check(lib().tor_context_handoff_stalled(self._h, C.byref(st), C.byref(tot)))
        return bool(st.value), int(tot.value)

    def render_gather_device(self, cam: Camera, nrows: int, ncols: int, spp: int, gamma: float, max_depth: int,
                             options: Options, root: int, d_frame_ptr: int, stream_ptr: int = 0):
        """This rank's row shard + the RCCL framebuffer gather + de-interleave, asynchronous on the stream."""
        _check(lib().tor_render_gather_device(self._h, C.byref(cam), nrows, ncols, spp, gamma, int(max_depth),
                                              C.byref(options), root, C.c_void_p(d_frame_ptr), C.c_void_p(stream_ptr)))

    def last_kernel_ms(self):
        """(kernel ms by HIP events, pixel-samples traced) of the last launch.  TOR_ERR_INCOMPLETE -- the launch's chain hand-off
        stalled and flagged the frame -- does not raise: the timing is valid, `self.last_incomplete` says the frame is not."""
        ms = C.c_float(0)
        n = C.c_int64(0)
        rc = lib().tor_last_kernel_ms(self._h, C.byref(ms), C.byref(n))
        self.last_incomplete = (rc == ERR_INCOMPLETE)
        if rc != ERR_INCOMPLETE:
            _check(rc)
        return float(ms.value), int(n.value)

    def kernel_ms_mean(self, last_n: int):
        ms = C.c_float(0)
        n = C.c_int32(0)
        _check(lib().tor_kernel_ms_mean(self._h, last_n, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def last_pixel_cost(self, n_pixels: int) -> np.ndarray:
        """Per-pixel closest-hit query counts of the last launch's cost probe (debug; tor_last_pixel_cost)."""
        buf = np.zeros(n_pixels, dtype=np.uint32)
        n = lib().tor_last_pixel_cost(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n_pixels)
        if n < 0:
            _check(int(n))
        return buf[:n]

    def last_handoff_counters(self) -> dict:
        """Chain hand-off of the last SEED_PIXEL launch (tor_last_handoff_counters)."""
        out = (C.c_uint64 * 16)()
        _check(lib().tor_last_handoff_counters(self._h, out))
        names = ("tickets", "pushed", "lane_waves_left", "server_workgroups", "push_threshold", "served", "hot_pushes", "tail_pushes",
                 "us_counter_dry", "us_lane_end", "us_hot_done", "us_tail_done", "its_hot", "its_tail", "servers_converted", "push_threshold_end")
        return {k: int(v) for k, v in zip(names, out)}

    def last_wave_log(self, cap_waves: int = 16384) -> np.ndarray:
        buf = np.zeros((cap_waves, 8), dtype=np.uint64)
        n = lib().tor_last_wave_log(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), cap_waves)
        if n < 0:
            _check(n)
        return buf[:n]

    def last_variant(self) -> tuple:
        """(seeding, arith, w, f32, blocks) of the integrate_kernel variant of the context's last render launch, all -1 before the
        first (tor_debug_last_variant)."""
        out = (C.c_int32 * 5)()
        _check(lib().tor_debug_last_variant(self._h, out))
        return tuple(int(v) for v in out)

    def last_split_tiles(self) -> int:
        """Tiles of 64 pixels the wave-per-pixel kernel took in the last launch's split mode, 0 when the launch ran one kernel
        (tor_debug_last_split_tiles).  Blocking."""
        out = C.c_int64(0)
        _check(lib().tor_debug_last_split_tiles(self._h, C.byref(out)))
        return int(out.value)

    def last_stats(self) -> Stats:
        st = Stats()
        _check(lib().tor_last_stats(self._h, C.byref(st)))
        return st

    def last_reach(self):
        """(whole words of the plane screen's stage one the last strict brute-force launch walked, whole words it met): the reach
        pass's counters (tor_debug_last_reach; statistics must be enabled).  Blocking."""
        out = (C.c_uint64 * 2)()
        _check(lib().tor_debug_last_reach(self._h, out))
        return int(out[0]), int(out[1])

    def set_groups(self, groups):
        """The visibility groups of the uploaded scene (tor_scene_groups): one 32-bit word per object, in list order -- anything
        numpy takes, uint32 or int32 (by its bits); None resets every object to 0xFFFFFFFF, the state after every upload that
        replaces the scene.  Object j takes part in a query of ray i with mask m_i iff groups[j] & m_i != 0 (the `mask` keyword of
        hit / occluded / visible / bounce / trace).  Renders and queries without a mask never read the words."""
        if groups is None:
            _check(lib().tor_scene_groups(self._h, getattr(self, "_n_uploaded", -1), C.c_void_p(0)))
            return
        g = _mask_words(np.asarray(groups).reshape(-1))
        _check(lib().tor_scene_groups(self._h, int(g.size), C.c_void_p(g.ctypes.data or 16)))

    def set_lights(self, objects, weights=None):
        """The light table of the uploaded scene (tor_scene_lights): `objects` are the indices of the emitters in the uploaded list
        (unique), `weights` one finite number >= 0 per light (None: all 1; at least one > 0) -- the emitted power, for example
        luminance * radius ** 2.  sample_lights / light_pdf / trace_direct read it.  An empty `objects` clears the table, and so
        does every upload that replaces the scene."""
        o = np.ascontiguousarray(np.asarray(objects).reshape(-1), dtype=np.int32)
        if weights is None:
            _check(lib().tor_scene_lights(self._h, int(o.size), C.c_void_p(o.ctypes.data or 16), C.c_void_p(0)))
            return
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.size != o.size:
            raise ValueError("Context.set_lights: one weight per light")
        _check(lib().tor_scene_lights(self._h, int(o.size), C.c_void_p(o.ctypes.data or 16), C.c_void_p(w.ctypes.data or 16)))

    def set_environment(self, rgb, importance=None):
        """The environment map of the context (tor_scene_environment): `rgb` is (n, n, 3) float64, finite and >= 0, the texels of
        an octahedral map in [row][col] order (environment_directions(n) gives the direction of every texel centre, so any sky
        is baked with one call); `importance` (n, n), finite and >= 0, is what sample_environment picks a texel by -- None: the
        texel's luminance times its solid angle.  None for `rgb` clears the map.  The map belongs to the context, not to the
        scene: uploads leave it alone, and environment / sample_environment need no scene."""
        if rgb is None:
            _check(lib().tor_scene_environment(self._h, 0, C.c_void_p(0), C.c_void_p(0)))
            return
        c = np.ascontiguousarray(np.asarray(rgb, dtype=np.float64))
        if c.ndim != 3 or c.shape[0] != c.shape[1] or c.shape[2] != 3 or c.shape[0] < 1:
            raise ValueError("Context.set_environment: rgb must be (n, n, 3) with n >= 1")
        n = int(c.shape[0])
        if importance is None:
            _check(lib().tor_scene_environment(self._h, n, C.c_void_p(c.ctypes.data), C.c_void_p(0)))
            return
        w = np.ascontiguousarray(np.asarray(importance, dtype=np.float64))
        if w.shape != (n, n):
            raise ValueError("Context.set_environment: importance must be (n, n), one value per texel")
        _check(lib().tor_scene_environment(self._h, n, C.c_void_p(c.ctypes.data), C.c_void_p(w.ctypes.data)))

    def _cuda(self):
        """The context's torch device (the current one for a context on the library's default device)."""
        import torch
        return torch.device("cuda", self._device if getattr(self, "_device", None) is not None else torch.cuda.current_device())

    def _to_device(self, a, dtype=None):
        """A numpy operand of a query that only the device answers: its contiguous copy on the context's device."""
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self._cuda())

    def hit(self, rays, t_range=None, time_range=None, mode="auto", mask=None) -> "HitResult":
        """Closest hits of a batch of rays against the uploaded scene: world.hit(r, t_min, t_max, rec) of the reference
        (hittables_lists.nim:48-55), bit for bit, per ray (tor_hit_device / tor_hit_host).

        rays: (n, 7) float64 {origin xyz, direction xyz, time} -- a torch CUDA tensor (zero-copy, asynchronous on torch's current
        stream) or anything numpy takes (copied, blocking).  t_range: None (render.nim's (0.001, +inf)) or (n, 2) {t_min, t_max} of
        the same kind; t_min >= 0 lets a ray use the block culling.  time_range: (lo, hi) the block bounds are built for (a speed hint:
        rays outside it are still exact); None = the finite min / max of the rays' times.  mode: "auto" | "brute" | "blocks".
        mask: None (every object), or an int / a per-ray (n,) uint32 or int32 tensor or array: ray i sees object j iff
        groups[j] & mask_i != 0 (set_groups) -- world.hit on the sub-list it sees, `object` the index in the full list."""
        m = HIT_MODES[mode] if isinstance(mode, str) else int(mode)
        ops = _operands(self, "hit", rays, "rays", 7)
        rays = ops.lead
        t_range = ops.rows(t_range, "t_range", 2)
        tr = ops.times(6, time_range)
        raw = ops.new(ops.n, 8, zero=False)
        mk, masked = (None, None) if mask is None else ops.mask(mask)
        ops.call(ops.ptr(rays), ops.ptr(t_range), tr[0], tr[1], m, ops.ptr(raw), masked=masked)
        return HitResult(raw, ops.words(raw), last_note(), keep=ops.keep(rays, t_range, mk))

    def radiance(self, rays, rng, max_depth=50, time_range=None, mode="auto"):
        """radiance(ray, world, max_depth, rng) of the reference (render.nim:21-47), bit for bit, per ray, on the uploaded scene
        (tor_radiance_device / tor_radiance_host).  Returns (color (n, 3) float64, rng (n, 4): the states after the path's last draw,
        mode: what ran, "blocks" or "brute force (...)").

        rays: (n, 7) float64 {origin xyz, direction xyz, time}; rng: (n, 4) xoshiro256+ states (rng_seed1/2/3, or camera_rays').
        Torch CUDA tensors (rng as int64 holding the u64 bits) are passed zero-copy, asynchronous on torch's current stream, and a
        contiguous rng tensor is updated in place; anything numpy takes is copied (blocking) and the states come back as uint64.
        time_range: (lo, hi) the block bounds are built for (a speed hint; the library adds 0); None = the rays' finite times.
        mode: "auto" | "brute" | "blocks"."""
        m = HIT_MODES[mode] if isinstance(mode, str) else int(mode)
        ops = _operands(self, "radiance", rays, "rays", 7)
        rng = ops.states(rng)
        tr = ops.times(6, time_range)
        color = ops.new(ops.n, 3, zero=False)
        ops.call(ops.ptr(ops.lead), ops.ptr(rng), int(max_depth), tr[0], tr[1], m, ops.ptr(color))
        return color, rng, _mode_of(last_note(), "radiance: ")

    def camera_rays(self, cam: Camera, nrows: int, ncols: int, first_sample: int = 0, n_samples: int = 1, seeding=SEED_SAMPLE,
                    pixels=None, rng=None):
        """The library's camera rays (render.nim:63-65 + cameras.nim:47-57, tor_camera_rays_device) for every pixel or a list of
        flat pixel indices row * ncols + col (row 0 = bottom): returns (rays (m, 7) float64, rng (m, 4) int64), CUDA tensors on the
        context's device, asynchronous on torch's current stream -- the rays and the states after the camera's draws, ready for
        radiance().  SEED_SAMPLE: seed3(row, col, s) for s in [first_sample, first_sample + n_samples), entry e and sample s at
        e * n_samples + (s - first_sample).  SEED_PIXEL: n_samples = 1 and rng (n_pixels, 4) the states to draw from (rng_seed2,
        or what radiance() left), updated in place when it is a contiguous int64 CUDA tensor."""
        import torch
        dev = self._cuda()
        if pixels is not None:
            pixels = torch.as_tensor(pixels).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            n_pix = int(pixels.numel())
        else:
            n_pix = int(nrows) * int(ncols)
        m = n_pix * int(n_samples)
        if int(seeding) == SEED_PIXEL:
            if rng is None:
                raise ValueError("Context.camera_rays: SEED_PIXEL needs the per-pixel states (rng)")
            if not isinstance(rng, torch.Tensor):
                rng = torch.from_numpy(np.ascontiguousarray(np.asarray(rng)).view(np.int64))
            rng = rng.to(device=dev).contiguous()
            if rng.dtype not in (torch.int64, torch.uint64) or tuple(rng.shape) != (m, 4):
                raise ValueError("Context.camera_rays: rng must be (n_pixels, 4) 64-bit integers")
        else:
            rng = torch.empty((m, 4), dtype=torch.int64, device=dev)
        rays = torch.empty((m, 7), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().tor_camera_rays_device(self._h, C.byref(cam), int(nrows), int(ncols),
                                            C.c_void_p(pixels.data_ptr() if pixels is not None else 0), n_pix, int(first_sample),
                                            int(n_samples), int(seeding), C.c_void_p(rng.data_ptr()), C.c_void_p(rays.data_ptr()),
                                            C.c_void_p(stream)))
        return rays, rng

    # ---- path steps (tor_bounce_device and friends): the pieces of radiance()'s loop for hosts that write their own integrator ----

    def bounce(self, rays, rng, index=None, time_range=None, mode="auto", out=None, mask=None) -> "BounceResult":
        """One iteration of radiance()'s loop (render.nim:26-38) for the listed rays, bit for bit (tor_bounce_device /
        tor_bounce_host): world.hit(ray, 0.001, +inf, rec), then rec.material.scatter(ray, rec, rng, attenuation, scattered).

        rays (n, 7) float64 and rng (n, 4) 64-bit states: torch CUDA tensors are passed zero-copy, asynchronous on torch's current
        stream, and contiguous ones are updated in place (a hit ray becomes `scattered`, its state the one after the scatter's last
        draw); anything numpy takes is copied (blocking).  index: the rays to step (int32, unique; entries outside [0, n) are
        skipped), None = all.  Arrays are indexed by the ray, so a host keeps full-size arrays and a shrinking index.  Returns a
        BounceResult: HitResult's fields, attenuation (n, 3), status (n,) int32 (BOUNCE_MISS / BOUNCE_SCATTERED / BOUNCE_ABSORBED),
        rays and rng (the updated arrays) and the mode that ran.  out: a BounceResult of an earlier step on as many rays, whose
        arrays are written again (rays that are not listed keep what they hold); otherwise new ones (object -1, the rest 0).
        mask: as for hit() (per-ray words are indexed by the ray): the closest VISIBLE object scatters; a ray that sees nothing
        misses, draws nothing and keeps its ray and state."""
        m = HIT_MODES[mode] if isinstance(mode, str) else int(mode)
        if mask is not None and not _is_tensor(rays):   # (the masked step has no blocking entry: through the device and back)
            import torch
            host = _Arrays(self, "bounce", np.array(rays, dtype=np.float64).reshape(-1, 7), "rays", 7)
            r, s = self._to_device(host.lead), self._to_device(host.states(rng).view(np.int64))
            if out is not None and isinstance(out.raw, np.ndarray):
                raw = self._to_device(out.raw)
                out = BounceResult(raw, raw.view(torch.int32), "", self._to_device(out.attenuation), self._to_device(out.status), None, None)
            res = self.bounce(r, s, index, time_range, mode, out, mask)
            torch.cuda.synchronize(r.device)
            raw = res.raw.cpu().numpy()
            return BounceResult(raw, raw.view(np.int32), "bounce: " + res.mode, res.attenuation.cpu().numpy(), res.status.cpu().numpy(),
                                res.rays.cpu().numpy(), res.rng.cpu().numpy().view(np.uint64))
        ops = _operands(self, "bounce", rays, "rays", 7, copy=True)
        n, rays = ops.n, ops.lead
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        tr = ops.times(6, time_range)
        if out is not None and ops.holds(out.raw):
            raw, att, status = out.raw, out.attenuation, out.status
        else:
            raw, att, status = ops.new(n, 8, unused=14), ops.new(n, 3), ops.new(n, dtype="int32")
        mk, masked = (None, None) if mask is None else ops.mask(mask)
        ops.call(ops.ptr(rays), ops.ptr(rng), p_list, n_list, tr[0], tr[1], m, ops.ptr(raw), ops.ptr(att), ops.ptr(status),
                 masked=masked)
        return BounceResult(raw, ops.words(raw), ops.note(n_list), att, status, rays, rng, keep=ops.keep(index, mk))

    def scatter(self, rays, hits, rng, index=None, out=None) -> "BounceResult":
        """rec.material.scatter(r_in, rec, rng, attenuation, scattered) (materials.nim:21-96) for the caller's hit records, bit for
        bit (tor_scatter_device / tor_scatter_host): the second half of bounce().  hits: a HitResult / BounceResult or its (n, 8)
        raw records -- the material of `object`, and p, normal, front_face as given (a host may have perturbed the normal); an
        object outside the scene counts as a miss.  rays, rng, index, out and the result as for bounce() (the result's hit
        fields are the caller's records); bounce() equals hit() followed by scatter()."""
        ops = _operands(self, "scatter", rays, "rays", 7, copy=True)
        n, rays = ops.n, ops.lead
        raw = ops.rows(hits.raw if hasattr(hits, "raw") else hits, "hits", 8)
        if raw is None:
            ops.bad("hits", "(n, 8) records")
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is not None and ops.holds(out.status):
            att, status = out.attenuation, out.status
        else:
            att, status = ops.new(n, 3), ops.new(n, dtype="int32")
        ops.call(ops.ptr(rays), ops.ptr(raw), ops.ptr(rng), p_list, n_list, ops.ptr(att), ops.ptr(status))
        return BounceResult(raw, ops.words(raw), "scatter", att, status, rays, rng, keep=ops.keep(index))

    def sky(self, rays, index=None, out=None):
        """The reference's sky (render.nim:41-44) without the attenuation for the listed rays (tor_sky_device): (n, 3) float64,
        (1 - t) * white + t * (0.5, 0.7, 1.0) with t = 0.5 * unit(direction).y + 1.0 (sic); rays that are not listed keep what
        `out` holds (a new array: 0).  CUDA tensors zero-copy on torch's current stream; numpy goes through the device and back."""
        as_numpy = not _is_tensor(rays)
        if as_numpy:
            rays = self._to_device(np.asarray(rays, dtype=np.float64).reshape(-1, 7))
            out = None if out is None else self._to_device(out, np.float64)
        ops = _Tensors(self, "sky", rays, "rays", 7)
        index, n_list, p_list = ops.index(index)
        if out is None:
            out = ops.new(ops.n, 3)
        elif not ops.fits(out, ops.n, 3):
            ops.bad("out", "a contiguous (n, 3) float64 tensor on the rays' device")
        ops.call(ops.ptr(ops.lead), p_list, n_list, ops.ptr(out))
        return out.cpu().numpy() if as_numpy else out

    def bounce_select(self, status, index=None):
        """The entries of `index` (None: every ray) whose status is BOUNCE_SCATTERED, in input order: the next step's list
        (tor_bounce_select_device, an ordered compaction on the device; blocking).  status: (n,) int32 CUDA tensor; returns an int32
        CUDA tensor."""
        import torch
        if not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.dim() != 1 or not status.is_cuda \
                or not status.is_contiguous():
            raise ValueError("Context.bounce_select: status must be a contiguous (n,) int32 CUDA tensor")
        n = int(status.shape[0])
        index, n_in, p_list = _tensor_list(index, n, status.device)
        lst = torch.empty((max(n_in, 1),), dtype=torch.int32, device=status.device)
        n_out = C.c_int64(0)
        _check(lib().tor_bounce_select_device(self._h, n, status.data_ptr(), p_list, n_in, lst.data_ptr(), C.byref(n_out),
                                              torch.cuda.current_stream(status.device).cuda_stream))
        return lst[:int(n_out.value)]

    def occluded(self, rays, t_range=None, index=None, time_range=None, mode="auto", out=None, mask=None) -> "OccludedResult":
        """Any-hit query for shadow rays (tor_occluded_device / tor_occluded_host): per listed ray ONE bit, whether
        world.hit(r, t_min, t_max, rec) of the reference returns true on the uploaded scene -- the reference's bit, exactly, at a
        fraction of hit()'s cost: the kernel stops at the first accepted root and writes 4 bytes per ray.

        rays: (n, 7) float64 -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or anything numpy takes
        (copied, blocking).  t_range: None ((0.001, +inf)) or (n, 2) {t_min, t_max} of the same kind; the segment p -> q is origin
        p, direction q - p, range (0.001, 1.0) (visible() builds these).  index: the rays to answer (int32, unique; entries outside
        [0, n) are skipped), None = all.  time_range and mode as for hit().  out: an OccludedResult of an earlier call on as many
        rays, or its raw int32 array, written again (rays that are not listed keep what it holds); otherwise a new one (0).
        Returns an OccludedResult: occluded (bool view), raw (int32) and mode.  Which object occludes is not defined; ask hit().
        mask: as for hit() (per-ray words are indexed by the ray): only the objects a ray sees can occlude it."""
        m = HIT_MODES[mode] if isinstance(mode, str) else int(mode)
        raw = out.raw if hasattr(out, "raw") else out
        ops = _operands(self, "occluded", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        t_range = ops.rows(t_range, "t_range", 2)
        index, n_list, p_list = ops.index(index)
        tr = ops.times(6, time_range)
        if raw is None:
            raw = ops.new(n, dtype="int32")
        elif not ops.fits(raw, n, dtype="int32"):
            ops.bad("out", "a contiguous (n,) int32 tensor or array, as the rays are")
        mk, masked = (None, None) if mask is None else ops.mask(mask)
        ops.call(ops.ptr(rays), ops.ptr(t_range), p_list, n_list, tr[0], tr[1], m, ops.ptr(raw), masked=masked)
        return OccludedResult(raw, ops.as_bool(raw), ops.note(n_list), keep=ops.keep(rays, t_range, index, mk))

    def crossings(self, rays, k, t_range=None, index=None, time_range=None, mode="auto", mask=None, records=False,
                  out=None) -> "CrossingsResult":
        """Ordered multi-hit query (tor_crossings_device / tor_crossings_host): per listed ray the first k surface crossings in
        (t_min, t_max), in order -- what transparent shadows, depth peeling, thickness / inside parity and picking through glass
        need, in one walk of the scene instead of k chained hit() calls.

        A crossing is (t, object, which): one for EACH root of the reference's sphere test (spheres.nim:29-48,
        moving_spheres.nim:39-66) with t_min < t < t_max, which = 0 for the near root (-half_b - sqrt(disc)) / a and 1 for the far
        one; ordered by t, then object, then which.  count (n,) is min(total, k); entries count .. k - 1 hold t = 0, object = -1,
        which = 0.  To learn whether MORE than k crossings exist, ask for k + 1.  Crossing 0 is hit()'s answer and count > 0 is
        occluded()'s bit, bit for bit.  1 <= k <= CROSSINGS_MAX.

        rays: (n, 7) float64 -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or anything numpy takes
        (copied, blocking).  t_range, index, time_range and mode as for occluded().  mask: as for hit() -- only the objects a ray
        sees are crossed, `object` stays the index in the full list; None is the unmasked query and reads no group state.
        records=True adds one TorHit per stored crossing (hits, (n, k, 8) raw records as hit() writes them; unused entries hold the
        miss record).  out: a CrossingsResult of an earlier call with the same n, k and records, written again (rays that are not
        listed keep what it holds); otherwise a new one (every entry unused, count 0).
        Returns a CrossingsResult: t (n, k), object, which, count (n,), raw, hits (None without records) and mode."""
        m = HIT_MODES[mode] if isinstance(mode, str) else int(mode)
        k = int(k)
        if not 1 <= k <= CROSSINGS_MAX:
            raise ValueError(f"Context.crossings: k must be in 1 .. {CROSSINGS_MAX}")
        if out is not None and not isinstance(out, CrossingsResult):
            raise ValueError("Context.crossings: out must be a CrossingsResult")
        ops = _operands(self, "crossings", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        t_range = ops.rows(t_range, "t_range", 2)
        index, n_list, p_list = ops.index(index)
        tr = ops.times(6, time_range)
        if out is None:
            raw, count = ops.new(n, k, 2, unused=2), ops.new(n, dtype="int32")
            hits = ops.new(n, k, 8, unused=14) if records else None
        else:
            raw, count, hits = out.raw, out.count, out.hits
            if not ops.fits(raw, n, k, 2) or not ops.fits(count, n, dtype="int32") or (hits is not None) != bool(records):
                ops.bad("out", "the result of a call with the same n, k and records, on tensors or arrays as the rays are")
        mk, (p_mask, word) = (None, (0, 0xFFFFFFFF)) if mask is None else ops.mask(mask)
        ops.call(ops.ptr(rays), ops.ptr(t_range), p_list, n_list, k, p_mask, word, tr[0], tr[1], m, ops.ptr(raw),
                 ops.ptr(count), ops.ptr(hits))
        return CrossingsResult(raw, ops.words(raw), count, hits, ops.note(n_list), keep=ops.keep(rays, t_range, index, mk))

    def nearest(self, points, k=1, max_distance=None, index=None, time_range=None, mode="auto", mask=None, out=None) -> "NearestResult":
        """Nearest-surface point query (tor_nearest_device / tor_nearest_host): per listed point the k objects whose surfaces lie
        nearest at the point's time, in order -- light culling around a shading point (visibility groups mark the emitters), a
        distance field for sphere tracing, proximity and contact tests.

        For point (p, time) and object j: d = length(p - centre_j(time)) - abs(radius_j) in float64, the reference's operations
        (vec3s.nim:23-27, moving_spheres.nim:39-44): the signed distance to the surface, negative inside.  Object j is a neighbour
        iff d is finite and d < max_distance (strict); neighbours are ordered by (d, object).  count (n,) is min(total, k); entries
        count .. k - 1 hold distance = 0, object = -1, inside = 0.  1 <= k <= NEAREST_MAX.

        points: (n, 4) float64 {x, y, z, time} -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or
        anything numpy takes (copied, blocking).  max_distance: None (+inf), a number, or one float64 per point of the points' kind.
        index, time_range and mode as for crossings() (time_range None: the finite min / max of the points' times).  mask: as for
        hit() -- only the objects a point sees are neighbours, `object` stays the index in the full list; None is the unmasked query
        and reads no group state.  out: a NearestResult of an earlier call with the same n and k, written again (points that are
        not listed keep what it holds); otherwise a new one (every entry unused, count 0).
        Returns a NearestResult: distance (n, k), object, inside, count (n,), raw and mode."""
        m = HIT_MODES[mode] if isinstance(mode, str) else int(mode)
        k = int(k)
        if not 1 <= k <= NEAREST_MAX:
            raise ValueError(f"Context.nearest: k must be in 1 .. {NEAREST_MAX}")
        if out is not None and not isinstance(out, NearestResult):
            raise ValueError("Context.nearest: out must be a NearestResult")
        ops = _operands(self, "nearest", points, "points", 4)
        n, points = ops.n, ops.lead
        max_distance = ops.rows(max_distance, "max_distance", or_number=True)
        index, n_list, p_list = ops.index(index)
        tr = ops.times(3, time_range)
        if out is None:
            raw, count = ops.new(n, k, 2, unused=2), ops.new(n, dtype="int32")
        else:
            raw, count = out.raw, out.count
            if not ops.fits(raw, n, k, 2) or not ops.fits(count, n, dtype="int32"):
                ops.bad("out", "the result of a call with the same n and k, on tensors or arrays as the points are")
        mk, (p_mask, word) = (None, (0, 0xFFFFFFFF)) if mask is None else ops.mask(mask)
        ops.call(ops.ptr(points), ops.ptr(max_distance), p_list, n_list, k, p_mask, word, tr[0], tr[1], m, ops.ptr(raw),
                 ops.ptr(count))
        return NearestResult(raw, ops.words(raw), count, ops.note(n_list), keep=ops.keep(points, max_distance, index, mk))

    def deposit(self, colors, pixels, sums, moments=None, counts=None, index=None, max_value=1.0, rejected=None) -> None:
        """Exact sample deposit (tor_deposit_device): adds the samples (colors[i], pixels[i]) to the film buffers in the progressive
        renders' arithmetic, so the sums do not depend on the order of the entries, the split into calls or the GPU, and
        resolve_device, accum_noise_device, adaptive_select_device and resolve_counts_device serve them.

        Per entry i (every entry, or the listed ones: index as for bounce(), entries outside [0, n) skipped, a repeated one deposits
        again): p = pixels[i]; outside [0, npix) nothing happens.  A colour with a NaN, infinite or negative channel is rejected as a
        whole (-0.0 passes) and counted in rejected.  Otherwise per channel q = quantize36(min(c, max_value)), sums[p] += q,
        moments[p] += quantize36(q * q), counts[p] += 1.  0 < max_value <= DEPOSIT_MAX_VALUE; exact while every pixel holds at most
        2^17 / max(max_value, max_value^2) accepted samples (the library cannot check that: Film.check_budget does).

        colors: (n, 3) float64, pixels: (n,) int32 -- torch CUDA tensors.  sums: float64, (..., 3), contiguous: npix = sums.numel() // 3
        pixels in that layout; moments (None or like sums), counts (None or int32 with npix elements), rejected (None or one int64)
        on the same device, contiguous, all ADDED to.  Asynchronous on torch's current stream."""
        import torch
        ops = _Tensors(self, "deposit", colors, "colors", 3)
        colors, n, dev = ops.lead, ops.n, ops.dev
        pixels = ops.rows(pixels, "pixels", dtype="int32")
        if pixels is None:
            ops.bad("pixels", "an (n,) int32 tensor on the colors' device")
        if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or sums.dim() < 1 or sums.shape[-1] != 3 \
                or sums.device != dev or not sums.is_contiguous():
            raise ValueError("Context.deposit: sums must be a contiguous (..., 3) float64 tensor on the colors' device")
        npix = int(sums.numel()) // 3
        if moments is not None and (not isinstance(moments, torch.Tensor) or moments.dtype != torch.float64
                                    or tuple(moments.shape) != tuple(sums.shape) or moments.device != dev or not moments.is_contiguous()):
            raise ValueError("Context.deposit: moments must be a contiguous float64 tensor of the sums' shape and device")
        if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or int(counts.numel()) != npix
                                   or counts.device != dev or not counts.is_contiguous()):
            raise ValueError("Context.deposit: counts must be a contiguous int32 tensor with one element per pixel on the sums' device")
        if rejected is not None and (not isinstance(rejected, torch.Tensor) or rejected.dtype != torch.int64 or int(rejected.numel()) != 1
                                     or rejected.device != dev):
            raise ValueError("Context.deposit: rejected must be one int64 on the sums' device")
        index, n_list, p_list = ops.index(index)
        ops.call(ops.ptr(colors), ops.ptr(pixels), p_list, n_list if index is not None else 0, float(max_value), npix,
                 ops.ptr(sums), ops.ptr(moments), ops.ptr(counts), ops.ptr(rejected))

    # ---- direct-light sampling (tor_light_sample_device, tor_light_pdf_device): the shadow rays of next-event estimation ----

    def sample_lights(self, points, rng, index=None, strategy="solid_angle", out=None) -> "LightSample":
        """One light sample per listed shading point (tor_light_sample_device / tor_light_sample_host): a light of the table
        (set_lights), a direction inside the cone its sphere subtends, the shadow segment and the density -- the definition,
        operation by operation in float64, is in include/tor_lights.h.

        points: (n, 4) float64 {x, y, z, time} -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or
        anything numpy takes (copied, blocking).  rng: (n, 4) 64-bit states as for bounce(): every listed point draws exactly
        three uniform01 from its state, sampled or not; a contiguous CUDA tensor is updated in place.  index as for bounce().
        strategy: "solid_angle" (importance weight * the solid-angle measure of the light seen from the point) or "weight".
        Returns a LightSample: rays (n, 7) {origin p, direction to the sampled surface point, time} -- parameter 1.0 is the
        surface point, so the rays go into occluded() with range (t_min, 1.0) and a mask that leaves the lamps out, or with a
        range that stops short --, pdf (n,) per unit solid angle at p with the selection probability included, light (n,) int32
        the picked light's OBJECT index (-1: none, then pdf = 0 and ray = 0), dist (n,), rng and mode.  out: a LightSample of an
        earlier call on as many points, written again (points that are not listed keep what it holds); otherwise a new one
        (light -1, the rest 0)."""
        strat = LIGHT_STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)
        if out is not None and not isinstance(out, LightSample):
            raise ValueError("Context.sample_lights: out must be a LightSample")
        ops = _operands(self, "light_sample", points, "points", 4)
        n, points = ops.n, ops.lead
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is None:
            rays, pdf, dist = ops.new(n, 7), ops.new(n), ops.new(n)
            light = ops.new(n, dtype="int32", zero=False)
            light[...] = -1
        else:
            rays, pdf, light, dist = out.rays, out.pdf, out.light, out.dist
            if not ops.fits(rays, n, 7) or not ops.fits(pdf, n) or not ops.fits(light, n, dtype="int32") or not ops.fits(dist, n):
                ops.bad("out", "the result of a call on as many points, on tensors or arrays as the points are")
        ops.call(ops.ptr(points), ops.ptr(rng), p_list, n_list, strat, ops.ptr(rays), ops.ptr(pdf), ops.ptr(light), ops.ptr(dist))
        return LightSample(rays, pdf, light, dist, rng, ops.note(n_list), keep=ops.keep(points, index))

    def light_pdf(self, points, objects, index=None, strategy="solid_angle"):
        """The density sample_lights gives the direction from each listed point towards the light whose object index is
        objects[i] (tor_light_pdf_device / tor_light_pdf_host): (n,) float64, 0 where the object is no light of the table or can
        not be picked (and for points that are not listed).  Same arithmetic and same sequential total as the sampler, nothing
        drawn: light_pdf(points, sample.light) equals sample.pdf in every bit.  points, index, strategy as for sample_lights;
        objects: (n,) int32 of the points' kind -- the object a ray from that point is taken to have reached."""
        strat = LIGHT_STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)
        ops = _operands(self, "light_pdf", points, "points", 4)
        n, points = ops.n, ops.lead
        objects = ops.rows(objects, "objects", dtype="int32")
        if objects is None:
            ops.bad("objects", "an (n,) int32 tensor or array, as the points are")
        index, n_list, p_list = ops.index(index)
        pdf = ops.new(n)
        ops.call(ops.ptr(points), ops.ptr(objects), p_list, n_list, strat, ops.ptr(pdf))
        self._light_keep = ops.keep(points, objects, index)   # (alive while the query may still run)
        return pdf

    def bsdf(self, rays_in, hits, rays_out, index=None, out=None) -> "BsdfEval":
        """Value and density of the reference's scatter (tor_bsdf_eval_device / tor_bsdf_eval_host): per listed item the
        solid-angle density rec.material.scatter gives the direction of rays_out[i] for the incoming direction of rays_in[i] at
        the record hits[i], and value = albedo * pdf (f_r cos) -- the definition, operation by operation in float64, is in
        include/tor_bsdf.h.  Lambertian: cos / pi; Metal with fuzz != 0: the closed-form density of reflect + fuzz * ball, gated
        by the scatter's own dot(out, n) > 0; both kind BSDF_DENSITY.  Dielectric and Metal with fuzz == 0: BSDF_DELTA, an
        object outside the scene: BSDF_NONE, both with value and pdf 0.

        rays_in (n, 7) float64: a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or anything numpy takes
        (blocking); only the direction is read.  hits: a HitResult / BounceResult or its (n, 8) raw records, as for scatter();
        normal and object are read as given.  rays_out (n, 7): any positive finite length -- the rays of sample_lights,
        sample_environment and scatter / bounce go straight in.  index as for bounce().  Nothing is drawn.  Returns a BsdfEval;
        out: one of an earlier call on as many items, written again (items that are not listed keep what it holds); otherwise a
        new one (all 0)."""
        if out is not None and not isinstance(out, BsdfEval):
            raise ValueError("Context.bsdf: out must be a BsdfEval")
        ops = _operands(self, "bsdf_eval", rays_in, "rays_in", 7)
        n, rays_in = ops.n, ops.lead
        raw = ops.rows(hits.raw if hasattr(hits, "raw") else hits, "hits", 8)
        rays_out = ops.rows(rays_out, "rays_out", 7)
        if raw is None or rays_out is None:
            ops.bad("hits and rays_out", "(n, 8) records and (n, 7) rays, as rays_in is")
        index, n_list, p_list = ops.index(index)
        if out is None:
            value, pdf, kind = ops.new(n, 3), ops.new(n), ops.new(n, dtype="int32")
        else:
            value, pdf, kind = out.value, out.pdf, out.kind
            if not ops.fits(value, n, 3) or not ops.fits(pdf, n) or not ops.fits(kind, n, dtype="int32"):
                ops.bad("out", "the result of a call on as many items, on tensors or arrays as rays_in is")
        ops.call(ops.ptr(rays_in), ops.ptr(raw), ops.ptr(rays_out), p_list, n_list, ops.ptr(value), ops.ptr(pdf), ops.ptr(kind))
        return BsdfEval(value, pdf, kind, ops.note(n_list), keep=ops.keep(rays_in, raw, rays_out, index))

    # ---- light-tracing queries (tor_light_emit_device, tor_camera_connect_device): emit from the lights, connect to the camera ----

    def connect_camera(self, cam: Camera, nrows: int, ncols: int, points, rng, index=None, out=None) -> "CameraConnection":
        """For each listed world point the pixel it lands in, the lens point it is seen through and the measurement weight
        (tor_camera_connect_device / tor_camera_connect_host) -- the inverse of camera_rays; the definition, operation by
        operation in float64, is in include/tor_camera.h.  It reads no scene.

        points: (n, 4) float64 {x, y, z, time} -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or
        anything numpy takes (copied, blocking).  rng: (n, 4) 64-bit states as for bounce(): every listed point draws exactly two
        uniform01 (the lens point), pinhole or not, connected or not; a contiguous CUDA tensor is updated in place.  index as for
        bounce().  Returns a CameraConnection: rays (n, 7) {origin the point, direction to the lens point, time} -- parameter
        1.0 is the lens point, so the rays go into occluded() with range (t_min, 1.0) --, pixel (n,) int32 row * ncols + col
        (row 0 = bottom; -1: behind the lens plane, outside the frame or not finite, then factor = 0 and ray = 0), factor (n,):
        a vertex with throughput beta, BSDF value f and cosine cos_y towards the lens point adds beta * f * cos_y * factor to
        the pixel's radiance estimate when the segment is free, lens (n, 2) the lens point in the camera's (u, v), rng and mode.
        out: a CameraConnection of an earlier call on as many points, written again (points that are not listed keep what it
        holds); otherwise a new one (pixel -1, the rest 0)."""
        if out is not None and not isinstance(out, CameraConnection):
            raise ValueError("Context.connect_camera: out must be a CameraConnection")
        ops = _operands(self, "camera_connect", points, "points", 4)
        n, points = ops.n, ops.lead
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is None:
            rays, factor, lens = ops.new(n, 7), ops.new(n), ops.new(n, 2)
            pixel = ops.new(n, dtype="int32", zero=False)
            pixel[...] = -1
        else:
            rays, pixel, factor, lens = out.rays, out.pixel, out.factor, out.lens
            if not ops.fits(rays, n, 7) or not ops.fits(pixel, n, dtype="int32") or not ops.fits(factor, n) or not ops.fits(lens, n, 2):
                ops.bad("out", "the result of a call on as many points, on tensors or arrays as the points are")
        _check(getattr(lib(), "tor_camera_connect" + ops.suffix)(
            ops.h, C.byref(cam), int(nrows), int(ncols), n, ops.ptr(points), ops.ptr(rng), p_list, n_list, ops.ptr(rays), ops.ptr(pixel),
            ops.ptr(factor), ops.ptr(lens), *ops.tail))
        return CameraConnection(rays, pixel, factor, lens, rng, ops.note(n_list), keep=ops.keep(points, index))

    def emit_lights(self, rng, time_range=(0.0, 0.0), index=None, out=None) -> "LightEmission":
        """One path start per listed state on the lamps of the light table (tor_light_emit_device / tor_light_emit_host;
        include/tor_camera.h): a time in time_range, a light by its weight, a uniform point of its sphere and a cosine-weighted
        direction about the normal there.

        rng: (n, 4) 64-bit states -- a torch CUDA tensor (int64 holding the u64 bits; zero-copy, asynchronous on torch's current
        stream, a contiguous one is updated in place) or anything numpy takes (copied, blocking): every listed path draws
        exactly six.  time_range: (lo, hi), finite, lo <= hi -- the camera's shutter interval.  index as for bounce().  Returns
        a LightEmission: rays (n, 7) {origin on the lamp, unit direction, time}, normal (n, 3), light (n,) int32 the OBJECT
        index, pdf_area (n,) per unit area with the pick included (+inf for a lamp of radius 0), pdf_dir (n,) = cos / pi per
        unit solid angle, rng and mode.  A lamp of uniform radiance Le starts its path with beta = Le * pi / pdf_area.  out: a
        LightEmission of an earlier call on as many states, written again; otherwise a new one (light -1, the rest 0)."""
        if out is not None and not isinstance(out, LightEmission):
            raise ValueError("Context.emit_lights: out must be a LightEmission")
        if _is_tensor(rng):
            import torch
            if rng.dtype not in (torch.int64, torch.uint64) or rng.dim() != 2 or rng.shape[1] != 4 or not rng.is_cuda:
                raise ValueError("Context.emit_lights: rng must be an (n, 4) int64 CUDA tensor")
            rng = rng.contiguous()
            words = rng.view(torch.float64)
        else:
            rng = np.asarray(rng)
            if rng.ndim != 2 or rng.shape[1] != 4 or rng.dtype.kind not in "iu" or rng.dtype.itemsize != 8:
                raise ValueError("Context.emit_lights: rng must be an (n, 4) array of 64-bit integers")
            words = np.ascontiguousarray(rng).view(np.float64)
        ops = _operands(self, "light_emit", words, "rng", 4)   # (the leading operand of the one operand layer: the states' words)
        n = ops.n
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is None:
            rays, normal, pdf = ops.new(n, 7), ops.new(n, 3), ops.new(n, 2)
            light = ops.new(n, dtype="int32", zero=False)
            light[...] = -1
        else:
            rays, normal, light, pdf = out.rays, out.normal, out.light, out.pdf
            if not ops.fits(rays, n, 7) or not ops.fits(normal, n, 3) or not ops.fits(light, n, dtype="int32") or not ops.fits(pdf, n, 2):
                ops.bad("out", "the result of a call on as many states, on tensors or arrays as the states are")
        ops.call(ops.ptr(rng), p_list, n_list, float(time_range[0]), float(time_range[1]), ops.ptr(rays), ops.ptr(normal),
                 ops.ptr(light), ops.ptr(pdf))
        return LightEmission(rays, normal, light, pdf, rng, ops.note(n_list), keep=ops.keep(index))

    # ---- photon-map queries (tor_photons_build_device, tor_photons_gather_device): density estimation in world space ----

    def build_photons(self, positions, powers, directions=None, radius=None, index=None) -> "PhotonMap":
        """Build the context's photon map (tor_photons_build_device / tor_photons_build_host; include/tor_photons.h): the listed
        photons {position, power, incoming direction} are copied into a hashed uniform grid of cell size radius * (1 + 2^-20)
        that the context owns; it replaces the previous map and survives upload(), set_lights() and set_environment().  A photon
        with a non-finite position or direction, a NaN, infinite or negative power channel (-0.0 passes) or a cell beyond
        +-2^30 is dropped and counted.  No scene is needed.

        positions, powers (n, 3) float64, directions (n, 3) or None -- torch CUDA tensors (zero-copy, asynchronous on torch's
        current stream; the arrays may go once the stream has passed the call) or anything numpy takes (blocking).  radius: the
        map's gather radius R, finite and > 0.  index: as for deposit() -- None every photon, entries outside [0, n) skipped, a
        repeated entry stored again.

        The powers are stored times a power of two chosen so that the largest finite channel lies in (1/2, 1] -- exact, short
        of underflow for channels 2^-1000 below the largest -- which puts them in the range the gather's max_value clamp and
        2^-36 quantum are made for; PhotonGather.irradiance divides it out again.  (Finding the largest channel of a tensor
        waits for it.)  Returns a PhotonMap: scale, radius, note and info(), which reads the counts back when it is asked."""
        if radius is None:
            raise ValueError("Context.build_photons: radius is required")
        ops = _operands(self, "photons_build", positions, "positions", 3)
        n, positions, xp = ops.n, ops.lead, ops.xp
        powers = ops.rows(powers, "powers", 3)
        if powers is None:
            ops.bad("powers", "an (n, 3) float64 array of the positions' kind")
        directions = ops.rows(directions, "directions", 3)
        index, n_list, p_list = ops.index(index)
        top = float(xp.where(xp.isfinite(powers), powers, xp.zeros_like(powers)).max()) if n else 0.0
        scale = 1.0
        if top > 0.0:
            mant, e = math.frexp(top)   # top = mant * 2^e, mant in [1/2, 1)
            scale = math.ldexp(1.0, -max(min(e - 1 if mant == 0.5 else e, 1000), -1000))
        scaled = powers * scale
        ops.call(ops.ptr(positions), ops.ptr(scaled), ops.ptr(directions), p_list, n_list, float(radius))
        self._photon_scale, self._photon_radius = scale, float(radius)
        self._photon_keep = ops.keep(positions, scaled, directions, index)   # (alive while the build may still run)
        return PhotonMap(self, scale, float(radius), last_note())

    def photons_info(self) -> dict:
        """tor_photons_info: {stored, dropped, n_buckets, largest_bucket} of the context's photon map.  Blocking."""
        out = (C.c_int64 * 4)()
        _check(lib().tor_photons_info(self._h, out))
        return {"stored": int(out[0]), "dropped": int(out[1]), "n_buckets": int(out[2]), "largest_bucket": int(out[3])}

    def gather_photons(self, points, normals=None, radius=None, index=None, kernel="epanechnikov", max_value=1.0, out=None) -> "PhotonGather":
        """Gather the photon map around points (tor_photons_gather_device / tor_photons_gather_host; include/tor_photons.h): per
        listed point x, over the stored photons j with d2 = |p_j - x|^2 < r^2 and, with normals, dir_j . n < 0 (strict, NaN
        fails), sums += quantize36(min(power_j * w, max_value)) per channel and count += 1, w = 1 (kernel "constant") or
        1 - d2 / r^2 ("epanechnikov").  The answer is the brute-force sum over every stored photon, bit for bit, while
        count * max_value < 2^17 (PhotonGather.check_budget); the grid only makes it fast.

        points (n, 3) float64, normals (n, 3) or None -- torch CUDA tensors (zero-copy, asynchronous on torch's current stream)
        or anything numpy takes (blocking).  radius: None (the map's R), a number or one float64 per point; min(radius, R) is
        used, a negative or NaN radius accepts nothing.  index as for bounce().  0 < max_value <= DEPOSIT_MAX_VALUE, in units of
        the scaled powers (build_photons).  out: a PhotonGather of an earlier call on as many points, written again (points
        that are not listed keep what it holds); otherwise a new one (zeros).  Returns a PhotonGather: sums (n, 3), count (n,)
        int32, and irradiance(paths) / check_budget()."""
        k = PHOTON_KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
        if out is not None and not isinstance(out, PhotonGather):
            raise ValueError("Context.gather_photons: out must be a PhotonGather")
        ops = _operands(self, "photons_gather", points, "points", 3)
        n, points, xp = ops.n, ops.lead, ops.xp
        normals = ops.rows(normals, "normals", 3)
        rad = ops.rows(radius, "radius", or_number=True)
        index, n_list, p_list = ops.index(index)
        if out is None:
            sums, count = ops.new(n, 3), ops.new(n, dtype="int32")
        else:
            sums, count = out.sums, out.count
            if not ops.fits(sums, n, 3) or not ops.fits(count, n, dtype="int32"):
                ops.bad("out", "the result of a call on as many points, on tensors or arrays as the points are")
        ops.call(ops.ptr(points), ops.ptr(normals), ops.ptr(rad), p_list, n_list, k, float(max_value), ops.ptr(sums), ops.ptr(count))
        big = getattr(self, "_photon_radius", None)
        used = big if rad is None else xp.where(rad < big, rad, xp.full_like(rad, big))   # min(radius, R) as the library takes it
        return PhotonGather(sums, count, getattr(self, "_photon_scale", 1.0), used, k, float(max_value), ops.note(n_list),
                            keep=ops.keep(points, normals, rad, index))

    # ---- environment-light queries (tor_env_eval_device, tor_env_sample_device): the sky as an emitter ----

    def environment(self, rays, index=None, out=None, pdf=False):
        """The environment map's colour in the direction of every listed ray (tor_env_eval_device / tor_env_eval_host): (n, 3)
        float64, the RGB of the texel the direction encodes into -- the definition, operation by operation, is in
        include/tor_env.h.  The direction need not be unit; one that is zero, NaN or infinite gives colour 0, pdf 0, texel -1.

        rays: (n, 7) float64 -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream, no host
        synchronisation) or anything numpy takes (copied, blocking).  index as for bounce().  out: an (n, 3) array of the rays'
        kind (or an EnvEval of an earlier call with pdf=True), written again -- rays that are not listed keep what it holds;
        otherwise new (colour and pdf 0, texel -1).  pdf=True: an EnvEval with color, pdf (n,) the solid-angle density
        sample_environment gives that direction (what multiple importance sampling needs) and texel (n,) int32
        row * n + col."""
        ops = _operands(self, "env_eval", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        index, n_list, p_list = ops.index(index)
        dens = texel = None
        if isinstance(out, EnvEval):
            color, dens, texel = out.color, out.pdf, out.texel
        else:
            color = out
        if color is None:
            color = ops.new(n, 3)
        elif not ops.fits(color, n, 3):
            ops.bad("out", "a contiguous (n, 3) float64 tensor or array, as the rays are")
        if pdf:
            if dens is None:
                dens = ops.new(n)
                texel = ops.new(n, dtype="int32", zero=False)
                texel[...] = -1
            elif not ops.fits(dens, n) or not ops.fits(texel, n, dtype="int32"):
                ops.bad("out", "the result of a call with pdf=True on as many rays")
        else:
            dens = texel = None
        ops.call(ops.ptr(rays), p_list, n_list, ops.ptr(color), ops.ptr(dens), ops.ptr(texel))
        self._env_keep = ops.keep(rays, index)   # (alive while the query may still run)
        return EnvEval(color, dens, texel, ops.note(n_list)) if pdf else color

    def sample_environment(self, points, rng, index=None, out=None) -> "EnvSample":
        """One direction per listed shading point, drawn in proportion to the environment map's importance
        (tor_env_sample_device / tor_env_sample_host; include/tor_env.h): a texel by its importance, a uniform position inside
        it, the octahedral decode.

        points: (n, 4) float64 {x, y, z, time} -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or
        anything numpy takes (copied, blocking).  rng: (n, 4) 64-bit states as for bounce(): every listed point draws exactly
        four uniform01; a contiguous CUDA tensor is updated in place.  index as for bounce().  Returns an EnvSample: rays
        (n, 7) {origin p, unit direction, time} -- they go into occluded() with the default range (0.001, +inf) --, pdf (n,)
        per unit solid angle, texel (n,) int32 row * n + col, color (n, 3) the texel's RGB, rng and mode.  out: an EnvSample of
        an earlier call on as many points, written again (points that are not listed keep what it holds); otherwise a new one
        (texel -1, the rest 0)."""
        if out is not None and not isinstance(out, EnvSample):
            raise ValueError("Context.sample_environment: out must be an EnvSample")
        ops = _operands(self, "env_sample", points, "points", 4)
        n, points = ops.n, ops.lead
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is None:
            rays, pdf, color = ops.new(n, 7), ops.new(n), ops.new(n, 3)
            texel = ops.new(n, dtype="int32", zero=False)
            texel[...] = -1
        else:
            rays, pdf, texel, color = out.rays, out.pdf, out.texel, out.color
            if not ops.fits(rays, n, 7) or not ops.fits(pdf, n) or not ops.fits(texel, n, dtype="int32") or not ops.fits(color, n, 3):
                ops.bad("out", "the result of a call on as many points, on tensors or arrays as the points are")
        ops.call(ops.ptr(points), ops.ptr(rng), p_list, n_list, ops.ptr(rays), ops.ptr(pdf), ops.ptr(texel), ops.ptr(color))
        return EnvSample(rays, pdf, texel, color, rng, ops.note(n_list), keep=ops.keep(points, index))

    # ---- participating media (tor_scene_media, tor_media_march_device, tor_media_scatter_device, tor_rng_uniform_device) ----

    def set_media(self, objects, sigma, albedo=None):
        """The media table of the uploaded scene (tor_scene_media): `objects` are the indices of the boundary spheres in the
        uploaded list (unique, at most MEDIA_MAX) -- ordinary scene objects, which a host hides from the surface queries with
        visibility groups --, `sigma` one extinction per unit length per medium (finite, >= 0), `albedo` None (1, 1, 1) or
        (n, 3), finite and >= 0.  march_media / scatter_media / transmittance / trace_media read it.  An empty `objects` clears
        the table, and so does every upload that replaces the scene."""
        o = np.ascontiguousarray(np.asarray(objects).reshape(-1), dtype=np.int32)
        s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(-1))
        if s.size != o.size:
            raise ValueError("Context.set_media: one sigma per medium")
        p_albedo = 0
        if albedo is not None:
            a = np.ascontiguousarray(np.asarray(albedo, dtype=np.float64).reshape(-1, 3))
            if a.shape[0] != o.size:
                raise ValueError("Context.set_media: albedo must be (n, 3), one colour per medium")
            p_albedo = a.ctypes.data or 16
        _check(lib().tor_scene_media(self._h, int(o.size), C.c_void_p(o.ctypes.data or 16), C.c_void_p(s.ctypes.data or 16),
                                     C.c_void_p(p_albedo)))
        self._n_media = int(o.size)   # (what set_media_phase(None) passes as the table's count)
        self._grid_media = set()      # (a new table has no density grids: media_grids() need not ask)

    def march_media(self, rays, tau, t_range=None, index=None, out=None) -> "MediaMarch":
        """The optical-depth march (tor_media_march_device / tor_media_march_host): per listed ray, where along it the accumulated
        sigma * length through the media of the table (set_media) reaches the budget `tau` -- a collision --, or, if it never
        does, how much depth the range holds.  The definition, operation by operation in float64, is in include/tor_media.h;
        overlapping media add their densities in table order.

        rays: (n, 7) float64 -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or anything numpy takes
        (copied, blocking).  tau: a number or (n,) float64 of the rays' kind; the library takes no logarithm: free-flight sampling
        passes -log1p(-u) of a uniform (Context.uniform), and tau = inf asks for the depth of the whole range, whose
        transmittance is exp(-depth).  t_range: None -- (0.0, +inf), NOT the (0.001, +inf) of the surface queries: a scattered
        ray starts inside the medium -- or (n, 2).  index as for bounce().  Returns a MediaMarch: status (n,) int32
        (MEDIA_COLLIDED: t is the collision, depth = tau, active the bit set of the media there, rho their summed sigma;
        MEDIA_ESCAPED: t = t_max, depth what was accumulated; MEDIA_REFUSED: tau not >= 0 or an empty range), t, depth, rho (n,)
        float64 and active (n,) int64 holding the 64 bits.  out: a MediaMarch of an earlier call on as many rays, written again
        (rays that are not listed keep what it holds); otherwise a new one (0)."""
        if out is not None and not isinstance(out, MediaMarch):
            raise ValueError("Context.march_media: out must be a MediaMarch")
        ops = _operands(self, "media_march", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        tau = ops.rows(tau, "tau", or_number=True)
        if tau is None:
            ops.bad("tau", "a number or an (n,) float64 tensor or array, as the rays are")
        t_range = ops.rows(t_range, "t_range", 2)
        index, n_list, p_list = ops.index(index)
        if out is None:
            status, t, depth, active, rho = ops.new(n, dtype="int32"), ops.new(n), ops.new(n), ops.new(n, dtype="int64"), ops.new(n)
        else:
            status, t, depth, active, rho = out.status, out.t, out.depth, out.active, out.rho
            if not ops.fits(status, n, dtype="int32") or not ops.fits(t, n) or not ops.fits(depth, n) \
                    or not ops.fits(active, n, dtype="int64") or not ops.fits(rho, n):
                ops.bad("out", "the result of a call on as many rays, on tensors or arrays as the rays are")
        ops.call(ops.ptr(rays), ops.ptr(t_range), ops.ptr(tau), p_list, n_list, ops.ptr(status), ops.ptr(t), ops.ptr(depth),
                 ops.ptr(active), ops.ptr(rho))
        return MediaMarch(status, t, depth, active, rho, ops.note(n_list), keep=ops.keep(rays, t_range, tau, index))

    def scatter_media(self, rays, march, rng, index=None, out=None) -> "MediaScatter":
        """The isotropic scatter at a collision (tor_media_scatter_device / tor_media_scatter_host): per listed ray the new ray
        {origin + t * direction, random_unit_vector(rng) (sampling.nim:51-55), time} and the albedo of the mixture there, sum of
        sigma * albedo over the active media divided by the sum of sigma, in table order.

        rays as for march_media; march: its MediaMarch, or a pair (t, active); rng: (n, 4) 64-bit states as for bounce() -- every
        listed ray draws exactly two outputs, sampled or not; a contiguous CUDA tensor is updated in place.  index as for
        bounce(): list the rays whose status is MEDIA_COLLIDED (an entry with no active medium gets attenuation 0 and a zero
        ray).  Returns a MediaScatter, which unpacks as (rays, attenuation) -- (n, 7) and (n, 3) -- and carries rng and mode.
        out: a MediaScatter (or a pair) of an earlier call on as many rays, written again; `rays` itself may be passed as out[0]."""
        ops = _operands(self, "media_scatter", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        t, active = (march.t, march.active) if isinstance(march, MediaMarch) else march
        t, active = ops.rows(t, "march.t"), ops.rows(active, "march.active", dtype="int64")
        if t is None or active is None:
            ops.bad("march", "a MediaMarch or a pair (t, active)")
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is None:
            rays_out, att = ops.new(n, 7), ops.new(n, 3)
        else:
            rays_out, att = out
            if not ops.fits(rays_out, n, 7) or not ops.fits(att, n, 3):
                ops.bad("out", "a pair of contiguous (n, 7) and (n, 3) float64 tensors or arrays, as the rays are")
        ops.call(ops.ptr(rays), ops.ptr(t), ops.ptr(active), ops.ptr(rng), p_list, n_list, ops.ptr(rays_out), ops.ptr(att))
        return MediaScatter(rays_out, att, rng, ops.note(n_list), keep=ops.keep(rays, t, active, index))

    # ---- phase functions (tor_scene_media_phase, tor_phase_sample_device, tor_phase_eval_device) ----

    def set_media_phase(self, g=None):
        """The Henyey-Greenstein asymmetry of every medium of the table (tor_scene_media_phase): `g` one value per medium, each 0
        (isotropic; what set_media leaves) or PHASE_G_MIN <= |g| <= PHASE_G_MAX; None: every medium 0.  sample_phase / phase /
        trace_media(phase=True) / trace_media_direct read it.  set_media resets it; a replacing upload clears the table."""
        if g is None:   # (the count set_media gave the table: the library refuses another)
            _check(lib().tor_scene_media_phase(self._h, int(getattr(self, "_n_media", 0)), None))
            return
        a = np.ascontiguousarray(np.asarray(g, dtype=np.float64).reshape(-1))
        _check(lib().tor_scene_media_phase(self._h, int(a.size), C.c_void_p(a.ctypes.data or 16)))

    def sample_phase(self, rays, march, rng, index=None, out=None) -> "PhaseSample":
        """The Henyey-Greenstein scatter at a collision (tor_phase_sample_device / tor_phase_sample_host): per listed ray one of
        the active media is chosen in proportion to sigma, the cosine to the incoming direction is drawn by inverting its
        phase function, the azimuth is uniform, and attenuation and pdf are those of the MIXTURE of the active media at that
        cosine -- the definition, operation by operation in float64, is in include/tor_phase.h.

        The operands of scatter_media: rays (n, 7); march: a MediaMarch or a pair (t, active); rng: (n, 4) 64-bit states --
        every listed ray draws exactly three outputs, sampled or not; a contiguous CUDA tensor is updated in place.  index as
        for bounce().  Returns a PhaseSample, which unpacks as (rays, attenuation) like a MediaScatter and carries pdf (n,), rng
        and mode.  out: a PhaseSample of an earlier call on as many rays, written again; `rays` itself may be passed as its
        rays."""
        if out is not None and not isinstance(out, PhaseSample):
            raise ValueError("Context.sample_phase: out must be a PhaseSample")
        ops = _operands(self, "phase_sample", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        t, active = (march.t, march.active) if isinstance(march, MediaMarch) else march
        t, active = ops.rows(t, "march.t"), ops.rows(active, "march.active", dtype="int64")
        if t is None or active is None:
            ops.bad("march", "a MediaMarch or a pair (t, active)")
        rng = ops.states(rng)
        index, n_list, p_list = ops.index(index)
        if out is None:
            rays_out, att, pdf = ops.new(n, 7), ops.new(n, 3), ops.new(n)
        else:
            rays_out, att, pdf = out.rays, out.attenuation, out.pdf
            if not ops.fits(rays_out, n, 7) or not ops.fits(att, n, 3) or not ops.fits(pdf, n):
                ops.bad("out", "the result of a call on as many rays, on tensors or arrays as the rays are")
        ops.call(ops.ptr(rays), ops.ptr(t), ops.ptr(active), ops.ptr(rng), p_list, n_list, ops.ptr(rays_out), ops.ptr(att),
                 ops.ptr(pdf))
        return PhaseSample(rays_out, att, pdf, rng, ops.note(n_list), keep=ops.keep(rays, t, active, index))

    def phase(self, rays_in, march_or_active, rays_out, index=None, out=None) -> "PhaseEval":
        """Value and density of the media's phase function (tor_phase_eval_device / tor_phase_eval_host), the twin of bsdf(): per
        listed item the solid-angle density with which sample_phase draws the direction of rays_out[i] for a path that was
        travelling along rays_in[i] through the media of the active word, and value = the single-scattering albedo of the
        mixture times that phase function, per channel.  Nothing is drawn.

        rays_in, rays_out (n, 7) float64, any positive finite length (the rays of sample_lights go straight in); only the
        directions are read.  march_or_active: a MediaMarch, or (n,) int64 active words.  index as for bounce().  Returns a
        PhaseEval(value (n, 3), pdf (n,), mode); out: one of an earlier call on as many items, written again."""
        if out is not None and not isinstance(out, PhaseEval):
            raise ValueError("Context.phase: out must be a PhaseEval")
        ops = _operands(self, "phase_eval", rays_in, "rays_in", 7)
        n, rays_in = ops.n, ops.lead
        active = ops.rows(march_or_active.active if isinstance(march_or_active, MediaMarch) else march_or_active, "active", dtype="int64")
        rays_out = ops.rows(rays_out, "rays_out", 7)
        if active is None or rays_out is None:
            ops.bad("active and rays_out", "(n,) int64 words and (n, 7) rays, as rays_in is")
        index, n_list, p_list = ops.index(index)
        if out is None:
            value, pdf = ops.new(n, 3), ops.new(n)
        else:
            value, pdf = out.value, out.pdf
            if not ops.fits(value, n, 3) or not ops.fits(pdf, n):
                ops.bad("out", "the result of a call on as many items, on tensors or arrays as rays_in is")
        ops.call(ops.ptr(rays_in), ops.ptr(active), ops.ptr(rays_out), p_list, n_list, ops.ptr(value), ops.ptr(pdf))
        return PhaseEval(value, pdf, ops.note(n_list), keep=ops.keep(rays_in, active, rays_out, index))

    def uniform(self, rng, n=1, index=None, out=None):
        """Plain uniforms from a path's stream (tor_rng_uniform_device / tor_rng_uniform_host): u[i, k] = uniform01(rng[i])
        (support/rng.nim:129-133) for k = 0 .. n - 1, for every listed state -- what free-flight sampling and Russian roulette
        draw, without running a sampler that consumes the uniform for a purpose of its own.  It needs no scene.

        rng: (m, 4) 64-bit states -- a CUDA int64 tensor (a contiguous one is advanced in place, asynchronous on torch's current
        stream) or an array of 64-bit integers (copied, blocking).  1 <= n <= UNIFORM_MAX_DRAWS.  index as for bounce().  out: an
        (m, n) float64 buffer of the states' kind, written again (states that are not listed keep what it holds); otherwise a
        new one (0).  Returns a Uniforms, which unpacks as (u, rng): the uniforms and the advanced states."""
        n = int(n)
        if not 1 <= n <= UNIFORM_MAX_DRAWS:
            raise ValueError(f"Context.uniform: n must be in 1 .. {UNIFORM_MAX_DRAWS}")
        if _is_tensor(rng):
            import torch
            if rng.dtype not in (torch.int64, torch.uint64) or rng.dim() != 2 or rng.shape[1] != 4 or not rng.is_cuda:
                raise ValueError("Context.uniform: rng must be an (m, 4) int64 CUDA tensor")
            st = rng.contiguous()
            ops = _Tensors(self, "rng_uniform", st.view(torch.float64), "rng", 4)
        else:
            st = np.asarray(rng)
            if st.ndim != 2 or st.shape[1] != 4 or st.dtype.kind not in "iu" or st.dtype.itemsize != 8:
                raise ValueError("Context.uniform: rng must be an (m, 4) array of 64-bit integers")
            st = np.ascontiguousarray(st).view(np.uint64).copy()
            ops = _Arrays(self, "rng_uniform", st.view(np.float64), "rng", 4)
        index, n_list, p_list = ops.index(index)
        if out is None:
            out = ops.new(ops.n, n)
        elif not ops.fits(out, ops.n, n):
            ops.bad("out", "a contiguous (m, n) float64 tensor or array, as the states are")
        ops.call(ops.ptr(ops.lead), p_list, n_list, n, ops.ptr(out))
        return Uniforms(out, st, ops.note(n_list), keep=ops.keep(index))

    # ---- heterogeneous media (tor_scene_media_grid, tor_media_grid_march_device, tor_media_grid_density_device) ----

    def set_media_grid(self, medium, density, box=None):
        """The density grid of medium `medium` of the table (tor_scene_media_grid, include/tor_grid.h): `density` an (nx, ny, nz)
        array, finite and >= 0 -- the local extinction is the medium's sigma times the cell's value inside both the boundary
        sphere and the box, 0 elsewhere --; `box` None (the sphere's bounding cube) or (lo xyz, hi xyz), six numbers, OFFSETS
        from the sphere's centre, so the grid rides a moving boundary.  density=None removes the medium's grid.  A medium with a
        grid takes no part in march_media: march_media_grid marches it, one medium per call.  set_media drops every grid, and so
        does an upload that replaces the scene."""
        if density is None:
            _check(lib().tor_scene_media_grid(self._h, int(medium), 0, 0, 0, None, None))
            getattr(self, "_grid_media", set()).discard(int(medium))
            return
        d = np.ascontiguousarray(np.asarray(density, dtype=np.float64))
        if d.ndim != 3 or d.size == 0:
            raise ValueError("Context.set_media_grid: density must be an (nx, ny, nz) array with at least one cell")
        p_box = None
        if box is not None:
            b = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
            if b.size != 6:
                raise ValueError("Context.set_media_grid: box must be (lo xyz, hi xyz), six numbers")
            p_box = C.c_void_p(b.ctypes.data)
        _check(lib().tor_scene_media_grid(self._h, int(medium), int(d.shape[0]), int(d.shape[1]), int(d.shape[2]), p_box,
                                          C.c_void_p(d.ctypes.data)))
        self._grid_media = getattr(self, "_grid_media", set()) | {int(medium)}

    def media_grid_info(self, medium):
        """(dims (nx, ny, nz) -- zeros: no grid --, box (6,) float64 or None, the 64-bit word of the media that have a grid)
        (tor_media_grid_info)."""
        dims, box, word = np.zeros(3, dtype=np.int32), np.zeros(6), np.zeros(1, dtype=np.uint64)
        _check(lib().tor_media_grid_info(self._h, int(medium), C.c_void_p(dims.ctypes.data), C.c_void_p(box.ctypes.data),
                                         C.c_void_p(word.ctypes.data)))
        return tuple(int(v) for v in dims), (box if dims[0] > 0 else None), int(word[0])

    def media_grids(self):
        """The media of the table that have a density grid, ascending.  A context that was given no grid since its last
        set_media answers [] without entering the library -- so that transmittance and the media integrators enter it exactly
        as they did before grids existed --; otherwise the library is asked (an upload that replaced the scene has dropped them,
        and with them the table: tor_media_grid_info then refuses, and [] is the answer).  This list, and so transmittance,
        trace_media and trace_media_direct, sees only grids set through set_media_grid of THIS object: a grid attached by calling
        tor_scene_media_grid on the context's handle directly is marched by march_media_grid and masked out of march_media, but
        is not in this list until set_media_grid has been called once (media_grid_info always asks the library)."""
        if not getattr(self, "_grid_media", None):
            return []
        word = np.zeros(1, dtype=np.uint64)
        dims = np.zeros(3, dtype=np.int32)
        if lib().tor_media_grid_info(self._h, 0, C.c_void_p(dims.ctypes.data), None, C.c_void_p(word.ctypes.data)) != 0:
            return []   # no scene or no media table any more: nothing to march
        return [m for m in range(MEDIA_MAX) if (int(word[0]) >> m) & 1]

    def march_media_grid(self, rays, tau, medium, t_range=None, index=None, out=None) -> "GridMarch":
        """The optical-depth march through the density grid of ONE medium (tor_media_grid_march_device / _host): regular tracking,
        an exact 3-D DDA walk through the piecewise-constant extinction sigma * density[cell] inside the medium's boundary sphere
        and the grid's box; the definition, operation by operation in float64, is in include/tor_grid.h.  The operands of
        march_media, and `medium`, the index of a medium that has a grid (set_media_grid).  Returns a GridMarch: a MediaMarch
        -- at a collision active is 1 << medium and rho the local extinction, so scatter_media, sample_phase and phase take it as
        they take march_media's -- with cell (n,) int32 (the cell of the collision, else -1) and medium.  Several sources: draw
        one budget per source (the table, each grid medium), march each, keep the earliest collision -- independent Poisson
        processes superpose --; the depths of a shadow segment add.  out: a GridMarch of an earlier call on as many rays."""
        if out is not None and not isinstance(out, GridMarch):
            raise ValueError("Context.march_media_grid: out must be a GridMarch")
        ops = _operands(self, "media_grid_march", rays, "rays", 7)
        n, rays = ops.n, ops.lead
        tau = ops.rows(tau, "tau", or_number=True)
        if tau is None:
            ops.bad("tau", "a number or an (n,) float64 tensor or array, as the rays are")
        t_range = ops.rows(t_range, "t_range", 2)
        index, n_list, p_list = ops.index(index)
        if out is None:
            status, t, depth, active, rho = ops.new(n, dtype="int32"), ops.new(n), ops.new(n), ops.new(n, dtype="int64"), ops.new(n)
            cell = ops.new(n, dtype="int32")
            cell[...] = -1
        else:
            status, t, depth, active, rho, cell = out.status, out.t, out.depth, out.active, out.rho, out.cell
            if not ops.fits(status, n, dtype="int32") or not ops.fits(t, n) or not ops.fits(depth, n) \
                    or not ops.fits(active, n, dtype="int64") or not ops.fits(rho, n) or not ops.fits(cell, n, dtype="int32"):
                ops.bad("out", "the result of a call on as many rays, on tensors or arrays as the rays are")
        ops.call(ops.ptr(rays), ops.ptr(t_range), ops.ptr(tau), int(medium), p_list, n_list, ops.ptr(status), ops.ptr(t),
                 ops.ptr(depth), ops.ptr(active), ops.ptr(rho), ops.ptr(cell))
        return GridMarch(status, t, depth, active, rho, cell, int(medium), ops.note(n_list), keep=ops.keep(rays, t_range, tau, index))

    def media_density(self, points, medium, index=None, out=None):
        """The density lookup (tor_media_grid_density_device / _host): per listed point (x, y, z, time) -- (n, 4) float64, a CUDA
        tensor or anything numpy takes -- the cell of medium `medium`'s grid that holds it and that cell's density (the grid's
        value, not multiplied by sigma); cell -1 and density 0 outside the boundary sphere or the box.  Returns (cell (n,) int32,
        density (n,) float64); out: such a pair of an earlier call, written again."""
        ops = _operands(self, "media_grid_density", points, "points", 4)
        n, points = ops.n, ops.lead
        index, n_list, p_list = ops.index(index)
        if out is None:
            cell, density = ops.new(n, dtype="int32"), ops.new(n)
            cell[...] = -1
        else:
            cell, density = out
            if not ops.fits(cell, n, dtype="int32") or not ops.fits(density, n):
                ops.bad("out", "a pair of contiguous (n,) int32 and (n,) float64 tensors or arrays, as the points are")
        ops.call(ops.ptr(points), int(medium), p_list, n_list, ops.ptr(cell), ops.ptr(density))
        return cell, density   # (copies made for the call are torch's, freed in stream order)

    # ---- surface textures (tor_scene_textures, tor_texture_eval_device): checker and octahedral image albedos ----

    def set_textures(self, textures, binding):
        """The texture table of the uploaded scene (tor_scene_textures, include/tor_texture.h): `textures` a list of Texture,
        `binding` (n_objects,) ints, the texture of every object of the uploaded list or -1 for none (such an object answers its
        material's albedo).  The images are packed into one atlas in list order.  An empty list clears the table, and so does
        every upload that replaces the scene; lights, environment, media, groups and photons leave it alone.  albedo() and
        trace(textures=True) / trace_direct(textures=True) read it; the render kernels and bounce() never do."""
        textures = list(textures)
        b = np.ascontiguousarray(np.asarray(binding).reshape(-1), dtype=np.int32)
        if not textures:
            _check(lib().tor_scene_textures(self._h, 0, None, int(b.size), None, 0, None))
            return
        table, atlas = pack_textures(textures)
        _check(lib().tor_scene_textures(self._h, len(textures), C.c_void_p(C.addressof(table)), int(b.size),
                                        C.c_void_p(b.ctypes.data) if b.size else None, int(atlas.shape[0]),
                                        C.c_void_p(atlas.ctypes.data) if atlas.size else None))

    def textures(self):
        """(n_textures -- 0: no table --, n_texels of the atlas, the objects bound to a texture) (tor_texture_info)."""
        out = np.zeros(3, dtype=np.int64)
        _check(lib().tor_texture_info(self._h, C.c_void_p(out.ctypes.data)))
        return int(out[0]), int(out[1]), int(out[2])

    def albedo(self, hits, index=None, out=None) -> "TextureEval":
        """The colour of the surface at each listed hit record (tor_texture_eval_device / tor_texture_eval_host): the texture bound
        to the record's object (set_textures) evaluated at the record -- a constant, a checker of p or of the outward normal, an
        octahedral image looked up by the outward normal -- or, for an object without a texture, the attenuation bounce() gives a
        ray that scattered off it; the definition, operation by operation in float64, is in include/tor_texture.h.

        hits: a HitResult / BounceResult or its (n, 8) raw records, as for bsdf(): a torch CUDA tensor (zero-copy, asynchronous on
        torch's current stream) or anything numpy takes (blocking); object, p, normal and front_face are read as given.  index as
        for bounce().  Nothing is drawn.  Returns a TextureEval(color (n, 3) float64, texel (n,) int32: an image's nearest texel
        row * n + col, a checker's parity, 0 for a constant, -1 where there is no texture or no usable direction); out: one of an
        earlier call on as many records, written again (records that are not listed keep what it holds); otherwise a new one
        (colour 0, texel -1)."""
        if out is not None and not isinstance(out, TextureEval):
            raise ValueError("Context.albedo: out must be a TextureEval")
        ops = _operands(self, "texture_eval", hits.raw if hasattr(hits, "raw") else hits, "hits", 8)
        n, raw = ops.n, ops.lead
        index, n_list, p_list = ops.index(index)
        if out is None:
            color, texel = ops.new(n, 3), ops.new(n, dtype="int32", zero=False)
            texel[...] = -1
        else:
            color, texel = out.color, out.texel
            if not ops.fits(color, n, 3) or not ops.fits(texel, n, dtype="int32"):
                ops.bad("out", "the result of a call on as many records, on tensors or arrays as the hits are")
        ops.call(ops.ptr(raw), p_list, n_list, ops.ptr(color), ops.ptr(texel))
        return TextureEval(color, texel, ops.note(n_list), keep=ops.keep(raw, index))

    # ---- planar patches (tor_scene_patches, tor_patch_hit_device, tor_patch_occluded_device): quads and triangles ----

    def set_patches(self, patches):
        """The patch table of the uploaded scene (tor_scene_patches, include/tor_patches.h): a list of Patch (Patch.quad,
        Patch.triangle, box_patches) -- static, two-sided parallelograms and triangles, each wearing the material of a scene
        object (or none) and a visibility word.  An empty list clears the table, and so does every upload that replaces the
        scene; lights, environment, media, textures, groups and photons leave it alone.  hit_patches(), occluded_patches() and
        trace_patches() read it; the render kernels, hit(), bounce() and every other query never do."""
        patches = list(patches)
        if not patches:
            _check(lib().tor_scene_patches(self._h, 0, None))
            return
        table = pack_patches(patches)
        _check(lib().tor_scene_patches(self._h, len(patches), C.c_void_p(C.addressof(table))))

    def patches(self):
        """(n_patches -- 0: no table --, the patches that wear a material) (tor_patch_info)."""
        out = np.zeros(2, dtype=np.int64)
        _check(lib().tor_patch_info(self._h, C.c_void_p(out.ctypes.data)))
        return int(out[0]), int(out[1])

    def _patch_operands(self, who, rays, t_range, index, mask):
        """What the two patch queries share: the rays, the ranges, the list and the mask pair (None: every group)."""
        ops = _operands(self, who, rays, "rays", 7)
        t_range = ops.rows(t_range, "t_range", 2)
        index, n_list, p_list = ops.index(index)
        mk, pair = (None, (0, 0xFFFFFFFF)) if mask is None else ops.mask(mask)
        return ops, t_range, index, n_list, p_list, mk, pair

    def hit_patches(self, rays, t_range=None, index=None, mask=None, merge=None, out=None) -> "PatchHits":
        """The closest patch of the table per listed ray (tor_patch_hit_device / tor_patch_hit_host): Moeller-Trumbore in float64,
        operation by operation as include/tor_patches.h defines it; the smallest accepted t wins, ties go to the lower index.

        rays: (n, 7) float64 -- a torch CUDA tensor (zero-copy, asynchronous on torch's current stream) or anything numpy takes
        (blocking); the time is not read.  t_range, index and mask as for occluded(): a patch takes part for ray i iff its
        groups & mask_i != 0.  merge: None -- the records are the patches' alone, a ray without a patch gets hit()'s miss record;
        or a HitResult / BounceResult or its (n, 8) raw records: the answer starts from a copy of them (in place with out=), a
        patch replaces a record only where it is strictly nearer than the record's t (a tie stays with the sphere), and a ray
        without such a patch keeps its record.  Returns PatchHits: a HitResult's fields -- `object` the patch's material -- plus
        patch (n,) int32 (-1: no patch) and uv (n, 2) float64, the patch's coordinates (a, b) of the point.  out: a PatchHits of
        an earlier call on as many rays, written again (rays that are not listed keep what it holds; with merge given too, out
        is merged into and merge itself only says so)."""
        if out is not None and not isinstance(out, PatchHits):
            raise ValueError("Context.hit_patches: out must be a PatchHits")
        ops, t_range, index, n_list, p_list, mk, pair = self._patch_operands("patch_hit", rays, t_range, index, mask)
        n, rays = ops.n, ops.lead
        if out is not None:
            raw, patch, uv = out.raw, out.patch, out.uv
            if not ops.fits(raw, n, 8) or not ops.fits(patch, n, dtype="int32") or not ops.fits(uv, n, 2):
                ops.bad("out", "the result of a call on as many rays, on tensors or arrays as the rays are")
        else:
            if merge is None:
                raw = ops.new(n, 8, unused=14)
            else:
                raw = ops.rows(merge.raw if hasattr(merge, "raw") else merge, "merge", 8)
                raw = raw.clone() if _is_tensor(raw) else raw.copy()
            patch, uv = ops.new(n, dtype="int32", zero=False), ops.new(n, 2)
            patch[...] = -1
        ops.call(ops.ptr(rays), ops.ptr(t_range), p_list, n_list, 0 if merge is None else 1, ops.ptr(raw), ops.ptr(patch),
                 ops.ptr(uv), after=pair)
        return PatchHits(raw, ops.words(raw), patch, uv, ops.note(n_list), keep=ops.keep(rays, t_range, index, mk))

    def occluded_patches(self, rays, t_range=None, index=None, mask=None, merge=None, out=None) -> "OccludedResult":
        """Any-hit query against the patch table (tor_patch_occluded_device / tor_patch_occluded_host): per listed ray ONE bit,
        whether some patch is accepted in (t_min, t_max).  rays, t_range, index, mask as for hit_patches().  merge: None -- the
        bit is written, 0 or 1; or an OccludedResult of occluded() (or its raw int32 array): the answer starts from a copy of it
        (in place with out=) and the query only ever writes 1, so the result is "a sphere or a patch occludes".  out: an
        OccludedResult of an earlier call on as many rays, or its raw int32 array, written again."""
        ops, t_range, index, n_list, p_list, mk, pair = self._patch_operands("patch_occluded", rays, t_range, index, mask)
        n, rays = ops.n, ops.lead
        raw = out.raw if hasattr(out, "raw") else out
        if raw is None:
            if merge is None:
                raw = ops.new(n, dtype="int32")
            else:
                raw = ops.rows(merge.raw if hasattr(merge, "raw") else merge, "merge", dtype="int32")
                raw = raw.clone() if _is_tensor(raw) else raw.copy()
        elif not ops.fits(raw, n, dtype="int32"):
            ops.bad("out", "a contiguous (n,) int32 tensor or array, as the rays are")
        ops.call(ops.ptr(rays), ops.ptr(t_range), p_list, n_list, 0 if merge is None else 1, ops.ptr(raw), after=pair)
        return OccludedResult(raw, ops.as_bool(raw), ops.note(n_list), keep=ops.keep(rays, t_range, index, mk))

    def transmittance(self, p, q, time=0.0, mask=None):
        """The transmittance of the segments p -> q through the media of the table: exp(-depth) of march_media on the rays
        p -> q - p with range (0, 1) and tau = inf -- the exp is torch's or numpy's, as p is; the library computes the depth
        alone.  With density grids (set_media_grid) the depth is march_media's plus each grid medium's march_media_grid depth at
        tau = inf, added in ascending medium order.  mask: None, or what may stand in the way as for visible(): the result is
        then multiplied by visible(p, q, time, mask=mask).  One value per segment, a tensor or an array as p is."""
        rays, tr = self.shadow_segments(p, q, time, 0.0)
        depth = self.march_media(rays, float("inf"), tr).depth
        for m in self.media_grids():
            depth = depth + self.march_media_grid(rays, float("inf"), m, tr).depth
        if _is_tensor(depth):
            import torch
            tm = torch.exp(-depth)
        else:
            tm = np.exp(-depth)
        if mask is not None:
            tm = tm * self.visible(p, q, time, mask=mask)
        return tm

    @staticmethod
    def shadow_segments(p, q, time=0.0, t_min=0.001):
        """The rays and ranges of the segments p -> q (what visible() queries): ((n, 7) rays with origin p, direction q - p and
        `time` (a scalar or one per segment), (n, 2) ranges (t_min, 1.0)) -- torch tensors when p is one, else numpy arrays."""
        if _is_tensor(p):
            import torch
            p = p.reshape(-1, 3)
            q = torch.as_tensor(q, dtype=p.dtype, device=p.device).reshape(-1, 3)
            n = int(p.shape[0])
            rays = torch.empty((n, 7), dtype=torch.float64, device=p.device)
            rays[:, 0:3], rays[:, 3:6] = p, q - p
            rays[:, 6] = torch.as_tensor(time, dtype=torch.float64, device=p.device)
            tr = torch.empty((n, 2), dtype=torch.float64, device=p.device)
            tr[:, 0], tr[:, 1] = float(t_min), 1.0
            return rays, tr
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
        n = p.shape[0]
        rays = np.empty((n, 7), dtype=np.float64)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = p, q - p, time
        tr = np.empty((n, 2), dtype=np.float64)
        tr[:, 0], tr[:, 1] = t_min, 1.0
        return rays, tr

    def visible(self, p, q, time=0.0, t_min=0.001, mask=None, **kw):
        """Is q visible from p?  Sugar over occluded(): the rays p -> q - p with range (t_min, 1.0) (shadow_segments), and
        ~occluded of them -- a bool tensor / array, one per segment.  mask: what may stand in the way, as for occluded() -- a
        segment towards a lamp leaves the lamp's group out instead of stopping short of its surface.  kw: index, time_range,
        mode of occluded()."""
        rays, tr = self.shadow_segments(p, q, time, t_min)
        if mask is not None:
            kw["mask"] = mask
        return ~self.occluded(rays, tr, **kw).occluded

    # (trace, trace_direct, trace_light, trace_photons, trace_photon_map, trace_environment and trace_media are the functions of
    # integrators.py, given to this class at the end of the module)


def _mode_of(note: str, prefix: str) -> str:
    for p in (prefix, prefix[:-2] + " (masked): "):
        if note.startswith(p):
            return note[len(p):]
    return note


def _mask_words(a: np.ndarray) -> np.ndarray:
    """Group / mask words as contiguous uint32: int32 words count by their bits, wider integers must fit 32 bits."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError("group and mask words must be integers")
    if a.dtype.itemsize == 4:
        return np.ascontiguousarray(a).view(np.uint32)
    if a.size and (int(a.min()) < -(1 << 31) or int(a.max()) > 0xFFFFFFFF):
        raise ValueError("group and mask words must fit 32 bits")
    return np.ascontiguousarray((a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32))


def environment_directions(n, a=0.5, b=0.5) -> np.ndarray:
    """The (n, n, 3) float64 unit directions of the positions (a, b) in [0, 1) inside every texel of an n x n octahedral
    environment map, [row][col] -- include/tor_env.h's decode, operation by operation in numpy; (0.5, 0.5) are the texel centres.
    A host bakes any sky with it: set_environment(f(environment_directions(n))) -- and any surface image, whose square is the
    same mapping of the outward normal: Texture.image(f(environment_directions(n)))."""
    n = int(n)
    if not 1 <= n <= ENV_MAX_SIDE:
        raise ValueError(f"environment_directions: need 1 <= n <= {ENV_MAX_SIDE}")
    h = 2.0 / float(n)
    s = np.broadcast_to(((np.arange(n, dtype=np.float64) + float(a)) * h - 1.0)[None, :], (n, n))
    t = np.broadcast_to(((np.arange(n, dtype=np.float64) + float(b)) * h - 1.0)[:, None], (n, n))
    py = (1.0 - np.abs(s)) - np.abs(t)
    up = py >= 0
    px = np.where(up, s, np.copysign(1.0 - np.abs(t), s))
    pz = np.where(up, t, np.copysign(1.0 - np.abs(s), t))
    inv = 1.0 / np.sqrt(px * px + py * py + pz * pz)
    return np.stack([px * inv, py * inv, pz * inv], axis=-1)


def diffuse_objects(scene) -> np.ndarray:
    """One bool per object of `scene` (a Scene or its (n, 16) records): is its material Lambertian (kind == MAT_LAMBERTIAN, read as
    groups_by_material reads the records) -- the `diffuse` operand of Context.trace_direct."""
    recs = scene.to_records() if hasattr(scene, "to_records") else np.asarray(scene, dtype=np.float64).reshape(-1, 16)
    return recs[:, 10].astype(np.int64) == MAT_LAMBERTIAN


def glossy_objects(scene) -> np.ndarray:
    """One bool per object of `scene` (a Scene or its (n, 16) records): is its material a Metal with fuzz != 0 -- a lobe with a
    density (Context.bsdf answers BSDF_DENSITY), not a mirror: the `glossy` operand of Context.trace_direct."""
    recs = scene.to_records() if hasattr(scene, "to_records") else np.asarray(scene, dtype=np.float64).reshape(-1, 16)
    return (recs[:, 10].astype(np.int64) == MAT_METAL) & (recs[:, 14] != 0.0)


def groups_by_material(scene) -> np.ndarray:
    """One group word per object of `scene` (a Scene or its (n, 16) records): 1 << material kind (MAT_LAMBERTIAN 0, MAT_METAL 1,
    MAT_DIELECTRIC 2), for Context.set_groups.  Shadow rays that skip glass: mask = ~(1 << MAT_DIELECTRIC) & 0xFFFFFFFF."""
    recs = scene.to_records() if hasattr(scene, "to_records") else np.asarray(scene, dtype=np.float64).reshape(-1, 16)
    return (np.uint32(1) << recs[:, 10].astype(np.uint32)).astype(np.uint32)


class TextureRecord(C.Structure):
    """TorTexture (include/tor_texture.h), 96 bytes."""
    _fields_ = [("kind", C.c_int32), ("option", C.c_int32), ("side", C.c_int32), ("reserved", C.c_int32), ("offset", C.c_int64),
                ("a", C.c_double * 3), ("b", C.c_double * 3), ("freq", C.c_double * 3)]


assert C.sizeof(TextureRecord) == 96, "TorTexture is 96 bytes on both sides of the ABI"


class Texture:
    """One texture of Context.set_textures (include/tor_texture.h): Texture.constant(rgb), Texture.checker(even, odd, freq,
    space) or Texture.image(rgb, filter).  kind, option, a, b, freq are the record's fields; rgb is an image's (n, n, 3) float64
    texels, [row][col] of the octahedral square of the OUTWARD NORMAL -- environment_directions(n) gives the direction of every
    texel centre, so an image is baked with one call: Texture.image(f(environment_directions(n)))."""
    __slots__ = ("kind", "option", "a", "b", "freq", "rgb")

    def __init__(self, kind, option=0, a=(0.0, 0.0, 0.0), b=(0.0, 0.0, 0.0), freq=(0.0, 0.0, 0.0), rgb=None):
        self.kind, self.option = int(kind), int(option)
        self.a, self.b, self.freq = (tuple(float(x) for x in np.asarray(c, dtype=np.float64).reshape(3)) for c in (a, b, freq))
        self.rgb = rgb

    @classmethod
    def constant(cls, rgb) -> "Texture":
        """One colour everywhere."""
        return cls(TEXTURE_CONSTANT, a=rgb)

    @classmethod
    def checker(cls, even, odd, freq=1.0, space="world") -> "Texture":
        """A 3-D checker: `even` where the parities of floor(x * freq) per axis sum to an even number, else `odd`; freq a number
        or one per axis (cells per unit); space "world" (x = the record's p) or "normal" (x = the outward normal: the pattern
        rides a moving sphere)."""
        if space not in TEXTURE_SPACES:
            raise ValueError('Texture.checker: space must be "world" or "normal"')
        f = np.broadcast_to(np.asarray(freq, dtype=np.float64), (3,))
        return cls(TEXTURE_CHECKER, TEXTURE_SPACES[space], even, odd, f)

    @classmethod
    def image(cls, rgb, filter="nearest") -> "Texture":
        """An (n, n, 3) octahedral image, looked up by the outward normal; filter "nearest" or "bilinear"."""
        if filter not in TEXTURE_FILTERS:
            raise ValueError('Texture.image: filter must be "nearest" or "bilinear"')
        c = np.ascontiguousarray(np.asarray(rgb, dtype=np.float64))
        if c.ndim != 3 or c.shape[0] != c.shape[1] or c.shape[2] != 3 or not 1 <= c.shape[0] <= TEXTURE_MAX_SIDE:
            raise ValueError(f"Texture.image: rgb must be (n, n, 3) with 1 <= n <= {TEXTURE_MAX_SIDE}")
        return cls(TEXTURE_IMAGE, TEXTURE_FILTERS[filter], rgb=c)


def pack_textures(textures):
    """The table and the atlas of a list of Texture: (a ctypes array of TextureRecord, (n_texels, 3) float64) -- the images one
    after the other in list order, each [row][col] from its offset."""
    textures = list(textures)
    table = (TextureRecord * max(1, len(textures)))()
    parts, at = [], 0
    for j, t in enumerate(textures):
        if not isinstance(t, Texture):
            raise ValueError("Context.set_textures: textures must be a list of Texture")
        r = table[j]
        r.kind, r.option = t.kind, t.option
        r.a[:], r.b[:], r.freq[:] = t.a, t.b, t.freq
        if t.kind == TEXTURE_IMAGE:
            r.side, r.offset = int(t.rgb.shape[0]), at
            parts.append(t.rgb.reshape(-1, 3))
            at += int(t.rgb.shape[0]) ** 2
    atlas = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 3), dtype=np.float64)
    return table, atlas


class PatchRecord(C.Structure):
    """TorPatch (include/tor_patches.h), 88 bytes."""
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("groups", C.c_uint32), ("reserved", C.c_int32),
                ("q", C.c_double * 3), ("u", C.c_double * 3), ("v", C.c_double * 3)]


assert C.sizeof(PatchRecord) == 88, "TorPatch is 88 bytes on both sides of the ABI"


class Patch:
    """One patch of Context.set_patches (include/tor_patches.h): the surface q + a * u + b * v, a parallelogram (Patch.quad:
    0 <= a, b <= 1) or a triangle (Patch.triangle: a, b >= 0, a + b <= 1), two-sided and static.  material: the index of the
    scene object whose material it wears (what a hit's `object` says), or -1 for none; groups: its visibility word."""
    __slots__ = ("kind", "material", "groups", "q", "u", "v")

    def __init__(self, kind, q, u, v, material=-1, groups=0xFFFFFFFF):
        self.kind, self.material, self.groups = int(kind), int(material), int(groups) & 0xFFFFFFFF
        self.q, self.u, self.v = (tuple(float(x) for x in np.asarray(c, dtype=np.float64).reshape(3)) for c in (q, u, v))

    @classmethod
    def quad(cls, q, u, v, material=-1, groups=0xFFFFFFFF) -> "Patch":
        """The parallelogram with the corner q and the edges u and v from it."""
        return cls(PATCH_QUAD, q, u, v, material, groups)

    @classmethod
    def triangle(cls, a, b, c, material=-1, groups=0xFFFFFFFF) -> "Patch":
        """The triangle with the corners a, b, c: q = a, u = b - a, v = c - a."""
        a, b, c = (np.asarray(x, dtype=np.float64).reshape(3) for x in (a, b, c))
        return cls(PATCH_TRIANGLE, a, b - a, c - a, material, groups)


def box_patches(lo, hi, material=-1, groups=0xFFFFFFFF) -> list:
    """The six quads of the axis-aligned box lo .. hi, cross(u, v) of each pointing outwards: -x, +x, -y, +y, -z, +z."""
    lo, hi = (np.asarray(x, dtype=np.float64).reshape(3) for x in (lo, hi))
    e = np.diag(hi - lo)
    out = []
    for k in range(3):
        a, b = e[(k + 1) % 3], e[(k + 2) % 3]   # cross(a, b) points along +k
        out.append(Patch.quad(lo, b, a, material, groups))
        out.append(Patch.quad(lo + e[k], a, b, material, groups))
    return out


def pack_patches(patches):
    """The table of a list of Patch: a ctypes array of PatchRecord."""
    patches = list(patches)
    table = (PatchRecord * max(1, len(patches)))()
    for j, p in enumerate(patches):
        if not isinstance(p, Patch):
            raise ValueError("Context.set_patches: patches must be a list of Patch")
        r = table[j]
        r.kind, r.material, r.groups = p.kind, p.material, p.groups
        r.q[:], r.u[:], r.v[:] = p.q, p.u, p.v
    return table


class HitResult:
    """Closest hits of Context.hit, one TorHit per ray (include/tor_render.h): t, p (n, 3), normal (n, 3), object (int32, -1 = miss)
    and front_face (int32) are views of `raw` ((n, 8) float64, the records as the library wrote them) -- torch tensors or numpy
    arrays, as the rays were.  `mode` is what ran: "blocks" or "brute force (...)" (tor_last_note)."""

    def __init__(self, raw, words, note: str, keep=None):
        self.raw, self._keep = raw, keep   # (keep: the rays' contiguous copy stays alive while the query may run)
        self.p, self.normal, self.t = raw[:, 0:3], raw[:, 3:6], raw[:, 6]
        self.object, self.front_face = words[:, 14], words[:, 15]
        self.mode = _mode_of(note, "hit: ")


class BounceResult(HitResult):
    """One path step of Context.bounce / Context.scatter: HitResult's fields (the records of the step's closest hits, or the caller's),
    attenuation (n, 3) float64, status (n,) int32 (BOUNCE_MISS / BOUNCE_SCATTERED / BOUNCE_ABSORBED), rays (n, 7) and rng (n, 4) as the
    step left them, and `mode`: "blocks" | "brute force (...)" for a bounce, "scatter" for a scatter."""

    def __init__(self, raw, words, note: str, attenuation, status, rays, rng, keep=None):
        super().__init__(raw, words, note, keep=keep)
        self.attenuation, self.status, self.rays, self.rng = attenuation, status, rays, rng
        self.mode = _mode_of(note, "bounce: ")


class PatchHits(HitResult):
    """Closest patches of Context.hit_patches, one per ray (include/tor_patches.h): HitResult's fields (object: the patch's
    material, or what the merged record held), patch (n,) int32 the table index (-1: no patch), uv (n, 2) float64 the patch's
    coordinates of the point, and `mode` ("patch hit")."""
    def __init__(self, raw, words, patch, uv, note: str, keep=None):
        super().__init__(raw, words, note, keep)
        self.patch, self.uv = patch, uv


class OccludedResult:
    """Any-hit answers of Context.occluded, one per ray: `occluded` is a bool view of `raw` ((n,) int32, 1 = world.hit returns true,
    as the library wrote it; rays that were not listed keep what `out` held) -- torch tensors or numpy arrays, as the rays were.
    `mode` is what ran: "blocks" or "brute force (...)" (tor_last_note)."""

    def __init__(self, raw, occluded, note: str, keep=None):
        self.raw, self.occluded, self._keep = raw, occluded, keep   # (keep: the operands' contiguous copies stay alive while the query may run)
        self.mode = _mode_of(note, "occluded: ")


class CrossingsResult:
    """Ordered crossings of Context.crossings, k per ray (TorCrossing, include/tor_render.h): t (n, k) float64, object (n, k) int32
    (-1 = unused entry) and which (n, k) int32 (0 = the near root, 1 = the far one) are views of `raw` ((n, k, 2) float64, the
    entries as the library wrote them); count (n,) int32 is how many entries of a ray are crossings; hits is None, or with
    records=True the (n, k, 8) raw TorHit records (HitResult's layout per crossing).  Torch tensors or numpy arrays, as the rays
    were.  `mode` is what ran: "blocks" or "brute force (...)" (tor_last_note)."""

    def __init__(self, raw, words, count, hits, note: str, keep=None):
        self.raw, self.count, self.hits, self._keep = raw, count, hits, keep   # (keep: the operands stay alive while the query may run)
        self.t, self.object, self.which = raw[:, :, 0], words[:, :, 2], words[:, :, 3]
        self.mode = _mode_of(note, "crossings: ")


class NearestResult:
    """Nearest neighbours of Context.nearest, k per point (TorNear, include/tor_render.h): distance (n, k) float64 (signed, negative
    inside), object (n, k) int32 (-1 = unused entry) and inside (n, k) int32 (1 = the point lies inside the object) are views of
    `raw` ((n, k, 2) float64, the entries as the library wrote them); count (n,) int32 is how many entries of a point are
    neighbours.  Torch tensors or numpy arrays, as the points were.  `mode` is what ran: "blocks" or "brute force (...)"
    (tor_last_note)."""

    def __init__(self, raw, words, count, note: str, keep=None):
        self.raw, self.count, self._keep = raw, count, keep   # (keep: the operands stay alive while the query may run)
        self.distance, self.object, self.inside = raw[:, :, 0], words[:, :, 2], words[:, :, 3]
        self.mode = _mode_of(note, "nearest: ")


class LightSample:
    """Light samples of Context.sample_lights, one per point (include/tor_lights.h): rays (n, 7) float64 {origin p, direction to
    the sampled surface point (parameter 1.0), time}, pdf (n,) float64 per unit solid angle with the selection probability
    included, light (n,) int32 the picked light's OBJECT index (-1: none), dist (n,) float64 the distance to the surface point,
    rng (n, 4) the states after the three draws -- torch tensors or numpy arrays, as the points were.  `mode`: "by weight" |
    "by solid angle"."""

    def __init__(self, rays, pdf, light, dist, rng, note: str, keep=None):
        self.rays, self.pdf, self.light, self.dist, self.rng, self._keep = rays, pdf, light, dist, rng, keep
        self.mode = _mode_of(note, "light sample: ")


class EnvSample:
    """Environment samples of Context.sample_environment, one per point (include/tor_env.h): rays (n, 7) float64 {origin p, unit
    direction, time}, pdf (n,) float64 per unit solid angle, texel (n,) int32 row * n + col (-1: never written), color (n, 3)
    float64 the texel's RGB, rng (n, 4) the states after the four draws -- torch tensors or numpy arrays, as the points were.
    `mode`: "env sample"."""

    def __init__(self, rays, pdf, texel, color, rng, note: str, keep=None):
        self.rays, self.pdf, self.texel, self.color, self.rng, self._keep = rays, pdf, texel, color, rng, keep
        self.mode = note


class CameraConnection:
    """Camera connections of Context.connect_camera, one per point (include/tor_camera.h): rays (n, 7) float64 {origin the point,
    direction to the lens point (parameter 1.0), time}, pixel (n,) int32 row * ncols + col (-1: none), factor (n,) float64 the
    measurement weight, lens (n, 2) float64 the lens point in the camera's (u, v), rng (n, 4) the states after the two draws --
    torch tensors or numpy arrays, as the points were.  `mode`: "pinhole" | "thin lens"."""

    def __init__(self, rays, pixel, factor, lens, rng, note: str, keep=None):
        self.rays, self.pixel, self.factor, self.lens, self.rng, self._keep = rays, pixel, factor, lens, rng, keep
        self.mode = _mode_of(note, "camera connect: ")


class LightEmission:
    """Path starts of Context.emit_lights, one per state (include/tor_camera.h): rays (n, 7) float64 {origin on the lamp, unit
    direction, time}, normal (n, 3) float64, light (n,) int32 the picked light's OBJECT index (-1: never written), pdf (n, 2)
    float64 whose columns are pdf_area (per unit area, the pick included) and pdf_dir (cos / pi per unit solid angle), rng
    (n, 4) the states after the six draws -- torch tensors or numpy arrays, as the states were.  `mode`: "by weight"."""

    def __init__(self, rays, normal, light, pdf, rng, note: str, keep=None):
        self.rays, self.normal, self.light, self.pdf, self.rng, self._keep = rays, normal, light, pdf, rng, keep
        self.pdf_area, self.pdf_dir = pdf[:, 0], pdf[:, 1]
        self.mode = _mode_of(note, "light emit: ")


class BsdfEval:
    """Answers of Context.bsdf, one per item (include/tor_bsdf.h): value (n, 3) float64 albedo * pdf (f_r cos), pdf (n,) the
    solid-angle density Material.scatter gives the outgoing direction, kind (n,) int32 (BSDF_NONE / BSDF_DENSITY / BSDF_DELTA)
    and note (tor_last_note)."""
    __slots__ = ("value", "pdf", "kind", "note", "_keep")

    def __init__(self, value, pdf, kind, note: str, keep=None):
        self.value, self.pdf, self.kind, self.note, self._keep = value, pdf, kind, note, keep


class TextureEval:
    """Answers of Context.albedo, one per record (include/tor_texture.h): color (n, 3) float64 the surface's colour, texel (n,)
    int32 (an image's nearest texel row * n + col, a checker's parity, 0 for a constant, -1: no texture, no object or no usable
    direction), and `mode` ("texture eval")."""
    __slots__ = ("color", "texel", "mode", "_keep")

    def __init__(self, color, texel, note: str, keep=None):
        self.color, self.texel, self.mode, self._keep = color, texel, note, keep


class PhotonMap:
    """What Context.build_photons returns: scale (the power of two the stored powers were multiplied by), radius (the map's R),
    note (tor_last_note) and info() -- {stored, dropped, n_buckets, largest_bucket}, read back (blocking) when first asked for.
    The map itself lives in the context; this names the one that was current when it was built."""
    __slots__ = ("ctx", "scale", "radius", "note", "_info")

    def __init__(self, ctx, scale: float, radius: float, note: str):
        self.ctx, self.scale, self.radius, self.note, self._info = ctx, scale, radius, note, None

    def info(self) -> dict:
        if self._info is None:
            self._info = self.ctx.photons_info()
        return self._info


class Photons:
    """Context.trace_photons' photons, the operands of Context.build_photons: position, power, direction (m, 3) float64, paths
    (the number of light paths that were started -- what PhotonGather.irradiance divides by), rng (the states after the paths'
    last draws) and mode."""
    __slots__ = ("position", "power", "direction", "paths", "rng", "mode")

    def __init__(self, position, power, direction, paths: int, rng=None, mode: str = ""):
        self.position, self.power, self.direction, self.paths, self.rng, self.mode = position, power, direction, int(paths), rng, mode


class PhotonGather:
    """Answers of Context.gather_photons, one per point (include/tor_photons.h): sums (n, 3) float64 the clamped, quantised
    weighted powers (in the map's scaled units), count (n,) int32 the accepted photons; scale, radius (min(radius, R): a number
    or one per point), kernel (0 constant, 1 Epanechnikov), max_value and note."""
    __slots__ = ("sums", "count", "scale", "radius", "kernel", "max_value", "note", "_keep")

    def __init__(self, sums, count, scale: float, radius, kernel: int, max_value: float, note: str, keep=None):
        self.sums, self.count, self.scale, self.radius, self.kernel, self.max_value = sums, count, scale, radius, kernel, max_value
        self.note, self._keep = note, keep

    def irradiance(self, paths):
        """The density estimate (n, 3): sums / scale, times the kernel's normalisation -- 1 / (pi r^2) for the constant disc,
        2 / (pi r^2) for Epanechnikov -- divided by `paths`, the number of light paths behind the map.  0 where nothing was
        accepted (a radius of 0, negative or NaN among them)."""
        c = (2.0 if self.kernel == 1 else 1.0) / (math.pi * float(paths) * self.scale)
        r = self.radius
        if isinstance(r, (int, float)):
            return self.sums * (c / (r * r)) if r > 0 else self.sums * 0.0
        xp = sys.modules["torch"] if _is_tensor(r) else np
        f = xp.where(self.count > 0, c / (r * r), xp.zeros_like(r))
        return self.sums * f[:, None]

    def budget(self) -> int:
        """The most photons a point may accept with exact sums: count * max_value < 2^17."""
        return int(math.ceil(MAX_ACCUM_SAMPLES / self.max_value)) - 1

    def check_budget(self) -> int:
        """Raises when a point accepted more photons than budget(), i.e. its sums may have stopped being exact and may depend on
        the order inside the buckets.  Returns the largest count.  Blocking."""
        n = int(self.count.max()) if len(self.count) else 0
        if n > self.budget():
            raise TorError(ERR_INVALID_ARGUMENT, f"PhotonGather.check_budget: {n} photons at one point, above the exactness bound "
                                                 f"{self.budget()} of max_value = {self.max_value:g}")
        return n


class MediaMarch:
    """The answers of Context.march_media, one per ray (include/tor_media.h): status (n,) int32 (MEDIA_COLLIDED / MEDIA_ESCAPED /
    MEDIA_REFUSED), t, depth and rho (n,) float64, active (n,) int64 holding the 64 bits of the active set -- torch tensors or numpy
    arrays, as the rays were; rays that were not listed keep what `out` held.  `mode` is the library's note ("5 media")."""

    def __init__(self, status, t, depth, active, rho, note: str, keep=None):
        self.status, self.t, self.depth, self.active, self.rho, self._keep = status, t, depth, active, rho, keep
        self.mode = _mode_of(note, "media march: ")


class GridMarch(MediaMarch):
    """The answers of Context.march_media_grid (include/tor_grid.h): a MediaMarch -- at a collision active is 1 << medium and rho the
    local extinction sigma * density[cell] -- with cell (n,) int32, the cell of the collision (-1 otherwise), and `medium`.  `mode`
    is the library's note ("medium 3, 16x16x16")."""

    def __init__(self, status, t, depth, active, rho, cell, medium: int, note: str, keep=None):
        super().__init__(status, t, depth, active, rho, note, keep)
        self.cell, self.medium = cell, medium
        self.mode = _mode_of(note, "media grid march: ")


class MediaScatter(tuple):
    """The answers of Context.scatter_media: the pair (rays (n, 7), attenuation (n, 3)), which also carries them by name with rng
    ((n, 4), the states as the scatter left them) and `mode`, the library's note."""

    def __new__(cls, rays, attenuation, rng, note: str, keep=None):
        self = super().__new__(cls, (rays, attenuation))
        self.rays, self.attenuation, self.rng, self._keep = rays, attenuation, rng, keep
        self.mode = _mode_of(note, "media scatter: ")
        return self


class PhaseSample(tuple):
    """The answers of Context.sample_phase: the pair (rays (n, 7), attenuation (n, 3)) as a MediaScatter is, which also carries
    them by name with pdf (n,) -- the solid-angle density of the drawn direction --, rng ((n, 4), the states as the draws left
    them) and `mode`, the library's note."""

    def __new__(cls, rays, attenuation, pdf, rng, note: str, keep=None):
        self = super().__new__(cls, (rays, attenuation))
        self.rays, self.attenuation, self.pdf, self.rng, self._keep = rays, attenuation, pdf, rng, keep
        self.mode = _mode_of(note, "phase sample: ")
        return self


class PhaseEval:
    """The answers of Context.phase, one per item (include/tor_phase.h): value (n, 3) float64 the mixture's albedo times its
    phase function, pdf (n,) the density sample_phase gives the outgoing direction, `mode` the library's note."""
    __slots__ = ("value", "pdf", "mode", "_keep")

    def __init__(self, value, pdf, note: str, keep=None):
        self.value, self.pdf, self._keep = value, pdf, keep
        self.mode = _mode_of(note, "phase eval: ")


class Uniforms(tuple):
    """The answers of Context.uniform: the pair (u (m, n) float64, rng (m, 4), the states as the draws left them), which also carries
    them by name with `mode`, the library's note."""

    def __new__(cls, u, rng, note: str, keep=None):
        self = super().__new__(cls, (u, rng))
        self.u, self.rng, self._keep = u, rng, keep   # (keep: the list stays alive while the query may run)
        self.mode = _mode_of(note, "rng uniform: ")
        return self


class EnvEval:
    """Context.environment(pdf=True), one entry per ray (include/tor_env.h): color (n, 3) float64, pdf (n,) float64 the density
    sample_environment gives the ray's direction, texel (n,) int32 row * n + col (-1: an unusable direction, or not listed).
    `mode`: "env eval"."""

    def __init__(self, color, pdf, texel, note: str):
        self.color, self.pdf, self.texel, self.mode = color, pdf, texel, note


class Progressive:
    """Progressive, resumable rendering of one (camera, size, depth, options) in TOR_SEED_SAMPLE mode: owns the device sums (and,
    with moments=True, the second moments) of this shard's rows.  Passes of samples add up exactly, so after any sequence of
    add() calls totalling n samples, image() is the canvas a one-shot n-spp render_device gives, bit for bit.

        pg = Progressive(ctx, cam, 1080, 1920, 50, make_options(seeding=SEED_SAMPLE), moments=True)
        pg.add(16); preview = pg.image(); pg.render_until(max_se=1e-3, max_samples=4096)

    The context must have the scene uploaded; all device work runs on torch's current stream of the buffers' device."""

    # what a subclass on other streams changes (PixelProgressive): the seeding it needs, its refusal, its default options
    _SEEDING = SEED_SAMPLE
    _REFUSAL = ("Progressive: needs TOR_SEED_SAMPLE (TOR_SEED_PIXEL pixels are sequential chains "
                "on one generator and cannot be resumed)")

    @staticmethod
    def _default_options() -> Options:
        return make_options(seeding=SEED_SAMPLE)

    def __init__(self, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None = None,
                 moments: bool = False, device=None):
        import torch
        self.ctx, self.nrows, self.ncols, self.max_depth = ctx, int(nrows), int(ncols), int(max_depth)
        self.cam = Camera.from_buffer_copy(cam)
        self.options = Options.from_buffer_copy(options if options is not None else self._default_options())
        if self.options.seeding != self._SEEDING:
            raise TorError(ERR_INVALID_ARGUMENT, self._REFUSAL)
        self.rows = len(shard_rows(self.nrows, max(int(self.options.row_tile), 1), int(self.options.shard_index),
                                   max(int(self.options.shard_count), 1)))
        dev = torch.device("cuda") if device is None else torch.device(device)
        self.sums = torch.zeros((self.rows, self.ncols, 3), dtype=torch.float64, device=dev)
        self.moments = torch.zeros_like(self.sums) if moments else None
        self.samples = 0

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.sums.device).cuda_stream

    def add(self, n: int) -> "Progressive":
        """Render the next n samples per pixel into the sums (asynchronous on the current stream)."""
        self.ctx.accumulate_device(self.cam, self.nrows, self.ncols, self.samples, int(n), self.max_depth, self.options,
                                   self.sums.data_ptr(), self.moments.data_ptr() if self.moments is not None else 0, self._stream())
        self.samples += int(n)
        return self

    def image(self, gamma: float = 2.2):
        """The gamma-corrected canvas of the samples so far: a new device float64 tensor (rows of this shard, ncols, 3)."""
        import torch
        out = torch.empty_like(self.sums)
        self.ctx.resolve_device(self.sums.data_ptr(), self.sums.numel(), self.samples, gamma, out.data_ptr(), self._stream())
        return out

    def to_canvas(self, canvas: Canvas) -> Canvas:
        """Fill a host Canvas (whole frame, unsharded options) with image(canvas.gamma_correction), so export_ppm works."""
        if (canvas.nrows, canvas.ncols) != (self.rows, self.ncols):
            raise TorError(ERR_INVALID_ARGUMENT, f"{type(self).__name__}.to_canvas: the canvas must have this render's rows and columns")
        canvas.pixels[...] = self.image(canvas.gamma_correction).cpu().numpy()
        canvas.samples_per_pixel = self.samples
        return canvas

    def noise(self):
        """(mean, max) over the pixels of the largest per-channel standard error of the mean, linear units.  Blocking."""
        if self.moments is None:
            raise TorError(ERR_INVALID_ARGUMENT, f"{type(self).__name__}.noise: created without moments=True")
        return self.ctx.accum_noise_device(self.sums.data_ptr(), self.moments.data_ptr(), self.rows * self.ncols, self.samples, 0,
                                           self._stream())

    def render_until(self, max_se: float, max_samples: int, pass_samples: int = 16) -> int:
        """Add passes of pass_samples until the largest per-pixel standard error is <= max_se or max_samples are reached
        (the last pass is shortened to land on max_samples).  Returns the sample count."""
        while self.samples < max_samples:
            self.add(min(int(pass_samples), int(max_samples) - self.samples))
            if self.moments is not None and self.samples >= 2 and self.noise()[1] <= max_se:
                break
        return self.samples

    def state(self) -> dict:
        """Checkpoint: the sums, the moments (or None) and the sample count as host numpy arrays / int."""
        return {"samples": self.samples, "sums": self.sums.cpu().numpy(),
                "moments": self.moments.cpu().numpy() if self.moments is not None else None}

    @classmethod
    def from_state(cls, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None,
                   state: dict, device=None) -> "Progressive":
        """Resume a checkpoint (state()) on this context -- any process, any GPU with the same scene uploaded."""
        import torch
        pg = cls(ctx, cam, nrows, ncols, max_depth, options, moments=state.get("moments") is not None, device=device)
        sums = np.ascontiguousarray(state["sums"], dtype=np.float64)
        if sums.shape != tuple(pg.sums.shape):
            raise TorError(ERR_INVALID_ARGUMENT, f"Progressive.from_state: sums of shape {sums.shape}, expected {tuple(pg.sums.shape)}")
        pg.sums.copy_(torch.from_numpy(sums))
        if pg.moments is not None:
            pg.moments.copy_(torch.from_numpy(np.ascontiguousarray(state["moments"], dtype=np.float64)))
        pg.samples = int(state["samples"])
        return pg


MAX_ACCUM_SAMPLES = 1 << 17  # exactness bound of the progressive sums (tor_render.h)


class Film:
    """The exact film for host-written integrators: owns the sums (and, where asked for, the second moments, the per-pixel counts)
    and the rejected counter of a whole nrows x ncols frame, filled by Context.deposit -- progressive, resumable, noise-driven and
    additive across GPUs like Progressive, whatever produced the colours.

        film = Film(ctx, 1080, 1920, moments=True, max_value=4.0)
        film.add_pass(cam, 16, tracer=lambda r, g: ctx.trace(r, g, emission=E)[0]); preview = film.image()

    With the default tracer (Context.radiance at max_depth) and max_value = 1, add_pass(cam, k) adds what Progressive.add(k) adds,
    bit for bit.  max_value clamps every channel (0 < max_value <= DEPOSIT_MAX_VALUE); the sums are exact while every pixel holds
    at most budget() accepted samples.  All device work runs on torch's current stream of the buffers' device."""

    def __init__(self, ctx: Context, nrows: int, ncols: int, moments: bool = False, counts: bool = False, max_value: float = 1.0,
                 device=None, max_depth: int = 50):
        import torch
        self.ctx, self.nrows, self.ncols, self.max_depth = ctx, int(nrows), int(ncols), int(max_depth)
        self.max_value = float(max_value)
        if not 0.0 < self.max_value <= DEPOSIT_MAX_VALUE:
            raise TorError(ERR_INVALID_ARGUMENT, f"Film: max_value must lie in (0, {DEPOSIT_MAX_VALUE:g}]")
        dev = torch.device("cuda") if device is None else torch.device(device)
        self.sums = torch.zeros((self.nrows, self.ncols, 3), dtype=torch.float64, device=dev)
        self.moments = torch.zeros_like(self.sums) if moments else None
        self.counts = torch.zeros((self.nrows, self.ncols), dtype=torch.int32, device=dev) if counts else None
        self._rejected = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.samples = 0       # samples per pixel of the uniform passes (add_pass)
        self.uniform = True    # only add_pass so far: every pixel holds `samples` samples

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.sums.device).cuda_stream

    def budget(self) -> int:
        """The most accepted samples a pixel may hold with exact sums: 2^17 / max(max_value, max_value^2)."""
        return int(MAX_ACCUM_SAMPLES / max(self.max_value, self.max_value * self.max_value))

    def deposit(self, pixels, colors, index=None) -> "Film":
        """Deposit arbitrary samples: colors (n, 3) float64 into the flat pixels (n,) row * ncols + col (splatting, light tracing).
        The pixels then hold unequal numbers of samples: image() needs counts=True (or the caller keeps `samples` right itself)."""
        import torch
        pixels = torch.as_tensor(pixels).to(device=self.sums.device, dtype=torch.int32).reshape(-1)
        self.ctx.deposit(colors, pixels, self.sums, self.moments, self.counts, index, self.max_value, self._rejected)
        self.uniform = False
        return self

    def add_pass(self, cam: Camera, k: int, tracer=None, chunk_pixels=None) -> "Film":
        """Samples [samples, samples + k) of every pixel: over ranges of at most chunk_pixels pixels the library's camera rays
        (Context.camera_rays, SEED_SAMPLE), colors = tracer(rays, rng) -- default Context.radiance at max_depth; a tracer may return
        a tuple whose first item is the colours -- and their deposit into pixel chunk[entry // k].  A textured frame:
        tracer=functools.partial(ctx.trace, max_depth=..., textures=True)."""
        import torch
        k = int(k)
        if k < 1:
            raise TorError(ERR_INVALID_ARGUMENT, "Film.add_pass: k must be >= 1")
        npix = self.nrows * self.ncols
        chunk_pixels = max(1, (1 << 22) // k) if chunk_pixels is None else int(chunk_pixels)
        if chunk_pixels < 1:
            raise TorError(ERR_INVALID_ARGUMENT, "Film.add_pass: chunk_pixels must be >= 1")
        if tracer is None:
            def tracer(rays, rng):
                return self.ctx.radiance(rays, rng, self.max_depth)
        dev = self.sums.device
        for a in range(0, npix, chunk_pixels):
            chunk = torch.arange(a, min(a + chunk_pixels, npix), dtype=torch.int32, device=dev)
            rays, rng = self.ctx.camera_rays(cam, self.nrows, self.ncols, first_sample=self.samples, n_samples=k, pixels=chunk)
            colors = tracer(rays, rng)
            if isinstance(colors, (tuple, list)):
                colors = colors[0]
            self.ctx.deposit(colors, chunk.repeat_interleave(k), self.sums, self.moments, self.counts, None, self.max_value,
                             self._rejected)
        self.samples += k
        return self

    def add_light_pass(self, cam: Camera, k: int, emission, diffuse, chunk_paths: int = 1 << 20, **kw) -> "Film":
        """A light-traced pass worth k samples per pixel: nrows * ncols * k light paths (Context.trace_light, kw its keywords),
        in chunks of at most chunk_paths, path p of the pass on the state rng_seed2(samples, p) -- `samples` before the pass
        numbers it --, every splat deposited (splat = self.deposit); then samples += k, so image() resolves sums / samples on a
        film without counts.  A light tracer's splats are small and many: the clamp max_value applies to each splat."""
        import torch
        k = int(k)
        if k < 1 or int(chunk_paths) < 1:
            raise TorError(ERR_INVALID_ARGUMENT, "Film.add_light_pass: k and chunk_paths must be >= 1")
        total = self.nrows * self.ncols * k
        for a in range(0, total, int(chunk_paths)):
            b = min(a + int(chunk_paths), total)
            st = rng_seed2(np.full(b - a, self.samples, dtype=np.uint64), np.arange(a, b, dtype=np.uint64))
            rng = torch.from_numpy(st.view(np.int64)).to(self.sums.device)
            self.ctx.trace_light(cam, self.nrows, self.ncols, rng, emission, diffuse, splat=self.deposit, **kw)
        self.samples += k
        return self

    def image(self, gamma: float = 2.2):
        """The gamma-corrected canvas so far, a new (nrows, ncols, 3) float64 device tensor: pow(sums / samples, 1 / gamma) after
        uniform passes (tor_resolve_device); with counts after deposit(), each pixel at its own count (tor_resolve_counts_device),
        a pixel without samples black."""
        import torch
        out = torch.empty_like(self.sums)
        if self.uniform or self.counts is None:
            self.ctx.resolve_device(self.sums.data_ptr(), self.sums.numel(), self.samples, gamma, out.data_ptr(), self._stream())
        else:
            counts = self.counts.clamp(min=1)   # a copy: count 0 resolves as count 1 (sums 0: black)
            self.ctx.resolve_counts_device(self.sums.data_ptr(), counts.data_ptr(), self.nrows * self.ncols, gamma, out.data_ptr(),
                                           self._stream())   # (same stream as the allocator's: `counts` may be dropped)
        return out

    def noise(self):
        """(mean, max) over the pixels of the largest per-channel standard error of the mean, as Progressive.noise.  Blocking."""
        if self.moments is None:
            raise TorError(ERR_INVALID_ARGUMENT, "Film.noise: created without moments=True")
        if not self.uniform:
            raise TorError(ERR_INVALID_ARGUMENT, "Film.noise: the pixels hold unequal numbers of samples (deposit() was used)")
        return self.ctx.accum_noise_device(self.sums.data_ptr(), self.moments.data_ptr(), self.nrows * self.ncols, self.samples, 0,
                                           self._stream())

    def rejected(self) -> int:
        """How many samples were rejected so far (a NaN, infinite or negative channel).  Blocking."""
        return int(self._rejected.item())

    def check_budget(self) -> int:
        """Raises when a pixel may hold more accepted samples than budget(), i.e. the sums may have stopped being exact:
        counts.max() after deposit() with counts, else `samples`.  Returns the number it checked.  Blocking."""
        n = int(self.counts.max().item()) if (self.counts is not None and not self.uniform) else self.samples
        if n > self.budget():
            raise TorError(ERR_INVALID_ARGUMENT, f"Film.check_budget: {n} samples in one pixel, above the exactness bound "
                                                 f"{self.budget()} of max_value = {self.max_value:g}")
        return n

    def state(self) -> dict:
        """Checkpoint: sizes, max_value, the sample count and every buffer as host numpy arrays."""
        return {"nrows": self.nrows, "ncols": self.ncols, "max_value": self.max_value, "max_depth": self.max_depth,
                "samples": self.samples, "uniform": self.uniform, "rejected": self.rejected(), "sums": self.sums.cpu().numpy(),
                "moments": self.moments.cpu().numpy() if self.moments is not None else None,
                "counts": self.counts.cpu().numpy() if self.counts is not None else None}

    @classmethod
    def from_state(cls, ctx: Context, state: dict, device=None) -> "Film":
        """Resume a checkpoint (state()) on this context -- any process, any GPU."""
        import torch
        film = cls(ctx, state["nrows"], state["ncols"], moments=state.get("moments") is not None,
                   counts=state.get("counts") is not None, max_value=state["max_value"], device=device,
                   max_depth=state.get("max_depth", 50))
        sums = np.ascontiguousarray(state["sums"], dtype=np.float64)
        if sums.shape != tuple(film.sums.shape):
            raise TorError(ERR_INVALID_ARGUMENT, f"Film.from_state: sums of shape {sums.shape}, expected {tuple(film.sums.shape)}")
        film.sums.copy_(torch.from_numpy(sums))
        if film.moments is not None:
            film.moments.copy_(torch.from_numpy(np.ascontiguousarray(state["moments"], dtype=np.float64)))
        if film.counts is not None:
            film.counts.copy_(torch.from_numpy(np.ascontiguousarray(state["counts"], dtype=np.int32)))
        film._rejected.fill_(int(state.get("rejected", 0)))
        film.samples, film.uniform = int(state["samples"]), bool(state.get("uniform", True))
        return film


class PixelProgressive(Progressive):
    """Progressive's surface on the REFERENCE's streams (TOR_SEED_PIXEL): owns, for this shard's rows, the per-pixel generator
    states, the raw sequential sums and (moments=True) the sequential sums of c * c.  After any sequence of add() calls totalling
    n samples, image() is the reference's n-spp canvas -- what a one-shot n-spp render_device(SEED_PIXEL) gives, bit for bit.

        pp = PixelProgressive(ctx, cam, 1080, 1920, 50, moments=True)
        pp.add(16); preview = pp.image(); pp.render_until(max_se=1e-3, max_samples=4096, pass_samples=128)

    Default options: TOR_SEED_PIXEL with both exact accelerations (tor_render()'s default).  The first add() starts the pixels, so
    no buffer needs clearing.  The context must have the scene uploaded; device work runs on torch's current stream."""

    _SEEDING = SEED_PIXEL
    _REFUSAL = ("PixelProgressive: needs TOR_SEED_PIXEL (it continues the reference's per-pixel "
                "streams); passes of TOR_SEED_SAMPLE streams are Progressive's")

    @staticmethod
    def _default_options() -> Options:
        return make_options(seeding=SEED_PIXEL, accel=ACCEL_BLOCKS | ACCEL_F32)

    def __init__(self, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None = None,
                 moments: bool = False, device=None):
        import torch
        super().__init__(ctx, cam, nrows, ncols, max_depth, options, moments, device)
        # one TorRng per pixel: the four xoshiro256+ words (held as int64 bit patterns; state() hands them out as uint64)
        self.rng = torch.zeros((self.rows, self.ncols, 4), dtype=torch.int64, device=self.sums.device)

    def add(self, n: int) -> "PixelProgressive":
        """Run the next n samples of every pixel's stream (asynchronous on the current stream)."""
        self.ctx.resume_device(self.cam, self.nrows, self.ncols, self.samples, int(n), self.max_depth, self.options,
                               self.rng.data_ptr(), self.sums.data_ptr(), self.moments.data_ptr() if self.moments is not None else 0,
                               self._stream())
        self.samples += int(n)
        return self

    def state(self) -> dict:
        """Checkpoint: Progressive.state() plus the per-pixel generator states as a (rows, ncols, 4) uint64 array."""
        st = super().state()
        st["rng"] = self.rng.cpu().numpy().view(np.uint64)
        return st

    @classmethod
    def from_state(cls, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None,
                   state: dict, device=None) -> "PixelProgressive":
        """Resume a checkpoint (state()) on this context -- any process, any GPU with the same scene uploaded."""
        import torch
        rng = np.asarray(state.get("rng"))
        pp = cls(ctx, cam, nrows, ncols, max_depth, options, moments=state.get("moments") is not None, device=device)
        if rng.dtype != np.uint64 or rng.shape != tuple(pp.rng.shape):
            raise TorError(ERR_INVALID_ARGUMENT, f"PixelProgressive.from_state: generator states of dtype {rng.dtype}, shape {rng.shape}; "
                                                 f"expected uint64 {tuple(pp.rng.shape)}")
        sums = np.ascontiguousarray(state["sums"], dtype=np.float64)
        if sums.shape != tuple(pp.sums.shape):
            raise TorError(ERR_INVALID_ARGUMENT, f"PixelProgressive.from_state: sums of shape {sums.shape}, expected {tuple(pp.sums.shape)}")
        pp.sums.copy_(torch.from_numpy(sums))
        if pp.moments is not None:
            mom = np.ascontiguousarray(state["moments"], dtype=np.float64)
            if mom.shape != tuple(pp.moments.shape):
                raise TorError(ERR_INVALID_ARGUMENT, f"PixelProgressive.from_state: moments of shape {mom.shape}, expected {tuple(pp.moments.shape)}")
            pp.moments.copy_(torch.from_numpy(mom))
        pp.rng.copy_(torch.from_numpy(np.ascontiguousarray(rng).view(np.int64)))
        pp.samples = int(state["samples"])
        return pp


def adaptive_select_host(sums, moments, pixels, n: int, abs_tol: float, rel_tol: float) -> np.ndarray:
    """tor_adaptive_select_device restated in numpy float64 (same operations, one rounding each): the entries of `pixels` (indices
    into sums / moments viewed as (npix, 3)) that have NOT converged at n samples, in input order."""
    S = np.asarray(sums, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(moments, dtype=np.float64).reshape(-1, 3)
    pix = np.asarray(pixels, dtype=np.int64)
    S, M, n = S[pix], M[pix], np.float64(n)
    mean = S / n
    var = (M - S * S / n) / (n - np.float64(1.0))
    var = np.where(var > 0.0, var, 0.0)
    se = np.sqrt(var / n)
    converged = np.all(se <= np.float64(abs_tol) + np.float64(rel_tol) * mean, axis=1)
    return pix[~converged].astype(np.int32)


class Adaptive:
    """Adaptive sampling of one (camera, size, depth, options) in TOR_SEED_SAMPLE mode: passes of pass_samples over the ACTIVE LIST
    of pixels that have not converged yet.  All pixels start on the list; once N >= min_samples a select after each pass drops every
    pixel whose per-channel standard error is <= abs_tol + rel_tol * mean (tor_render.h).  Each pixel's samples are the prefix
    [0, counts[p]), so pixel p of image() is pixel p of a uniform counts[p]-spp render, bit for bit.

        ad = Adaptive(ctx, cam, 1080, 1920, 50, make_options(seeding=SEED_SAMPLE), rel_tol=0.05)
        ad.run(); frame = ad.image(); spp_map = ad.counts()

    The context must have the scene uploaded; all device work runs on torch's current stream of the buffers' device."""

    # what a subclass on other streams changes (PixelAdaptive): the seeding it needs, its refusal, its default options, its pass
    _SEEDING = SEED_SAMPLE
    _REFUSAL = ("Adaptive: needs TOR_SEED_SAMPLE (adaptive sampling on the reference's TOR_SEED_PIXEL streams "
                "is PixelAdaptive's)")

    @staticmethod
    def _default_options() -> Options:
        return make_options(seeding=SEED_SAMPLE)

    def __init__(self, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None = None,
                 abs_tol: float = 0.0, rel_tol: float = 0.05, min_samples: int = 16, pass_samples: int = 16, max_samples: int = 4096,
                 device=None):
        self.ctx, self.nrows, self.ncols, self.max_depth = ctx, int(nrows), int(ncols), int(max_depth)
        self.cam = Camera.from_buffer_copy(cam)
        self.options = Options.from_buffer_copy(options if options is not None else self._default_options())
        if self.options.seeding != self._SEEDING:
            raise TorError(ERR_INVALID_ARGUMENT, self._REFUSAL)
        self.abs_tol, self.rel_tol = float(abs_tol), float(rel_tol)
        if not (self.abs_tol >= 0.0 and self.rel_tol >= 0.0):
            raise TorError(ERR_INVALID_ARGUMENT, f"{type(self).__name__}: abs_tol and rel_tol must be >= 0 (and not NaN)")
        self.min_samples, self.pass_samples, self.max_samples = int(min_samples), int(pass_samples), int(max_samples)
        if self.min_samples < 2 or self.pass_samples < 1 or not 1 <= self.max_samples <= MAX_ACCUM_SAMPLES:
            raise TorError(ERR_INVALID_ARGUMENT, f"{type(self).__name__}: need min_samples >= 2 (the variance needs two samples), "
                                                 "pass_samples >= 1 and 1 <= max_samples <= 2^17")
        self.rows = self._shard_rows(self.nrows, self.options)
        self.npix = self.rows * self.ncols
        self._alloc(device)

    @staticmethod
    def _shard_rows(nrows: int, options: Options) -> int:
        return len(shard_rows(int(nrows), max(int(options.row_tile), 1), int(options.shard_index), max(int(options.shard_count), 1)))

    def _alloc(self, device) -> None:
        import torch
        dev = torch.device("cuda") if device is None else torch.device(device)
        self.sums = torch.zeros((self.rows, self.ncols, 3), dtype=torch.float64, device=dev)
        self.moments = torch.zeros_like(self.sums)
        self._counts = torch.zeros((self.rows, self.ncols), dtype=torch.int32, device=dev)
        self._list = torch.arange(self.npix, dtype=torch.int32, device=dev)  # the active list is _list[:active]
        self._spare = torch.empty_like(self._list)
        self.active = self.npix
        self.samples = 0

    @staticmethod
    def validate_list(pixels, npix: int) -> np.ndarray:
        """A host-supplied active list as int32: strictly ascending (hence unique) shard-local pixel indices in [0, npix)."""
        a = np.asarray(pixels)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise TorError(ERR_INVALID_ARGUMENT, "Adaptive: a pixel list is a 1-D array of integers")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= npix):
            raise TorError(ERR_INVALID_ARGUMENT, f"Adaptive: pixel list entries must lie in [0, {npix})")
        if a.size > 1 and not np.all(np.diff(a) > 0):
            raise TorError(ERR_INVALID_ARGUMENT, "Adaptive: a pixel list must be strictly ascending (no duplicates)")
        return a.astype(np.int32)

    def _stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.sums.device).cuda_stream

    def step(self) -> "Adaptive":
        """One pass of pass_samples (shortened to land on max_samples) over the active list, then -- once N >= min_samples -- the
        select that drops the converged pixels.  A no-op when the list is empty or max_samples is reached."""
        k = min(self.pass_samples, self.max_samples - self.samples)
        if self.active == 0 or k <= 0:
            return self
        st = self._stream()
        self._pass(k, st)
        self.samples += k
        if self.samples >= self.min_samples:
            n = self.ctx.adaptive_select_device(self.sums.data_ptr(), self.moments.data_ptr(), self._list.data_ptr(), self.active,
                                                self.samples, self.abs_tol, self.rel_tol, self._spare.data_ptr(),
                                                self._counts.data_ptr(), st)
            self._list, self._spare = self._spare, self._list
            self.active = n
        else:  # (no select yet: every listed pixel simply has N samples)
            self._counts.view(-1).index_fill_(0, self._list[: self.active].long(), self.samples)
        return self

    def _pass(self, k: int, stream: int) -> None:
        """Samples [N, N + k) of the active list's pixels."""
        self.ctx.accumulate_list_device(self.cam, self.nrows, self.ncols, self._list.data_ptr(), self.active, self.samples, k,
                                        self.max_depth, self.options, self.sums.data_ptr(), self.moments.data_ptr(), stream)

    def run(self) -> int:
        """step() until the list is empty or max_samples is reached; the survivors then hold max_samples.  Returns N."""
        while self.active > 0 and self.samples < self.max_samples:
            self.step()
        return self.samples

    def counts(self):
        """The sample map: a device int32 tensor (rows of this shard, ncols)."""
        return self._counts.clone()

    def active_list(self):
        """The active list (device int32, ascending)."""
        return self._list[: self.active].clone()

    def total_samples(self) -> int:
        """Samples spent over the frame (the sum of counts())."""
        import torch
        return int(self._counts.sum(dtype=torch.int64).item())

    def image(self, gamma: float = 2.2):
        """Each pixel resolved at its own count: a new device float64 tensor (rows of this shard, ncols, 3)."""
        import torch
        if self.samples == 0:
            raise TorError(ERR_INVALID_ARGUMENT, f"{type(self).__name__}.image: no pass has run yet")
        out = torch.empty_like(self.sums)
        self.ctx.resolve_counts_device(self.sums.data_ptr(), self._counts.data_ptr(), self.npix, gamma, out.data_ptr(), self._stream())
        return out

    def to_canvas(self, canvas: Canvas) -> Canvas:
        """Fill a host Canvas (whole frame, unsharded options) with image(canvas.gamma_correction), so export_ppm works.  Its
        samples_per_pixel is N, the largest count."""
        if (canvas.nrows, canvas.ncols) != (self.rows, self.ncols):
            raise TorError(ERR_INVALID_ARGUMENT, f"{type(self).__name__}.to_canvas: the canvas must have this render's rows and columns")
        canvas.pixels[...] = self.image(canvas.gamma_correction).cpu().numpy()
        canvas.samples_per_pixel = self.samples
        return canvas

    def state(self) -> dict:
        """Checkpoint: N, the sums, moments, counts and the active list as host numpy arrays / int."""
        return {"samples": self.samples, "sums": self.sums.cpu().numpy(), "moments": self.moments.cpu().numpy(),
                "counts": self._counts.cpu().numpy(), "list": self._list[: self.active].cpu().numpy()}

    @classmethod
    def from_state(cls, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None, state: dict,
                   device=None, **policy) -> "Adaptive":
        """Resume a checkpoint (state()) on this context -- any process, any GPU with the same scene uploaded.  policy: the
        constructor's abs_tol, rel_tol, min_samples, pass_samples, max_samples."""
        import torch
        opts = options if options is not None else cls._default_options()
        npix = cls._shard_rows(nrows, opts) * int(ncols)
        lst = cls.validate_list(state["list"], npix)  # before any device work
        ad = cls(ctx, cam, nrows, ncols, max_depth, options, device=device, **policy)
        arrays = {"sums": (ad.sums, np.float64), "moments": (ad.moments, np.float64), "counts": (ad._counts, np.int32)}
        for key, (dst, dt) in arrays.items():
            a = np.ascontiguousarray(state[key], dtype=dt)
            if a.shape != tuple(dst.shape):
                raise TorError(ERR_INVALID_ARGUMENT, f"{cls.__name__}.from_state: {key} of shape {a.shape}, expected {tuple(dst.shape)}")
            dst.copy_(torch.from_numpy(a))
        ad.samples = int(state["samples"])
        if lst.size and not np.all(np.asarray(state["counts"]).reshape(-1)[lst] == ad.samples):
            raise TorError(ERR_INVALID_ARGUMENT, f"{cls.__name__}.from_state: every listed pixel must hold exactly N samples")
        ad._list[: lst.size].copy_(torch.from_numpy(lst))
        ad.active = int(lst.size)
        return ad


class PixelAdaptive(Adaptive):
    """Adaptive's surface on the REFERENCE's streams (TOR_SEED_PIXEL): owns, for this shard's rows, the per-pixel generator states
    next to the raw sequential sums, the sums of c * c, the counts and the active list.  A pass runs the next pass_samples samples
    of the LISTED pixels' own streams; a pixel that left the list keeps every bit of its state.  Pixel p of image() is the
    reference's pixel p at counts[p] samples per pixel -- what a one-shot counts[p]-spp render_device(SEED_PIXEL) gives there,
    bit for bit, whatever the schedule, accel and pixel_kernel.

        ad = PixelAdaptive(ctx, cam, 1080, 1920, 50, rel_tol=0.05, max_samples=1024)
        ad.run(); frame = ad.image(); spp_map = ad.counts()

    Default options: TOR_SEED_PIXEL with both exact accelerations (tor_render()'s default).  The first pass starts the pixels, so
    no buffer needs clearing.  The context must have the scene uploaded; device work runs on torch's current stream."""

    _SEEDING = SEED_PIXEL
    _REFUSAL = ("PixelAdaptive: needs TOR_SEED_PIXEL (it continues the reference's per-pixel streams); "
                "adaptive sampling on TOR_SEED_SAMPLE streams is Adaptive's")

    @staticmethod
    def _default_options() -> Options:
        return make_options(seeding=SEED_PIXEL, accel=ACCEL_BLOCKS | ACCEL_F32)

    def _alloc(self, device) -> None:
        import torch
        super()._alloc(device)
        # one TorRng per pixel: the four xoshiro256+ words (held as int64 bit patterns; state() hands them out as uint64)
        self.rng = torch.zeros((self.rows, self.ncols, 4), dtype=torch.int64, device=self.sums.device)

    def _pass(self, k: int, stream: int) -> None:
        """Samples [N, N + k) of the listed pixels' own streams (N == 0 starts them)."""
        self.ctx.resume_list_device(self.cam, self.nrows, self.ncols, self._list.data_ptr(), self.active, self.samples, k,
                                    self.max_depth, self.options, self.rng.data_ptr(), self.sums.data_ptr(), self.moments.data_ptr(),
                                    stream)

    def state(self) -> dict:
        """Checkpoint: Adaptive.state() plus the per-pixel generator states as a (rows, ncols, 4) uint64 array."""
        st = super().state()
        st["rng"] = self.rng.cpu().numpy().view(np.uint64)
        return st

    @classmethod
    def from_state(cls, ctx: Context, cam: Camera, nrows: int, ncols: int, max_depth: int, options: Options | None, state: dict,
                   device=None, **policy) -> "PixelAdaptive":
        """Resume a checkpoint (state()) on this context -- any process, any GPU with the same scene uploaded.  policy: the
        constructor's abs_tol, rel_tol, min_samples, pass_samples, max_samples."""
        import torch
        opts = options if options is not None else cls._default_options()
        want = (cls._shard_rows(nrows, opts), int(ncols), 4)
        rng = np.asarray(state.get("rng"))
        if rng.dtype != np.uint64 or rng.shape != want:  # before any device work
            raise TorError(ERR_INVALID_ARGUMENT, f"PixelAdaptive.from_state: generator states of dtype {rng.dtype}, shape {rng.shape}; "
                                                 f"expected uint64 {want}")
        ad = super().from_state(ctx, cam, nrows, ncols, max_depth, options, state, device=device, **policy)
        ad.rng.copy_(torch.from_numpy(np.ascontiguousarray(rng).view(np.int64)))
        return ad


def mp4_mux_file(src_annexb_path: str, dst_mp4_path: str, width: int, height: int, fps: int = 30) -> int:
    """MP4Muxer (io/mp4.nim:113-163): Annex-B .264 -> .mp4; returns the number of samples."""
    n = lib().tor_mp4_mux_file(os.fsencode(src_annexb_path), os.fsencode(dst_mp4_path), width, height, fps)
    if n < 0:
        raise TorError(n, lib().tor_last_error().decode())
    return n


def debug_accel_layout(world: HittableList, t_lo: float, t_hi: float):
    """(slot_object[n_blocks, 8], block_boxes[n_blocks_padded, 6], super_boxes[n, 6], two_level) or None."""
    cap = int(world.len) + 64
    slots = np.full(cap, -1, dtype=np.int64)
    boxes = np.zeros((cap // 8 + 16, 6), dtype=np.float64)
    supers = np.zeros((cap // 64 + 16, 6), dtype=np.float64)
    two = C.c_int32(0)
    n = lib().tor_debug_accel_layout(world, t_lo, t_hi, slots.ctypes.data_as(C.POINTER(C.c_int64)), cap,
                                     boxes.ctypes.data_as(C.POINTER(C.c_double)),
                                     supers.ctypes.data_as(C.POINTER(C.c_double)), boxes.shape[0], C.byref(two))
    if n < 0:
        raise TorError(n, "tor_debug_accel_layout failed")
    if n == 0:
        return None
    n_p = (n + 7) // 8 * 8
    return slots[: n * 8].reshape(n, 8), boxes[:n_p], supers[: n_p // 8], bool(two.value)


def selftest_filter32(o, d, c0, dc, moving, f, r2, origin):
    """(keep, need) int32 arrays: host build of the TOR_ACCEL_F32 pre-filter vs the float64 test."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, c0, dc, f, r2, origin = dp(o), dp(d), dp(c0), dp(dc), dp(f), dp(r2), dp(origin)
    moving = np.ascontiguousarray(moving, dtype=np.int32)
    n = len(f)
    keep = np.zeros(n, dtype=np.int32)
    need = np.zeros(n, dtype=np.int32)
    P = C.POINTER(C.c_double)
    I = C.POINTER(C.c_int32)
    _check(lib().tor_selftest_filter32_host(n, o.ctypes.data_as(P), d.ctypes.data_as(P), c0.ctypes.data_as(P),
                                            dc.ctypes.data_as(P), moving.ctypes.data_as(I), f.ctypes.data_as(P),
                                            r2.ctypes.data_as(P), origin.ctypes.data_as(P), keep.ctypes.data_as(I),
                                            need.ctypes.data_as(I)))
    return keep, need


def selftest_screen(o, d, c0, dc, moving, f, r2):
    """(keep, need) int32 arrays: host build of the strict object loop's conservative FMA screen vs the reference's test."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, c0, dc, f, r2 = dp(o), dp(d), dp(c0), dp(dc), dp(f), dp(r2)
    moving = np.ascontiguousarray(moving, dtype=np.int32)
    n = len(f)
    keep = np.zeros(n, dtype=np.int32)
    need = np.zeros(n, dtype=np.int32)
    P = C.POINTER(C.c_double)
    I = C.POINTER(C.c_int32)
    _check(lib().tor_selftest_screen_host(n, o.ctypes.data_as(P), d.ctypes.data_as(P), c0.ctypes.data_as(P), dc.ctypes.data_as(P),
                                          moving.ctypes.data_as(I), f.ctypes.data_as(P), r2.ctypes.data_as(P), keep.ctypes.data_as(I),
                                          need.ctypes.data_as(I)))
    return keep, need


def selftest_screen2(o, d, c0, dc, moving, f, r2, variant=0):
    """(keep, need): the screen's second form (expanded quadratic, normalised direction) on the host; variant 1 routes static
    spheres through the common-height record."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, c0, dc, f, r2 = dp(o), dp(d), dp(c0), dp(dc), dp(f), dp(r2)
    moving = np.ascontiguousarray(moving, dtype=np.int32)
    n = len(f)
    keep = np.zeros(n, dtype=np.int32)
    need = np.zeros(n, dtype=np.int32)
    P = C.POINTER(C.c_double)
    I = C.POINTER(C.c_int32)
    _check(lib().tor_selftest_screen2_host(n, o.ctypes.data_as(P), d.ctypes.data_as(P), c0.ctypes.data_as(P), dc.ctypes.data_as(P),
                                           moving.ctypes.data_as(I), f.ctypes.data_as(P), r2.ctypes.data_as(P), int(variant),
                                           keep.ctypes.data_as(I), need.ctypes.data_as(I)))
    return keep, need


def selftest_slab32(o, d, lo, hi, origin):
    """(keep, need) int32 arrays: host build of the float32 box test vs the float64 slab test."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, lo, hi, origin = dp(o), dp(d), dp(lo), dp(hi), dp(origin)
    n = len(o)
    keep = np.zeros(n, dtype=np.int32)
    need = np.zeros(n, dtype=np.int32)
    P = C.POINTER(C.c_double)
    I = C.POINTER(C.c_int32)
    _check(lib().tor_selftest_slab32_host(n, o.ctypes.data_as(P), d.ctypes.data_as(P), lo.ctypes.data_as(P), hi.ctypes.data_as(P),
                                          origin.ctypes.data_as(P), keep.ctypes.data_as(I), need.ctypes.data_as(I)))
    return keep, need


def debug_filter32_scene(world: HittableList, o, d, time):
    """keep[n_rays, n_objects] int8 (1 kept, 0 dropped, 2 float64 loop): the TOR_ACCEL_F32 segment walk on the host."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, time = dp(o), dp(d), dp(time)
    keep = np.zeros((len(time), int(world.len)), dtype=np.int8)
    P = C.POINTER(C.c_double)
    _check(lib().tor_debug_filter32_scene(world, len(time), o.ctypes.data_as(P), d.ctypes.data_as(P), time.ctypes.data_as(P),
                                          keep.ctypes.data_as(C.POINTER(C.c_int8))))
    return keep


def debug_layout_segments(world: HittableList, max_segs: int = 64):
    """[(xkind, objects, slots, first slot), ...]: the float64 layout's segments in the order the kernel walks them (host only)."""
    out = np.zeros((max_segs, 4), dtype=np.int32)
    n = C.c_int64(0)
    _check(lib().tor_debug_layout_segments(world, out.ctypes.data_as(C.POINTER(C.c_int32)), max_segs, C.byref(n)))
    return [tuple(int(v) for v in row) for row in out[:min(int(n.value), max_segs)]]


def debug_screen2_scene(world: HittableList, o, d, time, max_segs: int = 0):
    """(keep[n_rays, n_objects] int8, kind[n_objects] int32 [, pays[n_rays, max_segs] int8]): the strict layout's screened
    segments walked on the host -- 0 dropped by the plane screen, 1 dropped by stage two, 2 candidate, 3 no plane table; kind
    0 | 10..14; pays (with max_segs > 0): the rays' votes for stage one per segment (plane_pays)."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, time = dp(o), dp(d), dp(time)
    keep = np.zeros((len(time), int(world.len)), dtype=np.int8)
    kind = np.zeros(int(world.len), dtype=np.int32)
    pays = np.full((len(time), max(max_segs, 1)), -1, dtype=np.int8)
    P = C.POINTER(C.c_double)
    _check(lib().tor_debug_screen2_scene(world, len(time), o.ctypes.data_as(P), d.ctypes.data_as(P), time.ctypes.data_as(P),
                                         keep.ctypes.data_as(C.POINTER(C.c_int8)), kind.ctypes.data_as(C.POINTER(C.c_int32)),
                                         pays.ctypes.data_as(C.POINTER(C.c_int8)) if max_segs > 0 else None, max_segs))
    return (keep, kind, pays) if max_segs > 0 else (keep, kind)


def debug_plane32_scene(world: HittableList, o, d, time):
    """(keep[n_rays, n_objects] int8, pad_kept[n_rays] int32, n_pad): stage one of the plane-screened segments of xkind 10 / 11 /
    12 / 14 in float64 and in float32 on the host -- bit 0 of keep: the float64 screen keeps the object, bit 1: the float32 one;
    -1: the object is not on such a segment.  pad_kept: padding slots the float32 screen keeps, of n_pad."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, time = dp(o), dp(d), dp(time)
    keep = np.zeros((len(time), int(world.len)), dtype=np.int8)
    pad_kept = np.zeros(len(time), dtype=np.int32)
    n_pad = C.c_int64(0)
    P = C.POINTER(C.c_double)
    _check(lib().tor_debug_plane32_scene(world, len(time), o.ctypes.data_as(P), d.ctypes.data_as(P), time.ctypes.data_as(P),
                                         keep.ctypes.data_as(C.POINTER(C.c_int8)), pad_kept.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(n_pad)))
    return keep, pad_kept, int(n_pad.value)


def debug_reach_scene(world: HittableList, o, d, time):
    """(reach[n_rays, n_objects] int8, word[n_objects] int32, slot[n_objects] int32, boxes[n_words, 6] float64): the reach pass in
    front of the plane screen's whole words on the host (include/tor_reach.h) -- reach 0: the ray does not reach the boxed word of
    the object's slot, 1: it does, or the word carries no box; word: the object's word of the sorted list when it carries a box,
    else -1; slot: its slot; boxes: {xlo, xhi, zlo, zhi, ylo, yhi} per word in absolute coordinates (-inf, +inf: no box)."""
    dp = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    o, d, time = dp(o), dp(d), dp(time)
    n_obj = int(world.len)
    reach = np.zeros((len(time), n_obj), dtype=np.int8)
    word = np.zeros(n_obj, dtype=np.int32)
    slot = np.zeros(n_obj, dtype=np.int32)
    max_words = (n_obj + 31) // 32 + 8 * 64   # (every segment pads by less than a word; there are few of them)
    boxes = np.zeros((max_words, 6), dtype=np.float64)
    n_words = C.c_int64(0)
    P, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _check(lib().tor_debug_reach_scene(world, len(time), o.ctypes.data_as(P), d.ctypes.data_as(P), time.ctypes.data_as(P),
                                       reach.ctypes.data_as(C.POINTER(C.c_int8)), word.ctypes.data_as(I), slot.ctypes.data_as(I),
                                       boxes.ctypes.data_as(P), max_words, C.byref(n_words)))
    return reach, word, slot, boxes[:min(int(n_words.value), max_words)]


def selftest_math(op: int, x: np.ndarray, y: np.ndarray | None = None, where: str = "device", device: int = -1):
    """Run the kernel's math routines on arrays (op: 0 sincos, 1 x^5, 2 pow, 3 sqrt, 4 div, 5 quantize)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    yy = np.ascontiguousarray(y, dtype=np.float64) if y is not None else None
    o0 = np.zeros_like(x)
    o1 = np.zeros_like(x)
    dp = C.POINTER(C.c_double)
    yp = yy.ctypes.data_as(dp) if yy is not None else None
    if where == "device":
        _check(lib().tor_selftest_math_device(op, x.ctypes.data_as(dp), yp, o0.ctypes.data_as(dp),
                                              o1.ctypes.data_as(dp), x.size, device))
    else:
        _check(lib().tor_selftest_math_host(op, x.ctypes.data_as(dp), yp, o0.ctypes.data_as(dp),
                                            o1.ctypes.data_as(dp), x.size))
    return o0, o1


def selftest_rng(mode: int, a: int, b: int = 0, c: int = 0, n: int = 4):
    state = (C.c_uint64 * 4)()
    draws = (C.c_uint64 * max(n, 1))()
    _check(lib().tor_selftest_rng_host(mode, a, b, c, state, draws, n))
    return [int(v) for v in state], [int(v) for v in draws[:n]]


# Context.trace .. Context.trace_media: the functions of integrators.py as methods (last: that module imports this one's names)
from . import integrators   # noqa: E402

for _name in integrators.INTEGRATORS:
    setattr(Context, _name, getattr(integrators, _name))
