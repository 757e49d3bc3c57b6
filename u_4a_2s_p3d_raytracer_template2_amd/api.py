"""ctypes binding of libp3d_hip.so (include/p3d_hip.h + the p3dh_* host shim)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# P3D_LIB: an alternative build of the same library (tuning experiments under tools/ only)
LIB_PATH = os.environ.get("P3D_LIB") or os.path.join(_PKG, "libp3d_hip.so")

ACCEL_NONE, ACCEL_GRID, ACCEL_BVH = 0, 1, 2
FLAG_COUNTERS = 1
FLAG_TREE_KERNEL = 2
FLAG_NO_LDS_SCENE = 4
FLAG_PRIVATE_WALK = 8
FLAG_PROFILE = 16
FLAG_WAVEFRONT = 32
FLAG_TILE_KERNEL = 64
FLAG_DEVICE_SAMPLES = 128
FLAG_PACKET_WALK = 256
FEATURE_SOFT_SHADOW, FEATURE_FUZZY_REFLECTION, FEATURE_SKYBOX = 1, 2, 4
FEATURE_SCHLICK = 8          # the reference's SCHLICK_APPROX (RT/main.cpp:99), bit-exact
# p3d_generate_samples: pairs of draws one device thread reads, and threads (chunks) per workgroup -- kSampleChunkPairs and
# kSampleChunkThreads of csrc/sample_stream.h (tests/test_rand_port.py keeps them equal); tests size their shapes from these
SAMPLE_CHUNK_PAIRS, SAMPLE_WORKGROUP_CHUNKS = 496, 128


class P3DError(RuntimeError):
    pass


class SceneDesc(C.Structure):
    _fields_ = [("n_prims", C.c_uint32), ("prim_type", C.POINTER(C.c_uint32)),
                ("prim_data", C.POINTER(C.c_float)), ("prim_material", C.POINTER(C.c_uint32)),
                ("n_materials", C.c_uint32), ("materials", C.POINTER(C.c_float)),
                ("n_lights", C.c_uint32), ("lights", C.POINTER(C.c_float)),
                ("background", C.c_float * 3)]


class BuildOpts(C.Structure):
    _fields_ = [("leaf_max", C.c_uint32), ("sah_bins", C.c_uint32), ("builder", C.c_uint32), ("cull_never_hit", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("n", C.c_float * 3),
                ("w", C.c_float), ("h", C.c_float), ("plane_dist", C.c_float), ("aperture", C.c_float),
                ("focal_ratio", C.c_float), ("res_x", C.c_int32), ("res_y", C.c_int32)]


class RenderParams(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("accel", C.c_int32), ("spp", C.c_int32),
                ("samples", C.POINTER(C.c_float)), ("row_block", C.c_int32), ("rank", C.c_int32),
                ("world", C.c_int32), ("flags", C.c_uint32), ("features", C.c_uint32), ("seed", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("closest_queries", "shadow_queries", "box_tests", "sphere_tests",
                                          "tri_tests", "aabox_tests", "plane_tests", "pixels")]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_}
        d["rays"] = d["closest_queries"] + d["shadow_queries"]
        # SURVEY §8d algorithmic bytes, without the per-pixel output term
        d["algorithmic_bytes"] = (32 * d["box_tests"] + 16 * d["sphere_tests"] + 48 * d["tri_tests"] +
                                  32 * d["aabox_tests"] + 16 * d["plane_tests"])
        return d


class Outputs(C.Structure):
    _fields_ = [("rgb8", C.c_void_p), ("rgb32f", C.c_void_p), ("hit_id", C.c_void_p), ("memory", C.c_int32)]


class AovOutputs(C.Structure):
    """p3d_aov_outputs: depth [rows][W], normal and albedo [rows][W][3] floats; every plane may be NULL; host or device
    memory as the p3d_outputs of the same call says."""
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p)]


class Rays(C.Structure):
    """p3d_rays: n rays, origin / dir [n][3] floats on the host (memory 0) or the scene's device (memory 1)."""
    _fields_ = [("n", C.c_uint32), ("origin", C.c_void_p), ("dir", C.c_void_p), ("memory", C.c_int32)]


class RayOutputs(C.Structure):
    """p3d_ray_outputs: every plane may be NULL."""
    _fields_ = [("rgb32f", C.c_void_p), ("hit_id", C.c_void_p), ("t", C.c_void_p), ("normal", C.c_void_p),
                ("memory", C.c_int32)]


class OcclusionOutputs(C.Structure):
    """p3d_occlusion_outputs: occluded [n] bytes (may be NULL: the call then only validates), host or device memory."""
    _fields_ = [("occluded", C.c_void_p), ("memory", C.c_int32)]


class DenoiseParams(C.Structure):
    """p3d_denoise_params: n_frames frames of res_x x res_y back to back, iterations 0..6 passes, the three sigmas
    (sigma_color 0: no colour stop) and normal_power_log2 0..8 squarings of the normal weight."""
    _fields_ = [("res_x", C.c_int32), ("res_y", C.c_int32), ("n_frames", C.c_int32), ("iterations", C.c_int32),
                ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float), ("sigma_color", C.c_float),
                ("normal_power_log2", C.c_int32)]


class DenoiseInputs(C.Structure):
    """p3d_denoise_inputs: the colour and the AOV planes of p3d_render_aov, on the host (memory 0) or the scene's device (1)."""
    _fields_ = [("rgb32f", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("memory", C.c_int32)]


class DenoiseVarianceInputs(C.Structure):
    """p3d_denoise_variance_inputs: p3d_denoise_inputs' planes and the variance plane [n][H][W] that steers the colour stop."""
    _fields_ = [("rgb32f", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("variance", C.c_void_p),
                ("memory", C.c_int32)]


class DenoiseVarianceOutputs(C.Structure):
    """p3d_denoise_variance_outputs: each plane may be NULL."""
    _fields_ = [("rgb8", C.c_void_p), ("rgb32f", C.c_void_p), ("variance", C.c_void_p), ("memory", C.c_int32)]


# p3d_denoise's defaults (DESIGN "Denoising" says how they were chosen)
DENOISE_ITERATIONS = 4
DENOISE_SIGMA_DEPTH = 0.05
DENOISE_SIGMA_ALBEDO = 0.25
DENOISE_SIGMA_COLOR = 0.15
DENOISE_NORMAL_POWER_LOG2 = 5
# the defaults of p3d_accumulate_variance and p3d_denoise_variance (DESIGN "Variance-guided denoising" says how they were
# chosen): the history below which a pixel's variance is estimated from its neighbours, that neighbourhood's radius, and the
# colour stop's width in standard deviations; sigma_depth and normal_power_log2 are the denoiser's
VARIANCE_MIN_TEMPORAL = 4.0
VARIANCE_RADIUS = 3
VARIANCE_SIGMA_COLOR = 4.0
VARIANCE_SIGMA_DEPTH = DENOISE_SIGMA_DEPTH
VARIANCE_NORMAL_POWER_LOG2 = DENOISE_NORMAL_POWER_LOG2


class AccumulateParams(C.Structure):
    """p3d_accumulate_params: a sequence of n_frames frames of res_x x res_y back to back; the relative depth tolerance, the
    least normal agreement and the cap of the history length."""
    _fields_ = [("res_x", C.c_int32), ("res_y", C.c_int32), ("n_frames", C.c_int32), ("depth_tolerance", C.c_float),
                ("normal_min", C.c_float), ("max_history", C.c_float)]


class AccumulateFrames(C.Structure):
    """p3d_accumulate_frames: colour, depth, normal and (optionally) hit_id of the frames, on the host (memory 0) or the scene's
    device (1), and their cameras, always on the host."""
    _fields_ = [("rgb32f", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("hit_id", C.c_void_p),
                ("cams", C.POINTER(Camera)), ("memory", C.c_int32)]


class AccumulateHistory(C.Structure):
    """p3d_accumulate_history: what frame 0 looks back at -- one frame of accumulated colour and length, the depth, normal and
    (optionally) hit_id they were rendered with, and that frame's camera (host)."""
    _fields_ = [("rgb32f", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("length", C.c_void_p), ("hit_id", C.c_void_p),
                ("cam", C.POINTER(Camera)), ("memory", C.c_int32)]


class AccumulateOutputs(C.Structure):
    _fields_ = [("rgb32f", C.c_void_p), ("length", C.c_void_p), ("memory", C.c_int32)]


class AccumulateMotion(C.Structure):
    """p3d_accumulate_motion: the kinds of n_prims primitives, the [n_frames][n_prims][12] records the frames were rendered with
    and the [n_prims][12] records the history was rendered with (the form DeviceScene.update takes), host (memory 0) or device (1)."""
    _fields_ = [("n_prims", C.c_uint32), ("prim_type", C.c_void_p), ("prim_data", C.c_void_p), ("history_prim_data", C.c_void_p),
                ("memory", C.c_int32)]


class AccumulateMovingOutputs(C.Structure):
    _fields_ = [("rgb32f", C.c_void_p), ("length", C.c_void_p), ("prev_xy", C.c_void_p), ("memory", C.c_int32)]


class AccumulateVarianceParams(C.Structure):
    """p3d_accumulate_variance_params: pixels with a history shorter than min_temporal take the spatial estimate over
    (2 radius + 1)^2 neighbours, weighted by the denoiser's depth and normal stops."""
    _fields_ = [("min_temporal", C.c_float), ("radius", C.c_int32), ("sigma_depth", C.c_float), ("normal_power_log2", C.c_int32)]


class AccumulateVarianceOutputs(C.Structure):
    _fields_ = [("rgb32f", C.c_void_p), ("length", C.c_void_p), ("moments", C.c_void_p), ("variance", C.c_void_p), ("prev_xy", C.c_void_p),
                ("memory", C.c_int32)]


# p3d_accumulate's defaults: conveniences, not measured
ACCUMULATE_DEPTH_TOLERANCE = 0.05
ACCUMULATE_NORMAL_MIN = 0.9
ACCUMULATE_MAX_HISTORY = 32.0


class AoParams(C.Structure):
    """p3d_ao_params: samples (1, 2, 4, .. 64) segments of length radius per pixel, their origin moved bias along the normal
    that faces the eye; frame f keys its random streams with seed + f."""
    _fields_ = [("samples", C.c_int32), ("radius", C.c_float), ("bias", C.c_float), ("seed", C.c_uint32)]


class AoInputs(C.Structure):
    """p3d_ao_inputs: depth, normal and (optionally) colour planes as p3d_render_aov writes them, host (memory 0) or device (1)."""
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("rgb32f", C.c_void_p), ("memory", C.c_int32)]


class AoOutputs(C.Structure):
    _fields_ = [("ao", C.c_void_p), ("rgb32f", C.c_void_p), ("memory", C.c_int32)]


# p3d_ambient_occlusion's defaults: conveniences, not measured (bias: the reference's EPSILON, RT/macros.h:1)
AO_SAMPLES = 8
AO_RADIUS = 0.5
AO_BIAS = 0.001


class IndirectParams(C.Structure):
    """p3d_indirect_params: samples (1, 2, 4, .. 64) cosine-weighted rays per pixel, their origin moved bias along the normal
    that faces the eye; frame f keys its random streams with seed + f."""
    _fields_ = [("samples", C.c_int32), ("bias", C.c_float), ("seed", C.c_uint32)]


class IndirectInputs(C.Structure):
    """p3d_indirect_inputs: depth, normal and (optionally) albedo and colour planes as p3d_render_aov writes them, host
    (memory 0) or device (1)."""
    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("rgb32f", C.c_void_p), ("memory", C.c_int32)]


class IndirectOutputs(C.Structure):
    """p3d_indirect_outputs: each plane may be NULL, not both."""
    _fields_ = [("indirect", C.c_void_p), ("rgb32f", C.c_void_p), ("memory", C.c_int32)]


# p3d_indirect_diffuse's defaults: conveniences, not measured (bias: the reference's EPSILON, RT/macros.h:1)
INDIRECT_SAMPLES = 8
INDIRECT_BIAS = 0.001


class PathParams(C.Structure):
    """p3d_path_params: samples (1, 2, 4, .. 64) paths per pixel of at most bounces (1 .. 8) rays each, every vertex's origin
    moved bias along the normal that faces the incoming ray; frame f keys its random streams with seed + f."""
    _fields_ = [("samples", C.c_int32), ("bounces", C.c_int32), ("bias", C.c_float), ("seed", C.c_uint32)]


# p3d_indirect_paths' default: a convenience, not measured
PATH_BOUNCES = 3


class UpsampleParams(C.Structure):
    """p3d_upsample_params: n_frames low frames of res_x x res_y back to back, brought up by factor 1..4; channels 1 or 3 floats
    per pixel of the signal; the denoiser's depth stop and normal_power_log2 0..8 squarings of the normal weight."""
    _fields_ = [("res_x", C.c_int32), ("res_y", C.c_int32), ("factor", C.c_int32), ("n_frames", C.c_int32), ("channels", C.c_int32),
                ("sigma_depth", C.c_float), ("normal_power_log2", C.c_int32)]


class UpsampleInputs(C.Structure):
    """p3d_upsample_inputs: the low signal with the depth and normal it was computed on, and the full frame's depth and normal,
    on the host (memory 0) or the scene's device (1)."""
    _fields_ = [("low", C.c_void_p), ("low_depth", C.c_void_p), ("low_normal", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p),
                ("memory", C.c_int32)]


class UpsampleOutputs(C.Structure):
    """p3d_upsample_outputs: each plane may be NULL, not both."""
    _fields_ = [("plane", C.c_void_p), ("fallback", C.c_void_p), ("memory", C.c_int32)]


# p3d_upsample's defaults: the denoiser's stops
UPSAMPLE_SIGMA_DEPTH = DENOISE_SIGMA_DEPTH
UPSAMPLE_NORMAL_POWER_LOG2 = DENOISE_NORMAL_POWER_LOG2


class PrimUpdate(C.Structure):
    """p3d_prim_update: n primitives to replace ([n][12] floats, optionally [n] scene indices) on the host (memory 0) or the
    scene's device (memory 1); lights: NULL or [n_lights][6] on the host."""
    _fields_ = [("n", C.c_uint32), ("index", C.c_void_p), ("prim_data", C.c_void_p), ("memory", C.c_int32), ("lights", C.c_void_p)]


class RebuildInfo(C.Structure):
    """p3d_rebuild_info: whether p3d_scene_rebuild made a new tree, that tree's shape, and the SAH cost before and after."""
    _fields_ = [("rebuilt", C.c_uint32), ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("max_depth", C.c_uint32),
                ("sah_cost_before", C.c_float), ("sah_cost_after", C.c_float)]


class GridInfo(C.Structure):
    """p3d_grid_info: whether p3d_scene_build_grid built the grid, and the grid the handle holds after the call."""
    _fields_ = [("built", C.c_uint32), ("n", C.c_int32 * 3), ("mn", C.c_float * 3), ("mx", C.c_float * 3),
                ("n_cells", C.c_uint64), ("n_items", C.c_uint64)]


class SceneStats(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("max_depth", C.c_uint32),
                ("n_leaf_refs", C.c_uint32), ("n_spheres", C.c_uint32), ("n_triangles", C.c_uint32),
                ("n_boxes", C.c_uint32), ("n_planes", C.c_uint32), ("n_culled", C.c_uint32),
                ("device_bytes", C.c_uint64), ("sah_cost", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/p3d_hip.h declares (tests check that the library exports them all)
C_ABI_SYMBOLS = ["p3d_abi_version", "p3d_last_error", "p3d_device_count", "p3d_scene_create",
                 "p3d_scene_destroy", "p3d_scene_set_skybox", "p3d_scene_get_stats", "p3d_scene_update", "p3d_scene_rebuild", "p3d_scene_rebuild_with", "p3d_scene_last_builder", "p3d_scene_tree_cost", "p3d_scene_build_grid", "p3d_local_rows", "p3d_render", "p3d_render_frames", "p3d_render_aov", "p3d_generate_samples", "p3d_trace_rays", "p3d_occluded", "p3d_denoise", "p3d_denoise_variance", "p3d_accumulate", "p3d_accumulate_moving", "p3d_accumulate_variance", "p3d_ambient_occlusion", "p3d_indirect_diffuse", "p3d_indirect_paths", "p3d_upsample", "p3d_sync",
                 "p3d_get_counters", "p3d_get_profile", "p3d_last_schedule", "p3d_set_tuning", "p3d_set_primary_tiles", "p3d_last_primary_tiles", "p3d_set_sky_tiles", "p3d_last_sky_tiles", "p3d_set_prune_reflections", "p3d_get_prune_reflections", "p3d_last_level_rays", "p3d_set_stream", "p3d_timer_begin", "p3d_timer_end", "p3d_deinterleave_frames",
                 "p3d_deinterleave", "p3d_debug_intersect", "p3d_debug_powf", "p3d_debug_pow", "p3d_debug_schlick_kr", "p3d_debug_check_rcp", "p3d_debug_check_rcp_len", "p3d_debug_lbvh_build", "p3d_debug_ploc_build", "p3d_debug_grid_build", "p3d_debug_rand", "p3d_debug_sample_stream", "p3d_debug_denoise", "p3d_debug_denoise_variance", "p3d_debug_accumulate", "p3d_debug_accumulate_moving", "p3d_debug_accumulate_variance", "p3d_debug_upsample", "p3d_tune_schedule", "p3d_debug_set_stamps", "p3d_debug_set_stamp_level",
                 "p3d_comm_unique_id", "p3d_comm_create", "p3d_comm_create_all", "p3d_comm_destroy", "p3d_comm_info",
                 "p3d_gather", "p3d_gather_all", "p3d_device_alloc", "p3d_device_free", "p3d_upload", "p3d_download"]


def build_native(verbose=False):
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_PKG, "csrc"), "-j4", "all"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


_lib = None


def lib():
    """The loaded C-ABI library.  No fallback: a missing extension is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise P3DError("native extension %s is missing: run __graft_entry__.build() "
                       "(make -C u_4a_2s_p3d_raytracer_template2_amd/csrc)" % LIB_PATH)
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so (same
    # SONAME as /opt/rocm's).  If torch is going to be used next to this library (bench.py,
    # device-pointer outputs) it must be loaded FIRST so that both resolve to one runtime;
    # two runtimes in one process leave the second without a visible GPU.
    if "torch" not in sys.modules and os.environ.get("P3D_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    L.p3d_last_error.restype = C.c_char_p
    L.p3d_device_count.argtypes = [C.POINTER(C.c_int)]
    L.p3d_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(BuildOpts), C.c_int, C.POINTER(C.c_void_p)]
    L.p3d_scene_destroy.argtypes = [C.c_void_p]
    L.p3d_scene_set_skybox.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.p3d_scene_get_stats.argtypes = [C.c_void_p, C.POINTER(SceneStats)]
    L.p3d_scene_update.argtypes = [C.c_void_p, C.POINTER(PrimUpdate)]
    L.p3d_scene_rebuild.argtypes = [C.c_void_p, C.POINTER(RebuildInfo)]
    L.p3d_scene_rebuild_with.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(RebuildInfo)]
    L.p3d_scene_last_builder.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.p3d_scene_tree_cost.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.p3d_scene_build_grid.argtypes = [C.c_void_p, C.POINTER(GridInfo)]
    L.p3d_local_rows.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.p3d_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(Outputs)]
    L.p3d_render_frames.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.POINTER(RenderParams), C.POINTER(Outputs)]
    L.p3d_render_aov.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.POINTER(RenderParams), C.POINTER(Outputs),
                                 C.POINTER(AovOutputs)]
    L.p3d_generate_samples.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32]
    L.p3d_trace_rays.argtypes = [C.c_void_p, C.POINTER(Rays), C.POINTER(RenderParams), C.POINTER(RayOutputs)]
    L.p3d_occluded.argtypes = [C.c_void_p, C.POINTER(Rays), C.POINTER(RenderParams), C.POINTER(OcclusionOutputs)]
    L.p3d_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(DenoiseInputs), C.POINTER(Outputs)]
    L.p3d_debug_denoise.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoiseInputs), C.POINTER(Outputs)]
    L.p3dh_denoise.argtypes = [C.POINTER(DenoiseParams)] + [C.c_void_p] * 6
    L.p3d_denoise_variance.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(DenoiseVarianceInputs), C.POINTER(DenoiseVarianceOutputs)]
    L.p3d_debug_denoise_variance.argtypes = [C.c_int, C.POINTER(DenoiseParams), C.POINTER(DenoiseVarianceInputs), C.POINTER(DenoiseVarianceOutputs)]
    L.p3dh_denoise_variance.argtypes = [C.POINTER(DenoiseParams)] + [C.c_void_p] * 8
    L.p3dh_denoise_variance.restype = None
    _ups = [C.POINTER(UpsampleParams), C.POINTER(UpsampleInputs), C.POINTER(UpsampleOutputs)]
    L.p3d_upsample.argtypes = [C.c_void_p] + _ups
    L.p3d_debug_upsample.argtypes = [C.c_int] + _ups
    L.p3dh_upsample.argtypes = [C.POINTER(UpsampleParams)] + [C.c_void_p] * 7
    L.p3dh_upsample.restype = None
    _acc = [C.POINTER(AccumulateParams), C.POINTER(AccumulateFrames), C.POINTER(AccumulateHistory)]
    L.p3d_accumulate.argtypes = [C.c_void_p] + _acc + [C.POINTER(AccumulateOutputs)]
    L.p3d_debug_accumulate.argtypes = [C.c_int] + _acc + [C.POINTER(AccumulateOutputs)]
    L.p3dh_accumulate.argtypes = _acc + [C.c_void_p, C.c_void_p]
    L.p3dh_accumulate.restype = None
    _mov = _acc + [C.POINTER(AccumulateMotion)]
    L.p3d_accumulate_moving.argtypes = [C.c_void_p] + _mov + [C.POINTER(AccumulateMovingOutputs)]
    L.p3d_debug_accumulate_moving.argtypes = [C.c_int] + _mov + [C.POINTER(AccumulateMovingOutputs)]
    _var = [C.POINTER(AccumulateParams), C.POINTER(AccumulateVarianceParams), C.POINTER(AccumulateFrames), C.POINTER(AccumulateHistory),
            C.c_void_p, C.POINTER(AccumulateMotion)]
    L.p3d_accumulate_variance.argtypes = [C.c_void_p] + _var + [C.POINTER(AccumulateVarianceOutputs)]
    L.p3d_debug_accumulate_variance.argtypes = [C.c_int] + _var + [C.POINTER(AccumulateVarianceOutputs)]
    L.p3dh_accumulate_variance.argtypes = _var + [C.c_void_p] * 5
    L.p3dh_accumulate_variance.restype = None
    L.p3dh_accumulate_moving.argtypes = _mov + [C.c_void_p, C.c_void_p, C.c_void_p]
    L.p3dh_accumulate_moving.restype = None
    L.p3d_ambient_occlusion.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.POINTER(RenderParams), C.POINTER(AoParams),
                                        C.POINTER(AoInputs), C.POINTER(AoOutputs)]
    L.p3dh_ao_segments.argtypes = [C.POINTER(AoParams), C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    L.p3dh_ao_segments.restype = None
    L.p3dh_ao_resolve.argtypes = [C.c_int32, C.c_uint64] + [C.c_void_p] * 4
    L.p3dh_ao_resolve.restype = None
    L.p3d_indirect_diffuse.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.POINTER(RenderParams), C.POINTER(IndirectParams),
                                       C.POINTER(IndirectInputs), C.POINTER(IndirectOutputs)]
    L.p3dh_indirect_resolve.argtypes = [C.c_int32, C.c_uint64] + [C.c_void_p] * 6
    L.p3dh_indirect_resolve.restype = None
    L.p3d_indirect_paths.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.POINTER(RenderParams), C.POINTER(PathParams),
                                     C.POINTER(IndirectInputs), C.POINTER(IndirectOutputs)]
    L.p3dh_path_next.argtypes = [C.c_uint64, C.c_int32, C.c_float] + [C.c_void_p] * 13
    L.p3dh_path_next.restype = None
    L.p3dh_path_add.argtypes = [C.c_uint64, C.c_int32] + [C.c_void_p] * 4
    L.p3dh_path_add.restype = None
    L.p3d_sync.argtypes = [C.c_void_p]
    L.p3d_get_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
    L.p3d_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.p3d_get_profile.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.p3d_last_schedule.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.p3d_set_tuning.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.p3d_set_primary_tiles.argtypes = [C.c_void_p, C.c_int32]
    L.p3d_last_primary_tiles.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.p3d_set_sky_tiles.argtypes = [C.c_void_p, C.c_int32]
    L.p3d_last_sky_tiles.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.p3d_set_prune_reflections.argtypes = [C.c_void_p, C.c_int32]
    L.p3d_get_prune_reflections.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.p3d_last_level_rays.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int32]
    L.p3dh_tile_coverage.argtypes = [C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(SceneDesc), C.c_void_p]
    L.p3dh_tile_coverage.restype = C.c_int32
    L.p3d_timer_begin.argtypes = [C.c_void_p]
    L.p3d_timer_end.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.p3d_deinterleave.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_uint64]
    L.p3d_debug_set_stamps.argtypes = [C.c_void_p, C.c_void_p]
    L.p3d_debug_set_stamp_level.argtypes = [C.c_void_p, C.c_int32]
    L.p3d_comm_unique_id.argtypes = [C.c_void_p]
    L.p3d_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.p3d_comm_create_all.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
    L.p3d_comm_destroy.argtypes = [C.c_void_p]
    L.p3d_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.p3d_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.p3d_gather_all.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int,
                                 C.c_void_p, C.c_uint64]
    L.p3d_device_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.p3d_device_free.argtypes = [C.c_void_p, C.c_void_p]
    L.p3d_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.p3d_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.p3d_pt_reduce_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.p3d_debug_intersect.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 7
    L.p3d_debug_powf.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 3
    L.p3d_debug_pow.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 3
    L.p3d_debug_schlick_kr.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 4
    L.p3d_debug_check_rcp.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    L.p3d_debug_check_rcp_len.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    L.p3d_debug_lbvh_build.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 7
    L.p3d_debug_ploc_build.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 9
    L.p3d_debug_grid_build.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 8 + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.p3d_debug_rand.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
    L.p3d_debug_sample_stream.argtypes = [C.c_int, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_void_p,
                                          C.POINTER(C.c_int32)]
    L.p3d_tune_schedule.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    # host shim
    L.p3dh_scene_load.restype = C.c_void_p
    L.p3dh_scene_load.argtypes = [C.c_char_p]
    L.p3dh_scene_free.argtypes = [C.c_void_p]
    L.p3dh_scene_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.p3dh_scene_set_resolution.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.p3dh_scene_set_eye.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
    L.p3dh_orbit_eyes.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_void_p]
    L.p3dh_scene_orbit_cameras.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_void_p]
    L.p3dh_scene_desc.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
    L.p3dh_scene_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
    L.p3dh_primary_ray.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.p3dh_trace_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.p3dh_occluded.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.p3dh_generate_samples.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    L.p3dh_bvh_build.restype = C.c_void_p
    L.p3dh_bvh_build.argtypes = [C.POINTER(SceneDesc), C.c_uint32]
    L.p3dh_bvh_free.argtypes = [C.c_void_p]
    L.p3dh_bvh_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.p3dh_bvh_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.p3dh_bvh_quantise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.p3dh_grid_dump.restype = C.c_int64
    L.p3dh_grid_dump.argtypes = [C.POINTER(SceneDesc), C.c_uint32] + [C.c_void_p] * 7 + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.p3dh_build_prims.restype = C.c_int64
    L.p3dh_build_prims.argtypes = [C.POINTER(SceneDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    L.p3d_pt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.p3d_pt_destroy.argtypes = [C.c_void_p]
    L.p3d_pt_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.p3d_pt_render.argtypes = [C.c_void_p, C.POINTER(PtParams), C.POINTER(PtOutputs)]
    L.p3d_pt_sync.argtypes = [C.c_void_p]
    L.p3d_pt_timer_begin.argtypes = [C.c_void_p]
    L.p3d_pt_timer_end.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.p3d_pt_debug_hash.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.p3d_pt_debug_hit_world.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 14
    L.p3d_pt_debug_scatter.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 14
    L.p3d_pt_debug_direct_lighting.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 12
    _lib = L
    return L


class PtParams(C.Structure):
    _fields_ = [("res_x", C.c_int32), ("res_y", C.c_int32), ("n_frames", C.c_int32), ("first_frame", C.c_int32),
                ("frame_stride", C.c_int32), ("time0", C.c_float), ("dt", C.c_float), ("mouse_x", C.c_float),
                ("mouse_y", C.c_float)]


class PtOutputs(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("linear", C.c_void_p), ("memory", C.c_int32)]


# include/p3d_pathtracer.h
PT_C_ABI_SYMBOLS = ["p3d_pt_create", "p3d_pt_destroy", "p3d_pt_set_stream", "p3d_pt_render", "p3d_pt_sync",
                    "p3d_pt_timer_begin", "p3d_pt_timer_end", "p3d_pt_debug_hash", "p3d_pt_reduce_sum",
                    "p3d_pt_debug_hit_world", "p3d_pt_debug_scatter", "p3d_pt_debug_direct_lighting"]


def _check(rc, what):
    if rc != 0:
        raise P3DError("%s failed (%d): %s" % (what, rc, lib().p3d_last_error().decode()))


def device_count():
    n = C.c_int(0)
    rc = lib().p3d_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def local_rows(res_y, row_block=16, world=1):
    return lib().p3d_local_rows(res_y, row_block, world)


class HostScene:
    """Scene loaded by the C++ host layer (Scene::load_p3f mirror) and flattened for the C-ABI."""

    def __init__(self, path):
        self.h = lib().p3dh_scene_load(os.fsencode(path))
        if not self.h:
            raise P3DError("cannot load scene %s" % path)
        self._refresh()

    def _refresh(self):
        out = (C.c_int32 * 8)()
        lib().p3dh_scene_info(self.h, out)
        (self.n_prims, self.n_lights, self.n_materials, self.res_x, self.res_y, self.accel, self.spp,
         self.parse_ok) = [int(v) for v in out]

    def close(self):
        if self.h:
            lib().p3dh_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_resolution(self, w, h):
        lib().p3dh_scene_set_resolution(self.h, int(w), int(h))
        self._refresh()

    def set_eye(self, x, y, z):
        lib().p3dh_scene_set_eye(self.h, float(x), float(y), float(z))

    def orbit_cameras(self, n, step_deg, d_beta_deg=0.0):
        """n cameras of the reference's mouse orbit around this scene's eye (orbit_eyes; Camera::SetEye on a copy of the
        camera per eye, so the scene's own camera is unchanged)."""
        out = (Camera * int(n))()
        lib().p3dh_scene_orbit_cameras(self.h, int(n), float(step_deg), float(d_beta_deg), out)
        return list(out)

    def desc(self):
        d = SceneDesc()
        lib().p3dh_scene_desc(self.h, C.byref(d))
        return d

    def camera(self):
        c = Camera()
        lib().p3dh_scene_camera(self.h, C.byref(c))
        return c

    def primary_ray(self, px, py):
        o = (C.c_float * 3)()
        d = (C.c_float * 3)()
        lib().p3dh_primary_ray(self.h, px, py, o, d)
        return np.array(o, np.float32), np.array(d, np.float32)

    def trace_rays(self, origins, dirs, max_depth=4, accel=ACCEL_BVH, soft_shadow=False, device=0):
        """traceRays() of the C++ host layer: rayTracing(ray, 1, 1.0) per ray on one GPU -> rgb32f, hit_id, t, normal."""
        o, d, n = _ray_arrays(origins, dirs)
        out = _ray_planes(n, RAY_PLANES)
        _check(lib().p3dh_trace_rays(self.h, n, o.ctypes.data, d.ctypes.data, int(max_depth), int(accel), 1 if soft_shadow else 0,
                                     int(device), *[out[k].ctypes.data for k in RAY_PLANES]), "traceRays")
        return out

    def occluded(self, origins, dirs, accel=ACCEL_BVH, device=0):
        """occluded() of the C++ host layer: processLight()'s shadow query per segment on one GPU -> (n,) uint8, 1 = in shadow."""
        o, d, n = _ray_arrays(origins, dirs)
        out = np.zeros(n, np.uint8)
        _check(lib().p3dh_occluded(self.h, n, o.ctypes.data, d.ctypes.data, int(accel), int(device), out.ctypes.data), "occluded")
        return out

    def arrays(self):
        """numpy views of the flattened scene (type, data12, material, materials12, lights6, bg)."""
        d = self.desc()
        n = d.n_prims
        t = np.ctypeslib.as_array(d.prim_type, (n,)).copy() if n else np.zeros(0, np.uint32)
        data = np.ctypeslib.as_array(d.prim_data, (n, 12)).copy() if n else np.zeros((0, 12), np.float32)
        m = np.ctypeslib.as_array(d.prim_material, (n,)).copy() if n else np.zeros(0, np.uint32)
        mats = np.ctypeslib.as_array(d.materials, (d.n_materials, 12)).copy()
        li = np.ctypeslib.as_array(d.lights, (d.n_lights, 6)).copy() if d.n_lights else np.zeros((0, 6), np.float32)
        return t, data, m, mats, li, np.array(d.background, np.float32)

    def samples(self, seed, spp):
        cam = self.camera()
        out = np.zeros((self.res_y, self.res_x, spp * spp, 4), np.float32)
        lib().p3dh_generate_samples(int(seed), self.res_x, self.res_y, int(spp), cam.aperture,
                                    out.ctypes.data_as(C.c_void_p))
        return out


def orbit_eyes(eye, n, step_deg, d_beta_deg=0.0):
    """(n, 3) float32: the host layer's orbit_eyes, the reference's mouse orbit (RT/main.cpp:339-341, 419-421)."""
    out = np.zeros((int(n), 3), np.float32)
    lib().p3dh_orbit_eyes(float(eye[0]), float(eye[1]), float(eye[2]), int(n), float(step_deg), float(d_beta_deg),
                          out.ctypes.data_as(C.c_void_p))
    return out


RAY_PLANES = ("rgb32f", "hit_id", "t", "normal")       # the planes of p3d_ray_outputs, in its order
AOV_PLANES = ("depth", "normal", "albedo")             # the planes of p3d_aov_outputs, in its order


def host_tile_coverage(cam, desc, tile_h=16, row_block=16, rank=0, world=1):
    """(active [tiles_y, tiles_x] bool, fell_back): the level-1 launch's tile coverage mask of cam's frame over a scene
    description, on the host (csrc/p3d_tile_coverage.h through host/tile_coverage_host.cpp).  fell_back: every tile was
    marked because a primitive asked for it."""
    tiles_x, tiles_y = (cam.res_x + 15) // 16, local_rows(cam.res_y, row_block, world) // tile_h
    out = np.zeros((tiles_y, tiles_x), np.uint8)
    fell = lib().p3dh_tile_coverage(C.byref(cam), int(tile_h), int(row_block), int(rank), int(world), C.byref(desc), out.ctypes.data)
    return out.astype(bool), bool(fell)


def _ray_arrays(origins, dirs):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("origins and dirs differ in length")
    return o, d, len(o)


def _ray_planes(n, want):
    shape = {"rgb32f": ((n, 3), np.float32), "hit_id": ((n,), np.int32), "t": ((n,), np.float32), "normal": ((n, 3), np.float32)}
    for k in want:
        if k not in shape:
            raise ValueError("unknown ray output plane %r" % (k,))
    return {k: np.zeros(shape[k][0], shape[k][1]) for k in want}


def make_desc(ptype, data12, material, materials12, lights6, bg):
    """SceneDesc over caller-owned numpy arrays (returns (desc, keepalive))."""
    ptype = np.ascontiguousarray(ptype, np.uint32)
    data12 = np.ascontiguousarray(data12, np.float32).reshape(-1, 12)
    material = np.ascontiguousarray(material, np.uint32)
    materials12 = np.ascontiguousarray(materials12, np.float32).reshape(-1, 12)
    lights6 = np.ascontiguousarray(lights6, np.float32).reshape(-1, 6)
    d = SceneDesc()
    d.n_prims = len(ptype)
    d.prim_type = ptype.ctypes.data_as(C.POINTER(C.c_uint32))
    d.prim_data = data12.ctypes.data_as(C.POINTER(C.c_float))
    d.prim_material = material.ctypes.data_as(C.POINTER(C.c_uint32))
    d.n_materials = len(materials12)
    d.materials = materials12.ctypes.data_as(C.POINTER(C.c_float))
    d.n_lights = len(lights6)
    d.lights = lights6.ctypes.data_as(C.POINTER(C.c_float))
    d.background = (C.c_float * 3)(*[float(v) for v in bg])
    return d, (ptype, data12, material, materials12, lights6)


class DeviceScene:
    """p3d_scene on one GPU."""

    def __init__(self, desc, device=0, leaf_max=0, keepalive=None, builder=0, cull_never_hit=False):
        """builder: 0 = host SAH, 1 = device LBVH, 2 = device clustering (near SAH quality); cull_never_hit: see p3d_build_opts in p3d_hip.h."""
        self._keep = keepalive
        self.h = C.c_void_p()
        opts = BuildOpts(leaf_max, 0, builder, 1 if cull_never_hit else 0)
        _check(lib().p3d_scene_create(C.byref(desc), C.byref(opts), int(device), C.byref(self.h)),
               "p3d_scene_create")
        self.device = device

    @classmethod
    def from_host(cls, hs, device=0, leaf_max=0, builder=0, cull_never_hit=False):
        return cls(hs.desc(), device, leaf_max, keepalive=hs, builder=builder, cull_never_hit=cull_never_hit)

    def close(self):
        if self.h:
            lib().p3d_scene_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        s = SceneStats()
        _check(lib().p3d_scene_get_stats(self.h, C.byref(s)), "p3d_scene_get_stats")
        return s.as_dict()

    def update(self, prim12, indices=None, lights6=None):
        """p3d_scene_update from host arrays: primitives `indices` (None: 0 .. n-1) get the geometry prim12 [n, 12], in the
        form p3d_scene_desc::prim_data has for their kind; lights6 (None: unchanged) replaces all lights [n_lights, 6].
        The BVH is refitted on the device; every later frame equals that of a handle created from the moved scene."""
        data = np.ascontiguousarray(prim12 if prim12 is not None else np.zeros((0, 12)), np.float32).reshape(-1, 12)
        n = len(data)
        idx = None
        if indices is not None:
            idx = np.ascontiguousarray(indices, np.uint32).ravel()
            if len(idx) != n:
                raise ValueError("indices and prim12 differ in length")
        li = np.ascontiguousarray(lights6, np.float32).reshape(-1, 6) if lights6 is not None else None
        u = PrimUpdate(n, idx.ctypes.data if idx is not None and n else None, data.ctypes.data if n else None, 0,
                       li.ctypes.data if li is not None and len(li) else None)
        _check(lib().p3d_scene_update(self.h, C.byref(u)), "p3d_scene_update")

    def update_device(self, n, prim_ptr, index_ptr=0):
        """p3d_scene_update from caller-owned DEVICE buffers (raw pointers): prim_ptr [n][12] floats, index_ptr [n] uint32
        scene indices or 0 for primitives 0 .. n-1."""
        u = PrimUpdate(int(n), index_ptr or None, prim_ptr or None, 1, None)
        _check(lib().p3d_scene_update(self.h, C.byref(u)), "p3d_scene_update")

    def rebuild(self, builder=1):
        """p3d_scene_rebuild_with: a device builder's tree (1 = LBVH, what p3d_scene_rebuild makes; 2 = clustering) over the
        primitives where they are now, in place.  Frames stay what they were, bit for bit.  Returns p3d_rebuild_info as a
        dict (rebuilt == 0: a scene served from LDS, left alone)."""
        info = RebuildInfo()
        _check(lib().p3d_scene_rebuild_with(self.h, int(builder), C.byref(info)), "p3d_scene_rebuild_with")
        return {n: getattr(info, n) for n, _ in info._fields_}

    def last_builder(self):
        """p3d_scene_last_builder: whose tree the handle walks now (0 host SAH, 1 device LBVH, 2 device clustering)."""
        v = C.c_int32(-1)
        _check(lib().p3d_scene_last_builder(self.h, C.byref(v)), "p3d_scene_last_builder")
        return v.value

    def build_grid(self):
        """p3d_scene_build_grid: GRID mode's grid built on the device from what the handle holds there (after updates from
        device memory too).  Returns p3d_grid_info as a dict: built (0: the handle already had a grid), n [3] int32, mn / mx
        [3] float32, n_cells, n_items."""
        info = GridInfo()
        _check(lib().p3d_scene_build_grid(self.h, C.byref(info)), "p3d_scene_build_grid")
        return {"built": int(info.built), "n": np.array(list(info.n), np.int32), "mn": np.array(list(info.mn), np.float32),
                "mx": np.array(list(info.mx), np.float32), "n_cells": int(info.n_cells), "n_items": int(info.n_items)}

    def tree_cost(self):
        """p3d_scene_tree_cost: SAH cost of the tree as it stands (after updates: of the refitted boxes)."""
        v = C.c_float(0)
        _check(lib().p3d_scene_tree_cost(self.h, C.byref(v)), "p3d_scene_tree_cost")
        return v.value

    def generate_samples(self, seed, res_x, res_y, spp, aperture):
        """p3d_generate_samples into a numpy array (res_y, res_x, spp*spp, 4): the bits HostScene.samples / the host layer's
        generate_samples() gives for (seed, aperture), made on the device."""
        out = np.zeros((int(res_y), int(res_x), int(spp) * int(spp), 4), np.float32)
        _check(lib().p3d_generate_samples(self.h, int(seed) & 0xFFFFFFFF, int(res_x), int(res_y), int(spp), float(aperture),
                                          out.ctypes.data if out.size else None, 0), "p3d_generate_samples")
        return out

    def generate_samples_device(self, ptr, seed, res_x, res_y, spp, aperture):
        """p3d_generate_samples into a caller-owned DEVICE buffer (raw pointer) of res_y * res_x * spp*spp * 4 floats: what
        render_device(..., samples_ptr=ptr) reads.  Returns when the array is complete."""
        _check(lib().p3d_generate_samples(self.h, int(seed) & 0xFFFFFFFF, int(res_x), int(res_y), int(spp), float(aperture),
                                          C.c_void_p(int(ptr) or None), 1), "p3d_generate_samples")

    def set_skybox(self, faces):
        """Six uint8 arrays [H, W, 3 or 4]: right, left, top, bottom, front, back; row 0 = bottom row (Scene::LoadSkybox)."""
        faces = [np.ascontiguousarray(f, np.uint8) for f in faces]
        ptrs = (C.c_void_p * 6)(*[f.ctypes.data for f in faces])
        rx = (C.c_uint32 * 6)(*[f.shape[1] for f in faces])
        ry = (C.c_uint32 * 6)(*[f.shape[0] for f in faces])
        bpp = (C.c_uint32 * 6)(*[f.shape[2] for f in faces])
        _check(lib().p3d_scene_set_skybox(self.h, ptrs, rx, ry, bpp), "p3d_scene_set_skybox")

    def set_stream(self, stream_ptr):
        _check(lib().p3d_set_stream(self.h, C.c_void_p(stream_ptr)), "p3d_set_stream")

    def set_tuning(self, xcd_chunk=0, workspace_mib=0, waves_per_simd=-1):
        _check(lib().p3d_set_tuning(self.h, int(xcd_chunk), int(workspace_mib), int(waves_per_simd)),
               "p3d_set_tuning")

    def set_primary_tiles(self, tiles):
        """16x16 tiles per workgroup of the wavefront schedule's level-1 launch: 1, 2 or 3 (0: the default)."""
        _check(lib().p3d_set_primary_tiles(self.h, int(tiles)), "p3d_set_primary_tiles")

    def last_primary_tiles(self):
        """Tiles per workgroup the most recent render's level-1 launch ran with (1 where no such kernel is built)."""
        v = C.c_int32()
        _check(lib().p3d_last_primary_tiles(self.h, C.byref(v)), "p3d_last_primary_tiles")
        return v.value

    def set_sky_tiles(self, on):
        """Tile coverage mask of the multi-tile level-1 kernels (p3d_set_sky_tiles): tiles no primitive projects onto are
        filled with the background instead of traced.  Never changes results."""
        _check(lib().p3d_set_sky_tiles(self.h, 1 if on else 0), "p3d_set_sky_tiles")

    def last_sky_tiles(self):
        """(used, empty_tiles) of the most recent render: whether it ran with a tile coverage mask, and how many tiles the
        mask marked empty.  Waits for the stream."""
        used, empty = C.c_int32(), C.c_int32()
        _check(lib().p3d_last_sky_tiles(self.h, C.byref(used), C.byref(empty)), "p3d_last_sky_tiles")
        return bool(used.value), empty.value

    def set_prune_reflections(self, on):
        """p3d_set_prune_reflections: transmissive nodes spawn no reflection child (the reference scales it by KR = +0).
        Never changes a frame of a finite scene; counting and Schlick frames trace every ray whatever is set."""
        _check(lib().p3d_set_prune_reflections(self.h, 1 if on else 0), "p3d_set_prune_reflections")

    def prune_reflections(self):
        """Whether frames of this scene prune: the switch is on and the scene was finite when it was created."""
        v = C.c_int32()
        _check(lib().p3d_get_prune_reflections(self.h, C.byref(v)), "p3d_get_prune_reflections")
        return bool(v.value)

    def last_level_rays(self, n=16):
        """p3d_last_level_rays: closest-hit rays queued per tree level (index 0 = level 1) by the most recent
        wavefront-schedule frame or ray stream, as a uint32 array of n entries.  Waits for the stream."""
        v = (C.c_uint32 * int(n))()
        _check(lib().p3d_last_level_rays(self.h, v, int(n)), "p3d_last_level_rays")
        return np.array(list(v), np.uint32)

    def sync(self):
        _check(lib().p3d_sync(self.h), "p3d_sync")

    def timer_begin(self):
        _check(lib().p3d_timer_begin(self.h), "p3d_timer_begin")

    def timer_end(self):
        ms = C.c_float(0)
        _check(lib().p3d_timer_end(self.h, C.byref(ms)), "p3d_timer_end")
        return ms.value

    def profile(self):
        """(frame_ms, dominant_kernel_ms) of the last render made with profile=True."""
        f, k = C.c_float(0), C.c_float(0)
        _check(lib().p3d_get_profile(self.h, C.byref(f), C.byref(k)), "p3d_get_profile")
        return f.value, k.value

    def last_schedule(self):
        """'wavefront', 'tree' or 'tile': the kernel schedule of the most recent render."""
        v = C.c_int32()
        _check(lib().p3d_last_schedule(self.h, C.byref(v)), "p3d_last_schedule")
        return ("wavefront", "tree", "tile")[v.value]

    def debug_set_stamps(self, ptr):
        _check(lib().p3d_debug_set_stamps(self.h, C.c_void_p(ptr or None)), "p3d_debug_set_stamps")

    def debug_set_stamp_level(self, level):
        _check(lib().p3d_debug_set_stamp_level(self.h, int(level)), "p3d_debug_set_stamp_level")

    def counters(self):
        c = Counters()
        _check(lib().p3d_get_counters(self.h, C.byref(c)), "p3d_get_counters")
        return c.as_dict()

    def _params(self, max_depth, accel, spp, samples, rank, world, row_block, counters, tree=False, no_lds=False, profile=False, wavefront=False, soft_shadow=False, fuzzy_reflection=False, seed=0, tile=False, samples_ptr=0, packet=False, private_walk=False, skybox=False, schlick=False):
        p = RenderParams()
        p.max_depth, p.accel, p.spp = int(max_depth), int(accel), int(spp)
        p.samples = samples.ctypes.data_as(C.POINTER(C.c_float)) if samples is not None else None
        if samples_ptr:                      # sample array already on the device (uploaded once by the caller)
            p.samples = C.cast(C.c_void_p(int(samples_ptr)), C.POINTER(C.c_float))
        p.row_block, p.rank, p.world = int(row_block), int(rank), int(world)
        p.features = (FEATURE_SOFT_SHADOW if soft_shadow else 0) | (FEATURE_FUZZY_REFLECTION if fuzzy_reflection else 0) | (FEATURE_SKYBOX if skybox else 0) | (FEATURE_SCHLICK if schlick else 0)
        p.seed = int(seed) & 0xFFFFFFFF
        p.flags = (FLAG_COUNTERS if counters else 0) | (FLAG_TREE_KERNEL if tree else 0) | (FLAG_NO_LDS_SCENE if no_lds else 0) | (FLAG_PROFILE if profile else 0) | (FLAG_WAVEFRONT if wavefront else 0) | (FLAG_TILE_KERNEL if tile else 0) | (FLAG_DEVICE_SAMPLES if samples_ptr else 0) | (FLAG_PACKET_WALK if packet else 0) | (FLAG_PRIVATE_WALK if private_walk else 0)
        return p

    def render(self, cam, max_depth=4, accel=ACCEL_BVH, spp=0, samples=None, rank=0, world=1, row_block=16,
               want_f32=True, want_hit=True, counters=False, tree=False, no_lds=False, profile=False, wavefront=False, soft_shadow=False, fuzzy_reflection=False, seed=0, tile=False, packet=False, private_walk=False, skybox=False, schlick=False):
        """Render into host numpy arrays (rows: res_y for world==1, local_rows otherwise)."""
        rows = cam.res_y if world == 1 else local_rows(cam.res_y, row_block, world)
        rgb8 = np.zeros((rows, cam.res_x, 3), np.uint8)
        f32 = np.zeros((rows, cam.res_x, 3), np.float32) if want_f32 else None
        hid = np.full((rows, cam.res_x), -2, np.int32) if want_hit else None
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.float32)
        p = self._params(max_depth, accel, spp, samples, rank, world, row_block, counters, tree, no_lds, profile, wavefront, soft_shadow, fuzzy_reflection, seed, tile, 0, packet, private_walk, skybox, schlick)
        o = Outputs(rgb8.ctypes.data, f32.ctypes.data if want_f32 else None,
                    hid.ctypes.data if want_hit else None, 0)
        _check(lib().p3d_render(self.h, C.byref(cam), C.byref(p), C.byref(o)), "p3d_render")
        out = {"rgb8": rgb8, "rgb32f": f32, "hit_id": hid}
        if counters:
            out["counters"] = self.counters()
        return out

    def render_device(self, cam, rgb8_ptr=0, rgb32f_ptr=0, hit_ptr=0, max_depth=4, accel=ACCEL_BVH, spp=0,
                      samples=None, rank=0, world=1, row_block=16, counters=False, tree=False, no_lds=False, profile=False, wavefront=False, soft_shadow=False, fuzzy_reflection=False, seed=0, tile=False, samples_ptr=0, packet=False, private_walk=False, skybox=False, schlick=False):
        """Enqueue one frame into caller-owned DEVICE buffers (raw pointers); asynchronous.  samples_ptr: the
        spp > 0 sample array as a device pointer (uploaded once by the caller) instead of `samples`."""
        p = self._params(max_depth, accel, spp, samples, rank, world, row_block, counters, tree, no_lds, profile, wavefront, soft_shadow, fuzzy_reflection, seed, tile, samples_ptr, packet, private_walk, skybox, schlick)
        o = Outputs(rgb8_ptr or None, rgb32f_ptr or None, hit_ptr or None, 1)
        _check(lib().p3d_render(self.h, C.byref(cam), C.byref(p), C.byref(o)), "p3d_render")

    def render_frames(self, cams, max_depth=4, accel=ACCEL_BVH, spp=0, samples=None, rank=0, world=1, row_block=16,
                      want_f32=True, want_hit=True, counters=False, tree=False, no_lds=False, profile=False, wavefront=False,
                      soft_shadow=False, fuzzy_reflection=False, seed=0, tile=False, packet=False, private_walk=False, skybox=False,
                      schlick=False):
        """n frames of one configuration in one p3d_render_frames call, frame f seen through cams[f] with seed + f.
        samples (spp > 0): (n, res_y, res_x, spp*spp, 4), one sample array per frame.  Returns rgb8 (n, rows, W, 3),
        rgb32f (n, rows, W, 3) and hit_id (n, rows, W); rows = res_y for world == 1, local_rows otherwise."""
        arr, n = _camera_array(cams)
        c0 = arr[0]
        rows = c0.res_y if world == 1 else local_rows(c0.res_y, row_block, world)
        rgb8 = np.zeros((n, rows, c0.res_x, 3), np.uint8)
        f32 = np.zeros((n, rows, c0.res_x, 3), np.float32) if want_f32 else None
        hid = np.full((n, rows, c0.res_x), -2, np.int32) if want_hit else None
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.float32)
        p = self._params(max_depth, accel, spp, samples, rank, world, row_block, counters, tree, no_lds, profile, wavefront, soft_shadow, fuzzy_reflection, seed, tile, 0, packet, private_walk, skybox, schlick)
        o = Outputs(rgb8.ctypes.data if rgb8.size else None, f32.ctypes.data if want_f32 and f32.size else None,
                    hid.ctypes.data if want_hit and hid.size else None, 0)
        _check(lib().p3d_render_frames(self.h, arr, n, C.byref(p), C.byref(o)), "p3d_render_frames")
        out = {"rgb8": rgb8, "rgb32f": f32, "hit_id": hid}
        if counters:
            out["counters"] = self.counters()
        return out

    def render_frames_device(self, cams, rgb8_ptr=0, rgb32f_ptr=0, hit_ptr=0, max_depth=4, accel=ACCEL_BVH, spp=0,
                             samples=None, rank=0, world=1, row_block=16, counters=False, tree=False, no_lds=False, profile=False,
                             wavefront=False, soft_shadow=False, fuzzy_reflection=False, seed=0, tile=False, samples_ptr=0, packet=False,
                             private_walk=False, skybox=False, schlick=False):
        """Enqueue a batch into caller-owned DEVICE buffers holding n frames back to back (raw pointers); asynchronous."""
        arr, n = _camera_array(cams)
        p = self._params(max_depth, accel, spp, samples, rank, world, row_block, counters, tree, no_lds, profile, wavefront, soft_shadow, fuzzy_reflection, seed, tile, samples_ptr, packet, private_walk, skybox, schlick)
        o = Outputs(rgb8_ptr or None, rgb32f_ptr or None, hit_ptr or None, 1)
        _check(lib().p3d_render_frames(self.h, arr, n, C.byref(p), C.byref(o)), "p3d_render_frames")

    def render_aov(self, cam_or_cams, max_depth=4, accel=ACCEL_BVH, spp=0, samples=None, rank=0, world=1, row_block=16,
                   want=AOV_PLANES, **switches):
        """p3d_render_aov into host numpy arrays: the frames of render_frames (one Camera, or a sequence of n) and, written by
        the same launches, the planes named in `want` for the primary hit hit_id describes -- depth (n, rows, W): the
        intersector's t, +inf on a miss; normal (n, rows, W, 3); albedo (n, rows, W, 3): the material's diffuse rgb; zeros
        on a miss.  rows = res_y for world == 1, local_rows otherwise.  switches: the keyword switches of render_frames
        (wavefront, tile, tree, no_lds, private_walk, soft_shadow, ...).  Returns the dict of render_frames plus the planes."""
        for k in want:
            if k not in AOV_PLANES:
                raise ValueError("unknown AOV plane %r" % (k,))
        arr, n = _camera_array([cam_or_cams] if isinstance(cam_or_cams, Camera) else cam_or_cams)
        c0 = arr[0]
        rows = c0.res_y if world == 1 else local_rows(c0.res_y, row_block, world)
        out = {"rgb8": np.zeros((n, rows, c0.res_x, 3), np.uint8), "rgb32f": np.zeros((n, rows, c0.res_x, 3), np.float32),
               "hit_id": np.full((n, rows, c0.res_x), -2, np.int32)}
        for k in want:
            out[k] = np.zeros((n, rows, c0.res_x) if k == "depth" else (n, rows, c0.res_x, 3), np.float32)
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.float32)
        counters = bool(switches.pop("counters", False))
        p = self._params(max_depth, accel, spp, samples, rank, world, row_block, counters, **switches)
        ptr = lambda k: out[k].ctypes.data if k in out and out[k].size else None
        o = Outputs(ptr("rgb8"), ptr("rgb32f"), ptr("hit_id"), 0)
        a = AovOutputs(*[ptr(k) for k in AOV_PLANES])
        _check(lib().p3d_render_aov(self.h, arr, n, C.byref(p), C.byref(o), C.byref(a)), "p3d_render_aov")
        if counters:
            out["counters"] = self.counters()
        return out

    def render_aov_device(self, cam_or_cams, rgb8_ptr=0, rgb32f_ptr=0, hit_ptr=0, depth_ptr=0, normal_ptr=0, albedo_ptr=0,
                          max_depth=4, accel=ACCEL_BVH, spp=0, samples=None, rank=0, world=1, row_block=16, **switches):
        """Enqueue p3d_render_aov into caller-owned DEVICE buffers (raw pointers; 0 = no such plane); asynchronous."""
        arr, n = _camera_array([cam_or_cams] if isinstance(cam_or_cams, Camera) else cam_or_cams)
        counters = bool(switches.pop("counters", False))
        p = self._params(max_depth, accel, spp, samples, rank, world, row_block, counters, **switches)
        o = Outputs(rgb8_ptr or None, rgb32f_ptr or None, hit_ptr or None, 1)
        a = AovOutputs(depth_ptr or None, normal_ptr or None, albedo_ptr or None)
        _check(lib().p3d_render_aov(self.h, arr, n, C.byref(p), C.byref(o), C.byref(a)), "p3d_render_aov")

    def _ray_params(self, max_depth, accel, no_lds, private_walk, soft_shadow):
        return self._params(max_depth, accel, 0, None, 0, 1, 0, False, no_lds=no_lds, private_walk=private_walk, soft_shadow=soft_shadow)

    def trace_rays(self, origins, dirs, max_depth=4, accel=ACCEL_BVH, want=RAY_PLANES, no_lds=False, private_walk=False,
                   soft_shadow=False):
        """p3d_trace_rays on host arrays: ray i = rayTracing(Ray(origins[i], dirs[i]), 1, 1.0), directions used as given.
        Returns the planes named in `want`: rgb32f (n, 3) UNCLAMPED, hit_id (n,), t (n,), normal (n, 3)."""
        o, d, n = _ray_arrays(origins, dirs)
        out = _ray_planes(n, want)
        r = Rays(n, o.ctypes.data if n else None, d.ctypes.data if n else None, 0)
        ro = RayOutputs(*[out[k].ctypes.data if k in out and n else None for k in RAY_PLANES], 0)
        p = self._ray_params(max_depth, accel, no_lds, private_walk, soft_shadow)
        _check(lib().p3d_trace_rays(self.h, C.byref(r), C.byref(p), C.byref(ro)), "p3d_trace_rays")
        return out

    def trace_rays_device(self, n, origin_ptr, dir_ptr, rgb32f_ptr=0, hit_ptr=0, t_ptr=0, normal_ptr=0, max_depth=4, accel=ACCEL_BVH,
                          no_lds=False, private_walk=False, soft_shadow=False):
        """Enqueue a ray stream whose rays and output planes are caller-owned DEVICE buffers (raw pointers; 0 = no such
        plane); asynchronous on the scene's stream."""
        r = Rays(int(n), origin_ptr or None, dir_ptr or None, 1)
        ro = RayOutputs(rgb32f_ptr or None, hit_ptr or None, t_ptr or None, normal_ptr or None, 1)
        p = self._ray_params(max_depth, accel, no_lds, private_walk, soft_shadow)
        _check(lib().p3d_trace_rays(self.h, C.byref(r), C.byref(p), C.byref(ro)), "p3d_trace_rays")

    def occluded(self, origins, dirs, accel=ACCEL_BVH, no_lds=False, private_walk=False):
        """p3d_occluded on host arrays: segment i = the Ray(origins[i], dirs[i]) of processLight(), ending at origins[i] +
        dirs[i].  Returns (n,) uint8: 1 where the shadow query of `accel` answers "in shadow" (NONE: direction as given, no
        distance bound; BVH and GRID: t < |dir|; GRID: a segment that misses the grid's box is in shadow)."""
        o, d, n = _ray_arrays(origins, dirs)
        out = np.zeros(n, np.uint8)
        r = Rays(n, o.ctypes.data if n else None, d.ctypes.data if n else None, 0)
        oo = OcclusionOutputs(out.ctypes.data if n else None, 0)
        p = self._ray_params(1, accel, no_lds, private_walk, False)
        _check(lib().p3d_occluded(self.h, C.byref(r), C.byref(p), C.byref(oo)), "p3d_occluded")
        return out

    def occluded_device(self, n, origin_ptr, dir_ptr, out_ptr, accel=ACCEL_BVH, no_lds=False, private_walk=False):
        """Enqueue p3d_occluded on caller-owned DEVICE buffers (raw pointers): n segments in, n bytes out; asynchronous on
        the scene's stream."""
        r = Rays(int(n), origin_ptr or None, dir_ptr or None, 1)
        oo = OcclusionOutputs(out_ptr or None, 1)
        p = self._ray_params(1, accel, no_lds, private_walk, False)
        _check(lib().p3d_occluded(self.h, C.byref(r), C.byref(p), C.byref(oo)), "p3d_occluded")

    def denoise(self, rgb32f, depth, normal, albedo, **kw):
        """p3d_denoise on host arrays: rgb32f / normal / albedo (n, H, W, 3) or (H, W, 3), depth (n, H, W) or (H, W), as
        render_aov returns them.  Keywords: iterations, sigma_depth, sigma_albedo, sigma_color (0: no colour stop),
        normal_power_log2 (defaults: the DENOISE_* constants).  Returns {"rgb32f", "rgb8"} in the shape of rgb32f."""
        p, planes, shape = _denoise_request(rgb32f, depth, normal, albedo, **kw)
        out = {"rgb32f": np.zeros(shape, np.float32), "rgb8": np.zeros(shape, np.uint8)}
        i = DenoiseInputs(*[a.ctypes.data for a in planes], 0)
        o = Outputs(out["rgb8"].ctypes.data, out["rgb32f"].ctypes.data, None, 0)
        _check(lib().p3d_denoise(self.h, C.byref(p), C.byref(i), C.byref(o)), "p3d_denoise")
        return out

    def denoise_device(self, res_x, res_y, rgb32f_ptr, depth_ptr, normal_ptr, albedo_ptr, out_rgb32f_ptr=0, out_rgb8_ptr=0,
                       n_frames=1, iterations=DENOISE_ITERATIONS, sigma_depth=DENOISE_SIGMA_DEPTH, sigma_albedo=DENOISE_SIGMA_ALBEDO,
                       sigma_color=DENOISE_SIGMA_COLOR, normal_power_log2=DENOISE_NORMAL_POWER_LOG2):
        """Enqueue p3d_denoise on caller-owned DEVICE buffers (raw pointers; an output of 0 = no such plane); asynchronous on
        the scene's stream.  out_rgb32f_ptr may equal rgb32f_ptr."""
        p = DenoiseParams(int(res_x), int(res_y), int(n_frames), int(iterations), sigma_depth, sigma_albedo, sigma_color, int(normal_power_log2))
        i = DenoiseInputs(rgb32f_ptr or None, depth_ptr or None, normal_ptr or None, albedo_ptr or None, 1)
        o = Outputs(out_rgb8_ptr or None, out_rgb32f_ptr or None, None, 1)
        _check(lib().p3d_denoise(self.h, C.byref(p), C.byref(i), C.byref(o)), "p3d_denoise")

    def denoise_variance(self, rgb32f, depth, normal, albedo, variance, **kw):
        """p3d_denoise_variance on host arrays: DeviceScene.denoise's planes and variance (n, H, W) or (H, W), the variance
        of each pixel's luminance.  Keywords as denoise(); sigma_color (default VARIANCE_SIGMA_COLOR) is the colour stop's
        width in standard deviations and must be positive.  Returns {"rgb32f", "rgb8", "variance"}."""
        p, planes, out = _denoise_variance_request(rgb32f, depth, normal, albedo, variance, **kw)
        i = DenoiseVarianceInputs(*[a.ctypes.data for a in planes], 0)
        o = DenoiseVarianceOutputs(out["rgb8"].ctypes.data, out["rgb32f"].ctypes.data, out["variance"].ctypes.data, 0)
        _check(lib().p3d_denoise_variance(self.h, C.byref(p), C.byref(i), C.byref(o)), "p3d_denoise_variance")
        return out

    def denoise_variance_device(self, res_x, res_y, rgb32f_ptr, depth_ptr, normal_ptr, albedo_ptr, variance_ptr, out_rgb32f_ptr=0,
                                out_rgb8_ptr=0, out_variance_ptr=0, n_frames=1, iterations=DENOISE_ITERATIONS,
                                sigma_depth=DENOISE_SIGMA_DEPTH, sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_color=VARIANCE_SIGMA_COLOR,
                                normal_power_log2=DENOISE_NORMAL_POWER_LOG2):
        """Enqueue p3d_denoise_variance on caller-owned DEVICE buffers (raw pointers; an output of 0 = no such plane);
        asynchronous on the scene's stream.  out_rgb32f_ptr may equal rgb32f_ptr, out_variance_ptr may equal variance_ptr."""
        p = DenoiseParams(int(res_x), int(res_y), int(n_frames), int(iterations), sigma_depth, sigma_albedo, sigma_color, int(normal_power_log2))
        i = DenoiseVarianceInputs(rgb32f_ptr or None, depth_ptr or None, normal_ptr or None, albedo_ptr or None, variance_ptr or None, 1)
        o = DenoiseVarianceOutputs(out_rgb8_ptr or None, out_rgb32f_ptr or None, out_variance_ptr or None, 1)
        _check(lib().p3d_denoise_variance(self.h, C.byref(p), C.byref(i), C.byref(o)), "p3d_denoise_variance")

    def upsample(self, low, low_depth, low_normal, depth, normal, **kw):
        """p3d_upsample on host arrays: low (n, h, w[, 3]) or (h, w[, 3]) with low_depth / low_normal, the planes it was
        computed on, and depth / normal of the full frame, (n, h s, w s[, 3]) -- the factor s is read from the shapes.
        Keywords: sigma_depth, normal_power_log2 (defaults: the UPSAMPLE_* constants).  Returns {"plane", "fallback"}: the
        signal at the full resolution in the layout of low, and one byte per pixel, 1 where no low sample explained it."""
        p, planes, out = _upsample_request(low, low_depth, low_normal, depth, normal, **kw)
        i = UpsampleInputs(*[a.ctypes.data for a in planes], 0)
        o = UpsampleOutputs(out["plane"].ctypes.data, out["fallback"].ctypes.data, 0)
        _check(lib().p3d_upsample(self.h, C.byref(p), C.byref(i), C.byref(o)), "p3d_upsample")
        return out

    def upsample_device(self, res_x, res_y, factor, low_ptr, low_depth_ptr, low_normal_ptr, depth_ptr, normal_ptr, out_plane_ptr=0,
                        out_fallback_ptr=0, n_frames=1, channels=1, sigma_depth=UPSAMPLE_SIGMA_DEPTH,
                        normal_power_log2=UPSAMPLE_NORMAL_POWER_LOG2):
        """Enqueue p3d_upsample on caller-owned DEVICE buffers (raw pointers; an output of 0 = no such plane); res_x, res_y are
        the LOW resolution; asynchronous on the scene's stream."""
        p = UpsampleParams(int(res_x), int(res_y), int(factor), int(n_frames), int(channels), sigma_depth, int(normal_power_log2))
        i = UpsampleInputs(low_ptr or None, low_depth_ptr or None, low_normal_ptr or None, depth_ptr or None, normal_ptr or None, 1)
        o = UpsampleOutputs(out_plane_ptr or None, out_fallback_ptr or None, 1)
        _check(lib().p3d_upsample(self.h, C.byref(p), C.byref(i), C.byref(o)), "p3d_upsample")

    def accumulate(self, rgb32f, depth, normal, cams, hit_id=None, history=None, **kw):
        """p3d_accumulate on host arrays: the frames of a sequence, rgb32f / normal (n, H, W, 3) or (H, W, 3), depth and hit_id
        (n, H, W) or (H, W) as render_aov returns them, cams one Camera per frame.  history: None, or a dict with rgb32f,
        depth, normal, length and cam (optionally hit_id) of the frame before frame 0 -- the previous call's outputs and
        that frame's planes.  Keywords: depth_tolerance, normal_min, max_history (defaults: the ACCUMULATE_* constants).
        Returns {"rgb32f", "length"}: the accumulated colour in the shape of rgb32f and the history length per pixel."""
        p, fr, hi, out, keep = _accumulate_request(rgb32f, depth, normal, cams, hit_id, history, **kw)
        o = AccumulateOutputs(out["rgb32f"].ctypes.data, out["length"].ctypes.data, 0)
        _check(lib().p3d_accumulate(self.h, C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(o)), "p3d_accumulate")
        return out

    def accumulate_device(self, res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr=0, out_rgb32f_ptr=0, out_length_ptr=0,
                          history=None, depth_tolerance=ACCUMULATE_DEPTH_TOLERANCE, normal_min=ACCUMULATE_NORMAL_MIN,
                          max_history=ACCUMULATE_MAX_HISTORY):
        """Enqueue p3d_accumulate on caller-owned DEVICE buffers (raw pointers; 0 = no such plane) holding len(cams) frames;
        asynchronous on the scene's stream.  history: None, or a dict of device pointers rgb32f, depth, normal, length
        (optionally hit_id) and the host Camera cam.  out_rgb32f_ptr may equal rgb32f_ptr."""
        p, fr, hi, mo, keep = _accumulate_device_structs(res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr, history, None,
                                                         depth_tolerance, normal_min, max_history)
        o = AccumulateOutputs(out_rgb32f_ptr or None, out_length_ptr or None, 1)
        _check(lib().p3d_accumulate(self.h, C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(o)), "p3d_accumulate")

    def accumulate_moving(self, rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history=None, prev_xy=True, **kw):
        """p3d_accumulate_moving on host arrays: DeviceScene.accumulate for a sequence whose primitives moved between the frames.
        hit_id is needed; prim_type (n_prims,) and prim_data (n, n_prims, 12) or (n_prims, 12) are the geometry every frame was
        rendered with, as DeviceScene.update takes it; a history also carries prim_data, the (n_prims, 12) records it was
        rendered with.  Returns {"rgb32f", "length"} and, with prev_xy, "prev_xy" (n, H, W, 2): where each pixel's surface
        point was in the frame before (NaN where there is none)."""
        p, fr, hi, mo, out, keep = _accumulate_moving_request(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history, prev_xy, **kw)
        o = AccumulateMovingOutputs(out["rgb32f"].ctypes.data, out["length"].ctypes.data, out["prev_xy"].ctypes.data if prev_xy else None, 0)
        _check(lib().p3d_accumulate_moving(self.h, C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(mo), C.byref(o)),
               "p3d_accumulate_moving")
        return out

    def accumulate_moving_device(self, res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr, n_prims, prim_type_ptr, prim_data_ptr,
                                 out_rgb32f_ptr=0, out_length_ptr=0, out_prev_xy_ptr=0, history=None,
                                 depth_tolerance=ACCUMULATE_DEPTH_TOLERANCE, normal_min=ACCUMULATE_NORMAL_MIN, max_history=ACCUMULATE_MAX_HISTORY):
        """Enqueue p3d_accumulate_moving on caller-owned DEVICE buffers (raw pointers; 0 = no such plane) holding len(cams)
        frames and their geometry; asynchronous on the scene's stream.  history: None, or a dict of device pointers rgb32f,
        depth, normal, length, prim_data (optionally hit_id) and the host Camera cam.  out_rgb32f_ptr may equal rgb32f_ptr."""
        motion = dict(n_prims=n_prims, prim_type=prim_type_ptr, prim_data=prim_data_ptr)
        p, fr, hi, mo, keep = _accumulate_device_structs(res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr, history, motion,
                                                         depth_tolerance, normal_min, max_history)
        o = AccumulateMovingOutputs(out_rgb32f_ptr or None, out_length_ptr or None, out_prev_xy_ptr or None, 1)
        _check(lib().p3d_accumulate_moving(self.h, C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(mo), C.byref(o)),
               "p3d_accumulate_moving")

    def accumulate_variance(self, rgb32f, depth, normal, cams, hit_id=None, history=None, motion=None, **kw):
        """p3d_accumulate_variance on host arrays: DeviceScene.accumulate -- or, with motion = dict(prim_type, prim_data),
        DeviceScene.accumulate_moving -- that also carries the luminance moments.  A history also carries "moments" (H, W, 2),
        the moments output of the frame it describes (and "prim_data" with a motion).  Keywords: accumulate's, and
        min_temporal, radius, sigma_depth, normal_power_log2 (defaults: the VARIANCE_* constants).  Returns {"rgb32f",
        "length", "moments" (n, H, W, 2), "variance" (n, H, W)} and, with a motion, "prev_xy"."""
        p, vp, fr, hi, hm, mo, out, keep = _accumulate_variance_request(rgb32f, depth, normal, cams, hit_id, history, motion, **kw)
        o = AccumulateVarianceOutputs(*[out[k].ctypes.data if k in out else None for k in _VARIANCE_PLANES], 0)
        _check(lib().p3d_accumulate_variance(self.h, C.byref(p), C.byref(vp), C.byref(fr), C.byref(hi) if hi else None, hm,
                                             C.byref(mo) if mo else None, C.byref(o)), "p3d_accumulate_variance")
        return out

    def accumulate_variance_device(self, res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr=0, out_rgb32f_ptr=0, out_length_ptr=0,
                                   out_moments_ptr=0, out_variance_ptr=0, out_prev_xy_ptr=0, history=None, motion=None,
                                   depth_tolerance=ACCUMULATE_DEPTH_TOLERANCE, normal_min=ACCUMULATE_NORMAL_MIN, max_history=ACCUMULATE_MAX_HISTORY,
                                   min_temporal=VARIANCE_MIN_TEMPORAL, radius=VARIANCE_RADIUS, sigma_depth=VARIANCE_SIGMA_DEPTH,
                                   normal_power_log2=VARIANCE_NORMAL_POWER_LOG2):
        """Enqueue p3d_accumulate_variance on caller-owned DEVICE buffers (raw pointers; 0 = no such plane) holding len(cams)
        frames; asynchronous on the scene's stream.  history: None, or a dict of device pointers rgb32f, depth, normal, length,
        moments (optionally hit_id; prim_data with a motion) and the host Camera cam.  motion: None, or a dict of n_prims and
        the device pointers prim_type, prim_data.  out_rgb32f_ptr may equal rgb32f_ptr."""
        p, fr, hi, mo, keep = _accumulate_device_structs(res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr, history, motion,
                                                         depth_tolerance, normal_min, max_history)
        vp = AccumulateVarianceParams(min_temporal, int(radius), sigma_depth, int(normal_power_log2))
        o = AccumulateVarianceOutputs(out_rgb32f_ptr or None, out_length_ptr or None, out_moments_ptr or None, out_variance_ptr or None,
                                      out_prev_xy_ptr or None, 1)
        _check(lib().p3d_accumulate_variance(self.h, C.byref(p), C.byref(vp), C.byref(fr), C.byref(hi) if hi else None,
                                             (history or {}).get("moments") or None, C.byref(mo) if mo else None, C.byref(o)),
               "p3d_accumulate_variance")

    def ambient_occlusion(self, cam_or_cams, depth, normal, rgb32f=None, samples=AO_SAMPLES, radius=AO_RADIUS, bias=AO_BIAS, seed=0,
                          accel=ACCEL_BVH, no_lds=False, private_walk=False, want=("ao", "rgb32f")):
        """p3d_ambient_occlusion on host arrays: depth (n, H, W) or (H, W) and normal (n, H, W, 3) or (H, W, 3) as render_aov
        returns them, seen through one Camera or a sequence of n; rgb32f (optional) is the colour to modulate.  Returns
        the planes named in `want`: ao (n, H, W) and rgb32f (n, H, W, 3) -- ao * rgb32f, or (ao, ao, ao) without a colour."""
        arr, n = _camera_array([cam_or_cams] if isinstance(cam_or_cams, Camera) else cam_or_cams)
        H, W = arr[0].res_y, arr[0].res_x
        depth = np.ascontiguousarray(depth, np.float32).reshape(n, H, W)
        normal = np.ascontiguousarray(normal, np.float32).reshape(n, H, W, 3)
        if rgb32f is not None:
            rgb32f = np.ascontiguousarray(rgb32f, np.float32).reshape(n, H, W, 3)
        out = {}
        if "ao" in want:
            out["ao"] = np.zeros((n, H, W), np.float32)
        if "rgb32f" in want:
            out["rgb32f"] = np.zeros((n, H, W, 3), np.float32)
        p = self._ray_params(1, accel, no_lds, private_walk, False)
        a = AoParams(int(samples), radius, bias, int(seed) & 0xFFFFFFFF)
        i = AoInputs(depth.ctypes.data, normal.ctypes.data, rgb32f.ctypes.data if rgb32f is not None else None, 0)
        o = AoOutputs(out["ao"].ctypes.data if "ao" in out else None, out["rgb32f"].ctypes.data if "rgb32f" in out else None, 0)
        _check(lib().p3d_ambient_occlusion(self.h, arr, n, C.byref(p), C.byref(a), C.byref(i), C.byref(o)), "p3d_ambient_occlusion")
        return out

    def ambient_occlusion_device(self, cam_or_cams, depth_ptr, normal_ptr, rgb32f_ptr=0, out_ao_ptr=0, out_rgb32f_ptr=0, samples=AO_SAMPLES,
                                 radius=AO_RADIUS, bias=AO_BIAS, seed=0, accel=ACCEL_BVH, no_lds=False, private_walk=False):
        """Enqueue p3d_ambient_occlusion on caller-owned DEVICE buffers (raw pointers; 0 = no such plane) holding one frame per
        camera; asynchronous on the scene's stream."""
        arr, n = _camera_array([cam_or_cams] if isinstance(cam_or_cams, Camera) else cam_or_cams)
        p = self._ray_params(1, accel, no_lds, private_walk, False)
        a = AoParams(int(samples), radius, bias, int(seed) & 0xFFFFFFFF)
        i = AoInputs(depth_ptr or None, normal_ptr or None, rgb32f_ptr or None, 1)
        o = AoOutputs(out_ao_ptr or None, out_rgb32f_ptr or None, 1)
        _check(lib().p3d_ambient_occlusion(self.h, arr, n, C.byref(p), C.byref(a), C.byref(i), C.byref(o)), "p3d_ambient_occlusion")

    def indirect_diffuse(self, cam_or_cams, depth, normal, albedo=None, rgb32f=None, samples=INDIRECT_SAMPLES, bias=INDIRECT_BIAS, seed=0,
                         accel=ACCEL_BVH, no_lds=False, private_walk=False, want=("indirect", "rgb32f"), bounces=None):
        """p3d_indirect_diffuse on host arrays (bounces: see indirect_paths): depth (n, H, W) or (H, W) and normal (n, H, W, 3) or (H, W, 3) as render_aov
        returns them, seen through one Camera or a sequence of n; albedo and rgb32f (both optional) are the planes the
        gathered light is multiplied by and added to.  Returns the planes named in `want`: indirect (n, H, W, 3), the mean
        radiance of the samples, and rgb32f (n, H, W, 3) = rgb32f + albedo * indirect."""
        arr, n = _camera_array([cam_or_cams] if isinstance(cam_or_cams, Camera) else cam_or_cams)
        H, W = arr[0].res_y, arr[0].res_x
        depth = np.ascontiguousarray(depth, np.float32).reshape(n, H, W)
        normal = np.ascontiguousarray(normal, np.float32).reshape(n, H, W, 3)
        if albedo is not None:
            albedo = np.ascontiguousarray(albedo, np.float32).reshape(n, H, W, 3)
        if rgb32f is not None:
            rgb32f = np.ascontiguousarray(rgb32f, np.float32).reshape(n, H, W, 3)
        out = {k: np.zeros((n, H, W, 3), np.float32) for k in ("indirect", "rgb32f") if k in want}
        p = self._ray_params(1, accel, no_lds, private_walk, False)
        i = IndirectInputs(depth.ctypes.data, normal.ctypes.data, albedo.ctypes.data if albedo is not None else None,
                           rgb32f.ctypes.data if rgb32f is not None else None, 0)
        o = IndirectOutputs(out["indirect"].ctypes.data if "indirect" in out else None, out["rgb32f"].ctypes.data if "rgb32f" in out else None, 0)
        self._indirect_call(arr, n, p, samples, bias, seed, bounces, i, o)
        return out

    def _indirect_call(self, arr, n, p, samples, bias, seed, bounces, i, o):
        """p3d_indirect_diffuse (bounces None) or p3d_indirect_paths on filled input and output structs."""
        if bounces is None:
            g = IndirectParams(int(samples), bias, int(seed) & 0xFFFFFFFF)
            _check(lib().p3d_indirect_diffuse(self.h, arr, n, C.byref(p), C.byref(g), C.byref(i), C.byref(o)), "p3d_indirect_diffuse")
        else:
            g = PathParams(int(samples), int(bounces), bias, int(seed) & 0xFFFFFFFF)
            _check(lib().p3d_indirect_paths(self.h, arr, n, C.byref(p), C.byref(g), C.byref(i), C.byref(o)), "p3d_indirect_paths")

    def indirect_diffuse_device(self, cam_or_cams, depth_ptr, normal_ptr, albedo_ptr=0, rgb32f_ptr=0, out_indirect_ptr=0, out_rgb32f_ptr=0,
                                samples=INDIRECT_SAMPLES, bias=INDIRECT_BIAS, seed=0, accel=ACCEL_BVH, no_lds=False, private_walk=False,
                                bounces=None):
        """Enqueue p3d_indirect_diffuse on caller-owned DEVICE buffers (raw pointers; 0 = no such plane) holding one frame per
        camera; asynchronous on the scene's stream.  (bounces: see indirect_paths_device.)"""
        arr, n = _camera_array([cam_or_cams] if isinstance(cam_or_cams, Camera) else cam_or_cams)
        p = self._ray_params(1, accel, no_lds, private_walk, False)
        i = IndirectInputs(depth_ptr or None, normal_ptr or None, albedo_ptr or None, rgb32f_ptr or None, 1)
        o = IndirectOutputs(out_indirect_ptr or None, out_rgb32f_ptr or None, 1)
        self._indirect_call(arr, n, p, samples, bias, seed, bounces, i, o)

    def indirect_paths(self, cam_or_cams, depth, normal, albedo=None, rgb32f=None, samples=INDIRECT_SAMPLES, bounces=PATH_BOUNCES,
                       bias=INDIRECT_BIAS, seed=0, accel=ACCEL_BVH, no_lds=False, private_walk=False, want=("indirect", "rgb32f")):
        """p3d_indirect_paths on host arrays: indirect_diffuse's arguments and result, with `samples` paths per pixel of at most
        `bounces` (1 .. 8) rays each; bounces = 1 gives indirect_diffuse's bits."""
        return self.indirect_diffuse(cam_or_cams, depth, normal, albedo, rgb32f, samples, bias, seed, accel, no_lds, private_walk, want,
                                     bounces=int(bounces))

    def indirect_paths_device(self, cam_or_cams, depth_ptr, normal_ptr, albedo_ptr=0, rgb32f_ptr=0, out_indirect_ptr=0, out_rgb32f_ptr=0,
                              samples=INDIRECT_SAMPLES, bounces=PATH_BOUNCES, bias=INDIRECT_BIAS, seed=0, accel=ACCEL_BVH, no_lds=False,
                              private_walk=False):
        """Enqueue p3d_indirect_paths on caller-owned DEVICE buffers: indirect_diffuse_device's arguments, plus bounces."""
        self.indirect_diffuse_device(cam_or_cams, depth_ptr, normal_ptr, albedo_ptr, rgb32f_ptr, out_indirect_ptr, out_rgb32f_ptr, samples, bias,
                                     seed, accel, no_lds, private_walk, bounces=int(bounces))

    def deinterleave_frames(self, gathered_ptr, frames_ptr, res_x, res_y, row_block, world, bpp, n_frames,
                            rank_stride_bytes=0, tile_stride_bytes=0, frame_stride_bytes=0):
        L = lib()
        L.p3d_deinterleave_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.c_int32, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint64]
        _check(L.p3d_deinterleave_frames(self.h, C.c_void_p(gathered_ptr), C.c_void_p(frames_ptr), res_x, res_y, row_block,
                                         world, bpp, int(rank_stride_bytes), int(n_frames), int(tile_stride_bytes),
                                         int(frame_stride_bytes)), "p3d_deinterleave_frames")

    def deinterleave(self, gathered_ptr, frame_ptr, res_x, res_y, row_block, world, bpp, rank_stride_bytes=0):
        _check(lib().p3d_deinterleave(self.h, C.c_void_p(gathered_ptr), C.c_void_p(frame_ptr), res_x, res_y,
                                      row_block, world, bpp, int(rank_stride_bytes)), "p3d_deinterleave")


def _camera_array(cams):
    """A sequence of Camera structs -> (ctypes Camera array, n).  n == 0 is passed on: the library refuses it."""
    cams = list(cams)
    return (Camera * max(len(cams), 1))(*cams), len(cams)


def tune_schedule(handles, cam, rgb8_ptrs, frames=3, **kw):
    """p3d_tune_schedule over DeviceScene handles (one stream each): measure the schedule candidates with all of them in
    flight and adopt the fastest.  rgb8_ptrs: one device buffer per handle.  kw as for render_device.
    -> (best, [ms per frame of the six candidates]); best = -1: nothing to choose (rule or flag)."""
    n = len(handles)
    assert n >= 1 and len(rgb8_ptrs) == n
    k = dict(max_depth=4, accel=ACCEL_BVH, spp=0, samples=None, rank=0, world=1, row_block=16, counters=False, tree=False,
             no_lds=False, profile=False, wavefront=False, soft_shadow=False, fuzzy_reflection=False, seed=0, tile=False,
             samples_ptr=0, packet=False, private_walk=False, skybox=False, schlick=False)
    k.update(kw)
    p = handles[0]._params(k["max_depth"], k["accel"], k["spp"], k["samples"], k["rank"], k["world"], k["row_block"], k["counters"],
                           k["tree"], k["no_lds"], k["profile"], k["wavefront"], k["soft_shadow"], k["fuzzy_reflection"], k["seed"],
                           k["tile"], k["samples_ptr"], k["packet"], k["private_walk"], k["skybox"], k["schlick"])
    hs = (C.c_void_p * n)(*[h.h.value if isinstance(h.h, C.c_void_p) else h.h for h in handles])
    outs = (Outputs * n)(*[Outputs(int(q) or None, None, None, 1) for q in rgb8_ptrs])
    ms = (C.c_float * 6)()
    best = C.c_int32(-1)
    _check(lib().p3d_tune_schedule(hs, n, C.byref(cam), C.byref(p), outs, int(frames), ms, C.byref(best)), "p3d_tune_schedule")
    return int(best.value), [float(v) for v in ms]


COMM_ID_BYTES = 128


def comm_unique_id():
    """128 bytes rank 0 hands to the other ranks (ncclGetUniqueId behind the C-ABI)."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    _check(lib().p3d_comm_unique_id(buf), "p3d_comm_unique_id")
    return bytes(buf)


class Comm:
    """p3d_comm: one rank of the RCCL group the frame's gather runs on (include/p3d_hip.h)."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def create(cls, unique_id, rank, world, device):
        """One process per GPU: every rank calls this with rank 0's comm_unique_id() bytes."""
        h = C.c_void_p()
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(unique_id) if unique_id is not None else None
        _check(lib().p3d_comm_create(buf, int(rank), int(world), int(device), C.byref(h)), "p3d_comm_create")
        return cls(h.value)

    @classmethod
    def create_all(cls, devices):
        """One process driving len(devices) GPUs: returns the ranks in order."""
        n = len(devices)
        devs = (C.c_int * max(n, 1))(*devices)
        hs = (C.c_void_p * max(n, 1))()
        _check(lib().p3d_comm_create_all(devs, n, hs), "p3d_comm_create_all")
        return [cls(hs[i]) for i in range(n)]

    def info(self):
        r, w, d = C.c_int(), C.c_int(), C.c_int()
        _check(lib().p3d_comm_info(self.h, C.byref(r), C.byref(w), C.byref(d)), "p3d_comm_info")
        return r.value, w.value, d.value

    def gather(self, scene, tile_ptr, gathered_ptr, tile_bytes):
        """Enqueue this rank's part of the frame gather on `scene`'s stream (device pointers)."""
        _check(lib().p3d_gather(self.h, scene.h, C.c_void_p(tile_ptr), C.c_void_p(gathered_ptr or None),
                                int(tile_bytes)), "p3d_gather")

    def pt_reduce_sum(self, pt, linear_ptr, count):
        _check(lib().p3d_pt_reduce_sum(self.h, pt.h, C.c_void_p(linear_ptr), int(count)), "p3d_pt_reduce_sum")

    def close(self):
        if self.h:
            lib().p3d_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gather_all(comms, scenes, tile_ptrs, gathered_ptr, tile_bytes):
    """All ranks of a Comm.create_all() group from one thread (their sends / receives share one RCCL group)."""
    n = len(comms)
    cs = (C.c_void_p * n)(*[c.h.value for c in comms])
    ss = (C.c_void_p * n)(*[s.h.value for s in scenes])
    ts = (C.c_void_p * n)(*[int(t) for t in tile_ptrs])
    _check(lib().p3d_gather_all(cs, ss, ts, n, C.c_void_p(gathered_ptr), int(tile_bytes)), "p3d_gather_all")


def debug_intersect(ptype, prim12, origin, direction, device=0):
    """Device intersectors on n (ray, primitive) pairs -> (hit[n] bool, t[n], normal[n,3]).  ptype: 0 sphere, 1 triangle,
    2 box, 3 plane (prim12 = unit normal, D), 4 = a triangle through hit_triangle<true>, the frcp() form of the test that
    scenes read from HBM use."""
    ptype = np.ascontiguousarray(ptype, np.uint32)
    prim12 = np.ascontiguousarray(prim12, np.float32).reshape(-1, 12)
    origin = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    n = len(ptype)
    hit = np.zeros(n, np.int32)
    t = np.zeros(n, np.float32)
    nrm = np.zeros((n, 3), np.float32)
    _check(lib().p3d_debug_intersect(int(device), n, ptype.ctypes.data, prim12.ctypes.data, origin.ctypes.data,
                                     direction.ctypes.data, hit.ctypes.data, t.ctypes.data, nrm.ctypes.data),
           "p3d_debug_intersect")
    return hit.astype(bool), t, nrm


def debug_powf(x, y, device=0):
    """The device's restatement of the host libm's powf (csrc/p3d_powf.h) on n argument pairs."""
    x = np.ascontiguousarray(x, np.float32).ravel()
    y = np.ascontiguousarray(y, np.float32).ravel()
    assert x.shape == y.shape
    out = np.zeros_like(x)
    _check(lib().p3d_debug_powf(int(device), len(x), x.ctypes.data, y.ctypes.data, out.ctypes.data), "p3d_debug_powf")
    return out


def debug_rand(seed, first, n, device=0):
    """The device's restatement of libc's rand() (csrc/p3d_rand.h): values number first .. first + n - 1 after srand(seed)."""
    out = np.zeros(int(n), np.uint32)
    _check(lib().p3d_debug_rand(int(device), int(seed) & 0xFFFFFFFF, int(first), int(n), out.ctypes.data if n else None), "p3d_debug_rand")
    return out


def debug_sample_stream(seed, res_x, res_y, spp, aperture, pairs_per_pass=0, device=0):
    """The generator of p3d_generate_samples with every pass forced to pairs_per_pass pairs of draws (0: its own sizing).
    -> (samples (res_y, res_x, spp*spp, 4), passes that ran)."""
    out = np.zeros((int(res_y), int(res_x), int(spp) * int(spp), 4), np.float32)
    passes = C.c_int32(0)
    _check(lib().p3d_debug_sample_stream(int(device), int(seed) & 0xFFFFFFFF, int(res_x), int(res_y), int(spp), float(aperture),
                                         int(pairs_per_pass), out.ctypes.data if out.size else None, C.byref(passes)), "p3d_debug_sample_stream")
    return out, int(passes.value)


def _denoise_request(rgb32f, depth, normal, albedo, iterations=DENOISE_ITERATIONS, sigma_depth=DENOISE_SIGMA_DEPTH,
                     sigma_albedo=DENOISE_SIGMA_ALBEDO, sigma_color=DENOISE_SIGMA_COLOR, normal_power_log2=DENOISE_NORMAL_POWER_LOG2):
    """Host planes of one frame (H, W[, 3]) or n frames (n, H, W[, 3]) -> (DenoiseParams, contiguous float32 planes, shape of rgb32f)."""
    c = np.ascontiguousarray(rgb32f, np.float32)
    if c.ndim not in (3, 4) or c.shape[-1] != 3:
        raise ValueError("rgb32f must be (H, W, 3) or (n, H, W, 3)")
    n, (h, w) = (1 if c.ndim == 3 else c.shape[0]), c.shape[-3:-1]
    z = np.ascontiguousarray(depth, np.float32)
    nr = np.ascontiguousarray(normal, np.float32)
    al = np.ascontiguousarray(albedo, np.float32)
    if z.size != n * h * w or nr.size != c.size or al.size != c.size:
        raise ValueError("depth, normal and albedo must match rgb32f")
    p = DenoiseParams(w, h, n, int(iterations), sigma_depth, sigma_albedo, sigma_color, int(normal_power_log2))
    return p, (c, z, nr, al), c.shape


def host_denoise(rgb32f, depth, normal, albedo, **kw):
    """p3dh_denoise: the host layer's restatement of p3d_denoise, every bit of it, on host arrays (no GPU).  Arguments and
    result as DeviceScene.denoise."""
    p, planes, shape = _denoise_request(rgb32f, depth, normal, albedo, **kw)
    out = {"rgb32f": np.zeros(shape, np.float32), "rgb8": np.zeros(shape, np.uint8)}
    lib().p3dh_denoise(C.byref(p), *[a.ctypes.data for a in planes], out["rgb32f"].ctypes.data, out["rgb8"].ctypes.data)
    return out


def debug_denoise(rgb32f, depth, normal, albedo, device=0, **kw):
    """p3d_debug_denoise: the launches of p3d_denoise over host arrays, without a scene.  Arguments and result as
    DeviceScene.denoise."""
    p, planes, shape = _denoise_request(rgb32f, depth, normal, albedo, **kw)
    out = {"rgb32f": np.zeros(shape, np.float32), "rgb8": np.zeros(shape, np.uint8)}
    i = DenoiseInputs(*[a.ctypes.data for a in planes], 0)
    o = Outputs(out["rgb8"].ctypes.data, out["rgb32f"].ctypes.data, None, 0)
    _check(lib().p3d_debug_denoise(int(device), C.byref(p), C.byref(i), C.byref(o)), "p3d_debug_denoise")
    return out


def _upsample_request(low, low_depth, low_normal, depth, normal, sigma_depth=UPSAMPLE_SIGMA_DEPTH,
                      normal_power_log2=UPSAMPLE_NORMAL_POWER_LOG2):
    """Host planes of one frame or n frames -> (UpsampleParams, the five contiguous float32 planes, the zeroed outputs)."""
    lz = np.ascontiguousarray(low_depth, np.float32)
    z = np.ascontiguousarray(depth, np.float32)
    if lz.ndim not in (2, 3) or z.ndim != lz.ndim:
        raise ValueError("low_depth and depth must both be (h, w) or (n, h, w)")
    n, (h, w), (H, W) = (1 if lz.ndim == 2 else lz.shape[0]), lz.shape[-2:], z.shape[-2:]
    s = W // w if w else 0
    if s < 1 or (W, H) != (w * s, h * s) or (z.ndim == 3 and z.shape[0] != n):
        raise ValueError("depth must be low_depth's shape times one integer factor")
    lo = np.ascontiguousarray(low, np.float32)
    c = 3 if lo.ndim == lz.ndim + 1 else 1
    ln = np.ascontiguousarray(low_normal, np.float32)
    nr = np.ascontiguousarray(normal, np.float32)
    if lo.size != lz.size * c or (c == 3 and lo.shape[-1] != 3) or ln.size != lz.size * 3 or nr.size != z.size * 3:
        raise ValueError("low must be low_depth's shape (optionally with 3 channels), the normals their depth's shape with 3")
    p = UpsampleParams(w, h, s, n, c, sigma_depth, int(normal_power_log2))
    out = {"plane": np.zeros(z.shape + ((3,) if c == 3 else ()), np.float32), "fallback": np.zeros(z.shape, np.uint8)}
    return p, (lo, lz, ln, z, nr), out


def host_upsample(low, low_depth, low_normal, depth, normal, **kw):
    """p3dh_upsample: the host layer's restatement of p3d_upsample, every bit of it, on host arrays (no GPU).  Arguments and
    result as DeviceScene.upsample."""
    p, planes, out = _upsample_request(low, low_depth, low_normal, depth, normal, **kw)
    lib().p3dh_upsample(C.byref(p), *[a.ctypes.data for a in planes], out["plane"].ctypes.data, out["fallback"].ctypes.data)
    return out


def debug_upsample(low, low_depth, low_normal, depth, normal, device=0, **kw):
    """p3d_debug_upsample: the launch of p3d_upsample over host arrays, without a scene.  Arguments and result as
    DeviceScene.upsample."""
    p, planes, out = _upsample_request(low, low_depth, low_normal, depth, normal, **kw)
    i = UpsampleInputs(*[a.ctypes.data for a in planes], 0)
    o = UpsampleOutputs(out["plane"].ctypes.data, out["fallback"].ctypes.data, 0)
    _check(lib().p3d_debug_upsample(int(device), C.byref(p), C.byref(i), C.byref(o)), "p3d_debug_upsample")
    return out


def _denoise_variance_request(rgb32f, depth, normal, albedo, variance, sigma_color=VARIANCE_SIGMA_COLOR, **kw):
    """_denoise_request with the variance plane -> (DenoiseParams, the five contiguous planes, the zeroed outputs)."""
    p, planes, shape = _denoise_request(rgb32f, depth, normal, albedo, sigma_color=sigma_color, **kw)
    v = np.ascontiguousarray(variance, np.float32)
    if v.size != planes[1].size:
        raise ValueError("variance must match depth")
    out = {"rgb32f": np.zeros(shape, np.float32), "rgb8": np.zeros(shape, np.uint8), "variance": np.zeros(shape[:-1], np.float32)}
    return p, planes + (v,), out


def host_denoise_variance(rgb32f, depth, normal, albedo, variance, **kw):
    """p3dh_denoise_variance: the host layer's restatement of p3d_denoise_variance, every bit of it, on host arrays (no GPU).
    Arguments and result as DeviceScene.denoise_variance."""
    p, planes, out = _denoise_variance_request(rgb32f, depth, normal, albedo, variance, **kw)
    lib().p3dh_denoise_variance(C.byref(p), *[a.ctypes.data for a in planes], out["rgb32f"].ctypes.data, out["rgb8"].ctypes.data,
                                out["variance"].ctypes.data)
    return out


def debug_denoise_variance(rgb32f, depth, normal, albedo, variance, device=0, **kw):
    """p3d_debug_denoise_variance: the launches of p3d_denoise_variance over host arrays, without a scene.  Arguments and
    result as DeviceScene.denoise_variance."""
    p, planes, out = _denoise_variance_request(rgb32f, depth, normal, albedo, variance, **kw)
    i = DenoiseVarianceInputs(*[a.ctypes.data for a in planes], 0)
    o = DenoiseVarianceOutputs(out["rgb8"].ctypes.data, out["rgb32f"].ctypes.data, out["variance"].ctypes.data, 0)
    _check(lib().p3d_debug_denoise_variance(int(device), C.byref(p), C.byref(i), C.byref(o)), "p3d_debug_denoise_variance")
    return out


def _accumulate_device_structs(res_x, res_y, cams, rgb32f_ptr, depth_ptr, normal_ptr, hit_ptr, history, motion, depth_tolerance, normal_min,
                               max_history):
    """The structs the three accumulate_*_device methods share, over DEVICE pointers (0 = no such plane) -> (AccumulateParams,
    AccumulateFrames, AccumulateHistory or None, AccumulateMotion or None, what must stay alive during the call).  history
    and motion: the dicts of those methods, or None."""
    arr, n = _camera_array(cams)
    p = AccumulateParams(int(res_x), int(res_y), n, depth_tolerance, normal_min, max_history)
    fr = AccumulateFrames(rgb32f_ptr or None, depth_ptr or None, normal_ptr or None, hit_ptr or None, arr, 1)
    hi = hcam = None
    if history is not None:
        hcam = (Camera * 1)(history["cam"])
        hi = AccumulateHistory(history["rgb32f"] or None, history["depth"] or None, history["normal"] or None, history["length"] or None,
                               history.get("hit_id") or None, hcam, 1)
    mo = None
    if motion is not None:
        mo = AccumulateMotion(int(motion["n_prims"]), motion["prim_type"] or None, motion["prim_data"] or None,
                              (history or {}).get("prim_data") or None, 1)
    return p, fr, hi, mo, (arr, hcam)


def _accumulate_request(rgb32f, depth, normal, cams, hit_id=None, history=None, depth_tolerance=ACCUMULATE_DEPTH_TOLERANCE,
                        normal_min=ACCUMULATE_NORMAL_MIN, max_history=ACCUMULATE_MAX_HISTORY):
    """Host planes of one frame (H, W[, 3]) or n frames (n, H, W[, 3]) and their cameras -> (AccumulateParams, AccumulateFrames,
    AccumulateHistory or None, the zeroed outputs {"rgb32f", "length"}, what must stay alive while the structs are used)."""
    c = np.ascontiguousarray(rgb32f, np.float32)
    if c.ndim not in (3, 4) or c.shape[-1] != 3:
        raise ValueError("rgb32f must be (H, W, 3) or (n, H, W, 3)")
    n, (h, w) = (1 if c.ndim == 3 else c.shape[0]), c.shape[-3:-1]
    z = np.ascontiguousarray(depth, np.float32)
    nr = np.ascontiguousarray(normal, np.float32)
    hid = None if hit_id is None else np.ascontiguousarray(hit_id, np.int32)
    if z.size != n * h * w or nr.size != c.size or (hid is not None and hid.size != z.size):
        raise ValueError("depth, normal and hit_id must match rgb32f")
    arr, n_cams = _camera_array([cams] if isinstance(cams, Camera) else cams)
    if n_cams != n:
        raise ValueError("one camera per frame: %d frames, %d cameras" % (n, n_cams))
    p = AccumulateParams(w, h, n, depth_tolerance, normal_min, max_history)
    fr = AccumulateFrames(c.ctypes.data, z.ctypes.data, nr.ctypes.data, None if hid is None else hid.ctypes.data, arr, 0)
    keep = [c, z, nr, hid, arr]
    hi = None
    if history is not None:
        hp = [np.ascontiguousarray(history[k], np.float32) for k in ("rgb32f", "depth", "normal", "length")]
        hh = None if history.get("hit_id") is None else np.ascontiguousarray(history["hit_id"], np.int32)
        if hp[0].size != 3 * h * w or hp[1].size != h * w or hp[2].size != 3 * h * w or hp[3].size != h * w or (hh is not None and hh.size != h * w):
            raise ValueError("the history is one frame of the frames' resolution")
        hcam = (Camera * 1)(history["cam"])
        hi = AccumulateHistory(*[a.ctypes.data for a in hp], None if hh is None else hh.ctypes.data, hcam, 0)
        keep += hp + [hh, hcam]
    out = {"rgb32f": np.zeros(c.shape, np.float32), "length": np.zeros(c.shape[:-1], np.float32)}
    return p, fr, hi, out, keep


def host_accumulate(rgb32f, depth, normal, cams, hit_id=None, history=None, **kw):
    """p3dh_accumulate: the host layer's restatement of p3d_accumulate, every bit of it, on host arrays (no GPU).  Arguments
    and result as DeviceScene.accumulate."""
    p, fr, hi, out, keep = _accumulate_request(rgb32f, depth, normal, cams, hit_id, history, **kw)
    lib().p3dh_accumulate(C.byref(p), C.byref(fr), C.byref(hi) if hi else None, out["rgb32f"].ctypes.data, out["length"].ctypes.data)
    return out


def debug_accumulate(rgb32f, depth, normal, cams, hit_id=None, history=None, device=0, **kw):
    """p3d_debug_accumulate: the launches of p3d_accumulate over host arrays, without a scene.  Arguments and result as
    DeviceScene.accumulate."""
    p, fr, hi, out, keep = _accumulate_request(rgb32f, depth, normal, cams, hit_id, history, **kw)
    o = AccumulateOutputs(out["rgb32f"].ctypes.data, out["length"].ctypes.data, 0)
    _check(lib().p3d_debug_accumulate(int(device), C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(o)), "p3d_debug_accumulate")
    return out


def _accumulate_moving_request(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history=None, prev_xy=True, **kw):
    """_accumulate_request and the geometry -> (params, frames, history or None, AccumulateMotion, the zeroed outputs {"rgb32f",
    "length"[, "prev_xy"]}, what must stay alive)."""
    if hit_id is None:
        raise ValueError("accumulate_moving needs hit_id: the motion is looked up by it")
    p, fr, hi, out, keep = _accumulate_request(rgb32f, depth, normal, cams, hit_id, history, **kw)
    kind = np.ascontiguousarray(prim_type, np.uint32).reshape(-1)
    n_prims = kind.size
    data = np.ascontiguousarray(prim_data, np.float32)
    if data.size != p.n_frames * n_prims * 12:
        raise ValueError("prim_data must hold 12 floats per primitive and frame: (%d, %d, 12)" % (p.n_frames, n_prims))
    hdata = None
    if history is not None:
        hdata = np.ascontiguousarray(history["prim_data"], np.float32)
        if hdata.size != n_prims * 12:
            raise ValueError("the history's prim_data must be (%d, 12)" % n_prims)
    mo = AccumulateMotion(n_prims, kind.ctypes.data, data.ctypes.data, None if hdata is None else hdata.ctypes.data, 0)
    if prev_xy:
        out["prev_xy"] = np.zeros(out["length"].shape + (2,), np.float32)
    return p, fr, hi, mo, out, keep + [kind, data, hdata]


def host_accumulate_moving(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history=None, prev_xy=True, **kw):
    """p3dh_accumulate_moving: the host layer's restatement of p3d_accumulate_moving, every bit of it, on host arrays (no GPU).
    Arguments and result as DeviceScene.accumulate_moving."""
    p, fr, hi, mo, out, keep = _accumulate_moving_request(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history, prev_xy, **kw)
    lib().p3dh_accumulate_moving(C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(mo), out["rgb32f"].ctypes.data,
                                 out["length"].ctypes.data, out["prev_xy"].ctypes.data if prev_xy else None)
    return out


def debug_accumulate_moving(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history=None, prev_xy=True, device=0, **kw):
    """p3d_debug_accumulate_moving: the launches of p3d_accumulate_moving over host arrays, without a scene.  Arguments and result
    as DeviceScene.accumulate_moving."""
    p, fr, hi, mo, out, keep = _accumulate_moving_request(rgb32f, depth, normal, cams, hit_id, prim_type, prim_data, history, prev_xy, **kw)
    o = AccumulateMovingOutputs(out["rgb32f"].ctypes.data, out["length"].ctypes.data, out["prev_xy"].ctypes.data if prev_xy else None, 0)
    _check(lib().p3d_debug_accumulate_moving(int(device), C.byref(p), C.byref(fr), C.byref(hi) if hi else None, C.byref(mo), C.byref(o)),
           "p3d_debug_accumulate_moving")
    return out


_VARIANCE_PLANES = ("rgb32f", "length", "moments", "variance", "prev_xy")


def _accumulate_variance_request(rgb32f, depth, normal, cams, hit_id=None, history=None, motion=None, min_temporal=VARIANCE_MIN_TEMPORAL,
                                 radius=VARIANCE_RADIUS, sigma_depth=VARIANCE_SIGMA_DEPTH, normal_power_log2=VARIANCE_NORMAL_POWER_LOG2, **kw):
    """_accumulate_request or, with motion = dict(prim_type, prim_data), _accumulate_moving_request, and the moments -> (params,
    AccumulateVarianceParams, frames, history or None, the history's moments pointer or None, AccumulateMotion or None, the
    zeroed outputs, what must stay alive)."""
    if motion is not None:
        p, fr, hi, mo, out, keep = _accumulate_moving_request(rgb32f, depth, normal, cams, hit_id, motion["prim_type"], motion["prim_data"],
                                                              history, True, **kw)
    else:
        p, fr, hi, out, keep = _accumulate_request(rgb32f, depth, normal, cams, hit_id, history, **kw)
        mo = None
    hm = None
    if history is not None:
        hmom = np.ascontiguousarray(history["moments"], np.float32)
        if hmom.size != 2 * p.res_x * p.res_y:
            raise ValueError("the history's moments are one frame of 2 floats per pixel")
        hm = hmom.ctypes.data
        keep = keep + [hmom]
    out["moments"] = np.zeros(out["length"].shape + (2,), np.float32)
    out["variance"] = np.zeros(out["length"].shape, np.float32)
    vp = AccumulateVarianceParams(min_temporal, int(radius), sigma_depth, int(normal_power_log2))
    return p, vp, fr, hi, hm, mo, out, keep


def host_accumulate_variance(rgb32f, depth, normal, cams, hit_id=None, history=None, motion=None, **kw):
    """p3dh_accumulate_variance: the host layer's restatement of p3d_accumulate_variance, every bit of it, on host arrays (no
    GPU).  Arguments and result as DeviceScene.accumulate_variance."""
    p, vp, fr, hi, hm, mo, out, keep = _accumulate_variance_request(rgb32f, depth, normal, cams, hit_id, history, motion, **kw)
    lib().p3dh_accumulate_variance(C.byref(p), C.byref(vp), C.byref(fr), C.byref(hi) if hi else None, hm, C.byref(mo) if mo else None,
                                   *[out[k].ctypes.data if k in out else None for k in _VARIANCE_PLANES])
    return out


def debug_accumulate_variance(rgb32f, depth, normal, cams, hit_id=None, history=None, motion=None, device=0, **kw):
    """p3d_debug_accumulate_variance: the launches of p3d_accumulate_variance over host arrays, without a scene.  Arguments and
    result as DeviceScene.accumulate_variance."""
    p, vp, fr, hi, hm, mo, out, keep = _accumulate_variance_request(rgb32f, depth, normal, cams, hit_id, history, motion, **kw)
    o = AccumulateVarianceOutputs(*[out[k].ctypes.data if k in out else None for k in _VARIANCE_PLANES], 0)
    _check(lib().p3d_debug_accumulate_variance(int(device), C.byref(p), C.byref(vp), C.byref(fr), C.byref(hi) if hi else None, hm,
                                               C.byref(mo) if mo else None, C.byref(o)), "p3d_debug_accumulate_variance")
    return out


def host_ao_segments(cam, depth, normal, samples=AO_SAMPLES, radius=AO_RADIUS, bias=AO_BIAS, seed=0, frame=0):
    """p3dh_ao_segments: steps 1 to 6 of p3d_ambient_occlusion's definition on the host (no GPU), for ONE frame -- depth (H, W)
    and normal (H, W, 3) seen through cam, the frame-th of a batch.  Returns origin and dir (H, W, samples, 3), the segments
    p3d_occluded would be asked (zeros where the pixel has no query), and valid (H, W) uint8."""
    depth = np.ascontiguousarray(depth, np.float32)
    H, W = depth.shape
    normal = np.ascontiguousarray(normal, np.float32).reshape(H, W, 3)
    S = int(samples)
    origin = np.zeros((H, W, S, 3), np.float32)
    direction = np.zeros((H, W, S, 3), np.float32)
    valid = np.zeros((H, W), np.uint8)
    a = AoParams(S, radius, bias, int(seed) & 0xFFFFFFFF)
    lib().p3dh_ao_segments(C.byref(a), C.byref(cam), int(frame), W, H, depth.ctypes.data, normal.ctypes.data, origin.ctypes.data,
                           direction.ctypes.data, valid.ctypes.data)
    return origin, direction, valid


def host_ao_resolve(occluded, samples, rgb32f=None):
    """p3dh_ao_resolve: step 8 on the host -- occluded (...) int32 counts per pixel -> {"ao" (...), "rgb32f" (..., 3)}."""
    occluded = np.ascontiguousarray(occluded, np.int32)
    if rgb32f is not None:
        rgb32f = np.ascontiguousarray(rgb32f, np.float32).reshape(occluded.shape + (3,))
    out = {"ao": np.zeros(occluded.shape, np.float32), "rgb32f": np.zeros(occluded.shape + (3,), np.float32)}
    lib().p3dh_ao_resolve(int(samples), occluded.size, occluded.ctypes.data, rgb32f.ctypes.data if rgb32f is not None else None,
                          out["ao"].ctypes.data, out["rgb32f"].ctypes.data)
    return out


def host_indirect_resolve(radiance, valid, albedo=None, rgb32f=None):
    """p3dh_indirect_resolve: steps 8 and 9 of p3d_indirect_diffuse's definition on the host (no GPU) -- radiance
    (..., samples, 3), the colour of every sample's ray, and valid (...) uint8, 1 where the pixel has a query ->
    {"indirect" (..., 3), "rgb32f" (..., 3)}.  albedo and rgb32f (..., 3) are optional."""
    radiance = np.ascontiguousarray(radiance, np.float32)
    shape, S = radiance.shape[:-2], radiance.shape[-2]
    valid = np.ascontiguousarray(valid, np.uint8).reshape(shape)
    if albedo is not None:
        albedo = np.ascontiguousarray(albedo, np.float32).reshape(shape + (3,))
    if rgb32f is not None:
        rgb32f = np.ascontiguousarray(rgb32f, np.float32).reshape(shape + (3,))
    out = {"indirect": np.zeros(shape + (3,), np.float32), "rgb32f": np.zeros(shape + (3,), np.float32)}
    lib().p3dh_indirect_resolve(int(S), valid.size, radiance.ctypes.data, valid.ctypes.data, albedo.ctypes.data if albedo is not None else None,
                                rgb32f.ctypes.data if rgb32f is not None else None, out["indirect"].ctypes.data, out["rgb32f"].ctypes.data)
    return out


def host_path_next(b, bias, origin, direction, t, normal, hit_id, prim_material, materials12, pk0, sample, throughput=None):
    """p3dh_path_next: step 4 of p3d_indirect_paths' definition on the host (no GPU) for m paths that just traced ray b --
    origin, direction (m, 3), and t (m,), normal (m, 3), hit_id (m,) as p3d_trace_rays answered; prim_material and materials12
    of HostScene.arrays(); pk0 (m,) the pixels' keys, sample (m,) the paths' samples; throughput (m, 3) T_b (not read when
    b == 0).  Returns the next origin, direction (m, 3), T_(b+1) (m, 3) and alive (m,) uint8."""
    origin = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
    m = len(origin)
    direction = np.ascontiguousarray(direction, np.float32).reshape(m, 3)
    t = np.ascontiguousarray(t, np.float32).reshape(m)
    normal = np.ascontiguousarray(normal, np.float32).reshape(m, 3)
    hit_id = np.ascontiguousarray(hit_id, np.int32).reshape(m)
    prim_material = np.ascontiguousarray(prim_material, np.uint32)
    materials12 = np.ascontiguousarray(materials12, np.float32).reshape(-1, 12)
    pk0 = np.ascontiguousarray(pk0, np.uint32).reshape(m)
    sample = np.ascontiguousarray(sample, np.uint32).reshape(m)
    T = np.zeros((m, 3), np.float32) if throughput is None else np.array(throughput, np.float32).reshape(m, 3)
    o2, d2, alive = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.uint8)
    lib().p3dh_path_next(m, int(b), float(bias), origin.ctypes.data, direction.ctypes.data, t.ctypes.data, normal.ctypes.data, hit_id.ctypes.data,
                         prim_material.ctypes.data, materials12.ctypes.data, pk0.ctypes.data, sample.ctypes.data, T.ctypes.data,
                         o2.ctypes.data, d2.ctypes.data, alive.ctypes.data)
    return o2, d2, T, alive


def host_path_add(b, throughput, radiance, alive, total):
    """p3dh_path_add: step 3 on the host -- total (m, 3) with r_b (radiance (m, 3)) added under T_b (throughput (m, 3)) where
    alive (m,) is set: R = r_0 when b == 0, else R + T_b * r_b.  Returns the new sums; `total` is not modified."""
    radiance = np.ascontiguousarray(radiance, np.float32).reshape(-1, 3)
    m = len(radiance)
    throughput = np.ascontiguousarray(throughput, np.float32).reshape(m, 3)
    alive = np.ascontiguousarray(alive, np.uint8).reshape(m)
    out = np.array(total, np.float32).reshape(m, 3)
    lib().p3dh_path_add(m, int(b), throughput.ctypes.data, radiance.ctypes.data, alive.ctypes.data, out.ctypes.data)
    return out


def debug_pow(x, y, device=0):
    """The device's restatement of the host libm's pow(double, double) (csrc/p3d_pow.h) on n argument pairs."""
    x = np.ascontiguousarray(x, np.float64).ravel()
    y = np.ascontiguousarray(y, np.float64).ravel()
    assert x.shape == y.shape
    out = np.zeros_like(x)
    _check(lib().p3d_debug_pow(int(device), len(x), x.ctypes.data, y.ctypes.data, out.ctypes.data), "p3d_debug_pow")
    return out


def debug_schlick_kr(ior_1, new_ior, cos_theta_i, device=0):
    """The shading's SCHLICK_APPROX weight KR (RT/main.cpp:700-701) on the device for n (ior_1, newIor, cos_theta_i)."""
    a = np.ascontiguousarray(ior_1, np.float32).ravel()
    b = np.ascontiguousarray(new_ior, np.float32).ravel()
    c = np.ascontiguousarray(cos_theta_i, np.float32).ravel()
    assert a.shape == b.shape == c.shape
    out = np.zeros_like(c)
    _check(lib().p3d_debug_schlick_kr(int(device), len(c), a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data),
           "p3d_debug_schlick_kr")
    return out


def debug_check_rcp(first_bits=0, count=1 << 32, device=0):
    """(mismatches, first mismatching bit pattern) of the device's frcp() against 1.0f / x over `count` bit patterns."""
    n_bad, first_bad = C.c_uint64(0), C.c_uint32(0)
    _check(lib().p3d_debug_check_rcp(int(device), int(first_bits), int(count), C.byref(n_bad), C.byref(first_bad)), "p3d_debug_check_rcp")
    return int(n_bad.value), int(first_bad.value)


def debug_check_rcp_len(first_bits=0, count=1 << 31, device=0):
    """(mismatches, first mismatching bit pattern) of the device's rcp_len() against 1.0f / x over `count` bit patterns."""
    n_bad, first_bad = C.c_uint64(0), C.c_uint32(0)
    _check(lib().p3d_debug_check_rcp_len(int(device), int(first_bits), int(count), C.byref(n_bad), C.byref(first_bad)),
           "p3d_debug_check_rcp_len")
    return int(n_bad.value), int(first_bad.value)


def save_png(path, rgb8):
    """RT_Output.png writer of the host layer (csrc/host/p3d_scene.cpp): rgb8 is [H, W, 3] u8, bottom row first."""
    img = np.ascontiguousarray(rgb8, np.uint8)
    L = lib()
    L.p3dh_save_png.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]
    L.p3dh_save_png.restype = C.c_int
    if L.p3dh_save_png(os.fsencode(path), img.ctypes.data, img.shape[1], img.shape[0]) != 0:
        raise P3DError("cannot write %s" % path)


def host_bvh(desc, leaf_max=0):
    """Host-only BVH build (no GPU): dict(nodes [n,16] u32 view, refs, info)."""
    h = lib().p3dh_bvh_build(C.byref(desc), int(leaf_max))
    info = (C.c_uint32 * 5)()
    lib().p3dh_bvh_info(h, info)
    nodes = np.zeros((info[0], 16), np.uint32)
    refs = np.zeros(info[1], np.uint32)
    lib().p3dh_bvh_dump(h, nodes.ctypes.data, refs.ctypes.data)
    # the same nodes as scenes read from HBM get them: 32-byte pairs of 16-bit plane codes (8 dwords per node)
    qnodes = np.zeros((info[0], 8), np.uint32)
    qscale, qbase = np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib().p3dh_bvh_quantise(h, qnodes.ctypes.data, qscale.ctypes.data, qbase.ctypes.data)
    lib().p3dh_bvh_free(h)
    return {"nodes": nodes, "refs": refs, "n_leaves": int(info[2]), "max_depth": int(info[3]),
            "n_prims": int(info[4]), "qnodes": qnodes, "qscale": qscale, "qbase": qbase}


def host_build_prims(desc):
    """What either BVH builder is given for a scene (no GPU): (lo [n,3], hi [n,3], ref [n]) -- the padded bounds and leaf
    references of its bounded primitives, in scene order."""
    n = lib().p3dh_build_prims(C.byref(desc), None, None, None, 0)
    if n < 0:
        raise P3DError("p3dh_build_prims: the scene description is inconsistent")
    lo, hi, ref = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
    lib().p3dh_build_prims(C.byref(desc), lo.ctypes.data, hi.ctypes.data, ref.ctypes.data, n)
    return lo, hi, ref


def device_bvh(lo, hi, ref, device=0):
    """The device builder's tree (p3d_debug_lbvh_build) over n >= 4 build primitives: dict(nodes [L-1,16] u32 view, refs [n],
    n_nodes, n_leaves, n_leaf_refs, max_depth, sah_cost) with L = (n + 1) // 2, laid out like host_bvh()'s."""
    lo = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, np.uint32).ravel()
    n = len(ref)
    assert lo.shape == hi.shape == (n, 3)
    nodes = np.zeros((max((n + 1) // 2 - 1, 0), 16), np.uint32)
    refs = np.zeros(n, np.uint32)
    stats = np.zeros(4, np.uint32)
    sah = C.c_float(0.0)
    _check(lib().p3d_debug_lbvh_build(int(device), n, lo.ctypes.data, hi.ctypes.data, ref.ctypes.data, nodes.ctypes.data,
                                      refs.ctypes.data, stats.ctypes.data, C.addressof(sah)), "p3d_debug_lbvh_build")
    return {"nodes": nodes, "refs": refs, "n_nodes": int(stats[0]), "n_leaves": int(stats[1]), "n_leaf_refs": int(stats[2]),
            "max_depth": int(stats[3]), "sah_cost": float(np.float32(sah.value))}


def ploc_build(lo, hi, ref, device=0):
    """Builder 2's tree (p3d_debug_ploc_build) over n >= 4 build primitives: device_bvh()'s dict plus rounds and fell_back."""
    lo = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, np.uint32).ravel()
    n = len(ref)
    assert lo.shape == hi.shape == (n, 3)
    nodes = np.zeros((max((n + 1) // 2 - 1, 0), 16), np.uint32)
    refs = np.zeros(n, np.uint32)
    stats = np.zeros(4, np.uint32)
    sah = C.c_float(0.0)
    rounds, fell_back = C.c_int32(0), C.c_int32(0)
    _check(lib().p3d_debug_ploc_build(int(device), n, lo.ctypes.data, hi.ctypes.data, ref.ctypes.data, nodes.ctypes.data,
                                      refs.ctypes.data, stats.ctypes.data, C.addressof(sah), C.addressof(rounds),
                                      C.addressof(fell_back)), "p3d_debug_ploc_build")
    return {"nodes": nodes, "refs": refs, "n_nodes": int(stats[0]), "n_leaves": int(stats[1]), "n_leaf_refs": int(stats[2]),
            "max_depth": int(stats[3]), "sah_cost": float(np.float32(sah.value)), "rounds": rounds.value,
            "fell_back": fell_back.value}


def host_grid(desc):
    """Host-only build of the reference's uniform grid (no GPU): (dims[3], per-cell populations)."""
    L = lib()
    L.p3dh_grid_build.restype = C.c_int64
    L.p3dh_grid_build.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int32), C.c_void_p, C.c_uint64]
    dims = (C.c_int32 * 3)()
    n = L.p3dh_grid_build(C.byref(desc), dims, None, 0)
    counts = np.zeros(n, np.uint32)
    L.p3dh_grid_build(C.byref(desc), dims, counts.ctypes.data, n)
    return np.array(list(dims), np.int32), counts


def _grid_boxes(lo, hi, ref):
    lo = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, np.uint32).ravel()
    assert lo.shape == hi.shape == (len(ref), 3)
    return lo, hi, ref


def _grid_dict(dims, mn, mx, cell_start, items):
    return {"dims": dims, "mn": mn, "mx": mx, "cell_start": cell_start, "items": items}


def host_grid_arrays(desc=None, lo=None, hi=None, ref=None):
    """The whole of the host grid build (p3dh_grid_dump, no GPU), over a scene description or over boxes lo / hi [n, 3] listed
    under ref [n]: dict(dims [3] int32, mn / mx [3] float32, cell_start [cells + 1] uint32, items uint32)."""
    if desc is None:
        lo, hi, ref = _grid_boxes(lo, hi, ref)
    dims, mn, mx, n_items = np.zeros(3, np.int32), np.zeros(3, np.float32), np.zeros(3, np.float32), C.c_uint64(0)
    head = (C.byref(desc) if desc is not None else None, 0 if desc is not None else len(ref),
            None if desc is not None else lo.ctypes.data, None if desc is not None else hi.ctypes.data,
            None if desc is not None else ref.ctypes.data, dims.ctypes.data, mn.ctypes.data, mx.ctypes.data, C.addressof(n_items))
    cells = lib().p3dh_grid_dump(*head, None, 0, None, 0)
    if cells < 0:
        raise P3DError("p3dh_grid_dump: the reference's grid formula asks for more than 2^31 cells")
    cell_start, items = np.zeros(cells + 1, np.uint32), np.zeros(n_items.value, np.uint32)
    lib().p3dh_grid_dump(*head, cell_start.ctypes.data, len(cell_start), items.ctypes.data, len(items))
    return _grid_dict(dims, mn, mx, cell_start, items)


def debug_grid_build(lo, hi, ref, device=0):
    """The device grid build (p3d_debug_grid_build) over boxes lo / hi [n, 3] listed under ref [n]: the dict of
    host_grid_arrays, made by the function p3d_scene_build_grid runs."""
    lo, hi, ref = _grid_boxes(lo, hi, ref)
    n = len(ref)
    dims, mn, mx = np.zeros(3, np.int32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    n_cells, n_items = C.c_uint64(0), C.c_uint64(0)
    head = (int(device), n, lo.ctypes.data if n else None, hi.ctypes.data if n else None, ref.ctypes.data if n else None,
            dims.ctypes.data, mn.ctypes.data, mx.ctypes.data, C.addressof(n_cells), C.addressof(n_items))
    _check(lib().p3d_debug_grid_build(*head, None, 0, None, 0), "p3d_debug_grid_build")
    cell_start, items = np.zeros(n_cells.value + 1, np.uint32), np.zeros(max(n_items.value, 1), np.uint32)
    _check(lib().p3d_debug_grid_build(*head, cell_start.ctypes.data, len(cell_start), items.ctypes.data, n_items.value),
           "p3d_debug_grid_build")
    return _grid_dict(dims, mn, mx, cell_start, items[:n_items.value])


class PathTracer:
    """The reference's Shadertoy path tracer on one GPU (include/p3d_pathtracer.h)."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(lib().p3d_pt_create(int(device), C.byref(self.h)), "p3d_pt_create")

    def close(self):
        if self.h:
            lib().p3d_pt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, ptr):
        _check(lib().p3d_pt_set_stream(self.h, C.c_void_p(ptr)), "p3d_pt_set_stream")

    def sync(self):
        _check(lib().p3d_pt_sync(self.h), "p3d_pt_sync")

    def timer_begin(self):
        _check(lib().p3d_pt_timer_begin(self.h), "p3d_pt_timer_begin")

    def timer_end(self):
        ms = C.c_float(0)
        _check(lib().p3d_pt_timer_end(self.h, C.byref(ms)), "p3d_pt_timer_end")
        return ms.value

    @staticmethod
    def _params(res_x, res_y, n_frames, first_frame, frame_stride, time0, dt, mouse):
        return PtParams(int(res_x), int(res_y), int(n_frames), int(first_frame), int(frame_stride), float(time0),
                        float(dt), float(mouse[0]), float(mouse[1]))

    def render(self, res_x, res_y, n_frames, first_frame=0, frame_stride=1, time0=0.0, dt=1.0 / 60.0, mouse=(0.0, 0.0),
               want_rgba=True):
        """Host arrays: rgba [H,W,4] (gamma-encoded running mean + frame count), linear [H,W,3] (sum).
        want_rgba=False passes rgba = NULL (the linear-only form, whose frames may be cut into runs) and returns None for it."""
        rgba = np.zeros((res_y, res_x, 4), np.float32) if want_rgba else None
        lin = np.zeros((res_y, res_x, 3), np.float32)
        p = self._params(res_x, res_y, n_frames, first_frame, frame_stride, time0, dt, mouse)
        o = PtOutputs(rgba.ctypes.data if want_rgba else None, lin.ctypes.data, 0)
        _check(lib().p3d_pt_render(self.h, C.byref(p), C.byref(o)), "p3d_pt_render")
        return rgba, lin

    def render_device(self, rgba_ptr, linear_ptr, res_x, res_y, n_frames, first_frame=0, frame_stride=1, time0=0.0,
                      dt=1.0 / 60.0, mouse=(0.0, 0.0)):
        p = self._params(res_x, res_y, n_frames, first_frame, frame_stride, time0, dt, mouse)
        o = PtOutputs(rgba_ptr or None, linear_ptr or None, 1)
        _check(lib().p3d_pt_render(self.h, C.byref(p), C.byref(o)), "p3d_pt_render")


def pt_debug_hash(a, b, device=0):
    a = np.ascontiguousarray(a, np.uint32)
    b = np.ascontiguousarray(b, np.uint32)
    out = np.zeros(len(a), np.uint32)
    _check(lib().p3d_pt_debug_hash(int(device), len(a), a.ctypes.data, b.ctypes.data, out.ctypes.data), "p3d_pt_debug_hash")
    return out


def _f32(a, shape):
    a = np.ascontiguousarray(a, np.float32)
    assert a.shape == shape, (a.shape, shape)
    return a


def _rec_arrays(rec, n):
    return (_f32(rec["pos"], (n, 3)), _f32(rec["normal"], (n, 3)), _f32(rec["t"], (n,)),
            np.ascontiguousarray(rec["mat_type"], np.int32), _f32(rec["mat"], (n, 11)))


def pt_debug_hit_world(origin, direction, time, tmin, tmax, seed, active=None, fill=None, device=0):
    """The frame kernel's hit_world() on caller-supplied rays (p3d_pt_debug_hit_world).  Case i is lane i % 64 of
    workgroup i / 64.  `fill` (a dict like the result) presets the outputs: cases with active == 0 keep them."""
    n = len(seed)
    o, d = _f32(origin, (n, 3)), _f32(direction, (n, 3))
    tm, t0, t1, sd = (_f32(x, (n,)) for x in (time, tmin, tmax, seed))
    act = np.ones(n, np.int32) if active is None else np.ascontiguousarray(active, np.int32)
    shapes = {"hit": ((n,), np.int32), "t": ((n,), np.float32), "pos": ((n, 3), np.float32), "normal": ((n, 3), np.float32),
              "mat_type": ((n,), np.int32), "mat": ((n, 11), np.float32), "seed_out": ((n,), np.float32)}
    out = {k: (np.zeros(sh, dt) if fill is None else np.ascontiguousarray(fill[k], dt).reshape(sh).copy()) for k, (sh, dt) in shapes.items()}
    _check(lib().p3d_pt_debug_hit_world(int(device), n, o.ctypes.data, d.ctypes.data, tm.ctypes.data, t0.ctypes.data, t1.ctypes.data,
                                        sd.ctypes.data, act.ctypes.data, out["hit"].ctypes.data, out["t"].ctypes.data,
                                        out["pos"].ctypes.data, out["normal"].ctypes.data, out["mat_type"].ctypes.data,
                                        out["mat"].ctypes.data, out["seed_out"].ctypes.data), "p3d_pt_debug_hit_world")
    return out


def pt_debug_scatter(ray, rec, seed, device=0):
    """The frame kernel's scatter() (p3d_pt_debug_scatter).  ray = {o, d, t}; rec = {pos, normal, t, mat_type, mat}."""
    n = len(seed)
    o, d, t = _f32(ray["o"], (n, 3)), _f32(ray["d"], (n, 3)), _f32(ray["t"], (n,))
    pos, nrm, rt, mt, mat = _rec_arrays(rec, n)
    sd = _f32(seed, (n,))
    out = {"atten": np.zeros((n, 3), np.float32), "o": np.zeros((n, 3), np.float32), "d": np.zeros((n, 3), np.float32),
           "t": np.zeros(n, np.float32), "seed_out": np.zeros(n, np.float32)}
    _check(lib().p3d_pt_debug_scatter(int(device), n, o.ctypes.data, d.ctypes.data, t.ctypes.data, pos.ctypes.data, nrm.ctypes.data,
                                      rt.ctypes.data, mt.ctypes.data, mat.ctypes.data, sd.ctypes.data, out["atten"].ctypes.data,
                                      out["o"].ctypes.data, out["d"].ctypes.data, out["t"].ctypes.data, out["seed_out"].ctypes.data),
           "p3d_pt_debug_scatter")
    return out


def pt_debug_direct_lighting(light_pos, ray, rec, seed, device=0):
    """The frame kernel's direct_lighting() (p3d_pt_debug_direct_lighting): {rgb, seed_out}."""
    n = len(seed)
    lp = _f32(light_pos, (n, 3))
    o, d, t = _f32(ray["o"], (n, 3)), _f32(ray["d"], (n, 3)), _f32(ray["t"], (n,))
    pos, nrm, rt, mt, mat = _rec_arrays(rec, n)
    sd = _f32(seed, (n,))
    out = {"rgb": np.zeros((n, 3), np.float32), "seed_out": np.zeros(n, np.float32)}
    _check(lib().p3d_pt_debug_direct_lighting(int(device), n, lp.ctypes.data, o.ctypes.data, d.ctypes.data, t.ctypes.data,
                                              pos.ctypes.data, nrm.ctypes.data, rt.ctypes.data, mt.ctypes.data, mat.ctypes.data,
                                              sd.ctypes.data, out["rgb"].ctypes.data, out["seed_out"].ctypes.data),
           "p3d_pt_debug_direct_lighting")
    return out
