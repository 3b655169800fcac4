"""ctypes binding of libmi3pt.so (include/mi3pt.h).

Thin by design: one Python method per C entry point, numpy arrays in and out, status
codes turned into `Mi3ptError` (the way the N-API shim turns them into thrown Errors).
No compute happens here and there is no fallback: if the library or a HIP device is
missing the calls raise.
"""
import ctypes
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# (MI3PT_LIBRARY: another build of the library -- the sweeps under profiles/ point it at the experiment build,
# libmi3pt_exp.so, which reads its options from the environment; read here, by the Python host, not by the library)
LIB_PATH = os.environ.get("MI3PT_LIBRARY") or os.path.join(PKG_ROOT, "libmi3pt.so")

PASS_RAYTRACE, PASS_ACCUMULATE, PASS_FULLSCREEN = 0, 1, 2
PASS_AOV = 3          # mi3pt_pass_time_us only: the first-hit feature images have no uniform block
PASS_GUIDED = 4       # mi3pt_pass_time_us only: the feature-guided de-noise (denoise_guided)
PASS_CONVERGENCE = 5  # mi3pt_pass_time_us only: the per-tile error estimate (estimate_convergence)
PASS_REPROJECT = 6    # mi3pt_pass_time_us only: the gather kernel of reproject (its feature render is PASS_AOV's)
PASS_HISTORY = 7      # mi3pt_pass_time_us only: the kernel of merge_history
GUIDED_PRESENT = 1    # mi3pt_guided_params.flags: draw the canvas from the filtered image
GUIDED_VARIANCE = 2   # ... the colour weight steered by the per-pixel variance of the mean (needs set_moments(True))
GUIDED_YOUNG = 4      # ... with GUIDED_VARIANCE: a texel with fewer than GUIDED_YOUNG_COUNT samples takes the pooled variance of its 7 x 7 neighbours
GUIDED_YOUNG_COUNT = 4.0
# mi3pt_aov: the first-hit feature images (render_aovs takes an OR of 1 << AOV_*)
AOV_ALBEDO, AOV_NORMAL, AOV_POSITION, AOV_IDS, AOV_COUNT = 0, 1, 2, 3, 4
AOV_ALL = (1 << AOV_COUNT) - 1
AOV_NAMES = ("albedo", "normal", "position", "ids")
SUBMIT_RAYTRACE, SUBMIT_ACCUMULATE, SUBMIT_FULLSCREEN = 1, 2, 4
TEX_OUTPUT, TEX_ACCUMULATION, TEX_CANVAS = 0, 1, 2
STORAGE_F32, STORAGE_F16 = 0, 1
PRESENT_EXACT, PRESENT_LATEST = 0, 1
# mi3pt_option (include/mi3pt.h): scheduling options; none changes a bit of any image
(OPT_WALK_MIN, OPT_LEAF_MIN, OPT_SHADE_SPLIT, OPT_TAIL_POLICY, OPT_TOP_PACKETS, OPT_TRI_PAIR, OPT_JOB_REVERSE, OPT_JOB_GROUP,
 OPT_JOB_CHUNK, OPT_BATCH_LIMIT, OPT_BATCH, OPT_WAVES_PER_CU, OPT_CULL, OPT_WIDE, OPT_GATE, OPT_SLOT_SETS, OPT_PIPELINE,
 OPT_COST_ORDER, OPT_PRESENT_DEPTH, OPT_HOST_ANALYSES, OPT_GATHER_STAGED, OPT_DIAG_LITE,
 OPT_GATE_TIMEOUT_MS, OPT_GATE_RELEASES, OPT_DEBUG_SUPPRESS_DRAIN, OPT_CAMERA_BASE, OPT_PACKET_ORDER, OPT_SIX_WAVES, OPT_COLLAPSE, OPT_LAST_BUILD, OPT_WALK_ADAPT, OPT_SKY_TILES) = range(32)
COUNTER_NAMES = ("rays", "box_tests", "tri_tests", "hits", "misses", "stack_overflows", "pixels", "reserved")

# every symbol include/mi3pt.h declares; tests/test_capi_symbols.py checks the header
# against this list and against the built library.
SYMBOLS = (
    "mi3pt_abi_version", "mi3pt_last_error", "mi3pt_device_count", "mi3pt_device_name",
    "mi3pt_create", "mi3pt_destroy", "mi3pt_set_stream", "mi3pt_set_storage", "mi3pt_set_tile",
    "mi3pt_tile_local_rows", "mi3pt_upload_triangles", "mi3pt_upload_materials", "mi3pt_upload_bvh",
    "mi3pt_upload_environment", "mi3pt_upload_environment_cdf", "mi3pt_resize", "mi3pt_reset",
    "mi3pt_set_uniforms", "mi3pt_submit", "mi3pt_sync", "mi3pt_read_texture", "mi3pt_read_canvas_rgba8",
    "mi3pt_write_texture",
    "mi3pt_accumulation_device_ptr", "mi3pt_bind_accumulation", "mi3pt_enable_timing",
    "mi3pt_pass_time_us", "mi3pt_raytrace_launch_stats", "mi3pt_get_counters", "mi3pt_reset_counters", "mi3pt_set_kernel_variant",
    "mi3pt_set_env_sampling", "mi3pt_device_build_bvh",
    "mi3pt_set_pipelining", "mi3pt_flush", "mi3pt_set_present_mode", "mi3pt_raytrace_launch_span", "mi3pt_batch_capacity", "mi3pt_debug_active_variant", "mi3pt_debug_last_launch", "mi3pt_submit_frames", "mi3pt_debug_set_packet_layout",
    "mi3pt_debug_intersect", "mi3pt_debug_intersect_shipped", "mi3pt_debug_pairs", "mi3pt_debug_math", "mi3pt_debug_wave_times", "mi3pt_host_build_bvh", "mi3pt_host_build_bvh_f64",
    "mi3pt_host_env_cdf", "mi3pt_host_eight_wide_check", "mi3pt_host_sky_tiles", "mi3pt_host_scene_compile", "mi3pt_host_walk_buffer", "mi3pt_host_route", "mi3pt_debug_set_option", "mi3pt_debug_get_option",
    "mi3pt_create_group", "mi3pt_group_size", "mi3pt_group_member",
    "mi3pt_tile_global_row", "mi3pt_tile_owner",
    "mi3pt_render_aovs", "mi3pt_read_aov", "mi3pt_aov_device_ptr",
    "mi3pt_denoise_guided", "mi3pt_read_guided", "mi3pt_guided_device_ptr",
    "mi3pt_set_moments", "mi3pt_read_moments", "mi3pt_write_moments", "mi3pt_moments_device_ptr", "mi3pt_read_guided_variance",
    "mi3pt_estimate_convergence", "mi3pt_read_convergence", "mi3pt_read_convergence_tiles",
    "mi3pt_set_sample_mask", "mi3pt_read_sample_mask", "mi3pt_freeze_converged", "mi3pt_host_freeze_tiles",
    "mi3pt_set_mean_by_count", "mi3pt_host_view_frame", "mi3pt_reproject",
    "mi3pt_keep_geometry", "mi3pt_reproject_scene",
    "mi3pt_hold_history", "mi3pt_merge_history",
    "mi3pt_set_guided_despike", "mi3pt_read_guided_despiked",
    "mi3pt_device_refit_bvh", "mi3pt_host_bvh_cost",
    "mi3pt_device_build_bvh_ex",
)
BVH_METHODS = {"lbvh": 0, "ploc": 1}        # MI3PT_BVH_METHOD_*
PLOC_SEARCH_BLOCK = 256                     # MI3PT_PLOC_SEARCH_BLOCK: positions per workgroup of the clustering's neighbour search


class BvhBuildParams(ctypes.Structure):
    """mi3pt_bvh_build_params"""
    _fields_ = [("method", ctypes.c_int), ("radius", ctypes.c_int), ("max_search_iterations", ctypes.c_int), ("flags", ctypes.c_uint)]


class BvhBuildInfoStruct(ctypes.Structure):
    """mi3pt_bvh_build_info"""
    _fields_ = [("build_ms", ctypes.c_float), ("search_iterations", ctypes.c_uint32), ("forced_iterations", ctypes.c_uint32)]


class BvhBuildInfo(float):
    """What Context.device_build_bvh returns beside the records: the device time in milliseconds -- a float, as that call has always
    returned -- with mi3pt_bvh_build_info's fields as attributes: build_ms, search_iterations, forced_iterations."""

    def __new__(cls, build_ms, search_iterations=0, forced_iterations=0):
        self = super().__new__(cls, build_ms)
        self.build_ms, self.search_iterations, self.forced_iterations = float(build_ms), int(search_iterations), int(forced_iterations)
        return self


class GuidedParams(ctypes.Structure):
    """mi3pt_guided_params"""
    _fields_ = [("levels", ctypes.c_int), ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_albedo", ctypes.c_float), ("sigma_plane", ctypes.c_float), ("flags", ctypes.c_uint)]


class ReprojectParams(ctypes.Structure):
    """mi3pt_reproject_params"""
    _fields_ = [("plane_tolerance", ctypes.c_float), ("normal_cos_min", ctypes.c_float), ("max_history", ctypes.c_int),
                ("flags", ctypes.c_uint)]


class ReprojectSceneParams(ctypes.Structure):
    """mi3pt_reproject_scene_params"""
    _fields_ = [("plane_tolerance", ctypes.c_float), ("normal_cos_min", ctypes.c_float), ("max_history", ctypes.c_int),
                ("max_history_moved", ctypes.c_int), ("flags", ctypes.c_uint)]


class HistoryParams(ctypes.Structure):
    """mi3pt_history_params"""
    _fields_ = [("radius", ctypes.c_int), ("z_keep", ctypes.c_float), ("z_drop", ctypes.c_float), ("flags", ctypes.c_uint)]


class Convergence(ctypes.Structure):
    """mi3pt_convergence"""
    _fields_ = [("tiles", ctypes.c_uint32), ("tiles_above", ctypes.c_uint32), ("tiles_young", ctypes.c_uint32),
                ("tiles_nonfinite", ctypes.c_uint32), ("texels", ctypes.c_uint64), ("worst_tile", ctypes.c_float),
                ("worst_texel", ctypes.c_float), ("n_min", ctypes.c_float), ("threshold", ctypes.c_float)]


class Mi3ptError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"mi3pt error {code}: {message}")
        self.code = code
        self.message = message


_lib = None


def load_library(path=None):
    """Load libmi3pt.so (built by webgpu-pathtracer_amd/csrc/Makefile)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise Mi3ptError(-1, f"{path} not found: build it with `make -C webgpu-pathtracer_amd/csrc` "
                             "(or __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    c_void_p, c_size_t, c_int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.mi3pt_last_error.restype = ctypes.c_char_p
    lib.mi3pt_create.argtypes = [c_int, ctypes.POINTER(c_void_p)]
    lib.mi3pt_destroy.argtypes = [c_void_p]
    lib.mi3pt_set_stream.argtypes = [c_void_p, c_void_p]
    lib.mi3pt_set_storage.argtypes = [c_void_p, c_int]
    lib.mi3pt_set_tile.argtypes = [c_void_p, c_int, c_int, c_int]
    lib.mi3pt_set_kernel_variant.argtypes = [c_void_p, c_int]
    lib.mi3pt_set_env_sampling.argtypes = [c_void_p, c_int]
    lib.mi3pt_set_pipelining.argtypes = [c_void_p, c_int]
    lib.mi3pt_set_present_mode.argtypes = [c_void_p, c_int]
    for name in ("mi3pt_upload_triangles", "mi3pt_upload_materials", "mi3pt_upload_bvh"):
        getattr(lib, name).argtypes = [c_void_p, c_void_p, c_size_t]
    for name in ("mi3pt_upload_environment", "mi3pt_upload_environment_cdf"):
        getattr(lib, name).argtypes = [c_void_p, c_void_p, c_int, c_int]
    lib.mi3pt_resize.argtypes = [c_void_p, c_int, c_int]
    lib.mi3pt_reset.argtypes = [c_void_p]
    lib.mi3pt_set_uniforms.argtypes = [c_void_p, c_int, c_void_p, c_size_t]
    lib.mi3pt_submit.argtypes = [c_void_p, ctypes.c_uint]
    lib.mi3pt_submit_frames.argtypes = [c_void_p, ctypes.c_uint, ctypes.c_uint32]
    lib.mi3pt_sync.argtypes = [c_void_p]
    lib.mi3pt_flush.argtypes = [c_void_p]
    lib.mi3pt_read_texture.argtypes = [c_void_p, c_int, c_void_p, c_size_t]
    lib.mi3pt_read_canvas_rgba8.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_write_texture.argtypes = [c_void_p, c_int, c_void_p, c_size_t]
    lib.mi3pt_accumulation_device_ptr.argtypes = [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t)]
    lib.mi3pt_bind_accumulation.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_render_aovs.argtypes = [c_void_p, ctypes.c_uint]
    lib.mi3pt_read_aov.argtypes = [c_void_p, c_int, c_void_p, c_size_t]
    lib.mi3pt_aov_device_ptr.argtypes = [c_void_p, c_int, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t)]
    lib.mi3pt_denoise_guided.argtypes = [c_void_p, ctypes.POINTER(GuidedParams)]
    lib.mi3pt_read_guided.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_guided_device_ptr.argtypes = [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t)]
    lib.mi3pt_set_moments.argtypes = [c_void_p, c_int]
    lib.mi3pt_read_moments.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_write_moments.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_moments_device_ptr.argtypes = [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_size_t)]
    lib.mi3pt_read_guided_variance.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_set_guided_despike.argtypes = [c_void_p, c_int]
    lib.mi3pt_read_guided_despiked.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.mi3pt_estimate_convergence.argtypes = [c_void_p, ctypes.c_float, c_int]
    lib.mi3pt_read_convergence.argtypes = [c_void_p, ctypes.POINTER(Convergence)]
    lib.mi3pt_read_convergence_tiles.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_set_sample_mask.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.mi3pt_read_sample_mask.argtypes = [c_void_p, c_void_p, c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    lib.mi3pt_freeze_converged.argtypes = [c_void_p, c_int, ctypes.POINTER(ctypes.c_uint32)]
    lib.mi3pt_host_freeze_tiles.argtypes = [c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    lib.mi3pt_set_mean_by_count.argtypes = [c_void_p, c_int]
    lib.mi3pt_host_view_frame.argtypes = [c_void_p, c_size_t, c_void_p]
    lib.mi3pt_reproject.argtypes = [c_void_p, ctypes.POINTER(ReprojectParams)]
    lib.mi3pt_keep_geometry.argtypes = [c_void_p, c_int]
    lib.mi3pt_reproject_scene.argtypes = [c_void_p, ctypes.POINTER(ReprojectSceneParams)]
    lib.mi3pt_hold_history.argtypes = [c_void_p]
    lib.mi3pt_merge_history.argtypes = [c_void_p, ctypes.POINTER(HistoryParams)]
    lib.mi3pt_enable_timing.argtypes = [c_void_p, c_int]
    lib.mi3pt_pass_time_us.argtypes = [c_void_p, c_int, ctypes.POINTER(ctypes.c_float)]
    lib.mi3pt_raytrace_launch_stats.argtypes = [c_void_p, c_int, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.mi3pt_raytrace_launch_span.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_double)]
    lib.mi3pt_batch_capacity.argtypes = [c_void_p, ctypes.POINTER(c_int)]
    lib.mi3pt_debug_active_variant.argtypes = [c_void_p, ctypes.POINTER(c_int)]
    lib.mi3pt_debug_last_launch.argtypes = [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    lib.mi3pt_create_group.argtypes = [ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(c_void_p)]
    lib.mi3pt_group_size.argtypes = [c_void_p, ctypes.POINTER(c_int)]
    lib.mi3pt_group_member.argtypes = [c_void_p, c_int, ctypes.POINTER(c_void_p)]
    lib.mi3pt_debug_set_option.argtypes = [c_void_p, c_int, c_int]
    lib.mi3pt_debug_get_option.argtypes = [c_void_p, c_int, ctypes.POINTER(c_int)]
    lib.mi3pt_debug_set_packet_layout.argtypes = [c_void_p, c_int]
    lib.mi3pt_get_counters.argtypes = [c_void_p, c_void_p]
    lib.mi3pt_reset_counters.argtypes = [c_void_p]
    lib.mi3pt_debug_intersect.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mi3pt_debug_math.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
    lib.mi3pt_debug_intersect_shipped.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.mi3pt_debug_pairs.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t]
    lib.mi3pt_device_build_bvh.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.mi3pt_device_refit_bvh.argtypes = [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_size_t), ctypes.POINTER(ctypes.c_float)]
    lib.mi3pt_device_build_bvh_ex.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.mi3pt_host_bvh_cost.argtypes = [c_void_p, c_size_t, ctypes.POINTER(ctypes.c_double)]
    lib.mi3pt_debug_wave_times.argtypes = [c_void_p, c_int, c_void_p, c_size_t, ctypes.POINTER(c_size_t)]
    lib.mi3pt_host_build_bvh.argtypes = [c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(c_size_t), c_int]
    lib.mi3pt_host_build_bvh_f64.argtypes = [c_void_p, c_size_t, c_void_p, c_size_t, ctypes.POINTER(c_size_t), c_int]
    lib.mi3pt_host_env_cdf.argtypes = [c_void_p, c_int, c_int, c_void_p]
    lib.mi3pt_host_eight_wide_check.argtypes = [c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_void_p]
    lib.mi3pt_host_scene_compile.argtypes = [c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_size_t]
    lib.mi3pt_host_walk_buffer.argtypes = [c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(c_size_t)]
    lib.mi3pt_host_sky_tiles.argtypes = [c_void_p, c_size_t, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, ctypes.POINTER(c_size_t)]
    lib.mi3pt_host_route.argtypes = [c_void_p, c_size_t, c_void_p]
    lib.mi3pt_device_count.argtypes = [ctypes.POINTER(c_int)]
    lib.mi3pt_device_name.argtypes = [c_int, ctypes.c_char_p, c_size_t]
    lib.mi3pt_tile_local_rows.argtypes = [c_int, c_int, c_int, c_int]
    lib.mi3pt_tile_global_row.argtypes = [c_int, c_int, c_int, c_int]
    lib.mi3pt_tile_owner.argtypes = [c_int, c_int, c_int]
    if path == LIB_PATH:
        _lib = lib
    return lib


def _check(lib, rc):
    if rc != 0:
        raise Mi3ptError(rc, lib.mi3pt_last_error().decode("utf-8", "replace"))


def _ptr(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def device_count():
    lib = load_library()
    n = ctypes.c_int(0)
    _check(lib, lib.mi3pt_device_count(ctypes.byref(n)))
    return n.value


def device_name(device=0):
    lib = load_library()
    buf = ctypes.create_string_buffer(256)
    _check(lib, lib.mi3pt_device_name(device, buf, 256))
    return buf.value.decode()


def last_error():
    """Text of this thread's most recent error -- or warning (the launch gate's host-side release returns MI3PT_OK and leaves one)."""
    return load_library().mi3pt_last_error().decode(errors="replace")


def tile_local_rows(height, rank, nranks, block_rows):
    return load_library().mi3pt_tile_local_rows(height, rank, nranks, block_rows)


def tile_global_row(local_row, rank, nranks, block_rows):
    """The image row that local row `local_row` of `rank`'s compact texture holds (mi3pt_set_tile's deal)."""
    return load_library().mi3pt_tile_global_row(local_row, rank, nranks, block_rows)


def tile_owner(y, nranks, block_rows):
    return load_library().mi3pt_tile_owner(y, nranks, block_rows)


# ---- host-side scene compile (no device) ----

def host_build_bvh(triangles, nthreads=0):
    """triangles: structured array (layout.TRIANGLE) or raw bytes -> BVH_NODE array."""
    from . import layout
    lib = load_library()
    tri = np.ascontiguousarray(triangles)
    n = tri.nbytes // 112
    nodes = np.zeros(max(2 * n - 1, 1), layout.BVH_NODE)
    count = ctypes.c_size_t(0)
    _check(lib, lib.mi3pt_host_build_bvh(_ptr(tri), n, _ptr(nodes), nodes.nbytes, ctypes.byref(count), nthreads))
    return nodes[:count.value]


def host_build_bvh_f64(positions, nthreads=0):
    """positions: (n, 3, 3) float64 world-space triangle vertices."""
    from . import layout
    lib = load_library()
    pos = np.ascontiguousarray(positions, np.float64)
    n = pos.size // 9
    nodes = np.zeros(max(2 * n - 1, 1), layout.BVH_NODE)
    count = ctypes.c_size_t(0)
    _check(lib, lib.mi3pt_host_build_bvh_f64(_ptr(pos), n, _ptr(nodes), nodes.nbytes, ctypes.byref(count), nthreads))
    return nodes[:count.value]


def host_bvh_cost(nodes):
    """mi3pt_host_bvh_cost: the summed box areas of every 48-byte record over the root's -- the SAH figure a host compares before and
    after Context.device_refit_bvh."""
    lib = load_library()
    nd = np.ascontiguousarray(nodes)
    cost = ctypes.c_double(0.0)
    _check(lib, lib.mi3pt_host_bvh_cost(_ptr(nd), nd.nbytes // 48, ctypes.byref(cost)))
    return cost.value


def host_sky_tiles(nodes, raytrace_uniforms, width, height, rank=0, nranks=1, block_rows=8):
    """mi3pt_host_sky_tiles: the 8x8 tiles of a rank's image whose camera rays can reach no geometry, as a (tile rows, tile
    columns) array of 0 / 1 over the rank's local rows."""
    lib = load_library()
    nd = np.ascontiguousarray(nodes)
    un = np.frombuffer(bytes(raytrace_uniforms), np.uint8).copy()
    n = ctypes.c_size_t(0)
    _check(lib, lib.mi3pt_host_sky_tiles(_ptr(nd), nd.nbytes, _ptr(un), width, height, rank, nranks, block_rows, None, 0, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), np.uint8)
    _check(lib, lib.mi3pt_host_sky_tiles(_ptr(nd), nd.nbytes, _ptr(un), width, height, rank, nranks, block_rows, _ptr(out), out.nbytes, ctypes.byref(n)))
    tiles_x = (width + 7) // 8
    return out[:n.value].reshape(-1, tiles_x)


def host_eight_wide_check(nodes, triangles, greedy=False):
    """mi3pt_host_eight_wide_check: builds kernel variant 14's packets on the host and checks them independently of the builder;
    dict(packets, records, levels, children_per_packet, leaves, offered)."""
    lib = load_library()
    nd, tr = np.ascontiguousarray(nodes), np.ascontiguousarray(triangles)
    out = np.zeros(6, np.uint64)
    _check(lib, lib.mi3pt_host_eight_wide_check(_ptr(nd), nd.nbytes, _ptr(tr), tr.nbytes, 1 if greedy else 0, _ptr(out)))
    return {"packets": int(out[0]), "records": int(out[1]), "levels": int(out[2]), "children_per_packet": out[3] / 1000.0,
            "leaves": int(out[4]), "offered": bool(out[5])}


# what mi3pt_host_scene_compile fills in, in order (include/mi3pt.h): scalars, then one FNV-1a digest per device buffer (0: not built)
SCENE_COMPILE_FIELDS = (
    "nodes", "triangles", "packets", "leaf_cap", "tree_proper", "walk_stack_worst", "cull_stack_ok", "root_ref", "scene_flags",
    "max_tri_ref", "max_mat_ref", "analysed", "cull_ka", "cull_kb", "wide_ok", "cwide_ok", "cw8_ok", "wide_root_nested",
    "wide_stack_worst", "auto_wide_variant", "wide_packets", "cw8_packets", "cw8_records", "cw8_levels",
    "digest_node_packets", "digest_leaf_rank", "digest_tri_packets", "digest_wide_packets", "digest_cwide_packets",
    "digest_tri_records", "digest_cw8_packets", "digest_cw8_records")


def host_scene_compile(nodes, triangles, collapse=-1, packet_order=0, want_eight_wide=False):
    """mi3pt_host_scene_compile: what the uploads and a context's scene analysis compute for this tree + triangles, on the host;
    dict of SCENE_COMPILE_FIELDS (ints; cull_ka / cull_kb as the bits of the float)."""
    lib = load_library()
    nd, tr = np.ascontiguousarray(nodes), np.ascontiguousarray(triangles)
    out = np.zeros(len(SCENE_COMPILE_FIELDS), np.uint64)
    _check(lib, lib.mi3pt_host_scene_compile(_ptr(nd), nd.nbytes, _ptr(tr), tr.nbytes, int(collapse), int(packet_order),
                                             1 if want_eight_wide else 0, _ptr(out), len(out)))
    return dict(zip(SCENE_COMPILE_FIELDS, (int(x) for x in out)))


# mi3pt_host_walk_buffer's kinds, and the record size of each (csrc/pt_kernels.h: uint32, WidePacket, CWidePacket, TriPacket64, CW8Packet, TriPacket64)
WALK_CULL, WALK_WIDE, WALK_CWIDE, WALK_TRI64, WALK_CW8, WALK_TRI8 = range(6)
WALK_RECORD_BYTES = (4, 128, 64, 64, 80, 64)
WALK_DIGEST_FIELD = (None, "digest_wide_packets", "digest_cwide_packets", "digest_tri_records", "digest_cw8_packets", "digest_cw8_records")


def host_walk_buffer(nodes, triangles, kind, collapse=-1, packet_order=0):
    """mi3pt_host_walk_buffer: the bytes of one buffer of the scene compile's walk stage as (records, WALK_RECORD_BYTES[kind]) uint8;
    zero records when the compile does not build it for this tree."""
    lib = load_library()
    nd, tr = np.ascontiguousarray(nodes), np.ascontiguousarray(triangles)
    n = ctypes.c_size_t(0)
    args = (_ptr(nd), nd.nbytes, _ptr(tr), tr.nbytes, int(collapse), int(packet_order), int(kind))
    _check(lib, lib.mi3pt_host_walk_buffer(*args, None, 0, ctypes.byref(n)))
    out = np.zeros(max(n.value, 1), np.uint8)
    _check(lib, lib.mi3pt_host_walk_buffer(*args, _ptr(out), out.nbytes, ctypes.byref(n)))
    return out[:n.value].reshape(-1, WALK_RECORD_BYTES[kind])


# mi3pt_host_route's inputs and outputs, in order (include/mi3pt.h)
ROUTE_INPUTS = (
    "variant", "tex_w", "local_rows", "nframes", "num_cus", "waves_per_cu", "ntiles_active", "six_waves",
    "walk_min", "leaf_min", "shade_split", "tail_policy", "job_chunk", "tri_pair", "wave_times", "tile_cost", "service", "diag_lite",
    "max_bounces", "samples_per_frame", "res_x_bits", "res_y_bits", "nnodes", "flags", "root_ref", "leaf_cap", "cwide", "cw8")
ROUTE_BUILD = ("defer", "cull", "wide", "filt", "ymax", "diag", "toplds", "lite", "cw", "wmin", "waves", "w8")      # k_raytrace_sm's template arguments
ROUTE_OUTPUTS = ("kind", "variant", "lean", "blocks", "waves", "ymax", "walk_min") + tuple("build_" + b for b in ROUTE_BUILD) + ("has_kernel", "setup")


def host_route(rows):
    """mi3pt_host_route: the kernel each of `rows` (n x len(ROUTE_INPUTS) integers) would launch, as n x len(ROUTE_OUTPUTS) int64."""
    lib = load_library()
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, len(ROUTE_INPUTS))
    out = np.zeros((len(rows), len(ROUTE_OUTPUTS)), np.int64)
    _check(lib, lib.mi3pt_host_route(_ptr(rows), len(rows), _ptr(out)))
    return out


def host_freeze_tiles(records, threshold, min_frames, guard=1, mask=None):
    """The rule of adaptive sampling (include/mi3pt.h: mi3pt_host_freeze_tiles) on a (tiles_y, tiles_x, 4) tile map as
    read_convergence_tiles returns it and a (tiles_y, tiles_x) mask (None: every tile sampled): (new mask as uint8, sampled tiles).
    Plain host code, no device."""
    lib = load_library()
    rec = np.ascontiguousarray(records, np.float32)
    if rec.ndim != 3 or rec.shape[2] != 4:
        raise ValueError("records must be (tiles_y, tiles_x, 4)")
    ty, tx = rec.shape[:2]
    out = np.ones((ty, tx), np.uint8) if mask is None else (np.asarray(mask).reshape(ty, tx) != 0).astype(np.uint8)
    out = np.ascontiguousarray(out)
    n = ctypes.c_uint32()
    _check(lib, lib.mi3pt_host_freeze_tiles(_ptr(rec), tx, ty, threshold, int(min_frames), int(guard), _ptr(out), ctypes.byref(n)))
    return out, n.value


def host_view_frame(raytrace_uniforms):
    """The camera frame of a 96-byte raytrace uniform block as 16 float32 (include/mi3pt.h: mi3pt_host_view_frame): position, aspect |
    fwd, t | u, r | v, 0 -- what reproject projects the new view's first hits with.  Plain host code, no device."""
    lib = load_library()
    raw = bytes(raytrace_uniforms)
    out = np.zeros(16, np.float32)
    _check(lib, lib.mi3pt_host_view_frame(raw, len(raw), _ptr(out)))
    return out


def host_env_cdf(rgba):
    lib = load_library()
    env = np.ascontiguousarray(rgba, np.float32)
    h, w = env.shape[0], env.shape[1]
    out = np.empty((h, w, 4), np.float32)
    _check(lib, lib.mi3pt_host_env_cdf(_ptr(env), w, h, _ptr(out)))
    return out


class Context:
    """One mi3pt_ctx: a HIP device + stream + the path tracer's device resources."""

    def __init__(self, device=0, devices=None, block_rows=8):
        """device: one GPU.  devices = [d0, d1, ...]: a device group (mi3pt_create_group) -- the same methods, whole
        images in and out, the image's 8-row blocks dealt to one member context per listed device."""
        self.lib = load_library()
        handle = ctypes.c_void_p()
        self.group_size = 1
        self._group_block_rows = block_rows
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices)
            _check(self.lib, self.lib.mi3pt_create_group(arr, len(devices), block_rows, ctypes.byref(handle)))
            self.group_size = len(devices)
        else:
            _check(self.lib, self.lib.mi3pt_create(device, ctypes.byref(handle)))
        self.handle = handle
        self.width = self.height = 0
        self.local_rows = 0
        self._tile = (0, 1, 8)
        self._next_tile = (0, 1, 8)

    def close(self):
        if self.handle and not getattr(self, "_borrowed", False):
            self.lib.mi3pt_destroy(self.handle)
        self.handle = None

    def member(self, index):
        """A member context of a device group (index -1: the presenting context), owned by the group."""
        h = ctypes.c_void_p()
        self._c(self.lib.mi3pt_group_member(self.handle, index, ctypes.byref(h)))
        m = Context.__new__(Context)
        m.lib, m.handle, m._borrowed, m.group_size = self.lib, h, True, 1
        m.width, m.height = self.width, self.height
        n = self.group_size
        m._group_block_rows = 8
        m._tile = m._next_tile = (0, 1, 8) if index < 0 or n == 1 else (index, n, self._group_block_rows)
        m.local_rows = tile_local_rows(self.height, *m._tile) if self.height else 0
        return m

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc):
        _check(self.lib, rc)

    def set_stream(self, stream_ptr):
        self._c(self.lib.mi3pt_set_stream(self.handle, stream_ptr))

    def set_storage(self, storage):
        self._c(self.lib.mi3pt_set_storage(self.handle, storage))

    def set_kernel_variant(self, variant):
        self._c(self.lib.mi3pt_set_kernel_variant(self.handle, variant))

    def set_env_sampling(self, enabled):
        """Run the reference's dormant environment importance sampling (raytrace.wgsl:398-404 un-commented)."""
        self._c(self.lib.mi3pt_set_env_sampling(self.handle, int(bool(enabled))))

    def set_pipelining(self, enabled):
        self._c(self.lib.mi3pt_set_pipelining(self.handle, int(enabled)))

    def set_present_mode(self, mode):
        self._c(self.lib.mi3pt_set_present_mode(self.handle, int(mode)))

    def set_tile(self, rank, nranks, block_rows=8):
        self._c(self.lib.mi3pt_set_tile(self.handle, rank, nranks, block_rows))
        self._next_tile = (rank, nranks, block_rows)

    def upload_triangles(self, tris):
        a = np.ascontiguousarray(tris)
        self._c(self.lib.mi3pt_upload_triangles(self.handle, _ptr(a), a.nbytes))
        self._ntris_uploaded = a.nbytes // 112

    def upload_materials(self, mats):
        a = np.ascontiguousarray(mats)
        self._c(self.lib.mi3pt_upload_materials(self.handle, _ptr(a), a.nbytes))

    def upload_bvh(self, nodes):
        a = np.ascontiguousarray(nodes)
        self._c(self.lib.mi3pt_upload_bvh(self.handle, _ptr(a), a.nbytes))
        self._nnodes_uploaded = a.nbytes // 48

    def upload_environment(self, rgba):
        a = np.ascontiguousarray(rgba, np.float32)
        self._c(self.lib.mi3pt_upload_environment(self.handle, _ptr(a), a.shape[1], a.shape[0]))

    def upload_environment_cdf(self, rgba):
        a = np.ascontiguousarray(rgba, np.float32)
        self._c(self.lib.mi3pt_upload_environment_cdf(self.handle, _ptr(a), a.shape[1], a.shape[0]))

    def resize(self, width, height):
        self._c(self.lib.mi3pt_resize(self.handle, width, height))
        self.width, self.height = width, height
        self._tile = self._next_tile
        self.local_rows = tile_local_rows(height, *self._tile)

    def reset(self):
        self._c(self.lib.mi3pt_reset(self.handle))

    def set_uniforms(self, which, data):
        b = data if isinstance(data, (bytes, bytearray)) else data.tobytes()
        self._c(self.lib.mi3pt_set_uniforms(self.handle, which, b, len(b)))

    def submit(self, mask):
        self._c(self.lib.mi3pt_submit(self.handle, mask))

    def submit_frames(self, mask, count):
        self._c(self.lib.mi3pt_submit_frames(self.handle, mask, count))

    def flush(self):
        self._c(self.lib.mi3pt_flush(self.handle))

    def sync(self):
        self._c(self.lib.mi3pt_sync(self.handle))

    def read_texture(self, which):
        rows = self.height if which == TEX_CANVAS else self.local_rows
        out = np.empty((rows, self.width, 4), np.float32)
        self._c(self.lib.mi3pt_read_texture(self.handle, which, _ptr(out), out.size))
        return out

    def write_texture(self, which, image):
        a = np.ascontiguousarray(image, np.float32)
        self._c(self.lib.mi3pt_write_texture(self.handle, which, _ptr(a), a.size))

    def read_canvas_rgba8(self):
        out = np.empty((self.height, self.width, 4), np.uint8)
        self._c(self.lib.mi3pt_read_canvas_rgba8(self.handle, _ptr(out), out.nbytes))
        return out

    def accumulation_device_ptr(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._c(self.lib.mi3pt_accumulation_device_ptr(self.handle, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def render_aovs(self, mask=AOV_ALL):
        """Render the first-hit feature images named in `mask` (an OR of 1 << AOV_*) from the raytrace uniforms and the
        scene as they are now; asynchronous.  Not a raytrace pass: counters and queued sample frames are untouched."""
        self._c(self.lib.mi3pt_render_aovs(self.handle, int(mask)))

    def read_aov(self, which):
        """Feature image `which` as (rows, width, 4): float32, int32 for AOV_IDS.  rows = this rank's compact rows; a
        device group returns the whole image."""
        out = np.empty((self.local_rows, self.width, 4), np.int32 if which == AOV_IDS else np.float32)
        self._c(self.lib.mi3pt_read_aov(self.handle, int(which), _ptr(out), out.nbytes))
        return out

    def aov_device_ptr(self, which):
        """(device pointer, bytes) of feature image `which`, for zero-copy hand-off; sync() (or order your reads behind
        the context's stream) before reading it."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._c(self.lib.mi3pt_aov_device_ptr(self.handle, int(which), ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def denoise_guided(self, levels=3, sigma_color=1.0, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05, flags=0):
        """Filter the running mean (every frame submitted so far) with the feature-guided a-trous filter of include/mi3pt.h;
        needs all four feature images (render_aovs).  Asynchronous; the accumulation image is untouched.  flags:
        GUIDED_PRESENT draws the canvas from the filtered image."""
        p = GuidedParams(int(levels), float(sigma_color), float(sigma_normal), float(sigma_albedo), float(sigma_plane), int(flags))
        self._c(self.lib.mi3pt_denoise_guided(self.handle, ctypes.byref(p)))

    def read_guided(self):
        """The filtered image of the last denoise_guided as (rows, width, 4) float32."""
        out = np.empty((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.mi3pt_read_guided(self.handle, _ptr(out), out.nbytes))
        return out

    def guided_device_ptr(self):
        """(device pointer, bytes) of the filtered image, for zero-copy hand-off; sync() (or order your reads behind the
        context's stream) before reading it.  Valid until the next denoise_guided or resize."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._c(self.lib.mi3pt_guided_device_ptr(self.handle, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def read_guided_variance(self):
        """The last level's variance image of a denoise_guided with GUIDED_VARIANCE as (rows, width) float32."""
        out = np.empty((self.local_rows, self.width), np.float32)
        self._c(self.lib.mi3pt_read_guided_variance(self.handle, _ptr(out), out.size))
        return out

    def set_guided_despike(self, enabled=True):
        """The firefly pre-pass of denoise_guided (off by default): while on, every denoise_guided first scales a texel brighter
        than all 3 x 3 neighbours of its class (material, hit flag) down to the brightest of them, in the image the filter reads;
        the accumulation image is untouched."""
        self._c(self.lib.mi3pt_set_guided_despike(self.handle, int(bool(enabled))))

    def read_guided_despiked(self):
        """The number of texels the pre-pass of the last denoise_guided clamped (blocking)."""
        n = ctypes.c_uint32()
        self._c(self.lib.mi3pt_read_guided_despiked(self.handle, ctypes.byref(n)))
        return n.value

    def set_moments(self, enabled=True):
        """Keep the moments image (M2.rgb, n: Welford's sums around the running mean) beside the accumulation image from now
        on; allocates and zeroes it, False frees it.  The mean is bit-identical with and without."""
        self._c(self.lib.mi3pt_set_moments(self.handle, int(bool(enabled))))

    def read_moments(self):
        """The moments image as (rows, width, 4) float32: M2.r, M2.g, M2.b, n.  rows = this rank's compact rows; a device
        group returns the whole image."""
        out = np.empty((self.local_rows, self.width, 4), np.float32)
        self._c(self.lib.mi3pt_read_moments(self.handle, _ptr(out), out.nbytes))
        return out

    def write_moments(self, image):
        """Load a saved moments image (checkpoint / resume; after write_texture, which zeroes it)."""
        a = np.ascontiguousarray(image, np.float32)
        self._c(self.lib.mi3pt_write_moments(self.handle, _ptr(a), a.nbytes))

    def moments_device_ptr(self):
        """(device pointer, bytes) of the moments image, for zero-copy hand-off; sync() before reading it.  Valid until the
        next resize or set_moments."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._c(self.lib.mi3pt_moments_device_ptr(self.handle, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def estimate_convergence(self, threshold, min_frames=16):
        """Reduce the running mean and its moments image to one error record per 8 x 8 tile and a summary (include/mi3pt.h:
        mi3pt_estimate_convergence), of every frame submitted so far.  Asynchronous; needs set_moments(True)."""
        self._c(self.lib.mi3pt_estimate_convergence(self.handle, threshold, int(min_frames)))

    def read_convergence(self):
        """The summary of the last estimate_convergence as a dict of the nine fields of mi3pt_convergence.  Waits for that estimate
        only: frames flushed after it keep running.  Converged: tiles > 0 and tiles_above == 0."""
        c = Convergence()
        self._c(self.lib.mi3pt_read_convergence(self.handle, ctypes.byref(c)))
        return {name: getattr(c, name) for name, _ in Convergence._fields_}

    def read_convergence_tiles(self):
        """The tile map of the last estimate_convergence as (tiles_y, tiles_x, 4) float32: sum_r, max_r, count, n_min per 8 x 8
        tile of this rank's compact rows; a device group whose block_rows is a multiple of 8 returns the whole image's."""
        out = np.empty(((self.local_rows + 7) // 8, (self.width + 7) // 8, 4), np.float32)
        self._c(self.lib.mi3pt_read_convergence_tiles(self.handle, _ptr(out), out.size))
        return out

    def _mask_shape(self):
        return ((self.local_rows + 7) // 8, (self.width + 7) // 8)

    def set_sample_mask(self, mask):
        """Adaptive sampling (include/mi3pt.h: mi3pt_set_sample_mask): one value per 8 x 8 tile of this rank's compact rows (a device
        group: of the whole image), non-zero = sampled, zero = frozen; None removes the mask.  Frames queued so far run under the
        old mask.  reset() and resize() drop it."""
        if mask is None:
            self._c(self.lib.mi3pt_set_sample_mask(self.handle, None, 0))
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        self._c(self.lib.mi3pt_set_sample_mask(self.handle, _ptr(m), m.size))

    def read_sample_mask(self):
        """The sample mask as (tiles_y, tiles_x) uint8 of 0 / 1 (no mask: all 1)."""
        out = np.empty(self._mask_shape(), np.uint8)
        n = ctypes.c_uint32()
        self._c(self.lib.mi3pt_read_sample_mask(self.handle, _ptr(out), out.size, ctypes.byref(n)))
        return out

    def freeze_converged(self, guard=1):
        """Freeze the tiles the last estimate_convergence found under its threshold (guard 1: and whose eight neighbours are, too);
        returns the number of tiles still sampled.  Waits for that estimate only."""
        n = ctypes.c_uint32()
        self._c(self.lib.mi3pt_freeze_converged(self.handle, int(guard), ctypes.byref(n)))
        return n.value

    def set_mean_by_count(self, enabled=True):
        """The mean by count (include/mi3pt.h: mi3pt_set_mean_by_count): every accumulate step takes its weight from the texel's own
        sample count, the moments image's n, instead of the accumulate block's `frame`.  Needs set_moments(True)."""
        self._c(self.lib.mi3pt_set_mean_by_count(self.handle, int(bool(enabled))))

    def reproject(self, plane_tolerance=0.02, normal_cos_min=0.9, max_history=64, flags=0):
        """Carry the running mean and its moments from the view the POSITION / NORMAL / IDS images were rendered in into the view of the
        raytrace uniforms as they stand (include/mi3pt.h: mi3pt_reproject); renders all four feature images of the new view on the way
        and drops the sample mask.  Asynchronous.  Needs set_moments(True) and set_mean_by_count(True)."""
        p = ReprojectParams(plane_tolerance, normal_cos_min, int(max_history), int(flags))
        self._c(self.lib.mi3pt_reproject(self.handle, ctypes.byref(p)))

    def keep_geometry(self, keep=True):
        """Remember the triangle records as they are uploaded now as the previous geometry of reproject_scene (include/mi3pt.h:
        mi3pt_keep_geometry); the next upload_triangles hands the buffer over instead of freeing it: 112 B per triangle until
        keep_geometry(False)."""
        self._c(self.lib.mi3pt_keep_geometry(self.handle, int(bool(keep))))

    def reproject_scene(self, plane_tolerance=0.02, normal_cos_min=0.9, max_history=64, max_history_moved=8, flags=0):
        """reproject across a scene change (include/mi3pt.h: mi3pt_reproject_scene): a texel whose triangle moved since keep_geometry
        looks its point of the kept triangle up in the old view and carries at most max_history_moved samples; the others are
        reproject's, bit for bit.  The POSITION / NORMAL / IDS images must be of the kept geometry.  Asynchronous."""
        p = ReprojectSceneParams(plane_tolerance, normal_cos_min, int(max_history), int(max_history_moved), int(flags))
        self._c(self.lib.mi3pt_reproject_scene(self.handle, ctypes.byref(p)))

    def hold_history(self):
        """Set the running mean and its moments aside as the held history and leave the live pair zero-filled, as reset leaves it
        (include/mi3pt.h: mi3pt_hold_history); output, canvas, feature images, sample mask and counters stay.  Asynchronous.  Needs
        set_moments(True) and set_mean_by_count(True)."""
        self._c(self.lib.mi3pt_hold_history(self.handle))

    def merge_history(self, radius=1, z_keep=2.0, z_drop=4.0, flags=0):
        """Merge the held history into the mean sampled since hold_history, per texel as much of it as a two-sample test over a
        (2 * radius + 1)^2 window supports: all of it up to z_keep, none from z_drop (include/mi3pt.h: mi3pt_merge_history).
        Asynchronous."""
        p = HistoryParams(int(radius), z_keep, z_drop, int(flags))
        self._c(self.lib.mi3pt_merge_history(self.handle, ctypes.byref(p)))

    def bind_accumulation(self, dev_ptr, nbytes):
        self._c(self.lib.mi3pt_bind_accumulation(self.handle, dev_ptr, nbytes))

    def enable_timing(self, enabled=True):
        self._c(self.lib.mi3pt_enable_timing(self.handle, int(enabled)))

    def pass_time_us(self, which):
        v = ctypes.c_float()
        self._c(self.lib.mi3pt_pass_time_us(self.handle, which, ctypes.byref(v)))
        return v.value

    def raytrace_launch_stats(self, reset=False):
        """(total GPU ms, launches, frames) of the batched raytrace kernel since the last reset."""
        ms, n, f = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        self._c(self.lib.mi3pt_raytrace_launch_stats(self.handle, int(reset), ctypes.byref(ms), ctypes.byref(n),
                                                     ctypes.byref(f)))
        return ms.value, n.value, f.value

    def set_packet_layout(self, layout):
        self._c(self.lib.mi3pt_debug_set_packet_layout(self.handle, int(layout)))

    def set_option(self, option, value):
        """Scheduling options (OPT_*): how the work is cut into launches / steps / jobs; never what is computed."""
        self._c(self.lib.mi3pt_debug_set_option(self.handle, int(option), int(value)))

    def get_option(self, option):
        v = ctypes.c_int(0)
        self._c(self.lib.mi3pt_debug_get_option(self.handle, int(option), ctypes.byref(v)))
        return v.value

    def active_variant(self):
        v = ctypes.c_int()
        self._c(self.lib.mi3pt_debug_active_variant(self.handle, ctypes.byref(v)))
        return v.value

    def last_launch(self):
        """The kernel the most recent raytrace launch ran: dict(kind, variant, lean, workgroups) -- mi3pt_debug_last_launch."""
        k, v, l, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._c(self.lib.mi3pt_debug_last_launch(self.handle, ctypes.byref(k), ctypes.byref(v), ctypes.byref(l), ctypes.byref(w)))
        b = self.get_option(OPT_LAST_BUILD)
        return {"kind": k.value, "variant": v.value, "lean": bool(l.value), "workgroups": w.value,
                "waves_per_simd": b & 0xff, "ymax": bool(b & 0x100), "walk_min": (b >> 16) & 0xff}

    def batch_capacity(self):
        n = ctypes.c_int()
        self._c(self.lib.mi3pt_batch_capacity(self.handle, ctypes.byref(n)))
        return n.value

    def raytrace_launch_span(self):
        """GPU-clock ms from the start of the first to the end of the last batched launch since the reset."""
        ms = ctypes.c_double()
        self._c(self.lib.mi3pt_raytrace_launch_span(self.handle, ctypes.byref(ms)))
        return ms.value

    def counters(self):
        out = np.zeros(8, np.uint64)
        self._c(self.lib.mi3pt_get_counters(self.handle, _ptr(out)))
        return dict(zip(COUNTER_NAMES, (int(x) for x in out)))

    def reset_counters(self):
        self._c(self.lib.mi3pt_reset_counters(self.handle))

    def debug_intersect(self, rays):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.empty((len(r), 12), np.float32)
        self._c(self.lib.mi3pt_debug_intersect(self.handle, _ptr(r), len(r), _ptr(out)))
        return out

    def debug_intersect_shipped(self, rays):
        """debug_intersect's 12 floats per ray from the shipped first-hit walk (slots 9 / 10: node steps, leaves whose own box passed);
        Mi3ptError (state) where mi3pt_render_aovs would not run that walk."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.empty((len(r), 12), np.float32)
        self._c(self.lib.mi3pt_debug_intersect_shipped(self.handle, _ptr(r), len(r), _ptr(out)))
        return out

    def debug_pairs(self, fn, rays, geom):
        """The kernels' box (fn 0, geom n x 7: min, max, box_unsafe) / triangle (fn 1, geom n x 9: a, b, c) decisions per pair: n x 12
        (include/mi3pt.h: mi3pt_debug_pairs)."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        g = np.ascontiguousarray(geom, np.float32).reshape(len(r), 7 if fn == 0 else 9)
        out = np.empty((len(r), 12), np.float32)
        self._c(self.lib.mi3pt_debug_pairs(self.handle, fn, _ptr(r), _ptr(g), _ptr(out), len(r)))
        return out

    def enable_wave_times(self, enabled=True):
        self._c(self.lib.mi3pt_debug_wave_times(self.handle, int(enabled), None, 0, None))

    def wave_times(self):
        out = np.zeros((6144, 16), np.uint64)
        n = ctypes.c_size_t()
        self._c(self.lib.mi3pt_debug_wave_times(self.handle, 1, _ptr(out), len(out), ctypes.byref(n)))
        return out[:n.value]

    def device_build_bvh(self, method="lbvh", radius=16, max_search_iterations=1024):
        """A tree over the uploaded triangles, built on the device: (nodes, info), the records ready for upload_bvh.  An alternative to
        the reference's SAH tree (host_build_bvh_f64), in the same 48-byte records.  method "lbvh": the linear BVH (with no arguments,
        mi3pt_device_build_bvh as ever); "ploc": the locally-ordered clustering of include/mi3pt.h (mi3pt_device_build_bvh_ex), with
        its two parameters.  info is a BvhBuildInfo: the device time in milliseconds as a float, with the iteration counts as attributes."""
        from . import layout
        if method not in BVH_METHODS:
            raise ValueError(f"device_build_bvh: method {method!r} is none of {sorted(BVH_METHODS)}")
        n = ctypes.c_size_t()
        ntris = getattr(self, "_ntris_uploaded", 0)
        if ntris == 0:
            raise Mi3ptError(4, "no triangles uploaded")
        nodes = np.zeros(2 * ntris - 1, layout.BVH_NODE)
        if method == "lbvh":
            ms = ctypes.c_float()
            self._c(self.lib.mi3pt_device_build_bvh(self.handle, _ptr(nodes), nodes.nbytes, ctypes.byref(n), ctypes.byref(ms)))
            return nodes[: n.value], BvhBuildInfo(ms.value)
        params = BvhBuildParams(BVH_METHODS[method], int(radius), int(max_search_iterations), 0)
        info = BvhBuildInfoStruct()
        self._c(self.lib.mi3pt_device_build_bvh_ex(self.handle, ctypes.byref(params), _ptr(nodes), nodes.nbytes, ctypes.byref(n),
                                                   ctypes.byref(info)))
        return nodes[: n.value], BvhBuildInfo(info.build_ms, info.search_iterations, info.forced_iterations)

    def device_refit_bvh(self):
        """mi3pt_device_refit_bvh: the boxes of the uploaded tree re-fitted on the device to the triangles as uploaded since:
        (nodes, refit_ms), the records ready for upload_bvh.  The context's state does not move."""
        from . import layout
        n = ctypes.c_size_t()
        ms = ctypes.c_float()
        nodes = np.zeros(max(getattr(self, "_nnodes_uploaded", 0), 1), layout.BVH_NODE)      # (before the uploads: the library says so)
        self._c(self.lib.mi3pt_device_refit_bvh(self.handle, _ptr(nodes), nodes.nbytes, ctypes.byref(n), ctypes.byref(ms)))
        return nodes[: n.value], ms.value

    def debug_math(self, fn, a, b=None):
        a = np.ascontiguousarray(a, np.float32)
        out = np.empty_like(a)
        bb = np.ascontiguousarray(b, np.float32) if b is not None else None
        self._c(self.lib.mi3pt_debug_math(self.handle, fn, _ptr(a), _ptr(bb) if bb is not None else None,
                                          _ptr(out), a.size))
        return out
