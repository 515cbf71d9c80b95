"""ctypes binding of libflatmatch_gi.so (include/flatmatch_gi.h). No fallback: if the HIP library is
missing or a call fails, an exception is raised -- there is no CPU path in the product."""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# FMGI_LIB=<name> selects a profiling/experiment build libflatmatch_gi_<name>.so (make -C <pkg> timing,
# make -C <pkg> experiments (FMGI_LIB=exp: the experiment knobs), make -C <pkg> variant VNAME=<name> VFLAGS=...);
# the product and every test use libflatmatch_gi.so
LIB_PATH = os.path.join(PKG_DIR, f"libflatmatch_gi_{os.environ['FMGI_LIB']}.so" if os.environ.get("FMGI_LIB")
                        else "libflatmatch_gi.so")

# Exported symbols of the C ABI (tests check the built library exports exactly these + nothing
# that would clash with the reference objects main.c links against).
EXPORTS = (
    "performGlobalIlluminationCl",
    "getGlobalIlluminationCl",
    "fmgi_dropin_release",
    "fmgi_dropin_shards",
    "fmgi_dropin_reduce_order",
    "fmgi_dropin_rccl_ranks",
    "fmgi_version",
    "fmgi_last_error",
    "fmgi_device_count",
    "fmgi_create",
    "fmgi_destroy",
    "fmgi_set_scene",
    "fmgi_set_accumulation",
    "fmgi_get_accumulation",
    "fmgi_plan",
    "fmgi_get_plan",
    "fmgi_plan_count",
    "fmgi_bake_items",
    "fmgi_finalize",
    "fmgi_get_stats",
    "fmgi_reset_stats",
    "fmgi_trace_items",
    "fmgi_host_sincosf",
    "fmgi_device_sincosf",
    "fmgi_device_sincosf_library",
    "fmgi_device_unit",
    "fmgi_grid_sizes",
    "fmgi_set_grid_cells_per_record",
    "fmgi_experiments",
    "fmgi_set_option",
    "fmgi_grid_copy",
    "fmgi_lattice_copy",
    "fmgi_plan_copy",
    "fmgi_filter_copy",
    "fmgi_pairs_copy",
    "fmgi_get_stage_cycles",
    "fmgi_auto_kernel",
    "fmgi_last_bake_kernel",
    "fmgi_set_timing",
    "fmgi_get_timing",
    "performAmbientOcclusionGpu",
    "fmgi_ambient_occlusion",
    "fmgi_geosphere",
    "fmgi_ao_tree",
    "fmgi_output_tiles",
    "fmgi_output_tile_bytes",
    "performRadiosityGpu",
    "fmgi_radiosity",
    "fmgi_radiosity_jobs",
    "fmgi_radiosity_stats",
    "fmgi_rand_skip",
    "fmgi_rad_cache_bytes",
    "fmgi_rad_cache_create",
    "fmgi_rad_cache_destroy",
    "fmgi_rad_cache_info",
    "fmgi_rad_cache_sids",
    "fmgi_rad_reference_emit",
    "fmgi_rad_cache_solve",
    "fmgi_render_views",
    "fmgi_view_candidates",
    "fmgi_view_stats",
    "fmgi_shade_views",
    "fmgi_view_cache_bytes",
    "fmgi_view_cache_create",
    "fmgi_view_cache_destroy",
    "fmgi_view_cache_info",
    "fmgi_view_cache_tiles",
    "fmgi_view_cache_shade",
    "fmgi_shade_views_proj",
    "fmgi_view_candidates_proj",
    "fmgi_view_cache_create_proj",
    "fmgi_view_cache_projection",
    "fmgi_shade_views_gloss",
    "fmgi_view_gloss_stats",
    "fmgi_view_cache_create_gloss",
    "fmgi_view_cache_shade_gloss",
    "fmgi_view_cache_has_mirror",
    "fmgi_palette_reference",
    "fmgi_palette_table",
    "fmgi_states_bytes",
    "fmgi_bake_states",
    "fmgi_recolour",
    "fmgi_sparse_bytes",
    "fmgi_sparse_measure",
    "fmgi_sparse_compact",
    "fmgi_sparse_expand",
    "fmgi_recolour_sparse",
    "fmgi_sparse_check",
    "fmgi_bake_sparse_supported",
    "fmgi_bake_sparse",
    "fmgi_bake_sparse_take",
    "fmgi_sparse_from_codes",
    "fmgi_sparse_add_measure",
    "fmgi_sparse_add",
    "fmgi_bake_sparse_get_stats",
    "fmgi_filter_energy",
    "fmgi_filter_radii",
    "fmgi_filter_apply",
    "fmgi_sun_coverage",
    "fmgi_sun_get_stats",
    "fmgi_sun_add",
    "fmgi_sun_units",
    "fmgi_rad_cache_sun_bounce",
    "fmgi_sun_add_bounced",
)

KERNEL_EXACT = 0
KERNEL_FAST = 1
KERNEL_GRID = 2
KERNEL_HYBRID = 4
KERNEL_AUTO = 3
ACCUM_AUTO = 0
ACCUM_FX3 = 1
ACCUM_STATE = 2
ACCUM_NONE = 3  # profiling only: deposits discarded
ACCUM_STREAM = 4
VIEW_NEAREST = 0
VIEW_BILINEAR = 1
VIEW_MAX_SAMPLES = 8
VIEW_CACHE_MAX_SETS = 8
PROJ_PINHOLE = 0
PROJ_ORTHO = 1
PROJ_EQUIRECT = 2
RAD_CACHE_MAX_SETS = 8
RAD_CACHE_MAX_ITERATIONS = 64
COLOUR_STATE_COUNT = 1024
RECOLOUR_MAX_SCENARIOS = 8
SPARSE_COUNT_BITS = 54
FILTER_MAX_RADIUS = 16
FILTER_MAX_MAPS = 8
SUN_MAX_SAMPLES = 8
SUN_MAX_MAPS = 8
SUN_LISTS = 0
SUN_ALL = 1
SUN_BOUNCE_MAX_DIRS = 32
SUN_MAX_BOUNCES = 8
# fmgi_set_option (include/flatmatch_gi.h): tests' handles on product paths a scene would not take
OPTIONS = {"chunk_items": 1, "pool_limit": 2, "stream_layout": 3, "bucket_fill": 4, "wide_tiles": 5, "coop": 6,
           "no_axes": 7, "photon_lock": 8, "lattice": 9, "hist_batch": 10}


class FmgiError(RuntimeError):
    pass


class Stats(C.Structure):
    _fields_ = [
        ("photons", C.c_uint64),
        ("scans", C.c_uint64),
        ("deposits", C.c_uint64),
        ("escapes", C.c_uint64),
        ("exact_rescans", C.c_uint64),
        ("tests", C.c_uint64),
        ("rescans_tie", C.c_uint64),
        ("rescans_invalid", C.c_uint64),
        ("stream_overflow", C.c_uint64),
        ("bucket_fallback_codes", C.c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SunStats(C.Structure):
    """fmgi_sun_stats (include/flatmatch_gi.h)."""

    _fields_ = [
        ("samples", C.c_int64),
        ("facing", C.c_int64),
        ("crossing", C.c_int64),
        ("lit", C.c_int64),
        ("list_entries", C.c_int64),
        ("tests", C.c_int64),
        ("list_ms", C.c_double),
        ("rays_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: (float if k.endswith("ms") else int)(getattr(self, k)) for k, _ in self._fields_}


class Timing(C.Structure):
    _fields_ = [
        ("bake_ms", C.c_double),
        ("fold_ms", C.c_double),
        ("bake_launches", C.c_uint64),
        ("fold_launches", C.c_uint64),
    ]

    def as_dict(self):
        return {k: (float if k.endswith("ms") else int)(getattr(self, k)) for k, _ in self._fields_}


class RadStats(C.Structure):
    """fmgi_rad_stats (include/flatmatch_gi.h)."""

    _fields_ = [
        ("jobs", C.c_int64),
        ("rects", C.c_int64),
        ("texels", C.c_int64),
        ("rays", C.c_int64),
        ("rand_ms", C.c_double),
        ("rays_ms", C.c_double),
        ("bounce_ms", C.c_double),
        ("total_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: (float if k.endswith("ms") else int)(getattr(self, k)) for k, _ in self._fields_}


class RadCacheInfo(C.Structure):
    """struct fmgi_rad_cache_info (include/flatmatch_gi.h)."""

    _fields_ = [
        ("jobs", C.c_int64),
        ("rects", C.c_int64),
        ("windows", C.c_int64),
        ("lights", C.c_int64),
        ("texels", C.c_int64),
        ("rays", C.c_int64),
        ("bytes", C.c_int64),
        ("rand_ms", C.c_double),
        ("rays_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: (float if k.endswith("ms") else int)(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(RadCacheInfo) == 72


class ViewStats(C.Structure):
    """struct fmgi_view_stats (include/flatmatch_gi.h)."""

    _fields_ = [
        ("cameras", C.c_int64),
        ("rays", C.c_int64),
        ("candidates", C.c_int64),
        ("tests", C.c_int64),
        ("cand_ms", C.c_double),
        ("rays_ms", C.c_double),
        ("total_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: (float if k.endswith("ms") else int)(getattr(self, k)) for k, _ in self._fields_}


class ViewGlossStats(C.Structure):
    """struct fmgi_view_gloss_stats (include/flatmatch_gi.h)."""

    _fields_ = [("mirror_rays", C.c_int64), ("mirror_hits", C.c_int64), ("mirror_tests", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ViewCacheInfo(C.Structure):
    """struct fmgi_view_cache_info (include/flatmatch_gi.h)."""

    _fields_ = [
        ("cameras", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("samples", C.c_int32),
        ("filter", C.c_int32),
        ("num_texels", C.c_int32),
        ("tiles", C.c_int64),
        ("rays", C.c_int64),
        ("hits", C.c_int64),
        ("tests", C.c_int64),
        ("bytes", C.c_int64),
        ("cand_ms", C.c_double),
        ("trace_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: (float if k.endswith("ms") else int)(getattr(self, k)) for k, _ in self._fields_}


assert C.sizeof(ViewCacheInfo) == 80


class Palette(C.Structure):
    """fmgi_palette (include/flatmatch_gi.h): the colours a bake's histogram is folded with. Palette() is the
    reference's (photonmap.cl:167-169, 241-249); keywords replace single constants, e.g.
    Palette(light_rgb=(0, 0, 0)) switches the lamps off."""

    _fields_ = [
        ("window_rgb", C.c_float * 3),
        ("light_rgb", C.c_float * 3),
        ("floor_tint", C.c_float * 3),
        ("albedo", C.c_float),
    ]

    def __init__(self, window_rgb=(18, 18, 18), light_rgb=(16, 16, 18), floor_tint=(1.0, 0.85, 0.7), albedo=0.9):
        super().__init__()
        for name, v in (("window_rgb", window_rgb), ("light_rgb", light_rgb), ("floor_tint", floor_tint)):
            v = tuple(float(x) for x in v)
            if len(v) != 3:
                raise ValueError(f"{name}: three channels")
            setattr(self, name, (C.c_float * 3)(*v))
        self.albedo = float(albedo)

    @classmethod
    def reference(cls) -> "Palette":
        p = cls()
        load().fmgi_palette_reference(C.byref(p))
        return p

    def as_dict(self):
        return {"window_rgb": list(self.window_rgb), "light_rgb": list(self.light_rgb),
                "floor_tint": list(self.floor_tint), "albedo": float(self.albedo)}


assert C.sizeof(Palette) == 40


class SparseInfo(C.Structure):
    """fmgi_sparse_info (include/flatmatch_gi.h): the size and the sums of one sparse histogram blob."""

    _fields_ = [
        ("num_texels", C.c_int32),
        ("num_blocks", C.c_int32),
        ("rows", C.c_uint64),
        ("cells", C.c_uint64),
        ("deposits", C.c_uint64),
        ("too_large", C.c_uint64),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def __eq__(self, other):
        return isinstance(other, SparseInfo) and self.as_dict() == other.as_dict()

    __hash__ = None

    def __repr__(self):
        return f"SparseInfo({', '.join(f'{k}={v}' for k, v in self.as_dict().items())})"


assert C.sizeof(SparseInfo) == 40


class BakeSparseStats(C.Structure):
    """fmgi_bake_sparse_stats (include/flatmatch_gi.h): the last bake_sparse / sparse_from_codes of a context."""

    _fields_ = [
        ("chunks", C.c_uint64),
        ("merges", C.c_uint64),
        ("dense_chunks", C.c_uint64),
        ("codes", C.c_uint64),
        ("scratch_bytes", C.c_uint64),
    ]


assert C.sizeof(BakeSparseStats) == 40


class Geometry(C.Structure):
    """geometry.h:7-15 (80 B)."""

    _fields_ = [
        ("windows", C.c_void_p),
        ("lights", C.c_void_p),
        ("walls", C.c_void_p),
        ("boxWalls", C.c_void_p),
        ("numWindows", C.c_int32),
        ("numLights", C.c_int32),
        ("numWalls", C.c_int32),
        ("numBoxWalls", C.c_int32),
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("startingPositionX", C.c_float),
        ("startingPositionY", C.c_float),
        ("numTexels", C.c_int32),
        ("texels", C.c_void_p),
    ]


assert C.sizeof(Geometry) == 80

_lib = None


def load() -> C.CDLL:
    """Load the in-tree HIP library (built by __graft_entry__.build() / `make -C <pkg>`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FmgiError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` (no CPU fallback exists)")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64. Loaded first, it
    # satisfies this library's libamdhip64 dependency too; loaded second, a process ends up with two
    # runtimes that enumerate devices independently (observed: one of them then sees no GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    sig = {
        "fmgi_version": (C.c_char_p, []),
        "fmgi_last_error": (C.c_char_p, []),
        "fmgi_device_count": (C.c_int, []),
        "fmgi_create": (vp, [C.c_int]),
        "fmgi_destroy": (None, [vp]),
        "fmgi_set_scene": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int]),
        "fmgi_set_accumulation": (C.c_int, [vp, C.c_int]),
        "fmgi_get_accumulation": (C.c_int, [vp]),
        "fmgi_plan": (i64, [vp, C.c_int, C.c_int, vp, i64, C.POINTER(u64)]),
        "fmgi_get_plan": (i64, [vp, vp, i64]),
        "fmgi_plan_count": (i64, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(u64)]),
        "fmgi_bake_items": (C.c_int, [vp, u64, u64, vp, C.c_int, vp]),
        "fmgi_finalize": (C.c_int, [vp, vp, vp, vp, vp]),
        "fmgi_get_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "fmgi_reset_stats": (C.c_int, [vp]),
        "fmgi_trace_items": (C.c_int, [vp, u64, u64, C.c_int, vp, vp, vp]),
        "fmgi_host_sincosf": (None, [vp, vp, vp, i64]),
        "fmgi_device_sincosf": (C.c_int, [vp, vp, vp, vp, i64]),
        "fmgi_dropin_shards": (C.c_int, [C.c_uint64, C.c_int, C.c_int, vp, vp, vp]),
        "fmgi_dropin_reduce_order": (C.c_int, [C.c_int, vp, vp]),
        "fmgi_dropin_release": (None, []),
        "fmgi_dropin_rccl_ranks": (C.c_int, []),
        "fmgi_device_sincosf_library": (C.c_int, [vp, vp, vp, vp, i64]),
        "fmgi_device_unit": (C.c_int, [vp, C.c_int, vp, vp, vp, i64]),
        "fmgi_grid_sizes": (C.c_int, [vp, vp]),
        "fmgi_set_grid_cells_per_record": (C.c_int, [vp, C.c_int]),
        "fmgi_experiments": (C.c_int, []),
        "fmgi_set_option": (C.c_int, [vp, C.c_int, C.c_int64]),
        "fmgi_get_stage_cycles": (C.c_int, [vp, vp]),
        "fmgi_auto_kernel": (C.c_int, [vp]),
        "fmgi_last_bake_kernel": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "fmgi_set_timing": (C.c_int, [vp, C.c_int]),
        "fmgi_get_timing": (C.c_int, [vp, C.POINTER(Timing)]),
        "performAmbientOcclusionGpu": (None, [vp]),
        "fmgi_ambient_occlusion": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "fmgi_geosphere": (C.c_int, [C.c_int, vp, C.c_int]),
        "fmgi_ao_tree": (i64, [vp, vp, i64]),
        "fmgi_output_tiles": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
        "fmgi_output_tile_bytes": (i64, [vp]),
        "performRadiosityGpu": (None, [vp]),
        "fmgi_radiosity": (C.c_int, [vp, vp, vp]),
        "fmgi_radiosity_jobs": (i64, [vp]),
        "fmgi_radiosity_stats": (C.c_int, [C.POINTER(RadStats)]),
        "fmgi_rand_skip": (C.c_int, [C.c_uint64]),
        "fmgi_rad_cache_bytes": (i64, [vp]),
        "fmgi_rad_cache_create": (C.c_int, [vp, C.POINTER(vp)]),
        "fmgi_rad_cache_destroy": (None, [vp]),
        "fmgi_rad_cache_info": (C.c_int, [vp, C.POINTER(RadCacheInfo)]),
        "fmgi_rad_cache_sids": (C.c_int, [vp, vp]),
        "fmgi_rad_reference_emit": (C.c_int, [vp, vp]),
        "fmgi_rad_cache_solve": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
        "fmgi_render_views": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
        "fmgi_view_candidates": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "fmgi_view_stats": (C.c_int, [C.POINTER(ViewStats)]),
        "fmgi_shade_views": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]),
        "fmgi_view_cache_bytes": (i64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "fmgi_view_cache_create": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
        "fmgi_view_cache_destroy": (None, [vp]),
        "fmgi_view_cache_info": (C.c_int, [vp, C.POINTER(ViewCacheInfo)]),
        "fmgi_view_cache_tiles": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
        "fmgi_view_cache_shade": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, vp]),
        "fmgi_shade_views_proj": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]),
        "fmgi_view_candidates_proj": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int]),
        "fmgi_view_cache_create_proj": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(vp)]),
        "fmgi_view_cache_projection": (C.c_int, [vp]),
        "fmgi_shade_views_gloss": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int,
                                             C.c_float, vp, vp]),
        "fmgi_view_gloss_stats": (C.c_int, [C.POINTER(ViewGlossStats)]),
        "fmgi_view_cache_create_gloss": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(vp)]),
        "fmgi_view_cache_shade_gloss": (C.c_int, [vp, vp, C.c_int, vp, C.c_float, vp, vp, vp]),
        "fmgi_view_cache_has_mirror": (C.c_int, [vp]),
        "fmgi_palette_reference": (None, [C.POINTER(Palette)]),
        "fmgi_palette_table": (C.c_int, [C.POINTER(Palette), vp]),
        "fmgi_states_bytes": (C.c_size_t, [C.c_int]),
        "fmgi_bake_states": (C.c_int, [vp, u64, u64, vp, C.c_int, vp]),
        "fmgi_recolour": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, vp]),
        "fmgi_sparse_bytes": (C.c_size_t, [C.c_int, u64]),
        "fmgi_sparse_measure": (C.c_int, [vp, vp, C.POINTER(SparseInfo), vp]),
        "fmgi_sparse_compact": (C.c_int, [vp, vp, C.POINTER(SparseInfo), vp, vp]),
        "fmgi_sparse_expand": (C.c_int, [vp, vp, C.POINTER(SparseInfo), vp, vp]),
        "fmgi_recolour_sparse": (C.c_int, [vp, vp, C.POINTER(SparseInfo), C.c_int, vp, C.c_int, vp, vp]),
        "fmgi_sparse_check": (C.c_int, [vp, C.c_size_t, C.c_int, C.POINTER(SparseInfo)]),
        "fmgi_bake_sparse_supported": (C.c_int, [vp]),
        "fmgi_bake_sparse": (C.c_int, [vp, u64, u64, C.c_int, C.POINTER(SparseInfo), vp]),
        "fmgi_bake_sparse_take": (C.c_int, [vp, C.POINTER(SparseInfo), vp, vp]),
        "fmgi_sparse_from_codes": (C.c_int, [vp, vp, u64, C.POINTER(SparseInfo), C.POINTER(u64), vp]),
        "fmgi_sparse_add_measure": (C.c_int, [vp, vp, C.POINTER(SparseInfo), vp, C.POINTER(SparseInfo),
                                              C.POINTER(SparseInfo), vp]),
        "fmgi_sparse_add": (C.c_int, [vp, vp, C.POINTER(SparseInfo), vp, C.POINTER(SparseInfo),
                                      C.POINTER(SparseInfo), vp, vp]),
        "fmgi_bake_sparse_get_stats": (C.c_int, [vp, C.POINTER(BakeSparseStats)]),
        "fmgi_filter_energy": (u64, [C.POINTER(Palette), u64]),
        "fmgi_filter_radii": (C.c_int, [vp, vp, u64, C.c_int, vp, vp]),
        "fmgi_filter_apply": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
        "fmgi_sun_coverage": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
        "fmgi_sun_get_stats": (C.c_int, [vp, C.POINTER(SunStats)]),
        "fmgi_sun_add": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_double, vp, vp]),
        "fmgi_sun_units": (C.c_int, [vp, vp, vp, C.c_double, vp]),
        "fmgi_rad_cache_sun_bounce": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]),
        "fmgi_sun_add_bounced": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int, C.c_double, vp, vp]),
        "fmgi_grid_copy": (C.c_int, [vp, vp, vp, vp, vp]),
        "fmgi_lattice_copy": (C.c_int, [vp, vp]),
        "fmgi_plan_copy": (C.c_int, [vp, vp, vp]),
        "fmgi_filter_copy": (C.c_int, [vp, vp, vp, vp]),
        "fmgi_pairs_copy": (C.c_int, [vp, vp, vp, vp]),
        "getGlobalIlluminationCl": (C.c_int, [C.POINTER(Geometry), C.c_int, vp]),
        "performGlobalIlluminationCl": (None, [C.POINTER(Geometry), C.c_int]),
    }
    for name, (res, args) in sig.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            if os.environ.get("FMGI_LIB") == "base":  # an A/B build of an earlier commit may predate a symbol
                continue
            raise
        f.restype = res
        f.argtypes = args
    _ = i32
    _lib = lib
    return lib


def last_error() -> str:
    msg = load().fmgi_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise FmgiError(f"{what} failed ({rc}): {last_error()}")
    return rc
