"""fmgi -- Python mirror of the MI355X photon-mapping lightmap baker's C ABI.

The product is libflatmatch_gi.so (HIP kernels for gfx950 + the C ABI of include/flatmatch_gi.h);
this package only binds it with ctypes for tests, bench.py and Python callers:

  * ``Context``      -- fmgi_create / fmgi_set_scene / fmgi_plan / fmgi_bake_items / fmgi_finalize;
  * ``bake_geometry`` -- getGlobalIlluminationCl on host arrays (the reference's
                         performGlobalIlluminationCl semantics, global_illumination_cl.c:275-321);
  * ``scene``        -- the Rectangle/Geometry layout, fixtures and synthetic box scenes.

Device buffers are passed as plain integer addresses (e.g. ``torch.Tensor.data_ptr()``) and streams as
``hipStream_t`` integers; no torch type crosses the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import scene

HOST_ONLY = -1  # FMGI_HOST_ONLY: a context without a device (scene checks and planning only)
from ._lib import (ACCUM_AUTO, ACCUM_FX3, ACCUM_NONE, ACCUM_STATE, ACCUM_STREAM, KERNEL_AUTO, KERNEL_EXACT, KERNEL_FAST, KERNEL_GRID, KERNEL_HYBRID, RadStats, Timing, FmgiError, Geometry, Stats,
                   COLOUR_STATE_COUNT, RECOLOUR_MAX_SCENARIOS, Palette, FILTER_MAX_MAPS, FILTER_MAX_RADIUS,
                   SPARSE_COUNT_BITS, SparseInfo, BakeSparseStats,
                   VIEW_BILINEAR, VIEW_CACHE_MAX_SETS, VIEW_MAX_SAMPLES, VIEW_NEAREST, ViewCacheInfo, ViewGlossStats, ViewStats, check,
                   PROJ_EQUIRECT, PROJ_ORTHO, PROJ_PINHOLE,
                   RAD_CACHE_MAX_ITERATIONS, RAD_CACHE_MAX_SETS, RadCacheInfo,
                   SUN_ALL, SUN_BOUNCE_MAX_DIRS, SUN_LISTS, SUN_MAX_BOUNCES, SUN_MAX_MAPS, SUN_MAX_SAMPLES, SunStats,
                   load)
from .scene import RECT_DTYPE, Scene

LAUNCH_DTYPE = np.dtype(
    [("item_begin", "<u8"), ("count", "<u4"), ("rng_offset", "<i4"), ("source", "<i4"), ("is_window", "<i4")]
)
assert LAUNCH_DTYPE.itemsize == 24
EVENT_DTYPE = np.dtype(
    [("photon", "<i4"), ("depth", "<i4"), ("rect", "<i4"), ("texel", "<i4"), ("rgb", "<f4", 3), ("rng", "<u4")]
)
assert EVENT_DTYPE.itemsize == 32
EVENTS_PER_ITEM = 800
FX_SHIFT = 25

__all__ = [
    "Context",
    "bake_geometry",
    "plan_count",
    "scene",
    "Scene",
    "FmgiError",
    "KERNEL_EXACT",
    "KERNEL_FAST",
    "KERNEL_GRID",
    "KERNEL_AUTO",
    "ACCUM_AUTO",
    "ACCUM_FX3",
    "ACCUM_STATE",
    "ACCUM_STREAM",
    "LAUNCH_DTYPE",
    "EVENT_DTYPE",
    "device_count",
    "host_sincosf",
    "CAMERA_DTYPE",
    "camera",
    "render_views",
    "shade_views",
    "view_candidates",
    "view_stats",
    "view_gloss_stats",
    "ViewCache",
    "view_cache_bytes",
    "VIEW_CACHE_MAX_SETS",
    "PROJECTIONS",
    "RadCache",
    "rad_cache_bytes",
    "rad_reference_emit",
    "RAD_CACHE_MAX_SETS",
    "RAD_CACHE_MAX_ITERATIONS",
    "Palette",
    "palette_table",
    "states_bytes",
    "COLOUR_STATE_COUNT",
    "RECOLOUR_MAX_SCENARIOS",
    "FILTER_MAX_RADIUS",
    "FILTER_MAX_MAPS",
    "filter_energy",
    "filter_lightmap",
    "SparseInfo",
    "SPARSE_COUNT_BITS",
    "BAKE_FORMAT",
    "sparse_bytes",
    "sparse_check",
    "scene_hash",
    "save_bake",
    "load_bake",
    "sun_vector",
    "SUN_LISTS",
    "SUN_ALL",
    "SUN_MAX_SAMPLES",
    "SUN_MAX_MAPS",
    "SUN_BOUNCE_MAX_DIRS",
    "SUN_MAX_BOUNCES",
]


UNIT_SQRT = 0       # fmgi_device_unit ops (include/flatmatch_gi.h)
UNIT_TRUNC_DIV = 1
UNIT_TRUNC_DIV_INV = 2


def _ptr(a: np.ndarray | None):
    if a is None or len(a) == 0:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    return int(load().fmgi_device_count())


def host_sincosf(x):
    """Host fmgi_sincosf over an array (bit-identical to the device sampler's sin/cos)."""
    x = np.ascontiguousarray(np.atleast_1d(x), np.float32)
    s = np.empty_like(x)
    c = np.empty_like(x)
    load().fmgi_host_sincosf(_ptr(x), _ptr(s), _ptr(c), len(x))
    return s, c


def sun_vector(azimuth_deg: float, elevation_deg: float) -> np.ndarray:
    """The to_sun vector of a compass azimuth (degrees clockwise from north, +y is north, +x east) and an elevation
    above the horizon (degrees): float32 (sin az * cos el, cos az * cos el, sin el). The sun calls normalise it, so
    its float32 rounding only moves the direction by an ulp."""
    az, el = np.radians(float(azimuth_deg)), np.radians(float(elevation_deg))
    return np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)], np.float32)


_SUN_MODES = {"lists": SUN_LISTS, "all": SUN_ALL}


def palette_table(p: Palette) -> np.ndarray:
    """fmgi_palette_table: the deposit of every colour state under palette p, int64 [1024, 3] in units of
    2^-25 (host only). Raises FmgiError for a palette outside the ranges."""
    out = np.zeros((COLOUR_STATE_COUNT, 3), np.int64)
    check(load().fmgi_palette_table(C.byref(p), _ptr(out)), "fmgi_palette_table")
    return out


def states_bytes(num_texels: int) -> int:
    """Bytes of one histogram, uint64 [1024][num_texels] (fmgi_states_bytes)."""
    return int(load().fmgi_states_bytes(int(num_texels)))


def sparse_bytes(num_texels: int, rows: int) -> int:
    """Bytes of a sparse histogram blob of num_texels texels and `rows` rows (fmgi_sparse_bytes; 0 if
    num_texels < 1)."""
    return int(load().fmgi_sparse_bytes(int(num_texels), int(rows)))


def sparse_check(blob, num_texels: int) -> SparseInfo:
    """fmgi_sparse_check: validate a host copy of a sparse histogram blob (bytes, or an array whose bytes are
    the blob) of num_texels texels; returns its SparseInfo. Raises FmgiError naming the first violation."""
    raw = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview))
                               else np.asarray(blob)).view(np.uint8).reshape(-1)
    info = SparseInfo()
    buf = raw if len(raw) else np.zeros(1, np.uint8)
    check(load().fmgi_sparse_check(buf.ctypes.data_as(C.c_void_p), len(raw), int(num_texels), C.byref(info)),
          "fmgi_sparse_check")
    return info


BAKE_FORMAT = "fmgi-bake-1"


def scene_hash(sc: Scene) -> str:
    """SHA-256 (hex) over the scene's walls, windows and lights bytes and its texel count: what a saved bake is
    tied to."""
    import hashlib

    h = hashlib.sha256()
    for a in (sc.walls, sc.windows, sc.lights):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.int64(sc.num_texels).tobytes())
    return h.hexdigest()


def save_bake(path, sc: Scene, spa: int, wg: int, launches: np.ndarray, groups):
    """Write a traced scene as one .npz: the format tag, the scene's hash, spa, wg, the plan's launches
    (Context.get_plan()) and per group its label, item range, is_window, rows and sparse blob. groups: a list of
    (label, item_begin, item_end, is_window, blob) with blob a uint64 array (a host copy of the device blob). Every
    blob is checked (sparse_check) before anything is written."""
    launches = np.ascontiguousarray(launches, LAUNCH_DTYPE)
    out = {"format": np.array(BAKE_FORMAT), "scene_sha256": np.array(scene_hash(sc)),
           "num_texels": np.int64(sc.num_texels), "spa": np.int64(spa), "wg": np.int64(wg),
           "launches": launches.view(np.uint8).reshape(-1).copy(),
           "labels": np.array([str(g[0]) for g in groups], dtype=np.str_),
           "ranges": np.array([[int(g[1]), int(g[2])] for g in groups], np.uint64).reshape(len(groups), 2),
           "is_window": np.array([bool(g[3]) for g in groups], np.uint8)}
    rows = []
    for i, g in enumerate(groups):
        blob = np.ascontiguousarray(g[4], np.uint64).reshape(-1)
        rows.append(sparse_check(blob, sc.num_texels).rows)
        out[f"blob_{i}"] = blob
    out["rows"] = np.array(rows, np.uint64)
    with open(path, "wb") as f:
        np.savez(f, **out)


def load_bake(path, sc: Scene | None = None) -> dict:
    """Read a save_bake file (allow_pickle=False). Returns {"spa", "wg", "num_texels", "scene_sha256", "launches"
    (LAUNCH_DTYPE), "groups": [{"label", "item_begin", "item_end", "is_window", "rows", "info" (SparseInfo),
    "blob" (uint64)}]}. Every blob passes sparse_check. ValueError for a wrong format tag, a scene hash that
    differs from `sc`'s (when sc is given) or a blob that fails its check."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or str(z["format"]) != BAKE_FORMAT:
            tag = str(z["format"]) if "format" in z.files else None
            raise ValueError(f"{path}: format tag {tag!r}, not {BAKE_FORMAT!r}")
        d = {k: z[k] for k in z.files}
    sha, T = str(d["scene_sha256"]), int(d["num_texels"])
    if sc is not None and (sha != scene_hash(sc) or T != sc.num_texels):
        raise ValueError(f"{path}: baked for another scene (file {sha[:12]}..., {T} texels; scene {sc.name!r} "
                         f"{scene_hash(sc)[:12]}..., {sc.num_texels} texels)")
    launches = np.ascontiguousarray(d["launches"], np.uint8)
    if len(launches) % LAUNCH_DTYPE.itemsize:
        raise ValueError(f"{path}: {len(launches)} bytes of launches are no whole number of launches")
    groups = []
    for i, label in enumerate(d["labels"].tolist()):
        blob = np.ascontiguousarray(d[f"blob_{i}"], np.uint64).reshape(-1)
        try:
            info = sparse_check(blob, T)
        except FmgiError as e:
            raise ValueError(f"{path}: group {label!r}: {e}") from None
        if info.rows != int(d["rows"][i]):
            raise ValueError(f"{path}: group {label!r}: {info.rows} rows in the blob, {int(d['rows'][i])} recorded")
        groups.append({"label": str(label), "item_begin": int(d["ranges"][i][0]), "item_end": int(d["ranges"][i][1]),
                       "is_window": bool(d["is_window"][i]), "rows": int(info.rows), "info": info, "blob": blob})
    return {"spa": int(d["spa"]), "wg": int(d["wg"]), "num_texels": T, "scene_sha256": sha,
            "launches": launches.view(LAUNCH_DTYPE).copy(), "groups": groups}


def filter_energy(deposits: int, palette: Palette | None = None) -> int:
    """fmgi_filter_energy: the min_energy that stands for `deposits` first-bounce window photons under `palette`
    (None: the reference's), in units of 2^-25, mod 2^64 (host only)."""
    if palette is not None:
        palette_table(palette)  # raises FmgiError for a palette outside the ranges
    p = None if palette is None else C.byref(palette)
    return int(load().fmgi_filter_energy(p, int(deposits) & ((1 << 64) - 1)))


def filter_lightmap(sc: Scene, lm_fx: np.ndarray, min_deposits: int, max_radius: int = 4,
                    guide: np.ndarray | None = None, device: int = 0):
    """The adaptive density filter on host arrays (fmgi_filter_radii + fmgi_filter_apply on `device`): lm_fx is an
    int64 lightmap [numTexels, 3 or 4]; the radii come from `guide` (default: lm_fx itself) at min_energy =
    filter_energy(min_deposits). Returns (out, radii): out like lm_fx, radii uint8 [numTexels]."""
    import torch

    def four(a, what):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[0] != sc.num_texels or a.shape[1] not in (3, 4) or a.dtype != np.int64:
            raise FmgiError(f"filter_lightmap: {what} {a.shape} {a.dtype}, need int64 [{sc.num_texels}, 3 or 4]")
        out = np.zeros((sc.num_texels, 4), np.int64)
        out[:, : a.shape[1]] = a
        return out

    lm = four(lm_fx, "lm_fx")
    g = lm if guide is None else four(guide, "guide")
    dev = f"cuda:{device}"
    ctx = Context(device)
    try:
        ctx.set_scene(sc)
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            d_guide, d_lm = torch.from_numpy(g).to(dev), torch.from_numpy(lm).to(dev)
            d_radii = torch.zeros(sc.num_texels, dtype=torch.uint8, device=dev)
            ctx.filter_radii(d_guide.data_ptr(), filter_energy(min_deposits), max_radius, d_radii.data_ptr(),
                             s.cuda_stream)
            ctx.filter_apply(d_radii.data_ptr(), [d_lm.data_ptr()], [d_lm.data_ptr()], s.cuda_stream)
        s.synchronize()
        out, radii = d_lm.cpu().numpy()[:, : np.shape(lm_fx)[1]], d_radii.cpu().numpy()
    finally:
        ctx.close()
    return out, radii


def plan_count(sc: Scene, spa: int, wg: int = 256):
    """(launches, work items) of the reference schedule, without consuming rand()."""
    tot = C.c_uint64()
    w = np.ascontiguousarray(sc.windows)
    l = np.ascontiguousarray(sc.lights)
    n = check(load().fmgi_plan_count(_ptr(w), len(w), _ptr(l), len(l), spa, wg, C.byref(tot)), "fmgi_plan_count")
    return int(n), int(tot.value)


class Context:
    """One device's baker state (fmgi_context)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.h = self.lib.fmgi_create(device)
        if not self.h:
            raise FmgiError(f"fmgi_create({device}): {self.lib.fmgi_last_error().decode()}")
        self.device = device
        self.scene: Scene | None = None
        self.total_items = 0
        self.nlaunches = 0

    def close(self):
        if self.h:
            self.lib.fmgi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, sc: Scene):
        self._keep = [np.ascontiguousarray(a) for a in (sc.walls, sc.windows, sc.lights)]
        w, win, li = self._keep
        check(
            self.lib.fmgi_set_scene(self.h, _ptr(w), len(w), _ptr(win), len(win), _ptr(li), len(li), sc.num_texels),
            "fmgi_set_scene",
        )
        self.scene = sc

    def set_accumulation(self, mode: int):
        """ACCUM_FX3 (3 int64 atomics per deposit), ACCUM_STATE (1 u32 counter per colour state and
        texel) or ACCUM_AUTO. Both modes give identical bits."""
        check(self.lib.fmgi_set_accumulation(self.h, mode), "fmgi_set_accumulation")

    @property
    def accumulation(self) -> int:
        return int(self.lib.fmgi_get_accumulation(self.h))

    def plan(self, spa: int, wg: int = 256, rng_offsets=None) -> int:
        """Reference launch schedule. rng_offsets=None consumes libc rand() like the reference."""
        tot = C.c_uint64()
        offs = None if rng_offsets is None else np.ascontiguousarray(rng_offsets, np.int32)
        n = check(
            self.lib.fmgi_plan(self.h, spa, wg, _ptr(offs), 0 if offs is None else len(offs), C.byref(tot)),
            "fmgi_plan",
        )
        self.total_items = int(tot.value)
        self.nlaunches = int(n)
        return self.total_items

    def get_plan(self) -> np.ndarray:
        out = np.zeros(self.nlaunches, LAUNCH_DTYPE)
        check(self.lib.fmgi_get_plan(self.h, _ptr(out), len(out)), "fmgi_get_plan")
        return out

    def bake_items(self, begin: int, end: int, lm_fx_ptr: int, kernel: int = KERNEL_AUTO, stream: int = 0):
        """Launch on `stream` (a hipStream_t as int; pass the stream that produced lm_fx). 0/None selects
        the context's internal stream, which is NOT ordered with torch's default stream."""
        check(self.lib.fmgi_bake_items(self.h, begin, end, C.c_void_p(lm_fx_ptr), kernel, C.c_void_p(stream or None)),
              "fmgi_bake_items")

    def bake_states(self, begin: int, end: int, counts_ptr: int, kernel: int = KERNEL_AUTO, stream: int = 0):
        """fmgi_bake_states: trace items [begin, end) like bake_items, counting every deposit in the device
        histogram uint64 [1024][num_texels] at counts_ptr (states_bytes(num_texels) bytes; counts add to what it
        holds). The context's accumulation mode is left as it is."""
        check(self.lib.fmgi_bake_states(self.h, begin, end, C.c_void_p(counts_ptr), kernel, C.c_void_p(stream or None)),
              "fmgi_bake_states")

    def recolour(self, counts_ptrs, palettes, lm_ptrs, stream: int = 0):
        """fmgi_recolour: lm[k] += the histograms counts_ptrs[g] folded with palettes[k][g], exactly, for every
        scenario k (palettes: one row of len(counts_ptrs) Palette objects per scenario; lm_ptrs: one device
        lightmap int64 [num_texels][4] per scenario). Asynchronous on `stream`."""
        G, K = len(counts_ptrs), len(lm_ptrs)
        if len(palettes) != K or any(len(row) != G for row in palettes):
            raise FmgiError(f"recolour: palettes must be {K} scenarios x {G} groups")
        cp = (C.c_void_p * max(G, 1))(*[C.c_void_p(int(p)) for p in counts_ptrs])
        lp = (C.c_void_p * max(K, 1))(*[C.c_void_p(int(p)) for p in lm_ptrs])
        pal = (Palette * max(K * G, 1))()
        for k, row in enumerate(palettes):
            for g, p in enumerate(row):
                C.memmove(C.byref(pal, (k * G + g) * C.sizeof(Palette)), C.byref(p), C.sizeof(Palette))
        check(self.lib.fmgi_recolour(self.h, cp, G, pal, K, lp, C.c_void_p(stream or None)), "fmgi_recolour")

    def sparse_measure(self, counts_ptr: int, stream: int = 0) -> SparseInfo:
        """fmgi_sparse_measure: one pass over the device histogram at counts_ptr; synchronises `stream` and returns
        its SparseInfo (rows sizes the blob: sparse_bytes(num_texels, info.rows)). Raises FmgiError if a count is
        2^54 or more."""
        info = SparseInfo()
        check(self.lib.fmgi_sparse_measure(self.h, C.c_void_p(counts_ptr or None), C.byref(info),
                                           C.c_void_p(stream or None)), "fmgi_sparse_measure")
        return info

    def sparse_compact(self, counts_ptr: int, info: SparseInfo, sparse_ptr: int, stream: int = 0):
        """fmgi_sparse_compact: the device histogram at counts_ptr into its sparse blob at sparse_ptr
        (sparse_bytes(num_texels, info.rows) bytes; info from sparse_measure). Asynchronous on `stream`."""
        check(self.lib.fmgi_sparse_compact(self.h, C.c_void_p(counts_ptr or None), C.byref(info),
                                           C.c_void_p(sparse_ptr or None), C.c_void_p(stream or None)),
              "fmgi_sparse_compact")

    def sparse_expand(self, sparse_ptr: int, info: SparseInfo, counts_ptr: int, stream: int = 0):
        """fmgi_sparse_expand: adds the blob at sparse_ptr to the device histogram uint64 [1024][num_texels] at
        counts_ptr. Asynchronous on `stream`."""
        check(self.lib.fmgi_sparse_expand(self.h, C.c_void_p(sparse_ptr or None), C.byref(info),
                                          C.c_void_p(counts_ptr or None), C.c_void_p(stream or None)),
              "fmgi_sparse_expand")

    def recolour_sparse(self, sparse_ptrs, infos, palettes, lm_ptrs, stream: int = 0):
        """fmgi_recolour_sparse: recolour() on sparse blobs: lm[k] += the blobs sparse_ptrs[g] (with infos[g])
        folded with palettes[k][g], exactly. Asynchronous on `stream`."""
        G, K = len(sparse_ptrs), len(lm_ptrs)
        if len(infos) != G:
            raise FmgiError(f"recolour_sparse: {G} blobs, {len(infos)} infos")
        if len(palettes) != K or any(len(row) != G for row in palettes):
            raise FmgiError(f"recolour_sparse: palettes must be {K} scenarios x {G} groups")
        sp = (C.c_void_p * max(G, 1))(*[C.c_void_p(int(p)) for p in sparse_ptrs])
        lp = (C.c_void_p * max(K, 1))(*[C.c_void_p(int(p)) for p in lm_ptrs])
        inf = (SparseInfo * max(G, 1))()
        for g, i in enumerate(infos):
            C.memmove(C.byref(inf, g * C.sizeof(SparseInfo)), C.byref(i), C.sizeof(SparseInfo))
        pal = (Palette * max(K * G, 1))()
        for k, row in enumerate(palettes):
            for g, p in enumerate(row):
                C.memmove(C.byref(pal, (k * G + g) * C.sizeof(Palette)), C.byref(p), C.sizeof(Palette))
        check(self.lib.fmgi_recolour_sparse(self.h, sp, inf, G, pal, K, lp, C.c_void_p(stream or None)),
              "fmgi_recolour_sparse")

    def bake_sparse_supported(self) -> bool:
        """fmgi_bake_sparse_supported: whether bake_sparse / sparse_from_codes can serve the current scene (its
        STREAM layout is the per-tile bucket layout: at most 63 tiles of 2048 texels)."""
        return bool(check(self.lib.fmgi_bake_sparse_supported(self.h), "fmgi_bake_sparse_supported"))

    def bake_sparse(self, begin: int, end: int, kernel: int = KERNEL_AUTO, stream: int = 0) -> SparseInfo:
        """fmgi_bake_sparse: bake_items' trace of work items [begin, end) through the STREAM bucket path, its deposit
        codes counted into the sparse histogram of exactly these items (no dense histogram). The result is held in
        the context (bake_sparse_take); returns its SparseInfo. Synchronises `stream`."""
        info = SparseInfo()
        check(self.lib.fmgi_bake_sparse(self.h, int(begin), int(end), int(kernel), C.byref(info),
                                        C.c_void_p(stream or None)), "fmgi_bake_sparse")
        return info

    def bake_sparse_take(self, info: SparseInfo, sparse_ptr: int, stream: int = 0):
        """fmgi_bake_sparse_take: the held histogram's blob (sparse_bytes(num_texels, info.rows) bytes) to sparse_ptr;
        the context then holds nothing. Asynchronous on `stream`."""
        check(self.lib.fmgi_bake_sparse_take(self.h, C.byref(info), C.c_void_p(sparse_ptr or None),
                                             C.c_void_p(stream or None)), "fmgi_bake_sparse_take")

    def sparse_from_codes(self, codes_ptr: int, n: int, stream: int = 0):
        """fmgi_sparse_from_codes: the histogram of the n device codes (uint32: texel << 10 | state, any order) at
        codes_ptr as a held result (bake_sparse_take). Returns (SparseInfo, skipped): skipped counts the codes
        whose texel is outside the scene; codes of 0xFFFFFFFF are pads. Synchronises."""
        info, skipped = SparseInfo(), C.c_uint64(0)
        check(self.lib.fmgi_sparse_from_codes(self.h, C.c_void_p(codes_ptr or None), int(n), C.byref(info),
                                              C.byref(skipped), C.c_void_p(stream or None)), "fmgi_sparse_from_codes")
        return info, int(skipped.value)

    def sparse_add_measure(self, a_ptr: int, a_info: SparseInfo, b_ptr: int, b_info: SparseInfo,
                           stream: int = 0) -> SparseInfo:
        """fmgi_sparse_add_measure: the SparseInfo of a + b (device blobs); synchronises. Raises FmgiError if a
        summed count reaches 2^54."""
        info = SparseInfo()
        check(self.lib.fmgi_sparse_add_measure(self.h, C.c_void_p(a_ptr or None), C.byref(a_info),
                                               C.c_void_p(b_ptr or None), C.byref(b_info), C.byref(info),
                                               C.c_void_p(stream or None)), "fmgi_sparse_add_measure")
        return info

    def sparse_add(self, a_ptr: int, a_info: SparseInfo, b_ptr: int, b_info: SparseInfo, sum_info: SparseInfo,
                   sum_ptr: int, stream: int = 0):
        """fmgi_sparse_add: the canonical blob of a + b (sparse_bytes(num_texels, sum_info.rows) bytes; sum_info
        from sparse_add_measure) to sum_ptr, which must not alias an input. Asynchronous on `stream`."""
        check(self.lib.fmgi_sparse_add(self.h, C.c_void_p(a_ptr or None), C.byref(a_info), C.c_void_p(b_ptr or None),
                                       C.byref(b_info), C.byref(sum_info), C.c_void_p(sum_ptr or None),
                                       C.c_void_p(stream or None)), "fmgi_sparse_add")

    def bake_sparse_stats(self) -> dict:
        """fmgi_bake_sparse_get_stats: chunks, merges, dense_chunks, codes and scratch_bytes of the context's last
        bake_sparse / sparse_from_codes."""
        st = BakeSparseStats()
        check(self.lib.fmgi_bake_sparse_get_stats(self.h, C.byref(st)), "fmgi_bake_sparse_get_stats")
        return {k: int(getattr(st, k)) for k, _ in st._fields_}

    def filter_radii(self, guide_ptr: int, min_energy: int, max_radius: int, radii_ptr: int, stream: int = 0):
        """fmgi_filter_radii: per level-0 texel the smallest window radius in [0, max_radius] that holds
        min_energy (unsigned, units of 2^-25; see filter_energy) of the device guide lightmap int64
        [num_texels][4] at guide_ptr, into the device array uint8 [num_texels] at radii_ptr. Asynchronous on
        `stream`."""
        check(self.lib.fmgi_filter_radii(self.h, C.c_void_p(guide_ptr or None), int(min_energy) & ((1 << 64) - 1),
                                         int(max_radius), C.c_void_p(radii_ptr or None), C.c_void_p(stream or None)),
              "fmgi_filter_radii")

    def filter_apply(self, radii_ptr: int, in_ptrs, out_ptrs, stream: int = 0):
        """fmgi_filter_apply: out_ptrs[k] = the device lightmap in_ptrs[k] (int64 [num_texels][4]) averaged over
        every level-0 texel's window of the radii at radii_ptr, exactly; out_ptrs[k] may be in_ptrs[k].
        Asynchronous on `stream`."""
        K = len(in_ptrs)
        if len(out_ptrs) != K:
            raise FmgiError(f"filter_apply: {K} inputs, {len(out_ptrs)} outputs")
        ip = (C.c_void_p * max(K, 1))(*[C.c_void_p(int(p) or None) for p in in_ptrs])
        op = (C.c_void_p * max(K, 1))(*[C.c_void_p(int(p) or None) for p in out_ptrs])
        check(self.lib.fmgi_filter_apply(self.h, C.c_void_p(radii_ptr or None), ip, op, K, C.c_void_p(stream or None)),
              "fmgi_filter_apply")

    def sun_coverage(self, to_sun, samples: int, cover_ptr: int, mode: str = "lists", stream: int = 0):
        """fmgi_sun_coverage: per level-0 texel of every wall that faces the sun, how many of its
        samples x samples shadow rays towards to_sun (any non-zero length) leave through a window before they meet a
        wall, into the device array uint8 [num_texels] at cover_ptr; every other byte 0. mode "lists" (per-window
        occluder lists, the product path) or "all" (every wall that faces away from the sun): the same bytes.
        Asynchronous on `stream`."""
        if mode not in _SUN_MODES:
            raise FmgiError(f"mode {mode!r}: one of {sorted(_SUN_MODES)}")
        v = (C.c_float * 3)(*[float(x) for x in to_sun])
        check(self.lib.fmgi_sun_coverage(self.h, v, int(samples), _SUN_MODES[mode], C.c_void_p(cover_ptr or None),
                                         C.c_void_p(stream or None)), "fmgi_sun_coverage")

    def sun_add(self, cover_ptr: int, to_sun, samples: int, rgb, flux: float, lm_ptrs, stream: int = 0):
        """fmgi_sun_add: adds the sun of colour rgb[k] (palette units; window_rgb is 18) and `flux` photons per m²
        (the bake's spa) through the coverage map at cover_ptr (made with the same to_sun and samples) to the device
        lightmap int64 [num_texels][4] at lm_ptrs[k], in place. rgb is [K][3], or one colour for one map.
        Asynchronous on `stream`."""
        rgb = np.ascontiguousarray(np.atleast_2d(np.asarray(rgb, np.float32)))
        K = len(lm_ptrs)
        if rgb.shape != (K, 3):
            raise FmgiError(f"sun_add: {K} lightmaps, rgb of shape {rgb.shape}")
        v = (C.c_float * 3)(*[float(x) for x in to_sun])
        lp = (C.c_void_p * max(K, 1))(*[C.c_void_p(int(p) or None) for p in lm_ptrs])
        check(self.lib.fmgi_sun_add(self.h, C.c_void_p(cover_ptr or None), v, int(samples), _ptr(rgb), K, float(flux),
                                    lp, C.c_void_p(stream or None)), "fmgi_sun_add")

    def sun_add_bounced(self, bounce_ptr: int, bounces: int, rgb, refl, flux: float, lm_ptrs, stream: int = 0):
        """fmgi_sun_add_bounced: adds the sun's bounced light, the device table float32
        [bounces][num_texels] of one direction at bounce_ptr (RadCache.sun_bounce), under colour rgb[k] and
        reflectance refl[k] per channel to the device lightmap int64 [num_texels][4] at lm_ptrs[k], in place: bounce n
        weighs refl ** n. rgb and refl are [K][3], or one triple for one map; flux is the bake's spa.
        Asynchronous on `stream`."""
        rgb = np.ascontiguousarray(np.atleast_2d(np.asarray(rgb, np.float32)))
        refl = np.ascontiguousarray(np.atleast_2d(np.asarray(refl, np.float32)))
        K = len(lm_ptrs)
        if rgb.shape != (K, 3) or refl.shape != (K, 3):
            raise FmgiError(f"sun_add_bounced: {K} lightmaps, rgb of shape {rgb.shape}, refl of shape {refl.shape}")
        lp = (C.c_void_p * max(K, 1))(*[C.c_void_p(int(p) or None) for p in lm_ptrs])
        check(self.lib.fmgi_sun_add_bounced(self.h, C.c_void_p(bounce_ptr or None), int(bounces), _ptr(rgb), _ptr(refl), K,
                                            float(flux), lp, C.c_void_p(stream or None)), "fmgi_sun_add_bounced")

    def sun_stats(self) -> dict:
        """fmgi_sun_get_stats of the context's last sun_coverage (synchronises): samples, facing, crossing, lit,
        list_entries, tests, list_ms, rays_ms."""
        st = SunStats()
        check(self.lib.fmgi_sun_get_stats(self.h, C.byref(st)), "fmgi_sun_get_stats")
        return st.as_dict()

    def sun_units(self, to_sun, rgb, flux: float) -> np.ndarray:
        """fmgi_sun_units (host only): int64 [numWalls][3], what one fully lit texel of every wall gains in units of
        2^-25; zero rows for the walls that do not face the sun."""
        v = (C.c_float * 3)(*[float(x) for x in to_sun])
        c = (C.c_float * 3)(*[float(x) for x in rgb])
        out = np.zeros((len(self.scene.walls) if self.scene is not None else 0, 3), np.int64)
        check(self.lib.fmgi_sun_units(self.h, v, c, float(flux), out.ctypes.data_as(C.c_void_p)), "fmgi_sun_units")
        return out

    def source_ranges(self):
        """One (source, is_window, item_begin, item_end) per emitter of the planned schedule, windows first: the
        item ranges that cut a bake into per-source histograms (bake_states)."""
        out = []
        for L in self.get_plan():
            b, e = int(L["item_begin"]), int(L["item_begin"]) + int(L["count"])
            src, win = int(L["source"]), int(L["is_window"])
            if out and out[-1][0] == src:
                assert out[-1][3] == b, f"source {src}: launches not contiguous"
                out[-1] = (src, win, out[-1][2], e)
            else:
                assert src not in [o[0] for o in out], f"source {src}: launches not contiguous"
                out.append((src, win, b, e))
        return out

    def finalize(self, lm_fx_ptr: int, texels_in_ptr: int, texels_out_ptr: int, stream: int = 0):
        check(
            self.lib.fmgi_finalize(self.h, C.c_void_p(lm_fx_ptr), C.c_void_p(texels_in_ptr), C.c_void_p(texels_out_ptr),
                                   C.c_void_p(stream or None)),
            "fmgi_finalize",
        )

    def stats(self) -> dict:
        st = Stats()
        check(self.lib.fmgi_get_stats(self.h, C.byref(st)), "fmgi_get_stats")
        return st.as_dict()

    def reset_stats(self):
        check(self.lib.fmgi_reset_stats(self.h), "fmgi_reset_stats")

    def trace_items(self, begin: int, end: int, kernel: int = KERNEL_AUTO):
        """Per-photon bounce records of items [begin, end): (events[n, 800], counts[n], rng_final[n])."""
        n = end - begin
        ev = np.zeros(n * EVENTS_PER_ITEM, EVENT_DTYPE)
        cnt = np.zeros(n, np.int32)
        rng = np.zeros(n, np.uint32)
        check(self.lib.fmgi_trace_items(self.h, begin, end, kernel, _ptr(ev), _ptr(cnt), _ptr(rng)), "fmgi_trace_items")
        return ev.reshape(n, EVENTS_PER_ITEM), cnt, rng

    @property
    def auto_kernel(self) -> int:
        return int(self.lib.fmgi_auto_kernel(self.h))

    @property
    def last_bake_kernel(self) -> str:
        """the profiler's name of the k_bake instance(s) the last bake launch ran (fmgi_last_bake_kernel)"""
        if not hasattr(self.lib, "fmgi_last_bake_kernel"):  # (FMGI_LIB=base: an A/B build that predates it)
            return ""
        n = int(self.lib.fmgi_last_bake_kernel(self.h, None, 0))
        buf = C.create_string_buffer(n + 1)
        self.lib.fmgi_last_bake_kernel(self.h, buf, n + 1)
        return buf.value.decode()

    def set_timing(self, on: bool = True):
        check(self.lib.fmgi_set_timing(self.h, 1 if on else 0), "fmgi_set_timing")

    def timing(self) -> dict:
        """Device time of the bake / fold launches since the previous call (needs set_timing(True))."""
        t = Timing()
        check(self.lib.fmgi_get_timing(self.h, C.byref(t)), "fmgi_get_timing")
        return t.as_dict()

    def set_option(self, name: str, value: int):
        """fmgi_set_option: one of _lib.OPTIONS (chunk_items, pool_limit, stream_layout, bucket_fill, wide_tiles,
        coop, no_axes, photon_lock, lattice, hist_batch); takes effect at the next bake (no_axes: the next set_scene)."""
        from ._lib import OPTIONS

        check(self.lib.fmgi_set_option(self.h, OPTIONS[name], int(value)), "fmgi_set_option")

    def set_grid_cells_per_record(self, n: int):
        """The grid's cells per record for the next set_scene (0: the product's choice)."""
        check(self.lib.fmgi_set_grid_cells_per_record(self.h, int(n)), "fmgi_set_grid_cells_per_record")

    def grid_tables(self) -> dict:
        """FMGI_KERNEL_GRID's plane/cell/record tables (include/flatmatch_gi.h fmgi_grid_copy)."""
        sz = np.zeros(5, np.int32)
        check(self.lib.fmgi_grid_sizes(self.h, _ptr(sz)), "fmgi_grid_sizes")
        npairs = int(sz[:3].sum())
        planes = np.zeros(2 * max(npairs, 1), GRID_PLANE_DTYPE)
        cells = np.zeros(int(sz[3]), GRID_CELL_DTYPE)
        recs = np.zeros((int(sz[4]), 4), np.float32)
        idx = np.zeros(int(sz[4]), np.int32)
        check(self.lib.fmgi_grid_copy(self.h, _ptr(planes), _ptr(cells), _ptr(recs), _ptr(idx)), "fmgi_grid_copy")
        return {"J": [int(x) for x in sz[:3]], "planes": planes[: 2 * npairs], "cells": cells, "recs": recs,
                "idx": idx}

    def lattice_tables(self) -> dict:
        """The closed box's lattice descriptors (include/flatmatch_gi.h fmgi_lattice_copy): {"lattice": [6]
        records of LATTICE_DTYPE, per axis {+n plane, -n plane}}, empty when the scene has no verified lattice."""
        n = check(self.lib.fmgi_lattice_copy(self.h, None), "fmgi_lattice_copy")
        desc = np.zeros(n, LATTICE_DTYPE)
        if n:
            check(self.lib.fmgi_lattice_copy(self.h, _ptr(desc)), "fmgi_lattice_copy")
        return {"lattice": desc}

    def plan_tables(self) -> dict | None:
        """FMGI_KERNEL_HYBRID's floor plan of the walls (include/flatmatch_gi.h fmgi_plan_copy), or None."""
        n = C.c_int32(0)
        check(self.lib.fmgi_plan_copy(self.h, None, C.byref(n)), "fmgi_plan_copy")
        if n.value == 0:
            return None
        blob = np.zeros(n.value, np.uint8)
        check(self.lib.fmgi_plan_copy(self.h, _ptr(blob), C.byref(n)), "fmgi_plan_copy")
        h0 = blob[:16].view(np.float32)
        h1 = blob[16:32].view(np.int32)
        ncells, nent = int(h1[1]), int(h1[2])
        u16 = blob[32:].view(np.uint16)
        return {"x0": h0[0], "y0": h0[1], "ics": h0[2], "cs": h0[3], "nx": int(h1[0]) & 0xFFFF,
                "ny": int(h1[0]) >> 16, "start": u16[: ncells + 1].copy(),
                "entry": u16[ncells + 1 : ncells + 1 + nent].copy()}

    def filter_image(self) -> dict:
        """The filter image (include/flatmatch_gi.h fmgi_filter_copy): records [n, 8] as float32 (idx in
        column 5 as int32 bits) and the pairs per axis."""
        n = C.c_int32(0)
        J = np.zeros(3, np.int32)
        check(self.lib.fmgi_filter_copy(self.h, None, C.byref(n), _ptr(J)), "fmgi_filter_copy")
        img = np.zeros(n.value // 4, np.float32)
        check(self.lib.fmgi_filter_copy(self.h, _ptr(img), C.byref(n), _ptr(J)), "fmgi_filter_copy")
        recs = img.reshape(-1, 8)
        return {"J": [int(x) for x in J], "recs": recs, "idx": recs[:, 5].view(np.int32).copy()}

    def pair_image(self) -> dict:
        """The hybrid scan's wall-pair image (include/flatmatch_gi.h fmgi_pairs_copy): halves [n, 12] as
        float32 (the two rect indices in columns 10, 11 as int32 bits), two halves (+a, -a) per group, and the
        groups per axis (x, y)."""
        n = C.c_int32(0)
        G = np.zeros(2, np.int32)
        check(self.lib.fmgi_pairs_copy(self.h, None, C.byref(n), _ptr(G)), "fmgi_pairs_copy")
        img = np.zeros(n.value // 4, np.float32)
        check(self.lib.fmgi_pairs_copy(self.h, _ptr(img), C.byref(n), _ptr(G)), "fmgi_pairs_copy")
        halves = img.reshape(-1, 12)
        return {"G": [int(x) for x in G], "halves": halves, "idx": halves[:, 10:12].view(np.int32).copy()}

    def device_sincosf(self, x: np.ndarray, library: bool = False):
        """The samplers' sin/cos on the device (the restatement), or with library=True the device
        library's sinf/cosf that it restates."""
        x = np.ascontiguousarray(x, np.float32)
        s = np.empty_like(x)
        c = np.empty_like(x)
        fn = self.lib.fmgi_device_sincosf_library if library else self.lib.fmgi_device_sincosf
        check(fn(self.h, _ptr(x), _ptr(s), _ptr(c), len(x)), "fmgi_device_sincosf")
        return s, c

    def device_unit(self, op: int, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
        """The bake's device arithmetic helpers (include/flatmatch_gi.h fmgi_device_unit): op 0 = the
        sampler's sqrtf (returns float32), op 1 = (int)(a / b) of the tile index (returns int32)."""
        a = np.ascontiguousarray(a, np.float32)
        bb = None if b is None else np.ascontiguousarray(b, np.float32)
        out = np.empty(len(a), np.int32)
        check(self.lib.fmgi_device_unit(self.h, op, _ptr(a), None if bb is None else _ptr(bb), _ptr(out), len(a)),
              "fmgi_device_unit")
        return out.view(np.float32) if op == 0 else out


GRID_PLANE_DTYPE = np.dtype([("plane", "<f4"), ("u0", "<f4"), ("v0", "<f4"), ("iu", "<f4"), ("iv", "<f4"),
                             ("mu", "<f4"), ("mv", "<f4"), ("nu", "<i4"), ("nv", "<i4"), ("cell_off", "<i4"),
                             ("ulo", "<f4"), ("uhi", "<f4"), ("vlo", "<f4"), ("vhi", "<f4"),
                             ("pad0", "<f4"), ("pad1", "<f4")])
assert GRID_PLANE_DTYPE.itemsize == 64
GRID_CELL_DTYPE = np.dtype([("q0", "<u4", (2,)), ("q1", "<u4", (2,)), ("count", "<i4"), ("idx0", "<i4"),
                            ("idx1", "<i4"), ("rest", "<i4")])
assert GRID_CELL_DTYPE.itemsize == 32
LATTICE_DTYPE = np.dtype([("u0", "<f4"), ("iu", "<f4"), ("mu", "<f4"), ("lo_u", "<f4"),
                          ("v0", "<f4"), ("iv", "<f4"), ("mv", "<f4"), ("lo_v", "<f4"),
                          ("hi_u", "<f4"), ("hi_v", "<f4"), ("base", "<i4"), ("su", "<i4"),
                          ("sv", "<i4"), ("nu", "<i4"), ("nv", "<i4"), ("pad", "<i4")])
assert LATTICE_DTYPE.itemsize == 64


def make_geometry(sc: Scene, texels: np.ndarray):
    """A reference Geometry struct pointing at numpy arrays (kept alive by the returned tuple)."""
    keep = [np.ascontiguousarray(a) for a in (sc.windows, sc.lights, sc.walls)]
    g = Geometry()
    g.windows, g.lights, g.walls = (a.ctypes.data if len(a) else None for a in keep)
    g.boxWalls = None
    g.numWindows, g.numLights, g.numWalls = len(keep[0]), len(keep[1]), len(keep[2])
    g.numBoxWalls = 0
    g.numTexels = sc.num_texels
    g.texels = texels.ctypes.data
    return g, keep


def experiments() -> bool:
    """Whether the loaded library is the experiment build (reads the experiment knobs)."""
    return bool(load().fmgi_experiments())


def dropin_release():
    """Free the device state the drop-in entry points cache across calls (fmgi_dropin_release)."""
    load().fmgi_dropin_release()


def dropin_rccl_ranks() -> int:
    """Ranks of the RCCL communicator the last drop-in call reduced over (0: reduced without RCCL)."""
    return int(load().fmgi_dropin_rccl_ranks())


def dropin_shards(items: int, ngpu: int, nshard: int):
    """The drop-in's multi-GPU layout: (device, begin, end) per shard (fmgi_dropin_shards)."""
    dev = np.zeros(nshard, np.int32)
    b = np.zeros(nshard, np.uint64)
    e = np.zeros(nshard, np.uint64)
    check(load().fmgi_dropin_shards(items, ngpu, nshard, _ptr(dev), _ptr(b), _ptr(e)), "fmgi_dropin_shards")
    return dev, b, e


def dropin_reduce_order(nshard: int):
    """The drop-in's shard reduction: (dst, src) pairs in execution order (fmgi_dropin_reduce_order)."""
    dst = np.zeros(max(nshard, 1), np.int32)
    src = np.zeros(max(nshard, 1), np.int32)
    n = check(load().fmgi_dropin_reduce_order(nshard, _ptr(dst), _ptr(src)), "fmgi_dropin_reduce_order")
    return dst[:n], src[:n]


def bake_geometry(sc: Scene, spa: int, texels: np.ndarray | None = None) -> np.ndarray:
    """getGlobalIlluminationCl: bake on host arrays; consumes libc rand() like the reference."""
    tin = sc.texels() if texels is None else np.ascontiguousarray(texels, np.float32)
    out = np.empty_like(tin)
    g, keep = make_geometry(sc, tin)
    check(load().getGlobalIlluminationCl(C.byref(g), spa, out.ctypes.data_as(C.c_void_p)), "getGlobalIlluminationCl")
    del keep
    return out


# ---- ambient occlusion (include/flatmatch_gi.h) ----------------------------------

def ambient_occlusion(sc: Scene, wall_begin: int = 0, wall_end: int | None = None,
                      texels: np.ndarray | None = None) -> np.ndarray:
    """The reference's performAmbientOcclusionNative on the GPU (fmgi_ambient_occlusion): returns
    float32 [numTexels, 4] = `texels` (default zeros) with the level-0 texels of walls
    [wall_begin, wall_end) replaced by (d, d, d, 0)."""
    lib = load()
    tex = np.zeros((sc.num_texels, 4), np.float32) if texels is None else np.ascontiguousarray(texels, np.float32)
    out = np.empty_like(tex)
    g, keep = make_geometry(sc, tex)
    we = len(sc.walls) if wall_end is None else wall_end
    check(lib.fmgi_ambient_occlusion(C.byref(g), wall_begin, we, _ptr(out)), "fmgi_ambient_occlusion")
    return out


def radiosity(sc: Scene, with_sids: bool = False):
    """The reference's performRadiosityNative on the GPU (fmgi_radiosity): returns float32 [numTexels, 4]
    texels, and with with_sids also the int32 [jobs, 10000] sourceTexelIds rows of the level-0 wall
    texels. Consumes the process's libc rand() stream exactly as the reference does."""
    lib = load()
    tex = np.zeros((sc.num_texels, 4), np.float32)
    out = np.empty_like(tex)
    g, keep = make_geometry(sc, tex)
    jobs = int(lib.fmgi_radiosity_jobs(C.byref(g)))
    sids = np.zeros((jobs, 10000), np.int32) if with_sids else None
    check(lib.fmgi_radiosity(C.byref(g), _ptr(out), _ptr(sids) if with_sids else None), "fmgi_radiosity")
    return (out, sids) if with_sids else out


def radiosity_stats() -> dict:
    """fmgi_radiosity_stats: the last radiosity call's sizes and device phase times."""
    lib = load()
    st = RadStats()
    check(lib.fmgi_radiosity_stats(C.byref(st)), "fmgi_radiosity_stats")
    return st.as_dict()


# ---- radiosity scenarios (include/flatmatch_gi.h) ------------------------------------------

def rad_cache_bytes(sc: Scene) -> int:
    """fmgi_rad_cache_bytes: the device bytes a RadCache of the scene keeps (ids, jobs, rectangles)."""
    g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
    n = int(check(load().fmgi_rad_cache_bytes(C.byref(g)), "fmgi_rad_cache_bytes"))
    del keep
    return n


def rad_reference_emit(sc: Scene) -> np.ndarray:
    """fmgi_rad_reference_emit: the reference's palette, float32 [windows + lights, 3]: 30 for every window,
    (28, 28, 32) for every light."""
    g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
    emit = np.zeros((len(sc.windows) + len(sc.lights), 3), np.float32)
    check(load().fmgi_rad_reference_emit(C.byref(g), _ptr(emit)), "fmgi_rad_reference_emit")
    del keep
    return emit


class RadCache:
    """A radiosity cache (fmgi_rad_cache): radiosity()'s rays cast once from the current libc rand() position,
    their source texel ids kept on the device. solve() runs the bounces for any number of emitter palettes and
    leaves the texels on the device, where ViewCache.tiles reads them (spa = 0, tint_extra = 1)."""

    def __init__(self, sc: Scene):
        self.lib = load()
        self.h = None
        self.num_texels = sc.num_texels
        self.emitters = len(sc.windows) + len(sc.lights)
        g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
        h = C.c_void_p()
        check(self.lib.fmgi_rad_cache_create(C.byref(g), C.byref(h)), "fmgi_rad_cache_create")
        del keep
        self.h = h

    def close(self):
        if self.h:
            self.lib.fmgi_rad_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self) -> dict:
        """fmgi_rad_cache_info: jobs, rects, windows, lights, texels (the emitters' included), rays, bytes and the
        trace's rand_ms and rays_ms."""
        st = RadCacheInfo()
        check(self.lib.fmgi_rad_cache_info(self.h, C.byref(st)), "fmgi_rad_cache_info")
        return st.as_dict()

    def sids(self) -> np.ndarray:
        """fmgi_rad_cache_sids: int32 [jobs, 10000], radiosity(with_sids=True)'s rows."""
        out = np.zeros((self.info["jobs"], 10000), np.int32)
        check(self.lib.fmgi_rad_cache_sids(self.h, _ptr(out)), "fmgi_rad_cache_sids")
        return out

    def solve(self, emit, iterations: int = 7, stream=None):
        """fmgi_rad_cache_solve: emit float32 [K, windows + lights, 3] (one set may come as [emitters, 3]) ->
        a torch float32 device tensor [K, numTexels, 4]. Asynchronous on `stream`: a torch.cuda.Stream, a
        hipStream_t integer, or None for torch's current stream."""
        import os

        import torch

        emit = np.ascontiguousarray(emit, np.float32)
        if emit.ndim == 2:
            emit = emit[None]
        if emit.ndim != 3 or emit.shape[1:] != (self.emitters, 3):
            raise FmgiError(f"emit has shape {emit.shape}, the scene's palettes are [K, {self.emitters}, 3]")
        k = emit.shape[0]
        dev = torch.device("cuda", int(os.environ.get("FMGI_DEVICE", "0")))
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        out = torch.empty((k, self.num_texels, 4), dtype=torch.float32, device=dev)
        if isinstance(stream, int):
            handle = stream
        else:
            handle = stream.cuda_stream
            out.record_stream(stream)
        ptrs, n = _ptr_array(out[i].data_ptr() for i in range(k))
        check(self.lib.fmgi_rad_cache_solve(self.h, emit.ctypes.data_as(C.c_void_p), n, iterations, ptrs,
                                            C.c_void_p(handle or None)), "fmgi_rad_cache_solve")
        return out


    def sun_bounce(self, covers, to_suns, samples, bounces: int, stream=None):
        """fmgi_rad_cache_sun_bounce: covers are K coverage maps on the device (torch uint8 tensors of
        num_texels bytes, or addresses; Context.sun_coverage), to_suns float32 [K, 3] their directions, samples their
        samples per texel edge (one int for all, or K) -> a torch float32 device tensor [K, bounces, num_texels]: row
        n - 1 is g_n, the n-th bounce of a sun of unit colour on walls of unit reflectance. Asynchronous on `stream`:
        a torch.cuda.Stream, a hipStream_t integer, or None for torch's current stream."""
        import os

        import torch

        covers = list(covers)
        k = len(covers)
        to_suns = np.ascontiguousarray(np.asarray(to_suns, np.float32).reshape(-1, 3))
        samples = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, np.int32), (k,)))
        if to_suns.shape != (k, 3):
            raise FmgiError(f"sun_bounce: {k} coverage maps, to_suns of shape {to_suns.shape}")
        for c in covers:
            if hasattr(c, "data_ptr") and (c.dtype != torch.uint8 or c.numel() < self.num_texels or not c.is_contiguous()):
                raise FmgiError(f"sun_bounce: a coverage map is uint8 [{self.num_texels}], contiguous")
        dev = torch.device("cuda", int(os.environ.get("FMGI_DEVICE", "0")))
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        out = torch.empty((k, int(bounces), self.num_texels), dtype=torch.float32, device=dev)
        if isinstance(stream, int):
            handle = stream
        else:
            handle = stream.cuda_stream
            out.record_stream(stream)
        cp, _ = _ptr_array(c.data_ptr() if hasattr(c, "data_ptr") else c for c in covers)
        op, _ = _ptr_array(out[i].data_ptr() for i in range(k))
        check(self.lib.fmgi_rad_cache_sun_bounce(self.h, cp, _ptr(to_suns), _ptr(samples), k, int(bounces), op,
                                                 C.c_void_p(handle or None)), "fmgi_rad_cache_sun_bounce")
        return out


def geosphere(levels: int = 4) -> np.ndarray:
    """The AO direction table (fmgi_geosphere): float32 [n, 3] in the reference's order."""
    lib = load()
    n = lib.fmgi_geosphere(levels, None, 0)
    if n < 0:
        raise FmgiError(lib.fmgi_last_error().decode())
    out = np.zeros((n, 3), np.float32)
    lib.fmgi_geosphere(levels, _ptr(out), n)
    return out


def ao_tree(sc: Scene) -> np.ndarray:
    """The AO BSP tree (fmgi_ao_tree encoding)."""
    lib = load()
    tex = np.zeros((sc.num_texels, 4), np.float32)
    g, keep = make_geometry(sc, tex)
    n = lib.fmgi_ao_tree(C.byref(g), None, 0)
    if n < 0:
        raise FmgiError(lib.fmgi_last_error().decode())
    out = np.zeros(max(n, 1), np.int32)
    lib.fmgi_ao_tree(C.byref(g), _ptr(out), n)
    return out[:n]


def output_tiles(sc: Scene, texels: np.ndarray, spa: int, tint_extra: int = 0):
    """The output step on the GPU (fmgi_output_tiles): (normalised texels, RGB8 bytes of every tile)."""
    lib = load()
    tex = np.ascontiguousarray(texels, np.float32)
    out = np.empty_like(tex)
    g, keep = make_geometry(sc, tex)
    n = lib.fmgi_output_tile_bytes(C.byref(g))
    rgb = np.zeros(max(n, 1), np.uint8)
    check(lib.fmgi_output_tiles(C.byref(g), spa, tint_extra, _ptr(out), _ptr(rgb)), "fmgi_output_tiles")
    return out, rgb[:n]


# ---- view renderer (include/flatmatch_gi.h) ---------------------------------------

CAMERA_DTYPE = np.dtype([("pos", "<f4", 3), ("dir", "<f4", 3), ("up", "<f4", 3), ("pixel", "<f4")])
assert CAMERA_DTYPE.itemsize == 40


def camera(pos, dir, up=(0, 0, 1), pixel=0.001) -> np.ndarray:
    """One fmgi_camera record: position, viewing direction (any non-zero length), up vector (used as given)
    and the size of a pixel on the screen plane at distance 1 (the reference tool's is 1/1000)."""
    c = np.zeros((), CAMERA_DTYPE)
    c["pos"], c["dir"], c["up"], c["pixel"] = pos, dir, up, pixel
    return c


def _cameras(cams) -> np.ndarray:
    return np.ascontiguousarray(np.atleast_1d(np.asarray(cams, CAMERA_DTYPE)))


def render_views(sc: Scene, cams, width: int, height: int, tiles_rgb: np.ndarray | None = None,
                 background=(0, 0, 0)) -> dict:
    """The reference's debug raycaster on the GPU (fmgi_render_views): one width x height image per camera.
    Returns {"wall", "texel" (int32), "dist" (float32)} as [cameras, height, width] arrays (-1, -1, +inf where a
    ray hits nothing) and, when tiles_rgb (output_tiles' RGB8 bytes) is given, "rgb" (uint8, a trailing [3]):
    the hit tile's bytes, or `background`."""
    lib = load()
    cams = _cameras(cams)
    n = len(cams)
    g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
    tiles = None if tiles_rgb is None else np.ascontiguousarray(tiles_rgb, np.uint8)
    if tiles is not None and len(tiles) != lib.fmgi_output_tile_bytes(C.byref(g)):
        raise FmgiError(f"tiles_rgb holds {len(tiles)} bytes, the scene's tiles take {lib.fmgi_output_tile_bytes(C.byref(g))}")
    want_rgb = tiles is not None
    out = {"wall": np.empty((n, height, width), np.int32), "texel": np.empty((n, height, width), np.int32),
           "dist": np.empty((n, height, width), np.float32)}
    if want_rgb:
        out["rgb"] = np.empty((n, height, width, 3), np.uint8)
    bg = np.array(background, np.uint8)
    assert bg.shape == (3,)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731  (empty arrays keep a valid pointer)
    check(lib.fmgi_render_views(C.byref(g), p(cams), n, width, height, None if tiles is None else p(tiles), p(bg),
                                p(out["wall"]), p(out["texel"]), p(out["dist"]), p(out["rgb"]) if want_rgb else None),
          "fmgi_render_views")
    del keep
    return out


_VIEW_FILTERS = {"nearest": VIEW_NEAREST, "bilinear": VIEW_BILINEAR}
PROJECTIONS = {"pinhole": PROJ_PINHOLE, "ortho": PROJ_ORTHO, "equirect": PROJ_EQUIRECT}


def _projection(projection) -> int:
    if projection not in PROJECTIONS:
        raise FmgiError(f"projection {projection!r}: one of {sorted(PROJECTIONS)}")
    return PROJECTIONS[projection]


def shade_views(sc: Scene, cams, width: int, height: int, tiles_rgb: np.ndarray | None = None, background=(0, 0, 0),
                samples: int = 1, filter: str = "nearest", *, projection: str = "pinhole", gloss: float = 0.0) -> dict:
    """Supersampled, filtered camera views (fmgi_shade_views): samples x samples rays per pixel, each coloured
    from the hit wall's tiles ("nearest": the tile it lands in, "bilinear": the four around it, clamped to the
    wall) or `background`, averaged in fixed point. Returns {"coverage"} (uint8 [cameras, height, width]: the
    pixel's rays that hit a wall) and, when tiles_rgb is given, {"rgb"} (uint8, a trailing [3]). samples=1 with
    "nearest" gives render_views' rgb. projection: "pinhole", "ortho" (parallel rays along dir, `pixel` metres
    per pixel: the plan at true scale) or "equirect" (the 360-degree panorama from pos, column width / 2 looking
    along dir; fmgi_shade_views_proj). gloss in [0, 1]: a sample that lands on the floor (z <= 0.0005, where the
    bake mirrors its photons) casts one mirror ray and takes gloss of its colour from what that ray sees
    (fmgi_shade_views_gloss); 0 is the matt floor of the calls above."""
    lib = load()
    if filter not in _VIEW_FILTERS:
        raise FmgiError(f"filter {filter!r}: one of {sorted(_VIEW_FILTERS)}")
    proj = _projection(projection)
    cams = _cameras(cams)
    n = len(cams)
    g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
    tiles = None if tiles_rgb is None else np.ascontiguousarray(tiles_rgb, np.uint8)
    if tiles is not None and len(tiles) != lib.fmgi_output_tile_bytes(C.byref(g)):
        raise FmgiError(f"tiles_rgb holds {len(tiles)} bytes, the scene's tiles take {lib.fmgi_output_tile_bytes(C.byref(g))}")
    out = {"coverage": np.empty((n, height, width), np.uint8)}
    if tiles is not None:
        out["rgb"] = np.empty((n, height, width, 3), np.uint8)
    bg = np.array(background, np.uint8)
    assert bg.shape == (3,)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    if gloss != 0:
        check(lib.fmgi_shade_views_gloss(C.byref(g), p(cams), n, width, height, proj,
                                         None if tiles is None else p(tiles), p(bg), samples, _VIEW_FILTERS[filter],
                                         gloss, p(out["rgb"]) if tiles is not None else None, p(out["coverage"])),
              "fmgi_shade_views_gloss")
    elif proj == PROJ_PINHOLE:
        check(lib.fmgi_shade_views(C.byref(g), p(cams), n, width, height, None if tiles is None else p(tiles), p(bg),
                                   samples, _VIEW_FILTERS[filter], p(out["rgb"]) if tiles is not None else None,
                                   p(out["coverage"])), "fmgi_shade_views")
    else:
        check(lib.fmgi_shade_views_proj(C.byref(g), p(cams), n, width, height, proj,
                                        None if tiles is None else p(tiles), p(bg), samples, _VIEW_FILTERS[filter],
                                        p(out["rgb"]) if tiles is not None else None, p(out["coverage"])),
              "fmgi_shade_views_proj")
    del keep
    return out


def view_candidates(sc: Scene, cam, *, projection: str = "pinhole"):
    """One camera's sorted candidate list from the device (fmgi_view_candidates): (wall indices int32,
    minDistance float32), in the order the rays walk it. projection "ortho" / "equirect": that camera's list
    (fmgi_view_candidates_proj); "ortho" keys are depths along dir."""
    lib = load()
    proj = _projection(projection)
    cams = _cameras(cam)
    assert len(cams) == 1
    g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
    cap = len(sc.walls)
    idx = np.zeros(max(cap, 1), np.int32)
    md = np.zeros(max(cap, 1), np.float32)
    if proj == PROJ_PINHOLE:
        n = check(lib.fmgi_view_candidates(C.byref(g), cams.ctypes.data_as(C.c_void_p), _ptr(idx), _ptr(md), cap),
                  "fmgi_view_candidates")
    else:
        n = check(lib.fmgi_view_candidates_proj(C.byref(g), cams.ctypes.data_as(C.c_void_p), proj, _ptr(idx), _ptr(md),
                                                cap), "fmgi_view_candidates_proj")
    del keep
    return idx[:n], md[:n]


def view_stats() -> dict:
    """fmgi_view_stats: the last render_views or shade_views call's cameras, rays, candidates, intersects() tests and times."""
    st = ViewStats()
    check(load().fmgi_view_stats(C.byref(st)), "fmgi_view_stats")
    return st.as_dict()


def view_gloss_stats() -> dict:
    """fmgi_view_gloss_stats: the mirror rays, their hits and their intersects() tests of the last shade_views call
    with gloss > 0 or ViewCache(mirror=True); zeros after any other view call."""
    st = ViewGlossStats()
    check(load().fmgi_view_gloss_stats(C.byref(st)), "fmgi_view_gloss_stats")
    return st.as_dict()


# ---- traced views (include/flatmatch_gi.h) ------------------------------------------------

def view_cache_bytes(num_cams: int, width: int, height: int, samples: int = 1, filter: str = "nearest") -> int:
    """fmgi_view_cache_bytes: the device bytes of a ViewCache's records; 0 for arguments ViewCache rejects."""
    if filter not in _VIEW_FILTERS:
        raise FmgiError(f"filter {filter!r}: one of {sorted(_VIEW_FILTERS)}")
    return int(load().fmgi_view_cache_bytes(num_cams, width, height, samples, _VIEW_FILTERS[filter]))


def _ptr_array(ptrs):
    ptrs = [int(p) for p in ptrs]
    return (C.c_void_p * max(len(ptrs), 1))(*[C.c_void_p(p) for p in ptrs]), len(ptrs)


class ViewCache:
    """A traced view (fmgi_view_cache): shade_views' rays cast once, every sample's taps kept on the device.
    tiles() runs the output step on device lightmaps and shade() gathers one picture per tile set, each what
    output_tiles followed by shade_views gives, with no host round trip. Device buffers are integer addresses.
    mirror=True also traces every floor sample's mirror ray (fmgi_view_cache_create_gloss), so that shade() takes
    any gloss from the one trace."""

    def __init__(self, sc: Scene, cams, width: int, height: int, samples: int = 1, filter: str = "nearest", *,
                 projection: str = "pinhole", mirror: bool = False):
        self.lib = load()
        self.h = None
        if filter not in _VIEW_FILTERS:
            raise FmgiError(f"filter {filter!r}: one of {sorted(_VIEW_FILTERS)}")
        proj = _projection(projection)
        cams = _cameras(cams)
        g, keep = make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), np.float32))
        h = C.c_void_p()
        if mirror:
            check(self.lib.fmgi_view_cache_create_gloss(C.byref(g), cams.ctypes.data_as(C.c_void_p), len(cams), width,
                                                        height, proj, samples, _VIEW_FILTERS[filter], C.byref(h)),
                  "fmgi_view_cache_create_gloss")
        elif proj == PROJ_PINHOLE:
            check(self.lib.fmgi_view_cache_create(C.byref(g), cams.ctypes.data_as(C.c_void_p), len(cams), width, height,
                                                  samples, _VIEW_FILTERS[filter], C.byref(h)), "fmgi_view_cache_create")
        else:
            check(self.lib.fmgi_view_cache_create_proj(C.byref(g), cams.ctypes.data_as(C.c_void_p), len(cams), width,
                                                       height, proj, samples, _VIEW_FILTERS[filter], C.byref(h)),
                  "fmgi_view_cache_create_proj")
        del keep
        self.h = h

    @property
    def projection(self) -> str:
        """the camera model the view was traced with: "pinhole", "ortho" or "equirect" """
        code = check(self.lib.fmgi_view_cache_projection(self.h), "fmgi_view_cache_projection")
        return {v: k for k, v in PROJECTIONS.items()}[code]

    @property
    def has_mirror(self) -> bool:
        """whether the view holds mirror records (mirror=True)"""
        return bool(check(self.lib.fmgi_view_cache_has_mirror(self.h), "fmgi_view_cache_has_mirror"))

    def close(self):
        if self.h:
            self.lib.fmgi_view_cache_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        """fmgi_view_cache_info: the view's shape, the scene's tiles, rays, hits, tests, record bytes and times."""
        st = ViewCacheInfo()
        check(self.lib.fmgi_view_cache_info(self.h, C.byref(st)), "fmgi_view_cache_info")
        return st.as_dict()

    def tiles(self, texel_ptrs, spa: int, tile_ptrs, tint_extra: int = 0, stream: int = 0):
        """fmgi_view_cache_tiles: tile_ptrs[k] (info()["tiles"] * 3 bytes) = output_tiles' RGB8 bytes for the device
        texels float32 [num_texels][4] at texel_ptrs[k], which stay as they are. Asynchronous on `stream`."""
        tp, n = _ptr_array(texel_ptrs)
        op, m = _ptr_array(tile_ptrs)
        if n != m:
            raise FmgiError(f"tiles: {n} texel buffers for {m} tile buffers")
        check(self.lib.fmgi_view_cache_tiles(self.h, tp, n, spa, tint_extra, op, C.c_void_p(stream or None)),
              "fmgi_view_cache_tiles")

    def shade(self, tile_ptrs, rgb_ptrs, background=(0, 0, 0), coverage_ptr: int = 0, stream: int = 0, *,
              gloss: float = 0.0):
        """fmgi_view_cache_shade: rgb_ptrs[k] (uint8 [cameras][height][width][3]) = shade_views' rgb for the device
        tiles at tile_ptrs[k]; coverage_ptr (uint8 [cameras][height][width], or 0) = its coverage. Asynchronous on
        `stream`. gloss > 0 (fmgi_view_cache_shade_gloss) needs a view made with mirror=True."""
        tp, n = _ptr_array(tile_ptrs)
        rp, m = _ptr_array(rgb_ptrs)
        if n != m:
            raise FmgiError(f"shade: {n} tile buffers for {m} pictures")
        bg = np.array(background, np.uint8)
        assert bg.shape == (3,)
        if gloss != 0:
            check(self.lib.fmgi_view_cache_shade_gloss(self.h, tp, n, bg.ctypes.data_as(C.c_void_p), gloss, rp,
                                                       C.c_void_p(coverage_ptr or None), C.c_void_p(stream or None)),
                  "fmgi_view_cache_shade_gloss")
            return
        check(self.lib.fmgi_view_cache_shade(self.h, tp, n, bg.ctypes.data_as(C.c_void_p), rp,
                                             C.c_void_p(coverage_ptr or None), C.c_void_p(stream or None)),
              "fmgi_view_cache_shade")
