"""The radiosity cache (include/flatmatch_gi.h) without a device.

  tests/rad_solve_restate.py == oracle/rad_oracle.c bit for bit on three scenes: the restatement the GPU tests
  compare fmgi_rad_cache_solve with is pinned to the oracle, which tests/test_radiosity.py pins to the reference
  the scenes reach what the kernels must handle (window and light texels, misses, odd job counts)
  the restatement is exactly linear in the palette and its sets are independent
  argument errors of every new call, in the header's order, before a device is looked for
  tools/relight_radiosity.py's scenario handling
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
import rad_cache_cases as CASES
import rad_solve_restate as R
from conftest import PKG, REPO
from fmgi import _lib, scene

f32 = np.float32
ARG, NO_DEVICE = -3, -1
NEW = ("fmgi_rad_cache_bytes", "fmgi_rad_cache_create", "fmgi_rad_cache_destroy", "fmgi_rad_cache_info",
       "fmgi_rad_cache_sids", "fmgi_rad_reference_emit", "fmgi_rad_cache_solve")


def test_new_names_are_exported():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(lib, name)
    assert _lib.RAD_CACHE_MAX_SETS == fmgi.RAD_CACHE_MAX_SETS == 8
    assert _lib.RAD_CACHE_MAX_ITERATIONS == fmgi.RAD_CACHE_MAX_ITERATIONS == 64
    assert C.sizeof(_lib.RadCacheInfo) == 72
    assert callable(fmgi.RadCache) and callable(fmgi.rad_reference_emit) and callable(fmgi.rad_cache_bytes)
    with open(os.path.join(REPO, "include", "flatmatch_gi.h")) as f:
        header = f.read()
    assert "#define FMGI_RAD_CACHE_MAX_SETS 8" in header and all(name + "(" in header for name in NEW)


# ---- the restatement against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box", "open_tilted"])
def test_restatement_equals_oracle(libc, name):
    sc, tex, sids, _ = CASES.oracle(libc, name)
    got = R.solve(sc, sids, R.reference_emit(sc)[None], 7)
    assert got.shape == (1, sc.num_texels, 4)
    assert np.array_equal(got[0].view(np.uint32), tex.view(np.uint32))


def test_restatement_equals_oracle_and_is_linear_on_the_lit_box(libc):
    """one run of four sets: the reference palette (== the oracle), its double (== the double, bit for bit), zeros
    (== zeros), and a random palette that a run of its own reproduces: a set does not see its neighbours"""
    sc, tex, sids, _ = CASES.oracle(libc, "box_lit")
    pal = CASES.palettes("box_lit", 5)
    assert (pal[1] == 2 * pal[0]).all() and not pal[2].any() and pal[4].any()
    got = R.solve(sc, sids, pal[[0, 1, 2, 4]], 7)
    assert np.array_equal(got[0].view(np.uint32), tex.view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), (got[0] * f32(2)).view(np.uint32))
    assert np.array_equal(got[2].view(np.uint32), np.zeros_like(got[2]).view(np.uint32))
    alone = R.solve(sc, sids, pal[4:5], 7)
    assert np.array_equal(alone[0].view(np.uint32), got[3].view(np.uint32))
    assert got[3].any() and not np.array_equal(got[3], got[0])


def test_rounds_of_a_tuple_are_the_rounds_of_single_runs(libc):
    sc = scene.box_scene(8, tile_size=1.0)
    rng = np.random.default_rng(3)
    jobs = len(R.job_texels(sc))
    _, ntex = R.layout(sc)
    sids = rng.integers(-1, ntex, (jobs, R.RAYS)).astype(np.int32)
    both = R.solve(sc, sids, R.reference_emit(sc)[None], (1, 2))
    for n in (1, 2):
        assert np.array_equal(both[n].view(np.uint32), R.solve(sc, sids, R.reference_emit(sc)[None], n).view(np.uint32))
    assert not np.array_equal(both[1], both[2])


def test_the_scenes_reach_what_the_kernels_must_handle(libc):
    sc, _, sids, _ = CASES.oracle(libc, "box_lit")
    rects, ntex = R.layout(sc)
    first_light = rects[len(sc.walls) + len(sc.windows)][0]
    assert len(sc.windows) == 1 and len(sc.lights) == 1
    assert ((sids >= sc.num_texels) & (sids < first_light)).any(), "no ray reaches the window"
    assert ((sids >= first_light) & (sids < ntex)).any(), "no ray reaches the light"
    assert sids.max() < ntex
    sc, _, sids, _ = CASES.oracle(libc, "open_tilted")
    assert 0.10 < float((sids < 0).mean()) < 0.90
    jobs = len(R.job_texels(sc))
    assert jobs == len(sids) and jobs % 64 != 0 and jobs % 8 != 0, jobs


# ---- argument errors ------------------------------------------------------------------------------------------------

def _geo(sc):
    return fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))


def test_bytes_and_reference_emit_against_python_arithmetic():
    lib = _lib.load()
    for sc in (CASES.get_scene("box_lit"), CASES.get_scene("open_tilted"), scene.box_scene(8, tile_size=1.0)):
        jobs = len(R.job_texels(sc))
        rects = len(sc.walls) + len(sc.windows) + len(sc.lights)
        assert fmgi.rad_cache_bytes(sc) == 40_000 * jobs + 64 * jobs + 64 * rects
        assert np.array_equal(fmgi.rad_reference_emit(sc), R.reference_emit(sc))
    assert lib.fmgi_rad_cache_bytes(None) == ARG and "fmgi_rad_cache_bytes" in _lib.last_error()
    assert lib.fmgi_rad_reference_emit(None, None) == ARG and "fmgi_rad_reference_emit" in _lib.last_error()
    g, keep = _geo(CASES.get_scene("box_lit"))
    assert lib.fmgi_rad_reference_emit(C.byref(g), None) == ARG and "emit" in _lib.last_error()
    dark = scene.box_scene(8, tile_size=1.0)
    dark = scene.Scene("dark", dark.walls, dark.windows[:0], dark.lights[:0], dark.num_texels)
    g, keep = _geo(dark)
    assert lib.fmgi_rad_reference_emit(C.byref(g), None) == 0  # nothing to fill
    assert fmgi.rad_reference_emit(dark).shape == (0, 3)


def test_argument_errors_before_a_device_is_looked_for(libc):
    lib = _lib.load()
    sc = scene.box_scene(8, tile_size=1.0)
    g, keep = _geo(sc)
    h = C.c_void_p(77)
    fn = "fmgi_rad_cache_create"
    assert lib.fmgi_rad_cache_create(None, C.byref(h)) == ARG and h.value is None
    assert "geometry" in _lib.last_error() and fn in _lib.last_error()
    assert lib.fmgi_rad_cache_create(C.byref(g), None) == ARG
    assert "out" in _lib.last_error() and fn in _lib.last_error()
    bad = scene.Scene("bad", sc.walls.copy(), sc.windows, sc.lights, sc.num_texels)
    bad.walls["lm"][0, 1] = 0  # an empty lightmap: fmgi_radiosity's geometry check, under this call's name
    gb, keepb = _geo(bad)
    h = C.c_void_p(77)
    assert lib.fmgi_rad_cache_create(C.byref(gb), C.byref(h)) == ARG and h.value is None
    assert "lightmap" in _lib.last_error() and fn in _lib.last_error()
    assert lib.fmgi_rad_cache_bytes(C.byref(gb)) == ARG
    # the handle's calls
    assert lib.fmgi_rad_cache_destroy(None) is None
    info = _lib.RadCacheInfo()
    assert lib.fmgi_rad_cache_info(None, C.byref(info)) == ARG and "fmgi_rad_cache_info" in _lib.last_error()
    one = np.zeros(4, np.int32)
    assert lib.fmgi_rad_cache_sids(None, one.ctypes.data_as(C.c_void_p)) == ARG
    assert "fmgi_rad_cache_sids" in _lib.last_error()
    ptrs = (C.c_void_p * 1)(C.c_void_p(64))
    emit = np.full((1, 1, 3), 30, f32)
    for sets, iters in ((1, 7), (0, 7), (1, 0), (1, 65)):
        assert lib.fmgi_rad_cache_solve(None, emit.ctypes.data_as(C.c_void_p), sets, iters, ptrs, None) == ARG
        assert "fmgi_rad_cache_solve" in _lib.last_error()
    libc.srand(9)
    want = libc.rand()
    libc.srand(9)
    assert lib.fmgi_rad_cache_create(C.byref(gb), C.byref(h)) == ARG  # an argument error draws nothing
    assert libc.rand() == want


_NO_DEVICE_PROG = """
import ctypes as C, sys
sys.path.insert(0, %r)
import numpy as np
import fmgi
from fmgi import _lib, scene
lib = _lib.load()
libc = C.CDLL(None)
libc.rand.restype = C.c_int
libc.initstate.restype = C.c_void_p
libc.initstate.argtypes = [C.c_uint, C.c_void_p, C.c_size_t]
libc.setstate.restype = C.c_void_p
libc.setstate.argtypes = [C.c_void_p]
sc = scene.box_scene(8, tile_size=1.0)
g, keep = fmgi.make_geometry(sc, np.zeros((sc.num_texels, 4), np.float32))
h = C.c_void_p(77)
buf = (C.c_char * 64)()
prev = libc.initstate(12345, buf, 32)  # glibc's TYPE_1 generator
rc = lib.fmgi_rad_cache_create(C.byref(g), C.byref(h))
print("TYPE1", rc, h.value, "TYPE_3" in _lib.last_error())
libc.setstate(prev)
libc.srand(9)
want = [libc.rand() for _ in range(3)]
libc.srand(9)
rc = lib.fmgi_rad_cache_create(C.byref(g), C.byref(h))
print("NODEV", rc, h.value, [libc.rand() for _ in range(3)] == want)
try:
    fmgi.RadCache(sc)
except fmgi.FmgiError as e:
    print("ERR", e)
print("ALIVE")
"""


def test_no_device_is_an_error_code_and_the_stream_is_put_back(tmp_path):
    """libc's state is checked ahead of the device; without a device create returns FMGI_ERR_NO_DEVICE, leaves *out
    NULL and the rand() stream where it was, and the process lives on"""
    prog = tmp_path / "nogpu_rad_cache.py"
    prog.write_text(_NO_DEVICE_PROG % PKG)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"TYPE1 {ARG} None True", lines
    assert lines[1] == f"NODEV {NO_DEVICE} None True", lines
    assert "fmgi_rad_cache_create failed (-1)" in lines[2] and lines[3] == "ALIVE"


# ---- the tool -------------------------------------------------------------------------------------------------------

def _tool():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight_radiosity
    finally:
        sys.path.pop(0)
    return relight_radiosity


def test_tool_scenarios():
    tool = _tool()
    names, emit = tool.scenario_emit(
        [{"name": "day", "windows": [30, 30, 30], "lights": [[1, 2, 3], [4, 5, 6]]},
         {"name": "lamp", "lights": [0.5, 0.25, 0]}, {"name": "each", "windows": [[7, 8, 9]], "lights": [1, 1, 1]}], 1, 2)
    assert names == ["day", "lamp", "each"] and emit.dtype == f32 and emit.shape == (3, 3, 3)
    assert emit[0].tolist() == [[30, 30, 30], [1, 2, 3], [4, 5, 6]]
    assert emit[1].tolist() == [[0, 0, 0], [0.5, 0.25, 0], [0.5, 0.25, 0]]
    assert emit[2].tolist() == [[7, 8, 9], [1, 1, 1], [1, 1, 1]]
    with pytest.raises(SystemExit, match="3 lights triples for 2 lights"):
        tool.scenario_emit([{"name": "a", "lights": [[1, 1, 1]] * 3}], 1, 2)
    with pytest.raises(SystemExit, match="'a' appears twice"):
        tool.scenario_emit([{"name": "a"}, {"name": "b"}, {"name": "a"}], 1, 2)
    with pytest.raises(SystemExit, match="negative or not finite"):
        tool.scenario_emit([{"name": "a", "windows": [1, -1, 1]}], 1, 2)
    with pytest.raises(SystemExit, match="negative or not finite"):
        tool.scenario_emit([{"name": "a", "windows": [1, float("nan"), 1]}], 1, 2)
    with pytest.raises(SystemExit, match="keys"):
        tool.scenario_emit([{"name": "a", "window": [1, 1, 1]}], 1, 2)
    with pytest.raises(SystemExit):
        tool.scenario_emit([], 1, 2)
    a = tool.parse_args(["box8", "--scenarios", "s.json"])
    assert (a.iterations, a.view, a.output) == (7, False, "out")
