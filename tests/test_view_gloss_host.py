"""The glossy floor of the views (fmgi_*_gloss): what can be checked without a device.

  the restatement (view_gloss_restate.py) at gloss 0 == test_view_shade.shade / view_proj_restate.shade
  the pruned mirror walk == the brute one on every case: wall and distance bits
  the counts of the CPU prototype the definition was written from, at 2 x 2 samples
  every family of cases holds a mirror sample, a hit that does not mirror and (open scenes) a mirror ray that misses
  constant tiles under their own colour as background stay constant at any gloss
  gloss 1 on a mirror sample gives the mirror tap's bytes at one nearest sample
  argument errors in their order and the no-device code of the C ABI; the Python keywords; the tools' flag

fmgi_view_cache_shade_gloss on a view without mirror records (FMGI_ERR_STATE) needs a view, which needs a device:
test_gpu_view_gloss.py checks it.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
import test_view as T
import test_view_shade as V
import view_gloss_restate as G
import view_proj_restate as P
from conftest import PKG, REPO
from fmgi import _lib

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the restatement's own conditions -------------------------------------------------------------------------

@pytest.mark.parametrize("bilinear,S", [(False, 1), (True, 2), (True, 3)])
@pytest.mark.parametrize("name", G.CASES)
def test_gloss_zero_is_the_plain_restatement(name, S, bilinear):
    got = G.shade(name, S, bilinear, 0.0)
    exp = V._restated(name, S, bilinear) if name in G.PINHOLE_CASES else P.restated(name, S, bilinear)
    assert np.array_equal(got["rgb"], exp["rgb"]) and np.array_equal(got["coverage"], exp["coverage"])
    assert got["tests"] == exp["tests"]
    assert (got["mirror_rays"], got["mirror_hits"], got["mirror_tests"]) == (0, 0, 0)


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("name", G.CASES)
def test_pruned_mirror_walk_equals_the_brute_walk(name, S):
    """the early break (base + best) < key loses no hit: a wall is never nearer to the camera than its key, and the
    path camera -> floor -> hit is base + best long"""
    a, b = G.trace(name, S), G.trace(name, S, brute=True)
    assert np.array_equal(a["mirror"], b["mirror"]) and a["mirror"].any()
    assert np.array_equal(a["wall2"], b["wall2"]) and np.array_equal(_bits(a["best"]), _bits(b["best"]))
    nwalls = len(G.case(name)[0].walls)
    assert b["mirror_tests"] == int(a["mirror"].sum()) * nwalls and a["mirror_tests"] <= b["mirror_tests"]
    assert len(a["list"][0]) == nwalls and sorted(a["list"][0]) == list(range(nwalls)), "every wall, once"


# (mirror samples, primary misses or None, mirror misses, mirror tests or None) of the CPU prototype at 2 x 2 samples
PROTOTYPE = {"box8_A": (602, None, 0, 3586), "box8_C": (1008, 576, 0, None), "example_tool": (425, None, 0, 63391),
             "box8_ortho": (1786, None, 0, None), "example_equirect": (30, None, 0, None),
             "open_tilted_ortho": (1707, None, 1529, 297368), "open_tilted_equirect": (667, None, 459, 102468)}
RAYS = {"box8_A": 1920, "box8_C": 1920, "example_tool": 4800, "box8_ortho": 1920, "example_equirect": 3200}


@pytest.mark.parametrize("name", sorted(PROTOTYPE))
def test_the_prototype_counts(name):
    samples, primary_misses, misses, tests = PROTOTYPE[name]
    tr = G.trace(name, 2)
    assert int(tr["mirror"].sum()) == samples and int((tr["wall2"] < 0).sum()) == misses
    if name in RAYS:
        assert tr["wall"].size == RAYS[name]
    if primary_misses is not None:
        assert int((tr["wall"] < 0).sum()) == primary_misses
    if tests is not None:
        assert tr["mirror_tests"] == tests


def test_every_family_holds_what_the_comparisons_need():
    families = {"pinhole": G.PINHOLE_CASES, "ortho": [n for n in P.SHADE_CASES if n.endswith("ortho")],
                "equirect": [n for n in P.SHADE_CASES if n.endswith("equirect")]}
    for family, names in families.items():
        trs = [G.trace(n, 2) for n in names]
        assert any(t["mirror"].any() for t in trs), family
        assert any(((t["wall"] >= 0) & ~t["mirror"]).any() for t in trs), family + ": a hit that does not mirror"
        assert any((t["wall"] < 0).any() for t in trs), family + ": a primary miss"
    for name in G.OPEN_CASES:
        tr = G.trace(name, 2)
        assert (tr["wall2"] < 0).any() and (tr["wall2"] >= 0).any(), name + ": mirror rays that miss and that hit"
    # the mirror test asks for the height alone: box8's plan sees nothing but mirror samples, and a wall that is no
    # floor mirrors where a ray meets its foot
    assert G.trace("box8_ortho", 2)["mirror"].sum() == (G.trace("box8_ortho", 2)["wall"] >= 0).sum()
    # the bounce shows: at gloss 0.75 the picture differs from the matt one on every case
    for name in G.CASES:
        assert not np.array_equal(G.shade(name, 2, True, 0.75)["rgb"], G.shade(name, 2, True, 0.0)["rgb"]), name


@pytest.mark.parametrize("gloss", [0.3, 1.0])
@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("name", ["box8_C", "example_tool", "open_tilted_ortho", "open_tilted_equirect"])
def test_constant_colour_stays_constant(name, bilinear, gloss):
    sc = G.case(name)[0]
    tiles = np.tile(np.array(V.COLOUR, np.uint8), int(V._tile_counts(sc).sum()))
    r = G.shade(name, 3, bilinear, gloss, tiles=tiles, bg=V.COLOUR)
    assert np.all(r["rgb"] == np.array(V.COLOUR)) and r["mirror_rays"] > 0


@pytest.mark.parametrize("name", G.CASES)
def test_full_gloss_is_the_mirror_tap(name):
    """one nearest sample at gloss 1: a mirror pixel holds exactly the tile its mirror ray hit (or the background), any
    other pixel what the matt picture holds"""
    r, matt, tr = G.shade(name, 1, False, 1.0), G.shade(name, 1, False, 0.0), G.trace(name, 1)
    m = tr["mirror"][0, 0]
    assert np.array_equal(r["rgb"][m], r["mval"].astype(np.int64)), "(1 - 1) * val + 1 * mval == mval, bytes and all"
    assert np.array_equal(r["rgb"][~m], matt["rgb"][~m])
    missed = tr["wall2"] < 0
    assert np.all(r["mval"][missed] == np.array(G.BG, f32))


# ---- the C ABI's argument checks ------------------------------------------------------------------------------

def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _geometry(sc):
    return fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))


def _shade(sc, cams, proj, gloss, width=4, height=4, tiles="yes", samples=1, filt=0):
    """(fmgi_shade_views_gloss's return code, fmgi_shade_views_proj's for the same arguments, the message)"""
    lib = _lib.load()
    g, keep = _geometry(sc)
    cams = np.atleast_1d(np.asarray(cams, fmgi.CAMERA_DTYPE))
    t = P.tiles("box8") if tiles == "yes" else None
    out, cov, bg = np.zeros((len(cams), 4, 4, 3), np.uint8), np.zeros((len(cams), 4, 4), np.uint8), np.zeros(3, np.uint8)
    old = lib.fmgi_shade_views_proj(C.byref(g), _p(cams), len(cams), width, height, proj, _p(t), _p(bg), samples, filt,
                                    _p(out), _p(cov))
    rc = lib.fmgi_shade_views_gloss(C.byref(g), _p(cams), len(cams), width, height, proj, _p(t), _p(bg), samples, filt,
                                    gloss, _p(out), _p(cov))
    assert not out.any() and not cov.any()
    return rc, old, _lib.last_error()


OK = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1), pixel=0.02)
BAD_GLOSS = (np.nan, np.inf, -np.inf, -0.001, 1.001, -1.0, 2.0)


def check_argument_errors():
    sc = T._scene("box8")
    ok = fmgi.camera(**OK)
    lib = _lib.load()
    for proj in (_lib.PROJ_PINHOLE, _lib.PROJ_ORTHO, _lib.PROJ_EQUIRECT):
        for gloss in BAD_GLOSS:
            rc, old, msg = _shade(sc, ok, proj, gloss)
            assert (rc, old) == (-3, -1) and "gloss" in msg and "fmgi_shade_views_gloss" in msg, (proj, gloss, msg)
        for gloss in (0.0, 1.0, 0.3, 1e-30):
            assert _shade(sc, ok, proj, gloss)[:2] == (-1, -1), "every argument accepted: the missing device is left"
    # fmgi_shade_views_proj's errors come first, in their order, whatever gloss is
    par = fmgi.camera(**dict(OK, dir=(0, 0, -2)))
    for gloss in (0.5, np.nan):
        for kw, word in ((dict(width=0), "image size"), (dict(tiles=None), "tiles_rgb"), (dict(samples=9), "samples"),
                         (dict(filt=2), "filter")):
            rc, old, msg = _shade(sc, ok, _lib.PROJ_ORTHO, gloss, **kw)
            assert rc == old == -3 and word in msg, (gloss, kw, msg)
        for cam, proj, word in ((fmgi.camera(**dict(OK, pixel=0)), _lib.PROJ_PINHOLE, "pixel"),
                                (fmgi.camera(**dict(OK, dir=(0, 0, 0))), _lib.PROJ_EQUIRECT, "direction"),
                                (ok, 9, "projection"), (par, _lib.PROJ_ORTHO, "cross(dir, up)")):
            rc, old, msg = _shade(sc, cam, proj, gloss)
            assert rc == old == -3 and word in msg, (gloss, word, msg)
    # the gloss is checked before the call finds that it has no cameras to do
    none = np.zeros(0, fmgi.CAMERA_DTYPE)
    assert _shade(sc, none, _lib.PROJ_PINHOLE, 0.5)[:2] == (0, 0) and _shade(sc, none, _lib.PROJ_PINHOLE, np.nan)[0] == -3
    # the traced view
    g, keep = _geometry(sc)
    cams = np.atleast_1d(ok)
    h = C.c_void_p(0x5A5A)
    assert lib.fmgi_view_cache_create_gloss(C.byref(g), _p(cams), 1, 4, 4, _lib.PROJ_PINHOLE, 1, 0, C.byref(h)) == -1
    assert h.value is None, "*out is NULL after an error"
    for kw, word in (((0, 4, 0, 1, 0), "image size"), ((4, 4, 0, 0, 0), "samples"), ((4, 4, 0, 1, 2), "filter"),
                     ((4, 4, 9, 1, 0), "projection")):
        w_, h_, proj, samples, filt = kw
        assert lib.fmgi_view_cache_create_gloss(C.byref(g), _p(cams), 1, w_, h_, proj, samples, filt, C.byref(h)) == -3
        assert word in _lib.last_error() and "fmgi_view_cache_create_gloss" in _lib.last_error()
    assert lib.fmgi_view_cache_create_gloss(C.byref(g), _p(cams), 1, 4, 4, 0, 1, 0, None) == -3
    assert lib.fmgi_view_cache_has_mirror(None) == -3
    one = (C.c_void_p * 1)(C.c_void_p(16))
    bg = np.zeros(3, np.uint8)
    assert lib.fmgi_view_cache_shade_gloss(None, one, 1, _p(bg), 0.5, one, None, None) == -3
    assert "fmgi_view_cache_shade_gloss" in _lib.last_error()
    assert lib.fmgi_view_gloss_stats(None) == -3
    st = _lib.ViewGlossStats()
    assert lib.fmgi_view_gloss_stats(C.byref(st)) == 0 and st.as_dict() == {"mirror_rays": 0, "mirror_hits": 0, "mirror_tests": 0}


def test_argument_errors_without_a_device():
    """the gloss's FMGI_ERR_ARG after fmgi_shade_views_proj's and before FMGI_ERR_NO_DEVICE, in a process that sees no
    device"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "import conftest, test_view_gloss_host as H; H.check_argument_errors(); print('PASSED')"],
                       cwd=os.path.join(REPO, "tests"), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr


def test_python_keywords():
    sc = T._scene("box8")
    cam = fmgi.camera(**OK)
    for gloss in (-0.5, 1.5, float("nan")):
        with pytest.raises(fmgi.FmgiError, match="gloss"):
            fmgi.shade_views(sc, cam, 4, 4, gloss=gloss)
    with pytest.raises(TypeError):
        fmgi.shade_views(sc, cam, 4, 4, None, (0, 0, 0), 1, "nearest", "pinhole", 0.5)  # keyword only
    for name in ("fmgi_shade_views_gloss", "fmgi_view_gloss_stats", "fmgi_view_cache_create_gloss",
                 "fmgi_view_cache_shade_gloss", "fmgi_view_cache_has_mirror"):
        assert name in _lib.EXPORTS
    assert C.sizeof(_lib.ViewGlossStats) == 24


def test_no_device_is_an_error_code(tmp_path):
    """Without a device the gloss calls return FMGI_ERR_NO_DEVICE and the process lives on."""
    prog = tmp_path / "nogpu_gloss.py"
    prog.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import fmgi\n"
        "from fmgi import scene\n"
        "sc = scene.box_scene(8, tile_size=1.0)\n"
        "cam = fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), pixel=0.02)\n"
        "for call in (lambda: fmgi.shade_views(sc, cam, 8, 8, samples=2, filter='bilinear', gloss=0.5),\n"
        "             lambda: fmgi.shade_views(sc, cam, 8, 8, projection='equirect', gloss=1.0),\n"
        "             lambda: fmgi.ViewCache(sc, cam, 8, 8, projection='ortho', mirror=True)):\n"
        "    try:\n"
        "        call()\n"
        "    except fmgi.FmgiError as e:\n"
        "        print('ERR', e)\n"
        "print(fmgi.view_gloss_stats())\n"
        "print('ALIVE')\n" % PKG
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 5 and lines[4] == "ALIVE"
    assert "fmgi_shade_views_gloss failed (-1)" in lines[0] and "fmgi_shade_views_gloss failed (-1)" in lines[1]
    assert "fmgi_view_cache_create_gloss failed (-1)" in lines[2]
    assert lines[3] == "{'mirror_rays': 0, 'mirror_hits': 0, 'mirror_tests': 0}"


def test_tools_take_the_gloss_flag(capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
        import relight_radiosity
        import render_view
    finally:
        sys.path.pop(0)
    for tool in (relight, relight_radiosity):
        base = ["box200", "--scenarios", "s.json"] + (["--spa", "1000"] if tool is relight else [])
        assert tool.parse_args(base).gloss == 0.0
        assert tool.parse_args(base + ["--view", "--gloss", "0.75"]).gloss == 0.75
        for bad in ("1.5", "-0.1", "nan", "shiny"):
            with pytest.raises(SystemExit):
                tool.parse_args(base + ["--view", "--gloss", bad])
    with pytest.raises(SystemExit):
        render_view.main(["box8", "--gloss", "2"])
    assert "--gloss" in capsys.readouterr().err
    for tool in ("bench_view.py", "render_view.py"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", tool), "--help"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and "--gloss" in r.stdout, tool
