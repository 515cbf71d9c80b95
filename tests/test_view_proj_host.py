"""Orthographic and equirectangular cameras (fmgi_*_proj): what holds without a GPU.

  the restatement (view_proj_restate.py) on cases one can check by hand: the top-down frame, the floor texel under
  a pixel, a closed box that a panorama covers completely, the walls behind the viewing direction
  conditions the GPU comparisons rest on: the walk with its early break == a walk of the whole list on every case
  the GPU tests use, misses and partial coverage, constant tiles stay constant
  the C ABI's new argument errors, their order, their precedence over the missing device, PINHOLE == the old calls
  the tools' --projection flag

Every condition here is made on the restatement alone; the code under test appears only in the error checks.
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
import view_proj_restate as P
from conftest import PKG, REPO
from fmgi import _lib

f32 = np.float32


# ---- the restatement on hand-checkable cases ------------------------------------------------------------------

def test_ortho_looks_down_on_box8():
    sc, cam, proj, w, h = P.case("box8_ortho")
    pos, f, r, u = P.frame(cam)
    assert [float(c) for c in f] == [0, 0, -1]
    assert [float(c) for c in r] == [1, 0, 0] and [float(c) for c in u] == [0, 1, 0]
    floor, ceiling = 0, 1
    assert sc.walls[floor]["n"][2] == 1 and sc.walls[ceiling]["n"][2] == -1 and float(pos[2]) > 2.6
    cw, cd = P.candidates(sc, cam, proj)
    assert list(cw) == [floor], "the ceiling and the four walls (seen edge-on) are not in the list"
    assert float(cd[0]) == float(pos[2]), "the key is the floor's depth"
    got = P.restated("box8_ortho", 1, False)
    wall, tile = got["wall"][0, 0], got["tile"][0, 0]
    pixel = float(cam["pixel"])
    ox = float(pos[0]) + pixel * (np.arange(w) - w // 2)
    oy = float(pos[1]) - pixel * (np.arange(h) - h // 2)
    inside = (oy[:, None] > 0.01) & (oy[:, None] < 7.99) & (ox[None, :] > 0.01) & (ox[None, :] < 9.99)
    outside = (oy[:, None] < -0.01) | (oy[:, None] > 8.01) | (ox[None, :] < -0.01) | (ox[None, :] > 10.01)
    assert inside.sum() > 300 and outside.sum() > 20 and (inside | outside).all()
    assert np.all(wall[inside] == floor) and np.all(wall[outside] == -1)
    # the floor starts at (10, 0, 0), its width runs 10 m along -x over s1 tiles, its height 8 m along +y over s2
    s1, s2 = int(sc.walls[floor]["lm"][1]), int(sc.walls[floor]["lm"][2])
    assert [float(c) for c in sc.walls[floor]["pos"][:3]] == [10, 0, 0] and s1 > 1 and s2 > 1
    tu, tv = (10.0 - ox) * s1 / 10.0, oy * s2 / 8.0
    tx, ty = np.floor(tu).astype(int), np.floor(tv).astype(int)
    away = (np.abs(tu - np.round(tu))[None, :] > 1e-3) & (np.abs(tv - np.round(tv))[:, None] > 1e-3)  # off tile borders
    exp = ty[:, None] * s1 + tx[None, :]
    assert (inside & away).sum() > 200
    assert np.array_equal(tile[inside & away], exp[inside & away])
    assert np.array_equal(got["dist"][0, 0][inside].view(np.uint32), np.full(inside.sum(), pos[2], f32).view(np.uint32))
    assert np.array_equal(got["coverage"], (wall >= 0).astype(np.int64))


@pytest.mark.parametrize("S", [1, 3])
def test_equirect_inside_the_closed_box8(S):
    sc, cam, proj, w, h = P.case("box8_equirect")
    got = P.restated("box8_equirect", S, True)
    assert np.all(got["coverage"] == S * S), "a closed box: every sample hits"
    cw, _ = P.candidates(sc, cam, proj)
    assert sorted(cw) == list(range(6))
    if S != 1:
        return
    pin = T.restate(sc, fmgi.camera(cam["pos"], cam["dir"], cam["up"], 0.02), w, h)
    wall = got["wall"][0, 0]
    assert wall[h // 2, w // 2] == pin["wall"][h // 2, w // 2] >= 0, "column W/2 looks along dir"
    behind = sorted(set(cw) - set(pin["cand_wall"]))
    assert behind, "walls wholly behind the camera direction"
    left, right, middle = wall[:, :w // 4], wall[:, 3 * w // 4:], wall[:, 3 * w // 8:5 * w // 8]
    for b in behind:
        assert (left == b).any() and (right == b).any() and not (middle == b).any(), b
    assert wall[0, 0] == 1 and wall[h - 1, 0] == 0, "row 0 looks up at the ceiling, the last row down at the floor"
    # x grows to the right: a quarter turn to the right of dir = (1, 0.5, -0.1) lies the wall y = 0 (index 2)
    assert wall[h // 2, 3 * w // 4] == 2 and wall[h // 2, w // 4] == 3


def test_equirect_on_the_example_flat():
    got = P.restated("example_equirect", 3, True)
    cov = got["coverage"]
    assert int((cov == 0).sum()) > 0 and int(((cov > 0) & (cov < 9)).sum()) > 0 and int((cov == 9).sum()) > 0
    sc, cam, proj, _, _ = P.case("example_equirect")
    pin = T._candidates(sc, T._v(cam["pos"]), T._normalized(T._v(cam["dir"])))[0]
    assert set(pin) <= set(P.candidates(sc, cam, proj)[0]) and len(pin) > 100, "the pin-hole's walls and those behind"


def test_the_cases_hold_what_the_comparisons_need():
    for name in P.SHADE_CASES:
        near, lin = P.restated(name, 3, False), P.restated(name, 3, True)
        hit = near["coverage"] > 0
        assert hit.any(), name
        assert int((near["rgb"][hit] != lin["rgb"][hit]).any(axis=-1).sum()) > 0, name + ": bilinear != nearest"
        assert np.array_equal(near["coverage"], lin["coverage"]) and near["tests"] == lin["tests"]
        assert len(np.unique(near["wall"])) > 2 or name == "box8_ortho", name
        if name != "box8_equirect":
            assert int((near["coverage"] == 0).sum()) > 0, name + ": misses"
            assert int(((near["coverage"] > 0) & (near["coverage"] < 9)).sum()) > 0, name + ": silhouettes"
        cw, cd = P.candidates(*P.case(name)[:3])
        assert near["tests"] < near["wall"].size * len(cw) or len(cw) == 1, name + ": the early break ends walks"
    for proj in P.PROJECTIONS:
        n = [len(P.candidates(P.scene("floor"), c, proj)[0]) for c in P.BATCH_CAMS]
        assert n[1] == 0 and min(n[0], n[2], n[3]) > 0, "the batch's second camera has an empty list"
        for s in ("tilted56", "tilted57"):
            assert len(P.candidates(*P.case(f"{s}_{proj}")[:3])[0]) > 0
    assert len(P.scene("tilted56").walls) == 256 and len(P.scene("tilted57").walls) == 257
    keys = P.candidates(*P.case("open_tilted_ortho")[:3])[1]
    assert (keys[1:] == keys[:-1]).any() and (keys > 0).all(), "equal keys: the wall index decides"


def _walks_agree(sc, cam, w, h, S, proj, what):
    with np.errstate(all="ignore"):
        cw, cd = P.candidates(sc, cam, proj)
        src, d = P.rays(cam, w, h, S, proj)
        wall, dist, _ = T.walk(sc.walls, cw, cd, src, d)
        bwall, bdist = P.walk_brute(sc.walls, cw, src, d)
    assert np.array_equal(dist.view(np.uint32), bdist.view(np.uint32)), what
    assert np.array_equal(wall >= 0, bwall >= 0), what  # equal distance bits where the walls differ


@pytest.mark.parametrize("name", P.SHADE_CASES)
def test_walk_equals_brute_force(name):
    """The list's key bounds a hit's distance from below only up to rounding; the walk as written is the
    definition. On every case the GPU tests use, it finds what a walk of the whole list finds."""
    sc, cam, proj, w, h = P.case(name)
    for S in (1, 2, 3, 8):
        _walks_agree(sc, cam, w, h, S, proj, (name, S))
    if name.startswith("box8"):
        for ww, hh in ((1, 1), (1, 130), (130, 1)):
            _walks_agree(sc, cam, ww, hh, 3, proj, (name, ww, hh))
        for c in P.window_cams(proj):
            _walks_agree(sc, c, *P.WINDOW_SIZE, 2, proj, (name, "windows"))
        for c in (dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1)), ):  # the tools' tests
            _walks_agree(sc, fmgi.camera(pixel=0.1, **c), 32, 16, 3, proj, (name, "tool"))
    for cam in P.BATCH_CAMS:
        _walks_agree(P.scene("floor"), cam, *P.BATCH_SIZE, 3, proj, (name, "batch"))


@pytest.mark.parametrize("proj", P.PROJECTIONS)
@pytest.mark.parametrize("bilinear", [False, True])
def test_constant_colour_stays_constant(proj, bilinear):
    name = f"open_tilted_{proj}"
    sc, cam, _, w, h = P.case(name)
    tiles = np.tile(np.array(V.COLOUR, np.uint8), int(V._tile_counts(sc).sum()))
    r = P.shade(sc, cam, w, h, tiles, V.COLOUR, 3, bilinear, proj)
    assert np.all(r["rgb"] == np.array(V.COLOUR)) and 0 < int((r["coverage"] > 0).sum()) < w * h


# ---- the C ABI's argument checks ------------------------------------------------------------------------------

def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _geometry(sc):
    return fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))


def _shade(sc, cams, proj, width=4, height=4, tiles="yes", samples=1, filt=0, rgb=True):
    """(fmgi_shade_views_proj's return code, the old call's for the same arguments or None, the message)"""
    lib = _lib.load()
    g, keep = _geometry(sc)
    cams = np.atleast_1d(np.asarray(cams, fmgi.CAMERA_DTYPE))
    t = P.tiles("box8") if tiles == "yes" else None
    out, cov, bg = np.zeros((len(cams), 4, 4, 3), np.uint8), np.zeros((len(cams), 4, 4), np.uint8), np.zeros(3, np.uint8)
    rc = lib.fmgi_shade_views_proj(C.byref(g), _p(cams), len(cams), width, height, proj, _p(t), _p(bg), samples, filt,
                                   _p(out) if rgb else None, _p(cov))
    msg = _lib.last_error()
    old = None
    if proj == _lib.PROJ_PINHOLE:
        old = lib.fmgi_shade_views(C.byref(g), _p(cams), len(cams), width, height, _p(t), _p(bg), samples, filt,
                                   _p(out) if rgb else None, _p(cov))
        assert _lib.last_error() == msg
    assert not out.any() and not cov.any()
    return rc, old, msg


def _candidates(sc, cam, proj):
    lib = _lib.load()
    g, keep = _geometry(sc)
    cam = np.atleast_1d(np.asarray(cam, fmgi.CAMERA_DTYPE))
    idx, md = np.zeros(8, np.int32), np.zeros(8, f32)
    return lib.fmgi_view_candidates_proj(C.byref(g), _p(cam), proj, _p(idx), _p(md), 8), _lib.last_error()


def _create(sc, cams, proj, width=4, height=4, samples=1, filt=0):
    lib = _lib.load()
    g, keep = _geometry(sc)
    cams = np.atleast_1d(np.asarray(cams, fmgi.CAMERA_DTYPE))
    h = C.c_void_p(0x5A5A)
    rc = lib.fmgi_view_cache_create_proj(C.byref(g), _p(cams), len(cams), width, height, proj, samples, filt, C.byref(h))
    assert h.value is None, "*out is NULL after an error"
    return rc, _lib.last_error()


OK = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1), pixel=0.02)
PARALLEL = dict(OK, dir=(0, 0, -2), up=(0, 0, 1))


def _hidden(check):
    """run one of the checks below in a process that sees no device, so that an accepted call ends in
    FMGI_ERR_NO_DEVICE on any machine"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", f"import conftest, test_view_proj_host as H; H.{check}(); print('PASSED')"],
                       cwd=os.path.join(REPO, "tests"), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("PASSED"), r.stdout + r.stderr


def test_argument_errors_without_a_device():
    """every new FMGI_ERR_ARG case, in the stated order, before FMGI_ERR_NO_DEVICE"""
    _hidden("check_argument_errors")


def test_pinhole_errors_are_the_old_calls():
    _hidden("check_pinhole_errors")


def check_argument_errors():
    sc = T._scene("box8")
    ok, par = fmgi.camera(**OK), fmgi.camera(**PARALLEL)
    ORTHO, EQUI, PIN = _lib.PROJ_ORTHO, _lib.PROJ_EQUIRECT, _lib.PROJ_PINHOLE
    assert (PIN, ORTHO, EQUI) == (0, 1, 2)
    for bad in (3, -1, 7):
        for rc, msg in (_shade(sc, ok, bad)[::2], _candidates(sc, ok, bad), _create(sc, ok, bad)):
            assert rc == -3 and "projection" in msg, (bad, msg)
    for proj in (ORTHO, EQUI):
        for up in ((0, 0, 1), (0, 0, -3), (0, 0, 0), (np.nan, 0, 0), (np.inf, 1, 0)):
            cam = fmgi.camera(**dict(PARALLEL, up=up))
            for rc, msg in (_shade(sc, cam, proj)[::2], _candidates(sc, cam, proj), _create(sc, cam, proj)):
                assert rc == -3 and "cross(dir, up)" in msg, (proj, up, msg)
        assert _shade(sc, [ok, par], proj)[0] == -3 and _create(sc, [ok, par], proj)[0] == -3, "any camera of a batch"
    assert _shade(sc, par, PIN)[:2] == (-1, -1), "the pin-hole takes up as given: the call gets as far as the device"
    # the pixel size: metres per pixel for ORTHO, not read for EQUIRECT
    for pixel in (0.0, -0.01, np.inf, np.nan):
        cam = fmgi.camera(**dict(OK, pixel=pixel))
        for rc, msg in (_shade(sc, cam, ORTHO)[::2], _candidates(sc, cam, ORTHO), _create(sc, cam, ORTHO)):
            assert rc == -3 and "pixel" in msg, pixel
        for rc, msg in (_shade(sc, cam, EQUI)[::2], _candidates(sc, cam, EQUI), _create(sc, cam, EQUI)):
            assert rc == -1, (pixel, msg)  # FMGI_ERR_NO_DEVICE: every argument was accepted
    # the order: the existing checks first and in their order, then the projection, then the frame
    badpix_par = fmgi.camera(**dict(PARALLEL, pixel=0))
    assert "pixel" in _shade(sc, badpix_par, ORTHO)[2] and "pixel" in _shade(sc, badpix_par, 9)[2]
    assert "cross" in _shade(sc, badpix_par, EQUI)[2]
    assert "direction" in _shade(sc, fmgi.camera(**dict(OK, dir=(0, 0, 0))), EQUI)[2]
    assert "direction" in _shade(sc, [ok, fmgi.camera(**dict(OK, dir=(0, 0, 0)))], 9)[2]
    assert "projection" in _shade(sc, par, 9)[2]
    assert "samples" in _shade(sc, par, 9, samples=9)[2] and "filter" in _shade(sc, par, ORTHO, filt=2)[2]
    assert "tiles_rgb" in _shade(sc, par, EQUI, tiles=None)[2] and "image size" in _shade(sc, par, 9, width=0)[2]
    assert "samples" in _create(sc, par, 9, samples=0)[1] and "image size" in _create(sc, par, EQUI, height=0)[1]
    lib = _lib.load()
    g, keep = _geometry(sc)
    assert lib.fmgi_view_cache_create_proj(C.byref(g), _p(np.atleast_1d(par)), 1, 4, 4, 9, 1, 0, None) == -3
    assert "null out" in _lib.last_error()
    assert lib.fmgi_view_candidates_proj(C.byref(g), None, ORTHO, None, None, 0) == -3
    assert lib.fmgi_view_cache_projection(None) == -3
    # every argument accepted: the missing device is what is left
    for proj in (PIN, ORTHO, EQUI):
        assert _shade(sc, ok, proj)[0] == -1 and _candidates(sc, ok, proj)[0] == -1 and _create(sc, ok, proj)[0] == -1
        assert _shade(sc, np.zeros(0, fmgi.CAMERA_DTYPE), proj)[0] == 0, "no cameras: nothing to do"


def check_pinhole_errors():
    sc = T._scene("box8")
    ok = fmgi.camera(**OK)
    seen = set()
    for kw in (dict(samples=0), dict(samples=9), dict(filt=2), dict(tiles=None), dict(width=0), dict(height=-1), {}):
        rc, old, msg = _shade(sc, ok, _lib.PROJ_PINHOLE, **kw)
        assert rc == old, kw
        seen.add(rc)
    for cam in (dict(OK, pixel=0), dict(OK, pixel=np.nan), dict(OK, dir=(0, 0, 0))):
        rc, old, msg = _shade(sc, fmgi.camera(**cam), _lib.PROJ_PINHOLE)
        assert rc == old == -3
        lib = _lib.load()
        g, keep = _geometry(sc)
        c = np.atleast_1d(fmgi.camera(**cam))
        assert _candidates(sc, c, _lib.PROJ_PINHOLE)[0] == lib.fmgi_view_candidates(C.byref(g), _p(c), None, None, 0) == -3
        h = C.c_void_p()
        assert _create(sc, c, _lib.PROJ_PINHOLE)[0] == lib.fmgi_view_cache_create(C.byref(g), _p(c), 1, 4, 4, 1, 0, C.byref(h)) == -3
    assert seen == {-3, -1}


def test_python_keywords():
    sc = T._scene("box8")
    with pytest.raises(fmgi.FmgiError, match="projection"):
        fmgi.shade_views(sc, fmgi.camera(**OK), 4, 4, projection="fisheye")
    with pytest.raises(fmgi.FmgiError, match="projection"):
        fmgi.view_candidates(sc, fmgi.camera(**OK), projection="cube")
    with pytest.raises(fmgi.FmgiError, match="projection"):
        fmgi.ViewCache(sc, fmgi.camera(**OK), 4, 4, projection=1)
    with pytest.raises(fmgi.FmgiError, match="cross"):
        fmgi.shade_views(sc, fmgi.camera(**PARALLEL), 4, 4, projection="ortho")
    with pytest.raises(TypeError):
        fmgi.shade_views(sc, fmgi.camera(**OK), 4, 4, None, (0, 0, 0), 1, "nearest", "ortho")  # keyword only
    assert fmgi.PROJECTIONS == {"pinhole": 0, "ortho": 1, "equirect": 2}
    for name in ("fmgi_shade_views_proj", "fmgi_view_candidates_proj", "fmgi_view_cache_create_proj",
                 "fmgi_view_cache_projection"):
        assert name in _lib.EXPORTS


def test_no_device_is_an_error_code(tmp_path):
    """Without a device the three calls return FMGI_ERR_NO_DEVICE and the process lives on."""
    prog = tmp_path / "nogpu_proj.py"
    prog.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import fmgi\n"
        "from fmgi import scene\n"
        "sc = scene.box_scene(8, tile_size=1.0)\n"
        "cam = fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), pixel=0.02)\n"
        "for call in (lambda: fmgi.shade_views(sc, cam, 8, 8, samples=2, filter='bilinear', projection='equirect'),\n"
        "             lambda: fmgi.view_candidates(sc, cam, projection='ortho'),\n"
        "             lambda: fmgi.ViewCache(sc, cam, 8, 8, projection='ortho')):\n"
        "    try:\n"
        "        call()\n"
        "    except fmgi.FmgiError as e:\n"
        "        print('ERR', e)\n"
        "print('ALIVE')\n" % PKG
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 4 and lines[3] == "ALIVE"
    assert "fmgi_shade_views_proj failed (-1)" in lines[0] and "fmgi_view_candidates_proj failed (-1)" in lines[1]
    assert "fmgi_view_cache_create_proj failed (-1)" in lines[2]


# ---- the tools' argument handling -----------------------------------------------------------------------------

def test_tools_take_the_projection_flag(capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
        import relight_radiosity
        import render_view
    finally:
        sys.path.pop(0)
    for tool in (relight, relight_radiosity):
        base = ["box200", "--scenarios", "s.json"] + (["--spa", "1000"] if tool is relight else [])
        assert tool.parse_args(base).projection == "pinhole"
        for p in ("pinhole", "ortho", "equirect"):
            assert tool.parse_args(base + ["--view", "--projection", p]).projection == p
        with pytest.raises(SystemExit):
            tool.parse_args(base + ["--projection", "fisheye"])
    with pytest.raises(SystemExit):
        render_view.main(["box8", "--projection", "fisheye"])
    assert "invalid choice: 'fisheye'" in capsys.readouterr().err
    for tool in ("bench_view.py", "bench_view_cache.py", "render_view.py"):
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", tool), "--help"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and "--projection" in r.stdout, tool
