"""Traced views (fmgi_view_cache_* / fmgi.ViewCache): what the host decides without a device.

  the new names are exported; the size of the records
  fmgi_view_cache_create reports fmgi_shade_views' argument errors in its order, and its own, before a device is
  looked for; without a device it returns FMGI_ERR_NO_DEVICE and the process lives on
  destroy(NULL) returns; info, tiles and shade refuse a NULL handle
  tools/relight.py's arguments for --view are what they were
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import fmgi
import test_view_shade as V
from conftest import PKG, REPO
from fmgi import _lib

f32 = np.float32
NEW = ("fmgi_view_cache_bytes", "fmgi_view_cache_create", "fmgi_view_cache_destroy", "fmgi_view_cache_info",
       "fmgi_view_cache_tiles", "fmgi_view_cache_shade")


def test_new_names_are_exported():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and getattr(lib, name)
    assert _lib.VIEW_CACHE_MAX_SETS == fmgi.VIEW_CACHE_MAX_SETS == 8
    assert C.sizeof(_lib.ViewCacheInfo) == 80
    assert callable(fmgi.ViewCache) and callable(fmgi.view_cache_bytes)
    with open(os.path.join(REPO, "include", "flatmatch_gi.h")) as f:
        header = f.read()
    assert "#define FMGI_VIEW_CACHE_MAX_SETS 8" in header and all(name + "(" in header for name in NEW)


def test_record_bytes():
    lib = _lib.load()
    assert lib.fmgi_view_cache_bytes(1, 24, 20, 3, _lib.VIEW_NEAREST) == 17_280
    assert lib.fmgi_view_cache_bytes(2, 40, 30, 8, _lib.VIEW_BILINEAR) == 2_457_600
    assert fmgi.view_cache_bytes(1, 24, 20, 3) == 17_280
    assert fmgi.view_cache_bytes(2, 40, 30, 8, "bilinear") == 2_457_600
    for cams, width, samples, filt in ((1, 24, 0, 0), (1, 24, 9, 0), (1, 24, 3, 2), (1, 0, 3, 0), (0, 24, 3, 0)):
        assert lib.fmgi_view_cache_bytes(cams, width, 20, samples, filt) == 0, (cams, width, samples, filt)


def _create(sc, cams, width, height, samples=1, filt=0, n=None, out=True):
    """fmgi_view_cache_create through ctypes with explicit arguments; (return code, the handle left in *out)"""
    lib = _lib.load()
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    n = len(cams) if n is None else n
    h = C.c_void_p()
    rc = lib.fmgi_view_cache_create(C.byref(g), None if cams is None else cams.ctypes.data_as(C.c_void_p), n, width,
                                    height, samples, filt, C.byref(h) if out else None)
    return rc, h.value


def test_create_argument_errors_without_a_device():
    """test_view_shade.test_argument_errors_without_a_device's cases in its order, then the cache's own; every one
    is FMGI_ERR_ARG under the function's name and leaves *out NULL"""
    sc = V._scene("box8_C")
    cams = np.atleast_1d(V._cam("box8_C"))
    fn = "fmgi_view_cache_create"
    for samples in (0, 9, -1):
        assert _create(sc, cams, 4, 4, samples, 0) == (-3, None), samples
        assert "samples" in _lib.last_error() and fn in _lib.last_error()
    for filt in (2, -1):
        assert _create(sc, cams, 4, 4, 1, filt) == (-3, None), filt
        assert "filter" in _lib.last_error() and fn in _lib.last_error()
    assert _create(sc, cams, 0, 4) == (-3, None)  # inherited from fmgi_render_views
    assert "image size" in _lib.last_error() and fn in _lib.last_error()
    bad = cams.copy()
    bad["pixel"] = 0
    assert _create(sc, bad, 4, 4) == (-3, None)
    assert "pixel" in _lib.last_error() and fn in _lib.last_error()
    # the order of fmgi_shade_views: the image before the cameras before samples before filter before a camera
    assert _create(sc, bad, 0, 4, 0, 2)[0] == -3 and "image size" in _lib.last_error()
    assert _create(sc, bad, 4, 4, 0, 2, n=0)[0] == -3 and "cameras" in _lib.last_error()
    assert _create(sc, bad, 4, 4, 0, 2)[0] == -3 and "samples" in _lib.last_error()
    assert _create(sc, bad, 4, 4, 1, 2)[0] == -3 and "filter" in _lib.last_error()
    # the cache's own
    assert _create(sc, cams, 4, 4, n=0) == (-3, None)
    assert "cameras" in _lib.last_error() and fn in _lib.last_error()
    assert _create(sc, None, 4, 4, n=1) == (-3, None)
    assert "cameras" in _lib.last_error()
    assert _create(sc, cams, 4, 4, out=False) == (-3, None)
    assert "out" in _lib.last_error() and fn in _lib.last_error()
    try:
        fmgi.ViewCache(sc, cams, 4, 4, filter="cubic")
    except fmgi.FmgiError as e:
        assert "filter" in str(e)
    else:
        raise AssertionError("filter 'cubic' was accepted")


def test_null_handles():
    lib = _lib.load()
    assert lib.fmgi_view_cache_destroy(None) is None
    info = _lib.ViewCacheInfo()
    assert lib.fmgi_view_cache_info(None, C.byref(info)) == -3 and "fmgi_view_cache_info" in _lib.last_error()
    one = (C.c_void_p * 1)(C.c_void_p(64))
    bg = (C.c_uint8 * 3)(1, 2, 3)
    assert lib.fmgi_view_cache_tiles(None, one, 1, 0, 0, one, None) == -3
    assert "fmgi_view_cache_tiles" in _lib.last_error()
    assert lib.fmgi_view_cache_shade(None, one, 1, bg, one, None, None) == -3
    assert "fmgi_view_cache_shade" in _lib.last_error()


def test_no_device_is_an_error_code(tmp_path):
    """Without a device fmgi_view_cache_create returns FMGI_ERR_NO_DEVICE and the process lives on."""
    prog = tmp_path / "nogpu_view_cache.py"
    prog.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import fmgi\n"
        "from fmgi import scene\n"
        "sc = scene.box_scene(8, tile_size=1.0)\n"
        "cam = fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), pixel=0.02)\n"
        "try:\n"
        "    fmgi.ViewCache(sc, cam, 8, 8, samples=2, filter='bilinear')\n"
        "except fmgi.FmgiError as e:\n"
        "    print('ERR', e)\n"
        "print('ALIVE')\n" % PKG
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[1] == "ALIVE"
    assert "fmgi_view_cache_create failed (-1)" in lines[0]


def test_relight_view_arguments_are_unchanged(monkeypatch):
    """--view and its camera arguments: the names, defaults and help texts the tool had before it traced views"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
    finally:
        sys.path.pop(0)
    a = relight.parse_args(["box8", "--spa", "1", "--scenarios", "s.json"])
    assert a.view is False
    a = relight.parse_args(["box8", "--spa", "1", "--scenarios", "s.json", "--view"])  # no camera argument is required
    assert a.view is True
    assert (tuple(a.pos), tuple(a.dir), tuple(a.up), a.pixel) == ((5, 5.2, 1.6), (1, 1, 0), (0, 0, 1), 0.001)
    assert (a.width, a.height, tuple(a.background), a.samples, a.filter) == (1024, 768, (0, 0, 0), 2, "bilinear")
    monkeypatch.setenv("COLUMNS", "200")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "relight.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0
    for line in ("--view                also write OUT/<name>/view.ppm", "--pos POS POS POS", "--dir DIR DIR DIR",
                 "--up UP UP UP", "--pixel PIXEL", "--width WIDTH", "--height HEIGHT",
                 "--background BACKGROUND BACKGROUND BACKGROUND", "--samples SAMPLES     N x N rays per pixel (1..8)",
                 "--filter {nearest,bilinear}",
                 "With --view a camera picture (fmgi.shade_views) goes to OUT/<name>/view.ppm."):
        assert line in r.stdout, line
