"""CPU tests of the direct-sun layer (fmgi_sun_*): the argument checks in their order on a host-only
context, fmgi_sun_units against the restatement, the restatement's own conditions (what makes each case a test),
the energy of a fully lit texel, fmgi.sun_vector and the scenario parser of tools/relight.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fmgi
import sun_restate as R
from conftest import REPO
from fmgi import _lib

sys.path.insert(0, os.path.join(REPO, "tools"))

NO_DEVICE, ARG, STATE = -1, -3, -4
F3 = C.c_float * 3
SUN = F3(0.3, -1.0, 0.8)
RGB = F3(18.0, 18.0, 18.0)
P = C.c_void_p(64)  # a non-NULL "device" pointer: the checks end before anything reads it


def _ctx(sc=None):
    lib = _lib.load()
    h = lib.fmgi_create(fmgi.HOST_ONLY)
    assert h
    keep = None
    if sc is not None:
        keep = [np.ascontiguousarray(a) for a in (sc.walls, sc.windows, sc.lights)]
        p = [a.ctypes.data_as(C.c_void_p) if len(a) else None for a in keep]
        assert lib.fmgi_set_scene(h, p[0], len(keep[0]), p[1], len(keep[1]), p[2], len(keep[2]), sc.num_texels) == 0
    return lib, h, keep


def test_coverage_argument_errors_in_order():
    sc, _ = R.case("box")
    lib, h, keep = _ctx()
    try:
        cov = lambda *a: lib.fmgi_sun_coverage(*a)  # noqa: E731
        assert cov(None, SUN, 2, 0, P, None) == ARG
        assert cov(h, None, 2, 0, P, None) == ARG
        assert cov(h, SUN, 2, 0, None, None) == ARG
        for samples in (0, 9, -1):
            assert cov(h, SUN, samples, 0, P, None) == ARG and "samples" in _lib.last_error()
        for mode in (-1, 2):
            assert cov(h, SUN, 2, mode, P, None) == ARG and "mode" in _lib.last_error()
        for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0), (3e38, 3e38, 0), (1e-30, 0, 0)):
            assert cov(h, F3(*bad), 2, 0, P, None) == ARG and "to_sun" in _lib.last_error()
        # the argument errors come before the missing scene, the missing scene before the missing device
        assert cov(h, SUN, 9, 0, P, None) == ARG
        assert cov(h, SUN, 2, 0, P, None) == STATE
        st = _lib.SunStats()
        assert lib.fmgi_sun_get_stats(h, None) == ARG and lib.fmgi_sun_get_stats(None, C.byref(st)) == ARG
    finally:
        lib.fmgi_destroy(h)
    lib, h, keep = _ctx(sc)
    try:
        assert lib.fmgi_sun_coverage(h, SUN, 0, 0, P, None) == ARG
        assert lib.fmgi_sun_coverage(h, SUN, 2, 0, P, None) == NO_DEVICE
        assert lib.fmgi_sun_coverage(h, SUN, 8, 1, P, None) == NO_DEVICE
    finally:
        lib.fmgi_destroy(h)


def test_add_and_units_argument_errors_in_order():
    sc, _ = R.case("box")
    lms = (C.c_void_p * 2)(64, 64)
    rgb2 = (C.c_float * 6)(1, 2, 3, 4, 5, 6)
    lib, h, keep = _ctx()
    try:
        add = lambda *a: lib.fmgi_sun_add(*a)  # noqa: E731
        ok = (h, P, SUN, 2, rgb2, 2, 1000.0, lms, None)

        def but(i, v):
            return ok[:i] + (v,) + ok[i + 1:]

        for i in (0, 1, 2, 4, 7):
            assert add(*but(i, None)) == ARG
        assert add(*but(7, (C.c_void_p * 2)(64, None))) == ARG
        for samples in (0, 9):
            assert add(*but(3, samples)) == ARG and "samples" in _lib.last_error()
        assert add(*but(2, F3(0, 0, 0))) == ARG and "to_sun" in _lib.last_error()
        for n in (0, -1):
            assert add(*but(5, n)) == ARG and "num_maps" in _lib.last_error()
        for bad in (32.0, -1.0, np.nan, np.inf):
            assert add(*but(4, (C.c_float * 6)(1, 2, 3, 4, bad, 6))) == ARG and "rgb" in _lib.last_error()
        for bad in (0.0, -1.0, np.nan, np.inf):
            assert add(*but(6, bad)) == ARG and "flux" in _lib.last_error()
        assert add(*but(6, 0.0)) == ARG  # before the missing scene
        assert add(*ok) == STATE
        out = np.zeros((len(sc.walls), 3), np.int64)
        po = out.ctypes.data_as(C.c_void_p)
        assert lib.fmgi_sun_units(None, SUN, RGB, 1.0, po) == ARG
        assert lib.fmgi_sun_units(h, None, RGB, 1.0, po) == ARG
        assert lib.fmgi_sun_units(h, SUN, None, 1.0, po) == ARG
        assert lib.fmgi_sun_units(h, SUN, RGB, 1.0, None) == ARG
        assert lib.fmgi_sun_units(h, F3(0, 0, 0), RGB, 1.0, po) == ARG
        assert lib.fmgi_sun_units(h, SUN, F3(1, 2, 32), 1.0, po) == ARG
        assert lib.fmgi_sun_units(h, SUN, RGB, -1.0, po) == ARG
        assert lib.fmgi_sun_units(h, SUN, RGB, 1.0, po) == STATE
    finally:
        lib.fmgi_destroy(h)
    lib, h, keep = _ctx(sc)
    try:
        ok = (h, P, SUN, 2, rgb2, 2, 1000.0, lms, None)
        # a unit of 2^55 or more: the floor's texel is 10 * 8 / 2048 m^2, so 31 * c_w * flux * area * 2^25 passes it
        huge = 1e12
        assert float(R.units(sc, (0.3, -1.0, 0.8), (1, 2, 3), huge).max()) >= 2.0 ** 55
        assert lib.fmgi_sun_add(*(ok[:6] + (huge,) + ok[7:])) == ARG and "2^55" in _lib.last_error()
        out = np.zeros((len(sc.walls), 3), np.int64)
        assert lib.fmgi_sun_units(h, SUN, F3(1, 2, 3), huge, out.ctypes.data_as(C.c_void_p)) == ARG
        assert lib.fmgi_sun_add(*(ok[:5] + (0,) + ok[6:])) == ARG  # argument errors still first
        assert lib.fmgi_sun_add(*ok) == NO_DEVICE  # last
    finally:
        lib.fmgi_destroy(h)


@pytest.mark.parametrize("name", ["box", "box_level", "tilted12", "skylight", "example", "ragged"])
def test_units_equal_restatement(name):
    sc, to_sun = R.case(name)
    ctx = fmgi.Context(fmgi.HOST_ONLY)
    try:
        ctx.set_scene(sc)
        for rgb, flux in (((18, 18, 18), 65000.0), ((30.5, 28.25, 0.0), 6500000.0), ((0.1, 0.7, 31.99), 123.456)):
            got = ctx.sun_units(to_sun, rgb, flux)
            exp = R.units(sc, to_sun, rgb, flux)
            assert got.shape == exp.shape and np.array_equal(got, exp)
            facing = R.facing_cos(sc, to_sun) > 0
            assert not got[~facing].any() and (got[facing][:, 2 if rgb[2] else 0] > 0).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_conditions(name):
    """caps, not measurements: what makes each case the test it is named for"""
    sc, to_sun = R.case(name)
    for S in R.SAMPLES[name]:
        r = R.restate(name, S)
        level0 = sum(int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls)
        assert r["samples"] == level0 * S * S and r["cover"].shape == (sc.num_texels,)
        assert int(r["cover"].sum()) == r["lit"] <= r["crossing"] <= r["facing"] <= r["samples"]
        assert int(r["cover"].max(initial=0)) <= S * S and not r["cover"][~sc.level0_mask()].any()
        if name in R.POSITIVE:
            assert 0 < r["lit"] < r["facing"]
        if name in R.ZERO:
            assert r["crossing"] == 0 and r["facing"] > 0
        if name in ("crossing", "example", "tilted12", "open_tilted"):
            assert r["lit"] < r["crossing"]  # interior walls, reveals and panels block
        if name == "outside":
            assert r["crossing"] > 0 and r["lit"] == 0  # every ray meets a wall before the window: dw as `closest`
    c = R.facing_cos(sc, to_sun)
    if name == "box_level":
        assert c[0] == 0 and R.restate(name, 2)["cover"][:int(sc.walls[0]["lm"][1]) * int(sc.walls[0]["lm"][2])].sum() == 0
        assert R.restate(name, 2)["lit"] > 0  # the far wall is lit
    if name == "box_skew":  # the patch runs up the x = 10 wall (n = -x)
        side = [k for k, w in enumerate(sc.walls) if w["n"][0] < -0.5]
        assert len(side) == 1
        s0, n = int(sc.walls[side[0]]["lm"][0]), int(sc.walls[side[0]]["lm"][1]) * int(sc.walls[side[0]]["lm"][2])
        assert R.restate(name, 2)["cover"][s0:s0 + n].any() and R.restate(name, 2)["cover"][:2048].any()
    if name == "ragged":
        first = int(np.flatnonzero(c > 0)[0])
        assert first == 0 and tuple(sc.walls[0]["lm"][1:3]) == (1, 1)
        texels = R.restate(name, 1)["facing"]
        assert texels % 7 and texels % 16
    if name in ("tilted12", "open_tilted"):  # off-axis receivers: a panel is lit
        lit = [k for k, w in enumerate(sc.walls) if np.count_nonzero(np.abs(w["n"][:3]) > 1e-3) > 1 and
               R.restate(name, 2)["cover"][int(w["lm"][0]):int(w["lm"][0]) + int(w["lm"][1]) * int(w["lm"][2])].any()]
        assert lit


@pytest.mark.parametrize("name", ["box", "box_skew", "skylight", "example"])
def test_fully_lit_texel_gains_035_rgb_cosine(name):
    sc, to_sun = R.case(name)
    S = 2
    cover = R.restate(name, S)["cover"]
    rgb, spa = (30.0, 28.0, 24.0), 65000
    lm = R.add(sc, cover, to_sun, S, rgb, float(spa), np.zeros((sc.num_texels, 4), np.int64))
    tex = R.finalize(sc, lm, spa)
    c = R.facing_cos(sc, to_sun)
    full = 0
    for k, w in enumerate(sc.walls):
        s0, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        t = np.flatnonzero(cover[s0:s0 + n] == S * S)
        if len(t):
            exp = 0.35 * np.array(rgb, np.float64) * float(c[k])
            got = tex[s0 + t].astype(np.float64)
            assert np.all(np.abs(got - exp) <= 1e-5 * exp), (name, k)
            full += len(t)
    assert full > 0
    assert not lm[:, 3].any() and not lm[cover == 0].any()


def test_sun_vector():
    for (az, el), exp in {(0, 0): (0, 1, 0), (90, 0): (1, 0, 0), (180, 0): (0, -1, 0), (270, 0): (-1, 0, 0),
                          (0, 90): (0, 0, 1), (123, 90): (0, 0, 1)}.items():
        v = fmgi.sun_vector(az, el)
        assert v.dtype == np.float32 and v.shape == (3,)
        assert np.allclose(v, exp, rtol=0, atol=1e-7), (az, el, v)
    v = fmgi.sun_vector(200.0, 35.0).astype(np.float64)
    a, e = np.radians(200.0), np.radians(35.0)
    assert np.allclose(v, (np.sin(a) * np.cos(e), np.cos(a) * np.cos(e), np.sin(e)), rtol=0, atol=1e-7)
    assert v[0] < 0 and v[1] < 0 and v[2] > 0  # south-south-west, above the horizon


def test_relight_scenario_parser():
    import relight

    assert relight.sun_of({"name": "plain", "windows": {"scale": 0.5}}) is None
    to_sun, rgb = relight.sun_of({"name": "a", "sun": {"azimuth": 200, "elevation": 35, "rgb": [30, 28, 24]}})
    assert to_sun.dtype == np.float32 and np.array_equal(to_sun, fmgi.sun_vector(200, 35)) and rgb == [30.0, 28.0, 24.0]
    to_sun, rgb = relight.sun_of({"name": "b", "sun": {"to_sun": [0.3, -1, 0.8], "rgb": [1, 2, 3.5]}})
    assert np.array_equal(to_sun, np.array([0.3, -1, 0.8], np.float32)) and rgb == [1.0, 2.0, 3.5]
    bad = {"not an object": 3,
           "needs azimuth": {"rgb": [1, 2, 3]},
           "needs rgb": {"azimuth": 1, "elevation": 2},
           "not both": {"to_sun": [0, 1, 0], "azimuth": 3, "elevation": 4, "rgb": [1, 2, 3]},
           "no length": {"to_sun": [0, 0, 0], "rgb": [1, 2, 3]},
           "3 finite": {"to_sun": [0, 1], "rgb": [1, 2, 3]},
           "[0, 32)": {"to_sun": [0, 1, 0], "rgb": [1, 2, 32]},
           "finite number": {"azimuth": "south", "elevation": 4, "rgb": [1, 2, 3]},
           "keys": {"to_sun": [0, 1, 0], "rgb": [1, 2, 3], "colour": 1}}
    texts = {"not an object": "must be an object", "needs azimuth": "needs azimuth and elevation", "needs rgb": "needs rgb",
             "not both": "not both", "no length": "no length", "3 finite": "3 finite numbers", "[0, 32)": "[0, 32)",
             "finite number": "1 finite number", "keys": "colour"}
    for what, spec in bad.items():
        with pytest.raises(SystemExit) as e:
            relight.sun_of({"name": "x", "sun": spec})
        assert texts[what] in str(e.value) and "'x'" in str(e.value), (what, str(e.value))
    a = relight.parse_args(["box8", "--spa", "1000", "--scenarios", "s.json"])
    assert a.sun_samples == 4
    assert relight.parse_args(["box8", "--spa", "1000", "--scenarios", "s.json", "--sun-samples", "8"]).sun_samples == 8
    with pytest.raises(SystemExit):
        relight.parse_args(["box8", "--spa", "1000", "--scenarios", "s.json", "--sun-samples", "9"])
