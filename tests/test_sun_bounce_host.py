"""CPU tests of the bounced-sun layer (fmgi_rad_cache_sun_bounce / fmgi_sun_add_bounced): the
restatement's own conditions on the oracle's form factors (what makes each case a test), its independence of the other
directions, the argument checks of fmgi_sun_add_bounced in their order on a host-only context, the bound its 2^55
check rests on, and the new options of tools/relight.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fmgi
import rad_cache_cases as CASES
import sun_bounce_restate as B
import sun_restate as SR
from conftest import REPO
from fmgi import _lib

sys.path.insert(0, os.path.join(REPO, "tools"))

f32 = np.float32
NO_DEVICE, ARG, STATE = -1, -3, -4
P = C.c_void_p(64)  # a non-NULL "device" pointer: the checks end before anything reads it
N = 3

_rows = {}


def _restated(libc, name):
    """(scene, cover at S = 2, float32 [N, numTexels]) of a case on the oracle's ids"""
    if name not in _rows:
        key, sc, to_sun = B.case(name)
        sids = CASES.oracle(libc, key)[2]
        g = B.bounce(sc, sids, [B.cover(name, 2)], [to_sun], [2], N)[0]
        g.setflags(write=False)
        _rows[name] = (sc, B.cover(name, 2), g)
    return _rows[name]


def test_new_names_are_exported():
    lib = _lib.load()
    for name in ("fmgi_rad_cache_sun_bounce", "fmgi_sun_add_bounced"):
        assert name in _lib.EXPORTS and getattr(lib, name)
    assert _lib.SUN_BOUNCE_MAX_DIRS == fmgi.SUN_BOUNCE_MAX_DIRS == 32
    assert _lib.SUN_MAX_BOUNCES == fmgi.SUN_MAX_BOUNCES == 8
    assert callable(fmgi.RadCache.sun_bounce) and callable(fmgi.Context.sun_add_bounced)
    with open(os.path.join(REPO, "include", "flatmatch_gi.h")) as f:
        header = f.read()
    assert "#define FMGI_SUN_BOUNCE_MAX_DIRS 32" in header and "#define FMGI_SUN_MAX_BOUNCES 8" in header
    assert "fmgi_rad_cache_sun_bounce(" in header and "fmgi_sun_add_bounced(" in header


@pytest.mark.parametrize("name", B.POSITIVE)
def test_restatement_conditions(libc, name):
    """lit texels, some of them partly covered, and first-bounce light on at least half of the jobs"""
    sc, cover, g = _restated(libc, name)
    jobs = B.R.job_texels(sc)
    lit, partly = int((cover > 0).sum()), int(((cover > 0) & (cover < 4)).sum())
    reached = int((g[0][jobs] > 0).sum())
    print(name, "lit", lit, "partly covered", partly, "jobs with g_1 > 0:", reached, "of", len(jobs))
    assert lit > 0 and partly > 0
    assert 2 * reached >= len(jobs)
    off = np.ones(sc.num_texels, bool)
    off[jobs] = False
    assert off.any() and not g[:, off].view(np.uint32).any()  # +0 at every texel that is no job's
    assert (g >= 0).all() and (g <= f32(1.001)).all()        # what fmgi_sun_add_bounced's 2^55 check rests on
    assert (g[1][jobs] > 0).sum() >= reached and not np.array_equal(g[0], g[1])  # light spreads with every bounce
    if name == "open_tilted":
        sids = CASES.oracle(libc, "open_tilted")[2]
        assert 0.40 < (sids < 0).mean() < 0.46  # the rays that miss add nothing


def test_sun_behind_the_window_wall_gives_zero_tables(libc):
    sc, cover, g = _restated(libc, "box_lit_behind")
    assert not cover.any() and (SR.facing_cos(sc, B.case("box_lit_behind")[2]) > 0).any()
    assert g.shape == (N, sc.num_texels) and not g.view(np.uint32).any()


def test_a_direction_alone_equals_it_among_others(libc):
    key, sc, d0 = B.case("box_lit")
    d1 = B.case("box_lit_skew")[2]
    sids = CASES.oracle(libc, key)[2]
    both = B.bounce(sc, sids, [B.cover("box_lit", 2), B.cover("box_lit_skew", 3)], [d0, d1], [2, 3], 2)
    assert np.array_equal(both[0].view(np.uint32), _restated(libc, "box_lit")[2][:2].view(np.uint32))
    alone = B.bounce(sc, sids, [B.cover("box_lit_skew", 3)], [d1], [3], 2)
    assert np.array_equal(both[1].view(np.uint32), alone[0].view(np.uint32))
    assert not np.array_equal(both[0], both[1])


def test_start_table_ignores_what_no_facing_wall_owns():
    """bytes on walls that do not face the sun, on mip texels: +0; a byte above S * S is used as it is"""
    _, sc, to_sun = B.case("box_lit")
    cover = np.full(sc.num_texels, 9, np.uint8)
    e = B.start_table(sc, cover, to_sun, 2)
    c = SR.facing_cos(sc, to_sun)
    assert (c > 0).any() and (~(c > 0)).any()
    for k, w in enumerate(sc.walls):
        s0, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        want = (f32(9) * c[k]) / f32(4) if c[k] > 0 else f32(0)
        assert (e[s0:s0 + n] == want).all()
    assert not e[:sc.num_texels][~sc.level0_mask()].any() and not e[sc.num_texels:].any() and len(e) > sc.num_texels


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


def test_add_bounced_argument_errors_in_order():
    sc = CASES.get_scene("box_lit")
    lms = (C.c_void_p * 2)(64, 64)
    rgb2 = (C.c_float * 6)(1, 2, 3, 4, 5, 6)
    refl2 = (C.c_float * 6)(0.9, 0.9, 0.9, 1.0, 0.5, 0.0)
    lib, h, keep = _ctx()
    try:
        add = lambda *a: lib.fmgi_sun_add_bounced(*a)  # noqa: E731
        ok = (h, P, 2, rgb2, refl2, 2, 1000.0, lms, None)

        def but(i, v):
            return ok[:i] + (v,) + ok[i + 1:]

        for i in (0, 1, 3, 4, 7):
            assert add(*but(i, None)) == ARG
        assert add(*but(7, (C.c_void_p * 2)(64, None))) == ARG
        for n in (0, 9, -1):
            assert add(*but(2, n)) == ARG and "bounces" in _lib.last_error()
        for n in (0, -1):
            assert add(*but(5, n)) == ARG and "num_maps" in _lib.last_error()
        for bad in (32.0, -1.0, np.nan, np.inf):
            assert add(*but(3, (C.c_float * 6)(1, 2, 3, 4, bad, 6))) == ARG and "rgb" in _lib.last_error()
        for bad in (1.5, -0.1, np.nan, np.inf):
            assert add(*but(4, (C.c_float * 6)(0.9, 0.9, 0.9, 1.0, bad, 0.0))) == ARG and "refl" in _lib.last_error()
        for bad in (0.0, -1.0, np.nan, np.inf):
            assert add(*but(6, bad)) == ARG and "flux" in _lib.last_error()
        assert add(*but(2, 9)[:5] + (0,) + ok[6:]) == ARG and "bounces" in _lib.last_error()  # in the stated order
        assert add(*but(6, 0.0)) == ARG  # before the missing scene
        assert add(*ok) == STATE
    finally:
        lib.fmgi_destroy(h)
    lib, h, keep = _ctx(sc)
    try:
        ok = (h, P, 2, rgb2, refl2, 2, 1000.0, lms, None)
        # the largest flux the bound lets through for 2 bounces, and the next one up
        big = 2.0 ** 55 / B.bound(sc, 2, 1.0)
        assert B.bound(sc, 2, big * 1.01) >= 2.0 ** 55 > B.bound(sc, 2, big * 0.99)
        assert lib.fmgi_sun_add_bounced(*(ok[:6] + (big * 1.01,) + ok[7:])) == ARG and "2^55" in _lib.last_error()
        assert lib.fmgi_sun_add_bounced(*(ok[:6] + (big * 0.99,) + ok[7:])) == NO_DEVICE
        assert B.bound(sc, 8, big * 0.99) >= 2.0 ** 55  # the bound grows with the bounces
        assert lib.fmgi_sun_add_bounced(*((h, P, 8) + ok[3:6] + (big * 0.99,) + ok[7:])) == ARG
        assert lib.fmgi_sun_add_bounced(*(ok[:5] + (0,) + ok[6:])) == ARG  # argument errors still first
        assert lib.fmgi_sun_add_bounced(*ok) == NO_DEVICE  # last
    finally:
        lib.fmgi_destroy(h)


def test_sun_bounce_argument_errors_without_a_handle():
    lib = _lib.load()
    one = (C.c_void_p * 1)(64)
    d = (C.c_float * 3)(0.3, -1.0, 0.8)
    s = (C.c_int * 1)(2)
    assert lib.fmgi_rad_cache_sun_bounce(None, one, d, s, 1, 2, one, None) == ARG
    assert "fmgi_rad_cache_sun_bounce" in _lib.last_error()


def test_restated_add(libc):
    sc, _, g = _restated(libc, "box_lit")
    rng = np.random.default_rng(4)
    lm = rng.integers(0, 1 << 40, (sc.num_texels, 4)).astype(np.int64)
    flux = 65000.0
    assert B.bound(sc, N, flux) < 2.0 ** 55
    assert np.array_equal(B.add(sc, g, (30, 28, 24), (0, 0, 0), flux, lm), lm)  # no reflectance, no bounced light
    assert np.array_equal(B.add(sc, np.zeros_like(g), (30, 28, 24), (0.9, 0.9, 0.9), flux, lm), lm)
    got = B.add(sc, g, (30, 28, 24), (1.0, 0.5, 0.0), flux, lm)
    d = got - lm
    lit = g.any(axis=0)
    assert (d[:, 3] == 0).all() and not d[~sc.level0_mask()].any() and not d[~lit].any()
    assert (d[lit, 0] > 0).all() and (d[:, 2] == 0).all() and (d[lit, 0] > d[lit, 1]).all()
    # refl = 1: the rows simply add up; refl = 0.5: row n weighs 2^-n, exactly
    jobs = B.R.job_texels(sc)
    t = int(jobs[np.flatnonzero(lit[jobs])[0]])
    a, = [B.area_t(w) for w in sc.walls if 0 <= t - int(w["lm"][0]) < int(w["lm"][1]) * int(w["lm"][2])]
    v1 = float(g[0][t]) + float(g[1][t]) + float(g[2][t])
    v5 = (float(g[0][t]) * 0.5 + float(g[1][t]) * 0.25) + float(g[2][t]) * 0.125
    assert d[t, 0] == int(np.floor(np.ldexp(((30.0 * v1) * flux) * a, 25)))
    assert d[t, 1] == int(np.floor(np.ldexp(((28.0 * v5) * flux) * a, 25)))


def test_relight_options():
    import relight

    base = ["box8", "--spa", "1000", "--scenarios", "s.json"]
    a = relight.parse_args(base)
    assert a.sun_bounces == 0 and a.sun_reflectance == [0.9, 0.9, 0.9]
    a = relight.parse_args(base + ["--sun-bounces", "8", "--sun-reflectance", "1", "0.5", "0"])
    assert a.sun_bounces == 8 and a.sun_reflectance == [1.0, 0.5, 0.0]
    for bad in (["--sun-bounces", "9"], ["--sun-bounces", "-1"], ["--sun-reflectance", "0.5", "0.5", "1.5"],
                ["--sun-reflectance", "0.5", "nan", "0.5"]):
        with pytest.raises(SystemExit):
            relight.parse_args(base + bad)
