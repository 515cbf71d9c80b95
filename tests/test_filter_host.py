"""CPU tests of the adaptive density filter: the restatement (filter_restate.py) on hand-computed
cases and against its own word-for-word form, the identities the definition promises, fmgi_filter_energy against
Python integers, the argument checks of the two device calls on a host-only context, tools/relight.py's
arguments, and the quality property on the CPU oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import filter_restate as F
import fm_oracle as O
import fmgi
from conftest import GOLDEN, REPO
from fmgi import _lib, scene

M64 = F.M64


def _scene(dims):
    """box walls with the given level-0 grids (s1, s2), texel bases as the reference assigns them"""
    sc = scene.box_scene(200, tile_size=4.0, with_light=True)
    walls = sc.walls[: len(dims)].copy()
    for w, (s1, s2) in zip(walls, dims):
        w["lm"][1], w["lm"][2] = s1, s2
    return scene.Scene("grids", walls, sc.windows, sc.lights, scene.assign_texel_bases(walls))


def _lm(rows):
    return np.array([list(r) + [0] * (4 - len(r)) for r in rows], np.uint64)


# ---- hand-computed cases -------------------------------------------------------------------------------------------

def test_one_by_one():
    sc = _scene([(1, 1)])
    lm = _lm([(5, 7, 9, 3)])
    for R in (0, 1, 16):
        assert F.radii(sc, lm, 21, R).tolist() == [0]           # e = 21 reaches 21 at r = 0
        assert F.radii(sc, lm, 22, R).tolist() == [R]           # never reached: max_radius
    assert F.apply(sc, lm, np.array([16], np.uint8)).tolist() == [[5, 7, 9, 3]]


def test_two_by_one():
    sc = _scene([(2, 1)])                                       # s1 = 2, s2 = 1: texels 0, 1; texel 2 is the mip level
    assert sc.num_texels == 3
    lm = _lm([(10, 0, 1, 8), (3, 2, 0, 9), (100, 100, 100, 100)])
    # e = 11, 5; S_0 = 11, 5; S_1 = 16, 16
    assert F.radii(sc, lm, 11, 4).tolist() == [0, 1, 0]
    assert F.radii(sc, lm, 16, 4).tolist() == [1, 1, 0]
    assert F.radii(sc, lm, 17, 4).tolist() == [4, 4, 0]
    got = F.apply(sc, lm, np.array([0, 1, 9], np.uint8))
    assert got.tolist() == [[10, 0, 1, 8], [6, 1, 0, 9], [100, 100, 100, 100]]  # (10 + 3) // 2, (0 + 2) // 2, (1 + 0) // 2


def test_three_by_three():
    sc = _scene([(3, 3)])
    v = np.arange(1, 10)
    lm = _lm([(int(a), 0, 2 * int(a), 7) for a in v])           # e = 3, 6, ..., 27
    # S_1: corner (0, 0) = 3 * (1 + 2 + 4 + 5) = 36; edge (1, 0) = 3 * 21 = 63; centre = 3 * 45 = 135
    rad = F.radii(sc, lm, 27, 2)
    assert rad[:9].reshape(3, 3).tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 0]]  # only e(2, 2) = 27 reaches it alone
    assert F.radii(sc, lm, 36, 2)[:9].tolist() == [1] * 9       # e(2, 2) < 36 <= every S_1
    assert F.radii(sc, lm, 135, 2)[:9].reshape(3, 3).tolist() == [[2, 2, 2], [2, 1, 2], [2, 2, 2]]
    assert F.radii(sc, lm, 136, 2)[:9].tolist() == [2] * 9
    out = F.apply(sc, lm, np.array([1, 1, 0, 0, 1, 0, 0, 0, 2] + [0] * (sc.num_texels - 9), np.uint8))
    assert out[0].tolist() == [12 // 4, 0, 24 // 4, 7]
    assert out[1].tolist() == [21 // 6, 0, 42 // 6, 7]
    assert out[2].tolist() == [3, 0, 6, 7]
    assert out[4].tolist() == [5, 0, 10, 7]
    assert out[8].tolist() == [5, 0, 10, 7]                     # radius 2 from a corner: the whole wall
    assert np.array_equal(out[9:], lm[9:])


def test_numpy_restatement_equals_the_word_for_word_one():
    rng = np.random.default_rng(5)
    sc = _scene([(1, 1), (4, 2), (1, 8), (8, 1), (5, 3), (8, 8)])   # (5, 3): not a power of two
    T = sc.num_texels
    lm = rng.integers(0, 1 << 62, (T, 4), dtype=np.uint64)
    lm[::7] = rng.integers((1 << 64) - 1000, 1 << 64, (len(lm[::7]), 4), dtype=np.uint64, endpoint=False)  # sums wrap
    guide = rng.integers(0, 1000, (T, 4), dtype=np.uint64)
    walls = F.grids(sc)
    for E, R in ((0, 3), (2500, 2), (9000, 16), (M64, 1), (5000, 0)):
        rad = F.radii(sc, guide, E, R)
        assert rad.tolist() == F.radii_exact(walls, T, guide.tolist(), E, R)
        assert F.apply(sc, lm, rad).tolist() == F.apply_exact(walls, lm.tolist(), rad.tolist())
    rad = rng.integers(0, 256, T).astype(np.uint8)               # radii above 16 are 16
    assert F.apply(sc, lm, rad).tolist() == F.apply_exact(walls, lm.tolist(), rad.tolist())
    assert np.array_equal(F.apply(sc, lm.view(np.int64), rad), F.apply(sc, lm, rad).view(np.int64))


# ---- identities ------------------------------------------------------------------------------------------------------

def test_identities():
    rng = np.random.default_rng(6)
    sc = _scene([(8, 4), (1, 1), (16, 16), (2, 32)])
    T = sc.num_texels
    lm = rng.integers(0, 1 << 64, (T, 4), dtype=np.uint64, endpoint=False)
    assert not F.radii(sc, lm, 0, 16).any()                      # min_energy == 0
    assert not F.radii(sc, lm, M64, 0).any()                     # max_radius == 0
    assert np.array_equal(F.apply(sc, lm, np.zeros(T, np.uint8)), lm)
    assert not F.radii(sc, lm, 12345, 16)[~sc.level0_mask()].any()   # the mip levels
    const = lm.copy()                                            # walls whose texels are all equal stay unchanged
    for k, (s0, s1, s2) in enumerate(F.grids(sc)):
        const[s0 : s0 + s1 * s2, :3] = [(1 << 53) - 1 - k, 3 * k, 1 << 40]  # windows of <= 1089 texels stay below 2^64
    for rad in (F.radii(sc, const, M64, 16), F.radii(sc, const, 1 << 56, 16), rng.integers(0, 256, T).astype(np.uint8)):
        assert np.array_equal(F.apply(sc, const, rad), const)


# ---- fmgi_filter_energy --------------------------------------------------------------------------------------------

def test_filter_energy():
    assert fmgi.filter_energy(256) == 256 * 3 * 18 * 2**25 == 463856467968
    assert fmgi.filter_energy(0) == 0 and fmgi.filter_energy(1, fmgi.Palette.reference()) == 54 << 25
    p = fmgi.Palette(window_rgb=(2.5, 1.75, 31.999), light_rgb=(0, 0, 0), albedo=0.5)
    row = fmgi.palette_table(p)[512 | 1]                         # a first-bounce window photon's deposit
    one = sum(int(v) for v in row)
    assert one == sum(int(np.ldexp(np.float64(np.float32(v)), 25)) for v in (2.5, 1.75, 31.999))
    assert fmgi.filter_energy(64, p) == 64 * one
    assert fmgi.filter_energy(M64, p) == (M64 * one) & M64       # mod 2^64
    with pytest.raises(fmgi.FmgiError):
        fmgi.filter_energy(1, fmgi.Palette(window_rgb=(32, 0, 0)))
    bad = fmgi.Palette(albedo=2.0)
    assert _lib.load().fmgi_filter_energy(C.byref(bad), 5) == 0 and "palette" in _lib.last_error()


# ---- argument checks (host-only context) ---------------------------------------------------------------------------

ARG, STATE, NO_DEVICE = -3, -4, -1


def test_argument_errors_and_their_order():
    lib = _lib.load()
    vp = C.c_void_p
    p16 = vp(16)
    one = (vp * 1)(vp(16))
    null1 = (vp * 1)(None)
    two_null = (vp * 2)(vp(16), None)
    two = (vp * 2)(vp(16), vp(32))
    h = lib.fmgi_create(fmgi.HOST_ONLY)
    try:
        # without a scene: argument errors first, then the state
        assert lib.fmgi_filter_radii(None, p16, 1, 4, p16, None) == ARG
        assert lib.fmgi_filter_radii(h, None, 1, 4, p16, None) == ARG
        assert lib.fmgi_filter_radii(h, p16, 1, 4, None, None) == ARG
        assert lib.fmgi_filter_radii(h, p16, 1, -1, p16, None) == ARG
        assert lib.fmgi_filter_radii(h, p16, 1, 17, p16, None) == ARG and "max_radius" in _lib.last_error()
        assert lib.fmgi_filter_radii(h, p16, 1, 16, p16, None) == STATE
        assert lib.fmgi_filter_radii(h, p16, 1, 0, p16, None) == STATE
        assert lib.fmgi_filter_apply(None, p16, one, one, 1, None) == ARG
        assert lib.fmgi_filter_apply(h, None, one, one, 1, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, None, one, 1, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, one, None, 1, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, one, one, 0, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, one, one, -3, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, null1, one, 1, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, one, null1, 1, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, two, two_null, 2, None) == ARG and "map 1" in _lib.last_error()
        assert lib.fmgi_filter_apply(h, p16, two_null, two, 2, None) == ARG
        assert lib.fmgi_filter_apply(h, p16, one, one, 1, None) == STATE
        assert lib.fmgi_filter_apply(h, p16, two, two, 2, None) == STATE
    finally:
        lib.fmgi_destroy(h)
    ctx = fmgi.Context(fmgi.HOST_ONLY)
    try:
        ctx.set_scene(scene.box_scene(8))
        # with a scene: argument errors still first, then the missing device
        assert lib.fmgi_filter_radii(ctx.h, p16, 1, 17, p16, None) == ARG
        assert lib.fmgi_filter_radii(ctx.h, None, 1, 4, p16, None) == ARG
        assert lib.fmgi_filter_radii(ctx.h, p16, 1, 4, p16, None) == NO_DEVICE
        assert lib.fmgi_filter_apply(ctx.h, p16, one, one, 0, None) == ARG
        assert lib.fmgi_filter_apply(ctx.h, p16, two, two_null, 2, None) == ARG
        assert lib.fmgi_filter_apply(ctx.h, p16, one, one, 1, None) == NO_DEVICE
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
            ctx.filter_radii(16, 1, 99, 16)
        with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
            ctx.filter_radii(16, 1, 4, 16)
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
            ctx.filter_apply(16, [], [])
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
            ctx.filter_apply(0, [16], [16])
        with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
            ctx.filter_apply(16, [16, 32], [16, 32])
        with pytest.raises(fmgi.FmgiError, match="inputs"):
            ctx.filter_apply(16, [16, 32], [16])
    finally:
        ctx.close()


# ---- tools/relight.py ----------------------------------------------------------------------------------------------

def test_relight_arguments():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
    finally:
        sys.path.pop(0)
    base = ["box200", "--spa", "2000", "--scenarios", "s.json"]
    a = relight.parse_args(base)
    assert a.min_deposits == 0 and a.max_radius == 4             # without the flags: no filter
    a = relight.parse_args(base + ["--min-deposits", "64"])
    assert a.min_deposits == 64 and a.max_radius == 4
    a = relight.parse_args(base + ["--min-deposits", "256", "--max-radius", "16"])
    assert (a.min_deposits, a.max_radius) == (256, 16)
    for bad in (["--max-radius", "17"], ["--max-radius", "-1"], ["--min-deposits", "-5"]):
        with pytest.raises(SystemExit):
            relight.parse_args(base + bad)


# ---- quality on the CPU oracle -------------------------------------------------------------------------------------

def test_filtered_low_photon_bake_is_closer_to_a_reference_bake():
    """The box of DESIGN.md §13's table at half its photon counts (the table's pair, 20,000 against 400,000 samples
    per area, takes about 20 s on the CPU oracle; test_gpu_filter.py bakes that pair on the device): low bake
    spa 10,000, reference bake spa 200,000 with the offsets reversed, filtered at filter_energy(256), radius <= 4."""
    sc = scene.box_scene(200, tile_size=20.0, with_light=True)
    offsets = np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))
    low = O.bake(sc, O.schedule_with_offsets(sc, 10_000, offsets))[0]
    ref = O.bake(sc, O.schedule_with_offsets(sc, 200_000, offsets[::-1].copy()))[0]
    rad = F.radii(sc, low, fmgi.filter_energy(256), 4)
    out = F.apply(sc, low, rad)
    unfiltered, filtered = F.l1_pair(sc, low, out, ref)
    print(f"L1 unfiltered {unfiltered:.5f}, filtered {filtered:.5f}, mean radius {rad.mean():.3f} over "
          f"{sc.num_texels} texels")
    assert filtered < unfiltered
