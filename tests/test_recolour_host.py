"""CPU tests of the recolouring feature's host side: the palette tables against a numpy.float32
replay of their definition, the colour states re-derived from the oracle's bounce events, the argument checks of
fmgi_recolour on a host-only context, and Context.source_ranges."""
import ctypes as C

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import recolour_events as R
from fmgi import _lib

REFERENCE = dict(window_rgb=(18, 18, 18), light_rgb=(16, 16, 18), floor_tint=(1.0, 0.85, 0.7), albedo=0.9)
EVENING = dict(window_rgb=(2.5, 1.75, 3.0), light_rgb=(31.5, 24.0, 12.125), floor_tint=(0.9, 0.6, 0.3), albedo=0.77)
NIGHT = dict(window_rgb=(0, 0, 0.015625), light_rgb=(7.3, 7.1, 0.0), floor_tint=(1.0, 1.0, 0.0), albedo=1.0)


@pytest.mark.parametrize("pal", [REFERENCE, EVENING, NIGHT], ids=["reference", "evening", "night"])
def test_palette_table_equals_float32_replay(pal):
    got = fmgi.palette_table(fmgi.Palette(**pal))
    assert got.dtype == np.int64 and got.shape == (1024, 3)
    assert np.array_equal(got, R.table_replay(**pal))
    assert not got[0].any() and not got[512].any()
    assert got.min() >= 0 and got.max() < 2**30


def test_reference_palette_is_the_default():
    a, b = fmgi.Palette.reference(), fmgi.Palette()
    assert bytes(a) == bytes(b)
    t = fmgi.palette_table(a)
    assert t[513].tolist() == [18 << 25] * 3 and t[1].tolist() == [16 << 25, 16 << 25, 18 << 25]


def test_event_derived_states_give_the_oracle_lightmap():
    sc, L, _ = R.lit_box()
    table = fmgi.palette_table(fmgi.Palette.reference())
    tex, st, rgb = R.events_of()
    assert len(tex) > 50_000
    fx = np.ldexp(rgb.astype(np.float64), 25)
    assert np.array_equal(fx, np.floor(fx))  # every deposit is a multiple of 2^-25
    assert np.array_equal(fx.astype(np.int64), table[st])
    exp = sum(O.bake(sc, L, b, e)[0] for b, e in R.RANGES)
    got = np.array(R.fold(R.sparse_histogram(), table, sc.num_texels), dtype=object)
    assert np.array_equal(got, exp.astype(object))
    s, _, n = R.sparse_histogram()
    assert n.sum() == len(tex) and set(np.unique(s // 512)) == {0, 1}


def _host_ctx(sc):
    ctx = fmgi.Context(fmgi.HOST_ONLY)
    ctx.set_scene(sc)
    return ctx


def _recolour_rc(ctx, counts, pals, lms, groups=None, scenarios=None):
    G = len(counts) if groups is None else groups
    K = len(lms) if scenarios is None else scenarios
    cp = (C.c_void_p * max(len(counts), 1))(*counts)
    lp = (C.c_void_p * max(len(lms), 1))(*lms)
    pal = (fmgi.Palette * max(len(pals), 1))(*pals)
    return ctx.lib.fmgi_recolour(ctx.h, cp, G, pal, K, lp, None)


BAD = {"nan": dict(albedo=float("nan")), "inf": dict(window_rgb=(float("inf"), 1, 1)),
       "negative": dict(light_rgb=(16, -0.5, 18)), "emitter32": dict(window_rgb=(18, 32.0, 18)),
       "tint": dict(floor_tint=(1.0, 1.5, 0.7)), "albedo": dict(albedo=1.0000001)}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_bad_palettes_are_argument_errors(bad):
    p = fmgi.Palette(**BAD[bad])
    with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
        fmgi.palette_table(p)
    ctx = _host_ctx(R.lit_box()[0])
    try:
        assert _recolour_rc(ctx, [16], [p], [16]) == -3
        assert _recolour_rc(ctx, [16, 16], [fmgi.Palette(), p], [16]) == -3  # the second group's palette
    finally:
        ctx.close()


def test_recolour_argument_errors_come_before_the_device():
    sc = R.lit_box()[0]
    ctx = _host_ctx(sc)
    try:
        ok = fmgi.Palette()
        assert _recolour_rc(ctx, [16], [ok], [16], groups=0) == -3
        assert _recolour_rc(ctx, [16], [ok], [16], scenarios=0) == -3
        assert _recolour_rc(ctx, [None], [ok], [16]) == -3
        assert _recolour_rc(ctx, [16], [ok], [None]) == -3
        assert ctx.lib.fmgi_recolour(ctx.h, None, 1, None, 1, None, None) == -3
        assert ctx.lib.fmgi_palette_table(None, None) == -3
        # a valid call gets as far as the missing device, and so does a histogram bake
        assert _recolour_rc(ctx, [16], [ok], [16]) == -1
        assert _recolour_rc(ctx, [16, 32], [ok] * 18, [16] * 9) == -1
        ctx.plan(R.SPA, rng_offsets=R.lit_box()[2])
        assert ctx.lib.fmgi_bake_states(ctx.h, 0, 1, C.c_void_p(16), fmgi.KERNEL_AUTO, None) == -1
        assert ctx.lib.fmgi_bake_states(ctx.h, 0, 1, None, fmgi.KERNEL_AUTO, None) == -3
    finally:
        ctx.close()
    empty = fmgi.Context(fmgi.HOST_ONLY)  # no scene set
    try:
        assert _recolour_rc(empty, [16], [fmgi.Palette()], [16]) == -4
    finally:
        empty.close()
    assert fmgi.states_bytes(sc.num_texels) == 1024 * sc.num_texels * 8 and fmgi.states_bytes(0) == 0
    assert _lib.COLOUR_STATE_COUNT == 1024 and _lib.RECOLOUR_MAX_SCENARIOS == 8


def test_source_ranges_cover_the_plan(example_scene):
    offsets = R.lit_box()[2]
    for sc, spa in ((R.lit_box()[0], R.SPA), (example_scene, 65_000)):
        ctx = _host_ctx(sc)
        try:
            total = ctx.plan(spa, rng_offsets=offsets)
            rs = ctx.source_ranges()
            assert [r[0] for r in rs] == list(range(len(sc.sources)))
            assert [r[1] for r in rs] == [1] * len(sc.windows) + [0] * len(sc.lights)
            assert rs[0][2] == 0 and rs[-1][3] == total
            assert all(a[3] == b[2] for a, b in zip(rs, rs[1:])) and all(r[2] < r[3] for r in rs)
        finally:
            ctx.close()
    assert R.lit_box()[0].num_texels == 2152
    ctx = _host_ctx(R.lit_box()[0])
    ctx.plan(R.SPA, rng_offsets=offsets)
    assert ctx.source_ranges() == [(0, 1, 0, 256), (1, 0, 256, 512)]
    ctx.close()
