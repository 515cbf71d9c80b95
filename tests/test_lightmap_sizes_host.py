"""The scenes of tests/lightmap_sizes.py reach what the GPU tests (tests/test_gpu_lightmap_sizes.py) use them for.
On the oracle alone: the two item ranges together put a deposit in every fold tile of every even(T), in texel 0 and
in texel T - 1 (so a fold that loses a tile, or that stops one texel early, loses a deposit), and in exactly the
tiles that gapped(T)'s walls touch. On a host-only context: every scene is accepted, plans the same schedule, keeps
the box's lattice, and fmgi_bake_sparse_supported changes between 129,024 and 129,025 texels."""
import functools
import os

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import lightmap_sizes as LS
from conftest import GOLDEN

SCENES = [("even", T) for T in LS.EVEN_SIZES] + [("gapped", T) for T in LS.GAPPED_SIZES]
IDS = [f"{k}{T}" for k, T in SCENES]


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(None)
def _counts(kind, T):
    """deposits per texel of both ranges together, and the oracle's stats of each"""
    sc = LS.get(kind, T)
    L = O.schedule_with_offsets(sc, LS.SPA, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))
    assert int(L["item_begin"][-1] + L["count"][-1]) == LS.TOTAL_ITEMS
    assert int(L[L["is_window"] == 0]["item_begin"][0]) == LS.LAMP_BEGIN
    total, stats = np.zeros(T, np.int64), []
    for lo, hi in LS.RANGES:
        _, st, cnt = O.bake(sc, L, lo, hi, counts=True)
        assert st["photons"] == 100 * (hi - lo) and int(cnt.sum()) == st["deposits"]
        total += cnt
        stats.append(st)
    total.setflags(write=False)
    return total, stats


def _per_tile(cnt):
    P = LS.tiles_of(len(cnt))
    padded = np.zeros(P * LS.TILE_TEXELS, np.int64)
    padded[: len(cnt)] = cnt
    return padded.reshape(P, LS.TILE_TEXELS).sum(axis=1)


def test_the_sizes_have_their_tile_counts():
    for T, P in LS.EVEN_SIZES.items():
        assert LS.tiles_of(T) == P, T
    assert LS.tiles_of(LS.BUCKET_MAX) == 63 and LS.tiles_of(LS.BUCKET_MAX + 1) == 64
    assert [LS.tiles_of(T) for T in LS.GAPPED_SIZES] == [2048, 2048]
    assert LS.STREAM_END == 2048 * LS.TILE_TEXELS


@pytest.mark.parametrize("T", list(LS.EVEN_SIZES))
def test_even_walls_end_on_the_last_texel_and_reach_every_tile(T):
    sc = LS.even(T)
    assert sc.num_texels == T
    lm = sc.walls["lm"]
    ends = lm[:, 0] + lm[:, 1] * lm[:, 2]
    assert int(ends.max()) == T and int(lm[:, 0].min()) == 0
    assert LS.touched_tiles(sc) == list(range(LS.EVEN_SIZES[T]))
    if T >= 384:
        assert (lm[:, 2] == 64).all() and (lm[:, 1] == (T // 6) // 64).all()
    else:
        assert (lm[:, 2] == 1).all() and (lm[:, 1] == T // 6).all()


@pytest.mark.parametrize("T", list(LS.EVEN_SIZES))
def test_even_ranges_deposit_in_every_tile_and_both_end_texels(T):
    """(measured: the emptiest tile gets 8 deposits at 126,977 and 4 at 262,145; texel T - 1 gets 4 to 8 from
    126,977 texels up; texel 0 of even(6) gets 873,347)"""
    cnt, _ = _counts("even", T)
    tiles = _per_tile(cnt)
    print(f"even({T}): {len(tiles)} tiles, least {int(tiles.min())} deposits; texel 0: {int(cnt[0])}, "
          f"texel {T - 1}: {int(cnt[-1])}")
    assert len(tiles) == LS.EVEN_SIZES[T]
    assert (tiles >= 1).all(), f"tiles without a deposit: {np.flatnonzero(tiles == 0)[:8]}"
    assert cnt[0] >= 1 and cnt[T - 1] >= 1
    if T == 6:
        assert cnt[0] >= 100_000, int(cnt[0])  # a hot texel: every deposit on the floor


@pytest.mark.parametrize("T", LS.GAPPED_SIZES)
def test_gapped_ranges_deposit_in_exactly_the_walls_tiles(T):
    """(the last wall starts on a tile boundary at 4,194,304 texels: 14 tiles there, 15 at 4,194,303)"""
    sc = LS.gapped(T)
    touched = LS.touched_tiles(sc)
    assert len(touched) == (15 if T == LS.STREAM_END - 1 else 14)
    assert touched[:9] == [0, 1, 2, 62, 63, 64, 127, 128, 129] and touched[-1] == 2047
    cnt, _ = _counts("gapped", T)
    tiles = _per_tile(cnt)
    assert list(np.flatnonzero(tiles)) == touched
    print(f"gapped({T}): texel {T - 1}: {int(cnt[-1])} deposits")
    assert cnt[T - 1] >= 1 and cnt[0] >= 1
    assert not cnt[~sc.level0_mask()].any()


@pytest.mark.parametrize("kind,T", SCENES, ids=IDS)
def test_oracle_counters(kind, T):
    _, stats = _counts(kind, T)
    for st in stats:
        assert st["scans"] == st["deposits"] + st["escapes"]
    # the geometry is the same box whatever its lightmap: the same paths
    _, first = _counts("even", 6)
    assert stats == first


@pytest.mark.parametrize("kind,T", SCENES, ids=IDS)
def test_host_context_accepts_every_scene(offsets, kind, T):
    sc = LS.get(kind, T)
    ctx = fmgi.Context(fmgi.HOST_ONLY)
    ctx.set_scene(sc)
    assert ctx.plan(LS.SPA, rng_offsets=offsets) == LS.TOTAL_ITEMS
    ranges = ctx.source_ranges()
    assert [(r[1], r[2], r[3]) for r in ranges] == [(1, 0, LS.LAMP_BEGIN), (0, LS.LAMP_BEGIN, LS.TOTAL_ITEMS)]
    assert len(ctx.lattice_tables()["lattice"]) == 6
    assert ctx.bake_sparse_supported() is (T <= LS.BUCKET_MAX)
    ctx.close()


def test_bake_sparse_supported_follows_the_layout(offsets):
    ctx = fmgi.Context(fmgi.HOST_ONLY)
    ctx.set_scene(LS.even(LS.BUCKET_MAX))
    assert ctx.bake_sparse_supported() is True
    ctx.set_option("stream_layout", 0)
    assert ctx.bake_sparse_supported() is False
    ctx.set_option("stream_layout", -1)
    assert ctx.bake_sparse_supported() is True
    ctx.close()
