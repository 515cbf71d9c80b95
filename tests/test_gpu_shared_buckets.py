"""The bucket layout filled through per-workgroup tile blocks (AccShared, bucket_fill=2): int64 lightmaps against
the oracle, bit for bit, on the shapes where its protocol can go wrong: every lane of a workgroup on one tile
word (hundreds of block switches, ring slots reused, ranks past two blocks), one wide / two narrow tiles,
launches smaller than a wave or a workgroup, the product shapes (staged and compact closed box, the
cooperative scan's lead lanes, the hybrid scan) and an exhausted pool. Every test sets bucket_fill=2 itself,
so none depends on what AUTO chooses, and prints its bucket_fallback_codes."""
import functools
import os

import numpy as np
import pytest

import fm_oracle as O
import fmgi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOX_SPA = 172_413_793


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(maxsize=None)
def _small_box(tile_size):
    from fmgi import scene

    return scene.box_scene(200, tile_size=tile_size)


_ORACLE = {}


def _oracle(key, sc, spa, offsets, lo, hi):
    """the oracle's (lightmap, stats) of items [lo, hi), computed once per module and never modified"""
    k = (key, spa, lo, hi)
    if k not in _ORACLE:
        lm, st = O.bake(sc, O.schedule_with_offsets(sc, spa, offsets), lo, hi)
        lm.setflags(write=False)
        _ORACLE[k] = (lm, st)
    return _ORACLE[k]


def _ctx(sc, spa, offsets, **options):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(fmgi.ACCUM_STREAM)
    ctx.set_scene(sc)
    ctx.plan(spa, rng_offsets=offsets)
    ctx.set_option("bucket_fill", 2)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _bake(torch, ctx, lo, hi, kernel=fmgi.KERNEL_AUTO, fallback_allowed=False, label=""):
    """bakes items [lo, hi) on a fresh lightmap; checks the instance, the overflow flag and the fallback count"""
    ctx.reset_stats()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lm = torch.zeros((ctx.scene.num_texels, 4), dtype=torch.int64, device="cuda")
        ctx.bake_items(lo, hi, lm.data_ptr(), kernel, s.cuda_stream)
    s.synchronize()
    st = ctx.stats()
    print(f"{label or ctx.scene.name} items [{lo}, {hi}): bucket_fallback_codes = {st['bucket_fallback_codes']} "
          f"of {st['deposits']} deposits; {ctx.last_bake_kernel}")
    assert "AccShared" in ctx.last_bake_kernel
    assert st["stream_overflow"] == 0
    if not fallback_allowed:
        assert st["bucket_fallback_codes"] == 0
    got = lm.cpu().numpy()
    assert not got[:, 3].any()
    return got[:, :3], st


def test_one_tile_every_lane_on_one_word(torch_cuda, offsets):
    """1,176 texels = one fold tile: a workgroup's 768 lanes fill a 1,024-code block in under two iterations, so
    each workgroup switches blocks hundreds of times and reuses every ring slot; ranks past 2 BP are possible
    while an opener's pool atomic is in flight, so this is the one test whose bucket_fallback_codes may be
    non-zero (measured on an MI355X: 0 of 2,399,993 deposits)."""
    sc = _small_box(2.0)
    assert sc.num_texels == 1176
    olm, ost = _oracle("box200/2.0", sc, BOX_SPA, offsets, 0, 3000)
    ctx = _ctx(sc, BOX_SPA, offsets)
    lm, st = _bake(torch_cuda, ctx, 0, 3000, fallback_allowed=True)
    assert np.array_equal(lm, olm)
    for k in ("photons", "deposits", "escapes"):
        assert st[k] == ost[k], k
    ctx.close()


@pytest.mark.parametrize("wide", [0, 1])
def test_two_narrow_tiles_or_one_wide(torch_cuda, offsets, wide):
    sc = _small_box(4.0)
    assert sc.num_texels == 2152
    olm, _ = _oracle("box200/4.0", sc, BOX_SPA, offsets, 0, 3000)
    ctx = _ctx(sc, BOX_SPA, offsets, wide_tiles=wide)
    lm, _ = _bake(torch_cuda, ctx, 0, 3000)
    assert np.array_equal(lm, olm)
    ctx.close()


@pytest.mark.parametrize("items", [5, 70])
def test_partial_launches(torch_cuda, offsets, items):
    """fewer items than a wave / a workgroup has lanes: idle waves, published blocks that get no code, the
    lengths of partly filled blocks"""
    sc = _small_box(2.0)
    olm, _ = _oracle("box200/2.0", sc, BOX_SPA, offsets, 0, items)
    ctx = _ctx(sc, BOX_SPA, offsets)
    lm, _ = _bake(torch_cuda, ctx, 0, items)
    assert np.array_equal(lm, olm)
    ctx.close()


def test_split_launches_sum_to_one(torch_cuda, offsets):
    sc = _small_box(2.0)
    olm, _ = _oracle("box200/2.0", sc, BOX_SPA, offsets, 0, 3000)
    ctx = _ctx(sc, BOX_SPA, offsets)
    a, _ = _bake(torch_cuda, ctx, 0, 1234)
    b, _ = _bake(torch_cuda, ctx, 1234, 3000)
    assert np.array_equal(a + b, olm)
    ctx.close()


@pytest.mark.parametrize("wide", [0, 1])
def test_box200_staged(torch_cuda, box200, offsets, wide):
    olm, _ = _oracle("box200", box200, BOX_SPA, offsets, 7_000, 27_000)
    ctx = _ctx(box200, BOX_SPA, offsets, wide_tiles=wide)
    lm, _ = _bake(torch_cuda, ctx, 7_000, 27_000)
    assert np.array_equal(lm, olm)
    ctx.close()


def test_example_cooperative_lead_lanes(torch_cuda, example_scene, offsets):
    """300 items of example.png: the cooperative scan (only a group's lead lane deposits), 56 tiles"""
    olm, _ = _oracle("example", example_scene, 65_000, offsets, 0, 300)
    ctx = _ctx(example_scene, 65_000, offsets)
    lm, _ = _bake(torch_cuda, ctx, 0, 300)
    assert "ScanFast" in ctx.last_bake_kernel
    assert np.array_equal(lm, olm)
    ctx.close()


def test_example_hybrid(torch_cuda, example_scene, offsets):
    olm, _ = _oracle("example", example_scene, 6_500_000, offsets, 40_000, 52_000)
    ctx = _ctx(example_scene, 6_500_000, offsets)
    lm, _ = _bake(torch_cuda, ctx, 40_000, 52_000, kernel=fmgi.KERNEL_HYBRID)
    assert "ScanHybrid" in ctx.last_bake_kernel
    assert np.array_equal(lm, olm)
    ctx.close()


def test_box2000_compact(torch_cuda, box2000, offsets):
    olm, _ = _oracle("box2000", box2000, BOX_SPA, offsets, 5_000, 6_000)
    ctx = _ctx(box2000, BOX_SPA, offsets)
    lm, _ = _bake(torch_cuda, ctx, 5_000, 6_000)
    assert "ScanGridT<true, true, true>" in ctx.last_bake_kernel
    assert np.array_equal(lm, olm)
    ctx.close()


@pytest.mark.parametrize("limit", [64, 1])
def test_pool_exhaustion(torch_cuda, box200, offsets, limit):
    """a pool of 64 blocks (some, then none) and of 1 (none from init on): the rest through bucket_atomic"""
    olm, _ = _oracle("box200", box200, BOX_SPA, offsets, 2_000, 6_000)
    ctx = _ctx(box200, BOX_SPA, offsets, pool_limit=limit)
    lm, st = _bake(torch_cuda, ctx, 2_000, 6_000, fallback_allowed=True)
    assert st["bucket_fallback_codes"] > 0
    assert np.array_equal(lm, olm)
    ctx.close()
