"""The wave-locked photon loop of the closed boxes (k_bake_locked, photon_lock=1): int64 lightmaps, the four
counters and per-photon traces against the oracle, bit for bit, on the shapes where its wave-uniform control can
go wrong: launches that end inside a wave's round of 64 items, shards that start off a round, rounds whose lanes
hold both source kinds, photons that escape (their lanes are parked until the wave's next photon), every
accumulation the instance is built for, and the compact instance. Every test sets photon_lock=1 itself, so
none depends on what AUTO chooses."""
import functools
import os

import numpy as np
import pytest

import fm_oracle as O
import fmgi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOX_SPA = 172_413_793
COUNTERS = ("photons", "scans", "deposits", "escapes")
# items of box200 at BOX_SPA (schedule from glibc_rand_4096.npy) with a photon that escapes, found with
# O.trace_item on the CPU: their traces have 794, 799 and 798 events instead of 800
SHORT_ITEMS = (478, 2549, 5353)


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(maxsize=None)
def _small_box(with_light=False):
    from fmgi import scene

    return scene.box_scene(200, tile_size=2.0, with_light=with_light)


_ORACLE = {}


def _oracle(key, sc, spa, offsets, lo, hi, port=False):
    """the oracle's (lightmap, stats) of items [lo, hi), computed once per module and never modified (port: through
    O.bake_port, the same restatement several times faster, bit-identical by tests/test_oracle.py: the two
    ranges that take the plain oracle minutes)"""
    k = (key, spa, lo, hi)
    if k not in _ORACLE:
        lm, st = (O.bake_port if port else O.bake)(sc, O.schedule_with_offsets(sc, spa, offsets), lo, hi)
        lm.setflags(write=False)
        _ORACLE[k] = (lm, st)
    return _ORACLE[k]


def _ctx(sc, spa, offsets, accum=fmgi.ACCUM_STREAM, **options):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(accum)
    ctx.set_scene(sc)
    ctx.plan(spa, rng_offsets=offsets)
    ctx.set_option("photon_lock", 1)
    if accum == fmgi.ACCUM_STREAM and "bucket_fill" not in options:
        options["bucket_fill"] = 2
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _bake(torch, ctx, lo, hi):
    """bakes items [lo, hi) on a fresh lightmap; checks the instance and the overflow flag"""
    ctx.reset_stats()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lm = torch.zeros((ctx.scene.num_texels, 4), dtype=torch.int64, device="cuda")
        ctx.bake_items(lo, hi, lm.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
    s.synchronize()
    st = ctx.stats()
    print(f"{ctx.scene.name} items [{lo}, {hi}): {ctx.last_bake_kernel}")
    assert "k_bake_locked<" in ctx.last_bake_kernel, ctx.last_bake_kernel
    assert st["stream_overflow"] == 0
    got = lm.cpu().numpy()
    assert not got[:, 3].any()
    return got[:, :3], st


def _same_counters(st, ost, items):
    assert st["photons"] == 100 * items
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["scans"] == st["deposits"] + st["escapes"]


@pytest.mark.parametrize("lo,hi", [(0, 1), (0, 63), (0, 65), (0, 769), (5, 1000), (-100, None)])
def test_partial_waves_and_unaligned_shards(torch_cuda, offsets, lo, hi):
    """fewer items than a wave's round, one more than a round, one more than a 768-lane workgroup, a shard
    that starts off a round, and the schedule's last 100 items"""
    sc = _small_box()
    ctx = _ctx(sc, BOX_SPA, offsets)
    if hi is None:
        lo, hi = ctx.total_items + lo, ctx.total_items
    olm, ost = _oracle("small", sc, BOX_SPA, offsets, lo, hi)
    lm, st = _bake(torch_cuda, ctx, lo, hi)
    assert np.array_equal(lm, olm)
    _same_counters(st, ost, hi - lo)
    ctx.close()


def test_two_launches_sum_to_one(torch_cuda, offsets):
    sc = _small_box()
    olm, ost = _oracle("small", sc, BOX_SPA, offsets, 0, 700)
    ctx = _ctx(sc, BOX_SPA, offsets)
    a, sa = _bake(torch_cuda, ctx, 0, 300)
    b, sb = _bake(torch_cuda, ctx, 300, 700)
    assert np.array_equal(a + b, olm)
    for k in COUNTERS:
        assert sa[k] + sb[k] == ost[k], k
    ctx.close()


def test_escapes_park_their_lanes(torch_cuda, box200, offsets):
    """2e7 photons of box200 at the bench's samples per area: the oracle counts 137 escapes, each of which parks
    a lane until its wave starts the next photon"""
    n = 200_000
    olm, ost = _oracle("box200", box200, BOX_SPA, offsets, 0, n, port=True)
    assert ost["escapes"] >= 20, ost
    ctx = _ctx(box200, BOX_SPA, offsets)
    lm, st = _bake(torch_cuda, ctx, 0, n)
    assert np.array_equal(lm, olm)
    _same_counters(st, ost, n)
    ctx.close()


def test_traces_of_items_with_escapes(torch_cuda, box200, offsets):
    """three items with a photon that escapes, each with the other 63 items of its round of the trace launch:
    events, event counts and final RNG states (the TRACE instance, called as tests/test_gpu_parity.py does)"""
    L = O.schedule_with_offsets(box200, BOX_SPA, offsets)
    ctx = _ctx(box200, BOX_SPA, offsets)
    for w0 in SHORT_ITEMS:
        b = w0 - w0 % 64
        ev, cnt, rngf = ctx.trace_items(b, b + 64, fmgi.KERNEL_AUTO)
        assert "k_bake_locked<" in ctx.last_bake_kernel, ctx.last_bake_kernel
        assert ctx.stats()["stream_overflow"] == 0
        for w in range(b, b + 64):
            li = int(np.searchsorted(L["item_begin"], w, side="right") - 1)
            state = (w - int(L[li]["item_begin"]) + int(L[li]["rng_offset"])) & 0xFFFFFFFF
            oev, ofin = O.trace_item(box200, int(L[li]["source"]), int(L[li]["is_window"]), state)
            if w == w0:
                assert len(oev) < 800, (w, len(oev))
            k = w - b
            assert cnt[k] == len(oev), f"item {w}: {cnt[k]} vs {len(oev)} events"
            g = ev[k, : cnt[k]].view(np.uint32)
            assert np.array_equal(g, oev.view(np.uint32).reshape(g.shape)), f"item {w}"
            assert rngf[k] == ofin, f"item {w}: final RNG"
    ctx.close()


def test_mixed_sources_in_one_round(torch_cuda, offsets):
    """a range across the window's last launch and the ceiling light's first: rounds whose 64 lanes hold both
    source kinds; baked twice on one context, the second time through the fetch-order table (a launch of at
    most 16 items per lane measures its sources' costs, the next one fetches by them)"""
    sc = _small_box(with_light=True)
    L = O.schedule_with_offsets(sc, BOX_SPA, offsets)
    first_light = int(L["item_begin"][np.flatnonzero(L["is_window"] == 0)[0]])
    lo, hi = first_light - 100, first_light + 100
    assert 0 < lo and hi <= int(L["item_begin"][-1] + L["count"][-1])
    olm, ost = _oracle("small+light", sc, BOX_SPA, offsets, lo, hi)
    ctx = _ctx(sc, BOX_SPA, offsets)
    for _ in range(2):
        lm, st = _bake(torch_cuda, ctx, lo, hi)
        assert np.array_equal(lm, olm)
        _same_counters(st, ost, hi - lo)
    ctx.close()


@pytest.mark.parametrize("accum,fill", [(fmgi.ACCUM_FX3, None), (fmgi.ACCUM_STATE, None), (fmgi.ACCUM_STREAM, 1),
                                        (fmgi.ACCUM_STREAM, 2)])
def test_every_accumulation(torch_cuda, offsets, accum, fill):
    sc = _small_box()
    olm, ost = _oracle("small", sc, BOX_SPA, offsets, 0, 2000)
    ctx = _ctx(sc, BOX_SPA, offsets, accum, **({} if fill is None else {"bucket_fill": fill}))
    lm, st = _bake(torch_cuda, ctx, 0, 2000)
    name = {fmgi.ACCUM_FX3: "AccFx3", fmgi.ACCUM_STATE: "AccState"}.get(accum, "AccScatter" if fill == 1 else "AccShared")
    assert name in ctx.last_bake_kernel, ctx.last_bake_kernel
    assert np.array_equal(lm, olm)
    _same_counters(st, ost, 2000)
    ctx.close()


def test_compact_instance(torch_cuda, box2000, offsets):
    olm, ost = _oracle("box2000", box2000, BOX_SPA, offsets, 0, 4096, port=True)
    ctx = _ctx(box2000, BOX_SPA, offsets)
    lm, st = _bake(torch_cuda, ctx, 0, 4096)
    assert "ScanGridT<true, true, true>" in ctx.last_bake_kernel
    assert np.array_equal(lm, olm)
    _same_counters(st, ost, 4096)
    ctx.close()


def test_option_validation(torch_cuda, offsets):
    """photon_lock is -1, 0 or 1; 0 runs the per-lane loop's instance"""
    sc = _small_box()
    ctx = _ctx(sc, BOX_SPA, offsets)
    for bad in (2, -2):
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):  # FMGI_ERR_ARG
            ctx.set_option("photon_lock", bad)
    _bake(torch_cuda, ctx, 0, 128)  # (the refused values left photon_lock = 1)
    locked = ctx.last_bake_kernel
    ctx.set_option("photon_lock", 0)
    s = torch_cuda.cuda.Stream()
    with torch_cuda.cuda.stream(s):
        lm = torch_cuda.zeros((sc.num_texels, 4), dtype=torch_cuda.int64, device="cuda")
        ctx.bake_items(0, 128, lm.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
    s.synchronize()
    per_lane = ctx.last_bake_kernel
    assert "k_bake<" in per_lane and "k_bake_locked" not in per_lane, per_lane
    assert per_lane == locked.replace("k_bake_locked<", "k_bake<")
    assert np.array_equal(lm.cpu().numpy()[:, :3], _oracle("small", sc, BOX_SPA, offsets, 0, 128)[0])
    ctx.close()
