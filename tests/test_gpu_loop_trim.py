"""The trimmed depth loop of k_bake_locked's AccShared instances (kTrim): the emission and the bounce's sample are two
arms of the scalar branch on depth, the mirror writes dir in place after the diffuse arm, the RNG jumps over the last
bounce's unused sample behind a scalar branch, escapes and the scans they cut short are counted per lane where a
photon escapes (scans = 8 a photon less those), AccShared::append is called where the lane deposits, and the tile
product is the named 24-bit multiply (tile_uv_m24). The other accumulations' locked instances and the per-lane
k_bake loop keep the earlier code; they run here as the same checks' other arms. Per-photon traces, int64 lightmaps
and the four counters against the oracle, bit for bit, where that control can go wrong: a round that holds both
source kinds, rounds with a photon that escapes (its lane must start the next photon from the emitter's basis, and
the counters must still add up), the compact instance, and every accumulation of the locked instance. Every test
sets photon_lock and lattice itself."""
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
# items of box200 at BOX_SPA (schedule from glibc_rand_4096.npy) with a photon that escapes (794, 799 and 798 events)
SHORT_ITEMS = (478, 2549, 5353)


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(maxsize=None)
def _small_box(with_light=False):
    from fmgi import scene

    return scene.box_scene(200, tile_size=2.0, with_light=with_light)


_TRACES = {}


def _oracle_traces(key, sc, offsets, lo, hi):
    """the oracle's (events as uint32 rows, final RNG state) of items [lo, hi): computed once per module"""
    k = (key, lo, hi)
    if k not in _TRACES:
        L = O.schedule_with_offsets(sc, BOX_SPA, offsets)
        out = []
        for w in range(lo, hi):
            li = int(np.searchsorted(L["item_begin"], w, side="right") - 1)
            state = (w - int(L[li]["item_begin"]) + int(L[li]["rng_offset"])) & 0xFFFFFFFF
            oev, ofin = O.trace_item(sc, int(L[li]["source"]), int(L[li]["is_window"]), state)
            oev = oev.view(np.uint32).reshape(len(oev), -1)
            oev.setflags(write=False)
            out.append((oev, ofin))
        _TRACES[k] = out
    return _TRACES[k]


def _ctx(sc, offsets, lock, lattice=-1, accum=fmgi.ACCUM_STREAM, **options):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(accum)
    ctx.set_scene(sc)
    ctx.plan(BOX_SPA, rng_offsets=offsets)
    ctx.set_option("photon_lock", lock)
    ctx.set_option("lattice", lattice)
    if accum == fmgi.ACCUM_STREAM and "bucket_fill" not in options:
        options["bucket_fill"] = 2
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _same_traces(ctx, lock, key, sc, offsets, lo, hi):
    ev, cnt, rngf = ctx.trace_items(lo, hi, fmgi.KERNEL_AUTO)
    print(f"{sc.name} items [{lo}, {hi}): {ctx.last_bake_kernel}")
    assert ("k_bake_locked<" in ctx.last_bake_kernel) == bool(lock), ctx.last_bake_kernel
    assert ctx.stats()["stream_overflow"] == 0
    want = _oracle_traces(key, sc, offsets, lo, hi)
    for k, (oev, ofin) in enumerate(want):
        assert cnt[k] == len(oev), f"item {lo + k}: {cnt[k]} vs {len(oev)} events"
        g = ev[k, : cnt[k]].view(np.uint32)
        assert np.array_equal(g, oev.reshape(g.shape)), f"item {lo + k}"
        assert rngf[k] == ofin, f"item {lo + k}: final RNG"
    return want


@pytest.mark.parametrize("lock", [1, 0])
def test_traces_of_a_round_with_both_source_kinds(torch_cuda, offsets, lock):
    """64 items across the window's last launch and the ceiling light's first: the first sample of every photon
    takes its own emitter's basis (and the window's the folded sampler), never a rect's left from the photon
    before; the final RNG states and the events' rng fields show the last bounce's jump at any other depth"""
    sc = _small_box(with_light=True)
    L = O.schedule_with_offsets(sc, BOX_SPA, offsets)
    first_light = int(L["item_begin"][np.flatnonzero(L["is_window"] == 0)[0]])
    lo, hi = first_light - 32, first_light + 32
    assert 0 < lo and hi <= int(L["item_begin"][-1] + L["count"][-1])
    ctx = _ctx(sc, offsets, lock)
    _same_traces(ctx, lock, "small+light", sc, offsets, lo, hi)
    ctx.close()


@pytest.mark.parametrize("lattice", [0, 1])
@pytest.mark.parametrize("lock", [1, 0])
def test_traces_of_rounds_with_an_escape(torch_cuda, box200, offsets, lock, lattice):
    """the rounds of three items with a photon that escapes: the parked lane starts its next photon from the
    emitter's basis, and the escape is counted where it happens"""
    ctx = _ctx(box200, offsets, lock, lattice)
    for w0 in SHORT_ITEMS:
        b = w0 - w0 % 64
        want = _same_traces(ctx, lock, "box200", box200, offsets, b, b + 64)
        assert ("ScanGridLatticeT" in ctx.last_bake_kernel) == bool(lattice), ctx.last_bake_kernel
        assert len(want[w0 - b][0]) < 800
    ctx.close()


@pytest.mark.parametrize("lock", [1, 0])
def test_traces_of_the_compact_instance(torch_cuda, box2000, offsets, lock):
    """box2000's first 64 items: the compact tables' instances of both photon loops (the locked one's trace instance
    accumulates through AccShared, so it runs the trimmed loop)"""
    ctx = _ctx(box2000, offsets, lock)
    _same_traces(ctx, lock, "box2000", box2000, offsets, 0, 64)
    assert "ScanGridT<true, true, true>" in ctx.last_bake_kernel, ctx.last_bake_kernel
    ctx.close()


@functools.lru_cache(maxsize=None)
def _oracle_769():
    sc = _small_box()
    offs = np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))
    lm, st = O.bake_port(sc, O.schedule_with_offsets(sc, BOX_SPA, offs), 0, 769)
    lm.setflags(write=False)
    return lm, st


@pytest.mark.parametrize("accum,fill,name", [(fmgi.ACCUM_FX3, None, "AccFx3"), (fmgi.ACCUM_STATE, None, "AccState"),
                                             (fmgi.ACCUM_STREAM, 1, "AccScatter"), (fmgi.ACCUM_STREAM, 2, "AccShared")])
def test_lightmap_and_counters_of_every_accumulation(torch_cuda, offsets, accum, fill, name):
    """items [0, 769) (one more than a 768-lane workgroup) of the small box through every accumulation of the locked
    instance: the deposit codes and tile indices of the trimmed loop (AccShared) and of the untrimmed one (the
    others), and the counters, which the trimmed loop derives from its escapes instead of counting per scan"""
    sc = _small_box()
    olm, ost = _oracle_769()
    ctx = _ctx(sc, offsets, 1, accum=accum, **({} if fill is None else {"bucket_fill": fill}))
    ctx.reset_stats()
    s = torch_cuda.cuda.Stream()
    with torch_cuda.cuda.stream(s):
        lm = torch_cuda.zeros((sc.num_texels, 4), dtype=torch_cuda.int64, device="cuda")
        ctx.bake_items(0, 769, lm.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
    s.synchronize()
    st = ctx.stats()
    kernel = ctx.last_bake_kernel
    print(f"{sc.name} items [0, 769): {kernel}")
    assert "k_bake_locked<" in kernel and "ScanGridT<true, true, false>" in kernel and name in kernel, kernel
    assert st["stream_overflow"] == 0
    got = lm.cpu().numpy()
    assert not got[:, 3].any()
    assert np.array_equal(got[:, :3], olm)
    assert st["photons"] == 100 * 769
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["scans"] == st["deposits"] + st["escapes"]
    ctx.close()
