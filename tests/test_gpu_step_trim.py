"""The scan of k_bake_locked's trimmed loop (the AccShared instances): phase 1 runs its three far-plane
band tests behind one guard on the median of the three planes' distances, and phase 2's exact test has no early
return (intersect_exact_uv_flat). Both leave every valid lane's arithmetic as it was, so everything here is compared
by equality: the lightmap and the scan, deposit and escape counts against the oracle, and `tests`, `ties`, `invalid`
and `rescans` against the locked AccScatter instance and the per-lane k_bake loop, which keep the earlier scan
(`tests` counts the candidate tests: a far-plane visit the guard skipped would lower it). The scenes are those where
the changed paths run: a box of six rects and box200 at 4 texels/m² (far planes inside the band along edges and in
corners: ties and invalid winners), and emitters outside the box and tilted (photons that escape, i.e. no plane in
front: fm = INFINITY, and lanes behind planes). The first 256 items of every source."""
import functools
import os

import numpy as np
import pytest

import emitter_scenes
import fm_oracle as O
import fmgi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOX_SPA = 172_413_793
ITEMS = 256
COUNTERS = ("photons", "scans", "deposits", "escapes")
SCAN_COUNTERS = ("tests", "rescans_tie", "rescans_invalid", "exact_rescans")
SCENES = ("box8", "box200", "outside", "tilted_emitters")
# (photon_lock, bucket_fill): the trimmed loop first, then the two that keep the earlier scan
ARMS = {"locked_shared": (1, 2), "locked_scatter": (1, 1), "lane": (0, 2)}


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(None)
def _scene(name):
    from fmgi import scene

    if name == "box8":
        return scene.box_scene(8, tile_size=4.0)
    if name == "box200":
        return scene.box_scene(200, tile_size=4.0)
    return emitter_scenes.get(name)


def _spa(name):
    import bake_scenes

    return BOX_SPA if name.startswith("box") else bake_scenes.SPA


@functools.lru_cache(None)
def _schedule(name):
    return O.schedule_with_offsets(_scene(name), _spa(name), np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))


@functools.lru_cache(None)
def _ranges(name):
    """the first ITEMS items of every source"""
    L = _schedule(name)
    b = emitter_scenes.source_begins(L) + [int(L["item_begin"][-1] + L["count"][-1])]
    return tuple((b[s], min(b[s] + ITEMS, b[s + 1])) for s in range(len(b) - 1))


@functools.lru_cache(None)
def _oracle(name):
    """the oracle's lightmap and counters of the scene's ranges together; computed once and never modified"""
    lm = np.zeros((_scene(name).num_texels, 3), np.int64)
    total = dict.fromkeys(COUNTERS, 0)
    for lo, hi in _ranges(name):
        l, st = O.bake_port(_scene(name), _schedule(name), lo, hi)
        lm += l
        for k in COUNTERS:
            total[k] += st[k]
    lm.setflags(write=False)
    return lm, total


def _ctx(name, offsets, lock, fill):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(fmgi.ACCUM_STREAM)
    ctx.set_scene(_scene(name))
    ctx.plan(_spa(name), rng_offsets=offsets)
    ctx.set_option("photon_lock", lock)
    ctx.set_option("bucket_fill", fill)
    return ctx


_BAKED = {}


def _bake(torch, name, offsets, arm):
    """(lightmap [T, 3], stats, the instance's name without spaces) of the scene's ranges through one arm, once"""
    if (name, arm) not in _BAKED:
        lock, fill = ARMS[arm]
        ctx = _ctx(name, offsets, lock, fill)
        ctx.reset_stats()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            lm = torch.zeros((ctx.scene.num_texels, 4), dtype=torch.int64, device="cuda")
            for lo, hi in _ranges(name):
                ctx.bake_items(lo, hi, lm.data_ptr(), fmgi.KERNEL_GRID, s.cuda_stream)
        s.synchronize()
        st = ctx.stats()
        kernel = ctx.last_bake_kernel.replace(" ", "")
        print(f"{name} {arm} items {_ranges(name)}: {ctx.last_bake_kernel} "
              + " ".join(f"{k} {st[k]}" for k in COUNTERS + SCAN_COUNTERS))
        assert st["stream_overflow"] == 0
        got = lm.cpu().numpy()
        assert not got[:, 3].any()
        got = got[:, :3].copy()
        got.setflags(write=False)
        ctx.close()
        _BAKED[name, arm] = got, st, kernel
    return _BAKED[name, arm]


@pytest.mark.parametrize("name", SCENES)
def test_trimmed_scan_equals_the_oracle(torch_cuda, offsets, name):
    lm, st, kernel = _bake(torch_cuda, name, offsets, "locked_shared")
    assert "k_bake_locked<" in kernel and "AccShared" in kernel and "ScanGridT<true,true,false>" in kernel, kernel
    olm, ost = _oracle(name)
    bad = np.flatnonzero((lm != olm).any(axis=1))
    assert bad.size == 0, f"{name}: {bad.size} texels differ, first {bad[:8]}"
    assert st["photons"] == 100 * sum(hi - lo for lo, hi in _ranges(name))
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["scans"] == st["deposits"] + st["escapes"]
    if name == "outside":
        assert st["escapes"] > 0  # photons emitted above the ceiling leave: no plane in front of them


@pytest.mark.parametrize("other", ["locked_scatter", "lane"])
@pytest.mark.parametrize("name", SCENES)
def test_trimmed_scan_counts_what_the_earlier_scan_counts(torch_cuda, offsets, name, other):
    """tests, ties, invalid and rescans of the trimmed loop's scan against an instance that keeps the scan as it was"""
    lm, st, kernel = _bake(torch_cuda, name, offsets, "locked_shared")
    olm, ost, okernel = _bake(torch_cuda, name, offsets, other)
    assert "AccShared" in kernel and "k_bake_locked<" in kernel, kernel
    if other == "locked_scatter":
        assert "k_bake_locked<" in okernel and "AccScatter" in okernel, okernel
    else:
        assert "k_bake<" in okernel, okernel
    assert kernel.split("<", 1)[1].split(",(anonymousnamespace)::Acc")[0] == \
        okernel.split("<", 1)[1].split(",(anonymousnamespace)::Acc")[0], (kernel, okernel)  # the same scan type
    assert np.array_equal(lm, olm)
    for k in COUNTERS + SCAN_COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    if name in ("box8", "box200"):
        assert st["rescans_tie"] + st["rescans_invalid"] > 0  # the band path ran


def test_traces_on_the_six_rect_box(torch_cuda, offsets):
    """per-bounce events and final RNG states of box8's first 64 items through the locked trace instance (it
    accumulates through AccShared: the trimmed loop)"""
    sc, L = _scene("box8"), _schedule("box8")
    ctx = _ctx("box8", offsets, 1, 2)
    ev, cnt, rngf = ctx.trace_items(0, 64, fmgi.KERNEL_GRID)  # (AUTO takes the fast scan for six rects)
    kernel = ctx.last_bake_kernel
    print(f"box8 items [0, 64): {kernel}")
    assert "k_bake_locked<" in kernel and "AccShared" in kernel, kernel
    assert ctx.stats()["stream_overflow"] == 0
    for w in range(64):
        li = int(np.searchsorted(L["item_begin"], w, side="right") - 1)
        state = (w - int(L[li]["item_begin"]) + int(L[li]["rng_offset"])) & 0xFFFFFFFF
        oev, ofin = O.trace_item(sc, int(L[li]["source"]), int(L[li]["is_window"]), state)
        oev = oev.view(np.uint32).reshape(len(oev), -1)
        assert cnt[w] == len(oev), f"item {w}: {cnt[w]} vs {len(oev)} events"
        g = ev[w, : cnt[w]].view(np.uint32)
        assert np.array_equal(g, oev.reshape(g.shape)), f"item {w}"
        assert rngf[w] == ofin, f"item {w}: final RNG"
    ctx.close()
