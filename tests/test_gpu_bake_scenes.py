"""The bake's scans on the scenes of tests/bake_scenes.py, against the oracle, everything by equality: int64
lightmaps, the four counters and per-photon traces, for every scan and accumulation, on the paths that the closed
boxes and the layouts never take:

  open_box                the closed-box instances (ScanGridT<true, true, false>) and the wave-locked loop on a scene
                          that 98 % of the photons leave: whole waves parked, one (axis, class) list empty
  tilted*, open_tilted    ScanGridT<true, false, false>: the Axes phase 1, then the exact loop over the general
                          rects, and ordered_exact's general loop; the other scans' general lists
  crossing                ScanGridT<false, false, false> through grid_phase1_sorted (four plane slots)
  stacked3                ties of 4 coincident rects that ordered_exact resolves in index order
  stacked14, _200         ties of 15: ordered_exact runs out of rounds and ScanExact::literal decides; cells whose
                          overflow records (`rest`, `grecs`, `gridx`) are read in bulk, staged and from global memory

What each scene is to the host tables and to the oracle is checked on the CPU (tests/test_bake_scenes_host.py); the
oracle is pinned to the reference kernel on open_box, tilted12 and stacked14 (tests/test_reference_pin.py)."""
import functools
import os

import numpy as np
import pytest

import bake_scenes
import fm_oracle as O
import fmgi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SPA = bake_scenes.SPA
COUNTERS = ("photons", "scans", "deposits", "escapes")
LAUNCH_ITEMS = 25600  # items per reference launch (256 x 100)
RANGES = ((0, 4096), (LAUNCH_ITEMS - 64, LAUNCH_ITEMS + 64))  # the second straddles the first launch boundary
TRACE_RANGES = ((0, 64), (LAUNCH_ITEMS - 32, LAUNCH_ITEMS + 32))
KERNELS = [fmgi.KERNEL_EXACT, fmgi.KERNEL_FAST, fmgi.KERNEL_GRID, fmgi.KERNEL_HYBRID]
KERNEL_IDS = {fmgi.KERNEL_EXACT: "exact", fmgi.KERNEL_FAST: "fast", fmgi.KERNEL_GRID: "grid", fmgi.KERNEL_HYBRID: "hybrid"}
# the scan type in the instance's name (a kernel that does not fit LDS would run another: none of these scenes')
SCAN_OF = {fmgi.KERNEL_EXACT: "ScanExact", fmgi.KERNEL_FAST: "ScanFastT<", fmgi.KERNEL_GRID: "ScanGridT<",
           fmgi.KERNEL_HYBRID: "ScanHybridT<"}
# the grid scan's instance under STREAM: a scene of one plane slot per axis takes the closed box's (Axes), staged
# when it has no general rects (bake_common: the staged instance has no path for them); crossing has two slots on
# x and y and takes the general one
GRID_INSTANCE = {
    "open_box": "ScanGridT<true,true,false>", "stacked3": "ScanGridT<true,true,false>",
    "stacked14": "ScanGridT<true,true,false>", "stacked14_200": "ScanGridT<true,true,false>",
    "tilted1": "ScanGridT<true,false,false>", "tilted12": "ScanGridT<true,false,false>",
    "tilted57": "ScanGridT<true,false,false>", "open_tilted": "ScanGridT<true,false,false>",
    "crossing": "ScanGridT<false,false,false>",
}


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(None)
def _schedule(name):
    return O.schedule_with_offsets(bake_scenes.get(name), SPA, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))


@functools.lru_cache(None)
def _oracle(name, lo, hi):
    """the oracle's (lightmap, stats) of items [lo, hi), computed once per module and never modified (O.bake_port:
    the oracle's restatement, bit-identical on these scenes by tests/test_bake_scenes_host.py)"""
    lm, st = O.bake_port(bake_scenes.get(name), _schedule(name), lo, hi)
    lm.setflags(write=False)
    return lm, st


@functools.lru_cache(None)
def _oracle_trace(name, w):
    sc, L = bake_scenes.get(name), _schedule(name)
    li = int(np.searchsorted(L["item_begin"], w, side="right") - 1)
    state = (w - int(L[li]["item_begin"]) + int(L[li]["rng_offset"])) & 0xFFFFFFFF
    ev, fin = O.trace_item(sc, int(L[li]["source"]), int(L[li]["is_window"]), state)
    ev.setflags(write=False)
    return ev, fin


def _ctx(name, offsets, accum=fmgi.ACCUM_STREAM, **options):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(accum)
    ctx.set_scene(bake_scenes.get(name))
    assert ctx.plan(SPA, rng_offsets=offsets) == 10_000_128
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _bake(torch, ctx, lo, hi, kernel):
    """bakes items [lo, hi) on a fresh lightmap"""
    ctx.reset_stats()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lm = torch.zeros((ctx.scene.num_texels, 4), dtype=torch.int64, device="cuda")
        ctx.bake_items(lo, hi, lm.data_ptr(), kernel, s.cuda_stream)
    s.synchronize()
    st = ctx.stats()
    print(f"{ctx.scene.name} items [{lo}, {hi}): {ctx.last_bake_kernel} tests/scans {st['tests'] / max(st['scans'], 1):.3f} "
          f"ties {st['rescans_tie']} invalid {st['rescans_invalid']}")
    assert st["stream_overflow"] == 0
    got = lm.cpu().numpy()
    assert not got[:, 3].any()
    return got[:, :3], st


def _same_counters(st, ost, items):
    assert st["photons"] == 100 * items
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["scans"] == st["deposits"] + st["escapes"]


def _name(ctx):
    """the last bake's instance, spaces dropped (demanglers differ in how they close nested template lists)"""
    return ctx.last_bake_kernel.replace(" ", "")


def _check_ranges(torch, ctx, name, kernel, ranges=RANGES):
    for lo, hi in ranges:
        olm, ost = _oracle(name, lo, hi)
        lm, st = _bake(torch, ctx, lo, hi, kernel)
        assert SCAN_OF[kernel] in _name(ctx), ctx.last_bake_kernel
        bad = np.flatnonzero((lm != olm).any(axis=1))
        assert bad.size == 0, f"{name} items [{lo}, {hi}): {bad.size} texels differ, first {bad[:8]}"
        _same_counters(st, ost, hi - lo)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS.get)
@pytest.mark.parametrize("name", bake_scenes.NAMES)
def test_every_scan_on_every_scene(torch_cuda, offsets, name, kernel):
    ctx = _ctx(name, offsets)
    _check_ranges(torch_cuda, ctx, name, kernel)
    if kernel == fmgi.KERNEL_GRID:
        assert GRID_INSTANCE[name] in _name(ctx) and "Lattice" not in _name(ctx), ctx.last_bake_kernel
    ctx.close()


@pytest.mark.parametrize("accum", [fmgi.ACCUM_FX3, fmgi.ACCUM_STATE], ids=["fx3", "state"])
@pytest.mark.parametrize("name", bake_scenes.NAMES)
def test_grid_scan_fx3_and_state(torch_cuda, offsets, name, accum):
    ctx = _ctx(name, offsets, accum)
    _check_ranges(torch_cuda, ctx, name, fmgi.KERNEL_GRID)
    assert {fmgi.ACCUM_FX3: "AccFx3", fmgi.ACCUM_STATE: "AccState"}[accum] in _name(ctx), ctx.last_bake_kernel
    ctx.close()


LOOP_RANGES = ((0, 1), (0, 63), (0, 65), (0, 769), (5, 1000), (-100, None))
ACCUMS = [(fmgi.ACCUM_STREAM, 1), (fmgi.ACCUM_STREAM, 2), (fmgi.ACCUM_FX3, None), (fmgi.ACCUM_STATE, None)]


@pytest.mark.parametrize("accum,fill", ACCUMS, ids=["scatter", "shared", "fx3", "state"])
@pytest.mark.parametrize("lock", [0, 1], ids=["lane", "locked"])
@pytest.mark.parametrize("name", ["open_box", "stacked14", "stacked14_200"])
def test_both_photon_loops(torch_cuda, offsets, name, lock, accum, fill):
    """fewer items than a wave's round, one more than a round, one more than a 768-lane workgroup, a shard that
    starts off a round, and the schedule's last 100 items (as tests/test_gpu_wave_locked.py on box200), where most
    lanes of the wave-locked loop are parked (open_box) or every floor hit falls back twice (the stacks)"""
    ctx = _ctx(name, offsets, accum, photon_lock=lock, **({} if fill is None else {"bucket_fill": fill}))
    acc = {fmgi.ACCUM_FX3: "AccFx3", fmgi.ACCUM_STATE: "AccState"}.get(accum, "AccScatter" if fill == 1 else "AccShared")
    for lo, hi in LOOP_RANGES:
        if hi is None:
            lo, hi = ctx.total_items + lo, ctx.total_items
        olm, ost = _oracle(name, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi, fmgi.KERNEL_GRID)
        assert ("k_bake_locked<" in _name(ctx)) == bool(lock) and "k_bake" in _name(ctx), ctx.last_bake_kernel
        assert acc in _name(ctx), ctx.last_bake_kernel
        assert np.array_equal(lm, olm), (lo, hi)
        _same_counters(st, ost, hi - lo)
    if name == "open_box":  # two launches sum to one
        olm, ost = _oracle(name, 0, 700)
        a, sa = _bake(torch_cuda, ctx, 0, 300, fmgi.KERNEL_GRID)
        b, sb = _bake(torch_cuda, ctx, 300, 700, fmgi.KERNEL_GRID)
        assert np.array_equal(a + b, olm)
        for k in COUNTERS:
            assert sa[k] + sb[k] == ost[k], k
    ctx.close()


def _compare_traces(ctx, name, lo, hi, kernel):
    """events, event counts and final RNG states of items [lo, hi), as tests/test_gpu_parity.py"""
    ev, cnt, rngf = ctx.trace_items(lo, hi, kernel)
    assert ctx.stats()["stream_overflow"] == 0
    for w in range(lo, hi):
        oev, ofin = _oracle_trace(name, w)
        k = w - lo
        assert cnt[k] == len(oev), f"item {w}: {cnt[k]} vs {len(oev)} events"
        g = ev[k, : cnt[k]].view(np.uint32).ravel()
        o = oev.view(np.uint32).ravel()
        if not np.array_equal(g, o):
            e = int(np.flatnonzero(g != o)[0]) // (ev.dtype.itemsize // 4)
            raise AssertionError(f"item {w} event {e}: got {ev[k, e]}, oracle {oev[e]}")
        assert rngf[k] == ofin, f"item {w}: final RNG"


TRACE_CASES = [(n, k, -1) for n in ("open_box", "open_tilted", "tilted12", "crossing", "stacked14") for k in KERNELS
               if (n, k) != ("open_box", fmgi.KERNEL_GRID)] + [("open_box", fmgi.KERNEL_GRID, 0), ("open_box", fmgi.KERNEL_GRID, 1)]


@pytest.mark.parametrize("name,kernel,lock", TRACE_CASES,
                         ids=[f"{n}-{KERNEL_IDS[k]}" + {-1: "", 0: "-lane", 1: "-locked"}[l] for n, k, l in TRACE_CASES])
def test_traces(torch_cuda, offsets, name, kernel, lock):
    """(the open scenes' items end early: about 250 events instead of 800)"""
    ctx = _ctx(name, offsets, photon_lock=lock)
    for lo, hi in TRACE_RANGES:
        _compare_traces(ctx, name, lo, hi, kernel)
        assert SCAN_OF[kernel] in _name(ctx), ctx.last_bake_kernel
        if lock >= 0:
            assert ("k_bake_locked<" in _name(ctx)) == bool(lock), ctx.last_bake_kernel
    if name.startswith("open"):
        assert max(len(_oracle_trace(name, w)[0]) for w in range(64)) < 800
    ctx.close()


@pytest.mark.parametrize("name,hi", [("stacked14", 4096), ("stacked14_200", 1024)])
def test_a_stack_of_fifteen_takes_the_fallback(torch_cuda, offsets, name, hi):
    """every hit on the stack has 15 phase-1 candidates with one key: the separation test fails, ordered_exact runs
    out of its 12 rounds, and the literal scan gives the hit to the lowest index: at least one rescan per deposit
    on the duplicated rect, and none of them on a copy's texels (the lightmap equals the oracle's)"""
    sc = bake_scenes.get(name)
    olm, ost, cnt = O.bake(sc, _schedule(name), 0, hi, counts=True)
    (d0, d1), (c0, c1) = bake_scenes.stack_texels(name)
    on_stack = int(cnt[d0:d1].sum())
    assert on_stack >= 1000 and not cnt[c0:c1].any()
    ctx = _ctx(name, offsets)
    lm, st = _bake(torch_cuda, ctx, 0, hi, fmgi.KERNEL_GRID)
    assert GRID_INSTANCE[name] in _name(ctx), ctx.last_bake_kernel
    assert np.array_equal(lm, olm)
    assert not lm[c0:c1].any()
    _same_counters(st, ost, hi)
    assert st["rescans_tie"] + st["rescans_invalid"] >= on_stack, (st["rescans_tie"], st["rescans_invalid"], on_stack)
    ctx.close()


@pytest.mark.parametrize("name", ["open_box", "stacked14"])
def test_lattice_option_without_a_lattice(torch_cuda, offsets, name):
    """lattice = 1 on a scene of one plane per axis and class that is no verified lattice (a class without records;
    a cell of 15) runs the ordinary instance: the same kernel, lightmap and statistics as lattice = 0 (as
    tests/test_gpu_lattice.py test_scenes_without_a_lattice_bake_as_before)"""
    res = {}
    for lattice in (0, 1):
        ctx = _ctx(name, offsets, lattice=lattice)
        assert len(ctx.lattice_tables()["lattice"]) == 0
        lm, st = _bake(torch_cuda, ctx, 0, 512, fmgi.KERNEL_AUTO)
        res[lattice] = (lm, st, ctx.last_bake_kernel)
        ctx.close()
    assert res[0][2] == res[1][2] and "Lattice" not in res[1][2], (res[0][2], res[1][2])
    assert np.array_equal(res[0][0], res[1][0])
    # (every statistic but bucket_fallback_codes, which counts how often a wave ran ahead of its tile's opener: a
    # matter of timing on a lightmap of one or two fold tiles, tests/test_gpu_lattice.py _ctx)
    for k in res[0][1]:
        assert k == "bucket_fallback_codes" or res[0][1][k] == res[1][1][k], (k, res[0][1][k], res[1][1][k])
    assert np.array_equal(res[1][0], _oracle(name, 0, 512)[0])
