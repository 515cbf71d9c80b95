"""The bake on the scenes of tests/emitter_scenes.py, against the oracle, everything by equality: int64 lightmaps, the
four counters and per-photon traces, for every scan, accumulation and photon loop, on emitters that the boxes, the
layouts and tests/bake_scenes.py never have:

  skylight, lamps      windows and lights through either branch of the sampler basis (cl_sampler_basis in
                       k_scene_setup: photonmap.cl:43-48, :65-70)
  tilted_emitters      width, height and n without a zero component: the basis, the first direction and the emission
                       point `pos + width*dx + height*dy + dir*1e-5` (photonmap.cl:181; three copies, in k_bake and
                       k_bake_locked) are sums of three non-zero terms, whose order and rounding now show
  threshold(_panels)   |n.z| on either side of `>= 0.999999f`, as emitters and as walls
  outside              first rays that start outside the walls' bounding box: the closed-box scans (the staged, the
                       lattice and the compact instance, both photon loops) enter through back faces; a lamp whose
                       photons partly leave at once
  tilted12_emitters    the tilted emitters through the Axes phase 1 + general loop

Ranges start 37 items before a source's first item, so that waves and 768-lane workgroups hold lanes of two sources,
and of a window and a light. What each scene is to the host tables and to the oracle is checked on the CPU
(tests/test_emitter_scenes_host.py); the oracle is pinned to the reference kernel on lamps, tilted_emitters, threshold
and outside (tests/test_reference_pin.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bake_scenes
import emitter_scenes
import fm_oracle as O
import fmgi
from conftest import GOLDEN
from test_gpu_bake_scenes import (ACCUMS, KERNEL_IDS, KERNELS, LOOP_RANGES, SCAN_OF, _bake, _name,
                                  _same_counters)

pytestmark = pytest.mark.gpu

SPA = bake_scenes.SPA
STAGED, GENERAL, COMPACT = "ScanGridT<true,true,false>", "ScanGridT<true,false,false>", "ScanGridT<true,true,true>"
# the grid scan's instance under STREAM: the staged closed box's on the box's walls (its lattice form included:
# ScanGridLatticeT<ScanGridT<true,true,false>>), the Axes phase 1 without staging where there are general rects
GRID_INSTANCE = {n: STAGED for n in emitter_scenes.BOX}
GRID_INSTANCE.update(threshold_panels=GENERAL, tilted12_emitters=GENERAL)
CLOSED = ("lamps", "tilted_emitters", "threshold", "outside")  # of the traced scenes: those the staged instance runs


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(None)
def _scene(key):
    """'name' or 'name@lattice' / 'name@compact' / 'name@fine' (emitter_scenes.variant)"""
    name, _, kind = key.partition("@")
    return emitter_scenes.variant(name, kind) if kind else emitter_scenes.get(name)


@functools.lru_cache(None)
def _schedule(key):
    return O.schedule_with_offsets(_scene(key), SPA, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))


@functools.lru_cache(None)
def _begins(key):
    """b_s: the first item of every source; then the schedule's item count"""
    L = _schedule(key)
    return emitter_scenes.source_begins(L) + [int(L["item_begin"][-1] + L["count"][-1])]


@functools.lru_cache(None)
def _oracle(key, lo, hi):
    """the oracle's (lightmap, stats) of items [lo, hi), computed once per module and never modified (O.bake_port:
    the oracle's restatement, bit-identical on these scenes by tests/test_emitter_scenes_host.py)"""
    lm, st = O.bake_port(_scene(key), _schedule(key), lo, hi)
    lm.setflags(write=False)
    return lm, st


@functools.lru_cache(None)
def _oracle_trace(key, w):
    sc, L = _scene(key), _schedule(key)
    li = int(np.searchsorted(L["item_begin"], w, side="right") - 1)
    state = (w - int(L[li]["item_begin"]) + int(L[li]["rng_offset"])) & 0xFFFFFFFF
    ev, fin = O.trace_item(sc, int(L[li]["source"]), int(L[li]["is_window"]), state)
    ev.setflags(write=False)
    return ev, fin


def _ranges(key):
    """(0, 2048), 128 items over every source boundary from an odd lower bound, and the schedule's last 100"""
    b = _begins(key)
    return [(0, 2048)] + [(s - 37, s + 91) for s in b[1:-1]] + [(b[-1] - 100, b[-1])]


def _ctx(key, offsets, accum=fmgi.ACCUM_STREAM, **options):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(accum)
    ctx.set_scene(_scene(key))
    assert ctx.plan(SPA, rng_offsets=offsets) == _begins(key)[-1]
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _check_ranges(torch, ctx, key, kernel, ranges):
    for lo, hi in ranges:
        olm, ost = _oracle(key, lo, hi)
        lm, st = _bake(torch, ctx, lo, hi, kernel)
        assert SCAN_OF[kernel] in _name(ctx), ctx.last_bake_kernel
        bad = np.flatnonzero((lm != olm).any(axis=1))
        assert bad.size == 0, f"{key} items [{lo}, {hi}): {bad.size} texels differ, first {bad[:8]}"
        _same_counters(st, ost, hi - lo)


def test_ranges_hold_two_sources():
    """every boundary range has items of two sources, and in lamps, tilted_emitters, threshold and outside one of
    them holds a window's and a light's"""
    for name in emitter_scenes.NAMES:
        L = _schedule(name)
        src_of = lambda w: int(L["source"][np.searchsorted(L["item_begin"], w, side="right") - 1])  # noqa: E731
        mids = _ranges(name)[1:-1]
        assert len(mids) == len(_scene(name).sources) - 1
        for lo, hi in mids:
            assert lo % 2 == 1 and src_of(lo) + 1 == src_of(hi - 1)
        if name != "skylight":
            nw = len(_scene(name).windows)
            assert any(src_of(lo) < nw <= src_of(hi - 1) for lo, hi in mids)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS.get)
@pytest.mark.parametrize("name", emitter_scenes.NAMES)
def test_every_scan_on_every_scene(torch_cuda, offsets, name, kernel):
    ctx = _ctx(name, offsets)
    _check_ranges(torch_cuda, ctx, name, kernel, _ranges(name))
    if kernel == fmgi.KERNEL_GRID:
        assert GRID_INSTANCE[name] in _name(ctx), ctx.last_bake_kernel
    ctx.close()


@pytest.mark.parametrize("accum", [fmgi.ACCUM_FX3, fmgi.ACCUM_STATE], ids=["fx3", "state"])
@pytest.mark.parametrize("name", emitter_scenes.NAMES)
def test_grid_scan_fx3_and_state(torch_cuda, offsets, name, accum):
    ctx = _ctx(name, offsets, accum)
    _check_ranges(torch_cuda, ctx, name, fmgi.KERNEL_GRID, _ranges(name))
    assert {fmgi.ACCUM_FX3: "AccFx3", fmgi.ACCUM_STATE: "AccState"}[accum] in _name(ctx), ctx.last_bake_kernel
    ctx.close()


@pytest.mark.parametrize("accum,fill", ACCUMS, ids=["scatter", "shared", "fx3", "state"])
@pytest.mark.parametrize("lock", [0, 1], ids=["lane", "locked"])
@pytest.mark.parametrize("name", ["lamps", "tilted_emitters", "outside"])
def test_both_photon_loops(torch_cuda, offsets, name, lock, accum, fill):
    """tests/test_gpu_bake_scenes.py's ranges (fewer items than a wave's round, one more than a round, one more than
    a 768-lane workgroup, a shard that starts off a round), begun in the window's last five items and run into the
    first lamp's, and the schedule's last 100 items. outside parks lanes from the first event on."""
    ctx = _ctx(name, offsets, accum, photon_lock=lock, **({} if fill is None else {"bucket_fill": fill}))
    acc = {fmgi.ACCUM_FX3: "AccFx3", fmgi.ACCUM_STATE: "AccState"}.get(accum, "AccScatter" if fill == 1 else "AccShared")
    b = _begins(name)
    for lo, hi in LOOP_RANGES:
        lo, hi = (b[-1] + lo, b[-1]) if hi is None else (b[1] - 5 + lo, b[1] - 5 + hi)
        olm, ost = _oracle(name, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi, fmgi.KERNEL_GRID)
        assert ("k_bake_locked<" in _name(ctx)) == bool(lock) and "k_bake" in _name(ctx), ctx.last_bake_kernel
        assert acc in _name(ctx) and (STAGED in _name(ctx) or not lock), ctx.last_bake_kernel
        assert np.array_equal(lm, olm), (lo, hi)
        _same_counters(st, ost, hi - lo)
    ctx.close()


@pytest.mark.parametrize("accum,fill", ACCUMS, ids=["scatter", "shared", "fx3", "state"])
@pytest.mark.parametrize("lock", [0, 1], ids=["lane", "locked"])
def test_emission_point_on_a_fine_lightmap(torch_cuda, offsets, lock, accum, fill):
    """tilted_emitters' sources on box200 at 200 texels/m², the window's first 4,096 items and the lamp's first
    2,048, for the emission point's three copies: k_bake's (the per-lane loop), k_bake_locked's trimmed arm
    (AccShared) and its other arm. An oracle whose emission point is associated `pos + (width*dx + height*dy)`
    differs from the oracle on 30 texels of the first range and 298 of the second; on the 2 texels/m² scene it
    differs on none of items [0, 2048)."""
    key = "tilted_emitters@fine"
    ctx = _ctx(key, offsets, accum, photon_lock=lock, **({} if fill is None else {"bucket_fill": fill}))
    b = _begins(key)
    for lo, hi in ((0, 4096), (b[1], b[1] + 2048)):
        olm, ost = _oracle(key, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi, fmgi.KERNEL_GRID)
        assert ("k_bake_locked<" in _name(ctx)) == bool(lock), ctx.last_bake_kernel
        bad = np.flatnonzero((lm != olm).any(axis=1))
        assert bad.size == 0, f"items [{lo}, {hi}): {bad.size} texels differ, first {bad[:8]}"
        _same_counters(st, ost, hi - lo)
    ctx.close()


def _runs_lattice(ctx, lock, compact):
    """tests/test_gpu_lattice.py _runs: the lattice instance of the staged / compact closed box with this loop"""
    want = (f"{'k_bake_locked' if lock else 'k_bake'}<(anonymousnamespace)::ScanGridLatticeT<(anonymousnamespace)::"
            f"ScanGridT<true,true,{'true' if compact else 'false'}>>,")
    return want in _name(ctx)


@pytest.mark.parametrize("lattice", [0, 1])
@pytest.mark.parametrize("lock", [0, 1], ids=["lane", "locked"])
@pytest.mark.parametrize("name", ["outside", "tilted_emitters"])
def test_lattice_instances(torch_cuda, offsets, name, lock, lattice):
    """the emitters on the box of tests/test_gpu_lattice.py (4 texels/m²): a first ray from outside meets the
    nearest plane off the lattice (clamped, never `sure`) and takes the cell path"""
    key = name + "@lattice"
    ctx = _ctx(key, offsets, photon_lock=lock, lattice=lattice)
    assert len(ctx.lattice_tables()["lattice"]) == 6
    b = _begins(key)
    for lo, hi in ((0, 512), (b[1] - 37, b[1] + 91)):
        olm, ost = _oracle(key, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi, fmgi.KERNEL_GRID)
        if lattice:
            assert _runs_lattice(ctx, lock, False), ctx.last_bake_kernel
        else:
            assert "ScanGridLatticeT" not in _name(ctx) and "<(anonymousnamespace)::" + STAGED + "," in _name(ctx)
            assert ("k_bake_locked<" in _name(ctx)) == bool(lock), ctx.last_bake_kernel
        assert np.array_equal(lm, olm), (lo, hi)
        _same_counters(st, ost, hi - lo)
    ctx.close()


@pytest.mark.parametrize("name", ["outside", "tilted_emitters"])
def test_compact_instance(torch_cuda, offsets, name):
    """the emitters on box2000's walls: the compact closed box's instance, as tests/test_gpu_configs.py asserts"""
    key = name + "@compact"
    ctx = _ctx(key, offsets)
    b = _begins(key)
    for lo, hi in ((0, 512), (b[1] - 37, b[1] + 91)):
        olm, ost = _oracle(key, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi, fmgi.KERNEL_AUTO)
        assert COMPACT in _name(ctx), ctx.last_bake_kernel
        assert np.array_equal(lm, olm), (lo, hi)
        _same_counters(st, ost, hi - lo)
    ctx.close()


def _compare_traces(ctx, key, lo, hi, kernel):
    """events, event counts and final RNG states of items [lo, hi), as tests/test_gpu_parity.py. A photon's first
    event carries what emission did: its rect, its texel and the RNG state after the direction draw."""
    ev, cnt, rngf = ctx.trace_items(lo, hi, kernel)
    assert ctx.stats()["stream_overflow"] == 0
    for w in range(lo, hi):
        oev, ofin = _oracle_trace(key, w)
        k = w - lo
        assert cnt[k] == len(oev), f"item {w}: {cnt[k]} vs {len(oev)} events"
        g = ev[k, : cnt[k]].view(np.uint32).ravel()
        o = oev.view(np.uint32).ravel()
        if not np.array_equal(g, o):
            e = int(np.flatnonzero(g != o)[0]) // (ev.dtype.itemsize // 4)
            raise AssertionError(f"item {w} event {e}: got {ev[k, e]}, oracle {oev[e]}")
        assert rngf[k] == ofin, f"item {w}: final RNG"


TRACE_CASES = ([(n, k, -1) for n in CLOSED + ("tilted12_emitters",) for k in KERNELS
                if k != fmgi.KERNEL_GRID or n not in CLOSED]
               + [(n, fmgi.KERNEL_GRID, lock) for n in CLOSED for lock in (0, 1)])


@pytest.mark.parametrize("name,kernel,lock", TRACE_CASES,
                         ids=[f"{n}-{KERNEL_IDS[k]}" + {-1: "", 0: "-lane", 1: "-locked"}[l] for n, k, l in TRACE_CASES])
def test_traces(torch_cuda, offsets, name, kernel, lock):
    """the first 32 items of every source"""
    ctx = _ctx(name, offsets, photon_lock=lock)
    for b in _begins(name)[:-1]:
        _compare_traces(ctx, name, b, b + 32, kernel)
        assert SCAN_OF[kernel] in _name(ctx), ctx.last_bake_kernel
        if lock >= 0:
            assert ("k_bake_locked<" in _name(ctx)) == bool(lock), ctx.last_bake_kernel
    if name == "outside":  # the straddling lamp's first item ends early (776 events of 800)
        assert len(_oracle_trace(name, _begins(name)[2])[0]) < 800
    ctx.close()


@pytest.mark.parametrize("name,launches", [("tilted_emitters", 2), ("outside", 3)])
def test_drop_in(torch_cuda, libc, name, launches):
    """performGlobalIlluminationCl at spa 65,000 (as tests/test_gpu_parity.py test_drop_in_entry_points): it builds
    its schedule and its source table from the Geometry itself; the texels it adds to equal the oracle's bit for bit,
    and libc rand() is consumed once per reference launch"""
    spa = 65_000
    sc = emitter_scenes.get(name)
    golden = np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))
    L = O.schedule_with_offsets(sc, spa, golden)
    assert len(L) == launches
    olm, ost = O.bake(sc, L)
    assert ost["photons"] == 100 * int(L["count"].sum())
    tex = np.full((sc.num_texels, 4), 0.5, np.float32)
    g, keep = fmgi.make_geometry(sc, tex)
    libc.srand(1)
    os.environ["FMGI_QUIET"] = "1"
    fmgi._lib.load().performGlobalIlluminationCl(C.byref(g), spa)
    assert libc.rand() == golden[launches]
    exp = O.finalize(olm, np.full_like(tex, 0.5))
    assert np.array_equal(tex.view(np.uint32), exp.view(np.uint32))
    assert (exp != 0.5).any()
    del keep


def test_histograms_per_source(torch_cuda, offsets):
    """lamps, each source's first 512 items: bake_states with one group per source, recoloured with the reference
    palette, equals bake_items and the oracle; bake_sparse of each range gives the blob of bake_states + compact"""
    torch = torch_cuda
    key = "lamps"
    sc = _scene(key)
    T = sc.num_texels
    ctx = _ctx(key, offsets)
    assert ctx.bake_sparse_supported()
    ranges = [(b, b + 512) for b in _begins(key)[:-1]]
    assert len(ranges) == 3
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        hists = [torch.zeros((1024, T), dtype=torch.int64, device="cuda") for _ in ranges]
        lm = torch.zeros((T, 4), dtype=torch.int64, device="cuda")
        direct = torch.zeros((T, 4), dtype=torch.int64, device="cuda")
    blobs = []
    for h, (lo, hi) in zip(hists, ranges):
        ctx.bake_states(lo, hi, h.data_ptr(), fmgi.KERNEL_GRID, s.cuda_stream)
        info = ctx.sparse_measure(h.data_ptr(), s.cuda_stream)
        with torch.cuda.stream(s):
            blob = torch.zeros(fmgi.sparse_bytes(T, info.rows) // 8, dtype=torch.int64, device="cuda")
        ctx.sparse_compact(h.data_ptr(), info, blob.data_ptr(), s.cuda_stream)
        s.synchronize()
        blobs.append((info, blob.cpu().numpy()))
    ref = fmgi.Palette.reference()
    ctx.recolour([h.data_ptr() for h in hists], [[ref] * len(hists)], [lm.data_ptr()], s.cuda_stream)
    for lo, hi in ranges:
        ctx.bake_items(lo, hi, direct.data_ptr(), fmgi.KERNEL_GRID, s.cuda_stream)
    s.synchronize()
    got = lm.cpu().numpy()
    assert not got[:, 3].any() and np.array_equal(got, direct.cpu().numpy())
    assert np.array_equal(got[:, :3], sum(_oracle(key, lo, hi)[0] for lo, hi in ranges))
    deposits = 0
    for (info, blob), (lo, hi) in zip(blobs, ranges):
        sinfo = ctx.bake_sparse(lo, hi, fmgi.KERNEL_GRID, s.cuda_stream)
        assert ctx.bake_sparse_stats()["dense_chunks"] == 0
        with torch.cuda.stream(s):
            out = torch.zeros(fmgi.sparse_bytes(T, sinfo.rows) // 8, dtype=torch.int64, device="cuda")
        ctx.bake_sparse_take(sinfo, out.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert sinfo == info and out.cpu().numpy().tobytes() == blob.tobytes(), (lo, hi)
        assert info.deposits == _oracle(key, lo, hi)[1]["deposits"]
        deposits += info.deposits
    assert deposits > 3 * 400_000
    ctx.close()
