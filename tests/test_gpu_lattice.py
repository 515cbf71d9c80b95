"""The lattice instances of the closed boxes (ScanGridLatticeT<ScanGridT<true, true, ...>>, lattice=1): on the nearest plane a scan takes the
rect of the face lattice under the hit point instead of reading the grid cell and testing its records. int64
lightmaps, the four counters and per-photon traces against the oracle, bit for bit, on a 1 x 1 lattice per face
(box8: edges and clamping dominate), on the main case (box200) and on the compact instance (box2000), with both
photon loops; lattice=0 against lattice=1 over 1e6 photons; scenes without a lattice. Every test sets lattice=1
itself, so none depends on what AUTO chooses.

(Of the bit-for-bit five -- lightmap, photons, scans, deposits, escapes -- the last four are counters;
exact_rescans, rescans_tie and rescans_invalid may fall with the lattice, which sees one candidate where a cell's
quantized bounds can see two, and `tests` must fall.)"""
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
LAUNCH_ITEMS = 25600  # items per reference launch (256 x 100): [25536, 25664) straddles the first boundary
RANGES = ((0, 128), (LAUNCH_ITEMS - 64, LAUNCH_ITEMS + 64))


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(maxsize=None)
def _scene(name):
    from fmgi import scene

    if name in ("box8", "box200", "box2000"):
        return scene.box_scene(int(name[3:]), tile_size=4.0)
    if name == "example":
        return scene.load_geometry(os.path.join(GOLDEN, "example_geometry.bin"), "example")
    if name == "apartment30":
        return scene.load_geometry(os.path.join(GOLDEN, "apartment30_geometry.bin"), "a30")
    if name == "tilted":
        return scene.tilted_scene()
    assert name == "shifted"
    from test_lattice import _shifted_box200

    return _shifted_box200(scene.box_scene(200, tile_size=4.0))


_ORACLE = {}


def _oracle(name, spa, offsets, lo, hi):
    """the oracle's (lightmap, stats) of items [lo, hi), computed once per module and never modified (O.bake_port:
    the oracle's restatement, bit-identical by tests/test_oracle.py and several times faster)"""
    k = (name, spa, lo, hi)
    if k not in _ORACLE:
        sc = _scene(name)
        lm, st = O.bake_port(sc, O.schedule_with_offsets(sc, spa, offsets), lo, hi)
        lm.setflags(write=False)
        _ORACLE[k] = (lm, st)
    return _ORACLE[k]


def _ctx(name, spa, offsets, lock, accum=fmgi.ACCUM_STREAM, lattice=1):
    ctx = fmgi.Context(0)
    ctx.set_accumulation(accum)
    ctx.set_scene(_scene(name))
    ctx.plan(spa, rng_offsets=offsets)
    ctx.set_option("photon_lock", lock)
    ctx.set_option("lattice", lattice)
    if name == "box8" and accum == fmgi.ACCUM_STREAM:
        # box8's lightmap is one fold tile: with the per-workgroup blocks (AccShared, AUTO's choice) all 768 lanes
        # of a workgroup add to one tile word, and a wave that gets two blocks ahead of the tile's opener adds its
        # codes by the exact atomic fallback (seen once: 64 codes in 8e6 deposits, lattice = 1, per-lane loop),
        # which bucket_fallback_codes counts. The per-wave blocks take that path only when the pool runs out, so
        # the tests can assert 0.
        ctx.set_option("bucket_fill", 1)
    return ctx


def _bake(torch, ctx, lo, hi, kernel=fmgi.KERNEL_GRID):
    """bakes items [lo, hi) on a fresh lightmap with the grid scan (AUTO's choice for box200 and box2000; box8, of
    two filter pairs per axis, would take ScanFast)"""
    ctx.reset_stats()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lm = torch.zeros((ctx.scene.num_texels, 4), dtype=torch.int64, device="cuda")
        ctx.bake_items(lo, hi, lm.data_ptr(), kernel, s.cuda_stream)
    s.synchronize()
    st = ctx.stats()
    print(f"{ctx.scene.name} items [{lo}, {hi}): {ctx.last_bake_kernel} tests/scans {st['tests'] / max(st['scans'], 1):.4f}")
    assert st["stream_overflow"] == 0 and st["bucket_fallback_codes"] == 0
    got = lm.cpu().numpy()
    assert not got[:, 3].any()
    return got[:, :3], st


def _same_counters(st, ost, items):
    assert st["photons"] == 100 * items
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])


def _runs(ctx, lock, compact):
    """whether the last bake ran the lattice instance of the staged / compact closed box with this photon loop
    (spaces dropped: demanglers differ in how they close nested template lists)"""
    want = (f"{'k_bake_locked' if lock else 'k_bake'}<(anonymous namespace)::ScanGridLatticeT<(anonymous namespace)::"
            f"ScanGridT<true, true, {'true' if compact else 'false'}>>,")
    return want.replace(" ", "") in ctx.last_bake_kernel.replace(" ", "")


@pytest.mark.parametrize("lock", [0, 1])
@pytest.mark.parametrize("name", ["box8", "box200", "box2000"])
def test_lightmaps_and_counters_equal_the_oracle(torch_cuda, offsets, name, lock):
    ctx = _ctx(name, BOX_SPA, offsets, lock)
    assert len(ctx.lattice_tables()["lattice"]) == 6
    for lo, hi in RANGES:
        olm, ost = _oracle(name, BOX_SPA, offsets, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi)
        assert _runs(ctx, lock, name == "box2000"), ctx.last_bake_kernel
        assert np.array_equal(lm, olm)
        _same_counters(st, ost, hi - lo)
    ctx.close()


@pytest.mark.parametrize("lock", [0, 1])
@pytest.mark.parametrize("accum", [fmgi.ACCUM_FX3, fmgi.ACCUM_STATE])
def test_box200_fx3_and_state(torch_cuda, offsets, accum, lock):
    """(the per-lane loop stages no cells for FX3 and STATE, so its instance there has no lattice to take)"""
    ctx = _ctx("box200", BOX_SPA, offsets, lock, accum)
    for lo, hi in RANGES:
        olm, ost = _oracle("box200", BOX_SPA, offsets, lo, hi)
        lm, st = _bake(torch_cuda, ctx, lo, hi)
        if lock:
            assert _runs(ctx, 1, False), ctx.last_bake_kernel
        assert np.array_equal(lm, olm)
        _same_counters(st, ost, hi - lo)
    ctx.close()


@pytest.mark.parametrize("lock", [0, 1])
def test_box200_traces(torch_cuda, offsets, lock):
    """events, event counts and final RNG states of 64 items (the TRACE instance, as tests/test_gpu_parity.py)"""
    sc = _scene("box200")
    L = O.schedule_with_offsets(sc, BOX_SPA, offsets)
    ctx = _ctx("box200", BOX_SPA, offsets, lock)
    ev, cnt, rngf = ctx.trace_items(0, 64, fmgi.KERNEL_GRID)
    assert _runs(ctx, lock, False), ctx.last_bake_kernel
    assert ctx.stats()["stream_overflow"] == 0
    for w in range(64):
        li = int(np.searchsorted(L["item_begin"], w, side="right") - 1)
        state = (w - int(L[li]["item_begin"]) + int(L[li]["rng_offset"])) & 0xFFFFFFFF
        oev, ofin = O.trace_item(sc, int(L[li]["source"]), int(L[li]["is_window"]), state)
        assert cnt[w] == len(oev), f"item {w}: {cnt[w]} vs {len(oev)} events"
        g = ev[w, : cnt[w]].view(np.uint32)
        assert np.array_equal(g, oev.view(np.uint32).reshape(g.shape)), f"item {w}"
        assert rngf[w] == ofin, f"item {w}: final RNG"
    ctx.close()


@pytest.mark.parametrize("lock", [0, 1])
@pytest.mark.parametrize("name", ["box8", "box200", "box2000"])
def test_lattice_off_and_on_agree_over_a_million_photons(torch_cuda, offsets, name, lock):
    """10,000 items: 8e6 scans, several thousand of them in the band along the rects' edges. `tests` must fall
    where a cell holds more than one record (box200, box2000); every cell of box8's 1 x 1 lattices holds its
    face's one record, so there the cell path counts one test per lookup as the lattice does, and `tests` cannot
    fall: it must not rise."""
    n = 10_000
    res = {}
    for lattice in (0, 1):
        ctx = _ctx(name, BOX_SPA, offsets, lock, lattice=lattice)
        res[lattice] = _bake(torch_cuda, ctx, 0, n)
        assert ("ScanGridLatticeT" in ctx.last_bake_kernel) == bool(lattice), ctx.last_bake_kernel
        ctx.close()
    (lm0, st0), (lm1, st1) = res[0], res[1]
    assert np.array_equal(lm0, lm1)
    for k in COUNTERS:
        assert st0[k] == st1[k], (k, st0[k], st1[k])
    print(f"{name} lock {lock}: tests {st0['tests']} -> {st1['tests']} over {st1['scans']} scans; ties "
          f"{st0['rescans_tie']} -> {st1['rescans_tie']}, invalid {st0['rescans_invalid']} -> {st1['rescans_invalid']}")
    if name == "box8":
        assert st1["tests"] <= st0["tests"]
    else:
        assert st1["tests"] < st0["tests"]
    assert st1["rescans_tie"] <= st0["rescans_tie"] and st1["rescans_invalid"] <= st0["rescans_invalid"]
    if name == "box200":
        assert st1["tests"] <= 1.01 * st1["scans"], (st1["tests"], st1["scans"])


@pytest.mark.parametrize("name", ["example", "apartment30", "tilted", "shifted"])
def test_scenes_without_a_lattice_bake_as_before(torch_cuda, offsets, name):
    """lattice = 1 on a scene without a verified lattice runs the ordinary instance: the same kernel, lightmap and
    statistics as lattice = 0"""
    sc = _scene(name)
    spa = 65_000 if name in ("example", "apartment30") else BOX_SPA
    res = {}
    for lattice in (0, 1):
        ctx = _ctx(name, spa, offsets, -1, lattice=lattice)
        assert len(ctx.lattice_tables()["lattice"]) == 0
        hi = min(ctx.total_items, 512)
        lm, st = _bake(torch_cuda, ctx, 0, hi, fmgi.KERNEL_AUTO)
        res[lattice] = (lm, st, ctx.last_bake_kernel)
        ctx.close()
    assert res[0][2] == res[1][2] and "Lattice" not in res[1][2], (res[0][2], res[1][2])
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    assert sc.num_texels == res[1][0].shape[0]


def test_option_validation(torch_cuda, offsets):
    """lattice is -1, 0 or 1; a refused value leaves the previous one"""
    ctx = _ctx("box200", BOX_SPA, offsets, 1)
    for v in (-1, 0, 1):
        ctx.set_option("lattice", v)
    for bad in (2, -2):
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):  # FMGI_ERR_ARG
            ctx.set_option("lattice", bad)
    lm, _ = _bake(torch_cuda, ctx, 0, 128)  # (the refused values left lattice = 1)
    assert "ScanGridLatticeT" in ctx.last_bake_kernel, ctx.last_bake_kernel
    assert np.array_equal(lm, _oracle("box200", BOX_SPA, offsets, 0, 128)[0])
    ctx.set_option("lattice", 0)
    for bad in (2, -2):
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
            ctx.set_option("lattice", bad)
    lm, _ = _bake(torch_cuda, ctx, 0, 128)
    assert "ScanGridLatticeT" not in ctx.last_bake_kernel and "<(anonymous namespace)::ScanGridT<true, true, false>," in ctx.last_bake_kernel
    assert np.array_equal(lm, _oracle("box200", BOX_SPA, offsets, 0, 128)[0])
    ctx.close()
