"""The bake's deposit fold at the lightmap sizes where it changes (tests/lightmap_sizes.py), against
the oracle, everything by equality: the three int64 channels, a fourth word of zeros, the four counters, no stream
overflow, and the words behind the lightmap untouched.

  P = ceil(numTexels / 2048) <= 63   the bucket layouts (the rings, AccScatter, AccShared; 2048- and 4096-texel
                                     tiles) at 1, 2, 3 and 63 tiles, on lightmaps that end one texel before, on and
                                     one texel behind a tile; both photon loops, several chunks, an exhausted pool
                                     and the sparse histograms at 63 tiles, where the last tile's table slot lies
                                     beside the waves' reserve (kFree)
  64 <= P <= 128                     the slice-sorted stream with 8192-code slices, by size and not by option
  P > 128                            32768-code slices and packed runs
  numTexels = 4,194,303 / 4,194,304  the largest STREAM lightmap (2048 tiles, 15 of them hit) and the FX3 fallback

What the scenes give these tests (a deposit in every tile, in texel 0 and in texel T - 1) is checked on the CPU
(tests/test_lightmap_sizes_host.py)."""
import functools
import os

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import lightmap_sizes as LS
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

COUNTERS = ("photons", "scans", "deposits", "escapes")
GUARD = 64  # texels of all ones behind every lightmap
FILL_NAME = {0: "AccStreamT<2>", 1: "AccScatter", 2: "AccShared"}
FILL_IDS = {0: "ring", 1: "scatter", 2: "shared"}
SLICED = "AccStreamT<0>"
BUCKET_SIZES = (6, 2047, 2048, 2049, 126_977, 129_023, 129_024)
BUCKET_CASES = [(T, w) for T in BUCKET_SIZES for w in (0, 1)] + [(4096, 1), (4097, 1)]
SLICED_SIZES = (129_025, 131_072, 262_144, 262_145)


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(None)
def _schedule(kind, T):
    return O.schedule_with_offsets(LS.get(kind, T), LS.SPA, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))


@functools.lru_cache(None)
def _oracle(kind, T, ranges):
    """the oracle's lightmap of the item ranges together as int64 [T, 4] (a fourth word of zeros, as the device
    lightmap has) and its summed counters; computed once per module and never modified"""
    lm4 = np.zeros((T, 4), np.int64)
    total = dict.fromkeys(COUNTERS, 0)
    for lo, hi in ranges:
        lm, st = O.bake(LS.get(kind, T), _schedule(kind, T), lo, hi)
        lm4[:, :3] += lm
        for k in COUNTERS:
            total[k] += st[k]
    lm4.setflags(write=False)
    return lm4, total


def _ctx(kind, T, offsets, accum=None, **options):
    ctx = fmgi.Context(0)
    if accum is not None:
        ctx.set_accumulation(accum)
    ctx.set_scene(LS.get(kind, T))
    assert ctx.plan(LS.SPA, rng_offsets=offsets) == LS.TOTAL_ITEMS
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _name(ctx):
    """the last bake's instance, spaces dropped (demanglers differ in how they close nested template lists)"""
    return ctx.last_bake_kernel.replace(" ", "")


def _bake(torch, ctx, ranges, kernel=fmgi.KERNEL_GRID):
    """bakes the item ranges into one fresh lightmap; returns (int64 [T, 4], stats, the instances' names)"""
    T = ctx.scene.num_texels
    ctx.reset_stats()
    names = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf = torch.full((T + GUARD, 4), -1, dtype=torch.int64, device="cuda")
        buf[:T].zero_()
        for lo, hi in ranges:
            ctx.bake_items(lo, hi, buf.data_ptr(), kernel, s.cuda_stream)
            names.append(_name(ctx))
    s.synchronize()
    st = ctx.stats()
    print(f"{ctx.scene.name} items {ranges}: {ctx.last_bake_kernel} bucket_fallback_codes {st['bucket_fallback_codes']} "
          f"of {st['deposits']} deposits")
    assert st["stream_overflow"] == 0
    got = buf.cpu().numpy()
    assert (got[T:] == -1).all(), "the words behind the lightmap were written"
    return got[:T], st, names


def _same_counters(st, ost, items):
    assert st["photons"] == 100 * items
    for k in COUNTERS:
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["scans"] == st["deposits"] + st["escapes"]


def _check(torch, ctx, kind, T, kernel=fmgi.KERNEL_GRID, ranges=LS.RANGES, want=(), never=()):
    """every range on its own fresh lightmap against the oracle; returns the lightmaps and the last stats"""
    lms, st = [], None
    for r in ranges:
        olm, ost = _oracle(kind, T, (r,))
        lm, st, names = _bake(torch, ctx, (r,), kernel)
        for n in names:
            assert all(w in n for w in want) and not any(w in n for w in never), ctx.last_bake_kernel
        if not np.array_equal(lm, olm):
            bad = np.flatnonzero((lm != olm).any(axis=1))
            raise AssertionError(f"{ctx.scene.name} items {r}: {bad.size} texels differ, first {bad[:8]}, last {bad[-8:]}")
        _same_counters(st, ost, r[1] - r[0])
        lms.append(lm)
    return lms, st


# ---- the bucket layouts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0, 1, 2], ids=FILL_IDS.get)
@pytest.mark.parametrize("T,wide", BUCKET_CASES, ids=[f"{T}-{'wide' if w else 'narrow'}" for T, w in BUCKET_CASES])
def test_bucket_layouts(torch_cuda, offsets, T, wide, fill):
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM, bucket_fill=fill, wide_tiles=wide)
    one_tile = T <= (4096 if wide else 2048)
    for r in LS.RANGES:
        _, st = _check(torch_cuda, ctx, "even", T, ranges=(r,), want=(FILL_NAME[fill],), never=(SLICED,))
        # a lightmap of one bucket tile: a workgroup's lanes may run ahead of the tile's opener
        # (tests/test_gpu_shared_buckets.py test_one_tile_every_lane_on_one_word); printed by _bake
        if fill and not one_tile:
            assert st["bucket_fallback_codes"] == 0
    ctx.close()


@pytest.mark.parametrize("fill", [1, 2], ids=FILL_IDS.get)
@pytest.mark.parametrize("lock", [0, 1], ids=["lane", "locked"])
def test_both_photon_loops_at_63_tiles(torch_cuda, offsets, lock, fill):
    T = LS.BUCKET_MAX
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM, bucket_fill=fill, photon_lock=lock)
    _, st = _check(torch_cuda, ctx, "even", T, want=(FILL_NAME[fill], "k_bake"))
    assert ("k_bake_locked<" in _name(ctx)) == bool(lock), ctx.last_bake_kernel
    assert st["bucket_fallback_codes"] == 0
    ctx.close()


@pytest.mark.parametrize("fill", [1, 2], ids=FILL_IDS.get)
def test_chunks_at_63_tiles(torch_cuda, offsets, fill):
    """the window's 2048 items in three chunks, the lamp's 1024 in two: every chunk's blocks listed and folded
    into the same lightmap"""
    T = LS.BUCKET_MAX
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM, bucket_fill=fill, chunk_items=700)
    _check(torch_cuda, ctx, "even", T, want=(FILL_NAME[fill],))
    ctx.close()


@pytest.mark.parametrize("fill", [0, 1, 2], ids=FILL_IDS.get)
def test_pool_exhaustion_at_63_tiles(torch_cuda, offsets, fill):
    """64 pool blocks for 63 tiles (tests/test_gpu_parity.py test_bucket_pool_exhaustion_falls_back_exactly on 46):
    the rest of the codes through bucket_atomic, the lightmap the oracle's"""
    T = LS.BUCKET_MAX
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM, bucket_fill=fill, pool_limit=64)
    _, st = _check(torch_cuda, ctx, "even", T, want=(FILL_NAME[fill],))
    if fill == 2:  # (only AccShared counts its fallback codes)
        assert st["bucket_fallback_codes"] > 0
    ctx.close()


# ---- AUTO ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", list(LS.EVEN_SIZES))
def test_auto_on_every_size(torch_cuda, offsets, T):
    """no accumulation, option or kernel chosen: STREAM, a bucket layout up to 63 tiles and the sliced stream above"""
    ctx = _ctx("even", T, offsets)
    assert ctx.accumulation == fmgi.ACCUM_STREAM
    _check(torch_cuda, ctx, "even", T, kernel=fmgi.KERNEL_AUTO)
    n = _name(ctx)
    assert (SLICED in n) == (T > LS.BUCKET_MAX), ctx.last_bake_kernel
    assert (T > LS.BUCKET_MAX) or any(v in n for v in FILL_NAME.values()), ctx.last_bake_kernel
    ctx.close()


@pytest.mark.parametrize("T", [LS.BUCKET_MAX, LS.BUCKET_MAX + 1])
def test_fx3_and_state_equal_stream(torch_cuda, offsets, T):
    lms = {}
    stream = SLICED if T > LS.BUCKET_MAX else "k_bake"
    for accum, name in ((fmgi.ACCUM_STREAM, stream), (fmgi.ACCUM_FX3, "AccFx3"), (fmgi.ACCUM_STATE, "AccState")):
        ctx = _ctx("even", T, offsets, accum)
        assert ctx.accumulation == accum
        lms[accum], _ = _check(torch_cuda, ctx, "even", T, want=(name,))
        ctx.close()
    for accum in (fmgi.ACCUM_FX3, fmgi.ACCUM_STATE):
        for a, b in zip(lms[accum], lms[fmgi.ACCUM_STREAM]):
            assert np.array_equal(a, b)


# ---- the slice-sorted stream by size -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", SLICED_SIZES)
def test_sliced_stream_by_size(torch_cuda, offsets, T):
    """64 and 128 tiles: 8192-code slices, one run at a time (k_slice_sort<8192, 256>, k_tile_runs); 129: 32768-code
    slices and packed runs (k_slice_sort<32768, 1024>, k_tile_runs_pre); nothing forced"""
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM)
    _check(torch_cuda, ctx, "even", T, want=(SLICED,), never=tuple(FILL_NAME.values()))
    ctx.close()


def test_sliced_stream_forced_at_63_tiles(torch_cuda, offsets):
    T = LS.BUCKET_MAX
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM, stream_layout=0)
    sliced, _ = _check(torch_cuda, ctx, "even", T, want=(SLICED,), never=tuple(FILL_NAME.values()))
    ctx.set_option("stream_layout", -1)
    buckets, _ = _check(torch_cuda, ctx, "even", T, never=(SLICED,))
    for a, b in zip(sliced, buckets):
        assert np.array_equal(a, b)
    ctx.close()


# ---- the ends of STREAM --------------------------------------------------------------------------------------------------------

def _gapped(torch, ctx, T, want):
    """both ranges into one lightmap, one comparison of its 134 MB"""
    olm, ost = _oracle("gapped", T, LS.RANGES)
    lm, st, names = _bake(torch, ctx, LS.RANGES)
    for n in names:
        assert want in n, n
    assert np.array_equal(lm, olm)
    _same_counters(st, ost, sum(hi - lo for lo, hi in LS.RANGES))


def test_largest_stream_lightmap(torch_cuda, offsets):
    """2048 tiles (k_slice_sort's cnt[] and loc[] full), 15 of them hit, every other tile's run empty"""
    T = LS.STREAM_END - 1
    ctx = _ctx("gapped", T, offsets, fmgi.ACCUM_STREAM)
    assert ctx.accumulation == fmgi.ACCUM_STREAM
    _gapped(torch_cuda, ctx, T, SLICED)
    ctx.close()


@pytest.mark.parametrize("accum", [None, fmgi.ACCUM_STREAM], ids=["auto", "stream"])
def test_fx3_from_4194304_texels(torch_cuda, offsets, accum):
    T = LS.STREAM_END
    ctx = _ctx("gapped", T, offsets, accum)
    assert ctx.accumulation == fmgi.ACCUM_FX3
    _gapped(torch_cuda, ctx, T, "AccFx3")
    ctx.close()


# ---- sparse histograms at the largest supported lightmap -----------------------------------------------------------------------

def _blob(torch, ctx, s, info, fill):
    """a device buffer for a blob of info.rows rows with GUARD words of all ones behind it, filled by fill(ptr)"""
    words = fmgi.sparse_bytes(ctx.scene.num_texels, info.rows) // 8
    with torch.cuda.stream(s):
        buf = torch.full((words + GUARD,), -1, dtype=torch.int64, device="cuda")
    fill(buf.data_ptr())
    s.synchronize()
    got = buf.cpu().numpy()
    assert (got[words:] == -1).all(), "the guard words behind the blob were written"
    return buf, got[:words]


@pytest.mark.parametrize("r", LS.RANGES, ids=["window", "lamp"])
@pytest.mark.parametrize("T", [126_977, LS.BUCKET_MAX])
def test_sparse_histograms_at_63_tiles(torch_cuda, offsets, T, r):
    """fmgi_bake_sparse against fmgi_bake_states + measure + compact on the same context (the dense histogram, 1 GB,
    stays on the device), and recoloured with the reference palette against the oracle"""
    torch = torch_cuda
    ctx = _ctx("even", T, offsets, fmgi.ACCUM_STREAM)
    assert ctx.bake_sparse_supported()
    s = torch.cuda.Stream()
    ctx.reset_stats()
    info = ctx.bake_sparse(r[0], r[1], fmgi.KERNEL_GRID, s.cuda_stream)
    st = ctx.bake_sparse_stats()
    print(f"{ctx.scene.name} {r}: {info} {st} {ctx.last_bake_kernel}")
    assert st["dense_chunks"] == 0 and st["codes"] == info.deposits
    olm, ost = _oracle("even", T, (r,))
    assert info.deposits == ost["deposits"] and info.num_texels == T
    _same_counters(ctx.stats(), ost, r[1] - r[0])
    blob, got = _blob(torch, ctx, s, info, lambda p: ctx.bake_sparse_take(info, p, s.cuda_stream))
    assert fmgi.sparse_check(got.view(np.uint64), T) == info
    # the parent route
    with torch.cuda.stream(s):
        dense = torch.zeros((1024, T), dtype=torch.int64, device="cuda")
    ctx.bake_states(r[0], r[1], dense.data_ptr(), fmgi.KERNEL_GRID, s.cuda_stream)
    pinfo = ctx.sparse_measure(dense.data_ptr(), s.cuda_stream)
    assert pinfo == info
    _, pgot = _blob(torch, ctx, s, pinfo, lambda p: ctx.sparse_compact(dense.data_ptr(), pinfo, p, s.cuda_stream))
    del dense
    assert got.tobytes() == pgot.tobytes()
    # recoloured
    with torch.cuda.stream(s):
        lm = torch.zeros((T, 4), dtype=torch.int64, device="cuda")
    ctx.recolour_sparse([blob.data_ptr()], [info], [[fmgi.Palette.reference()]], [lm.data_ptr()], s.cuda_stream)
    s.synchronize()
    assert np.array_equal(lm.cpu().numpy(), olm)
    assert ctx.accumulation == fmgi.ACCUM_STREAM
    ctx.close()


def test_sparse_is_refused_at_64_tiles(torch_cuda, offsets):
    ctx = _ctx("even", LS.BUCKET_MAX + 1, offsets, fmgi.ACCUM_STREAM)
    assert not ctx.bake_sparse_supported()
    with pytest.raises(fmgi.FmgiError, match=r"\(-4\).*63 tiles"):
        ctx.bake_sparse(0, 10, fmgi.KERNEL_GRID)
    ctx.close()
