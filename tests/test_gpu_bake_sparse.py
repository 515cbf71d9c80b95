"""GPU tests of the sparse photon histograms built from deposit codes. Every comparison is equality:
fmgi_sparse_from_codes against the numpy restatement on synthetic codes; fmgi_sparse_add against the restated sum;
fmgi_bake_sparse on the lit box against the event-derived histogram, against fmgi_bake_states + fmgi_sparse_compact
and (recoloured) against fmgi_bake_items and the oracle; several chunks; every bucket filler of the bake; the dense
route of a chunk whose bucket fallback fired; an unsupported scene; and tools/relight.py --sparse-from-codes."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bake_sparse_restate as H
import fm_oracle as O
import fmgi
import recolour_events as R
import sparse_restate as S
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
BIG = (1 << 54) - 1
GUARD = 64  # words of all ones behind every output buffer
BOX_SPA = 172_413_793


class Dev:
    """a context on a scene, a stream, and the calls of the tests"""

    def __init__(self, torch, sc):
        self.torch, self.sc, self.T = torch, sc, sc.num_texels
        self.ctx = fmgi.Context(0)
        self.ctx.set_scene(sc)
        self.s = torch.cuda.Stream(device="cuda:0")

    def close(self):
        self.ctx.close()

    def zeros(self, *shape):
        with self.torch.cuda.stream(self.s):
            return self.torch.zeros(shape, dtype=self.torch.int64, device="cuda:0")

    def upload(self, a, dtype=np.int64):
        with self.torch.cuda.stream(self.s):
            t = self.torch.from_numpy(np.ascontiguousarray(a).view(dtype).copy()).to("cuda:0")
        self.s.synchronize()
        return t

    def guarded(self, info):
        """a buffer for a blob of info.rows rows with GUARD words of all ones behind it"""
        words = fmgi.sparse_bytes(self.T, info.rows) // 8
        with self.torch.cuda.stream(self.s):
            return self.torch.full((words + GUARD,), -1, dtype=self.torch.int64, device="cuda:0"), words

    def words(self, buf, words):
        """the blob's words (uint64 numpy) of a guarded buffer whose guard must be untouched"""
        self.s.synchronize()
        got = buf.cpu().numpy().view(np.uint64)
        assert (got[words:] == np.uint64(M64)).all(), "the guard words behind the blob were written"
        return got[:words]

    def take(self, info):
        """(device buffer, the held blob's words); a second take finds nothing held"""
        buf, words = self.guarded(info)
        self.ctx.bake_sparse_take(info, buf.data_ptr(), self.s.cuda_stream)
        got = self.words(buf, words)
        with pytest.raises(fmgi.FmgiError, match=r"\(-4\).*held"):
            self.ctx.bake_sparse_take(info, buf.data_ptr(), self.s.cuda_stream)
        return buf, got

    def from_codes(self, codes):
        d = self.upload(np.asarray(codes, np.uint32), np.int32) if len(codes) else self.zeros(1)
        info, skipped = self.ctx.sparse_from_codes(d.data_ptr(), len(codes), self.s.cuda_stream)
        buf, got = self.take(info)
        return info, skipped, buf, got

    def bake_sparse(self, b, e, kernel=fmgi.KERNEL_AUTO):
        info = self.ctx.bake_sparse(b, e, kernel, self.s.cuda_stream)
        name, st = self.ctx.last_bake_kernel, self.ctx.bake_sparse_stats()
        buf, got = self.take(info)
        return info, buf, got, st, name

    def states_compact(self, ranges, kernel=fmgi.KERNEL_AUTO):
        """the parent route: fmgi_bake_states into a zeroed dense histogram, measure, compact"""
        h = self.zeros(1024, self.T)
        for b, e in ranges:
            self.ctx.bake_states(b, e, h.data_ptr(), kernel, self.s.cuda_stream)
        info = self.ctx.sparse_measure(h.data_ptr(), self.s.cuda_stream)
        buf, words = self.guarded(info)
        self.ctx.sparse_compact(h.data_ptr(), info, buf.data_ptr(), self.s.cuda_stream)
        return info, buf, self.words(buf, words)

    def compact(self, dense):
        h = self.upload(dense)
        info = self.ctx.sparse_measure(h.data_ptr(), self.s.cuda_stream)
        buf, words = self.guarded(info)
        self.ctx.sparse_compact(h.data_ptr(), info, buf.data_ptr(), self.s.cuda_stream)
        return info, buf, self.words(buf, words)

    def add(self, a, ai, b, bi):
        si = self.ctx.sparse_add_measure(a.data_ptr(), ai, b.data_ptr(), bi, self.s.cuda_stream)
        buf, words = self.guarded(si)
        self.ctx.sparse_add(a.data_ptr(), ai, b.data_ptr(), bi, si, buf.data_ptr(), self.s.cuda_stream)
        return si, buf, self.words(buf, words)


def _synthetic_scene(T):
    from fmgi import scene

    sc = scene.box_scene(200, tile_size=4.0, with_light=True)
    return scene.Scene(f"synthetic{T}", sc.walls[:0], sc.windows, sc.lights, T)


@pytest.fixture(scope="module")
def devs(torch_cuda):
    """one context per synthetic texel count, made on first use"""
    made = {}

    def get(T):
        if T not in made:
            made[T] = Dev(torch_cuda, _synthetic_scene(T))
        return made[T]

    yield get
    for d in made.values():
        d.close()


# ---- 1. from codes, synthetic ------------------------------------------------------------------------------------------

EDGE_TEXELS = (0, 31, 32, 63, 64, 2047, 2048, 4095, 4096)


def _codes(T, n, seed=0):
    """n codes: random cells, a third of the texels either side of the half-block, block and tile edges, half of
    the states 0 / 512 / 1023; then an eighth pads and an eighth texels T and T + 5"""
    rng = np.random.default_rng(1000 * T + n + seed)
    tex = rng.integers(0, T, n)
    edges = np.array([t for t in EDGE_TEXELS + (T - 1,) if t < T])
    at = rng.random(n) < 1 / 3
    tex[at] = rng.choice(edges, int(at.sum()))
    st = rng.integers(0, 1024, n)
    at = rng.random(n) < 0.5
    st[at] = rng.choice(np.array([0, 512, 1023]), int(at.sum()))
    codes = H.code(tex, st)
    if n >= 8:
        codes[rng.choice(n, n // 8, replace=False)] = np.uint32(H.PAD)
        at = rng.choice(n, n // 8, replace=False)
        codes[at] = H.code(np.where(rng.random(len(at)) < 0.5, T, T + 5), st[at])
    return codes


def _check_from_codes(dev, codes):
    want_blob, want_info, want_skipped = H.from_codes(codes, dev.T)
    info, skipped, _, got = dev.from_codes(codes)
    print(info, "skipped", skipped, dev.ctx.bake_sparse_stats())
    assert info.as_dict() == want_info and skipped == want_skipped
    assert got.tobytes() == want_blob.tobytes()
    assert fmgi.sparse_check(got, dev.T) == info
    st = dev.ctx.bake_sparse_stats()
    assert st["chunks"] == 1 and st["dense_chunks"] == 0 and st["codes"] == info.deposits
    return info, st


@pytest.mark.parametrize("n", [0, 1, 1023, 1025, 300_000])
@pytest.mark.parametrize("wide", [0, 1])
@pytest.mark.parametrize("T", [1, 63, 65, 2047, 2049, 4097])
def test_from_codes_equals_the_restatement(devs, T, wide, n):
    dev = devs(T)
    dev.ctx.set_option("wide_tiles", wide)
    dev.ctx.set_option("hist_batch", 0)
    info, _ = _check_from_codes(dev, _codes(T, n))
    if n == 0:
        assert info.rows == 0 and info.deposits == 0
    if n == 300_000 and T == 1:
        assert info.rows == 1024  # every state of the one texel


@pytest.mark.parametrize("T,batch", [(65, 1000), (2049, 5000), (4097, 1), (4097, 40_000)])
def test_from_codes_in_several_batches(devs, T, batch):
    """FMGI_OPT_HIST_BATCH cuts the blocks into batches of at most `batch` codes (one block at least): the pieces
    joined behind the scanned offsets are the same blob"""
    dev = devs(T)
    dev.ctx.set_option("wide_tiles", -1)
    dev.ctx.set_option("hist_batch", batch)
    try:
        _check_from_codes(dev, _codes(T, 300_000, seed=1))
    finally:
        dev.ctx.set_option("hist_batch", 0)


def test_from_codes_a_million_copies_of_one_code(devs):
    dev = devs(65)
    codes = np.full(1_000_000, H.code(64, 1023), np.uint32)
    info, _ = _check_from_codes(dev, codes)
    assert (info.rows, info.cells, info.deposits) == (1, 1, 1_000_000)


def test_from_codes_uniform_cells_fill_every_row(devs):
    dev = devs(65)
    rng = np.random.default_rng(5)
    codes = H.code(rng.integers(0, 65, 300_000), rng.integers(0, 1024, 300_000))
    codes[0] = H.code(64, 1023)
    info, _ = _check_from_codes(dev, codes)
    assert info.rows > 2 * 1000 and info.cells > 0.95 * 65 * 1024


def test_from_codes_edge_pairs_and_states(devs):
    """one code per (edge texel, state 0 / 512 / 1023), twice for the upper texel of every pair"""
    dev = devs(4097)
    tex = np.array([31, 32, 32, 63, 64, 64, 2047, 2048, 2048, 4095, 4096, 4096])
    codes = np.concatenate([H.code(tex, np.full(len(tex), s)) for s in (0, 512, 1023)])
    codes = np.concatenate([codes, np.array([H.PAD] * 3, np.uint32), H.code([4097, 4102], [0, 1023])])
    info, _ = _check_from_codes(dev, codes)
    assert info.cells == 3 * 8 and info.deposits == 36


# ---- 2. the sum ------------------------------------------------------------------------------------------------------------

def _dense(T, seed):
    rng = np.random.default_rng(100 * T + seed)
    d = (rng.integers(1, 200, (1024, T)).astype(np.uint64) * (rng.random((1024, T)) < 0.02)).astype(np.uint64)
    d[0, 0], d[1023, T - 1], d[512, T // 2] = 1 + seed, (1 << 32) + 5, BIG >> 1
    return d


@pytest.mark.parametrize("T", [1, 64, 257])
def test_sum_equals_the_restated_sum(devs, T):
    dev = devs(T)
    da, db = _dense(T, 0), _dense(T, 1)
    if T == 257:
        db[:, 64:128] = 0   # a block only a has, and one neither has
        da[:, 192:256] = 0
        db[:, 192:256] = 0
    ai, a, aw = dev.compact(da)
    bi, b, bw = dev.compact(db)
    for (xi, x, xw), (yi, y, yw) in (((ai, a, aw), (bi, b, bw)), ((ai, a, aw), (ai, a, aw))):
        want_blob, want_info = H.add(xw, yw, T)
        si, _, got = dev.add(x, xi, y, yi)
        assert si.as_dict() == want_info and got.tobytes() == want_blob.tobytes()
        assert fmgi.sparse_check(got, T) == si
    empty_i, empty, _ = dev.compact(np.zeros((1024, T), np.uint64))
    si, _, got = dev.add(a, ai, empty, empty_i)
    assert si == ai and got.tobytes() == aw.tobytes()


def test_sum_of_2_to_the_54_is_refused(devs):
    T = 65
    dev = devs(T)
    da = _dense(T, 0)
    da[700, 64] = BIG
    db = np.zeros((1024, T), np.uint64)
    db[700, 64] = 1
    ai, a, _ = dev.compact(da)
    bi, b, _ = dev.compact(db)
    out = fmgi.SparseInfo()
    rc = dev.ctx.lib.fmgi_sparse_add_measure(dev.ctx.h, C.c_void_p(a.data_ptr()), C.byref(ai), C.c_void_p(b.data_ptr()),
                                             C.byref(bi), C.byref(out), C.c_void_p(dev.s.cuda_stream))
    assert rc == -3 and "2^54" in fmgi._lib.last_error()
    assert out.too_large == 1 and out.cells == ai.cells and out.num_texels == T
    with pytest.raises(fmgi.FmgiError, match=r"\(-3\).*too_large"):  # and such an info is refused before any launch
        dev.ctx.sparse_add(a.data_ptr(), ai, b.data_ptr(), bi, out, a.data_ptr(), dev.s.cuda_stream)


def test_sum_with_fewer_rows_stays_inside(devs):
    """a sum written with an info of fewer rows than it has: every offset is clamped, the words behind the smaller
    blob stay as they were, and the rows that fit hold what the whole sum holds there"""
    T = 257
    dev = devs(T)
    ai, a, aw = dev.compact(_dense(T, 0))
    bi, b, bw = dev.compact(_dense(T, 1))
    want_blob, _ = H.add(aw, bw, T)
    si = dev.ctx.sparse_add_measure(a.data_ptr(), ai, b.data_ptr(), bi, dev.s.cuda_stream)
    cut = fmgi.SparseInfo.from_buffer_copy(si)
    cut.rows = si.rows // 2
    buf, words = dev.guarded(si)  # room for the whole sum; the cut blob's words are fewer
    cut_words = fmgi.sparse_bytes(T, cut.rows) // 8
    dev.ctx.sparse_add(a.data_ptr(), ai, b.data_ptr(), bi, cut, buf.data_ptr(), dev.s.cuda_stream)
    dev.s.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[cut_words:] == np.uint64(M64)).all()
    B = (T + 63) // 64
    assert [int(v) for v in got[: B + 1]] == [min(int(v), cut.rows) for v in want_blob[: B + 1]]
    rows0 = min(int(want_blob[1]), cut.rows)
    assert np.array_equal(got[B + 1: B + 1 + 64 * rows0], want_blob[B + 1: B + 1 + 64 * rows0])


# ---- 3. the lit box --------------------------------------------------------------------------------------------------------

class Box(Dev):
    def __init__(self, torch):
        sc, self.L, self.offsets = R.lit_box()
        super().__init__(torch, sc)
        assert self.ctx.plan(R.SPA, rng_offsets=self.offsets) == 512
        self._parent = {}

    def parent(self, ranges, wide=-1):
        key = (ranges, wide)
        if key not in self._parent:
            self.ctx.set_option("wide_tiles", wide)
            self._parent[key] = self.states_compact(ranges)
            self.ctx.set_option("wide_tiles", -1)
        return self._parent[key]

    def bake(self, b, e):
        lm = self.zeros(self.T, 4)
        self.ctx.bake_items(b, e, lm.data_ptr(), fmgi.KERNEL_AUTO, self.s.cuda_stream)
        self.s.synchronize()
        return lm.cpu().numpy()


@pytest.fixture(scope="module")
def box(torch_cuda):
    b = Box(torch_cuda)
    yield b
    b.close()


WINDOW, LAMP, WHOLE = ((0, 256),), ((256, 512),), ((0, 512),)


@pytest.mark.parametrize("wide", [0, 1])
def test_lit_box_equals_the_events_and_the_parent_route(box, wide):
    mode = box.ctx.accumulation
    box.ctx.set_option("wide_tiles", wide)
    try:
        # RANGES: two calls and their sum
        (b0, e0), (b1, e1) = R.RANGES
        i0, x0, _, st0, _ = box.bake_sparse(b0, e0)
        i1, x1, _, st1, _ = box.bake_sparse(b1, e1)
        info, _, got = box.add(x0, i0, x1, i1)
        want_blob, want_info = S.pack(R.dense_histogram(R.RANGES))
        assert info.as_dict() == want_info and got.tobytes() == want_blob.tobytes()
        assert (info.cells, info.rows, got.nbytes, info.deposits) == (46_916, 1_230, 630_040, 102_400)
        assert fmgi.sparse_check(got, box.T) == info
        assert st0["dense_chunks"] == 0 and st1["dense_chunks"] == 0
        assert st0["codes"] + st1["codes"] == info.deposits
        pi, _, pw = box.parent(R.RANGES, wide)
        assert pi == info and pw.tobytes() == got.tobytes()
        # (0, 512) in one call
        box.ctx.reset_stats()
        winfo, wblob, wgot, wst, _ = box.bake_sparse(0, 512)
        want_blob, want_info = S.pack(R.dense_histogram(WHOLE))
        assert winfo.as_dict() == want_info and wgot.tobytes() == want_blob.tobytes()
        assert (winfo.cells, winfo.rows, wgot.nbytes, winfo.deposits) == (92_513, 2_230, 1_142_040, 409_600)
        assert wst["dense_chunks"] == 0 and wst["chunks"] == 1 and wst["merges"] == 0
        assert wst["codes"] == winfo.deposits == box.ctx.stats()["deposits"]
        assert wst["scratch_bytes"] < fmgi.states_bytes(box.T)
        pi, _, pw = box.parent(WHOLE, wide)
        assert pi == winfo and pw.tobytes() == wgot.tobytes()
        # recoloured with the reference palette: fmgi_bake_items' lightmap, which is the oracle's
        ref = fmgi.Palette.reference()
        lm = box.zeros(1, box.T, 4)
        box.ctx.recolour_sparse([wblob.data_ptr()], [winfo], [[ref]], [lm[0].data_ptr()], box.s.cuda_stream)
        box.s.synchronize()
        lm = lm.cpu().numpy()[0]
        assert not lm[:, 3].any() and np.array_equal(lm, box.bake(0, 512))
        assert np.array_equal(lm[:, :3], O.bake(box.sc, box.L, 0, 512)[0])
    finally:
        box.ctx.set_option("wide_tiles", -1)
    assert box.ctx.accumulation == mode


def test_lit_box_empty_range_and_small_launches(box):
    info, _, got, st, _ = box.bake_sparse(0, 0)
    assert info.rows == 0 and info.cells == 0 and info.deposits == 0 and info.num_texels == box.T
    assert len(got) == (box.T + 63) // 64 + 1 and not got.any()
    info, _, got, st, _ = box.bake_sparse(300, 300)
    assert info.rows == 0 and not got.any()
    for items in (5, 70):  # fewer items than a wave / a workgroup has lanes
        info, _, got, st, _ = box.bake_sparse(0, items)
        pi, _, pw = box.parent(((0, items),))
        assert info == pi and got.tobytes() == pw.tobytes() and st["dense_chunks"] == 0


def test_lit_box_sums_of_groups_and_of_item_ranges(box):
    """window + lamp = whole, and items (0, 128) + (128, 256) = (0, 256): blobs of the parent route, summed"""
    (wi, w, _), (li, l, _), (ai, _, aw) = box.parent(WINDOW), box.parent(LAMP), box.parent(WHOLE)
    si, _, got = box.add(w, wi, l, li)
    assert si == ai and got.tobytes() == aw.tobytes()
    (xi, x, _), (yi, y, _) = box.parent(((0, 128),)), box.parent(((128, 256),))
    si, _, got = box.add(x, xi, y, yi)
    assert si == wi and got.tobytes() == box.parent(WINDOW)[2].tobytes()


# ---- 4. chunks -------------------------------------------------------------------------------------------------------------

def test_chunks_are_joined(box):
    box.ctx.set_option("chunk_items", 100)
    try:
        info, _, got, st, _ = box.bake_sparse(0, 512)
    finally:
        box.ctx.set_option("chunk_items", 0)
    pi, _, pw = box.parent(WHOLE)
    assert info == pi and got.tobytes() == pw.tobytes()
    assert st["chunks"] == 6 and st["merges"] >= 5 and st["dense_chunks"] == 0 and st["codes"] == info.deposits


# ---- 5. every bucket filler ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(maxsize=None)
def _small_box(tile_size):
    from fmgi import scene

    return scene.box_scene(200, tile_size=tile_size)


def _filler(torch, sc, spa, offsets, lo, hi, names, kernel=fmgi.KERNEL_AUTO, **options):
    """bake_sparse of items [lo, hi) against bake_states + compact on the same context; the instance's name"""
    dev = Dev(torch, sc)
    try:
        dev.ctx.set_accumulation(fmgi.ACCUM_STREAM)
        dev.ctx.plan(spa, rng_offsets=offsets)
        for k, v in options.items():
            dev.ctx.set_option(k, v)
        info, _, got, st, name = dev.bake_sparse(lo, hi, kernel)
        print(f"{sc.name} [{lo}, {hi}): {info} {st} {name}")
        for want in names:
            assert want in name, name
        assert "AccState" not in name
        assert st["dense_chunks"] == 0 and st["codes"] == info.deposits
        # the scratch follows the codes (one batch of at most 64 Mi codes = 256 MB, the blob, its pieces), not
        # 1024 x T: below one dense histogram wherever that is larger than a batch
        if fmgi.states_bytes(dev.T) > 512 << 20:
            assert st["scratch_bytes"] < fmgi.states_bytes(dev.T)
        pi, _, pw = dev.states_compact(((lo, hi),), kernel)
        assert info == pi and got.tobytes() == pw.tobytes()
        assert dev.ctx.accumulation == fmgi.ACCUM_STREAM
    finally:
        dev.close()


def test_filler_box200_shared_staged(torch_cuda, box200, offsets):
    _filler(torch_cuda, box200, BOX_SPA, offsets, 7_000, 27_000, ["AccShared"], bucket_fill=2)


def test_filler_box2000_compact_scatter(torch_cuda, box2000, offsets):
    _filler(torch_cuda, box2000, BOX_SPA, offsets, 5_000, 6_000, ["AccScatter"], bucket_fill=1)


def test_filler_one_tile(torch_cuda, offsets):
    sc = _small_box(2.0)
    assert sc.num_texels == 1176
    _filler(torch_cuda, sc, BOX_SPA, offsets, 0, 3000, [])


def test_filler_example_hybrid(torch_cuda, example_scene, offsets):
    _filler(torch_cuda, example_scene, 6_500_000, offsets, 40_000, 52_000, ["ScanHybrid"], kernel=fmgi.KERNEL_HYBRID)


def test_filler_example_cooperative_lanes(torch_cuda, example_scene, offsets):
    _filler(torch_cuda, example_scene, 65_000, offsets, 0, 300, ["ScanFast"])


@pytest.mark.parametrize("fill,name", [(0, "AccStreamT<2>"), (1, "AccScatter"), (2, "AccShared")])
def test_filler_lit_box_every_bucket_fill(box, fill, name):
    box.ctx.set_option("bucket_fill", fill)
    try:
        info, _, got, st, kname = box.bake_sparse(0, 512)
    finally:
        box.ctx.set_option("bucket_fill", -1)
    assert name.replace(" ", "") in kname.replace(" ", ""), kname
    pi, _, pw = box.parent(WHOLE)
    assert info == pi and got.tobytes() == pw.tobytes() and st["dense_chunks"] == 0


# ---- 6. the dense route of a chunk whose bucket fallback fired ------------------------------------------------------------------

def test_fallback_chunks_take_the_dense_route(torch_cuda, box200, offsets):
    lo, hi = 2_000, 6_000
    olm, ost = O.bake(box200, O.schedule_with_offsets(box200, BOX_SPA, offsets), lo, hi)
    dev = Dev(torch_cuda, box200)
    try:
        dev.ctx.set_accumulation(fmgi.ACCUM_STREAM)
        dev.ctx.plan(BOX_SPA, rng_offsets=offsets)
        dev.ctx.set_option("bucket_fill", 2)
        dev.ctx.reset_stats()
        info, blob, want, st, _ = dev.bake_sparse(lo, hi)
        assert st["dense_chunks"] == 0
        for k in ("photons", "deposits", "escapes"):
            assert dev.ctx.stats()[k] == ost[k], k
        lm = dev.zeros(1, dev.T, 4)
        dev.ctx.recolour_sparse([blob.data_ptr()], [info], [[fmgi.Palette.reference()]], [lm[0].data_ptr()],
                                dev.s.cuda_stream)
        dev.s.synchronize()
        assert np.array_equal(lm.cpu().numpy()[0, :, :3], olm)
        for limit in (64, 1):
            dev.ctx.set_option("pool_limit", limit)
            dev.ctx.reset_stats()
            li, _, got, lst, name = dev.bake_sparse(lo, hi)
            print(f"pool_limit {limit}: {lst} {name}")
            assert li == info and got.tobytes() == want.tobytes()
            assert lst["dense_chunks"] > 0 and lst["dense_chunks"] == lst["chunks"]
            assert lst["scratch_bytes"] >= fmgi.states_bytes(dev.T)
            stats = dev.ctx.stats()
            for k in ("photons", "deposits", "escapes"):  # every item counted once
                assert stats[k] == ost[k], k
            assert stats["bucket_fallback_codes"] == 0  # put back with the rest of the dropped chunk's stats
        dev.ctx.set_option("pool_limit", 0)
        hi2, _, got, st, _ = dev.bake_sparse(lo, hi)  # healthy again: no dense scratch is left allocated
        assert hi2 == info and got.tobytes() == want.tobytes()
        assert st["dense_chunks"] == 0 and st["scratch_bytes"] < fmgi.states_bytes(dev.T)
    finally:
        dev.close()


# ---- 7. an unsupported scene ---------------------------------------------------------------------------------------------------

def test_unsupported_scene_is_refused_and_nothing_is_held(torch_cuda, offsets):
    sc = fmgi.scene.load_geometry(os.path.join(GOLDEN, "apartment30_geometry.bin"), "apartment30")
    dev = Dev(torch_cuda, sc)
    try:
        assert sc.num_texels > 63 * 2048 and not dev.ctx.bake_sparse_supported()
        dev.ctx.plan(65_000, rng_offsets=offsets)
        with pytest.raises(fmgi.FmgiError, match=r"\(-4\).*63 tiles"):
            dev.ctx.bake_sparse(0, 10, fmgi.KERNEL_AUTO, dev.s.cuda_stream)
        codes = dev.zeros(16)
        with pytest.raises(fmgi.FmgiError, match=r"\(-4\).*63 tiles"):
            dev.ctx.sparse_from_codes(codes.data_ptr(), 16, dev.s.cuda_stream)
        info = fmgi.SparseInfo()
        info.num_texels, info.num_blocks = sc.num_texels, (sc.num_texels + 63) // 64
        with pytest.raises(fmgi.FmgiError, match=r"\(-4\).*held"):
            dev.ctx.bake_sparse_take(info, codes.data_ptr(), dev.s.cuda_stream)
    finally:
        dev.close()


def test_set_scene_releases_a_held_result(torch_cuda):
    dev = Dev(torch_cuda, _synthetic_scene(65))
    try:
        d = dev.upload(H.code([1, 2, 3], [4, 5, 6]), np.int32)
        info, _ = dev.ctx.sparse_from_codes(d.data_ptr(), 3, dev.s.cuda_stream)
        assert info.cells == 3
        dev.ctx.set_scene(_synthetic_scene(65))
        buf, _ = dev.guarded(info)
        with pytest.raises(fmgi.FmgiError, match=r"\(-4\).*held"):
            dev.ctx.bake_sparse_take(info, buf.data_ptr(), dev.s.cuda_stream)
        info, _ = dev.ctx.sparse_from_codes(d.data_ptr(), 3, dev.s.cuda_stream)
        wrong = fmgi.SparseInfo.from_buffer_copy(info)
        wrong.rows += 1
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\).*rows"):
            dev.ctx.bake_sparse_take(wrong, buf.data_ptr(), dev.s.cuda_stream)
        dev.take(info)
    finally:
        dev.close()


# ---- 8. tools/relight.py ---------------------------------------------------------------------------------------------------------

def test_relight_sparse_from_codes_equals_sparse(tmp_path):
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": [{"scale": 0.5, "floor_tint": [1.0, 0.5, 0.25]}]}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    tool = [sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4", "--with-light",
            "--scenarios", str(tmp_path / "scenarios.json"), "--spa", str(R.SPA), "--per-light", "--offsets",
            os.path.join(GOLDEN, "glibc_rand_4096.npy")]
    out = {}
    for name, flag in (("sparse", "--sparse"), ("codes", "--sparse-from-codes")):
        r = subprocess.run(tool + [flag, "--save-bake", str(tmp_path / f"{name}.npz"), "-o", str(tmp_path / name)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = r.stdout
        print(r.stdout)
        assert "512 items traced" in r.stdout and "fill 0." in r.stdout and "bake saved" in r.stdout
    assert "from the deposit codes" in out["codes"] and "0 dense chunks" in out["codes"]
    assert "from the deposit codes" not in out["sparse"]
    for scn in ("day", "evening"):
        for f in ("texels.npy", "tiles.npy"):
            assert (tmp_path / "sparse" / scn / f).read_bytes() == (tmp_path / "codes" / scn / f).read_bytes(), (scn, f)
    sc = R.lit_box()[0]
    a, b = fmgi.load_bake(str(tmp_path / "sparse.npz"), sc), fmgi.load_bake(str(tmp_path / "codes.npz"), sc)
    assert len(a["groups"]) == len(b["groups"]) == 2
    for ga, gb in zip(a["groups"], b["groups"]):
        assert ga["info"] == gb["info"] and ga["blob"].tobytes() == gb["blob"].tobytes()
        assert (ga["label"], ga["item_begin"], ga["item_end"]) == (gb["label"], gb["item_begin"], gb["item_end"])
