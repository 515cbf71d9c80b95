"""GPU tests of the sparse photon histograms, everything bit for bit: fmgi_sparse_measure,
fmgi_sparse_compact and fmgi_sparse_expand against the numpy restatement of the format on synthetic histograms
(texel counts around a block, empty and full texels, the extreme states and counts); fmgi_recolour_sparse against
fmgi_recolour on the dense input and against Python integers; the offsets' clamp to the host's row count; the real
bake of the lit box; and tools/relight.py --sparse / --save-bake / --load-bake against the dense run."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
import recolour_events as R
import sparse_restate as S
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
BIG = (1 << 54) - 1
EVENING = dict(window_rgb=(2.5, 1.75, 3.0), light_rgb=(31.5, 24.0, 12.125), floor_tint=(0.9, 0.6, 0.3), albedo=0.77)
OFF = dict(window_rgb=(0, 0, 0), light_rgb=(0, 0, 0))


class Dev:
    """a context on a scene of T texels, a stream and the calls of the tests"""

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

    def full(self, value, *shape):
        with self.torch.cuda.stream(self.s):
            return self.torch.full(shape, value, dtype=self.torch.int64, device="cuda:0")

    def upload(self, a):
        """a uint64 (or int64) numpy array -> an int64 device tensor of the same bits"""
        with self.torch.cuda.stream(self.s):
            t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda:0")
        self.s.synchronize()
        return t

    def measure(self, h):
        return self.ctx.sparse_measure(h.data_ptr(), self.s.cuda_stream)

    def compact(self, h, info=None):
        """(device blob, info, the blob's words as uint64 numpy)"""
        info = self.measure(h) if info is None else info
        n = fmgi.sparse_bytes(self.T, info.rows)
        assert n == 8 * ((self.T + 63) // 64 + 1) + 512 * info.rows
        blob = self.zeros(n // 8)
        self.ctx.sparse_compact(h.data_ptr(), info, blob.data_ptr(), self.s.cuda_stream)
        self.s.synchronize()
        return blob, info, blob.cpu().numpy().view(np.uint64)

    def expand(self, blob, info, into):
        self.ctx.sparse_expand(blob.data_ptr(), info, into.data_ptr(), self.s.cuda_stream)
        self.s.synchronize()
        return into.cpu().numpy().view(np.uint64)

    def lightmaps(self, K):
        with self.torch.cuda.stream(self.s):
            lms = self.torch.zeros((K, self.T, 4), dtype=self.torch.int64, device="cuda:0")
            lms[:, :, 3] = 7  # .s[3] is not touched
        return lms

    def recolour_sparse(self, blobs, infos, palettes, lms):
        self.ctx.recolour_sparse([b.data_ptr() for b in blobs], infos, palettes, [lm.data_ptr() for lm in lms],
                                 self.s.cuda_stream)
        self.s.synchronize()
        return lms.cpu().numpy() if hasattr(lms, "cpu") else [lm.cpu().numpy() for lm in lms]

    def recolour(self, hists, palettes, lms):
        self.ctx.recolour([h.data_ptr() for h in hists], palettes, [lm.data_ptr() for lm in lms], self.s.cuda_stream)
        self.s.synchronize()
        return lms.cpu().numpy() if hasattr(lms, "cpu") else [lm.cpu().numpy() for lm in lms]


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


# ---- synthetic histograms ---------------------------------------------------------------------------------------------

def _edges(T, seed=0):
    """about 2 % of the cells at random, and on top the extreme states and counts"""
    rng = np.random.default_rng(100 * T + seed)
    d = rng.integers(1, 200, (1024, T)).astype(np.uint64) * (rng.random((1024, T)) < 0.02)
    d = d.astype(np.uint64)
    d[0, 0], d[512, 0], d[1023, 0] = 1, (1 << 32) + 5, BIG
    d[0, T - 1], d[512, T // 2], d[1023, T - 1] = BIG, 1, (1 << 32) + 5
    d[513, T // 2] = (1 << 32) + 5      # large counts under table values near 2^29 and 2^30 (_palettes)
    d[513, T - 1] = BIG
    return d


def _contents(T, what):
    d = np.zeros((1024, T), np.uint64)
    if what == "zero":
        return d
    if what == "full_texel":  # a texel with all 1024 states next to texels with none
        d[:, T // 2] = np.arange(1, 1025, dtype=np.uint64)
        d[:, T - 1] += np.uint64(3)
        return d
    if what == "edges":
        return _edges(T)
    if what == "edges2":
        return _edges(T, 2)
    assert what == "gap" and T == 257  # blocks 1 and 3 empty between full ones; block 4 is the single last texel
    d = _edges(T, 1)
    d[:, 64:128] = 0
    d[:, 192:256] = 0
    return d


_CASES = [(T, w) for T in (1, 63, 64, 65, 257) for w in ("zero", "full_texel", "edges")] + [(257, "gap")]
_RESTATED = {}


def restated(T, what):
    if (T, what) not in _RESTATED:
        d = _contents(T, what)
        blob, info = S.pack(d)
        for a in (d, blob):
            a.setflags(write=False)
        _RESTATED[(T, what)] = (d, blob, info)
    return _RESTATED[(T, what)]


@pytest.mark.parametrize("T,what", _CASES, ids=[f"{T}-{w}" for T, w in _CASES])
def test_measure_compact_expand(devs, T, what):
    dev = devs(T)
    dense, want_blob, want_info = restated(T, what)
    h = dev.upload(dense)
    info = dev.measure(h)
    print(info, f"fill {info.cells / max(64 * info.rows, 1):.2f}")
    assert info.as_dict() == want_info
    if what == "zero":
        assert info.rows == 0 and fmgi.sparse_bytes(T, 0) == 8 * ((T + 63) // 64 + 1)
    if what == "gap":
        off = [int(v) for v in want_blob[:6]]
        assert off[1] == off[2] and off[3] == off[4] and off[0] < off[1] < off[3] < off[5]
    blob, _, got = dev.compact(h, info)
    assert got.tobytes() == want_blob.tobytes()
    assert np.array_equal(dev.expand(blob, info, dev.zeros(1024, T)), dense)
    assert dev.torch.equal(h, dev.upload(dense))  # the histogram is only read
    three = dev.full(3, 1024, T)
    assert np.array_equal(dev.expand(blob, info, three), dense + np.uint64(3))  # expand adds


def test_a_count_of_2_to_the_54_is_too_large(devs):
    dev = devs(65)
    dense = _edges(65).copy()
    dense[700, 64] = 1 << 54
    h = dev.upload(dense)
    info = fmgi.SparseInfo()
    rc = dev.ctx.lib.fmgi_sparse_measure(dev.ctx.h, C.c_void_p(h.data_ptr()), C.byref(info), C.c_void_p(dev.s.cuda_stream))
    assert rc == -3 and "2^54" in fmgi._lib.last_error()
    assert info.too_large == 1 and info.num_texels == 65 and info.num_blocks == 2
    assert info.cells == int((dense != 0).sum())
    with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
        dev.measure(h)
    with pytest.raises(fmgi.FmgiError, match=r"\(-3\).*too_large"):  # and such an info is refused before any launch
        dev.ctx.sparse_compact(h.data_ptr(), info, h.data_ptr(), dev.s.cuda_stream)


# ---- recolour_sparse against fmgi_recolour and Python integers --------------------------------------------------------

def _palettes(K, G):
    rng = np.random.default_rng(11)
    rows = [[fmgi.Palette(window_rgb=rng.uniform(0, 31.9, 3), light_rgb=rng.uniform(0, 31.9, 3),
                          floor_tint=rng.uniform(0, 1, 3), albedo=rng.uniform(0.3, 1)) for _ in range(G)]
            for _ in range(K)]
    rows[0][0] = fmgi.Palette(window_rgb=(15.999, 31.999, 0.5), albedo=1.0)  # table[513] near 2^29 and 2^30
    if K > 2:
        rows[2] = [fmgi.Palette(**OFF) for _ in range(G)]                   # a scenario with everything off
    if G > 1:
        for row in rows:
            row[1] = fmgi.Palette(**OFF)                                      # group 1 is off in every scenario
    return rows


def _python_fold(blobs, T, pals):
    """[K][T][3] Python integers mod 2^64"""
    out = []
    for row in pals:
        acc = [[0, 0, 0] for _ in range(T)]
        for blob, p in zip(blobs, row):
            table = fmgi.palette_table(p)
            if not table.any():
                continue
            part = S.fold(blob, T, table)
            acc = [[(a + b) & M64 for a, b in zip(x, y)] for x, y in zip(acc, part)]
        out.append(acc)
    return out


@pytest.mark.parametrize("K", [1, 8, 9])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("T", [63, 257])
def test_recolour_sparse_equals_recolour_and_integers(devs, T, G, K):
    dev = devs(T)
    kinds = ["edges", "gap" if T == 257 else "full_texel", "full_texel" if T == 257 else "edges2"][:G]
    dense = [restated(T, w)[0] for w in kinds]
    host_blobs = [restated(T, w)[1] for w in kinds]
    hists = [dev.upload(d) for d in dense]
    blobs, infos = [], []
    for h in hists:
        b, i, _ = dev.compact(h)
        blobs.append(b)
        infos.append(i)
    pals = _palettes(K, G)
    t513 = fmgi.palette_table(pals[0][0])[513]
    assert t513[0] > 0.99 * 2**29 and t513[1] > 0.99 * 2**30
    if G > 1:
        # group 1 is off in every scenario, so its blob must not be read: it is handed another histogram's blob
        # (readable, in bounds under its own info, full of counts), which would show in every sum
        blobs[1], infos[1] = blobs[0], infos[0]
    want_dense = dev.recolour(hists, pals, dev.lightmaps(K))
    lms = dev.lightmaps(K)
    got = dev.recolour_sparse(blobs, infos, pals, lms)
    assert (got[:, :, 3] == 7).all()
    assert np.array_equal(got, want_dense)
    want = np.array(_python_fold(host_blobs, T, pals), dtype=object)
    assert np.array_equal(got[:, :, :3].astype(np.uint64).astype(object), want)
    assert any(v for v in want[0].reshape(-1))
    if K > 2:
        assert not got[2, :, :3].any()
    twice = dev.recolour_sparse(blobs, infos, pals, lms)  # a second call adds the same again
    assert (twice[:, :, 3] == 7).all()
    assert np.array_equal(twice[:, :, :3].astype(np.uint64), got[:, :, :3].astype(np.uint64) * np.uint64(2))


# ---- the clamp ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [65, 257])
def test_offsets_are_clamped_to_the_hosts_rows(devs, T):
    """The blob lies whole in its buffer; the info claims fewer rows than its offsets do. Every read the unclamped
    offsets ask for is inside the allocation, so a missing clamp shows as a wrong sum."""
    dev = devs(T)
    dense, host_blob, want_info = restated(T, "edges")
    h = dev.upload(dense)
    blob, info, _ = dev.compact(h)
    B = (T + 63) // 64
    off = [int(v) for v in host_blob[: B + 1]]
    assert off[B] == info.rows and off[B - 1] > 2
    pal = fmgi.Palette(**EVENING)
    table = fmgi.palette_table(pal)
    full = np.array(S.fold(host_blob, T, table), dtype=object)
    for rows in (off[B] - 1, off[B - 1] - 2, off[1] // 2):  # inside the last block, before it, inside the first
        cut = fmgi.SparseInfo.from_buffer_copy(info)
        cut.rows = rows
        got = dev.recolour_sparse([blob], [cut], [[pal]], dev.lightmaps(1))
        want = np.array(S.fold(host_blob, T, table, rows=rows), dtype=object)
        assert not np.array_equal(want, full)
        assert np.array_equal(got[0, :, :3].astype(np.uint64).astype(object), want), rows
        assert np.array_equal(dev.expand(blob, cut, dev.zeros(1024, T)), S.unpack(host_blob, T, rows=rows)), rows
    # offsets that decrease: the block whose begin exceeds its end is skipped, the others count
    bad = host_blob.copy()
    bad[1] = np.uint64(off[B])  # block 0 = everything; block 1 begins past its end
    dblob = dev.upload(bad)
    got = dev.recolour_sparse([dblob], [info], [[pal]], dev.lightmaps(1))
    want = np.array(S.fold(bad, T, table, rows=info.rows), dtype=object)
    assert np.array_equal(got[0, :, :3].astype(np.uint64).astype(object), want)


def test_compact_with_fewer_rows_than_the_histogram_stays_inside(devs):
    """compact with an info of fewer rows than the histogram has (the histogram `changed since measure`): every
    offset is clamped, and the guard words behind the smaller blob stay as they were."""
    T = 65
    dev = devs(T)
    dense, host_blob, _ = restated(T, "edges")
    h = dev.upload(dense)
    info = dev.measure(h)
    cut = fmgi.SparseInfo.from_buffer_copy(info)
    cut.rows = info.rows // 2
    words = fmgi.sparse_bytes(T, cut.rows) // 8
    buf = dev.full(-1, fmgi.sparse_bytes(T, info.rows) // 8)  # room for the whole blob, all ones
    dev.ctx.sparse_compact(h.data_ptr(), cut, buf.data_ptr(), dev.s.cuda_stream)
    dev.s.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[words:] == np.uint64(M64)).all()
    assert [int(v) for v in got[:3]] == [min(int(v), cut.rows) for v in host_blob[:3]]
    rows0 = min(int(host_blob[1]), cut.rows)  # block 0's clamped rows hold what the whole blob holds there
    assert np.array_equal(got[3: 3 + 64 * rows0], host_blob[3: 3 + 64 * rows0])


# ---- the real bake on the lit box ----------------------------------------------------------------------------------------

class Box(Dev):
    def __init__(self, torch):
        sc, self.L, self.offsets = R.lit_box()
        super().__init__(torch, sc)
        assert self.ctx.plan(R.SPA, rng_offsets=self.offsets) == 512
        self._cache = {}

    def hist(self, ranges):
        if ranges not in self._cache:
            h = self.zeros(1024, self.T)
            for b, e in ranges:
                self.ctx.bake_states(b, e, h.data_ptr(), fmgi.KERNEL_AUTO, self.s.cuda_stream)
            with self.torch.cuda.stream(self.s):
                keep = h.clone()
            self.s.synchronize()
            self._cache[ranges] = (h, keep) + self.compact(h)
        return self._cache[ranges]

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


def test_lit_box_blobs_equal_the_restatement(box):
    import fm_oracle as O

    mode = box.ctx.accumulation
    _, _, blob, info, words = box.hist(R.RANGES)
    want_blob, want_info = S.pack(R.dense_histogram(R.RANGES))
    assert info.as_dict() == want_info and words.tobytes() == want_blob.tobytes()
    assert (info.cells, info.rows, words.nbytes, info.deposits) == (46_916, 1_230, 630_040, 102_400)
    assert fmgi.sparse_check(words, box.T) == info
    _, _, wblob, winfo, wwords = box.hist(WHOLE)
    assert (winfo.cells, winfo.rows, wwords.nbytes, winfo.deposits) == (92_513, 2_230, 1_142_040, 409_600)
    assert fmgi.sparse_check(wwords, box.T) == winfo
    ref = fmgi.Palette.reference()
    lm = box.recolour_sparse([wblob], [winfo], [[ref]], box.zeros(1, box.T, 4))[0]
    assert not lm[:, 3].any()
    assert np.array_equal(lm, box.bake(0, 512))
    assert np.array_equal(lm[:, :3], O.bake(box.sc, box.L, 0, 512)[0])
    assert box.ctx.accumulation == mode


def test_lit_box_groups_add_up(box):
    mode = box.ctx.accumulation
    (wh, wh0, wb, wi, _), (lh, lh0, lb, li, _), (ah, ah0, ab, ai, _) = box.hist(WINDOW), box.hist(LAMP), box.hist(WHOLE)
    assert wi.cells + li.cells == ai.cells and wi.deposits + li.deposits == ai.deposits  # bit 9 keeps them apart
    ref, off, evening = fmgi.Palette(), fmgi.Palette(**OFF), fmgi.Palette(**EVENING)
    both, no_lamp, dusk = box.recolour_sparse([wb, lb], [wi, li], [[ref, ref], [ref, off], [evening, evening]],
                                              box.zeros(3, box.T, 4))
    whole = box.recolour_sparse([ab], [ai], [[ref]], box.zeros(1, box.T, 4))[0]
    assert whole.any() and np.array_equal(both, whole)
    assert np.array_equal(no_lamp, box.bake(0, 256))
    dense = box.recolour([wh, lh], [[evening, evening]], box.zeros(1, box.T, 4))[0]
    assert dense.any() and np.array_equal(dusk, dense)
    # expand(window) + expand(lamp) into one buffer is the whole histogram
    h = box.zeros(1024, box.T)
    box.expand(wb, wi, h)
    assert np.array_equal(box.expand(lb, li, h), ah.cpu().numpy().view(np.uint64))
    for now, before in ((wh, wh0), (lh, lh0), (ah, ah0)):
        assert box.torch.equal(now, before)
    assert box.ctx.accumulation == mode


# ---- tools/relight.py ------------------------------------------------------------------------------------------------------

def test_relight_sparse_save_and_load(tmp_path):
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": [{"scale": 0.5, "floor_tint": [1.0, 0.5, 0.25]}]},
            {"name": "night", "windows": {"off": True}}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    tool = [sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4", "--with-light"]
    common = ["--scenarios", str(tmp_path / "scenarios.json"), "--min-deposits", "64"]
    trace = ["--spa", str(R.SPA), "--per-light", "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy")]
    bake = str(tmp_path / "box.npz")
    runs = {"dense": trace, "sparse": trace + ["--sparse", "--save-bake", bake], "loaded": ["--load-bake", bake]}
    out = {}
    for name, extra in runs.items():
        r = subprocess.run(tool + common + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = r.stdout
        print(r.stdout)
    assert "histograms of" in out["dense"] and "sparse histograms" not in out["dense"]
    assert "512 items traced" in out["sparse"] and "fill 0." in out["sparse"] and "bake saved" in out["sparse"]
    assert "0 items traced" in out["loaded"] and "512 items traced" not in out["loaded"]
    assert len(fmgi.load_bake(bake, R.lit_box()[0])["groups"]) == 2
    for name in ("sparse", "loaded"):
        for scn in ("day", "evening", "night"):
            for f in ("texels.npy", "tiles.npy"):
                a, b = (tmp_path / "dense" / scn / f).read_bytes(), (tmp_path / name / scn / f).read_bytes()
                assert a == b, (name, scn, f)
    assert np.load(tmp_path / "dense" / "day" / "texels.npy").any()
