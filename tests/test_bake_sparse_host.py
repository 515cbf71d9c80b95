"""CPU tests of the sparse histograms built from deposit codes: the argument checks of the six calls
in their order on a host-only context, fmgi_bake_sparse_supported on three scenes, the restated sum on hand-made
blobs, and the new argument of tools/relight.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bake_sparse_restate as H
import fmgi
import recolour_events as R
import sparse_restate as S
from conftest import GOLDEN, REPO
from fmgi import _lib

ARG, STATE, NODEV = -3, -4, -1
T_BOX = 2152


def _info(T, rows=3, too_large=0, blocks=None):
    i = fmgi.SparseInfo()
    i.num_texels, i.num_blocks = T, (T + 63) // 64 if blocks is None else blocks
    i.rows, i.cells, i.deposits, i.too_large = rows, rows, rows, too_large
    return i


@pytest.fixture(scope="module")
def ctxs():
    """(the lit box with its plan, no scene, the 30-room layout, the lit box on the sliced stream)"""
    sc, _, offsets = R.lit_box()
    box = fmgi.Context(fmgi.HOST_ONLY)
    box.set_scene(sc)
    assert box.plan(R.SPA, rng_offsets=offsets) == 512
    empty = fmgi.Context(fmgi.HOST_ONLY)
    big = fmgi.Context(fmgi.HOST_ONLY)
    big.set_scene(fmgi.scene.load_geometry(os.path.join(GOLDEN, "apartment30_geometry.bin"), "apartment30"))
    sliced = fmgi.Context(fmgi.HOST_ONLY)
    sliced.set_scene(sc)
    sliced.set_option("stream_layout", 0)
    sliced.plan(R.SPA, rng_offsets=offsets)
    yield box, empty, big, sliced
    for c in (box, empty, big, sliced):
        c.close()


def test_the_new_names_are_exported():
    for name in ("fmgi_bake_sparse_supported", "fmgi_bake_sparse", "fmgi_bake_sparse_take", "fmgi_sparse_from_codes",
                 "fmgi_sparse_add_measure", "fmgi_sparse_add", "fmgi_bake_sparse_get_stats"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert _lib.OPTIONS["hist_batch"] == 10


def test_supported_on_three_scenes(ctxs):
    box, empty, big, sliced = ctxs
    lib = _lib.load()
    assert box.scene.num_texels == T_BOX and box.bake_sparse_supported() is True
    assert big.scene.num_texels > 63 * 2048 and big.bake_sparse_supported() is False
    assert sliced.bake_sparse_supported() is False
    assert lib.fmgi_bake_sparse_supported(None) == ARG
    assert lib.fmgi_bake_sparse_supported(empty.h) == STATE
    with pytest.raises(fmgi.FmgiError, match=r"\(-4\)"):
        empty.bake_sparse_supported()


def test_bake_sparse_argument_errors_in_order(ctxs):
    box, empty, big, sliced = ctxs
    lib = _lib.load()
    out = fmgi.SparseInfo()
    f = lib.fmgi_bake_sparse
    assert f(None, 0, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == ARG
    assert f(box.h, 0, 1, fmgi.KERNEL_AUTO, None, None) == ARG
    assert f(box.h, 2, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == ARG
    assert "reversed" in _lib.last_error()
    assert f(empty.h, 2, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == ARG     # ARG before the missing scene
    assert f(empty.h, 0, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == STATE
    assert "no scene" in _lib.last_error()
    noplan = fmgi.Context(fmgi.HOST_ONLY)
    noplan.set_scene(box.scene)
    try:
        assert f(noplan.h, 0, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == STATE
        assert "no plan" in _lib.last_error()
    finally:
        noplan.close()
    # a range past the plan: fmgi_bake_states' report (its code and text), before the layout and the device
    assert f(box.h, 0, 513, fmgi.KERNEL_AUTO, C.byref(out), None) == ARG
    assert "outside plan of 512" in _lib.last_error()
    assert f(sliced.h, 0, 513, fmgi.KERNEL_AUTO, C.byref(out), None) == ARG
    assert f(sliced.h, 0, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == STATE   # unsupported before NO_DEVICE
    assert "63 tiles" in _lib.last_error()
    assert f(box.h, 0, 1, fmgi.KERNEL_AUTO, C.byref(out), None) == NODEV
    assert f(box.h, 0, 0, fmgi.KERNEL_AUTO, C.byref(out), None) == NODEV
    with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
        box.bake_sparse(0, 1)


def test_from_codes_argument_errors_in_order(ctxs):
    box, empty, big, sliced = ctxs
    lib = _lib.load()
    out, skipped, p16 = fmgi.SparseInfo(), C.c_uint64(7), C.c_void_p(16)
    f = lib.fmgi_sparse_from_codes
    assert f(None, p16, 1, C.byref(out), C.byref(skipped), None) == ARG
    assert f(box.h, None, 1, C.byref(out), C.byref(skipped), None) == ARG
    assert f(box.h, p16, 1, None, C.byref(skipped), None) == ARG
    assert f(box.h, p16, 1 << 32, C.byref(out), None, None) == ARG
    assert f(empty.h, None, 1, C.byref(out), None, None) == ARG
    assert f(empty.h, p16, 1, C.byref(out), None, None) == STATE
    assert f(big.h, p16, 1, C.byref(out), None, None) == STATE
    assert "63 tiles" in _lib.last_error()
    assert f(sliced.h, p16, 1, C.byref(out), None, None) == STATE
    assert f(box.h, p16, 1, C.byref(out), None, None) == NODEV       # skipped may be NULL
    assert f(box.h, p16, 1, C.byref(out), C.byref(skipped), None) == NODEV
    assert skipped.value == 7                                         # nothing was written
    with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
        box.sparse_from_codes(16, 1)


def test_take_and_stats_argument_errors_in_order(ctxs):
    box, empty, big, sliced = ctxs
    lib = _lib.load()
    p16 = C.c_void_p(16)
    ok, other = _info(T_BOX), _info(70)
    bad_blocks, large = _info(T_BOX, blocks=33), _info(T_BOX, too_large=1)
    f = lib.fmgi_bake_sparse_take
    assert f(None, C.byref(ok), p16, None) == ARG
    assert f(box.h, None, p16, None) == ARG
    assert f(box.h, C.byref(ok), None, None) == ARG
    assert f(box.h, C.byref(bad_blocks), p16, None) == ARG
    assert "num_blocks" in _lib.last_error()
    assert f(box.h, C.byref(large), p16, None) == ARG
    assert "too_large" in _lib.last_error()
    assert f(empty.h, C.byref(large), p16, None) == ARG
    assert f(empty.h, C.byref(ok), p16, None) == STATE
    assert f(box.h, C.byref(other), p16, None) == ARG
    assert "70 texels" in _lib.last_error()
    assert f(empty.h, C.byref(other), p16, None) == STATE
    assert f(box.h, C.byref(ok), p16, None) == NODEV
    st = _lib.BakeSparseStats()
    assert lib.fmgi_bake_sparse_get_stats(None, C.byref(st)) == ARG
    assert lib.fmgi_bake_sparse_get_stats(box.h, None) == ARG
    assert box.bake_sparse_stats() == dict(chunks=0, merges=0, dense_chunks=0, codes=0, scratch_bytes=0)


def test_sum_argument_errors_in_order(ctxs):
    box, empty, big, sliced = ctxs
    lib = _lib.load()
    p16, p32, p48 = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)
    ok, other = _info(T_BOX), _info(70)
    bad_blocks, large = _info(T_BOX, blocks=33), _info(T_BOX, too_large=1)
    out = fmgi.SparseInfo()

    def measure(c, a=p16, ai=ok, b=p32, bi=ok, o=out):
        r = lambda v: None if v is None else C.byref(v)
        return lib.fmgi_sparse_add_measure(c, a, r(ai), b, r(bi), r(o), None)

    def add(c, a=p16, ai=ok, b=p32, bi=ok, si=ok, s=p48):
        r = lambda v: None if v is None else C.byref(v)
        return lib.fmgi_sparse_add(c, a, r(ai), b, r(bi), r(si), s, None)

    for f in (measure, add):
        assert f(None) == ARG
        assert f(box.h, a=None) == ARG
        assert f(box.h, ai=None) == ARG
        assert f(box.h, b=None) == ARG
        assert f(box.h, bi=None) == ARG
        assert f(box.h, ai=bad_blocks) == ARG
        assert "num_blocks" in _lib.last_error()
        assert f(box.h, bi=large) == ARG
        assert "too_large" in _lib.last_error()
        assert f(empty.h, bi=large) == ARG      # a bad info comes before the missing scene
        assert f(empty.h) == STATE
        assert f(box.h, ai=other) == ARG        # a well-formed info of another texel count
        assert f(box.h, bi=other) == ARG
        assert f(empty.h, ai=other) == STATE    # ... comes after the missing scene
        assert f(box.h) == NODEV
        assert f(big.h, ai=_info(big.scene.num_texels), bi=_info(big.scene.num_texels),
                 **({} if f is measure else {"si": _info(big.scene.num_texels)})) == NODEV  # any scene can be summed
    assert measure(box.h, o=None) == ARG
    assert add(box.h, si=None) == ARG
    assert add(box.h, s=None) == ARG
    assert add(box.h, si=large) == ARG
    assert add(box.h, si=other) == ARG
    assert add(empty.h, si=other) == STATE
    with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
        box.sparse_add_measure(16, ok, 32, ok)
    with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
        box.sparse_add(16, ok, 32, ok, ok, 48)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def _dense(T, cells):
    d = np.zeros((1024, T), np.uint64)
    for (s, t), n in cells.items():
        d[s, t] = n
    return d


@pytest.mark.parametrize("T", [1, 65])
def test_restated_sum_on_hand_made_blobs(T):
    last = T - 1
    a = _dense(T, {(0, 0): 5, (512, 0): 1, (1023, last): 9})
    a_blob, a_info = S.pack(a)
    # disjoint cells: every cell of either is a cell of the sum, each texel's states ascending
    b = _dense(T, {(1, 0): 7, (700, last): 2})
    blob, info = H.add(a_blob, S.pack(b)[0], T)
    assert info["cells"] == 5 and info["deposits"] == 24 and info["too_large"] == 0
    assert np.array_equal(S.unpack(blob, T), a + b)
    assert fmgi.sparse_check(blob, T).as_dict() == info
    ts, ss, ns = S.cells(blob, T)
    assert sorted(zip(ts, ss, ns)) == sorted([(0, 0, 5), (0, 1, 7), (0, 512, 1), (last, 700, 2), (last, 1023, 9)])
    if T == 1:
        assert info["rows"] == 5 and [int(v) >> 54 for v in blob[2:: 64][:5]] == [0, 1, 512, 700, 1023]
    else:
        assert info["rows"] == 3 + 2 and [int(v) for v in blob[:3]] == [0, 3, 5]
    # equal cells: the counts add, the cells stay
    blob, info = H.add(a_blob, a_blob, T)
    assert info["cells"] == a_info["cells"] and info["rows"] == a_info["rows"] and info["deposits"] == 30
    assert np.array_equal(S.unpack(blob, T), a * np.uint64(2))
    # a sum of 2^54 has no sparse form
    big = _dense(T, {(1023, last): (1 << 54) - 9, (3, 0): 1})
    blob, info = H.add(a_blob, S.pack(big)[0], T)
    assert blob is None and info["too_large"] == 1 and info["cells"] == 4
    assert info["deposits"] == 15 + (1 << 54) - 9 + 1
    blob, info = H.add(a_blob, S.pack(_dense(T, {(1023, last): (1 << 54) - 10}))[0], T)
    assert blob is not None and info["too_large"] == 0      # one below the limit still has
    # a + empty == a
    blob, info = H.add(a_blob, S.pack(np.zeros((1024, T), np.uint64))[0], T)
    assert blob.tobytes() == a_blob.tobytes() and info == a_info


def test_restated_histogram_of_codes():
    T = 65
    codes = np.concatenate([H.code([0, 0, 0, 64, 64, 31, 32], [5, 5, 1023, 0, 0, 512, 512]),
                            np.array([H.PAD, H.PAD], np.uint32), H.code([65, 70], [1, 2])])
    blob, info, skipped = H.from_codes(codes, T)
    assert skipped == 2 and info["deposits"] == 7 and info["cells"] == 5 and info["rows"] == 2 + 1
    want = _dense(T, {(5, 0): 2, (1023, 0): 1, (0, 64): 2, (512, 31): 1, (512, 32): 1})
    assert np.array_equal(S.unpack(blob, T), want)
    empty, einfo, _ = H.from_codes(np.zeros(0, np.uint32), T)
    assert einfo["rows"] == 0 and empty.nbytes == 8 * 3 and not empty.any()


# ---- tools/relight.py ------------------------------------------------------------------------------------------------

def _relight():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
    finally:
        sys.path.pop(0)
    return relight


def test_relight_sparse_from_codes_arguments(tmp_path):
    relight = _relight()
    base = ["box200", "--spa", "2000", "--scenarios", "s.json"]
    a = relight.parse_args(base + ["--sparse-from-codes"])
    assert a.sparse_from_codes and a.sparse and a.save_bake is None
    a = relight.parse_args(base + ["--sparse-from-codes", "--save-bake", "b.npz"])
    assert a.sparse_from_codes and a.sparse and a.save_bake == "b.npz"
    a = relight.parse_args(base + ["--sparse"])
    assert a.sparse and not a.sparse_from_codes
    assert not relight.parse_args(base).sparse_from_codes
    with pytest.raises(SystemExit):
        relight.parse_args(["box200", "--scenarios", "s.json", "--sparse-from-codes"])  # --spa is still required
    with pytest.raises(SystemExit):
        relight.parse_args(["box200", "--scenarios", "s.json", "--load-bake", "b.npz", "--sparse-from-codes"])
    # the same refusal from the command line, in a process that sees no device
    (tmp_path / "s.json").write_text(json.dumps([{"name": "day"}]))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--scenarios",
                        str(tmp_path / "s.json"), "--load-bake", "b.npz", "--sparse-from-codes"], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 2 and "nothing is traced" in r.stderr and "no HIP device" not in r.stderr
