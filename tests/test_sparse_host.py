"""CPU tests of the sparse photon histograms' host side: fmgi_sparse_bytes and fmgi_sparse_check
against the numpy restatement of the format on the lit box's event-derived histograms, every violation the checker
names, the argument checks of the four device-facing calls on a host-only context, the bake file (fmgi.save_bake /
fmgi.load_bake) and the new arguments of tools/relight.py."""
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
from conftest import REPO
from fmgi import _lib

T_BOX = 2152
WHOLE = ((0, 512),)
# the issue's table: ranges -> (cells, rows, bytes, deposits)
EXPECT = {R.RANGES: (46_916, 1_230, 630_040, 102_400), WHOLE: (92_513, 2_230, 1_142_040, 409_600)}

_PACKED = {}


def packed(ranges):
    """(blob, info) of the event-derived histogram of `ranges` (made once, read-only)."""
    if ranges not in _PACKED:
        blob, info = S.pack(R.dense_histogram(ranges))
        blob.setflags(write=False)
        _PACKED[ranges] = (blob, info)
    return _PACKED[ranges]


def test_sparse_bytes_is_the_formula():
    assert fmgi.sparse_bytes(2152, 2230) == 1_142_040
    for T, rows in ((1, 0), (1, 1024), (63, 5), (64, 5), (65, 5), (257, 0), (2152, 1230), (4_194_304, 70_000_000)):
        assert fmgi.sparse_bytes(T, rows) == 8 * ((T + 63) // 64 + 1) + 512 * rows == S.nbytes(T, rows)
    for T in (0, -1, -(2**31)):
        assert fmgi.sparse_bytes(T, 7) == 0
    assert _lib.SPARSE_COUNT_BITS == S.COUNT_BITS == 54 and fmgi.SPARSE_COUNT_BITS == 54


@pytest.mark.parametrize("ranges", [R.RANGES, WHOLE], ids=["128items", "512items"])
def test_restated_blobs_of_the_lit_box(ranges):
    assert R.lit_box()[0].num_texels == T_BOX
    blob, info = packed(ranges)
    cells, rows, nbytes, deposits = EXPECT[ranges]
    assert (info["cells"], info["rows"], blob.nbytes, info["deposits"]) == (cells, rows, nbytes, deposits)
    assert info["num_texels"] == T_BOX and info["num_blocks"] == 34 and info["too_large"] == 0
    assert nbytes == fmgi.sparse_bytes(T_BOX, rows)
    assert 10 * nbytes < fmgi.states_bytes(T_BOX)
    print(f"{nbytes} bytes = {100 * nbytes / fmgi.states_bytes(T_BOX):.1f} % of dense, fill {cells / (64 * rows):.2f}")
    got = fmgi.sparse_check(blob, T_BOX)
    assert isinstance(got, fmgi.SparseInfo) and got.as_dict() == info
    assert fmgi.sparse_check(blob.tobytes(), T_BOX).as_dict() == info  # bytes are taken too
    assert np.array_equal(S.unpack(blob, T_BOX), R.dense_histogram(ranges))


def _small():
    """a histogram of 70 texels (two blocks; 6 live lanes in the second) with a few cells, and its blob"""
    d = np.zeros((1024, 70), np.uint64)
    d[3, 0], d[512, 0], d[1023, 0] = 5, 1, (1 << 54) - 1
    d[0, 1] = 9
    d[7, 63] = 2
    d[100, 64], d[200, 64] = 4, 6
    d[300, 69] = 8
    blob, info = S.pack(d)
    assert info["rows"] == 5 and [int(v) for v in blob[:3]] == [0, 3, 5]
    return d, blob, info


def _entry(blob, T, row, lane):
    return (T + 63) // 64 + 1 + 64 * row + lane


def _violations():
    d, blob, info = _small()
    T = 70
    out = {}
    out["truncated"] = (blob.tobytes()[:16], "truncated")           # not even off[]
    out["short"] = (blob.tobytes()[:-8], "size")                    # off[] whole, an entry missing
    out["long"] = (blob.tobytes() + bytes(8), "size")
    b = blob.copy(); b[0] = 1
    out["off0"] = (b, r"off\[0\]")
    b = blob.copy(); b[1] = 6                                        # 0, 6, 5
    out["decreasing"] = (b, "decreases")
    b = blob.copy(); b[_entry(b, T, 1, 0)] = b[_entry(b, T, 0, 0)]   # texel 0: state 3 twice
    out["duplicate"] = (b, "duplicate state 3")
    b = blob.copy()
    i, j = _entry(b, T, 0, 0), _entry(b, T, 1, 0)
    b[i], b[j] = b[j], b[i]                                          # texel 0: 512, 3, 1023
    out["descending"] = (b, "descending")
    b = blob.copy()
    b[_entry(b, T, 1, 1)] = b[_entry(b, T, 0, 1)]; b[_entry(b, T, 0, 1)] = 0  # texel 1: padding, then its cell
    out["padding_first"] = (b, "padding before")
    b = blob.copy(); b[_entry(b, T, 3, 6)] = (5 << 54) | 1           # block 1, lane 6 = texel 70 >= T
    out["past_T"] = (b, "past the last texel")
    # a spare row: block 1 gets a third, all-padding row
    b = np.concatenate([blob[:3], blob[3:], np.zeros(64, np.uint64)]); b[2] = 6
    out["spare_row"] = (b, "spare row")
    return T, blob, info, out


_T, _BLOB, _INFO, _VIOL = _violations()


def test_sparse_check_accepts_the_small_blob():
    assert fmgi.sparse_check(_BLOB, _T).as_dict() == _INFO
    z, zi = S.pack(np.zeros((1024, 130), np.uint64))
    assert z.nbytes == 8 * 4 and zi["rows"] == 0 and fmgi.sparse_check(z, 130).as_dict() == zi
    info = fmgi.SparseInfo()
    assert _lib.load().fmgi_sparse_check(None, 64, 70, C.byref(info)) == -3
    assert _lib.load().fmgi_sparse_check(_BLOB.ctypes.data_as(C.c_void_p), _BLOB.nbytes, 70, None) == -3
    assert _lib.load().fmgi_sparse_check(_BLOB.ctypes.data_as(C.c_void_p), _BLOB.nbytes, 0, C.byref(info)) == -3


@pytest.mark.parametrize("name", sorted(_VIOL))
def test_sparse_check_names_the_violation(name):
    bad, word = _VIOL[name]
    with pytest.raises(fmgi.FmgiError, match=r"\(-3\).*" + word):
        fmgi.sparse_check(bad, _T)


# ---- argument checks, in their order, on a host-only context ---------------------------------------------------------

def _info(T, rows=3, too_large=0, blocks=None):
    i = fmgi.SparseInfo()
    i.num_texels, i.num_blocks = T, (T + 63) // 64 if blocks is None else blocks
    i.rows, i.cells, i.deposits, i.too_large = rows, rows, rows, too_large
    return i


def _rs(ctx, blobs, infos, pals, lms, groups=None, scenarios=None):
    G = len(blobs) if groups is None else groups
    K = len(lms) if scenarios is None else scenarios
    sp = (C.c_void_p * max(len(blobs), 1))(*blobs)
    lp = (C.c_void_p * max(len(lms), 1))(*lms)
    inf = (fmgi.SparseInfo * max(len(infos), 1))()
    for g, i in enumerate(infos):
        C.memmove(C.byref(inf, g * C.sizeof(fmgi.SparseInfo)), C.byref(i), C.sizeof(fmgi.SparseInfo))
    pal = (fmgi.Palette * max(len(pals), 1))(*pals)
    return ctx.lib.fmgi_recolour_sparse(ctx.h, sp, inf, G, pal, K, lp, None)


def test_argument_errors_come_in_order_before_the_device():
    ARG, STATE, NODEV = -3, -4, -1
    sc = R.lit_box()[0]
    lib = _lib.load()
    ctx = fmgi.Context(fmgi.HOST_ONLY)
    ctx.set_scene(sc)
    empty = fmgi.Context(fmgi.HOST_ONLY)  # no scene
    p16 = C.c_void_p(16)
    ok, other = _info(T_BOX), _info(70)
    bad_blocks, big = _info(T_BOX, blocks=33), _info(T_BOX, too_large=1)
    out = fmgi.SparseInfo()
    try:
        # measure: NULLs, then the scene, then the device
        assert lib.fmgi_sparse_measure(None, p16, C.byref(out), None) == ARG
        assert lib.fmgi_sparse_measure(ctx.h, None, C.byref(out), None) == ARG
        assert lib.fmgi_sparse_measure(ctx.h, p16, None, None) == ARG
        assert lib.fmgi_sparse_measure(empty.h, None, C.byref(out), None) == ARG   # ARG before STATE
        assert lib.fmgi_sparse_measure(empty.h, p16, C.byref(out), None) == STATE
        assert lib.fmgi_sparse_measure(ctx.h, p16, C.byref(out), None) == NODEV
        for f in (lib.fmgi_sparse_compact, lib.fmgi_sparse_expand):
            # (ctx, src, info, dst, stream) for both: compact's info sits between its two buffers as expand's does
            assert f(None, p16, C.byref(ok), p16, None) == ARG
            assert f(ctx.h, None, C.byref(ok), p16, None) == ARG
            assert f(ctx.h, p16, None, p16, None) == ARG
            assert f(ctx.h, p16, C.byref(ok), None, None) == ARG
            assert f(ctx.h, p16, C.byref(bad_blocks), p16, None) == ARG
            assert "num_blocks" in fmgi._lib.last_error()
            assert f(ctx.h, p16, C.byref(big), p16, None) == ARG
            assert "too_large" in fmgi._lib.last_error()
            assert f(empty.h, p16, C.byref(big), p16, None) == ARG      # a bad info comes before the missing scene
            assert f(empty.h, p16, C.byref(ok), p16, None) == STATE
            assert f(ctx.h, p16, C.byref(other), p16, None) == ARG      # a well-formed info of another texel count
            assert "70 texels" in fmgi._lib.last_error()
            assert f(empty.h, p16, C.byref(other), p16, None) == STATE  # ... comes after the missing scene
            assert f(ctx.h, p16, C.byref(ok), p16, None) == NODEV
        pal = fmgi.Palette()
        nan = fmgi.Palette(albedo=float("nan"))
        assert lib.fmgi_recolour_sparse(None, None, None, 1, None, 1, None, None) == ARG
        assert lib.fmgi_recolour_sparse(ctx.h, None, None, 1, None, 1, None, None) == ARG
        assert _rs(ctx, [16], [ok], [pal], [16], groups=0) == ARG
        assert _rs(ctx, [16], [ok], [pal], [16], scenarios=0) == ARG
        assert _rs(ctx, [None], [ok], [pal], [16]) == ARG
        assert _rs(ctx, [16], [ok], [pal], [None]) == ARG
        assert _rs(ctx, [16], [ok], [nan], [16]) == ARG
        assert _rs(ctx, [16, 16], [ok, ok], [pal, nan], [16]) == ARG
        assert _rs(ctx, [16, 16], [ok, bad_blocks], [pal, pal], [16]) == ARG
        assert _rs(ctx, [16, 16], [ok, big], [pal, pal], [16]) == ARG
        assert _rs(empty, [16], [big], [pal], [16]) == ARG
        assert _rs(empty, [16], [ok], [pal], [16]) == STATE
        assert _rs(empty, [16], [other], [pal], [16]) == STATE
        assert _rs(ctx, [16, 16], [ok, other], [pal, pal], [16]) == ARG
        assert _rs(ctx, [16], [ok], [pal], [16]) == NODEV
        assert _rs(ctx, [16, 32], [ok, ok], [pal] * 18, [16] * 9) == NODEV
        # the Python mirror raises with the code
        with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
            ctx.sparse_measure(16)
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):
            ctx.sparse_compact(16, big, 16)
        with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
            ctx.sparse_expand(16, ok, 16)
        with pytest.raises(fmgi.FmgiError, match=r"\(-1\)"):
            ctx.recolour_sparse([16], [ok], [[pal]], [16])
        with pytest.raises(fmgi.FmgiError, match="infos"):
            ctx.recolour_sparse([16], [ok, ok], [[pal]], [16])
    finally:
        ctx.close()
        empty.close()


def test_the_new_names_are_exported():
    for name in ("fmgi_sparse_bytes", "fmgi_sparse_measure", "fmgi_sparse_compact", "fmgi_sparse_expand",
                 "fmgi_recolour_sparse", "fmgi_sparse_check"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)


# ---- the bake file ---------------------------------------------------------------------------------------------------

def _launches():
    L = np.zeros(2, fmgi.LAUNCH_DTYPE)
    L["item_begin"], L["count"], L["rng_offset"], L["source"], L["is_window"] = [0, 256], 256, [11, 22], [0, 1], [1, 0]
    return L


def _save(path, sc):
    window, lamp = (S.pack(R.dense_histogram(((b, e),)))[0] for b, e in R.RANGES)
    fmgi.save_bake(path, sc, R.SPA, 256, _launches(), [("windows", 0, 64, True, window), ("lights", 256, 320, False, lamp)])
    return window, lamp


@pytest.fixture(scope="module")
def bake_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bake") / "lit_box.npz")
    return (path,) + _save(path, R.lit_box()[0])


def test_bake_file_round_trip(bake_file):
    path, window, lamp = bake_file
    sc = R.lit_box()[0]
    with np.load(path, allow_pickle=False) as z:
        assert str(z["format"]) == "fmgi-bake-1" == fmgi.BAKE_FORMAT
        assert str(z["scene_sha256"]) == fmgi.scene_hash(sc) and len(fmgi.scene_hash(sc)) == 64
        assert z["blob_0"].dtype == np.uint64
    for given in (sc, None):
        b = fmgi.load_bake(path, given)
        assert (b["spa"], b["wg"], b["num_texels"]) == (R.SPA, 256, T_BOX)
        assert b["launches"].dtype == fmgi.LAUNCH_DTYPE and b["launches"].tobytes() == _launches().tobytes()
        g0, g1 = b["groups"]
        assert (g0["label"], g0["item_begin"], g0["item_end"], g0["is_window"]) == ("windows", 0, 64, True)
        assert (g1["label"], g1["item_begin"], g1["item_end"], g1["is_window"]) == ("lights", 256, 320, False)
        assert g0["blob"].dtype == np.uint64 and np.array_equal(g0["blob"], window) and np.array_equal(g1["blob"], lamp)
        assert g0["info"] == fmgi.sparse_check(window, T_BOX) and g0["rows"] == g0["info"].rows
    # the two groups add up to the restated histogram of both ranges
    assert np.array_equal(S.unpack(window, T_BOX) + S.unpack(lamp, T_BOX), R.dense_histogram(R.RANGES))


def _rewrite(src, dst, **changes):
    with np.load(src, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d.update(changes)
    np.savez(dst, **d)
    return dst


def test_load_bake_refuses_what_does_not_fit(bake_file, tmp_path):
    from fmgi import scene

    path, window, _ = bake_file
    unlit = scene.box_scene(200, tile_size=4.0)
    assert unlit.num_texels == T_BOX  # the same lightmap, another scene
    with pytest.raises(ValueError, match="another scene"):
        fmgi.load_bake(path, unlit)
    with pytest.raises(ValueError, match="format tag"):
        fmgi.load_bake(_rewrite(path, str(tmp_path / "tag.npz"), format=np.array("fmgi-bake-0")), None)
    bad = window.copy()
    bad[0] = 1
    with pytest.raises(ValueError, match=r"windows.*off\[0\]"):
        fmgi.load_bake(_rewrite(path, str(tmp_path / "blob.npz"), blob_0=bad), R.lit_box()[0])
    with pytest.raises(fmgi.FmgiError, match=r"off\[0\]"):  # and nothing is written for a blob that fails
        fmgi.save_bake(str(tmp_path / "never.npz"), R.lit_box()[0], R.SPA, 256, _launches(), [("w", 0, 64, True, bad)])
    assert not os.path.exists(tmp_path / "never.npz")


# ---- tools/relight.py ------------------------------------------------------------------------------------------------

def _relight():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
    finally:
        sys.path.pop(0)
    return relight


def test_relight_arguments_for_bake_files():
    relight = _relight()
    a = relight.parse_args(["box200", "--scenarios", "s.json", "--load-bake", "b.npz"])
    assert a.spa is None and a.load_bake == "b.npz" and a.sparse
    a = relight.parse_args(["box200", "--scenarios", "s.json", "--load-bake", "b.npz", "--spa", "2000"])
    assert a.spa == 2000
    with pytest.raises(SystemExit):
        relight.parse_args(["box200", "--scenarios", "s.json"])  # --spa is still required without --load-bake
    with pytest.raises(SystemExit):
        relight.parse_args(["box200", "--scenarios", "s.json", "--sparse"])
    a = relight.parse_args(["box200", "--spa", "2000", "--scenarios", "s.json"])
    assert not a.sparse and a.save_bake is None and a.load_bake is None
    assert relight.parse_args(["box200", "--spa", "2000", "--scenarios", "s.json", "--sparse"]).sparse
    assert relight.parse_args(["box200", "--spa", "2000", "--scenarios", "s.json", "--save-bake", "b.npz"]).sparse


def test_relight_refuses_a_bake_of_another_scene_without_a_device(bake_file, tmp_path):
    path = bake_file[0]
    (tmp_path / "s.json").write_text(json.dumps([{"name": "day"}]))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4"]
    rest = ["--scenarios", str(tmp_path / "s.json"), "--load-bake", path, "-o", str(tmp_path / "out")]
    r = subprocess.run(base + rest, capture_output=True, text=True, timeout=300, env=env)  # the box without its lamp
    assert r.returncode != 0 and "another scene" in r.stderr and "no HIP device" not in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--with-light", "--spa", "1999"] + rest, capture_output=True, text=True, timeout=300,
                       env=env)  # the right scene, another --spa than the file's
    assert r.returncode != 0 and f"--spa {R.SPA}" in r.stderr and "no HIP device" not in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(tmp_path / "out")
