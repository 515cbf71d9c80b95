"""The radiosity cache on the GPU (include/flatmatch_gi.h). Every comparison is an equality of bits.

  create      sids == the oracle's from a seeded mid-stream libc position, the stream left where the oracle leaves it,
              info == fmgi.radiosity_stats()
  solve       reference palette, 7 rounds == fmgi.radiosity from the same position
              == tests/rad_solve_restate.py for K in {1, 2, 3, 8, 9, 17} (a padded pass, a full pass, the pass
              boundary, three passes) x rounds {1, 7, 8} on the lit box; on open_tilted (586 jobs: no multiple of
              64 or 8, 43 % misses, 1-D mip steps)
              a K = 9 call == nine K = 1 calls; the palette times 2 == the texels times 2
              no emitters, no walls; two calls on one stream with no host synchronise between them
  downstream  ViewCache.tiles on solve's device texels == fmgi.output_tiles of the downloaded texels
              tools/relight_radiosity.py's texels.npy == solve's, its view.ppm == the host path's picture
The scenes have 832 jobs at most: 8.3 M rays.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import emitter_scenes
import fmgi
import rad_cache_cases as CASES
import rad_solve_restate as R
from conftest import REPO
from fmgi import _lib, scene

f32 = np.float32
pytestmark = pytest.mark.gpu
ALL_K, ALL_ROUNDS = 17, (1, 7, 8)

_caches = {}


def _cache(libc, name):
    """(the scene's RadCache, traced from the case's libc position; the rand() drawn right after)"""
    if name not in _caches:
        CASES.seed(libc, name)
        rc = fmgi.RadCache(CASES.get_scene(name))
        _caches[name] = (rc, libc.rand())
    return _caches[name]


@pytest.fixture(scope="module", autouse=True)
def _close_caches():
    yield
    for rc, _ in _caches.values():
        rc.close()
    _caches.clear()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{int(bad.sum())} values differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("name", CASES.NAMES)
def test_create_and_reference_palette(torch_cuda, libc, name):
    sc, _, sids, nxt = CASES.oracle(libc, name)
    rc, after = _cache(libc, name)
    assert after == nxt, "create must leave the libc stream where fmgi_radiosity leaves it"
    assert np.array_equal(rc.sids(), sids)
    CASES.seed(libc, name)
    tex = fmgi.radiosity(sc)
    assert libc.rand() == nxt
    st, info = fmgi.radiosity_stats(), rc.info
    assert {k: info[k] for k in ("jobs", "rects", "texels", "rays")} == {k: st[k] for k in ("jobs", "rects", "texels", "rays")}
    assert (info["windows"], info["lights"]) == (len(sc.windows), len(sc.lights))
    assert info["bytes"] == fmgi.rad_cache_bytes(sc) and info["rays_ms"] > 0 and info["rand_ms"] > 0
    libc.srand(123)
    first = libc.rand()
    libc.srand(123)
    got = rc.solve(fmgi.rad_reference_emit(sc)[None], 7)
    assert libc.rand() == first, "solve draws nothing"
    assert got.shape == (1, sc.num_texels, 4) and got.is_cuda
    _same(got[0], tex)


def test_reference_palette_on_tilted_emitters(torch_cuda, libc):
    """tests/emitter_scenes.py's tilted window and lamp, emitters and hit geometry of the cache: its reference
    palette equals fmgi.radiosity from the same libc position (which tests/test_offaxis_radiosity.py compares with
    the oracle and the reference)"""
    sc = emitter_scenes.get("tilted_emitters")
    CASES.seed(libc, "tilted_emitters")
    tex = fmgi.radiosity(sc)
    nxt = libc.rand()
    CASES.seed(libc, "tilted_emitters")
    rc = fmgi.RadCache(sc)
    try:
        assert libc.rand() == nxt
        assert (rc.info["windows"], rc.info["lights"]) == (1, 1)
        _same(rc.solve(fmgi.rad_reference_emit(sc)[None], 7)[0], tex)
    finally:
        rc.close()


@pytest.mark.parametrize("rounds", ALL_ROUNDS)
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 17])
def test_solve_equals_restatement_on_the_lit_box(torch_cuda, libc, k, rounds):
    want = CASES.restated(libc, "box_lit", ALL_K, ALL_ROUNDS)[rounds]
    rc, _ = _cache(libc, "box_lit")
    got = rc.solve(CASES.palettes("box_lit", ALL_K)[:k], rounds)
    assert not _bits(got)[..., 3].any()
    _same(got, want[:k])


@pytest.mark.parametrize("k", [3, 9])
def test_solve_equals_restatement_on_the_open_scene(torch_cuda, libc, k):
    want = CASES.restated(libc, "open_tilted", 9, (7,))[7]
    rc, _ = _cache(libc, "open_tilted")
    assert rc.info["jobs"] % 64 != 0 and rc.info["jobs"] % 8 != 0
    _same(rc.solve(CASES.palettes("open_tilted", 9)[:k], 7), want[:k])


def test_sets_are_independent_and_scale_exactly(torch_cuda, libc):
    rc, _ = _cache(libc, "box_lit")
    pal = CASES.palettes("box_lit", 9)
    nine = rc.solve(pal, 7).cpu().numpy()
    for i in range(9):
        _same(rc.solve(pal[i:i + 1], 7)[0], nine[i])
    assert (pal[1] == 2 * pal[0]).all()
    _same(nine[1], nine[0] * f32(2))
    assert not nine[2].any() and nine[3].any()  # all zeros in, all zeros out; the window alone lights the box


def test_scenes_without_emitters_and_without_walls(torch_cuda, libc):
    sc = scene.box_scene(8, tile_size=1.0)
    dark = scene.Scene("dark", sc.walls, sc.windows[:0], sc.lights[:0], sc.num_texels)
    libc.srand(1)
    rc = fmgi.RadCache(dark)
    got = rc.solve(np.zeros((3, 0, 3), f32), 7)
    assert got.shape == (3, dark.num_texels, 4) and not _bits(got).any()
    rc.close()
    empty = scene.Scene("empty", sc.walls[:0], sc.windows, sc.lights, 0)
    libc.srand(1)
    first = libc.rand()
    libc.srand(1)
    rc = fmgi.RadCache(empty)
    assert libc.rand() == first and rc.info["jobs"] == 0 and rc.sids().shape == (0, 10000)
    assert rc.solve(fmgi.rad_reference_emit(empty)[None], 7).shape == (1, 0, 4)
    rc.close()


def test_two_solves_back_to_back_on_one_stream(torch_cuda, libc):
    """the second call reuses the first one's scratch; its stream waits, the host does not"""
    want = CASES.restated(libc, "box_lit", ALL_K, ALL_ROUNDS)
    rc, _ = _cache(libc, "box_lit")
    pal = CASES.palettes("box_lit", ALL_K)
    s = torch_cuda.cuda.Stream()
    a = rc.solve(pal[:3], 7, stream=s)
    b = rc.solve(pal[3:5], 8, stream=s)
    c = rc.solve(pal[5:6], 1, stream=s.cuda_stream)
    s.synchronize()
    _same(a, want[7][:3])
    _same(b, want[8][3:5])
    _same(c, want[1][5:6])


def test_solve_feeds_the_view_path(torch_cuda, libc):
    sc = CASES.get_scene("box_lit")
    rc, _ = _cache(libc, "box_lit")
    tex = rc.solve(CASES.palettes("box_lit", 2), 7)
    vc = fmgi.ViewCache(sc, fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), pixel=0.02), 16, 12)
    n = 3 * vc.info()["tiles"]
    tiles = torch_cuda.zeros((2, n), dtype=torch_cuda.uint8, device=tex.device)
    vc.tiles([tex[k].data_ptr() for k in range(2)], 0, [tiles[k].data_ptr() for k in range(2)], tint_extra=1)
    torch_cuda.cuda.synchronize()
    host = tex.cpu().numpy()
    for k in range(2):
        assert np.array_equal(tiles[k].cpu().numpy(), fmgi.output_tiles(sc, host[k], 0, 1)[1])
    vc.close()


def test_argument_errors_with_a_handle(torch_cuda, libc):
    """what needs a handle to be reached: a NULL set, and an emit value that is NaN, negative or infinite"""
    lib = _lib.load()
    rc, _ = _cache(libc, "box_lit")
    pal = CASES.palettes("box_lit", 1).copy()
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        p = pal.copy()
        p[0, 1, 2] = bad
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\).*fmgi_rad_cache_solve: an emit value"):
            rc.solve(p, 7)
    for rounds in (0, 65):
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\).*iterations"):
            rc.solve(pal, rounds)
    with pytest.raises(fmgi.FmgiError, match="shape"):
        rc.solve(pal[:, :1], 7)
    null = (C.c_void_p * 1)(None)
    assert lib.fmgi_rad_cache_solve(rc.h, pal.ctypes.data_as(C.c_void_p), 1, 7, null, None) == -3
    assert lib.fmgi_rad_cache_solve(rc.h, None, 1, 7, null, None) == -3
    _same(rc.solve(pal, 7), CASES.restated(libc, "box_lit", ALL_K, ALL_ROUNDS)[7][:1])  # the handle is still good


def test_the_tool_end_to_end(torch_cuda, libc, tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight_radiosity as tool
    finally:
        sys.path.pop(0)
    scen = [{"name": "day", "windows": [30, 30, 30], "lights": [28, 28, 32]}, {"name": "lamp", "lights": [[3, 2, 1]]},
            {"name": "dusk", "windows": [0.5, 0.25, 2]}]
    f = tmp_path / "s.json"
    f.write_text(json.dumps(scen))
    rc, _ = _cache(libc, "box_lit")
    names, emit = tool.scenario_emit(scen, 1, 1)
    want = rc.solve(emit, 7).cpu().numpy()
    CASES.seed(libc, "box_lit")
    W, H, view = 32, 24, {"pos": (5, 4, 1.3), "dir": (1, 0.5, -0.1), "pixel": 0.03}
    tool.main(["box200", "--tile-size", "2", "--with-light", "--scenarios", str(f), "-o", str(tmp_path / "out"), "--view",
               "--width", str(W), "--height", str(H), "--samples", "2", "--pixel", str(view["pixel"]),
               "--pos", *map(str, view["pos"]), "--dir", *map(str, view["dir"]), "--background", "7", "8", "9"])
    sc = CASES.get_scene("box_lit")
    for k, name in enumerate(names):
        tex = np.load(tmp_path / "out" / name / "texels.npy")
        _same(tex, want[k])
        tiles = fmgi.output_tiles(sc, want[k], 0, 1)[1]
        assert np.array_equal(np.load(tmp_path / "out" / name / "tiles.npy"), tiles)
        # view.ppm: the picture the host path makes of the downloaded texels
        host = fmgi.shade_views(sc, fmgi.camera(**view), W, H, tiles, (7, 8, 9), samples=2, filter="bilinear")["rgb"][0]
        ppm = (tmp_path / "out" / name / "view.ppm").read_bytes()
        head = b"P6\n%d %d\n255\n" % (W, H)
        assert ppm.startswith(head) and ppm[len(head):] == host.tobytes()
    _same(want[0], CASES.oracle(libc, "box_lit")[1])
