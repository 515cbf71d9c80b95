"""Orthographic and equirectangular cameras on the GPU (fmgi_*_proj).

The numpy restatement (view_proj_restate.py; its own conditions are checked in test_view_proj_host.py) is the
oracle and every comparison is equality:

  FMGI_PROJ_PINHOLE through the three *_proj calls == the calls without the suffix
  candidate lists (indices, key bits) == the restatement's, on closed, open and tilted scenes, at the
  power-of-two edge of the sort, and for a camera whose list is empty
  rgb, coverage and tests == the restatement, both projections x both filters x 1, 2, 3, 8 samples
  image-size edges, a batch with an empty-list camera, windowed launches, NULL outputs, no cameras
  ViewCache(projection=...).tiles + .shade == output_tiles + shade_views(projection=...), 1, 3 and 9 lightmaps
  tools/render_view.py --projection and tools/relight.py --view --projection write the API's bytes
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
import recolour_events as R
import test_gpu_view_cache as VC
import test_view as T
import test_view_shade as V
import view_proj_restate as P
from conftest import GOLDEN, REPO
from fmgi import _lib

pytestmark = pytest.mark.gpu

f32 = np.float32
BG = P.BG


def _filter(bilinear):
    return "bilinear" if bilinear else "nearest"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _assert_equal(got, k, exp):
    bad = (got["rgb"][k].astype(np.int64) != exp["rgb"]).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} pixels differ, the first at {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(got["coverage"][k].astype(np.int64), exp["coverage"])


def _gpu(name, S, bilinear, width=None, height=None):
    sc, cam, proj, w, h = P.case(name)
    if width:
        w, h = width, height
    return fmgi.shade_views(sc, cam, w, h, P.tiles(name.rsplit("_", 1)[0]), BG, samples=S, filter=_filter(bilinear),
                            projection=proj)


# ---- FMGI_PROJ_PINHOLE is the existing call -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box8_A", "example_tool"])
def test_pinhole_through_the_proj_calls(torch_cuda, name):
    lib = _lib.load()
    sc, cam, (w, h) = V._scene(name), V._cam(name), V.SIZES[name]
    cams = np.atleast_1d(cam)
    tiles = V._tiles(name)
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    bg = np.array(BG, np.uint8)
    # candidates
    idx, md = fmgi.view_candidates(sc, cam)
    idx2, md2 = np.zeros(len(sc.walls), np.int32), np.zeros(len(sc.walls), f32)
    n = lib.fmgi_view_candidates_proj(C.byref(g), _p(cams), _lib.PROJ_PINHOLE, _p(idx2), _p(md2), len(sc.walls))
    assert n == len(idx) > 0 and np.array_equal(idx2[:n], idx) and np.array_equal(md2[:n].view(np.uint32), md.view(np.uint32))
    # shade
    old = fmgi.shade_views(sc, cam, w, h, tiles, BG, samples=3, filter="bilinear")
    st = fmgi.view_stats()
    rgb, cov = np.zeros((1, h, w, 3), np.uint8), np.zeros((1, h, w), np.uint8)
    assert lib.fmgi_shade_views_proj(C.byref(g), _p(cams), 1, w, h, _lib.PROJ_PINHOLE, _p(tiles), _p(bg), 3, 1, _p(rgb),
                                     _p(cov)) == 0
    st2 = fmgi.view_stats()
    assert np.array_equal(rgb, old["rgb"]) and np.array_equal(cov, old["coverage"])
    assert all(st2[k] == st[k] for k in ("cameras", "rays", "tests", "candidates"))
    # the traced view
    h_ = C.c_void_p()
    assert lib.fmgi_view_cache_create_proj(C.byref(g), _p(cams), 1, w, h, _lib.PROJ_PINHOLE, 3, 1, C.byref(h_)) == 0
    vc = fmgi.ViewCache.__new__(fmgi.ViewCache)
    vc.lib, vc.h = lib, h_
    ref = fmgi.ViewCache(sc, cam, w, h, 3, "bilinear")
    assert vc.projection == ref.projection == "pinhole"
    a, b = vc.info(), ref.info()
    assert all(a[k] == b[k] for k in a if not k.endswith("_ms")) and a["tests"] == st["tests"]
    buf = VC._upload(torch_cuda, tiles)
    pics = []
    for cache in (vc, ref):
        out, c, shape = VC._shade(torch_cuda, cache, [buf])
        torch_cuda.cuda.synchronize()
        pics.append((out[0].get(shape + (3,)), c.get(shape)))
        cache.close()
    assert np.array_equal(pics[0][0], pics[1][0]) and np.array_equal(pics[0][0], old["rgb"])
    assert np.array_equal(pics[0][1], pics[1][1]) and np.array_equal(pics[0][1], old["coverage"])
    del keep


# ---- candidate lists ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", P.LIST_CASES)
def test_candidate_lists_equal_the_restatement(torch_cuda, name):
    sc, cam, proj, _, _ = P.case(name)
    exp_idx, exp_key = P.candidates(sc, cam, proj)
    idx, key = fmgi.view_candidates(sc, cam, projection=proj)
    n = min(len(idx), len(exp_idx))
    bad = np.flatnonzero((idx[:n] != exp_idx[:n]) | (key[:n].view(np.uint32) != exp_key[:n].view(np.uint32)))
    assert len(bad) == 0, f"candidate lists differ from entry {bad[0]}"
    assert len(idx) == len(exp_idx) > 0


@pytest.mark.parametrize("proj", P.PROJECTIONS)
def test_an_empty_candidate_list(torch_cuda, proj):
    sc = P.scene("floor")
    idx, key = fmgi.view_candidates(sc, P.EMPTY_CAM, projection=proj)
    assert len(idx) == 0 and len(P.candidates(sc, P.EMPTY_CAM, proj)[0]) == 0
    got = fmgi.shade_views(sc, P.EMPTY_CAM, 20, 9, P.tiles("floor"), BG, samples=2, filter="bilinear", projection=proj)
    assert np.all(got["coverage"] == 0) and np.all(got["rgb"] == np.array(BG, np.uint8))
    st = fmgi.view_stats()
    assert (st["tests"], st["candidates"], st["rays"]) == (0, 0, 20 * 9 * 4)


# ---- pictures -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("name", P.SHADE_CASES)
def test_gpu_equals_restatement(torch_cuda, name, S, bilinear):
    _, _, _, w, h = P.case(name)
    exp = P.restated(name, S, bilinear)
    got = _gpu(name, S, bilinear)
    assert set(got) == {"rgb", "coverage"}
    _assert_equal(got, 0, exp)
    st = fmgi.view_stats()
    assert st["tests"] == exp["tests"]
    assert st["rays"] == w * h * S * S and st["cameras"] == 1
    assert st["candidates"] == len(P.candidates(*P.case(name)[:3])[0])


@pytest.mark.parametrize("width,height", [(1, 1), (1, 130), (130, 1)])
@pytest.mark.parametrize("proj", P.PROJECTIONS)
def test_gpu_image_size_edges(torch_cuda, proj, width, height):
    name = f"box8_{proj}"
    exp = P.restated(name, 3, True, width, height)
    got = _gpu(name, 3, True, width, height)
    _assert_equal(got, 0, exp)
    assert fmgi.view_stats()["tests"] == exp["tests"] and fmgi.view_stats()["rays"] == width * height * 9


@pytest.mark.parametrize("proj", P.PROJECTIONS)
def test_gpu_batch_of_cameras(torch_cuda, proj):
    """four cameras on the floor scene in one call (the empty-list camera between the others) == one call per
    camera == the restatement"""
    sc, (W, H) = P.scene("floor"), P.BATCH_SIZE
    tiles = P.tiles("floor")
    batch = fmgi.shade_views(sc, P.BATCH_CAMS, W, H, tiles, BG, samples=3, filter="bilinear", projection=proj)
    st = fmgi.view_stats()
    tests = cands = 0
    for k, cam in enumerate(P.BATCH_CAMS):
        exp = P.shade(sc, cam, W, H, tiles, BG, 3, True, proj)
        one = fmgi.shade_views(sc, cam, W, H, tiles, BG, samples=3, filter="bilinear", projection=proj)
        _assert_equal(one, 0, exp)
        _assert_equal(batch, k, exp)
        assert fmgi.view_stats()["tests"] == exp["tests"]
        tests += exp["tests"]
        cands += len(P.candidates(sc, cam, proj)[0])
    assert batch["coverage"].shape == (4, H, W) and np.all(batch["coverage"][1] == 0) and np.all(batch["rgb"][1] == BG)
    assert all(batch["coverage"][k].any() for k in (0, 2, 3))
    assert (st["cameras"], st["rays"], st["tests"], st["candidates"]) == (4, 4 * W * H * 9, tests, cands)


@pytest.mark.parametrize("proj", P.PROJECTIONS)
def test_gpu_windowed_launches(torch_cuda, monkeypatch, proj):
    """a ray budget far below one image (FMGI_VIEW_RAYS_PER_LAUNCH) splits the call into windows of pixels, and a
    batch into single cameras: the same bytes and counts"""
    name = f"box8_{proj}"
    sc, cams, (W, H) = P.case(name)[0], P.window_cams(proj), P.WINDOW_SIZE
    whole = fmgi.shade_views(sc, cams, W, H, P.tiles("box8"), BG, samples=2, filter="bilinear", projection=proj)
    st = fmgi.view_stats()
    monkeypatch.setenv("FMGI_VIEW_RAYS_PER_LAUNCH", "2048")  # 16 x 32 pixel windows at 2 x 2 samples
    parts = fmgi.shade_views(sc, cams, W, H, P.tiles("box8"), BG, samples=2, filter="bilinear", projection=proj)
    assert np.array_equal(parts["rgb"], whole["rgb"]) and np.array_equal(parts["coverage"], whole["coverage"])
    st2 = fmgi.view_stats()
    assert all(st2[k] == st[k] for k in ("cameras", "rays", "tests", "candidates"))
    for k in range(2):
        _assert_equal(parts, k, P.shade(sc, cams[k], W, H, P.tiles("box8"), BG, 2, True, proj))
    assert not np.array_equal(parts["rgb"][0], parts["rgb"][1])
    # the traced view under the same budget
    vc = fmgi.ViewCache(sc, cams, W, H, 2, "bilinear", projection=proj)
    assert vc.info()["tests"] == st["tests"] and vc.info()["hits"] == int(whole["coverage"].astype(np.int64).sum())
    rgb, cov, shape = VC._shade(torch_cuda, vc, [VC._upload(torch_cuda, P.tiles("box8"))])
    torch_cuda.cuda.synchronize()
    assert np.array_equal(rgb[0].get(shape + (3,)), whole["rgb"]) and np.array_equal(cov.get(shape), whole["coverage"])
    vc.close()


@pytest.mark.parametrize("proj", P.PROJECTIONS)
def test_gpu_no_cameras_and_null_outputs(torch_cuda, proj):
    lib = _lib.load()
    name = f"open_tilted_{proj}"
    sc, cam, _, w, h = P.case(name)
    tiles, code = P.tiles("open_tilted"), fmgi.PROJECTIONS[proj]
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    bg = np.array(BG, np.uint8)
    cams = np.atleast_1d(cam)

    def call(cams, n, tiles, rgb, cov):
        return lib.fmgi_shade_views_proj(C.byref(g), _p(cams), n, w, h, code, _p(tiles), _p(bg), 3, 1, _p(rgb), _p(cov))

    rgb, cov = np.full((1, h, w, 3), 0xA5, np.uint8), np.full((1, h, w), 0x5A, np.uint8)
    assert call(None, 0, tiles, rgb, cov) == 0
    assert np.all(rgb == 0xA5) and np.all(cov == 0x5A)
    st = fmgi.view_stats()
    assert st["cameras"] == 0 and st["rays"] == 0 and st["tests"] == 0
    empty = fmgi.shade_views(sc, np.zeros(0, fmgi.CAMERA_DTYPE), w, h, tiles, samples=2, projection=proj)
    assert empty["rgb"].shape == (0, h, w, 3) and empty["coverage"].shape == (0, h, w)
    exp = P.restated(name, 3, True)
    assert call(cams, 1, tiles, rgb, None) == 0
    assert fmgi.view_stats()["tests"] == exp["tests"]
    assert np.array_equal(rgb[0].astype(np.int64), exp["rgb"]) and np.all(cov == 0x5A)
    rgb[...] = 0xA5
    assert call(cams, 1, None, None, cov) == 0  # coverage needs no tiles
    assert np.array_equal(cov[0].astype(np.int64), exp["coverage"]) and np.all(rgb == 0xA5)
    assert fmgi.view_stats()["tests"] == exp["tests"]
    assert call(cams, 1, tiles, None, None) == 0
    assert fmgi.view_stats()["tests"] == exp["tests"]
    only_cov = fmgi.shade_views(sc, cams, w, h, samples=3, filter="bilinear", projection=proj)
    assert set(only_cov) == {"coverage"} and np.array_equal(only_cov["coverage"], cov)
    del keep


# ---- the traced view ------------------------------------------------------------------------------------------

SETS = 9  # more than one pass of fmgi.VIEW_CACHE_MAX_SETS


@pytest.mark.parametrize("bilinear,S", [(True, 3), (False, 2)])
@pytest.mark.parametrize("name", ["example_ortho", "example_equirect", "open_tilted_ortho", "open_tilted_equirect"])
def test_view_cache_equals_the_host_path(torch_cuda, name, bilinear, S):
    """ViewCache.tiles + .shade == output_tiles + shade_views(projection=...) for 1, 3 and 9 random device lightmaps
    (nine take two passes); info's tests and hits are the shade call's"""
    torch = torch_cuda
    sc, cam, proj, w, h = P.case(name)
    spa = 1000  # VC._texels' values spread over the bytes at this normalisation
    vc = fmgi.ViewCache(sc, cam, w, h, S, _filter(bilinear), projection=proj)
    info = vc.info()
    assert vc.projection == proj and info["rays"] == w * h * S * S
    assert info["bytes"] == fmgi.view_cache_bytes(1, w, h, S, _filter(bilinear))
    tex = [VC._texels(sc, k) for k in range(SETS)]
    old = []
    for k in range(SETS):
        _, t = fmgi.output_tiles(sc, tex[k], spa)
        old.append(fmgi.shade_views(sc, cam, w, h, t, BG, samples=S, filter=_filter(bilinear), projection=proj))
    st = fmgi.view_stats()
    assert info["tests"] == st["tests"] == P.restated(name, S, bilinear)["tests"]
    assert info["hits"] == int(old[0]["coverage"].astype(np.int64).sum()) > 0
    dev = [VC._upload(torch, t) for t in tex]
    for K in (1, 3, SETS):
        tiles = [VC.Out(torch, 3 * info["tiles"]) for _ in range(K)]
        rgb = [VC.Out(torch, w * h * 3) for _ in range(K)]
        cov = VC.Out(torch, w * h)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device="cuda:0")
        # two calls on one stream: the second reads what the first wrote, with no host synchronise between them
        vc.tiles([d.data_ptr() for d in dev[:K]], spa, [o.ptr for o in tiles], stream=s.cuda_stream)
        vc.shade([o.ptr for o in tiles], [o.ptr for o in rgb], BG, cov.ptr, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(cov.get((1, h, w)), old[0]["coverage"])
        for k in range(K):
            got = rgb[k].get((1, h, w, 3))
            bad = (got != old[k]["rgb"]).any(axis=-1)
            assert not bad.any(), f"K {K} set {k}: {int(bad.sum())} pixels differ, the first at {tuple(np.argwhere(bad)[0])}"
        assert len({rgb[k].get().tobytes() for k in range(K)}) == K
    vc.close()


# ---- tools ----------------------------------------------------------------------------------------------------

def test_render_view_tool_equirect(torch_cuda, tmp_path):
    """tools/render_view.py --projection equirect --samples 3 --filter bilinear writes shade_views' bytes"""
    sc = T._scene("box8")
    rng = np.random.default_rng(5)
    tex = (10.0 ** rng.uniform(-3, 1, (sc.num_texels, 4))).astype(f32)
    np.save(tmp_path / "texels.npy", tex)
    ppm = tmp_path / "pano.ppm"
    cam = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1), pixel=0.1)
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "render_view.py"), "box8", "--tile-size", "1",
                        "--texels", str(tmp_path / "texels.npy"), "--spa", "1000", "--pos", *flat(cam["pos"]),
                        "--dir", *flat(cam["dir"]), "--up", *flat(cam["up"]), "--width", "32", "--height", "16",
                        "--background", "1", "2", "3", "--samples", "3", "--filter", "bilinear", "--projection",
                        "equirect", "-o", str(ppm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{32 * 16 * 9} of {32 * 16 * 9} rays" in r.stdout, "a closed box: every ray hits"
    blob = ppm.read_bytes()
    head = b"P6\n32 16\n255\n"
    assert blob.startswith(head) and len(blob) == len(head) + 32 * 16 * 3
    _, tiles = fmgi.output_tiles(sc, tex, 1000, 0)
    got = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 16, tiles, (1, 2, 3), samples=3, filter="bilinear",
                           projection="equirect")
    pin = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 16, tiles, (1, 2, 3), samples=3, filter="bilinear")
    assert blob[len(head):] == got["rgb"][0].tobytes() and not np.array_equal(got["rgb"], pin["rgb"])


def test_relight_view_tool_ortho(tmp_path):
    """tools/relight.py --view --projection ortho on the lit box: each view.ppm holds shade_views' plan of the tiles
    the tool wrote"""
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": {"scale": 0.5}}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    cam = dict(pos=(5, 4, 2.0), dir=(0, 0, -1), up=(0, 1, 0), pixel=0.4)  # below the ceiling: the plan with the walls' feet
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4",
                        "--with-light", "--scenarios", str(tmp_path / "scenarios.json"), "--spa", str(R.SPA),
                        "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy"), "--sparse-from-codes", "--view",
                        "--projection", "ortho", "--pos", *flat(cam["pos"]), "--dir", *flat(cam["dir"]), "--up",
                        *flat(cam["up"]), "--pixel", "0.4", "--width", "32", "--height", "24", "--samples", "3",
                        "--background", "7", "8", "9", "-o", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sc = R.lit_box()[0]
    head = b"P6\n32 24\n255\n"
    blobs = []
    for name in ("day", "evening"):
        tiles = np.load(tmp_path / "out" / name / "tiles.npy")
        exp = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 24, tiles, BG, samples=3, filter="bilinear", projection="ortho")
        blob = (tmp_path / "out" / name / "view.ppm").read_bytes()
        assert blob.startswith(head) and blob[len(head):] == exp["rgb"][0].tobytes(), name
        assert 0 < int((exp["coverage"] > 0).sum()) < 32 * 24
        blobs.append(blob)
    assert blobs[0] != blobs[1]
