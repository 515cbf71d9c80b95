"""The glossy floor of the views on the GPU (fmgi_*_gloss).

The numpy restatement (view_gloss_restate.py; its own conditions are checked in test_view_gloss_host.py) is the
oracle and every comparison is equality:

  rgb, coverage, tests and the mirror counts == the restatement: three cameras x nine cases x four glosses x both
  filters x 1, 2, 3 samples, and 8 samples once
  gloss 0 through the new call == fmgi_shade_views_proj: bytes and tests
  image-size edges, a batch with an empty-list camera, windowed launches, NULL outputs, no cameras
  ViewCache(mirror=True).tiles + .shade(gloss=g) == output_tiles + shade_views(gloss=g), 1, 3 and 9 lightmaps, three
  glosses from one trace; gloss > 0 on a view without mirror records is FMGI_ERR_STATE
  tools/render_view.py --gloss and tools/relight.py --view --gloss write the API's bytes
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
import view_gloss_restate as G
import view_proj_restate as P
from conftest import GOLDEN, REPO
from fmgi import _lib

pytestmark = pytest.mark.gpu

f32 = np.float32
BG = G.BG


def _filter(bilinear):
    return "bilinear" if bilinear else "nearest"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _assert_equal(got, k, exp):
    bad = (got["rgb"][k].astype(np.int64) != exp["rgb"]).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} pixels differ, the first at {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(got["coverage"][k].astype(np.int64), exp["coverage"])


def _assert_stats(exp, rays):
    st, gs = fmgi.view_stats(), fmgi.view_gloss_stats()
    assert st["tests"] == exp["tests"] and st["rays"] == rays, "rays stay the primary rays, tests count both walks"
    assert gs == {k: exp[k] for k in ("mirror_rays", "mirror_hits", "mirror_tests")}


def _gpu(name, S, bilinear, gloss, width=None, height=None):
    sc, cam, proj, w, h, tiles = G.case(name)
    if width:
        w, h = width, height
    return fmgi.shade_views(sc, cam, w, h, tiles, BG, samples=S, filter=_filter(bilinear), projection=proj, gloss=gloss)


# ---- pictures -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("name", G.CASES)
def test_gpu_equals_restatement(torch_cuda, name, S):
    _, _, _, w, h, _ = G.case(name)
    for bilinear in (False, True):
        for gloss in G.GLOSSES:  # 0.3: 1 - gloss is inexact
            exp = G.shade(name, S, bilinear, gloss)
            got = _gpu(name, S, bilinear, gloss)
            assert set(got) == {"rgb", "coverage"}
            _assert_equal(got, 0, exp)
            _assert_stats(exp, w * h * S * S)
            assert fmgi.view_stats()["cameras"] == 1 and exp["mirror_rays"] > 0


def test_gpu_eight_samples(torch_cuda):
    w, h = V.SIZES["box8_C"]
    for bilinear, gloss in ((True, 0.3), (False, 1.0)):
        exp = G.shade("box8_C", 8, bilinear, gloss)
        _assert_equal(_gpu("box8_C", 8, bilinear, gloss), 0, exp)
        _assert_stats(exp, w * h * 64)


@pytest.mark.parametrize("name", ["box8_C", "example_tool", "example_ortho", "open_tilted_equirect"])
def test_gloss_zero_is_the_call_without_it(torch_cuda, name):
    """gloss == 0 through fmgi_shade_views_gloss == fmgi_shade_views_proj: bytes, tests, and no mirror ray"""
    lib = _lib.load()
    sc, cam, proj, w, h, tiles = G.case(name)
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    cams, bg, code = np.atleast_1d(cam), np.array(BG, np.uint8), fmgi.PROJECTIONS[proj]
    old = fmgi.shade_views(sc, cam, w, h, tiles, BG, samples=3, filter="bilinear", projection=proj)
    st = fmgi.view_stats()
    _gpu(name, 3, True, 0.5)
    assert fmgi.view_gloss_stats()["mirror_rays"] > 0
    for gloss in (0.0, -0.0):
        rgb, cov = np.zeros((1, h, w, 3), np.uint8), np.zeros((1, h, w), np.uint8)
        assert lib.fmgi_shade_views_gloss(C.byref(g), _p(cams), 1, w, h, code, _p(tiles), _p(bg), 3, 1, gloss, _p(rgb),
                                          _p(cov)) == 0
        st2 = fmgi.view_stats()
        assert np.array_equal(rgb, old["rgb"]) and np.array_equal(cov, old["coverage"])
        assert all(st2[k] == st[k] for k in ("cameras", "rays", "tests", "candidates"))
        assert fmgi.view_gloss_stats() == {"mirror_rays": 0, "mirror_hits": 0, "mirror_tests": 0}
    # any other view call zeroes the mirror counts as well
    _gpu(name, 1, False, 0.5)
    assert fmgi.view_gloss_stats()["mirror_rays"] > 0
    fmgi.render_views(sc, V._cam("box8_C"), 8, 8)
    assert fmgi.view_gloss_stats() == {"mirror_rays": 0, "mirror_hits": 0, "mirror_tests": 0}
    del keep


@pytest.mark.parametrize("width,height", [(1, 1), (1, 130), (130, 1)])
@pytest.mark.parametrize("name", ["box8_C", "box8_ortho", "box8_equirect"])
def test_gpu_image_size_edges(torch_cuda, name, width, height):
    exp = G.shade(name, 3, True, 0.3, width, height)
    got = _gpu(name, 3, True, 0.3, width, height)
    _assert_equal(got, 0, exp)
    _assert_stats(exp, width * height * 9)


@pytest.mark.parametrize("proj", P.PROJECTIONS)
def test_gpu_batch_of_cameras(torch_cuda, proj):
    """four cameras on the floor scene in one call == one call per camera == the restatement. The camera below the
    floor has an empty primary list: its mirror list holds every wall, but without a primary hit it casts no mirror
    ray"""
    sc, (W, H) = P.scene("floor"), P.BATCH_SIZE
    tiles = P.tiles("floor")
    batch = fmgi.shade_views(sc, P.BATCH_CAMS, W, H, tiles, BG, samples=3, filter="bilinear", projection=proj, gloss=0.75)
    st, gs = fmgi.view_stats(), fmgi.view_gloss_stats()
    total = {k: 0 for k in ("tests", "mirror_rays", "mirror_hits", "mirror_tests")}
    for k, cam in enumerate(P.BATCH_CAMS):
        exp = G.shade_camera(sc, cam, proj, W, H, tiles, BG, 3, True, 0.75)
        one = fmgi.shade_views(sc, cam, W, H, tiles, BG, samples=3, filter="bilinear", projection=proj, gloss=0.75)
        _assert_equal(one, 0, exp)
        _assert_equal(batch, k, exp)
        _assert_stats(exp, W * H * 9)
        if k == 1:
            assert exp["mirror_rays"] == 0 and exp["tests"] == 0 and np.all(batch["coverage"][1] == 0)
            assert np.all(batch["rgb"][1] == BG)
        for key in total:
            total[key] += exp[key]
    assert total["mirror_rays"] > 0
    assert (st["cameras"], st["rays"], st["tests"]) == (4, 4 * W * H * 9, total["tests"])
    assert gs == {k: total[k] for k in gs}


def _window_case(proj):
    if proj == "pinhole":
        return V._scene("box8_C"), np.array([V._cam("box8_C"), V._cam("box8_A")], fmgi.CAMERA_DTYPE), V._tiles("box8_C")
    return P.case(f"box8_{proj}")[0], P.window_cams(proj), P.tiles("box8")


@pytest.mark.parametrize("proj", ("pinhole",) + tuple(P.PROJECTIONS))
def test_gpu_windowed_launches(torch_cuda, monkeypatch, proj):
    """a ray budget far below one image (FMGI_VIEW_RAYS_PER_LAUNCH, counted in primary rays) splits the call into
    windows of pixels, and a batch into single cameras: the same bytes and counts, for the traced view as well"""
    sc, cams, tiles = _window_case(proj)
    W, H = P.WINDOW_SIZE
    whole = fmgi.shade_views(sc, cams, W, H, tiles, BG, samples=2, filter="bilinear", projection=proj, gloss=0.3)
    st, gs = fmgi.view_stats(), fmgi.view_gloss_stats()
    monkeypatch.setenv("FMGI_VIEW_RAYS_PER_LAUNCH", "2048")  # 16 x 32 pixel windows at 2 x 2 samples
    parts = fmgi.shade_views(sc, cams, W, H, tiles, BG, samples=2, filter="bilinear", projection=proj, gloss=0.3)
    assert np.array_equal(parts["rgb"], whole["rgb"]) and np.array_equal(parts["coverage"], whole["coverage"])
    st2 = fmgi.view_stats()
    assert all(st2[k] == st[k] for k in ("cameras", "rays", "tests", "candidates")) and fmgi.view_gloss_stats() == gs
    tests = 0
    for k in range(2):
        exp = G.shade_camera(sc, cams[k], proj, W, H, tiles, BG, 2, True, 0.3)
        _assert_equal(parts, k, exp)
        tests += exp["tests"]
    assert st["tests"] == tests and gs["mirror_rays"] > 0
    vc = fmgi.ViewCache(sc, cams, W, H, 2, "bilinear", projection=proj, mirror=True)
    assert vc.info()["tests"] == tests and vc.info()["hits"] == int(whole["coverage"].astype(np.int64).sum())
    assert fmgi.view_gloss_stats() == gs
    i = vc.info()
    shape = (i["cameras"], i["height"], i["width"])
    rgb, cov = VC.Out(torch_cuda, int(np.prod(shape)) * 3), VC.Out(torch_cuda, int(np.prod(shape)))
    torch_cuda.cuda.synchronize()
    vc.shade([VC._upload(torch_cuda, tiles).data_ptr()], [rgb.ptr], BG, cov.ptr, gloss=0.3)
    torch_cuda.cuda.synchronize()
    assert np.array_equal(rgb.get(shape + (3,)), whole["rgb"]) and np.array_equal(cov.get(shape), whole["coverage"])
    vc.close()


@pytest.mark.parametrize("name", ["box8_C", "open_tilted_ortho", "open_tilted_equirect"])
def test_gpu_no_cameras_and_null_outputs(torch_cuda, name):
    lib = _lib.load()
    sc, cam, proj, w, h, tiles = G.case(name)
    code = fmgi.PROJECTIONS[proj]
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    bg = np.array(BG, np.uint8)
    cams = np.atleast_1d(cam)

    def call(cams, n, tiles, rgb, cov):
        return lib.fmgi_shade_views_gloss(C.byref(g), _p(cams), n, w, h, code, _p(tiles), _p(bg), 3, 1, 0.75, _p(rgb),
                                          _p(cov))

    rgb, cov = np.full((1, h, w, 3), 0xA5, np.uint8), np.full((1, h, w), 0x5A, np.uint8)
    assert call(None, 0, tiles, rgb, cov) == 0
    assert np.all(rgb == 0xA5) and np.all(cov == 0x5A)
    st = fmgi.view_stats()
    assert st["cameras"] == 0 and st["rays"] == 0 and st["tests"] == 0 and fmgi.view_gloss_stats()["mirror_rays"] == 0
    empty = fmgi.shade_views(sc, np.zeros(0, fmgi.CAMERA_DTYPE), w, h, tiles, samples=2, projection=proj, gloss=0.75)
    assert empty["rgb"].shape == (0, h, w, 3) and empty["coverage"].shape == (0, h, w)
    exp = G.shade(name, 3, True, 0.75)
    assert call(cams, 1, tiles, rgb, None) == 0
    _assert_stats(exp, w * h * 9)
    assert np.array_equal(rgb[0].astype(np.int64), exp["rgb"]) and np.all(cov == 0x5A)
    rgb[...] = 0xA5
    assert call(cams, 1, None, None, cov) == 0  # coverage needs no tiles; both walks run and are counted all the same
    assert np.array_equal(cov[0].astype(np.int64), exp["coverage"]) and np.all(rgb == 0xA5)
    _assert_stats(exp, w * h * 9)
    assert call(cams, 1, tiles, None, None) == 0
    _assert_stats(exp, w * h * 9)
    only_cov = fmgi.shade_views(sc, cams, w, h, samples=3, filter="bilinear", projection=proj, gloss=0.75)
    assert set(only_cov) == {"coverage"} and np.array_equal(only_cov["coverage"], cov)
    del keep


# ---- the traced view ------------------------------------------------------------------------------------------

SETS = 9  # more than one pass of fmgi.VIEW_CACHE_MAX_SETS
CACHE_GLOSSES = (0.0, 0.3, 0.75)


@pytest.mark.parametrize("name,bilinear,S", [("example_tool", True, 2), ("example_tool", False, 3),
                                             ("open_tilted_equirect", True, 3), ("open_tilted_equirect", False, 2),
                                             ("open_tilted_ortho", True, 2), ("open_tilted_ortho", False, 3)])
def test_view_cache_equals_the_host_path(torch_cuda, name, bilinear, S):
    """ViewCache(mirror=True).tiles + .shade(gloss=g) == output_tiles + shade_views(gloss=g) for 1, 3 and 9 random
    device lightmaps (nine take two passes) and three glosses, all from one trace; info's tests are both walks',
    its hits the primary hits, its bytes both planes'"""
    torch = torch_cuda
    sc, cam, proj, w, h, _ = G.case(name)
    spa = 1000  # VC._texels' values spread over the bytes at this normalisation
    vc = fmgi.ViewCache(sc, cam, w, h, S, _filter(bilinear), projection=proj, mirror=True)
    gs = fmgi.view_gloss_stats()
    info = vc.info()
    exp = G.shade(name, S, bilinear, 0.75)
    assert vc.has_mirror and vc.projection == proj and info["rays"] == w * h * S * S
    assert info["bytes"] == 2 * fmgi.view_cache_bytes(1, w, h, S, _filter(bilinear))
    assert info["tests"] == exp["tests"] and gs == {k: exp[k] for k in gs} and gs["mirror_rays"] > 0
    tex = [VC._texels(sc, k) for k in range(SETS)]
    old = {}
    for k in range(SETS):
        _, t = fmgi.output_tiles(sc, tex[k], spa)
        for g in CACHE_GLOSSES:
            old[k, g] = fmgi.shade_views(sc, cam, w, h, t, BG, samples=S, filter=_filter(bilinear), projection=proj, gloss=g)
    assert info["tests"] == fmgi.view_stats()["tests"], "the last host call had gloss > 0"
    assert info["hits"] == int(old[0, 0.0]["coverage"].astype(np.int64).sum()) > 0
    assert not np.array_equal(old[0, 0.0]["rgb"], old[0, 0.75]["rgb"])
    dev = [VC._upload(torch, t) for t in tex]
    for K in (1, 3, SETS):
        for g in CACHE_GLOSSES:
            tiles = [VC.Out(torch, 3 * info["tiles"]) for _ in range(K)]
            rgb = [VC.Out(torch, w * h * 3) for _ in range(K)]
            cov = VC.Out(torch, w * h)
            torch.cuda.synchronize()
            s = torch.cuda.Stream(device="cuda:0")
            # two calls on one stream: the second reads what the first wrote, with no host synchronise between them
            vc.tiles([d.data_ptr() for d in dev[:K]], spa, [o.ptr for o in tiles], stream=s.cuda_stream)
            vc.shade([o.ptr for o in tiles], [o.ptr for o in rgb], BG, cov.ptr, stream=s.cuda_stream, gloss=g)
            s.synchronize()
            assert np.array_equal(cov.get((1, h, w)), old[0, g]["coverage"])
            for k in range(K):
                got = rgb[k].get((1, h, w, 3))
                bad = (got != old[k, g]["rgb"]).any(axis=-1)
                assert not bad.any(), f"K {K} gloss {g} set {k}: {int(bad.sum())} pixels differ, the first at {tuple(np.argwhere(bad)[0])}"
            assert len({rgb[k].get().tobytes() for k in range(K)}) == K
    vc.close()


def test_view_cache_without_mirror_records(torch_cuda):
    """a plain view takes gloss 0 and refuses gloss > 0 with FMGI_ERR_STATE, before any launch; the mirror view's plain
    shade is the plain view's"""
    name = "example_tool"
    sc, cam, proj, w, h, tiles = G.case(name)
    plain, mirror = fmgi.ViewCache(sc, cam, w, h, 2, "bilinear"), fmgi.ViewCache(sc, cam, w, h, 2, "bilinear", mirror=True)
    assert not plain.has_mirror and mirror.has_mirror
    assert plain.info()["bytes"] * 2 == mirror.info()["bytes"] and plain.info()["hits"] == mirror.info()["hits"]
    assert plain.info()["tests"] < mirror.info()["tests"]
    buf = VC._upload(torch_cuda, tiles)
    lib = _lib.load()
    out = VC.Out(torch_cuda, w * h * 3)
    torch_cuda.cuda.synchronize()
    tp, rp, bg = (C.c_void_p * 1)(buf.data_ptr()), (C.c_void_p * 1)(out.ptr), np.array(BG, np.uint8)
    assert lib.fmgi_view_cache_shade_gloss(plain.h, tp, 1, _p(bg), 0.5, rp, None, None) == -4
    assert "mirror records" in _lib.last_error()
    with pytest.raises(fmgi.FmgiError, match="mirror records"):
        plain.shade([buf.data_ptr()], [out.ptr], BG, gloss=0.5)
    for bad in (np.nan, 1.5, -0.25):
        assert lib.fmgi_view_cache_shade_gloss(mirror.h, tp, 1, _p(bg), bad, rp, None, None) == -3
        assert lib.fmgi_view_cache_shade_gloss(plain.h, tp, 1, _p(bg), bad, rp, None, None) == -3, "the argument first"
    torch_cuda.cuda.synchronize()
    assert np.all(out.get() == 0xA5), "nothing was launched"
    matt = fmgi.shade_views(sc, cam, w, h, tiles, BG, samples=2, filter="bilinear")["rgb"]
    for vc, call in ((plain, "plain"), (mirror, "plain"), (plain, "zero"), (mirror, "zero")):
        rgb = VC.Out(torch_cuda, w * h * 3)
        torch_cuda.cuda.synchronize()
        if call == "plain":
            vc.shade([buf.data_ptr()], [rgb.ptr], BG)
        else:
            assert lib.fmgi_view_cache_shade_gloss(vc.h, tp, 1, _p(bg), 0.0, (C.c_void_p * 1)(rgb.ptr), None, None) == 0
        torch_cuda.cuda.synchronize()
        assert np.array_equal(rgb.get((1, h, w, 3)), matt)
    plain.close()
    mirror.close()


# ---- tools ----------------------------------------------------------------------------------------------------

def test_render_view_tool_gloss(torch_cuda, tmp_path):
    """tools/render_view.py --gloss 0.75 --samples 2 --filter bilinear writes shade_views(gloss=0.75)'s bytes"""
    sc = T._scene("box8")
    rng = np.random.default_rng(5)
    tex = (10.0 ** rng.uniform(-3, 1, (sc.num_texels, 4))).astype(f32)
    np.save(tmp_path / "texels.npy", tex)
    ppm = tmp_path / "glossy.ppm"
    cam = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.4), up=(0, 0, 1), pixel=0.05)
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "render_view.py"), "box8", "--tile-size", "1",
                        "--texels", str(tmp_path / "texels.npy"), "--spa", "1000", "--pos", *flat(cam["pos"]),
                        "--dir", *flat(cam["dir"]), "--up", *flat(cam["up"]), "--pixel", "0.05", "--width", "32",
                        "--height", "24", "--background", "1", "2", "3", "--samples", "2", "--filter", "bilinear",
                        "--gloss", "0.75", "-o", str(ppm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = ppm.read_bytes()
    head = b"P6\n32 24\n255\n"
    assert blob.startswith(head) and len(blob) == len(head) + 32 * 24 * 3
    _, tiles = fmgi.output_tiles(sc, tex, 1000, 0)
    got = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 24, tiles, (1, 2, 3), samples=2, filter="bilinear", gloss=0.75)
    gs = fmgi.view_gloss_stats()
    assert f"{gs['mirror_rays']} mirror rays" in r.stdout and 0 < gs["mirror_rays"] < 32 * 24 * 4
    matt = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 24, tiles, (1, 2, 3), samples=2, filter="bilinear")
    assert blob[len(head):] == got["rgb"][0].tobytes() and not np.array_equal(got["rgb"], matt["rgb"])


def test_relight_view_tool_gloss(tmp_path):
    """tools/relight.py --view --gloss 0.75 on the lit box: each view.ppm holds shade_views(gloss=0.75) of the tiles the
    tool wrote"""
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": {"scale": 0.5}}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    cam = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.4), up=(0, 0, 1), pixel=0.05)
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4",
                        "--with-light", "--scenarios", str(tmp_path / "scenarios.json"), "--spa", str(R.SPA),
                        "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy"), "--sparse-from-codes", "--view",
                        "--gloss", "0.75", "--pos", *flat(cam["pos"]), "--dir", *flat(cam["dir"]), "--up",
                        *flat(cam["up"]), "--pixel", "0.05", "--width", "32", "--height", "24", "--samples", "3",
                        "--background", "7", "8", "9", "-o", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sc = R.lit_box()[0]
    head = b"P6\n32 24\n255\n"
    blobs = []
    for name in ("day", "evening"):
        tiles = np.load(tmp_path / "out" / name / "tiles.npy")
        exp = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 24, tiles, BG, samples=3, filter="bilinear", gloss=0.75)
        matt = fmgi.shade_views(sc, fmgi.camera(**cam), 32, 24, tiles, BG, samples=3, filter="bilinear")
        blob = (tmp_path / "out" / name / "view.ppm").read_bytes()
        assert blob.startswith(head) and blob[len(head):] == exp["rgb"][0].tobytes(), name
        assert not np.array_equal(exp["rgb"], matt["rgb"])
        blobs.append(blob)
    assert blobs[0] != blobs[1]
