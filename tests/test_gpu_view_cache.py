"""Traced views on the GPU (fmgi_view_cache_* / fmgi.ViewCache).

A view's rays are cast once and kept as per-sample records; every tile set is then shaded by a gather. The old host
path is the oracle, and every comparison is equality:

  ViewCache.shade == fmgi.shade_views and test_view_shade's numpy restatement, for 1, 3 and 9 tile sets (one pass,
  one pass, two passes), both filters, 1 to 8 samples; coverage, hits and tests
  image sizes off the 16-pixel workgroup, two cameras, a windowed trace, no coverage, two streams, guard bytes
  ViewCache.tiles == fmgi.output_tiles' bytes from device texels that stay as they are
  bake_sparse -> recolour_sparse -> finalize -> tiles -> shade == the host path on the downloaded texels
  tools/relight.py --view writes those bytes
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
import recolour_events as R
import test_view_shade as V
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

f32 = np.float32
BG = V.BG
GUARD = 64  # bytes of 0xA5 before and after every output buffer
SETS = 9    # tile sets of a case: more than one pass of fmgi.VIEW_CACHE_MAX_SETS


class Out:
    """a device byte buffer between two guards"""

    def __init__(self, torch, n):
        self.torch, self.n = torch, n
        self.t = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.t.data_ptr() + GUARD

    def get(self, shape=None):
        """the bytes (after the caller has synchronised); the guards must be untouched"""
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == 0xA5).all() and (a[GUARD + self.n:] == 0xA5).all(), "guard bytes were written"
        a = a[GUARD:GUARD + self.n]
        return a if shape is None else a.reshape(shape)


def _upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(None)
def _tile_set(name, k):
    """set 0 is test_view_shade's"""
    n = 3 * int(V._tile_counts(V._scene(name)).sum())
    return np.random.default_rng(5 + k).integers(0, 256, n, dtype=np.uint8)


@functools.lru_cache(None)
def _restated(name, k, S, bilinear, width, height):
    return V.shade(V._scene(name), V._cam(name), width, height, _tile_set(name, k), BG, S, bilinear)


def _filter(bilinear):
    return "bilinear" if bilinear else "nearest"


def _shade(torch, vc, tile_bufs, coverage=True, stream=0, background=BG):
    """ViewCache.shade of device tile buffers: (guarded rgb outputs, guarded coverage or None)"""
    i = vc.info()
    shape = (i["cameras"], i["height"], i["width"])
    rgb = [Out(torch, int(np.prod(shape)) * 3) for _ in tile_bufs]
    cov = Out(torch, int(np.prod(shape))) if coverage else None
    torch.cuda.current_stream().synchronize()  # the guards are filled before another stream writes between them
    vc.shade([t.data_ptr() for t in tile_bufs], [o.ptr for o in rgb], background, cov.ptr if cov else 0, stream)
    return rgb, cov, shape


def test_the_cases_hold_what_the_comparisons_need():
    """test_view_shade.test_input_conditions for the cases below: pixels on a silhouette, misses, clamped taps and
    bilinear != nearest, so a cache that kept no miss or no clamped tap cannot pass unnoticed"""
    for name in ("box8_C", "example_tool"):
        w, h = V.SIZES[name]
        cov = _restated(name, 0, 3, True, w, h)["coverage"]
        assert int(((cov > 0) & (cov < 9)).sum()) > 0, name + ": pixels on a wall's silhouette"
    w, h = V.SIZES["box8_C"]
    assert int((_restated("box8_C", 0, 3, True, w, h)["coverage"] == 0).sum()) > 0, "misses"
    for name in V.CASES:
        w, h = V.SIZES[name]
        near, lin = _restated(name, 0, 1, False, w, h), _restated(name, 0, 1, True, w, h)
        assert lin["clamped"] > 0, name + ": taps clamped at a wall's edge"
        hit = near["coverage"] > 0
        assert int((near["rgb"][hit] != lin["rgb"][hit]).any(axis=-1).sum()) > 0, name


@pytest.mark.parametrize("bilinear", [False, True])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("name", V.CASES)
def test_shade_equals_both_oracles(torch_cuda, name, S, bilinear):
    sc, cam, (w, h) = V._scene(name), V._cam(name), V.SIZES[name]
    vc = fmgi.ViewCache(sc, cam, w, h, S, _filter(bilinear))
    info = vc.info()
    assert info["bytes"] == fmgi.view_cache_bytes(1, w, h, S, _filter(bilinear)) == w * h * S * S * (16 if bilinear else 4)
    assert (info["cameras"], info["width"], info["height"], info["samples"], info["filter"]) == (1, w, h, S, int(bilinear))
    assert info["tiles"] * 3 == len(_tile_set(name, 0)) and info["rays"] == w * h * S * S
    assert info["num_texels"] == sc.num_texels
    old = [fmgi.shade_views(sc, cam, w, h, _tile_set(name, k), BG, samples=S, filter=_filter(bilinear))
           for k in range(SETS)]
    assert info["tests"] == fmgi.view_stats()["tests"]
    assert info["hits"] == int(old[0]["coverage"].astype(np.int64).sum())
    bufs = [_upload(torch_cuda, _tile_set(name, k)) for k in range(SETS)]
    for K in (1, 3, SETS):
        rgb, cov, shape = _shade(torch_cuda, vc, bufs[:K])
        torch_cuda.cuda.synchronize()
        c = cov.get(shape)
        assert np.array_equal(c, old[0]["coverage"])
        for k in range(K):
            got = rgb[k].get(shape + (3,))
            exp = _restated(name, k, S, bilinear, w, h)
            bad = (got != old[k]["rgb"]).any(axis=-1)
            assert not bad.any(), f"K {K} set {k}: {int(bad.sum())} pixels differ from shade_views, the first at {tuple(np.argwhere(bad)[0])}"
            assert np.array_equal(got[0].astype(np.int64), exp["rgb"]), (K, k)
            assert np.array_equal(c[0].astype(np.int64), exp["coverage"]) and info["tests"] == exp["tests"]
    vc.close()


@pytest.mark.parametrize("width,height", [(17, 1), (1, 17), (33, 18)])
def test_image_sizes_off_the_workgroup(torch_cuda, width, height):
    name = "box8_C"
    sc, cam = V._scene(name), V._cam(name)
    bufs = [_upload(torch_cuda, _tile_set(name, k)) for k in range(2)]
    for bilinear in (False, True):
        vc = fmgi.ViewCache(sc, cam, width, height, 3, _filter(bilinear))
        rgb, cov, shape = _shade(torch_cuda, vc, bufs)
        torch_cuda.cuda.synchronize()
        for k in range(2):
            old = fmgi.shade_views(sc, cam, width, height, _tile_set(name, k), BG, samples=3, filter=_filter(bilinear))
            exp = _restated(name, k, 3, bilinear, width, height)
            assert np.array_equal(rgb[k].get(shape + (3,)), old["rgb"])
            assert np.array_equal(old["rgb"][0].astype(np.int64), exp["rgb"])
            assert np.array_equal(cov.get(shape), old["coverage"])
        assert vc.info()["tests"] == fmgi.view_stats()["tests"]
        vc.close()


def _two_cameras():
    return np.array([V._cam("box8_A"), V._cam("box8_C")], fmgi.CAMERA_DTYPE)


def test_two_cameras_and_a_windowed_trace(torch_cuda, monkeypatch):
    sc, cams, (w, h) = V._scene("box8_C"), _two_cameras(), V.SIZES["box8_C"]
    tiles = _tile_set("box8_C", 0)
    old = fmgi.shade_views(sc, cams, w, h, tiles, BG, samples=3, filter="bilinear")
    tests = fmgi.view_stats()["tests"]
    buf = _upload(torch_cuda, tiles)
    got = []
    assert w * h * 9 > 4096  # one camera's 4320 rays are over the budget: four windows of 16 x 16 pixels each
    for budget in (None, "4096"):
        if budget:
            monkeypatch.setenv("FMGI_VIEW_RAYS_PER_LAUNCH", budget)
        vc = fmgi.ViewCache(sc, cams, w, h, 3, "bilinear")
        info = vc.info()
        assert (info["cameras"], info["rays"], info["tests"]) == (2, 2 * w * h * 9, tests)
        assert info["hits"] == int(old["coverage"].astype(np.int64).sum())
        rgb, cov, shape = _shade(torch_cuda, vc, [buf])
        torch_cuda.cuda.synchronize()
        assert shape == (2, h, w)
        got.append((rgb[0].get(shape + (3,)), cov.get(shape)))
        vc.close()
    for rgb, cov in got:
        assert np.array_equal(rgb, old["rgb"]) and np.array_equal(cov, old["coverage"])
    for k, name in enumerate(("box8_A", "box8_C")):  # both cameras look at the box8 scene
        exp = V.shade(sc, cams[k], w, h, tiles, BG, 3, True)
        assert np.array_equal(got[0][0][k].astype(np.int64), exp["rgb"]), name
    assert not np.array_equal(old["rgb"][0], old["rgb"][1])


def test_no_coverage_and_two_streams(torch_cuda):
    """coverage_dev = NULL; then one cache shaded twice with different sets on two streams, the second call
    reusing the packed-tile scratch of the first"""
    name = "example_tool"
    sc, cam, (w, h) = V._scene(name), V._cam(name), V.SIZES[name]
    vc = fmgi.ViewCache(sc, cam, w, h, 2, "bilinear")
    bufs = [_upload(torch_cuda, _tile_set(name, k)) for k in range(4)]
    torch_cuda.cuda.synchronize()
    rgb, cov, shape = _shade(torch_cuda, vc, bufs[:1], coverage=False)
    torch_cuda.cuda.synchronize()
    assert cov is None
    assert np.array_equal(rgb[0].get(shape + (3,))[0].astype(np.int64), _restated(name, 0, 2, True, w, h)["rgb"])
    s1, s2 = torch_cuda.cuda.Stream(device="cuda:0"), torch_cuda.cuda.Stream(device="cuda:0")
    a, _, _ = _shade(torch_cuda, vc, bufs[:2], coverage=False, stream=s1.cuda_stream)
    b, cov_b, _ = _shade(torch_cuda, vc, bufs[2:], stream=s2.cuda_stream, background=(200, 100, 50))
    s1.synchronize()
    s2.synchronize()
    for k, out in enumerate(a + b):
        bg = BG if k < 2 else (200, 100, 50)
        old = fmgi.shade_views(sc, cam, w, h, _tile_set(name, k), bg, samples=2, filter="bilinear")
        assert np.array_equal(out.get(shape + (3,)), old["rgb"]), k
    assert np.array_equal(cov_b.get(shape), old["coverage"])
    vc.close()


# ---- the output step from device texels -----------------------------------------------------------------------------

def _texels(sc, k):
    """seeded float texels: spread over decades, an all-zero texel (0/0 -> NaN -> byte 0) and one above the clamp"""
    tex = (10.0 ** np.random.default_rng(40 + k).uniform(-3, 1, (sc.num_texels, 4))).astype(f32)
    first = int(sc.walls[0]["lm"][0])
    tex[first + k] = 0
    tex[first + 7 + k, :3] = (3.0e4, 5.0e5, 1.0e6)
    return tex


@pytest.mark.parametrize("spa,tint", [(0, 0), (65_000, 0), (65_000, 1)])
def test_tiles_equal_output_tiles(torch_cuda, spa, tint):
    sc = V._scene("example_tool")
    floors = [r for r in sc.walls if r["pos"][2] == 0 and r["width"][2] == 0 and r["height"][2] == 0]
    assert floors and len(floors) < len(sc.walls), "a floor wall and another"
    vc = fmgi.ViewCache(sc, V._cam("example_tool"), 16, 16)
    n = 3 * vc.info()["tiles"]
    tex = [_texels(sc, k) for k in range(3)]
    dev = [_upload(torch_cuda, t) for t in tex]
    outs = [Out(torch_cuda, n) for _ in tex]
    vc.tiles([d.data_ptr() for d in dev], spa, [o.ptr for o in outs], tint_extra=tint)
    torch_cuda.cuda.synchronize()
    for k in range(3):
        exp = fmgi.output_tiles(sc, tex[k], spa, tint)[1]
        got = outs[k].get()
        assert np.array_equal(got, exp), (k, int((got != exp).sum()))
        assert np.array_equal(dev[k].cpu().numpy(), tex[k]), "the input texels were written"
    assert len({o.get().tobytes() for o in outs}) == 3
    vc.close()


# ---- end to end: the relight session's lightmaps ----------------------------------------------------------------------

CAM = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1), pixel=0.02)  # inside the lit box
PALETTES = ((fmgi.Palette(), fmgi.Palette()),                                             # the reference
            (fmgi.Palette(window_rgb=(0, 0, 0), light_rgb=(0, 0, 0)), fmgi.Palette()),    # windows off
            (fmgi.Palette(), fmgi.Palette(light_rgb=(4, 4, 4.5))))                        # lamp dimmed


def test_bake_recolour_finalize_tiles_shade(torch_cuda):
    torch = torch_cuda
    sc, _, offsets = R.lit_box()
    T = sc.num_texels
    ctx = fmgi.Context(0)
    ctx.set_scene(sc)
    assert ctx.plan(R.SPA, rng_offsets=offsets) == 512
    s = torch.cuda.Stream(device="cuda:0")
    W, H = 32, 24
    with torch.cuda.stream(s):
        infos, blobs = [], []
        for b, e in ((0, 256), (256, 512)):  # the window, the lamp
            info = ctx.bake_sparse(b, e, fmgi.KERNEL_AUTO, s.cuda_stream)
            blob = torch.empty(fmgi.sparse_bytes(T, info.rows) // 8, dtype=torch.int64, device="cuda:0")
            ctx.bake_sparse_take(info, blob.data_ptr(), s.cuda_stream)
            infos.append(info)
            blobs.append(blob)
        lms = [torch.zeros((T, 4), dtype=torch.int64, device="cuda:0") for _ in PALETTES]
        ctx.recolour_sparse([b.data_ptr() for b in blobs], infos, [list(p) for p in PALETTES],
                            [lm.data_ptr() for lm in lms], s.cuda_stream)
        zero = torch.zeros((T, 4), dtype=torch.float32, device="cuda:0")
        texels = [torch.empty((T, 4), dtype=torch.float32, device="cuda:0") for _ in PALETTES]
        for lm, t in zip(lms, texels):
            ctx.finalize(lm.data_ptr(), zero.data_ptr(), t.data_ptr(), s.cuda_stream)
        vc = fmgi.ViewCache(sc, fmgi.camera(**CAM), W, H, 2, "bilinear")
        tiles = [Out(torch, 3 * vc.info()["tiles"]) for _ in PALETTES]
        vc.tiles([t.data_ptr() for t in texels], R.SPA, [o.ptr for o in tiles], stream=s.cuda_stream)
        rgb = [Out(torch, W * H * 3) for _ in PALETTES]
        vc.shade([o.ptr for o in tiles], [o.ptr for o in rgb], BG, stream=s.cuda_stream)
    s.synchronize()
    pictures = []
    for k in range(len(PALETTES)):
        _, exp_tiles = fmgi.output_tiles(sc, texels[k].cpu().numpy(), R.SPA)
        assert np.array_equal(tiles[k].get(), exp_tiles), k
        exp = fmgi.shade_views(sc, fmgi.camera(**CAM), W, H, exp_tiles, BG, samples=2, filter="bilinear")
        got = rgb[k].get((1, H, W, 3))
        assert np.array_equal(got, exp["rgb"]), k
        pictures.append(got.tobytes())
    assert len(set(pictures)) == 3 and exp["coverage"].any()
    vc.close()
    ctx.close()


def test_relight_view_tool(tmp_path):
    """tools/relight.py --view on the lit box: each view.ppm holds fmgi.shade_views' bytes for the tiles it wrote"""
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": {"scale": 0.5}}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4",
                        "--with-light", "--scenarios", str(tmp_path / "scenarios.json"), "--spa", str(R.SPA),
                        "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy"), "--sparse-from-codes", "--view",
                        "--pos", *flat(CAM["pos"]), "--dir", *flat(CAM["dir"]), "--up", *flat(CAM["up"]), "--pixel",
                        "0.02", "--width", "32", "--height", "24", "--samples", "3", "--background", "7", "8", "9",
                        "-o", str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sc = R.lit_box()[0]
    head = b"P6\n32 24\n255\n"
    blobs = []
    for name in ("day", "evening"):
        tiles = np.load(tmp_path / "out" / name / "tiles.npy")
        exp = fmgi.shade_views(sc, fmgi.camera(**CAM), 32, 24, tiles, BG, samples=3, filter="bilinear")
        blob = (tmp_path / "out" / name / "view.ppm").read_bytes()
        assert blob.startswith(head) and blob[len(head):] == exp["rgb"][0].tobytes(), name
        blobs.append(blob)
    assert blobs[0] != blobs[1]
