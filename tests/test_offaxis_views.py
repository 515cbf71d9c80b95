"""Camera views and the output step on partitioned, tilted and open scenes (tests/offaxis_scenes.py).

tests/test_view.py's cases are axis-aligned and, but for a camera pointed out of a window, closed. Here the
reference's debug raycaster was recorded (tests/golden/make_view_fixtures.py offaxis -> view_ref_offaxis.npz) for
two 64 x 48 cameras on each of crossing, tilted12 and open_tilted: one looks along a tilted panel, meeting it at
about two degrees, and one looks up and out of the scene without a ceiling.

  reference == test_view.restate on the six cases; what the cases must hold                               (CPU)
  fmgi.view_candidates / render_views / view_stats == fixture and restatement, bit for bit               (GPU)
  view_candidates == the restatement's sorted list at 256 and 257 rects (sort_n 256 and 512)             (GPU)
  shade_views: one nearest sample == render_views' rgb; 2 x 2 bilinear == test_view_shade.shade          (GPU)
  ViewCache tiles + shade == output_tiles + shade_views on open_tilted (miss records), tilted12 (grazing) (GPU)
  output_tiles on open_tilted == the oracle's bytes; only floor walls take the floor tint                (GPU)
"""
import functools
import json
import os

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import offaxis_scenes as S
import test_view as T
import test_view_shade as V
from conftest import GOLDEN

f32 = np.float32
CASES = ["crossing_P", "crossing_C", "tilted12_graze", "tilted12_A", "open_tilted_graze", "open_tilted_sky"]
W, H = 64, 48
BG = V.BG
KEYS = ("camera", "cand_wall", "cand_bits", "wall", "texel", "dist_bits", "tests")


@functools.lru_cache(None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, "view_ref_offaxis.npz"))
    meta = json.loads(str(z["meta"]))
    return {name: dict(m, **{k: z[f"{name}.{k}"] for k in KEYS}) for name, m in meta.items()}


def _case(name):
    fx = _fixture()[name]
    return fx, S.get(fx["scene"]), T._camera(fx["camera"])


@functools.lru_cache(None)
def _restated(name):
    fx, sc, cam = _case(name)
    return T.restate(sc, cam, fx["width"], fx["height"])


@functools.lru_cache(None)
def _tiles(scene_name, k=0):
    """random RGB8 tiles in wall order"""
    n = 3 * int(V._tile_counts(S.get(scene_name)).sum())
    return np.random.default_rng(5 + k).integers(0, 256, n, dtype=np.uint8)


@functools.lru_cache(None)
def _shaded(name, samples, bilinear):
    fx, sc, cam = _case(name)
    return V.shade(sc, cam, W, H, _tiles(fx["scene"]), BG, samples, bilinear)


# ---- CPU ----------------------------------------------------------------------------------------------------

def test_fixture_holds_the_six_cases():
    assert sorted(_fixture()) == sorted(CASES)
    assert all((f["width"], f["height"]) == (W, H) for f in _fixture().values())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    fx, r = _fixture()[name], _restated(name)
    assert np.array_equal(r["cand_wall"], fx["cand_wall"])
    assert np.array_equal(T._bits(r["cand_dist"]), fx["cand_bits"])
    assert np.array_equal(r["wall"], fx["wall"]), int((r["wall"] != fx["wall"]).sum())
    assert np.array_equal(r["texel"], fx["texel"]), int((r["texel"] != fx["texel"]).sum())
    assert np.array_equal(T._bits(r["dist"]), fx["dist_bits"])
    assert r["tests"] == int(fx["tests"])


def _ray_dirs(cam, width, height):
    """the pixel rays of test_view.restate"""
    cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
    pos, up, pixel = T._v(cam["pos"]), T._v(cam["up"]), f32(cam["pixel"])
    cam_dir = T._normalized(T._v(cam["dir"]))
    y, x = np.mgrid[0:height, 0:width]
    fx, fy = pixel * (x - width // 2).astype(f32), -pixel * (y - height // 2).astype(f32)
    screen = T._add(T._add(T._add(pos, cam_dir), T._mul(T._cross(cam_dir, up), fx)), T._mul(up, fy))
    return np.stack(T._normalized(T._sub(screen, pos)), axis=-1)


def test_fixture_conditions():
    fxs = _fixture()
    # a tilted panel seen edge-on: every ray that lands on it meets it at less than five degrees
    for name, panel in (("tilted12_graze", 200), ("open_tilted_graze", 164)):
        fx, sc, cam = _case(name)
        n = sc.walls[panel]["n"][:3]
        assert (np.abs(n) > 1e-3).sum() >= 2, "the panel is off-axis"
        on = fx["wall"] == panel
        # edge-on it is a sliver: 0.98 m tall at no more than 1.75 m is 28 rows of 0.02, at least a pixel wide
        assert int(on.sum()) >= 28, name
        sin = np.abs(_ray_dirs(cam, W, H)[on] @ n.astype(np.float64))
        assert sin.max() < np.sin(np.radians(5.0)), float(np.degrees(np.arcsin(sin.max())))
    # hits on tilted and sloped rects in the general views
    seen = set(np.unique(fxs["tilted12_A"]["wall"])) | set(np.unique(fxs["tilted12_graze"]["wall"]))
    assert len(seen & set(range(200, 212))) >= 3
    # misses: through the missing ceiling, and past the box from above
    sky = fxs["open_tilted_sky"]["wall"]
    assert 0.5 < float((sky < 0).mean()) < 0.95
    assert 0 < int((fxs["open_tilted_graze"]["wall"] < 0).sum()) < W * H
    assert int((fxs["crossing_C"]["wall"] < 0).sum()) > 0
    # the partitions are seen
    assert len(set(np.unique(fxs["crossing_P"]["wall"])) & set(range(200, 216))) >= 4
    for f in fxs.values():
        missed = f["wall"] < 0
        assert np.all(f["texel"][missed] == -1) and np.all(f["dist_bits"][missed] == 0x7F800000)


# ---- GPU ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_equals_reference_and_restatement(torch_cuda, name):
    fx, sc, cam = _case(name)
    r = _restated(name)
    idx, md = fmgi.view_candidates(sc, cam)
    assert np.array_equal(idx, fx["cand_wall"]) and np.array_equal(T._bits(md), fx["cand_bits"])
    tiles = _tiles(fx["scene"])
    got = fmgi.render_views(sc, cam, W, H, tiles_rgb=tiles, background=BG)
    T._assert_equal(got, 0, fx["wall"], fx["texel"], fx["dist_bits"])
    T._assert_equal(got, 0, r["wall"], r["texel"], T._bits(r["dist"]))
    st = fmgi.view_stats()
    assert st["tests"] == int(fx["tests"]) and st["candidates"] == len(fx["cand_wall"])
    assert st["rays"] == W * H and st["cameras"] == 1
    # one nearest sample is the debug raycaster's picture
    near = fmgi.shade_views(sc, cam, W, H, tiles, BG, samples=1, filter="nearest")
    assert np.array_equal(near["rgb"], got["rgb"])
    assert np.array_equal(near["coverage"], (got["wall"] >= 0).astype(np.uint8))
    exp = _shaded(name, 1, False)
    assert np.array_equal(near["rgb"][0].astype(np.int64), exp["rgb"])
    assert np.all(got["rgb"][0][fx["wall"] < 0] == np.array(BG, np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_bilinear_supersampled_equals_restatement(torch_cuda, name):
    fx, sc, cam = _case(name)
    exp = _shaded(name, 2, True)
    got = fmgi.shade_views(sc, cam, W, H, _tiles(fx["scene"]), BG, samples=2, filter="bilinear")
    V._assert_equal(got, 0, exp)
    st = fmgi.view_stats()
    assert st["tests"] == exp["tests"] and st["rays"] == W * H * 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tilted56", "tilted57"])
@pytest.mark.parametrize("cam", ["tilted12_A", "tilted12_graze"])
def test_gpu_candidates_at_the_power_of_two_edge(torch_cuda, name, cam):
    """256 rects sort as 256 keys without padding, 257 as 512 keys with 255 pad keys"""
    sc, camera = S.get(name), T._camera(_fixture()[cam]["camera"])
    pos, cam_dir = T._v(camera["pos"]), T._normalized(T._v(camera["dir"]))
    with np.errstate(all="ignore"):
        cw, cd = T._candidates(sc, pos, cam_dir)
    assert len(cw) > 100
    idx, md = fmgi.view_candidates(sc, camera)
    assert np.array_equal(idx, cw) and np.array_equal(T._bits(md), T._bits(cd))
    r = T.restate(sc, camera, 32, 24)
    got = fmgi.render_views(sc, camera, 32, 24)
    T._assert_equal(got, 0, r["wall"], r["texel"], T._bits(r["dist"]))
    assert fmgi.view_stats()["tests"] == r["tests"]


def _texels(sc, k):
    """seeded float texels over decades, an all-zero texel (0/0 in the tone map) and one above the clamp"""
    tex = (10.0 ** np.random.default_rng(40 + k).uniform(-3, 1, (sc.num_texels, 4))).astype(f32)
    tex[3 + k] = 0
    tex[11 + k, :3] = (3.0e4, 5.0e5, 1.0e6)
    return tex


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["open_tilted_sky", "open_tilted_graze", "tilted12_graze"])
def test_gpu_view_cache_equals_the_host_path(torch_cuda, name):
    """ViewCache.tiles + ViewCache.shade == fmgi.output_tiles + fmgi.shade_views == the restatement"""
    import test_gpu_view_cache as G

    fx, sc, cam = _case(name)
    spa = 65_000
    for bilinear, samples in ((True, 2), (False, 1)):
        filt = "bilinear" if bilinear else "nearest"
        vc = fmgi.ViewCache(sc, cam, W, H, samples, filt)
        info = vc.info()
        tex = [_texels(sc, k) for k in range(2)]
        dev = [G._upload(torch_cuda, t) for t in tex]
        tiles = [G.Out(torch_cuda, 3 * info["tiles"]) for _ in tex]
        vc.tiles([d.data_ptr() for d in dev], spa, [o.ptr for o in tiles], tint_extra=1)
        rgb = [G.Out(torch_cuda, W * H * 3) for _ in tex]
        cov = G.Out(torch_cuda, W * H)
        torch_cuda.cuda.synchronize()
        vc.shade([o.ptr for o in tiles], [o.ptr for o in rgb], BG, cov.ptr)
        torch_cuda.cuda.synchronize()
        for k in range(2):
            exp_tiles = fmgi.output_tiles(sc, tex[k], spa, 1)[1]
            assert np.array_equal(tiles[k].get(), exp_tiles), k
            assert np.array_equal(exp_tiles, O.output_tiles(sc, tex[k], spa, 1)[1]), k
            old = fmgi.shade_views(sc, cam, W, H, exp_tiles, BG, samples=samples, filter=filt)
            assert np.array_equal(rgb[k].get((1, H, W, 3)), old["rgb"]), k
            assert np.array_equal(cov.get((1, H, W)), old["coverage"])
            V._assert_equal(old, 0, V.shade(sc, cam, W, H, exp_tiles, BG, samples, bilinear))
        exp = _shaded(name, samples, bilinear)
        assert info["tests"] == exp["tests"] and info["hits"] == int(exp["coverage"].sum())
        assert info["rays"] == W * H * samples * samples
        vc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tint", [0, 1])
def test_gpu_output_tiles_on_the_open_tilted_scene(torch_cuda, tint):
    sc = S.get("open_tilted")
    rng = np.random.default_rng(11 + tint)
    tex = (10.0 ** rng.uniform(-6, 3, (sc.num_texels, 4))).astype(f32)
    tex[rng.random(sc.num_texels) < 0.01] = 0
    for spa in (0, 172_413_793):
        n_o, rgb_o = O.output_tiles(sc, tex, spa, tint)
        n_g, rgb_g = fmgi.output_tiles(sc, tex, spa, tint)
        assert np.array_equal(rgb_g, rgb_o), int((rgb_g != rgb_o).sum())
        assert np.array_equal(n_g.view(np.uint32), n_o.view(np.uint32))
    # grey texels: a tile without the floor tint keeps r == g == b, a floor tile gets g = int(0.95 r) or less
    grey = np.repeat(rng.uniform(0.05, 1.5, (sc.num_texels, 1)).astype(f32), 4, axis=1)
    _, rgb = fmgi.output_tiles(sc, grey, 0, tint)
    assert np.array_equal(rgb, O.output_tiles(sc, grey, 0, tint)[1])
    counts = V._tile_counts(sc)
    first = np.concatenate([[0], np.cumsum(counts)])
    px = rgb.reshape(-1, 3).astype(np.int64)
    for i, w in enumerate(sc.walls):
        t = px[first[i]:first[i + 1]]
        is_floor = w["pos"][2] == 0 and w["width"][2] == 0 and w["height"][2] == 0
        assert is_floor == (i < 36)
        assert t[:, 0].min() > 20
        if is_floor:
            assert np.all(t[:, 1] < t[:, 0]) and np.all(t[:, 2] < t[:, 1]), i
        else:
            assert np.all(t[:, 0] == t[:, 1]) and np.all(t[:, 1] == t[:, 2]), i
    assert len(sc.walls) - 12 == 164 and all((np.abs(w["n"][:3]) > 1e-3).sum() >= 2 for w in sc.walls[164:])
