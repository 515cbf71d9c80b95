"""Supersampled, filtered camera views (fmgi_shade_views / fmgi.shade_views).

No reference program exists for this feature; its definition (include/flatmatch_gi.h) is restated below in
float32 numpy on top of test_view.py's candidate list and walk, and the GPU has to give the restatement's bytes:

  the restatement at one sample / nearest == test_view.restate's wall and texel -> tile bytes            (CPU)
  conditions on the inputs (partial coverage, clamped taps, bilinear != nearest), constant colour       (CPU)
  argument checks and the no-device error of the C ABI                                                  (CPU)
  one sample / nearest == fmgi.render_views' rgb and tests                                              (GPU)
  rgb, coverage and tests == the restatement, bit for bit; batches, image-size edges, windowed launches,
  NULL outputs, no cameras, tools/render_view.py --samples --filter                                     (GPU)

Every comparison is exact: per-sample colours go to 24.8 fixed point and are summed as integers.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
import test_view as T
from conftest import PKG, REPO
from fmgi import _lib

f32 = np.float32
BG = (7, 8, 9)
# fixture cameras at small images, the pixel size scaled by fixture_width / width
SIZES = {"box8_A": (24, 20), "box8_C": (24, 20), "example_tool": (40, 30)}
CASES = list(SIZES)


def _cam(name, width=None):
    fx = T._fixture()[name]
    w = np.array(fx["camera"], f32)
    w[9] = f32(float(w[9]) * fx["width"] / (width or SIZES[name][0]))
    return T._camera(w)


def _scene(name):
    return T._scene(T._fixture()[name]["scene"])


def _tile_counts(sc):
    return np.array([int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls], np.int64)


@functools.lru_cache(None)
def _tiles(name):
    """random RGB8 tiles in wall order"""
    return np.random.default_rng(5).integers(0, 256, 3 * int(_tile_counts(_scene(name)).sum()), dtype=np.uint8)


# ---- the restatement of the definition: float32 in the stated order, vectorised over samples and pixels --------

def _axis(u, n):
    """one axis of the bilinear footprint: the two tile indices, the second one's weight, taps clamped"""
    t = u - f32(0.5)
    t0 = np.floor(t)
    k = t0.astype(np.int64)
    return np.clip(k, 0, n - 1), np.clip(k + 1, 0, n - 1), t - t0, (k < 0) | (k + 1 > n - 1)


def shade(sc, cam, width, height, tiles, bg, S, bilinear):
    """fmgi_shade_views for one camera: dict of rgb and coverage (int64, unclipped), tests, and clamped = the
    number of samples with a bilinear tap clamped to the wall's grid"""
    with np.errstate(all="ignore"):
        cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
        pos, up, pixel = T._v(cam["pos"]), T._v(cam["up"]), f32(cam["pixel"])
        cam_dir = T._normalized(T._v(cam["dir"]))
        centre = T._add(pos, cam_dir)
        right = T._cross(cam_dir, up)
        cw, cd = T._candidates(sc, pos, cam_dir)
        offs = (2 * np.arange(S) + 1 - S).astype(f32) / f32(2 * S)
        j, i, y, x = np.meshgrid(np.arange(S), np.arange(S), np.arange(height), np.arange(width), indexing="ij")
        fx = pixel * ((x - width // 2).astype(f32) + offs[i])
        fy = -pixel * ((y - height // 2).astype(f32) + offs[j])
        d = T._normalized(T._sub(T._add(T._add(centre, T._mul(right, fx)), T._mul(up, fy)), pos))
        wall, dist, tests = T.walk(sc.walls, cw, cd, pos, d)
        hit_pt = T._add(pos, T._mul(d, np.where(wall >= 0, dist, f32(0))))
        val = np.empty(wall.shape + (3,), f32)
        val[...] = np.asarray(bg, f32)
        first = np.concatenate([[0], np.cumsum(_tile_counts(sc))])
        texels = np.asarray(tiles, np.uint8).reshape(-1, 3)
        clamped = 0
        for k in np.unique(wall[wall >= 0]):
            m = wall == k
            r = sc.walls[k]
            w, h = T._v(r["width"]), T._v(r["height"])
            pdir = T._sub(tuple(c[m] for c in hit_pt), T._v(r["pos"]))
            wl, hl = T._length(w), T._length(h)
            s1, s2 = int(r["lm"][1]), int(r["lm"][2])
            u = T._dot(T._mul(w, f32(1.0) / wl), pdir) * f32(s1) / wl  # getTileIdAt, rectangle.c:205-230
            v = T._dot(T._mul(h, f32(1.0) / hl), pdir) * f32(s2) / hl
            tw = texels[first[k]:first[k + 1]].reshape(s2, s1, 3).astype(f32)
            if not bilinear:
                val[m] = tw[np.clip(T._x86_int(v), 0, s2 - 1), np.clip(T._x86_int(u), 0, s1 - 1)]
                continue
            xa, xb, fu, cu = _axis(u, s1)
            ya, yb, fv, cv = _axis(v, s2)
            clamped += int((cu | cv).sum())
            one, fu, fv = f32(1), fu[:, None], fv[:, None]
            top = (one - fu) * tw[ya, xa] + fu * tw[ya, xb]
            bot = (one - fu) * tw[yb, xa] + fu * tw[yb, xb]
            val[m] = (one - fv) * top + fv * bot
        q = (val * f32(256.0) + f32(0.5)).astype(np.int64)
        rgb = (q.sum(axis=(0, 1)) + 128 * S * S) // (256 * S * S)
        return {"rgb": rgb, "coverage": (wall >= 0).sum(axis=(0, 1)), "tests": tests, "clamped": clamped}


@functools.lru_cache(None)
def _restated(name, S, bilinear, width=None, height=None):
    w, h = (width, height) if width else SIZES[name]
    return shade(_scene(name), _cam(name), w, h, _tiles(name), BG, S, bilinear)


# ---- CPU ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_one_nearest_sample_is_the_debug_raycaster(name):
    sc, (w, h) = _scene(name), SIZES[name]
    ref = T.restate(sc, _cam(name), w, h)
    first = np.concatenate([[0], np.cumsum(_tile_counts(sc))[:-1]])
    s0 = np.array([int(r["lm"][0]) for r in sc.walls], np.int64)
    hit = ref["wall"] >= 0
    exp = np.empty((h, w, 3), np.int64)
    exp[...] = BG
    exp[hit] = _tiles(name).reshape(-1, 3)[first[ref["wall"][hit]] + ref["texel"][hit] - s0[ref["wall"][hit]]]
    got = _restated(name, 1, False)
    assert np.array_equal(got["rgb"], exp)
    assert np.array_equal(got["coverage"], hit.astype(np.int64))
    assert got["tests"] == ref["tests"]


def test_input_conditions():
    """what the cases must hold for the comparisons below to mean something"""
    for name in ("box8_C", "example_tool"):
        cov = _restated(name, 3, True)["coverage"]
        assert int(((cov > 0) & (cov < 9)).sum()) > 0, name + ": pixels on a wall's silhouette"
    assert int((_restated("box8_C", 3, True)["coverage"] == 0).sum()) > 0, "misses"
    assert len(T._candidates(_scene("example_tool"), T._v(_cam("example_tool")["pos"]),
                             T._normalized(T._v(_cam("example_tool")["dir"])))[0]) > 100
    for name in CASES:
        near, lin = _restated(name, 1, False), _restated(name, 1, True)
        assert lin["clamped"] > 0, name + ": taps clamped at a wall's edge"
        hit = near["coverage"] > 0
        assert int((near["rgb"][hit] != lin["rgb"][hit]).any(axis=-1).sum()) > 0, name
        assert np.array_equal(near["rgb"][~hit], lin["rgb"][~hit])
        assert np.array_equal(near["coverage"], lin["coverage"]) and near["tests"] == lin["tests"]


@pytest.mark.parametrize("name,S,bilinear", [("box8_A", 2, True), ("box8_C", 3, True), ("box8_C", 8, True),
                                              ("example_tool", 3, True), ("example_tool", 4, False)])
def test_resolved_values_are_bytes(name, S, bilinear):
    r = _restated(name, S, bilinear)
    assert r["rgb"].min() >= 0 and r["rgb"].max() <= 255
    assert r["coverage"].min() >= 0 and r["coverage"].max() == S * S


COLOUR = (201, 3, 255)


def _constant_tiles(name):
    return np.tile(np.array(COLOUR, np.uint8), int(_tile_counts(_scene(name)).sum()))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("bilinear", [False, True])
def test_constant_colour_stays_constant(S, bilinear):
    w, h = SIZES["box8_C"]
    r = shade(_scene("box8_C"), _cam("box8_C"), w, h, _constant_tiles("box8_C"), COLOUR, S, bilinear)
    assert np.all(r["rgb"] == np.array(COLOUR)) and 0 < int((r["coverage"] > 0).sum()) < w * h


def _call(sc, cams, width, height, tiles=None, samples=1, filt=0, rgb=None, cov=None, n=None):
    """fmgi_shade_views through ctypes with explicit arguments; returns the return code"""
    lib = _lib.load()
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    n = len(cams) if n is None else n
    bg = np.array(BG, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return lib.fmgi_shade_views(C.byref(g), p(cams), n, width, height, p(tiles), p(bg), samples, filt, p(rgb), p(cov))


def test_argument_errors_without_a_device():
    """every FMGI_ERR_ARG case is reported before a device is looked for"""
    sc, tiles = _scene("box8_C"), _tiles("box8_C")
    cams = np.atleast_1d(_cam("box8_C"))
    rgb, cov = np.zeros((1, 4, 4, 3), np.uint8), np.zeros((1, 4, 4), np.uint8)
    for samples in (0, 9, -1):
        assert _call(sc, cams, 4, 4, tiles, samples, 0, rgb, cov) == -3, samples
        assert "samples" in _lib.last_error()
    for filt in (2, -1):
        assert _call(sc, cams, 4, 4, tiles, 1, filt, rgb, cov) == -3, filt
        assert "filter" in _lib.last_error()
    assert _call(sc, cams, 4, 4, None, 1, 0, rgb, cov) == -3
    assert "tiles_rgb" in _lib.last_error() and "fmgi_shade_views" in _lib.last_error()
    assert _call(sc, cams, 0, 4, tiles, 1, 0, rgb, cov) == -3  # inherited from fmgi_render_views
    bad = cams.copy()
    bad["pixel"] = 0
    assert _call(sc, bad, 4, 4, tiles, 1, 0, rgb, cov) == -3
    assert "pixel" in _lib.last_error()
    assert not rgb.any() and not cov.any()
    with pytest.raises(fmgi.FmgiError, match="filter"):
        fmgi.shade_views(sc, cams, 4, 4, tiles, filter="cubic")
    assert (_lib.VIEW_NEAREST, _lib.VIEW_BILINEAR, _lib.VIEW_MAX_SAMPLES) == (0, 1, 8)


def test_no_device_is_an_error_code(tmp_path):
    """Without a device fmgi_shade_views returns FMGI_ERR_NO_DEVICE and the process lives on."""
    prog = tmp_path / "nogpu_shade.py"
    prog.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import fmgi\n"
        "from fmgi import scene\n"
        "sc = scene.box_scene(8, tile_size=1.0)\n"
        "cam = fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), pixel=0.02)\n"
        "try:\n"
        "    fmgi.shade_views(sc, cam, 8, 8, samples=2, filter='bilinear')\n"
        "except fmgi.FmgiError as e:\n"
        "    print('ERR', e)\n"
        "print('ALIVE')\n" % PKG
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[1] == "ALIVE"
    assert "fmgi_shade_views failed (-1)" in lines[0]


# ---- GPU ----------------------------------------------------------------------------------------------------

def _assert_equal(got, k, exp):
    bad = (got["rgb"][k].astype(np.int64) != exp["rgb"]).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} pixels differ, the first at {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(got["coverage"][k].astype(np.int64), exp["coverage"])


def _gpu(name, S, bilinear, width=None, height=None, **kw):
    w, h = (width, height) if width else SIZES[name]
    return fmgi.shade_views(_scene(name), _cam(name), w, h, _tiles(name), BG, samples=S,
                            filter="bilinear" if bilinear else "nearest", **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_one_nearest_sample_equals_render_views(torch_cuda, name):
    w, h = SIZES[name]
    ref = fmgi.render_views(_scene(name), _cam(name), w, h, tiles_rgb=_tiles(name), background=BG)
    tests = fmgi.view_stats()["tests"]
    got = _gpu(name, 1, False)
    assert set(got) == {"rgb", "coverage"}
    assert np.array_equal(got["rgb"], ref["rgb"])
    assert np.array_equal(got["coverage"], (ref["wall"] >= 0).astype(np.uint8))
    st = fmgi.view_stats()
    assert st["tests"] == tests and st["rays"] == w * h and st["cameras"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,S,bilinear", [("box8_C", 1, True), ("box8_C", 2, False), ("box8_C", 3, True),
                                              ("box8_C", 4, True), ("box8_C", 8, True), ("example_tool", 3, True),
                                              ("example_tool", 4, False)])
def test_gpu_equals_restatement(torch_cuda, name, S, bilinear):
    w, h = SIZES[name]
    exp = _restated(name, S, bilinear)
    got = _gpu(name, S, bilinear)
    _assert_equal(got, 0, exp)
    st = fmgi.view_stats()
    assert st["tests"] == exp["tests"]
    assert st["rays"] == w * h * S * S and st["cameras"] == 1


@pytest.mark.gpu
def test_gpu_batch_of_cameras(torch_cuda):
    """four box200 cameras in one call (the empty-list camera B between the others) == one call per camera"""
    sc = T._scene("box200")
    names = ["box200_A", "box200_B", "box200_C", "box200_D"]
    cams = np.array([_cam(n, 24) for n in names], fmgi.CAMERA_DTYPE)
    W, H = 24, 20
    tiles = np.random.default_rng(5).integers(0, 256, 3 * int(_tile_counts(sc).sum()), dtype=np.uint8)
    batch = fmgi.shade_views(sc, cams, W, H, tiles, BG, samples=3, filter="bilinear")
    st = fmgi.view_stats()
    tests = cands = 0
    for k, cam in enumerate(cams):
        exp = shade(sc, cam, W, H, tiles, BG, 3, True)
        one = fmgi.shade_views(sc, cam, W, H, tiles, BG, samples=3, filter="bilinear")
        _assert_equal(one, 0, exp)
        _assert_equal(batch, k, exp)
        assert fmgi.view_stats()["tests"] == exp["tests"]
        tests += exp["tests"]
        cands += fmgi.view_stats()["candidates"]
    assert batch["coverage"].shape == (4, H, W) and np.all(batch["coverage"][1] == 0) and np.all(batch["rgb"][1] == BG)
    assert batch["coverage"][0].any()
    assert (st["cameras"], st["rays"], st["tests"], st["candidates"]) == (4, 4 * W * H * 9, tests, cands)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(1, 1), (1, 130), (130, 1)])
def test_gpu_image_size_edges(torch_cuda, width, height):
    exp = _restated("box8_C", 3, True, width, height)
    got = _gpu("box8_C", 3, True, width, height)
    _assert_equal(got, 0, exp)
    assert fmgi.view_stats()["tests"] == exp["tests"] and fmgi.view_stats()["rays"] == width * height * 9


@pytest.mark.gpu
def test_gpu_windowed_launches(torch_cuda, monkeypatch):
    """a ray budget far below one image (FMGI_VIEW_RAYS_PER_LAUNCH) splits the call into windows of pixels, and
    a batch into single cameras: the same bytes and counts"""
    sc = _scene("box8_C")
    cams = np.array([_cam("box8_C"), _cam("box8_A")], fmgi.CAMERA_DTYPE)
    W, H = 50, 37
    whole = fmgi.shade_views(sc, cams, W, H, _tiles("box8_C"), BG, samples=2, filter="bilinear")
    st = fmgi.view_stats()
    monkeypatch.setenv("FMGI_VIEW_RAYS_PER_LAUNCH", "2048")  # 16 x 32 pixel windows at 2 x 2 samples
    parts = fmgi.shade_views(sc, cams, W, H, _tiles("box8_C"), BG, samples=2, filter="bilinear")
    assert np.array_equal(parts["rgb"], whole["rgb"]) and np.array_equal(parts["coverage"], whole["coverage"])
    st2 = fmgi.view_stats()
    assert all(st2[k] == st[k] for k in ("cameras", "rays", "tests", "candidates"))
    _assert_equal(parts, 0, shade(sc, cams[0], W, H, _tiles("box8_C"), BG, 2, True))


@pytest.mark.gpu
def test_gpu_no_cameras_and_null_outputs(torch_cuda):
    sc, tiles = _scene("box8_C"), _tiles("box8_C")
    w, h = SIZES["box8_C"]
    rgb, cov = np.full((1, h, w, 3), 0xA5, np.uint8), np.full((1, h, w), 0x5A, np.uint8)
    assert _call(sc, None, w, h, tiles, 3, 1, rgb, cov, n=0) == 0
    assert np.all(rgb == 0xA5) and np.all(cov == 0x5A)
    st = fmgi.view_stats()
    assert st["cameras"] == 0 and st["rays"] == 0 and st["tests"] == 0
    empty = fmgi.shade_views(sc, np.zeros(0, fmgi.CAMERA_DTYPE), w, h, tiles, samples=2)
    assert empty["rgb"].shape == (0, h, w, 3) and empty["coverage"].shape == (0, h, w)
    # either output may be NULL
    exp = _restated("box8_C", 3, True)
    cams = np.atleast_1d(_cam("box8_C"))
    assert _call(sc, cams, w, h, tiles, 3, 1, rgb, None) == 0
    assert fmgi.view_stats()["tests"] == exp["tests"]
    assert np.array_equal(rgb[0].astype(np.int64), exp["rgb"]) and np.all(cov == 0x5A)
    rgb[...] = 0xA5
    assert _call(sc, cams, w, h, None, 3, 1, None, cov) == 0  # coverage needs no tiles
    assert np.array_equal(cov[0].astype(np.int64), exp["coverage"]) and np.all(rgb == 0xA5)
    assert fmgi.view_stats()["tests"] == exp["tests"]
    assert _call(sc, cams, w, h, tiles, 3, 1, None, None) == 0
    assert fmgi.view_stats()["tests"] == exp["tests"]
    only_cov = fmgi.shade_views(sc, cams, w, h, samples=3, filter="bilinear")
    assert set(only_cov) == {"coverage"} and np.array_equal(only_cov["coverage"], cov)


@pytest.mark.gpu
@pytest.mark.parametrize("bilinear", [False, True])
def test_gpu_constant_colour_at_eight_samples(torch_cuda, bilinear):
    w, h = SIZES["box8_C"]
    got = fmgi.shade_views(_scene("box8_C"), _cam("box8_C"), w, h, _constant_tiles("box8_C"), COLOUR, samples=8,
                           filter="bilinear" if bilinear else "nearest")
    assert np.all(got["rgb"] == np.array(COLOUR, np.uint8))
    assert got["coverage"].max() == 64 and got["coverage"].min() == 0


@pytest.mark.gpu
def test_gpu_render_view_tool(torch_cuda, tmp_path):
    """tools/render_view.py --samples 3 --filter bilinear writes the bytes shade_views returns"""
    sc = T._scene("box8")
    rng = np.random.default_rng(5)
    tex = (10.0 ** rng.uniform(-3, 1, (sc.num_texels, 4))).astype(f32)
    np.save(tmp_path / "texels.npy", tex)
    ppm = tmp_path / "view.ppm"
    cam = dict(pos=(5, 4, 20), dir=(0, 0, -1), up=(0, 1, 0), pixel=0.1)  # from above: hits and misses
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "render_view.py"), "box8", "--tile-size", "1",
                        "--texels", str(tmp_path / "texels.npy"), "--spa", "1000", "--pos", *flat(cam["pos"]),
                        "--dir", *flat(cam["dir"]), "--up", *flat(cam["up"]), "--pixel", "0.1", "--width", "16",
                        "--height", "12", "--background", "1", "2", "3", "--samples", "3", "--filter", "bilinear",
                        "-o", str(ppm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{16 * 12 * 9} rays" in r.stdout
    blob = ppm.read_bytes()
    head = b"P6\n16 12\n255\n"
    assert blob.startswith(head) and len(blob) == len(head) + 16 * 12 * 3
    _, tiles = fmgi.output_tiles(sc, tex, 1000, 0)
    got = fmgi.shade_views(sc, fmgi.camera(**cam), 16, 12, tiles, (1, 2, 3), samples=3, filter="bilinear")
    near = fmgi.render_views(sc, fmgi.camera(**cam), 16, 12, tiles_rgb=tiles, background=(1, 2, 3))
    assert 0 < int((got["coverage"] > 0).sum()) < 16 * 12 and not np.array_equal(got["rgb"], near["rgb"])
    assert blob[len(head):] == got["rgb"][0].tobytes()
