"""View renderer: the reference's debug raycaster (debugRaytracer.cc:121-176 over
radiosityNative.c:25-90) on the GPU, for any camera and for batches of cameras.

  reference functions (tests/golden/view_ref_main.c, view_ref.npz) == the numpy restatement below   (CPU)
  argument checks and the no-device error of the C ABI                                             (CPU)
  fixture == fmgi.view_candidates / fmgi.render_views / fmgi.view_stats, bit for bit, every pixel   (GPU)
  batches, image-size edge cases, lit pixels from the output step's tiles, tools/render_view.py     (GPU)

Every comparison is exact: candidate indices and distance bits, per-pixel wall, texel and distance bits,
and the number of intersects() evaluations (which pins where each ray's walk of the sorted list stops).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fmgi
from conftest import GOLDEN, PKG, REPO
from fmgi import _lib, scene

f32 = np.float32
CASES = ["example_tool", "example_plan", "example_tool_pixel", "box200_A", "box200_C", "box200_D", "box200_B",
         "box2000_A", "box2000_C", "box2000_D", "box8_A", "box8_C"]


@functools.lru_cache(None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, "view_ref.npz"))
    meta = json.loads(str(z["meta"]))
    return {name: dict(m, **{k: z[f"{name}.{k}"] for k in ("camera", "cand_wall", "cand_bits", "wall", "texel",
                                                            "dist_bits", "tests")})
            for name, m in meta.items()}


@functools.lru_cache(None)
def _scene(name):
    if name == "example":
        return scene.load_geometry(os.path.join(GOLDEN, "example_geometry.bin"), "example")
    return {"box200": lambda: scene.box_scene(200, tile_size=2.0), "box2000": lambda: scene.box_scene(2000, tile_size=2.0),
            "box8": lambda: scene.box_scene(8, tile_size=1.0)}[name]()


def _camera(words):
    w = np.asarray(words, f32)
    return fmgi.camera(w[0:3], w[3:6], w[6:9], w[9])


# ---- the restatement: every operation float32, in the reference's order, vectorised over walls / pixels ----

def _v(a):
    """three float32 components (scalars or arrays) of an [..., >=3] array"""
    a = np.asarray(a, f32)
    return a[..., 0], a[..., 1], a[..., 2]


def _add(a, b):
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1], a[2] - b[2]


def _mul(a, f):
    return a[0] * f, a[1] * f, a[2] * f


def _dot(a, b):  # vector3_cl.c:76-79, left to right
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):  # vector3_cl.c:81-86
    return a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]


def _length(a):  # vector3_cl.c:93
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _normalized(a):  # vector3_cl.c:95-100: one reciprocal, three multiplies
    return _mul(a, f32(1.0) / _length(a))


def _candidates(sc, pos, cam_dir):
    """getSortedIntersectableRects (radiosityNative.c:25-62) over the walls: (wall indices, minDistance)."""
    W = sc.walls
    p, w, h, n = _v(W["pos"]), _v(W["width"]), _v(W["height"]), _v(W["n"])
    backface = _dot(n, _sub(p, pos)) > 0
    corners = (p, _add(p, w), _add(p, h), _add(_add(p, w), h))  # isBehindRay, rectangle.c:97-113
    behind = np.ones(len(W), bool)
    for c in corners:
        behind &= _dot(_sub(c, pos), cam_dir) < 0
    # getShortestDistanceRectToPoint, rectangle.c:442-473
    on_plane = _sub(pos, _mul(n, _dot(_sub(pos, p), n)))
    pd = _sub(on_plane, p)
    u = _dot(pd, _normalized(h)) / _length(h)
    v = _dot(pd, _normalized(w)) / _length(w)
    u = np.where(u < 0, f32(0), np.where(u > 1, f32(1), u))
    v = np.where(v < 0, f32(0), np.where(v > 1, f32(1), v))
    md = _length(_sub(pos, _add(_add(p, _mul(w, v)), _mul(h, u))))
    keep = np.flatnonzero(~backface & ~behind)
    order = keep[np.lexsort((keep, md[keep]))]  # a stable sort of the filtered walls: (distance, wall index)
    return order.astype(np.int32), md[order].astype(f32)


def _intersects(r, src, d, closest):
    """rectangle.c:67-95 on one wall for all pixels: the hit distance, or -1"""
    n, p, w, h = _v(r["n"]), _v(r["pos"]), _v(r["width"]), _v(r["height"])
    denom = _dot(n, d)
    ok = ~(denom >= 0)
    fac = _dot(n, _sub(p, src)) / denom
    ok &= ~(fac < 0)
    ray = _mul(d, fac)
    ok &= ~(closest * closest < _dot(ray, ray))
    pdir = _sub(_add(src, ray), p)
    wl, hl = _length(w), _length(h)
    dx = _dot(_mul(w, f32(1.0) / wl), pdir)  # div_vec3, vector3_cl.c:53-58
    dy = _dot(_mul(h, f32(1.0) / hl), pdir)
    ok &= ~((dx < 0) | (dy < 0) | (dx > wl) | (dy > hl))
    return np.where(ok, fac, f32(-1))


def _x86_int(v):
    """cvttss2si, the reference's (int) cast: out of range and NaN give INT_MIN"""
    ok = (v >= f32(-2147483648.0)) & (v < f32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64), -2 ** 31)


def _tile_id(r, pt):
    """getTileIdAt, rectangle.c:205-230"""
    w, h = _v(r["width"]), _v(r["height"])
    pdir = _sub(pt, _v(r["pos"]))
    wl, hl = _length(w), _length(h)
    dx = _dot(_mul(w, f32(1.0) / wl), pdir)
    dy = _dot(_mul(h, f32(1.0) / hl), pdir)
    s1, s2 = int(r["lm"][1]), int(r["lm"][2])
    tx = np.clip(_x86_int(dx * f32(s1) / wl), 0, s1 - 1)
    ty = np.clip(_x86_int(dy * f32(s2) / hl), 0, s2 - 1)
    return ty * s1 + tx


def walk(walls, cw, cd, src, d):
    """findClosestIntersectionSorted (radiosityNative.c:67-90) for an array of rays over one candidate list:
    (wall index or -1, distance or inf, number of intersects() evaluations)"""
    shape = np.shape(d[0])
    dist = np.full(shape, np.inf, f32)
    wall = np.full(shape, -1, np.int32)
    walking = np.ones(shape, bool)
    tests = 0
    for i, md in zip(cw, cd):
        walking &= ~(dist < md)
        if not walking.any():
            break
        tests += int(walking.sum())
        dn = _intersects(walls[i], src, d, dist)
        take = walking & ~(dn < 0) & (dn <= dist)
        wall[take] = i
        dist[take] = dn[take]
    return wall, dist, tests


def restate(sc, cam, width, height):
    """The loop of debugRaytracer.cc:121-176 for one camera: dict of cand_wall, cand_dist, wall, texel, dist,
    tests."""
    with np.errstate(all="ignore"):
        cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
        pos, up, pixel = _v(cam["pos"]), _v(cam["up"]), f32(cam["pixel"])
        cam_dir = _normalized(_v(cam["dir"]))
        centre = _add(pos, cam_dir)
        right = _cross(cam_dir, up)
        cw, cd = _candidates(sc, pos, cam_dir)
        y, x = np.mgrid[0:height, 0:width]
        fx = pixel * (x - width // 2).astype(f32)
        fy = -pixel * (y - height // 2).astype(f32)
        screen = _add(_add(centre, _mul(right, fx)), _mul(up, fy))  # add3: left to right
        d = _normalized(_sub(screen, pos))
        wall, dist, tests = walk(sc.walls, cw, cd, pos, d)
        texel = np.full((height, width), -1, np.int32)
        hit_pt = _add(pos, _mul(d, np.where(wall >= 0, dist, f32(0))))
        for i in np.unique(wall[wall >= 0]):
            m = wall == i
            texel[m] = (int(sc.walls[i]["lm"][0]) + _tile_id(sc.walls[i], tuple(c[m] for c in hit_pt))).astype(np.int32)
    return {"cand_wall": cw, "cand_dist": cd, "wall": wall, "texel": texel, "dist": dist, "tests": tests}


@functools.lru_cache(None)
def _restated(name):
    fx = _fixture()[name]
    return restate(_scene(fx["scene"]), _camera(fx["camera"]), fx["width"], fx["height"])


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- CPU ----------------------------------------------------------------------------------------------------

def test_fixture_holds_the_twelve_cases():
    assert sorted(_fixture()) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference(name):
    fx, r = _fixture()[name], _restated(name)
    assert np.array_equal(r["cand_wall"], fx["cand_wall"])
    assert np.array_equal(_bits(r["cand_dist"]), fx["cand_bits"])
    assert np.array_equal(r["wall"], fx["wall"]), int((r["wall"] != fx["wall"]).sum())
    assert np.array_equal(r["texel"], fx["texel"]), int((r["texel"] != fx["texel"]).sum())
    assert np.array_equal(_bits(r["dist"]), fx["dist_bits"])
    assert r["tests"] == int(fx["tests"])


def _ties(fx):
    b = fx["cand_bits"]
    return int((b[1:] == b[:-1]).sum())


def test_fixture_conditions():
    fxs = _fixture()
    hits = {n: int((f["wall"] >= 0).sum()) for n, f in fxs.items()}
    pix = {n: f["wall"].size for n, f in fxs.items()}
    assert any(0 < hits[n] < pix[n] for n in fxs), "a case with hits and misses"
    assert any(len(f["cand_wall"]) == 0 and hits[n] == 0 for n, f in fxs.items()), "a case without candidates"
    assert any(_ties(f) > 0 for f in fxs.values()), "a case with equal-distance candidates"
    kinds = set()
    f = fxs["example_tool"]
    sc = _scene("example")
    for w in np.unique(f["wall"][f["wall"] >= 0]):
        nz = float(sc.walls[w]["n"][2])
        kinds.add("floor" if nz > 0.5 else "ceiling" if nz < -0.5 else "wall")
    assert kinds == {"floor", "ceiling", "wall"}
    for n, f in fxs.items():
        if len(f["cand_wall"]):
            assert int(f["tests"]) < pix[n] * len(f["cand_wall"]), n
        else:
            assert int(f["tests"]) == 0
        missed = f["wall"] < 0
        assert np.all(f["texel"][missed] == -1) and np.all(f["dist_bits"][missed] == 0x7F800000)
        s0 = np.array([int(w["lm"][0]) for w in _scene(f["scene"]).walls])
        n_t = np.array([int(w["lm"][1]) * int(w["lm"][2]) for w in _scene(f["scene"]).walls])
        hw = f["wall"][~missed]
        assert np.all(f["texel"][~missed] >= s0[hw]) and np.all(f["texel"][~missed] < s0[hw] + n_t[hw])


def _call(sc, cams, width, height, tiles=None, rgb=False, num_walls=None, num_texels=None, n=None):
    """fmgi_render_views through ctypes with explicit arguments; returns the return code"""
    lib = _lib.load()
    cams = np.ascontiguousarray(np.atleast_1d(np.asarray(cams, fmgi.CAMERA_DTYPE)))
    g, keep = fmgi.make_geometry(sc, np.zeros((max(sc.num_texels, 1), 4), f32))
    if num_walls is not None:
        g.numWalls = num_walls
    if num_texels is not None:
        g.numTexels = num_texels
    n = len(cams) if n is None else n
    out = np.zeros((max(n, 1), height if height > 0 else 1, width if width > 0 else 1, 3), np.uint8)
    bg = np.zeros(3, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return lib.fmgi_render_views(C.byref(g), p(cams), n, width, height, None if tiles is None else p(tiles), p(bg),
                                 None, None, None, p(out) if rgb else None)


CAM_A = dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1), pixel=0.02)


def test_argument_errors_without_a_device():
    """every FMGI_ERR_ARG case is reported before a device is looked for"""
    sc = _scene("box8")
    ok = fmgi.camera(**CAM_A)
    assert _call(sc, ok, 0, 4) == -3 and _call(sc, ok, 4, 0) == -3 and _call(sc, ok, -1, 4) == -3
    for pixel in (0.0, -0.01, np.inf, np.nan):
        assert _call(sc, fmgi.camera(**dict(CAM_A, pixel=pixel)), 4, 4) == -3, pixel
    assert "pixel" in _lib.last_error()
    assert _call(sc, fmgi.camera(**dict(CAM_A, dir=(0, 0, 0))), 4, 4) == -3
    assert "direction" in _lib.last_error()
    assert _call(sc, [ok, fmgi.camera(**dict(CAM_A, dir=(0, 0, 0)))], 4, 4) == -3, "any camera of a batch"
    assert _call(sc, ok, 4, 4, rgb=True) == -3
    assert "tiles_rgb" in _lib.last_error()
    many = scene.Scene("many", np.tile(sc.walls[:1], 16385), sc.windows, sc.lights, sc.num_texels)
    assert _call(many, ok, 4, 4) == -3
    assert "16384" in _lib.last_error()
    assert _call(sc, ok, 4, 4, num_texels=int(sc.walls[-1]["lm"][0])) == -3
    assert "outside" in _lib.last_error()
    neg = sc.walls.copy()
    neg[0]["lm"][0] = -1
    assert _call(scene.Scene("neg", neg, sc.windows, sc.lights, sc.num_texels), ok, 4, 4) == -3
    assert fmgi.CAMERA_DTYPE.itemsize == 40
    with pytest.raises(fmgi.FmgiError, match="tiles_rgb"):
        _lib.check(_call(sc, ok, 4, 4, rgb=True), "fmgi_render_views")


def test_no_device_is_an_error_code(tmp_path):
    """Without a device fmgi_render_views returns FMGI_ERR_NO_DEVICE and the process lives on."""
    prog = tmp_path / "nogpu_view.py"
    prog.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import fmgi\n"
        "from fmgi import scene\n"
        "sc = scene.box_scene(8, tile_size=1.0)\n"
        "cam = fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), pixel=0.02)\n"
        "try:\n"
        "    fmgi.render_views(sc, cam, 8, 8)\n"
        "except fmgi.FmgiError as e:\n"
        "    print('ERR', e)\n"
        "try:\n"
        "    fmgi.view_candidates(sc, cam)\n"
        "except fmgi.FmgiError as e:\n"
        "    print('ERR', e)\n"
        "print('ALIVE')\n" % PKG
    )
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and lines[2] == "ALIVE"
    assert "fmgi_render_views failed (-1)" in lines[0] and "fmgi_view_candidates failed (-1)" in lines[1]


# ---- GPU ----------------------------------------------------------------------------------------------------

def _assert_equal(got, k, exp_wall, exp_texel, exp_dist_bits):
    assert np.array_equal(got["wall"][k], exp_wall), int((got["wall"][k] != exp_wall).sum())
    assert np.array_equal(got["texel"][k], exp_texel), int((got["texel"][k] != exp_texel).sum())
    assert np.array_equal(_bits(got["dist"][k]), exp_dist_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_gpu_equals_reference(torch_cuda, name):
    fx = _fixture()[name]
    sc, cam = _scene(fx["scene"]), _camera(fx["camera"])
    idx, md = fmgi.view_candidates(sc, cam)
    n = min(len(idx), len(fx["cand_wall"]))
    bad = np.flatnonzero((idx[:n] != fx["cand_wall"][:n]) | (_bits(md[:n]) != fx["cand_bits"][:n]))
    assert len(bad) == 0, f"candidate lists differ from entry {bad[0]}"
    assert len(idx) == len(fx["cand_wall"])
    got = fmgi.render_views(sc, cam, fx["width"], fx["height"])
    assert set(got) == {"wall", "texel", "dist"}
    _assert_equal(got, 0, fx["wall"], fx["texel"], fx["dist_bits"])
    st = fmgi.view_stats()
    assert st["tests"] == int(fx["tests"])
    assert st["candidates"] == len(fx["cand_wall"])
    assert st["rays"] == fx["width"] * fx["height"] and st["cameras"] == 1


@pytest.mark.gpu
def test_gpu_batch_of_cameras(torch_cuda):
    """the four box200 cameras at one common size in one call (the empty-list camera B between the others) ==
    one call per camera == the restatement"""
    sc = _scene("box200")
    names = ["box200_A", "box200_B", "box200_C", "box200_D"]
    cams = np.array([_camera(_fixture()[n]["camera"]) for n in names], fmgi.CAMERA_DTYPE)
    W, H = 67, 45
    batch = fmgi.render_views(sc, cams, W, H)
    st = fmgi.view_stats()
    tests = cands = 0
    for k, cam in enumerate(cams):
        one = fmgi.render_views(sc, cam, W, H)
        exp = restate(sc, cam, W, H)
        _assert_equal(one, 0, exp["wall"], exp["texel"], _bits(exp["dist"]))
        _assert_equal(batch, k, exp["wall"], exp["texel"], _bits(exp["dist"]))
        assert fmgi.view_stats()["tests"] == exp["tests"]
        tests += exp["tests"]
        cands += len(exp["cand_wall"])
    assert batch["wall"].shape == (4, H, W) and np.all(batch["wall"][1] == -1)
    assert (st["cameras"], st["rays"], st["tests"], st["candidates"]) == (4, 4 * W * H, tests, cands)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", [(1, 1), (1, 130), (130, 1)])
def test_gpu_image_size_edges(torch_cuda, width, height):
    sc, cam = _scene("box200"), _camera(_fixture()["box200_A"]["camera"])
    got = fmgi.render_views(sc, cam, width, height)
    exp = restate(sc, cam, width, height)
    _assert_equal(got, 0, exp["wall"], exp["texel"], _bits(exp["dist"]))
    assert fmgi.view_stats()["tests"] == exp["tests"] and fmgi.view_stats()["rays"] == width * height


@pytest.mark.gpu
def test_gpu_no_cameras_writes_nothing(torch_cuda):
    sc = _scene("box200")
    lib = _lib.load()
    g, keep = fmgi.make_geometry(sc, np.zeros((sc.num_texels, 4), f32))
    wall = np.full((2, 8, 8), 0x5A5A5A5A, np.int32)
    texel, dist, rgb = wall.copy(), np.full((2, 8, 8), 1234.5, f32), np.full((2, 8, 8, 3), 0xA5, np.uint8)
    tiles = np.zeros(lib.fmgi_output_tile_bytes(C.byref(g)), np.uint8)
    bg = np.zeros(3, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.fmgi_render_views(C.byref(g), None, 0, 8, 8, p(tiles), p(bg), p(wall), p(texel), p(dist), p(rgb)) == 0
    assert np.all(wall == 0x5A5A5A5A) and np.all(texel == 0x5A5A5A5A) and np.all(dist == f32(1234.5))
    assert np.all(rgb == 0xA5)
    st = fmgi.view_stats()
    assert st["cameras"] == 0 and st["rays"] == 0 and st["tests"] == 0
    empty = fmgi.render_views(sc, np.zeros(0, fmgi.CAMERA_DTYPE), 8, 8)
    assert empty["wall"].shape == (0, 8, 8)


def _first_tile(sc):
    n = np.array([int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls], np.int64)
    return np.concatenate([[0], np.cumsum(n)[:-1]]), np.array([int(w["lm"][0]) for w in sc.walls], np.int64)


@pytest.mark.gpu
def test_gpu_lit_pixels(torch_cuda):
    """rgb == the output step's tile bytes at 3 * (first_tile[wall] + texel - s0); a miss == the background"""
    sc = _scene("box200")
    rng = np.random.default_rng(23)
    tex = (10.0 ** rng.uniform(-6, 3, (sc.num_texels, 4))).astype(f32)
    tex[rng.random(sc.num_texels) < 0.05] = 0
    _, tiles = fmgi.output_tiles(sc, tex, 0, 0)
    assert len(np.unique(tiles)) > 100
    fx = _fixture()["box200_C"]  # hits and misses
    cams = np.array([_camera(fx["camera"]), _camera(_fixture()["box200_A"]["camera"])], fmgi.CAMERA_DTYPE)
    got = fmgi.render_views(sc, cams, fx["width"], fx["height"], tiles_rgb=tiles, background=(7, 8, 9))
    _assert_equal(got, 0, fx["wall"], fx["texel"], fx["dist_bits"])
    first, s0 = _first_tile(sc)
    hit = got["wall"] >= 0
    assert hit[0].any() and (~hit[0]).any() and hit[1].all()
    w = got["wall"][hit]
    at = 3 * (first[w] + got["texel"][hit] - s0[w])
    exp = np.stack([tiles[at], tiles[at + 1], tiles[at + 2]], axis=-1)
    assert np.array_equal(got["rgb"][hit], exp), int((got["rgb"][hit] != exp).any(axis=-1).sum())
    assert np.all(got["rgb"][~hit] == np.array([7, 8, 9], np.uint8))
    with pytest.raises(fmgi.FmgiError, match="tiles_rgb"):  # rgb without tiles
        _lib.check(_call(sc, cams, 8, 8, rgb=True), "fmgi_render_views")
    with pytest.raises(fmgi.FmgiError):
        fmgi.render_views(sc, cams, 8, 8, tiles_rgb=tiles[:-3])


@pytest.mark.gpu
def test_gpu_render_view_tool(torch_cuda, tmp_path):
    """tools/render_view.py: texels in, PPM out, the pixels render_views gives for the same tiles"""
    sc = _scene("box8")
    rng = np.random.default_rng(5)
    tex = (10.0 ** rng.uniform(-3, 1, (sc.num_texels, 4))).astype(f32)
    np.save(tmp_path / "texels.npy", tex)
    ppm = tmp_path / "view.ppm"
    cam = dict(pos=(5, 4, 20), dir=(0, 0, -1), up=(0, 1, 0), pixel=0.1)  # from above: hits and misses
    flat = lambda v: [str(x) for x in v]  # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "render_view.py"), "box8", "--tile-size", "1",
                        "--texels", str(tmp_path / "texels.npy"), "--spa", "1000", "--pos", *flat(cam["pos"]),
                        "--dir", *flat(cam["dir"]), "--up", *flat(cam["up"]), "--pixel", "0.1", "--width", "16",
                        "--height", "12", "--background", "1", "2", "3", "-o", str(ppm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    blob = ppm.read_bytes()
    head = b"P6\n16 12\n255\n"
    assert blob.startswith(head) and len(blob) == len(head) + 16 * 12 * 3
    _, tiles = fmgi.output_tiles(sc, tex, 1000, 0)
    got = fmgi.render_views(sc, fmgi.camera(**cam), 16, 12, tiles_rgb=tiles, background=(1, 2, 3))
    assert (got["wall"] >= 0).any() and (got["wall"] < 0).any()
    assert blob[len(head):] == got["rgb"][0].tobytes()
