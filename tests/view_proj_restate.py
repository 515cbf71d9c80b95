"""The orthographic and equirectangular cameras (fmgi_*_proj) restated in float32 numpy.

No reference program exists for the two projections: their definition (include/flatmatch_gi.h) is
restated here on test_view's vector helpers, intersects() and walk, and on test_view_shade's tap code, every
operation float32 in the stated order. Sines and cosines come from the oracle's own restatement of the device
library (fm_oracle.sincos), not from the product. test_view_proj_host.py checks the restatement's own
conditions, test_gpu_view_proj.py holds the GPU to it bit for bit.

  frame(cam)                          pos, f, r, u
  candidates(sc, cam, projection)     the projection's sorted list: wall indices, keys
  rays(cam, W, H, S, projection)      per-sample origins and directions, [S (j), S (i), H, W]
  shade(...)                          fmgi_shade_views_proj for one camera; brute=True walks without the early break
  CASES                               the scenes, cameras and image sizes both test files use
"""
import functools

import numpy as np

import fm_oracle as O
import fmgi
import offaxis_scenes as S
import test_view as T
import test_view_shade as V

f32 = np.float32
BG = V.BG
PROJECTIONS = ("ortho", "equirect")


def frame(cam):
    """the camera frame of the two projections, as the host computes it"""
    cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
    pos, up = T._v(cam["pos"]), T._v(cam["up"])
    f = T._normalized(T._v(cam["dir"]))
    r = T._normalized(T._cross(f, up))
    return pos, f, r, T._cross(r, f)


def _min(a, b):
    return np.where(a < b, a, b)


def candidates(sc, cam, projection):
    """(wall indices int32, keys float32) in the order the rays walk them: sorted by (key bits, wall index)"""
    with np.errstate(all="ignore"):
        pos, f, _, _ = frame(cam)
        if projection == "equirect":
            # the pin-hole's list without isBehindRay: against a zero direction no corner's dot is < 0
            return T._candidates(sc, pos, (f32(0), f32(0), f32(0)))
        W = sc.walls
        p, w, h, n = T._v(W["pos"]), T._v(W["width"]), T._v(W["height"]), T._v(W["n"])
        e = [T._dot(T._sub(c, pos), f) for c in (p, T._add(p, w), T._add(p, h), T._add(T._add(p, w), h))]
        behind = (e[0] < 0) & (e[1] < 0) & (e[2] < 0) & (e[3] < 0)
        m = _min(_min(e[0], e[1]), _min(e[2], e[3]))
        key = np.where(m < 0, f32(0), m).astype(f32)
        keep = np.flatnonzero((T._dot(n, f) < 0) & ~behind)
        order = keep[np.lexsort((keep, key[keep].view(np.uint32)))]
        return order.astype(np.int32), key[order]


def _sincos(x):
    s, c = O.sincos(np.ascontiguousarray(x, f32).reshape(-1))
    return s.reshape(x.shape), c.reshape(x.shape)


def rays(cam, width, height, S_, projection):
    """(origins, directions) of every sample: tuples of three float32 arrays that broadcast to [S, S, H, W]"""
    cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
    pos, f, r, u = frame(cam)
    offs = (2 * np.arange(S_) + 1 - S_).astype(f32) / f32(2 * S_)
    j, i, y, x = np.meshgrid(np.arange(S_), np.arange(S_), np.arange(height), np.arange(width), indexing="ij")
    shape = x.shape
    if projection == "ortho":
        pixel = f32(cam["pixel"])
        fx = pixel * ((x - width // 2).astype(f32) + offs[i])
        fy = -pixel * ((y - height // 2).astype(f32) + offs[j])
        src = T._add(T._add(pos, T._mul(r, fx)), T._mul(u, fy))
        return src, tuple(np.full(shape, c, f32) for c in f)
    kphi, ktheta = f32(6.2831855) / f32(width), f32(3.1415927) / f32(height)
    phi = (x.astype(f32) + (f32(0.5) + offs[i])) * kphi
    theta = (y.astype(f32) + (f32(0.5) + offs[j])) * ktheta
    assert 0 < phi.min() and phi.max() < 2 * np.pi and 0 < theta.min() and theta.max() < np.pi
    (sp, cp), (st, ct) = _sincos(phi), _sincos(theta)
    a, b, c = (-cp) * st, (-sp) * st, ct
    d = T._normalized(T._add(T._add(T._mul(f, a), T._mul(r, b)), T._mul(u, c)))
    return tuple(np.full(shape, p, f32) for p in pos), d


def walk_brute(walls, cw, src, d):
    """T.walk over the same list without the early break: (wall, distance)"""
    shape = np.shape(d[0])
    dist = np.full(shape, np.inf, f32)
    wall = np.full(shape, -1, np.int32)
    for i in cw:
        dn = T._intersects(walls[i], src, d, dist)
        take = ~(dn < 0) & (dn <= dist)
        wall[take] = i
        dist[take] = dn[take]
    return wall, dist


def shade(sc, cam, width, height, tiles, bg, S_, bilinear, projection, brute=False):
    """fmgi_shade_views_proj for one camera: test_view_shade.shade's taps and resolve on the projection's rays.
    dict of rgb and coverage (int64), tests, and per sample wall, dist and tile (the nearest tile's index in its
    wall's grid, -1 for a miss)"""
    with np.errstate(all="ignore"):
        cw, cd = candidates(sc, cam, projection)
        src, d = rays(cam, width, height, S_, projection)
        if brute:
            (wall, dist), tests = walk_brute(sc.walls, cw, src, d), None
        else:
            wall, dist, tests = T.walk(sc.walls, cw, cd, src, d)
        hit_pt = T._add(src, T._mul(d, np.where(wall >= 0, dist, f32(0))))
        val = np.empty(wall.shape + (3,), f32)
        val[...] = np.asarray(bg, f32)
        tile = np.full(wall.shape, -1, np.int64)
        first = np.concatenate([[0], np.cumsum(V._tile_counts(sc))])
        texels = np.asarray(tiles, np.uint8).reshape(-1, 3)
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
            ty, tx = np.clip(T._x86_int(v), 0, s2 - 1), np.clip(T._x86_int(u), 0, s1 - 1)
            tile[m] = ty * s1 + tx
            if not bilinear:
                val[m] = tw[ty, tx]
                continue
            xa, xb, fu, _ = V._axis(u, s1)
            ya, yb, fv, _ = V._axis(v, s2)
            one, fu, fv = f32(1), fu[:, None], fv[:, None]
            top = (one - fu) * tw[ya, xa] + fu * tw[ya, xb]
            bot = (one - fu) * tw[yb, xa] + fu * tw[yb, xb]
            val[m] = (one - fv) * top + fv * bot
        q = (val * f32(256.0) + f32(0.5)).astype(np.int64)
        rgb = (q.sum(axis=(0, 1)) + 128 * S_ * S_) // (256 * S_ * S_)
        return {"rgb": rgb, "coverage": (wall >= 0).sum(axis=(0, 1)), "tests": tests, "wall": wall, "dist": dist,
                "tile": tile}


# ---- the cases of both test files ----------------------------------------------------------------------------

EXAMPLE_POS = (5, 5.2, 1.6)  # the reference tool's camera position and direction (debugRaytracer.cc:121-123)
EXAMPLE_DIR = (1, 1, 0)


@functools.lru_cache(None)
def scene(name):
    if name in ("box8", "example"):
        return T._scene(name)
    if name == "floor":  # box200's floor alone: open to every side, and nothing to see from below
        from fmgi import scene as fs

        walls = T._scene("box200").walls[:36].copy()
        return fs.Scene("floor", walls, T._scene("box200").windows, T._scene("box200").lights, fs.assign_texel_bases(walls))
    return S.get(name)


def plan_camera(sc, width, height):
    """top-down over the whole scene: above the highest corner, x to the right, y up, 2 % of margin"""
    W = sc.walls
    pts = np.concatenate([W["pos"], W["pos"] + W["width"], W["pos"] + W["height"],
                          W["pos"] + W["width"] + W["height"]])[:, :3].astype(np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pixel = 1.02 * max((hi[0] - lo[0]) / width, (hi[1] - lo[1]) / height)
    return fmgi.camera(((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[2] + 1.0), (0, 0, -1), (0, 1, 0), pixel)


@functools.lru_cache(None)
def case(name):
    """(scene, camera, projection, width, height)"""
    sname, projection = name.rsplit("_", 1)
    sc = scene(sname)
    w, h = {"box8": (24, 20), "example": (40, 20) if projection == "equirect" else (40, 30), "open_tilted": (32, 16),
            "tilted56": (32, 16), "tilted57": (32, 16)}[sname]
    if projection == "ortho":
        if sname == "open_tilted":  # no ceiling: a slanted look into the box from above, walls and panels in sight
            cam = fmgi.camera((3.5, 2.5, 6.0), (0.25, 0.2, -1), (0, 1, 0), 0.36)
        else:
            cam = plan_camera(sc, w, h)
    elif sname == "example":
        cam = fmgi.camera(EXAMPLE_POS, EXAMPLE_DIR, (0, 0, 1), 1.0)
    elif sname == "box8":
        cam = fmgi.camera((5, 4, 1.3), (1, 0.5, -0.1), (0, 0, 1), 1.0)  # test_view's camera A, inside the box
    else:
        cam = fmgi.camera((4.1, 3.3, 1.2), (1, 0.4, 0.2), (0, 0, 1), 1.0)
    return sc, cam, projection, w, h


SHADE_CASES = [f"{s}_{p}" for s in ("box8", "example", "open_tilted") for p in PROJECTIONS]
LIST_CASES = SHADE_CASES + [f"{s}_{p}" for s in ("tilted56", "tilted57") for p in PROJECTIONS]
# the batch of four on the floor scene; camera 1 is below the floor looking down and its list is empty (ORTHO: every
# wall lies behind the screen plane; EQUIRECT: every wall shows the point its back)
EMPTY_CAM = fmgi.camera((5, 4, -3.0), (0, 0, -1), (0, 1, 0), 0.5)
BATCH_CAMS = np.array([fmgi.camera((5, 4, 3.0), (0, 0, -1), (0, 1, 0), 0.5), EMPTY_CAM,
                       fmgi.camera((2, 7, 1.0), (1, -0.5, -0.4), (0, 0, 1), 0.45),
                       fmgi.camera((11, 4, 5.0), (-0.6, 0.1, -1), (0, 1, 0), 0.6)], fmgi.CAMERA_DTYPE)
BATCH_SIZE = (24, 20)


def window_cams(proj):
    """the two box8 cameras of the windowed launches: the case's own and a second one"""
    other = fmgi.camera((2, 6, 1.9 if proj == "equirect" else 4.0), (0.3, -1, -0.5), (0, 0, 1), 0.3)
    return np.array([case(f"box8_{proj}")[1], other], fmgi.CAMERA_DTYPE)


WINDOW_SIZE = (50, 37)


@functools.lru_cache(None)
def tiles(sname, k=0):
    """random RGB8 tiles in wall order; set 0 of box8 and example is test_view_shade's"""
    n = 3 * int(V._tile_counts(scene(sname)).sum())
    return np.random.default_rng(5 + k).integers(0, 256, n, dtype=np.uint8)


@functools.lru_cache(None)
def restated(name, S_, bilinear, width=None, height=None, brute=False, k=0):
    sc, cam, projection, w, h = case(name)
    if width:
        w, h = width, height
    return shade(sc, cam, w, h, tiles(name.rsplit("_", 1)[0], k), BG, S_, bilinear, projection, brute)
