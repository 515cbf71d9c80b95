"""The glossy floor of the views (fmgi_*_gloss) restated in float32 numpy.

No reference program exists for the mirror bounce: its definition (include/flatmatch_gi.h) is restated
here on test_view's vector helpers, intersects() and walk, on test_view_shade's taps and on view_proj_restate's
rays, lists and cases, every operation float32 in the stated order. test_view_gloss_host.py checks the
restatement's own conditions, test_gpu_view_gloss.py holds the GPU to it bit for bit.

  mirror_list(sc, pos)                every wall by (distance-to-pos bits, index): wall indices, keys
  trace(name, S, ...)                 both walks of a case, per sample; brute=True: the mirror walk without its break
  shade(name, S, bilinear, gloss)     fmgi_shade_views_gloss for one camera
  CASES                               the three pin-hole cases of test_view_shade and the six of view_proj_restate
"""
import functools

import numpy as np

import fmgi
import test_view as T
import test_view_shade as V
import view_proj_restate as P

f32 = np.float32
BG = V.BG
MIRROR_Z = f32(4.99999965541064739227294921875e-4)  # (double)z > 0.0005 in float32, as the bake has it
PINHOLE_CASES = list(V.CASES)
CASES = PINHOLE_CASES + list(P.SHADE_CASES)
OPEN_CASES = ("open_tilted_ortho", "open_tilted_equirect")
GLOSSES = (0.25, 0.3, 0.75, 1.0)


@functools.lru_cache(None)
def case(name):
    """(scene, camera, projection, width, height, tiles)"""
    if name in PINHOLE_CASES:
        return (V._scene(name), V._cam(name), "pinhole") + V.SIZES[name] + (V._tiles(name),)
    sc, cam, projection, w, h = P.case(name)
    return sc, cam, projection, w, h, P.tiles(name.rsplit("_", 1)[0])


def mirror_list(sc, pos):
    """every wall of the scene, no culls: getShortestDistanceRectToPoint (rectangle.c:442-473) to pos as the key,
    sorted by (key bits, wall index)"""
    W = sc.walls
    p, w, h, n = T._v(W["pos"]), T._v(W["width"]), T._v(W["height"]), T._v(W["n"])
    on_plane = T._sub(pos, T._mul(n, T._dot(T._sub(pos, p), n)))
    pd = T._sub(on_plane, p)
    u = T._dot(pd, T._normalized(h)) / T._length(h)
    v = T._dot(pd, T._normalized(w)) / T._length(w)
    u = np.where(u < 0, f32(0), np.where(u > 1, f32(1), u))
    v = np.where(v < 0, f32(0), np.where(v > 1, f32(1), v))
    md = T._length(T._sub(pos, T._add(T._add(p, T._mul(w, v)), T._mul(h, u)))).astype(f32)
    order = np.lexsort((np.arange(len(W)), md.view(np.uint32)))
    return order.astype(np.int32), md[order]


def pinhole_rays(cam, width, height, S_):
    """test_view_shade.shade's rays: (origins, directions) that broadcast to [S, S, H, W]"""
    cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
    pos, up, pixel = T._v(cam["pos"]), T._v(cam["up"]), f32(cam["pixel"])
    cam_dir = T._normalized(T._v(cam["dir"]))
    centre = T._add(pos, cam_dir)
    right = T._cross(cam_dir, up)
    offs = (2 * np.arange(S_) + 1 - S_).astype(f32) / f32(2 * S_)
    j, i, y, x = np.meshgrid(np.arange(S_), np.arange(S_), np.arange(height), np.arange(width), indexing="ij")
    fx = pixel * ((x - width // 2).astype(f32) + offs[i])
    fy = -pixel * ((y - height // 2).astype(f32) + offs[j])
    d = T._normalized(T._sub(T._add(T._add(centre, T._mul(right, fx)), T._mul(up, fy)), pos))
    return tuple(np.full(x.shape, c, f32) for c in pos), d


def mirror_walk(walls, mw, mk, Q, d2, base, brute=False):
    """the mirror walk for arrays of rays over one mirror list: (wall or -1, distance or inf, tests)"""
    shape = np.shape(base)
    best = np.full(shape, np.inf, f32)
    wall2 = np.full(shape, -1, np.int32)
    walking = np.ones(shape, bool)
    tests = 0
    for i, key in zip(mw, mk):
        if not brute:
            walking &= ~((base + best) < key)
            if not walking.any():
                break
        tests += int(walking.sum())
        dn = T._intersects(walls[i], Q, d2, best)
        take = walking & ~(dn < 0) & (dn <= best)
        wall2[take] = i
        best[take] = dn[take]
    return wall2, best, tests


def sample_walks(sc, cam, projection, width, height, S_, brute=False):
    """both walks of one camera. Per sample [S, S, H, W]: wall, dist, pt (the hit point; garbage on a miss) and
    mirror (bool); for the mirror samples, flat in C order: wall2, best, mpt (the mirror ray's hit point). tests is
    the primary walk's count, mirror_tests the second walk's."""
    with np.errstate(all="ignore"):
        cam = np.asarray(cam, fmgi.CAMERA_DTYPE).reshape(())
        pos = T._v(cam["pos"])
        if projection == "pinhole":
            cw, cd = T._candidates(sc, pos, T._normalized(T._v(cam["dir"])))
            src, d = pinhole_rays(cam, width, height, S_)
        else:
            cw, cd = P.candidates(sc, cam, projection)
            src, d = P.rays(cam, width, height, S_, projection)
        wall, dist, tests = T.walk(sc.walls, cw, cd, src, d)
        pt = T._add(src, T._mul(d, dist))
        mirror = (wall >= 0) & ~(pt[2] > MIRROR_Z)
        n = T._v(sc.walls["n"][wall[mirror]])
        dm = tuple(np.broadcast_to(c, wall.shape)[mirror] for c in d)
        pm = tuple(c[mirror] for c in pt)
        two = f32(2.0) * T._dot(n, dm)
        d2 = T._sub(dm, T._mul(n, two))  # not normalised again
        Q = T._add(pm, T._mul(d2, f32(1e-5)))
        base = T._length(T._sub(Q, pos))
        mw, mk = mirror_list(sc, pos)
        wall2, best, mtests = mirror_walk(sc.walls, mw, mk, Q, d2, base, brute)
        mpt = T._add(Q, T._mul(d2, np.where(wall2 >= 0, best, f32(0))))
        return {"wall": wall, "dist": dist, "pt": pt, "mirror": mirror, "wall2": wall2, "best": best, "mpt": mpt,
                "tests": tests, "mirror_tests": mtests, "list": (mw, mk)}


@functools.lru_cache(None)
def trace(name, S_, width=None, height=None, brute=False):
    sc, cam, projection, w, h, _ = case(name)
    if width:
        w, h = width, height
    return sample_walks(sc, cam, projection, w, h, S_, brute)


def taps(sc, tiles, wall, pt, bilinear, out):
    """out[k] = the colour (float32 [3], before the fixed-point step) of the hit on wall[k] at pt[k]: getTileIdAt's
    coordinates (rectangle.c:205-230) and test_view_shade's taps"""
    first = np.concatenate([[0], np.cumsum(V._tile_counts(sc))])
    texels = np.asarray(tiles, np.uint8).reshape(-1, 3)
    for k in np.unique(wall[wall >= 0]):
        m = wall == k
        r = sc.walls[k]
        w, h = T._v(r["width"]), T._v(r["height"])
        pdir = T._sub(tuple(c[m] for c in pt), T._v(r["pos"]))
        wl, hl = T._length(w), T._length(h)
        s1, s2 = int(r["lm"][1]), int(r["lm"][2])
        u = T._dot(T._mul(w, f32(1.0) / wl), pdir) * f32(s1) / wl
        v = T._dot(T._mul(h, f32(1.0) / hl), pdir) * f32(s2) / hl
        tw = texels[first[k]:first[k + 1]].reshape(s2, s1, 3).astype(f32)
        if not bilinear:
            out[m] = tw[np.clip(T._x86_int(v), 0, s2 - 1), np.clip(T._x86_int(u), 0, s1 - 1)]
            continue
        xa, xb, fu, _ = V._axis(u, s1)
        ya, yb, fv, _ = V._axis(v, s2)
        one, fu, fv = f32(1), fu[:, None], fv[:, None]
        top = (one - fu) * tw[ya, xa] + fu * tw[ya, xb]
        bot = (one - fu) * tw[yb, xa] + fu * tw[yb, xb]
        out[m] = (one - fv) * top + fv * bot


def colour(sc, tr, tiles, bg, S_, bilinear, gloss):
    """the pictures of one traced camera: dict of rgb and coverage (int64), tests (both walks), mirror_rays,
    mirror_hits, mirror_tests, and val / mval, the primary and mirror colours per sample"""
    with np.errstate(all="ignore"):
        g = f32(gloss)
        wall, mirror = tr["wall"], tr["mirror"]
        val = np.empty(wall.shape + (3,), f32)
        val[...] = np.asarray(bg, f32)
        taps(sc, tiles, wall, tr["pt"], bilinear, val)
        mval = np.empty(tr["wall2"].shape + (3,), f32)
        mval[...] = np.asarray(bg, f32)
        taps(sc, tiles, tr["wall2"], tr["mpt"], bilinear, mval)
        out = val.copy()
        if g > 0:  # gloss == 0 is the call without the bounce
            out[mirror] = (f32(1.0) - g) * val[mirror] + g * mval
        q = (out * f32(256.0) + f32(0.5)).astype(np.int64)
        rgb = (q.sum(axis=(0, 1)) + 128 * S_ * S_) // (256 * S_ * S_)
        on = g > 0
        return {"rgb": rgb, "coverage": (wall >= 0).sum(axis=(0, 1)),
                "tests": tr["tests"] + (tr["mirror_tests"] if on else 0),
                "mirror_rays": int(mirror.sum()) if on else 0,
                "mirror_hits": int((tr["wall2"] >= 0).sum()) if on else 0,
                "mirror_tests": tr["mirror_tests"] if on else 0, "val": val, "mval": mval}


def shade(name, S_, bilinear, gloss, width=None, height=None, brute=False, tiles=None, bg=BG):
    sc, _, _, _, _, own = case(name)
    return colour(sc, trace(name, S_, width, height, brute), own if tiles is None else tiles, bg, S_, bilinear, gloss)


def shade_camera(sc, cam, projection, width, height, tiles, bg, S_, bilinear, gloss):
    """shade for a camera that is not one of the cases"""
    return colour(sc, sample_walks(sc, cam, projection, width, height, S_), tiles, bg, S_, bilinear, gloss)
