"""Direct sunlight through windows (fmgi_sun_*) restated in float32 numpy.

No reference program has a sun: its definition (include/flatmatch_gi.h, "Direct sunlight through windows") is restated
here on test_view's vector helpers and intersects(), every operation float32 in the stated order, brute force over
every wall: no lists, no culls, no early exit. test_sun_host.py checks the restatement's own conditions and the host
calls, test_gpu_sun.py holds the GPU to it byte for byte.

  NAMES, case(name)          the cases: (scene, to_sun); POSITIVE, ZERO and SAMPLES say what each is for
  restate(name, S)           {"cover": uint8 [numTexels], "samples", "facing", "crossing", "lit"}; cached
  coverage(sc, to_sun, S)    the same for any scene and direction
  units(sc, to_sun, rgb, flux)   int64 [numWalls, 3]: a fully lit texel's deposit, zero rows for walls that do not face
  add(sc, cover, to_sun, S, rgb, flux, lm)   fmgi_sun_add on an int64 [numTexels, 4] lightmap, a copy
  finalize(sc, lm, spa)      fmgi_finalize on zero texels, then main.c:68-79's normalisation: float32 [numTexels, 3]
"""
import functools
import os

import numpy as np

import emitter_scenes
import offaxis_scenes
import test_view as T
from conftest import GOLDEN
from fmgi import scene

f32 = np.float32
INF = f32(np.inf)
DIR = (0.3, -1.0, 0.8)  # late morning on a south window (+y is north)
LOW = (0.2, -1.0, 0.35)  # a lower sun that reaches the panels of the tilted scenes


def _ragged_scene():
    """box8 with a 0.2 m panel of 1 x 1 tiles facing up as wall 0: with DIR its level-0 texels are the first job,
    and the facing walls' texel count is no multiple of 7 or 16, so the last wave of S = 3 and S = 2 is ragged"""
    box = scene.box_scene(8, tile_size=20.0)
    panel = scene.create_rectangle(4.2, 1.0, 0.3, -0.2, 0, 0, 0, 0.2, 0, 0.0)
    walls = np.concatenate([np.array([panel], scene.RECT_DTYPE), box.walls]).copy()
    return scene.Scene("ragged", walls, box.windows, box.lights, scene.assign_texel_bases(walls))


@functools.lru_cache(None)
def _scene(key):
    if key == "box8":
        return scene.box_scene(8, tile_size=20.0)
    if key == "ragged":
        return _ragged_scene()
    if key == "example":
        return scene.load_geometry(os.path.join(GOLDEN, "example_geometry.bin"), "example")
    if key in offaxis_scenes.NAMES:
        return offaxis_scenes.get(key)
    return emitter_scenes.get(key)


# name -> (scene key, to_sun)
_CASES = {
    "box": ("box8", DIR),                              # a patch on the floor
    "box_skew": ("box8", (-2.0, -1.0, 0.8)),           # ... that runs up the x = 10 side
    "box_behind": ("box8", (0.3, 1.0, 0.8)),           # the sun behind the window wall: all zero
    "box_level": ("box8", (0.0, -1.0, 0.0)),           # the floor's c_w is exactly 0: `> 0` decides
    "box_zenith": ("box8", (0.0, 0.0, 1.0)),           # dot(n_window, s) = 0: no crossing
    "box_grazing": ("box8", (0.0, -0.9998477, 0.017452406)),  # 1 degree of elevation
    "crossing": ("crossing", DIR),                     # interior partitions block
    "tilted12": ("tilted12", LOW),                     # off-axis occluders and receivers: panels block and are lit
    "open_tilted": ("open_tilted", LOW),               # ... without a ceiling
    "skylight": ("skylight", (0.05, 0.1, 1.0)),        # a window in the ceiling, the sun overhead
    "outside": ("outside", DIR),                       # a window outside the walls: crossed only after a wall
    "example": ("example", (-0.5, -1.0, 0.7)),         # 172 walls, 7 windows, reveals; an afternoon
    "ragged": ("ragged", DIR),
}
NAMES = tuple(_CASES)
POSITIVE = ("box", "box_skew", "box_grazing", "crossing", "tilted12", "open_tilted", "skylight", "example", "ragged")
ZERO = ("box_behind", "box_zenith")  # no sample crosses a window
SAMPLES = {name: ((1, 2) if name == "example" else (1, 2, 3, 8)) for name in NAMES}


def case(name):
    """(scene, to_sun as float32 [3])"""
    key, d = _CASES[name]
    return _scene(key), np.array(d, f32)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sun_dir(to_sun):
    x, y, z = (f32(v) for v in to_sun)
    l = np.sqrt((x * x + y * y) + z * z)
    return x / l, y / l, z / l


def facing_cos(sc, to_sun):
    """c_w of every wall, float32 [numWalls]"""
    return dot(T._v(sc.walls["n"]), sun_dir(to_sun)).astype(f32)


def coverage(sc, to_sun, S):
    with np.errstate(all="ignore"):
        s = sun_dir(to_sun)
        cover = np.zeros(sc.num_texels, np.uint8)
        out = {"samples": 0, "facing": 0, "crossing": 0, "lit": 0}
        c = facing_cos(sc, to_sun)
        i = np.arange(S)
        frac = (2 * i + 1).astype(f32) / f32(2 * S)
        for k, w in enumerate(sc.walls):
            s0, s1, s2 = (int(v) for v in w["lm"][:3])
            out["samples"] += s1 * s2 * S * S
            if not c[k] > 0:
                continue
            out["facing"] += s1 * s2 * S * S
            ty, tx, sj, si = np.meshgrid(np.arange(s2), np.arange(s1), i, i, indexing="ij")
            a = (tx.astype(f32) + frac[si]) / f32(s1)
            b = (ty.astype(f32) + frac[sj]) / f32(s2)
            P = T._add(T._add(T._v(w["pos"]), T._mul(T._v(w["width"]), a)), T._mul(T._v(w["height"]), b))
            Q = T._add(P, T._mul(s, f32(1e-5)))
            dw = np.full(a.shape, INF, f32)
            found = np.zeros(a.shape, bool)
            for win in sc.windows:  # the window as the scene holds it: its normal points into the room
                d = T._intersects(win, Q, s, INF)
                hit = d != f32(-1)
                better = hit & (~found | (d < dw))
                dw = np.where(better, d, dw)
                found |= hit
            # occlusion matters for the crossing samples only; every wall of the scene is tested
            Qf = tuple(q[found] for q in Q)
            dwf = dw[found]
            blocked = np.zeros(dwf.shape, bool)
            for r in sc.walls:
                blocked |= T._intersects(r, Qf, s, dwf) != f32(-1)
            lit = np.zeros(a.shape, bool)
            lit[found] = ~blocked
            cover[s0:s0 + s1 * s2] = lit.sum(axis=(2, 3)).reshape(-1)
            out["crossing"] += int(found.sum())
            out["lit"] += int(lit.sum())
        out["cover"] = cover
        return out


@functools.lru_cache(None)
def restate(name, S):
    sc, to_sun = case(name)
    return coverage(sc, to_sun, S)


def units(sc, to_sun, rgb, flux):
    c = facing_cos(sc, to_sun)
    out = np.zeros((len(sc.walls), 3), np.int64)
    for k, w in enumerate(sc.walls):
        if not c[k] > 0:
            continue
        wl, hl = T._length(T._v(w["width"])), T._length(T._v(w["height"]))
        area_t = (float(wl) * float(hl)) / float(int(w["lm"][1]) * int(w["lm"][2]))
        for ch in range(3):
            out[k, ch] = int(np.floor(np.ldexp(float(f32(rgb[ch])) * float(c[k]) * float(flux) * area_t, 25)))
    return out


def add(sc, cover, to_sun, S, rgb, flux, lm):
    """lm + the sun's deposits: int64 [numTexels, 4], word 3 untouched"""
    u = units(sc, to_sun, rgb, flux)
    c = facing_cos(sc, to_sun)
    out = np.array(lm, np.int64, copy=True)
    for k, w in enumerate(sc.walls):
        if not c[k] > 0:
            continue
        s0, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        cv = cover[s0:s0 + n].astype(np.int64)[:, None]
        out[s0:s0 + n, :3] += (cv * u[k][None, :] + (S * S) // 2) // (S * S)
    return out


def finalize(sc, lm, spa):
    """k_finalize on zero texels ((float)((double)0 + (double)q * 2^-25)), then the output step's level-0 scale
    (float)(0.35 * (tiles / (area * spa))) with area = |width| * |height| and the quotient in float32"""
    tex = (np.asarray(lm, np.int64)[:, :3].astype(np.float64) * 2.0 ** -25).astype(f32)
    for w in sc.walls:
        s0, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        area = T._length(T._v(w["width"])) * T._length(T._v(w["height"]))
        per = f32(n) / (area * f32(spa))
        tex[s0:s0 + n] *= f32(0.35 * float(per))
    return tex
