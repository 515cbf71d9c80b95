"""Bounced sunlight (fmgi_rad_cache_sun_bounce / fmgi_sun_add_bounced) restated in numpy from the
definition in include/flatmatch_gi.h ("Bounced sunlight"), not from the kernels. The gather is float32, one Python step
per ray in ray order, vectorised over jobs and directions as rad_solve_restate.py does it; the add is float64. The
scenes, seeds and form factors are rad_cache_cases'; the coverage maps and cosines are sun_restate's.

  CASES, case(name)                     (rad_cache_cases scene name, to_sun); POSITIVE and ZERO say what each is for
  cover(name, S)                        sun_restate.coverage of the case: uint8 [numTexels]; cached
  start_table(sc, cover, to_sun, S)     e_0: float32 [texels incl. the emitters']
  bounce(sc, sids, covers, to_suns, samples, N)   float32 [K, N, numTexels]: rows g_1 .. g_N per direction
  add(sc, g, rgb, refl, flux, lm)       fmgi_sun_add_bounced on an int64 [numTexels, 4] lightmap, a copy
  bound(sc, bounces, flux)              the value that must stay below 2^55
"""
import functools

import numpy as np

import rad_cache_cases as C
import rad_solve_restate as R
import sun_restate as SR
import test_view as T

f32 = np.float32
RAYS = f32(10000.0)

# name -> (rad_cache_cases scene, to_sun)
CASES = {
    "box_lit": ("box_lit", SR.DIR),                   # a patch on the floor
    "box_lit_skew": ("box_lit", (-2.0, -1.0, 0.8)),   # ... that runs up the x = 10 side
    "open_tilted": ("open_tilted", SR.LOW),           # panels, no ceiling: 43 % of the rays miss
    "box_lit_behind": ("box_lit", (0.3, 1.0, 0.8)),   # the sun behind the window wall: all zero
}
POSITIVE = ("box_lit", "box_lit_skew", "open_tilted")
ZERO = ("box_lit_behind",)
SAMPLES = (1, 2, 3, 8)


def case(name):
    """(rad_cache_cases name, scene, to_sun as float32 [3])"""
    key, d = CASES[name]
    return key, C.get_scene(key), np.array(d, f32)


@functools.lru_cache(None)
def cover(name, S):
    _, sc, to_sun = case(name)
    out = SR.coverage(sc, to_sun, S)["cover"]
    out.setflags(write=False)
    return out


def start_table(sc, cover, to_sun, S):
    """e_0[t] = ((float)cover[t] * c_w) / (float)(S * S) on the level-0 texels of the walls with c_w > 0, else +0"""
    _, ntex = R.layout(sc)
    e = np.zeros(ntex, f32)
    c = SR.facing_cos(sc, to_sun)
    for k, w in enumerate(sc.walls):
        if not c[k] > 0:
            continue
        s0, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        e[s0:s0 + n] = (np.asarray(cover[s0:s0 + n]).astype(f32) * c[k]) / f32(S * S)
    assert e.dtype == f32
    return e


def gather(sc, sids, e0, bounces):
    """e0 float32 [texels, K] -> float32 [K, bounces, numTexels]"""
    jobs = R.job_texels(sc)
    sids = np.asarray(sids)
    assert sids.shape == (len(jobs), R.RAYS)
    nt = int(sc.num_texels)
    cols = np.ascontiguousarray(sids.T)
    e = np.ascontiguousarray(e0, f32)
    out = np.zeros((e.shape[1], bounces, nt), f32)
    for n in range(bounces):
        acc = np.zeros((len(jobs), e.shape[1]), f32)
        for ray in range(R.RAYS):
            ids = cols[ray]
            hit = (ids >= 0) & (ids < nt)
            acc = np.where(hit[:, None], acc + e[np.where(hit, ids, 0)], acc)
        g = np.zeros_like(e)
        g[jobs] = acc / RAYS
        assert g.dtype == f32
        out[:, n] = g[:nt].T
        e = g
    return out


def bounce(sc, sids, covers, to_suns, samples, bounces):
    e0 = np.stack([start_table(sc, c, d, int(S)) for c, d, S in zip(covers, to_suns, samples)], axis=1)
    return gather(sc, sids, e0, bounces)


def area_t(w):
    wl, hl = T._length(T._v(w["width"])), T._length(T._v(w["height"]))
    return (float(wl) * float(hl)) / float(int(w["lm"][1]) * int(w["lm"][2]))


def add(sc, g, rgb, refl, flux, lm):
    """lm + the bounced deposits of g float32 [N, numTexels]: int64 [numTexels, 4], word 3 and mip texels untouched"""
    out = np.array(lm, np.int64, copy=True)
    g = np.asarray(g, f32)
    for w in sc.walls:
        s0, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        gw = g[:, s0:s0 + n].astype(np.float64)
        a = area_t(w)
        for ch in range(3):
            r = float(f32(refl[ch]))
            p, v = r, np.zeros(n, np.float64)
            for k in range(g.shape[0]):
                v = v + gw[k] * p
                p = p * r
            q = np.floor(np.ldexp(((float(f32(rgb[ch])) * v) * float(flux)) * a, 25)).astype(np.int64)
            out[s0:s0 + n, ch] += q
    return out


def bound(sc, bounces, flux):
    """32 * bounces * 1.001 * flux * max area_t * 2^25"""
    return float(np.ldexp(32.0 * float(bounces) * 1.001 * float(flux) * max((area_t(w) for w in sc.walls), default=0.0), 25))
