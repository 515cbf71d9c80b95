"""Shared by test_filter_host.py and test_gpu_filter.py: the adaptive density filter's definition
(include/flatmatch_gi.h) restated twice, from the text and not from the kernels.

  * radii_exact / apply_exact: the definition word for word in Python integers, every window summed texel by
    texel (for the hand-computed cases and small random walls);
  * radii / apply: the same in numpy uint64, whose arithmetic is mod 2^64 like the definition's. A window sum
    is built from shifted copies of the wall's grid (a texel outside the wall contributes nothing, which is the
    clipping of the window), never from prefix sums.

Grid and windows: wall w has lightmapSetup {s0, s1, s2, 0}; its level-0 texel (x, y) is s0 + y * s1 + x;
W_r(x, y) = [max(x - r, 0), min(x + r, s1 - 1)] x [max(y - r, 0), min(y + r, s2 - 1)].
"""
import numpy as np

M64 = (1 << 64) - 1
MAX_RADIUS = 16
u64 = np.uint64


def grids(sc):
    """[(s0, s1, s2)] of the scene's walls"""
    return [(int(w["lm"][0]), int(w["lm"][1]), int(w["lm"][2])) for w in sc.walls]


# ---- word for word, Python integers ----------------------------------------------------------------------------

def _window(x, y, r, s1, s2):
    return [(xx, yy) for yy in range(max(y - r, 0), min(y + r, s2 - 1) + 1)
            for xx in range(max(x - r, 0), min(x + r, s1 - 1) + 1)]


def radii_exact(walls, num_texels, guide, min_energy, max_radius):
    """guide: [num_texels][>= 3] integers; returns a list of num_texels radii"""
    e = [(int(g[0]) + int(g[1]) + int(g[2])) & M64 for g in guide]
    out = [0] * num_texels
    for s0, s1, s2 in walls:
        for y in range(s2):
            for x in range(s1):
                rad = max_radius
                for r in range(max_radius + 1):
                    s = sum(e[s0 + yy * s1 + xx] for xx, yy in _window(x, y, r, s1, s2)) & M64
                    if s >= min_energy:
                        rad = r
                        break
                out[s0 + y * s1 + x] = rad
    return out


def apply_exact(walls, lm, radii):
    """lm: [num_texels][4] integers (taken mod 2^64); returns a list of [4] lists of unsigned integers"""
    out = [[int(v) & M64 for v in px] for px in lm]
    src = [list(px) for px in out]
    for s0, s1, s2 in walls:
        for y in range(s2):
            for x in range(s1):
                t = s0 + y * s1 + x
                win = _window(x, y, min(int(radii[t]), MAX_RADIUS), s1, s2)
                for c in range(3):
                    out[t][c] = (sum(src[s0 + yy * s1 + xx][c] for xx, yy in win) & M64) // len(win)
    return out


# ---- numpy uint64 ------------------------------------------------------------------------------------------------

def _box(a, r):
    """window sums of radius r of the grid a (uint64 [s2, s1]), windows clipped to the grid; mod 2^64"""
    s2, s1 = a.shape
    h = a.copy()
    for d in range(1, min(r, s1 - 1) + 1):
        h[:, d:] += a[:, :-d]
        h[:, :-d] += a[:, d:]
    v = h.copy()
    for d in range(1, min(r, s2 - 1) + 1):
        v[d:] += h[:-d]
        v[:-d] += h[d:]
    return v


def radii(sc, guide, min_energy, max_radius):
    """uint8 [num_texels]; guide: 64-bit integers [num_texels, >= 3]"""
    g = np.ascontiguousarray(guide).view(u64) if guide.dtype != u64 else guide
    e = g[:, 0] + g[:, 1] + g[:, 2]
    out = np.zeros(sc.num_texels, np.uint8)
    for s0, s1, s2 in grids(sc):
        grid = e[s0 : s0 + s1 * s2].reshape(s2, s1)
        rad = np.full((s2, s1), max_radius, np.uint8)
        todo = np.ones((s2, s1), bool)
        for r in range(max_radius + 1):
            hit = todo & (_box(grid, r) >= u64(min_energy))
            rad[hit] = r
            todo &= ~hit
            if not todo.any():
                break
        out[s0 : s0 + s1 * s2] = rad.reshape(-1)
    return out


def apply(sc, lm, rad):
    """lm: 64-bit integers [num_texels, 3 or 4]; returns the filtered copy (same dtype and shape)"""
    src = np.ascontiguousarray(lm).view(u64)
    out = src.copy()
    for s0, s1, s2 in grids(sc):
        rr = np.minimum(rad[s0 : s0 + s1 * s2].reshape(s2, s1), MAX_RADIUS)
        for r in np.unique(rr).tolist():
            sel = (rr == r).reshape(-1)
            n = _box(np.ones((s2, s1), u64), r).reshape(-1)
            for c in range(3):
                s = _box(src[s0 : s0 + s1 * s2, c].reshape(s2, s1), r).reshape(-1)
                out[s0 : s0 + s1 * s2, c][sel] = s[sel] // n[sel]
    return out.view(lm.dtype)


# ---- the quality metric -------------------------------------------------------------------------------------------

def density_scale(sc):
    """float64 [num_texels]: s1 * s2 / (|width| * |height|) on a wall's level-0 texels, 0 elsewhere"""
    k = np.zeros(sc.num_texels)
    for w, (s0, s1, s2) in zip(sc.walls, grids(sc)):
        area = np.linalg.norm(w["width"][:3].astype(np.float64)) * np.linalg.norm(w["height"][:3].astype(np.float64))
        k[s0 : s0 + s1 * s2] = s1 * s2 / area
    return k


def l1_pair(sc, low, low_filtered, ref):
    """(L1 unfiltered, L1 filtered) of a low-photon lightmap and its filtered version against a reference bake:
    every level-0 texel scaled by density_scale, the low bake rescaled once so that its unfiltered sum equals
    the reference's; L1 = sum |v - v_ref| / sum v_ref over the level-0 texels and the three channels."""
    k = density_scale(sc)[:, None]
    a, b, r = (np.asarray(v)[:, :3].astype(np.float64) * k for v in (low, low_filtered, ref))
    gain = r.sum() / a.sum()
    return float(np.abs(gain * a - r).sum() / r.sum()), float(np.abs(gain * b - r).sum() / r.sum())
