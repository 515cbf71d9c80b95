"""Lightmaps of chosen sizes on one small scene (tests/test_lightmap_sizes_host.py, tests/test_gpu_lightmap_sizes.py):
how the bake's deposit codes are folded into the int64 lightmap depends on P = ceil(numTexels / 2048), the count of
2048-texel fold tiles, and these scenes put P on both sides of every value at which it changes.

The scene is box_scene(8, tile_size=2.0, with_light=True): six rects, one window and one lamp, a verified lattice.
Only `lm` = {texel base, tiles along width, tiles along height} of its walls and its texel count are rewritten:
fmgi_set_scene asks no more of a wall than that its level 0 lies inside numTexels, so the bases need not be the
running mip-mapped sum, and numTexels is free.

  even(T)     T >= 384: every wall W x 64 tiles with W = (T // 6) // 64, wall i at base i * W * 64, the last wall
              at T - W * 64: its last level-0 texel is texel T - 1, and the six walls reach every fold tile.
              T < 384: W = T // 6, H = 1 (T = 6: one texel per wall, hundreds of thousands of deposits on texel 0)
  gapped(T)   six walls of 64 x 64 at bases 0, 2048 - 100, 63 * 2048 - 2000, 128 * 2048 - 7, 2^21 + 5 and T - 4096:
              a very large lightmap whose deposits fall in a handful of tiles (15 at T = 4,194,303), every other
              tile's run empty

Every scene is planned at SPA with the schedule of tests/golden/glibc_rand_4096.npy: 10,431,232 items, the lamp's
from 10,000,128 on. RANGES are the window's first 2048 items and the lamp's last 1024.
"""
import functools

import numpy as np

from fmgi import scene

TILE_TEXELS = 2048  # one fold tile (FMGI_TILE_BITS = 11)
SPA = 172_413_793
TOTAL_ITEMS = 10_431_232
LAMP_BEGIN = 10_000_128
RANGES = ((0, 2048), (TOTAL_ITEMS - 1024, TOTAL_ITEMS))
WINDOW_RANGE, LAMP_RANGE = RANGES

# numTexels: P
EVEN_SIZES = {6: 1, 2047: 1, 2048: 1, 2049: 2, 4096: 2, 4097: 3, 126_977: 63, 129_023: 63, 129_024: 63,
              129_025: 64, 131_072: 64, 262_144: 128, 262_145: 129}
BUCKET_MAX = 129_024      # 63 tiles (FMGI_PRESORT_MAX_TILES): the largest lightmap of the bucket layouts
STREAM_END = 4_194_304    # kStreamMaxTexels: from here on a STREAM request becomes FX3
GAPPED_SIZES = (STREAM_END - 1, STREAM_END)


def tiles_of(T):
    return (T + TILE_TEXELS - 1) // TILE_TEXELS


def _box():
    return scene.box_scene(8, tile_size=2.0, with_light=True)


def _with_lm(name, lms, T):
    box = _box()
    assert len(box.walls) == len(lms) == 6
    walls = box.walls.copy()
    for w, (base, s1, s2) in zip(walls, lms):
        assert 0 <= base and base + s1 * s2 <= T, (name, base, s1, s2)
        w["lm"][:] = (base, s1, s2, 0)
    return scene.Scene(name, walls, box.windows, box.lights, T)


def even_lm(T):
    """(base, tiles along width, tiles along height) of the six walls of even(T)"""
    if T < 6:
        raise ValueError("even(T) needs a texel per wall")
    H = 64 if T >= 384 else 1
    W = (T // 6) // H
    return [(i * W * H if i < 5 else T - W * H, W, H) for i in range(6)]


def gapped_lm(T):
    if T < (1 << 21) + 5 + 2 * 4096:
        raise ValueError("gapped(T) needs room behind 2^21 + 5")
    return [(b, 64, 64) for b in (0, 2048 - 100, 63 * 2048 - 2000, 128 * 2048 - 7, (1 << 21) + 5, T - 4096)]


@functools.lru_cache(None)
def even(T):
    """shared between tests, so treat it as read-only"""
    return _with_lm(f"even{T}", even_lm(T), T)


@functools.lru_cache(None)
def gapped(T):
    """shared between tests, so treat it as read-only"""
    return _with_lm(f"gapped{T}", gapped_lm(T), T)


def get(kind, T):
    return {"even": even, "gapped": gapped}[kind](T)


def touched_tiles(sc):
    """the fold tiles that hold a level-0 texel of a wall"""
    tiles = set()
    for w in sc.walls:
        b, n = int(w["lm"][0]), int(w["lm"][1]) * int(w["lm"][2])
        tiles.update(range(b // TILE_TEXELS, (b + n - 1) // TILE_TEXELS + 1))
    return sorted(tiles)
