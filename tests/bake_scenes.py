"""Scenes on which the bake's scans take paths the boxes and layouts never reach (tests/test_bake_scenes_host.py,
tests/test_gpu_bake_scenes.py, tests/golden/make_ref_fixtures.py). All at 2 texels/m², baked at SPA with the schedule
of tests/golden/glibc_rand_4096.npy (10,000,128 items each).

  open_box       box200 without its ceiling (walls 36..71): one plane slot per axis, so the closed-box instances and
                 the wave-locked loop run it, with one (axis, class) list empty and 98 % of the photons escaping
  open_tilted, tilted1, tilted12, tilted57, crossing
                 tests/offaxis_scenes.py: one plane slot per axis plus a `general` list (the Axes phase 1 without
                 staging, then the exact general loop); crossing has two slots on x and y (the sorted phase 1)
  stacked3       box8 plus 3 exact copies of wall rect 3: every hit on the stack is a tie of 4 candidates that
                 the reference's index-order scan with its strict `d < closest` gives to rect 3, neither the first
                 nor the last rect of the scene
  stacked14      box8 plus 14 exact copies of the floor (rect 0): 15 candidates per hit, more than ordered_exact's
                 rounds, so every hit on the stack ends in the literal scan
  stacked14_200  box200 plus 14 copies of the interior floor rect 14: the same on the staged tables' overflow records
"""
import functools

import numpy as np

import offaxis_scenes
from fmgi import scene

TILE = 2.0
SPA = 172_413_793
OFFAXIS = ("open_tilted", "tilted1", "tilted12", "tilted57", "crossing")
NAMES = ("open_box",) + OFFAXIS + ("stacked3", "stacked14", "stacked14_200")
# name -> (box_scene's size, index of the duplicated rect, copies appended after the box's rects)
STACKED = {"stacked3": (8, 3, 3), "stacked14": (8, 0, 14), "stacked14_200": (200, 2 * 6 + 2, 14)}


def _with_walls(name, box, walls):
    walls = np.ascontiguousarray(walls, scene.RECT_DTYPE).copy()
    return scene.Scene(name, walls, box.windows, box.lights, scene.assign_texel_bases(walls))


def open_box_scene():
    box = scene.box_scene(200, tile_size=TILE)
    return _with_walls("open_box", box, np.concatenate([box.walls[:36], box.walls[72:]]))


def stacked_scene(name):
    n, dup, copies = STACKED[name]
    box = scene.box_scene(n, tile_size=TILE)
    return _with_walls(name, box, np.concatenate([box.walls, np.repeat(box.walls[dup:dup + 1], copies)]))


@functools.lru_cache(None)
def get(name):
    """The scene of that name; shared between tests, so treat it as read-only."""
    if name == "open_box":
        return open_box_scene()
    if name in STACKED:
        return stacked_scene(name)
    if name in OFFAXIS:
        return offaxis_scenes.get(name)
    raise KeyError(name)


def stack_texels(name):
    """(texel range of the duplicated rect, texel range of all its copies) of a stacked scene"""
    sc = get(name)
    _, dup, copies = STACKED[name]
    base = [int(b) for b in sc.walls["lm"][:, 0]] + [sc.num_texels]
    return (base[dup], base[dup + 1]), (base[len(sc.walls) - copies], sc.num_texels)
