"""Scenes with tilted, open and partitioned geometry for the AO, radiosity, view and output tests
(tests/test_offaxis_*.py, tests/golden/make_*_fixtures.py). Everything is built from fmgi.scene at
2 texels/m², so an oracle run of any of them takes seconds.

  crossing     box200 plus two back-to-back partitions that cross each other (16 rects): the BSP tree
               has nodes with two children and leaves with items, unlike a box's chain
  tilted1/12   box200 plus 1 / 12 rects that are not axis-aligned (scene.tilted_scene)
  open_tilted  tilted12 without its ceiling (walls 36..71): rays leave the scene
  tilted56/57  256 / 257 rects: the power-of-two edge of the device sorts (sort_n 256 and 512)
"""
import functools

import numpy as np

from fmgi import scene

f32 = np.float32
TILE = 2.0
NAMES = ("crossing", "tilted1", "tilted12", "open_tilted", "tilted56", "tilted57")


def crossing_scene():
    box = scene.box_scene(200, tile_size=TILE)
    walls = list(box.walls)
    R = lambda *a: walls.append(scene.create_rectangle(*a, TILE))  # noqa: E731
    Z = f32(2.6)
    for k in range(4):
        y0, y1 = f32(0.5 + 1.75 * k), f32(0.5 + 1.75 * (k + 1))
        x0, x1 = f32(1 + 2 * k), f32(1 + 2 * (k + 1))
        R(5, y0, 0, 0, f32(y1 - y0), 0, 0, 0, Z)
        R(5, y1, 0, 0, f32(y0 - y1), 0, 0, 0, Z)
        R(x0, 4, 0, f32(x1 - x0), 0, 0, 0, 0, Z)
        R(x1, 4, 0, f32(x0 - x1), 0, 0, 0, 0, Z)
    walls = np.array(walls, scene.RECT_DTYPE)
    return scene.Scene("crossing", walls, box.windows, box.lights, scene.assign_texel_bases(walls))


def open_tilted_scene():
    sc = scene.tilted_scene(12, tile_size=TILE)
    walls = np.concatenate([sc.walls[:36], sc.walls[72:]]).copy()
    return scene.Scene("open_tilted", walls, sc.windows, sc.lights, scene.assign_texel_bases(walls))


@functools.lru_cache(None)
def get(name):
    """The scene of that name; shared between tests, so treat it as read-only."""
    if name == "crossing":
        return crossing_scene()
    if name == "open_tilted":
        return open_tilted_scene()
    if name.startswith("tilted"):
        return scene.tilted_scene(int(name[6:]), tile_size=TILE)
    raise KeyError(name)


def level0_jobs(sc):
    return int(sum(int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls))


def decode_tree(enc):
    """fmgi_ao_tree's encoding -> list of (left, right, plane, items)"""
    enc = np.asarray(enc)
    nodes, p = [], 0
    while p < len(enc):
        left, right, plane, n = (int(v) for v in enc[p:p + 4])
        nodes.append((left, right, plane, [int(v) for v in enc[p + 4:p + 4 + n]]))
        p += 4 + n
    return nodes


def tree_depth(nodes, i=0):
    left, right = nodes[i][0], nodes[i][1]
    return 1 + max(tree_depth(nodes, left) if left >= 0 else 0, tree_depth(nodes, right) if right >= 0 else 0)
