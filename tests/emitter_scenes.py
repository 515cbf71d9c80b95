"""Scenes whose emitters are not the axis-aligned, vertical window and ceiling light of every other scene
(tests/test_emitter_scenes_host.py, tests/test_gpu_emitter_scenes.py, tests/golden/make_ref_fixtures.py,
tests/golden/make_rad_fixtures.py). All on scene.box_scene(200, tile_size=2.0)'s walls unless said otherwise, every
emitter from scene.create_rectangle, baked at bake_scenes.SPA with the schedule of tests/golden/glibc_rand_4096.npy.

  skylight           one 4 m x 1.45 m window, horizontal at z = 2.599 and facing down: a window through the sampler
                     basis' colinear branch (helper axis (0, 1, 0), photonmap.cl:43-48)
  lamps              the box's window; a 0.5 x 0.5 lamp on the x = 0 wall (n = +x): a light through the other branch
                     (photonmap.cl:65-70); a 0.5 x 0.5 up-light on the floor (n = +z): the colinear branch with n.z > 0.
                     Three sources of two kinds in one schedule
  tilted_emitters    one window and one lamp, each turned about z and leaned, wholly inside the room: all nine
                     components of width, height and n non-zero, so the basis, the direction and the emission point
                     (photonmap.cl:181) are full three-term sums; both edge lengths inexact in the schedule's area
  threshold          two 1 x 1 windows and two 0.5 x 0.5 lamps under the ceiling with width = (L, 0, L*eps), height =
                     (0, L, 0), eps = 1.3e-3 and 1.5e-3: |n.z| on either side of the basis' `>= 0.999999f`, and a cross
                     product of length 1.5e-3 through cl_normalize
  threshold_panels   threshold's emitters, plus two 1 x 1 wall panels at z = 0.3 of the same two tilts facing up,
                     appended after the box's rects: the bounce sampler and the walls' setup on those normals
  outside            a 4 x 1.45 window at y = -0.05 facing +y, a 0.5 x 0.5 lamp at z = 2.65 facing down, and a tilted
                     lamp that straddles the ceiling: first rays that start outside the walls' bounding box and enter
                     through back faces (photonmap.cl:126-128 culls them); photons emitted above the ceiling leave
  tilted12_emitters  tilted_emitters' sources on offaxis_scenes.get("tilted12")'s walls

variant(name, "lattice") puts a scene's emitters on box_scene(200, tile_size=4.0)'s walls (the box of
tests/test_gpu_lattice.py, which has a verified lattice), variant(name, "compact") on box_scene(2000, tile_size=2.0)'s
(the compact closed-box instance), variant(name, "fine") on box_scene(200)'s at the reference's 200 texels/m²: 92,824
texels of 7 cm instead of 1,176 of 70 cm. A float32 rounding of an emission point moves a hit by 1e-7 m and shows in a
lightmap only where that crosses a texel's edge, so the fine lightmap sees a misrounded emission point 10 times as
often per photon.
"""
import functools

import numpy as np

import offaxis_scenes
from fmgi import scene

f32 = np.float32
TILE = 2.0
EPS = (1.3e-3, 1.5e-3)  # threshold's tilts
# the scenes on the closed box's walls (one plane slot per axis); threshold_panels adds two general rects to them
BOX = ("skylight", "lamps", "tilted_emitters", "threshold", "threshold_panels", "outside")
NAMES = BOX + ("tilted12_emitters",)
VARIANT_WALLS = {"lattice": (200, 4.0), "compact": (2000, 2.0), "fine": (200, float(scene.TILE_SIZE))}


def _rects(*rects):
    return np.array(list(rects), scene.RECT_DTYPE) if rects else np.zeros(0, scene.RECT_DTYPE)


def _threshold_rect(x, y, z, L, eps, tile_size):
    return scene.create_rectangle(x, y, z, L, 0, f32(L * eps), 0, L, 0, tile_size)


def emitters(name):
    """(windows, lights) of the scene"""
    if name == "skylight":
        return _rects(scene.create_rectangle(3.0, 3.0, 2.599, 4.0, 0, 0, 0, 1.45, 0)), _rects()
    if name == "lamps":
        return (scene.box_scene(8).windows,
                _rects(scene.create_rectangle(0.001, 4.25, 1.0, 0, -0.5, 0, 0, 0, 0.5, 0.0),      # n = +x
                       scene.create_rectangle(5.25, 3.75, 0.001, -0.5, 0, 0, 0, 0.5, 0, 0.0)))    # n = +z
    if name in ("tilted_emitters", "tilted12_emitters"):
        # a 1.6 x 1.2 window and a 0.5 x 0.55 lamp, width along x and height along z, rolled about y, leaned about
        # x and turned about z by (0.25, 0.35, 0.5) and (-0.3, 1.9, 2.1) rad; written out, so that no libm is in it
        return (_rects(scene.create_rectangle(2.0, 1.0, 0.9, 1.2954063, 0.8623527, -0.37184724,
                                              0.4516809, -0.20754534, 1.0922039)),
                _rects(scene.create_rectangle(6.5, 5.0, 2.1, -0.120450355, 0.48291802, -0.0477693,
                                              0.51126003, 0.11071651, -0.16986768, 0.0)))
    if name in ("threshold", "threshold_panels"):
        return (_rects(*[_threshold_rect(2.0 + 4.0 * k, 2.0, 2.5, 1.0, e, scene.TILE_SIZE) for k, e in enumerate(EPS)]),
                _rects(*[_threshold_rect(2.25 + 4.0 * k, 5.0, 2.5, 0.5, e, 0.0) for k, e in enumerate(EPS)]))
    if name == "outside":
        return (_rects(scene.create_rectangle(3.0, -0.05, 0.85, 4.0, 0, 0, 0, 0, 1.45)),
                _rects(scene.create_rectangle(5.0, 4.0, 2.65, 0.5, 0, 0, 0, 0.5, 0, 0.0),
                       # width (0.4 cos 2.1, 0.4 sin 2.1, 0.1), height (0.2 sin 2.1, -0.2 cos 2.1, 0.35), written out:
                       # its top corner is at z = 2.65
                       scene.create_rectangle(6.0, 5.0, 2.2, -0.20193844, 0.34528375, 0.1, 0.17264187, 0.10096922, 0.35,
                                              0.0)))
    raise KeyError(name)


def panels():
    """threshold_panels' two walls: threshold's tilts about y, facing up (n.x as the emitters', n.z negated)"""
    return _rects(*[scene.create_rectangle(3.0 + 4.0 * k, 3.0, 0.3, -1.0, 0, f32(1.0 * e), 0, 1.0, 0, TILE)
                    for k, e in enumerate(EPS)])


def _on(name, walls):
    walls = np.ascontiguousarray(walls, scene.RECT_DTYPE).copy()
    windows, lights = emitters(name)
    return scene.Scene(name, walls, windows, lights, scene.assign_texel_bases(walls))


@functools.lru_cache(None)
def get(name):
    """The scene of that name; shared between tests, so treat it as read-only."""
    if name not in NAMES:
        raise KeyError(name)
    if name == "tilted12_emitters":
        return _on(name, offaxis_scenes.get("tilted12").walls)
    walls = scene.box_scene(200, tile_size=TILE).walls
    if name == "threshold_panels":
        walls = np.concatenate([walls, panels()])
    return _on(name, walls)


@functools.lru_cache(None)
def variant(name, kind):
    """The emitters of `name` on the walls of another closed box: kind "lattice", "compact" or "fine"."""
    n, tile = VARIANT_WALLS[kind]
    sc = _on(name, scene.box_scene(n, tile_size=tile).walls)
    sc.name = f"{name}_{kind}"
    return sc


def source_begins(L):
    """the first item of every source of a schedule, in source order"""
    return [int(L["item_begin"][np.flatnonzero(L["source"] == s)[0]]) for s in range(int(L["source"].max()) + 1)]
