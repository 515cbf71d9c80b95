"""The scenes of tests/emitter_scenes.py reach what the GPU tests (tests/test_gpu_emitter_scenes.py) use them for, as
exact values: every emitter's float32 normal and the side of the sampler basis' `fabs(n.z) >= 0.999999f`
(photonmap.cl:43-48, :65-70) it is on; the schedules' item counts at three densities against the oracle's, field for
field; what the host tables make of each scene; and the oracle's counters on the first 256 items of every source, with
the conditions that keep a scene from testing nothing (outside's window shines in, its straddling lamp loses a few
per cent of its photons, nothing else escapes). The oracle's own invariants on these scenes: O.bake == O.bake_port,
split invariance and thread-count invariance over a source boundary."""
import ctypes
import functools
import os

import numpy as np
import pytest

import bake_scenes
import emitter_scenes
import fm_oracle as O
import fmgi
from conftest import GOLDEN

SPA = bake_scenes.SPA
THRESHOLD = np.float32(0.999999)
# per source, windows first: the float32 normal's bits
NORMALS = {
    "skylight": [(0x00000000, 0x00000000, 0xBF7FFFFF)],
    "lamps": [(0x00000000, 0x3F7FFFFF, 0x00000000), (0x3F800000, 0x00000000, 0x80000000),
              (0x00000000, 0x80000000, 0x3F800000)],
    "tilted_emitters": [(0xBEE6957D, 0x3F530A62, 0x3EAF904D), (0x3E8EE1D1, 0x3E2720E8, 0x3F7240B9)],
    "threshold": [(0x3AAA64BA, 0x00000000, 0xBF7FFFF2), (0x3AC49B98, 0x00000000, 0xBF7FFFEE)] * 2,
    "outside": [(0x00000000, 0x3F7FFFFF, 0x00000000), (0x00000000, 0x00000000, 0xBF800000),
                (0xBF2E7F8E, 0xBF0A8F54, 0x3EFC1763)],
}
NORMALS["threshold_panels"] = NORMALS["threshold"]
NORMALS["tilted12_emitters"] = NORMALS["tilted_emitters"]
PANEL_NORMALS = [(0x3AAA64BA, 0x80000000, 0x3F7FFFF2), (0x3AC49B98, 0x80000000, 0x3F7FFFEE)]
# per source: whether the basis takes the colinear branch (helper axis (0, 1, 0))
COLINEAR = {
    "skylight": [True], "lamps": [False, False, True], "tilted_emitters": [False, False],
    "threshold": [True, False, True, False], "threshold_panels": [True, False, True, False],
    "outside": [False, True, False], "tilted12_emitters": [False, False],
}
# spa: per source the items of its launches (the BASELINE densities 65,000 and 1,724,137,931, and SPA)
ITEMS = {
    "skylight": {SPA: [10_000_128], 65_000: [3_840], 1_724_137_931: [100_000_256]},
    "lamps": {SPA: [10_000_128, 431_104, 431_104], 65_000: [3_840, 256, 256],
              1_724_137_931: [100_000_256, 4_310_528, 4_310_528]},
    "tilted_emitters": {SPA: [3_310_592, 474_368], 65_000: [1_280, 256], 1_724_137_931: [33_103_616, 4_741_632]},
    "threshold": {SPA: [1_724_160, 1_724_160, 431_104, 431_104], 65_000: [768, 768, 256, 256],
                  1_724_137_931: [17_241_600, 17_241_600, 4_310_528, 4_310_528]},
    "outside": {SPA: [10_000_128, 431_104, 286_720], 65_000: [3_840, 256, 256],
                1_724_137_931: [100_000_256, 4_310_528, 2_865_664]},
}
ITEMS["threshold_panels"] = ITEMS["threshold"]
ITEMS["tilted12_emitters"] = ITEMS["tilted_emitters"]
LAUNCHES = {"skylight": 391, "lamps": 425, "tilted_emitters": 149, "threshold": 170, "threshold_panels": 170,
            "outside": 420, "tilted12_emitters": 149}  # at SPA
# name: (walls, grid J, filter J, general rects, AUTO's kernel, most records in a grid cell, lattice faces). The box's
# walls at 2 texels/m² are a verified lattice of six faces (as at the 4 texels/m² of tests/test_gpu_lattice.py); a
# scene with general rects has none
FACTS = {
    "skylight": (200, [1, 1, 1], [32, 32, 36], 0, fmgi.KERNEL_GRID, 4, 6),
    "lamps": (200, [1, 1, 1], [32, 32, 36], 0, fmgi.KERNEL_GRID, 4, 6),
    "tilted_emitters": (200, [1, 1, 1], [32, 32, 36], 0, fmgi.KERNEL_GRID, 4, 6),
    "threshold": (200, [1, 1, 1], [32, 32, 36], 0, fmgi.KERNEL_GRID, 4, 6),
    "threshold_panels": (202, [1, 1, 1], [32, 32, 36], 2, fmgi.KERNEL_GRID, 4, 0),
    "outside": (200, [1, 1, 1], [32, 32, 36], 0, fmgi.KERNEL_GRID, 4, 6),
    "tilted12_emitters": (212, [1, 1, 1], [32, 32, 36], 12, fmgi.KERNEL_GRID, 4, 0),
}
# per source: the oracle's (scans, deposits, escapes) of the 25,600 photons of its first 256 items
ORACLE_256 = {
    "skylight": [(204_800, 204_800, 0)],
    "lamps": [(204_800, 204_800, 0), (204_797, 204_796, 1), (204_800, 204_800, 0)],
    "tilted_emitters": [(204_798, 204_797, 1), (204_800, 204_800, 0)],
    "threshold": [(204_800, 204_800, 0), (204_800, 204_800, 0), (204_797, 204_796, 1), (204_800, 204_800, 0)],
    "threshold_panels": [(204_800, 204_800, 0), (204_800, 204_800, 0), (204_797, 204_796, 1), (204_800, 204_800, 0)],
    "outside": [(204_667, 204_648, 19), (204_793, 204_792, 1), (200_229, 199_576, 653)],
    "tilted12_emitters": [(204_798, 204_797, 1), (204_800, 204_800, 0)],
}
STRADDLER = ("outside", 2)  # the lamp whose top corner is above the ceiling


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@pytest.fixture(scope="module")
def offsets_8192(offsets):
    """glibc's rand() after srand(1), twice as far as the fixture goes: lamps and outside have 4,245 and 4,188
    launches at spa 1,724,137,931"""
    lib = ctypes.CDLL(None)
    lib.rand.restype = ctypes.c_int
    lib.srand(1)
    out = np.array([lib.rand() for _ in range(8192)], np.int64)
    lib.srand(1)
    assert np.array_equal(out[:4096], offsets)
    return out


@functools.lru_cache(None)
def _schedule(name):
    sc = emitter_scenes.get(name)
    return O.schedule_with_offsets(sc, SPA, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))


@functools.lru_cache(None)
def _begins(name):
    return emitter_scenes.source_begins(_schedule(name))


@functools.lru_cache(None)
def _port_256(name, s):
    b = _begins(name)[s]
    lm, st = O.bake_port(emitter_scenes.get(name), _schedule(name), b, b + 256)
    lm.setflags(write=False)
    return lm, st


def _bits(v):
    return tuple(int(x) for x in np.ascontiguousarray(v[:3], np.float32).view(np.uint32))


def _sources(name):
    return [(name, s) for s in range(len(NORMALS[name]))]


ALL_SOURCES = [p for name in emitter_scenes.NAMES for p in _sources(name)]


def test_every_scene_has_its_facts():
    for table in (NORMALS, COLINEAR, ITEMS, LAUNCHES, FACTS, ORACLE_256):
        assert set(table) == set(emitter_scenes.NAMES)
    assert len(emitter_scenes.NAMES) == 7 and len(bake_scenes.NAMES) == 9
    assert set(emitter_scenes.BOX) == {n for n in FACTS if FACTS[n][0] in (200, 202)}


@pytest.mark.parametrize("name", emitter_scenes.NAMES)
def test_normals_and_branches(name):
    sc = emitter_scenes.get(name)
    assert len(sc.sources) == len(NORMALS[name]) == len(COLINEAR[name])
    for s, src in enumerate(sc.sources):
        assert _bits(src["n"]) == NORMALS[name][s], (s, [hex(b) for b in _bits(src["n"])])
        assert bool(np.abs(src["n"][2]) >= THRESHOLD) == COLINEAR[name][s], s
    nw = len(sc.windows)
    kinds = COLINEAR[name][:nw], COLINEAR[name][nw:]
    if name == "threshold":  # one window and one lamp on either side of the compare
        assert sorted(kinds[0]) == sorted(kinds[1]) == [False, True]
    if name == "lamps":  # a light through either branch, the colinear one with n.z > 0
        assert kinds[1] == [False, True] and sc.lights[1]["n"][2] == 1.0
    if name == "skylight":
        assert kinds == ([True], []) and sc.windows[0]["n"][2] == np.float32(-0.99999994)


def test_the_panels_have_the_emitters_tilts():
    sc = emitter_scenes.get("threshold_panels")
    box = emitter_scenes.get("threshold")
    assert np.array_equal(sc.walls[:200], box.walls) and len(sc.walls) == 202
    for k, wall in enumerate(sc.walls[200:]):
        assert _bits(wall["n"]) == PANEL_NORMALS[k]
        e = NORMALS["threshold"][k]
        assert PANEL_NORMALS[k][0] == e[0] and PANEL_NORMALS[k][2] == e[2] ^ 0x80000000  # the same tilt, facing up
        assert bool(np.abs(wall["n"][2]) >= THRESHOLD) == COLINEAR["threshold"][k]


@pytest.mark.parametrize("name", ["tilted_emitters", "tilted12_emitters"])
def test_tilted_emitters_have_no_zero_component_and_inexact_edges(name):
    sc = emitter_scenes.get(name)
    assert len(sc.windows) == 1 and len(sc.lights) == 1
    for src in sc.sources:
        for field in ("width", "height", "n"):
            assert (src[field][:3] != 0).all(), field
        for field in ("width", "height"):
            v = src[field][:3].astype(np.float64)
            dot = float(v @ v)
            assert float(np.float32(np.sqrt(dot))) ** 2 != dot, field
        # wholly inside the room: every corner 0.05 m from the walls' planes
        p, w, h = (src[f][:3].astype(np.float64) for f in ("pos", "width", "height"))
        for c in (p, p + w, p + h, p + w + h):
            assert 0.05 < c[2] < 2.55 and 0.05 <= c[0] <= 9.95 and 0.05 <= c[1] <= 7.95, c


def test_outside_s_emitters_are_outside():
    sc = emitter_scenes.get("outside")
    lo = sc.walls["pos"][:, :3].min(axis=0)
    assert sc.windows[0]["pos"][1] == np.float32(-0.05) < lo[1] == 0
    assert sc.lights[0]["pos"][2] == np.float32(2.65) > np.float32(2.6)
    s = sc.lights[1]
    z = [float(s["pos"][2]), float(s["pos"][2] + s["width"][2]), float(s["pos"][2] + s["height"][2]),
         float(np.float32(s["pos"][2] + s["width"][2]) + s["height"][2])]
    assert min(z) < 2.6 < max(z) and abs(max(z) - 2.65) < 1e-6


@pytest.mark.parametrize("spa", [SPA, 65_000, 1_724_137_931])
@pytest.mark.parametrize("name", emitter_scenes.NAMES)
def test_item_counts_and_plan(offsets_8192, name, spa):
    sc = emitter_scenes.get(name)
    ctx = fmgi.Context(-1)
    ctx.set_scene(sc)
    assert ctx.plan(spa, rng_offsets=offsets_8192) == sum(ITEMS[name][spa])
    L = O.schedule_with_offsets(sc, spa, offsets_8192)
    plan = ctx.get_plan()
    assert plan.dtype == L.dtype and len(plan) == len(L)
    for field in L.dtype.names:
        assert np.array_equal(plan[field], L[field]), field
    assert [int(L["count"][L["source"] == s].sum()) for s in range(len(sc.sources))] == ITEMS[name][spa]
    assert np.array_equal(L["is_window"], L["source"] < len(sc.windows))
    if spa == SPA:
        assert len(L) == LAUNCHES[name]
        assert plan.tobytes() == _schedule(name).tobytes()  # (the 4,096 offsets of the fixture suffice)
    ctx.close()


@pytest.mark.parametrize("name", emitter_scenes.NAMES)
def test_host_tables(offsets, name):
    sc = emitter_scenes.get(name)
    walls, gJ, fJ, ngeneral, auto, max_count, faces = FACTS[name]
    ctx = fmgi.Context(-1)
    ctx.set_scene(sc)
    assert ctx.plan(SPA, rng_offsets=offsets) == sum(ITEMS[name][SPA])
    assert len(sc.walls) == walls
    g = ctx.grid_tables()
    assert g["J"] == gJ
    assert ctx.filter_image()["J"] == fJ
    general = sorted(set(range(walls)) - {int(i) for i in ctx.filter_image()["idx"]})
    assert general == list(range(walls - ngeneral, walls))  # (threshold_panels: exactly its two panels)
    assert len(ctx.lattice_tables()["lattice"]) == faces
    assert ctx.auto_kernel == auto
    assert int(g["cells"]["count"].max()) == max_count
    ctx.close()


@pytest.mark.parametrize("name,kind,walls", [("outside", "lattice", 200), ("tilted_emitters", "lattice", 200),
                                             ("outside", "compact", 2000), ("tilted_emitters", "compact", 2000),
                                             ("tilted_emitters", "fine", 200)])
def test_the_variants_on_other_boxes(offsets, name, kind, walls):
    sc = emitter_scenes.variant(name, kind)
    assert sc.num_texels == {"lattice": 2152, "compact": 2000, "fine": 92824}[kind]
    base = emitter_scenes.get(name)
    assert len(sc.walls) == walls and np.array_equal(sc.sources, base.sources)
    ctx = fmgi.Context(-1)
    ctx.set_scene(sc)
    assert ctx.plan(SPA, rng_offsets=offsets) == sum(ITEMS[name][SPA])
    assert ctx.get_plan().tobytes() == _schedule(name).tobytes()
    assert ctx.grid_tables()["J"] == [1, 1, 1] and len(ctx.lattice_tables()["lattice"]) == 6
    assert ctx.auto_kernel == fmgi.KERNEL_GRID
    ctx.close()


@pytest.mark.parametrize("name,s", ALL_SOURCES)
def test_oracle_counters(name, s):
    _, st = _port_256(name, s)
    assert st["photons"] == 25_600
    assert (st["scans"], st["deposits"], st["escapes"]) == ORACLE_256[name][s]
    assert st["scans"] == st["deposits"] + st["escapes"]


@pytest.mark.parametrize("name,s", [p for p in ALL_SOURCES if p[0] != "tilted12_emitters"])
def test_what_leaves_a_closed_scene(name, s):
    """(each photon escapes at most once, so the escapes count photons)"""
    lm, st = _port_256(name, s)
    if (name, s) == STRADDLER:
        assert 256 <= st["escapes"] <= 2560, st["escapes"]  # between 1 % and 10 % (measured: 653 of 25,600)
    else:
        assert st["escapes"] <= (256 if (name, s) == ("outside", 0) else 2), st["escapes"]
    assert lm.any()


def test_outside_s_window_shines_in():
    """at least 99 % of its photons deposit at least once: every photon scans at least once, a scan deposits or
    escapes, and an escape ends the photon, so the photons that never deposit are among the 19 that escape"""
    _, st = _port_256("outside", 0)
    assert st["photons"] - st["escapes"] >= 0.99 * st["photons"], st["escapes"]


def test_the_straddling_lamp_s_first_item():
    """776 of 800 events in the first item of the lamp that straddles the ceiling: the photons emitted above it
    leave at once"""
    sc, L = emitter_scenes.get("outside"), _schedule("outside")
    li = int(np.flatnonzero(L["source"] == STRADDLER[1])[0])
    ev, _ = O.trace_item(sc, STRADDLER[1], 0, int(L[li]["rng_offset"]) & 0xFFFFFFFF)
    assert len(ev) == 776


@pytest.mark.parametrize("name,s", ALL_SOURCES)
def test_port_build_equals_the_oracle(name, s):
    b = _begins(name)[s]
    lm, st = O.bake(emitter_scenes.get(name), _schedule(name), b, b + 256)
    plm, pst = _port_256(name, s)
    assert np.array_equal(lm, plm)
    assert st == pst


@pytest.mark.parametrize("name", emitter_scenes.NAMES)
def test_oracle_split_and_thread_invariance(name):
    """a range over the last source boundary (skylight has one source: its first items)"""
    sc, L = emitter_scenes.get(name), _schedule(name)
    b = _begins(name)[-1]
    lo, cut, hi = max(b - 250, 0), max(b - 250, 0) + 250, max(b - 250, 0) + 600
    whole, st = O.bake(sc, L, lo, hi, nthreads=8)
    a, sa = O.bake(sc, L, lo, cut, nthreads=8)
    c, sc_ = O.bake(sc, L, cut, hi, nthreads=8)
    assert np.array_equal(whole, a + c)
    for k in ("photons", "scans", "deposits", "escapes"):
        assert st[k] == sa[k] + sc_[k], k
    one, st1 = O.bake(sc, L, lo, hi, nthreads=1)
    assert np.array_equal(whole, one) and st1 == st
