"""The scenes of tests/bake_scenes.py reach what the GPU tests (tests/test_gpu_bake_scenes.py) use them for: what
the host tables make of each (plane slots, filter pairs, general rects, no lattice, AUTO's scan, the fullest grid
cell) as exact values, and what the oracle does on them (escapes, hits on general rects, who wins a stack of
coincident rects). The oracle's own invariants on these scenes, which tests/test_oracle.py checks on closed boxes
and layouts only: split invariance, thread-count invariance, and O.bake == O.bake_port."""
import functools
import os

import numpy as np
import pytest

import bake_scenes
import fm_oracle as O
import fmgi
from conftest import GOLDEN

SPA = bake_scenes.SPA
# name: (walls, grid J, filter J, general rects, AUTO's kernel, most records in a grid cell); every scene: no lattice
FACTS = {
    "open_box": (164, [1, 1, 1], [32, 32, 36], 0, fmgi.KERNEL_GRID, 4),
    "open_tilted": (176, [1, 1, 1], [32, 32, 36], 12, fmgi.KERNEL_GRID, 4),
    "tilted1": (201, [1, 1, 1], [32, 32, 36], 1, fmgi.KERNEL_GRID, 4),
    "tilted12": (212, [1, 1, 1], [32, 32, 36], 12, fmgi.KERNEL_GRID, 4),
    "tilted57": (257, [1, 1, 1], [32, 32, 36], 57, fmgi.KERNEL_GRID, 4),
    "crossing": (216, [2, 2, 1], [36, 36, 36], 0, fmgi.KERNEL_GRID, 4),
    "stacked3": (9, [1, 1, 1], [1, 4, 1], 0, fmgi.KERNEL_FAST, 4),
    "stacked14": (20, [1, 1, 1], [1, 1, 15], 0, fmgi.KERNEL_GRID, 15),
    "stacked14_200": (214, [1, 1, 1], [32, 32, 50], 0, fmgi.KERNEL_GRID, 18),
}
# the oracle's (scans, deposits, escapes) of the 102,400 photons of items [0, 1024)
ORACLE_1024 = {
    "open_box": (324_122, 223_855, 100_267),
    "open_tilted": (353_735, 255_351, 98_384),
    "tilted1": (819_195, 819_194, 1),
    "tilted12": (819_200, 819_200, 0),
    "tilted57": (819_200, 819_200, 0),
    "crossing": (819_197, 819_196, 1),
    "stacked3": (819_195, 819_194, 1),
    "stacked14": (819_195, 819_194, 1),
    "stacked14_200": (819_195, 819_194, 1),
}
K_ORDERED_ROUNDS = 12  # fmgi_kernels.hip ScanGridImpl::kOrderedRounds


@pytest.fixture(scope="module")
def offsets():
    return np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))


@functools.lru_cache(None)
def _schedule(name):
    sc = bake_scenes.get(name)
    return O.schedule_with_offsets(sc, SPA, np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))


@functools.lru_cache(None)
def _port_1024(name):
    lm, st = O.bake_port(bake_scenes.get(name), _schedule(name), 0, 1024)
    lm.setflags(write=False)
    return lm, st


def _general(sc, ctx):
    """the rects that are in no filter record: the scans' `general` list"""
    return sorted(set(range(len(sc.walls))) - {int(i) for i in ctx.filter_image()["idx"]})


def test_every_scene_has_its_facts():
    assert set(bake_scenes.NAMES) == set(FACTS) == set(ORACLE_1024) and len(bake_scenes.NAMES) == 9


@pytest.mark.parametrize("name", bake_scenes.NAMES)
def test_host_tables(offsets, name):
    sc = bake_scenes.get(name)
    walls, gJ, fJ, ngeneral, auto, max_count = FACTS[name]
    ctx = fmgi.Context(-1)
    ctx.set_scene(sc)
    assert ctx.plan(SPA, rng_offsets=offsets) == 10_000_128
    assert len(sc.walls) == walls
    g = ctx.grid_tables()
    assert g["J"] == gJ
    assert ctx.filter_image()["J"] == fJ
    general = _general(sc, ctx)
    assert len(general) == ngeneral
    # the general rects are the scene's last ones: the tests below count hits on them by index
    assert general == list(range(walls - ngeneral, walls))
    assert len(ctx.lattice_tables()["lattice"]) == 0
    assert ctx.auto_kernel == auto
    assert int(g["cells"]["count"].max()) == max_count
    ctx.close()


@pytest.mark.parametrize("name", ["stacked14", "stacked14_200"])
def test_a_stack_outnumbers_the_ordered_scan_s_rounds(name):
    """ordered_exact gives up after kOrderedRounds candidates and the scan falls back to the literal one: a cell
    of at most that many records would never get there, and these two scenes would test nothing"""
    ctx = fmgi.Context(-1)
    ctx.set_scene(bake_scenes.get(name))
    assert int(ctx.grid_tables()["cells"]["count"].max()) > K_ORDERED_ROUNDS
    ctx.close()


@pytest.mark.parametrize("name", bake_scenes.NAMES)
def test_oracle_counters(name):
    _, st = _port_1024(name)
    assert st["photons"] == 102_400
    assert (st["scans"], st["deposits"], st["escapes"]) == ORACLE_1024[name]
    assert st["scans"] == st["deposits"] + st["escapes"]


@pytest.mark.parametrize("name", ["open_box", "open_tilted"])
def test_most_photons_leave_the_open_scenes(name):
    _, st = _port_1024(name)
    assert st["escapes"] >= 0.9 * st["photons"], f"{st['escapes']} escapes of {st['photons']} photons (measured: 100,267 / 98,384)"
    assert st["scans"] == st["deposits"] + st["escapes"]


@pytest.mark.parametrize("name,least", [("tilted12", 1000), ("tilted1", 20), ("open_tilted", 1)])
def test_general_rects_are_hit(name, least):
    """events on rects outside the filter image in items 0..31 of launch 0 (measured: tilted12 1,902 of 25,600,
    tilted1 59, open_tilted 1,174 of 8,086)"""
    sc, L = bake_scenes.get(name), _schedule(name)
    first = FACTS[name][0] - FACTS[name][3]
    events = hits = longest = 0
    for gid in range(32):
        ev, _ = O.trace_item(sc, int(L[0]["source"]), int(L[0]["is_window"]), (gid + int(L[0]["rng_offset"])) & 0xFFFFFFFF)
        events += len(ev)
        hits += int((ev["rect"] >= first).sum())
        longest = max(longest, len(ev))
    assert hits >= least, f"{hits} of {events} events on general rects"
    if name == "open_tilted":
        assert longest < 800, f"an item of {longest} events: no photon of it left the scene"


@functools.lru_cache(None)
def _counts_4096(name):
    return O.bake(bake_scenes.get(name), _schedule(name), 0, 4096, counts=True)


@pytest.mark.parametrize("name", list(bake_scenes.STACKED))
def test_the_reference_gives_a_stack_to_its_first_rect(name):
    """the reference scans in index order and replaces the hit only when `d < closest` (photonmap.cl:189-206): of
    coincident rects the one of the lowest index takes every deposit (measured over items [0, 4096): stacked3
    356,937, stacked14 1,158,899, stacked14_200 37,064 on the duplicated rect)"""
    _, _, cnt = _counts_4096(name)
    (d0, d1), (c0, c1) = bake_scenes.stack_texels(name)
    assert c1 == bake_scenes.get(name).num_texels and d1 <= c0
    assert not cnt[c0:c1].any(), f"{int(cnt[c0:c1].sum())} deposits on the copies"
    assert cnt[d0:d1].sum() >= 10_000, int(cnt[d0:d1].sum())


@pytest.mark.parametrize("name", bake_scenes.NAMES)
def test_oracle_split_and_thread_invariance(name):
    sc, L = bake_scenes.get(name), _schedule(name)
    whole, st = O.bake(sc, L, 0, 600, nthreads=8)
    a, sa = O.bake(sc, L, 0, 250, nthreads=8)
    b, sb = O.bake(sc, L, 250, 600, nthreads=8)
    assert np.array_equal(whole, a + b)
    for k in ("photons", "scans", "deposits", "escapes"):
        assert st[k] == sa[k] + sb[k], k
    one, st1 = O.bake(sc, L, 0, 600, nthreads=1)
    assert np.array_equal(whole, one) and st1 == st


@pytest.mark.parametrize("name", bake_scenes.NAMES)
def test_port_build_equals_the_oracle(name):
    """tests/test_oracle.py compares the two builds on closed boxes and a layout: here with most photons escaping,
    with general rects and with coincident rects"""
    lm, st = O.bake(bake_scenes.get(name), _schedule(name), 0, 1024)
    plm, pst = _port_1024(name)
    assert np.array_equal(lm, plm)
    assert st == pst
