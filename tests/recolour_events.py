"""Shared by test_recolour_host.py and test_gpu_recolour.py: the small lit box, its schedule, and the per-state
photon histogram derived from the oracle's bounce events alone (no knowledge of the kernel's state word).

A photon's deposited colour changes from one bounce to the next in one of three ways (photonmap.cl:236-258):
unchanged (a mirror bounce), times 0.9f (a diffuse bounce), or green times 0.85f and blue times 0.7f, then
times 0.9f (a diffuse bounce on the floor). The colour state is the source kind in bit 9 and, below a leading
1, one bit per diffuse bounce, oldest first, set when that bounce was on the floor.
"""
import functools
import os

import numpy as np

import fm_oracle as O
from conftest import GOLDEN
from fmgi import scene

SPA = 2000
STATES = 1024
f32 = np.float32
RANGES = ((0, 64), (256, 320))  # the first 64 items of the window and of the lamp


@functools.lru_cache(maxsize=None)
def lit_box():
    """(scene, schedule): 2,152 texels, one window (items 0-255) and one lamp (items 256-511)."""
    sc = scene.box_scene(200, tile_size=4.0, with_light=True)
    offsets = np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))
    L = O.schedule_with_offsets(sc, SPA, offsets)
    assert [(int(l["item_begin"]), int(l["count"]), int(l["is_window"])) for l in L] == [(0, 256, 1), (256, 256, 0)]
    return sc, L, offsets


def table_replay(window_rgb, light_rgb, floor_tint, albedo):
    """fmgi_palette_table's definition in numpy.float32: int64 [1024, 3]."""
    out = np.zeros((STATES, 3), np.int64)
    tint = np.array(floor_tint, f32)
    alb = f32(albedo)
    for sid in range(STATES):
        s = sid & 511
        if s == 0:
            continue
        c = np.array(window_rgb if sid & 512 else light_rgb, f32)
        nb = s.bit_length() - 1
        for b in range(nb - 1, -1, -1):
            if (s >> b) & 1:
                c = (c * tint).astype(f32)
            c = (c * alb).astype(f32)
        out[sid] = [int(np.ldexp(np.float64(v), 25)) for v in c]
    return out


def item_events(sc, L, item):
    li = int(np.searchsorted(L["item_begin"], item, side="right") - 1)
    gid = item - int(L[li]["item_begin"])
    state = (gid + int(L[li]["rng_offset"])) & 0xFFFFFFFF
    ev, _ = O.trace_item(sc, int(L[li]["source"]), int(L[li]["is_window"]), state)
    return ev, int(L[li]["is_window"])


def derive_states(ev, is_window):
    """The colour state of every event of one work item, from the colours alone; asserts that exactly one of
    the three transitions explains each step."""
    src = np.array([18, 18, 18] if is_window else [16, 16, 18], f32)
    tint = np.array([1.0, 0.85, 0.7], f32)
    n = len(ev)
    if n == 0:
        return np.zeros(0, np.int64)
    rgb = ev["rgb"].astype(f32)
    first = np.ones(n, bool)
    first[1:] = ev["photon"][1:] != ev["photon"][:-1]
    prev = np.empty_like(rgb)
    prev[1:] = rgb[:-1]
    prev[first] = src
    diffuse = prev * f32(0.9)
    floor = (prev * tint) * f32(0.9)
    assert diffuse.dtype == f32 and floor.dtype == f32
    hits = np.stack([(rgb == prev).all(1), (rgb == diffuse).all(1), (rgb == floor).all(1)], 1)
    assert (hits.sum(1) == 1).all(), "a colour transition is ambiguous or unknown"
    kind = hits.argmax(1).tolist()
    out, state = [], 0
    for i, k in enumerate(kind):
        if first[i]:
            state = (512 if is_window else 0) | 1
        if k:
            assert (state & 511) < 256, "more than eight diffuse bounces"
            state = (state & 512) | ((state & 511) << 1) | (k == 2)
        out.append(state)
    return np.array(out, np.int64)


@functools.lru_cache(maxsize=None)
def events_of(ranges=RANGES):
    """Every event of the items in `ranges`: (texel int64 [n], state int64 [n], rgb float32 [n, 3])."""
    sc, L, _ = lit_box()
    tex, st, rgb = [], [], []
    for b, e in ranges:
        for item in range(b, e):
            ev, win = item_events(sc, L, item)
            tex.append(ev["texel"].astype(np.int64))
            st.append(derive_states(ev, win))
            rgb.append(ev["rgb"].copy())
    return np.concatenate(tex), np.concatenate(st), np.concatenate(rgb)


@functools.lru_cache(maxsize=None)
def sparse_histogram(ranges=RANGES):
    """The event-derived histogram as (state, texel, count) arrays of its non-empty cells, sorted by cell."""
    sc, _, _ = lit_box()
    tex, st, _ = events_of(ranges)
    cell, cnt = np.unique(st * sc.num_texels + tex, return_counts=True)
    return cell // sc.num_texels, cell % sc.num_texels, cnt.astype(np.int64)


def dense_histogram(ranges=RANGES):
    sc, _, _ = lit_box()
    s, t, n = sparse_histogram(ranges)
    h = np.zeros((STATES, sc.num_texels), np.uint64)
    h[s, t] = n.astype(np.uint64)
    return h


def fold(sparse, table, num_texels):
    """sum over the cells of count * table[state] in Python integers: [num_texels][3] (a list of lists)."""
    out = [[0, 0, 0] for _ in range(num_texels)]
    for s, t, n in zip(*(a.tolist() for a in sparse)):
        row = table[s]
        o = out[t]
        for c in range(3):
            o[c] += n * int(row[c])
    return out
