"""Radiosity on partitioned, tilted and open scenes (tests/offaxis_scenes.py).

The box scenes of tests/test_radiosity.py are closed: no ray ever misses, so `target = -1` in k_rad_rays
and the `id < 0` path of k_rad_gather have not run, and the candidate sort has only seen 200 -> 256 and
172 -> 256 keys. Here:

  open_tilted        no ceiling: 43 % of the rays leave the scene; lightmaps of (1,2), (2,1), (2,2), (2,4) and
                     (4,2) texels, so the mip chain takes its 1-D steps
  crossing           partitions inside the box
  tilted56/tilted57  256 and 257 rects: sort_n 256 (no padding) and 512 (255 pad keys)
  tilted_emitters    tests/emitter_scenes.py: a window and a lamp that are not axis-aligned, which the backend puts
                     into its rect list as hit geometry and as emitters (the window with its 32 x 16 grid: the
                     backend gives every emitter a texel base of its own behind the walls', radiosityNative.c:111-126)

  reference (oracle/_ref/rad_ref, tests/golden/rad_ref.json) == oracle/rad_oracle.c          (CPU)
  GPU texels and sourceTexelIds == oracle bit for bit; the libc stream left in place;
  open_tilted and crossing == the reference hash; open_tilted again in chunks of 37 jobs    (GPU)
"""
import hashlib
import json
import os

import numpy as np
import pytest

import fm_oracle as O
import emitter_scenes
import fmgi
import offaxis_scenes as S
from conftest import GOLDEN

PINNED = {"crossing": 3, "open_tilted": 5, "tilted12": 9, "tilted_emitters": 11}  # name: seed of the reference run
GPU_SCENES = ["crossing", "open_tilted", "tilted56", "tilted57", "tilted_emitters"]
SEED, PRE = 5, 777  # the GPU cases start mid-stream, except where the reference fixture fixes the seed


def _scene(name):
    return emitter_scenes.get(name) if name in emitter_scenes.NAMES else S.get(name)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _fixtures():
    with open(os.path.join(GOLDEN, "rad_ref.json")) as f:
        return json.load(f)


def _seed(libc, name):
    if name in PINNED:
        libc.srand(PINNED[name])
    else:
        libc.srand(SEED)
        for _ in range(PRE):
            libc.rand()


_cache = {}


def _oracle(libc, name):
    """the oracle's (texels, sids, next rand()) from the case's stream position; computed once, read-only"""
    if name not in _cache:
        _seed(libc, name)
        tex, sids = O.radiosity(_scene(name), with_sids=True)
        nxt = libc.rand()
        tex.setflags(write=False)
        sids.setflags(write=False)
        _cache[name] = (tex, sids, nxt)
    return _cache[name]


def test_lightmap_shapes_of_the_open_scene():
    shapes = {(int(w["lm"][1]), int(w["lm"][2])) for w in S.get("open_tilted").walls}
    assert {(1, 2), (2, 1), (2, 2), (2, 4), (4, 2)} <= shapes


@pytest.mark.parametrize("name", list(PINNED))
def test_oracle_reproduces_reference(name, libc):
    ref = _fixtures()[name]
    assert ref["seed"] == PINNED[name]
    sc = _scene(name)
    tex, sids, nxt = _oracle(libc, name)
    assert nxt == ref["next_rand"]
    first = [float(tex[int(w["lm"][0]), 0]) for w in sc.walls]
    assert first == ref["first_texel_per_wall"]
    assert _sha(tex) == ref["sha256_f32"]
    assert sids.shape == (S.level0_jobs(sc), O.RAD_RAYS)


def test_miss_share(libc):
    """open_tilted is open enough to exercise the miss paths and closed enough to exercise the hits; the
    closed scenes have no miss at all"""
    sids = _oracle(libc, "open_tilted")[1]
    share = float((sids < 0).mean())
    assert 0.10 < share < 0.90, share
    assert (sids[sids < 0] == -1).all()
    assert (_oracle(libc, "crossing")[1] >= 0).all()


@pytest.mark.parametrize("name", ["tilted56", "tilted57"])
def test_rect_counts_at_the_power_of_two_edge(name):
    n = len(S.get(name).walls)
    assert n == {"tilted56": 256, "tilted57": 257}[name]
    assert 1 << (n - 1).bit_length() == {"tilted56": 256, "tilted57": 512}[name]


# ---- GPU ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_gpu_equals_oracle(torch_cuda, libc, name):
    sc = _scene(name)
    t_o, s_o, nxt = _oracle(libc, name)
    _seed(libc, name)
    t_g, s_g = fmgi.radiosity(sc, with_sids=True)
    assert libc.rand() == nxt, "the libc stream must be left where the reference leaves it"
    assert np.array_equal(s_g, s_o), f"{int((s_g != s_o).sum())} sourceTexelIds differ"
    bad = (t_g.view(np.uint32) != t_o.view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} texels differ, first {np.nonzero(bad)[0][:5]}"
    st = fmgi.radiosity_stats()
    assert st["jobs"] == S.level0_jobs(sc) and st["rays"] == st["jobs"] * 10000
    if name in PINNED:
        assert _sha(t_g) == _fixtures()[name]["sha256_f32"]


@pytest.mark.gpu
def test_gpu_chunked_rand_replay_with_misses(torch_cuda, libc, monkeypatch):
    """open_tilted's jobs in chunks of 37 for the device rand() replay: same texels, same sids"""
    ref = _fixtures()["open_tilted"]
    t_o, s_o, nxt = _oracle(libc, "open_tilted")
    monkeypatch.setenv("FMGI_RAD_CHUNK", "37")
    _seed(libc, "open_tilted")
    t_g, s_g = fmgi.radiosity(S.get("open_tilted"), with_sids=True)
    assert libc.rand() == nxt == ref["next_rand"]
    assert np.array_equal(s_g, s_o)
    assert np.array_equal(t_g.view(np.uint32), t_o.view(np.uint32))
    assert _sha(t_g) == ref["sha256_f32"]
