"""Ambient occlusion on partitioned and tilted scenes (tests/offaxis_scenes.py).

A closed box gives the reference's BSP build a chain: every wall is a centre item of some plane, no leaf
holds an item and no node has two children, so the far-child entry of the traversal (`shift + pd`) and
its pruning never run. `crossing` adds partitions that the tree really splits, `tilted56` adds walls
that are not axis-aligned.

  reference (oracle/_ref/ao_ref, tests/golden/ao_ref.json) == oracle/ao_oracle.c on crossing, tilted56   (CPU)
  the product's tree == the oracle's tree; crossing's tree branches                                     (CPU)
  tilted1 / tilted12 / open_tilted: the reference's build rule has no end there; product
  and oracle report the BSP depth at once, and the process lives on                                     (CPU)
  GPU texels == oracle bit for bit == reference hash; a wall range leaves the other texels alone        (GPU)
"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import offaxis_scenes as S
from conftest import GOLDEN, ORACLE, PKG, REPO
from fmgi import _lib, scene

PINNED = ["crossing", "tilted56"]   # the reference finishes on these
ENDLESS = ["tilted1", "tilted12", "open_tilted"]
AO_MAX_DEPTH = 48                   # FMGI_AO_MAX_DEPTH, csrc/fmgi_ao.h


def _ref(name):
    with open(os.path.join(GOLDEN, "ao_ref.json")) as f:
        return json.load(f)[name]


def test_depth_bound_is_the_header_constant():
    with open(os.path.join(PKG, "csrc", "fmgi_ao.h")) as f:
        assert f"#define FMGI_AO_MAX_DEPTH {AO_MAX_DEPTH} " in f.read()
    with open(os.path.join(ORACLE, "ao_oracle.c")) as f:
        assert f"#define O_MAX_DEPTH {AO_MAX_DEPTH}\n" in f.read()


def test_scene_sizes():
    assert (len(S.get("crossing").walls), S.get("crossing").num_texels) == (216, 1512)
    assert len(S.get("tilted56").walls) == 256 and len(S.get("tilted57").walls) == 257
    assert (len(S.get("open_tilted").walls), S.get("open_tilted").num_texels) == (176, 836)
    off = S.get("tilted56").walls[200:]
    assert np.all((np.abs(off["n"][:, :3]) > 1e-3).sum(axis=1) >= 2), "the added rects are off-axis"


def test_crossing_tree_branches():
    """what makes `crossing` worth its name: a later edit of the scene cannot quietly turn it into a chain"""
    nodes = S.decode_tree(O.ao_tree(S.get("crossing")))
    assert sum(1 for left, right, _, _ in nodes if left >= 0 and right >= 0) >= 1, "a node with two children"
    assert sum(1 for left, right, _, items in nodes if left < 0 and right < 0 and items) >= 1, "a leaf with items"
    assert S.tree_depth(nodes) <= AO_MAX_DEPTH
    assert sorted(i for n in nodes for i in n[3]) == list(range(216)), "every wall is in exactly one node"
    box = S.decode_tree(O.ao_tree(scene.box_scene(200, tile_size=S.TILE)))
    assert all(left < 0 or right < 0 for left, right, _, _ in box), "the box alone is a chain"


@pytest.mark.parametrize("name", PINNED + ["tilted57"])
def test_product_bsp_equals_oracle_bsp(name):
    sc = S.get(name)
    assert np.array_equal(fmgi.ao_tree(sc), O.ao_tree(sc))


@pytest.mark.parametrize("name", PINNED)
def test_oracle_reproduces_reference_ao(name):
    ref, sc = _ref(name), S.get(name)
    tex = O.ambient_occlusion(sc)
    first = [float(tex[int(w["lm"][0]), 0]) for w in sc.walls]
    assert first == ref["first_texel_per_wall"]
    assert hashlib.sha256(tex.tobytes()).hexdigest() == ref["sha256_f32"]


@pytest.mark.parametrize("name", ENDLESS)
def test_endless_build_is_an_error_not_a_crash(name):
    """The reference recurses without end on these scenes (a tilted rect off its own plane in fp32 is handed to
    a child with the whole node). Product and oracle stop at the depth bound, within seconds."""
    import ctypes as C

    sc = S.get(name)
    lib = _lib.load()
    O.load()
    t0 = time.perf_counter()
    with pytest.raises(fmgi.FmgiError, match="BSP depth"):
        fmgi.ao_tree(sc)
    with pytest.raises(fmgi.FmgiError, match="BSP depth"):  # an argument error: reported with or without a device
        fmgi.ambient_occlusion(sc)
    g, keep = fmgi.make_geometry(sc, sc.texels())
    assert lib.fmgi_ao_tree(C.byref(g), None, 0) == -3  # FMGI_ERR_ARG
    with pytest.raises(O.BspDepthError, match="BSP depth"):
        O.ao_tree(sc)
    with pytest.raises(O.BspDepthError, match="BSP depth"):
        O.ambient_occlusion(sc)
    assert time.perf_counter() - t0 < 5.0
    assert len(fmgi.ao_tree(S.get("crossing"))) > 0, "the library goes on working"


def test_drop_in_entry_prints_the_depth_and_exits(tmp_path):
    """performAmbientOcclusionGpu has no return value: it prints "[Err] ..." and exits as for its other errors"""
    prog = tmp_path / "ao_dropin.py"
    prog.write_text(
        "import sys; sys.path[:0] = [%r, %r]\n"
        "import ctypes as C\n"
        "import fmgi, offaxis_scenes as S\n"
        "sc = S.get('tilted1')\n"
        "g, keep = fmgi.make_geometry(sc, sc.texels())\n"
        "fmgi._lib.load().performAmbientOcclusionGpu(C.byref(g))\n"
        "print('RETURNED')\n" % (PKG, os.path.join(REPO, "tests"))
    )
    r = subprocess.run([sys.executable, str(prog)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 255, (r.returncode, r.stdout, r.stderr)  # exit(-1), not a signal
    assert "[Err] performAmbientOcclusionGpu" in r.stdout and "BSP depth" in r.stdout
    assert "RETURNED" not in r.stdout


# ---- GPU ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_ao():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = O.ambient_occlusion(S.get(name))
            cache[name].setflags(write=False)
        return cache[name]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", PINNED)
def test_gpu_ao_bitwise_equals_oracle_and_reference(torch_cuda, oracle_ao, name):
    sc = S.get(name)
    got = fmgi.ambient_occlusion(sc)
    exp = oracle_ao(name)
    bad = (got.view(np.uint32) != exp.view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} texels differ, first {np.nonzero(bad)[0][:5]}"
    assert hashlib.sha256(got.tobytes()).hexdigest() == _ref(name)["sha256_f32"]


@pytest.mark.gpu
def test_gpu_ao_wall_range_over_box_walls_and_partitions(torch_cuda, oracle_ao):
    sc = S.get("crossing")
    base = np.random.default_rng(3).random((sc.num_texels, 4), dtype=np.float32)
    part = fmgi.ambient_occlusion(sc, 190, 216, texels=base)
    mask = np.zeros(sc.num_texels, bool)
    for w in sc.walls[190:216]:
        mask[w["lm"][0]: w["lm"][0] + w["lm"][1] * w["lm"][2]] = True
    assert mask.any() and not mask.all()
    assert np.array_equal(part[mask].view(np.uint32), oracle_ao("crossing")[mask].view(np.uint32))
    assert np.array_equal(part[~mask].view(np.uint32), base[~mask].view(np.uint32))
