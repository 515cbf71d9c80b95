"""The oracle pinned against the REFERENCE KERNEL's own output (CPU test over committed fixtures).

tests/golden/ref_items_<case>_<variant>.npz were produced on an MI355X by make_ref_fixtures.py: the
reference photonmap.cl, compiled for gfx950 with ROCm's OpenCL device libraries (oracle/build_ref.sh),
launched one work item per launch on a zeroed lightColors buffer. Here the oracle's fp32 per-item sum
(fm_oracle.trace_item_f32: the same deposits added in the same order) must reproduce those lightmaps:
  strict  (IEEE div/sqrt, no contraction = the oracle contract, with the OpenCL builtins as ROCm builds
          them for gfx950): every item bit for bit -- 912 items over twelve scenes: example.png (configs 1
          and 2, incl. the config-2 schedule's last launches), box200 (config 3 and the last launches of config 4),
          box2000 (config 5), the generated 30-room layout, and 32 items each of three scenes of
          tests/bake_scenes.py (strict only): open_box (most photons escape, photonmap.cl:208), tilted12 (rects
          that are not axis-aligned) and stacked14 (15 coincident rects: the index-order scan's strict
          `d < closest`, photonmap.cl:189-206, gives every hit to the first), and 32 items of every source of four
          scenes of tests/emitter_scenes.py (strict only): lamps (96: lights through either branch of the sampler
          basis, photonmap.cl:65-70), tilted_emitters (64: width, height and n without a zero component in
          photonmap.cl:27-74 and :181), threshold (128: |n.z| on either side of 0.999999f) and outside (96: first
          rays from outside the walls, a lamp that straddles the ceiling);
  relaxed (-cl-unsafe-math-optimizations): the same deposit totals, most items bit for bit -- relaxed
          math moves a few hit points across texel boundaries, it does not change colours.
"""
import os

import numpy as np
import pytest

import fm_oracle as O
from conftest import GOLDEN


def _items(path):
    d = np.load(path)
    parts = sorted({int(k.rsplit("_", 1)[1]) for k in d.keys()})
    for p in parts:
        b = d[f"bounds_{p}"]
        for k, st in enumerate(d[f"rng_state_{p}"]):
            yield (int(d[f"source_{p}"]), int(d[f"is_window_{p}"]), int(st),
                   d[f"texel_{p}"][b[k] : b[k + 1]], d[f"value_{p}"][b[k] : b[k + 1]])


def _scene(name, example_scene, box200, box2000):
    from fmgi import scene

    if name in ("open_box", "tilted12", "stacked14"):
        import bake_scenes

        return bake_scenes.get(name)
    if name in ("lamps", "tilted_emitters", "threshold", "outside"):
        import emitter_scenes

        return emitter_scenes.get(name)
    if name == "apartment30":
        return scene.load_geometry(os.path.join(GOLDEN, "apartment30_geometry.bin"), "apartment30")
    return {"example": example_scene, "example_late": example_scene, "box200": box200, "box200_late": box200,
            "box2000": box2000}[name]


# (fixture, items): launches 0/7 of config 1 and item 1000.. of config 3 (round 1); late launches of the
# config-2 and config-4 schedules (rng offsets deep in the glibc prefix), the first and last launch of
# config 5 (box2000) and the generated 30-room layout (round 2); launch 0, gids 0..31 of an open box, a box with
# tilted rects and a box with 15 coincident floors (tests/bake_scenes.py); gids 0..31 of the first launch of every
# source of four scenes of tests/emitter_scenes.py
PINNED = [("example", 128), ("box200", 48), ("example_late", 64), ("box200_late", 64), ("box2000", 64),
          ("apartment30", 64), ("open_box", 32), ("tilted12", 32), ("stacked14", 32),
          ("lamps", 96), ("tilted_emitters", 64), ("threshold", 128), ("outside", 96)]


def test_pinned_item_count():
    assert sum(n for _, n in PINNED) == 912  # the figure README.md and DESIGN.md §2 quote


@pytest.mark.parametrize("name,n_items", PINNED)
def test_oracle_reproduces_reference_kernel_strict(name, n_items, example_scene, box200, box2000):
    sc = _scene(name, example_scene, box200, box2000)
    seen = 0
    for src, isw, st, tex, val in _items(os.path.join(GOLDEN, f"ref_items_{name}_strict.npz")):
        mine = O.trace_item_f32(sc, src, isw, st)
        nz = np.nonzero(mine.any(axis=1))[0]
        assert np.array_equal(nz, tex), f"item rng={st}: deposits on different texels"
        assert np.array_equal(mine[nz].view(np.uint32), val.view(np.uint32)), f"item rng={st}: values differ"
        seen += 1
    assert seen == n_items


@pytest.mark.parametrize("name,min_identical", [("example", 120), ("box200", 42), ("example_late", 56),
                                                 ("box200_late", 56), ("box2000", 56), ("apartment30", 56)])
def test_relaxed_math_reference_stays_close(name, min_identical, example_scene, box200, box2000):
    sc = _scene(name, example_scene, box200, box2000)
    same = total = 0
    for src, isw, st, tex, val in _items(os.path.join(GOLDEN, f"ref_items_{name}_relaxed.npz")):
        mine = O.trace_item_f32(sc, src, isw, st)
        ref = np.zeros_like(mine)
        ref[tex] = val
        same += np.array_equal(mine.view(np.uint32), ref.view(np.uint32))
        np.testing.assert_allclose(mine[:, :3].sum(axis=0), ref[:, :3].sum(axis=0), rtol=1e-6)
        total += 1
    assert same >= min_identical, f"{same}/{total}"
