"""Pin the oracle against the REFERENCE KERNEL ITSELF (run on the GPU box; outputs are committed).

The reference's photonmap.cl, compiled for gfx950 by oracle/build_ref.sh with ROCm's OpenCL device
libraries, is launched one work item at a time on a zeroed lightColors buffer (oracle/ref_runner.cpp;
one item per launch removes the kernel's data race, photonmap.cl:256). Each item's fp32 lightmap is
stored sparsely as a fixture and compared with the oracle's fp32 per-item sum (fm_oracle.trace_item_f32):

  ref_items_<scene>_<variant>.npz : rng_state[n], source, is_window, and for every item the non-zero
                                    texel indices and their float4 values (reference kernel output)

variant "strict": -cl-fp32-correctly-rounded-divide-sqrt -ffp-contract=off (IEEE, the oracle contract)
variant "relaxed": -cl-unsafe-math-optimizations (mad/contraction, relaxed div/sqrt, no signed zeros):
                  the reference's own -cl-fast-relaxed-math (global_illumination_cl.c:196) minus
                  finite-math-only, which makes photonmap.cl:208 undefined (escaping photons fault) --
                  quantifies how far a relaxed-math build of the reference drifts from an exact one.
Prints a JSON summary (items bit-identical to the oracle, max relative texel difference).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "oracle"), os.path.join(REPO, "flatmatch-global-illumination_amd"),
                os.path.join(REPO, "tests")]

import bake_scenes  # noqa: E402
import emitter_scenes  # noqa: E402
import fm_oracle as O  # noqa: E402
from fmgi import scene as S  # noqa: E402


def run(sc, L, li, gids, variant):
    src, isw = int(L[li]["source"]), int(L[li]["is_window"])
    states = np.array([(g + int(L[li]["rng_offset"])) & 0xFFFFFFFF for g in gids], np.uint32)
    ref = O.ref_run_items(sc, src, isw, states, variant)
    idx, vals, bounds = [], [], [0]
    same, maxrel = 0, 0.0
    for k, st in enumerate(states):
        nz = np.nonzero(ref[k].any(axis=1))[0]
        idx.append(nz)
        vals.append(ref[k][nz])
        bounds.append(bounds[-1] + len(nz))
        mine = O.trace_item_f32(sc, src, isw, int(st))
        if np.array_equal(mine.view(np.uint32), ref[k].view(np.uint32)):
            same += 1
        tot_m, tot_r = mine[:, :3].sum(), ref[k][:, :3].sum()
        maxrel = max(maxrel, abs(float(tot_m) - float(tot_r)) / max(float(tot_r), 1e-30))
    return dict(rng_state=states, source=src, is_window=isw, bounds=np.array(bounds, np.int64),
                texel=np.concatenate(idx).astype(np.int32), value=np.concatenate(vals).astype(np.float32)), same, maxrel


def main():
    offs = np.load(os.path.join(HERE, "glibc_rand_4096.npy"))
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    summary = {}
    example = S.load_geometry(os.path.join(HERE, "example_geometry.bin"), "example")
    apartment = S.load_geometry(os.path.join(HERE, "apartment30_geometry.bin"), "apartment30")
    both = ("strict", "relaxed")
    cases = [  # (fixture name, scene, spa, [(launch index, gids)], variants)
        ("example", example, 65_000, [(0, range(0, 96)), (7, range(0, 32))], both),
        ("box200", S.box_scene(200), 172_413_793, [(0, range(1000, 1048))], both),
        # BASELINE config 2 schedule (43 launches): late launches, rng offsets deep in the glibc prefix
        ("example_late", example, 6_500_000, [(40, range(0, 32)), (42, range(10_400, 10_432))], both),
        # BASELINE config 4 schedule (3,907 launches): the last two launches
        ("box200_late", S.box_scene(200), 1_724_137_931, [(3905, range(0, 32)), (3906, range(6_600, 6_632))], both),
        # BASELINE config 5 (2000 rects): the first and the last launch
        ("box2000", S.box_scene(2000), 172_413_793, [(0, range(1000, 1032)), (390, range(16_000, 16_032))], both),
        # generated 30-room layout (654 walls, 34 sources): a window launch and the last light launch
        ("apartment30", apartment, 3_000_000, [(0, range(0, 32)), (77, range(19_900, 19_932))], both),
    ]
    # tests/bake_scenes.py (strict only): most photons escaping, rects that are not axis-aligned, and 15 coincident
    # rects, whose hits the kernel's index-order scan gives to the first of them
    cases += [(name, bake_scenes.get(name), bake_scenes.SPA, [(0, range(0, 32))], ("strict",))
              for name in ("open_box", "tilted12", "stacked14")]
    # tests/emitter_scenes.py (strict only): gids 0..31 of the first launch of every source: windows and lights through
    # either branch of the sampler basis, emitters without a zero component, and first rays from outside the walls
    for name in ("lamps", "tilted_emitters", "threshold", "outside"):
        sc = emitter_scenes.get(name)
        L = O.schedule_with_offsets(sc, bake_scenes.SPA, offs)
        firsts = [int(np.flatnonzero(L["source"] == s)[0]) for s in range(len(sc.sources))]
        cases.append((name, sc, bake_scenes.SPA, [(li, range(0, 32)) for li in firsts], ("strict",)))
    only = os.environ.get("FMGI_REF_CASES")  # e.g. "box2000,apartment30": regenerate a subset
    if only:
        cases = [c for c in cases if c[0] in only.split(",")]
    for name, sc, spa, parts, variants in cases:
        L = O.schedule_with_offsets(sc, spa, offs)
        for variant in variants:
            acc = {}
            n_same = n_tot = 0
            worst = 0.0
            for li, gids in parts:
                d, same, maxrel = run(sc, L, li, list(gids), variant)
                for k, v in d.items():
                    acc.setdefault(k, []).append(v)
                n_same += same
                n_tot += len(gids)
                worst = max(worst, maxrel)
            np.savez_compressed(os.path.join(out_dir, f"ref_items_{name}_{variant}.npz"),
                                **{f"{k}_{i}": v for k, vs in acc.items() for i, v in enumerate(vs)})
            summary[f"{name}/{variant}"] = {"items": n_tot, "bit_identical_to_oracle": n_same,
                                            "max_rel_item_total_diff": worst}
    print(json.dumps(summary, indent=1))
    path = os.path.join(out_dir, "ref_items_summary.json")
    if only and os.path.exists(path):  # keep the entries of the cases not regenerated
        old = json.load(open(path))
        old.update(summary)
        summary = old
    with open(path, "w") as f:
        json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
