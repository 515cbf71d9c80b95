#!/usr/bin/env python
"""Adaptive density filter measurement (not the BASELINE metric).

For example.png (113,964 texels) and box200 (92,824 texels), in one process, device times from events on the
calls' stream, medians after warm-up rounds, the kinds of call interleaved within a round:

  * fmgi_filter_radii (min_energy = fmgi_filter_energy(--min-deposits), radius <= --max-radius) on a low-photon
    bake of the scene (example: BASELINE config 1, spa 65,000; box200: a thousandth of config 3);
  * fmgi_filter_apply of 1 and of 8 lightmaps with those radii;
  * the yardsticks: a device-to-device copy of one and of eight lightmaps, and the low-photon fmgi_bake_items
    itself (for example.png that is config 1's bake: radii + a one-map apply must stay well below it).

Bytes are computed from the shapes: the compulsory traffic (the guide or the maps in, the radii or the maps
out) and the scratch traffic of the prefix sums (rows written, columns read and written, four lookups per window).
The device result is checked against itself: radii all zero must give out == in.

  python tools/bench_filter.py [--configs example box200] [--reps 15] [--batch 20] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd")]

CONFIGS = {"example": ("example", 65_000), "box200": ("box200", 172_414)}


def load_scene(name):
    from fmgi import scene

    if name == "example":
        return scene.load_geometry(os.path.join(REPO, "tests", "golden", "example_geometry.bin"), "example")
    return scene.box_scene(int(name[3:]))


def timed(torch, stream, fn, batch=1):
    """device ms per fn() on `stream`: `batch` calls between one pair of events (a call of some 20 us is too
    short for a pair of its own)"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(batch):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["example", "box200"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20, help="calls per pair of events (the bake: one)")
    ap.add_argument("--min-deposits", type=int, default=256)
    ap.add_argument("--max-radius", type=int, default=4)
    ap.add_argument("--out", default=None, help="directory for filter_<config>.json")
    a = ap.parse_args()
    import torch

    import fmgi

    med = statistics.median
    for name in a.configs:
        sname, spa = CONFIGS[name]
        sc = load_scene(sname)
        T = sc.num_texels
        T0 = int(sc.level0_mask().sum())
        ctx = fmgi.Context(0)
        ctx.set_scene(sc)
        items = ctx.plan(spa)
        s = torch.cuda.Stream(device="cuda:0")
        E = fmgi.filter_energy(a.min_deposits)
        with torch.cuda.stream(s):
            lm = torch.zeros((T, 4), dtype=torch.int64, device="cuda:0")
            ctx.bake_items(0, items, lm.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            scratch = torch.zeros_like(lm)
            maps = torch.stack([lm * (k + 1) for k in range(8)])
            outs = torch.zeros_like(maps)
            copy1, copy8 = torch.empty_like(lm), torch.empty_like(maps)
            radii = torch.zeros(T, dtype=torch.uint8, device="cuda:0")
            zero_radii = torch.zeros(T, dtype=torch.uint8, device="cuda:0")
            in8, out8 = [m.data_ptr() for m in maps], [o.data_ptr() for o in outs]
            st = s.cuda_stream

            def bake():
                scratch.zero_()
                ctx.bake_items(0, items, scratch.data_ptr(), fmgi.KERNEL_AUTO, st)

            calls = {
                "radii": lambda: ctx.filter_radii(lm.data_ptr(), E, a.max_radius, radii.data_ptr(), st),
                "apply_k1": lambda: ctx.filter_apply(radii.data_ptr(), in8[:1], out8[:1], st),
                "apply_k8": lambda: ctx.filter_apply(radii.data_ptr(), in8, out8, st),
                "copy_k1": lambda: copy1.copy_(lm),
                "copy_k8": lambda: copy8.copy_(maps),
                "bake": bake,
            }
            ms = {k: [] for k in calls}
            for i in range(a.warmup + a.reps):
                for k, fn in calls.items():
                    x = timed(torch, s, fn, 1 if k == "bake" else a.batch)
                    if i >= a.warmup:
                        ms[k].append(x)
            # radii all zero: out == in
            ctx.filter_apply(zero_radii.data_ptr(), in8, out8, st)
            s.synchronize()
            identity = bool(torch.equal(outs, maps))
            ctx.filter_apply(radii.data_ptr(), in8, out8, st)
            s.synchronize()
            rad = radii.cpu().numpy()
        res = {"metric": "adaptive density filter: ms per call against a copy and the low-photon bake",
               "config": name, "texels": T, "level0_texels": T0, "spa": spa, "photons": 100 * items, "n_gpus": 1,
               "min_deposits": a.min_deposits, "max_radius": a.max_radius, "calls_per_event_pair": a.batch, "mean_radius": float(rad.mean()),
               "radius_histogram": [int(v) for v in np.bincount(rad, minlength=a.max_radius + 1)],
               "zero_radii_give_the_input": identity, "bake_kernel": ctx.last_bake_kernel}
        for k, v in ms.items():
            res[f"{k}_ms"] = med(v)
            res[f"{k}_ms_min"] = min(v)
        res["radii_plus_apply_k1_ms"] = res["radii_ms"] + res["apply_k1_ms"]
        res["radii_plus_apply_k1_over_bake"] = res["radii_plus_apply_k1_ms"] / res["bake_ms"]
        # bytes from the shapes. compulsory: what any filter must move; scratch: the prefix sums' own traffic
        # (per plane: rows write T words, columns read and write T0 words, at most four lookups per window)
        res["radii_compulsory_bytes"] = 32 * T + T
        res["radii_scratch_bytes"] = 8 * (T + 2 * T0 + 4 * (a.max_radius + 1) * T0)
        for K in (1, 8):
            res[f"apply_k{K}_compulsory_bytes"] = K * 64 * T + T
            res[f"apply_k{K}_scratch_bytes"] = 3 * K * 8 * (T + 2 * T0 + 4 * T0)
            res[f"apply_k{K}_compulsory_bytes_per_s"] = res[f"apply_k{K}_compulsory_bytes"] / (res[f"apply_k{K}_ms"] / 1e3)
            res[f"copy_k{K}_bytes_per_s"] = K * 64 * T / (res[f"copy_k{K}_ms"] / 1e3)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"filter_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        del lm, scratch, maps, outs, copy1, copy8
        ctx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
