#!/usr/bin/env python
"""Sparse photon histograms from the bake's deposit codes against the dense route (not the BASELINE
metric).

For box200 (BASELINE config 3) and example.png (config 2) with one group (the whole bake), and example.png with one
group per source, in one process, device times from events on the calls' stream, --reps alternating rounds after
two warm-up rounds, every round running both arms on the same items and launch offsets:

  (A) the dense route: fmgi_bake_states into a zeroed dense histogram (the zeroing is timed apart), then
      fmgi_sparse_measure, then fmgi_sparse_compact;
  (B) fmgi_bake_sparse + fmgi_bake_sparse_take.

Per arm: the median with min and max; the context's bake / fold timers (for B the fold timer is the whole histogram
pass: binning, scatter, both counting passes and the joining of the pieces; the passes are not timed apart); B's
peak scratch bytes and the pool's code bytes; fmgi_sparse_add of the result with itself as the cost of one join.
The blobs of the two arms must be equal. A gain counts when the medians differ by more than the sum of the two
arms' ranges.

  python tools/bench_bake_sparse.py [--configs box200 example example_per_light] [--reps 7] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

from bench_recolour import load_scene, timed  # noqa: E402

# name -> (scene, spa, one group per source)
CONFIGS = {"example": ("example", 6_500_000, False), "box200": ("box200", 172_413_793, False),
           "example_per_light": ("example", 6_500_000, True)}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=sorted(CONFIGS), choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=7, help="timed alternating rounds after two warm-up rounds")
    ap.add_argument("--out", default=None, help="directory for bake_sparse_<config>.json")
    a = ap.parse_args()
    import numpy as np
    import torch

    import fmgi
    from relight import source_groups

    offsets = np.load(os.path.join(REPO, "tests", "golden", "glibc_rand_4096.npy"))
    for name in a.configs:
        sname, spa, per_light = CONFIGS[name]
        sc = load_scene(sname)
        T = sc.num_texels
        ctx = fmgi.Context(0)
        ctx.set_scene(sc)
        items = ctx.plan(spa, rng_offsets=offsets)
        if not ctx.bake_sparse_supported():
            raise SystemExit(f"{name}: fmgi_bake_sparse cannot serve {T} texels")
        groups = source_groups(ctx.source_ranges(), True) if per_light else [("all", 0, items, False)]
        s = torch.cuda.Stream(device="cuda:0")
        res = {"metric": "sparse histograms from deposit codes (B) against bake_states + measure + compact (A), ms",
               "config": name, "texels": T, "photons": 100 * items, "groups": len(groups),
               "dense_bytes": fmgi.states_bytes(T), "n_gpus": 1}
        ctx.set_timing(True)
        with torch.cuda.stream(s):
            dense = torch.zeros((1024, T), dtype=torch.int64, device="cuda:0")
            blobs = {"A": [None] * len(groups), "B": [None] * len(groups)}
            infos = {"A": [None] * len(groups), "B": [None] * len(groups)}
            peak = codes = dense_chunks = 0

            def arm_a():
                for g, (_, b, e, _) in enumerate(groups):
                    dense.zero_()
                    ctx.bake_states(b, e, dense.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
                    i = ctx.sparse_measure(dense.data_ptr(), s.cuda_stream)
                    blob = torch.empty(fmgi.sparse_bytes(T, i.rows) // 8, dtype=torch.int64, device="cuda:0")
                    ctx.sparse_compact(dense.data_ptr(), i, blob.data_ptr(), s.cuda_stream)
                    blobs["A"][g], infos["A"][g] = blob, i

            def arm_b():
                nonlocal peak, codes, dense_chunks
                codes = 0
                for g, (_, b, e, _) in enumerate(groups):
                    i = ctx.bake_sparse(b, e, fmgi.KERNEL_AUTO, s.cuda_stream)
                    blob = torch.empty(fmgi.sparse_bytes(T, i.rows) // 8, dtype=torch.int64, device="cuda:0")
                    ctx.bake_sparse_take(i, blob.data_ptr(), s.cuda_stream)
                    blobs["B"][g], infos["B"][g] = blob, i
                    st = ctx.bake_sparse_stats()
                    peak, codes, dense_chunks = max(peak, st["scratch_bytes"]), codes + st["codes"], dense_chunks + st["dense_chunks"]

            ms = {"A": [], "B": []}
            tm = {"A": [], "B": []}
            for r in range(2 + a.reps):  # alternating rounds
                for arm, fn in (("A", arm_a), ("B", arm_b)):
                    ctx.timing()
                    x = timed(torch, s, fn, 0, 1)
                    t = ctx.timing()
                    if r >= 2:
                        ms[arm] += x
                        tm[arm].append(t)
            zero_ms = timed(torch, s, lambda: dense.zero_(), 1, 3)
            s.synchronize()
            same = all(x == y for x, y in zip(infos["A"], infos["B"])) and \
                all(torch.equal(x, y) for x, y in zip(blobs["A"], blobs["B"]))
            # one join: the first group's blob added to itself
            b0, i0 = blobs["B"][0], infos["B"][0]

            def join():
                si = ctx.sparse_add_measure(b0.data_ptr(), i0, b0.data_ptr(), i0, s.cuda_stream)
                out = torch.empty(fmgi.sparse_bytes(T, si.rows) // 8, dtype=torch.int64, device="cuda:0")
                ctx.sparse_add(b0.data_ptr(), i0, b0.data_ptr(), i0, si, out.data_ptr(), s.cuda_stream)

            add_ms = timed(torch, s, join, 1, a.reps)
        for arm in ("A", "B"):
            res[f"{arm}_ms"] = spread(ms[arm])
            res[f"{arm}_bake_ms"] = spread([t["bake_ms"] for t in tm[arm]])
            res[f"{arm}_fold_ms"] = spread([t["fold_ms"] for t in tm[arm]])
        gap = res["A_ms"]["median"] - res["B_ms"]["median"]
        ranges = sum(res[f"{k}_ms"]["max"] - res[f"{k}_ms"]["min"] for k in ("A", "B"))
        res.update({"blobs_equal": bool(same), "A_zero_ms": statistics.median(zero_ms), "add_ms": spread(add_ms),
                    "A_over_B": res["A_ms"]["median"] / res["B_ms"]["median"],
                    "B_gain_counts": bool(gap > ranges), "A_gain_counts": bool(-gap > ranges),
                    "B_peak_scratch_bytes": peak, "B_pool_code_bytes": 4 * codes, "B_dense_chunks": dense_chunks,
                    "sparse_bytes": sum(fmgi.sparse_bytes(T, i.rows) for i in infos["B"]),
                    "deposits": sum(i.deposits for i in infos["B"]), "cells": sum(i.cells for i in infos["B"])})
        del dense, blobs
        ctx.close()
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"bake_sparse_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        if not same:
            raise SystemExit(f"{name}: the two arms' blobs differ")


if __name__ == "__main__":
    main()
