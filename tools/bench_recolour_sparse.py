#!/usr/bin/env python
"""Sparse photon histograms: size and speed against the dense form (not the BASELINE metric).

For example.png (BASELINE config 2) and box200 (config 3) with one group (the whole bake), and example.png with one
group per source (--per-light's groups), in one process, device times from events on the calls' stream, medians of
--recolour-reps rounds after two warm-up rounds, the kinds of call interleaved inside a round:

  * the blobs: bytes, rows, cells and fill (cells / slots) against fmgi_states_bytes;
  * fmgi_sparse_measure + fmgi_sparse_compact of every group against one dense fmgi_recolour (K = 1) and against
    the histogram bake (fmgi_bake_states, median of --reps);
  * fmgi_recolour_sparse with K = 1 and K = 8 against fmgi_recolour with K = 1 and K = 8 on the same histograms in
    the same rounds, and the bytes each reads over its time as a share of the 8 TB/s HBM peak;
  * with --relight: tools/relight.py --load-bake end to end (wall clock of the process) against a run that traces.

The four timed kinds are checked: on fresh lightmaps the sparse results must equal the dense ones bit for bit.

  python tools/bench_recolour_sparse.py [--configs example box200 example_per_light] [--relight] [--out DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

from bench_recolour import HBM_PEAK, load_scene, timed  # noqa: E402

# name -> (scene, spa, one group per source)
CONFIGS = {"example": ("example", 6_500_000, False), "box200": ("box200", 172_413_793, False),
           "example_per_light": ("example", 6_500_000, True)}


def relight_end_to_end(spa, per_light):
    """wall-clock seconds of relight.py on example.png, one scenario: tracing (and saving), then loading"""
    scene = os.path.join(REPO, "tests", "golden", "example_geometry.bin")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "s.json"), "w") as f:
            json.dump([{"name": "day"}], f)
        base = [sys.executable, os.path.join(REPO, "tools", "relight.py"), scene, "--scenarios", os.path.join(d, "s.json")]
        # the recorded launch offsets: every tracing process then traces the same photons (with libc rand() two
        # processes need not), so the three runs' files can be compared
        offsets = ["--offsets", os.path.join(REPO, "tests", "golden", "glibc_rand_4096.npy")]
        bake = os.path.join(d, "bake.npz")
        runs = (("trace_dense", ["--spa", str(spa)] + offsets),
                ("trace_sparse_save", ["--spa", str(spa), "--save-bake", bake] + offsets), ("load", ["--load-bake", bake]))
        for name, extra in runs:
            extra = extra + (["--per-light"] if per_light and name != "load" else []) + ["-o", os.path.join(d, name)]
            t0 = time.perf_counter()
            r = subprocess.run(base + extra, capture_output=True, text=True)
            out[f"relight_{name}_wall_s"] = time.perf_counter() - t0
            if r.returncode != 0:
                raise SystemExit(f"relight {name} failed:\n{r.stdout}{r.stderr}")
            out[f"relight_{name}_traced_nothing"] = " 0 items traced" in r.stdout
        out["bake_file_bytes"] = os.path.getsize(bake)
        same = all(open(os.path.join(d, "trace_dense", "day", f), "rb").read() == open(os.path.join(d, n, "day", f), "rb").read()
                   for n in ("trace_sparse_save", "load") for f in ("texels.npy", "tiles.npy"))
        out["relight_outputs_identical"] = bool(same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=sorted(CONFIGS), choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=3, help="timed histogram bakes of each group")
    ap.add_argument("--recolour-reps", type=int, default=15)
    ap.add_argument("--relight", action="store_true", help="also time tools/relight.py end to end on example.png")
    ap.add_argument("--out", default=None, help="directory for sparse_<config>.json")
    a = ap.parse_args()
    import torch

    import fmgi
    from relight import source_groups

    med = statistics.median
    for name in a.configs:
        sname, spa, per_light = CONFIGS[name]
        sc = load_scene(sname)
        T = sc.num_texels
        ctx = fmgi.Context(0)
        ctx.set_scene(sc)
        items = ctx.plan(spa)
        groups = source_groups(ctx.source_ranges(), True) if per_light else [("all", 0, items, False)]
        G = len(groups)
        s = torch.cuda.Stream(device="cuda:0")
        res = {"metric": "sparse histograms: bytes and ms against the dense form", "config": name, "texels": T,
               "photons": 100 * items, "groups": G, "dense_bytes": G * fmgi.states_bytes(T), "n_gpus": 1}
        with torch.cuda.stream(s):
            hists = [torch.zeros((1024, T), dtype=torch.int64, device="cuda:0") for _ in groups]
            bake_ms = 0.0
            for h, (_, b, e, _) in zip(hists, groups):
                ms = []
                for _ in range(1 + a.reps):  # the first is the warm-up; every bake starts from zeros
                    h.zero_()
                    ms += timed(torch, s, lambda: ctx.bake_states(b, e, h.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream), 0, 1)
                bake_ms += med(ms[1:])
            infos = [ctx.sparse_measure(h.data_ptr(), s.cuda_stream) for h in hists]
            blobs = [torch.empty(fmgi.sparse_bytes(T, i.rows) // 8, dtype=torch.int64, device="cuda:0") for i in infos]

            def compact_all():
                for h, b in zip(hists, blobs):
                    i = ctx.sparse_measure(h.data_ptr(), s.cuda_stream)
                    ctx.sparse_compact(h.data_ptr(), i, b.data_ptr(), s.cuda_stream)

            compact_all()
            pals = [[fmgi.Palette(window_rgb=(18 - k, 18 - 2 * k, 18), light_rgb=(16, 16 - k, 18 - k),
                                  floor_tint=(1.0, 0.85 - 0.05 * k, 0.7), albedo=0.9 - 0.02 * k)] * G for k in range(8)]
            hp, bp = [h.data_ptr() for h in hists], [b.data_ptr() for b in blobs]

            def lightmaps():
                return [torch.zeros((T, 4), dtype=torch.int64, device="cuda:0") for _ in range(8)]

            lms = lightmaps()
            lp = [m.data_ptr() for m in lms]
            kinds = {"dense_k1": lambda: ctx.recolour(hp, pals[:1], lp[:1], s.cuda_stream),
                     "sparse_k1": lambda: ctx.recolour_sparse(bp, infos, pals[:1], lp[:1], s.cuda_stream),
                     "dense_k8": lambda: ctx.recolour(hp, pals, lp, s.cuda_stream),
                     "sparse_k8": lambda: ctx.recolour_sparse(bp, infos, pals, lp, s.cuda_stream),
                     "measure_compact": compact_all}
            ms = {k: [] for k in kinds}
            for i in range(2 + a.recolour_reps):  # interleaved rounds
                for k, fn in kinds.items():
                    x = timed(torch, s, fn, 0, 1)
                    if i >= 2:
                        ms[k] += x
            # the check: fresh lightmaps, sparse against dense, K = 1 and K = 8
            same = True
            for K in (1, 8):
                d, sp = lightmaps()[:K], lightmaps()[:K]
                ctx.recolour(hp, pals[:K], [m.data_ptr() for m in d], s.cuda_stream)
                ctx.recolour_sparse(bp, infos, pals[:K], [m.data_ptr() for m in sp], s.cuda_stream)
                s.synchronize()
                same = same and all(torch.equal(x, y) for x, y in zip(d, sp)) and bool(d[0].any().item())
        sparse_bytes = sum(fmgi.sparse_bytes(T, i.rows) for i in infos)
        cells, rows = sum(i.cells for i in infos), sum(i.rows for i in infos)
        res.update({
            "sparse_equals_dense": bool(same),
            "sparse_bytes": sparse_bytes, "sparse_over_dense_bytes": sparse_bytes / res["dense_bytes"],
            "rows": rows, "cells": cells, "fill": cells / max(64 * rows, 1),
            "cells_over_dense_cells": cells / (G * 1024 * T), "deposits": sum(i.deposits for i in infos),
            "bake_states_ms": bake_ms,
            "measure_compact_ms": med(ms["measure_compact"]),
            "measure_compact_over_dense_recolour_k1": med(ms["measure_compact"]) / med(ms["dense_k1"]),
            "measure_compact_over_bake_states": med(ms["measure_compact"]) / bake_ms,
        })
        for k in ("dense_k1", "sparse_k1", "dense_k8", "sparse_k8"):
            nbytes = res["dense_bytes"] if k.startswith("dense") else sparse_bytes
            res[f"{k}_ms"], res[f"{k}_ms_min"] = med(ms[k]), min(ms[k])
            res[f"{k}_bytes_per_s"] = nbytes / (med(ms[k]) / 1e3)
            res[f"{k}_fraction_of_hbm_peak"] = nbytes / (med(ms[k]) / 1e3) / HBM_PEAK
        res["sparse_over_dense_k1_ms"] = res["sparse_k1_ms"] / res["dense_k1_ms"]
        res["sparse_over_dense_k8_ms"] = res["sparse_k8_ms"] / res["dense_k8_ms"]
        del hists, blobs, lms
        ctx.close()
        torch.cuda.empty_cache()
        if a.relight and sname == "example":
            res.update(relight_end_to_end(spa, per_light))
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"sparse_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
