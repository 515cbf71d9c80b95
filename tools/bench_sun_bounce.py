#!/usr/bin/env python
"""Bounced-sun measurement (not the BASELINE metric).

For example.png and box200 at 200 texels/m²: a RadCache of the scene is traced once, --directions sun directions of a
day's arc (tools/bench_sun.py's) get their coverage maps at --samples x --samples rays per texel, and --bounces bounces
of all of them are gathered.
  arm B: one sun_bounce call of all the directions (4 B per texel and direction: 32 directions share a 128-B line)
  arm A: what the same directions would cost as palettes: directions / 8 RadCache.solve calls of 8 sets with
         iterations = --bounces on the same cache (16 B per texel and set). Its results are not compared: it is the
         radiosity solve's gather at the same number of values.
One process, two warm-up rounds, then --rounds rounds with the arms alternating; HIP events on the calls' stream around
each arm; median (min-max) in ms, and ms per bounce and direction. Then sun_bounce alone at K = 1, 8 and all, and
fmgi_sun_add_bounced for one map and for eight (median of --reps batches of --batch calls).

  python tools/bench_sun_bounce.py [--scenes example box200] [--directions 32] [--samples 4] [--bounces 3] [--out DIR]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def fmt(s):
    return f"{s['median']:.3f} ({s['min']:.3f}-{s['max']:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["example", "box200"])
    ap.add_argument("--directions", type=int, default=32)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=3)
    ap.add_argument("--peak", type=float, default=60.0, help="the arc's highest elevation in degrees")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--batch", type=int, default=20, help="fmgi_sun_add_bounced calls per pair of events")
    ap.add_argument("--out", default=None, help="directory for sun_bounce_<scene>.json")
    a = ap.parse_args()
    import torch

    import fmgi
    from bench_sun import day_arc, load_scene

    dev = "cuda:0"
    libc = ctypes.CDLL(None)
    libc.srand.argtypes = [ctypes.c_uint]
    K, S, N = a.directions, a.samples, a.bounces
    for name in a.scenes:
        sc = load_scene(name)
        T = sc.num_texels
        ctx = fmgi.Context(0)
        ctx.set_scene(sc)
        libc.srand(1)
        rc = fmgi.RadCache(sc)
        info = rc.info
        dirs = day_arc(K, a.peak)
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            covers = [torch.empty(max(T, 1), dtype=torch.uint8, device=dev) for _ in dirs]
            for d, c in zip(dirs, covers):
                ctx.sun_coverage(d, S, c.data_ptr(), stream=s.cuda_stream)
        s.synchronize()
        lit = [int((c > 0).sum().item()) for c in covers]
        emit = np.random.default_rng(5).uniform(0.05, 30.0, (8, rc.emitters, 3)).astype(np.float32)
        res = {"scene": sc.name, "walls": len(sc.walls), "texels": T, "info": info, "samples": S, "directions": K,
               "bounces": N, "lit_texels_per_direction": {"min": min(lit), "max": max(lit)}}

        def arm_a():
            return [rc.solve(emit, N, stream=s) for _ in range((K + 7) // 8)]

        def arm_b(k=K):
            return rc.sun_bounce(covers[:k], dirs[:k], S, N, stream=s)

        def timed(fn):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            s.synchronize()
            ev[0].record(s)
            out = fn()
            ev[1].record(s)
            s.synchronize()
            del out
            return ev[0].elapsed_time(ev[1])

        ta, tb = [], []
        for r in range(2 + a.rounds):
            for arm in ((arm_a, arm_b) if r % 2 == 0 else (arm_b, arm_a)):
                ms = timed(arm)
                if r >= 2:
                    (ta if arm is arm_a else tb).append(ms)
        A, B = spread(ta), spread(tb)
        res.update({"A_ms": A, "B_ms": B, "A_over_B": A["median"] / B["median"],
                    "B_beats_A_by_more_than_the_ranges": A["median"] - B["median"] > (A["max"] - A["min"]) + (B["max"] - B["min"]),
                    "A_ms_per_bounce_and_direction": A["median"] / N / K, "B_ms_per_bounce_and_direction": B["median"] / N / K})
        for k in sorted({1, min(8, K), K}):
            t = [timed(lambda: arm_b(k)) for _ in range(2 + a.rounds)][2:]
            res[f"sun_bounce_K{k}_ms"] = spread(t)

        # a first-bounce table that holds light, for the add
        g = arm_b(K)
        s.synchronize()
        best = int(np.argmax(lit))
        res["g1_max"] = float(g[best, 0].max().item())
        for M in (1, 8):
            with torch.cuda.stream(s):
                lms = [torch.zeros((T, 4), dtype=torch.int64, device=dev) for _ in range(M)]
            ptrs = [lm.data_ptr() for lm in lms]
            times = []
            for rep in range(a.reps + 2):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(s)
                for _ in range(a.batch):
                    ctx.sun_add_bounced(g[best].data_ptr(), N, [[30.0, 28.0, 24.0]] * M, [[0.9, 0.9, 0.9]] * M, 65000.0, ptrs,
                                        s.cuda_stream)
                t1.record(s)
                t1.synchronize()
                if rep >= 2:
                    times.append(t0.elapsed_time(t1) / a.batch)
            res[f"add_bounced_{M}_ms"] = statistics.median(times)
        rc.close()
        ctx.close()

        print(f"{sc.name}: {info['jobs']} jobs, {T} texels, {K} directions at S = {S}, {N} bounces")
        print(f"  A, {(K + 7) // 8} solve calls of 8 sets: {fmt(A)} ms, {res['A_ms_per_bounce_and_direction']:.4f} ms per bounce "
              f"and direction")
        print(f"  B, one sun_bounce call:      {fmt(B)} ms, {res['B_ms_per_bounce_and_direction']:.4f} ms per bounce and "
              f"direction; A / B = {res['A_over_B']:.2f}, beats A by more than the ranges: "
              f"{res['B_beats_A_by_more_than_the_ranges']}")
        print("  sun_bounce alone: " + ", ".join(f"K = {k[12:-3]}: {fmt(v)} ms" for k, v in res.items()
                                                  if k.startswith("sun_bounce_K")))
        print(f"  fmgi_sun_add_bounced: {res['add_bounced_1_ms'] * 1e3:.1f} us for one map, "
              f"{res['add_bounced_8_ms'] * 1e3:.1f} us for eight; the largest g_1 is {res['g1_max']:.4f}")
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"sun_bounce_{sc.name}.json"), "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
