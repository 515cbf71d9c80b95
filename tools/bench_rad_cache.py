#!/usr/bin/env python
"""Radiosity scenarios from one trace (not the BASELINE metric).

A RadCache of the scene is traced once; K emitter palettes are then solved with 7 rounds each.
  arm A: K one-set solve calls (every set gathers on its own: ids and texel lines fetched K times)
  arm B: one K-set solve call (the sets of a pass interleaved per texel: one id read and one line serve them all)
One process, two warm-up rounds, then --rounds rounds with the arms alternating; HIP events on the calls' stream
around each arm, median (min-max) in ms per K. The two arms' texels are compared for equality.
For context, once per scene: create's rand_ms + rays_ms against fmgi_radiosity's (the same work), the time of a
whole fmgi_radiosity call (host clock) that a scenario cost before, and the bytes model of a round's gather:
the ids once per pass (4 B x 10000 x jobs) and, per ray and job, one line of kp x 16 B instead of K lines of 16 B.

  python tools/bench_rad_cache.py [--cases example box200] [--sets 1 4 8] [--rounds 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402

ITERATIONS = 7


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["example", "box200"])
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch

    import fmgi
    from bench_rad import load_scene
    from fmgi import scene

    libc = ctypes.CDLL(None)
    libc.srand.argtypes = [ctypes.c_uint]
    warm = fmgi.RadCache(scene.box_scene(8, tile_size=1.0))  # the first calls load the kernels
    warm.solve(np.ones((8, 1, 3), np.float32), 1)
    torch.cuda.synchronize()
    warm.close()
    for name in a.cases:
        sc = load_scene(name)
        libc.srand(1)
        fmgi.radiosity(sc)  # warm-up at this size
        libc.srand(1)
        t0 = time.perf_counter()
        whole = fmgi.radiosity(sc)
        call_ms = (time.perf_counter() - t0) * 1e3
        st = fmgi.radiosity_stats()
        libc.srand(1)
        t0 = time.perf_counter()
        rc = fmgi.RadCache(sc)
        create_ms = (time.perf_counter() - t0) * 1e3
        info = rc.info
        jobs, ntex = info["jobs"], info["texels"]
        res = {"case": name, "walls": int(len(sc.walls)), "info": info, "create_call_ms": create_ms,
               "create_trace_ms": info["rand_ms"] + info["rays_ms"],
               "radiosity": {"call_ms": call_ms, "trace_ms": st["rand_ms"] + st["rays_ms"], "bounce_ms": st["bounce_ms"],
                             "total_ms": st["total_ms"]}}
        ref = fmgi.rad_reference_emit(sc)
        rng = np.random.default_rng(5)
        emit = np.stack([ref] + [(ref * rng.uniform(0.05, 2.0, ref.shape)).astype(np.float32)
                                 for _ in range(max(a.sets) - 1)])
        s = torch.cuda.Stream()
        first = rc.solve(emit[:1], ITERATIONS, stream=s)
        s.synchronize()
        res["reference_palette_equals_radiosity"] = bool(np.array_equal(first[0].cpu().numpy().view(np.uint32),
                                                                        whole.view(np.uint32)))

        def arm_a(K):
            return [rc.solve(emit[k:k + 1], ITERATIONS, stream=s) for k in range(K)]

        def arm_b(K):
            return [rc.solve(emit[:K], ITERATIONS, stream=s)]

        for K in a.sets:
            kp = 1 << (K - 1).bit_length()
            ta, tb, host_a, host_b = [], [], [], []
            for r in range(2 + a.rounds):
                order = (arm_a, arm_b) if r % 2 == 0 else (arm_b, arm_a)
                for arm in order:
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    s.synchronize()
                    h0 = time.perf_counter()
                    ev[0].record(s)
                    out = arm(K)
                    ev[1].record(s)
                    host = (time.perf_counter() - h0) * 1e3  # the calls' host time: they do not wait for the device
                    s.synchronize()
                    del out
                    if r < 2:
                        continue
                    (ta if arm is arm_a else tb).append(ev[0].elapsed_time(ev[1]))
                    (host_a if arm is arm_a else host_b).append(host)
            parts, many = arm_a(K), arm_b(K)[0]
            s.synchronize()  # the comparison runs on torch's current stream, not on s
            one = torch.cat(parts)
            A, B = spread(ta), spread(tb)
            ranges = (A["max"] - A["min"]) + (B["max"] - B["min"])
            res[f"K{K}"] = {
                "A_ms": A, "B_ms": B, "A_over_B": A["median"] / B["median"],
                "B_beats_A_by_more_than_the_ranges": A["median"] - B["median"] > ranges,
                "A_host_ms": spread(host_a), "B_host_ms": spread(host_b), "texels_equal": bool(torch.equal(one, many)),
                "B_ms_per_round_and_set": B["median"] / ITERATIONS / K,
                "whole_radiosity_calls_ms": K * call_ms,
                "gather_model_bytes_per_round": {
                    "A": {"ids": 4 * 10000 * jobs * K, "texel_lines": 10000 * jobs * K, "line_bytes_used": 16},
                    "B": {"ids": 4 * 10000 * jobs, "texel_lines": 10000 * jobs * max(1, kp * 16 // 128),
                          "line_bytes_used": kp * 16}},
                "table_bytes": ntex * kp * 16}
        print(json.dumps(res), flush=True)
        rc.close()


if __name__ == "__main__":
    main()
