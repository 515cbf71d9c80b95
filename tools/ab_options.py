#!/usr/bin/env python
"""A/B of per-context option sets (fmgi_set_option) in one process. The arms alternate (A B A B ...) for
`--reps` rounds after one warm-up bake each, so clock and temperature drift hits every arm alike. Prints one
JSON line per arm with the k_bake and fold times per step (HIP events, fmgi_set_timing) as median and
min-max, the k_bake instance the arm ran and its bucket_fallback_codes. The first arm's int64 lightmap is the
reference and every other arm must equal it bit for bit. Exits non-zero if bucket_fill had no effect, i.e. an
arm with bucket_fill=1 and one with bucket_fill=2 ran the same k_bake instance.

  python tools/ab_options.py --config box200 --reps 5
  python tools/ab_options.py --config example --arm bucket_fill=1 --arm bucket_fill=2

Default arms: bucket_fill=1 and bucket_fill=2, each with wide_tiles=0 and wide_tiles=1.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), REPO]

import numpy as np  # noqa: E402

DEFAULT_ARMS = ["bucket_fill=1 wide_tiles=0", "bucket_fill=2 wide_tiles=0",
                "bucket_fill=1 wide_tiles=1", "bucket_fill=2 wide_tiles=1"]


def parse_arm(text):
    return {k: int(v) for k, v in (kv.split("=", 1) for kv in text.split())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="box200")
    ap.add_argument("--arm", action="append", default=[], help="space-separated option=value pairs of one arm")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=0,
                    help="profiling runs: after the warm-ups, this many timed steps per arm and no lightmap copies")
    args = ap.parse_args()
    import torch

    import bench
    import fmgi
    from fmgi._lib import OPTIONS

    arms = [parse_arm(a) for a in (args.arm or DEFAULT_ARMS)]
    names = [" ".join(f"{k}={v}" for k, v in a.items()) for a in arms]
    touched = sorted({k for a in arms for k in a})
    for k in touched:
        if k not in OPTIONS:
            raise SystemExit(f"unknown option {k!r} (one of {sorted(OPTIONS)})")
    cfg = bench.CONFIGS[args.config]
    sc = bench.load_scene(cfg["scene"])
    ctx = fmgi.Context(0)
    ctx.set_scene(sc)
    ctypes.CDLL(None).srand(1)
    items = ctx.plan(cfg["spa"])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    lm = torch.zeros((sc.num_texels, 4), dtype=torch.int64, device=dev)
    ctx.set_timing(True)

    def bake(arm):
        for k in touched:  # options an arm does not name are at their default (-1 / 0)
            ctx.set_option(k, arm.get(k, 0 if k in ("chunk_items", "pool_limit", "coop", "no_axes") else -1))
        lm.zero_()
        ctx.timing()
        ctx.reset_stats()
        ctx.bake_items(0, items, lm.data_ptr(), fmgi.KERNEL_AUTO, stream.cuda_stream)
        torch.cuda.synchronize()
        t = ctx.timing()
        return t["bake_ms"], t["fold_ms"]

    ref = None
    same = [True] * len(arms)
    kern = [""] * len(arms)
    fallback = [0] * len(arms)
    deposits = [0] * len(arms)
    bake_ms = [[] for _ in arms]
    fold_ms = [[] for _ in arms]
    for i, arm in enumerate(arms):  # warm-up: first use of the arm's kernels and buffers
        bake(arm)
        kern[i] = ctx.last_bake_kernel
    for _ in range(args.steps or args.reps):
        for i, arm in enumerate(arms):
            b, f = bake(arm)
            bake_ms[i].append(b)
            fold_ms[i].append(f)
            st = ctx.stats()
            fallback[i] = max(fallback[i], st.get("bucket_fallback_codes", 0))
            deposits[i] = st["deposits"]
            if st["stream_overflow"]:
                raise SystemExit(f"arm {names[i]!r}: stream_overflow = {st['stream_overflow']}")
            if args.steps:
                continue
            got = lm.cpu().numpy()
            if ref is None:
                ref = got.copy()
            same[i] = same[i] and bool(np.array_equal(got, ref))

    def summary(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    for i in range(len(arms)):
        tot = [b + f for b, f in zip(bake_ms[i], fold_ms[i])]
        print(json.dumps({"config": args.config, "arm": names[i], "k_bake_ms": summary(bake_ms[i]),
                          "fold_ms": summary(fold_ms[i]), "bake_plus_fold_ms": summary(tot), "kernel": kern[i],
                          "deposits": deposits[i], "bucket_fallback_codes": fallback[i],
                          "bit_identical_to_first": same[i] if not args.steps else None}), flush=True)
    ctx.close()
    if not all(same):
        raise SystemExit("an arm's lightmap differs from the first arm's")
    k1 = {kern[i] for i, a in enumerate(arms) if a.get("bucket_fill") == 1}
    k2 = {kern[i] for i, a in enumerate(arms) if a.get("bucket_fill") == 2}
    if k1 and k2 and (k1 & k2):
        raise SystemExit(f"bucket_fill had no effect: both arms ran {sorted(k1 & k2)}")


if __name__ == "__main__":
    main()
