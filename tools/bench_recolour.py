#!/usr/bin/env python
"""Recolouring measurement (not the BASELINE metric).

For example.png (BASELINE config 2) and box200 (config 3), in one process, device times from events on the
calls' stream, medians after warm-up:

  * the cost of keeping the histogram: fmgi_bake_states against STREAM fmgi_bake_items over the same items;
  * fmgi_recolour of one whole-bake histogram (G = 1) with K = 1 and K = 8 scenarios: ms per call (its table
    upload and its launch), histogram bytes per second, the same buffer's device-to-device copy timed in the
    same rounds, and the fraction of the 8 TB/s HBM peak;
  * K scenarios by recolouring against K STREAM bakes.

The histogram of the timed bakes (every repetition adds to it) is checked: recoloured with the reference
palette it must equal that many times the STREAM bake's lightmap, bit for bit.

  python tools/bench_recolour.py [--configs example box200] [--reps 3] [--recolour-reps 15] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd")]

HBM_PEAK = 8.0e12  # bytes/s, the MI355X data sheet's

CONFIGS = {"example": ("example", 6_500_000), "box200": ("box200", 172_413_793)}


def load_scene(name):
    from fmgi import scene

    if name == "example":
        return scene.load_geometry(os.path.join(REPO, "tests", "golden", "example_geometry.bin"), "example")
    return scene.box_scene(int(name[3:]))


def timed(torch, stream, fn, warmup, reps):
    """device ms of fn() on `stream`, one pair of events per call: the list of the reps"""
    out = []
    for i in range(warmup + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        fn()
        t1.record(stream)
        t1.synchronize()
        if i >= warmup:
            out.append(t0.elapsed_time(t1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["example", "box200"], choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=3, help="timed bakes of each kind")
    ap.add_argument("--recolour-reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="directory for recolour_<config>.json")
    a = ap.parse_args()
    import torch

    import fmgi

    med = statistics.median
    for name in a.configs:
        sname, spa = CONFIGS[name]
        sc = load_scene(sname)
        T = sc.num_texels
        ctx = fmgi.Context(0)
        ctx.set_scene(sc)
        items = ctx.plan(spa)
        s = torch.cuda.Stream(device="cuda:0")
        res = {"metric": "recolour: histogram bytes/s, and ms against a re-bake", "config": name, "texels": T,
               "photons": 100 * items, "histogram_bytes": fmgi.states_bytes(T), "n_gpus": 1}
        with torch.cuda.stream(s):
            hist = torch.zeros((1024, T), dtype=torch.int64, device="cuda:0")
            copy = torch.empty_like(hist)
            lm = torch.zeros((T, 4), dtype=torch.int64, device="cuda:0")
            lms = [torch.zeros((T, 4), dtype=torch.int64, device="cuda:0") for _ in range(8)]
            # STREAM bake (the product's), then the histogram bake, same items
            stream_ms = timed(torch, s, lambda: ctx.bake_items(0, items, lm.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream),
                              1, a.reps)
            res["bake_stream_kernel"] = ctx.last_bake_kernel
            n_state = 1 + a.reps
            state_ms = timed(torch, s, lambda: ctx.bake_states(0, items, hist.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream),
                             1, a.reps)
            res["bake_states_kernel"] = ctx.last_bake_kernel
            # check: the n_state bakes' histogram under the reference palette = n_state x one STREAM bake
            one = torch.zeros((T, 4), dtype=torch.int64, device="cuda:0")
            ctx.bake_items(0, items, one.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            chk = torch.zeros((T, 4), dtype=torch.int64, device="cuda:0")
            ctx.recolour([hist.data_ptr()], [[fmgi.Palette()]], [chk.data_ptr()], s.cuda_stream)
            s.synchronize()
            res["recolour_equals_stream_bake"] = bool(torch.equal(chk, one * n_state))
            nz = hist != 0
            res["histogram_nonzero_cells"] = int(nz.sum().item())
            res["histogram_states_used"] = int(nz.any(dim=1).sum().item())
            res["histogram_max_count"] = int(hist.max().item())
            del nz
            pals = [[fmgi.Palette(window_rgb=(18 - k, 18 - 2 * k, 18), light_rgb=(16, 16 - k, 18 - k),
                                  floor_tint=(1.0, 0.85 - 0.05 * k, 0.7), albedo=0.9 - 0.02 * k)] for k in range(8)]
            r1, r8, cp = [], [], []
            for i in range(2 + a.recolour_reps):  # interleaved rounds: K = 1, K = 8, the copy
                x1 = timed(torch, s, lambda: ctx.recolour([hist.data_ptr()], pals[:1], [lms[0].data_ptr()], s.cuda_stream), 0, 1)
                x8 = timed(torch, s, lambda: ctx.recolour([hist.data_ptr()], pals, [m.data_ptr() for m in lms], s.cuda_stream), 0, 1)
                xc = timed(torch, s, lambda: copy.copy_(hist), 0, 1)
                if i >= 2:
                    r1 += x1
                    r8 += x8
                    cp += xc
        B = res["histogram_bytes"]
        res.update({
            "bake_stream_ms": med(stream_ms), "bake_stream_ms_all": stream_ms,
            "bake_states_ms": med(state_ms), "bake_states_ms_all": state_ms,
            "bake_states_over_stream": med(state_ms) / med(stream_ms),
            "recolour_k1_ms": med(r1), "recolour_k1_ms_min": min(r1),
            "recolour_k8_ms": med(r8), "recolour_k8_ms_min": min(r8),
            "recolour_k1_bytes_per_s": B / (med(r1) / 1e3), "recolour_k8_bytes_per_s": B / (med(r8) / 1e3),
            "recolour_k1_fraction_of_hbm_peak": B / (med(r1) / 1e3) / HBM_PEAK,
            "recolour_k8_fraction_of_hbm_peak": B / (med(r8) / 1e3) / HBM_PEAK,
            "copy_d2d_ms": med(cp), "copy_d2d_read_bytes_per_s": B / (med(cp) / 1e3),
            "recolour_k8_over_eight_k1": med(r8) / (8 * med(r1)),
            "eight_scenarios_recolour_ms": med(r8), "eight_scenarios_rebake_ms": 8 * med(stream_ms),
            "one_scenario_recolour_ms": med(r1), "one_scenario_rebake_ms": med(stream_ms),
        })
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"recolour_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        del hist, copy, lm, lms, one, chk
        ctx.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
