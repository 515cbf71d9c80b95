#!/usr/bin/env python
"""Traced views against the host path (not the BASELINE metric).

K scenario lightmaps (float32 texels) lie on the device, as a relight session leaves them, and each wants a picture.
  arm A, the host path, per scenario: download the texels, fmgi.output_tiles, fmgi.shade_views
  arm B, the traced view: ViewCache.tiles and ViewCache.shade for all K at once, pictures left on the device
One process, two warm-up rounds, then --rounds rounds with the arms alternating; host times around a synchronise,
median (min-max) per scenario. Once per case: the cost of ViewCache (cand_ms, trace_ms) against arm A's rays_ms, the
records' bytes, and k_view_resolve's own time (device events) with the bytes of DESIGN §16's model over it. The two
arms' pictures are compared for equality at the size timed. The texels are seeded random values: what a ray hits
does not depend on them. The cameras are bench_view.py's, the pixel size scaled to the image width. Arm A's pictures
(host arrays a device copy went through) are kept until a K's rounds are over; --free-pictures frees them between
the arms, as a caller that drops each picture would.

  python tools/bench_view_cache.py [--width 1024 --height 768 --samples 4 --filter bilinear] [--rounds 7] [--free-pictures]

With --projection ortho | equirect the tool instead compares that camera's traced view with the pin-hole's
of the same process: ViewCache's trace time per ray (k_view_trace_proj against k_view_trace), and tiles + shade per
scenario for 8 scenarios (device events; the same kernels read the same records). Two warm-up rounds, then --rounds
rounds with the arms alternating. The cameras are bench_view.py --projection's.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402

SPA = 65_000
BG = (7, 8, 9)
HBM_PEAK = 8.0e12  # bytes/s


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def projection_main(a):
    import torch

    import fmgi
    from bench_view import CASES, load_scene, plan_camera

    W, H, S, K = a.width, a.height, a.samples, 8
    dev = "cuda:0"
    for name in a.cases:
        sname, _, cam, pixel = CASES[name]
        sc = load_scene(sname)
        pin = fmgi.camera(pixel=pixel * 4096 / W, **cam)
        if a.projection == "ortho":
            kw, metres = plan_camera(sc, W, H)
            new = fmgi.camera(pixel=metres, **kw)
        else:
            new = fmgi.camera(pixel=1.0, **cam)
        arms = {"pinhole": pin, a.projection: new}
        rng = np.random.default_rng(11)
        texels = [torch.from_numpy((10.0 ** rng.uniform(-3, 1, (sc.num_texels, 4))).astype(np.float32)).to(dev)
                  for _ in range(K)]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        rows = {k: {"trace_ms": [], "ns_per_ray": [], "ns_per_test": [], "tiles_shade_ms": []} for k in arms}
        tiles = rgb = None
        for r in range(2 + a.rounds):
            order = list(arms) if r % 2 == 0 else list(arms)[::-1]
            for k in order:
                vc = fmgi.ViewCache(sc, arms[k], W, H, S, a.filter, projection=k)
                info = vc.info()
                if tiles is None:
                    tiles = [torch.empty(max(3 * info["tiles"], 1), dtype=torch.uint8, device=dev) for _ in texels]
                    rgb = [torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev) for _ in texels]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                torch.cuda.synchronize()
                ev[0].record()
                vc.tiles(ptr(texels), SPA, ptr(tiles))
                vc.shade(ptr(tiles), ptr(rgb), BG)
                ev[1].record()
                torch.cuda.synchronize()
                vc.close()
                if r < 2:
                    continue
                row = rows[k]
                row["trace_ms"].append(info["trace_ms"])
                row["ns_per_ray"].append(info["trace_ms"] * 1e6 / info["rays"])
                row["ns_per_test"].append(info["trace_ms"] * 1e6 / max(info["tests"], 1))
                row["tiles_shade_ms"].append(ev[0].elapsed_time(ev[1]) / K)
                row.update(rays=info["rays"], tests=info["tests"], hits=info["hits"], bytes=info["bytes"])
        res = {"metric": "traced view: k_view_trace_proj against k_view_trace", "case": name, "walls": int(len(sc.walls)),
               "width": W, "height": H, "samples": S, "filter": a.filter, "projection": a.projection, "scenarios": K,
               "rounds": a.rounds}
        for k, row in rows.items():
            res[k] = {"trace_ms": spread(row["trace_ms"]), "trace_ns_per_ray": spread(row["ns_per_ray"]),
                      "trace_ns_per_test": spread(row["ns_per_test"]),
                      "tiles_shade_ms_per_scenario": spread(row["tiles_shade_ms"]), "rays": row["rays"],
                      "tests_per_ray": row["tests"] / row["rays"], "hit_fraction": row["hits"] / row["rays"],
                      "bytes": row["bytes"]}
        p, q = res["pinhole"]["tiles_shade_ms_per_scenario"], res[a.projection]["tiles_shade_ms_per_scenario"]
        res["tiles_shade_ranges_overlap"] = bool(q["min"] <= p["max"] and p["min"] <= q["max"])
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--projection", choices=("ortho", "equirect"), default=None,
                    help="compare this camera's traced view with the pin-hole's instead")
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--filter", choices=("nearest", "bilinear"), default="bilinear")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="+", default=["example", "box2000"])
    ap.add_argument("--free-pictures", dest="hold", action="store_false",
                    help="free arm A's pictures between the arms instead of keeping them until a K's rounds are over: "
                         "at K = 8 the next device work of either arm then waits 11 to 22 ms (DESIGN §16)")
    a = ap.parse_args()
    if a.projection:
        return projection_main(a)
    import torch

    import fmgi
    from bench_view import CASES, load_scene

    W, H, S = a.width, a.height, a.samples
    dev = "cuda:0"
    for name in a.cases:
        sname, _, cam, pixel = CASES[name]
        sc = load_scene(sname)
        c = fmgi.camera(pixel=pixel * 4096 / W, **cam)
        fmgi.ViewCache(sc, c, W, H, S, a.filter).close()  # warm-up: the first call loads the kernels
        t0 = time.perf_counter()
        vc = fmgi.ViewCache(sc, c, W, H, S, a.filter)
        create_call_ms = (time.perf_counter() - t0) * 1e3
        info = vc.info()
        ntile = info["tiles"]
        res = {"case": name, "walls": int(len(sc.walls)), "width": W, "height": H, "samples": S, "filter": a.filter,
               "create": {k: info[k] for k in ("cand_ms", "trace_ms", "bytes", "rays", "hits", "tests", "tiles")}}
        res["create"]["call_ms"] = create_call_ms
        rng = np.random.default_rng(11)
        texels = [torch.from_numpy((10.0 ** rng.uniform(-3, 1, (sc.num_texels, 4))).astype(np.float32)).to(dev)
                  for _ in range(fmgi.VIEW_CACHE_MAX_SETS)]
        tiles = [torch.empty(max(3 * ntile, 1), dtype=torch.uint8, device=dev) for _ in texels]
        rgb = [torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev) for _ in texels]
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        torch.cuda.synchronize()

        def arm_a(K):
            out, rays_ms = [], 0.0
            for k in range(K):
                _, t = fmgi.output_tiles(sc, texels[k].cpu().numpy(), SPA)
                out.append(fmgi.shade_views(sc, c, W, H, t, BG, samples=S, filter=a.filter)["rgb"])
                rays_ms += fmgi.view_stats()["rays_ms"]
            return out, rays_ms / K

        split = []  # arm B's host time after each of its three steps, per call

        def arm_b(K):
            t = [time.perf_counter()]
            vc.tiles(ptr(texels[:K]), SPA, ptr(tiles[:K]))
            t.append(time.perf_counter())
            vc.shade(ptr(tiles[:K]), ptr(rgb[:K]), BG)
            t.append(time.perf_counter())
            torch.cuda.synchronize()
            t.append(time.perf_counter())
            split.append([(y - x) * 1e3 for x, y in zip(t, t[1:])])

        for K in (1, fmgi.VIEW_CACHE_MAX_SETS):
            ta, tb, rays, held, got = [], [], [], [], None
            del split[:]
            for r in range(2 + a.rounds):
                order = (arm_a, arm_b) if r % 2 == 0 else (arm_b, arm_a)
                for arm in order:
                    if a.hold and got is not None:
                        held.append(got)  # no host buffer a copy went through is freed while the rounds run
                    got = None  # otherwise the other arm's pictures are freed here, outside the timed span
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = arm(K)
                    dt = (time.perf_counter() - t0) * 1e3 / K
                    if r < 2:
                        continue
                    if arm is arm_a:
                        ta.append(dt)
                        rays.append(got[1])
                    else:
                        tb.append(dt)
            b_split = [statistics.median(col) for col in zip(*split[2:])]  # tiles call, shade call, synchronise
            old, _ = arm_a(K)
            arm_b(K)
            equal = all(np.array_equal(rgb[k].cpu().numpy(), old[k]) for k in range(K))
            # k_view_resolve on its own: the tiles made, the pack and the gather between two events
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            tr, tt, host = [], [], []
            for _ in range(a.rounds):
                h0 = time.perf_counter()
                ev[0].record()
                vc.tiles(ptr(texels[:K]), SPA, ptr(tiles[:K]))
                ev[1].record()
                vc.shade(ptr(tiles[:K]), ptr(rgb[:K]), BG)
                ev[2].record()
                host.append((time.perf_counter() - h0) * 1e3)  # the calls' host time: they do not wait for the device
                torch.cuda.synchronize()
                tt.append(ev[0].elapsed_time(ev[1]))
                tr.append(ev[1].elapsed_time(ev[2]))
            spp, pix = S * S, W * H
            rec = 16 if a.filter == "bilinear" else 4
            terms = {"records": pix * spp * rec, "gathered": pix * spp * K * (16 if a.filter == "bilinear" else 4),
                     "output": pix * (3 * K + 1), "pack": ntile * 7 * K}
            model = sum(terms.values())
            A, B = spread(ta), spread(tb)
            res[f"K{K}"] = {
                "A_ms_per_scenario": A, "B_ms_per_scenario": B, "A_over_B": A["median"] / B["median"],
                "gap_exceeds_ranges": A["min"] > B["max"], "B_host_ms_tiles_shade_sync": b_split, "A_rays_ms": spread(rays), "pictures_equal": equal,
                "tiles_ms": spread(tt), "shade_ms": spread(tr), "calls_host_ms": spread(host), "model_bytes": terms,
                "model_share_of_hbm_peak": model / (statistics.median(tr) * 1e-3) / HBM_PEAK}
        a1 = res["K1"]["A_ms_per_scenario"]["median"]
        b8 = res[f"K{fmgi.VIEW_CACHE_MAX_SETS}"]["B_ms_per_scenario"]["median"]
        create = create_call_ms
        res["trace_over_A_rays"] = info["trace_ms"] / res["K1"]["A_rays_ms"]["median"]
        # create + K * B <= K * A
        res["break_even_scenarios"] = create / (a1 - b8) if a1 > b8 else None
        print(json.dumps(res), flush=True)
        vc.close()


if __name__ == "__main__":
    main()
