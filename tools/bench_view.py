#!/usr/bin/env python
"""View renderer measurement (not the BASELINE metric).

Times fmgi_render_views at the reference debug raycaster's image size (4096 x 3072, debugRaytracer.cc:115):
the whole call (host setup, uploads, candidate list, ray casts, download of wall / texel / dist) and its
device phases (fmgi_view_stats, HIP events). Unit of work = one camera ray. Two cases: the example geometry
with the tool's own camera, and box2000 with camera A of tests/golden/make_view_fixtures.py. A small image of
each case is first checked against the reference fixture (tests/golden/view_ref.npz) where one exists.

Then, in the same process and on the same cases, fmgi_shade_views (k_view_shade; random tiles, rgb and coverage
out, 4 bytes per pixel) at (samples, filter) = (1, nearest), (2, bilinear), (4, bilinear): one line each, with
its kernel rate per ray relative to k_view_rays' of the line above. (1, nearest) is checked against
fmgi_render_views' rgb and test count at the full size.

  python tools/bench_view.py [--reps 3] [--width 4096 --height 3072] [--no-shade]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd")]

import numpy as np  # noqa: E402

SHADE = [(1, "nearest"), (2, "bilinear"), (4, "bilinear")]
CASES = {
    # name: (scene, fixture case sharing the camera position and direction, camera, pixel at 4096 x 3072)
    "example": ("example", "example_tool_pixel", dict(pos=(5, 5.2, 1.6), dir=(1, 1, 0), up=(0, 0, 1)), 0.001),
    "box2000": ("box2000", "box2000_A", dict(pos=(5, 4, 1.3), dir=(1, 0.5, -0.1), up=(0, 0, 1)), 0.001),
}


def load_scene(name):
    from fmgi import scene

    if name == "example":
        return scene.load_geometry(os.path.join(REPO, "tests", "golden", "example_geometry.bin"), "example")
    return scene.box_scene(int(name[3:]), tile_size=2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=3072)
    ap.add_argument("--no-shade", action="store_true", help="fmgi_render_views only")
    a = ap.parse_args()
    import fmgi

    z = np.load(os.path.join(REPO, "tests", "golden", "view_ref.npz"))
    meta = json.loads(str(z["meta"]))
    for name, (sname, fx, cam, pixel) in CASES.items():
        sc = load_scene(sname)
        res = {"metric": "view rays/s (whole fmgi_render_views call)", "case": name, "walls": int(len(sc.walls)),
               "width": a.width, "height": a.height, "n_gpus": 1}
        w = z[f"{fx}.camera"]
        small = fmgi.render_views(sc, fmgi.camera(w[0:3], w[3:6], w[6:9], w[9]), meta[fx]["width"], meta[fx]["height"])
        res["equal_to_reference_fixture"] = bool(
            np.array_equal(small["wall"][0], z[f"{fx}.wall"]) and np.array_equal(small["texel"][0], z[f"{fx}.texel"])
            and np.array_equal(small["dist"][0].view(np.uint32), z[f"{fx}.dist_bits"])
            and fmgi.view_stats()["tests"] == int(z[f"{fx}.tests"]))
        c = fmgi.camera(pixel=pixel, **cam)
        fmgi.render_views(sc, c, a.width, a.height)  # warm-up (first allocations of this size)
        ts, st = [], None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fmgi.render_views(sc, c, a.width, a.height)
            ts.append(time.perf_counter() - t0)
            s = fmgi.view_stats()
            if st is None or s["rays_ms"] < st["rays_ms"]:
                st = s
        t = min(ts)
        res.update({"value": st["rays"] / t, "unit": "rays/s", "call_s": t, "stats": st,
                    "device_rays_per_s": st["rays"] / (st["rays_ms"] / 1e3),
                    "device_tests_per_s": st["tests"] / (st["rays_ms"] / 1e3),
                    "tests_per_ray": st["tests"] / st["rays"], "candidates": st["candidates"],
                    "hit_fraction": float((out["wall"] >= 0).mean())})
        print(json.dumps(res), flush=True)
        if a.no_shade:
            continue
        n_tiles = sum(int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls)
        tiles = np.random.default_rng(5).integers(0, 256, 3 * n_tiles, dtype=np.uint8)
        base = res["device_rays_per_s"]
        lit = fmgi.render_views(sc, c, a.width, a.height, tiles_rgb=tiles, background=(7, 8, 9))["rgb"]
        lit_tests = fmgi.view_stats()["tests"]
        for samples, filt in SHADE:
            got = fmgi.shade_views(sc, c, a.width, a.height, tiles, (7, 8, 9), samples=samples, filter=filt)  # warm-up
            sres = {"metric": "view rays/s (whole fmgi_shade_views call)", "case": name, "samples": samples,
                    "filter": filt, "width": a.width, "height": a.height, "n_gpus": 1}
            if (samples, filt) == (1, "nearest"):
                sres["equal_to_render_views"] = bool(np.array_equal(got["rgb"], lit)
                                                     and fmgi.view_stats()["tests"] == lit_tests)
            ts, st = [], None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                got = fmgi.shade_views(sc, c, a.width, a.height, tiles, (7, 8, 9), samples=samples, filter=filt)
                ts.append(time.perf_counter() - t0)
                s = fmgi.view_stats()
                if st is None or s["rays_ms"] < st["rays_ms"]:
                    st = s
            t = min(ts)
            rate = st["rays"] / (st["rays_ms"] / 1e3)
            sres.update({"value": st["rays"] / t, "unit": "rays/s", "call_s": t, "stats": st, "device_rays_per_s": rate,
                         "device_tests_per_s": st["tests"] / (st["rays_ms"] / 1e3),
                         "tests_per_ray": st["tests"] / st["rays"], "per_ray_rate_vs_k_view_rays": rate / base,
                         "covered_fraction": float(got["coverage"].mean(dtype=np.float64)) / samples ** 2})
            print(json.dumps(sres), flush=True)


if __name__ == "__main__":
    main()
