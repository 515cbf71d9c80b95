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

With --projection ortho | equirect the tool instead times that camera's k_view_shade_proj against the
pin-hole k_view_shade of the same process at the same ray count (--samples x --samples, --filter): two warm-up
rounds, then --rounds rounds with the arms alternating, medians with ranges of the kernel time (fmgi_view_stats'
rays_ms), rays/s, candidates per list, tests per ray and the time per intersects() evaluation. ortho looks down
on the whole scene, equirect stands at the case's camera position.

  python tools/bench_view.py --projection equirect --width 2048 --height 1024
  python tools/bench_view.py --projection ortho --width 2048 --height 1536

With --gloss G the tool times the glossy floor: k_view_shade_gloss at gloss G against k_view_shade (gloss
0) of the same process, arms alternating, best of --rounds after two warm-up rounds, on the two cases and on a
camera that looks straight down at box200's floor so that every sample mirrors. It prints the mirror rays, the
mirror tests and tests per mirror ray, the time the second walk adds per mirror test against k_view_shade's time
per test on box2000, and for a traced view the trace with and without mirror records and shade per picture
with and without gloss.

  python tools/bench_view.py --gloss 0.75 --width 1024 --height 768 --rounds 5
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd")]

import statistics  # noqa: E402

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


def plan_camera(sc, width, height, margin=1.02):
    """the orthographic camera above the scene that looks down on all of it: (camera keywords, metres per pixel)"""
    W = sc.walls
    pts = np.concatenate([W["pos"], W["pos"] + W["width"], W["pos"] + W["height"],
                          W["pos"] + W["width"] + W["height"]])[:, :3].astype(np.float64)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pixel = margin * max((hi[0] - lo[0]) / width, (hi[1] - lo[1]) / height)
    pos = (float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), float(hi[2] + 1.0))
    return dict(pos=pos, dir=(0, 0, -1), up=(0, 1, 0)), float(pixel)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def projection_main(a):
    """k_view_shade_proj<projection> against the pin-hole k_view_shade, arms alternating in one process"""
    import fmgi

    W, H, S = a.width, a.height, a.samples
    for name, (sname, _, cam, pixel) in CASES.items():
        sc = load_scene(sname)
        n_tiles = sum(int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls)
        tiles = np.random.default_rng(5).integers(0, 256, 3 * n_tiles, dtype=np.uint8)
        pin = fmgi.camera(pixel=pixel * 4096 / W, **cam)
        if a.projection == "ortho":
            kw, metres = plan_camera(sc, W, H)
            new = fmgi.camera(pixel=metres, **kw)
        else:
            new = fmgi.camera(pixel=1.0, **cam)
        arms = {"pinhole": (pin, "pinhole"), a.projection: (new, a.projection)}
        rows = {k: {"rays_ms": [], "ns_per_test": []} for k in arms}
        for r in range(2 + a.rounds):
            order = list(arms) if r % 2 == 0 else list(arms)[::-1]
            for k in order:
                c, proj = arms[k]
                got = fmgi.shade_views(sc, c, W, H, tiles, (7, 8, 9), samples=S, filter=a.filter, projection=proj)
                st = fmgi.view_stats()
                if r < 2:
                    continue
                rows[k]["rays_ms"].append(st["rays_ms"])
                rows[k]["ns_per_test"].append(st["rays_ms"] * 1e6 / max(st["tests"], 1))
                rows[k].update(rays=st["rays"], tests=st["tests"], candidates=st["candidates"], cand_ms=st["cand_ms"],
                               covered_fraction=float(got["coverage"].mean(dtype=np.float64)) / S ** 2)
        res = {"metric": "k_view_shade_proj against k_view_shade", "case": name, "walls": int(len(sc.walls)), "width": W,
               "height": H, "samples": S, "filter": a.filter, "projection": a.projection, "rounds": a.rounds, "n_gpus": 1}
        for k, row in rows.items():
            ms = spread(row["rays_ms"])
            res[k] = {"kernel_ms": ms, "rays_per_s": row["rays"] / (ms["median"] / 1e3), "candidates": row["candidates"],
                      "tests_per_ray": row["tests"] / row["rays"], "ns_per_test": spread(row["ns_per_test"]),
                      "cand_ms": row["cand_ms"], "covered_fraction": row["covered_fraction"]}
        p, q = res["pinhole"]["ns_per_test"], res[a.projection]["ns_per_test"]
        res["ns_per_test_ratio"] = q["median"] / p["median"]
        res["within_the_yardsticks_range"] = bool(q["median"] <= p["max"])
        print(json.dumps(res), flush=True)


# box200 from 2.5 m above its 10 m x 8 m floor, looking straight down: the screen plane is 1 m away, so a span of
# 2.048 m covers 5.12 m x 3.84 m of floor at 4 : 3; the image stays on the floor and every sample mirrors
FLOOR_CASE = ("box200", dict(pos=(5, 4, 2.5), dir=(0, 0, -1), up=(0, 1, 0)), 0.002 * 1024)


def gloss_main(a):
    """k_view_shade_gloss against k_view_shade, arms alternating in one process; then the traced view"""
    import torch

    import fmgi

    W, H, S, G = a.width, a.height, a.samples, a.gloss
    cases = {name: (sname, cam, pixel * 4096) for name, (sname, _, cam, pixel) in CASES.items()}
    cases["box200_floor"] = FLOOR_CASE
    per_test = {}
    for name, (sname, cam, span) in cases.items():
        sc = load_scene(sname)
        n_tiles = sum(int(w["lm"][1]) * int(w["lm"][2]) for w in sc.walls)
        tiles = np.random.default_rng(5).integers(0, 256, 3 * n_tiles, dtype=np.uint8)
        c = fmgi.camera(pixel=span / W, **cam)
        rows = {0.0: [], G: []}
        stats = {}
        for r in range(2 + a.rounds):
            for g in ((0.0, G) if r % 2 == 0 else (G, 0.0)):
                fmgi.shade_views(sc, c, W, H, tiles, (7, 8, 9), samples=S, filter=a.filter, gloss=g)
                st = fmgi.view_stats()
                stats[g] = (st, fmgi.view_gloss_stats())
                if r >= 2:
                    rows[g].append(st["rays_ms"])
        (st0, _), (st1, gs) = stats[0.0], stats[G]
        t0, t1 = min(rows[0.0]), min(rows[G])
        per_test[name] = t0 * 1e6 / max(st0["tests"], 1)
        res = {"metric": "k_view_shade_gloss against k_view_shade", "case": name, "walls": int(len(sc.walls)), "width": W,
               "height": H, "samples": S, "filter": a.filter, "gloss": G, "rounds": a.rounds, "n_gpus": 1,
               "kernel_ms": {"gloss_0": spread(rows[0.0]), "gloss": spread(rows[G])}, "rays": st1["rays"],
               "primary_tests": st0["tests"], "mirror_rays": gs["mirror_rays"], "mirror_hits": gs["mirror_hits"],
               "mirror_tests": gs["mirror_tests"], "tests_per_ray": st0["tests"] / st0["rays"],
               "tests_per_mirror_ray": gs["mirror_tests"] / max(gs["mirror_rays"], 1),
               "mirror_share": gs["mirror_rays"] / st1["rays"], "all_samples_mirror": gs["mirror_rays"] == st1["rays"],
               "ns_per_test_gloss_0": per_test[name], "time_ratio": t1 / t0,
               "ns_per_mirror_test": (t1 - t0) * 1e6 / max(gs["mirror_tests"], 1)}
        if name == "box200_floor":
            res["yardstick_ns_per_test_box2000"] = per_test["box2000"]
            res["ratio_to_yardstick"] = res["ns_per_mirror_test"] / per_test["box2000"]
            res["within_1.10"] = bool(res["ratio_to_yardstick"] <= 1.10)
        # the traced view: the trace with and without mirror records, shade per picture with and without gloss
        dev = f"cuda:{int(os.environ.get('FMGI_DEVICE', 0))}"
        tiles_dev = torch.from_numpy(tiles).to(dev)
        rgb_dev = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        trace = {}
        for mirror in (False, True):
            ms = []
            for _ in range(3):
                vc = fmgi.ViewCache(sc, c, W, H, S, a.filter, mirror=mirror)
                ms.append(vc.info()["trace_ms"])
                if len(ms) < 3:
                    vc.close()
            trace["mirror" if mirror else "plain"] = min(ms)
            if not mirror:
                vc.close()
        shade = {}
        for g in (0.0, G):
            ms = []
            for r in range(2 + a.rounds):
                ev[0].record()
                vc.shade([tiles_dev.data_ptr()], [rgb_dev.data_ptr()], (7, 8, 9), gloss=g)
                ev[1].record()
                ev[1].synchronize()
                if r >= 2:
                    ms.append(ev[0].elapsed_time(ev[1]))
            shade["gloss_0" if g == 0 else "gloss"] = min(ms)
        host = fmgi.shade_views(sc, c, W, H, tiles, (7, 8, 9), samples=S, filter=a.filter, gloss=G)["rgb"][0]
        res["traced_view"] = {"trace_ms": trace, "bytes": vc.info()["bytes"], "shade_ms": shade,
                              "equal_to_shade_views": bool(np.array_equal(rgb_dev.cpu().numpy(), host))}
        vc.close()
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--projection", choices=("ortho", "equirect"), default=None,
                    help="time this camera's k_view_shade_proj against the pin-hole k_view_shade instead")
    ap.add_argument("--gloss", type=float, default=None,
                    help="time the glossy floor at this mirror weight (0 < G <= 1) against the matt floor instead")
    ap.add_argument("--samples", type=int, default=4, help="--projection: N x N rays per pixel")
    ap.add_argument("--filter", choices=("nearest", "bilinear"), default="bilinear", help="--projection: the tile filter")
    ap.add_argument("--rounds", type=int, default=7, help="--projection: timed rounds after two warm-up rounds")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=3072)
    ap.add_argument("--no-shade", action="store_true", help="fmgi_render_views only")
    a = ap.parse_args()
    if a.gloss is not None:
        if a.projection or not 0 < a.gloss <= 1:
            ap.error("--gloss takes a weight in (0, 1] and the pin-hole camera")
        return gloss_main(a)
    if a.projection:
        return projection_main(a)
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
