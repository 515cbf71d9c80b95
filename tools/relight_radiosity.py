#!/usr/bin/env python
"""Radiosity under several emitter palettes from one trace (fmgi.RadCache).

The scene's form factors are traced once, from the process's libc rand() position as the reference's radiosity mode
does; every scenario of the file is then solved from them on the device, eight to a pass.

  python tools/relight_radiosity.py SCENE --scenarios FILE [-o out] [--iterations 7] [--view ...]

SCENE is a geometry fixture or box8 / box200 / box2000 (--tile-size, --with-light). FILE is a JSON list of
  {"name": "evening", "windows": [2, 2, 6], "lights": [28, 28, 32]}
where "windows" and "lights" are an RGB triple for every emitter of the kind, or a list with one triple per emitter;
a kind that is left out is switched off. Values are the emitters' starting radiosities (the reference: 30 for
windows, (28, 28, 32) for lights), finite and >= 0.

Writes OUT/<name>/texels.npy (float32 [numTexels, 4]) and tiles.npy (the RGB8 tiles of the reference's radiosity
mode: numSamplesPerArea = 0, tintExtra = 1) and, with --view, view.ppm: one ViewCache casts the camera's rays once
and shades every scenario from the device texels the solve left; --gloss G draws the floor with one mirror bounce.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402

SPA, TINT = 0, 1  # main.c:88-91: the radiosity mode's output step


def load_scene(name, tile_size, with_light):
    from fmgi import scene

    if name.startswith("box") and name[3:].isdigit():
        kw = {} if tile_size is None else {"tile_size": tile_size}
        return scene.box_scene(int(name[3:]), with_light=with_light, **kw)
    return scene.load_geometry(name)


def _triples(spec, count, kind, name):
    """`count` RGB triples from one triple, a list of `count` triples, or nothing (off)."""
    if spec is None:
        return np.zeros((count, 3), np.float32)
    a = np.asarray(spec, np.float64)
    if a.shape == (3,):
        a = np.broadcast_to(a, (count, 3))
    elif a.ndim != 2 or a.shape[1:] != (3,):
        raise SystemExit(f"scenario {name!r}: {kind} is neither an RGB triple nor a list of triples")
    elif len(a) != count:
        raise SystemExit(f"scenario {name!r}: {len(a)} {kind} triples for {count} {kind}")
    if not np.isfinite(a).all() or (a < 0).any():
        raise SystemExit(f"scenario {name!r}: a {kind} value is negative or not finite")
    return a.astype(np.float32)


def scenario_emit(entries, num_windows, num_lights):
    """(names, emit float32 [K, windows + lights, 3]) of a scenario list"""
    if not isinstance(entries, list) or not entries:
        raise SystemExit("the scenario file holds a non-empty JSON list")
    names, emit = [], []
    for e in entries:
        if not isinstance(e, dict) or not isinstance(e.get("name"), str) or not e["name"]:
            raise SystemExit("every scenario is an object with a name")
        name = e["name"]
        unknown = set(e) - {"name", "windows", "lights"}
        if unknown:
            raise SystemExit(f"scenario {name!r}: keys {sorted(unknown)}: name, windows or lights")
        if name in names:
            raise SystemExit(f"scenario name {name!r} appears twice")
        if os.sep in name or name in (".", ".."):
            raise SystemExit(f"scenario name {name!r} cannot name a directory")
        names.append(name)
        emit.append(np.concatenate([_triples(e.get("windows"), num_windows, "windows", name),
                                    _triples(e.get("lights"), num_lights, "lights", name)]))
    return names, np.stack(emit).astype(np.float32).reshape(len(names), num_windows + num_lights, 3)


def gloss_value(text):
    """--gloss: a number in [0, 1]"""
    try:
        g = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number")
    if not 0.0 <= g <= 1.0:
        raise argparse.ArgumentTypeError(f"{text} is outside [0, 1]")
    return g


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("scene", help="geometry fixture path, or box8 / box200 / box2000")
    ap.add_argument("--tile-size", type=float, default=None, help="box scenes: lightmap texels per m^2 (default 200)")
    ap.add_argument("--with-light", action="store_true", help="box scenes: add the ceiling light")
    ap.add_argument("--scenarios", required=True, help="JSON file: a list of {name, windows, lights}")
    ap.add_argument("--iterations", type=int, default=7, help="bounce rounds (the reference: 7)")
    ap.add_argument("-o", "--output", default="out")
    ap.add_argument("--view", action="store_true", help="also write OUT/<name>/view.ppm")
    ap.add_argument("--pos", type=float, nargs=3, default=(5, 5.2, 1.6))
    ap.add_argument("--dir", type=float, nargs=3, default=(1, 1, 0))
    ap.add_argument("--up", type=float, nargs=3, default=(0, 0, 1))
    ap.add_argument("--pixel", type=float, default=0.001)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--background", type=int, nargs=3, default=(0, 0, 0))
    ap.add_argument("--samples", type=int, default=2, help="N x N rays per pixel (1..8)")
    ap.add_argument("--filter", choices=("nearest", "bilinear"), default="bilinear")
    ap.add_argument("--projection", choices=("pinhole", "ortho", "equirect"), default="pinhole",
                    help="--view's camera model: pin-hole, orthographic plan (--pixel metres per pixel), or panorama")
    ap.add_argument("--gloss", type=gloss_value, default=0.0,
                    help="--view: the floor's mirror weight in [0, 1], one mirror bounce from every floor sample "
                         "(default 0: matt)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    sc = load_scene(a.scene, a.tile_size, a.with_light)
    with open(a.scenarios) as f:
        names, emit = scenario_emit(json.load(f), len(sc.windows), len(sc.lights))
    if not 1 <= a.iterations <= 64:
        raise SystemExit("--iterations outside 1..64")
    import torch

    import fmgi

    rc = fmgi.RadCache(sc)
    info = rc.info
    print(f"{sc.name}: {info['jobs']} jobs, {info['rays']} rays traced in {info['rand_ms'] + info['rays_ms']:.1f} ms, "
          f"{info['bytes'] / 2 ** 20:.1f} MiB kept; {len(names)} scenarios")
    dev = f"cuda:{int(os.environ.get('FMGI_DEVICE', 0))}"
    st = torch.cuda.Stream(device=dev)
    views = []
    with torch.cuda.stream(st):
        texels = rc.solve(emit, a.iterations, stream=st)
        if a.view:
            vc = fmgi.ViewCache(sc, fmgi.camera(a.pos, a.dir, a.up, a.pixel), a.width, a.height, a.samples, a.filter,
                                projection=a.projection, mirror=a.gloss > 0)
            nbytes = max(3 * vc.info()["tiles"], 1)
            for k0 in range(0, len(names), fmgi.VIEW_CACHE_MAX_SETS):
                part = [texels[k] for k in range(k0, min(k0 + fmgi.VIEW_CACHE_MAX_SETS, len(names)))]
                tiles_dev = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in part]
                rgb_dev = [torch.empty((a.height, a.width, 3), dtype=torch.uint8, device=dev) for _ in part]
                vc.tiles([t.data_ptr() for t in part], SPA, [t.data_ptr() for t in tiles_dev], TINT, stream=st.cuda_stream)
                vc.shade([t.data_ptr() for t in tiles_dev], [t.data_ptr() for t in rgb_dev], tuple(a.background),
                         stream=st.cuda_stream, gloss=a.gloss)
                views += rgb_dev
    st.synchronize()
    if a.view:
        views = [v.cpu().numpy() for v in views]
        vc.close()
    host = texels.cpu().numpy()
    for k, name in enumerate(names):
        d = os.path.join(a.output, name)
        os.makedirs(d, exist_ok=True)
        _, tiles = fmgi.output_tiles(sc, host[k], SPA, TINT)
        np.save(os.path.join(d, "texels.npy"), host[k])
        np.save(os.path.join(d, "tiles.npy"), tiles)
        if a.view:
            from render_view import write_ppm

            write_ppm(os.path.join(d, "view.ppm"), views[k])
        print(f"  {d}: mean texel {host[k][:, :3].mean():.6g}")
    rc.close()


if __name__ == "__main__":
    main()
