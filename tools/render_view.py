#!/usr/bin/env python
"""Render a camera view of a (baked) scene on the GPU and write it as a binary PPM.

The scene is a FMGIGEO1 geometry fixture (a path) or a box scene name (box8, box200, box2000). With
--texels (a float32 [numTexels, 4] .npy, e.g. the texels.npy that `bench.py --dump-outputs DIR` writes) the
output step builds the walls' RGB8 tiles (fmgi.output_tiles: --spa as the bake used it, 0 for AO / radiosity
results) and fmgi.render_views colours every pixel with the tile it sees: the picture shows what the
reference's tile PNGs would. Without --texels every wall gets one flat colour from its index, as the
reference's debug raycaster paints.

  python tools/render_view.py box200 --texels out/texels.npy --spa 172413793 --pos 5 4 1.3 --dir 1 0.5 -0.1 \\
      --pixel 0.002 --width 1024 --height 768 -o view.ppm

With --samples N (N x N rays per pixel, up to 8) and / or --filter bilinear the picture comes from
fmgi.shade_views instead: supersampled edges and linearly filtered tiles, as a viewer of the tiles draws them.

--projection ortho draws the plan at true scale (parallel rays along --dir, --pixel metres per pixel), --projection
equirect the 360-degree panorama from --pos (column width / 2 looks along --dir; --pixel is not used, the usual
picture has --width = 2 * --height); both go through fmgi.shade_views:

  python tools/render_view.py flat.bin --texels out/texels.npy --spa 172413793 --projection ortho --pos 6 5 10 \\
      --dir 0 0 -1 --up 0 1 0 --pixel 0.01 --width 1400 --height 1100 --samples 4 --filter bilinear -o plan.ppm

--gloss G (0..1) draws the floor as the bake treats it: a sample that lands on the floor casts one mirror ray and
takes G of its colour from what that ray sees (fmgi.shade_views(gloss=G)); 0 is the matt floor:

  python tools/render_view.py flat.bin --texels out/texels.npy --spa 172413793 --samples 4 --filter bilinear \\
      --gloss 0.75 -o glossy.ppm

A PNG is written next to the PPM when PIL can be imported.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd")]

import numpy as np  # noqa: E402


def load_scene(name, tile_size):
    from fmgi import scene

    if name.startswith("box") and name[3:].isdigit():
        return scene.box_scene(int(name[3:]), **({} if tile_size is None else {"tile_size": tile_size}))
    return scene.load_geometry(name)


def wall_colour_tiles(sc):
    """One flat colour per wall (a fixed hash of its index), as RGB8 tiles in wall order."""
    parts = []
    for i, w in enumerate(sc.walls):
        h = (i * 2654435761 + 0x9E3779B9) & 0xFFFFFFFF
        rgb = np.array([64 + (h & 127), 64 + ((h >> 8) & 127), 64 + ((h >> 16) & 127)], np.uint8)
        parts.append(np.tile(rgb, int(w["lm"][1]) * int(w["lm"][2])))
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def write_ppm(path, rgb):
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())


def gloss_value(text):
    """--gloss: a number in [0, 1]"""
    try:
        g = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number")
    if not 0.0 <= g <= 1.0:
        raise argparse.ArgumentTypeError(f"{text} is outside [0, 1]")
    return g


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", help="geometry fixture path, or box8 / box200 / box2000")
    ap.add_argument("--tile-size", type=float, default=None, help="box scenes: lightmap texels per m^2 (default 200)")
    ap.add_argument("--texels", default=None, help="float32 [numTexels, 4] .npy of the baked texels")
    ap.add_argument("--spa", type=int, default=0, help="numSamplesPerArea of the bake (0: no normalisation)")
    ap.add_argument("--tint-extra", type=int, default=0)
    ap.add_argument("--pos", type=float, nargs=3, default=(5, 5.2, 1.6))
    ap.add_argument("--dir", type=float, nargs=3, default=(1, 1, 0))
    ap.add_argument("--up", type=float, nargs=3, default=(0, 0, 1))
    ap.add_argument("--pixel", type=float, default=0.001)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=3072)
    ap.add_argument("--background", type=int, nargs=3, default=(0, 0, 0))
    ap.add_argument("--samples", type=int, default=1, help="N x N rays per pixel (1..8)")
    ap.add_argument("--filter", choices=("nearest", "bilinear"), default="nearest", help="how a ray reads the tiles")
    ap.add_argument("--projection", choices=("pinhole", "ortho", "equirect"), default="pinhole",
                    help="camera model: pin-hole, orthographic plan, or equirectangular panorama")
    ap.add_argument("--gloss", type=gloss_value, default=0.0,
                    help="the floor's mirror weight in [0, 1]: one mirror bounce from every floor sample (default 0: matt)")
    ap.add_argument("-o", "--output", default="view.ppm")
    a = ap.parse_args(argv)
    import fmgi

    sc = load_scene(a.scene, a.tile_size)
    if a.texels:
        tex = np.load(a.texels).astype(np.float32)
        if tex.shape != (sc.num_texels, 4):
            sys.exit(f"{a.texels}: shape {tex.shape}, the scene has {sc.num_texels} texels of 4 floats")
        _, tiles = fmgi.output_tiles(sc, tex, a.spa, a.tint_extra)
    else:
        tiles = wall_colour_tiles(sc)
    cam = fmgi.camera(a.pos, a.dir, a.up, a.pixel)
    if a.samples == 1 and a.filter == "nearest" and a.projection == "pinhole" and a.gloss == 0:
        out = fmgi.render_views(sc, cam, a.width, a.height, tiles_rgb=tiles, background=tuple(a.background))
        hits, unit = int((out["wall"] >= 0).sum()), "pixels"
    else:
        out = fmgi.shade_views(sc, cam, a.width, a.height, tiles, tuple(a.background), samples=a.samples, filter=a.filter,
                               projection=a.projection, gloss=a.gloss)
        hits, unit = int(out["coverage"].sum(dtype=np.int64)), "rays"
    write_ppm(a.output, out["rgb"][0])
    st = fmgi.view_stats()
    print(f"{a.output}: {a.width}x{a.height}, {hits} of {st['rays']} {unit} hit a wall, "
          f"{st['candidates']} candidates, {st['tests'] / max(st['rays'], 1):.1f} tests/ray, {st['total_ms']:.2f} ms")
    if a.gloss:
        gs = fmgi.view_gloss_stats()
        print(f"  gloss {a.gloss:g}: {gs['mirror_rays']} mirror rays, {gs['mirror_hits']} hit a wall, "
              f"{gs['mirror_tests'] / max(gs['mirror_rays'], 1):.1f} tests/mirror ray")
    try:
        from PIL import Image
    except ImportError:
        return
    Image.fromarray(out["rgb"][0], "RGB").save(os.path.splitext(a.output)[0] + ".png")


if __name__ == "__main__":
    main()
