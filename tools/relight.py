#!/usr/bin/env python
"""Bake a scene once, then light it as often as wanted: per-state photon histograms.

The scene (a FMGIGEO1 geometry fixture, or box8 / box200 / box2000 with --tile-size / --with-light) is traced
once into one histogram per group of sources: all windows together, and the lights together or, with
--per-light, one group each. Every scenario of the JSON file then costs one pass over the histograms
(fmgi.Context.recolour) instead of a bake: the lightmap is exactly what a bake with the scenario's colours in
place of photonmap.cl's constants would give. Each result is finalised, normalised and turned into the walls'
RGB8 tiles (fmgi.output_tiles), and written to OUT/<name>/texels.npy (float32 [numTexels, 4], normalised) and
OUT/<name>/tiles.npy (uint8). With --view a camera picture (fmgi.shade_views) goes to OUT/<name>/view.ppm.
--gloss G draws that picture's floor with one mirror bounce.

The scenario file is a JSON list; every entry has a name and a palette per group:

  [{"name": "day"},
   {"name": "evening", "windows": {"window_rgb": [4, 3, 6]}, "lights": {"light_rgb": [20, 16, 9]}},
   {"name": "night",   "windows": {"off": true}, "lights": [{"scale": 0.5}, {"off": true}]}]

A palette may set window_rgb, light_rgb, floor_tint, albedo (defaults: the reference's 18,18,18 / 16,16,18 /
1,0.85,0.7 / 0.9), "scale" (multiplies both emitter colours) or "off" (emitters 0). "lights" is one palette for
every light group, or with --per-light a list with one palette per light. A histogram takes 8 KiB per texel and
group of device memory.

An entry may also carry a sun: "sun": {"azimuth": 200, "elevation": 35, "rgb": [30, 28, 24]} (degrees; +y is north,
fmgi.sun_vector) or "sun": {"to_sun": [x, y, z], "rgb": [..]}. Its direct light through the windows is
added to that scenario's lightmap after the filter and before it is finalised: --sun-samples N x N shadow rays per
texel, one coverage map per distinct direction of the file, the flux the bake's --spa. It needs no photons and is
the same on the dense, --sparse and --load-bake routes.

--sun-bounces N (default 0) adds the sun's bounced light as well: the geometry's radiosity form factors
are traced once (fmgi.RadCache, from the process's libc rand() position), every distinct direction's coverage map is
gathered through them N times, 32 directions to a pass, and each scenario's bounced layer is added right after its
direct sun. --sun-reflectance R G B is the walls' reflectance per channel, one for every wall; its default 0.9 is the
bake's diffuse factor (photonmap.cl:249). The floor's tint and mirror are not modelled. With N = 0 none of this runs and
the files are the bytes they were.

A bake of few photons is speckled; --min-deposits N smooths every scenario's lightmap with the adaptive density
filter before it is finalised: per texel a window of radius <= --max-radius, grown until it
holds the energy of N first-bounce window photons in the reference-palette lightmap of all groups, so all
scenarios share one radius map.

With --sparse every group's histogram is compacted into its sparse, blocked form as soon as it is
traced, through one reused dense scratch histogram, and the scenarios are folded from the sparse blobs
(fmgi.Context.recolour_sparse): one dense histogram plus the blobs of device memory instead of one dense histogram
per group, the same lightmaps bit for bit. --save-bake FILE (implies --sparse) writes the traced scene to one .npz
(fmgi.save_bake); --load-bake FILE lights it again without tracing anything: --spa is then optional (it is taken
from the file and must agree if given) and --per-light follows the file's groups. A file baked for another scene is
refused before any device is touched. --sparse-from-codes (implies --sparse) traces every group with
fmgi.Context.bake_sparse: the bake's deposit codes are counted straight into the blob, so no dense
histogram exists at any time; the blobs, the outputs and a saved bake file are the same bytes. A scene the call
cannot serve (more than 63 tiles of 2048 texels) takes the --sparse route, and the run says so.

  python tools/relight.py tests/golden/example_geometry.bin --spa 6500000 --scenarios scenarios.json -o out
  python tools/relight.py tests/golden/example_geometry.bin --spa 6500000 --per-light --save-bake example.npz --scenarios a.json
  python tools/relight.py tests/golden/example_geometry.bin --load-bake example.npz --scenarios b.json -o out_b
  python tools/relight.py tests/golden/example_geometry.bin --spa 65000 --min-deposits 256 --scenarios scenarios.json
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "flatmatch-global-illumination_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402


def load_scene(name, tile_size, with_light):
    from fmgi import scene

    if name.startswith("box") and name[3:].isdigit():
        kw = {} if tile_size is None else {"tile_size": tile_size}
        return scene.box_scene(int(name[3:]), with_light=with_light, **kw)
    return scene.load_geometry(name)


def palette_of(spec):
    """A fmgi.Palette from a scenario file's palette object."""
    import fmgi

    spec = dict(spec or {})
    off, scale = bool(spec.pop("off", False)), float(spec.pop("scale", 1.0))
    unknown = set(spec) - {"window_rgb", "light_rgb", "floor_tint", "albedo"}
    if unknown:
        raise SystemExit(f"palette keys {sorted(unknown)}: window_rgb, light_rgb, floor_tint, albedo, scale or off")
    p = fmgi.Palette(**spec)
    if off or scale != 1.0:
        k = 0.0 if off else scale
        p = fmgi.Palette(window_rgb=[k * v for v in p.window_rgb], light_rgb=[k * v for v in p.light_rgb],
                         floor_tint=list(p.floor_tint), albedo=p.albedo)
    return p


def source_groups(ranges, per_light):
    """[(label, item_begin, item_end, is_window)]: the windows, then the lights (together, or one group each)."""
    win = [r for r in ranges if r[1]]
    lights = [r for r in ranges if not r[1]]
    groups = []
    if win:
        groups.append(("windows", win[0][2], win[-1][3], True))
    if lights and per_light:
        groups += [(f"light{k}", r[2], r[3], False) for k, r in enumerate(lights)]
    elif lights:
        groups.append(("lights", lights[0][2], lights[-1][3], False))
    return groups


def scenario_palettes(entry, groups):
    """One palette per group for a scenario entry."""
    lights = entry.get("lights")
    n_light = sum(1 for g in groups if not g[3])
    if isinstance(lights, list):
        if len(lights) != n_light:
            raise SystemExit(f"scenario {entry['name']!r}: {len(lights)} light palettes for {n_light} light groups")
        per = list(lights)
    else:
        per = [lights] * n_light
    row, k = [], 0
    for g in groups:
        if g[3]:
            row.append(palette_of(entry.get("windows")))
        else:
            row.append(palette_of(per[k]))
            k += 1
    return row


def sun_of(entry):
    """A scenario entry's sun: None without a "sun" key, else (to_sun float32 [3], rgb [r, g, b]). The object holds
    "rgb" and either "azimuth" and "elevation" in degrees (fmgi.sun_vector: +y is north) or "to_sun": [x, y, z]."""
    import fmgi

    if "sun" not in entry:
        return None
    where = f"scenario {entry.get('name')!r}: sun"
    spec = entry["sun"]
    if not isinstance(spec, dict):
        raise SystemExit(f"{where} must be an object with rgb and azimuth + elevation, or rgb and to_sun")
    unknown = set(spec) - {"azimuth", "elevation", "to_sun", "rgb"}
    if unknown:
        raise SystemExit(f"{where} keys {sorted(unknown)}: azimuth, elevation, to_sun or rgb")

    def numbers(value, n, what):
        ok = (isinstance(value, (list, tuple)) and len(value) == n
              and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in value))
        if not ok or not np.all(np.isfinite(np.asarray(value, np.float64))):
            raise SystemExit(f"{where}: {what} must be {n} finite number{'s' if n > 1 else ''}")
        return [float(v) for v in value]

    if "rgb" not in spec:
        raise SystemExit(f"{where} needs rgb: [r, g, b] in the palette's units (window_rgb is 18)")
    rgb = numbers(spec["rgb"], 3, "rgb")
    if not all(0.0 <= v < 32.0 for v in rgb):
        raise SystemExit(f"{where}: rgb must lie in [0, 32)")
    if "to_sun" in spec:
        if "azimuth" in spec or "elevation" in spec:
            raise SystemExit(f"{where} takes to_sun or azimuth + elevation, not both")
        to_sun = np.array(numbers(spec["to_sun"], 3, "to_sun"), np.float32)
    elif "azimuth" in spec and "elevation" in spec:
        az, = numbers([spec["azimuth"]], 1, "azimuth")
        el, = numbers([spec["elevation"]], 1, "elevation")
        to_sun = fmgi.sun_vector(az, el)
    else:
        raise SystemExit(f"{where} needs azimuth and elevation, or to_sun")
    length = float(np.sqrt(np.sum(to_sun.astype(np.float64) ** 2)))
    if not np.isfinite(length) or not length > 0:
        raise SystemExit(f"{where}: the direction has no length")
    return to_sun, rgb


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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", help="geometry fixture path, or box8 / box200 / box2000")
    ap.add_argument("--tile-size", type=float, default=None, help="box scenes: lightmap texels per m^2 (default 200)")
    ap.add_argument("--with-light", action="store_true", help="box scenes: add the ceiling light")
    ap.add_argument("--spa", type=int, default=None, help="numSamplesPerArea of the bake (optional with --load-bake)")
    ap.add_argument("--scenarios", required=True, help="JSON file: a list of {name, windows, lights}")
    ap.add_argument("--per-light", action="store_true", help="one histogram per light instead of one for all")
    ap.add_argument("--offsets", default=None, help=".npy of int32 launch offsets (default: libc rand(), as the reference)")
    ap.add_argument("--kernel", choices=("auto", "exact", "fast", "grid", "hybrid"), default="auto")
    ap.add_argument("--device", type=int, default=0)
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
    ap.add_argument("--min-deposits", type=int, default=0,
                    help="adaptive density filter: grow every texel's window until it holds the energy of N "
                         "first-bounce window photons (default 0: no filter)")
    ap.add_argument("--max-radius", type=int, default=4, help="the filter's largest window radius in texels (0..16)")
    ap.add_argument("--sun-samples", type=int, default=4,
                    help="scenarios with a sun: N x N shadow rays per texel (1..8, default 4)")
    ap.add_argument("--sun-bounces", type=int, default=0,
                    help="scenarios with a sun: bounces of its light through the radiosity form factors (0..8, default "
                         "0: direct sun only)")
    ap.add_argument("--sun-reflectance", type=float, nargs=3, default=[0.9, 0.9, 0.9], metavar=("R", "G", "B"),
                    help="--sun-bounces: the walls' reflectance per channel in [0, 1] (default 0.9, the bake's diffuse "
                         "factor)")
    ap.add_argument("--sparse", action="store_true",
                    help="compact every group's histogram into its sparse form and recolour from the blobs")
    ap.add_argument("--save-bake", default=None, metavar="FILE", help="write the traced scene to FILE (implies --sparse)")
    ap.add_argument("--load-bake", default=None, metavar="FILE", help="light the bake of FILE: nothing is traced")
    ap.add_argument("--sparse-from-codes", action="store_true",
                    help="trace every group with bake_sparse: the blobs from the deposit codes, no dense scratch "
                         "histogram (implies --sparse)")
    a = ap.parse_args(argv)
    if a.sparse_from_codes and a.load_bake is not None:
        ap.error("--sparse-from-codes with --load-bake: nothing is traced")
    if a.sparse_from_codes:
        a.sparse = True
    if a.load_bake is None and a.spa is None:
        ap.error("the following arguments are required: --spa")
    if a.load_bake is not None and a.save_bake is not None:
        ap.error("--save-bake with --load-bake: the file already exists")
    if a.save_bake is not None or a.load_bake is not None:
        a.sparse = True
    if a.min_deposits < 0:
        ap.error("--min-deposits must not be negative")
    if not 0 <= a.max_radius <= 16:
        ap.error("--max-radius must be in 0..16")
    if not 1 <= a.sun_samples <= 8:
        ap.error("--sun-samples must be in 1..8")
    if not 0 <= a.sun_bounces <= 8:
        ap.error("--sun-bounces must be in 0..8")
    if not all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in a.sun_reflectance):
        ap.error("--sun-reflectance must be three numbers in [0, 1]")
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch

    import fmgi

    with open(a.scenarios) as f:
        entries = json.load(f)
    if not isinstance(entries, list) or not entries or any("name" not in e for e in entries):
        sys.exit(f"{a.scenarios}: a non-empty JSON list of objects with a name")
    names = [str(e["name"]) for e in entries]
    if len(set(names)) != len(names) or any(os.sep in n or n in ("", ".", "..") for n in names):
        sys.exit(f"{a.scenarios}: scenario names must be distinct directory names")
    suns = [sun_of(e) for e in entries]  # a malformed one ends the run here
    sc = load_scene(a.scene, a.tile_size, a.with_light)
    loaded = None
    if a.load_bake is not None:  # every mismatch ends the run here, before a device context exists
        try:
            loaded = fmgi.load_bake(a.load_bake, sc)
        except (ValueError, OSError) as e:
            sys.exit(f"--load-bake: {e}")
        if a.spa is not None and a.spa != loaded["spa"]:
            sys.exit(f"--load-bake: {a.load_bake} was baked with --spa {loaded['spa']}, not {a.spa}")
        a.spa = loaded["spa"]
    dev = f"cuda:{a.device}"
    ctx = fmgi.Context(a.device)
    ctx.set_scene(sc)
    if loaded is None:
        items = ctx.plan(a.spa, rng_offsets=None if a.offsets is None else np.load(a.offsets))
        groups = source_groups(ctx.source_ranges(), a.per_light)
    else:
        items = int(loaded["launches"]["count"].sum())
        groups = [(g["label"], g["item_begin"], g["item_end"], g["is_window"]) for g in loaded["groups"]]
    if not groups:
        sys.exit("the scene has no windows and no lights")
    palettes = [scenario_palettes(e, groups) for e in entries]
    kernel = {"auto": fmgi.KERNEL_AUTO, "exact": fmgi.KERNEL_EXACT, "fast": fmgi.KERNEL_FAST,
              "grid": fmgi.KERNEL_GRID, "hybrid": fmgi.KERNEL_HYBRID}[a.kernel]
    T = sc.num_texels
    from_codes = []  # --sparse-from-codes: per group (dense_chunks, scratch_bytes)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        if loaded is not None:
            infos = [g["info"] for g in loaded["groups"]]
            blobs = [torch.from_numpy(g["blob"].view(np.int64)).to(dev) for g in loaded["groups"]]
        elif a.sparse_from_codes and ctx.bake_sparse_supported():
            infos, blobs = [], []
            for _, b, e, _ in groups:
                info = ctx.bake_sparse(b, e, kernel, s.cuda_stream)
                blob = torch.empty(fmgi.sparse_bytes(T, info.rows) // 8, dtype=torch.int64, device=dev)
                ctx.bake_sparse_take(info, blob.data_ptr(), s.cuda_stream)
                infos.append(info)
                blobs.append(blob)
                st = ctx.bake_sparse_stats()
                from_codes.append((st["dense_chunks"], st["scratch_bytes"]))
        elif a.sparse:
            if a.sparse_from_codes:
                print(f"{sc.name}: --sparse-from-codes cannot serve {T} texels (more than 63 tiles of 2048): "
                      "the --sparse route through one dense scratch histogram instead")
            # one dense scratch histogram for every group in turn: bake, measure, compact, zero
            scratch = torch.zeros((fmgi.COLOUR_STATE_COUNT, T), dtype=torch.int64, device=dev)
            infos, blobs = [], []
            for _, b, e, _ in groups:
                ctx.bake_states(b, e, scratch.data_ptr(), kernel, s.cuda_stream)
                info = ctx.sparse_measure(scratch.data_ptr(), s.cuda_stream)
                blob = torch.empty(fmgi.sparse_bytes(T, info.rows) // 8, dtype=torch.int64, device=dev)
                ctx.sparse_compact(scratch.data_ptr(), info, blob.data_ptr(), s.cuda_stream)
                scratch.zero_()
                infos.append(info)
                blobs.append(blob)
            del scratch
        else:
            hists = [torch.zeros((fmgi.COLOUR_STATE_COUNT, T), dtype=torch.int64, device=dev) for _ in groups]
            for h, (_, b, e, _) in zip(hists, groups):
                ctx.bake_states(b, e, h.data_ptr(), kernel, s.cuda_stream)

        def recolour(pals, lm_ptrs):
            if a.sparse:
                ctx.recolour_sparse([b.data_ptr() for b in blobs], infos, pals, lm_ptrs, s.cuda_stream)
            else:
                ctx.recolour([h.data_ptr() for h in hists], pals, lm_ptrs, s.cuda_stream)

        lms = [torch.zeros((T, 4), dtype=torch.int64, device=dev) for _ in entries]
        recolour(palettes, [lm.data_ptr() for lm in lms])
        if a.min_deposits > 0:
            # one radius map for every scenario, from the photon density: the reference-palette lightmap of all groups
            guide = torch.zeros((T, 4), dtype=torch.int64, device=dev)
            recolour([[fmgi.Palette()] * len(groups)], [guide.data_ptr()])
            radii = torch.zeros(T, dtype=torch.uint8, device=dev)
            ctx.filter_radii(guide.data_ptr(), fmgi.filter_energy(a.min_deposits), a.max_radius, radii.data_ptr(),
                             s.cuda_stream)
            ptrs = [lm.data_ptr() for lm in lms]
            ctx.filter_apply(radii.data_ptr(), ptrs, ptrs, s.cuda_stream)
        # direct sun, after the filter: it is not noise and must not be smoothed. One coverage map per
        # distinct direction of the file; every scenario of that direction adds its colour through it
        by_dir = {}
        for k, sun in enumerate(suns):
            if sun is not None:
                by_dir.setdefault(sun[0].tobytes(), []).append(k)
        covers = []
        for ks in by_dir.values():
            to_sun = suns[ks[0]][0]
            cover = torch.empty(max(T, 1), dtype=torch.uint8, device=dev)
            ctx.sun_coverage(to_sun, a.sun_samples, cover.data_ptr(), stream=s.cuda_stream)
            covers.append(cover)
        bounced = None
        if a.sun_bounces > 0 and by_dir:
            # the sun's bounced light: the form factors once, every direction's tables in one call
            if int(os.environ.get("FMGI_DEVICE", 0)) != a.device:
                sys.exit(f"--sun-bounces: the form factors are traced on device FMGI_DEVICE, not on --device {a.device}")
            rad = fmgi.RadCache(sc)
            bounced = rad.sun_bounce(covers, [suns[ks[0]][0] for ks in by_dir.values()], a.sun_samples, a.sun_bounces,
                                     stream=s.cuda_stream)
        for d, (ks, cover) in enumerate(zip(by_dir.values(), covers)):
            to_sun, ptrs = suns[ks[0]][0], [lms[k].data_ptr() for k in ks]
            ctx.sun_add(cover.data_ptr(), to_sun, a.sun_samples, [suns[k][1] for k in ks], a.spa, ptrs, s.cuda_stream)
            if bounced is not None:
                ctx.sun_add_bounced(bounced[d].data_ptr(), a.sun_bounces, [suns[k][1] for k in ks],
                                    [a.sun_reflectance] * len(ks), a.spa, ptrs, s.cuda_stream)
        zero = torch.zeros((T, 4), dtype=torch.float32, device=dev)
        texels = [torch.empty((T, 4), dtype=torch.float32, device=dev) for _ in entries]
        for lm, t in zip(lms, texels):
            ctx.finalize(lm.data_ptr(), zero.data_ptr(), t.data_ptr(), s.cuda_stream)
    s.synchronize()
    if a.save_bake is not None:
        fmgi.save_bake(a.save_bake, sc, a.spa, 256, ctx.get_plan(),
                       [(g[0], g[1], g[2], g[3], b.cpu().numpy().view(np.uint64)) for g, b in zip(groups, blobs)])
    if not a.sparse:
        print(f"{sc.name}: {100 * items} photons, {T} texels, {len(groups)} histograms of "
              f"{fmgi.states_bytes(T) / 2**20:.1f} MiB ({', '.join(g[0] for g in groups)}), {len(entries)} scenarios")
    else:
        sizes = [fmgi.sparse_bytes(T, i.rows) for i in infos]
        cells, slots = sum(i.cells for i in infos), 64 * sum(i.rows for i in infos)
        traced = (f"loaded from {a.load_bake}, 0 items traced" if loaded is not None else f"{items} items traced")
        print(f"{sc.name}: {100 * items} photons ({traced}), {T} texels, {len(groups)} sparse histograms of "
              f"{', '.join(f'{g[0]} {n / 2**20:.2f} MiB' for g, n in zip(groups, sizes))} "
              f"({100.0 * sum(sizes) / (len(groups) * fmgi.states_bytes(T)):.1f} % of dense, fill "
              f"{cells / max(slots, 1):.2f}), {len(entries)} scenarios")
        if from_codes:
            print(f"  from the deposit codes: peak scratch {max(v[1] for v in from_codes) / 2**20:.2f} MiB (a dense "
                  f"histogram: {fmgi.states_bytes(T) / 2**20:.1f} MiB), {sum(v[0] for v in from_codes)} dense chunks")
        if a.save_bake is not None:
            print(f"  bake saved to {a.save_bake}: {os.path.getsize(a.save_bake)} bytes")
    if by_dir:
        print(f"  sun: {len(by_dir)} direction{'s' if len(by_dir) > 1 else ''}, {a.sun_samples} x {a.sun_samples} "
              f"rays per texel, {sum(len(ks) for ks in by_dir.values())} scenarios")
    if bounced is not None:
        info = rad.info
        print(f"  sun bounces: {a.sun_bounces} through {info['jobs']} jobs' form factors ({info['rays']} rays traced in "
              f"{info['rand_ms'] + info['rays_ms']:.1f} ms), reflectance {' '.join(f'{v:g}' for v in a.sun_reflectance)}")
        rad.close()
    if a.min_deposits > 0:
        print(f"  filtered: {a.min_deposits} deposits, radius <= {a.max_radius}, mean radius "
              f"{radii.float().mean().item():.3f}")
    views = []
    if a.view:
        # the camera's rays are cast once; every scenario's picture is gathered from its device texels
        vdev = f"cuda:{int(os.environ.get('FMGI_DEVICE', 0))}"  # the device of the geometry-based calls
        vc = fmgi.ViewCache(sc, fmgi.camera(a.pos, a.dir, a.up, a.pixel), a.width, a.height, a.samples, a.filter,
                            projection=a.projection, mirror=a.gloss > 0)
        nbytes = max(3 * vc.info()["tiles"], 1)
        vs = torch.cuda.Stream(device=vdev)
        with torch.cuda.stream(vs):
            for k0 in range(0, len(texels), fmgi.VIEW_CACHE_MAX_SETS):
                part = [t.to(vdev) for t in texels[k0:k0 + fmgi.VIEW_CACHE_MAX_SETS]]
                tiles_dev = [torch.empty(nbytes, dtype=torch.uint8, device=vdev) for _ in part]
                rgb_dev = [torch.empty((a.height, a.width, 3), dtype=torch.uint8, device=vdev) for _ in part]
                vc.tiles([t.data_ptr() for t in part], a.spa, [t.data_ptr() for t in tiles_dev], stream=vs.cuda_stream)
                vc.shade([t.data_ptr() for t in tiles_dev], [t.data_ptr() for t in rgb_dev], tuple(a.background),
                         stream=vs.cuda_stream, gloss=a.gloss)
                views += rgb_dev
        vs.synchronize()
        views = [v.cpu().numpy() for v in views]
        vc.close()
    for k, (name, t) in enumerate(zip(names, texels)):
        d = os.path.join(a.output, name)
        os.makedirs(d, exist_ok=True)
        tex, tiles = fmgi.output_tiles(sc, t.cpu().numpy(), a.spa)
        np.save(os.path.join(d, "texels.npy"), tex)
        np.save(os.path.join(d, "tiles.npy"), tiles)
        if a.view:
            from render_view import write_ppm

            write_ppm(os.path.join(d, "view.ppm"), views[k])
        print(f"  {d}: mean texel {tex[:, :3].mean():.6g}")
    ctx.close()


if __name__ == "__main__":
    main()
