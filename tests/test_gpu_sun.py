"""GPU tests of the direct-sun layer (fmgi_sun_coverage / fmgi_sun_add). Every comparison is equality:
the coverage bytes and the four order-independent counts against the float32 restatement (sun_restate.py) in both
modes, the occluder lists against the all-walls mode on seeded directions, the deposits against the integer
restatement, two streams against one, the empty scenes, and tools/relight.py against the API route."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import recolour_events as E
import sun_restate as R
from conftest import GOLDEN, REPO
from fmgi import scene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COUNTS = ("samples", "facing", "crossing", "lit")


@pytest.fixture(scope="module")
def ctxs(torch_cuda):
    """one context per scene, shared by the module's tests"""
    made = {}

    def get(sc):
        if id(sc) not in made:
            ctx = fmgi.Context(0)
            ctx.set_scene(sc)
            made[id(sc)] = (ctx, sc)
        return made[id(sc)][0]

    yield get
    for ctx, _ in made.values():
        ctx.close()


def _cover(torch, ctx, sc, to_sun, S, mode, fill=0xFF):
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        cover = torch.full((max(sc.num_texels, 1),), fill, dtype=torch.uint8, device=DEV)
        ctx.sun_coverage(to_sun, S, cover.data_ptr(), mode, s.cuda_stream)
    s.synchronize()
    return cover.cpu().numpy()[:sc.num_texels], ctx.sun_stats()


@pytest.mark.parametrize("mode", ["lists", "all"])
@pytest.mark.parametrize("name,S", [(n, S) for n in R.NAMES for S in R.SAMPLES[n]])
def test_cover_and_counts_equal_restatement(torch_cuda, ctxs, name, S, mode):
    sc, to_sun = R.case(name)
    exp = R.restate(name, S)
    got, st = _cover(torch_cuda, ctxs(sc), sc, to_sun, S, mode)
    print(name, S, mode, {k: st[k] for k in st})
    assert {k: st[k] for k in COUNTS} == {k: exp[k] for k in COUNTS}
    assert np.array_equal(got, exp["cover"])
    assert not got[~sc.level0_mask()].any()  # the buffer held 0xFF: the mip texels were written too


@pytest.mark.parametrize("name", ["crossing", "example"])
def test_lists_equal_all_on_seeded_directions(torch_cuda, ctxs, name):
    sc, _ = R.case(name)
    ctx = ctxs(sc)
    rng = np.random.default_rng(20)
    lit = shorter = 0
    for _ in range(32):
        az, el = rng.uniform(0, 360), rng.uniform(1, 80)
        to_sun = fmgi.sun_vector(az, el)
        a, sa = _cover(torch_cuda, ctx, sc, to_sun, 2, "all")
        b, sb = _cover(torch_cuda, ctx, sc, to_sun, 2, "lists")
        assert np.array_equal(a, b), (az, el)
        assert {k: sa[k] for k in COUNTS} == {k: sb[k] for k in COUNTS}, (az, el)
        assert int(a.sum()) == sa["lit"]
        lit += sa["lit"] > 0
        shorter += sb["tests"] < sa["tests"]
    assert lit >= 4  # the sun comes in for some of them
    print(name, "directions with sun:", lit, "with fewer tests through the lists:", shorter)


def _bake(torch, ctx, sc):
    """a lightmap that holds a bake: the first items of the scene's schedule"""
    ctx.plan(2000, rng_offsets=np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        lm = torch.zeros((sc.num_texels, 4), dtype=torch.int64, device=DEV)
        ctx.bake_items(0, min(ctx.total_items, 64), lm.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    return lm


@pytest.mark.parametrize("name,S", [("box", 3), ("tilted12", 2), ("ragged", 8), ("example", 2)])
def test_sun_add_equals_integer_restatement(torch_cuda, ctxs, name, S):
    torch = torch_cuda
    sc, to_sun = R.case(name)
    ctx = ctxs(sc)
    cover_h = R.restate(name, S)["cover"]
    base = _bake(torch, ctx, sc)
    base[:, 3] = 7  # word 3 is not the sun's
    base_h = base.cpu().numpy()
    assert base_h[:, :3].any()
    flux = 65000.0
    colours = np.array([[30.0, 28.0, 24.0], [18, 18, 18], [0.5, 31.5, 0.0], [1, 2, 3], [4, 5, 6], [7, 8, 9],
                        [10, 11, 12], [13, 14, 15], [16.25, 17.5, 19.75]], np.float32)
    s = torch.cuda.Stream(device=DEV)
    for K in (1, 3, 9):
        with torch.cuda.stream(s):
            cover = torch.from_numpy(cover_h).to(DEV)
            lms = [base.clone() for _ in range(K)]
            ctx.sun_add(cover.data_ptr(), to_sun, S, colours[:K], flux, [lm.data_ptr() for lm in lms], s.cuda_stream)
        s.synchronize()
        for k, lm in enumerate(lms):
            exp = R.add(sc, cover_h, to_sun, S, colours[k], flux, base_h)
            got = lm.cpu().numpy()
            assert np.array_equal(got, exp), (K, k)
            assert (got[:, 3] == 7).all() and not np.array_equal(got, base_h)
    with torch.cuda.stream(s):  # an all-zero cover leaves the maps as they are
        zero = torch.zeros(sc.num_texels, dtype=torch.uint8, device=DEV)
        lm = base.clone()
        ctx.sun_add(zero.data_ptr(), to_sun, S, colours[:1], flux, [lm.data_ptr()], s.cuda_stream)
    s.synchronize()
    assert np.array_equal(lm.cpu().numpy(), base_h)


def test_two_streams_equal_two_calls_in_sequence(torch_cuda, ctxs):
    torch = torch_cuda
    sc, d0 = R.case("crossing")
    d1 = np.array(R.LOW, np.float32)
    ctx = ctxs(sc)
    seq = [_cover(torch, ctx, sc, d, 3, "lists")[0] for d in (d0, d1)]
    assert not np.array_equal(seq[0], seq[1]) and seq[0].any() and seq[1].any()
    for _ in range(4):
        streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
        covers = []
        for s, d in zip(streams, (d0, d1)):  # neither call waits for the other on the host
            with torch.cuda.stream(s):
                covers.append(torch.full((sc.num_texels,), 0xFF, dtype=torch.uint8, device=DEV))
                ctx.sun_coverage(d, 3, covers[-1].data_ptr(), "lists", s.cuda_stream)
        lms = [torch.zeros((sc.num_texels, 4), dtype=torch.int64, device=DEV) for _ in range(2)]
        torch.cuda.synchronize()
        for s, d, c, lm in zip(streams, (d0, d1), covers, lms):
            with torch.cuda.stream(s):
                ctx.sun_add(c.data_ptr(), d, 3, [18, 18, 18], 1000.0, [lm.data_ptr()], s.cuda_stream)
        for s in streams:
            s.synchronize()
        for k in range(2):
            assert np.array_equal(covers[k].cpu().numpy(), seq[k])
            exp = R.add(sc, seq[k], (d0, d1)[k], 3, (18, 18, 18), 1000.0, np.zeros((sc.num_texels, 4), np.int64))
            assert np.array_equal(lms[k].cpu().numpy(), exp)


def test_no_windows_and_no_facing_wall_give_zeros(torch_cuda):
    torch = torch_cuda
    box = R._scene("box8")
    cases = {"no windows": (scene.Scene("dark", box.walls, box.windows[:0], box.lights, box.num_texels), R.DIR),
             "no facing wall": (scene.Scene("floor", box.walls[:1], box.windows, box.lights, box.num_texels), (0.3, -1.0, -0.2))}
    for what, (sc, to_sun) in cases.items():
        ctx = fmgi.Context(0)
        try:
            ctx.set_scene(sc)
            for mode in ("lists", "all"):
                got, st = _cover(torch, ctx, sc, to_sun, 4, mode)
                assert not got.any(), (what, mode)
                assert st["crossing"] == 0 and st["lit"] == 0 and st["samples"] > 0, (what, mode)
                assert (st["facing"] == 0) == (what == "no facing wall")
            s = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(s):
                cover = torch.from_numpy(got.copy()).to(DEV)
                lm = torch.full((sc.num_texels, 4), -3, dtype=torch.int64, device=DEV)
                ctx.sun_add(cover.data_ptr(), to_sun, 4, [18, 18, 18], 1000.0, [lm.data_ptr()], s.cuda_stream)
            s.synchronize()
            assert (lm == -3).all().item(), what
        finally:
            ctx.close()


# ---- tools/relight.py ------------------------------------------------------------------------------------------------

def test_relight_tool_with_a_sun(torch_cuda, tmp_path):
    torch = torch_cuda
    sun_a = {"azimuth": 200, "elevation": 35, "rgb": [30, 28, 24]}
    sun_b = {"to_sun": [0.3, -1, 0.8], "rgb": [20, 12, 6]}
    pal = {"windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8}, "lights": {"scale": 0.5}}
    scen = [{"name": "noon", "sun": sun_a}, {"name": "noon_dim", "sun": sun_a, **pal}, {"name": "late", "sun": sun_b, **pal},
            {"name": "overcast", **pal}]
    plain = [{k: v for k, v in e.items() if k != "sun"} for e in scen]
    (tmp_path / "sun.json").write_text(json.dumps(scen))
    (tmp_path / "plain.json").write_text(json.dumps(plain))
    tool = [sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4", "--with-light",
            "--sun-samples", "3"]
    trace = ["--spa", str(E.SPA), "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy")]
    bake = str(tmp_path / "box.npz")
    runs = {"sun": ["--scenarios", str(tmp_path / "sun.json")] + trace,
            "plain": ["--scenarios", str(tmp_path / "plain.json")] + trace,
            "saved": ["--scenarios", str(tmp_path / "sun.json"), "--save-bake", bake] + trace,
            "loaded": ["--scenarios", str(tmp_path / "sun.json"), "--load-bake", bake]}
    out = {}
    for name, extra in runs.items():
        r = subprocess.run(tool + extra + ["-o", str(tmp_path / name)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = r.stdout
    assert "sun: 2 directions, 3 x 3 rays per texel, 3 scenarios" in out["sun"] and "sun:" not in out["plain"]
    assert "0 items traced" in out["loaded"]

    # the API route: histograms per group, recolour, sun_add, finalize
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import relight

    sc = E.lit_box()[0]
    T = sc.num_texels
    ctx = fmgi.Context(0)
    try:
        ctx.set_scene(sc)
        ctx.plan(E.SPA, rng_offsets=np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))
        groups = relight.source_groups(ctx.source_ranges(), False)
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            hists = [torch.zeros((fmgi.COLOUR_STATE_COUNT, T), dtype=torch.int64, device=DEV) for _ in groups]
            for h, (_, b, e, _) in zip(hists, groups):
                ctx.bake_states(b, e, h.data_ptr(), stream=s.cuda_stream)
            lms = [torch.zeros((T, 4), dtype=torch.int64, device=DEV) for _ in scen]
            ctx.recolour([h.data_ptr() for h in hists], [relight.scenario_palettes(e, groups) for e in scen],
                         [lm.data_ptr() for lm in lms], s.cuda_stream)
            no_sun = [lm.clone() for lm in lms]
            cover = torch.empty(T, dtype=torch.uint8, device=DEV)
            for e, lm in zip(scen, lms):
                if "sun" in e:
                    to_sun, rgb = relight.sun_of(e)
                    ctx.sun_coverage(to_sun, 3, cover.data_ptr(), stream=s.cuda_stream)
                    ctx.sun_add(cover.data_ptr(), to_sun, 3, rgb, E.SPA, [lm.data_ptr()], s.cuda_stream)
        s.synchronize()
    finally:
        ctx.close()
    for k, e in enumerate(scen):
        with_sun, without = (O.finalize(lm[k].cpu().numpy()[:, :3], sc.texels()) for lm in (lms, no_sun))
        exp = {"sun": with_sun, "saved": with_sun, "loaded": with_sun, "plain": without}
        assert np.array_equal(with_sun, without) == ("sun" not in e), e["name"]
        for run, tex in exp.items():
            exp_tex, exp_tiles = fmgi.output_tiles(sc, tex, E.SPA)
            got = np.load(tmp_path / run / e["name"] / "texels.npy")
            assert np.array_equal(got.view(np.uint32), exp_tex.view(np.uint32)), (run, e["name"])
            assert np.array_equal(np.load(tmp_path / run / e["name"] / "tiles.npy"), exp_tiles), (run, e["name"])
