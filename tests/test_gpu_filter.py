"""GPU tests of the adaptive density filter: fmgi_filter_radii and fmgi_filter_apply against the
restatement (filter_restate.py), bit for bit, on a synthetic scene whose level-0 grids cover the kernels' shapes
(single texels, single rows and columns, rows of one and of two waves, a wall whose prefix sums wrap, a grid that
is no power of two, mip texels between the walls, the last wall ending at numTexels), on a real bake, the quality
property on a device bake, and tools/relight.py --min-deposits against the API path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_restate as F
import fm_oracle as O
import fmgi
import recolour_events as R
from conftest import GOLDEN, REPO
from fmgi import scene

pytestmark = pytest.mark.gpu

M64 = F.M64
GRIDS = [(1, 1), (1, 2), (2, 1), (64, 1), (1, 64), (128, 2), (2, 128), (128, 64), (3, 5)]  # (s1, s2)
MID = 1 << 52


def synthetic_scene():
    sc = scene.box_scene(200, tile_size=4.0, with_light=True)
    walls = sc.walls[: len(GRIDS)].copy()
    for w, (s1, s2) in zip(walls, GRIDS):
        w["lm"][1], w["lm"][2] = s1, s2
    scene.assign_texel_bases(walls)
    last = walls[-1]["lm"]
    T = int(last[0]) + int(last[1]) * int(last[2])  # the last wall's level 0 ends the texel buffer
    return scene.Scene("filter_grids", walls, sc.windows, sc.lights, T)


class Env:
    """one context on the synthetic scene, a stream, and the host data the tests share (made once, never changed)"""

    def __init__(self, torch):
        self.torch = torch
        self.sc = synthetic_scene()
        self.T = T = self.sc.num_texels
        mask = self.sc.level0_mask()
        assert mask[-1] and not mask.all() and T == 11_965
        rng = np.random.default_rng(2024)
        # lightmaps: below 2^53 per channel, so a window of 33 x 33 texels stays below 2^64 while the prefix sums
        # of the 128 x 64 wall (8192 texels, mean 2^52) pass it; .s[3] and the mip texels hold values of their own
        self.maps = rng.integers(0, 1 << 53, (9, T, 4), dtype=np.int64)
        self.maps[:, :, 3] = rng.integers(-(1 << 62), 1 << 62, (9, T), dtype=np.int64)
        assert int(self.maps[0, :, 0].astype(object).sum()) > 1 << 64
        # the guide: 2^(0..53) per channel, so a few texels carry most of the energy and the radii are mixed
        self.guide = (1 << rng.integers(0, 54, (T, 4), dtype=np.int64)).astype(np.int64)
        self.radii = F.radii(self.sc, self.guide, MID, 16)
        assert len(np.unique(self.radii[mask])) >= 6 and not self.radii[~mask].any()
        rad = self.radii.copy()
        rad[::5] = 255          # above 16: treated as 16 (mip texels too: they stay copies)
        rad[1::11] = 17
        self.radii_any = rad
        for a in (self.maps, self.guide, self.radii, self.radii_any):
            a.setflags(write=False)
        self.ctx = fmgi.Context(0)
        self.ctx.set_scene(self.sc)
        self.s = torch.cuda.Stream(device="cuda:0")
        self._exp = {}

    def dev(self, a):
        with self.torch.cuda.stream(self.s):
            return self.torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: the shared arrays are read-only)

    def expected(self, k, which="any"):
        key = (k, which)
        if key not in self._exp:
            self._exp[key] = F.apply(self.sc, self.maps[k], self.radii_any if which == "any" else self.radii)
        return self._exp[key]

    def device_radii(self, guide, E, Rmax):
        g = self.dev(guide)
        out = self.dev(np.full(self.T, 99, np.uint8))
        self.ctx.filter_radii(g.data_ptr(), E, Rmax, out.data_ptr(), self.s.cuda_stream)
        self.s.synchronize()
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def env(torch_cuda):
    e = Env(torch_cuda)
    yield e
    e.ctx.close()


# ---- radii -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [0, MID, M64], ids=["zero", "mid", "max"])
@pytest.mark.parametrize("Rmax", [0, 1, 4, 16])
def test_radii(env, Rmax, E):
    got = env.device_radii(env.guide, E, Rmax)
    exp = F.radii(env.sc, env.guide, E, Rmax)
    assert got.dtype == np.uint8 and np.array_equal(got, exp)
    mask = env.sc.level0_mask()
    if E == 0 or Rmax == 0:
        assert not got.any()
    if E == M64:
        assert (got[mask] == Rmax).all() and not got[~mask].any()


def test_radii_of_an_all_zero_guide(env):
    mask = env.sc.level0_mask()
    zero = np.zeros((env.T, 4), np.int64)
    got = env.device_radii(zero, 1, 7)
    assert (got[mask] == 7).all() and not got[~mask].any()
    assert not env.device_radii(zero, 0, 7).any()


def test_radii_ignore_the_fourth_word_and_wrap_like_the_definition(env):
    g = env.guide.copy()
    g[:, 3] = -1
    g[:, 0] = -5          # e = g0 + g1 + g2 mod 2^64
    for E in (MID, 1 << 63):
        assert np.array_equal(env.device_radii(g, E, 4), F.radii(env.sc, g, E, 4))


# ---- apply -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 8, 9])
def test_apply(env, K):
    torch = env.torch
    src = env.dev(env.maps[:K])
    keep = src.clone()
    out = env.dev(np.full((K, env.T, 4), -7, np.int64))
    rad = env.dev(env.radii_any)
    env.ctx.filter_apply(rad.data_ptr(), [src[k].data_ptr() for k in range(K)], [out[k].data_ptr() for k in range(K)],
                         env.s.cuda_stream)
    env.s.synchronize()
    assert torch.equal(src, keep) and np.array_equal(rad.cpu().numpy(), env.radii_any)
    got = out.cpu().numpy()
    mask = env.sc.level0_mask()
    for k in range(K):
        assert np.array_equal(got[k], env.expected(k)), f"map {k}"
        assert np.array_equal(got[k][~mask], env.maps[k][~mask])       # mip texels: copied, all four words
        assert np.array_equal(got[k][:, 3], env.maps[k][:, 3])
    assert not np.array_equal(got[0][mask], env.maps[0][mask])


def test_apply_in_place(env):
    buf = env.dev(env.maps[:9])
    rad = env.dev(env.radii_any)
    ptrs = [buf[k].data_ptr() for k in range(9)]
    env.ctx.filter_apply(rad.data_ptr(), ptrs, ptrs, env.s.cuda_stream)
    env.s.synchronize()
    got = buf.cpu().numpy()
    for k in range(9):
        assert np.array_equal(got[k], env.expected(k)), f"map {k}"


def test_zero_radii_and_zero_energy_give_the_input(env):
    src = env.dev(env.maps[:2])
    out = env.dev(np.zeros((2, env.T, 4), np.int64))
    rad = env.dev(np.full(env.T, 3, np.uint8))
    env.ctx.filter_radii(src[0].data_ptr(), 0, 16, rad.data_ptr(), env.s.cuda_stream)     # min_energy == 0
    env.ctx.filter_apply(rad.data_ptr(), [src[0].data_ptr()], [out[0].data_ptr()], env.s.cuda_stream)
    env.ctx.filter_radii(src[1].data_ptr(), M64, 0, rad.data_ptr(), env.s.cuda_stream)    # max_radius == 0
    env.ctx.filter_apply(rad.data_ptr(), [src[1].data_ptr()], [out[1].data_ptr()], env.s.cuda_stream)
    env.s.synchronize()
    assert env.torch.equal(out, src) and not rad.any().item()


def test_constant_walls_stay_unchanged(env):
    lm = env.maps[0].copy()
    for k, (s0, s1, s2) in enumerate(F.grids(env.sc)):
        lm[s0 : s0 + s1 * s2, :3] = [(1 << 53) - 1 - k, 3 * k, 1 << 40]
    buf = env.dev(lm)
    rad = env.dev(env.radii_any)
    env.ctx.filter_apply(rad.data_ptr(), [buf.data_ptr()], [buf.data_ptr()], env.s.cuda_stream)
    env.s.synchronize()
    assert np.array_equal(buf.cpu().numpy(), lm)


def test_calls_back_to_back_reuse_the_scratch(env):
    """radii, a nine-map apply (two passes), radii of another guide and a one-map apply on one stream without a
    host synchronisation in between: each call's prefix sums replace the previous call's in the same scratch"""
    g1, g2 = env.dev(env.guide), env.dev(env.maps[3])
    r1, r2 = env.dev(np.zeros(env.T, np.uint8)), env.dev(np.zeros(env.T, np.uint8))
    src = env.dev(env.maps)
    outA, outB = env.dev(np.zeros((9, env.T, 4), np.int64)), env.dev(np.zeros((env.T, 4), np.int64))
    st = env.s.cuda_stream
    env.ctx.filter_radii(g1.data_ptr(), MID, 16, r1.data_ptr(), st)
    env.ctx.filter_apply(r1.data_ptr(), [src[k].data_ptr() for k in range(9)], [outA[k].data_ptr() for k in range(9)], st)
    env.ctx.filter_radii(g2.data_ptr(), 40 << 52, 4, r2.data_ptr(), st)
    env.ctx.filter_apply(r2.data_ptr(), [src[5].data_ptr()], [outB.data_ptr()], st)
    env.s.synchronize()
    assert np.array_equal(r1.cpu().numpy(), env.radii)
    exp2 = F.radii(env.sc, env.maps[3], 40 << 52, 4)
    assert np.array_equal(r2.cpu().numpy(), exp2) and len(np.unique(exp2)) >= 3
    gotA = outA.cpu().numpy()
    for k in range(9):
        assert np.array_equal(gotA[k], env.expected(k, "mid")), f"map {k}"
    assert np.array_equal(outB.cpu().numpy(), F.apply(env.sc, env.maps[5], exp2))


# ---- a real bake -----------------------------------------------------------------------------------------------------

def test_real_bake(torch_cuda):
    torch = torch_cuda
    sc, L, offsets = R.lit_box()
    oracle = O.bake(sc, L, 0, 512)[0]
    E = fmgi.filter_energy(1024)  # (this bake holds some 150 deposits per texel: radii 0 to 4)
    exp_rad = F.radii(sc, oracle, E, 4)
    exp = F.apply(sc, oracle, exp_rad)
    assert len(np.unique(exp_rad)) >= 3 and not np.array_equal(exp, oracle)
    ctx = fmgi.Context(0)
    try:
        ctx.set_scene(sc)
        assert ctx.plan(R.SPA, rng_offsets=offsets) == 512
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            lm = torch.zeros((sc.num_texels, 4), dtype=torch.int64, device="cuda:0")
            out = torch.zeros_like(lm)
            rad = torch.zeros(sc.num_texels, dtype=torch.uint8, device="cuda:0")
            ctx.bake_items(0, 512, lm.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            ctx.filter_radii(lm.data_ptr(), E, 4, rad.data_ptr(), s.cuda_stream)
            ctx.filter_apply(rad.data_ptr(), [lm.data_ptr()], [out.data_ptr()], s.cuda_stream)
        s.synchronize()
        assert np.array_equal(lm.cpu().numpy()[:, :3], oracle)
        assert np.array_equal(rad.cpu().numpy(), exp_rad)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :3], exp) and not got[:, 3].any()
    finally:
        ctx.close()
    # the host-array convenience: the same through a context of its own
    out2, rad2 = fmgi.filter_lightmap(sc, oracle, 1024, 4)
    assert out2.shape == oracle.shape and np.array_equal(out2, exp) and np.array_equal(rad2, exp_rad)
    out3, rad3 = fmgi.filter_lightmap(sc, 2 * oracle, 1024, 2, guide=oracle)
    assert np.array_equal(rad3, F.radii(sc, oracle, E, 2)) and np.array_equal(out3, F.apply(sc, 2 * oracle, rad3))


# ---- quality on the device -------------------------------------------------------------------------------------------

def test_filtered_low_photon_bake_is_closer_to_a_reference_bake(torch_cuda):
    """DESIGN.md §13's box pair, baked and filtered on the device: box_scene(200, tile_size=20.0, with_light=True),
    low bake spa 20,000 with the offsets of glibc_rand_4096.npy, reference bake spa 400,000 with the same
    offsets reversed, filter_energy(256), radius <= 4. Measured on the CPU oracle: L1 0.07299 unfiltered,
    0.04221 filtered, mean radius 0.747."""
    torch = torch_cuda
    sc = scene.box_scene(200, tile_size=20.0, with_light=True)
    offsets = np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))
    ctx = fmgi.Context(0)
    try:
        ctx.set_scene(sc)
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            low, ref, out = (torch.zeros((sc.num_texels, 4), dtype=torch.int64, device="cuda:0") for _ in range(3))
            rad = torch.zeros(sc.num_texels, dtype=torch.uint8, device="cuda:0")
            items = ctx.plan(20_000, rng_offsets=offsets)
            ctx.bake_items(0, items, low.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            s.synchronize()
            items = ctx.plan(400_000, rng_offsets=offsets[::-1].copy())
            ctx.bake_items(0, items, ref.data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            ctx.filter_radii(low.data_ptr(), fmgi.filter_energy(256), 4, rad.data_ptr(), s.cuda_stream)
            ctx.filter_apply(rad.data_ptr(), [low.data_ptr()], [out.data_ptr()], s.cuda_stream)
        s.synchronize()
        low, ref, out, rad = (t.cpu().numpy() for t in (low, ref, out, rad))
    finally:
        ctx.close()
    exp_rad = F.radii(sc, low, fmgi.filter_energy(256), 4)
    assert np.array_equal(rad, exp_rad) and np.array_equal(out, F.apply(sc, low, exp_rad))
    unfiltered, filtered = F.l1_pair(sc, low, out, ref)
    print(f"L1 unfiltered {unfiltered:.5f}, filtered {filtered:.5f}, mean radius {rad.mean():.3f} over "
          f"{sc.num_texels} texels")
    assert filtered < unfiltered


# ---- tools/relight.py ------------------------------------------------------------------------------------------------

def test_relight_tool_with_and_without_the_filter(torch_cuda, tmp_path):
    """box200 at 20 texels per m^2 holds some 30 deposits per texel at this spa, so --min-deposits 64 widens most
    windows; both tool runs (with the filter, and without the flags) must equal the API path"""
    torch = torch_cuda
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": {"scale": 0.5, "floor_tint": [1.0, 0.5, 0.25]}}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    base = [sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "20", "--with-light",
            "--spa", str(R.SPA), "--scenarios", str(tmp_path / "scenarios.json"),
            "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy")]
    runs = {"plain": subprocess.Popen(base + ["-o", str(tmp_path / "plain")], stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True),
            "filtered": subprocess.Popen(base + ["--min-deposits", "64", "-o", str(tmp_path / "filtered")],
                                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)}
    # the API path meanwhile
    sc = scene.box_scene(200, tile_size=20.0, with_light=True)
    offsets = np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy"))
    T = sc.num_texels
    pals = [[fmgi.Palette(), fmgi.Palette()],
            [fmgi.Palette(window_rgb=(2.5, 1.75, 3.0), albedo=0.8),
             fmgi.Palette(window_rgb=(9, 9, 9), light_rgb=(8, 8, 9), floor_tint=(1.0, 0.5, 0.25))]]
    ctx = fmgi.Context(0)
    try:
        ctx.set_scene(sc)
        assert ctx.plan(R.SPA, rng_offsets=offsets) == 512
        assert [r[1:] for r in ctx.source_ranges()] == [(1, 0, 256), (0, 256, 512)]  # the window, then the lamp
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            hists = [torch.zeros((1024, T), dtype=torch.int64, device="cuda:0") for _ in range(2)]
            ctx.bake_states(0, 256, hists[0].data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            ctx.bake_states(256, 512, hists[1].data_ptr(), fmgi.KERNEL_AUTO, s.cuda_stream)
            lms = [torch.zeros((T, 4), dtype=torch.int64, device="cuda:0") for _ in range(3)]
            hp = [h.data_ptr() for h in hists]
            ctx.recolour(hp, pals + [[fmgi.Palette(), fmgi.Palette()]], [lm.data_ptr() for lm in lms], s.cuda_stream)
            s.synchronize()
            plain = [lm.cpu().numpy() for lm in lms[:2]]
            rad = torch.zeros(T, dtype=torch.uint8, device="cuda:0")
            ctx.filter_radii(lms[2].data_ptr(), fmgi.filter_energy(64), 4, rad.data_ptr(), s.cuda_stream)
            ptrs = [lm.data_ptr() for lm in lms[:2]]
            ctx.filter_apply(rad.data_ptr(), ptrs, ptrs, s.cuda_stream)
        s.synchronize()
        filtered = [lm.cpu().numpy() for lm in lms[:2]]
        assert rad.any().item()
    finally:
        ctx.close()
    for name, p in runs.items():
        text, _ = p.communicate(timeout=300)
        assert p.returncode == 0, text
        assert ("filtered:" in text) == (name == "filtered")
    for run, lms_np in (("plain", plain), ("filtered", filtered)):
        for name, lm in zip(("day", "evening"), lms_np):
            tex = O.finalize(lm[:, :3], sc.texels())
            exp_tex, exp_tiles = fmgi.output_tiles(sc, tex, R.SPA)
            got = np.load(tmp_path / run / name / "texels.npy")
            assert exp_tex.any() and np.array_equal(got.view(np.uint32), exp_tex.view(np.uint32)), (run, name)
            assert np.array_equal(np.load(tmp_path / run / name / "tiles.npy"), exp_tiles), (run, name)
    a = np.load(tmp_path / "plain" / "day" / "tiles.npy")
    b = np.load(tmp_path / "filtered" / "day" / "tiles.npy")
    assert not np.array_equal(a, b)
