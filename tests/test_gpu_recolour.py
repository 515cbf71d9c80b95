"""GPU tests of the per-state photon histograms and their recolouring: fmgi_bake_states against
the histogram derived from the oracle's events, fmgi_recolour against fmgi_bake_items, the oracle and Python
integers, bit for bit; synthetic histograms for the kernel's shapes (texel counts that are no multiple of a
wave, two passes, counts of 2^32 and more); and tools/relight.py against the API path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import recolour_events as R
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
EVENING = dict(window_rgb=(2.5, 1.75, 3.0), light_rgb=(31.5, 24.0, 12.125), floor_tint=(0.9, 0.6, 0.3), albedo=0.77)
OFF = dict(window_rgb=(0, 0, 0), light_rgb=(0, 0, 0))


class Env:
    """one context on the lit box, a stream, and the device work the tests share (each made once)"""

    def __init__(self, torch):
        self.torch = torch
        self.sc, self.L, self.offsets = R.lit_box()
        self.T = self.sc.num_texels
        self.ctx = fmgi.Context(0)
        self.ctx.set_scene(self.sc)
        assert self.ctx.plan(R.SPA, rng_offsets=self.offsets) == 512
        self.s = torch.cuda.Stream(device="cuda:0")
        self._cache = {}

    def zeros(self, *shape):
        with self.torch.cuda.stream(self.s):
            return self.torch.zeros(shape, dtype=self.torch.int64, device="cuda:0")

    def hist(self, ranges, kernel=fmgi.KERNEL_AUTO):
        """device histogram of the item ranges (cached; never modified by a test)"""
        key = (tuple(ranges), kernel)
        if key not in self._cache:
            h = self.zeros(1024, self.T)
            for b, e in ranges:
                self.ctx.bake_states(b, e, h.data_ptr(), kernel, self.s.cuda_stream)
            self.s.synchronize()
            self._cache[key] = h
        return self._cache[key]

    def bake(self, b, e):
        lm = self.zeros(self.T, 4)
        self.ctx.bake_items(b, e, lm.data_ptr(), fmgi.KERNEL_AUTO, self.s.cuda_stream)
        self.s.synchronize()
        return lm.cpu().numpy()

    def recolour(self, hists, palettes, lms=None):
        lms = [self.zeros(self.T, 4) for _ in palettes] if lms is None else lms
        self.ctx.recolour([h.data_ptr() for h in hists], palettes, [lm.data_ptr() for lm in lms], self.s.cuda_stream)
        self.s.synchronize()
        return lms

    def oracle(self, b, e):
        key = ("oracle", b, e)
        if key not in self._cache:
            lm = O.bake(self.sc, self.L, b, e)[0]
            lm.setflags(write=False)
            self._cache[key] = lm
        return self._cache[key]


@pytest.fixture(scope="module")
def env(torch_cuda):
    e = Env(torch_cuda)
    yield e
    e.ctx.close()


@pytest.mark.parametrize("kernel", [fmgi.KERNEL_AUTO, fmgi.KERNEL_EXACT], ids=["auto", "exact"])
def test_histogram_equals_the_events(env, kernel):
    mode = env.ctx.accumulation
    got = env.hist(R.RANGES, kernel).cpu().numpy()
    assert env.ctx.accumulation == mode
    exp = R.dense_histogram().astype(np.int64)
    print(f"deposits {int(exp.sum())}, non-empty cells {int((exp != 0).sum())}, largest count {int(exp.max())}")
    assert np.array_equal(got, exp)


def test_reference_palette_equals_bake_items_and_the_oracle(env):
    whole = env.hist(((0, 512),))
    lm = env.recolour([whole], [[fmgi.Palette.reference()]])[0].cpu().numpy()
    assert not lm[:, 3].any()
    assert np.array_equal(lm, env.bake(0, 512))
    assert np.array_equal(lm[:, :3], env.oracle(0, 512))
    st = env.hist(((0, 512),)).cpu().numpy()
    print(f"deposits {int(st.sum())}, states {int((st.sum(1) != 0).sum())}, cells {int((st != 0).sum())}, max {int(st.max())}")


def test_recolour_leaves_the_histogram_and_the_context_alone(env):
    whole = env.hist(((0, 512),))
    before = whole.clone()
    mode = env.ctx.accumulation
    lm = env.zeros(env.T, 4)
    lm[:, 3] = 7  # .s[3] is not touched
    env.recolour([whole], [[fmgi.Palette()]], [lm])
    once = lm.cpu().numpy().copy()
    env.recolour([whole], [[fmgi.Palette()]], [lm])
    twice = lm.cpu().numpy()
    assert env.torch.equal(whole, before)
    assert (once[:, 3] == 7).all() and (twice[:, 3] == 7).all()
    assert np.array_equal(twice[:, :3], 2 * once[:, :3]) and np.array_equal(once[:, :3], env.oracle(0, 512))
    assert env.ctx.accumulation == mode == fmgi.ACCUM_STREAM
    assert np.array_equal(env.bake(0, 512)[:, :3], env.oracle(0, 512))
    assert "AccState" not in env.ctx.last_bake_kernel


def test_groups_add_up(env):
    window, lamp, whole = env.hist(((0, 256),)), env.hist(((256, 512),)), env.hist(((0, 512),))
    assert env.torch.equal(window + lamp, whole)
    ref, off = fmgi.Palette(), fmgi.Palette(**OFF)
    day, no_lamp, no_window = env.recolour([window, lamp], [[ref, ref], [ref, off], [off, ref]])
    assert np.array_equal(day.cpu().numpy()[:, :3], env.oracle(0, 512))
    assert np.array_equal(no_lamp.cpu().numpy(), env.bake(0, 256))
    assert np.array_equal(no_window.cpu().numpy()[:, :3], env.oracle(256, 512))
    # a palette of its own per group, against Python integers over the event-derived histogram
    sparse = R.sparse_histogram()
    pal = fmgi.Palette(**EVENING)
    exp = np.array(R.fold(sparse, fmgi.palette_table(pal), env.T), dtype=np.int64)
    got = env.recolour([env.hist(R.RANGES)], [[pal]])[0].cpu().numpy()
    assert exp.any() and np.array_equal(got[:, :3], exp) and not got[:, 3].any()


# ---- synthetic histograms: the kernel alone -------------------------------------------------------------------

def _palettes(K, G):
    rng = np.random.default_rng(11)
    rows = []
    for k in range(K):
        row = []
        for g in range(G):
            row.append(fmgi.Palette(window_rgb=rng.uniform(0, 31.9, 3), light_rgb=rng.uniform(0, 31.9, 3),
                                    floor_tint=rng.uniform(0, 1, 3), albedo=rng.uniform(0.3, 1)))
        rows.append(row)
    rows[0][0] = fmgi.Palette(window_rgb=(15.999, 31.999, 0.5), albedo=1.0)  # table[513] near 2^29 and 2^30
    if K > 2:
        rows[2] = [fmgi.Palette(**OFF) for _ in range(G)]                   # a scenario with everything off
    if G > 1 and K > 1:
        rows[1][1] = fmgi.Palette(**OFF)                                      # one group off in one scenario
    return rows


_SYN = {}


def _synthetic(torch, T, G):
    """counts [G][1024][T] at about 2 % density with the special cells, and its exact fold with 9 scenarios"""
    if (T, G) in _SYN:
        return _SYN[(T, G)]
    gen = torch.Generator().manual_seed(1000 * T + G)
    counts = torch.randint(1, 200, (G, 1024, T), generator=gen, dtype=torch.int64)
    counts *= (torch.rand((G, 1024, T), generator=gen) < 0.02).to(torch.int64)
    counts[:, 0, :] = 3                       # rows 0 and 512 hold counts, and contribute nothing
    counts[:, 512, :] = 5
    counts[:, 1023, :] = 2                    # a full row of the last state
    counts[G - 1, 1, T - 1] = 9               # the last texel of the lowest live state
    big = [(0, 513, T // 2, (1 << 32) + 5), (G - 1, 1023, T - 1, (1 << 40) + (1 << 32) + 1)]
    small = counts.numpy().copy()
    for g, s, t, v in big:
        counts[g, s, t] = v
        small[g, s, t] = 0
    pals = _palettes(9, G)
    tables = np.array([[fmgi.palette_table(p) for p in row] for row in pals])  # [9][G][1024][3]
    assert tables[0, 0, 513, 0] > 0.99 * 2**29 and tables[0, 0, 513, 1] > 0.99 * 2**30
    assert not tables[:, :, 0].any() and not tables[:, :, 512].any()
    # counts < 200 and table values < 2^30: every partial sum is below 2^8 * 2^30 * 1024 * G < 2^63, so the int64
    # products and sums below are the exact integers; the cells of 2^32 and more are added as Python integers
    exp = np.einsum("gst,kgsc->ktc", small, tables, optimize=True)
    assert exp.dtype == np.int64
    exp = exp.astype(object)
    for g, s, t, v in big:
        for k in range(9):
            for c in range(3):
                exp[k, t, c] = (int(exp[k, t, c]) + v * int(tables[k, g, s, c])) & M64
    out = (counts, pals, exp)
    _SYN[(T, G)] = out
    return out


@pytest.mark.parametrize("K", [1, 8, 9])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("T", [1, 63, 257, 2152])
def test_synthetic_histograms(torch_cuda, T, G, K):
    torch = torch_cuda
    counts, pals, exp = _synthetic(torch, T, G)
    from fmgi import scene

    sc = scene.box_scene(200, tile_size=4.0, with_light=True)
    ctx = fmgi.Context(0)
    try:
        ctx.set_scene(scene.Scene(f"synthetic{T}", sc.walls[:0], sc.windows, sc.lights, T))
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            dev = counts.to("cuda:0", non_blocking=False)
            keep = dev.clone()
            lms = torch.full((K, T, 4), 1, dtype=torch.int64, device="cuda:0")  # distinct outputs, all start at 1
            ctx.recolour([dev[g].data_ptr() for g in range(G)], [row for row in pals[:K]],
                         [lms[k].data_ptr() for k in range(K)], s.cuda_stream)
        s.synchronize()
        got = lms.cpu().numpy()
        assert torch.equal(dev, keep)
    finally:
        ctx.close()
    assert (got[:, :, 3] == 1).all()
    want = np.array([[[(int(v) + 1) & M64 for v in px] for px in exp[k]] for k in range(K)], dtype=object)
    have = got[:, :, :3].astype(np.uint64).astype(object)
    assert np.array_equal(have, want)
    if K > 2:
        assert (got[2, :, :3] == 1).all()  # the scenario with everything off


def test_all_zero_histogram(torch_cuda):
    torch = torch_cuda
    from fmgi import scene

    sc = scene.box_scene(200, tile_size=4.0, with_light=True)
    T = 130
    ctx = fmgi.Context(0)
    try:
        ctx.set_scene(scene.Scene("empty", sc.walls[:0], sc.windows, sc.lights, T))
        s = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(s):
            h = torch.zeros((1024, T), dtype=torch.int64, device="cuda:0")
            lm = torch.full((T, 4), -3, dtype=torch.int64, device="cuda:0")
            ctx.recolour([h.data_ptr()], [[fmgi.Palette()]], [lm.data_ptr()], s.cuda_stream)
        s.synchronize()
        assert (lm == -3).all().item()
    finally:
        ctx.close()


def test_relight_tool_equals_the_api_path(env, tmp_path):
    scen = [{"name": "day"}, {"name": "evening", "windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8},
                              "lights": {"scale": 0.5, "floor_tint": [1.0, 0.5, 0.25]}}]
    (tmp_path / "scenarios.json").write_text(json.dumps(scen))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "relight.py"), "box200", "--tile-size", "4",
                        "--with-light", "--spa", str(R.SPA), "--scenarios", str(tmp_path / "scenarios.json"),
                        "--offsets", os.path.join(GOLDEN, "glibc_rand_4096.npy"), "-o", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    window, lamp = env.hist(((0, 256),)), env.hist(((256, 512),))
    pals = [[fmgi.Palette(), fmgi.Palette()],
            [fmgi.Palette(window_rgb=(2.5, 1.75, 3.0), albedo=0.8),
             fmgi.Palette(window_rgb=(9, 9, 9), light_rgb=(8, 8, 9), floor_tint=(1.0, 0.5, 0.25))]]
    lms = env.recolour([window, lamp], pals)
    for name, lm in zip(("day", "evening"), lms):
        tex = O.finalize(lm.cpu().numpy()[:, :3], env.sc.texels())
        exp_tex, exp_tiles = fmgi.output_tiles(env.sc, tex, R.SPA)
        got = np.load(tmp_path / "out" / name / "texels.npy")
        assert exp_tex.any() and np.array_equal(got.view(np.uint32), exp_tex.view(np.uint32)), name
        assert np.array_equal(np.load(tmp_path / "out" / name / "tiles.npy"), exp_tiles), name
