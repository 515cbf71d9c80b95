"""GPU tests of the bounced-sun layer (fmgi_rad_cache_sun_bounce / fmgi_sun_add_bounced). Every
comparison is an equality of bits against tests/sun_bounce_restate.py on the cache's own ids.

  real maps     the three cases and the all-zero one, maps from fmgi_sun_coverage at S in {1, 2, 3, 8}, N in {1, 2, 8}
  pass shapes   seeded random bytes on every texel (the masking of walls that do not face, of mip texels), mixed S,
                seeded directions: K in {1, 2, 3, 5, 9, 17, 32, 33} on the lit box (every kp, padding slots, two
                passes), K in {3, 33} on open_tilted (586 jobs: ragged job groups); a K = 33 call == 33 K = 1 calls
  buffers       the outputs hold 0xFF bytes before every call: every float is written
  streams       two calls back to back on one stream, no host synchronise between them
  add           1, 3 and 9 maps in place on a lightmap that holds a bake; word 3 and mip texels kept; zero tables
  errors        what needs a handle to be reached
  relight.py    --sun-bounces 2 against the API route, --sun-bounces 0 against a run without the option
The caches have 832 and 586 jobs.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import fm_oracle as O
import fmgi
import rad_cache_cases as CASES
import recolour_events as E
import sun_bounce_restate as B
from conftest import GOLDEN, REPO
from fmgi import _lib

f32 = np.float32
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARG = -3
KMAX, NSYN = 33, 2

_caches, _ctxs, _memo = {}, {}, {}


def _cache(libc, key):
    """the scene's RadCache, traced from the case's libc position"""
    if key not in _caches:
        CASES.seed(libc, key)
        _caches[key] = fmgi.RadCache(CASES.get_scene(key))
    return _caches[key]


def _sids(libc, key):
    if ("sids", key) not in _memo:
        _memo[("sids", key)] = _cache(libc, key).sids()
    return _memo[("sids", key)]


def _ctx(key):
    if key not in _ctxs:
        ctx = fmgi.Context(0)
        ctx.set_scene(CASES.get_scene(key))
        _ctxs[key] = ctx
    return _ctxs[key]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for rc in _caches.values():
        rc.close()
    for ctx in _ctxs.values():
        ctx.close()
    _caches.clear(), _ctxs.clear(), _memo.clear()


def _bounce(torch, rc, covers, dirs, samples, n, stream=None, sync=True):
    """fmgi_rad_cache_sun_bounce into buffers that hold 0xFF bytes: (the device tensor [K, n, T], what to keep alive)"""
    lib = _lib.load()
    k, T = len(covers), rc.num_texels
    s = stream or torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        dev = [torch.from_numpy(np.array(c)).to(DEV) if isinstance(c, np.ndarray) else c for c in covers]
        out = torch.full((k, n, T * 4), 0xFF, dtype=torch.uint8, device=DEV)
        cp = (C.c_void_p * k)(*[d.data_ptr() for d in dev])
        op = (C.c_void_p * k)(*[out[i].data_ptr() for i in range(k)])
        d = np.ascontiguousarray(dirs, f32).reshape(k, 3)
        sa = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, np.int32), (k,)))
        rc_ = lib.fmgi_rad_cache_sun_bounce(rc.h, cp, d.ctypes.data_as(C.c_void_p), sa.ctypes.data_as(C.c_void_p), k, n, op,
                                            C.c_void_p(s.cuda_stream))
    assert rc_ == 0, _lib.last_error()
    if sync:
        s.synchronize()
    return out.view(torch.float32), dev


def _same(got, want):
    g = np.ascontiguousarray(got.cpu().numpy() if hasattr(got, "cpu") else got, f32).view(np.uint32)
    w = np.ascontiguousarray(want, f32).view(np.uint32)
    assert g.shape == w.shape, (g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{int(bad.sum())} values differ, first at {np.argwhere(bad)[:4].tolist()}"


# ---- real maps -------------------------------------------------------------------------------------------------------

def _real(torch, libc, name):
    """(device covers at B.SAMPLES from fmgi_sun_coverage, the restated rows float32 [4, 8, T])"""
    if ("real", name) not in _memo:
        key, sc, to_sun = B.case(name)
        ctx = _ctx(key)
        s = torch.cuda.Stream(device=DEV)
        covers = []
        with torch.cuda.stream(s):
            for S in B.SAMPLES:
                covers.append(torch.full((sc.num_texels,), 0xFF, dtype=torch.uint8, device=DEV))
                ctx.sun_coverage(to_sun, S, covers[-1].data_ptr(), "lists", s.cuda_stream)
        s.synchronize()
        host = [c.cpu().numpy() for c in covers]
        for S, h in zip(B.SAMPLES, host):
            assert np.array_equal(h, B.cover(name, S))
        want = B.bounce(sc, _sids(libc, key), host, [to_sun] * len(host), B.SAMPLES, 8)
        want.setflags(write=False)
        _memo[("real", name)] = (covers, want)
    return _memo[("real", name)]


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("name", B.POSITIVE + B.ZERO)
def test_real_maps_equal_restatement(torch_cuda, libc, name, n):
    key, sc, to_sun = B.case(name)
    covers, want = _real(torch_cuda, libc, name)
    got, _ = _bounce(torch_cuda, _cache(libc, key), covers, [to_sun] * len(covers), B.SAMPLES, n)
    _same(got, want[:, :n])
    assert want[:, :n].any() == (name in B.POSITIVE)


def test_python_wrapper(torch_cuda, libc):
    key, sc, to_sun = B.case("box_lit")
    covers, want = _real(torch_cuda, libc, "box_lit")
    rc = _cache(libc, key)
    got = rc.sun_bounce(covers[1:3], [to_sun, to_sun], B.SAMPLES[1:3], 2)
    torch_cuda.cuda.synchronize()
    assert got.shape == (2, 2, sc.num_texels) and got.is_cuda and got.dtype == torch_cuda.float32
    _same(got, want[1:3, :2])
    s = torch_cuda.cuda.Stream(device=DEV)
    one = rc.sun_bounce([covers[0].data_ptr()], to_sun, 1, 1, stream=s)  # an address, one direction, one int
    s.synchronize()
    _same(one, want[:1, :1])
    with pytest.raises(fmgi.FmgiError, match="to_suns of shape"):
        rc.sun_bounce(covers[:2], [to_sun], 2, 1)
    with pytest.raises(fmgi.FmgiError, match="uint8"):
        rc.sun_bounce([covers[0][:5]], [to_sun], 2, 1)


# ---- pass shapes on synthetic maps ------------------------------------------------------------------------------------

def _synthetic(libc, key):
    """(covers uint8 [KMAX, T], dirs float32 [KMAX, 3], samples int32 [KMAX], restated float32 [KMAX, NSYN, T])"""
    if ("syn", key) not in _memo:
        sc = CASES.get_scene(key)
        rng = np.random.default_rng(21)
        samples = rng.choice([1, 2, 3, 4, 5, 8], KMAX).astype(np.int32)
        covers = np.stack([rng.integers(0, S * S + 1, sc.num_texels).astype(np.uint8) for S in samples])
        dirs = np.stack([fmgi.sun_vector(rng.uniform(0, 360), rng.uniform(-20, 85)) for _ in range(KMAX)])
        dirs *= rng.uniform(0.1, 10, (KMAX, 1)).astype(f32)  # any length
        assert covers[:, ~sc.level0_mask()].any()  # mip texels carry bytes that must be ignored
        facing = np.stack([B.SR.facing_cos(sc, d) > 0 for d in dirs])
        assert (~facing).any(axis=1).all() and facing.any(axis=1).all()  # ... and so do walls that do not face
        want = B.bounce(sc, _sids(libc, key), covers, dirs, samples, NSYN)
        assert all(want[k].any() for k in range(KMAX))
        for a in (covers, dirs, samples, want):
            a.setflags(write=False)
        _memo[("syn", key)] = (covers, dirs, samples, want)
    return _memo[("syn", key)]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 9, 17, 32, 33])
def test_pass_shapes_on_the_lit_box(torch_cuda, libc, k):
    covers, dirs, samples, want = _synthetic(libc, "box_lit")
    got, _ = _bounce(torch_cuda, _cache(libc, "box_lit"), list(covers[:k]), dirs[:k], samples[:k], NSYN)
    _same(got, want[:k])


@pytest.mark.parametrize("k", [3, 33])
def test_pass_shapes_on_the_open_scene(torch_cuda, libc, k):
    rc = _cache(libc, "open_tilted")
    assert rc.info["jobs"] % 64 != 0 and rc.info["jobs"] % 8 != 0
    covers, dirs, samples, want = _synthetic(libc, "open_tilted")
    got, _ = _bounce(torch_cuda, rc, list(covers[:k]), dirs[:k], samples[:k], NSYN)
    _same(got, want[:k])


def test_one_call_equals_one_call_per_direction(torch_cuda, libc):
    covers, dirs, samples, _ = _synthetic(libc, "box_lit")
    rc = _cache(libc, "box_lit")
    dev = [torch_cuda.from_numpy(c.copy()).to(DEV) for c in covers]
    whole, _ = _bounce(torch_cuda, rc, dev, dirs, samples, NSYN)
    whole = whole.cpu().numpy()
    for k in range(KMAX):
        one, _ = _bounce(torch_cuda, rc, dev[k:k + 1], dirs[k:k + 1], samples[k:k + 1], NSYN)
        _same(one[0], whole[k])


def test_every_float_is_written(torch_cuda, libc):
    """zero maps: the rows are all +0, and nothing of the 0xFF fill is left, mip texels and all"""
    rc = _cache(libc, "box_lit")
    sc = CASES.get_scene("box_lit")
    zero = [np.zeros(sc.num_texels, np.uint8)] * 3
    got, _ = _bounce(torch_cuda, rc, zero, [B.SR.DIR] * 3, 2, 8)
    assert got.shape == (3, 8, sc.num_texels) and not got.cpu().numpy().view(np.uint32).any()


def test_two_calls_back_to_back_on_one_stream(torch_cuda, libc):
    """the second call reuses the first one's scratch, with other slots per texel; its stream waits, the host does not"""
    covers, dirs, samples, want = _synthetic(libc, "box_lit")
    rc = _cache(libc, "box_lit")
    s = torch_cuda.cuda.Stream(device=DEV)
    a, keep_a = _bounce(torch_cuda, rc, list(covers[:9]), dirs[:9], samples[:9], NSYN, stream=s, sync=False)
    b, keep_b = _bounce(torch_cuda, rc, list(covers[9:12]), dirs[9:12], samples[9:12], 1, stream=s, sync=False)
    c, keep_c = _bounce(torch_cuda, rc, list(covers[12:13]), dirs[12:13], samples[12:13], NSYN, stream=s, sync=False)
    s.synchronize()
    _same(a, want[:9])
    _same(b, want[9:12, :1])
    _same(c, want[12:13])


# ---- fmgi_sun_add_bounced -----------------------------------------------------------------------------------------

def _bake(torch, ctx, sc):
    """a lightmap that holds a bake: the first items of the scene's schedule"""
    ctx.plan(2000, rng_offsets=np.load(os.path.join(GOLDEN, "glibc_rand_4096.npy")))
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        lm = torch.zeros((sc.num_texels, 4), dtype=torch.int64, device=DEV)
        ctx.bake_items(0, min(ctx.total_items, 64), lm.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    return lm


@pytest.mark.parametrize("name,n", [("box_lit", 8), ("box_lit_skew", 2), ("open_tilted", 3)])
def test_add_bounced_equals_restatement(torch_cuda, libc, name, n):
    torch = torch_cuda
    key, sc, _ = B.case(name)
    ctx = _ctx(key)
    g_h = np.array(_real(torch, libc, name)[1][1, :n])  # S = 2; a writable copy for torch
    base = _bake(torch, ctx, sc)
    base[:, 3] = 7  # word 3 is not the sun's
    base[torch.from_numpy(~sc.level0_mask()).to(DEV), :3] = 5  # ... and neither are the mip texels, which a bake leaves 0
    base_h = base.cpu().numpy()
    assert base_h[sc.level0_mask(), :3].any() and (base_h[~sc.level0_mask(), :3] == 5).all()
    flux = 65000.0
    colours = np.array([[30.0, 28.0, 24.0], [18, 18, 18], [0.5, 31.5, 0.0], [1, 2, 3], [4, 5, 6], [7, 8, 9],
                        [10, 11, 12], [13, 14, 15], [16.25, 17.5, 19.75]], f32)
    refls = np.array([[0.9, 0.9, 0.9], [1.0, 0.5, 0.0], [0.3, 0.6, 1.0], [0.9, 0.85, 0.7], [1, 1, 1], [0, 0, 0],
                      [0.123, 0.456, 0.789], [0.5, 0.5, 0.5], [0.99, 0.01, 0.7]], f32)
    s = torch.cuda.Stream(device=DEV)
    for K in (1, 3, 9):
        with torch.cuda.stream(s):
            g = torch.from_numpy(g_h).to(DEV)
            lms = [base.clone() for _ in range(K)]
            ctx.sun_add_bounced(g.data_ptr(), n, colours[:K], refls[:K], flux, [lm.data_ptr() for lm in lms], s.cuda_stream)
        s.synchronize()
        for k, lm in enumerate(lms):
            exp = B.add(sc, g_h, colours[k], refls[k], flux, base_h)
            got = lm.cpu().numpy()
            assert np.array_equal(got, exp), (K, k)
            assert (got[:, 3] == 7).all() and np.array_equal(got[~sc.level0_mask()], base_h[~sc.level0_mask()])
            assert np.array_equal(got, base_h) == (not refls[k].any()), (K, k)
    with torch.cuda.stream(s):  # all-zero tables leave the map as it is
        zero = torch.zeros((n, sc.num_texels), dtype=torch.float32, device=DEV)
        lm = base.clone()
        ctx.sun_add_bounced(zero.data_ptr(), n, colours[:1], refls[:1], flux, [lm.data_ptr()], s.cuda_stream)
    s.synchronize()
    assert np.array_equal(lm.cpu().numpy(), base_h)


# ---- argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors_with_a_handle(torch_cuda, libc):
    lib = _lib.load()
    rc = _cache(libc, "box_lit")
    one = (C.c_void_p * 1)(64)
    two = (C.c_void_p * 2)(64, None)
    d = (C.c_float * 6)(0.3, -1.0, 0.8, 0.3, -1.0, 0.8)
    sa = (C.c_int * 2)(2, 2)
    call = lib.fmgi_rad_cache_sun_bounce
    ok = (rc.h, one, d, sa, 1, 2, one, None)

    def but(i, v):
        return ok[:i] + (v,) + ok[i + 1:]

    for i in (1, 2, 3, 6):
        assert call(*but(i, None)) == ARG and "null" in _lib.last_error()
    for n in (0, -1):
        assert call(*but(4, n)) == ARG and "num_dirs" in _lib.last_error()
    for n in (0, 9, -1):
        assert call(*but(5, n)) == ARG and "bounces" in _lib.last_error()
    assert call(rc.h, two, d, sa, 2, 2, (C.c_void_p * 2)(64, 64), None) == ARG and "NULL" in _lib.last_error()
    assert call(rc.h, (C.c_void_p * 2)(64, 64), d, sa, 2, 2, two, None) == ARG and "NULL" in _lib.last_error()
    for bad in (0, 9, -1):
        assert call(*but(3, (C.c_int * 1)(bad))) == ARG and "samples" in _lib.last_error()
    for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0), (3e38, 3e38, 0), (1e-30, 0, 0)):
        assert call(*but(2, (C.c_float * 3)(*bad))) == ARG and "to_sun" in _lib.last_error()
    # the handle is still good
    covers, want = _real(torch_cuda, libc, "box_lit")
    got, _ = _bounce(torch_cuda, rc, covers[:1], [B.SR.DIR], 1, 1)
    _same(got, want[:1, :1])


# ---- tools/relight.py -------------------------------------------------------------------------------------------------

def test_relight_tool_with_bounced_sun(torch_cuda, libc, tmp_path):
    torch = torch_cuda
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import relight
    finally:
        sys.path.pop(0)
    sun_a = {"azimuth": 200, "elevation": 35, "rgb": [30, 28, 24]}
    sun_b = {"to_sun": [0.3, -1, 0.8], "rgb": [20, 12, 6]}
    pal = {"windows": {"window_rgb": [2.5, 1.75, 3.0], "albedo": 0.8}, "lights": {"scale": 0.5}}
    scen = [{"name": "noon", "sun": sun_a}, {"name": "noon_dim", "sun": sun_a, **pal}, {"name": "late", "sun": sun_b, **pal},
            {"name": "overcast", **pal}]
    (tmp_path / "sun.json").write_text(json.dumps(scen))
    refl = [0.9, 0.7, 0.5]
    tool = ["box200", "--tile-size", "4", "--with-light", "--sun-samples", "3", "--spa", str(E.SPA), "--offsets",
            os.path.join(GOLDEN, "glibc_rand_4096.npy"), "--scenarios", str(tmp_path / "sun.json")]
    runs = {"plain": [], "zero": ["--sun-bounces", "0", "--sun-reflectance", *map(str, refl)],
            "two": ["--sun-bounces", "2", "--sun-reflectance", *map(str, refl)]}
    fmgi.Context(0).close()  # the runtime is up before the stream is seeded: its start draws from libc rand()
    torch.zeros(1, device=DEV)
    for name, extra in runs.items():
        libc.srand(11)
        relight.main(tool + extra + ["-o", str(tmp_path / name)])
    for e in scen:  # no bounces: the bytes of a run without the option
        for f in ("texels.npy", "tiles.npy"):
            assert (tmp_path / "zero" / e["name"] / f).read_bytes() == (tmp_path / "plain" / e["name"] / f).read_bytes()

    # the API route: histograms per group, recolour, sun_add, the form factors, sun_bounce, sun_add_bounced, finalize
    sc = E.lit_box()[0]
    T = sc.num_texels
    ctx = fmgi.Context(0)
    rad = None
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
            libc.srand(11)
            rad = fmgi.RadCache(sc)
            direct = []
            for e, lm in zip(scen, lms):
                if "sun" in e:
                    to_sun, rgb = relight.sun_of(e)
                    cover = torch.empty(T, dtype=torch.uint8, device=DEV)
                    ctx.sun_coverage(to_sun, 3, cover.data_ptr(), stream=s.cuda_stream)
                    ctx.sun_add(cover.data_ptr(), to_sun, 3, rgb, E.SPA, [lm.data_ptr()], s.cuda_stream)
                    direct.append(lm.clone())
                    g = rad.sun_bounce([cover], [to_sun], 3, 2, stream=s)
                    ctx.sun_add_bounced(g[0].data_ptr(), 2, rgb, refl, E.SPA, [lm.data_ptr()], s.cuda_stream)
                else:
                    direct.append(lm.clone())
        s.synchronize()
    finally:
        if rad is not None:
            rad.close()
        ctx.close()
    for k, e in enumerate(scen):
        two, plain = (O.finalize(lm[k].cpu().numpy()[:, :3], sc.texels()) for lm in (lms, direct))
        assert np.array_equal(two, plain) == ("sun" not in e), e["name"]
        for run, tex in {"two": two, "plain": plain}.items():
            exp_tex, exp_tiles = fmgi.output_tiles(sc, tex, E.SPA)
            got = np.load(tmp_path / run / e["name"] / "texels.npy")
            assert np.array_equal(got.view(np.uint32), exp_tex.view(np.uint32)), (run, e["name"])
            assert np.array_equal(np.load(tmp_path / run / e["name"] / "tiles.npy"), exp_tiles), (run, e["name"])
