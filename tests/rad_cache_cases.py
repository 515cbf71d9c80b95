"""Scenes, oracle runs and palettes the radiosity cache's tests share (tests/test_rad_cache_host.py,
tests/test_gpu_rad_cache.py). Seeds and scenes are tests/test_offaxis_radiosity.py's: the boxes start at its
mid-stream position (seed 5, 777 draws in), open_tilted at its pinned seed. Everything returned is read-only.
"""
import numpy as np

import fm_oracle as O
import offaxis_scenes as S
import rad_solve_restate as R
import test_offaxis_radiosity as T
from fmgi import scene

f32 = np.float32
NAMES = ("box_lit", "box", "open_tilted")


def get_scene(name):
    if name == "box_lit":
        return scene.box_scene(200, tile_size=2.0, with_light=True)
    if name == "box":
        return scene.box_scene(200, tile_size=2.0)
    return S.get(name)


def seed(libc, name):
    T._seed(libc, name)


_oracle, _restated = {}, {}


def oracle(libc, name):
    """(scene, texels, sids, the next rand()) of the oracle's run from the case's libc position"""
    if name not in _oracle:
        sc = get_scene(name)
        seed(libc, name)
        tex, sids = O.radiosity(sc, with_sids=True)
        nxt = libc.rand()
        tex.setflags(write=False)
        sids.setflags(write=False)
        _oracle[name] = (sc, tex, sids, nxt)
    return _oracle[name]


def palettes(name, count, rng_seed=17):
    """`count` palettes [count, emitters, 3] of a scene: the reference's, its double, all zeros, the first emitter
    alone, then random values spread over 1e-3 .. 1e3 with a tenth of them zero"""
    sc = get_scene(name)
    ref = R.reference_emit(sc)
    e = len(ref)
    rng = np.random.default_rng(rng_seed)
    first = np.zeros_like(ref)
    first[:1] = ref[:1]
    out = [ref, ref * f32(2), np.zeros_like(ref), first]
    while len(out) < count:
        p = (10.0 ** rng.uniform(-3, 3, (e, 3))).astype(f32)
        p[rng.random((e, 3)) < 0.1] = 0
        out.append(p)
    out = np.stack(out[:count]).astype(f32).reshape(count, e, 3)
    out.setflags(write=False)
    return out


def restated(libc, name, count, iterations):
    """{n: float32 [count, numTexels, 4]} for n in `iterations`: the restatement on the oracle's ids, once per case"""
    key = (name, count, tuple(iterations))
    if key not in _restated:
        sc, _, sids, _ = oracle(libc, name)
        res = R.solve(sc, sids, palettes(name, count), tuple(iterations))
        for v in res.values():
            v.setflags(write=False)
        _restated[key] = res
    return _restated[key]
