"""A numpy restatement of a radiosity cache's solve (include/flatmatch_gi.h), written from the
definition and the reference's lines, not from the kernels:

  radiosityNative.c:108-131   the windows' and lights' texels are appended after numTexels, mip levels included
  radiosityNative.c:135-145   walls start at 0, every texel of emitter e at emit[k][e]
  radiosityNative.c:232-240   dest[t] += src[id] for rays 0..9999 in order, skipping id < 0
  radiosityNative.c:242-247   src = src * (1 - 0.3f) + dest * (0.3f / 10000): two rounded products, one add
  rectangle.c:508-575         mipmap(): add4's order a + b + c + d, times 0.25f; the 1-D steps (a + b) * 0.5f

Everything is float32; the K sets ride along as an array axis and never meet.
"""
import numpy as np

f32 = np.float32
RAYS = 10000
KEEP = f32(1) - f32(0.3)
GAIN = f32(0.3) / f32(RAYS)


def num_mip_texels(w, h):
    """rectangle.c:166-190"""
    n = w * h
    while w > 1 or h > 1:
        if w > 1:
            w //= 2
        if h > 1:
            h //= 2
        n += w * h
    return n


def layout(sc):
    """(rects as (base, w, h) for walls, windows, lights; the texel count with the emitters' texels)"""
    rects = [(int(r["lm"][0]), int(r["lm"][1]), int(r["lm"][2])) for r in sc.walls]
    ntex = int(sc.num_texels)
    for r in list(sc.windows) + list(sc.lights):
        w, h = int(r["lm"][1]), int(r["lm"][2])
        rects.append((ntex, w, h))
        ntex += num_mip_texels(w, h)
    return rects, ntex


def job_texels(sc):
    """the level-0 texel of every job, wall/tile order (radiosityNative.c:166-176)"""
    out = [np.arange(int(r["lm"][1]) * int(r["lm"][2]), dtype=np.int64) + int(r["lm"][0]) for r in sc.walls]
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def reference_emit(sc):
    """radiosityNative.c:139-142"""
    return np.array([[30, 30, 30]] * len(sc.windows) + [[28, 28, 32]] * len(sc.lights), f32).reshape(-1, 3)


def mipmap(t, base, w, h):
    """rectangle.c:535-569 on t[texel, set, channel], in place"""
    while w > 1 or h > 1:
        if w == 1 or h == 1:
            m = w if h == 1 else h
            s = t[base:base + m]
            t[base + m:base + m + m // 2] = (s[0::2] + s[1::2]) * f32(0.5)
            base += m
            if h == 1:
                w = m // 2
            else:
                h = m // 2
        else:
            s = t[base:base + w * h].reshape(h, w, *t.shape[1:])
            a, b, c, d = s[0::2, 0::2], s[1::2, 0::2], s[0::2, 1::2], s[1::2, 1::2]
            avg = (((a + b) + c) + d) * f32(0.25)
            t[base + w * h:base + w * h + (w // 2) * (h // 2)] = avg.reshape(-1, *t.shape[1:])
            base += w * h
            w //= 2
            h //= 2


def solve(sc, sids, emit, iterations=7):
    """sids int32 [jobs, 10000], emit [K, windows + lights, 3] -> float32 [K, numTexels, 4], w = 0.
    iterations may be a tuple: the rounds run once and {n: the result of n rounds} comes back (the state after
    round n is the result of n rounds, since every round ends with its mipmap)."""
    if not isinstance(iterations, int):
        return _solve(sc, sids, emit, sorted(iterations))
    return _solve(sc, sids, emit, [iterations])[iterations]


def _solve(sc, sids, emit, wanted):
    emit = np.asarray(emit, f32)
    k = emit.shape[0]
    rects, ntex = layout(sc)
    nwalls = len(sc.walls)
    assert emit.shape == (k, len(rects) - nwalls, 3)
    jobs = job_texels(sc)
    sids = np.asarray(sids)
    assert sids.shape == (len(jobs), RAYS)
    src = np.zeros((ntex, k, 3), f32)
    for e, (base, w, h) in enumerate(rects[nwalls:]):
        src[base:base + num_mip_texels(w, h)] = emit[:, e]
    cols = np.ascontiguousarray(sids.T)
    results = {}
    for it in range(1, wanted[-1] + 1):
        acc = np.zeros((len(jobs), k, 3), f32)
        for ray in range(RAYS):
            ids = cols[ray]
            acc = np.where((ids >= 0)[:, None, None], acc + src[np.maximum(ids, 0)], acc)
        dest = np.zeros_like(src)
        dest[jobs] = acc
        src = src * KEEP + dest * GAIN
        assert src.dtype == f32
        for base, w, h in rects:
            mipmap(src, base, w, h)
        if it in wanted:
            out = np.zeros((k, int(sc.num_texels), 4), f32)
            out[:, :, :3] = src[:int(sc.num_texels)].transpose(1, 0, 2)
            results[it] = out
    return results
