"""CPU tests of the closed boxes' lattice descriptors (fmgi_lattice_copy; host-only context, no device needed).

The lattice instances of the grid scan (csrc/fmgi_kernels.hip grid_phase1_axes, Lattice = true) skip the grid cell
wherever the kernel's float32 lattice arithmetic calls a hit point sure: there they take rect base + i su + j sv
as the only record of the plane that passes the float filter test |fl(x - c)| <= hw on both axes. Here that
arithmetic is replayed in numpy float32 (same operations, same order) on adversarial and random points of every
plane of box8, box200 and box2000, and each sure point is checked against the filter records themselves. Scenes
whose planes are no uniform lattices must get no descriptors."""
import os

import numpy as np
import pytest

import fmgi
from conftest import GOLDEN

f32 = np.float32
INF = f32(np.inf)


def _tables(sc):
    ctx = fmgi.Context(-1)
    ctx.set_scene(sc)
    lat = ctx.lattice_tables()["lattice"]
    f = ctx.filter_image()
    ctx.close()
    return lat, f


def _plane_records(f, a, c):
    """records {cu, hwu, cv, hwv} [n, 4] and rect indices [n] of class c (0: +n, 1: -n) of axis a"""
    off = 2 * sum(f["J"][:a])
    rows = f["recs"][off + c : off + 2 * f["J"][a] : 2]
    ids = rows[:, 5].copy().view(np.int32)
    keep = ids >= 0
    return rows[keep, 1:5].astype(f32), ids[keep]


def _cell(x, o, inv, m):
    """the kernel's lattice cell and fraction of coordinate x: r = (x - o) * inv, c = floor(med3(r, 0, m)), r - c"""
    r = (np.asarray(x, f32) - f32(o)) * f32(inv)
    c = np.floor(np.minimum(np.maximum(r, f32(0)), f32(m)))
    return c, r - c


def _fkey(x):
    b = np.asarray(x, f32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF) - 1)


def _kfloat(k):
    k = np.asarray(k, np.int64)
    b = np.where(k >= 0, k, (-(k + 1)) | 0x80000000).astype(np.uint32)
    return b.view(f32)


def _bisect(inside, pred, hi):
    """per element, the last float from `inside` (pred true) towards +/-inf for which the monotone pred holds"""
    inn = _fkey(inside)
    out = np.full_like(inn, int(_fkey(INF if hi else -INF)))
    idx = np.arange(len(inn))
    for _ in range(70):
        gap = np.abs(out - inn) > 1
        mid = inn + (out - inn) // 2
        ok = pred(_kfloat(mid), idx)
        inn = np.where(gap & ok, mid, inn)
        out = np.where(gap & ~ok, mid, out)
    return _kfloat(inn)


def _around(x):
    """x and the floats one ulp either side"""
    x = np.asarray(x, f32)
    return np.concatenate([x, np.nextafter(x, INF), np.nextafter(x, -INF)])


def _axis_specials(c, hw, o, inv, m, lo, hi, n):
    """the coordinates where an axis can go wrong: every record's passing-interval ends, every column's
    sure-interval ends, the box edges, each with the floats one ulp either side; and the columns' centres"""
    ends = [_bisect(c, lambda x, i: np.abs(x - c[i]) <= hw[i], side) for side in (False, True)]
    cols = np.arange(n)
    fi = cols.astype(f32)
    mids = ((fi + f32(0.5)) / f32(inv) + f32(o)).astype(f32)
    cm, fm = _cell(mids, o, inv, m)
    assert np.array_equal(cm, fi) and ((fm >= lo) & (fm <= hi)).all(), "a column's centre is not sure"

    def sure(x, i):
        cc, ff = _cell(x, o, inv, m)
        return (cc == fi[i]) & (ff >= f32(lo)) & (ff <= f32(hi))

    s_lo, s_hi = _bisect(mids, sure, False), _bisect(mids, sure, True)
    box = np.array([(c - hw).min(), (c + hw).max()], f32)
    return np.unique(np.concatenate([_around(e) for e in (*ends, s_lo, s_hi, box)] + [mids])), (s_lo, s_hi)


def _check_plane(d, recs, ids, rng, nrand=20000):
    cu, hwu, cv, hwv = (recs[:, k] for k in range(4))
    assert int(d["nu"]) * int(d["nv"]) == len(ids)
    assert d["mu"] == d["nu"] - 1 and d["mv"] == d["nv"] - 1
    su_, (ulo, uhi) = _axis_specials(cu, hwu, d["u0"], d["iu"], d["mu"], d["lo_u"], d["hi_u"], int(d["nu"]))
    sv_, (vlo, vhi) = _axis_specials(cv, hwv, d["v0"], d["iv"], d["mv"], d["lo_v"], d["hi_v"], int(d["nv"]))
    assert (ulo <= uhi).all() and (vlo <= vhi).all()
    gu, gv = np.meshgrid(su_, sv_, indexing="ij")
    b_u, b_v = ((cu - hwu).min(), (cu + hwu).max()), ((cv - hwv).min(), (cv + hwv).max())
    ru = rng.uniform(b_u[0], b_u[1], nrand).astype(f32)
    rv = rng.uniform(b_v[0], b_v[1], nrand).astype(f32)
    # far outside the box, infinities and NaN: never sure
    odd = np.array([-INF, INF, f32(np.nan), f32(-1e30), f32(1e30)], f32)
    U = np.concatenate([gu.ravel(), ru, odd, np.full(len(odd), cu[0], f32)])
    V = np.concatenate([gv.ravel(), rv, np.full(len(odd), cv[0], f32), odd])
    with np.errstate(invalid="ignore"):
        ci, fu = _cell(U, d["u0"], d["iu"], d["mu"])
        cj, fv = _cell(V, d["v0"], d["iv"], d["mv"])
        sure = (fu >= d["lo_u"]) & (fu <= d["hi_u"]) & (fv >= d["lo_v"]) & (fv <= d["hi_v"])
    assert not sure[-2 * len(odd):].any(), "a point far outside the plane, or NaN, is called sure"
    k = np.flatnonzero(sure)
    bad = 0
    for s in range(0, len(k), 4096):  # (points x records in slabs)
        kk = k[s : s + 4096]
        inside = (np.abs(U[kk, None] - cu[None, :]) <= hwu[None, :]) & (np.abs(V[kk, None] - cv[None, :]) <= hwv[None, :])
        want = int(d["base"]) + ci[kk].astype(np.int64) * int(d["su"]) + cj[kk].astype(np.int64) * int(d["sv"])
        one = inside.sum(axis=1) == 1
        got = ids[np.argmax(inside, axis=1)]
        bad += int((~one | (got != want)).sum())
    assert bad == 0, f"{bad} sure points that do not pass exactly the lattice cell's record"
    # every lattice cell's index is a record of this plane, each once
    ii, jj = np.meshgrid(np.arange(int(d["nu"])), np.arange(int(d["nv"])), indexing="ij")
    assert sorted((int(d["base"]) + ii * int(d["su"]) + jj * int(d["sv"])).ravel().tolist()) == sorted(ids.tolist())
    share = float(sure[gu.size : gu.size + nrand].mean())
    return share, len(k)


def _box(name, box200, box2000):
    from fmgi import scene

    return {"box8": lambda: scene.box_scene(8), "box200": lambda: box200, "box2000": lambda: box2000}[name]()


@pytest.mark.parametrize("name,min_share", [("box8", 0.0), ("box200", 0.995), ("box2000", 0.99)])
def test_sure_points_pass_exactly_their_lattice_record(name, min_share, box200, box2000):
    sc = _box(name, box200, box2000)
    lat, f = _tables(sc)
    assert len(lat) == 6, "every plane of a closed box is a lattice"
    rng = np.random.default_rng(5)
    seen = 0
    sure_rand = []
    for a in range(3):
        for c in range(2):
            recs, ids = _plane_records(f, a, c)
            share, nsure = _check_plane(lat[2 * a + c], recs, ids, rng)
            assert nsure > 0
            sure_rand.append(share)
            seen += len(ids)
    assert seen == len(sc.walls)
    print(f"{name}: sure share of uniform points per plane {[round(s, 5) for s in sure_rand]}")
    # against a vacuous pass: the band leaves almost every uniform point of the plane on the lattice path
    assert min(sure_rand) >= min_share, sure_rand
    assert float(np.mean(sure_rand)) >= min_share


def _shifted_box200(box200):
    """box200 with the floor's interior edge x = xs[3] moved by 0.3 m for one row of rects: both neighbours
    are adjusted, so the floor stays closed, but it is no uniform lattice any more"""
    walls = box200.walls.copy()
    g = 6
    j, i = 2, 2  # floor rect (i, j) = walls[j * g + i]: pos at its x end, width -dx (scene.box_scene)
    left, right = walls[j * g + i], walls[j * g + i + 1]
    d = f32(0.3)
    edge = f32(left["pos"][0] + d)
    assert left["pos"][0] == f32(right["pos"][0] + right["width"][0])  # the shared edge
    x0 = f32(left["pos"][0] + left["width"][0])
    left["pos"][0] = edge
    left["width"][0] = f32(x0 - edge)
    right["width"][0] = f32(edge - right["pos"][0])
    walls[j * g + i], walls[j * g + i + 1] = left, right
    from fmgi.scene import Scene

    return Scene("box200_shifted", walls, box200.windows, box200.lights, box200.num_texels)


def _no_lattice_scene(name, example_scene, box200):
    from fmgi import scene

    return {"example": lambda: example_scene,
            "apartment30": lambda: scene.load_geometry(os.path.join(GOLDEN, "apartment30_geometry.bin"), "a30"),
            "tilted": lambda: scene.tilted_scene(),
            "shifted": lambda: _shifted_box200(box200)}[name]()


@pytest.mark.parametrize("name", ["example", "apartment30", "tilted", "shifted"])
def test_scenes_without_a_lattice_get_none(name, example_scene, box200):
    lat, _ = _tables(_no_lattice_scene(name, example_scene, box200))
    assert len(lat) == 0


def test_shifted_box_is_still_closed(box200):
    """the shifted floor covers what the floor covered: the two rects still meet and keep their outer edges"""
    sc = _shifted_box200(box200)
    a, b = sc.walls[2 * 6 + 2], sc.walls[2 * 6 + 3]
    oa, ob = box200.walls[2 * 6 + 2], box200.walls[2 * 6 + 3]
    assert a["pos"][0] == f32(b["pos"][0] + b["width"][0])
    assert f32(a["pos"][0] + a["width"][0]) == f32(oa["pos"][0] + oa["width"][0]) and b["pos"][0] == ob["pos"][0]
    assert abs(float(a["pos"][0]) - float(oa["pos"][0])) == pytest.approx(0.3, abs=1e-6)


def test_option_is_known_to_the_binding():
    from fmgi._lib import OPTIONS

    assert OPTIONS["lattice"] == 9
    ctx = fmgi.Context(-1)
    for v in (-1, 0, 1):
        ctx.set_option("lattice", v)
    for bad in (2, -2):
        with pytest.raises(fmgi.FmgiError, match=r"\(-3\)"):  # FMGI_ERR_ARG
            ctx.set_option("lattice", bad)
    ctx.close()
