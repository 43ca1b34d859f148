"""CPU-side checks (no device needed) of the distance-field boundary (include/mon_core.h): the mon_dist_field_* calls, mon_scene_dist_field
and mon_online_dist_field are declared, exported and bound with the header's signatures; the new sources are listed for every build; every argument error is
MON_ERR_ARG before any device work, with a message and the outputs and *field untouched; and the reference the GPU tests compare with
(tests/dist_field_reference.py) is pinned on its own, three ways: exactly on affine fields, against float64 with a derived bound (and against scipy where it
is installed), and by closed forms.  (The rows that need a device are in tests/test_dist_field.py.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, p as _p
import dist_field_reference as dr

NEW = ("mon_dist_field_create", "mon_scene_dist_field", "mon_online_dist_field", "mon_dist_field_info", "mon_dist_field_read", "mon_dist_field_sample",
       "mon_dist_field_score", "mon_dist_field_destroy")
MON_ERR_ARG, MON_ERR_NO_DEVICE = 1, 2
F = np.float32
U = 2.0 ** -24                                                                      # the unit roundoff of float32


def _kind(arg):
    if "*" in arg:
        return "ptr"
    return {"size_t": "u64", "int": "int", "int32_t": "int", "uint32_t": "uint32", "float": "float"}[arg.split()[0]]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [8, 11, 9, 2, 2, 6, 14, 1]
    assert [_kind(a) for a in _decl("mon_dist_field_create")] == ["int", "ptr", "int", "int", "int", "ptr", "ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_scene_dist_field")] == ["ptr", "u64", "int", "ptr", "ptr", "int", "int", "int", "float", "float", "ptr"]
    assert _decl("mon_online_dist_field")[1:] == _decl("mon_scene_dist_field")[3:]                      # "the same from origin3 on"
    assert _decl("mon_scene_dist_field")[:10] == _decl("mon_scene_distance_lattice")[:10]               # the distance call's arguments up to max_dist
    assert [_kind(a) for a in _decl("mon_dist_field_sample")] == ["ptr", "ptr", "u64", "float", "ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_dist_field_score")] == ["ptr", "ptr", "u64", "ptr", "int", "u64", "u64", "u64"] + ["ptr"] * 6
    assert C.sizeof(pkg.DistFieldDesc) == 44 and C.sizeof(pkg.TrajScoreParams) == 12
    for name in ("dist_field_create", "scene_dist_field"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.dist_field)
    for name in ("info", "read", "sample", "score", "close"):
        assert callable(getattr(pkg.DistField, name)), name


def test_new_sources_are_listed_for_every_build():
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    for src in ("kernels_clearance.hip", "dist_field.cpp"):
        assert src in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", src)), src


def test_argument_errors_need_no_device(pkg):
    """Creation: dist, origin, step or field NULL; the shape as the distance calls refuse it; a field entry or an origin that is not finite; an axis of more
    than one cell with a step that is 0 or not finite (an axis of one cell may have any step); the scene and online calls with what
    mon_scene_distance_lattice refuses and with max_dist +inf, NaN, 0 or negative.  Sample and score: every NULL, count and value the header lists -- judged
    before the handle is looked at, so a NULL handle with good arguments fails on the handle alone.  MON_ERR_ARG with a message, every output and *field
    untouched, whether or not a device is present."""
    L = pkg.lib()
    SENT = 0x5a5a5a50
    field = C.c_void_p(SENT)
    d = np.linspace(0.0, 3.0, 24).astype(F); o3 = np.array([0.5, -1.0, 2.0], F); s3 = np.array([0.25, -0.5, 0.125], F)

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def mk(dist=d, shape=(2, 3, 4), o=o3, s=s3, f=field, device=0):
        return L.mon_dist_field_create(device, _p(dist), *shape, _p(o), _p(s), C.byref(f) if f is not None else None)

    wrap = ((1 << 30, 1 << 30, 1 << 30), (1 << 22, 1 << 21, 1 << 21), (2147483647, 2147483647, 2147483647), (1, 1 << 22, 2), (1 << 16, 1 << 16, 1 << 16))
    refused = (dict(dist=None), dict(o=None), dict(s=None), dict(f=None), dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)),
               dict(shape=(-1, 3, 4)), dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)), dict(dist=ed(d, 7, np.nan)), dict(dist=ed(d, 23, np.inf)),
               dict(dist=ed(d, 0, -np.inf)), dict(o=ed(o3, 0, np.nan)), dict(o=ed(o3, 2, np.inf)), dict(s=ed(s3, 0, 0.0)), dict(s=ed(s3, 1, -0.0)),
               dict(s=ed(s3, 2, np.nan)), dict(s=ed(s3, 1, np.inf)), dict(shape=(24, 1, 1), s=ed(s3, 0, 0.0))) + tuple(dict(shape=w) for w in wrap)
    for kw in refused:
        assert mk(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    for kw, word in ((dict(dist=None), b"dist"), (dict(f=None), b"field"), (dict(dist=ed(d, 7, np.nan)), b"dist[7]"), (dict(s=ed(s3, 0, 0.0)), b"axis 0"),
                     (dict(s=ed(s3, 2, np.nan)), b"axis 2"), (dict(o=ed(o3, 0, np.nan)), b"origin"), (dict(shape=(1 << 11, 1 << 11, 2)), b"points")):
        assert mk(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    if pkg.device_count() == 0:                                                    # accepted by the checks; then no device
        for kw in (dict(), dict(shape=(24, 1, 1), s=ed(ed(s3, 1, 0.0), 2, np.nan)), dict(shape=(1, 1, 24), s=ed(ed(s3, 0, np.inf), 1, 0.0)), dict(shape=(1, 1, 1), dist=d[:1])):
            assert mk(**kw) == MON_ERR_NO_DEVICE and L.mon_last_error(), kw
    assert field.value == SENT

    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), smin=1.0, mx=2.0, f=field):
        return L.mon_scene_dist_field(objs, n_objs, side, _p(o), _p(s), *shape, smin, mx, C.byref(f) if f is not None else None)

    def onl(o=o3, s=s3, shape=(2, 3, 4), smin=1.0, mx=2.0, f=field):
        return L.mon_online_dist_field(None, _p(o), _p(s), *shape, smin, mx, C.byref(f) if f is not None else None)

    accepted = (dict(), dict(smin=0.0), dict(mx=1e-30), dict(mx=3e38), dict(side=1), dict(shape=(1, 3, 4), s=ed(s3, 0, 0.0)))
    refused = (dict(objs=None), dict(o=None), dict(s=None), dict(f=None), dict(n_objs=0), dict(objs=many, n_objs=257), dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)),
               dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)), dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)), dict(side=2), dict(side=-1),
               dict(o=ed(o3, 0, np.nan)), dict(o=ed(o3, 2, np.inf)), dict(s=ed(s3, 1, np.nan)), dict(s=ed(s3, 0, -np.inf)), dict(s=ed(s3, 0, 0.0)),
               dict(s=ed(s3, 2, -0.0)), dict(shape=(1, 3, 4), s=ed(s3, 0, np.nan)), dict(smin=-1e-6), dict(smin=float("nan")), dict(smin=np.inf), dict(mx=0.0),
               dict(mx=-2.0), dict(mx=float("nan")), dict(mx=np.inf), dict(mx=-np.inf)) + tuple(dict(shape=w) for w in wrap)
    for kw in accepted + refused:
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw                 # (the accepted ones: a NULL element of objs)
    for kw in accepted:
        assert lat(**kw) == MON_ERR_ARG and b"object" in L.mon_last_error(), kw    # accepted by the argument checks: fails on the NULL object alone
    for kw, word in ((dict(smin=-1e-6), b"sigma_min"), (dict(side=2), b"side"), (dict(objs=many, n_objs=257), b"objects"), (dict(f=None), b"field"),
                     (dict(mx=np.inf), b"max_dist"), (dict(mx=0.0), b"max_dist"), (dict(s=ed(s3, 0, 0.0)), b"axis 0")):
        assert lat(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in (dict(), dict(smin=-1.0), dict(shape=(0, 1, 1)), dict(f=None), dict(mx=np.inf), dict(mx=0.0)):
        assert onl(**kw) == MON_ERR_ARG, kw                                        # a NULL manager, with good and with bad arguments
    assert field.value == SENT

    # the calls on a handle
    xyz = np.zeros((5, 3), F); dist = np.full(5, 7.0, F); grad = np.full((5, 3), 7.0, F)
    info = pkg.DistFieldDesc(); info.nx = 77

    def smp(f=None, x=xyz, n=5, out=dist, g=grad):
        return L.mon_dist_field_sample(f, _p(x), n, -1.0, _p(out), _p(g))

    for kw, word in ((dict(x=None), b"xyz"), (dict(out=None), b"dist_out"), (dict(n=0), b"points"), (dict(n=(1 << 24) + 1), b"points"), (dict(), b"field"),
                     (dict(g=None), b"field")):
        assert smp(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    assert L.mon_dist_field_info(None, C.byref(info)) == MON_ERR_ARG and b"field" in L.mon_last_error() and info.nx == 77
    assert L.mon_dist_field_read(None, _p(dist)) == MON_ERR_ARG and b"field" in L.mon_last_error()
    assert L.mon_dist_field_destroy(None) == 0

    sph = np.array([[0, 0, 0, 0.5], [0.1, 0.2, 0.3, 0.0]], F); ways = np.zeros((3, 4, 16), F); prm = pkg.TrajScoreParams(0.0, 0.1, 0.5)
    mc = np.full(3, 7.0, F); fh = np.full(3, 7, np.int32); co = np.full(3, 7.0, F); wc = np.full((3, 4), 7.0, F); wg = np.full((3, 4, 3), 7.0, F)
    big = np.zeros((33, 4), F)

    def sc(f=None, b=sph, nb=2, w=ways, wf=3, nt=3, nw=4, ns=2, p=prm, m=mc, rest=(fh, co, wc, wg)):
        return L.mon_dist_field_score(f, _p(b), nb, _p(w), wf, nt, nw, ns, C.byref(p) if p is not None else None, _p(m), *[_p(a) for a in rest])

    P = pkg.TrajScoreParams
    refused = ((dict(b=None), b"spheres"), (dict(w=None), b"ways"), (dict(p=None), b"params"), (dict(m=None), b"min_clear"), (dict(nb=0), b"spheres"),
               (dict(b=big, nb=33), b"spheres"), (dict(wf=0), b"way_floats"), (dict(wf=4), b"way_floats"), (dict(wf=12), b"way_floats"), (dict(wf=-3), b"way_floats"),
               (dict(nw=0), b"n_way"), (dict(nw=257), b"n_way"), (dict(ns=0), b"n_sub"), (dict(ns=17), b"n_sub"), (dict(nt=0), b"n_traj"), (dict(nt=65537), b"n_traj"),
               (dict(nt=65536, nw=256, ns=2), b"samples"), (dict(nt=4112, nw=256, ns=16), b"samples"), (dict(b=ed(sph, (1, 3), -1e-6)), b"sphere 1"),
               (dict(b=ed(sph, (0, 3), np.nan)), b"sphere 0"), (dict(b=ed(sph, (0, 3), np.inf)), b"sphere 0"), (dict(b=ed(sph, (1, 0), np.inf)), b"sphere 1"),
               (dict(b=ed(sph, (0, 2), np.nan)), b"sphere 0"), (dict(p=P(np.nan, 0.1, 0.5)), b"param"), (dict(p=P(0.0, np.inf, 0.5)), b"param"),
               (dict(p=P(0.0, 0.1, -np.inf)), b"param"))
    accepted = (dict(), dict(wf=16), dict(rest=(None,) * 4), dict(ns=16), dict(nw=1), dict(nt=65536, nw=256, ns=1), dict(nt=4111, nw=256, ns=16), dict(nt=65536, nw=2, ns=16), dict(b=ed(sph, (0, 3), 0.0)), dict(p=P(-5.0, -1.0, -2.0)))
    for kw, word in refused:
        assert sc(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in accepted:
        assert sc(**kw) == MON_ERR_ARG and b"field" in L.mon_last_error(), (kw, L.mon_last_error())     # good arguments: the NULL handle alone
    assert (dist == 7.0).all() and (grad == 7.0).all() and (mc == 7.0).all() and (fh == 7).all() and (co == 7.0).all() and (wc == 7.0).all() and (wg == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
STEPS = ((0.3, 0.7, 1.1), (0.25, 0.5, 0.125), (-0.3, 0.2, -0.45), (1.7e-6, 2.3e-6, 0.9e-6))      # anisotropic, powers of two, with negatives, tiny


def test_reference_is_exact_on_affine_fields():
    """D = a0 + ax i + ay j + az k with power-of-two coefficients, power-of-two steps (one negative), points at multiples of 1/8 cell: every operation of the
    rule is exact, so d equals the affine function and grad its slope in every bit -- also on the last cell (g = n - 1, i = n - 2, f = 1)."""
    rng = np.random.default_rng(11)
    nx, ny, nz = 9, 6, 5
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    D = (F(4.0) + F(0.5) * i + F(2.0) * j + F(0.25) * k).astype(F)
    o = np.array([1.0, -2.0, 0.5], F); s = np.array([0.25, -0.5, 2.0], F)
    g = np.stack([rng.integers(0, 8 * (n - 1) + 1, 10000) / 8.0 for n in (nx, ny, nz)], 1)
    g[:64] = np.array([[(nx - 1) * (m & 1), (ny - 1) * ((m >> 1) & 1), (nz - 1) * ((m >> 2) & 1)] for m in range(64)], float)     # the corners, last cells included
    p = (o + g * s).astype(F)
    assert np.array_equal(p.astype(np.float64), o + g * s.astype(np.float64))       # the points themselves are exact
    d, grad = dr.sample(D, o, s, p, outside=-1.0)
    want = (4.0 + 0.5 * g[:, 0] + 2.0 * g[:, 1] + 0.25 * g[:, 2]).astype(F)
    assert np.array_equal(_bits(d), _bits(want))
    slope = np.array([0.5 / 0.25, 2.0 / -0.5, 0.25 / 2.0], F)
    assert np.array_equal(_bits(grad), _bits(np.broadcast_to(slope, grad.shape)))
    ax, inside = dr.cell_and_fraction(D.shape, o, s, p)
    assert inside.all()
    last = g[:, 0] == nx - 1
    assert last.sum() >= 32 and (ax[0][0][last] == nx - 2).all() and (ax[0][1][last] == 1.0).all()


SHAPES = ((64, 64, 64), (17, 23, 19), (5, 4, 3), (1, 7, 9))


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_against_float64(shape):
    """Trilinear interpolation in float64 from the rule's own (i, f), on random non-negative fields.  The bound is derived: the rule's d is a convex
    combination of values in [0, max D] built by nine roundings (three per lerp, three lerps on the longest chain), each of at most 2^-24 of a value that
    stays within [0, max D] (1 + 2^-24), so |d - d64| <= 10 * 2^-24 * max D, the tenth for the second-order terms."""
    nx, ny, nz = shape
    rng = np.random.default_rng(100 + nx)
    for si, step in enumerate(STEPS):
        D = (rng.random((nz, ny, nx)) * 3.0).astype(F)
        o = np.array([0.4, -1.3, 2.2], F) * (1e-5 if si == 3 else 1.0); s = np.array(step, F)
        n = 100000 if nx == 64 else 20000
        g = rng.random((n, 3)) * (np.array([nx, ny, nz]) - 1)
        p = (o.astype(np.float64) + g * s.astype(np.float64)).astype(F)
        ax, inside = dr.cell_and_fraction(D.shape, o, s, p)
        d, _ = dr.sample(D, o, s, p, outside=-1.0)
        d64 = dr.trilinear64(D, [(np.where(inside, i, 0), f, m) for i, f, m in ax])
        assert inside.mean() > 0.95
        err = np.abs(d[inside].astype(np.float64) - d64[inside]).max()
        assert err <= 10 * U * float(D.max()), (shape, step, err / (U * float(D.max())))


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_against_scipy(shape):
    """scipy.ndimage.map_coordinates(order=1) in float64 at the exact coordinates (p - o) / s, for the points the rule calls inside.  Beside the 10 * 2^-24 *
    max D above, the rule's coordinate differs from the exact one: g = fl(fl(p - o) / s) carries two roundings, |g - g_exact| <= 2.01 * 2^-24 * (n_a - 1)
    (f = fl(g - i) is exact: g and i are within a factor of two of each other, or i = 0).  The interpolant is continuous and piecewise linear along an axis
    with a slope per cell of at most L_a, the largest difference of two cells adjacent along that axis, so the coordinates add
    sum_a L_a * 2.01 * 2^-24 * (n_a - 1); scipy's own float64 arithmetic adds less than 1e-12 * max D.  mode='nearest': an exact coordinate a rounding
    outside the lattice is clamped to the edge, which moves it towards the rule's."""
    ndi = pytest.importorskip("scipy.ndimage")
    nx, ny, nz = shape
    rng = np.random.default_rng(200 + nx)
    for si, step in enumerate(STEPS):
        D = (rng.random((nz, ny, nx)) * 3.0).astype(F)
        o = np.array([0.4, -1.3, 2.2], F) * (1e-5 if si == 3 else 1.0); s = np.array(step, F)
        g = rng.random((20000, 3)) * (np.array([nx, ny, nz]) - 1)
        p = (o.astype(np.float64) + g * s.astype(np.float64)).astype(F)
        _, inside = dr.cell_and_fraction(D.shape, o, s, p)
        d, _ = dr.sample(D, o, s, p, outside=-1.0)
        ge = (p.astype(np.float64) - o.astype(np.float64)) / s.astype(np.float64)
        ge[:, [n == 1 for n in (nx, ny, nz)]] = 0.0
        want = ndi.map_coordinates(D.astype(np.float64), [ge[:, 2], ge[:, 1], ge[:, 0]], order=1, mode="nearest")
        D64 = D.astype(np.float64)
        lip = [np.abs(np.diff(D64, axis=a)).max() if D64.shape[a] > 1 else 0.0 for a in (2, 1, 0)]
        bound = 10 * U * D64.max() + sum(l * 2.01 * U * (n - 1) for l, n in zip(lip, (nx, ny, nz))) + 1e-12 * D64.max()
        err = np.abs(d[inside].astype(np.float64) - want[inside]).max()
        assert err <= bound, (shape, step, err, bound)


def _tree(v):
    """a plain recursive pairwise sum over a power-of-two list"""
    return v[0] if len(v) == 1 else F(_tree(v[:len(v) // 2]) + _tree(v[len(v) // 2:]))


def test_cost_tree_is_a_pairwise_sum():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 63, 64, 65, 255, 257, 4081):
        pen = (rng.random((3, n)) * 2.0).astype(F)
        got = dr.pairwise_tree(pen)
        P = 1 << max(0, (n - 1).bit_length())
        for t in range(3):
            assert got[t] == _tree(list(pen[t]) + [F(0)] * (P - n)), n
        dy = (rng.integers(0, 64, (3, n)) / 8.0).astype(F)                          # dyadic penalties: every partial sum is exact
        assert [float(x) for x in dr.pairwise_tree(dy)] == [math.fsum(map(float, r)) for r in dy]


def _wall(nx=33, ny=5, nz=4, x0=16, step=0.25):
    """dist = |x - x0| on a lattice with origin 0: a wall at the plane i = x0"""
    D = np.broadcast_to(np.abs(np.arange(nx) - x0).astype(F) * F(step), (nz, ny, nx)).copy()
    return D, np.zeros(3, F), np.array([step, step, step], F)


def test_score_on_a_wall_field():
    """A straight trajectory along x through a wall, one sphere of radius 0.5 at the body's origin, step 0.25, waypoints a cell apart, n_sub 2: every number
    is exact.  clear(q) = |x_q - 4| - 0.5; the first sample with clear <= margin is known; min_clear is -0.5 at the wall; way_clear is clear at the
    waypoints and way_grad the wall's normal -1 / +1 (0 on the wall's own cell boundary side rule: the cell to the right of x0 has slope +1)."""
    D, o, s = _wall()
    n_way = 33; x = (np.arange(n_way) * 0.25).astype(F)
    ways = np.zeros((1, n_way, 3), F); ways[0, :, 0] = x; ways[0, :, 1] = 0.5; ways[0, :, 2] = 0.25
    sph = np.array([[0, 0, 0, 0.5]], F)
    r = dr.score(D, o, s, sph, ways, 2, outside=9.0, margin=0.25, safe=1.0)
    xq = np.arange(65) * 0.125
    clear = np.abs(xq - 4.0) - 0.5
    assert r["min_clear"][0] == F(-0.5)
    assert r["first_hit"][0] == int(np.flatnonzero(clear <= 0.25)[0]) == 26        # x = 3.25: clear = 0.25 == margin counts as a hit
    assert np.array_equal(r["way_clear"][0], clear[::2].astype(F))
    pen = np.maximum(0.0, 1.0 - clear) ** 2
    assert float(r["cost"][0]) == math.fsum(pen)                                    # dyadic: the tree is exact
    gx = r["way_grad"][0, :, 0]
    assert (gx[:16] == -1.0).all() and (gx[16:32] == 1.0).all() and gx[32] == 1.0 and (r["way_grad"][0, :, 1:] == 0).all()
    # a margin just below that clearance moves the first hit on by one sample
    assert dr.score(D, o, s, sph, ways, 2, outside=9.0, margin=np.nextafter(F(0.25), F(0)), safe=1.0)["first_hit"][0] == 27
    assert dr.score(D, o, s, sph, ways, 2, outside=9.0, margin=-1.0, safe=1.0)["first_hit"][0] == -1


def test_score_edge_cases():
    """n_way = 1 (one sample, whatever n_sub); points outside take `outside` and a zero gradient; NaN and inf waypoints are outside; an axis of one cell is
    ignored; ties in the sphere that attains way_clear go to the lowest k."""
    D, o, s = _wall()
    sph = np.array([[0, 0, 0, 0.5], [0.25, 0, 0, 0.25]], F)
    one = dr.score(D, o, s, sph, np.array([[[1.0, 0.5, 0.25]]], F), 7, outside=9.0, margin=0.0, safe=0.0)
    assert one["min_clear"][0] == F(2.5) and one["first_hit"][0] == -1 and one["cost"][0] == 0 and one["way_clear"].shape == (1, 1)
    assert one["way_grad"][0, 0].tolist() == [-1.0, 0.0, 0.0]                       # both spheres have clear 2.5: the gradient is sphere 0's
    bad = np.array([[[np.nan, 0.5, 0.25], [1.0, 0.5, 0.25]], [[1.0, np.inf, 0.25], [1.0, 0.5, 0.25]], [[-0.125, 0.5, 0.25], [9.0, 0.5, 0.25]]], F)
    r = dr.score(D, o, s, sph[:1], bad, 1, outside=7.0, margin=0.0, safe=0.0)
    assert (r["way_clear"][:, 0] == F(6.5)).all() and (r["way_grad"][:, 0] == 0).all() and (r["way_clear"][:2, 1] == F(2.5)).all()
    assert r["way_clear"][2, 1] == F(6.5) and (r["min_clear"] == F([2.5, 2.5, 6.5])).all()
    d, g = dr.sample(D, o, s, np.array([[np.nan, 0, 0], [0, -1e-9, 0], [8.0 + 1e-6, 0, 0], [8.0, 1.0, 0.75], [1e30, 0, 0]], F), outside=-3.0)
    assert d.tolist() == [-3.0, -3.0, -3.0, 4.0, -3.0] and (g[[0, 1, 2, 4]] == 0).all() and g[3].tolist() == [1.0, 0.0, 0.0]
    # an axis of one cell: any coordinate, any step, no gradient
    D1 = D[:1, :1, :].copy()
    d1, g1 = dr.sample(D1, o, np.array([0.25, 0.0, np.nan], F), np.array([[1.0, 1e30, -5.0], [1.0, np.nan, np.inf]], F), outside=-3.0)
    assert d1.tolist() == [3.0, 3.0] and g1.tolist() == [[-1.0, 0.0, 0.0]] * 2
