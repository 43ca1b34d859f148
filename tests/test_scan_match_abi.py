"""CPU-side checks (no device needed) of the scan-matching boundary (include/mon_core.h): mon_dist_field_match, mon_register_default and
mon_dist_field_register are declared, exported and bound with the header's signatures; the new sources are listed for every build; every argument error is
MON_ERR_ARG before any device work, with a message and the outputs untouched, the handle judged last; and the reference the GPU tests compare with
(tests/scan_match_reference.py) is pinned on its own: against a float64 evaluation of the same terms with a derived bound, against central differences of the
float64 cost, by a closed form on D = z, and on a scan that lies wholly outside.  (The rows that need a device are in tests/test_scan_match.py.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, p as _p
import dist_field_reference as dr
import scan_match_reference as sm

NEW = ("mon_dist_field_match", "mon_register_default", "mon_dist_field_register")
MON_ERR_ARG = 1
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
    assert [_kind(a) for a in _decl("mon_dist_field_match")] == ["ptr", "ptr", "u64", "ptr", "u64", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_register_default")] == ["ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_dist_field_register")] == ["ptr", "ptr", "u64", "ptr", "u64"] + ["ptr"] * 8
    assert C.sizeof(pkg.ScanMatchParams) == 8 and C.sizeof(pkg.RegisterParams) == 40
    assert [f for f, _ in pkg.RegisterParams._fields_] == ["huber", "outside", "max_evals", "lambda0", "lambda_up", "lambda_down", "lambda_max", "tol_trans",
                                                           "tol_rot", "min_inside"]
    for name in ("match", "register_default", "register"):
        assert callable(getattr(pkg.DistField, name)), name


def test_new_sources_are_listed_for_every_build():
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_scan_match.hip" in txt
    for src in ("kernels_scan_match.hip", "field_sample_device.h"):
        assert os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", src)), src
    # the sample helpers live in the shared header only, and both kernel files take them from it
    for src in ("kernels_clearance.hip", "kernels_scan_match.hip"):
        body = open(os.path.join(ROOT, "ro-map_amd", "csrc", src)).read()
        assert '#include "field_sample_device.h"' in body and "FdAxis fd_axis(" not in body and "bool fd_sample(" not in body, src


def _pose(seed, t=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    T = np.eye(4); T[:3, :3] = dr.rotation(rng.normal(size=3), rng.uniform(-3.0, 3.0)); T[:3, 3] = t
    T[3] = rng.normal(size=4)                                                       # junk, which the rule ignores
    return T.astype(F)


def test_argument_errors_need_no_device(pkg):
    """Every NULL, count and value the header lists, for both calls -- judged before the handle is looked at, so a NULL handle with good arguments fails on
    the handle alone.  MON_ERR_ARG with a message, every output untouched, whether or not a device is present."""
    L = pkg.lib()
    pts = np.zeros((5, 3), F); poses = np.stack([_pose(1), _pose(2)]).reshape(2, 16); piv = np.zeros((2, 3), F)
    cost = np.full(2, 7.0, F); ni = np.full(2, 7, np.int32); nl = np.full(2, 7, np.int32); nrm = np.full((2, 27), 7.0, F)
    MP = pkg.ScanMatchParams
    many = np.tile(poses[:1], (4097, 1))

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def mt(f=None, x=pts, n=5, T=poses, H=2, c=piv, p=MP(0.5, 3.0), co=cost, rest=(ni, nl, nrm)):
        return L.mon_dist_field_match(f, _p(x), n, _p(T), H, _p(c), C.byref(p) if p is not None else None, _p(co), *[_p(a) for a in rest])

    refused = ((dict(x=None), b"points"), (dict(T=None), b"poses16"), (dict(p=None), b"params"), (dict(co=None), b"cost"), (dict(n=0), b"points"),
               (dict(n=(1 << 20) + 1), b"points"), (dict(H=0), b"poses"), (dict(T=many, H=4097, c=None), b"poses"), (dict(T=many, H=65, c=None, n=1 << 20), b"pairs"),
               (dict(T=many, H=4096, c=None, n=(1 << 14) + 1), b"pairs"), (dict(T=ed(poses, (1, 0), np.nan)), b"pose 1"), (dict(T=ed(poses, (0, 11), np.inf)), b"pose 0"),
               (dict(T=ed(poses, (1, 7), -np.inf)), b"pose 1"), (dict(c=ed(piv, (1, 2), np.nan)), b"pivot 1"), (dict(c=ed(piv, (0, 0), np.inf)), b"pivot 0"),
               (dict(p=MP(0.0, 3.0)), b"huber"), (dict(p=MP(-1.0, 3.0)), b"huber"), (dict(p=MP(np.nan, 3.0)), b"huber"), (dict(p=MP(-np.inf, 3.0)), b"huber"),
               (dict(p=MP(0.5, np.nan)), b"outside"), (dict(p=MP(0.5, np.inf)), b"outside"), (dict(p=MP(0.5, -np.inf)), b"outside"))
    accepted = (dict(), dict(c=None), dict(rest=(None, None, None)), dict(rest=(ni, None, None)), dict(p=MP(np.inf, -3.0)), dict(p=MP(1e-30, 0.0)),
                dict(T=ed(poses, (1, 13), np.nan)), dict(T=many, H=4096, c=None, n=1 << 14), dict(T=many, H=64, c=None, n=1 << 20), dict(n=1, H=1))
    for kw, word in refused:
        assert mt(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in accepted:
        assert mt(**kw) == MON_ERR_ARG and b"field" in L.mon_last_error(), (kw, L.mon_last_error())      # good arguments: the NULL handle alone
    assert (cost == 7.0).all() and (ni == 7).all() and (nl == 7).all() and (nrm == 7.0).all()

    RP = pkg.RegisterParams
    good = dict(huber=0.2, outside=3.0, max_evals=30, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_max=1e6, tol_trans=1e-4, tol_rot=1e-4, min_inside=6)

    def rp(**kw):
        return RP(**dict(good, **kw))

    out = np.full((2, 16), 7.0, F); ev = np.full(2, 7, np.int32); st = np.full(2, 7, np.int32); best = C.c_int32(7)
    big = np.zeros(((1 << 14) + 1, 3), F)

    def rg(f=None, x=pts, n=5, T=poses, H=2, p=rp(), po=out, co=cost, rest=(ni, nl, ev, st)):
        return L.mon_dist_field_register(f, _p(x), n, _p(T), H, C.byref(p) if p is not None else None, _p(po), _p(co), *[_p(a) for a in rest], C.byref(best))

    refused = ((dict(x=None), b"points"), (dict(T=None), b"poses16_in"), (dict(p=None), b"null p"), (dict(po=None), b"poses16_out"), (dict(co=None), b"cost"),
               (dict(n=0), b"points"), (dict(n=(1 << 20) + 1), b"points"), (dict(H=0), b"poses"), (dict(T=many, H=4097), b"poses"),
               (dict(T=many, H=4096, x=big, n=(1 << 14) + 1), b"pairs"), (dict(T=ed(poses, (1, 3), np.nan)), b"pose 1"), (dict(T=ed(poses, (0, 0), np.inf)), b"pose 0"),
               (dict(p=rp(huber=0.0)), b"huber"), (dict(p=rp(huber=-2.0)), b"huber"), (dict(p=rp(huber=np.nan)), b"huber"), (dict(p=rp(outside=np.nan)), b"outside"),
               (dict(p=rp(outside=np.inf)), b"outside"), (dict(p=rp(lambda0=np.nan)), b"lambda"), (dict(p=rp(lambda0=np.inf)), b"lambda"),
               (dict(p=rp(lambda0=0.0)), b"lambda"), (dict(p=rp(lambda_max=np.inf)), b"lambda"), (dict(p=rp(lambda_max=np.nan)), b"lambda"),
               (dict(p=rp(lambda_up=np.inf)), b"lambda"), (dict(p=rp(lambda_down=np.nan)), b"lambda"), (dict(p=rp(lambda_up=1.0)), b"factors"),
               (dict(p=rp(lambda_up=0.5)), b"factors"), (dict(p=rp(lambda_down=1.0)), b"factors"), (dict(p=rp(lambda_down=-3.0)), b"factors"),
               (dict(p=rp(tol_trans=np.nan)), b"tolerance"), (dict(p=rp(tol_rot=np.inf)), b"tolerance"), (dict(p=rp(tol_rot=-1e-3)), b"tolerance"),
               (dict(p=rp(max_evals=0)), b"max_evals"), (dict(p=rp(max_evals=-4)), b"max_evals"), (dict(p=rp(min_inside=-1)), b"min_inside"))
    accepted = (dict(), dict(rest=(None,) * 4), dict(p=rp(huber=np.inf)), dict(p=rp(max_evals=1)), dict(p=rp(tol_trans=0.0, tol_rot=0.0)), dict(p=rp(min_inside=0)),
                dict(p=rp(lambda_up=1.5, lambda_down=1.0001)), dict(T=ed(poses, (0, 15), np.inf)))
    for kw, word in refused:
        assert rg(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in accepted:
        assert rg(**kw) == MON_ERR_ARG and b"field" in L.mon_last_error(), (kw, L.mon_last_error())
    assert (out == 7.0).all() and (cost == 7.0).all() and (ni == 7).all() and (nl == 7).all() and (ev == 7).all() and (st == 7).all() and best.value == 7

    prm = rp(huber=123.0)
    assert L.mon_register_default(None, C.byref(prm)) == MON_ERR_ARG and b"field" in L.mon_last_error() and prm.huber == 123.0
    assert L.mon_register_default(None, None) == MON_ERR_ARG and L.mon_last_error()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
def _random_field(seed=3, shape=(7, 11, 13), lo=-1.0, hi=2.0):
    rng = np.random.default_rng(seed)
    D = (rng.random(shape) * (hi - lo) + lo).astype(F)
    return D, np.array([0.4, -1.3, 2.2], F), np.array([0.3, -0.2, 0.45], F)


def _scan(D, o, s, pose, n, seed, frac=(0.0, 1.0), stray=0):
    """n body points whose images under `pose` are at random cells and cell fractions in `frac`; the first `stray` of them are then pushed far out"""
    rng = np.random.default_rng(seed); nz, ny, nx = D.shape
    cell = np.stack([rng.integers(0, m - 1, n) for m in (nx, ny, nz)], 1)
    g = cell + rng.uniform(frac[0], frac[1], (n, 3))
    pw = o.astype(np.float64) + g * s.astype(np.float64)
    T = pose.astype(np.float64)
    body = (pw - T[:3, 3]) @ T[:3, :3]
    body[:stray] += 1e3
    return body.astype(F)


def _tree_list(v):
    return v[0] if len(v) == 1 else F(_tree_list(v[:len(v) // 2]) + _tree_list(v[len(v) // 2:]))


def test_tree_is_the_pairwise_sum_and_returns_no_negative_zero():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 64, 65, 1000):
        T = rng.normal(size=(2, n, 3)).astype(F)
        got = sm.tree(T); P = 1 << max(0, (n - 1).bit_length())
        for h in range(2):
            for k in range(3):
                assert got[h, k] == _tree_list(list(T[h, :, k]) + [F(0)] * (P - n)), (n, h, k)
    neg = np.full((1, 4, 2), -0.0, F)
    assert _bits(sm.tree(neg)).tolist() == [[0, 0]]                                 # -0 + -0 = -0 through the tree: returned as +0


@pytest.mark.parametrize("n", [1, 5, 64, 1000])
def test_reference_against_float64_terms(n):
    """The 28 sums against the float64 sum of the same terms formed in float64 from the rule's own float32 d and J.  Derived: a term carries at most four
    roundings (w = fl(huber / m), fl(w J_i), the second product; rho: fl(2 m) is exact, then a difference and a product) and the tree adds log2 P more on
    every path from a leaf to the root, so |sum32 - exact| <= (log2 P + 4) * 2^-24 * sum |terms| per entry (the bound's own second-order terms are below one
    of the four: no term has more than three roundings that are not exact)."""
    D, o, s = _random_field()
    poses = np.stack([_pose(10 + k, t=(2.2, -2.4, 3.6)) for k in range(3)])
    pts = _scan(D, o, s, poses[0], n, 20 + n, stray=n // 8)
    piv = np.array([[2.0, -2.5, 3.5], [0, 0, 0], [3.0, -1.0, 4.0]], F)
    P = 1 << max(0, (n - 1).bit_length())
    for huber in (0.3, np.inf):
        got = sm.match(D, o, s, pts, poses, piv, huber, 1.5)
        T64 = sm.terms64(D, o, s, pts, poses, piv, huber, 1.5)
        exact = T64.sum(1); bound = (math.log2(P) + 4) * U * np.abs(T64).sum(1)
        got32 = np.concatenate([got["A"], got["b"], got["cost"][:, None]], 1).astype(np.float64)
        assert (np.abs(got32 - exact) <= bound).all(), (n, huber, (np.abs(got32 - exact) / np.maximum(bound, 1e-300)).max())
        if n >= 64:
            assert (got["n_inside"] > 0).any() and (got["n_inside"] < n).all() and (np.abs(exact[0]) > 0).all()      # not vacuous
            if huber == 0.3:
                assert (got["n_inlier"][0] > 0) and (got["n_inlier"][0] < got["n_inside"][0])


def test_reference_against_central_differences():
    """b is half the gradient of the cost in the twist: central differences of the float64 cost (plain float64 trilinear interpolation at float64 poses) at
    steps h and h / 2.  The points sit at cell fractions 0.3 .. 0.7, so no difference leaves its cell, where the interpolant is a polynomial.  The bound per
    component i, every part from the figures of the case itself:
      * the sum and the forming of the terms, as in the float64 test: (log2 P + 4) u sum |J_i d|;
      * the float32 q against the exact one: six roundings of values of at most Q = |R| |p| + |t| per component, eq = 6 u Q; the sample's own error
        10 u max |D| (tests/test_dist_field_abi.py) plus the field's slope G (the largest one-axis difference over its step) times eq per axis: ed;
      * the gradient's own error: it is the same interpolation of differences over a step: 10 u G, plus the largest mixed second difference over its two
        steps, M, times eq per axis: eg; for the rotational components |a| eg and |g| ea = G (eq + u |a|) twice each, plus three roundings: eJ;
      * these enter b_i = sum J_i d as sum (|J_i| ed + |d| eJ_i);
      * the differences themselves: their truncation error falls by four from h to h / 2, so |FD_h - FD_(h/2)| is three times that of h / 2; and their
        float64 rounding, 8 * 2^-52 * cost / h."""
    D, o, s = _random_field(seed=8, shape=(7, 8, 9))
    pose = _pose(31, t=(1.9, -2.1, 3.4)); n = 200
    pts = _scan(D, o, s, pose, n, 77, frac=(0.3, 0.7))
    T = pose.astype(np.float64)
    cen = pts.astype(np.float64).mean(0); piv = (T[:3, :3] @ cen + T[:3, 3]).astype(F)
    q, d, J, inside = sm.sample_and_jacobian(D, o, s, pts, pose.reshape(1, 16), piv.reshape(1, 3))
    assert inside.all()
    got = sm.match(D, o, s, pts, pose.reshape(1, 16), piv.reshape(1, 3))
    h = 1e-5
    fd = []
    for hh in (h, h / 2):
        g = np.zeros(6)
        for i in range(6):
            e = np.zeros(6); e[i] = hh
            g[i] = (sm.cost64(D, o, s, pts, pose, piv, e) - sm.cost64(D, o, s, pts, pose, piv, -e)) / (2 * hh)
        fd.append(g)
    want = 0.5 * fd[1]
    D64 = D.astype(np.float64); s64 = np.abs(s.astype(np.float64))
    slope = [np.abs(np.diff(D64, axis=2 - a)).max() / s64[a] for a in range(3)]
    G = max(slope)
    M = max(np.abs(np.diff(np.diff(D64, axis=2 - a), axis=2 - b)).max() / (s64[a] * s64[b]) for a in range(3) for b in range(3) if a != b)
    Q = np.abs(T[:3, :3]).sum(1).max() * np.abs(pts).max() + np.abs(T[:3, 3]).max()
    eq = 6 * U * Q
    ed = 10 * U * np.abs(D64).max() + 3 * G * eq
    eg = 10 * U * G + 3 * M * eq
    a = np.abs(q[0].astype(np.float64) - piv.astype(np.float64)); amax = a.max()
    eJ = np.array([eg] * 3 + [2 * (amax * eg + G * (eq + U * amax)) + 3 * U * amax * G] * 3)
    absJ = np.abs(J[0].astype(np.float64)); absd = np.abs(d[0].astype(np.float64))
    P = 256
    bound = ((math.log2(P) + 4) * U * (absJ * absd[:, None]).sum(0) + (absJ * ed).sum(0) + absd.sum() * eJ
             + 0.5 * np.abs(fd[0] - fd[1]) + 0.5 * 8 * 2.0 ** -52 * float(got["cost"][0]) / (h / 2))
    err = np.abs(got["b"][0].astype(np.float64) - want)
    assert (err <= bound).all(), (err / bound).max()
    # the check has teeth: a component with a wrong sign, or without the half, misses by at least |want|, which is over five times its bound
    assert (np.abs(want) > 5 * bound).all(), (want, bound)


def test_closed_form_on_a_plane_field():
    """D = z on dyadic values, which trilinear interpolation reproduces exactly; poses that are signed permutations with dyadic translations, points and
    pivots at multiples of 1/8: every operation is exact, g = (0, 0, 1), d = q_z, J = (0, 0, 1, a_y, -a_x, 0), cost = sum q_z^2, and A and b are the plain
    sums, entry by entry."""
    nx = ny = nz = 9
    o = np.full(3, -2.0, F); s = np.full(3, 0.5, F)
    D = np.broadcast_to((o[2] + np.arange(nz) * s[2]).astype(F)[:, None, None], (nz, ny, nx)).copy()
    rng = np.random.default_rng(2); n = 200
    pts = (rng.integers(-8, 9, (n, 3)) / 8.0).astype(F)
    R = [np.eye(3), np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]]), np.array([[0, 0, 1], [0, -1, 0], [1, 0, 0.0]])]
    t = [(0.5, -0.25, 0.25), (0.0, 0.5, -0.5), (-0.25, 0.25, 0.125)]
    poses = np.zeros((3, 4, 4), F)
    for k in range(3):
        poses[k, :3, :3] = R[k]; poses[k, :3, 3] = t[k]; poses[k, 3] = (9, 9, 9, 9)
    piv = np.array([[0.125, -0.5, 0.25], [0, 0, 0], [1.0, 0.375, -0.125]], F)
    got = sm.match(D, o, s, pts, poses.reshape(3, 16), piv, np.inf, 5.0)
    for k in range(3):
        q = pts.astype(np.float64) @ R[k].T + np.array(t[k]); a = q - piv[k].astype(np.float64)
        J = np.stack([0 * q[:, 0], 0 * q[:, 0], 1 + 0 * q[:, 0], a[:, 1], -a[:, 0], 0 * q[:, 0]], 1); d = q[:, 2]
        assert float(got["cost"][k]) == math.fsum(d * d) and got["n_inside"][k] == n and got["n_inlier"][k] == n
        for m, (i, j) in enumerate(sm.PAIRS):
            assert float(got["A"][k, m]) == math.fsum(J[:, i] * J[:, j]), (k, i, j)
        for i in range(6):
            assert float(got["b"][k, i]) == math.fsum(J[:, i] * d), (k, i)
    # with a Huber threshold of 1/2: w = 1/2 / |d| and rho = 1/2 (2 |d| - 1/2) beyond it; |d| is a multiple of 1/8, so rho is exact
    hub = sm.match(D, o, s, pts, poses.reshape(3, 16), piv, 0.5, 5.0)
    for k in range(3):
        d = np.abs((pts.astype(np.float64) @ R[k].T + np.array(t[k]))[:, 2])
        assert float(hub["cost"][k]) == math.fsum(np.where(d <= 0.5, d * d, 0.5 * (2 * d - 0.5))) and hub["n_inlier"][k] == int((d <= 0.5).sum()) < n


@pytest.mark.parametrize("n", [1, 6, 100])
def test_a_scan_wholly_outside(n):
    """every point outside (far away, NaN, inf): cost = n * rho(outside) through the tree, all of A and b +0, both counts 0 -- below and beyond the Huber
    threshold"""
    D, o, s = _random_field()
    pts = np.full((n, 3), 1e4, F); pts[::3, 1] = np.nan; pts[1::3, 0] = -np.inf
    poses = np.stack([_pose(4), _pose(5)]).reshape(2, 16)
    for huber, outside, rho in ((np.inf, -1.5, F(2.25)), (0.5, -1.5, F(0.5) * (F(2) * F(1.5) - F(0.5))), (2.0, 1.5, F(2.25))):
        got = sm.match(D, o, s, pts, poses, None, huber, outside)
        want = sm.tree(np.full((1, n, 1), rho, F))[0, 0]
        assert (_bits(got["cost"]) == _bits(want)).all() and (got["n_inside"] == 0).all() and (got["n_inlier"] == 0).all()
        assert (_bits(got["A"]) == 0).all() and (_bits(got["b"]) == 0).all()


def test_reference_lm_recovers_the_known_pose():
    """the committed numpy Levenberg-Marquardt on the recovery case of tests/test_scan_match.py: from each of the eight starts it ends within a tenth of a
    cell and 0.02 rad of the known pose, from 0.15 rad and a cell (a loose sanity bar: the interpolated field is not the analytic one; the figures
    themselves are printed, and are the GPU test's yardstick)"""
    case = sm.recovery_case()
    prm = sm.register_default(case["D"].shape, case["step"], float(case["D"].max()))
    worst = [0.0, 0.0]
    for T0 in case["starts"]:
        a0, c0 = sm.pose_errors(T0, case["pose"], case["centroid"])
        assert abs(a0 - 0.15) < 1e-4 and abs(c0 - 0.1) < 1e-4
        r = sm.register(case["D"], case["origin"], case["step"], case["points"], T0, prm)
        ang, cen = sm.pose_errors(r["pose"], case["pose"], case["centroid"])
        print("reference LM: status %d after %d evaluations, %.3g rad, %.3g cell" % (r["status"], r["evals"], ang, cen / 0.1))
        worst = [max(worst[0], ang), max(worst[1], cen)]
        assert r["status"] in (0, 1, 2)
    assert worst[0] < 0.02 and worst[1] < 0.01, worst
