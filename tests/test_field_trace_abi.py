"""CPU-side checks (no device needed) of the ray-tracing boundary (include/mon_core.h): mon_trace_default, mon_dist_field_trace and
mon_dist_field_beam_score are declared, exported and bound with the header's signatures; the new source is listed for every build; every argument error is
MON_ERR_ARG before any device work, with a message and the outputs untouched, the handle judged last; and the reference the GPU tests compare with
(tests/field_trace_reference.py) is pinned on its own: by a closed form on D = z, against the same loop in float64 with a derived bound, and against exact ray
intersections with the analytic scene; the beam score by its exact rules.  (The rows that need a device are in tests/test_field_trace.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, p as _p
import dist_field_reference as dr
import field_trace_reference as ft
import scan_match_reference as sm

NEW = ("mon_trace_default", "mon_dist_field_trace", "mon_dist_field_beam_score")
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
    assert [_kind(a) for a in _decl("mon_trace_default")] == ["ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_dist_field_trace")] == ["ptr", "ptr", "u64", "ptr", "u64"] + ["ptr"] * 5
    assert [_kind(a) for a in _decl("mon_dist_field_beam_score")] == ["ptr", "ptr", "u64", "ptr", "ptr", "u64"] + ["ptr"] * 5
    assert C.sizeof(pkg.TraceParams) == 28 and C.sizeof(pkg.BeamParams) == 4
    assert [f for f, _ in pkg.TraceParams._fields_] == list(ft.FIELDS)
    for name in ("trace_default", "trace", "beam_score", "line_of_sight"):
        assert callable(getattr(pkg.DistField, name)), name


def test_new_source_is_listed_for_every_build():
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_field_trace.hip" in txt
    body = open(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_field_trace.hip")).read()
    # the sample is the shared header's and the fold is kernels_scan_match.hip's: neither is copied
    assert '#include "field_sample_device.h"' in body and "bool fd_sample(" not in body and "void k_scan_fold(" not in body and "launch_scan_fold(" in body


def _pose(seed, t=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    T = np.eye(4); T[:3, :3] = dr.rotation(rng.normal(size=3), rng.uniform(-3.0, 3.0)); T[:3, 3] = t
    T[3] = rng.normal(size=4)                                                       # junk, which the rule ignores
    return T.astype(F)


def test_argument_errors_need_no_device(pkg):
    """Every NULL, count and value the header lists, for both calls -- judged before the handle is looked at, so a NULL handle with good arguments fails on
    the handle alone.  MON_ERR_ARG with a message, every output untouched, whether or not a device is present."""
    L = pkg.lib()
    TP, BP = pkg.TraceParams, pkg.BeamParams
    rays = np.zeros((5, 6), F); rays[:, 5] = 1.0
    poses = np.stack([_pose(1), _pose(2)]).reshape(2, 16)
    many = np.tile(poses[:1], (4097, 1))
    good = dict(t_min=0.0, t_max=3.0, eps=0.01, step_min=0.02, relax=0.5, step_outside=0.05, max_steps=64)
    rng_o = np.full((2, 5), 7.0, F); st = np.full((2, 5), 7, np.int32); sp = np.full((2, 5), 7, np.int32); nrm = np.full((2, 5, 3), 7.0, F)

    def tp(**kw):
        return TP(**dict(good, **kw))

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def tr(f=None, r=rays, n=5, T=poses, H=2, p=tp(), ro=rng_o, rest=(st, sp, nrm)):
        return L.mon_dist_field_trace(f, _p(r), n, _p(T), H, C.byref(p) if p is not None else None, _p(ro), *[_p(a) for a in rest])

    bad_params = ((dict(t_min=np.nan), b"not finite"), (dict(t_max=np.inf), b"not finite"), (dict(eps=np.nan), b"not finite"),
                  (dict(eps=-np.inf), b"not finite"),
                  (dict(step_min=np.inf), b"not finite"), (dict(relax=np.nan), b"not finite"), (dict(step_outside=np.inf), b"not finite"),
                  (dict(t_min=3.5), b"t_min"), (dict(step_min=0.0), b"step_min"), (dict(step_min=-0.1), b"step_min"), (dict(step_outside=0.0), b"step_outside"),
                  (dict(step_outside=-1.0), b"step_outside"), (dict(relax=0.0), b"relax"), (dict(relax=-0.5), b"relax"), (dict(relax=1.0001), b"relax"),
                  (dict(max_steps=0), b"max_steps"), (dict(max_steps=-3), b"max_steps"), (dict(max_steps=4097), b"max_steps"))
    refused = [(dict(r=None), b"rays"), (dict(p=None), b"params"), (dict(ro=None), b"range"), (dict(n=0), b"rays"), (dict(n=(1 << 20) + 1), b"rays"),
               (dict(H=0), b"poses"), (dict(T=many, H=4097, n=1), b"poses"), (dict(T=many, H=4096, n=(1 << 10) + 1), b"pairs"),
               (dict(T=many, H=5, n=1 << 20), b"pairs"), (dict(T=None, H=2), b"poses16"), (dict(T=None, H=0), b"poses"),
               (dict(T=ed(poses, (1, 0), np.nan)), b"pose 1"), (dict(T=ed(poses, (0, 11), np.inf)), b"pose 0"), (dict(T=ed(poses, (1, 7), -np.inf)), b"pose 1")]
    refused += [(dict(p=tp(**kw)), word) for kw, word in bad_params]
    accepted = (dict(), dict(T=None, H=1), dict(rest=(None, None, None)), dict(rest=(st, None, None)), dict(rest=(None, sp, None)),
                dict(rest=(None, None, nrm)),
                dict(T=ed(poses, (1, 13), np.nan)), dict(T=many, H=4096, n=1 << 10), dict(T=many, H=4, n=1 << 20), dict(n=1, H=1),
                dict(r=ed(rays, (0, 0), np.nan)), dict(p=tp(t_min=3.0)), dict(p=tp(relax=1.0)), dict(p=tp(max_steps=1)), dict(p=tp(max_steps=4096)),
                dict(p=tp(eps=-5.0)), dict(p=tp(t_min=-2.0)))
    for kw, word in refused:
        assert tr(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in accepted:
        assert tr(**kw) == MON_ERR_ARG and b"field" in L.mon_last_error(), (kw, L.mon_last_error())       # good arguments: the NULL handle alone
    assert (rng_o == 7.0).all() and (st == 7).all() and (sp == 7).all() and (nrm == 7.0).all()

    z = np.ones(5, F); cost = np.full(2, 7.0, F); nv = np.full(2, 7, np.int32); nh = np.full(2, 7, np.int32)

    def bs(f=None, r=rays, n=5, m=z, T=poses, H=2, p=tp(), b=BP(0.5), co=cost, rest=(nv, nh)):
        return L.mon_dist_field_beam_score(f, _p(r), n, _p(m), _p(T), H, C.byref(p) if p is not None else None, C.byref(b) if b is not None else None, _p(co),
                                           *[_p(a) for a in rest])

    refused = [(dict(r=None), b"rays"), (dict(m=None), b"measured"), (dict(p=None), b"params"), (dict(b=None), b"beam"), (dict(co=None), b"cost"),
               (dict(n=0), b"rays"), (dict(n=(1 << 20) + 1), b"rays"), (dict(H=0), b"poses"), (dict(T=many, H=4097, n=1), b"poses"),
               (dict(T=many, H=4096, n=(1 << 12) + 1), b"pairs"), (dict(T=many, H=17, n=1 << 20), b"pairs"), (dict(T=None, H=2), b"poses16"),
               (dict(T=ed(poses, (1, 3), np.nan)), b"pose 1"), (dict(b=BP(0.0)), b"huber"), (dict(b=BP(-1.0)), b"huber"), (dict(b=BP(np.nan)), b"huber"),
               (dict(b=BP(-np.inf)), b"huber")]
    refused += [(dict(p=tp(**kw)), word) for kw, word in bad_params]
    accepted = (dict(), dict(T=None, H=1), dict(rest=(None, None)), dict(rest=(nv, None)), dict(b=BP(np.inf)), dict(b=BP(1e-30)), dict(m=ed(z, 2, np.nan)),
                dict(T=many, H=4096, n=1 << 12), dict(T=many, H=16, n=1 << 20), dict(T=ed(poses, (0, 15), np.inf)))
    for kw, word in refused:
        assert bs(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in accepted:
        assert bs(**kw) == MON_ERR_ARG and b"field" in L.mon_last_error(), (kw, L.mon_last_error())
    assert (cost == 7.0).all() and (nv == 7).all() and (nh == 7).all()

    prm = tp(eps=123.0)
    assert L.mon_trace_default(None, C.byref(prm)) == MON_ERR_ARG and b"field" in L.mon_last_error() and prm.eps == 123.0
    assert L.mon_trace_default(None, None) == MON_ERR_ARG and L.mon_last_error()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
def _plane():
    """D = z on 9^3 cells of 1/2 from (-2, -2, 0): dyadic values, which trilinear interpolation reproduces exactly"""
    o = np.array([-2.0, -2.0, 0.0], F); s = np.full(3, 0.5, F)
    return np.broadcast_to((np.arange(9) * 0.5).astype(F)[:, None, None], (9, 9, 9)).copy(), o, s


PLANE_PRM = dict(t_min=F(0), t_max=F(8), eps=F(3 * 2.0 ** -6), step_min=F(2.0 ** -7), relax=F(0.5), step_outside=F(0.5), max_steps=64)


def test_default_parameters():
    p = ft.trace_default((16, 20, 24), np.full(3, 0.1, F))
    c = F(0.1); e = [F(23) * c, F(19) * c, F(15) * c]
    assert p["t_max"] == np.sqrt(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2])) and p["t_min"] == 0 and p["max_steps"] == 256
    assert (p["eps"], p["step_min"], p["relax"], p["step_outside"]) == (c / F(8), c / F(4), F(0.5), c / F(2))
    q = ft.trace_default((1, 8, 9), np.array([0.25, -0.125, 7.0], F))               # the smallest |step|, a negative one included; z has one cell
    assert q["eps"] == F(0.125 / 8) and q["t_max"] == np.sqrt(F(4.0 + 0.875 ** 2))
    assert ft.trace_default((1, 1, 1), np.zeros(3, F))["eps"] == F(1 / 8) and ft.trace_default((1, 1, 1), np.zeros(3, F))["t_max"] == 0


def test_closed_form_on_a_plane_field():
    """(a) D = z, relax = 1/2, a ray straight down from z0 = 2: d halves per step, so sample k is at t_k = z0 (1 - 2^-k) exactly, checked entry by entry by
    cutting the march at max_steps = 1 .. 6 (status 2, range = t_k).  With eps = 3/64 the first d <= eps is d_6 = 1/32 after d_5 = 1/16: status 0 after 7
    samples, and the crossing is t_5 + (t_6 - t_5) (1/16 - 3/64) / (1/16 - 1/32) = t_5 + 1/64, where z = eps exactly; normal = (0, 0, 1).  A ray that starts
    above the lattice steps by step_outside until it is inside; one that points up leaves through the top face (status 3, range = the last inside t)."""
    D, o, s = _plane(); z0 = 2.0
    down = np.array([[0.25, -0.5, z0, 0, 0, -1]], F)
    for j in range(1, 7):
        r = ft.trace(D, o, s, down, None, dict(PLANE_PRM, max_steps=j))
        assert (r["status"][0, 0], r["steps"][0, 0]) == (ft.OUT_OF_STEPS, j) and float(r["range"][0, 0]) == z0 * (1 - 2.0 ** -j), j
    r = ft.trace(D, o, s, down, None, PLANE_PRM, normals=True)
    assert (r["status"][0, 0], r["steps"][0, 0]) == (ft.HIT, 7)
    assert float(r["range"][0, 0]) == z0 * (1 - 2.0 ** -5) + 2.0 ** -6 and z0 - float(r["range"][0, 0]) == float(PLANE_PRM["eps"])
    assert r["normal"][0, 0].tolist() == [0.0, 0.0, 1.0]
    # the same ray as a sensor-frame ray under a pose that is a signed permutation with a dyadic translation: every operation is exact
    T = np.zeros((4, 4), F); T[:3, :3] = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]; T[:3, 3] = (0.25, -0.5, 0.5); T[3] = 9
    body = np.array([[0, 1.5, 0, 0, -1, 0]], F)                                     # o -> (0.25, -0.5, 2), u -> (0, 0, -1)
    rp = ft.trace(D, o, s, body, T.reshape(1, 16), PLANE_PRM, normals=True)
    for k in ("range", "status", "steps", "normal"):
        assert (np.asarray(rp[k]) == np.asarray(r[k])).all(), k
    # from above the lattice (z = 5): outside at t = 0 and 1/2, inside at t = 1 on the top face (d = 4), then t = 3, 4, 4.5 ..: t_k = 5 - 4 * 2^-(k - 2)
    above = np.array([[0, 0, 5.0, 0, 0, -1]], F)
    r = ft.trace(D, o, s, above, None, dict(PLANE_PRM, max_steps=5))
    assert (r["status"][0, 0], r["steps"][0, 0], float(r["range"][0, 0])) == (ft.OUT_OF_STEPS, 5, 4.5)
    # upwards from z = 2: t = 0, 1 (z = 3, d = 3), 2.5 (z = 4.5: outside): left, range = 1, no normal
    up = np.array([[0, 0, 2.0, 0, 0, 1]], F)
    r = ft.trace(D, o, s, up, None, PLANE_PRM, normals=True)
    assert (r["status"][0, 0], r["steps"][0, 0], float(r["range"][0, 0])) == (ft.LEFT, 3, 1.0) and not r["normal"].any()
    # away from the lattice from outside: step_outside until t_max: 8 / 0.5 + 1 samples, then passed
    away = np.array([[0, 0, 5.0, 0, 0, 1]], F)
    r = ft.trace(D, o, s, away, None, PLANE_PRM)
    assert (r["status"][0, 0], r["steps"][0, 0], float(r["range"][0, 0])) == (ft.PASSED, 17, 8.0)
    # t_min == t_max: one sample; the first sample hits where eps is above the field: range = t_min
    r = ft.trace(D, o, s, down, None, dict(PLANE_PRM, t_min=F(0.5), t_max=F(0.5)))
    assert (r["status"][0, 0], r["steps"][0, 0], float(r["range"][0, 0])) == (ft.PASSED, 1, 0.5)
    r = ft.trace(D, o, s, down, None, dict(PLANE_PRM, t_min=F(0.5), eps=F(9)))
    assert (r["status"][0, 0], r["steps"][0, 0], float(r["range"][0, 0])) == (ft.HIT, 1, 0.5)


def _random_field():
    """tests/test_scan_match.py's 13 x 11 x 7 field with steps of mixed sign, the field the device tests run on"""
    rng = np.random.default_rng(21)
    return (rng.random((7, 11, 13)) * 3.0 - 1.0).astype(F), np.array((0.4, 1.3, -2.2), F), np.array((0.3, -0.2, 0.45), F)


def test_reference_against_float64():
    """(b) The float32 march against the same loop in float64 (plain float64 trilinear interpolation) from the rule's own float32 a and w, on the random
    field the device tests use: 2 000 rays under 3 poses.  Where both take the same status and step count the ranges differ by at most a bound assembled
    from the case's own figures:
      * a point: two roundings per component of values of at most Q = max |a| + t_max max |w|: eq = 2 u Q; with the march's t off by E the sample is off by
        ed(E) = S E + G eq + 10 u max |D| (the sample's own error: tests/test_dist_field_abi.py), G = the sum over the axes of the field's largest one-axis
        difference over its step and S = the same sum weighted by |w_a|, which bounds the interpolant's derivative along the ray;
      * a step t <- fl(t + fmax(fl(relax d), step_min)), fmax being 1-Lipschitz: E' <= (1 + relax S) E + c, c = relax (G eq + 10 u max |D|) + u (relax
        max |D| + t_max); a step outside adds u t_max <= c.  From E = 0: E_K = c ((1 + relax S)^K - 1) / (relax S) after K = steps - 1 advances;
      * status 1 returns t_max itself (0); status 2 and a first-sample hit return t (E_K); status 3 returns t_prev (E_K);
      * a crossing t_prev + (t - t_prev) r, r = (d_prev - eps) / (d_prev - d) in (0, 1]: numerator and denominator are off by ed(E_K) + u and 2 ed(E_K) + u
        of themselves, so dr = (ed + r 2 ed) / (den - 2 ed) + 3 u (no bound where den <= 2 ed: such rays are counted with the disagreeing ones), and the
        range by E_K + (2 E_K + u t_max) (r + dr) + (t - t_prev) dr + 2 u t_max.
    The bound grows as (1 + relax S)^K: the march amplifies an error by the field's slope at every step, and a random field is steep.  It has teeth where K
    is small, which is most rays here: over half of the compared crossings have a bound below 1e-3 of t_max; the rays for which it gives nothing (no finite
    value, or a denominator within its own error) are counted and printed.  The share of rays where the two disagree on status or steps (a sample within
    rounding of eps or of a face) is printed and stays under 2 %.  Measured: 0 % disagree, 9.2 % have no bound, worst error 4.6e-5 at 0.006 of its bound."""
    field = _random_field(); D, o, s = field
    prm = ft.trace_default(D.shape, s)
    rays = ft.random_rays(field, 2000, 5); poses = ft.field_poses(field, 3, 6)
    got = ft.trace(D, o, s, rays, poses, prm); ref = ft.trace64(D, o, s, rays, poses, prm)
    r32 = got["range"].reshape(-1).astype(np.float64); r64 = ref["range"].reshape(-1)
    st = ref["status"].reshape(-1); K = np.maximum(ref["steps"].reshape(-1) - 1, 0).astype(np.float64)
    same = (got["status"].reshape(-1) == st) & (got["steps"] == ref["steps"]).reshape(-1)
    a = np.abs(ref["a"].astype(np.float64)); w = np.abs(ref["w"].astype(np.float64))
    D64 = D.astype(np.float64); s64 = np.abs(s.astype(np.float64)); t_max = float(prm["t_max"]); relax = float(prm["relax"]); Dmax = np.abs(D64).max()
    slope = np.array([np.abs(np.diff(D64, axis=2 - ax)).max() / s64[ax] for ax in range(3)])
    G = slope.sum(); S = w @ slope
    eq = 2 * U * (a.max(1) + t_max * w.max(1))
    c = relax * (G * eq + 10 * U * Dmax) + U * (relax * Dmax + t_max)
    with np.errstate(all="ignore"):
        E = c * ((1 + relax * S) ** K - 1) / (relax * S)
        edE = S * E + G * eq + 10 * U * Dmax
        last = ref["last"]; den = last["d_prev"] - last["d"]; r = (last["d_prev"] - float(prm["eps"])) / den
        dr_ = (edE + r * 2 * edE) / (den - 2 * edE) + 3 * U
        cross = E + (2 * E + U * t_max) * (r + dr_) + (last["t"] - last["t_prev"]) * dr_ + 2 * U * t_max
    crossing = (st == ft.HIT) & last["seen"]
    bound = np.where(st == ft.PASSED, 0.0, np.where(crossing, cross, E))
    loose = crossing & ~(den > 2 * edE)
    judged = same & ~loose & np.isfinite(bound)
    err = np.abs(r32 - r64)
    share = 1.0 - same.mean()
    print("float64 restatement: %d of %d rays compared; %.2f %% differ in status or steps, %.2f %% more have no bound; statuses %s; worst error / bound %.3g; "
          "median bound %.3g, worst error %.3g" % (judged.sum(), judged.size, 100 * share, 100 * (same & ~judged).mean(), np.bincount(st, minlength=4).tolist(),
                                                    (err[judged] / np.maximum(bound[judged], 1e-300)).max(), np.median(bound[judged]), err[judged].max()))
    assert (err[judged] <= bound[judged]).all(), (err[judged] / np.maximum(bound[judged], 1e-300)).max()
    assert share < 0.02, share
    assert np.median(bound[judged & crossing]) < 1e-3 * t_max                       # the bound has teeth
    assert all((st[judged] == k).sum() > 20 for k in (ft.HIT, ft.PASSED, ft.LEFT)) and (crossing & judged).sum() > 200        # and the case is not vacuous


@pytest.mark.parametrize("k", [0, 1, 2])
def test_reference_on_the_analytic_scene(k):
    """(c) The two boxes and the sphere of tests/test_scan_match.py's recovery case on 24 x 20 x 16 cells of 0.1, default parameters, 128 azimuths x 16
    elevations from three free sensor positions, against exact ray intersections: every judged ray is a hit, no ray with a cell of clearance is a hit.
    Measured on the CPU: 422, 109 and 172 judged rays, none missed, no false hit among 1 172, 1 722 and 1 662 clear rays, worst range error 0.367, 0.367
    and 0.307 cell.  The bar here and for the device is twice the worst of the three, 0.734 cell (a range error comes from the level eps = c / 8 sitting
    before the surface, divided by the incidence, and from the interpolated field's own offset from the analytic one)."""
    c = ft.analytic_case(ft.SENSORS[k])
    assert sm.sdf_scene(np.array(ft.SENSORS[k])) > 0.1
    r = ft.trace(c["D"], c["origin"], c["step"], c["rays"])
    j = c["judged"]; hit = r["status"][0] == ft.HIT
    err = np.abs(r["range"][0].astype(np.float64) - c["t"])[j & hit] / 0.1
    print("sensor %d: %d judged rays, %d missed, %d false hits among %d clear rays, worst range error %.3f cell; lane utilisation %.2f"
          % (k, j.sum(), (j & ~hit).sum(), (c["clear"] & hit).sum(), c["clear"].sum(), err.max(), ft.utilisation(r["steps"])))
    assert 100 <= j.sum() <= 440 and c["clear"].sum() >= 100
    assert not (j & ~hit).any() and not (c["clear"] & hit).any()
    assert err.max() <= ft.ANALYTIC_BAR_CELLS


# ---------------------------------------------------------------------------------------------------------------------------------- the beam score
def test_beam_score_rules():
    """measured equal to a pose's own ranges: cost +0 exactly, n_valid = n, n_hit = that pose's hits; among 17 poses -- the true one and 16 moved by up to
    0.1 rad about the sensor and up to one cell -- the lowest cost is the true pose's, with and without a Huber threshold; NaN beams are skipped: the cost is
    the tree over the others' terms with +0 in their places, and the counts leave them out; -0 does not come out"""
    D, o, s = ft.analytic_field(); G = ft.sensor_pose(); rays = ft.sensor_rays(); n = rays.shape[0]
    rng = np.random.default_rng(3); poses = [G]
    for _ in range(16):
        ax = rng.normal(size=3); v = rng.normal(size=3)
        d = np.concatenate([0.1 * rng.uniform(0.3, 1.0) * v / np.linalg.norm(v), 0.1 * rng.uniform(0.3, 1.0) * ax / np.linalg.norm(ax)])
        poses.append(sm.twist_pose(G, G[:3, 3], d).astype(F))
    order = rng.permutation(17); true = int(np.flatnonzero(order == 0)[0])
    poses = np.stack(poses)[order].reshape(17, 16)
    tr = ft.trace(D, o, s, rays, poses)
    z = tr["range"][true].copy()
    for hub in (np.inf, 0.2):
        got = ft.beam_score(D, o, s, rays, z, poses, huber=hub)
        assert _bits(got["cost"][true]) == 0 and got["n_hit"][true] == (tr["status"][true] == ft.HIT).sum() > 500 and (got["n_valid"] == n).all()
        assert int(np.argmin(got["cost"])) == true and (np.delete(got["cost"], true) > 0).all()
        assert (got["n_hit"] == (tr["status"] == ft.HIT).sum(1)).all()
    z[::7] = np.nan; z[5] = np.nan
    got = ft.beam_score(D, o, s, rays, z, poses, huber=0.2)
    keep = ~np.isnan(z)
    rho, valid = ft.beam_terms(tr["range"], np.where(keep, z, F(0)), 0.2)
    rho[:, ~keep] = 0
    assert valid.all() and (_bits(got["cost"]) == _bits(sm.tree(rho[..., None])[:, 0])).all()
    assert (got["n_valid"] == keep.sum()).all() and (got["n_hit"] == ((tr["status"] == ft.HIT) & keep[None]).sum(1)).all()
    assert _bits(got["cost"][true]) == 0
    none = ft.beam_score_of(np.zeros((2, 3), F), np.zeros((2, 3), np.int32), np.full(3, np.nan, F))
    assert (_bits(none["cost"]) == 0).all() and (none["n_valid"] == 0).all() and (none["n_hit"] == 0).all()
    # the terms themselves: below the threshold e^2, beyond it huber (2 |e| - huber), on dyadic values
    rho, _ = ft.beam_terms(np.array([[1.0, 1.0, 3.0]], F), np.array([0.75, 2.0, 1.0], F), 0.5)
    assert rho.tolist() == [[0.0625, 0.5 * (2 * 1.0 - 0.5), 0.5 * (2 * 2.0 - 0.5)]]
