"""CPU-side checks (no device needed) of the signed, sub-cell distance fields (include/mon_core.h): the five new calls are declared,
exported and bound with the header's signatures; the new source is listed for every build; every argument error is MON_ERR_ARG before any device work,
with a message and the outputs untouched; the numpy reference the GPU tests compare with (tests/signed_distance_reference.py) is pinned on its own -- its
separable form against its brute force over all (cell, crossing) pairs, and against closed forms; and on an analytic scene the field it makes is held
against the mask-made signed field dist - free_dist in field error and in registration.  (The rows that need a device are in
tests/test_signed_distance.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p
import distance_reference as dr
import scan_match_reference as sm
import signed_distance_reference as sr

NEW = ("mon_signed_distance_transform", "mon_scene_signed_distance_lattice", "mon_scene_signed_dist_field", "mon_online_signed_distance_lattice",
       "mon_online_signed_dist_field")
MON_ERR_ARG = 1
F = np.float32


def _bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [10, 17, 12, 15, 10]
    assert [_kind(a) for a in _decl(NEW[0])] == ["int", "ptr", "float", "int", "int", "int", "ptr", "float", "ptr", "ptr"]
    assert [_kind(a) for a in _decl(NEW[1])] == ["ptr", "u64", "int", "ptr", "ptr", "int", "int", "int", "float", "uint32", "float"] + ["ptr"] * 6
    assert _decl(NEW[3])[1:] == _decl(NEW[1])[3:] and _decl(NEW[4])[1:] == _decl(NEW[2])[3:]      # "the same from origin3 on"
    for name in ("signed_distance_transform", "scene_signed_distance_lattice", "scene_signed_dist_field", "edge_points"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.signed_distance_lattice) and callable(pkg.OnlineManager.signed_dist_field)
    assert pkg.MON_SIGNED_LOG == 1 and "#define MON_SIGNED_LOG 1u" in open(os.path.join(ROOT, "include", "mon_core.h")).read()


def test_new_source_is_listed_for_every_build():
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_signed_distance.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_signed_distance.hip"))


def test_argument_errors_need_no_device(pkg):
    """NULL val / step / origin / sdist / objs / element / manager / field; a dimension below 1; nx * ny * nz above 2^22; a non-finite step or origin; iso
    NaN; sigma_min negative, NaN or infinite; a flag bit other than MON_SIGNED_LOG; max_dist 0, negative or NaN (the handle constructors: not finite); side
    not 0 / 1; n_objs 0 and above 256: MON_ERR_ARG with a message and every output untouched, whether or not a device is present.  The optional outputs
    may be NULL, iso may be infinite, sigma_min may be 0 and max_dist may be +inf: the scene call then fails on the NULL object alone."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    val = np.ones(24, F); s3 = np.array([0.25, 0.0, -0.125], F); o3 = np.array([0.5, -1.0, 2.0], F); s3f = np.array([0.25, 0.5, -0.125], F)
    sd = np.full(64, 7.0, F); edge = np.full(64, 7, np.int32); own = np.full(64, 7, np.int32); sig = np.full(64, 7.0, F); vout = np.full(64, 7.0, F)
    iso = np.full(1, 7.0, F)

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def tr(v=val, iso_=0.0, shape=(2, 3, 4), s=s3, md=1.0, d=sd, e=edge):
        return L.mon_signed_distance_transform(0, _p(v), iso_, *shape, _p(s), md, _p(d), _p(e))

    wrap = ((1 << 30, 1 << 30, 1 << 30), (2147483647, 2147483647, 2147483647), (1, 1 << 22, 2))
    for kw in (dict(v=None), dict(s=None), dict(d=None), dict(iso_=float("nan")), dict(shape=(0, 3, 4)), dict(shape=(2, 3, -7)),
               dict(shape=((1 << 22) + 1, 1, 1)), dict(s=ed(s3, 0, np.nan)), dict(s=ed(s3, 1, np.inf)), dict(md=0.0), dict(md=-1.0), dict(md=float("nan")),
               dict(d=None, e=None)) + tuple(dict(shape=w) for w in wrap):
        assert tr(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert tr(v=None) == MON_ERR_ARG and b"val" in L.mon_last_error()
    assert tr(iso_=float("nan")) == MON_ERR_ARG and b"iso" in L.mon_last_error()
    assert tr(md=0.0) == MON_ERR_ARG and b"max_dist" in L.mon_last_error()

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), smin=1.0, flags=1, md=1.0, d=sd, rest=(edge, own, sig, vout, iso)):
        return L.mon_scene_signed_distance_lattice(objs, n_objs, side, _p(o), _p(s), *shape, smin, flags, md, _p(d), *[_p(a) for a in rest])

    def onl(o=o3, s=s3, shape=(2, 3, 4), smin=1.0, flags=1, md=1.0, d=sd, rest=(edge, own, sig, vout, iso)):
        return L.mon_online_signed_distance_lattice(None, _p(o), _p(s), *shape, smin, flags, md, _p(d), *[_p(a) for a in rest])

    bad = (dict(objs=None), dict(o=None), dict(s=None), dict(d=None), dict(n_objs=0), dict(objs=many, n_objs=257), dict(shape=(0, 3, 4)),
           dict(shape=(2, 3, 0)), dict(shape=((1 << 22) + 1, 1, 1)), dict(side=2), dict(side=-1), dict(o=ed(o3, 0, np.nan)), dict(s=ed(s3, 1, np.nan)),
           dict(smin=-1e-6), dict(smin=float("nan")), dict(smin=np.inf), dict(flags=2), dict(flags=3), dict(flags=0x80000000), dict(md=0.0), dict(md=-2.0),
           dict(md=float("nan"))) + tuple(dict(shape=w) for w in wrap)
    good = (dict(), dict(rest=(None,) * 5), dict(md=np.inf), dict(smin=0.0), dict(flags=0))
    for kw in good + bad:
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    for kw in good:
        assert lat(**kw) == MON_ERR_ARG and b"object" in L.mon_last_error(), kw     # accepted by the argument checks: fails on the NULL object alone
    assert lat(flags=2) == MON_ERR_ARG and b"flags" in L.mon_last_error()
    assert lat(smin=-1e-6) == MON_ERR_ARG and b"sigma_min" in L.mon_last_error()
    assert lat(md=float("nan")) == MON_ERR_ARG and b"max_dist" in L.mon_last_error()
    for kw in (dict(), dict(md=0.0), dict(flags=2), dict(shape=(0, 1, 1)), dict(d=None)):
        assert onl(**kw) == MON_ERR_ARG, kw                                          # a NULL manager, with good and with bad arguments

    h = C.c_void_p(0x7777)

    def fld(objs=nulls, n_objs=1, side=0, o=o3, s=s3f, shape=(2, 3, 4), smin=1.0, flags=1, md=1.0, out=True):
        return L.mon_scene_signed_dist_field(objs, n_objs, side, _p(o), _p(s), *shape, smin, flags, md, C.byref(h) if out else None)

    for kw in (dict(out=False), dict(md=np.inf), dict(md=0.0), dict(md=float("nan")), dict(flags=4), dict(s=s3), dict(smin=-1.0), dict(side=3),
               dict(shape=(2, 0, 4)), dict(objs=None)):
        assert fld(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert fld(md=np.inf) == MON_ERR_ARG and b"max_dist" in L.mon_last_error()
    assert fld(s=s3) == MON_ERR_ARG and b"step 0" in L.mon_last_error()
    assert fld() == MON_ERR_ARG and b"object" in L.mon_last_error()
    assert fld(shape=(2, 1, 4), s=s3) == MON_ERR_ARG and b"object" in L.mon_last_error()      # a step of 0 on an axis of one cell is fine
    assert L.mon_online_signed_dist_field(None, _p(o3), _p(s3f), 2, 3, 4, 1.0, 1, 1.0, C.byref(h)) == MON_ERR_ARG
    assert h.value == 0x7777
    assert (sd == 7.0).all() and (sig == 7.0).all() and (vout == 7.0).all() and (edge == 7).all() and (own == 7).all() and (iso == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
SHAPES = ((5, 4, 3), (7, 1, 9), (1, 1, 1), (13, 11, 7), (9, 8, 1))
STEPS = ((0.1, 0.1, 0.1), (0.1, -0.2, 0.3), (0.25, 0.5, 0.125), (0.05, 0.0, 0.05))
KINDS = ("random", "nonfinite", "sparse")


def values(shape, kind, seed):
    """(nz, ny, nx) float32: "random": normal; "nonfinite": normal with about a tenth of the cells +inf, -inf or NaN; "sparse": almost all outside (one
    cell in thirty above the level 0); "smooth": a sum of three slow waves (few crossings); "noise": normal (a crossing on most edges)"""
    nx, ny, nz = shape; rng = np.random.default_rng(seed)
    v = rng.normal(size=(nz, ny, nx)).astype(F)
    if kind == "nonfinite":
        r = rng.random(v.shape)
        v[r < 0.04] = np.inf; v[(r >= 0.04) & (r < 0.08)] = -np.inf; v[(r >= 0.08) & (r < 0.11)] = np.nan
    elif kind == "sparse":
        v = np.where(rng.random(v.shape) < 1 / 30, np.abs(v) + F(0.01), -np.abs(v) - F(0.01)).astype(F)
    elif kind == "smooth":
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        v = (np.sin(0.11 * i + 0.3) + np.sin(0.13 * j + 1.1) + np.sin(0.07 * k + 2.0) + 0.05 * v - 1.3).astype(F)
    return v


@pytest.mark.parametrize("step", STEPS)
def test_reference_separable_equals_brute_force(step):
    """On 5 x 4 x 3, 7 x 1 x 9, 1 x 1 x 1, 13 x 11 x 7 and 9 x 8 x 1 with isotropic, mixed-sign, power-of-two and one-zero steps, on random values, values
    with infinities and NaN mixed in and almost-all-outside values: the separable d2 equals the brute force over all (cell, crossing) pairs bit for bit;
    the edge equals the brute force's wherever the minimiser is unique, and names a crossing edge at the minimal d2 everywhere."""
    n_unique = 0
    for shape in SHAPES:
        for ki, kind in enumerate(KINDS):
            v = values(shape, kind, 100 * ki + sum(shape))
            d2, edge = sr.separable(v, 0.0, step)
            b2, bedge, tie = sr.brute_force(v, 0.0, step)
            assert d2.dtype == np.float32 and _bits(d2, b2), (shape, kind)
            none = ~(b2 < np.inf)
            assert (edge[none] == -1).all() and (edge[~none] >= 0).all(), (shape, kind)
            assert np.array_equal(edge[~tie], bedge[~tie]), (shape, kind)
            has = [sr.crossings(v, 0.0, a)[0].reshape(-1) for a in range(3)]
            e = edge[~none].astype(np.int64)
            assert all(has[a][e[e % 3 == a] // 3].all() for a in range(3)), (shape, kind)
            n_unique += int((~tie & ~none).sum())
    assert n_unique > 500, n_unique


def test_chain_x_is_the_distance_transform_of_cell_centres():
    """Values -1 / +1 with the level midway put every x crossing at f = 0.5: chain x then equals the plain transform's passes seeded with the squares of
    the half-integer offsets, and the whole transform is symmetric under val -> -val but for the sign."""
    v = np.where(dr.random_mask((11, 9, 7), 0.3, 5) != 0, F(1), F(-1)).astype(F)
    step = (0.25, 0.5, 0.125)
    for a in range(3):
        assert (sr.crossings(v, 0.0, a)[1][sr.crossings(v, 0.0, a)[0]] == 0.5).all()
    s1, e1 = sr.transform(v, 0.0, step); s2, e2 = sr.transform(-v, 0.0, step)
    assert _bits(s1, -s2) and np.array_equal(e1, e2)


def test_closed_forms():
    f = F
    # a plane: val = x0 - x with dyadic x0 and step: |sdist| = |x - x0| exactly, the sign negative where x < x0
    nx, ny, nz = 24, 20, 16; step = (0.25, 0.25, 0.25); x0 = 1.3125
    x = (np.arange(nx, dtype=F) * f(0.25))[None, None, :] + np.zeros((nz, ny, nx), F)
    sd, edge = sr.transform(f(x0) - x, 0.0, step)
    assert _bits(sd, x - f(x0)) and (edge % 3 == 0).all() and ((edge // 3) % nx == 5).all()
    assert (sr.crossings(f(x0) - x, 0.0, 0)[1][..., 5] == 0.25).all()
    # ... and truncation at exactly a distance the field holds keeps its edge
    md = 0.4375
    cut, cedge = sr.transform(f(x0) - x, 0.0, step, md)
    at = np.abs(sd) == f(md)
    assert at.any() and (cedge[at] >= 0).all() and (np.abs(cut[at]) == f(md)).all() and (cedge[np.abs(sd) > f(md)] == -1).all()
    assert (np.abs(cut[np.abs(sd) > f(md)]) == f(md)).all() and _bits(np.sign(cut), np.sign(sd))
    # a single inside cell with dyadic neighbours: f in {0, 1/4, 1/2, 3/4, 1}; val == iso is outside, with f = 0 on the edge that leaves it upward
    v = np.full((5, 5, 5), -1, F); v[2, 2, 2] = 1
    v[2, 2, 3] = -1; v[2, 3, 2] = -3; v[3, 2, 2] = 0; v[2, 2, 1] = 0; v[2, 1, 2] = -1; v[1, 2, 2] = -3
    ins = sr.inside(v, 0.0)
    assert ins.sum() == 1 and ins[2, 2, 2]
    fx = sr.crossings(v, 0.0, 0); fy = sr.crossings(v, 0.0, 1); fz = sr.crossings(v, 0.0, 2)
    assert fx[0].sum() == 2 and fy[0].sum() == 2 and fz[0].sum() == 2
    assert (fx[1][2, 2, 2], fy[1][2, 2, 2], fz[1][2, 2, 2]) == (0.5, 0.25, 1.0)
    assert (fx[1][2, 2, 1], fy[1][2, 1, 2], fz[1][1, 2, 2]) == (0.0, 0.5, 0.75)
    sd, edge = sr.transform(v, 0.0, (1.0, 1.0, 1.0))
    c = (2 * 5 + 2) * 5 + 2
    assert sd[2, 2, 2] == -0.25 and edge[2, 2, 2] == 3 * c + 1                       # +y at 1/4 and -z at 1/4 tie: y comes first in the combine
    assert sd[2, 2, 1] == 0.0 and sd[3, 2, 2] == 0.0 and (sd[~ins] >= 0).all()       # the cells at the level lie on a crossing, outside
    # edges between infinite and NaN values: f = 0.5
    for pair in ((-np.inf, np.inf), (np.nan, -np.inf), (np.inf, -np.inf), (-np.inf, np.nan)):
        has, fr = sr.crossings(np.array(pair, F).reshape(1, 1, 2), 0.0, 0)
        assert has[0, 0, 0] and fr[0, 0, 0] == 0.5, pair
    # all inside and all outside: -max_dist and +max_dist, no edge
    for v, sign in ((np.full((3, 4, 5), 2, F), -1), (np.full((3, 4, 5), -2, F), 1), (np.full((3, 4, 5), np.nan, F), -1)):
        for md in (0.75, np.inf):
            sd, edge = sr.transform(v, 0.0, (0.1, 0.1, 0.1), md)
            assert (sd == f(sign * md)).all() and (edge == -1).all()


# ---------------------------------------------------------------------------------------------------------------- accuracy on the offset analytic lattice
ORIGIN = (0.013, 0.029, 0.041)
_CASE = {}


def analytic_case():
    """The recovery case of tests/scan_match_reference.py (its points, pose and eight starts) on a 24 x 20 x 16 lattice of cell 0.1 whose origin is moved
    off the box faces: S the analytic signed distance, val = -S / 0.02 (a log density), iso = 0; `mask_field` the mask-made dist - free_dist; `sub_field`
    the reference's sub-cell field.  Computed once."""
    if not _CASE:
        c = sm.recovery_case()
        nx, ny, nz = 24, 20, 16; cell = 0.1
        o = np.asarray(ORIGIN, F); s = np.full(3, cell, F)
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        S = sm.sdf_scene(np.stack([i, j, k], -1) * s.astype(np.float64) + o.astype(np.float64))
        val = (-S / 0.02).astype(F)
        mask = sr.inside(val, 0.0)
        step = tuple(float(x) for x in s)
        mask_field = dr.transform(mask, step)[0] - dr.transform(~mask, step)[0]
        sub_field = sr.transform(val, 0.0, step)[0]
        _CASE.update(c, origin=o, step=s, S=S, val=val, cell=cell, mask_field=mask_field, sub_field=sub_field)
    return _CASE


def field_error(D, c):
    """(rms, mean) of D - S in cells over the cells within 3 cells of the surface"""
    near = np.abs(c["S"]) <= 3 * c["cell"]
    e = (D.astype(np.float64) - c["S"])[near] / c["cell"]
    return float(np.sqrt((e * e).mean())), float(e.mean())


def registration_figures(c, run):
    """run(start) -> (pose (4, 4), status) for each of the eight starts -> (statuses, worst rotation error in rad, worst translation error in cells)"""
    st, rot, tr = [], 0.0, 0.0
    for m in range(8):
        pose, status = run(c["starts"][m])
        a, t = sm.pose_errors(pose, c["pose"], c["centroid"])
        st.append(int(status)); rot = max(rot, a); tr = max(tr, t / c["cell"])
    return st, rot, tr


def cpu_registration(D, c):
    prm = sm.register_default(D.shape, c["step"], float(D.max()))

    def run(start):
        r = sm.register(D, c["origin"], c["step"], c["points"], start, prm)
        return r["pose"], r["status"]
    key = "reg%d" % id(D)
    if key not in c:
        c[key] = registration_figures(c, run)
    return c[key]


def test_edge_points_are_where_the_distance_points(pkg):
    """binding.edge_points (host only): on the analytic case every cell's nearest crossing lies |sdist| from the cell, on a lattice edge between cells of
    different sides (the reference's edge_point), within half a cell of the analytic surface; an edge of -1 (max_dist 0.45) gives NaN."""
    c = analytic_case(); step = tuple(float(x) for x in c["step"]); nz, ny, nx = c["val"].shape
    sd, edge = sr.transform(c["val"], 0.0, step, 0.45)
    pts = pkg.edge_points(edge, c["val"], 0.0, c["origin"], c["step"])
    assert pts.shape == edge.shape + (3,)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cells = np.stack([i, j, k], -1) * c["step"].astype(np.float64) + c["origin"].astype(np.float64)
    ok = edge >= 0
    assert ok.any() and (~ok).any() and np.isnan(pts[~ok]).all() and np.isfinite(pts[ok]).all()
    assert np.abs(np.linalg.norm(pts[ok] - cells[ok], axis=-1) - np.abs(sd[ok])).max() < 1e-5
    assert np.abs(sm.sdf_scene(pts[ok])).max() < 0.5 * c["cell"]
    f_axes = [sr.crossings(c["val"], 0.0, a)[1] for a in range(3)]
    want = sr.edge_point(edge[ok].astype(np.int64), f_axes, c["val"].shape) * c["step"].astype(np.float64) + c["origin"].astype(np.float64)
    assert np.abs(pts[ok] - want).max() < 1e-12


def test_accuracy_on_the_offset_analytic_lattice():
    """Origin (0.013, 0.029, 0.041), 24 x 20 x 16, cell 0.1, val = -S / 0.02, iso = 0.  The sub-cell field's rms error within 3 cells of the surface is
    below half the mask-made field's (dist - free_dist of the same lattice); the eight starts of the recovery case, run through
    scan_match_reference.register on the sub-cell field, all end with status 0, and their worst translation error is below half the mask-made field's.
    Measured: see the printed figures (DESIGN.md 3.4c-12 records them)."""
    c = analytic_case()
    rms_sub, mean_sub = field_error(c["sub_field"], c); rms_mask, mean_mask = field_error(c["mask_field"], c)
    print("field error within 3 cells, rms / mean in cells: sub-cell %.3f / %+.3f, mask dist - free_dist %.3f / %+.3f" % (rms_sub, mean_sub, rms_mask, mean_mask))
    st_sub, rot_sub, tr_sub = cpu_registration(c["sub_field"], c)
    st_mask, rot_mask, tr_mask = cpu_registration(c["mask_field"], c)
    print("registration, worst of 8 starts, rot rad / trans cell: sub-cell %.3e / %.3f (status %s), mask %.3e / %.3f (status %s)"
          % (rot_sub, tr_sub, st_sub, rot_mask, tr_mask, st_mask))
    assert rms_sub < 0.5 * rms_mask, (rms_sub, rms_mask)
    assert st_sub == [0] * 8, st_sub
    assert tr_sub < 0.5 * tr_mask, (tr_sub, tr_mask)
