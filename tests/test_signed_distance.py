"""GPU tests (-m gpu) of the signed, sub-cell distance fields (mon_signed_distance_transform, mon_scene_signed_distance_lattice,
mon_scene_signed_dist_field and their online counterparts; kernels k_surface_line_pass, k_signed_values and k_signed_finish in
kernels_signed_distance.hip, k_distance_pass from values).  The yardstick of the transform is tests/signed_distance_reference.py, the header's rule in
numpy fp32, itself pinned against a brute force over all (cell, crossing) pairs by tests/test_signed_distance_abi.py: the device equals it bit for bit,
in sdist and in nearest_edge, whatever the kernels prune.  The scene calls are held to public calls: sigma to mon_scene_query_lattice, the field to
mon_signed_distance_transform of the values the call brings home.  The scene, the trained objects and the manager's feed are those of
tests/test_scene_render.py."""
import os

import numpy as np
import pytest

from conftest import ROOT
import field_trace_reference as ft
import signed_distance_reference as sr
import test_scene_distance as tsd
import test_scene_render as tsr
import test_signed_distance_abi as tsa
from test_scene_render import scene, trained       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu
F = np.float32

# 1 x 1 x 1; one line along each axis; no dimension a multiple of the tile; more than one block; three lines that cross the 2 048-cell tile twice
SHAPES = ((1, 1, 1), (37, 1, 1), (1, 37, 1), (1, 1, 37), (5, 4, 3), (19, 23, 17), (33, 31, 29), (4133, 3, 2), (3, 4133, 2), (2, 3, 4133))
STEPS = ((0.013, 0.0217, 0.0091), (0.25, 0.25, 0.25), (0.1, -0.2, 0.3), (0.05, 0.0, 0.05))
KINDS = ("none", "one", "smooth", "noise", "nonfinite")
SHAPE = tsd.SHAPE

_cache = {}


def _values(shape, kind):
    nx, ny, nz = shape; seed = 7 * sum(shape) + KINDS.index(kind)
    if kind == "none":
        return np.full((nz, ny, nx), -1.5, F)
    if kind == "one":
        v = np.full((nz, ny, nx), -1.5, F); v.reshape(-1)[np.random.default_rng(seed).integers(v.size)] = 0.5
        return v
    return tsa.values(shape, "random" if kind == "noise" else kind, seed)


def _case(shape, step, kind):
    """the values of (shape, kind) and their reference (d2, edge) under `step`, computed once"""
    key = (shape, step, kind)
    if key not in _cache:
        v = _values(shape, kind)
        _cache[key] = (v,) + sr.separable(v, 0.0, step)
    return _cache[key]


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ne = got.view(np.uint32) != want.view(np.uint32)
    assert not ne.any(), (what, int(ne.sum()), got[ne][:4], want[ne][:4])


def _ordered(x):
    """fp32 values as integers whose difference counts the floats between two values, across 0 too"""
    i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


# ---------------------------------------------------------------------------------------------------------------- 1: the transform against the reference
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_transform_equals_the_reference(pkg, shape, step, kind):
    """mon_signed_distance_transform equals the numpy restatement bit for bit in sdist and nearest_edge: without a crossing, with one inside cell, on a
    smooth field with few crossings (the pruning acts), on white noise (a crossing on most edges) and on values with infinities and NaN."""
    v, d2, edge = _case(shape, step, kind)
    ins = sr.inside(v, 0.0)
    want = sr.finish(d2, edge, ins, np.inf)
    sd, near = pkg.signed_distance_transform(v, 0.0, step)
    _same(sd, want[0], ("sdist", shape, step, kind)); _same(near, want[1], ("nearest_edge", shape, step, kind))
    if kind == "none":
        assert (sd == np.inf).all() and (near == -1).all()
    if kind == "one" and v.size > 1:
        assert ins.sum() == 1 and (near >= 0).all() and np.signbit(sd[ins]).all()      # (-0 on a line whose step is 0)
    if kind == "smooth" and v.size > 1000:
        n_cross = sum(int(sr.crossings(v, 0.0, a)[0].sum()) for a in range(3))
        assert 0 < n_cross < 3 * v.size // 8, n_cross


# ---------------------------------------------------------------------------------------------------------------- 2: truncation, NULL, determinism
@pytest.mark.parametrize("shape,step,kind", [((19, 23, 17), STEPS[0], "smooth"), ((33, 31, 29), STEPS[1], "one"), ((4133, 3, 2), STEPS[2], "one")])
def test_truncation(pkg, shape, step, kind):
    """max_dist below one step, equal to a distance the field holds, and large: each equals the untruncated result cut by the header's rule, bit for bit,
    and the reference's finish; the cells at exactly max_dist keep their edges; nearest_edge NULL leaves sdist as it is."""
    v, d2, edge = _case(shape, step, kind); ins = sr.inside(v, 0.0)
    full, near = pkg.signed_distance_transform(v, 0.0, step)
    mag = np.abs(full); pos = np.unique(mag[mag > 0])
    occurs = float(pos[len(pos) // 2]); below = 0.25 * min(abs(s) for s in step if s != 0)
    for md in (below, occurs, 1e30, np.inf):
        sd, nr = pkg.signed_distance_transform(v, 0.0, step, max_dist=md)
        cut = ~(mag <= F(md))
        _same(sd, np.where(cut, np.where(ins, -F(md), F(md)), full), ("sdist", md)); _same(nr, np.where(cut, np.int32(-1), near), ("nearest_edge", md))
        want = sr.finish(d2, edge, ins, md)
        _same(sd, want[0], ("reference sdist", md)); _same(nr, want[1], ("reference edge", md))
    sd, nr = pkg.signed_distance_transform(v, 0.0, step, max_dist=occurs)
    at = mag == F(occurs)
    assert at.any() and (nr[at] >= 0).all() and (np.abs(sd[at]) == F(occurs)).all() and (mag > F(occurs)).any()
    only = pkg.signed_distance_transform(v, 0.0, step, max_dist=occurs, nearest=False)
    assert only[1] is None
    _same(only[0], sd, "nearest_edge NULL")


def test_determinism_and_prefix(pkg):
    """Two calls give equal bits; nothing is written behind the lattice; another level moves the surface as the reference says"""
    import ctypes as C
    L = pkg.lib(); shape = (33, 31, 29); step = STEPS[0]; nx, ny, nz = shape
    v, d2, edge = _case(shape, step, "noise")
    a = pkg.signed_distance_transform(v, 0.0, step); b = pkg.signed_distance_transform(v, 0.0, step)
    _same(a[0], b[0], "sdist twice"); _same(a[1], b[1], "edge twice")
    sd = np.empty(v.size + 64, F); nr = np.empty(v.size + 64, np.int32); sd[v.size:] = 7.0; nr[v.size:] = 7
    s = np.asarray(step, F); vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.mon_signed_distance_transform(0, vp(v), 0.0, nx, ny, nz, vp(s), float("inf"), vp(sd), vp(nr)) == 0
    _same(sd[:v.size].reshape(v.shape), a[0], "prefix sdist"); _same(nr[:v.size].reshape(v.shape), a[1], "prefix edge")
    assert (sd[v.size:] == 7.0).all() and (nr[v.size:] == 7).all()
    want = sr.transform(v, 0.37, step, 0.05)
    got = pkg.signed_distance_transform(v, 0.37, step, max_dist=0.05)
    _same(got[0], want[0], "iso 0.37 sdist"); _same(got[1], want[1], "iso 0.37 edge")


# ---------------------------------------------------------------------------------------------------------------- 3: the scene and online calls
def _check_scene(pkg, call, query, step, what):
    """`call(sigma_min, max_dist, log)` = the signed call, `query()` = the lattice query over the same objects: the properties of the scene call"""
    nx, ny, nz = SHAPE; n = nx * ny * nz
    sigma, _, owner, _, _ = query()
    smin = tsd._sigma_min(sigma)
    ins = ~(sigma <= F(smin)); n_in = int(ins.sum())
    print("%s: sigma_min %.5g, %d of %d cells inside" % (what, smin, n_in, n))
    assert n_in >= n // 100 + 1 and n - n_in >= n // 100 + 1, (n_in, n)
    stride = np.array([1, nx, nx * ny])
    for log in (False, True):
        for md in (np.inf, 0.35):
            sd, edge, eown, sig, val, iso = call(smin, md, log)
            _same(sig, sigma, (what, "sigma", log, md))
            assert np.array_equal(np.signbit(sd), ins), (what, "sign", log, md)
            if log:
                # The device logf against float64 log(sigma).  The bound: 2 ulp, the "maximum ULP difference" the ROCm documentation lists for logf
                # (HIP math API reference, single precision mathematical functions), plus one ulp for the rounding of the float64 value to fp32.
                # Measured on MI355X over these lattices: worst 2 ulp against the rounded float64 value.
                with np.errstate(all="ignore"):
                    ref = np.log(sigma.astype(np.float64)).astype(F); riso = F(np.log(np.float64(F(smin))))
                fin = np.isfinite(ref)
                _same(val[~fin], ref[~fin], (what, "log of 0, inf or NaN passes through"))
                ulp = np.abs(_ordered(val[fin]) - _ordered(ref[fin]))
                print("%s: logf against float64, worst %d ulp over %d finite values" % (what, int(ulp.max()), int(fin.sum())))
                assert ulp.max() <= 3, int(ulp.max())
                assert abs(int(_ordered(F(iso)).reshape(-1)[0]) - int(_ordered(riso).reshape(-1)[0])) <= 3 if np.isfinite(riso) else F(iso) == riso
            else:
                _same(val, sigma, (what, "val is sigma")); assert F(iso) == F(smin)
            assert np.array_equal(sr.inside(val, iso), ins), (what, "the side read from val is the side read from sigma", log)
            wd, we = pkg.signed_distance_transform(val.reshape(nz, ny, nx), iso, step, max_dist=md)
            _same(sd, wd.reshape(-1), (what, "sdist", log, md)); _same(edge, we.reshape(-1), (what, "nearest_edge", log, md))
            ok = edge >= 0; q = np.maximum(edge, 0) // 3; other = np.minimum(q + stride[np.maximum(edge, 0) % 3], n - 1)
            assert (ins[q] != ins[other])[ok].all()
            assert np.array_equal(eown, np.where(ok, owner[np.where(ins[q], q, other)], -1)), (what, "nearest_owner", log, md)
            if md == np.inf:
                assert ok.all()
    return smin


@pytest.mark.parametrize("side", [0, 1])
def test_scene_call(pkg, scene, trained, side):
    """On a 24 x 20 x 18 lattice around the three objects, sides 0 and 1, with and without MON_SIGNED_LOG, untruncated and with max_dist 0.35: sigma equals
    mon_scene_query_lattice's bits; sign(sdist) is the mask !(sigma <= sigma_min); sdist and nearest_edge equal mon_signed_distance_transform of the
    returned val and iso; nearest_owner == owner[the inside end of the edge]; the log values are held to float64; with every optional output NULL sdist
    has the same bits."""
    import ctypes as C
    L = pkg.lib(); _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = tsd._enclosing(scene, SHAPE)
    smin = _check_scene(pkg, lambda smin, md, log: pkg.scene_signed_distance_lattice(lst, origin, step, SHAPE, smin, md, side=side, log=log),
                        lambda: pkg.query_scene_lattice(lst, origin, step, SHAPE, side), step, "side %d" % side)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]; d = np.empty(n, F); hs = (C.c_void_p * 3)(*[o.h for o in lst])
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.mon_scene_signed_distance_lattice(hs, 3, side, vp(origin), vp(step), *SHAPE, smin, 1, float("inf"), vp(d), None, None, None, None, None) == 0
    _same(d, pkg.scene_signed_distance_lattice(lst, origin, step, SHAPE, smin, side=side)[0], "sdist with every optional output NULL")
    # sigma_min = 0: the level logf(0) = -inf; every cell inside a box with a density is inside, the crossings at the box faces sit at f = 0.5
    sd0, e0, _, sig0, val0, iso0 = pkg.scene_signed_distance_lattice(lst, origin, step, SHAPE, 0.0, side=side)
    assert iso0 == -np.inf and np.array_equal(np.signbit(sd0), ~(sig0 <= 0))
    w0 = pkg.signed_distance_transform(val0.reshape(SHAPE[::-1]), iso0, step)
    _same(sd0, w0[0].reshape(-1), "sigma_min 0: sdist"); _same(e0, w0[1].reshape(-1), "sigma_min 0: edge")


def test_online_call(pkg, ss, scene, trained):
    """Before any publication the online calls return MON_ERR_STATE; once the manager's objects are idle they equal the scene calls on side 1 over the
    borrowed objects bit for bit, and meet the scene call's checks."""
    sc = scene
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    origin, step = tsd._enclosing(sc, SHAPE)
    for f in (lambda: m.signed_distance_lattice(origin, step, SHAPE, 1.0), lambda: m.signed_dist_field(origin, step, SHAPE, 1.0, 0.3)):
        with pytest.raises(pkg.MonError) as e:
            f()
        assert e.value.code == 5
    ids = tsr._online_feed(pkg, ss, sc, m, 3, 20)
    assert tsr._wait_trained(m, ids, 2)
    m.wait_threads_end()
    borrowed = [m.object(i) for i in ids]

    def call(smin, md, log):
        got = m.signed_distance_lattice(origin, step, SHAPE, smin, md, log=log)
        want = pkg.scene_signed_distance_lattice(borrowed, origin, step, SHAPE, smin, md, side=1, log=log)
        for g, w, name in zip(got[:5], want[:5], ("sdist", "nearest_edge", "nearest_owner", "sigma", "val")):
            _same(g, w, ("online", name, md, log))
        assert F(got[5]).view(np.uint32) == F(want[5]).view(np.uint32)
        return got
    smin = _check_scene(pkg, call, lambda: m.query_lattice(origin, step, SHAPE), step, "online")
    with m.signed_dist_field(origin, step, SHAPE, smin, 0.3) as f:
        _same(f.read().reshape(-1), call(smin, 0.3, True)[0], "online handle")
    m.close()


# ---------------------------------------------------------------------------------------------------------------- 4: the handle form
def test_handle_form(pkg, scene, trained):
    """A handle made by mon_scene_signed_dist_field: read() equals the lattice call's sdist; max_value is the largest value (the field has negative
    entries); sample, score, match and trace on it equal those of mon_dist_field_create(read()); a ray started inside matter with eps below 0 does not
    hit at its first sample, and status and range equal tests/field_trace_reference.py on the read-back field; the existing lattice routes keep their bits
    after signed calls of other sizes."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]; origin, step = tsd._enclosing(scene, SHAPE)
    nx, ny, nz = SHAPE
    sigma = pkg.query_scene_lattice(lst, origin, step, SHAPE, 0)[0]
    smin = tsd._sigma_min(sigma)

    def routes():
        comp = pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 1, 0.02, 18, side=0, rows=("dist",))
        path = pkg.scene_paths_lattice(lst, origin, step, SHAPE, smin, [0], side=0)
        with pkg.scene_dist_field(lst, origin, step, SHAPE, smin, 0.3, side=0) as g:
            cells = g.read()
        return (list(pkg.query_scene_lattice(lst, origin, step, SHAPE, 0)) + list(pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=0)) +
                [comp[0], comp[1], comp[4]["dist"]] + [path[0], path[1], cells])

    before = routes()
    for side, log in ((0, True), (1, False)):
        want = pkg.scene_signed_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=side, log=log)[0]
        with pkg.scene_signed_dist_field(lst, origin, step, SHAPE, smin, 0.3, side=side, log=log) as f:
            cells = f.read()
            _same(cells.reshape(-1), want, ("read", side, log))
            assert cells.min() < 0 < cells.max() and f.info().max_value == cells.max() and np.abs(cells).max() <= F(0.3)
            if side == 1:
                continue
            field = (cells, np.asarray(origin, F), np.asarray(step, F))
            rng = np.random.default_rng(31)
            with pkg.dist_field_create(cells, origin, step) as h:
                xyz = pkg.lattice_points(origin, step, SHAPE)[::5] + rng.normal(0, 0.3 * abs(float(step[0])), (len(range(0, nx * ny * nz, 5)), 3)).astype(F)
                for a, b in zip(f.sample(xyz, outside=0.3), h.sample(xyz, outside=0.3)):
                    _same(a, b, "sample")
                ways = xyz[:64 * 6].reshape(64, 6, 3); spheres = np.array([[0, 0, 0, 0.02], [0.03, 0, 0, 0.01]], F)
                sa = f.score(spheres, ways, n_sub=3, outside=0.3, margin=0.0, safe=0.05); sb = h.score(spheres, ways, n_sub=3, outside=0.3, margin=0.0, safe=0.05)
                for k in sa:
                    _same(sa[k], sb[k], ("score", k))
                poses = ft.field_poses(field, 3, 24)
                ma = f.match(xyz[:300], poses, huber=0.1, outside=0.3); mb = h.match(xyz[:300], poses, huber=0.1, outside=0.3)
                for k in ma:
                    _same(ma[k], mb[k], ("match", k))
                rays = ft.random_rays(field, 500, 23)
                ta = f.trace(rays, poses, normals=True); tb = h.trace(rays, poses, normals=True)
                for k in ta:
                    _same(ta[k], tb[k], ("trace", k))
            # rays from inside matter, less than 0.4 cell below the surface, along +x and -x; the level half a cell below the surface
            cell = abs(float(step[0])); flat = cells.reshape(-1); deep = np.flatnonzero((flat < 0) & (flat > -F(0.4 * cell)))
            assert deep.size >= 8, deep.size
            o = pkg.lattice_points(origin, step, SHAPE)[deep[:: max(1, deep.size // 64)]]
            rays = np.concatenate([np.concatenate([o, np.tile(F([1, 0, 0]), (len(o), 1))], 1), np.concatenate([o, np.tile(F([-1, 0, 0]), (len(o), 1))], 1)])
            prm = ft.trace_default(cells.shape, field[2]); prm["eps"] = F(-0.5 * cell)
            tp = pkg.TraceParams(*[int(prm[k]) if k == "max_steps" else float(prm[k]) for k in ft.FIELDS])
            got = f.trace(rays, None, tp); ref = ft.trace(cells, field[1], field[2], rays, None, prm)
            for k in ("range", "status", "steps"):
                _same(got[k], ref[k], ("trace from inside", k))
            first = (got["status"] == ft.HIT) & (got["steps"] <= 1)
            assert not first.any() and (got["steps"] > 1).any(), int(first.sum())
        pkg.scene_signed_distance_lattice(lst, origin, step * F(0.5), (40, 33, 30), smin, 0.2, side=side, log=log)      # 39 600 cells: the buffers grow
        pkg.scene_signed_distance_lattice(lst, origin, step, (5, 4, 3), smin, side=side)
    for i, (x, y) in enumerate(zip(before, routes())):
        _same(y, x, ("route output", i))


# ---------------------------------------------------------------------------------------------------------------- 5: the round trip on the device
def test_round_trip_registers_on_the_device(pkg):
    """The offset analytic case of tests/test_signed_distance_abi.py: mon_signed_distance_transform of val = -S / 0.02 equals the CPU reference's field bit
    for bit; a handle is created from it and mon_dist_field_register runs from the eight starts.  The bar is twice the worst figures the CPU chain reaches
    on the same field (1.535e-2 rad and 0.018 cell, so 3.07e-2 rad and 0.037 cell): the field is the same in every bit, the margin covers the host's
    double-precision solves, which the rule does not pin."""
    c = tsa.analytic_case()
    st, rot, tr = tsa.cpu_registration(c["sub_field"], c)
    sd, _ = pkg.signed_distance_transform(c["val"], 0.0, c["step"])
    _same(sd, c["sub_field"], "the device's field is the reference's")
    with pkg.dist_field_create(sd, c["origin"], c["step"]) as f:
        got = f.register(c["points"], c["starts"])
    done = iter(range(8))
    figs = tsa.registration_figures(c, lambda start: (lambda m: (got["poses"][m], got["status"][m]))(next(done)))      # (the starts come in order)
    print("device: status %s, worst %.3e rad, %.3f cell (CPU chain: %s, %.3e rad, %.3f cell)" % (figs[0], figs[1], figs[2], st, rot, tr))
    assert figs[0] == [0] * 8, figs[0]
    assert figs[1] <= 2 * rot and figs[2] <= 2 * tr, (figs, rot, tr)
