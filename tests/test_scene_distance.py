"""GPU tests (-m gpu) of the distance fields (mon_distance_transform, mon_scene_distance_lattice, mon_online_distance_lattice; kernels k_distance_pass,
k_distance_mask and k_distance_finish in kernels_distance.hip).  The yardstick of the transform is tests/distance_reference.py, the header's rule in
numpy fp32, itself pinned against a brute force over all pairs by tests/test_scene_distance_abi.py: the device equals it bit for bit, in dist and in
nearest, whatever the kernel prunes.  The scene call is held to public calls: its sigma to mon_scene_query_lattice, its fields to mon_distance_transform
of the mask derived from that sigma.  The scene, the trained objects and the manager's feed are those of tests/test_scene_render.py."""
import os

import numpy as np
import pytest

from conftest import ROOT
import distance_reference as dr
import test_scene_render as tsr
from test_scene_render import scene, trained       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu

# 1 x 1 x 1; one line along each axis; no dimension a multiple of 32; more cells than one 16 384-point pass; three lines that cross the 4 096-cell tile
SHAPES = ((1, 1, 1), (37, 1, 1), (1, 41, 1), (1, 1, 29), (19, 23, 17), (33, 31, 29), (4133, 3, 2), (3, 4133, 2), (2, 3, 4133))
STEPS = ((0.013, 0.0217, 0.0091), (0.25, 0.25, 0.25), (0.1, -0.2, 0.3), (0.05, 0.0, 0.05))
DENSITIES = (0, "one", 0.02, 0.5, 1)

_cache = {}


def _case(shape, step, di):
    """the mask of (shape, density DENSITIES[di]) and its reference (d2, site) under `step`, computed once"""
    key = (shape, step, di)
    if key not in _cache:
        m = dr.random_mask(shape, DENSITIES[di], seed=1000 * di + sum(shape))
        _cache[key] = (m,) + dr.separable(m, step)
    return _cache[key]


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    ne = got.view(np.uint32) != want.view(np.uint32)
    assert not ne.any(), (what, int(ne.sum()), got[ne][:4], want[ne][:4])


# ---------------------------------------------------------------------------------------------------------------- 1: the transform against the reference
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_transform_equals_the_reference(pkg, shape, step):
    """mon_distance_transform equals the numpy restatement bit for bit in dist and nearest, at densities 0, one cell, 2 %, 50 % and all cells (1 x 1 x 1:
    free and occupied).  dist is np.sqrt of the reference's d2, the correctly rounded root."""
    for di in range(len(DENSITIES)):
        m, d2, site = _case(shape, step, di)
        want = dr.finish(d2, site, np.inf)
        dist, near = pkg.distance_transform(m, step)
        _same(dist, want[0], ("dist", shape, step, DENSITIES[di])); _same(near, want[1], ("nearest", shape, step, DENSITIES[di]))
        if not m.any():
            assert np.isinf(dist).all() and (near == -1).all()
    if shape == (1, 1, 1):
        assert _case(shape, step, 0)[0].sum() == 0 and _case(shape, step, 4)[0].sum() == 1


# ---------------------------------------------------------------------------------------------------------------- 2: truncation
@pytest.mark.parametrize("shape,step,di", [((19, 23, 17), STEPS[0], 2), ((33, 31, 29), STEPS[1], 2), ((4133, 3, 2), STEPS[2], 1)])
def test_truncation(pkg, shape, step, di):
    """max_dist below one step, equal to a distance that occurs in the field, and large: each equals the untruncated result clipped by the header's rule
    (where not (dist <= max_dist): dist = max_dist, nearest = -1), bit for bit; the cells at exactly max_dist keep their sites."""
    m, d2, site = _case(shape, step, di)
    full, near = pkg.distance_transform(m, step)
    _same(full, dr.finish(d2, site, np.inf)[0], "untruncated")
    pos = np.unique(full[full > 0])
    occurs = float(pos[len(pos) // 2])                                                 # a distance of the field, from the middle of those that occur
    below = 0.5 * min(abs(s) for s in step if s != 0)
    for md in (below, occurs, 1e30, np.inf):
        dist, nr = pkg.distance_transform(m, step, max_dist=md)
        cut = ~(full <= np.float32(md))
        _same(dist, np.where(cut, np.float32(md), full), ("dist", md)); _same(nr, np.where(cut, np.int32(-1), near), ("nearest", md))
        _same(dist, dr.finish(d2, site, md)[0], ("reference", md))
    dist, nr = pkg.distance_transform(m, step, max_dist=occurs)
    at = full == np.float32(occurs)
    assert at.any() and (nr[at] >= 0).all() and (dist[at] == np.float32(occurs)).all() and (full > np.float32(occurs)).any()
    dist, nr = pkg.distance_transform(m, step, max_dist=below)
    assert (dist[m != 0] == 0).all() and (dist[m == 0] == np.float32(below)).all() and (nr[m == 0] == -1).all()
    _same(pkg.distance_transform(m, step, max_dist=occurs, nearest=False)[0], dr.finish(d2, site, occurs)[0], "nearest NULL")


# ---------------------------------------------------------------------------------------------------------------- 3: determinism
def test_determinism_and_prefix(pkg):
    """Two calls give equal bits; the transform of a mask that is the prefix of a larger buffer (other bytes behind it) is unchanged; any non-zero byte
    counts as occupied."""
    L = pkg.lib(); shape = (33, 31, 29); step = STEPS[0]; nx, ny, nz = shape
    m, d2, site = _case(shape, step, 2)
    a = pkg.distance_transform(m, step); b = pkg.distance_transform(m, step)
    _same(a[0], b[0], "dist twice"); _same(a[1], b[1], "nearest twice")
    big = np.concatenate([m.reshape(-1) * np.uint8(200), np.full(5000, 1, np.uint8)])
    dist = np.empty(m.size + 64, np.float32); near = np.empty(m.size + 64, np.int32); dist[m.size:] = 7.0; near[m.size:] = 7
    s = np.asarray(step, np.float32)
    vp = lambda x: x.ctypes.data_as(__import__("ctypes").c_void_p)      # noqa: E731
    assert L.mon_distance_transform(0, vp(big), nx, ny, nz, vp(s), float("inf"), vp(dist), vp(near)) == 0
    _same(dist[:m.size].reshape(m.shape), a[0], "prefix dist"); _same(near[:m.size].reshape(m.shape), a[1], "prefix nearest")
    assert (dist[m.size:] == 7.0).all() and (near[m.size:] == 7).all()                 # nothing is written behind the lattice


# ---------------------------------------------------------------------------------------------------------------- 4: the scene call
SHAPE = (24, 20, 18)


def _enclosing(sc, shape, margin=0.1):
    """origin and step of a lattice that encloses the three objects' boxes with a margin of 10 % of the extent on every side"""
    pts = []
    for ob in sc.objects[:3]:
        c = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * ob["half"]
        pts.append(c @ ob["Two"][:3, :3].T + ob["Two"][:3, 3])
    pts = np.concatenate(pts); lo = pts.min(0); hi = pts.max(0); pad = margin * (hi - lo)
    lo -= pad; hi += pad
    return lo.astype(np.float32), ((hi - lo) / (np.array(shape) - 1)).astype(np.float32)


def _sigma_min(sigma):
    """A threshold that leaves both kinds of cell: the 90th percentile of the lattice query's own sigma, one of its values (0 where fewer than a tenth of
    the cells lie in a box: then every cell inside a box is occupied).  The test asserts the two counts before it calls the new code."""
    return float(np.percentile(sigma, 90.0, method="lower"))


def _check_scene(pkg, call, query, what, n_owners):
    """`call(sigma_min, max_dist, free)` = the distance call, `query()` = the lattice query over the same objects: the five properties of the scene call"""
    nx, ny, nz = SHAPE; n = nx * ny * nz
    sigma, _, owner, _, _ = query()
    smin = _sigma_min(sigma)
    occ = ~(sigma <= np.float32(smin)); n_occ = int(occ.sum())
    print("%s: sigma_min %.5g, %d of %d cells occupied" % (what, smin, n_occ, n))
    assert n_occ >= n // 100 + 1 and n - n_occ >= n // 100 + 1, (n_occ, n)
    mask = occ.reshape(nz, ny, nx)
    for md in (np.inf, 0.35):
        dist, near, nown, free, sig = call(smin, md, True)
        _same(sig, sigma, (what, "sigma", md))
        wd, wn = call.step_transform(mask, md)
        _same(dist, wd.reshape(-1), (what, "dist", md)); _same(near, wn.reshape(-1), (what, "nearest", md))
        _same(free, call.step_transform(~mask, md)[0].reshape(-1), (what, "free_dist", md))
        assert np.array_equal(nown, np.where(near >= 0, owner[np.maximum(near, 0)], -1)), (what, "nearest_owner", md)
        assert (dist[occ] == 0).all() and (free[~occ] == 0).all() and (dist[~occ] > 0).all() and (free[occ] > 0).all()
        d_only = call(smin, md, False)
        assert d_only[3] is None
        _same(d_only[0], dist, (what, "dist without free_dist", md))
    assert len(set(np.unique(nown)) - {-1}) >= n_owners, np.unique(nown)
    return smin


@pytest.mark.parametrize("side", [0, 1])
def test_scene_call(pkg, scene, trained, side):
    """On a 24 x 20 x 18 lattice around the three objects (b0's inflated box covers part of it, a1 and a2 their own boxes), sides 0 and 1: sigma equals
    mon_scene_query_lattice's bits; dist and nearest equal mon_distance_transform of the mask derived from that sigma; free_dist equals the transform
    of the complement; nearest_owner == owner[nearest]; with free_dist, nearest and nearest_owner passed as NULL, dist has the same bits.  Untruncated and
    with max_dist 0.35."""
    L = pkg.lib(); _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = _enclosing(scene, SHAPE)

    def call(smin, md, free):
        return pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, md, side=side, free=free)
    call.step_transform = lambda mask, md: pkg.distance_transform(mask, step, max_dist=md)
    smin = _check_scene(pkg, call, lambda: pkg.query_scene_lattice(lst, origin, step, SHAPE, side), "side %d" % side, 2)
    # dist alone: every optional output NULL
    import ctypes as C
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]; d = np.empty(n, np.float32); hs = (C.c_void_p * 3)(*[o.h for o in lst])
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.mon_scene_distance_lattice(hs, 3, side, vp(origin), vp(step), *SHAPE, smin, float("inf"), vp(d), None, None, None, None) == 0
    _same(d, call(smin, np.inf, True)[0], "dist with every optional output NULL")


# ---------------------------------------------------------------------------------------------------------------- 5: the online call
def test_online_call(pkg, ss, scene, trained):
    """Before any publication mon_online_distance_lattice returns MON_ERR_STATE; once the manager's objects are idle it equals the scene call on side 1
    over the borrowed objects bit for bit, nearest_owner holding the manager's indices (here the list's own), and meets the scene call's checks."""
    sc = scene
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    origin, step = _enclosing(sc, SHAPE)
    with pytest.raises(pkg.MonError) as e:
        m.distance_lattice(origin, step, SHAPE, 1.0)
    assert e.value.code == 5
    ids = tsr._online_feed(pkg, ss, sc, m, 3, 20)
    assert tsr._wait_trained(m, ids, 2)
    m.wait_threads_end()
    borrowed = [m.object(i) for i in ids]

    def call(smin, md, free):
        got = m.distance_lattice(origin, step, SHAPE, smin, md, free=free)
        want = pkg.scene_distance_lattice(borrowed, origin, step, SHAPE, smin, md, side=1, free=free)
        for g, w, name in zip(got, want, ("dist", "nearest", "nearest_owner", "free_dist", "sigma")):
            if w is None:
                assert g is None
            else:
                _same(g, w, ("online", name, md))
        return got
    call.step_transform = lambda mask, md: pkg.distance_transform(mask, step, max_dist=md)
    _check_scene(pkg, call, lambda: m.query_lattice(origin, step, SHAPE), "online", 1)
    m.close()


# ---------------------------------------------------------------------------------------------------------------- 6: the existing routes
def test_existing_routes_keep_their_bits(pkg, scene, trained):
    """The lattice query's five outputs (and a list query's, and the gradients') after distance calls of other sizes in the same side's workspace are the
    bits from before them: the shared workspace is not disturbed."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = _enclosing(scene, SHAPE)
    for side in (0, 1):
        before = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)
        xyz = pkg.lattice_points(origin, step, SHAPE)[::7]
        g_before = pkg.query_scene_gradients(lst, xyz, side=side)
        smin = _sigma_min(before[0])
        pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, side=side)
        pkg.scene_distance_lattice(lst, origin, step * np.float32(0.5), (40, 33, 30), smin, 0.2, side=side)      # 39 600 cells: the buffers grow
        pkg.scene_distance_lattice(lst, origin, step, (5, 4, 3), smin, side=side, free=False)
        after = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)
        for b, a, name in zip(before, after, ("sigma", "rgb", "owner", "owner_sigma", "n_inside")):
            _same(a, b, ("lattice query", name, side))
        for b, a in zip(g_before, pkg.query_scene_gradients(lst, xyz, side=side)):
            _same(a, b, ("gradients", side))
