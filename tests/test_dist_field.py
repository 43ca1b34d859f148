"""Device-resident distance fields on the GPU (include/mon_core.h): mon_dist_field_sample and mon_dist_field_score against the numpy
restatement of the rule (tests/dist_field_reference.py, pinned on its own in tests/test_dist_field_abi.py), bit for bit in every case -- there is no tolerance
in this file; mon_scene_dist_field and mon_online_dist_field against mon_scene_distance_lattice's dist; the handle as a snapshot that outlives what it was
made from; and the existing lattice routes' bits after field creations of other sizes."""
import os

import numpy as np
import pytest

from conftest import ROOT
import dist_field_reference as dr
import test_scene_render as tsr
from test_scene_render import scene, trained       # noqa: F401 -- the module-scoped fixtures of the scene render's tests
from test_components import SHAPE, _enclosing

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = ((1, 1, 1), (37, 1, 1), (1, 37, 1), (1, 1, 37), (5, 4, 3), (19, 23, 17))                    # (nx, ny, nz)
STEPS = ((0.3, 0.7, 1.1), (0.25, 0.5, 0.125), (-0.3, 0.2, -0.45), (1.7e-6, 2.3e-6, 0.9e-6))         # anisotropic, powers of two, with negatives, tiny
SCORE_OUT = ("min_clear", "first_hit", "cost", "way_clear", "way_grad")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = _bits(got).reshape(-1); want = _bits(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "%d of %d differ, the first at %d: %#x, want %#x" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


_FIELDS = {}


def _field(shape, si):
    """a random non-negative field of the shape on step set si (computed once): (D (nz, ny, nx), origin, step)"""
    if (shape, si) not in _FIELDS:
        nx, ny, nz = shape; rng = np.random.default_rng(1000 + 10 * SHAPES.index(shape) + si)
        D = (rng.random((nz, ny, nx)) * 3.0).astype(F)
        o = (np.array([0.4, -1.3, 2.2], F) * F(1e-5 if si == 3 else 1.0)).astype(F)
        _FIELDS[shape, si] = (D, o, np.array(STEPS[si], F))
    return _FIELDS[shape, si]


def _points(shape, o, s, n, seed):
    """n points: most inside; then per axis coordinates on a face, one ulp to either side of it, far outside and NaN"""
    rng = np.random.default_rng(seed); dims = np.array(shape, np.float64)
    g = rng.random((n, 3)) * (dims - 1)
    p = (o.astype(np.float64) + g * s.astype(np.float64)).astype(F)
    k = 0
    for a in range(3):
        for face in (0.0, dims[a] - 1):
            on = F(np.float64(o[a]) + face * np.float64(s[a]))
            for v in (on, np.nextafter(on, F(np.inf)), np.nextafter(on, F(-np.inf)), F(on + F(1e6) * s[a]), F(on - F(1e6) * s[a]), F(np.nan), F(np.inf)):
                if k < n:
                    p[k, a] = v; k += 2                                             # (every other point stays wholly inside)
    return p


@pytest.mark.parametrize("shape", SHAPES)
def test_sample_equals_the_reference(pkg, shape):
    """every shape on the four step sets, 257 points each: d and grad in every bit, and d alone with grad3_out NULL"""
    for si in range(len(STEPS)):
        D, o, s = _field(shape, si)
        with pkg.dist_field_create(D, o, s) as f:
            info = f.info()
            assert (info.nx, info.ny, info.nz) == shape and info.max_value == D.max() and list(info.origin) == o.tolist()
            _same(f.read(), D, ("read", shape, si))
            p = _points(shape, o, s, 257, 7 * si + 1)
            d, g = f.sample(p, outside=-2.5)
            wd, wg = dr.sample(D, o, s, p, outside=-2.5)
            _same(d, wd, ("d", shape, si)); _same(g, wg, ("grad", shape, si))
            assert (wd == F(-2.5)).sum() >= (8 if max(shape) > 1 else 0) and (wd != F(-2.5)).sum() >= 100      # both sides of the faces are met
            d2, none = f.sample(p, outside=-2.5, grad=False)
            assert none is None
            _same(d2, wd, ("d without grad", shape, si))


@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_sample_counts(pkg, n):
    D, o, s = _field((19, 23, 17), 2)
    with pkg.dist_field_create(D, o, s) as f:
        p = _points((19, 23, 17), o, s, n, 50 + n)
        d, g = f.sample(p, outside=9.0)
        wd, wg = dr.sample(D, o, s, p, outside=9.0)
        _same(d, wd, ("d", n)); _same(g, wg, ("grad", n))
        again = f.sample(p, outside=9.0)
        _same(again[0], d, ("d again", n)); _same(again[1], g, ("grad again", n))


def _ways(shape, o, s, n_traj, n_way, seed, pose):
    """a short random walk per trajectory from a start in the lattice's box grown by a twentieth on every side (so bodies leave it here and there);
    trajectory 1 (if any) wholly outside"""
    rng = np.random.default_rng(seed); dims = np.array(shape, np.float64)
    g = rng.random((n_traj, n_way, 3)) * (dims - 1) * 1.1 - 0.05 * (dims - 1)
    g = np.cumsum(rng.normal(size=g.shape) * 0.3, axis=1) + g[:, :1]               # a walk from a random start: neighbouring waypoints are near each other
    p = (o.astype(np.float64) + g * s.astype(np.float64)).astype(F)
    if n_traj > 1:
        p[1] = (p[1] + F(1e3) * np.abs(s) * F(max(shape))).astype(F)
    return dr.pose_ways(p, seed) if pose else p


def _spheres(s, n, seed):
    rng = np.random.default_rng(seed); scale = np.abs(s).astype(np.float64)
    b = np.zeros((n, 4), F)
    b[:, :3] = (rng.normal(size=(n, 3)) * scale * 1.5).astype(F); b[:, 3] = (rng.random(n) * 0.6).astype(F)      # offsets in cells, radii in field values
    b[0, 3] = 0.0
    return b


KW = dict(outside=2.0, margin=0.8, safe=1.5)                                        # the fields' values lie in [0, 3)


# n_way, n_sub -> n_samp = (n_way - 1) n_sub + 1: 1, 2, 63, 64, 65 (a wave), 128, 129 (the workgroup of 128), 255, 257 (that of 256), 4 081 (the longest)
SCORE_CASES = (  # shape, step set, n_way, n_sub, n_spheres, n_traj, pose
    ((19, 23, 17), 0, 1, 3, 3, 5, False), ((19, 23, 17), 2, 2, 1, 1, 1, True), ((5, 4, 3), 2, 63, 1, 3, 5, False), ((19, 23, 17), 0, 22, 3, 32, 5, True),
    ((19, 23, 17), 1, 5, 16, 32, 300, False), ((19, 23, 17), 0, 5, 16, 3, 300, True), ((37, 1, 1), 1, 128, 1, 3, 5, False), ((1, 37, 1), 3, 129, 1, 1, 5, True),
    ((1, 1, 37), 2, 255, 1, 3, 5, False), ((19, 23, 17), 3, 17, 16, 3, 5, True), ((19, 23, 17), 2, 256, 16, 3, 5, False), ((5, 4, 3), 0, 256, 16, 1, 1, True),
    ((1, 1, 1), 0, 22, 3, 3, 5, False), ((19, 23, 17), 1, 44, 3, 1, 300, False))


@pytest.mark.parametrize("case", range(len(SCORE_CASES)))
def test_score_equals_the_reference(pkg, case):
    """all five outputs in every bit; a second call gives the same bits; so do three trajectories scored alone, and min_clear with every optional output
    NULL, and each optional output asked for alone"""
    shape, si, n_way, n_sub, n_sph, n_traj, pose = SCORE_CASES[case]
    D, o, s = _field(shape, si)
    ways = _ways(shape, o, s, n_traj, n_way, 300 + case, pose); sph = _spheres(s, n_sph, 400 + case)
    kw = dict(n_sub=n_sub, **KW)
    want = dr.score(D, o, s, sph, ways, **kw)
    if max(shape) > 1:                                                              # the case is not vacuous
        if n_traj > 1:
            assert want["min_clear"][1] == F(2.0) - sph[:, 3].max() and want["first_hit"][1] == -1 and (want["way_grad"][1] == 0).all()      # wholly outside
            assert len(set(want["first_hit"].tolist())) >= 2 and (want["way_grad"] != 0).any() and (want["first_hit"] >= 0).any()
        assert (want["cost"] > 0).any(), case
    with pkg.dist_field_create(D, o, s) as f:
        got = f.score(sph, ways, **kw)
        assert set(got) == set(SCORE_OUT)
        for k in SCORE_OUT:
            _same(got[k], want[k], (case, k))
        again = f.score(sph, ways, **kw)
        for k in SCORE_OUT:
            _same(again[k], got[k], (case, k, "second call"))
        for t in sorted({0, n_traj // 2, n_traj - 1}):
            alone = f.score(sph, ways[t:t + 1], **kw)
            for k in SCORE_OUT:
                _same(alone[k], got[k][t:t + 1], (case, k, "trajectory %d alone" % t))
        bare = f.score(sph, ways, outputs=(), **kw)
        assert set(bare) == {"min_clear"}
        _same(bare["min_clear"], got["min_clear"], (case, "every optional output NULL"))
        for k in SCORE_OUT[1:]:
            one = f.score(sph, ways, outputs=(k,), **kw)
            assert set(one) == {"min_clear", k}
            _same(one[k], got[k], (case, k, "asked for alone")); _same(one["min_clear"], got["min_clear"], (case, "min_clear beside", k))


def test_score_ties_on_a_wall(pkg):
    """dist = |x - 4| (exact numbers throughout): two spheres a quarter to either side of the body with equal radii tie at the wall, and the gradient is the
    lower one's (-1, not +1); a margin exactly equal to a clearance is a hit; first_hit is the lowest such sample although later ones hit too."""
    nx, ny, nz = 33, 5, 4
    D = np.broadcast_to(np.abs(np.arange(nx) - 16).astype(F) * F(0.25), (nz, ny, nx)).copy(); o = np.zeros(3, F); s = np.full(3, 0.25, F)
    n_way = 33; ways = np.zeros((2, n_way, 3), F)
    ways[:, :, 0] = (np.arange(n_way) * 0.25).astype(F); ways[:, :, 1] = 0.5; ways[:, :, 2] = 0.25; ways[1, :, 0] = ways[1, ::-1, 0].copy()
    sph = np.array([[-0.25, 0, 0, 0.125], [0.25, 0, 0, 0.125]], F)
    kw = dict(n_sub=2, outside=9.0, margin=0.5, safe=1.0)
    want = dr.score(D, o, s, sph, ways, **kw)
    # waypoint 16 is on the wall: the spheres sit at 3.75 and 4.25, both 0.25 from it; one sample on, a sphere's centre is on the wall itself
    assert want["way_grad"][:, 16].tolist() == [[-1.0, 0.0, 0.0]] * 2 and (want["way_clear"][:, 16] == F(0.125)).all() and (want["min_clear"] == F(-0.125)).all()
    # the body's leading sphere is 0.625 from the wall, clear 0.5 == margin, when the body is at 3.125 going up and at 4.875 going down: sample 25 of both
    assert want["first_hit"].tolist() == [25, 25]
    with pkg.dist_field_create(D, o, s) as f:
        got = f.score(sph, ways, **kw)
    for k in SCORE_OUT:
        _same(got[k], want[k], ("wall", k))


@pytest.fixture(scope="module")
def lattice(scene):
    return _enclosing(scene, SHAPE)


def _probe(pkg, f, o, s, seed=9):
    """a handle's answers to one fixed sample call and one fixed score call"""
    p = _points(SHAPE, o, s, 500, seed)
    ways = _ways(SHAPE, o, s, 7, 9, seed + 1, True); sph = _spheres(s, 4, seed + 2)
    sc = f.score(sph, ways, n_sub=4, outside=0.5, margin=0.02, safe=0.1)
    return [f.read()] + list(f.sample(p, outside=0.5)) + [sc[k] for k in SCORE_OUT]


def _same_probe(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, (what, i))


def _pick_sigma_min(sigma):
    smin = float(np.percentile(sigma, 90.0, method="lower"))
    occ = int((~(sigma <= F(smin))).sum())
    assert smin >= 0 and 0 < occ < sigma.size
    return smin


@pytest.mark.parametrize("side", [0, 1])
def test_scene_field_equals_the_distance_call(pkg, scene, trained, lattice, side):
    """mon_dist_field_read equals mon_scene_distance_lattice's dist for the same arguments in every bit; sample and score on the handle equal the same calls
    on mon_dist_field_create(that dist); info reports the lattice and the largest value"""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]; origin, step = lattice
    smin = _pick_sigma_min(pkg.query_scene_lattice(lst, origin, step, SHAPE, side)[0])
    for max_dist in (0.3, 1e3):
        dist = pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, max_dist, side=side, free=False)[0]
        assert 0 < (dist == 0).sum() < dist.size
        with pkg.scene_dist_field(lst, origin, step, SHAPE, smin, max_dist, side=side) as f, \
                pkg.dist_field_create(dist.reshape(SHAPE[::-1]), origin, step) as h:
            info = f.info()
            assert (info.nx, info.ny, info.nz) == SHAPE and list(info.origin) == origin.tolist() and list(info.step) == step.tolist()
            assert info.max_value == dist.max() <= F(max_dist)
            _same(f.read(), dist, ("read", side, max_dist))
            _same_probe(_probe(pkg, f, origin, step), _probe(pkg, h, origin, step), ("scene handle against created handle", side, max_dist))


def test_online_field_outlives_its_manager(pkg, ss, scene, lattice):
    """mon_online_dist_field: MON_ERR_STATE before any publication; then the cells of mon_online_distance_lattice; the handle answers with the same bits
    after the manager is destroyed"""
    sc = scene; origin, step = lattice
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    with pytest.raises(pkg.MonError) as e:
        m.dist_field(origin, step, SHAPE, 1.0, 0.5)
    assert e.value.code == 5
    ids = tsr._online_feed(pkg, ss, sc, m, 3, 20)
    assert tsr._wait_trained(m, ids, 2)
    m.wait_threads_end()
    smin = _pick_sigma_min(m.query_lattice(origin, step, SHAPE)[0])
    dist = m.distance_lattice(origin, step, SHAPE, smin, 0.4, free=False)[0]
    f = m.dist_field(origin, step, SHAPE, smin, 0.4)
    _same(f.read(), dist, "online read")
    before = _probe(pkg, f, origin, step)
    m.close()
    _same_probe(_probe(pkg, f, origin, step), before, "after the manager is gone")
    f.close()


def test_existing_routes_keep_their_bits(pkg, scene, trained, lattice):
    """the lattice query, the gradients, the distance, the components and the paths calls after field creations of other sizes in the same side's
    workspace give the bits from before them"""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]; origin, step = lattice

    def routes(side, smin):
        xyz = pkg.lattice_points(origin, step, SHAPE)[::7]
        comp = pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 1, 0.02, 18, side=side, rows=("dist",))
        path = pkg.scene_paths_lattice(lst, origin, step, SHAPE, smin, [0], side=side)
        return (list(pkg.query_scene_lattice(lst, origin, step, SHAPE, side)) + list(pkg.query_scene_gradients(lst, xyz, side=side)) +
                list(pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=side)) + [comp[0], comp[1], comp[4]["dist"]] + [path[0], path[1]])

    for side in (0, 1):
        smin = _pick_sigma_min(pkg.query_scene_lattice(lst, origin, step, SHAPE, side)[0])
        before = routes(side, smin)
        pkg.scene_dist_field(lst, origin, step * F(0.5), (40, 33, 30), smin, 0.2, side=side).close()      # the buffers grow
        with pkg.scene_dist_field(lst, origin, step * F(4), (5, 4, 3), smin, 5.0, side=side) as small:
            assert small.read().shape == (3, 4, 5)
        pkg.scene_dist_field(lst, origin, step, SHAPE, smin, 0.3, side=side).close()
        for i, (b, a) in enumerate(zip(before, routes(side, smin))):
            _same(a, b, ("route output", i, side))


def test_handle_is_a_snapshot(pkg, scene, trained, lattice):
    """(last: it trains the module's objects further)  The handle still answers with the same bits after the objects have trained on, while a new
    field of the same arguments has moved"""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]; origin, step = lattice
    for side in (0, 1):
        smin = _pick_sigma_min(pkg.query_scene_lattice(lst, origin, step, SHAPE, side)[0])
        f = pkg.scene_dist_field(lst, origin, step, SHAPE, smin, 0.3, side=side)
        before = _probe(pkg, f, origin, step)
        sigma0 = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)[0]
        for ob in lst:
            ob.train(20)
        assert not np.array_equal(pkg.query_scene_lattice(lst, origin, step, SHAPE, side)[0], sigma0)      # the map did move
        _same_probe(_probe(pkg, f, origin, step), before, ("after further training", side))
        f.close()
