"""GPU tests (-m gpu) of the point queries against the object map (mon_object_query_points, mon_scene_query_points, mon_scene_query_lattice,
mon_online_query_points / _lattice; kernels k_scene_points and k_scene_points_fold in kernels_scene_points.hip).  The yardsticks are ones the project
already trusts: the raw outputs against the existing density lattice (mon_object_density_grid) and against the oracle's encode + MLP at the weights the
device reports, held to the bar of test_object_mesh_matches_oracle; the transform against an fp64 restatement within a bound counted rounding by
rounding; the scene call against a numpy fold of the diagnostic rows, bit for bit; the activations against fp64 functions of the rows' own raw
outputs within a counted bound; list against lattice, order against order, manager against scene call, bit for bit.  The scene, the trained objects
and the overlap view are those of tests/test_scene_render.py."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import ROOT
import test_scene_render as tsr
from test_scene_render import scene, trained, overlap_view       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu

CHUNK = 16384                # kRenderChunkRays: the points of one pass
U = 2.0 ** -24               # unit roundoff of fp32
TINY = 2.0 ** -126           # the smallest normal fp32: below it the hardware exponential may flush to zero
F32_MAX = float(np.finfo(np.float32).max)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same_bits(got, want, what=""):
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, i, int((_bits(g) != _bits(w)).sum()))


def _box(sc, k, inflate=1.0):
    """Object k's device-side constants as the tests' fixtures create them: Tow16 (fp32, column-major), aabb min / max (fp32)."""
    ob = sc.objects[k]
    return (np.ascontiguousarray(np.asarray(ob["Tow"], np.float32).T.reshape(16)), np.asarray(-ob["half"] * inflate, np.float32),
            np.asarray(ob["half"] * inflate, np.float32))


def _world(sc, k, p_obj):
    """Object-frame points of object k in the world, fp64 -> fp32."""
    Two = sc.objects[k]["Two"]
    return (np.asarray(p_obj, np.float64) @ Two[:3, :3].T + Two[:3, 3]).astype(np.float32)


def _in_box(sc, k, n, rng, inflate=1.0):
    return _world(sc, k, rng.uniform(-1.0, 1.0, (n, 3)) * sc.objects[k]["half"] * inflate)


@pytest.fixture(scope="module")
def cloud(scene):
    """3 937 world points (no multiple of 32 or 256): 3 000 uniform in 1.2 x b0's box (object 0's box inflated 5 x, which reaches into both others; the
    margin leaves points outside every box), 300 in each object's own box, the eight corners of a1's box computed in fp64, and 29 more in a1's box."""
    rng = np.random.RandomState(11); sc = scene
    h1 = sc.objects[1]["half"]
    corners = _world(sc, 1, np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h1)
    x = np.concatenate([_in_box(sc, 0, 3000, rng, 6.0)] + [_in_box(sc, k, 300, rng) for k in range(3)] + [corners, _in_box(sc, 1, 29, rng)])
    assert x.shape[0] == 3937
    return x


def _oracle_raw(orc, kw, params_u16, u):
    """orc_encode + orc_mlp_forward of the oracle at unit-cube points u (n, 3) on the fp16 parameter vector given: raw outputs (n, 4) widened to fp32."""
    m = orc.OracleModel(orc.default_config(**kw))
    try:
        u = np.ascontiguousarray(u, np.float32); n = u.shape[0]; prm = np.ascontiguousarray(params_u16, np.uint16)
        assert prm.size == m.n_params
        E = np.zeros(n * m.Epad, np.uint16); hid = np.zeros(n * m.W * m.NH, np.uint16); O = np.zeros(n * 4, np.uint16)
        P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        m.L.orc_encode(m.h, P(prm), P(u), n, P(E)); m.L.orc_mlp_forward(m.h, P(prm), P(E), n, P(hid), P(O))
        return orc.h2f(O.reshape(n, 4))
    finally:
        m.close()


def _lattice_u(r):
    f = np.float32
    z, y, x = np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij")
    return np.ascontiguousarray(np.stack([x.astype(f) / f(r - 1), y.astype(f) / f(r - 1), z.astype(f) / f(r - 1)], -1).reshape(-1, 3))


def _logistic64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _mesh_bar(raw, ref, what, share=True):
    """The bar test_object_mesh_matches_oracle holds the lattice and the vertex colours to: raw3 equal on more than 0.999 of the points (asked on the
    32^3 lattice only), |d raw3| < 0.05, colours after the logistic within 2e-3."""
    eq = float((raw[:, 3] == ref[:, 3]).mean()); d3 = float(np.abs(raw[:, 3] - ref[:, 3]).max())
    dc = float(np.abs(_logistic64(raw[:, :3]) - _logistic64(ref[:, :3])).max())
    print("%s: raw3 equal on %.5f of %d points, max |d raw3| %.4g, max |d colour| %.3g" % (what, eq, raw.shape[0], d3, dc))
    assert d3 < 0.05 and dc < 2e-3, what
    if share:
        assert eq > 0.999, what


# ---------------------------------------------------------------------------------------------------------------- 1: the existing lattice route
# (object, tile_render) paths whose density lattice the point query reproduces bit for bit: the default path (level tiles + the MFMA network of
# kernels_tilerender.hip).  With tile_render 0 the lattice comes from the layer-at-a-time kernels (k_encode + the fp32-sum MLP of kernels_net.hip, the oracle's
# summation order), which differ from the MFMA network by one fp16 ulp on 0.04 % of a 32^3 lattice (equal on 0.99960, max |d| 0.0156 on both networks;
# 17^3: 0.99980 / 0.99939): that path is held to test 2's bar
EXACT = {("a1", -1), ("n2", -1)}


@pytest.mark.parametrize("tile", [-1, 0])
@pytest.mark.parametrize("name", ["a1", "n2"])
def test_raw_outputs_against_the_density_lattice(pkg, trained, name, tile):
    """mon_object_query_points at the 17^3 lattice u = i / 16 (and the 32^3 lattice u = i / 31): channel 3 against mon_object_density_grid, with the option
    tile_render at its default (-1 here: left alone) and at 0, on a 64 x 1 and a 32 x 2 network.  Bit equality on the paths of EXACT; a path that is not
    in it is held to test 2's bar instead (the share on the 32^3 lattice)."""
    _, objs = trained; o = objs[name]
    old = pkg.get_option("tile_render")
    try:
        if tile == 0:
            pkg.set_option("tile_render", 0)
        d17 = o.density_grid(17, 17, 17); d32 = o.density_grid(32, 32, 32)
    finally:
        pkg.set_option("tile_render", old)
    r17 = pkg.query_object_points(o, _lattice_u(17)); r32 = pkg.query_object_points(o, _lattice_u(32))
    assert np.isfinite(r17).all() and np.isfinite(r32).all() and np.ptp(r17[:, 3]) > 1.0          # a trained field, not a constant
    for r, d, n in ((r17, d17, 17), (r32, d32, 32)):
        print("%s tile_render %d, %d^3: raw3 equal on %.5f, max |d| %.4g" % (name, tile, n, float((r[:, 3] == d).mean()), float(np.abs(r[:, 3] - d).max())))
    if (name, tile) in EXACT:
        assert np.array_equal(_bits(r17[:, 3]), _bits(d17)) and np.array_equal(_bits(r32[:, 3]), _bits(d32))
    else:
        assert np.abs(r17[:, 3] - d17).max() < 0.05 and np.abs(r32[:, 3] - d32).max() < 0.05 and (r32[:, 3] == d32).mean() > 0.999


# ---------------------------------------------------------------------------------------------------------------- 2: the oracle
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", ["a1", "n2"])
def test_raw_outputs_against_the_oracle(pkg, orc, trained, name, side):
    """mon_object_query_points at 1 037 points (the 9^3 lattice, the 8 corners, 300 random interior points) and at the 32^3 lattice against orc_encode +
    orc_mlp_forward on the inference weights the object reports (the EMA: what side 0 reads and what the last train call published to side 1).  The
    bar of test_object_mesh_matches_oracle: |d raw3| < 0.05, colours after the logistic within 2e-3, and raw3 equal on more than 0.999 of the 32^3
    lattice.  A point outside the unit cube is MON_ERR_ARG."""
    _, objs = trained; o = objs[name]; kw = tsr.NARROW if name == "n2" else tsr.BASE
    rng = np.random.RandomState(5)
    corners = np.array([[sx, sy, sz] for sx in (0, 1) for sy in (0, 1) for sz in (0, 1)], np.float32)
    u = np.concatenate([_lattice_u(9), corners, rng.uniform(0.0, 1.0, (300, 3)).astype(np.float32)])
    assert u.shape[0] == 1037
    ema = o.get_params(2)
    _mesh_bar(pkg.query_object_points(o, u, side), _oracle_raw(orc, kw, ema, u), "%s side %d, 1 037 points" % (name, side), share=False)
    u32 = _lattice_u(32)
    _mesh_bar(pkg.query_object_points(o, u32, side), _oracle_raw(orc, kw, ema, u32), "%s side %d, 32^3" % (name, side))
    bad = u.copy(); bad[500, 1] = np.float32(1.0000001)
    with pytest.raises(pkg.MonError) as e:
        pkg.query_object_points(o, bad, side)
    assert e.value.code == 1


# ---------------------------------------------------------------------------------------------------------------- 3: independence
def test_independence(pkg, scene, trained):
    """16 384 + 37 points (two passes with a ragged tail) against {b0, a1, a2}: asked in order, permuted, as a strict subset and with duplicates, every
    point's five outputs keep their bits."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    rng = np.random.RandomState(17); n = CHUNK + 37
    x = np.concatenate([_in_box(scene, 0, n - 600, rng, 6.0), _in_box(scene, 1, 300, rng), _in_box(scene, 2, 300, rng)])[rng.permutation(n)]
    base = pkg.query_scene_points(lst, x)
    assert (base[4] >= 2).sum() >= 50 and (base[4] == 0).sum() >= 50 and (base[2] > 0).sum() >= 50
    for what, idx in (("permuted", rng.permutation(n)), ("subset", np.sort(rng.choice(n, 5003, replace=False))),
                      ("duplicates", rng.randint(0, n, n + 300)), ("reversed tail", np.arange(n - 1, n - 300, -1))):
        _same_bits(pkg.query_scene_points(lst, x[idx]), [a[idx] for a in base], what)


# ---------------------------------------------------------------------------------------------------------------- 4: the transform rows
def ref_unit(Tow16, mn, mx, x):
    """fp64 restatement of a point's way into an object's unit cube on the fp32 inputs, with the first-order forward error bound of its fp32 evaluation,
    counted the way tests/test_scene_cast.py's ref_world_rays counts (each rounding at most U = 2^-24 relative to its result):
      q = Row x + tow          one rot3 of (mul, fma, fma) and one add                 ->  Eq = 4 U Mo, Mo = |Row| |x| + |tow| (the terms summed)
      q - mn                   inherits Eq, one rounding                               ->  Eq + U |q - mn|
      mx - mn                  one rounding: U relative in the divisor                 ->  U |u|
      u = (q - mn) / (mx - mn) one rounding                                            ->  U |u|
    so E_u = (4 U Mo + U |q - mn|) / |mx - mn| + 2 U |u|.  Returns u, E_u."""
    T = np.asarray(Tow16, np.float32).astype(np.float64).reshape(4, 4).T; R, t = T[:3, :3], T[:3, 3]
    x = np.asarray(x, np.float32).astype(np.float64); mn = np.asarray(mn, np.float32).astype(np.float64); mx = np.asarray(mx, np.float32).astype(np.float64)
    q = x @ R.T + t; w = mx - mn; u = (q - mn) / w
    Mo = np.abs(x) @ np.abs(R).T + np.abs(t)
    return u, (4 * U * Mo + U * np.abs(q - mn)) / np.abs(w) + 2 * U * np.abs(u)


def test_transform_rows_against_fp64(pkg, scene, trained, cloud):
    """Every object's rows of {b0, a1, a2} at the cloud: u within ref_unit's bound of the fp64 value; the inside flag equals the fp64 decision except
    where a coordinate lies within its bound of 0 or 1 -- those points are left out, at most 1 % of them per object (checked on the fp64 restatement
    alone, before the device is asked); the eight corners of a1's box, computed in fp64, are among the points (ambiguous for a1: left out there).  A
    point outside the box holds u, 0 and eight zeros."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]; x = cloud
    boxes = [_box(scene, 0, 5.0), _box(scene, 1), _box(scene, 2)]
    refs = []
    for Tow, mn, mx in boxes:
        u, E = ref_unit(Tow, mn, mx, x)
        amb = ((np.abs(u) <= E) | (np.abs(u - 1.0) <= E)).any(1)
        assert amb.mean() <= 0.01, amb.mean()
        refs.append((u, E, amb, ((u >= 0.0) & (u <= 1.0)).all(1)))
    print("a1's corners (points 3900..3907): ambiguous for a1 %d of 8, inside b0 %d of 8" % (refs[1][2][3900:3908].sum(), refs[0][3][3900:3908].sum()))
    worst = 0.0
    for k in range(3):
        rows = pkg.scene_point_rows(lst, x, k); u, E, amb, ins = refs[k]
        r = np.abs(rows[:, :3].astype(np.float64) - u) / E
        worst = max(worst, float(r.max()))
        assert (r <= 1.0).all(), (k, float(r.max()))
        flag = rows[:, 3]
        assert set(np.unique(flag)) <= {0.0, 1.0} and np.array_equal(flag[~amb] != 0, ins[~amb]), k
        assert (flag != 0).sum() >= 300 and (flag == 0).sum() >= 300
        assert (rows[flag == 0, 4:] == 0).all() and np.isfinite(rows).all()
        # the flag is the comparison of the row's own u
        assert np.array_equal(flag != 0, ((rows[:, :3] >= 0) & (rows[:, :3] <= 1)).all(1))
    print("transform rows: largest |u - fp64| / bound %.3f; left out %s" % (worst, [int(r[2].sum()) for r in refs]))


# ---------------------------------------------------------------------------------------------------------------- 5: the fold
def np_fold(rows):
    """numpy restatement of k_scene_points_fold on the objects' rows [K][n][12]: the fp32 sum in list order, the first largest sigma_k."""
    rows = np.asarray(rows, np.float32); K, n = rows.shape[:2]
    ins = rows[:, :, 3] != 0; sig = rows[:, :, 8]
    s = np.zeros(n, np.float32)
    with np.errstate(over="ignore"):
        for k in range(K):
            s = np.where(ins[k], (s + sig[k]).astype(np.float32), s)
    key = np.where(ins, sig, -1.0)                                                           # sigma_k >= 0: -1 never wins against an inside object
    own = np.where(ins.any(0), key.argmax(0), -1).astype(np.int32)                           # (argmax: the first maximum)
    pick = rows[np.maximum(own, 0), np.arange(n)]
    has = own >= 0
    return (s, np.where(has[:, None], pick[:, 9:12], 0.0).astype(np.float32), own, np.where(has, pick[:, 8], 0.0).astype(np.float32),
            ins.sum(0).astype(np.uint32))


@pytest.mark.parametrize("names", [("a1",), ("a0", "b0", "n2"), ("b0", "a1", "a2")])
def test_fold_and_activations(pkg, trained, cloud, names):
    """K = 1, K = 3 ({a0, b0, n2}: a0's box lies inside b0's, n2 is a 32 x 2 network) and {b0, a1, a2}: the five outputs equal, bit for bit, np_fold of
    the objects' diagnostic rows.  Each list holds at least 50 points inside two or more boxes (K = 1 cannot: a point is inside one box or none), at least
    50 inside exactly one and at least 50 inside none, and at least 50 points owned by an object other than the first (K = 1 has none to own them).
    Every inside row's raw4 is, bit for bit, mon_object_query_points of that object at the row's own u: the compacted tile evaluated the network where
    the row says it did (the world route's tile lanes form u again; tests 1 and 2 reach only the route without the transform).
    The activations against fp64 functions of the row's own raw4, with a counted bound.  sigma = __expf(x) is v_exp_f32(x * log2(e)): the constant's
    and the product's roundings put the exponent off by at most 2 U |x| log2(e), i.e. 2 U |x| relative in the result, and the hardware exponential is
    good to 1 ulp <= 2 U relative: |d sigma| <= (2 |x| + 2) U exp(x), plus 2^-126 absolute for a result below the normal range (the instruction may flush
    it).  c = logistic_f(x) = 1 / (1 + __expf(-x)): the exponential's relative error (2 |x| + 2) U enters with weight e / (1 + e) = 1 - c, the addition
    and the (correctly rounded) division round once each: |d c| <= ((2 |x| + 2) (1 - c) + 2) U c, plus 2^-126.  An overflowing exponential is +inf on
    both sides."""
    _, objs = trained; lst = [objs[n] for n in names]; x = cloud; K = len(lst)
    out = pkg.query_scene_points(lst, x)
    rows = np.stack([pkg.scene_point_rows(lst, x, k) for k in range(K)])
    _same_bits(out, np_fold(rows), names)
    nin = out[4]
    print("%s: points inside 0 / 1 / 2+ boxes: %d / %d / %d; owners %s" % (names, (nin == 0).sum(), (nin == 1).sum(), (nin >= 2).sum(),
                                                                         dict(zip(*np.unique(out[2], return_counts=True)))))
    assert (nin == 1).sum() >= 50 and (nin == 0).sum() >= 50
    if K > 1:                                                                                # (K = 1: no second box and no owner but 0: nothing to ask)
        assert (nin >= 2).sum() >= 50 and (out[2] > 0).sum() >= 50
    assert ((out[2] < 0) == (nin == 0)).all() and (out[0][nin == 0] == 0).all() and (out[1][nin == 0] == 0).all()
    worst = [0.0, 0.0]
    for k in range(K):
        r = rows[k][rows[k][:, 3] != 0]; raw = r[:, 4:8].astype(np.float64)
        assert np.array_equal(_bits(pkg.query_object_points(lst[k], r[:, :3])), _bits(r[:, 4:8])), k
        with np.errstate(over="ignore"):
            want = np.exp(raw[:, 3])
        fin = want <= F32_MAX
        assert np.isinf(r[~fin, 8]).all()
        e = np.abs(r[fin, 8].astype(np.float64) - want[fin]) / ((2 * np.abs(raw[fin, 3]) + 2) * U * want[fin] + TINY)
        c = _logistic64(raw[:, :3])
        ec = np.abs(r[:, 9:12].astype(np.float64) - c) / (((2 * np.abs(raw[:, :3]) + 2) * (1 - c) + 2) * U * c + TINY)
        worst = [max(worst[0], float(e.max())), max(worst[1], float(ec.max()))]
        assert (e <= 1.0).all() and (ec <= 1.0).all(), (k, float(e.max()), float(ec.max()))
    print("activations: largest error / bound  sigma %.3f  colour %.3f" % tuple(worst))


# ---------------------------------------------------------------------------------------------------------------- 6: the lattice
def _span(sc, shape):
    """A world lattice of this shape around the three objects (0.8 x 0.7 x 0.25 either side of their centroid), the y step negative."""
    c = np.mean([ob["Two"][:3, 3] for ob in sc.objects], 0); ext = np.array([0.8, 0.7, 0.25])
    sgn = np.array([1.0, -1.0, 1.0]); n = np.array(shape, np.float64)
    return (c - sgn * ext).astype(np.float32), (sgn * 2 * ext / np.maximum(n - 1, 1)).astype(np.float32)


@pytest.mark.parametrize("shape", [(5, 7, 11), (33, 32, 17)])
def test_lattice_equals_its_points(pkg, scene, trained, shape):
    """mon_scene_query_lattice equals mon_scene_query_points(mon_lattice_points(...)) bit for bit, at 5 x 7 x 11 and at 33 x 32 x 17 (17 952 points: the
    lattice crosses a pass boundary); the steps are of mixed sign.  The lattice spans the three objects."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = _span(scene, shape)
    got = pkg.query_scene_lattice(lst, origin, step, shape)
    xyz = pkg.lattice_points(origin, step, shape)
    _same_bits(got, pkg.query_scene_points(lst, xyz), shape)
    few = 50; big = xyz.shape[0] > CHUNK                                               # (the coarse lattice meets no overlap of two boxes)
    assert (got[4] >= 2).sum() >= (few if big else 0) and (got[4] == 1).sum() >= few and (got[4] == 0).sum() >= few
    assert len(set(np.unique(got[2]))) >= (4 if big else 2)


# ---------------------------------------------------------------------------------------------------------------- 7: geometry
def test_geometry_sanity(pkg, scene, trained):
    """No tuned number: for each trained object, the median sigma at 0.5 x the ellipsoid radii (inside the surface) exceeds the median at 1.5 x the radii
    (outside it, still inside the box); and points at 0.5 x the radii of object k, asked of {a0, a1, a2}, have owner k more often than any other."""
    _, objs = trained; lst = [objs["a0"], objs["a1"], objs["a2"]]
    rng = np.random.RandomState(23)
    for k in range(3):
        ob = scene.objects[k]
        d = rng.normal(size=(4000, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        far = 1.5 * ob["radii"] * d; far = far[(np.abs(far) <= 0.98 * ob["half"]).all(1)]
        assert far.shape[0] >= 200
        s_in = pkg.query_scene_points([lst[k]], _world(scene, k, 0.5 * ob["radii"] * d[:1000]))
        s_out = pkg.query_scene_points([lst[k]], _world(scene, k, far))
        assert (s_in[4] == 1).all() and (s_out[4] == 1).all()
        print("object %d: median sigma inside %.4g, outside %.4g" % (k, np.median(s_in[0]), np.median(s_out[0])))
        assert np.median(s_in[0]) > np.median(s_out[0])
        own = pkg.query_scene_points(lst, _world(scene, k, 0.5 * ob["radii"] * d[:1000]))[2]
        cnt = [(own == j).sum() for j in (-1, 0, 1, 2)]
        assert int(np.argmax(cnt)) - 1 == k, cnt


# ---------------------------------------------------------------------------------------------------------------- 8: online and refusals
def test_online_and_refusals(pkg, ss, scene, trained, cloud):
    """Before any publication mon_online_query_points / _lattice return MON_ERR_STATE; one query from a second thread while the manager's objects still
    train returns finite outputs and no error; once they are idle both forms equal the scene calls on side 1 over the borrowed objects bit for bit, with
    the manager's indices as owners.  A layer-kernel shape (16 neurons) and a fused shape switched to backend 0 are refused with MON_ERR_STATE, an
    unpublished object on side 1 too; an XORWOW object, which the ray routes refuse, is served (nothing is jittered here)."""
    sc = scene; ds, objs = trained
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    x = cloud; origin = x.min(0); shape = (9, 8, 7); step = ((x.max(0) - origin) / (np.array(shape) - 1)).astype(np.float32)
    for call in (lambda: m.query_points(x), lambda: m.query_lattice(origin, step, shape)):
        with pytest.raises(pkg.MonError) as e:
            call()
        assert e.value.code == 5
    seen = dict(n=0, err=None)

    def planner():
        try:
            out = m.query_points(x)
            assert all(np.isfinite(a).all() for a in out) and set(np.unique(out[2])) <= {-1, 0, 1, 2}
            seen["n"] += 1
        except Exception as ex:        # noqa: BLE001 -- reported by the main thread
            seen["err"] = ex

    calls = 100
    ids = tsr._online_feed(pkg, ss, sc, m, 3, calls)
    assert tsr._wait_trained(m, ids, 2)                                                # every object has published
    th = threading.Thread(target=planner); th.start(); th.join(timeout=120)
    still = [m.object_info(i)["train_calls"] for i in ids]
    m.wait_threads_end()
    assert seen["err"] is None and seen["n"] == 1, seen
    print("online: train calls when the query was through:", still)
    assert min(still) < calls                                                           # they were still training
    borrowed = [m.object(i) for i in ids]
    got = m.query_points(x)
    _same_bits(got, pkg.query_scene_points(borrowed, x, side=1), "points, side 1")
    _same_bits(m.query_lattice(origin, step, shape), pkg.query_scene_lattice(borrowed, origin, step, shape, side=1), "lattice, side 1")
    assert set(np.unique(got[2])) == {-1, 0, 1, 2} and (got[4] >= 1).sum() >= 300
    m.close()
    _, c = ge.make_problem(pkg, sc, dict(n_neurons=16), dataset=ds)
    _, b0 = ge.make_problem(pkg, sc, tsr.BASE, dataset=ds); b0.set_backend(0)
    _, xw = ge.make_problem(pkg, sc, dict(tsr.BASE, rng_flags=1), dataset=ds)
    _, fresh = ge.make_problem(pkg, sc, tsr.BASE, obj_index=1, dataset=ds)
    try:
        for lst, side in (([c], 0), ([objs["a0"], c], 0), ([b0], 0), ([objs["a1"], b0], 1), ([fresh], 1), ([objs["a0"], fresh], 1)):
            with pytest.raises(pkg.MonError) as e:
                pkg.query_scene_points(lst, x, side)
            assert e.value.code == 5, (len(lst), side)
            with pytest.raises(pkg.MonError) as e:
                pkg.query_scene_lattice(lst, origin, step, shape, side)
            assert e.value.code == 5, (len(lst), side)
        with pytest.raises(pkg.MonError) as e:
            pkg.query_object_points(c, np.full((4, 3), 0.5, np.float32))
        assert e.value.code == 5
        out = pkg.query_scene_points([objs["a0"], xw], x)
        assert all(np.isfinite(a).all() for a in out)
    finally:
        for o in (c, b0, xw, fresh):
            o.close()
