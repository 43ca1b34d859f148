"""GPU tests (-m gpu) of the shortest-path cost fields (mon_shortest_paths, mon_scene_paths_lattice, mon_online_paths_lattice; the kernels of
kernels_paths.hip).  The field has a unique definition in fp32, so there is no tolerance anywhere: cost is compared as bits and next as integers with
tests/paths_reference.py -- a heap Dijkstra and a whole-lattice Jacobi sweep, pinned against each other by tests/test_paths_abi.py -- or with closed forms
where the lattice is too large for a host reference.  The scene call is held to public calls: its sigma and owner to mon_scene_query_lattice, its dist to
mon_scene_distance_lattice, its field to mon_shortest_paths of the mask and the multiplier derived from that dist.  The scene, the trained objects and the
manager's feed are those of tests/test_scene_render.py; the lattice and the choice of sigma_min those of tests/test_components.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import components_reference as cr
import paths_reference as pr
import test_components as tcomp
import test_scene_render as tsr
from test_scene_render import scene, trained       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu

# The kernel's tile is 32 x 8 x 4 cells (the components tile): 1 x 1 x 1; one line along each axis; lattices with no dimension a multiple of a tile's;
# (45, 19, 11) and (70, 18, 10): every tile dimension straddled unevenly on all three axes
SHAPES = ((1, 1, 1), (37, 1, 1), (1, 41, 1), (1, 1, 29), (19, 23, 17), (33, 31, 29), (45, 19, 11), (70, 18, 10))
# lines of 4 133 cells: 130 / 517 / 1 034 tiles in a row, one sweep per tile crossed: many batches of sweeps
LINES = ((4133, 1, 1), (1, 4133, 1), (1, 1, 4133))
SHARES = (0, "one", 0.5, 0.69, 0.98, 1)
CONNS = (6, 18, 26)
STEPS = ((0.3, 0.7, 1.1), (0.25, 0.5, 0.125), (-0.3, 0.2, -0.45), (0.3, 0.0, 0.2))          # anisotropic, powers of two, negative, one zero
SEEDS = ("one", "three", "blocked", "duplicate")
COSTS = (None, "random", None, "random", "zero", "random")                                  # by share: multipliers in [1, 5], constant 0, or none

_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = got != want
    assert not ne.any(), (what, int(ne.sum()), np.flatnonzero(ne.reshape(-1))[:4], got[ne][:4], want[ne][:4])


def _same_field(got, want, what):
    _same(_bits(got[0]), _bits(want[0]), (what, "cost")); _same(got[1], want[1], (what, "next"))


def _inputs(shape, di, si):
    """mask, seeds, step, multiplier of share di on `shape`, with seed mode and step set number si (both rotate with the share)"""
    key = ("in", shape, di, si)
    if key not in _cache:
        rng = np.random.default_rng(4000 + 100 * di + 10 * si + sum(shape))
        m = pr.random_mask(shape, SHARES[di], seed=1000 * di + sum(shape))
        on = np.flatnonzero(m.reshape(-1)); off = np.flatnonzero(m.reshape(-1) == 0)
        mode = SEEDS[si % 4]
        pick = (lambda k: rng.choice(on, min(k, on.size), replace=False)) if on.size else (lambda k: rng.choice(off, min(k, off.size), replace=False))
        seeds = pick(1) if mode == "one" else pick(3) if mode == "three" else pick(2)
        if mode == "blocked" and off.size:
            seeds = np.concatenate([rng.choice(off, 1), seeds])
        if mode == "duplicate":
            seeds = np.concatenate([seeds, seeds[:1], seeds])
        kind = COSTS[di]
        c = None if kind is None else np.zeros(m.shape, np.float32) if kind == "zero" else (1 + 4 * rng.random(m.shape)).astype(np.float32)
        _cache[key] = (m, seeds.astype(np.int32), np.array(STEPS[si % 4], np.float32), c)
        for a in _cache[key]:
            if a is not None:
                a.setflags(write=False)
    return _cache[key]


def _ref(key, args, conn, solver=pr.jacobi):
    """the reference field of args = (mask, seeds, step, multiplier) under conn, computed once and left unchanged"""
    if (key, conn) not in _cache:
        m, seeds, step, c = args
        _cache[(key, conn)] = pr.field(m, seeds, step, conn, c, solver=solver)
        for a in _cache[(key, conn)]:
            a.setflags(write=False)
    return _cache[(key, conn)]


# ---------------------------------------------------------------------------------------------------------------- 1: random masks against the reference
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_field_equals_the_reference(pkg, shape, conn):
    """mon_shortest_paths equals the reference bit for bit in cost and next at passable shares 0, one cell, 50 %, 69 %, 98 % and all cells; the step sets
    (anisotropic, powers of two, negative, one zero) and the seed sets (one, three, one of them on a blocked cell, duplicates) rotate with the share and
    the connectivity, the multipliers (none, random in [1, 5], constant 0) go with the share.  Constant 0: everything reachable costs 0 and next is -1."""
    for di in range(len(SHARES)):
        si = di + CONNS.index(conn) + SHAPES.index(shape)
        args = _inputs(shape, di, si); m, seeds, step, c = args
        want = _ref(("rnd", shape, di, si), args, conn)
        got = pkg.shortest_paths(m, seeds, step, conn, c)
        _same_field(got, want, (shape, conn, SHARES[di], SEEDS[si % 4], STEPS[si % 4]))
        if COSTS[di] == "zero":
            assert (got[0][np.isfinite(got[0])] == 0).all() and (got[1] == -1).all() and np.isfinite(got[0]).sum() >= 1
    if SHARES[0] == 0:
        assert np.isinf(pkg.shortest_paths(*_inputs(shape, 0, 0)[:3], conn)[0]).all()       # nothing passable: every seed lies on a blocked cell


@pytest.mark.parametrize("shape", LINES)
def test_lines_across_many_tiles(pkg, shape):
    """4 133 cells in a row, all passable, one seed near an end and one in the middle: the field crosses every tile of the line, one per sweep, in many
    batches of sweeps.  With every 5th cell but those of a stretch blocked under 26-connectivity nothing leaves the stretch."""
    n = 4133; step = np.array(STEPS[0], np.float32)
    m = np.ones(shape[::-1], np.uint8)
    tiles = {0: 130, 1: 517, 2: 1034}[shape.index(n)]
    for conn, seeds in ((6, [3]), (26, [n // 2, n - 1])):
        args = (m, np.array(seeds, np.int32), step, None)
        _same_field(pkg.shortest_paths(m, seeds, step, conn), _ref(("line", shape, tuple(seeds)), args, conn, pr.dijkstra), (shape, conn))
        if conn == 6:                                                              # from one end: every tile of the line in turn
            sweeps, batches, busy = pkg.paths_stats()
            print("%s: %d sweeps enqueued in %d batches, %d left work" % (shape, sweeps, batches, busy))
            assert busy >= tiles - 1 and sweeps > busy and batches >= 2, (sweeps, batches, busy)
    cut = m.copy(); cut.reshape(-1)[::5] = 0; cut.reshape(-1)[2000:2300] = 1
    rng = np.random.default_rng(5); c = (1 + 4 * rng.random(cut.shape)).astype(np.float32)
    args = (cut, np.array([2100], np.int32), step, c)
    got = pkg.shortest_paths(cut, [2100], step, 26, c)
    _same_field(got, _ref(("line cut", shape), args, 26, pr.dijkstra), (shape, "cut"))
    assert np.isfinite(got[0]).sum() == 300 + 4                                    # the stretch and the four cells that join it (1996 .. 1999: 1995 is blocked)


# ---------------------------------------------------------------------------------------------------------------- 2: max_cost
def test_max_cost(pkg):
    """max_cost below one step (only the seeds survive), at a cost of the field (that cell keeps its value and its next) and large (nothing is cut): the
    reference's cut of the untruncated field, bit for bit."""
    shape = (33, 31, 29); conn = 18
    args = _inputs(shape, 3, 1); m, seeds, step, c = args
    cost, nxt = _ref(("rnd", shape, 3, 1), args, conn)
    fin = np.sort(cost[np.isfinite(cost) & (cost > 0)])
    assert fin.size > 1000
    at = float(fin[fin.size // 2])
    for mc in (float(fin[0]) * 0.5, at, 1e30):
        got = pkg.shortest_paths(m, seeds, step, conn, c, max_cost=mc)
        _same_field(got, pr.truncate(cost, nxt, mc), ("max_cost", mc))
    got = pkg.shortest_paths(m, seeds, step, conn, c, max_cost=at)
    assert (got[0] == np.float32(at)).sum() >= 1 and np.isinf(got[0][cost > np.float32(at)]).all() and np.isfinite(got[0]).sum() < np.isfinite(cost).sum()
    only = pkg.shortest_paths(m, seeds, step, conn, c, max_cost=float(fin[0]) * 0.5)
    assert np.isfinite(only[0]).sum() == np.unique(seeds).size


# ---------------------------------------------------------------------------------------------------------------- 3: the serpentine
def test_serpentine(pkg):
    """One 6-connected path of 11 627 cells through 37 x 35 x 33 that crosses tile borders thousands of times -- the stated worst case for the number of
    sweeps -- against the Dijkstra reference, under 6 with an anisotropic step and under 26 (the diagonals cut the bends) with multipliers."""
    shape = (37, 35, 33)
    m = cr.serpentine(shape); assert int(m.sum()) == 11627
    rng = np.random.default_rng(9); c = (1 + 4 * rng.random(m.shape)).astype(np.float32)
    for conn, cc in ((6, None), (26, c)):
        args = (m, np.array([0], np.int32), np.array(STEPS[0], np.float32), cc)
        want = _ref(("serpentine", conn), args, conn, pr.dijkstra)
        got = pkg.shortest_paths(m, [0], STEPS[0], conn, cc)
        _same_field(got, want, ("serpentine", conn))
        print("serpentine under %d: sweeps enqueued, batches, sweeps that left work = %s" % (conn, pkg.paths_stats()))
    want6 = _cache[(("serpentine", 6), 6)]
    far = int(np.argmax(np.where(np.isfinite(want6[0]), want6[0], -1)))
    assert len(pr.follow(want6[1], far)) == 11627                                   # under 6 the way back from the far end is the whole path


# ---------------------------------------------------------------------------------------------------------------- 4: 2^22 cells, closed forms only
BIG = (256, 128, 128)


def test_largest_lattice(pkg):
    """256 x 128 x 128 = 2^22 cells, 6-connected, steps 0.5 / 0.25 / 0.125 (every sum exact), seed at cell 0.  All passable: cost = i sx + j sy + k sz and
    next the -z, else -y, else -x neighbour.  With the plane i = 128 blocked but for one hole: in front of the wall the same, behind it the cost to the
    hole plus the cost from it."""
    nx, ny, nz = BIG; step = np.array([0.5, 0.25, 0.125], np.float32)
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.int32), np.arange(ny, dtype=np.int32), np.arange(nx, dtype=np.int32), indexing="ij", sparse=True)
    m = np.ones((nz, ny, nx), np.uint8)
    cost, nxt = pkg.shortest_paths(m, [0], step, 6)
    open_cost = (i * np.float32(0.5) + j * np.float32(0.25) + k * np.float32(0.125)).astype(np.float32)
    _same(_bits(cost), _bits(open_cost), "cost")
    flat = (k * ny + j) * nx + i
    _same(nxt, np.where(k > 0, flat - nx * ny, np.where(j > 0, flat - nx, np.where(i > 0, flat - 1, -1))).astype(np.int32), "next")
    hj, hk = 77, 101
    w = pr.wall_with_hole(BIG, 128, (hj, hk))
    cost, _ = pkg.shortest_paths(w, [0], step, 6)
    to_hole = np.float32(128 * 0.5 + hj * 0.25 + hk * 0.125)
    behind = (to_hole + (abs(i - 128) * np.float32(0.5) + abs(j - hj) * np.float32(0.25) + abs(k - hk) * np.float32(0.125))).astype(np.float32)
    want = np.where(i < 128, open_cost, behind); want[:, :, 128] = np.inf; want[hk, hj, 128] = to_hole
    _same(_bits(cost), _bits(want), "cost behind the wall")


# ---------------------------------------------------------------------------------------------------------------- 5: call hygiene
_CHILD = """
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as ge, paths_reference as pr
pkg = ge.load_package()
m = pr.random_mask((19, 23, 17), 0.69, seed=77); rng = np.random.default_rng(78); c = (1 + 4 * rng.random(m.shape)).astype(np.float32)
cost, nxt = pkg.shortest_paths(m, [int(np.flatnonzero(m.reshape(-1))[5])], (0.3, 0.7, 1.1), 26, c)
np.save(sys.argv[1], cost); np.save(sys.argv[2], nxt)
"""


def test_call_hygiene(pkg, tmp_path):
    """next NULL leaves cost unchanged, and nothing is written behind the lattice; any non-zero byte counts as passable; two calls give equal bits; a
    smaller call after a larger one gives the bits of a fresh process's call."""
    L = pkg.lib(); shape = (19, 23, 17); nx, ny, nz = shape
    m = pr.random_mask(shape, 0.69, seed=77); rng = np.random.default_rng(78); c = (1 + 4 * rng.random(m.shape)).astype(np.float32)
    seed = int(np.flatnonzero(m.reshape(-1))[5]); step = np.array([0.3, 0.7, 1.1], np.float32)
    a = pkg.shortest_paths(m, [seed], step, 26, c)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    big = np.concatenate([m.reshape(-1) * np.uint8(200), np.full(5000, 1, np.uint8)]); sd = np.array([seed], np.int32)
    cost = np.full(m.size + 64, 7.0, np.float32)
    assert L.mon_shortest_paths(0, vp(big), nx, ny, nz, vp(step), 26, vp(c), vp(sd), 1, float("inf"), vp(cost), None) == 0
    _same(_bits(cost[:m.size]), _bits(a[0]).reshape(-1), "cost alone"); assert (cost[m.size:] == 7.0).all()
    other = pkg.shortest_paths(cr.serpentine((45, 19, 11)), [0], step, 6)            # a larger call of another kind in between
    assert np.isfinite(other[0]).sum() == int(cr.serpentine((45, 19, 11)).sum())
    b = pkg.shortest_paths(m, [seed], step, 26, c)
    _same_field(b, a, "twice")
    f_cost, f_next = str(tmp_path / "cost.npy"), str(tmp_path / "next.npy")
    code = _CHILD % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code, f_cost, f_next], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _same_field(b, (np.load(f_cost), np.load(f_next)), "a fresh process")


# ---------------------------------------------------------------------------------------------------------------- 6: the scene call
SHAPE = tcomp.SHAPE


def _pick_clearance(pkg, dist):
    """A clearance, a seed and the share of passable cells the seed cannot reach under 6-connectivity, such that the reference itself leaves both
    reachable and unreachable passable cells: among 0.2 and distances of the field, the first whose mask dist > clearance has at least two components
    (mon_label_components); the seed lies in the largest.  Asserted: the test cannot pass vacuously."""
    nx, ny, nz = SHAPE
    pos = np.unique(dist[np.isfinite(dist) & (dist > 0)])
    for clr in [0.2] + [float(pos[int(q * (pos.size - 1))]) for q in (0.3, 0.2, 0.4, 0.1, 0.5, 0.6, 0.05, 0.7)]:
        mask = (dist > np.float32(clr)).reshape(nz, ny, nx)
        if not mask.any():
            continue
        label, comp, table, n = pkg.label_components(mask, 6)
        if n >= 2:
            big = int(np.argmax(table["cells"]))
            return clr, int(table["rep"][big]), int(mask.sum()) - int(table["cells"][big])
    raise AssertionError("no clearance tried leaves the passable cells in at least 2 components")


def _check_scene(pkg, call, query, distance, step, what):
    """`call(sigma_min, clearance, soft_radius, soft_weight, connectivity, seeds, max_cost, rows)` = the paths call; `query()` the lattice query and
    `distance(sigma_min)` the distance call over the same objects: cost and next equal mon_shortest_paths of the mask dist > clearance and of the multiplier
    formed in numpy fp32 from that dist by the header's formula; the optional rows are those calls' bits."""
    nx, ny, nz = SHAPE; F = np.float32
    sigma, _, owner, _, _ = query()
    smin, occ = tcomp._pick_sigma_min(sigma)
    dist = distance(smin)
    clr, seed, cut_off = _pick_clearance(pkg, dist)
    mask = (dist > F(clr)).reshape(nz, ny, nx)
    radius = float(np.float32(0.5) * (np.float32(clr) + dist[np.isfinite(dist)].max()))      # halfway between the clearance and the largest distance
    assert radius > clr
    print("%s: sigma_min %.5g, clearance %.4g: %d of %d cells passable, %d of them cut off from the seed; soft radius %.4g" %
          (what, smin, clr, int(mask.sum()), mask.size, cut_off, radius))
    seeds = np.array([seed, seed, int(np.flatnonzero(~mask.reshape(-1))[0])], np.int32)      # a duplicate and a seed on a blocked cell
    for sw, conn, mc in ((0.0, 6, np.inf), (2.5, 6, np.inf), (1.5, 26, np.inf), (2.5, 18, None)):
        c = None
        if sw > 0:
            with np.errstate(invalid="ignore"):
                c = (F(1) + F(sw) * (np.maximum(F(0), F(radius) - dist) / F(radius))).astype(F).reshape(mask.shape)
            assert c.dtype == F and (c >= 1).all() and (c[mask] > 1).any() and (c == 1).any()
        if mc is None:                                                             # a cost of the field, from the middle of those that occur
            full = pkg.shortest_paths(mask, seeds, step, conn, c)[0]
            mc = float(np.sort(full[np.isfinite(full)])[np.isfinite(full).sum() // 2])
        want = pkg.shortest_paths(mask, seeds, step, conn, c, max_cost=mc)
        cost, nxt, rows = call(smin, clr, radius, sw, conn, seeds, mc, ("dist", "sigma", "owner"))
        _same_field((cost, nxt), (want[0].reshape(-1), want[1].reshape(-1)), (what, sw, conn, mc))
        _same(_bits(rows["dist"]), _bits(dist), (what, "dist")); _same(_bits(rows["sigma"]), _bits(sigma), (what, "sigma")); _same(rows["owner"], owner, (what, "owner"))
        if conn == 6 and np.isinf(mc):
            reach = np.isfinite(cost)
            assert int(mask.sum()) - int(reach.sum()) == cut_off > 0 and reach.sum() > 1, (what, "both reachable and unreachable passable cells")
            goal = int(np.argmax(np.where(reach, cost, -1)))
            path = pkg.lattice_path(nxt, goal)
            assert path[0] == goal and path[-1] == seed and (np.diff(cost[path]) < 0).all() and mask.reshape(-1)[path].all()
    alone = call(smin, clr, radius, 2.5, 6, seeds, np.inf, ())
    assert alone[2] == {}
    _same_field(alone[:2], call(smin, clr, radius, 2.5, 6, seeds, np.inf, ("owner",))[:2], (what, "without rows"))
    return smin, clr, radius, seeds


@pytest.mark.parametrize("side", [0, 1])
def test_scene_call(pkg, scene, trained, side):
    """On the 24 x 20 x 18 lattice around the three objects, sides 0 and 1: the field equals mon_shortest_paths of the mask and multiplier formed from the
    public distance call, with soft_weight 0 and > 0, at a clearance that cuts passable cells off from the seed; the optional rows equal the public
    calls' bits; every optional output NULL leaves cost unchanged; a smaller call after a larger one in the same workspace gives the standalone call's
    bits."""
    L = pkg.lib(); _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = tcomp._enclosing(scene, SHAPE)

    def call(smin, clr, sr, sw, conn, seeds, mc, rows):
        return pkg.scene_paths_lattice(lst, origin, step, SHAPE, smin, seeds, clr, sr, sw, conn, mc, side=side, rows=rows)
    smin, clr, radius, seeds = _check_scene(pkg, call, lambda: pkg.query_scene_lattice(lst, origin, step, SHAPE, side),
                                            lambda s: pkg.scene_distance_lattice(lst, origin, step, SHAPE, s, side=side, free=False)[0], step, "side %d" % side)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]; cost = np.empty(n, np.float32); hs = (C.c_void_p * 3)(*[o.h for o in lst])
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.mon_scene_paths_lattice(hs, 3, side, vp(origin), vp(step), *SHAPE, smin, clr, radius, 2.5, 6, vp(seeds), seeds.size, float("inf"), vp(cost),
                                     None, None, None, None) == 0
    _same(_bits(cost), _bits(call(smin, clr, radius, 2.5, 6, seeds, np.inf, ())[0]), "cost with every optional output NULL")
    pkg.scene_paths_lattice(lst, origin, step * np.float32(0.5), (40, 33, 30), smin, [0], 0.0, 0.1, 1.0, 26, side=side, rows=("dist", "owner"))   # the buffers grow
    small = (5, 4, 3)
    got = pkg.scene_paths_lattice(lst, origin, step * np.float32(4), small, smin, [0, 59], 0.0, radius, 1.0, 18, side=side, rows=("dist",))
    d = got[2]["dist"]; F = np.float32
    c = (F(1) + F(1.0) * (np.maximum(F(0), F(radius) - d) / F(radius))).astype(F).reshape(small[::-1])
    want = pkg.shortest_paths((d > 0).reshape(small[::-1]), [0, 59], step * np.float32(4), 18, c)
    _same_field(got[:2], (want[0].reshape(-1), want[1].reshape(-1)), "a smaller call after a larger one")


def test_online_call(pkg, ss, scene, trained):
    """Before any publication mon_online_paths_lattice returns MON_ERR_STATE; once the manager's objects are idle it equals the scene call on side 1 over
    the borrowed objects bit for bit, owner holding the manager's indices (here the list's own), and meets the scene call's checks."""
    sc = scene
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    origin, step = tcomp._enclosing(sc, SHAPE)
    with pytest.raises(pkg.MonError) as e:
        m.paths_lattice(origin, step, SHAPE, 1.0, [0])
    assert e.value.code == 5
    ids = tsr._online_feed(pkg, ss, sc, m, 3, 20)
    assert tsr._wait_trained(m, ids, 2)
    m.wait_threads_end()
    borrowed = [m.object(i) for i in ids]

    def call(smin, clr, sr, sw, conn, seeds, mc, rows):
        got = m.paths_lattice(origin, step, SHAPE, smin, seeds, clr, sr, sw, conn, mc, rows=rows)
        want = pkg.scene_paths_lattice(borrowed, origin, step, SHAPE, smin, seeds, clr, sr, sw, conn, mc, side=1, rows=rows)
        assert set(got[2]) == set(want[2]) == set(rows)
        _same_field(got[:2], want[:2], ("online", sw, conn))
        for k in rows:
            _same(got[2][k].view(np.uint32), want[2][k].view(np.uint32), ("online", k, conn))
        return got
    _check_scene(pkg, call, lambda: m.query_lattice(origin, step, SHAPE), lambda s: m.distance_lattice(origin, step, SHAPE, s, free=False)[0], step, "online")
    m.close()


# ---------------------------------------------------------------------------------------------------------------- 7: the existing routes
def test_existing_routes_keep_their_bits(pkg, scene, trained):
    """The lattice query's five outputs, the gradients', the distance call's and the components call's after paths calls of other sizes in the same
    side's workspace are the bits from before them: the shared workspace is not disturbed."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = tcomp._enclosing(scene, SHAPE)
    for side in (0, 1):
        before = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)
        xyz = pkg.lattice_points(origin, step, SHAPE)[::7]
        g_before = pkg.query_scene_gradients(lst, xyz, side=side)
        smin = float(np.percentile(before[0], 90.0, method="lower"))
        d_before = pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=side)
        c_before = pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 1, 0.05, 18, side=side, rows=("dist", "owner"))
        pkg.scene_paths_lattice(lst, origin, step, SHAPE, smin, [0], side=side)
        pkg.scene_paths_lattice(lst, origin, step * np.float32(0.5), (40, 33, 30), smin, [0, 5], 0.05, 0.2, 2.0, 26, side=side, rows=("dist", "sigma", "owner"))
        pkg.scene_paths_lattice(lst, origin, step, (5, 4, 3), smin, [59], 0.0, 0.1, 1.0, 6, 0.5, side=side)
        after = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)
        for b, a, name in zip(before, after, ("sigma", "rgb", "owner", "owner_sigma", "n_inside")):
            _same(a.view(np.uint32), b.view(np.uint32), ("lattice query", name, side))
        for b, a in zip(g_before, pkg.query_scene_gradients(lst, xyz, side=side)):
            _same(a.view(np.uint32), b.view(np.uint32), ("gradients", side))
        for b, a, name in zip(d_before, pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=side), ("dist", "nearest", "owner", "free", "sigma")):
            _same(a.view(np.uint32), b.view(np.uint32), ("distance call", name, side))
        c_after = pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 1, 0.05, 18, side=side, rows=("dist", "owner"))
        for b, a, name in zip(c_before[:3], c_after[:3], ("label", "comp", "table")):
            _same(a, b, ("components call", name, side))
        assert c_before[3] == c_after[3]
        for k in ("dist", "owner"):
            _same(c_after[4][k].view(np.uint32), c_before[4][k].view(np.uint32), ("components call", k, side))
