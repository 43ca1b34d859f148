"""GPU tests (-m gpu) of the connected components (mon_label_components, mon_scene_components_lattice, mon_online_components_lattice; the kernels of
kernels_components.hip).  The result is pure integers with a unique definition, so there is no tolerance anywhere: label, comp, n_components and the table
equal tests/components_reference.py -- a sequential flood fill, pinned on its own by tests/test_components_abi.py -- bit for bit, or closed forms where
the lattice is too large for a host reference.  The scene call is held to public calls: its sigma to mon_scene_query_lattice, its dist to
mon_scene_distance_lattice, its components to mon_label_components of the mask derived from them.  The scene, the trained objects and the manager's
feed are those of tests/test_scene_render.py."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import components_reference as cr
import test_scene_render as tsr
from test_scene_render import scene, trained       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu

# The kernel's tile is 32 x 8 x 4 cells.  1 x 1 x 1; one line along each axis; two lattices with no dimension a multiple of a tile's; three lines that
# cross 130 / 517 / 1 034 tiles; (45, 19, 11) = 32 + 13, 2 * 8 + 3, 2 * 4 + 3 and (70, 18, 10): every tile dimension straddled unevenly on all three axes
SHAPES = ((1, 1, 1), (37, 1, 1), (1, 41, 1), (1, 1, 29), (19, 23, 17), (33, 31, 29), (4133, 3, 2), (3, 4133, 2), (2, 3, 4133), (45, 19, 11), (70, 18, 10))
DENSITIES = (0, "one", 0.02, 0.31, 0.5, 1)
CONNS = (6, 18, 26)

_cache = {}


def _ref(key, make, conn):
    """the reference of the mask make() under conn, computed once and left unchanged"""
    if (key, conn) not in _cache:
        if key not in _cache:
            _cache[key] = make()
        _cache[(key, conn)] = cr.components(_cache[key], conn)
        for a in _cache[(key, conn)][:3]:
            a.setflags(write=False)
    return (_cache[key],) + _cache[(key, conn)]


def _random(shape, di, conn):
    return _ref((shape, di), lambda: cr.random_mask(shape, DENSITIES[di], seed=1000 * di + sum(shape)), conn)


def _same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    ne = got != want
    assert not ne.any(), (what, int(ne.sum()), got[ne][:4], want[ne][:4])


def _equals_reference(pkg, m, want, conn, what):
    label, comp, table, n = pkg.label_components(m, conn)
    assert n == want[3], (what, n, want[3])
    _same(label, want[0], (what, "label")); _same(comp, want[1], (what, "comp")); _same(table, want[2], (what, "table"))


# ---------------------------------------------------------------------------------------------------------------- 1: random masks against the reference
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_labelling_equals_the_reference(pkg, shape, conn):
    """mon_label_components equals the flood fill bit for bit in label, comp, n_components and the table, at densities 0, one cell, 2 %, 31 %, 50 % and all
    cells (1 x 1 x 1: outside and inside the mask).  All cells of a 4 133-cell line: one component across every tile of the line."""
    for di in range(len(DENSITIES)):
        m, *want = _random(shape, di, conn)
        _equals_reference(pkg, m, want, conn, (shape, conn, DENSITIES[di]))
    assert _random(shape, 0, conn)[4] == 0 and _random(shape, 1, conn)[4] == 1
    m, label, comp, table, n = _random(shape, 5, conn)
    assert n == 1 and table[0]["cells"] == m.size and table[0]["hi"].tolist() == [shape[0] - 1, shape[1] - 1, shape[2] - 1] and (label == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 2: the named masks
@pytest.mark.parametrize("shape", [(10, 9, 8), (45, 19, 11)])
def test_checkerboard(pkg, shape):
    """(i + j + k) % 2 == 0: under 6 every mask cell is its own component; under 18 and 26 there is exactly one.  And the reference, bit for bit."""
    key = ("checkerboard", shape)
    for conn in CONNS:
        m, *want = _ref(key, lambda: cr.checkerboard(shape), conn)
        _equals_reference(pkg, m, want, conn, (key, conn))
        label, comp, table, n = pkg.label_components(m, conn)
        if conn == 6:
            assert n == int(m.sum()) and (label[m != 0] == np.flatnonzero(m.reshape(-1))).all() and (table["cells"] == 1).all()
        else:
            assert n == 1 and table[0]["rep"] == 0 and table[0]["cells"] == int(m.sum())


@pytest.mark.parametrize("shape", [(37, 35, 33), (45, 19, 11), (70, 18, 10)])
def test_serpentine(pkg, shape):
    """One 6-connected path through the whole lattice that crosses every tile border many times (37 x 35 x 33: 11 627 cells, eccentricity 11 626 from
    cell 0): one component, rep 0, under every connectivity; the reference, bit for bit."""
    key = ("serpentine", shape)
    for conn in CONNS:
        m, *want = _ref(key, lambda: cr.serpentine(shape), conn)
        assert want[3] == 1
        _equals_reference(pkg, m, want, conn, (key, conn))
        label, comp, table, n = pkg.label_components(m, conn)
        assert n == 1 and table[0]["rep"] == 0 and table[0]["cells"] == int(m.sum()) and (label[m != 0] == 0).all() and (comp[m != 0] == 0).all()
    if shape == (37, 35, 33):
        assert int(_cache[key].sum()) == 11627


# ---------------------------------------------------------------------------------------------------------------- 3: 2^22 cells, closed forms only
BIG = (256, 128, 128)


def _raw(pkg, m, conn, cap, table_words, fill=-77):
    """the C call with a table of table_words int32 prefilled with `fill`: (label, comp, table words, n_components)"""
    nz, ny, nx = m.shape
    label = np.empty(m.size, np.int32); comp = np.empty(m.size, np.int32); table = np.full(table_words, fill, np.int32); n = C.c_uint32(0xdead)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert pkg.lib().mon_label_components(0, vp(m), nx, ny, nz, conn, vp(label), vp(comp), vp(table), cap, C.byref(n)) == 0
    return label, comp, table, n.value


def test_largest_lattice_all_cells(pkg):
    """256 x 128 x 128 = 2^22 cells, all in the mask: one component, rep 0, 2^22 cells, the lattice as its box; label and comp 0 everywhere."""
    nx, ny, nz = BIG
    m = np.ones((nz, ny, nx), np.uint8)
    for conn in (6, 26):
        label, comp, table, n = _raw(pkg, m, conn, 4, 64)
        assert n == 1 and not label.any() and not comp.any()
        assert table[:8].tolist() == [0, 1 << 22, 0, 0, 0, nx - 1, ny - 1, nz - 1] and (table[8:] == -77).all()


def test_largest_lattice_checkerboard(pkg):
    """The 2^22-cell checkerboard: under 6, 2^21 components, every label its own index, comp the cell's rank among the mask cells, and with cap = 1 000
    the table is cut: 1 000 records of one cell each, the words behind them untouched.  Under 26: one component of 2^21 cells."""
    nx, ny, nz = BIG
    m = cr.checkerboard(BIG); flat = m.reshape(-1) != 0; idx = np.flatnonzero(flat).astype(np.int32)
    label, comp, table, n = _raw(pkg, m, 6, 1000, 8 * 1000 + 4096)
    assert n == 1 << 21 == idx.size
    _same(label, np.where(flat, np.arange(m.size, dtype=np.int32), np.int32(-1)), "label")
    _same(comp[flat], np.arange(idx.size, dtype=np.int32), "comp"); assert (comp[~flat] == -1).all()
    rec = table[:8000].reshape(1000, 8); r = idx[:1000]
    ijk = np.stack([r % nx, (r // nx) % ny, r // (nx * ny)], axis=1).astype(np.int32)
    _same(rec[:, 0], r, "rep"); assert (rec[:, 1] == 1).all()
    _same(rec[:, 2:5], ijk, "lo"); _same(rec[:, 5:8], ijk, "hi")
    assert (table[8000:] == -77).all()
    label, comp, table, n = _raw(pkg, m, 26, 1000, 64)
    assert n == 1 and (label[flat] == 0).all() and (label[~flat] == -1).all() and (comp[flat] == 0).all() and (comp[~flat] == -1).all()
    assert table[:8].tolist() == [0, 1 << 21, 0, 0, 0, nx - 1, ny - 1, nz - 1] and (table[8:] == -77).all()


# ---------------------------------------------------------------------------------------------------------------- 4: cap, optional outputs, determinism
def test_cap_optional_outputs_and_determinism(pkg):
    """cap 0, below, equal to and above n_components: n_components is the total, the records below min(n_components, cap) equal the reference's, nothing
    behind them is written.  With comp, table and n_components NULL, label has the same bits.  Two calls, and a call after one of another size, give equal
    bits; any non-zero byte counts as in the mask, and nothing is read or written behind the lattice."""
    L = pkg.lib(); shape = (19, 23, 17); nx, ny, nz = shape
    m, label, comp, table, n = _random(shape, 3, 6)
    assert n > 40
    want = table.view(np.int32).reshape(-1, 8)
    for cap in (0, n - 3, n, n + 5):
        got = _raw(pkg, m, 6, cap, 8 * (n + 16))
        used = min(n, cap)
        assert got[3] == n, cap
        _same(got[0].reshape(m.shape), label, ("label", cap)); _same(got[1].reshape(m.shape), comp, ("comp", cap))
        _same(got[2][:8 * used].reshape(-1, 8), want[:used], ("table", cap)); assert (got[2][8 * used:] == -77).all(), cap
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    big = np.concatenate([m.reshape(-1) * np.uint8(200), np.full(5000, 1, np.uint8)])
    lab = np.full(m.size + 64, 7, np.int32)
    assert L.mon_label_components(0, vp(big), nx, ny, nz, 6, vp(lab), None, None, 0, None) == 0
    _same(lab[:m.size].reshape(m.shape), label, "label alone"); assert (lab[m.size:] == 7).all()
    a = pkg.label_components(m, 18)
    other = pkg.label_components(cr.serpentine((45, 19, 11)), 18); assert other[3] == 1
    b = pkg.label_components(m, 18)
    for x, y, name in zip(a, b, ("label", "comp", "table")):
        _same(x, y, (name, "twice"))
    assert a[3] == b[3] == _random(shape, 3, 18)[4]
    cut = pkg.label_components(m, 6, cap=5)
    assert cut[3] == n and cut[2].size == 5
    _same(cut[2], table[:5], "the binding's cut table")


# ---------------------------------------------------------------------------------------------------------------- 5: the scene call
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


def _pick_sigma_min(sigma):
    """Among the 90th, 80th, 95th, 70th and 60th percentile of the lattice query's own sigma (each one of its values): the first that leaves between 2 %
    and 50 % of the cells occupied, in at least 2 components under 6-connectivity by the host reference.  Asserted: the test cannot pass vacuously."""
    nx, ny, nz = SHAPE; n = nx * ny * nz
    for pct in (90.0, 80.0, 95.0, 70.0, 60.0):
        smin = float(np.percentile(sigma, pct, method="lower"))
        occ = ~(sigma <= np.float32(smin)); n_occ = int(occ.sum())
        if smin >= 0 and 0.02 * n <= n_occ <= 0.5 * n and cr.components(occ.reshape(nz, ny, nx), 6)[3] >= 2:
            return smin, occ.reshape(nz, ny, nx)
    raise AssertionError("no percentile of sigma gives 2 % to 50 % occupied cells in at least 2 components")


def _check_scene(pkg, call, query, distance, what):
    """`call(sigma_min, region, clearance, connectivity, rows)` = the components call; `query()` the lattice query and `distance(sigma_min)` the distance
    call over the same objects: region 0 equals mon_label_components of the mask formed from the query's sigma, region 1 that of dist > clearance with the
    distance call's untruncated dist; the optional rows are those calls' bits."""
    nx, ny, nz = SHAPE; n_cells = nx * ny * nz
    sigma, _, owner, _, _ = query()
    smin, occ = _pick_sigma_min(sigma)
    print("%s: sigma_min %.5g, %d of %d cells occupied" % (what, smin, int(occ.sum()), n_cells))
    for conn in (6, 26):
        label, comp, table, n, rows = call(smin, 0, 0.0, conn, ("sigma", "owner"))
        wl, wc, wt, wn = pkg.label_components(occ, conn)
        assert n == wn and (conn != 6 or n >= 2), (what, conn, n, wn)
        _same(label, wl.reshape(-1), (what, "label", conn)); _same(comp, wc.reshape(-1), (what, "comp", conn)); _same(table, wt, (what, "table", conn))
        _same(rows["sigma"].view(np.uint32), sigma.view(np.uint32), (what, "sigma")); _same(rows["owner"], owner, (what, "owner"))
        assert set(rows) == {"sigma", "owner"}
    alone = call(smin, 0, 0.0, 6, ())
    assert alone[4] == {}
    _same(alone[0], call(smin, 0, 0.0, 6, ("owner",))[0], (what, "label without rows"))
    dist = distance(smin)
    free = dist > 0; pos = np.unique(dist[free])
    clearance = float(pos[len(pos) // 2])                                          # a distance of the field, from the middle of those that occur
    for clr, conn in ((0.0, 6), (clearance, 6), (clearance, 18)):
        mask = (dist > np.float32(clr)).reshape(nz, ny, nx)
        if clr == 0.0:
            assert np.array_equal(mask.reshape(-1), ~occ.reshape(-1))              # clearance 0: exactly the free cells
        else:
            assert 0 < int(mask.sum()) < int(free.sum()), (what, clr)              # neither empty nor all free cells
        label, comp, table, n, rows = call(smin, 1, clr, conn, ("dist", "sigma", "owner"))
        wl, wc, wt, wn = pkg.label_components(mask, conn)
        print("%s: region 1, clearance %.4g, connectivity %d: %d of %d cells in %d components" % (what, clr, conn, int(mask.sum()), n_cells, wn))
        assert n == wn >= 1, (what, clr, conn, n, wn)
        _same(label, wl.reshape(-1), (what, "label", clr, conn)); _same(comp, wc.reshape(-1), (what, "comp", clr, conn)); _same(table, wt, (what, "table", clr))
        _same(rows["dist"].view(np.uint32), dist.view(np.uint32), (what, "dist")); _same(rows["sigma"].view(np.uint32), sigma.view(np.uint32), (what, "sigma"))
        _same(rows["owner"], owner, (what, "owner"))
    only = call(smin, 1, clearance, 6, ("dist",))
    assert set(only[4]) == {"dist"}
    _same(only[4]["dist"].view(np.uint32), dist.view(np.uint32), (what, "dist alone"))
    return smin, clearance


@pytest.mark.parametrize("side", [0, 1])
def test_scene_call(pkg, scene, trained, side):
    """On a 24 x 20 x 18 lattice around the three objects, sides 0 and 1: regions 0 and 1 equal mon_label_components of the masks formed from the public
    lattice query and distance call, the optional rows equal those calls' bits, and every optional output NULL leaves label unchanged."""
    L = pkg.lib(); _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = _enclosing(scene, SHAPE)

    def call(smin, region, clr, conn, rows):
        return pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, region, clr, conn, side=side, rows=rows)
    smin, clearance = _check_scene(pkg, call, lambda: pkg.query_scene_lattice(lst, origin, step, SHAPE, side),
                                   lambda s: pkg.scene_distance_lattice(lst, origin, step, SHAPE, s, side=side, free=False)[0], "side %d" % side)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]; lab = np.empty(n, np.int32); hs = (C.c_void_p * 3)(*[o.h for o in lst])
    vp = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    for region in (0, 1):
        assert L.mon_scene_components_lattice(hs, 3, side, vp(origin), vp(step), *SHAPE, smin, region, clearance, 6, vp(lab), None, None, 0, None,
                                              None, None, None) == 0
        _same(lab, call(smin, region, clearance, 6, ())[0], ("label with every optional output NULL", region))
    cut = pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 0, 0.0, 6, side=side, cap=1)
    full = call(smin, 0, 0.0, 6, ())
    assert cut[3] == full[3] >= 2 and cut[2].size == 1
    _same(cut[2], full[2][:1], "cap 1")


# ---------------------------------------------------------------------------------------------------------------- 6: the online call
def test_online_call(pkg, ss, scene, trained):
    """Before any publication mon_online_components_lattice returns MON_ERR_STATE; once the manager's objects are idle it equals the scene call on side 1
    over the borrowed objects bit for bit, owner holding the manager's indices (here the list's own), and meets the scene call's checks."""
    sc = scene
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    origin, step = _enclosing(sc, SHAPE)
    with pytest.raises(pkg.MonError) as e:
        m.components_lattice(origin, step, SHAPE, 1.0)
    assert e.value.code == 5
    ids = tsr._online_feed(pkg, ss, sc, m, 3, 20)
    assert tsr._wait_trained(m, ids, 2)
    m.wait_threads_end()
    borrowed = [m.object(i) for i in ids]

    def call(smin, region, clr, conn, rows):
        got = m.components_lattice(origin, step, SHAPE, smin, region, clr, conn, rows=rows)
        want = pkg.scene_components_lattice(borrowed, origin, step, SHAPE, smin, region, clr, conn, side=1, rows=rows)
        assert got[3] == want[3] and set(got[4]) == set(want[4]) == set(rows)
        for g, w, name in zip(got[:3], want[:3], ("label", "comp", "table")):
            _same(g, w, ("online", name, region, conn))
        for k in rows:
            _same(got[4][k].view(np.uint32), want[4][k].view(np.uint32), ("online", k, region, conn))
        return got
    _check_scene(pkg, call, lambda: m.query_lattice(origin, step, SHAPE),
                 lambda s: m.distance_lattice(origin, step, SHAPE, s, free=False)[0], "online")
    m.close()


# ---------------------------------------------------------------------------------------------------------------- 7: the existing routes
def test_existing_routes_keep_their_bits(pkg, scene, trained):
    """The lattice query's five outputs, the gradients' and the distance call's after components calls of other sizes and regions in the same side's
    workspace are the bits from before them: the shared workspace is not disturbed."""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]
    origin, step = _enclosing(scene, SHAPE)
    for side in (0, 1):
        before = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)
        xyz = pkg.lattice_points(origin, step, SHAPE)[::7]
        g_before = pkg.query_scene_gradients(lst, xyz, side=side)
        smin = float(np.percentile(before[0], 90.0, method="lower"))
        d_before = pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=side)
        pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 0, side=side)
        pkg.scene_components_lattice(lst, origin, step * np.float32(0.5), (40, 33, 30), smin, 1, 0.05, 26, side=side, rows=("dist", "owner"))      # the buffers grow
        pkg.scene_components_lattice(lst, origin, step, (5, 4, 3), smin, 1, 0.0, 18, side=side, cap=2)
        after = pkg.query_scene_lattice(lst, origin, step, SHAPE, side)
        for b, a, name in zip(before, after, ("sigma", "rgb", "owner", "owner_sigma", "n_inside")):
            _same(a.view(np.uint32), b.view(np.uint32), ("lattice query", name, side))
        for b, a in zip(g_before, pkg.query_scene_gradients(lst, xyz, side=side)):
            _same(a.view(np.uint32), b.view(np.uint32), ("gradients", side))
        for b, a, name in zip(d_before, pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=side), ("dist", "nearest", "owner", "free", "sigma")):
            _same(a.view(np.uint32), b.view(np.uint32), ("distance call", name, side))
