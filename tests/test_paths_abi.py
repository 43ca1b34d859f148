"""CPU-side checks (no device needed) of the shortest-path boundary (include/mon_core.h): mon_shortest_paths, mon_scene_paths_lattice,
mon_online_paths_lattice and mon_lattice_path are declared, exported and bound with the header's signatures; the new source is listed for every build;
every argument error is MON_ERR_ARG before any device work, with a message and the outputs untouched; mon_lattice_path (host only) in full; and the
reference the GPU tests compare with (tests/paths_reference.py) is pinned on its own: its two solvers against each other in every bit, against scipy where
it is installed, and against closed forms.  (The rows that need a device are in tests/test_paths.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, p as _p
import paths_reference as pr

NEW = ("mon_shortest_paths", "mon_scene_paths_lattice", "mon_online_paths_lattice", "mon_lattice_path")
MON_ERR_ARG, MON_ERR_NO_DEVICE = 1, 2
INF = float("inf")


def _kind(arg):
    """abi_decl.kind, which knows no int32_t parameter (ctypes.c_int32 is c_int here)"""
    if "*" in arg:
        return "ptr"
    return {"size_t": "u64", "int": "int", "int32_t": "int", "uint32_t": "uint32", "float": "float"}[arg.split()[0]]


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [13, 21, 19, 6]
    assert [_kind(a) for a in _decl("mon_shortest_paths")] == ["int", "ptr", "int", "int", "int", "ptr", "int", "ptr", "ptr", "u64", "float", "ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_scene_paths_lattice")] == (["ptr", "u64", "int", "ptr", "ptr", "int", "int", "int"] + ["float"] * 4 +
                                                                   ["int", "ptr", "u64", "float"] + ["ptr"] * 5)
    assert _decl("mon_online_paths_lattice")[1:] == _decl("mon_scene_paths_lattice")[3:]                # "the same from origin3 on"
    assert [_kind(a) for a in _decl("mon_lattice_path")] == ["ptr", "u64", "int", "ptr", "u64", "ptr"]
    for name in ("shortest_paths", "scene_paths_lattice", "lattice_path"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.paths_lattice)
    assert "mon_debug_paths_stats" in pkg.diag_symbols() and "mon_debug_paths_stats" not in pkg.exported_symbols()


def test_new_source_is_listed_for_every_build():
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_paths.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_paths.hip"))


def test_argument_errors_need_no_device(pkg):
    """Everything the distance and components calls refuse for the shared arguments; cost or seeds NULL; n_seeds 0 or above 2^22; a seed outside the
    lattice; a connectivity other than 6 / 18 / 26; max_cost <= 0 or NaN; clearance or soft_weight negative or not finite; soft_weight > 0 with
    soft_radius not finite or <= 0; the standalone call with a cell_cost entry negative or not finite: MON_ERR_ARG with a message and every output
    untouched, whether or not a device is present.  What the argument checks accept fails on the NULL object alone; the standalone call without a device
    is MON_ERR_NO_DEVICE after its checks."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    mask = np.ones(24, np.uint8); s3 = np.array([0.25, 0.0, -0.125], np.float32); o3 = np.array([0.5, -1.0, 2.0], np.float32)
    cc = np.linspace(0.0, 5.0, 24).astype(np.float32); seeds = np.array([0, 23, 23, 5], np.int32)
    cost = np.full(64, 7.0, np.float32); nxt = np.full(64, 7, np.int32)
    dist = np.full(64, 7.0, np.float32); sig = np.full(64, 7.0, np.float32); own = np.full(64, 7, np.int32)
    lots = np.zeros((1 << 22) + 1, np.int32)

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def sp(m=mask, shape=(2, 3, 4), s=s3, conn=26, c=cc, sd=seeds, ns=4, mx=INF, co=cost, nx_=nxt, device=0):
        return L.mon_shortest_paths(device, _p(m), *shape, _p(s), conn, _p(c), _p(sd), ns, mx, _p(co), _p(nx_))

    wrap = ((1 << 30, 1 << 30, 1 << 30), (1 << 22, 1 << 21, 1 << 21), (2147483647, 2147483647, 2147483647), (1, 1 << 22, 2), (1 << 16, 1 << 16, 1 << 16))
    refused = (dict(m=None), dict(s=None), dict(co=None), dict(sd=None), dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)),
               dict(shape=(-1, 3, 4)), dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)), dict(s=ed(s3, 1, np.nan)), dict(s=ed(s3, 0, -np.inf)),
               dict(conn=0), dict(conn=4), dict(conn=8), dict(conn=27), dict(conn=-6), dict(ns=0), dict(sd=lots, ns=(1 << 22) + 1), dict(sd=ed(seeds, 1, 24)),
               dict(sd=ed(seeds, 3, -1)), dict(sd=ed(seeds, 0, 1 << 30)), dict(mx=0.0), dict(mx=-1.0), dict(mx=float("nan")), dict(mx=-INF),
               dict(c=ed(cc, 7, -1e-6)), dict(c=ed(cc, 23, np.nan)), dict(c=ed(cc, 0, np.inf))) + tuple(dict(shape=w) for w in wrap)
    for kw in refused:
        assert sp(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    for kw, word in ((dict(co=None), b"cost"), (dict(sd=None), b"seeds"), (dict(conn=8), b"connectivity"), (dict(ns=0), b"seeds"), (dict(sd=ed(seeds, 1, 24)), b"seed 1"),
                     (dict(mx=0.0), b"max_cost"), (dict(c=ed(cc, 7, -1e-6)), b"cell_cost[7]"), (dict(shape=(1 << 11, 1 << 11, 2)), b"points"), (dict(m=None), b"passable")):
        assert sp(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    if pkg.device_count() == 0:
        for kw in (dict(), dict(nx_=None), dict(c=None), dict(conn=6), dict(conn=18), dict(mx=1e-30), dict(ns=1), dict(c=np.zeros(24, np.float32))):
            assert sp(**kw) == MON_ERR_NO_DEVICE and L.mon_last_error(), kw                            # accepted by the checks; then no device

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), smin=1.0, clr=0.0, sr=0.0, sw=0.0, conn=26, sd=seeds, ns=4, mx=INF, co=cost,
            rest=(nxt, dist, sig, own)):
        return L.mon_scene_paths_lattice(objs, n_objs, side, _p(o), _p(s), *shape, smin, clr, sr, sw, conn, _p(sd), ns, mx, _p(co), *[_p(a) for a in rest])

    def onl(o=o3, s=s3, shape=(2, 3, 4), smin=1.0, clr=0.0, sr=0.0, sw=0.0, conn=26, sd=seeds, ns=4, mx=INF, co=cost, rest=(nxt, dist, sig, own)):
        return L.mon_online_paths_lattice(None, _p(o), _p(s), *shape, smin, clr, sr, sw, conn, _p(sd), ns, mx, _p(co), *[_p(a) for a in rest])

    accepted = (dict(), dict(rest=(None,) * 4), dict(smin=0.0), dict(conn=6), dict(conn=18), dict(clr=0.5), dict(sw=0.0, sr=-1.0), dict(sw=0.0, sr=float("nan")),
                dict(sw=2.0, sr=0.5), dict(mx=1e-30), dict(ns=1))
    refused = (dict(objs=None), dict(o=None), dict(s=None), dict(co=None), dict(sd=None), dict(n_objs=0), dict(objs=many, n_objs=257),
               dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)), dict(shape=(1 << 11, 1 << 11, 2)),
               dict(shape=((1 << 22) + 1, 1, 1)), dict(side=2), dict(side=-1), dict(o=ed(o3, 0, np.nan)), dict(o=ed(o3, 2, np.inf)), dict(s=ed(s3, 1, np.nan)),
               dict(s=ed(s3, 0, -np.inf)), dict(smin=-1e-6), dict(smin=float("nan")), dict(smin=np.inf), dict(conn=0), dict(conn=7), dict(conn=27),
               dict(clr=-1e-6), dict(clr=float("nan")), dict(clr=np.inf), dict(sw=-1e-6), dict(sw=float("nan")), dict(sw=np.inf), dict(sw=1.0, sr=0.0),
               dict(sw=1.0, sr=-0.5), dict(sw=1.0, sr=float("nan")), dict(sw=1.0, sr=np.inf), dict(ns=0), dict(sd=lots, ns=(1 << 22) + 1),
               dict(sd=ed(seeds, 2, 24)), dict(sd=ed(seeds, 0, -1)), dict(mx=0.0), dict(mx=-2.0), dict(mx=float("nan"))) + tuple(dict(shape=w) for w in wrap)
    for kw in accepted + refused:
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw                 # (the accepted ones: a NULL element of objs)
    for kw in accepted:
        assert lat(**kw) == MON_ERR_ARG and b"object" in L.mon_last_error(), kw    # accepted by the argument checks: fails on the NULL object alone
    for kw, word in ((dict(smin=-1e-6), b"sigma_min"), (dict(conn=7), b"connectivity"), (dict(clr=-1e-6), b"clearance"), (dict(sw=-1e-6), b"soft_weight"),
                     (dict(sw=1.0, sr=0.0), b"soft_radius"), (dict(side=2), b"side"), (dict(objs=many, n_objs=257), b"objects"), (dict(co=None), b"cost"),
                     (dict(sd=None), b"seeds"), (dict(ns=0), b"seeds"), (dict(sd=ed(seeds, 2, 24)), b"seed 2"), (dict(mx=0.0), b"max_cost")):
        assert lat(**kw) == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
    for kw in (dict(), dict(conn=5), dict(smin=-1.0), dict(shape=(0, 1, 1)), dict(co=None), dict(sd=None), dict(clr=-1.0), dict(mx=0.0)):
        assert onl(**kw) == MON_ERR_ARG, kw                                        # a NULL manager, with good and with bad arguments
    assert (cost == 7.0).all() and (nxt == 7).all() and (dist == 7.0).all() and (sig == 7.0).all() and (own == 7).all()


def test_lattice_path(pkg):
    """A straight line with cap 0, below, at and above the length (*n_path is the whole length; nothing behind min(cap, length) is written); a start that
    is an end; NULL next / n_path, a start out of range, an entry out of range on the walk (one off it does no harm), a planted cycle: MON_ERR_ARG with
    path and n_path untouched."""
    L = pkg.lib()
    nxt = np.arange(-1, 9, dtype=np.int32)                                         # cell v steps to v - 1; cell 0 ends
    n = C.c_size_t(77)

    def walk(nx_=nxt, n_cells=10, start=6, cap=16, path="own", np_=n):
        buf = np.full(16, -5, np.int32)
        rc = L.mon_lattice_path(_p(nx_), n_cells, start, _p(buf) if path == "own" else None, cap, C.byref(np_) if np_ is not None else None)
        return rc, buf

    for cap in (0, 3, 7, 12):
        rc, buf = walk(cap=cap)
        assert rc == 0 and n.value == 7, cap
        k = min(cap, 7)
        assert buf[:k].tolist() == list(range(6, 6 - k, -1)) and (buf[k:] == -5).all(), cap
    rc, _ = walk(cap=0, path=None); assert rc == 0 and n.value == 7
    rc, buf = walk(start=0); assert rc == 0 and n.value == 1 and buf[0] == 0 and (buf[1:] == -5).all()
    assert pkg.lattice_path(nxt, 9).tolist() == list(range(9, -1, -1)) and pkg.lattice_path(nxt, 0).tolist() == [0]
    n.value = 77
    bad_far = nxt.copy(); bad_far[3] = 10; bad_low = nxt.copy(); bad_low[2] = -2; cyc = nxt.copy(); cyc[2] = 5; self_ = nxt.copy(); self_[4] = 4
    for kw, word in ((dict(nx_=None), b"next"), (dict(np_=None), b"n_path"), (dict(path=None, cap=4), b"path"), (dict(start=-1), b"start"), (dict(start=10), b"start"),
                     (dict(start=1 << 30), b"start"), (dict(nx_=bad_far), b"next holds 10"), (dict(nx_=bad_low), b"next holds -2"), (dict(nx_=cyc), b"cycle"),
                     (dict(nx_=self_), b"cycle"), (dict(n_cells=0, start=0), b"start")):
        rc, buf = walk(**kw)
        assert rc == MON_ERR_ARG and word in L.mon_last_error(), (kw, L.mon_last_error())
        assert (buf == -5).all() and n.value == 77, kw
    rc, buf = walk(nx_=bad_far, start=2); assert rc == 0 and n.value == 3 and buf[:3].tolist() == [2, 1, 0]      # the damaged entry is not on this walk
    with pytest.raises(pkg.MonError):
        pkg.lattice_path(cyc, 6)


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


CASES = (  # shape (nx, ny, nz), passable share, connectivity, step, multipliers, seeds
    ((13, 11, 9), 0.69, 6, (0.3, 0.7, 1.1), False, 1), ((13, 11, 9), 0.69, 18, (0.25, 0.5, 0.125), True, 3), ((13, 11, 9), 0.5, 26, (-0.3, 0.2, -0.45), True, 1),
    ((17, 5, 12), 0.98, 26, (0.3, 0.0, 0.2), False, 3), ((17, 5, 12), 0.69, 18, (0.11, 0.13, 0.17), True, 2), ((9, 14, 10), 0.5, 6, (0.5, 0.25, 2.0), True, 3),
    ((9, 14, 10), 1, 26, (0.0, 0.37, 0.0), True, 1), ((21, 1, 19), 0.69, 26, (1.0, 1.0, 1.0), False, 2))


def _case(i):
    shape, share, conn, step, with_c, n_seeds = CASES[i]
    rng = np.random.default_rng(500 + i)
    m = pr.random_mask(shape, share, seed=300 + i)
    c = (1 + 4 * rng.random(m.shape)).astype(np.float32) if with_c else None
    seeds = rng.choice(np.flatnonzero(m.reshape(-1)), n_seeds, replace=False).astype(np.int32)
    return m, seeds, np.array(step, np.float32), conn, c


@pytest.mark.parametrize("i", range(len(CASES)))
def test_dijkstra_equals_jacobi_in_every_bit(i):
    """The header's argument, pinned: a heap Dijkstra and a whole-lattice Jacobi sweep -- two relaxation orders as far apart as they come -- give the same
    fp32 field bit for bit under all three connectivities, anisotropic / power-of-two / negative / zero steps, with and without multipliers in [1, 5]."""
    m, seeds, step, conn, c = _case(i)
    a = pr.dijkstra(m, seeds, step, conn, c); b, sweeps = pr.jacobi(m, seeds, step, conn, c, return_sweeps=True)
    assert np.array_equal(_bits(a), _bits(b)), (i, int((_bits(a) != _bits(b)).sum()))
    assert np.isinf(a[m == 0]).all() and (a.reshape(-1)[seeds] == 0).all() and sweeps > 3
    reach = np.isfinite(a)
    assert reach.sum() > len(seeds), i                                             # the case is not vacuous
    if conn == 6 and c is not None or i == 0:
        assert (reach & (m != 0)).sum() < (m != 0).sum(), i                         # ... and under 6-connectivity leaves passable cells unreached


def test_reference_equals_scipy():
    """6-connected, steps 0.25 / 0.5 / 0.125, distances of at most a few dozen steps: every sum is exact in fp32 and in fp64, so scipy's fp64 Dijkstra on
    the explicit graph must give the same numbers."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    shape = (12, 10, 9); nx, ny, nz = shape; step = np.array([0.25, 0.5, 0.125], np.float32)
    for seed, share in ((1, 0.69), (2, 0.98)):
        m = pr.random_mask(shape, share, seed)
        on = m.reshape(-1) != 0; idx = np.arange(m.size).reshape(m.shape)
        rows, cols, w = [], [], []
        for ax, st in ((2, step[0]), (1, step[1]), (0, step[2])):
            a = np.moveaxis(idx, ax, 0)[:-1].reshape(-1); b = np.moveaxis(idx, ax, 0)[1:].reshape(-1)
            ok = on[a] & on[b]
            rows += [a[ok], b[ok]]; cols += [b[ok], a[ok]]; w += [np.full(ok.sum() * 2, float(st))]
        g = sp.csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(m.size, m.size))
        seeds = np.flatnonzero(on)[[0, -1]].astype(np.int32)
        want = dijkstra(g, directed=False, indices=seeds, min_only=True)
        want[~on] = np.inf
        got = pr.jacobi(m, seeds, step, 6)
        assert np.array_equal(got.reshape(-1).astype(np.float64), want), (seed, share)
        assert np.array_equal(_bits(pr.dijkstra(m, seeds, step, 6)), _bits(got))


def test_reference_on_closed_forms():
    """Empty lattice, seed at cell 0, 6-connected: cost = i * sx + j * sy + k * sz (power-of-two steps: exact), next = the -z, else -y, else -x neighbour.
    A full wall with one hole: the cost behind the wall is the cost to the hole plus the cost from it.  Two seeds: the least of the two fields.  A seed on
    a blocked cell contributes nothing; duplicates change nothing; max_cost keeps the cell at exactly max_cost."""
    shape = (9, 7, 5); nx, ny, nz = shape; step = np.array([0.5, 0.25, 2.0], np.float32)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    m = np.ones((nz, ny, nx), np.uint8)
    cost, nxt = pr.field(m, [0], step, 6)
    assert np.array_equal(cost, (i * 0.5 + j * 0.25 + k * 2.0).astype(np.float32))
    flat = (k * ny + j) * nx + i
    assert np.array_equal(nxt, np.where(k > 0, flat - nx * ny, np.where(j > 0, flat - nx, np.where(i > 0, flat - 1, -1))).astype(np.int32))
    w = pr.wall_with_hole(shape, 4, (3, 2))
    cw = pr.jacobi(w, [0], step, 6)
    via = lambda ii, jj, kk: abs(ii - 4) * 0.5 + abs(jj - 3) * 0.25 + abs(kk - 2) * 2.0      # noqa: E731
    want = np.where(i < 4, i * 0.5 + j * 0.25 + k * 2.0, via(0, 0, 0) + via(i, j, k)); want[:, :, 4] = np.inf; want[2, 3, 4] = via(0, 0, 0)
    assert np.array_equal(cw, want.astype(np.float32))
    far = nx * ny * nz - 1
    both = pr.jacobi(m, [0, far], step, 6)
    assert np.array_equal(both, np.minimum(pr.jacobi(m, [0], step, 6), pr.jacobi(m, [far], step, 6))) and both.reshape(-1)[far] == 0
    blocked = int(flat[1, 1, 4])
    assert np.isinf(pr.jacobi(w, [blocked], step, 26)).all()
    assert np.array_equal(pr.jacobi(w, [0, blocked, 0, 0], step, 26), pr.jacobi(w, [0], step, 26))
    mc = float(cost[1, 2, 3])
    tc, tn = pr.field(m, [0], step, 6, max_cost=mc)
    assert tc[1, 2, 3] == np.float32(mc) and tn[1, 2, 3] == nxt[1, 2, 3] and np.isinf(tc[cost > mc]).all() and (tn[cost > mc] == -1).all()
    assert np.array_equal(tc[cost <= mc], cost[cost <= mc])


def test_next_leads_to_a_seed():
    """Under non-zero steps and multipliers in [1, 5] every reachable non-seed cell has next >= 0 (a weight below 2^-24 of a cost does not occur at these
    sizes), and following it reaches a seed with cost falling strictly."""
    for i in (1, 2, 4, 5):
        m, seeds, step, conn, c = _case(i)
        cost, nxt = pr.field(m, seeds, step, conn, c)
        reach = np.isfinite(cost); fc = cost.reshape(-1); fn = nxt.reshape(-1)
        is_seed = np.zeros(m.size, bool); is_seed[seeds] = True
        assert ((fn >= 0) == (reach.reshape(-1) & ~is_seed)).all(), i
        assert (fc[fn[fn >= 0]] < fc[fn >= 0]).all(), i
        for start in np.flatnonzero(reach.reshape(-1))[::37]:
            path = pr.follow(nxt, start)
            assert is_seed[path[-1]] and (np.diff(fc[path]) < 0).all(), (i, start)


def test_next_under_a_zero_step():
    """With a zero step some moves are free: cells joined by them share their cost, and the cells with next == -1 are exactly those the rule names -- the
    reachable cells without a neighbour that is strictly cheaper and explains their cost (checked cell by cell in plain Python).  Case 3 has sy = 0 (a
    diagonal that uses y is as long as the move without it, so few cells are left without a way); case 6 has sx = sz = 0 and multipliers: every plane of
    constant j is one plateau, entered only where a move from the plane before attains the plateau's cost, so most cells end the walk."""
    for case in (3, 6):
        m, seeds, step, conn, c = _case(case)
        assert (step == 0).sum() == (1 if case == 3 else 2)
        cost, nxt = pr.field(m, seeds, step, conn, c)
        nz, ny, nx = m.shape; offs = pr.offsets(conn); F = np.float32
        none = 0
        for v in range(m.size):
            i, j, k = v % nx, (v // nx) % ny, v // (nx * ny)
            want = -1
            if np.isfinite(cost[k, j, i]):
                for dx, dy, dz in offs:
                    I, J, K = i + dx, j + dy, k + dz
                    if not (0 <= I < nx and 0 <= J < ny and 0 <= K < nz and cost[K, J, I] < cost[k, j, i]):
                        continue
                    w = pr.move_length(step, dx, dy, dz)
                    if c is not None:
                        w = F(w * F(F(0.5) * F(c[K, J, I] + c[k, j, i])))
                    if F(cost[K, J, I] + w) == cost[k, j, i]:
                        want = (K * ny + J) * nx + I
                        break
                none += want < 0
            assert nxt[k, j, i] == want, (case, v)
        assert none > len(seeds), case                                              # more ends than seeds: the zero step's plateaus
        if case == 6:
            assert none > m.size // 2
