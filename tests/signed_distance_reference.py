"""The signed, sub-cell distance transform of include/mon_core.h (mon_signed_distance_transform) restated in numpy fp32, twice:
`separable` is the header's rule as it reads -- per axis a the seed pass over the line's crossings, then tests/distance_reference.py's `_pass` over the
other two axes in ascending order, then the combine -- and `brute_force` is the definition, the minimum over all (cell, crossing) pairs of the nested
expression.  Every numpy operation here is one separately rounded fp32 operation, as every device operation is.  A plain module: no fixtures, no hooks.

Values have shape (nz, ny, nx) (x fastest), step = (sx, sy, sz); an edge is 3 * flat(q) + a, q its lower cell, a its axis (0 x, 1 y, 2 z)."""
import numpy as np

import distance_reference as dr

F = np.float32
INF = F(np.inf)
NP_AXIS = (2, 1, 0)                                              # the numpy axis of lattice axis a
OTHERS = ((1, 2), (0, 2), (0, 1))                                # the plain passes behind the seed pass along a, ascending


def inside(val, iso):
    """not (val <= iso): a NaN or +inf counts as inside"""
    return ~(np.asarray(val, F) <= F(iso))


def crossings(val, iso, a, ins=None):
    """-> (has, f): per cell q whether the edge (q, a) carries a crossing, and its fraction f = fl(fl(iso - v0) / fl(v1 - v0)), 0.5 where that is not in
    [0, 1]; both of val's shape (the last cell of every line has no edge).  ins: the cells' sides when they are not read from val (the scene calls)."""
    val = np.asarray(val, F); ins = inside(val, iso) if ins is None else np.asarray(ins, bool)
    v = np.moveaxis(val, NP_AXIS[a], 0); s = np.moveaxis(ins, NP_AXIS[a], 0)
    has = np.zeros(v.shape, bool); f = np.zeros(v.shape, F)
    if v.shape[0] > 1:
        has[:-1] = s[:-1] != s[1:]
        with np.errstate(all="ignore"):
            q = (F(iso) - v[:-1]) / (v[1:] - v[:-1])
        assert q.dtype == np.float32
        f[:-1] = np.where((q >= 0) & (q <= 1), q, F(0.5))
    return np.ascontiguousarray(np.moveaxis(has, 0, NP_AXIS[a])), np.ascontiguousarray(np.moveaxis(f, 0, NP_AXIS[a]))


def _seed(has, f, a, step):
    """the seed pass along a: u(p) = min over the line's crossing edges q, ascending, of fl(t t), t = fl(fl((float)(p - q) - f) * step); strictly smaller
    replaces; site 3 * flat(q) + a"""
    n = has.shape[NP_AXIS[a]]
    site_of = (3 * np.arange(has.size, dtype=np.int32).reshape(has.shape) + a).astype(np.int32)
    h = np.moveaxis(has, NP_AXIS[a], 0); ff = np.moveaxis(f, NP_AXIS[a], 0); so = np.moveaxis(site_of, NP_AXIS[a], 0)
    best = np.full(h.shape, INF, F); site = np.full(h.shape, -1, np.int32)
    tail = (slice(None),) + (None,) * (h.ndim - 1)
    p = np.arange(n)
    for q in range(n - 1):
        if not h[q].any():
            continue
        t = ((p - q).astype(F)[tail] - ff[q][None]) * F(step)
        cand = np.where(h[q][None], t * t, INF)
        assert cand.dtype == np.float32
        rep = cand < best
        best = np.where(rep, cand, best); site = np.where(rep, so[q][None], site)
    return np.ascontiguousarray(np.moveaxis(best, 0, NP_AXIS[a])), np.ascontiguousarray(np.moveaxis(site, 0, NP_AXIS[a]))


def chain(val, iso, a, step, ins=None):
    """w_a and its edges: the seed pass along a, then the two plain passes"""
    has, f = crossings(val, iso, a, ins)
    v, s = _seed(has, f, a, step[a])
    for b in OTHERS[a]:
        v, s = dr._pass(v, s, NP_AXIS[b], step[b])
    return v, s


def separable(val, iso, step, ins=None):
    """(d2, edge): the least of w_x, w_y, w_z in that order, a strictly smaller one replaces.  Without a crossing: +inf and -1."""
    d2, edge = chain(val, iso, 0, step, ins)
    for a in (1, 2):
        w, s = chain(val, iso, a, step, ins)
        rep = w < d2
        d2 = np.where(rep, w, d2); edge = np.where(rep, s, edge)
    return d2, edge


def finish(d2, edge, ins, max_dist):
    """d = the correctly rounded root; where not (d <= max_dist): d = max_dist and no edge; sdist = -d inside, d outside"""
    d = np.sqrt(d2.astype(F)); edge = edge.copy()
    cut = ~(d <= F(max_dist))
    d[cut] = F(max_dist); edge[cut] = -1
    return np.where(ins, -d, d).astype(F), edge


def transform(val, iso, step, max_dist=np.inf, ins=None):
    val = np.asarray(val, F)
    return finish(*separable(val, iso, step, ins), inside(val, iso) if ins is None else np.asarray(ins, bool), max_dist)


def brute_force(val, iso, step):
    """The definition over all (cell, crossing) pairs (small lattices only): (d2, edge, tie) -- per axis a the least nested expression over its crossings
    (the square along a first, then the other two axes ascending), the three combined in the order x, y, z; the lowest edge number among those of the
    winning axis that attain it; and whether more than one crossing attains the minimum."""
    val = np.asarray(val, F); nz, ny, nx = val.shape
    k, j, i = (g.reshape(-1).astype(np.int32) for g in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"))
    coord = (i, j, k)
    best = np.full(val.size, INF, F); edge = np.full(val.size, -1, np.int32); count = np.zeros(val.size, np.int64)
    for a in range(3):
        has, f = crossings(val, iso, a)
        on = np.flatnonzero(has.reshape(-1))
        if on.size == 0:
            continue
        fq = f.reshape(-1)[on]
        t = ((coord[a][:, None] - coord[a][on][None, :]).astype(F) - fq[None, :]) * F(step[a])
        d2 = t * t
        for b in OTHERS[a]:
            e = (coord[b][:, None] - coord[b][on][None, :]).astype(F) * F(step[b])
            d2 = e * e + d2
        assert d2.dtype == np.float32
        w = d2.min(axis=1); first = d2.argmin(axis=1); fin = w < INF
        cnt = (d2 == w[:, None]).sum(axis=1)
        rep = w < best
        count = np.where(rep, cnt, np.where((w == best) & fin, count + cnt, count))
        edge = np.where(rep, (3 * on[first] + a).astype(np.int32), edge); best = np.where(rep, w, best)
    return best.reshape(val.shape), edge.reshape(val.shape), (count > 1).reshape(val.shape)


def edge_point(edge, f_axes, shape):
    """the lattice coordinates (in cells) of the crossings on the edges `edge` (>= 0): f_axes = the three f arrays of `crossings`"""
    nz, ny, nx = shape
    a = edge % 3; q = edge // 3
    ijk = np.stack([q % nx, (q // nx) % ny, q // (nx * ny)], -1).astype(np.float64)
    fr = np.choose(a, [f_axes[0].reshape(-1)[q], f_axes[1].reshape(-1)[q], f_axes[2].reshape(-1)[q]]).astype(np.float64)
    ijk[np.arange(len(q)), a] += fr
    return ijk
