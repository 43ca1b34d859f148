"""The distance transform of include/mon_core.h (mon_distance_transform) restated in numpy fp32, twice: `separable` is the header's
three minimisations with its site rule, written as the rule reads (candidates in ascending index, a strictly smaller one replaces, the site below it is
carried along); `brute_force` is the definition, the minimum over all pairs of the nested expression.  Every numpy operation here is one separately
rounded fp32 operation, as every device operation is.  A plain module, like tests/pose_reference.py: no fixtures, no hooks.

Masks have shape (nz, ny, nx) (x fastest), step = (sx, sy, sz); a site is a flat index (k * ny + j) * nx + i."""
import numpy as np

F = np.float32
INF = F(np.inf)


def _squares(n, step):
    """fl(fl(d * step)^2) for d = 0 .. n - 1 (the sign of d does not matter: the product is squared)"""
    a = np.arange(n, dtype=np.float32) * F(step)
    return a * a


def _pass(v, s, axis, step):
    """One minimisation along `axis` of the (nz, ny, nx) arrays: out(p) = min over q of fl(a(p - q)^2 + v(q)), q ascending, strictly smaller replaces."""
    v = np.moveaxis(v, axis, 0); s = np.moveaxis(s, axis, 0)
    n = v.shape[0]; a2 = _squares(n, step); idx = np.arange(n)
    best = np.full(v.shape, INF, np.float32); site = np.full(v.shape, -1, np.int32)
    tail = (slice(None),) + (None,) * (v.ndim - 1)
    for q in range(n):
        if not (v[q] < INF).any():                               # (a candidate of +inf is never strictly smaller)
            continue
        cand = a2[np.abs(idx - q)][tail] + v[q][None]
        rep = cand < best
        best = np.where(rep, cand, best); site = np.where(rep, s[q][None], site)
    return np.ascontiguousarray(np.moveaxis(best, 0, axis)), np.ascontiguousarray(np.moveaxis(site, 0, axis))


def separable(occ, step):
    """(d2, site) of the mask by the x, y and z pass.  Without an occupied cell: +inf and -1."""
    occ = np.asarray(occ) != 0
    nz, ny, nx = occ.shape
    v = np.where(occ, F(0), INF).astype(np.float32)
    s = np.where(occ, np.arange(occ.size, dtype=np.int32).reshape(occ.shape), np.int32(-1)).astype(np.int32)
    for axis, st in ((2, step[0]), (1, step[1]), (0, step[2])):
        v, s = _pass(v, s, axis, st)
    return v, s


def finish(d2, site, max_dist):
    """dist = the correctly rounded root; where not (dist <= max_dist): dist = max_dist and no site"""
    dist = np.sqrt(d2.astype(np.float32)); site = site.copy()
    cut = ~(dist <= F(max_dist))
    dist[cut] = F(max_dist); site[cut] = -1
    return dist, site


def transform(occ, step, max_dist=np.inf):
    return finish(*separable(occ, step), max_dist)


def brute_force(occ, step):
    """The definition over all pairs (small masks only): (d2, site, tie) -- the least ((a_x^2 + a_y^2) + a_z^2) over the occupied cells, the lowest flat
    index among the cells that attain it, and whether more than one does."""
    occ = np.asarray(occ) != 0
    nz, ny, nx = occ.shape
    k, j, i = (g.reshape(-1).astype(np.int32) for g in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij"))
    on = np.flatnonzero(occ.reshape(-1))
    if on.size == 0:
        return np.full(occ.shape, INF, np.float32), np.full(occ.shape, -1, np.int32), np.zeros(occ.shape, bool)

    def sq(c, st):
        a = (c[:, None] - c[on][None, :]).astype(np.float32) * F(st)
        return a * a
    d2 = (sq(i, step[0]) + sq(j, step[1])) + sq(k, step[2])      # [cell][occupied cell], the occupied cells in ascending flat index
    assert d2.dtype == np.float32
    best = d2.min(axis=1); first = d2.argmin(axis=1)
    fin = best < INF                                             # (an overflowed distance replaces nothing: the rule's +inf keeps no site)
    tie = ((d2 == best[:, None]).sum(axis=1) > 1) & fin
    site = np.where(fin, on[first], -1).astype(np.int32)
    return best.reshape(occ.shape), site.reshape(occ.shape), tie.reshape(occ.shape)


def random_mask(shape_xyz, density, seed):
    """density: 0, "one" (one cell), 1 (all cells) or the fraction of occupied cells; shape_xyz = (nx, ny, nz) -> mask (nz, ny, nx) of uint8"""
    nx, ny, nz = shape_xyz; rng = np.random.default_rng(seed)
    m = np.zeros((nz, ny, nx), np.uint8)
    if density == "one":
        m.reshape(-1)[rng.integers(m.size)] = 1
    elif density >= 1:
        m[:] = 1
    elif density > 0:
        m[:] = rng.random(m.shape) < density
    return m
