"""The rule of mon_dist_field_sample and mon_dist_field_score (include/mon_core.h) restated in numpy: every operation is one float32
ufunc, so each is rounded on its own and nothing is contracted.  The GPU tests (tests/test_dist_field.py) compare with it bit for bit; tests/test_dist_field_abi.py
pins it on its own.  A plain module, like tests/paths_reference.py: no fixtures, no hooks.  Fields have shape (nz, ny, nx), x fastest."""
import numpy as np

F = np.float32


def _axis(p, o, s, n):
    """(i, f, inside) of one axis: g = fl(fl(p - o) / s); inside iff 0 <= g <= n - 1; i = min(floor(g), n - 2); f = fl(g - i).  n == 1: 0, 0, inside"""
    if n == 1:
        return np.zeros(p.shape, np.int64), np.zeros(p.shape, F), np.ones(p.shape, bool)
    with np.errstate(all="ignore"):
        g = (p - F(o)) / F(s)
        inside = (g >= F(0)) & (g <= F(n - 1))
    gi = np.where(inside, g, F(0)).astype(F)
    i = np.minimum(np.floor(gi).astype(np.int64), n - 2)
    return i, gi - i.astype(F), inside


def cell_and_fraction(shape, origin, step, xyz):
    """the rule's (i, f, inside) per axis x, y, z for points (n, 3); shape = (nz, ny, nx)"""
    nz, ny, nx = shape
    x = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    ax = [_axis(x[:, a], origin[a], step[a], n) for a, n in enumerate((nx, ny, nz))]
    return ax, ax[0][2] & ax[1][2] & ax[2][2]


def _lerp(a, d, f):
    return a + f * d                                                                # two ufuncs: fl(a + fl(f * d)), d = fl(b - a)


def sample(D, origin, step, xyz, outside=0.0):
    """-> (d (n,), grad (n, 3)) of the field D (nz, ny, nx) at points (n, 3)"""
    D = np.ascontiguousarray(D, F); nz, ny, nx = D.shape
    (ix, fx, _), (iy, fy, _), (iz, fz, _) = ax = cell_and_fraction(D.shape, origin, step, xyz)[0]
    inside = ax[0][2] & ax[1][2] & ax[2][2]
    ix, iy, iz = (np.where(inside, i, 0) for i in (ix, iy, iz))
    ux, uy, uz = int(nx > 1), int(ny > 1), int(nz > 1)
    c, e = {}, {}
    for dk in (0, 1):
        for dj in (0, 1):
            lo = D[iz + dk * uz, iy + dj * uy, ix]; hi = D[iz + dk * uz, iy + dj * uy, ix + ux]
            e[dj, dk] = hi - lo
            c[dj, dk] = _lerp(lo, e[dj, dk], fx)
    h0 = c[1, 0] - c[0, 0]; h1 = c[1, 1] - c[0, 1]
    c0 = _lerp(c[0, 0], h0, fy); c1 = _lerp(c[0, 1], h1, fy)
    w = c1 - c0
    d = _lerp(c0, w, fz)
    e0 = _lerp(e[0, 0], e[1, 0] - e[0, 0], fy); e1 = _lerp(e[0, 1], e[1, 1] - e[0, 1], fy)
    zero = np.zeros(d.shape, F)
    with np.errstate(all="ignore"):
        gx = _lerp(e0, e1 - e0, fz) / F(step[0]) if nx > 1 else zero
        gy = _lerp(h0, h1 - h0, fz) / F(step[1]) if ny > 1 else zero
        gz = w / F(step[2]) if nz > 1 else zero
    grad = np.stack([gx, gy, gz], 1).astype(F)
    return np.where(inside, d, F(outside)).astype(F), np.where(inside[:, None], grad, F(0)).astype(F)


def trilinear64(D, ax):
    """plain trilinear interpolation in float64 from the rule's own (i, f) (cell_and_fraction's first result)"""
    D64 = np.asarray(D, np.float64); nz, ny, nx = D64.shape
    (ix, fx, _), (iy, fy, _), (iz, fz, _) = ax
    ux, uy, uz = int(nx > 1), int(ny > 1), int(nz > 1)
    fx, fy, fz = (f.astype(np.float64) for f in (fx, fy, fz))
    out = 0.0
    for dk in (0, 1):
        for dj in (0, 1):
            for di in (0, 1):
                wgt = (fx if di else 1 - fx) * (fy if dj else 1 - fy) * (fz if dk else 1 - fz)
                out = out + wgt * D64[iz + dk * uz, iy + dj * uy, ix + di * ux]
    return out


def centres(spheres, ways):
    """the centre of every sphere at every waypoint: (n_traj, n_way, n_spheres, 3).  ways (n_traj, n_way, 3 | 16)"""
    b = np.ascontiguousarray(spheres, F).reshape(-1, 4); w = np.ascontiguousarray(ways, F)
    w = w.reshape(w.shape[0], w.shape[1], -1)
    with np.errstate(all="ignore"):
        if w.shape[2] == 3:
            return (w[:, :, None, :] + b[None, None, :, :3]).astype(F)
        M = w.reshape(w.shape[0], w.shape[1], 1, 4, 4)
        bx, by, bz = (b[None, None, :, a] for a in range(3))
        return np.stack([((M[..., a, 0] * bx + M[..., a, 1] * by) + M[..., a, 2] * bz) + M[..., a, 3] for a in range(3)], -1).astype(F)


def sample_centres(c, n_sub):
    """(n_traj, n_way, K, 3) -> (n_traj, n_samp, K, 3): sample q = w * n_sub + u is the waypoint's centre for u == 0, else fl(c_w + fl(tau * fl(c_(w+1) -
    c_w))) with tau = fl(u / n_sub)"""
    n_way = c.shape[1]; n_samp = (n_way - 1) * n_sub + 1
    q = np.arange(n_samp); w = q // n_sub; u = q % n_sub
    tau = (u.astype(F) / F(n_sub))[None, :, None, None]
    cw = c[:, w]; cn = c[:, np.minimum(w + 1, n_way - 1)]
    with np.errstate(all="ignore"):
        mid = cw + tau * (cn - cw)
    return np.where((u == 0)[None, :, None, None], cw, mid).astype(F)


def pairwise_tree(pen):
    """(n_traj, n_samp) -> (n_traj,): pad with +0 to the next power of two, then v'[i] = fl(v[2 i] + v[2 i + 1]) level by level"""
    n = pen.shape[1]; P = 1
    while P < n:
        P *= 2
    v = np.zeros((pen.shape[0], P), F); v[:, :n] = pen
    with np.errstate(all="ignore"):
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def score(D, origin, step, spheres, ways, n_sub, outside=0.0, margin=0.0, safe=0.0, chunk=8):
    """-> dict(min_clear, first_hit, cost, way_clear, way_grad), the header's outputs; trajectories are taken `chunk` at a time to bound the memory"""
    b = np.ascontiguousarray(spheres, F).reshape(-1, 4); ways = np.ascontiguousarray(ways, F)
    ways = ways.reshape(ways.shape[0], ways.shape[1], -1)
    outs = {k: [] for k in ("min_clear", "first_hit", "cost", "way_clear", "way_grad")}
    for t0 in range(0, ways.shape[0], chunk):
        c = sample_centres(centres(b, ways[t0:t0 + chunk]), n_sub)                 # (T, S, K, 3)
        T, S, K, _ = c.shape
        d, _ = sample(D, origin, step, c.reshape(-1, 3), outside)
        clear = d.reshape(T, S, K) - b[None, None, :, 3]
        outs["min_clear"].append(clear.min(axis=(1, 2)))
        hit = (~(clear > F(margin))).any(axis=2)
        outs["first_hit"].append(np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int32))
        with np.errstate(all="ignore"):
            h = np.maximum(F(0), F(safe) - clear)
            pen = np.zeros((T, S), F)
            for k in range(K):
                pen = pen + h[:, :, k] * h[:, :, k]
        outs["cost"].append(pairwise_tree(pen))
        wc = clear[:, ::n_sub, :]                                                   # the waypoints' own samples, q = w * n_sub
        kmin = wc.argmin(axis=2)                                                    # (the first, so the lowest, k that attains the minimum)
        outs["way_clear"].append(wc.min(axis=2))
        cmin = np.take_along_axis(c[:, ::n_sub], kmin[:, :, None, None], axis=2)[:, :, 0, :]
        _, g = sample(D, origin, step, cmin.reshape(-1, 3), outside)
        outs["way_grad"].append(g.reshape(T, -1, 3))
    return {k: np.concatenate(v, 0) for k, v in outs.items()}


def rotation(axis, angle):
    """a row-major 4 x 4 rigid transform's rotation part (float64 Rodrigues; the caller rounds to float32 once)"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose_ways(positions, seed):
    """positions (n_traj, n_way, 3) -> (n_traj, n_way, 16): each waypoint a matrix with a rotation of its own (not trivial, not axis-aligned), the position
    in the last column and a last row of junk, which the rule ignores"""
    rng = np.random.default_rng(seed); p = np.asarray(positions, F)
    M = np.zeros(p.shape[:2] + (4, 4), F)
    for t in range(p.shape[0]):
        for w in range(p.shape[1]):
            M[t, w, :3, :3] = rotation(rng.normal(size=3), rng.uniform(-3.0, 3.0)).astype(F)
    M[:, :, :3, 3] = p
    M[:, :, 3, :] = rng.normal(size=p.shape[:2] + (4,)).astype(F)
    return M.reshape(p.shape[0], p.shape[1], 16)
