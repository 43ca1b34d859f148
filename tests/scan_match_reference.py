"""The rule of mon_dist_field_match and mon_dist_field_register (include/mon_core.h) restated in numpy: every operation of the match is one
float32 ufunc, so each is rounded on its own and nothing is contracted; the sample and the centre formula are tests/dist_field_reference.py's.  The GPU tests
(tests/test_scan_match.py) compare the match with it bit for bit and take the recovery bar from its Levenberg-Marquardt loop; tests/test_scan_match_abi.py
pins it on its own.  A plain module, like tests/dist_field_reference.py: no fixtures, no hooks.  Fields have shape (nz, ny, nx), x fastest."""
import numpy as np

import dist_field_reference as dr

F = np.float32
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]                             # the 21 A terms: row-major upper triangle


def posed(points, poses):
    """q (H, n, 3): the way_floats 16 centre formula of mon_dist_field_score applied to every pose and point"""
    x = np.ascontiguousarray(points, F).reshape(-1, 3); T = np.ascontiguousarray(poses, F).reshape(-1, 16)
    b = np.concatenate([x, np.zeros((x.shape[0], 1), F)], 1)
    return dr.centres(b, T[:, None, :])[:, 0]


def sample_and_jacobian(D, origin, step, points, poses, pivots=None, outside=0.0):
    """-> q (H, n, 3), d (H, n), J (H, n, 6), inside (H, n): steps 1 to 4 of the rule (d = outside and J = 0 where q is outside)"""
    q = posed(points, poses); H, n, _ = q.shape
    d, g = dr.sample(D, origin, step, q.reshape(-1, 3), outside)
    inside = dr.cell_and_fraction(np.shape(D), origin, step, q.reshape(-1, 3))[1].reshape(H, n)
    d = d.reshape(H, n); g = g.reshape(H, n, 3)
    c = np.zeros((H, 3), F) if pivots is None else np.ascontiguousarray(pivots, F).reshape(H, 3)
    with np.errstate(all="ignore"):
        a = q - c[:, None, :]
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]; a0, a1, a2 = a[..., 0], a[..., 1], a[..., 2]
        J = np.stack([g0, g1, g2, a1 * g2 - a2 * g1, a2 * g0 - a0 * g2, a0 * g1 - a1 * g0], -1)
    J = np.where(inside[..., None], J, F(0)).astype(F)
    return q, d, J, inside


def terms(D, origin, step, points, poses, pivots=None, huber=np.inf, outside=0.0):
    """-> T (H, n, 28) = the 21 A terms, the 6 b terms and rho per pose and point, inside (H, n), inlier (H, n): steps 1 to 6"""
    _, d, J, inside = sample_and_jacobian(D, origin, step, points, poses, pivots, outside)
    hub = F(huber)
    with np.errstate(all="ignore"):
        m = np.abs(d); quad = m <= hub
        w = np.where(quad, F(1), hub / m).astype(F)
        rho = np.where(quad, d * d, hub * (F(2) * m - hub)).astype(F)
        wJ = w[..., None] * J
        A = np.stack([wJ[..., i] * J[..., j] for i, j in PAIRS], -1)
        b = wJ * d[..., None]
    T = np.concatenate([A, b, rho[..., None]], -1).astype(F)
    T[~inside, :27] = F(0)
    return T, inside, inside & quad


def tree(T):
    """(H, n, K) -> (H, K): pad with +0 to the next power of two, then v'[i] = fl(v[2 i] + v[2 i + 1]) level by level; -0 is returned as +0"""
    H, n, K = T.shape; P = 1
    while P < n:
        P *= 2
    v = np.zeros((H, P, K), F); v[:, :n] = T
    with np.errstate(all="ignore"):
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
        return v[:, 0] + F(0)


def match(D, origin, step, points, poses, pivots=None, huber=np.inf, outside=0.0):
    """-> dict(cost (H,), n_inside, n_inlier (H,) int32, A (H, 21), b (H, 6)), the outputs of mon_dist_field_match"""
    T, inside, inlier = terms(D, origin, step, points, poses, pivots, huber, outside)
    s = tree(T)
    return {"cost": s[:, 27].copy(), "n_inside": inside.sum(1).astype(np.int32), "n_inlier": inlier.sum(1).astype(np.int32), "A": s[:, :21].copy(),
            "b": s[:, 21:27].copy()}


def terms64(D, origin, step, points, poses, pivots=None, huber=np.inf, outside=0.0):
    """the same 28 terms formed in float64 from the rule's own float32 d and J: (H, n, 28)"""
    _, d, J, inside = sample_and_jacobian(D, origin, step, points, poses, pivots, outside)
    d = d.astype(np.float64); J = J.astype(np.float64); hub = np.float64(F(huber))
    with np.errstate(all="ignore"):
        m = np.abs(d); quad = m <= hub
        w = np.where(quad, 1.0, hub / m)
        rho = np.where(quad, d * d, hub * (2.0 * m - hub))
    A = np.stack([w * J[..., i] * J[..., j] for i, j in PAIRS], -1); b = (w * d)[..., None] * J
    T = np.concatenate([A, b, rho[..., None]], -1)
    T[~inside, :27] = 0.0
    return T


def exp_so3(w):
    """Rodrigues in float64"""
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    A = 1.0 - th * th / 6.0 if th < 1e-8 else np.sin(th) / th
    B = 0.5 - th * th / 24.0 if th < 1e-4 else (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + A * K + B * (K @ K)


def twist_pose(pose, pivot, delta):
    """pose <- Exp(v, w) about the pivot, delta = (v, w): R' = Exp(w) R, t' = Exp(w) (t - c) + c + v, in float64: a 4 x 4 float64 matrix"""
    T = np.asarray(pose, np.float64).reshape(4, 4).copy(); c = np.asarray(pivot, np.float64); E = exp_so3(delta[3:])
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    T[:3, :3] = E @ R; T[:3, 3] = E @ (t - c) + c + np.asarray(delta[:3], np.float64)
    return T


def cost64(D, origin, step, points, pose, pivot, delta, huber=np.inf):
    """the cost of one pose moved by the twist delta, wholly in float64 (plain trilinear interpolation; every point must stay inside)"""
    T = twist_pose(pose, pivot, delta); x = np.asarray(points, np.float64).reshape(-1, 3)
    q = x @ T[:3, :3].T + T[:3, 3]
    nz, ny, nx = np.shape(D); ax = []
    for a, n in enumerate((nx, ny, nz)):
        if n == 1:
            ax.append((np.zeros(len(q), np.int64), np.zeros(len(q)), None)); continue
        g = (q[:, a] - np.float64(F(origin[a]))) / np.float64(F(step[a]))
        assert (g >= 0).all() and (g <= n - 1).all()
        i = np.minimum(np.floor(g).astype(np.int64), n - 2)
        ax.append((i, g - i, None))
    d = dr.trilinear64(D, ax); m = np.abs(d); hub = np.float64(F(huber))
    with np.errstate(all="ignore"):
        return float(np.where(m <= hub, d * d, hub * (2.0 * m - hub)).sum())


# ---------------------------------------------------------------------------------------------------- Levenberg-Marquardt, as mon_dist_field_register runs it
DEFAULTS = dict(max_evals=30, lambda0=1e-3, lambda_up=10.0, lambda_down=10.0, lambda_max=1e6, tol_rot=1e-4, min_inside=6)


def register_default(shape, step, max_value):
    """mon_register_default for a field of shape (nz, ny, nx)"""
    nz, ny, nx = shape
    s = max([abs(float(F(step[a]))) for a, n in enumerate((nx, ny, nz)) if n > 1] or [1.0])
    return dict(DEFAULTS, huber=2.0 * s, outside=float(max_value), tol_trans=1e-3 * s)


def _solve(A21, b6, lam):
    M = np.zeros((6, 6))
    for k, (i, j) in enumerate(PAIRS):
        M[i, j] = M[j, i] = float(A21[k])
    M[np.diag_indices(6)] *= 1.0 + lam
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None
    delta = np.linalg.solve(L.T, np.linalg.solve(L, -np.asarray(b6, np.float64)))
    return delta if np.isfinite(delta).all() else None


def register(D, origin, step, points, pose, prm):
    """one hypothesis -> dict(pose (4, 4) float32, cost, n_inside, n_inlier, evals, status).  The match is the float32 rule above; the solves and the pose
    updates are float64 and rounded to float32 per step, as the library's host side does them (they are not pinned bit for bit)."""
    x = np.ascontiguousarray(points, F).reshape(-1, 3); T = np.ascontiguousarray(pose, F).reshape(4, 4).copy()
    fin = np.isfinite(x).all(1)
    cen = x[fin].astype(np.float64).mean(0) if fin.any() else np.zeros(3)
    c = (T[:3, :3].astype(np.float64) @ cen + T[:3, 3].astype(np.float64)).astype(F)

    def ev(P):
        return match(D, origin, step, x, P.reshape(1, 16), c.reshape(1, 3), prm["huber"], prm["outside"])

    cur = ev(T); evals = 1; lam = float(prm["lambda0"]); status = None
    if cur["n_inside"][0] < prm["min_inside"]:
        status = 3
    while status is None:
        if lam > prm["lambda_max"]:
            status = 2; break
        if evals >= prm["max_evals"]:
            status = 1; break
        delta = _solve(cur["A"][0], cur["b"][0], lam)
        if delta is None:
            lam *= prm["lambda_up"]; continue
        cand = T.copy(); cand[:3] = twist_pose(T, c, delta)[:3].astype(F)
        new = ev(cand); evals += 1
        if new["cost"][0] < cur["cost"][0]:
            T, cur = cand, new; lam /= prm["lambda_down"]
            if np.linalg.norm(delta[:3]) < prm["tol_trans"] and np.linalg.norm(delta[3:]) < prm["tol_rot"]:
                status = 0
        else:
            lam *= prm["lambda_up"]
    return {"pose": T, "cost": cur["cost"][0], "n_inside": int(cur["n_inside"][0]), "n_inlier": int(cur["n_inlier"][0]), "evals": evals, "status": status}


def pose_errors(T, T_true, centroid):
    """-> (rotation angle between the two poses in rad, distance between the two images of the scan's centroid)"""
    T = np.asarray(T, np.float64).reshape(4, 4); G = np.asarray(T_true, np.float64).reshape(4, 4)
    R = T[:3, :3] @ G[:3, :3].T
    ang = float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    c = np.asarray(centroid, np.float64)
    return ang, float(np.linalg.norm((T[:3, :3] @ c + T[:3, 3]) - (G[:3, :3] @ c + G[:3, 3])))


# ---------------------------------------------------------------------------------------------------- the recovery case of tests/test_scan_match.py
def sdf_scene(q):
    """the analytic signed distance to two boxes and a sphere (their union) at points q (.., 3), float64"""
    q = np.asarray(q, np.float64)

    def box(centre, half):
        e = np.abs(q - np.array(centre)) - np.array(half)
        return np.linalg.norm(np.maximum(e, 0.0), axis=-1) + np.minimum(e.max(-1), 0.0)

    return np.minimum(np.minimum(box((0.7, 1.0, 0.8), (0.35, 0.5, 0.3)), box((1.6, 0.7, 0.6), (0.25, 0.3, 0.45))),
                      np.linalg.norm(q - np.array((1.5, 1.4, 0.9)), axis=-1) - 0.35)


def recovery_case(shape=(24, 20, 16), cell=0.1, n=512, seed=7):
    """-> dict(D (nz, ny, nx) float32, origin, step, points (n, 3) body frame, pose (4, 4) the known pose, starts (8, 4, 4), centroid): the field is
    sdf_scene on the lattice; the points are random points near the surfaces projected onto the zero set (Newton steps along the analytic gradient by central
    differences), then put into a body frame by the inverse of the known pose; each start is the known pose moved by 0.15 rad about a random axis through the
    scan's centroid and by one cell in a random direction."""
    nx, ny, nz = shape; rng = np.random.default_rng(seed)
    o = np.zeros(3, F); s = np.full(3, cell, F)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    D = sdf_scene(np.stack([i, j, k], -1) * float(F(cell))).astype(F)
    hi = (np.array(shape) - 1) * cell
    pts = np.zeros((0, 3))
    while len(pts) < n:
        q = rng.random((4 * n, 3)) * (hi - 4 * cell) + 2 * cell
        for _ in range(20):
            h = 1e-6; d = sdf_scene(q)
            g = np.stack([(sdf_scene(q + h * e) - sdf_scene(q - h * e)) / (2 * h) for e in np.eye(3)], -1)
            q = q - d[:, None] * g / np.maximum((g * g).sum(-1, keepdims=True), 1e-12)
        ok = (np.abs(sdf_scene(q)) < 1e-9) & (q > 1.5 * cell).all(1) & (q < hi - 1.5 * cell).all(1)
        pts = np.concatenate([pts, q[ok]])
    pts = pts[:n]
    G = np.eye(4); G[:3, :3] = dr.rotation((0.3, -0.5, 0.8), 0.7); G[:3, 3] = (0.4, -0.2, 0.3)
    G = G.astype(F).astype(np.float64)
    body = ((pts - G[:3, 3]) @ G[:3, :3]).astype(F)                                 # R^T (p - t)
    cen = body.astype(np.float64).mean(0); cw = G[:3, :3] @ cen + G[:3, 3]
    starts = np.zeros((8, 4, 4), F)
    for m in range(8):
        ax = rng.normal(size=3); v = rng.normal(size=3); v *= cell / np.linalg.norm(v)
        starts[m] = twist_pose(G, cw, np.concatenate([v, 0.15 * ax / np.linalg.norm(ax)])).astype(F)
    return dict(D=D, origin=o, step=s, points=body, pose=G.astype(F), starts=starts, centroid=cen)
