"""The rule of mon_dist_field_trace and mon_dist_field_beam_score (include/mon_core.h) restated in numpy: every operation is one float32
ufunc, so each is rounded on its own and nothing is contracted; the sample is tests/dist_field_reference.py's, the centre formula and the tree are
tests/scan_match_reference.py's.  The march is vectorised over the rays with a live mask.  The GPU tests (tests/test_field_trace.py) compare with it bit for
bit; tests/test_field_trace_abi.py pins it on its own: by a closed form, against the same loop in float64 (trace64) and against exact ray intersections with
the analytic scene of tests/scan_match_reference.py.  A plain module: no fixtures, no hooks.  Fields have shape (nz, ny, nx), x fastest."""
import numpy as np

import dist_field_reference as dr
import scan_match_reference as sm

F = np.float32
HIT, PASSED, OUT_OF_STEPS, LEFT = 0, 1, 2, 3
FIELDS = ("t_min", "t_max", "eps", "step_min", "relax", "step_outside", "max_steps")


def trace_default(shape, step):
    """mon_trace_default for a field of shape (nz, ny, nx): a dict of the seven parameters (the floats as float32)"""
    nz, ny, nx = shape
    c = min([abs(F(step[a])) for a, n in enumerate((nx, ny, nz)) if n > 1] or [F(1)])
    acc = None
    for a, n in enumerate((nx, ny, nz)):
        e = F(n - 1) * (abs(F(step[a])) if n > 1 else F(0))
        acc = e * e if acc is None else acc + e * e
    return dict(t_min=F(0), t_max=np.sqrt(acc), eps=c / F(8), step_min=c / F(4), relax=F(0.5), step_outside=c / F(2), max_steps=256)


def world_rays(rays, poses=None):
    """-> a, w (H, n, 3): step 1 of the rule; poses None: the rays as given, H = 1"""
    r = np.ascontiguousarray(rays, F).reshape(-1, 6)
    if poses is None:
        return r[None, :, :3].copy(), r[None, :, 3:].copy()
    T = np.ascontiguousarray(poses, F).reshape(-1, 1, 4, 4)
    ux, uy, uz = (r[None, :, 3 + a] for a in range(3))
    with np.errstate(all="ignore"):
        w = np.stack([(T[..., a, 0] * ux + T[..., a, 1] * uy) + T[..., a, 2] * uz for a in range(3)], -1).astype(F)
    return sm.posed(r[:, :3], poses), w


def sample32(D, origin, step, pts):
    """-> (d, inside) by the rule's sample"""
    return dr.sample(D, origin, step, pts)[0], dr.cell_and_fraction(np.shape(D), origin, step, pts)[1]


def sample64(D, origin, step, pts):
    """the same sample in float64: plain trilinear interpolation, the same inside test"""
    nz, ny, nx = np.shape(D); ax = []; inside = np.ones(len(pts), bool)
    for a, n in enumerate((nx, ny, nz)):
        if n == 1:
            ax.append((np.zeros(len(pts), np.int64), np.zeros(len(pts)), None)); continue
        with np.errstate(all="ignore"):
            g = (pts[:, a] - np.float64(F(origin[a]))) / np.float64(F(step[a]))
            ok = (g >= 0) & (g <= n - 1)
        g = np.where(ok, g, 0.0); i = np.minimum(np.floor(g).astype(np.int64), n - 2)
        ax.append((i, g - i, None)); inside &= ok
    return dr.trilinear64(D, ax), inside


def march(sample, a, w, prm, T=F):
    """step 3 of the rule for rays a, w (m, 3) in the number type T -> range (m,), status (m,), steps (m,), last; sample(points) -> (d, inside); last =
    dict(t, d, t_prev, d_prev, seen) as they stood when each ray ended (d: the hit's sample)"""
    a = np.asarray(a, T); w = np.asarray(w, T); m = a.shape[0]
    t_max, eps, step_min, relax, step_out = (T(prm[k]) for k in ("t_max", "eps", "step_min", "relax", "step_outside"))
    t = np.full(m, T(prm["t_min"]), T); t_prev = np.zeros(m, T); d_prev = np.zeros(m, T)
    seen = np.zeros(m, bool); live = np.ones(m, bool); k = np.zeros(m, np.int32)
    rng = np.zeros(m, T); status = np.full(m, -1, np.int32); d_hit = np.zeros(m, T)
    with np.errstate(all="ignore"):
        while live.any():
            idx = np.flatnonzero(live)
            done = idx[~(t[idx] <= t_max)]
            status[done] = PASSED; rng[done] = t_max; live[done] = False
            idx = np.flatnonzero(live)
            done = idx[k[idx] == prm["max_steps"]]
            status[done] = OUT_OF_STEPS; rng[done] = t[done]; live[done] = False
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            d, inside = sample((a[idx] + t[idx, None] * w[idx]).astype(T))
            k[idx] += 1
            out = idx[~inside]
            done = out[seen[out]]
            status[done] = LEFT; rng[done] = t_prev[done]; live[done] = False
            skip = out[~seen[out]]
            t[skip] = t[skip] + step_out
            ins = idx[inside]; di = d[inside].astype(T)
            hit = di <= eps
            h = ins[hit]; dh = di[hit]
            cross = t_prev[h] + (t[h] - t_prev[h]) * ((d_prev[h] - eps) / (d_prev[h] - dh))
            rng[h] = np.where(seen[h], cross, t[h]); status[h] = HIT; live[h] = False; d_hit[h] = dh
            go = ins[~hit]; dg = di[~hit]
            seen[go] = True; t_prev[go] = t[go]; d_prev[go] = dg
            t[go] = t[go] + np.fmax(relax * dg, step_min)
    return rng, status, k, dict(t=t, d=d_hit, t_prev=t_prev, d_prev=d_prev, seen=seen)


def trace(D, origin, step, rays, poses=None, prm=None, normals=False):
    """-> dict(range (H, n), status, steps (H, n) int32, normal (H, n, 3) with normals), the outputs of mon_dist_field_trace"""
    prm = prm or trace_default(np.shape(D), step)
    a, w = world_rays(rays, poses); H, n, _ = a.shape
    a = a.reshape(-1, 3); w = w.reshape(-1, 3)
    rng, status, k, _ = march(lambda p: sample32(D, origin, step, p), a, w, prm)
    out = {"range": rng.reshape(H, n), "status": status.reshape(H, n), "steps": k.reshape(H, n)}
    if normals:
        with np.errstate(all="ignore"):
            g = dr.sample(D, origin, step, (a + rng[:, None] * w).astype(F))[1]     # (0 0 0 where the point is outside)
        out["normal"] = np.where((status == HIT)[:, None], g, F(0)).astype(F).reshape(H, n, 3)
    return out


def trace64(D, origin, step, rays, poses=None, prm=None):
    """the same loop in float64 from the rule's own float32 a and w -> range, status, steps (H, n)"""
    prm = prm or trace_default(np.shape(D), step)
    a, w = world_rays(rays, poses); H, n, _ = a.shape
    rng, status, k, last = march(lambda p: sample64(D, origin, step, p), a.reshape(-1, 3), w.reshape(-1, 3), prm, np.float64)
    return {"range": rng.reshape(H, n), "status": status.reshape(H, n), "steps": k.reshape(H, n), "last": last, "a": a.reshape(-1, 3), "w": w.reshape(-1, 3)}


def beam_terms(rng, measured, huber=np.inf):
    """-> rho (H, n) float32, valid (n,): e = fl(range - measured), then step 5 of the scan-matching rule; a NaN in measured gives +0 and is not valid"""
    z = np.ascontiguousarray(measured, F).reshape(-1); hub = F(huber); valid = ~np.isnan(z)
    with np.errstate(all="ignore"):
        e = np.asarray(rng, F) - z[None, :]
        m = np.abs(e); quad = m <= hub
        rho = np.where(quad, e * e, hub * (F(2) * m - hub)).astype(F)
    return np.where(valid[None, :], rho, F(0)).astype(F), valid


def beam_score_of(rng, status, measured, huber=np.inf):
    """the beam score from ranges and statuses (H, n) -> dict(cost (H,), n_valid, n_hit (H,) int32)"""
    rho, valid = beam_terms(rng, measured, huber)
    hit = valid[None, :] & (np.asarray(status) == HIT)
    return {"cost": sm.tree(rho[..., None])[:, 0].copy(), "n_valid": np.full(rho.shape[0], valid.sum(), np.int32), "n_hit": hit.sum(1).astype(np.int32)}


def beam_score(D, origin, step, rays, measured, poses, prm=None, huber=np.inf):
    """the outputs of mon_dist_field_beam_score"""
    r = trace(D, origin, step, rays, poses, prm)
    return beam_score_of(r["range"], r["status"], measured, huber)


def utilisation(steps):
    """the share of lane-steps that do work when 64 consecutive rays of a pose share a wave (blocks of 256 rays start a new wave): steps (H, n)"""
    s = np.asarray(steps, np.int64); H, n = s.shape
    pad = np.zeros((H, -(-n // 64) * 64), np.int64); pad[:, :n] = s
    return float(s.sum()) / float(64 * pad.reshape(H, -1, 64).max(2).sum())


# ---------------------------------------------------------------------------------------------------- the analytic scene of sm.sdf_scene, exactly
BOXES = (((0.7, 1.0, 0.8), (0.35, 0.5, 0.3)), ((1.6, 0.7, 0.6), (0.25, 0.3, 0.45)))
SPHERE = ((1.5, 1.4, 0.9), 0.35)
# three free positions inside the lattice.  From none of them does a beam pass another surface closer than eps on its way to its exact hit: such a beam ends
# at the graze by the rule (the level eps is the surface), which is no range error, so it has no place in a comparison with exact intersections
SENSORS = ((1.2, 0.25, 0.75), (0.3, 0.3, 0.4), (0.25, 1.0, 1.35))
# twice the reference's own worst range error against exact intersections from these positions with default parameters, 0.367 cell, measured on the CPU
# (tests/test_field_trace_abi.py prints the figures)
ANALYTIC_BAR_CELLS = 0.734


def analytic_field(shape=(24, 20, 16), cell=0.1):
    """-> (D (nz, ny, nx) float32, origin, step): sm.sdf_scene on the lattice, as sm.recovery_case builds it"""
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return sm.sdf_scene(np.stack([i, j, k], -1) * float(F(cell))).astype(F), np.zeros(3, F), np.full(3, cell, F)


def scan_directions(n_az=128, n_el=16, el=0.7):
    """(n_az * n_el, 3) float32 unit directions, azimuth fastest: a spinning scanner's beams"""
    az = 2 * np.pi * (np.arange(n_az) + 0.5) / n_az; e = np.linspace(-el, el, n_el)
    return np.stack([np.cos(e)[:, None] * np.cos(az)[None, :], np.cos(e)[:, None] * np.sin(az)[None, :], np.sin(e)[:, None] * np.ones(n_az)[None, :]],
                    -1).reshape(-1, 3).astype(F)


def exact_hits(o, u):
    """the first intersection of the rays o + t u (float64, (m, 3)) with the two boxes and the sphere -> t (m,) (inf: none), normal (m, 3)"""
    o = np.asarray(o, np.float64); u = np.asarray(u, np.float64); m = o.shape[0]
    best = np.full(m, np.inf); nrm = np.zeros((m, 3))
    with np.errstate(all="ignore"):
        for c, h in BOXES:
            lo = (np.array(c) - np.array(h) - o) / u; hi = (np.array(c) + np.array(h) - o) / u
            near = np.minimum(lo, hi); far = np.maximum(lo, hi)
            t0 = near.max(1); t1 = far.min(1); ax = near.argmax(1)
            ok = (t0 <= t1) & (t0 > 0) & (t0 < best)
            n = np.zeros((m, 3)); n[np.arange(m), ax] = -np.sign(u[np.arange(m), ax])
            best = np.where(ok, t0, best); nrm = np.where(ok[:, None], n, nrm)
        c, r = SPHERE
        oc = o - np.array(c); b = (oc * u).sum(1); q = (oc * oc).sum(1) - r * r; uu = (u * u).sum(1)
        disc = b * b - uu * q
        t0 = (-b - np.sqrt(disc)) / uu
        ok = (disc >= 0) & (t0 > 0) & (t0 < best)
        n = (oc + t0[:, None] * u) / r
        best = np.where(ok, t0, best); nrm = np.where(ok[:, None], n, nrm)
    return best, nrm


# ---------------------------------------------------------------------------------------------------- the cases the two test files share
def random_rays(field, n, seed, spread=0.75):
    """n rays: origins spread about the lattice's centre by `spread` of its half extent per axis (0.75: a part outside), unit directions at random"""
    D, o, s = field; nz, ny, nx = D.shape; rng = np.random.default_rng(seed)
    half = 0.5 * (np.array([nx, ny, nz], np.float64) - 1) * s.astype(np.float64)
    org = o.astype(np.float64) + half + rng.uniform(-1, 1, (n, 3)) * np.abs(half) * 2 * spread
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    return np.concatenate([org, u], 1).astype(F)


def field_poses(field, H, seed):
    """pose 0 is the identity; the others turn by up to 0.2 rad about the lattice's centre and shift by up to a cell; the last row is junk"""
    D, o, s = field; nz, ny, nx = D.shape; rng = np.random.default_rng(seed)
    centre = o.astype(np.float64) + 0.5 * (np.array([nx, ny, nz]) - 1) * s.astype(np.float64)
    T = np.zeros((H, 4, 4))
    for h in range(H):
        R = np.eye(3) if h == 0 else dr.rotation(rng.normal(size=3), rng.uniform(-0.2, 0.2))
        dt = np.zeros(3) if h == 0 else rng.uniform(-1, 1, 3) * np.abs(s)
        T[h, :3, :3] = R; T[h, :3, 3] = centre - R @ centre + dt; T[h, 3] = rng.normal(size=4)
    return T.astype(F).reshape(H, 16)


def analytic_case(position):
    """-> dict for one sensor position of SENSORS: the 128 x 16 world rays, the exact range and normal per ray, which rays are judged, which must not
    hit, and the field.  Judged: the exact hit lies at least one cell inside the lattice, |u . n| >= 0.3, and the ray is still at least half a cell inside
    matter 1.5 cells past the hit (thin corner clips are not resolvable at this cell size).  Clear: the exact path keeps at least one cell of clearance
    inside the lattice (the analytic distance sampled every hundredth of a cell; it is 1-Lipschitz, so the sampled minimum is held half a spacing higher)."""
    D, o, s = analytic_field(); cell = 0.1; hi = (np.array([24, 20, 16]) - 1) * cell
    u = scan_directions(); n = u.shape[0]
    rays = np.concatenate([np.tile(np.array(position, F), (n, 1)), u], 1).astype(F)
    o64 = rays[:, :3].astype(np.float64); u64 = rays[:, 3:].astype(np.float64)
    t, nrm = exact_hits(o64, u64)
    with np.errstate(all="ignore"):
        p = o64 + np.where(np.isfinite(t), t, 0.0)[:, None] * u64
        inside = np.isfinite(t) & (p >= cell).all(1) & (p <= hi - cell).all(1)
        incidence = np.abs((u64 * nrm).sum(1)) >= 0.3
        deep = sm.sdf_scene(p + 1.5 * cell * u64) <= -0.5 * cell
    judged = inside & incidence & deep
    h = 0.01 * cell; ts = np.arange(0.0, np.linalg.norm(hi) + h, h)
    clear = np.zeros(n, bool)
    for i0 in range(0, n, 256):
        q = o64[i0:i0 + 256, None, :] + ts[None, :, None] * u64[i0:i0 + 256, None, :]
        inl = (q >= 0).all(2) & (q <= hi).all(2)
        clear[i0:i0 + 256] = np.where(inl, sm.sdf_scene(q), np.inf).min(1) >= cell + 0.5 * h
    return dict(D=D, origin=o, step=s, rays=rays, t=t, judged=judged, clear=clear & ~np.isfinite(t))


def sensor_pose():
    """a sensor pose in the analytic scene: at SENSORS[0], turned 0.4 rad about a skew axis; sensor-frame rays start at its origin"""
    G = np.eye(4); G[:3, :3] = dr.rotation((0.2, -0.4, 0.9), 0.4); G[:3, 3] = SENSORS[0]
    return G.astype(F)


def sensor_rays():
    u = scan_directions(); return np.concatenate([np.zeros_like(u), u], 1)
