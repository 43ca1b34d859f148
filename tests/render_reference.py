"""Shared reference of the render-list tests (a helper module like stage_reference.py, not a test file): what k_fused_render puts into one object's sample
list, restated for any subset of a rect's rays.  NumPy only; not imported by the product; reads nothing outside the repository.

  samples      the pose_reference.pose_rays restatement with the kernel's own fused operations -- t = fmaf(dtr, k + jitter, t0), p = fmaf(t, d, o),
               u = (p - amin) / (amax - amin) in fp32 (kernels_render.hip:62-66) -- on the restated ray rows or on rows given by the caller
  raw_bounds   the fp64 network on the object's fp16 inference weights (field_grad_reference.gather, every layer output rounded to fp16) and, next to it,
               a running first-order error bound delta of the device's evaluation, made of counted terms only (below)
  intervals    alpha and colour intervals in fp64 from raw +- delta, widened by the counted activation bound of test_scene_points.test_fold_and_activations
  count_rule   0 / 32 / 64 from given alphas, with np_composite's ambiguity window
and, for the layer chain (k_render_rays .. k_composite_render, k_grid_points, k_mesh_warp; tests/test_layer_inference*.py):
  lattice_u, mesh_warp   the lattice and the warped mesh vertices from the kernels' own operations
  slab_edge              rays whose slab test the restated ray row cannot decide
  composite_render64     k_composite_render in fp64 with a counted bound next to every output and an ambiguity flag per ray
  chain_regime           how hard a render is, from the reference's wanted values

The bound (U = 2^-24, the unit roundoff of fp32; every rounding is at most U relative to its result):
  encoding     K_ENC U sum_k |w_k f_k|: a corner weight is two products of factors of which each may be a rounded 1 - frac (5 roundings), its term passes
               through at most eight fused multiply-adds (8): K_ENC = 13.  frac itself is exact: fmaf(scale, u, 0.5) is one operation on equal inputs
               and q - floor(q) is exact.  Plus |dE / du| pos_err, the feature's first-order sensitivity to the point times the caller's bound on the point
               (zero where the point is restated bit for bit from the device's own ray row; position_bound counts it for the restated rows)
  a layer      |W| e_in + K U |W| (|a_in| + e_in), K the inner dimension: any fp32 summation order of exact fp16 x fp16 products
  every h()    + ulp16 at |want| + e: two values e apart may round to neighbours.  A ReLU output whose pre-activation cannot reach 0 within e is 0 on both
               sides: no error.  The zero padding of the encoding is exact.
  activations  sigma = __expf(r): (2 |r| + 2) U relative (+ 2^-126); y = sigma dt, dt one subtraction: (2 |r| + 4) U relative; e = __expf(-y):
               |de| <= e (y (2 |r| + 6) U + 2 U) + 2^-126; alpha = 1 - e: + U alpha.  colour: ((2 |r| + 2) (1 - c) + 2) U c + 2^-126."""
import numpy as np

import field_grad_reference as fgr
import pose_reference as pr
from stage_reference import EPS, U, h, ulp16

TINY = 2.0 ** -126            # the smallest normal fp32: below it the hardware exponential may flush to zero
K_ENC = 13
CHUNK = 1 << 15               # samples per pass of the fp64 network (memory: the gathered corners are [L, n, 8, 2] doubles)
f32 = np.float32


def fma32(a, b, c):
    """fmaf in fp32: the product of two fp32 is exact in fp64, the sum rounds once to 53 bits and once more to 24 (a double rounding differs from the fused
    one only where the 53-bit sum lands on an fp32 midpoint: one chance in 2^29 per operation)"""
    return (np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64) + np.asarray(c, f32).astype(np.float64)).astype(f32)


# ------------------------------------------------------------------ (a) samples
def sample_t(t0, t1, q, sample_seed):
    """t [P, 64] of the rays whose pixel inside the rect is q: fmaf((t1 - t0) / 64, k + rand01(sample_seed, 3, 0, q * 64 + k), t0)"""
    t0 = np.asarray(t0, f32); t1 = np.asarray(t1, f32)
    k = np.arange(64, dtype=np.uint64)[None, :]
    jit = pr.rand01(sample_seed, pr.STREAM_RENDER, 0, np.asarray(q, np.uint64)[:, None] * np.uint64(64) + k)
    dtr = ((t1 - t0) / f32(64.0)).astype(f32)
    return fma32(dtr[:, None], (np.arange(64, dtype=f32)[None, :] + jit).astype(f32), t0[:, None])


def position_bound(sc, view, Tow, rr, aabb, t):
    """Counted bound [P, 64, 3] on the unit-cube point's disagreement between pose_reference.camera_rays (fp32 sums) and the kernels' pixel_ray (fmaf
    chains) at equal t: the camera direction's norm (4 roundings a side), the division by it (1), two rot3 (3 each) -> E_d = 22 U |Row| |Rwc| |dn|;
    o: one rot3 and one add a side -> E_o = 8 U (|Row| |twc| + |tow|); p = fmaf(t, d, o) and p - amin one rounding a side each; the division two."""
    E_d, E_o = ray_row_bound(sc, view, Tow, rr["x"], rr["y"])
    mn = np.asarray(aabb[0], np.float64); ext = np.asarray(aabb[1], np.float64) - mn
    t = np.asarray(t, np.float64); p = t[..., None] * rr["d"].astype(np.float64)[:, None, :] + rr["o"].astype(np.float64)[:, None, :]
    return (np.abs(t)[..., None] * E_d[:, None, :] + E_o + 2 * U * (np.abs(p) + np.abs(p - mn))) / ext + 4 * U * np.abs((p - mn) / ext)


def samples(sc, rect, Tow, aabb, cls, sample_seed, which=None, rows=None):
    """The samples of the rays `which` (pixel indices inside the rect, all by default) of one rect under the dataset pose of its view.  rows None: the
    ray rows are pose_rays' own restatement and pos_err its counted distance from the device's; rows [P, 10] (o[3], d[3], t0, t1, flag, dn: the device's
    own rows of these rays): everything after the rows is restated bit for bit and pos_err is None.  Returns pose_rays' dict with t [P, 64], pos
    [P, 64, 3], u [P, 64, 3] (float32) and pos_err."""
    rr = pr.pose_rays(sc, [rect], Tow, aabb, cls, n_rays=0, sample_seed=sample_seed, which=which)
    aabb = np.asarray(aabb, f32)
    if rows is not None:
        rows = np.asarray(rows, f32)
        rr = dict(rr, o=rows[:, 0:3].copy(), d=rows[:, 3:6].copy(), t0=rows[:, 6].copy(), t1=rows[:, 7].copy(), hit=rows[:, 8] > 0, dn=rows[:, 9].copy())
    t = sample_t(rr["t0"], rr["t1"], rr["p"], sample_seed)
    pos = fma32(t[..., None], rr["d"][:, None, :], rr["o"][:, None, :])
    u = ((pos - aabb[0]) / (aabb[1] - aabb[0])).astype(f32)
    pos_err = position_bound(sc, int(rect[0]), Tow, rr, aabb, t) if rows is None else None
    return dict(rr, t=t, pos=pos, u=u, pos_err=pos_err)


def choose_crop(sc, k, size, views=None, stride=4):
    """The size x size crop (FrameId, x, y, h, w) over object k's silhouette that best holds all three kinds of ray, decided from the scene's geometry
    alone: the crop maximising min(rays that miss the box, rays inside the silhouette, rays inside the box but off the silhouette) over the views."""
    ob = sc.objects[k]; aabb = np.stack([-ob["half"], ob["half"]]).astype(f32); best = None
    K4 = np.array([sc.fx, sc.fy, sc.cx, sc.cy])
    for v in (range(sc.n_views) if views is None else views):
        py, px = np.mgrid[0:sc.H, 0:sc.W]
        o, d, _ = pr.camera_rays(K4, sc.Twc[v], ob["Tow"], px.reshape(-1), py.reshape(-1))
        hit = pr.slab(aabb, o, d)[0].reshape(sc.H, sc.W); sil = (sc.instance[v] == ob["cls"]) & hit
        kinds = []
        for m in (~hit, sil, hit & ~sil):
            I = np.zeros((sc.H + 1, sc.W + 1), np.int64); I[1:, 1:] = m.cumsum(0).cumsum(1)
            kinds.append((I[size:, size:] - I[:-size, size:] - I[size:, :-size] + I[:-size, :-size])[::stride, ::stride])
        score = np.minimum(np.minimum(kinds[0], kinds[1]), kinds[2])
        j = int(score.argmax()); y, x = np.unravel_index(j, score.shape)
        if best is None or score[y, x] > best[0]:
            best = (int(score[y, x]), np.array([v, x * stride, y * stride, size, size], np.uint32))
    return best[1], best[0]


# ------------------------------------------------------------------ (b) raw outputs with a bound
def _encode_bound(net, frac, feat, pos_err):
    """(E [n, Ep] unrounded, e [n, Ep]): the trilinear sum, K_ENC U sum |w f| and the first-order position term"""
    L = int(net["L"]); n = frac.shape[1]; Ep = int(net["Ep"])
    E = np.zeros((n, Ep)); A = np.zeros((n, Ep)); S = np.zeros((n, Ep))
    for l in range(L):
        fr = frac[l]; dEd = np.zeros((n, 3, 2))
        for k in range(8):
            fac = [fr[:, d] if (k >> d) & 1 else 1 - fr[:, d] for d in range(3)]
            wk = fac[0] * fac[1] * fac[2]
            E[:, 2 * l:2 * l + 2] += wk[:, None] * feat[l, :, k]; A[:, 2 * l:2 * l + 2] += np.abs(wk[:, None] * feat[l, :, k])
            if pos_err is not None:
                for d in range(3):
                    sgn = 1.0 if (k >> d) & 1 else -1.0
                    dEd[:, d] += (sgn * fac[(d + 1) % 3] * fac[(d + 2) % 3])[:, None] * feat[l, :, k]
        if pos_err is not None:
            S[:, 2 * l:2 * l + 2] = float(net["scl"][l]) * (np.abs(dEd) * pos_err[:, :, None]).sum(1)
    return E, K_ENC * U * A + S


def _round_bound(want_pre, e_pre):
    """h() of a value known within e_pre: (h(want), e + ulp16 at |want| + e)"""
    return h(want_pre), e_pre + ulp16(np.abs(want_pre) + e_pre)


def raw_bounds(net, u, pos_err=None):
    """raw [n, 4] (fp64 values of fp16 numbers) and delta [n, 4] at the fp32 unit-cube points u [n, 3]; pos_err [n, 3] or None (the points are the device's)"""
    u = np.ascontiguousarray(u, f32).reshape(-1, 3); n = u.shape[0]; NH = int(net["NH"]); L = int(net["L"])
    mats, _ = fgr.matrices(net)
    raw = np.zeros((n, 4)); delta = np.zeros((n, 4))
    for s in range(0, n, CHUNK):
        uc = u[s:s + CHUNK]; frac, feat = fgr.gather(net, uc)
        E, e = _encode_bound(net, frac, feat, None if pos_err is None else np.asarray(pos_err, np.float64).reshape(-1, 3)[s:s + CHUNK])
        a, e = _round_bound(E, e); e[:, 2 * L:] = 0.0                               # (the padding is an exact zero on both sides)
        for layer in range(NH + 1):
            Wl = mats[layer] if layer < NH else mats[NH][:4]; K = Wl.shape[1]; aW = np.abs(Wl).T
            z = a @ Wl.T; ez = e @ aW + K * U * ((np.abs(a) + e) @ aW)
            if layer < NH:
                a, e = _round_bound(np.maximum(z, 0.0), ez); e = np.where(z + ez <= 0.0, 0.0, e)
            else:
                raw[s:s + CHUNK], delta[s:s + CHUNK] = _round_bound(z, ez)
    return raw, delta


# ------------------------------------------------------------------ (c) activation intervals, the count rule
def alpha_of(r, dt):
    """(alpha, err) in fp64: alpha = 1 - exp(-exp(r) dt) and the counted bound of its fp32 evaluation from an exact r and an exact dt"""
    r = np.asarray(r, np.float64); dt = np.asarray(dt, np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = np.exp(r) * dt; y = np.where(dt == 0.0, 0.0, y)
        e = np.exp(-y); alpha = -np.expm1(-y)
        ye = np.where(np.isfinite(y), y * e, 0.0)
        err = ye * (2 * np.abs(r) + 6) * U + e * (2 * U + TINY * dt) + U * alpha + TINY
    return alpha, err


def colour_of(r):
    r = np.asarray(r, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        c = 1.0 / (1.0 + np.exp(-r))
    return c, ((2 * np.abs(r) + 2) * (1 - c) + 2) * U * c + TINY


def intervals(raw, delta, dt):
    """alpha in [lo, hi] [n] and colour in [lo, hi] [n, 3] for raw within delta of `raw` and the interval dt: both activations are monotone in raw"""
    a_lo, ea = alpha_of(raw[..., 3] - delta[..., 3], dt); a_lo = a_lo - ea
    a_hi, ea = alpha_of(raw[..., 3] + delta[..., 3], dt); a_hi = a_hi + ea
    c_lo, ec = colour_of(raw[..., :3] - delta[..., :3]); c_lo = c_lo - ec
    c_hi, ec = colour_of(raw[..., :3] + delta[..., :3]); c_hi = c_hi + ec
    return a_lo, a_hi, c_lo, c_hi


def intervals_dt(t):
    """the interval of every slot of lists t [P, 64]: t - tprev, tprev = 0 at slot 0, the hand-over from slot 31 to slot 32 included (fp64, exact)"""
    t = np.asarray(t, np.float64)
    return t - np.concatenate([np.zeros((t.shape[0], 1)), t[:, :-1]], 1)


def count_rule(alpha, hit):
    """(count [P], ambiguous [P]) from given alphas [P, 64] in fp64: T32 = prod(1 - alpha[:32]); 64 if T32 >= EPS else 32; 0 on a miss; ambiguous where
    T32 / EPS lies within max(1e-3, 4 * 32 U) of 1 (np_composite's window at the 32nd sample)"""
    T32 = np.prod(1.0 - np.asarray(alpha, np.float64)[:, :32], axis=1)
    count = np.where(hit, np.where(T32 >= EPS, 64, 32), 0).astype(np.uint32)
    return count, hit & (np.abs(T32 / EPS - 1.0) < max(1e-3, 4.0 * 32 * U)), T32


def reference_lists(raw, t, hit):
    """the reference's own lists from its wanted raw outputs: alpha [P, 64], colour [P, 64, 3], count [P], ambiguous [P] (fp64)"""
    alpha, _ = alpha_of(raw[..., 3], intervals_dt(t)); alpha = np.where(hit[:, None], alpha, 0.0)
    col, _ = colour_of(raw[..., :3])
    count, amb, _ = count_rule(alpha, hit)
    return alpha, col, count, amb


def regime(raw, alpha, count, hit):
    """the regime figures from the reference's wanted values: largest raw density of a hit ray, share of hit rays with count 32, rays of each count,
    share of emitted samples whose wanted alpha rounds to 1.0f and share below 2^-24"""
    ev = np.arange(64)[None, :] < count[:, None]
    a = alpha[ev]
    return dict(raw_max=float(raw[..., 3][ev].max()) if ev.any() else -np.inf, cut_share=float((count[hit] == 32).mean()) if hit.any() else 0.0,
                n32=int((count == 32).sum()), n64=int((count == 64).sum()), n0=int((count == 0).sum()),
                one_share=float((a.astype(f32) == f32(1.0)).mean()), tiny_share=float((a < 2.0 ** -24).mean()))


# ------------------------------------------------------------------ (d) the layer chain: lattice points, mesh warp, slab margin, composite
def lattice_u(rx, ry, rz):
    """k_grid_points bit for bit: point p = (x, y, z), x fastest, at fp32(i) / fp32(r - 1) per axis (one correctly rounded division) -> [rx ry rz, 3] fp32"""
    ax = [(np.arange(r, dtype=f32) / f32(r - 1)).astype(f32) for r in (rx, ry, rz)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], -1)


def mesh_warp(verts, aabb):
    """k_mesh_warp from its own operations, (v - mn) / (mx - mn) in fp32 on the device's vertices -> (u [n, 3] fp32, pos_err [n, 3]).  The bound counts
    the two subtractions and the division, one U each relative to the quotient: 3 U |u|.  Where every operation is correctly rounded the restated u is
    the device's own and the term only widens; it covers a division that is not."""
    v = np.asarray(verts, f32).reshape(-1, 3); aabb = np.asarray(aabb, f32)
    u = ((v - aabb[0]) / (aabb[1] - aabb[0])).astype(f32)
    return u, 3 * U * np.abs(u.astype(np.float64))


def ray_row_bound(sc, view, Tow, x, y):
    """(E_d [P, 3], E_o [3]) of position_bound: the counted distance of a restated ray row's direction and origin from the kernels' pixel_ray"""
    Rwc = np.abs(np.asarray(sc.Twc[view], np.float64)[:3, :3]); twc = np.abs(np.asarray(sc.Twc[view], np.float64)[:3, 3])
    Row = np.abs(np.asarray(Tow, np.float64)[:3, :3]); tow = np.abs(np.asarray(Tow, np.float64)[:3, 3])
    fx, fy, cx, cy = (float(v) for v in (sc.fx, sc.fy, sc.cx, sc.cy))
    dc = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(np.shape(x)[0])], -1); dn = np.abs(dc) / np.linalg.norm(dc, axis=1, keepdims=True)
    return 22 * U * (dn @ Rwc.T @ Row.T), 8 * U * (Row @ twc + tow)


def slab_edge(sc, view, Tow, aabb, rr):
    """Rays the restated slab test cannot decide [P]: a plane distance a = (m - o) / d of a row known within E_o, E_d moves by at most
    (E_o + |a| E_d) / |d| + 3 U |a| (the subtraction and the division on either side, the other side's own rounding of the quotient); a ray whose
    entry and exit distance lie within twice the largest such movement of its six planes is set aside."""
    E_d, E_o = ray_row_bound(sc, view, Tow, rr["x"], rr["y"])
    o = rr["o"].astype(np.float64); d = rr["d"].astype(np.float64); aabb = np.asarray(aabb, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.stack([(aabb[0][None] - o) / d, (aabb[1][None] - o) / d], 0)
        mv = (E_o[None, None] + np.abs(a) * E_d[None]) / np.abs(d)[None] + 3 * U * np.abs(a)
    lo = np.minimum(a[0], a[1]).max(1); hi = np.maximum(a[0], a[1]).min(1)
    mv = np.where(np.isfinite(mv), mv, 0.0).max((0, 2))
    return np.abs(hi - lo) <= 2 * mv


def composite_render64(O, tdist, flag, dn):
    """k_composite_render in fp64 for P rays of 64 samples: O [P, 64, 4] the fp16 raw outputs (uint16 bit patterns or their values), tdist [P, 64], flag
    [P], dn [P].  Serial over the samples, the break where T < EPS before a sample, alpha and colour formed from the fp16 O as the kernel forms them,
    rgb + T where 1 - T > 0.5 and white / 0 / 0 elsewhere, depth = dep / dn.
    Next to every output a running first-order bound of the kernel's fp32 evaluation, counted terms only: alpha_of / colour_of's activation terms (they
    cover __expf and the subtraction that forms dt), one U per product, per sum and per update of T, one for 1 - alpha, one for the division by dn.
    Returns a dict: rgb [P, 3], depth, mask [P] (the image); e_rgb [P, 3], e_depth [P] (its bound; 0 on a pixel the rule whitens); amb [P] (the bound
    cannot decide the break at some sample, T against EPS, or the mask, 1 - T against 0.5); n_used [P] (samples composited); and before the rule
    r [P, 3] (= rgb sums + T), dep [P], T [P] with e_r, e_dep, e_T."""
    O = np.asarray(O)
    v = (O.view(np.float16) if O.dtype == np.uint16 else O).astype(np.float64).reshape(-1, 64, 4); P = v.shape[0]
    t = np.asarray(tdist, np.float64).reshape(P, 64); hit = np.asarray(flag).reshape(P) != 0; dn = np.asarray(dn, np.float64).reshape(P)
    v = np.where(hit[:, None, None], v, 0.0); t = np.where(hit[:, None], t, 0.0)                # (a missed ray's rows hold nothing)
    c, ec = colour_of(v[..., :3]); alpha, ea = alpha_of(v[..., 3], intervals_dt(t))
    T = np.ones(P); eT = np.zeros(P); r = np.zeros((P, 3)); er = np.zeros((P, 3)); dep = np.zeros(P); edep = np.zeros(P)
    alive = hit.copy(); amb = np.zeros(P, bool); n_used = np.zeros(P, np.int64)
    for n in range(64):
        amb |= alive & (np.abs(T - EPS) <= eT)
        alive = alive & (T >= EPS); n_used += alive
        a = alpha[:, n]; w = a * T; ew = ea[:, n] * T + a * eT + U * w
        wc = w[:, None] * c[:, n]; ewc = ew[:, None] * c[:, n] + w[:, None] * ec[:, n] + U * wc
        r2 = r + wc; er2 = er + ewc + U * r2
        wt = w * t[:, n]; d2 = dep + wt; ed2 = edep + ew * t[:, n] + U * wt + U * d2
        om = 1.0 - a; eom = ea[:, n] + U * om
        T2 = T * om; eT2 = eT * om + T * eom + U * T2
        r = np.where(alive[:, None], r2, r); er = np.where(alive[:, None], er2, er); dep = np.where(alive, d2, dep); edep = np.where(alive, ed2, edep)
        T = np.where(alive, T2, T); eT = np.where(alive, eT2, eT)
    op = 1.0 - T; eop = eT + U * op
    amb |= hit & (np.abs(op - 0.5) <= eop)
    r_out = r + T[:, None]; e_r = er + eT[:, None] + U * r_out
    depth = dep / dn; e_depth = edep / dn + U * depth
    m = hit & (op > 0.5)
    return dict(rgb=np.where(m[:, None], r_out, 1.0), depth=np.where(m, depth, 0.0), mask=m.astype(np.float64), e_rgb=np.where(m[:, None], e_r, 0.0),
                e_depth=np.where(m, e_depth, 0.0), amb=amb, n_used=n_used, r=r_out, e_r=e_r, dep=dep, e_dep=edep, T=T, e_T=eT, hit=hit)


def chain_regime(raw, tdist, flag, dn):
    """the regime figures of a layer-chain render from the reference's wanted raw outputs [P, 64, 4]: largest raw density of a composited sample, share of
    the hit rays that break before sample 64, rays masked in / masked out / missed, the reference's own ambiguous rays"""
    cr = composite_render64(raw, tdist, flag, dn); hit = cr["hit"]
    used = np.arange(64)[None, :] < cr["n_used"][:, None]
    return dict(raw_max=float(np.asarray(raw, np.float64).reshape(-1, 64, 4)[..., 3][used].max()) if used.any() else -np.inf,
                cut_share=float((cr["n_used"][hit] < 64).mean()) if hit.any() else 0.0, n_in=int((cr["mask"] > 0).sum()),
                n_out=int((hit & (cr["mask"] == 0)).sum()), n_miss=int((~hit).sum()), n_amb=int(cr["amb"].sum()), n_hit=int(hit.sum()))
