"""GPU tests (-m gpu) of the scene probe (mon_scene_probe, mon_online_probe_scene; kernels k_scene_probe_rays and k_scene_probe_composite in
kernels_scene_probe.hip, the keyed instantiation of k_fused_render<EMIT>).  The yardstick is the scene render itself, bit for bit: a probe of a rect's
pixels equals mon_scene_render of the rect; a query's outputs do not depend on its company, its place, the number of poses or the pass boundary; the
first-hit outputs equal a NumPy merge of the dumped sample lists (fp64 transmittance) away from ties at 0.5; the ray rows at sub-pixel points stay within
a forward error bound of an fp64 restatement of pixel_ray and ray_intersect.  The scene, the trained objects and the overlap view are those of
tests/test_scene_render.py."""
import os
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import ROOT
import test_scene_render as tsr
from test_scene_render import scene, trained, overlap_view       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu

CHUNK = 16384                # kRenderChunkRays: the queries of one pass
TIE = 1e-4                   # a ray is left out of the hit comparison when a reference T_{i+1} lies within this (relative) of 0.5
U = 2.0 ** -24               # unit roundoff of fp32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(g).reshape(-1), _bits(w).reshape(-1)), (what, k)


def _pick_rect(sc, v, i, j, h=24, w=40):
    """A 40 x 24 rect of view v that holds background, pixels of one of the objects i, j alone and pixels where both silhouettes overlap: the window
    (on a 4-pixel lattice) with the largest minimum of the three counts."""
    sil = tsr._silhouettes(sc, v)
    both = sil[i][0] & sil[j][0]; alone = sil[i][0] ^ sil[j][0]; bg = ~(sil[0][0] | sil[1][0] | sil[2][0])
    best = None
    for y in range(0, sc.H - h + 1, 4):
        for x in range(0, sc.W - w + 1, 4):
            s = min(int(q[y:y + h, x:x + w].sum()) for q in (both, alone, bg))
            if best is None or s > best[0]:
                best = (s, x, y)
    assert best[0] >= 30, best
    return np.array([v, best[1], best[2], h, w], np.uint32)


@pytest.fixture(scope="module")
def setup(pkg, ss, scene, trained, overlap_view):       # noqa: F811
    """The three objects of the overlap view (object 0 on its inflated box, so that sample segments interleave), the rect, its queries and pose, and the
    reference of tests 2 and 3: the probe of the rect's pixels with K = 3 on side 0, skipping off -- computed once and left unchanged."""
    sc = scene; _, objs = trained; v, i, j = overlap_view
    objs3 = [objs["b0"], objs["a1"], objs["a2"]]
    rect = _pick_rect(sc, v, i, j); pose = tsr._pose(ss, sc, v)
    q = pkg.rect_queries(rect)
    for o in objs3:
        o.set_render_skip(False)
    base = pkg.probe_scene(objs3, q, pose)
    for a in base:
        a.setflags(write=False)
    return dict(sc=sc, objs=objs, objs3=objs3, pair=(i, j), v=v, rect=rect, pose=pose, q=q, base=base)


def np_first_hit(t, alpha, count, with_index=False):
    """NumPy reference of the hit outputs: lists [K, P, 64] with count [K, P], merged by (t, list, slot); the transmittance after every merged sample in
    fp64.  Returns per ray: has a crossing 1 - T_{i+1} > 0.5, the fp32 t of the first one, its list, and near = some T_{i+1} within TIE (relative) of 0.5;
    with_index: also the crossing's place i in the merged order (0 without a crossing)."""
    K, P = count.shape
    slot = np.arange(64)
    valid = slot[None, None, :] < count[..., None]
    tt = np.where(valid, t, np.float32(np.inf)).transpose(1, 0, 2).reshape(P, K * 64).astype(np.float32)
    aa = np.where(valid, alpha, 0.0).transpose(1, 0, 2).reshape(P, K * 64).astype(np.float64)
    vv = valid.transpose(1, 0, 2).reshape(P, K * 64)
    kk = np.broadcast_to(np.arange(K)[:, None, None], (K, P, 64)).transpose(1, 0, 2).reshape(P, K * 64)
    ii = np.broadcast_to(slot, (P, K, 64)).reshape(P, K * 64)
    order = np.lexsort((ii, kk, tt), axis=-1)
    tt, aa, kk, vv = (np.take_along_axis(x, order, 1) for x in (tt, aa, kk, vv))
    incl = np.cumprod(1.0 - aa, axis=1)
    cross = vv & (1.0 - incl > 0.5)
    has = cross.any(1); first = cross.argmax(1); r = np.arange(P)
    near = (vv & (np.abs(incl / 0.5 - 1.0) < TIE)).any(1)
    out = has, np.where(has, tt[r, first], np.float32(0)).astype(np.float32), np.where(has, kk[r, first], -1).astype(np.int32), near
    return out + (np.where(has, first, 0),) if with_index else out


def _check_hits(out, t, alpha, count, dn, cap=0.01):
    """hit_depth / hit_instance of a probe output against np_first_hit under the near-tie rule; at most `cap` of the rays with opacity > 0.5 left out."""
    has, ht, hk, near = np_first_hit(t, alpha, count)
    opaque = out[2] > 0.5
    left_out = int((near & opaque).sum())
    print("hit check: %d rays, %d hits, %d near a tie (%d of %d opaque)" % (has.size, int(has.sum()), int(near.sum()), left_out, int(opaque.sum())))
    assert left_out <= cap * max(int(opaque.sum()), 1), (left_out, int(opaque.sum()))
    ok = ~near
    want_d = np.where(has, ht / dn.astype(np.float32), np.float32(0)).astype(np.float32)
    assert np.array_equal(out[5][ok], hk[ok])
    assert np.array_equal(_bits(out[4])[ok], _bits(want_d)[ok])
    return has, near


def _check_invariants(pkg, objs, rect, pose, out, side=0):
    """Test 7: hit_instance >= 0 implies opacity > 0.5 - 1e-4; hit_depth lies between the smallest and the largest emitted t / dn of the ray; K = 1 gives
    hit_instance in {-1, 0}.  `out` = the probe of rect's pixels (row-major) under the objects' present skip setting."""
    t, a, c, n = tsr._dump(pkg, objs, rect, pose, side)
    dn = pkg.scene_probe_rays(objs, pkg.rect_queries(rect), pose, 0, side)[:, 9]
    rgb, depth, op, inst, hd, hi = out
    assert (op[hi >= 0] > 0.5 - 1e-4).all()
    valid = np.arange(64)[None, None, :] < n[..., None]
    td = t / dn[None, :, None]
    lo = np.where(valid, td, np.inf).min((0, 2)); hi_t = np.where(valid, td, -np.inf).max((0, 2))
    h = hi >= 0
    assert (hd[h] >= lo[h]).all() and (hd[h] <= hi_t[h]).all()
    assert (hd[~h] == 0).all() and set(np.unique(hi)) <= set(range(-1, len(objs)))
    if len(objs) == 1:
        assert set(np.unique(hi)) <= {-1, 0}
    return t, a, c, n, dn


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("skip", [False, True])
def test_bit_rule(pkg, setup, skip, K, side):
    """Test 1: every pixel of the rect as a query, row-major, key = the pixel index: rgb, depth, opacity and instance are mon_scene_render's bits, with
    render skipping off and on (min_alpha 1e-3), K = 1 and 3, on both sides.  (Test 7's invariants on every case.)"""
    s = setup; objs = s["objs3"] if K == 3 else [s["objs3"][s["pair"][0]]]
    for o in objs:
        o.set_render_skip(skip, 1e-3)
    try:
        want = pkg.render_scene(objs, s["rect"], s["pose"], side)
        got = pkg.probe_scene(objs, s["q"], s["pose"], side)
        _same_bits(got[:4], want, (skip, K, side))
        assert (want[2] > 0.5).sum() >= (50 if K == 3 else 20) and (want[2] < 0.5).sum() >= 30      # the rect holds objects and background
        _check_invariants(pkg, objs, s["rect"], s["pose"], got, side)
    finally:
        for o in objs:
            o.set_render_skip(False)
    if K == 3 and side == 0 and not skip:
        _same_bits(got, s["base"], "equal arguments, equal bits")


def test_independence(pkg, ss, setup):
    """Test 2: the queries of test 1 shuffled, a subset of 37, repeated to kRenderChunkRays + 100 (a pass boundary inside the list) and interleaved with
    the queries of two other poses (P = 3): every query's six outputs are its bits from test 1, or from the single-pose call of its own pose."""
    s = setup; objs, q, pose, base = s["objs3"], s["q"], s["pose"], s["base"]; P = q.shape[0]
    rng = np.random.RandomState(11)
    perm = rng.permutation(P)
    _same_bits(pkg.probe_scene(objs, q[perm], pose), [a[perm] for a in base], "shuffled")
    sub = rng.choice(P, 37, replace=False)
    _same_bits(pkg.probe_scene(objs, q[sub], pose), [a[sub] for a in base], "subset")
    rep = (np.arange(CHUNK + 100) * 7 + 3) % P
    _same_bits(pkg.probe_scene(objs, q[rep], pose), [a[rep] for a in base], "pass boundary")
    poses = np.stack([pose, pose, pose])                                                # two other poses: the camera moved a few pixels' worth
    poses[1, 12] += np.float32(0.03); poses[2, 13] -= np.float32(0.02); poses[2, 14] += np.float32(0.01)
    singles = [base] + [pkg.probe_scene(objs, q, poses[p]) for p in (1, 2)]
    for p in (1, 2):                                                                    # (test 7 on the two other poses)
        _check_invariants(pkg, objs, s["rect"], poses[p], singles[p])
    qs = []
    for p in range(3):
        qp = q.copy(); qp["pose"] = p; qs.append(qp)
    mixed = np.stack(qs, 1).reshape(-1)                                                 # query i of pose 0, of pose 1, of pose 2, query i + 1, ...
    got = pkg.probe_scene(objs, mixed, poses)
    for p in range(3):
        _same_bits([a[p::3] for a in got], singles[p], "pose %d of 3" % p)
    for p in (1, 2):                                                                    # the other poses see the objects too, and differently
        assert (singles[p][2] > 0.5).sum() >= 20 and not np.array_equal(_bits(singles[p][0]), _bits(base[0]))


def test_hit_outputs(pkg, setup):
    """Test 3: each object's lists of the rect (mon_debug_scene_samples) merged in NumPy with ties to the lower object index, then the lower slot, T in
    fp64: hit_depth is t_i / dn of the reference's first crossing exactly and hit_instance its object, rays near a tie left out on both sides (at most
    1 % of the opaque ones).  At least 50 rays have a hit and at least 10 hold samples of two objects whose t ranges overlap (the overlap view's rect
    gives them: object 0's inflated box reaches into the others)."""
    s = setup; objs = s["objs3"]
    t, a, c, n, dn = _check_invariants(pkg, objs, s["rect"], s["pose"], s["base"])
    has, near = _check_hits(s["base"], t, a, n, dn)
    assert int((has & ~near).sum()) >= 50
    lo = np.where(n > 0, t[..., 0], np.inf); hi = np.where(n > 0, np.take_along_axis(t, np.maximum(n.astype(np.int64) - 1, 0)[..., None], 2)[..., 0], -np.inf)
    inter = np.zeros(n.shape[1], bool)
    for i in range(3):
        for j in range(i + 1, 3):
            inter |= (n[i] > 0) & (n[j] > 0) & (lo[i] < hi[j]) & (lo[j] < hi[i])
    assert int(inter.sum()) >= 10, int(inter.sum())
    # the hit depth is a sample distance in front of (or at) the smeared depth's far end: where two objects are crossed it names the front one
    hit = s["base"][5] >= 0
    assert (s["base"][4][hit] > 0).all()


# the adversarial cases of test 4: tests/test_scene_render.py's recipe (_adversarial), per (K, equal_t) one generator seeded 300 + K + 7 equal_t that draws
# 700 rays with alpha_hi 0.3 (0.6 for K = 1: most rays end at the cut) and 1 000 rays with alpha_hi 0.1 (for K <= 3 almost no ray reaches the cut: every
# block and list is walked).  A ray is near a tie with probability about 2 TIE / mean alpha, so smaller alphas would pass the cap: alpha_hi 0.02 gave up to
# 2 % on 300 rays.  The near-tie shares of these draws, from np_first_hit on the CPU before any GPU run: at most 0.74 % of the opaque rays (4 of 538).
ADVERSARIAL = [(K, eq) for K in (1, 3, 16) for eq in (False, True)]


def adversarial_draws(K, equal_t):
    rng = np.random.RandomState(300 + K + 7 * int(equal_t))
    return [tsr._adversarial(rng, K, 700, equal_t, alpha_hi=0.3 if K > 1 else 0.6), tsr._adversarial(rng, K, 1000, equal_t, alpha_hi=0.1)]


@pytest.mark.parametrize("K,equal_t", ADVERSARIAL)
def test_composite_hook_on_adversarial_lists(pkg, K, equal_t):
    """Test 4: mon_debug_scene_probe_composite on _adversarial's lists: the four old outputs are mon_debug_scene_composite's bits, the hit outputs agree
    with the NumPy reference under test 3's near-tie rule and 1 % cap."""
    for t, alpha, rgb, count, dn in adversarial_draws(K, equal_t):
        got = pkg.scene_probe_composite(t, alpha, rgb, count, dn)
        _same_bits(got[:4], pkg.scene_composite(t, alpha, rgb, count, dn), (K, equal_t))
        _check_hits(got, t, alpha, count, dn)


def test_composite_hook_edge_rows(pkg):
    """Test 4's edge rows: an empty list, a single sample, 64 samples of alpha 0 (no hit), a first sample of alpha 0.6 (a hit at slot 0) -- and the same
    with the sample in the last of three lists."""
    rng = np.random.RandomState(9)
    for K, k in ((1, 0), (3, 2)):
        t, alpha, rgb, count, dn = tsr._adversarial(rng, K, 5)
        count[:] = 0; alpha[:] = 0.25
        count[k, 1] = 1; alpha[k, 1, 0] = 0.3                       # a single sample that does not stop the ray
        count[k, 2] = 64; alpha[k, 2] = 0.0                        # 64 samples of alpha 0
        count[k, 3] = 64; alpha[k, 3, 0] = 0.6                     # the first sample stops the ray
        count[k, 4] = 1; alpha[k, 4, 0] = 0.75                     # a single sample that does
        got = pkg.scene_probe_composite(t, alpha, rgb, count, dn)
        _same_bits(got[:4], pkg.scene_composite(t, alpha, rgb, count, dn), K)
        assert got[5].tolist() == [-1, -1, -1, k, k]
        assert got[4][:3].tolist() == [0.0, 0.0, 0.0]
        assert got[4][3] == t[k, 3, 0] / dn[3] and got[4][4] == t[k, 4, 0] / dn[4]
        assert (got[0][0] == 1.0).all() and got[2][0] == 0.0 and got[3][0] == -1 and (got[0][2] == 1.0).all() and got[2][2] == 0.0
        _check_hits(got, t, alpha, count, dn, cap=1.0)


def ref_rays(K, Twc, Tow, mn, mx, u, v):
    """fp64 restatement of pixel_ray and ray_intersect (device_common.h) on the fp32 inputs, with the forward error bounds of their fp32 evaluation.
    Counting roundings (each at most U = 2^-24 relative to its result, first order):
      dn = |camera ray|      sub, div, mul, fma, fma, sqrt                                  ->  6 U dn
      d  = Row Rwc dc / dn   the six above, the division by dn, two rot3 of (mul, fma, fma)  -> 13 ops; squaring doubles the error of dc, so 14 U Md,
                             Md = |Row| |Rwc| |dc / dn| (the magnitude of the terms summed)
      o  = Row twc + tow     one rot3 and one add                                            ->  4 U Mo, Mo = |Row| |twc| + |tow|
      a slab distance        t = (b - o) / d: the subtraction's rounding, o's and d's errors, the division's rounding
                             -> (Eo + U (|b| + |o|)) / |d| + |t| (Ed / |d| + U)
      t0 = the largest near distance, t1 = the smallest far one (max and min do not amplify)  -> the largest of the six slab bounds.
    Returns o, d, dn, t0 (before the clamp at 0), t1, hit and the bounds Eo, Ed, Edn, Et (Et = inf where a component of d is within its bound of 0)."""
    fx, fy, cx, cy = (np.float64(np.float32(x)) for x in K)
    Twc = np.asarray(Twc, np.float32).astype(np.float64).reshape(4, 4).T; Tow = np.asarray(Tow, np.float32).astype(np.float64).reshape(4, 4).T
    mn = np.asarray(mn, np.float32).astype(np.float64); mx = np.asarray(mx, np.float32).astype(np.float64)
    u = np.asarray(u, np.float32).astype(np.float64); v = np.asarray(v, np.float32).astype(np.float64)
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    dn = np.sqrt((dc * dc).sum(-1)); dcn = dc / dn[:, None]
    Rwc, twc, Row, tow = Twc[:3, :3], Twc[:3, 3], Tow[:3, :3], Tow[:3, 3]
    d = dcn @ Rwc.T @ Row.T
    o = np.broadcast_to(Row @ twc + tow, d.shape)
    Ed = 14 * U * (np.abs(dcn) @ np.abs(Rwc).T @ np.abs(Row).T)
    Eo = np.broadcast_to(4 * U * (np.abs(Row) @ np.abs(twc) + np.abs(tow)), d.shape)
    Edn = 6 * U * dn
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (mn - o) / d, (mx - o) / d
        near, far = np.minimum(ta, tb), np.maximum(ta, tb)
        t0, t1 = near.max(-1), far.min(-1)
        Et = np.zeros(len(u))
        for b, t in ((mn, ta), (mx, tb)):
            Et = np.maximum(Et, ((Eo + U * (np.abs(b) + np.abs(o))) / np.abs(d) + np.abs(t) * (Ed / np.abs(d) + U)).max(-1))
    Et = np.where((np.abs(d) <= 2 * Ed).any(-1) | ~np.isfinite(Et), np.inf, Et)
    return o, d, dn, t0, t1, t0 <= t1, Eo, Ed, Edn, Et


def test_subpixel_rays(pkg, ss, setup):
    """Test 5: fractional (u, v), inside and outside the image, under three poses, for each of the three objects: the rows of
    mon_debug_scene_probe_rays against ref_rays within its bounds; the flag agrees except where the reference's slab distances tie within the bound.
    Integer-valued queries give the rows k_render_rays writes for that pixel, bit for bit."""
    s = setup; sc = s["sc"]; objs = s["objs3"]
    lst = [s["objs"]["a0"], s["objs"]["a1"], s["objs"]["a2"], s["objs"]["b0"]]           # the three true boxes, and object 0's box inflated 5 x
    rng = np.random.RandomState(5); N = 6000
    u = rng.uniform(-60.0, sc.W + 60.0, N).astype(np.float32); v = rng.uniform(-45.0, sc.H + 45.0, N).astype(np.float32)
    views = [s["v"], 2, 13]; poses = np.stack([tsr._pose(ss, sc, w) for w in views])
    q = pkg.scene_queries(rng.randint(0, 3, N), np.arange(N), u, v)
    outside = (u < 0) | (u > sc.W - 1) | (v < 0) | (v > sc.H - 1)
    assert outside.sum() > 200 and (u != np.round(u)).all()
    Kc = (sc.fx, sc.fy, sc.cx, sc.cy)
    flags = []
    for k, (idx, infl) in enumerate(((0, 1.0), (1, 1.0), (2, 1.0), (0, 5.0))):
        ob = sc.objects[idx]; half = (ob["half"] * infl).astype(np.float32)
        rows = pkg.scene_probe_rays(lst, q, poses, k)
        flag = rows[:, 8] > 0; flags.append(flag)
        worst = dict(o=0.0, d=0.0, dn=0.0, t=0.0); n_tie = 0
        for p in range(3):
            m = q["pose"] == p
            o, d, dn, t0, t1, hit, Eo, Ed, Edn, Et = ref_rays(Kc, poses[p], ss.colmajor(ob["Tow"]), -half, half, u[m], v[m])
            r = rows[m].astype(np.float64); f = flag[m]
            assert (np.abs(r[:, 9] - dn) <= Edn).all()
            sure = np.abs(t1 - t0) > 2 * Et                                           # the slab distances do not tie within the bound
            n_tie += int((~sure).sum())
            assert np.array_equal(f[sure], hit[sure])
            g = f & hit & np.isfinite(Et)
            assert (np.abs(r[g, 0:3] - o[g]) <= Eo[g]).all() and (np.abs(r[g, 3:6] - d[g]) <= Ed[g]).all()
            assert (np.abs(r[g, 6] - np.maximum(t0[g], 0.0)) <= Et[g]).all() and (np.abs(r[g, 7] - t1[g]) <= Et[g]).all()
            assert (r[~f][:, :8] == 0).all()
            for key, err, bound in (("o", np.abs(r[g, 0:3] - o[g]) / Eo[g], None), ("d", np.abs(r[g, 3:6] - d[g]) / Ed[g], None),
                                    ("dn", np.abs(r[:, 9] - dn) / Edn, None), ("t", np.abs(r[g, 7] - t1[g]) / Et[g], None)):
                if err.size:
                    worst[key] = max(worst[key], float(err.max()))
        print("object %d: %d hits of %d, %d rows within the tie bound, largest error / bound %s" % (k, int(flag.sum()), N, n_tie, worst))
        assert flag.sum() > 30 and n_tie < 0.02 * N
    none = ~(flags[0] | flags[1] | flags[2])
    assert none.sum() > 20                                                             # some rays miss every one of the three true boxes
    out = pkg.probe_scene(lst[:3], q, poses)
    assert (out[0][none] == 1.0).all() and (out[1][none] == 0.0).all() and (out[2][none] == 0.0).all() and (out[3][none] == -1).all()
    assert (out[4][none] == 0.0).all() and (out[5][none] == -1).all()
    # integer-valued queries: the rows k_render_rays leaves in the object's render rays after a scene render of the rect on side 0
    rect, pose = s["rect"], s["pose"]; P = s["q"].shape[0]; n_with_hits = 0
    for k, o in enumerate(objs):
        rows = pkg.scene_probe_rays(objs, s["q"], pose, k)
        pkg.render_scene([o], rect, pose, 0)
        flag = o.buffer("ray_flag")[:P]; hit = flag != 0
        assert np.array_equal(rows[:, 8] != 0, hit) and np.array_equal(_bits(rows[:, 9]), _bits(o.buffer("ray_dn")[:P]))
        assert np.array_equal(_bits(rows[:, 0:3])[hit], _bits(o.buffer("ray_o")[:3 * P].reshape(P, 3))[hit])
        assert np.array_equal(_bits(rows[:, 3:6])[hit], _bits(o.buffer("ray_d")[:3 * P].reshape(P, 3))[hit])
        assert np.array_equal(_bits(rows[:, 6])[hit], _bits(o.buffer("ray_t0")[:P])[hit])
        assert np.array_equal(_bits(rows[:, 7])[hit], _bits(o.buffer("ray_t1")[:P])[hit])
        n_with_hits += int(hit.sum() > 0)
    assert n_with_hits >= 2                                                            # (the rect need not see the third box)


def test_misses(pkg, ss, setup):
    """Test 6: queries whose rays hit no box (a camera that looks past every box, at sub-pixel points; alone and next to a pose that does hit) give
    rgb 1, depth 0, opacity 0, instance -1, hit_depth 0, hit_instance -1."""
    s = setup; objs = s["objs"]; lst = [objs["a0"], objs["a1"], objs["a2"]]
    away = ss.colmajor(ss._look_at(np.array([0.0, 0.0, 3.0]), np.array([10.0, 0.0, 3.0])))
    rng = np.random.RandomState(2); n = 300
    u = rng.uniform(0.0, s["sc"].W - 1.0, n).astype(np.float32); v = rng.uniform(0.0, s["sc"].H - 1.0, n).astype(np.float32)
    q = pkg.scene_queries(0, np.arange(n), u, v)
    for k in range(3):
        assert (pkg.scene_probe_rays(lst, q, away, k)[:, 8] == 0).all()
    both = np.concatenate([q, s["q"]]); both["pose"][n:] = 1
    for out in (pkg.probe_scene(lst, q, away), [a[:n] for a in pkg.probe_scene(lst, both, np.stack([away, s["pose"]]))]):
        assert (out[0] == 1.0).all() and (out[1] == 0.0).all() and (out[2] == 0.0).all() and (out[3] == -1).all()
        assert (out[4] == 0.0).all() and (out[5] == -1).all()


def test_mixed_network_shapes(pkg, setup):
    """Test 8: a 32 x 2 object and a 64 x 1 object probed together (each through its own keyed instantiation), as the scene render's test of mixed shapes:
    the bit rule of test 1 holds."""
    s = setup; objs = s["objs"]
    for lst in ([objs["n2"], objs["a1"]], [objs["a1"], objs["b0"], objs["n2"]]):
        want = pkg.render_scene(lst, s["rect"], s["pose"])
        got = pkg.probe_scene(lst, s["q"], s["pose"])
        _same_bits(got[:4], want, len(lst))
        assert (want[2] > 0.5).sum() >= 50
        _check_invariants(pkg, lst, s["rect"], s["pose"], got)


def _state(o):
    i = o.info()
    return [o.get_params(0), o.get_params(1), o.get_params(2)], tuple(getattr(i, f) for f, _ in type(i)._fields_), (o.render_skip_stats(0), o.render_skip_stats(1))


def _same_state(a, b):
    assert all(np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y) for x, y in zip(a[0], b[0]))
    assert a[1] == b[1] and a[2] == b[2]


def test_read_only(pkg, setup):
    """Test 9: parameters (all three copies), mon_object_info_get and the skip statistics of both sides are identical before and after probes on both
    sides, with skipping off and on (the grids built beforehand, as a scene render builds them); a training step after a probe gives the parameters the
    same step gives without it."""
    s = setup; sc = s["sc"]; ds, _ = None, None
    objs = s["objs3"]
    for skip in (False, True):
        for o in objs:
            o.set_render_skip(skip, 1e-3)
        for side in (0, 1):
            pkg.render_scene(objs, s["rect"], s["pose"], side)                         # (skip on: this builds the side's grids where they are stale)
        before = [_state(o) for o in objs]
        for side in (0, 1):
            pkg.probe_scene(objs, s["q"], s["pose"], side)
        for o, b in zip(objs, before):
            _same_state(_state(o), b)
    for o in objs:
        o.set_render_skip(False)
    ds, a = ge.make_problem(pkg, sc, tsr.BASE)
    _, b = ge.make_problem(pkg, sc, tsr.BASE, dataset=ds)
    try:
        a.set_backend(1); b.set_backend(1); a.train(20); b.train(20)
        for side in (0, 1):
            pkg.probe_scene([a], s["q"], s["pose"], side)
        a.train(1); b.train(1)
        for w in (0, 1, 2):
            x, y = a.get_params(w), b.get_params(w)
            assert np.array_equal(x.view(np.uint32) if w == 0 else x, y.view(np.uint32) if w == 0 else y), w
    finally:
        a.close(); b.close(); ds.close()


def test_online(pkg, ss, setup):
    """Test 10: before any publication mon_online_probe_scene returns MON_ERR_STATE; a second thread calls it ten times while the manager's objects still
    train (every call MON_OK with finite outputs); once they are idle it equals mon_online_render_scene over a rect's pixels bit for bit and
    mon_scene_probe(side 1) of the manager's objects, with the manager's indices in both instance outputs."""
    s = setup; sc = s["sc"]
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    v = 7; frame = tsr._frame(sc, v); rect = np.array([v, 140, 108, 24, 40], np.uint32); pose = tsr._pose(ss, sc, v)
    q = pkg.rect_queries(rect); q_frame = pkg.rect_queries(frame)
    with pytest.raises(pkg.MonError) as e:
        m.probe_scene(q, pose)
    assert e.value.code == 5
    seen = dict(n=0, err=None)

    def front_end():
        try:
            for _ in range(10):
                out = m.probe_scene(q, pose)
                assert all(np.isfinite(a).all() for a in out) and set(np.unique(out[3])) <= {-1, 0, 1, 2} and set(np.unique(out[5])) <= {-1, 0, 1, 2}
                seen["n"] += 1
        except Exception as ex:        # noqa: BLE001 -- reported by the main thread
            seen["err"] = ex

    calls = 100
    ids = tsr._online_feed(pkg, ss, sc, m, 3, calls)
    assert tsr._wait_trained(m, ids, 2)                                                # every object has published
    th = threading.Thread(target=front_end); th.start(); th.join(timeout=120)
    still = [m.object_info(i)["train_calls"] for i in ids]
    m.wait_threads_end()
    assert seen["err"] is None and seen["n"] == 10, seen
    print("online: train calls when the ten probes were through:", still)
    assert min(still) < calls                                                           # they were still training
    want = m.render_scene(frame, pose)                                                  # (the whole frame: five passes of queries)
    got = m.probe_scene(q_frame, pose)
    _same_bits(got[:4], want, "online")
    _same_bits(got, pkg.probe_scene([m.object(i) for i in ids], q_frame, pose, side=1), "side 1")
    assert (got[2] > 0.5).mean() > 0.02 and set(np.unique(got[5])) - {-1} and set(np.unique(got[5])) <= {-1, 0, 1, 2}
    m.close()
