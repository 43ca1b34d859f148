"""GPU tests (-m gpu) of the scene composite kernels at 17 to 256 lists (kSceneMaxLists): k_scene_composite, k_scene_probe_composite,
k_scene_cast_composite and k_scene_composite_grad through their debug entries on the synthetic lists of tests/test_scene_many_lists_reference.py, and
whole routes (render, samples, probe, cast, pose loss and its batch: k_scene_composite_loss) with 70 and 130 objects.  One wave handles one ray, so every
loop over lists runs in groups of 64: these are the cases that make a second, third and fourth trip through them (compaction across ballot groups, merged
sequences of up to 16 384 samples, 64 different lists in one block, the arg-max and the mask loss over more than 64 lists, 37 888 / 39 936 B of LDS,
and the two-float transmittance scan that sequences of more than 1 024 samples take).
The references are the suite's fp64 restatements; every bar is max(the bar of the kernel's K <= 16 test, 4 E_seq) with E_seq the error of an fp32
sequential evaluation of the same lists against fp64 (computed per case on the CPU, in the reference file); rays whose cut lies within
max(1e-3, 4 (i + 1) 2^-24) of 1e-4 are left out (at most 2 %).  Padding is held to the bit: 16 lists scattered over 256 slots give the bits of the 16.

Hits (probe, cast): regimes whose crossing is sharp (the wall, alpha of 0.15 and more) keep the 1 % cap of tests/test_scene_probe.py on rays near a
tie; where alpha is a few 1e-4 most rays lie within TIE of the threshold (about 2 TIE / mean alpha of them) and the hits are compared on the others."""
import numpy as np
import pytest

from conftest import ROOT                                    # noqa: F401
import test_scene_cast as tsc                               # noqa: E402
import test_scene_many_lists_reference as mlr               # noqa: E402
import test_scene_probe as tsp                              # noqa: E402
import test_scene_render as tsr                             # noqa: E402
import test_scene_track as tst                              # noqa: E402
from test_scene_render import scene, trained, overlap_view   # noqa: F401,E402 -- the module-scoped fixtures of the scene render's tests
from test_scene_track import COMP_GRAD_BAR                   # noqa: E402

pytestmark = pytest.mark.gpu
_bits, _same_bits = tsp._bits, tsp._same_bits


@pytest.fixture(scope="module", params=mlr.CASES, ids=mlr.case_id)
def case(request):
    """One case with its references and bars (tests are grouped by case: each is computed once)."""
    return mlr.Case(request.param)


def _report(c, kernel, errs):
    """one line per case and kernel: every quantity's worst error next to its bar, and the worst ratio"""
    worst = max(errs[k] / c.bar[k] for k in errs)
    print("MANY %s %s: %s worst error / bar %.3f" % (mlr.case_id(c.case), kernel, ", ".join("%s %.2e / %.2e" % (k, errs[k], c.bar[k]) for k in errs), worst))


# ------------------------------------------------------------------ 1. the kernels on synthetic lists
def _composite_errors(c, got):
    ref_rgb, ref_d, ref_op, ref_inst, wk, amb = c.ref
    ok = ~amb
    on = ok & (ref_op > 0.5 + 1e-4) & (got[2] > 0.5)
    errs = dict(rgb=float(np.abs(got[0] - ref_rgb)[ok].max()), opacity=float(np.abs(got[2] - ref_op)[ok].max()),
                depth=float(((np.abs(got[1] - ref_d)[on] - 1e-6) / np.abs(ref_d[on])).max()) if on.any() else 0.0)
    return errs, ok, on


def test_composite(pkg, case):
    """mon_debug_scene_composite: rgb, opacity and depth within the case's bars of np_composite, the instance exact away from opacity 0.5 and from
    near-ties of the per-list weights.
    Measured on an MI355X, worst error / bar: 0.20 up to K = 65 (ties_through-K64), 0.22 from K = 128 on (ties_through-K256: rgb 3.15e-6 against
    1.52e-5); at 16 384 samples rgb 5.28e-6 against 3.02e-5.  With the plain tile scan on every sequence the cases of small alpha missed the bar from
    K = 128 on (1.02 to 1.25 at K = 128 / 129, up to 1.65 at K = 256: opacity 1.90e-5 against 1.15e-5; 3.38e-5 at 16 384 samples): that scan loses
    the term a b of every product (1 - a)(1 - b) below 2^-12, a drift that grows with the sample count, and sequences of more than kSceneLongSeq
    samples now take scan_mul32_comp (scene_device.h)."""
    c = case; t, alpha, rgb, count, dn = c.lists
    got = pkg.scene_composite(t, alpha, rgb, count, dn)
    errs, ok, on = _composite_errors(c, got)
    _report(c, "composite", errs)
    ref_rgb, ref_d, ref_op, ref_inst, wk, amb = c.ref
    assert errs["rgb"] <= c.bar["rgb"] and errs["opacity"] <= c.bar["opacity"]
    assert (np.abs(got[1] - ref_d)[on] <= c.bar["depth"] * np.abs(ref_d[on]) + 1e-6).all()
    far = ok & (np.abs(ref_op - 0.5) > 1e-4) & ~tsr._near_tie(wk)
    assert far.sum() >= 0.9 * ok.sum() - 1
    assert np.array_equal(got[3][far], ref_inst[far])
    assert (got[3][far & (ref_op > 0.5)] >= 0).all()


def test_probe_composite(pkg, case):
    """mon_debug_scene_probe_composite: the four old outputs are mon_debug_scene_composite's bits; hit_depth and hit_instance are np_first_hit's
    first crossing exactly, rays near a tie left out."""
    c = case; t, alpha, rgb, count, dn = c.lists
    got = pkg.scene_probe_composite(t, alpha, rgb, count, dn)
    _same_bits(got[:4], pkg.scene_composite(t, alpha, rgb, count, dn), c.case)
    has, near = tsp._check_hits(got, t, alpha, count, dn, cap=mlr.HIT_CAP if c.regime in mlr.SHARP else 1.0)
    if c.regime in mlr.SHARP:
        assert (has & ~near).sum() >= 10


def test_cast_composite(pkg, case):
    """mon_debug_scene_cast_composite at the thresholds 0.5 and 0.8: rgb, dist / dn, opacity and instance are mon_debug_scene_composite's bits;
    hit_sample_t and hit_instance are np_crossing's first crossing, hit_t lies within its first-order bound; at 0.5 the hit is the probe's."""
    c = case; t, alpha, rgb, count, dn = c.lists
    want = pkg.scene_composite(t, alpha, rgb, count, dn)
    worst = 0.0
    for thr in mlr.CAST_THR:
        got = pkg.scene_cast_composite(t, alpha, rgb, count, c.entry, thr)
        _same_bits((got[0], (got[1] / dn).astype(np.float32), got[2], got[3]), want, (c.case, thr))
        worst = max(worst, tsc._check_crossing(got, t, alpha, count, c.entry, thr, cap=mlr.HIT_CAP if c.regime in mlr.SHARP else 1.0))
        if thr == 0.5:
            probe = pkg.scene_probe_composite(t, alpha, rgb, count, dn)
            _same_bits(((got[5] / dn).astype(np.float32), got[6]), probe[4:], "the probe's hit")
    print("MANY %s cast: hit_t worst error / bound %.3f" % (mlr.case_id(c.case), worst))


def test_composite_grad(pkg, case):
    """mon_debug_scene_composite_grad: l, W_j, D and every dL/dalpha and dL/dc within the case's bars of np_composite_grad (errors relative to the
    case's largest magnitude of the quantity, as tests/test_scene_track.py measures them); a ray with no list gives zeros.
    Measured on an MI355X, worst error / bar: 0.34 up to K = 65 (ties_wall-K17), 0.26 from K = 128 on (through-K128); at 16 384 samples dL/dalpha
    3.38e-6 against 2.43e-5.  (With the plain tile scan on every sequence: up to 2.76 at K = 256, dL/dalpha 3.55e-5 against 1.29e-5 -- test_composite's
    drift, the forward's transmittance being the same scan.)"""
    c = case; t, alpha, rgb, count, dn = c.lists; cstar, mstar, dstar = c.targets
    got = pkg.scene_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, *mlr.GRAD_W)
    ref = c.gref; ok = ~c.amb
    sel = lambda k, v: v[ok] if k in ("l", "D") else v[:, ok]                               # noqa: E731
    errs = {k: mlr._rel(sel(k, got[k]), sel(k, ref[k])) for k in mlr.GRAD_KEYS}
    _report(c, "composite_grad", errs)
    for k in mlr.GRAD_KEYS:
        assert errs[k] <= c.bar[k], (k, errs[k], c.bar[k])
    none = count.sum(0) == 0
    assert (got["dalpha"][:, none] == 0).all() and (got["W"][:, none] == 0).all() and (got["D"][none] == 0).all()
    empty = count == 0                                                                  # an empty list receives nothing and weighs nothing
    assert (got["W"][empty] == 0).all() and (got["dalpha"][empty] == 0).all() and (got["dc"][empty] == 0).all()


# ------------------------------------------------------------------ padding invariance: to the bit
PAD_REGIMES = ("through", "early", "wall", "ties_through", "ties_wall", "full_through", "singles")
PAD_TABLES = dict(spread=(16, mlr.SLOTS_SPREAD), packed=(16, mlr.SLOTS_PACKED), three=(3, mlr.SLOTS_THREE))


@pytest.mark.parametrize("table", sorted(PAD_TABLES))
@pytest.mark.parametrize("regime", PAD_REGIMES)
def test_padding_changes_no_bit(pkg, regime, table):
    """K = 16 (3) lists of each regime -- sizes the K <= 16 tests hold to numpy -- scattered, order kept, over 256 slots whose others are empty:
    compaction yields the same compact sequence, so rgb, depth, opacity, the probe's and the cast's hit outputs come back in the same bits, instances map
    through the slot table, W, D, dL/dalpha and dL/dc at the occupied slots are the same bits and zero elsewhere.  Only l has a tolerance
    (COMP_GRAD_BAR): its mask term is summed per group of 64 lists, and the groups change."""
    K, slots = PAD_TABLES[table]; R = 64; sl = np.asarray(slots)
    seed = 700 + 10 * mlr.REGIMES.index(regime) + K
    t, alpha, rgb, count, dn = mlr.make_lists(regime, K, R, seed)
    if regime == "singles":                                                               # (16 samples of alpha 0.05 stop no ray: some must, for the instance)
        alpha = np.minimum(alpha * np.float32(18.0), np.float32(0.95))
    T, A, C, N = mlr.scatter((t, alpha, rgb, count), slots, 256)
    remap = lambda i: np.where(i >= 0, sl[np.maximum(i, 0)], -1)                            # noqa: E731
    a = pkg.scene_composite(t, alpha, rgb, count, dn); b = pkg.scene_composite(T, A, C, N, dn)
    assert (a[2] > 0.5).any() and (a[3] >= 0).any()
    _same_bits(a[:3], b[:3], "composite"); assert np.array_equal(remap(a[3]), b[3])
    a = pkg.scene_probe_composite(t, alpha, rgb, count, dn); b = pkg.scene_probe_composite(T, A, C, N, dn)
    _same_bits(a[:3] + a[4:5], b[:3] + b[4:5], "probe"); assert np.array_equal(remap(a[3]), b[3]) and np.array_equal(remap(a[5]), b[5])
    assert (a[5] >= 0).any()
    entry = tsc._entries(t, seed + 2); (E,) = mlr.scatter((entry,), slots, 256)
    for thr in (0.2, 0.5, 0.8):
        a = pkg.scene_cast_composite(t, alpha, rgb, count, entry, thr); b = pkg.scene_cast_composite(T, A, C, N, E, thr)
        _same_bits(a[:3] + a[4:6], b[:3] + b[4:6], ("cast", thr)); assert np.array_equal(remap(a[3]), b[3]) and np.array_equal(remap(a[6]), b[6])
    D = tsr.np_composite(t, alpha, rgb, count, dn.astype(np.float64))[1]
    cstar, mstar, dstar = mlr.make_targets(t, count, D, seed)
    (M,) = mlr.scatter((mstar,), slots, 256)
    a = pkg.scene_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, *mlr.GRAD_W)
    b = pkg.scene_composite_grad(T, A, C, N, cstar, M, dstar, dn, *mlr.GRAD_W)
    assert np.abs(a["dalpha"]).max() > 0 and np.abs(a["dc"]).max() > 0
    for k in ("W", "dalpha", "dc"):
        assert np.array_equal(_bits(a[k]), _bits(b[k][sl])), k
        assert (np.delete(b[k], sl, 0) == 0).all(), k                                      # (dL/dc = w G: a zero of either sign)
    assert np.array_equal(_bits(a["D"]), _bits(b["D"]))
    assert mlr._rel(b["l"], a["l"].astype(np.float64)) <= COMP_GRAD_BAR


def test_edge_cases_at_256_lists(pkg):
    """K = 256: every list empty (the background exactly, instance -1, no hit, zero gradients); a single non-empty list, at slot 255 (the bits of
    that list alone); an opaque first sample held by list 200 (rgb its colour exactly, opacity 1, instance 200, the hit there) --
    test_composite_kernel_edge_cases' recipe."""
    rng = np.random.RandomState(4); K, R = 256, 64
    t, alpha, rgb, count, dn = tsr._adversarial(rng, K, R)
    entry = tsc._entries(t, 5)
    zero = np.zeros_like(count)
    got = pkg.scene_composite(t, alpha, rgb, zero, dn)
    assert (got[0] == 1.0).all() and (got[1] == 0.0).all() and (got[2] == 0.0).all() and (got[3] == -1).all()
    got = pkg.scene_probe_composite(t, alpha, rgb, zero, dn)
    assert (got[0] == 1.0).all() and (got[2] == 0.0).all() and (got[3] == -1).all() and (got[4] == 0.0).all() and (got[5] == -1).all()
    got = pkg.scene_cast_composite(t, alpha, rgb, zero, entry, 0.5)
    assert (got[0] == 1.0).all() and (got[2] == 0.0).all() and (got[3] == -1).all() and (got[4] == 0.0).all() and (got[5] == 0.0).all() and (got[6] == -1).all()
    cstar = rng.uniform(0, 1, (R, 3)).astype(np.float32); mstar = np.zeros((K, R), np.float32); mstar[7] = 1.0; dstar = np.full(R, 1.5, np.float32)
    g = pkg.scene_composite_grad(t, alpha, rgb, zero, cstar, mstar, dstar, dn, *mlr.GRAD_W)
    assert (g["W"] == 0).all() and (g["D"] == 0).all() and (g["dalpha"] == 0).all() and (g["dc"] == 0).all()
    # l = w_mask (0 - 1)^2 + w_depth Huber(0 - 1.5) = 1 + 0.05 (1.5 - 0.025): the rgb residual is zero
    assert np.allclose(g["l"], 1.0 + 0.05 * (1.5 - 0.025), rtol=1e-6)
    # a single non-empty list, at slot 255
    one = zero.copy(); one[255] = count[255]; one[255, :8] = 64
    a = pkg.scene_probe_composite(t[255:], alpha[255:], rgb[255:], one[255:], dn); b = pkg.scene_probe_composite(t, alpha, rgb, one, dn)
    assert (a[3] == 0).any()
    _same_bits(a[:3] + a[4:5], b[:3] + b[4:5], "one list")
    assert np.array_equal(np.where(a[3] >= 0, 255, -1), b[3]) and np.array_equal(np.where(a[5] >= 0, 255, -1), b[5])
    _same_bits(pkg.scene_composite(t, alpha, rgb, one, dn)[:3], b[:3])
    ga = pkg.scene_composite_grad(t[255:], alpha[255:], rgb[255:], one[255:], cstar, mstar[255:], dstar, dn, *mlr.GRAD_W)
    gb = pkg.scene_composite_grad(t, alpha, rgb, one, cstar, mstar * 0, dstar, dn, *mlr.GRAD_W)
    for k in ("W", "dalpha", "dc"):
        assert np.array_equal(_bits(ga[k][0]), _bits(gb[k][255])) and (gb[k][:255] == 0).all(), k
    # an opaque first sample, held by list 200
    count[:] = 64; alpha[:] = 0.2
    t[200, :, 0] = np.float32(0.25); alpha[200, :, 0] = 1.0                               # (every other t >= 0.5)
    got = pkg.scene_cast_composite(t, alpha, rgb, count, entry, 0.5)
    assert np.array_equal(got[0], rgb[200, :, 0]) and (got[2] == 1.0).all() and (got[3] == 200).all()
    assert (got[6] == 200).all() and (got[5] == t[200, :, 0]).all() and np.array_equal(got[4], entry[200])          # alpha 1: f = 0, hit_t = the entry
    got = pkg.scene_probe_composite(t, alpha, rgb, count, dn)
    assert np.array_equal(got[0], rgb[200, :, 0]) and (got[2] == 1.0).all() and (got[3] == 200).all() and (got[5] == 200).all()
    assert np.array_equal(_bits(got[1]), _bits((t[200, :, 0] / dn).astype(np.float32))) and np.array_equal(_bits(got[4]), _bits(got[1]))
    _same_bits(pkg.scene_composite(t, alpha, rgb, count, dn), got[:4])


# ------------------------------------------------------------------ 2. whole routes with more than 64 objects
RECT_H, RECT_W = 24, 32


@pytest.fixture(scope="module")
def routes(pkg, ss, scene, trained, overlap_view):       # noqa: F811
    """The trained objects b0, a1, a2 (object 0 on its inflated box) of the overlap view, a 32 x 24 rect of it that holds background, one object alone
    and two overlapping, and what the routes give for the three objects alone before any large call: computed once, left unchanged."""
    sc = scene; _, objs = trained; v, i, j = overlap_view
    three = [objs["b0"], objs["a1"], objs["a2"]]
    for o in three:
        o.set_render_skip(False)
    rect = tsp._pick_rect(sc, v, i, j, h=RECT_H, w=RECT_W); pose = tsr._pose(ss, sc, v)
    q = pkg.rect_queries(rect)
    rays, dn = pkg.camera_rays(tsc._K(sc), pose, q)
    boxes = tst._view_boxes(sc, v, (0, 1)); prm = pkg.pose_refine_default(rays_per_iter=256)
    poses = np.stack([pose, pose, pose, pose])
    poses[1, 12] += np.float32(0.03); poses[2, 13] -= np.float32(0.02); poses[3, 14] += np.float32(0.01)
    s = dict(sc=sc, three=three, rect=rect, pose=pose, q=q, rays=rays, dn=dn, boxes=boxes, prm=prm, poses=poses)
    s["before"] = _small_calls(pkg, s)
    return s


def _lists(q):
    """a dumped list with the slots behind its count zeroed (they hold whatever the workspace held): t, alpha, rgb, count"""
    t, a, c, n = q
    valid = np.arange(64)[None, None, :] < n[..., None]
    return np.where(valid, t, np.float32(0)), np.where(valid, a, np.float32(0)), np.where(valid[..., None], c, np.float32(0)), n


def _small_calls(pkg, s):
    """every route with the three objects alone, both sides, as raw bits"""
    out = []
    for side in (0, 1):
        out += list(pkg.render_scene(s["three"], s["rect"], s["pose"], side)) + list(pkg.probe_scene(s["three"], s["q"], s["pose"], side))
        out += list(pkg.cast_scene(s["three"], s["rays"], 0.5, side))
        out += [pkg.scene_pose_loss_batch(s["three"], s["boxes"], s["poses"], s["prm"], side=side, iteration=3)]
        loss, g6 = pkg.scene_pose_loss(s["three"], s["boxes"], s["pose"], s["prm"], side=side, iteration=3)
        out += [np.float32(loss).reshape(1), g6]
        for k in range(3):
            out += list(_lists(pkg.scene_samples(s["three"], s["rect"], s["pose"], k, side)))
    return [_bits(np.ascontiguousarray(a)).copy() for a in out]


def _route_bars(t, a, c, n, dn64):
    """the bars of item 1 for the dumped lists of a route: max(today's, 4 E_seq), and the rays at the cut's tie"""
    ref = tsr.np_composite(t, a, c, n, dn64, amb_u=mlr.U)
    tw = mlr.np_composite_seq32(t, a, c, n, dn64.astype(np.float32))
    ok = ~ref[5]; on = ok & (ref[2] > 0.5 + 1e-4) & (tw[2] > 0.5)
    e = dict(rgb=float(np.abs(tw[0] - ref[0])[ok].max()), opacity=float(np.abs(tw[2] - ref[2])[ok].max()),
             depth=float((np.abs(tw[1] - ref[1])[on] / np.abs(ref[1][on])).max()))
    return ref, {k: max(1e-5, mlr.MARGIN * v) for k, v in e.items()}


@pytest.mark.parametrize("n_objs", [70, 130])
def test_routes_with_many_objects(pkg, routes, n_objs):
    """70 and 130 handles cycling through three trained objects (equal lists with equal t: the tie rule across many lists), both sides, on the rect:
    render_scene equals np_composite of the dumped lists at item 1's caps and bars; an object's dumped list does not depend on the number of objects
    (k and k + 3 give the same bits, which are the three-object call's); probe_scene and cast_scene agree with their references on the dumped lists and
    with the render's bits; scene_pose_loss_batch of four poses equals four scene_pose_loss calls as raw uint32 (k_scene_composite_loss beyond 64 lists)."""
    s = routes; sc = s["sc"]; rect, pose = s["rect"], s["pose"]
    many = [s["three"][k % 3] for k in range(n_objs)]
    P = RECT_H * RECT_W
    for side in (0, 1):
        out = pkg.render_scene(many, rect, pose, side)
        three_lists = [_lists(pkg.scene_samples(s["three"], rect, pose, k, side)) for k in range(3)]
        for k in (0, 1, 2, 61, 62, 63, 64, 65, n_objs - 4):
            got = _lists(pkg.scene_samples(many, rect, pose, k, side))
            _same_bits(got, _lists(pkg.scene_samples(many, rect, pose, k + 3, side)), ("k and k + 3", k, side))
            _same_bits(got, three_lists[k % 3], ("the three-object call's list", k, side))
        t3 = np.stack([q[0].reshape(P, 64) for q in three_lists]); a3 = np.stack([q[1].reshape(P, 64) for q in three_lists])
        c3 = np.stack([q[2].reshape(P, 64, 3) for q in three_lists]); n3 = np.stack([q[3].reshape(P) for q in three_lists])
        idx = np.arange(n_objs) % 3
        t, a, c, n = t3[idx], a3[idx], c3[idx], n3[idx]                                    # the dumped lists of all n_objs (each checked equal above)
        assert set(np.unique(n).tolist()) <= {0, 32, 64} and n.astype(np.int64).sum(0).max() > 1024      # more than 16 blocks on some ray ...
        assert n_objs < 130 or (n > 0).sum(0).max() > 64                                   # ... and at 130 objects more than 64 non-empty lists
        dn64 = tsr._dn(sc, rect).astype(np.float64)
        ref, bar = _route_bars(t, a, c, n, dn64)
        ref_rgb, ref_d, ref_op, ref_inst, wk, amb = ref
        rgb, depth, op, inst = (x.reshape(-1, 3) if x.ndim == 3 else x.reshape(-1) for x in out)
        ok = ~amb
        assert amb.mean() <= mlr.AMB_CAP
        errs = dict(rgb=float(np.abs(rgb - ref_rgb)[ok].max()), opacity=float(np.abs(op - ref_op)[ok].max()))
        on = ok & (ref_op > 0.5 + 1e-4) & (op > 0.5)
        errs["depth"] = float(((np.abs(depth - ref_d)[on] - 1e-6) / np.abs(ref_d[on])).max())
        print("MANY route-%d side %d render: %s" % (n_objs, side, ", ".join("%s %.2e / %.2e" % (k, errs[k], bar[k]) for k in errs)))
        assert errs["rgb"] <= bar["rgb"] and errs["opacity"] <= bar["opacity"] and errs["depth"] <= bar["depth"]
        assert (ref_op[ok] > 0.5).sum() >= 50 and (ref_op[ok] < 0.5).sum() >= 30
        # equal lists tie in weight: the instance is one of the copies of the winning object, and with ties to the lower list the first copy
        far = ok & (np.abs(ref_op - 0.5) > 1e-4)
        w3 = np.stack([wk[:, idx == k].sum(1) for k in range(3)], 1)
        clear = far & ~tsr._near_tie(w3) & (ref_op > 0.5)
        assert clear.sum() >= 50 and np.array_equal(inst[clear] % 3, w3.argmax(1)[clear]) and (inst[far & (ref_op < 0.5)] == -1).all()
        # the probe and the cast at the same pixels and rays
        probe = pkg.probe_scene(many, s["q"], pose, side)
        _same_bits(probe[:4], out, ("the render's bits", side))
        dn = pkg.scene_probe_rays(many, s["q"], pose, 0, side)[:, 9]
        has, near = tsp._check_hits(probe, t, a, n, dn, cap=mlr.HIT_CAP)
        assert (has & ~near).sum() >= 50
        entry = np.stack([pkg.scene_cast_rays(s["three"], s["rays"], k, side)[1] for k in range(3)])[idx]
        _same_bits([pkg.scene_cast_rays(many, s["rays"], 66, side)[1]], [entry[66]])
        cast = pkg.cast_scene(many, s["rays"], 0.5, side)
        tsc._check_crossing(cast, t, a, n, entry, 0.5, cap=mlr.HIT_CAP)
        _same_bits(tsc._as_probe(cast, s["dn"])[:4] + (cast[6],), probe[:4] + (probe[5],), ("the probe's bits", side))
        # the batch of four poses against four single calls
        batch = pkg.scene_pose_loss_batch(many, s["boxes"], s["poses"], s["prm"], side=side, iteration=3)
        single = np.array([pkg.scene_pose_loss(many, s["boxes"], p, s["prm"], side=side, iteration=3)[0] for p in s["poses"]], np.float32)
        assert np.isfinite(batch).all() and (batch > 0).all() and len(set(_bits(batch).tolist())) == 4
        assert np.array_equal(_bits(batch), _bits(single)), (batch, single)


def test_small_calls_keep_their_bits_after_large_ones(pkg, routes):
    """The workspaces only grow: after the calls with 70 and 130 objects, every route called with the three objects alone gives the bits it gave
    before them."""
    many = [routes["three"][k % 3] for k in range(130)]
    pkg.render_scene(many, routes["rect"], routes["pose"])                              # (the large calls of the test above, should it not have run)
    pkg.scene_pose_loss_batch(many, routes["boxes"], routes["poses"], routes["prm"], iteration=3)
    after = _small_calls(pkg, routes)
    assert len(after) == len(routes["before"])
    for k, (x, y) in enumerate(zip(routes["before"], after)):
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("case_", [("through", 17), ("through", 65), ("ties_through", 129), ("through", 256), ("full_through", 256), ("singles", 256)],
                         ids=mlr.case_id)
def test_opacity_is_the_walks_product_order_to_the_bit(pkg, case_):
    """Where no ray reaches the cut, the device's opacity is np_opacity_scan32's -- the walk's own product order emulated in float32 -- in every
    bit: rays of up to kSceneLongSeq = 1 024 merged samples by the plain tile scan (K = 17, the singles, part of K = 65: the order of every K <= 16
    render), longer ones by the two-float scan, at up to 16 384 samples.  What separates the device from fp64 is that order's rounding, not an index."""
    regime, K = case_
    t, alpha, rgb, count, dn = mlr.make_lists(regime, K, mlr.n_rays(K), mlr.seed_of(case_))
    want = mlr.np_opacity_scan32(t, alpha, count)
    for got in (pkg.scene_composite(t, alpha, rgb, count, dn)[2], pkg.scene_cast_composite(t, alpha, rgb, count, tsc._entries(t, 1), 0.5)[2]):
        assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    cstar, mstar, dstar = mlr.make_targets(t, count, np.zeros(len(dn)), 1)
    W = pkg.scene_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, *mlr.GRAD_W)["W"]
    assert np.abs(W.astype(np.float64).sum(0) - want).max() <= 64 * K * mlr.U              # (the weights sum to the opacity: a loose cross-check)
