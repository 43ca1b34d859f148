"""GPU tests (-m gpu) of the scene render (mon_scene_render, mon_online_render_scene; kernels k_fused_render<EMIT> and k_scene_composite in
kernels_render.hip).  The reference renders one object per call, so the bars are the contract itself: one object reproduces its own render, an object's
sample lists do not depend on the other objects in the call, the composite equals a numpy merge-composite of the dumped lists (also on adversarial
lists), the object order only permutes the instance map, misses give the background exactly, and a trained three-object scene resolves the occlusion
that per-object renders cannot."""
import os
import threading
import time

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import ROOT

pytestmark = pytest.mark.gpu

EPS = 1e-4                   # kTransmittanceEps
BASE = dict(sample_seed=5)                                  # base.json: 64 x 1
NARROW = dict(sample_seed=7, n_neurons=32, n_hidden_layers=2)


@pytest.fixture(scope="module")
def scene(ss):
    return ss.make_scene(n_views=24, H=240, W=320, f=260.0, n_objects=3, seed=3, elev_deg=10.0)


def _pose(ss, sc, v):
    return ss.colmajor(sc.Twc[v])


def _frame(sc, v):
    return np.array([v, 0, 0, sc.H, sc.W], np.uint32)


def _object(pkg, ss, ds, sc, k, kw, inflate=1.0, steps=300):
    ob = sc.objects[k]
    o = pkg.ObjectNeRF(ds, pkg.default_config(**kw), ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"] * inflate, ob["half"] * inflate)
    o.add_boxes(ob["boxes"]); o.set_backend(1); o.train(steps)
    return o


@pytest.fixture(scope="module")
def trained(pkg, ss, scene):
    """The three objects on their true boxes, object 0 again on a box inflated 5x (its box then reaches into both others), and object 2 as a 32 x 2
    network; 300 iterations each (published: the snapshot side renders too)."""
    sc = scene
    ds, a0 = ge.make_problem(pkg, sc, BASE, obj_index=0)
    a0.set_backend(1); a0.train(300)
    objs = dict(a0=a0, a1=_object(pkg, ss, ds, sc, 1, BASE), a2=_object(pkg, ss, ds, sc, 2, BASE), b0=_object(pkg, ss, ds, sc, 0, BASE, inflate=5.0),
                n2=_object(pkg, ss, ds, sc, 2, NARROW))
    yield ds, objs
    for o in objs.values():
        o.close()
    ds.close()


def _silhouettes(sc, v):
    """numpy ray-cast of the scene's ellipsoids (tools/synth_scene.py): per object, hit mask and z-depth of the full frame of view v."""
    ys, xs = np.mgrid[0:sc.H, 0:sc.W]
    dc = np.stack([(xs - sc.cx) / sc.fx, (ys - sc.cy) / sc.fy, np.ones_like(xs, np.float64)], -1)
    Rwc, twc = sc.Twc[v][:3, :3], sc.Twc[v][:3, 3]
    dw = dc @ Rwc.T; out = []
    for ob in sc.objects:
        Row, tow = ob["Tow"][:3, :3], ob["Tow"][:3, 3]
        on, dn = (Row @ twc + tow) / ob["radii"], (dw @ Row.T) / ob["radii"]
        a = (dn * dn).sum(-1); b = 2.0 * (dn * on).sum(-1); c = (on * on).sum() - 1.0
        disc = b * b - 4 * a * c; hit = disc > 0
        t = np.where(hit, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), np.inf); hit &= t > 0
        out.append((hit, np.where(hit, t, np.inf)))
    return out


@pytest.fixture(scope="module")
def overlap_view(scene):
    """The view with the most pixels where two objects' silhouettes overlap (one occludes the other), and that pair."""
    best = None
    for v in range(scene.n_views):
        s = _silhouettes(scene, v)
        for i in range(3):
            for j in range(i + 1, 3):
                n = int((s[i][0] & s[j][0]).sum())
                if best is None or n > best[0]:
                    best = (n, v, i, j)
    assert best[0] > 200, best
    return best[1], best[2], best[3]


def _dn(sc, rect):
    v, x0, y0, h, w = (int(q) for q in rect)
    py, px = np.mgrid[y0:y0 + h, x0:x0 + w].astype(np.float32)
    a, b = (px - np.float32(sc.cx)) / np.float32(sc.fx), (py - np.float32(sc.cy)) / np.float32(sc.fy)
    return np.sqrt(a * a + b * b + np.float32(1.0)).reshape(-1)


def np_composite(t, alpha, rgb, count, dn, amb_u=0.0):
    """numpy restatement (float64) of the merge-composite: lists [K, P, 64] (rgb [K, P, 64, 3]) with count [K, P]; merged by (t, list, slot), front to
    back, stopped at the first sample with T < EPS.  Returns rgb [P, 3], depth, opacity, instance, per-list weight sums [P, K] and a flag per ray whose
    stopping point lies within 0.1 % of EPS (float32 and float64 may stop one sample apart there).  amb_u > 0 (the unit roundoff of the arithmetic under
    test) widens that window for long sequences: max(1e-3, 4 (i + 1) amb_u) at merged sample i, the forward bound of a product of i + 1 rounded factors."""
    K, P = count.shape
    slot = np.arange(64)
    valid = slot[None, None, :] < count[..., None]
    tt = np.where(valid, t, np.inf).transpose(1, 0, 2).reshape(P, K * 64).astype(np.float64)
    aa = np.where(valid, alpha, 0.0).transpose(1, 0, 2).reshape(P, K * 64).astype(np.float64)
    cc = np.where(valid[..., None], rgb, 0.0).transpose(1, 0, 2, 3).reshape(P, K * 64, 3).astype(np.float64)
    kk = np.broadcast_to(np.arange(K)[:, None, None], (K, P, 64)).transpose(1, 0, 2).reshape(P, K * 64)
    ii = np.broadcast_to(slot, (P, K, 64)).reshape(P, K * 64)
    order = np.lexsort((ii, kk, tt), axis=-1)
    tt, aa, kk = (np.take_along_axis(q, order, 1) for q in (tt, aa, kk))
    cc = np.take_along_axis(cc, order[..., None], 1)
    N = K * 64
    incl = np.cumprod(1.0 - aa, axis=1)
    T = np.concatenate([np.ones((P, 1)), incl[:, :-1]], 1)
    active = np.logical_and.accumulate(T >= EPS, axis=1)
    nact = active.sum(1)
    w = np.where(active, aa * T, 0.0)
    Tend = np.where(nact == N, incl[:, -1], T[np.arange(P), np.minimum(nact, N - 1)])
    out_rgb = (w[..., None] * cc).sum(1) + Tend[:, None]
    dep = (w * np.where(np.isfinite(tt), tt, 0.0)).sum(1)
    op = 1.0 - Tend
    depth = np.where(op > 0.5, dep / dn, 0.0)
    wk = np.stack([(w * (kk == k)).sum(1) for k in range(K)], 1)
    inst = np.where(op > 0.5, wk.argmax(1), -1)
    win = np.maximum(1e-3, 4.0 * amb_u * (np.arange(N) + 1.0))
    ambiguous = (np.abs(T / EPS - 1.0) < win).any(1) | (np.abs(incl / EPS - 1.0) < win).any(1)
    return out_rgb, depth, op, inst, wk, ambiguous


def _near_tie(wk, rel=1e-4):
    if wk.shape[1] < 2:
        return np.zeros(wk.shape[0], bool)
    s = np.sort(wk, 1)
    return (s[:, -1] - s[:, -2]) <= rel * np.maximum(s[:, -1], 1e-30)


def _dump(pkg, objs, rect, pose, side=0):
    lists = [pkg.scene_samples(objs, rect, pose, k, side) for k in range(len(objs))]
    P = int(rect[3]) * int(rect[4])
    t = np.stack([q[0].reshape(P, 64) for q in lists]); a = np.stack([q[1].reshape(P, 64) for q in lists])
    c = np.stack([q[2].reshape(P, 64, 3) for q in lists]); n = np.stack([q[3].reshape(P) for q in lists])
    return t, a, c, n


def _check_against_numpy(pkg, sc, objs, rect, pose, side=0):
    out = pkg.render_scene(objs, rect, pose, side)
    t, a, c, n = _dump(pkg, objs, rect, pose, side)
    assert set(np.unique(n)) <= {0, 32, 64}
    ref_rgb, ref_d, ref_op, ref_inst, wk, amb = np_composite(t, a, c, n, _dn(sc, rect).astype(np.float64))
    rgb, depth, op, inst = (q.reshape(-1, 3) if q.ndim == 3 else q.reshape(-1) for q in out)
    ok = ~amb
    assert amb.mean() < 1e-3
    assert np.abs(rgb - ref_rgb)[ok].max() <= 1e-5 and np.abs(op - ref_op)[ok].max() <= 1e-5
    on = ok & (ref_op > 0.5 + 1e-4) & (op > 0.5)
    assert (np.abs(depth - ref_d)[on] <= 1e-5 * np.abs(ref_d[on]) + 1e-6).all()
    far = ok & (np.abs(ref_op - 0.5) > 1e-4) & ~_near_tie(wk)
    assert np.array_equal(inst[far], ref_inst[far])
    return t, n, out


def test_single_object_equals_its_own_render(pkg, ss, scene, trained):
    """One object, full frame, both sides, skipping off and on: on the pixels its own render covers (mask 1), rgb and depth are that render's up to
    summation order (1e-5 on >= 99.99 %, 2 x kTransmittanceEps on all) and the instance is 0; away from opacity 0.5 the instance is -1 exactly where
    the mask is 0.  The scene render leaves the object's skip statistics as they were."""
    sc = scene; _, objs = trained; o = objs["a0"]
    v = 5; rect = _frame(sc, v); pose = _pose(ss, sc, v)
    for side in (0, 1):
        for skip in (False, True):
            o.set_render_skip(skip, 1e-3)
            ref = o.render(rect, pose) if side == 0 else o.render_snapshot(rect, pose)[:3]
            st0 = o.render_skip_stats(side) if skip else None
            rgb, depth, op, inst = pkg.render_scene([o], rect, pose, side)
            if skip:
                assert o.render_skip_stats(side) == st0
            m = ref[2] > 0.5
            assert m.mean() > 0.02, (side, skip)
            drgb = np.abs(rgb - ref[0]).max(-1)[m]
            dd = (np.abs(depth - ref[1]) / np.maximum(np.abs(ref[1]), 1e-6))[m]
            for d in (drgb, dd):
                assert (d <= 1e-5).mean() >= 0.9999 and d.max() <= 2 * EPS, (side, skip, d.max())
            assert (inst[m] == 0).all()
            clear = np.abs(op - 0.5) > 1e-4
            assert np.array_equal((inst == -1)[clear], (~m)[clear]), (side, skip)
    o.set_render_skip(False)


def test_emitted_lists_do_not_depend_on_company(pkg, ss, scene, trained):
    """Object A's sample lists (mon_debug_scene_samples) are bit-identical rendered alone and with two other objects, in any list order."""
    sc = scene; _, objs = trained; A, B, C = objs["a0"], objs["a1"], objs["b0"]
    v = 9; rect = _frame(sc, v); pose = _pose(ss, sc, v)
    ref = pkg.scene_samples([A], rect, pose, 0)
    assert (ref[3] > 0).mean() > 0.02
    valid = np.arange(64)[None, None, :] < ref[3][..., None]
    for lst, k in (([B, A, C], 1), ([C, B, A], 2), ([A, C], 0)):
        got = pkg.scene_samples(lst, rect, pose, k)
        assert np.array_equal(got[3], ref[3])
        for q, r in ((got[0], ref[0]), (got[1], ref[1])):
            assert np.array_equal(q.view(np.uint32)[valid], r.view(np.uint32)[valid])
        assert np.array_equal(got[2].view(np.uint32)[valid], ref[2].view(np.uint32)[valid])


def test_composite_equals_numpy_restatement(pkg, ss, scene, trained, overlap_view):
    """Three trained objects, one on an inflated box so that their sample segments interleave along many rays: the scene outputs equal a numpy
    merge-composite of the dumped lists (rgb / opacity 1e-5, depth 1e-5 relative, instance exact away from near-ties), on both sides."""
    sc = scene; _, objs = trained; v = overlap_view[0]
    objs3 = [objs["b0"], objs["a1"], objs["a2"]]
    rect = _frame(sc, v); pose = _pose(ss, sc, v)
    for side in (0, 1):
        t, n, _ = _check_against_numpy(pkg, sc, objs3, rect, pose, side)
    # the inflated box really interleaves with the others: rays where two lists' t ranges overlap
    lo = np.where(n > 0, t[..., 0], np.inf); hi = np.where(n > 0, np.take_along_axis(t, np.maximum(n.astype(np.int64) - 1, 0)[..., None], 2)[..., 0], -np.inf)
    inter = np.zeros(n.shape[1], bool)
    for i in range(3):
        for j in range(i + 1, 3):
            inter |= (n[i] > 0) & (n[j] > 0) & (lo[i] < hi[j]) & (lo[j] < hi[i])
    assert inter.sum() > 500, inter.sum()


def _adversarial(rng, K, R, equal_t=False, alpha_hi=0.3):
    count = rng.randint(0, 65, size=(K, R)).astype(np.uint32)
    count[rng.rand(K, R) < 0.2] = 0
    if equal_t:
        t = np.sort(rng.randint(0, 40, size=(K, R, 64)) * 0.05 + 1.0, -1).astype(np.float32)
    else:
        t = np.sort(rng.uniform(0.5, 3.0, size=(K, R, 64)), -1).astype(np.float32)
    alpha = rng.uniform(0.0, alpha_hi, size=(K, R, 64)).astype(np.float32)
    alpha[rng.rand(K, R) < 0.1] = 0.0
    rgb = rng.uniform(0.0, 1.0, size=(K, R, 64, 3)).astype(np.float32)
    dn = rng.uniform(1.0, 1.3, size=R).astype(np.float32)
    return t, alpha, rgb, count, dn


def _composite_case(pkg, t, alpha, rgb, count, dn):
    got = pkg.scene_composite(t, alpha, rgb, count, dn)
    ref_rgb, ref_d, ref_op, ref_inst, wk, amb = np_composite(t, alpha, rgb, count, dn.astype(np.float64))
    ok = ~amb
    assert np.abs(got[0] - ref_rgb)[ok].max() <= 1e-5 and np.abs(got[2] - ref_op)[ok].max() <= 1e-5
    on = ok & (ref_op > 0.5 + 1e-4) & (got[2] > 0.5)
    assert (np.abs(got[1] - ref_d)[on] <= 1e-5 * np.abs(ref_d[on]) + 1e-6).all()
    far = ok & (np.abs(ref_op - 0.5) > 1e-4) & ~_near_tie(wk)
    assert np.array_equal(got[3][far], ref_inst[far])
    return got


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("equal_t", [False, True])
def test_composite_kernel_on_adversarial_lists(pkg, K, equal_t):
    """mon_debug_scene_composite on random lists: interleaved or drawn from a coarse set of t (equal t inside and across lists: ties go to the lower
    list), empty lists, lists of alpha 0, any count 0..64, K = 1, 3 and 16; against the numpy restatement."""
    rng = np.random.RandomState(100 + K + 7 * int(equal_t))
    _composite_case(pkg, *_adversarial(rng, K, 700, equal_t, alpha_hi=0.3 if K > 1 else 0.6))
    _composite_case(pkg, *_adversarial(rng, K, 300, equal_t, alpha_hi=0.02))          # (rarely terminates: every block and list reached)


def test_composite_kernel_edge_cases(pkg):
    """An opaque first sample ends the ray (rgb = its colour, opacity 1, depth its t / dn); all-zero alpha and empty lists give the background exactly."""
    rng = np.random.RandomState(4)
    t, alpha, rgb, count, dn = _adversarial(rng, 3, 64)
    count[:] = 64; alpha[:] = 0.2
    first = np.argmin(t[:, :, 0], axis=0)                           # the list holding each ray's nearest sample (ties: the lower list)
    for r in range(64):
        alpha[first[r], r, 0] = 1.0
    got = pkg.scene_composite(t, alpha, rgb, count, dn)
    front = rgb[first, np.arange(64), 0]
    assert np.array_equal(got[0], front) and (got[2] == 1.0).all() and np.array_equal(got[3], first.astype(np.int32))
    assert np.allclose(got[1], t[first, np.arange(64), 0] / dn, rtol=1e-6)
    _composite_case(pkg, t, alpha, rgb, count, dn)
    alpha[:] = 0.0
    got = pkg.scene_composite(t, alpha, rgb, count, dn)
    assert (got[0] == 1.0).all() and (got[1] == 0.0).all() and (got[2] == 0.0).all() and (got[3] == -1).all()
    count[:] = 0
    got = pkg.scene_composite(t, alpha, rgb, count, dn)
    assert (got[0] == 1.0).all() and (got[1] == 0.0).all() and (got[2] == 0.0).all() and (got[3] == -1).all()


def test_object_order_only_permutes_the_instance(pkg, ss, scene, trained, overlap_view):
    """Permuting the object list leaves rgb / depth / opacity within 1e-6 and permutes the instance map accordingly."""
    sc = scene; _, objs = trained; v = overlap_view[0]
    base = [objs["b0"], objs["a1"], objs["a2"]]; perm = [2, 0, 1]
    rect = _frame(sc, v); pose = _pose(ss, sc, v)
    r1 = pkg.render_scene(base, rect, pose)
    r2 = pkg.render_scene([base[p] for p in perm], rect, pose)
    for a, b in zip(r1[:3], r2[:3]):
        assert np.abs(a - b).max() <= 1e-6
    mapped = np.where(r2[3] >= 0, np.asarray(perm)[np.maximum(r2[3], 0)], -1)
    assert np.array_equal(mapped, r1[3])


def test_misses_give_background_and_min_alpha_zero_is_identical(pkg, ss, scene, trained):
    """A pose whose rays pass every box, and a rect of pixels whose rays miss every box, give rgb 1, depth 0, opacity 0, instance -1 exactly.  Render skipping at
    min_alpha = 0 is bit-identical to skipping off, on both sides."""
    sc = scene; _, objs = trained; lst = [objs["a0"], objs["a1"], objs["a2"]]
    # (a box behind the camera is hit as in the object render, which clamps t0 at 0: this camera's rays pass 2.7 above every box both ways)
    away = ss.colmajor(ss._look_at(np.array([0.0, 0.0, 3.0]), np.array([10.0, 0.0, 3.0])))
    rgb, depth, op, inst = pkg.render_scene(lst, _frame(sc, 0), away)
    assert (rgb == 1.0).all() and (depth == 0.0).all() and (op == 0.0).all() and (inst == -1).all()
    v = 3; pose = _pose(ss, sc, v)
    corners = [np.array([v, x, y, 6, 8], np.uint32) for x in (0, sc.W - 8) for y in (0, sc.H - 6)]
    empty = [c for c in corners if all((pkg.scene_samples(lst, c, pose, k)[3] == 0).all() for k in range(3))]
    assert empty                                                   # some image corner of the view sees none of the boxes
    rgb, depth, op, inst = pkg.render_scene(lst, empty[0], pose)
    assert (rgb == 1.0).all() and (depth == 0.0).all() and (op == 0.0).all() and (inst == -1).all()
    rect = _frame(sc, v)
    for side in (0, 1):
        for o in lst:
            o.set_render_skip(False)
        plain = pkg.render_scene(lst, rect, pose, side)
        for o in lst:
            o.set_render_skip(True, 0.0)
        skip = pkg.render_scene(lst, rect, pose, side)
        for a, b in zip(plain, skip):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), side
    for o in lst:
        o.set_render_skip(False)


def test_ground_truth_instance_and_depth_with_occlusion(pkg, ss, scene, trained, overlap_view):
    """The three trained objects on their true boxes, the view where two of them overlap most in 2-D: per-object IoU of the instance map against the
    scene's ground truth, the front object winning on the overlap pixels, and the median relative depth error against the ground-truth z-depth where
    both agree.  Per-object renders alone cannot tell which object is in front.  Measured on the first MI355X run (view 23, objects 0 in front of 1,
    1432 overlap pixels): IoU 0.997 / 0.999, front object wins 100 % of the overlap, median relative depth error 0.0057.  Bars with a margin: IoU >= 0.95,
    >= 98 % won, median <= 0.015."""
    sc = scene; _, objs = trained; v, i, j = overlap_view
    lst = [objs["a0"], objs["a1"], objs["a2"]]
    rect = _frame(sc, v); pose = _pose(ss, sc, v)
    rgb, depth, op, inst = pkg.render_scene(lst, rect, pose)
    gt = sc.instance[v]; cls = [ob["cls"] for ob in sc.objects]
    gt_idx = np.full(gt.shape, -1)
    for k, c in enumerate(cls):
        gt_idx[gt == c] = k
    ious = []
    for k in range(3):
        a, b = inst == k, gt_idx == k
        if b.sum() > 50:
            ious.append(float((a & b).sum()) / float((a | b).sum()))
    sil = _silhouettes(sc, v)
    both = sil[i][0] & sil[j][0]
    front = np.where(sil[i][1] < sil[j][1], i, j)
    core = both & (gt_idx == front)
    won = float((inst[core] == front[core]).mean())
    agree = (inst == gt_idx) & (gt_idx >= 0) & (sc.depth[v] > 0)
    rel = np.abs(depth[agree] - sc.depth[v][agree]) / sc.depth[v][agree]
    med = float(np.median(rel))
    print("scene GT view %d pair (%d, %d): IoU %s, front wins %.4f on %d px, median rel depth %.4f" % (v, i, j, ["%.3f" % q for q in ious], won,
          int(core.sum()), med))
    assert len(ious) >= 2 and min(ious) >= 0.95 and won >= 0.98 and med <= 0.015


def _online_feed(pkg, ss, sc, m, n_obj, train_calls):
    ids = []
    for v in range(sc.n_views):
        m.new_frame(v, "%.6f" % (v * 0.1), sc.rgb[v][..., ::-1], sc.instance[v], ss.colmajor(sc.Twc[v]))
    for k in range(n_obj):
        ob = sc.objects[k]
        ids.append(m.create_nerf(ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"] / 1.1, ob["half"] / 1.1))
    for k in range(n_obj):
        m.update_nerf_bbox(ids[k], sc.objects[k]["boxes"], train_calls)
    return ids


def _wait_trained(m, ids, calls, limit_s=90.0):
    t0 = time.time()
    while time.time() - t0 < limit_s:
        if all(m.object_info(i)["train_calls"] >= calls for i in ids):
            return True
        time.sleep(0.05)
    return False


def test_online_viewer_path_and_errors(pkg, ss, scene, trained):
    """mon_online_render_scene from a viewer thread while the manager's three objects train (a time-limited run), then the same snapshots through
    mon_scene_render(side 1): identical.  Errors: objects on two logical devices (MON_ERR_ARG; the online wrapper MON_ERR_STATE), a layer-kernel shape,
    an XORWOW object and an unpublished object on side 1 (MON_ERR_STATE)."""
    sc = scene; ds, objs = trained
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    v = 7; rect = _frame(sc, v); pose = _pose(ss, sc, v)
    seen = dict(n=0, covered=0, err=None); stop = threading.Event()

    def viewer():
        try:
            while not stop.is_set():
                rgb, depth, op, inst = m.render_scene(rect, pose)
                assert set(np.unique(inst)) <= {-1, 0, 1, 2} and np.isfinite(rgb).all()
                seen["n"] += 1; seen["covered"] += int((op > 0.5).sum() > 0)
                time.sleep(0.01)
        except Exception as e:        # noqa: BLE001 -- reported by the main thread
            seen["err"] = e

    th = threading.Thread(target=viewer); th.start()
    try:
        ids = _online_feed(pkg, ss, sc, m, 3, 4)
        ok = _wait_trained(m, ids, 2)
    finally:
        stop.set(); th.join(timeout=60)
    m.wait_threads_end()
    assert ok and seen["err"] is None and seen["n"] > 5 and seen["covered"] > 0, seen
    a = m.render_scene(rect, pose)
    b = pkg.render_scene([m.object(i) for i in ids], rect, pose, side=1)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (a[2] > 0.5).mean() > 0.02
    m.close()
    # shapes and modes the scene render refuses
    _, c = ge.make_problem(pkg, sc, dict(n_neurons=16), dataset=ds)
    _, x = ge.make_problem(pkg, sc, dict(BASE, rng_flags=1), dataset=ds)
    _, fresh = ge.make_problem(pkg, sc, BASE, obj_index=1, dataset=ds)
    for lst, side in (([c], 0), ([objs["a0"], c], 0), ([x], 0), ([fresh], 1), ([objs["a0"], fresh], 1)):
        with pytest.raises(pkg.MonError) as e:
            pkg.render_scene(lst, rect, pose, side)
        assert e.value.code == 5, (len(lst), side)
    for o in (c, x, fresh):
        o.close()
    # two logical devices
    pkg.set_logical_devices(2)
    try:
        ds0, o0 = ge.make_problem(pkg, sc, BASE, device=0, obj_index=0)
        ds1, o1 = ge.make_problem(pkg, sc, BASE, device=1, obj_index=1)
        with pytest.raises(pkg.MonError) as e:
            pkg.render_scene([o0, o1], rect, pose)
        assert e.value.code == 1
        for o in (o0, o1, ds0, ds1):
            o.close()
        m2 = pkg.OnlineManager(cfg, False, 20)
        m2.init(); m2.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
        ids2 = _online_feed(pkg, ss, sc, m2, 2, 1)
        assert _wait_trained(m2, ids2, 1)
        assert sorted(m2.object_info(i)["device"] for i in ids2) == [0, 1]
        with pytest.raises(pkg.MonError) as e:
            m2.render_scene(rect, pose)
        assert e.value.code == 5
        m2.wait_threads_end(); m2.close()
    finally:
        pkg.set_logical_devices(0)


def test_mixed_network_shapes(pkg, ss, scene, trained, overlap_view):
    """A 32 x 2 object and a 64 x 1 object (and the inflated 64 x 1 box) in one scene: each emits through its own k_fused_render<EMIT> instantiation and
    the composite equals the numpy restatement."""
    sc = scene; _, objs = trained; v = overlap_view[0]
    rect = _frame(sc, v); pose = _pose(ss, sc, v)
    _check_against_numpy(pkg, sc, [objs["n2"], objs["a1"]], rect, pose)
    _check_against_numpy(pkg, sc, [objs["a1"], objs["b0"], objs["n2"]], rect, pose)
