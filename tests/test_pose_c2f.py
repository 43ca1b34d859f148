"""GPU tests (-m gpu) of coarse-to-fine pose refinement (mon_object_pose_loss_levels, mon_object_refine_pose_c2f, mon_online_refine_pose_c2f; the
k_pose_grad<.., LW = true> instantiations in kernels_pose.hip).  The bars are the contract of include/mon_core.h: weights of 1 give the plain gradient bit
for bit, weights of 0 give none, the gradient is linear in the weights and equals an fp64 torch autograd graph in which each level's position dependence is
scaled by its weight, step i of a refinement uses the weights of step i, and the schedule brings a perturbed base.json object back."""
import os
import threading
import time

import numpy as np
import pytest

from conftest import ROOT                                    # (first: it puts the repository root on the path of the torch child process)
import __graft_entry__ as ge                                # noqa: E402
import pose_reference as pref                               # noqa: E402
from test_pose_refine import _crops, _perturb, _pose_errors, _mat, _six_boxes, _snapshot_state      # noqa: E402

pytestmark = pytest.mark.gpu

BASE = dict(sample_seed=5, use_depth=1)                     # base.json: 16 levels, 64 x 1
NARROW = dict(sample_seed=7, n_neurons=32, n_hidden_layers=2, use_depth=1)
WIDE = dict(sample_seed=8, n_neurons=128, n_hidden_layers=1, use_depth=1)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(ss):
    return ss.make_scene(n_views=24, H=240, W=320, f=260.0, seed=3)


@pytest.fixture(scope="module")
def trained(pkg, ss, scene):
    """base.json, 32 x 2 and 128 x 1 objects on the scene's one object, 500 iterations each on the true pose (published: side 1 holds the same EMA)."""
    sc = scene
    ds, a = ge.make_problem(pkg, sc, BASE, use_depth=True)
    objs = dict(base=a)
    for name, kw in (("narrow", NARROW), ("wide", WIDE)):
        objs[name] = ge.make_problem(pkg, sc, kw, use_depth=True, dataset=ds)[1]
    for o in objs.values():
        o.set_backend(1); o.train(500)
    yield ds, objs
    for o in objs.values():
        o.close()
    ds.close()


def _window(L, alpha):
    """the BARF window of include/mon_core.h in float64"""
    a = alpha - np.arange(L, dtype=np.float64)
    return np.where(a <= 0, 0.0, np.where(a >= 1, 1.0, (1 - np.cos(np.pi * np.clip(a, 0, 1))) / 2))


# ------------------------------------------------------------------ 1. weights of 1 are the plain gradient, bit for bit
@pytest.mark.parametrize("rays", [0, 4096])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", ["base", "narrow", "wide"])
def test_ones_equal_plain_bit_for_bit(pkg, ss, scene, trained, name, side, rays):
    sc = scene; _, objs = trained; o = objs[name]; ob = sc.objects[0]
    boxes = _crops(sc) if rays == 0 else _six_boxes(sc)
    prm = pkg.pose_refine_default(rays_per_iter=rays); ones = np.ones(o.cfg.n_levels, np.float32)
    diag = float(np.linalg.norm(2 * ob["half"]))
    for T in (ob["Tow"], _perturb(ob["Tow"], 5.0, 0.05 * diag, 2)):
        T16 = ss.colmajor(T)
        l0, g0 = o.pose_loss(boxes, T16, prm, side=side, iteration=3)
        l1, g1 = o.pose_loss_levels(boxes, T16, ones, prm, side=side, iteration=3)
        assert np.array_equal(_bits(l0), _bits(l1)) and np.array_equal(_bits(g0), _bits(g1)), (l0, l1, g0, g1)
        assert np.linalg.norm(g0) > 0


def test_full_window_refinement_equals_plain_bit_for_bit(pkg, ss, scene, trained):
    sc = scene; _, objs = trained; o = objs["base"]; ob = sc.objects[0]; L = o.cfg.n_levels
    diag = float(np.linalg.norm(2 * ob["half"])); boxes = _six_boxes(sc); prm = pkg.pose_refine_default(iters=20)
    T0 = ss.colmajor(_perturb(ob["Tow"], 5.0, 0.05 * diag, 1))
    for side in (0, 1):
        p0, t0 = o.refine_pose(boxes, T0, prm, side=side)
        p1, t1 = o.refine_pose_c2f(boxes, T0, prm, pkg.pose_c2f_default(level_start=L, level_end=L), side=side)
        assert np.array_equal(_bits(p0), _bits(p1)) and np.array_equal(_bits(t0), _bits(t1))
    # the end of the ramp on: every level at 1 as well (level_end past L)
    p2, t2 = o.refine_pose_c2f(boxes, T0, prm, pkg.pose_c2f_default(level_start=L + 0.5, level_end=L + 7.0, ramp=0.3))
    assert np.array_equal(_bits(p0), _bits(p2)) and np.array_equal(_bits(t0), _bits(t2))


# ------------------------------------------------------------------ 2. zeros, and linearity in the weights
@pytest.mark.parametrize("name", ["base", "narrow"])
def test_zero_weights_and_linearity(pkg, ss, scene, trained, name):
    sc = scene; _, objs = trained; o = objs[name]; ob = sc.objects[0]; L = o.cfg.n_levels
    diag = float(np.linalg.norm(2 * ob["half"])); boxes = _six_boxes(sc); prm = pkg.pose_refine_default()
    T16 = ss.colmajor(_perturb(ob["Tow"], 3.0, 0.03 * diag, 7))
    l_plain, g_plain = o.pose_loss(boxes, T16, prm)
    l0, g0 = o.pose_loss_levels(boxes, T16, np.zeros(L, np.float32), prm)
    assert np.array_equal(g0, np.zeros(6, np.float32)) and np.array_equal(_bits(l0), _bits(l_plain))
    E = np.stack([o.pose_loss_levels(boxes, T16, np.eye(L, dtype=np.float32)[l], prm)[1] for l in range(L)]).astype(np.float64)   # [L][6]
    bar = 1e-5 * np.abs(E).sum(0)
    print("%s: |grad6(e_l)| by level %s" % (name, np.array2string(np.linalg.norm(E, axis=1), precision=4)))
    assert np.all(np.abs(E.sum(0) - g_plain) <= bar), (E.sum(0), g_plain, bar)
    rs = np.random.RandomState(5)
    for _ in range(3):
        w = rs.uniform(0, 1, L).astype(np.float32)
        g = o.pose_loss_levels(boxes, T16, w, prm)[1]
        want = (w.astype(np.float64)[:, None] * E).sum(0)
        assert np.all(np.abs(g - want) <= bar), (g, want, bar)


# ------------------------------------------------------------------ 3. the weighted gradient is fp64 autograd of the scaled graph
def test_weighted_gradient_matches_fp64_autograd(pkg, orc, ss, scene, trained, tmp_path):
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch not installed")
    sc = scene; _, objs = trained; o = objs["base"]; ob = sc.objects[0]; cfg = o.cfg; L = cfg.n_levels
    boxes = _crops(sc); prm = pkg.pose_refine_default(rays_per_iter=0)
    diag = float(np.linalg.norm(2 * ob["half"]))
    poses = [ob["Tow"], _perturb(ob["Tow"], 3.0, 0.03 * diag, seed=11)]
    w = _window(L, 6.4).astype(np.float32)                             # levels 0-5 whole, level 6 in the ramp, the rest off
    aabb = np.stack([-ob["half"], ob["half"]]).astype(np.float32)
    results, cases = [], []
    for Tow in poses:
        T16 = ss.colmajor(Tow)
        loss, g6 = o.pose_loss_levels(boxes, T16, w, prm)
        x, _, _ = o.pose_samples(boxes, T16, prm)
        results.append(dict(loss=loss, g6=g6, x=x))
        rr = pref.pose_rays(sc, boxes, Tow, aabb, ob["cls"], sample_seed=cfg.sample_seed)
        cases.append(dict(x=x, t=rr["t"], hit=rr["hit"], dn=rr["dn"], tgt=rr["tgt"], lw=w, pos=rr["pos"]))
    refs = pref.reference(tmp_path, pref.net_inputs(o, orc, prm), aabb, cases)
    for i, got in enumerate(results):
        want6 = refs[i]["g6"]; ev = refs[i]["ev"]
        assert np.abs(got["x"][ev] - cases[i]["pos"][ev]).max() < 1e-5, "sample positions"
        assert abs(got["loss"] - refs[i]["loss"]) <= 1e-4 * abs(refs[i]["loss"])
        rel = np.linalg.norm(got["g6"] - want6) / np.linalg.norm(want6)
        print("pose %d: grad6(w) %s ref %s rel %.2e" % (i, np.array2string(got["g6"], precision=5), np.array2string(want6, precision=5), rel))
        assert rel <= 1e-2, rel


# ------------------------------------------------------------------ 4. step i of a refinement uses the weights of step i
def _se3_exp32(xi):
    """k_pose_update's se3_exp in float32 (column-major R[9])"""
    f = np.float32
    w0, w1, w2 = (f(v) for v in xi[3:])
    th2 = f(w0 * w0 + w1 * w1 + w2 * w2); th = f(np.sqrt(th2))
    if th < f(1e-3):
        A = f(1) - th2 / f(6); B = f(0.5) - th2 / f(24); C = f(1.0 / 6.0) - th2 / f(120)
    else:
        s, c = f(np.sin(th)), f(np.cos(th)); A = s / th; B = (f(1) - c) / th2; C = (th - s) / (th2 * th)
    K = np.array([0, w2, -w1, -w2, 0, w0, w1, -w0, 0], np.float32)
    K2 = np.zeros(9, np.float32)
    for cc in range(3):
        for r in range(3):
            v = f(0)
            for k in range(3):
                v = f(v + K[k * 3 + r] * K[cc * 3 + k])
            K2[cc * 3 + r] = v
    I = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    R = (I + A * K + B * K2).astype(np.float32); V = (I + B * K + C * K2).astype(np.float32)
    t = np.array([V[r] * f(xi[0]) + V[3 + r] * f(xi[1]) + V[6 + r] * f(xi[2]) for r in range(3)], np.float32)
    return R, t


def _adam_step32(pose16, mom, g, it, lr_t, lr_r):
    """k_pose_update's step `it` (0-based) in float32: Adam on the twist, pose <- exp(delta^) pose, Gram-Schmidt"""
    f = np.float32; b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    tt = f(it + 1); c1 = f(1) - f(np.power(b1, tt)); c2 = f(1) - f(np.power(b2, tt))
    delta = np.zeros(6, np.float32)
    for j in range(6):
        gj = f(g[j]); m = b1 * mom[j] + (f(1) - b1) * gj; v = b2 * mom[6 + j] + (f(1) - b2) * gj * gj
        mom[j] = m; mom[6 + j] = v
        lr = f(lr_t) if j < 3 else f(lr_r)
        delta[j] = -lr * (m / c1) / (f(np.sqrt(v / c2)) + eps)
    Rd, td = _se3_exp32(delta)
    P = np.asarray(pose16, np.float32)
    Rn = np.zeros(9, np.float32)
    for cc in range(3):
        for r in range(3):
            Rn[cc * 3 + r] = sum(f(Rd[k * 3 + r] * P[cc * 4 + k]) for k in range(3))
    tn = np.array([Rd[r] * P[12] + Rd[3 + r] * P[13] + Rd[6 + r] * P[14] + td[r] for r in range(3)], np.float32)
    a0, a1 = Rn[0:3].copy(), Rn[3:6].copy()
    a0 = a0 / f(np.sqrt((a0 * a0).sum())); a1 = a1 - f((a0 * a1).sum()) * a0; a1 = a1 / f(np.sqrt((a1 * a1).sum()))
    a2 = np.cross(a0, a1).astype(np.float32)
    out = np.zeros(16, np.float32)
    for cc, col in enumerate((a0, a1, a2)):
        out[cc * 4:cc * 4 + 3] = col
    out[12:15] = tn; out[15] = 1
    return out


def test_schedule_step_uses_its_own_row(pkg, ss, scene, trained):
    """Step 0 of a 2-step schedule (alpha 2) and step 1 (alpha 6) against a float32 restatement of k_pose_update fed with pose_loss_levels at the weights
    of that step: the 1-step refinement is step 0 (alpha(0) = level_start either way), and from its pose step 1 with the other row."""
    sc = scene; _, objs = trained; o = objs["base"]; ob = sc.objects[0]; L = o.cfg.n_levels
    diag = float(np.linalg.norm(2 * ob["half"])); boxes = _six_boxes(sc)
    c = pkg.pose_c2f_default(level_start=2.0, level_end=10.0, ramp=1.0)
    T0 = ss.colmajor(_perturb(ob["Tow"], 5.0, 0.05 * diag, 3))
    w0, w1 = pkg.pose_c2f_weights(L, 2, 0, c), pkg.pose_c2f_weights(L, 2, 1, c)
    assert not np.array_equal(w0, w1)                                   # alpha 2, then 6
    prm1, prm2 = pkg.pose_refine_default(iters=1), pkg.pose_refine_default(iters=2)
    pose1, trace1 = o.refine_pose_c2f(boxes, T0, prm1, c)
    pose2, trace2 = o.refine_pose_c2f(boxes, T0, prm2, c)
    mom = np.zeros(12, np.float32)
    l0, g0 = o.pose_loss_levels(boxes, T0, w0, prm2, iteration=0)
    p1 = _adam_step32(T0, mom, g0, 0, prm2.lr_trans, prm2.lr_rot)
    print("step 0: device %s\n        numpy  %s" % (np.array2string(pose1, precision=6), np.array2string(p1, precision=6)))
    assert np.array_equal(_bits(trace1[0]), _bits(l0)) and np.array_equal(_bits(trace2[0]), _bits(l0))
    assert np.abs(pose1 - p1).max() <= 1e-5, np.abs(pose1 - p1).max()
    l1, g1 = o.pose_loss_levels(boxes, pose1, w1, prm2, iteration=1)
    p2 = _adam_step32(pose1, mom.copy(), g1, 1, prm2.lr_trans, prm2.lr_rot)
    print("step 1: device %s\n        numpy  %s" % (np.array2string(pose2, precision=6), np.array2string(p2, precision=6)))
    assert np.array_equal(_bits(trace2[1]), _bits(l1))
    assert np.abs(pose2 - p2).max() <= 1e-5, np.abs(pose2 - p2).max()
    # step 1 with step 0's row lands elsewhere: the row of each step is what it used
    g1x = o.pose_loss_levels(boxes, pose1, w0, prm2, iteration=1)[1]
    assert np.abs(_adam_step32(pose1, mom.copy(), g1x, 1, prm2.lr_trans, prm2.lr_rot) - p2).max() > 1e-5


# ------------------------------------------------------------------ 5. base.json converges under the default schedule
CONV_ROT_DEG, CONV_TRANS_FRAC = 0.6, 0.005          # bars: see the docstring
DRIFT_ROT_DEG, DRIFT_TRANS_FRAC = 0.6, 0.0025


def test_base_json_converges_with_the_default_schedule(pkg, ss, scene, trained):
    """24 views of 240 x 320, 500 training iterations on the true pose of base.json (16 levels, finest resolution 2^19); the pose perturbed by 5 degrees and
    5 % of the box diagonal (three seeds), the defaults of both parameter structs (100 steps of 4096 rays; level_start 4, level_end 5, ramp 0.7) on 6 boxes.
    Measured on an MI355X: rotation 0.132 / 0.156 / 0.276 degrees, centre 0.134 / 0.109 / 0.046 % of the diagonal, loss 0.062-0.072 -> 0.0006-0.0007; from
    the true pose 0.273 degrees and 0.112 %.  Plain refine_pose from the same starts ends 4.9-6.1 degrees and 2.4-7.4 % off.
    Bars: rotation <= 0.6 degrees and centre <= 0.5 % of the diagonal, the loss trace ending below half its start; the drift from the true pose <= 0.6
    degrees and 0.25 % (>= 2x margin each).  The rotation bars sit above the 0.5 degrees of the 8-level test because the floor is Adam's step at the
    default lr_rot (4e-3 rad = 0.23 degrees): 0.2-0.35 degrees over every schedule of the sweep (profiles/r09_pose_c2f.md)."""
    sc = scene; _, objs = trained; o = objs["base"]; ob = sc.objects[0]
    diag = float(np.linalg.norm(2 * ob["half"])); boxes = _six_boxes(sc); prm = pkg.pose_refine_default(); c = pkg.pose_c2f_default()
    for seed in (1, 2, 3):
        T0 = _perturb(ob["Tow"], 5.0, 0.05 * diag, seed)
        pose, trace = o.refine_pose_c2f(boxes, ss.colmajor(T0), prm, c)
        pp, pt = o.refine_pose(boxes, ss.colmajor(T0), prm)
        e0 = _pose_errors(T0, ob["Tow"]); e1 = _pose_errors(_mat(pose), ob["Tow"]); ep = _pose_errors(_mat(pp), ob["Tow"])
        print("seed %d: rotation %.3f -> %.4f deg, centre %.5f (%.3f%% of the diagonal), loss %.5f -> %.5f | plain: %.4f deg, %.3f%%, loss -> %.5f" % (
              seed, e0[0], e1[0], e1[1], 100 * e1[1] / diag, trace[0], trace[-1], ep[0], 100 * ep[1] / diag, pt[-1]))
        assert np.isfinite(trace).all() and trace[-1] < 0.5 * trace[0], trace[[0, -1]]
        assert e1[0] <= CONV_ROT_DEG and e1[1] <= CONV_TRANS_FRAC * diag, (e1, diag)
    pose, trace = o.refine_pose_c2f(boxes, ss.colmajor(ob["Tow"]), prm, c)
    e = _pose_errors(_mat(pose), ob["Tow"])
    print("from the true pose: drift %.4f deg, %.5f (%.3f%%)" % (e[0], e[1], 100 * e[1] / diag))
    assert e[0] <= DRIFT_ROT_DEG and e[1] <= DRIFT_TRANS_FRAC * diag, e


# ------------------------------------------------------------------ 6. read-only, deterministic, both sides, online
def test_c2f_is_read_only_and_deterministic(pkg, ss, scene):
    sc = scene; ob = sc.objects[0]
    ds, a = ge.make_problem(pkg, sc, dict(sample_seed=13), use_depth=True)
    _, b = ge.make_problem(pkg, sc, dict(sample_seed=13), use_depth=True, dataset=ds)
    try:
        a.set_backend(1); b.set_backend(1); a.train(200); b.train(200)
        L = a.cfg.n_levels
        box = sc.objects[0]["boxes"][3]; Twc = ss.colmajor(sc.Twc[int(box[0])])
        before = _snapshot_state(a, box, Twc)
        T0 = ss.colmajor(_perturb(ob["Tow"], 3.0, 0.02, 4)); boxes = _six_boxes(sc); prm = pkg.pose_refine_default(iters=20); c = pkg.pose_c2f_default()
        p1, t1 = a.refine_pose_c2f(boxes, T0, prm, c, side=0)
        p2, t2 = a.refine_pose_c2f(boxes, T0, prm, c, side=0)
        p3, t3 = a.refine_pose_c2f(boxes, T0, prm, c, side=1)
        assert np.array_equal(_bits(p1), _bits(p2)) and np.array_equal(_bits(t1), _bits(t2))
        assert np.array_equal(_bits(p1), _bits(p3)) and np.array_equal(_bits(t1), _bits(t3))      # same weights
        w = pkg.pose_c2f_weights(L, 20, 5, c)
        l1, g1 = a.pose_loss_levels(boxes, T0, w, prm, iteration=7); l2, g2 = a.pose_loss_levels(boxes, T0, w, prm, iteration=7)
        l3, g3 = a.pose_loss_levels(boxes, T0, w, prm, side=1, iteration=7)
        assert l1 == l2 == l3 and np.array_equal(g1, g2) and np.array_equal(g1, g3)
        after = _snapshot_state(a, box, Twc)
        for x, y in zip(before[0], after[0]):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        assert before[1] == after[1] and before[2] == after[2]
        for x, y in zip(before[3], after[3]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        a.train(50); b.train(50)
        for k in range(3):
            assert np.array_equal(a.get_params(k).view(np.uint8), b.get_params(k).view(np.uint8)), k
    finally:
        a.close(); b.close(); ds.close()


def test_online_refine_c2f_while_training(pkg, ss, scene):
    sc = scene; ob = sc.objects[0]
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    for v in range(sc.n_views):
        m.new_frame(v, "%.6f" % (v * 0.1), sc.rgb[v][..., ::-1], sc.instance[v], ss.colmajor(sc.Twc[v]))
    idx = m.create_nerf(ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    boxes = _six_boxes(sc); prm = pkg.pose_refine_default(iters=20); c = pkg.pose_c2f_default()
    T0 = ss.colmajor(_perturb(ob["Tow"], 3.0, 0.02, 5))
    with pytest.raises(pkg.MonError) as e:
        m.refine_pose_c2f(idx, boxes, T0, prm, c)            # nothing published yet
    assert e.value.code == 5
    seen = dict(n=0, err=None); stop = threading.Event()

    def frontend():
        try:
            while not stop.is_set():
                try:
                    p, tr = m.refine_pose_c2f(idx, boxes, T0, prm, c)
                except pkg.MonError as ex:
                    if ex.code != 5:
                        raise
                    time.sleep(0.01); continue
                assert np.isfinite(p).all() and np.isfinite(tr).all()
                seen["n"] += 1
        except Exception as ex:        # noqa: BLE001 -- reported by the main thread
            seen["err"] = ex

    th = threading.Thread(target=frontend); th.start()
    try:
        m.update_nerf_bbox(idx, ob["boxes"], 4)
        t0 = time.time()
        while m.object_info(idx)["train_calls"] < 3 and time.time() - t0 < 90:
            time.sleep(0.05)
    finally:
        stop.set(); th.join(timeout=60)
    m.wait_threads_end()
    assert seen["err"] is None and seen["n"] > 0, seen
    a = m.refine_pose_c2f(idx, boxes, T0, prm, c)
    b = m.object(idx).refine_pose_c2f(boxes, T0, prm, c, side=1)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    m.close()


# ------------------------------------------------------------------ 7. errors
def test_c2f_errors(pkg, ss, scene, trained):
    sc = scene; ds, objs = trained; ob = sc.objects[0]
    T = ss.colmajor(ob["Tow"]); boxes = _crops(sc); prm = pkg.pose_refine_default(iters=2); c = pkg.pose_c2f_default()
    _, lk = ge.make_problem(pkg, sc, dict(n_neurons=16), dataset=ds)
    _, x = ge.make_problem(pkg, sc, dict(rng_flags=1), dataset=ds)
    _, fresh = ge.make_problem(pkg, sc, dict(), dataset=ds)
    try:
        for o, side in ((lk, 0), (x, 0), (fresh, 1)):
            ones = np.ones(o.cfg.n_levels, np.float32)
            for call in (lambda: o.refine_pose_c2f(boxes, T, prm, c, side=side), lambda: o.pose_loss_levels(boxes, T, ones, prm, side=side)):
                with pytest.raises(pkg.MonError) as e:
                    call()
                assert e.value.code == 5, side
        o = objs["base"]; L = o.cfg.n_levels
        for bad in (-1e-3, float("nan"), float("inf")):
            w = np.ones(L, np.float32); w[L - 1] = bad
            with pytest.raises(pkg.MonError) as e:
                o.pose_loss_levels(boxes, T, w, prm)
            assert e.value.code == 1, bad
        for kw in (dict(level_start=-1.0), dict(level_start=5.0, level_end=4.0), dict(ramp=0.0), dict(ramp=1.5), dict(level_end=float("nan"))):
            with pytest.raises(pkg.MonError) as e:
                o.refine_pose_c2f(boxes, T, prm, pkg.pose_c2f_default(**kw))
            assert e.value.code == 1, kw
        with pytest.raises(ValueError):
            o.pose_loss_levels(boxes, T, np.ones(L - 1, np.float32), prm)
        # iters 0: no step, the trace holds the loss of the start
        p, tr = o.refine_pose_c2f(boxes, T, pkg.pose_refine_default(iters=0), c)
        assert np.array_equal(_bits(p), _bits(np.asarray(T, np.float32))) and tr.shape == (1,)
        assert np.array_equal(_bits(tr[0]), _bits(o.pose_loss(boxes, T, pkg.pose_refine_default(iters=0))[0]))
    finally:
        for q in (lk, x, fresh):
            q.close()
