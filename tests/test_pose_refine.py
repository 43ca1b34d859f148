"""GPU tests (-m gpu) of object pose refinement (mon_object_pose_loss, mon_object_refine_pose, mon_online_refine_pose; kernels k_pose_rays,
k_pose_grad, k_pose_update in kernels_pose.hip).  The bars are the contract of include/mon_core.h: the loss equals a numpy restatement from the render's own
samples, the gradient equals an fp64 torch autograd graph of the same objective (and per sample through mon_debug_pose_samples), refinement pulls a
perturbed pose back, and nothing about the object changes."""
import math
import os
import threading
import time

import numpy as np
import pytest

from conftest import ROOT                                    # (first: it puts the repository root on the path)
import __graft_entry__ as ge                                # noqa: E402
import pose_reference as pref                               # noqa: E402
from pose_reference import targets as _targets, EPS         # noqa: E402

pytestmark = pytest.mark.gpu

BASE = dict(sample_seed=5, use_depth=1)                     # base.json: 16 levels, 64 x 1
NARROW = dict(sample_seed=7, n_neurons=32, n_hidden_layers=2, use_depth=1)


@pytest.fixture(scope="module")
def scene(ss):
    return ss.make_scene(n_views=24, H=240, W=320, f=260.0, seed=3)


def _object(pkg, ss, ds, sc, kw, steps=500):
    ob = sc.objects[0]
    o = pkg.ObjectNeRF(ds, pkg.default_config(**kw), ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    o.add_boxes(ob["boxes"]); o.set_backend(1)
    if steps:
        o.train(steps)
    return o


@pytest.fixture(scope="module")
def trained(pkg, ss, scene):
    """A base.json object and a 32 x 2 object on the scene's one object, 500 iterations each on the true pose (published: side 1 holds the same EMA)."""
    sc = scene
    ds, a = ge.make_problem(pkg, sc, BASE, use_depth=True)
    a.set_backend(1); a.train(500)
    objs = dict(base=a, narrow=_object(pkg, ss, ds, sc, NARROW))
    yield ds, objs
    for o in objs.values():
        o.close()
    ds.close()


def _crops(sc, n=2, size=24, views=(2, 11)):
    out = []
    boxes = {int(b[0]): b for b in sc.objects[0]["boxes"]}
    for v in views[:n]:
        _, x, y, h, w = (int(q) for q in boxes[v])
        out.append((v, x + (w - size) // 2, y + (h - size) // 2, size, size))
    return np.array(out, np.uint32)


def _so3(phi):
    th = np.linalg.norm(phi); K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def _perturb(T, rot_deg, trans, seed):
    """exp(xi^) T with a random rotation axis and translation direction: rotation of rot_deg about the object origin's image, displacement `trans`."""
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    D = np.eye(4); D[:3, :3] = _so3(ax * math.radians(rot_deg)); D[:3, 3] = d * trans
    return D @ T


def _pose_errors(Tow, Tow_true):
    """(rotation error in degrees, displacement of the object's centre in world units)"""
    R = Tow[:3, :3] @ Tow_true[:3, :3].T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2))))
    c = -Tow[:3, :3].T @ Tow[:3, 3]; c0 = -Tow_true[:3, :3].T @ Tow_true[:3, 3]
    return ang, float(np.linalg.norm(c - c0))


def _mat(T16):
    return np.asarray(T16, np.float64).reshape(4, 4).T


def _dn(sc, box):
    v, x0, y0, h, w = (int(q) for q in box)
    py, px = np.mgrid[y0:y0 + h, x0:x0 + w].astype(np.float32)
    a, b = (px - np.float32(sc.cx)) / np.float32(sc.fx), (py - np.float32(sc.cy)) / np.float32(sc.fy)
    return np.sqrt(a * a + b * b + np.float32(1.0)).reshape(-1)


def _huber(x, delta):
    ax = np.abs(x)
    return np.where(ax <= delta, 0.5 * x * x, delta * (ax - 0.5 * delta))


# ------------------------------------------------------------------ 1. the loss is the objective of the render's own samples
@pytest.mark.parametrize("name", ["base", "narrow"])
def test_loss_equals_numpy_restatement(pkg, ss, scene, trained, name):
    sc = scene; _, objs = trained; o = objs[name]; cls = sc.objects[0]["cls"]
    Tow = ss.colmajor(sc.objects[0]["Tow"]); boxes = _crops(sc)
    prm = pkg.pose_refine_default(rays_per_iter=0)
    total, n = 0.0, 0
    for box in boxes:
        t, a, c, cnt = pkg.scene_samples([o], box, ss.colmajor(sc.Twc[int(box[0])]), 0)
        P = cnt.size; t = t.reshape(P, 64).astype(np.float64); a = a.reshape(P, 64).astype(np.float64); c = c.reshape(P, 64, 3).astype(np.float64)
        valid = np.arange(64)[None, :] < cnt.reshape(P, 1)
        a = np.where(valid, a, 0.0)
        incl = np.cumprod(1.0 - a, 1); T = np.concatenate([np.ones((P, 1)), incl[:, :-1]], 1)
        active = np.logical_and.accumulate(T >= EPS, 1) & valid
        w = np.where(active, a * T, 0.0)
        nact = active.sum(1); Tend = np.where(nact > 0, T[np.arange(P), np.maximum(nact - 1, 0)] * (1.0 - a[np.arange(P), np.maximum(nact - 1, 0)]), 1.0)
        rgb_t, m, d = _targets(sc, box, cls)
        r = (w[..., None] * (c - rgb_t[:, None, :])).sum(1)
        O = 1.0 - Tend; D = (w * t).sum(1) / _dn(sc, box)
        hitd = (m > 0) & (d > 0)
        l = prm.w_rgb * m * (r * r).sum(1) / 3.0 + prm.w_mask * (O - m) ** 2 + prm.w_depth * np.where(hitd, _huber(D - d, prm.depth_huber), 0.0)
        total += l.sum(); n += P
    want = total / n
    for side in (0, 1):
        got, g = o.pose_loss(boxes, Tow, prm, side=side)
        print("%s side %d: loss %.7f numpy %.7f" % (name, side, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
        assert np.isfinite(g).all()


# ------------------------------------------------------------------ 2. the gradient is fp64 autograd of the same objective
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("name", ["base", "narrow"])
def test_gradient_matches_fp64_autograd(pkg, orc, ss, scene, trained, name, side, tmp_path):
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch not installed")
    sc = scene; _, objs = trained; o = objs[name]; ob = sc.objects[0]
    boxes = _crops(sc); prm = pkg.pose_refine_default(rays_per_iter=0)
    diag = float(np.linalg.norm(2 * ob["half"]))
    poses = [ob["Tow"], _perturb(ob["Tow"], 3.0, 0.03 * diag, seed=11)]
    aabb = np.stack([-ob["half"], ob["half"]]).astype(np.float32)
    results, cases = [], []
    for Tow in poses:
        T16 = ss.colmajor(Tow)
        loss, g6 = o.pose_loss(boxes, T16, prm, side=side)
        x, raw, dldx = o.pose_samples(boxes, T16, prm, side=side)
        results.append(dict(loss=loss, g6=g6, x=x, raw=raw, dldx=dldx))
        rr = pref.pose_rays(sc, boxes, Tow, aabb, ob["cls"], sample_seed=o.cfg.sample_seed)
        cases.append(dict(x=x, t=rr["t"], hit=rr["hit"], dn=rr["dn"], tgt=rr["tgt"], pos=rr["pos"]))
    refs = pref.reference(tmp_path, pref.net_inputs(o, orc, prm), aabb, cases)
    for i, got in enumerate(results):
        ref = refs[i]; xs = cases[i]["pos"]; want6 = ref["g6"]; ev = ref["ev"]
        want_s = ref["gs"] / got["x"].shape[0]                             # the gradient of the mean
        assert np.abs(got["x"][ev] - xs[ev]).max() < 1e-5, "sample positions"
        assert abs(got["loss"] - ref["loss"]) <= 1e-4 * abs(ref["loss"])
        rel = np.linalg.norm(got["g6"] - want6) / np.linalg.norm(want6)
        gs = got["dldx"][ev]; ws = want_s[ev]
        scale = np.linalg.norm(ws, axis=-1).max()
        # (a floor of 1 % of the largest sample's norm: dL/dO, dL/dh and dL/dE are fp16 in the kernel, as in training)
        ok = np.linalg.norm(gs - ws, axis=-1) <= 2e-2 * np.maximum(np.linalg.norm(ws, axis=-1), 1e-2 * scale)
        print("%s side %d pose %d: loss %.6f grad6 %s ref %s rel %.2e; per-sample within bar %.5f of %d" % (name, side, i, got["loss"],
              np.array2string(got["g6"], precision=5), np.array2string(want6, precision=5), rel, ok.mean(), ok.size))
        assert rel <= 1e-2, rel
        assert ok.mean() >= 0.999, ok.mean()


# ------------------------------------------------------------------ 3. refinement pulls a perturbed pose back
CONV_ROT_DEG, CONV_TRANS_FRAC = 0.5, 0.005          # bars: see the docstring
DRIFT_ROT_DEG, DRIFT_TRANS_FRAC = 0.5, 0.0025
COARSE = dict(sample_seed=9, n_levels=8, per_level_scale=1.5)


@pytest.fixture(scope="module")
def conv_object(pkg, ss, scene):
    sc = scene
    ds, o = ge.make_problem(pkg, sc, COARSE, use_depth=True)
    o.set_backend(1); o.train(500)
    yield ds, o
    o.close(); ds.close()


def _six_boxes(sc):
    b = sc.objects[0]["boxes"]
    return b[np.linspace(0, len(b) - 1, 6).astype(int)]


def test_refinement_converges(pkg, ss, scene, conv_object):
    """24 views of 240 x 320, 500 training iterations on the true pose of an 8-level grid with per-level scale 1.5 (finest resolution 273); the pose
    perturbed by 5 degrees and 5 % of the box diagonal (three seeds), the defaults (100 steps of 4096 rays) on 6 boxes.  Measured on an MI355X: rotation
    0.124 / 0.116 / 0.149 degrees, centre 0.091 / 0.053 / 0.020 % of the diagonal, loss 0.066 -> 0.0005; from the true pose 0.232 degrees and 0.071 %.
    Bars: rotation <= 0.5 degrees and centre <= 0.5 % of the diagonal (>= 3x margin), the loss trace ending below half its start; the drift from the true
    pose <= 0.5 degrees and 0.25 % (>= 2x margin).  The drift is the Adam steps' noise floor (lr_rot 4e-3 rad = 0.23 degrees per step), so it cannot sit
    below a tenth of the convergence bars at these step sizes.  base.json's grid (16 levels, finest resolution 2^19) is not used here: its position gradient
    is dominated by the finest levels and does not point downhill on the pose scale."""
    sc = scene; _, o = conv_object; ob = sc.objects[0]
    diag = float(np.linalg.norm(2 * ob["half"])); boxes = _six_boxes(sc); prm = pkg.pose_refine_default()
    for seed in (1, 2, 3):
        T0 = _perturb(ob["Tow"], 5.0, 0.05 * diag, seed)
        pose, trace = o.refine_pose(boxes, ss.colmajor(T0), prm)
        e0 = _pose_errors(T0, ob["Tow"]); e1 = _pose_errors(_mat(pose), ob["Tow"])
        print("seed %d: rotation %.3f -> %.4f deg, centre %.4f -> %.5f (%.3f%% of the diagonal), loss %.5f -> %.5f" % (seed, e0[0], e1[0], e0[1], e1[1],
              100 * e1[1] / diag, trace[0], trace[-1]))
        assert np.isfinite(trace).all() and trace[-1] < 0.5 * trace[0], trace[[0, -1]]
        assert e1[0] <= CONV_ROT_DEG and e1[1] <= CONV_TRANS_FRAC * diag, (e1, diag)
    pose, trace = o.refine_pose(boxes, ss.colmajor(ob["Tow"]), prm)
    e = _pose_errors(_mat(pose), ob["Tow"])
    print("from the true pose: drift %.4f deg, %.5f" % e)
    assert e[0] <= DRIFT_ROT_DEG and e[1] <= DRIFT_TRANS_FRAC * diag, e


# ------------------------------------------------------------------ 4. / 5. read-only and deterministic
def _snapshot_state(o, box, Twc):
    i = o.info()
    st = tuple(getattr(i, f) for f, _ in type(i)._fields_)
    rgb, depth, mask = o.render(box, Twc)
    return [o.get_params(0), o.get_params(1), o.get_params(2)], st, (o.render_skip_stats(0), o.render_skip_stats(1)), (rgb, depth, mask)


def test_refinement_is_read_only_and_deterministic(pkg, ss, scene):
    sc = scene; ob = sc.objects[0]
    ds, a = ge.make_problem(pkg, sc, dict(sample_seed=13), use_depth=True)
    _, b = ge.make_problem(pkg, sc, dict(sample_seed=13), use_depth=True, dataset=ds)
    try:
        a.set_backend(1); b.set_backend(1); a.train(200); b.train(200)
        box = sc.objects[0]["boxes"][3]; Twc = ss.colmajor(sc.Twc[int(box[0])])
        before = _snapshot_state(a, box, Twc)
        T0 = ss.colmajor(_perturb(ob["Tow"], 3.0, 0.02, 4)); boxes = _six_boxes(sc); prm = pkg.pose_refine_default(iters=20)
        p1, t1 = a.refine_pose(boxes, T0, prm, side=0)
        p2, t2 = a.refine_pose(boxes, T0, prm, side=0)
        p3, t3 = a.refine_pose(boxes, T0, prm, side=1)
        assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t2.view(np.uint32))
        assert np.array_equal(p1.view(np.uint32), p3.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t3.view(np.uint32))   # same weights
        l1, g1 = a.pose_loss(boxes, T0, prm, iteration=7); l2, g2 = a.pose_loss(boxes, T0, prm, iteration=7)
        assert l1 == l2 and np.array_equal(g1, g2)
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


# ------------------------------------------------------------------ 6. the online path while the manager trains
def test_online_refine_while_training(pkg, ss, scene):
    sc = scene; ob = sc.objects[0]
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    for v in range(sc.n_views):
        m.new_frame(v, "%.6f" % (v * 0.1), sc.rgb[v][..., ::-1], sc.instance[v], ss.colmajor(sc.Twc[v]))
    idx = m.create_nerf(ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    boxes = _six_boxes(sc); prm = pkg.pose_refine_default(iters=20)
    T0 = ss.colmajor(_perturb(ob["Tow"], 3.0, 0.02, 5))
    with pytest.raises(pkg.MonError) as e:
        m.refine_pose(idx, boxes, T0, prm)                  # nothing published yet
    assert e.value.code == 5
    seen = dict(n=0, err=None); stop = threading.Event()

    def frontend():
        try:
            while not stop.is_set():
                try:
                    p, tr = m.refine_pose(idx, boxes, T0, prm)
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
    a = m.refine_pose(idx, boxes, T0, prm)
    b = m.object(idx).refine_pose(boxes, T0, prm, side=1)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    m.close()


# ------------------------------------------------------------------ 7. errors
def test_pose_refine_errors(pkg, ss, scene, trained):
    sc = scene; ds, objs = trained; ob = sc.objects[0]
    T = ss.colmajor(ob["Tow"]); boxes = _crops(sc); prm = pkg.pose_refine_default(iters=2)
    _, c = ge.make_problem(pkg, sc, dict(n_neurons=16), dataset=ds)
    _, x = ge.make_problem(pkg, sc, dict(rng_flags=1), dataset=ds)
    _, fresh = ge.make_problem(pkg, sc, dict(), dataset=ds)
    try:
        for o, side in ((c, 0), (x, 0), (fresh, 1)):
            with pytest.raises(pkg.MonError) as e:
                o.refine_pose(boxes, T, prm, side=side)
            assert e.value.code == 5, side
        o = objs["base"]
        bad = boxes.copy(); bad[0, 0] = 200                               # a frame the dataset does not hold
        for b in (bad, np.array([[2, sc.W - 10, 0, 8, 16]], np.uint32), np.array([[2, 0, sc.H - 4, 8, 8]], np.uint32), np.array([[2, 0, 0, 0, 8]], np.uint32)):
            for call in (lambda: o.refine_pose(b, T, prm), lambda: o.pose_loss(b, T, prm, side=1)):
                with pytest.raises(pkg.MonError) as e:
                    call()
                assert e.value.code == 1
    finally:
        for q in (c, x, fresh):
            q.close()
