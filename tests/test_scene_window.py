"""GPU tests (-m gpu) of joint refinement of a window of camera poses and object poses (mon_scene_window_loss, mon_scene_refine_window,
mon_online_refine_window, mon_object_set_pose, mon_online_set_object_pose; kernels k_scene_window_rays, k_scene_window_composite, k_scene_window_obj,
k_scene_window_update).  The contract is include/mon_core.h's and DESIGN.md 3.4h's: every frame of a window equals its single-frame call bit for bit, the
object gradient equals one fp64 autograd graph of the objective at the bars of tests/test_pose_shapes.py, cameras-only refinement equals F separate
refinements bit for bit, the objects move by the stated step, nothing about the objects, the dataset or a manager changes, and a stored object pose is what
training, renders and checkpoints see."""
import ctypes as C
import math
import os
import threading
import zlib

import numpy as np
import pytest

from conftest import ROOT                                    # (first: it puts the repository root on the path)
import __graft_entry__ as ge                                # noqa: E402
import pose_reference as pref                               # noqa: E402
import scene_pose_reference as sref                         # noqa: E402

pytestmark = pytest.mark.gpu

BASE = dict(sample_seed=5, use_depth=1)                     # base.json: 16 levels, 64 x 1
NARROW = dict(sample_seed=7, n_neurons=32, n_hidden_layers=2, use_depth=1)
COARSE = dict(sample_seed=9, n_levels=8, per_level_scale=1.5, use_depth=1)
LOSS_RTOL, G6_RTOL = 1e-4, 1e-2                             # the bars of this arithmetic chain (tests/test_pose_shapes.py, used by tests/test_scene_track.py)
ADAM_ROT_DEG, ADAM_TRANS = 0.23, 2e-3
VIEW = 23
# every-pixel crops of test 3 (x, y, h, w): view 23's is test_scene_track's; views 22 and 21 lie over the seam between the two objects' silhouettes
CROPS = {23: (194, 91, 48, 48), 22: (186, 92, 48, 48), 21: (190, 90, 48, 48)}


@pytest.fixture(scope="module")
def scene(ss):
    return ss.make_scene(n_views=24, H=240, W=320, f=260.0, n_objects=3, seed=3, elev_deg=10.0)


def _object(pkg, ss, ds, sc, k, kw, inflate=1.0, steps=300):
    ob = sc.objects[k]
    o = pkg.ObjectNeRF(ds, pkg.default_config(**kw), ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"] * inflate, ob["half"] * inflate)
    o.add_boxes(ob["boxes"]); o.set_backend(1)
    if steps:
        o.train(steps)
    return o


@pytest.fixture(scope="module")
def trained(pkg, ss, scene):
    """test_scene_track's objects (300 iterations each with depth), and object 2 as a 32 x 2 network for K = 3"""
    sc = scene
    ds, b0 = ge.make_problem(pkg, sc, BASE, use_depth=True, obj_index=0)
    b0.close()
    objs = dict(b0=_object(pkg, ss, ds, sc, 0, BASE, inflate=5.0), n1=_object(pkg, ss, ds, sc, 1, NARROW),
                a0=_object(pkg, ss, ds, sc, 0, BASE), a1=_object(pkg, ss, ds, sc, 1, BASE),
                c0=_object(pkg, ss, ds, sc, 0, COARSE), c1=_object(pkg, ss, ds, sc, 1, COARSE), n2=_object(pkg, ss, ds, sc, 2, NARROW))
    yield ds, objs
    for o in objs.values():
        o.close()
    ds.close()


def _meta(sc, k, o, inflate=1.0, Tow=None):
    ob = sc.objects[k]
    return dict(Tow=ob["Tow"] if Tow is None else Tow, aabb=np.stack([-ob["half"] * inflate, ob["half"] * inflate]).astype(np.float32), cls=ob["cls"],
                sample_seed=o.cfg.sample_seed)


def _view_boxes(sc, v, ks, pad=16):
    out = []
    for k in ks:
        b = [q for q in sc.objects[k]["boxes"] if int(q[0]) == v][0]
        _, x, y, h, w = (int(q) for q in b)
        x0, y0 = max(0, x - pad), max(0, y - pad); x1, y1 = min(sc.W, x + w + pad), min(sc.H, y + h + pad)
        out.append((v, x0, y0, y1 - y0, x1 - x0))
    return np.array(out, np.uint32)


def _so3(phi):
    th = np.linalg.norm(phi); K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def _se3(xi):
    """exp(xi^), xi = (rho, phi), in fp64 (closed form)"""
    rho, phi = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(phi); K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    V = np.eye(3) + 0.5 * K + K @ K / 6 if th < 1e-9 else np.eye(3) + (1 - math.cos(th)) / th ** 2 * K + (th - math.sin(th)) / th ** 3 * K @ K
    T = np.eye(4); T[:3, :3] = _so3(phi); T[:3, 3] = V @ rho
    return T


def _perturb_camera(Twc, rot_deg, trans, seed):
    """Twc D: the camera turned by rot_deg about its own centre and moved by `trans` (random axis and direction)"""
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    D = np.eye(4); D[:3, :3] = _so3(ax * math.radians(rot_deg)); D[:3, 3] = d * trans
    return Twc @ D


def _perturb_object(Tow, rot_deg, trans, seed):
    """D Tow: the object frame turned by rot_deg about its own origin and moved by `trans`"""
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    D = np.eye(4); D[:3, :3] = _so3(ax * math.radians(rot_deg)); D[:3, 3] = d * trans
    return D @ Tow


def _pose_errors(T, T_true):
    R = T[:3, :3].T @ T_true[:3, :3]
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def _mat(T16):
    return np.asarray(T16, np.float64).reshape(4, 4).T


def _cam_dist(sc, v):
    c = np.mean([-ob["Tow"][:3, :3].T @ ob["Tow"][:3, 3] for ob in sc.objects[:2]], 0)
    return float(np.linalg.norm(sc.Twc[v][:3, 3] - c))


def _diag(sc, k):
    return float(np.linalg.norm(2 * sc.objects[k]["half"]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _window(frames):
    """frames: [(boxes of one frame, Twc16)] -> (obs, Twc16s)"""
    return np.concatenate([np.asarray(b, np.uint32).reshape(-1, 5) for b, _ in frames]), np.stack([np.asarray(T, np.float32).reshape(16) for _, T in frames])


_SINGLE = {}                                                # single-frame results, computed once and shared by the tests of this module


def _single(pkg, key, objs, boxes, Twc16, prm, side=0, iteration=0, lw=None):
    k = (key, np.asarray(boxes, np.uint32).tobytes(), np.asarray(Twc16, np.float32).tobytes(), int(prm.rays_per_iter), int(prm.seed), side, iteration,
         None if lw is None else np.asarray(lw, np.float32).tobytes())
    if k not in _SINGLE:
        _SINGLE[k] = pkg.scene_pose_loss(objs, boxes, Twc16, prm, side=side, iteration=iteration, level_weights=lw)
    return _SINGLE[k]


def _check_frames(pkg, tag, key, objs, frames, prm, side=0, iteration=0, lw=None):
    """the window call over `frames` against each frame's single call, bit for bit; returns the window's outputs"""
    obs, Twc = _window(frames)
    L, fl, cg, og = pkg.scene_window_loss(objs, obs, Twc, None, prm, side=side, iteration=iteration, level_weights=lw)
    acc = np.float32(0)
    for f, (boxes, T) in enumerate(frames):
        ls, gs = _single(pkg, key, objs, boxes, T, prm, side, iteration, lw)
        assert _bits(fl[f]) == _bits(ls), (tag, f, fl[f], ls)
        assert np.array_equal(_bits(cg[f]), _bits(gs)), (tag, f, cg[f], gs)
        acc = np.float32(acc + fl[f])
    assert _bits(L) == _bits(acc), (tag, L, acc)                               # L = sum_f L_f in window order, fp32
    assert np.isfinite(og).all()
    return L, fl, cg, og


# ------------------------------------------------------------------ 1. every frame equals its single call
def test_every_frame_equals_its_single_call(pkg, ss, scene, trained):
    """frame_loss and cam_grad6 of mon_scene_window_loss against mon_scene_pose_loss per frame, by their bits: three every-pixel frames of unequal size (a
    48 x 48 crop, a 40 x 33 crop, a 1-pixel box); three frames of 257 drawn rays (no multiple of the wave count or of 256) with K = 1, 2, 3; 3 x 6000 drawn
    rays (two passes, the second ragged); a frame of exactly 16384 rays next to a small one, in both orders; side 1; a c2f weight row; a frame no object's box
    covers (mask term only, gradient 0); the same frames in another order and alone; the call repeated."""
    sc = scene; _, o = trained
    T = {v: ss.colmajor(_perturb_camera(sc.Twc[v], 1.0, 0.01, v)) for v in (20, 21, 22, 23)}
    pair, three = [o["c0"], o["c1"]], [o["b0"], o["n1"], o["n2"]]
    p_all = pkg.pose_refine_default(rays_per_iter=0)
    A = (np.array([[23, 194, 91, 48, 48]], np.uint32), T[23]); B = (np.array([[22, 186, 92, 33, 40]], np.uint32), T[22])
    C1 = (np.array([[21, 180, 110, 1, 1]], np.uint32), T[21])
    _check_frames(pkg, "every-pixel", "pair", pair, [A, B, C1], p_all)
    _check_frames(pkg, "every-pixel K = 3", "three", three, [A, B, C1], p_all)
    # drawn rays over the padded boxes of two objects per frame; K = 1, 2, 3
    D = [(_view_boxes(sc, v, (0, 1)), T[v]) for v in (23, 22, 21)]
    p257 = pkg.pose_refine_default(rays_per_iter=257)
    for key, objs in (("one", [o["a0"]]), ("pair", pair), ("three", three)):
        _check_frames(pkg, "257 drawn, K = %d" % len(objs), key, objs, D, p257, iteration=7)
    # position independence: another order, and alone
    L1, fl1, cg1, og1 = _check_frames(pkg, "257 drawn", "pair", pair, D, p257, iteration=7)
    L2, fl2, cg2, og2 = _check_frames(pkg, "257 drawn, reordered", "pair", pair, [D[2], D[0], D[1]], p257, iteration=7)
    assert np.array_equal(_bits(fl2), _bits(fl1[[2, 0, 1]])) and np.array_equal(_bits(cg2), _bits(cg1[[2, 0, 1]]))
    L3, fl3, cg3, og3 = _check_frames(pkg, "257 drawn, alone", "pair", pair, [D[1]], p257, iteration=7)
    assert _bits(fl3[0]) == _bits(fl1[1]) and _bits(L3) == _bits(fl1[1])
    # the repeated call
    L4, fl4, cg4, og4 = _check_frames(pkg, "257 drawn, again", "pair", pair, D, p257, iteration=7)
    assert _bits(L4) == _bits(L1) and np.array_equal(_bits(fl4), _bits(fl1)) and np.array_equal(_bits(cg4), _bits(cg1))
    assert np.array_equal(_bits(og4), _bits(og1))
    # two passes, the second ragged (6000 + 6000 | 6000)
    _check_frames(pkg, "3 x 6000 drawn", "pair", pair, D, pkg.pose_refine_default(rays_per_iter=6000), iteration=3)
    # a frame of exactly 16384 rays (128 x 128 pixels) next to a small one
    big = (np.array([[23, 150, 60, 128, 128]], np.uint32), T[23])
    _check_frames(pkg, "16384 + small", "pair", pair, [big, B], p_all)
    _check_frames(pkg, "small + 16384", "pair", pair, [B, big], p_all)
    # side 1, and a c2f weight row (Lmax = 16 with a base.json object in the list)
    _check_frames(pkg, "side 1", "three", three, D, p257, side=1, iteration=7)
    lw = pkg.pose_c2f_weights(16, 100, 35)
    _, _, cgw, ogw = _check_frames(pkg, "c2f row", "three", three, D, p257, iteration=7, lw=lw)
    _, _, cg0, og0 = _check_frames(pkg, "no weights", "three", three, D, p257, iteration=7)
    assert not np.array_equal(_bits(cgw), _bits(cg0)) and not np.array_equal(_bits(ogw), _bits(og0))
    # a frame none of the objects' boxes covers: 16 x 16 pixels of object 2's silhouette in view 20 under a camera turned away by 120 degrees -- every ray
    # misses every box, m*_2 = 1 on every pixel
    Daway = np.eye(4); Daway[:3, :3] = _so3(np.array([0.0, math.radians(120.0), 0.0]))
    away = (np.array([[20, 34, 122, 16, 16]], np.uint32), ss.colmajor(sc.Twc[20] @ Daway))
    tight = [o["a0"], o["a1"], o["n2"]]                                       # (true boxes: the camera stands outside all of them)
    L, fl, cg, og = _check_frames(pkg, "uncovered frame", "tight", tight, [A, away, B], p_all)
    print("uncovered frame: loss %.6f, cam grad6 %s" % (fl[1], cg[1]))
    assert fl[1] > 0 and (cg[1] == 0).all(), (fl[1], cg[1])
    Lx, flx, cgx, ogx = _check_frames(pkg, "uncovered frame alone", "tight", tight, [away], p_all)
    assert (ogx == 0).all() and (cgx == 0).all()


# ------------------------------------------------------------------ 2. object poses passed in Tow16s
@pytest.fixture(scope="module")
def twin(pkg, ss, scene, trained, tmp_path_factory):
    """a checkpoint twin of object n1 holding T' = object 1's Tow 3 degrees / 3 % of its box diagonal off, set with mon_object_set_pose"""
    sc = scene; ds, o = trained
    path = str(tmp_path_factory.mktemp("window") / "n1.ckpt")
    o["n1"].save(path)
    t = pkg.ObjectNeRF.load(ds, path)
    Tp = _perturb_object(sc.objects[1]["Tow"], 3.0, 0.03 * _diag(sc, 1), 21)
    t.set_pose(ss.colmajor(Tp))
    yield t, Tp
    t.close()


def test_object_poses_passed_in_Tow16s(pkg, ss, scene, trained, twin):
    """mon_scene_pose_loss on {b0, the twin holding T'} equals, bit for bit per frame, the window call on {b0, n1} with Tow16s = {Tow_0, T'}; with
    Tow16s = the objects' own poses the window call equals Tow16s = NULL"""
    sc = scene; _, o = trained; tw, Tp = twin
    frames = [(_view_boxes(sc, v, (0, 1)), ss.colmajor(sc.Twc[v])) for v in (23, 22, 21)]
    obs, Twc = _window(frames); prm = pkg.pose_refine_default(rays_per_iter=1024)
    Tow = np.stack([ss.colmajor(sc.objects[0]["Tow"]), ss.colmajor(Tp)])
    L, fl, cg, og = pkg.scene_window_loss([o["b0"], o["n1"]], obs, Twc, Tow, prm, iteration=5)
    for f, (boxes, T) in enumerate(frames):
        ls, gs = pkg.scene_pose_loss([o["b0"], tw], boxes, T, prm, iteration=5)
        assert _bits(fl[f]) == _bits(ls) and np.array_equal(_bits(cg[f]), _bits(gs)), (f, fl[f], ls)
    L0, fl0, cg0, og0 = pkg.scene_window_loss([o["b0"], o["n1"]], obs, Twc, None, prm, iteration=5)
    assert not np.array_equal(_bits(fl0), _bits(fl))
    own = np.stack([ss.colmajor(sc.objects[0]["Tow"]), ss.colmajor(sc.objects[1]["Tow"])])
    L1, fl1, cg1, og1 = pkg.scene_window_loss([o["b0"], o["n1"]], obs, Twc, own, prm, iteration=5)
    assert np.array_equal(_bits(fl1), _bits(fl0)) and np.array_equal(_bits(cg1), _bits(cg0)) and np.array_equal(_bits(og1), _bits(og0))


# ------------------------------------------------------------------ 3. the object gradient against fp64 autograd
WINDOW3 = (23, 22, 21)


@pytest.mark.parametrize("drawn", [False, True])
@pytest.mark.parametrize("off", [False, True])
def test_object_gradient_matches_fp64_autograd(pkg, orc, ss, scene, trained, twin, tmp_path, drawn, off):
    """{object 0 on its 5x box, object 1 as 32 x 2} over views 23, 22, 21: every pixel of one 48 x 48 crop per view, or 2048 drawn rays per frame over the
    padded boxes at iteration 7; at the dataset poses, or with the cameras 3 degrees / 3 % of their distance off and object 1's Tow 3 degrees / 3 % of its box
    diagonal off.  Per frame the device's own samples (mon_debug_scene_pose_samples) go through the fp64 autograd graph of tests/scene_pose_reference.py;
    obj_grad6_j = sum_f (sum gs_j, sum x_o x gs_j) / P_f in fp64.  Bars: each frame's loss 1e-4 relative, each 6-vector 1e-2 of its largest component.  Rays
    within 0.1 % of a cut are left out on both sides -- of each frame's loss, of its camera gradient and of the object gradients; the device's share of them
    is the fp64 composite of its own dumped outputs (loss) and its per-sample dump (gradients) -- at most 1 % of a case's rays."""
    sc = scene; _, o = trained; tw, Tp = twin
    objs = [o["b0"], o["n1"]]; dump_objs = [o["b0"], tw if off else o["n1"]]
    Tow1 = _mat(ss.colmajor(Tp)) if off else sc.objects[1]["Tow"]             # (T' as the device holds it)
    metas = [_meta(sc, 0, o["b0"], 5.0), _meta(sc, 1, o["n1"], Tow=Tow1)]
    prm = pkg.pose_refine_default(rays_per_iter=2048 if drawn else 0); it = 7 if drawn else 0
    frames = []
    for v in WINDOW3:
        boxes = _view_boxes(sc, v, (0, 1)) if drawn else np.array([[v, *CROPS[v]]], np.uint32)
        Tc = _perturb_camera(sc.Twc[v], 3.0, 0.03 * _cam_dist(sc, v), 11 + v) if off else sc.Twc[v]
        frames.append((boxes, ss.colmajor(Tc)))
    obs, Twc = _window(frames)
    Tow = np.stack([ss.colmajor(sc.objects[0]["Tow"]), ss.colmajor(Tow1)])
    L, fl, cg, og = pkg.scene_window_loss(objs, obs, Twc, Tow, prm, iteration=it)
    nets = [dict(pref.net_inputs(q, orc, prm), aabb=m["aabb"]) for q, m in zip(objs, metas)]
    cases, dumps_all, rss = [], [], []
    for boxes, T16 in frames:
        rs = sref.scene_rays(sc, boxes, _mat(T16), metas, n_rays=int(prm.rays_per_iter), seed=prm.seed, iteration=it)
        dumps = [pkg.scene_pose_samples(dump_objs, boxes, T16, k, prm, iteration=it) for k in range(2)]
        Toc = np.stack([np.asarray(m["Tow"], np.float64) @ _mat(T16) for m in metas])
        rss.append(rs)
        cases.append(dict(x_o=np.stack([d["x_o"] for d in dumps]), x_c=np.stack([d["x_c"] for d in dumps]), t=np.stack([d["t"] for d in dumps]),
                          count=np.stack([d["count"] for d in dumps]), dn=rs["dn"], cstar=rs["cstar"], mstar=np.stack([q["mstar"] for q in rs["objs"]]),
                          dstar=rs["dstar"], Toc=Toc, lw=None))
        dumps_all.append(dumps)
    refs = sref.reference(tmp_path, nets, cases, (prm.w_rgb, prm.w_mask, prm.w_depth, prm.depth_huber), tag="win")
    tag = "%s %s" % ("drawn" if drawn else "crops", "off" if off else "true")
    n_amb = sum(int(r["amb"].sum()) for r in refs); n_all = sum(r["amb"].size for r in refs)
    print("%s: %d of %d rays within 0.1 %% of a cut" % (tag, n_amb, n_all))
    assert n_amb <= n_all // 100, (tag, n_amb, n_all)
    og_ref = np.zeros((2, 6)); og_dev = og.astype(np.float64).copy()
    for f, (ref, dumps, case) in enumerate(zip(refs, dumps_all, cases)):
        P = ref["amb"].size; ok = ~ref["amb"]
        # the frame's loss and camera gradient without the rays left out: the fp64 side sums the rays kept; the device's share of the others is the fp64
        # composite of its own dumped outputs (loss) and its per-sample dump mapped by g_c = R_oc^T g_o, (sum g_c, sum x_c x g_c) (gradient)
        l_ref = ref["l"][ok].sum() / P; l_dev = float(fl[f]); g_ref = np.zeros(6); g_dev = cg[f].astype(np.float64).copy()
        if not ok.all():
            lists = [sref.lists_from_raw(d["raw"], d["t"], rss[f]["objs"][j]["hit"]) for j, d in enumerate(dumps)]
            npc = sref.np_composite_grad(np.stack([d["t"] for d in dumps]), np.stack([q[0] for q in lists]), np.stack([q[1] for q in lists]),
                                         np.stack([d["count"].astype(np.uint32) for d in dumps]), rss[f]["cstar"], case["mstar"], rss[f]["dstar"], rss[f]["dn"],
                                         (prm.w_rgb, prm.w_mask, prm.w_depth, prm.depth_huber))
            l_dev -= npc["l"][~ok].sum() / P
        for j in range(2):
            ev = (np.arange(64)[None, :] < case["count"][j][:, None])
            x = case["x_o"][j].astype(np.float64); g = np.where((ev & ok[:, None])[..., None], ref["gs"][j], 0.0) / P
            og_ref[j, :3] += g.sum((0, 1)); og_ref[j, 3:] += np.cross(x, g).sum((0, 1))
            gd = np.where((ev & ~ok[:, None])[..., None], dumps[j]["dldx"].astype(np.float64), 0.0)      # the device's share of the rays left out
            og_dev[j, :3] -= gd.sum((0, 1)); og_dev[j, 3:] -= np.cross(x, gd).sum((0, 1))
            R = case["Toc"][j][:3, :3]; xc = case["x_c"][j].astype(np.float64)
            gc = g @ R; g_ref[:3] += gc.sum((0, 1)); g_ref[3:] += np.cross(xc, gc).sum((0, 1))
            gc = gd @ R; g_dev[:3] -= gc.sum((0, 1)); g_dev[3:] -= np.cross(xc, gc).sum((0, 1))
        if ok.all():                                                          # (nothing left out: the graph's own mean and grad6)
            assert abs(l_ref - ref["loss"]) <= 1e-9 * abs(ref["loss"]) and np.abs(g_ref - ref["g6"]).max() <= 1e-6 * np.abs(ref["g6"]).max()
            l_ref, g_ref = ref["loss"], ref["g6"]
        print("%s frame %d: %d rays left out, loss %.6f (fp64 %.6f, rel %.2e), cam grad6 rel %.2e" % (tag, f, int((~ok).sum()), l_dev, l_ref,
              abs(l_dev - l_ref) / abs(l_ref), np.abs(g_dev - g_ref).max() / np.abs(g_ref).max()))
        assert abs(l_dev - l_ref) <= LOSS_RTOL * abs(l_ref), (tag, f, l_dev, l_ref)
        assert np.abs(g_dev - g_ref).max() <= G6_RTOL * np.abs(g_ref).max(), (tag, f, g_dev, g_ref)
    for j in range(2):
        rel = np.abs(og_dev[j] - og_ref[j]).max() / np.abs(og_ref[j]).max()
        print("%s object %d: obj_grad6 rel %.2e  %s" % (tag, j, rel, og_ref[j]))
        assert rel <= G6_RTOL, (tag, j, og_dev[j], og_ref[j])


def test_one_object_one_frame_equals_the_object_route(pkg, ss, scene, trained):
    """K = 1, F = 1 at the dataset's Twc: obj_grad6 is mon_object_pose_loss's grad6 and the loss that call's, each within twice the fp64 bars (each side is
    within one bar of the same reference); level weights of 0 give both gradients exactly 0, weights of 1 the bits of NULL"""
    sc = scene; _, objs = trained
    for name, k in (("a0", 0), ("n1", 1), ("c1", 1)):
        o = objs[name]; ob = sc.objects[k]
        Twc16 = ss.colmajor(sc.Twc[VIEW]); Tow16 = ss.colmajor(ob["Tow"])
        for prm, it in ((pkg.pose_refine_default(rays_per_iter=0), 0), (pkg.pose_refine_default(rays_per_iter=2048), 7)):
            # (a frame holds at most 16384 rays: every pixel of a 96 x 96 crop over the object, the draws over its padded box)
            boxes = _view_boxes(sc, VIEW, (k,)) if prm.rays_per_iter else np.array([[VIEW, 170, 80, 96, 96]], np.uint32)
            L, fl, cg, og = pkg.scene_window_loss([o], boxes, Twc16, None, prm, iteration=it)
            lo, go = o.pose_loss(boxes, Tow16, prm, iteration=it)
            print("%s rays %d: loss %.6f / %.6f, obj_grad6 rel %.2e" % (name, prm.rays_per_iter, L, lo, np.abs(og[0] - go).max() / np.abs(go).max()))
            assert abs(L - lo) <= 2 * LOSS_RTOL * abs(lo), (name, L, lo)
            assert np.abs(og[0] - go).max() <= 2 * G6_RTOL * np.abs(go).max(), (name, og[0], go)
            nl = o.cfg.n_levels
            L0, fl0, cg0, og0 = pkg.scene_window_loss([o], boxes, Twc16, None, prm, iteration=it, level_weights=np.zeros(nl, np.float32))
            L1, fl1, cg1, og1 = pkg.scene_window_loss([o], boxes, Twc16, None, prm, iteration=it, level_weights=np.ones(nl, np.float32))
            assert _bits(L0) == _bits(L) and (cg0 == 0).all() and (og0 == 0).all()
            assert _bits(L1) == _bits(L) and np.array_equal(_bits(cg1), _bits(cg)) and np.array_equal(_bits(og1), _bits(og))


# ------------------------------------------------------------------ 4. cameras only equals F separate refinements
@pytest.mark.parametrize("c2f", [None, True])
def test_cameras_only_equals_separate_refinements(pkg, ss, scene, trained, c2f):
    """refine_objects = 0, n_fixed_frames = 0, 5 steps: every final Twc_f and every column of frame_trace equal mon_scene_refine_camera of that frame, bit for
    bit; with n_fixed_frames = 1 frame 0 comes back as given and the others as before"""
    sc = scene; _, o = trained; pair = [o["a0"], o["a1"]]
    frames = [(_view_boxes(sc, v, (0, 1)), ss.colmajor(_perturb_camera(sc.Twc[v], 2.0, 0.02, v))) for v in (23, 21, 22)]
    obs, Twc0 = _window(frames); prm = pkg.pose_refine_default(iters=5, rays_per_iter=1024)
    Twc, Tow, trace, ftrace = pkg.scene_refine_window(pair, obs, Twc0, None, prm, c2f=c2f, window=dict(n_fixed_frames=0, refine_objects=0))
    assert Tow is None and trace.shape == (6,) and ftrace.shape == (6, 3)
    for f, (boxes, T) in enumerate(frames):
        pose, tr = pkg.scene_refine_camera(pair, boxes, T, prm, c2f=c2f)
        assert np.array_equal(_bits(Twc[f]), _bits(pose)), (f, Twc[f], pose)
        assert np.array_equal(_bits(ftrace[:, f]), _bits(tr)), (f, ftrace[:, f], tr)
        assert not np.array_equal(_bits(pose), _bits(T))
    for i in range(6):
        acc = np.float32(0)
        for f in range(3):
            acc = np.float32(acc + ftrace[i, f])
        assert _bits(trace[i]) == _bits(acc)
    own = np.stack([ss.colmajor(sc.objects[k]["Tow"]) for k in (0, 1)])
    Twc1, Tow1, trace1, ftrace1 = pkg.scene_refine_window(pair, obs, Twc0, own, prm, c2f=c2f, window=dict(n_fixed_frames=1, refine_objects=0))
    assert np.array_equal(_bits(Twc1[0]), _bits(Twc0[0])) and np.array_equal(_bits(Twc1[1:]), _bits(Twc[1:]))
    assert np.array_equal(_bits(Tow1), _bits(own))                          # refine_objects = 0: the object poses come back as given
    assert np.array_equal(_bits(ftrace1[:, 1:]), _bits(ftrace[:, 1:])) and _bits(ftrace1[0, 0]) == _bits(ftrace[0, 0])


# ------------------------------------------------------------------ 5. the objects move as stated
def test_objects_move_as_stated(pkg, ss, scene, trained):
    """every frame fixed, refine_objects = 1: loss_trace[0] is mon_scene_window_loss at the start and loss_trace[iters] that call at the returned poses with
    iteration = iters, bit for bit; the cameras come back as given; after one step Tow_j = exp(delta^) Tow_j with Adam's first step
    delta = -lr g / (|g| + 1e-8), in fp64 from obj_grad6, within 1e-6 per matrix entry"""
    sc = scene; _, o = trained; pair = [o["c0"], o["c1"]]
    frames = [(_view_boxes(sc, v, (0, 1)), ss.colmajor(sc.Twc[v])) for v in (22, 23)]
    obs, Twc0 = _window(frames)
    Tow0 = np.stack([ss.colmajor(_perturb_object(sc.objects[k]["Tow"], 2.0, 0.02 * _diag(sc, k), 31 + k)) for k in (0, 1)])
    wp = pkg.window_default(n_fixed_frames=2, refine_objects=1)
    for iters in (3, 1):
        prm = pkg.pose_refine_default(iters=iters, rays_per_iter=1024)
        Twc, Tow, trace, ftrace = pkg.scene_refine_window(pair, obs, Twc0, Tow0, prm, window=wp)
        assert np.array_equal(_bits(Twc), _bits(Twc0))
        L0, _, _, og = pkg.scene_window_loss(pair, obs, Twc0, Tow0, prm, iteration=0)
        L1, fl1, _, _ = pkg.scene_window_loss(pair, obs, Twc, Tow, prm, iteration=iters)
        assert _bits(trace[0]) == _bits(L0) and _bits(trace[iters]) == _bits(L1), (trace, L0, L1)
        assert np.array_equal(_bits(ftrace[iters]), _bits(fl1))
    for j in range(2):
        g = og[j].astype(np.float64); lr = np.array([wp.lr_obj_trans] * 3 + [wp.lr_obj_rot] * 3, np.float64)
        want = _se3(-lr * g / (np.abs(g) + 1e-8)) @ _mat(Tow0[j])
        err = np.abs(_mat(Tow[j]) - want).max()
        print("object %d: largest entry difference from exp(delta^) Tow %.2e" % (j, err))
        assert err <= 1e-6, (j, err)
        assert not np.array_equal(_bits(Tow[j]), _bits(Tow0[j]))


# ------------------------------------------------------------------ 6. a refinement run, measured
# 100 default steps over views 20-23: frame 0 fixed at its dataset pose, the other cameras 3 degrees / 3 % of their distance off (0.0353 / 0.0337 / 0.0319),
# object 1's Tow 3 degrees / 3 % of its box diagonal off, object 0 at its true pose but free; seeds 1 / 2 / 3.  Measured on an MI355X (degrees / scene units):
#   8-level grid, plain      loss 0.451-0.606 -> joint 0.0130 / 0.0054 / 0.0090, cameras only (object 1 left off) 0.0220 / 0.0211 / 0.0321
#     cameras, joint:        2.727/0.0270 1.178/0.0161 1.837/0.0174 | 0.317/0.0107 0.741/0.0105 0.690/0.0030 | 0.476/0.0049 0.466/0.0026 1.416/0.0143
#     cameras only:          2.525/0.0261 0.908/0.0136 1.392/0.0157 | 1.001/0.0153 0.983/0.0129 0.385/0.0044 | 0.817/0.0095 0.901/0.0093 1.301/0.0145
#     per frame, true map:   2.323/0.0223 0.511/0.0048 1.198/0.0139 | 0.226/0.0022 0.229/0.0037 0.410/0.0049 | 0.674/0.0066 0.114/0.0020 1.281/0.0150
#     object 1, joint:       3.000/0.0116 -> 1.043/0.0081 | 3.000/0.0086 -> 1.613/0.0155 | 3.000/0.0247 -> 1.230/0.0097;  object 0 drifts to 1.641/0.0052 |
#                            0.711/0.0052 | 1.432/0.0114
#   base.json, default c2f   loss 0.448-0.607 -> joint 0.0105 / 0.0093 / 0.0141, cameras only 0.0250 / 0.0212 / 0.0235
#     cameras, joint:        2.590/0.0245 1.351/0.0136 2.030/0.0178 | 0.327/0.0110 0.461/0.0113 0.981/0.0051 | 0.493/0.0064 0.512/0.0021 1.352/0.0153
#     cameras only:          2.242/0.0253 0.999/0.0117 1.391/0.0156 | 0.998/0.0152 0.804/0.0116 0.741/0.0076 | 1.031/0.0120 0.939/0.0098 1.277/0.0148
#     per frame, true map:   2.358/0.0196 0.859/0.0049 1.220/0.0142 | 0.115/0.0018 0.070/0.0015 0.361/0.0042 | 0.385/0.0042 0.077/0.0017 1.285/0.0146
#     object 1, joint:       -> 1.450/0.0128 | 1.069/0.0146 | 1.371/0.0113;  object 0 drifts to 1.515/0.0023 | 0.590/0.0056 | 1.498/0.0125
# ("per frame, true map": mon_scene_refine_camera of each frame with the objects at their stored, true poses -- what the cameras reach when the map is right.
# Per-frame refinement with object 1 left off is the cameras-only window call bit for bit: asserted in the test on a checkpoint twin that holds the pose.)
# Joint refinement ends at a loss 2-4x below cameras-only in every run and brings object 1's rotation from 3 degrees to 1.0-1.6, but it does NOT end closer
# than the baselines in the cameras (closer in 10 of 18 camera figures of the 8-level runs, worse in every figure of seed 1) and object 0, which started
# true, drifts 0.6-1.6 degrees: one anchor frame ties two small objects to the world only weakly (3.4f's turn-against-shift ambiguity, now per object as
# well), so cameras and objects can move together at nearly no cost in the loss.  Hence only the loss is barred: every trace ends below
# its start (asserted in advance), and the joint run's ending loss stays within 2x the worst seed measured (REFINE_BARS' rule).
REFINE_LOSS_MEASURED = dict(coarse=0.01303, base_c2f=0.01408)
REFINE_LOSS_BARS = {k: 2 * v for k, v in REFINE_LOSS_MEASURED.items()}


@pytest.mark.parametrize("tag", ["coarse", "base_c2f"])
def test_window_refinement_run(pkg, ss, scene, trained, tmp_path, tag):
    """views 20-23, {c0, c1} plain and {a0, a1} with the default c2f: the joint run next to cameras-only window refinement with object 1 left at its
    perturbed pose and per-frame mon_scene_refine_camera; everything finite, every trace ends below its start, the joint run's ending loss within
    REFINE_LOSS_BARS; the ending camera and object errors are printed (the comment above).  The like-for-like per-frame baseline -- mon_scene_refine_camera
    of each frame against a checkpoint twin of object 1 that holds the perturbed pose -- equals the cameras-only window run bit for bit (asserted)."""
    sc = scene; ds, o = trained
    pair, c2f = ([o["c0"], o["c1"]], None) if tag == "coarse" else ([o["a0"], o["a1"]], True)
    path = str(tmp_path / "obj1.ckpt"); pair[1].save(path); twin = pkg.ObjectNeRF.load(ds, path)
    views = (20, 21, 22, 23); prm = pkg.pose_refine_default()
    boxes = [_view_boxes(sc, v, (0, 1)) for v in views]; obs = np.concatenate(boxes)
    Tow_true = [sc.objects[k]["Tow"] for k in (0, 1)]
    for seed in (1, 2, 3):
        Tc0 = [sc.Twc[views[0]]] + [_perturb_camera(sc.Twc[v], 3.0, 0.03 * _cam_dist(sc, v), 10 * seed + f) for f, v in enumerate(views[1:])]
        To0 = [Tow_true[0], _perturb_object(Tow_true[1], 3.0, 0.03 * _diag(sc, 1), 50 + seed)]
        Twc0 = np.stack([ss.colmajor(T) for T in Tc0]); Tow0 = np.stack([ss.colmajor(T) for T in To0])
        Twc, Tow, trace, _ = pkg.scene_refine_window(pair, obs, Twc0, Tow0, prm, c2f=c2f, window=pkg.window_default())
        TwcC, _, traceC, ftraceC = pkg.scene_refine_window(pair, obs, Twc0, Tow0, prm, c2f=c2f, window=dict(n_fixed_frames=1, refine_objects=0))
        assert np.isfinite(Twc).all() and np.isfinite(Tow).all() and np.isfinite(trace).all() and np.isfinite(TwcC).all() and np.isfinite(traceC).all()
        assert np.array_equal(_bits(Twc[0]), _bits(Twc0[0]))
        assert trace[-1] < trace[0], (tag, seed, trace[[0, -1]])
        assert traceC[-1] < traceC[0], (tag, seed, traceC[[0, -1]])
        assert trace[-1] <= REFINE_LOSS_BARS[tag], (tag, seed, trace[-1], REFINE_LOSS_BARS[tag])
        cam0 = [_pose_errors(Tc0[f], sc.Twc[v]) for f, v in enumerate(views)][1:]
        camJ = [_pose_errors(_mat(Twc[f]), sc.Twc[v]) for f, v in enumerate(views)][1:]
        camC = [_pose_errors(_mat(TwcC[f]), sc.Twc[v]) for f, v in enumerate(views)][1:]
        camS = []
        for f, v in list(enumerate(views))[1:]:                               # per-frame mon_scene_refine_camera, the objects as they are stored
            pose, _ = pkg.scene_refine_camera(pair, boxes[f], Twc0[f], prm, c2f=c2f)
            camS.append(_pose_errors(_mat(pose), sc.Twc[v]))
        twin.set_pose(Tow0[1])
        for f in range(1, len(views)):                                        # ... and with object 1 as perturbed as the window call sees it
            pose, tr = pkg.scene_refine_camera([pair[0], twin], boxes[f], Twc0[f], prm, c2f=c2f)
            assert np.array_equal(_bits(pose), _bits(TwcC[f])) and np.array_equal(_bits(tr), _bits(ftraceC[:, f])), (tag, seed, f)
        ob0 = _pose_errors(To0[1], Tow_true[1]); obJ = _pose_errors(_mat(Tow[1]), Tow_true[1]); obJ0 = _pose_errors(_mat(Tow[0]), Tow_true[0])
        fmt = lambda e: " ".join("%.3f/%.4f" % q for q in e)                  # noqa: E731
        print("%s seed %d: loss %.5f -> joint %.5f, cameras only %.5f" % (tag, seed, trace[0], trace[-1], traceC[-1]))
        print("  cameras (deg/units) start %s | joint %s | cameras only %s | per frame, true objects %s" % (fmt(cam0), fmt(camJ), fmt(camC), fmt(camS)))
        print("  object 1 start %.3f/%.4f -> joint %.3f/%.4f; object 0 (started true) -> %.3f/%.4f" % (*ob0, *obJ, *obJ0))
    twin.close()


# ------------------------------------------------------------------ 7. read-only
def _stats_tuple(s):
    return tuple(sorted(s.items()))


@pytest.mark.parametrize("side", [0, 1])
def test_window_calls_are_read_only(pkg, ss, scene, trained, side):
    """around a window loss and a joint refinement on each side, for every object: parameter CRCs (all three copies), mon_object_info, render-skip
    statistics, the snapshot step, a following mon_object_pose_loss at the object's own Tow bit for bit, and the dataset's poses through a single-frame
    loss; the refinement repeated returns the same bits"""
    sc = scene; _, objs = trained; pair = [objs["c0"], objs["c1"]]
    views = (22, 23); boxes = [_view_boxes(sc, v, (0, 1)) for v in views]; obs = np.concatenate(boxes)
    prm = pkg.pose_refine_default(iters=6, rays_per_iter=512); p1 = pkg.pose_refine_default(rays_per_iter=256)

    def snap():
        out = []
        for k, o in enumerate(pair):
            i = o.info()
            out.append((tuple(zlib.crc32(o.get_params(c).tobytes()) for c in range(3)), tuple(getattr(i, f) for f, _ in type(i)._fields_),
                        _stats_tuple(o.render_skip_stats(0)), _stats_tuple(o.render_skip_stats(1)),
                        int(o.render_snapshot(boxes[1][k], ss.colmajor(sc.Twc[VIEW]))[-1])))
        return out

    def losses():
        return [o.pose_loss(boxes[1][k:k + 1], ss.colmajor(sc.objects[k]["Tow"]), p1, iteration=3) for k, o in enumerate(pair)]

    def renders():                                                          # (a render uses the object's own Tow)
        return [zlib.crc32(o.render(boxes[1][k], ss.colmajor(sc.Twc[VIEW]))[0].tobytes()) for k, o in enumerate(pair)]

    r_before = renders(); l_before = losses(); before = snap()
    Twc0 = np.stack([ss.colmajor(sc.Twc[22]), ss.colmajor(_perturb_camera(sc.Twc[23], 2.0, 0.02, 5))])
    Tow0 = np.stack([ss.colmajor(sc.objects[0]["Tow"]), ss.colmajor(_perturb_object(sc.objects[1]["Tow"], 2.0, 0.01, 6))])
    pkg.scene_window_loss(pair, obs, Twc0, Tow0, prm, side=side, iteration=2)
    a = pkg.scene_refine_window(pair, obs, Twc0, Tow0, prm, c2f=True, window=pkg.window_default(), side=side)
    b = pkg.scene_refine_window(pair, obs, Twc0, Tow0, prm, c2f=True, window=pkg.window_default(), side=side)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(_bits(a[1][1]), _bits(Tow0[1])) and not np.array_equal(_bits(a[0][1]), _bits(Twc0[1]))
    assert before == snap()
    for (la, ga), (lb, gb) in zip(l_before, losses()):
        assert la == lb and np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    assert r_before == renders()


# ------------------------------------------------------------------ 8. status codes
def test_window_errors(pkg, ss, scene, trained):
    """MON_ERR_ARG rows that need objects: what the single-frame call rejects per frame (a frame the dataset does not hold, a box outside the frame, side 2,
    iters < 0, bad level weights and schedules, objects on two datasets), more than 16384 rays in one frame drawn or every-pixel, n_fixed_frames above F,
    refine_objects without an anchor or without Tow16s, bad object step sizes; MON_ERR_STATE for a layer-kernel shape, the XORWOW mode and side 1
    unpublished.  Each leaves the poses as given."""
    sc = scene; ds, objs = trained; pair = [objs["a0"], objs["a1"]]
    frames = [(_view_boxes(sc, v, (0, 1)), ss.colmajor(sc.Twc[v])) for v in (22, 23)]
    obs, Twc = _window(frames); prm = pkg.pose_refine_default(iters=2, rays_per_iter=256)
    own = np.stack([ss.colmajor(sc.objects[k]["Tow"]) for k in (0, 1)])

    def code(fn):
        with pytest.raises(pkg.MonError) as e:
            fn()
        return e.value.code
    absent = obs.copy(); absent[2:, 0] = 200
    outside = obs.copy(); outside[3] = (23, sc.W - 10, 0, 8, 16)
    split = obs[[0, 2, 1, 3]]                                                 # frame 22, 23, 22, 23
    for b in (absent, outside, split):
        assert code(lambda: pkg.scene_window_loss(pair, b, Twc, None, prm)) == 1
        assert code(lambda: pkg.scene_refine_window(pair, b, Twc, own, prm)) == 1
    assert code(lambda: pkg.scene_window_loss(pair, obs, Twc, None, prm, side=2)) == 1
    assert code(lambda: pkg.scene_refine_window(pair, obs, Twc, own, pkg.pose_refine_default(iters=-1))) == 1
    assert code(lambda: pkg.scene_window_loss(pair, obs, Twc, None, pkg.pose_refine_default(rays_per_iter=16385))) == 1
    wide = np.array([[22, 150, 60, 128, 128], [23, 150, 60, 129, 128]], np.uint32)
    assert code(lambda: pkg.scene_window_loss(pair, wide, Twc, None, pkg.pose_refine_default(rays_per_iter=0))) == 1
    assert code(lambda: pkg.scene_window_loss(pair, obs, Twc, None, prm, level_weights=-np.ones(16, np.float32))) == 1
    assert code(lambda: pkg.scene_refine_window(pair, obs, Twc, own, prm, c2f=dict(ramp=0.0))) == 1
    for w in (dict(n_fixed_frames=3), dict(n_fixed_frames=0), dict(lr_obj_trans=-1.0), dict(lr_obj_rot=float("nan"))):
        assert code(lambda: pkg.scene_refine_window(pair, obs, Twc, own, prm, window=w)) == 1, w
    assert code(lambda: pkg.scene_refine_window(pair, obs, Twc, None, prm)) == 1              # refine_objects without Tow16s
    bad = own.copy(); bad[1, 13] = np.nan
    assert code(lambda: pkg.scene_window_loss(pair, obs, Twc, bad, prm)) == 1
    assert code(lambda: pkg.scene_refine_window(pair, obs, Twc, bad, prm)) == 1
    ds2, other = ge.make_problem(pkg, sc, BASE, use_depth=True, obj_index=1)
    _, c = ge.make_problem(pkg, sc, dict(n_neurons=16), dataset=ds)
    _, x = ge.make_problem(pkg, sc, dict(BASE, rng_flags=1), dataset=ds)
    _, fresh = ge.make_problem(pkg, sc, BASE, obj_index=1, dataset=ds)
    try:
        assert code(lambda: pkg.scene_window_loss([objs["a0"], other], obs, Twc, None, prm)) == 1            # another dataset
        for lst, side in (([c], 0), ([objs["a0"], c], 0), ([x], 0), ([fresh], 1), ([objs["a0"], fresh], 1)):
            assert code(lambda: pkg.scene_window_loss(lst, obs, Twc, None, prm, side=side)) == 5, (len(lst), side)
            assert code(lambda: pkg.scene_refine_window(lst, obs, Twc, None, prm, window=dict(refine_objects=0), side=side)) == 5, (len(lst), side)
    finally:
        for q in (c, x, fresh, other, ds2):
            q.close()


# ------------------------------------------------------------------ 9. mon_object_set_pose
def _crcs(o):
    return tuple(zlib.crc32(o.get_params(c).tobytes()) for c in range(3))


@pytest.mark.parametrize("use_graph", [0, 1])
def test_set_pose_of_the_own_pose_leaves_training_as_it_was(pkg, ss, scene, trained, tmp_path, use_graph):
    """an object trained 40 steps and its checkpoint twin; mon_object_set_pose(its own Tow) on one of them, 20 more steps on both: parameters, info and loss
    bit for bit -- on the fused chain with its prepared candidates, and with use_graph = 1 (the captured graph is dropped and captured again)"""
    sc = scene; ds, _ = trained
    pkg.set_option("use_graph", use_graph)
    try:
        a = _object(pkg, ss, ds, sc, 1, COARSE, steps=40)
        path = str(tmp_path / "a.ckpt"); a.save(path)
        b = pkg.ObjectNeRF.load(ds, path)
        a.train(10); b.train(10)
        assert _crcs(a) == _crcs(b)
        a.set_pose(ss.colmajor(sc.objects[1]["Tow"]))
        la, lb = a.train(20), b.train(20)
        ia, ib = a.info(), b.info()
        assert la == lb and _crcs(a) == _crcs(b)
        assert tuple(getattr(ia, f) for f, _ in type(ia)._fields_) == tuple(getattr(ib, f) for f, _ in type(ib)._fields_)
        a.close(); b.close()
    finally:
        pkg.set_option("use_graph", 0)


def test_set_pose_is_what_renders_and_checkpoints_see(pkg, ss, scene, trained, tmp_path):
    """after set_pose(T'): mon_object_save stores T' (mon_checkpoint_read_info), and mon_object_render equals, bit for bit, the render of a checkpoint twin
    loaded from that file; the render differs from the one before; NULL and non-finite matrices are MON_ERR_ARG, a call between the stages of an iteration
    MON_ERR_STATE, and each leaves the pose as it was"""
    sc = scene; ds, _ = trained
    o = _object(pkg, ss, ds, sc, 1, NARROW, steps=100)
    box = _view_boxes(sc, VIEW, (1,))[0]; Twc16 = ss.colmajor(sc.Twc[VIEW])
    r0 = o.render(box, Twc16)
    Tp = ss.colmajor(_perturb_object(sc.objects[1]["Tow"], 4.0, 0.05 * _diag(sc, 1), 9))
    o.set_pose(Tp)
    r1 = o.render(box, Twc16)
    assert not np.array_equal(r0[0], r1[0])
    path = str(tmp_path / "moved.ckpt"); o.save(path)
    info = pkg.checkpoint_info(path)
    assert np.array_equal(_bits(np.array(list(info.Tow), np.float32)), _bits(Tp))
    t = pkg.ObjectNeRF.load(ds, path)
    r2 = t.render(box, Twc16)
    for x, y in zip(r1, r2):
        assert np.array_equal(_bits(x), _bits(y))
    L = pkg.lib(); bad = Tp.copy(); bad[13] = np.nan
    assert L.mon_object_set_pose(o.h, None) == 1
    assert L.mon_object_set_pose(o.h, bad.ctypes.data) == 1
    o.train_stages(1 | 2)
    assert L.mon_object_set_pose(o.h, Tp.ctypes.data) == 5
    o.train_stages(4)
    o.set_pose(Tp)                                                          # (a whole step later the call is accepted again)
    o.close(); t.close()


# ------------------------------------------------------------------ 10. the online path while the manager trains
def test_online_refine_window_while_training(pkg, ss, scene):
    """mon_online_refine_window with a NULL obs / Twc16s / p / w, no boxes, iters < 0, bad window parameters, split frames and a wrong object count
    (MON_ERR_ARG) and before anything is published (MON_ERR_STATE), then from a second thread while the manager's two objects train: MON_OK, finite
    poses and a trace that ends below its start, `included` marks both objects; mon_online_set_object_pose stores a refined pose while training goes on; the
    dataset's poses are what they were and the objects finish their training"""
    sc = scene
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    views = (22, 23); obs = np.concatenate([_view_boxes(sc, v, (0, 1)) for v in views]); prm = pkg.pose_refine_default(iters=20, rays_per_iter=1024)
    Twc0 = np.stack([ss.colmajor(sc.Twc[22]), ss.colmajor(_perturb_camera(sc.Twc[23], 2.0, 0.02, 6))])
    Tow0 = np.stack([ss.colmajor(sc.objects[0]["Tow"]), ss.colmajor(_perturb_object(sc.objects[1]["Tow"], 2.0, 0.01, 7))])
    for v in range(sc.n_views):
        m.new_frame(v, "%.6f" % (v * 0.1), sc.rgb[v][..., ::-1], sc.instance[v], ss.colmajor(sc.Twc[v]))
    ids = [m.create_nerf(sc.objects[k]["cls"], ss.colmajor(sc.objects[k]["Tow"]), -sc.objects[k]["half"] / 1.1, sc.objects[k]["half"] / 1.1) for k in range(2)]
    with pytest.raises(pkg.MonError) as e:
        m.refine_window(obs, Twc0, Tow0, prm)               # objects, nothing published
    assert e.value.code == 5
    with pytest.raises(pkg.MonError) as e:
        m.refine_window(obs, Twc0, Tow0[:1], prm)           # one row for two manager objects
    assert e.value.code == 1
    L = pkg.lib(); wp = pkg.window_default(); tr = np.full(prm.iters + 1, 7.0, np.float32); inc = np.full(2, 7, np.uint8)

    def rc(obs_=obs, poses=Twc0, p=prm, w=wp, n_obs=None, n=2):
        return L.mon_online_refine_window(m.h, None if obs_ is None else obs_.ctypes.data, obs.shape[0] if n_obs is None else n_obs,
                                          None if p is None else C.byref(p), None, None if w is None else C.byref(w),
                                          None if poses is None else poses.ctypes.data, Tow0.ctypes.data, n, inc.ctypes.data, tr.ctypes.data, None)
    for kw in (dict(obs_=None), dict(poses=None), dict(p=None), dict(w=None), dict(n_obs=0), dict(p=pkg.pose_refine_default(iters=-1)),
               dict(w=pkg.window_default(n_fixed_frames=3)), dict(w=pkg.window_default(n_fixed_frames=0)), dict(obs_=obs[[0, 2, 1, 3]]), dict(n=3)):
        assert rc(**kw) == 1, kw                                            # MON_ERR_ARG before the objects are looked at
    assert rc() == 5 and (tr == 7.0).all() and (inc == 7).all()              # nothing published
    poses_before = [m.get_pose(v).copy() for v in views]
    published = threading.Event(); res = dict(err=None, out=None, calls=None)

    def backend():
        try:
            published.wait(timeout=120)
            res["out"] = m.refine_window(obs, Twc0, Tow0, prm, c2f=True)
            res["calls"] = [m.object_info(i)["train_calls"] for i in ids]
            m.set_object_pose(ids[1], res["out"][1][1])
            m.set_object_pose(ids[1], ss.colmajor(sc.objects[1]["Tow"]))      # ... and the true pose back, for the rest of the training
        except Exception as ex:        # noqa: BLE001 -- reported by the main thread
            res["err"] = ex

    th = threading.Thread(target=backend); th.start()
    try:
        for k in range(2):
            m.update_nerf_bbox(ids[k], sc.objects[k]["boxes"], 200)
        import time
        t0 = time.time()
        while not all(m.object_info(i)["train_calls"] >= 1 for i in ids) and time.time() - t0 < 90:
            time.sleep(0.02)
    finally:
        published.set(); th.join(timeout=120)
    m.wait_threads_end()
    assert res["err"] is None and res["out"] is not None, res
    Twc, Tow, inc, trace, ftrace = res["out"]
    done = [m.object_info(i)["train_calls"] for i in ids]
    print("online: trace %.5f -> %.5f, train calls at the call %s, at the end %s" % (trace[0], trace[-1], res["calls"], done))
    assert np.isfinite(Twc).all() and np.isfinite(Tow).all() and np.isfinite(trace).all() and np.isfinite(ftrace).all() and trace[-1] < trace[0]
    assert inc.tolist() == [1, 1]
    assert np.array_equal(_bits(Twc[0]), _bits(Twc0[0])) and not np.array_equal(_bits(Tow[1]), _bits(Tow0[1]))
    assert all(d >= 200 for d in done) and all(np.isfinite(m.object_info(i)["loss"]) for i in ids)       # training went on to its end
    for v, p in zip(views, poses_before):
        assert np.array_equal(m.get_pose(v).view(np.uint32), p.view(np.uint32))
    m.close()
