"""GPU tests (-m gpu) of camera pose refinement against a scene of object NeRFs (mon_scene_pose_loss, mon_scene_refine_camera, mon_online_refine_camera;
kernels k_scene_pose_rays, k_scene_pose_obj, k_scene_composite_grad, k_scene_pose_update in kernels_scene_pose.hip).  The contract is include/mon_core.h's
and DESIGN.md 3.4f's: the composite's loss and backward equal an fp64 restatement, the whole chain equals one fp64 autograd graph of the objective at the
bars of tests/test_pose_shapes.py, one object reduces to mon_object_pose_loss, refinement pulls a perturbed camera back, and nothing about the objects, the
dataset or a manager changes."""
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
# the bars of this arithmetic chain (tests/test_pose_shapes.py)
POS_TOL, LOSS_RTOL, G6_RTOL, DLDX_TOL, DLDX_FRAC, DLDX_FLOOR = 1e-5, 1e-4, 1e-2, 2e-2, 0.999, 0.01
# k_scene_composite_grad against fp64 on the adversarial lists of test 1: fp32 end to end, no bar in the tree before.  Measured on an MI355X, the largest
# error over l, W, D, dL/dalpha and dL/dc, relative to the case's largest magnitude of that quantity: 5.5e-7 (K = 1), 5.4e-7 (K = 2), 6.4e-7 (K = 3),
# 6.8e-7 (K = 8).  The bar is 4x the largest of them, for the changed summation order on other seeds.
COMP_GRAD_MEASURED, COMP_GRAD_BAR = 6.9e-7, 2.8e-6
# Ending errors of the refinement runs of test 5 (degrees, scene units), measured on an MI355X from 3 degrees / 0.0319 off, seeds 1 / 2 / 3:
#   8-level grid, plain:   1.625 / 0.344 / 1.908 degrees, 0.0190 / 0.0044 / 0.0236      (loss 0.11-0.14 -> 0.0007-0.0037)
#   base.json, c2f:        1.638 / 0.256 / 2.002 degrees, 0.0187 / 0.0036 / 0.0236      (loss 0.11-0.14 -> 0.0017-0.0031)
#   base.json, plain:      6.06 / 7.69 / 6.04 degrees, 0.094 / 0.070 / 0.021: drifts away (reported, not barred)
# The bars are 2x the worst seed (no tighter than Adam's step at the default lr_rot, 0.23 degrees, and lr_trans, 2e-3).  The loss falls by two orders of
# magnitude while the pose error falls by less: two small neighbouring objects leave a turn about the camera centre and a sideways shift nearly
# indistinguishable, and no lr_trans / lr_rot of the sweep (tools/scene_track_timing.py --sweep) ends closer than the defaults.
ADAM_ROT_DEG, ADAM_TRANS = 0.23, 2e-3
REFINE_MEASURED = dict(coarse=(1.908, 0.0236), base_c2f=(2.002, 0.0236))
REFINE_BARS = {k: (max(2 * v[0], ADAM_ROT_DEG), max(2 * v[1], ADAM_TRANS)) for k, v in REFINE_MEASURED.items()}


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
    """Objects of the scene-render tests' scene, 300 iterations each with depth: object 0 on a box inflated 5x (base.json), object 1 on its true box as a
    32 x 2 network, objects 0 and 1 on their true boxes on base.json and on an 8-level grid of per-level scale 1.5."""
    sc = scene
    ds, b0 = ge.make_problem(pkg, sc, BASE, use_depth=True, obj_index=0)
    b0.close()
    objs = dict(b0=_object(pkg, ss, ds, sc, 0, BASE, inflate=5.0), n1=_object(pkg, ss, ds, sc, 1, NARROW),
                a0=_object(pkg, ss, ds, sc, 0, BASE), a1=_object(pkg, ss, ds, sc, 1, BASE),
                c0=_object(pkg, ss, ds, sc, 0, COARSE), c1=_object(pkg, ss, ds, sc, 1, COARSE))
    infl = dict(b0=5.0)
    yield ds, objs, infl
    for o in objs.values():
        o.close()
    ds.close()


VIEW = 23                                                   # the view with the largest silhouette overlap of the scene (object 0 in front of object 1)


def _meta(sc, k, o, inflate=1.0):
    ob = sc.objects[k]
    return dict(Tow=ob["Tow"], aabb=np.stack([-ob["half"] * inflate, ob["half"] * inflate]).astype(np.float32), cls=ob["cls"], sample_seed=o.cfg.sample_seed)


def _pair(sc, objs, order):
    """the whole-chain pair {object 0 on the inflated box, object 1 narrow} in the given order: (objects, their metadata)"""
    both = [(objs["b0"], _meta(sc, 0, objs["b0"], 5.0)), (objs["n1"], _meta(sc, 1, objs["n1"]))]
    both = [both[i] for i in order]
    return [b[0] for b in both], [b[1] for b in both]


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


def _perturb_camera(Twc, rot_deg, trans, seed):
    """Twc D with a random rotation axis and translation direction: the camera turned by rot_deg about its own centre and moved by `trans`"""
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    D = np.eye(4); D[:3, :3] = _so3(ax * math.radians(rot_deg)); D[:3, 3] = d * trans
    return Twc @ D


def _camera_errors(T, T_true):
    R = T[:3, :3].T @ T_true[:3, :3]
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def _mat(T16):
    return np.asarray(T16, np.float64).reshape(4, 4).T


def _cam_dist(sc, v):
    """distance of the camera of view v from the centre of the scene's objects"""
    c = np.mean([-ob["Tow"][:3, :3].T @ ob["Tow"][:3, 3] for ob in sc.objects[:2]], 0)
    return float(np.linalg.norm(sc.Twc[v][:3, 3] - c))


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------ 1. the composite-grad kernel alone
def _adversarial(rng, K, R, equal_t, alpha_hi, wall=False):
    """lists in the style of test_scene_render._adversarial, with counts from {0, 32, 64}, a ray with no list at all, a list wholly behind the cut, and
    targets: m* of the front, the back and no list, d* = 0 and d* > 0 on both Huber branches"""
    count = rng.choice(np.array([0, 32, 64], np.uint32), size=(K, R), p=[0.2, 0.3, 0.5]).astype(np.uint32)
    count[:, 0] = 0                                                       # a ray with every count 0
    if equal_t:
        t = np.sort(rng.randint(0, 40, size=(K, R, 64)) * 0.05 + 1.0, -1).astype(np.float32)
    else:
        t = np.sort(rng.uniform(0.5, 3.0, size=(K, R, 64)), -1).astype(np.float32)
    alpha = rng.uniform(0.0, alpha_hi, size=(K, R, 64)).astype(np.float32)
    alpha[rng.rand(K, R) < 0.1] = 0.0
    if wall:                                                              # six nearly opaque samples somewhere in one list of most rays: the cut falls there
        for r in range(9, R):
            live = np.nonzero(count[:, r] > 0)[0]
            if live.size and rng.rand() < 0.8:
                kw = live[rng.randint(live.size)]; sw = rng.randint(0, int(count[kw, r]) - 5)
                alpha[kw, r, sw:sw + 6] = rng.uniform(0.8, 0.95, 6).astype(np.float32)
    if K > 1:                                                             # a list lying wholly behind an opaque one: rays 1..8
        for r in range(1, 9):
            count[0, r] = 64; count[K - 1, r] = 64
            t[K - 1, r] = np.sort(rng.uniform(5.0, 6.0, 64)).astype(np.float32); alpha[0, r] = np.float32(0.5)
    rgb = rng.uniform(0.0, 1.0, size=(K, R, 64, 3)).astype(np.float32)
    dn = rng.uniform(1.0, 1.3, size=R).astype(np.float32)
    cstar = rng.uniform(0.0, 1.0, size=(R, 3)).astype(np.float32)
    tf = np.where(count > 0, t[..., 0], np.inf); tl = np.where(count > 0, np.take_along_axis(t, np.maximum(count.astype(np.int64) - 1, 0)[..., None], 2)[..., 0], -np.inf)
    mstar = np.zeros((K, R), np.float32); sel = rng.randint(0, 3, size=R)          # 0: the front list, 1: the back list, 2: none
    front, back = np.argmin(tf, 0), np.argmax(tl, 0)
    mstar[front[sel == 0], np.nonzero(sel == 0)[0]] = 1.0; mstar[back[sel == 1], np.nonzero(sel == 1)[0]] = 1.0
    dsel = rng.randint(0, 3, size=R)                                      # 0: no depth, 1: near the composite's depth (quadratic), 2: far off (linear)
    D = sref.np_composite_grad(t, alpha, rgb, count, cstar, mstar, np.zeros(R), dn, (1.0, 1.0, 0.0, 0.05))["D"]      # (D does not depend on d*)
    near = np.maximum(D + rng.uniform(-0.04, 0.04, R), 1e-3)
    dstar = np.where(dsel == 0, 0.0, np.where(dsel == 1, near, D + rng.uniform(1.0, 3.0, R))).astype(np.float32)
    return t, alpha, rgb, count, cstar, mstar, dstar, dn


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_composite_grad_kernel_on_adversarial_lists(pkg, K):
    """mon_debug_scene_composite_grad on R = 256 rays of random lists, interleaved or with equal t inside and across lists: alpha up to 0.6 (the cut falls
    inside the first block), alpha up to 0.01 with six nearly opaque samples at a random place of one list (the cut falls in any block, a middle and the last
    one of a ray's merged samples included) and alpha up to 0.02 (no cut: every block reached), against the fp64 restatement: l, W_j, D and every dL/dalpha
    and dL/dc.  Rays whose stopping point lies within 0.1 % of 1e-4 are left out (<= 1 % of the rays, asserted)."""
    w = (1.0, 1.0, 1.0, 0.05); R = 256; worst = 0.0; cuts = set()
    for equal_t in (False, True):
        for alpha_hi, wall in ((0.6, False), (0.01, True), (0.02, False)):
            rng = np.random.RandomState(4300 + 10 * K + int(equal_t) + int(1000 * alpha_hi))          # (seeds on which at most one ray per case is ambiguous)
            t, alpha, rgb, count, cstar, mstar, dstar, dn = _adversarial(rng, K, R, equal_t, alpha_hi, wall)
            got = pkg.scene_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, *w)
            ref = sref.np_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, w)
            ok = ~ref["amb"]
            assert (~ok).sum() <= R // 100, (~ok).sum()
            cut_in = ref["ncut"] < ref["ntot"]
            blk, last = ref["ncut"][cut_in] // 64, (ref["ntot"][cut_in] - 1) // 64
            cuts |= ({"first"} if (blk == 0).any() else set()) | ({"middle"} if ((blk > 0) & (blk < last)).any() else set()) | \
                    ({"last"} if ((blk > 0) & (blk == last)).any() else set())
            hub = np.abs(ref["D"] - dstar)[(mstar.max(0) > 0) & (dstar > 0)]
            assert (hub <= w[3]).any(), "no ray on the quadratic Huber branch"
            assert (hub > w[3]).any(), "no ray on the linear Huber branch"
            errs = dict(l=_rel(got["l"][ok], ref["l"][ok]), W=_rel(got["W"][:, ok], ref["W"][:, ok]), D=_rel(got["D"][ok], ref["D"][ok]),
                        dalpha=_rel(got["dalpha"][:, ok], ref["dalpha"][:, ok]), dc=_rel(got["dc"][:, ok], ref["dc"][:, ok]))
            print("K %d equal_t %d alpha_hi %.2f: %s, cut inside the lists on %d rays" % (K, equal_t, alpha_hi, {k: "%.2e" % v for k, v in errs.items()},
                  int(cut_in.sum())))
            assert (got["dalpha"][:, 0] == 0).all() and (got["W"][:, 0] == 0).all() and got["D"][0] == 0          # the ray with no list
            worst = max(worst, max(errs.values()))
    if K == 8:
        assert cuts == {"first", "middle", "last"}, cuts                      # the cut fell inside the first, a middle and the last block of a ray
    print("K %d: largest relative error %.3e (bar %.1e)" % (K, worst, COMP_GRAD_BAR))
    assert worst <= COMP_GRAD_BAR


# ------------------------------------------------------------------ 2. the whole chain against fp64 autograd
def _dump_all(pkg, objs, boxes, Twc16, prm, side=0, iteration=0, lw=None):
    return [pkg.scene_pose_samples(objs, boxes, Twc16, k, prm, side=side, iteration=iteration, level_weights=lw) for k in range(len(objs))]


def _groups(rs, dumps, ref_amb):
    """ray groups of a case by the restatement (rs) and the device's counts"""
    hit = np.stack([o["hit"] for o in rs["objs"]]); n_hit = hit.sum(0)
    t0 = np.stack([o["t0"] for o in rs["objs"]]); t1 = np.stack([o["t1"] for o in rs["objs"]])
    inter = (n_hit == 2) & (np.maximum(t0[0], t0[1]) < np.minimum(t1[0], t1[1]))
    return dict(miss=n_hit == 0, one=n_hit == 1, interleaved=inter)


def _chain_case(pkg, orc, ss, sc, objs, metas, boxes, Twc, prm, tmp_path, tag, side=0, iteration=0, lw=None):
    Twc16 = ss.colmajor(Twc)
    n_rays = int(prm.rays_per_iter)
    rs = sref.scene_rays(sc, boxes, _mat(Twc16), metas, n_rays=n_rays, seed=prm.seed, iteration=iteration)
    dumps = _dump_all(pkg, objs, boxes, Twc16, prm, side, iteration, lw)
    loss, g6 = pkg.scene_pose_loss(objs, boxes, Twc16, prm, side=side, iteration=iteration, level_weights=lw)
    K = len(objs); P = rs["x"].size
    # positions equal the restatement (the 1e-5 bar of test_pose_shapes, box units)
    for j in range(K):
        h = rs["objs"][j]["hit"]; ext = float(np.linalg.norm(metas[j]["aabb"][1] - metas[j]["aabb"][0]))
        assert np.array_equal(dumps[j]["count"] > 0, h), (tag, j)
        assert np.abs(dumps[j]["x_o"][h] - rs["objs"][j]["x_o"][h]).max() <= POS_TOL * ext, (tag, j)
        assert np.abs(dumps[j]["t"][h] - rs["objs"][j]["t"][h]).max() <= POS_TOL * ext
        assert np.abs(dumps[j]["x_c"][h] - dumps[j]["t"][h][..., None] * rs["uc"][h][:, None, :]).max() <= POS_TOL * ext
    nets = [dict(pref.net_inputs(o, orc, prm), aabb=m["aabb"]) for o, m in zip(objs, metas)]
    Toc = np.stack([np.asarray(m["Tow"], np.float64) @ _mat(Twc16) for m in metas])
    case = dict(x_o=np.stack([d["x_o"] for d in dumps]), x_c=np.stack([d["x_c"] for d in dumps]), t=np.stack([d["t"] for d in dumps]),
                count=np.stack([d["count"] for d in dumps]), dn=rs["dn"], cstar=rs["cstar"], mstar=np.stack([o["mstar"] for o in rs["objs"]]),
                dstar=rs["dstar"], Toc=Toc, lw=lw)
    ref = sref.reference(tmp_path, nets, [case], (prm.w_rgb, prm.w_mask, prm.w_depth, prm.depth_huber), tag=tag)[0]
    amb = ref["amb"]
    assert amb.sum() <= P // 100, (tag, int(amb.sum()))
    return rs, dumps, loss, g6, ref, case


def _check_chain(tag, rs, dumps, loss, g6, ref, P):
    ok = ~ref["amb"]
    l_ref = ref["l"].mean() if ok.all() else None
    if l_ref is not None:
        print("%s: loss %.6f (fp64 %.6f, rel %.2e)  grad6 rel %.2e" % (tag, loss, ref["loss"], abs(loss - ref["loss"]) / abs(ref["loss"]),
              np.abs(g6 - ref["g6"]).max() / np.abs(ref["g6"]).max()))
        assert abs(loss - ref["loss"]) <= LOSS_RTOL * abs(ref["loss"]), (tag, loss, ref["loss"])
        assert np.abs(g6 - ref["g6"]).max() <= G6_RTOL * np.abs(ref["g6"]).max(), (tag, g6, ref["g6"])
    big = max(np.abs(ref["gs"][:, ok]).max() / P, 1e-30); n_bad = 0; n_all = 0
    for j, d in enumerate(dumps):
        ev = (np.arange(64)[None, :] < d["count"][:, None]) & ok[:, None]
        a = d["dldx"][ev].astype(np.float64); b = ref["gs"][j][ev] / P
        err = np.abs(a - b).max(-1); tol = DLDX_TOL * np.maximum(np.abs(b).max(-1), DLDX_FLOOR * big)
        n_bad += int((err > tol).sum()); n_all += err.size
    print("%s: %d of %d samples' dL/dx outside the bar" % (tag, n_bad, n_all))
    assert n_all > 0 and n_bad <= (1.0 - DLDX_FRAC) * n_all, (tag, n_bad, n_all)
    return l_ref is not None


def _np_ref_from_dumps(dumps, rs, prm):
    """the fp64 composite (loss, cut) of the device's own raw outputs and distances, each object's own cut held at the device's count"""
    lists = []
    for j, d in enumerate(dumps):
        a, c, _ = sref.lists_from_raw(d["raw"], d["t"], rs["objs"][j]["hit"])
        lists.append((d["t"], a, c, d["count"].astype(np.uint32)))
    return sref.np_composite_grad(np.stack([q[0] for q in lists]), np.stack([q[1] for q in lists]), np.stack([q[2] for q in lists]),
                                  np.stack([q[3] for q in lists]), rs["cstar"], np.stack([o["mstar"] for o in rs["objs"]]), rs["dstar"], rs["dn"],
                                  (prm.w_rgb, prm.w_mask, prm.w_depth, prm.depth_huber))


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_whole_chain_matches_fp64_autograd(pkg, orc, ss, scene, trained, tmp_path, order):
    """{object 0 on its 5x box (base.json), object 1 (32 x 2)} in both orders on view 23: every pixel of one 48 x 48 crop over the silhouette overlap, and 2048
    drawn rays over the two padded boxes at iteration 7; each at the dataset's pose and 3 degrees / 3 % of the camera distance off; one case with a c2f
    window row as level weights and one on side 1.  Loss, grad6 and every sample's dL/dx against one fp64 autograd graph of the objective."""
    sc = scene; _, objs_all, _ = trained
    objs, metas = _pair(sc, objs_all, order)
    crop = np.array([[VIEW, 194, 91, 48, 48]], np.uint32); padded = _view_boxes(sc, VIEW, (0, 1))
    Ttrue = sc.Twc[VIEW]; Toff = _perturb_camera(Ttrue, 3.0, 0.03 * _cam_dist(sc, VIEW), 11)
    p_all = pkg.pose_refine_default(rays_per_iter=0); p_draw = pkg.pose_refine_default(rays_per_iter=2048)
    lw = pkg.pose_c2f_weights(16, 100, 35)
    cases = [("crop_true", crop, Ttrue, p_all, 0, 0, None), ("crop_off", crop, Toff, p_all, 0, 0, None), ("draw_true", padded, Ttrue, p_draw, 0, 7, None),
             ("draw_off", padded, Toff, p_draw, 0, 7, None), ("draw_off_lw", padded, Toff, p_draw, 0, 7, lw), ("draw_off_side1", padded, Toff, p_draw, 1, 7, None)]
    for tag, boxes, T, prm, side, it, w in cases:
        rs, dumps, loss, g6, ref, case = _chain_case(pkg, orc, ss, sc, objs, metas, boxes, T, prm, tmp_path, tag, side, it, w)
        P = rs["x"].size
        g = _groups(rs, dumps, ref["amb"])
        npc = _np_ref_from_dumps(dumps, rs, prm)
        cut_before_far = (npc["ncut"] < npc["ntot"]) & g["interleaved"]       # the merged cut falls before the farther list ends
        inst = rs["inst"]; cls = [m["cls"] for m in metas]
        M = case["mstar"].max(0) > 0; herr = np.abs(ref["D"] - rs["dstar"])[M & (rs["dstar"] > 0)]
        counts = dict(miss=int(g["miss"].sum()), one=int(g["one"].sum()), interleaved=int(g["interleaved"].sum()), cut=int(cut_before_far.sum()),
                      inst_a=int((inst == cls[0]).sum()), inst_b=int((inst == cls[1]).sum()), background=int((inst == 0).sum()),
                      huber_lin=int((herr > prm.depth_huber).sum()), huber_quad=int((herr <= prm.depth_huber).sum()))
        print(tag, counts)
        need = ["interleaved", "cut", "background"] + (["huber_lin", "huber_quad"] if T is Toff else [])
        for k in need:
            assert counts[k] >= 10, (tag, k, counts)
        # groups the view's geometry may not have at all (object 1 is wholly hidden behind object 0 in view 23; the 5x box fills the crop)
        for k in ("miss", "one", "inst_a", "inst_b"):
            assert counts[k] == 0 or counts[k] >= 10, (tag, k, counts)
        assert counts["inst_a"] + counts["inst_b"] >= 10, (tag, counts)
        if not _check_chain(tag, rs, dumps, loss, g6, ref, P):
            # rays at the cut's edge left out of the fp64 mean: the device's loss against the fp64 composite of its own raw outputs instead
            pytest.fail("%s: %d ambiguous rays; pick another crop" % (tag, int(ref["amb"].sum())))


# ------------------------------------------------------------------ 3. K = 1 equals the object route
def test_one_object_equals_the_object_route(pkg, ss, scene, trained):
    """objs = {o} at the dataset's Twc: the loss is mon_object_pose_loss(o, Tow_o)'s and grad6 is that call's mapped into the camera frame by
    grad_rho = R^T G_rho, grad_phi = R^T (G_phi - p x G_rho), Toc = (R, p) -- each within twice the fp64 bars (each side is within one bar of the same
    reference).  Level weights of 0 give grad6 == 0 exactly, weights of 1 the NULL-weights bits."""
    sc = scene; _, objs, _ = trained
    for name, k in (("a0", 0), ("n1", 1), ("c1", 1)):
        o = objs[name]; ob = sc.objects[k]; boxes = _view_boxes(sc, VIEW, (k,))
        Twc16 = ss.colmajor(sc.Twc[VIEW]); Tow16 = ss.colmajor(ob["Tow"])
        for prm, it in ((pkg.pose_refine_default(rays_per_iter=0), 0), (pkg.pose_refine_default(rays_per_iter=2048), 7)):
            ls, gs = pkg.scene_pose_loss([o], boxes, Twc16, prm, iteration=it)
            lo, go = o.pose_loss(boxes, Tow16, prm, iteration=it)
            Toc = np.asarray(ob["Tow"], np.float64) @ sc.Twc[VIEW]; R, p = Toc[:3, :3], Toc[:3, 3]
            gm = np.concatenate([R.T @ go[:3], R.T @ (go[3:] - np.cross(p, go[:3]))])
            print("%s rays %d: loss %.6f / %.6f, grad6 rel %.2e" % (name, prm.rays_per_iter, ls, lo, np.abs(gs - gm).max() / np.abs(gm).max()))
            assert abs(ls - lo) <= 2 * LOSS_RTOL * abs(lo), (name, ls, lo)
            assert np.abs(gs - gm).max() <= 2 * G6_RTOL * np.abs(gm).max(), (name, gs, gm)
            L = o.cfg.n_levels
            l0, g0 = pkg.scene_pose_loss([o], boxes, Twc16, prm, iteration=it, level_weights=np.zeros(L, np.float32))
            l1, g1 = pkg.scene_pose_loss([o], boxes, Twc16, prm, iteration=it, level_weights=np.ones(L, np.float32))
            assert l0 == ls and (g0 == 0).all()
            assert l1 == ls and np.array_equal(g1.view(np.uint32), gs.view(np.uint32))


# ------------------------------------------------------------------ 4. past one grid pass
@pytest.mark.parametrize("N", [1, 4095, 4097, 12289])
def test_drawn_rays_past_one_grid_pass(pkg, ss, scene, trained, N):
    """K = 2, N drawn rays (one workgroup pass of the objects' kernels holds 4096): positions equal the restatement, the loss equals the fp64 composite of the
    dumped raw outputs, rays i < min(N, 4095) are those of another N bit for bit, and the repeated call returns the same bits."""
    sc = scene; _, objs_all, _ = trained
    objs, metas = _pair(sc, objs_all, (0, 1)); boxes = _view_boxes(sc, VIEW, (0, 1))
    Twc16 = ss.colmajor(_perturb_camera(sc.Twc[VIEW], 1.0, 0.01, 3)); prm = pkg.pose_refine_default(rays_per_iter=N)
    IT = 6                                                                # (ray 0 of this iteration is pixel (223, 100), on object 0: N = 1 has a loss to compare)
    rs = sref.scene_rays(sc, boxes, _mat(Twc16), metas, n_rays=N, seed=prm.seed, iteration=IT)
    assert rs["inst"][0] == sc.objects[0]["cls"]
    dumps = _dump_all(pkg, objs, boxes, Twc16, prm, 0, IT)
    for j, d in enumerate(dumps):
        h = rs["objs"][j]["hit"]; ext = float(np.linalg.norm(metas[j]["aabb"][1] - metas[j]["aabb"][0]))
        assert np.array_equal(d["count"] > 0, h)
        if h.any():
            assert np.abs(d["x_o"][h] - rs["objs"][j]["x_o"][h]).max() <= POS_TOL * ext
    ref = _np_ref_from_dumps(dumps, rs, prm)
    loss, g6 = pkg.scene_pose_loss(objs, boxes, Twc16, prm, iteration=IT)
    loss2, g62 = pkg.scene_pose_loss(objs, boxes, Twc16, prm, iteration=IT)
    assert loss == loss2 and np.array_equal(g6.view(np.uint32), g62.view(np.uint32))
    assert ref["amb"].sum() <= max(N // 100, 0) or N < 100
    if not ref["amb"].any():
        print("N %d: loss %.6f, fp64 composite of the dumped outputs %.6f" % (N, loss, ref["l"].mean()))
        assert abs(loss - ref["l"].mean()) <= LOSS_RTOL * abs(ref["l"].mean())
    m = min(N, 4095)
    other = _dump_all(pkg, objs, boxes, Twc16, pkg.pose_refine_default(rays_per_iter=4095 if N != 4095 else 4097), 0, IT)
    for d, e in zip(dumps, other):
        for key in ("x_o", "x_c", "t", "raw", "count"):
            assert np.array_equal(d[key][:m].view(np.uint32), e[key][:m].view(np.uint32)), key


# ------------------------------------------------------------------ 5. refinement
def _refine_runs(pkg, ss, sc, objs, c2f, tag):
    boxes = _view_boxes(sc, VIEW, (0, 1)); Ttrue = sc.Twc[VIEW]; prm = pkg.pose_refine_default(); out = []
    for seed in (1, 2, 3):
        T0 = _perturb_camera(Ttrue, 3.0, 0.03 * _cam_dist(sc, VIEW), seed)
        pose, trace = pkg.scene_refine_camera(objs, boxes, ss.colmajor(T0), prm, c2f=c2f)
        e0 = _camera_errors(T0, Ttrue); e1 = _camera_errors(_mat(pose), Ttrue)
        print("%s seed %d: rotation %.3f -> %.4f deg, translation %.4f -> %.5f, loss %.5f -> %.5f" % (tag, seed, e0[0], e1[0], e0[1], e1[1], trace[0], trace[-1]))
        assert np.isfinite(trace).all() and np.isfinite(pose).all()
        out.append((e0, e1, trace))
    return out


def test_refinement_pulls_the_camera_back(pkg, ss, scene, trained):
    """The camera of view 23 started 3 degrees / 3 % of its distance off (three seeds), 100 default steps over the frame's two padded boxes: two objects on
    an 8-level, scale-1.5 grid; two base.json objects with the default c2f schedule; and the same without it (reported, not barred).  Every run's trace ends
    below its start; every 8-level and every base.json c2f run ends closer to the true camera pose than it started in angle and translation, within
    REFINE_BARS (2x the worst seed measured on an MI355X, no tighter than Adam's step)."""
    sc = scene; _, objs, _ = trained
    for tag, pair, c2f in (("coarse", [objs["c0"], objs["c1"]], None), ("base_c2f", [objs["a0"], objs["a1"]], True), ("base_plain", [objs["a0"], objs["a1"]], None)):
        runs = _refine_runs(pkg, ss, sc, pair, c2f, tag)
        for e0, e1, trace in runs:
            if tag != "base_plain":                                           # (the plain base.json run is reported, not barred)
                assert trace[-1] < trace[0], (tag, trace[[0, -1]])
                assert e1[0] < e0[0] and e1[1] < e0[1], (tag, e0, e1)
                assert e1[0] <= REFINE_BARS[tag][0] and e1[1] <= REFINE_BARS[tag][1], (tag, e1, REFINE_BARS[tag])
        print("%s: worst end %.4f deg, %.5f" % (tag, max(r[1][0] for r in runs), max(r[1][1] for r in runs)))


# ------------------------------------------------------------------ 6. read-only
def _stats_tuple(s):
    return tuple(sorted(s.items()))


@pytest.mark.parametrize("side", [0, 1])
def test_refinement_is_read_only(pkg, ss, scene, trained, side):
    """around a refinement on each side, for every object: parameter CRCs (all three copies), mon_object_info, render-skip statistics and grid_builds, the
    snapshot step, and a following mon_object_pose_loss bit for bit"""
    sc = scene; _, objs, _ = trained; pair = [objs["c0"], objs["c1"]]
    boxes = _view_boxes(sc, VIEW, (0, 1)); prm = pkg.pose_refine_default(iters=10, rays_per_iter=1024); p1 = pkg.pose_refine_default(rays_per_iter=256)

    def snap():
        out = []
        for k, o in enumerate(pair):
            i = o.info()
            out.append((tuple(zlib.crc32(o.get_params(c).tobytes()) for c in range(3)), tuple(getattr(i, f) for f, _ in type(i)._fields_),
                        _stats_tuple(o.render_skip_stats(0)), _stats_tuple(o.render_skip_stats(1)),
                        int(o.render_snapshot(boxes[k], ss.colmajor(sc.Twc[VIEW]))[-1])))
        return out

    def losses():
        return [o.pose_loss(boxes[k:k + 1], ss.colmajor(sc.objects[k]["Tow"]), p1, iteration=3) for k, o in enumerate(pair)]

    l_before = losses(); before = snap()
    T0 = ss.colmajor(_perturb_camera(sc.Twc[VIEW], 2.0, 0.02, 5))
    pose, trace = pkg.scene_refine_camera(pair, boxes, T0, prm, c2f=True, side=side)
    pose2, trace2 = pkg.scene_refine_camera(pair, boxes, T0, prm, c2f=True, side=side)
    assert np.array_equal(pose.view(np.uint32), pose2.view(np.uint32)) and np.array_equal(trace.view(np.uint32), trace2.view(np.uint32))
    assert before == snap()
    for (a, ga), (b, gb) in zip(l_before, losses()):
        assert a == b and np.array_equal(ga.view(np.uint32), gb.view(np.uint32))


# ------------------------------------------------------------------ 7. the online path while the manager trains, and the errors
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


def test_online_refine_camera_while_training(pkg, ss, scene):
    """mon_online_refine_camera before anything is published (MON_ERR_STATE), then from a second thread while the manager's two objects train: MON_OK with a
    finite, decreasing trace; the dataset's pose of the frame is what it was."""
    sc = scene
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    boxes = _view_boxes(sc, VIEW, (0, 1)); prm = pkg.pose_refine_default(iters=20, rays_per_iter=1024)
    T0 = ss.colmajor(_perturb_camera(sc.Twc[VIEW], 2.0, 0.02, 6))
    for v in range(sc.n_views):
        m.new_frame(v, "%.6f" % (v * 0.1), sc.rgb[v][..., ::-1], sc.instance[v], ss.colmajor(sc.Twc[v]))
    with pytest.raises(pkg.MonError) as e:
        m.refine_camera(boxes, T0, prm)                     # no object at all
    assert e.value.code == 5
    ids = [m.create_nerf(sc.objects[k]["cls"], ss.colmajor(sc.objects[k]["Tow"]), -sc.objects[k]["half"] / 1.1, sc.objects[k]["half"] / 1.1) for k in range(2)]
    with pytest.raises(pkg.MonError) as e:
        m.refine_camera(boxes, T0, prm)                     # objects, nothing published
    assert e.value.code == 5
    pose_before = m.get_pose(VIEW).copy()
    published = threading.Event(); res = dict(err=None, out=None, state_errors=0)

    def frontend():
        try:
            published.wait(timeout=120)
            res["out"] = m.refine_camera(boxes, T0, prm, c2f=True)
        except Exception as ex:        # noqa: BLE001 -- reported by the main thread
            res["err"] = ex

    th = threading.Thread(target=frontend); th.start()
    try:
        for k in range(2):
            m.update_nerf_bbox(ids[k], sc.objects[k]["boxes"], 200)
        import time
        t0 = time.time()
        while not all(m.object_info(i)["train_calls"] >= 1 for i in ids) and time.time() - t0 < 90:
            time.sleep(0.02)
    finally:
        published.set(); th.join(timeout=120)
    still_training = any(m.object_info(i)["train_calls"] < 200 for i in ids)
    m.wait_threads_end()
    assert res["err"] is None and res["out"] is not None, res
    pose, trace = res["out"]
    print("online: trace %.5f -> %.5f, objects still training when the call was made: %s" % (trace[0], trace[-1], still_training))
    assert np.isfinite(pose).all() and np.isfinite(trace).all() and trace[-1] < trace[0]
    assert np.array_equal(m.get_pose(VIEW).view(np.uint32), pose_before.view(np.uint32))
    m.close()


def test_scene_pose_errors(pkg, ss, scene, trained):
    """MON_ERR_ARG rows that need objects: boxes of two frames, a frame the dataset does not hold, boxes outside the frame, objects on two datasets, other
    intrinsics or two logical devices, bad level weights and schedules; MON_ERR_STATE for a layer-kernel shape, the XORWOW mode and side 1 unpublished."""
    sc = scene; ds, objs, _ = trained; pair = [objs["a0"], objs["a1"]]
    T = ss.colmajor(sc.Twc[VIEW]); boxes = _view_boxes(sc, VIEW, (0, 1)); prm = pkg.pose_refine_default(iters=2, rays_per_iter=256)

    def code(fn):
        with pytest.raises(pkg.MonError) as e:
            fn()
        return e.value.code
    two = boxes.copy(); two[1, 0] = VIEW - 1
    absent = boxes.copy(); absent[:, 0] = 200
    for b in (two, absent, np.array([[VIEW, sc.W - 10, 0, 8, 16]], np.uint32), np.array([[VIEW, 0, 0, 0, 8]], np.uint32)):
        assert code(lambda: pkg.scene_pose_loss(pair, b, T, prm)) == 1
        assert code(lambda: pkg.scene_refine_camera(pair, b, T, prm)) == 1
    assert code(lambda: pkg.scene_refine_camera(pair, boxes, T, pkg.pose_refine_default(iters=-1))) == 1
    assert code(lambda: pkg.scene_pose_loss(pair, boxes, T, pkg.pose_refine_default(rays_per_iter=(1 << 22) + 1))) == 1
    assert code(lambda: pkg.scene_pose_loss(pair, boxes, T, prm, side=2)) == 1
    assert code(lambda: pkg.scene_pose_loss(pair, boxes, T, prm, level_weights=-np.ones(16, np.float32))) == 1
    assert code(lambda: pkg.scene_refine_camera(pair, boxes, T, prm, c2f=dict(ramp=0.0))) == 1
    ds2, other = ge.make_problem(pkg, sc, BASE, use_depth=True, obj_index=1)
    ds3 = pkg.Dataset(0, sc.H, sc.W, sc.fx * 1.5, sc.fy, sc.cx, sc.cy, sc.n_views, use_depth=True)
    ob = sc.objects[1]
    o3 = pkg.ObjectNeRF(ds3, pkg.default_config(**BASE), ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    _, c = ge.make_problem(pkg, sc, dict(n_neurons=16), dataset=ds)
    _, x = ge.make_problem(pkg, sc, dict(BASE, rng_flags=1), dataset=ds)
    _, fresh = ge.make_problem(pkg, sc, BASE, obj_index=1, dataset=ds)
    try:
        assert code(lambda: pkg.scene_pose_loss([objs["a0"], other], boxes, T, prm)) == 1            # another dataset
        assert code(lambda: pkg.scene_pose_loss([objs["a0"], o3], boxes, T, prm)) == 1               # other intrinsics
        for lst, side in (([c], 0), ([objs["a0"], c], 0), ([x], 0), ([fresh], 1), ([objs["a0"], fresh], 1)):
            assert code(lambda: pkg.scene_pose_loss(lst, boxes, T, prm, side=side)) == 5, (len(lst), side)
    finally:
        for q in (c, x, fresh, other, o3, ds2, ds3):
            q.close()
    pkg.set_logical_devices(2)
    try:
        ds0, o0 = ge.make_problem(pkg, sc, BASE, device=0, obj_index=0)
        ds1, o1 = ge.make_problem(pkg, sc, BASE, device=1, obj_index=1)
        assert code(lambda: pkg.scene_pose_loss([o0, o1], boxes, T, prm)) == 1
        for o in (o0, o1, ds0, ds1):
            o.close()
    finally:
        pkg.set_logical_devices(0)
