#!/usr/bin/env python
"""Cost and step-size sweep of camera refinement against a scene of objects (mon_scene_refine_camera: per Adam step k_scene_pose_rays, every object's
k_scene_pose_obj forward, k_scene_composite_grad, every object's k_scene_pose_obj backward, k_scene_pose_update) on trained objects (runs on the GPU box).

    python tools/scene_track_timing.py [--steps 300] [--iters 100] [--reps 5]
    python tools/scene_track_timing.py --sweep            (lr_trans / lr_rot sweep of the refinement on view 23 of the scene, three perturbation seeds)
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/scene_track_timing.py     (per-kernel times: OUT/.../t_kernel_stats.csv)

Cost: K in {1, 2, 8} base.json objects of the three-object synthetic scene (24 views of 240 x 320; K = 8 repeats the three objects) and 1 024 / 4 096 rays
per step over the view's padded boxes: the wall time of an `iters`-step refinement (best of `reps`, after a warm-up) minus that of a 0-step call, divided
by `iters`, next to K x the same figure of mon_object_refine_pose on one of the objects in the same run.  One JSON line per case."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VIEW = 23


def _boxes(sc, ks, pad=16):
    out = []
    for k in ks:
        b = [q for q in sc.objects[k]["boxes"] if int(q[0]) == VIEW][0]
        _, x, y, h, w = (int(q) for q in b)
        x0, y0 = max(0, x - pad), max(0, y - pad); x1, y1 = min(sc.W, x + w + pad), min(sc.H, y + h + pad)
        out.append((VIEW, x0, y0, y1 - y0, x1 - x0))
    return np.array(out, np.uint32)


def _best(fn, reps):
    fn(); best = None
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def _perturb(Twc, rot_deg, trans, seed):
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    th = math.radians(rot_deg); K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    D = np.eye(4); D[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K; D[:3, 3] = d * trans
    return Twc @ D


def _errors(T, T_true):
    R = T[:3, :3].T @ T_true[:3, :3]
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2)))), float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=240, W=320, f=260.0, n_objects=3, seed=3, elev_deg=10.0)
    ds = None; objs = []
    for k in range(3):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=5 + k), use_depth=True, obj_index=k, dataset=ds)
        o.set_backend(1); o.train(a.steps); objs.append(o)
    Ttrue = sc.Twc[VIEW]; T = ss.colmajor(Ttrue)
    if a.sweep:
        boxes = _boxes(sc, (0, 1)); dist = float(np.linalg.norm(Ttrue[:3, 3]))
        for c2f in (True, None):
            for lr_t, lr_r in ((1e-3, 2e-3), (2e-3, 4e-3), (5e-3, 4e-3), (5e-3, 1e-2), (1e-2, 4e-3)):
                ends = []
                for seed in (1, 2, 3):
                    T0 = _perturb(Ttrue, 3.0, 0.03 * dist, seed)
                    pose, trace = pkg.scene_refine_camera(objs[:2], boxes, ss.colmajor(T0), pkg.pose_refine_default(lr_trans=lr_t, lr_rot=lr_r), c2f=c2f)
                    ends.append(_errors(np.asarray(pose, np.float64).reshape(4, 4).T, Ttrue) + (float(trace[0]), float(trace[-1])))
                print(json.dumps(dict(c2f=bool(c2f), lr_trans=lr_t, lr_rot=lr_r, end_deg=[round(e[0], 4) for e in ends], end_trans=[round(e[1], 5) for e in ends],
                                      loss=[(round(e[2], 5), round(e[3], 5)) for e in ends])), flush=True)
    else:
        for K in (1, 2, 8):
            lst = [objs[i % 3] for i in range(K)]; boxes = _boxes(sc, sorted(set(i % 3 for i in range(K))))
            ob = sc.objects[0]; Tow = ss.colmajor(ob["Tow"])
            for rays in (1024, 4096):
                out = {}; one = {}
                for iters in (0, a.iters):
                    prm = pkg.pose_refine_default(iters=iters, rays_per_iter=rays)
                    out[iters] = _best(lambda: pkg.scene_refine_camera(lst, boxes, T, prm), a.reps)
                    one[iters] = _best(lambda: objs[0].refine_pose(boxes[:1], Tow, prm), a.reps)
                per = (out[a.iters] - out[0]) / a.iters; per1 = (one[a.iters] - one[0]) / a.iters
                print(json.dumps(dict(K=K, rays=rays, iters=a.iters, ms_per_step=round(1e3 * per, 4), ms_fixed=round(1e3 * out[0], 3),
                                      K_x_object_ms_per_step=round(1e3 * K * per1, 4), object_ms_per_step=round(1e3 * per1, 4))), flush=True)
    for o in objs:
        o.close()
    ds.close()


if __name__ == "__main__":
    main()
