#!/usr/bin/env python
"""Cost of batched pose scoring (mon_scene_pose_loss_batch: per pass k_scene_score_rays, every object's k_scene_pose_obj forward, k_scene_composite_loss,
k_scene_loss_reduce) against the loop of single mon_scene_pose_loss calls it replaces, on trained objects (runs on the GPU box).

    python tools/reloc_timing.py [--steps 300] [--reps 5]
    python tools/reloc_timing.py --reloc           (one mon_scene_relocalise next to one mon_scene_refine_camera: wall time and ending errors)
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/reloc_timing.py     (per-kernel times: OUT/.../t_kernel_stats.csv)

K in {1, 2, 8} base.json objects of the three-object synthetic scene (24 views of 240 x 320; K = 8 repeats the three objects), H in {16, 64, 256} candidate
poses within 10 degrees / 5 % of the camera of view 23, 256 / 1 024 rays per hypothesis over the view's padded boxes.  Wall time of one batch call and of the
loop of H single calls (best of `reps`, after a warm-up), and whether the two gave the same bits.  One JSON line per case."""
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
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--reloc", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=240, W=320, f=260.0, n_objects=3, seed=3, elev_deg=10.0)
    ds = None; objs = []
    for k in range(3):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=5 + k), use_depth=True, obj_index=k, dataset=ds)
        o.set_backend(1); o.train(a.steps); objs.append(o)
    Ttrue = sc.Twc[VIEW]; T = ss.colmajor(Ttrue)
    centre = np.mean([-ob["Tow"][:3, :3].T @ ob["Tow"][:3, 3] for ob in sc.objects[:2]], 0); dist = float(np.linalg.norm(Ttrue[:3, 3] - centre))
    if a.reloc:
        boxes = _boxes(sc, (0, 1)); prm = pkg.pose_refine_default(); rp = pkg.reloc_default()
        for seed in (1, 2, 3):
            T0 = _perturb(Ttrue, 12.0, 0.10 * dist, seed); T16 = ss.colmajor(T0)
            pivot = (np.linalg.inv(T0) @ np.append(centre, 1.0))[:3].astype(np.float32)
            cand = pkg.pose_hypotheses(T16, 64, math.radians(15.0), 0.10 * dist, pivot=pivot, seed=seed)
            out = {}
            t_reloc = _best(lambda: out.__setitem__("r", pkg.scene_relocalise(objs[:2], boxes, cand, prm, True, rp)), 1)
            t_local = _best(lambda: out.__setitem__("l", pkg.scene_refine_camera(objs[:2], boxes, T16, prm, c2f=True)), 1)
            er = _errors(np.asarray(out["r"][0], np.float64).reshape(4, 4).T, Ttrue); el = _errors(np.asarray(out["l"][0], np.float64).reshape(4, 4).T, Ttrue)
            print(json.dumps(dict(seed=seed, reloc_ms=round(1e3 * t_reloc, 2), local_ms=round(1e3 * t_local, 2), reloc_end=(round(er[0], 3), round(er[1], 4)),
                                  local_end=(round(el[0], 3), round(el[1], 4)), best_candidate=int(out["r"][1].best_candidate),
                                  refined=int(out["r"][1].refined), score_final=float(out["r"][1].score_final))), flush=True)
    else:
        for K in (1, 2, 8):
            lst = [objs[i % 3] for i in range(K)]; boxes = _boxes(sc, sorted(set(i % 3 for i in range(K))))
            pivot = (np.linalg.inv(Ttrue) @ np.append(centre, 1.0))[:3].astype(np.float32)
            for rays in (256, 1024):
                prm = pkg.pose_refine_default(rays_per_iter=rays)
                for H in (16, 64, 256):
                    cand = pkg.pose_hypotheses(T, H, math.radians(10.0), 0.05 * dist, pivot=pivot, seed=1)
                    out = {}
                    t_batch = _best(lambda: out.__setitem__("b", pkg.scene_pose_loss_batch(lst, boxes, cand, prm, iteration=3)), a.reps)
                    t_loop = _best(lambda: out.__setitem__("s", np.array([pkg.scene_pose_loss(lst, boxes, c, prm, iteration=3)[0] for c in cand], np.float32)),
                                   a.reps)
                    print(json.dumps(dict(K=K, rays=rays, H=H, batch_ms=round(1e3 * t_batch, 3), loop_ms=round(1e3 * t_loop, 3),
                                          speedup=round(t_loop / t_batch, 2), passes=-(-H // min(H, 16384 // rays)),
                                          same_bits=bool(np.array_equal(out["b"].view(np.uint32), out["s"].view(np.uint32))))), flush=True)
    for o in objs:
        o.close()
    ds.close()


if __name__ == "__main__":
    main()
