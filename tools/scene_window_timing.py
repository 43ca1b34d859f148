#!/usr/bin/env python
"""Cost of window refinement (mon_scene_refine_window: per Adam step and pass k_scene_window_rays, every object's k_scene_pose_obj forward,
k_scene_window_composite, every object's k_scene_window_obj, then one k_scene_window_update) against the same frames through F mon_scene_refine_camera
calls in the same run, on trained objects (runs on the GPU box).

    python tools/scene_window_timing.py [--steps 300] [--iters 100] [--reps 7]
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/scene_window_timing.py     (per-kernel times: OUT/.../t_kernel_stats.csv)

F in {2, 8, 32} frames of the three-object synthetic scene (32 views of 240 x 320), {256, 1 024} rays per frame over each view's padded boxes, K in {1, 2, 8}
base.json objects (K = 8 repeats the three objects).  Per case the wall time of an `iters`-step call minus that of a 0-step call, divided by `iters`: the
window call with every camera free and the objects fixed (the work F single-frame refinements do), the window call with the objects free as well, and the
loop of F single-frame calls.  The variants alternate inside every repetition (one process, warm-up first); median and best of `reps` are reported, with the
launch counts per step: passes x (2 K + 2) + 1 against F x (2 K + 3), and 1 synchronisation against F.  One JSON line per case."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PASS_RAYS = 16384


def _boxes(sc, v, ks, pad=16):
    out = []
    for k in ks:
        b = [q for q in sc.objects[k]["boxes"] if int(q[0]) == v][0]
        _, x, y, h, w = (int(q) for q in b)
        x0, y0 = max(0, x - pad), max(0, y - pad); x1, y1 = min(sc.W, x + w + pad), min(sc.H, y + h + pad)
        out.append((v, x0, y0, y1 - y0, x1 - x0))
    return np.array(out, np.uint32)


def _time(fn):
    t0 = time.perf_counter(); fn(); return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, nargs="*", default=[2, 8, 32]); ap.add_argument("--rays", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--objects", type=int, nargs="*", default=[1, 2, 8])
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=32, H=240, W=320, f=260.0, n_objects=3, seed=3, elev_deg=10.0)
    ds = None; objs = []
    for k in range(3):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=5 + k), use_depth=True, obj_index=k, dataset=ds)
        o.set_backend(1); o.train(a.steps); objs.append(o)
    for K in a.objects:
        lst = [objs[i % 3] for i in range(K)]; ks = sorted(set(i % 3 for i in range(K)))
        own = np.stack([ss.colmajor(sc.objects[i % 3]["Tow"]) for i in range(K)])
        for F in a.frames:
            views = list(range(F)); per_frame = [_boxes(sc, v, ks) for v in views]; obs = np.concatenate(per_frame)
            Twc = np.stack([ss.colmajor(sc.Twc[v]) for v in views])
            for rays in a.rays:
                prm = {it: pkg.pose_refine_default(iters=it, rays_per_iter=rays) for it in (0, a.iters)}
                cams = pkg.window_default(n_fixed_frames=0, refine_objects=0); joint = pkg.window_default(n_fixed_frames=1, refine_objects=1)
                run = {
                    "window_cameras": lambda it: pkg.scene_refine_window(lst, obs, Twc, None, prm[it], window=cams),
                    "window_joint": lambda it: pkg.scene_refine_window(lst, obs, Twc, own, prm[it], window=joint),
                    "single_calls": lambda it: [pkg.scene_refine_camera(lst, per_frame[f], Twc[f], prm[it]) for f in range(F)],
                }
                for fn in run.values():                                           # warm-up of every shape the timed window uses
                    fn(0); fn(a.iters)
                t = {name: {0: [], a.iters: []} for name in run}
                for _ in range(a.reps):
                    for name, fn in run.items():
                        for it in (0, a.iters):
                            t[name][it].append(_time(lambda: fn(it)))
                row = dict(K=K, F=F, rays=rays, iters=a.iters, passes=-(-F * rays // (PASS_RAYS // rays * rays)) if rays else 0)
                row["launches_window"] = row["passes"] * (2 * K + 2) + 1; row["launches_single"] = F * (2 * K + 3)
                for name in run:
                    per = [(x - y) / a.iters for x, y in zip(t[name][a.iters], t[name][0])]
                    row[name + "_ms_per_step"] = round(1e3 * statistics.median(per), 4); row[name + "_ms_per_step_best"] = round(1e3 * min(per), 4)
                    row[name + "_ms_fixed"] = round(1e3 * statistics.median(t[name][0]), 3)
                row["single_over_window_cameras"] = round(row["single_calls_ms_per_step"] / row["window_cameras_ms_per_step"], 2)
                print(json.dumps(row), flush=True)
    for o in objs:
        o.close()
    ds.close()


if __name__ == "__main__":
    main()
