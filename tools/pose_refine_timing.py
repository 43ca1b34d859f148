#!/usr/bin/env python
"""Cost of pose refinement (mon_object_refine_pose: k_pose_rays + k_pose_grad + k_pose_update per Adam step) on a trained object (runs on the GPU box).

    python tools/pose_refine_timing.py [--steps 500] [--iters 100] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/pose_refine_timing.py     (per-kernel times: OUT/.../t_kernel_stats.csv)

For base.json (16 levels, 64 x 1) and a 32 x 2 network, each trained `steps` iterations on a one-object synthetic scene (24 views of 240 x 320), and for
1 024 / 4 096 / 16 384 rays per step on 6 boxes: the wall time of `iters`-step refinements (best of `reps`, after a warm-up) minus that of a 0-step call
(the upload, the fragment image and the final read-back), divided by `iters` -- what one step costs with the whole refinement enqueued at once.  One JSON
line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500); ap.add_argument("--iters", type=int, default=100); ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=240, W=320, f=260.0, seed=3)
    ob = sc.objects[0]; b = ob["boxes"]; boxes = b[np.linspace(0, len(b) - 1, 6).astype(int)]
    ds = None
    for name, kw in (("base.json", dict(sample_seed=5)), ("32x2", dict(sample_seed=7, n_neurons=32, n_hidden_layers=2))):
        ds, o = ge.make_problem(pkg, sc, kw, use_depth=True, dataset=ds)
        o.set_backend(1); o.train(a.steps)
        T = ss.colmajor(ob["Tow"])
        for rays in (1024, 4096, 16384):
            out = {}
            for iters in (0, a.iters):
                prm = pkg.pose_refine_default(iters=iters, rays_per_iter=rays)
                o.refine_pose(boxes, T, prm)
                best = None
                for _ in range(a.reps):
                    t0 = time.perf_counter(); o.refine_pose(boxes, T, prm); dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                out[iters] = best
            per = (out[a.iters] - out[0]) / a.iters
            print(json.dumps(dict(network=name, rays=rays, iters=a.iters, ms_per_step=round(1e3 * per, 4), ms_call=round(1e3 * out[a.iters], 3),
                                  ms_fixed=round(1e3 * out[0], 3), us_per_kray=round(1e6 * per / (rays / 1024.0), 2))), flush=True)
        o.close()
    ds.close()


if __name__ == "__main__":
    main()
