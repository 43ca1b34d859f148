#!/usr/bin/env python
"""Kernel times of the ray cast (mon_scene_cast: k_scene_cast_rays + keyed k_fused_render<EMIT> + k_scene_cast_composite) beside the scene probe's
for the same rays, from the same process (runs on the GPU box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_cast_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/scene_cast_timing.py stats OUT/configs.json OUT/p >> profiles/r15_scene_cast.md

`run` trains eight base.json objects of an eight-object synthetic scene (480 x 640 views, as tools/scene_probe_timing.py), then for K = 1 and 8 objects
on side 0, render skipping off, and n = 512, 2 048 and 8 192 sub-pixel points drawn uniformly over the frame under one pose: `reps` probes of the n
queries and `reps` casts of mon_camera_rays' rays for them (the same rays, the same keys, hit_opacity 0.5).  Every block of work starts and ends with a
marker dispatch (mon_debug_scene_composite on 1 + block-number rays: a k_scene_composite whose grid identifies the block).  The host's wall time per
call is taken too (under the tracer, so it is an upper figure).  `stats` splits the trace at the markers and prints per-call kernel milliseconds and
the cast / probe ratio."""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_RAYS = (512, 2048, 8192)


def run(a):
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=480, W=640, f=525.0, n_objects=8, seed=0)
    ds = None; objs = []
    for k in range(8):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=2024 + k), obj_index=k, dataset=ds); o.set_backend(1); o.train(a.steps); objs.append(o)
    pose = ss.colmajor(sc.Twc[0])
    rng = np.random.RandomState(0)
    blocks = []

    def marker():
        n = len(blocks) + 1
        pkg.scene_composite(np.zeros((1, n, 64), np.float32), np.zeros((1, n, 64), np.float32), np.zeros((1, n, 64, 3), np.float32),
                            np.zeros((1, n), np.uint32), np.ones(n, np.float32))
        return n

    def block(what, K, n, fn):
        for _ in range(2):                                                   # warm-up (workspace grown)
            fn()
        out = fn()
        b = dict(id=marker(), what=what, K=K, n=n, reps=a.reps, coverage=round(float((out[2] > 0.5).mean()), 4))
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        b["wall_ms"] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
        blocks.append(b); print(json.dumps(b), flush=True)
        blocks.append(dict(id=marker(), what="gap"))                          # (the next block's warm-up belongs to no row)

    for K in (1, 8):
        lst = objs[:K]
        for n in N_RAYS:
            u = rng.uniform(0.0, 639.0, n).astype(np.float32); v = rng.uniform(0.0, 479.0, n).astype(np.float32)
            q = pkg.scene_queries(0, np.arange(n), u, v)
            rays, _ = pkg.camera_rays((sc.fx, sc.fy, sc.cx, sc.cy), pose, q)
            block("probe", K, n, lambda: pkg.probe_scene(lst, q, pose, 0))
            block("cast", K, n, lambda: pkg.cast_scene(lst, rays, 0.5, 0))
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


def short(name):
    s = re.sub(r"\(.*", "", name); s = re.sub(r"^void ", "", s); return re.sub(r"^mon::", "", s)


def stats(a):
    blocks = {b["id"]: b for b in json.load(open(a.configs))}
    rows = []
    for p in sorted(glob.glob(os.path.join(a.trace, "**", "*_results.db"), recursive=True)):
        cur = sqlite3.connect(p).cursor()
        rows += list(cur.execute("select name, start, end, grid_x, workgroup_x from kernels order by start"))
    rows.sort(key=lambda r: r[1])
    acc = {}; cur_id = None
    for name, s, e, gx, wx in rows:
        n = short(name); blocks_n = gx // max(1, wx)
        if n == "k_scene_composite" and blocks_n in blocks and blocks_n < 4096:
            cur_id = blocks_n; continue
        if cur_id is None:
            continue
        kind = ("emit" if n.startswith("k_fused_render") else "composite" if n in ("k_scene_cast_composite", "k_scene_probe_composite") else
                "rays" if n in ("k_scene_cast_rays", "k_scene_probe_rays") else "other")
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Ray cast beside the scene probe: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/scene_cast_timing.py`; 8 base.json objects, 300 iterations each,"
          " side 0, render skipping off, one pose).  `probe` = `mon_scene_probe` of n sub-pixel points; `cast` = `mon_scene_cast` of `mon_camera_rays`' rays"
          " for the same points, hit_opacity 0.5, from the same process.  `other` = fragment images and the copy home.  `wall` = host time per repetition"
          " under the tracer.  `cast / probe` = the ratio of the two totals.\n")
    print("| K | what | rays | coverage | emit | composite | rays kernel | other | total | us per ray | wall ms | cast / probe |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    probe_total = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(d.values()) / r
        if b["what"] == "probe":
            probe_total[(b["K"], b["n"])] = tot
        base = probe_total.get((b["K"], b["n"]), 0.0)
        ratio = "%.3f" % (tot / base) if b["what"] == "cast" and base > 0 else ""
        print("| %d | %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s |" % (b["K"], b["what"], b["n"], b["coverage"], f("emit"),
              f("composite"), f("rays"), f("other"), tot, 1e3 * tot / b["n"], b["wall_ms"], ratio))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
