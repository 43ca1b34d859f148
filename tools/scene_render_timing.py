#!/usr/bin/env python
"""Kernel times of the scene render (mon_scene_render: k_fused_render<EMIT> + k_scene_composite) against the same objects' own renders (runs on the GPU
box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_render_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/scene_render_timing.py stats OUT/configs.json OUT/p > profiles/r08_scene_render.md

`run` trains eight base.json objects of an eight-object synthetic scene (480 x 640 views), then for a 240 x 320 rect (the frame's centre) and the whole
640 x 480 frame, K = 1, 2, 4, 8 objects, side 0 and 1, render skipping off and on (min_alpha 1e-3): `reps` scene renders, then `reps` rounds of the K
objects' own renders of the same rect on the gather path (tile_render 0; mon_object_render on side 0, mon_object_render_snapshot on side 1).  Every
block of work starts with a marker dispatch (mon_debug_scene_composite on 1 + block-number rays: a k_scene_composite whose grid identifies the block;
the render's own composite launches have 8192 workgroups).  `stats` splits the trace at the markers and prints per-render kernel milliseconds."""
import argparse
import glob
import json
import os
import re
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a):
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=480, W=640, f=525.0, n_objects=8, seed=0)
    ds = None; objs = []
    for k in range(8):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=2024 + k), obj_index=k, dataset=ds); o.set_backend(1); o.train(a.steps); objs.append(o)
    v = 0; pose = ss.colmajor(sc.Twc[v])
    rects = {"320x240": np.array([v, 160, 120, 240, 320], np.uint32), "640x480": np.array([v, 0, 0, 480, 640], np.uint32)}
    blocks = []

    def marker():
        n = len(blocks) + 1
        pkg.scene_composite(np.zeros((1, n, 64), np.float32), np.zeros((1, n, 64), np.float32), np.zeros((1, n, 64, 3), np.float32),
                            np.zeros((1, n), np.uint32), np.ones(n, np.float32))
        return n

    pkg.set_option("tile_render", 0)
    for rname, rect in rects.items():
        for K in (1, 2, 4, 8):
            lst = objs[:K]
            for side in (0, 1):
                for skip in (False, True):
                    for o in lst:
                        o.set_render_skip(skip, 1e-3)
                    for _ in range(2):                                       # warm-up (grids built, workspace grown)
                        pkg.render_scene(lst, rect, pose, side)
                        for o in lst:
                            o.render(rect, pose) if side == 0 else o.render_snapshot(rect, pose)
                    cov = float((pkg.render_scene(lst, rect, pose, side)[2] > 0.5).mean())
                    blocks.append(dict(id=marker(), what="scene", rect=rname, K=K, side=side, skip=skip, reps=a.reps, coverage=round(cov, 4)))
                    for _ in range(a.reps):
                        pkg.render_scene(lst, rect, pose, side)
                    blocks.append(dict(id=marker(), what="own", rect=rname, K=K, side=side, skip=skip, reps=a.reps))
                    for _ in range(a.reps):
                        for o in lst:
                            o.render(rect, pose) if side == 0 else o.render_snapshot(rect, pose)
                    print(json.dumps(blocks[-2]), flush=True)
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.set_render_skip(False); o.close()
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
        kind = ("emit" if n.startswith("k_fused_render") and n.endswith("true>") else "composite" if n == "k_scene_composite" else
                "render" if n.startswith("k_fused_render") else "rays" if n == "k_render_rays" else "other")
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Scene render: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per render, ms of kernel time summed over the call's dispatches (`tools/scene_render_timing.py`; 8 base.json objects, 300 iterations each).")
    print("`own` = the same K objects rendered one by one on the gather path (`k_render_rays` + `k_fused_render`).  `other` = fragment images, grid builds,"
          " the copy home.\n")
    print("| rect | K | side | skip | coverage | scene: emit | composite | rays + other | total | own renders: total | scene / own |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    by = {}
    for i, b in blocks.items():
        if b["what"] in ("scene", "own"):
            by.setdefault((b["rect"], b["K"], b["side"], b["skip"]), {})[b["what"]] = (b, acc.get(i, {}))
    for key in sorted(by, key=lambda k: (k[0], k[1], k[2], k[3])):
        sb, sd = by[key]["scene"]; ob, od = by[key].get("own", (None, {}))
        r = sb["reps"]; f = lambda d, k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(sd.values()) / r; own = sum(od.values()) / r if od else float("nan")
        print("| %s | %d | %d | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f |" % (key[0], key[1], key[2], "on" if key[3] else "off",
              sb.get("coverage", 0.0), f(sd, "emit"), f(sd, "composite"), f(sd, "rays") + f(sd, "other"), tot, own, tot / own if own == own else 0.0))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
