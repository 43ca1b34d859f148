#!/usr/bin/env python
"""Kernel times of the distance fields (mon_scene_distance_lattice: the lattice query's kernels, then k_distance_mask + three k_distance_pass +
k_distance_finish, once more for free_dist) beside what a caller pays today before a host transform even starts -- mon_scene_query_lattice on the same
lattice with its copy home -- from the same process (runs on the GPU box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_distance_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/scene_distance_timing.py stats OUT/configs.json OUT/p >> profiles/r18_scene_distance.md

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_points_timing.py), then on side 0, for lattices of 64^3 and
128^3 over the objects' bounding region and K = 1 (object 0 alone) and K = 8 objects: `reps` times the lattice query (`query`), the distance call without
free_dist (`dist`) and with it (`dist+free`), and the standalone transform of the same mask from the host (`host mask`).  sigma_min is the density of
opacity 0.5 over one lattice step, -ln(0.5) / l.  Every block of work starts and ends with a marker dispatch (mon_debug_scene_composite on 1 +
block-number rays).  `stats` splits the trace at the markers and prints per-call kernel milliseconds by kind, the ratio (transform kernels) / (lattice
query kernels), and the whole call's wall time against the lattice query's."""
import argparse
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from scene_points_timing import short       # noqa: E402

SIZES = (64, 128)


def run(a):
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=480, W=640, f=525.0, n_objects=8, seed=0)
    ds = None; objs = []
    for k in range(8):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=2024 + k), obj_index=k, dataset=ds); o.set_backend(1); o.train(a.steps); objs.append(o)
    blocks = []

    def marker():
        n = len(blocks) + 1
        pkg.scene_composite(np.zeros((1, n, 64), np.float32), np.zeros((1, n, 64), np.float32), np.zeros((1, n, 64, 3), np.float32),
                            np.zeros((1, n), np.uint32), np.ones(n, np.float32))
        return n

    def block(what, K, n, fn, **extra):
        for _ in range(2):                                                   # warm-up (workspace grown)
            fn()
        b = dict(id=marker(), what=what, K=K, n=n, reps=a.reps, **extra)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        b["wall_ms"] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
        blocks.append(b); print(json.dumps(b), flush=True)
        blocks.append(dict(id=marker(), what="gap"))                          # (the next block's warm-up belongs to no row)

    sgn = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    for K in (1, 8):
        lst = objs[:K]
        cor = np.concatenate([(sgn * ob["half"]) @ ob["Two"][:3, :3].T + ob["Two"][:3, 3] for ob in sc.objects[:K]])
        lo, hi = cor.min(0), cor.max(0); pad = 0.1 * (hi - lo); lo = lo - pad; hi = hi + pad
        for r in SIZES:
            shape = (r, r, r); origin = lo.astype(np.float32); step = ((hi - lo) / (r - 1)).astype(np.float32)
            smin = float(-np.log(0.5) / float(step.min()))
            sigma = pkg.query_scene_lattice(lst, origin, step, shape, 0)[0]
            mask = (~(sigma <= np.float32(smin))).reshape(r, r, r)
            occ = int(mask.sum())
            block("query", K, r ** 3, lambda: pkg.query_scene_lattice(lst, origin, step, shape, 0), occupied=occ)
            block("dist", K, r ** 3, lambda: pkg.scene_distance_lattice(lst, origin, step, shape, smin, side=0, free=False), occupied=occ)
            block("dist+free", K, r ** 3, lambda: pkg.scene_distance_lattice(lst, origin, step, shape, smin, side=0, free=True), occupied=occ)
            if K == 1:
                block("host mask", 0, r ** 3, lambda: pkg.distance_transform(mask, step), occupied=occ)
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


QUERY = ("k_scene_points", "k_scene_points_fold", "k_build_frag_image")
PASSES = ("k_distance_pass",)
EDGES = ("k_distance_mask", "k_distance_finish")


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
        kind = "query" if n in QUERY else "passes" if n in PASSES else "edges" if n in EDGES else "other"
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Distance fields beside the lattice query: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/scene_distance_timing.py`; 8 base.json objects, 300 iterations"
          " each, side 0; lattices over the objects' bounding region).  `query` = one `mon_scene_query_lattice`; `dist` = one `mon_scene_distance_lattice`"
          " without free_dist; `dist+free` = with it; `host mask` = `mon_distance_transform` of the same mask uploaded from the host.  `query kernels` ="
          " `k_scene_points` + fold + fragment images; `passes` = the `k_distance_pass` dispatches (3 per transform); `mask+finish` = `k_distance_mask`"
          " and `k_distance_finish`; `other` = the copy kernel.  `wall` = host time per repetition under the tracer (copies home included).\n")
    print("| K | what | cells | occupied | query kernels | passes | mask+finish | other | total | transform / query (kernel) | wall ms | wall / query wall |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    qwall = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(d.values()) / r; key = (b["K"], b["n"])
        if b["what"] == "query":
            qwall[key] = b["wall_ms"]
        tr = f("passes") + f("edges")
        ratio = "%.3f" % (tr / f("query")) if f("query") > 0 and tr > 0 else ""
        rw = "%.3f" % (b["wall_ms"] / qwall[key]) if key in qwall and b["what"] != "query" else ""
        print("| %d | %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %.3f | %s |" % (b["K"], b["what"], b["n"], b.get("occupied", 0), f("query"),
              f("passes"), f("edges"), f("other"), tot, ratio, b["wall_ms"], rw))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
