#!/usr/bin/env python
"""Kernel times of the point gradients (mon_scene_query_gradients / mon_scene_query_lattice_gradients: k_scene_point_grads + k_scene_gradients_fold)
beside what a caller had to do before them -- six point queries at x +- h e_a -- from the same process (runs on the GPU box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_gradients_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/scene_gradients_timing.py stats OUT/configs.json OUT/p >> profiles/r17_scene_gradients.md

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_points_timing.py), then on side 0:
  * lists of 512, 2 048, 8 192 and 262 144 world points drawn uniformly over the objects' bounding region, against all eight objects: `reps` times one
    point query, the six point queries of a central difference, and one gradient call (no weights, no select);
  * a 64^3 lattice inside object 0's box (every point inside: every tile is full), against object 0 alone: the lattice query, its six shifted
    lattices, and the lattice gradient call.
Every block of work starts and ends with a marker dispatch (mon_debug_scene_composite on 1 + block-number rays).  `stats` splits the trace at the
markers and prints per-call kernel milliseconds, the ratio of the gradient call to the six queries, and the cost per evaluated 32-point tile of
k_scene_point_grads beside k_scene_points'."""
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

from scene_points_timing import N_POINTS, short       # noqa: E402

H_DIFF = 1e-3                # the step of the six-query difference (world units; its size does not change the work)


def run(a):
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=480, W=640, f=525.0, n_objects=8, seed=0)
    ds = None; objs = []
    for k in range(8):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=2024 + k), obj_index=k, dataset=ds); o.set_backend(1); o.train(a.steps); objs.append(o)
    rng = np.random.RandomState(0)
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
    cor = np.concatenate([(sgn * ob["half"]) @ ob["Two"][:3, :3].T + ob["Two"][:3, 3] for ob in sc.objects])
    lo, hi = cor.min(0), cor.max(0)
    shifts = [np.eye(3, dtype=np.float32)[d] * np.float32(s * H_DIFF) for d in range(3) for s in (1, -1)]
    for n in N_POINTS:
        x = rng.uniform(lo, hi, (n, 3)).astype(np.float32); six = [x + e for e in shifts]
        nin = pkg.query_scene_points(objs, x, 0)[4]
        block("points", 8, n, lambda: pkg.query_scene_points(objs, x, 0), inside=int((nin > 0).sum()), tiles_inside=int(nin.sum()))
        block("six", 8, n, lambda: [pkg.query_scene_points(objs, y, 0) for y in six])
        block("grads", 8, n, lambda: pkg.query_scene_gradients(objs, x))
    ob = sc.objects[0]; h = 0.95 * float(ob["half"].min()) / np.sqrt(3.0) - H_DIFF; c = ob["Two"][:3, 3]
    origin = (c - h).astype(np.float32); step = np.full(3, 2 * h / 63, np.float32); shape = (64, 64, 64); tiles = 64 ** 3 // 32
    assert (pkg.query_scene_lattice(objs[:1], origin, step, shape, 0)[4] == 1).all()
    block("points", 1, 64 ** 3, lambda: pkg.query_scene_lattice(objs[:1], origin, step, shape, 0), tiles=tiles)
    block("six", 1, 64 ** 3, lambda: [pkg.query_scene_lattice(objs[:1], origin + e, step, shape, 0) for e in shifts], tiles=6 * tiles)
    block("grads", 1, 64 ** 3, lambda: pkg.query_scene_lattice_gradients(objs[:1], origin, step, shape), tiles=tiles)
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


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
        kind = "net" if n in ("k_scene_points", "k_scene_point_grads") else "fold" if n in ("k_scene_points_fold", "k_scene_gradients_fold") else "other"
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Point gradients beside six point queries: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/scene_gradients_timing.py`; 8 base.json objects, 300 iterations"
          " each, side 0).  `points` = one `mon_scene_query_points` (K = 1: `mon_scene_query_lattice` of a 64^3 lattice inside object 0's box); `six` = the"
          " six point queries of a central difference; `grads` = one `mon_scene_query_gradients` (K = 1: `mon_scene_query_lattice_gradients`).  `other` ="
          " fragment images and the copies.  `wall` = host time per repetition under the tracer.  `us per tile` = the network kernel's time per evaluated"
          " 32-point tile (the all-inside lattice only).\n")
    print("| K | what | n | network kernel | fold | other | total | wall ms | tiles | us per tile | grads / six (kernel) | grads / six (wall) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    six = {}; per_tile = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(d.values()) / r; key = (b["K"], b["n"])
        if b["what"] == "six":
            six[key] = (tot, b["wall_ms"])
        rk = "%.3f" % (tot / six[key][0]) if b["what"] == "grads" and key in six and six[key][0] > 0 else ""
        rw = "%.3f" % (b["wall_ms"] / six[key][1]) if b["what"] == "grads" and key in six and six[key][1] > 0 else ""
        tiles = b.get("tiles", 0); upt = 1e3 * f("net") / tiles if tiles else 0.0
        if tiles:
            per_tile[b["what"]] = upt
        print("| %d | %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %s | %s | %s |" % (b["K"], b["what"], b["n"], f("net"), f("fold"), f("other"), tot,
              b["wall_ms"], tiles or "", ("%.4f" % upt) if tiles else "", rk, rw))
    if "points" in per_tile and "grads" in per_tile and per_tile["points"] > 0:
        print("\nPer evaluated tile: k_scene_point_grads %.4f us, k_scene_points %.4f us: ratio %.2f." % (per_tile["grads"], per_tile["points"],
              per_tile["grads"] / per_tile["points"]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
