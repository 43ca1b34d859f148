#!/usr/bin/env python
"""Kernel times of the point queries (mon_scene_query_points / mon_scene_query_lattice: k_scene_points + k_scene_points_fold) beside the parent's ways
of asking the same thing, from the same process (runs on the GPU box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_points_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/scene_points_timing.py stats OUT/configs.json OUT/p >> profiles/r16_scene_points.md

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_cast_timing.py), then on side 0, render skipping off:
  * lists of 512, 2 048, 8 192 and 262 144 world points drawn uniformly over the objects' bounding region, against all eight objects: `reps` point
    queries, and `reps` ray casts that answer the same points by a ray each (origin at the point, 64 evaluated samples per answer where a box is hit);
  * a 64^3 lattice inside object 0's box (every point inside: every tile of the new kernel is full), against object 0 alone;
  * the emit yardstick: `reps` scene probes of a rect through object 0's box (the keyed k_fused_render<EMIT>); the 32-sample tiles it evaluates are
    counted from mon_debug_scene_samples' counts of the same rect.
Every block of work starts and ends with a marker dispatch (mon_debug_scene_composite on 1 + block-number rays).  `stats` splits the trace at the
markers and prints per-call kernel milliseconds, the point / cast ratio, and the cost per evaluated 32-sample tile of the new kernel beside the emit's.
`run --lattice-only` trains object 0 alone and takes the last two blocks only: with MON_CORE_LIB pointing at a variant library built with another pass
size (tools/variant_build.sh pass128k -DMON_POINTS_PASS=131072u) it shows what the pass size costs."""
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

N_POINTS = (512, 2048, 8192, 262144)


def run(a):
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=24, H=480, W=640, f=525.0, n_objects=8, seed=0)
    ds = None; objs = []
    for k in range(1 if a.lattice_only else 8):
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

    # the objects' bounding region in the world (their box corners)
    sgn = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    cor = np.concatenate([(sgn * ob["half"]) @ ob["Two"][:3, :3].T + ob["Two"][:3, 3] for ob in sc.objects])
    lo, hi = cor.min(0), cor.max(0)
    for n in (() if a.lattice_only else N_POINTS):
        x = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
        rays = pkg.scene_rays(x, np.broadcast_to(np.array([0, 0, 1], np.float32), (n, 3)), t_max=np.inf, key=np.arange(n) % (1 << 26))
        nin = pkg.query_scene_points(objs, x, 0)[4]
        block("points", 8, n, lambda: pkg.query_scene_points(objs, x, 0), inside=int((nin > 0).sum()), tiles_inside=int(nin.sum()))
        block("cast", 8, n, lambda: pkg.cast_scene(objs, rays, 0.5, 0))
    # the all-inside lattice: a world cube inscribed in the sphere that object 0's box contains
    ob = sc.objects[0]; h = 0.95 * float(ob["half"].min()) / np.sqrt(3.0); c = ob["Two"][:3, 3]
    origin = (c - h).astype(np.float32); step = np.full(3, 2 * h / 63, np.float32)
    nin = pkg.query_scene_lattice(objs[:1], origin, step, (64, 64, 64), 0)[4]
    assert (nin == 1).all()
    block("lattice", 1, 64 ** 3, lambda: pkg.query_scene_lattice(objs[:1], origin, step, (64, 64, 64), 0), inside=int(nin.sum()), tiles=64 ** 3 // 32)
    # the emit yardstick: a rect around object 0's silhouette in view 0, probed; its evaluated tiles from the sample counts of the same rect
    v = int(ob["boxes"][0][0]); _, bx, by, bh, bw = (int(q) for q in ob["boxes"][0])
    rect = np.array([v, bx, by, bh, bw], np.uint32); pose = ss.colmajor(sc.Twc[v]); q = pkg.rect_queries(rect)
    cnt = pkg.scene_samples(objs[:1], rect, pose, 0, 0)[3]
    block("emit", 1, int(q.shape[0]), lambda: pkg.probe_scene(objs[:1], q, pose, 0), tiles=int(cnt.sum()) // 32)
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


def short(name):
    s = re.sub(r"\(.*", "", name); s = re.sub(r"^void ", "", s); s = re.sub(r"<.*", "", s); return re.sub(r"^mon::", "", s)


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
        kind = ("points" if n == "k_scene_points" else "fold" if n == "k_scene_points_fold" else "emit" if n == "k_fused_render" else
                "composite" if n in ("k_scene_cast_composite", "k_scene_probe_composite") else "rays" if n in ("k_scene_cast_rays", "k_scene_probe_rays") else "other")
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Point queries beside the ray cast and the emit kernel: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/scene_points_timing.py`; 8 base.json objects, 300 iterations each,"
          " side 0, render skipping off).  `points` = `mon_scene_query_points` of n world points drawn over the objects' bounding region; `cast` ="
          " `mon_scene_cast` of one ray per point (origin at the point, direction +z); `lattice` = `mon_scene_query_lattice` of a 64^3 lattice inside object 0's"
          " box, object 0 alone; `emit` = `mon_scene_probe` of a rect through object 0's box, object 0 alone.  `other` = fragment images and the copies."
          "  `wall` = host time per repetition under the tracer.  `us per tile` = the network kernel's time (k_scene_points, or the emit) per evaluated"
          " 32-sample tile.\n")
    print("| K | what | n | points / emit kernel | fold / composite | rays kernel | other | total | wall ms | tiles | us per tile | points / cast |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    tot_points = {}; per_tile = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(d.values()) / r
        net = f("points") if b["what"] in ("points", "lattice") else f("emit")
        if b["what"] == "points":
            tot_points[b["n"]] = tot
        ratio = "%.3f" % (tot_points[b["n"]] / tot) if b["what"] == "cast" and tot > 0 and b["n"] in tot_points else ""
        tiles = b.get("tiles", 0); upt = 1e3 * net / tiles if tiles else 0.0
        if tiles:
            per_tile[b["what"]] = upt
        print("| %d | %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %s | %s |" % (b["K"], b["what"], b["n"], net, f("fold") + f("composite"), f("rays"),
              f("other"), tot, b["wall_ms"], tiles or "", ("%.4f" % upt) if tiles else "", ratio))
    if "lattice" in per_tile and "emit" in per_tile and per_tile["emit"] > 0:
        print("\nPer evaluated tile: k_scene_points %.4f us, the emit %.4f us: ratio %.2f (allowed: 1.25)." % (per_tile["lattice"], per_tile["emit"],
              per_tile["lattice"] / per_tile["emit"]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    r.add_argument("--lattice-only", action="store_true", help="object 0 alone: the all-inside lattice and the emit yardstick (e.g. for a variant library)")
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
