#!/usr/bin/env python
"""Kernel times of the signed, sub-cell distance fields (mon_scene_signed_distance_lattice: the lattice query's kernels, then k_distance_mask,
k_signed_values, three k_surface_line_pass, six k_distance_pass and k_signed_finish) beside today's route to a signed field, mon_scene_distance_lattice
with free_dist (two plain transforms), from the same process (runs on the GPU box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/signed_distance_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/signed_distance_timing.py stats OUT/configs.json OUT/p >> profiles/r28_signed_distance.md

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_distance_timing.py), then on side 0, for lattices of 64^3 and
128^3 over the objects' bounding region and K = 1 (object 0 alone) and K = 8 objects: `reps` times the lattice query (`query`), the distance call with
free_dist (`dist+free`), the signed call in log density (`signed`) and, for K = 1, the standalone signed transform of the same values from the host
(`host values`).  sigma_min is the density of opacity 0.5 over one lattice step, -ln(0.5) / l.  Every block of work starts and ends with a marker
dispatch (mon_debug_scene_composite on 1 + block-number rays).  `stats` splits the trace at the markers and prints per-call kernel milliseconds by kind,
the seed passes against the plain passes per dispatch, the signed transform against one plain transform, and its share of the whole signed call."""
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
            out = pkg.scene_signed_distance_lattice(lst, origin, step, shape, smin, side=0)
            val = out[4].reshape(r, r, r); iso = out[5]
            cross = int((out[1] >= 0).sum()); inside = int(np.signbit(out[0]).sum())
            block("query", K, r ** 3, lambda: pkg.query_scene_lattice(lst, origin, step, shape, 0), inside=inside)
            block("dist+free", K, r ** 3, lambda: pkg.scene_distance_lattice(lst, origin, step, shape, smin, side=0, free=True), inside=inside)
            block("signed", K, r ** 3, lambda: pkg.scene_signed_distance_lattice(lst, origin, step, shape, smin, side=0), inside=inside, with_edge=cross)
            if K == 1:
                block("host values", 0, r ** 3, lambda: pkg.signed_distance_transform(val, iso, step), inside=inside)
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


QUERY = ("k_scene_points", "k_scene_points_fold", "k_build_frag_image")
KINDS = {"k_surface_line_pass": "seed", "k_distance_pass": "plain", "k_distance_mask": "small", "k_distance_finish": "small", "k_signed_values": "small",
         "k_signed_finish": "small"}


def stats(a):
    blocks = {b["id"]: b for b in json.load(open(a.configs))}
    rows = []
    for p in sorted(glob.glob(os.path.join(a.trace, "**", "*_results.db"), recursive=True)):
        cur = sqlite3.connect(p).cursor()
        rows += list(cur.execute("select name, start, end, grid_x, workgroup_x from kernels order by start"))
    rows.sort(key=lambda r: r[1])
    acc = {}; cnt = {}; cur_id = None
    for name, s, e, gx, wx in rows:
        n = short(name); blocks_n = gx // max(1, wx)
        if n == "k_scene_composite" and blocks_n in blocks and blocks_n < 4096:
            cur_id = blocks_n; continue
        if cur_id is None:
            continue
        kind = "query" if n in QUERY else KINDS.get(n, "other")
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
        c = cnt.setdefault(cur_id, {}); c[kind] = c.get(kind, 0) + 1
    print("# Signed, sub-cell distance fields beside the mask-made signed field: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/signed_distance_timing.py`; 8 base.json objects, 300 iterations"
          " each, side 0; lattices over the objects' bounding region).  `query` = one `mon_scene_query_lattice`; `dist+free` = one"
          " `mon_scene_distance_lattice` with free_dist (two plain transforms, today's route to a signed field); `signed` = one"
          " `mon_scene_signed_distance_lattice` in log density; `host values` = `mon_signed_distance_transform` of the same values uploaded from the host."
          "  `seed` = the `k_surface_line_pass` dispatches (3 per signed transform); `plain` = the `k_distance_pass` dispatches (6 per signed transform, 3"
          " per plain one); `small` = `k_distance_mask`, `k_distance_finish`, `k_signed_values`, `k_signed_finish`; `seed / plain` compares one dispatch of"
          " each; `transform / plain transform` = (seed + plain + small) against half of the `dist+free` row's; `share` = the transform's part of the"
          " call's kernel time.  `wall` = host time per repetition under the tracer (copies home included).\n")
    print("| K | what | cells | inside | query kernels | seed | plain | small | other | total | seed / plain (per dispatch) | transform / plain transform | share | wall ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    plain_tr = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); c = cnt.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(d.values()) / r; key = b["n"]
        tr = f("seed") + f("plain") + f("small")
        if b["what"] == "dist+free":
            plain_tr[(b["K"], key)] = tr / 2
        per = "%.2f" % ((d["seed"] / c["seed"]) / (d["plain"] / c["plain"])) if c.get("seed") and c.get("plain") else ""
        base = plain_tr.get((b["K"], key)) or plain_tr.get((1, key))
        ratio = "%.2f" % (tr / base) if base and b["what"] in ("signed", "host values") else ""
        share = "%.3f" % (tr / tot) if tot > 0 and tr > 0 else ""
        print("| %d | %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %s | %s | %.3f |" % (b["K"], b["what"], b["n"], b.get("inside", 0),
              f("query"), f("seed"), f("plain"), f("small"), f("other"), tot, per, ratio, share, b["wall_ms"]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
