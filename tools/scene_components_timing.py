#!/usr/bin/env python
"""Kernel times of the connected components (mon_label_components, mon_scene_components_lattice: k_cc_local, k_cc_merge, k_cc_flatten, k_cc_scan,
k_cc_number, k_cc_table) beside their yardsticks from the same process (runs on the GPU box, under rocprofv3): the three k_distance_pass launches of
mon_distance_transform on the same mask, the kernels of mon_scene_query_lattice on the same lattice, and -- where scipy is importable -- what a caller
pays today: the lattice query with its copy home plus scipy.ndimage.label on the host.

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_components_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/scene_components_timing.py stats OUT/configs.json OUT/p >> profiles/r19_scene_components.md

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_distance_timing.py), then on side 0, for lattices of 64^3 and
128^3 over the objects' bounding region: `reps` times the lattice query (`query`), the components call on region 0 and on region 1 at a clearance of
two lattice steps (`scene r0`, `scene r1`), and, on host masks of the same shape -- the scene's own (!(sigma <= sigma_min), sigma_min the density of
opacity 0.5 over one lattice step), a random one of 31 % and the serpentine of tests/components_reference.py -- the standalone labelling under 6 and 26
(`label 6`, `label 26`) and the standalone distance transform (`distance`).  Every block of work starts and ends with a marker dispatch
(mon_debug_scene_composite on 1 + block-number rays).  `stats` splits the trace at the markers and prints per-call kernel milliseconds by kernel."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from scene_points_timing import short       # noqa: E402

SIZES = (64, 128)


def run(a):
    import __graft_entry__ as ge
    import components_reference as cr
    pkg = ge.load_package(); ss = ge.load_tools()
    try:
        from scipy import ndimage as ndi
    except ImportError:
        ndi = None
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

    def block(what, mask, n, fn, **extra):
        for _ in range(2):                                                   # warm-up (workspace grown)
            fn()
        b = dict(id=marker(), what=what, mask=mask, n=n, reps=a.reps, **extra)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        b["wall_ms"] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
        blocks.append(b); print(json.dumps(b), flush=True)
        blocks.append(dict(id=marker(), what="gap"))                          # (the next block's warm-up belongs to no row)

    sgn = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    cor = np.concatenate([(sgn * ob["half"]) @ ob["Two"][:3, :3].T + ob["Two"][:3, 3] for ob in sc.objects[:8]])
    lo, hi = cor.min(0), cor.max(0); pad = 0.1 * (hi - lo); lo = lo - pad; hi = hi + pad
    for r in SIZES:
        shape = (r, r, r); origin = lo.astype(np.float32); step = ((hi - lo) / (r - 1)).astype(np.float32)
        smin = float(-np.log(0.5) / float(step.min())); clearance = 2.0 * float(step.max())
        sigma = pkg.query_scene_lattice(objs, origin, step, shape, 0)[0]
        masks = (("scene", (~(sigma <= np.float32(smin))).reshape(r, r, r).astype(np.uint8)),
                 ("random 31 %", cr.random_mask(shape, 0.31, seed=r)), ("serpentine", cr.serpentine(shape)))
        block("query", "scene", r ** 3, lambda: pkg.query_scene_lattice(objs, origin, step, shape, 0), cells=int(masks[0][1].sum()))
        for region in (0, 1):
            got = pkg.scene_components_lattice(objs, origin, step, shape, smin, region, clearance, 6, side=0, cap=1024)
            block("scene r%d" % region, "scene", r ** 3,
                  lambda: pkg.scene_components_lattice(objs, origin, step, shape, smin, region, clearance, 6, side=0, cap=1024),
                  cells=int((got[0] >= 0).sum()), components=got[3])
        for name, m in masks:
            for conn in (6, 26):
                n_comp = pkg.label_components(m, conn, cap=1024)[3]
                block("label %d" % conn, name, r ** 3, lambda: pkg.label_components(m, conn, cap=1024), cells=int(m.sum()), components=n_comp)
            block("distance", name, r ** 3, lambda: pkg.distance_transform(m, step), cells=int(m.sum()))
            if ndi is not None:
                t0 = time.perf_counter()
                for _ in range(3):
                    ndi.label(m)
                blocks.append(dict(id=marker(), what="scipy label 6", mask=name, n=r ** 3, reps=1, cells=int(m.sum()),
                                   wall_ms=round((time.perf_counter() - t0) * 1e3 / 3, 4)))
                print(json.dumps(blocks[-1]), flush=True)
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


QUERY = ("k_scene_points", "k_scene_points_fold", "k_build_frag_image")
PASSES = ("k_distance_pass",)
CC = ("k_cc_local", "k_cc_merge", "k_cc_flatten", "k_cc_scan", "k_cc_number", "k_cc_table")


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
        kind = "query" if n in QUERY else "passes" if n in PASSES else n if n in CC else "other"
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Connected components beside the distance passes and the lattice query: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/scene_components_timing.py`; 8 base.json objects, 300"
          " iterations each, side 0; lattices over the objects' bounding region).  `query` = one `mon_scene_query_lattice`; `scene r0` / `scene r1` = one"
          " `mon_scene_components_lattice` on region 0 / on region 1 at a clearance of two steps (6-connectivity, cap 1 024); `label 6` / `label 26` = one"
          " `mon_label_components` of a host mask; `distance` = one `mon_distance_transform` of the same mask (its `passes` are the yardstick);"
          " `scipy label 6` = `scipy.ndimage.label` on the host (wall only; a caller today pays it on top of `query`'s wall).  `labelling` = the six"
          " `k_cc_*` columns summed; `other` = masks, finish, copies.  `wall` = host time per repetition under the tracer.\n")
    print("| what | mask | cells | in mask | components | query | passes | local | merge | flatten | scan | number | table | labelling | other |"
          " labelling / passes | wall ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    passes = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] == "distance":
            passes[(b["mask"], b["n"])] = acc.get(i, {}).get("passes", 0.0) / b["reps"]
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}) if b["what"] != "scipy label 6" else {}; r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        lab = sum(f(k) for k in CC); ps = passes.get((b["mask"], b["n"]), 0.0)
        ratio = "%.3f" % (lab / ps) if lab > 0 and ps > 0 else ""
        print("| %s | %s | %d | %d | %s | %.3f | %.3f | %s | %.3f | %.3f | %s | %.3f |" % (
              b["what"], b["mask"], b["n"], b.get("cells", 0), b.get("components", ""), f("query"), f("passes"),
              " | ".join("%.3f" % f(k) for k in CC), lab, f("other"), ratio, b["wall_ms"]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
