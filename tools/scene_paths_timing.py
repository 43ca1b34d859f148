#!/usr/bin/env python
"""Kernel times of the shortest-path cost fields (mon_shortest_paths, mon_scene_paths_lattice: k_paths_init, k_paths_seed, k_paths_sweep, k_paths_finish,
k_paths_soft) beside their yardsticks from the same process (runs on the GPU box, under rocprofv3): the three k_distance_pass launches and the components
labelling on the same mask, the kernels of mon_scene_query_lattice on the same lattice, and what a caller pays today: scipy.sparse.csgraph.dijkstra on the
passable graph on the host (the heap reference of tests/paths_reference.py where scipy is missing).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scene_paths_timing.py run OUT/configs.json [--reps 5] [--steps 300]
    python tools/scene_paths_timing.py stats OUT/configs.json OUT/p >> profiles/r21_scene_paths.md
    MON_CORE_LIB=ro-map_amd/build_b8/libmon_core.so python tools/scene_paths_timing.py batch      (a variant build -DMON_PATHS_BATCH=8; no profiler)

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_components_timing.py), then on side 0, for lattices of 64^3 and
128^3 over the objects' bounding region, the goal = the passable cell nearest the lattice's centre: `reps` times the lattice query (`query`), the paths
call at a clearance of two lattice steps without and with the soft multiplier (`scene`, `scene soft`), and on host masks of the same shape -- the scene's
own passable cells (dist > clearance), and the serpentine of tests/components_reference.py -- the standalone field (`paths 6`, `paths 26`, `paths 26 c`
with multipliers), the standalone distance transform (`distance`) and labelling (`label 26`).  Every block of work starts and ends with a marker dispatch
(mon_debug_scene_composite on 1 + block-number rays).  `stats` splits the trace at the markers and prints per-call kernel milliseconds by kernel.
`batch` prints host milliseconds per standalone call for the library in use, with the sweeps and batches it took."""
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


def host_dijkstra(mask, seed, step):
    """what a caller runs today: the 6-connected passable graph in fp64 through scipy (graph build included), or the heap reference; -> (ms, name)"""
    t0 = time.perf_counter()
    try:
        from scipy import sparse as sp
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        import paths_reference as pr
        pr.dijkstra(mask, [seed], step, 6)
        return (time.perf_counter() - t0) * 1e3, "heap reference 6"
    on = mask.reshape(-1) != 0; idx = np.arange(mask.size).reshape(mask.shape); rows, cols, w = [], [], []
    for ax, st in ((2, step[0]), (1, step[1]), (0, step[2])):
        a = np.moveaxis(idx, ax, 0)[:-1].reshape(-1); b = np.moveaxis(idx, ax, 0)[1:].reshape(-1); ok = on[a] & on[b]
        rows.append(a[ok]); cols.append(b[ok]); w.append(np.full(int(ok.sum()), float(st)))
    g = sp.csr_matrix((np.concatenate(w), (np.concatenate(rows), np.concatenate(cols))), shape=(mask.size, mask.size))
    dijkstra(g, directed=False, indices=[seed], min_only=True)
    return (time.perf_counter() - t0) * 1e3, "scipy dijkstra 6"


def run(a):
    import __graft_entry__ as ge
    import components_reference as cr
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

    def block(what, mask, n, fn, paths=False, **extra):
        for _ in range(2):                                                   # warm-up (workspace grown)
            fn()
        b = dict(id=marker(), what=what, mask=mask, n=n, reps=a.reps, **extra)
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        b["wall_ms"] = round((time.perf_counter() - t0) * 1e3 / a.reps, 4)
        if paths:
            b["sweeps"], b["batches"], b["busy"] = pkg.paths_stats()
        blocks.append(b); print(json.dumps(b), flush=True)
        blocks.append(dict(id=marker(), what="gap"))                          # (the next block's warm-up belongs to no row)

    sgn = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    cor = np.concatenate([(sgn * ob["half"]) @ ob["Two"][:3, :3].T + ob["Two"][:3, 3] for ob in sc.objects[:8]])
    lo, hi = cor.min(0), cor.max(0); pad = 0.1 * (hi - lo); lo = lo - pad; hi = hi + pad
    for r in SIZES:
        shape = (r, r, r); origin = lo.astype(np.float32); step = ((hi - lo) / (r - 1)).astype(np.float32); n = r ** 3
        smin = float(-np.log(0.5) / float(step.min())); clearance = 2.0 * float(step.max()); radius = 4.0 * clearance
        dist = pkg.scene_distance_lattice(objs, origin, step, shape, smin, side=0, free=False)[0]
        scene_mask = (dist > np.float32(clearance)).reshape(r, r, r).astype(np.uint8)
        k, j, i = np.nonzero(scene_mask); goal_at = int(np.argmin((i - r / 2) ** 2 + (j - r / 2) ** 2 + (k - r / 2) ** 2))
        goal = int((k[goal_at] * r + j[goal_at]) * r + i[goal_at])
        rng = np.random.default_rng(r); mult = (1 + 4 * rng.random(scene_mask.shape)).astype(np.float32)
        block("query", "scene", n, lambda: pkg.query_scene_lattice(objs, origin, step, shape, 0), cells=int(scene_mask.sum()))
        for name, sw in (("scene", 0.0), ("scene soft", 2.0)):
            got = pkg.scene_paths_lattice(objs, origin, step, shape, smin, [goal], clearance, radius, sw, 26, side=0)
            block(name, "scene", n, lambda: pkg.scene_paths_lattice(objs, origin, step, shape, smin, [goal], clearance, radius, sw, 26, side=0), paths=True,
                  cells=int(scene_mask.sum()), reached=int(np.isfinite(got[0]).sum()))
        block("components r1", "scene", n, lambda: pkg.scene_components_lattice(objs, origin, step, shape, smin, 1, clearance, 26, side=0, cap=1024),
              cells=int(scene_mask.sum()))
        for mname, m, seed in (("scene", scene_mask, goal), ("serpentine", cr.serpentine(shape), 0)):
            for what, conn, c in (("paths 6", 6, None), ("paths 26", 26, None), ("paths 26 c", 26, mult)):
                got = pkg.shortest_paths(m, [seed], step, conn, c)
                block(what, mname, n, lambda: pkg.shortest_paths(m, [seed], step, conn, c), paths=True, cells=int(m.sum()),
                      reached=int(np.isfinite(got[0]).sum()))
            block("distance", mname, n, lambda: pkg.distance_transform(m == 0, step), cells=int(m.sum()))
            block("label 26", mname, n, lambda: pkg.label_components(m, 26, cap=1024), cells=int(m.sum()))
            ms, hname = host_dijkstra(m, seed, step)
            blocks.append(dict(id=marker(), what=hname, mask=mname, n=n, reps=1, cells=int(m.sum()), wall_ms=round(ms, 3)))
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
PT = ("k_paths_init", "k_paths_seed", "k_paths_soft", "k_paths_sweep", "k_paths_finish")


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
        kind = "query" if n in QUERY else "passes" if n in PASSES else "labelling" if n in CC else n if n in PT else "other"
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("### Shortest-path cost fields beside the distance passes, the labelling and the lattice query: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/scene_paths_timing.py`; 8 base.json objects, 300 iterations"
          " each, side 0; lattices over the objects' bounding region; one seed).  `sweeps` = `k_paths_sweep` launches enqueued, `busy` = those that left"
          " work for the next, `batches` = read-backs.  `field` = init + seed + soft + sweep + finish.  `wall` = host time per repetition under the"
          " tracer; the host rows are wall time only.\n")
    print("| what | mask | cells | passable | reached | sweeps | busy | batches | query | passes | labelling | init+seed+soft | sweep | finish | field | other |"
          " wall ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        host = "dijkstra" in b["what"] or "reference" in b["what"]
        d = {} if host else acc.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        pre = f("k_paths_init") + f("k_paths_seed") + f("k_paths_soft"); field = pre + f("k_paths_sweep") + f("k_paths_finish")
        print("| %s | %s | %d | %d | %s | %s | %s | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
              b["what"], b["mask"], b["n"], b.get("cells", 0), b.get("reached", ""), b.get("sweeps", ""), b.get("busy", ""), b.get("batches", ""),
              f("query"), f("passes"), f("labelling"), pre, f("k_paths_sweep"), f("k_paths_finish"), field, f("other"), b["wall_ms"]))


def batch(a):
    import __graft_entry__ as ge
    import components_reference as cr
    import paths_reference as pr
    pkg = ge.load_package()
    step = np.array([0.05, 0.05, 0.05], np.float32)
    for r in SIZES:
        shape = (r, r, r)
        for name, m in (("random 69 %", pr.random_mask(shape, 0.69, seed=r)), ("open", np.ones((r, r, r), np.uint8)), ("serpentine", cr.serpentine(shape))):
            seed = int(np.flatnonzero(m.reshape(-1))[0])
            for conn in (6, 26):
                for _ in range(2):
                    pkg.shortest_paths(m, [seed], step, conn)
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    pkg.shortest_paths(m, [seed], step, conn)
                ms = (time.perf_counter() - t0) * 1e3 / a.reps
                sweeps, batches, busy = pkg.paths_stats()
                print(json.dumps(dict(lib=os.path.basename(os.path.dirname(pkg.lib_path())), mask=name, n=r ** 3, conn=conn, wall_ms=round(ms, 3), sweeps=sweeps,
                                      batches=batches, busy=busy)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=5); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    b = sub.add_parser("batch"); b.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    {"run": run, "stats": stats, "batch": batch}[a.mode](a)


if __name__ == "__main__":
    main()
