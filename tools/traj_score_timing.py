#!/usr/bin/env python
"""Kernel times of the device-resident distance field (mon_scene_dist_field, mon_dist_field_score) beside the kernels of the field's own
creation and beside the parent route for the same answer -- mon_scene_distance_lattice with its copy home plus scipy.ndimage.map_coordinates on the host --
from the same process (runs on the GPU box, under rocprofv3).

    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/traj_score_timing.py run OUT/configs.json [--reps 10] [--steps 300]
    python tools/traj_score_timing.py stats OUT/configs.json OUT/p >> profiles/r22_dist_field.md

`run` trains eight base.json objects of an eight-object synthetic scene (as tools/scene_distance_timing.py), then on side 0, for lattices of 64^3 and 128^3
over the objects' bounding region: `reps` times the field's creation (`create`), the score of 4 096 trajectories x 32 waypoints x n_sub 4 x 8 spheres with
every output (`score`) and with min_clear alone (`score min`), a score of 4 096 x 16 x 4 x 8 (61 samples: the wave kernel, `score short`), the distance call
with dist alone (`dist home`) and, timed on the host only, the same centres interpolated by scipy (`host interp`, order 1, float64).  sigma_min is the
density of opacity 0.5 over one lattice step; max_dist is a quarter of the region's diagonal.  Every block of work starts and ends with a marker dispatch
(mon_debug_scene_composite on 1 + block-number rays).  `stats` splits the trace at the markers and prints per-call kernel milliseconds by kind, the score
against the creation, and k_traj_score against its gather count."""
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
N_TRAJ, N_WAY, N_SUB, N_SPH = 4096, 32, 4, 8


def trajectories(lo, hi, n_way, seed):
    """random walks of n_way waypoints through the region, a fortieth of its diagonal per step, and a body of N_SPH spheres a fiftieth of it in size"""
    rng = np.random.default_rng(seed); diag = float(np.linalg.norm(hi - lo))
    start = lo + rng.random((N_TRAJ, 1, 3)) * (hi - lo)
    ways = (start + np.cumsum(rng.normal(size=(N_TRAJ, n_way, 3)) * diag / 40 / np.sqrt(3), axis=1)).astype(np.float32)
    sph = np.zeros((N_SPH, 4), np.float32)
    sph[:, :3] = rng.normal(size=(N_SPH, 3)) * diag / 50; sph[:, 3] = diag / 100
    return ways, sph


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

    def block(what, n, fn, reps=None, **extra):
        reps = reps or a.reps
        for _ in range(2):                                                   # warm-up (workspace grown)
            fn()
        b = dict(id=marker(), what=what, n=n, reps=reps, **extra)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        b["wall_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 4)
        blocks.append(b); print(json.dumps(b), flush=True)
        blocks.append(dict(id=marker(), what="gap"))                          # (the next block's warm-up belongs to no row)

    sgn = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    cor = np.concatenate([(sgn * ob["half"]) @ ob["Two"][:3, :3].T + ob["Two"][:3, 3] for ob in sc.objects[:8]])
    lo, hi = cor.min(0), cor.max(0); pad = 0.1 * (hi - lo); lo = lo - pad; hi = hi + pad
    max_dist = 0.25 * float(np.linalg.norm(hi - lo))
    ways, sph = trajectories(lo, hi, N_WAY, 1); ways_short, _ = trajectories(lo, hi, 16, 2)
    try:
        from scipy.ndimage import map_coordinates
    except ImportError:
        map_coordinates = None
    import dist_field_reference as dr
    for r in SIZES:
        shape = (r, r, r); origin = lo.astype(np.float32); step = ((hi - lo) / (r - 1)).astype(np.float32)
        smin = float(-np.log(0.5) / float(step.min()))
        kw = dict(n_sub=N_SUB, outside=max_dist, margin=float(step.min()), safe=4 * float(step.min()))
        made = []

        def create():
            made.append(pkg.scene_dist_field(objs, origin, step, shape, smin, max_dist, side=0))
            if len(made) > 1:
                made.pop(0).close()
        block("create", r ** 3, create)
        f = made[-1]
        n_ss = N_TRAJ * ((N_WAY - 1) * N_SUB + 1) * N_SPH
        res = {}
        block("score", r ** 3, lambda: res.update(f.score(sph, ways, **kw)), sphere_samples=n_ss)
        block("score min", r ** 3, lambda: f.score(sph, ways, outputs=(), **kw), sphere_samples=n_ss)
        block("score short", r ** 3, lambda: f.score(sph, ways_short, **kw), sphere_samples=N_TRAJ * (15 * N_SUB + 1) * N_SPH)
        hits = int((res["first_hit"] >= 0).sum())
        dist = {}
        block("dist home", r ** 3, lambda: dist.update(d=pkg.scene_distance_lattice(objs, origin, step, shape, smin, max_dist, side=0, free=False)[0]), hits=hits)
        if map_coordinates is not None:
            c = dr.sample_centres(dr.centres(sph, ways), N_SUB).reshape(-1, 3).astype(np.float64)
            g = (c - origin.astype(np.float64)) / step.astype(np.float64)
            D = dist["d"].reshape(r, r, r).astype(np.float64)
            block("host interp", r ** 3, lambda: map_coordinates(D, [g[:, 2], g[:, 1], g[:, 0]], order=1, mode="constant", cval=max_dist), reps=2, sphere_samples=n_ss)
        f.close()
    blocks.append(dict(id=marker(), what="end"))
    for o in objs:
        o.close()
    ds.close()
    with open(a.configs, "w") as f:
        json.dump(blocks, f, indent=1)


QUERY = ("k_scene_points", "k_scene_points_fold", "k_build_frag_image")
TRANSFORM = ("k_distance_pass", "k_distance_mask", "k_distance_finish")
SCORE = ("k_traj_score",)
EXTRA = ("k_field_max",)


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
        kind = "query" if n in QUERY else "transform" if n in TRANSFORM else "score" if n in SCORE else "max" if n in EXTRA else "other"
        d = acc.setdefault(cur_id, {}); d[kind] = d.get(kind, 0.0) + (e - s) / 1e6
    print("# Device-resident distance fields: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one repetition (`tools/traj_score_timing.py`; 8 base.json objects, 300 iterations each,"
          " side 0; lattices over the objects' bounding region).  `create` = one `mon_scene_dist_field`; `score` = one `mon_dist_field_score` of 4 096"
          " trajectories x 32 waypoints x n_sub 4 (125 samples) x 8 spheres with every output; `score min` = min_clear alone; `score short` = 16 waypoints"
          " (61 samples, the wave kernel); `dist home` = one `mon_scene_distance_lattice` with dist alone; `host interp` = scipy's `map_coordinates`"
          " (order 1, float64) at the same sphere centres, host only.  `query kernels` = `k_scene_points` + fold + fragment images; `transform` = mask,"
          " passes and finish; `max` = `k_field_max`; `other` = the copy kernels.  `wall` = host time per repetition under the tracer.  `G loads/s` ="
          " 4 x sphere-samples (the 8-byte corner loads) over the score kernel's time; `GB/s` = 32 B per sphere-sample over it.\n")
    print("| what | cells | query kernels | transform | max | score | other | total | score / create (kernel) | wall ms | G loads/s | GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    create = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); r = b["reps"]; f = lambda k: d.get(k, 0.0) / r            # noqa: E731
        tot = sum(d.values()) / r
        if b["what"] == "create":
            create[b["n"]] = tot
        ratio = "%.4f" % (tot / create[b["n"]]) if b["what"].startswith("score") and b["n"] in create else ""
        rate = ("%.1f" % (4 * b["sphere_samples"] / f("score") / 1e6), "%.0f" % (32 * b["sphere_samples"] / f("score") / 1e6)) if f("score") > 0 else ("", "")
        print("| %s | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s | %.3f | %s | %s |" % (b["what"], b["n"], f("query"), f("transform"), f("max"), f("score"),
              f("other"), tot, ratio, b["wall_ms"], rate[0], rate[1]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10); r.add_argument("--steps", type=int, default=300)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace")
    a = ap.parse_args()
    if a.mode == "run":
        sys.path.insert(0, os.path.join(ROOT, "tests"))                        # (the host yardstick's sphere centres: tests/dist_field_reference.py)
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
