#!/usr/bin/env python
"""Times of scan matching against a device-resident distance field (mon_dist_field_match, mon_dist_field_register) beside the route a
user had before them -- mon_dist_field_sample with gradients plus the normal equations in numpy on the host -- from the same process (runs on the GPU box).

    python tools/scan_match_timing.py run OUT/wall.json [--reps 20]                                                     # host wall times
    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/scan_match_timing.py run OUT/configs.json [--reps 20]
    python tools/scan_match_timing.py stats OUT/configs.json OUT/p [OUT/wall.json] >> profiles/r23_scan_match.md

`run` needs no trained object: the field is the analytic signed distance of tests/scan_match_reference.py (two boxes and a sphere) sampled on 64^3 and 128^3
lattices over [0, 2.3]^3, the scan 2 048 points on its zero set in a body frame.  Per lattice, `reps` times each: `match H` for H = 1, 256 and 4 096 poses
(the known pose moved by up to 0.05 rad and half a cell) with the normal equations, `match lite 4096` without them, `register 8` (eight starts 0.15 rad and
one 0.1 step away, default parameters), and `host route H` for H = 1 and 16: per pose the posed points in numpy, one mon_dist_field_sample with gradients
and the 27 sums in numpy float64.  Then, on 64^3 only, `register 8` against fields made from the binary mask D < 0 by mon_distance_transform (unsigned, and
signed as dist - free distance): the cell-quantised case, whose errors are printed.  Every block starts and ends with a marker dispatch (mon_dist_field_sample
on 256 x (1000 + block number) points: k_field_sample with that many workgroups).  `stats` splits the trace at the markers and prints kernel milliseconds per
call by kernel, with the host wall time per call of both runs."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                                    # (the analytic field, the scan and the error measure)

SIZES = (64, 128)
N, EXTENT, MARK = 2048, 2.3, 1000


def host_route(f, pts64, poses, pivots, huber):
    """what a user did per pose before mon_dist_field_match: pose the points on the host, sample d and grad, form the 27 sums in numpy"""
    out = []
    for T, c in zip(poses.reshape(-1, 4, 4).astype(np.float64), pivots.astype(np.float64)):
        q = pts64 @ T[:3, :3].T + T[:3, 3]
        d, g = f.sample(q.astype(np.float32), outside=0.0)
        d = d.astype(np.float64); g = g.astype(np.float64)
        J = np.concatenate([g, np.cross(q - c, g)], 1)
        m = np.abs(d); w = np.where(m <= huber, 1.0, huber / np.maximum(m, 1e-30))
        out.append(((J * w[:, None]).T @ J, (J * (w * d)[:, None]).sum(0)))
    return out


def run(a):
    import __graft_entry__ as ge
    import scan_match_reference as sm
    pkg = ge.load_package()
    blocks = []
    probe = pkg.dist_field_create(np.zeros((2, 2, 2), np.float32), np.zeros(3), np.ones(3))

    def marker():
        n = MARK + len(blocks) + 1
        probe.sample(np.zeros((256 * n, 3), np.float32), grad=False)
        return n

    def block(what, cells, fn, reps=None, **extra):
        reps = reps or a.reps
        for _ in range(2):                                                   # warm-up (buffers grown)
            fn()
        b = dict(id=marker(), what=what, cells=cells, reps=reps, **extra)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        b["wall_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 4)
        blocks.append(b); print(json.dumps(b), flush=True)
        blocks.append(dict(id=marker(), what="gap"))                          # (the next block's warm-up belongs to no row)

    def errors(case, res):
        e = np.array([sm.pose_errors(T, case["pose"], case["centroid"]) for T in res["poses"]])
        return dict(rad_worst=float(e[:, 0].max()), cell_worst=float(e[:, 1].max() / float(case["step"][0])), status=res["status"].tolist(),
                    evals=res["evals"].tolist())

    rng = np.random.default_rng(0)
    for r in SIZES:
        cell = EXTENT / (r - 1)
        case = sm.recovery_case(shape=(r, r, r), cell=cell, n=N, seed=11)
        D, o, s, pts, G = case["D"], case["origin"], case["step"], case["points"], case["pose"].astype(np.float64)
        cw = G[:3, :3] @ case["centroid"] + G[:3, 3]
        # the recovery starts are a tenth of a unit away whatever the lattice: the same basin on both
        starts = np.stack([sm.twist_pose(G, cw, np.concatenate([0.1 * v / np.linalg.norm(v), 0.15 * w / np.linalg.norm(w)])).astype(np.float32)
                           for v, w in zip(rng.normal(size=(8, 3)), rng.normal(size=(8, 3)))])
        f = pkg.dist_field_create(D, o, s)
        prm = f.register_default()
        for H in (1, 256, 4096):
            poses = np.stack([sm.twist_pose(G, cw, np.concatenate([rng.uniform(-0.5, 0.5, 3) * cell, rng.uniform(-0.05, 0.05, 3)])).astype(np.float32)
                              for _ in range(H)])
            piv = np.tile(cw.astype(np.float32), (H, 1))
            block("match %d" % H, r ** 3, lambda: f.match(pts, poses, piv, huber=prm.huber, outside=prm.outside), pairs=N * H)
            if H == 4096:
                block("match lite 4096", r ** 3, lambda: f.match(pts, poses, piv, huber=prm.huber, outside=prm.outside, normal=False), pairs=N * H)
        res = {}
        block("register 8", r ** 3, lambda: res.update(f.register(pts, starts)))
        blocks[-2].update(errors(case, res)); print(json.dumps(blocks[-2]), flush=True)
        pts64 = pts.astype(np.float64)
        for H in (1, 16):
            piv = np.tile(cw.astype(np.float32), (H, 1))
            block("host route %d" % H, r ** 3, lambda: host_route(f, pts64, starts[np.arange(H) % 8], piv, float(prm.huber)), reps=max(2, a.reps // 4), pairs=N * H)
        f.close()
        if r == SIZES[0]:
            # the cell-quantised case: a field made from the binary mask D < 0
            occ = D < 0
            dist = pkg.distance_transform(occ, s, nearest=False)[0]; free = pkg.distance_transform(~occ, s, nearest=False)[0]
            for name, Dq in (("unsigned mask field", dist), ("signed mask field", dist - free)):
                with pkg.dist_field_create(Dq, o, s) as fq:
                    res = {}
                    block("register 8, " + name, r ** 3, lambda: res.update(fq.register(pts, starts)))
                    blocks[-2].update(errors(case, res)); print(json.dumps(blocks[-2]), flush=True)
    blocks.append(dict(id=marker(), what="end"))
    probe.close()
    with open(a.configs, "w") as fh:
        json.dump(blocks, fh, indent=1)


def short(name):
    n = name.split("(")[0]
    for k in ("k_scan_match<true>", "k_scan_match<false>", "k_scan_match", "k_scan_fold", "k_field_sample"):
        if k.replace("<true>", "ILb1").replace("<false>", "ILb0") in n or k in n:
            return k
    return "other"


def stats(a):
    blocks = {b["id"]: b for b in json.load(open(a.configs))}
    wall = {b["id"]: b for b in json.load(open(a.wall))} if a.wall else {}
    rows = []
    for p in sorted(glob.glob(os.path.join(a.trace, "**", "*_results.db"), recursive=True)):
        cur = sqlite3.connect(p).cursor()
        rows += list(cur.execute("select name, start, end, grid_x, workgroup_x from kernels order by start"))
    rows.sort(key=lambda r: r[1])
    acc = {}; cnt = {}; cur_id = None
    for name, s, e, gx, wx in rows:
        n = short(name); blocks_n = gx // max(1, wx)
        if n == "k_field_sample" and blocks_n in blocks:
            cur_id = blocks_n; continue
        if cur_id is None:
            continue
        d = acc.setdefault(cur_id, {}); d[n] = d.get(n, 0.0) + (e - s) / 1e6
        c = cnt.setdefault(cur_id, {}); c[n] = c.get(n, 0) + 1
    print("# Scan matching: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one call (`tools/scan_match_timing.py`; the analytic signed distance field on a lattice"
          " over [0, 2.3]^3, a scan of 2 048 points).  `match H` = one `mon_dist_field_match` of H poses with the normal equations, `match lite` without;"
          " `register 8` = one `mon_dist_field_register` of eight starts (the launches column counts its rounds); `host route H` = per pose one"
          " `mon_dist_field_sample` with gradients and the sums in numpy.  `wall (traced)` = host ms per call under the tracer, `wall` = the same in a run"
          " without it.  `G pairs/s` = point-pose pairs over the match kernel's time.\n")
    print("| what | cells | k_scan_match | k_scan_fold | k_field_sample | other | kernels total | match launches | wall (traced) ms | wall ms | G pairs/s |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] in ("end", "gap"):
            continue
        d = acc.get(i, {}); c = cnt.get(i, {}); r = b["reps"]
        km = (d.get("k_scan_match<true>", 0.0) + d.get("k_scan_match<false>", 0.0) + d.get("k_scan_match", 0.0)) / r
        nm = (c.get("k_scan_match<true>", 0) + c.get("k_scan_match<false>", 0) + c.get("k_scan_match", 0)) / r
        rate = "%.2f" % (b["pairs"] / km / 1e6) if km > 0 and "pairs" in b and b["what"].startswith("match") else ""
        w = wall.get(i, {}).get("wall_ms")
        print("| %s | %d | %.4f | %.4f | %.4f | %.4f | %.4f | %.1f | %.3f | %s | %s |" % (b["what"], b["cells"], km, d.get("k_scan_fold", 0.0) / r,
              d.get("k_field_sample", 0.0) / r, d.get("other", 0.0) / r, sum(d.values()) / r, nm, b["wall_ms"], "%.3f" % w if w is not None else "", rate))
    print("\nRecovery on these fields (worst of the eight starts; each start 0.15 rad and 0.1 away):\n")
    print("| what | cells | worst rotation error, rad | worst centroid error, cells | status | evaluations |")
    print("|---|---|---|---|---|---|")
    for i in sorted(blocks):
        b = blocks[i]
        if "rad_worst" in b:
            print("| %s | %d | %.3g | %.3g | %s | %s |" % (b["what"], b["cells"], b["rad_worst"], b["cell_worst"], b["status"], b["evals"]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=20)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace"); s.add_argument("wall", nargs="?")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
