#!/usr/bin/env python
"""Times of ray tracing against a device-resident distance field (mon_dist_field_trace, mon_dist_field_beam_score) beside the route a
user had before them -- one mon_dist_field_sample per march step from a host loop -- from the same process (runs on the GPU box).

    python tools/field_trace_timing.py run OUT/wall.json [--reps 10]                                                     # host wall times
    rocprofv3 --kernel-trace --stats -d OUT/p -o t -- python tools/field_trace_timing.py run OUT/configs.json [--reps 10]
    python tools/field_trace_timing.py stats OUT/configs.json OUT/p [OUT/wall.json] >> profiles/r25_field_trace.md

`run` needs no trained object (so mon_scene_cast, which marches objects, has nothing to be asked here): the field is the analytic signed distance of
tests/scan_match_reference.py (two boxes and a sphere) sampled on 64^3 and 128^3 lattices over [0, 2.3]^3, the scans 360 x 16 and 1 024 x 64 beams from a
sensor pose in free space, default parameters.  Per lattice and scan, three times over (the repeats of the spread), `reps` calls each: `trace H` and
`beam H` for H = 1, 256 and 4 096 poses (the sensor pose moved by up to 0.05 rad and half a cell) where n * H is within the call's limit; once per lattice
and scan `host loop`: the same march for the same rays of one pose with one mon_dist_field_sample per step.  steps[H][n] of the first call of a block gives
the total steps and the lane utilisation, sum(steps) / (64 * sum over waves of max steps).  Every block starts and ends with a marker dispatch
(mon_dist_field_sample on 256 x (1000 + block number) points: k_field_sample with that many workgroups).  `stats` splits the trace at the markers and prints
kernel milliseconds per call by kernel with the spread over the three repeats, the host wall time per call of both runs, and the march kernel's time
beside its gather count: total steps x four 8-byte loads."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                                    # (the analytic field and the rule's reference)

SIZES = (64, 128)
SCANS = ((360, 16), (1024, 64))
POSES = (1, 256, 4096)
EXTENT, MARK, REPEATS = 2.3, 1000, 3
TRACE_MAX, BEAM_MAX = 1 << 22, 1 << 24


def host_loop(f, rays, pose, prm):
    """what a user did before mon_dist_field_trace: the rule's march with one mon_dist_field_sample per step (the points formed in numpy)"""
    import field_trace_reference as ft
    a, w = ft.world_rays(rays, pose.reshape(1, 16))
    inside_of = lambda p: f.sample(p, outside=np.inf, grad=False)[0]                # noqa: E731 -- a sample outside comes back as +inf
    calls = [0]

    def sample(p):
        calls[0] += 1
        d = inside_of(p)
        return np.where(np.isfinite(d), d, 0).astype(np.float32), np.isfinite(d)

    rng, status, k, _ = ft.march(sample, a[0], w[0], prm)
    return rng, status, k, calls[0]


def run(a):
    import __graft_entry__ as ge
    import dist_field_reference as dr
    import field_trace_reference as ft
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

    rng = np.random.default_rng(0)
    G = np.eye(4); G[:3, :3] = dr.rotation((0.2, -0.4, 0.9), 0.4); G[:3, 3] = ft.SENSORS[0]
    for r in SIZES:
        cell = EXTENT / (r - 1)
        D, o, s = ft.analytic_field((r, r, r), cell)
        f = pkg.dist_field_create(D, o, s)
        prm = f.trace_default()
        for n_az, n_el in SCANS:
            u = ft.scan_directions(n_az, n_el); rays = np.concatenate([np.zeros_like(u), u], 1); n = rays.shape[0]
            for H in POSES:
                poses = np.stack([sm.twist_pose(G, G[:3, 3], np.concatenate([rng.uniform(-0.5, 0.5, 3) * cell, rng.uniform(-0.05, 0.05, 3)])).astype(np.float32)
                                  for _ in range(H)])
                poses[0] = G.astype(np.float32)
                if n * H <= BEAM_MAX:
                    z = f.trace(rays, poses[:1], prm, status=False, steps=False)["range"][0]
                for rep in range(REPEATS):
                    if n * H <= TRACE_MAX:
                        st = f.trace(rays, poses, prm)
                        extra = dict(beams=n, poses=H, repeat=rep, steps=int(st["steps"].sum()), utilisation=round(ft.utilisation(st["steps"]), 4),
                                     hits=int((st["status"] == 0).sum()))
                        block("trace", r ** 3, lambda: f.trace(rays, poses, prm, status=False, steps=False), **extra)
                    if n * H <= BEAM_MAX:
                        block("beam", r ** 3, lambda: f.beam_score(rays, z, poses, prm, huber=2 * cell), beams=n, poses=H, repeat=rep)
            res = []
            block("host loop", r ** 3, lambda: res.append(host_loop(f, rays, poses[0], {k: getattr(prm, k) for k in ft.FIELDS})), reps=2, beams=n, poses=1,
                  repeat=0)
            blocks[-2].update(sample_calls=res[-1][3], steps=int(res[-1][2].sum())); print(json.dumps(blocks[-2]), flush=True)
        f.close()
    blocks.append(dict(id=marker(), what="end"))
    probe.close()
    with open(a.configs, "w") as fh:
        json.dump(blocks, fh, indent=1)


def short(name):
    n = name.split("(")[0]
    for k in ("k_field_trace", "k_beam_terms", "k_scan_fold", "k_field_sample"):
        if k in n:
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
    acc = {}; cur_id = None
    for name, s, e, gx, wx in rows:
        n = short(name); blocks_n = gx // max(1, wx)
        if n == "k_field_sample" and blocks_n in blocks:
            cur_id = blocks_n; continue
        if cur_id is None:
            continue
        d = acc.setdefault(cur_id, {}); d[n] = d.get(n, 0.0) + (e - s) / 1e6
    groups = {}
    for i in sorted(blocks):
        b = blocks[i]
        if b["what"] not in ("end", "gap"):
            groups.setdefault((b["cells"], b["beams"], b["what"], b["poses"]), []).append(i)
    print("# Ray tracing against a distance field: kernel times (`rocprofv3 --kernel-trace`, MI355X)\n")
    print("Per row, ms of kernel time summed over the dispatches of one call (`tools/field_trace_timing.py`; the analytic signed distance field on a lattice"
          " over [0, 2.3]^3, default parameters), the median of three repeats of `reps` calls each with the spread (largest - smallest) of the march kernel"
          " over the repeats.  `trace` = one `mon_dist_field_trace` (range only), `beam` = one `mon_dist_field_beam_score`, `host loop` = the same march for"
          " one pose with one `mon_dist_field_sample` per step.  `wall (traced)` = host ms per call under the tracer, `wall` = the same in a run without it. "
          " `G steps/s` = march steps over the march kernel's time; `GB/s gathered` = steps x four 8-byte loads over the same time.\n")
    print("| what | cells | beams | poses | k_field_trace | spread | k_beam_terms | k_scan_fold | k_field_sample | wall (traced) ms | wall ms | steps |"
          " utilisation | G steps/s | GB/s gathered |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for (cells, beams, what, poses), ids in groups.items():
        per = lambda k: sorted(acc.get(i, {}).get(k, 0.0) / blocks[i]["reps"] for i in ids)      # noqa: E731
        med = lambda v: v[len(v) // 2]                                                           # noqa: E731
        kt = per("k_field_trace"); b = blocks[ids[0]]
        w = [wall[i]["wall_ms"] for i in ids if i in wall]
        steps = b.get("steps"); rate = steps / med(kt) / 1e6 if steps and med(kt) > 0 else None
        print("| %s | %d | %d | %d | %.4f | %.4f | %.4f | %.4f | %.4f | %.3f | %s | %s | %s | %s | %s |" % (
            what, cells, beams, poses, med(kt), kt[-1] - kt[0], med(per("k_beam_terms")), med(per("k_scan_fold")), med(per("k_field_sample")),
            med(sorted(blocks[i]["wall_ms"] for i in ids)), "%.3f" % med(sorted(w)) if w else "", steps if steps else "", b.get("utilisation", ""),
            "%.2f" % rate if rate else "", "%.1f" % (rate * 32) if rate else ""))
    print("\nThe host loop made %s sample calls per scan (one per step of its slowest ray)." % ", ".join(
        str(blocks[i]["sample_calls"]) for i in sorted(blocks) if "sample_calls" in blocks[i]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run"); r.add_argument("configs"); r.add_argument("--reps", type=int, default=10)
    s = sub.add_parser("stats"); s.add_argument("configs"); s.add_argument("trace"); s.add_argument("wall", nargs="?")
    a = ap.parse_args()
    run(a) if a.mode == "run" else stats(a)


if __name__ == "__main__":
    main()
