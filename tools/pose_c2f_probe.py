#!/usr/bin/env python
"""Coarse-to-fine pose refinement on base.json objects (mon_object_pose_loss_levels, mon_object_refine_pose_c2f): what chose mon_pose_c2f_default
(runs on an MI355X; DESIGN.md 3.4e, profiles/r09_pose_c2f.md).

    python tools/pose_c2f_probe.py [--out pose_c2f_probe.jsonl] [--train 500,2000] [--no-sweep] [--no-timing]

On the synthetic scene of the pose tests (24 views of 240 x 320, one object), a base.json object (16 levels, 64 x 1, sample_seed 5, depth on) trained
`train` iterations on the true pose, 6 boxes, rays_per_iter 4096 of evaluation key 0:
  1. "levels": grad6 of each level alone (L one-hot pose_loss_levels calls) at the true pose and at 5 degrees / 5 % of the box diagonal off;
  2. "cosine": for alpha = 1..16 (levels 0..alpha-1 weighted 1, the rest 0), the cosine between grad6(w(alpha)) and a central difference of the loss in the
     six twist directions (Tow <- exp(+-h e_j^) Tow), h = 1e-3 and 1e-2; alpha = 16 is the plain gradient;
  3. "sweep": refine_pose_c2f for level_start in {2, 3, 4, 5}, level_end in {4, 5, 6, 7, 8, 10, 12, 16} (>= level_start), ramp in {0.5, 0.7, 1.0},
     and the prior (4, 8, 0.6); 100 and 200 steps, from three seeds
     of 5 degrees / 5 %, one of 15 degrees / 10 % and the true pose; plain refine_pose from the same starts;
  4. "timing": the cost of a c2f step against a plain one at 1 024 / 4 096 / 16 384 rays (100-step calls minus a 0-step call, best of 5).
One JSON line per record into --out; a summary on stdout."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _so3(phi):
    th = np.linalg.norm(phi); K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1 - math.cos(th)) / th ** 2 * K @ K


def _se3(xi):
    """exp(xi^), xi = (rho, phi)"""
    rho, phi = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(phi); K = np.array([[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]])
    if th < 1e-12:
        V = np.eye(3) + 0.5 * K
    else:
        V = np.eye(3) + (1 - math.cos(th)) / th ** 2 * K + (th - math.sin(th)) / th ** 3 * K @ K
    D = np.eye(4); D[:3, :3] = _so3(phi); D[:3, 3] = V @ rho
    return D


def perturb(T, rot_deg, trans, seed):
    """the pose tests' perturbation: a random axis and direction, rotation rot_deg, displacement trans"""
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    D = np.eye(4); D[:3, :3] = _so3(ax * math.radians(rot_deg)); D[:3, 3] = d * trans
    return D @ T


def pose_errors(Tow, Tow_true):
    R = Tow[:3, :3] @ Tow_true[:3, :3].T
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2))))
    c = -Tow[:3, :3].T @ Tow[:3, 3]; c0 = -Tow_true[:3, :3].T @ Tow_true[:3, 3]
    return ang, float(np.linalg.norm(c - c0))


def _mat(T16):
    return np.asarray(T16, np.float64).reshape(4, 4).T


def _cos(a, b):
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    return float(np.dot(a, b) / (na * nb)) if na > 0 and nb > 0 else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="pose_c2f_probe.jsonl")
    ap.add_argument("--train", default="500,2000")
    ap.add_argument("--no-sweep", action="store_true"); ap.add_argument("--no-timing", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fout = open(a.out, "w")

    def emit(rec):
        fout.write(json.dumps(rec) + "\n"); fout.flush()

    sc = ss.make_scene(n_views=24, H=240, W=320, f=260.0, seed=3)
    ob = sc.objects[0]; b = ob["boxes"]; boxes = b[np.linspace(0, len(b) - 1, 6).astype(int)]
    diag = float(np.linalg.norm(2 * ob["half"])); Ttrue = ob["Tow"]
    prm = pkg.pose_refine_default()
    ds = None
    for steps in (int(v) for v in a.train.split(",")):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=5), use_depth=True, dataset=ds)
        o.set_backend(1); o.train(steps)
        L = o.cfg.n_levels
        t_start = time.time()
        # ---- 1. / 2. per-level split and cosine to the central difference
        for pname, T in (("true", Ttrue), ("5deg5pct", perturb(Ttrue, 5.0, 0.05 * diag, 1))):
            T16 = ss.colmajor(T)
            lv = []
            for l in range(L):
                e = np.zeros(L, np.float32); e[l] = 1
                lv.append(o.pose_loss_levels(boxes, T16, e, prm)[1].astype(np.float64))
            lv = np.array(lv)
            loss0, gfull = o.pose_loss(boxes, T16, prm)
            emit(dict(kind="levels", train=steps, pose=pname, loss=loss0, grad6_by_level=lv.tolist(), grad6=gfull.tolist()))
            fds = {}
            for h in (1e-3, 1e-2):
                fd = np.zeros(6)
                for j in range(6):
                    xi = np.zeros(6); xi[j] = h
                    lp = o.pose_loss(boxes, ss.colmajor(_se3(xi) @ T), prm)[0]; lm = o.pose_loss(boxes, ss.colmajor(_se3(-xi) @ T), prm)[0]
                    fd[j] = (lp - lm) / (2 * h)
                fds[h] = fd
            for alpha in range(1, L + 1):
                w = (np.arange(L) < alpha).astype(np.float32)
                g = o.pose_loss_levels(boxes, T16, w, prm)[1].astype(np.float64)
                rec = dict(kind="cosine", train=steps, pose=pname, alpha=alpha, grad6=g.tolist())
                for h, fd in fds.items():
                    rec["cos_h%g" % h] = _cos(g, fd); rec["fd_h%g" % h] = fd.tolist()
                emit(rec)
                print("train %d %-8s alpha %2d  cos(h=1e-3) %+.4f  cos(h=1e-2) %+.4f" % (steps, pname, alpha, rec["cos_h0.001"], rec["cos_h0.01"]), flush=True)
        # ---- 3. the sweep
        starts = [("5deg5pct_s%d" % s, perturb(Ttrue, 5.0, 0.05 * diag, s)) for s in (1, 2, 3)] + [("15deg10pct_s1", perturb(Ttrue, 15.0, 0.10 * diag, 1)),
                                                                                                   ("true", Ttrue)]
        for iters in (100, 200):
            p = pkg.pose_refine_default(iters=iters)
            for sname, T0 in starts:
                pose, trace = o.refine_pose(boxes, ss.colmajor(T0), p)
                e = pose_errors(_mat(pose), Ttrue)
                emit(dict(kind="plain", train=steps, iters=iters, start=sname, rot_deg=e[0], centre_pct=100 * e[1] / diag, loss0=float(trace[0]),
                          loss_end=float(trace[-1])))
        if not a.no_sweep:
            grid = [(s, e, r) for s in (2, 3, 4, 5) for e in (4, 5, 6, 7, 8, 10, 12, 16) for r in (0.5, 0.7, 1.0) if e >= s] + [(4, 8, 0.6)]
            for (ls, le, rp) in grid:
                for iters in (100, 200):
                    p = pkg.pose_refine_default(iters=iters); c = pkg.pose_c2f_default(level_start=ls, level_end=le, ramp=rp)
                    for sname, T0 in starts:
                        pose, trace = o.refine_pose_c2f(boxes, ss.colmajor(T0), p, c)
                        e = pose_errors(_mat(pose), Ttrue)
                        emit(dict(kind="c2f", train=steps, level_start=ls, level_end=le, ramp=rp, iters=iters, start=sname, rot_deg=e[0],
                                  centre_pct=100 * e[1] / diag, loss0=float(trace[0]), loss_end=float(trace[-1])))
        print("train %d: probes %.1f s" % (steps, time.time() - t_start), flush=True)
        # ---- 4. c2f step against plain
        if not a.no_timing and steps == int(a.train.split(",")[0]):
            T = ss.colmajor(Ttrue); c = pkg.pose_c2f_default()
            for rays in (1024, 4096, 16384):
                res = {}
                for mode in ("plain", "c2f"):
                    out = {}
                    for iters in (0, 100):
                        p = pkg.pose_refine_default(iters=iters, rays_per_iter=rays)
                        call = (lambda: o.refine_pose(boxes, T, p)) if mode == "plain" else (lambda: o.refine_pose_c2f(boxes, T, p, c))
                        call(); best = None
                        for _ in range(5):
                            t0 = time.perf_counter(); call(); dt = time.perf_counter() - t0
                            best = dt if best is None else min(best, dt)
                        out[iters] = best
                    res[mode] = (out[100] - out[0]) / 100
                rec = dict(kind="timing", rays=rays, ms_per_step_plain=1e3 * res["plain"], ms_per_step_c2f=1e3 * res["c2f"],
                           ratio=res["c2f"] / res["plain"])
                emit(rec); print(json.dumps(rec), flush=True)
        o.close()
    ds.close(); fout.close()


if __name__ == "__main__":
    main()
