#!/usr/bin/env python
"""Cost of object checkpoints (mon_object_save / mon_object_load) on the GPU box.

    python tools/checkpoint_timing.py [--steps 64] [--reps 3] [--dir /tmp] [--shapes base,T22]

For base.json and for T = 2^22 (log2_hashmap_size = 22: chunk records, lazy EMA, a 1.7 GB file): the wall time of a save and of a load (best of `reps`,
after one warm-up of each), the HIP-event time of the pack / unpack kernels inside them (mon_debug_checkpoint_timing; zero for base.json, whose optimizer
state sits in plain arrays apart from the 16-bit step counters), the file's bytes over the wall time, and for context what the only persistence before
checkpoints cost: mon_object_create + mon_object_set_params of the same shape.  Files go to --dir (a RAM-backed directory measures the library, a disk
measures the disk).  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"base": dict(), "T22": dict(log2_hashmap_size=22)}


def best_of(reps, fn):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--shapes", default="base,T22")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=12, H=120, W=160, f=130.0, seed=0)
    ds = None
    for name in a.shapes.split(","):
        ds, o = ge.make_problem(pkg, sc, SHAPES[name], dataset=ds)
        o.train(a.steps)
        path = os.path.join(a.dir, "checkpoint_timing_%s_%d.monckpt" % (name, os.getpid()))
        loaded = []

        def save():
            o.save(path)

        def load():
            loaded.append(pkg.ObjectNeRF.load(ds, path)); loaded.pop().close()
        save(); load()                                                    # warm-up: page cache, first-use allocations
        pkg.checkpoint_timing(True)
        t_save = best_of(a.reps, save); k_save = pkg.checkpoint_timing(True) / a.reps
        t_load = best_of(a.reps, load); k_load = pkg.checkpoint_timing(False) / a.reps
        size = os.path.getsize(path)
        # the close of the loaded object is inside t_load; so is the destroy here
        master = o.get_params(0); ob = sc.objects[0]; cfg = o.cfg

        def create_set():
            q = pkg.ObjectNeRF(ds, cfg, ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"]); q.set_params(master); q.close()
        create_set(); t_create = best_of(a.reps, create_set)
        i = o.info()
        print(json.dumps(dict(shape=name, n_params=i.n_params, file_bytes=size, save_ms=round(1e3 * t_save, 2), load_ms=round(1e3 * t_load, 2),
                              save_kernel_ms=round(k_save, 3), load_kernel_ms=round(k_load, 3), save_GBps=round(size / t_save / 1e9, 3),
                              load_GBps=round(size / t_load / 1e9, 3), create_plus_set_params_ms=round(1e3 * t_create, 2))), flush=True)
        os.remove(path); o.close()
    ds.close()


if __name__ == "__main__":
    main()
