#!/usr/bin/env python
"""When the waves that share a SIMD leave k_encode_tiles' sample loops (GPU box; build first: tools/variant_build.sh enctime -DMON_ENCODE_TIMING;
MON_CORE_LIB names another timing build, e.g. one with -DMON_WAVE_PRIO=0 on top).  A workgroup is its CU's only one, so the four waves of a SIMD are its
own; a stamp drains the wave's stores first, so a loop owns the latency of what it stored."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MON_CORE_LIB", os.path.join(ROOT, "ro-map_amd", "build_enctime", "libmon_core.so"))
import __graft_entry__ as ge  # noqa: E402


def table(buf, col, name):
    start = buf[:, :, 0]; start = np.where(start - start.min(1, keepdims=True) > 2 ** 23, start - 2 ** 24, start)      # (24-bit clock: unwrap inside a workgroup)
    fin = start - start.min(1, keepdims=True) + buf[:, :, col]; simd = buf[:, :, 3].astype(int)
    print("| level | waves of a SIMD in finishing order, clock counts after the workgroup's first wave entered | last - first | per wave, min / mean / max: kernel entry to the end of the first loop; end of the first loop (barrier, second tile copy) to the end of the second |")
    print("|---|---|---|---|")
    for lv in range(buf.shape[0] // 16):
        rows = []
        for g in range(16 * lv, 16 * lv + 16):
            for s in range(4):
                f = np.sort(fin[g][simd[g] == s])
                if len(f) == 4 and buf[g, 0, col] > 0:
                    rows.append(f)
        if rows:
            r = np.array(rows); own = buf[16 * lv:16 * lv + 16, :, col] - (buf[16 * lv:16 * lv + 16, :, 1] if col == 2 else 0)
            print("| %d %s | " % (lv, name) + " / ".join("%.0f" % v for v in r.mean(0)) + " | %.0f | %.0f / %.0f / %.0f |" % ((r[:, 3] - r[:, 0]).mean(), own.min(),
                    own.mean(), own.max()))


def phases(buf):
    """per level: workgroup means of the slowest wave's marks (a barrier lets the workgroup go when its last wave arrives), in clock64() counts like the table above"""
    print("| level | copy 1 (+ positions): entry to behind the first barrier | walk 1: to the last wave's end of the first loop | copy 2: to behind the barrier "
          "after the second copy | walk 2: to the last wave's end of the second loop | XCDs of the 16 workgroups (workgroups on each) |")
    print("|---|---|---|---|---|---|")
    for lv in range(buf.shape[0] // 16):
        g = buf[16 * lv:16 * lv + 16]
        if g[:, 0, 1].max() <= 0:
            continue
        b1, w1, b2, w2 = g[:, :, 4].max(1), g[:, :, 1].max(1), g[:, :, 5].max(1), g[:, :, 2].max(1)
        xcd = g[:, 0, 6].astype(int); where = ", ".join("%d (%d)" % (x, (xcd == x).sum()) for x in sorted(set(xcd)))
        if b2.max() > 0:
            print("| %d | %.0f | %.0f | %.0f | %.0f | %s |" % (lv, b1.mean(), (w1 - b1).mean(), (b2 - w1).mean(), (w2 - b2).mean(), where))
        else:
            print("| %d (whole tile) | %.0f | %.0f | | | %s |" % (lv, b1.mean(), (w1 - b1).mean(), where))


def main():
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=40, H=480, W=640, f=525.0, seed=0)
    ds, obj = ge.make_problem(pkg, sc, dict(sample_seed=2024))
    L = C.CDLL(os.environ["MON_CORE_LIB"])
    for steps, name in ((10, "dense (step 10)"), (800, "late (step 810)")):
        obj.train(steps)
        buf = np.zeros((256, 16, 8), np.float32)
        assert L.mon_debug_encode_timing(buf.ctypes.data_as(C.c_void_p)) == 0
        print("\n== %s: %s" % (name, os.environ["MON_CORE_LIB"]))
        table(buf, 1, "first loop (whole tile: the only one)"); table(buf, 2, "second loop"); print(); phases(buf)
    obj.close(); ds.close()


if __name__ == "__main__":
    main()
