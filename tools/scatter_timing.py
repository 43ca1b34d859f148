#!/usr/bin/env python
"""Per-phase cycle breakdown of k_grid_scatter and the walk's finish times per SIMD (GPU box; build first: tools/variant_build.sh sctime -DMON_SCATTER_TIMING;
MON_CORE_LIB names another timing build, e.g. one with -DMON_WAVE_PRIO=0 on top)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MON_CORE_LIB", os.path.join(ROOT, "ro-map_amd", "build_sctime", "libmon_core.so"))
import __graft_entry__ as ge  # noqa: E402

PH = ["setup (counters, level constants)", "tile clear", "barrier after clear", "walk (+ the dW row loads behind it)", "barrier (wait for the slowest wave)",
        "tile write-out", "wave start (low 24 bits of the clock)"]


def simd_finish_table(buf, simd):
    """When the waves that share a SIMD leave the walk: clock counts after the workgroup's first wave entered the kernel, the SIMD's waves in finishing order,
    mean over the workgroups' SIMDs that hold four waves (a workgroup is the CU's only one: its 16 waves are all of the SIMD's)."""
    start = buf[:, :, 6]; start = np.where(start - start.min(1, keepdims=True) > 2 ** 23, start - 2 ** 24, start)      # (24-bit clock: unwrap inside a workgroup)
    fin = start - start.min(1, keepdims=True) + buf[:, :, :4].sum(2); rows = []
    for g in range(buf.shape[0]):
        for s in range(4):
            f = np.sort(fin[g][simd[g] == s])
            if len(f) == 4 and buf[g, 0, 3] > 0:
                rows.append(f)
    if rows:
        r = np.array(rows); print("walk finish per SIMD (%d SIMDs with four waves), waves in finishing order: " % len(r) + " / ".join("%.0f" % v for v in r.mean(0))
                + "; last - first: mean %.0f max %.0f" % ((r[:, 3] - r[:, 0]).mean(), (r[:, 3] - r[:, 0]).max()))


def main():
    pkg = ge.load_package(); ss = ge.load_tools()
    sc = ss.make_scene(n_views=40, H=480, W=640, f=525.0, seed=0)
    ds, obj = ge.make_problem(pkg, sc, dict(sample_seed=2024))
    L = C.CDLL(os.environ["MON_CORE_LIB"])
    for steps, name in ((10, "dense (step 10)"), (800, "sparse (step 810)")):
        obj.train(steps)
        buf = np.zeros((256, 16, 8), np.float32); L.mon_debug_scatter_timing(buf.ctypes.data_as(C.c_void_p))
        lv = buf[:, 0, 7].astype(int) & 15; simd = (buf[:, :, 7].astype(int) >> 4) & 3
        print("\n== %s: mean cycles per wave; workgroups by level" % name)
        print("| level | " + " | ".join(PH) + " | total |"); print("|---|" + "---|" * (len(PH) + 1))
        for l in sorted(set(lv)):
            m = buf[lv == l][:, :, :7].mean((0, 1)); print("| %d | " % l + " | ".join("%.0f" % v for v in m) + " | %.0f |" % m.sum())
        w = buf[:, :, 3]; print("walk cycles per wave: min %.0f mean %.0f max %.0f" % (w.min(), w.mean(), w.max()))
        simd_finish_table(buf, simd)
        wg = int(np.where(lv == 7)[0][0]); print("workgroup %d (level 7), per wave:" % wg)
        print(np.array2string(buf[wg, :, :7], precision=0, suppress_small=True, max_line_width=200))
        st = buf[:, :, 6]
        print("wave start clock (low bits): spread inside a workgroup max %.0f; over the grid %.0f" % ((st.max(1) - st.min(1)).max(), st.max() - st.min()))
    obj.close(); ds.close()


if __name__ == "__main__":
    main()
