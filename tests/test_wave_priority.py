"""Wave priorities in the training kernels (device_common.h wave_prio_graded / wave_prio_set; -DMON_WAVE_PRIO=0 builds the kernels without them).

A priority decides which wave of a SIMD issues next, never what a wave computes: no load, store or arithmetic instruction differs.  What CAN go wrong is
the new scalar control flow around the s_setprio instructions (a miscompiled branch, a wave leaving its loop early).  So every check is bit-for-bit against
the build WITHOUT the priorities: three steps of training at the smallest batch of the level-tile chain (3072 rays), base.json's level table (level 0: a
whole-level tile, level 1: a parity-64 tile in k_grid_scatter, levels 2..15: hashed parity tiles, level 12: res = 65 536, whose index ignores y and z), in
three cases that take every changed path:

  dense   from initialisation: every sample carries a gradient, all waves of a workgroup walk the same number of rounds;
  live    a pinned occupancy grid: k_encode_tiles walks live-sample lists, waves skip rounds and their trip counts differ;
  short   after WARM steps without keep_zero_samples: the compacted ray bins hold at most 512 rows, k_grid_scatter's waves split into G > 1 groups.

tests/golden/wave_priority_parent_crc.json holds the CRCs of (master, fp16 copy, EMA) that the parent commit's build gave for these cases on an MI355X:

    tools/variant_build.sh parent          # in a checkout of the parent commit; or, in this one: tools/variant_build.sh parent -DMON_WAVE_PRIO=0
    MON_CORE_LIB=ro-map_amd/build_parent/libmon_core.so python tests/test_wave_priority.py --record

Bit equality is the condition: there is no tolerance."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wave_priority_parent_crc.json")
KW = dict(rays_per_batch=3072, sample_seed=1213)                 # base.json's network and level table otherwise
SCENE = dict(n_views=12, H=120, W=160, f=130.0, seed=0)          # (conftest's small_scene)
WARM = 1500                                                       # steps in front of the `short` case
N_BINS, BIN_ROWS_GROUPED = 16, 512                               # k_grid_scatter: ray bins of a batch; the longest run its waves still split into groups for
CASES = ("dense", "live", "short")
N_OCC = 64                                                       # occupancy grid: cells per axis


def _occ_bits():
    """Half of the cells live, at random: one bit per cell, x fastest, 32 cells per word."""
    live = np.random.RandomState(5).uniform(size=N_OCC ** 3) < 0.5
    return np.packbits(live.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def run_case(pkg, ss, case):
    """(CRCs of master / fp16 copy / EMA after the case's three steps, gradient-carrying samples of its last step)"""
    sc = ss.make_scene(**SCENE)
    ds, obj = ge.make_problem(pkg, sc, dict(KW, occupancy_skip=1) if case == "live" else KW)
    i = obj.info()
    assert int(i.backend) == 1 and i.n_params == 3072 + 2 * (4096 + 32768 + 14 * 65536), (int(i.backend), i.n_params)
    if case == "live":
        obj.set_train_occupancy(_occ_bits())
        assert obj.occupancy_grid()[3] > 0, "the level-tile chain without live-sample lists"
    if case == "short":
        obj.train(WARM)
    obj.train(3)
    n_grad = int(obj.buffer("state")[24])
    crc = ["%08x" % zlib.crc32(obj.get_params(w).tobytes()) for w in (0, 1, 2)]
    assert obj.info().skipped_batches == 0
    obj.close(); ds.close()
    return crc, n_grad


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_priorities_leave_the_trained_parameters_bit_identical(pkg, ss, case):
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    crc, n_grad = run_case(pkg, ss, case)
    print(case, crc, n_grad, want)
    if case == "dense":
        assert n_grad == KW["rays_per_batch"] * 32                # every sample: full bins, one bin per step
    if case == "short":
        assert 0 < n_grad <= N_BINS * BIN_ROWS_GROUPED // 2      # bins of rays (ray mod 16) around n_grad / 16 rows: under 512 with a factor 2 to spare
    assert n_grad == want["n_grad"] and crc == want["crc"], (case, crc, n_grad, want)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: MON_CORE_LIB=<library of the parent commit> python tests/test_wave_priority.py --record")
    pkg_, ss_ = ge.load_package(), ge.load_tools()
    out = {}
    for c in CASES:
        crc_, n_ = run_case(pkg_, ss_, c); out[c] = dict(crc=crc_, n_grad=n_)
    print(json.dumps(out))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1); f.write("\n")
