"""k_fused_train's shortened ray chain (fused_device.h MON_FUSED_XLOAD, MON_FUSED_TR) against the parent commit's build, bit for bit.

Neither change may alter a value: the PRE instantiations load the sample positions the position pass wrote instead of recomputing them from the same
record with the same expressions, and the dW transposes hand every MFMA the same operand elements through another LDS image (packed stores, transposed
reads).  What CAN go wrong is a load one ray ahead that runs past the batch, a stale or misindexed x_all row, a transposed read that puts a sample into the
wrong k slot or runs with lanes switched off, a pad column of the feature image that is not zero.  Every case therefore trains a few steps and compares the
CRC32 of master / fp16 copy / EMA, the bits of the returned loss and the number of gradient-carrying samples (state[24]) with
tests/golden/fused_chain_parent_crc.json, recorded once from a library of the parent commit:

    tools/variant_build.sh parent          # in a checkout of the parent commit; or, in this one: ... parent -DMON_FUSED_XLOAD=0 -DMON_FUSED_TR=0
    MON_CORE_LIB=ro-map_amd/build_parent/libmon_core.so python tests/test_fused_chain_bits.py --record

All cases use the 12-view 160 x 120 scene and the smallest shapes at which each changed path can go wrong:

  tiles_dense   R = 3072, base.json's network, 3 steps from initialisation: the level-tile chain's smallest batch; 3072 rays over 2048 waves, so half of
                the waves walk two rays and half one -- the loads one ray ahead must stop at the last ray;
  tiles_short   the same after 1500 warm steps: most rays skip the backward branch and some take it (the transposed reads need every lane there);
  tiles_live    the same with a pinned occupancy grid (OCC && PRE: dead samples keep zero features, the live bits come from the record);
  tiles_depth   R = 3072 with a depth-supervised dataset (tdp > 0);
  tiles_2x64    R = 3072, two hidden layers of 64: NH = 2, the one-wave-per-SIMD instantiation, both hidden images;
  gather_c1     BASELINE configs[0] (R = 1024, L = 4, 2 x 32): EPAD = 16 (32-byte feature rows), W = 32, not PRE -- positions computed in the kernel;
  gather_small  R = 256, base.json's network: the gather chain at the benched network shape;
  skipped       an object whose boxes hold no ray: every batch is skipped, counted, and changes nothing.

Bit equality is the condition: there is no tolerance."""
import json
import os
import struct
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_chain_parent_crc.json")
SCENE = dict(n_views=12, H=120, W=160, f=130.0, seed=0)          # (conftest's small_scene)
TILES = dict(rays_per_batch=3072, sample_seed=1213)              # base.json's network and level table otherwise
WARM = 1500                                                       # steps in front of the `short` case
N_OCC = 64                                                       # occupancy grid: cells per axis
# case -> (config, level-tile chain?, steps)
CASES = {
    "tiles_dense": (TILES, True, 3),
    "tiles_short": (TILES, True, 3),
    "tiles_live": (dict(TILES, occupancy_skip=1), True, 3),
    "tiles_depth": (TILES, True, 3),
    "tiles_2x64": (dict(TILES, n_neurons=64, n_hidden_layers=2), True, 3),
    "gather_c1": (dict(rays_per_batch=1024, n_levels=4, n_neurons=32, n_hidden_layers=2, sample_seed=1213), False, 3),
    "gather_small": (dict(rays_per_batch=256, sample_seed=1213), False, 3),
    "skipped": (TILES, True, 3),
}


def _occ_bits():
    """Half of the cells live, at random: one bit per cell, x fastest, 32 cells per word (the grid of tests/test_wave_priority.py)."""
    live = np.random.RandomState(5).uniform(size=N_OCC ** 3) < 0.5
    return np.packbits(live.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def _crcs(obj):
    return ["%08x" % zlib.crc32(obj.get_params(w).tobytes()) for w in (0, 1, 2)]


def run_case(pkg, ss, case):
    """dict(crc of master / fp16 copy / EMA, bits of the returned loss, gradient-carrying samples of the last step, skipped batches)"""
    kw, tiles, steps = CASES[case]
    sc = ss.make_scene(**SCENE)
    ds, obj = ge.make_problem(pkg, sc, kw, use_depth=(case == "tiles_depth"))
    other = None
    if case == "skipped":
        # (tests/test_store_policy.py: the same box list on an object 50 m away -- no candidate ray meets it)
        ob = sc.objects[0]; far = ob["Tow"].copy(); far[:3, 3] += 50.0
        other = obj; obj = pkg.ObjectNeRF(ds, pkg.default_config(**kw), ob["cls"], ss.colmajor(far), -ob["half"], ob["half"]); obj.add_boxes(ob["boxes"])
    assert int(obj.info().backend) == 1
    # the chain in use: the position pass's buffer exists with the level-tile chain only
    try:
        obj.buffer("x_all"); has_tiles = True
    except pkg.MonError:
        has_tiles = False
    assert has_tiles == tiles, (case, has_tiles)
    if case == "tiles_live":
        obj.set_train_occupancy(_occ_bits())
        assert obj.occupancy_grid()[3] > 0, "the level-tile chain without live-sample lists"
    if case == "tiles_short":
        obj.train(WARM)
    before = _crcs(obj)
    loss = obj.train(steps)
    out = dict(crc=_crcs(obj), loss="%08x" % struct.unpack("<I", struct.pack("<f", loss))[0], n_grad=int(obj.buffer("state")[24]),
               skipped=int(obj.info().skipped_batches))
    if case == "skipped":
        assert out["crc"] == before and obj.info().last_n_valid == 0, (before, out)
        other.close()
    obj.close(); ds.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_shortened_ray_chain_leaves_training_bit_identical(pkg, ss, case):
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = run_case(pkg, ss, case)
    print(case, got, want)
    kw, _, steps = CASES[case]
    if case == "skipped":
        assert got["skipped"] == steps
    else:
        assert got["skipped"] == 0
    if case == "tiles_dense":
        assert got["n_grad"] == kw["rays_per_batch"] * 32             # every sample carries a gradient: every ray takes the backward branch
    if case == "tiles_short":
        assert 0 < got["n_grad"] < kw["rays_per_batch"] * 32 // 4     # ... and here most rays do not
    assert got == want, (case, got, want)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: MON_CORE_LIB=<library of the parent commit> python tests/test_fused_chain_bits.py --record")
    pkg_, ss_ = ge.load_package(), ge.load_tools()
    out_ = {c: run_case(pkg_, ss_, c) for c in sorted(CASES)}
    print(json.dumps(out_))
    with open(GOLDEN, "w") as f:
        json.dump(out_, f, indent=1); f.write("\n")
