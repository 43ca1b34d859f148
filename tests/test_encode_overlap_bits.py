"""k_encode_tiles' first copy phase and workgroup order (kernels_encode.hip MON_ENC_POSWAIT; model.h MON_ENC_XCD) against the gathers inside
k_fused_train, bit for bit.

Neither changes an operation on a value: the first barrier waits for the tile copy by count instead of for everything (the copy is kept out of the compiler's
wait bookkeeping, the positions are fetched as 12 bytes, the state words come through the scalar cache), and a workgroup takes its (level, partition) from a
permutation of the grid.  What CAN go wrong is a wave that reads the tile before its copy landed (a count that does not match the loads the wave issued), a
round that uses a position before it arrived, and a workgroup that walks another's pair.  Every such fault changes features, and with them every parameter.

The reference does not run the code under test: DESIGN.md section 3 states that the level-tile chain (option lds_encode = 2: tiles at any batch size) and the
gather chain (lds_encode = 0: the forward gathers inside k_fused_train, or inside the layer kernels' encode) give the same bits.  Each case trains 3 steps
from initialisation on the 12-view 160 x 120 scene once on either chain and compares the CRC32 of master, fp16 copy and EMA and the bits of the returned loss.
There is no tolerance.

Cases, the smallest shapes at which each item can go wrong:

  r64, r256     64 / 256 rays, base.json's table: 128 / 512 samples per workgroup, so 14 / 8 of its 16 waves have no sample, issue no position load and must
                wait for everything; the others walk one round;
  res36_l2      base_resolution 36, n_levels 2: level 0 is a DENSE parity level of 36^3 = 46 656 entries, half tiles of 93 312 bytes (no multiple of a wave's
                1 KB: the last copy instruction of a wave is partly masked); level 1 is hashed; 32 workgroups in the plain order;
  levels5, levels1   80 / 16 workgroups in the plain order (no multiple of 4 levels); res36_l2 aside, the cases with 16 levels take the XCD order;
  r4160         133 120 samples: two batch chunks (blockIdx.y = 0, 1);
  live          3072 rays, occupancy_skip = 1 with the pinned grid of tests/test_fused_chain_bits.py: the live-sample lists, which keep the full wait;
  neurons16     the layer-at-a-time backend, whose forward encode is k_encode_tiles too;
  levels8       n_levels 8: the XCD order with four partitions per label."""
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

SEED = dict(sample_seed=1213)
N_OCC = 64
# case -> (config, backend the shape runs on)
CASES = {
    "r64": (dict(SEED, rays_per_batch=64), 1),
    "r256": (dict(SEED, rays_per_batch=256), 1),
    "res36_l2": (dict(SEED, rays_per_batch=1024, base_resolution=36, n_levels=2), 1),
    "levels5": (dict(SEED, rays_per_batch=1024, n_levels=5), 1),
    "levels1": (dict(SEED, rays_per_batch=1024, n_levels=1), 1),
    "r4160": (dict(SEED, rays_per_batch=4160), 1),
    "live": (dict(SEED, rays_per_batch=3072, occupancy_skip=1), 1),
    "neurons16": (dict(SEED, rays_per_batch=3072, n_neurons=16), 0),
    "levels8": (dict(SEED, rays_per_batch=1024, n_levels=8), 1),
}
STEPS = 3


def _occ_bits():
    """Half of the cells live, at random: one bit per cell, x fastest, 32 cells per word (the grid of tests/test_fused_chain_bits.py)."""
    live = np.random.RandomState(5).uniform(size=N_OCC ** 3) < 0.5
    return np.packbits(live.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def run_chain(pkg, sc, case, lds_encode):
    kw, backend = CASES[case]
    old = pkg.get_option("lds_encode")
    try:
        pkg.set_option("lds_encode", lds_encode)          # (read when the object is created)
        ds, obj = ge.make_problem(pkg, sc, kw)
    finally:
        pkg.set_option("lds_encode", old)
    assert int(obj.info().backend) == backend, (case, int(obj.info().backend))
    try:
        obj.buffer("x_all"); has_tiles = True              # the position pass's buffer exists with the level-tile chain only
    except pkg.MonError:
        has_tiles = False
    assert has_tiles == (lds_encode != 0), (case, lds_encode, has_tiles)
    if case == "live":
        obj.set_train_occupancy(_occ_bits())
        assert (obj.occupancy_grid()[3] > 0) == (lds_encode != 0), "the level-tile chain without live-sample lists"
    loss = obj.train(STEPS)
    out = dict(crc=["%08x" % zlib.crc32(obj.get_params(w).tobytes()) for w in (0, 1, 2)], loss="%08x" % struct.unpack("<I", struct.pack("<f", loss))[0],
               skipped=int(obj.info().skipped_batches), n_valid=int(obj.info().last_n_valid))
    obj.close(); ds.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_level_tiles_give_the_bits_of_the_gather_chain(pkg, small_scene, case):
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    want = run_chain(pkg, small_scene, case, 0)
    got = run_chain(pkg, small_scene, case, 2)
    print(case, got, want)
    assert want["skipped"] == 0 and want["n_valid"] > 0 and np.isfinite(struct.unpack("<f", struct.pack("<I", int(want["loss"], 16)))[0]), want
    assert got == want, (case, got, want)
