"""The merge-composite kernels' outputs, bit for bit against the build of the commit before their LDS layout (SceneLds) and their 64-sample block
(scene_fetch, scene_transmittance, scene_block_add, scene_list_weights, scene_carry; scene_device.h) were written once.

tests/test_scene_routes_crc.py holds the routes that run these kernels, with two objects: at most 128 merged samples per ray.  It never reaches a second
ballot group of lists, 64 lists in one block, a cut inside a late block or the two-float transmittance scan.  So the four debug entries --
mon_debug_scene_composite, mon_debug_scene_probe_composite, mon_debug_scene_cast_composite at the thresholds 0.5 and 0.8 and
mon_debug_scene_composite_grad with GRAD_W -- are called on synthetic lists that do, and the CRC32 of every array they return must equal the one
recorded from the parent commit's build (1f29db9, "k_encode_tiles: counted wait before the first barrier, XCD block order") on an MI355X:

    tools/variant_build.sh parent          # in a checkout of the parent commit
    MON_CORE_LIB=<that checkout>/ro-map_amd/build_parent/libmon_core.so python tests/test_scene_composite_bits.py --record

(libmon_core_diag.so is taken from the same directory.)  The record was made twice and the two files were identical: these kernels use no atomics.

The lists come from the suites' own generators with their seeds and ray counts:
  render-K{1,3,16}[-ties]   tests/test_scene_render.py's _adversarial, both of its draws (700 rays of alpha up to 0.3, 0.6 at K = 1; 300 rays of alpha up to
                            0.02): a list compositing to its own render's arithmetic, ties to the lower list
  track-K2[-ties]           tests/test_scene_track.py's _adversarial with the wall, and its targets: counts {0, 32, 64}, a ray with no list, a list behind
                            the cut, both Huber branches
  through-K17               tests/test_scene_many_lists_reference.py's cases from here on: the first K above 16, no cut
  wall-K64, early-K65       one full ballot group, and one list into the second; the cut inside a block
  ties_wall-K129            a third group, equal t across lists
  singles-K65, sparse-K256  64 different lists in one block; compaction over empty slots
  full_through-K256         16 384 samples: scan_mul32_comp, 256 blocks, s.T full
Where a generator has no targets or entries they are that reference file's make_targets (on the fp64 depth of np_composite) and tests/test_scene_cast.py's
_entries, seeded as its Case seeds them.  The CRC32s of the inputs are recorded too: a case whose inputs differ from the record's fails on that, before
any kernel is compared.

Bit equality is the condition: there is no tolerance."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import __graft_entry__ as ge                                # noqa: E402
import test_scene_cast as tsc                               # noqa: E402
import test_scene_many_lists_reference as mlr               # noqa: E402
import test_scene_render as tsr                             # noqa: E402
import test_scene_track as tst                              # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_composite_parent_crc.json")
MLR_CASES = (("through", 17), ("wall", 64), ("early", 65), ("ties_wall", 129), ("singles", 65), ("sparse", 256), ("full_through", 256))
CASES = [("render", K, eq) for K in (1, 3, 16) for eq in (False, True)] + [("track", 2, eq) for eq in (False, True)] + [("mlr",) + c for c in MLR_CASES]
ENTRIES = ("scene_composite", "scene_probe_composite", "scene_cast_composite_0.5", "scene_cast_composite_0.8", "scene_composite_grad")
TRACK_ALPHA_HI = 0.01                                        # test_composite_grad_kernel_on_adversarial_lists' draw with the wall


def case_id(case):
    return mlr.case_id(case[1:]) if case[0] == "mlr" else "%s-K%d%s" % (case[0], case[1], "-ties" if case[2] else "")


def _crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def _with_targets(lists, seed):
    """(t, alpha, rgb, count, dn) -> the nine inputs: + cstar, mstar, dstar (mlr.make_targets on np_composite's depth) and the entries, as mlr.Case"""
    t, alpha, rgb, count, dn = lists
    D = tsr.np_composite(t, alpha, rgb, count, dn.astype(np.float64), amb_u=mlr.U)[1]
    return lists + mlr.make_targets(t, count, D, seed) + (tsc._entries(t, seed + 2),)


def inputs(case):
    """the case's draws, each (t, alpha, rgb, count, dn, cstar, mstar, dstar, entry)"""
    kind, K = case[0], case[1]
    if kind == "render":                                     # test_composite_kernel_on_adversarial_lists
        equal_t = case[2]; seed = 100 + K + 7 * int(equal_t)
        rng = np.random.RandomState(seed)
        draws = [tsr._adversarial(rng, K, 700, equal_t, alpha_hi=0.3 if K > 1 else 0.6), tsr._adversarial(rng, K, 300, equal_t, alpha_hi=0.02)]
        return [_with_targets(d, seed + n) for n, d in enumerate(draws)]
    if kind == "track":                                      # test_composite_grad_kernel_on_adversarial_lists
        equal_t = case[2]; seed = 4300 + 10 * K + int(equal_t) + int(1000 * TRACK_ALPHA_HI)
        t, alpha, rgb, count, cstar, mstar, dstar, dn = tst._adversarial(np.random.RandomState(seed), K, 256, equal_t, TRACK_ALPHA_HI, wall=True)
        return [(t, alpha, rgb, count, dn, cstar, mstar, dstar, tsc._entries(t, seed + 2))]
    seed = mlr.seed_of(case[1:])
    return [_with_targets(mlr.make_lists(case[1], case[2], mlr.n_rays(case[2]), seed), seed)]


def run_case(pkg, case):
    """{"inputs": [CRC32 of every input array], entry: [CRC32 of every array it returns]}, the draws of a case one after the other"""
    out = {k: [] for k in ("inputs",) + ENTRIES}
    for arrays in inputs(case):
        t, alpha, rgb, count, dn, cstar, mstar, dstar, entry = arrays
        out["inputs"] += [_crc(a) for a in arrays]
        out["scene_composite"] += [_crc(a) for a in pkg.scene_composite(t, alpha, rgb, count, dn)]
        out["scene_probe_composite"] += [_crc(a) for a in pkg.scene_probe_composite(t, alpha, rgb, count, dn)]
        for thr in mlr.CAST_THR:
            out["scene_cast_composite_%.1f" % thr] += [_crc(a) for a in pkg.scene_cast_composite(t, alpha, rgb, count, entry, thr)]
        g = pkg.scene_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, *mlr.GRAD_W)
        out["scene_composite_grad"] += [_crc(g[k]) for k in sorted(g)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_debug_entries_return_the_parent_builds_bits(pkg, case):
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(case)]
    got = run_case(pkg, case)
    print(case_id(case), got)
    assert got["inputs"] == want["inputs"], "the case's lists are not the recorded ones: %s" % case_id(case)
    bad = {k: (got[k], want[k]) for k in ENTRIES if got[k] != want[k]}
    assert set(got) == set(want) and not bad, (case_id(case), bad)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: MON_CORE_LIB=<library of the parent commit> python tests/test_scene_composite_bits.py --record [file]")
    pkg_ = ge.load_package()
    rec = {case_id(c): run_case(pkg_, c) for c in CASES}
    with open(sys.argv[2] if len(sys.argv) == 3 else GOLDEN, "w") as f:
        json.dump(rec, f, indent=1); f.write("\n")
    print("recorded %d cases" % len(rec))
