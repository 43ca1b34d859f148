"""The fp64 stage references of tests/stage_reference.py judged with the CPU ORACLE in the device's place (no GPU): the oracle is trained 150 steps at c1
and c2s, the trained parameters are set on a fresh oracle, and every stage comparison of tests/test_trained_stages.py runs on the oracle's own buffers.  This
pins the restatement where no device is at hand and records what the fp32 oracle itself needs (printed: exact-match shares and k per stage)."""
import numpy as np
import pytest

import __graft_entry__ as ge
import stage_reference as sr
from parity import CFGS

STEPS = 150
BUFS = ("half", "E", "Hid", "O", "dO", "dHid", "dE", "gmlp", "tdist", "bgcol", "target", "target_depth", "ray_flag", "rgb_ray", "mask_ray", "depth_ray",
        "loss_ray", "pts", "ggrid", "ggrid_h")


@pytest.fixture(scope="module", params=sorted(CFGS))
def trained(request, orc, small_scene):
    """(name, oracle holding one forward/backward at its own 150-step weights, its buffers)"""
    kw = CFGS[request.param]
    m = ge.make_oracle(orc, small_scene, kw); m.train(STEPS); p = m.buffer("master"); m.close()
    ref = ge.make_oracle(orc, small_scene, kw); ref.set_params(p); ref.generate_batch(); ref.forward_backward()
    assert ref.n_valid > 0
    yield request.param, ref, {b: ref.buffer(b) for b in BUFS}
    ref.close()


def test_ulp16_and_half_bar():
    x = np.array([0.0, 2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 1.0, 1.5, 2.0, 65504.0])
    assert np.array_equal(sr.ulp16(x), [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** 5])
    assert np.array_equal(sr.ulp16(-x), sr.ulp16(x))
    for v in x[1:-1]:                                                           # the spacing of numpy's own fp16
        assert np.float64(np.nextafter(np.float16(v), np.float16(np.inf))) - v == sr.ulp16(v)
    # just below a binade edge, within the slack: the ulp of the binade above
    assert sr.half_bar(np.array([2.0 - 1e-9]), 1e-8)[0] == 0.5 * 2.0 ** -9 + 1e-8 and sr.half_bar(np.array([1.9]), 1e-8)[0] == 0.5 * 2.0 ** -10 + 1e-8
    assert sr.h(2.0 ** -25 * 1.01) == 2.0 ** -24 and sr.h(2.0 ** -25) == 0.0     # subnormals kept, ties to even


def test_composite_reference_closed_forms():
    """composite_and_gradient on rays small enough to do by hand: a ray that is cut (samples after the cut neither composite nor carry a gradient, the
    cut falls BEFORE the first sample with T < 1e-4), the first interval measured from t = 0, a background ray's 0.01 dsig term and the +-15 clamp."""
    S = 4; raw = np.array([[0, 0, 0, 3.0], [0, 0, 0, 3.0], [0, 0, 0, 3.0], [0, 0, 0, 3.0]], np.float16)
    O = np.stack([raw, raw]).view(np.uint16); t = np.tile(np.array([0.5, 1.0, 1.5, 2.0], np.float32), (2, 1))
    cg = sr.composite_and_gradient(O, t, np.zeros((2, 3), np.float32), np.full((2, 3), 0.5, np.float32), np.zeros(2, np.float32), np.array([1, 0], np.uint8),
                                   2, 128.0)
    om = np.exp(-np.exp(3.0) * 0.5)                                             # per sample, the first one from t = 0: 4.4e-5 < 1e-4
    assert np.array_equal(cg["n_act"], [1, 1]) and np.allclose(cg["mask"], 1 - om, rtol=1e-14) and np.allclose(cg["rgb"], 0.5 * (1 - om), rtol=1e-14)
    assert not cg["dO"][:, 1:].any() and cg["dO"][:, 0].all()
    g = 2 * (0.5 * (1 - om) - 0.5); dsig = np.exp(3.0)
    want_obj = 64.0 * dsig * 0.5 * (3 * g * (om * 0.5 - 0.0) - 0.5 * om); want_bg = 64.0 * (dsig * 0.5 * 0.5 * om + dsig * 0.01)
    assert np.isclose(cg["dO"][0, 0, 3], want_obj, rtol=1e-12) and np.isclose(cg["dO"][1, 0, 3], want_bg, rtol=1e-12)
    assert (cg["A"] >= np.abs(cg["dO"])).all()
    big = np.array([[[0, 0, 0, 16.0]] * S], np.float16).view(np.uint16)
    a = sr.composite_and_gradient(big, t[:1] * 1e-9, np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros(1, np.float32), np.array([0], np.uint8),
                                  1, 1.0)
    assert np.isclose(a["dO"][0, 0, 3] / (0.5 * 0.5e-9 * (1 - a["mask"][0]) + 0.01), np.exp(15.0), rtol=1e-12)       # dsig clamped, sigma not


def test_every_stage_of_the_oracle_at_trained_weights(trained):
    """Figures of this test on the oracle (150 steps; printed with -s): every MLP stage >= 99.988 % of elements equal h(want), >= 99.999 % within one ulp,
    worst 2 ulp, the error beyond the final rounding <= 4.9 u A (bar K u A); gmlp <= 5.3 u A; composite outputs within 3.1e-7; dL/dO 99.82-99.96 % equal
    h(want), >= 99.97 % within one ulp, worst 4 ulp (cancellation in T c - suffix), k = 0.25 (c2s) and 0.03 (c1) against DLDO_K_ORACLE = 1, zero pattern
    after the cut exact, no ambiguous ray; every wanted non-zero dL/dE of the all-subnormal rows non-zero (30 206 at c2s, 10 574 at c1)."""
    name, ref, b = trained
    L = ref.cfg.n_levels
    st = sr.mlp_stages(b, ref.n_mlp, ref.Epad, ref.W, ref.NH, L)
    for stage, f in sorted(st.items()):
        print("%s %-6s %s" % (name, stage, f))
    for stage, f in st.items():
        assert f["n_bad"] == 0, (name, stage, f)
        if stage != "gmlp":
            assert f["exact"] >= 0.9995 and f["within1"] >= 0.9999 and f["worst_ulp"] <= 2, (name, stage, f)
    assert st["gmlp"]["pad_rows_zero"] and st["dE"]["zero_rows_exact"] and all(st["dHid%d" % l]["zero_rows_exact"] for l in range(ref.NH))
    # the subnormal rows: the oracle keeps every one of their wanted non-zero dL/dE
    assert st["dE"]["sub_rows"] >= 200 and st["dE"]["sub_got_nonzero"] == st["dE"]["sub_wanted_nonzero"] > 0, st["dE"]
    f, cg = sr.composite_stages(b, ref.R, ref.cfg.loss_scale, sr.DLDO_K_ORACLE)
    print(name, "composite", {k: v for k, v in f.items() if k != "dO"}); print(name, "dL/dO", f["dO"])
    # (COMPOSITE_ERR_ORACLE is the worst this measured, 3.0e-7 at c2s; held here to the 4 x of it that the device's bar is made of: the training
    # trajectory, and with it the batch, moves with the number of threads the oracle sums its weight gradient over)
    assert max(f["rgb"], f["mask"], f["depth"], f["loss"]) <= 4.0 * sr.COMPOSITE_ERR_ORACLE, f
    assert f["dO"]["n_bad"] == 0 and f["dO"]["k"] <= sr.DLDO_K_ORACLE and f["dO"]["after_cut_nonzero"] == 0, f["dO"]
    assert f["dO"]["exact"] >= 0.995 and f["dO"]["within1"] >= 0.999, f["dO"]
    assert f["ambiguous"] <= 0.01, f
    rg = sr.regime(cg, st["dE"]["wanted_nonzero_subnormal"])
    print(name, "regime", rg)
    for key, bar in sr.REGIME_BARS.items():
        assert rg[key] >= bar, (name, key, rg)
    # grid gradient: the oracle's fp32 sum of the fp16-rounded contributions, and its fp16 table after one more h()
    dE = sr.h2d(b["dE"]).reshape(-1, ref.Epad)
    want, A, cnt = sr.grid_scatter(dE, b["pts"], ref.cfg)
    got = b["ggrid"].astype(np.float64).reshape(-1, 2); bar = 2.0 ** -9 * A + cnt * sr.U
    assert (np.abs(got - want) <= bar).all() and not got[cnt == 0].any(), float(np.abs(got - want).max())
    flip = np.abs(want) <= cnt * sr.U                                           # (a sum within the one-ulp flips of its contributions may come out zero)
    assert np.array_equal((got != 0)[~flip], (want != 0)[~flip]) and (want != 0).sum() > 1000
    gh = sr.h2d(b["ggrid_h"]).reshape(-1, 2)
    assert (np.abs(gh - want) <= sr.half_bar(want, bar)).all()
