"""The layer-chain references of tests/render_reference.py (lattice_u, composite_render64, chain_regime; raw_bounds outside the fused shapes) judged with
the CPU ORACLE in the device's place (no GPU): the oracle is trained 150 steps at 16 x 1 and 64 x 3, two shapes the fused kernels do not take, and at its
EMA weights the lattice, the composite, its counted bound and the regime are checked before any GPU time is spent (tests/test_layer_inference.py holds
the device to the same references).

Figures of this file on the oracle (150 steps, R = 256; printed with -s; the oracle's trajectory moves with the number of threads it sums its weight gradient
over, so they move in the last digit):
  lattice        |oracle - want| / delta on raw3, worst / median: 16 x 1: 7 x 5 x 3 0 / 0, 17^3 0.23 / 0 (equal fp16 numbers on 99.98 %, delta3 median 0.022);
                 64 x 3: 7 x 5 x 3 0 / 0, 17^3 0.16 / 0 (99.94 %, delta3 median 0.25)
  composite      composite_render64 of orc_encode + orc_mlp_forward at the restated samples against orc_render, 24 x 24: no mask flip, rgb within 3.8e-4
                 (16 x 1) and 1.5e-3 (64 x 3), depth within 7.7e-5 and 8.6e-4 (bars 4e-3); no ambiguous ray of 410 hit rays
  bound          the oracle's fp32 composite_ray on the same O and t, share of the counted bound used, worst: rgb 0.05 / 0.06, depth 0.07 / 0.03,
                 1 - T 0.49 / 0.50 (the half ulp of the subtraction where T is negligible)
  regime         16 x 1: raw3 max 7.5, 36 % of hit rays break early, 171 / 239 / 166 rays masked in / out / missed; 64 x 3: 8.2, 36 %, 173 / 237 / 166"""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import field_grad_reference as fgr
import pose_reference as pr
import render_reference as rref
import stage_reference as sr

STEPS = 150
CROP = 24
SHAPES = {"16x1": dict(rays_per_batch=256, n_neurons=16, n_hidden_layers=1), "64x3": dict(rays_per_batch=256, n_neurons=64, n_hidden_layers=3)}
P_ = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


@pytest.fixture(scope="module", params=sorted(SHAPES))
def trained(request, orc, small_scene):
    """(name, the oracle after 150 steps, the network dict of its EMA weights)"""
    m = ge.make_oracle(orc, small_scene, SHAPES[request.param]); m.train(STEPS)
    off, scl, res = pr.level_table(orc, m.cfg)
    net = fgr.net_of(m.buffer("ema").copy(), off, scl, res, m.cfg.n_levels, m.W, m.NH)
    assert net["n_mlp"] == m.n_mlp and net["Ep"] == m.Epad
    yield request.param, m, net
    m.close()


def oracle_O(m, params_u16, u):
    """orc_encode + orc_mlp_forward at unit-cube points u (n, 3) on the fp16 parameter vector given: (E, O) as uint16 [n, Epad], [n, 4]"""
    u = np.ascontiguousarray(u, np.float32).reshape(-1, 3); n = u.shape[0]; prm = np.ascontiguousarray(params_u16, np.uint16)
    E = np.zeros(n * m.Epad, np.uint16); hid = np.zeros(n * m.W * m.NH, np.uint16); O = np.zeros(n * 4, np.uint16)
    m.L.orc_encode(m.h, P_(prm), P_(u), n, P_(E)); m.L.orc_mlp_forward(m.h, P_(prm), P_(E), n, P_(hid), P_(O))
    return E.reshape(n, m.Epad), O.reshape(n, 4)


def test_closed_forms():
    """lattice_u by hand; an opaque first sample breaks at n = 1; an all-transparent ray comes out white; an opacity of exactly 0.5 and a T on EPS are
    flagged ambiguous and nothing else is"""
    u = rref.lattice_u(3, 2, 2)
    assert u.dtype == np.float32 and u.shape == (12, 3) and u[:4].tolist() == [[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [0, 1, 0]] and u[6].tolist() == [0, 0, 1]
    assert np.array_equal(rref.lattice_u(9, 9, 5), rref.lattice_u(129, 129, 65).reshape(65, 129, 129, 3)[::16, ::16, ::16].reshape(-1, 3))
    O = np.zeros((5, 64, 4)); O[..., 3] = -30.0; t = np.tile(np.arange(1, 65, dtype=np.float32) * np.float32(0.01), (5, 1))
    O[0, 0, 3] = 15.0; O[0, 0, :3] = [2.0, 0.0, -2.0]                                         # opaque at once
    t[2, 0] = np.float32(np.log(2.0)); t[2, 1:] += 1; O[2, 0, 3] = 0.0                          # alpha = 1/2 at sample 0, nothing behind it
    t[3, 0] = np.float32(-np.log(sr.EPS)); t[3, 1:] += 10; O[3, 0, 3] = 0.0                     # T = EPS after sample 0
    cr = rref.composite_render64(O, t, np.array([1, 1, 1, 1, 0]), np.full(5, 2.0))
    assert cr["n_used"].tolist() == [1, 64, 64, cr["n_used"][3], 0] and cr["n_used"][3] in (1, 64)
    c = 1.0 / (1.0 + np.exp(-np.array([2.0, 0.0, -2.0])))
    assert cr["mask"].tolist()[:2] == [1.0, 0.0] and np.allclose(cr["rgb"][0], c, rtol=0, atol=1e-12) and abs(cr["depth"][0] - 0.005) < 1e-9
    assert (cr["rgb"][[1, 4]] == 1.0).all() and (cr["depth"][[1, 4]] == 0.0).all() and cr["mask"][4] == 0.0
    assert cr["amb"].tolist() == [False, False, True, True, False]
    assert (cr["e_rgb"][0] > 0).all() and (cr["e_rgb"][0] < 1e-6).all() and 0 < cr["e_depth"][0] < 1e-8 and (cr["e_rgb"][[1, 4]] == 0).all()
    # uint16 bit patterns and fp16 values are the same input
    c2 = rref.composite_render64(O.astype(np.float16).view(np.uint16), t, np.array([1, 1, 1, 1, 0]), np.full(5, 2.0))
    assert np.array_equal(c2["rgb"], cr["rgb"]) and np.array_equal(c2["amb"], cr["amb"])
    # mesh_warp: the kernel's three operations and a bound of three roundings
    w, e = rref.mesh_warp(np.array([[0.25, -0.5, 1.0]], np.float32), np.array([[-1, -1, -1], [1, 1, 3]], np.float32))
    assert w.tolist() == [[0.625, 0.25, 0.5]] and np.array_equal(e, 3 * sr.U * np.array([[0.625, 0.25, 0.5]]))


@pytest.mark.parametrize("res3", [(7, 5, 3), (17, 17, 17)])
def test_lattice_within_delta(trained, res3):
    name, m, net = trained
    u = rref.lattice_u(*res3)
    raw, delta = rref.raw_bounds(net, u)
    got = m.density_grid(*res3, use_ema=True).astype(np.float64)
    ratio = np.abs(got - raw[:, 3]) / delta[:, 3]
    print("%s: lattice %s: |oracle - want| / delta worst %.3f median %.3g; equal fp16 on %.5f; delta3 median %.3g worst %.3g; raw3 max %.2f" % (
        name, res3, ratio.max(), np.median(ratio), (got == raw[:, 3]).mean(), np.median(delta[:, 3]), delta[:, 3].max(), raw[:, 3].max()))
    assert got.shape == (res3[0] * res3[1] * res3[2],) and (ratio <= 1.0).all(), float(ratio.max())


def test_composite_bound_and_regime(trained, ss, small_scene):
    name, m, net = trained; sc = small_scene; ob = sc.objects[0]
    aabb = np.stack([-ob["half"], ob["half"]]).astype(np.float32)
    rect, score = rref.choose_crop(sc, 0, CROP)
    smp = rref.samples(sc, rect, ob["Tow"], aabb, ob["cls"], int(m.cfg.sample_seed))
    hit = smp["hit"]; P = hit.size
    assert P == CROP * CROP and score >= 100, (rect, score)
    O = np.zeros((P, 64, 4), np.uint16); O[hit] = oracle_O(m, net["params"], smp["u"][hit])[1].reshape(-1, 64, 4)
    cr = rref.composite_render64(O, smp["t"], hit, smp["dn"])
    # the image against orc_render at the bars of test_render_matches_oracle_and_golden (the NumPy ray rows differ from the oracle's in the last bit)
    orgb, odepth, omask = m.render(rect, ss.colmajor(sc.Twc[int(rect[0])]))
    orgb = orgb.reshape(-1, 3); odepth = odepth.reshape(-1); omask = omask.reshape(-1)
    ok = ~cr["amb"]; same = ok & (cr["mask"] == omask)
    flips = float((cr["mask"] != omask)[ok].mean())
    print("%s: composite: flips %.4g, rgb %.3g, depth %.3g, ambiguous %d of %d hit rays" % (
        name, flips, np.abs(cr["rgb"] - orgb)[same].max(), np.abs(cr["depth"] - odepth)[same].max(), cr["amb"].sum(), hit.sum()))
    assert flips < 5e-3 and (cr["mask"] > 0).sum() >= 100
    assert np.abs(cr["rgb"] - orgb)[same].max() < 4e-3 and np.abs(cr["depth"] - odepth)[same].max() < 4e-3
    assert cr["amb"].sum() <= 0.01 * hit.sum()
    # the counted bound with factor 1: the oracle's fp32 composite_ray (white background) on the same O and the same t
    rgb = np.zeros((P, 3), np.float32); dep = np.zeros(P, np.float32); msk = np.zeros(P, np.float32); bg = np.ones(3, np.float32)
    t32 = np.ascontiguousarray(smp["t"], np.float32)
    for i in np.flatnonzero(hit):
        m.L.orc_composite(P_(O[i]), P_(t32[i]), 64, P_(bg), P_(rgb[i]), P_(dep[i:i + 1]), P_(msk[i:i + 1]))
    j = hit & ok
    e_op = cr["e_T"] + sr.U * (1.0 - cr["T"])
    use = [np.abs(rgb - cr["r"])[j] / cr["e_r"][j], np.abs(dep - cr["dep"])[j] / cr["e_dep"][j], np.abs(msk - (1.0 - cr["T"]))[j] / e_op[j]]
    print("%s: bound: share used, worst: rgb %.3f, depth %.3f, 1 - T %.3f (median %.3g / %.3g / %.3g)" % (
        name, use[0].max(), use[1].max(), use[2].max(), np.median(use[0]), np.median(use[1]), np.median(use[2])))
    assert all((q <= 1.0).all() for q in use), [float(q.max()) for q in use]
    # the regime from the reference's wanted values
    raw = np.zeros((P, 64, 4)); raw[hit] = rref.raw_bounds(net, smp["u"][hit].reshape(-1, 3))[0].reshape(-1, 64, 4)
    rg = rref.chain_regime(raw, smp["t"], hit, smp["dn"])
    print(name, "regime", rg)
    assert rg["raw_max"] >= sr.REGIME_BARS["raw_max"] and rg["cut_share"] >= sr.REGIME_BARS["cut_share"], rg
    assert min(rg["n_in"], rg["n_out"], rg["n_miss"]) >= 100 and rg["n_amb"] <= 0.01 * rg["n_hit"], rg
    # slab_edge sets aside at most 1 % of the crop and no ray the slab test decides by a wide margin
    edge = rref.slab_edge(sc, int(rect[0]), ob["Tow"], aabb, smp)
    assert edge.sum() <= 0.01 * P and not edge[hit & ((smp["t1"] - smp["t0"]) > 1e-3)].any()
