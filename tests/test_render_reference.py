"""The render-list reference of tests/render_reference.py judged with the CPU ORACLE in the device's place (no GPU): the oracle is trained 150 steps at c1 and
c2s, and at its EMA weights the reference's raw outputs, bound, lists, count rule and regime are checked on one 24 x 24 crop before any GPU time is spent
(tests/test_render_lists.py holds the device to the same reference).

Figures of this file on the oracle (150 steps; printed with -s):
  raw within delta   c1: worst |diff| / delta 0.30, median 0; c2s: worst 0.40, median 0 (99.9 % of the elements are the same fp16 number); delta on a raw
                     output 0.04 (c1) and 0.013 (c2s) at the median
  regime             c1: raw3 max 11.4, 39 % of 410 hit rays cut after tile 0, 161 / 249 / 166 rays of count 32 / 64 / 0; c2s: 8.4, 36 %, 149 / 261 / 166
  image              the reference's own lists composited by np_composite against orc_render: no mask flip, rgb within 1.6e-7 (c1) and 7.5e-4 (c2s; the NumPy
                     ray rows differ from the oracle's in the last bit), depth within 2.7e-5 (bars 4e-3), no ambiguous ray
(the oracle's training trajectory moves with the number of threads it sums its weight gradient over: the figures move in the last digit)"""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import field_grad_reference as fgr
import pose_reference as pr
import render_reference as rref
import scene_pose_reference as spr
import stage_reference as sr
from parity import CFGS
from test_scene_render import np_composite

STEPS = 150
CROP = 24


@pytest.fixture(scope="module", params=sorted(CFGS))
def trained(request, orc, small_scene):
    """(name, the oracle after 150 steps, the network dict of its EMA weights)"""
    kw = CFGS[request.param]
    m = ge.make_oracle(orc, small_scene, kw); m.train(STEPS)
    off, scl, res = pr.level_table(orc, m.cfg)
    net = fgr.net_of(m.buffer("ema").copy(), off, scl, res, m.cfg.n_levels, m.W, m.NH)
    assert net["n_mlp"] == m.n_mlp and net["Ep"] == m.Epad
    yield request.param, m, net
    m.close()


def _oracle_raw(m, params_u16, u):
    """orc_encode + orc_mlp_forward at unit-cube points u (n, 3) on the fp16 parameter vector given: raw outputs (n, 4) in fp64"""
    u = np.ascontiguousarray(u, np.float32); n = u.shape[0]; prm = np.ascontiguousarray(params_u16, np.uint16)
    E = np.zeros(n * m.Epad, np.uint16); hid = np.zeros(n * m.W * m.NH, np.uint16); O = np.zeros(n * 4, np.uint16)
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    m.L.orc_encode(m.h, P(prm), P(u), n, P(E)); m.L.orc_mlp_forward(m.h, P(prm), P(E), n, P(hid), P(O))
    return sr.h2d(O).reshape(n, 4)


def test_fma_and_closed_forms():
    """fma32 rounds once where mul + add rounds twice; the count rule on rays done by hand; alpha at the saturated and the vanishing end"""
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)
    assert rref.fma32(a, b, c) == np.float32(2.0 ** -11 + 2.0 ** -24) and np.float32(a * b) + c == np.float32(2.0 ** -11)
    al = np.zeros((4, 64)); al[1, 3] = 1.0; al[2, :32] = 1.0 - sr.EPS ** (1.0 / 32) * (1 - 1e-5); al[3, 40] = 1.0
    cnt, amb, _ = rref.count_rule(al, np.array([True, True, True, False]))
    assert list(cnt) == [64, 32, 32, 0] and list(amb) == [False, False, True, False]
    v, e = rref.alpha_of(np.array([12.0, -30.0]), np.array([0.01, 0.01]))
    assert v[0] == 1.0 and 0 < v[1] < 2.0 ** -40 and (e < 1e-6).all()
    assert np.array_equal(rref.intervals_dt(np.array([[1.0, 1.5, 3.0] + [3.0] * 61]))[0, :4], [1.0, 0.5, 1.5, 0.0])


def test_reference_against_the_oracle_at_trained_weights(trained, ss, small_scene):
    name, m, net = trained; sc = small_scene; ob = sc.objects[0]
    aabb = np.stack([-ob["half"], ob["half"]]).astype(np.float32)
    rect, score = rref.choose_crop(sc, 0, CROP)
    smp = rref.samples(sc, rect, ob["Tow"], aabb, ob["cls"], int(m.cfg.sample_seed))
    hit = smp["hit"]; P = hit.size
    assert P == CROP * CROP and score >= 100, (rect, score)
    # (b): every raw output of the hit rays within delta of the oracle's at the same points
    u = smp["u"][hit].reshape(-1, 3)
    assert (u >= -1e-6).all() and (u <= 1 + 1e-6).all()                                   # (an end point of the slab may round just outside the cube)
    raw_h, delta_h = rref.raw_bounds(net, u)
    assert np.array_equal(raw_h, fgr.forward(net, fgr.gather(net, u))[0])                 # the bound's own forward is field_grad_reference's
    got = _oracle_raw(m, net["params"], u)
    ratio = np.abs(got - raw_h) / delta_h
    print("%s: crop %s, %d hit rays; |oracle - want| / delta worst %.3f median %.3g; equal fp16 on %.5f; delta median %.3g worst %.3g" % (
        name, list(rect), hit.sum(), ratio.max(), np.median(ratio), (got == raw_h).mean(), np.median(delta_h), delta_h.max()))
    assert (ratio <= 1.0).all(), float(ratio.max())
    # the position term only widens the bound
    _, d2 = rref.raw_bounds(net, u[:4096], smp["pos_err"][hit].reshape(-1, 3)[:4096])
    assert (d2 >= delta_h[:4096]).all() and (smp["pos_err"] > 0).all() and smp["pos_err"][hit].max() < 1e-5
    # (c): the reference's own lists, its count rule against scene_pose_reference.lists_from_raw, the regime and ambiguity conditions of the GPU test
    raw = np.zeros((P, 64, 4)); raw[hit] = raw_h.reshape(-1, 64, 4)
    alpha, col, count, amb = rref.reference_lists(raw, smp["t"], hit)
    a2, c2, n2 = spr.lists_from_raw(raw, smp["t"], hit)
    assert np.array_equal(alpha[hit], a2[hit]) or np.abs(alpha[hit] - a2[hit]).max() < 1e-15
    assert np.array_equal(count[~amb], n2[~amb]) and np.allclose(col, c2, rtol=0, atol=1e-15)
    rg = rref.regime(raw, alpha, count, hit)
    print(name, "regime", rg, "ambiguous", int(amb.sum()))
    assert rg["raw_max"] >= sr.REGIME_BARS["raw_max"] and rg["cut_share"] >= sr.REGIME_BARS["cut_share"], rg
    assert min(rg["n0"], rg["n32"], rg["n64"]) >= 100, rg
    assert amb.sum() <= 0.01 * hit.sum()
    # every activation interval holds its own wanted value and has a positive width
    a_lo, a_hi, c_lo, c_hi = rref.intervals(raw[hit], np.zeros_like(raw[hit]), rref.intervals_dt(smp["t"][hit]))
    assert (a_lo < alpha[hit]).all() and (alpha[hit] < a_hi).all() and (c_lo < col[hit]).all() and (col[hit] < c_hi).all()
    # the image: np_composite of the reference's lists against orc_render, within the bars of test_render_matches_oracle_and_golden
    out = np_composite(smp["t"][None], alpha[None], col[None], count[None], smp["dn"].astype(np.float64))
    rgb, depth, op, amb_c = out[0], out[1], out[2], out[5]
    orgb, odepth, omask = m.render(rect, ss.colmajor(sc.Twc[int(rect[0])]))
    ok = ~(amb_c | amb); mask = op > 0.5
    rgb = np.where(mask[:, None], rgb, 1.0); depth = np.where(mask, depth, 0.0)
    omask = omask.reshape(-1) > 0.5; same = ok & (mask == omask)
    flips = float((mask != omask)[ok].mean())
    print("%s: image: flips %.4g, rgb %.3g, depth %.3g, ambiguous %d" % (name, flips, np.abs(rgb - orgb.reshape(-1, 3))[same].max(),
                                                                       np.abs(depth - odepth.reshape(-1))[same].max(), int((~ok).sum())))
    assert flips < 5e-3 and mask.sum() >= 100
    assert np.abs(rgb - orgb.reshape(-1, 3))[same].max() < 4e-3 and np.abs(depth - odepth.reshape(-1))[same].max() < 4e-3
