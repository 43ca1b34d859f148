"""GPU tests (-m gpu) of pose refinement at every fused shape and past one grid pass (k_pose_rays, k_pose_grad, k_pose_update in kernels_pose.hip),
against the shared fp64 reference of tests/pose_reference.py: the numpy restatement of the drawn rays and the fp64 torch autograd graph of the objective.

Bars (the project's, as in test_pose_refine / test_pose_c2f): positions <= 1e-5 absolute; loss <= 1e-4 relative to fp64; grad6 relative error <= 1e-2;
>= 99.9 % of samples within 2e-2 relative of the fp64 dL/dx, with a floor of 1 % of the largest sample (dL/dO, dL/dh and dL/dE are fp16 in the kernel).
Each case must reach the edges: >= 10 rays that miss the box, that are cut inside tile 0, that evaluate tile 1, with m* = 0 and a hit, and (perturbed
pose with depth) in the Huber linear and quadratic branches.  Every case prints one `POSE_CASE` line (the table of DESIGN.md 3.4d)."""
import math

import numpy as np
import pytest

import __graft_entry__ as ge
import pose_reference as pref

pytestmark = pytest.mark.gpu

# (Epad, W, NH, L): all ten fused instantiations, odd L in both encoder groups; (32, 32, 2, 16) and (32, 64, 1, 16) are test_pose_refine's anchors
SHAPES = [(16, 32, 1, 5), (16, 32, 2, 8), (16, 64, 1, 7), (16, 64, 2, 3), (16, 128, 1, 6),
          (32, 32, 1, 9), (32, 32, 2, 16), (32, 64, 1, 16), (32, 64, 2, 13), (32, 128, 1, 11)]
DRAWN, DRAWN_IT = 2048, 7
MIN_EDGE = 10


def _sid(s):
    return "E%d_%dx%d_L%d" % s


@pytest.fixture(scope="module")
def scene(ss):
    return ss.make_scene(n_views=24, H=240, W=320, f=260.0, seed=3)


@pytest.fixture(scope="module")
def objects(pkg, scene):
    """one object per fused shape, 500 iterations with use_depth on the true pose (published: side 1 holds the same EMA)"""
    sc = scene; ds = None; objs = {}
    for j, (E, W, NH, L) in enumerate(SHAPES):
        ds, o = ge.make_problem(pkg, sc, dict(sample_seed=20 + j, n_levels=L, n_neurons=W, n_hidden_layers=NH), use_depth=True, dataset=ds)
        o.set_backend(1); o.train(500)
        assert o.info().encoded_width == E, (E, W, NH, L, o.info().encoded_width)
        objs[(E, W, NH, L)] = o
    yield objs
    for o in objs.values():
        o.close()
    ds.close()


def _perturb(T, rot_deg, trans, seed):
    rs = np.random.RandomState(seed)
    ax = rs.normal(size=3); ax /= np.linalg.norm(ax); d = rs.normal(size=3); d /= np.linalg.norm(d)
    th = math.radians(rot_deg); K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    D = np.eye(4); D[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K; D[:3, 3] = d * trans
    return D @ T


def _poses(sc):
    """the true pose and one perturbed by 5 degrees and 5 % of the box diagonal (at test_pose_refine's 3 degrees / 3 % only 4-10 rays of the crops reach
    the Huber linear branch)"""
    ob = sc.objects[0]; diag = float(np.linalg.norm(2 * ob["half"]))
    return [("true", ob["Tow"]), ("pert", _perturb(ob["Tow"], 5.0, 0.05 * diag, seed=11))]


def _aabb(sc):
    return np.stack([-sc.objects[0]["half"], sc.objects[0]["half"]]).astype(np.float32)


def _pad(sc, box, pad):
    v, x, y, h, w = (int(q) for q in box)
    x0, y0 = max(0, x - pad), max(0, y - pad); x1, y1 = min(sc.W, x + w + pad), min(sc.H, y + h + pad)
    return (v, x0, y0, y1 - y0, x1 - x0)


def _six_padded(sc, pad=16):
    b = sc.objects[0]["boxes"]
    return np.array([_pad(sc, q, pad) for q in b[np.linspace(0, len(b) - 1, 6).astype(int)]], np.uint32)


def _straddle(sc, views=(2, 11), size=32):
    """32 x 32 crops centred 10 px inside the left edge of the object's 2-D box in two views, where the 3-D box's outline runs: about half of their
    rays miss the 3-D box"""
    boxes = {int(b[0]): b for b in sc.objects[0]["boxes"]}; out = []
    for v in views:
        _, x, y, h, w = (int(q) for q in boxes[v])
        out.append((v, min(max(x + 10 - size // 2, 0), sc.W - size), min(max(y + h // 2 - size // 2, 0), sc.H - size), size, size))
    return np.array(out, np.uint32)


def _border_box(sc):
    """view 3's box padded by 40 px: it touches the image border"""
    b = {int(q[0]): q for q in sc.objects[0]["boxes"]}[3]
    box = _pad(sc, b, 40)
    assert box[2] == 0 or box[1] == 0 or box[2] + box[3] == sc.H or box[1] + box[4] == sc.W, box
    return np.array([box], np.uint32)


def _evaluate(pkg, sc, o, boxes, Tow, n_rays, side=0, lw=None, use_depth=True):
    """device loss / grad6 / per-sample dump of one evaluation, and the numpy restatement of its rays"""
    prm = pkg.pose_refine_default(rays_per_iter=n_rays); it = DRAWN_IT if n_rays else 0
    T16 = sc_colmajor(Tow)
    if lw is None:
        loss, g6 = o.pose_loss(boxes, T16, prm, side=side, iteration=it)
    else:
        loss, g6 = o.pose_loss_levels(boxes, T16, lw, prm, side=side, iteration=it)
    x, raw, dldx = o.pose_samples(boxes, T16, prm, side=side, iteration=it)
    rr = pref.pose_rays(sc, boxes, Tow, _aabb(sc), sc.objects[0]["cls"], n_rays=n_rays, seed=prm.seed, iteration=it,
                        sample_seed=o.cfg.sample_seed, use_depth=use_depth)
    return dict(loss=loss, g6=g6, x=x, raw=raw, dldx=dldx, rr=rr, prm=prm, lw=lw, aabb=_aabb(sc))


def sc_colmajor(T):
    return ge.load_tools().colmajor(T)


def _grazing(rr):
    """rays whose restated slab is within 1e-4 of empty: positions agree to ~1e-6 only, so the device may decide them either way"""
    return np.abs(rr["t1"] - rr["t0"]) <= 1e-4


def _check_cases(tag, pkg, orc, o, cases, tmp_path, huber):
    """runs the fp64 reference on every case of one object, prints the table row of each, asserts the bars and the edge counts"""
    prm = cases[0][1]["prm"]
    refs = pref.reference(tmp_path, pref.net_inputs(o, orc, prm), cases[0][1]["aabb"],
                          [dict(x=c["x"], t=c["rr"]["t"], hit=c["rr"]["hit"], dn=c["rr"]["dn"], tgt=c["rr"]["tgt"], lw=c["lw"]) for _, c in cases],
                          tag=tag)
    failures = []
    for (name, c), ref in zip(cases, refs):
        rr = c["rr"]; N = c["x"].shape[0]; hit = rr["hit"]; ev = ref["ev"]
        dev_hit = np.any(c["x"] != 0, axis=(1, 2)); ev = ev & dev_hit[:, None]
        flags_ok = not (dev_hit != hit)[~_grazing(rr)].any()
        pos_err = float(np.abs(c["x"][ev] - rr["pos"][ev]).max()) if ev.any() else 0.0
        loss_rel = abs(c["loss"] - ref["loss"]) / abs(ref["loss"])
        g6_rel = float(np.linalg.norm(c["g6"] - ref["g6"]) / np.linalg.norm(ref["g6"]))
        share = float("nan")
        if c["lw"] is None:
            ws = ref["gs"][ev] / N; gs = c["dldx"][ev]
            scale = np.linalg.norm(ws, axis=-1).max()
            ok = np.linalg.norm(gs - ws, axis=-1) <= 2e-2 * np.maximum(np.linalg.norm(ws, axis=-1), 1e-2 * scale)
            share = float(ok.mean())
        m, d = rr["tgt"][:, 3], rr["tgt"][:, 4]
        dep_on = hit & (m > 0) & (d > 0); err = np.abs(ref["D"] - d)
        cnt = dict(miss=int((~hit).sum()), cut0=int((hit & ~ref["ev1"]).sum()), tile1=int(ref["ev1"].sum()), m0hit=int((hit & (m == 0)).sum()),
                   lin=int((dep_on & (err > prm.depth_huber)).sum()), quad=int((dep_on & (err <= prm.depth_huber)).sum()))
        print("POSE_CASE %s %s rays %d | pos %.1e loss %.2e grad6 %.2e share %.5f | miss %.3f cut0 %.3f tile1 %.3f m0hit %.3f lin %.3f quad %.3f | %s" % (
              tag, name, N, pos_err, loss_rel, g6_rel, share, *(v / N for v in cnt.values()), " ".join("%s=%d" % kv for kv in cnt.items())))
        need = ["miss", "cut0", "tile1", "m0hit"] + (["lin", "quad"] if huber and name.startswith("pert") else [])
        checks = [("hit flags", flags_ok), ("positions", pos_err <= 1e-5), ("loss", loss_rel <= 1e-4), ("grad6", g6_rel <= 1e-2),
                  ("per-sample", c["lw"] is not None or share >= 0.999)] + [("count " + k, cnt[k] >= MIN_EDGE) for k in need]
        failures += ["%s %s: %s" % (tag, name, what) for what, good in checks if not good]
    assert not failures, failures


def _straddle_checked(sc):
    boxes = _straddle(sc); ob = sc.objects[0]
    for _, Tow in _poses(sc):
        rr = pref.pose_rays(sc, boxes, Tow, _aabb(sc), ob["cls"])
        miss = 1 - rr["hit"].mean()
        print("straddling crops %s: %.3f of the rays miss the box" % (boxes.tolist(), miss))
        assert 0.2 <= miss <= 0.8, miss
    return boxes


# ------------------------------------------------------------------ 1. every fused shape, both modes, true and perturbed pose
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_shape_matches_fp64_autograd(pkg, orc, scene, objects, shape, tmp_path):
    sc = scene; o = objects[shape]
    crops = _straddle_checked(sc); six = _six_padded(sc)
    cases = []
    for pname, Tow in _poses(sc):
        cases.append((pname + " crops", _evaluate(pkg, sc, o, crops, Tow, 0)))
        cases.append((pname + " drawn", _evaluate(pkg, sc, o, six, Tow, DRAWN)))
    _check_cases(_sid(shape), pkg, orc, o, cases, tmp_path, huber=True)


# ------------------------------------------------------------------ 2. level weights (odd L, fractional window), no depth, side 1
def _window(L, alpha):
    a = alpha - np.arange(L, dtype=np.float64)
    return np.where(a <= 0, 0.0, np.where(a >= 1, 1.0, (1 - np.cos(np.pi * np.clip(a, 0, 1))) / 2))


@pytest.mark.parametrize("shape", [(16, 64, 1, 7), (32, 32, 1, 9)], ids=_sid)
def test_level_weighted_odd_L(pkg, orc, scene, objects, shape, tmp_path):
    """The window at alpha = L / 2 + 2 (5.5 for L = 7, 6.5 for L = 9): one level in the ramp at weight 0.5, levels at 1 below it and at 0 above it, the
    three of them among the upper half-wave's levels, where the lane map of an odd L matters.  Loss, positions and grad6 against the weighted graph."""
    sc = scene; o = objects[shape]; L = shape[3]
    w = _window(L, L / 2 + 2).astype(np.float32)
    assert (w > 0).any() and (w == 0).any() and ((w > 0) & (w < 1)).any()
    crops = _straddle_checked(sc)
    cases = [(pname + " crops w", _evaluate(pkg, sc, o, crops, Tow, 0, lw=w)) for pname, Tow in _poses(sc)]
    _check_cases(_sid(shape) + "_lw", pkg, orc, o, cases, tmp_path, huber=True)


def test_dataset_without_depth(pkg, orc, scene, tmp_path):
    """base.json's shape on a dataset without depth (d* = 0, so no depth term), drawn rays over a box that touches the image border"""
    sc = scene
    ds, o = ge.make_problem(pkg, sc, dict(sample_seed=41), use_depth=False)
    try:
        o.set_backend(1); o.train(500)
        box = _border_box(sc)
        cases = [(pname + " drawn border", _evaluate(pkg, sc, o, box, Tow, DRAWN, use_depth=False)) for pname, Tow in _poses(sc)]
        assert all(np.all(c["rr"]["tgt"][:, 4] == 0) for _, c in cases)
        _check_cases("nodepth_E32_64x1_L16", pkg, orc, o, cases, tmp_path, huber=False)
    finally:
        o.close(); ds.close()


def test_side_1(pkg, orc, scene, objects, tmp_path):
    sc = scene; shape = (16, 32, 2, 8); o = objects[shape]
    crops = _straddle_checked(sc)
    cases = [(pname + " crops side1", _evaluate(pkg, sc, o, crops, Tow, 0, side=1)) for pname, Tow in _poses(sc)]
    _check_cases(_sid(shape) + "_side1", pkg, orc, o, cases, tmp_path, huber=True)


# ------------------------------------------------------------------ 3. a union above 2^24 pixels
def test_large_union_draw(pkg, scene, objects):
    """256 boxes naming one full frame (19 660 800 px), 4096 drawn rays: the device's samples are the restated wider draw's, and that draw puts rays on
    pixels the 24-bit draw can never reach"""
    sc = scene; o = objects[(16, 32, 1, 5)]; ob = sc.objects[0]
    boxes = np.array([(3, 0, 0, sc.H, sc.W)] * 256, np.uint32); total = 256 * sc.H * sc.W
    prm = pkg.pose_refine_default(rays_per_iter=4096)
    x, _, _ = o.pose_samples(boxes, sc_colmajor(ob["Tow"]), prm, iteration=0)
    rr = pref.pose_rays(sc, boxes, ob["Tow"], _aabb(sc), ob["cls"], n_rays=4096, seed=prm.seed, iteration=0, sample_seed=o.cfg.sample_seed)
    hit = rr["hit"] & ~_grazing(rr); dev_hit = np.any(x != 0, axis=(1, 2)) & ~_grazing(rr)
    unreachable = ~pref.reachable24(rr["p"], total)
    moved = hit & (rr["p"] != pref.draw24(prm.seed, 0, 4096, total).astype(np.int64))
    err = float(np.abs(x[hit] - rr["pos"][hit]).max())
    print("large union: %d hits, %d drawn pixels the 24-bit draw cannot reach, %d hits on a pixel other than the 24-bit draw's, positions %.1e" % (
          hit.sum(), unreachable.sum(), moved.sum(), err))
    assert np.array_equal(dev_hit, hit)
    assert err <= 1e-5
    assert unreachable.sum() >= 1
    assert moved.sum() >= MIN_EDGE                                      # (so that the position check can tell the two draws apart)
    # more than 2^28 pixels together: MON_ERR_ARG before any device work
    too_many = np.array([(3, 0, 0, sc.H, sc.W)] * (pref.MAX_UNION // (sc.H * sc.W) + 1), np.uint32)
    with pytest.raises(pkg.MonError) as e:
        o.pose_loss(too_many, sc_colmajor(ob["Tow"]), prm)
    assert e.value.code == 1


# ------------------------------------------------------------------ 4. past one grid pass (1024 blocks x 4 waves = 4096 rays)
NS = [1, 3, 4095, 4096, 4097, 12289, 1 << 18]
U = 2.0 ** -24


def _grad6_sums(x, g):
    """fp64 sum of the dumped per-sample terms (already x 1/N) and of their magnitudes, per grad6 component, chunked"""
    want = np.zeros(6); mag = np.zeros(6)
    n = x.shape[0]
    for s in range(0, n, 16384):
        xx = x[s:s + 16384].reshape(-1, 3).astype(np.float64); gg = g[s:s + 16384].reshape(-1, 3).astype(np.float64)
        want[:3] += gg.sum(0); mag[:3] += np.abs(gg).sum(0)
        want[3:] += np.cross(xx, gg).sum(0)
        mag[3] += (np.abs(xx[:, 1] * gg[:, 2]) + np.abs(xx[:, 2] * gg[:, 1])).sum()
        mag[4] += (np.abs(xx[:, 2] * gg[:, 0]) + np.abs(xx[:, 0] * gg[:, 2])).sum()
        mag[5] += (np.abs(xx[:, 0] * gg[:, 1]) + np.abs(xx[:, 1] * gg[:, 0])).sum()
    return want, mag


def _loss_restated(raw, rr, w):
    tot = 0.0
    for s in range(0, raw.shape[0], 16384):
        sl = slice(s, s + 16384)
        tot += pref.composite_loss(raw[sl], rr["t"][sl], rr["hit"][sl], rr["dn"][sl], rr["tgt"][sl], w).sum()
    return tot / raw.shape[0]


def _pass_checks(name, N, loss, g6, x, raw, dldx, rr, prm):
    hit = rr["hit"] & ~_grazing(rr); dev_hit = np.any(x != 0, axis=(1, 2)) & ~_grazing(rr)
    err = float(np.abs(x[hit] - rr["pos"][hit]).max()) if hit.any() else 0.0
    want_l = _loss_restated(raw, rr, [prm.w_rgb, prm.w_mask, prm.w_depth, prm.depth_huber])
    want6, mag = _grad6_sums(x, dldx)
    bound = (2 * math.ceil(N / 4096) + 96) * U * mag
    print("PASS %s N %d: hits %d positions %.1e loss %.7f restated %.7f (rel %.1e) | grad6 err/bound %s" % (
          name, N, hit.sum(), err, loss, want_l, abs(loss - want_l) / abs(want_l), np.array2string(np.abs(g6 - want6) / bound, precision=3)))
    assert np.array_equal(dev_hit, hit), name
    assert err <= 1e-5, (name, err)
    assert abs(loss - want_l) <= 1e-4 * abs(want_l), (name, loss, want_l)
    assert np.all(np.abs(g6 - want6) <= bound), (name, g6, want6, bound)


def test_past_one_grid_pass(pkg, orc, scene, objects, tmp_path):
    """base.json's shape at the perturbed pose, drawn N rays over the six padded boxes at iteration 0, then every pixel of one padded box.  N = 1's loss is
    ray 0's alone, so the evaluation is one where ray 0 hits the object (m* = 1, d* > 0; asserted from the restatement): a ray with m* = 0 through empty
    space has a loss of O^2 ~ 1e-14, at the fp32 resolution of O = 1 - T_end, where no relative bar can hold."""
    sc = scene; o = objects[(32, 64, 1, 16)]; ob = sc.objects[0]
    six = _six_padded(sc); Tow = _poses(sc)[1][1]; T16 = sc_colmajor(Tow); it = 0
    r0 = pref.pose_rays(sc, six, Tow, _aabb(sc), ob["cls"], n_rays=1, seed=pkg.pose_refine_default().seed, iteration=it)
    assert r0["hit"][0] and r0["tgt"][0, 3] == 1 and r0["tgt"][0, 4] > 0
    prev = None; later = []
    for N in NS:
        prm = pkg.pose_refine_default(rays_per_iter=N)
        loss, g6 = o.pose_loss(six, T16, prm, iteration=it)
        x, raw, dldx = o.pose_samples(six, T16, prm, iteration=it)
        rr = pref.pose_rays(sc, six, Tow, _aabb(sc), ob["cls"], n_rays=N, seed=prm.seed, iteration=it, sample_seed=o.cfg.sample_seed)
        _pass_checks("drawn", N, loss, g6, x, raw, dldx, rr, prm)
        if prev is not None:                                                         # rays i < N of two draws: the same rays
            M0, x0, raw0, g0 = prev
            assert np.array_equal(x[:M0].view(np.uint32), x0.view(np.uint32)) and np.array_equal(raw[:M0].view(np.uint32), raw0.view(np.uint32)), (M0, N)
            # the dumps differ only by their 1/N rounding: divided by the kernel's own fp32 1/N, each is gf (1 + d), |d| <= 2^-24
            a = g0.astype(np.float64) / np.float64(np.float32(1.0) / np.float32(M0)); b = dldx[:M0].astype(np.float64) / np.float64(np.float32(1.0) / np.float32(N))
            ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
            worst = float((np.abs(a - b) / ulp).max())
            print("prefix %d of %d: dL/dx x N within %.2f ulp" % (M0, N, worst))
            assert worst <= 2.0, worst
        if N in (12289, 1 << 18):
            rs = np.random.RandomState(N)
            pool = np.nonzero(rr["hit"] & (np.arange(N) >= 4096))[0]
            sel = np.sort(rs.choice(pool, 1024, replace=False))
            later.append((N, sel, x[sel], dldx[sel], {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (N,) else v) for k, v in rr.items()}))
        prev = (N, x, raw, dldx)
        del x, raw, dldx, rr
    prev = None
    # rays_per_iter = 0 on one padded training box (every pixel, in order)
    box = six[:1]; prm = pkg.pose_refine_default(rays_per_iter=0)
    loss, g6 = o.pose_loss(box, T16, prm)
    x, raw, dldx = o.pose_samples(box, T16, prm)
    rr = pref.pose_rays(sc, box, Tow, _aabb(sc), ob["cls"], sample_seed=o.cfg.sample_seed)
    assert x.shape[0] > 4096 * 4
    _pass_checks("box", x.shape[0], loss, g6, x, raw, dldx, rr, prm)
    del x, raw, dldx, rr
    # autograd on 1024 rays of passes 2 and later
    prm = pkg.pose_refine_default()
    refs = pref.reference(tmp_path, pref.net_inputs(o, orc, prm), _aabb(sc),
                          [dict(x=xs, t=r["t"], hit=r["hit"], dn=r["dn"], tgt=r["tgt"]) for _, _, xs, _, r in later], tag="later")
    for (N, sel, xs, gs, r), ref in zip(later, refs):
        ev = ref["ev"]
        assert np.abs(xs[ev] - r["pos"][ev]).max() <= 1e-5
        ws = ref["gs"][ev] / N; g = gs[ev]
        scale = np.linalg.norm(ws, axis=-1).max()
        ok = np.linalg.norm(g - ws, axis=-1) <= 2e-2 * np.maximum(np.linalg.norm(ws, axis=-1), 1e-2 * scale)
        print("PASS later N %d: rays %d..%d, per-sample within bar %.5f of %d" % (N, sel[0], sel[-1], ok.mean(), ok.size))
        assert ok.mean() >= 0.999, ok.mean()
