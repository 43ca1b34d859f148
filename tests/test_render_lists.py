"""GPU tests (-m gpu) of what k_fused_render<EMIT> puts into an object's sample list at TRAINED weights, against the fp64 reference of
tests/render_reference.py (tests/test_render_reference.py holds that reference to the CPU oracle first).

Every other check of the inference side compares kernels with each other, or composites lists the device itself produced; the only independent one runs at
the pattern parameters, where raw density is of order +-1 and no ray is cut.  Here seven objects, one per instantiation family of MON_FUSED_DISPATCH, are
trained 300 steps on the device (use_depth, backend 1), and one 48 x 48 crop of each is dumped through mon_debug_scene_samples and compared sample by sample:
  (d) t bit for bit with fmaf(dtr, k + jitter, t0) on the object's own ray rows (mon_debug_scene_probe_rays at the integer queries: the fp32 NumPy
      restatement of pixel_ray sums in another order and does not reproduce t0 / t1 to the bit), count 0 exactly where the independent restatement misses
      the box, t ascending
  (e) alpha and each colour inside the interval of render_reference.intervals: the fp64 network at the restated point, a counted first-order bound on the
      device's raw outputs, the counted activation bound; no sample is excluded
  (f) the count equals render_reference.count_rule of the device's OWN tile-0 alphas; ambiguous rays (T32 within 0.1 % of the cut) at most 1 % of the hits
  (g) with render skipping on every sample keeps its bits or keeps its t with alpha and colour exactly 0; counts follow (f)
  (h) side 1 after train() equals side 0 bit for bit
  (i) slot 32 of every ray with count 64 uses t[32] - t[31]: the wanted alpha with dt = t[32] lies outside the interval on at least 100 samples
and, on base.json and 32 x 2, the cross-route tie: mon_debug_pose_samples (k_pose_grad, another kernel on the same tile_forward) returns the same positions
bit for bit and raw outputs from which the render's alpha and colours follow within the activation bound alone.
One more case renders a 129 x 128 rect of base.json (two passes of kRenderChunkRays) and checks 1 500 of its rays, the 128 of the second pass among them.
The regime (raw3 max >= 6, >= 25 % of hit rays cut after tile 0, >= 100 rays of every count) is asserted from the reference's wanted values.

Measured on an MI355X (this file's output with -s; the table is DESIGN.md section 1, "Render lists at trained weights"):
  regime        base: raw3 max 15.1, 47.6 % of hit rays cut after tile 0, 770 / 730 / 804 rays of count 0 / 32 / 64, 4.8 % of the wanted alphas round to 1.0f,
                73.2 % lie below 2^-24;  32 x 2: 12.9, 47.4 %, 770 / 727 / 807, 2.8 %, 77.3 %;  128 x 1 L 16: 13.7, 47.4 %, 770 / 727 / 807, 3.4 %, 74.1 %;
                128 x 1 L 6: 15.9, 47.5 %, 770 / 728 / 806, 4.0 %, 73.9 %;  L 8 scale 1.5: 14.2, 47.7 %, 770 / 732 / 802, 3.3 %, 71.5 %;  T 2^14 L 8 base 8: 19.7,
                47.7 %, 770 / 731 / 803, 13.9 %, 72.2 %;  T 2^16 scale 2: 15.6, 47.7 %, 770 / 731 / 803, 4.6 %, 72.8 %;  129 x 128: 14.3, 39.4 %, 700 / 315 / 485
  (d)           the NumPy pixel_ray reproduces the device's t0 on 99.9 % of the hit rays (99.6 % at 129 x 128); on the device's rows every t, every miss, every count
  (e)           |got - want| / half-width: alpha worst 0.39-0.43, median 2e-6 to 1e-3; colour worst 0.12-0.18, median 2e-6 to 1e-5; delta on raw3 0.03-0.08 at the
                median, 0.15 at worst (32 x 2)
  (f)           no ambiguous ray in any case;  (g) 76 % of the emitted samples zeroed, no count moved;  (i) 156 (32 x 2) to 494 (L 8 scale 1.5) samples tell
  cross-route   positions equal bit for bit; 100 % of 74 816 / 74 912 samples inside the activation bound of the route's own raw, none needs the ulp; the route's
                raw equals the reference's fp16 number on 99.57 % / 99.44 %
  planted       (scratch builds) tprev = 0 at slot 32: (i), (e) and the tie fail;  idx_base of pass 2 short by 64: (d) of the two-pass case fails, 5 568 values;
                two colours swapped: (e) and the tie fail;  raw3 before its fp16 rounding: the tie's fp16 assertion fails, (e) holds (half an ulp)"""
import numpy as np
import pytest

import __graft_entry__ as ge
import field_grad_reference as fgr
import pose_reference as pr
import render_reference as rref
import stage_reference as sr

pytestmark = pytest.mark.gpu

CHUNK = 16384                # kRenderChunkRays
CROP = 48
# one shape per instantiation family of MON_FUSED_DISPATCH
SHAPES = {"base": dict(sample_seed=5),                                                       # base.json: 64 x 1, 16 levels, Epad 32
          "w32x2": dict(sample_seed=7, n_neurons=32, n_hidden_layers=2),
          "w128L16": dict(sample_seed=9, n_neurons=128),
          "w128L6": dict(sample_seed=11, n_neurons=128, n_levels=6),                         # Epad 16
          "L8s15": dict(sample_seed=13, n_levels=8, per_level_scale=1.5),
          "h14L8b8": dict(sample_seed=15, log2_hashmap_size=14, n_levels=8, base_resolution=8),
          "h16s2": dict(sample_seed=17, log2_hashmap_size=16, per_level_scale=2.0)}          # (a level that indexes by x alone)
CROSS = ("base", "w32x2")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(ss):
    return ss.make_scene(n_views=24, H=240, W=320, f=260.0, n_objects=3, seed=3, elev_deg=10.0)          # the scene-render tests' scene


@pytest.fixture(scope="module")
def objects(pkg, scene):
    """object 0 at every shape: use_depth, backend 1, 300 iterations (published: side 1 holds the same EMA)"""
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    ds = None; objs = {}
    for name, kw in SHAPES.items():
        ds, o = ge.make_problem(pkg, scene, kw, use_depth=True, dataset=ds)
        o.set_backend(1); loss = o.train(300); assert np.isfinite(loss), name
        objs[name] = o
    yield objs
    for o in objs.values():
        o.close()
    ds.close()


def _flat(lists, P):
    t, a, c, n = lists
    return t.reshape(P, 64), a.reshape(P, 64), c.reshape(P, 64, 3), n.reshape(P).astype(np.int64)


def _case(pkg, orc, ss, sc, o, rect, which=None):
    """One dump of the rect on side 0 with skipping off, and the reference on the rays `which` (all by default), computed once and left unchanged."""
    ob = sc.objects[0]; aabb = np.stack([-ob["half"], ob["half"]]).astype(np.float32)
    pose = ss.colmajor(sc.Twc[int(rect[0])]); P = int(rect[3]) * int(rect[4])
    idx = np.arange(P) if which is None else np.asarray(which, np.int64)
    o.set_render_skip(False)
    t, a, c, n = (v[idx] for v in _flat(pkg.scene_samples([o], rect, pose, 0, 0), P))
    q = pkg.rect_queries(rect)
    rows = pkg.scene_probe_rays([o], q[idx], pose, 0)
    own = pr.pose_rays(sc, [rect], ob["Tow"], aabb, ob["cls"], n_rays=0, sample_seed=int(o.cfg.sample_seed), which=idx)      # the independent ray rows
    smp = rref.samples(sc, rect, ob["Tow"], aabb, ob["cls"], int(o.cfg.sample_seed), which=idx, rows=rows)
    hit = smp["hit"]; net = fgr.net_of_object(o, orc)
    raw = np.zeros((idx.size, 64, 4)); delta = np.zeros((idx.size, 64, 4))
    r, d = rref.raw_bounds(net, smp["u"][hit].reshape(-1, 3)); raw[hit] = r.reshape(-1, 64, 4); delta[hit] = d.reshape(-1, 64, 4)
    want_a, want_c, want_n, want_amb = rref.reference_lists(raw, smp["t"], hit)
    return dict(o=o, rect=rect, pose=pose, P=P, idx=idx, t=t, a=a, c=c, n=n, valid=np.arange(64)[None, :] < n[:, None], rows=rows, own=own, smp=smp, hit=hit,
                raw=raw, delta=delta, want_a=want_a, want_c=want_c, want_n=want_n, want_amb=want_amb, net=net)


_cases = {}


def _shape_case(name, pkg, orc, ss, scene, objects):
    """the 48 x 48 crop of one shape: dumped and referenced once per module"""
    if name not in _cases:
        rect, score = rref.choose_crop(scene, 0, CROP)
        assert score >= 100, (rect, score)
        _cases[name] = _case(pkg, orc, ss, scene, objects[name], rect)
    return _cases[name]


@pytest.fixture(scope="module", params=sorted(SHAPES))
def case(request, pkg, orc, ss, scene, objects):
    return request.param, _shape_case(request.param, pkg, orc, ss, scene, objects)


def _two_pass_rect(sc):
    """the 129 x 128 rect (FrameId, x, y, h, w) whose last row -- the 128 rays of the second pass -- holds the most rays that hit object 0's box"""
    ob = sc.objects[0]; aabb = np.stack([-ob["half"], ob["half"]]).astype(np.float32); K4 = np.array([sc.fx, sc.fy, sc.cx, sc.cy]); best = None
    for b in ob["boxes"]:
        v, x, y, h, w = (int(q) for q in b)
        x0 = int(np.clip(x + w // 2 - 64, 0, sc.W - 128)); y0 = int(np.clip(y + h // 2 - 128, 0, sc.H - 129))
        o, d, _ = pr.camera_rays(K4, sc.Twc[v], ob["Tow"], np.arange(x0, x0 + 128), np.full(128, y0 + 128))
        n = int(pr.slab(aabb, o, d)[0].sum())
        if best is None or n > best[0]:
            best = (n, np.array([v, x0, y0, 129, 128], np.uint32))
    return best[1], best[0]


@pytest.fixture(scope="module")
def two_pass(pkg, orc, ss, scene, objects):
    rect, n_hit = _two_pass_rect(scene)
    assert n_hit >= 50, (rect, n_hit)
    which = np.sort(np.concatenate([np.random.RandomState(3).choice(CHUNK, 1500 - 128, replace=False), np.arange(CHUNK, CHUNK + 128)]))
    return "base-129x128", _case(pkg, orc, ss, scene, objects["base"], rect, which)


def _check_t_misses_counts(name, cs):
    """(d)"""
    hit, valid, smp = cs["hit"], cs["valid"], cs["smp"]
    same_rows = float((_bits(cs["own"]["t0"]) == _bits(smp["t0"]))[hit].mean())
    print("%s: (d) %d rays, %d hit; the NumPy pixel_ray reproduces the device's t0 bit for bit on %.3f of them" % (name, hit.size, hit.sum(), same_rows))
    assert set(np.unique(cs["n"])) <= {0, 32, 64}
    assert np.array_equal(cs["n"] == 0, ~cs["own"]["hit"]) and np.array_equal(hit, cs["own"]["hit"])
    assert np.array_equal(_bits(cs["t"])[valid], _bits(smp["t"])[valid]), int((_bits(cs["t"]) != _bits(smp["t"]))[valid].sum())
    step = np.diff(cs["t"].astype(np.float64), axis=1); inside = valid[:, 1:]
    assert (step[inside] >= 0).all() and (step[inside & ((smp["t1"] - smp["t0"]) > 1e-3)[:, None]] > 0).all()


def _ratio(got, want, lo, hi):
    """|got - want| over the half-width of the side it lies on"""
    with np.errstate(invalid="ignore", divide="ignore"):                      # (the rows of rays that miss the box hold nothing; the callers mask them)
        return np.where(got >= want, (got - want) / (hi - want), (want - got) / (want - lo))


def _check_alpha_colours(name, cs):
    """(e) and the regime"""
    valid = cs["valid"]; dt = rref.intervals_dt(cs["t"])
    a_lo, a_hi, c_lo, c_hi = rref.intervals(cs["raw"], cs["delta"], dt)
    want_a, _ = rref.alpha_of(cs["raw"][..., 3], dt); want_c, _ = rref.colour_of(cs["raw"][..., :3])
    ga = cs["a"].astype(np.float64); gc = cs["c"].astype(np.float64)
    ra = _ratio(ga, want_a, a_lo, a_hi)[valid]; rc = _ratio(gc, want_c, c_lo, c_hi)[valid]
    rg = rref.regime(cs["raw"], cs["want_a"], cs["want_n"], cs["hit"])
    print("%s: regime raw3 max %.2f, cut after tile 0 %.3f of hit rays, rays of count 0 / 32 / 64: %d / %d / %d, wanted alpha rounds to 1.0f %.4f, below 2^-24 "
          "%.4f" % (name, rg["raw_max"], rg["cut_share"], rg["n0"], rg["n32"], rg["n64"], rg["one_share"], rg["tiny_share"]))
    print("%s: (e) %d samples; |got - want| / half-width: alpha worst %.3f median %.3g, colour worst %.3f median %.3g; delta3 median %.3g worst %.3g" % (
        name, valid.sum(), ra.max(), np.median(ra), rc.max(), np.median(rc), np.median(cs["delta"][valid][:, 3]), cs["delta"][valid][:, 3].max()))
    assert rg["raw_max"] >= sr.REGIME_BARS["raw_max"] and rg["cut_share"] >= sr.REGIME_BARS["cut_share"], rg
    assert rg["n32"] >= 100 and rg["n64"] >= 100, rg
    assert ((ga >= a_lo) & (ga <= a_hi))[valid].all(), (float(ra.max()), int((ra > 1).sum()))
    assert ((gc >= c_lo) & (gc <= c_hi))[valid].all(), (float(rc.max()), int((rc > 1).sum()))


def _check_count_rule(name, cs, a=None, n=None):
    """(f): the device's count against the rule on its own emitted tile-0 alphas"""
    a = cs["a"] if a is None else a; n = cs["n"] if n is None else n; hit = cs["hit"]
    a0 = np.where(hit[:, None], a.astype(np.float64), 0.0)                    # (tile 0 is always emitted on a hit; the rule reads alpha[:32] only)
    want, amb, _ = rref.count_rule(a0, hit)
    print("%s: (f) ambiguous rays %d of %d hits (%.4f)" % (name, amb.sum(), hit.sum(), amb.sum() / max(1, hit.sum())))
    assert amb.sum() <= 0.01 * hit.sum()
    assert np.array_equal(n[~amb], want[~amb].astype(np.int64)), int((n != want)[~amb].sum())
    return amb


def test_t_misses_and_counts(case):
    name, cs = case
    _check_t_misses_counts(name, cs)
    assert (cs["n"] == 0).sum() >= 100


def test_alpha_and_colours_inside_the_reference_interval(case):
    _check_alpha_colours(*case)


def test_count_follows_the_devices_own_alphas(case):
    _check_count_rule(*case)


def test_tile_hand_over(case):
    """(i): at slot 32 the interval is t[32] - t[31], not t[32] - 0"""
    name, cs = case
    r64 = cs["n"] == 64; t = cs["t"].astype(np.float64)[r64]; raw = cs["raw"][r64, 32]; delta = cs["delta"][r64, 32]
    a_lo, a_hi, _, _ = rref.intervals(raw, delta, t[:, 32] - t[:, 31])
    got = cs["a"].astype(np.float64)[r64, 32]
    wrong, _ = rref.alpha_of(raw[:, 3], t[:, 32])                             # a tlast of 0
    tells = (wrong < a_lo) | (wrong > a_hi)
    print("%s: (i) %d rays of count 64, the interval from 0 would leave the bound on %d" % (name, r64.sum(), tells.sum()))
    assert tells.sum() >= 100
    assert ((got >= a_lo) & (got <= a_hi)).all()


def test_render_skipping(pkg, case):
    """(g)"""
    name, cs = case; o = cs["o"]; P = cs["P"]
    try:
        o.set_render_skip(True, 1e-3)
        t, a, c, n = _flat(pkg.scene_samples([o], cs["rect"], cs["pose"], 0, 0), P)
    finally:
        o.set_render_skip(False)
    assert np.array_equal(n == 0, cs["n"] == 0)
    v2 = np.arange(64)[None, :] < n[:, None]; both = v2 & cs["valid"]
    assert np.array_equal(_bits(t)[v2], _bits(cs["smp"]["t"])[v2])
    same = (_bits(a) == _bits(cs["a"])) & (_bits(c) == _bits(cs["c"])).all(-1)
    zero = (a == 0) & (c == 0).all(-1)
    assert (same | zero)[both].all(), int((~(same | zero))[both].sum())
    # samples only the skipping render emits (its tile 0 let more through): zero or inside the reference interval
    only = v2 & ~cs["valid"]
    if only.any():
        a_lo, a_hi, c_lo, c_hi = rref.intervals(cs["raw"], cs["delta"], rref.intervals_dt(t))
        ins = (a >= a_lo) & (a <= a_hi) & ((c >= c_lo) & (c <= c_hi)).all(-1)
        assert (ins | zero)[only].all()
    amb = _check_count_rule(name + " skip", cs, a, n)
    amb0 = rref.count_rule(np.where(cs["hit"][:, None], cs["a"].astype(np.float64), 0.0), cs["hit"])[1]
    moved = (n != cs["n"]) & ~amb & ~amb0
    want_on = rref.count_rule(np.where(cs["hit"][:, None], a.astype(np.float64), 0.0), cs["hit"])[0]
    want_off = rref.count_rule(np.where(cs["hit"][:, None], cs["a"].astype(np.float64), 0.0), cs["hit"])[0]
    assert (want_on[moved] != want_off[moved]).all()
    print("%s: (g) zeroed samples %d of %d, counts moved on %d rays" % (name, (zero & ~same)[both].sum(), both.sum(), (n != cs["n"]).sum()))


def test_side_1_equals_side_0(pkg, case):
    """(h)"""
    name, cs = case
    t, a, c, n = _flat(pkg.scene_samples([cs["o"]], cs["rect"], cs["pose"], 0, 1), cs["P"])
    v = cs["valid"]
    assert np.array_equal(n, cs["n"])
    assert np.array_equal(_bits(t)[v], _bits(cs["t"])[v]) and np.array_equal(_bits(a)[v], _bits(cs["a"])[v]) and np.array_equal(_bits(c)[v], _bits(cs["c"])[v])


def test_second_pass(two_pass):
    """1 500 rays of a 129 x 128 rect, the 128 of the second pass among them: (d), (e) and (f) with the jitter index past the pass boundary"""
    name, cs = two_pass
    late = cs["idx"] >= CHUNK
    assert late.sum() >= 100 and (late & cs["hit"]).sum() >= 50, (late.sum(), (late & cs["hit"]).sum())
    _check_t_misses_counts(name, cs)
    _check_alpha_colours(name, cs)
    _check_count_rule(name, cs)


@pytest.mark.parametrize("name", CROSS)
def test_cross_route_tie(pkg, orc, ss, scene, objects, name):
    """the pose route's positions and raw outputs (k_pose_grad on the same tile_forward) against the render's lists"""
    cs = _shape_case(name, pkg, orc, ss, scene, objects)
    o = cs["o"]; valid = cs["valid"]
    x, raw, _ = o.pose_samples(np.asarray(cs["rect"], np.uint32).reshape(1, 5), ss.colmajor(scene.objects[0]["Tow"]), pkg.pose_refine_default(rays_per_iter=0))
    # the same t: p = fmaf(t, d, o) of the restated t on the object's ray row, bit for bit
    assert np.array_equal(_bits(x)[valid], _bits(cs["smp"]["pos"])[valid]), int((_bits(x) != _bits(cs["smp"]["pos"]))[valid].sum())
    raw = raw.astype(np.float64); dt = rref.intervals_dt(cs["t"])
    assert np.array_equal(sr.h(raw), raw)                                       # fp16 numbers
    ga = cs["a"].astype(np.float64); gc = cs["c"].astype(np.float64)
    tight = rref.intervals(raw, np.zeros_like(raw), dt); loose = rref.intervals(raw, sr.ulp16(raw), dt)
    ok = [(ga >= q[0]) & (ga <= q[1]) & ((gc >= q[2]) & (gc <= q[3])).all(-1) for q in (tight, loose)]
    print("%s: cross-route: %d samples, inside the activation bound of the route's own raw %.6f, equal to the reference's raw %.5f" % (
        name, valid.sum(), ok[0][valid].mean(), (raw == cs["raw"]).all(-1)[valid].mean()))
    assert ok[1][valid].all(), int((~ok[1])[valid].sum())
