"""Ray tracing against a device-resident distance field on the GPU (include/mon_core.h; k_field_trace and k_beam_terms in
kernels_field_trace.hip, folded by k_scan_fold): mon_dist_field_trace and mon_dist_field_beam_score against the numpy restatement of the rule
(tests/field_trace_reference.py, pinned on its own in tests/test_field_trace_abi.py) bit for bit in range, status, steps, normal, cost and counts, in every
case; the analytic scene against exact intersections; a traced scan registered back to its pose by mon_dist_field_register; a handle made by
mon_scene_dist_field; line of sight."""
import numpy as np
import pytest

import field_trace_reference as ft
import scan_match_reference as sm
from test_scene_render import scene, trained                                        # noqa: F401 -- the module-scoped fixtures of the scene render's tests
from test_components import SHAPE, _enclosing

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("range", "status", "steps", "normal")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = _bits(got).reshape(-1); want = _bits(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "%d of %d differ, the first at %d: %#x, want %#x" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def _field(shape, seed, step, origin):
    """tests/test_scan_match.py's random finite fields of shape (nx, ny, nz) with values in [-1, 2): (D (nz, ny, nx), origin, step)"""
    nx, ny, nz = shape; rng = np.random.default_rng(seed)
    return (rng.random((nz, ny, nx)) * 3.0 - 1.0).astype(F), np.array(origin, F), np.array(step, F)


FIELD = _field((13, 11, 7), 21, (0.3, -0.2, 0.45), (0.4, 1.3, -2.2))               # steps of mixed sign
FLAT = _field((9, 8, 1), 22, (0.25, 0.5, 7.0), (-1.0, 0.5, 0.3))                    # an axis of one cell
ONE = (np.full((1, 1, 1), 0.75, F), np.array((0.5, -1.0, 2.0), F), np.array((1.0, 1.0, 1.0), F))
ANALYTIC = ft.analytic_field()


def _tp(pkg, prm):
    return pkg.TraceParams(*[int(prm[k]) if k == "max_steps" else float(prm[k]) for k in ft.FIELDS])


def _rays(field, n, seed):
    """n rays: random origins (a part outside the lattice) and unit directions; then, on every other ray from the first: per face an origin exactly on it,
    one ulp to either side and far outside, pointing in, and the lattice's centre pointing out through it; a zero direction; NaN, inf and -inf in the origin
    and in the direction; from far outside pointing away"""
    D, o, s = field; nz, ny, nx = D.shape; dims = np.array([nx, ny, nz], np.float64)
    r = ft.random_rays(field, n, seed)
    centre = (o.astype(np.float64) + 0.5 * (dims - 1) * s.astype(np.float64)).astype(F)
    special = []
    for a in range(3):
        for face in (0.0, dims[a] - 1):
            on = F(np.float64(o[a]) + face * np.float64(s[a]))
            inward = np.zeros(3, F); inward[a] = np.sign(np.float64(centre[a]) - np.float64(on)) or 1.0
            for v in (on, np.nextafter(on, F(np.inf)), np.nextafter(on, F(-np.inf)), F(on - F(7.3) * np.abs(s[a]) * inward[a])):
                p = centre.copy(); p[a] = v; special.append(np.concatenate([p, inward]))
            special.append(np.concatenate([centre, -inward]))
            p = centre.copy(); p[a] = F(on - F(7.3) * np.abs(s[a]) * inward[a]); special.append(np.concatenate([p, -inward]))
    special.append(np.concatenate([centre, np.zeros(3, F)]))
    for bad in (np.nan, np.inf, -np.inf):
        p = centre.copy(); p[1] = bad; special.append(np.concatenate([p, (1, 0, 0)]))
        u = np.array((0.6, 0.0, 0.8), F); u[2] = bad; special.append(np.concatenate([centre, u]))
    for k, ray in enumerate(special):
        if 2 * k < n:
            r[2 * k] = ray
    return r


def _check_trace(pkg, field, n, H, seed, prm=None, calls=True):
    """H poses (0: world rays, poses16 NULL): every output against the reference; then each optional output NULL and alone, a second call and the last pose
    alone"""
    D, o, s = field
    rays = _rays(field, n, seed); poses = ft.field_poses(field, H, seed + 1) if H else None
    prm = prm or ft.trace_default(D.shape, s)
    want = ft.trace(D, o, s, rays, poses, prm, normals=True)
    with pkg.dist_field_create(D, o, s) as f:
        got = f.trace(rays, poses, _tp(pkg, prm), normals=True)
        for k in KEYS:
            _same(got[k], want[k], (n, H, k))
        if calls:
            bare = f.trace(rays, poses, _tp(pkg, prm), status=False, steps=False)
            assert set(bare) == {"range"}; _same(bare["range"], want["range"], (n, H, "range alone"))
            for k, kw in (("status", dict(steps=False)), ("steps", dict(status=False)), ("normal", dict(status=False, steps=False, normals=True))):
                one = f.trace(rays, poses, _tp(pkg, prm), **kw)
                assert set(one) == {"range", k}; _same(one[k], want[k], (n, H, k, "alone")); _same(one["range"], want["range"], (n, H, k, "alone: range"))
            again = f.trace(rays, poses, _tp(pkg, prm), normals=True)
            for k in KEYS:
                _same(again[k], want[k], (n, H, k, "again"))
            if H > 1:
                last = f.trace(rays, poses[H - 1:], _tp(pkg, prm), normals=True)
                for k in KEYS:
                    _same(last[k], want[k][H - 1:], (n, H, k, "the last pose alone"))
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_trace_equals_the_reference(pkg, n):
    """the 13 x 11 x 7 field with steps of mixed sign and default parameters: every n with poses16 NULL and H = 1, 3, 17; the rays include origins on every
    face and one ulp to either side, rays from outside pointing in and away, rays leaving through each face, a zero direction, NaN and inf in origin and
    direction; range, status, steps and normal in every bit; each optional output NULL and alone; a second call; the last pose alone"""
    for H in (0, 1, 3, 17):
        want = _check_trace(pkg, FIELD, n, H, 100 * n + H)
        if n >= 255:                                                                # the case is not vacuous: every way to end but the step budget
            assert all((want["status"] == k).any() for k in (ft.HIT, ft.PASSED, ft.LEFT)) and want["normal"].any() and want["steps"].max() > 20


@pytest.mark.parametrize("n,H", [(16, 4096), (4099, 64)])
def test_trace_at_the_ends_of_its_range(pkg, n, H):
    """the largest batch of poses; and more than sixteen blocks of rays under many poses"""
    _check_trace(pkg, FIELD, n, H, 7, calls=False)


@pytest.mark.parametrize("case", ["max_steps 1", "max_steps 2", "max_steps 7", "max_steps 256", "t_min == t_max", "eps above the field", "eps below the field",
                                  "relax 1"])
def test_trace_parameters(pkg, case):
    """the step budget at 1, 2, 7 and 256 with steps short enough to use it up; t_min == t_max (one sample); an eps above the field's maximum (the first
    inside sample hits, range = its t) and one below its minimum (never a hit); relax at its upper end"""
    D, o, s = FIELD; prm = ft.trace_default(D.shape, s)
    if case.startswith("max_steps"):
        prm.update(max_steps=int(case.split()[1]), step_min=F(0.004), relax=F(0.01), step_outside=F(0.01))
    elif case == "t_min == t_max":
        prm.update(t_min=F(0.7), t_max=F(0.7))
    elif case == "eps above the field":
        prm.update(eps=F(2.5))
    elif case == "eps below the field":
        prm.update(eps=F(-1.5))
    else:
        prm.update(relax=F(1.0))
    want = _check_trace(pkg, FIELD, 257, 3, 31, prm, calls=False)
    st = want["status"]
    if case.startswith("max_steps"):
        assert (st == ft.OUT_OF_STEPS).any() and (want["steps"][st == ft.OUT_OF_STEPS] == prm["max_steps"]).all()
    elif case == "t_min == t_max":
        assert (want["steps"] == 1).all() and set(np.unique(st)) <= {ft.HIT, ft.PASSED} and (st == ft.HIT).any()
    elif case == "eps above the field":
        assert not (st == ft.LEFT).any() and (st == ft.HIT).sum() > st.size // 4 and (want["steps"][st == ft.HIT] < 256).all()
    elif case == "eps below the field":
        assert not (st == ft.HIT).any() and not want["normal"].any()


@pytest.mark.parametrize("name", ["flat", "one cell", "analytic"])
def test_trace_on_other_fields(pkg, name):
    """a 9 x 8 x 1 lattice (z is neither interpolated nor range-checked and the normal's z is 0), a single cell (never outside; t_max = 0 by default, and a
    longer march) and the analytic field"""
    field = {"flat": FLAT, "one cell": ONE, "analytic": ANALYTIC}[name]
    for n, H in ((65, 0), (257, 3)):
        want = _check_trace(pkg, field, n, H, 50 + n, calls=False)
        if name == "flat":
            assert (_bits(want["normal"][..., 2]) == 0).all() and want["normal"].any()
        if name == "one cell":
            assert (want["status"] == ft.PASSED).all() and (want["steps"] == 1).all()
            prm = dict(ft.trace_default((1, 1, 1), ONE[2]), t_max=F(3))
            long = _check_trace(pkg, field, n, H, 60 + n, prm, calls=False)
            assert (long["steps"] > 1).all() and not (long["status"] == ft.LEFT).any()
            _check_trace(pkg, field, n, H, 70 + n, dict(prm, eps=F(0.75)), calls=False)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_analytic_scene_against_exact_intersections(pkg, k):
    """tests/test_field_trace_abi.py's case (c) on the device: the reference's bits, every judged ray a hit, no clear ray a hit, and the range within that
    test's bar of the exact intersection: 0.734 cell, twice the reference's own worst"""
    c = ft.analytic_case(ft.SENSORS[k])
    want = ft.trace(c["D"], c["origin"], c["step"], c["rays"], normals=True)
    with pkg.dist_field_create(c["D"], c["origin"], c["step"]) as f:
        got = f.trace(c["rays"], normals=True)
    for key in KEYS:
        _same(got[key], want[key], (k, key))
    hit = got["status"][0] == ft.HIT; j = c["judged"]
    assert not (j & ~hit).any() and not (c["clear"] & hit).any()
    err = np.abs(got["range"][0].astype(np.float64) - c["t"])[j] / 0.1
    print("sensor %d: worst range error %.3f cell over %d judged rays; lane utilisation %.2f" % (k, err.max(), j.sum(), ft.utilisation(got["steps"])))
    assert err.max() <= ft.ANALYTIC_BAR_CELLS


def test_trace_after_other_calls_on_the_handle(pkg):
    """score, match and beam_score use the same scratch: a trace after them, and they after a trace, give the bits of a fresh handle"""
    D, o, s = FIELD
    rays = _rays(FIELD, 300, 11); poses = ft.field_poses(FIELD, 5, 12)
    want = ft.trace(D, o, s, rays, poses, normals=True)
    rng = np.random.default_rng(13)
    pts = ft.random_rays(FIELD, 2000, 14)[:, :3]
    ways = ft.random_rays(FIELD, 40, 15)[:, :3].reshape(4, 10, 3); sph = np.array([[0, 0, 0, 0.1], [0.1, 0, 0, 0.05]], F)
    z = rng.uniform(0.1, 2.0, 300).astype(F)
    with pkg.dist_field_create(D, o, s) as f, pkg.dist_field_create(D, o, s) as fresh:
        sc0 = fresh.score(sph, ways, n_sub=4, outside=0.5, margin=0.02, safe=0.1); m0 = fresh.match(pts, poses, None, huber=1.0, outside=1.7)
        b0 = f.beam_score(rays, z, poses, huber=0.3)
        sc = f.score(sph, ways, n_sub=4, outside=0.5, margin=0.02, safe=0.1)
        m = f.match(pts, poses, None, huber=1.0, outside=1.7)
        got = f.trace(rays, poses, normals=True)
        for k in KEYS:
            _same(got[k], want[k], (k, "after score, match and beam_score"))
        for k in sc0:
            _same(f.score(sph, ways, n_sub=4, outside=0.5, margin=0.02, safe=0.1)[k], sc0[k], (k, "score after trace")); _same(sc[k], sc0[k], (k, "score"))
        for k in m0:
            _same(f.match(pts, poses, None, huber=1.0, outside=1.7)[k], m0[k], (k, "match after trace")); _same(m[k], m0[k], (k, "match"))
        b1 = f.beam_score(rays, z, poses, huber=0.3)
        for k in b0:
            _same(b1[k], b0[k], (k, "beam_score after the others"))


# ---------------------------------------------------------------------------------------------------------------------------------- the beam score
def _measured(want_range, seed):
    """measured ranges: pose 0's own ranges moved by up to 0.3, every fifth beam (and beam 1) without a return"""
    rng = np.random.default_rng(seed); n = want_range.shape[1]
    z = (want_range[0] + rng.uniform(-0.3, 0.3, n)).astype(F)
    z[4::5] = np.nan
    if n > 1:
        z[1] = np.nan
    return z


def _check_beam(pkg, n, H, seed):
    D, o, s = FIELD
    rays = _rays(FIELD, n, seed); poses = ft.field_poses(FIELD, H, seed + 1)
    tr = ft.trace(D, o, s, rays, poses)
    z = _measured(tr["range"], seed + 2)
    with pkg.dist_field_create(D, o, s) as f:
        own = f.trace(rays, poses)
        for hub in (0.2, np.inf):
            want = ft.beam_score_of(tr["range"], tr["status"], z, hub)
            got = f.beam_score(rays, z, poses, huber=hub)
            for k in want:
                _same(got[k], want[k], (n, H, hub, k))
            mine = ft.beam_score_of(own["range"], own["status"], z, hub)            # the tree over trace's own returned ranges
            for k in mine:
                _same(got[k], mine[k], (n, H, hub, k, "over the call's own ranges"))
        full = np.where(np.isnan(z), F(1), z)
        _same(f.beam_score(rays, full, poses, huber=0.2)["n_valid"], np.full(H, n, np.int32), (n, H, "no NaN"))
        world = f.beam_score(rays, z, None, huber=0.2); w0 = ft.beam_score(D, o, s, rays, z, None, huber=0.2)
        for k in w0:
            _same(world[k], w0[k], (n, k, "poses16 NULL"))
    return want


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_beam_score_equals_the_reference(pkg, n):
    """cost, n_valid and n_hit in every bit at H = 1 and 17, with and without a Huber threshold, NaN beams included; the cost is the reference's tree over
    the ranges mon_dist_field_trace itself returns for the same call; poses16 NULL.  The sizes are test_match_equals_the_reference's boundaries of the
    block row the two kernels share (fd_block_row): a ragged quad at the start, a full wave, one lane into the next wave, one short of a chunk, a chunk,
    one past it.  (The reference alone, on the CPU, meets the condition below at 256, 257 and 1 023 too: 44 to 241 hits of 204 to 818 valid beams.)"""
    for H in (1, 17):
        want = _check_beam(pkg, n, H, 300 + 10 * n + H)
        if n >= 255:
            assert (want["cost"] > 0).all() and (0 < want["n_hit"]).all() and (want["n_hit"] < want["n_valid"]).all() and (want["n_valid"] < n).all()


def test_beam_score_with_two_fold_launches(pkg):
    """more than 64 chunks of 1 024 beams, where the chunk rows are folded in two launches"""
    D, o, s = FIELD; n, H = 66001, 2
    rays = ft.random_rays(FIELD, n, 41, spread=0.45); poses = ft.field_poses(FIELD, H, 42)
    tr = ft.trace(D, o, s, rays, poses); z = _measured(tr["range"], 43)
    want = ft.beam_score_of(tr["range"], tr["status"], z, 0.2)
    with pkg.dist_field_create(D, o, s) as f:
        got = f.beam_score(rays, z, poses, huber=0.2)
    for k in want:
        _same(got[k], want[k], (n, H, k))


# ---------------------------------------------------------------------------------------------------------------------------------- round trip
def test_traced_scan_registers_back_to_its_pose(pkg):
    """On the analytic field a 128 x 16 scan is traced from a known sensor pose; its hits become sensor-frame points o + range u, and
    mon_dist_field_register starts from eight poses 0.15 rad (about the scan's centroid) and one cell away.  The bar is twice the worst error of the same
    chain run here on the CPU by the two committed references (the trace's rule, then tests/scan_match_reference.py's Levenberg-Marquardt), as in
    tests/test_scan_match.py.  The reference chain's figures, measured on the CPU: every start ends with status 0 after 6 to 19 evaluations at 1.04e-2 rad
    and 0.166 cell (the level eps = c / 8 sits before the surface, so the scan is that much short and the recovered pose is off by a share of it); so the
    bars are 2.08e-2 rad and 0.332 cell."""
    D, o, s = ANALYTIC; G = ft.sensor_pose(); rays = ft.sensor_rays()
    want = ft.trace(D, o, s, rays, G.reshape(1, 16))
    with pkg.dist_field_create(D, o, s) as f:
        got = f.trace(rays, G.reshape(1, 16))
        for k in ("range", "status", "steps"):
            _same(got[k], want[k], k)
        hit = got["status"][0] == ft.HIT
        assert hit.sum() > 500
        pts = (rays[hit, :3] + got["range"][0, hit, None] * rays[hit, 3:]).astype(F)
        cen = pts.astype(np.float64).mean(0); G64 = G.astype(np.float64); cw = G64[:3, :3] @ cen + G64[:3, 3]
        rng = np.random.default_rng(17); starts = np.zeros((8, 4, 4), F)
        for m in range(8):
            ax = rng.normal(size=3); v = rng.normal(size=3); v *= 0.1 / np.linalg.norm(v)
            starts[m] = sm.twist_pose(G64, cw, np.concatenate([v, 0.15 * ax / np.linalg.norm(ax)])).astype(F)
        ref = sm.register_default(D.shape, s, float(D.max())); worst = [0.0, 0.0]
        for T0 in starts:
            r = sm.register(D, o, s, pts, T0, ref)
            e = sm.pose_errors(r["pose"], G, cen)
            worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        reg = f.register(pts, starts)
    assert (reg["status"] != 3).all() and 0 <= reg["best"] < 8
    for h in range(8):
        ang, c = sm.pose_errors(reg["poses"][h], G, cen)
        print("start %d: status %d after %d evaluations, %.3g rad, %.3g cell (the reference chain's worst: %.3g rad, %.3g cell)"
              % (h, reg["status"][h], reg["evals"][h], ang, c / 0.1, worst[0], worst[1] / 0.1))
        assert ang <= 2 * worst[0] and c <= 2 * worst[1], (h, ang, c, worst)


# ---------------------------------------------------------------------------------------------------------------------------------- scene handles
def test_trace_on_a_scene_handle(pkg, scene, trained):
    """a handle made by mon_scene_dist_field over three small objects at 24 x 20 x 18: trace and beam_score equal those on mon_dist_field_create(read()),
    and the existing lattice routes give the bits from before"""
    _, objs = trained; lst = [objs["b0"], objs["a1"], objs["a2"]]; origin, step = _enclosing(scene, SHAPE)
    sigma = pkg.query_scene_lattice(lst, origin, step, SHAPE, 0)[0]
    smin = float(np.percentile(sigma, 90.0, method="lower"))

    def routes():
        comp = pkg.scene_components_lattice(lst, origin, step, SHAPE, smin, 1, 0.02, 18, side=0, rows=("dist",))
        path = pkg.scene_paths_lattice(lst, origin, step, SHAPE, smin, [0], side=0)
        return (list(pkg.query_scene_lattice(lst, origin, step, SHAPE, 0)) + list(pkg.scene_distance_lattice(lst, origin, step, SHAPE, smin, 0.3, side=0)) +
                [comp[0], comp[1], comp[4]["dist"]] + [path[0], path[1]])

    before = routes()
    with pkg.scene_dist_field(lst, origin, step, SHAPE, smin, 0.3, side=0) as f:
        cells = f.read(); field = (cells, np.asarray(origin, F), np.asarray(step, F))
        assert 0 < (cells == 0).sum() < cells.size
        rays = _rays(field, 700, 23); poses = ft.field_poses(field, 3, 24)
        z = np.random.default_rng(25).uniform(0.0, 0.5, 700).astype(F)
        with pkg.dist_field_create(cells, origin, step) as h:
            d0, d1 = f.trace_default(), h.trace_default()
            assert bytes(d0) == bytes(d1) and _tp(pkg, ft.trace_default(cells.shape, field[2])).eps == d0.eps
            a = f.trace(rays, poses, normals=True); b = h.trace(rays, poses, normals=True)
            for k in KEYS:
                _same(a[k], b[k], (k, "scene handle against created handle"))
            assert (a["status"] == ft.HIT).any() and (a["status"] == ft.LEFT).any()
            sa = f.beam_score(rays, z, poses, huber=0.1); sb = h.beam_score(rays, z, poses, huber=0.1)
            for k in sa:
                _same(sa[k], sb[k], (k, "beam score, scene handle against created handle"))
        want = ft.trace(cells, field[1], field[2], rays, poses, normals=True)
        for k in KEYS:
            _same(a[k], want[k], (k, "scene handle against the reference"))
    for i, (x, y) in enumerate(zip(before, routes())):
        _same(y, x, ("route output", i))


def test_default_parameters_and_line_of_sight(pkg):
    """mon_trace_default equals the reference's on every field; line_of_sight on the analytic scene: free between two points on one side of a box, blocked
    through it, and equal to a trace along the segment"""
    for field in (FIELD, FLAT, ONE, ANALYTIC):
        D, o, s = field
        with pkg.dist_field_create(D, o, s) as f:
            assert bytes(f.trace_default()) == bytes(_tp(pkg, ft.trace_default(D.shape, s))), D.shape
    D, o, s = ANALYTIC
    a = np.array([[0.2, 0.3, 0.8], [0.2, 0.3, 0.8], [0.2, 0.3, 0.8]]); b = np.array([[2.0, 0.2, 1.3], [1.2, 1.7, 0.8], [0.7, 1.0, 0.8]])
    with pkg.dist_field_create(D, o, s) as f:
        free = f.line_of_sight(a, b)
        assert free.tolist() == [True, False, False] and f.line_of_sight(a[0], b[0]) is True
        for m in range(3):
            v = b[m] - a[m]; length = np.linalg.norm(v)
            prm = dict(ft.trace_default(D.shape, s), t_max=F(length))
            want = ft.trace(D, o, s, np.concatenate([a[m], v / length]).astype(F), None, prm)
            assert bool(want["status"][0, 0] == ft.PASSED) == bool(free[m]), m
