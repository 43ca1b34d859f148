"""Scan matching against a device-resident distance field on the GPU (include/mon_core.h; k_scan_match and k_scan_fold in
kernels_scan_match.hip): mon_dist_field_match against the numpy restatement of the rule (tests/scan_match_reference.py, pinned on its own in
tests/test_scan_match_abi.py) bit for bit in every case; mon_dist_field_register by its exact rules (its cost and counts are the match's at the returned pose,
batches equal single calls, the statuses, `best`, how far a returned rotation may be from orthonormal) and by recovery of a known pose on an analytic signed
distance field, with the bar taken from the reference's own Levenberg-Marquardt loop run here on the CPU."""
import numpy as np
import pytest

import dist_field_reference as dr
import scan_match_reference as sm

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("cost", "n_inside", "n_inlier", "A", "b")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    got = _bits(got).reshape(-1); want = _bits(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "%d of %d differ, the first at %d: %#x, want %#x" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def _field(shape, seed, step, origin):
    """a random finite field of shape (nx, ny, nz) with values in [-1, 2): (D (nz, ny, nx), origin, step)"""
    nx, ny, nz = shape; rng = np.random.default_rng(seed)
    return (rng.random((nz, ny, nx)) * 3.0 - 1.0).astype(F), np.array(origin, F), np.array(step, F)


FIELD = _field((13, 11, 7), 21, (0.3, -0.2, 0.45), (0.4, 1.3, -2.2))               # steps of mixed sign
FLAT = _field((9, 8, 1), 22, (0.25, 0.5, 7.0), (-1.0, 0.5, 0.3))                    # an axis of one cell


def _poses(field, H, seed):
    """pose 0 is the identity (so the points are world points and can sit on a face exactly); the others turn by up to 0.2 rad about the lattice's centre
    and shift by up to a cell; the last row is junk, which the rule ignores"""
    D, o, s = field; nz, ny, nx = D.shape; rng = np.random.default_rng(seed)
    centre = o.astype(np.float64) + 0.5 * (np.array([nx, ny, nz]) - 1) * s.astype(np.float64)
    T = np.zeros((H, 4, 4))
    for h in range(H):
        R = np.eye(3) if h == 0 else dr.rotation(rng.normal(size=3), rng.uniform(-0.2, 0.2))
        dt = np.zeros(3) if h == 0 else rng.uniform(-1, 1, 3) * np.abs(s)
        T[h, :3, :3] = R; T[h, :3, 3] = centre - R @ centre + dt; T[h, 3] = rng.normal(size=4)
    return T.astype(F).reshape(H, 16)


def _points(field, n, seed):
    """n points: most inside; then, on every other point, per axis a coordinate on a face (the last cell's upper face included), one ulp to either side of
    it, far outside, NaN and inf"""
    D, o, s = field; nz, ny, nx = D.shape; dims = np.array([nx, ny, nz], np.float64); rng = np.random.default_rng(seed)
    p = (o.astype(np.float64) + rng.random((n, 3)) * (dims - 1) * s.astype(np.float64)).astype(F)
    k = 0
    for a in range(3):
        for face in (dims[a] - 1, 0.0):
            on = F(np.float64(o[a]) + face * np.float64(s[a]))
            for v in (on, np.nextafter(on, F(np.inf)), np.nextafter(on, F(-np.inf)), F(on + F(1e6) * s[a]), F(np.nan), F(np.inf), F(-np.inf)):
                if k < n:
                    p[k, a] = v; k += 2
    return p


HUBERS = (0.05, 1.0, np.inf)                                                        # small (most points beyond it), large, none
OUTSIDE = 1.7


def _check_match(pkg, field, n, H, seed):
    D, o, s = field
    pts = _points(field, n, seed); poses = _poses(field, H, seed + 1)
    rng = np.random.default_rng(seed + 2)
    centre = o.astype(np.float64) + 0.5 * (np.array(D.shape[::-1]) - 1) * s.astype(np.float64)
    piv = (centre + rng.normal(size=(H, 3)) * 0.3).astype(F)
    with pkg.dist_field_create(D, o, s) as f:
        for c in (piv, None):
            for hub in HUBERS:
                want = sm.match(D, o, s, pts, poses, c, hub, OUTSIDE)
                got = f.match(pts, poses, c, huber=hub, outside=OUTSIDE)
                for k in KEYS:
                    _same(got[k], want[k], (n, H, c is None, hub, k))
                lite = f.match(pts, poses, c, huber=hub, outside=OUTSIDE, normal=False)
                assert set(lite) == {"cost", "n_inside", "n_inlier"}
                for k in lite:
                    _same(lite[k], got[k], (n, H, c is None, hub, k, "normal NULL"))
                bare = f.match(pts, poses, c, huber=hub, outside=OUTSIDE, normal=False, counts=False)
                _same(bare["cost"], got["cost"], (n, H, c is None, hub, "cost alone"))
        again = f.match(pts, poses, piv, huber=1.0, outside=OUTSIDE)
        last = f.match(pts, poses[H - 1:], piv[H - 1:], huber=1.0, outside=OUTSIDE)
        want = sm.match(D, o, s, pts, poses, piv, 1.0, OUTSIDE)
        for k in KEYS:
            _same(again[k], want[k], (n, H, k, "again")); _same(last[k], want[k][H - 1:], (n, H, k, "the last pose alone"))
    return want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_match_equals_the_reference(pkg, n):
    """the 13 x 11 x 7 field with steps of mixed sign: every n with H = 1, 3, 17, pivots given and NULL, huber small, large and +inf; the points include NaN
    and inf, points outside the lattice and points on the last cell's upper face; cost, counts, A and b in every bit; normal == NULL (and the counts NULL
    too) gives the same cost and counts; a second call and the last pose alone give the same bits"""
    for H in (1, 3, 17):
        want = _check_match(pkg, FIELD, n, H, 100 * n + H)
        if n >= 63:                                                                 # the case is not vacuous
            assert (want["n_inside"] > 0).all() and (want["n_inside"] < n).all() and (want["n_inlier"] < want["n_inside"]).all()
            assert (want["A"] != 0).any() and (want["b"] != 0).any()


@pytest.mark.parametrize("n,H", [(66001, 2), (3, 4096)])
def test_match_at_the_ends_of_its_range(pkg, n, H):
    """more than 64 chunks of 1 024 points, where the chunk rows are folded in two launches; and the largest batch of poses"""
    D, o, s = FIELD
    pts = _points(FIELD, n, 5); poses = _poses(FIELD, H, 6)
    want = sm.match(D, o, s, pts, poses, None, 1.0, OUTSIDE)
    with pkg.dist_field_create(D, o, s) as f:
        got = f.match(pts, poses, None, huber=1.0, outside=OUTSIDE)
        for k in KEYS:
            _same(got[k], want[k], (n, H, k))
        lite = f.match(pts, poses, None, huber=1.0, outside=OUTSIDE, normal=False)
        for k in lite:
            _same(lite[k], want[k], (n, H, k, "normal NULL"))


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_match_on_an_axis_of_one_cell(pkg, n):
    """a 9 x 8 x 1 lattice: z is neither interpolated nor range-checked, its gradient component is 0, and row and column 2 of A and b_2 are +0"""
    want = _check_match(pkg, FLAT, n, 3, 900 + n)
    zero = [m for m, (i, j) in enumerate(sm.PAIRS) if 2 in (i, j)]
    assert (_bits(want["A"][:, zero]) == 0).all() and (_bits(want["b"][:, 2]) == 0).all()
    if n > 1:
        assert (want["A"][:, [0, 6, 15]] > 0).all()                                 # A_00, A_11 and A_33 = sum w (a_z g_y)^2 are not


# ------------------------------------------------------------------------------------------------------------------------------------- register
_CASE = {}


def _case():
    if not _CASE:
        _CASE.update(sm.recovery_case())
    return _CASE


def _pivots(points, poses):
    """the pivot of every hypothesis as the library forms it: the centroid of the finite points summed in ascending index in double, the pose applied in
    double, rounded to float32 once"""
    acc = np.zeros(3); m = 0
    for q in np.asarray(points, F):
        if np.isfinite(q).all():
            acc = acc + q.astype(np.float64); m += 1
    cen = acc / m
    T = np.asarray(poses, F).reshape(-1, 4, 4).astype(np.float64)
    return np.stack([[((T[h, a, 0] * cen[0] + T[h, a, 1] * cen[1]) + T[h, a, 2] * cen[2]) + T[h, a, 3] for a in range(3)] for h in range(len(T))]).astype(F)


def _far(T):
    """the pose moved a thousand units away: the whole scan lies outside"""
    T = np.array(T, F).reshape(4, 4); T[:3, 3] += F(1e3); return T


def test_register_exact_rules(pkg):
    """cost and counts equal the match at the returned pose, bit for bit; cost is at most the match's at the input pose; a batch of five equals five single
    calls and two equal calls give equal bits; max_evals = 1 returns the inputs with status 1; a hypothesis whose scan lies outside returns status 3 and its
    input bits; best follows its rule; a returned rotation is orthonormal to (1 + evals) 2^-22"""
    c = _case(); D, o, s, pts = c["D"], c["origin"], c["step"], c["points"]
    starts = c["starts"]
    batch = np.stack([_far(starts[0]), starts[0], starts[1], starts[0], starts[2]])
    piv = _pivots(pts, batch)
    with pkg.dist_field_create(D, o, s) as f:
        prm = f.register_default()
        assert prm.huber == F(0.2) and prm.outside == D.max() and (prm.max_evals, prm.min_inside) == (30, 6) and prm.tol_trans == F(1e-3) * F(0.1)
        assert (prm.lambda0, prm.lambda_up, prm.lambda_down, prm.lambda_max, prm.tol_rot) == (F(1e-3), 10.0, 10.0, 1e6, F(1e-4))
        got = f.register(pts, batch)
        again = f.register(pts, batch)
        for k in got:
            _same(np.asarray(again[k]), np.asarray(got[k]), (k, "second call"))
        for h in range(5):
            one = f.register(pts, batch[h:h + 1])
            for k in ("poses", "cost", "n_inside", "n_inlier", "evals", "status"):
                _same(one[k], got[k][h:h + 1], (k, "hypothesis %d alone" % h))
            assert one["best"] == (-1 if h == 0 else 0)
        assert got["status"][0] == 3 and got["evals"][0] == 1 and got["n_inside"][0] == 0
        _same(got["poses"][0], batch[0], "status 3 returns its input")
        assert (got["status"][1:] != 3).all() and (got["evals"][1:] > 1).all() and (got["evals"] <= 30).all()
        _same(got["poses"][3], got["poses"][1], "equal hypotheses"); assert got["cost"][3] == got["cost"][1]
        ok = np.flatnonzero(got["status"] != 3)
        assert got["best"] == ok[np.argmin(got["cost"][ok])]                        # (argmin: the first of equal costs)
        at_out = f.match(pts, got["poses"], piv, huber=prm.huber, outside=prm.outside)
        at_in = f.match(pts, batch, piv, huber=prm.huber, outside=prm.outside)
        for k in ("cost", "n_inside", "n_inlier"):
            _same(got[k], at_out[k], (k, "the match at the returned pose"))
        assert (got["cost"] <= at_in["cost"]).all() and (got["cost"][1:] < at_in["cost"][1:]).all()
        _same(got["poses"][:, 3], batch[:, 3], "the last row is the input's")
        for h in range(1, 5):
            R = got["poses"][h, :3, :3].astype(np.float64)
            assert np.abs(R.T @ R - np.eye(3)).max() <= (1 + got["evals"][h]) * 2.0 ** -22, h
        first = f.register(pts, batch, max_evals=1)
        _same(first["poses"], batch, "max_evals = 1 returns the inputs")
        assert first["status"].tolist() == [3, 1, 1, 1, 1] and (first["evals"] == 1).all()
        for k in ("cost", "n_inside", "n_inlier"):
            _same(first[k], at_in[k], (k, "max_evals = 1: the match at the input pose"))
        lost = f.register(pts, np.stack([_far(starts[0]), _far(starts[1])]))
        assert lost["status"].tolist() == [3, 3] and lost["best"] == -1


def test_register_recovers_a_known_pose(pkg):
    """The analytic signed distance to two boxes and a sphere on 24 x 20 x 16 cells of 0.1; 512 points on its zero set in a body frame; eight starts, each
    0.15 rad and one cell from the known pose.  The bar is the committed numpy Levenberg-Marquardt of tests/scan_match_reference.py run here on the CPU with
    the same parameters: rotation error and centroid error each at most twice its worst over the eight starts (the factor covers the double-precision host
    steps, which the rule does not pin bit for bit).  The reference's figures, measured on the CPU: every start ends with status 0 after 18 to 28
    evaluations, at 6.2e-3 to 7.1e-3 rad and 0.028 to 0.031 cell -- the interpolated field's own offset from the analytic one; so the bars are 1.42e-2 rad
    and 0.062 cell."""
    c = _case(); D, o, s, pts = c["D"], c["origin"], c["step"], c["points"]
    ref = sm.register_default(D.shape, s, float(D.max()))
    worst = [0.0, 0.0]
    for T0 in c["starts"]:
        r = sm.register(D, o, s, pts, T0, ref)
        e = sm.pose_errors(r["pose"], c["pose"], c["centroid"])
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    with pkg.dist_field_create(D, o, s) as f:
        got = f.register(pts, c["starts"])
    assert (got["status"] != 3).all() and 0 <= got["best"] < 8
    for h in range(8):
        ang, cen = sm.pose_errors(got["poses"][h], c["pose"], c["centroid"])
        print("start %d: status %d after %d evaluations, %.3g rad, %.3g cell (reference's worst: %.3g rad, %.3g cell)"
              % (h, got["status"][h], got["evals"][h], ang, cen / 0.1, worst[0], worst[1] / 0.1))
        assert ang <= 2 * worst[0] and cen <= 2 * worst[1], (h, ang, cen, worst)
