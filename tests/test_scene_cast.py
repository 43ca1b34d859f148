"""GPU tests (-m gpu) of the ray cast against the object map (mon_scene_cast, mon_online_cast_rays; kernels k_scene_cast_rays and
k_scene_cast_composite in kernels_scene_cast.hip, the keyed instantiation of k_fused_render<EMIT> unchanged).  The yardstick of everything the cast
shares with the probe is the probe itself, bit for bit: the cast of mon_camera_rays' rays at hit_opacity 0.5 equals mon_scene_probe of the queries.
What is new has references of its own: the ray rows of arbitrary world rays against an fp64 restatement within a counted bound, the axis-aligned
cases against the IEEE outcome of ray_intersect stated case by case, the first crossing at a threshold against an fp64 merge, and the interpolated
hit against the fp64 closed form within a counted first-order bound.  The scene, the trained objects and the overlap view are those of
tests/test_scene_render.py; the rect, the queries and the helpers those of tests/test_scene_probe.py."""
import os
import threading

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import ROOT
import test_scene_probe as tsp
import test_scene_render as tsr
from test_scene_probe import setup                                # noqa: F401 -- the probe tests' module fixture: the 40 x 24 rect and its three objects
from test_scene_render import scene, trained, overlap_view       # noqa: F401 -- the module-scoped fixtures of the scene render's tests

pytestmark = pytest.mark.gpu

CHUNK = tsp.CHUNK            # kRenderChunkRays: the rays of one pass
TIE = tsp.TIE                # a ray is left out of the hit comparison when a reference T_{i+1} lies within this (relative) of 1 - threshold
U = tsp.U                    # unit roundoff of fp32
LOG_ULP = 3                  # logf: at most 3 ulp (the OpenCL full-profile bound the device library documents), 1 ulp <= 2 U relative
_bits, _same_bits = tsp._bits, tsp._same_bits


def _K(sc):
    return (sc.fx, sc.fy, sc.cx, sc.cy)


def _as_probe(cast, dn):
    """The six probe outputs from a cast's seven, as the bit rule states them: dist / dn and hit_sample_t / dn in fp32 on the host."""
    rgb, dist, op, inst, ht, hs, hi = cast
    return rgb, (dist / dn).astype(np.float32), op, inst, (hs / dn).astype(np.float32), hi


def _subpixel_queries(pkg, sc, rng, n, key0):
    u = rng.uniform(-60.0, sc.W + 60.0, n).astype(np.float32); v = rng.uniform(-45.0, sc.H + 45.0, n).astype(np.float32)
    return pkg.scene_queries(rng.randint(0, 3, n), key0 + np.arange(n), u, v)


def _behind(pkg, objs, q, poses, side=0):
    """Per object and query: the probe's ray row says hit although the box lies wholly behind the camera (the line meets it at negative t only: t1 <= the
    clamped t0).  mon_scene_probe and mon_scene_render sample such an object at negative t; for mon_scene_cast it is a miss (lo < hi fails)."""
    rows = np.stack([pkg.scene_probe_rays(objs, q, poses, k, side) for k in range(len(objs))])
    return (rows[..., 8] > 0) & (rows[..., 7] <= rows[..., 6])


def _three_poses(ss, s):
    return np.stack([s["pose"]] + [tsr._pose(ss, s["sc"], w) for w in (2, 13)])


# ---------------------------------------------------------------------------------------------------------------- 4: the bit rule
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("skip", [False, True])
def test_bit_rule(pkg, ss, setup, skip, K, side):       # noqa: F811
    """Test 4: rays = mon_camera_rays(the dataset's K, poses, q), the queries' keys, t_max = +inf, hit_opacity 0.5: rgb, opacity, instance and
    hit_instance are mon_scene_probe(q)'s bits, dist / dn and hit_sample_t / dn its depth and hit_depth.  q = every pixel of the rect under its pose
    and 300 sub-pixel points inside and outside the image under three poses; K = 1 (the rect's most visible object) and 3, render skipping off and on
    (min_alpha 1e-3), both sides.  The rect holds at least 50 opaque and 30 background rays.
    The rule has one exception, which the header states: an object whose box lies wholly behind a ray's origin (the probe's row is a hit with t1 < 0:
    from view 2 some of the sub-pixel rays meet object 0's inflated box that way).  The probe samples it at negative t; the cast takes it for a miss.
    On those rays the cast equals the probe over the other objects of the list, or the background when none is left."""
    s = setup; sc = s["sc"]
    best = int(np.bincount(s["base"][3][s["base"][3] >= 0], minlength=3).argmax())
    objs = s["objs3"] if K == 3 else [s["objs3"][best]]
    poses = _three_poses(ss, s); P = s["q"].shape[0]
    q = np.concatenate([s["q"], _subpixel_queries(pkg, sc, np.random.RandomState(21), 300, P)])
    outside = (q["u"] < 0) | (q["u"] > sc.W - 1) | (q["v"] < 0) | (q["v"] > sc.H - 1)
    assert outside[P:].sum() > 30 and (~outside[P:]).sum() > 30
    rays, dn = pkg.camera_rays(_K(sc), poses, q)
    for o in objs:
        o.set_render_skip(skip, 1e-3)
    try:
        want = pkg.probe_scene(objs, q, poses, side)
        got = pkg.cast_scene(objs, rays, 0.5, side)
    finally:
        for o in objs:
            o.set_render_skip(False)
    n_op, n_bg = int((want[2][:P] > 0.5).sum()), int((want[2][:P] < 0.5).sum())
    print("bit rule skip %d K %d side %d: %d opaque and %d background rays in the rect, %d hits among the sub-pixel points"
          % (skip, K, side, n_op, n_bg, int((want[5][P:] >= 0).sum())))
    behind = _behind(pkg, objs, q, poses, side); clean = ~behind.any(0); mine = _as_probe(got, dn)
    assert not behind[:, :P].any()                                                      # (every pixel of the rect is a clean ray)
    _same_bits([x[clean] for x in mine], [x[clean] for x in want], (skip, K, side))
    for pat in {tuple(b) for b in behind[:, ~clean].T}:
        sel = (behind.T == np.array(pat)).all(1); keep = np.array([k for k in range(len(objs)) if not pat[k]], np.int32)
        if keep.size:
            ref = list(pkg.probe_scene([objs[k] for k in keep], q[sel], poses, side))
            for col in (3, 5):
                ref[col] = np.where(ref[col] >= 0, keep[np.maximum(ref[col], 0)], -1).astype(np.int32)
        else:
            m = int(sel.sum()); z = np.zeros(m, np.float32); none = np.full(m, -1, np.int32)
            ref = [np.ones((m, 3), np.float32), z, z, none, z, none]
        _same_bits([x[sel] for x in mine], ref, ("a box behind the origin", pat))
    print("  %d rays with a box behind their origin" % int((~clean).sum()))
    assert n_op >= 50 and n_bg >= 30
    # at 0.5 the interpolated hit lies in the sample's interval and exists exactly where the probe's hit does
    hit = got[6] >= 0
    assert (got[4][hit] >= 0).all() and (got[4][hit] <= got[5][hit]).all() and (got[4][~hit] == 0).all() and (got[5][~hit] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 5: ray rows
def test_camera_ray_rows_are_the_probes(pkg, ss, setup):       # noqa: F811
    """Test 5a: for camera rays the rows of mon_debug_scene_cast_rays are the bits of mon_debug_scene_probe_rays' rows (o, d, t0, t1, flag), except
    dn = 1; the entry row is t0 where the flag is set and 0 elsewhere.  Where the probe's row is a hit on a box wholly behind the camera (t1 <= the
    clamped t0) the cast's row is a miss."""
    s = setup; sc = s["sc"]; objs = s["objs3"]; poses = _three_poses(ss, s)
    q = np.concatenate([s["q"], _subpixel_queries(pkg, sc, np.random.RandomState(22), 600, s["q"].shape[0])])
    rays, dn = pkg.camera_rays(_K(sc), poses, q)
    n_hit = 0
    for k in range(3):
        want = pkg.scene_probe_rays(objs, q, poses, k)
        rows, entry = pkg.scene_cast_rays(objs, rays, k)
        back = (want[:, 8] > 0) & (want[:, 7] <= want[:, 6])
        assert (rows[back, :9] == 0).all()
        assert np.array_equal(_bits(rows[~back, :9]), _bits(want[~back, :9])), (k, int(back.sum()))
        assert np.array_equal(_bits(want[:, 9]), _bits(dn)) and (rows[:, 9] == 1.0).all()
        assert np.array_equal(_bits(entry), _bits(np.where(rows[:, 8] > 0, rows[:, 6], np.float32(0))))
        n_hit += int((rows[:, 8] > 0).sum())
    assert n_hit > 500


def ref_world_rays(Tow, mn, mx, o_w, d_w, t_max):
    """fp64 restatement of k_scene_cast_rays on the fp32 inputs, with the forward error bounds of its fp32 evaluation, counted the way
    tests/test_scene_probe.py's ref_rays counts them (each rounding at most U = 2^-24 relative to its result, first order):
      d  = Row d_w           one rot3 of (mul, fma, fma)      ->  3 U Md, Md = |Row| |d_w| (the magnitude of the terms summed)
      o  = Row o_w + tow     one rot3 and one add             ->  4 U Mo, Mo = |Row| |o_w| + |tow|
      a slab distance        t = (b - o) / d: the subtraction's rounding, o's and d's errors, the division's rounding
                             -> (Eo + U (|b| + |o|)) / |d| + |t| (Ed / |d| + U)
      t0 = the largest near distance, t1 = the smallest far one, lo = max(t0, 0), hi = min(t1, t_max): max and min do not amplify and t_max is
      exact -> the largest of the six slab bounds.
    Returns o, d, lo, hi, on (the box is hit and lo < hi), the bounds Eo, Ed, Et (Et = inf where a component of d is within its bound of 0) and t1."""
    Tow = np.asarray(Tow, np.float32).astype(np.float64).reshape(4, 4).T
    mn = np.asarray(mn, np.float32).astype(np.float64); mx = np.asarray(mx, np.float32).astype(np.float64)
    o_w = np.asarray(o_w, np.float32).astype(np.float64); d_w = np.asarray(d_w, np.float32).astype(np.float64)
    t_max = np.asarray(t_max, np.float32).astype(np.float64)
    Row, tow = Tow[:3, :3], Tow[:3, 3]
    d = d_w @ Row.T; o = o_w @ Row.T + tow
    Ed = 3 * U * (np.abs(d_w) @ np.abs(Row).T); Eo = 4 * U * (np.abs(o_w) @ np.abs(Row).T + np.abs(tow))
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (mn - o) / d, (mx - o) / d
        near, far = np.minimum(ta, tb), np.maximum(ta, tb)
        t0, t1 = near.max(-1), far.min(-1)
        Et = np.zeros(len(o))
        for b, t in ((mn, ta), (mx, tb)):
            Et = np.maximum(Et, ((Eo + U * (np.abs(b) + np.abs(o))) / np.abs(d) + np.abs(t) * (Ed / np.abs(d) + U)).max(-1))
    Et = np.where((np.abs(d) <= 2 * Ed).any(-1) | ~np.isfinite(Et), np.inf, Et)
    lo, hi = np.maximum(t0, 0.0), np.minimum(t1, t_max)
    return o, d, lo, hi, (t0 <= t1) & (lo < hi), Eo, Ed, Et, t1


def _unit(v):
    """fp32 directions normalised in fp64 and rounded: |d|^2 within a few U of 1."""
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def test_world_ray_rows_against_fp64(pkg, ss, setup, trained):       # noqa: F811
    """Test 5b: 6 000 world rays -- origins drawn around the scene, a quarter of the directions drawn on the sphere and the rest aimed at a point near
    an object, t_max infinite for a third, else drawn so that segments end in front of, inside and behind the boxes -- for each of the three true
    boxes, object 0's inflated one and a box under a rotated Tow (the scene's own objects have identity rotations, which make d exact): o, d, lo, hi
    within ref_world_rays' bounds; the flag agrees except where hi - lo lies within the slab-tie bound
    2 Et of 0; entry = lo; dn = 1; a row without the flag is zero."""
    s = setup; sc = s["sc"]
    rng = np.random.RandomState(6); N = 6000
    centres = np.stack([np.linalg.inv(np.asarray(ob["Tow"], np.float64))[:3, 3] for ob in sc.objects[:3]])
    w = np.array([0.3, -0.5, 0.4]); th = np.linalg.norm(w); Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    Trot = np.eye(4); Trot[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx; Trot[:3, 3] = -Trot[:3, :3] @ centres[1]
    Trot = Trot.astype(np.float32); half_rot = np.array([0.3, 0.2, 0.25], np.float32)       # a box about object 1's centre, turned by 0.7 rad
    rot = pkg.ObjectNeRF(trained[0], pkg.default_config(**tsr.BASE), sc.objects[1]["cls"], ss.colmajor(Trot), -half_rot, half_rot)
    lst = [s["objs"]["a0"], s["objs"]["a1"], s["objs"]["a2"], s["objs"]["b0"], rot]
    boxes = [(sc.objects[i]["Tow"], (sc.objects[i]["half"] * f).astype(np.float32)) for i, f in ((0, 1.0), (1, 1.0), (2, 1.0), (0, 5.0))] + [(Trot, half_rot)]
    o_w = (centres.mean(0) + rng.uniform(-3.0, 3.0, (N, 3))).astype(np.float32)
    aim = centres[rng.randint(0, 3, N)] + rng.normal(0.0, 0.1, (N, 3))
    d_w = _unit(np.where((np.arange(N) % 4 == 0)[:, None], rng.normal(size=(N, 3)), aim - o_w))
    reach = np.linalg.norm(aim - o_w, axis=-1)
    t_max = np.where(np.arange(N) % 3 == 0, np.inf,
                     reach * np.where(np.arange(N) % 3 == 1, rng.uniform(0.3, 1.6, N), rng.uniform(0.95, 1.05, N))).astype(np.float32)
    rays = pkg.scene_rays(o_w, d_w, t_max, np.arange(N))
    for k, (Tow, half) in enumerate(boxes):
        try:
            rows, entry = pkg.scene_cast_rays(lst, rays, k)
        finally:
            if k == len(boxes) - 1:
                rot.close()
        flag = rows[:, 8] > 0
        o, d, lo, hi, on, Eo, Ed, Et, t1 = ref_world_rays(ss.colmajor(Tow), -half, half, o_w, d_w, t_max)
        r = rows.astype(np.float64)
        sure = np.abs(hi - lo) > 2 * Et
        n_tie = int((~sure).sum())
        assert np.array_equal(flag[sure], on[sure])
        g = flag & on & np.isfinite(Et)
        assert (np.abs(r[g, 0:3] - o[g]) <= Eo[g]).all() and (np.abs(r[g, 3:6] - d[g]) <= Ed[g]).all()
        assert (np.abs(r[g, 6] - lo[g]) <= Et[g]).all() and (np.abs(r[g, 7] - hi[g]) <= Et[g]).all()
        cut = g & np.isfinite(t_max) & (t1 - t_max > 2 * Et) & (t_max - lo > 2 * Et)       # the segment ends well inside the box: hi is t_max itself
        assert np.array_equal(_bits(rows[cut, 7]), _bits(t_max[cut]))
        assert (rows[:, 9] == 1.0).all() and (r[~flag][:, :8] == 0).all() and (rows[flag, 6] < rows[flag, 7]).all() and (rows[flag, 6] >= 0).all()
        assert np.array_equal(_bits(entry), _bits(np.where(flag, rows[:, 6], np.float32(0))))
        assert k < 4 or float(np.abs(r[g, 3:6] - d[g]).max()) > 0                          # (the rotated box: d is rounded, and inside its bound)
        worst = dict(o=float((np.abs(r[g, 0:3] - o[g]) / Eo[g]).max()), d=float((np.abs(r[g, 3:6] - d[g]) / Ed[g]).max()),
                     lo=float((np.abs(r[g, 6] - lo[g]) / Et[g]).max()), hi=float((np.abs(r[g, 7] - hi[g]) / Et[g]).max()))
        print("object %d: %d rows flagged of %d (%d cut by t_max inside the box), %d within the tie bound, largest error / bound %s"
              % (k, int(flag.sum()), N, int(cut.sum()), n_tie, worst))
        assert flag.sum() > 100 and cut.sum() > 20 and n_tie < 0.02 * N


def _slab32(mn, mx, o, d):
    """ray_intersect (device_common.h) statement by statement in IEEE fp32 (numpy scalars): returns hit, t0, t1."""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        tmin, tmax = (f(mn[0]) - o[0]) / d[0], (f(mx[0]) - o[0]) / d[0]
        if tmin > tmax:
            tmin, tmax = tmax, tmin
        for a in (1, 2):
            ta, tb = (f(mn[a]) - o[a]) / d[a], (f(mx[a]) - o[a]) / d[a]
            if ta > tb:
                ta, tb = tb, ta
            if tmin > tb or ta > tmax:
                return False, f(0), f(0)
            if ta > tmin:
                tmin = ta
            if tb < tmax:
                tmax = tb
    return True, tmin, tmax


def _rot3_32(M, v):
    """rot3 (device_common.h) on a column-major 4 x 4 in fp32 with separate multiplies and adds: the fused operations' bits, signed zeros included,
    whenever the rotation is the identity (a product with 0 or 1 is exact, so each fma rounds what the separate operations round)."""
    f = np.float32
    return np.array([f(f(M[8 + r] * v[2]) + f(f(M[4 + r] * v[1]) + f(M[r] * v[0]))) for r in range(3)], f)


def test_axis_aligned_rays(pkg, ss, scene, trained):       # noqa: F811
    """Test 5c: an object whose Tow rotation is the identity (translation (0.25, -0.5, 0.125), box [-0.5, 0.5] x [-0.25, 0.25] x [-0.75, 0.75]), rays
    with one and with two direction components exactly 0 (+0 and -0).  In the object's frame such a component divides the slab's two distances to
    +-inf: -inf / +inf when the origin lies inside the slab (no constraint), both +inf or both -inf when it lies outside (a miss).  Stated flags and
    rows (exact: with an identity rotation o = o_w + tow is one rounding and the slab distances divide by +-1 or are the same fp32 operations):
      straight through along -z from above        flag 1, lo = o_z - 0.75, hi = o_z + 0.75
      the same, direction (-0, -0, -1)            the same lo and hi (the object-frame direction keeps its negative zeros)
      parallel beside the box (x outside)         flag 0
      parallel beside the box (y outside)         flag 0
      one zero component, (0.6, 0, -0.8), y inside flag 1, the row of the fp32 slab test
      one zero component, y outside               flag 0
      origin inside the box                       flag 1, lo = 0, hi = the exit
      box behind the origin (+z from above)       flag 0
      t_max short of the box                      flag 0
      t_max inside the box                        flag 1, hi == t_max bit for bit
      t_max exactly at the entry                  flag 0 (lo < hi fails)
    A row with flag 0 is zero; entry = lo; nothing is NaN or infinite."""
    sc = scene; ds, _ = trained; f = np.float32
    tow = np.array([0.25, -0.5, 0.125], f); mn = np.array([-0.5, -0.25, -0.75], f); mx = -mn
    Tow = np.eye(4, dtype=f); Tow[:3, 3] = tow
    obj = pkg.ObjectNeRF(ds, pkg.default_config(**tsr.BASE), sc.objects[0]["cls"], ss.colmajor(Tow), mn, mx)
    try:
        z = f(0.0); nz = f(-0.0)
        top = np.array([0.125, 0.0625, 3.0], f) - tow                     # object frame (0.125, 0.0625, 3): above the box, inside the x and y slabs
        cases = [  # world origin, direction, t_max, flag
            (top, [z, z, -1], np.inf, 1), (top, [nz, nz, -1], np.inf, 1),
            (np.array([0.75, 0.0, 3.0], f) - tow, [z, z, -1], np.inf, 0), (np.array([0.0, -0.3, 3.0], f) - tow, [z, nz, -1], np.inf, 0),
            (np.array([-1.0, 0.125, 1.5], f) - tow, [0.6, z, -0.8], np.inf, 1), (np.array([-1.0, 0.375, 1.5], f) - tow, [0.6, z, -0.8], np.inf, 0),
            (np.array([0.25, -0.125, 0.5], f) - tow, [z, z, -1], np.inf, 1), (np.array([0.25, -0.125, 0.5], f) - tow, [z, -1, nz], np.inf, 1),
            (top, [z, z, 1], np.inf, 0),
            (top, [z, z, -1], 2.0, 0), (top, [z, z, -1], 3.0, 1), (top, [z, z, -1], 2.25, 0), (top, [z, z, -1], 2.2500002, 1),
            (top, [z, z, -1], 100.0, 1),
        ]
        o_w = np.stack([c[0] for c in cases]).astype(f); d_w = np.array([c[1] for c in cases], f); t_max = np.array([c[2] for c in cases], f)
        rows, entry = pkg.scene_cast_rays([obj], pkg.scene_rays(o_w, d_w, t_max, np.arange(len(cases))), 0)
        assert np.isfinite(rows).all() and np.isfinite(entry).all()
        for i, (ow, dw, tm, flag) in enumerate(cases):
            M = ss.colmajor(Tow).astype(f); o = (_rot3_32(M, ow.astype(f)) + tow).astype(f); d = _rot3_32(M, np.array(dw, f))
            hit, t0, t1 = _slab32(mn, mx, o, d)
            lo, hi = max(t0, f(0)), min(t1, f(tm))
            assert bool(hit and lo < hi) == bool(flag), (i, hit, t0, t1)                # the stated flag is what IEEE gives the slab test
            assert rows[i, 8] == flag and rows[i, 9] == 1.0, i
            want = np.concatenate([o, d, [lo, hi]]).astype(f) if flag else np.zeros(8, f)
            assert np.array_equal(_bits(rows[i, :8]), _bits(want)), (i, rows[i], want)
            assert _bits(entry[i:i + 1])[0] == _bits(np.array([lo if flag else 0], f))[0], i
        # the rows spelled out
        assert rows[0, 6] == f(2.25) and rows[0, 7] == f(3.75) and np.array_equal(rows[1, 6:8], rows[0, 6:8])
        assert np.signbit(rows[1, 3:5]).all() and not np.signbit(rows[0, 3:5]).any()
        assert rows[6, 6] == 0.0 and rows[6, 7] == f(1.25) and rows[7, 6] == 0.0 and rows[7, 7] == f(0.125)
        assert _bits(rows[10, 7:8])[0] == _bits(np.array([3.0], f))[0] and rows[10, 6] == f(2.25)
        assert _bits(rows[12, 7:8])[0] == _bits(np.array([2.2500002], f))[0]
        assert rows[13, 7] == f(3.75)
        # and the whole call on them: an untrained object, every output finite, a miss the background
        out = pkg.cast_scene([obj], pkg.scene_rays(o_w, d_w, t_max, np.arange(len(cases))), 0.5)
        assert all(np.isfinite(a).all() for a in out)
        miss = rows[:, 8] == 0
        assert (out[0][miss] == 1.0).all() and (out[1][miss] == 0).all() and (out[2][miss] == 0).all() and (out[3][miss] == -1).all()
        assert (out[4][miss] == 0).all() and (out[5][miss] == 0).all() and (out[6][miss] == -1).all()
    finally:
        obj.close()


# ---------------------------------------------------------------------------------------------------------------- 6: independence
def test_independence(pkg, setup):       # noqa: F811
    """Test 6: the rect's camera rays shuffled, a subset of 37, and repeated to kRenderChunkRays + 100 (a pass boundary inside the list): every ray's
    seven outputs are its own bits; equal arguments give equal bits."""
    s = setup; objs = s["objs3"]
    rays, _ = pkg.camera_rays(_K(s["sc"]), s["pose"], s["q"]); P = rays.shape[0]
    base = pkg.cast_scene(objs, rays, 0.3)
    _same_bits(pkg.cast_scene(objs, rays, 0.3), base, "equal arguments")
    assert (base[6] >= 0).sum() >= 50
    rng = np.random.RandomState(12)
    perm = rng.permutation(P)
    _same_bits(pkg.cast_scene(objs, rays[perm], 0.3), [a[perm] for a in base], "shuffled")
    sub = rng.choice(P, 37, replace=False)
    _same_bits(pkg.cast_scene(objs, rays[sub], 0.3), [a[sub] for a in base], "subset")
    rep = (np.arange(CHUNK + 100) * 7 + 3) % P
    _same_bits(pkg.cast_scene(objs, rays[rep], 0.3), [a[rep] for a in base], "pass boundary")


# ---------------------------------------------------------------------------------------------------------------- 7: the composite
def np_crossing(t, alpha, count, entry, thr):
    """NumPy reference of the cast's hit outputs: lists [K, P, 64] with count [K, P] and entry [K, P], merged by (t, list, slot) as
    tests/test_scene_probe.py's np_first_hit merges them, the transmittance in fp64.  Per ray: has a crossing 1 - T_{i+1} > thr; the fp32 t_i of the
    first one; its list; near = some T_{i+1} within TIE (relative) of 1 - thr; hit_t = p + f (t_i - p) in fp64 with
    f = clamp(ln(T_i / (1 - thr)) / (-ln(1 - alpha_i)), 0, 1) (0 when alpha_i = 1), p = the previous t of the same list or its entry; p; and the
    first-order bound of the fp32 evaluation of hit_t.  Counting roundings (each at most U relative to its result):
      T_i              the merged product of i factors 1 - alpha_j: i subtractions, fewer than i multiplications among them (the scans') and two
                       more per block of 64 begun (by the carried transmittance and by the first half-wave's), b = i // 64 + 1 blocks
                                                                                                -> n_T U relative, n_T = 2 i + 2 b
      x = T_i / (1 - thr)   the subtraction and the division                                    -> (n_T + 2) U relative
      N = ln x         x's error is absolute in the logarithm, logf adds LOG_ULP ulp of N       -> (n_T + 2) U + 2 LOG_ULP U |N|
      D = -ln(1 - alpha_i)  the subtraction (absolute in the logarithm) and logf                -> U + 2 LOG_ULP U D
      f = N / D        -> (E_N + f E_D) / D + U f        (the clamp does not amplify)
      hit_t = fma(f, t_i - p, p)   the subtraction and the fma                                   -> (t_i - p) (E_f + U f) + U hit_t
    The bound scales with 1 / D and is capped at the interval length t_i - p, which the clamp guarantees."""
    K, P = count.shape
    thr = np.float64(np.float32(thr)); slot = np.arange(64)
    valid = slot[None, None, :] < count[..., None]
    prev = np.concatenate([entry[..., None], t[..., :-1]], -1)

    def flat(x):
        return x.transpose(1, 0, 2).reshape(P, K * 64)
    tt = flat(np.where(valid, t, np.float32(np.inf))).astype(np.float32); aa = flat(np.where(valid, alpha, 0.0)).astype(np.float64); vv = flat(valid)
    pp = flat(prev).astype(np.float64)
    kk = flat(np.broadcast_to(np.arange(K)[:, None, None], (K, P, 64))); ii = np.broadcast_to(slot, (P, K, 64)).reshape(P, K * 64)
    order = np.lexsort((ii, kk, tt), axis=-1)
    tt, aa, kk, vv, pp = (np.take_along_axis(x, order, 1) for x in (tt, aa, kk, vv, pp))
    om = 1.0 - aa
    incl = np.cumprod(om, axis=1); excl = np.concatenate([np.ones((P, 1)), incl[:, :-1]], 1)
    cross = vv & (1.0 - incl > thr)
    has = cross.any(1); first = cross.argmax(1); r = np.arange(P)
    near = (vv & (np.abs(incl / (1.0 - thr) - 1.0) < TIE)).any(1)
    ti = tt[r, first].astype(np.float64); Ti = excl[r, first]; omi = om[r, first]; p = pp[r, first]
    with np.errstate(divide="ignore", invalid="ignore"):
        N = np.log(Ti / (1.0 - thr)); D = -np.log(omi)
        f = np.where(omi == 0.0, 0.0, np.clip(N / D, 0.0, 1.0))
        E_N = (2 * first + 2 * (first // 64 + 1) + 2) * U + 2 * LOG_ULP * U * np.abs(N); E_D = U + 2 * LOG_ULP * U * D
        E_f = np.where(omi == 0.0, 0.0, (E_N + f * E_D) / D + U * f)
    ht = p + f * (ti - p)
    bound = np.minimum((ti - p) * (E_f + U * f) + U * np.abs(ht), ti - p)
    z = np.float32(0)
    return (has, np.where(has, tt[r, first], z).astype(np.float32), np.where(has, kk[r, first], -1).astype(np.int32), near,
            np.where(has, ht, 0.0), np.where(has, p, 0.0), np.where(has, bound, 0.0))


def _check_crossing(got, t, alpha, count, entry, thr, cap=0.01):
    """hit_sample_t / hit_instance of a cast output exactly the reference's first crossing, hit_t within the bound, p <= hit_t <= hit_sample_t;
    rays near a tie left out of the first two, at most `cap` of the rays that have a crossing.  Returns the worst error / bound."""
    has, ts, hk, near, ht, p, bound = np_crossing(t, alpha, count, entry, thr)
    left_out = int((near & has).sum())
    ok = ~near
    assert left_out <= cap * max(int(has.sum()), 1), (left_out, int(has.sum()))
    assert np.array_equal(got[6][ok], hk[ok]) and np.array_equal(_bits(got[5])[ok], _bits(ts)[ok])
    hit = got[6] >= 0
    assert (got[4][hit] <= got[5][hit]).all() and (got[4][~hit] == 0).all() and (got[5][~hit] == 0).all()
    g = ok & has
    assert (got[4][g].astype(np.float64) >= p[g].astype(np.float32)).all()              # (p is an fp32 number: a list's t or its entry)
    err = np.abs(got[4][g].astype(np.float64) - ht[g])
    assert (err <= bound[g]).all(), (float(err.max()), int((err > bound[g]).sum()))
    ratio = float((err[bound[g] > 0] / bound[g][bound[g] > 0]).max()) if (bound[g] > 0).any() else 0.0
    print("crossing at %.1f: %d rays, %d crossings, %d near a tie left out, hit_t worst error / bound %.3f (largest error %.3g)"
          % (thr, has.size, int(has.sum()), left_out, ratio, float(err.max()) if err.size else 0.0))
    return ratio


def _entries(t, seed):
    """An entry row for caller lists: each list's box entry, up to 0.2 in front of its first t."""
    rng = np.random.RandomState(seed)
    return (t[..., 0] - rng.uniform(0.0, 0.2, t.shape[:2])).astype(np.float32)


@pytest.mark.parametrize("K,equal_t", tsp.ADVERSARIAL)
def test_composite_hook_on_adversarial_lists(pkg, K, equal_t):
    """Test 7: mon_debug_scene_cast_composite on _adversarial's lists (tests/test_scene_probe.py's recipe and seeds, K = 1, 3 and 16, equal t on and
    off) at the thresholds 0.2, 0.5 and 0.8: rgb, dist / dn, opacity and instance are mon_debug_scene_composite's bits; hit_sample_t and hit_instance
    equal the fp64 merge's first crossing away from ties at 1 - threshold (at most 1 % of the rays that have a crossing left out); hit_t lies within
    np_crossing's first-order bound of the fp64 closed form and p <= hit_t <= hit_sample_t.  Worst error / bound seen on an MI355X: see DESIGN.md
    3.4c-3."""
    worst = 0.0
    for n_draw, (t, alpha, rgb, count, dn) in enumerate(tsp.adversarial_draws(K, equal_t)):
        entry = _entries(t, 900 + K + n_draw)
        want = pkg.scene_composite(t, alpha, rgb, count, dn)
        for thr in (0.2, 0.5, 0.8):
            got = pkg.scene_cast_composite(t, alpha, rgb, count, entry, thr)
            _same_bits((got[0], (got[1] / dn).astype(np.float32), got[2], got[3]), want, (K, equal_t, thr))
            worst = max(worst, _check_crossing(got, t, alpha, count, entry, thr))
        probe = pkg.scene_probe_composite(t, alpha, rgb, count, dn)                       # 0.5 is the probe's rule
        got = pkg.scene_cast_composite(t, alpha, rgb, count, entry, 0.5)
        _same_bits(((got[5] / dn).astype(np.float32), got[6]), probe[4:], "the probe's hit")
    print("K %d equal_t %d: hit_t worst error / bound %.3f" % (K, equal_t, worst))


def test_composite_hook_edge_rows(pkg):
    """Test 7's edge rows, with the list in question alone and as the last of three: an empty list (no hit, the background), a single sample that
    does not cross, 64 samples of alpha 0, alpha exactly 1 at the crossing (f = 0: hit_t = p), a crossing at slot 0 (p = the entry row, not 0),
    a crossing at a later slot (p = the previous t of that list)."""
    rng = np.random.RandomState(9); f = np.float32
    for K, k in ((1, 0), (3, 2)):
        t, alpha, rgb, count, dn = tsr._adversarial(rng, K, 7)
        entry = _entries(t, 77)
        count[:] = 0; alpha[:] = 0.25
        count[k, 1] = 1; alpha[k, 1, 0] = 0.3                       # a single sample that does not cross 0.5
        count[k, 2] = 64; alpha[k, 2] = 0.0                        # 64 samples of alpha 0
        count[k, 3] = 64; alpha[k, 3, 0] = 0.1; alpha[k, 3, 1] = 1.0      # alpha exactly 1 at the crossing, slot 1
        count[k, 4] = 64; alpha[k, 4, 0] = 0.75                    # a crossing at slot 0
        count[k, 5] = 64; alpha[k, 5, :3] = 0.25                   # 1 - 0.75^3 = 0.578: a crossing at slot 2
        count[k, 6] = 1; alpha[k, 6, 0] = 1.0                      # alpha 1 at slot 0: hit_t = the entry
        got = pkg.scene_cast_composite(t, alpha, rgb, count, entry, 0.5)
        _same_bits((got[0], (got[1] / dn).astype(np.float32), got[2], got[3]), pkg.scene_composite(t, alpha, rgb, count, dn), K)
        assert got[6].tolist() == [-1, -1, -1, k, k, k, k]
        assert got[4][:3].tolist() == [0.0] * 3 and got[5][:3].tolist() == [0.0] * 3
        assert (got[0][0] == 1.0).all() and got[2][0] == 0.0 and got[3][0] == -1 and (got[0][2] == 1.0).all() and got[2][2] == 0.0
        assert got[5][3] == t[k, 3, 1] and got[4][3] == t[k, 3, 0]                                   # f = 0: p, the previous sample
        assert got[5][4] == t[k, 4, 0] and entry[k, 4] < got[4][4] < t[k, 4, 0]                      # inside [entry, t_0], not measured from 0
        f4 = np.log(1.0 / 0.5) / -np.log(1.0 - np.float64(f(0.75)))
        assert abs(got[4][4] - (entry[k, 4] + f4 * (np.float64(t[k, 4, 0]) - entry[k, 4]))) < 1e-5
        assert got[5][5] == t[k, 5, 2] and t[k, 5, 1] <= got[4][5] <= t[k, 5, 2]
        assert got[5][6] == t[k, 6, 0] and got[4][6] == entry[k, 6]
        _check_crossing(got, t, alpha, count, entry, 0.5, cap=1.0)
        lo = pkg.scene_cast_composite(t, alpha, rgb, count, entry, 0.2)                              # a lower threshold: the single 0.3 sample crosses
        assert lo[6].tolist() == [-1, k, -1, k, k, k, k] and entry[k, 1] < lo[4][1] < t[k, 1, 0]
        assert lo[5][5] == t[k, 5, 0] and lo[5][3] == t[k, 3, 1]                                      # (alpha 0.1 at slot 0 does not cross 0.2)


# ---------------------------------------------------------------------------------------------------------------- 8: end to end
def test_end_to_end_on_trained_objects(pkg, setup):       # noqa: F811
    """Test 8: the rect's camera rays against the three objects on their true boxes, at the thresholds 0.2, 0.5 and 0.8.  hit_t lies within one
    sample interval of hit_sample_t (the gap to the previous sample, which jitter makes at most twice the stride (hi - lo) / 64 of the hit object's
    row) and equals the fp64 closed form on the dumped lists within test 7's bound; per ray hit_t is non-decreasing in the threshold up to the two
    bounds (a later crossing lies in a later interval of the same list, or in a box further along the ray: the true boxes are disjoint along these
    rays); a ray with a hit, recast with t_max = half its first box entry, gives opacity 0 and instance -1; rays that miss every box give rgb 1 and
    zeros / -1 (the rect's, and every ray turned round so that the boxes lie behind its origin)."""
    s = setup; o = s["objs"]; objs = [o["a0"], o["a1"], o["a2"]]
    rays, dn = pkg.camera_rays(_K(s["sc"]), s["pose"], s["q"]); P = rays.shape[0]
    t, a, c, n = tsr._dump(pkg, objs, s["rect"], s["pose"])
    rr = [pkg.scene_cast_rays(objs, rays, k) for k in range(3)]
    rows = np.stack([x[0] for x in rr]); entry = np.stack([x[1] for x in rr]); flag = rows[..., 8] > 0
    out = {thr: pkg.cast_scene(objs, rays, thr) for thr in (0.2, 0.5, 0.8)}
    ref = {}
    for thr, got in out.items():
        _check_crossing(got, t, a, n, entry, thr)
        ref[thr] = np_crossing(t, a, n, entry, thr)
        hit = got[6] >= 0
        stride = ((rows[..., 7] - rows[..., 6]) / 64.0)[np.maximum(got[6], 0), np.arange(P)]
        gap = got[5] - got[4]
        assert (gap[hit] >= 0).all() and (gap[hit] <= 2.0 * stride[hit] * (1 + 1e-5)).all()
        assert hit.sum() >= 50
    for lo_thr, hi_thr in ((0.2, 0.5), (0.5, 0.8)):
        both = (out[lo_thr][6] >= 0) & (out[hi_thr][6] >= 0)
        assert np.array_equal(both, out[hi_thr][6] >= 0)                                   # a hit at the higher threshold is one at the lower
        slack = ref[lo_thr][6] + ref[hi_thr][6]
        assert (out[lo_thr][4][both] <= out[hi_thr][4][both] + slack[both]).all()
        assert (out[lo_thr][5][both] <= out[hi_thr][5][both]).all()
    got = out[0.5]; hit = got[6] >= 0
    first_entry = np.where(flag, rows[..., 6], np.inf).min(0)
    assert (first_entry[hit] > 0).all() and np.isfinite(first_entry[hit]).all()
    short = rays[hit].copy(); short["t_max"] = (first_entry[hit] * np.float32(0.5)).astype(np.float32)
    cut = pkg.cast_scene(objs, short, 0.5)
    assert (cut[2] == 0).all() and (cut[3] == -1).all() and (cut[0] == 1.0).all() and (cut[6] == -1).all() and (cut[4] == 0).all()
    none = ~flag.any(0)                                                                 # the rect's rays that miss every box, if it has any ...
    away = rays.copy(); away["d"] = -rays["d"]                                          # ... and the same rays turned round: every box lies behind
    assert all((pkg.scene_cast_rays(objs, away, k)[0][:, 8] == 0).all() for k in range(3))
    for g, m in [(x, none) for x in out.values()] + [(pkg.cast_scene(objs, away, 0.2), np.ones(P, bool))]:
        assert (g[0][m] == 1.0).all() and (g[1][m] == 0).all() and (g[2][m] == 0).all() and (g[3][m] == -1).all()
        assert (g[4][m] == 0).all() and (g[5][m] == 0).all() and (g[6][m] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- 9, 10, 11
def test_mixed_network_shapes(pkg, ss, setup):       # noqa: F811
    """Test 9: a 32 x 2 object and a 64 x 1 object cast together (each through its own keyed instantiation), as the probe's test of mixed shapes: the
    bit rule of test 4 holds.  And no camera is involved: an object of a dataset with other intrinsics joins the list (the probe refuses it)."""
    s = setup; objs = s["objs"]; sc = s["sc"]
    rays, dn = pkg.camera_rays(_K(sc), s["pose"], s["q"])
    for lst in ([objs["n2"], objs["a1"]], [objs["a1"], objs["b0"], objs["n2"]]):
        want = pkg.probe_scene(lst, s["q"], s["pose"])
        _same_bits(_as_probe(pkg.cast_scene(lst, rays, 0.5), dn), want, len(lst))
        assert (want[2] > 0.5).sum() >= 50
    ds2 = pkg.Dataset(0, sc.H, sc.W, sc.fx * 1.5, sc.fy * 1.5, sc.cx, sc.cy, sc.n_views)
    ob = sc.objects[1]
    other = pkg.ObjectNeRF(ds2, pkg.default_config(**tsr.BASE), ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    try:
        with pytest.raises(pkg.MonError) as e:
            pkg.probe_scene([objs["a0"], other], s["q"], s["pose"])
        assert e.value.code == 1
        alone = pkg.cast_scene([objs["a0"]], rays, 0.5)
        both = pkg.cast_scene([objs["a0"], other], rays, 0.5)
        assert all(np.isfinite(x).all() for x in both) and set(np.unique(both[3])) <= {-1, 0, 1}
        untouched = pkg.scene_cast_rays([objs["a0"], other], rays, 1)[0][:, 8] == 0      # rays that miss the other object's box: object 0 alone
        assert untouched.sum() > 100
        _same_bits([x[untouched] for x in both], [x[untouched] for x in alone], "the other object's misses")
    finally:
        other.close(); ds2.close()


def test_read_only(pkg, setup):       # noqa: F811
    """Test 10: parameters (all three copies), mon_object_info_get and the skip statistics of both sides are identical before and after casts on both
    sides, with skipping off and on (the grids built beforehand, as a scene render builds them): the state comparison of the probe's test_read_only."""
    s = setup; objs = s["objs3"]
    rays, _ = pkg.camera_rays(_K(s["sc"]), s["pose"], s["q"])
    try:
        for skip in (False, True):
            for o in objs:
                o.set_render_skip(skip, 1e-3)
            for side in (0, 1):
                pkg.render_scene(objs, s["rect"], s["pose"], side)                     # (skip on: this builds the side's grids where they are stale)
            before = [tsp._state(o) for o in objs]
            for side in (0, 1):
                out = pkg.cast_scene(objs, rays, 0.4, side)
                assert (out[6] >= 0).sum() >= 50
            for o, b in zip(objs, before):
                tsp._same_state(tsp._state(o), b)
    finally:
        for o in objs:
            o.set_render_skip(False)


def test_online(pkg, ss, setup):       # noqa: F811
    """Test 11: before any publication mon_online_cast_rays returns MON_ERR_STATE; one cast from a second thread while the manager's objects still
    train returns MON_OK with finite outputs; once they are idle it equals mon_scene_cast(side 1) of the manager's objects bit for bit, with the
    manager's indices in both instance outputs.  Objects on two logical devices: MON_ERR_ARG from mon_scene_cast."""
    s = setup; sc = s["sc"]
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    m = pkg.OnlineManager(cfg, False, 40)
    m.init(); m.dataset_init(sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W, sc.n_views)
    v = 7; rect = np.array([v, 140, 108, 24, 40], np.uint32); pose = tsr._pose(ss, sc, v)
    rays, _ = pkg.camera_rays(_K(sc), pose, pkg.rect_queries(rect))
    with pytest.raises(pkg.MonError) as e:
        m.cast_rays(rays, 0.5)
    assert e.value.code == 5
    seen = dict(n=0, err=None)

    def planner():
        try:
            out = m.cast_rays(rays, 0.1)
            assert all(np.isfinite(a).all() for a in out) and set(np.unique(out[3])) <= {-1, 0, 1, 2} and set(np.unique(out[6])) <= {-1, 0, 1, 2}
            seen["n"] += 1
        except Exception as ex:        # noqa: BLE001 -- reported by the main thread
            seen["err"] = ex

    calls = 100
    ids = tsr._online_feed(pkg, ss, sc, m, 3, calls)
    assert tsr._wait_trained(m, ids, 2)                                                # every object has published
    th = threading.Thread(target=planner); th.start(); th.join(timeout=120)
    still = [m.object_info(i)["train_calls"] for i in ids]
    m.wait_threads_end()
    assert seen["err"] is None and seen["n"] == 1, seen
    print("online: train calls when the cast was through:", still)
    assert min(still) < calls                                                           # they were still training
    got = m.cast_rays(rays, 0.5)
    _same_bits(got, pkg.cast_scene([m.object(i) for i in ids], rays, 0.5, side=1), "side 1")
    assert (got[2] > 0.5).mean() > 0.02 and set(np.unique(got[6])) - {-1} and set(np.unique(got[6])) <= {-1, 0, 1, 2}
    m.close()
    pkg.set_logical_devices(2)
    try:
        ds0, o0 = ge.make_problem(pkg, sc, tsr.BASE, device=0, obj_index=0)
        ds1, o1 = ge.make_problem(pkg, sc, tsr.BASE, device=1, obj_index=1)
        with pytest.raises(pkg.MonError) as e:
            pkg.cast_scene([o0, o1], rays, 0.5)
        assert e.value.code == 1
        for o in (o0, o1, ds0, ds1):
            o.close()
    finally:
        pkg.set_logical_devices(0)
