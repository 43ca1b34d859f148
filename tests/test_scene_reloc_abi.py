"""CPU-side checks (no device needed) of the wide-basin relocalisation boundary (include/mon_core.h): mon_scene_pose_loss_batch,
mon_pose_hypotheses, mon_reloc_default, mon_scene_relocalise and mon_online_relocalise are declared, exported and bound with the header's signatures; every
argument error that can be formed without a device-resident object is MON_ERR_ARG before any device work; mon_pose_hypotheses (host only) equals a numpy
restatement built on tests/pose_reference.py's counter RNG.  (The rows that need objects are in tests/test_scene_reloc.py.)"""
import ctypes as C
import math
import os
import re

import numpy as np

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p
import pose_reference as pref

NEW = ("mon_scene_pose_loss_batch", "mon_pose_hypotheses", "mon_reloc_default", "mon_scene_relocalise", "mon_online_relocalise")
MON_ERR_ARG = 1
STREAM_POSE_HYP = 6                                         # model.h kStreamPoseHyp


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    for name in ("scene_pose_loss_batch", "pose_hypotheses", "scene_relocalise", "reloc_default"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.relocalise)
    # the structs have the header's layout: three uint32; two uint32 and three floats
    assert C.sizeof(pkg.RelocParams) == 12 and C.sizeof(pkg.RelocResult) == 20
    assert [f for f, _ in pkg.RelocParams._fields_] == ["score_rays", "keep", "score_iteration"]
    assert [f for f, _ in pkg.RelocResult._fields_] == ["best_candidate", "refined", "score_candidate0", "score_best_candidate", "score_final"]


def test_reloc_default(pkg):
    r = pkg.reloc_default()
    assert (r.score_rays, r.keep, r.score_iteration) == (256, 4, 0)
    assert pkg.reloc_default(keep=2).keep == 2
    assert pkg.lib().mon_reloc_default(None) == MON_ERR_ARG


def test_argument_errors_need_no_device(pkg):
    """NULL pointers, n_poses / n_candidates outside 1..4096, more than 16384 rays per hypothesis, score_rays outside 1..16384, keep outside 1..16, n_objs 0
    and above 256, a NULL element of objs, a NULL manager: MON_ERR_ARG with the outputs untouched, whether or not a device is present (no object exists, so
    nothing can reach one)."""
    L = pkg.lib(); prm = pkg.pose_refine_default(iters=2, rays_per_iter=256); rp = pkg.reloc_default(); c2f = pkg.pose_c2f_default()
    boxes = np.array([[0, 0, 0, 8, 8]], np.uint32); T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (4, 1))
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    losses = np.full(4, 7.0, np.float32); out = np.full(16, 7.0, np.float32); scores = np.full(4, 7.0, np.float32); res = pkg.RelocResult()

    def batch_rc(objs=nulls, n=1, obs=boxes, n_obs=1, poses=T, n_poses=4, p=prm, dst=losses):
        return L.mon_scene_pose_loss_batch(objs, n, 0, _p(obs), n_obs, _p(poses), n_poses, None if p is None else C.byref(p), 0, _p(dst))

    def reloc_rc(objs=nulls, n=1, obs=boxes, n_obs=1, cands=T, n_c=4, p=prm, c=None, r=rp, dst=out):
        return L.mon_scene_relocalise(objs, n, 0, _p(obs), n_obs, _p(cands), n_c, None if p is None else C.byref(p), None if c is None else C.byref(c),
                                      None if r is None else C.byref(r), _p(dst), C.byref(res), _p(scores))

    def online_rc(mgr=None, obs=boxes, cands=T, n_c=4, p=prm, r=rp, dst=out):
        return L.mon_online_relocalise(mgr, _p(obs), 1, _p(cands), n_c, None if p is None else C.byref(p), None, None if r is None else C.byref(r), _p(dst),
                                       C.byref(res), _p(scores))
    for kw in (dict(objs=None), dict(obs=None), dict(poses=None), dict(p=None), dict(dst=None), dict(n=0), dict(objs=many, n=257), dict(n_obs=0),
               dict(n_poses=0), dict(n_poses=4097), dict(p=pkg.pose_refine_default(rays_per_iter=16385)), dict()):          # (the last: a NULL element of objs)
        assert batch_rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    for kw in (dict(objs=None), dict(obs=None), dict(cands=None), dict(p=None), dict(r=None), dict(dst=None), dict(n=0), dict(objs=many, n=257),
               dict(n_c=0), dict(n_c=4097), dict(r=pkg.reloc_default(score_rays=0)), dict(r=pkg.reloc_default(score_rays=16385)),
               dict(r=pkg.reloc_default(keep=0)), dict(r=pkg.reloc_default(keep=17)), dict()):
        assert reloc_rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert reloc_rc(r=pkg.reloc_default(keep=17)) == MON_ERR_ARG and b"keep" in L.mon_last_error()
    assert reloc_rc(r=pkg.reloc_default(score_rays=16385)) == MON_ERR_ARG and b"score_rays" in L.mon_last_error()
    for kw in (dict(), dict(mgr=None, obs=None)):
        assert online_rc(**kw) == MON_ERR_ARG, kw
    assert (losses == 7.0).all() and (out == 7.0).all() and (scores == 7.0).all()
    # mon_pose_hypotheses: NULL pointers, n = 0 and above 4096, negative and non-finite bounds
    H = np.full((4, 16), 7.0, np.float32); T0 = T[0]

    def hyp_rc(pose=T0, rot=0.1, trans=0.1, n=4, dst=H):
        return L.mon_pose_hypotheses(_p(pose), None, rot, trans, n, 1, _p(dst))
    for kw in (dict(pose=None), dict(dst=None), dict(n=0), dict(n=4097), dict(rot=-0.1), dict(trans=-0.1), dict(rot=float("nan")), dict(trans=float("inf"))):
        assert hyp_rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert (H == 7.0).all()
    assert hyp_rc() == 0


# ------------------------------------------------------------------ mon_pose_hypotheses against numpy
def _np_hypotheses(Twc16, n, max_rot, max_trans, pivot, seed):
    """include/mon_core.h's rule in float64 over pose_reference.rand01 (stream 6 keyed (seed, h, k)); poses as 4 x 4 matrices"""
    T = np.asarray(Twc16, np.float64).reshape(4, 4).T; c = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64)
    out = [T]
    for h in range(1, n):
        u = pref.rand01(seed, STREAM_POSE_HYP, h, np.arange(6)).astype(np.float64)
        rho = max_trans * (2 * u[:3] - 1)
        z = 2 * u[4] - 1; s = math.sqrt(max(0.0, 1 - z * z)); az = 2 * math.pi * u[5]
        e = np.array([s * math.cos(az), s * math.sin(az), z]); th = max_rot * np.cbrt(u[3])
        K = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
        R = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
        D = np.eye(4); D[:3, :3] = R; D[:3, 3] = c - R @ c + rho
        out.append(T @ D)
    return np.stack(out)


def _some_pose(seed):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4); T[:3, :3] = q; T[:3, 3] = rs.uniform(-1, 1, 3)           # unit scale
    return T.T.astype(np.float32).reshape(16)


def _mats(P):
    return np.asarray(P, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)


def test_pose_hypotheses_match_numpy(pkg):
    """hypothesis 0 bit-equal to the input; every element within 1e-6 of the float64 restatement (the two sides' libm differ: no bit equality asked); every
    rotation block orthonormal to 1e-6; every relative rotation angle <= max_rot + 1e-6; with max_trans = 0 the pivot stays where it was to 1e-5; equal
    arguments give equal bytes, another seed other poses."""
    n = 257
    for seed, max_rot, max_trans, pivot in ((1, math.radians(10), 0.05, None), (2, math.radians(15), 0.1, np.array([0.1, -0.2, 0.9], np.float32)),
                                            (3, math.radians(40), 0.0, np.array([-0.3, 0.1, 0.7], np.float32)), (4, 0.0, 0.0, None)):
        T0 = _some_pose(seed)
        got = pkg.pose_hypotheses(T0, n, max_rot, max_trans, pivot=pivot, seed=seed)
        assert got.shape == (n, 16) and got.dtype == np.float32
        assert np.array_equal(got[0].view(np.uint32), T0.view(np.uint32))
        ref = _np_hypotheses(T0, n, max_rot, max_trans, pivot, seed); G = _mats(got)
        err = np.abs(G - ref).max()
        print("seed %d: largest difference from the float64 restatement %.2e" % (seed, err))
        assert err <= 1e-6
        assert np.array_equal(G[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))
        R = G[:, :3, :3]
        assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-6
        rel = np.linalg.inv(_mats(T0)[0][:3, :3]) @ R                            # |R - I|_F = 2 sqrt(2) sin(angle / 2): well conditioned near 0
        ang = 2 * np.arcsin(np.minimum(np.linalg.norm(rel - np.eye(3), axis=(1, 2)) / (2 * math.sqrt(2)), 1.0))
        assert ang.max() <= max_rot + 1e-6, (ang.max(), max_rot)
        if max_rot > 0:
            assert ang.max() > 0.8 * max_rot                                    # (the ball is filled, not a shell near 0)
        if max_trans == 0.0:
            c = np.append(np.zeros(3) if pivot is None else pivot.astype(np.float64), 1.0)
            world = G @ c
            assert np.abs(world - world[0]).max() <= 1e-5
        else:
            d = np.linalg.norm((np.linalg.inv(_mats(T0)[0]) @ G)[:, :3, 3], axis=1)   # (the pivot's shift bounds the rest: rho alone when c = 0)
            assert d.max() > 0
        again = pkg.pose_hypotheses(T0, n, max_rot, max_trans, pivot=pivot, seed=seed)
        assert again.tobytes() == got.tobytes()
        if max_rot > 0 or max_trans > 0:
            other = pkg.pose_hypotheses(T0, n, max_rot, max_trans, pivot=pivot, seed=seed + 100)
            assert other[1:].tobytes() != got[1:].tobytes() and np.array_equal(other[0], got[0])
        # a prefix of a longer draw: hypothesis h does not depend on n
        assert pkg.pose_hypotheses(T0, 5, max_rot, max_trans, pivot=pivot, seed=seed).tobytes() == got[:5].tobytes()
