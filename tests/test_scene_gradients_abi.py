"""CPU-side checks (no device needed) of the point-gradient boundary (include/mon_core.h): mon_object_query_gradients,
mon_scene_query_gradients, mon_scene_query_lattice_gradients, mon_scene_cast_normals and the two online forms are declared, exported and bound with the
header's signatures; the diagnostic hook is exported by libmon_core_diag.so and not by the core; the new source is listed for every build; every argument
error that can be formed without a device-resident object is MON_ERR_ARG before any device work, with the outputs untouched -- a bad first level weight
and a select outside [-1, n_objs) among them.  And the fp64 reference the GPU tests hold the kernel to (tests/field_grad_reference.py) is pinned by two
second sources, torch fp64 autograd and a central difference, at random weights.  (The rows that need objects are in tests/test_scene_gradients.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p
import field_grad_reference as fgr
import pose_reference as pr

NEW = ("mon_object_query_gradients", "mon_scene_query_gradients", "mon_scene_query_lattice_gradients", "mon_scene_cast_normals",
       "mon_online_query_gradients", "mon_online_cast_normals")
DIAG = ("mon_debug_scene_gradient_rows",)
MON_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [7, 15, 17, 17, 13, 15]
    for name in ("query_object_gradients", "query_scene_gradients", "query_scene_lattice_gradients", "cast_scene_normals", "scene_gradient_rows"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.query_gradients) and callable(pkg.OnlineManager.cast_normals)


def test_diag_hook_lives_in_the_diag_library(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path()); dl = pkg.diag_lib()
    for name in DIAG:
        assert name in pkg.diag_symbols() and name not in pkg.exported_symbols()
        assert hasattr(dl, name) and not hasattr(core, name), name
        assert [_kind(a) for a in _decl(name, "mon_core_diag.h")] == [_bound(t) for t in b._DIAG_SIGS[name][1]], name
    assert len(_decl("mon_debug_scene_gradient_rows", "mon_core_diag.h")) == 8


def test_new_source_is_listed_for_every_build():
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_scene_gradients.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_scene_gradients.hip"))


def test_argument_errors_need_no_device(pkg):
    """The point queries' argument errors (NULL objs / element / points / sigma, counts, sides, non-finite points, lattice shapes), and the new ones: a
    NULL grad_log (grad_unit, normal), a select below -1 or at / above n_objs, a first level weight that is negative, NaN or infinite (the weights behind
    it need the objects' level counts: tests/test_scene_gradients.py) -- MON_ERR_ARG with a message and the outputs untouched.  Accepted arguments fail
    on the NULL object alone."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    x = np.array([[0.1, 0.2, 0.3], [1.5, -2.0, 0.25], [0, 0, 0]], np.float32); n = x.shape[0]
    f7 = lambda *s: np.full(s, 7.0, np.float32)     # noqa: E731
    sig, rgb, own, osg, nin = f7(64), f7(64, 3), np.full(64, 7, np.int32), f7(64), np.full(64, 7, np.uint32)
    gl, gs, nr, raw, r16, hx = f7(64, 3), f7(64, 3), f7(64, 3), f7(64, 4), f7(64, 16), f7(64, 3)
    w = np.ones(16, np.float32); sel = np.array([-1, 0, 1], np.int32)

    def edit(a, i, j, v):
        b = a.copy(); b[i, j] = v; return b

    def ed1(a, i, v):
        b = a.copy(); b[i] = v; return b

    def pts(objs=nulls, n_objs=2, side=0, xyz=x, n_pts=None, lw=w, select=sel, o_sig=sig, o_rest=(rgb, own, osg, nin), o_gl=gl, o_opt=(gs, nr)):
        return L.mon_scene_query_gradients(objs, n_objs, side, _p(xyz), (0 if xyz is None else xyz.shape[0]) if n_pts is None else n_pts, _p(lw), _p(select),
                                           _p(o_sig), *[_p(a) for a in o_rest], _p(o_gl), *[_p(a) for a in o_opt])
    for kw in (dict(), dict(o_rest=(None,) * 4, o_opt=(None, None)), dict(lw=None, select=None), dict(objs=None), dict(xyz=None, n_pts=3), dict(o_sig=None),
               dict(o_gl=None), dict(n_objs=0), dict(objs=many, n_objs=257), dict(n_pts=0), dict(n_pts=(1 << 22) + 1), dict(side=2), dict(side=-1),
               dict(xyz=edit(x, 0, 1, np.nan)), dict(xyz=edit(x, 2, 2, np.inf)), dict(select=ed1(sel, 1, -2)), dict(select=ed1(sel, 2, 2)),
               dict(select=ed1(sel, 0, 2 ** 31 - 1)), dict(lw=ed1(w, 0, -1.0)), dict(lw=ed1(w, 0, np.nan)), dict(lw=ed1(w, 0, np.inf)),
               dict(lw=ed1(w, 0, -0.5), select=None)):
        assert pts(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert pts(select=ed1(sel, 2, 2)) == MON_ERR_ARG and b"select" in L.mon_last_error()
    assert pts(select=ed1(sel, 1, -2)) == MON_ERR_ARG and b"select" in L.mon_last_error()
    assert pts(lw=ed1(w, 0, np.nan)) == MON_ERR_ARG and b"level weight" in L.mon_last_error()
    assert pts(o_gl=None) == MON_ERR_ARG and b"grad_log" in L.mon_last_error()
    assert pts() == MON_ERR_ARG and b"object" in L.mon_last_error()                          # accepted by the argument checks: fails on the NULL object alone
    assert pts(lw=ed1(w, 0, 0.0)) == MON_ERR_ARG and b"object" in L.mon_last_error()         # (a weight of 0 is a weight)

    o3 = np.array([0.5, -1.0, 2.0], np.float32); s3 = np.array([0.25, 0.0, -0.125], np.float32)

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), lw=w, o_sig=sig, o_gl=gl):
        return L.mon_scene_query_lattice_gradients(objs, n_objs, side, _p(o), _p(s), *shape, _p(lw), _p(o_sig), _p(rgb), _p(own), _p(osg), _p(nin), _p(o_gl),
                                                   _p(gs), _p(nr))
    for kw in (dict(), dict(lw=None), dict(objs=None), dict(o=None), dict(s=None), dict(o_sig=None), dict(o_gl=None), dict(n_objs=0), dict(shape=(0, 3, 4)),
               dict(shape=(2, 3, -7)), dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=(1 << 30, 1 << 30, 1 << 30)), dict(side=2),
               dict(o=ed1(o3, 0, np.nan)), dict(s=ed1(s3, 0, 3e38), shape=(3, 1, 1)), dict(lw=ed1(w, 0, -1.0)), dict(lw=ed1(w, 0, np.nan))):
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert lat(shape=(1 << 11, 1 << 11, 1)) == MON_ERR_ARG and b"object" in L.mon_last_error()      # 2^22 points: accepted

    u = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.75]], np.float32)
    assert L.mon_object_query_gradients(None, 0, _p(u), 3, _p(w), _p(raw), _p(gl)) == MON_ERR_ARG and b"object" in L.mon_last_error()
    assert L.mon_object_query_gradients(None, 0, _p(u), 3, None, None, _p(gl)) == MON_ERR_ARG and b"object" in L.mon_last_error()
    for bad in (edit(u, 2, 0, 1.0001), edit(u, 0, 1, -1e-6), edit(u, 1, 2, np.nan)):
        assert L.mon_object_query_gradients(None, 0, _p(bad), 3, _p(w), _p(raw), _p(gl)) == MON_ERR_ARG and b"unit cube" in L.mon_last_error()
    for args in ((0, None, 3, _p(w), _p(raw), _p(gl)), (0, _p(u), 3, _p(w), _p(raw), None), (0, _p(u), 0, _p(w), _p(raw), _p(gl)),
                 (0, _p(u), (1 << 22) + 1, _p(w), _p(raw), _p(gl)), (2, _p(u), 3, _p(w), _p(raw), _p(gl)), (0, _p(u), 3, _p(ed1(w, 0, -2.0)), _p(raw), _p(gl)),
                 (0, _p(u), 3, _p(ed1(w, 0, np.inf)), _p(raw), _p(gl))):
        assert L.mon_object_query_gradients(None, *args) == MON_ERR_ARG and L.mon_last_error(), args[0:3:2]

    rays = np.zeros(3, pkg.SCENE_RAY_DTYPE); rays["d"] = (0, 0, 1); rays["t_max"] = np.inf
    dist, op, inst, ht, hs, hi = f7(64), f7(64), np.full(64, 7, np.int32), f7(64), f7(64), np.full(64, 7, np.int32)

    def cast(objs=nulls, n_objs=1, r=rays, n_r=3, thr=0.5, lw=w, o_rgb=rgb, o_dist=dist, o_nr=nr):
        return L.mon_scene_cast_normals(objs, n_objs, 0, _p(r), n_r, C.c_float(thr), _p(lw), _p(o_rgb), _p(o_dist), _p(op), _p(inst), _p(ht), _p(hs), _p(hi),
                                        _p(hx), _p(o_nr), _p(gl))
    bad_d = rays.copy(); bad_d["d"][1] = (0, 0, 2)
    for kw in (dict(), dict(lw=None), dict(objs=None), dict(r=None), dict(n_r=0), dict(thr=0.0), dict(thr=1.0), dict(r=bad_d), dict(o_rgb=None),
               dict(o_dist=None), dict(o_nr=None), dict(n_objs=0), dict(lw=ed1(w, 0, -1.0)), dict(lw=ed1(w, 0, np.nan))):
        assert cast(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert cast(o_nr=None) == MON_ERR_ARG and b"normal" in L.mon_last_error()
    assert cast() == MON_ERR_ARG and b"object" in L.mon_last_error()
    # the online forms: a NULL manager (the other rows need one)
    assert L.mon_online_query_gradients(None, _p(x), n, _p(w), _p(sel), _p(sig), _p(rgb), _p(own), _p(osg), _p(nin), _p(gl), _p(gs), _p(nr)) == MON_ERR_ARG
    assert L.mon_online_cast_normals(None, _p(rays), 3, C.c_float(0.5), _p(w), _p(rgb), _p(dist), _p(op), _p(inst), _p(ht), _p(hs), _p(hi), _p(hx), _p(nr),
                                     _p(gl)) == MON_ERR_ARG
    # the diagnostic hook judges the same arguments
    D = pkg.diag_lib()
    for args in ((nulls, 1, 0, _p(x), n, _p(w), 0, _p(r16)), (nulls, 1, 0, _p(x), n, None, 1, _p(r16)), (nulls, 1, 0, _p(edit(x, 0, 0, np.nan)), n, _p(w), 0, _p(r16)),
                 (nulls, 1, 0, _p(x), n, _p(w), 0, None), (nulls, 1, 0, _p(x), n, _p(ed1(w, 0, -1.0)), 0, _p(r16))):
        assert D.mon_debug_scene_gradient_rows(*args) == MON_ERR_ARG
    for a in (sig, rgb, osg, gl, gs, nr, raw, r16, hx, dist, op, ht, hs):
        assert (a == 7.0).all()
    for a in (own, nin, inst, hi):
        assert (a == 7).all()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on the CPU
SHAPES = [dict(L=16, W=64, NH=1), dict(L=5, W=32, NH=2)]             # 64 x 1 with 16 levels (base.json's); 32 x 2 with an odd level count
H = 1e-9


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d_L%d" % (s["W"], s["NH"], s["L"]))
def pinned(request, orc):
    """A network of random fp16 weights on base.json's grid of L levels, 600 random unit-cube points, one random weight vector, and the reference there."""
    s = request.param; rng = np.random.RandomState(100 + s["L"])
    off, scl, res = pr.level_table(orc, orc.default_config(n_levels=s["L"], n_neurons=s["W"], n_hidden_layers=s["NH"]))
    Ep = ((2 * s["L"] + 15) // 16) * 16; nm = fgr.n_mlp_params(s["W"], s["NH"], Ep)
    prm = np.concatenate([rng.normal(0, 0.35, nm), rng.uniform(-1.0, 1.0, 2 * int(off[s["L"]]))]).astype(np.float16)
    net = fgr.net_of(prm.view(np.uint16), off, scl, res, s["L"], s["W"], s["NH"])
    u = rng.uniform(0.0, 1.0, (600, 3)).astype(np.float32)
    lw = rng.uniform(0.0, 1.0, s["L"]); lw[rng.randint(s["L"])] = 0.0        # (the range of the windows mon_pose_c2f_weights forms; one level off)
    return net, u, lw, fgr.gradient(net, u, lw)


def test_reference_against_torch_autograd(pinned, tmp_path):
    """The numpy derivative against torch fp64 autograd of the same graph (child process), at random level weights: per point within 1e-10 of the point's
    largest component (floored at 1e-6 of the largest over all points: both are fp64 sums of a few thousand products of like size, so their error is
    near 1e-13 of that scale); raw3 equal to 1e-12."""
    net, u, lw, (raw, g, per) = pinned
    raw3_t, g_t = fgr.torch_gradient(tmp_path, net, u, lw)
    scale = np.maximum(np.abs(g_t).max(1), 1e-6 * np.abs(g_t).max())
    err = np.abs(g - g_t).max(1) / scale
    print("reference vs torch autograd: worst relative error %.3g, max |grad| %.4g, points with a zero gradient %d" %
          (err.max(), np.abs(g_t).max(), (np.abs(g_t).max(1) == 0).sum()))
    assert np.abs(g_t).max() > 0 and np.abs(raw[:, 3] - raw3_t).max() <= 1e-12
    assert err.max() <= 1e-10
    assert np.abs(per.sum(0) - g).max() == 0


def _window(L, alpha):
    """the coarse-to-fine window of include/mon_core.h at position alpha: 1 below it, a cosine ramp across one level, 0 above"""
    a = alpha - np.arange(L, dtype=np.float64)
    return np.where(a <= 0, 0.0, np.where(a >= 1, 1.0, (1 - np.cos(np.pi * np.clip(a, 0, 1))) / 2))


def _central_difference(net, u, lw):
    """(err, flip, keep, cap) per point: the relative error of the reference against the difference, whether a ReLU changes sides between -h and +h on
    some axis, whether the point stays 2 h clear of every weighted level's cell faces, and the difference's own rounding relative to the gradient"""
    raw, g, _ = fgr.gradient(net, u, lw)
    gth = fgr.gather(net, u); frac = gth[0]; L = int(net["L"])
    step = np.asarray(net["scl"][:L], np.float64) * lw                                         # d frac_l / d u
    keep = np.ones(u.shape[0], bool)
    for l in range(L):
        keep &= ((frac[l] - 2 * H * step[l] > 0) & (frac[l] + 2 * H * step[l] < 1)).all(1)
    _, resid, _ = fgr.forward(net, gth)
    fd = np.zeros_like(g); flip = np.zeros(u.shape[0], bool)
    for d in range(3):
        e = np.zeros((u.shape[0], 3)); e[:, d] = H
        rp, _, mp = fgr.forward(net, gth, e, lw, resid); rm, _, mm = fgr.forward(net, gth, -e, lw, resid)
        fd[:, d] = (rp[:, 3] - rm[:, 3]) / (2 * H)
        for a, b in zip(mp, mm):
            flip |= (a != b).any(1)
    scale = np.maximum(np.abs(g).max(1), 1e-6 * np.abs(g).max())
    return np.abs(fd - g).max(1) / scale, flip, keep, 4 * 2.0 ** -53 * np.abs(raw[:, 3]) / H / scale


def test_reference_against_a_central_difference(pinned):
    """... and against (raw3(+h) - raw3(-h)) / 2h in fp64, h = 1e-9 in u, the forward's fp16 roundings held constant (field_grad_reference.forward with
    the base point's residuals).  Points within 2 h of a cell face of any weighted level are left out.  Along an axis the field is piecewise linear, so the
    difference is exact up to its own rounding, about 1e-16 |raw3| / h -- checked here to stay below the bar's 1e-5 of the gradient on the points kept --
    except where a ReLU changes sides inside [-h, h].  The bar: 1e-5 relative (to the point's largest component) on at least 99 % of the points kept.
    How many points straddle a kink depends on the level weights, which are this test's to choose.  h moves level l by h scale_l lw_l of a cell and with
    it a unit's pre-activation by about 0.3 h scale_l lw_l of its spread (measured on the 16-level network: 1.7e-4 of it at the finest level, scale
    2^19, under weights near 0.5); |z| lies inside that with probability 0.8 times it, on each of 3 axes and W units: about 4.6e-8 scale_top at W = 64,
    i.e. 2.4 % with the finest level on and 0.15 % with level 11 the finest one on.  So
      * the bar is held under a random window (position drawn in [L / 2, 3 L / 4]: the kind of weights the header tells callers to pass for normals);
      * under the fixture's random weights on every level (where the share is printed, 97.9 % on the 16-level network, and not held to 99 %) every
        point outside 1e-5 must be one where a ReLU does change sides between -h and +h: what the issue calls the remainder, checked point by point."""
    net, u, lw, _ = pinned; L = int(net["L"])
    err, flip, keep, cap = _central_difference(net, u, lw)
    # (a point is left out with probability about 12 h sum_l scale_l lw_l: some 0.1 at 16 levels, whose finest scale is near 2^19)
    assert keep.mean() > 2.0 / 3.0, keep.mean()
    print("reference vs central difference, weights on every level: %d of %d points kept, within 1e-5 on %.4f of them, %d outside, %d with a ReLU "
          "changing sides; rounding cap: worst %.3g" % (keep.sum(), u.shape[0], (err[keep] <= 1e-5).mean(), (err[keep] > 1e-5).sum(), flip[keep].sum(), cap[keep].max()))
    assert cap[keep].max() <= 1e-5
    assert flip[keep & (err > 1e-5)].all()
    win = _window(L, np.random.RandomState(7 + L).uniform(L / 2, 3 * L / 4))
    assert (win == 1).any() and (win == 0).any()
    err, flip, keep, cap = _central_difference(net, u, win)
    print("reference vs central difference, window %s: %d of %d points kept, within 1e-5 on %.4f of them, median %.3g; rounding cap: worst %.3g" %
          (np.array2string(win, precision=2), keep.sum(), u.shape[0], (err[keep] <= 1e-5).mean(), np.median(err[keep]), cap[keep].max()))
    assert keep.mean() > 2.0 / 3.0 and cap[keep].max() <= 1e-5
    assert (err[keep] <= 1e-5).mean() >= 0.99
