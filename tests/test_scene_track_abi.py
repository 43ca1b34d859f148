"""CPU-side checks (no device needed) of the camera-refinement boundary: mon_scene_pose_loss, mon_scene_refine_camera and mon_online_refine_camera are
declared, exported and bound with the header's signatures, the two diagnostics live in the diagnostics library only, and every argument error that can be
formed without a device-resident object is MON_ERR_ARG before any device work.  (The rows that need objects -- boxes of two frames, objects of two datasets,
devices or intrinsics -- are in tests/test_scene_track.py.)"""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p

NEW = ("mon_scene_pose_loss", "mon_scene_refine_camera", "mon_online_refine_camera")
NEW_DIAG = ("mon_debug_scene_pose_samples", "mon_debug_scene_composite_grad")
MON_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound(pkg):
    core = C.CDLL(pkg.lib_path()); diag = pkg.diag_lib()
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        _decl(name, "mon_core.h")
    for name in NEW_DIAG:
        assert name in pkg.diag_symbols() and hasattr(diag, name) and not hasattr(core, name), name
        _decl(name, "mon_core_diag.h")
    assert not set(NEW_DIAG) & set(pkg.exported_symbols())


def test_binding_tables_match_the_headers(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    for name in NEW:
        assert [_kind(a) for a in _decl(name, "mon_core.h")] == [_bound(t) for t in b._SIGS[name][1]], name
    for name in NEW_DIAG:
        assert [_kind(a) for a in _decl(name, "mon_core_diag.h")] == [_bound(t) for t in b._DIAG_SIGS[name][1]], name


def test_argument_errors_need_no_device(pkg):
    """NULL objs / obs / pose / params, n_objs 0 and above 256, a NULL element of objs: MON_ERR_ARG from both entry points, with a message, whether or not a
    device is present (no object exists, so nothing can reach one)."""
    L = pkg.lib(); prm = pkg.pose_refine_default(iters=2); c2f = pkg.pose_c2f_default()
    boxes = np.array([[0, 0, 0, 8, 8]], np.uint32); T = np.eye(4, dtype=np.float32).reshape(16); trace = np.zeros(3, np.float32)
    g = np.zeros(6, np.float32); loss = C.c_float(0)
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()

    def loss_rc(objs, n, obs=boxes, n_obs=1, pose=T, p=prm, side=0):
        return L.mon_scene_pose_loss(objs, n, side, _p(obs), n_obs, _p(pose), None if p is None else C.byref(p), 0, None, C.byref(loss), _p(g))

    def refine_rc(objs, n, obs=boxes, n_obs=1, pose=T, p=prm, side=0, c=None):
        return L.mon_scene_refine_camera(objs, n, side, _p(obs), n_obs, None if p is None else C.byref(p), None if c is None else C.byref(c), _p(pose),
                                         _p(trace))
    for fn in (loss_rc, refine_rc):
        assert fn(None, 1) == MON_ERR_ARG and b"objs" in L.mon_last_error()
        assert fn(nulls, 0) == MON_ERR_ARG
        assert fn(many, 257) == MON_ERR_ARG and b"257" in L.mon_last_error()
        assert fn(nulls, 4) == MON_ERR_ARG and b"null object" in L.mon_last_error()
        assert fn(nulls, 1) == MON_ERR_ARG
    # the manager's call: NULL arguments, no boxes, iters < 0 and a bad schedule before anything else
    assert L.mon_online_refine_camera(None, _p(boxes), 1, C.byref(prm), None, _p(T), _p(trace)) == MON_ERR_ARG
    cfg = os.path.join(ROOT, "ro-map_amd", "configs", "c1_small.json")
    h = C.c_void_p(None)
    if L.mon_online_create(cfg.encode(), 0, 10, C.byref(h)) == 0:
        try:
            assert L.mon_online_refine_camera(h, None, 1, C.byref(prm), None, _p(T), _p(trace)) == MON_ERR_ARG
            assert L.mon_online_refine_camera(h, _p(boxes), 1, None, None, _p(T), _p(trace)) == MON_ERR_ARG
            assert L.mon_online_refine_camera(h, _p(boxes), 1, C.byref(prm), None, None, _p(trace)) == MON_ERR_ARG
            assert L.mon_online_refine_camera(h, _p(boxes), 0, C.byref(prm), None, _p(T), _p(trace)) == MON_ERR_ARG
            neg = pkg.pose_refine_default(iters=-1)
            assert L.mon_online_refine_camera(h, _p(boxes), 1, C.byref(neg), None, _p(T), _p(trace)) == MON_ERR_ARG
            bad = pkg.pose_c2f_default(ramp=0.0)
            assert L.mon_online_refine_camera(h, _p(boxes), 1, C.byref(prm), C.byref(bad), _p(T), _p(trace)) == MON_ERR_ARG
            assert L.mon_online_refine_camera(h, _p(boxes), 1, C.byref(prm), C.byref(c2f), _p(T), _p(trace)) == 5      # MON_ERR_STATE: nothing published
        finally:
            L.mon_online_destroy(h)
    # the composite-grad diagnostic rejects empty and oversized problems before touching a device
    D = pkg.diag_lib(); z = np.zeros(64, np.float32)
    for n_rays, n_lists in ((0, 1), (1, 0), (1, 257)):
        assert D.mon_debug_scene_composite_grad(0, n_rays, n_lists, _p(z), _p(z), _p(z), _p(z.view(np.uint32)), _p(z), _p(z), _p(z), _p(z), 1.0, 1.0, 1.0, 0.05,
                                                _p(z), _p(z), _p(z), _p(z), _p(z)) == MON_ERR_ARG
