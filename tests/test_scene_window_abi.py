"""CPU-side checks (no device needed) of the window-refinement boundary (include/mon_core.h): mon_window_default, mon_window_frames,
mon_scene_window_loss, mon_scene_refine_window, mon_online_refine_window, mon_object_set_pose and mon_online_set_object_pose are declared, exported and bound
with the header's signatures; mon_window_frames (host only) returns the order of first appearance and rejects non-contiguous frames, 33 frames and NULL
arguments; every argument error of the three compute calls that can be formed without a device-resident object is MON_ERR_ARG before any device work.  (The
rows that need objects are in tests/test_scene_window.py.)"""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p

NEW = ("mon_window_default", "mon_window_frames", "mon_scene_window_loss", "mon_scene_refine_window", "mon_online_refine_window", "mon_object_set_pose",
       "mon_online_set_object_pose")
MON_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    for name in ("window_frames", "window_default", "scene_window_loss", "scene_refine_window"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.ObjectNeRF.set_pose) and callable(pkg.OnlineManager.refine_window) and callable(pkg.OnlineManager.set_object_pose)
    # the struct has the header's layout: uint32, int32, two floats
    assert C.sizeof(pkg.WindowParams) == 16
    assert [f for f, _ in pkg.WindowParams._fields_] == ["n_fixed_frames", "refine_objects", "lr_obj_trans", "lr_obj_rot"]
    txt = open(os.path.join(ROOT, "include", "mon_core.h")).read()
    m = re.search(r"typedef struct mon_window_params \{(.*?)\} mon_window_params;", txt, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)\s+([\w, ]+);", body) == [("uint32_t", "n_fixed_frames"), ("int32_t", "refine_objects"), ("float", "lr_obj_trans, lr_obj_rot")]


def test_window_default(pkg):
    w = pkg.window_default()
    assert (w.n_fixed_frames, w.refine_objects) == (1, 1)
    assert w.lr_obj_trans == np.float32(2e-3) and w.lr_obj_rot == np.float32(4e-3)
    d = pkg.pose_refine_default()
    assert (w.lr_obj_trans, w.lr_obj_rot) == (d.lr_trans, d.lr_rot)                      # mon_pose_refine_default's steps
    assert pkg.window_default(n_fixed_frames=2, refine_objects=0).n_fixed_frames == 2
    assert pkg.lib().mon_window_default(None) == MON_ERR_ARG


def _boxes(frame_ids):
    return np.array([[f, 0, 0, 4, 4] for f in frame_ids], np.uint32)


def test_window_frames(pkg):
    L = pkg.lib()
    assert pkg.window_frames(_boxes([7, 7, 3, 9, 9, 9, 0])).tolist() == [7, 3, 9, 0]         # order of first appearance, not sorted
    assert pkg.window_frames(_boxes([5])).tolist() == [5]
    assert pkg.window_frames(_boxes(range(32))).tolist() == list(range(32))
    assert pkg.window_frames(_boxes([k // 2 for k in range(64)])).tolist() == list(range(32))
    ids = np.full(32, 77, np.uint32); n = C.c_size_t(99)

    def rc(obs, n_obs=None, dst=ids, cnt=n):
        return L.mon_window_frames(_p(obs), (0 if obs is None else obs.shape[0]) if n_obs is None else n_obs, _p(dst), None if cnt is None else C.byref(cnt))
    assert rc(_boxes([1, 2, 1])) == MON_ERR_ARG and b"contiguous" in L.mon_last_error()     # frame 1 comes back after frame 2
    assert rc(_boxes([4, 4, 5, 5, 6, 4])) == MON_ERR_ARG
    assert rc(_boxes(range(33))) == MON_ERR_ARG and b"32" in L.mon_last_error()
    assert rc(None, n_obs=1) == MON_ERR_ARG
    assert rc(_boxes([1]), dst=None) == MON_ERR_ARG
    assert rc(_boxes([1]), cnt=None) == MON_ERR_ARG
    assert n.value == 99                                                                    # a rejected call writes no count
    assert rc(_boxes([3, 3, 8])) == 0 and n.value == 2 and ids[:2].tolist() == [3, 8]


def test_argument_errors_need_no_device(pkg):
    """NULL obs / Twc16s / p / w, no boxes, non-contiguous frames, 33 frames, n_fixed_frames above F, negative and non-finite object step sizes,
    refine_objects without a fixed frame or without Tow16s, a bad schedule, NULL objs, n_objs 0 and above 256, a NULL element of objs, a NULL manager:
    MON_ERR_ARG with the outputs untouched, whether or not a device is present (no object exists, so nothing can reach one)."""
    L = pkg.lib(); prm = pkg.pose_refine_default(iters=2, rays_per_iter=256); wp = pkg.window_default()
    boxes = _boxes([0, 0, 1, 2]); T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (3, 1)); Tow = T[:1].copy()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    loss = C.c_float(7.0); fl = np.full(3, 7.0, np.float32); cg = np.full(18, 7.0, np.float32); og = np.full(6, 7.0, np.float32)
    trace = np.full(3, 7.0, np.float32); ftrace = np.full(9, 7.0, np.float32); inc = np.full(4, 7, np.uint8)
    T_in = T.copy(); Tow_in = Tow.copy()

    def loss_rc(objs=nulls, n=1, obs=boxes, poses=T, tow=None, p=prm):
        return L.mon_scene_window_loss(objs, n, 0, _p(obs), 0 if obs is None else obs.shape[0], _p(poses), _p(tow), None if p is None else C.byref(p), 0, None,
                                       C.byref(loss), _p(fl), _p(cg), _p(og))

    def refine_rc(objs=nulls, n=1, obs=boxes, poses=T, tow=Tow, p=prm, c=None, w=wp):
        return L.mon_scene_refine_window(objs, n, 0, _p(obs), 0 if obs is None else obs.shape[0], None if p is None else C.byref(p),
                                         None if c is None else C.byref(c), None if w is None else C.byref(w), _p(poses), _p(tow), _p(trace), _p(ftrace))

    def online_rc():
        return L.mon_online_refine_window(None, _p(boxes), boxes.shape[0], C.byref(prm), None, C.byref(wp), _p(T), _p(Tow), 1, _p(inc), _p(trace), _p(ftrace))
    empty = np.zeros((0, 5), np.uint32)
    common = (dict(objs=None), dict(obs=None), dict(poses=None), dict(p=None), dict(obs=empty), dict(obs=_boxes([1, 2, 1])), dict(obs=_boxes(range(33))),
              dict(n=0), dict(objs=many, n=257), dict())                                  # (the last: a NULL element of objs)
    for kw in common:
        assert loss_rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
        assert refine_rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    bad_c = pkg.pose_c2f_default(); bad_c.ramp = 0.0
    for kw in (dict(w=None), dict(w=pkg.window_default(n_fixed_frames=4)), dict(w=pkg.window_default(lr_obj_trans=-1e-3)),
               dict(w=pkg.window_default(lr_obj_rot=float("nan"))), dict(w=pkg.window_default(lr_obj_trans=float("inf"))),
               dict(w=pkg.window_default(n_fixed_frames=0)), dict(tow=None), dict(c=bad_c)):
        assert refine_rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert refine_rc(w=pkg.window_default(n_fixed_frames=4)) == MON_ERR_ARG and b"n_fixed_frames" in L.mon_last_error()
    assert refine_rc(w=pkg.window_default(n_fixed_frames=0)) == MON_ERR_ARG and b"fixed frame" in L.mon_last_error()
    assert refine_rc(obs=_boxes([1, 2, 1])) == MON_ERR_ARG and b"contiguous" in L.mon_last_error()
    assert online_rc() == MON_ERR_ARG                                      # a NULL manager (the other rows need one: tests/test_scene_window.py)
    assert L.mon_object_set_pose(None, _p(Tow)) == MON_ERR_ARG and L.mon_online_set_object_pose(None, 0, _p(Tow)) == MON_ERR_ARG
    assert loss.value == 7.0 and (fl == 7.0).all() and (cg == 7.0).all() and (og == 7.0).all() and (trace == 7.0).all() and (ftrace == 7.0).all()
    assert (inc == 7).all() and np.array_equal(T, T_in) and np.array_equal(Tow, Tow_in)
