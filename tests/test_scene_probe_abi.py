"""CPU-side checks (no device needed) of the scene-probe boundary (include/mon_core.h): mon_scene_probe and mon_online_probe_scene are
declared, exported and bound with the header's signatures; mon_scene_query is 16 bytes with the fields pose, key, u, v; the two diagnostic hooks are exported by
libmon_core_diag.so and not by the core; every argument error that can be formed without a device-resident object is MON_ERR_ARG before any device work,
with the outputs untouched.  (The rows that need objects are in tests/test_scene_probe.py.)"""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p

NEW = ("mon_scene_probe", "mon_online_probe_scene")
DIAG = ("mon_debug_scene_probe_rays", "mon_debug_scene_probe_composite")
MON_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert len(_decl("mon_scene_probe")) == 13 and len(_decl("mon_online_probe_scene")) == 11
    for name in ("probe_scene", "scene_queries", "rect_queries", "scene_probe_rays", "scene_probe_composite"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.probe_scene)


def test_query_struct_layout(pkg):
    assert C.sizeof(pkg.SceneQuery) == 16
    assert [f for f, _ in pkg.SceneQuery._fields_] == ["pose", "key", "u", "v"]
    assert [pkg.SceneQuery.pose.offset, pkg.SceneQuery.key.offset, pkg.SceneQuery.u.offset, pkg.SceneQuery.v.offset] == [0, 4, 8, 12]
    dt = pkg.SCENE_QUERY_DTYPE
    assert dt.itemsize == 16 and dt.names == ("pose", "key", "u", "v") and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]
    txt = open(os.path.join(ROOT, "include", "mon_core.h")).read()
    m = re.search(r"typedef struct mon_scene_query \{(.*?)\} mon_scene_query;", txt, flags=re.S)
    assert m
    assert re.findall(r"(\w+)\s+([\w, ]+);", m.group(1)) == [("uint32_t", "pose"), ("uint32_t", "key"), ("float", "u, v")]
    q = pkg.rect_queries((0, 10, 20, 2, 3), pose=4)
    assert q["key"].tolist() == [0, 1, 2, 3, 4, 5] and q["u"].tolist() == [10, 11, 12, 10, 11, 12] and q["v"].tolist() == [20, 20, 20, 21, 21, 21]
    assert (q["pose"] == 4).all()


def test_diag_hooks_live_in_the_diag_library(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path()); dl = pkg.diag_lib()
    for name in DIAG:
        assert name in pkg.diag_symbols() and name not in pkg.exported_symbols()
        assert hasattr(dl, name) and not hasattr(core, name), name
        assert [_kind(a) for a in _decl(name, "mon_core_diag.h")] == [_bound(t) for t in b._DIAG_SIGS[name][1]], name


def test_new_source_is_listed_for_every_build():
    """sources.sh is what build.sh, the variant builds and the ThreadSanitizer host build (tests/tsan/build_and_run.sh, run by tests/test_tsan_host.py)
    compile: the probe's kernels are in it."""
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_scene_probe.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_scene_probe.hip"))
    assert "sources.sh" in open(os.path.join(ROOT, "tests", "tsan", "build_and_run.sh")).read()


def test_argument_errors_need_no_device(pkg):
    """NULL objs / element / Twc16s / q / rgb / depth, n_objs 0 and above 256, n_poses 0 and above 4096, n_q 0 and above 2^22, a pose index >= n_poses,
    a key >= 2^26, non-finite u, v and pose matrix, side not 0 / 1, a NULL manager: MON_ERR_ARG with a message and the outputs untouched, whether or
    not a device is present (no object exists, so nothing can reach one)."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (2, 1))
    q = pkg.scene_queries([0, 1, 0], [5, 6, (1 << 26) - 1], [1.5, 2.5, -3.0], [0.25, 7.0, 900.0]); n = q.shape[0]
    rgb = np.full((n, 3), 7.0, np.float32); dep = np.full(n, 7.0, np.float32); op = np.full(n, 7.0, np.float32); inst = np.full(n, 7, np.int32)
    hd = np.full(n, 7.0, np.float32); hi = np.full(n, 7, np.int32)

    def rc(objs=nulls, n_objs=1, side=0, poses=T, n_poses=None, qq=q, n_q=None, o_rgb=rgb, o_dep=dep):
        return L.mon_scene_probe(objs, n_objs, side, _p(poses), (0 if poses is None else poses.shape[0]) if n_poses is None else n_poses, _p(qq),
                                 (0 if qq is None else qq.shape[0]) if n_q is None else n_q, _p(o_rgb), _p(o_dep), _p(op), _p(inst), _p(hd), _p(hi))

    def edit(field, i, value):
        b = q.copy(); b[field][i] = value; return b
    Tbad = T.copy(); Tbad[1, 13] = np.inf
    Tnan = T.copy(); Tnan[0, 0] = np.nan
    rows = (dict(), dict(objs=None), dict(poses=None, n_poses=2), dict(qq=None, n_q=3), dict(o_rgb=None), dict(o_dep=None), dict(n_objs=0),
            dict(objs=many, n_objs=257), dict(n_poses=0), dict(n_poses=4097), dict(n_q=0), dict(n_q=(1 << 22) + 1), dict(side=2), dict(side=-1),
            dict(qq=edit("pose", 1, 2)), dict(qq=edit("key", 0, 1 << 26)), dict(qq=edit("key", 2, 0xffffffff)), dict(qq=edit("u", 0, np.nan)),
            dict(qq=edit("v", 2, np.inf)), dict(qq=edit("u", 1, -np.inf)), dict(poses=Tbad), dict(poses=Tnan))
    for kw in rows:                                                                         # (the first: a NULL element of objs)
        assert rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert rc(qq=edit("pose", 1, 2)) == MON_ERR_ARG and b"pose" in L.mon_last_error()
    assert rc(qq=edit("key", 0, 1 << 26)) == MON_ERR_ARG and b"key" in L.mon_last_error()
    assert rc(n_poses=4097) == MON_ERR_ARG and b"4096" in L.mon_last_error()
    # the online form: a NULL manager (the other rows need one: tests/test_scene_probe.py)
    assert L.mon_online_probe_scene(None, _p(T), 2, _p(q), n, _p(rgb), _p(dep), _p(op), _p(inst), _p(hd), _p(hi)) == MON_ERR_ARG
    # the diagnostic hooks judge the same arguments
    D = pkg.diag_lib(); r10 = np.full((n, 10), 7.0, np.float32)
    assert D.mon_debug_scene_probe_rays(nulls, 1, 0, _p(T), 2, _p(q), n, 0, _p(r10)) == MON_ERR_ARG
    assert D.mon_debug_scene_probe_rays(nulls, 1, 0, _p(T), 2, _p(q), n, 1, _p(r10)) == MON_ERR_ARG
    assert D.mon_debug_scene_probe_rays(nulls, 1, 0, _p(T), 2, _p(edit("pose", 0, 9)), n, 0, _p(r10)) == MON_ERR_ARG
    z = np.zeros((1, 1, 64), np.float32); c3 = np.zeros((1, 1, 64, 3), np.float32); cnt = np.zeros((1, 1), np.uint32); one = np.ones(1, np.float32)
    assert D.mon_debug_scene_probe_composite(0, 1, 1, _p(z), _p(z), _p(c3), _p(cnt), _p(one), _p(rgb), _p(dep), _p(op), _p(inst), None, _p(hi)) == MON_ERR_ARG
    assert D.mon_debug_scene_probe_composite(0, 0, 1, _p(z), _p(z), _p(c3), _p(cnt), _p(one), _p(rgb), _p(dep), _p(op), _p(inst), _p(hd), _p(hi)) == MON_ERR_ARG
    assert D.mon_debug_scene_probe_composite(0, 1, 257, _p(z), _p(z), _p(c3), _p(cnt), _p(one), _p(rgb), _p(dep), _p(op), _p(inst), _p(hd), _p(hi)) == MON_ERR_ARG
    for a in (rgb, dep, op, hd, r10):
        assert (a == 7.0).all()
    assert (inst == 7).all() and (hi == 7).all()
