"""CPU-side checks of the scene-render ABI (include/mon_core.h: mon_scene_render, mon_online_render_scene; include/mon_core_diag.h:
mon_debug_scene_samples, mon_debug_scene_composite): the exports exist and null or empty arguments fail with MON_ERR_ARG before any device is touched."""
import ctypes as C

import numpy as np

from abi_decl import p as pp

MON_ERR_ARG = 1


def test_scene_render_exports(pkg):
    L = C.CDLL(pkg.lib_path())
    for s in ("mon_scene_render", "mon_online_render_scene"):
        assert hasattr(L, s) and s in pkg.exported_symbols(), s
    for s in ("mon_debug_scene_samples", "mon_debug_scene_composite"):
        assert s in pkg.diag_symbols() and hasattr(pkg.diag_lib(), s) and not hasattr(L, s), s
    assert callable(pkg.render_scene) and callable(pkg.OnlineManager.render_scene)


def test_scene_render_null_and_empty_arguments(pkg):
    L = pkg.lib(); D = pkg.diag_lib()
    pose = np.eye(4, dtype=np.float32).reshape(16); out = np.zeros(64, np.float32); inst = np.zeros(16, np.int32)
    box = pkg.MonBBox(0, 0, 0, 4, 4); empty = pkg.MonBBox(0, 0, 0, 0, 4)
    one_null = (C.c_void_p * 1)(None)
    # no object list, an empty one, a null object, empty rect, null pose / outputs
    assert L.mon_scene_render(None, 1, 0, box, pp(pose), pp(out), pp(out), None, None) == MON_ERR_ARG
    assert L.mon_scene_render(one_null, 0, 0, box, pp(pose), pp(out), pp(out), None, None) == MON_ERR_ARG
    assert L.mon_scene_render(one_null, 1, 0, box, pp(pose), pp(out), pp(out), pp(out), pp(inst)) == MON_ERR_ARG
    assert L.mon_scene_render(one_null, 1, 1, empty, pp(pose), pp(out), pp(out), None, None) == MON_ERR_ARG
    assert L.mon_scene_render(one_null, 1, 0, box, None, pp(out), pp(out), None, None) == MON_ERR_ARG
    assert L.mon_scene_render(one_null, 1, 0, box, pp(pose), None, pp(out), None, None) == MON_ERR_ARG
    assert L.mon_scene_render(one_null, 1, 0, box, pp(pose), pp(out), None, None, None) == MON_ERR_ARG
    assert L.mon_online_render_scene(None, box, pp(pose), pp(out), pp(out), None, None) == MON_ERR_ARG
    # diagnostics
    assert D.mon_debug_scene_samples(None, 1, 0, box, pp(pose), 0, None, None, None, None) == MON_ERR_ARG
    assert D.mon_debug_scene_samples(one_null, 1, 0, box, pp(pose), 1, None, None, None, None) == MON_ERR_ARG
    t = np.zeros(64, np.float32); rgb = np.zeros(192, np.float32); cnt = np.zeros(1, np.uint32); dn = np.ones(1, np.float32)
    o3 = np.zeros(3, np.float32); o1 = np.zeros(1, np.float32); oi = np.zeros(1, np.int32)
    args = (pp(t), pp(t), pp(rgb), pp(cnt), pp(dn), pp(o3), pp(o1), pp(o1), pp(oi))
    assert D.mon_debug_scene_composite(0, 1, 0, *args) == MON_ERR_ARG
    assert D.mon_debug_scene_composite(0, 0, 1, *args) == MON_ERR_ARG
    assert D.mon_debug_scene_composite(0, 1, 257, *args) == MON_ERR_ARG
    assert D.mon_debug_scene_composite(0, 1, 1, None, *args[1:]) == MON_ERR_ARG
    cnt[0] = 65
    assert D.mon_debug_scene_composite(0, 1, 1, *args) == MON_ERR_ARG
