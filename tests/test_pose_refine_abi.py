"""CPU-side checks of the pose-refinement ABI (include/mon_core.h: mon_pose_refine_params, mon_pose_refine_default, mon_object_pose_loss,
mon_object_refine_pose, mon_online_refine_pose; include/mon_core_diag.h: mon_debug_pose_samples): the exports live in the right libraries, the defaults
are the header's, the ctypes struct has the C layout, and bad arguments fail with MON_ERR_ARG before any device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import p as pp

MON_ERR_ARG = 1
CORE = ("mon_pose_refine_default", "mon_object_pose_loss", "mon_object_refine_pose", "mon_online_refine_pose")


def test_pose_refine_exports(pkg):
    L = C.CDLL(pkg.lib_path())
    for s in CORE:
        assert hasattr(L, s) and s in pkg.exported_symbols(), s
    s = "mon_debug_pose_samples"
    assert s in pkg.diag_symbols() and hasattr(pkg.diag_lib(), s) and not hasattr(L, s)
    for name in ("PoseRefineParams", "pose_refine_default"):
        assert hasattr(pkg, name), name
    assert callable(pkg.ObjectNeRF.pose_loss) and callable(pkg.ObjectNeRF.refine_pose) and callable(pkg.OnlineManager.refine_pose)


def test_pose_refine_defaults_match_the_header(pkg):
    p = pkg.pose_refine_default()
    txt = open(os.path.join(ROOT, "include", "mon_core.h")).read()
    m = re.search(r"Defaults \(mon_pose_refine_default[^:]*:(.*?)\.\s*\n", txt, flags=re.S)
    assert m, "the header records the defaults"
    stated = dict(re.findall(r"([a-z_]+) ([0-9.e+-]+)", " ".join(m.group(1).replace("*", " ").split())))
    assert set(stated) == {f for f, _ in pkg.PoseRefineParams._fields_}, stated
    for f, _ in pkg.PoseRefineParams._fields_:
        assert getattr(p, f) == pytest.approx(float(stated[f]), rel=1e-6), f
    assert p.iters >= 0 and p.lr_trans > 0 and p.lr_rot > 0


def test_pose_refine_params_layout_matches_c(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "layout.c"
    fields = [f for f, _ in pkg.PoseRefineParams._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mon_core.h"\nint main(void) {\n  printf("size %zu\\n", sizeof(mon_pose_refine_params));\n'
                   + "".join('  printf("%s %%zu\\n", offsetof(mon_pose_refine_params, %s));\n' % (f, f) for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(pkg.PoseRefineParams)
    for f in fields:
        assert int(got[f]) == getattr(pkg.PoseRefineParams, f).offset, f


def test_pose_refine_bad_arguments_fail_before_the_device(pkg):
    L = pkg.lib(); D = pkg.diag_lib()
    fake = np.zeros(64, np.uint64)                         # stands in for an object: every check below comes before it is looked at
    obj = pp(fake)
    obs = np.array([[0, 0, 0, 4, 4]], np.uint32); pose = np.eye(4, dtype=np.float32).reshape(16); g = np.zeros(6, np.float32)
    trace = np.zeros(8, np.float32); loss = C.c_float(0)
    prm = pkg.pose_refine_default(); prm.iters = 2
    bad_iters = pkg.pose_refine_default(); bad_iters.iters = -1
    P = C.byref
    # mon_object_pose_loss
    assert L.mon_object_pose_loss(None, 0, pp(obs), 1, pp(pose), P(prm), 0, P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss(obj, 0, None, 1, pp(pose), P(prm), 0, P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss(obj, 0, pp(obs), 0, pp(pose), P(prm), 0, P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss(obj, 0, pp(obs), 1, None, P(prm), 0, P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss(obj, 0, pp(obs), 1, pp(pose), None, 0, P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss(obj, 0, pp(obs), 1, pp(pose), P(bad_iters), 0, P(loss), pp(g)) == MON_ERR_ARG
    for side in (-1, 2):
        assert L.mon_object_pose_loss(obj, side, pp(obs), 1, pp(pose), P(prm), 0, P(loss), pp(g)) == MON_ERR_ARG
    # mon_object_refine_pose
    assert L.mon_object_refine_pose(None, 0, pp(obs), 1, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose(obj, 0, None, 1, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose(obj, 0, pp(obs), 0, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose(obj, 0, pp(obs), 1, None, pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose(obj, 0, pp(obs), 1, P(prm), None, pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose(obj, 0, pp(obs), 1, P(bad_iters), pp(pose), pp(trace)) == MON_ERR_ARG
    for side in (-1, 2):
        assert L.mon_object_refine_pose(obj, side, pp(obs), 1, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    # mon_online_refine_pose: null manager / arguments
    assert L.mon_online_refine_pose(None, 0, pp(obs), 1, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose(obj, 0, None, 1, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose(obj, 0, pp(obs), 0, P(prm), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose(obj, 0, pp(obs), 1, None, pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose(obj, 0, pp(obs), 1, P(prm), None, pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose(obj, 0, pp(obs), 1, P(bad_iters), pp(pose), pp(trace)) == MON_ERR_ARG
    # the diagnostic
    assert D.mon_debug_pose_samples(None, 0, pp(obs), 1, pp(pose), P(prm), 0, None, None, None) == MON_ERR_ARG
    assert D.mon_debug_pose_samples(obj, 0, None, 1, pp(pose), P(prm), 0, None, None, None) == MON_ERR_ARG
    assert D.mon_debug_pose_samples(obj, 0, pp(obs), 0, pp(pose), P(prm), 0, None, None, None) == MON_ERR_ARG
    assert D.mon_debug_pose_samples(obj, 0, pp(obs), 1, None, P(prm), 0, None, None, None) == MON_ERR_ARG
    assert D.mon_debug_pose_samples(obj, 0, pp(obs), 1, pp(pose), None, 0, None, None, None) == MON_ERR_ARG
    assert L.mon_pose_refine_default(None) == MON_ERR_ARG
