"""CPU-side checks of the coarse-to-fine pose-refinement ABI (include/mon_core.h: mon_pose_c2f_params, mon_pose_c2f_default, mon_pose_c2f_weights,
mon_object_pose_loss_levels, mon_object_refine_pose_c2f, mon_online_refine_pose_c2f): the exports live in the product library only, the defaults are the
header's, the ctypes struct has the C layout, the weights are the window and schedule the header states, and bad arguments fail with MON_ERR_ARG before any
device is touched."""
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
CORE = ("mon_pose_c2f_default", "mon_pose_c2f_weights", "mon_object_pose_loss_levels", "mon_object_refine_pose_c2f", "mon_online_refine_pose_c2f")


def test_pose_c2f_exports(pkg):
    L = C.CDLL(pkg.lib_path())
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("no nm")
    diag_defined = set(subprocess.run([nm, "-D", "--defined-only", pkg.diag_lib_path()], capture_output=True, text=True, check=True).stdout.split())
    for s in CORE:
        assert hasattr(L, s) and s in pkg.exported_symbols(), s
        assert s not in pkg.diag_symbols() and s not in diag_defined, s                    # the product's, not the diagnostics library's
    for name in ("PoseC2FParams", "pose_c2f_default", "pose_c2f_weights"):
        assert hasattr(pkg, name), name
    assert callable(pkg.ObjectNeRF.pose_loss_levels) and callable(pkg.ObjectNeRF.refine_pose_c2f) and callable(pkg.OnlineManager.refine_pose_c2f)


def test_pose_c2f_defaults_match_the_header(pkg):
    c = pkg.pose_c2f_default()
    txt = open(os.path.join(ROOT, "include", "mon_core.h")).read()
    m = re.search(r"C2F defaults \(mon_pose_c2f_default[^:]*:(.*?)\.\s*\n", txt, flags=re.S)
    assert m, "the header records the defaults"
    stated = dict(re.findall(r"([a-z_]+) ([0-9.e+-]+)", " ".join(m.group(1).replace("*", " ").split())))
    assert set(stated) == {f for f, _ in pkg.PoseC2FParams._fields_}, stated
    for f, _ in pkg.PoseC2FParams._fields_:
        assert getattr(c, f) == pytest.approx(float(stated[f]), rel=1e-6), f
    assert 0 <= c.level_start <= c.level_end and 0 < c.ramp <= 1


def test_pose_c2f_params_layout_matches_c(pkg, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler")
    src = tmp_path / "layout.c"
    fields = [f for f, _ in pkg.PoseC2FParams._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mon_core.h"\nint main(void) {\n  printf("size %zu\\n", sizeof(mon_pose_c2f_params));\n'
                   + "".join('  printf("%s %%zu\\n", offsetof(mon_pose_c2f_params, %s));\n' % (f, f) for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(pkg.PoseC2FParams)
    for f in fields:
        assert int(got[f]) == getattr(pkg.PoseC2FParams, f).offset, f


def _weights_np(start, end, ramp, L, iters, step):
    """the window and schedule of include/mon_core.h, restated in float64"""
    alpha = start + (end - start) * min(1.0, step / (ramp * iters))
    a = alpha - np.arange(L, dtype=np.float64)
    return alpha, np.where(a <= 0, 0.0, np.where(a >= 1, 1.0, (1 - np.cos(np.pi * np.clip(a, 0, 1))) / 2))


GRID = [(s, e, r, L, it) for s in (0.0, 2.0, 3.5, 4.0) for e in (4.0, 8.0, 12.25, 16.0, 20.0) for r in (0.3, 0.6, 1.0) for L in (4, 8, 16)
        for it in (1, 7, 100) if e >= s]


@pytest.mark.parametrize("start,end,ramp,L,iters", GRID)
def test_pose_c2f_weights_match_numpy(pkg, start, end, ramp, L, iters):
    c = pkg.pose_c2f_default(level_start=start, level_end=end, ramp=ramp)
    prev = None
    for step in range(iters):
        w = pkg.pose_c2f_weights(L, iters, step, c)
        alpha, want = _weights_np(start, end, ramp, L, iters, step)
        assert w.dtype == np.float32 and w.shape == (L,)
        assert np.abs(w - want).max() <= 1e-6, (step, w, want)
        assert np.all((w >= 0) & (w <= 1)) and np.all(np.diff(w) <= 0), w                  # in [0, 1], non-increasing in the level
        if alpha == int(alpha):                                                            # integer alpha: exactly 0 / 1
            assert np.array_equal(w, (np.arange(L) < alpha).astype(np.float32)), (alpha, w)
        if alpha >= L:
            assert np.all(w == 1)
        if prev is not None:
            assert np.all(w >= prev), (step, prev, w)                                       # non-decreasing in the step
        prev = w
    if iters == 1 or ramp == 1.0:
        assert np.abs(pkg.pose_c2f_weights(L, iters, 0, c) - _weights_np(start, end, ramp, L, iters, 0)[1]).max() <= 1e-6


def test_pose_c2f_weights_edges(pkg):
    z = pkg.pose_c2f_weights(16, 10, 0, pkg.pose_c2f_default(level_start=0.0, level_end=8.0))
    assert np.array_equal(z, np.zeros(16, np.float32))                                     # alpha 0: nothing
    o = pkg.pose_c2f_weights(16, 10, 9, pkg.pose_c2f_default(level_start=16.0, level_end=16.0))
    assert np.array_equal(o, np.ones(16, np.float32))                                      # alpha >= L: everything
    h = pkg.pose_c2f_weights(4, 1, 0, pkg.pose_c2f_default(level_start=1.5, level_end=3.0, ramp=1.0))
    assert np.allclose(h, [1.0, 0.5, 0.0, 0.0], atol=1e-7)                                  # iters 1: alpha = level_start
    # the default schedule reaches level_end after ramp * iters steps and holds it
    d = pkg.pose_c2f_default(); it = 100; k = int(np.ceil(d.ramp * it))
    for step in (k, k + 1, it - 1):
        assert np.abs(pkg.pose_c2f_weights(16, it, step, d) - _weights_np(d.level_start, d.level_end, d.ramp, 16, it, k)[1]).max() <= 1e-6


def test_pose_c2f_bad_arguments_fail_before_the_device(pkg):
    L = pkg.lib()
    fake = np.zeros(64, np.uint64)                         # stands in for an object / manager: every check below comes before it is looked at
    obj = pp(fake)
    obs = np.array([[0, 0, 0, 4, 4]], np.uint32); pose = np.eye(4, dtype=np.float32).reshape(16); g = np.zeros(6, np.float32)
    trace = np.zeros(8, np.float32); loss = C.c_float(0); w = np.ones(16, np.float32)
    prm = pkg.pose_refine_default(); prm.iters = 2
    bad_iters = pkg.pose_refine_default(); bad_iters.iters = -1
    good = pkg.pose_c2f_default()
    bads = [pkg.pose_c2f_default(**kw) for kw in (dict(level_start=-0.5), dict(level_start=6.0, level_end=5.0), dict(ramp=0.0), dict(ramp=-0.2),
                                                   dict(ramp=1.01), dict(level_start=float("nan")), dict(level_end=float("inf")), dict(ramp=float("nan")))]
    P = C.byref
    # mon_pose_c2f_default / mon_pose_c2f_weights
    assert L.mon_pose_c2f_default(None) == MON_ERR_ARG
    assert L.mon_pose_c2f_weights(None, 16, 10, 0, pp(w)) == MON_ERR_ARG
    assert L.mon_pose_c2f_weights(P(good), 16, 10, 0, None) == MON_ERR_ARG
    for n_levels, iters, step in ((0, 10, 0), (16, 0, 0), (16, -3, 0), (16, 10, -1), (16, 10, 10), (16, 1, 1)):
        assert L.mon_pose_c2f_weights(P(good), n_levels, iters, step, pp(w)) == MON_ERR_ARG, (n_levels, iters, step)
    for b in bads:
        assert L.mon_pose_c2f_weights(P(b), 16, 10, 0, pp(w)) == MON_ERR_ARG
    assert L.mon_pose_c2f_weights(P(good), 16, 10, 0, pp(w)) == 0
    # mon_object_pose_loss_levels: the checks of mon_object_pose_loss, then NULL weights (negative / non-finite weights: tests/test_pose_c2f.py, they
    # need the object's level count)
    assert L.mon_object_pose_loss_levels(None, 0, pp(obs), 1, pp(pose), P(prm), 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss_levels(obj, 0, None, 1, pp(pose), P(prm), 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss_levels(obj, 0, pp(obs), 0, pp(pose), P(prm), 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss_levels(obj, 0, pp(obs), 1, None, P(prm), 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss_levels(obj, 0, pp(obs), 1, pp(pose), None, 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss_levels(obj, 0, pp(obs), 1, pp(pose), P(bad_iters), 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    assert L.mon_object_pose_loss_levels(obj, 0, pp(obs), 1, pp(pose), P(prm), 0, None, P(loss), pp(g)) == MON_ERR_ARG
    for side in (-1, 2):
        assert L.mon_object_pose_loss_levels(obj, side, pp(obs), 1, pp(pose), P(prm), 0, pp(w), P(loss), pp(g)) == MON_ERR_ARG
    # mon_object_refine_pose_c2f
    assert L.mon_object_refine_pose_c2f(None, 0, pp(obs), 1, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose_c2f(obj, 0, None, 1, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose_c2f(obj, 0, pp(obs), 0, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose_c2f(obj, 0, pp(obs), 1, None, P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose_c2f(obj, 0, pp(obs), 1, P(prm), None, pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose_c2f(obj, 0, pp(obs), 1, P(prm), P(good), None, pp(trace)) == MON_ERR_ARG
    assert L.mon_object_refine_pose_c2f(obj, 0, pp(obs), 1, P(bad_iters), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    for side in (-1, 2):
        assert L.mon_object_refine_pose_c2f(obj, side, pp(obs), 1, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    for b in bads:
        assert L.mon_object_refine_pose_c2f(obj, 0, pp(obs), 1, P(prm), P(b), pp(pose), pp(trace)) == MON_ERR_ARG
    # mon_online_refine_pose_c2f
    assert L.mon_online_refine_pose_c2f(None, 0, pp(obs), 1, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose_c2f(obj, 0, None, 1, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose_c2f(obj, 0, pp(obs), 0, P(prm), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose_c2f(obj, 0, pp(obs), 1, None, P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose_c2f(obj, 0, pp(obs), 1, P(prm), None, pp(pose), pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose_c2f(obj, 0, pp(obs), 1, P(prm), P(good), None, pp(trace)) == MON_ERR_ARG
    assert L.mon_online_refine_pose_c2f(obj, 0, pp(obs), 1, P(bad_iters), P(good), pp(pose), pp(trace)) == MON_ERR_ARG
    for b in bads:
        assert L.mon_online_refine_pose_c2f(obj, 0, pp(obs), 1, P(prm), P(b), pp(pose), pp(trace)) == MON_ERR_ARG
