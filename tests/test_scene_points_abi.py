"""CPU-side checks (no device needed) of the point-query boundary (include/mon_core.h): mon_object_query_points,
mon_scene_query_points, mon_scene_query_lattice, mon_lattice_points and the two online forms are declared, exported and bound with the header's
signatures; the diagnostic hook is exported by libmon_core_diag.so and not by the core; the new source is listed for every build; every argument error
that can be formed without a device-resident object is MON_ERR_ARG before any device work, with the outputs untouched; mon_lattice_points (host only)
against an exact restatement.  (The rows that need objects are in tests/test_scene_points.py.)"""
import ctypes as C
import os
from fractions import Fraction

import numpy as np

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p

NEW = ("mon_object_query_points", "mon_scene_query_points", "mon_scene_query_lattice", "mon_lattice_points", "mon_online_query_points",
       "mon_online_query_lattice")
DIAG = ("mon_debug_scene_point_rows",)
MON_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [5, 10, 13, 6, 8, 11]
    for name in ("query_object_points", "query_scene_points", "query_scene_lattice", "lattice_points", "scene_point_rows"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.query_points) and callable(pkg.OnlineManager.query_lattice)


def test_diag_hook_lives_in_the_diag_library(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path()); dl = pkg.diag_lib()
    for name in DIAG:
        assert name in pkg.diag_symbols() and name not in pkg.exported_symbols()
        assert hasattr(dl, name) and not hasattr(core, name), name
        assert [_kind(a) for a in _decl(name, "mon_core_diag.h")] == [_bound(t) for t in b._DIAG_SIGS[name][1]], name
    assert len(_decl("mon_debug_scene_point_rows", "mon_core_diag.h")) == 7


def test_new_source_is_listed_for_every_build():
    """sources.sh is what build.sh, the variant builds and the ThreadSanitizer host build compile: the point kernels are in it."""
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_scene_points.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_scene_points.hip"))
    assert "sources.sh" in open(os.path.join(ROOT, "tests", "tsan", "build_and_run.sh")).read()


def test_argument_errors_need_no_device(pkg):
    """NULL objs / element / points / sigma, n_objs 0 and above 256, n 0 and above 2^22, a lattice of more than 2^22 points, nx, ny or nz below 1,
    NULL origin or step, non-finite points, origin or step, side not 0 / 1, a NULL manager, a NULL object and a unit-cube point outside [0, 1]^3:
    MON_ERR_ARG with a message and the outputs untouched, whether or not a device is present (no object exists, so nothing can reach one).  The four
    optional outputs may be NULL: the call then still fails only on the NULL object."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    x = np.array([[0.1, 0.2, 0.3], [1.5, -2.0, 0.25], [0, 0, 0]], np.float32); n = x.shape[0]
    sig = np.full(64, 7.0, np.float32); rgb = np.full((64, 3), 7.0, np.float32); own = np.full(64, 7, np.int32); osg = np.full(64, 7.0, np.float32)
    nin = np.full(64, 7, np.uint32); raw = np.full((64, 4), 7.0, np.float32); r12 = np.full((64, 12), 7.0, np.float32)
    rest = (rgb, own, osg, nin)

    def pts(objs=nulls, n_objs=1, side=0, xyz=x, n_pts=None, o_sig=sig, o_rest=rest):
        return L.mon_scene_query_points(objs, n_objs, side, _p(xyz), (0 if xyz is None else xyz.shape[0]) if n_pts is None else n_pts, _p(o_sig),
                                        *[_p(a) for a in o_rest])

    def edit(a, i, j, v):
        b = a.copy(); b[i, j] = v; return b
    for kw in (dict(), dict(o_rest=(None,) * 4), dict(objs=None), dict(xyz=None, n_pts=3), dict(o_sig=None), dict(n_objs=0), dict(objs=many, n_objs=257),
               dict(n_pts=0), dict(n_pts=(1 << 22) + 1), dict(side=2), dict(side=-1), dict(xyz=edit(x, 0, 1, np.nan)), dict(xyz=edit(x, 2, 2, np.inf)),
               dict(xyz=edit(x, 1, 0, -np.inf))):                                            # (the first two: a NULL element of objs)
        assert pts(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert pts(xyz=edit(x, 0, 1, np.nan)) == MON_ERR_ARG and b"finite" in L.mon_last_error()
    assert pts(n_pts=0) == MON_ERR_ARG and b"points" in L.mon_last_error()
    assert pts() == MON_ERR_ARG and b"object" in L.mon_last_error()                          # accepted by the argument checks: fails on the NULL object alone

    o3 = np.array([0.5, -1.0, 2.0], np.float32); s3 = np.array([0.25, 0.0, -0.125], np.float32)

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), o_sig=sig, o_rest=rest):
        return L.mon_scene_query_lattice(objs, n_objs, side, _p(o), _p(s), *shape, _p(o_sig), *[_p(a) for a in o_rest])

    def ed1(a, i, v):
        b = a.copy(); b[i] = v; return b
    for kw in (dict(), dict(o_rest=(None,) * 4), dict(objs=None), dict(o=None), dict(s=None), dict(o_sig=None), dict(n_objs=0), dict(objs=many, n_objs=257),
               dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)), dict(shape=(2, 3, -7)),
               dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)), dict(shape=(1 << 30, 1 << 30, 1 << 30)), dict(side=2), dict(side=-1),
               dict(o=ed1(o3, 0, np.nan)), dict(o=ed1(o3, 2, np.inf)), dict(s=ed1(s3, 1, np.nan)), dict(s=ed1(s3, 0, -np.inf)),
               dict(s=ed1(s3, 0, 3e38), shape=(3, 1, 1))):                                   # (the last: a finite step that leaves the finite floats)
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert lat(shape=(1 << 11, 1 << 11, 2)) == MON_ERR_ARG and b"points" in L.mon_last_error()
    assert lat(shape=(1 << 11, 1 << 11, 1)) == MON_ERR_ARG and b"object" in L.mon_last_error()      # 2^22 points: accepted
    # shapes whose product wraps 64 bits (2^90, 2^64 and 2^66 - ..: 0 or small modulo 2^64) are judged by their size, not by the NULL object behind it
    for shape in ((1 << 30, 1 << 30, 1 << 30), (1 << 22, 1 << 21, 1 << 21), (2147483647, 2147483647, 2147483647), (1, 1 << 22, 2), (1 << 16, 1 << 16, 1 << 16)):
        assert lat(shape=shape) == MON_ERR_ARG and b"points" in L.mon_last_error(), shape
    # the object call: the points are judged in front of the object, so that the rule can be seen without one
    u = np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.75]], np.float32)
    assert L.mon_object_query_points(None, 0, _p(u), 3, _p(raw)) == MON_ERR_ARG and b"object" in L.mon_last_error()
    for bad in (edit(u, 2, 0, 1.0001), edit(u, 0, 1, -1e-6), edit(u, 1, 2, np.nan), edit(u, 1, 2, np.inf)):
        assert L.mon_object_query_points(None, 0, _p(bad), 3, _p(raw)) == MON_ERR_ARG and b"unit cube" in L.mon_last_error()
    for args in ((0, None, 3, _p(raw)), (0, _p(u), 3, None), (0, _p(u), 0, _p(raw)), (0, _p(u), (1 << 22) + 1, _p(raw)), (2, _p(u), 3, _p(raw))):
        assert L.mon_object_query_points(None, *args) == MON_ERR_ARG and L.mon_last_error(), args[0:3:2]
    # the online forms: a NULL manager (the other rows need one: tests/test_scene_points.py)
    assert L.mon_online_query_points(None, _p(x), n, _p(sig), *[_p(a) for a in rest]) == MON_ERR_ARG
    assert L.mon_online_query_lattice(None, _p(o3), _p(s3), 2, 3, 4, _p(sig), *[_p(a) for a in rest]) == MON_ERR_ARG
    # the diagnostic hook judges the same arguments
    D = pkg.diag_lib()
    assert D.mon_debug_scene_point_rows(nulls, 1, 0, _p(x), n, 0, _p(r12)) == MON_ERR_ARG
    assert D.mon_debug_scene_point_rows(nulls, 1, 0, _p(x), n, 1, _p(r12)) == MON_ERR_ARG
    assert D.mon_debug_scene_point_rows(nulls, 1, 0, _p(edit(x, 0, 0, np.nan)), n, 0, _p(r12)) == MON_ERR_ARG
    assert D.mon_debug_scene_point_rows(nulls, 1, 0, _p(x), n, 0, None) == MON_ERR_ARG
    for a in (sig, rgb, osg, raw, r12):
        assert (a == 7.0).all()
    assert (own == 7).all() and (nin == 7).all()


def _correctly_rounded(got, exact):
    """Is the fp32 value `got` the round-to-nearest-even fp32 of the rational `exact`?  Decided in rational arithmetic: no other fp32 is nearer, and on a
    tie the significand of `got` is even."""
    g = np.float32(got)
    if not np.isfinite(g):
        return False
    e = abs(exact - Fraction(float(g)))
    for nb in (np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))):
        e2 = abs(exact - Fraction(float(nb)))
        if e2 < e or (e2 == e and (int(g.view(np.uint32)) & 1)):
            return False
    return True


def test_lattice_points_are_the_correctly_rounded_fma(pkg):
    """mon_lattice_points at 1 x 1 x 1, 5 x 7 x 11 and 33 x 32 x 17 with steps of mixed sign and one zero step: point (i, j, k) sits at index
    (k ny + j) nx + i, and each coordinate is the correctly rounded fp32 of i * step + origin, the exact rational (an fmaf's result is exactly that; a
    separately rounded product is not, and the origins and steps here are chosen so that the two differ on most indices).  NULL pointers and bad shapes are
    MON_ERR_ARG, the output untouched."""
    L = pkg.lib()
    cases = (((1, 1, 1), (0.1, -2.3, 7.7), (0.013, -0.07, 0.0)), ((5, 7, 11), (0.1, -2.3, 7.7), (0.013, -0.07, 0.0)),
             ((33, 32, 17), (-1.2345678, 3.3333333, 0.7071068), (0.0371, 0.0, -0.2113)), ((33, 32, 17), (1e-3, -65.4321, 1024.77), (-3.1e-5, 1.9999999, 0.3)))
    n_double = 0
    for shape, origin, step in cases:
        o = np.array(origin, np.float32); s = np.array(step, np.float32); nx, ny, nz = shape
        xyz = pkg.lattice_points(o, s, shape)
        assert xyz.shape == (nx * ny * nz, 3) and xyz.dtype == np.float32
        g = xyz.reshape(nz, ny, nx, 3)
        for a, cnt in enumerate(shape):
            line = np.moveaxis(g[..., a], 2 - a, 0)                                          # [index along axis a][the two other axes]
            col = line.reshape(cnt, -1)
            assert (col.view(np.uint32) == col[:, :1].view(np.uint32)).all()                 # a coordinate depends on its own index alone
            for i in range(cnt):
                exact = Fraction(i) * Fraction(float(s[a])) + Fraction(float(o[a]))
                assert _correctly_rounded(col[i, 0], exact), (shape, a, i, col[i, 0])
                n_double += int(np.float32(np.float32(i) * s[a]) + o[a] != col[i, 0])
    assert n_double > 20, n_double                                                           # the check can tell an fma from a multiply and an add
    keep = np.full((6, 3), 7.0, np.float32); o = np.zeros(3, np.float32); s = np.ones(3, np.float32)
    for shape in ((1 << 30, 1 << 30, 1 << 30), (1 << 22, 1 << 21, 1 << 21), (1 << 11, 1 << 11, 2)):                      # (the first two wrap a 64-bit product)
        assert L.mon_lattice_points(_p(o), _p(s), *shape, _p(keep)) == MON_ERR_ARG and b"points" in L.mon_last_error(), shape
    for args in ((None, _p(s), 1, 2, 3, _p(keep)), (_p(o), None, 1, 2, 3, _p(keep)), (_p(o), _p(s), 1, 2, 3, None), (_p(o), _p(s), 0, 2, 3, _p(keep)),
                 (_p(o), _p(s), 1, -2, 3, _p(keep)), (_p(o), _p(s), 1 << 12, 1 << 12, 1, _p(keep)),
                 (_p(np.array([0, np.nan, 0], np.float32)), _p(s), 1, 2, 3, _p(keep)), (_p(o), _p(np.array([0, 0, np.inf], np.float32)), 1, 2, 3, _p(keep))):
        assert L.mon_lattice_points(*args) == MON_ERR_ARG and L.mon_last_error(), args[2:5]
    assert (keep == 7.0).all()
