"""CPU-side checks (no device needed) of the ray-cast boundary (include/mon_core.h): mon_scene_cast, mon_online_cast_rays and
mon_camera_rays are declared, exported and bound with the header's signatures; mon_scene_ray is 32 bytes with the fields o, t_max, d, key; the two
diagnostic hooks are exported by libmon_core_diag.so and not by the core; the new source is listed for every build; every argument error that can be
formed without a device-resident object is MON_ERR_ARG before any device work, with the outputs untouched; mon_camera_rays (host only) against an
fp64 restatement.  (The rows that need objects are in tests/test_scene_cast.py.)"""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p

NEW = ("mon_scene_cast", "mon_online_cast_rays", "mon_camera_rays")
DIAG = ("mon_debug_scene_cast_rays", "mon_debug_scene_cast_composite")
MON_ERR_ARG = 1
U = 2.0 ** -24               # unit roundoff of fp32


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert len(_decl("mon_scene_cast")) == 13 and len(_decl("mon_online_cast_rays")) == 11 and len(_decl("mon_camera_rays")) == 10
    for name in ("cast_scene", "scene_rays", "camera_rays", "scene_cast_rays", "scene_cast_composite"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.cast_rays)


def test_ray_struct_layout(pkg):
    R = pkg.SceneRay
    assert C.sizeof(R) == 32
    assert [f for f, _ in R._fields_] == ["o", "t_max", "d", "key"]
    assert [R.o.offset, R.t_max.offset, R.d.offset, R.key.offset] == [0, 12, 16, 28]
    dt = pkg.SCENE_RAY_DTYPE
    assert dt.itemsize == 32 and dt.names == ("o", "t_max", "d", "key") and [dt.fields[n][1] for n in dt.names] == [0, 12, 16, 28]
    txt = open(os.path.join(ROOT, "include", "mon_core.h")).read()
    m = re.search(r"typedef struct mon_scene_ray \{(.*?)\} mon_scene_ray;", txt, flags=re.S)
    assert m
    assert re.findall(r"(\w+)\s+([\w\[\]]+);", m.group(1)) == [("float", "o[3]"), ("float", "t_max"), ("float", "d[3]"), ("uint32_t", "key")]
    r = pkg.scene_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [1, 0, 0]], t_max=[2.5, np.inf], key=[7, 9])
    assert r["o"].tolist() == [[1, 2, 3], [4, 5, 6]] and r["d"].tolist() == [[0, 0, 1], [1, 0, 0]] and r["key"].tolist() == [7, 9]
    assert r["t_max"][0] == 2.5 and np.isinf(r["t_max"][1])


def test_diag_hooks_live_in_the_diag_library(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path()); dl = pkg.diag_lib()
    for name in DIAG:
        assert name in pkg.diag_symbols() and name not in pkg.exported_symbols()
        assert hasattr(dl, name) and not hasattr(core, name), name
        assert [_kind(a) for a in _decl(name, "mon_core_diag.h")] == [_bound(t) for t in b._DIAG_SIGS[name][1]], name


def test_new_source_is_listed_for_every_build():
    """sources.sh is what build.sh, the variant builds and the ThreadSanitizer host build compile: the cast's kernels are in it."""
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_scene_cast.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_scene_cast.hip"))
    assert "sources.sh" in open(os.path.join(ROOT, "tests", "tsan", "build_and_run.sh")).read()


def _good_rays(pkg):
    d = np.array([[0, 0, 1], [0.6, 0, 0.8], [-1, 0, 0]], np.float32)
    return pkg.scene_rays([[0, 0, -3], [1, 2, 3], [5, 0, 0]], d, t_max=[np.inf, 2.0, 7.5], key=[5, 6, (1 << 26) - 1])


def test_argument_errors_need_no_device(pkg):
    """NULL objs / element / rays / rgb / dist, n_objs 0 and above 256, n_rays 0 and above 2^22, a key >= 2^26, a non-finite o or d, a non-unit d
    (|d|^2 off by more than 1e-3 either way, and the zero vector), t_max 0, negative and NaN, hit_opacity 0, negative, above 0.999 and NaN, side not
    0 / 1, a NULL manager: MON_ERR_ARG with a message and the outputs untouched, whether or not a device is present (no object exists, so nothing can
    reach one).  The other five outputs may be NULL: the call then still fails only on the NULL object."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    r = _good_rays(pkg); n = r.shape[0]
    rgb = np.full((n, 3), 7.0, np.float32); dist = np.full(n, 7.0, np.float32); op = np.full(n, 7.0, np.float32); inst = np.full(n, 7, np.int32)
    ht = np.full(n, 7.0, np.float32); hs = np.full(n, 7.0, np.float32); hi = np.full(n, 7, np.int32)

    def rc(objs=nulls, n_objs=1, side=0, rays=r, n_rays=None, thr=0.5, o_rgb=rgb, o_dist=dist, rest=(op, inst, ht, hs, hi)):
        return L.mon_scene_cast(objs, n_objs, side, _p(rays), (0 if rays is None else rays.shape[0]) if n_rays is None else n_rays, C.c_float(thr),
                                _p(o_rgb), _p(o_dist), *[_p(a) for a in rest])

    def edit(field, i, value):
        b = r.copy(); b[field][i] = value; return b
    rows = (dict(), dict(rest=(None,) * 5), dict(objs=None), dict(rays=None, n_rays=3), dict(o_rgb=None), dict(o_dist=None), dict(n_objs=0),
            dict(objs=many, n_objs=257), dict(n_rays=0), dict(n_rays=(1 << 22) + 1), dict(side=2), dict(side=-1),
            dict(rays=edit("key", 0, 1 << 26)), dict(rays=edit("key", 2, 0xffffffff)),
            dict(rays=edit("o", 0, [np.nan, 0, 0])), dict(rays=edit("o", 2, [0, np.inf, 0])), dict(rays=edit("d", 1, [0.6, np.nan, 0.8])),
            dict(rays=edit("d", 0, [0, 0, -np.inf])),
            dict(rays=edit("d", 0, [0, 0, 1.001])), dict(rays=edit("d", 1, [0.6, 0, 0.799])), dict(rays=edit("d", 2, [0, 0, 0])),
            dict(rays=edit("t_max", 1, 0.0)), dict(rays=edit("t_max", 0, -1.0)), dict(rays=edit("t_max", 2, np.nan)), dict(rays=edit("t_max", 2, -np.inf)),
            dict(thr=0.0), dict(thr=-0.5), dict(thr=0.9995), dict(thr=1.0), dict(thr=np.nan), dict(thr=np.inf))
    for kw in rows:                                                                         # (the first two: a NULL element of objs)
        assert rc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    assert rc(rays=edit("key", 0, 1 << 26)) == MON_ERR_ARG and b"key" in L.mon_last_error()
    assert rc(rays=edit("d", 0, [0, 0, 1.001])) == MON_ERR_ARG and b"unit" in L.mon_last_error()
    assert rc(rays=edit("t_max", 1, 0.0)) == MON_ERR_ARG and b"t_max" in L.mon_last_error()
    assert rc(thr=1.0) == MON_ERR_ARG and b"hit_opacity" in L.mon_last_error()
    # accepted by the argument checks (the call then fails on the NULL object alone): |d|^2 within 1e-3 of 1, the largest threshold, +inf t_max
    assert rc(rays=edit("d", 0, [0, 0, 1.0004]), thr=0.999) == MON_ERR_ARG and b"object" in L.mon_last_error()
    # the online form: a NULL manager (the other rows need one: tests/test_scene_cast.py)
    assert L.mon_online_cast_rays(None, _p(r), n, C.c_float(0.5), _p(rgb), _p(dist), _p(op), _p(inst), _p(ht), _p(hs), _p(hi)) == MON_ERR_ARG
    # the diagnostic hooks judge the same arguments
    D = pkg.diag_lib(); r10 = np.full((n, 10), 7.0, np.float32); en = np.full(n, 7.0, np.float32)
    assert D.mon_debug_scene_cast_rays(nulls, 1, 0, _p(r), n, 0, _p(r10), _p(en)) == MON_ERR_ARG
    assert D.mon_debug_scene_cast_rays(nulls, 1, 0, _p(r), n, 1, _p(r10), _p(en)) == MON_ERR_ARG
    assert D.mon_debug_scene_cast_rays(nulls, 1, 0, _p(edit("t_max", 0, 0.0)), n, 0, _p(r10), _p(en)) == MON_ERR_ARG
    assert D.mon_debug_scene_cast_rays(nulls, 1, 0, _p(r), n, 0, _p(r10), None) == MON_ERR_ARG
    z = np.zeros((1, 1, 64), np.float32); c3 = np.zeros((1, 1, 64, 3), np.float32); cnt = np.zeros((1, 1), np.uint32); one = np.ones(1, np.float32)

    def comp(n_rays=1, n_lists=1, thr=0.5, o_ht=ht, entry=one):
        return D.mon_debug_scene_cast_composite(0, n_rays, n_lists, _p(z), _p(z), _p(c3), _p(cnt), _p(entry), C.c_float(thr), _p(rgb), _p(dist), _p(op), _p(inst),
                                                _p(o_ht), _p(hs), _p(hi))
    for kw in (dict(o_ht=None), dict(entry=None), dict(n_rays=0), dict(n_lists=257), dict(thr=0.0), dict(thr=1.0)):
        assert comp(**kw) == MON_ERR_ARG, kw
    for a in (rgb, dist, op, ht, hs, r10, en):
        assert (a == 7.0).all()
    assert (inst == 7).all() and (hi == 7).all()


def ref_camera_rays(K, Twc, u, v):
    """fp64 restatement of pixel_ray's world-frame branch on the fp32 inputs, with the forward error bounds of its fp32 evaluation, counted the way
    tests/test_scene_probe.py's ref_rays counts them (each rounding at most U = 2^-24 relative to its result, first order):
      dn = |camera ray|   sub, div, mul, fma, fma, sqrt                                              ->  6 U dn
      d  = Rwc dc / dn    the six above, the division by dn, one rot3 of (mul, fma, fma): 10 roundings; squaring doubles the error of dc, so 11 U Md,
                          Md = |Rwc| |dc / dn| (the magnitude of the terms summed)
      o  = twc            copied: exact."""
    fx, fy, cx, cy = (np.float64(np.float32(x)) for x in K)
    Twc = np.asarray(Twc, np.float32).astype(np.float64).reshape(4, 4).T
    u = np.asarray(u, np.float32).astype(np.float64); v = np.asarray(v, np.float32).astype(np.float64)
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    dn = np.sqrt((dc * dc).sum(-1)); dcn = dc / dn[:, None]
    return Twc[:3, 3], dcn @ Twc[:3, :3].T, dn, 11 * U * (np.abs(dcn) @ np.abs(Twc[:3, :3]).T), 6 * U * dn


def test_camera_rays_against_fp64(pkg, ss):
    """mon_camera_rays under three poses at 2 000 sub-pixel points inside and outside a 320 x 240 image: o is the pose's translation bit for bit,
    t_max = +inf, the keys are the queries', d and dn lie within ref_camera_rays' bounds (11 U Md and 6 U dn) and d passes mon_scene_cast's unit test.
    dn_out may be NULL.  A pose index >= n_poses, NULL pointers, empty lists and non-finite inputs are MON_ERR_ARG, outputs untouched."""
    rng = np.random.RandomState(3); N = 2000
    K = (260.0, 255.5, 159.5, 119.25)
    poses = np.stack([ss.colmajor(ss._look_at(rng.uniform(-3, 3, 3), rng.uniform(-0.5, 0.5, 3))) for _ in range(3)]).astype(np.float32)
    u = rng.uniform(-60.0, 380.0, N).astype(np.float32); v = rng.uniform(-45.0, 285.0, N).astype(np.float32)
    q = pkg.scene_queries(rng.randint(0, 3, N), rng.randint(0, 1 << 26, N), u, v)
    rays, dn = pkg.camera_rays(K, poses, q)
    assert np.array_equal(rays["key"], q["key"]) and np.isinf(rays["t_max"]).all() and (rays["t_max"] > 0).all()
    worst = [0.0, 0.0]
    for p in range(3):
        m = q["pose"] == p
        o, d, n, Ed, Edn = ref_camera_rays(K, poses[p], u[m], v[m])
        assert np.array_equal(rays["o"][m].view(np.uint32), np.broadcast_to(poses[p, 12:15], (int(m.sum()), 3)).view(np.uint32))
        ed = np.abs(rays["d"][m].astype(np.float64) - d) / Ed; en = np.abs(dn[m].astype(np.float64) - n) / Edn
        worst = [max(worst[0], float(ed.max())), max(worst[1], float(en.max()))]
        assert (ed <= 1.0).all() and (en <= 1.0).all()
    print("camera rays: largest error / bound  d %.3f  dn %.3f" % tuple(worst))
    nn = (rays["d"].astype(np.float32) ** 2).sum(-1)
    assert (np.abs(nn - 1.0) < 1e-5).all()
    L = pkg.lib(); P = _p(poses)
    out = np.zeros(N, pkg.SCENE_RAY_DTYPE)
    assert L.mon_camera_rays(*[C.c_float(x) for x in K], P, 3, _p(q), N, _p(out), None) == 0
    assert np.array_equal(out.view(np.uint32), rays.view(np.uint32))
    out[:] = 0; keep = out.copy(); dn7 = np.full(N, 7.0, np.float32)
    bad = q.copy(); bad["pose"][N - 1] = 3
    nanq = q.copy(); nanq["u"][5] = np.nan
    badpose = poses.copy(); badpose[2, 3] = np.inf
    Kc = [C.c_float(x) for x in K]
    for args in ((Kc, P, 3, _p(bad), N, _p(out)), (Kc, P, 2, _p(q), N, _p(out)), (Kc, None, 3, _p(q), N, _p(out)), (Kc, P, 3, None, N, _p(out)),
                 (Kc, P, 3, _p(q), N, None), (Kc, P, 0, _p(q), N, _p(out)), (Kc, P, 3, _p(q), 0, _p(out)), (Kc, P, 3, _p(nanq), N, _p(out)),
                 (Kc, _p(badpose), 3, _p(q), N, _p(out)), ([C.c_float(0.0)] + Kc[1:], P, 3, _p(q), N, _p(out)),
                 (Kc[:2] + [C.c_float(np.nan)] + Kc[3:], P, 3, _p(q), N, _p(out))):
        kc, rest = args[0], args[1:]
        assert L.mon_camera_rays(*kc, *rest, _p(dn7)) == MON_ERR_ARG and L.mon_last_error(), rest[1:4]
    assert np.array_equal(out.view(np.uint32), keep.view(np.uint32)) and (dn7 == 7.0).all()
