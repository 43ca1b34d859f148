"""CPU-side checks (no device needed) of the distance-field boundary (include/mon_core.h): mon_distance_transform,
mon_scene_distance_lattice and mon_online_distance_lattice are declared, exported and bound with the header's signatures; the new source is listed for
every build; every argument error is MON_ERR_ARG before any device work, with a message and the outputs untouched; and the numpy reference the GPU tests
compare with (tests/distance_reference.py) is pinned on its own: its separable form against its brute force over all pairs.  (The rows that need a
device are in tests/test_scene_distance.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p
import distance_reference as dr

NEW = ("mon_distance_transform", "mon_scene_distance_lattice", "mon_online_distance_lattice")
MON_ERR_ARG = 1


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [9, 15, 13]
    assert [_kind(a) for a in _decl("mon_distance_transform")] == ["int", "ptr", "int", "int", "int", "ptr", "float", "ptr", "ptr"]
    assert [_kind(a) for a in _decl("mon_scene_distance_lattice")] == ["ptr", "u64", "int", "ptr", "ptr", "int", "int", "int", "float", "float"] + ["ptr"] * 5
    assert _decl("mon_online_distance_lattice")[1:] == _decl("mon_scene_distance_lattice")[3:]      # "the same from origin3 on"
    for name in ("distance_transform", "scene_distance_lattice"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.distance_lattice)


def test_new_source_is_listed_for_every_build():
    """sources.sh is what build.sh, the variant builds and the ThreadSanitizer host build compile: the distance kernels are in it."""
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_distance.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_distance.hip"))
    assert "sources.sh" in open(os.path.join(ROOT, "ro-map_amd", "build.sh")).read()


def test_argument_errors_need_no_device(pkg):
    """NULL occupied / step / origin / dist / objs / element / manager; a dimension below 1; nx * ny * nz above 2^22 (shapes whose product wraps 64 bits
    included); a non-finite step or origin; sigma_min negative, NaN or infinite; max_dist 0, negative or NaN; side not 0 / 1; n_objs 0 and above 256:
    MON_ERR_ARG with a message and every output untouched, whether or not a device is present (the checks come before the device is looked for, and no
    object exists).  The optional outputs may be NULL and max_dist may be +inf: the scene call then fails on the NULL object alone."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    occ = np.ones(24, np.uint8); s3 = np.array([0.25, 0.0, -0.125], np.float32); o3 = np.array([0.5, -1.0, 2.0], np.float32)
    dist = np.full(64, 7.0, np.float32); near = np.full(64, 7, np.int32); nown = np.full(64, 7, np.int32); free = np.full(64, 7.0, np.float32)
    sig = np.full(64, 7.0, np.float32)

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def dt(m=occ, shape=(2, 3, 4), s=s3, md=1.0, d=dist, nr=near, device=0):
        return L.mon_distance_transform(device, _p(m), *shape, _p(s), md, _p(d), _p(nr))

    wrap = ((1 << 30, 1 << 30, 1 << 30), (1 << 22, 1 << 21, 1 << 21), (2147483647, 2147483647, 2147483647), (1, 1 << 22, 2), (1 << 16, 1 << 16, 1 << 16))
    for kw in (dict(m=None), dict(s=None), dict(d=None), dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)),
               dict(shape=(2, 3, -7)), dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)), dict(s=ed(s3, 0, np.nan)),
               dict(s=ed(s3, 1, np.inf)), dict(s=ed(s3, 2, -np.inf)), dict(md=0.0), dict(md=-1.0), dict(md=float("nan")), dict(md=-np.inf),
               dict(d=None, nr=None)) + tuple(dict(shape=w) for w in wrap):
        assert dt(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    for w in wrap + ((1 << 11, 1 << 11, 2),):
        assert dt(shape=w) == MON_ERR_ARG and b"points" in L.mon_last_error(), w
    assert dt(s=ed(s3, 0, np.nan)) == MON_ERR_ARG and b"finite" in L.mon_last_error()
    assert dt(md=0.0) == MON_ERR_ARG and b"max_dist" in L.mon_last_error()
    assert dt(d=None) == MON_ERR_ARG and b"dist" in L.mon_last_error()

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), smin=1.0, md=1.0, d=dist, rest=(near, nown, free, sig)):
        return L.mon_scene_distance_lattice(objs, n_objs, side, _p(o), _p(s), *shape, smin, md, _p(d), *[_p(a) for a in rest])

    def onl(o=o3, s=s3, shape=(2, 3, 4), smin=1.0, md=1.0, d=dist, rest=(near, nown, free, sig)):
        return L.mon_online_distance_lattice(None, _p(o), _p(s), *shape, smin, md, _p(d), *[_p(a) for a in rest])

    for kw in (dict(), dict(rest=(None,) * 4), dict(md=np.inf), dict(smin=0.0), dict(objs=None), dict(o=None), dict(s=None), dict(d=None), dict(n_objs=0),
               dict(objs=many, n_objs=257), dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)),
               dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)), dict(side=2), dict(side=-1), dict(o=ed(o3, 0, np.nan)),
               dict(o=ed(o3, 2, np.inf)), dict(s=ed(s3, 1, np.nan)), dict(s=ed(s3, 0, -np.inf)), dict(smin=-1e-6), dict(smin=float("nan")),
               dict(smin=np.inf), dict(md=0.0), dict(md=-2.0), dict(md=float("nan"))) + tuple(dict(shape=w) for w in wrap):
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw               # (the first four: a NULL element of objs)
    for kw in (dict(), dict(rest=(None,) * 4), dict(md=np.inf), dict(smin=0.0)):
        assert lat(**kw) == MON_ERR_ARG and b"object" in L.mon_last_error(), kw  # accepted by the argument checks: fails on the NULL object alone
    assert lat(shape=(1 << 11, 1 << 11, 1)) == MON_ERR_ARG and b"object" in L.mon_last_error()      # 2^22 cells: accepted
    assert lat(smin=-1e-6) == MON_ERR_ARG and b"sigma_min" in L.mon_last_error()
    assert lat(md=float("nan")) == MON_ERR_ARG and b"max_dist" in L.mon_last_error()
    assert lat(side=2) == MON_ERR_ARG and b"side" in L.mon_last_error()
    assert lat(objs=many, n_objs=257) == MON_ERR_ARG and b"objects" in L.mon_last_error()
    for kw in (dict(), dict(md=0.0), dict(smin=-1.0), dict(shape=(0, 1, 1)), dict(d=None)):
        assert onl(**kw) == MON_ERR_ARG, kw                                        # a NULL manager, with good and with bad arguments
    assert (dist == 7.0).all() and (free == 7.0).all() and (sig == 7.0).all() and (near == 7).all() and (nown == 7).all()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
SHAPES = ((1, 1, 1), (11, 1, 1), (1, 9, 1), (1, 1, 7), (5, 4, 3), (11, 9, 7))
STEPS = ((0.1, 0.1, 0.1), (0.013, 0.0217, 0.0091), (0.1, -0.2, 0.3), (0.25, 0.25, 0.25), (0.5, 2.0, 0.125), (0.05, 0.0, 0.05))
DENSITIES = (0, "one", 0.03, 0.3, 0.9)


@pytest.mark.parametrize("step", STEPS)
def test_reference_separable_equals_brute_force(step):
    """On lattices of at most 11 x 9 x 7, at densities 0, one cell, 3 %, 30 % and 90 %, with isotropic, anisotropic, negative, power-of-two and zero
    steps: the separable d2 equals the brute force over all pairs bit for bit; the separable site equals the brute force's (the lowest flat index among
    the nearest) wherever the brute force has no tie, and wherever it has one it names an occupied cell at the minimal d2 (recomputed for that pair by the
    nested expression)."""
    f = np.float32
    n_tie = n_cells = 0
    for shape in SHAPES:
        nx, ny, nz = shape
        for di, dens in enumerate(DENSITIES):
            m = dr.random_mask(shape, dens, seed=100 * di + nx + ny + nz)
            d2, site = dr.separable(m, step)
            b2, bsite, tie = dr.brute_force(m, step)
            assert d2.dtype == np.float32 and np.array_equal(d2.view(np.uint32), b2.view(np.uint32)), (shape, dens)
            if not m.any():
                assert np.isinf(d2).all() and (site == -1).all()
                continue
            assert np.array_equal(site[~tie], bsite[~tie]), (shape, dens)
            k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
            s = site.astype(np.int64); assert (s >= 0).all() and m.reshape(-1)[s.reshape(-1)].all()
            sq = lambda a, b, st: ((a - b).astype(f) * f(st)) * ((a - b).astype(f) * f(st))      # noqa: E731
            at = (sq(i, s % nx, step[0]) + sq(j, (s // nx) % ny, step[1])) + sq(k, s // (nx * ny), step[2])
            assert np.array_equal(at.view(np.uint32), d2.view(np.uint32)), (shape, dens)
            if min(abs(v) for v in step) > 0:                                         # no zero step: an occupied cell is its own nearest cell
                assert (site[m != 0].reshape(-1) == np.flatnonzero(m.reshape(-1))).all(), (shape, dens)
            n_tie += int(tie.sum()); n_cells += m.size
    if step == (0.25, 0.25, 0.25):
        assert n_tie > 100, n_tie                                                     # power-of-two steps: ties are everywhere, and the check saw them


def test_reference_truncation_rule():
    """finish: the correctly rounded root; a cell at exactly max_dist keeps its site, one above it loses it; +inf cuts nothing; an empty mask gives max_dist."""
    m = np.zeros((1, 1, 6), np.uint8); m[0, 0, 0] = 1
    d2, site = dr.separable(m, (0.5, 1.0, 1.0))
    assert np.array_equal(d2.reshape(-1), np.float32([0, 0.25, 1.0, 2.25, 4.0, 6.25])) and (site == 0).all()
    dist, near = dr.finish(d2, site, 1.5)
    assert np.array_equal(dist.reshape(-1), np.float32([0, 0.5, 1.0, 1.5, 1.5, 1.5])) and near.reshape(-1).tolist() == [0, 0, 0, 0, -1, -1]
    dist, near = dr.finish(d2, site, np.inf)
    assert np.array_equal(dist.reshape(-1), np.float32([0, 0.5, 1.0, 1.5, 2.0, 2.5])) and (near == 0).all()
    dist, near = dr.transform(np.zeros((2, 2, 2), np.uint8), (1, 1, 1), 3.0)
    assert (dist == 3.0).all() and (near == -1).all()
    dist, near = dr.transform(np.zeros((2, 2, 2), np.uint8), (1, 1, 1))
    assert np.isinf(dist).all() and (near == -1).all()
