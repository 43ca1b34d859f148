"""CPU-side checks (no device needed) of the connected-components boundary (include/mon_core.h): mon_label_components,
mon_scene_components_lattice and mon_online_components_lattice are declared, exported and bound with the header's signatures; mon_lattice_component is 32
bytes; the new source is listed for every build; every argument error is MON_ERR_ARG before any device work, with a message and the outputs untouched;
and the reference the GPU tests compare with (tests/components_reference.py, a sequential flood fill) is pinned on its own: against closed forms, and
against scipy.ndimage where scipy is installed.  (The rows that need a device are in tests/test_components.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from abi_decl import bound as _bound, decl as _decl, kind as _kind, p as _p
import components_reference as cr

NEW = ("mon_label_components", "mon_scene_components_lattice", "mon_online_components_lattice")
MON_ERR_ARG, MON_ERR_NO_DEVICE = 1, 2


def test_symbols_are_declared_exported_and_bound(pkg):
    import importlib
    b = importlib.import_module(pkg.__name__ + ".binding")
    core = C.CDLL(pkg.lib_path())
    for name in NEW:
        assert name in pkg.exported_symbols() and hasattr(core, name), name
        assert [_kind(a) for a in _decl(name)] == [_bound(t) for t in b._SIGS[name][1]], name
    assert [len(_decl(n)) for n in NEW] == [11, 20, 18]
    assert [_kind(a) for a in _decl("mon_label_components")] == ["int", "ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr", "uint32", "ptr"]
    assert [_kind(a) for a in _decl("mon_scene_components_lattice")] == (["ptr", "u64", "int", "ptr", "ptr", "int", "int", "int", "float", "int", "float", "int"] +
                                                                        ["ptr"] * 3 + ["uint32"] + ["ptr"] * 4)
    assert _decl("mon_online_components_lattice")[1:] == _decl("mon_scene_components_lattice")[3:]      # "the same from origin3 on"
    for name in ("label_components", "scene_components_lattice"):
        assert callable(getattr(pkg, name)), name
    assert callable(pkg.OnlineManager.components_lattice)


def test_component_record_is_32_bytes(pkg):
    """the header's struct, field by field, and the dtype the binding returns tables in"""
    txt = open(os.path.join(ROOT, "include", "mon_core.h")).read()
    m = re.search(r"typedef struct mon_lattice_component \{([^}]*)\} mon_lattice_component;", txt)
    assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == ["int32_t rep", "uint32_t cells", "int32_t lo[3]", "int32_t hi[3]"]
    d = pkg.LATTICE_COMPONENT_DTYPE
    assert d.itemsize == 32 and cr.TABLE_DTYPE == d
    assert [(n, d.fields[n][1]) for n in d.names] == [("rep", 0), ("cells", 4), ("lo", 8), ("hi", 20)]


def test_new_source_is_listed_for_every_build():
    """sources.sh is what build.sh, the variant builds and the ThreadSanitizer host build compile: the components kernels are in it."""
    txt = open(os.path.join(ROOT, "ro-map_amd", "sources.sh")).read()
    assert "kernels_components.hip" in txt and os.path.exists(os.path.join(ROOT, "ro-map_amd", "csrc", "kernels_components.hip"))


def test_argument_errors_need_no_device(pkg):
    """NULL mask / label / step / origin / objs / element / manager; a table without n_components; a dimension below 1; nx * ny * nz above 2^22 (shapes
    whose product wraps 64 bits included); a connectivity other than 6 / 18 / 26; a non-finite step or origin; sigma_min negative, NaN or infinite; a
    region other than 0 / 1; region 1 with a negative, NaN or infinite clearance; region 0 with dist; side not 0 / 1; n_objs 0 and above 256: MON_ERR_ARG
    with a message and every output untouched, whether or not a device is present.  What the argument checks accept (optional outputs NULL, region 0 with
    any clearance, region 1 with dist) fails on the NULL object alone; the standalone call without a device is MON_ERR_NO_DEVICE after its checks."""
    L = pkg.lib()
    nulls = (C.c_void_p * 4)(None, None, None, None); many = (C.c_void_p * 300)()
    mask = np.ones(24, np.uint8); s3 = np.array([0.25, 0.0, -0.125], np.float32); o3 = np.array([0.5, -1.0, 2.0], np.float32)
    label = np.full(64, 7, np.int32); comp = np.full(64, 7, np.int32); table = np.full(64 * 8, 7, np.int32); nc = np.full(1, 7, np.uint32)
    dist = np.full(64, 7.0, np.float32); sig = np.full(64, 7.0, np.float32); own = np.full(64, 7, np.int32)

    def ed(a, i, v):
        b = a.copy(); b[i] = v; return b

    def lc(m=mask, shape=(2, 3, 4), conn=6, lab=label, cm=comp, tab=table, cap=64, n=nc, device=0):
        return L.mon_label_components(device, _p(m), *shape, conn, _p(lab), _p(cm), _p(tab), cap, _p(n))

    wrap = ((1 << 30, 1 << 30, 1 << 30), (1 << 22, 1 << 21, 1 << 21), (2147483647, 2147483647, 2147483647), (1, 1 << 22, 2), (1 << 16, 1 << 16, 1 << 16))
    for kw in (dict(m=None), dict(lab=None), dict(n=None), dict(lab=None, cm=None, tab=None, n=None), dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)),
               dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)), dict(shape=(2, 3, -7)), dict(shape=(1 << 11, 1 << 11, 2)), dict(shape=((1 << 22) + 1, 1, 1)),
               dict(conn=0), dict(conn=4), dict(conn=8), dict(conn=27), dict(conn=-6), dict(conn=1)) + tuple(dict(shape=w) for w in wrap):
        assert lc(**kw) == MON_ERR_ARG and L.mon_last_error(), kw
    for w in wrap + ((1 << 11, 1 << 11, 2),):
        assert lc(shape=w) == MON_ERR_ARG and b"points" in L.mon_last_error(), w
    assert lc(conn=8) == MON_ERR_ARG and b"connectivity" in L.mon_last_error()
    assert lc(lab=None) == MON_ERR_ARG and b"label" in L.mon_last_error()
    assert lc(n=None) == MON_ERR_ARG and b"n_components" in L.mon_last_error()
    if pkg.device_count() == 0:
        for kw in (dict(), dict(cm=None, tab=None, n=None), dict(conn=18), dict(conn=26), dict(cap=0)):
            assert lc(**kw) == MON_ERR_NO_DEVICE and L.mon_last_error(), kw                            # accepted by the checks; then no device

    def lat(objs=nulls, n_objs=1, side=0, o=o3, s=s3, shape=(2, 3, 4), smin=1.0, region=0, clr=0.0, conn=6, lab=label, cm=comp, tab=table, cap=64, n=nc,
            rest=(None, sig, own)):
        return L.mon_scene_components_lattice(objs, n_objs, side, _p(o), _p(s), *shape, smin, region, clr, conn, _p(lab), _p(cm), _p(tab), cap, _p(n),
                                              *[_p(a) for a in rest])

    def onl(o=o3, s=s3, shape=(2, 3, 4), smin=1.0, region=0, clr=0.0, conn=6, lab=label, cm=comp, tab=table, cap=64, n=nc, rest=(None, sig, own)):
        return L.mon_online_components_lattice(None, _p(o), _p(s), *shape, smin, region, clr, conn, _p(lab), _p(cm), _p(tab), cap, _p(n),
                                               *[_p(a) for a in rest])

    accepted = (dict(), dict(cm=None, tab=None, n=None, rest=(None,) * 3), dict(smin=0.0), dict(conn=18), dict(conn=26), dict(clr=-1.0),
                dict(clr=float("nan")), dict(region=1, clr=0.0, rest=(dist, sig, own)), dict(region=1, clr=0.5), dict(tab=None), dict(cap=0))
    refused = (dict(objs=None), dict(o=None), dict(s=None), dict(lab=None), dict(n=None), dict(n_objs=0), dict(objs=many, n_objs=257),
               dict(shape=(0, 3, 4)), dict(shape=(2, 0, 4)), dict(shape=(2, 3, 0)), dict(shape=(-1, 3, 4)), dict(shape=(1 << 11, 1 << 11, 2)),
               dict(shape=((1 << 22) + 1, 1, 1)), dict(side=2), dict(side=-1), dict(o=ed(o3, 0, np.nan)), dict(o=ed(o3, 2, np.inf)), dict(s=ed(s3, 1, np.nan)),
               dict(s=ed(s3, 0, -np.inf)), dict(smin=-1e-6), dict(smin=float("nan")), dict(smin=np.inf), dict(conn=0), dict(conn=7), dict(conn=27),
               dict(region=2), dict(region=-1), dict(region=1, clr=-1e-6), dict(region=1, clr=float("nan")), dict(region=1, clr=np.inf),
               dict(region=0, rest=(dist, sig, own))) + tuple(dict(shape=w) for w in wrap)
    for kw in accepted + refused:
        assert lat(**kw) == MON_ERR_ARG and L.mon_last_error(), kw                 # (the accepted ones: a NULL element of objs)
    for kw in accepted:
        assert lat(**kw) == MON_ERR_ARG and b"object" in L.mon_last_error(), kw    # accepted by the argument checks: fails on the NULL object alone
    assert lat(shape=(1 << 11, 1 << 11, 1)) == MON_ERR_ARG and b"object" in L.mon_last_error()      # 2^22 cells: accepted
    for kw, word in ((dict(smin=-1e-6), b"sigma_min"), (dict(conn=7), b"connectivity"), (dict(region=2), b"region"), (dict(region=1, clr=-1e-6), b"clearance"),
                     (dict(region=0, rest=(dist, sig, own)), b"dist"), (dict(side=2), b"side"), (dict(objs=many, n_objs=257), b"objects"),
                     (dict(lab=None), b"label"), (dict(n=None), b"n_components")):
        assert lat(**kw) == MON_ERR_ARG and word in L.mon_last_error(), kw
    for kw in (dict(), dict(conn=5), dict(smin=-1.0), dict(shape=(0, 1, 1)), dict(lab=None), dict(region=3), dict(region=1, clr=-1.0)):
        assert onl(**kw) == MON_ERR_ARG, kw                                        # a NULL manager, with good and with bad arguments
    assert (label == 7).all() and (comp == 7).all() and (table == 7).all() and (nc == 7).all() and (own == 7).all()
    assert (dist == 7.0).all() and (sig == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- the reference, pinned on its own
def _consistent(mask, label, comp, table, n, conn):
    """what the header's definitions imply, whatever produced the arrays"""
    on = mask != 0
    flat = np.arange(mask.size, dtype=np.int32).reshape(mask.shape)
    assert ((label >= 0) == on).all() and ((comp >= 0) == on).all() and (label[on] <= flat[on]).all()
    assert (label.reshape(-1)[label[on]] == label[on]).all()                       # label[rep] == rep
    assert n == table.size == np.unique(label[on]).size and (np.diff(table["rep"]) > 0).all()
    assert (table["rep"][comp[on]] == label[on]).all() and int(table["cells"].sum()) == int(on.sum())
    nz, ny, nx = mask.shape
    for dx, dy, dz in cr.offsets(conn):                                            # adjacent mask cells carry one label
        a = label[max(dz, 0):nz + min(dz, 0), max(dy, 0):ny + min(dy, 0), max(dx, 0):nx + min(dx, 0)]
        b = label[max(-dz, 0):nz + min(-dz, 0), max(-dy, 0):ny + min(-dy, 0), max(-dx, 0):nx + min(-dx, 0)]
        both = (a >= 0) & (b >= 0)
        assert (a[both] == b[both]).all(), (dx, dy, dz)


def test_reference_on_closed_forms():
    """10 x 9 x 8 checkerboard: under 6 every mask cell is its own component, under 18 and 26 there is exactly one.  The serpentine on 37 x 35 x 33 is one
    component of 11 627 cells under 6 in which every cell has two mask neighbours but the two ends: a pure path, of eccentricity 11 626 from cell 0.  An
    empty mask has no component, a full one a single component with rep 0 and the lattice as its box."""
    m = cr.checkerboard((10, 9, 8)); assert m.shape == (8, 9, 10) and m.sum() == 360
    label, comp, table, n = cr.components(m, 6)
    assert n == 360 and (label[m != 0] == np.flatnonzero(m.reshape(-1))).all() and (table["cells"] == 1).all() and (table["lo"] == table["hi"]).all()
    for conn in (18, 26):
        label, comp, table, n = cr.components(m, conn)
        assert n == 1 and table[0]["rep"] == 0 and table[0]["cells"] == 360 and table[0]["lo"].tolist() == [0, 0, 0] and table[0]["hi"].tolist() == [9, 8, 7]
        _consistent(m, label, comp, table, n, conn)
    s = cr.serpentine((37, 35, 33)); assert s.sum() == 11627 and s[0, 0, 0] == 1
    label, comp, table, n = cr.components(s, 6)
    assert n == 1 and table[0]["cells"] == 11627 and (label[s != 0] == 0).all()
    pad = np.pad(s.astype(np.int32), 1)
    deg = sum(np.roll(pad, sh, ax) for ax in range(3) for sh in (-1, 1))[1:-1, 1:-1, 1:-1]
    assert sorted(np.bincount(deg[s != 0]).tolist()) == [0, 2, 11625] and deg[0, 0, 0] == 1     # two ends (cell 0 is one), every other cell inside the path
    for shape in ((5, 4, 3), (1, 1, 1), (6, 1, 4), (1, 7, 2), (8, 8, 8), (37, 35, 33)):          # every size: one component under 6, from cell 0
        sm = cr.serpentine(shape)
        assert cr.components(sm, 6)[3] == 1 and sm[0, 0, 0] == 1, shape
    z = np.zeros((3, 4, 5), np.uint8)
    label, comp, table, n = cr.components(z, 26); assert n == 0 and table.size == 0 and (label == -1).all() and (comp == -1).all()
    label, comp, table, n = cr.components(z + 1, 6)
    assert n == 1 and (label == 0).all() and (comp == 0).all() and table[0]["cells"] == 60 and table[0]["hi"].tolist() == [4, 3, 2]


@pytest.mark.parametrize("conn", [6, 18, 26])
@pytest.mark.parametrize("shape", [(19, 23, 17), (33, 31, 29)])
def test_reference_equals_scipy(shape, conn):
    """Random masks at 2 %, 31 % and 50 %: label equals scipy.ndimage.label's components named by ndimage.minimum of the flat index; comp equals
    scipy's numbering minus one (scipy numbers in raster order of the first cell met, which is ascending representative); cells and boxes equal
    ndimage.sum and ndimage.find_objects."""
    ndi = pytest.importorskip("scipy.ndimage")
    nx, ny, nz = shape
    for di, dens in enumerate((0.02, 0.31, 0.5)):
        m = cr.random_mask(shape, dens, seed=7000 + 10 * di + nx)
        label, comp, table, n = cr.components(m, conn)
        lbl, cnt = ndi.label(m, structure=ndi.generate_binary_structure(3, cr.SUM_LIMIT[conn]))
        assert cnt == n, (shape, conn, dens)
        flat = np.arange(m.size).reshape(m.shape)
        mins = np.asarray(ndi.minimum(flat, lbl, index=np.arange(1, cnt + 1))).astype(np.int32)
        want = np.where(lbl > 0, mins[np.maximum(lbl, 1) - 1], -1).astype(np.int32)
        assert np.array_equal(label, want), (shape, conn, dens)
        assert np.array_equal(comp, lbl.astype(np.int32) - 1), (shape, conn, dens)
        assert np.array_equal(table["rep"], mins) and np.array_equal(table["cells"], np.asarray(ndi.sum(m, lbl, index=np.arange(1, cnt + 1))).astype(np.uint32))
        for c, sl in enumerate(ndi.find_objects(lbl)):
            assert table[c]["lo"].tolist() == [sl[2].start, sl[1].start, sl[0].start] and table[c]["hi"].tolist() == [sl[2].stop - 1, sl[1].stop - 1, sl[0].stop - 1]
        _consistent(m, label, comp, table, n, conn)
        if shape == (33, 31, 29) and conn == 6 and di == 1:
            print("31 %% under 6 on 33 x 31 x 29: %d components, the largest %d of %d cells" % (n, int(table["cells"].max()), int(m.sum())))
            assert n > 1000 and table["cells"].max() > 500                                            # the near-percolation regime
