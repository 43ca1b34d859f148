"""The connected components of include/mon_core.h (mon_label_components) restated independently of the device's algorithm: a sequential
flood fill that visits the cells in ascending flat index, so the first unlabelled mask cell it meets is by construction the lowest cell of its component
and gives the component its label.  No tiles, no unions, no atomics.  Helpers derive comp and the table from label as the header defines them, and the
named masks of the tests are generated here.  A plain module, like tests/distance_reference.py: no fixtures, no hooks.

Masks have shape (nz, ny, nx) (x fastest); a label is a flat index (k * ny + j) * nx + i."""
import numpy as np

TABLE_DTYPE = np.dtype([("rep", np.int32), ("cells", np.uint32), ("lo", np.int32, 3), ("hi", np.int32, 3)])
SUM_LIMIT = {6: 1, 18: 2, 26: 3}


def offsets(connectivity):
    """(dx, dy, dz) of the adjacent cells: each coordinate differs by at most 1, the sum of the absolute differences by at most m, not all 0"""
    m = SUM_LIMIT[connectivity]
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 < abs(dx) + abs(dy) + abs(dz) <= m]


def flood_fill(mask, connectivity):
    """label of the mask's shape, int32: the lowest flat index of the cell's component, -1 outside the mask"""
    m = np.asarray(mask) != 0
    nz, ny, nx = m.shape
    pad = np.zeros((nz + 2, ny + 2, nx + 2), bool); pad[1:-1, 1:-1, 1:-1] = m                       # a border of cells outside the mask: nothing wraps
    sy, sz = nx + 2, (ny + 2) * (nx + 2)
    offs = [dz * sz + dy * sy + dx for dx, dy, dz in offsets(connectivity)]
    todo = pad.reshape(-1).tolist()                                                                  # True: a mask cell without a label yet
    lab = [-1] * len(todo)
    padded = ((np.arange(nz)[:, None, None] + 1) * sz + (np.arange(ny)[None, :, None] + 1) * sy + (np.arange(nx)[None, None, :] + 1)).reshape(-1).tolist()
    for flat, p in enumerate(padded):                                                                # ascending flat index
        if todo[p]:
            todo[p] = False; lab[p] = flat; stack = [p]
            while stack:
                c = stack.pop()
                for o in offs:
                    q = c + o
                    if todo[q]:
                        todo[q] = False; lab[q] = flat; stack.append(q)
    return np.ascontiguousarray(np.array(lab, np.int32).reshape(pad.shape)[1:-1, 1:-1, 1:-1])


def representatives(label):
    flat = label.reshape(-1)
    return np.flatnonzero(flat == np.arange(flat.size, dtype=np.int64)).astype(np.int32)


def comp_of(label):
    """the rank of each cell's component by ascending representative, -1 outside the mask"""
    reps = representatives(label)
    comp = np.searchsorted(reps, label).astype(np.int32)
    comp[label < 0] = -1
    return comp


def table_of(label):
    """one record per component, by ascending representative: rep, cells, the inclusive bounding box in (i, j, k)"""
    nz, ny, nx = label.shape
    reps = representatives(label); comp = comp_of(label).reshape(-1)
    t = np.zeros(reps.size, TABLE_DTYPE)
    t["rep"] = reps
    on = comp >= 0; c = comp[on]
    t["cells"] = np.bincount(c, minlength=reps.size)
    flat = np.flatnonzero(on)
    ijk = np.stack([flat % nx, (flat // nx) % ny, flat // (nx * ny)], axis=1).astype(np.int32)
    lo = np.full((reps.size, 3), np.iinfo(np.int32).max, np.int32); hi = np.full((reps.size, 3), np.iinfo(np.int32).min, np.int32)
    np.minimum.at(lo, c, ijk); np.maximum.at(hi, c, ijk)
    t["lo"] = lo; t["hi"] = hi
    return t


def components(mask, connectivity):
    """(label, comp, table, n_components) of the mask"""
    label = flood_fill(mask, connectivity)
    table = table_of(label)
    return label, comp_of(label), table, int(table.size)


# ---------------------------------------------------------------------------------------------------------------- the named masks
def random_mask(shape_xyz, density, seed):
    """density: 0, "one" (one cell), 1 (all cells) or the fraction of mask cells; shape_xyz = (nx, ny, nz) -> mask (nz, ny, nx) of uint8"""
    nx, ny, nz = shape_xyz; rng = np.random.default_rng(seed)
    m = np.zeros((nz, ny, nx), np.uint8)
    if density == "one":
        m.reshape(-1)[rng.integers(m.size)] = 1
    elif density >= 1:
        m[:] = 1
    elif density > 0:
        m[:] = rng.random(m.shape) < density
    return m


def checkerboard(shape_xyz):
    """(i + j + k) % 2 == 0: no two mask cells share a face, every mask cell has an edge neighbour in the mask"""
    nx, ny, nz = shape_xyz
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return ((i + j + k) % 2 == 0).astype(np.uint8)


def serpentine(shape_xyz):
    """One 6-connected path through the whole lattice, from cell 0.  In every slab of even k: the full rows of even j, joined by one cell on the odd j
    between two of them, alternately at i = nx - 1 and at i = 0 -- a path from (0, 0) to the end of the last even row.  Between two even slabs one cell on
    the odd k, alternately at the place where that path ends and at (0, 0): the next slab runs the same path backwards."""
    nx, ny, nz = shape_xyz
    slab = np.zeros((ny, nx), np.uint8)
    slab[0::2, :] = 1
    for r, j in enumerate(range(1, ny - 1, 2)):                                                      # (an odd j with a row behind it)
        slab[j, nx - 1 if r % 2 == 0 else 0] = 1
    rows = (ny + 1) // 2
    end = (2 * (rows - 1), nx - 1 if rows % 2 == 1 else 0)                                            # (j, i) where the slab's path ends
    m = np.zeros((nz, ny, nx), np.uint8)
    m[0::2] = slab
    for r, k in enumerate(range(1, nz - 1, 2)):
        j, i = end if r % 2 == 0 else (0, 0)
        m[k, j, i] = 1
    return m
