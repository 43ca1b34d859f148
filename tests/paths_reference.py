"""The shortest-path cost field of include/mon_core.h (mon_shortest_paths) restated twice on the host, independently of the device's
tiles and of each other: a heap Dijkstra that settles one cell at a time, and a whole-lattice Jacobi sweep in numpy that relaxes every cell from the
previous sweep's values until nothing changes.  Both do the rule's arithmetic in fp32, every operation rounded on its own, so by the header's argument (fp32
addition is monotone and fl(c + w) >= c for w >= 0: the least fold over all walks is the least fixed point under any relaxation order) they agree with
each other and with the device in every bit.  `next_of` is the header's rule for next, `truncate` its max_cost cut.  A plain module, like
tests/components_reference.py: no fixtures, no hooks.

Masks, multipliers, cost and next have shape (nz, ny, nx) (x fastest); a cell's flat index is (k * ny + j) * nx + i; step = (sx, sy, sz)."""
import heapq

import numpy as np

F = np.float32
SUM_LIMIT = {6: 1, 18: 2, 26: 3}


def offsets(connectivity):
    """(dx, dy, dz) of the adjacent cells in ascending flat index: dz slowest, dx fastest"""
    m = SUM_LIMIT[connectivity]
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 < abs(dx) + abs(dy) + abs(dz) <= m]


def move_length(step, dx, dy, dz):
    """len = sqrtf(((a_x * a_x) + (a_y * a_y)) + (a_z * a_z)) with a = (float)d * step, every operation an fp32 one"""
    s = np.asarray(step, F)
    ax, ay, az = F(dx) * s[0], F(dy) * s[1], F(dz) * s[2]
    with np.errstate(over="ignore"):
        return np.sqrt(F(F(F(ax * ax) + F(ay * ay)) + F(az * az)), dtype=F)


def _padded(mask, cell_cost):
    """the mask with a border of blocked cells (nothing wraps), the multiplier with a border of zeros, both flat; the padded index of every cell"""
    m = np.asarray(mask) != 0
    nz, ny, nx = m.shape
    pm = np.zeros((nz + 2, ny + 2, nx + 2), bool); pm[1:-1, 1:-1, 1:-1] = m
    pc = None
    if cell_cost is not None:
        pc = np.zeros(pm.shape, F); pc[1:-1, 1:-1, 1:-1] = np.asarray(cell_cost, F).reshape(m.shape)
    sy, sz = nx + 2, (ny + 2) * (nx + 2)
    cells = ((np.arange(nz)[:, None, None] + 1) * sz + (np.arange(ny)[None, :, None] + 1) * sy + (np.arange(nx)[None, None, :] + 1)).reshape(-1)
    return pm.reshape(-1), None if pc is None else pc.reshape(-1), cells, sy, sz


def _weights(step, connectivity, pc, sy, sz):
    """per offset: its padded stride and w(u, v) for u = v + stride -- an fp32 scalar without a multiplier, else an fp32 array over the padded cells v,
    fl(len * fl(0.5f * fl(c[u] + c[v]))) (np.roll's wrap only reaches border cells, which are blocked)"""
    out = []
    for dx, dy, dz in offsets(connectivity):
        st = dz * sz + dy * sy + dx
        ln = move_length(step, dx, dy, dz)
        if pc is None:
            out.append((st, ln))
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                out.append((st, (ln * (F(0.5) * (np.roll(pc, -st) + pc).astype(F)).astype(F)).astype(F)))
    return out


def _seeded(pm, cells, seeds):
    cost = np.full(pm.size, np.inf, F)
    sd = cells[np.asarray(seeds, np.int64).reshape(-1)]
    cost[sd[pm[sd]]] = 0
    return cost


def dijkstra(mask, seeds, step, connectivity, cell_cost=None):
    """cost of the mask's shape, fp32: one cell settled at a time, the cheapest first.  (The fold's values are kept as Python floats that hold fp32 values;
    a + w is exact enough in double that rounding it to fp32 is the fp32 sum.)"""
    pm, pc, cells, sy, sz = _padded(mask, cell_cost)
    w = _weights(step, connectivity, pc, sy, sz)
    strides = [st for st, _ in w]
    wl = [x.astype(np.float64).tolist() if pc is not None else float(x) for _, x in w]
    cost = _seeded(pm, cells, seeds).astype(np.float64).tolist()
    ok = pm.tolist(); done = [False] * len(ok)
    heap = [(0.0, int(c)) for c in np.flatnonzero(np.asarray(cost) == 0)]
    heapq.heapify(heap)
    while heap:
        c, v = heapq.heappop(heap)
        if done[v] or c > cost[v]:
            continue
        done[v] = True
        for k, st in enumerate(strides):
            u = v + st
            if not ok[u] or done[u]:
                continue
            wk = wl[k][v] if pc is not None else wl[k]          # (offset k's array at v pairs v with v + st = u, and w is symmetric)
            cand = float(F(c + wk))
            if cand < cost[u]:
                cost[u] = cand; heapq.heappush(heap, (cand, u))
    return np.ascontiguousarray(np.array(cost, np.float64).astype(F)[cells].reshape(np.asarray(mask).shape))


def jacobi(mask, seeds, step, connectivity, cell_cost=None, return_sweeps=False):
    """cost of the mask's shape, fp32: every passable cell takes the least of its value and fl(neighbour + w) over the previous sweep's values, the whole
    lattice at once, until a sweep changes nothing"""
    pm, pc, cells, sy, sz = _padded(mask, cell_cost)
    w = _weights(step, connectivity, pc, sy, sz)
    cost = _seeded(pm, cells, seeds)
    sweeps = 0
    while True:
        new = cost.copy()
        with np.errstate(invalid="ignore"):
            for st, wk in w:
                cand = (np.roll(cost, -st) + wk).astype(F)      # cand[v] = fl(cost[v + st] + w(v + st, v))
                better = pm & (cand < new)
                new[better] = cand[better]
        sweeps += 1
        if np.array_equal(new, cost):
            break
        cost = new
    out = np.ascontiguousarray(cost[cells].reshape(np.asarray(mask).shape))
    return (out, sweeps) if return_sweeps else out


def next_of(cost, mask, step, connectivity, cell_cost=None):
    """next by the header's rule on the untruncated cost: per cell the first neighbour u in ascending flat index with cost[u] < cost[v] and
    fl(cost[u] + w(u, v)) == cost[v], as a flat index of the lattice; -1 without one, on unreachable cells and outside the mask"""
    pm, pc, cells, sy, sz = _padded(mask, cell_cost)
    w = _weights(step, connectivity, pc, sy, sz)
    pcst = np.full(pm.size, np.inf, F); pcst[cells] = np.asarray(cost, F).reshape(-1)
    flat = np.full(pm.size, -1, np.int64); flat[cells] = np.arange(cells.size)
    nxt = np.full(pm.size, -1, np.int64)
    live = pm & np.isfinite(pcst)
    with np.errstate(invalid="ignore"):
        for st, wk in w:
            cu = np.roll(pcst, -st)
            hit = live & (nxt < 0) & (cu < pcst) & ((cu + wk).astype(F) == pcst)
            nxt[hit] = np.roll(flat, -st)[hit]
    return np.ascontiguousarray(nxt[cells].astype(np.int32).reshape(np.asarray(mask).shape))


def truncate(cost, nxt, max_cost):
    """where !(cost <= max_cost): cost = +inf and next = -1"""
    cut = ~(cost <= F(max_cost))
    c = cost.copy(); n = nxt.copy()
    c[cut] = np.inf; n[cut] = -1
    return c, n


def field(mask, seeds, step, connectivity, cell_cost=None, max_cost=np.inf, solver=jacobi):
    """(cost, next) as mon_shortest_paths returns them"""
    cost = solver(mask, seeds, step, connectivity, cell_cost)
    return truncate(cost, next_of(cost, mask, step, connectivity, cell_cost), max_cost)


def follow(nxt, start):
    """the flat indices from start along next to the first -1, start included (mon_lattice_path)"""
    flat = np.asarray(nxt).reshape(-1); path = [int(start)]
    while flat[path[-1]] >= 0:
        path.append(int(flat[path[-1]]))
        assert len(path) <= flat.size, "next holds a cycle"
    return path


# ---------------------------------------------------------------------------------------------------------------- the named masks
def random_mask(shape_xyz, share, seed):
    """share: 0, "one" (one passable cell), 1 (all cells) or the fraction of passable cells; shape_xyz = (nx, ny, nz) -> mask (nz, ny, nx) of uint8"""
    nx, ny, nz = shape_xyz; rng = np.random.default_rng(seed)
    m = np.zeros((nz, ny, nx), np.uint8)
    if share == "one":
        m.reshape(-1)[rng.integers(m.size)] = 1
    elif share >= 1:
        m[:] = 1
    elif share > 0:
        m[:] = rng.random(m.shape) < share
    return m


def wall_with_hole(shape_xyz, i_wall, hole_jk):
    """all cells passable but the plane i = i_wall, which is blocked except at (j, k) = hole_jk"""
    nx, ny, nz = shape_xyz
    m = np.ones((nz, ny, nx), np.uint8)
    m[:, :, i_wall] = 0
    m[hole_jk[1], hole_jk[0], i_wall] = 1
    return m
