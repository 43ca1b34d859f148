// kernels_components.hip -- connected components over a lattice (mon_label_components, mon_scene_components_lattice): per mask cell the
// lowest flat index of its component (label), the component's rank by ascending representative (comp), the count and one record per component.
// Four stages, every one a launch of its own, nothing waits for another workgroup:
//   1  k_cc_local<CONN>   a workgroup labels a tile of 32 x 8 x 4 cells in LDS and writes each cell's tile-local root as a flat index
//   2  k_cc_merge<CONN>   unites cells across tile borders: union by lowest index on label[], decided by what the atomic returns
//   3  k_cc_flatten       label[i] = root(i); counts the representatives (label[i] == i) per block;  k_cc_scan: the blocks' offsets and the total
//   4  k_cc_number        the representatives' ranks by prefix sum, their table records opened;  k_cc_table: comp of every cell, the records filled with
//                         integer add / min / max atomics (they commute: the bits do not depend on the order)
// The result is a function of the mask, the shape and the connectivity alone.  The labelling is integers only; no scratch, vector atomics only.
// Every loop walks strictly decreasing indices or is a fixed point whose rounds the tile bounds; each also has an explicit cap, and exceeding one sets
// the flag word the host turns into MON_ERR_STATE.
#include <algorithm>
#include <climits>
#include "lattice_device.h"

namespace mon {

constexpr uint32_t kCcPer = kTileCells / 256;
static_assert(kCcPer * 256 == kTileCells, "every thread owns kCcPer cells of the tile");
constexpr uint32_t kCcRoundCap = kTileCells + 1;                   // a tile's fixed point: at most one round per cell (see k_cc_local), one more to see it
constexpr uint32_t kCcWalkCap = (1u << 22) + 1;                 // a walk to the root strictly decreases an index below n <= 2^22
constexpr uint32_t kCcUnionCap = (1u << 23) + 2;                // a union's rounds strictly decrease a + b < 2 n

__device__ __forceinline__ int32_t cc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_fail(uint32_t* flag) { atomicOr(flag, 1u); }

// f(dx, dy, dz) for every admitted neighbour among the 13 of lower flat index: dz = -1 with any dx, dy; dz = 0, dy = -1 with any dx; (-1, 0, 0)
template <int CONN, class F> __device__ __forceinline__ void cc_lower_neighbours(F&& f) {
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const bool lower = dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)));
                if (lower && admits<CONN>(dx, dy, dz)) f(dx, dy, dz);
            }
}

// ---- 1: a tile in LDS.  lab[c] (c = (lz * 8 + ly) * 32 + lx, the order of the flat indices) is -1 outside the mask or the lattice, else a cell of c's
// component inside the tile with lab[c] <= c: a forest whose parents only decrease.  A round: every edge (c, lower neighbour) with different labels a, b
// links the higher of the two to the lower (atomicMin on lab[max(a, b)]); then every cell walks to its root and stores it.  After a round a cell's label is
// at most each neighbour's label of before it, so the component's lowest cell reaches every cell within a path's length of rounds: at most the tile's cells.
// The fixed point (no edge with two labels) gives every cell its component's lowest cell of the tile.
template <int CONN> __global__ void __launch_bounds__(256) k_cc_local(const uint8_t* __restrict__ occ, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t tiles_x,
        uint32_t tiles_y, int32_t* __restrict__ label, uint32_t* __restrict__ flag) {
    __shared__ int32_t lab[kTileCells];
    const uint32_t tid = threadIdx.x;
    const Cell t = split(blockIdx.x, tiles_x, tiles_y); const uint32_t tx = t.x, ty = t.y, tz = t.z;
    const uint32_t lx = tid % kTileX, ly = tid / kTileX;                              // the thread's cells: (lx, ly, q), q < kCcPer = kTileZ
    const uint32_t x = tx * kTileX + lx, y = ty * kTileY + ly;
    bool on[kCcPer];                                                                // the cell lies in the lattice and in the mask
#pragma unroll
    for (uint32_t q = 0; q < kCcPer; ++q) {
        const uint32_t z = tz * kTileZ + q, c = q * 256u + tid;
        on[q] = x < nx && y < ny && z < nz && occ[((size_t)z * ny + y) * nx + x] != 0;
        lab[c] = on[q] ? (int32_t)c : -1;
    }
    __syncthreads();
    uint32_t round = 0;
    for (; round < kCcRoundCap; ++round) {
        bool changed = false;
#pragma unroll
        for (uint32_t q = 0; q < kCcPer; ++q) {
            if (!on[q]) continue;
            const uint32_t c = q * 256u + tid;
            const int32_t a = lab[c];
            cc_lower_neighbours<CONN>([&](int dx, int dy, int dz) {
                if ((int)lx + dx < 0 || (int)lx + dx >= (int)kTileX || (int)ly + dy < 0 || (int)ly + dy >= (int)kTileY || (int)q + dz < 0) return;
                const int32_t b = lab[(int)c + (dz * (int)kTileY + dy) * (int)kTileX + dx];
                if (b >= 0 && b != a) { atomicMin(&lab[max(a, b)], min(a, b)); changed = true; }
            });
        }
        if (!__syncthreads_or(changed)) break;
#pragma unroll
        for (uint32_t q = 0; q < kCcPer; ++q) {
            if (!on[q]) continue;
            const uint32_t c = q * 256u + tid;
            int32_t l = lab[c];
            for (uint32_t it = 0; it < kTileCells; ++it) { const int32_t p = lab[l]; if (p == l) break; l = p; }      // strictly decreasing
            lab[c] = l;
        }
        __syncthreads();
    }
    if (round == kCcRoundCap && tid == 0) cc_fail(flag);
#pragma unroll
    for (uint32_t q = 0; q < kCcPer; ++q) {
        const uint32_t z = tz * kTileZ + q;
        if (!(x < nx && y < ny && z < nz)) continue;
        int32_t out = -1;
        if (on[q]) {
            const uint32_t r = (uint32_t)lab[q * 256u + tid];
            out = (int32_t)((((size_t)(tz * kTileZ + r / 256u)) * ny + (ty * kTileY + (r % 256u) / kTileX)) * nx + (tx * kTileX + r % kTileX));
        }
        label[((size_t)z * ny + y) * nx + x] = out;
    }
}

// ---- 2: union by lowest index on label[].  label[] is a forest: label[i] <= i, a root has label[r] == r, parents only decrease, and every value a
// cell ever held is a cell of its component.  Loads may be stale (another workgroup's atomic is not seen by a cached line): a stale value is an earlier
// parent, still a cell of the component above the root, so a walk over stale values ends at a cell of the component.  A link is decided by what the atomic
// returns: atomicMin(&label[a], b) with a > b returned a -> a was a root and now hangs under b; it returned something else -> a had the parent `old`
// already (label[a] is now min(old, b), both of the component), and old and b remain to be united: nothing is lost.  a + b decreases every round.
__device__ __forceinline__ int32_t cc_find(const int32_t* label, int32_t x, uint32_t* flag) {
    for (uint32_t it = 0; it < kCcWalkCap; ++it) { const int32_t p = cc_load(label + x); if (p >= x) return x; x = p; }
    cc_fail(flag); return x;
}
__device__ __forceinline__ void cc_union(int32_t* label, int32_t a, int32_t b, uint32_t* flag) {
    for (uint32_t it = 0; it < kCcUnionCap; ++it) {
        a = cc_find(label, a, flag); b = cc_find(label, b, flag);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(&label[a], b);
        if (old == a) return;
        a = old;
    }
    cc_fail(flag);
}
template <int CONN> __global__ void __launch_bounds__(256) k_cc_merge(uint32_t nx, uint32_t ny, uint32_t nz, int32_t* __restrict__ label,
        uint32_t* __restrict__ flag) {
    const uint32_t n = nx * ny * nz, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Cell c = split(i, nx, ny); const uint32_t x = c.x, y = c.y, z = c.z;
    // only a cell on a low face of its tile, or next to a tile's side in x or y, has a lower neighbour in another tile
    if ((x % kTileX) != 0 && (x % kTileX) != kTileX - 1 && (y % kTileY) != 0 && (y % kTileY) != kTileY - 1 && (z % kTileZ) != 0) return;
    if (label[i] < 0) return;
    cc_lower_neighbours<CONN>([&](int dx, int dy, int dz) {
        const int X = (int)x + dx, Y = (int)y + dy, Z = (int)z + dz;
        if (X < 0 || X >= (int)nx || Y < 0 || Y >= (int)ny || Z < 0) return;
        if ((uint32_t)X / kTileX == x / kTileX && (uint32_t)Y / kTileY == y / kTileY && (uint32_t)Z / kTileZ == z / kTileZ) return;      // stage 1 did it
        const uint32_t j = ((uint32_t)Z * ny + (uint32_t)Y) * nx + (uint32_t)X;
        if (label[j] >= 0) cc_union(label, (int32_t)i, (int32_t)j, flag);           // (in or out of the mask never changes: a plain load)
    });
}

// ---- 3, 4: block-wide exclusive scan of one counter
__device__ __forceinline__ uint32_t cc_block_excl_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t w = 0; w < nw; ++w) { const uint32_t s = lds[w]; if (w < wave) base += s; tot += s; }
    __syncthreads();
    total = tot;
    return base + inc - v;
}
// label[i] = the root.  (Another thread may read label[i] on its own walk while this one stores: it sees the earlier parent or the root, both on its way.)
__global__ void __launch_bounds__(256) k_cc_flatten(uint32_t n, int32_t* __restrict__ label, uint32_t* __restrict__ block_sums, uint32_t* __restrict__ flag) {
    __shared__ uint32_t lds[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t rep = 0;
    if (i < n) {
        const int32_t l = label[i];
        if (l >= 0) { const int32_t r = cc_find(label, l, flag); if (r != l) label[i] = r; rep = r == (int32_t)i ? 1u : 0u; }
    }
    uint32_t total; cc_block_excl_scan(rep, lds, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}
// single block: exclusive scan of the block sums in place; the total -> meta[0] (n_components)
__global__ void __launch_bounds__(1024) k_cc_scan(uint32_t* __restrict__ block_sums, uint32_t nb, uint32_t* __restrict__ meta) {
    __shared__ uint32_t lds[16];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += 1024u) {
        const uint32_t b = b0 + threadIdx.x, v = b < nb ? block_sums[b] : 0u; uint32_t total;
        const uint32_t ex = cc_block_excl_scan(v, lds, total);
        if (b < nb) block_sums[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) meta[0] = carry;
}
// the representatives: comp[rep] = its rank; the records below cap opened {rep, 0 cells, lo = INT_MAX, hi = INT_MIN}
__global__ void __launch_bounds__(256) k_cc_number(uint32_t n, const int32_t* __restrict__ label, const uint32_t* __restrict__ block_offs,
        int32_t* __restrict__ comp, int32_t* __restrict__ table, uint32_t cap) {
    __shared__ uint32_t lds[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool rep = i < n && label[i] == (int32_t)i;
    uint32_t total; const uint32_t rank = block_offs[blockIdx.x] + cc_block_excl_scan(rep ? 1u : 0u, lds, total);
    if (!rep) return;
    comp[i] = (int32_t)rank;
    if (table && rank < cap) {
        int32_t* t = table + 8 * (size_t)rank;
        t[0] = (int32_t)i; t[1] = 0; t[2] = t[3] = t[4] = INT_MAX; t[5] = t[6] = t[7] = INT_MIN;
    }
}
// a count and a box into component c's record: seven atomics (they commute)
__device__ __forceinline__ void cc_send(int32_t* table, int32_t c, uint32_t cells, int32_t lx, int32_t ly, int32_t lz, int32_t hx, int32_t hy, int32_t hz) {
    int32_t* t = table + 8 * (size_t)c;
    atomicAdd(reinterpret_cast<uint32_t*>(t + 1), cells);
    atomicMin(t + 2, lx); atomicMin(t + 3, ly); atomicMin(t + 4, lz); atomicMax(t + 5, hx); atomicMax(t + 6, hy); atomicMax(t + 7, hz);
}
// the same into the workgroup's gathering table in LDS: kCcSlots records {component (-1: free), cells, lo, hi}, open addressing with at most kCcProbes
// probes; a run that finds no slot goes to memory directly
constexpr uint32_t kCcTablePer = 16, kCcSlots = 128, kCcProbes = 8;
__device__ __forceinline__ void cc_gather(int32_t (*slot)[8], int32_t* table, int32_t c, uint32_t cells, int32_t lx, int32_t ly, int32_t lz, int32_t hx,
        int32_t hy, int32_t hz) {
    uint32_t h = ((uint32_t)c * 2654435761u) >> 25;
    static_assert(kCcSlots == 128, "the hash keeps 7 bits");
    for (uint32_t p = 0; p < kCcProbes; ++p, h = (h + 1u) & (kCcSlots - 1u)) {
        const int32_t k = atomicCAS(&slot[h][0], -1, c);
        if (k != -1 && k != c) continue;
        int32_t* t = slot[h];
        atomicAdd(reinterpret_cast<uint32_t*>(t + 1), cells);
        atomicMin(t + 2, lx); atomicMin(t + 3, ly); atomicMin(t + 4, lz); atomicMax(t + 5, hx); atomicMax(t + 6, hy); atomicMax(t + 7, hz);
        return;
    }
    cc_send(table, c, cells, lx, ly, lz, hx, hy, hz);
}
// comp of every cell; the records' cells, lo and hi.  Atomics on one record run at the rate of one address (a component of 2 M cells sent wave by wave took
// 2.6 ms of the first version), so they are gathered first: a workgroup takes kCcTablePer x 256 consecutive cells, a thread every 256th of them and keeps
// a run (component, count, box) in registers; a run that ends goes into the workgroup's table in LDS, and the table's used slots go to memory at the end:
// seven atomics per component and 4 096 cells.
__global__ void __launch_bounds__(256) k_cc_table(uint32_t nx, uint32_t ny, uint32_t nz, const int32_t* __restrict__ label, int32_t* __restrict__ comp,
        int32_t* __restrict__ table, uint32_t cap) {
    __shared__ int32_t slot[kCcSlots][8];
    const uint32_t n = nx * ny * nz, tid = threadIdx.x;
    if (tid < kCcSlots) {
        int32_t* t = slot[tid];
        t[0] = -1; t[1] = 0; t[2] = t[3] = t[4] = INT_MAX; t[5] = t[6] = t[7] = INT_MIN;
    }
    __syncthreads();
    int32_t cur = -1, lx = INT_MAX, ly = INT_MAX, lz = INT_MAX, hx = INT_MIN, hy = INT_MIN, hz = INT_MIN; uint32_t cnt = 0;
    for (uint32_t k = 0; k < kCcTablePer; ++k) {
        const uint32_t i = (blockIdx.x * kCcTablePer + k) * 256u + tid;
        if (i >= n) break;
        const int32_t l = label[i];
        const int32_t c = l >= 0 ? comp[l] : -1;                                    // (a representative reads and rewrites its own rank)
        comp[i] = c;
        if (table == nullptr || c < 0 || (uint32_t)c >= cap) continue;
        if (c != cur) {
            if (cur >= 0) cc_gather(slot, table, cur, cnt, lx, ly, lz, hx, hy, hz);
            cur = c; cnt = 0; lx = ly = lz = INT_MAX; hx = hy = hz = INT_MIN;
        }
        const Cell at = split(i, nx, ny); const int32_t x = (int32_t)at.x, y = (int32_t)at.y, z = (int32_t)at.z;
        ++cnt; lx = min(lx, x); ly = min(ly, y); lz = min(lz, z); hx = max(hx, x); hy = max(hy, y); hz = max(hz, z);
    }
    if (cur >= 0) cc_gather(slot, table, cur, cnt, lx, ly, lz, hx, hy, hz);
    __syncthreads();
    if (tid < kCcSlots && slot[tid][0] >= 0) {
        const int32_t* t = slot[tid];
        cc_send(table, t[0], (uint32_t)t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    }
}

// the traversable cells of a clearance field: occ = dist > clearance (a NaN dist does not occur: dist is a root of a sum of squares)
__global__ void __launch_bounds__(256) k_cc_clear_mask(uint32_t n, const float* __restrict__ dist, float clearance, uint8_t* __restrict__ occ) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) occ[i] = dist[i] > clearance ? 1 : 0;
}

// the result home in one copy: words [0, n_words) of src -> dst, of the table's words (from table_word on, 8 per record, table_cap records) only those of
// the records that were written, c < min(n_components, cap)
__global__ void __launch_bounds__(256) k_cc_home(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t n_words, uint32_t table_word,
        uint32_t table_cap, const uint32_t* __restrict__ meta) {
    const uint32_t used = min(meta[0], table_cap);
    for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += gridDim.x * blockDim.x) {
        if (w >= table_word + 8u * used && w < table_word + 8u * table_cap) continue;
        dst[w] = src[w];
    }
}

size_t components_scan_words(uint32_t n) { return (n + 255u) / 256u + 1u; }

void launch_components(hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, int32_t* label, int32_t* comp, uint32_t* scan,
        mon_lattice_component* table, uint32_t cap, uint32_t* meta) {
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny, nz = (uint32_t)g.nz, n = nx * ny * nz, nb = (n + 255u) / 256u;
    const Tiles tl = tiles(g);
    const dim3 cells(nb), b(256);
    uint32_t* flag = meta + 1;
    int32_t* t = reinterpret_cast<int32_t*>(table);
    (void)hipMemsetAsync(meta, 0, 2 * sizeof(uint32_t), s);
    dispatch_connectivity(connectivity, [&](auto conn) {
        hipLaunchKernelGGL(k_cc_local<conn.value>, dim3(tl.n()), b, 0, s, occ, nx, ny, nz, tl.x, tl.y, label, flag);
        hipLaunchKernelGGL(k_cc_merge<conn.value>, cells, b, 0, s, nx, ny, nz, label, flag);
    });
    hipLaunchKernelGGL(k_cc_flatten, cells, b, 0, s, n, label, scan, flag);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, s, scan, nb, meta);
    hipLaunchKernelGGL(k_cc_number, cells, b, 0, s, n, label, scan, comp, t, cap);
    hipLaunchKernelGGL(k_cc_table, dim3((n + 256u * kCcTablePer - 1u) / (256u * kCcTablePer)), b, 0, s, nx, ny, nz, label, comp, t, cap);
}
void launch_components_clear_mask(hipStream_t s, uint32_t n, const float* dist, float clearance, uint8_t* occ) {
    hipLaunchKernelGGL(k_cc_clear_mask, dim3((n + 255u) / 256u), dim3(256), 0, s, n, dist, clearance, occ);
}
void launch_components_home(hipStream_t s, const uint32_t* src, uint32_t* dst, uint32_t n_words, uint32_t table_word, uint32_t table_cap, const uint32_t* meta) {
    const uint32_t blocks = std::min((n_words + 255u) / 256u, 2048u);
    hipLaunchKernelGGL(k_cc_home, dim3(blocks), dim3(256), 0, s, src, dst, n_words, table_word, table_cap, meta);
}

}  // namespace mon
