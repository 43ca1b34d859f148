// kernels_paths.hip -- shortest-path cost fields over a lattice (mon_shortest_paths, mon_scene_paths_lattice): per passable cell the least
// fp32 left fold of the move weights over all walks from a seed (cost), and the neighbour to step to (next).  The rule is in include/mon_core.h.
//   1  k_paths_init, k_paths_seed   cost = +inf; 0 at every passable seed, and sweep 0's flag of every tile that sees the seed
//   2  k_paths_sweep<CONN, COST>    a launch per sweep, a workgroup per tile of 32 x 8 x 4 cells (lattice_device.h).  A tile without a flag returns.  A
//                                   flagged one stages its cells and a one-cell halo in LDS, relaxes its own cells to the fixed point under that halo,
//                                   stores the cells that fell and raises the next sweep's flag of every neighbour tile that can see one of them
//   3  k_paths_finish<CONN, COST>   a thread per cell: next by the header's rule on the untruncated field, then the max_cost cut
// cost[] only falls, and every value a cell ever holds is the fold of a real walk from a seed: an upper bound of the answer.  A halo word read while its
// owner is at work is therefore late at worst, never wrong (4-byte stores do not tear), and whoever lowers a cell that a neighbour tile can see has raised
// that tile's flag for the next launch, which sees every store of this one.  The flags are two rows of a byte per tile: sweep s reads row s & 1, a tile
// clears its own byte there and raises bytes of the other row only, so no byte is raised and cleared in one launch.  A sweep that raises no flag leaves the
// other row empty: the fixed point, which is the answer whatever the order of the relaxations was (fp32 addition is monotone and fl(c + w) >= c for
// w >= 0).  No workgroup waits for another; the tile's rounds are bounded (a tile that ran into the bound would raise its own flag again); plain C++, vector
// stores only, no atomics, no scratch.
#include <cmath>
#include "lattice_device.h"

namespace mon {

constexpr uint32_t kPtPer = kTileCells / 256;
constexpr uint32_t kPtHX = kTileX + 2, kPtHY = kTileY + 2, kPtHZ = kTileZ + 2, kPtHalo = kPtHX * kPtHY * kPtHZ;      // 34 x 10 x 6 = 2 040 words
static_assert(kPtPer == kTileZ && kTileX * kTileY == 256, "a thread owns the column (lx, ly) of its tile");
// Rounds of a tile.  Under the values of its halo a cell's fixed point is the fold of a walk inside the tile from a halo cell or from a cell that keeps its
// value; a least walk need not visit a cell twice (costs never fall along a walk), so it has at most kTileCells moves, and round r has settled the walks of r
// moves (a relaxation that reads a neighbour's newer value is only earlier).  One more round sees that nothing changed.
constexpr uint32_t kPtRoundCap = kTileCells + 1;

__device__ __forceinline__ float pt_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// f(dx, dy, dz) for every admitted neighbour, in ascending flat index
template <int CONN, class F> __device__ __forceinline__ void pt_neighbours(F&& f) {
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
                if (admits<CONN>(dx, dy, dz)) f(dx, dy, dz);
}
// The lengths of the moves by which axes they use: len[(dz != 0) * 4 + (dy != 0) * 2 + (dx != 0)] = sqrtf(((ax * ax) + (ay * ay)) + (az * az)), every
// operation rounded on its own; an axis the move does not use adds an exact +0, and (-s) * (-s) == s * s.  (sqrtf: the IEEE root, as k_distance_finish.)
struct PtLen { float v[8]; };
__device__ __forceinline__ PtLen pt_lengths(float sx, float sy, float sz) {
    const float x2 = __fmul_rn(sx, sx), y2 = __fmul_rn(sy, sy), z2 = __fmul_rn(sz, sz);
    PtLen l;
#pragma unroll
    for (int m = 0; m < 8; ++m) l.v[m] = sqrtf(__fadd_rn(__fadd_rn((m & 1) ? x2 : 0.f, (m & 2) ? y2 : 0.f), (m & 4) ? z2 : 0.f));
    return l;
}
__device__ __forceinline__ float pt_len(const PtLen& l, int dx, int dy, int dz) { return l.v[(dz != 0) * 4 + (dy != 0) * 2 + (dx != 0)]; }
// fl(cu + w(u, v)): w = len, or fl(len * fl(0.5 * fl(c[u] + c[v])))
template <bool COST> __device__ __forceinline__ float pt_step(float cu, float len, float mu, float mv) {
    const float w = COST ? __fmul_rn(len, __fmul_rn(0.5f, __fadd_rn(mu, mv))) : len;
    return __fadd_rn(cu, w);
}

// ---- 1
__global__ void __launch_bounds__(256) k_paths_init(uint32_t n, float* __restrict__ cost) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cost[i] = INFINITY;
}
// A seed's 0 is a cell that fell: the flags of sweep 0 go to every tile that sees it, the seed's own and those whose halo holds it (the tiles of the seed's
// 26 neighbours, whatever the connectivity: a tile flagged in vain finds nothing to do).  Duplicate seeds store the same words; a seed outside the mask
// contributes nothing.
__global__ void __launch_bounds__(256) k_paths_seed(const uint8_t* __restrict__ occ, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t tiles_x,
        uint32_t tiles_y, const int32_t* __restrict__ seeds, uint32_t n_seeds, float* __restrict__ cost, uint8_t* __restrict__ flags) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_seeds) return;
    const uint32_t i = (uint32_t)seeds[k];
    if (occ[i] == 0) return;
    const Cell at = split(i, nx, ny); const int x = (int)at.x, y = (int)at.y, z = (int)at.z;
    cost[i] = 0.f;
    for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
        const int X = x + dx, Y = y + dy, Z = z + dz;
        if (X < 0 || X >= (int)nx || Y < 0 || Y >= (int)ny || Z < 0 || Z >= (int)nz) continue;
        flags[(((uint32_t)Z / kTileZ) * tiles_y + (uint32_t)Y / kTileY) * tiles_x + (uint32_t)X / kTileX] = 1;
    }
}

// ---- 2.  cur: this sweep's flags, nxt: the next one's; raised: the word that says a flag of nxt was raised
template <int CONN, bool COST> __global__ void __launch_bounds__(256) k_paths_sweep(const uint8_t* __restrict__ occ, uint32_t nx, uint32_t ny, uint32_t nz,
        uint32_t tiles_x, uint32_t tiles_y, uint32_t tiles_z, float sx, float sy, float sz, const float* __restrict__ mult, float* cost, uint8_t* cur,
        uint8_t* nxt, uint32_t* __restrict__ raised) {
    __shared__ float c_s[kPtHalo];
    __shared__ float m_s[COST ? kPtHalo : 1];
    __shared__ uint32_t nb[27];
    const uint32_t tile = blockIdx.x;
    if (cur[tile] == 0) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / (tiles_x * tiles_y);   // (split() here reorders the halo's compares)
    // the tile and its halo; outside the lattice: +inf, which no relaxation lowers and from which nothing is reached
    for (uint32_t h = tid; h < kPtHalo; h += 256u) {
        const int X = (int)(tx * kTileX + h % kPtHX) - 1, Y = (int)(ty * kTileY + (h / kPtHX) % kPtHY) - 1, Z = (int)(tz * kTileZ + h / (kPtHX * kPtHY)) - 1;
        const bool in = X >= 0 && X < (int)nx && Y >= 0 && Y < (int)ny && Z >= 0 && Z < (int)nz;
        const size_t g = ((size_t)(in ? Z : 0) * ny + (size_t)(in ? Y : 0)) * nx + (size_t)(in ? X : 0);
        c_s[h] = in ? pt_load(cost + g) : INFINITY;
        if (COST) m_s[h] = in ? mult[g] : 0.f;
    }
    if (tid < 27u) nb[tid] = 0u;
    const uint32_t lx = tid % kTileX, ly = tid / kTileX, x = tx * kTileX + lx, y = ty * kTileY + ly;
    bool on[kPtPer]; float first[kPtPer];
#pragma unroll
    for (uint32_t q = 0; q < kPtPer; ++q) {
        const uint32_t z = tz * kTileZ + q;
        on[q] = x < nx && y < ny && z < nz && occ[((size_t)z * ny + y) * nx + x] != 0;
    }
    __syncthreads();                                                                // (every thread has read cur[tile])
    if (tid == 0) cur[tile] = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPtPer; ++q) first[q] = c_s[((q + 1u) * kPtHY + ly + 1u) * kPtHX + lx + 1u];
    const PtLen len = pt_lengths(sx, sy, sz);
    // A round: every passable cell of the tile takes the least of its value and fl(neighbour + w).  Only its owner stores a cell; a neighbour read while its
    // owner stores is the older or the newer value, both folds of real walks.  A round without a store read a state at rest: the fixed point.
    uint32_t round = 0;
    for (; round < kPtRoundCap; ++round) {
        bool changed = false;
#pragma unroll
        for (uint32_t q = 0; q < kPtPer; ++q) {
            if (!on[q]) continue;
            const int c = (int)(((q + 1u) * kPtHY + ly + 1u) * kPtHX + lx + 1u);
            const float old = c_s[c], mv = COST ? m_s[c] : 0.f;
            float best = old;
            pt_neighbours<CONN>([&](int dx, int dy, int dz) {
                const int u = c + (dz * (int)kPtHY + dy) * (int)kPtHX + dx;
                const float cand = pt_step<COST>(c_s[u], pt_len(len, dx, dy, dz), COST ? m_s[u] : 0.f, mv);
                if (cand < best) best = cand;
            });
            if (best < old) { c_s[c] = best; changed = true; }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // the cells that fell go to memory; a neighbour tile sees such a cell iff the cell lies on the face, edge or corner the two share (under CONN: a tile
    // offset of m axes is reached only by a move of at least m axes)
#pragma unroll
    for (uint32_t q = 0; q < kPtPer; ++q) {
        if (!on[q]) continue;
        const float v = c_s[((q + 1u) * kPtHY + ly + 1u) * kPtHX + lx + 1u];
        if (!(v < first[q])) continue;
        cost[((size_t)(tz * kTileZ + q) * ny + y) * nx + x] = v;
        const int bx = lx == 0 ? -1 : lx == kTileX - 1 ? 1 : 0, by = ly == 0 ? -1 : ly == kTileY - 1 ? 1 : 0, bz = q == 0 ? -1 : q == kTileZ - 1 ? 1 : 0;
#pragma unroll
        for (int m = 1; m < 8; ++m) {
            const int ox = (m & 1) ? bx : 0, oy = (m & 2) ? by : 0, oz = (m & 4) ? bz : 0;
            if (((m & 1) && bx == 0) || ((m & 2) && by == 0) || ((m & 4) && bz == 0)) continue;
            if (!admits<CONN>(ox, oy, oz)) continue;
            nb[(oz + 1) * 9 + (oy + 1) * 3 + (ox + 1)] = 1u;
        }
    }
    __syncthreads();                                                                // nb[] is complete
    if (round == kPtRoundCap && tid == 0) { nxt[tile] = 1; *raised = 1u; }          // (not reached, by the bound above; the tile would go on next sweep)
    if (tid < 27u && tid != 13u && nb[tid] != 0u) {
        const int X = (int)tx + (int)(tid % 3u) - 1, Y = (int)ty + (int)((tid / 3u) % 3u) - 1, Z = (int)tz + (int)(tid / 9u) - 1;
        if (X >= 0 && X < (int)tiles_x && Y >= 0 && Y < (int)tiles_y && Z >= 0 && Z < (int)tiles_z) {
            nxt[((uint32_t)Z * tiles_y + (uint32_t)Y) * tiles_x + (uint32_t)X] = 1;
            *raised = 1u;
        }
    }
}

// ---- 3.  next[v]: among the neighbours u of v in ascending flat index the first with cost[u] < cost[v] and fl(cost[u] + w(u, v)) == cost[v], on the
// untruncated field (a seed has cost 0 and nothing below it: -1 without a special case); then where !(cost <= max_cost): +inf and -1.  cost_out is another
// array than cost: the neighbours' untruncated values are still being read.
template <int CONN, bool COST> __global__ void __launch_bounds__(256) k_paths_finish(const uint8_t* __restrict__ occ, uint32_t nx, uint32_t ny, uint32_t nz,
        float sx, float sy, float sz, const float* __restrict__ mult, const float* __restrict__ cost, float max_cost, float* __restrict__ cost_out,
        int32_t* __restrict__ next) {
    const uint32_t n = nx * ny * nz, i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float cv = occ[i] != 0 ? cost[i] : INFINITY;
    int32_t to = -1;
    if (next != nullptr && cv < INFINITY && cv <= max_cost) {
        const Cell at = split(i, nx, ny); const int x = (int)at.x, y = (int)at.y, z = (int)at.z;
        const PtLen len = pt_lengths(sx, sy, sz);
        const float mv = COST ? mult[i] : 0.f;
        pt_neighbours<CONN>([&](int dx, int dy, int dz) {
            const int X = x + dx, Y = y + dy, Z = z + dz;
            if (to >= 0 || X < 0 || X >= (int)nx || Y < 0 || Y >= (int)ny || Z < 0 || Z >= (int)nz) return;
            const uint32_t u = ((uint32_t)Z * ny + (uint32_t)Y) * nx + (uint32_t)X;
            const float cu = cost[u];                                               // (+inf outside the mask: never below cv)
            if (cu < cv && pt_step<COST>(cu, pt_len(len, dx, dy, dz), COST ? mult[u] : 0.f, mv) == cv) to = (int32_t)u;
        });
    }
    if (!(cv <= max_cost)) { cv = INFINITY; to = -1; }
    cost_out[i] = cv;
    if (next != nullptr) next[i] = to;
}

// the scene call's multiplier: c = fl(1 + fl(soft_weight * fl(fmaxf(0, fl(soft_radius - dist)) / soft_radius))); 1 from soft_radius outward and at +inf
__global__ void __launch_bounds__(256) k_paths_soft(uint32_t n, const float* __restrict__ dist, float soft_radius, float soft_weight, float* __restrict__ mult) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mult[i] = __fadd_rn(1.f, __fmul_rn(soft_weight, __fdiv_rn(fmaxf(0.f, __fsub_rn(soft_radius, dist[i])), soft_radius)));
}

uint32_t paths_tiles(const Lattice& g) { return tiles(g).n(); }
void launch_paths_init(hipStream_t s, const uint8_t* occ, const Lattice& g, const int32_t* seeds, uint32_t n_seeds, float* cost, uint8_t* flags) {
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny, nz = (uint32_t)g.nz, n = nx * ny * nz; const Tiles tl = tiles(g);
    (void)hipMemsetAsync(flags, 0, 2 * (size_t)tl.n(), s);
    hipLaunchKernelGGL(k_paths_init, dim3((n + 255u) / 256u), dim3(256), 0, s, n, cost);
    hipLaunchKernelGGL(k_paths_seed, dim3((n_seeds + 255u) / 256u), dim3(256), 0, s, occ, nx, ny, nz, tl.x, tl.y, seeds, n_seeds, cost, flags);
}
// f(connectivity and "with a multiplier" as compile-time constants)
template <class F> static void paths_dispatch(int connectivity, bool cost, F&& f) {
    dispatch_connectivity(connectivity, [&](auto conn) { cost ? f(conn, std::true_type{}) : f(conn, std::false_type{}); });
}
void launch_paths_sweep(hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, const float* mult, float* cost, uint8_t* flags, uint32_t sweep,
        uint32_t* raised) {
    const Tiles tl = tiles(g);
    uint8_t* cur = flags + (sweep & 1u) * (size_t)tl.n(); uint8_t* nxt = flags + ((sweep + 1u) & 1u) * (size_t)tl.n();
    paths_dispatch(connectivity, mult != nullptr, [&](auto conn, auto with) {
        hipLaunchKernelGGL((k_paths_sweep<conn.value, with.value>), dim3(tl.n()), dim3(256), 0, s, occ, (uint32_t)g.nx, (uint32_t)g.ny, (uint32_t)g.nz, tl.x, tl.y,
                tl.z, g.step[0], g.step[1], g.step[2], mult, cost, cur, nxt, raised);
    });
}
void launch_paths_finish(hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, const float* mult, const float* cost, float max_cost,
        float* cost_out, int32_t* next) {
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny, nz = (uint32_t)g.nz;
    paths_dispatch(connectivity, mult != nullptr, [&](auto conn, auto with) {
        hipLaunchKernelGGL((k_paths_finish<conn.value, with.value>), dim3((nx * ny * nz + 255u) / 256u), dim3(256), 0, s, occ, nx, ny, nz, g.step[0], g.step[1],
                g.step[2], mult, cost, max_cost, cost_out, next);
    });
}
void launch_paths_soft(hipStream_t s, uint32_t n, const float* dist, float soft_radius, float soft_weight, float* mult) {
    hipLaunchKernelGGL(k_paths_soft, dim3((n + 255u) / 256u), dim3(256), 0, s, n, dist, soft_radius, soft_weight, mult);
}

}  // namespace mon
