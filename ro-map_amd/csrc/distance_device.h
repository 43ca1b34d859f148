// distance_device.h -- what the passes along a lattice axis share (k_distance_pass, kernels_distance.hip; k_surface_line_pass,
// kernels_signed_distance.hip): the block shape, the block-wide maximum behind the pruning bound, and one axis's lines and tile as a launch sees them.
#pragma once
#include <algorithm>
#include "model.h"

namespace mon {

// A line is cut into tiles of R = 2^logR cells; a workgroup owns a block of kDistTile cells, R along the lines by C = kDistTile / R lines side by side,
// and every thread kDistOut of them, all on one line, in registers.  Input tiles of the same shape go through LDS one at a time.
constexpr uint32_t kDistTile = 2048, kDistOut = kDistTile / 256;
static_assert(kDistTile <= 4096, "a line tile holds at most 4 096 cells (a line may be 2^22 long: it is never held whole)");
static_assert(kDistOut * 256 == kDistTile && kDistOut >= 1, "every thread owns kDistOut cells of the block");

// One axis of a lattice as a pass walks it, and the pass's grid
struct DistAxis {
    uint32_t n, m, stride;                                      // cells per line, lines, elements between two cells of a line
    uint32_t cw, cs;                                            // line c begins at element (c / cw) * cs + c % cw
    uint32_t logR, rows_fast;                                   // the tile; rows_fast: consecutive threads take consecutive cells of a line (the x axis)
    float step;
    uint32_t blocks() const { const uint32_t R = 1u << logR, C = kDistTile >> logR; return ((m + C - 1u) / C) * ((n + R - 1u) / R); }
};
inline uint32_t dist_ceil_log2(uint32_t x) { uint32_t l = 0; while ((1u << l) < x) ++l; return l; }
inline DistAxis dist_axis(const Lattice& g, int ax) {
    const uint32_t nx = (uint32_t)g.nx, ny = (uint32_t)g.ny, nz = (uint32_t)g.nz;
    const uint32_t len[3] = { nx, ny, nz }, lines[3] = { ny * nz, nx * nz, nx * ny }, stride[3] = { 1u, nx, nx * ny };
    const uint32_t cw[3] = { 1u, nx, nx * ny }, cs[3] = { nx, nx * ny, 0u };
    DistAxis a{};
    a.n = len[ax]; a.m = lines[ax]; a.stride = stride[ax]; a.cw = cw[ax]; a.cs = cs[ax]; a.step = g.step[ax];
    a.rows_fast = ax == 0 ? 1u : 0u;
    // x: the tile as long as the line allows (at least kDistOut rows: a thread's cells are rows of one line); y, z: up to 64 lines side by side
    a.logR = ax == 0 ? std::min(std::max(dist_ceil_log2(a.n), dist_ceil_log2(kDistOut)), dist_ceil_log2(kDistTile))
                     : dist_ceil_log2(kDistTile) - std::min(dist_ceil_log2(a.m), 6u);
    return a;
}

#if defined(__HIPCC__)
// the largest x of the workgroup (x >= 0, no NaN); `red`: four floats of LDS.  Two barriers.
__device__ __forceinline__ float dist_block_max(float x, float* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return x;
}
#endif

}  // namespace mon
