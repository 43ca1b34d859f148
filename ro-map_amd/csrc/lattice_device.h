// lattice_device.h -- what the kernels over a lattice's cells share (kernels_components.hip, kernels_paths.hip): the tile a workgroup takes, how many tiles
// cover a lattice, a flat index split into its coordinates, which neighbours a connectivity admits, and the connectivity as a compile-time constant.
#pragma once
#include <cstdint>
#include <type_traits>
#include "model.h"

namespace mon {
// A workgroup's tile: 32 x 8 x 4 cells, thread t the column (t % 32, t / 32).  The path sweeps raise flags per tile of the labelling's shape: one tile.
constexpr uint32_t kTileX = 32, kTileY = 8, kTileZ = 4, kTileCells = kTileX * kTileY * kTileZ;
struct Tiles { uint32_t x, y, z; uint32_t n() const { return x * y * z; } };
inline Tiles tiles(const Lattice& g) { return { ((uint32_t)g.nx + kTileX - 1u) / kTileX, ((uint32_t)g.ny + kTileY - 1u) / kTileY, ((uint32_t)g.nz + kTileZ - 1u) / kTileZ }; }
// flat index i = (z * ny + y) * nx + x, x fastest: of a cell in its lattice, of a tile among the tiles
struct Cell { uint32_t x, y, z; };
__device__ __forceinline__ Cell split(uint32_t i, uint32_t nx, uint32_t ny) { return { i % nx, (i / nx) % ny, i / (nx * ny) }; }
// connectivity 6 / 18 / 26 admits the moves whose |dx| + |dy| + |dz| is 1 / at most 2 / at most 3
template <int CONN> __host__ __device__ __forceinline__ constexpr bool admits(int dx, int dy, int dz) {
    const int m = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
    return m != 0 && m <= (CONN == 6 ? 1 : CONN == 18 ? 2 : 3);
}
// f(std::integral_constant<int, connectivity>): connectivity is 6, 18 or 26 (checked by the caller)
template <class F> void dispatch_connectivity(int connectivity, F&& f) {
    switch (connectivity) {
        case 6:  f(std::integral_constant<int, 6>{}); break;
        case 18: f(std::integral_constant<int, 18>{}); break;
        default: f(std::integral_constant<int, 26>{}); break;
    }
}
}  // namespace mon
