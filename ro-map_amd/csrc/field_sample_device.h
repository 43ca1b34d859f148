// field_sample_device.h -- the sample of a device-resident distance field at a world point and a body point under a pose, as every kernel that asks a
// mon_dist_field takes them (kernels_clearance.hip, kernels_scan_match.hip, kernels_field_trace.hip).  The rule is in include/mon_core.h: trilinear
// interpolation with every fp32 operation rounded on its own (nothing is contracted), the gradient from the same intermediates.  The corners of a cell come
// as four 8-byte loads where n_x > 1 (the two x-neighbours are adjacent words; the address is 4-byte aligned only).  Behind the sample: the two steps of the
// calls' summation tree that more than one kernel takes (fd_block_row, fd_lds_fold).
#pragma once
#include <cmath>
#include "model.h"

namespace mon {

typedef float FdPair __attribute__((ext_vector_type(2), aligned(4)));                 // two adjacent words, loaded at once
// one axis of a point: inside, the cell and the fraction.  An axis of one cell is neither interpolated nor range-checked.
struct FdAxis { int i; float f; bool in; };
__device__ __forceinline__ FdAxis fd_axis(float p, float o, float s, int n) {
    FdAxis a{ 0, 0.f, true };
    if (n > 1) {
        const float g = __fdiv_rn(__fsub_rn(p, o), s);
        a.in = g >= 0.f && g <= (float)(n - 1);                                     // (a NaN fails)
        const float gi = a.in ? g : 0.f;
        a.i = min((int)floorf(gi), n - 2);
        a.f = __fsub_rn(gi, (float)a.i);
    }
    return a;
}
__device__ __forceinline__ float fd_lerp(float a, float d, float f) { return __fadd_rn(a, __fmul_rn(f, d)); }      // a + f * (b - a), d = fl(b - a)
// The field at p.  false: p is outside on some axis (d and g are not written).  GRAD: the gradient in world units, 0 along an axis of one cell.
template <bool GRAD> __device__ __forceinline__ bool fd_sample(const DistFieldView& F, float px, float py, float pz, float& d, float* g) {
    const FdAxis ax = fd_axis(px, F.o[0], F.s[0], F.nx), ay = fd_axis(py, F.o[1], F.s[1], F.ny), az = fd_axis(pz, F.o[2], F.s[2], F.nz);
    if (!(ax.in && ay.in && az.in)) return false;
    const size_t base = ((size_t)az.i * (size_t)F.ny + (size_t)ay.i) * (size_t)F.nx + (size_t)ax.i;
    const size_t dy = F.ny > 1 ? (size_t)F.nx : 0, dz = F.nz > 1 ? (size_t)F.nx * (size_t)F.ny : 0;
    const size_t at[4] = { base, base + dy, base + dz, base + dy + dz };            // (j, k) = (0, 0), (1, 0), (0, 1), (1, 1)
    float c[4], e[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float lo, hi;
        if (F.nx > 1) { const FdPair v = *reinterpret_cast<const FdPair*>(F.D + at[m]); lo = v.x; hi = v.y; }
        else { lo = F.D[at[m]]; hi = lo; }
        e[m] = __fsub_rn(hi, lo);
        c[m] = fd_lerp(lo, e[m], ax.f);
    }
    const float h0 = __fsub_rn(c[1], c[0]), h1 = __fsub_rn(c[3], c[2]);
    const float c0 = fd_lerp(c[0], h0, ay.f), c1 = fd_lerp(c[2], h1, ay.f);
    const float w = __fsub_rn(c1, c0);
    d = fd_lerp(c0, w, az.f);
    if (GRAD) {
        const float e0 = fd_lerp(e[0], __fsub_rn(e[1], e[0]), ay.f), e1 = fd_lerp(e[2], __fsub_rn(e[3], e[2]), ay.f);
        g[0] = F.nx > 1 ? __fdiv_rn(fd_lerp(e0, __fsub_rn(e1, e0), az.f), F.s[0]) : 0.f;
        g[1] = F.ny > 1 ? __fdiv_rn(fd_lerp(h0, __fsub_rn(h1, h0), az.f), F.s[1]) : 0.f;
        g[2] = F.nz > 1 ? __fdiv_rn(w, F.s[2]) : 0.f;
    }
    return true;
}

// The centre of sphere b at waypoint `way` (3 floats: a position; 16: a row-major 4 x 4 matrix, its last row ignored)
struct Fd3 { float x, y, z; };
template <bool POSE> __device__ __forceinline__ Fd3 fd_centre(const float* __restrict__ way, float bx, float by, float bz) {
    if (!POSE) return Fd3{ __fadd_rn(way[0], bx), __fadd_rn(way[1], by), __fadd_rn(way[2], bz) };
    Fd3 c;
    c.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(way[0], bx), __fmul_rn(way[1], by)), __fmul_rn(way[2], bz)), way[3]);
    c.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(way[4], bx), __fmul_rn(way[5], by)), __fmul_rn(way[6], bz)), way[7]);
    c.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(way[8], bx), __fmul_rn(way[9], by)), __fmul_rn(way[10], bz)), way[11]);
    return c;
}

// ---- the two shared steps of the rule's pairwise tree (padded with +0 to a power of two, v'[i] = fl(v[2 i] + v[2 i + 1]) level by level).
// The block row, for a block of 256 threads over kScanMatchChunk = 1 024 consecutive items: item(k, t) writes the NV terms of this lane's item k = 0 .. 3 (a
// padding item gives +0 throughout).  A lane trees its four consecutive items in registers; lanes hold consecutive subtrees, so __shfl_down by 1, 2 .. 32
// continues the same tree (level m pairs lane l with lane l + m; lane 0 ends with the wave's node over 256 items); the four waves combine through LDS.
// row[kScanMatchRow]: +0 but for the NV sums in the columns 32 - 2 - NV .. 29 (the row's last two words are 0).  A row is a node of the tree whatever the
// chunk size: the levels above the items' own power of two add +0, which changes no bit of a sum except -0 (k_scan_fold returns -0 as +0).
template <int NV, typename Item> __device__ __forceinline__ void fd_block_row(Item item, float* __restrict__ row) {
    constexpr int FIRST = (int)kScanMatchRow - 2 - NV;
    __shared__ float wave_s[4][NV];
    float s[NV], t[NV], u[NV];
    item(0, s);
    item(1, t);
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = __fadd_rn(s[j], t[j]);
    item(2, t);
    item(3, u);
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = __fadd_rn(s[j], __fadd_rn(t[j], u[j]));
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int j = 0; j < NV; ++j) s[j] = __fadd_rn(s[j], __shfl_down(s[j], m));
    if ((threadIdx.x & 63u) == 0u)
#pragma unroll
        for (int j = 0; j < NV; ++j) wave_s[threadIdx.x >> 6][j] = s[j];
    __syncthreads();
    if (threadIdx.x < kScanMatchRow) {
        const int c = (int)threadIdx.x - FIRST;
        float r = 0.f;
        if (c >= 0 && c < NV) r = __fadd_rn(__fadd_rn(wave_s[0][c], wave_s[1][c]), __fadd_rn(wave_s[2][c], wave_s[3][c]));
        row[threadIdx.x] = r;
    }
}
// The tree over v[0], v[stride] .. v[(pad - 1) * stride] in LDS (pad a power of two), in place, by `n_who` threads of which this one is `who`; the sum
// ends in v[0].  Level m keeps its sums at the multiples of 2 m and reads nothing another thread writes; one barrier per level, which every thread of the
// block reaches: pad is uniform.  The caller has synchronised after writing v.
__device__ __forceinline__ void fd_lds_fold(float* v, uint32_t stride, uint32_t pad, uint32_t who, uint32_t n_who) {
    for (uint32_t m = 1; m < pad; m <<= 1) {
        for (uint32_t i = who * 2u * m; i < pad; i += n_who * 2u * m) v[i * stride] = __fadd_rn(v[i * stride], v[(i + m) * stride]);
        __syncthreads();
    }
}

}  // namespace mon
