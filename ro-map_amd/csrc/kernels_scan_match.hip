// kernels_scan_match.hip -- scan end points scored against a device-resident distance field under many poses (mon_dist_field_match,
// mon_dist_field_register).  The rule is in include/mon_core.h: per pose and point the field's sample and gradient at the posed point, a
// Huber weight, and the 21 + 6 + 1 terms of the Gauss-Newton normal equations and the cost, each summed over the points by ONE pairwise tree in ascending
// index, padded with +0 to a power of two.
//   k_scan_match<NORMAL>  block (c, h): the run of kScanMatchChunk = 1 024 consecutive points c of pose h, four consecutive points to a lane, summed by
//                         fd_block_row (field_sample_device.h).  The block's row of kScanMatchRow = 32 words goes to part[h][c]: 21 A terms (row-major
//                         upper triangle), 6 b terms, the cost, n_inside, n_inlier, 0, 0.  NORMAL false: the last five columns only; the others are +0.
//   k_scan_fold           block (g, h): kScanMatchFold = 64 consecutive rows of pose h folded to one by the same tree in LDS (fd_lds_fold per column),
//                         padded with +0; it returns -0 as +0 as the rule asks.
// The two counts ride the same tree as floats: a count is at most 2^20 and so exact.  The pose
// and the pivot are uniform per block (scalar loads).  Plain C++, vector stores only, no atomics, no scratch; no workgroup waits for another; every loop is
// bounded by an argument the host has checked.
#include "field_sample_device.h"

namespace mon {

constexpr int kSmA = 21, kSmB = 6;                                                  // columns: A | b | cost, n_inside, n_inlier

// the terms of one point into t[NV] (NV = 30, or 3 without the normal equations); a padding point (!live) gives +0 throughout
template <bool NORMAL> __device__ __forceinline__ void sm_point(const DistFieldView& F, const float* __restrict__ pose, float cx, float cy, float cz,
        float huber, float outside, bool live, float px, float py, float pz, float* __restrict__ t) {
    constexpr int NV = NORMAL ? kSmA + kSmB + 3 : 3, R = NV - 3;
#pragma unroll
    for (int j = 0; j < NV; ++j) t[j] = 0.f;
    if (live) {
        const Fd3 q = fd_centre<true>(pose, px, py, pz);
        float d = outside, g[3] = { 0.f, 0.f, 0.f };
        const bool in = fd_sample<NORMAL>(F, q.x, q.y, q.z, d, g);
        const float m = fabsf(d);
        const bool quad = m <= huber;
        const float w = quad ? 1.f : __fdiv_rn(huber, m);
        t[R] = quad ? __fmul_rn(d, d) : __fmul_rn(huber, __fsub_rn(__fmul_rn(2.f, m), huber));
        if (in) {
            t[R + 1] = 1.f; t[R + 2] = quad ? 1.f : 0.f;
            if (NORMAL) {
                const float ax = __fsub_rn(q.x, cx), ay = __fsub_rn(q.y, cy), az = __fsub_rn(q.z, cz);
                const float J[6] = { g[0], g[1], g[2], __fsub_rn(__fmul_rn(ay, g[2]), __fmul_rn(az, g[1])), __fsub_rn(__fmul_rn(az, g[0]), __fmul_rn(ax, g[2])),
                                     __fsub_rn(__fmul_rn(ax, g[1]), __fmul_rn(ay, g[0])) };
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const float wj = __fmul_rn(w, J[i]);
#pragma unroll
                    for (int j = i; j < 6; ++j) t[i * 6 - (i * (i - 1)) / 2 + (j - i)] = __fmul_rn(wj, J[j]);
                    t[kSmA + i] = __fmul_rn(wj, d);
                }
            }
        }
    }
}

template <bool NORMAL> __global__ void __launch_bounds__(256) k_scan_match(DistFieldView F, ScanMatchArgs a, float* __restrict__ part) {
    constexpr int NV = NORMAL ? kSmA + kSmB + 3 : 3;
    const uint32_t chunk = blockIdx.x, h = blockIdx.y;
    const float* __restrict__ pose = a.poses + 16 * (size_t)h;
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (a.pivots != nullptr) { cx = a.pivots[3 * (size_t)h]; cy = a.pivots[3 * (size_t)h + 1]; cz = a.pivots[3 * (size_t)h + 2]; }
    // the lane's four consecutive points: 48 bytes at a multiple of 48 (the host keeps the points 16-byte aligned), or what is left of them
    const uint32_t i0 = chunk * kScanMatchChunk + threadIdx.x * 4u;
    float p[12];
    if (i0 + 4u <= a.n) {
        const float4* v = reinterpret_cast<const float4*>(a.points + 3 * (size_t)i0);
        const float4 v0 = v[0], v1 = v[1], v2 = v[2];
        p[0] = v0.x; p[1] = v0.y; p[2] = v0.z; p[3] = v0.w; p[4] = v1.x; p[5] = v1.y; p[6] = v1.z; p[7] = v1.w; p[8] = v2.x; p[9] = v2.y; p[10] = v2.z;
        p[11] = v2.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[3 * k + c] = i0 + (uint32_t)k < a.n ? a.points[3 * (size_t)(i0 + (uint32_t)k) + c] : 0.f;
    }
    fd_block_row<NV>([&](int k, float* __restrict__ t) {
        sm_point<NORMAL>(F, pose, cx, cy, cz, a.huber, a.outside, i0 + (uint32_t)k < a.n, p[3 * k], p[3 * k + 1], p[3 * k + 2], t); },
        part + ((size_t)h * gridDim.x + chunk) * kScanMatchRow);
}

// in[pose][n_in][32] -> out[pose][gridDim.x][width]: block (g, h) folds rows 64 g .. of pose h and writes the columns first .. first + width - 1
__global__ void __launch_bounds__(256) k_scan_fold(const float* __restrict__ in, uint32_t n_in, float* __restrict__ out, uint32_t first, uint32_t width) {
    __shared__ float v_s[kScanMatchFold][kScanMatchRow];
    const uint32_t col = threadIdx.x & 31u, sub = threadIdx.x >> 5, g = blockIdx.x, h = blockIdx.y;
    const uint32_t base = g * kScanMatchFold, cnt = min(kScanMatchFold, n_in - base);
    uint32_t pad = 1;
    while (pad < cnt) pad <<= 1;                                                    // (at most 64)
    for (uint32_t r = sub; r < pad; r += 8u) v_s[r][col] = r < cnt ? in[((size_t)h * n_in + base + r) * kScanMatchRow + col] : 0.f;
    __syncthreads();
    fd_lds_fold(&v_s[0][col], kScanMatchRow, pad, sub, 8u);
    if (sub == 0u && col >= first && col < first + width)
        out[((size_t)h * gridDim.x + g) * width + (col - first)] = __fadd_rn(v_s[0][col], 0.f);      // (-0 leaves as +0)
}

static uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }
// part rows of the match launch, then those of a first fold where the chunks exceed one fold's reach
size_t scan_match_scratch(uint32_t n, uint32_t n_pose) {
    const uint32_t chunks = ceil_div(n, kScanMatchChunk);
    return (size_t)n_pose * kScanMatchRow * ((size_t)chunks + (chunks > kScanMatchFold ? ceil_div(chunks, kScanMatchFold) : 0u));
}
void launch_scan_match(hipStream_t s, const float* D, const Lattice& g, const ScanMatchArgs& a, bool normal, float* scratch, float* rows) {
    const DistFieldView F = dist_field_view(D, g);
    uint32_t n_in = ceil_div(a.n, kScanMatchChunk);
    const dim3 grid(n_in, a.n_pose);
    if (normal) hipLaunchKernelGGL((k_scan_match<true>), grid, dim3(256), 0, s, F, a, scratch);
    else hipLaunchKernelGGL((k_scan_match<false>), grid, dim3(256), 0, s, F, a, scratch);
    // the whole row, or without the normal equations the cost, the two counts and one 0
    launch_scan_fold(s, scratch, n_in, a.n_pose, rows, normal ? 0u : (uint32_t)(kSmA + kSmB), normal ? kScanMatchRow : kScanMatchLite);
}
// scratch[n_pose][n_in][32], the part rows of a launch (scan_match_scratch's layout: the rows of a first fold go behind them) -> rows[n_pose][width], the
// columns first .. first + width - 1 of each pose's folded row
void launch_scan_fold(hipStream_t s, float* scratch, uint32_t n_in, uint32_t n_pose, float* rows, uint32_t first, uint32_t width) {
    const float* in = scratch;
    if (n_in > kScanMatchFold) {                                                    // (once: n <= 2^20 gives at most 1 024 chunks, 16 rows after it)
        float* mid = scratch + (size_t)n_pose * kScanMatchRow * n_in;
        const uint32_t n_out = ceil_div(n_in, kScanMatchFold);
        hipLaunchKernelGGL(k_scan_fold, dim3(n_out, n_pose), dim3(256), 0, s, in, n_in, mid, 0u, kScanMatchRow);
        in = mid; n_in = n_out;
    }
    hipLaunchKernelGGL(k_scan_fold, dim3(1, n_pose), dim3(256), 0, s, in, n_in, rows, first, width);
}

}  // namespace mon
