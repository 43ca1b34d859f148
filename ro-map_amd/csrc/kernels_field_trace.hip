// kernels_field_trace.hip -- rays sphere-traced through a device-resident distance field under many poses (mon_dist_field_trace,
// mon_dist_field_beam_score).  The rule is in include/mon_core.h: a ray's origin and direction under the pose, a march whose step is
// relax x the sampled distance (at least step_min; step_outside until the lattice is entered), the crossing of the level eps between the last two samples,
// and for the beam score a Huber term on range - measured summed by ONE pairwise tree in ascending beam index, padded with +0 to a power of two.
//   k_field_trace<NORMAL>  block (c, h): the 256 consecutive rays c of pose h, a lane per ray: range, and where asked for status and steps, at
//                          [h * stride + ray]; NORMAL: one more sample, with its gradient, at the hit.  Consecutive rays are consecutive beams of a scan, so
//                          neighbouring lanes walk neighbouring cells and share 64-byte lines.  A wave runs as long as its slowest ray.
//   k_beam_terms           block (c, h): the run of kScanMatchChunk = 1 024 consecutive beams c of pose h, read from the ranges and statuses a trace launch
//                          left at stride (a multiple of 4), four consecutive beams to a lane, summed by fd_block_row (field_sample_device.h), as
//                          k_scan_match sums its points.  The block's row of kScanMatchRow = 32 words goes to part[h][c]: +0 but for the lite columns
//                          27 .. 30 = cost, n_valid, n_hit, 0.
// The rows are folded by k_scan_fold (kernels_scan_match.hip), launched as it is through launch_scan_fold.  The sample (fd_sample, fd_centre) is
// field_sample_device.h's too.  The pose is uniform per block (scalar loads).  Plain C++, vector stores only, no atomics, no scratch; no workgroup waits for
// another; every loop is bounded by an argument the host has checked: the march by max_steps.
#include "field_sample_device.h"

namespace mon {

typedef float FtPair __attribute__((ext_vector_type(2)));                           // two adjacent words of a ray record (24 bytes: 8-byte aligned)

// one ray of one pose: origin a, direction w (world), marched by the header's rule; g is written only where NORMAL
template <bool NORMAL> __device__ __forceinline__ void ft_march(const DistFieldView& F, const FieldTraceArgs& p, float ax, float ay, float az, float wx,
        float wy, float wz, float& range, int32_t& status, int32_t& steps, float* __restrict__ g) {
    float t = p.t_min, t_prev = 0.f, d_prev = 0.f;
    uint32_t k = 0;
    bool seen = false;
    for (;;) {                                                                      // (every pass ends the ray or raises k, which ends it at max_steps)
        if (!(t <= p.t_max)) { status = 1; range = p.t_max; break; }
        if (k == p.max_steps) { status = 2; range = t; break; }
        float d = 0.f;
        const bool in = fd_sample<false>(F, __fadd_rn(ax, __fmul_rn(t, wx)), __fadd_rn(ay, __fmul_rn(t, wy)), __fadd_rn(az, __fmul_rn(t, wz)), d, nullptr);
        ++k;
        if (!in) {
            if (seen) { status = 3; range = t_prev; break; }
            t = __fadd_rn(t, p.step_outside);
            continue;
        }
        if (d <= p.eps) {
            status = 0;
            range = seen ? __fadd_rn(t_prev, __fmul_rn(__fsub_rn(t, t_prev), __fdiv_rn(__fsub_rn(d_prev, p.eps), __fsub_rn(d_prev, d)))) : t;
            break;
        }
        seen = true; t_prev = t; d_prev = d;
        t = __fadd_rn(t, fmaxf(__fmul_rn(p.relax, d), p.step_min));
    }
    steps = (int32_t)k;
    if (NORMAL) {
        g[0] = 0.f; g[1] = 0.f; g[2] = 0.f;
        if (status == 0) {
            float d;
            (void)fd_sample<true>(F, __fadd_rn(ax, __fmul_rn(range, wx)), __fadd_rn(ay, __fmul_rn(range, wy)), __fadd_rn(az, __fmul_rn(range, wz)), d, g);
        }
    }
}

template <bool NORMAL> __global__ void __launch_bounds__(256) k_field_trace(DistFieldView F, FieldTraceArgs p) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x, h = blockIdx.y;
    if (r >= p.n) return;
    const FtPair* __restrict__ rec = reinterpret_cast<const FtPair*>(p.rays + 6 * (size_t)r);
    const FtPair v0 = rec[0], v1 = rec[1], v2 = rec[2];
    float ax = v0.x, ay = v0.y, az = v1.x, wx = v1.y, wy = v2.x, wz = v2.y;         // poses == nullptr: world rays, used as given
    if (p.poses != nullptr) {
        const float* __restrict__ M = p.poses + 16 * (size_t)h;
        const Fd3 a = fd_centre<true>(M, ax, ay, az);
        const float ux = wx, uy = wy, uz = wz;
        wx = __fadd_rn(__fadd_rn(__fmul_rn(M[0], ux), __fmul_rn(M[1], uy)), __fmul_rn(M[2], uz));
        wy = __fadd_rn(__fadd_rn(__fmul_rn(M[4], ux), __fmul_rn(M[5], uy)), __fmul_rn(M[6], uz));
        wz = __fadd_rn(__fadd_rn(__fmul_rn(M[8], ux), __fmul_rn(M[9], uy)), __fmul_rn(M[10], uz));
        ax = a.x; ay = a.y; az = a.z;
    }
    float range, g[3]; int32_t status, steps;
    ft_march<NORMAL>(F, p, ax, ay, az, wx, wy, wz, range, status, steps, g);
    const size_t at = (size_t)h * p.stride + r;
    p.range[at] = range;
    if (p.status != nullptr) p.status[at] = status;
    if (p.steps != nullptr) p.steps[at] = steps;
    if (NORMAL) { p.normal[3 * at] = g[0]; p.normal[3 * at + 1] = g[1]; p.normal[3 * at + 2] = g[2]; }
}

// the terms of one beam into t[3] = rho, valid, hit; a padding beam (!live) and a beam without a return (a NaN) give +0 throughout
__device__ __forceinline__ void ft_beam(float huber, bool live, float range, int32_t status, float measured, float* __restrict__ t) {
    t[0] = 0.f; t[1] = 0.f; t[2] = 0.f;
    if (live && !(measured != measured)) {
        const float e = __fsub_rn(range, measured), m = fabsf(e);
        t[0] = m <= huber ? __fmul_rn(e, e) : __fmul_rn(huber, __fsub_rn(__fmul_rn(2.f, m), huber));
        t[1] = 1.f; t[2] = status == 0 ? 1.f : 0.f;
    }
}

__global__ void __launch_bounds__(256) k_beam_terms(const float* __restrict__ range, const int32_t* __restrict__ status, const float* __restrict__ measured,
        uint32_t n, uint32_t stride, float huber, float* __restrict__ part) {
    const uint32_t chunk = blockIdx.x, h = blockIdx.y;
    // the lane's four consecutive beams: 16 bytes at a multiple of 16 (the stride and the host's offsets are multiples of 4 words), or what is left of them
    const uint32_t i0 = chunk * kScanMatchChunk + threadIdx.x * 4u;
    const size_t at = (size_t)h * stride + i0;
    float rg[4] = { 0.f, 0.f, 0.f, 0.f }, me[4] = { 0.f, 0.f, 0.f, 0.f }; int32_t st[4] = { 1, 1, 1, 1 };
    if (i0 + 4u <= n) {
        const float4 a = *reinterpret_cast<const float4*>(range + at), b = *reinterpret_cast<const float4*>(measured + i0);
        const int4 c = *reinterpret_cast<const int4*>(status + at);
        rg[0] = a.x; rg[1] = a.y; rg[2] = a.z; rg[3] = a.w; me[0] = b.x; me[1] = b.y; me[2] = b.z; me[3] = b.w;
        st[0] = c.x; st[1] = c.y; st[2] = c.z; st[3] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + (uint32_t)k < n) { rg[k] = range[at + k]; st[k] = status[at + k]; me[k] = measured[i0 + (uint32_t)k]; }
    }
    fd_block_row<3>([&](int k, float* __restrict__ t) { ft_beam(huber, i0 + (uint32_t)k < n, rg[k], st[k], me[k], t); },
        part + ((size_t)h * gridDim.x + chunk) * kScanMatchRow);
}

void launch_field_trace(hipStream_t s, const float* D, const Lattice& g, const FieldTraceArgs& a) {
    const DistFieldView F = dist_field_view(D, g);
    const dim3 grid((a.n + 255u) / 256u, a.n_pose);
    if (a.normal != nullptr) hipLaunchKernelGGL((k_field_trace<true>), grid, dim3(256), 0, s, F, a);
    else hipLaunchKernelGGL((k_field_trace<false>), grid, dim3(256), 0, s, F, a);
}
size_t beam_score_scratch(uint32_t n, uint32_t n_pose) { return scan_match_scratch(n, n_pose); }
void launch_beam_score(hipStream_t s, const float* range, const int32_t* status, const float* measured, uint32_t n, uint32_t n_pose, uint32_t stride,
        float huber, float* scratch, float* rows) {
    const uint32_t chunks = (n + kScanMatchChunk - 1u) / kScanMatchChunk;
    hipLaunchKernelGGL(k_beam_terms, dim3(chunks, n_pose), dim3(256), 0, s, range, status, measured, n, stride, huber, scratch);
    launch_scan_fold(s, scratch, chunks, n_pose, rows, kScanMatchRow - 2u - 3u, kScanMatchLite);
}

}  // namespace mon
