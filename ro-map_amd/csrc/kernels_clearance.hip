// kernels_clearance.hip -- a device-resident distance field asked at world points and along trajectories (mon_dist_field_sample, mon_dist_field_score;
// DESIGN.md 3.4c-9).  The rule is in include/mon_core.h: trilinear interpolation with every fp32 operation rounded on its own (nothing is contracted), the
// gradient from the same intermediates, a body of up to 32 spheres swept along a trajectory's samples.
//   k_field_sample       a thread per point: d and, when asked for, the gradient
//   k_traj_score<false>  n_samp <= 64: a wave per trajectory (four to a workgroup), a lane per sample; min_clear, first_hit and the cost tree by shuffles
//   k_traj_score<true>   longer ones: a workgroup per trajectory (128 threads up to 128 samples, 256 above), a thread per sample and round; the penalties
//                        in LDS in sample order, the cost tree there (fd_lds_fold), the two minima by shuffles and through LDS across the waves
//   k_field_max          the largest value of a field that was made on the device (mon_dist_field_info), in two launches of partial maxima
// A lane owns a sample: the loop over the body's spheres runs inside it, so the fold over k and the minimum over k need no exchange.  A sample's two end
// centres are recomputed from the waypoints (a few scalar-cached words) instead of being staged.  The sample itself (fd_axis, fd_lerp, fd_sample, fd_centre)
// is field_sample_device.h's, shared with kernels_scan_match.hip and kernels_field_trace.hip.  Plain C++, vector stores only, no atomics, no scratch; no workgroup waits for another;
// every loop is bounded by an argument the host has checked.
#include "field_sample_device.h"

namespace mon {

__global__ void __launch_bounds__(256) k_field_sample(DistFieldView F, const float* __restrict__ xyz, uint32_t n, float outside, float* __restrict__ dist,
        float* __restrict__ grad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float d = outside, g[3] = { 0.f, 0.f, 0.f };
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (grad != nullptr) (void)fd_sample<true>(F, x, y, z, d, g); else (void)fd_sample<false>(F, x, y, z, d, g);
    dist[i] = d;
    if (grad != nullptr) { grad[3 * (size_t)i] = g[0]; grad[3 * (size_t)i + 1] = g[1]; grad[3 * (size_t)i + 2] = g[2]; }
}

// ---- trajectories.  A sample's sphere centres come from the waypoints by fd_centre (field_sample_device.h)
// sample q of a trajectory (its waypoints at `ways`): the centre of sphere b
template <bool POSE> __device__ __forceinline__ Fd3 fd_sample_centre(const float* __restrict__ ways, uint32_t w, uint32_t u, float tau, float bx, float by,
        float bz) {
    constexpr uint32_t WF = POSE ? 16u : 3u;
    Fd3 c = fd_centre<POSE>(ways + (size_t)w * WF, bx, by, bz);
    if (u != 0u) {
        const Fd3 n = fd_centre<POSE>(ways + (size_t)(w + 1u) * WF, bx, by, bz);
        c.x = __fadd_rn(c.x, __fmul_rn(tau, __fsub_rn(n.x, c.x))); c.y = __fadd_rn(c.y, __fmul_rn(tau, __fsub_rn(n.y, c.y)));
        c.z = __fadd_rn(c.z, __fmul_rn(tau, __fsub_rn(n.z, c.z)));
    }
    return c;
}
// what a lane learns of its sample q of trajectory t: the least clearance over the body, whether some sphere is within the margin, the penalty; a waypoint's
// own sample (u == 0) also writes way_clear and way_grad
struct FdSampleOut { float clear; bool hit; float pen; };
template <bool POSE> __device__ __forceinline__ FdSampleOut fd_score_sample(const DistFieldView& F, const float* __restrict__ spheres, uint32_t n_spheres,
        const float* __restrict__ ways, uint32_t t, uint32_t q, const TrajScoreArgs& a) {
    const uint32_t w = q / a.n_sub, u = q - w * a.n_sub;
    const float tau = __fdiv_rn((float)u, (float)a.n_sub);
    FdSampleOut o{ INFINITY, false, 0.f };
    uint32_t kmin = 0;
    for (uint32_t k = 0; k < n_spheres; ++k) {
        const float bx = spheres[4 * k], by = spheres[4 * k + 1], bz = spheres[4 * k + 2], r = spheres[4 * k + 3];
        const Fd3 c = fd_sample_centre<POSE>(ways, w, u, tau, bx, by, bz);
        float d = a.outside;
        (void)fd_sample<false>(F, c.x, c.y, c.z, d, nullptr);
        const float clear = __fsub_rn(d, r);
        if (clear < o.clear) { o.clear = clear; kmin = k; }
        o.hit = o.hit || !(clear > a.margin);
        const float h = fmaxf(0.f, __fsub_rn(a.safe, clear));
        o.pen = __fadd_rn(o.pen, __fmul_rn(h, h));
    }
    if (u == 0u) {
        const size_t at = (size_t)t * a.n_way + w;
        if (a.way_clear != nullptr) a.way_clear[at] = o.clear;
        if (a.way_grad != nullptr) {
            const Fd3 c = fd_sample_centre<POSE>(ways, w, 0u, 0.f, spheres[4 * kmin], spheres[4 * kmin + 1], spheres[4 * kmin + 2]);
            float d, g[3] = { 0.f, 0.f, 0.f };
            (void)fd_sample<true>(F, c.x, c.y, c.z, d, g);
            a.way_grad[3 * at] = g[0]; a.way_grad[3 * at + 1] = g[1]; a.way_grad[3 * at + 2] = g[2];
        }
    }
    return o;
}
__device__ __forceinline__ float fd_wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ uint32_t fd_wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}
constexpr uint32_t kFdNoHit = 0xffffffffu;

// WG false: blockDim 256, wave w of block b scores trajectory 4 b + w; n_samp <= 64.  WG true: block b scores trajectory b with blockDim 128 or 256; its
// dynamic LDS holds the penalties padded with +0 to P, the power of two at or above n_samp.
template <bool WG, bool POSE> __global__ void __launch_bounds__(256) k_traj_score(DistFieldView F, const float* __restrict__ spheres, uint32_t n_spheres,
        const float* __restrict__ ways_all, TrajScoreArgs a) {
    extern __shared__ float pen_s[];
    __shared__ float min_s[4];
    __shared__ uint32_t hit_s[4];
    constexpr uint32_t WF = POSE ? 16u : 3u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t t = WG ? blockIdx.x : blockIdx.x * 4u + wave;
    if (t >= a.n_traj) return;                                                      // (WG false: a whole wave; it meets no barrier below)
    const float* ways = ways_all + (size_t)t * a.n_way * WF;
    float clear = INFINITY; uint32_t first = kFdNoHit;
    if (!WG) {
        float pen = 0.f;
        if (lane < a.n_samp) {
            const FdSampleOut o = fd_score_sample<POSE>(F, spheres, n_spheres, ways, t, lane, a);
            clear = o.clear; pen = o.pen; if (o.hit) first = lane;
        }
        clear = fd_wave_min(clear); first = fd_wave_min(first);
        // the tree over the 64 lanes: the header's tree over P values followed by levels that add +0, which changes no bit of a sum that is >= +0
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) pen = __fadd_rn(pen, __shfl_down(pen, m));
        if (lane == 0u) {
            a.min_clear[t] = clear;
            if (a.first_hit != nullptr) a.first_hit[t] = first == kFdNoHit ? -1 : (int32_t)first;
            if (a.cost != nullptr) a.cost[t] = pen;
        }
        return;
    }
    for (uint32_t q = threadIdx.x; q < a.pad; q += blockDim.x) {
        float pen = 0.f;
        if (q < a.n_samp) {
            const FdSampleOut o = fd_score_sample<POSE>(F, spheres, n_spheres, ways, t, q, a);
            clear = fminf(clear, o.clear); pen = o.pen; if (o.hit) first = min(first, q);
        }
        pen_s[q] = pen;
    }
    clear = fd_wave_min(clear); first = fd_wave_min(first);
    if (lane == 0u) { min_s[wave] = clear; hit_s[wave] = first; }
    __syncthreads();
    fd_lds_fold(pen_s, 1u, a.pad, threadIdx.x, blockDim.x);
    if (threadIdx.x == 0u) {
        const uint32_t waves = blockDim.x >> 6;
        for (uint32_t k = 1; k < waves; ++k) { clear = fminf(clear, min_s[k]); first = min(first, hit_s[k]); }
        a.min_clear[t] = clear;
        if (a.first_hit != nullptr) a.first_hit[t] = first == kFdNoHit ? -1 : (int32_t)first;
        if (a.cost != nullptr) a.cost[t] = pen_s[0];
    }
}

// the largest of n values, none of them a NaN: `blocks` partial maxima, then (blocks == 1) their maximum into out[0]
__global__ void __launch_bounds__(256) k_field_max(const float* __restrict__ v, uint32_t n, float* __restrict__ out) {
    __shared__ float m_s[4];
    float m = -INFINITY;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) m = fmaxf(m, v[i]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
    if ((threadIdx.x & 63u) == 0u) m_s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) out[blockIdx.x] = fmaxf(fmaxf(m_s[0], m_s[1]), fmaxf(m_s[2], m_s[3]));
}

void launch_field_sample(hipStream_t s, const float* D, const Lattice& g, const float* xyz, uint32_t n, float outside, float* dist, float* grad) {
    const DistFieldView F = dist_field_view(D, g);
    hipLaunchKernelGGL(k_field_sample, dim3((n + 255u) / 256u), dim3(256), 0, s, F, xyz, n, outside, dist, grad);
}
uint32_t traj_score_pad(uint32_t n_samp) { uint32_t p = 1; while (p < n_samp) p <<= 1; return p; }
void launch_traj_score(hipStream_t s, const float* D, const Lattice& g, const float* spheres, uint32_t n_spheres, const float* ways, bool pose,
        TrajScoreArgs a) {
    const DistFieldView F = dist_field_view(D, g);
    a.pad = traj_score_pad(a.n_samp);
    if (a.n_samp <= 64u) {
        const dim3 grid((a.n_traj + 3u) / 4u);
        if (pose) hipLaunchKernelGGL((k_traj_score<false, true>), grid, dim3(256), 0, s, F, spheres, n_spheres, ways, a);
        else hipLaunchKernelGGL((k_traj_score<false, false>), grid, dim3(256), 0, s, F, spheres, n_spheres, ways, a);
    } else {
        const dim3 grid(a.n_traj), block(a.n_samp <= 128u ? 128 : 256);
        if (pose) hipLaunchKernelGGL((k_traj_score<true, true>), grid, block, 4 * (size_t)a.pad, s, F, spheres, n_spheres, ways, a);
        else hipLaunchKernelGGL((k_traj_score<true, false>), grid, block, 4 * (size_t)a.pad, s, F, spheres, n_spheres, ways, a);
    }
}
void launch_field_max(hipStream_t s, const float* v, uint32_t n, float* partial, float* out) {
    hipLaunchKernelGGL(k_field_max, dim3(kFieldMaxBlocks), dim3(256), 0, s, v, n, partial);
    hipLaunchKernelGGL(k_field_max, dim3(1), dim3(256), 0, s, partial, kFieldMaxBlocks, out);
}

}  // namespace mon
