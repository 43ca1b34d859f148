// scene_device.h -- device code shared by the merge-composite kernels of the scene render (k_scene_composite, kernels_render.hip) and of camera refinement
// (k_scene_composite_grad, kernels_scene_pose.hip): the compaction of one ray's non-empty sample lists and the merged order of their samples.
#pragma once
#include "fused_device.h"

namespace mon {

// One wavefront (= one workgroup) per ray.  The ray's non-empty lists are compacted into LDS in list order (s_id: compact -> list, s_c its count, s_tf / s_tl
// its first / last t, s_w zeroed), then every sample's place in the merged order is counted: its index in its own list + the samples of each other list that
// come before it (ties to the lower list index) -- the whole list or none where the t ranges do not overlap, a binary search of that list where they do.
// s_perm[rank] = compact list << 6 | index.  na = the non-empty lists, n_tot = their samples.  Ends with a barrier.
__device__ __forceinline__ void scene_merge_lists(uint32_t ray, uint32_t n_lists, uint32_t cap, const float* __restrict__ tl, const uint32_t* __restrict__ cnt,
        int lane, uint16_t* s_perm, uint32_t* s_id, uint32_t* s_c, float* s_tf, float* s_tl, float* s_w, uint32_t& na_out, uint32_t& n_tot_out) {
    constexpr uint32_t L2S = 64u;                                                       // kSceneListLen
    // ---- the ray's non-empty lists, in list order
    uint32_t na = 0u, n_tot = 0u;
    for (uint32_t g = 0; g < n_lists; g += 64u) {
        const uint32_t k = g + (uint32_t)lane;
        uint32_t c = k < n_lists ? cnt[(size_t)k * cap + ray] : 0u;
        c = c < L2S ? c : L2S;
        const unsigned long long b = __ballot(c > 0u);
        if (c > 0u) {
            const uint32_t pos = na + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            const float* q = tl + ((size_t)k * cap + ray) * L2S;
            s_id[pos] = k; s_c[pos] = c; s_tf[pos] = q[0]; s_tl[pos] = q[c - 1u]; s_w[pos] = 0.f;
        }
        na += (uint32_t)__popcll(b);
        n_tot += (uint32_t)__builtin_amdgcn_readlane((int)scan_add64_u32(c), 63);
    }
    __syncthreads();
    // ---- merged order: rank of every sample
    for (uint32_t a = 0; a < na; ++a) {
        const uint32_t c = s_c[a];
        if ((uint32_t)lane < c) {
            const float tv = tl[((size_t)s_id[a] * cap + ray) * L2S + lane];
            uint32_t r = (uint32_t)lane;
            for (uint32_t b = 0; b < na; ++b) {
                if (b == a) continue;
                const bool first = b < a;                                          // (list b's samples at an equal t come first)
                const uint32_t cb = s_c[b];
                const float lb = s_tl[b], fb = s_tf[b];
                if (first ? lb <= tv : lb < tv) r += cb;                           // all of list b is in front
                else if (first ? fb <= tv : fb < tv) {                             // part of it: count (binary search; the last one is not in front)
                    const float* q = tl + ((size_t)s_id[b] * cap + ray) * L2S;
                    uint32_t pos = 0u;
                    for (uint32_t step = L2S / 2u; step; step >>= 1)
                        if (pos + step <= cb) { const float v = q[pos + step - 1u]; if (first ? v <= tv : v < tv) pos += step; }
                    r += pos;
                }
            }
            s_perm[r] = (uint16_t)((a << 6) | (uint32_t)lane);                     // (r <= n_tot - 1 whatever the lists hold)
        }
    }
    __syncthreads();
    na_out = na; n_tot_out = n_tot;
}

}  // namespace mon
