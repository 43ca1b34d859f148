// pose_device.h -- device code shared by the pose kernels: object pose refinement (kernels_pose.hip) and camera refinement against a scene of objects
// (kernels_scene_pose.hip): the half-wave scans of the composite backward, the hash-grid position gradient of one level pair, the MLP backward of one
// 32-sample tile down to dL/dx, and the closed-form SE(3) exponential of the Adam step.
#pragma once
#include "fused_device.h"

namespace mon {

// 32-lane inclusive SUFFIX sum (each half-wave on its own; lanes 0-31 are the ones read): row_shl within each row, then row 0 takes row 1's total
__device__ __forceinline__ float suffix_add32(float v) {
    v += dpp_f<0x101, 0xF>(0.f, v); v += dpp_f<0x102, 0xF>(0.f, v); v += dpp_f<0x104, 0xF>(0.f, v); v += dpp_f<0x108, 0xF>(0.f, v);
    const float r1 = lane_bcast(v, 16), r3 = lane_bcast(v, 48);
    const int lane = threadIdx.x & 63;
    return v + ((lane & 16) ? 0.f : (lane < 32 ? r1 : r3));
}
// value of the next lane (wave_shl:1; lane 63 keeps `fill`)
__device__ __forceinline__ float lane_next(float v, float fill) { return dpp_f<0x130, 0xF>(fill, v); }
__device__ __forceinline__ float max32(float v) {                                       // (v >= 0) max over each half-wave, in lane 31 / 63
    v = fmaxf(v, dpp_f<0x111, 0xF>(0.f, v)); v = fmaxf(v, dpp_f<0x112, 0xF>(0.f, v)); v = fmaxf(v, dpp_f<0x114, 0xF>(0.f, v));
    v = fmaxf(v, dpp_f<0x118, 0xF>(0.f, v)); v = fmaxf(v, dpp_f<0x142, 0xA>(0.f, v));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { const float s = scan_add32(v); return lane_bcast(s, 31) + lane_bcast(s, 63); }
__device__ __forceinline__ float huber_f(float x, float delta) { const float ax = fabsf(x); return ax <= delta ? 0.5f * x * x : delta * (ax - 0.5f * delta); }

// dL/dx (normalised box coordinates) of one level pair: the trilinear weights' derivative against the corner features, dotted with dL/dE of the level this
// half-wave owns (de0, de1); the corners are the ones the encode gathered (encode_swap of the same window)
// LW: the level's term times its weight (lw: lane il / 32 + il holds the weight of the level it holds in LevelRegs), after the term is formed in fp32
template <bool LW>
__device__ __forceinline__ void pose_level_grad(float (&g)[3], int il, const uint32_t (&c0)[4], const uint32_t (&c1)[4], const LevelRegs& lr, const float x[3],
        int h, int L, float de0, float de1, float lw) {
    const int LPH = (L + 1) >> 1;
    const float scale = h ? lane_f(lr.scale, 32 + il) : lane_f(lr.scale, il);
    float pos[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { const float q = fmaf(scale, x[d], 0.5f); pos[d] = q - floorf(q); }
    const float wx[2] = { 1.f - pos[0], pos[0] }, wy[2] = { 1.f - pos[1], pos[1] }, wz[2] = { 1.f - pos[2], pos[2] };
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const half2_t v = __builtin_bit_cast(half2_t, (k & 1) ? c1[k >> 1] : c0[k >> 1]);
        const float f = fmaf(de1, (float)v.y, de0 * (float)v.x);
        const float sx = (k & 1) ? 1.f : -1.f, sy = ((k >> 1) & 1) ? 1.f : -1.f, sz = (k >> 2) ? 1.f : -1.f;
        const float ax = wx[k & 1], ay = wy[(k >> 1) & 1], az = wz[k >> 2];
        gx = fmaf(sx * ay * az, f, gx); gy = fmaf(ax * sy * az, f, gy); gz = fmaf(ax * ay * sz, f, gz);
    }
    const bool real = il < LPH && h * LPH + il < L;
    if constexpr (LW) {
        const float wl = h ? lane_f(lw, 32 + il) : lane_f(lw, il);
        g[0] += real ? wl * (scale * gx) : 0.f; g[1] += real ? wl * (scale * gy) : 0.f; g[2] += real ? wl * (scale * gz) : 0.f;
    } else {
        g[0] += real ? scale * gx : 0.f; g[1] += real ? scale * gy : 0.f; g[2] += real ? scale * gz : 0.f;
    }
}

// Backward of one evaluated 32-sample tile from dL/dO (dOt[4], lanes of half-wave 0; `up` the ray's power-of-two scale, `down` its inverse) to the position
// gradient: MLP backward on MFMA through the transposed fragments (F_WOT / F_W1T / F_W0T) -> dL/dE -> the corners once more, level pair by level pair
// through the encode's gather window.  gl += dL/dx in the object frame, this half-wave's levels only (the caller adds the halves where it needs the sum).
template <int EPAD, int W, int NH, bool LW>
__device__ __forceinline__ void pose_tile_backward(float (&gl)[3], TileState<EPAD, W, NH>& st, half_t* frags, const LevelRegs& lregs,
        const __amdgpu_buffer_rsrc_t rsrc, const float (&xt)[3], const float (&dOt)[4], float up, float down, const float (&ext)[3], int lane, int h, int L,
        float lw) {
    using S = FusedShape<EPAD, W, NH>;
    half8_t bdo;
#pragma unroll
    for (int j = 0; j < 8; ++j) bdo[j] = (half_t)0.f;
    if (h == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) bdo[c] = (half_t)(dOt[c] * up);
    }
    half8_t dhl[S::MB][2];
#pragma unroll
    for (int mb = 0; mb < S::MB; ++mb) {
        float16_t ac = float16_t{ 0 };
        ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(lds_frag(frags, S::F_WOT + mb, lane), bdo, ac, 0, 0, 0);
        if constexpr (NH == 2) mask_pack(ac, st.h1[mb][0], st.h1[mb][1], dhl[mb][0], dhl[mb][1]);
        else mask_pack(ac, st.h0[mb][0], st.h0[mb][1], dhl[mb][0], dhl[mb][1]);
    }
    half8_t dh0[S::MB][2];
    if constexpr (NH == 2) {
#pragma unroll
        for (int mb = 0; mb < S::MB; ++mb) {
            float16_t ac = float16_t{ 0 };
#pragma unroll
            for (int s = 0; s < S::KSW; ++s) ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(lds_frag(frags, S::F_W1T + mb * S::KSW + s, lane),
                    dhl[s >> 1][s & 1], ac, 0, 0, 0);
            mask_pack(ac, st.h0[mb][0], st.h0[mb][1], dh0[mb][0], dh0[mb][1]);
        }
    } else {
#pragma unroll
        for (int mb = 0; mb < S::MB; ++mb) { dh0[mb][0] = dhl[mb][0]; dh0[mb][1] = dhl[mb][1]; }
    }
    float16_t de = float16_t{ 0 };
#pragma unroll
    for (int s = 0; s < S::KSW; ++s) de = __builtin_amdgcn_mfma_f32_32x32x16_f16(lds_frag(frags, S::F_W0T + s, lane), dh0[s >> 1][s & 1], de, 0, 0, 0);
    // ---- position gradient: the corners once more, level pair by level pair through the encode's gather window
    constexpr int EB = GatherWindow<EPAD, W, NH>::EB;
    GatherWindow<EPAD, W, NH> g;
    encode_begin<EPAD, W, NH, false>(g, lregs, rsrc, xt, lane, true);
#pragma unroll
    for (int il = 0; il < S::LLV; ++il) {
        uint32_t c0[4], c1[4];
        encode_swap<EPAD, W, NH>(g, il, c0, c1);
        if (il + EB < S::LLV) encode_issue<EPAD, W, NH, false>(g, il + EB, lregs, rsrc, xt, h, true);
        pose_level_grad<LW>(gl, il, c0, c1, lregs, xt, h, L, de[2 * il], de[2 * il + 1], lw);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) gl[d] = gl[d] * down / ext[d];                   // object frame (this half-wave's levels)
}

// closed-form SE(3) exponential of xi = (rho, phi): R = I + A [phi]x + B [phi]x^2, t = (I + B [phi]x + C [phi]x^2) rho; column-major 3x3 in R[9]
__device__ inline void se3_exp(const float xi[6], float R[9], float t[3]) {
    const float w0 = xi[3], w1 = xi[4], w2 = xi[5];
    const float th2 = w0 * w0 + w1 * w1 + w2 * w2, th = sqrtf(th2);
    float A, B, C;
    if (th < 1e-3f) { A = 1.f - th2 / 6.f; B = 0.5f - th2 / 24.f; C = 1.f / 6.f - th2 / 120.f; }
    else { const float s = sinf(th), c = cosf(th); A = s / th; B = (1.f - c) / th2; C = (th - s) / (th2 * th); }
    // K = [phi]x, K2 = K K
    const float K[9] = { 0.f, w2, -w1, -w2, 0.f, w0, w1, -w0, 0.f };                 // column-major
    float K2[9];
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) {
        float v = 0.f; for (int k = 0; k < 3; ++k) v += K[k * 3 + r] * K[c * 3 + k]; K2[c * 3 + r] = v; }
    float V[9];
    for (int i = 0; i < 9; ++i) { const float I = (i % 4 == 0) ? 1.f : 0.f; R[i] = I + A * K[i] + B * K2[i]; V[i] = I + B * K[i] + C * K2[i]; }
    for (int r = 0; r < 3; ++r) t[r] = V[r] * xi[0] + V[3 + r] * xi[1] + V[6 + r] * xi[2];
}

}  // namespace mon
