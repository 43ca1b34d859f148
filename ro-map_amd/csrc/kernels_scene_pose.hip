// kernels_scene_pose.hip -- camera pose refinement against a scene of object NeRFs (mon_scene_pose_loss / mon_scene_refine_camera): the drawn rays under the
// candidate camera pose in every object's frame, each object's sample lists (forward only), the merged composite with its loss and its backward, each
// object's MLP backward and hash-grid position gradient from the gradients the composite left in the lists, and the Adam step on the camera twist.
// The objective is stated in include/mon_core.h and DESIGN.md 3.4f.  No atomics anywhere: every sum runs in a fixed order.
// Window refinement runs the composite and the object backward over a pass of whole frames: k_scene_window_composite and k_scene_window_obj
// stand next to the single-frame kernels and share their bodies, each workgroup confined to one frame's rays and to that frame's single-frame walk.
#include <type_traits>
#include "pose_device.h"
#include "scene_device.h"

namespace mon {

// ------------------------------------------------------------------ k_scene_pose_rays
// One thread per drawn ray of the chunk (global ray i = ray0 + r): scene_pose_ray (scene_device.h) under the candidate Twc in device memory.
__global__ void __launch_bounds__(256) k_scene_pose_rays(ScenePoseRayArgs a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rays) return;
    scene_pose_ray(a, r, a.ray0 + r, a.pose);
}

// ------------------------------------------------------------------ k_scene_pose_obj
// One sample tile of one object's ray: position, network forward, sigma, colour, alpha (the render's arithmetic; the first interval from `tlast`)
template <int EPAD, int W, int NH>
struct SceneTile { TileState<EPAD, W, NH> ts; float t, x[3], p[3], dt, sigma, alpha, col[3]; };
template <int EPAD, int W, int NH>
__device__ __forceinline__ void scene_tile_forward(SceneTile<EPAD, W, NH>& q, int tile, int n, int lane, const float (&ro)[3], const float (&rd)[3], float t0,
        float dtr, float jitter, float tlast, const Aabb& aabb, const float (&ext)[3], half_t* frags, const LevelRegs& lregs, const half2_t* table,
        uint32_t table_bytes, int L) {
    const uint32_t k = (uint32_t)tile * 32u + (uint32_t)n;
    const float t = fmaf(dtr, (float)k + jitter, t0);
    q.t = t;
#pragma unroll
    for (int d = 0; d < 3; ++d) { const float v = fmaf(t, rd[d], ro[d]); q.p[d] = v; q.x[d] = (v - aabb.mn[d]) / ext[d]; }
    tile_forward<EPAD, W, NH>(q.ts, frags, lregs, table, table_bytes, L, q.x, lane);
    q.sigma = __expf(q.ts.out4[3]);
    q.col[0] = logistic_f(q.ts.out4[0]); q.col[1] = logistic_f(q.ts.out4[1]); q.col[2] = logistic_f(q.ts.out4[2]);
    float tprev = lane_prev(t, tlast); if (n == 0) tprev = tlast;
    q.dt = t - tprev;
    q.alpha = 1.f - __expf(-q.sigma * q.dt);
}

// One wavefront per ray of one object, its 2S = 64 samples as two 32-sample tiles (k_fused_render's placement, jitter, alpha, colour; the second tile only
// where the object's own transmittance after the first is >= eps).
// BWD = false: the forward alone.  Writes the object's list of the ray in the EMIT format of the scene render: t, {alpha, r, g, b}, count (0 a miss, else
// 32 per evaluated tile).
// BWD = true: recomputes the forward of the tiles the count names, takes dL/dalpha and w of every sample from the list slots k_scene_composite_grad filled
// and G_rgb from the ray's row, forms dL/dO (x the ray's power-of-two scale), and runs pose_tile_backward -- k_pose_grad's MLP backward and position
// gradient.  Per lane: sums of g and x x g over its samples, object frame; per workgroup: one partial row of 8 floats {g, x x g, 0, 0}.
// The body walks rays r = blk * WAVES + wave, + n_blk * WAVES, ... < n_rays of the lists' slots v0 + r and writes the row `row` of `partials`:
// k_scene_pose_obj is (blockIdx.x, gridDim.x, p.n_rays, 0, blockIdx.x); k_scene_window_obj confines a workgroup to one frame of a window pass.
template <int EPAD, int W, int NH, bool LW, bool BWD>
__device__ __forceinline__ void scene_pose_obj_body(const FusedArgs& a, const ScenePoseObjArgs& p, uint32_t blk, uint32_t n_blk, uint32_t n_rays, uint32_t v0,
        size_t row) {
    using S = FusedShape<EPAD, W, NH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t* frags = reinterpret_cast<half_t*>(smem);
    LevelLds* llt = reinterpret_cast<LevelLds*>(smem + S::FRAG_BYTES);
    float* red = reinterpret_cast<float*>(smem + S::FRAG_BYTES + 512);                  // [WAVES][8]
    build_fragments<EPAD, W, NH>(frags, llt, a, BWD);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int L = a.nd.L;
    const half2_t* table = reinterpret_cast<const half2_t*>(a.params + a.nd.n_mlp);
    const LevelRegs lregs = load_level_regs_uniform(a.lt, L, lane); const uint32_t table_bytes = a.lt.offset[L] * 4u;
    const __amdgpu_buffer_rsrc_t rsrc = table_rsrc(table, table_bytes);
    float lw = 1.f;                                                                     // LW: the weight of this lane's level (LevelRegs' placement)
    if constexpr (LW) {
        const int LPH = (L + 1) >> 1, lv = lane < 32 ? lane : lane - 32 + LPH;
        lw = ((lane & 31) < LPH && lv < L) ? p.level_w[lv] : 0.f;
    }
    float ext[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) ext[d] = a.oc.aabb.mx[d] - a.oc.aabb.mn[d];
    float acc[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    for (uint32_t rl = blk * S::WAVES + wave; rl < n_rays; rl += n_blk * S::WAVES) {
        const uint32_t ray = v0 + rl;
        const float4* rr = p.rec + 3 * (size_t)ray;
        const float4 r0 = rr[0], r1 = rr[1], r2 = rr[2];
        const float ro[3] = { r0.x, r0.y, r0.z }, rd[3] = { r1.x, r1.y, r1.z };
        const float t0 = r0.w, t1 = r1.w;
        const bool hit = r2.x != 0.f; const uint32_t base = __builtin_bit_cast(uint32_t, r2.y);
        const float dtr = (t1 - t0) / 64.0f;
        const size_t slot0 = (size_t)ray * 64u;
        if constexpr (!BWD) {
            if (!hit) { if (lane == 0) p.cnt[ray] = 0u; continue; }
            float Tc = 1.f, tlast = 0.f; uint32_t n_emit = 0u;
            for (int tile = 0; tile < 2; ++tile) {
                if (tile == 1 && !(Tc >= kTransmittanceEps)) break;
                SceneTile<EPAD, W, NH> q;
                const uint32_t k = (uint32_t)tile * 32u + (uint32_t)n;
                scene_tile_forward<EPAD, W, NH>(q, tile, n, lane, ro, rd, t0, dtr, rand01(p.seed, p.stream, p.step, base + k), tlast, a.oc.aabb, ext, frags,
                        lregs, table, table_bytes, L);
                if (lane < 32) { p.t[slot0 + k] = q.t; p.attr[slot0 + k] = make_float4(q.alpha, q.col[0], q.col[1], q.col[2]); }
                n_emit += 32u;
                const float tincl = scan_mul32(1.f - q.alpha) * Tc;
                float T = lane_prev(tincl, Tc); if (n == 0) T = Tc;
                const int nact = __popc((uint32_t)__ballot(T >= kTransmittanceEps));
                Tc = (nact > 0) ? lane_bcast(tincl, nact > 0 ? nact - 1 : 0) : Tc;
                tlast = lane_bcast(q.t, 31);
            }
            if (lane == 0) p.cnt[ray] = n_emit;
        } else {
            const uint32_t count = hit ? p.cnt[ray] : 0u;
            if (count == 0u && !p.dbg) continue;                                        // nothing of this object on the ray
            const float4 G = p.grow[ray];                                               // {G_rgb, l}
            const float Gc[3] = { G.x, G.y, G.z };
            SceneTile<EPAD, W, NH> q[2];
            float dO[2][4]; float mx = 0.f, tlast = 0.f;
#pragma unroll
            for (int tile = 0; tile < 2; ++tile) {
                const uint32_t k = (uint32_t)tile * 32u + (uint32_t)n;
                if ((uint32_t)tile * 32u >= count) {
                    const float t = fmaf(dtr, (float)k + rand01(p.seed, p.stream, p.step, base + k), t0);
                    q[tile].t = t;
#pragma unroll
                    for (int d = 0; d < 3; ++d) { q[tile].p[d] = fmaf(t, rd[d], ro[d]); q[tile].x[d] = 0.f; }
#pragma unroll
                    for (int c = 0; c < 4; ++c) dO[tile][c] = 0.f;
                    continue;
                }
                scene_tile_forward<EPAD, W, NH>(q[tile], tile, n, lane, ro, rd, t0, dtr, rand01(p.seed, p.stream, p.step, base + k), tlast, a.oc.aabb, ext,
                        frags, lregs, table, table_bytes, L);
                tlast = lane_bcast(q[tile].t, 31);
                const float2 gw = p.gw[slot0 + (size_t)k];                              // {dL/dalpha, w} of this sample in the merged composite
                const bool on = h == 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) dO[tile][c] = on ? Gc[c] * gw.y * (q[tile].col[c] * (1.f - q[tile].col[c])) : 0.f;
                dO[tile][3] = on ? gw.x * (1.f - q[tile].alpha) * q[tile].dt * q[tile].sigma : 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) mx = fmaxf(mx, fabsf(dO[tile][c]));
            }
            mx = lane_bcast(max32(mx), 31);
            // power-of-two scale: the largest |dL/dO| of the ray lands in [32, 64) -- exact to undo
            int e = 0; (void)frexpf(mx, &e);
            const float up = ldexpf(1.f, 6 - e), down = ldexpf(1.f, e - 6);
            const float4 uc = p.dbg ? p.ray[3 * (size_t)ray + 2] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int tile = 0; tile < 2; ++tile) {
                float gl[3] = { 0.f, 0.f, 0.f };
                const bool ev = (uint32_t)tile * 32u < count;
                if (ev && mx > 0.f)
                    pose_tile_backward<EPAD, W, NH, LW>(gl, q[tile].ts, frags, lregs, rsrc, q[tile].x, dO[tile], up, down, ext, lane, h, L, lw);
                acc[0] += gl[0]; acc[1] += gl[1]; acc[2] += gl[2];
                const float* x = q[tile].p;
                acc[3] += x[1] * gl[2] - x[2] * gl[1]; acc[4] += x[2] * gl[0] - x[0] * gl[2]; acc[5] += x[0] * gl[1] - x[1] * gl[0];
                if (p.dbg) {
                    float gf[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) gf[d] = gl[d] + __shfl_xor(gl[d], 32);
                    if (lane < 32) {                                                    // [ray][64][14]: x_o, x_c, t, raw, dL/dx
                        float* o = p.dbg + ((size_t)(p.ray0 + ray) * 64u + (uint32_t)tile * 32u + (uint32_t)n) * 14u;
                        const float tv = q[tile].t;
                        for (int d = 0; d < 3; ++d) { o[d] = hit ? x[d] : 0.f; o[7 + 4 + d] = gf[d] * p.inv_n; }
                        o[3] = hit ? tv * uc.x : 0.f; o[4] = hit ? tv * uc.y : 0.f; o[5] = hit ? tv * uc.z : 0.f; o[6] = hit ? tv : 0.f;
                        for (int c = 0; c < 4; ++c) o[7 + c] = ev ? q[tile].ts.out4[c] : 0.f;
                    }
                }
            }
        }
    }
    if constexpr (BWD) {
        // ---- wave sums, then the workgroup's row in wave order
        float tot6[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) tot6[j] = wave_sum(acc[j]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 6; ++j) red[wave * 8 + j] = tot6[j];
            red[wave * 8 + 6] = 0.f; red[wave * 8 + 7] = 0.f;
        }
        __syncthreads();
        if (threadIdx.x < 8) {
            float s = 0.f;
            for (int w = 0; w < S::WAVES; ++w) s += red[w * 8 + threadIdx.x];
            p.partials[row * 8 + threadIdx.x] = s;
        }
    }
}
template <int EPAD, int W, int NH, bool LW, bool BWD>
__global__ void __launch_bounds__(256) k_scene_pose_obj(FusedArgs a, ScenePoseObjArgs p) {
    scene_pose_obj_body<EPAD, W, NH, LW, BWD>(a, p, blockIdx.x, gridDim.x, p.n_rays, 0u, (size_t)blockIdx.x);
}
// The backward of one pass of a window (mon_scene_window_loss / mon_scene_refine_window), grid (workgroups, frames of the pass): workgroup (b, f) is workgroup
// b of the backward a single-frame call of frame f's N_f rays launches on gridc_f workgroups -- the same rays in the same order into the same sums -- and
// writes row row0_f + b of the object's partial rows.  Workgroups beyond the frame's own grid leave before any barrier.
template <int EPAD, int W, int NH, bool LW>
__global__ void __launch_bounds__(256) k_scene_window_obj(FusedArgs a, ScenePoseObjArgs p, const SceneWinFrame* __restrict__ frames) {
    const SceneWinFrame fr = frames[blockIdx.y];
    if (blockIdx.x >= fr.gridc) return;
    scene_pose_obj_body<EPAD, W, NH, LW, true>(a, p, blockIdx.x, fr.gridc, fr.n_rays, fr.v0, (size_t)fr.row0 + blockIdx.x);
}

// ------------------------------------------------------------------ k_scene_composite_grad
// 64-lane inclusive suffix sum from the two half-wave suffix sums
__device__ __forceinline__ float suffix_add64(float v) {
    const float s = suffix_add32(v);
    return s + ((threadIdx.x & 32) ? 0.f : lane_bcast(s, 32));
}
// One wavefront (= one workgroup) per ray: scene_composite_ray (scene_device.h; k_scene_composite's compaction and merged order, then the composite forward
// in blocks of 64 with a carried transmittance, each block's entry transmittance kept in LDS, the per-list weight sums W_j and the ray's loss
//   l = w_rgb M* |r|^2 / 3 + w_mask sum_j (W_j - m*_j)^2 + w_depth M* [d* > 0] Huber(D - d*)),
// then the blocks again in reverse with a carried suffix sum: with q_i = G_rgb . (c_i - c*) + G_D t_i + 2 w_mask (W_j(i) - m*_j(i)),
//   dL/dalpha_i = T_i q_i - sum_{n > i} w_n q_n / (1 - alpha_i)       (so that dL/dsigma_i = dt_i (T_{i+1} q_i - sum_{n > i} w_n q_n))
// Every merged sample's list slot receives {dL/dalpha, w} (0, 0 from the cut on); the ray's row receives {G_rgb, l}.  The workgroup's rays' losses are summed
// in ray order into loss_part[blockIdx.x].
// The walk: rays r = r0, r0 + stride, ... < n_rays at the lists' slots v0 + r; returns the sum of their losses in that order.
__device__ __forceinline__ float scene_composite_grad_walk(const SceneCompGradArgs& a, uint32_t r0, uint32_t n_rays, uint32_t stride, uint32_t v0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SceneLds s = scene_lds<true>(smem, a.n_lists);
    const int lane = threadIdx.x;
    float loss_acc = 0.f;
    for (uint32_t rl = r0; rl < n_rays; rl += stride) {
        const uint32_t ray = v0 + rl;
        SceneRayFwd f;
        scene_composite_ray<true>(a, s, ray, lane, f);
        loss_acc += f.l;
        const float Gc[3] = { a.w_rgb * f.Mstar * 2.f * f.res[0] / 3.f, a.w_rgb * f.Mstar * 2.f * f.res[1] / 3.f, a.w_rgb * f.Mstar * 2.f * f.res[2] / 3.f };
        const float GD = f.dep_on ? a.w_depth * clamp_f(f.D - f.dstar, -a.huber, a.huber) / f.dn : 0.f;
        if (lane == 0) { a.grow[ray] = make_float4(Gc[0], Gc[1], Gc[2], f.l); if (a.out_D) a.out_D[ray] = f.D; }
        __syncthreads();
        // ---- backward: the blocks in reverse (the forward's fetch and transmittance from each block's kept entry), the suffix sum of w q carried from
        // block to block
        float carry = 0.f;
        for (uint32_t bb = f.n_blocks; bb > 0u; --bb) {
            const uint32_t blk = bb - 1u, p = blk * 64u + (uint32_t)lane;
            SceneSample m = scene_fetch<false>(s, p, ray, a.cap, f.na, f.n_tot, a.t, a.attr);
            const bool have = m.a != ~0u;
            if (blk >= f.n_done) { if (have) a.gw[m.idx] = make_float2(0.f, 0.f); continue; }          // behind the cut
            scene_load(m, a.t, a.attr);
            const float qm = have ? s.q[m.a] : 0.f, omv = 1.f - m.al;
            const SceneTrans x = scene_transmittance(omv, s.T[blk], f.n_tot, lane);
            const float wgt = x.active ? m.al * x.T : 0.f;
            const float q = Gc[0] * (m.c0 - f.cs[0]) + Gc[1] * (m.c1 - f.cs[1]) + Gc[2] * (m.c2 - f.cs[2]) + GD * m.t + qm;
            const float sin = suffix_add64(wgt * q);                                   // inclusive
            float sfx = lane_next(sin, 0.f); if (lane == 63) sfx = 0.f;               // samples behind this one, this block
            sfx += carry;
            const float g = (x.active && have) ? x.T * q - (omv > 0.f ? sfx / omv : 0.f) : 0.f;
            if (have) a.gw[m.idx] = make_float2(g, wgt);
            carry += lane_bcast(sin, 0);
        }
        __syncthreads();
    }
    return loss_acc;
}
__global__ void __launch_bounds__(64) k_scene_composite_grad(SceneCompGradArgs a) {
    const float loss_acc = scene_composite_grad_walk(a, blockIdx.x, a.n_rays, gridDim.x, 0u);
    if (threadIdx.x == 0) a.loss_part[blockIdx.x] = loss_acc;
}
// One pass of a window, grid (workgroups, frames of the pass): workgroup (b, f) walks rays b, b + parts_f, ... of frame f -- k_scene_composite_grad's walk of
// a single-frame call of N_f rays on parts_f = scene_comp_grad_grid(N_f) workgroups -- and writes loss_part[lp0_f + b], as k_scene_composite_loss does per
// hypothesis.  Workgroups beyond parts_f leave before any barrier.
__global__ void __launch_bounds__(64) k_scene_window_composite(SceneCompGradArgs a, const SceneWinFrame* __restrict__ frames) {
    const SceneWinFrame fr = frames[blockIdx.y];
    if (blockIdx.x >= fr.parts) return;
    const float loss_acc = scene_composite_grad_walk(a, blockIdx.x, fr.n_rays, fr.parts, fr.v0);
    if (threadIdx.x == 0) a.loss_part[fr.lp0 + blockIdx.x] = loss_acc;
}

// ------------------------------------------------------------------ k_scene_pose_update
// One workgroup.  Per object, in index order: its partial rows summed in k_pose_update's fixed order (32 strided groups per column, then the groups in
// order), x 1/N -> G_j = (sum g_o, sum x_o x g_o) in the object frame; with Toc_j = Tow_j Twc = (R, p) mapped to the camera frame,
// grad_rho += R^T G_rho, grad_phi += R^T (G_phi - p x G_rho).  The loss partials are summed 256-strided, then in order.  out[8 * it] = {loss, grad6, 0};
// step != 0: Adam on the twist and Twc <- Twc exp(delta^), its rotation re-orthonormalised (Gram-Schmidt on the columns).
__global__ void __launch_bounds__(256) k_scene_pose_update(ScenePoseUpdateArgs a) {
    __shared__ float part[32][8];
    __shared__ float lpart[256];
    const uint32_t col = threadIdx.x & 7u, grp = threadIdx.x >> 3;
    float grad[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    for (uint32_t j = 0; j < a.n_objs; ++j) {
        const float* rows = a.partials + (size_t)j * a.row_stride * 8;
        float s = 0.f;
        for (uint32_t b = grp; b < a.n_rows; b += 32u) s += rows[(size_t)b * 8 + col];
        part[grp][col] = s;
        __syncthreads();
        if (threadIdx.x == 0) { float v[6]; scene_rows_to_camera(part, a.inv_n, a.objs[j].Tow, a.pose, grad, v); }
        __syncthreads();
    }
    float ls = 0.f;
    for (uint32_t b = threadIdx.x; b < a.n_loss_parts; b += 256u) ls += a.loss_part[b];
    lpart[threadIdx.x] = ls;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float loss = 0.f;
    for (int g = 0; g < 256; ++g) loss += lpart[g];
    loss *= a.inv_n;
    float* o = a.out + 8 * (size_t)a.it;
    o[0] = loss; for (int j = 0; j < 6; ++j) o[1 + j] = grad[j]; o[7] = 0.f;
    if (!a.step) return;
    scene_camera_adam_step(grad, a.moments, a.lr_t, a.lr_r, a.it, a.pose);
}

// ------------------------------------------------------------------ launchers
template <int EPAD, int W, int NH>
static void scene_pose_obj_t(hipStream_t s, const FusedArgs& a, const ScenePoseObjArgs& p, uint32_t grid, int backward, int build_image) {
    using S = FusedShape<EPAD, W, NH>;
    const uint32_t smem = S::FRAG_BYTES + 512 + S::WAVES * 32;
    if (build_image) hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::N_FRAGS * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    if (!backward) hipLaunchKernelGGL((k_scene_pose_obj<EPAD, W, NH, false, false>), dim3(grid), dim3(256), smem, s, a, p);
    else if (p.level_w) hipLaunchKernelGGL((k_scene_pose_obj<EPAD, W, NH, true, true>), dim3(grid), dim3(256), smem, s, a, p);
    else hipLaunchKernelGGL((k_scene_pose_obj<EPAD, W, NH, false, true>), dim3(grid), dim3(256), smem, s, a, p);
}

template <int EPAD, int W, int NH>
static void scene_window_obj_t(hipStream_t s, const FusedArgs& a, const ScenePoseObjArgs& p, uint32_t grid, uint32_t n_frames, const SceneWinFrame* frames) {
    using S = FusedShape<EPAD, W, NH>;
    const uint32_t smem = S::FRAG_BYTES + 512 + S::WAVES * 32;
    if (p.level_w) hipLaunchKernelGGL((k_scene_window_obj<EPAD, W, NH, true>), dim3(grid, n_frames), dim3(256), smem, s, a, p, frames);
    else hipLaunchKernelGGL((k_scene_window_obj<EPAD, W, NH, false>), dim3(grid, n_frames), dim3(256), smem, s, a, p, frames);
}

void launch_scene_pose_rays(hipStream_t s, const ScenePoseRayArgs& a) {
    if (!a.n_rays || !a.n_objs) return;
    hipLaunchKernelGGL(k_scene_pose_rays, dim3((a.n_rays + 255) / 256), dim3(256), 0, s, a);
}
void launch_scene_pose_obj(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ObjectConst& oc, const uint16_t* params, uint16_t* frag_image,
        int build_image, int backward, uint32_t grid, const ScenePoseObjArgs& p) {
    if (!p.n_rays) return;
    FusedArgs a{}; a.lt = lt; a.nd = nd; a.oc = oc; a.params = params; a.frag_image = frag_image;
    MON_FUSED_DISPATCH(scene_pose_obj_t, s, a, p, grid, backward, build_image);
}
// frames = the pass's first row of the device table; grid = the largest gridc among its n_frames frames
void launch_scene_window_obj(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ObjectConst& oc, const uint16_t* params, uint16_t* frag_image,
        uint32_t grid, uint32_t n_frames, const SceneWinFrame* frames, const ScenePoseObjArgs& p) {
    if (!grid || !n_frames) return;
    FusedArgs a{}; a.lt = lt; a.nd = nd; a.oc = oc; a.params = params; a.frag_image = frag_image;
    MON_FUSED_DISPATCH(scene_window_obj_t, s, a, p, grid, n_frames, frames);
}
uint32_t scene_comp_grad_grid(uint32_t n_rays) { return n_rays < kSceneLossParts ? (n_rays ? n_rays : 1u) : kSceneLossParts; }
void launch_scene_composite_grad(hipStream_t s, const SceneCompGradArgs& a) {
    if (!a.n_rays || !a.n_lists || a.n_lists > kSceneMaxLists) return;
    hipLaunchKernelGGL(k_scene_composite_grad, dim3(scene_comp_grad_grid(a.n_rays)), dim3(64), scene_composite_grad_lds(a.n_lists), s, a);
}
// grid = the largest parts among the pass's n_frames frames
void launch_scene_window_composite(hipStream_t s, const SceneCompGradArgs& a, uint32_t grid, uint32_t n_frames, const SceneWinFrame* frames) {
    if (!grid || !n_frames || !a.n_lists || a.n_lists > kSceneMaxLists) return;
    hipLaunchKernelGGL(k_scene_window_composite, dim3(grid, n_frames), dim3(64), scene_composite_grad_lds(a.n_lists), s, a, frames);
}
void launch_scene_pose_update(hipStream_t s, const ScenePoseUpdateArgs& a) {
    hipLaunchKernelGGL(k_scene_pose_update, dim3(1), dim3(256), 0, s, a);
}

}  // namespace mon
