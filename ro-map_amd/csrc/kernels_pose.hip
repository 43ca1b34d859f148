// kernels_pose.hip -- object pose refinement through a trained field (mon_object_pose_loss / mon_object_refine_pose): the pose's rays, the loss and its
// gradient with respect to the sample positions (forward + composite backward + MLP backward on MFMA + hash-grid position gradient), and the Adam step on
// the twist.  Instantiated for the fused shapes only (MON_FUSED_DISPATCH); the network runs through the tile_forward / mlp_forward of fused_device.h.
// The objective is stated in include/mon_core.h and DESIGN.md 3.4d.
#include <type_traits>
#include "pose_device.h"

namespace mon {

// ------------------------------------------------------------------ k_pose_rays
// One thread per drawn ray.  Pixel p of the union of the boxes (box b holds [prefix[b], prefix[b + 1])): ray i itself (every pixel) or a draw of stream
// kStreamPoseXY.  Reads the pose from the device (pose[16], world -> object), builds the ray mon_object_render builds for that pixel, intersects it with the
// box and fetches the target.  Record (4 x float4): {o, t0} {d, t1} {|camera ray|, hit, m*, d*} {c*, jitter index base (bits)}.
// The draw (include/mon_core.h): z = the key's 64-bit mix; p = ((z >> 40) total) >> 24 for total <= 2^24 (rand01's 24 bits), else ((z >> 32) total) >> 32
// -- a step of total / 2^32 < 1 pixel between consecutive 32-bit values, so every pixel of a union of up to 2^28 can be drawn.
__global__ void __launch_bounds__(256) k_pose_rays(PoseRayArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_rays) return;
    uint32_t p = i;
    if (a.drawn) {
        const uint64_t z = rand_mix(a.seed, kStreamPoseXY, a.iteration, i);
        p = a.total <= (1u << 24) ? (uint32_t)(((z >> 40) * a.total) >> 24) : (uint32_t)(((z >> 32) * a.total) >> 32);
    }
    uint32_t lo = 0u, hi = a.n_obs - 1u;                                                // the box: last b with prefix[b] <= p
    while (lo < hi) { const uint32_t mid = (lo + hi + 1u) >> 1; if (a.prefix[mid] <= p) lo = mid; else hi = mid - 1u; }
    const mon_frame_bbox box = a.boxes[lo];
    const uint32_t q = p - a.prefix[lo], x = box.x + q % box.w, y = box.y + q / box.w;
    const size_t pix = ((size_t)box.FrameId * a.ds.K.H + y) * a.ds.K.W + x;
    const uint32_t rgba = a.ds.rgba[pix];
    const float mstar = (rgba >> 24) == a.instance_id ? 1.f : 0.f;
    const float dstar = a.ds.depth ? a.ds.depth[pix] : 0.f;
    float o[3], d[3], dn, t0 = 0.f, t1 = 0.f;
    pixel_ray(a.ds.K, (float)x, (float)y, a.ds.poses + (size_t)box.FrameId * 16, a.pose, false, o, d, dn);
    const bool hit = ray_intersect(a.aabb, o, d, t0, t1);
    const uint32_t base = a.drawn ? i * 64u : q * 64u;                                  // (2S = 64: the fused shapes)
    float4* r = a.rec + 4 * (size_t)i;
    r[0] = make_float4(o[0], o[1], o[2], fmaxf(t0, 0.0f));
    r[1] = make_float4(d[0], d[1], d[2], t1);
    r[2] = make_float4(dn, hit ? 1.f : 0.f, mstar, dstar);
    r[3] = make_float4((float)(rgba & 0xffu) / 255.0f, (float)((rgba >> 8) & 0xffu) / 255.0f, (float)((rgba >> 16) & 0xffu) / 255.0f,
            __builtin_bit_cast(float, base));
}

// ------------------------------------------------------------------ k_pose_grad

// One wavefront per ray, its 2S = 64 samples as two 32-sample tiles (k_fused_render's placement, jitter rand01(seed, stream, step, base + k), alpha,
// colour and early cut).  Forward of both tiles kept in registers -> per-ray loss -> composite backward (T_{k+1} form, suffix scans) -> dL/dO (scaled by a
// power of two so that fp16 neither overflows nor flushes) -> MLP backward on MFMA (the transposed fragments training uses) -> dL/dE -> position gradient
// from a second gather of each level's corners.  Per lane: sum of g and x × g over its samples (its half-wave's levels); per wave: the ray losses; per
// workgroup: one partial row of 8 floats {g, x × g, loss, 0} -- no atomics, so the sums are the same from run to run.
// LW (mon_object_pose_loss_levels / the coarse-to-fine schedule): each level's term of g scaled by p.level_w[l]; the arguments of LW = false stay PoseGradArgs.
template <int EPAD, int W, int NH, bool LW>
__global__ void __launch_bounds__(256) k_pose_grad(FusedArgs a, std::conditional_t<LW, PoseGradArgsLW, PoseGradArgs> p) {
    using S = FusedShape<EPAD, W, NH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t* frags = reinterpret_cast<half_t*>(smem);
    LevelLds* llt = reinterpret_cast<LevelLds*>(smem + S::FRAG_BYTES);
    float* red = reinterpret_cast<float*>(smem + S::FRAG_BYTES + 512);                  // [WAVES][8]
    build_fragments<EPAD, W, NH>(frags, llt, a, true);
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
    float acc[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f }, loss_acc = 0.f;
    for (uint32_t ray = blockIdx.x * S::WAVES + wave; ray < p.n_rays; ray += gridDim.x * S::WAVES) {
        const float4* rr = p.rec + 4 * (size_t)ray;
        const float4 r0 = rr[0], r1 = rr[1], r2 = rr[2], r3 = rr[3];
        const float ro[3] = { r0.x, r0.y, r0.z }, rd[3] = { r1.x, r1.y, r1.z }, cs[3] = { r3.x, r3.y, r3.z };
        const float t0 = r0.w, t1 = r1.w, dn = r2.x, mstar = r2.z, dstar = r2.w;
        const bool hit = r2.y != 0.f; const uint32_t base = __builtin_bit_cast(uint32_t, r3.w);
        const bool dep_on = p.w_depth != 0.f && mstar != 0.f && dstar > 0.f;
        if (!hit) {                                                                     // O = D = r = 0
            loss_acc += p.w_mask * mstar * mstar + (dep_on ? p.w_depth * huber_f(-dstar, p.huber) : 0.f);
            if (p.dbg_x && lane < 32)
                for (int tile = 0; tile < 2; ++tile) { const size_t s = (size_t)ray * 64u + tile * 32u + (uint32_t)n;
                    for (int d = 0; d < 3; ++d) { p.dbg_x[3 * s + d] = 0.f; p.dbg_g[3 * s + d] = 0.f; }
                    for (int c = 0; c < 4; ++c) p.dbg_raw[4 * s + c] = 0.f; }
            continue;
        }
        const float dtr = (t1 - t0) / 64.0f;
        // ---- forward, both tiles (the second only where the first left T >= eps, as the render does)
        TileState<EPAD, W, NH> ts[2];
        float tk[2], xk[2][3], pk[2][3], dtk[2], sig[2], col[2][3], wgt[2], tinc[2];
        bool act[2];
        bool ev1 = false;
        float Tc = 1.f, tlast = 0.f;
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
            if (tile == 1) ev1 = Tc >= kTransmittanceEps;
            const uint32_t k = tile * 32u + (uint32_t)n;
            const float t = fmaf(dtr, (float)k + rand01(p.seed, p.stream, p.step, base + k), t0);
            tk[tile] = t;
#pragma unroll
            for (int d = 0; d < 3; ++d) { const float q = fmaf(t, rd[d], ro[d]); pk[tile][d] = q; xk[tile][d] = (q - a.oc.aabb.mn[d]) / ext[d]; }
            if (tile == 1 && !ev1) { wgt[1] = 0.f; act[1] = false; tinc[1] = Tc; dtk[1] = 0.f; sig[1] = 0.f; col[1][0] = col[1][1] = col[1][2] = 0.f; break; }
            tile_forward<EPAD, W, NH>(ts[tile], frags, lregs, table, table_bytes, L, xk[tile], lane);
            const float sigma = __expf(ts[tile].out4[3]);
            const float c0 = logistic_f(ts[tile].out4[0]), c1 = logistic_f(ts[tile].out4[1]), c2 = logistic_f(ts[tile].out4[2]);
            float tprev = lane_prev(t, tlast); if (n == 0) tprev = tlast;
            const float dt = t - tprev;
            const float alpha = 1.f - __expf(-sigma * dt), omv = 1.f - alpha;
            const float tincl = scan_mul32(omv) * Tc;
            float T = lane_prev(tincl, Tc); if (n == 0) T = Tc;
            const bool active = T >= kTransmittanceEps;
            const int nact = __popc((uint32_t)__ballot(active));
            sig[tile] = sigma; dtk[tile] = dt; col[tile][0] = c0; col[tile][1] = c1; col[tile][2] = c2;
            wgt[tile] = active ? alpha * T : 0.f; act[tile] = active; tinc[tile] = tincl;
            Tc = (nact > 0) ? lane_bcast(tincl, nact > 0 ? nact - 1 : 0) : Tc;
            tlast = lane_bcast(t, 31);
        }
        // ---- per-ray quantities and loss
        float res[3] = { 0.f, 0.f, 0.f }, dsum = 0.f;
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
#pragma unroll
            for (int c = 0; c < 3; ++c) res[c] += lane_bcast(scan_add32(wgt[tile] * (col[tile][c] - cs[c])), 31);
            dsum += lane_bcast(scan_add32(wgt[tile] * tk[tile]), 31);
        }
        const float O = 1.f - Tc, D = dsum / dn;
        const float l = p.w_rgb * mstar * (res[0] * res[0] + res[1] * res[1] + res[2] * res[2]) / 3.f + p.w_mask * (O - mstar) * (O - mstar)
                + (dep_on ? p.w_depth * huber_f(D - dstar, p.huber) : 0.f);
        loss_acc += l;
        const float Gc[3] = { p.w_rgb * mstar * 2.f * res[0] / 3.f, p.w_rgb * mstar * 2.f * res[1] / 3.f, p.w_rgb * mstar * 2.f * res[2] / 3.f };
        const float GO = 2.f * p.w_mask * (O - mstar);
        const float GD = dep_on ? p.w_depth * clamp_f(D - dstar, -p.huber, p.huber) / dn : 0.f;
        // ---- composite backward: dL/dsigma_k = dt_k (T_{k+1} q_k - sum_{j>k} w_j q_j + G_O T_end), q = G . (c - c*) + G_D t
        float qk[2], sfx_in[2], tot[2];
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
            qk[tile] = Gc[0] * (col[tile][0] - cs[0]) + Gc[1] * (col[tile][1] - cs[1]) + Gc[2] * (col[tile][2] - cs[2]) + GD * tk[tile];
            sfx_in[tile] = suffix_add32(wgt[tile] * qk[tile]);
            tot[tile] = lane_bcast(sfx_in[tile], 0);
        }
        float dO[2][4]; float mx = 0.f;
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
            float sfx = lane_next(sfx_in[tile], 0.f); if (n == 31) sfx = 0.f;
            if (tile == 0) sfx += tot[1];
            const float A = tinc[tile] * qk[tile] - sfx + GO * Tc;
            const bool on = act[tile] && h == 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) dO[tile][c] = on ? Gc[c] * wgt[tile] * (col[tile][c] * (1.f - col[tile][c])) : 0.f;
            dO[tile][3] = on ? A * dtk[tile] * sig[tile] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) mx = fmaxf(mx, fabsf(dO[tile][c]));
        }
        mx = lane_bcast(max32(mx), 31);
        // power-of-two scale: the largest |dL/dO| of the ray lands in [32, 64) -- exact to undo
        int e = 0; (void)frexpf(mx, &e);
        const float up = ldexpf(1.f, 6 - e), down = ldexpf(1.f, e - 6);
        // ---- backward per evaluated tile
#pragma unroll
        for (int tile = 0; tile < 2; ++tile) {
            if (tile == 1 && !ev1) break;
            float gl[3] = { 0.f, 0.f, 0.f };
            if (mx > 0.f) {
                pose_tile_backward<EPAD, W, NH, LW>(gl, ts[tile], frags, lregs, rsrc, xk[tile], dO[tile], up, down, ext, lane, h, L, lw);
            }
            acc[0] += gl[0]; acc[1] += gl[1]; acc[2] += gl[2];
            const float* x = pk[tile];
            acc[3] += x[1] * gl[2] - x[2] * gl[1]; acc[4] += x[2] * gl[0] - x[0] * gl[2]; acc[5] += x[0] * gl[1] - x[1] * gl[0];
            if (p.dbg_x) {
                float gf[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) gf[d] = gl[d] + __shfl_xor(gl[d], 32);
                if (lane < 32) {
                    const size_t s = (size_t)ray * 64u + tile * 32u + (uint32_t)n;
                    for (int d = 0; d < 3; ++d) { p.dbg_x[3 * s + d] = x[d]; p.dbg_g[3 * s + d] = gf[d] * p.inv_n; }
                    for (int c = 0; c < 4; ++c) p.dbg_raw[4 * s + c] = ts[tile].out4[c];
                }
            }
        }
        if (p.dbg_x && !ev1 && lane < 32) {
            const size_t s = (size_t)ray * 64u + 32u + (uint32_t)n;
            for (int d = 0; d < 3; ++d) { p.dbg_x[3 * s + d] = pk[1][d]; p.dbg_g[3 * s + d] = 0.f; }
            for (int c = 0; c < 4; ++c) p.dbg_raw[4 * s + c] = 0.f;
        }
    }
    // ---- wave sums, then the workgroup's row in wave order
    float tot6[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) tot6[j] = wave_sum(acc[j]);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) red[wave * 8 + j] = tot6[j];
        red[wave * 8 + 6] = loss_acc; red[wave * 8 + 7] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        float s = 0.f;
        for (int w = 0; w < S::WAVES; ++w) s += red[w * 8 + threadIdx.x];
        p.partials[(size_t)blockIdx.x * 8 + threadIdx.x] = s;
    }
}

// ------------------------------------------------------------------ k_pose_update

// One workgroup: the partial rows summed in a fixed order (32 strided groups per column, then the groups in order) -> loss, grad6 (both x 1/N) into
// out[8 * it] (loss, grad6) and trace[it]; step != 0: Adam on the twist (moments[12]: m, v; bias correction by the step number) and pose <- exp(delta^) pose,
// its rotation re-orthonormalised (Gram-Schmidt on the columns).
__global__ void __launch_bounds__(256) k_pose_update(const float* __restrict__ partials, uint32_t n_parts, float inv_n, float* __restrict__ out,
        float* __restrict__ trace, uint32_t it, int step, float lr_t, float lr_r, float* __restrict__ pose, float* __restrict__ moments) {
    __shared__ float part[32][8];
    const uint32_t col = threadIdx.x & 7u, grp = threadIdx.x >> 3;
    float s = 0.f;
    for (uint32_t b = grp; b < n_parts; b += 32u) s += partials[(size_t)b * 8 + col];
    part[grp][col] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float v[7];
    for (int j = 0; j < 7; ++j) { float q = 0.f; for (int g = 0; g < 32; ++g) q += part[g][j]; v[j] = q * inv_n; }
    float* o = out + 8 * (size_t)it;
    o[0] = v[6]; for (int j = 0; j < 6; ++j) o[1 + j] = v[j]; o[7] = 0.f;
    if (trace) trace[it] = v[6];
    if (!step) return;
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const float tt = (float)(it + 1u);
    const float c1 = 1.f - powf(b1, tt), c2 = 1.f - powf(b2, tt);
    float delta[6];
    for (int j = 0; j < 6; ++j) {
        const float g = v[j];
        const float m = b1 * moments[j] + (1.f - b1) * g, w = b2 * moments[6 + j] + (1.f - b2) * g * g;
        moments[j] = m; moments[6 + j] = w;
        const float lr = j < 3 ? lr_t : lr_r;
        delta[j] = -lr * (m / c1) / (sqrtf(w / c2) + eps);
    }
    float Rd[9], td[3];
    se3_exp(delta, Rd, td);
    float Rn[9], tn[3];
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) {
        float q = 0.f; for (int k = 0; k < 3; ++k) q += Rd[k * 3 + r] * pose[c * 4 + k]; Rn[c * 3 + r] = q; }
    for (int r = 0; r < 3; ++r) tn[r] = Rd[r] * pose[12] + Rd[3 + r] * pose[13] + Rd[6 + r] * pose[14] + td[r];
    // Gram-Schmidt: column 0 normalised, column 1 made orthogonal to it and normalised, column 2 = c0 x c1
    float* a0 = Rn; float* a1 = Rn + 3; float* a2 = Rn + 6;
    float nn = rsqrtf(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]); for (int r = 0; r < 3; ++r) a0[r] *= nn;
    const float dp = a0[0] * a1[0] + a0[1] * a1[1] + a0[2] * a1[2]; for (int r = 0; r < 3; ++r) a1[r] -= dp * a0[r];
    nn = rsqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]); for (int r = 0; r < 3; ++r) a1[r] *= nn;
    a2[0] = a0[1] * a1[2] - a0[2] * a1[1]; a2[1] = a0[2] * a1[0] - a0[0] * a1[2]; a2[2] = a0[0] * a1[1] - a0[1] * a1[0];
    for (int c = 0; c < 3; ++c) { for (int r = 0; r < 3; ++r) pose[c * 4 + r] = Rn[c * 3 + r]; pose[c * 4 + 3] = 0.f; }
    for (int r = 0; r < 3; ++r) pose[12 + r] = tn[r];
    pose[15] = 1.f;
}

template <int EPAD, int W, int NH>
static void pose_grad_t(hipStream_t s, const FusedArgs& a, const PoseGradArgs& p, uint32_t grid, int build_image, const float* level_w) {
    using S = FusedShape<EPAD, W, NH>;
    if (build_image) hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::N_FRAGS * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    if (level_w) {
        PoseGradArgsLW q; static_cast<PoseGradArgs&>(q) = p; q.level_w = level_w;
        hipLaunchKernelGGL((k_pose_grad<EPAD, W, NH, true>), dim3(grid), dim3(256), S::FRAG_BYTES + 512 + S::WAVES * 32, s, a, q);
    } else {
        hipLaunchKernelGGL((k_pose_grad<EPAD, W, NH, false>), dim3(grid), dim3(256), S::FRAG_BYTES + 512 + S::WAVES * 32, s, a, p);
    }
}

uint32_t pose_grad_grid(uint32_t n_rays) { uint32_t g = (n_rays + 3u) / 4u; if (g > kPoseMaxGrid) g = kPoseMaxGrid; return g ? g : 1u; }

void launch_pose_rays(hipStream_t s, const PoseRayArgs& a) {
    if (!a.n_rays) return;
    hipLaunchKernelGGL(k_pose_rays, dim3((a.n_rays + 255) / 256), dim3(256), 0, s, a);
}
void launch_pose_grad(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ObjectConst& oc, const uint16_t* params, uint16_t* frag_image,
        int build_image, const PoseGradArgs& p, const float* level_w) {
    FusedArgs a{}; a.lt = lt; a.nd = nd; a.oc = oc; a.params = params; a.frag_image = frag_image;
    const uint32_t grid = pose_grad_grid(p.n_rays);
    MON_FUSED_DISPATCH(pose_grad_t, s, a, p, grid, build_image, level_w);
}
void launch_pose_update(hipStream_t s, const float* partials, uint32_t n_parts, float inv_n, float* out, float* trace, uint32_t it, int step, float lr_t,
        float lr_r, float* pose, float* moments) {
    hipLaunchKernelGGL(k_pose_update, dim3(1), dim3(256), 0, s, partials, n_parts, inv_n, out, trace, it, step, lr_t, lr_r, pose, moments);
}

}  // namespace mon
