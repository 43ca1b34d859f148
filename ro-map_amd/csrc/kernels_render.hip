// kernels_render.hip -- k_fused_render (NeRF_Model::Render: one wavefront per pixel ray, 2 x 32 samples) and the occupancy grid kernels of the opt-in
// forward-pass skipping; both evaluate the network with the tile_forward of fused_device.h (gathers + MFMA MLP).
#include "fused_device.h"
#include "scene_device.h"

namespace mon {

// ------------------------------------------------------------------ fused render kernel
// One wavefront per pixel ray, 2S = 64 samples as two 32-sample tiles with a carried transmittance;
// rays that miss the box and tiles behind an opaque prefix are skipped (wave-uniform).
// GenerateRenderInputPoints :593-626 + inference + VolumeRender_Render :1134-1229.
// OCC (empty-space skipping of the render, opt-in per object; a.occ_bits = the render's grid): a sample in a dead cell issues no gathers and contributes
// what a sample of alpha 0 contributes -- its alpha and colour are SELECTED to 0, its interval is the one it always had; a tile with no live sample
// is skipped whole (no MLP, Tc unchanged, tlast = the tile's last t).  stats[0] += the ray's samples in live cells, stats[1] += 2S per ray in the box.
// EMIT (the scene render, mon_scene_render): nothing is composited; the ray's samples go out as a list for k_scene_composite.  The pointers change meaning:
// rgb = t [ray][2S], depth = {alpha, r, g, b} [ray][2S] (float4), stats = the ray's sample count [ray] (0: missed the box; 32 per tile evaluated); mask is
// unused.  The list stops where THIS object's transmittance ends the ray (the scene's is never larger).  A dead tile is emitted with alpha 0 and colour 0.
// The skip counters are not touched.
// KEYED (the scene probe, mon_scene_probe; with EMIT): the ray's jitter indices are key[ray] * 2S + k in place of idx_base + ray * 2S + k; mask = the keys
// (uint32 [ray]), idx_base is unused.
template <int EPAD, int W, int NH, bool OCC = false, bool EMIT = false, bool KEYED = false>
__global__ void __launch_bounds__(256) k_fused_render(FusedArgs a, uint32_t n_rays, uint32_t idx_base, float* __restrict__ rgb, float* __restrict__ depth,
        float* __restrict__ mask, uint32_t* __restrict__ stats) {
    using S = FusedShape<EPAD, W, NH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t* frags = reinterpret_cast<half_t*>(smem);
    LevelLds* llt = reinterpret_cast<LevelLds*>(smem + S::FRAG_BYTES);
    build_fragments<EPAD, W, NH>(frags, llt, a, false);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31;
    const int L = a.nd.L; const uint32_t S2 = 2u * a.oc.S;      // 64
    const half2_t* table = reinterpret_cast<const half2_t*>(a.params + a.nd.n_mlp);
    // (from the argument segment: it ends up in the buffer descriptor, which must be scalar)
    const LevelRegs lregs = load_level_regs_uniform(a.lt, L, lane); const uint32_t table_bytes = a.lt.offset[L] * 4u;
    uint32_t n_live = 0u, n_box = 0u;                                                  // (OCC: this wave's counts, one atomic each at the end)
    for (uint32_t ray = blockIdx.x * S::WAVES + wave; ray < n_rays; ray += gridDim.x * S::WAVES) {
        float o0 = 1.f, o1 = 1.f, o2 = 1.f, od = 0.f, om_ = 0.f;
        uint32_t n_emit = 0u;                                                           // (EMIT) samples written for this ray
        if (a.b.ray_flag[ray]) {
            const float t0 = a.b.ray_t0[ray], t1 = a.b.ray_t1[ray], dtr = (t1 - t0) / (float)S2;
            float Tc = 1.f, r0 = 0.f, r1 = 0.f, r2 = 0.f, dep = 0.f, tlast = 0.f;
            uint32_t lb0 = ~0u, lb1 = ~0u;                                              // (OCC, uniform) the ray's live samples of tile 0 / 1
            const uint32_t jit0 = KEYED ? reinterpret_cast<const uint32_t*>(mask)[ray] * S2 : idx_base + ray * S2;      // the ray's first jitter index
            if constexpr (OCC) {
                // both tiles up front: the count covers every sample in the box, evaluated or behind an opaque first tile (as on the tile path)
#pragma unroll
                for (uint32_t tile = 0; tile < 2u; ++tile) {
                    const uint32_t k = tile * 32u + (uint32_t)n;
                    const float t = fmaf(dtr, (float)k + render_rand(a.oc, jit0 + k), t0);
                    float x[3];
#pragma unroll
                    for (int d = 0; d < 3; ++d) { const float p = fmaf(t, a.b.ray_d[3 * ray + d], a.b.ray_o[3 * ray + d]);
                        x[d] = (p - a.oc.aabb.mn[d]) / (a.oc.aabb.mx[d] - a.oc.aabb.mn[d]); }
                    const uint32_t bits = (uint32_t)__ballot(occ_cell_live(a.occ_bits, x));
                    if (tile == 0u) lb0 = bits; else lb1 = bits;
                }
                n_live += (uint32_t)__popc(lb0) + (uint32_t)__popc(lb1); n_box += S2;
            }
            for (uint32_t tile = 0; tile < 2u; ++tile) {
                if (Tc < kTransmittanceEps) break;
                const uint32_t k = tile * 32u + (uint32_t)n;
                const float t = fmaf(dtr, (float)k + render_rand(a.oc, jit0 + k), t0);
                float x[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) { const float p = fmaf(t, a.b.ray_d[3 * ray + d], a.b.ray_o[3 * ray + d]);
                    x[d] = (p - a.oc.aabb.mn[d]) / (a.oc.aabb.mx[d] - a.oc.aabb.mn[d]); }
                const uint32_t lw = tile ? lb1 : lb0;
                if (OCC && lw == 0u) {                                                  // a dead tile: alpha 0 everywhere, Tc unchanged
                    if constexpr (EMIT) {
                        if (lane < 32) { rgb[(size_t)ray * S2 + k] = t; reinterpret_cast<float4*>(depth)[(size_t)ray * S2 + k] = make_float4(0.f, 0.f, 0.f, 0.f); }
                        n_emit += 32u;
                    }
                    tlast = lane_bcast(t, 31); continue;
                }
                const bool live = !OCC || ((lw >> n) & 1u) != 0u;
                TileState<EPAD, W, NH> ts;
                if constexpr (OCC) {                                                    // dead lanes issue no gathers: their features are 0
                    const __amdgpu_buffer_rsrc_t rsrc = table_rsrc(table, table_bytes);
                    GatherWindow<EPAD, W, NH> g;
                    encode_begin<EPAD, W, NH, true>(g, lregs, rsrc, x, lane, live);
                    encode_finish<EPAD, W, NH, true>(ts, g, lregs, rsrc, x, lane, L, live);
                    mlp_forward<EPAD, W, NH>(ts, frags, lane);
                } else tile_forward<EPAD, W, NH>(ts, frags, lregs, table, table_bytes, L, x, lane);
                const float sigma = __expf(ts.out4[3]);
                const float c0 = OCC && !live ? 0.f : logistic_f(ts.out4[0]), c1 = OCC && !live ? 0.f : logistic_f(ts.out4[1]),
                            c2 = OCC && !live ? 0.f : logistic_f(ts.out4[2]);                 // (selects)
                float tprev = lane_prev(t, tlast); if (n == 0) tprev = tlast;
                const float alpha = OCC && !live ? 0.f : 1.f - __expf(-sigma * (t - tprev)), omv = 1.f - alpha;
                if constexpr (EMIT) {
                    if (lane < 32) { rgb[(size_t)ray * S2 + k] = t; reinterpret_cast<float4*>(depth)[(size_t)ray * S2 + k] = make_float4(alpha, c0, c1, c2); }
                    n_emit += 32u;
                }
                const float tincl = scan_mul32(omv) * Tc;
                float T = lane_prev(tincl, Tc); if (n == 0) T = Tc;
                const bool active = T >= kTransmittanceEps;
                const int nact = __popc((uint32_t)__ballot(active));
                const float wgt = active ? alpha * T : 0.f;
                r0 += lane_bcast(scan_add32(wgt * c0), 31); r1 += lane_bcast(scan_add32(wgt * c1), 31); r2 += lane_bcast(scan_add32(wgt * c2), 31);
                dep += lane_bcast(scan_add32(wgt * t), 31);
                Tc = (nact > 0) ? lane_bcast(tincl, nact > 0 ? nact - 1 : 0) : Tc;      // all 64 lanes carry half-wave 0's state (uniform control flow)
                tlast = lane_bcast(t, 31);
            }
            if (1.f - Tc > 0.5f) { o0 = r0 + Tc; o1 = r1 + Tc; o2 = r2 + Tc; od = dep / a.b.ray_dn[ray]; om_ = 1.f; }      // :1213-1220
        }
        if constexpr (EMIT) { if (lane == 0) stats[ray] = n_emit; }
        else if (lane == 0) { rgb[3 * ray] = o0; rgb[3 * ray + 1] = o1; rgb[3 * ray + 2] = o2; depth[ray] = od; mask[ray] = om_; }
    }
    if constexpr (OCC && !EMIT) if (lane == 0 && n_box) { atomicAdd(stats, n_live); atomicAdd(stats + 1, n_box); }
}

// ------------------------------------------------------------------ occupancy grid (N1: forward-pass skipping, default off)
// BASELINE.json's north star names occupancy-grid skipping; the reference has none (it always takes 32 uniform samples inside the box,
// nerf_model.cu:536-566), so the feature is opt-in (mon_config::occupancy_skip) and the parity tests run without it.  A kOccRes^3 bit grid over
// the object's box is refreshed from the CURRENT training weights every kOccInterval iterations after a warm-up: one wavefront evaluates the
// network's raw density at the centres of 32 cells (the same tile_forward as training) and ballots "density above the threshold" into one
// word; a second pass dilates by one cell in every direction.  k_fused_train then skips the gathers of samples in empty cells.
template <int EPAD, int W, int NH>
__global__ void __launch_bounds__(256) k_occ_density(FusedArgs a, float raw_threshold, uint32_t* __restrict__ bits_out) {
    using S = FusedShape<EPAD, W, NH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t* frags = reinterpret_cast<half_t*>(smem);
    LevelLds* llt = reinterpret_cast<LevelLds*>(smem + S::FRAG_BYTES);
    build_fragments<EPAD, W, NH>(frags, llt, a, false);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31;
    const half2_t* table = reinterpret_cast<const half2_t*>(a.params + a.nd.n_mlp);
    constexpr uint32_t n_words = kOccRes * kOccRes * kOccRes / 32;
    const LevelRegs lregs = load_level_regs_uniform(a.lt, a.nd.L, lane); const uint32_t table_bytes = a.lt.offset[a.nd.L] * 4u;
    for (uint32_t word = blockIdx.x * S::WAVES + wave; word < n_words; word += gridDim.x * S::WAVES) {
        const uint32_t cell = word * 32u + (uint32_t)n, cx = cell % kOccRes, cy = (cell / kOccRes) % kOccRes, cz = cell / (kOccRes * kOccRes);
        const float x[3] = { ((float)cx + 0.5f) / (float)kOccRes, ((float)cy + 0.5f) / (float)kOccRes, ((float)cz + 0.5f) / (float)kOccRes };
        TileState<EPAD, W, NH> ts;
        tile_forward<EPAD, W, NH>(ts, frags, lregs, table, table_bytes, a.nd.L, x, lane);
        // raw channel 3 = log density (network_to_density = exp, nerf_model.cu:49)
        const uint32_t occ = (uint32_t)__ballot(lane < 32 && ts.out4[3] > raw_threshold);
        if (lane == 0) bits_out[word] = occ;
    }
}
// a cell stays live if it or any of its 26 neighbours is occupied (the network is only sampled at cell centres)
__global__ void __launch_bounds__(256) k_occ_dilate(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    constexpr int WPR = kOccRes / 32;                                                   // words per x row
    const uint32_t word = blockIdx.x * blockDim.x + threadIdx.x;
    if (word >= (uint32_t)(kOccRes * kOccRes * WPR)) return;
    const int wx = (int)(word % WPR), cy = (int)((word / WPR) % kOccRes), cz = (int)(word / (WPR * kOccRes));
    uint32_t acc = 0u;
    for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) {
        const int y = cy + dy, z = cz + dz; if (y < 0 || y >= kOccRes || z < 0 || z >= kOccRes) continue;
        const uint32_t* row = in + ((size_t)z * kOccRes + y) * WPR;
        const uint32_t w = row[wx], wl = wx > 0 ? row[wx - 1] : 0u, wr = wx + 1 < WPR ? row[wx + 1] : 0u;
        acc |= w | (w << 1) | (w >> 1) | (wl >> 31) | (wr << 31);
    }
    out[word] = acc;
}
template <int EPAD, int W, int NH>
static void occ_update_t(hipStream_t s, const FusedArgs& a, float raw_threshold, uint32_t* tmp, uint32_t* bits) {
    using S = FusedShape<EPAD, W, NH>;
    constexpr uint32_t n_words = kOccRes * kOccRes * kOccRes / 32;
    hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::F_WOT * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    hipLaunchKernelGGL((k_occ_density<EPAD, W, NH>), dim3(n_words / S::WAVES), dim3(256), S::FRAG_BYTES + S::LT_BYTES, s, a, raw_threshold, tmp);
    hipLaunchKernelGGL(k_occ_dilate, dim3((n_words + 255) / 256), dim3(256), 0, s, tmp, bits);
}
template <int EPAD, int W, int NH>
static void fused_render_t(hipStream_t s, const FusedArgs& a, uint32_t n_rays, uint32_t idx_base, float* rgb, float* depth, float* mask, uint32_t* stats) {
    using S = FusedShape<EPAD, W, NH>;
    const uint32_t smem = S::FRAG_BYTES + S::LT_BYTES;
    uint32_t grid = (n_rays + 3) / 4; if (grid > 2048u) grid = 2048u;
    // first chunk of a render call
    if (a.keep_zero & 1u) hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::F_WOT * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    if (a.occ_bits) hipLaunchKernelGGL((k_fused_render<EPAD, W, NH, true>), dim3(grid), dim3(256), smem, s, a, n_rays, idx_base, rgb, depth, mask, stats);
    else hipLaunchKernelGGL((k_fused_render<EPAD, W, NH>), dim3(grid), dim3(256), smem, s, a, n_rays, idx_base, rgb, depth, mask, stats);
}

template <int EPAD, int W, int NH>
static void fused_emit_t(hipStream_t s, const FusedArgs& a, uint32_t n_rays, uint32_t idx_base, float* t, float* attr, uint32_t* cnt, const uint32_t* keys) {
    using S = FusedShape<EPAD, W, NH>;
    const uint32_t smem = S::FRAG_BYTES + S::LT_BYTES;
    uint32_t grid = (n_rays + 3) / 4; if (grid > 2048u) grid = 2048u;
    if (a.keep_zero & 1u) hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::F_WOT * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    float* kp = reinterpret_cast<float*>(const_cast<uint32_t*>(keys));                 // (KEYED reads its keys through the unused mask pointer)
    if (keys) {
        if (a.occ_bits) hipLaunchKernelGGL((k_fused_render<EPAD, W, NH, true, true, true>), dim3(grid), dim3(256), smem, s, a, n_rays, 0u, t, attr, kp, cnt);
        else hipLaunchKernelGGL((k_fused_render<EPAD, W, NH, false, true, true>), dim3(grid), dim3(256), smem, s, a, n_rays, 0u, t, attr, kp, cnt);
    }
    else if (a.occ_bits) hipLaunchKernelGGL((k_fused_render<EPAD, W, NH, true, true>), dim3(grid), dim3(256), smem, s, a, n_rays, idx_base, t, attr, nullptr, cnt);
    else hipLaunchKernelGGL((k_fused_render<EPAD, W, NH, false, true>), dim3(grid), dim3(256), smem, s, a, n_rays, idx_base, t, attr, nullptr, cnt);
}

// ------------------------------------------------------------------ scene render: merge-composite of the objects' sample lists
// One wavefront (= one workgroup) per pixel ray.  List k of the ray holds cnt[k * cap + ray] samples (<= 2S, ascending in t) at (k * cap + ray) * 2S:
// t in `tl`, {alpha, r, g, b} in `attr`.  The ray's non-empty lists are compacted into LDS with their first and last t; every sample's place in the merged
// order is counted: its index in its own list + the samples of each other list that come before it (ties to the lower list index) -- the whole list or
// none where the t ranges do not overlap (always the case for disjoint boxes), a binary search of that list where they do.  The merged order (list, index)
// goes to LDS, and the sequence is composited front to back in blocks of 64 with a carried transmittance.  Each half-wave scans its 32 samples as
// k_fused_render scans a tile, and the sums are added half by half, so one object's list composites to exactly that render's arithmetic.  Per-list weight
// sums (one wave reduction per list present in a block) give the instance.
__global__ void __launch_bounds__(64) k_scene_composite(uint32_t n_rays, uint32_t n_lists, uint32_t cap, const float* __restrict__ tl,
        const float4* __restrict__ attr, const uint32_t* __restrict__ cnt, const float* __restrict__ dn, float* __restrict__ out_rgb,
        float* __restrict__ out_depth, float* __restrict__ out_opacity, int32_t* __restrict__ out_instance) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SceneLds s = scene_lds(smem, n_lists);
    const int lane = threadIdx.x;
    for (uint32_t ray = blockIdx.x; ray < n_rays; ray += gridDim.x) {
        uint32_t na, n_tot;
        scene_merge_lists(s, ray, n_lists, cap, tl, cnt, lane, na, n_tot);
        SceneWalk w;
        scene_composite_walk<false>(s, ray, cap, na, n_tot, tl, attr, lane, w);
        if (lane == 0) scene_composite_store(s, ray, na, w, dn, out_rgb, out_depth, out_opacity, out_instance);
        __syncthreads();
    }
}


void launch_fused_render(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const BatchPtrs& b, const ObjectConst& oc,
        uint32_t n_rays, uint32_t idx_base, float* rgb, float* depth, float* mask, uint16_t* frag_image, int build_image, const RenderSkipArgs& skip) {
    // `keep_zero` doubles as "build the fragment image first" on the host side of the render path
    FusedArgs a{ lt, nd, oc, b, params, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, frag_image, build_image ? 1u : 0u };
    a.occ_bits = skip.bits;
    MON_FUSED_DISPATCH(fused_render_t, s, a, n_rays, idx_base, rgb, depth, mask, skip.stats);
}


void launch_fused_render_emit(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const BatchPtrs& b, const ObjectConst& oc,
        uint32_t n_rays, uint32_t idx_base, float* t, float* attr, uint32_t* cnt, uint16_t* frag_image, int build_image, const uint32_t* skip_bits,
        const uint32_t* keys) {
    FusedArgs a{ lt, nd, oc, b, params, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, frag_image, build_image ? 1u : 0u };
    a.occ_bits = skip_bits;
    MON_FUSED_DISPATCH(fused_emit_t, s, a, n_rays, idx_base, t, attr, cnt, keys);
}

void launch_scene_composite(hipStream_t s, uint32_t n_rays, uint32_t n_lists, uint32_t cap, const float* t, const float* attr, const uint32_t* cnt,
        const float* dn, float* rgb, float* depth, float* opacity, int32_t* instance) {
    if (!n_rays || !n_lists || n_lists > kSceneMaxLists) return;
    hipLaunchKernelGGL(k_scene_composite, dim3(scene_composite_grid(n_rays)), dim3(64), scene_composite_lds(n_lists), s, n_rays, n_lists, cap, t,
            reinterpret_cast<const float4*>(attr), cnt, dn, rgb, depth, opacity, instance);
}


void launch_occupancy_update(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const ObjectConst& oc, uint16_t* frag_image,
        float raw_threshold, uint32_t* tmp, uint32_t* bits) {
    FusedArgs a{}; a.lt = lt; a.nd = nd; a.oc = oc; a.params = params; a.frag_image = frag_image;
    MON_FUSED_DISPATCH(occ_update_t, s, a, raw_threshold, tmp, bits);
}

}  // namespace mon
