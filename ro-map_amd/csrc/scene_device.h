// scene_device.h -- device code shared by the merge-composite kernels of the scene render (k_scene_composite, kernels_render.hip), of camera refinement
// (k_scene_composite_grad, k_scene_window_composite, kernels_scene_pose.hip) and of batched pose scoring (k_scene_composite_loss, kernels_scene_score.hip):
// the LDS of one ray (SceneLds, its bytes in model.h); the compaction of one ray's non-empty sample lists and the merged order of their samples; the steps of
// one block of 64 merged samples, written once for every loop over the blocks -- scene_fetch (a position of the merged order -> the sample and where it
// lies), scene_transmittance, scene_block_add, scene_list_weights, scene_carry; the composite walk of the merged sequence and its outputs, shared by the
// render's composite and the probe's (k_scene_probe_composite, kernels_scene_probe.hip), which adds the first hit, and the ray cast's
// (k_scene_cast_composite, kernels_scene_cast.hip), which places the hit inside its sample's interval; one drawn ray's targets and per-object records under a
// camera pose; the composite forward of one ray with its loss (the reverse sweep over the same blocks is scene_composite_grad_walk, kernels_scene_pose.hip);
// the tail of an evaluation (rows -> camera-frame gradient, the Adam steps on a camera and on an object twist) shared with window refinement
// (kernels_scene_window.hip).
#pragma once
#include "fused_device.h"
#include "pose_device.h"

namespace mon {

// The longest merged sequence 16 lists can make.  Up to here a block's transmittance is k_fused_render's tile scan (scan_mul32), which fixes the bits of
// every render of up to 16 objects and makes one object's list composite to its own render.  That scan loses the term a b of every product
// (1 - a)(1 - b) with a, b < 2^-12, so T comes out low by an amount that grows with the sample count (3.4e-5 in opacity at 16 384 samples of alpha 1e-4);
// longer sequences take scan_mul32_comp, whose block product is rounded once.  Wave-uniform: n_tot is the ray's.
constexpr uint32_t kSceneLongSeq = 16u * kSceneListLen;
__device__ __forceinline__ float scene_scan_mul32(float omv, uint32_t n_tot) { return n_tot > kSceneLongSeq ? scan_mul32_comp(omv) : scan_mul32(omv); }

// The dynamic LDS of one ray's merge and composite: the arrays scene_lds_word (model.h) places, which also gives the launchers their byte counts.
struct SceneLds {
    uint16_t* perm;                                                                     // [kSceneListLen * n_lists] merged order: scene_perm_pack(compact list, slot)
    uint32_t *id, *c;                                                                   // [n_lists] compact list -> list; its count
    float *tf, *tl, *w;                                                                 // [n_lists] its first t; its last t; its summed weight W
    // GRAD: [n_lists] its 2 w_mask (W - m*); the entry transmittance of each 64-sample block.  n_tot <= kSceneListLen * n_lists, so the ray's
    // ceil(n_tot / 64) blocks are at most n_lists.
    float *q, *T;
};
template <bool GRAD = false>
__device__ __forceinline__ SceneLds scene_lds(unsigned char* smem, uint32_t n_lists) {
    static_assert(kSceneLdsWords == 5u && kSceneLdsGradWords == 7u, "id, c, tf, tl, w; q, T");
    static_assert(scene_lds_word(3, 6) == scene_lds_word(3, 0) + 6u * 3u * sizeof(uint32_t), "the word arrays lie n_lists words apart");
    uint32_t* p = reinterpret_cast<uint32_t*>(smem + scene_lds_word(n_lists, 0));       // word array i at scene_lds_word(n_lists, i): n_lists words apart
    const auto u = [&] { uint32_t* q = p; p += n_lists; return q; };
    const auto f = [&] { return reinterpret_cast<float*>(u()); };
    return { reinterpret_cast<uint16_t*>(smem), u(), u(), f(), f(), f(), GRAD ? f() : nullptr, GRAD ? f() : nullptr };
}
// An entry of perm: the compact list and the slot in it (16 bits hold kSceneMaxLists * kSceneListLen of them)
static_assert(kSceneMaxLists * kSceneListLen <= 0x10000u && kSceneListLen == 64u, "perm is uint16_t; a block and a list are one wavefront long");
__device__ __forceinline__ uint16_t scene_perm_pack(uint32_t a, uint32_t slot) { return (uint16_t)(a * kSceneListLen | slot); }
__device__ __forceinline__ uint32_t scene_perm_list(uint32_t e) { return e / kSceneListLen; }
__device__ __forceinline__ uint32_t scene_perm_slot(uint32_t e) { return e % kSceneListLen; }

// One wavefront (= one workgroup) per ray.  The ray's non-empty lists are compacted into LDS in list order (s.id: compact -> list, s.c its count, s.tf / s.tl
// its first / last t, s.w zeroed), then every sample's place in the merged order is counted: its index in its own list + the samples of each other list that
// come before it (ties to the lower list index) -- the whole list or none where the t ranges do not overlap, a binary search of that list where they do.
// s.perm[rank] = scene_perm_pack(compact list, index).  na = the non-empty lists, n_tot = their samples.  Ends with a barrier.
__device__ __forceinline__ void scene_merge_lists(const SceneLds& s, uint32_t ray, uint32_t n_lists, uint32_t cap, const float* __restrict__ tl,
        const uint32_t* __restrict__ cnt, int lane, uint32_t& na_out, uint32_t& n_tot_out) {
    constexpr uint32_t L2S = kSceneListLen;
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
            s.id[pos] = k; s.c[pos] = c; s.tf[pos] = q[0]; s.tl[pos] = q[c - 1u]; s.w[pos] = 0.f;
        }
        na += (uint32_t)__popcll(b);
        n_tot += (uint32_t)__builtin_amdgcn_readlane((int)scan_add64_u32(c), 63);
    }
    __syncthreads();
    // ---- merged order: rank of every sample
    for (uint32_t a = 0; a < na; ++a) {
        const uint32_t c = s.c[a];
        if ((uint32_t)lane < c) {
            const float tv = tl[((size_t)s.id[a] * cap + ray) * L2S + lane];
            uint32_t r = (uint32_t)lane;
            for (uint32_t b = 0; b < na; ++b) {
                if (b == a) continue;
                const bool first = b < a;                                          // (list b's samples at an equal t come first)
                const uint32_t cb = s.c[b];
                const float lb = s.tl[b], fb = s.tf[b];
                if (first ? lb <= tv : lb < tv) r += cb;                           // all of list b is in front
                else if (first ? fb <= tv : fb < tv) {                             // part of it: count (binary search; the last one is not in front)
                    const float* q = tl + ((size_t)s.id[b] * cap + ray) * L2S;
                    uint32_t pos = 0u;
                    for (uint32_t step = L2S / 2u; step; step >>= 1)
                        if (pos + step <= cb) { const float v = q[pos + step - 1u]; if (first ? v <= tv : v < tv) pos += step; }
                    r += pos;
                }
            }
            s.perm[r] = scene_perm_pack(a, (uint32_t)lane);                             // (r <= n_tot - 1 whatever the lists hold)
        }
    }
    __syncthreads();
    na_out = na; n_tot_out = n_tot;
}

// ---- the steps of one block of 64 merged samples, one per lane.  Every loop over a ray's blocks is made of these: scene_composite_walk, the forward of
// scene_composite_ray and the reverse sweep of scene_composite_grad_walk (kernels_scene_pose.hip).
// Position p of the merged order -> the sample: its compact list a (~0u: p holds no sample, and alpha 0), its slot there, its flat index idx into the
// lists, and with LOAD its t, alpha and colour (scene_load: the same for a sample fetched without them).
struct SceneSample { uint32_t a, slot; size_t idx; float t, al, c0, c1, c2; };
__device__ __forceinline__ void scene_load(SceneSample& m, const float* __restrict__ tl, const float4* __restrict__ attr) {
    if (m.a != ~0u) { const float4 v = attr[m.idx]; m.t = tl[m.idx]; m.al = v.x; m.c0 = v.y; m.c1 = v.z; m.c2 = v.w; }
}
template <bool LOAD = true>
__device__ __forceinline__ SceneSample scene_fetch(const SceneLds& s, uint32_t p, uint32_t ray, uint32_t cap, uint32_t na, uint32_t n_tot,
        const float* __restrict__ tl, const float4* __restrict__ attr) {
    SceneSample m = { ~0u, 0u, 0, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (p < n_tot) {
        const uint32_t e = s.perm[p];
        if (scene_perm_list(e) < na) {
            m.a = scene_perm_list(e); m.slot = scene_perm_slot(e);
            m.idx = ((size_t)s.id[m.a] * cap + ray) * kSceneListLen + m.slot;
            if constexpr (LOAD) scene_load(m, tl, attr);
        }
    }
    return m;
}
// The block's transmittances from omv = 1 - alpha and the transmittance Tc the block is entered with: incl behind each lane's sample, T in front of it, and
// whether the sample still counts (active; nact = how many of the block's do).  Each half-wave scans its 32 samples as k_fused_render scans a tile; the
// second carries the first's last product.
struct SceneTrans { float incl, T; bool active; int nact; };
__device__ __forceinline__ SceneTrans scene_transmittance(float omv, float Tc, uint32_t n_tot, int lane) {
    const float sc = scene_scan_mul32(omv, n_tot), lo = sc * Tc, mid = lane_bcast(lo, 31);
    const float incl = lane < 32 ? lo : sc * mid;
    float T = lane_prev(incl, Tc); if (lane == 0) T = Tc; if (lane == 32) T = mid;
    const bool active = T >= kTransmittanceEps;
    return { incl, T, active, (int)__popcll(__ballot(active)) };
}
// Each a += the block's sum of its v, half by half: the first half-wave's sum, then the second's.  Four at once, so that the four scans run abreast.
__device__ __forceinline__ void scene_block_add(float& a0, float& a1, float& a2, float& a3, float v0, float v1, float v2, float v3) {
    const float x0 = scan_add32(v0), x1 = scan_add32(v1), x2 = scan_add32(v2), x3 = scan_add32(v3);
    a0 += lane_bcast(x0, 31); a1 += lane_bcast(x1, 31); a2 += lane_bcast(x2, 31); a3 += lane_bcast(x3, 31);
    a0 += lane_bcast(x0, 63); a1 += lane_bcast(x1, 63); a2 += lane_bcast(x2, 63); a3 += lane_bcast(x3, 63);
}
// Per-list weight sums into s.w: one reduction per list present in the block, in the order of the lowest pending lane
__device__ __forceinline__ void scene_list_weights(const SceneLds& s, uint32_t a, float wgt, int lane) {
    unsigned long long pend = __ballot(a != ~0u && wgt != 0.f);
    while (pend) {
        const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)a, (int)__builtin_ctzll(pend));
        const bool mine = a == a0;
        const float xs = scan_add32(mine ? wgt : 0.f);
        const float sum = lane_bcast(xs, 31) + lane_bcast(xs, 63);
        if (lane == 0) s.w[a0] += sum;
        pend &= ~__ballot(mine);
    }
}
// The transmittance behind the block's last active sample, which the next block is entered with; false: transmittance ran out inside this block (the
// cut), and no block follows
__device__ __forceinline__ bool scene_carry(const SceneTrans& x, float& Tc) {
    Tc = x.nact > 0 ? lane_bcast(x.incl, x.nact > 0 ? x.nact - 1 : 0) : Tc;
    return x.nact >= 64;
}

// The front-to-back composite of one ray's merged sequence (k_scene_composite, k_scene_probe_composite), after scene_merge_lists: blocks of 64 with a
// carried transmittance.  The sums are added half by half (scene_block_add), so one object's list composites to exactly k_fused_render's arithmetic.
// Per-list weight sums go to s.w.
// HIT (the probe): also the first merged sample after which 1 - T > 0.5 -- one ballot per block, the wave stays uniform: its t and compact list.
// CAST (the ray cast, k_scene_cast_composite; with HIT): the threshold is the argument thr in place of 0.5, and the crossing lane also yields, through
// readlanes, the transmittance in front of its sample as the walk carries it (hit_T), the sample's alpha and its slot in its own list.
// Every lane returns the same values.
struct SceneWalk { float Tc, r0, r1, r2, dep, hit_t; uint32_t hit_a; bool hit; float hit_T, hit_alpha; uint32_t hit_slot; };
template <bool HIT, bool CAST = false>
__device__ __forceinline__ void scene_composite_walk(const SceneLds& s, uint32_t ray, uint32_t cap, uint32_t na, uint32_t n_tot,
        const float* __restrict__ tl, const float4* __restrict__ attr, int lane, SceneWalk& w, float thr = 0.5f) {
    static_assert(HIT || !CAST, "CAST extends HIT");
    float Tc = 1.f, r0 = 0.f, r1 = 0.f, r2 = 0.f, dep = 0.f;
    w.hit = false; w.hit_t = 0.f; w.hit_a = 0u;
    if constexpr (CAST) { w.hit_T = 1.f; w.hit_alpha = 0.f; w.hit_slot = 0u; }
    for (uint32_t base = 0; base < n_tot; base += 64u) {
        const SceneSample m = scene_fetch(s, base + (uint32_t)lane, ray, cap, na, n_tot, tl, attr);
        const SceneTrans x = scene_transmittance(1.f - m.al, Tc, n_tot, lane);
        const float wgt = x.active ? m.al * x.T : 0.f;
        scene_block_add(r0, r1, r2, dep, wgt * m.c0, wgt * m.c1, wgt * m.c2, wgt * m.t);
        if constexpr (HIT) {
            // (a slot that holds no sample has alpha 0 and cannot be the first to cross)
            const unsigned long long cross = __ballot(m.a != ~0u && 1.f - x.incl > (CAST ? thr : 0.5f));
            if (!w.hit && cross) {
                const int l = (int)__builtin_ctzll(cross);
                w.hit = true; w.hit_t = lane_bcast(m.t, l); w.hit_a = (uint32_t)__builtin_amdgcn_readlane((int)m.a, l);
                if constexpr (CAST) {
                    w.hit_T = lane_bcast(x.T, l); w.hit_alpha = lane_bcast(m.al, l); w.hit_slot = (uint32_t)__builtin_amdgcn_readlane((int)m.slot, l);
                }
            }
        }
        scene_list_weights(s, m.a, wgt, lane);
        if (!scene_carry(x, Tc)) break;
    }
    w.Tc = Tc; w.r0 = r0; w.r1 = r1; w.r2 = r2; w.dep = dep;
}
// ... and what one lane writes of it: mon_scene_render's four outputs of the ray (DN false, the ray cast: the distance sum w t itself, dn is not read)
template <bool DN = true>
__device__ __forceinline__ void scene_composite_store(const SceneLds& s, uint32_t ray, uint32_t na, const SceneWalk& w, const float* __restrict__ dn,
        float* __restrict__ out_rgb, float* __restrict__ out_depth, float* __restrict__ out_opacity, int32_t* __restrict__ out_instance) {
    const float Tc = w.Tc, op = 1.f - Tc;
    out_rgb[3 * (size_t)ray] = w.r0 + Tc; out_rgb[3 * (size_t)ray + 1] = w.r1 + Tc; out_rgb[3 * (size_t)ray + 2] = w.r2 + Tc;
    if constexpr (DN) out_depth[ray] = op > 0.5f ? w.dep / dn[ray] : 0.f;
    else out_depth[ray] = op > 0.5f ? w.dep : 0.f;
    out_opacity[ray] = op;
    int32_t inst = -1;
    if (op > 0.5f) { float best = -1.f; for (uint32_t a = 0; a < na; ++a) if (s.w[a] > best) { best = s.w[a]; inst = (int32_t)s.id[a]; } }
    out_instance[ray] = inst;
}

// One drawn ray of camera refinement (k_scene_pose_rays, k_scene_score_rays): global ray i of the evaluation, written to slot r of the chunk, under the
// camera pose Twc16 (device memory).  The pixel as k_pose_rays draws it (keyed by seed, iteration and i -- not by the pose), its targets, and for every
// object j the ray mon_object_render builds for that pixel under Twc and the object's Tow, intersected with the object's box.
// Per ray (3 x float4): {c*, d*} {|camera ray|, M*, 0, 0} {unit camera ray, 0}.  Per object and ray (3 x float4 at (j * cap + r) * 3): {o, t0} {d, t1}
// {hit, jitter index base (bits), 0, 0}; m*_j at j * cap + r.
__device__ __forceinline__ void scene_pose_ray(const ScenePoseRayArgs& a, uint32_t r, uint32_t i, const float* __restrict__ Twc16) {
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
    const uint32_t rgba = a.ds.rgba[pix], inst = rgba >> 24;
    const float dstar = a.ds.depth ? a.ds.depth[pix] : 0.f;
    const uint32_t base = a.drawn ? i * 64u : q * 64u;                                  // (2S = 64: the fused shapes)
    float Twc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Twc[k] = Twc16[k];
    float dn = 1.f, Mstar = 0.f;
    for (uint32_t j = 0; j < a.n_objs; ++j) {
        const SceneObjConst& oc = a.objs[j];
        float o[3], d[3], t0 = 0.f, t1 = 0.f;
        pixel_ray(a.ds.K, (float)x, (float)y, Twc, oc.Tow, false, o, d, dn);
        const bool hit = ray_intersect(oc.aabb, o, d, t0, t1);
        const float m = inst == oc.instance_id ? 1.f : 0.f;
        Mstar = fmaxf(Mstar, m);
        float4* rr = a.rec + 3 * ((size_t)j * a.cap + r);
        rr[0] = make_float4(o[0], o[1], o[2], fmaxf(t0, 0.0f));
        rr[1] = make_float4(d[0], d[1], d[2], t1);
        rr[2] = make_float4(hit ? 1.f : 0.f, __builtin_bit_cast(float, base), 0.f, 0.f);
        a.mstar[(size_t)j * a.cap + r] = m;
    }
    // the unit camera ray, as pixel_ray forms it
    const float dc[3] = { ((float)x - a.ds.K.cx) / a.ds.K.fx, ((float)y - a.ds.K.cy) / a.ds.K.fy, 1.0f };
    const float n = sqrtf(fmaf(dc[2], dc[2], fmaf(dc[1], dc[1], dc[0] * dc[0])));
    float4* ray = a.ray + 3 * (size_t)r;
    ray[0] = make_float4((float)(rgba & 0xffu) / 255.0f, (float)((rgba >> 8) & 0xffu) / 255.0f, (float)((rgba >> 16) & 0xffu) / 255.0f, dstar);
    ray[1] = make_float4(n, Mstar, 0.f, 0.f);
    ray[2] = make_float4(dc[0] / n, dc[1] / n, dc[2] / n, 0.f);
}

// The composite forward of one ray of camera refinement, one wavefront (= one workgroup) per ray: k_scene_composite's compaction and merged order
// (scene_merge_lists), the composite in blocks of 64 with a carried transmittance (the walk's steps, summing w (c - c*) in place of w c), the per-list
// weight sums W_j (s.w) and the ray's loss
//   l = w_rgb M* |r|^2 / 3 + w_mask sum_j (W_j - m*_j)^2 + w_depth M* [d* > 0] Huber(D - d*).
// GRAD (k_scene_composite_grad): also keeps what the reverse sweep needs -- each block's entry transmittance in s.T, 2 w_mask (W_j - m*_j) in s.q -- and
// writes the debug output out_W.  Without it (k_scene_composite_loss) s.q and s.T are not touched and nothing is stored to global memory.
// Every lane returns the same values.  The LDS arrays are read again by the caller only after its own barrier.
struct SceneRayFwd {
    uint32_t na, n_tot, n_blocks, n_done;                                               // n_done: blocks composited (the cut lies in the last of them, or nowhere)
    float cs[3], dstar, dn, Mstar, res[3], D, l; bool dep_on;
};
template <bool GRAD>
__device__ __forceinline__ void scene_composite_ray(const SceneCompGradArgs& a, const SceneLds& s, uint32_t ray, int lane, SceneRayFwd& f) {
    const uint32_t n_lists = a.n_lists, cap = a.cap;
    uint32_t na, n_tot;
    scene_merge_lists(s, ray, n_lists, cap, a.t, a.cnt, lane, na, n_tot);
    const float4 tg = a.ray[3 * (size_t)ray], tg1 = a.ray[3 * (size_t)ray + 1];
    const float cs[3] = { tg.x, tg.y, tg.z }, dstar = tg.w, dn = tg1.x, Mstar = tg1.y;
    // ---- forward
    float Tc = 1.f, r0 = 0.f, r1 = 0.f, r2 = 0.f, dep = 0.f;
    const uint32_t n_blocks = (n_tot + 63u) / 64u;
    uint32_t n_done = 0u;
    for (uint32_t blk = 0; blk < n_blocks; ++blk) {
        const SceneSample m = scene_fetch(s, blk * 64u + (uint32_t)lane, ray, cap, na, n_tot, a.t, a.attr);
        if constexpr (GRAD) { if (lane == 0) s.T[blk] = Tc; }
        const SceneTrans x = scene_transmittance(1.f - m.al, Tc, n_tot, lane);
        const float wgt = x.active ? m.al * x.T : 0.f;
        scene_block_add(r0, r1, r2, dep, wgt * (m.c0 - cs[0]), wgt * (m.c1 - cs[1]), wgt * (m.c2 - cs[2]), wgt * m.t);
        scene_list_weights(s, m.a, wgt, lane);
        n_done = blk + 1u;
        if (!scene_carry(x, Tc)) break;
    }
    __syncthreads();
    // ---- the ray's loss
    const float D = dep / dn;
    const bool dep_on = a.w_depth != 0.f && Mstar != 0.f && dstar > 0.f;
    float lmask = 0.f;                                                              // sum_j (W_j - m*_j)^2 over every list, in list order by wave
    for (uint32_t g = 0; g < n_lists; g += 64u) {
        const uint32_t k = g + (uint32_t)lane;
        float term = 0.f;
        if (k < n_lists) {
            // compact index of list k, if it has one: binary search over s.id[0, na)
            uint32_t lo2 = 0u, hi2 = na;
            while (lo2 < hi2) { const uint32_t mid2 = (lo2 + hi2) >> 1; if (s.id[mid2] < k) lo2 = mid2 + 1u; else hi2 = mid2; }
            const bool present = lo2 < na && s.id[lo2] == k;
            const float Wk = present ? s.w[lo2] : 0.f, m = a.mstar[(size_t)k * cap + ray];
            const float dW = Wk - m;
            term = dW * dW;
            if constexpr (GRAD) {
                if (present) s.q[lo2] = 2.f * a.w_mask * dW;
                if (a.out_W) a.out_W[(size_t)k * cap + ray] = Wk;
            }
        }
        lmask += wave_sum(term);
    }
    f.l = a.w_rgb * Mstar * (r0 * r0 + r1 * r1 + r2 * r2) / 3.f + a.w_mask * lmask
            + (dep_on ? a.w_depth * huber_f(D - dstar, a.huber) : 0.f);
    f.na = na; f.n_tot = n_tot; f.n_blocks = n_blocks; f.n_done = n_done;
    f.cs[0] = cs[0]; f.cs[1] = cs[1]; f.cs[2] = cs[2]; f.dstar = dstar; f.dn = dn; f.Mstar = Mstar;
    f.res[0] = r0; f.res[1] = r1; f.res[2] = r2; f.D = D; f.dep_on = dep_on;
}

// ---- the tail of an evaluation, shared by k_scene_pose_update and k_scene_window_update (one thread)
// part = the 32 strided group sums of one object's partial rows: the groups in order, x 1/N -> v = G_j = (sum g_o, sum x_o x g_o) in the object frame; with
// Toc_j = Tow_j Twc = (R, p): grad_rho += R^T G_rho, grad_phi += R^T (G_phi - p x G_rho).
__device__ __forceinline__ void scene_rows_to_camera(const float (*part)[8], float inv_n, const float* Tow, const float* Twc, float (&grad)[6], float (&v)[6]) {
    for (int k = 0; k < 6; ++k) { float q = 0.f; for (int g = 0; g < 32; ++g) q += part[g][k]; v[k] = q * inv_n; }
    float R[9], p[3];                                                                   // Toc = Tow Twc, column-major 3x3
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) {
        float q = 0.f; for (int k = 0; k < 3; ++k) q += Tow[k * 4 + r] * Twc[c * 4 + k]; R[c * 3 + r] = q; }
    for (int r = 0; r < 3; ++r) p[r] = Tow[r] * Twc[12] + Tow[4 + r] * Twc[13] + Tow[8 + r] * Twc[14] + Tow[12 + r];
    const float m[3] = { v[3] - (p[1] * v[2] - p[2] * v[1]), v[4] - (p[2] * v[0] - p[0] * v[2]), v[5] - (p[0] * v[1] - p[1] * v[0]) };
    for (int c = 0; c < 3; ++c) {                                                       // R^T: row c of R^T is column c of R
        grad[c] += R[c * 3] * v[0] + R[c * 3 + 1] * v[1] + R[c * 3 + 2] * v[2];
        grad[3 + c] += R[c * 3] * m[0] + R[c * 3 + 1] * m[1] + R[c * 3 + 2] * m[2];
    }
}
// Adam (0.9, 0.999, 1e-8; bias correction by the step number it + 1) on a twist: moments[12] = m, v; delta = the step
__device__ __forceinline__ void twist_adam(const float* grad, float* moments, float lr_t, float lr_r, uint32_t it, float (&delta)[6]) {
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const float tt = (float)(it + 1u);
    const float c1 = 1.f - powf(b1, tt), c2 = 1.f - powf(b2, tt);
    for (int j = 0; j < 6; ++j) {
        const float g = grad[j];
        const float m = b1 * moments[j] + (1.f - b1) * g, w = b2 * moments[6 + j] + (1.f - b2) * g * g;
        moments[j] = m; moments[6 + j] = w;
        const float lr = j < 3 ? lr_t : lr_r;
        delta[j] = -lr * (m / c1) / (sqrtf(w / c2) + eps);
    }
}
// (Rn, tn) -> pose (column-major 4x4), the rotation re-orthonormalised by Gram-Schmidt: column 0 normalised, column 1 made orthogonal to it and normalised,
// column 2 = c0 x c1
__device__ __forceinline__ void pose_store_orthonormal(float (&Rn)[9], const float (&tn)[3], float* pose) {
    float* a0 = Rn; float* a1 = Rn + 3; float* a2 = Rn + 6;
    float nn = rsqrtf(a0[0] * a0[0] + a0[1] * a0[1] + a0[2] * a0[2]); for (int r = 0; r < 3; ++r) a0[r] *= nn;
    const float dp = a0[0] * a1[0] + a0[1] * a1[1] + a0[2] * a1[2]; for (int r = 0; r < 3; ++r) a1[r] -= dp * a0[r];
    nn = rsqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]); for (int r = 0; r < 3; ++r) a1[r] *= nn;
    a2[0] = a0[1] * a1[2] - a0[2] * a1[1]; a2[1] = a0[2] * a1[0] - a0[0] * a1[2]; a2[2] = a0[0] * a1[1] - a0[1] * a1[0];
    for (int c = 0; c < 3; ++c) { for (int r = 0; r < 3; ++r) pose[c * 4 + r] = Rn[c * 3 + r]; pose[c * 4 + 3] = 0.f; }
    for (int r = 0; r < 3; ++r) pose[12 + r] = tn[r];
    pose[15] = 1.f;
}
// k_scene_pose_update's step: Adam on the camera twist and Twc <- Twc exp(delta^)
__device__ __forceinline__ void scene_camera_adam_step(const float* grad, float* moments, float lr_t, float lr_r, uint32_t it, float* pose) {
    float delta[6];
    twist_adam(grad, moments, lr_t, lr_r, it, delta);
    float Rd[9], td[3];
    se3_exp(delta, Rd, td);
    float Rn[9], tn[3];                                                                 // Twc exp(delta^): R <- R Rd, t <- R td + t
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) {
        float q = 0.f; for (int k = 0; k < 3; ++k) q += pose[k * 4 + r] * Rd[c * 3 + k]; Rn[c * 3 + r] = q; }
    for (int r = 0; r < 3; ++r) tn[r] = pose[r] * td[0] + pose[4 + r] * td[1] + pose[8 + r] * td[2] + pose[12 + r];
    pose_store_orthonormal(Rn, tn, pose);
}
// k_pose_update's step: Adam on the object twist and Tow <- exp(delta^) Tow
__device__ __forceinline__ void scene_object_adam_step(const float* grad, float* moments, float lr_t, float lr_r, uint32_t it, float* pose) {
    float delta[6];
    twist_adam(grad, moments, lr_t, lr_r, it, delta);
    float Rd[9], td[3];
    se3_exp(delta, Rd, td);
    float Rn[9], tn[3];
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) {
        float q = 0.f; for (int k = 0; k < 3; ++k) q += Rd[k * 3 + r] * pose[c * 4 + k]; Rn[c * 3 + r] = q; }
    for (int r = 0; r < 3; ++r) tn[r] = Rd[r] * pose[12] + Rd[3 + r] * pose[13] + Rd[6 + r] * pose[14] + td[r];
    pose_store_orthonormal(Rn, tn, pose);
}

}  // namespace mon
