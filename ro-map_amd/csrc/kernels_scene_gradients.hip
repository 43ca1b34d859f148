// kernels_scene_gradients.hip -- the point queries with the field's derivative (mon_scene_query_gradients, mon_scene_query_lattice_gradients,
// mon_object_query_gradients; the normals of mon_scene_cast_normals come through the first): per world point the log density's gradient, the density's
// gradient and the surface normal beside the point query's five outputs.  k_scene_point_grads is k_scene_points (kernels_scene_points.hip) with one more
// step per tile: pose_tile_backward (pose_device.h) seeded with dO = (0, 0, 0, 1), i.e. d raw3 / d x; k_scene_gradients_fold is k_scene_points_fold plus the
// three new outputs and the `select` rule.  The contract is in include/mon_core.h and DESIGN.md 3.4c-5.
#include "pose_device.h"

namespace mon {

// The seed of the backward: dO3 = 1 times 2^5 -- the lower end of the band [32, 64) k_pose_grad scales a ray's largest |dL/dO| into -- undone exactly
constexpr float kGradSeedUp = 32.f, kGradSeedDown = 1.f / 32.f;

// scene_point_unit of kernels_scene_points.hip, restated operation for operation (that file keeps every line; tests/test_scene_gradients.py holds the two
// to equal bits): item i of the pass in object coordinates, and whether it lies in the unit cube
template <bool WORLD>
__device__ __forceinline__ bool grad_point_unit(const ScenePointsArgs& p, const ObjectConst& oc, uint32_t i, float (&u)[3]) {
    float x[3];
    if (p.pts) { x[0] = p.pts[3 * (size_t)i]; x[1] = p.pts[3 * (size_t)i + 1]; x[2] = p.pts[3 * (size_t)i + 2]; }
    else {
        const uint32_t g = p.first + i, ix = g % p.nx, iy = (g / p.nx) % p.ny, iz = g / (p.nx * p.ny);
        x[0] = fmaf((float)ix, p.step[0], p.origin[0]); x[1] = fmaf((float)iy, p.step[1], p.origin[1]); x[2] = fmaf((float)iz, p.step[2], p.origin[2]);
    }
    if constexpr (WORLD) {
        float t[3];
        rot3(oc.Tow.m, x, t);
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float q = t[a] + oc.Tow.m[12 + a]; u[a] = (q - oc.aabb.mn[a]) / (oc.aabb.mx[a] - oc.aabb.mn[a]); }
    } else { u[0] = x[0]; u[1] = x[1]; u[2] = x[2]; }
    return u[0] >= 0.f && u[0] <= 1.f && u[1] >= 0.f && u[1] <= 1.f && u[2] >= 0.f && u[2] <= 1.f;
}

// One object's rows of the n points of a pass: rows[i][16] = u[3], inside (0 / 1), raw4, sigma, r, g, b (k_scene_points' twelve, the same bits), g[3], 0.
// k_scene_points' block structure: blocks of 256 points, the inside points compacted by ballot into per-wave quarters of the LDS list, wave w takes tiles
// w, w + 4, ... of 32 compacted points.  The fragments are the full set (build_fragments(.., true): the transposed matrices follow the forward ones, whose
// place and bits do not change).  Per tile: tile_forward, then pose_tile_backward<LW = true> from the seed; the corners and the ReLU masks are the
// forward's, only the trilinear weights are differentiated; level l's term times level_w[l] (an array of ones for "no weights": wl * (scale * gx) with
// wl = 1 changes no bit, so there is no LW = false copy).  The halves' sums are added (each half-wave owns half of the levels).
//   WORLD: g = R_ow^T g_obj, g_obj = d raw3 / d q per unit of object-frame length (pose_tile_backward divides by the box extent), the world gradient of
//          this object's log density: g_a = fmaf(R(2,a), g_obj2, fmaf(R(1,a), g_obj1, R(0,a) * g_obj0)).
//   else:  g = d raw3 / d u, the extent passed as 1 1 1 (a division by 1 is exact).
// Outside the box g = 0.  No atomics, no scratch; LDS as k_scene_points (fragments + level table + the list).
template <int EPAD, int W, int NH, bool WORLD>
__global__ void __launch_bounds__(256) k_scene_point_grads(FusedArgs a, ScenePointsArgs p, const float* __restrict__ level_w) {
    using S = FusedShape<EPAD, W, NH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t* frags = reinterpret_cast<half_t*>(smem);
    LevelLds* llt = reinterpret_cast<LevelLds*>(smem + S::FRAG_BYTES);
    uint16_t* s_list = reinterpret_cast<uint16_t*>(smem + S::FRAG_BYTES + 512);         // [4][64] a wave's inside points: index in the block
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(smem + S::FRAG_BYTES + 512 + 512);    // [4] their number
    build_fragments<EPAD, W, NH>(frags, llt, a, true);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int L = a.nd.L;
    const half2_t* table = reinterpret_cast<const half2_t*>(a.params + a.nd.n_mlp);
    const LevelRegs lregs = load_level_regs_uniform(a.lt, L, lane); const uint32_t table_bytes = a.lt.offset[L] * 4u;
    const __amdgpu_buffer_rsrc_t rsrc = table_rsrc(table, table_bytes);
    const int LPH = (L + 1) >> 1, lv = lane < 32 ? lane : lane - 32 + LPH;              // the weight of this lane's level (LevelRegs' placement)
    const float lw = (n < LPH && lv < L) ? level_w[lv] : 0.f;
    float ext[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) ext[d] = WORLD ? a.oc.aabb.mx[d] - a.oc.aabb.mn[d] : 1.f;
    const float seed[4] = { 0.f, 0.f, 0.f, 1.f };
    const uint32_t n_blocks = (p.n + 255u) / 256u;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t base = blk * 256u, i = base + threadIdx.x;
        bool inside = false;
        if (i < p.n) {
            float u[3];
            inside = grad_point_unit<WORLD>(p, a.oc, i, u);
            float4* row = reinterpret_cast<float4*>(p.rows + 16 * (size_t)i);
            row[0] = make_float4(u[0], u[1], u[2], inside ? 1.f : 0.f);
            if (!inside) { row[1] = make_float4(0.f, 0.f, 0.f, 0.f); row[2] = make_float4(0.f, 0.f, 0.f, 0.f); row[3] = make_float4(0.f, 0.f, 0.f, 0.f); }
        }
        const unsigned long long b = __ballot(inside);
        if (inside) s_list[wave * 64 + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] = (uint16_t)threadIdx.x;
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        const uint32_t c0 = s_cnt[0], c1 = c0 + s_cnt[1], c2 = c1 + s_cnt[2], total = c2 + s_cnt[3];
        for (uint32_t tile = (uint32_t)wave; tile * 32u < total; tile += S::WAVES) {
            const uint32_t c = tile * 32u + (uint32_t)n;
            const bool live = c < total;
            float x[3] = { 0.5f, 0.5f, 0.5f };
            uint32_t pt = 0u;
            if (live) {
                const uint32_t w = c < c0 ? 0u : c < c1 ? 1u : c < c2 ? 2u : 3u, first = w == 0u ? 0u : w == 1u ? c0 : w == 2u ? c1 : c2;
                pt = base + s_list[w * 64u + (c - first)];
                grad_point_unit<WORLD>(p, a.oc, pt, x);
            }
            TileState<EPAD, W, NH> ts;
            tile_forward<EPAD, W, NH>(ts, frags, lregs, table, table_bytes, L, x, lane);
            float gl[3] = { 0.f, 0.f, 0.f };
            pose_tile_backward<EPAD, W, NH, true>(gl, ts, frags, lregs, rsrc, x, seed, kGradSeedUp, kGradSeedDown, ext, lane, h, L, lw);
            float go[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) go[d] = gl[d] + __shfl_xor(gl[d], 32);
            if (live && lane < 32) {
                const float sigma = __expf(ts.out4[3]);
                const float k0 = logistic_f(ts.out4[0]), k1 = logistic_f(ts.out4[1]), k2 = logistic_f(ts.out4[2]);
                float g[3] = { go[0], go[1], go[2] };
                if constexpr (WORLD) {
                    const float* M = a.oc.Tow.m;
#pragma unroll
                    for (int d = 0; d < 3; ++d) g[d] = fmaf(M[4 * d + 2], go[2], fmaf(M[4 * d + 1], go[1], M[4 * d] * go[0]));
                }
                float4* row = reinterpret_cast<float4*>(p.rows + 16 * (size_t)pt);
                row[1] = make_float4(ts.out4[0], ts.out4[1], ts.out4[2], ts.out4[3]);
                row[2] = make_float4(sigma, k0, k1, k2);
                row[3] = make_float4(g[0], g[1], g[2], 0.f);
            }
        }
        __syncthreads();
    }
}

// One thread per point: the K rows of the point ([K][cap][16], object order) -> k_scene_points_fold's five outputs by its operations (the same bits when
// nothing is selected), and
//   grad_sigma = sum over the objects whose box holds the point, in list order, per component acc = fmaf(sigma_j, g_j, acc)
//   grad_log   = g of the reported object, normal = -grad_log / |grad_log| with |g| = sqrtf(fmaf(g2, g2, fmaf(g1, g1, g0 * g0))) and one division per
//                component; 0 0 0 without a reported object, or where |g| is 0 (underflow of the squares included) or not finite (their overflow included)
// select (may be nullptr; -1 = the owner rule): the object reported in owner, rgb, owner_sigma, grad_log and normal, if the point lies in its box; else none.
__global__ void __launch_bounds__(256) k_scene_gradients_fold(uint32_t n, uint32_t n_objs, uint32_t cap, const float* __restrict__ rows,
        const int32_t* __restrict__ select, float* __restrict__ sigma, float* __restrict__ rgb, int32_t* __restrict__ owner, float* __restrict__ owner_sigma,
        uint32_t* __restrict__ n_inside, float* __restrict__ grad_log, float* __restrict__ grad_sigma, float* __restrict__ normal) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t sel = select ? select[i] : -1;
    float sum = 0.f, best = 0.f, r = 0.f, g = 0.f, bl = 0.f; int32_t own = -1; uint32_t cnt = 0u;
    float gs[3] = { 0.f, 0.f, 0.f }, go[3] = { 0.f, 0.f, 0.f };
    for (uint32_t j = 0; j < n_objs; ++j) {
        const float4* row = reinterpret_cast<const float4*>(rows + 16 * ((size_t)j * cap + i));
        if (row[0].w == 0.f) continue;
        const float4 v = row[2], d = row[3];
        sum += v.x; ++cnt;
        gs[0] = fmaf(v.x, d.x, gs[0]); gs[1] = fmaf(v.x, d.y, gs[1]); gs[2] = fmaf(v.x, d.z, gs[2]);
        if (sel < 0 ? (own < 0 || v.x > best) : (int32_t)j == sel) { best = v.x; own = (int32_t)j; r = v.y; g = v.z; bl = v.w; go[0] = d.x; go[1] = d.y; go[2] = d.z; }
    }
    sigma[i] = sum; rgb[3 * (size_t)i] = r; rgb[3 * (size_t)i + 1] = g; rgb[3 * (size_t)i + 2] = bl;
    owner[i] = own; owner_sigma[i] = best; n_inside[i] = cnt;
    const float len = sqrtf(fmaf(go[2], go[2], fmaf(go[1], go[1], go[0] * go[0])));
    const bool ok = own >= 0 && len > 0.f && len < INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        grad_log[3 * (size_t)i + a] = go[a]; grad_sigma[3 * (size_t)i + a] = gs[a];
        normal[3 * (size_t)i + a] = ok ? -go[a] / len : 0.f;
    }
}

template <int EPAD, int W, int NH>
static void scene_point_grads_t(hipStream_t s, const FusedArgs& a, const ScenePointsArgs& p, bool world, const float* level_w) {
    using S = FusedShape<EPAD, W, NH>;
    const uint32_t smem = S::FRAG_BYTES + 512 + 1024, grid = (p.n + 255u) / 256u;       // (a pass holds at most 64 blocks of 256 points)
    if (a.keep_zero & 1u) hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::N_FRAGS * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    if (world) hipLaunchKernelGGL((k_scene_point_grads<EPAD, W, NH, true>), dim3(grid), dim3(256), smem, s, a, p, level_w);
    else hipLaunchKernelGGL((k_scene_point_grads<EPAD, W, NH, false>), dim3(grid), dim3(256), smem, s, a, p, level_w);
}

void launch_scene_point_grads(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const ObjectConst& oc, uint16_t* frag_image,
        int build_image, bool world, const ScenePointsArgs& p, const float* level_w) {
    if (!p.n) return;
    // (`keep_zero` doubles as "build the fragment image first", as on the render path)
    FusedArgs a{}; a.lt = lt; a.nd = nd; a.oc = oc; a.params = params; a.frag_image = frag_image; a.keep_zero = build_image ? 1u : 0u;
    MON_FUSED_DISPATCH(scene_point_grads_t, s, a, p, world, level_w);
}
void launch_scene_gradients_fold(hipStream_t s, uint32_t n, uint32_t n_objs, uint32_t cap, const float* rows, const int32_t* select, float* sigma, float* rgb,
        int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma, float* normal) {
    if (!n || !n_objs) return;
    hipLaunchKernelGGL(k_scene_gradients_fold, dim3((n + 255u) / 256u), dim3(256), 0, s, n, n_objs, cap, rows, select, sigma, rgb, owner, owner_sigma,
            n_inside, grad_log, grad_sigma, normal);
}

}  // namespace mon
