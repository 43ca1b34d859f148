// kernels_scene_points.hip -- the object map asked at places (mon_scene_query_points, mon_scene_query_lattice, mon_object_query_points): density, colour
// and owner per world point, no ray and no sample list.  k_scene_points writes one object's row of every point of a pass (the point in the object's unit
// cube, whether it lies in the box, the network's raw outputs there and their activations); k_scene_points_fold folds the K rows of a point into the five
// outputs.  The network is the render's: build_fragments, load_level_regs_uniform and tile_forward of fused_device.h, unchanged.
#include "fused_device.h"

namespace mon {

// A point of the pass in object coordinates.  Item i is point i of `pts` ([n][3]), or, without a list, lattice point first + i:
// p(ix, iy, iz) = fmaf(i_a, step_a, origin_a), ix fastest (mon_lattice_points forms the same floats on the host).  WORLD: the point goes into the object's
// frame as k_scene_cast_rays takes a ray origin there (rot3(Tow, x) + tow) and into the unit cube by k_fused_render's operation on a sample point,
// (q - mn) / (mx - mn).  Otherwise (mon_object_query_points) it is the unit-cube point as given.  Returns whether 0 <= u <= 1 on all three axes.
template <bool WORLD>
__device__ __forceinline__ bool scene_point_unit(const ScenePointsArgs& p, const ObjectConst& oc, uint32_t i, float (&u)[3]) {
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

// One object's rows of the n points of a pass: rows[i][12] = u[3], inside (0 / 1), raw4, sigma, r, g, b.  The shape of k_occ_density: a workgroup of four
// waves builds the fragments once, then strides over blocks of 256 points.  Per block every thread takes one point into the object (scene_point_unit) and
// writes u and the flag -- and the eight zeros of a point outside the box; the inside points are compacted by ballot and prefix count, each wave into its own
// quarter of an LDS index list (so one barrier is enough: the quarters' counts give a compacted point's place); then wave w takes tiles w, w + 4, ... of 32
// compacted points through tile_forward, and half-wave 0 writes raw4 and sigma = __expf(raw3), c = logistic_f(raw0..2) (k_fused_render's two lines) to
// the points' rows.  A tile lane forms its point's u again from the point (the same operations, the same bits) instead of reading it back.  Lanes past the
// last compacted point evaluate the cube's centre and store nothing; a block without an inside point evaluates no tile.  A second barrier before the list
// is written again.  No atomics, no scratch; LDS = fragments + level table + the list (512 B of indices, 16 B of counts).
template <int EPAD, int W, int NH, bool WORLD>
__global__ void __launch_bounds__(256) k_scene_points(FusedArgs a, ScenePointsArgs p) {
    using S = FusedShape<EPAD, W, NH>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    half_t* frags = reinterpret_cast<half_t*>(smem);
    LevelLds* llt = reinterpret_cast<LevelLds*>(smem + S::FRAG_BYTES);
    uint16_t* s_list = reinterpret_cast<uint16_t*>(smem + S::FRAG_BYTES + 512);         // [4][64] a wave's inside points: index in the block
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(smem + S::FRAG_BYTES + 512 + 512);    // [4] their number
    build_fragments<EPAD, W, NH>(frags, llt, a, false);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n = lane & 31;
    const half2_t* table = reinterpret_cast<const half2_t*>(a.params + a.nd.n_mlp);
    const LevelRegs lregs = load_level_regs_uniform(a.lt, a.nd.L, lane); const uint32_t table_bytes = a.lt.offset[a.nd.L] * 4u;
    const uint32_t n_blocks = (p.n + 255u) / 256u;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t base = blk * 256u, i = base + threadIdx.x;
        bool inside = false;
        if (i < p.n) {
            float u[3];
            inside = scene_point_unit<WORLD>(p, a.oc, i, u);
            float4* row = reinterpret_cast<float4*>(p.rows + 12 * (size_t)i);
            row[0] = make_float4(u[0], u[1], u[2], inside ? 1.f : 0.f);
            if (!inside) { row[1] = make_float4(0.f, 0.f, 0.f, 0.f); row[2] = make_float4(0.f, 0.f, 0.f, 0.f); }
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
                scene_point_unit<WORLD>(p, a.oc, pt, x);
            }
            TileState<EPAD, W, NH> ts;
            tile_forward<EPAD, W, NH>(ts, frags, lregs, table, table_bytes, a.nd.L, x, lane);
            if (live && lane < 32) {
                const float sigma = __expf(ts.out4[3]);
                const float k0 = logistic_f(ts.out4[0]), k1 = logistic_f(ts.out4[1]), k2 = logistic_f(ts.out4[2]);
                float4* row = reinterpret_cast<float4*>(p.rows + 12 * (size_t)pt);
                row[1] = make_float4(ts.out4[0], ts.out4[1], ts.out4[2], ts.out4[3]);
                row[2] = make_float4(sigma, k0, k1, k2);
            }
        }
        __syncthreads();
    }
}

// One thread per point: the K rows of the point ([K][cap][12], object order) -> sigma = the fp32 sum, in list order, of sigma_j over the objects whose box
// holds the point; owner = the first of them with the largest sigma_j (-1: none), rgb its colour (0 0 0), owner_sigma its sigma_j (0); n_inside = their number.
__global__ void __launch_bounds__(256) k_scene_points_fold(uint32_t n, uint32_t n_objs, uint32_t cap, const float* __restrict__ rows, float* __restrict__ sigma,
        float* __restrict__ rgb, int32_t* __restrict__ owner, float* __restrict__ owner_sigma, uint32_t* __restrict__ n_inside) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sum = 0.f, best = 0.f, r = 0.f, g = 0.f, bl = 0.f; int32_t own = -1; uint32_t cnt = 0u;
    for (uint32_t j = 0; j < n_objs; ++j) {
        const float4* row = reinterpret_cast<const float4*>(rows + 12 * ((size_t)j * cap + i));
        if (row[0].w == 0.f) continue;
        const float4 v = row[2];
        sum += v.x; ++cnt;
        if (own < 0 || v.x > best) { best = v.x; own = (int32_t)j; r = v.y; g = v.z; bl = v.w; }
    }
    sigma[i] = sum; rgb[3 * (size_t)i] = r; rgb[3 * (size_t)i + 1] = g; rgb[3 * (size_t)i + 2] = bl;
    owner[i] = own; owner_sigma[i] = best; n_inside[i] = cnt;
}

template <int EPAD, int W, int NH>
static void scene_points_t(hipStream_t s, const FusedArgs& a, const ScenePointsArgs& p, bool world) {
    using S = FusedShape<EPAD, W, NH>;
    const uint32_t smem = S::FRAG_BYTES + 512 + 1024, grid = (p.n + 255u) / 256u;       // (a pass holds at most 64 blocks of 256 points)
    if (a.keep_zero & 1u) hipLaunchKernelGGL((k_build_frag_image<EPAD, W, NH>), dim3((S::F_WOT * 512 + 255) / 256), dim3(256), 0, s, a.params, a.nd.L,
            const_cast<uint16_t*>(a.frag_image), (const DevState*)nullptr);
    if (world) hipLaunchKernelGGL((k_scene_points<EPAD, W, NH, true>), dim3(grid), dim3(256), smem, s, a, p);
    else hipLaunchKernelGGL((k_scene_points<EPAD, W, NH, false>), dim3(grid), dim3(256), smem, s, a, p);
}

void launch_scene_points(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const ObjectConst& oc, uint16_t* frag_image,
        int build_image, bool world, const ScenePointsArgs& p) {
    if (!p.n) return;
    // (`keep_zero` doubles as "build the fragment image first", as on the render path)
    FusedArgs a{}; a.lt = lt; a.nd = nd; a.oc = oc; a.params = params; a.frag_image = frag_image; a.keep_zero = build_image ? 1u : 0u;
    MON_FUSED_DISPATCH(scene_points_t, s, a, p, world);
}
void launch_scene_points_fold(hipStream_t s, uint32_t n, uint32_t n_objs, uint32_t cap, const float* rows, float* sigma, float* rgb, int32_t* owner,
        float* owner_sigma, uint32_t* n_inside) {
    if (!n || !n_objs) return;
    hipLaunchKernelGGL(k_scene_points_fold, dim3((n + 255u) / 256u), dim3(256), 0, s, n, n_objs, cap, rows, sigma, rgb, owner, owner_sigma, n_inside);
}

}  // namespace mon
