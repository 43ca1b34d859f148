// kernels_scene_probe.hip -- the scene probe (mon_scene_probe): what mon_scene_render returns, at a list of sub-pixel image points under several camera
// poses, plus the depth at which each ray is stopped.  k_scene_probe_rays fills one object's ray rows from the query list; the samples come from
// k_fused_render<EMIT, KEYED> (kernels_render.hip); k_scene_probe_composite is k_scene_composite with the two hit outputs.
#include "fused_device.h"
#include "scene_device.h"

namespace mon {

// One thread per query of the pass, for one object: the body of k_render_rays with (u, v) and the pose taken from the query.  keys (object 0's launch only,
// else nullptr) = the queries' jitter keys as the keyed emit reads them.
__global__ void __launch_bounds__(256) k_scene_probe_rays(BatchPtrs b, Intrinsics K, ObjectConst oc, const mon_scene_query* __restrict__ q,
        const float* __restrict__ poses, uint32_t* __restrict__ keys, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mon_scene_query qi = q[i];
    float Twc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Twc[k] = poses[16 * (size_t)qi.pose + k];
    float o[3], d[3], dn, t0, t1;
    pixel_ray(K, qi.u, qi.v, Twc, oc.Tow.m, false, o, d, dn);
    const bool hit = ray_intersect(oc.aabb, o, d, t0, t1);
    b.ray_flag[i] = hit ? 1 : 0;
    b.ray_dn[i] = dn;
    if (keys) keys[i] = qi.key;
    if (hit) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.ray_o[3 * i + a] = o[a]; b.ray_d[3 * i + a] = d[a]; }
        b.ray_t0[i] = fmaxf(t0, 0.0f); b.ray_t1[i] = t1;
    }
}

// One wavefront (= one workgroup) per query: k_scene_composite's merge, walk and outputs (scene_device.h), and from the walk's first crossing of
// 1 - T > 0.5 the depth of that sample and its list (0 and -1 where the ray is never stopped).  LDS as k_scene_composite's.
__global__ void __launch_bounds__(64) k_scene_probe_composite(uint32_t n_rays, uint32_t n_lists, uint32_t cap, const float* __restrict__ tl,
        const float4* __restrict__ attr, const uint32_t* __restrict__ cnt, const float* __restrict__ dn, float* __restrict__ out_rgb,
        float* __restrict__ out_depth, float* __restrict__ out_opacity, int32_t* __restrict__ out_instance, float* __restrict__ out_hit_depth,
        int32_t* __restrict__ out_hit_instance) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SceneLds s = scene_lds(smem, n_lists);
    const int lane = threadIdx.x;
    for (uint32_t ray = blockIdx.x; ray < n_rays; ray += gridDim.x) {
        uint32_t na, n_tot;
        scene_merge_lists(s, ray, n_lists, cap, tl, cnt, lane, na, n_tot);
        SceneWalk w;
        scene_composite_walk<true>(s, ray, cap, na, n_tot, tl, attr, lane, w);
        if (lane == 0) {
            scene_composite_store(s, ray, na, w, dn, out_rgb, out_depth, out_opacity, out_instance);
            out_hit_depth[ray] = w.hit ? w.hit_t / dn[ray] : 0.f;
            out_hit_instance[ray] = w.hit ? (int32_t)s.id[w.hit_a] : -1;
        }
        __syncthreads();
    }
}

void launch_scene_probe_rays(hipStream_t s, const BatchPtrs& b, const Intrinsics& K, const ObjectConst& oc, const mon_scene_query* q, const float* poses,
        uint32_t* keys, uint32_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_scene_probe_rays, dim3((n + 255) / 256), dim3(256), 0, s, b, K, oc, q, poses, keys, n);
}
void launch_scene_probe_composite(hipStream_t s, uint32_t n_rays, uint32_t n_lists, uint32_t cap, const float* t, const float* attr, const uint32_t* cnt,
        const float* dn, float* rgb, float* depth, float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance) {
    if (!n_rays || !n_lists || n_lists > kSceneMaxLists) return;
    hipLaunchKernelGGL(k_scene_probe_composite, dim3(scene_composite_grid(n_rays)), dim3(64), scene_composite_lds(n_lists), s, n_rays, n_lists, cap, t,
            reinterpret_cast<const float4*>(attr), cnt, dn, rgb, depth, opacity, instance, hit_depth, hit_instance);
}

}  // namespace mon
