// kernels_scene_cast.hip -- the ray cast against the object map (mon_scene_cast): world rays x(t) = o + t d in place of a camera's pixels, and a first hit
// placed inside its sample's interval.  k_scene_cast_rays fills one object's ray rows from the ray list; the samples come from k_fused_render<EMIT, KEYED>
// (kernels_render.hip, unchanged); k_scene_cast_composite is k_scene_probe_composite with the threshold as an argument and the interpolated hit.
#include <cmath>
#include "fused_device.h"
#include "scene_device.h"

namespace mon {

// One thread per ray of the pass, for one object: the world ray taken into the object's frame as pixel_ray takes a camera ray there (rot3(Tow, d),
// rot3(Tow, o) + tow; d is used as given, not renormalised), intersected with the box by ray_intersect and clipped to the segment: lo = max(t0, 0),
// hi = min(t1, t_max).  The object contributes iff the box is hit and lo < hi; its row then holds t0 = lo, t1 = hi, dn = 1, and entry[i] = lo (what the
// composite takes for the near end of slot 0's interval); otherwise flag 0, dn 1, entry 0.
// A direction component that is exactly 0 makes both slab distances of that axis infinite: of equal sign (a miss) when the origin lies outside the slab,
// -inf / +inf (the slab binds nothing) when it lies inside.  With the origin exactly in a slab plane of such an axis one distance is 0 / 0 = NaN, which
// every comparison of ray_intersect fails: the outcome depends on the axis and on the sign of the zero (a miss, or the interval of the other two slabs, or
// a NaN in t0 / t1).  A NaN end is taken for a miss here, so nothing that is not finite ever reaches the emit.
// keys (object 0's launch only, else nullptr) = the rays' jitter keys as the keyed emit reads them.
__global__ void __launch_bounds__(256) k_scene_cast_rays(BatchPtrs b, ObjectConst oc, const mon_scene_ray* __restrict__ rays, uint32_t* __restrict__ keys,
        float* __restrict__ entry, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mon_scene_ray r = rays[i];
    float o[3], d[3], t[3], t0 = 0.f, t1 = 0.f;
    rot3(oc.Tow.m, r.d, d);
    rot3(oc.Tow.m, r.o, t);
    o[0] = t[0] + oc.Tow.m[12]; o[1] = t[1] + oc.Tow.m[13]; o[2] = t[2] + oc.Tow.m[14];
    const bool hit = ray_intersect(oc.aabb, o, d, t0, t1);
    const float lo = fmaxf(t0, 0.0f), hi = fminf(t1, r.t_max);
    const bool on = hit && t0 == t0 && t1 == t1 && lo < hi;
    b.ray_flag[i] = on ? 1 : 0;
    b.ray_dn[i] = 1.0f;
    entry[i] = on ? lo : 0.0f;
    if (keys) keys[i] = r.key;
    if (on) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.ray_o[3 * i + a] = o[a]; b.ray_d[3 * i + a] = d[a]; }
        b.ray_t0[i] = lo; b.ray_t1[i] = hi;
    }
}

// One wavefront (= one workgroup) per ray: k_scene_composite's merge, walk and outputs (scene_device.h; the distance sum w t undivided), and from the walk's
// first crossing of 1 - T > thr at merged sample i: hit_sample_t = t_i, its list, and
//   hit_t = p + f (t_i - p),   f = clamp(ln(T_i / (1 - thr)) / (-ln(1 - alpha_i)), 0, 1),   f = 0 when 1 - alpha_i == 0
// the point inside the sample's interval at which the transmittance of a constant density reaches 1 - thr.  p = the previous sample's t of the same list, or
// for slot 0 the list's entry (entry[list * cap + ray]: the box entry, not 0).  T_i = the merged transmittance in front of the sample as the walk carries it.
// One logf pair per ray, by lane 0.  LDS as k_scene_composite's.
__global__ void __launch_bounds__(64) k_scene_cast_composite(uint32_t n_rays, uint32_t n_lists, uint32_t cap, float thr, const float* __restrict__ tl,
        const float4* __restrict__ attr, const uint32_t* __restrict__ cnt, const float* __restrict__ entry, float* __restrict__ out_rgb,
        float* __restrict__ out_dist, float* __restrict__ out_opacity, int32_t* __restrict__ out_instance, float* __restrict__ out_hit_t,
        float* __restrict__ out_hit_sample_t, int32_t* __restrict__ out_hit_instance) {
    constexpr uint32_t L2S = kSceneListLen;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SceneLds s = scene_lds(smem, n_lists);
    const int lane = threadIdx.x;
    for (uint32_t ray = blockIdx.x; ray < n_rays; ray += gridDim.x) {
        uint32_t na, n_tot;
        scene_merge_lists(s, ray, n_lists, cap, tl, cnt, lane, na, n_tot);
        SceneWalk w;
        scene_composite_walk<true, true>(s, ray, cap, na, n_tot, tl, attr, lane, w, thr);
        if (lane == 0) {
            scene_composite_store<false>(s, ray, na, w, nullptr, out_rgb, out_dist, out_opacity, out_instance);
            float ht = 0.f, hs = 0.f; int32_t hi = -1;
            if (w.hit) {
                const size_t row = (size_t)s.id[w.hit_a] * cap + ray;
                const float p = w.hit_slot ? tl[row * L2S + w.hit_slot - 1u] : entry[row];
                const float om = 1.f - w.hit_alpha;
                float f = 0.f;
                if (om != 0.f) f = fminf(fmaxf(logf(w.hit_T / (1.f - thr)) / -logf(om), 0.f), 1.f);
                hs = w.hit_t; ht = fmaf(f, hs - p, p); hi = (int32_t)s.id[w.hit_a];
            }
            out_hit_t[ray] = ht; out_hit_sample_t[ray] = hs; out_hit_instance[ray] = hi;
        }
        __syncthreads();
    }
}

void launch_scene_cast_rays(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, const mon_scene_ray* rays, uint32_t* keys, float* entry, uint32_t n) {
    if (!n) return;
    hipLaunchKernelGGL(k_scene_cast_rays, dim3((n + 255) / 256), dim3(256), 0, s, b, oc, rays, keys, entry, n);
}
void launch_scene_cast_composite(hipStream_t s, uint32_t n_rays, uint32_t n_lists, uint32_t cap, float thr, const float* t, const float* attr,
        const uint32_t* cnt, const float* entry, float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t,
        int32_t* hit_instance) {
    if (!n_rays || !n_lists || n_lists > kSceneMaxLists) return;
    hipLaunchKernelGGL(k_scene_cast_composite, dim3(scene_composite_grid(n_rays)), dim3(64), scene_composite_lds(n_lists), s, n_rays, n_lists, cap, thr, t,
            reinterpret_cast<const float4*>(attr), cnt, entry, rgb, dist, opacity, instance, hit_t, hit_sample_t, hit_instance);
}

}  // namespace mon
