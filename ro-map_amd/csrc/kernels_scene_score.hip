// kernels_scene_score.hip -- batched camera pose scoring against a scene of object NeRFs (mon_scene_pose_loss_batch): the forward half of the chain of
// kernels_scene_pose.hip over many candidate poses at once.  A pass holds G hypotheses of n rays each as G * n virtual rays v = g * n + r in the list
// workspace of one evaluation: k_scene_score_rays (every hypothesis's records of the same drawn pixels) -> per object k_scene_pose_obj<.., false, false>
// over the virtual rays (kernels_scene_pose.hip) -> k_scene_composite_loss (one loss partial per hypothesis and workgroup) -> k_scene_loss_reduce (one loss
// per hypothesis).  Every sum runs in mon_scene_pose_loss's order, so each loss has that call's bits.  No atomics anywhere.
#include "pose_device.h"
#include "scene_device.h"

namespace mon {

// ------------------------------------------------------------------ k_scene_score_rays
// One thread per virtual ray v = g * n_per + r of the pass: scene_pose_ray for ray r of the evaluation, written to slot v, under the pose of hypothesis
// h0 + g.  The pixel, its targets and the jitter index base depend on r alone, so every hypothesis sees the same pixels and the same jitter.
__global__ void __launch_bounds__(256) k_scene_score_rays(SceneScoreRayArgs a) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_rays) return;
    const uint32_t g = v / a.n_per, r = v - g * a.n_per;
    scene_pose_ray(a, v, r, a.pose + 16u * (size_t)(a.h0 + g));
}

// ------------------------------------------------------------------ k_scene_composite_loss
// The forward half of k_scene_composite_grad (scene_composite_ray, scene_device.h), one wavefront (= one workgroup) per ray.  Grid (parts, G): workgroup
// (b, g) walks rays b, b + parts, ... of hypothesis g in that order -- k_scene_composite_grad's walk of one evaluation on a grid of `parts` -- and writes
// their summed losses to loss_part[g * parts + b].  Nothing else is stored.
__global__ void __launch_bounds__(64) k_scene_composite_loss(SceneCompGradArgs a, uint32_t n_per) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SceneLds s = scene_lds(smem, a.n_lists);
    const int lane = threadIdx.x;
    const uint32_t v0 = blockIdx.y * n_per;
    float loss_acc = 0.f;
    for (uint32_t r = blockIdx.x; r < n_per; r += gridDim.x) {
        SceneRayFwd f;
        scene_composite_ray<false>(a, s, v0 + r, lane, f);
        loss_acc += f.l;
        __syncthreads();
    }
    if (lane == 0) a.loss_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = loss_acc;
}

// ------------------------------------------------------------------ k_scene_loss_reduce
// One workgroup per hypothesis: its loss partials summed 256-strided, then the 256 sums in order by thread 0, x 1/N -- k_scene_pose_update's order.
__global__ void __launch_bounds__(256) k_scene_loss_reduce(const float* __restrict__ loss_part, uint32_t n_parts, float inv_n, float* __restrict__ out) {
    __shared__ float lpart[256];
    const float* part = loss_part + (size_t)blockIdx.x * n_parts;
    float ls = 0.f;
    for (uint32_t b = threadIdx.x; b < n_parts; b += 256u) ls += part[b];
    lpart[threadIdx.x] = ls;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float loss = 0.f;
    for (int g = 0; g < 256; ++g) loss += lpart[g];
    loss *= inv_n;
    out[blockIdx.x] = loss;
}

// ------------------------------------------------------------------ launchers
void launch_scene_score_rays(hipStream_t s, const SceneScoreRayArgs& a) {
    if (!a.n_rays || !a.n_objs || !a.n_per) return;
    hipLaunchKernelGGL(k_scene_score_rays, dim3((a.n_rays + 255) / 256), dim3(256), 0, s, a);
}
// a.n_rays = G * n_per virtual rays; a.loss_part receives G * scene_comp_grad_grid(n_per) partials
void launch_scene_composite_loss(hipStream_t s, const SceneCompGradArgs& a, uint32_t n_per) {
    if (!a.n_rays || !n_per || a.n_rays % n_per || !a.n_lists || a.n_lists > kSceneMaxLists) return;
    const uint32_t parts = n_per < kSceneLossParts ? n_per : kSceneLossParts;
    hipLaunchKernelGGL(k_scene_composite_loss, dim3(parts, a.n_rays / n_per), dim3(64), scene_composite_lds(a.n_lists), s, a, n_per);
}
void launch_scene_loss_reduce(hipStream_t s, const float* loss_part, uint32_t n_hyp, uint32_t n_parts, float inv_n, float* out) {
    if (!n_hyp) return;
    hipLaunchKernelGGL(k_scene_loss_reduce, dim3(n_hyp), dim3(256), 0, s, loss_part, n_parts, inv_n, out);
}

}  // namespace mon
