// kernels_scene_window.hip -- joint refinement of a window of camera poses and object poses (mon_scene_window_loss / mon_scene_refine_window): the rays of a
// pass of whole frames packed as virtual rays into the list workspace of camera refinement, and the tail of an evaluation -- every frame's loss and camera
// gradient in mon_scene_pose_loss's order, the object gradients, the Adam steps on every free camera and object.  The object forward is
// k_scene_pose_obj<.., false, false> unchanged; the composite and the object backward of a pass are k_scene_window_composite / k_scene_window_obj next to the
// bodies they share with the single-frame chain (kernels_scene_pose.hip).  The objective is stated in include/mon_core.h and DESIGN.md 3.4h.  No atomics.
#include "pose_device.h"
#include "scene_device.h"

namespace mon {

// ------------------------------------------------------------------ k_scene_window_rays
// One thread per virtual ray v of the pass: its frame f is the last row with v0_f <= v; scene_pose_ray for ray v - v0_f of that frame -- its boxes, its own
// prefix, its pose -- written to slot v.  The pixel draw and the jitter base are keyed by the in-frame ray index, as a single-frame call keys them.
__global__ void __launch_bounds__(256) k_scene_window_rays(SceneWindowRayArgs a) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_rays) return;
    uint32_t f = 0u;
    for (uint32_t k = 1u; k < a.n_frames; ++k) if (a.frames[k].v0 <= v) f = k;
    const SceneWinFrame fr = a.frames[f];
    ScenePoseRayArgs b = a;
    b.boxes = a.boxes + fr.box0; b.prefix = a.prefix + fr.prefix0; b.n_obs = fr.n_box; b.total = fr.total;
    scene_pose_ray(b, v, v - fr.v0, a.pose + fr.pose);
}

// ------------------------------------------------------------------ k_scene_window_update
// One workgroup.  The frames in window order; per frame the objects in index order: object j's partial rows of the frame summed in k_scene_pose_update's
// fixed order, x 1/N_f -> G_{f,j}, mapped to the camera frame into grad6_f (scene_rows_to_camera, that kernel's arithmetic) and added into obj_grad6_j; the
// frame's loss partials summed in that kernel's order, x 1/N_f -> L_f; L = sum_f L_f.  All of it at the poses the step starts from.  Then, step != 0: Adam on
// every free camera (Twc <- Twc exp(delta^)) and, refine_objs != 0, on every object (Tow <- exp(delta^) Tow, into SceneObjConst::Tow for the next rays).
__global__ void __launch_bounds__(256) k_scene_window_update(SceneWindowUpdateArgs a) {
    __shared__ float part[32][8];
    __shared__ float lpart[256];
    const uint32_t col = threadIdx.x & 7u, grp = threadIdx.x >> 3;
    float* o = a.out + (size_t)a.out_stride * a.it;
    float* Lf = o + 1; float* cg = Lf + a.n_frames; float* og = cg + 6u * a.n_frames;
    if (threadIdx.x == 0) for (uint32_t k = 0; k < 6u * a.n_objs; ++k) og[k] = 0.f;
    float L = 0.f;
    for (uint32_t f = 0; f < a.n_frames; ++f) {
        const SceneWinFrame fr = a.frames[f];
        float grad[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        for (uint32_t j = 0; j < a.n_objs; ++j) {
            const float* rows = a.partials + ((size_t)j * a.row_stride + fr.row0) * 8;
            float s = 0.f;
            for (uint32_t b = grp; b < fr.gridc; b += 32u) s += rows[(size_t)b * 8 + col];
            part[grp][col] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                float v[6];
                scene_rows_to_camera(part, fr.inv_n, a.objs[j].Tow, a.poses + fr.pose, grad, v);
                for (int k = 0; k < 6; ++k) og[6u * j + k] += v[k];
            }
            __syncthreads();
        }
        float ls = 0.f;
        for (uint32_t b = threadIdx.x; b < fr.parts; b += 256u) ls += a.loss_part[fr.lp0 + b];
        lpart[threadIdx.x] = ls;
        __syncthreads();
        if (threadIdx.x == 0) {
            float loss = 0.f;
            for (int g = 0; g < 256; ++g) loss += lpart[g];
            loss *= fr.inv_n;
            Lf[f] = loss; L += loss;
            for (int k = 0; k < 6; ++k) cg[6u * f + k] = grad[k];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    o[0] = L;
    if (!a.step) return;
    for (uint32_t f = a.n_fixed; f < a.n_frames; ++f)
        scene_camera_adam_step(cg + 6u * f, a.moments + 12u * f, a.lr_t, a.lr_r, a.it, a.poses + a.frames[f].pose);
    if (a.refine_objs)
        for (uint32_t j = 0; j < a.n_objs; ++j)
            scene_object_adam_step(og + 6u * j, a.moments + 12u * (a.n_frames + j), a.lr_obj_t, a.lr_obj_r, a.it, a.objs[j].Tow);
}

// ------------------------------------------------------------------ launchers
void launch_scene_window_rays(hipStream_t s, const SceneWindowRayArgs& a) {
    if (!a.n_rays || !a.n_objs || !a.n_frames) return;
    hipLaunchKernelGGL(k_scene_window_rays, dim3((a.n_rays + 255) / 256), dim3(256), 0, s, a);
}
void launch_scene_window_update(hipStream_t s, const SceneWindowUpdateArgs& a) {
    hipLaunchKernelGGL(k_scene_window_update, dim3(1), dim3(256), 0, s, a);
}

}  // namespace mon
