// pose.cpp -- object pose refinement through a trained object NeRF: the host side of kernels_pose.hip
#include <cmath>
#include <cstring>
#include "model_internal.h"

namespace mon {
// ---- pose refinement (mon_object_pose_loss / mon_object_refine_pose): k_pose_rays -> k_pose_grad -> k_pose_update per evaluation, the pose in device memory
// Per object and side, grow-only, freed with the object: a viewer (side 1) and the trainer (side 0) run at the same time.  A call holds `mu` until its stream
// has been synchronised.
struct PoseWs {
    std::mutex mu;
    DevBuf<float4> rec;                                                           // ray records, 4 float4 per drawn ray
    DevBuf<float> out;                                                            // {loss, grad6, 0} per evaluation
    DevBuf<mon_frame_bbox> boxes; DevBuf<uint32_t> prefix;
    DevBuf<float> small;                                                          // partials [kPoseMaxGrid][8] | pose [16] | moments [12]
    DevBuf<uint16_t> frag;                                                        // the A-fragment image, backward fragments included
    DevBuf<float> dbg;                                                            // mon_debug_pose_samples: x | raw | dL/dx of every sample
    DevBuf<float> lw;                                                             // level weights [evaluation][L] of the weighted calls
};
static std::mutex g_pose_mu;
static PoseWs& pose_ws(Model& m, int side) { std::lock_guard<std::mutex> l(g_pose_mu); if (!m.pose_ws[side]) m.pose_ws[side] = new PoseWs(); return *m.pose_ws[side]; }
void pose_ws_free(Model& m) { for (int k = 0; k < 2; ++k) { delete m.pose_ws[k]; m.pose_ws[k] = nullptr; } }
int pose_box_check(const char* what, const Dataset& ds, const mon_frame_bbox& b, size_t i, uint64_t& total) {
    if (b.FrameId >= ds.max_frames || !ds.present[b.FrameId]) { set_error("%s: box %zu names frame %u, which the dataset does not hold", what, i, b.FrameId);
        return MON_ERR_ARG; }
    if (b.w == 0 || b.h == 0 || (uint64_t)b.x + b.w > (uint64_t)ds.K.W || (uint64_t)b.y + b.h > (uint64_t)ds.K.H) {
        set_error("%s: box %zu (frame %u, x %u y %u h %u w %u) empty or outside the %dx%d frame", what, i, b.FrameId, b.x, b.y, b.h, b.w, ds.K.W, ds.K.H);
        return MON_ERR_ARG; }
    total += (uint64_t)b.w * b.h;                                                   // (a frame is at most 2^31 pixels; 2^22 boxes of them would not fit)
    if (total > kPoseMaxRays * 64ull) { set_error("%s: the boxes hold too many pixels", what); return MON_ERR_ARG; }
    return MON_OK;
}
uint32_t pose_n_rays(const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params& p) {
    if (p.rays_per_iter) return p.rays_per_iter;
    uint64_t t = 0; for (size_t i = 0; i < n_obs; ++i) t += (uint64_t)obs[i].w * obs[i].h;
    return t > 0xffffffffull ? 0xffffffffu : (uint32_t)t;
}
int pose_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p) {
    REQUIRE_ARG("pose", obs, "obs"); REQUIRE_ARG("pose", Tow16, "pose"); REQUIRE_ARG("pose", p, "params");
    if (n_obs == 0) { set_error("pose: no boxes"); return MON_ERR_ARG; }
    if (p->iters < 0) { set_error("pose: iters %d < 0", p->iters); return MON_ERR_ARG; }
    if (side != 0 && side != 1) { set_error("pose: side %d (0 or 1)", side); return MON_ERR_ARG; }
    return MON_OK;
}
int level_weights_check(const char* what, const float* w, int n) {
    for (int l = 0; l < n; ++l)
        if (!std::isfinite(w[l]) || w[l] < 0.f) { set_error("%s: level weight %d is %g (finite, >= 0)", what, l, w[l]); return MON_ERR_ARG; }
    return MON_OK;
}
int pose_refine(Model& m, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params& p, int iters,
                uint32_t iteration, float* pose_out, float* loss_trace, float* loss, float* grad6, const PoseDump* dump, const float* level_w) {
    if (p.rays_per_iter > kPoseMaxRays) { set_error("pose: rays_per_iter %u above %u", p.rays_per_iter, kPoseMaxRays); return MON_ERR_ARG; }
    std::vector<uint32_t> prefix(n_obs + 1, 0u);
    {   uint64_t t = 0;
        for (size_t i = 0; i < n_obs; ++i) { const int rc = pose_box_check("pose", *m.ds, obs[i], i, t); if (rc) return rc; prefix[i + 1] = (uint32_t)t; } }
    if (!rskip_supported(m) || 2u * m.oc.S != 64u) { set_error("pose: this object does not run on the fused kernels"); return MON_ERR_STATE; }
    if (m.d_xw) { set_error("pose: this object renders with the XORWOW sample stream (rng_flags)"); return MON_ERR_STATE; }
    if (side == 1 && !model_has_snapshot(m)) { set_error("pose: side 1 and nothing published yet"); return MON_ERR_STATE; }
    const uint32_t total = prefix[n_obs], n_rays = p.rays_per_iter ? p.rays_per_iter : total;
    if (!p.rays_per_iter && total > kPoseMaxRays) { set_error("pose: %u pixels in the boxes (at most %u with rays_per_iter = 0)", total, kPoseMaxRays);
        return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device));
    const int n_eval = iters < 0 ? 1 : iters + 1;
    // the weights of the side, and its stream
    hipStream_t s; const uint16_t* prm;
    std::unique_lock<std::mutex> dev_lock;
    SnapshotPin pin;
    if (side == 1) {
        InferShared* sh = m.infer->shared; dev_lock = std::unique_lock<std::mutex>(sh->mu); s = sh->stream;
        { const int rc = pin.take(m.infer, s); if (rc) return rc; }
        prm = pin.snap();
    } else {
        model_leave_lane(m); { const int rc = ensure_ema_current(m); if (rc) return rc; }
        s = m.train_stream; prm = (m.h_state.step > 0) ? m.P.ema : m.P.half;
    }
    PoseWs& w = pose_ws(m, side); std::lock_guard<std::mutex> wl(w.mu);
    const FragDims fd{ m.nd.Epad, m.nd.W, m.nd.NH, m.nd.L };
    int rc;
    if ((rc = w.rec.grow(4 * (size_t)n_rays)) || (rc = w.out.grow(8 * (size_t)n_eval)) || (rc = w.prefix.grow(n_obs + 1)) || (rc = w.boxes.grow(n_obs)) ||
        (rc = w.small.grow((size_t)kPoseMaxGrid * 8 + 16 + 12)) || (rc = w.frag.grow((size_t)fd.N_FRAGS() * 512))) return rc;
    float* partials = w.small.p; float* d_pose = partials + (size_t)kPoseMaxGrid * 8; float* d_mom = d_pose + 16;
    float *dx = nullptr, *draw = nullptr, *dg = nullptr;
    if (dump) {
        if ((rc = w.dbg.grow((size_t)n_rays * 64 * 10))) return rc;
        dx = w.dbg.p; draw = dx + (size_t)n_rays * 64 * 3; dg = dx + (size_t)n_rays * 64 * 7;
    }
    // weighted: one row of L per evaluation that steps (or the one evaluation of iters < 0); the last evaluation of a refinement, whose gradient is not
    // used, runs unweighted (the loss does not depend on the weights)
    const int L = (int)m.nd.L, n_wrows = level_w ? (iters < 0 ? 1 : iters) : 0;
    if (n_wrows) {
        if ((rc = w.lw.grow((size_t)n_wrows * L))) return rc;
        HIPCHECK(hipMemcpyAsync(w.lw.p, level_w, sizeof(float) * (size_t)n_wrows * L, hipMemcpyHostToDevice, s));
    }
    HIPCHECK(hipMemcpyAsync(w.boxes.p, obs, sizeof(mon_frame_bbox) * n_obs, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(w.prefix.p, prefix.data(), 4 * (n_obs + 1), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_pose, Tow16, 64, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(d_mom, 0, 48, s));
    const bool drawn = p.rays_per_iter != 0;
    const uint32_t grid = pose_grad_grid(n_rays);
    for (int it = 0; it < n_eval; ++it) {
        const uint32_t key = iters < 0 ? iteration : (uint32_t)it;
        PoseRayArgs ra{}; ra.boxes = w.boxes.p; ra.prefix = w.prefix.p; ra.n_obs = (uint32_t)n_obs; ra.n_rays = n_rays; ra.total = total; ra.drawn = drawn ? 1u : 0u;
        ra.iteration = key; ra.seed = p.seed; ra.ds = m.ds->ptrs(); ra.aabb = m.oc.aabb; ra.instance_id = m.oc.instance_id; ra.pose = d_pose; ra.rec = w.rec.p;
        launch_pose_rays(s, ra);
        PoseGradArgs ga{}; ga.rec = w.rec.p; ga.n_rays = n_rays;
        ga.seed = drawn ? p.seed : m.oc.sample_seed; ga.stream = drawn ? kStreamPose : (uint32_t)kStreamRender; ga.step = drawn ? key : 0u;
        ga.w_rgb = p.w_rgb; ga.w_mask = p.w_mask; ga.w_depth = p.w_depth; ga.huber = p.depth_huber; ga.inv_n = 1.f / (float)n_rays;
        ga.partials = partials; ga.dbg_x = dx; ga.dbg_raw = draw; ga.dbg_g = dg;
        launch_pose_grad(s, m.lf, m.nd, m.oc, prm, w.frag.p, it == 0, ga, it < n_wrows ? w.lw.p + (size_t)it * L : nullptr);
        launch_pose_update(s, partials, grid, 1.f / (float)n_rays, w.out.p, nullptr, (uint32_t)it, iters >= 0 && it < iters, p.lr_trans, p.lr_rot, d_pose, d_mom);
    }
    HIPCHECK(hipGetLastError());
    std::vector<float> h_out(8 * (size_t)n_eval); float h_pose[16];
    HIPCHECK(hipMemcpyAsync(h_out.data(), w.out.p, 32 * (size_t)n_eval, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(h_pose, d_pose, 64, hipMemcpyDeviceToHost, s));
    std::vector<float> h_dbg;
    if (dump) { h_dbg.resize((size_t)n_rays * 64 * 10); HIPCHECK(hipMemcpyAsync(h_dbg.data(), w.dbg.p, h_dbg.size() * 4, hipMemcpyDeviceToHost, s)); }
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    if (loss) *loss = h_out[0];
    if (grad6) for (int j = 0; j < 6; ++j) grad6[j] = h_out[1 + j];
    if (loss_trace) for (int it = 0; it < n_eval; ++it) loss_trace[it] = h_out[8 * (size_t)it];
    if (pose_out) std::memcpy(pose_out, h_pose, 64);
    if (dump) {
        const size_t ns = (size_t)n_rays * 64;
        if (dump->x) std::memcpy(dump->x, h_dbg.data(), ns * 12);
        if (dump->raw) std::memcpy(dump->raw, h_dbg.data() + ns * 3, ns * 16);
        if (dump->dldx) std::memcpy(dump->dldx, h_dbg.data() + ns * 7, ns * 12);
    }
    return MON_OK;
}

}  // namespace mon
