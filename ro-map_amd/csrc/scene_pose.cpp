// scene_pose.cpp -- the scene pose family: camera refinement against several object NeRFs, batched hypothesis scoring, the window of frames and object
// poses, relocalisation.  The boundary and the entry to a side are scene.cpp's (model_internal.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include "model_internal.h"

namespace mon {
// ---- camera refinement against a scene of objects (mon_scene_pose_loss / mon_scene_refine_camera): per evaluation and chunk of rays k_scene_pose_rays ->
// every object's k_scene_pose_obj (forward) -> k_scene_composite_grad -> every object's k_scene_pose_obj (backward), then k_scene_pose_update; the camera
// pose lives in device memory between steps.  Per device and side, grow-only, never freed (like SceneWs, whose users are untouched).  A call holds `mu` until
// its stream has been synchronised.
struct ScenePoseWs {
    std::mutex mu;
    DevBuf<float> t; DevBuf<float4> attr; DevBuf<float2> gw;                      // [objects][cap][64]
    DevBuf<uint32_t> cnt; DevBuf<float> mstar; DevBuf<float4> rec;                // [objects][cap]( x 3)
    DevBuf<float4> ray, grow;                                                     // [cap] x 3, [cap]
    DevBuf<float> partials, loss_part;
    DevBuf<SceneObjConst> objs; DevBuf<uint16_t> frag;
    DevBuf<mon_frame_bbox> boxes; DevBuf<uint32_t> prefix;
    DevBuf<float> small;                                                          // pose [16] | moments [12]
    DevBuf<float> out; PinnedBuf<float> h_out;                                    // {loss, grad6, 0} per evaluation | pose; pinned staging
    DevBuf<float> lw;                                                             // level weights [evaluation][Lmax]
    DevBuf<float> dbg; DevBuf<uint32_t> dbg_cnt;
    DevBuf<float> poses, scores; PinnedBuf<float> h_scores;                       // scene_pose_batch: [hypotheses][16], [hypotheses], their pinned staging
    DevBuf<SceneWinFrame> wframes; DevBuf<float> wmom;                            // scene_window: the frame table, moments [F + K][12]
    std::vector<hipEvent_t> ev;
};
// what scene_pose asks of its arguments without an object ...
int scene_pose_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16, const mon_pose_refine_params* p) {
    REQUIRE_ARG("scene pose", obs, "obs"); REQUIRE_ARG("scene pose", Twc16, "pose"); REQUIRE_ARG("scene pose", p, "params");
    if (n_obs == 0) { set_error("scene pose: no boxes"); return MON_ERR_ARG; }
    if (p->iters < 0) { set_error("scene pose: iters %d < 0", p->iters); return MON_ERR_ARG; }
    return side_check("scene pose", side);
}
// ... and of the rays: at most kPoseMaxRays of them, the boxes of one frame, each inside a frame the objects' dataset holds.  (The first two need no object.
// They stand here because the online manager has always reported "nothing published yet", a MON_ERR_STATE, in front of them.)
static int scene_boxes_check(const Dataset& ds, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params& p) {
    if (p.rays_per_iter > kPoseMaxRays) { set_error("scene pose: rays_per_iter %u above %u", p.rays_per_iter, kPoseMaxRays); return MON_ERR_ARG; }
    uint64_t total = 0;
    for (size_t i = 0; i < n_obs; ++i) {
        if (obs[i].FrameId != obs[0].FrameId) { set_error("scene pose: boxes name frames %u and %u (one frame per call)", obs[0].FrameId, obs[i].FrameId);
            return MON_ERR_ARG; }
        { const int rc = pose_box_check("scene pose", ds, obs[i], i, total); if (rc) return rc; }
    }
    if (!p.rays_per_iter && total > kPoseMaxRays) { set_error("scene pose: %llu pixels in the boxes (at most %u with rays_per_iter = 0)",
        (unsigned long long)total, kPoseMaxRays); return MON_ERR_ARG; }
    return MON_OK;
}
int scene_pose_objects_check(Model* const* ms, size_t n, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p) {
    { const int rc = scene_objects_check("scene pose", ms, n, true, true); if (rc) return rc; }
    return scene_boxes_check(*ms[0]->ds, obs, n_obs, *p);
}

// ---- what scene_pose, scene_pose_batch and scene_window set up alike.
// the exclusive prefix sums of a frame's box areas, n + 1 entries appended to `prefix`; returns the frame's pixels
static uint32_t append_prefix(std::vector<uint32_t>& prefix, const mon_frame_bbox* obs, size_t n) {
    uint32_t total = 0; for (size_t i = 0; i < n; ++i) { prefix.push_back(total); total += obs[i].w * obs[i].h; } prefix.push_back(total);
    return total;
}
// The prologue of a call whose passes hold at most `cap` rays: the list buffers every pass's ray kernel, forward launches and composite write (`n_lp` loss
// partials), object j's fragment image at frag_off[j], and on stream s the level weights (n_wrows rows of Lmax, or none), the object table (Tow16s, where
// given, in place of the objects' own poses), the boxes and their prefix sums.  The camera pose(s) and whatever else a route keeps on the device follow.
static int scene_pose_prologue(ScenePoseWs& w, hipStream_t s, Model* const* ms, size_t n, const float* Tow16s, const mon_frame_bbox* obs, size_t n_obs,
                               const std::vector<uint32_t>& prefix, uint32_t cap, size_t n_lp, const float* level_w, int n_wrows, int Lmax,
                               std::vector<size_t>& frag_off) {
    frag_off.assign(n + 1, 0);
    for (size_t j = 0; j < n; ++j) { const NetDims& nd = ms[j]->nd; const FragDims fd{ nd.Epad, nd.W, nd.NH, nd.L }; frag_off[j + 1] = frag_off[j] + (size_t)fd.N_FRAGS() * 512; }
    const size_t lists = n * (size_t)cap;
    int rc;
    if ((rc = w.t.grow(lists * kSceneListLen)) || (rc = w.attr.grow(lists * kSceneListLen)) || (rc = w.cnt.grow(lists)) || (rc = w.mstar.grow(lists)) ||
        (rc = w.rec.grow(lists * 3)) || (rc = w.ray.grow((size_t)cap * 3)) || (rc = w.loss_part.grow(n_lp)) || (rc = w.objs.grow(n)) ||
        (rc = w.frag.grow(frag_off[n])) || (rc = w.boxes.grow(n_obs)) || (rc = w.prefix.grow(prefix.size()))) return rc;
    if (n_wrows) {
        if ((rc = w.lw.grow((size_t)n_wrows * Lmax))) return rc;
        HIPCHECK(hipMemcpyAsync(w.lw.p, level_w, sizeof(float) * (size_t)n_wrows * Lmax, hipMemcpyHostToDevice, s));
    }
    std::vector<SceneObjConst> h_objs(n);
    for (size_t j = 0; j < n; ++j) { const ObjectConst& oc = ms[j]->oc; std::memcpy(h_objs[j].Tow, Tow16s ? Tow16s + 16 * j : oc.Tow.m, 64); h_objs[j].aabb = oc.aabb;
        h_objs[j].instance_id = oc.instance_id; h_objs[j].pad = 0u; }
    HIPCHECK(hipMemcpyAsync(w.objs.p, h_objs.data(), sizeof(SceneObjConst) * n, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(w.boxes.p, obs, sizeof(mon_frame_bbox) * n_obs, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(w.prefix.p, prefix.data(), 4 * prefix.size(), hipMemcpyHostToDevice, s));
    return MON_OK;
}
// ... and of the routes with a backward pass: what the composite backward writes into every list slot and per ray, `rows` partial rows per object
static int scene_pose_backward_bufs(ScenePoseWs& w, size_t n, uint32_t cap, size_t rows) {
    int rc;
    if ((rc = w.gw.grow(n * (size_t)cap * kSceneListLen)) || (rc = w.grow.grow((size_t)cap)) || (rc = w.partials.grow(n * rows * 8))) return rc;
    return MON_OK;
}
// the ray kernel's arguments that do not depend on the pass (n_rays, ray0, pose and a route's own fields follow)
static void scene_ray_args(ScenePoseRayArgs& ra, const ScenePoseWs& w, Model* const* ms, size_t n, uint32_t cap, const mon_pose_refine_params& p,
                           uint32_t key) {
    ra.boxes = w.boxes.p; ra.prefix = w.prefix.p; ra.drawn = p.rays_per_iter ? 1u : 0u; ra.iteration = key; ra.seed = p.seed; ra.ds = ms[0]->ds->ptrs();
    ra.objs = w.objs.p; ra.n_objs = (uint32_t)n; ra.cap = cap; ra.rec = w.rec.p; ra.mstar = w.mstar.p; ra.ray = w.ray.p;
}
// object j's forward over n_rays rays of a pass of `cap`: its records and lists, the jitter key (the backward's inputs follow where there is one)
static ScenePoseObjArgs scene_obj_args(const ScenePoseWs& w, const Model& m, size_t j, uint32_t cap, uint32_t n_rays, uint32_t ray0,
                                       const mon_pose_refine_params& p, uint32_t key, float inv_n) {
    const size_t l0 = j * (size_t)cap; const bool drawn = p.rays_per_iter != 0;
    ScenePoseObjArgs a{}; a.rec = w.rec.p + l0 * 3; a.n_rays = n_rays; a.ray0 = ray0;
    a.seed = drawn ? p.seed : m.oc.sample_seed; a.stream = drawn ? kStreamPose : (uint32_t)kStreamRender; a.step = drawn ? key : 0u;
    a.t = w.t.p + l0 * kSceneListLen; a.attr = w.attr.p + l0 * kSceneListLen; a.cnt = w.cnt.p + l0; a.ray = w.ray.p; a.inv_n = inv_n;
    return a;
}
static void scene_obj_backward_args(ScenePoseObjArgs& a, const ScenePoseWs& w, size_t j, uint32_t cap, float* partials, const float* level_w) {
    a.gw = w.gw.p + j * (size_t)cap * kSceneListLen; a.grow = w.grow.p; a.partials = partials; a.level_w = level_w;
}
// the composite's view of a pass: every object's lists, the targets, the loss weights (loss_part and, with a backward pass, gw and grow follow)
static SceneCompGradArgs scene_comp_args(const ScenePoseWs& w, size_t n, uint32_t cap, uint32_t n_rays, const mon_pose_refine_params& p) {
    SceneCompGradArgs ca{}; ca.n_rays = n_rays; ca.n_lists = (uint32_t)n; ca.cap = cap; ca.t = w.t.p; ca.attr = w.attr.p; ca.cnt = w.cnt.p; ca.mstar = w.mstar.p;
    ca.ray = w.ray.p; ca.w_rgb = p.w_rgb; ca.w_mask = p.w_mask; ca.w_depth = p.w_depth; ca.huber = p.depth_huber;
    return ca;
}

int scene_pose(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16, const mon_pose_refine_params& p, int iters,
               uint32_t iteration, float* pose_out, float* loss_trace, float* loss, float* grad6, const ScenePoseDump* dump, const float* level_w) {
    { const int rc = scene_state_check("scene pose", ms, n, side); if (rc) return rc; }
    const int Lmax = scene_levels(ms, n).Lmax;
    std::vector<uint32_t> prefix;
    const uint32_t total = append_prefix(prefix, obs, n_obs), n_rays = p.rays_per_iter ? p.rays_per_iter : total;
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const int n_eval = iters < 0 ? 1 : iters + 1;
    ScenePoseWs& w = side_ws<ScenePoseWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, w.mu, w.ev); if (rc) return rc; }
    const std::vector<const uint16_t*>& prm = sd.prm; const hipStream_t s = sd.s;
    // chunks of the rays (the cap scene_render chunks its rect by); each chunk's partial rows follow the previous chunk's
    const uint32_t cap = std::min(n_rays, kRenderChunkRays), n_chunks = (n_rays + cap - 1u) / cap;
    const uint32_t gridc = std::min(pose_grad_grid(cap), std::max(1u, kPoseMaxGrid / n_chunks)), n_rows = n_chunks * gridc;
    uint32_t n_lp = 0; for (uint32_t c = 0; c < n_chunks; ++c) n_lp += scene_comp_grad_grid(std::min(cap, n_rays - c * cap));
    const size_t out_floats = 8 * (size_t)n_eval + 16;
    int rc;
    if ((rc = scene_pose_backward_bufs(w, n, cap, n_rows)) || (rc = w.small.grow(28)) || (rc = w.out.grow(out_floats)) || (rc = w.h_out.grow(out_floats))) return rc;
    if (dump) { if ((rc = w.dbg.grow((size_t)n_rays * 64 * 14)) || (rc = w.dbg_cnt.grow((size_t)n_rays))) return rc; }
    const int n_wrows = level_w ? (iters < 0 ? 1 : iters) : 0;
    std::vector<size_t> frag_off;
    if ((rc = scene_pose_prologue(w, s, ms, n, nullptr, obs, n_obs, prefix, cap, n_lp, level_w, n_wrows, Lmax, frag_off))) return rc;
    float* d_pose = w.small.p; float* d_mom = d_pose + 16;
    HIPCHECK(hipMemcpyAsync(d_pose, Twc16, 64, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(d_mom, 0, 48, s));
    const float inv_n = 1.f / (float)n_rays;
    std::vector<ScenePoseObjArgs> oa(n);
    for (int it = 0; it < n_eval; ++it) {
        const uint32_t key = iters < 0 ? iteration : (uint32_t)it;
        const float* lw_row = it < n_wrows ? w.lw.p + (size_t)it * Lmax : nullptr;
        uint32_t lp_off = 0;
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t p0 = c * cap, nc = std::min(cap, n_rays - p0);
            ScenePoseRayArgs ra{}; scene_ray_args(ra, w, ms, n, cap, p, key);
            ra.n_obs = (uint32_t)n_obs; ra.n_rays = nc; ra.ray0 = p0; ra.total = total; ra.pose = d_pose;
            launch_scene_pose_rays(s, ra);
            for (size_t j = 0; j < n; ++j) {
                Model& m = *ms[j];
                oa[j] = scene_obj_args(w, m, j, cap, nc, p0, p, key, inv_n);
                scene_obj_backward_args(oa[j], w, j, cap, w.partials.p + ((size_t)j * n_rows + (size_t)c * gridc) * 8, lw_row);
                oa[j].dbg = (dump && dump->k == j) ? w.dbg.p : nullptr;
                launch_scene_pose_obj(s, m.lf, m.nd, m.oc, prm[j], w.frag.p + frag_off[j], it == 0 && c == 0, 0, pose_grad_grid(nc), oa[j]);
            }
            SceneCompGradArgs ca = scene_comp_args(w, n, cap, nc, p); ca.gw = w.gw.p; ca.grow = w.grow.p; ca.loss_part = w.loss_part.p + lp_off;
            launch_scene_composite_grad(s, ca);
            lp_off += scene_comp_grad_grid(nc);
            for (size_t j = 0; j < n; ++j) { Model& m = *ms[j];
                launch_scene_pose_obj(s, m.lf, m.nd, m.oc, prm[j], w.frag.p + frag_off[j], 0, 1, gridc, oa[j]); }
            if (dump) HIPCHECK(hipMemcpyAsync(w.dbg_cnt.p + p0, w.cnt.p + dump->k * (size_t)cap, 4 * (size_t)nc, hipMemcpyDeviceToDevice, s));
        }
        ScenePoseUpdateArgs ua{}; ua.partials = w.partials.p; ua.n_objs = (uint32_t)n; ua.n_rows = n_rows; ua.row_stride = n_rows; ua.loss_part = w.loss_part.p;
        ua.n_loss_parts = n_lp; ua.objs = w.objs.p; ua.inv_n = inv_n; ua.out = w.out.p; ua.it = (uint32_t)it; ua.step = iters >= 0 && it < iters;
        ua.lr_t = p.lr_trans; ua.lr_r = p.lr_rot; ua.pose = d_pose; ua.moments = d_mom;
        launch_scene_pose_update(s, ua);
    }
    HIPCHECK(hipGetLastError());
    // results home through the pinned staging: {loss, grad6, 0} of every evaluation, then the pose
    // (copy kernels on the call's stream, as the scene render's results go home)
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(d_pose), reinterpret_cast<uint16_t*>(w.out.p + 8 * (size_t)n_eval), 32u);
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(w.out.p), reinterpret_cast<uint16_t*>(w.h_out.p), (uint32_t)(out_floats * 2));
    std::vector<float> h_dbg; std::vector<uint32_t> h_cnt;
    if (dump) { h_dbg.resize((size_t)n_rays * 64 * 14); h_cnt.resize(n_rays);
        HIPCHECK(hipMemcpyAsync(h_dbg.data(), w.dbg.p, h_dbg.size() * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(h_cnt.data(), w.dbg_cnt.p, (size_t)n_rays * 4, hipMemcpyDeviceToHost, s)); }
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    const float* h = w.h_out.p;
    if (loss) *loss = h[0];
    if (grad6) for (int j = 0; j < 6; ++j) grad6[j] = h[1 + j];
    if (loss_trace) for (int it = 0; it < n_eval; ++it) loss_trace[it] = h[8 * (size_t)it];
    if (pose_out) std::memcpy(pose_out, h + 8 * (size_t)n_eval, 64);
    if (dump) {
        for (size_t i = 0; i < (size_t)n_rays * 64; ++i) {
            const float* q = h_dbg.data() + 14 * i;
            if (dump->x_o) std::memcpy(dump->x_o + 3 * i, q, 12);
            if (dump->x_c) std::memcpy(dump->x_c + 3 * i, q + 3, 12);
            if (dump->t) dump->t[i] = q[6];
            if (dump->raw) std::memcpy(dump->raw + 4 * i, q + 7, 16);
            if (dump->dldx) std::memcpy(dump->dldx + 3 * i, q + 11, 12);
        }
        if (dump->count) std::memcpy(dump->count, h_cnt.data(), 4 * (size_t)n_rays);
    }
    return MON_OK;
}

// ---- batched pose scoring (mon_scene_pose_loss_batch): the forward half of scene_pose's chain over n_poses camera poses.  A pass holds G = floor(cap / n)
// hypotheses of n rays each as G n virtual rays in scene_pose's own list workspace (no more list memory than one evaluation of the chunk cap takes): K + 3
// launches per pass, everything enqueued at once, one synchronisation, one copy home.
static_assert(kSceneScoreMaxRays == kRenderChunkRays, "a hypothesis holds at most one chunk of scene_pose's rays");
int scene_pose_batch_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, size_t n_poses, const mon_pose_refine_params* p,
                           const float* losses) {
    REQUIRE_ARG("scene pose batch", Twc16s, "Twc16s"); REQUIRE_ARG("scene pose batch", losses, "losses");
    if (n_poses == 0 || n_poses > kSceneScoreMaxPoses) { set_error("scene pose batch: %zu poses (1 to %u)", n_poses, kSceneScoreMaxPoses); return MON_ERR_ARG; }
    if (p && p->rays_per_iter > kSceneScoreMaxRays) { set_error("scene pose batch: rays_per_iter %u (at most %u per hypothesis)", p->rays_per_iter,
        kSceneScoreMaxRays); return MON_ERR_ARG; }
    return scene_pose_check(side, obs, n_obs, Twc16s, p);
}
int scene_pose_batch_objects_check(Model* const* ms, size_t n, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p) {
    { const int rc = scene_pose_objects_check(ms, n, obs, n_obs, p); if (rc) return rc; }
    const uint64_t n_rays = pose_n_rays(obs, n_obs, *p);
    if (n_rays > kSceneScoreMaxRays) { set_error("scene pose batch: %llu rays per hypothesis (at most %u)", (unsigned long long)n_rays, kSceneScoreMaxRays);
        return MON_ERR_ARG; }
    return MON_OK;
}
int scene_pose_batch(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, size_t n_poses,
                     const mon_pose_refine_params& p, uint32_t iteration, float* losses) {
    { const int rc = scene_state_check("scene pose", ms, n, side); if (rc) return rc; }
    std::vector<uint32_t> prefix;
    const uint32_t total = append_prefix(prefix, obs, n_obs), n_rays = p.rays_per_iter ? p.rays_per_iter : total, H = (uint32_t)n_poses;
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    ScenePoseWs& w = side_ws<ScenePoseWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, w.mu, w.ev); if (rc) return rc; }
    const std::vector<const uint16_t*>& prm = sd.prm; const hipStream_t s = sd.s;
    // passes of Gmax whole hypotheses (n_rays <= the chunk cap, so Gmax >= 1); virtual ray v = g * n_rays + r at slot v of the lists
    const uint32_t Gmax = std::min(H, kSceneScoreMaxRays / n_rays), cap = Gmax * n_rays, parts = scene_comp_grad_grid(n_rays);
    int rc;
    if ((rc = w.poses.grow((size_t)H * 16)) || (rc = w.scores.grow((size_t)H)) || (rc = w.h_scores.grow((size_t)H))) return rc;
    std::vector<size_t> frag_off;
    if ((rc = scene_pose_prologue(w, s, ms, n, nullptr, obs, n_obs, prefix, cap, (size_t)Gmax * parts, nullptr, 0, 0, frag_off))) return rc;
    HIPCHECK(hipMemcpyAsync(w.poses.p, Twc16s, 64 * (size_t)H, hipMemcpyHostToDevice, s));
    const float inv_n = 1.f / (float)n_rays;
    for (uint32_t h0 = 0; h0 < H; h0 += Gmax) {
        const uint32_t G = std::min(Gmax, H - h0), nv = G * n_rays;
        SceneScoreRayArgs ra{}; scene_ray_args(ra, w, ms, n, cap, p, iteration);
        ra.n_obs = (uint32_t)n_obs; ra.n_rays = nv; ra.ray0 = 0u; ra.total = total; ra.pose = w.poses.p; ra.n_per = n_rays; ra.h0 = h0;
        launch_scene_score_rays(s, ra);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j];
            launch_scene_pose_obj(s, m.lf, m.nd, m.oc, prm[j], w.frag.p + frag_off[j], h0 == 0, 0, pose_grad_grid(nv),
                    scene_obj_args(w, m, j, cap, nv, 0u, p, iteration, inv_n));
        }
        SceneCompGradArgs ca = scene_comp_args(w, n, cap, nv, p); ca.loss_part = w.loss_part.p;
        launch_scene_composite_loss(s, ca, n_rays);
        launch_scene_loss_reduce(s, w.loss_part.p, G, parts, inv_n, w.scores.p + h0);
    }
    HIPCHECK(hipGetLastError());
    // (a copy kernel on the call's stream into the pinned staging, as scene_pose's results go home)
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(w.scores.p), reinterpret_cast<uint16_t*>(w.h_scores.p), H * 2u);
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    std::memcpy(losses, w.h_scores.p, (size_t)H * 4);
    return MON_OK;
}

// ---- window refinement (mon_scene_window_loss / mon_scene_refine_window): scene_pose's chain over the frames of a window, whole frames packed as virtual
// rays into scene_pose's list workspace (passes of at most kWindowPassRays rays, greedily in window order): passes x (2K + 2) + 1 launches per evaluation,
// every camera pose and every object's Tow on the device between steps, everything enqueued at once, one synchronisation.
int window_frames(const mon_frame_bbox* obs, size_t n_obs, uint32_t* frame_ids, size_t* n_frames) {
    if (!obs || !frame_ids || !n_frames) { set_error("window frames: null argument"); return MON_ERR_ARG; }
    size_t F = 0;
    for (size_t i = 0; i < n_obs; ++i) {
        if (i && obs[i].FrameId == obs[i - 1].FrameId) continue;
        for (size_t k = 0; k < F; ++k) if (frame_ids[k] == obs[i].FrameId) {
            set_error("window frames: the boxes of frame %u are not contiguous (box %zu)", obs[i].FrameId, i); return MON_ERR_ARG; }
        if (F == kWindowMaxFrames) { set_error("window frames: more than %u frames", kWindowMaxFrames); return MON_ERR_ARG; }
        frame_ids[F++] = obs[i].FrameId;
    }
    *n_frames = F;
    return MON_OK;
}
int scene_window_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, const mon_pose_refine_params* p, const mon_window_params* w,
                       const float* Tow16s, bool refine) {
    REQUIRE_ARG("scene window", obs, "obs"); REQUIRE_ARG("scene window", Twc16s, "Twc16s"); REQUIRE_ARG("scene window", p, "params");
    if (refine) REQUIRE_ARG("scene window", w, "window params");
    if (n_obs == 0) { set_error("scene window: no boxes"); return MON_ERR_ARG; }
    if (p->iters < 0) { set_error("scene window: iters %d < 0", p->iters); return MON_ERR_ARG; }
    { const int rc = side_check("scene pose", side); if (rc) return rc; }
    uint32_t ids[kWindowMaxFrames]; size_t F = 0;
    { const int rc = window_frames(obs, n_obs, ids, &F); if (rc) return rc; }
    if (refine) {
        if (w->n_fixed_frames > F) { set_error("scene window: n_fixed_frames %u of %zu frames", w->n_fixed_frames, F); return MON_ERR_ARG; }
        if (!std::isfinite(w->lr_obj_trans) || !std::isfinite(w->lr_obj_rot) || w->lr_obj_trans < 0.f || w->lr_obj_rot < 0.f) {
            set_error("scene window: object step sizes %g, %g (finite, >= 0)", w->lr_obj_trans, w->lr_obj_rot); return MON_ERR_ARG; }
        if (w->refine_objects && w->n_fixed_frames == 0) {
            set_error("scene window: refine_objects with no fixed frame (nothing would hold the map in place)"); return MON_ERR_ARG; }
        if (w->refine_objects && !Tow16s) { set_error("scene window: refine_objects with a null Tow16s"); return MON_ERR_ARG; }
    }
    return MON_OK;
}
// ... and what needs the objects (the frames are contiguous, at most kWindowMaxFrames): each frame's boxes as scene_pose takes them, its rays in one pass
int scene_window_objects_check(Model* const* ms, size_t n, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16s, const mon_pose_refine_params* p) {
    { const int rc = scene_objects_check("scene pose", ms, n, true, true); if (rc) return rc; }
    for (size_t i0 = 0; i0 < n_obs; ) {
        size_t i1 = i0 + 1; while (i1 < n_obs && obs[i1].FrameId == obs[i0].FrameId) ++i1;
        { const int rc = scene_boxes_check(*ms[0]->ds, obs + i0, i1 - i0, *p); if (rc) return rc; }
        const uint64_t n_rays = pose_n_rays(obs + i0, i1 - i0, *p);
        if (n_rays > kWindowPassRays) { set_error("scene window: %llu rays in frame %u (at most %u: a frame is never split across passes)",
            (unsigned long long)n_rays, obs[i0].FrameId, kWindowPassRays); return MON_ERR_ARG; }
        i0 = i1;
    }
    if (Tow16s) for (size_t k = 0; k < 16 * n; ++k) if (!std::isfinite(Tow16s[k])) {
        set_error("scene window: Tow16s of object %zu is not finite", k / 16); return MON_ERR_ARG; }
    return MON_OK;
}
int scene_window(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, const float* Tow16s,
                 const mon_pose_refine_params& p, const mon_window_params* wp, int iters, uint32_t iteration, const float* level_w, float* Twc16s_out,
                 float* Tow16s_out, float* loss_trace, float* frame_trace, float* loss, float* frame_loss, float* cam_grad6, float* obj_grad6) {
    { const int rc = scene_state_check("scene pose", ms, n, side); if (rc) return rc; }
    const int Lmax = scene_levels(ms, n).Lmax;
    // the frames in window order, each with the grids a single-frame call of its rays uses; the passes
    std::vector<SceneWinFrame> fr; std::vector<uint32_t> prefix; std::vector<uint32_t> pass0{ 0u };   // pass k holds frames [pass0[k], pass0[k + 1])
    uint32_t row_stride = 0, n_lp = 0, cap = 0, v_next = 0;
    for (size_t i0 = 0; i0 < n_obs; ) {
        size_t i1 = i0 + 1; while (i1 < n_obs && obs[i1].FrameId == obs[i0].FrameId) ++i1;
        SceneWinFrame f{}; f.pose = 16u * (uint32_t)fr.size(); f.box0 = (uint32_t)i0; f.n_box = (uint32_t)(i1 - i0); f.prefix0 = (uint32_t)prefix.size();
        f.total = append_prefix(prefix, obs + i0, i1 - i0); f.n_rays = p.rays_per_iter ? p.rays_per_iter : f.total; f.inv_n = 1.f / (float)f.n_rays;
        if (v_next + f.n_rays > kWindowPassRays) { pass0.push_back((uint32_t)fr.size()); v_next = 0; }
        f.v0 = v_next; v_next += f.n_rays; cap = std::max(cap, v_next);
        f.gridc = pose_grad_grid(f.n_rays); f.row0 = row_stride; row_stride += f.gridc;
        f.parts = scene_comp_grad_grid(f.n_rays); f.lp0 = n_lp; n_lp += f.parts;
        fr.push_back(f); i0 = i1;
    }
    pass0.push_back((uint32_t)fr.size());
    const uint32_t F = (uint32_t)fr.size(), n_pass = (uint32_t)pass0.size() - 1u;
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const int n_eval = iters < 0 ? 1 : iters + 1;
    ScenePoseWs& w = side_ws<ScenePoseWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, w.mu, w.ev); if (rc) return rc; }
    const std::vector<const uint16_t*>& prm = sd.prm; const hipStream_t s = sd.s;
    const uint32_t out_stride = 1u + 7u * F + 6u * (uint32_t)n;
    constexpr size_t kObjFloats = sizeof(SceneObjConst) / 4;
    const size_t out_floats = (size_t)out_stride * n_eval + 16 * (size_t)F + kObjFloats * n;      // the evaluations | every Twc | every SceneObjConst
    int rc;
    if ((rc = scene_pose_backward_bufs(w, n, cap, row_stride)) || (rc = w.poses.grow((size_t)F * 16)) || (rc = w.wframes.grow((size_t)F)) ||
        (rc = w.wmom.grow(12 * ((size_t)F + n))) || (rc = w.out.grow(out_floats)) || (rc = w.h_out.grow(out_floats))) return rc;
    const int n_wrows = level_w ? (iters < 0 ? 1 : iters) : 0;
    std::vector<size_t> frag_off;
    if ((rc = scene_pose_prologue(w, s, ms, n, Tow16s, obs, n_obs, prefix, cap, n_lp, level_w, n_wrows, Lmax, frag_off))) return rc;
    HIPCHECK(hipMemcpyAsync(w.poses.p, Twc16s, 64 * (size_t)F, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(w.wframes.p, fr.data(), sizeof(SceneWinFrame) * F, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(w.wmom.p, 0, 48 * ((size_t)F + n), s));
    std::vector<ScenePoseObjArgs> oa(n);
    for (int it = 0; it < n_eval; ++it) {
        const uint32_t key = iters < 0 ? iteration : (uint32_t)it;
        const float* lw_row = it < n_wrows ? w.lw.p + (size_t)it * Lmax : nullptr;
        for (uint32_t k = 0; k < n_pass; ++k) {
            const uint32_t f0 = pass0[k], nf = pass0[k + 1] - f0, nv = fr[f0 + nf - 1].v0 + fr[f0 + nf - 1].n_rays;
            uint32_t gmax = 0, pmax = 0; for (uint32_t f = f0; f < f0 + nf; ++f) { gmax = std::max(gmax, fr[f].gridc); pmax = std::max(pmax, fr[f].parts); }
            SceneWindowRayArgs ra{}; scene_ray_args(ra, w, ms, n, cap, p, key);
            ra.n_rays = nv; ra.pose = w.poses.p; ra.frames = w.wframes.p + f0; ra.n_frames = nf;
            launch_scene_window_rays(s, ra);
            for (size_t j = 0; j < n; ++j) {
                Model& m = *ms[j];
                oa[j] = scene_obj_args(w, m, j, cap, nv, 0u, p, key, 0.f);
                scene_obj_backward_args(oa[j], w, j, cap, w.partials.p + (size_t)j * row_stride * 8, lw_row);
                launch_scene_pose_obj(s, m.lf, m.nd, m.oc, prm[j], w.frag.p + frag_off[j], it == 0 && k == 0, 0, pose_grad_grid(nv), oa[j]);
            }
            SceneCompGradArgs ca = scene_comp_args(w, n, cap, nv, p); ca.gw = w.gw.p; ca.grow = w.grow.p; ca.loss_part = w.loss_part.p;
            launch_scene_window_composite(s, ca, pmax, nf, w.wframes.p + f0);
            for (size_t j = 0; j < n; ++j) { Model& m = *ms[j];
                launch_scene_window_obj(s, m.lf, m.nd, m.oc, prm[j], w.frag.p + frag_off[j], gmax, nf, w.wframes.p + f0, oa[j]); }
        }
        SceneWindowUpdateArgs ua{}; ua.partials = w.partials.p; ua.n_objs = (uint32_t)n; ua.row_stride = row_stride; ua.loss_part = w.loss_part.p;
        ua.frames = w.wframes.p; ua.n_frames = F; ua.n_fixed = wp ? wp->n_fixed_frames : F; ua.refine_objs = wp ? wp->refine_objects : 0; ua.objs = w.objs.p;
        ua.poses = w.poses.p; ua.moments = w.wmom.p; ua.out = w.out.p; ua.out_stride = out_stride; ua.it = (uint32_t)it; ua.step = iters >= 0 && it < iters;
        ua.lr_t = p.lr_trans; ua.lr_r = p.lr_rot; ua.lr_obj_t = wp ? wp->lr_obj_trans : 0.f; ua.lr_obj_r = wp ? wp->lr_obj_rot : 0.f;
        launch_scene_window_update(s, ua);
    }
    HIPCHECK(hipGetLastError());
    // results home through the pinned staging: every evaluation's row, then the poses, then the objects' constants (their Tow)
    float* d_tail = w.out.p + (size_t)out_stride * n_eval;
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(w.poses.p), reinterpret_cast<uint16_t*>(d_tail), 32u * F);
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(w.objs.p), reinterpret_cast<uint16_t*>(d_tail + 16 * (size_t)F), (uint32_t)(2 * kObjFloats * n));
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(w.out.p), reinterpret_cast<uint16_t*>(w.h_out.p), (uint32_t)(out_floats * 2));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    const float* h = w.h_out.p;
    if (loss) *loss = h[0];
    if (frame_loss) std::memcpy(frame_loss, h + 1, 4 * (size_t)F);
    if (cam_grad6) std::memcpy(cam_grad6, h + 1 + F, 24 * (size_t)F);
    if (obj_grad6) std::memcpy(obj_grad6, h + 1 + 7 * (size_t)F, 24 * n);
    for (int it = 0; it < n_eval; ++it) {
        const float* r = h + (size_t)out_stride * it;
        if (loss_trace) loss_trace[it] = r[0];
        if (frame_trace) std::memcpy(frame_trace + (size_t)F * it, r + 1, 4 * (size_t)F);
    }
    const float* tail = h + (size_t)out_stride * n_eval;
    if (Twc16s_out) for (uint32_t f = wp ? std::min(wp->n_fixed_frames, F) : F; f < F; ++f) std::memcpy(Twc16s_out + 16 * (size_t)f, tail + 16 * (size_t)f, 64);
    if (Tow16s_out && wp && wp->refine_objects) for (size_t j = 0; j < n; ++j) std::memcpy(Tow16s_out + 16 * j, tail + 16 * (size_t)F + kObjFloats * j, 64);
    return MON_OK;
}

// ---- wide-basin relocalisation (mon_scene_relocalise / mon_online_relocalise): score every candidate, refine the best few with scene_pose, score the
// refined poses and their starts together, return the winner.  2 + min(keep, n_cands) stream synchronisations: one per scoring round, one per refinement.
int scene_reloc_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* cands, size_t n_cands, const mon_pose_refine_params* p,
                      const mon_reloc_params* r, const float* pose_out) {
    REQUIRE_ARG("relocalise", cands, "candidates"); REQUIRE_ARG("relocalise", p, "params"); REQUIRE_ARG("relocalise", r, "reloc params");
    REQUIRE_ARG("relocalise", pose_out, "Twc16_out");
    if (n_cands == 0 || n_cands > kSceneScoreMaxPoses) { set_error("relocalise: %zu candidates (1 to %u)", n_cands, kSceneScoreMaxPoses); return MON_ERR_ARG; }
    if (r->score_rays == 0 || r->score_rays > kSceneScoreMaxRays) { set_error("relocalise: score_rays %u (1 to %u)", r->score_rays, kSceneScoreMaxRays);
        return MON_ERR_ARG; }
    if (r->keep == 0 || r->keep > kRelocMaxKeep) { set_error("relocalise: keep %u (1 to %u)", r->keep, kRelocMaxKeep); return MON_ERR_ARG; }
    return scene_pose_check(side, obs, n_obs, cands, p);
}
int scene_relocalise(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* cands, size_t n_cands,
                     const mon_pose_refine_params& p, const float* level_w, const mon_reloc_params& r, float* pose_out, mon_reloc_result* result,
                     float* scores) {
    mon_pose_refine_params ps = p; ps.rays_per_iter = r.score_rays;
    // 1. every candidate's score
    std::vector<float> S(n_cands);
    int rc = scene_pose_batch(ms, n, side, obs, n_obs, cands, n_cands, ps, r.score_iteration, S.data()); if (rc) return rc;
    if (scores) std::memcpy(scores, S.data(), n_cands * 4);
    // 2. the kept set: candidate 0, then the others by ascending score (ties to the lower index, a non-finite score last)
    std::vector<uint32_t> order; for (uint32_t i = 1; i < n_cands; ++i) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const bool fa = std::isfinite(S[a]), fb = std::isfinite(S[b]);
        return fa != fb ? fa : (fa && S[a] < S[b]); });
    const size_t k = std::min<size_t>(r.keep, n_cands);
    std::vector<uint32_t> kept{ 0u }; kept.insert(kept.end(), order.begin(), order.begin() + (ptrdiff_t)(k - 1));
    // 3. each of them refined as mon_scene_refine_camera refines it (level_w: its schedule's table, or nullptr)
    std::vector<float> list(2 * k * 16);
    for (size_t i = 0; i < k; ++i) {
        const float* start = cands + 16 * (size_t)kept[i]; float* pose = list.data() + 16 * i;
        std::memcpy(list.data() + 16 * (k + i), start, 64); std::memcpy(pose, start, 64);
        rc = scene_pose(ms, n, side, obs, n_obs, pose, p, p.iters, 0u, pose, nullptr, nullptr, nullptr, nullptr, level_w);
        if (rc) return rc;
    }
    // 4. the refined poses and their starts under the common key; the lowest finite score wins (ties to the earlier entry)
    std::vector<float> F(2 * k);
    rc = scene_pose_batch(ms, n, side, obs, n_obs, list.data(), 2 * k, ps, r.score_iteration, F.data()); if (rc) return rc;
    size_t win = 2 * k;
    for (size_t i = 0; i < 2 * k; ++i) if (std::isfinite(F[i]) && (win == 2 * k || F[i] < F[win])) win = i;
    const bool none = win == 2 * k; if (none) win = k;                          // no finite score: candidate 0 as given
    std::memcpy(pose_out, list.data() + 16 * win, 64);
    if (result) {
        result->best_candidate = kept[win % k]; result->refined = (!none && win < k) ? 1u : 0u;
        result->score_candidate0 = S[0]; result->score_best_candidate = S[kept[win % k]]; result->score_final = F[win];
    }
    return MON_OK;
}

}  // namespace mon
