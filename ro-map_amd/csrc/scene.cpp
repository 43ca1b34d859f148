// scene.cpp -- several object NeRFs under one camera: the boundary every entry to a scene route passes (its checks, handles to models; model.h), the entry
// to a side and the call over its workspace that every route runs (model_internal.h), the scene render, the probe and the ray cast over one list chain.
// The field queries: scene_field.cpp; the scene pose family: scene_pose.cpp
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include "model_internal.h"

namespace mon {
// ---- the boundary of the scene routes.  Every entry to a route -- the C ABI, the online manager, a dump entry of the diagnostics library --
// runs the same four steps: the route's *_check (what can be judged without an object), the objects (scene_models from handles, the manager's own pick), the
// route's *_objects_check (what needs them), the route itself.  A schedule's pose_c2f_check is a call of its own.  None of them does device work; the routes
// below repeat none of them.  `what`: the message prefix ("scene_render", "scene pose").
static int scene_count_check(const char* what, size_t n) {
    if (n == 0 || n > kSceneMaxLists) { set_error("%s: %zu objects (1 to %u)", what, n, kSceneMaxLists); return MON_ERR_ARG; }
    return MON_OK;
}
int scene_models(const char* what, mon_object* const* objs, size_t n, std::vector<Model*>& ms) {
    if (!objs) { set_error("%s: null objs", what); return MON_ERR_ARG; }
    { const int rc = scene_count_check(what, n); if (rc) return rc; }
    ms.resize(n);
    for (size_t j = 0; j < n; ++j) { if (!objs[j] || !objs[j]->m) { set_error("%s: null object %zu", what, j); return MON_ERR_ARG; } ms[j] = objs[j]->m; }
    return MON_OK;
}
// the objects of one call: 1 to kSceneMaxLists of them on one device, looking through one camera (every call but the ray cast, which has no camera) and,
// where the call reads a frame's pixels, of one dataset
int scene_objects_check(const char* what, Model* const* ms, size_t n, bool camera, bool one_dataset) {
    { const int rc = scene_count_check(what, n); if (rc) return rc; }
    const Model& m0 = *ms[0]; const Intrinsics& K = m0.ds->K;
    for (size_t j = 1; j < n; ++j) {
        const Model& m = *ms[j]; const Intrinsics& k = m.ds->K;
        if (m.device != m0.device) { set_error("%s: objects on logical devices %d and %d", what, m0.device, m.device); return MON_ERR_ARG; }
        if (camera && (k.fx != K.fx || k.fy != K.fy || k.cx != K.cx || k.cy != K.cy || k.W != K.W || k.H != K.H)) {
            set_error("%s: object %zu has other intrinsics", what, j); return MON_ERR_ARG; }
        if (one_dataset && m.ds != m0.ds) { set_error("%s: object %zu is on another dataset", what, j); return MON_ERR_ARG; }
    }
    return MON_OK;
}
SceneLevels scene_levels(Model* const* ms, size_t n, const mon_pose_c2f_params* c, int iters) {
    SceneLevels lv;
    for (size_t j = 0; j < n; ++j) lv.Lmax = std::max(lv.Lmax, (int)ms[j]->nd.L);
    if (c) lv.table = pose_c2f_table(*c, lv.Lmax, iters);
    return lv;
}
int scene_state_check(const char* what, Model* const* ms, size_t n, int side, bool lists) {
    for (size_t j = 0; j < n; ++j) {
        Model& m = *ms[j];
        if (!rskip_supported(m) || (lists && 2u * m.oc.S != kSceneListLen)) { set_error("%s: object %zu does not run on the fused kernels", what, j); return MON_ERR_STATE; }
        if (lists && m.d_xw) { set_error("%s: object %zu renders with the XORWOW sample stream (rng_flags)", what, j); return MON_ERR_STATE; }
        if (side == 1 && !model_has_snapshot(m)) { set_error("%s: object %zu has no published snapshot", what, j); return MON_ERR_STATE; }
    }
    return MON_OK;
}
int side_check(const char* what, int side) {
    if (side != 0 && side != 1) { set_error("%s: side %d (0 or 1)", what, side); return MON_ERR_ARG; }
    return MON_OK;
}

// ---- entering a side of a scene (SceneSide, model_internal.h)
int SceneSide::enter(Model* const* ms, size_t n, int side, std::mutex& ws_mu, std::vector<hipEvent_t>& ev) {
    prm.assign(n, nullptr); epoch.assign(n, 0);
    if (side == 1) {
        InferShared* sh = ms[0]->infer->shared; dev_lock = std::unique_lock<std::mutex>(sh->mu); s = sh->stream;
        pins = std::vector<SnapshotPin>(n);
        for (size_t j = 0; j < n; ++j) {
            const int rc = pins[j].take(ms[j]->infer, s); if (rc) return rc;
            prm[j] = pins[j].snap(); epoch[j] = pins[j].epoch;
        }
    }
    ws_lock = std::unique_lock<std::mutex>(ws_mu);
    if (side == 0) {
        for (size_t j = 0; j < n; ++j) { Model& m = *ms[j]; model_leave_lane(m); int rc = ensure_ema_current(m); if (rc) return rc; }
        s = ms[0]->train_stream;
        while (ev.size() < n) { hipEvent_t e; HIPCHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); ev.push_back(e); }
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j];
            if (m.train_stream != s) { HIPCHECK(hipEventRecord(ev[j], m.train_stream)); HIPCHECK(hipStreamWaitEvent(s, ev[j], 0)); }
            prm[j] = (m.h_state.step > 0) ? m.P.ema : m.P.half; epoch[j] = m.weights_epoch;
        }
    }
    return MON_OK;
}

// ---- one call of a route over SceneWs (SceneCall, model_internal.h): the render, the probe and the cast below, the field queries of scene_field.cpp
int SceneCall::enter(const char* what, Model* const* ms, size_t n, int side, bool lists) {
    { const int rc = scene_state_check(what, ms, n, side, lists); if (rc) return rc; }
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    ws = &side_ws<SceneWs>(device, side);
    { const int rc = sd.enter(ms, n, side, ws->mu, ws->ev); if (rc) return rc; }
    s = sd.s;
    src.resize(n);
    for (size_t j = 0; j < n; ++j) {
        Model& m = *ms[j]; RenderSkipSide& rs = side == 1 ? m.infer->rskip : m.rskip;
        src[j].b = side == 1 ? &m.infer->rb : &m.B; src[j].frag = side == 1 ? m.infer->frag : m.d_frag_render;
        src[j].bits = lists && m.rskip_on.load() != 0 ? rskip_grid(m, rs, s, m.rskip_alpha.load(), sd.prm[j], sd.epoch[j], src[j].frag) : nullptr;
    }
    return MON_OK;
}
// (grow-only; nothing of the workspace is in flight: every user synchronised before unlocking)
int SceneCall::grow_lists(size_t n, uint32_t cap) {
    const size_t need = n * (size_t)cap; int rc;
    if ((rc = ws->t.grow(need * kSceneListLen)) || (rc = ws->attr.grow(need * kSceneListLen * 4)) || (rc = ws->cnt.grow(need))) return rc;
    return MON_OK;
}
int SceneCall::finish() {
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    return MON_OK;
}
int SceneCall::home(size_t floats) {
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws->out.p), reinterpret_cast<uint16_t*>(ws->h_out.p), (uint32_t)(2 * floats));
    return finish();
}

// ---- scene render (mon_scene_render): every object's sample lists of a chunk of the rect (k_fused_render<EMIT>), then one merge-composite launch
int scene_render_check(int side, mon_frame_bbox rect, const float* Twc16) {
    REQUIRE_ARG("scene_render", Twc16, "Twc16");
    if (rect.w == 0 || rect.h == 0) { set_error("scene_render: empty rect"); return MON_ERR_ARG; }
    return side_check("scene_render", side);
}
int scene_render_outputs_check(const float* rgb, const float* depth) {
    REQUIRE_ARG("scene_render", rgb, "rgb"); REQUIRE_ARG("scene_render", depth, "depth");
    return MON_OK;
}
int scene_render(Model* const* ms, size_t n, int side, mon_frame_bbox rect, const float* Twc16, float* rgb, float* depth, float* opacity, int32_t* instance,
                 const int32_t* ids, const SceneDump* dump) {
    SceneCall c; { const int rc = c.enter("scene_render", ms, n, side, true); if (rc) return rc; }
    const Intrinsics K = ms[0]->ds->K;
    const uint32_t n_pix = rect.w * rect.h, cap = std::min(n_pix, kRenderChunkRays), L = (uint32_t)n;
    Mat4 pose; std::memcpy(pose.m, Twc16, 64);
    SceneWs& ws = *c.ws; const SceneSide& sd = c.sd; const std::vector<SceneSrc>& src = c.src; const hipStream_t s = c.s;
    { int rc; if ((rc = c.grow_lists(n, cap)) || (rc = ws.out.grow(6 * (size_t)n_pix)) || (rc = ws.h_out.grow(6 * (size_t)n_pix))) return rc; }
    float* o_rgb = ws.out.p; float* o_depth = ws.out.p + 3 * (size_t)n_pix; float* o_op = ws.out.p + 4 * (size_t)n_pix;
    int32_t* o_inst = reinterpret_cast<int32_t*>(ws.out.p + 5 * (size_t)n_pix);
    std::vector<float> d_t, d_attr; std::vector<uint32_t> d_cnt;         // mon_debug_scene_samples: one list of the whole rect
    if (dump) { d_t.resize((size_t)n_pix * kSceneListLen); d_attr.resize((size_t)n_pix * kSceneListLen * 4); d_cnt.resize(n_pix); }
    for (uint32_t p0 = 0; p0 < n_pix; p0 += cap) {
        const uint32_t nc = std::min(cap, n_pix - p0);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j]; const size_t l0 = j * (size_t)cap;
            launch_render_rays(s, *src[j].b, K, m.oc, rect, pose, 0, p0, nc);
            launch_fused_render_emit(s, m.lf, m.nd, sd.prm[j], *src[j].b, m.oc, nc, p0 * kSceneListLen, ws.t.p + l0 * kSceneListLen, ws.attr.p + l0 * kSceneListLen * 4,
                    ws.cnt.p + l0, src[j].frag, p0 == 0u, src[j].bits);
        }
        // (every object's ray kernel wrote the same dn: it depends on the pixel and the intrinsics only)
        launch_scene_composite(s, nc, L, cap, ws.t.p, ws.attr.p, ws.cnt.p, src[0].b->ray_dn, o_rgb + 3 * (size_t)p0, o_depth + p0, o_op + p0, o_inst + p0);
        if (dump) {
            const size_t l0 = dump->list * (size_t)cap;
            HIPCHECK(hipMemcpyAsync(d_t.data() + (size_t)p0 * kSceneListLen, ws.t.p + l0 * kSceneListLen, (size_t)nc * kSceneListLen * 4, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_attr.data() + (size_t)p0 * kSceneListLen * 4, ws.attr.p + l0 * kSceneListLen * 4, (size_t)nc * kSceneListLen * 16,
                    hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_cnt.data() + p0, ws.cnt.p + l0, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
        }
    }
    { const int rc = c.home(6 * (size_t)n_pix); if (rc) return rc; }
    std::memcpy(rgb, ws.h_out.p, 12 * (size_t)n_pix); std::memcpy(depth, ws.h_out.p + 3 * (size_t)n_pix, 4 * (size_t)n_pix);
    if (opacity) std::memcpy(opacity, ws.h_out.p + 4 * (size_t)n_pix, 4 * (size_t)n_pix);
    if (instance) {
        const int32_t* q = reinterpret_cast<const int32_t*>(ws.h_out.p + 5 * (size_t)n_pix);
        for (uint32_t i = 0; i < n_pix; ++i) instance[i] = (q[i] >= 0 && ids) ? ids[q[i]] : q[i];
    }
    if (dump) {
        for (size_t i = 0; i < (size_t)n_pix * kSceneListLen; ++i) {
            if (dump->t) dump->t[i] = d_t[i];
            if (dump->alpha) dump->alpha[i] = d_attr[4 * i];
            if (dump->rgb) for (int c = 0; c < 3; ++c) dump->rgb[3 * i + c] = d_attr[4 * i + 1 + c];
        }
        if (dump->count) std::memcpy(dump->count, d_cnt.data(), 4 * (size_t)n_pix);
    }
    return MON_OK;
}

// ---- the chain scene_probe and scene_cast share: a list of n_items rays of some kind against the objects, in passes of at most kRenderChunkRays in the
// render's list workspace.  Per pass and object `rays` (the call's ray kernel: object j's ray rows of items [p0, p0 + nc), for j == 0 also the keys into
// ws.keys) + the keyed emit, then `composite` (the call's composite of the pass, outputs at ws.out + the item's place in `rows` rows of n_items floats).
// `upload` grows and fills what the call keeps in the workspace beside the lists.  Everything is enqueued at once; the output rows go home through the pinned
// staging with one synchronisation, and `home` unpacks them while the workspace is still locked.  dump: object k's ray rows of every pass (and its entry row).
struct SceneListCall {
    const char* what; Model* const* ms; size_t n; int side; size_t n_items; uint32_t rows;
    std::function<int(SceneWs&, hipStream_t, uint32_t cap)> upload;
    std::function<void(SceneWs&, hipStream_t, const SceneSrc&, Model&, size_t j, uint32_t p0, uint32_t nc, uint32_t cap)> rays;
    std::function<void(SceneWs&, hipStream_t, uint32_t L, uint32_t cap, const float* dn, uint32_t p0, uint32_t nc)> composite;
    std::function<void(const float* h)> home;
    const SceneRaysDump* dump;
};
static int scene_list_run(const SceneListCall& c) {
    Model* const* ms = c.ms; const size_t n = c.n, n_q = c.n_items; const int side = c.side; const SceneRaysDump* dump = c.dump;
    SceneCall call; { const int rc = call.enter(c.what, ms, n, side, true); if (rc) return rc; }
    const uint32_t nq = (uint32_t)n_q, cap = std::min(nq, kRenderChunkRays), L = (uint32_t)n;
    SceneWs& ws = *call.ws; const SceneSide& sd = call.sd; const std::vector<SceneSrc>& src = call.src; const hipStream_t s = call.s;
    {   int rc;
        if ((rc = call.grow_lists(n, cap)) || (rc = ws.out.grow(c.rows * n_q)) || (rc = ws.h_out.grow(c.rows * n_q)) || (rc = ws.keys.grow(cap)) ||
            (rc = c.upload(ws, s, cap))) return rc; }
    std::vector<float> d_o, d_d, d_t0, d_t1, d_dn; std::vector<uint8_t> d_flag;       // the dump: object k's ray rows of every pass
    if (dump) { d_o.resize(3 * n_q); d_d.resize(3 * n_q); d_t0.resize(n_q); d_t1.resize(n_q); d_dn.resize(n_q); d_flag.resize(n_q); }
    for (uint32_t p0 = 0; p0 < nq; p0 += cap) {
        const uint32_t nc = std::min(cap, nq - p0);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j]; const size_t l0 = j * (size_t)cap;
            c.rays(ws, s, src[j], m, j, p0, nc, cap);
            launch_fused_render_emit(s, m.lf, m.nd, sd.prm[j], *src[j].b, m.oc, nc, 0u, ws.t.p + l0 * kSceneListLen, ws.attr.p + l0 * kSceneListLen * 4,
                    ws.cnt.p + l0, src[j].frag, p0 == 0u, src[j].bits, ws.keys.p);
        }
        // (every object's ray kernel wrote the same dn: it depends on the item alone)
        c.composite(ws, s, L, cap, src[0].b->ray_dn, p0, nc);
        if (dump) {
            const BatchPtrs& b = *src[dump->k].b;
            HIPCHECK(hipMemcpyAsync(d_o.data() + 3 * (size_t)p0, b.ray_o, 12 * (size_t)nc, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_d.data() + 3 * (size_t)p0, b.ray_d, 12 * (size_t)nc, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_t0.data() + p0, b.ray_t0, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_t1.data() + p0, b.ray_t1, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_dn.data() + p0, b.ray_dn, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(d_flag.data() + p0, b.ray_flag, (size_t)nc, hipMemcpyDeviceToHost, s));
            if (dump->entry) HIPCHECK(hipMemcpyAsync(dump->entry + p0, ws.entry.p + dump->k * (size_t)cap, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
        }
    }
    { const int rc = call.home(c.rows * n_q); if (rc) return rc; }
    c.home(ws.h_out.p);
    if (dump) for (size_t i = 0; i < n_q; ++i) {                                        // (a row that missed the box holds only flag and dn)
        float* r = dump->rows + 10 * i; const bool hit = d_flag[i] != 0;
        for (int a = 0; a < 3; ++a) { r[a] = hit ? d_o[3 * i + a] : 0.f; r[3 + a] = hit ? d_d[3 * i + a] : 0.f; }
        r[6] = hit ? d_t0[i] : 0.f; r[7] = hit ? d_t1[i] : 0.f; r[8] = hit ? 1.f : 0.f; r[9] = d_dn[i];
    }
    return MON_OK;
}
// an instance row home: the call's list indices, or the caller's ids for them
void scene_instances_home(int32_t* out, const float* row, size_t n, const int32_t* ids) {
    const int32_t* q = reinterpret_cast<const int32_t*>(row);
    if (out) for (size_t i = 0; i < n; ++i) out[i] = (q[i] >= 0 && ids) ? ids[q[i]] : q[i];
}

// ---- scene probe (mon_scene_probe): the chain over a list of sub-pixel queries under several poses: k_scene_probe_rays, k_scene_probe_composite; eight
// output rows (rgb 3n | depth | opacity | instance | hit_depth | hit_instance).
int scene_probe_check(int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q, const float* rgb, const float* depth) {
    if (!Twc16s || !q || !rgb || !depth) { set_error("scene_probe: null argument"); return MON_ERR_ARG; }
    { const int rc = side_check("scene_probe", side); if (rc) return rc; }
    if (n_poses == 0 || n_poses > kSceneProbeMaxPoses) { set_error("scene_probe: %zu poses (1 to %u)", n_poses, kSceneProbeMaxPoses); return MON_ERR_ARG; }
    if (n_q == 0 || n_q > kSceneProbeMaxQueries) { set_error("scene_probe: %zu queries (1 to %u)", n_q, kSceneProbeMaxQueries); return MON_ERR_ARG; }
    for (size_t k = 0; k < 16 * n_poses; ++k) if (!std::isfinite(Twc16s[k])) { set_error("scene_probe: pose %zu is not finite", k / 16); return MON_ERR_ARG; }
    for (size_t i = 0; i < n_q; ++i) {
        if (q[i].pose >= n_poses) { set_error("scene_probe: query %zu names pose %u of %zu", i, q[i].pose, n_poses); return MON_ERR_ARG; }
        if (q[i].key >= kSceneProbeMaxKey) { set_error("scene_probe: query %zu has key %u (below %u)", i, q[i].key, kSceneProbeMaxKey); return MON_ERR_ARG; }
        if (!std::isfinite(q[i].u) || !std::isfinite(q[i].v)) { set_error("scene_probe: query %zu is not finite", i); return MON_ERR_ARG; }
    }
    return MON_OK;
}
int scene_probe(Model* const* ms, size_t n, int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q, float* rgb, float* depth,
                float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance, const int32_t* ids, const SceneRaysDump* dump) {
    SceneListCall c{ "scene_probe", ms, n, side, n_q, 8u, {}, {}, {}, {}, dump };
    c.upload = [&](SceneWs& ws, hipStream_t s, uint32_t) -> int {
        int rc; if ((rc = ws.q.grow(n_q)) || (rc = ws.poses.grow(16 * n_poses))) return rc;
        HIPCHECK(hipMemcpyAsync(ws.q.p, q, sizeof(mon_scene_query) * n_q, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(ws.poses.p, Twc16s, 64 * n_poses, hipMemcpyHostToDevice, s));
        return MON_OK;
    };
    c.rays = [&](SceneWs& ws, hipStream_t s, const SceneSrc& src, Model& m, size_t j, uint32_t p0, uint32_t nc, uint32_t) {
        launch_scene_probe_rays(s, *src.b, ms[0]->ds->K, m.oc, ws.q.p + p0, ws.poses.p, j == 0 ? ws.keys.p : nullptr, nc);
    };
    c.composite = [&](SceneWs& ws, hipStream_t s, uint32_t L, uint32_t cap, const float* dn, uint32_t p0, uint32_t nc) {
        float* o = ws.out.p;
        launch_scene_probe_composite(s, nc, L, cap, ws.t.p, ws.attr.p, ws.cnt.p, dn, o + 3 * (size_t)p0, o + 3 * n_q + p0, o + 4 * n_q + p0,
                reinterpret_cast<int32_t*>(o + 5 * n_q) + p0, o + 6 * n_q + p0, reinterpret_cast<int32_t*>(o + 7 * n_q) + p0);
    };
    c.home = [&](const float* h) {
        std::memcpy(rgb, h, 12 * n_q); std::memcpy(depth, h + 3 * n_q, 4 * n_q);
        if (opacity) std::memcpy(opacity, h + 4 * n_q, 4 * n_q);
        if (hit_depth) std::memcpy(hit_depth, h + 6 * n_q, 4 * n_q);
        scene_instances_home(instance, h + 5 * n_q, n_q, ids); scene_instances_home(hit_instance, h + 7 * n_q, n_q, ids);
    };
    return scene_list_run(c);
}

// ---- ray cast (mon_scene_cast): the chain over a list of world rays: k_scene_cast_rays, k_scene_cast_composite; nine output rows (rgb 3n | dist | opacity
// | instance | hit_t | hit_sample_t | hit_instance).  No camera: the objects need only share a device.
int scene_cast_check(int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* rgb, const float* dist) {
    if (!rays || !rgb || !dist) { set_error("scene_cast: null argument"); return MON_ERR_ARG; }
    { const int rc = side_check("scene_cast", side); if (rc) return rc; }
    if (n_rays == 0 || n_rays > kSceneProbeMaxQueries) { set_error("scene_cast: %zu rays (1 to %u)", n_rays, kSceneProbeMaxQueries); return MON_ERR_ARG; }
    if (!(hit_opacity > 0.f && hit_opacity <= 0.999f)) { set_error("scene_cast: hit_opacity %g (above 0, at most 0.999)", (double)hit_opacity); return MON_ERR_ARG; }
    for (size_t i = 0; i < n_rays; ++i) {
        const mon_scene_ray& r = rays[i];
        if (r.key >= kSceneProbeMaxKey) { set_error("scene_cast: ray %zu has key %u (below %u)", i, r.key, kSceneProbeMaxKey); return MON_ERR_ARG; }
        float nn = 0.f;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(r.o[a]) || !std::isfinite(r.d[a])) { set_error("scene_cast: ray %zu is not finite", i); return MON_ERR_ARG; }
            nn += r.d[a] * r.d[a];
        }
        if (!(std::fabs(nn - 1.f) <= 1e-3f)) { set_error("scene_cast: the direction of ray %zu is not unit (|d|^2 = %g)", i, (double)nn); return MON_ERR_ARG; }
        if (!(r.t_max > 0.f)) { set_error("scene_cast: ray %zu has t_max %g (above 0)", i, (double)r.t_max); return MON_ERR_ARG; }
    }
    return MON_OK;
}
int scene_cast(Model* const* ms, size_t n, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, float* rgb, float* dist, float* opacity,
               int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance, const int32_t* ids, const SceneRaysDump* dump) {
    const size_t n_q = n_rays;
    SceneListCall c{ "scene_cast", ms, n, side, n_q, 9u, {}, {}, {}, {}, dump };
    c.upload = [&](SceneWs& ws, hipStream_t s, uint32_t cap) -> int {
        int rc; if ((rc = ws.rays.grow(n_q)) || (rc = ws.entry.grow(n * (size_t)cap))) return rc;
        HIPCHECK(hipMemcpyAsync(ws.rays.p, rays, sizeof(mon_scene_ray) * n_q, hipMemcpyHostToDevice, s));
        return MON_OK;
    };
    c.rays = [&](SceneWs& ws, hipStream_t s, const SceneSrc& src, Model& m, size_t j, uint32_t p0, uint32_t nc, uint32_t cap) {
        launch_scene_cast_rays(s, *src.b, m.oc, ws.rays.p + p0, j == 0 ? ws.keys.p : nullptr, ws.entry.p + j * (size_t)cap, nc);
    };
    c.composite = [&](SceneWs& ws, hipStream_t s, uint32_t L, uint32_t cap, const float*, uint32_t p0, uint32_t nc) {
        float* o = ws.out.p;
        launch_scene_cast_composite(s, nc, L, cap, hit_opacity, ws.t.p, ws.attr.p, ws.cnt.p, ws.entry.p, o + 3 * (size_t)p0, o + 3 * n_q + p0, o + 4 * n_q + p0,
                reinterpret_cast<int32_t*>(o + 5 * n_q) + p0, o + 6 * n_q + p0, o + 7 * n_q + p0, reinterpret_cast<int32_t*>(o + 8 * n_q) + p0);
    };
    c.home = [&](const float* h) {
        std::memcpy(rgb, h, 12 * n_q); std::memcpy(dist, h + 3 * n_q, 4 * n_q);
        if (opacity) std::memcpy(opacity, h + 4 * n_q, 4 * n_q);
        if (hit_t) std::memcpy(hit_t, h + 6 * n_q, 4 * n_q);
        if (hit_sample_t) std::memcpy(hit_sample_t, h + 7 * n_q, 4 * n_q);
        scene_instances_home(instance, h + 5 * n_q, n_q, ids); scene_instances_home(hit_instance, h + 8 * n_q, n_q, ids);
    };
    return scene_list_run(c);
}
// mon_camera_rays: pixel_ray's world-frame branch (pose_is_Toc: the pose alone, no object) on the host -- the operations k_scene_probe_rays runs before it
// applies an object's Tow, which k_scene_cast_rays applies to these rays in the same way
int scene_camera_rays(float fx, float fy, float cx, float cy, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                      mon_scene_ray* rays_out, float* dn_out) {
    if (!Twc16s || !q || !rays_out) { set_error("camera_rays: null argument"); return MON_ERR_ARG; }
    if (n_poses == 0 || n_q == 0) { set_error("camera_rays: no poses or no queries"); return MON_ERR_ARG; }
    if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || fx == 0.f || fy == 0.f) {
        set_error("camera_rays: intrinsics not finite or a zero focal length"); return MON_ERR_ARG; }
    for (size_t k = 0; k < 16 * n_poses; ++k) if (!std::isfinite(Twc16s[k])) { set_error("camera_rays: pose %zu is not finite", k / 16); return MON_ERR_ARG; }
    for (size_t i = 0; i < n_q; ++i) {
        if (q[i].pose >= n_poses) { set_error("camera_rays: query %zu names pose %u of %zu", i, q[i].pose, n_poses); return MON_ERR_ARG; }
        if (!std::isfinite(q[i].u) || !std::isfinite(q[i].v)) { set_error("camera_rays: query %zu is not finite", i); return MON_ERR_ARG; }
    }
    const Intrinsics K{ fx, fy, cx, cy, 0, 0 };
    for (size_t i = 0; i < n_q; ++i) {
        mon_scene_ray& r = rays_out[i]; float dn;
        pixel_ray(K, q[i].u, q[i].v, Twc16s + 16 * (size_t)q[i].pose, nullptr, true, r.o, r.d, dn);
        r.t_max = INFINITY; r.key = q[i].key;
        if (dn_out) dn_out[i] = dn;
    }
    return MON_OK;
}

}  // namespace mon
