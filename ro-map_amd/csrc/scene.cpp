// scene.cpp -- several object NeRFs under one camera: the boundary every entry to a scene route passes (its checks, handles to models; model.h), the scene
// render, the probe and the ray cast over one list chain, and the scene pose family (camera refinement, batched scoring, window, relocalisation)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
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
// every MON_ERR_STATE of a scene call that needs no device work (the routes run it themselves: it is their own question, asked once)
static int scene_state_check(const char* what, Model* const* ms, size_t n, int side) {
    for (size_t j = 0; j < n; ++j) {
        Model& m = *ms[j];
        if (!rskip_supported(m) || 2u * m.oc.S != kSceneListLen) { set_error("%s: object %zu does not run on the fused kernels", what, j); return MON_ERR_STATE; }
        if (m.d_xw) { set_error("%s: object %zu renders with the XORWOW sample stream (rng_flags)", what, j); return MON_ERR_STATE; }
        if (side == 1 && !model_has_snapshot(m)) { set_error("%s: object %zu has no published snapshot", what, j); return MON_ERR_STATE; }
    }
    return MON_OK;
}
static int side_check(const char* what, int side) {
    if (side != 0 && side != 1) { set_error("%s: side %d (0 or 1)", what, side); return MON_ERR_ARG; }
    return MON_OK;
}

// ---- entering a side of a scene: the weights every object is read from, their stamps, the stream of the call.  Side 1: the shared inference stream under
// its device lock, every object's snapshot pinned.  Side 0: the train side as model_render picks it (EMA once trained, brought up to date), object 0's train
// stream after every object's pending work (the workspace's events `ev`).  Lock order: the device's inference lock, then the workspace's `ws_mu`;
// InferState::mu only inside SnapshotPin::take.  Holds the locks and the pins until it goes (after the call's stream has been synchronised).
struct SceneSide {
    hipStream_t s = nullptr; std::vector<const uint16_t*> prm; std::vector<uint64_t> epoch;
    std::unique_lock<std::mutex> dev_lock; std::vector<SnapshotPin> pins; std::unique_lock<std::mutex> ws_lock;
    int enter(Model* const* ms, size_t n, int side, std::mutex& ws_mu, std::vector<hipEvent_t>& ev) {
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
};

// the workspace of type W of a device and side: made on first use, never freed
template <class W> static W& side_ws(int device, int side) {
    static std::mutex mu; static std::map<std::pair<int, int>, W*> all;
    std::lock_guard<std::mutex> l(mu); W*& w = all[{ device, side }]; if (!w) w = new W(); return *w;
}

// ---- scene render (mon_scene_render): every object's sample lists of a chunk of the rect (k_fused_render<EMIT>), then one merge-composite launch
// Per device and side, grow-only, never freed (like the tile workspaces): the lists of one chunk for every object, the rect's outputs, their pinned staging,
// the events that order the objects' streams in front of side 0's render.  A render holds `mu` until its stream has been synchronised.
struct SceneWs {
    std::mutex mu;
    DevBuf<float> t, attr; DevBuf<uint32_t> cnt;                                  // [lists][cap][kSceneListLen] t, float4 attr; [lists][cap]
    DevBuf<float> out; PinnedBuf<float> h_out;                                    // rgb 3n | depth n | opacity n | instance n (int32)
    DevBuf<mon_scene_query> q; DevBuf<float> poses; DevBuf<uint32_t> keys;        // scene_probe: the queries, the poses [n_poses][16], a pass's keys [cap]
    DevBuf<mon_scene_ray> rays; DevBuf<float> entry;                              // scene_cast: the rays, a pass's box entries [lists][cap]
    DevBuf<float> pts, rows;                                                      // scene_points: the points [n][3], a pass's rows [objects][cap][12]
    DevBuf<uint16_t> gfrag; DevBuf<float> lw; DevBuf<int32_t> sel;                // scene_gradients (rows of 16): full fragment images, weights [Lmax], select [n]
    DevBuf<uint8_t> docc; DevBuf<float> dv; DevBuf<int32_t> dsite;                // scene_distance: the mask [n], the passes' squared distances and sites [2][n]
    DevBuf<uint32_t> cscan;                                                       // scene_components: the numbering's block sums (its mask is docc)
    std::vector<hipEvent_t> ev;
};
// what each object renders with on a side; the render grids are the objects' own per-side caches, built if stale (their skip counters stay as they are).
// grids = false (the point queries, which consult no skipping): no grid is looked at or built, bits = nullptr
struct SceneSrc { BatchPtrs* b; uint16_t* frag; const uint32_t* bits; };
static std::vector<SceneSrc> scene_sources(Model* const* ms, size_t n, int side, const SceneSide& sd, bool grids = true) {
    std::vector<SceneSrc> src(n);
    for (size_t j = 0; j < n; ++j) {
        Model& m = *ms[j]; RenderSkipSide& rs = side == 1 ? m.infer->rskip : m.rskip;
        src[j].b = side == 1 ? &m.infer->rb : &m.B; src[j].frag = side == 1 ? m.infer->frag : m.d_frag_render;
        src[j].bits = grids && m.rskip_on.load() != 0 ? rskip_grid(m, rs, sd.s, m.rskip_alpha.load(), sd.prm[j], sd.epoch[j], src[j].frag) : nullptr;
    }
    return src;
}
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
    { const int rc = scene_state_check("scene_render", ms, n, side); if (rc) return rc; }
    const Intrinsics K = ms[0]->ds->K; const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const uint32_t n_pix = rect.w * rect.h, cap = std::min(n_pix, kRenderChunkRays), L = (uint32_t)n;
    Mat4 pose; std::memcpy(pose.m, Twc16, 64);
    SceneWs& ws = side_ws<SceneWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, ws.mu, ws.ev); if (rc) return rc; }
    const hipStream_t s = sd.s;
    const std::vector<SceneSrc> src = scene_sources(ms, n, side, sd);
    // workspace (grow-only; nothing of it is in flight: every user synchronised before unlocking)
    const size_t need_lists = (size_t)L * cap;
    {   int rc;
        if ((rc = ws.t.grow(need_lists * kSceneListLen)) || (rc = ws.attr.grow(need_lists * kSceneListLen * 4)) || (rc = ws.cnt.grow(need_lists)) ||
            (rc = ws.out.grow(6 * (size_t)n_pix)) || (rc = ws.h_out.grow(6 * (size_t)n_pix))) return rc; }
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
    // results home through the pinned staging (a copy kernel on the render's stream, as the snapshot render does)
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.out.p), reinterpret_cast<uint16_t*>(ws.h_out.p), (uint32_t)(12 * (size_t)n_pix));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
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
    { const int rc = scene_state_check(c.what, ms, n, side); if (rc) return rc; }
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const uint32_t nq = (uint32_t)n_q, cap = std::min(nq, kRenderChunkRays), L = (uint32_t)n;
    SceneWs& ws = side_ws<SceneWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, ws.mu, ws.ev); if (rc) return rc; }
    const hipStream_t s = sd.s;
    const std::vector<SceneSrc> src = scene_sources(ms, n, side, sd);
    const size_t need_lists = (size_t)L * cap;
    {   int rc;
        if ((rc = ws.t.grow(need_lists * kSceneListLen)) || (rc = ws.attr.grow(need_lists * kSceneListLen * 4)) || (rc = ws.cnt.grow(need_lists)) ||
            (rc = ws.out.grow(c.rows * n_q)) || (rc = ws.h_out.grow(c.rows * n_q)) || (rc = ws.keys.grow(cap)) || (rc = c.upload(ws, s, cap))) return rc; }
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
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.out.p), reinterpret_cast<uint16_t*>(ws.h_out.p), (uint32_t)(2 * c.rows * n_q));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    c.home(ws.h_out.p);
    if (dump) for (size_t i = 0; i < n_q; ++i) {                                        // (a row that missed the box holds only flag and dn)
        float* r = dump->rows + 10 * i; const bool hit = d_flag[i] != 0;
        for (int a = 0; a < 3; ++a) { r[a] = hit ? d_o[3 * i + a] : 0.f; r[3 + a] = hit ? d_d[3 * i + a] : 0.f; }
        r[6] = hit ? d_t0[i] : 0.f; r[7] = hit ? d_t1[i] : 0.f; r[8] = hit ? 1.f : 0.f; r[9] = d_dn[i];
    }
    return MON_OK;
}
// an instance row home: the call's list indices, or the caller's ids for them
static void scene_instances_home(int32_t* out, const float* row, size_t n, const int32_t* ids) {
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

// ---- point queries (mon_scene_query_points, mon_scene_query_lattice, mon_object_query_points): the map asked at places.  A small sibling of
// scene_list_run: no rays, no sample lists, no composite.  Per pass of at most kRenderChunkRays points every object's k_scene_points writes its rows
// [objects][cap][12] (u[3], inside, raw4, sigma, r, g, b), then k_scene_points_fold writes the pass's slice of the seven output rows (sigma | rgb 3n | owner
// | owner_sigma | n_inside).  Everything is enqueued at once; the outputs go home through the pinned staging with one synchronisation.  Render grids are
// not consulted (nothing is skipped), and neither the sample count nor the XORWOW render mode matters: nothing is sampled or jittered.
// The points of one pass: kRenderChunkRays, as the other scene routes.  A variant build (tools/variant_build.sh <tag> -DMON_POINTS_PASS=n) takes another
// size for measurements (tools/scene_points_timing.py: a pass of 16 384 points is a grid of 64 workgroups); outputs do not depend on it.
#ifndef MON_POINTS_PASS
#define MON_POINTS_PASS kRenderChunkRays
#endif
constexpr uint32_t kScenePointsPass = MON_POINTS_PASS;
static int points_outputs_check(const char* what, int side, const float* sigma) {
    REQUIRE_ARG(what, sigma, "sigma");
    return side_check(what, side);
}
int scene_points_check(int side, const float* xyz, size_t n, const float* sigma) {
    REQUIRE_ARG("scene_points", xyz, "points");
    { const int rc = points_outputs_check("scene_points", side, sigma); if (rc) return rc; }
    if (n == 0 || n > kSceneProbeMaxQueries) { set_error("scene_points: %zu points (1 to %u)", n, kSceneProbeMaxQueries); return MON_ERR_ARG; }
    for (size_t i = 0; i < 3 * n; ++i) if (!std::isfinite(xyz[i])) { set_error("scene_points: point %zu is not finite", i / 3); return MON_ERR_ARG; }
    return MON_OK;
}
// the lattice's shape alone (mon_lattice_points, which has no side and no outputs) ...
static int lattice_dims_check(const char* what, int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) { set_error("%s: lattice %d x %d x %d (each at least 1)", what, nx, ny, nz); return MON_ERR_ARG; }
    // (each factor bounded before it is multiplied: three ints of up to 2^31 - 1 wrap a 64-bit product)
    const uint64_t mx = kSceneProbeMaxQueries;
    if ((uint64_t)nx > mx || (uint64_t)ny > mx / (uint64_t)nx || (uint64_t)nz > mx / ((uint64_t)nx * (uint64_t)ny)) { set_error("%s: lattice %d x %d x %d has more than %u points", what, nx, ny, nz,
        kSceneProbeMaxQueries); return MON_ERR_ARG; }
    return MON_OK;
}
static int lattice_shape_check(const char* what, const float* origin3, const float* step3, int nx, int ny, int nz) {
    REQUIRE_ARG(what, origin3, "origin"); REQUIRE_ARG(what, step3, "step");
    { const int rc = lattice_dims_check(what, nx, ny, nz); if (rc) return rc; }
    const int dims[3] = { nx, ny, nz };
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin3[a]) || !std::isfinite(step3[a])) { set_error("%s: origin or step is not finite", what); return MON_ERR_ARG; }
        // (fmaf is monotone in the index: the far end is finite iff every point of the axis is)
        if (!std::isfinite(std::fmaf((float)(dims[a] - 1), step3[a], origin3[a]))) { set_error("%s: the lattice leaves the finite floats on axis %d", what, a);
            return MON_ERR_ARG; }
    }
    return MON_OK;
}
// ... and the query on it
int scene_lattice_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, const float* sigma) {
    { const int rc = lattice_shape_check("scene_lattice", origin3, step3, nx, ny, nz); if (rc) return rc; }
    return points_outputs_check("scene_lattice", side, sigma);
}
// mon_lattice_points: the floats k_scene_points forms from a lattice index, on the host (one fmaf per coordinate, ix fastest)
int scene_lattice_points(const float* origin3, const float* step3, int nx, int ny, int nz, float* xyz_out) {
    { const int rc = lattice_shape_check("lattice_points", origin3, step3, nx, ny, nz); if (rc) return rc; }
    REQUIRE_ARG("lattice_points", xyz_out, "xyz_out");
    float* o = xyz_out;
    for (int iz = 0; iz < nz; ++iz) for (int iy = 0; iy < ny; ++iy) for (int ix = 0; ix < nx; ++ix, o += 3) {
        o[0] = std::fmaf((float)ix, step3[0], origin3[0]); o[1] = std::fmaf((float)iy, step3[1], origin3[1]); o[2] = std::fmaf((float)iz, step3[2], origin3[2]); }
    return MON_OK;
}
// the MON_ERR_STATE cases of a point query: the layer-kernel shapes and, on side 1, a missing snapshot
static int scene_points_state_check(const char* what, Model* const* ms, size_t n, int side) {
    for (size_t j = 0; j < n; ++j) {
        Model& m = *ms[j];
        if (!rskip_supported(m)) { set_error("%s: object %zu does not run on the fused kernels", what, j); return MON_ERR_STATE; }
        if (side == 1 && !model_has_snapshot(m)) { set_error("%s: object %zu has no published snapshot", what, j); return MON_ERR_STATE; }
    }
    return MON_OK;
}
// q.xyz: the list ([q.n][3]; `world` false: unit-cube points of the one object), or nullptr: the lattice q.origin, q.step, q.nx x q.ny x q.nz (q.n its points).
// rows (mon_debug_scene_point_rows, mon_object_query_points; may be nullptr) = object rows_k's rows of every point, host array [q.n][12].
static int scene_points_run(const char* what, Model* const* ms, size_t n, int side, const ScenePoints& q, bool world, float* sigma, float* rgb, int32_t* owner,
                            float* owner_sigma, uint32_t* n_inside, const int32_t* ids, size_t rows_k, float* rows) {
    { const int rc = scene_points_state_check(what, ms, n, side); if (rc) return rc; }
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const size_t n_q = q.n; const uint32_t nq = (uint32_t)n_q, cap = std::min(nq, kScenePointsPass), L = (uint32_t)n;
    SceneWs& ws = side_ws<SceneWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, ws.mu, ws.ev); if (rc) return rc; }
    const hipStream_t s = sd.s;
    const std::vector<SceneSrc> src = scene_sources(ms, n, side, sd, false);
    // the output area: [the dumped rows 12 n_q |] sigma | rgb 3 n_q | owner | owner_sigma | n_inside (the rows first: every piece copied stays 16-byte aligned)
    const size_t rows_floats = rows ? 12 * n_q : 0, out_floats = rows_floats + 7 * n_q;
    {   int rc;
        if ((rc = ws.rows.grow((size_t)L * cap * 12)) || (rc = ws.out.grow(out_floats)) || (rc = ws.h_out.grow(out_floats)) ||
            (q.xyz && (rc = ws.pts.grow(3 * n_q)))) return rc; }
    if (q.xyz) HIPCHECK(hipMemcpyAsync(ws.pts.p, q.xyz, 12 * n_q, hipMemcpyHostToDevice, s));
    float* o = ws.out.p + rows_floats;
    for (uint32_t p0 = 0; p0 < nq; p0 += cap) {
        const uint32_t nc = std::min(cap, nq - p0);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j];
            ScenePointsArgs a{}; a.pts = q.xyz ? ws.pts.p + 3 * (size_t)p0 : nullptr; a.nx = (uint32_t)q.nx; a.ny = (uint32_t)q.ny; a.first = p0; a.n = nc;
            for (int k = 0; k < 3; ++k) { a.origin[k] = q.origin[k]; a.step[k] = q.step[k]; }
            a.rows = ws.rows.p + j * (size_t)cap * 12;
            launch_scene_points(s, m.lf, m.nd, sd.prm[j], m.oc, src[j].frag, p0 == 0u, world, a);
        }
        launch_scene_points_fold(s, nc, L, cap, ws.rows.p, o + p0, o + n_q + 3 * (size_t)p0, reinterpret_cast<int32_t*>(o + 4 * n_q) + p0, o + 5 * n_q + p0,
                reinterpret_cast<uint32_t*>(o + 6 * n_q) + p0);
        if (rows) launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.rows.p + rows_k * (size_t)cap * 12),
                reinterpret_cast<uint16_t*>(ws.out.p + 12 * (size_t)p0), 24u * nc);
    }
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.out.p), reinterpret_cast<uint16_t*>(ws.h_out.p), (uint32_t)(2 * out_floats));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    const float* h = ws.h_out.p + rows_floats;
    if (rows) std::memcpy(rows, ws.h_out.p, 4 * rows_floats);
    if (sigma) std::memcpy(sigma, h, 4 * n_q);
    if (rgb) std::memcpy(rgb, h + n_q, 12 * n_q);
    scene_instances_home(owner, h + 4 * n_q, n_q, ids);
    if (owner_sigma) std::memcpy(owner_sigma, h + 5 * n_q, 4 * n_q);
    if (n_inside) std::memcpy(n_inside, h + 6 * n_q, 4 * n_q);
    return MON_OK;
}
int scene_points(Model* const* ms, size_t n, int side, const ScenePoints& q, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside,
                 const int32_t* ids, size_t rows_k, float* rows) {
    return scene_points_run(q.xyz ? "scene_points" : "scene_lattice", ms, n, side, q, true, sigma, rgb, owner, owner_sigma, n_inside, ids, rows_k, rows);
}
// mon_object_query_points: the same kernel with the transform switched off, on points of the object's unit cube; raw4 out of its rows
int object_points_check(int side, const float* unit_xyz, size_t n, const float* raw4) {
    REQUIRE_ARG("object_points", unit_xyz, "points"); REQUIRE_ARG("object_points", raw4, "raw4");
    { const int rc = side_check("object_points", side); if (rc) return rc; }
    if (n == 0 || n > kSceneProbeMaxQueries) { set_error("object_points: %zu points (1 to %u)", n, kSceneProbeMaxQueries); return MON_ERR_ARG; }
    for (size_t i = 0; i < 3 * n; ++i) if (!(unit_xyz[i] >= 0.f && unit_xyz[i] <= 1.f)) { set_error("object_points: point %zu lies outside the unit cube", i / 3);
        return MON_ERR_ARG; }
    return MON_OK;
}
int object_points(Model& m, int side, const float* unit_xyz, size_t n, float* raw4) {
    Model* ms[1] = { &m };
    ScenePoints q{}; q.xyz = unit_xyz; q.n = n; q.nx = q.ny = q.nz = 1;
    std::vector<float> rows(12 * n);
    const int rc = scene_points_run("object_points", ms, 1, side, q, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) std::memcpy(raw4 + 4 * i, rows.data() + 12 * i + 4, 16);
    return MON_OK;
}

// ---- distance fields (mon_distance_transform, mon_scene_distance_lattice): clearance over a lattice.  scene_distance is the lattice
// query's sibling: the same state check, side, passes of k_scene_points and fold, whose sigma and owner rows stay on the device; then the mask
// (k_distance_mask), the three passes of k_distance_pass and k_distance_finish, once more on the complement when free_dist is asked for, one copy home
// and one synchronisation.  The side's workspace keeps the mask (1 B per cell) and the passes' two halves of squared distance and site (16 B per cell),
// shared by the two transforms, which run one after the other.
static int distance_outputs_check(const char* what, float max_dist, const float* dist) {
    REQUIRE_ARG(what, dist, "dist");
    if (!(max_dist > 0.f)) { set_error("%s: max_dist %g (above 0; +inf for no limit)", what, (double)max_dist); return MON_ERR_ARG; }
    return MON_OK;
}
int distance_transform_check(const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, const float* dist) {
    REQUIRE_ARG("distance_transform", occupied, "occupied"); REQUIRE_ARG("distance_transform", step3, "step");
    { const int rc = lattice_dims_check("distance_transform", nx, ny, nz); if (rc) return rc; }
    for (int a = 0; a < 3; ++a) if (!std::isfinite(step3[a])) { set_error("distance_transform: step is not finite"); return MON_ERR_ARG; }
    return distance_outputs_check("distance_transform", max_dist, dist);
}
int scene_distance_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist, const float* dist) {
    { const int rc = lattice_shape_check("scene_distance", origin3, step3, nx, ny, nz); if (rc) return rc; }
    { const int rc = side_check("scene_distance", side); if (rc) return rc; }
    if (!std::isfinite(sigma_min) || sigma_min < 0.f) { set_error("scene_distance: sigma_min %g (finite, >= 0)", (double)sigma_min); return MON_ERR_ARG; }
    return distance_outputs_check("scene_distance", max_dist, dist);
}
// mon_distance_transform: the transform alone on a host mask, in buffers of its own on the device's default stream
int distance_transform(int device, const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, float* dist, int32_t* nearest) {
    int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("no HIP device available"); return MON_ERR_NO_DEVICE; }
    HIPCHECK(use_device(device));
    const size_t n = (size_t)nx * ny * nz;
    DevBuf<uint8_t> occ; DevBuf<float> v; DevBuf<int32_t> site;                     // v, site: the passes' two halves, then the output row
    { int rc; if ((rc = occ.grow(n)) || (rc = v.grow(3 * n)) || (rc = site.grow(3 * n))) return rc; }
    HIPCHECK(hipMemcpy(occ.p, occupied, n, hipMemcpyHostToDevice));
    launch_distance_passes(nullptr, occ.p, false, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, step3, v.p, site.p);
    launch_distance_finish(nullptr, (uint32_t)n, v.p, site.p, max_dist, nullptr, v.p + 2 * n, nearest ? site.p + 2 * n : nullptr, nullptr);
    HIPCHECK(hipGetLastError());
    std::vector<float> h_dist(n); std::vector<int32_t> h_near(nearest ? n : 0);     // (the caller's arrays are written only once everything has succeeded)
    HIPCHECK(hipMemcpy(h_dist.data(), v.p + 2 * n, 4 * n, hipMemcpyDeviceToHost));
    if (nearest) HIPCHECK(hipMemcpy(h_near.data(), site.p + 2 * n, 4 * n, hipMemcpyDeviceToHost));
    std::memcpy(dist, h_dist.data(), 4 * n);
    if (nearest) std::memcpy(nearest, h_near.data(), 4 * n);
    return MON_OK;
}
// the lattice query's kernels as scene_distance and scene_components run them in front of their own: every pass's k_scene_points per object and its fold,
// the five rows (sigma n_q | rgb 3 n_q | owner n_q | owner_sigma n_q | n_inside n_q) at the places given; rows: the pass's workspace [objects][cap][12]
static void lattice_query_enqueue(hipStream_t s, Model* const* ms, size_t n, const ScenePoints& q, const SceneSide& sd, const std::vector<SceneSrc>& src,
        float* rows, uint32_t cap, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside) {
    const uint32_t nq = (uint32_t)q.n, L = (uint32_t)n;
    for (uint32_t p0 = 0; p0 < nq; p0 += cap) {
        const uint32_t nc = std::min(cap, nq - p0);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j];
            ScenePointsArgs a{}; a.pts = nullptr; a.nx = (uint32_t)q.nx; a.ny = (uint32_t)q.ny; a.first = p0; a.n = nc;
            for (int k = 0; k < 3; ++k) { a.origin[k] = q.origin[k]; a.step[k] = q.step[k]; }
            a.rows = rows + j * (size_t)cap * 12;
            launch_scene_points(s, m.lf, m.nd, sd.prm[j], m.oc, src[j].frag, p0 == 0u, true, a);
        }
        launch_scene_points_fold(s, nc, L, cap, rows, sigma + p0, rgb + 3 * (size_t)p0, owner + p0, owner_sigma + p0, n_inside + p0);
    }
}
// q: a lattice (scene_lattice).  ids as scene_points', applied to nearest_owner.  max_dist truncates dist and free_dist alike.
int scene_distance(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float max_dist, float* dist, int32_t* nearest,
                   int32_t* nearest_owner, float* free_dist, float* sigma, const int32_t* ids) {
    { const int rc = scene_points_state_check("scene_distance", ms, n, side); if (rc) return rc; }
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const size_t n_q = q.n; const uint32_t nq = (uint32_t)n_q, cap = std::min(nq, kScenePointsPass), L = (uint32_t)n;
    SceneWs& ws = side_ws<SceneWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, ws.mu, ws.ev); if (rc) return rc; }
    const hipStream_t s = sd.s;
    const std::vector<SceneSrc> src = scene_sources(ms, n, side, sd, false);
    // the output area: sigma | dist | nearest | nearest_owner | free_dist (what may go home, from the front) | rgb 3 n_q | owner | owner_sigma | n_inside
    const size_t out_floats = 11 * n_q, home_rows = free_dist ? 5 : nearest_owner ? 4 : nearest ? 3 : 2;
    {   int rc;
        if ((rc = ws.rows.grow((size_t)L * cap * 12)) || (rc = ws.out.grow(out_floats)) || (rc = ws.h_out.grow(home_rows * n_q)) || (rc = ws.docc.grow(n_q)) ||
            (rc = ws.dv.grow(2 * n_q)) || (rc = ws.dsite.grow(2 * n_q))) return rc; }
    float* o = ws.out.p; int32_t* o_owner = reinterpret_cast<int32_t*>(o + 8 * n_q);
    lattice_query_enqueue(s, ms, n, q, sd, src, ws.rows.p, cap, o, o + 5 * n_q, o_owner, o + 9 * n_q, reinterpret_cast<uint32_t*>(o + 10 * n_q));
    launch_distance_mask(s, nq, o, sigma_min, ws.docc.p);
    launch_distance_passes(s, ws.docc.p, false, (uint32_t)q.nx, (uint32_t)q.ny, (uint32_t)q.nz, q.step, ws.dv.p, ws.dsite.p);
    launch_distance_finish(s, nq, ws.dv.p, ws.dsite.p, max_dist, o_owner, o + n_q, nearest ? reinterpret_cast<int32_t*>(o + 2 * n_q) : nullptr,
            nearest_owner ? reinterpret_cast<int32_t*>(o + 3 * n_q) : nullptr);
    if (free_dist) {
        launch_distance_passes(s, ws.docc.p, true, (uint32_t)q.nx, (uint32_t)q.ny, (uint32_t)q.nz, q.step, ws.dv.p, ws.dsite.p);
        launch_distance_finish(s, nq, ws.dv.p, ws.dsite.p, max_dist, nullptr, o + 4 * n_q, nullptr, nullptr);
    }
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.out.p), reinterpret_cast<uint16_t*>(ws.h_out.p), (uint32_t)(2 * home_rows * n_q));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    const float* h = ws.h_out.p;
    if (sigma) std::memcpy(sigma, h, 4 * n_q);
    std::memcpy(dist, h + n_q, 4 * n_q);
    if (nearest) std::memcpy(nearest, h + 2 * n_q, 4 * n_q);
    if (nearest_owner) scene_instances_home(nearest_owner, h + 3 * n_q, n_q, ids);
    if (free_dist) std::memcpy(free_dist, h + 4 * n_q, 4 * n_q);
    return MON_OK;
}

// ---- connected components (mon_label_components, mon_scene_components_lattice): which cells belong together.  scene_components is
// scene_distance's sibling: the lattice query's kernels, k_distance_mask, for region 1 the untruncated transform and the mask dist > clearance (written
// over the first mask, which the passes have consumed), the labelling (launch_components), one copy home (k_cc_home: the records that were written, not
// the table's whole room) and one synchronisation.  Per cell the side's workspace keeps the mask (1 B, shared with the distance call) and, in the output
// area, label and comp (8 B); region 1 also uses the distance call's passes (16 B).  The numbering's block sums are 4 B per 256 cells.
static int components_outputs_check(const char* what, int connectivity, const int32_t* label, const mon_lattice_component* table, const uint32_t* n_components) {
    REQUIRE_ARG(what, label, "label");
    if (table && !n_components) { set_error("%s: a table without n_components (the count says how many records were written)", what); return MON_ERR_ARG; }
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) { set_error("%s: connectivity %d (6, 18 or 26)", what, connectivity); return MON_ERR_ARG; }
    return MON_OK;
}
int label_components_check(const uint8_t* mask, int nx, int ny, int nz, int connectivity, const int32_t* label, const mon_lattice_component* table,
                           const uint32_t* n_components) {
    REQUIRE_ARG("label_components", mask, "mask");
    { const int rc = lattice_dims_check("label_components", nx, ny, nz); if (rc) return rc; }
    return components_outputs_check("label_components", connectivity, label, table, n_components);
}
int scene_components_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, int region, float clearance,
                           int connectivity, const int32_t* label, const mon_lattice_component* table, const uint32_t* n_components, const float* dist) {
    { const int rc = lattice_shape_check("scene_components", origin3, step3, nx, ny, nz); if (rc) return rc; }
    { const int rc = side_check("scene_components", side); if (rc) return rc; }
    if (!std::isfinite(sigma_min) || sigma_min < 0.f) { set_error("scene_components: sigma_min %g (finite, >= 0)", (double)sigma_min); return MON_ERR_ARG; }
    if (region != 0 && region != 1) { set_error("scene_components: region %d (0: occupied matter, 1: traversable space)", region); return MON_ERR_ARG; }
    if (region == 1 && (!std::isfinite(clearance) || clearance < 0.f)) { set_error("scene_components: clearance %g (finite, >= 0)", (double)clearance);
        return MON_ERR_ARG; }
    if (region == 0 && dist) { set_error("scene_components: dist belongs to region 1 (region 0 runs no distance transform)"); return MON_ERR_ARG; }
    return components_outputs_check("scene_components", connectivity, label, table, n_components);
}
static int components_flag_check(const char* what, uint32_t flag) {
    if (flag) { set_error("%s: a device loop ran into its cap (flag %#x); no output was written", what, flag); return MON_ERR_STATE; }
    return MON_OK;
}
// mon_label_components: the labelling alone on a host mask, in buffers of its own on the device's default stream.
// w: label n | comp n | meta 8 (n_components, the cap flag) | the table's records, 8 words each | the numbering's block sums
int label_components(int device, const uint8_t* mask, int nx, int ny, int nz, int connectivity, int32_t* label, int32_t* comp, mon_lattice_component* table,
                     uint32_t cap, uint32_t* n_components) {
    int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("no HIP device available"); return MON_ERR_NO_DEVICE; }
    HIPCHECK(use_device(device));
    const size_t n = (size_t)nx * ny * nz, tcap = table ? std::min((size_t)cap, n) : 0, front = 2 * n + 8;
    DevBuf<uint8_t> occ; DevBuf<uint32_t> w;
    { int rc; if ((rc = occ.grow(n)) || (rc = w.grow(front + 8 * tcap + components_scan_words((uint32_t)n)))) return rc; }
    HIPCHECK(hipMemcpy(occ.p, mask, n, hipMemcpyHostToDevice));
    int32_t* d_label = reinterpret_cast<int32_t*>(w.p); uint32_t* d_meta = w.p + 2 * n;
    launch_components(nullptr, occ.p, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, connectivity, d_label, d_label + n, w.p + front + 8 * tcap,
            tcap ? reinterpret_cast<mon_lattice_component*>(w.p + front) : nullptr, (uint32_t)tcap, d_meta);
    HIPCHECK(hipGetLastError());
    std::vector<uint32_t> h(front);                                                 // (the caller's arrays are written only once everything has succeeded)
    HIPCHECK(hipMemcpy(h.data(), w.p, 4 * front, hipMemcpyDeviceToHost));
    { const int rc = components_flag_check("label_components", h[2 * n + 1]); if (rc) return rc; }
    const size_t used = std::min((size_t)h[2 * n], tcap);
    std::vector<uint32_t> h_table(8 * used);
    if (used) HIPCHECK(hipMemcpy(h_table.data(), w.p + front, 32 * used, hipMemcpyDeviceToHost));
    std::memcpy(label, h.data(), 4 * n);
    if (comp) std::memcpy(comp, h.data() + n, 4 * n);
    if (used) std::memcpy(table, h_table.data(), 32 * used);
    if (n_components) *n_components = h[2 * n];
    return MON_OK;
}
// q: a lattice (scene_lattice).  ids as scene_points', applied to owner.
int scene_components(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, int region, float clearance, int connectivity,
                     int32_t* label, int32_t* comp, mon_lattice_component* table, uint32_t cap, uint32_t* n_components, float* dist, float* sigma,
                     int32_t* owner, const int32_t* ids) {
    { const int rc = scene_points_state_check("scene_components", ms, n, side); if (rc) return rc; }
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const size_t n_q = q.n; const uint32_t nq = (uint32_t)n_q, pass = std::min(nq, kScenePointsPass), L = (uint32_t)n;
    SceneWs& ws = side_ws<SceneWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, ws.mu, ws.ev); if (rc) return rc; }
    const hipStream_t s = sd.s;
    const std::vector<SceneSrc> src = scene_sources(ms, n, side, sd, false);
    // the output area, what may go home from the front: label | comp | meta 8 | the table's records | (region 1: dist) | sigma | owner, then rgb 3 n_q |
    // owner_sigma | n_inside
    const size_t tcap = table ? std::min((size_t)cap, n_q) : 0, front = 2 * n_q + 8, rows0 = front + 8 * tcap, n_opt = region == 1 ? 3 : 2;
    const size_t home = rows0 + (owner ? n_opt : sigma ? n_opt - 1 : dist ? 1 : 0) * n_q;
    {   int rc;
        if ((rc = ws.rows.grow((size_t)L * pass * 12)) || (rc = ws.out.grow(rows0 + (n_opt + 5) * n_q)) || (rc = ws.h_out.grow(home)) || (rc = ws.docc.grow(n_q)) ||
            (rc = ws.cscan.grow(components_scan_words(nq))) || (region == 1 && ((rc = ws.dv.grow(2 * n_q)) || (rc = ws.dsite.grow(2 * n_q))))) return rc; }
    float* o = ws.out.p; uint32_t* o_meta = reinterpret_cast<uint32_t*>(o + 2 * n_q);
    float* o_dist = o + rows0; float* o_sigma = o + rows0 + (n_opt - 2) * n_q; int32_t* o_owner = reinterpret_cast<int32_t*>(o_sigma + n_q);
    float* o_rest = o_sigma + 2 * n_q;
    lattice_query_enqueue(s, ms, n, q, sd, src, ws.rows.p, pass, o_sigma, o_rest, o_owner, o_rest + 3 * n_q, reinterpret_cast<uint32_t*>(o_rest + 4 * n_q));
    launch_distance_mask(s, nq, o_sigma, sigma_min, ws.docc.p);
    if (region == 1) {
        launch_distance_passes(s, ws.docc.p, false, (uint32_t)q.nx, (uint32_t)q.ny, (uint32_t)q.nz, q.step, ws.dv.p, ws.dsite.p);
        launch_distance_finish(s, nq, ws.dv.p, ws.dsite.p, INFINITY, nullptr, o_dist, nullptr, nullptr);
        launch_components_clear_mask(s, nq, o_dist, clearance, ws.docc.p);
    }
    launch_components(s, ws.docc.p, (uint32_t)q.nx, (uint32_t)q.ny, (uint32_t)q.nz, connectivity, reinterpret_cast<int32_t*>(o), reinterpret_cast<int32_t*>(o + n_q),
            ws.cscan.p, tcap ? reinterpret_cast<mon_lattice_component*>(o + front) : nullptr, (uint32_t)tcap, o_meta);
    launch_components_home(s, reinterpret_cast<const uint32_t*>(o), reinterpret_cast<uint32_t*>(ws.h_out.p), (uint32_t)home, (uint32_t)front, (uint32_t)tcap, o_meta);
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    const float* h = ws.h_out.p; const uint32_t* h_meta = reinterpret_cast<const uint32_t*>(h + 2 * n_q);
    { const int rc = components_flag_check("scene_components", h_meta[1]); if (rc) return rc; }
    std::memcpy(label, h, 4 * n_q);
    if (comp) std::memcpy(comp, h + n_q, 4 * n_q);
    if (table) std::memcpy(table, h + front, 32 * std::min((size_t)h_meta[0], tcap));
    if (n_components) *n_components = h_meta[0];
    if (dist) std::memcpy(dist, h + rows0, 4 * n_q);
    if (sigma) std::memcpy(sigma, h + rows0 + (n_opt - 2) * n_q, 4 * n_q);
    if (owner) scene_instances_home(owner, h + rows0 + (n_opt - 1) * n_q, n_q, ids);
    return MON_OK;
}

// ---- point gradients (mon_scene_query_gradients, mon_scene_query_lattice_gradients, mon_object_query_gradients): scene_points_run's
// sibling with rows of 16 floats (k_scene_point_grads) and the fold that adds grad_log, grad_sigma and normal.  Beside the points the call keeps in the
// side's workspace every object's FULL fragment image (the backward reads the transposed matrices; the objects' own render images hold the forward set
// only and are left alone), the level weights (ones for NULL) and `select`.  The same passes, one enqueue, one synchronisation.
// What can be judged without an object: the points as scene_points_check judges them, the required outputs, select's range (n_objs is an argument) and
// the first weight (every object has at least one level, so level_weights[0] is always read); the other weights need Lmax: scene_gradients_weights_check.
static int weight_value_check(const char* what, const float* w, int l) {
    if (!std::isfinite(w[l]) || w[l] < 0.f) { set_error("%s: level weight %d is %g (finite, >= 0)", what, l, (double)w[l]); return MON_ERR_ARG; }
    return MON_OK;
}
static int gradients_args_check(const char* what, const float* level_w, const int32_t* select, size_t n_pts, size_t n_objs, const float* grad_log) {
    REQUIRE_ARG(what, grad_log, "grad_log");
    if (level_w) { const int rc = weight_value_check(what, level_w, 0); if (rc) return rc; }
    if (select) for (size_t i = 0; i < n_pts; ++i) if (select[i] < -1 || (int64_t)select[i] >= (int64_t)n_objs) {
        set_error("%s: select[%zu] = %d (-1 or an index below %zu)", what, i, select[i], n_objs); return MON_ERR_ARG; }
    return MON_OK;
}
int scene_gradients_check(int side, const float* xyz, size_t n, const float* level_w, const int32_t* select, size_t n_objs, const float* sigma,
                          const float* grad_log) {
    { const int rc = scene_points_check(side, xyz, n, sigma); if (rc) return rc; }
    return gradients_args_check("scene_gradients", level_w, select, n, n_objs, grad_log);
}
int scene_lattice_gradients_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, const float* level_w, const float* sigma,
                                  const float* grad_log) {
    { const int rc = scene_lattice_check(side, origin3, step3, nx, ny, nz, sigma); if (rc) return rc; }
    return gradients_args_check("scene_lattice_gradients", level_w, nullptr, 0, 0, grad_log);
}
int scene_gradients_weights_check(Model* const* ms, size_t n, const float* level_w) {
    return level_w ? level_weights_check("scene_gradients", level_w, scene_levels(ms, n).Lmax) : MON_OK;
}
// rows (mon_debug_scene_gradient_rows, mon_object_query_gradients; may be nullptr) = object rows_k's rows of every point, host array [q.n][16].
static int scene_gradients_run(const char* what, Model* const* ms, size_t n, int side, const ScenePoints& q, bool world, const float* level_w,
                               const int32_t* select, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log,
                               float* grad_sigma, float* normal, const int32_t* ids, size_t rows_k, float* rows) {
    { const int rc = scene_points_state_check(what, ms, n, side); if (rc) return rc; }
    const int device = ms[0]->device;
    HIPCHECK(use_device(device));
    const size_t n_q = q.n; const uint32_t nq = (uint32_t)n_q, cap = std::min(nq, kScenePointsPass), L = (uint32_t)n;
    const int Lmax = scene_levels(ms, n).Lmax;
    std::vector<size_t> frag_off(n + 1, 0);
    for (size_t j = 0; j < n; ++j) { const NetDims& nd = ms[j]->nd; const FragDims fd{ nd.Epad, nd.W, nd.NH, nd.L }; frag_off[j + 1] = frag_off[j] + (size_t)fd.N_FRAGS() * 512; }
    const std::vector<float> ones(level_w ? 0 : (size_t)Lmax, 1.f);
    SceneWs& ws = side_ws<SceneWs>(device, side);
    SceneSide sd; { const int rc = sd.enter(ms, n, side, ws.mu, ws.ev); if (rc) return rc; }
    const hipStream_t s = sd.s;
    // the output area: [the dumped rows 16 n_q |] sigma | rgb 3 n_q | owner | owner_sigma | n_inside | grad_log 3 n_q | grad_sigma 3 n_q | normal 3 n_q
    const size_t rows_floats = rows ? 16 * n_q : 0, out_floats = rows_floats + 16 * n_q;
    {   int rc;
        if ((rc = ws.rows.grow((size_t)L * cap * 16)) || (rc = ws.out.grow(out_floats)) || (rc = ws.h_out.grow(out_floats)) || (rc = ws.gfrag.grow(frag_off[n])) ||
            (rc = ws.lw.grow((size_t)Lmax)) || (q.xyz && (rc = ws.pts.grow(3 * n_q))) || (select && (rc = ws.sel.grow(n_q)))) return rc; }
    if (q.xyz) HIPCHECK(hipMemcpyAsync(ws.pts.p, q.xyz, 12 * n_q, hipMemcpyHostToDevice, s));
    if (select) HIPCHECK(hipMemcpyAsync(ws.sel.p, select, 4 * n_q, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(ws.lw.p, level_w ? level_w : ones.data(), 4 * (size_t)Lmax, hipMemcpyHostToDevice, s));
    float* o = ws.out.p + rows_floats;
    for (uint32_t p0 = 0; p0 < nq; p0 += cap) {
        const uint32_t nc = std::min(cap, nq - p0);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j];
            ScenePointsArgs a{}; a.pts = q.xyz ? ws.pts.p + 3 * (size_t)p0 : nullptr; a.nx = (uint32_t)q.nx; a.ny = (uint32_t)q.ny; a.first = p0; a.n = nc;
            for (int k = 0; k < 3; ++k) { a.origin[k] = q.origin[k]; a.step[k] = q.step[k]; }
            a.rows = ws.rows.p + j * (size_t)cap * 16;
            launch_scene_point_grads(s, m.lf, m.nd, sd.prm[j], m.oc, ws.gfrag.p + frag_off[j], p0 == 0u, world, a, ws.lw.p);
        }
        launch_scene_gradients_fold(s, nc, L, cap, ws.rows.p, select ? ws.sel.p + p0 : nullptr, o + p0, o + n_q + 3 * (size_t)p0,
                reinterpret_cast<int32_t*>(o + 4 * n_q) + p0, o + 5 * n_q + p0, reinterpret_cast<uint32_t*>(o + 6 * n_q) + p0, o + 7 * n_q + 3 * (size_t)p0,
                o + 10 * n_q + 3 * (size_t)p0, o + 13 * n_q + 3 * (size_t)p0);
        if (rows) launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.rows.p + rows_k * (size_t)cap * 16),
                reinterpret_cast<uint16_t*>(ws.out.p + 16 * (size_t)p0), 32u * nc);
    }
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.out.p), reinterpret_cast<uint16_t*>(ws.h_out.p), (uint32_t)(2 * out_floats));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    const float* h = ws.h_out.p + rows_floats;
    if (rows) std::memcpy(rows, ws.h_out.p, 4 * rows_floats);
    if (sigma) std::memcpy(sigma, h, 4 * n_q);
    if (rgb) std::memcpy(rgb, h + n_q, 12 * n_q);
    scene_instances_home(owner, h + 4 * n_q, n_q, ids);
    if (owner_sigma) std::memcpy(owner_sigma, h + 5 * n_q, 4 * n_q);
    if (n_inside) std::memcpy(n_inside, h + 6 * n_q, 4 * n_q);
    if (grad_log) std::memcpy(grad_log, h + 7 * n_q, 12 * n_q);
    if (grad_sigma) std::memcpy(grad_sigma, h + 10 * n_q, 12 * n_q);
    if (normal) std::memcpy(normal, h + 13 * n_q, 12 * n_q);
    return MON_OK;
}
int scene_gradients(Model* const* ms, size_t n, int side, const ScenePoints& q, const float* level_w, const int32_t* select, float* sigma, float* rgb,
                    int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma, float* normal, const int32_t* ids,
                    size_t rows_k, float* rows) {
    return scene_gradients_run(q.xyz ? "scene_gradients" : "scene_lattice_gradients", ms, n, side, q, true, level_w, select, sigma, rgb, owner, owner_sigma,
                               n_inside, grad_log, grad_sigma, normal, ids, rows_k, rows);
}
// mon_object_query_gradients: the same kernel with the transform switched off and the extent taken as 1 (nothing is divided): raw4 and d raw3 / d u
int object_gradients_check(int side, const float* unit_xyz, size_t n, const float* level_w, const float* grad_unit) {
    REQUIRE_ARG("object_gradients", grad_unit, "grad_unit");
    { const int rc = object_points_check(side, unit_xyz, n, grad_unit); if (rc) return rc; }
    return level_w ? weight_value_check("object_gradients", level_w, 0) : MON_OK;
}
int object_gradients(Model& m, int side, const float* unit_xyz, size_t n, const float* level_w, float* raw4, float* grad_unit) {
    if (level_w) { const int rc = level_weights_check("object_gradients", level_w, (int)m.nd.L); if (rc) return rc; }
    Model* ms[1] = { &m };
    ScenePoints q{}; q.xyz = unit_xyz; q.n = n; q.nx = q.ny = q.nz = 1;
    std::vector<float> rows(16 * n);
    const int rc = scene_gradients_run("object_gradients", ms, 1, side, q, false, level_w, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr, 0, rows.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) { if (raw4) std::memcpy(raw4 + 4 * i, rows.data() + 16 * i + 4, 16); std::memcpy(grad_unit + 3 * i, rows.data() + 16 * i + 12, 12); }
    return MON_OK;
}
// mon_scene_cast_normals / mon_online_cast_normals: a host-side rule over two routes -- the cast; x = fmaf(hit_t, d, o) per axis for the rays with a hit;
// the gradients at those points, compacted in ray order, with select = the hit object; scattered back, 0 0 0 for a miss.  Two enqueues, two
// synchronisations (one when no ray hits).  ids: applied to both instance outputs at the end (the rule itself runs on indices into ms).
int scene_cast_normals_check(int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* level_w, const float* rgb, const float* dist,
                             const float* normal) {
    { const int rc = scene_cast_check(side, rays, n_rays, hit_opacity, rgb, dist); if (rc) return rc; }
    REQUIRE_ARG("scene_cast_normals", normal, "normal");
    return level_w ? weight_value_check("scene_cast_normals", level_w, 0) : MON_OK;
}
int scene_cast_normals(Model* const* ms, size_t n, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* level_w, float* rgb,
                       float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance, float* hit_xyz, float* normal,
                       float* grad_log, const int32_t* ids) {
    std::vector<float> t_own; std::vector<int32_t> inst_own;
    if (!hit_t) { t_own.resize(n_rays); hit_t = t_own.data(); }
    if (!hit_instance) { inst_own.resize(n_rays); hit_instance = inst_own.data(); }
    { const int rc = scene_cast(ms, n, side, rays, n_rays, hit_opacity, rgb, dist, opacity, instance, hit_t, hit_sample_t, hit_instance, nullptr, nullptr);
      if (rc) return rc; }
    std::vector<float> x; std::vector<int32_t> sel; std::vector<size_t> at;
    for (size_t i = 0; i < n_rays; ++i) {
        if (hit_instance[i] < 0) continue;
        for (int a = 0; a < 3; ++a) x.push_back(std::fmaf(hit_t[i], rays[i].d[a], rays[i].o[a]));
        sel.push_back(hit_instance[i]); at.push_back(i);
    }
    const size_t nh = at.size();
    std::vector<float> sg(nh), gl(3 * nh), nr(3 * nh);
    if (nh) {
        ScenePoints q{}; q.xyz = x.data(); q.n = nh; q.nx = q.ny = q.nz = 1;
        const int rc = scene_gradients(ms, n, side, q, level_w, sel.data(), sg.data(), nullptr, nullptr, nullptr, nullptr, gl.data(), nullptr, nr.data(), nullptr,
                                       0, nullptr);
        if (rc) return rc;
    }
    if (hit_xyz) std::fill(hit_xyz, hit_xyz + 3 * n_rays, 0.f);
    if (grad_log) std::fill(grad_log, grad_log + 3 * n_rays, 0.f);
    std::fill(normal, normal + 3 * n_rays, 0.f);
    for (size_t k = 0; k < nh; ++k) for (int a = 0; a < 3; ++a) {
        if (hit_xyz) hit_xyz[3 * at[k] + a] = x[3 * k + a];
        if (grad_log) grad_log[3 * at[k] + a] = gl[3 * k + a];
        normal[3 * at[k] + a] = nr[3 * k + a];
    }
    if (ids) for (size_t i = 0; i < n_rays; ++i) {
        if (instance && instance[i] >= 0) instance[i] = ids[instance[i]];
        if (hit_instance[i] >= 0) hit_instance[i] = ids[hit_instance[i]];
    }
    return MON_OK;
}

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
