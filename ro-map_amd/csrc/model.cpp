// model.cpp -- host side of one object NeRF on one gfx950 device.
// Mirrors nerf::NeRF_Model (CORE/src/nerf_model.cu:1259-1830) and nerf::NeRF_Dataset
// (CORE/src/nerf_data.cu:123-339) without Eigen/OpenCV/tcnn types.  Differences by design:
//   * the whole iteration is enqueued on one HIP stream with no host synchronisation (the
//     reference syncs 3x per iteration: nerf_model.cu:1459,1469,1645); counters live in DevState;
//   * an iteration can be replayed as a hipGraph;
//   * the dataset is one packed RGBA8+instance slab per device instead of per-frame float buffers.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <dlfcn.h>
#include "model_internal.h"
#include "xorwow.h"

namespace mon {

static thread_local std::string g_err;
void set_error(const char* fmt, ...) {
    char buf[1024]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap); g_err = buf;
}
const char* last_error() { return g_err.c_str(); }

// Logical devices: what the managers and the C ABI number 0 .. n-1.  By default they are the physical HIP devices; mon_set_logical_devices(n)
// maps n logical devices round-robin onto the physical ones, so the multi-device code paths (object k -> device k mod nGPU, one dataset replica and
// one stream pool per device, CORE/src/nerf.cu:27-33, nerf_manager.cu:44-55) also run -- oversubscribed -- on a box with fewer GPUs.
static std::atomic<int> g_logical_devices{ 0 };
static int physical_count() {          // (asked once: use_device sits on every entry point, and the runtime call takes a process-wide lock)
    static const int n = [] { int c = 0; return (hipGetDeviceCount(&c) == hipSuccess) ? c : 0; }();
    return n;
}
hipError_t use_device(int logical) {
    const int phys = physical_count(); if (phys < 1) return hipErrorNoDevice;
    const int n = g_logical_devices.load(); if (logical < 0 || logical >= (n > 0 ? n : phys)) return hipErrorInvalidDevice;
    return hipSetDevice(logical % phys);
}
int device_enter(int device) {
    int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("no HIP device available"); return MON_ERR_NO_DEVICE; }
    HIPCHECK(use_device(device));
    return MON_OK;
}
int physical_device(int logical, int* phys_out) {
    const int phys = physical_count(); const int n = g_logical_devices.load();
    if (phys < 1 || logical < 0 || logical >= (n > 0 ? n : phys) || !phys_out) { set_error("physical_device: no such logical device %d", logical);
        return MON_ERR_ARG; }
    *phys_out = logical % phys; return MON_OK;
}
int set_logical_devices(int n) {
    if (n < 0 || n > 64) { set_error("set_logical_devices: 0 (= the physical devices) .. 64"); return MON_ERR_ARG; }
    g_logical_devices.store(n); return MON_OK;
}
int device_count(int* n) {
    int c = 0; hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c < 1) { *n = 0; set_error("Can not Detect GPU: %s", hipGetErrorString(e)); return MON_ERR_NO_DEVICE; }
    const int l = g_logical_devices.load(); *n = l > 0 ? l : c; return MON_OK;
}

// ------------------------------------------------------------------ dataset
// the devices' inference streams and pinned result buffers (InferShared, model_internal.h)
static std::mutex g_infer_mu; static std::map<int, InferShared*> g_infer_shared;
static int infer_shared_get(int device, size_t pixels_hint, InferShared** out) {
    InferShared* sh = nullptr;
    {   std::lock_guard<std::mutex> l(g_infer_mu);       // the map lookup only: a viewer render holds sh->mu across stream syncs, and object creation
        InferShared*& slot = g_infer_shared[device];     // (SLAM thread, any device) must not queue behind it with the global lock held
        if (!slot) {
            slot = new InferShared();
            int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&slot->stream, hipStreamNonBlocking, hi) != hipSuccess) {
                delete slot; slot = nullptr; set_error("inference stream creation failed on device %d", device); return MON_ERR_HIP;
            }
        }
        sh = slot;
    }
    if (5 * pixels_hint > sh->h_cap.load(std::memory_order_acquire)) {      // (grow-only: the common case takes no lock at all)
        std::lock_guard<std::mutex> l2(sh->mu);          // h_out / growth belong to sh->mu: model_render_snapshot resizes them under it
        if (5 * pixels_hint <= sh->h_cap.load(std::memory_order_relaxed)) { *out = sh; return MON_OK; }
        float* q = nullptr; if (hipHostMalloc((void**)&q, 5 * pixels_hint * sizeof(float), hipHostMallocDefault) != hipSuccess) {
            set_error("pinned render buffer allocation failed"); return MON_ERR_HIP; }
        if (sh->h_out) hipHostFree(sh->h_out);
        sh->h_out = q; sh->h_cap = 5 * pixels_hint;
    }
    *out = sh; return MON_OK;
}

// ---- tile render workspace (kernels_tilerender.hip): per device and side, grow-only, never freed (like the inference stream)
static std::atomic<uint64_t> g_weights_epoch{ 1 };
uint64_t next_weights_epoch() { return g_weights_epoch.fetch_add(1); }
// objects: tile-capable objects alive on the device (under g_tile_mu); the buffers go with the last one
struct TileWsPair { TileWs side[2]; int objects = 0; };
static std::mutex g_tile_mu; static std::map<int, TileWsPair*> g_tile_ws;
template <class T> static int ws_grow(T*& p, size_t n_elems) {      // (contents are scratch: nothing to carry over)
    void* q = nullptr;
    if (hipMalloc(&q, n_elems * sizeof(T)) != hipSuccess) { set_error("tile render workspace: allocation of %zu bytes failed", n_elems * sizeof(T));
        return MON_ERR_HIP; }
    if (p) hipFree(p);
    p = (T*)q; return MON_OK;
}
// caller must hold ws->mu before it touches the buffers; the capacity checks below run under it too (two objects of one device may ask at once)
int tile_ws_get(Model& m, int side, size_t n_pix, TileWs** out) {
    // (the workspace is filed under m.device: allocate it there whatever device the calling thread happens to have current)
    HIPCHECK(use_device(m.device));
    TileWsPair* pr = nullptr;
    {   std::lock_guard<std::mutex> l(g_tile_mu);
        TileWsPair*& slot = g_tile_ws[m.device]; if (!slot) slot = new TileWsPair(); pr = slot; }
    TileWs& ws = pr->side[side & 1];
    std::lock_guard<std::mutex> l(ws.mu);
    int rc;
    const uint32_t cap = kTileChunkJobs * 64u;
    if (!ws.counters) {
        if ((rc = ws_grow(ws.counters, 64))) return rc;
        // (hipMemset of device memory may return before the fill has run, and the renders' streams are non-blocking: without the synchronisation the fill can
        // land in the middle of the first render's ray kernel -- the job count restarts, k_tile_render reads job records nobody wrote and writes to the pixel
        // index it finds there: the memory fault of the object-churn test, seen whenever a device's last object had returned the workspace)
        HIPCHECK(hipMemset(ws.counters, 0, 256)); HIPCHECK(hipDeviceSynchronize());
    }
    if (ws.cap < cap || ws.L_cap < m.nd.L) {
        const int L = std::max(ws.L_cap, m.nd.L);
        if ((rc = ws_grow(ws.x, 4 * (size_t)cap)) || (rc = ws_grow(ws.e, (size_t)L * 2 * cap)) || (rc = ws_grow(ws.O, 4 * (size_t)cap))) return rc;
        ws.cap = cap; ws.L_cap = L;
    }
    if (!ws.frag && (rc = ws_grow(ws.frag, 64 * 512))) return rc;
    if (ws.image_cap < 2 * (size_t)m.n_grid) { if ((rc = ws_grow(ws.image, 2 * (size_t)m.n_grid + 64))) return rc; ws.image_cap = 2 * (size_t)m.n_grid;
        ws.key_epoch = ~0ull; }
    if (ws.rec_cap < n_pix) { const size_t c = std::max<size_t>(n_pix, 2 * ws.rec_cap); if ((rc = ws_grow(ws.rec, 12 * c))) return rc; ws.rec_cap = c; }
    *out = &ws; return MON_OK;
}
int tile_ws_skip_buffers(TileWs& ws, size_t n_pix) {
    int rc;
    const size_t chunks = (n_pix + kTileChunkJobs - 1) / kTileChunkJobs, cnt_words = std::max<size_t>(chunks, 1) * render_list_parts() * kRenderListStride;
    if (ws.job_bits_cap < n_pix) { const size_t c = std::max<size_t>(n_pix, 2 * ws.job_bits_cap); if ((rc = ws_grow(ws.job_bits, 2 * c))) return rc;
        ws.job_bits_cap = c; }
    if (ws.live_cnt_cap < cnt_words) { if ((rc = ws_grow(ws.live_cnt, cnt_words))) return rc; ws.live_cnt_cap = cnt_words; }
    if (!ws.live_idx && (rc = ws_grow(ws.live_idx, (size_t)render_list_parts() * render_list_spw(ws.cap)))) return rc;
    return MON_OK;
}
static void tile_ws_object_born(int device) { std::lock_guard<std::mutex> l(g_tile_mu); TileWsPair*& slot = g_tile_ws[device];
    if (!slot) slot = new TileWsPair(); ++slot->objects; }
static void tile_ws_object_gone(int device) {
    std::lock_guard<std::mutex> l(g_tile_mu);
    auto it = g_tile_ws.find(device); if (it == g_tile_ws.end() || --it->second->objects > 0) return;
    // the device's last object: a few hundred MB of scratch are returned (nobody can hold ws.mu: users are objects)
    for (TileWs& ws : it->second->side) {
        std::lock_guard<std::mutex> wl(ws.mu);
        for (void* q : { (void*)ws.rec, (void*)ws.counters, (void*)ws.x, (void*)ws.e, (void*)ws.O, (void*)ws.image, (void*)ws.frag, (void*)ws.job_bits,
                         (void*)ws.live_idx, (void*)ws.live_cnt }) if (q) hipFree(q);
        ws.rec = nullptr; ws.counters = nullptr; ws.x = nullptr; ws.e = nullptr; ws.O = nullptr; ws.image = nullptr; ws.frag = nullptr;
        ws.job_bits = nullptr; ws.live_idx = nullptr; ws.live_cnt = nullptr; ws.job_bits_cap = 0; ws.live_cnt_cap = 0;
        ws.rec_cap = 0; ws.cap = 0; ws.L_cap = 0; ws.image_cap = 0; ws.flip = 0; ws.key_params = nullptr; ws.key_epoch = ~0ull;
    }
}
static int tile_ws_objects(int device) { std::lock_guard<std::mutex> l(g_tile_mu); auto it = g_tile_ws.find(device);
    return it == g_tile_ws.end() ? 0 : it->second->objects; }
void tile_ws_weights(Model& m, TileWs& ws, hipStream_t s, const uint16_t* prm, uint64_t epoch) {
    if (ws.key_params == prm && ws.key_epoch == epoch) return;
    launch_build_feat_image(s, m.lf, m.nd, prm, ws.image, nullptr);
    launch_forward_frag_image(s, m.nd, prm, ws.frag);
    ws.key_params = prm; ws.key_epoch = epoch;
}
void tile_points_forward(Model& m, TileWs& ws, hipStream_t s, uint32_t n) {
    launch_encode_feat(s, m.lf, m.nd, ws.image, ws.x, ws.e, ws.cap, n, nullptr, 0u, 0u, 1u);
    launch_tile_points_mlp(s, m.nd, ws.frag, ws.e, ws.cap, n, ws.O);
}
// NeRF_Model::Render's body (:1768-1828) for a whole crop on the tile path: rays + hit compaction, then per chunk of jobs points -> encode -> MLP + composite
// into the device buffers rgb / depth / mask (pixel order); caller holds ws.mu and has called tile_ws_weights.  sk.bits: render skipping (the OCC / LIVE
// kernels; the lists' counters of every chunk are cleared up front)
static int tile_render_crop(Model& m, TileWs& ws, hipStream_t s, const ObjectConst& oc, mon_frame_bbox box, const Mat4& pose, int pose_is_Toc,
                            float* rgb, float* depth, float* mask, RenderSkipArgs sk = RenderSkipArgs{}) {
    const uint32_t n_pix = box.w * box.h;
    if (sk.bits) {
        { const int rc = tile_ws_skip_buffers(ws, n_pix); if (rc) return rc; }
        const size_t chunks = (n_pix + kTileChunkJobs - 1) / kTileChunkJobs;
        HIPCHECK(hipMemsetAsync(ws.live_cnt, 0, chunks * render_list_parts() * kRenderListStride * 4, s));
        sk.job_bits = ws.job_bits; sk.idx = ws.live_idx; sk.spw = render_list_spw(ws.cap);
    }
    uint32_t* cnt = ws.counters + 16u * (ws.flip & 1u); uint32_t* next = ws.counters + 16u * ((ws.flip + 1u) & 1u); ++ws.flip;
    launch_render_rays_jobs(s, m.ds->K, oc, box, pose, pose_is_Toc, n_pix, ws.rec, cnt, next, rgb, depth, mask);
    for (uint32_t j0 = 0; j0 < n_pix; j0 += kTileChunkJobs) {          // (the job count lives on the device: chunks past it return at once)
        const uint32_t jc = std::min(kTileChunkJobs, n_pix - j0);
        if (sk.bits) sk.cnt = ws.live_cnt + (size_t)(j0 / kTileChunkJobs) * render_list_parts() * kRenderListStride;
        launch_render_points(s, oc, ws.rec, cnt, j0, jc, ws.x, sk);
        launch_encode_feat(s, m.lf, m.nd, ws.image, ws.x, ws.e, ws.cap, 0u, cnt, j0, jc, 2u * oc.S, sk);
        launch_tile_render(s, m.nd, oc, ws.frag, ws.rec, cnt, j0, jc, ws.x, ws.e, ws.cap, n_pix, rgb, depth, mask, sk);
    }
    return MON_OK;
}
// whether a crop of n_pix rays goes to the tile path (option tile_render: 0 never, 1 from 4096 rays up -- below that the tile copies cost what the gathers cost
// --, 2 always)
static bool tile_render_wanted(const Model& m, size_t n_pix) {
    const long o = options().tile_render;
    return m.backend == 1 && m.plan.tile_render && m.oc.S == 32u && o != 0 && (o >= 2 || n_pix >= 4096);
}

int dataset_create(int device, int H, int W, float fx, float fy, float cx, float cy, uint32_t max_frames, int use_depth, Dataset** out) {
    int n = 0; int rc = device_count(&n); if (rc) return rc;
    if (device < 0 || device >= n || H <= 0 || W <= 0 || max_frames == 0) { set_error("dataset_create: bad argument"); return MON_ERR_ARG; }
    HIPCHECK(use_device(device));
    Dataset* d = new Dataset();
    d->device = device; d->K = Intrinsics{ fx, fy, cx, cy, H, W }; d->max_frames = max_frames; d->use_depth = use_depth != 0;
    const size_t px = (size_t)H * W;
    const auto alloc = [&]() -> int {
        HIPCHECK(hipMalloc((void**)&d->d_rgba, px * 4 * max_frames));
        // a frame id never uploaded reads as black / instance 0, not as whatever the allocation held
        HIPCHECK(hipMemset(d->d_rgba, 0, px * 4 * max_frames));
        if (d->use_depth) { HIPCHECK(hipMalloc((void**)&d->d_depth, px * 4 * max_frames)); HIPCHECK(hipMemset(d->d_depth, 0, px * 4 * max_frames)); }
        HIPCHECK(hipMalloc((void**)&d->d_poses, 64 * (size_t)max_frames));
        HIPCHECK(hipMemset(d->d_poses, 0, 64 * (size_t)max_frames));
        // hipMemset returns before the fill has run (null stream), and the upload stream is non-blocking: without this wait the fill can land AFTER the first
        // frames' packing kernels and wipe them (seen as frames that read as black / instance 0 now and then -- more valid candidate rays than the oracle has)
        HIPCHECK(hipStreamSynchronize(nullptr));
        return MON_OK;
    };
    if ((rc = alloc())) { dataset_destroy(d); return rc; }          // e.g. out of memory for max_frames images: free what was taken
    d->present.assign(max_frames, 0);
    // frames arrive through a pinned staging buffer and are packed by a kernel on the device's high-priority stream (see dataset_add_frame)
    { InferShared* sh = nullptr; if ((rc = infer_shared_get(device, px, &sh))) { dataset_destroy(d); return rc; } d->upload = sh; }
    (void)lanes_get(device);                                            // the device's training lanes exist before its first object
    // (coherent pinned memory, and the packing kernels read it with system-scope loads: the same host addresses are rewritten for every frame)
    d->stage_bytes = px * 9 + 128;                                      // raw colour (<= 4 B/pixel), instance (1 B), depth (4 B), pose
    if (hipHostMalloc((void**)&d->h_stage, d->stage_bytes, hipHostMallocCoherent) != hipSuccess) {
        set_error("dataset_create: pinned staging allocation failed"); dataset_destroy(d); return MON_ERR_HIP; }
    *out = d; return MON_OK;
}
int dataset_add_frame(Dataset* d, uint32_t id, const uint8_t* rgb, int ch, int is_bgr, const uint8_t* inst, const float* depth, const float* Twc) {
    if (!d || !rgb || !inst || !Twc || (ch != 3 && ch != 4)) { set_error("dataset_add_frame: bad argument"); return MON_ERR_ARG; }
    if (id >= d->max_frames) { set_error("dataset_add_frame: frame id %u >= capacity %u", id, d->max_frames); return MON_ERR_ARG; }
    if (d->use_depth && !depth) { set_error("depth img error: dataset was created with use_depth"); return MON_ERR_ARG; }      // nerf_data.cu:296-300
    HIPCHECK(use_device(d->device));
    const size_t px = (size_t)d->K.H * d->K.W;
    const int ri = is_bgr ? 2 : 0, bi = is_bgr ? 0 : 2;             // cv::COLOR_BGR2RGB, nerf_data.cu:167,286
    // The caller's (pageable) images are copied into pinned memory and packed to 4 B/pixel by a kernel that reads them across PCIe, on the device's
    // high-priority stream: a synchronous hipMemcpy from pageable memory goes through the runtime's blit path at normal priority and, with a dozen objects
    // training, kept the SLAM thread 4 ms per frame (8 ms worst case); the host-side pack loop alone cost 0.4 ms.
    InferShared* sh = static_cast<InferShared*>(d->upload); std::lock_guard<std::mutex> one(sh->mu);
    uint8_t* st_rgb = d->h_stage, *st_inst = st_rgb + px * 4; float* st_depth = reinterpret_cast<float*>(st_inst + ((px + 15) & ~(size_t)15));
    float* st_pose = st_depth + (d->use_depth ? px : 0);
    std::memcpy(st_rgb, rgb, px * (size_t)ch); std::memcpy(st_inst, inst, px); std::memcpy(st_pose, Twc, 64);
    launch_pack_frame(sh->stream, st_rgb, ch, ri, bi, st_inst, d->d_rgba + px * id, (uint32_t)px);
    if (d->use_depth) { std::memcpy(st_depth, depth, px * 4); launch_copy_from_host(sh->stream, st_depth, d->d_depth + px * id, (uint32_t)px); }
    launch_copy_from_host(sh->stream, st_pose, d->d_poses + 16 * (size_t)id, 16u);
    HIPCHECK(hipStreamSynchronize(sh->stream)); HIPCHECK(hipGetLastError());
    if (id + 1 > d->n_frames) d->n_frames = id + 1;                 // mFrameDataNum, nerf_data.cu:338
    d->present[id] = 1;
    return MON_OK;
}
// UpdateDataGPU (nerf_data.cu:341-353): overwrite the poses of n consecutive frames
int dataset_update_poses(Dataset* d, uint32_t first, uint32_t n, const float* Twc16s) {
    if (!d || !Twc16s || first + n > d->max_frames) {
        set_error("update_poses: frames %u..%u outside the dataset (%u frames)", first, first + n, d ? d->max_frames : 0u); return MON_ERR_ARG; }
    HIPCHECK(use_device(d->device));
    HIPCHECK(hipMemcpy(d->d_poses + 16 * (size_t)first, Twc16s, 64 * (size_t)n, hipMemcpyHostToDevice));
    return MON_OK;
}
int dataset_destroy(Dataset* d) {
    if (!d) return MON_OK;
    use_device(d->device);
    if (d->d_rgba) hipFree(d->d_rgba);
    if (d->d_depth) hipFree(d->d_depth);
    if (d->d_poses) hipFree(d->d_poses);
    if (d->h_stage) hipHostFree(d->h_stage);
    delete d; return MON_OK;
}

// ------------------------------------------------------------------ model
// hipStreamCreate costs ~8 ms (a hardware queue is set up), and CreateNeRF runs on the SLAM thread: streams of destroyed objects are
// kept for the next object of that device, and a manager can reserve some ahead of time (mon_online_dataset_init).
static std::mutex g_stream_mu; static std::map<int, std::vector<hipStream_t>> g_stream_pool;
static int stream_acquire(int device, hipStream_t* out) {
    { std::lock_guard<std::mutex> l(g_stream_mu); auto& v = g_stream_pool[device]; if (!v.empty()) { *out = v.back(); v.pop_back(); return MON_OK; } }
    HIPCHECK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));       // mpTrainStream, nerf_model.cu:1268
    return MON_OK;
}
static void stream_release(int device, hipStream_t s) { std::lock_guard<std::mutex> l(g_stream_mu); g_stream_pool[device].push_back(s); }
int stream_pool_reserve(int device, int n) {
    HIPCHECK(use_device(device));
    std::vector<hipStream_t> fresh;
    { std::lock_guard<std::mutex> l(g_stream_mu); n -= (int)g_stream_pool[device].size(); }
    int rc = MON_OK;
    for (int i = 0; i < n; ++i) {
        hipStream_t s; const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess) { set_error("hipStreamCreateWithFlags failed: %s", hipGetErrorString(e)); rc = MON_ERR_HIP; break; }
        fresh.push_back(s);
    }
    std::lock_guard<std::mutex> l(g_stream_mu); for (hipStream_t s : fresh) g_stream_pool[device].push_back(s);      // what was created is kept either way
    return rc;
}

// ---- render skipping (mon_object_set_render_skip): per side, a grid of the weights the render reads, cached per weights stamp and min_alpha
static int rskip_alloc(Model& m, RenderSkipSide& k) {
    if (k.d_grid) return MON_OK;
    int rc;
    if ((rc = dev_alloc(m, k.d_grid, kOccWords)) || (rc = dev_alloc(m, k.d_raw, kOccWords)) || (rc = dev_alloc(m, k.d_stats, 4))) return rc;
    HIPCHECK(hipHostMalloc((void**)&k.h_stats, 16, hipHostMallocDefault)); std::memset(k.h_stats, 0, 16);
    return MON_OK;
}
const uint32_t* rskip_grid(Model& m, RenderSkipSide& k, hipStream_t s, float alpha, const uint16_t* prm, uint64_t epoch, uint16_t* frag) {
    if (!k.d_grid) return nullptr;
    if (!k.pinned && (!k.built || k.epoch != epoch || k.alpha != alpha)) {
        if (alpha <= 0.f) {                                              // every cell live: no density pass
            (void)hipMemsetAsync(k.d_raw, 0xff, kOccWords * 4, s); (void)hipMemsetAsync(k.d_grid, 0xff, kOccWords * 4, s);
        } else {
            // alpha >= min_alpha  <=>  sigma >= -log(1 - min_alpha) / dt  <=>  raw density (log sigma) >= log(-log1p(-min_alpha) / dt), dt = diagonal / 2S
            double diag2 = 0.0; for (int a = 0; a < 3; ++a) diag2 += (double)(m.oc.aabb.mx[a] - m.oc.aabb.mn[a]) * (m.oc.aabb.mx[a] - m.oc.aabb.mn[a]);
            const double dt = std::max(std::sqrt(diag2) / (2.0 * m.oc.S), 1e-9);
            launch_occupancy_update(s, m.lf, m.nd, prm, m.oc, frag, (float)std::log(-std::log1p(-(double)alpha) / dt), k.d_raw, k.d_grid);
        }
        k.built = true; k.epoch = epoch; k.alpha = alpha; ++k.builds;
    }
    return k.d_grid;
}
// before a render of `prm` (stamp `epoch`) on stream s: the grid and the cleared counters; bits == nullptr when the switch is off
static RenderSkipArgs rskip_begin(Model& m, RenderSkipSide& k, hipStream_t s, bool on, float alpha, const uint16_t* prm, uint64_t epoch, uint16_t* frag) {
    k.active = false;
    if (!on || !k.d_grid) return RenderSkipArgs{};
    rskip_grid(m, k, s, alpha, prm, epoch, frag);
    (void)hipMemsetAsync(k.d_stats, 0, 16, s);
    k.active = true;
    RenderSkipArgs a; a.bits = k.d_grid; a.stats = k.d_stats; return a;
}
// the counters home inside the copy the render synchronises on (a copy kernel into pinned memory, like the snapshot render's results)
static void rskip_read(hipStream_t s, RenderSkipSide& k) { if (k.active) launch_copy_params(s, reinterpret_cast<const uint16_t*>(k.d_stats),
        reinterpret_cast<uint16_t*>(k.h_stats), 4u); }
static void rskip_end(RenderSkipSide& k) { if (k.active) { k.samples_live = k.h_stats[0]; k.samples_in_box = k.h_stats[1]; } }

// fp32 master weights from the host into the model (the arrays, or the chunk records through a staging buffer) + the fp16 working copy h(master)
static int upload_master(Model& m, const float* master) {
    const size_t n = m.n_params;
    if (!m.P.rec) {
        HIPCHECK(hipMemcpy(m.P.master, master, n * 4, hipMemcpyHostToDevice));
        launch_master_to_half(m.train_stream, m.P.master, m.P.half, (uint32_t)n);        // h(master), same rounding as every later update
        return MON_OK;
    }
    float* tmp = nullptr; HIPCHECK(hipMalloc((void**)&tmp, n * 4));
    hipError_t e = hipMemcpy(tmp, master, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) { launch_state_pack_master(m.train_stream, tmp, m.P.rec, (uint32_t)n);
        launch_master_to_half(m.train_stream, tmp, m.P.half, (uint32_t)n); e = hipStreamSynchronize(m.train_stream); }
    (void)hipFree(tmp); HIPCHECK(e); return MON_OK;
}
// ---- the plan of an object (TrainPlan, model.h): every rule about which chains a shape can run, once.  No HIP calls.
static uint32_t all_levels_mask(int L) { return (1u << L) - 1u; }          // (L <= kMaxLevels = 16)
// level-tile encode (kernels_encode.hip), batch size: a workgroup's two tile copies, four barriers and the launch cost the same whatever it walks -- measured
// (tools/kernel_times.py, both chains, same box):
// R = 1024 (C1) 48.9 vs 41.3 us per step for the gather chain, R = 2048 75.1 vs 75.4, R = 4096 99 vs 107, R = 8192 166 vs 172.  Option lds_encode = 1
// (default) takes the tile chain from 3072 rays (98 304 samples) up, 2 always (tests), 0 never.
static bool level_tiles_pay(long lds_encode, uint32_t Btrain) { return lds_encode != 0 && (lds_encode >= 2 || Btrain >= 98304u); }
TrainPlan train_plan(const mon_config& cfg, const LevelTable& lt, const NetDims& nd, uint32_t R, uint32_t S, bool lazy_ema, const PlanOptions& opt) {
    TrainPlan p{}; const uint32_t Btrain = R * S;
    p.lazy_ema = lazy_ema; p.fused = fused_supported(nd, S, R);
    p.fused_backend = p.fused && opt.backend != 0;             // option backend: -1 what the shape allows, 0 the layer-at-a-time kernels
    p.xorwow = rng_stream_mode(cfg.rng_flags) != 0;
    ScatterLevels sl{}; const uint32_t mask = scatter_plan(lt, nd, sl); const bool all = mask == all_levels_mask(nd.L);
    // every level must fit two LDS tiles and go through the LDS scatter (option lds_encode = 0: gathers inside k_fused_train)
    const bool tiles_fit = level_tiles_pay(opt.lds_encode, Btrain) && all && encode_tiles_supported(lt, nd);
    if (p.fused) {
        p.lds_mask = mask; p.lds_all = all; p.level_tiles = tiles_fit;
        // Levels beyond the LDS plan (more than 2^18 entries): binned exact scatter while many samples carry a gradient (kernels_bigscatter.hip).
        // Option big_switch = gradient-carrying samples below which the global-atomic path takes over (0: atomics always).
        p.big_scatter = mask && big_scatter_workspace_bytes(lt, nd, mask, Btrain) && opt.big_switch;
        // chunk flags for the lazy optimizer (tables above 8 M parameters with levels outside the LDS plan); MON_VARIANT_NO_FLAGS: scan the gradient table
        p.touched_flags = kTouchedFlags && lazy_ema && mask && !all;
        p.occupancy = cfg.occupancy_skip != 0;
        // (a position block's 256 samples lie in one sample partition of the encode, and a partition's list fits its spw slots)
        const uint32_t spw = encode_tiles_spw(Btrain), parts = (Btrain + spw - 1u) / spw, blocks = (Btrain + 255u) / 256u;
        p.live_lists = p.occupancy && p.level_tiles && Btrain % 256u == 0u && parts <= kLiveMaxParts && ((blocks + parts - 1u) / parts) * 256u <= spw;
        p.tile_render = !lazy_ema && tile_render_supported(lt, nd);
    } else {
        p.layer_ws = (Btrain & 31u) == 0u;
        // (16 neurons, 2 x 128, three / four hidden layers; tables up to 2^18 entries per level -- see k_rows_to_bins)
        p.hybrid_scatter = S == 32u && !lazy_ema && all && (R % kDefaultScatterBins) == 0u;
        // ... and their forward encode from LDS level tiles like the fused chain's (k_encode_tiles; same batch-size rule, option lds_encode)
        p.level_tiles = p.hybrid_scatter && p.layer_ws && tiles_fit;
    }
    p.inference_side = p.fused_backend && !lazy_ema && !p.xorwow;
    return p;
}
// ---- model_init's pieces, one per group of buffers; each allocates what the plan says
// parameters (ResetNetwork :1286-1342; Trainer init)
static int init_parameters(Model& m, bool init_params) {
    const size_t n = m.n_params; int rc;
    // per-parameter step counters in 16 bits, saturating, where that is EXACT: 1 - beta^t == 1.0f (beta^t < 2^-25) for every t >= 65535 and both betas
    // (variant build MON_VARIANT_STEPS32: always 32 bits).  The device evaluates 1 - exp2f(t * log2(beta)) in fp32; the host test runs in double, so it keeps a
    // margin of four binades (beta^65535 < 2^-29, i.e. beta <= 0.99969) instead of sitting on the rounding boundary.
    const bool steps16 = steps16_exact(m.cfg);
    // large tables (lazy EMA, 16-bit step counters): the optimizer state as one 128-byte record per chunk (ParamPtrs::rec) instead of four arrays
    const bool records = m.plan.lazy_ema && steps16 && kStateRecords && (n & 7u) == 0u;
    if (records) { if ((rc = dev_alloc(m, m.P.rec, 4 * n))) return rc; }
    else if ((rc = dev_alloc(m, m.P.master, n, false)) || (rc = dev_alloc(m, m.P.m1, n)) || (rc = dev_alloc(m, m.P.m2, n)) ||
             (rc = steps16 ? dev_alloc(m, m.P.steps16, n + 8) : dev_alloc(m, m.P.steps, n))) return rc;
    // (chunk records keep the EMA step in their pad word: no array, ParamPtrs::lazy says "lazy")
    if ((rc = dev_alloc(m, m.P.half, n, false)) || (rc = dev_alloc(m, m.P.ema, n)) || (rc = records ? MON_OK : dev_alloc(m, m.d_ema_step, n / 8 + 1)) ||
        (rc = dev_alloc(m, m.P.gmlp, m.nd.n_mlp)) || (rc = dev_alloc(m, m.P.ggrid, m.n_grid))) return rc;
    if (init_params) {
        std::vector<float> master; init_params_host(m.cfg, m.nd, m.n_params, master);
        const int urc = upload_master(m, master.data()); if (urc) return urc;
    }
    return MON_OK;
}
// a candidate set of R rays; the rays of a batch or render pass
static int alloc_candidates(Model& m, BatchPtrs& b) {
    const size_t R = m.oc.R; int rc;
    if ((rc = dev_alloc(m, b.cand_o, 3 * R)) || (rc = dev_alloc(m, b.cand_d, 3 * R)) || (rc = dev_alloc(m, b.cand_dn, R)) || (rc = dev_alloc(m, b.cand_t0, R)) ||
        (rc = dev_alloc(m, b.cand_t1, R)) || (rc = dev_alloc(m, b.cand_depth, R)) || (rc = dev_alloc(m, b.cand_rgba, R))) return rc;
    return dev_alloc(m, b.mask, (R + 63) / 64 + 64);
}
static int alloc_rays(Model& m, BatchPtrs& b, size_t n) {
    int rc; if ((rc = dev_alloc(m, b.ray_o, 3 * n)) || (rc = dev_alloc(m, b.ray_d, 3 * n)) || (rc = dev_alloc(m, b.ray_dn, n)) || (rc = dev_alloc(m, b.ray_t0, n)) ||
        (rc = dev_alloc(m, b.ray_t1, n))) return rc;
    return dev_alloc(m, b.ray_flag, n);
}
// batch workspace (AllocateBatchWorkspace :1344-1427), sized for max(train batch, render chunk)
static int init_batch_workspace(Model& m) {
    const uint32_t R = m.oc.R, S = m.oc.S; int rc;
    m.ws_rays = R > kRenderChunkRays ? R : kRenderChunkRays;
    // the layer-at-a-time buffers (pts, tdist, E, O) serve a render pass of the unfused backend; an object whose inference runs on the fused kernels / level
    // tiles only needs them at the training batch's size (64 + 12 + 8 + 4 MB less per base.json object: a render of the unfused backend then takes passes of
    // ws_samples / 2S rays)
    const uint32_t Btrain = R * S, Brender = m.plan.fused_backend ? Btrain : kRenderChunkRays * 2 * S;
    m.ws_samples = Btrain > Brender ? Btrain : Brender;
    BatchPtrs& B = m.B;
    if ((rc = alloc_candidates(m, B)) || (rc = alloc_rays(m, B, m.ws_rays)) || (rc = dev_alloc(m, B.target, 3 * (size_t)R)) ||
        (rc = dev_alloc(m, B.target_depth, R)) || (rc = dev_alloc(m, B.bgcol, 3 * (size_t)R)) ||
        (rc = dev_alloc(m, B.pts, 3 * (size_t)m.ws_samples)) || (rc = dev_alloc(m, B.tdist, m.ws_samples)) ||
        (rc = dev_alloc(m, B.E, (size_t)m.ws_samples * m.nd.Epad)) || (rc = dev_alloc(m, B.O, (size_t)m.ws_samples * kOut)) ||
        (rc = dev_alloc(m, B.Hid, (size_t)Btrain * m.nd.W * m.nd.NH)) || (rc = dev_alloc(m, B.dO, (size_t)Btrain * kOut)) ||
        (rc = dev_alloc(m, B.dHid, (size_t)Btrain * m.nd.W * m.nd.NH)) || (rc = dev_alloc(m, B.dE, (size_t)Btrain * m.nd.Epad)) ||
        (rc = dev_alloc(m, B.rgb_ray, 3 * (size_t)R)) || (rc = dev_alloc(m, B.depth_ray, R)) || (rc = dev_alloc(m, B.mask_ray, R))
                || (rc = dev_alloc(m, B.loss_ray, R)) ||
        (rc = dev_alloc(m, m.d_state, 2)) || (rc = dev_alloc(m, m.d_dw_partials, (size_t)(fused_partial_cols(m.nd) + 64) * kMaxFusedGrid)) ||
        (rc = dev_alloc(m, m.d_out_all, 5 * (size_t)kRenderChunkRays))) return rc;
    m.out_cap = kRenderChunkRays; return MON_OK;
}
// "same inputs" mode: the reference's XORWOW stream (xorwow.h) instead of the counter RNG
static int init_xorwow(Model& m) {
    const uint32_t R = m.oc.R, S = m.oc.S; int rc;
    m.xw_lanes = rng_xorwow_lanes(m.cfg.rng_flags); m.xw_flavour = rng_stream_mode(m.cfg.rng_flags) == 2 ? kXorwowRocrand : kXorwowCurand;
    std::vector<XorwowState> st; xorwow_lane_states(0ull /* the generator's default seed: nerf_model.cu never sets one */, m.xw_flavour, m.xw_lanes, st);
    XorwowState *d_a = nullptr, *d_b = nullptr, *d_c = nullptr;
    if ((rc = dev_alloc(m, d_a, m.xw_lanes, false)) || (rc = dev_alloc(m, d_b, m.xw_lanes, false)) || (rc = dev_alloc(m, d_c, m.xw_lanes, false)) ||
        (rc = dev_alloc(m, m.d_xw, 2 * (size_t)(5 + S) * R))) return rc;
    HIPCHECK(hipMemcpy(d_a, st.data(), sizeof(XorwowState) * m.xw_lanes, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_c, st.data(), sizeof(XorwowState) * m.xw_lanes, hipMemcpyHostToDevice));
    m.d_xw_states = d_a; m.d_xw_render_states = d_b; m.d_xw_render_init = d_c;
    m.oc.xw[0] = m.d_xw; m.oc.xw[1] = m.d_xw + (size_t)(5 + S) * R; return MON_OK;
}
// k_grid_scatter's plan, hand-over buffers and partial tables for the levels of `mask` (a prefix: the fused chain's, or every level for the hybrid scatter)
static int alloc_lds_scatter(Model& m, uint32_t mask) {
    const size_t Btrain = (size_t)m.oc.R * m.oc.S; int rc;
    (void)scatter_plan(m.lt, m.nd, m.scatter);
    // a partial table spans the entries up to the end of the LAST LDS-scattered level (the plan covers a prefix of the levels: sizes grow with the level);
    // sized by the whole table it was 16 x 211 MB = 3.4 GB of a T = 2^22 object for the 37 k entries of its two small levels
    int last = -1; for (int l = 0; l < m.nd.L; ++l) if ((mask >> l) & 1u) last = l;
    m.part_halves = last < 0 ? 0u : ((2u * m.lt.offset[last + 1] + 15u) & ~15u);
    if (mask && ((rc = dev_alloc(m, m.d_de_soa, (size_t)m.nd.L * Btrain * 2)) || (rc = dev_alloc(m, m.d_x_soa, 4 * Btrain)))) return rc;
    return mask ? dev_alloc(m, m.d_gpart, (size_t)m.scatter.max_P * m.part_halves) : MON_OK;
}
// level-tile encode: positions, encoded features, the fp16 grid in tile order
static int alloc_level_tiles(Model& m) {
    const size_t Btrain = (size_t)m.oc.R * m.oc.S; int rc;
    if ((rc = dev_alloc(m, m.d_x_all, 4 * Btrain)) || (rc = dev_alloc(m, m.d_e_soa, (size_t)m.nd.L * Btrain * 2))
            || (rc = dev_alloc(m, m.d_half_tiles, (size_t)m.n_grid + 64))) return rc;
    encode_tiles_setup_device(); return MON_OK;
}
// fused-chain buffers
static int init_fused_buffers(Model& m) {
    const TrainPlan& p = m.plan; const uint32_t R = m.oc.R, Btrain = R * m.oc.S; int rc;
    if ((rc = dev_alloc(m, m.d_frag_train, 64 * 512)) || (rc = dev_alloc(m, m.d_frag_render, 64 * 512))) return rc;       // <= 30 fragments of 512 halves
    if ((rc = alloc_lds_scatter(m, p.lds_mask))) return rc;
    if (p.big_scatter && (rc = dev_alloc(m, m.d_big_ws, big_scatter_workspace_bytes(m.lt, m.nd, p.lds_mask, Btrain)))) return rc;
    if (p.level_tiles) {
        if ((rc = dev_alloc(m, m.B.ray_rec, 12 * (size_t)R))) return rc;
        m.B_alt = m.B;                             // (the second candidate set: cand_* / mask of its own, everything else shared)
        if ((rc = alloc_candidates(m, m.B_alt)) || (rc = alloc_level_tiles(m))) return rc;
    }
    return p.touched_flags ? dev_alloc(m, m.d_touched, (m.n_params >> 3) + 16) : MON_OK;
}
// layer-chain buffers (shapes outside the fused kernels)
static int init_layer_buffers(Model& m) {
    const TrainPlan& p = m.plan; int rc;
    // (zeroed: k_wgrad_reduce sums whole partial rows, and the entries no job writes -- rows 4..15 of the padded output layer -- must not be whatever the
    // allocation held before: they reach the pad weights' Adam state, and two identical objects then differ in get_params)
    if (p.layer_ws && (rc = dev_alloc(m, m.d_layers_T, layers_workspace_halves(m.nd, m.oc.R * m.oc.S)))) return rc;
    if (p.hybrid_scatter && (rc = alloc_lds_scatter(m, all_levels_mask(m.nd.L)))) return rc;
    if (p.level_tiles && (rc = alloc_level_tiles(m))) return rc;
    return MON_OK;
}
// occupancy grid (cfg.occupancy_skip) and the live-sample lists of the level-tile chain
static int init_occupancy(Model& m) {
    constexpr size_t words = (size_t)kOccRes * kOccRes * kOccRes / 32; int rc;
    if ((rc = dev_alloc(m, m.d_occ, words, false)) || (rc = dev_alloc(m, m.d_occ_tmp, words, false))
            || (rc = dev_alloc(m, m.d_frag_occ, 64 * 512))) return rc;
    HIPCHECK(hipMemset(m.d_occ, 0xff, words * 4));                       // warm-up: every cell counts as occupied
    // a cell is empty when one sample interval through it would be transparent: alpha = 1 - exp(-sigma * dt) < 1e-3 with dt = box diagonal / samples
    float diag2 = 0.f; for (int a = 0; a < 3; ++a) diag2 += (m.oc.aabb.mx[a] - m.oc.aabb.mn[a]) * (m.oc.aabb.mx[a] - m.oc.aabb.mn[a]);
    const float dt = std::sqrt(diag2) / (float)m.oc.S;
    m.occ_raw_threshold = std::log(1e-3f / std::max(dt, 1e-6f));
    if (m.plan.live_lists && ((rc = dev_alloc(m, m.d_live_idx, m.oc.R * m.oc.S)) || (rc = dev_alloc(m, m.d_live_cnt, 2u * kLiveMaxParts * kLiveCntStride))))
        return rc;
    return MON_OK;
}
// inference side: the published snapshots and a render workspace of their own (InferState, model_internal.h)
static int init_inference_side(Model& m) {
    InferState* is = new InferState(); m.infer = is; int rc;
    // (a whole frame fits: no growth in front of a viewer)
    if ((rc = infer_shared_get(m.device, (size_t)m.ds->K.W * (size_t)m.ds->K.H, &is->shared))) return rc;
    for (int k = 0; k < 2; ++k) { if ((rc = dev_alloc(m, is->snap[k], m.n_params, false))) return rc;
        HIPCHECK(hipEventCreateWithFlags(&is->ready[k], hipEventDisableTiming)); }
    is->rb = m.B;
    if ((rc = alloc_rays(m, is->rb, kRenderChunkRays)) || (rc = dev_alloc(m, is->out_all, 5 * (size_t)kRenderChunkRays)) ||
        (rc = dev_alloc(m, is->frag, 64 * 512))) return rc;
    is->out_cap = kRenderChunkRays; return MON_OK;
}
static int model_init(Model& m, Dataset* ds, const mon_config& cfg, int class_id, const float* Tow, const float* amin, const float* amax, bool init_params) {
    m.ds = ds; m.cfg = cfg; m.device = ds->device;
    int rc = level_table_build(cfg, m.lt, m.nd, m.n_grid); if (rc) return rc;
    m.n_params = m.nd.n_mlp + m.n_grid;
    level_fast_build(m.lt, m.nd, m.lf);
    HIPCHECK(use_device(m.device));
    // fixed-point unit of the exact LDS gradient accumulation: 2^-24 (every fp16 value is a multiple of it) up to the reference's loss scale of
    // 128, coarser by the next power of two of loss_scale / 128 beyond it, so that the int32 range always spans un-scaled gradient sums below 1.0
    int shift = 0; while (shift < 23 && 128.0f * (float)(1u << shift) < cfg.loss_scale) ++shift;
    m.lf.fix_scale = 16777216.0f / (float)(1u << shift); m.lf.fix_clamp = 100.0f * (float)(1u << shift);
    std::memcpy(m.oc.Tow.m, Tow, 64);
    for (int a = 0; a < 3; ++a) { m.oc.aabb.mn[a] = amin[a]; m.oc.aabb.mx[a] = amax[a]; }
    m.oc.instance_id = (uint32_t)(uint8_t)class_id;                 // nerf.cu:75,158
    m.oc.R = (uint32_t)cfg.rays_per_batch; m.oc.S = (uint32_t)cfg.n_samples; m.oc.use_depth = cfg.use_depth && m.ds->use_depth;
    m.oc.sample_seed = cfg.sample_seed; m.oc.loss_scale = cfg.loss_scale;
    m.n_bins = kDefaultScatterBins;
    m.opt = OptimConst{ cfg.beta1, cfg.beta2, cfg.epsilon, cfg.l2_reg, cfg.ema_decay, cfg.loss_scale, cfg.decay_base, std::log2(cfg.beta1),
            std::log2(cfg.beta2), std::log2(cfg.ema_decay), cfg.decay_start, cfg.decay_interval, m.nd.n_mlp, m.n_params };
    // lazy EMA: only where the optimizer is not the dense variant anyway and the table is large (> 8 M parameters)
    const PlanOptions opt{ options().backend, options().lds_encode, (uint32_t)options().big_switch };
    m.plan = train_plan(cfg, m.lt, m.nd, m.oc.R, m.oc.S, m.n_grid > (8u << 20), opt);
    const TrainPlan& p = m.plan;
    if (p.big_scatter) m.big_switch = opt.big_switch;
    { const int rcs = stream_acquire(m.device, &m.own_stream); if (rcs) return rcs; }
    m.train_stream = m.own_stream; m.lanes = lanes_get(m.device); lanes_objects_add(m.lanes, 1);
    if ((rc = init_parameters(m, init_params)) || (rc = init_batch_workspace(m)) || (p.xorwow && (rc = init_xorwow(m))) ||
        (rc = p.fused ? init_fused_buffers(m) : init_layer_buffers(m)) || (p.occupancy && (rc = init_occupancy(m)))) return rc;
    m.boxes_cap = 1024; if ((rc = dev_alloc(m, m.d_boxes, m.boxes_cap))) return rc;
    m.B.boxes = m.d_boxes; m.B_alt.boxes = m.d_boxes;
    m.h_state = DevState{}; m.h_state.lr = cfg.learning_rate;
    m.h_state.ema_deb_old = 0.0f; m.h_state.ema_deb_new = 1.0f / (1.0f - (float)std::pow((double)cfg.ema_decay, 1.0));   // step 1
    m.d_state_next = m.d_state + 1;                          // two states: iteration i runs on one, k_optimizer(i) writes the other for iteration i + 1
    HIPCHECK(hipMemcpy(m.d_state, &m.h_state, sizeof(DevState), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(m.d_state_next, &m.h_state, sizeof(DevState), hipMemcpyHostToDevice));
    HIPCHECK(hipHostMalloc((void**)&m.h_state_pinned, sizeof(DevState), hipHostMallocDefault));
    m.backend = p.fused_backend ? 1 : 0;
    m.mesh = mesh_state_create(m.device); m.weights_epoch = next_weights_epoch();
    if (p.tile_render) { tile_ws_object_born(m.device); m.tile_counted = true; }
    if (p.inference_side && (rc = init_inference_side(m))) return rc;
    // what this object's creation enqueued: the fills of its allocations (null stream) and its own stream's kernels.  NOT the device: with other objects'
    // training threads running, a device-wide wait stands behind everything they have queued -- a whole Train_Step of 500 iterations each in the offline
    // manager (CreateNeRF of the 8th object of a job took 125-140 ms, 9-23 ms with an idle device; eight objects 0.71-0.80 s -> 0.28-0.32 s of the caller's
    // time, same PSNRs, same job wall: tools/offline_job.py, A/B/A/B on one box)
    HIPCHECK(hipStreamSynchronize(nullptr)); HIPCHECK(hipStreamSynchronize(m.train_stream));
    return MON_OK;
}

// Owner thread, after a train call's state read-back: copy the inference weights (EMA once a step has been taken) into the snapshot buffer no reader
// holds and make it the current one.  ~4 us of device-to-device copy at base.json size, ordered on the train stream.
// A publication costs the owner thread ~15 us of host time (copy + event), which matters when the online manager trains in slices of a few
// iterations: unless forced (long train calls, set_params), it happens when a viewer has asked since the last one or 10 ms have passed.
int publish_snapshot(Model& m, bool force) {
    InferState* is = m.infer; if (!is) return MON_OK;
    const auto now = std::chrono::steady_clock::now();
    if (!force && is->latest >= 0 && !is->wanted.load() && now - is->last_pub < std::chrono::milliseconds(10)) return MON_OK;
    int w;
    {   std::lock_guard<std::mutex> l(is->mu); w = is->latest == 0 ? 1 : 0;
        // a render still reads the older buffer: keep the current snapshot this round (the viewer's request stays standing)
        if (is->readers[w] > 0) return MON_OK;
        // from here until the new copy's event is recorded the buffer is not a valid fall-back for a render: its event still shows the PREVIOUS copy as
        // complete
        // (two publications back to back, the first copy still queued behind other objects' chunks: a render fell back to this buffer while it was rewritten)
        is->written[w] = false; }
    const uint16_t* src = (m.h_state.step > 0) ? m.P.ema : m.P.half;
    launch_copy_params(m.train_stream, src, is->snap[w], m.n_params);
    HIPCHECK(hipEventRecord(is->ready[w], m.train_stream));
    { std::lock_guard<std::mutex> l(is->mu); is->step_of[w] = m.h_state.step; is->epoch_of[w] = next_weights_epoch(); is->written[w] = true; is->latest = w; }
    is->wanted.store(false); is->last_pub = now;          // (only now: a publication skipped above must not discard the viewer's request)
    return MON_OK;
}

int model_create_impl(Dataset* ds, const mon_config& cfg, int class_id, const float* Tow, const float* amin, const float* amax, bool init_params, Model** out) {
    if (!ds || !Tow || !amin || !amax) { set_error("object_create: bad argument"); return MON_ERR_ARG; }
    { const int rc = config_check(cfg); if (rc) return rc; }
    Model* mp = new Model();
    const int rc = model_init(*mp, ds, cfg, class_id, Tow, amin, amax, init_params);
    if (rc) { model_destroy(mp); return rc; }          // a failed allocation half-way must not leak what came before it
    *out = mp; return MON_OK;
}
int model_create(Dataset* ds, const mon_config& cfg, int class_id, const float* Tow, const float* amin, const float* amax, Model** out) {
    return model_create_impl(ds, cfg, class_id, Tow, amin, amax, true, out);
}

int model_destroy(Model* mp) {
    if (!mp) return MON_OK;
    Model& m = *mp; use_device(m.device);
    model_mesh_free(m);
    if (m.own_stream) model_leave_lane(m);
    if (m.train_stream) hipStreamSynchronize(m.train_stream);
    if (m.infer) {
        // (the stream and the pinned buffer stay with the device)
        InferState* is = m.infer; if (is->shared) { std::lock_guard<std::mutex> l(is->shared->mu); hipStreamSynchronize(is->shared->stream); }
        for (int k = 0; k < 2; ++k) if (is->ready[k]) hipEventDestroy(is->ready[k]);
        for (void* p : is->grown) hipFree(p);
        if (is->rskip.h_stats) (void)hipHostFree(is->rskip.h_stats);
        delete is; m.infer = nullptr;
    }
    pose_ws_free(m);
    drop_graph(m);
    if (m.tile_counted) { tile_ws_object_gone(m.device); m.tile_counted = false; }
    for (auto& e : m.ev_pool) hipEventDestroy(e);
    for (void* p : m.allocs) hipFree(p);
    if (m.h_state_pinned) hipHostFree(m.h_state_pinned);
    if (m.h_out) (void)hipHostFree(m.h_out);
    if (m.rskip.h_stats) (void)hipHostFree(m.rskip.h_stats);
    if (m.lanes) lanes_objects_add(m.lanes, -1);
    if (m.switch_event) hipEventDestroy(m.switch_event);
    if (m.sync_event) hipEventDestroy(m.sync_event);
    if (m.own_stream) { hipStreamSynchronize(m.own_stream); stream_release(m.device, m.own_stream); }        // idle: the next object of this device takes it
    delete mp; return MON_OK;
}

int model_add_boxes(Model& m, const mon_frame_bbox* boxes, size_t n) {
    if (!boxes || n == 0) { set_error("add_boxes: empty"); return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device));
    for (size_t i = 0; i < n; ++i) {
        const mon_frame_bbox& b = boxes[i];
        if (b.FrameId >= m.ds->max_frames || b.w == 0 || b.h == 0 || b.x + b.w > (uint32_t)m.ds->K.W || b.y + b.h > (uint32_t)m.ds->K.H) {
            set_error("add_boxes: box %zu (frame %u, x %u y %u h %u w %u) outside the %dx%d image / dataset capacity", i, b.FrameId, b.x, b.y, b.h, b.w,
                    m.ds->K.W, m.ds->K.H);
            return MON_ERR_ARG;
        }
        // the reference's callers always hand the frame over first (LocalMapping.cc:1175 before :1242); rays of an absent frame would train on nothing
        if (!m.ds->present[b.FrameId]) {
            set_error("add_boxes: box %zu names frame %u, which has not been added to the dataset", i, b.FrameId);
            return MON_ERR_STATE;
        }
    }
    model_leave_lane(m); HIPCHECK(hipStreamSynchronize(m.train_stream));
    bool moved = false;
    if (m.n_boxes + n > m.boxes_cap) {
        uint32_t cap = m.boxes_cap; while (cap < m.n_boxes + n) cap *= 2;
        mon_frame_bbox* nb = nullptr; int rc = dev_alloc(m, nb, cap); if (rc) return rc;
        HIPCHECK(hipMemcpy(nb, m.d_boxes, sizeof(mon_frame_bbox) * m.n_boxes, hipMemcpyDeviceToDevice));
        m.d_boxes = nb; m.B.boxes = nb; m.B_alt.boxes = nb; m.boxes_cap = cap; moved = true;       // old buffer stays in allocs until destroy
    }
    HIPCHECK(hipMemcpy(m.d_boxes + m.n_boxes, boxes, sizeof(mon_frame_bbox) * n, hipMemcpyHostToDevice));   // nerf_model.cu:1625
    m.n_boxes += (uint32_t)n;
    HIPCHECK(hipMemcpy(&m.d_state->n_boxes, &m.n_boxes, 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(&m.d_state_next->n_boxes, &m.n_boxes, 4, hipMemcpyHostToDevice));
    // (the copies above ran on the null stream, which the object's non-blocking streams do not wait for: a grown box list's zero-fill and device-to-device copy
    // are done before the next batch reads it)
    HIPCHECK(hipStreamSynchronize(nullptr));
    model_mark_stale(m, kStaleRays, moved);                 // candidates pre-generated for the next iteration used the old box list; a captured pair its address
    return MON_OK;
}

// ---- profiling helpers: HIP events on the train stream around each kernel class
static hipEvent_t get_event(Model& m) {
    if (!m.ev_pool.empty()) { hipEvent_t e = m.ev_pool.back(); m.ev_pool.pop_back(); return e; }
    hipEvent_t e; hipEventCreate(&e); return e;
}
// roctx ranges per phase (option "roctx" = 1): the phases of an iteration show up by name in a rocprofv3 --marker-trace of the host side.  The
// library is looked up at run time (librocprofiler-sdk-roctx.so, then libroctx64.so) -- nothing links against it, and without the option nothing is loaded.
struct Roctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    Roctx() {
        for (const char* lib : { "librocprofiler-sdk-roctx.so", "libroctx64.so" }) {
            void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL); if (!h) continue;
            push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA")); pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (push && pop) break;
            push = nullptr; pop = nullptr;
        }
    }
};
static Roctx* roctx() { if (!options().roctx) return nullptr; static Roctx r; return r.push ? &r : nullptr; }
static const char* const kPhaseName[MON_K_COUNT] = { "mon.batch (GenerateBatch)", "mon.fwd_bwd (k_fused_train)", "mon.optimizer (k_optimizer)", "mon.render",
        "mon.scatter (k_grid_scatter)", "mon.reduce_partials", "mon.encode (k_encode_tiles)", "mon.points (k_sample_points)" };
ProfScope::ProfScope(Model& mm, int c) : m(mm), cls(c), rx(roctx()) { if (rx) rx->push(kPhaseName[c]); if (m.profiling) { a = get_event(m); b = get_event(m);
        hipEventRecord(a, m.train_stream); } }
ProfScope::~ProfScope() { if (m.profiling) { hipEventRecord(b, m.train_stream); m.ev_pending.push_back({ cls, { a, b } }); } if (rx) rx->pop(); }
void collect_profile(Model& m) {
    for (auto& p : m.ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.second.first, p.second.second) == hipSuccess) { m.prof.ms[p.first] += ms; m.prof.launches[p.first] += 1; }
        m.ev_pool.push_back(p.second.first); m.ev_pool.push_back(p.second.second);
    }
    m.ev_pending.clear();
}

void mlp_forward_inference(Model& m, hipStream_t s, const uint16_t* params, const uint16_t* E, uint16_t* O, uint32_t n) {
    // (shapes outside the fused kernels: the whole-network MFMA forward, nothing but O written; a tail of fewer than 32 samples on the per-sample kernel)
    const uint32_t body = m.d_layers_T ? (n & ~31u) : 0u; uint32_t done = 0;
    if (body && launch_mlp_forward_layers(s, m.nd, params, E, nullptr, O, body, nullptr, nullptr)) done = body;
    if (done < n) launch_mlp_forward(s, m.nd, params, E + (size_t)done * m.nd.Epad, nullptr, O + (size_t)done * kOut, n - done, nullptr);
}

// Render of the latest PUBLISHED inference weights on the inference stream: callable from any thread while the owner trains (no model mutex,
// no train-stream work).  MON_ERR_STATE when nothing has been published yet (or the model has no inference side): the caller falls back to
// model_render under the model mutex.
int model_render_snapshot(Model& m, mon_frame_bbox box, const float* pose16, int pose_is_Toc, float* rgb, float* depth, float* mask, uint32_t* snapshot_step) {
    if (!pose16 || !rgb || !depth || !mask || box.w == 0 || box.h == 0) { set_error("render: bad argument"); return MON_ERR_ARG; }
    InferState* is = m.infer; if (!is) { set_error("render_snapshot: this object renders on its train stream"); return MON_ERR_STATE; }
    InferShared* sh = is->shared; std::lock_guard<std::mutex> one(sh->mu);      // one snapshot render per device at a time
    HIPCHECK(use_device(m.device));
    hipStream_t s = sh->stream;
    SnapshotPin pin;
    {   const int rc = pin.take(is, s);
        if (rc == MON_ERR_STATE) set_error("render_snapshot: no weights published yet");
        if (rc) return rc; }
    const int r = pin.r; if (snapshot_step) *snapshot_step = pin.step;
    Mat4 pose; std::memcpy(pose.m, pose16, 64);
    const uint32_t n_pix = box.w * box.h, S2 = 2 * m.oc.S;
    // one buffer of 5 floats per pixel: rgb | depth | mask laid out back to back for THIS crop, so one copy brings them home
    if (n_pix > is->out_cap) {
        const size_t cap = std::max<size_t>(n_pix, 2 * is->out_cap); void* q = nullptr;
        HIPCHECK(hipMalloc(&q, 20 * cap));
        is->grown.push_back(q);                                         // (freed with the object; the superseded ones are smaller than the live one)
        is->out_all = (float*)q; is->out_cap = cap;
    }
    is->out_rgb = is->out_all; is->out_depth = is->out_all + 3 * (size_t)n_pix; is->out_mask = is->out_all + 4 * (size_t)n_pix;
    // A viewer's render competes with the training kernels of every object on the device.  k_encode_feat's workgroups need a whole CU each (160 KB of LDS) and
    // wait until training workgroups have drained from one; the gather render's small workgroups slip in anywhere.  Measured (tools/online_replay.py,
    // 60 keyframes every 50 ms, mean / p99 of the viewer's crop): 1 object 0.85 / 1.13 ms on tiles against 1.20 / 1.93 ms through the gathers, 4 objects 0.51 / 2.0 against 0.68 / 1.7,
    // 12 objects 0.58 / 3.1 against 0.67 / 1.7 -- so the tiles serve the viewer while few objects live on the device, the gathers once many do
    // (tile_ws_objects counts the tile-capable objects ALIVE on the device: in the online manager every live object has a training thread).
    TileWs* tws = nullptr; std::unique_lock<std::mutex> tile_lock;
    const uint64_t ep = pin.epoch;
    // render skipping: the snapshot's own grid, built on this stream from the snapshot (stamp epoch_of[r]) through the side's fragment image
    const RenderSkipArgs sk = rskip_begin(m, is->rskip, s, m.rskip_on.load() != 0, m.rskip_alpha.load(), is->snap[r], ep, is->frag);
    // level tiles in LDS (kernels_tilerender.hip); the inference side's own workspace
    if (tile_render_wanted(m, n_pix) && (options().tile_render >= 2 || tile_ws_objects(m.device) <= 4)) {
        { const int rc = tile_ws_get(m, 1, n_pix, &tws); if (rc) return rc; }
        tile_lock = std::unique_lock<std::mutex>(tws->mu);                // (held until the stream is synchronised below)
        tile_ws_weights(m, *tws, s, is->snap[r], ep);
        { const int rc = tile_render_crop(m, *tws, s, m.oc, box, pose, pose_is_Toc, is->out_rgb, is->out_depth, is->out_mask, sk); if (rc) return rc; }
    } else {
        for (uint32_t p0 = 0; p0 < n_pix; p0 += kRenderChunkRays) {
            const uint32_t n = (n_pix - p0) < kRenderChunkRays ? (n_pix - p0) : kRenderChunkRays;
            launch_render_rays(s, is->rb, m.ds->K, m.oc, box, pose, pose_is_Toc, p0, n);
            launch_fused_render(s, m.lf, m.nd, is->snap[r], is->rb, m.oc, n, p0 * S2, is->out_rgb + 3 * (size_t)p0, is->out_depth + p0, is->out_mask + p0,
                    is->frag, p0 == 0u, sk);
        }
    }
    rskip_read(s, is->rskip);
    // results: through a PINNED staging buffer of the inference side.  A device-to-host copy into the caller's pageable memory is done by the runtime's own
    // blit path, which queues at normal priority behind every training kernel on the device (12 objects training: 5-6 ms for 1 MB, one render in five); into
    // pinned memory it is ordered on this high-priority stream.
    if (5 * (size_t)n_pix > sh->h_cap) {                                  // (a crop larger than a frame: not produced by the managers)
        float* q = nullptr; HIPCHECK(hipHostMalloc((void**)&q, 5 * (size_t)n_pix * sizeof(float), hipHostMallocDefault));
        if (sh->h_out) hipHostFree(sh->h_out);
        sh->h_out = q; sh->h_cap = 5 * (size_t)n_pix;
    }
    // (a copy KERNEL on this stream writing the pinned buffer over PCIe, not hipMemcpyAsync: the runtime's copy path has its own queueing, 1-2 ms on a device
    //  busy with a dozen training objects, while a kernel inherits the stream's priority like the render kernels before it)
    launch_copy_params(s, reinterpret_cast<const uint16_t*>(is->out_all), reinterpret_cast<uint16_t*>(sh->h_out), (uint32_t)(10 * (size_t)n_pix));
    HIPCHECK(hipStreamSynchronize(s));
    HIPCHECK(hipGetLastError());
    rskip_end(is->rskip);
    std::memcpy(rgb, sh->h_out, 12 * (size_t)n_pix); std::memcpy(depth, sh->h_out + 3 * (size_t)n_pix, 4 * (size_t)n_pix);
    std::memcpy(mask, sh->h_out + 4 * (size_t)n_pix, 4 * (size_t)n_pix);
    return MON_OK;
}

// Render / RenderVideo body :1768-1828, chunked; inference (EMA) weights once training has run.
// Lazy EMA: apply the steps untouched chunks sat out before the inference weights are read.
int ensure_ema_current(Model& m) {
    if (!m.ema_pending) return MON_OK;
    HIPCHECK(use_device(m.device)); model_leave_lane(m);
    ParamPtrs P = m.P; P.ema_step = m.d_ema_step; P.lazy = 1;
    launch_ema_finalize(m.train_stream, P, m.opt, m.d_state);
    HIPCHECK(hipGetLastError()); m.ema_pending = false; m.weights_epoch = next_weights_epoch(); return MON_OK;
}

int model_render(Model& m, mon_frame_bbox box, const float* pose16, int pose_is_Toc, float* rgb, float* depth, float* mask, int dst_on_device) {
    if (!pose16 || !rgb || !depth || !mask || box.w == 0 || box.h == 0) { set_error("render: bad argument"); return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device));
    model_leave_lane(m);
    { int rc = ensure_ema_current(m); if (rc) return rc; }
    hipStream_t s = m.train_stream;
    // (no state read-back: every call that advances the optimizer ends with sync_state, so the host's copy of the step counter is current whenever this thread
    // gets here -- the read-back and the synchronisation in front of it were two host round trips per render)
    const uint16_t* prm = (m.h_state.step > 0) ? m.P.ema : m.P.half;
    Mat4 pose; std::memcpy(pose.m, pose16, 64);
    const uint32_t n_pix = box.w * box.h, S2 = 2 * m.oc.S;
    // whole-crop output buffer (grow-only): all chunks are enqueued back to back, one copy-out and one sync per call
    if (n_pix > m.out_cap) {
        // doubling: the superseded buffers (freed with the object) add up to less than the live one
        const size_t cap = std::max<size_t>(n_pix, 2 * m.out_cap);
        int rc; if ((rc = dev_alloc(m, m.d_out_all, 5 * cap, false))) return rc;
        m.out_cap = cap;
    }
    // rgb | depth | mask of THIS crop, back to back
    m.d_out_rgb = m.d_out_all; m.d_out_depth = m.d_out_all + 3 * (size_t)n_pix; m.d_out_mask = m.d_out_all + 4 * (size_t)n_pix;
    if (!dst_on_device && 5 * (size_t)n_pix > m.h_out_cap) {          // pinned staging: one device-to-host copy instead of three into pageable memory
        const size_t cap = std::max<size_t>(5 * (size_t)n_pix, 2 * m.h_out_cap); float* q = nullptr;
        HIPCHECK(hipHostMalloc((void**)&q, cap * sizeof(float), hipHostMallocDefault));
        if (m.h_out) (void)hipHostFree(m.h_out);
        m.h_out = q; m.h_out_cap = cap;
    }
    if (m.d_xw) {          // XORWOW mode: a NEW generator per Render (default seed) draws the whole crop's RandDt in one call (nerf_model.cu:1725-1728, :1781)
        const size_t need = (size_t)n_pix * S2;
        if (need > m.xw_render_cap) { int rc = dev_alloc(m, m.d_xw_render, need, false); if (rc) return rc; m.xw_render_cap = need; }
        HIPCHECK(hipMemcpyAsync(m.d_xw_render_states, m.d_xw_render_init, sizeof(XorwowState) * m.xw_lanes, hipMemcpyDeviceToDevice, s));
        launch_xorwow_fill(s, m.d_xw_render_states, m.xw_lanes, m.xw_flavour, 0u, m.d_xw_render, (uint32_t)need, nullptr, 0u, nullptr, 0u);
        m.oc.xw_render = m.d_xw_render;
    }
    TileWs* tws = nullptr; std::unique_lock<std::mutex> tile_lock;
    // render skipping (fused backend only): the train side's grid of the weights rendered, through the side's fragment image (d_frag_render)
    RenderSkipArgs sk; m.rskip.active = false;
    if (m.backend == 1 && m.rskip_on.load() != 0) { ProfScope ps(m, MON_K_RENDER);
        sk = rskip_begin(m, m.rskip, s, true, m.rskip_alpha.load(), prm, m.weights_epoch, m.d_frag_render); }
    // level tiles in LDS (kernels_tilerender.hip), the device's train-side workspace: held until the stream is synchronised below
    if (tile_render_wanted(m, n_pix)) {
        { const int rc = tile_ws_get(m, 0, n_pix, &tws); if (rc) return rc; }
        tile_lock = std::unique_lock<std::mutex>(tws->mu);
        ProfScope ps(m, MON_K_RENDER);
        tile_ws_weights(m, *tws, s, prm, m.weights_epoch);
        { const int rc = tile_render_crop(m, *tws, s, m.oc, box, pose, pose_is_Toc, m.d_out_rgb, m.d_out_depth, m.d_out_mask, sk); if (rc) return rc; }
    } else
    {
      // rays per pass: the fused kernel takes kRenderChunkRays; the layer-at-a-time kernels what their sample buffers hold
      const uint32_t pass = m.backend == 0 ? std::max(1u, std::min(kRenderChunkRays, m.ws_samples / S2)) : kRenderChunkRays;
      for (uint32_t p0 = 0; p0 < n_pix; p0 += pass) {
        const uint32_t n = (n_pix - p0) < pass ? (n_pix - p0) : pass;
        ProfScope ps(m, MON_K_RENDER);
        launch_render_rays(s, m.B, m.ds->K, m.oc, box, pose, pose_is_Toc, p0, n);
        if (m.backend == 0) {
            launch_gen_samples(s, m.B, m.oc, m.d_state, S2, n * S2, kStreamRender, p0 * S2, 1);
            launch_encode(s, m.lt, m.nd, prm, m.B.pts, m.B.E, n * S2, nullptr);
            mlp_forward_inference(m, s, prm, m.B.E, m.B.O, n * S2);
            launch_composite_render(s, m.B, S2, n, m.d_out_rgb + 3 * (size_t)p0, m.d_out_depth + p0, m.d_out_mask + p0);
        } else {
            launch_fused_render(s, m.lf, m.nd, prm, m.B, m.oc, n, p0 * S2, m.d_out_rgb + 3 * (size_t)p0, m.d_out_depth + p0, m.d_out_mask + p0,
                    m.d_frag_render, p0 == 0u, sk);
        }
      }
    }
    rskip_read(s, m.rskip);
    if (dst_on_device) {
        HIPCHECK(hipMemcpyAsync(rgb, m.d_out_rgb, 12 * (size_t)n_pix, hipMemcpyDeviceToDevice, s));
        HIPCHECK(hipMemcpyAsync(depth, m.d_out_depth, 4 * (size_t)n_pix, hipMemcpyDeviceToDevice, s));
        HIPCHECK(hipMemcpyAsync(mask, m.d_out_mask, 4 * (size_t)n_pix, hipMemcpyDeviceToDevice, s));
        HIPCHECK(hipStreamSynchronize(s));
    } else {
        HIPCHECK(hipMemcpyAsync(m.h_out, m.d_out_all, 20 * (size_t)n_pix, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        std::memcpy(rgb, m.h_out, 12 * (size_t)n_pix); std::memcpy(depth, m.h_out + 3 * (size_t)n_pix, 4 * (size_t)n_pix);
        std::memcpy(mask, m.h_out + 4 * (size_t)n_pix, 4 * (size_t)n_pix);
    }
    HIPCHECK(hipGetLastError());
    rskip_end(m.rskip);
    collect_profile(m);
    return MON_OK;
}

// GetDensityOnGrid :2007-2048
int model_density_grid(Model& m, int rx, int ry, int rz, float* out_host) {
    if (rx < 2 || ry < 2 || rz < 2 || !out_host || (uint64_t)rx * (uint64_t)ry * (uint64_t)rz > (1ull << 31)) { set_error("density_grid: bad argument");
        return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device));
    model_leave_lane(m);
    { int rc = ensure_ema_current(m); if (rc) return rc; }
    hipStream_t s = m.train_stream;
    HIPCHECK(hipStreamSynchronize(s));
    // (the head: the slot counters behind it are 16 KB the host never reads)
    HIPCHECK(hipMemcpy(&m.h_state, m.d_state, offsetof(DevState, n_scatter), hipMemcpyDeviceToHost));
    const uint16_t* prm = (m.h_state.step > 0) ? m.P.ema : m.P.half;
    const uint32_t total = (uint32_t)rx * ry * rz, chunk = m.ws_samples;
    if (m.backend == 1 && m.plan.tile_render && options().tile_render != 0) {      // level tiles in LDS: the device's train-side workspace
        TileWs* ws = nullptr; { const int rc = tile_ws_get(m, 0, 0, &ws); if (rc) return rc; }
        std::lock_guard<std::mutex> wl(ws->mu);
        tile_ws_weights(m, *ws, s, prm, m.weights_epoch);
        const uint32_t tchunk = std::min(ws->cap, m.ws_samples);
        for (uint32_t p0 = 0; p0 < total; p0 += tchunk) {
            const uint32_t n = std::min(total - p0, tchunk);
            launch_grid_points4(s, ws->x, rx, ry, rz, p0, n);
            tile_points_forward(m, *ws, s, n);
            launch_extract_density(s, ws->O, m.B.tdist, n);
            HIPCHECK(hipMemcpyAsync(out_host + p0, m.B.tdist, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipStreamSynchronize(s));
        }
        return MON_OK;
    }
    for (uint32_t p0 = 0; p0 < total; p0 += chunk) {
        const uint32_t n = (total - p0) < chunk ? (total - p0) : chunk;
        launch_grid_points(s, m.B.pts, rx, ry, rz, p0, n);
        launch_encode(s, m.lt, m.nd, prm, m.B.pts, m.B.E, n, nullptr);
        mlp_forward_inference(m, s, prm, m.B.E, m.B.O, n);
        launch_extract_density(s, m.B.O, m.B.tdist, n);
        HIPCHECK(hipMemcpyAsync(out_host + p0, m.B.tdist, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    }
    return MON_OK;
}

// ---- render skipping: the switch, its statistics, the grids
bool rskip_supported(const Model& m) { return m.backend == 1 && m.plan.fused; }
int model_set_render_skip(Model& m, int enable, float min_alpha) {
    if (!rskip_supported(m)) { set_error("set_render_skip: this object does not run on the fused kernels (layer-kernel backend)"); return MON_ERR_STATE; }
    if (!(min_alpha < 1.0f)) { set_error("set_render_skip: min_alpha must be < 1"); return MON_ERR_ARG; }
    if (enable) {      // (the buffers of both sides are allocated here, by the owner: a viewer thread never allocates into the object)
        HIPCHECK(use_device(m.device));
        int rc; if ((rc = rskip_alloc(m, m.rskip)) || (m.infer && (rc = rskip_alloc(m, m.infer->rskip)))) return rc;
    }
    m.rskip_alpha.store(min_alpha); m.rskip_on.store(enable != 0); return MON_OK;
}
// the side's state under the lock that orders it against that side's renders (side 1: the device's snapshot-render mutex)
template <class F> static int rskip_with_side(Model& m, int side, const char* what, F&& f) {
    if (side == 0) return f(m.rskip);
    if (side != 1) { set_error("%s: side must be 0 or 1", what); return MON_ERR_ARG; }
    if (!m.infer) { set_error("%s: this object has no inference side", what); return MON_ERR_STATE; }
    std::lock_guard<std::mutex> l(m.infer->shared->mu); return f(m.infer->rskip);
}
int model_render_skip_stats(Model& m, int side, mon_render_skip_stats* out) {
    if (!out) { set_error("render_skip_stats: null out"); return MON_ERR_ARG; }
    return rskip_with_side(m, side, "render_skip_stats", [&](RenderSkipSide& k) {
        mon_render_skip_stats st{}; st.active = k.active ? 1u : 0u; st.grid_builds = k.builds;
        if (k.active) {
            st.samples_in_box = k.samples_in_box; st.samples_live = k.samples_live;
            std::vector<uint32_t> g(kOccWords);
            HIPCHECK(use_device(m.device)); HIPCHECK(hipMemcpy(g.data(), k.d_grid, kOccWords * 4, hipMemcpyDeviceToHost));      // (the render synchronised)
            for (uint32_t w : g) st.live_cells += (uint32_t)__builtin_popcount(w);
        }
        *out = st; return MON_OK;
    });
}
int model_render_occupancy(Model& m, int side, int dilated, uint32_t* bits) {
    if (!bits) { set_error("render_occupancy: null bits"); return MON_ERR_ARG; }
    return rskip_with_side(m, side, "render_occupancy", [&](RenderSkipSide& k) {
        if (!k.built && !k.pinned) { set_error("render_occupancy: no skipping render on this side yet"); return MON_ERR_STATE; }
        HIPCHECK(use_device(m.device)); HIPCHECK(hipMemcpy(bits, dilated || k.pinned ? k.d_grid : k.d_raw, kOccWords * 4, hipMemcpyDeviceToHost));
        return MON_OK;
    });
}
int model_debug_set_render_grid(Model& m, int side, const uint32_t* bits) {
    if (!rskip_supported(m)) { set_error("debug_set_render_grid: this object does not run on the fused kernels"); return MON_ERR_STATE; }
    HIPCHECK(use_device(m.device));
    { int rc; if ((rc = rskip_alloc(m, m.rskip)) || (m.infer && (rc = rskip_alloc(m, m.infer->rskip)))) return rc; }
    return rskip_with_side(m, side, "debug_set_render_grid", [&](RenderSkipSide& k) {
        if (bits) { HIPCHECK(hipMemcpy(k.d_grid, bits, kOccWords * 4, hipMemcpyHostToDevice)); HIPCHECK(hipMemcpy(k.d_raw, bits, kOccWords * 4,
                hipMemcpyHostToDevice)); k.pinned = true; }
        else { k.pinned = false; k.built = false; }          // the object's own grid is rebuilt by the next skipping render
        return MON_OK;
    });
}

bool model_has_snapshot(Model& m) {
    if (!m.infer) return false;
    std::lock_guard<std::mutex> l(m.infer->mu); return m.infer->latest >= 0;
}

// ---- storing an object pose (mon_object_set_pose): oc.Tow and nothing else.  Weights, optimizer state, counters, the occupancy grid and the render-skip grids
// live in the object frame and stay; what was built under the old pose -- the candidate rays prepared for the coming iteration, a captured graph (its kernel
// arguments hold oc by value) -- is dropped.
int model_set_pose(Model& m, const float* Tow16) {
    if (!Tow16) { set_error("set_pose: null Tow16"); return MON_ERR_ARG; }
    for (int k = 0; k < 16; ++k) if (!std::isfinite(Tow16[k])) { set_error("set_pose: Tow16[%d] is not finite", k); return MON_ERR_ARG; }
    if (m.scatter_pending) { set_error("set_pose: between the stages of an iteration (mon_object_train_stages)"); return MON_ERR_STATE; }
    HIPCHECK(use_device(m.device));
    {   // side 1 calls read oc.Tow under the device's inference lock, from any thread: the pose changes under it, between two of them
        std::unique_lock<std::mutex> infer_lock;
        if (m.infer && m.infer->shared) infer_lock = std::unique_lock<std::mutex>(m.infer->shared->mu);
        std::memcpy(m.oc.Tow.m, Tow16, 64);
    }
    model_mark_stale(m, kStaleRays, true);
    return MON_OK;
}

int model_get_params(Model& m, int which, void* dst, size_t bytes) {
    const void* src = nullptr; size_t need = 0;
    if (which == 0 && m.P.rec) {                             // chunk records: the master weights through a staging buffer
        if (!dst || bytes < (size_t)m.n_params * 4) { set_error("get_params: buffer too small"); return MON_ERR_ARG; }
        HIPCHECK(use_device(m.device)); model_leave_lane(m);
        float* tmp = nullptr; HIPCHECK(hipMalloc((void**)&tmp, (size_t)m.n_params * 4));
        launch_state_unpack(m.train_stream, m.P.rec, 0, tmp, m.n_params);
        hipError_t e = hipStreamSynchronize(m.train_stream); if (e == hipSuccess) e = hipMemcpy(dst, tmp, (size_t)m.n_params * 4, hipMemcpyDeviceToHost);
        (void)hipFree(tmp); HIPCHECK(e); return MON_OK;
    }
    switch (which) { case 0: src = m.P.master; need = (size_t)m.n_params * 4; break; case 1: src = m.P.half; need = (size_t)m.n_params * 2; break;
                     case 2: src = m.P.ema; need = (size_t)m.n_params * 2; break; default: set_error("get_params: which must be 0..2"); return MON_ERR_ARG; }
    if (!dst || bytes < need) { set_error("get_params: buffer too small (%zu < %zu)", bytes, need); return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device)); model_leave_lane(m);
    if (which == 2) { int rc = ensure_ema_current(m); if (rc) return rc; }
    HIPCHECK(hipStreamSynchronize(m.train_stream));
    HIPCHECK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost)); return MON_OK;
}
int model_set_params(Model& m, const float* master, size_t n) {
    if (!master || n != m.n_params) { set_error("set_params: expected %u values", m.n_params); return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device)); model_leave_lane(m); HIPCHECK(hipStreamSynchronize(m.train_stream));
    { const int urc = upload_master(m, master); if (urc) return urc; }
    HIPCHECK(hipStreamSynchronize(m.train_stream));
    model_mark_stale(m, kStaleWeights);                     // the fragment image and the tile image no longer match the weights
    m.weights_epoch = next_weights_epoch();
    { const int rc = publish_snapshot(m); if (rc) return rc; }   // (viewers of an untrained object see the weights just set:
    // the snapshot is complete before the call returns, so no render prefers the one before it)
    HIPCHECK(hipStreamSynchronize(m.train_stream)); return MON_OK;
}

}  // namespace mon
