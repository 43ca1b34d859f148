// model_internal.h -- what model.cpp, train.cpp, pose.cpp, scene.cpp, scene_field.cpp, dist_field.cpp, scene_pose.cpp and checkpoint.cpp need from each other and nobody else needs (c_api.cpp, manager.cpp and
// diag.cpp go through model.h).
#pragma once
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <vector>
#include "model.h"

namespace mon {

#define HIPCHECK(expr)                                                                                         \
    do { hipError_t _e = (expr); if (_e != hipSuccess) {                                                       \
        set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); return MON_ERR_HIP; } } while (0)
// a NULL pointer argument of a route's check, by the name the header gives it: "<what>: null <name>"
#define REQUIRE_ARG(what, p, name) do { if (!(p)) { set_error("%s: null %s", what, name); return MON_ERR_ARG; } } while (0)
constexpr uint32_t kRenderChunkRays = 16384;   // rays per render pass (x 2S samples)

// One high-priority stream and one pinned result buffer per DEVICE, shared by the objects on it (viewer renders) and by the device's dataset (frame uploads):
// created with the device's first object (CreateNeRF is a
// milliseconds call anyway; created by the first render it was a 10 ms spike in front of the viewer), and only one more hardware-queue client however many
// objects train (a high-priority queue per object measurably slowed sliced training).  Renders of one device take turns on it.
// h_cap only grows; h_out / growth belong to mu
struct InferShared { std::mutex mu; hipStream_t stream = nullptr; float* h_out = nullptr; std::atomic<size_t> h_cap{ 0 }; };

// ---- inference side of a model (the reference's second stream, nerf_model.cu:1268-1269).  The training thread PUBLISHES the inference weights
// at the end of every train call / online slice: a device-to-device copy into one of two snapshot buffers, ordered on the train stream, with an
// event.  A viewer thread renders from the latest published snapshot on the inference stream (created with the highest priority) and in a
// workspace of its own: it takes no model mutex, never touches the train stream, and its kernels do not queue behind training slices.
struct InferState {
    InferShared* shared = nullptr;                                      // the device's inference stream (highest priority) and pinned result buffer
    uint16_t* snap[2] = { nullptr, nullptr }; hipEvent_t ready[2] = { nullptr, nullptr }; uint32_t step_of[2] = { 0, 0 }; bool written[2] = { false, false };
    int latest = -1, readers[2] = { 0, 0 }; std::mutex mu;              // which snapshot is current, who is reading which
    // weights stamp of each snapshot (next_weights_epoch at publication: the tile render's image key)
    uint64_t epoch_of[2] = { 0, 0 };
    std::atomic<bool> wanted{ false }; std::chrono::steady_clock::time_point last_pub{};      // a viewer asked since the last publication; when that was
    BatchPtrs rb{}; float *out_all = nullptr, *out_rgb = nullptr, *out_depth = nullptr, *out_mask = nullptr; size_t out_cap = 0; uint16_t* frag = nullptr;
    std::vector<void*> grown;                                           // superseded output buffers, freed with the object
    RenderSkipSide rskip;                                               // render skipping of the snapshot renders (under shared->mu, on its stream)
};

// The published snapshot a side-1 call reads, pinned (readers[r], which keeps publish_snapshot off the buffer) from take() until the pin goes: on every way
// out of the call.  take() also tells the training side that a viewer asked (it refreshes the snapshot at the end of its current slice) and orders the
// snapshot's copy in front of the caller's stream `s`.  Which snapshot:
// the newest snapshot's copy may still be queued behind other objects' training kernels (it runs on the train stream, at normal priority: 1-2 ms on a
// busy device); the one before it is complete, and nobody writes it before the train stream has been synchronised again -- by which time the newest is
// complete and chosen here.  A viewer prefers a finished snapshot one slice older to waiting.
struct SnapshotPin {
    InferState* held = nullptr; int r = -1; uint32_t step = 0; uint64_t epoch = 0;      // step_of[r], epoch_of[r]: neither changes while the pin is held
    SnapshotPin() = default; SnapshotPin(const SnapshotPin&) = delete; SnapshotPin& operator=(const SnapshotPin&) = delete;
    // MON_ERR_STATE, with nothing pinned, while nothing has been published
    int take(InferState* is, hipStream_t s) {
        is->wanted.store(true);
        {   std::lock_guard<std::mutex> l(is->mu); r = is->latest; if (r < 0) { set_error("no weights published yet"); return MON_ERR_STATE; }
            if (is->written[1 - r] && hipEventQuery(is->ready[r]) != hipSuccess && hipEventQuery(is->ready[1 - r]) == hipSuccess) r = 1 - r;
            ++is->readers[r]; held = is; step = is->step_of[r]; epoch = is->epoch_of[r]; }
        HIPCHECK(hipStreamWaitEvent(s, is->ready[r], 0));
        return MON_OK;
    }
    const uint16_t* snap() const { return held->snap[r]; }
    ~SnapshotPin() { if (held) { std::lock_guard<std::mutex> l(held->mu); --held->readers[r]; } }
};

// Grow-only scratch in device memory (Pinned: in pinned host memory): growth frees and allocates, the contents are not carried over; freed with its owner.
template <class T, bool Pinned = false> struct DevBuf {
    T* p = nullptr; size_t cap = 0;
    DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    void release() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; cap = 0; }
    int grow(size_t n) {
        if (n <= cap && p) return MON_OK;
        release();
        HIPCHECK(Pinned ? hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, n * sizeof(T))); cap = n; return MON_OK;
    }
    ~DevBuf() { release(); }
};
template <class T> using PinnedBuf = DevBuf<T, true>;

// device memory that lives as long as the object (freed by model_destroy)
template <class T> int dev_alloc(Model& m, T*& p, size_t n, bool zero = true) {
    void* q = nullptr; const size_t bytes = (n ? n : 1) * sizeof(T);
    HIPCHECK(hipMalloc(&q, bytes));
    if (zero) HIPCHECK(hipMemset(q, 0, bytes));
    m.allocs.push_back(q); p = (T*)q; return MON_OK;
}
// train.cpp: the device's training lanes (made with its dataset), the objects counted on them; a captured pair of iterations
struct TrainLanes* lanes_get(int device);
void lanes_objects_add(struct TrainLanes* t, int n);
void drop_graph(Model& m);
// profiling (model.cpp): HIP events on the train stream around each kernel class (mon_object_set_profiling) and a roctx range per phase (option roctx)
struct ProfScope { Model& m; int cls; hipEvent_t a = nullptr, b = nullptr; struct Roctx* rx; ProfScope(Model& mm, int c); ~ProfScope(); };
void collect_profile(Model& m);

bool rskip_supported(const Model& m);          // the object runs on the fused kernels
// the side's grid of `prm` (stamp `epoch`) on stream s: the cached one, or built through the training grid's kernels into `frag`, the side's fragment image
// of the same weights; nullptr when the side has no grid buffers
const uint32_t* rskip_grid(Model& m, RenderSkipSide& k, hipStream_t s, float alpha, const uint16_t* prm, uint64_t epoch, uint16_t* frag);
int config_check(const mon_config& cfg);       // what mon_object_create rejects before the level table is built
bool steps16_exact(const mon_config& cfg);     // model_init's rule for the step counters; a checkpoint records which one its object kept
// init_params = false (model_load): the parameters are left for the caller to stream in -- nothing of table size is staged
int model_create_impl(Dataset* ds, const mon_config& cfg, int class_id, const float* Tow, const float* amin, const float* amax, bool init_params, Model** out);
int publish_snapshot(Model& m, bool force = true);
struct MeshState* mesh_state_create(int device); void model_mesh_free(Model& m);      // mesh.cpp
void pose_ws_free(Model& m);                   // pose.cpp: the object's pose refinement scratch
// pose.cpp: box i of a pose call names a frame the dataset holds and lies inside it; its pixels join `total` (at most 64 kPoseMaxRays).  `what`: the message
// prefix ("pose", "scene pose")
int pose_box_check(const char* what, const Dataset& ds, const mon_frame_bbox& b, size_t i, uint64_t& total);

// ---- scene.cpp: what the files of the scene routes (scene.cpp, scene_field.cpp, scene_pose.cpp) share
int side_check(const char* what, int side);
// every MON_ERR_STATE of a scene call that needs no device work (the routes run it themselves: it is their own question, asked once).  lists = false (the
// field queries): nothing is sampled or jittered, so neither the sample count nor the XORWOW render mode matters
int scene_state_check(const char* what, Model* const* ms, size_t n, int side, bool lists = true);
// Entering a side of a scene: the weights every object is read from, their stamps, the stream of the call.  Side 1: the shared inference stream under
// its device lock, every object's snapshot pinned.  Side 0: the train side as model_render picks it (EMA once trained, brought up to date), object 0's train
// stream after every object's pending work (the workspace's events `ev`).  Lock order: the device's inference lock, then the workspace's `ws_mu`;
// InferState::mu only inside SnapshotPin::take.  Holds the locks and the pins until it goes (after the call's stream has been synchronised).
struct SceneSide {
    hipStream_t s = nullptr; std::vector<const uint16_t*> prm; std::vector<uint64_t> epoch;
    std::unique_lock<std::mutex> dev_lock; std::vector<SnapshotPin> pins; std::unique_lock<std::mutex> ws_lock;
    int enter(Model* const* ms, size_t n, int side, std::mutex& ws_mu, std::vector<hipEvent_t>& ev);
};
// the workspace of type W of a device and side: made on first use, never freed
template <class W> W& side_ws(int device, int side) {
    static std::mutex mu; static std::map<std::pair<int, int>, W*> all;
    std::lock_guard<std::mutex> l(mu); W*& w = all[{ device, side }]; if (!w) w = new W(); return *w;
}
// The workspace of the render, the list routes and the field queries (the lattice routes' shared stages, scene_field.cpp, own docc, dv and dsite).  Per device and side, grow-only, never freed (like the tile workspaces): the lists of
// one chunk for every object, the call's outputs, their pinned staging, the events that order the objects' streams in front of side 0's call.  A call holds
// `mu` until its stream has been synchronised, so the routes of one side take turns.
struct SceneWs {
    std::mutex mu;
    DevBuf<float> t, attr; DevBuf<uint32_t> cnt;                                  // [lists][cap][kSceneListLen] t, float4 attr; [lists][cap]
    DevBuf<float> out; PinnedBuf<float> h_out;                                    // rgb 3n | depth n | opacity n | instance n (int32)
    DevBuf<mon_scene_query> q; DevBuf<float> poses; DevBuf<uint32_t> keys;        // scene_probe: the queries, the poses [n_poses][16], a pass's keys [cap]
    DevBuf<mon_scene_ray> rays; DevBuf<float> entry;                              // scene_cast: the rays, a pass's box entries [lists][cap]
    DevBuf<float> pts, rows;                                                      // field queries: the points [n][3], a pass's rows [objects][cap][12 or 16]
    DevBuf<uint16_t> gfrag; DevBuf<float> lw; DevBuf<int32_t> sel;                // gradients (rows of 16): full fragment images, weights [Lmax], select [n]
    DevBuf<uint8_t> docc; DevBuf<float> dv; DevBuf<int32_t> dsite;                // lattice routes: the mask [n], the passes' squared distances and sites [2][n] (the signed routes: [4][n])
    DevBuf<uint32_t> cscan;                                                       // scene_components: the numbering's block sums (its mask is docc)
    DevBuf<float> pcost, pmul; DevBuf<int32_t> pseeds; DevBuf<uint8_t> pflags;    // scene_paths: the working cost [n], the multiplier [n], the seeds, two flag
    DevBuf<uint32_t> praised; PinnedBuf<uint32_t> h_raised;                       // bytes per tile, a batch's "left work" words and their pinned copy (mask: docc)
    std::vector<hipEvent_t> ev;
};
// what each object renders with on a side; bits: its render grid (nullptr: none, or a call that consults no skipping)
struct SceneSrc { BatchPtrs* b; uint16_t* frag; const uint32_t* bits; };
// One call of a route over SceneWs, from its state check to its synchronisation.  enter: the state check, the device, the side's workspace and its locks
// (SceneSide), every object's sources -- lists: the render, the probe and the cast, whose render grids are the objects' own per-side caches, built if stale
// (their skip counters stay as they are); not lists: the field queries, which look at no grid.  grow_lists: the list workspace of `cap` rays per object.
// finish: one synchronisation and the launches' error; home: ws.out's first `floats` to the pinned staging (a copy kernel on the call's stream, as the
// snapshot render does), then finish.  The locks go with the object, after that.
struct SceneCall {
    SceneWs* ws = nullptr; SceneSide sd; std::vector<SceneSrc> src; hipStream_t s = nullptr;
    int enter(const char* what, Model* const* ms, size_t n, int side, bool lists);
    int grow_lists(size_t n, uint32_t cap);
    int finish();
    int home(size_t floats);
};
// dist_field.cpp: a distance field on the device (scene_field.cpp fills the cells and max_value of the one dist_field_adopt made)
struct DistField {
    std::mutex mu;
    int device = 0; Lattice g; float max_value = 0.f;
    float* cells = nullptr; hipStream_t s = nullptr;
    DevBuf<float> in, out; PinnedBuf<float> h_out;                                   // a call's inputs, its outputs and their pinned staging
};
// scene_field.cpp: a lattice of at least one cell per axis and at most max_cells in all (the lattice routes; dist_field.cpp's handles)
int lattice_dims_check(const char* what, int nx, int ny, int nz, size_t max_cells);
// an instance row home: the call's list indices, or the caller's ids for them
void scene_instances_home(int32_t* out, const float* row, size_t n, const int32_t* ids);
// A call's output area on the device (a scene route's in ws.out, a handle call's in its `out`), described once: pieces taken in order, whose offsets serve
// the device pointers the kernels get and the unpacking from the pinned staging alike.  row: `width` floats per point.  piece: `floats` floats the caller may
// ask for -- host: where they go (nullptr: not asked for; the room is taken all the same, so a call that gives such a piece no room passes 0 floats),
// instance: by way of scene_instances_home.  out: a piece that is a row.  keep: words the route itself reads at home.  `home`: the front of the area up to
// the last piece asked for or kept, all a scene route brings home; unpack: the pieces asked for, out of the staging.
struct Area {
    struct Out { size_t at, floats; void* host; bool instance; };
    size_t n_q = 0, end = 0, home = 0; Out outs[8]; int n_outs = 0;
    size_t take(size_t floats) { const size_t at = end; end += floats; return at; }
    size_t row(size_t width = 1) { return take(width * n_q); }
    size_t keep(size_t floats) { const size_t at = take(floats); home = end; return at; }
    size_t piece(void* host, size_t floats, bool instance = false) {
        const size_t at = take(floats);
        if (host) { home = end; outs[n_outs++] = Out{ at, floats, host, instance }; }
        return at;
    }
    size_t out(void* host, size_t width = 1, bool instance = false) { return piece(host, width * n_q, instance); }
    void unpack(const float* h, const int32_t* ids) const {
        for (int k = 0; k < n_outs; ++k) {
            const Out& o = outs[k];
            if (o.instance) scene_instances_home(static_cast<int32_t*>(o.host), h + o.at, n_q, ids); else std::memcpy(o.host, h + o.at, 4 * o.floats);
        }
    }
};

}  // namespace mon
