// trace_driver.cpp -- walks the C ABI single-threaded on the host side built --offload-host-only against tests/tsan/hip_stub.cpp (no sanitizer) with the
// stub's launch trace on: every kernel launch and asynchronous fill / copy of every training path as one line of text, under a heading per case and per call.
// tests/test_launch_trace.py compares the output with tests/golden/launch_trace.txt.  Usage: trace_driver <scratch dir> <config json>.  TEST INFRASTRUCTURE.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include <mon_core.h>

extern "C" void hip_stub_trace(int on);

#define OK(expr) do { const int rc_ = (expr); \
        if (rc_ != MON_OK) { std::fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, mon_last_error()); std::exit(3); } } while (0)
// a call under its own heading
#define CALL(expr) do { std::printf("-- %s\n", #expr); OK(expr); } while (0)

static const int H = 48, W = 64, kFrames = 16;
static float g_pose[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, -2, 1 }, g_Tow[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
static const float g_amin[3] = { -0.3f, -0.3f, -0.3f }, g_amax[3] = { 0.3f, 0.3f, 0.3f };
static std::string g_dir;
struct Opt { const char* name; long value; };

// A train call publishes a weight snapshot when a viewer has asked since the last one or 10 ms have passed: a viewer asks before every call (untraced), so
// that the publication's copy is in the trace whatever the clock says
static void viewer_asks(mon_object* o) {
    float c[3 * 16], d[16], m[16]; uint32_t step = 0;
    hip_stub_trace(0); (void)mon_object_render_snapshot(o, mon_frame_bbox{ 0, 8, 8, 4, 4 }, g_pose, 0, c, d, m, &step); hip_stub_trace(1);
}
#define TRAIN(o, n) do { viewer_asks(o); CALL(mon_object_train(o, n, &loss)); } while (0)

static void train_calls(mon_object* o) {
    float loss = 0.f;
    TRAIN(o, 3); CALL(mon_object_train_stages(o, 1)); CALL(mon_object_train_stages(o, 1 | 2)); CALL(mon_object_train_stages(o, 4));
    CALL(mon_object_train_stages(o, 2 | 4));
}
// everything that marks prepared work stale, each followed by one iteration
static void stale_calls(mon_object* o, bool fused) {
    float loss = 0.f;
    const mon_frame_bbox one{ 1, 8, 8, 24, 32 }; std::vector<mon_frame_bbox> many(1100, mon_frame_bbox{ 2, 4, 4, 16, 16 });
    CALL(mon_object_add_boxes(o, &one, 1)); TRAIN(o, 1);                       // within the box list's capacity (1024)
    CALL(mon_object_add_boxes(o, many.data(), many.size())); TRAIN(o, 1);      // past it: the list moves
    mon_object_info info; OK(mon_object_info_get(o, &info)); std::vector<float> master(info.n_params, 0.01f);
    CALL(mon_object_set_params(o, master.data(), master.size())); TRAIN(o, 1);
    float Tow[16]; std::memcpy(Tow, g_Tow, 64); Tow[12] = 0.01f;
    CALL(mon_object_set_pose(o, Tow)); TRAIN(o, 1);
    CALL(mon_object_set_backend(o, 0)); TRAIN(o, 2);
    if (fused) { CALL(mon_object_set_backend(o, 1)); TRAIN(o, 2); }
    CALL(mon_object_set_debug_dump(o, 1)); TRAIN(o, 1); CALL(mon_object_set_debug_dump(o, 0)); TRAIN(o, 1);
}
// a checkpoint save and load, then one iteration of the loaded object
static void checkpoint_calls(mon_dataset* ds, mon_object*& o) {
    float loss = 0.f;
    const std::string path = g_dir + "/trace_object.ckpt";
    CALL(mon_object_save(o, path.c_str()));
    mon_object* o2 = nullptr; std::printf("-- mon_object_load\n"); OK(mon_object_load(ds, path.c_str(), MON_LOAD_BOXES, &o2));
    OK(mon_object_destroy(o)); o = o2;
    TRAIN(o, 1);
}

// walk: 0 the train calls | 1 + every call that marks prepared work stale | 2 + a checkpoint save and load | 3 both
static void object_case(mon_dataset* ds, const char* title, const mon_config& cfg, std::vector<Opt> opts, bool fused, int long_train = 0,
                        int walk = 0) {
    std::printf("== %s\n", title);
    std::vector<long> before(opts.size());
    for (size_t i = 0; i < opts.size(); ++i) { OK(mon_get_option(opts[i].name, &before[i])); OK(mon_set_option(opts[i].name, opts[i].value)); }
    mon_object* o = nullptr; OK(mon_object_create(ds, &cfg, 7, g_Tow, g_amin, g_amax, &o));
    const mon_frame_bbox b{ 0, 8, 8, 24, 32 }; OK(mon_object_add_boxes(o, &b, 1));
    float loss = 0.f;
    if (long_train) TRAIN(o, long_train);
    train_calls(o); if (walk & 1) stale_calls(o, fused); if (walk & 2) checkpoint_calls(ds, o);
    OK(mon_object_destroy(o));
    for (size_t i = 0; i < opts.size(); ++i) OK(mon_set_option(opts[i].name, before[i]));
}

// the online manager: one object, two Train_Step_Online of 4 iterations with a pose update between them; this thread waits (without a launch of its own)
// until the object's thread has finished each
static void online_case(const char* cfg_json, const unsigned char* rgb, const unsigned char* inst) {
    std::printf("== online manager: update_dataset between two slices\n");
    hip_stub_trace(0);
    mon_online* om = nullptr; OK(mon_online_create(cfg_json, 0, 4, &om)); OK(mon_online_init(om));
    OK(mon_online_dataset_init(om, 60.f, 60.f, 32.f, 24.f, H, W, kFrames));
    for (int v = 0; v < kFrames; ++v) { char stamp[32]; std::snprintf(stamp, sizeof stamp, "%.6f", v * 0.1);
        OK(mon_online_new_frame(om, (uint32_t)v, stamp, rgb, 3, inst, nullptr, g_pose)); }
    size_t idx = 0; const float bb[6] = { -0.3f, -0.3f, -0.3f, 0.3f, 0.3f, 0.3f };
    OK(mon_online_create_nerf(om, 7, g_Tow, bb, bb + 3, &idx));
    hip_stub_trace(1);
    const auto viewer_asks = [&] { float c[3 * 16], d[16], m[16]; hip_stub_trace(0);
        (void)mon_online_render(om, idx, mon_frame_bbox{ 0, 8, 8, 4, 4 }, g_pose, c, d, m); hip_stub_trace(1); };       // (the object's thread is idle)
    const auto wait_calls = [&](int n) { for (;;) { int calls = 0; OK(mon_online_object_info(om, idx, nullptr, &calls, nullptr, nullptr)); if (calls >= n) return;
            std::this_thread::sleep_for(std::chrono::milliseconds(2)); } };
    std::vector<mon_frame_bbox> boxes; for (int v = 0; v < 12; ++v) boxes.push_back(mon_frame_bbox{ (uint32_t)v, 8, 8, 24, 32 });
    CALL(mon_online_update_nerf_bbox(om, idx, boxes.data(), boxes.size(), 1)); wait_calls(1); viewer_asks();
    float Twc[2 * 16]; std::memcpy(Twc, g_pose, 64); std::memcpy(Twc + 16, g_pose, 64);
    CALL(mon_online_update_dataset(om, 4, 2, Twc));
    const mon_frame_bbox more{ 12, 8, 8, 24, 32 };
    CALL(mon_online_update_nerf_bbox(om, idx, &more, 1, 1)); wait_calls(2); viewer_asks();
    CALL(mon_online_wait_threads_end(om));
    OK(mon_online_destroy(om));
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: trace_driver <scratch dir> <config json>\n"); return 2; }
    g_dir = argv[1];
    std::vector<unsigned char> rgb((size_t)H * W * 3, 128), inst((size_t)H * W, 7);
    mon_dataset* ds = nullptr; OK(mon_dataset_create(0, H, W, 60.f, 60.f, 32.f, 24.f, kFrames, 0, &ds));
    for (int v = 0; v < kFrames; ++v) OK(mon_dataset_add_frame(ds, v, rgb.data(), 3, 0, inst.data(), nullptr, g_pose));
    mon_config base; OK(mon_config_from_json(argv[2], &base)); base.rays_per_batch = 256;
    hip_stub_trace(1);
    object_case(ds, "base.json shape, lds_encode 0", base, { { "lds_encode", 0 } }, true);
    object_case(ds, "base.json shape, lds_encode 1", base, { { "lds_encode", 1 } }, true);
    object_case(ds, "base.json shape, lds_encode 2", base, { { "lds_encode", 2 } }, true, 0, 3);
    object_case(ds, "base.json shape, option backend 0", base, { { "backend", 0 } }, true);
    mon_config c = base; c.n_neurons = 16;
    object_case(ds, "16 neurons (outside the fused kernels), S 32", c, {}, false);
    object_case(ds, "16 neurons, S 32, lds_encode 2 (hybrid scatter, tile encode)", c, { { "lds_encode", 2 } }, false, 0, 1);
    object_case(ds, "16 neurons, S 32, lds_encode 2, step_variant 1", c, { { "lds_encode", 2 }, { "step_variant", 1 } }, false);
    c = base; c.n_samples = 16; c.rays_per_batch = 64;
    object_case(ds, "S 16 (outside the fused kernels, no hybrid scatter), R 64", c, {}, false);
    c = base; c.log2_hashmap_size = 19;
    object_case(ds, "2^19 entries per level (> 8 M parameters: records, big scatter, touched flags, lazy EMA)", c, {}, true, 0, 2);
    c = base; c.occupancy_skip = 1;
    object_case(ds, "occupancy_skip, one train call past the first refresh", c, {}, true, 300);
    object_case(ds, "occupancy_skip, lds_encode 2 (live-sample lists)", c, { { "lds_encode", 2 } }, true, 300);
    c = base; c.rng_flags = 1;
    object_case(ds, "rng_flags 1 (XORWOW)", c, {}, true);
    OK(mon_dataset_destroy(ds));
    online_case(argv[2], rgb.data(), inst.data());
    hip_stub_trace(0);
    return 0;
}
