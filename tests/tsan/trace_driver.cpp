// trace_driver.cpp -- walks the C ABI single-threaded on the host side built --offload-host-only against tests/tsan/hip_stub.cpp (no sanitizer) with the
// stub's launch trace on: every kernel launch and asynchronous fill / copy of every training path as one line of text, under a heading per case and per call;
// then (part two) of every scene, pose and field-query route on both sides and through the online manager, the cost fields and the device-resident distance
// fields (ray tracing, beam scores and the signed fields included) in a section of their own, and a list of the calls those routes refuse, with code and message.
// tests/test_launch_trace.py compares the output with tests/golden/launch_trace.txt.  Usage: trace_driver <scratch dir> <config json>.  TEST INFRASTRUCTURE.
#include <chrono>
#include <cmath>
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

// ---- part two: the inference routes.  Every argument of every route in one record: a route reads its own fields, a case changes one or two of them.
struct Args {
    mon_object* const* objs; size_t n_objs; int side;
    mon_frame_bbox rect; const float* Twc; float* rgb; float* depth;                      // render (rgb, depth: the required outputs of probe and cast too)
    const float* poses; size_t n_poses; const mon_scene_query* q; size_t n_q;             // probe; poses: also the batch's poses and the candidates
    const mon_scene_ray* rays; size_t n_rays; float hit_opacity;                          // cast
    const mon_frame_bbox* obs; size_t n_obs; const mon_pose_refine_params* p; const mon_pose_c2f_params* c; const float* lw; float* pose_io;
    float* losses; const mon_reloc_params* r; float* pose_out;                            // batch, relocalise
    const mon_frame_bbox* wobs; size_t n_wobs; float* wTwc; float* Tow16s; const mon_window_params* w;      // window
    mon_object* obj; const mon_pose_c2f_params* cc; const float* lwl;                     // object pose routes (cc, lwl: the arguments the _c2f / _levels calls require)
    mon_online* om; size_t idx; size_t n_online;
    float* out;                                                                           // every optional output
    // the field queries: point lists (world, unit cube), the lattice, what gradients, distance and components add, their required outputs; opt: the optional
    // outputs are asked for (each in a slice of `out` of its own: cast_normals reads its own instance row back) or all NULL
    const float* pts; size_t n_pts; const float* upts; const float* origin; const float* step; int nx, ny, nz; const float* glw; const int32_t* sel;
    float sigma_min, max_dist; int region; float clearance; int conn; mon_lattice_component* table; uint32_t cap; uint32_t* n_comp; const uint8_t* mask;
    float* sigma; float* grad; float* raw4; float* normal; float* dist; int32_t* label; float* xyz_out; mon_scene_ray* rays_out; bool opt;
    // the cost fields (mask: the passable cells), a walk along next, and the device-resident distance fields: a handle with what its sample, score, match
    // and register calls read (pts, n_pts: the sampled points and the scan; field_max: the scene calls' finite max_dist)
    const float* cell_cost; const int32_t* seeds; size_t n_seeds; float max_cost, soft_radius, soft_weight; float* cost;
    const int32_t* next; size_t n_cells; int32_t start; int32_t* path; size_t path_cap; size_t* n_path;
    mon_dist_field* field; mon_dist_field** field_out; const float* fdist; mon_dist_field_desc* info; float field_max, outside;
    const float* spheres; size_t n_spheres; const float* ways; int way_floats; size_t n_traj, n_way, n_sub; const mon_traj_score_params* tp; float* min_clear;
    const float* mposes; size_t n_h; const float* pivots; const mon_scan_match_params* mp; mon_register_params* rp; float* poses_out;
    // ray tracing on a handle (frays[n][6]; tposes NULL: world rays) and the signed fields (val: host values per cell; max_dist and field_max as above)
    const float* frays; size_t n_frays; const float* tposes; size_t n_tposes; mon_trace_params* trp; const float* measured; const mon_beam_params* bp; float* range;
    const float* val; float iso; uint32_t flags;
};
static int32_t* as_i32(float* p) { return reinterpret_cast<int32_t*>(p); }
static int scene_render(const Args& a) { return mon_scene_render(a.objs, a.n_objs, a.side, a.rect, a.Twc, a.rgb, a.depth, a.out, as_i32(a.out)); }
static int scene_probe(const Args& a) { return mon_scene_probe(a.objs, a.n_objs, a.side, a.poses, a.n_poses, a.q, a.n_q, a.rgb, a.depth, a.out, as_i32(a.out), a.out,
        as_i32(a.out)); }
static int scene_cast(const Args& a) { return mon_scene_cast(a.objs, a.n_objs, a.side, a.rays, a.n_rays, a.hit_opacity, a.rgb, a.depth, a.out, as_i32(a.out), a.out,
        a.out, as_i32(a.out)); }
static int scene_pose_loss(const Args& a) { return mon_scene_pose_loss(a.objs, a.n_objs, a.side, a.obs, a.n_obs, a.Twc, a.p, 3u, a.lw, a.out, a.out + 8); }
static int scene_refine_camera(const Args& a) { return mon_scene_refine_camera(a.objs, a.n_objs, a.side, a.obs, a.n_obs, a.p, a.c, a.pose_io, a.out); }
static int scene_pose_loss_batch(const Args& a) { return mon_scene_pose_loss_batch(a.objs, a.n_objs, a.side, a.obs, a.n_obs, a.poses, a.n_poses, a.p, 3u, a.losses); }
static int scene_relocalise(const Args& a) { mon_reloc_result res; return mon_scene_relocalise(a.objs, a.n_objs, a.side, a.obs, a.n_obs, a.poses, a.n_poses, a.p,
        a.c, a.r, a.pose_out, &res, a.out); }
static int scene_window_loss(const Args& a) { return mon_scene_window_loss(a.objs, a.n_objs, a.side, a.wobs, a.n_wobs, a.wTwc, a.Tow16s, a.p, 3u, a.lw, a.out,
        a.out + 8, a.out + 64, a.out + 512); }
static int scene_refine_window(const Args& a) { return mon_scene_refine_window(a.objs, a.n_objs, a.side, a.wobs, a.n_wobs, a.p, a.c, a.w, a.wTwc, a.Tow16s, a.out,
        a.out + 64); }
static int object_pose_loss(const Args& a) { return mon_object_pose_loss(a.obj, a.side, a.obs, a.n_obs, a.Twc, a.p, 3u, a.out, a.out + 8); }
static int object_pose_loss_levels(const Args& a) { return mon_object_pose_loss_levels(a.obj, a.side, a.obs, a.n_obs, a.Twc, a.p, 3u, a.lwl, a.out, a.out + 8); }
static int object_refine_pose(const Args& a) { return mon_object_refine_pose(a.obj, a.side, a.obs, a.n_obs, a.p, a.pose_io, a.out); }
static int object_refine_pose_c2f(const Args& a) { return mon_object_refine_pose_c2f(a.obj, a.side, a.obs, a.n_obs, a.p, a.cc, a.pose_io, a.out); }
static int online_render_scene(const Args& a) { return mon_online_render_scene(a.om, a.rect, a.Twc, a.rgb, a.depth, a.out, as_i32(a.out)); }
static int online_probe_scene(const Args& a) { return mon_online_probe_scene(a.om, a.poses, a.n_poses, a.q, a.n_q, a.rgb, a.depth, a.out, as_i32(a.out), a.out,
        as_i32(a.out)); }
static int online_cast_rays(const Args& a) { return mon_online_cast_rays(a.om, a.rays, a.n_rays, a.hit_opacity, a.rgb, a.depth, a.out, as_i32(a.out), a.out, a.out,
        as_i32(a.out)); }
static int online_refine_camera(const Args& a) { return mon_online_refine_camera(a.om, a.obs, a.n_obs, a.p, a.c, a.pose_io, a.out); }
static int online_refine_window(const Args& a) { uint8_t inc[8]; return mon_online_refine_window(a.om, a.wobs, a.n_wobs, a.p, a.c, a.w, a.wTwc, a.Tow16s, a.n_online,
        inc, a.out, a.out + 64); }
static int online_relocalise(const Args& a) { mon_reloc_result res; return mon_online_relocalise(a.om, a.obs, a.n_obs, a.poses, a.n_poses, a.p, a.c, a.r, a.pose_out,
        &res, a.out); }
static int online_refine_pose(const Args& a) { return mon_online_refine_pose(a.om, a.idx, a.obs, a.n_obs, a.p, a.pose_io, a.out); }
static int online_refine_pose_c2f(const Args& a) { return mon_online_refine_pose_c2f(a.om, a.idx, a.obs, a.n_obs, a.p, a.cc, a.pose_io, a.out); }

// the field queries.  sl(a, k): optional output k of such a route
static float* sl(const Args& a, int k) { return a.opt ? a.out + (size_t)k * 65536 : nullptr; }
static uint32_t* as_u32(float* p) { return reinterpret_cast<uint32_t*>(p); }
static int object_query_points(const Args& a) { return mon_object_query_points(a.obj, a.side, a.upts, a.n_pts, a.raw4); }
static int scene_query_points(const Args& a) { return mon_scene_query_points(a.objs, a.n_objs, a.side, a.pts, a.n_pts, a.sigma, sl(a, 1), as_i32(sl(a, 2)), sl(a, 3),
        as_u32(sl(a, 4))); }
static int scene_query_lattice(const Args& a) { return mon_scene_query_lattice(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma, sl(a, 1),
        as_i32(sl(a, 2)), sl(a, 3), as_u32(sl(a, 4))); }
static int object_query_gradients(const Args& a) { return mon_object_query_gradients(a.obj, a.side, a.upts, a.n_pts, a.glw, sl(a, 1), a.grad); }
static int scene_query_gradients(const Args& a) { return mon_scene_query_gradients(a.objs, a.n_objs, a.side, a.pts, a.n_pts, a.glw, a.sel, a.sigma, sl(a, 1),
        as_i32(sl(a, 2)), sl(a, 3), as_u32(sl(a, 4)), a.grad, sl(a, 13), sl(a, 14)); }
static int scene_query_lattice_gradients(const Args& a) { return mon_scene_query_lattice_gradients(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.glw,
        a.sigma, sl(a, 1), as_i32(sl(a, 2)), sl(a, 3), as_u32(sl(a, 4)), a.grad, sl(a, 13), sl(a, 14)); }
static int scene_cast_normals(const Args& a) { return mon_scene_cast_normals(a.objs, a.n_objs, a.side, a.rays, a.n_rays, a.hit_opacity, a.glw, a.rgb, a.depth, sl(a, 1),
        as_i32(sl(a, 2)), sl(a, 3), sl(a, 4), as_i32(sl(a, 13)), sl(a, 14), a.normal, sl(a, 15)); }
static int scene_distance_lattice(const Args& a) { return mon_scene_distance_lattice(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min,
        a.max_dist, a.dist, as_i32(sl(a, 1)), as_i32(sl(a, 2)), sl(a, 3), sl(a, 4)); }
// region 0 has no dist; the table (and its count) is an argument of its own
static int scene_components_lattice(const Args& a) { return mon_scene_components_lattice(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min,
        a.region, a.clearance, a.conn, a.label, as_i32(sl(a, 1)), a.table, a.cap, a.n_comp, a.region == 1 ? sl(a, 2) : nullptr, sl(a, 3), as_i32(sl(a, 4))); }
static int components_with_dist(const Args& a) { return mon_scene_components_lattice(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min,
        a.region, a.clearance, a.conn, a.label, nullptr, a.table, a.cap, a.n_comp, a.out + 2 * 65536, nullptr, nullptr); }
static int distance_transform(const Args& a) { return mon_distance_transform(0, a.mask, a.nx, a.ny, a.nz, a.step, a.max_dist, a.dist, as_i32(sl(a, 1))); }
static int label_components(const Args& a) { return mon_label_components(0, a.mask, a.nx, a.ny, a.nz, a.conn, a.label, as_i32(sl(a, 1)), a.table, a.cap, a.n_comp); }
static int lattice_points(const Args& a) { return mon_lattice_points(a.origin, a.step, a.nx, a.ny, a.nz, a.xyz_out); }
static int camera_rays(const Args& a) { return mon_camera_rays(60.f, 60.f, 32.f, 24.f, a.poses, a.n_poses, a.q, a.n_q, a.rays_out, sl(a, 1)); }
static int online_query_points(const Args& a) { return mon_online_query_points(a.om, a.pts, a.n_pts, a.sigma, sl(a, 1), as_i32(sl(a, 2)), sl(a, 3), as_u32(sl(a, 4))); }
static int online_query_lattice(const Args& a) { return mon_online_query_lattice(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma, sl(a, 1), as_i32(sl(a, 2)), sl(a, 3),
        as_u32(sl(a, 4))); }
static int online_query_gradients(const Args& a) { return mon_online_query_gradients(a.om, a.pts, a.n_pts, a.glw, a.sel, a.sigma, sl(a, 1), as_i32(sl(a, 2)), sl(a, 3),
        as_u32(sl(a, 4)), a.grad, sl(a, 13), sl(a, 14)); }
static int online_cast_normals(const Args& a) { return mon_online_cast_normals(a.om, a.rays, a.n_rays, a.hit_opacity, a.glw, a.rgb, a.depth, sl(a, 1), as_i32(sl(a, 2)),
        sl(a, 3), sl(a, 4), as_i32(sl(a, 13)), sl(a, 14), a.normal, sl(a, 15)); }
static int online_distance_lattice(const Args& a) { return mon_online_distance_lattice(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.max_dist, a.dist,
        as_i32(sl(a, 1)), as_i32(sl(a, 2)), sl(a, 3), sl(a, 4)); }
static int online_components_lattice(const Args& a) { return mon_online_components_lattice(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.region, a.clearance,
        a.conn, a.label, as_i32(sl(a, 1)), a.table, a.cap, a.n_comp, a.region == 1 ? sl(a, 2) : nullptr, sl(a, 3), as_i32(sl(a, 4))); }
// the cost fields and the device-resident distance fields
static int shortest_paths(const Args& a) { return mon_shortest_paths(0, a.mask, a.nx, a.ny, a.nz, a.step, a.conn, a.cell_cost, a.seeds, a.n_seeds, a.max_cost, a.cost,
        as_i32(sl(a, 1))); }
static int scene_paths_lattice(const Args& a) { return mon_scene_paths_lattice(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.clearance,
        a.soft_radius, a.soft_weight, a.conn, a.seeds, a.n_seeds, a.max_cost, a.cost, as_i32(sl(a, 1)), sl(a, 2), sl(a, 3), as_i32(sl(a, 4))); }
static int online_paths_lattice(const Args& a) { return mon_online_paths_lattice(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.clearance, a.soft_radius,
        a.soft_weight, a.conn, a.seeds, a.n_seeds, a.max_cost, a.cost, as_i32(sl(a, 1)), sl(a, 2), sl(a, 3), as_i32(sl(a, 4))); }
static int lattice_path(const Args& a) { return mon_lattice_path(a.next, a.n_cells, a.start, a.path, a.path_cap, a.n_path); }
static int dist_field_create(const Args& a) { return mon_dist_field_create(0, a.fdist, a.nx, a.ny, a.nz, a.origin, a.step, a.field_out); }
static int scene_dist_field(const Args& a) { return mon_scene_dist_field(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.field_max,
        a.field_out); }
static int online_dist_field(const Args& a) { return mon_online_dist_field(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.field_max, a.field_out); }
static int dist_field_info(const Args& a) { return mon_dist_field_info(a.field, a.info); }
static int dist_field_read(const Args& a) { return mon_dist_field_read(a.field, a.dist); }
static int dist_field_destroy(const Args& a) { return mon_dist_field_destroy(a.field); }
static int dist_field_sample(const Args& a) { return mon_dist_field_sample(a.field, a.pts, a.n_pts, a.outside, a.dist, sl(a, 1)); }
static int dist_field_score(const Args& a) { return mon_dist_field_score(a.field, a.spheres, a.n_spheres, a.ways, a.way_floats, a.n_traj, a.n_way, a.n_sub, a.tp,
        a.min_clear, as_i32(sl(a, 1)), sl(a, 2), sl(a, 3), sl(a, 4)); }
static int dist_field_match(const Args& a) { return mon_dist_field_match(a.field, a.pts, a.n_pts, a.mposes, a.n_h, a.pivots, a.mp, a.cost, as_i32(sl(a, 1)),
        as_i32(sl(a, 2)), sl(a, 3)); }
static int register_default(const Args& a) { return mon_register_default(a.field, a.rp); }
static int dist_field_register(const Args& a) { return mon_dist_field_register(a.field, a.pts, a.n_pts, a.mposes, a.n_h, a.rp, a.poses_out, a.cost, as_i32(sl(a, 1)),
        as_i32(sl(a, 2)), as_i32(sl(a, 3)), as_i32(sl(a, 4)), as_i32(sl(a, 13))); }
static int trace_default(const Args& a) { return mon_trace_default(a.field, a.trp); }
static int dist_field_trace(const Args& a) { return mon_dist_field_trace(a.field, a.frays, a.n_frays, a.tposes, a.n_tposes, a.trp, a.range, as_i32(sl(a, 1)),
        as_i32(sl(a, 2)), sl(a, 3)); }
static int dist_field_beam_score(const Args& a) { return mon_dist_field_beam_score(a.field, a.frays, a.n_frays, a.measured, a.tposes, a.n_tposes, a.trp, a.bp, a.cost,
        as_i32(sl(a, 1)), as_i32(sl(a, 2))); }
// the signed distance fields
static int signed_distance_transform(const Args& a) { return mon_signed_distance_transform(0, a.val, a.iso, a.nx, a.ny, a.nz, a.step, a.max_dist, a.dist,
        as_i32(sl(a, 1))); }
static int scene_signed_distance_lattice(const Args& a) { return mon_scene_signed_distance_lattice(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz,
        a.sigma_min, a.flags, a.max_dist, a.dist, as_i32(sl(a, 1)), as_i32(sl(a, 2)), sl(a, 3), sl(a, 4), sl(a, 13)); }
static int scene_signed_dist_field(const Args& a) { return mon_scene_signed_dist_field(a.objs, a.n_objs, a.side, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min,
        a.flags, a.field_max, a.field_out); }
static int online_signed_distance_lattice(const Args& a) { return mon_online_signed_distance_lattice(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.flags,
        a.max_dist, a.dist, as_i32(sl(a, 1)), as_i32(sl(a, 2)), sl(a, 3), sl(a, 4), sl(a, 13)); }
static int online_signed_dist_field(const Args& a) { return mon_online_signed_dist_field(a.om, a.origin, a.step, a.nx, a.ny, a.nz, a.sigma_min, a.flags, a.field_max,
        a.field_out); }

// a call that must fail, on one line with its code and message (no exit); `change` edits a copy `a` of the good arguments
#define ERR(route, change) do { Args a = good; change; const int rc_ = route(a); \
        std::printf("-- %s, %s -> %d: %s\n", #route, #change, rc_, rc_ != MON_OK ? mon_last_error() : "no error"); } while (0)
// what every route with an object list refuses of it
#define OBJS_ERRS(route) do { ERR(route, a.objs = nullptr); ERR(route, a.n_objs = 0); ERR(route, a.objs = many.data(); a.n_objs = 257); ERR(route, a.side = 2); \
        ERR(route, a.objs = with_null); ERR(route, a.objs = other_K); ERR(route, a.objs = other_ds); ERR(route, a.objs = narrow); ERR(route, a.objs = xorwow); \
        ERR(route, a.objs = unpublished; a.side = 1); } while (0)
// ... and every route with boxes of one frame and refinement parameters (b_, p_: the fields the route reads them from)
#define OBS_ERRS(route, b_, n_) do { ERR(route, a.b_ = nullptr); ERR(route, a.n_ = 0); ERR(route, a.p = nullptr); ERR(route, a.p = &p_neg); \
        ERR(route, a.p = &p_many); ERR(route, a.b_ = &box_noframe; a.n_ = 1); ERR(route, a.b_ = &box_outside; a.n_ = 1); ERR(route, a.b_ = &box_empty; a.n_ = 1); \
        } while (0)

static mon_object* trained_object(mon_dataset* ds, const mon_config& cfg, float tx, int steps) {
    float Tow[16]; std::memcpy(Tow, g_Tow, 64); Tow[12] = tx;
    mon_object* o = nullptr; OK(mon_object_create(ds, &cfg, 7, Tow, g_amin, g_amax, &o));
    const mon_frame_bbox b{ 0, 8, 8, 24, 32 }; OK(mon_object_add_boxes(o, &b, 1));
    float loss = 0.f;
    if (steps) { viewer_asks(o); hip_stub_trace(0); OK(mon_object_train(o, steps, &loss)); }      // (the viewer's request forces the publication)
    return o;
}
static mon_dataset* make_dataset(float fx, const unsigned char* rgb, const unsigned char* inst) {
    mon_dataset* ds = nullptr; OK(mon_dataset_create(0, H, W, fx, 60.f, 32.f, 24.f, kFrames, 0, &ds));
    for (int v = 0; v < kFrames; ++v) OK(mon_dataset_add_frame(ds, v, rgb, 3, 0, inst, nullptr, g_pose));
    return ds;
}
// an online manager of two objects over the driver's frames; publish: both get twelve boxes and train one Train_Step_Online, which ends with a publication
// -- this thread waits for each (without a launch of its own), after which both object threads sleep
static mon_online* make_online(const char* cfg_json, const unsigned char* rgb, const unsigned char* inst, bool publish) {
    mon_online* om = nullptr; OK(mon_online_create(cfg_json, 0, 4, &om)); OK(mon_online_init(om));
    OK(mon_online_dataset_init(om, 60.f, 60.f, 32.f, 24.f, H, W, kFrames));
    for (int v = 0; v < kFrames; ++v) { char stamp[32]; std::snprintf(stamp, sizeof stamp, "%.6f", v * 0.1);
        OK(mon_online_new_frame(om, (uint32_t)v, stamp, rgb, 3, inst, nullptr, g_pose)); }
    const float bb[6] = { -0.3f, -0.3f, -0.3f, 0.3f, 0.3f, 0.3f };
    std::vector<mon_frame_bbox> boxes; for (int v = 0; v < 12; ++v) boxes.push_back(mon_frame_bbox{ (uint32_t)v, 8, 8, 24, 32 });
    for (int k = 0; k < 2; ++k) {
        size_t idx = 0; OK(mon_online_create_nerf(om, 7, g_Tow, bb, bb + 3, &idx));
        if (!publish) continue;
        OK(mon_online_update_nerf_bbox(om, idx, boxes.data(), boxes.size(), 1));
        for (;;) { int calls = 0; OK(mon_online_object_info(om, idx, nullptr, &calls, nullptr, nullptr)); if (calls >= 1) break;
            std::this_thread::sleep_for(std::chrono::milliseconds(2)); }
    }
    return om;
}

static void inference_part(const char* cfg_json, const mon_config& base, const unsigned char* rgb, const unsigned char* inst) {
    // ---- the set-up, untraced
    hip_stub_trace(0);
    mon_dataset* ds = make_dataset(60.f, rgb, inst); mon_dataset* ds_K = make_dataset(61.f, rgb, inst); mon_dataset* ds_2 = make_dataset(60.f, rgb, inst);
    mon_object* o0 = trained_object(ds, base, 0.f, 2); mon_object* o1 = trained_object(ds, base, 0.05f, 2);
    mon_object* o_K = trained_object(ds_K, base, 0.f, 2); mon_object* o_2 = trained_object(ds_2, base, 0.f, 2);
    mon_config c16 = base; c16.n_neurons = 16; mon_config cxw = base; cxw.rng_flags = 1;
    mon_object* o_16 = trained_object(ds, c16, 0.f, 2); mon_object* o_xw = trained_object(ds, cxw, 0.f, 2); mon_object* o_un = trained_object(ds, base, 0.f, 0);
    hip_stub_trace(0);
    mon_online* om = make_online(cfg_json, rgb, inst, true); mon_online* om_none = make_online(cfg_json, rgb, inst, false);
    mon_object* objs[2] = { o0, o1 }; mon_object* with_null[2] = { o0, nullptr }; mon_object* other_K[2] = { o0, o_K }; mon_object* other_ds[2] = { o0, o_2 };
    mon_object* narrow[2] = { o0, o_16 }; mon_object* xorwow[2] = { o0, o_xw }; mon_object* unpublished[2] = { o0, o_un };
    std::vector<mon_object*> many(257, o0);
    std::vector<float> out(1u << 21, 0.f), many_poses(16 * 4097);
    for (size_t i = 0; i < many_poses.size(); i += 16) std::memcpy(&many_poses[i], g_pose, 64);
    float poses3[3 * 16], pose_io[16], pose_out[16], wTwc[2 * 16], Tow16s[2 * 16], nan_pose[16], nan_Tow[2 * 16], lw[64], lw_neg[64];
    for (int k = 0; k < 3; ++k) std::memcpy(poses3 + 16 * k, g_pose, 64);
    std::memcpy(pose_io, g_pose, 64); std::memcpy(wTwc, poses3, 128); std::memcpy(Tow16s, g_Tow, 64); std::memcpy(Tow16s + 16, g_Tow, 64);
    std::memcpy(nan_pose, g_pose, 64); nan_pose[13] = NAN; std::memcpy(nan_Tow, Tow16s, 128); nan_Tow[16 + 12] = INFINITY;
    for (int l = 0; l < 64; ++l) { lw[l] = 1.f; lw_neg[l] = l == 1 ? -1.f : 1.f; }
    const mon_scene_query q[5] = { { 0, 0, 10.5f, 8.25f }, { 1, 1, 32.f, 24.f }, { 0, 2, 40.f, 30.f }, { 1, 3, 0.f, 0.f }, { 0, 4, 63.f, 47.f } };
    mon_scene_query q_nan[5], q_pose[5], q_key[5];
    for (int i = 0; i < 5; ++i) q_nan[i] = q_pose[i] = q_key[i] = q[i];
    q_nan[2].u = NAN; q_pose[3].pose = 2; q_key[4].key = 1u << 26;
    const mon_scene_ray rays[4] = { { { 0, 0, -2 }, 10.f, { 0, 0, 1 }, 0 }, { { 0.1f, 0, -2 }, 10.f, { 0, 0, 1 }, 1 }, { { 0, 0.1f, -2 }, 1.f, { 0, 0, 1 }, 2 },
                                    { { 0, 0, 2 }, INFINITY, { 0, 0, -1 }, 3 } };
    mon_scene_ray r_nan[4], r_long[4], r_tmax[4], r_key[4];
    for (int i = 0; i < 4; ++i) r_nan[i] = r_long[i] = r_tmax[i] = r_key[i] = rays[i];
    r_nan[1].o[2] = NAN; r_long[2].d[2] = 1.1f; r_tmax[3].t_max = 0.f; r_key[0].key = 1u << 26;
    const mon_frame_bbox obs[2] = { { 0, 8, 8, 16, 16 }, { 0, 30, 20, 8, 12 } };
    const mon_frame_bbox wobs[3] = { { 0, 8, 8, 16, 16 }, { 0, 30, 20, 8, 12 }, { 1, 8, 8, 16, 16 } };          // a window of two frames, the first with two boxes
    const mon_frame_bbox two_frames[2] = { { 0, 8, 8, 16, 16 }, { 1, 8, 8, 16, 16 } }, apart[3] = { { 0, 8, 8, 16, 16 }, { 1, 8, 8, 16, 16 }, { 0, 30, 20, 8, 12 } };
    const mon_frame_bbox box_noframe{ 99, 8, 8, 16, 16 }, box_outside{ 0, 40, 8, 16, 32 }, box_empty{ 0, 8, 8, 0, 16 };
    std::vector<mon_frame_bbox> frames33; for (uint32_t f = 0; f < 33; ++f) frames33.push_back(mon_frame_bbox{ f, 8, 8, 16, 16 });
    mon_pose_refine_params p; OK(mon_pose_refine_default(&p)); p.iters = 2; p.rays_per_iter = 64;
    mon_pose_refine_params p_neg = p, p_many = p, p_score = p; p_neg.iters = -1; p_many.rays_per_iter = (1u << 22) + 1u; p_score.rays_per_iter = 16385;
    mon_pose_c2f_params c2f; OK(mon_pose_c2f_default(&c2f)); mon_pose_c2f_params c_bad = c2f; c_bad.ramp = 0.f;
    mon_reloc_params r; OK(mon_reloc_default(&r)); r.score_rays = 32; r.keep = 2;
    mon_reloc_params r_rays0 = r, r_rays_many = r, r_keep0 = r, r_keep17 = r; r_rays0.score_rays = 0; r_rays_many.score_rays = 16385; r_keep0.keep = 0; r_keep17.keep = 17;
    mon_window_params w; OK(mon_window_default(&w));
    mon_window_params w_fixed3 = w, w_free = w, w_lr = w; w_fixed3.n_fixed_frames = 3; w_free.n_fixed_frames = 0; w_lr.lr_obj_rot = -1.f;
    float* const o = out.data();
    // the field queries: five world points in and around the boxes, five of the unit cube, a lattice of 3 x 2 x 2 around the objects
    const float pts[15] = { 0.f, 0.f, 0.f, 0.05f, 0.1f, -0.1f, 0.3f, 0.2f, 0.1f, -0.2f, 0.25f, 0.f, 1.f, 1.f, 1.f };
    const float upts[15] = { 0.f, 0.f, 0.f, 0.5f, 0.5f, 0.5f, 1.f, 1.f, 1.f, 0.25f, 0.75f, 0.125f, 0.9f, 0.1f, 0.3f };
    float pts_nan[15], upts_out[15]; std::memcpy(pts_nan, pts, 60); pts_nan[7] = NAN; std::memcpy(upts_out, upts, 60); upts_out[10] = 1.5f;
    const float origin[3] = { -0.3f, -0.3f, -0.3f }, step[3] = { 0.3f, 0.6f, 0.6f }, origin_nan[3] = { -0.3f, NAN, -0.3f }, step_inf[3] = { 0.3f, 0.6f, INFINITY };
    const float origin_far[3] = { 3e38f, 0.f, 0.f }, step_far[3] = { 3e38f, 0.6f, 0.6f };
    const int32_t sel[5] = { 0, 1, -1, 1, 0 }, sel_2[5] = { 0, 1, -1, 2, 0 }, sel_m2[5] = { 0, -2, -1, 1, 0 };
    float glw[64], lw_neg0[64]; for (int l = 0; l < 64; ++l) { glw[l] = l % 2 ? 0.5f : 1.f; lw_neg0[l] = l == 0 ? -1.f : 1.f; }
    const uint8_t mask[12] = { 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 1 };
    uint32_t n_comp = 0;
    Args g0{ objs, 2, 0, mon_frame_bbox{ 0, 4, 4, 16, 24 }, g_pose, o, o, poses3, 2, q, 5, rays, 4, 0.5f, obs, 2, &p, nullptr, nullptr, pose_io, o, &r, pose_out,
             wobs, 3, wTwc, Tow16s, &w, o0, &c2f, lw, om, 0, 2, o };
    g0.pts = pts; g0.n_pts = 5; g0.upts = upts; g0.origin = origin; g0.step = step; g0.nx = 3; g0.ny = 2; g0.nz = 2; g0.glw = nullptr; g0.sel = nullptr;
    g0.sigma_min = 1.f; g0.max_dist = INFINITY; g0.region = 0; g0.clearance = 0.1f; g0.conn = 26; g0.table = nullptr; g0.cap = 64; g0.n_comp = nullptr; g0.mask = mask;
    g0.sigma = o; g0.grad = o + 5 * 65536; g0.raw4 = o + 6 * 65536; g0.normal = o + 7 * 65536; g0.dist = o + 8 * 65536; g0.label = as_i32(o + 9 * 65536);
    g0.xyz_out = o + 11 * 65536; g0.rays_out = reinterpret_cast<mon_scene_ray*>(o + 12 * 65536); g0.opt = true;
    mon_lattice_component* const table = reinterpret_cast<mon_lattice_component*>(o + 10 * 65536);
    // the cost fields and the distance-field handles: two seeds, a multiplier and a field per cell of either lattice, a walk of three cells, a body of two
    // spheres on two trajectories of three waypoints (positions, matrices), the scan = pts under three poses
    const size_t n_big = 33 * 32 * 16;
    const int32_t seeds[2] = { 0, 11 }, seeds_out[2] = { 0, 12 }, next4[4] = { 1, 2, -1, 0 }, next_cycle[4] = { 1, 0, -1, 0 }, next_bad[4] = { 1, 9, -1, 0 };
    float cell_cost[12], cost_neg[12], fdist[12], fdist_nan[12];
    for (int i = 0; i < 12; ++i) { cell_cost[i] = cost_neg[i] = 1.5f; fdist[i] = fdist_nan[i] = 0.1f * (float)i; }
    cost_neg[5] = -1.f; fdist_nan[7] = NAN;
    const std::vector<uint8_t> big_mask(n_big, 1); const std::vector<float> big_cost(n_big, 1.f), big_fdist(n_big, 0.25f);
    std::vector<float> big_val(n_big); for (size_t i = 0; i < n_big; ++i) big_val[i] = (float)(i % 33) / 32.f;
    const float step_zero[3] = { 0.3f, 0.f, 0.6f };
    const float spheres[8] = { 0.f, 0.f, 0.f, 0.05f, 0.1f, 0.f, 0.f, 0.02f }, sphere_neg[8] = { 0.f, 0.f, 0.f, 0.05f, 0.1f, 0.f, 0.f, -1.f };
    float ways3[2 * 3 * 3], ways16[2 * 3 * 16];
    for (int k = 0; k < 6; ++k) { for (int a = 0; a < 3; ++a) ways3[3 * k + a] = -0.2f + 0.1f * (float)k;
        std::memcpy(ways16 + 16 * k, g_Tow, 64); ways16[16 * k + 3] = -0.2f + 0.1f * (float)k; }
    const mon_traj_score_params tp{ 0.5f, 0.01f, 0.1f }, tp_nan{ 0.5f, NAN, 0.1f };
    float pose_nan3[3 * 16], pivots[9], pivots_nan[9]; std::memcpy(pose_nan3, poses3, 192); pose_nan3[16 + 3] = NAN;
    for (int k = 0; k < 9; ++k) pivots[k] = pivots_nan[k] = 0.01f * (float)k;
    pivots_nan[4] = INFINITY;
    const mon_scan_match_params mp{ 0.1f, 0.5f }, mp_huber0{ 0.f, 0.5f }, mp_nan{ 0.1f, NAN };
    int32_t path[8]; size_t n_path = 0; mon_dist_field* fh = nullptr; mon_dist_field_desc info; mon_register_params rp{};
    g0.cell_cost = cell_cost; g0.seeds = seeds; g0.n_seeds = 2; g0.max_cost = INFINITY; g0.soft_radius = 0.5f; g0.soft_weight = 2.f; g0.cost = o + 16 * 65536;
    g0.next = next4; g0.n_cells = 4; g0.start = 3; g0.path = path; g0.path_cap = 8; g0.n_path = &n_path;
    g0.field = nullptr; g0.field_out = &fh; g0.fdist = fdist; g0.info = &info; g0.field_max = 0.5f; g0.outside = 0.5f;
    g0.spheres = spheres; g0.n_spheres = 2; g0.ways = ways3; g0.way_floats = 3; g0.n_traj = 2; g0.n_way = 3; g0.n_sub = 2; g0.tp = &tp; g0.min_clear = o + 17 * 65536;
    g0.mposes = poses3; g0.n_h = 3; g0.pivots = pivots; g0.mp = &mp; g0.rp = &rp; g0.poses_out = o + 18 * 65536;
    // four rays into the lattice from its corner and from outside, one beam without a return; the signed fields read fdist as values around iso 0.45
    const float frays[24] = { -0.3f, -0.3f, -0.3f, 1.f, 0.f, 0.f, -0.3f, 0.f, 0.f, 0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 2.f, 0.f, 0.f, -1.f };
    const float measured[4] = { 0.2f, NAN, 0.5f, 0.1f };
    mon_trace_params trp{}; const mon_beam_params bp{ 0.1f }, bp_huber0{ 0.f };
    g0.frays = frays; g0.n_frays = 4; g0.tposes = poses3; g0.n_tposes = 1; g0.trp = &trp; g0.measured = measured; g0.bp = &bp; g0.range = o + 19 * 65536;
    g0.val = fdist; g0.iso = 0.45f; g0.flags = 0u;
    Args good = g0;

    // ---- every route once, on both sides
    std::printf("== inference routes\n");
    hip_stub_trace(1);
    for (int side = 0; side < 2; ++side) {
        std::printf("-- side %d\n", side);
        Args a = good; a.side = side; Args ac = a; ac.c = &c2f; Args al = a; al.lw = lw; Args a3 = a; a3.n_poses = 3;
        CALL(scene_render(a)); CALL(scene_probe(a)); CALL(scene_cast(a)); CALL(scene_pose_loss(a)); CALL(scene_pose_loss(al));
        CALL(scene_refine_camera(a)); CALL(scene_refine_camera(ac)); CALL(scene_pose_loss_batch(a3)); CALL(scene_relocalise(a3)); CALL(scene_relocalise(ac));
        CALL(scene_window_loss(al)); CALL(scene_refine_window(a)); CALL(scene_refine_window(ac));
        CALL(object_pose_loss(a)); CALL(object_pose_loss_levels(a)); CALL(object_refine_pose(a)); CALL(object_refine_pose_c2f(a));
        // the field queries; big: 33 x 32 x 16 = 16 896 cells, one pass boundary with a ragged tail of 512; bare: every optional output NULL
        Args big = a; big.nx = 33; big.ny = 32; big.nz = 16; Args ag = a; ag.glw = glw; ag.sel = sel; Args bare = a; bare.opt = false;
        Args dt = a; dt.max_dist = 0.5f; Args c0 = a; c0.table = table; c0.n_comp = &n_comp; Args c1 = a; c1.region = 1; c1.conn = 6;
        Args c1bare = c1; c1bare.opt = false; Args bigc = big; bigc.region = 1; bigc.table = table; bigc.n_comp = &n_comp;
        CALL(object_query_points(a)); CALL(scene_query_points(a)); CALL(scene_query_lattice(a)); CALL(scene_query_lattice(big));
        CALL(object_query_gradients(a)); CALL(scene_query_gradients(ag)); CALL(scene_query_gradients(a)); CALL(scene_query_lattice_gradients(a));
        CALL(scene_query_lattice_gradients(big)); CALL(scene_cast_normals(a));
        CALL(scene_distance_lattice(dt)); CALL(scene_distance_lattice(bare)); CALL(scene_distance_lattice(big));
        CALL(scene_components_lattice(c0)); CALL(scene_components_lattice(c1)); CALL(scene_components_lattice(c1bare)); CALL(scene_components_lattice(bigc));
    }
    {   std::printf("-- no side\n");
        Args a = good; Args c0 = a; c0.table = table; c0.n_comp = &n_comp;
        CALL(distance_transform(a)); CALL(label_components(c0)); CALL(lattice_points(a)); CALL(camera_rays(a));
    }
    {   std::printf("-- online manager, both objects published\n");
        Args a = good; Args ac = a; ac.c = &c2f; Args a3 = a; a3.n_poses = 3;
        CALL(online_render_scene(a)); CALL(online_probe_scene(a)); CALL(online_cast_rays(a)); CALL(online_refine_camera(a)); CALL(online_refine_camera(ac));
        CALL(online_refine_window(a)); CALL(online_refine_window(ac)); CALL(online_relocalise(a3)); CALL(online_refine_pose(a)); CALL(online_refine_pose_c2f(a));
        Args ag = a; ag.glw = glw; ag.sel = sel; Args c1 = a; c1.region = 1; c1.table = table; c1.n_comp = &n_comp;
        CALL(online_query_points(a)); CALL(online_query_lattice(a)); CALL(online_query_gradients(ag)); CALL(online_cast_normals(a));
        CALL(online_distance_lattice(a)); CALL(online_components_lattice(c1));
    }
    // ---- the lattice routes that joined later: cost fields and device-resident distance fields.  A section of its own behind the others: a handle makes a
    // stream, and the streams above keep their creation indices.  big: as above.  The stand-in runtime leaves every read-back 0: a cost field settles after
    // its first batch of sweeps, and a registration ends in its first round (status 3 under the default min_inside, status 2 under min_inside 0)
    for (int side = 0; side < 2; ++side) {
        std::printf("-- lattice routes, side %d\n", side);
        Args a = good; a.side = side; Args big = a; big.nx = 33; big.ny = 32; big.nz = 16; Args bare = a; bare.opt = false; bare.soft_weight = 0.f;
        CALL(scene_paths_lattice(a)); CALL(scene_paths_lattice(bare)); CALL(scene_paths_lattice(big));
        Args f = a;
        CALL(scene_dist_field(a)); f.field = fh; CALL(dist_field_destroy(f));
        CALL(scene_dist_field(big)); f.field = fh; CALL(dist_field_destroy(f));
    }
    {   std::printf("-- lattice routes, no side\n");
        Args a = good; Args bare = a; bare.opt = false; bare.cell_cost = nullptr;
        Args big = a; big.nx = 33; big.ny = 32; big.nz = 16; big.mask = big_mask.data(); big.cell_cost = big_cost.data(); big.fdist = big_fdist.data();
        CALL(shortest_paths(a)); CALL(shortest_paths(bare)); CALL(shortest_paths(big)); CALL(lattice_path(a));
        CALL(dist_field_create(a));
        Args f = a; f.field = fh; Args fbare = f; fbare.opt = false; Args f16 = f; f16.ways = ways16; f16.way_floats = 16;
        Args fnopiv = f; fnopiv.pivots = nullptr;
        CALL(dist_field_info(f)); CALL(dist_field_read(f)); CALL(dist_field_sample(f)); CALL(dist_field_sample(fbare));
        CALL(dist_field_score(f)); CALL(dist_field_score(f16)); CALL(dist_field_score(fbare));
        CALL(dist_field_match(f)); CALL(dist_field_match(fbare)); CALL(dist_field_match(fnopiv));
        CALL(register_default(f)); CALL(dist_field_register(f)); rp.min_inside = 0; CALL(dist_field_register(f)); CALL(dist_field_register(fbare));
        // ray tracing: range alone, every optional output, world rays, three poses; the beam score with and without its counts
        Args ftbare = fbare; Args ftworld = f; ftworld.tposes = nullptr; Args ft3 = f; ft3.n_tposes = 3; Args ft3bare = ft3; ft3bare.opt = false;
        CALL(trace_default(f)); CALL(dist_field_trace(ftbare)); CALL(dist_field_trace(f)); CALL(dist_field_trace(ftworld)); CALL(dist_field_trace(ft3));
        CALL(dist_field_beam_score(ft3)); CALL(dist_field_beam_score(ft3bare));
        CALL(dist_field_destroy(f));
        CALL(dist_field_create(big)); f.field = fh; CALL(dist_field_read(f)); CALL(dist_field_sample(f)); CALL(dist_field_destroy(f));
        Args sbig = big; sbig.val = big_val.data(); sbig.iso = 0.5f;
        CALL(signed_distance_transform(a)); CALL(signed_distance_transform(bare)); CALL(signed_distance_transform(sbig));
    }
    {   std::printf("-- lattice routes, online manager\n");
        Args a = good; Args f = a;
        CALL(online_paths_lattice(a)); CALL(online_dist_field(a)); f.field = fh; CALL(dist_field_destroy(f));
        CALL(online_signed_distance_lattice(a)); CALL(online_signed_dist_field(a)); f.field = fh; CALL(dist_field_destroy(f));
    }
    // the signed fields per side, behind every handle above: their handles' streams take the next creation indices
    for (int side = 0; side < 2; ++side) {
        std::printf("-- lattice routes, signed distance, side %d\n", side);
        Args a = good; a.side = side; Args big = a; big.nx = 33; big.ny = 32; big.nz = 16; Args bare = a; bare.opt = false; Args lg = a; lg.flags = MON_SIGNED_LOG;
        Args f = a;
        CALL(scene_signed_distance_lattice(a)); CALL(scene_signed_distance_lattice(bare)); CALL(scene_signed_distance_lattice(lg));
        CALL(scene_signed_distance_lattice(big));
        CALL(scene_signed_dist_field(a)); f.field = fh; CALL(dist_field_destroy(f));
        CALL(scene_signed_dist_field(big)); f.field = fh; CALL(dist_field_destroy(f));
    }
    // a handle for the refusals below, made untraced; its register parameters are the defaults again
    hip_stub_trace(0); OK(mon_dist_field_create(0, fdist, 3, 2, 2, origin, step, &fh)); OK(mon_register_default(fh, &rp)); OK(mon_trace_default(fh, &trp));
    hip_stub_trace(1);
    mon_dist_field* const fh_err = fh; good.field = fh_err;
    mon_register_params rp_huber0 = rp, rp_up1 = rp, rp_lambda0 = rp, rp_tol = rp, rp_evals0 = rp, rp_inside = rp;
    rp_huber0.huber = 0.f; rp_up1.lambda_up = 1.f; rp_lambda0.lambda0 = 0.f; rp_tol.tol_rot = -1.f; rp_evals0.max_evals = 0; rp_inside.min_inside = -1;
    mon_trace_params trp_tmin = trp, trp_relax0 = trp, trp_relax2 = trp, trp_step0 = trp, trp_steps0 = trp, trp_steps_many = trp, trp_nan = trp;
    trp_tmin.t_min = trp.t_max + 1.f; trp_relax0.relax = 0.f; trp_relax2.relax = 1.5f; trp_step0.step_min = 0.f; trp_steps0.max_steps = 0;
    trp_steps_many.max_steps = 4097; trp_nan.eps = NAN;

    // ---- the calls every route refuses, with code and message; the trace stays on: none of them may reach the device
    std::printf("== inference errors\n");
    OBJS_ERRS(scene_render);
    ERR(scene_render, a.Twc = nullptr); ERR(scene_render, a.rgb = nullptr); ERR(scene_render, a.depth = nullptr); ERR(scene_render, a.rect.w = 0);
    ERR(scene_render, a.rect.h = 0); ERR(scene_render, a.objs = with_null; a.rect.w = 0);
    OBJS_ERRS(scene_probe);
    ERR(scene_probe, a.poses = nullptr); ERR(scene_probe, a.q = nullptr); ERR(scene_probe, a.rgb = nullptr); ERR(scene_probe, a.depth = nullptr);
    ERR(scene_probe, a.n_poses = 0); ERR(scene_probe, a.poses = many_poses.data(); a.n_poses = 4097); ERR(scene_probe, a.n_q = 0); ERR(scene_probe, a.poses = nan_pose; a.n_poses = 1);
    ERR(scene_probe, a.q = q_nan); ERR(scene_probe, a.q = q_pose); ERR(scene_probe, a.q = q_key);
    ERR(scene_probe, a.objs = with_null; a.n_poses = 0); ERR(scene_probe, a.objs = with_null; a.n_q = 0); ERR(scene_probe, a.objs = with_null; a.q = q_nan);
    ERR(scene_probe, a.n_objs = 0; a.n_q = 0);
    OBJS_ERRS(scene_cast);
    ERR(scene_cast, a.rays = nullptr); ERR(scene_cast, a.rgb = nullptr); ERR(scene_cast, a.depth = nullptr); ERR(scene_cast, a.n_rays = 0);
    ERR(scene_cast, a.hit_opacity = 0.f); ERR(scene_cast, a.hit_opacity = 1.f); ERR(scene_cast, a.rays = r_nan); ERR(scene_cast, a.rays = r_long);
    ERR(scene_cast, a.rays = r_tmax); ERR(scene_cast, a.rays = r_key); ERR(scene_cast, a.objs = with_null; a.n_rays = 0); ERR(scene_cast, a.objs = with_null; a.rays = r_long);
    ERR(scene_cast, a.n_objs = 257; a.objs = many.data(); a.hit_opacity = 0.f);
    OBJS_ERRS(scene_pose_loss); OBS_ERRS(scene_pose_loss, obs, n_obs);
    ERR(scene_pose_loss, a.Twc = nullptr); ERR(scene_pose_loss, a.obs = two_frames); ERR(scene_pose_loss, a.lw = lw_neg);
    ERR(scene_pose_loss, a.objs = with_null; a.n_obs = 0); ERR(scene_pose_loss, a.objs = with_null; a.lw = lw_neg);
    OBJS_ERRS(scene_refine_camera); OBS_ERRS(scene_refine_camera, obs, n_obs);
    ERR(scene_refine_camera, a.pose_io = nullptr); ERR(scene_refine_camera, a.c = &c_bad); ERR(scene_refine_camera, a.objs = with_null; a.c = &c_bad);
    ERR(scene_refine_camera, a.objs = narrow; a.c = &c_bad); ERR(scene_refine_camera, a.obs = &box_noframe; a.n_obs = 1; a.c = &c_bad);
    OBJS_ERRS(scene_pose_loss_batch); OBS_ERRS(scene_pose_loss_batch, obs, n_obs);
    ERR(scene_pose_loss_batch, a.poses = nullptr); ERR(scene_pose_loss_batch, a.losses = nullptr); ERR(scene_pose_loss_batch, a.n_poses = 0);
    ERR(scene_pose_loss_batch, a.poses = many_poses.data(); a.n_poses = 4097); ERR(scene_pose_loss_batch, a.p = &p_score);
    ERR(scene_pose_loss_batch, a.objs = with_null; a.n_poses = 0); ERR(scene_pose_loss_batch, a.objs = with_null; a.p = &p_score);
    ERR(scene_pose_loss_batch, a.objs = with_null; a.n_obs = 0);
    OBJS_ERRS(scene_relocalise); OBS_ERRS(scene_relocalise, obs, n_obs);
    ERR(scene_relocalise, a.poses = nullptr); ERR(scene_relocalise, a.r = nullptr); ERR(scene_relocalise, a.pose_out = nullptr); ERR(scene_relocalise, a.n_poses = 0);
    ERR(scene_relocalise, a.poses = many_poses.data(); a.n_poses = 4097); ERR(scene_relocalise, a.r = &r_rays0); ERR(scene_relocalise, a.r = &r_rays_many);
    ERR(scene_relocalise, a.r = &r_keep0); ERR(scene_relocalise, a.r = &r_keep17); ERR(scene_relocalise, a.c = &c_bad);
    ERR(scene_relocalise, a.objs = with_null; a.r = &r_keep0); ERR(scene_relocalise, a.objs = with_null; a.r = &r_rays0); ERR(scene_relocalise, a.objs = with_null; a.n_poses = 0);
    ERR(scene_relocalise, a.objs = with_null; a.c = &c_bad); ERR(scene_relocalise, a.objs = narrow; a.c = &c_bad); ERR(scene_relocalise, a.n_obs = 0; a.r = &r_keep17);
    OBJS_ERRS(scene_window_loss); OBS_ERRS(scene_window_loss, wobs, n_wobs);
    ERR(scene_window_loss, a.wTwc = nullptr); ERR(scene_window_loss, a.wobs = frames33.data(); a.n_wobs = 33); ERR(scene_window_loss, a.wobs = apart);
    ERR(scene_window_loss, a.Tow16s = nan_Tow); ERR(scene_window_loss, a.lw = lw_neg); ERR(scene_window_loss, a.objs = with_null; a.wobs = apart);
    ERR(scene_window_loss, a.objs = with_null; a.lw = lw_neg);
    OBJS_ERRS(scene_refine_window); OBS_ERRS(scene_refine_window, wobs, n_wobs);
    ERR(scene_refine_window, a.wTwc = nullptr); ERR(scene_refine_window, a.w = nullptr); ERR(scene_refine_window, a.wobs = frames33.data(); a.n_wobs = 33);
    ERR(scene_refine_window, a.wobs = apart); ERR(scene_refine_window, a.w = &w_fixed3); ERR(scene_refine_window, a.w = &w_free); ERR(scene_refine_window, a.w = &w_lr);
    ERR(scene_refine_window, a.Tow16s = nullptr); ERR(scene_refine_window, a.Tow16s = nan_Tow); ERR(scene_refine_window, a.c = &c_bad);
    ERR(scene_refine_window, a.objs = with_null; a.c = &c_bad); ERR(scene_refine_window, a.objs = with_null; a.w = &w_free); ERR(scene_refine_window, a.objs = narrow; a.c = &c_bad);
#define OBJECT_ERRS(route) do { ERR(route, a.obj = nullptr); ERR(route, a.side = 2); ERR(route, a.obj = o_16); ERR(route, a.obj = o_xw); ERR(route, a.obj = o_un; a.side = 1); \
        ERR(route, a.obj = nullptr; a.n_obs = 0); ERR(route, a.obj = o_16; a.side = 2); ERR(route, a.obj = o_16; a.obs = &box_noframe; a.n_obs = 1); } while (0)
    OBJECT_ERRS(object_pose_loss); OBS_ERRS(object_pose_loss, obs, n_obs); ERR(object_pose_loss, a.Twc = nullptr);
    OBJECT_ERRS(object_pose_loss_levels); OBS_ERRS(object_pose_loss_levels, obs, n_obs); ERR(object_pose_loss_levels, a.Twc = nullptr);
    ERR(object_pose_loss_levels, a.lwl = nullptr); ERR(object_pose_loss_levels, a.lwl = lw_neg); ERR(object_pose_loss_levels, a.lwl = nullptr; a.n_obs = 0);
    OBJECT_ERRS(object_refine_pose); OBS_ERRS(object_refine_pose, obs, n_obs); ERR(object_refine_pose, a.pose_io = nullptr);
    OBJECT_ERRS(object_refine_pose_c2f); OBS_ERRS(object_refine_pose_c2f, obs, n_obs); ERR(object_refine_pose_c2f, a.pose_io = nullptr);
    ERR(object_refine_pose_c2f, a.cc = nullptr); ERR(object_refine_pose_c2f, a.cc = &c_bad); ERR(object_refine_pose_c2f, a.cc = &c_bad; a.obj = o_16);
    ERR(object_refine_pose_c2f, a.cc = &c_bad; a.obs = &box_noframe; a.n_obs = 1);
    // the online routes: a NULL manager, a manager none of whose objects has published, then the arguments of each
#define ONLINE_ERRS(route) do { ERR(route, a.om = nullptr); ERR(route, a.om = om_none); } while (0)
    ONLINE_ERRS(online_render_scene);
    ERR(online_render_scene, a.Twc = nullptr); ERR(online_render_scene, a.rgb = nullptr); ERR(online_render_scene, a.depth = nullptr); ERR(online_render_scene, a.rect.w = 0);
    ERR(online_render_scene, a.om = om_none; a.rect.h = 0);
    ONLINE_ERRS(online_probe_scene);
    ERR(online_probe_scene, a.poses = nullptr); ERR(online_probe_scene, a.q = nullptr); ERR(online_probe_scene, a.rgb = nullptr); ERR(online_probe_scene, a.depth = nullptr);
    ERR(online_probe_scene, a.n_poses = 0); ERR(online_probe_scene, a.poses = many_poses.data(); a.n_poses = 4097); ERR(online_probe_scene, a.n_q = 0);
    ERR(online_probe_scene, a.poses = nan_pose; a.n_poses = 1); ERR(online_probe_scene, a.q = q_nan); ERR(online_probe_scene, a.om = om_none; a.n_q = 0);
    ONLINE_ERRS(online_cast_rays);
    ERR(online_cast_rays, a.rays = nullptr); ERR(online_cast_rays, a.rgb = nullptr); ERR(online_cast_rays, a.depth = nullptr); ERR(online_cast_rays, a.n_rays = 0);
    ERR(online_cast_rays, a.hit_opacity = 0.f); ERR(online_cast_rays, a.hit_opacity = 1.f); ERR(online_cast_rays, a.rays = r_nan); ERR(online_cast_rays, a.rays = r_long);
    ERR(online_cast_rays, a.rays = r_tmax); ERR(online_cast_rays, a.om = om_none; a.n_rays = 0);
    ONLINE_ERRS(online_refine_camera); OBS_ERRS(online_refine_camera, obs, n_obs);
    ERR(online_refine_camera, a.pose_io = nullptr); ERR(online_refine_camera, a.c = &c_bad); ERR(online_refine_camera, a.obs = two_frames);
    ERR(online_refine_camera, a.om = om_none; a.c = &c_bad); ERR(online_refine_camera, a.om = om_none; a.n_obs = 0); ERR(online_refine_camera, a.om = om_none; a.p = &p_many);
    ONLINE_ERRS(online_refine_window); OBS_ERRS(online_refine_window, wobs, n_wobs);
    ERR(online_refine_window, a.wTwc = nullptr); ERR(online_refine_window, a.w = nullptr); ERR(online_refine_window, a.wobs = frames33.data(); a.n_wobs = 33);
    ERR(online_refine_window, a.wobs = apart); ERR(online_refine_window, a.w = &w_fixed3); ERR(online_refine_window, a.w = &w_free); ERR(online_refine_window, a.w = &w_lr);
    ERR(online_refine_window, a.Tow16s = nullptr); ERR(online_refine_window, a.Tow16s = nan_Tow); ERR(online_refine_window, a.c = &c_bad);
    ERR(online_refine_window, a.n_online = 3); ERR(online_refine_window, a.n_online = 3; a.om = om_none); ERR(online_refine_window, a.n_online = 3; a.w = &w_free);
    ERR(online_refine_window, a.om = om_none; a.c = &c_bad);
    ERR(online_refine_window, a.c = &c_bad; a.w = &w_free);
    ONLINE_ERRS(online_relocalise); OBS_ERRS(online_relocalise, obs, n_obs);
    ERR(online_relocalise, a.poses = nullptr); ERR(online_relocalise, a.r = nullptr); ERR(online_relocalise, a.pose_out = nullptr); ERR(online_relocalise, a.n_poses = 0);
    ERR(online_relocalise, a.poses = many_poses.data(); a.n_poses = 4097); ERR(online_relocalise, a.r = &r_rays0); ERR(online_relocalise, a.r = &r_rays_many);
    ERR(online_relocalise, a.r = &r_keep0); ERR(online_relocalise, a.r = &r_keep17); ERR(online_relocalise, a.c = &c_bad);
    ERR(online_relocalise, a.om = om_none; a.r = &r_keep0); ERR(online_relocalise, a.om = om_none; a.c = &c_bad); ERR(online_relocalise, a.n_obs = 0; a.r = &r_keep17);
    ONLINE_ERRS(online_refine_pose); OBS_ERRS(online_refine_pose, obs, n_obs);
    ERR(online_refine_pose, a.pose_io = nullptr); ERR(online_refine_pose, a.idx = 2); ERR(online_refine_pose, a.idx = 2; a.n_obs = 0);
    ONLINE_ERRS(online_refine_pose_c2f); OBS_ERRS(online_refine_pose_c2f, obs, n_obs);
    ERR(online_refine_pose_c2f, a.pose_io = nullptr); ERR(online_refine_pose_c2f, a.idx = 2); ERR(online_refine_pose_c2f, a.cc = nullptr);
    ERR(online_refine_pose_c2f, a.cc = &c_bad); ERR(online_refine_pose_c2f, a.idx = 2; a.cc = &c_bad); ERR(online_refine_pose_c2f, a.om = om_none; a.cc = &c_bad);
    // the field queries.  Their object lists need no common camera (other_K) and no common dataset (other_ds), and no sample stream is drawn (xorwow)
#define POINTS_ERRS(route, pts_, bad_) do { ERR(route, a.pts_ = nullptr); ERR(route, a.n_pts = 0); ERR(route, a.n_pts = (1u << 22) + 1u); ERR(route, a.pts_ = bad_); \
        } while (0)
#define LATTICE_ERRS(route) do { ERR(route, a.origin = nullptr); ERR(route, a.step = nullptr); ERR(route, a.nx = 0); ERR(route, a.ny = 0); ERR(route, a.nz = 0); \
        ERR(route, a.nx = 2048; a.ny = 2048; a.nz = 2); ERR(route, a.origin = origin_nan); ERR(route, a.step = step_inf); \
        ERR(route, a.origin = origin_far; a.step = step_far); } while (0)
#define WEIGHTS_ERRS(route) do { ERR(route, a.glw = lw_neg0); ERR(route, a.glw = lw_neg); } while (0)
#define OBJECT_FIELD_ERRS(route) do { ERR(route, a.obj = nullptr); ERR(route, a.side = 2); ERR(route, a.obj = o_16); ERR(route, a.obj = o_xw); \
        ERR(route, a.obj = o_un; a.side = 1); } while (0)
#define DISTANCE_ERRS(route) do { ERR(route, a.dist = nullptr); ERR(route, a.sigma_min = -1.f); ERR(route, a.sigma_min = NAN); ERR(route, a.max_dist = 0.f); } while (0)
#define COMPONENTS_ERRS(route) do { ERR(route, a.label = nullptr); ERR(route, a.sigma_min = -1.f); ERR(route, a.region = 2); ERR(route, a.region = 1; a.clearance = -1.f); \
        ERR(route, a.conn = 7); ERR(route, a.table = table); } while (0)
    OBJECT_FIELD_ERRS(object_query_points); POINTS_ERRS(object_query_points, upts, upts_out); ERR(object_query_points, a.raw4 = nullptr);
    ERR(object_query_points, a.obj = nullptr; a.n_pts = 0);
    OBJS_ERRS(scene_query_points); POINTS_ERRS(scene_query_points, pts, pts_nan); ERR(scene_query_points, a.sigma = nullptr);
    ERR(scene_query_points, a.objs = with_null; a.n_pts = 0);
    OBJS_ERRS(scene_query_lattice); LATTICE_ERRS(scene_query_lattice); ERR(scene_query_lattice, a.sigma = nullptr); ERR(scene_query_lattice, a.objs = with_null; a.nx = 0);
    OBJECT_FIELD_ERRS(object_query_gradients); POINTS_ERRS(object_query_gradients, upts, upts_out); WEIGHTS_ERRS(object_query_gradients);
    ERR(object_query_gradients, a.grad = nullptr); ERR(object_query_gradients, a.obj = o_16; a.glw = lw_neg);
    OBJS_ERRS(scene_query_gradients); POINTS_ERRS(scene_query_gradients, pts, pts_nan); WEIGHTS_ERRS(scene_query_gradients);
    ERR(scene_query_gradients, a.sigma = nullptr); ERR(scene_query_gradients, a.grad = nullptr); ERR(scene_query_gradients, a.sel = sel_2);
    ERR(scene_query_gradients, a.sel = sel_m2); ERR(scene_query_gradients, a.objs = with_null; a.sel = sel_2); ERR(scene_query_gradients, a.objs = with_null; a.glw = lw_neg);
    OBJS_ERRS(scene_query_lattice_gradients); LATTICE_ERRS(scene_query_lattice_gradients); WEIGHTS_ERRS(scene_query_lattice_gradients);
    ERR(scene_query_lattice_gradients, a.sigma = nullptr); ERR(scene_query_lattice_gradients, a.grad = nullptr);
    OBJS_ERRS(scene_cast_normals); WEIGHTS_ERRS(scene_cast_normals);
    ERR(scene_cast_normals, a.rays = nullptr); ERR(scene_cast_normals, a.rgb = nullptr); ERR(scene_cast_normals, a.depth = nullptr); ERR(scene_cast_normals, a.normal = nullptr);
    ERR(scene_cast_normals, a.n_rays = 0); ERR(scene_cast_normals, a.n_rays = (1u << 22) + 1u); ERR(scene_cast_normals, a.hit_opacity = 0.f);
    ERR(scene_cast_normals, a.rays = r_nan); ERR(scene_cast_normals, a.rays = r_long); ERR(scene_cast_normals, a.objs = with_null; a.glw = lw_neg);
    OBJS_ERRS(scene_distance_lattice); LATTICE_ERRS(scene_distance_lattice); DISTANCE_ERRS(scene_distance_lattice);
    ERR(scene_distance_lattice, a.objs = with_null; a.max_dist = 0.f);
    OBJS_ERRS(scene_components_lattice); LATTICE_ERRS(scene_components_lattice); COMPONENTS_ERRS(scene_components_lattice);
    ERR(components_with_dist, a.region = 0); ERR(scene_components_lattice, a.objs = with_null; a.conn = 7);
    ERR(distance_transform, a.mask = nullptr); ERR(distance_transform, a.step = nullptr); ERR(distance_transform, a.dist = nullptr); ERR(distance_transform, a.nx = 0);
    ERR(distance_transform, a.nx = 2048; a.ny = 2048; a.nz = 2); ERR(distance_transform, a.step = step_inf); ERR(distance_transform, a.max_dist = 0.f);
    ERR(label_components, a.mask = nullptr); ERR(label_components, a.label = nullptr); ERR(label_components, a.nz = 0); ERR(label_components, a.nx = 2048; a.ny = 2048; a.nz = 2);
    ERR(label_components, a.conn = 7); ERR(label_components, a.table = table);
    LATTICE_ERRS(lattice_points); ERR(lattice_points, a.xyz_out = nullptr);
    ERR(camera_rays, a.poses = nullptr); ERR(camera_rays, a.q = nullptr); ERR(camera_rays, a.rays_out = nullptr); ERR(camera_rays, a.n_poses = 0); ERR(camera_rays, a.n_q = 0);
    ERR(camera_rays, a.poses = nan_pose; a.n_poses = 1); ERR(camera_rays, a.q = q_nan); ERR(camera_rays, a.q = q_pose);
    ONLINE_ERRS(online_query_points); POINTS_ERRS(online_query_points, pts, pts_nan); ERR(online_query_points, a.sigma = nullptr);
    ERR(online_query_points, a.om = om_none; a.n_pts = 0);
    ONLINE_ERRS(online_query_lattice); LATTICE_ERRS(online_query_lattice); ERR(online_query_lattice, a.sigma = nullptr);
    ONLINE_ERRS(online_query_gradients); POINTS_ERRS(online_query_gradients, pts, pts_nan); WEIGHTS_ERRS(online_query_gradients);
    ERR(online_query_gradients, a.sigma = nullptr); ERR(online_query_gradients, a.grad = nullptr); ERR(online_query_gradients, a.sel = sel_2);
    ERR(online_query_gradients, a.sel = sel_m2); ERR(online_query_gradients, a.om = om_none; a.sel = sel_2);
    ONLINE_ERRS(online_cast_normals); WEIGHTS_ERRS(online_cast_normals);
    ERR(online_cast_normals, a.rays = nullptr); ERR(online_cast_normals, a.rgb = nullptr); ERR(online_cast_normals, a.depth = nullptr); ERR(online_cast_normals, a.normal = nullptr);
    ERR(online_cast_normals, a.n_rays = 0); ERR(online_cast_normals, a.hit_opacity = 1.f); ERR(online_cast_normals, a.rays = r_tmax);
    ONLINE_ERRS(online_distance_lattice); LATTICE_ERRS(online_distance_lattice); DISTANCE_ERRS(online_distance_lattice);
    ONLINE_ERRS(online_components_lattice); LATTICE_ERRS(online_components_lattice); COMPONENTS_ERRS(online_components_lattice);
    ERR(online_components_lattice, a.om = om_none; a.region = 2);
    // the cost fields and the device-resident distance fields (good.field: a live handle)
#define PATHS_ERRS(route) do { ERR(route, a.cost = nullptr); ERR(route, a.seeds = nullptr); ERR(route, a.conn = 7); ERR(route, a.max_cost = 0.f); ERR(route, a.n_seeds = 0); \
        ERR(route, a.n_seeds = (1u << 22) + 1u); ERR(route, a.seeds = seeds_out); } while (0)
#define SCENE_PATHS_ERRS(route) do { ERR(route, a.sigma_min = -1.f); ERR(route, a.clearance = -1.f); ERR(route, a.clearance = NAN); ERR(route, a.soft_weight = -1.f); \
        ERR(route, a.soft_radius = 0.f); } while (0)
#define FIELD_ERRS(route) do { ERR(route, a.field_out = nullptr); ERR(route, a.sigma_min = -1.f); ERR(route, a.field_max = 0.f); ERR(route, a.field_max = INFINITY); \
        ERR(route, a.step = step_zero); } while (0)
    ERR(shortest_paths, a.mask = nullptr); ERR(shortest_paths, a.step = nullptr); ERR(shortest_paths, a.nx = 0); ERR(shortest_paths, a.nx = 2048; a.ny = 2048; a.nz = 2);
    ERR(shortest_paths, a.step = step_inf); PATHS_ERRS(shortest_paths); ERR(shortest_paths, a.cell_cost = cost_neg); ERR(shortest_paths, a.mask = nullptr; a.conn = 7);
    OBJS_ERRS(scene_paths_lattice); LATTICE_ERRS(scene_paths_lattice); SCENE_PATHS_ERRS(scene_paths_lattice); PATHS_ERRS(scene_paths_lattice);
    ERR(scene_paths_lattice, a.objs = with_null; a.conn = 7); ERR(scene_paths_lattice, a.objs = with_null; a.seeds = seeds_out);
    ONLINE_ERRS(online_paths_lattice); LATTICE_ERRS(online_paths_lattice); SCENE_PATHS_ERRS(online_paths_lattice); PATHS_ERRS(online_paths_lattice);
    ERR(online_paths_lattice, a.om = om_none; a.max_cost = 0.f);
    ERR(lattice_path, a.next = nullptr); ERR(lattice_path, a.n_path = nullptr); ERR(lattice_path, a.path = nullptr); ERR(lattice_path, a.start = -1);
    ERR(lattice_path, a.start = 4); ERR(lattice_path, a.next = next_cycle); ERR(lattice_path, a.next = next_bad);
    ERR(dist_field_create, a.field_out = nullptr); ERR(dist_field_create, a.fdist = nullptr); ERR(dist_field_create, a.origin = nullptr);
    ERR(dist_field_create, a.step = nullptr); ERR(dist_field_create, a.nx = 0); ERR(dist_field_create, a.nx = 2048; a.ny = 2048; a.nz = 2);
    ERR(dist_field_create, a.origin = origin_nan); ERR(dist_field_create, a.step = step_inf); ERR(dist_field_create, a.step = step_zero);
    ERR(dist_field_create, a.fdist = fdist_nan); ERR(dist_field_create, a.field_out = nullptr; a.nx = 0);
    OBJS_ERRS(scene_dist_field); LATTICE_ERRS(scene_dist_field); FIELD_ERRS(scene_dist_field); ERR(scene_dist_field, a.objs = with_null; a.field_max = INFINITY);
    ONLINE_ERRS(online_dist_field); LATTICE_ERRS(online_dist_field); FIELD_ERRS(online_dist_field); ERR(online_dist_field, a.om = om_none; a.field_max = 0.f);
    ERR(dist_field_info, a.field = nullptr); ERR(dist_field_info, a.info = nullptr); ERR(dist_field_read, a.field = nullptr); ERR(dist_field_read, a.dist = nullptr);
    ERR(dist_field_destroy, a.field = nullptr);
    ERR(dist_field_sample, a.pts = nullptr); ERR(dist_field_sample, a.dist = nullptr); ERR(dist_field_sample, a.n_pts = 0); ERR(dist_field_sample, a.n_pts = (1u << 24) + 1u);
    ERR(dist_field_sample, a.field = nullptr); ERR(dist_field_sample, a.field = nullptr; a.n_pts = 0);
    ERR(dist_field_score, a.spheres = nullptr); ERR(dist_field_score, a.ways = nullptr); ERR(dist_field_score, a.tp = nullptr); ERR(dist_field_score, a.min_clear = nullptr);
    ERR(dist_field_score, a.n_spheres = 0); ERR(dist_field_score, a.n_spheres = 33); ERR(dist_field_score, a.way_floats = 4); ERR(dist_field_score, a.n_way = 0);
    ERR(dist_field_score, a.n_way = 257); ERR(dist_field_score, a.n_sub = 0); ERR(dist_field_score, a.n_sub = 17); ERR(dist_field_score, a.n_traj = 0);
    ERR(dist_field_score, a.n_traj = 65537); ERR(dist_field_score, a.n_traj = 65536; a.n_way = 256; a.n_sub = 16); ERR(dist_field_score, a.spheres = sphere_neg);
    ERR(dist_field_score, a.tp = &tp_nan); ERR(dist_field_score, a.field = nullptr); ERR(dist_field_score, a.field = nullptr; a.way_floats = 4);
#define MATCH_ERRS(route) do { ERR(route, a.pts = nullptr); ERR(route, a.mposes = nullptr); ERR(route, a.cost = nullptr); ERR(route, a.n_pts = 0); \
        ERR(route, a.n_pts = (1u << 20) + 1u); ERR(route, a.n_h = 0); ERR(route, a.mposes = many_poses.data(); a.n_h = 4097); ERR(route, a.n_pts = 1u << 20; a.n_h = 65); \
        ERR(route, a.mposes = pose_nan3); ERR(route, a.field = nullptr); ERR(route, a.field = nullptr; a.n_h = 0); } while (0)
    MATCH_ERRS(dist_field_match); ERR(dist_field_match, a.mp = nullptr); ERR(dist_field_match, a.pivots = pivots_nan); ERR(dist_field_match, a.mp = &mp_huber0);
    ERR(dist_field_match, a.mp = &mp_nan); ERR(dist_field_match, a.field = nullptr; a.mp = &mp_huber0);
    ERR(register_default, a.rp = nullptr); ERR(register_default, a.field = nullptr);
    MATCH_ERRS(dist_field_register); ERR(dist_field_register, a.rp = nullptr); ERR(dist_field_register, a.poses_out = nullptr); ERR(dist_field_register, a.rp = &rp_huber0);
    ERR(dist_field_register, a.rp = &rp_up1); ERR(dist_field_register, a.rp = &rp_lambda0); ERR(dist_field_register, a.rp = &rp_tol); ERR(dist_field_register, a.rp = &rp_evals0);
    ERR(dist_field_register, a.rp = &rp_inside); ERR(dist_field_register, a.field = nullptr; a.rp = &rp_up1);
    // ray tracing (kTraceMaxRays 2^20, kTraceMaxPoses 4 096, kTraceMaxHome 2^22, kTraceMaxBeams 2^24, max_steps 1 to 4 096) and the signed fields
#define TRACE_ERRS(route) do { ERR(route, a.frays = nullptr); ERR(route, a.trp = nullptr); ERR(route, a.n_frays = 0); ERR(route, a.n_frays = (1u << 20) + 1u); \
        ERR(route, a.n_tposes = 0); ERR(route, a.tposes = many_poses.data(); a.n_tposes = 4097); ERR(route, a.tposes = nullptr; a.n_tposes = 2); \
        ERR(route, a.tposes = pose_nan3; a.n_tposes = 3); ERR(route, a.trp = &trp_nan); ERR(route, a.trp = &trp_tmin); ERR(route, a.trp = &trp_step0); \
        ERR(route, a.trp = &trp_relax0); ERR(route, a.trp = &trp_relax2); ERR(route, a.trp = &trp_steps0); ERR(route, a.trp = &trp_steps_many); \
        ERR(route, a.field = nullptr); ERR(route, a.field = nullptr; a.n_frays = 0); } while (0)
    ERR(trace_default, a.trp = nullptr); ERR(trace_default, a.field = nullptr);
    TRACE_ERRS(dist_field_trace); ERR(dist_field_trace, a.range = nullptr);
    ERR(dist_field_trace, a.n_frays = 1u << 20; a.tposes = many_poses.data(); a.n_tposes = 5);
    TRACE_ERRS(dist_field_beam_score); ERR(dist_field_beam_score, a.measured = nullptr); ERR(dist_field_beam_score, a.bp = nullptr); ERR(dist_field_beam_score, a.cost = nullptr);
    ERR(dist_field_beam_score, a.n_frays = 1u << 20; a.tposes = many_poses.data(); a.n_tposes = 17); ERR(dist_field_beam_score, a.bp = &bp_huber0);
    ERR(dist_field_beam_score, a.field = nullptr; a.bp = &bp_huber0);
#define SIGNED_ERRS(route) do { ERR(route, a.dist = nullptr); ERR(route, a.sigma_min = -1.f); ERR(route, a.sigma_min = NAN); ERR(route, a.flags = 2u); \
        ERR(route, a.max_dist = 0.f); } while (0)
#define SIGNED_FIELD_ERRS(route) do { FIELD_ERRS(route); ERR(route, a.flags = 2u); } while (0)
    ERR(signed_distance_transform, a.val = nullptr); ERR(signed_distance_transform, a.step = nullptr); ERR(signed_distance_transform, a.dist = nullptr);
    ERR(signed_distance_transform, a.nx = 0); ERR(signed_distance_transform, a.nx = 2048; a.ny = 2048; a.nz = 2); ERR(signed_distance_transform, a.step = step_inf);
    ERR(signed_distance_transform, a.iso = NAN); ERR(signed_distance_transform, a.max_dist = 0.f); ERR(signed_distance_transform, a.val = nullptr; a.iso = NAN);
    OBJS_ERRS(scene_signed_distance_lattice); LATTICE_ERRS(scene_signed_distance_lattice); SIGNED_ERRS(scene_signed_distance_lattice);
    ERR(scene_signed_distance_lattice, a.objs = with_null; a.flags = 2u);
    OBJS_ERRS(scene_signed_dist_field); LATTICE_ERRS(scene_signed_dist_field); SIGNED_FIELD_ERRS(scene_signed_dist_field);
    ERR(scene_signed_dist_field, a.objs = with_null; a.field_max = INFINITY);
    ONLINE_ERRS(online_signed_distance_lattice); LATTICE_ERRS(online_signed_distance_lattice); SIGNED_ERRS(online_signed_distance_lattice);
    ONLINE_ERRS(online_signed_dist_field); LATTICE_ERRS(online_signed_dist_field); SIGNED_FIELD_ERRS(online_signed_dist_field);
    ERR(online_signed_dist_field, a.om = om_none; a.field_max = 0.f);
    hip_stub_trace(0);
    OK(mon_dist_field_destroy(fh_err));
    // (the trace ends here: two object threads sign off on stdout in the order they happen to end)
    std::fflush(stdout); if (!std::freopen("/dev/null", "w", stdout)) std::exit(3);
    OK(mon_online_wait_threads_end(om)); OK(mon_online_destroy(om)); OK(mon_online_wait_threads_end(om_none)); OK(mon_online_destroy(om_none));
    for (mon_object* x : { o0, o1, o_K, o_2, o_16, o_xw, o_un }) OK(mon_object_destroy(x));
    for (mon_dataset* d : { ds, ds_K, ds_2 }) OK(mon_dataset_destroy(d));
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
    inference_part(argv[2], base, rgb.data(), inst.data());
    hip_stub_trace(0);
    return 0;
}
