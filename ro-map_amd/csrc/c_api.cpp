// c_api.cpp -- extern "C" surface declared in include/mon_core.h.  The scene and pose routes enter through the boundary of model.h: their checks are in
// scene.cpp, scene_field.cpp, scene_pose.cpp and pose.cpp, shared with manager.cpp and diag.cpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "model.h"
#include "frag_layout.h"

// ---- coarse-to-fine level weights (include/mon_core.h): the checks of a schedule, one row of weights, the table of a whole refinement
namespace mon {
int pose_c2f_check(const mon_pose_c2f_params* c) {
    if (!c) { set_error("pose c2f: null params"); return MON_ERR_ARG; }
    if (!std::isfinite(c->level_start) || !std::isfinite(c->level_end) || !std::isfinite(c->ramp)) { set_error("pose c2f: a non-finite parameter"); return MON_ERR_ARG; }
    if (c->level_start < 0.f || c->level_end < c->level_start) { set_error("pose c2f: level_start %g, level_end %g (0 <= start <= end)", c->level_start,
            c->level_end); return MON_ERR_ARG; }
    if (!(c->ramp > 0.f && c->ramp <= 1.f)) { set_error("pose c2f: ramp %g outside (0, 1]", c->ramp); return MON_ERR_ARG; }
    return MON_OK;
}
// the window and schedule of include/mon_core.h, in double, rounded once to float (also the table of mon_object_refine_pose_c2f)
static void c2f_row(const mon_pose_c2f_params& c, int n_levels, int iters, int step, float* w) {
    const double f = std::min(1.0, (double)step / ((double)c.ramp * (double)iters));
    const double alpha = (double)c.level_start + ((double)c.level_end - (double)c.level_start) * f;
    for (int l = 0; l < n_levels; ++l) {
        const double a = alpha - l;
        w[l] = a <= 0.0 ? 0.f : a >= 1.0 ? 1.f : (float)((1.0 - std::cos(M_PI * a)) / 2.0);
    }
}
// the [iters][L] weight table of a scheduled refinement (empty for iters 0)
std::vector<float> pose_c2f_table(const mon_pose_c2f_params& c, int n_levels, int iters) {
    std::vector<float> t((size_t)iters * n_levels);
    for (int i = 0; i < iters; ++i) c2f_row(c, n_levels, iters, i, t.data() + (size_t)i * n_levels);
    return t;
}
}  // namespace mon

using namespace mon;


#define REQUIRE(p, what) do { if (!(p)) { set_error("%s: null %s", __func__, what); return MON_ERR_ARG; } } while (0)

extern "C" {

const char* mon_last_error(void) { return last_error(); }
int mon_version(void) { return 100; }
int mon_device_count(int* n) { REQUIRE(n, "n_devices"); return device_count(n); }
int mon_set_logical_devices(int n) { return set_logical_devices(n); }
int mon_offline_set_schedule(int outer, int inner) {
    if (outer < 1 || inner < 1) { set_error("offline_set_schedule: %d x %d", outer, inner); return MON_ERR_ARG; }
    options().offline_outer = outer; options().offline_inner = inner; return MON_OK;
}
int mon_set_option(const char* name, long value) { return option_set(name, value); }
int mon_get_option(const char* name, long* value) { return option_get(name, value); }
int mon_config_default(mon_config* cfg) { REQUIRE(cfg, "cfg"); config_default(*cfg); return MON_OK; }
int mon_config_from_json(const char* path, mon_config* cfg) { REQUIRE(path, "path"); REQUIRE(cfg, "cfg"); return config_from_json(path, *cfg); }

int mon_dataset_create(int device, int H, int W, float fx, float fy, float cx, float cy, uint32_t max_frames, int use_depth, mon_dataset** out) {
    REQUIRE(out, "out"); Dataset* d = nullptr;
    int rc = dataset_create(device, H, W, fx, fy, cx, cy, max_frames, use_depth, &d); if (rc) return rc;
    *out = new mon_dataset{ d }; return MON_OK;
}
int mon_dataset_add_frame(mon_dataset* ds, uint32_t frame_id, const uint8_t* rgb, int channels, int is_bgr, const uint8_t* instance, const float* depth,
        const float* Twc16) {
    REQUIRE(ds, "dataset"); return dataset_add_frame(ds->d, frame_id, rgb, channels, is_bgr, instance, depth, Twc16);
}
int mon_dataset_n_frames(const mon_dataset* ds, uint32_t* n) { REQUIRE(ds, "dataset"); REQUIRE(n, "n"); *n = ds->d->n_frames; return MON_OK; }
int mon_dataset_destroy(mon_dataset* ds) { if (!ds) return MON_OK; dataset_destroy(ds->d); delete ds; return MON_OK; }

int mon_object_create(mon_dataset* ds, const mon_config* cfg, int class_id, const float* Tow16, const float* aabb_min3, const float* aabb_max3,
        mon_object** out) {
    REQUIRE(ds, "dataset"); REQUIRE(cfg, "cfg"); REQUIRE(out, "out"); Model* m = nullptr;
    int rc = model_create(ds->d, *cfg, class_id, Tow16, aabb_min3, aabb_max3, &m); if (rc) return rc;
    *out = new mon_object{ m }; return MON_OK;
}
int mon_object_add_boxes(mon_object* o, const mon_frame_bbox* boxes, size_t n) { REQUIRE(o, "object"); return model_add_boxes(*o->m, boxes, n); }
int mon_object_train(mon_object* o, int iters, float* loss) { REQUIRE(o, "object"); return model_train(*o->m, iters, loss, 7); }
int mon_object_train_stages(mon_object* o, int stage_bits) { REQUIRE(o, "object"); return model_train(*o->m, 1, nullptr, stage_bits & 7); }
int mon_object_render(mon_object* o, mon_frame_bbox box, const float* pose16, int pose_is_Toc, float* rgb, float* depth, float* mask, int dst_on_device) {
    REQUIRE(o, "object"); return model_render(*o->m, box, pose16, pose_is_Toc, rgb, depth, mask, dst_on_device);
}
int mon_object_render_snapshot(mon_object* o, mon_frame_bbox box, const float* pose16, int pose_is_Toc, float* rgb, float* depth, float* mask,
        uint32_t* snapshot_step) {
    REQUIRE(o, "object"); return model_render_snapshot(*o->m, box, pose16, pose_is_Toc, rgb, depth, mask, snapshot_step);
}
int mon_object_generate_mesh(mon_object* o, int res, float thresh, uint32_t* n_verts, uint32_t* n_indices) { REQUIRE(o, "object");
    return model_generate_mesh(*o->m, res, thresh, n_verts, n_indices); }
int mon_object_mesh_counts(mon_object* o, uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices) { REQUIRE(o, "object");
    return model_mesh_counts(*o->m, n_verts, n_verts_real, n_indices); }
int mon_object_get_mesh(mon_object* o, float* verts, float* normals, uint8_t* colors, uint32_t* indices, int try_lock_only) { REQUIRE(o, "object");
    return model_get_mesh(*o->m, verts, normals, colors, indices, nullptr, nullptr, try_lock_only); }
int mon_object_get_mesh_raw(mon_object* o, float* normals_raw, float* colors_f32) { REQUIRE(o, "object");
    return model_get_mesh(*o->m, nullptr, nullptr, nullptr, nullptr, normals_raw, colors_f32, 0); }
int mon_object_copy_mesh(mon_object* o, uint32_t cap_verts, uint32_t cap_indices, float* verts, float* normals, uint8_t* colors, uint32_t* indices,
                         uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices, int try_lock_only) {
    REQUIRE(o, "object");
    return model_copy_mesh(*o->m, cap_verts, cap_indices, verts, normals, colors, indices, n_verts, n_verts_real, n_indices, try_lock_only);
}
int mon_object_mesh_generation(mon_object* o, uint64_t* generation) { REQUIRE(o, "object"); REQUIRE(generation, "generation");
    return model_mesh_generation(*o->m, generation); }
int mon_object_save_mesh(mon_object* o, const char* path) { REQUIRE(o, "object"); REQUIRE(path, "path"); return model_save_mesh(*o->m, path); }
int mon_marching_cubes(int device, const float* density, int rx, int ry, int rz, float thresh, const float* aabb_min3, const float* aabb_max3,
                       float* verts, float* normals_raw, uint32_t* indices, uint32_t cap_verts, uint32_t cap_indices, uint32_t* n_verts,
                               uint32_t* n_verts_real, uint32_t* n_indices) {
    return marching_cubes_host(device, density, rx, ry, rz, thresh, aabb_min3, aabb_max3, verts, normals_raw, indices, cap_verts, cap_indices, n_verts,
            n_verts_real, n_indices);
}
int mon_object_set_render_skip(mon_object* o, int enable, float min_alpha) { REQUIRE(o, "object"); return model_set_render_skip(*o->m, enable, min_alpha); }
int mon_object_render_skip_stats(mon_object* o, int side, mon_render_skip_stats* out) { REQUIRE(o, "object"); REQUIRE(out, "out");
    return model_render_skip_stats(*o->m, side, out); }
int mon_object_render_occupancy(mon_object* o, int side, int dilated, uint32_t* bits) { REQUIRE(o, "object"); REQUIRE(bits, "bits");
    return model_render_occupancy(*o->m, side, dilated, bits); }
// ---- the scene routes, each in the four steps of model.h's boundary: its check, the models, its objects' check, the route
int mon_scene_render(mon_object* const* objs, size_t n_objs, int side, mon_frame_bbox rect, const float* Twc16, float* rgb, float* depth, float* opacity,
        int32_t* instance) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_render_check(side, rect, Twc16)) || (rc = scene_render_outputs_check(rgb, depth)) || (rc = scene_models("scene_render", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_render", ms.data(), n_objs))) return rc;
    return scene_render(ms.data(), n_objs, side, rect, Twc16, rgb, depth, opacity, instance, nullptr, nullptr);
}
int mon_scene_probe(mon_object* const* objs, size_t n_objs, int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q, float* rgb,
        float* depth, float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_probe_check(side, Twc16s, n_poses, q, n_q, rgb, depth)) || (rc = scene_models("scene_probe", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_probe", ms.data(), n_objs))) return rc;
    return scene_probe(ms.data(), n_objs, side, Twc16s, n_poses, q, n_q, rgb, depth, opacity, instance, hit_depth, hit_instance, nullptr, nullptr);
}
int mon_scene_cast(mon_object* const* objs, size_t n_objs, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, float* rgb, float* dist,
        float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_cast_check(side, rays, n_rays, hit_opacity, rgb, dist)) || (rc = scene_models("scene_cast", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_cast", ms.data(), n_objs, false))) return rc;
    return scene_cast(ms.data(), n_objs, side, rays, n_rays, hit_opacity, rgb, dist, opacity, instance, hit_t, hit_sample_t, hit_instance, nullptr, nullptr);
}
int mon_camera_rays(float fx, float fy, float cx, float cy, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q, mon_scene_ray* rays_out,
        float* dn_out) {
    return scene_camera_rays(fx, fy, cx, cy, Twc16s, n_poses, q, n_q, rays_out, dn_out);
}
int mon_object_query_points(mon_object* o, int side, const float* unit_xyz, size_t n, float* raw4) {
    { const int rc = object_points_check(side, unit_xyz, n, raw4); if (rc) return rc; }
    REQUIRE(o, "object");
    return object_points(*o->m, side, unit_xyz, n, raw4);
}
int mon_scene_query_points(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, float* sigma, float* rgb, int32_t* owner,
        float* owner_sigma, uint32_t* n_inside) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_points_check(side, world_xyz, n, sigma)) || (rc = scene_models("scene_points", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_points", ms.data(), n_objs, false))) return rc;
    const ScenePoints q = scene_point_list(world_xyz, n);
    return scene_points(ms.data(), n_objs, side, q, sigma, rgb, owner, owner_sigma, n_inside, nullptr, 0, nullptr);
}
int mon_scene_query_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz, float* sigma,
        float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_lattice_check(side, origin3, step3, nx, ny, nz, sigma)) || (rc = scene_models("scene_lattice", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_lattice", ms.data(), n_objs, false))) return rc;
    const ScenePoints q = scene_lattice(origin3, step3, nx, ny, nz);
    return scene_points(ms.data(), n_objs, side, q, sigma, rgb, owner, owner_sigma, n_inside, nullptr, 0, nullptr);
}
int mon_lattice_points(const float* origin3, const float* step3, int nx, int ny, int nz, float* xyz_out) {
    return scene_lattice_points(origin3, step3, nx, ny, nz, xyz_out);
}
int mon_distance_transform(int device, const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, float* dist, int32_t* nearest) {
    { const int rc = distance_transform_check(occupied, nx, ny, nz, step3, max_dist, dist); if (rc) return rc; }
    return distance_transform(device, occupied, nx, ny, nz, step3, max_dist, dist, nearest);
}
int mon_scene_distance_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
        float sigma_min, float max_dist, float* dist, int32_t* nearest, int32_t* nearest_owner, float* free_dist, float* sigma) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_distance_check(side, origin3, step3, nx, ny, nz, sigma_min, max_dist, dist)) || (rc = scene_models("scene_distance", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_distance", ms.data(), n_objs, false))) return rc;
    return scene_distance(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), sigma_min, max_dist, dist, nearest, nearest_owner, free_dist, sigma,
                          nullptr);
}
int mon_label_components(int device, const uint8_t* mask, int nx, int ny, int nz, int connectivity, int32_t* label, int32_t* comp,
        mon_lattice_component* table, uint32_t cap, uint32_t* n_components) {
    { const int rc = label_components_check(mask, nx, ny, nz, connectivity, label, table, n_components); if (rc) return rc; }
    return label_components(device, mask, nx, ny, nz, connectivity, label, comp, table, cap, n_components);
}
int mon_scene_components_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
        float sigma_min, int region, float clearance, int connectivity, int32_t* label, int32_t* comp, mon_lattice_component* table, uint32_t cap,
        uint32_t* n_components, float* dist, float* sigma, int32_t* owner) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_components_check(side, origin3, step3, nx, ny, nz, sigma_min, region, clearance, connectivity, label, table, n_components, dist)) ||
        (rc = scene_models("scene_components", objs, n_objs, ms)) || (rc = scene_objects_check("scene_components", ms.data(), n_objs, false))) return rc;
    return scene_components(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), sigma_min, region, clearance, connectivity, label, comp, table,
                            cap, n_components, dist, sigma, owner, nullptr);
}
int mon_shortest_paths(int device, const uint8_t* passable, int nx, int ny, int nz, const float* step3, int connectivity, const float* cell_cost,
        const int32_t* seeds, size_t n_seeds, float max_cost, float* cost, int32_t* next) {
    { const int rc = shortest_paths_check(passable, nx, ny, nz, step3, connectivity, cell_cost, seeds, n_seeds, max_cost, cost); if (rc) return rc; }
    return shortest_paths(device, passable, nx, ny, nz, step3, connectivity, cell_cost, seeds, n_seeds, max_cost, cost, next);
}
int mon_scene_paths_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min,
        float clearance, float soft_radius, float soft_weight, int connectivity, const int32_t* seeds, size_t n_seeds, float max_cost, float* cost,
        int32_t* next, float* dist, float* sigma, int32_t* owner) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_paths_check(side, origin3, step3, nx, ny, nz, sigma_min, clearance, soft_radius, soft_weight, connectivity, seeds, n_seeds, max_cost, cost)) ||
        (rc = scene_models("scene_paths", objs, n_objs, ms)) || (rc = scene_objects_check("scene_paths", ms.data(), n_objs, false))) return rc;
    return scene_paths(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), sigma_min, clearance, soft_radius, soft_weight, connectivity, seeds,
                       n_seeds, max_cost, cost, next, dist, sigma, owner, nullptr);
}
int mon_lattice_path(const int32_t* next, size_t n_cells, int32_t start, int32_t* path, size_t cap, size_t* n_path) {
    return lattice_path(next, n_cells, start, path, cap, n_path);
}
int mon_dist_field_create(int device, const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, mon_dist_field** field) {
    { const int rc = dist_field_create_check(dist, nx, ny, nz, origin3, step3, field); if (rc) return rc; }
    DistField* f = nullptr;
    { const int rc = dist_field_create(device, dist, nx, ny, nz, origin3, step3, &f); if (rc) return rc; }
    *field = new mon_dist_field{ f }; return MON_OK;
}
int mon_scene_dist_field(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min,
        float max_dist, mon_dist_field** field) {
    std::vector<Model*> ms; int rc; DistField* f = nullptr;
    if ((rc = scene_dist_field_check(side, origin3, step3, nx, ny, nz, sigma_min, max_dist, field)) || (rc = scene_models("scene_dist_field", objs, n_objs, ms)) ||
        (rc = scene_objects_check("scene_dist_field", ms.data(), n_objs, false)) ||
        (rc = scene_dist_field(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), sigma_min, max_dist, &f))) return rc;
    *field = new mon_dist_field{ f }; return MON_OK;
}
int mon_signed_distance_transform(int device, const float* val, float iso, int nx, int ny, int nz, const float* step3, float max_dist, float* sdist,
        int32_t* nearest_edge) {
    { const int rc = signed_distance_transform_check(val, iso, nx, ny, nz, step3, max_dist, sdist); if (rc) return rc; }
    return signed_distance_transform(device, val, iso, nx, ny, nz, step3, max_dist, sdist, nearest_edge);
}
int mon_scene_signed_distance_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
        float sigma_min, uint32_t flags, float max_dist, float* sdist, int32_t* nearest_edge, int32_t* nearest_owner, float* sigma, float* val, float* iso_out) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_signed_distance_check(side, origin3, step3, nx, ny, nz, sigma_min, flags, max_dist, sdist)) ||
        (rc = scene_models("scene_signed_distance", objs, n_objs, ms)) || (rc = scene_objects_check("scene_signed_distance", ms.data(), n_objs, false))) return rc;
    return scene_signed_distance(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), sigma_min, flags, max_dist, sdist, nearest_edge,
                                 nearest_owner, sigma, val, iso_out, nullptr);
}
int mon_scene_signed_dist_field(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
        float sigma_min, uint32_t flags, float max_dist, mon_dist_field** field) {
    std::vector<Model*> ms; int rc; DistField* f = nullptr;
    if ((rc = scene_signed_dist_field_check(side, origin3, step3, nx, ny, nz, sigma_min, flags, max_dist, field)) ||
        (rc = scene_models("scene_signed_dist_field", objs, n_objs, ms)) || (rc = scene_objects_check("scene_signed_dist_field", ms.data(), n_objs, false)) ||
        (rc = scene_signed_dist_field(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), sigma_min, flags, max_dist, &f))) return rc;
    *field = new mon_dist_field{ f }; return MON_OK;
}
int mon_dist_field_info(mon_dist_field* field, mon_dist_field_desc* info) { return dist_field_info(field ? field->f : nullptr, info); }
int mon_dist_field_read(mon_dist_field* field, float* dist_out) { return dist_field_read(field ? field->f : nullptr, dist_out); }
int mon_dist_field_sample(mon_dist_field* field, const float* xyz, size_t n, float outside, float* dist_out, float* grad3_out) {
    return dist_field_sample(field ? field->f : nullptr, xyz, n, outside, dist_out, grad3_out);
}
int mon_dist_field_score(mon_dist_field* field, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj, size_t n_way,
        size_t n_sub, const mon_traj_score_params* params, float* min_clear, int32_t* first_hit, float* cost, float* way_clear, float* way_grad) {
    return dist_field_score(field ? field->f : nullptr, spheres, n_spheres, ways, way_floats, n_traj, n_way, n_sub, params, min_clear, first_hit, cost, way_clear,
                            way_grad);
}
int mon_dist_field_destroy(mon_dist_field* field) { if (field) { dist_field_free(field->f); delete field; } return MON_OK; }
int mon_dist_field_match(mon_dist_field* field, const float* points, size_t n, const float* poses16, size_t n_poses, const float* pivots,
        const mon_scan_match_params* params, float* cost, int32_t* n_inside, int32_t* n_inlier, float* normal) {
    return dist_field_match(field ? field->f : nullptr, points, n, poses16, n_poses, pivots, params, cost, n_inside, n_inlier, normal);
}
int mon_trace_default(mon_dist_field* field, mon_trace_params* p) { return dist_field_trace_default(field ? field->f : nullptr, p); }
int mon_dist_field_trace(mon_dist_field* field, const float* rays, size_t n, const float* poses16, size_t n_poses, const mon_trace_params* p, float* range,
        int32_t* status, int32_t* steps, float* normal3) {
    return dist_field_trace(field ? field->f : nullptr, rays, n, poses16, n_poses, p, range, status, steps, normal3);
}
int mon_dist_field_beam_score(mon_dist_field* field, const float* rays, size_t n, const float* measured, const float* poses16, size_t n_poses,
        const mon_trace_params* p, const mon_beam_params* b, float* cost, int32_t* n_valid, int32_t* n_hit) {
    return dist_field_beam_score(field ? field->f : nullptr, rays, n, measured, poses16, n_poses, p, b, cost, n_valid, n_hit);
}
int mon_register_default(mon_dist_field* field, mon_register_params* p) { return dist_field_register_default(field ? field->f : nullptr, p); }
int mon_dist_field_register(mon_dist_field* field, const float* points, size_t n, const float* poses16_in, size_t n_poses, const mon_register_params* p,
        float* poses16_out, float* cost, int32_t* n_inside, int32_t* n_inlier, int32_t* evals, int32_t* status, int32_t* best) {
    return dist_field_register(field ? field->f : nullptr, points, n, poses16_in, n_poses, p, poses16_out, cost, n_inside, n_inlier, evals, status, best);
}
int mon_object_query_gradients(mon_object* o, int side, const float* unit_xyz, size_t n, const float* level_weights, float* raw4, float* grad_unit) {
    { const int rc = object_gradients_check(side, unit_xyz, n, level_weights, grad_unit); if (rc) return rc; }
    REQUIRE(o, "object");
    return object_gradients(*o->m, side, unit_xyz, n, level_weights, raw4, grad_unit);
}
int mon_scene_query_gradients(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, const float* level_weights,
        const int32_t* select, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma,
        float* normal) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_gradients_check(side, world_xyz, n, level_weights, select, n_objs, sigma, grad_log)) ||
        (rc = scene_models("scene_gradients", objs, n_objs, ms)) || (rc = scene_objects_check("scene_gradients", ms.data(), n_objs, false)) ||
        (rc = scene_gradients_weights_check(ms.data(), n_objs, level_weights))) return rc;
    const ScenePoints q = scene_point_list(world_xyz, n);
    return scene_gradients(ms.data(), n_objs, side, q, level_weights, select, sigma, rgb, owner, owner_sigma, n_inside, grad_log, grad_sigma, normal, nullptr, 0,
                           nullptr);
}
int mon_scene_query_lattice_gradients(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
        const float* level_weights, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma,
        float* normal) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_lattice_gradients_check(side, origin3, step3, nx, ny, nz, level_weights, sigma, grad_log)) ||
        (rc = scene_models("scene_lattice_gradients", objs, n_objs, ms)) || (rc = scene_objects_check("scene_lattice_gradients", ms.data(), n_objs, false)) ||
        (rc = scene_gradients_weights_check(ms.data(), n_objs, level_weights))) return rc;
    return scene_gradients(ms.data(), n_objs, side, scene_lattice(origin3, step3, nx, ny, nz), level_weights, nullptr, sigma, rgb, owner, owner_sigma, n_inside,
                           grad_log, grad_sigma, normal, nullptr, 0, nullptr);
}
int mon_scene_cast_normals(mon_object* const* objs, size_t n_objs, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity,
        const float* level_weights, float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance,
        float* hit_xyz, float* normal, float* grad_log) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_cast_normals_check(side, rays, n_rays, hit_opacity, level_weights, rgb, dist, normal)) ||
        (rc = scene_models("scene_cast_normals", objs, n_objs, ms)) || (rc = scene_objects_check("scene_cast_normals", ms.data(), n_objs, false)) ||
        (rc = scene_gradients_weights_check(ms.data(), n_objs, level_weights))) return rc;
    return scene_cast_normals(ms.data(), n_objs, side, rays, n_rays, hit_opacity, level_weights, rgb, dist, opacity, instance, hit_t, hit_sample_t, hit_instance,
                              hit_xyz, normal, grad_log, nullptr);
}
int mon_pose_refine_default(mon_pose_refine_params* p) {
    REQUIRE(p, "params");
    p->iters = 100; p->rays_per_iter = 4096; p->lr_trans = 2e-3f; p->lr_rot = 4e-3f;
    p->w_rgb = 1.f; p->w_mask = 1.f; p->w_depth = 1.f; p->depth_huber = 0.05f; p->seed = 1;
    return MON_OK;
}
int mon_object_pose_loss(mon_object* o, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p,
        uint32_t iteration, float* loss, float* grad6) {
    REQUIRE(o, "object");
    const int rc = pose_check(side, obs, n_obs, Tow16, p); if (rc) return rc;
    return pose_refine(*o->m, side, obs, n_obs, Tow16, *p, -1, iteration, nullptr, nullptr, loss, grad6, nullptr);
}
int mon_object_refine_pose(mon_object* o, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p, float* Tow16_inout,
        float* loss_trace) {
    REQUIRE(o, "object");
    const int rc = pose_check(side, obs, n_obs, Tow16_inout, p); if (rc) return rc;
    return pose_inout(Tow16_inout, [&](float* pose) {
        return pose_refine(*o->m, side, obs, n_obs, pose, *p, p->iters, 0u, pose, loss_trace, nullptr, nullptr, nullptr); });
}
// ---- camera refinement against a scene of objects
int mon_scene_pose_loss(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16,
                        const mon_pose_refine_params* p, uint32_t iteration, const float* level_weights, float* loss, float* grad6) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_pose_check(side, obs, n_obs, Twc16, p)) || (rc = scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = scene_pose_objects_check(ms.data(), n_objs, obs, n_obs, p))) return rc;
    if (level_weights && (rc = level_weights_check("scene pose", level_weights, scene_levels(ms.data(), n_objs).Lmax))) return rc;
    return scene_pose(ms.data(), n_objs, side, obs, n_obs, Twc16, *p, -1, iteration, nullptr, nullptr, loss, grad6, nullptr, level_weights);
}
int mon_scene_refine_camera(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p,
                            const mon_pose_c2f_params* c, float* Twc16_inout, float* loss_trace) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_pose_check(side, obs, n_obs, Twc16_inout, p)) || (rc = scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = scene_pose_objects_check(ms.data(), n_objs, obs, n_obs, p)) || (c && (rc = pose_c2f_check(c)))) return rc;
    const SceneLevels lv = scene_levels(ms.data(), n_objs, c, p->iters);
    return pose_inout(Twc16_inout, [&](float* pose) {
        return scene_pose(ms.data(), n_objs, side, obs, n_obs, pose, *p, p->iters, 0u, pose, loss_trace, nullptr, nullptr, nullptr, lv.w()); });
}
// ---- joint refinement of a window of camera poses and object poses
int mon_window_default(mon_window_params* w) {
    REQUIRE(w, "params");
    w->n_fixed_frames = 1; w->refine_objects = 1; w->lr_obj_trans = 2e-3f; w->lr_obj_rot = 4e-3f;
    return MON_OK;
}
int mon_window_frames(const mon_frame_bbox* obs, size_t n_obs, uint32_t* frame_ids_out, size_t* n_frames_out) {
    return window_frames(obs, n_obs, frame_ids_out, n_frames_out);
}
int mon_scene_window_loss(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, const float* Tow16s,
                          const mon_pose_refine_params* p, uint32_t iteration, const float* level_weights, float* loss, float* frame_loss, float* cam_grad6,
                          float* obj_grad6) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_window_check(side, obs, n_obs, Twc16s, p, nullptr, Tow16s, false)) || (rc = scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = scene_window_objects_check(ms.data(), n_objs, obs, n_obs, Tow16s, p))) return rc;
    if (level_weights && (rc = level_weights_check("scene pose", level_weights, scene_levels(ms.data(), n_objs).Lmax))) return rc;
    return scene_window(ms.data(), n_objs, side, obs, n_obs, Twc16s, Tow16s, *p, nullptr, -1, iteration, level_weights, nullptr, nullptr, nullptr, nullptr, loss,
                        frame_loss, cam_grad6, obj_grad6);
}
int mon_scene_refine_window(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p,
                            const mon_pose_c2f_params* c, const mon_window_params* w, float* Twc16s_inout, float* Tow16s_inout, float* loss_trace,
                            float* frame_trace) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_window_check(side, obs, n_obs, Twc16s_inout, p, w, Tow16s_inout, true)) || (rc = scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = scene_window_objects_check(ms.data(), n_objs, obs, n_obs, Tow16s_inout, p)) || (c && (rc = pose_c2f_check(c)))) return rc;
    const SceneLevels lv = scene_levels(ms.data(), n_objs, c, p->iters);
    return scene_window(ms.data(), n_objs, side, obs, n_obs, Twc16s_inout, Tow16s_inout, *p, w, p->iters, 0u, lv.w(), Twc16s_inout, Tow16s_inout, loss_trace,
                        frame_trace, nullptr, nullptr, nullptr, nullptr);
}
int mon_object_set_pose(mon_object* o, const float* Tow16) { REQUIRE(o, "object"); REQUIRE(Tow16, "Tow16"); return model_set_pose(*o->m, Tow16); }
// ---- wide-basin relocalisation: batched scoring, candidate poses, the driver
int mon_scene_pose_loss_batch(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s,
                              size_t n_poses, const mon_pose_refine_params* p, uint32_t iteration, float* losses) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_pose_batch_check(side, obs, n_obs, Twc16s, n_poses, p, losses)) || (rc = scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = scene_pose_batch_objects_check(ms.data(), n_objs, obs, n_obs, p))) return rc;
    return scene_pose_batch(ms.data(), n_objs, side, obs, n_obs, Twc16s, n_poses, *p, iteration, losses);
}
int mon_pose_hypotheses(const float* Twc16, const float* pivot_cam3, float max_rot_rad, float max_trans, size_t n, uint64_t seed, float* Twc16s_out) {
    REQUIRE(Twc16, "Twc16"); REQUIRE(Twc16s_out, "Twc16s_out");
    if (n == 0 || n > kSceneScoreMaxPoses) { set_error("pose hypotheses: n %zu (1 to %u)", n, kSceneScoreMaxPoses); return MON_ERR_ARG; }
    if (!std::isfinite(max_rot_rad) || max_rot_rad < 0.f || !std::isfinite(max_trans) || max_trans < 0.f) {
        set_error("pose hypotheses: max_rot_rad %g, max_trans %g (finite, >= 0)", max_rot_rad, max_trans); return MON_ERR_ARG; }
    float T0[16]; std::memcpy(T0, Twc16, 64);                                       // (Twc16s_out may begin at Twc16)
    std::memcpy(Twc16s_out, T0, 64);
    const double c[3] = { pivot_cam3 ? (double)pivot_cam3[0] : 0.0, pivot_cam3 ? (double)pivot_cam3[1] : 0.0, pivot_cam3 ? (double)pivot_cam3[2] : 0.0 };
    const double two_pi = 6.283185307179586476925286766559;
    for (size_t h = 1; h < n; ++h) {
        double u[6]; for (uint32_t k = 0; k < 6; ++k) u[k] = (double)rand01(seed, kStreamPoseHyp, (uint32_t)h, k);
        const double rho[3] = { max_trans * (2.0 * u[0] - 1.0), max_trans * (2.0 * u[1] - 1.0), max_trans * (2.0 * u[2] - 1.0) };
        const double z = 2.0 * u[4] - 1.0, sxy = std::sqrt(std::max(0.0, 1.0 - z * z)), az = two_pi * u[5];
        const double e[3] = { sxy * std::cos(az), sxy * std::sin(az), z }, th = (double)max_rot_rad * std::cbrt(u[3]);
        // Rodrigues: R = I + sin(th) K + (1 - cos(th)) K^2, K = e^ (row-major here)
        const double K[9] = { 0.0, -e[2], e[1], e[2], 0.0, -e[0], -e[1], e[0], 0.0 }, sn = std::sin(th), cs1 = 1.0 - std::cos(th);
        double R[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
            double k2 = 0.0; for (int q = 0; q < 3; ++q) k2 += K[i * 3 + q] * K[q * 3 + j];
            R[i * 3 + j] = (i == j ? 1.0 : 0.0) + sn * K[i * 3 + j] + cs1 * k2; }
        double t[3]; for (int i = 0; i < 3; ++i) t[i] = c[i] - (R[i * 3] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2]) + rho[i];
        float* o = Twc16s_out + 16 * h;                                               // Twc D, column-major
        for (int col = 0; col < 3; ++col) { for (int row = 0; row < 3; ++row) {
            double v = 0.0; for (int q = 0; q < 3; ++q) v += (double)T0[q * 4 + row] * R[q * 3 + col];
            o[col * 4 + row] = (float)v; } o[col * 4 + 3] = 0.f; }
        for (int row = 0; row < 3; ++row) o[12 + row] = (float)((double)T0[row] * t[0] + (double)T0[4 + row] * t[1] + (double)T0[8 + row] * t[2] + (double)T0[12 + row]);
        o[15] = 1.f;
    }
    return MON_OK;
}
int mon_reloc_default(mon_reloc_params* r) {
    REQUIRE(r, "params");
    r->score_rays = 256; r->keep = 4; r->score_iteration = 0;
    return MON_OK;
}
int mon_scene_relocalise(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16_candidates,
                         size_t n_candidates, const mon_pose_refine_params* p, const mon_pose_c2f_params* c, const mon_reloc_params* r, float* Twc16_out,
                         mon_reloc_result* result, float* scores) {
    std::vector<Model*> ms; int rc;
    if ((rc = scene_reloc_check(side, obs, n_obs, Twc16_candidates, n_candidates, p, r, Twc16_out)) || (rc = scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = scene_pose_objects_check(ms.data(), n_objs, obs, n_obs, p)) || (c && (rc = pose_c2f_check(c)))) return rc;
    const SceneLevels lv = scene_levels(ms.data(), n_objs, c, p->iters);
    return scene_relocalise(ms.data(), n_objs, side, obs, n_obs, Twc16_candidates, n_candidates, *p, lv.w(), *r, Twc16_out, result, scores);
}
int mon_pose_c2f_default(mon_pose_c2f_params* c) {
    REQUIRE(c, "params");
    c->level_start = 4.f; c->level_end = 5.f; c->ramp = 0.7f;
    return MON_OK;
}
int mon_pose_c2f_weights(const mon_pose_c2f_params* c, int n_levels, int iters, int step, float* w) {
    const int rc = pose_c2f_check(c); if (rc) return rc;
    REQUIRE(w, "weights");
    if (n_levels < 1 || iters < 1 || step < 0 || step >= iters) { set_error("pose c2f weights: n_levels %d, iters %d, step %d (n_levels >= 1, 0 <= step < iters)",
            n_levels, iters, step); return MON_ERR_ARG; }
    c2f_row(*c, n_levels, iters, step, w);
    return MON_OK;
}
int mon_object_pose_loss_levels(mon_object* o, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p,
        uint32_t iteration, const float* level_weights, float* loss, float* grad6) {
    REQUIRE(o, "object");
    int rc = pose_check(side, obs, n_obs, Tow16, p); if (rc) return rc;
    REQUIRE(level_weights, "level_weights");
    if ((rc = level_weights_check("pose", level_weights, (int)o->m->nd.L))) return rc;
    return pose_refine(*o->m, side, obs, n_obs, Tow16, *p, -1, iteration, nullptr, nullptr, loss, grad6, nullptr, level_weights);
}
int mon_object_refine_pose_c2f(mon_object* o, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p, const mon_pose_c2f_params* c,
        float* Tow16_inout, float* loss_trace) {
    REQUIRE(o, "object");
    int rc = pose_check(side, obs, n_obs, Tow16_inout, p); if (rc) return rc;
    if ((rc = pose_c2f_check(c))) return rc;
    const SceneLevels lv = scene_levels(&o->m, 1, c, p->iters);
    return pose_inout(Tow16_inout, [&](float* pose) {
        return pose_refine(*o->m, side, obs, n_obs, pose, *p, p->iters, 0u, pose, loss_trace, nullptr, nullptr, nullptr, lv.w()); });
}
int mon_object_density_grid(mon_object* o, int rx, int ry, int rz, float* out_host) { REQUIRE(o, "object");
    return model_density_grid(*o->m, rx, ry, rz, out_host); }
int mon_object_get_config(mon_object* o, mon_config* cfg) { REQUIRE(o, "object"); REQUIRE(cfg, "cfg"); *cfg = o->m->cfg; return MON_OK; }
int mon_object_info_get(mon_object* o, mon_object_info* info) {
    REQUIRE(o, "object"); REQUIRE(info, "info"); Model& m = *o->m;
    info->n_params = m.n_params; info->n_mlp_params = m.nd.n_mlp; info->n_grid_params = m.n_grid; info->encoded_width = (uint32_t)m.nd.Epad;
    info->train_step = m.h_state.step; info->n_boxes = m.n_boxes; info->last_n_valid = m.h_state.n_valid; info->device = m.device;
    info->last_loss = m.h_state.loss_sum / (float)m.oc.R; info->learning_rate = m.h_state.lr; info->backend = m.backend;
    info->skipped_batches = m.h_state.skipped; return MON_OK;
}
int mon_object_get_params(mon_object* o, int which, void* dst, size_t bytes) { REQUIRE(o, "object"); return model_get_params(*o->m, which, dst, bytes); }
int mon_object_set_params(mon_object* o, const float* master, size_t n) { REQUIRE(o, "object"); return model_set_params(*o->m, master, n); }
int mon_checkpoint_read_info(const char* path, int verify, mon_checkpoint_info* out) { return checkpoint_read_info(path, verify, out); }
int mon_object_save(mon_object* o, const char* path) { REQUIRE(o, "object"); REQUIRE(path, "path"); return model_save(*o->m, path); }
int mon_object_load(mon_dataset* ds, const char* path, uint32_t flags, mon_object** out) {
    if (out) *out = nullptr;
    REQUIRE(ds, "dataset"); REQUIRE(path, "path"); REQUIRE(out, "out"); Model* m = nullptr;
    const int rc = model_load(ds->d, path, flags, &m); if (rc) return rc;
    *out = new mon_object{ m }; return MON_OK;
}
int mon_object_set_backend(mon_object* o, int backend) { REQUIRE(o, "object"); return model_set_backend(*o->m, backend); }
int mon_object_set_debug_dump(mon_object* o, int enable) { REQUIRE(o, "object"); return model_set_debug_dump(*o->m, enable); }
int mon_object_set_profiling(mon_object* o, int enable) { REQUIRE(o, "object"); o->m->profiling = enable != 0; return MON_OK; }
int mon_object_get_profile(mon_object* o, mon_profile* out, int reset) {
    REQUIRE(o, "object"); REQUIRE(out, "out"); *out = o->m->prof; if (reset) std::memset(&o->m->prof, 0, sizeof(mon_profile)); return MON_OK;
}
int mon_object_destroy(mon_object* o) { if (!o) return MON_OK; model_destroy(o->m); delete o; return MON_OK; }

int mon_physical_device(int logical_device, int* physical_device) { return mon::physical_device(logical_device, physical_device); }
int mon_device_synchronize(int device) {
    if (use_device(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { set_error("device synchronize failed"); return MON_ERR_HIP; }
    return MON_OK;
}
int mon_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes) {
    REQUIRE(free_bytes, "free_bytes"); REQUIRE(total_bytes, "total_bytes");
    if (use_device(device) != hipSuccess || hipMemGetInfo(free_bytes, total_bytes) != hipSuccess) { set_error("hipMemGetInfo failed on device %d", device);
        return MON_ERR_HIP; }
    return MON_OK;
}

}  // extern "C"
