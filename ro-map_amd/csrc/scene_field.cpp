// scene_field.cpp -- the field queries: the object map asked at places instead of along rays.  Points and lattices (density, colour, owner), their
// gradients and normals, normals at ray hits, distance fields (brought home, or kept on the device as a field handle: dist_field.cpp), connected components
// and shortest-path cost fields over a lattice.  One host chain
// (DESIGN.md 3.4c-4): a SceneCall (scene.cpp) without lists or grids, an output area described once (Area), the passes of field_passes_enqueue, each
// route's own kernels behind them, one copy home and one synchronisation (the cost fields: one more per batch of sweeps).  The routes over a lattice share
// their stages behind the passes too (the lattice routes' chain) and the checks they word alike.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include "model_internal.h"

namespace mon {
// ---- what the routes ask of their arguments without an object (mon_scene_query_points, mon_scene_query_lattice, mon_object_query_points, mon_lattice_points)
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
// the lattice's shape alone (mon_lattice_points, which has no side and no outputs; the host-mask calls; max_cells: dist_field.cpp's handles hold fewer) ...
int lattice_dims_check(const char* what, int nx, int ny, int nz, size_t max_cells) {
    if (nx < 1 || ny < 1 || nz < 1) { set_error("%s: lattice %d x %d x %d (each at least 1)", what, nx, ny, nz); return MON_ERR_ARG; }
    // (each factor bounded before it is multiplied: three ints of up to 2^31 - 1 wrap a 64-bit product)
    const uint64_t mx = max_cells;
    if ((uint64_t)nx > mx || (uint64_t)ny > mx / (uint64_t)nx || (uint64_t)nz > mx / ((uint64_t)nx * (uint64_t)ny)) {
        set_error("%s: lattice %d x %d x %d has more than %zu points", what, nx, ny, nz, max_cells); return MON_ERR_ARG; }
    return MON_OK;
}
// ... and what several routes ask of one argument in the same words
static int step_finite_check(const char* what, const float* step3) {
    for (int a = 0; a < 3; ++a) if (!std::isfinite(step3[a])) { set_error("%s: step is not finite", what); return MON_ERR_ARG; }
    return MON_OK;
}
static int nonneg_check(const char* what, const char* name, float v) {
    if (!std::isfinite(v) || v < 0.f) { set_error("%s: %s %g (finite, >= 0)", what, name, (double)v); return MON_ERR_ARG; }
    return MON_OK;
}
static int connectivity_check(const char* what, int connectivity) {
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) { set_error("%s: connectivity %d (6, 18 or 26)", what, connectivity); return MON_ERR_ARG; }
    return MON_OK;
}
static int lattice_shape_check(const char* what, const float* origin3, const float* step3, int nx, int ny, int nz) {
    REQUIRE_ARG(what, origin3, "origin"); REQUIRE_ARG(what, step3, "step");
    { const int rc = lattice_dims_check(what, nx, ny, nz, kSceneProbeMaxQueries); if (rc) return rc; }
    const int dims[3] = { nx, ny, nz };
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin3[a]) || !std::isfinite(step3[a])) { set_error("%s: origin or step is not finite", what); return MON_ERR_ARG; }
        // (fmaf is monotone in the index: the far end is finite iff every point of the axis is)
        if (!std::isfinite(std::fmaf((float)(dims[a] - 1), step3[a], origin3[a]))) { set_error("%s: the lattice leaves the finite floats on axis %d", what, a);
            return MON_ERR_ARG; }
    }
    return MON_OK;
}
// what every lattice route over the object map asks first: the lattice, the side, sigma_min
static int lattice_route_check(const char* what, int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min) {
    int rc;
    if ((rc = lattice_shape_check(what, origin3, step3, nx, ny, nz)) || (rc = side_check(what, side)) || (rc = nonneg_check(what, "sigma_min", sigma_min))) return rc;
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

// ---- the chain.  Per pass of at most kScenePointsPass points every object's point kernel writes its rows [objects][cap][width] -- k_scene_points: 12 floats
// (u[3], inside, raw4, sigma, r, g, b); k_scene_point_grads: 16 (the same twelve, g[3], 0) -- then the fold writes the pass's slice of the output rows (sigma
// | rgb 3 | owner | owner_sigma | n_inside, the gradient fold also grad_log 3 | grad_sigma 3 | normal 3).  Everything is enqueued at once; the outputs go home
// through the pinned staging with one synchronisation.  Render grids are not consulted (nothing is skipped), and neither the sample count nor the XORWOW
// render mode matters: nothing is sampled or jittered.
// The points of one pass: kRenderChunkRays, as the other scene routes.  A variant build (tools/variant_build.sh <tag> -DMON_POINTS_PASS=n) takes another
// size for measurements (tools/scene_points_timing.py: a pass of 16 384 points is a grid of 64 workgroups); outputs do not depend on it.
#ifndef MON_POINTS_PASS
#define MON_POINTS_PASS kRenderChunkRays
#endif
constexpr uint32_t kScenePointsPass = MON_POINTS_PASS;
// (A route's output area in ws.out is an Area, model_internal.h.)
// where a route keeps the fold's output rows (grad_log, grad_sigma, normal: the gradient fold's).  A route places the rows it sends home where its area
// wants them; fold_rows_rest places the others behind, in this order
constexpr size_t kNoRow = ~(size_t)0;
struct FoldRows { size_t sigma = kNoRow, rgb = kNoRow, owner = kNoRow, owner_sigma = kNoRow, n_inside = kNoRow, grad_log = kNoRow, grad_sigma = kNoRow, normal = kNoRow; };
static void fold_rows_rest(Area& A, FoldRows& f, bool grads) {
    size_t* const at[8] = { &f.sigma, &f.rgb, &f.owner, &f.owner_sigma, &f.n_inside, &f.grad_log, &f.grad_sigma, &f.normal };
    const size_t width[8] = { 1, 3, 1, 1, 1, 3, 3, 3 };
    for (int k = 0; k < (grads ? 8 : 5); ++k) if (*at[k] == kNoRow) *at[k] = A.row(width[k]);
}
// what the gradient routes take beside the points: the caller's level weights (nullptr: ones) and select (may be nullptr), in ws.lw and ws.sel for the
// kernels; every object's FULL fragment image at frag_off[j] of ws.gfrag (the backward reads the transposed matrices; the objects' own render images hold
// the forward set only and are left alone)
struct FieldGrads { const float* level_w; const int32_t* select; std::vector<size_t> frag_off; };
// the passes' workspace: a pass's rows and, for a list, its points on the device
static int field_passes_prepare(const SceneCall& c, size_t n, const ScenePoints& q, uint32_t cap, uint32_t width) {
    SceneWs& ws = *c.ws; int rc;
    if ((rc = ws.rows.grow(n * (size_t)cap * width)) || (q.xyz && (rc = ws.pts.grow(3 * q.n)))) return rc;
    if (q.xyz) HIPCHECK(hipMemcpyAsync(ws.pts.p, q.xyz, 12 * q.n, hipMemcpyHostToDevice, c.s));
    return MON_OK;
}
// The passes of every field query: q.xyz: the list ([q.n][3]; `world` false: unit-cube points of the one object), or nullptr: the lattice q.g
// (q.n its points).  g: the gradient kernels and rows of 16, nullptr: the forward kernels and rows of 12.  f: the fold's rows in ws.out.
// dump (may be nullptr): where in ws.out object rows_k's rows of every point go, [q.n][width].
static void field_passes_enqueue(const SceneCall& c, Model* const* ms, size_t n, const ScenePoints& q, bool world, uint32_t cap, const FoldRows& f,
                                 const FieldGrads* g, size_t rows_k, float* dump) {
    SceneWs& ws = *c.ws; const hipStream_t s = c.s; float* o = ws.out.p;
    const uint32_t nq = (uint32_t)q.n, L = (uint32_t)n, width = g ? 16u : 12u;
    for (uint32_t p0 = 0; p0 < nq; p0 += cap) {
        const uint32_t nc = std::min(cap, nq - p0);
        for (size_t j = 0; j < n; ++j) {
            Model& m = *ms[j];
            ScenePointsArgs a{}; a.pts = q.xyz ? ws.pts.p + 3 * (size_t)p0 : nullptr; a.nx = (uint32_t)q.g.nx; a.ny = (uint32_t)q.g.ny; a.first = p0; a.n = nc;
            for (int k = 0; k < 3; ++k) { a.origin[k] = q.g.origin[k]; a.step[k] = q.g.step[k]; }
            a.rows = ws.rows.p + j * (size_t)cap * width;
            if (g) launch_scene_point_grads(s, m.lf, m.nd, c.sd.prm[j], m.oc, ws.gfrag.p + g->frag_off[j], p0 == 0u, world, a, ws.lw.p);
            else launch_scene_points(s, m.lf, m.nd, c.sd.prm[j], m.oc, c.src[j].frag, p0 == 0u, world, a);
        }
        float* sigma = o + f.sigma + p0; float* rgb = o + f.rgb + 3 * (size_t)p0; int32_t* owner = reinterpret_cast<int32_t*>(o + f.owner) + p0;
        float* owner_sigma = o + f.owner_sigma + p0; uint32_t* n_inside = reinterpret_cast<uint32_t*>(o + f.n_inside) + p0;
        if (g) launch_scene_gradients_fold(s, nc, L, cap, ws.rows.p, g->select ? ws.sel.p + p0 : nullptr, sigma, rgb, owner, owner_sigma, n_inside,
                o + f.grad_log + 3 * (size_t)p0, o + f.grad_sigma + 3 * (size_t)p0, o + f.normal + 3 * (size_t)p0);
        else launch_scene_points_fold(s, nc, L, cap, ws.rows.p, sigma, rgb, owner, owner_sigma, n_inside);
        if (dump) launch_copy_params(s, reinterpret_cast<const uint16_t*>(ws.rows.p + rows_k * (size_t)cap * width),
                reinterpret_cast<uint16_t*>(dump + width * (size_t)p0), 2u * width * nc);
    }
}

// ---- point queries and point gradients (mon_scene_query_points, _lattice, _gradients, _lattice_gradients, mon_object_query_points, _gradients; DESIGN.md
// 3.4c-4, 3.4c-5): the chain and nothing behind it.  The host arrays of a call, each may be nullptr
struct FieldOut { float* sigma; float* rgb; int32_t* owner; float* owner_sigma; uint32_t* n_inside; float* grad_log; float* grad_sigma; float* normal; };
// rows (the debug row dumps, mon_object_query_points, mon_object_query_gradients; may be nullptr) = object rows_k's rows of every point, host array
// [q.n][12], with g [q.n][16].
static int scene_field_run(const char* what, Model* const* ms, size_t n, int side, const ScenePoints& q, bool world, FieldGrads* g, const FieldOut& out,
                           const int32_t* ids, size_t rows_k, float* rows) {
    SceneCall c; { const int rc = c.enter(what, ms, n, side, false); if (rc) return rc; }
    SceneWs& ws = *c.ws; const hipStream_t s = c.s;
    const size_t n_q = q.n; const uint32_t cap = std::min((uint32_t)n_q, kScenePointsPass), width = g ? 16u : 12u;
    // the output area: [the dumped rows |] the fold's rows (the dumped rows first: every piece copied stays 16-byte aligned)
    Area A{ n_q }; const size_t r_dump = A.take(rows ? width * n_q : 0);
    FoldRows f; f.sigma = A.out(out.sigma); f.rgb = A.out(out.rgb, 3); f.owner = A.out(out.owner, 1, true); f.owner_sigma = A.out(out.owner_sigma);
    f.n_inside = A.out(out.n_inside);
    if (g) { f.grad_log = A.out(out.grad_log, 3); f.grad_sigma = A.out(out.grad_sigma, 3); f.normal = A.out(out.normal, 3); }
    { int rc; if ((rc = field_passes_prepare(c, n, q, cap, width)) || (rc = ws.out.grow(A.end)) || (rc = ws.h_out.grow(A.end))) return rc; }
    std::vector<float> ones;
    if (g) {
        const int Lmax = scene_levels(ms, n).Lmax;
        g->frag_off.assign(n + 1, 0);
        for (size_t j = 0; j < n; ++j) { const NetDims& nd = ms[j]->nd; const FragDims fd{ nd.Epad, nd.W, nd.NH, nd.L }; g->frag_off[j + 1] = g->frag_off[j] + (size_t)fd.N_FRAGS() * 512; }
        if (!g->level_w) ones.assign((size_t)Lmax, 1.f);
        { int rc; if ((rc = ws.gfrag.grow(g->frag_off[n])) || (rc = ws.lw.grow((size_t)Lmax)) || (g->select && (rc = ws.sel.grow(n_q)))) return rc; }
        if (g->select) HIPCHECK(hipMemcpyAsync(ws.sel.p, g->select, 4 * n_q, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(ws.lw.p, g->level_w ? g->level_w : ones.data(), 4 * (size_t)Lmax, hipMemcpyHostToDevice, s));
    }
    field_passes_enqueue(c, ms, n, q, world, cap, f, g, rows_k, rows ? ws.out.p + r_dump : nullptr);
    { const int rc = c.home(A.end); if (rc) return rc; }
    const float* h = ws.h_out.p;
    if (rows) std::memcpy(rows, h + r_dump, 4 * width * n_q);
    A.unpack(h, ids);
    return MON_OK;
}
int scene_points(Model* const* ms, size_t n, int side, const ScenePoints& q, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside,
                 const int32_t* ids, size_t rows_k, float* rows) {
    const FieldOut out{ sigma, rgb, owner, owner_sigma, n_inside, nullptr, nullptr, nullptr };
    return scene_field_run(q.xyz ? "scene_points" : "scene_lattice", ms, n, side, q, true, nullptr, out, ids, rows_k, rows);
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
    const ScenePoints q = scene_point_list(unit_xyz, n);
    std::vector<float> rows(12 * n);
    const int rc = scene_field_run("object_points", ms, 1, side, q, false, nullptr, FieldOut{}, nullptr, 0, rows.data());
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) std::memcpy(raw4 + 4 * i, rows.data() + 12 * i + 4, 16);
    return MON_OK;
}

// ---- what the gradient routes ask of their arguments.
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
int scene_gradients(Model* const* ms, size_t n, int side, const ScenePoints& q, const float* level_w, const int32_t* select, float* sigma, float* rgb,
                    int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma, float* normal, const int32_t* ids,
                    size_t rows_k, float* rows) {
    FieldGrads g{ level_w, select, {} }; const FieldOut out{ sigma, rgb, owner, owner_sigma, n_inside, grad_log, grad_sigma, normal };
    return scene_field_run(q.xyz ? "scene_gradients" : "scene_lattice_gradients", ms, n, side, q, true, &g, out, ids, rows_k, rows);
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
    const ScenePoints q = scene_point_list(unit_xyz, n);
    std::vector<float> rows(16 * n); FieldGrads g{ level_w, nullptr, {} };
    const int rc = scene_field_run("object_gradients", ms, 1, side, q, false, &g, FieldOut{}, nullptr, 0, rows.data());
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
        const ScenePoints q = scene_point_list(x.data(), nh);
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

// ---- distance fields (mon_distance_transform, mon_scene_distance_lattice): clearance over a lattice.  scene_distance: the lattice chain
// below with the transform behind the mask, once more on the complement when free_dist is asked for (the two run one after the other in the same halves).
static int distance_outputs_check(const char* what, float max_dist, const float* dist) {
    REQUIRE_ARG(what, dist, "dist");
    if (!(max_dist > 0.f)) { set_error("%s: max_dist %g (above 0; +inf for no limit)", what, (double)max_dist); return MON_ERR_ARG; }
    return MON_OK;
}
int distance_transform_check(const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, const float* dist) {
    REQUIRE_ARG("distance_transform", occupied, "occupied"); REQUIRE_ARG("distance_transform", step3, "step");
    { int rc; if ((rc = lattice_dims_check("distance_transform", nx, ny, nz, kSceneProbeMaxQueries)) || (rc = step_finite_check("distance_transform", step3))) return rc; }
    return distance_outputs_check("distance_transform", max_dist, dist);
}
int scene_distance_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist, const float* dist) {
    { const int rc = lattice_route_check("scene_distance", side, origin3, step3, nx, ny, nz, sigma_min); if (rc) return rc; }
    return distance_outputs_check("scene_distance", max_dist, dist);
}
// The tail of the two standalone transforms: the launches' error, then the value array and, where asked for, the index array read back; the caller's
// arrays are written only once everything has succeeded
static int transform_home(size_t n, const float* d_val, float* val, const int32_t* d_index, int32_t* index) {
    HIPCHECK(hipGetLastError());
    std::vector<float> h_val(n); std::vector<int32_t> h_index(index ? n : 0);
    HIPCHECK(hipMemcpy(h_val.data(), d_val, 4 * n, hipMemcpyDeviceToHost));
    if (index) HIPCHECK(hipMemcpy(h_index.data(), d_index, 4 * n, hipMemcpyDeviceToHost));
    std::memcpy(val, h_val.data(), 4 * n);
    if (index) std::memcpy(index, h_index.data(), 4 * n);
    return MON_OK;
}
// mon_distance_transform: the transform alone on a host mask, in buffers of its own on the device's default stream
int distance_transform(int device, const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, float* dist, int32_t* nearest) {
    { const int rc = device_enter(device); if (rc) return rc; }
    const size_t n = (size_t)nx * ny * nz;
    DevBuf<uint8_t> occ; DevBuf<float> v; DevBuf<int32_t> site;                     // v, site: the passes' two halves, then the output row
    { int rc; if ((rc = occ.grow(n)) || (rc = v.grow(3 * n)) || (rc = site.grow(3 * n))) return rc; }
    HIPCHECK(hipMemcpy(occ.p, occupied, n, hipMemcpyHostToDevice));
    launch_distance_passes(nullptr, occ.p, false, Lattice(nullptr, step3, nx, ny, nz), v.p, site.p);
    launch_distance_finish(nullptr, (uint32_t)n, v.p, site.p, max_dist, nullptr, v.p + 2 * n, nearest ? site.p + 2 * n : nullptr, nullptr);
    return transform_home(n, v.p + 2 * n, dist, site.p + 2 * n, nearest);
}
// ---- the lattice routes' chain: scene_distance, scene_dist_field, scene_components and scene_paths each declare their area -- the rows
// they may send home at the front (Area::out, in the order a caller may ask for them), the fold's other rows behind (fold_rows_rest) -- run the stages below,
// put their own kernels behind them, and bring A.home floats home (SceneCall::home, then Area::unpack).
// Stage 1: the workspace, the passes over the lattice and the mask !(sigma <= sigma_min) in ws.docc.
static int lattice_occupancy(const SceneCall& c, Model* const* ms, size_t n, const ScenePoints& q, const Area& A, const FoldRows& f, float sigma_min) {
    SceneWs& ws = *c.ws; const uint32_t nq = (uint32_t)q.n, cap = std::min(nq, kScenePointsPass);
    { int rc; if ((rc = field_passes_prepare(c, n, q, cap, 12u)) || (rc = ws.out.grow(A.end)) || (rc = ws.h_out.grow(A.home)) || (rc = ws.docc.grow(q.n))) return rc; }
    field_passes_enqueue(c, ms, n, q, true, cap, f, nullptr, 0, nullptr);
    launch_distance_mask(c.s, nq, ws.out.p + f.sigma, sigma_min, ws.docc.p);
    return MON_OK;
}
// The transform of the mask (the passes' two halves of squared distance and site, 16 B per cell, are the side's): dist into row r_dist, cut at max_dist
static int lattice_distance(const SceneCall& c, const ScenePoints& q, bool invert, float max_dist, const int32_t* owner, size_t r_dist, int32_t* nearest,
                            int32_t* nearest_owner) {
    SceneWs& ws = *c.ws;
    { int rc; if ((rc = ws.dv.grow(2 * q.n)) || (rc = ws.dsite.grow(2 * q.n))) return rc; }
    launch_distance_passes(c.s, ws.docc.p, invert, q.g, ws.dv.p, ws.dsite.p);
    launch_distance_finish(c.s, (uint32_t)q.n, ws.dv.p, ws.dsite.p, max_dist, owner, ws.out.p + r_dist, nearest, nearest_owner);
    return MON_OK;
}
// Stage 2: the untruncated transform, then the mask dist > clearance written over the first one, which the passes have consumed
static int lattice_clearance(const SceneCall& c, const ScenePoints& q, size_t r_dist, float clearance) {
    { const int rc = lattice_distance(c, q, false, INFINITY, nullptr, r_dist, nullptr, nullptr); if (rc) return rc; }
    launch_components_clear_mask(c.s, (uint32_t)q.n, c.ws->out.p + r_dist, clearance, c.ws->docc.p);
    return MON_OK;
}
static int32_t* as_i32(float* p) { return reinterpret_cast<int32_t*>(p); }

// What scene_distance and scene_dist_field share.  The rows: sigma | dist | nearest | nearest_owner | free_dist, then the fold's other rows.
struct DistanceRows { FoldRows f; size_t dist, nearest, nearest_owner, free; };
static DistanceRows distance_rows(Area& A, float* sigma, float* dist, int32_t* nearest, int32_t* nearest_owner, float* free_dist) {
    DistanceRows r; r.f.sigma = A.out(sigma); r.dist = A.out(dist); r.nearest = A.out(nearest); r.nearest_owner = A.out(nearest_owner, 1, true);
    r.free = A.out(free_dist); fold_rows_rest(A, r.f, false);
    return r;
}
static int distance_chain(const SceneCall& c, Model* const* ms, size_t n, const ScenePoints& q, float sigma_min, float max_dist, const Area& A,
                          const DistanceRows& r, bool nearest, bool nearest_owner) {
    { const int rc = lattice_occupancy(c, ms, n, q, A, r.f, sigma_min); if (rc) return rc; }
    float* o = c.ws->out.p;
    return lattice_distance(c, q, false, max_dist, as_i32(o + r.f.owner), r.dist, nearest ? as_i32(o + r.nearest) : nullptr,
                            nearest_owner ? as_i32(o + r.nearest_owner) : nullptr);
}
// q: a lattice (scene_lattice).  ids as scene_points', applied to nearest_owner.  max_dist truncates dist and free_dist alike.
int scene_distance(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float max_dist, float* dist, int32_t* nearest,
                   int32_t* nearest_owner, float* free_dist, float* sigma, const int32_t* ids) {
    SceneCall c; { const int rc = c.enter("scene_distance", ms, n, side, false); if (rc) return rc; }
    Area A{ q.n }; const DistanceRows r = distance_rows(A, sigma, dist, nearest, nearest_owner, free_dist);
    { const int rc = distance_chain(c, ms, n, q, sigma_min, max_dist, A, r, nearest != nullptr, nearest_owner != nullptr); if (rc) return rc; }
    if (free_dist) { const int rc = lattice_distance(c, q, true, max_dist, nullptr, r.free, nullptr, nullptr); if (rc) return rc; }
    { const int rc = c.home(A.home); if (rc) return rc; }
    A.unpack(c.ws->h_out.p, ids);
    return MON_OK;
}
// mon_scene_dist_field / mon_online_dist_field: the same chain with dist kept on the device.  What a fill asks beyond its lattice route:
// a finite max_dist, so that every value lies within it, and no step 0 on an axis of several cells (a handle's sample divides by the step)
static int field_fill_check(const char* what, const float* step3, int nx, int ny, int nz, float max_dist) {
    if (!std::isfinite(max_dist) || !(max_dist > 0.f)) { set_error("%s: max_dist %g (finite, above 0)", what, (double)max_dist); return MON_ERR_ARG; }
    const int dims[3] = { nx, ny, nz };
    for (int a = 0; a < 3; ++a) if (dims[a] > 1 && step3[a] == 0.f) { set_error("%s: step 0 on axis %d, which has %d cells", what, a, dims[a]);
        return MON_ERR_ARG; }
    return MON_OK;
}
int scene_dist_field_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist, const void* field_out) {
    REQUIRE_ARG("scene_dist_field", field_out, "field");
    float unused = 0.f;
    { const int rc = scene_distance_check(side, origin3, step3, nx, ny, nz, sigma_min, 1.f, &unused); if (rc) return rc; }
    return field_fill_check("scene_dist_field", step3, nx, ny, nz, max_dist);
}
// The fill of a handle, for scene_dist_field and scene_signed_dist_field.  The route's area opens with four words for the field's largest value (r_max) --
// all that goes home -- and ends with the partial maxima (r_part).  The handle is made before `chain` enqueues the route's stages; then the row r_keep goes
// into the handle's buffer by a device-to-device copy, the largest value is formed, and A.home floats come home.  The handle is freed on every failure.
template <class Chain> static int lattice_field_fill(const char* what, SceneCall& c, int device, const Lattice& g, const Area& A, size_t r_keep, size_t r_max,
                                                     size_t r_part, Chain chain, DistField** out) {
    DistField* f = nullptr;
    { const int rc = dist_field_adopt(device, g, &f); if (rc) return rc; }
    int rc = chain();
    if (!rc) {
        float* o = c.ws->out.p;
        const hipError_t e = hipMemcpyAsync(f->cells, o + r_keep, 4 * g.n(), hipMemcpyDeviceToDevice, c.s);
        if (e != hipSuccess) { set_error("%s: the copy into the handle failed: %s", what, hipGetErrorString(e)); rc = MON_ERR_HIP; }
        else { launch_field_max(c.s, o + r_keep, (uint32_t)g.n(), o + r_part, o + r_max); rc = c.home(A.home); }
    }
    if (rc) { dist_field_free(f); return rc; }
    f->max_value = c.ws->h_out.p[r_max];
    *out = f;
    return MON_OK;
}
int scene_dist_field(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float max_dist, DistField** out) {
    SceneCall c; { const int rc = c.enter("scene_dist_field", ms, n, side, false); if (rc) return rc; }
    Area A{ q.n }; const size_t r_max = A.keep(4); const DistanceRows r = distance_rows(A, nullptr, nullptr, nullptr, nullptr, nullptr);
    const size_t r_part = A.take(kFieldMaxBlocks);
    return lattice_field_fill("scene_dist_field", c, ms[0]->device, q.g, A, r.dist, r_max, r_part,
                              [&] { return distance_chain(c, ms, n, q, sigma_min, max_dist, A, r, false, false); }, out);
}

// ---- signed, sub-cell distance fields (mon_signed_distance_transform, mon_scene_signed_distance_lattice, mon_scene_signed_dist_field; DESIGN.md
// 3.4c-12): the distance to the density's level set placed inside the lattice edges, negative inside matter.  The scene calls: the lattice chain, the values
// (k_signed_values: val, iso and the side, which replaces the mask in ws.docc by the same bits), the nine passes in ws.dv and ws.dsite ([4][n] here: three
// chains' results and the passes' other half, 32 B per cell) and the finish; one copy home, one synchronisation.
static int signed_flags_check(const char* what, uint32_t flags) {
    if (flags & ~(uint32_t)MON_SIGNED_LOG) { set_error("%s: flags %#x (MON_SIGNED_LOG or 0)", what, flags); return MON_ERR_ARG; }
    return MON_OK;
}
int signed_distance_transform_check(const float* val, float iso, int nx, int ny, int nz, const float* step3, float max_dist, const float* sdist) {
    const char* what = "signed_distance_transform";
    REQUIRE_ARG(what, val, "val"); REQUIRE_ARG(what, step3, "step");
    { int rc; if ((rc = lattice_dims_check(what, nx, ny, nz, kSceneProbeMaxQueries)) || (rc = step_finite_check(what, step3))) return rc; }
    if (std::isnan(iso)) { set_error("%s: iso is NaN", what); return MON_ERR_ARG; }
    return distance_outputs_check(what, max_dist, sdist);
}
int scene_signed_distance_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, uint32_t flags, float max_dist,
                                const float* sdist) {
    const char* what = "scene_signed_distance";
    int rc;
    if ((rc = lattice_route_check(what, side, origin3, step3, nx, ny, nz, sigma_min)) || (rc = signed_flags_check(what, flags))) return rc;
    return distance_outputs_check(what, max_dist, sdist);
}
// mon_signed_distance_transform: the transform alone on host values, in buffers of its own on the device's default stream
int signed_distance_transform(int device, const float* val, float iso, int nx, int ny, int nz, const float* step3, float max_dist, float* sdist,
                              int32_t* nearest_edge) {
    { const int rc = device_enter(device); if (rc) return rc; }
    const Lattice g(nullptr, step3, nx, ny, nz); const size_t n = g.n();
    DevBuf<uint8_t> ins; DevBuf<float> v; DevBuf<int32_t> site;                     // v: val | the passes' four parts | sdist; site: the four parts | nearest_edge
    { int rc; if ((rc = ins.grow(n)) || (rc = v.grow(6 * n)) || (rc = site.grow(5 * n))) return rc; }
    HIPCHECK(hipMemcpy(v.p, val, 4 * n, hipMemcpyHostToDevice));
    launch_signed_values(nullptr, (uint32_t)n, v.p, iso, false, nullptr, ins.p, nullptr);
    launch_signed_passes(nullptr, v.p, ins.p, nullptr, iso, g, v.p + n, site.p);
    launch_signed_finish(nullptr, g, v.p + n, site.p, ins.p, max_dist, nullptr, v.p + 5 * n, nearest_edge ? site.p + 4 * n : nullptr, nullptr);
    return transform_home(n, v.p + 5 * n, sdist, site.p + 4 * n, nearest_edge);
}
// What the two scene calls share.  The rows: iso (four words) | sigma | sdist | nearest_edge | nearest_owner | val, then the fold's other rows.
struct SignedRows { FoldRows f; size_t iso, sdist, edge, edge_owner, val; };
static SignedRows signed_rows(Area& A, float* sigma, float* sdist, int32_t* nearest_edge, int32_t* nearest_owner, float* val, bool iso_home) {
    SignedRows r; r.iso = iso_home ? A.keep(4) : A.take(4); r.f.sigma = A.out(sigma); r.sdist = A.out(sdist); r.edge = A.out(nearest_edge);
    r.edge_owner = A.out(nearest_owner, 1, true); r.val = A.out(val); fold_rows_rest(A, r.f, false);
    return r;
}
static int signed_chain(const SceneCall& c, Model* const* ms, size_t n, const ScenePoints& q, float sigma_min, uint32_t flags, float max_dist, const Area& A,
                        const SignedRows& r, bool nearest_edge, bool nearest_owner) {
    { const int rc = lattice_occupancy(c, ms, n, q, A, r.f, sigma_min); if (rc) return rc; }
    SceneWs& ws = *c.ws; float* o = ws.out.p;
    { int rc; if ((rc = ws.dv.grow(4 * q.n)) || (rc = ws.dsite.grow(4 * q.n))) return rc; }
    launch_signed_values(c.s, (uint32_t)q.n, o + r.f.sigma, sigma_min, (flags & MON_SIGNED_LOG) != 0u, o + r.val, ws.docc.p, o + r.iso);
    launch_signed_passes(c.s, o + r.val, ws.docc.p, o + r.iso, 0.f, q.g, ws.dv.p, ws.dsite.p);
    launch_signed_finish(c.s, q.g, ws.dv.p, ws.dsite.p, ws.docc.p, max_dist, as_i32(o + r.f.owner), o + r.sdist, nearest_edge ? as_i32(o + r.edge) : nullptr,
            nearest_owner ? as_i32(o + r.edge_owner) : nullptr);
    return MON_OK;
}
// q: a lattice (scene_lattice).  ids as scene_points', applied to nearest_owner.
int scene_signed_distance(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, uint32_t flags, float max_dist, float* sdist,
                          int32_t* nearest_edge, int32_t* nearest_owner, float* sigma, float* val, float* iso_out, const int32_t* ids) {
    SceneCall c; { const int rc = c.enter("scene_signed_distance", ms, n, side, false); if (rc) return rc; }
    Area A{ q.n }; const SignedRows r = signed_rows(A, sigma, sdist, nearest_edge, nearest_owner, val, iso_out != nullptr);
    { const int rc = signed_chain(c, ms, n, q, sigma_min, flags, max_dist, A, r, nearest_edge != nullptr, nearest_owner != nullptr); if (rc) return rc; }
    { const int rc = c.home(A.home); if (rc) return rc; }
    A.unpack(c.ws->h_out.p, ids);
    if (iso_out) *iso_out = c.ws->h_out.p[r.iso];
    return MON_OK;
}
// mon_scene_signed_dist_field / mon_online_signed_dist_field: the same chain with sdist kept on the device, as scene_dist_field keeps dist
// (lattice_field_fill).
int scene_signed_dist_field_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, uint32_t flags, float max_dist,
                                  const void* field_out) {
    const char* what = "scene_signed_dist_field";
    REQUIRE_ARG(what, field_out, "field");
    int rc;
    if ((rc = lattice_route_check(what, side, origin3, step3, nx, ny, nz, sigma_min)) || (rc = signed_flags_check(what, flags))) return rc;
    return field_fill_check(what, step3, nx, ny, nz, max_dist);
}
int scene_signed_dist_field(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, uint32_t flags, float max_dist, DistField** out) {
    SceneCall c; { const int rc = c.enter("scene_signed_dist_field", ms, n, side, false); if (rc) return rc; }
    Area A{ q.n }; const size_t r_max = A.keep(4); const SignedRows r = signed_rows(A, nullptr, nullptr, nullptr, nullptr, nullptr, false);
    const size_t r_part = A.take(kFieldMaxBlocks);
    return lattice_field_fill("scene_signed_dist_field", c, ms[0]->device, q.g, A, r.sdist, r_max, r_part,
                              [&] { return signed_chain(c, ms, n, q, sigma_min, flags, max_dist, A, r, false, false); }, out);
}

// ---- connected components (mon_label_components, mon_scene_components_lattice): which cells belong together.  scene_components: the
// lattice chain (region 1: with its second stage), the labelling (launch_components; its block sums are 4 B per 256 cells), k_cc_home and one synchronisation.
static int components_outputs_check(const char* what, int connectivity, const int32_t* label, const mon_lattice_component* table, const uint32_t* n_components) {
    REQUIRE_ARG(what, label, "label");
    if (table && !n_components) { set_error("%s: a table without n_components (the count says how many records were written)", what); return MON_ERR_ARG; }
    return connectivity_check(what, connectivity);
}
int label_components_check(const uint8_t* mask, int nx, int ny, int nz, int connectivity, const int32_t* label, const mon_lattice_component* table,
                           const uint32_t* n_components) {
    REQUIRE_ARG("label_components", mask, "mask");
    { const int rc = lattice_dims_check("label_components", nx, ny, nz, kSceneProbeMaxQueries); if (rc) return rc; }
    return components_outputs_check("label_components", connectivity, label, table, n_components);
}
int scene_components_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, int region, float clearance,
                           int connectivity, const int32_t* label, const mon_lattice_component* table, const uint32_t* n_components, const float* dist) {
    { const int rc = lattice_route_check("scene_components", side, origin3, step3, nx, ny, nz, sigma_min); if (rc) return rc; }
    if (region != 0 && region != 1) { set_error("scene_components: region %d (0: occupied matter, 1: traversable space)", region); return MON_ERR_ARG; }
    if (region == 1) { const int rc = nonneg_check("scene_components", "clearance", clearance); if (rc) return rc; }
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
    { const int rc = device_enter(device); if (rc) return rc; }
    const size_t n = (size_t)nx * ny * nz, tcap = table ? std::min((size_t)cap, n) : 0, front = 2 * n + 8;
    DevBuf<uint8_t> occ; DevBuf<uint32_t> w;
    { int rc; if ((rc = occ.grow(n)) || (rc = w.grow(front + 8 * tcap + components_scan_words((uint32_t)n)))) return rc; }
    HIPCHECK(hipMemcpy(occ.p, mask, n, hipMemcpyHostToDevice));
    int32_t* d_label = reinterpret_cast<int32_t*>(w.p); uint32_t* d_meta = w.p + 2 * n;
    launch_components(nullptr, occ.p, Lattice(nullptr, nullptr, nx, ny, nz), connectivity, d_label, d_label + n, w.p + front + 8 * tcap,
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
    SceneCall c; { const int rc = c.enter("scene_components", ms, n, side, false); if (rc) return rc; }
    SceneWs& ws = *c.ws; const hipStream_t s = c.s;
    const size_t n_q = q.n, tcap = table ? std::min((size_t)cap, n_q) : 0; const uint32_t nq = (uint32_t)n_q;
    // the area: label | comp | meta 8 (n_components, the cap flag) | the table's records, 8 words each | (region 1: dist) | sigma | owner, the fold's rest
    Area A{ n_q }; const size_t r_label = A.out(label), r_comp = A.out(comp), r_meta = A.keep(8), r_table = A.keep(8 * tcap);
    const size_t r_dist = region == 1 ? A.out(dist) : A.end;
    FoldRows f; f.sigma = A.out(sigma); f.owner = A.out(owner, 1, true); fold_rows_rest(A, f, false);
    { int rc; if ((rc = ws.cscan.grow(components_scan_words(nq))) || (rc = lattice_occupancy(c, ms, n, q, A, f, sigma_min))) return rc; }
    if (region == 1) { const int rc = lattice_clearance(c, q, r_dist, clearance); if (rc) return rc; }
    float* o = ws.out.p; uint32_t* o_meta = reinterpret_cast<uint32_t*>(o + r_meta);
    launch_components(s, ws.docc.p, q.g, connectivity, as_i32(o + r_label), as_i32(o + r_comp), ws.cscan.p,
            tcap ? reinterpret_cast<mon_lattice_component*>(o + r_table) : nullptr, (uint32_t)tcap, o_meta);
    // (k_cc_home: of the table's room only the records that were written)
    launch_components_home(s, reinterpret_cast<const uint32_t*>(o), reinterpret_cast<uint32_t*>(ws.h_out.p), (uint32_t)A.home, (uint32_t)r_table, (uint32_t)tcap, o_meta);
    { const int rc = c.finish(); if (rc) return rc; }
    const float* h = ws.h_out.p; const uint32_t* h_meta = reinterpret_cast<const uint32_t*>(h + r_meta);
    { const int rc = components_flag_check("scene_components", h_meta[1]); if (rc) return rc; }
    A.unpack(h, ids);
    if (table) std::memcpy(table, h + r_table, 32 * std::min((size_t)h_meta[0], tcap));
    if (n_components) *n_components = h_meta[0];
    return MON_OK;
}

// ---- shortest-path cost fields (mon_shortest_paths, mon_scene_paths_lattice, mon_lattice_path): how far the goal is through the space the
// robot may occupy, and which way to go.  scene_paths: both stages of the lattice chain, the multiplier, then the sweeps (paths_relax) and the finish.  How
// many sweeps the field needs depends on the data, so they are enqueued in batches of kPathsBatch, each sweep with a "left work" word of its own, and the
// words are read back once per batch: one small synchronisation per batch, not per sweep.  The sweeps behind the first one that left no work found no flag
// and returned at once.  A variant build (tools/variant_build.sh <tag> -DMON_PATHS_BATCH=n) takes another batch for measurements
// (tools/scene_paths_timing.py, profiles/r21_scene_paths.md); outputs do not depend on it.
#ifndef MON_PATHS_BATCH
#define MON_PATHS_BATCH 32
#endif
constexpr uint32_t kPathsBatch = MON_PATHS_BATCH, kPathsMaxSeeds = 1u << 22;
static std::atomic<uint32_t> g_paths_stats[3];                                      // (the sides' calls may overlap: the latest writer's figures)
void paths_last_stats(uint32_t out3[3]) { for (int k = 0; k < 3; ++k) out3[k] = g_paths_stats[k].load(); }

static int paths_args_check(const char* what, int connectivity, const int32_t* seeds, size_t n_seeds, size_t n_cells, float max_cost, const float* cost) {
    REQUIRE_ARG(what, cost, "cost"); REQUIRE_ARG(what, seeds, "seeds");
    { const int rc = connectivity_check(what, connectivity); if (rc) return rc; }
    if (!(max_cost > 0.f)) { set_error("%s: max_cost %g (above 0; +inf for no limit)", what, (double)max_cost); return MON_ERR_ARG; }
    if (n_seeds == 0 || n_seeds > kPathsMaxSeeds) { set_error("%s: %zu seeds (1 to %u)", what, n_seeds, kPathsMaxSeeds); return MON_ERR_ARG; }
    for (size_t k = 0; k < n_seeds; ++k) if (seeds[k] < 0 || (size_t)seeds[k] >= n_cells) {
        set_error("%s: seed %zu is cell %d (0 to %zu)", what, k, seeds[k], n_cells - 1); return MON_ERR_ARG; }
    return MON_OK;
}
int shortest_paths_check(const uint8_t* passable, int nx, int ny, int nz, const float* step3, int connectivity, const float* cell_cost, const int32_t* seeds,
                         size_t n_seeds, float max_cost, const float* cost) {
    REQUIRE_ARG("shortest_paths", passable, "passable"); REQUIRE_ARG("shortest_paths", step3, "step");
    { int rc; if ((rc = lattice_dims_check("shortest_paths", nx, ny, nz, kSceneProbeMaxQueries)) || (rc = step_finite_check("shortest_paths", step3))) return rc; }
    const size_t n = (size_t)nx * ny * nz;
    { const int rc = paths_args_check("shortest_paths", connectivity, seeds, n_seeds, n, max_cost, cost); if (rc) return rc; }
    if (cell_cost) for (size_t i = 0; i < n; ++i) if (!std::isfinite(cell_cost[i]) || cell_cost[i] < 0.f) {
        set_error("shortest_paths: cell_cost[%zu] is %g (finite, >= 0)", i, (double)cell_cost[i]); return MON_ERR_ARG; }
    return MON_OK;
}
int scene_paths_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float clearance, float soft_radius,
                      float soft_weight, int connectivity, const int32_t* seeds, size_t n_seeds, float max_cost, const float* cost) {
    {   int rc;
        if ((rc = lattice_route_check("scene_paths", side, origin3, step3, nx, ny, nz, sigma_min)) || (rc = nonneg_check("scene_paths", "clearance", clearance)) ||
            (rc = nonneg_check("scene_paths", "soft_weight", soft_weight))) return rc; }
    if (soft_weight > 0.f && (!std::isfinite(soft_radius) || !(soft_radius > 0.f))) {
        set_error("scene_paths: soft_radius %g (finite, above 0, with a soft_weight above 0)", (double)soft_radius); return MON_ERR_ARG; }
    return paths_args_check("scene_paths", connectivity, seeds, n_seeds, (size_t)nx * ny * nz, max_cost, cost);
}
// The sweeps on stream s until one leaves no work.  d_raised: kPathsBatch words on the device, h_raised: as many on the host (pinned in the scene call).
// At most n + 1 sweeps: a sweep that leaves work has carried some cell's least walk across a tile border, and Bellman-Ford needs no more than n rounds.
static int paths_relax(const char* what, hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, const float* mult, float* cost, uint8_t* flags,
                       uint32_t* d_raised, uint32_t* h_raised) {
    const uint64_t cap = (uint64_t)g.n() + 1u;
    uint32_t sweeps = 0, batches = 0;
    for (;;) {
        const uint32_t b = (uint32_t)std::min<uint64_t>(kPathsBatch, cap - sweeps);
        HIPCHECK(hipMemsetAsync(d_raised, 0, 4 * (size_t)b, s));
        for (uint32_t k = 0; k < b; ++k) launch_paths_sweep(s, occ, g, connectivity, mult, cost, flags, sweeps + k, d_raised + k);
        HIPCHECK(hipMemcpyAsync(h_raised, d_raised, 4 * (size_t)b, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipGetLastError());
        uint32_t busy = 0; while (busy < b && h_raised[busy]) ++busy;
        g_paths_stats[0] = sweeps + b; g_paths_stats[1] = ++batches; g_paths_stats[2] = sweeps + busy;
        if (busy < b) return MON_OK;
        sweeps += b;
        if (sweeps >= cap) { set_error("%s: the field did not settle within %llu sweeps; no output was written", what, (unsigned long long)cap); return MON_ERR_STATE; }
    }
}
// mon_shortest_paths: the field alone on a host mask, in buffers of its own on the device's default stream.
// w: working cost n | cost n | next n | multiplier n | seeds | a batch's words
int shortest_paths(int device, const uint8_t* passable, int nx, int ny, int nz, const float* step3, int connectivity, const float* cell_cost,
                   const int32_t* seeds, size_t n_seeds, float max_cost, float* cost, int32_t* next) {
    { const int rc = device_enter(device); if (rc) return rc; }
    const Lattice g(nullptr, step3, nx, ny, nz); const size_t n = g.n();
    DevBuf<uint8_t> occ, flags; DevBuf<uint32_t> w;
    { int rc; if ((rc = occ.grow(n)) || (rc = flags.grow(2 * (size_t)paths_tiles(g))) || (rc = w.grow(4 * n + n_seeds + kPathsBatch))) return rc; }
    float* d_work = reinterpret_cast<float*>(w.p); float* d_cost = d_work + n; int32_t* d_next = reinterpret_cast<int32_t*>(w.p + 2 * n);
    float* d_mult = cell_cost ? reinterpret_cast<float*>(w.p + 3 * n) : nullptr; int32_t* d_seeds = reinterpret_cast<int32_t*>(w.p + 4 * n);
    uint32_t* d_raised = w.p + 4 * n + n_seeds;
    HIPCHECK(hipMemcpy(occ.p, passable, n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_seeds, seeds, 4 * n_seeds, hipMemcpyHostToDevice));
    if (cell_cost) HIPCHECK(hipMemcpy(d_mult, cell_cost, 4 * n, hipMemcpyHostToDevice));
    launch_paths_init(nullptr, occ.p, g, d_seeds, (uint32_t)n_seeds, d_work, flags.p);
    std::vector<uint32_t> h_raised(kPathsBatch);
    { const int rc = paths_relax("shortest_paths", nullptr, occ.p, g, connectivity, d_mult, d_work, flags.p, d_raised, h_raised.data());
      if (rc) return rc; }
    launch_paths_finish(nullptr, occ.p, g, connectivity, d_mult, d_work, max_cost, d_cost, next ? d_next : nullptr);
    HIPCHECK(hipGetLastError());
    std::vector<uint32_t> h(next ? 2 * n : n);                                      // (the caller's arrays are written only once everything has succeeded)
    HIPCHECK(hipMemcpy(h.data(), d_cost, 4 * h.size(), hipMemcpyDeviceToHost));
    std::memcpy(cost, h.data(), 4 * n);
    if (next) std::memcpy(next, h.data() + n, 4 * n);
    return MON_OK;
}
// q: a lattice (scene_lattice).  ids as scene_points', applied to owner.
int scene_paths(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float clearance, float soft_radius, float soft_weight,
                int connectivity, const int32_t* seeds, size_t n_seeds, float max_cost, float* cost, int32_t* next, float* dist, float* sigma, int32_t* owner,
                const int32_t* ids) {
    SceneCall c; { const int rc = c.enter("scene_paths", ms, n, side, false); if (rc) return rc; }
    SceneWs& ws = *c.ws; const hipStream_t s = c.s;
    const size_t n_q = q.n; const uint32_t nq = (uint32_t)n_q;
    // the area: cost | next | dist | sigma | owner, then the fold's other rows
    Area A{ n_q }; const size_t r_cost = A.out(cost), r_next = A.out(next), r_dist = A.out(dist);
    FoldRows f; f.sigma = A.out(sigma); f.owner = A.out(owner, 1, true); fold_rows_rest(A, f, false);
    {   int rc;
        if ((rc = ws.pcost.grow(n_q)) || (soft_weight > 0.f && (rc = ws.pmul.grow(n_q))) || (rc = ws.pseeds.grow(n_seeds)) ||
            (rc = ws.pflags.grow(2 * (size_t)paths_tiles(q.g))) || (rc = ws.praised.grow(kPathsBatch)) || (rc = ws.h_raised.grow(kPathsBatch))) return rc; }
    const float* mult = soft_weight > 0.f ? ws.pmul.p : nullptr;
    HIPCHECK(hipMemcpyAsync(ws.pseeds.p, seeds, 4 * n_seeds, hipMemcpyHostToDevice, s));
    { int rc; if ((rc = lattice_occupancy(c, ms, n, q, A, f, sigma_min)) || (rc = lattice_clearance(c, q, r_dist, clearance))) return rc; }
    float* o = ws.out.p;
    if (mult) launch_paths_soft(s, nq, o + r_dist, soft_radius, soft_weight, ws.pmul.p);
    launch_paths_init(s, ws.docc.p, q.g, ws.pseeds.p, (uint32_t)n_seeds, ws.pcost.p, ws.pflags.p);
    { const int rc = paths_relax("scene_paths", s, ws.docc.p, q.g, connectivity, mult, ws.pcost.p, ws.pflags.p, ws.praised.p, ws.h_raised.p); if (rc) return rc; }
    launch_paths_finish(s, ws.docc.p, q.g, connectivity, mult, ws.pcost.p, max_cost, o + r_cost, next ? as_i32(o + r_next) : nullptr);
    { const int rc = c.home(A.home); if (rc) return rc; }
    A.unpack(ws.h_out.p, ids);
    return MON_OK;
}
// mon_lattice_path: the cells from start along next to the first -1.  A walk of more than n_cells cells has come by some cell twice: a damaged array.
int lattice_path(const int32_t* next, size_t n_cells, int32_t start, int32_t* path, size_t cap, size_t* n_path) {
    REQUIRE_ARG("lattice_path", next, "next"); REQUIRE_ARG("lattice_path", n_path, "n_path");
    if (cap > 0) REQUIRE_ARG("lattice_path", path, "path");
    if (start < 0 || (size_t)start >= n_cells) { set_error("lattice_path: start %d (0 to %zu)", start, n_cells ? n_cells - 1 : 0); return MON_ERR_ARG; }
    size_t len = 0;
    for (int32_t v = start; v != -1; v = next[v]) {                                 // first pass: the array is sound and the length known before path is touched
        if (v < -1 || (size_t)v >= n_cells) { set_error("lattice_path: next holds %d behind cell %zu of the walk (-1, or 0 to %zu)", v, len, n_cells - 1);
            return MON_ERR_ARG; }
        if (++len > n_cells) { set_error("lattice_path: the walk from %d is longer than the lattice's %zu cells (next holds a cycle)", start, n_cells);
            return MON_ERR_ARG; }
    }
    size_t k = 0;
    for (int32_t v = start; v != -1 && k < cap; v = next[v]) path[k++] = v;
    *n_path = len;
    return MON_OK;
}

}  // namespace mon
