// dist_field.cpp -- device-resident distance fields (mon_dist_field_*): the handle, the standalone calls and the launch wrappers.  A
// DistField is a snapshot: its cells in device memory of its own, the lattice they sit on, a stream and the scratch of its calls.  It refers to no object
// and to no manager.  A sample or score call uploads its inputs, enqueues one kernel and the copy of its outputs to the pinned staging on the handle's
// stream, and synchronises once; calls on one handle take turns on its mutex.  (mon_scene_dist_field's chain is scene_field.cpp's: it fills a handle made by
// dist_field_adopt.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include "model_internal.h"

namespace mon {

constexpr size_t kFieldMaxPoints = (size_t)1 << 24, kFieldMaxSpheres = 32, kFieldMaxWays = 256, kFieldMaxSub = 16, kFieldMaxTraj = 65536,
                 kFieldMaxSamples = (size_t)1 << 24, kFieldMaxCells = (size_t)1 << 22;

struct DistField {
    std::mutex mu;
    int device = 0, nx = 1, ny = 1, nz = 1; float origin[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 }, max_value = 0.f;
    float* cells = nullptr; hipStream_t s = nullptr;
    DevBuf<float> in, out; PinnedBuf<float> h_out;                                   // a call's inputs, its outputs and their pinned staging
    size_t n() const { return (size_t)nx * ny * nz; }
    DistFieldView view() const {
        DistFieldView v{ cells, nx, ny, nz, { origin[0], origin[1], origin[2] }, { step[0], step[1], step[2] } };
        return v;
    }
};
float* dist_field_cells(DistField& f) { return f.cells; }
void dist_field_set_max(DistField& f, float max_value) { f.max_value = max_value; }
void dist_field_free(DistField* f) {
    if (!f) return;
    if (use_device(f->device) == hipSuccess) {
        if (f->s) { (void)hipStreamSynchronize(f->s); (void)hipStreamDestroy(f->s); }
        if (f->cells) (void)hipFree(f->cells);
        f->in.release(); f->out.release(); f->h_out.release();
    }
    delete f;
}
// the handle of a lattice with its cells' room and its stream; the caller has set the device
int dist_field_adopt(int device, const ScenePoints& q, DistField** out) {
    DistField* f = new DistField();
    f->device = device; f->nx = q.nx; f->ny = q.ny; f->nz = q.nz;
    for (int a = 0; a < 3; ++a) { f->origin[a] = q.origin[a]; f->step[a] = q.step[a]; }
    hipError_t e = hipMalloc((void**)&f->cells, 4 * f->n());
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("dist_field: no room for a field of %zu cells: %s", f->n(), hipGetErrorString(e)); dist_field_free(f); return MON_ERR_HIP; }
    *out = f;
    return MON_OK;
}

// ---- what the calls ask of their arguments, without a device
static int field_dims_check(const char* what, int nx, int ny, int nz) {
    if (nx < 1 || ny < 1 || nz < 1) { set_error("%s: lattice %d x %d x %d (each at least 1)", what, nx, ny, nz); return MON_ERR_ARG; }
    // (each factor bounded before it is multiplied: three ints of up to 2^31 - 1 wrap a 64-bit product)
    const uint64_t mx = kFieldMaxCells;
    if ((uint64_t)nx > mx || (uint64_t)ny > mx / (uint64_t)nx || (uint64_t)nz > mx / ((uint64_t)nx * (uint64_t)ny)) {
        set_error("%s: lattice %d x %d x %d has more than %zu points", what, nx, ny, nz, kFieldMaxCells); return MON_ERR_ARG; }
    return MON_OK;
}
int dist_field_create_check(const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, const void* field_out) {
    const char* what = "dist_field_create";
    REQUIRE_ARG(what, field_out, "field"); REQUIRE_ARG(what, dist, "dist"); REQUIRE_ARG(what, origin3, "origin"); REQUIRE_ARG(what, step3, "step");
    { const int rc = field_dims_check(what, nx, ny, nz); if (rc) return rc; }
    const int dims[3] = { nx, ny, nz };
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin3[a])) { set_error("%s: origin is not finite", what); return MON_ERR_ARG; }
        if (dims[a] > 1 && (!std::isfinite(step3[a]) || step3[a] == 0.f)) {
            set_error("%s: step %g on axis %d, which has %d cells (finite, not 0)", what, (double)step3[a], a, dims[a]); return MON_ERR_ARG; }
    }
    const size_t n = (size_t)nx * ny * nz;
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(dist[i])) { set_error("%s: dist[%zu] is not finite", what, i); return MON_ERR_ARG; }
    return MON_OK;
}
int dist_field_create(int device, const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, DistField** out) {
    int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("no HIP device available"); return MON_ERR_NO_DEVICE; }
    HIPCHECK(use_device(device));
    ScenePoints q = scene_lattice(origin3, step3, nx, ny, nz);
    const int dims[3] = { nx, ny, nz };
    for (int a = 0; a < 3; ++a) if (dims[a] == 1) q.step[a] = 0.f;                  // (ignored; what mon_dist_field_info reports of it)
    DistField* f = nullptr;
    { const int rc = dist_field_adopt(device, q, &f); if (rc) return rc; }
    const hipError_t e = hipMemcpy(f->cells, dist, 4 * q.n, hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error("dist_field_create: the upload failed: %s", hipGetErrorString(e)); dist_field_free(f); return MON_ERR_HIP; }
    f->max_value = *std::max_element(dist, dist + q.n);
    *out = f;
    return MON_OK;
}

int dist_field_info(DistField* f, mon_dist_field_desc* info) {
    REQUIRE_ARG("dist_field_info", f, "field"); REQUIRE_ARG("dist_field_info", info, "info");
    std::lock_guard<std::mutex> l(f->mu);
    info->nx = f->nx; info->ny = f->ny; info->nz = f->nz; info->device = f->device; info->max_value = f->max_value;
    for (int a = 0; a < 3; ++a) { info->origin[a] = f->origin[a]; info->step[a] = f->step[a]; }
    return MON_OK;
}
// a call's outputs: out.p's first `floats` to the pinned staging, one synchronisation
static int field_home(DistField& f, size_t floats) {
    HIPCHECK(hipMemcpyAsync(f.h_out.p, f.out.p, 4 * floats, hipMemcpyDeviceToHost, f.s));
    HIPCHECK(hipStreamSynchronize(f.s));
    HIPCHECK(hipGetLastError());
    return MON_OK;
}
int dist_field_read(DistField* f, float* dist_out) {
    REQUIRE_ARG("dist_field_read", f, "field"); REQUIRE_ARG("dist_field_read", dist_out, "dist_out");
    std::lock_guard<std::mutex> l(f->mu);
    HIPCHECK(use_device(f->device));
    const size_t n = f->n();
    { const int rc = f->h_out.grow(n); if (rc) return rc; }
    HIPCHECK(hipMemcpyAsync(f->h_out.p, f->cells, 4 * n, hipMemcpyDeviceToHost, f->s));
    HIPCHECK(hipStreamSynchronize(f->s));
    std::memcpy(dist_out, f->h_out.p, 4 * n);                                       // (the caller's array is written only once everything has succeeded)
    return MON_OK;
}
int dist_field_sample(DistField* f, const float* xyz, size_t n, float outside, float* dist_out, float* grad3_out) {
    const char* what = "dist_field_sample";
    REQUIRE_ARG(what, xyz, "xyz"); REQUIRE_ARG(what, dist_out, "dist_out");
    if (n == 0 || n > kFieldMaxPoints) { set_error("%s: %zu points (1 to %zu)", what, n, kFieldMaxPoints); return MON_ERR_ARG; }
    REQUIRE_ARG(what, f, "field");                                                  // (last: what needs no handle is judged without one)
    std::lock_guard<std::mutex> l(f->mu);
    HIPCHECK(use_device(f->device));
    const size_t n_out = grad3_out ? 4 * n : n;
    { int rc; if ((rc = f->in.grow(3 * n)) || (rc = f->out.grow(n_out)) || (rc = f->h_out.grow(n_out))) return rc; }
    HIPCHECK(hipMemcpyAsync(f->in.p, xyz, 12 * n, hipMemcpyHostToDevice, f->s));
    launch_field_sample(f->s, f->view(), f->in.p, (uint32_t)n, outside, f->out.p, grad3_out ? f->out.p + n : nullptr);
    { const int rc = field_home(*f, n_out); if (rc) return rc; }
    std::memcpy(dist_out, f->h_out.p, 4 * n);
    if (grad3_out) std::memcpy(grad3_out, f->h_out.p + n, 12 * n);
    return MON_OK;
}
static int score_check(const char* what, const DistField* f, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj,
                       size_t n_way, size_t n_sub, const mon_traj_score_params* p, const float* min_clear) {
    REQUIRE_ARG(what, spheres, "spheres"); REQUIRE_ARG(what, ways, "ways"); REQUIRE_ARG(what, p, "params");
    REQUIRE_ARG(what, min_clear, "min_clear");
    if (n_spheres == 0 || n_spheres > kFieldMaxSpheres) { set_error("%s: %zu spheres (1 to %zu)", what, n_spheres, kFieldMaxSpheres); return MON_ERR_ARG; }
    if (way_floats != 3 && way_floats != 16) { set_error("%s: way_floats %d (3: a position, 16: a 4 x 4 matrix)", what, way_floats); return MON_ERR_ARG; }
    if (n_way == 0 || n_way > kFieldMaxWays) { set_error("%s: n_way %zu (1 to %zu)", what, n_way, kFieldMaxWays); return MON_ERR_ARG; }
    if (n_sub == 0 || n_sub > kFieldMaxSub) { set_error("%s: n_sub %zu (1 to %zu)", what, n_sub, kFieldMaxSub); return MON_ERR_ARG; }
    if (n_traj == 0 || n_traj > kFieldMaxTraj) { set_error("%s: n_traj %zu (1 to %zu)", what, n_traj, kFieldMaxTraj); return MON_ERR_ARG; }
    const size_t n_samp = (n_way - 1) * n_sub + 1;
    if (n_traj * n_samp > kFieldMaxSamples) { set_error("%s: %zu trajectories of %zu samples (at most %zu samples in all)", what, n_traj, n_samp,
        kFieldMaxSamples); return MON_ERR_ARG; }
    for (size_t k = 0; k < n_spheres; ++k) {
        const float* b = spheres + 4 * k;
        if (!std::isfinite(b[0]) || !std::isfinite(b[1]) || !std::isfinite(b[2]) || !std::isfinite(b[3]) || b[3] < 0.f) {
            set_error("%s: sphere %zu is (%g %g %g) r %g (finite, r >= 0)", what, k, (double)b[0], (double)b[1], (double)b[2], (double)b[3]); return MON_ERR_ARG; }
    }
    if (!std::isfinite(p->outside) || !std::isfinite(p->margin) || !std::isfinite(p->safe)) { set_error("%s: a param is not finite", what); return MON_ERR_ARG; }
    REQUIRE_ARG(what, f, "field");                                                  // (last: what needs no handle is judged without one)
    return MON_OK;
}
// in: spheres [n_spheres][4] (padded to 32 records) | ways.  out: min_clear | first_hit | cost (n_traj each) | way_clear | way_grad, those asked for
int dist_field_score(DistField* f, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj, size_t n_way, size_t n_sub,
                     const mon_traj_score_params* p, float* min_clear, int32_t* first_hit, float* cost, float* way_clear, float* way_grad) {
    const char* what = "dist_field_score";
    { const int rc = score_check(what, f, spheres, n_spheres, ways, way_floats, n_traj, n_way, n_sub, p, min_clear); if (rc) return rc; }
    std::lock_guard<std::mutex> l(f->mu);
    HIPCHECK(use_device(f->device));
    const size_t n_ways = n_traj * n_way, way_words = n_ways * (size_t)way_floats, at_ways = 4 * kFieldMaxSpheres;
    const size_t r_min = 0, r_hit = n_traj, r_cost = 2 * n_traj, r_wc = 3 * n_traj, r_wg = r_wc + (way_clear ? n_ways : 0), n_out = r_wg + (way_grad ? 3 * n_ways : 0);
    { int rc; if ((rc = f->in.grow(at_ways + way_words)) || (rc = f->out.grow(n_out)) || (rc = f->h_out.grow(n_out))) return rc; }
    HIPCHECK(hipMemcpyAsync(f->in.p, spheres, 16 * n_spheres, hipMemcpyHostToDevice, f->s));
    HIPCHECK(hipMemcpyAsync(f->in.p + at_ways, ways, 4 * way_words, hipMemcpyHostToDevice, f->s));
    float* o = f->out.p;
    TrajScoreArgs a{};
    a.n_traj = (uint32_t)n_traj; a.n_way = (uint32_t)n_way; a.n_sub = (uint32_t)n_sub; a.n_samp = (uint32_t)((n_way - 1) * n_sub + 1);
    a.outside = p->outside; a.margin = p->margin; a.safe = p->safe;
    a.min_clear = o + r_min; a.first_hit = first_hit ? reinterpret_cast<int32_t*>(o + r_hit) : nullptr; a.cost = cost ? o + r_cost : nullptr;
    a.way_clear = way_clear ? o + r_wc : nullptr; a.way_grad = way_grad ? o + r_wg : nullptr;
    launch_traj_score(f->s, f->view(), f->in.p, (uint32_t)n_spheres, f->in.p + at_ways, way_floats == 16, a);
    { const int rc = field_home(*f, n_out); if (rc) return rc; }
    const float* h = f->h_out.p;
    std::memcpy(min_clear, h + r_min, 4 * n_traj);
    if (first_hit) std::memcpy(first_hit, h + r_hit, 4 * n_traj);
    if (cost) std::memcpy(cost, h + r_cost, 4 * n_traj);
    if (way_clear) std::memcpy(way_clear, h + r_wc, 4 * n_ways);
    if (way_grad) std::memcpy(way_grad, h + r_wg, 12 * n_ways);
    return MON_OK;
}

}  // namespace mon
