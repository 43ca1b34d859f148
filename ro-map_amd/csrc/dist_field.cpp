// dist_field.cpp -- device-resident distance fields (mon_dist_field_*): the handle, the standalone calls and the launch wrappers.  A
// DistField is a snapshot: its cells in device memory of its own, the lattice they sit on, a stream and the scratch of its calls.  It refers to no object
// and to no manager.  A call on a handle goes through FieldCall (the handle's lock and device, room for inputs, outputs and staging, one copy home): it uploads its
// inputs, enqueues one kernel and the copy of its outputs to the pinned staging on the handle's stream, and synchronises once; calls on one handle take
// turns on its mutex.  The sample, score and trace calls describe their outputs once, as an Area (model_internal.h): the pieces' offsets give the kernels'
// pointers, A.end sizes room and home, A.unpack fills the caller's arrays.  (mon_scene_dist_field's chain is scene_field.cpp's: it fills a handle made by
// dist_field_adopt.)  Scan matching (mon_dist_field_match, mon_dist_field_register) is here too: the match call follows the same
// pattern; the register call keeps the scan on the device and runs Levenberg-Marquardt over all hypotheses in lockstep, one match launch, one read-back and
// one synchronisation per round, with the 6 x 6 solves and the pose updates on the host in double.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "model_internal.h"

namespace mon {

constexpr size_t kFieldMaxPoints = (size_t)1 << 24, kFieldMaxSpheres = 32, kFieldMaxWays = 256, kFieldMaxSub = 16, kFieldMaxTraj = 65536,
                 kFieldMaxSamples = (size_t)1 << 24, kFieldMaxCells = (size_t)1 << 22;

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
int dist_field_adopt(int device, const Lattice& g, DistField** out) {
    DistField* f = new DistField();
    f->device = device; f->g = g;
    hipError_t e = hipMalloc((void**)&f->cells, 4 * g.n());
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->s, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("dist_field: no room for a field of %zu cells: %s", g.n(), hipGetErrorString(e)); dist_field_free(f); return MON_ERR_HIP; }
    *out = f;
    return MON_OK;
}

// ---- what the calls ask of their arguments, without a device
int dist_field_create_check(const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, const void* field_out) {
    const char* what = "dist_field_create";
    REQUIRE_ARG(what, field_out, "field"); REQUIRE_ARG(what, dist, "dist"); REQUIRE_ARG(what, origin3, "origin"); REQUIRE_ARG(what, step3, "step");
    { const int rc = lattice_dims_check(what, nx, ny, nz, kFieldMaxCells); if (rc) return rc; }
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
    { const int rc = device_enter(device); if (rc) return rc; }
    Lattice g(origin3, step3, nx, ny, nz);
    const int dims[3] = { nx, ny, nz };
    for (int a = 0; a < 3; ++a) if (dims[a] == 1) g.step[a] = 0.f;                  // (ignored; what mon_dist_field_info reports of it)
    DistField* f = nullptr;
    { const int rc = dist_field_adopt(device, g, &f); if (rc) return rc; }
    const hipError_t e = hipMemcpy(f->cells, dist, 4 * g.n(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { set_error("dist_field_create: the upload failed: %s", hipGetErrorString(e)); dist_field_free(f); return MON_ERR_HIP; }
    f->max_value = *std::max_element(dist, dist + g.n());
    *out = f;
    return MON_OK;
}

int dist_field_info(DistField* f, mon_dist_field_desc* info) {
    REQUIRE_ARG("dist_field_info", f, "field"); REQUIRE_ARG("dist_field_info", info, "info");
    std::lock_guard<std::mutex> l(f->mu);
    info->nx = f->g.nx; info->ny = f->g.ny; info->nz = f->g.nz; info->device = f->device; info->max_value = f->max_value;
    for (int a = 0; a < 3; ++a) { info->origin[a] = f->g.origin[a]; info->step[a] = f->g.step[a]; }
    return MON_OK;
}
// One call on a handle, the counterpart of SceneCall (scene.cpp).  enter: the handle -- judged last, what needs no handle has been judged without one -- its
// lock, which the call holds until it goes, and its device.  room: the call's inputs, outputs and their pinned staging (floats; 0: not used).  home: `floats`
// from `from` (the handle's memory) to the staging, one synchronisation, the launches' error.
struct FieldCall {
    DistField* f = nullptr; std::unique_lock<std::mutex> lock;
    int enter(const char* what, DistField* field) {
        REQUIRE_ARG(what, field, "field");
        f = field; lock = std::unique_lock<std::mutex>(f->mu);
        HIPCHECK(use_device(f->device));
        return MON_OK;
    }
    int room(size_t in, size_t out, size_t h_out) {
        int rc; if ((in && (rc = f->in.grow(in))) || (out && (rc = f->out.grow(out))) || (rc = f->h_out.grow(h_out))) return rc;
        return MON_OK;
    }
    int home(const float* from, size_t floats) {
        HIPCHECK(hipMemcpyAsync(f->h_out.p, from, 4 * floats, hipMemcpyDeviceToHost, f->s));
        HIPCHECK(hipStreamSynchronize(f->s));
        HIPCHECK(hipGetLastError());
        return MON_OK;
    }
};
int dist_field_read(DistField* field, float* dist_out) {
    FieldCall c; { const int rc = c.enter("dist_field_read", field); if (rc) return rc; }
    REQUIRE_ARG("dist_field_read", dist_out, "dist_out");
    DistField& f = *c.f; const size_t n = f.g.n();
    { int rc; if ((rc = c.room(0, 0, n)) || (rc = c.home(f.cells, n))) return rc; }
    std::memcpy(dist_out, f.h_out.p, 4 * n);                                        // (the caller's array is written only once everything has succeeded)
    return MON_OK;
}
int dist_field_sample(DistField* field, const float* xyz, size_t n, float outside, float* dist_out, float* grad3_out) {
    const char* what = "dist_field_sample";
    REQUIRE_ARG(what, xyz, "xyz"); REQUIRE_ARG(what, dist_out, "dist_out");
    if (n == 0 || n > kFieldMaxPoints) { set_error("%s: %zu points (1 to %zu)", what, n, kFieldMaxPoints); return MON_ERR_ARG; }
    FieldCall c; { const int rc = c.enter(what, field); if (rc) return rc; }
    DistField& f = *c.f;
    Area A; const size_t r_dist = A.piece(dist_out, n), r_grad = A.piece(grad3_out, grad3_out ? 3 * n : 0);
    { const int rc = c.room(3 * n, A.end, A.end); if (rc) return rc; }
    HIPCHECK(hipMemcpyAsync(f.in.p, xyz, 12 * n, hipMemcpyHostToDevice, f.s));
    launch_field_sample(f.s, f.cells, f.g, f.in.p, (uint32_t)n, outside, f.out.p + r_dist, grad3_out ? f.out.p + r_grad : nullptr);
    { const int rc = c.home(f.out.p, A.end); if (rc) return rc; }
    A.unpack(f.h_out.p, nullptr);
    return MON_OK;
}
static int score_check(const char* what, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj,
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
    return MON_OK;
}
// in: spheres [n_spheres][4] (padded to 32 records) | ways.  out: min_clear | first_hit | cost (n_traj each, asked for or not) | way_clear | way_grad, those
// asked for; the whole area comes home
int dist_field_score(DistField* field, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj, size_t n_way, size_t n_sub,
                     const mon_traj_score_params* p, float* min_clear, int32_t* first_hit, float* cost, float* way_clear, float* way_grad) {
    const char* what = "dist_field_score";
    { const int rc = score_check(what, spheres, n_spheres, ways, way_floats, n_traj, n_way, n_sub, p, min_clear); if (rc) return rc; }
    FieldCall c; { const int rc = c.enter(what, field); if (rc) return rc; }
    DistField& f = *c.f;
    const size_t n_ways = n_traj * n_way, way_words = n_ways * (size_t)way_floats, at_ways = 4 * kFieldMaxSpheres;
    Area A; const size_t r_min = A.piece(min_clear, n_traj), r_hit = A.piece(first_hit, n_traj), r_cost = A.piece(cost, n_traj);
    const size_t r_wc = A.piece(way_clear, way_clear ? n_ways : 0), r_wg = A.piece(way_grad, way_grad ? 3 * n_ways : 0);
    { const int rc = c.room(at_ways + way_words, A.end, A.end); if (rc) return rc; }
    HIPCHECK(hipMemcpyAsync(f.in.p, spheres, 16 * n_spheres, hipMemcpyHostToDevice, f.s));
    HIPCHECK(hipMemcpyAsync(f.in.p + at_ways, ways, 4 * way_words, hipMemcpyHostToDevice, f.s));
    float* o = f.out.p;
    TrajScoreArgs a{};
    a.n_traj = (uint32_t)n_traj; a.n_way = (uint32_t)n_way; a.n_sub = (uint32_t)n_sub; a.n_samp = (uint32_t)((n_way - 1) * n_sub + 1);
    a.outside = p->outside; a.margin = p->margin; a.safe = p->safe;
    a.min_clear = o + r_min; a.first_hit = first_hit ? reinterpret_cast<int32_t*>(o + r_hit) : nullptr; a.cost = cost ? o + r_cost : nullptr;
    a.way_clear = way_clear ? o + r_wc : nullptr; a.way_grad = way_grad ? o + r_wg : nullptr;
    launch_traj_score(f.s, f.cells, f.g, f.in.p, (uint32_t)n_spheres, f.in.p + at_ways, way_floats == 16, a);
    { const int rc = c.home(f.out.p, A.end); if (rc) return rc; }
    A.unpack(f.h_out.p, nullptr);
    return MON_OK;
}

// ---- scan matching.  What the two calls ask of the scan and the poses, without a device
constexpr size_t kMatchMaxPoints = (size_t)1 << 20, kMatchMaxPoses = 4096, kMatchMaxWork = (size_t)1 << 26;
static int match_check(const char* what, const float* points, size_t n, const float* poses16, size_t H, const float* pivots, float huber, float outside) {
    if (n == 0 || n > kMatchMaxPoints) { set_error("%s: %zu points (1 to %zu)", what, n, kMatchMaxPoints); return MON_ERR_ARG; }
    if (H == 0 || H > kMatchMaxPoses) { set_error("%s: %zu poses (1 to %zu)", what, H, kMatchMaxPoses); return MON_ERR_ARG; }
    if (n * H > kMatchMaxWork) { set_error("%s: %zu points under %zu poses (at most %zu pairs in all)", what, n, H, kMatchMaxWork); return MON_ERR_ARG; }
    for (size_t h = 0; h < H; ++h) {
        for (int k = 0; k < 12; ++k) if (!std::isfinite(poses16[16 * h + k])) { set_error("%s: pose %zu is not finite", what, h); return MON_ERR_ARG; }
        for (int k = 0; pivots && k < 3; ++k) if (!std::isfinite(pivots[3 * h + k])) { set_error("%s: pivot %zu is not finite", what, h); return MON_ERR_ARG; }
    }
    if (!(huber > 0.f)) { set_error("%s: huber %g (above 0; +inf is allowed)", what, (double)huber); return MON_ERR_ARG; }
    if (!std::isfinite(outside)) { set_error("%s: outside is not finite", what); return MON_ERR_ARG; }
    return MON_OK;
}
// The device side of both calls, on the locked handle.  in: points (3 n floats, rounded up to a multiple of 4) | poses [H][16] | pivots [H][3]; out: the
// kernels' scratch | rows.  match_room makes room for H poses; match_round uploads `live` poses (and pivots) and brings their rows home: 32 words per pose,
// or 4 without the normal equations.
struct MatchRoom { size_t at_pose, at_rows; };
static size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }
static int match_room(FieldCall& c, const float* points, size_t n, size_t H, MatchRoom& r) {
    r.at_pose = round4(3 * n); r.at_rows = round4(scan_match_scratch((uint32_t)n, (uint32_t)H));
    { const int rc = c.room(r.at_pose + 19 * H, r.at_rows + kScanMatchRow * H, kScanMatchRow * H); if (rc) return rc; }
    HIPCHECK(hipMemcpyAsync(c.f->in.p, points, 12 * n, hipMemcpyHostToDevice, c.f->s));
    return MON_OK;
}
static int match_round(FieldCall& c, const MatchRoom& r, size_t n, const float* poses16, const float* pivots, size_t live, float huber, float outside,
                       bool normal) {
    DistField& f = *c.f;
    float* d_pose = f.in.p + r.at_pose; float* d_piv = d_pose + 16 * live;
    HIPCHECK(hipMemcpyAsync(d_pose, poses16, 64 * live, hipMemcpyHostToDevice, f.s));
    if (pivots) HIPCHECK(hipMemcpyAsync(d_piv, pivots, 12 * live, hipMemcpyHostToDevice, f.s));
    const ScanMatchArgs a{ f.in.p, d_pose, pivots ? d_piv : nullptr, (uint32_t)n, (uint32_t)live, huber, outside };
    launch_scan_match(f.s, f.cells, f.g, a, normal, f.out.p, f.out.p + r.at_rows);
    return c.home(f.out.p + r.at_rows, (normal ? kScanMatchRow : kScanMatchLite) * live);
}
constexpr int kRowCost = 27, kRowInside = 28, kRowInlier = 29;                      // a full row: 21 A terms, 6 b terms, then these
// H rows of `width` words at home: the cost at column c0 and the two counts behind it (either may not be asked for)
static void rows_unpack(const float* rows, size_t H, size_t width, size_t c0, float* cost, int32_t* count1, int32_t* count2) {
    for (size_t h = 0; h < H; ++h) {
        const float* row = rows + width * h;
        cost[h] = row[c0];
        if (count1) count1[h] = (int32_t)row[c0 + 1];
        if (count2) count2[h] = (int32_t)row[c0 + 2];
    }
}

int dist_field_match(DistField* field, const float* points, size_t n, const float* poses16, size_t H, const float* pivots, const mon_scan_match_params* p,
                     float* cost, int32_t* n_inside, int32_t* n_inlier, float* normal) {
    const char* what = "dist_field_match";
    REQUIRE_ARG(what, points, "points"); REQUIRE_ARG(what, poses16, "poses16"); REQUIRE_ARG(what, p, "params"); REQUIRE_ARG(what, cost, "cost");
    { const int rc = match_check(what, points, n, poses16, H, pivots, p->huber, p->outside); if (rc) return rc; }
    FieldCall c; { const int rc = c.enter(what, field); if (rc) return rc; }
    DistField* const f = c.f; MatchRoom r;
    { const int rc = match_room(c, points, n, H, r); if (rc) return rc; }
    { const int rc = match_round(c, r, n, poses16, pivots, H, p->huber, p->outside, normal != nullptr); if (rc) return rc; }
    rows_unpack(f->h_out.p, H, normal ? kScanMatchRow : kScanMatchLite, normal ? kRowCost : 0, cost, n_inside, n_inlier);
    for (size_t h = 0; normal && h < H; ++h) std::memcpy(normal + 27 * h, f->h_out.p + kScanMatchRow * h, 4 * 27);
    return MON_OK;
}

int dist_field_register_default(DistField* f, mon_register_params* p) {
    REQUIRE_ARG("register_default", p, "p"); REQUIRE_ARG("register_default", f, "field");
    std::lock_guard<std::mutex> l(f->mu);
    const int dims[3] = { f->g.nx, f->g.ny, f->g.nz };
    float step = 0.f;
    for (int a = 0; a < 3; ++a) if (dims[a] > 1) step = std::max(step, std::fabs(f->g.step[a]));
    if (step == 0.f) step = 1.f;
    *p = mon_register_params{ 2.f * step, f->max_value, 30, 1e-3f, 10.f, 10.f, 1e6f, 1e-3f * step, 1e-4f, 6 };
    return MON_OK;
}

// (A + lambda diag(A)) delta = -b in double by Cholesky; row: 21 A terms (row-major upper triangle), then 6 b terms.  false: not positive definite
static bool lm_solve(const float* row, double lambda, double delta[6]) {
    double M[6][6], L[6][6] = {}, y[6];
    for (int i = 0, k = 0; i < 6; ++i) for (int j = i; j < 6; ++j, ++k) M[i][j] = M[j][i] = (double)row[k];
    for (int i = 0; i < 6; ++i) M[i][i] += lambda * M[i][i];
    for (int j = 0; j < 6; ++j) {
        double s = M[j][j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double t = M[i][j];
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) { double t = -(double)row[21 + i]; for (int k = 0; k < i; ++k) t -= L[i][k] * y[k]; y[i] = t / L[i][i]; }
    for (int i = 5; i >= 0; --i) { double t = y[i]; for (int k = i + 1; k < 6; ++k) t -= L[k][i] * delta[k]; delta[i] = t / L[i][i]; }
    for (int i = 0; i < 6; ++i) if (!std::isfinite(delta[i])) return false;
    return true;
}
// pose <- Exp(v, w) about the pivot c: R' = Exp(w) R, t' = Exp(w) (t - c) + c + v (Rodrigues in double), rounded to fp32; the last row is kept
static void lm_step(const float* pose, const float* c, const double delta[6], float* out) {
    const double wx = delta[3], wy = delta[4], wz = delta[5], th2 = wx * wx + wy * wy + wz * wz, th = std::sqrt(th2);
    const double A = th < 1e-8 ? 1.0 - th2 / 6.0 : std::sin(th) / th, B = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - std::cos(th)) / th2;
    const double K[3][3] = { { 0, -wz, wy }, { wz, 0, -wx }, { -wy, wx, 0 } };
    double E[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double kk = 0; for (int k = 0; k < 3; ++k) kk += K[i][k] * K[k][j];
        E[i][j] = (i == j ? 1.0 : 0.0) + A * K[i][j] + B * kk;
    }
    const double t[3] = { (double)pose[3] - c[0], (double)pose[7] - c[1], (double)pose[11] - c[2] };
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[4 * i + j] = (float)(E[i][0] * pose[j] + E[i][1] * pose[4 + j] + E[i][2] * pose[8 + j]);
        out[4 * i + 3] = (float)(E[i][0] * t[0] + E[i][1] * t[1] + E[i][2] * t[2] + (double)c[i] + delta[i]);
    }
    for (int j = 12; j < 16; ++j) out[j] = pose[j];
}

static int register_check(const char* what, const float* points, size_t n, const float* poses16_in, size_t H, const mon_register_params* p,
                          const float* poses16_out, const float* cost) {
    REQUIRE_ARG(what, points, "points"); REQUIRE_ARG(what, poses16_in, "poses16_in"); REQUIRE_ARG(what, p, "p"); REQUIRE_ARG(what, poses16_out, "poses16_out");
    REQUIRE_ARG(what, cost, "cost");
    { const int rc = match_check(what, points, n, poses16_in, H, nullptr, p->huber, p->outside); if (rc) return rc; }
    if (!std::isfinite(p->lambda0) || !std::isfinite(p->lambda_up) || !std::isfinite(p->lambda_down) || !std::isfinite(p->lambda_max) || !(p->lambda0 > 0.f) ||
        !(p->lambda_max > 0.f)) { set_error("%s: a lambda parameter is not finite or not above 0", what); return MON_ERR_ARG; }
    if (!(p->lambda_up > 1.f) || !(p->lambda_down > 1.f)) {
        set_error("%s: lambda factors %g and %g (each above 1)", what, (double)p->lambda_up, (double)p->lambda_down); return MON_ERR_ARG; }
    if (!std::isfinite(p->tol_trans) || !std::isfinite(p->tol_rot) || p->tol_trans < 0.f || p->tol_rot < 0.f) {
        set_error("%s: a tolerance is not finite or below 0", what); return MON_ERR_ARG; }
    if (p->max_evals < 1) { set_error("%s: max_evals %d (at least 1)", what, p->max_evals); return MON_ERR_ARG; }
    if (p->min_inside < 0) { set_error("%s: min_inside %d (at least 0)", what, p->min_inside); return MON_ERR_ARG; }
    return MON_OK;
}
// one hypothesis of the lockstep: its pose so far with that pose's row, the candidate under evaluation and the step that led to it
struct LmState { float pose[16], cand[16], pivot[3], row[kScanMatchRow]; double lambda, delta[6]; int32_t evals = 0, status = -1; };
// the next candidate of a running hypothesis; false: lambda went above lambda_max over failed factorisations (status 2)
static bool lm_propose(LmState& s, const mon_register_params& p) {
    while (!lm_solve(s.row, s.lambda, s.delta)) {
        s.lambda *= (double)p.lambda_up;
        if (s.lambda > (double)p.lambda_max) { s.status = 2; return false; }
    }
    lm_step(s.pose, s.pivot, s.delta, s.cand);
    return true;
}
int dist_field_register(DistField* field, const float* points, size_t n, const float* poses16_in, size_t H, const mon_register_params* p, float* poses16_out,
                        float* cost, int32_t* n_inside, int32_t* n_inlier, int32_t* evals, int32_t* status, int32_t* best) {
    const char* what = "dist_field_register";
    { const int rc = register_check(what, points, n, poses16_in, H, p, poses16_out, cost); if (rc) return rc; }
    FieldCall c; { const int rc = c.enter(what, field); if (rc) return rc; }
    // the pivots: each input pose applied to the centroid of the finite points (the scan is read only now; still before any device work)
    double cen[3] = { 0, 0, 0 }; size_t n_fin = 0;
    for (size_t i = 0; i < n; ++i) {
        const float* q = points + 3 * i;
        if (std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2])) { cen[0] += q[0]; cen[1] += q[1]; cen[2] += q[2]; ++n_fin; }
    }
    for (int a = 0; a < 3; ++a) cen[a] = n_fin ? cen[a] / (double)n_fin : 0.0;
    std::vector<LmState> st(H);
    std::vector<size_t> live(H);
    for (size_t h = 0; h < H; ++h) {
        LmState& s = st[h]; live[h] = h;
        std::memcpy(s.pose, poses16_in + 16 * h, 64); std::memcpy(s.cand, s.pose, 64);
        for (int a = 0; a < 3; ++a) {
            s.pivot[a] = (float)((double)s.pose[4 * a] * cen[0] + (double)s.pose[4 * a + 1] * cen[1] + (double)s.pose[4 * a + 2] * cen[2] + (double)s.pose[4 * a + 3]);
            if (!std::isfinite(s.pivot[a])) { set_error("%s: the pivot of pose %zu is not finite", what, h); return MON_ERR_ARG; }
        }
        s.lambda = (double)p->lambda0;
    }
    DistField* const f = c.f; MatchRoom r;
    { const int rc = match_room(c, points, n, H, r); if (rc) return rc; }
    std::vector<float> up(19 * H);
    for (bool first = true; !live.empty(); first = false) {
        // the candidates of the hypotheses still running: poses, then pivots, as match_round lays them out
        for (size_t k = 0; k < live.size(); ++k) {
            std::memcpy(up.data() + 16 * k, st[live[k]].cand, 64); std::memcpy(up.data() + 16 * live.size() + 3 * k, st[live[k]].pivot, 12);
        }
        { const int rc = match_round(c, r, n, up.data(), up.data() + 16 * live.size(), live.size(), p->huber, p->outside, true); if (rc) return rc; }
        std::vector<size_t> next;
        for (size_t k = 0; k < live.size(); ++k) {
            LmState& s = st[live[k]]; const float* row = f->h_out.p + kScanMatchRow * k;
            ++s.evals;
            bool small = false;
            if (first) {
                std::memcpy(s.row, row, 4 * kScanMatchRow);
                if (row[kRowInside] < (float)p->min_inside) { s.status = 3; continue; }
            } else if (row[kRowCost] < s.row[kRowCost]) {
                std::memcpy(s.pose, s.cand, 64); std::memcpy(s.row, row, 4 * kScanMatchRow);
                s.lambda /= (double)p->lambda_down;
                small = std::sqrt(s.delta[0] * s.delta[0] + s.delta[1] * s.delta[1] + s.delta[2] * s.delta[2]) < (double)p->tol_trans &&
                        std::sqrt(s.delta[3] * s.delta[3] + s.delta[4] * s.delta[4] + s.delta[5] * s.delta[5]) < (double)p->tol_rot;
            } else {
                s.lambda *= (double)p->lambda_up;
            }
            if (small) s.status = 0;
            else if (s.lambda > (double)p->lambda_max) s.status = 2;
            else if (s.evals >= p->max_evals) s.status = 1;
            else if (lm_propose(s, *p)) next.push_back(live[k]);
        }
        live.swap(next);
    }
    int32_t b = -1;
    for (size_t h = 0; h < H; ++h) {
        const LmState& s = st[h];
        std::memcpy(poses16_out + 16 * h, s.pose, 64);
        cost[h] = s.row[kRowCost];
        if (n_inside) n_inside[h] = (int32_t)s.row[kRowInside];
        if (n_inlier) n_inlier[h] = (int32_t)s.row[kRowInlier];
        if (evals) evals[h] = s.evals;
        if (status) status[h] = s.status;
        if (s.status != 3 && (b < 0 || s.row[kRowCost] < st[(size_t)b].row[kRowCost])) b = (int32_t)h;
    }
    if (best) *best = b;
    return MON_OK;
}

// ---- ray tracing.  What the two calls ask of the rays, the poses and the march, without a device
constexpr size_t kTraceMaxRays = (size_t)1 << 20, kTraceMaxPoses = 4096, kTraceMaxHome = (size_t)1 << 22, kTraceMaxBeams = (size_t)1 << 24;
constexpr int32_t kTraceMaxSteps = 4096;
static int trace_check(const char* what, size_t n, const float* poses16, size_t H, size_t max_work, const mon_trace_params* p) {
    if (n == 0 || n > kTraceMaxRays) { set_error("%s: %zu rays (1 to %zu)", what, n, kTraceMaxRays); return MON_ERR_ARG; }
    if (H == 0 || H > kTraceMaxPoses) { set_error("%s: %zu poses (1 to %zu)", what, H, kTraceMaxPoses); return MON_ERR_ARG; }
    if (n * H > max_work) { set_error("%s: %zu rays under %zu poses (at most %zu pairs in all)", what, n, H, max_work); return MON_ERR_ARG; }
    if (!poses16 && H != 1) { set_error("%s: %zu poses without poses16 (world rays are one pose)", what, H); return MON_ERR_ARG; }
    for (size_t h = 0; poses16 && h < H; ++h)
        for (int k = 0; k < 12; ++k) if (!std::isfinite(poses16[16 * h + k])) { set_error("%s: pose %zu is not finite", what, h); return MON_ERR_ARG; }
    if (!std::isfinite(p->t_min) || !std::isfinite(p->t_max) || !std::isfinite(p->eps) || !std::isfinite(p->step_min) || !std::isfinite(p->relax) ||
        !std::isfinite(p->step_outside)) { set_error("%s: a march parameter is not finite", what); return MON_ERR_ARG; }
    if (p->t_min > p->t_max) { set_error("%s: t_min %g above t_max %g", what, (double)p->t_min, (double)p->t_max); return MON_ERR_ARG; }
    if (!(p->step_min > 0.f) || !(p->step_outside > 0.f)) {
        set_error("%s: step_min %g, step_outside %g (each above 0)", what, (double)p->step_min, (double)p->step_outside); return MON_ERR_ARG; }
    if (!(p->relax > 0.f) || p->relax > 1.f) { set_error("%s: relax %g (above 0, at most 1)", what, (double)p->relax); return MON_ERR_ARG; }
    if (p->max_steps < 1 || p->max_steps > kTraceMaxSteps) { set_error("%s: max_steps %d (1 to %d)", what, p->max_steps, kTraceMaxSteps); return MON_ERR_ARG; }
    return MON_OK;
}
int dist_field_trace_default(DistField* f, mon_trace_params* p) {
    REQUIRE_ARG("trace_default", p, "p"); REQUIRE_ARG("trace_default", f, "field");
    std::lock_guard<std::mutex> l(f->mu);
    const int dims[3] = { f->g.nx, f->g.ny, f->g.nz };
    float c = INFINITY, sum = 0.f;
    for (int a = 0; a < 3; ++a) {
        if (dims[a] > 1) c = std::min(c, std::fabs(f->g.step[a]));
        const float e = (float)(dims[a] - 1) * std::fabs(f->g.step[a]);
        const float ee = e * e;
        sum = a == 0 ? ee : sum + ee;
    }
    if (!(c < INFINITY)) c = 1.f;
    *p = mon_trace_params{ 0.f, std::sqrt(sum), c / 8.f, c / 4.f, 0.5f, c / 2.f, 256 };
    return MON_OK;
}
// The device side of both calls, on the locked handle: the rays, then the poses, uploaded; the march's arguments but for its outputs
static int trace_upload(FieldCall& c, const float* rays, size_t n, const float* poses16, size_t H, size_t at_pose, const mon_trace_params* p,
                        FieldTraceArgs& a) {
    DistField& f = *c.f;
    HIPCHECK(hipMemcpyAsync(f.in.p, rays, 24 * n, hipMemcpyHostToDevice, f.s));
    if (poses16) HIPCHECK(hipMemcpyAsync(f.in.p + at_pose, poses16, 64 * H, hipMemcpyHostToDevice, f.s));
    a = FieldTraceArgs{};
    a.rays = f.in.p; a.poses = poses16 ? f.in.p + at_pose : nullptr; a.n = (uint32_t)n; a.n_pose = (uint32_t)H;
    a.t_min = p->t_min; a.t_max = p->t_max; a.eps = p->eps; a.step_min = p->step_min; a.relax = p->relax; a.step_outside = p->step_outside;
    a.max_steps = (uint32_t)p->max_steps;
    return MON_OK;
}
// out: range | status | steps | normal ([H][n] each, the normal three floats per ray), those asked for
int dist_field_trace(DistField* field, const float* rays, size_t n, const float* poses16, size_t H, const mon_trace_params* p, float* range, int32_t* status,
                     int32_t* steps, float* normal3) {
    const char* what = "dist_field_trace";
    REQUIRE_ARG(what, rays, "rays"); REQUIRE_ARG(what, p, "params"); REQUIRE_ARG(what, range, "range");
    { const int rc = trace_check(what, n, poses16, H, kTraceMaxHome, p); if (rc) return rc; }
    FieldCall c; { const int rc = c.enter(what, field); if (rc) return rc; }
    DistField& f = *c.f;
    const size_t m = n * H, at_pose = round4(6 * n);
    Area A; const size_t r_range = A.piece(range, m), r_status = A.piece(status, status ? m : 0), r_steps = A.piece(steps, steps ? m : 0);
    const size_t r_normal = A.piece(normal3, normal3 ? 3 * m : 0);
    { const int rc = c.room(at_pose + 16 * H, A.end, A.end); if (rc) return rc; }
    FieldTraceArgs a;
    { const int rc = trace_upload(c, rays, n, poses16, H, at_pose, p, a); if (rc) return rc; }
    float* o = f.out.p;
    a.stride = (uint32_t)n; a.range = o + r_range; a.status = status ? reinterpret_cast<int32_t*>(o + r_status) : nullptr;
    a.steps = steps ? reinterpret_cast<int32_t*>(o + r_steps) : nullptr; a.normal = normal3 ? o + r_normal : nullptr;
    launch_field_trace(f.s, f.cells, f.g, a);
    { const int rc = c.home(f.out.p, A.end); if (rc) return rc; }
    A.unpack(f.h_out.p, nullptr);
    return MON_OK;
}
// in: rays | measured | poses.  out: range | status ([H][stride] each, stride = n rounded up to a multiple of 4) | the fold's scratch | rows [H][4]; only
// the rows come home
int dist_field_beam_score(DistField* field, const float* rays, size_t n, const float* measured, const float* poses16, size_t H, const mon_trace_params* p,
                          const mon_beam_params* b, float* cost, int32_t* n_valid, int32_t* n_hit) {
    const char* what = "dist_field_beam_score";
    REQUIRE_ARG(what, rays, "rays"); REQUIRE_ARG(what, measured, "measured"); REQUIRE_ARG(what, p, "params"); REQUIRE_ARG(what, b, "beam");
    REQUIRE_ARG(what, cost, "cost");
    { const int rc = trace_check(what, n, poses16, H, kTraceMaxBeams, p); if (rc) return rc; }
    if (!(b->huber > 0.f)) { set_error("%s: huber %g (above 0; +inf is allowed)", what, (double)b->huber); return MON_ERR_ARG; }
    FieldCall c; { const int rc = c.enter(what, field); if (rc) return rc; }
    DistField& f = *c.f;
    const size_t stride = round4(n), at_meas = round4(6 * n), at_pose = at_meas + stride;
    const size_t r_status = H * stride, r_part = 2 * r_status, r_rows = r_part + round4(beam_score_scratch((uint32_t)n, (uint32_t)H));
    { const int rc = c.room(at_pose + 16 * H, r_rows + kScanMatchLite * H, kScanMatchLite * H); if (rc) return rc; }
    FieldTraceArgs a;
    { const int rc = trace_upload(c, rays, n, poses16, H, at_pose, p, a); if (rc) return rc; }
    HIPCHECK(hipMemcpyAsync(f.in.p + at_meas, measured, 4 * n, hipMemcpyHostToDevice, f.s));
    float* o = f.out.p;
    a.stride = (uint32_t)stride; a.range = o; a.status = reinterpret_cast<int32_t*>(o + r_status);
    launch_field_trace(f.s, f.cells, f.g, a);
    launch_beam_score(f.s, a.range, a.status, f.in.p + at_meas, (uint32_t)n, (uint32_t)H, (uint32_t)stride, b->huber, o + r_part, o + r_rows);
    { const int rc = c.home(o + r_rows, kScanMatchLite * H); if (rc) return rc; }
    rows_unpack(f.h_out.p, H, kScanMatchLite, 0, cost, n_valid, n_hit);
    return MON_OK;
}

}  // namespace mon
