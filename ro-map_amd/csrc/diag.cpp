// diag.cpp -- libmon_core_diag.so: diagnostics and test scaffolding (include/mon_core_diag.h).  Links against libmon_core.so and reads its objects
// through the internal headers; nothing here is on the product path.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "model.h"
#include "frag_layout.h"
#include "../../include/mon_core_diag.h"

namespace mon {
int selftest_mfma(int device, const uint16_t* A, const uint16_t* B, float* D);
bool read_yaml_number(const std::string& text, const char* key, double& v);

#define HIPCHECK(expr)                                                                                         \
    do { hipError_t _e = (expr); if (_e != hipSuccess) {                                                       \
        set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); return MON_ERR_HIP; } } while (0)

int model_debug_read(Model& m, int which, void* dst, size_t bytes) {
    model_leave_lane(m);
    if (which == MON_BUF_EMA) { int rc = ensure_ema_current(m); if (rc) return rc; }
    const size_t R = m.oc.R, B = R * m.oc.S, n = m.n_params; const void* src = nullptr; size_t sz = 0;
    // optimizer state kept as chunk records
    if (m.P.rec && (which == MON_BUF_MASTER || which == MON_BUF_M1 || which == MON_BUF_M2 || which == MON_BUF_STEPS)) {
        if (!dst || bytes < n * 4) { set_error("debug_read: buffer too small"); return MON_ERR_ARG; }
        HIPCHECK(use_device(m.device)); void* tmp = nullptr; HIPCHECK(hipMalloc(&tmp, n * 4));
        launch_state_unpack(m.train_stream, m.P.rec, which == MON_BUF_MASTER ? 0 : which == MON_BUF_M1 ? 1 : which == MON_BUF_M2 ? 2 : 3, tmp, (uint32_t)n);
        hipError_t e = hipStreamSynchronize(m.train_stream); if (e == hipSuccess) e = hipMemcpy(dst, tmp, n * 4, hipMemcpyDeviceToHost);
        (void)hipFree(tmp); HIPCHECK(e); return MON_OK;
    }
    switch (which) {
        case MON_BUF_MASTER: src = m.P.master; sz = n * 4; break;       case MON_BUF_HALF: src = m.P.half; sz = n * 2; break;
        case MON_BUF_EMA: src = m.P.ema; sz = n * 2; break;             case MON_BUF_M1: src = m.P.m1; sz = n * 4; break;
        // (16-bit counters are widened below)
        case MON_BUF_M2: src = m.P.m2; sz = n * 4; break;
        case MON_BUF_STEPS: src = m.P.steps ? (const void*)m.P.steps : (const void*)m.P.steps16; sz = n * 4; break;
        case MON_BUF_GMLP: src = m.P.gmlp; sz = (size_t)m.nd.n_mlp * 4; break;
        case MON_BUF_GGRID_H: src = m.P.ggrid; sz = (size_t)m.n_grid * 2; break;
        case MON_BUF_GGRID_F32: src = m.P.ggrid; sz = (size_t)m.n_grid * 4; break;
        case MON_BUF_PTS: src = m.B.pts; sz = B * 12; break;            case MON_BUF_TDIST: src = m.B.tdist; sz = B * 4; break;
        case MON_BUF_E: src = m.B.E; sz = B * m.nd.Epad * 2; break;     case MON_BUF_HID: src = m.B.Hid; sz = B * m.nd.W * m.nd.NH * 2; break;
        case MON_BUF_O: src = m.B.O; sz = B * 8; break;                 case MON_BUF_DO: src = m.B.dO; sz = B * 8; break;
        case MON_BUF_DHID: src = m.B.dHid; sz = B * m.nd.W * m.nd.NH * 2; break;
        case MON_BUF_DE: src = m.B.dE; sz = B * m.nd.Epad * 2; break;
        case MON_BUF_RGB_RAY: src = m.B.rgb_ray; sz = R * 12; break;    case MON_BUF_DEPTH_RAY: src = m.B.depth_ray; sz = R * 4; break;
        case MON_BUF_MASK_RAY: src = m.B.mask_ray; sz = R * 4; break;   case MON_BUF_LOSS_RAY: src = m.B.loss_ray; sz = R * 4; break;
        case MON_BUF_RAY_O: src = m.B.ray_o; sz = R * 12; break;        case MON_BUF_RAY_D: src = m.B.ray_d; sz = R * 12; break;
        case MON_BUF_RAY_T0: src = m.B.ray_t0; sz = R * 4; break;       case MON_BUF_RAY_T1: src = m.B.ray_t1; sz = R * 4; break;
        case MON_BUF_TARGET: src = m.B.target; sz = R * 12; break;      case MON_BUF_TARGET_DEPTH: src = m.B.target_depth; sz = R * 4; break;
        case MON_BUF_BGCOL: src = m.B.bgcol; sz = R * 12; break;        case MON_BUF_RAY_FLAG: src = m.B.ray_flag; sz = R; break;
        case MON_BUF_RAY_DN: src = m.B.ray_dn; sz = R * 4; break;       case MON_BUF_MASK: src = m.B.mask; sz = (R / 64) * 8; break;
        case MON_BUF_STATE: src = m.d_state; sz = sizeof(DevState); break;
        case MON_BUF_FRAG_TRAIN: src = m.d_frag_train; sz = 64 * 512 * 2; break;
        case MON_BUF_X_ALL: if (!m.d_x_all) { set_error("debug_read: level-tile encode not in use"); return MON_ERR_STATE; } src = m.d_x_all; sz = B * 16;
        break;
        case MON_BUF_E_SOA: if (!m.d_e_soa) { set_error("debug_read: level-tile encode not in use"); return MON_ERR_STATE; } src = m.d_e_soa;
        sz = B * (size_t)m.nd.L * 4; break;
        case MON_BUF_HALF_TILES: if (!m.d_half_tiles) { set_error("debug_read: level-tile encode not in use"); return MON_ERR_STATE; } src = m.d_half_tiles;
        sz = (size_t)m.n_grid * 2; break;
        case MON_BUF_LIVE_CNT: if (!m.d_live_cnt) { set_error("debug_read: no live-sample lists (occupancy_skip off, or not on the level tiles)"); return MON_ERR_STATE; }
            src = m.d_live_cnt; sz = 2u * kLiveMaxParts * kLiveCntStride * 4u; break;
        case MON_BUF_FRAG_REF:
            if (!m.d_frag_render) { set_error("debug_read: fused backend not available"); return MON_ERR_STATE; }
            HIPCHECK(use_device(m.device)); HIPCHECK(hipMemsetAsync(m.d_frag_render, 0, 64 * 512 * 2, m.train_stream));
            launch_build_frag_image(m.train_stream, m.P.half, m.nd, m.d_frag_render); src = m.d_frag_render; sz = 64 * 512 * 2; break;
        default: set_error("debug_read: unknown buffer id %d", which); return MON_ERR_ARG;
    }
    if (!dst || bytes < sz) { set_error("debug_read: buffer too small (%zu < %zu)", bytes, sz); return MON_ERR_ARG; }
    HIPCHECK(use_device(m.device)); HIPCHECK(hipStreamSynchronize(m.train_stream));
    // saturating 16-bit counters on the device (ParamPtrs::steps16): hand out uint32 like before
    if (which == MON_BUF_STEPS && !m.P.steps) {
        std::vector<uint16_t> h16(n); HIPCHECK(hipMemcpy(h16.data(), src, n * 2, hipMemcpyDeviceToHost));
        uint32_t* out = reinterpret_cast<uint32_t*>(dst); for (size_t i = 0; i < n; ++i) out[i] = h16[i];
        return MON_OK;
    }
    // the grid gradient as k_optimizer forms it: the fp16 gradient table (large levels: binned sums or tcnn's atomics) plus the fp16 partial tables of the
    // LDS-scattered levels, summed in fp32 in the kernel's order -- pairs of partitions, (a + b) added to the running sum (update_chunk, kernels_optim.hip)
    if (which == MON_BUF_GGRID_H || which == MON_BUF_GGRID_F32) {
        std::vector<uint16_t> tab(m.n_grid); HIPCHECK(hipMemcpy(tab.data(), m.P.ggrid, (size_t)m.n_grid * 2, hipMemcpyDeviceToHost));
        std::vector<float> acc(m.n_grid);
        for (uint32_t i = 0; i < m.n_grid; ++i) { _Float16 h; std::memcpy(&h, &tab[i], 2); acc[i] = (float)h; }
        // whole steps of the shapes outside the fused kernels keep their partial tables too (hybrid_scatter); the dense optimizer then never reads the table
        const bool parts = (m.backend == 1 && m.plan.lds_mask) || (m.backend == 0 && m.plan.hybrid_scatter && which == MON_BUF_GGRID_F32);
        if (parts) {
            // partial tables are planar: [partition][feature][parity][entry / 2], over the LDS-scattered levels' entries
            const uint32_t n_ent = m.part_halves / 2, n_half = n_ent / 2;
            std::vector<uint16_t> pa(m.part_halves), pb(m.part_halves);
            auto val = [&](const std::vector<uint16_t>& part, uint32_t e, uint32_t f) { _Float16 h;
                std::memcpy(&h, &part[((size_t)f * 2 + (e & 1u)) * n_half + (e >> 1)], 2); return (float)h; };
            for (uint32_t q = 0; q < m.scatter.max_P; q += 2) {
                HIPCHECK(hipMemcpy(pa.data(), m.d_gpart + (size_t)q * m.part_halves, (size_t)m.part_halves * 2, hipMemcpyDeviceToHost));
                if (q + 1 < m.scatter.max_P) HIPCHECK(hipMemcpy(pb.data(), m.d_gpart + (size_t)(q + 1) * m.part_halves, (size_t)m.part_halves * 2,
                        hipMemcpyDeviceToHost));
                for (int l = 0; l < m.nd.L; ++l) {
                    // (a level with fewer partial tables: the rest of the buffer is not its data)
                    const bool lds_level = m.backend == 1 ? ((m.plan.lds_mask >> l) & 1u) != 0u : true;
                    if (q >= m.scatter.P[l] || !lds_level) continue;
                    const bool two = q + 1 < m.scatter.P[l];
                    for (uint32_t e = m.lt.offset[l]; e < m.lt.offset[l + 1]; ++e) for (uint32_t f = 0; f < 2; ++f)
                        acc[2 * e + f] += two ? val(pa, e, f) + val(pb, e, f) : val(pa, e, f);
                }
            }
        }
        if (which == MON_BUF_GGRID_F32) {
            if (!dst || bytes < (size_t)m.n_grid * 4) { set_error("debug_read: buffer too small"); return MON_ERR_ARG; }
            std::memcpy(dst, acc.data(), (size_t)m.n_grid * 4); return MON_OK;
        }
        uint16_t* out = reinterpret_cast<uint16_t*>(dst);
        for (uint32_t i = 0; i < m.n_grid; ++i) { const _Float16 h = (_Float16)acc[i]; std::memcpy(&out[i], &h, 2); }
        return MON_OK;
    }
    HIPCHECK(hipMemcpy(dst, src, sz, hipMemcpyDeviceToHost));
    return MON_OK;
}


}  // namespace mon

using namespace mon;
#define REQUIRE(p, what) do { if (!(p)) { set_error("%s: null %s", __func__, what); return MON_ERR_ARG; } } while (0)

extern "C" {
int mon_object_debug_read(mon_object* o, int which, void* dst, size_t bytes) { REQUIRE(o, "object"); return model_debug_read(*o->m, which, dst, bytes); }
int mon_dataset_debug_read(mon_dataset* ds, uint32_t frame, uint32_t* rgba, float* depth, float* pose16) {
    REQUIRE(ds, "dataset"); Dataset& d = *ds->d;
    if (frame >= d.max_frames) { set_error("dataset_debug_read: frame %u >= capacity %u", frame, d.max_frames); return MON_ERR_ARG; }
    const size_t px = (size_t)d.K.H * d.K.W;
    HIPCHECK(use_device(d.device)); HIPCHECK(hipDeviceSynchronize());
    if (rgba) HIPCHECK(hipMemcpy(rgba, d.d_rgba + px * frame, px * 4, hipMemcpyDeviceToHost));
    if (depth && d.d_depth) HIPCHECK(hipMemcpy(depth, d.d_depth + px * frame, px * 4, hipMemcpyDeviceToHost));
    if (pose16) HIPCHECK(hipMemcpy(pose16, d.d_poses + 16 * (size_t)frame, 64, hipMemcpyDeviceToHost));
    return MON_OK;
}
int mon_microbench(int device, int mode, int pattern, uint32_t n_entries, uint32_t n_ops, float* ms) { REQUIRE(ms, "ms");
    return microbench(device, mode, pattern, n_entries, n_ops, ms); }
int mon_debug_fast_index(const mon_config* cfg, int level, uint32_t x, uint32_t y, uint32_t z, uint32_t* index, uint32_t* size) {
    REQUIRE(cfg, "cfg"); REQUIRE(index, "index"); REQUIRE(size, "size");
    LevelTable lt{}; NetDims nd{}; uint32_t n_grid = 0; int rc = level_table_build(*cfg, lt, nd, n_grid); if (rc) return rc;
    if (level < 0 || level >= nd.L) { set_error("level out of range"); return MON_ERR_ARG; }
    LevelFast lf{}; level_fast_build(lt, nd, lf);
    *index = fast_grid_index(lf, level, x, y, z); *size = lf.size[level]; return MON_OK;
}
int mon_debug_frag_layout(int epad, int W, int NH, int L, int* source, int* slots, int* n_image, int* n_mlp) {
    if (!(epad == 16 || epad == 32) || !((((W == 32 || W == 64) && (NH == 1 || NH == 2)) || (W == 128 && NH == 1))) || L < 1 || 2 * L > epad) { set_error("frag_layout: unsupported shape");
        return MON_ERR_ARG; }
    const FragDims d{ epad, W, NH, L };
    if (n_image) *n_image = d.N_FRAGS() * 512;
    if (n_mlp) *n_mlp = d.N_MLP();
    if (source) for (int i = 0; i < d.N_FRAGS() * 512; ++i) source[i] = frag_source(d, i);
    if (slots) for (int p = 0; p < d.N_MLP(); ++p) { int o[2] = { -1, -1 }; const int n = frag_slots(d, p, o); slots[2 * p] = n > 0 ? o[0] : -1;
        slots[2 * p + 1] = n > 1 ? o[1] : -1; }
    return MON_OK;
}
int mon_debug_acc_layout(int epad, int W, int NH, int L, int* param, int* n_cols) {
    if (!(epad == 16 || epad == 32) || !((((W == 32 || W == 64) && (NH == 1 || NH == 2)) || (W == 128 && NH == 1))) || L < 1 || 2 * L > epad) { set_error("acc_layout: unsupported shape");
        return MON_ERR_ARG; }
    const FragDims d{ epad, W, NH, L };
    if (n_cols) *n_cols = acc_cols(d);
    if (param) for (int i = 0; i < acc_cols(d); ++i) param[i] = acc_param(d, i);
    return MON_OK;
}
int mon_selftest_mfma(int device, const uint16_t* A, const uint16_t* B, float* D) { REQUIRE(A, "A"); REQUIRE(B, "B"); REQUIRE(D, "D");
    return selftest_mfma(device, A, B, D); }
int mon_debug_checkpoint_timing(int enable, double* kernel_ms) { return mon::checkpoint_timing(enable, kernel_ms); }
int mon_debug_occupancy_state(mon_object* o, uint32_t out[2]) {
    if (!o || !o->m || !out) { mon::set_error("debug_occupancy_state: null argument"); return MON_ERR_ARG; }
    out[0] = o->m->occ_refreshed_iter; out[1] = o->m->occ_next_refresh; return MON_OK;
}
int mon_debug_occupancy_grid(mon_object* o, uint32_t* raw, uint32_t* dilated, float* raw_threshold, uint32_t* n_parts) {
    if (!o || !o->m) { mon::set_error("debug_occupancy_grid: null object"); return MON_ERR_ARG; }
    mon::Model& m = *o->m;
    if (!m.d_occ) { mon::set_error("debug_occupancy_grid: the object has no occupancy grid"); return MON_ERR_STATE; }
    mon::model_leave_lane(m);
    HIPCHECK(mon::use_device(m.device)); HIPCHECK(hipStreamSynchronize(m.train_stream));
    constexpr size_t bytes = (size_t)mon::kOccWords * 4;
    // (nothing has written the raw grid before the first refresh or pin: the grid in use is the warm-up's all-ones one)
    if (raw) HIPCHECK(hipMemcpy(raw, m.occ_refreshed_iter ? m.d_occ_tmp : m.d_occ, bytes, hipMemcpyDeviceToHost));
    if (dilated) HIPCHECK(hipMemcpy(dilated, m.d_occ, bytes, hipMemcpyDeviceToHost));
    if (raw_threshold) *raw_threshold = m.occ_raw_threshold;
    if (n_parts) { const uint32_t B = m.oc.R * m.oc.S, spw = mon::encode_tiles_spw(B); *n_parts = m.d_live_idx ? (B + spw - 1u) / spw : 0u; }
    return MON_OK;
}
int mon_debug_set_train_occupancy(mon_object* o, const uint32_t* bits) {
    if (!o || !o->m) { mon::set_error("debug_set_train_occupancy: null object"); return MON_ERR_ARG; }
    mon::Model& m = *o->m;
    if (!m.d_occ) { mon::set_error("debug_set_train_occupancy: the object has no occupancy grid"); return MON_ERR_STATE; }
    mon::model_leave_lane(m);
    HIPCHECK(mon::use_device(m.device)); HIPCHECK(hipStreamSynchronize(m.train_stream));
    constexpr size_t bytes = (size_t)mon::kOccWords * 4;
    if (bits) {
        HIPCHECK(hipMemcpy(m.d_occ, bits, bytes, hipMemcpyHostToDevice)); HIPCHECK(hipMemcpy(m.d_occ_tmp, bits, bytes, hipMemcpyHostToDevice));
        m.occ_pinned = true; if (!m.occ_refreshed_iter) m.occ_refreshed_iter = m.h_state.iter > 1u ? m.h_state.iter : 1u;      // in use from now on
    } else if (m.occ_pinned) {
        m.occ_pinned = false;
        if (m.h_state.iter < (uint32_t)mon::kOccWarmup) { HIPCHECK(hipMemset(m.d_occ, 0xff, bytes)); m.occ_refreshed_iter = 0; }
        m.occ_next_refresh = 0;                              // (after the warm-up: due at the next iteration)
    }
    mon::model_mark_stale(m, mon::kStaleOccupancy);          // the positions sampled ahead carry the old grid's live bits and lists, as after a refresh
    return MON_OK;
}
int mon_debug_render_jobs(mon_object* o, int side, uint32_t* jobs) {
    if (!o || !o->m || !jobs) { mon::set_error("debug_render_jobs: null argument"); return MON_ERR_ARG; }
    if (!o->m->plan.tile_render) { mon::set_error("debug_render_jobs: this object does not render on level tiles"); return MON_ERR_STATE; }
    mon::TileWs* ws = nullptr; const int rc = mon::tile_ws_get(*o->m, side, 0, &ws); if (rc) return rc;
    std::lock_guard<std::mutex> l(ws->mu);
    if (!ws->counters) { mon::set_error("debug_render_jobs: no tile workspace on the object's device"); return MON_ERR_STATE; }
    if (mon::use_device(o->m->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { mon::set_error("debug_render_jobs: device error");
        return MON_ERR_HIP; }
    if (hipMemcpy(jobs, ws->counters + 16u * ((ws->flip + 1u) & 1u), 4, hipMemcpyDeviceToHost) != hipSuccess) {
        mon::set_error("debug_render_jobs: copy failed"); return MON_ERR_HIP; }
    return MON_OK;
}
int mon_debug_set_render_grid(mon_object* o, int side, const uint32_t* bits) { REQUIRE(o, "object");
    return mon::model_debug_set_render_grid(*o->m, side, bits); }
int mon_debug_scene_samples(mon_object* const* objs, size_t n_objs, int side, mon_frame_bbox rect, const float* Twc16, size_t k, float* t, float* alpha,
                            float* rgb, uint32_t* count) {
    std::vector<mon::Model*> ms; int rc;                                   // (the image and the depth are this call's own, made once the rect is known to be good)
    if ((rc = mon::scene_render_check(side, rect, Twc16)) || (rc = mon::scene_models("scene_render", objs, n_objs, ms)) ||
        (rc = mon::scene_objects_check("scene_render", ms.data(), n_objs))) return rc;
    if (k >= n_objs) { set_error("debug_scene_samples: k out of range"); return MON_ERR_ARG; }
    const size_t px = (size_t)rect.w * rect.h; std::vector<float> img(3 * px), dep(px);
    const mon::SceneDump dump{ (uint32_t)k, t, alpha, rgb, count };
    return mon::scene_render(ms.data(), n_objs, side, rect, Twc16, img.data(), dep.data(), nullptr, nullptr, nullptr, &dump);
}
// mon_debug_scene_composite; with the hit outputs mon_debug_scene_probe_composite (the probe's kernel on the same lists); with an entry array
// [n_lists][n_rays] in place of dn, the threshold and a third hit output mon_debug_scene_cast_composite (the cast's kernel).  aux = dn or entry.
enum DebugComposite { kDebugRender = 0, kDebugProbe = 1, kDebugCast = 2 };
static int debug_scene_composite(DebugComposite kind, int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb,
                                 const uint32_t* count, const float* aux, float thr, float* out_rgb, float* out_depth, float* out_opacity,
                                 int32_t* out_instance, float* out_hit_a, float* out_hit_b, int32_t* out_hit_instance) {
    REQUIRE(t, "t"); REQUIRE(alpha, "alpha"); REQUIRE(rgb, "rgb"); REQUIRE(count, "count"); REQUIRE(aux, kind == kDebugCast ? "entry" : "dn");
    REQUIRE(out_rgb, "out_rgb"); REQUIRE(out_depth, "out_depth"); REQUIRE(out_opacity, "out_opacity"); REQUIRE(out_instance, "out_instance");
    if (n_rays == 0 || n_lists == 0 || n_lists > mon::kSceneMaxLists) { set_error("debug_scene_composite: %u rays, %u lists", n_rays, n_lists);
        return MON_ERR_ARG; }
    if (kind == kDebugCast && !(thr > 0.f && thr <= 0.999f)) { set_error("debug_scene_cast_composite: hit_opacity %g", (double)thr); return MON_ERR_ARG; }
    const size_t nl = (size_t)n_lists * n_rays, ns = nl * mon::kSceneListLen, R = n_rays, rows = kind == kDebugCast ? 9 : kind == kDebugProbe ? 8 : 6;
    for (size_t i = 0; i < nl; ++i) if (count[i] > mon::kSceneListLen) { set_error("debug_scene_composite: count %u > 64", count[i]); return MON_ERR_ARG; }
    std::vector<float> attr(4 * ns);
    for (size_t i = 0; i < ns; ++i) { attr[4 * i] = alpha[i]; attr[4 * i + 1] = rgb[3 * i]; attr[4 * i + 2] = rgb[3 * i + 1]; attr[4 * i + 3] = rgb[3 * i + 2]; }
    HIPCHECK(mon::use_device(device));
    char* d = nullptr; const size_t b_t = ns * 4, b_a = ns * 16, b_c = nl * 4, b_aux = (kind == kDebugCast ? nl : R) * 4, b_out = R * 4 * rows;
    HIPCHECK(hipMalloc((void**)&d, b_t + b_a + b_c + b_aux + b_out));
    float* d_t = (float*)d; float* d_a = (float*)(d + b_t); uint32_t* d_c = (uint32_t*)(d + b_t + b_a); float* d_aux = (float*)(d + b_t + b_a + b_c);
    float* d_out = (float*)(d + b_t + b_a + b_c + b_aux);
    hipError_t e = hipMemcpy(d_t, t, b_t, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_a, attr.data(), b_a, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_c, count, b_c, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_aux, aux, b_aux, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        int32_t* d_inst = reinterpret_cast<int32_t*>(d_out + 5 * R);
        if (kind == kDebugCast) mon::launch_scene_cast_composite(nullptr, n_rays, n_lists, n_rays, thr, d_t, d_a, d_c, d_aux, d_out, d_out + 3 * R, d_out + 4 * R,
                d_inst, d_out + 6 * R, d_out + 7 * R, reinterpret_cast<int32_t*>(d_out + 8 * R));
        else if (kind == kDebugProbe) mon::launch_scene_probe_composite(nullptr, n_rays, n_lists, n_rays, d_t, d_a, d_c, d_aux, d_out, d_out + 3 * R, d_out + 4 * R,
                d_inst, d_out + 6 * R, reinterpret_cast<int32_t*>(d_out + 7 * R));
        else mon::launch_scene_composite(nullptr, n_rays, n_lists, n_rays, d_t, d_a, d_c, d_aux, d_out, d_out + 3 * R, d_out + 4 * R, d_inst);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<float> out(rows * R);
    if (e == hipSuccess) e = hipMemcpy(out.data(), d_out, b_out, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHECK(e);
    std::memcpy(out_rgb, out.data(), 12 * R); std::memcpy(out_depth, out.data() + 3 * R, 4 * R);
    std::memcpy(out_opacity, out.data() + 4 * R, 4 * R); std::memcpy(out_instance, out.data() + 5 * R, 4 * R);
    if (kind != kDebugRender) { std::memcpy(out_hit_a, out.data() + 6 * R, 4 * R); std::memcpy(out_hit_instance, out.data() + (rows - 1) * R, 4 * R); }
    if (kind == kDebugCast) std::memcpy(out_hit_b, out.data() + 7 * R, 4 * R);
    return MON_OK;
}
int mon_debug_scene_composite(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                              const float* dn, float* out_rgb, float* out_depth, float* out_opacity, int32_t* out_instance) {
    return debug_scene_composite(kDebugRender, device, n_rays, n_lists, t, alpha, rgb, count, dn, 0.5f, out_rgb, out_depth, out_opacity, out_instance, nullptr,
                                 nullptr, nullptr);
}
int mon_debug_scene_probe_composite(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                                    const float* dn, float* out_rgb, float* out_depth, float* out_opacity, int32_t* out_instance, float* out_hit_depth,
                                    int32_t* out_hit_instance) {
    REQUIRE(out_hit_depth, "out_hit_depth"); REQUIRE(out_hit_instance, "out_hit_instance");
    return debug_scene_composite(kDebugProbe, device, n_rays, n_lists, t, alpha, rgb, count, dn, 0.5f, out_rgb, out_depth, out_opacity, out_instance,
                                 out_hit_depth, nullptr, out_hit_instance);
}
int mon_debug_scene_cast_composite(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                                   const float* entry, float hit_opacity, float* out_rgb, float* out_dist, float* out_opacity, int32_t* out_instance,
                                   float* out_hit_t, float* out_hit_sample_t, int32_t* out_hit_instance) {
    REQUIRE(out_hit_t, "out_hit_t"); REQUIRE(out_hit_sample_t, "out_hit_sample_t"); REQUIRE(out_hit_instance, "out_hit_instance");
    return debug_scene_composite(kDebugCast, device, n_rays, n_lists, t, alpha, rgb, count, entry, hit_opacity, out_rgb, out_dist, out_opacity, out_instance,
                                 out_hit_t, out_hit_sample_t, out_hit_instance);
}
int mon_debug_scene_probe_rays(mon_object* const* objs, size_t n_objs, int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                               size_t k, float* rows) {
    REQUIRE(rows, "rows");
    std::vector<mon::Model*> ms; int rc;
    if ((rc = mon::scene_probe_check(side, Twc16s, n_poses, q, n_q, rows, rows)) || (rc = mon::scene_models("scene_probe", objs, n_objs, ms)) ||
        (rc = mon::scene_objects_check("scene_probe", ms.data(), n_objs))) return rc;
    if (k >= n_objs) { set_error("debug_scene_probe_rays: k out of range"); return MON_ERR_ARG; }
    std::vector<float> img(3 * n_q), dep(n_q);
    const mon::SceneRaysDump dump{ (uint32_t)k, rows, nullptr };
    return mon::scene_probe(ms.data(), n_objs, side, Twc16s, n_poses, q, n_q, img.data(), dep.data(), nullptr, nullptr, nullptr, nullptr, nullptr, &dump);
}
int mon_debug_scene_cast_rays(mon_object* const* objs, size_t n_objs, int side, const mon_scene_ray* rays, size_t n_rays, size_t k, float* rows, float* entry) {
    REQUIRE(rows, "rows"); REQUIRE(entry, "entry");
    std::vector<mon::Model*> ms; int rc;
    if ((rc = mon::scene_cast_check(side, rays, n_rays, 0.5f, rows, rows)) || (rc = mon::scene_models("scene_cast", objs, n_objs, ms)) ||
        (rc = mon::scene_objects_check("scene_cast", ms.data(), n_objs, false))) return rc;
    if (k >= n_objs) { set_error("debug_scene_cast_rays: k out of range"); return MON_ERR_ARG; }
    std::vector<float> img(3 * n_rays), dep(n_rays);
    const mon::SceneRaysDump dump{ (uint32_t)k, rows, entry };
    return mon::scene_cast(ms.data(), n_objs, side, rays, n_rays, 0.5f, img.data(), dep.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &dump);
}
int mon_debug_scene_point_rows(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, size_t k, float* rows) {
    REQUIRE(rows, "rows");
    std::vector<mon::Model*> ms; int rc;
    if ((rc = mon::scene_points_check(side, world_xyz, n, rows)) || (rc = mon::scene_models("scene_points", objs, n_objs, ms)) ||
        (rc = mon::scene_objects_check("scene_points", ms.data(), n_objs, false))) return rc;
    if (k >= n_objs) { set_error("debug_scene_point_rows: k out of range"); return MON_ERR_ARG; }
    const mon::ScenePoints q = mon::scene_point_list(world_xyz, n);
    return mon::scene_points(ms.data(), n_objs, side, q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, k, rows);
}
int mon_debug_scene_gradient_rows(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, const float* level_weights, size_t k,
                                  float* rows) {
    REQUIRE(rows, "rows");
    std::vector<mon::Model*> ms; int rc;
    if ((rc = mon::scene_gradients_check(side, world_xyz, n, level_weights, nullptr, n_objs, rows, rows)) ||
        (rc = mon::scene_models("scene_gradients", objs, n_objs, ms)) || (rc = mon::scene_objects_check("scene_gradients", ms.data(), n_objs, false)) ||
        (rc = mon::scene_gradients_weights_check(ms.data(), n_objs, level_weights))) return rc;
    if (k >= n_objs) { set_error("debug_scene_gradient_rows: k out of range"); return MON_ERR_ARG; }
    const mon::ScenePoints q = mon::scene_point_list(world_xyz, n);
    return mon::scene_gradients(ms.data(), n_objs, side, q, level_weights, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                k, rows);
}
int mon_debug_encode_block(uint32_t block, int n_levels, uint32_t* level, uint32_t* part) {
    REQUIRE(level, "level"); REQUIRE(part, "part");
    if (n_levels < 1 || n_levels > kMaxLevels || block >= (uint32_t)n_levels * kEncWgPerLevel) { set_error("encode_block: block %u of %d levels", block, n_levels);
        return MON_ERR_ARG; }
    const EncBlock eb = enc_block_decode(block, (uint32_t)n_levels); *level = eb.level; *part = eb.part; return MON_OK;
}
int mon_debug_paths_stats(uint32_t* out3) { REQUIRE(out3, "out3"); mon::paths_last_stats(out3); return MON_OK; }
int mon_debug_pose_samples(mon_object* o, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p,
                           uint32_t iteration, float* x, float* raw, float* dldx) {
    REQUIRE(o, "object");
    { const int rc = mon::pose_check(side, obs, n_obs, Tow16, p); if (rc) return rc; }
    const mon::PoseDump dump{ x, raw, dldx };
    return mon::pose_refine(*o->m, side, obs, n_obs, Tow16, *p, -1, iteration, nullptr, nullptr, nullptr, nullptr, &dump);
}
int mon_debug_scene_pose_samples(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16,
                                 const mon_pose_refine_params* p, uint32_t iteration, const float* level_weights, size_t k, float* x_o, float* x_c, float* t,
                                 float* raw, float* dldx, uint32_t* count) {
    std::vector<mon::Model*> ms; int rc;
    if ((rc = mon::scene_pose_check(side, obs, n_obs, Twc16, p)) || (rc = mon::scene_models("scene pose", objs, n_objs, ms)) ||
        (rc = mon::scene_pose_objects_check(ms.data(), n_objs, obs, n_obs, p))) return rc;
    if (k >= n_objs) { set_error("debug_scene_pose_samples: k out of range"); return MON_ERR_ARG; }
    const mon::ScenePoseDump dump{ (uint32_t)k, x_o, x_c, t, raw, dldx, count };
    return mon::scene_pose(ms.data(), n_objs, side, obs, n_obs, Twc16, *p, -1, iteration, nullptr, nullptr, nullptr, nullptr, &dump, level_weights);
}
int mon_debug_scene_composite_grad(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                                   const float* cstar, const float* mstar, const float* dstar, const float* dn, float w_rgb, float w_mask, float w_depth,
                                   float huber, float* out_l, float* out_W, float* out_D, float* out_dalpha, float* out_dc) {
    REQUIRE(t, "t"); REQUIRE(alpha, "alpha"); REQUIRE(rgb, "rgb"); REQUIRE(count, "count"); REQUIRE(cstar, "cstar"); REQUIRE(mstar, "mstar");
    REQUIRE(dstar, "dstar"); REQUIRE(dn, "dn"); REQUIRE(out_l, "out_l"); REQUIRE(out_W, "out_W"); REQUIRE(out_D, "out_D"); REQUIRE(out_dalpha, "out_dalpha");
    REQUIRE(out_dc, "out_dc");
    if (n_rays == 0 || n_lists == 0 || n_lists > mon::kSceneMaxLists) { set_error("debug_scene_composite_grad: %u rays, %u lists", n_rays, n_lists);
        return MON_ERR_ARG; }
    const size_t nl = (size_t)n_lists * n_rays, ns = nl * mon::kSceneListLen;
    for (size_t i = 0; i < nl; ++i) if (count[i] > mon::kSceneListLen) { set_error("debug_scene_composite_grad: count %u > 64", count[i]); return MON_ERR_ARG; }
    std::vector<float> attr(4 * ns), ray(12 * (size_t)n_rays, 0.f);
    for (size_t i = 0; i < ns; ++i) { attr[4 * i] = alpha[i]; attr[4 * i + 1] = rgb[3 * i]; attr[4 * i + 2] = rgb[3 * i + 1]; attr[4 * i + 3] = rgb[3 * i + 2]; }
    for (size_t r = 0; r < n_rays; ++r) {
        float M = 0.f; for (uint32_t k = 0; k < n_lists; ++k) M = std::max(M, mstar[(size_t)k * n_rays + r]);
        float* q = ray.data() + 12 * r; q[0] = cstar[3 * r]; q[1] = cstar[3 * r + 1]; q[2] = cstar[3 * r + 2]; q[3] = dstar[r]; q[4] = dn[r]; q[5] = M;
    }
    HIPCHECK(mon::use_device(device));
    const uint32_t n_lp = mon::scene_comp_grad_grid(n_rays);
    const size_t b_t = ns * 4, b_a = ns * 16, b_c = nl * 4, b_m = nl * 4, b_ray = (size_t)n_rays * 48, b_gw = ns * 8, b_grow = (size_t)n_rays * 16,
                 b_lp = (size_t)n_lp * 4, b_W = nl * 4, b_D = (size_t)n_rays * 4;
    const size_t sizes[] = { b_a, b_ray, b_grow, b_gw, b_t, b_c, b_m, b_lp, b_W, b_D };                   // (the 16-byte-aligned ones first)
    size_t off[11] = { 0 }; for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + ((sizes[i] + 15) & ~(size_t)15);
    char* d = nullptr; HIPCHECK(hipMalloc((void**)&d, off[10]));
    float* d_a = (float*)(d + off[0]); float* d_ray = (float*)(d + off[1]); float* d_grow = (float*)(d + off[2]); float* d_gw = (float*)(d + off[3]);
    float* d_t = (float*)(d + off[4]); uint32_t* d_c = (uint32_t*)(d + off[5]); float* d_m = (float*)(d + off[6]); float* d_lp = (float*)(d + off[7]);
    float* d_W = (float*)(d + off[8]); float* d_D = (float*)(d + off[9]);
    hipError_t e = hipMemcpy(d_t, t, b_t, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_a, attr.data(), b_a, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_c, count, b_c, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_m, mstar, b_m, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_ray, ray.data(), b_ray, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_gw, 0, b_gw);
    if (e == hipSuccess) {
        mon::SceneCompGradArgs a{}; a.n_rays = n_rays; a.n_lists = n_lists; a.cap = n_rays; a.t = d_t; a.attr = reinterpret_cast<const float4*>(d_a); a.cnt = d_c;
        a.mstar = d_m; a.ray = reinterpret_cast<const float4*>(d_ray); a.w_rgb = w_rgb; a.w_mask = w_mask; a.w_depth = w_depth; a.huber = huber;
        a.gw = reinterpret_cast<float2*>(d_gw); a.grow = reinterpret_cast<float4*>(d_grow); a.loss_part = d_lp; a.out_W = d_W; a.out_D = d_D;
        mon::launch_scene_composite_grad(nullptr, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<float> gw(2 * ns), grow(4 * (size_t)n_rays);
    if (e == hipSuccess) e = hipMemcpy(gw.data(), d_gw, b_gw, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(grow.data(), d_grow, b_grow, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_W, d_W, b_W, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_D, d_D, b_D, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHECK(e);
    for (size_t r = 0; r < n_rays; ++r) out_l[r] = grow[4 * r + 3];
    for (size_t i = 0; i < ns; ++i) {                                     // dL/dc = w G_rgb, as the objects' backward forms it
        const size_t r = (i / mon::kSceneListLen) % n_rays;
        out_dalpha[i] = gw[2 * i];
        for (int c = 0; c < 3; ++c) out_dc[3 * i + c] = gw[2 * i + 1] * grow[4 * r + c];
    }
    return MON_OK;
}
int mon_debug_yaml_number(const char* text, const char* key, double* value) {
    REQUIRE(text, "text"); REQUIRE(key, "key"); REQUIRE(value, "value");
    if (!read_yaml_number(text, key, *value)) { set_error("config.yaml: %s missing or not a number", key); return MON_ERR_IO; }
    return MON_OK;
}
}
