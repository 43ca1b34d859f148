// model.h -- host-side mirror of nerf::NeRF_Model / nerf::NeRF_Dataset for gfx950.
// Reference: CORE/include/nerf_model.h:92-184, CORE/include/nerf_data.h:19-71.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/mon_core.h"
#include "device_common.h"
#include "frag_layout.h"

namespace mon {

// ---- device-resident per-object state updated by kernels (no host round trips inside an iteration)
struct DevState {
    uint32_t step;       // optimizer steps taken (mnTrainingStep)
    uint32_t iter;       // batches generated (RNG counter); advances even when a batch is skipped
    uint32_t n_valid;    // rays of the current batch inside the 3-D box
    uint32_t n_boxes;    // mnBbox
    float lr;            // Adam learning rate after ExponentialDecay
    float loss_sum;      // sum of per-ray losses of the current batch (SumLoss, nerf_model.cu:1231-1253)
    // level-tile encode: n_valid of THIS iteration as counted by the position pass that ran ahead of it (k_sample_points / k_optimizer's position blocks)
    uint32_t n_valid_pre;
    uint32_t skipped;    // batches skipped because n_valid == 0
    // gradient-carrying samples of the CURRENT iteration (written by k_grid_scatter; the optimizer's last block makes it n_scatter_last, so every kernel of an
    // iteration sees the same previous count)
    uint32_t n_scatter_now;
    float ema_deb_even_old, ema_deb_even_new;   // EMA debias factors of the next EVEN optimizer step (see ema_deb_old)
    uint32_t reserved_bins[13];
    uint32_t n_scatter_last;  // their sum in the last completed iteration (reporting)
    uint32_t n_scatter_total; // running sum over all iterations, modulo 2^32 (reporting: differences over a measurement window)
    // EMA debias factors (1 - d^(t-1), 1 / (1 - d^t)) of the next ODD optimizer step t; step t's kernel reads its pair and one of its threads writes the
    float ema_deb_old, ema_deb_new;
                                      // other pair for step t + 1 at kernel ENTRY (two double-precision pows: at the end of the last block they were ~1 us of
                                      // serial tail per step)
    // fused backend: slot counters of the gradient rows k_fused_train hands to k_grid_scatter -- samples with a non-zero dL/dO, per ray bin (ray & (bins - 1));
    // a wave reserves its slots with one returning atomic per ray.  Counter of bin b at [set * kMaxScatterBins * stride + b * stride]: a 64-byte line each
    // (returning atomics on one line serialise in its L2 channel: 4096 of them on 16 adjacent counters cost 7 us of k_fused_train).  TWO sets, by iteration
    // parity: k_fused_train(i) counts in set i & 1, k_grid_scatter(i) reads it and clears the other one for iteration i + 1.
    uint32_t n_scatter[2 * kMaxScatterBins * kScatterCounterStride];
};

// ---- dataset pointers (HBM layout: one slab per kind, frame-major)
struct DatasetPtrs {
    const uint32_t* rgba;    // [frames][H*W]  r | g<<8 | b<<16 | instance<<24  (4 B/pixel; the reference keeps 13 B/pixel)
    const float* depth;      // [frames][H*W]  metres, or nullptr
    const float* poses;      // [frames][16]   Twc column-major
    Intrinsics K;
};

struct ObjectConst {
    Mat4 Tow; Aabb aabb;
    uint32_t instance_id; uint32_t R; uint32_t S; int use_depth;
    uint64_t sample_seed;
    float loss_scale;
    // "same inputs" mode (mon_config::rng_flags, xorwow.h): per iteration parity the three arrays SampleXY[2R] | RandColors[3R] | RandDt[S R] that
    // k_xorwow_fill wrote for that iteration; nullptr = the counter RNG.  xw_render: RandDt of the crop being rendered (index = sample index within the crop).
    const float* xw[2]; const float* xw_render;
};
// one uniform of training iteration `step`, stream kStreamXY / kStreamColor / kStreamDt (index semantics of the reference's arrays: nerf_model.cu:395-396,
// :760, :553)
__device__ __forceinline__ float batch_rand(const ObjectConst& oc, uint32_t stream, uint32_t step, uint32_t idx) {
    if (oc.xw[0]) return oc.xw[step & 1u][(stream == kStreamXY ? 0u : stream == kStreamColor ? 2u * oc.R : 5u * oc.R) + idx];
    return rand01(oc.sample_seed, stream, step, idx);
}
__device__ __forceinline__ float render_rand(const ObjectConst& oc, uint32_t idx) {
    return oc.xw_render ? oc.xw_render[idx] : rand01(oc.sample_seed, kStreamRender, 0u, idx); }

struct BatchPtrs {
    const mon_frame_bbox* boxes;
    // candidates (un-compacted), R entries
    float *cand_o, *cand_d, *cand_dn, *cand_t0, *cand_t1, *cand_depth; uint32_t* cand_rgba; unsigned long long* mask;
    // training / render rays
    float *ray_o, *ray_d, *ray_dn, *ray_t0, *ray_t1, *target, *target_depth, *bgcol; uint8_t* ray_flag;
    // samples
    float *pts, *tdist;
    // network activations (unfused backend only) -- fp16
    uint16_t *E, *Hid, *O, *dO, *dHid, *dE;
    // per-ray results
    float *rgb_ray, *depth_ray, *mask_ray, *loss_ray;
    // level-tile encode: the compacted batch's ray records, 12 floats per training ray {rgba bits, t0, t1, d[3], o[3], target depth, candidate index bits, 0},
    // written by the position pass (k_sample_points / k_optimizer's position blocks) so that k_fused_train<PRE> needs neither the ballot scan nor the candidate
    // select
    float* ray_rec;
};

// LDS scatter plan: levels handled by k_grid_scatter and their sample-partition counts (partial tables per level)
struct ScatterLevels { uint32_t entry_offset[kMaxLevels + 1]; uint8_t P[kMaxLevels]; uint8_t level[kMaxLevels]; uint32_t n_levels; uint32_t max_P; };

struct ParamPtrs {
    float* master; uint16_t* half; uint16_t* ema; float* m1; float* m2; uint32_t* steps;
    // the per-parameter step counters as SATURATING 16-bit values (steps == nullptr then): exact whenever beta^65535 < 2^-25 for both betas -- the bias
    // correction 1 - beta^t is then exactly 1.0f for every t the counter can no longer tell apart (beta <= 0.99973; base.json: 0.9 / 0.99)
    uint16_t* steps16;
    // large tables (lazy EMA): the optimizer state as ONE 128-byte record per 8-parameter chunk -- master[8] | m1[8] | m2[8] | 8 x uint16 step counters | pad (word 28: the lazy EMA's step, round 5) --
    // instead of the four arrays above (which are null then): late in training a few per cent of the chunks are touched, and a touched chunk among untouched
    // ones is then one full line, not four half-used 64-byte sectors.  nullptr = the arrays (small tables: every chunk is streamed anyway)
    float* rec;
    float* gmlp;        // fp32 dW [n_mlp]
    uint16_t* ggrid;    // fp16 grid gradient [n_grid], accumulated with global_atomic_pk_add_f16
    // fused backend: dense fp16 partial gradient tables from k_grid_scatter (stride in halves); nullptr = unused
    const uint16_t* gpart; uint32_t part_stride;
    ScatterLevels sl;                                               // per-level partial-table counts
    // lazy EMA (large tables; `lazy` set by the launcher's caller): per 8-parameter chunk, the optimizer step its EMA is current for -- in word 28 (the pad) of the
    // chunk's record when `rec` is set (ema_step is nullptr then: nothing may index it), in this array otherwise.  set_params / upload_master leave the steps
    // alone: new weights enter the average from the next step on, chunks that sat steps out catch up with the weights they find (as the arrays always did)
    uint32_t* ema_step; int lazy;
    // lazy EMA + fused backend: one byte per 8-parameter chunk, set by whoever adds into ggrid (k_fused_train's atomics, k_big_accum),
    uint8_t* touched; uint32_t first_flag_chunk;
                                                                    // read and cleared by k_optimizer instead of scanning ggrid; chunks below first_flag_chunk
                                                                    // (MLP, LDS-scattered levels) are always visited
    int all_levels_dense;                                           // every level is LDS-scattered (no global-atomic table in use)
    // level-tile encode: the fp16 grid a second time, in LDS-tile order (tile_slot below), kept current by k_optimizer; nullptr = unused
    uint16_t* half_tiles;
};

// Tile image of the level-tile encode (kernels_encode.hip): a level that fits the CU's LDS whole keeps its entry order; a larger one (two parity tiles)
// stores its even entries first, then its odd ones, so that either tile is one contiguous copy.  Entry e of a level (offset off, size entries) sits at:
constexpr uint32_t kEncWholeMax = 163840u / 4u;                     // entries (half2) of a level that fits in one 160 KB tile
__host__ __device__ inline uint32_t tile_slot(uint32_t off, uint32_t size, uint32_t e_rel) {
    return size <= kEncWholeMax ? off + e_rel : off + (e_rel & 1u) * (size >> 1) + (e_rel >> 1); }
// Workgroup b of a row of k_encode_tiles' grid (16 L workgroups, one row per batch chunk) -> (level, sample partition).  Workgroups are dealt round-robin
// over the chip's 8 XCDs, each with an L2 of its own, so b & 7 labels the workgroups that share one.  With level = b / 16 every label walks two partitions of
// every level and every L2 fetches the whole tile image each step.  For L = 4, 8, 16 a label gets four levels x L / 2 partitions instead (L = 16: labels 2 g and
// 2 g + 1 share levels 4 g .. 4 g + 3, partitions 0..7 and 8..15): an L2 then fetches a quarter of the image and half of the positions.  A permutation of
// [0, 16 L) for every L (other L: the identity); where the workgroups really land only decides the traffic (-DMON_ENC_XCD=0: the identity throughout).
#ifndef MON_ENC_XCD
#define MON_ENC_XCD 1
#endif
constexpr uint32_t kEncWgPerLevel = 16;                             // sample partitions per level and chunk
struct EncBlock { uint32_t level, part; };
__host__ __device__ inline EncBlock enc_block_decode(uint32_t b, uint32_t L) {
#if MON_ENC_XCD
    if (L == 4u || L == 8u || L == 16u) { const uint32_t ppx = L / 2u, per = kEncWgPerLevel / ppx, x = b & 7u, s = b >> 3;
        return EncBlock{ 4u * (x / per) + s / ppx, (x % per) * ppx + s % ppx }; }
#endif
    (void)L; return EncBlock{ b / kEncWgPerLevel, b % kEncWgPerLevel };
}

struct OptimConst {
    float beta1, beta2, epsilon, l2_reg, ema_decay, loss_scale, decay_base, log2_beta1, log2_beta2, log2_decay;
    int decay_start, decay_interval;
    uint32_t n_mlp, n_params;
};

// Occupancy-grid skipping on the level-tile chain (north_star N1; cfg.occupancy_skip): the position pass looks every sample's cell up in the bit grid, leaves
// the ray's 32 live bits in word 11 of its record (k_fused_train<PRE, OCC> takes them from there: both kernels see the grid as the position pass saw it) and
// compacts the LIVE samples of each of k_encode_tiles' sample partitions into an index list, so that the encode walks the live samples only.
//   idx [B]: partition w's list at [w * spw, w * spw + count_w), in arrival order (irrelevant: a sample's features go to its own slot).  WHICH list a sample
//     is on is free for the same reason: position block b (256 consecutive samples) appends to list b mod n_parts, so the lists come out equally long
//     whatever part of the batch is live (by sample range the longest list of the bench scene's late batches had 2355 entries against a mean of 2010: three
//     rounds of the encode's 1024 threads instead of two)
//   cnt [2][kLiveMaxParts][kLiveCntStride]: count_w of the iteration with parity p at [p][w][0] -- a 64-byte line each (one returning atomic per position
//     block lands there); the position pass of iteration j counts in set j & 1, k_encode_tiles(j) reads it and clears the other one for iteration j + 1
constexpr uint32_t kLiveMaxParts = 64, kLiveCntStride = 16;
struct LiveArgs { const uint32_t* occ_bits; uint32_t* idx; uint32_t* cnt; uint32_t spw, n_parts; };      // occ_bits == nullptr: every sample is evaluated, no lists

// What k_optimizer prepares for the next iteration of the fused backend (all zero = nothing): candidate rays and the A-fragment image.
struct OptimNext { uint32_t cand_blocks; uint16_t* frag_image; FragDims fd; BatchPtrs b; DatasetPtrs ds; ObjectConst oc;
                   // pos_blocks > 0 (level-tile encode): `b` holds the NEXT iteration's candidates already (k_encode_tiles generated them), these blocks sample
                   // its positions
                   uint32_t pos_blocks; float* x_all; LiveArgs live; };

// debug buffer ids for mon_object_debug_read (stable numbering, see binding.py BUF)
enum {
    MON_BUF_MASTER = 0, MON_BUF_HALF = 1, MON_BUF_EMA = 2, MON_BUF_M1 = 3, MON_BUF_M2 = 4, MON_BUF_STEPS = 5,
    MON_BUF_GMLP = 6, MON_BUF_GGRID_H = 9, MON_BUF_PTS = 10, MON_BUF_TDIST = 11, MON_BUF_E = 12, MON_BUF_HID = 13,
    MON_BUF_O = 14, MON_BUF_DO = 15, MON_BUF_DHID = 16, MON_BUF_DE = 17, MON_BUF_RGB_RAY = 18, MON_BUF_DEPTH_RAY = 19,
    MON_BUF_MASK_RAY = 20, MON_BUF_LOSS_RAY = 21, MON_BUF_RAY_O = 22, MON_BUF_RAY_D = 23, MON_BUF_RAY_T0 = 24,
    MON_BUF_RAY_T1 = 25, MON_BUF_TARGET = 26, MON_BUF_TARGET_DEPTH = 27, MON_BUF_BGCOL = 28, MON_BUF_RAY_FLAG = 29,
    MON_BUF_RAY_DN = 31, MON_BUF_MASK = 32, MON_BUF_STATE = 33,
    MON_BUF_FRAG_TRAIN = 34,    // the A-fragment image the next fused iteration will use (64 x 512 halves)
    MON_BUF_FRAG_REF = 35,      // the same image rebuilt from the current fp16 weights by k_build_frag_image (layout test)
    MON_BUF_X_ALL = 36,         // level-tile encode: positions float4 [B] of the batch the next / last iteration uses
    MON_BUF_E_SOA = 37,         // level-tile encode: encoded features half2 [L][B] of the last iteration
    MON_BUF_HALF_TILES = 38,    // level-tile encode: the fp16 grid in tile order (ParamPtrs::half_tiles)
    MON_BUF_LIVE_CNT = 40,      // occupancy-grid skipping on the level tiles: the live-sample counters [2][kLiveMaxParts][kLiveCntStride] (LiveArgs)
    MON_BUF_GGRID_F32 = 39      // the grid gradient the next k_optimizer will form, fp32: gradient table + the partial tables summed in the kernel's order
};

// Process-wide test and tuning switches (mon_set_option, include/mon_core.h); defaults are the product behaviour.
struct Options {      // (atomics: tests and tools flip options while object threads read them)
    std::atomic<long> backend{ -1 }, use_graph{ 0 }, big_switch{ 16384 }, lds_encode{ 1 }, train_lanes{ 2 }, roctx{ 0 }, step_variant{ 0 },
         keep_zero_samples{ 0 },   // 1: k_fused_train hands zero-gradient samples to the scatter too (the exactness test's A/B; same parameters, slower)
         tile_render{ 1 };      // inference on feature-planar level tiles: 0 never (gathers), 1 crops of 4096 rays and more + point queries, 2 always
    // NerfManagerOffline's 10 x 500 iterations (nerf_manager.cu:89): mon_offline_set_schedule, read by mon_offline_init
    std::atomic<long> offline_outer{ 10 }, offline_inner{ 500 };
};
// Round 6: the A/B switches whose losing setting only a measurement ever wanted are VARIANT BUILDS now (tools/variant_build.sh <tag> -DMON_VARIANT_...; the
// oracle tests of the large-table optimizer run against each, tools/gpu_variants_large.sh), not runtime options of the shipping library:
//   MON_VARIANT_STEPS32   per-parameter step counters always 32 bits (shipping: saturating 16-bit ones where that is exact)
//   MON_VARIANT_ARRAYS    tables above 8 M parameters keep master / m1 / m2 / steps as four arrays (shipping: 128-byte chunk records)
//   MON_VARIANT_NO_FLAGS  the lazy optimizer finds touched chunks by scanning the gradient table (shipping: byte flags next to it)
#ifdef MON_VARIANT_STEPS32
constexpr bool kSteps16 = false;
#else
constexpr bool kSteps16 = true;
#endif
#ifdef MON_VARIANT_ARRAYS
constexpr bool kStateRecords = false;
#else
constexpr bool kStateRecords = true;
#endif
#ifdef MON_VARIANT_NO_FLAGS
constexpr bool kTouchedFlags = false;
#else
constexpr bool kTouchedFlags = true;
#endif
constexpr int kLaneChunk = 16;          // iterations an object enqueues per turn on a training lane (measured best, HISTORY 7.2)
constexpr long kOnlineSliceMin = 2;     // shortest training slice of the online manager (iterations)
Options& options();
int option_set(const char* name, long value);
int option_get(const char* name, long* value);

hipError_t use_device(int logical_device);      // hipSetDevice through the logical-device map (model.cpp)
int device_enter(int logical_device);            // a standalone call's way in: MON_ERR_NO_DEVICE without a device, then use_device
int set_logical_devices(int n);

// ---- kernel launchers (kernels_*.hip)
void launch_gen_candidates(hipStream_t s, const BatchPtrs& b, const DatasetPtrs& ds, const ObjectConst& oc, const DevState* st);
void launch_build_rays(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, DevState* st);
void launch_gen_samples(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, const DevState* st, uint32_t S, uint32_t n_samples, uint32_t stream_id,
        uint32_t idx_base, int render, float* x4_or_null = nullptr);
void launch_render_rays(hipStream_t s, const BatchPtrs& b, const Intrinsics& K, const ObjectConst& oc, mon_frame_bbox box, const Mat4& pose, int pose_is_Toc,
        uint32_t pix0, uint32_t n);
void launch_grid_points(hipStream_t s, float* pts, int rx, int ry, int rz, uint32_t p0, uint32_t n);

// unfused network path (kernels_net.hip)
void launch_encode(hipStream_t s, const LevelTable& lt, const NetDims& nd, const uint16_t* params, const float* pts, uint16_t* E, uint32_t n,
        const DevState* st_or_null);
void launch_mlp_forward(hipStream_t s, const NetDims& nd, const uint16_t* params, const uint16_t* E, uint16_t* Hid_or_null, uint16_t* O, uint32_t n,
        const DevState* st_or_null);
void launch_mlp_backward(hipStream_t s, const NetDims& nd, const uint16_t* params, const uint16_t* Hid, const uint16_t* dO, uint16_t* dHid, uint16_t* dE,
        uint32_t n, const DevState* st);
void launch_weight_grads(hipStream_t s, const NetDims& nd, const uint16_t* E, const uint16_t* Hid, const uint16_t* dHid, const uint16_t* dO, float* gmlp,
        uint32_t n, const DevState* st);
void launch_grid_backward(hipStream_t s, const LevelTable& lt, const NetDims& nd, const float* pts, const uint16_t* dE, uint16_t* ggrid, uint32_t n,
        const DevState* st);

// MFMA layer-at-a-time kernels (kernels_layers.hip): the shapes the fused kernels do not take.  ws_T: the T-layout copies the weight gradients read
// (layers_workspace_halves(nd, n) halves; nullptr = forward only, nothing is kept).  false: shape / batch not covered, nothing was launched
size_t layers_workspace_halves(const NetDims& nd, uint32_t n);
bool launch_mlp_forward_layers(hipStream_t s, const NetDims& nd, const uint16_t* params, const uint16_t* E, uint16_t* Hid, uint16_t* O, uint32_t n,
        const DevState* st_or_null, uint16_t* ws_T_or_null,
        // the features as k_encode_tiles wrote them ([L][n] half2) instead of row-major E; E_out: where the row-major copy goes
        const uint16_t* e_soa_or_null = nullptr, uint16_t* E_out = nullptr,
        // false (whole steps): the activations go out in T layout + one ReLU mask bit each; row-major Hid is not written and launch_mlp_backward_layers must be
        // called with keep_rowmajor = false too
        bool keep_rowmajor = true);
bool launch_mlp_backward_layers(hipStream_t s, const NetDims& nd, const uint16_t* params, const uint16_t* Hid, const uint16_t* dO, uint16_t* dHid, uint16_t* dE,
        uint32_t n, const DevState* st, uint16_t* ws_T,
        bool keep_rowmajor = true /* false: dHid is written in T layout only -- the weight gradients' copy; the debug read-back then sees stale rows */,
        // != nullptr (whole steps of the hybrid scatter): dL/dE and the positions go straight into k_grid_scatter's hand-over layout (what k_rows_to_bins writes:
        // every sample at its natural slot of its ray's bin, every bin counter = its capacity) instead of row-major dE
        const struct BinsOut* bins = nullptr);
struct BinsOut { uint16_t* de_soa; float* x_soa; const float* pts; uint32_t n_bins; float clampv; DevState* st; };
void launch_weight_grads_layers(hipStream_t s, const NetDims& nd, float* gmlp, uint32_t n, const DevState* st, uint16_t* ws_T);
struct Model;
// inference forward of n samples E -> O with the layer kernels where the object has them (Hid of the training batch as scratch, piece by piece), else k_mlp_forward
void mlp_forward_inference(Model& m, hipStream_t s, const uint16_t* params, const uint16_t* E, uint16_t* O, uint32_t n);

// composite / loss gradient (kernels_composite.hip)
void launch_composite_grad(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, DevState* st);
// DevState::loss_sum = the sum of loss_ray[0 .. R) in a fixed order (one workgroup; a skipped batch keeps its zero)
void launch_loss_sum(hipStream_t s, const float* loss_ray, uint32_t R, DevState* st);
void launch_composite_render(hipStream_t s, const BatchPtrs& b, uint32_t S, uint32_t n_rays, float* rgb, float* depth, float* mask);
void launch_extract_density(hipStream_t s, const uint16_t* O, float* out, uint32_t n);
void launch_master_to_half(hipStream_t s, const float* master, uint16_t* half, uint32_t n);
// ParamPtrs::rec -> a flat array (0 master, 1 m1, 2 m2, 3 step counters as uint32)
void launch_state_unpack(hipStream_t s, const float* rec, int which, void* dst, uint32_t n);
void launch_state_pack_master(hipStream_t s, const float* master, float* rec, uint32_t n);
// checkpoints: chunks [first_chunk, first_chunk + n_chunks) of the records <-> a flat staging array whose element 0 is the range's first (which: 0 master,
// 1 m1, 2 m2, 3 step counters as uint32, 4 the lazy EMA's per-chunk step); 16 bytes per lane.  steps16: the array layout's 16-bit counters <-> uint32
void launch_state_unpack_range(hipStream_t s, const float* rec, int which, void* dst, uint32_t first_chunk, uint32_t n_chunks);
void launch_state_pack_range(hipStream_t s, float* rec, int which, const void* src, uint32_t first_chunk, uint32_t n_chunks);
void launch_steps16_unpack_range(hipStream_t s, const uint16_t* steps16, void* dst, uint32_t first_chunk, uint32_t n_chunks);
void launch_steps16_pack_range(hipStream_t s, uint16_t* steps16, const void* src, uint32_t first_chunk, uint32_t n_chunks);
void launch_copy_params(hipStream_t s, const uint16_t* src, uint16_t* dst, uint32_t n);
void model_leave_lane(struct Model& m);      // non-training work goes to the object's own stream (model.cpp, training lanes)
// host (pinned) images -> packed RGBA8 | instance << 24
void launch_pack_frame(hipStream_t s, const uint8_t* rgb, int ch, int ri, int bi, const uint8_t* inst, uint32_t* dst, uint32_t px);
// source: pinned host memory the host rewrites (system-scope loads)
void launch_copy_from_host(hipStream_t s, const void* src, void* dst, uint32_t n_words);

// NeRF_Model::Step's schedule (kernels_step.hip; option step_variant): sample compaction + rollover of the batch between the two network passes
void launch_step_compaction(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, DevState* st, uint32_t* steps, float* pts_compacted);

// optimizer (kernels_optim.hip)
// lazy_below: gradient-carrying samples at or below which the dense-table optimizer requests Adam state per touched chunk only
void launch_optimizer(hipStream_t s, const ParamPtrs& p, const OptimConst& oc, const DevState* st, DevState* st_next, const OptimNext& nx, uint32_t lazy_below);
void launch_ema_finalize(hipStream_t s, const ParamPtrs& p, const OptimConst& oc, const DevState* st);
void launch_reduce_partials(hipStream_t s, const float* partials, uint32_t n_partials, const NetDims& nd, float* gmlp, DevState* st);
uint32_t fused_partial_cols(const NetDims& nd);      // columns of a k_fused_train dW partial row (accumulator layout), the loss partial follows

// fused MFMA path (kernels_fused.hip)
constexpr uint32_t kMaxFusedGrid = 512;       // workgroups of k_fused_train (= dW partial rows per step): two per CU
bool fused_supported(const NetDims& nd, uint32_t S, uint32_t R);
uint32_t fused_train_grid(const NetDims& nd, uint32_t R);
void launch_fused_train(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ParamPtrs& p, const BatchPtrs& b, const ObjectConst& oc, DevState* st,
        float* dw_partials, int debug_dump,
                        uint16_t* de_soa, float* x_soa, uint32_t lds_level_mask, uint16_t* frag_image, uint32_t big_switch, uint8_t* touched,
                                const uint32_t* occ_bits, uint32_t n_bins, const uint16_t* e_soa_or_null, const float* x_all_or_null);
// level-tile encode (kernels_encode.hip): the forward gathers as LDS reads of a level tile, one workgroup per (level, sample partition)
bool encode_tiles_supported(const LevelTable& lt, const NetDims& nd);
void encode_tiles_setup_device();
void launch_sample_points(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, DevState* st, float* x_all, const LiveArgs& live = LiveArgs{});
void launch_encode_tiles(hipStream_t s, const LevelFast& lf, const NetDims& nd, const uint16_t* half_tiles, const float* x_all, uint16_t* e_soa, uint32_t B,
        const DevState* st,
                         // b_next: the candidate set GenerateRays of the next iteration goes to
                         const BatchPtrs* b_next_or_null, const DatasetPtrs& ds, const ObjectConst& oc, const LiveArgs& live = LiveArgs{});
uint32_t encode_tiles_spw(uint32_t B);          // samples per sample partition of k_encode_tiles (a partition's live list starts at w * spw)
// XORWOW sample stream (kernels_encode.hip k_xorwow_fill): one thread per lane, the generate calls of one iteration / one Render in the reference's order
void launch_xorwow_fill(hipStream_t s, void* lane_states, uint32_t lanes, int flavour, uint32_t start_lane, float* out0, uint32_t n0, float* out1, uint32_t n1,
        float* out2, uint32_t n2);
void launch_build_tiles_image(hipStream_t s, const LevelFast& lf, const NetDims& nd, const uint16_t* params, uint16_t* half_tiles);
void launch_occupancy_update(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const ObjectConst& oc, uint16_t* frag_image,
        float raw_threshold, uint32_t* tmp, uint32_t* bits);
uint32_t scatter_plan(const LevelTable& lt, const NetDims& nd, ScatterLevels& sl);
uint32_t scatter_level_mask(const LevelTable& lt, const NetDims& nd);
bool grid_scatter_sums_partials(const LevelTable& lt, const NetDims& nd);
void launch_grid_scatter(hipStream_t s, const LevelTable& lt, const LevelFast& lf, const NetDims& nd, const uint16_t* de_soa, const float* x_soa, uint32_t B,
        uint32_t n_bins, uint16_t* gpart, uint32_t part_stride_entries, DevState* st,
                         // partials != null: also sums the dW partial rows (k_reduce_partials folded in)
                         const float* partials_or_null, uint32_t n_partials, float* gmlp, DevState* st_next);
// layer-at-a-time backend: dL/dE rows + positions of every sample into k_grid_scatter's hand-over layout (kernels_scatter.hip)
void launch_rows_to_bins(hipStream_t s, const LevelFast& lf, const NetDims& nd, const uint16_t* dE, const float* pts, uint32_t R, uint32_t S, uint32_t n_bins,
        uint16_t* de_soa, float* x_soa, DevState* st);
size_t big_scatter_workspace_bytes(const LevelTable& lt, const NetDims& nd, uint32_t lds_mask, uint32_t B);
void launch_big_scatter(hipStream_t s, const LevelTable& lt, const LevelFast& lf, const NetDims& nd, uint32_t lds_mask, const uint16_t* de_soa,
        const float* x_soa, uint32_t B,
                        uint32_t n_bins, const DevState* st, uint32_t big_switch, void* workspace, uint16_t* ggrid, uint8_t* touched_grid);
// Empty-space skipping of a render (mon_object_set_render_skip, default off).  bits == nullptr: the plain kernels, nothing else is read.
struct RenderSkipArgs {
    const uint32_t* bits = nullptr;   // the render's kOccRes^3 grid (dilated), x fastest
    uint32_t* stats = nullptr;        // device counters: [0] += samples in live cells, [1] += samples of rays that hit the box (zeroed by the caller)
    // tile path, per chunk: each job's 64 live bits (two words per job slot), the live-sample lists of k_encode_feat's partitions (spw slots each) and their
    // counters (kRenderListStride words apart)
    uint32_t* job_bits = nullptr; uint32_t* idx = nullptr; uint32_t* cnt = nullptr; uint32_t spw = 0;
};
constexpr uint32_t kRenderListStride = 16;
void launch_fused_render(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const BatchPtrs& b, const ObjectConst& oc,
        uint32_t n_rays, uint32_t idx_base, float* rgb, float* depth, float* mask, uint16_t* frag_image, int build_image,
        const RenderSkipArgs& skip = RenderSkipArgs{});
void launch_build_frag_image(hipStream_t s, const uint16_t* params, const NetDims& nd, uint16_t* image);
// Scene render (mon_scene_render, kernels_render.hip).  Sample lists of kSceneListLen (= 2S) slots, list k of ray r at (k * cap + r) * kSceneListLen:
// t [fp32], {alpha, r, g, b} [float4], and a count per (list, ray).  k_fused_render<EMIT> writes one object's lists (skip_bits: its render grid or nullptr;
// the skip counters are not touched); k_scene_composite merges a ray's lists by t (ties to the lower list) and composites them front to back.
constexpr uint32_t kSceneListLen = 64, kSceneMaxLists = 256;
// The kernels' dynamic LDS (SceneLds, scene_device.h): the merged order, one uint16_t per sample slot, then kSceneLdsWords arrays of one 4-byte word per list
// (kSceneLdsGradWords in the kernels that keep the composite gradient's two more).  scene_lds_word = the byte offset of word array i; that of the array
// behind the last one is the size.
constexpr uint32_t kSceneLdsWords = 5, kSceneLdsGradWords = kSceneLdsWords + 2;
constexpr uint32_t scene_lds_word(uint32_t n_lists, uint32_t i) { return n_lists * (2u * kSceneListLen + 4u * i); }
constexpr uint32_t scene_composite_lds(uint32_t n_lists) { return scene_lds_word(n_lists, kSceneLdsWords); }
constexpr uint32_t scene_composite_grad_lds(uint32_t n_lists) { return scene_lds_word(n_lists, kSceneLdsGradWords); }
static_assert(scene_composite_lds(1) == 2u * kSceneListLen + 20u && scene_composite_grad_lds(1) == 2u * kSceneListLen + 28u &&
              scene_composite_lds(kSceneMaxLists) == kSceneMaxLists * (2u * kSceneListLen + 20u) &&
              scene_composite_grad_lds(kSceneMaxLists) == kSceneMaxLists * (2u * kSceneListLen + 28u), "the LDS per list that profiles and DESIGN.md quote");
// one workgroup per ray, at most 8 192 of them
constexpr uint32_t scene_composite_grid(uint32_t n_rays) { return n_rays < 8192u ? n_rays : 8192u; }
void launch_fused_render_emit(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const BatchPtrs& b, const ObjectConst& oc,
        uint32_t n_rays, uint32_t idx_base, float* t, float* attr, uint32_t* cnt, uint16_t* frag_image, int build_image, const uint32_t* skip_bits,
        const uint32_t* keys = nullptr);
void launch_scene_composite(hipStream_t s, uint32_t n_rays, uint32_t n_lists, uint32_t cap, const float* t, const float* attr, const uint32_t* cnt,
        const float* dn, float* rgb, float* depth, float* opacity, int32_t* instance);
// Scene probe (mon_scene_probe, kernels_scene_probe.hip).  k_scene_probe_rays: one object's ray rows of n queries (their poses from `poses`; keys, where
// given, receives the queries' keys); the keyed emit (launch_fused_render_emit with keys: jitter index keys[ray] * 2S + k, idx_base unused);
// k_scene_probe_composite: k_scene_composite plus the depth and list of the first sample after which 1 - T > 0.5 (0 and -1: none).
constexpr uint32_t kSceneProbeMaxPoses = 4096, kSceneProbeMaxQueries = 1u << 22, kSceneProbeMaxKey = 1u << 26;
void launch_scene_probe_rays(hipStream_t s, const BatchPtrs& b, const Intrinsics& K, const ObjectConst& oc, const mon_scene_query* q, const float* poses,
        uint32_t* keys, uint32_t n);
void launch_scene_probe_composite(hipStream_t s, uint32_t n_rays, uint32_t n_lists, uint32_t cap, const float* t, const float* attr, const uint32_t* cnt,
        const float* dn, float* rgb, float* depth, float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance);
// Ray cast (mon_scene_cast, kernels_scene_cast.hip).  k_scene_cast_rays: one object's ray rows of n world rays clipped to [0, t_max] (dn = 1), their box
// entries lo into entry[n], and (keys given) their keys; the keyed emit as the probe uses it; k_scene_cast_composite: k_scene_probe_composite with the
// threshold thr, the distance undivided, and the hit placed inside its sample's interval (entry = [lists][cap]).
void launch_scene_cast_rays(hipStream_t s, const BatchPtrs& b, const ObjectConst& oc, const mon_scene_ray* rays, uint32_t* keys, float* entry, uint32_t n);
void launch_scene_cast_composite(hipStream_t s, uint32_t n_rays, uint32_t n_lists, uint32_t cap, float thr, const float* t, const float* attr,
        const uint32_t* cnt, const float* entry, float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t,
        int32_t* hit_instance);
// Point queries (mon_scene_query_points / _lattice, mon_object_query_points; kernels_scene_points.hip).  k_scene_points: one object's rows [n][12] = u[3],
// inside, raw4, sigma, r, g, b of the n points of a pass -- item i is point i of `pts` (device, [n][3]) or, with pts == nullptr, lattice point first + i
// (ix fastest, fmaf(i_a, step_a, origin_a)); world = false: the points are unit-cube points of the object, taken as given.  build_image: build the
// fragment image first (a call's first pass).  k_scene_points_fold: the K rows of each point ([K][cap][12]) -> the five outputs.
// A lattice: nx x ny x nz cells, cell (i, j, k) at flat index (k * ny + j) * nx + i and at origin + (i, j, k) * step.  What the lattice queries ask, what a
// distance-field handle sits on and what the launch wrappers of the kernels over a lattice take (the standalone calls have no origin: 0).
struct Lattice {
    int nx = 1, ny = 1, nz = 1; float origin[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 };
    Lattice(const float* origin3 = nullptr, const float* step3 = nullptr, int nx_ = 1, int ny_ = 1, int nz_ = 1) : nx(nx_), ny(ny_), nz(nz_) {
        for (int a = 0; a < 3; ++a) { origin[a] = origin3 ? origin3[a] : 0.f; step[a] = step3 ? step3[a] : 0.f; }
    }
    size_t n() const { return (size_t)nx * ny * nz; }
};
struct ScenePointsArgs { const float* pts; float origin[3], step[3]; uint32_t nx, ny, first, n; float* rows; };
void launch_scene_points(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const ObjectConst& oc, uint16_t* frag_image,
        int build_image, bool world, const ScenePointsArgs& p);
void launch_scene_points_fold(hipStream_t s, uint32_t n, uint32_t n_objs, uint32_t cap, const float* rows, float* sigma, float* rgb, int32_t* owner,
        float* owner_sigma, uint32_t* n_inside);
// Point gradients (mon_scene_query_gradients / _lattice_gradients, mon_object_query_gradients; kernels_scene_gradients.hip).  k_scene_point_grads:
// k_scene_points with rows [n][16] = its twelve floats (the same bits), g[3], 0 -- world: g = R_ow^T d raw3 / d q, the world gradient of the object's log
// density; else g = d raw3 / d u.  frag_image: the FULL fragment image (N_FRAGS x 512 halves; built first when build_image), level_w: device, the
// object's L weights.  k_scene_gradients_fold: the K rows of each point ([K][cap][16]) -> the five outputs, grad_log, grad_sigma, normal; select: device,
// [n] or nullptr.
void launch_scene_point_grads(hipStream_t s, const LevelFast& lt, const NetDims& nd, const uint16_t* params, const ObjectConst& oc, uint16_t* frag_image,
        int build_image, bool world, const ScenePointsArgs& p, const float* level_w);
void launch_scene_gradients_fold(hipStream_t s, uint32_t n, uint32_t n_objs, uint32_t cap, const float* rows, const int32_t* select, float* sigma, float* rgb,
        int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma, float* normal);
// Distance fields (mon_distance_transform, mon_scene_distance_lattice; kernels_distance.hip).  k_distance_mask: occ[i] = !(sigma[i] <= sigma_min).
// launch_distance_passes: the x, y and z pass of k_distance_pass over the mask (`invert`: over its complement) -> the squared distance to the nearest
// occupied cell in v[0 .. n) and that cell's flat index in site[0 .. n) (+inf and -1 without one); v and site hold 2 n elements, n = nx ny nz <= 2^22.
// k_distance_finish: dist = the root, max_dist applied; nearest and nearest_owner (= owner[nearest]; owner: device, [n]) may be nullptr.
void launch_distance_mask(hipStream_t s, uint32_t n, const float* sigma, float sigma_min, uint8_t* occ);
void launch_distance_passes(hipStream_t s, const uint8_t* occ, bool invert, const Lattice& g, float* v, int32_t* site);
void launch_distance_finish(hipStream_t s, uint32_t n, const float* d2, const int32_t* site, float max_dist, const int32_t* owner, float* dist,
        int32_t* nearest, int32_t* nearest_owner);
// launch_distance_axis: one pass of k_distance_pass along axis ax (0, 1, 2) from the values and sites of a pass before (launch_distance_passes' y and z
// pass; any axis may be run so).
void launch_distance_axis(hipStream_t s, int ax, const Lattice& g, const float* v_in, const int32_t* s_in, float* v_out, int32_t* s_out);
// Signed, sub-cell distance fields (mon_signed_distance_transform, mon_scene_signed_distance_lattice; kernels_signed_distance.hip).  k_signed_values:
// ins[i] = !(sigma[i] <= sigma_min), val[i] = sigma[i] or logf(sigma[i]) (val nullptr: not written), iso_out[0] = sigma_min or logf(sigma_min) (nullptr:
// not written).  launch_signed_passes (the level: iso_p[0] on the device, nullptr: iso): per axis k_surface_line_pass and two passes of k_distance_pass -> the three chains' squared distances and edges in
// v[0 .. 3 n) and site[0 .. 3 n); v and site hold 4 n elements.  k_signed_finish: the least of the three, the root, max_dist, the sign from ins;
// nearest_edge and nearest_owner (= owner[the inside end of the edge]; owner: device, [n]) may be nullptr.
void launch_signed_values(hipStream_t s, uint32_t n, const float* sigma, float sigma_min, bool use_log, float* val, uint8_t* ins, float* iso_out);
void launch_signed_passes(hipStream_t s, const float* val, const uint8_t* ins, const float* iso_p, float iso, const Lattice& g, float* v, int32_t* site);
void launch_signed_finish(hipStream_t s, const Lattice& g, const float* v, const int32_t* site, const uint8_t* ins, float max_dist, const int32_t* owner,
        float* sdist, int32_t* nearest_edge, int32_t* nearest_owner);
// Connected components (mon_label_components, mon_scene_components_lattice; kernels_components.hip).  launch_components: the mask occ[n] -> label[n] and
// comp[n] (both required here), the count in meta[0] and the cap flag in meta[1] (meta: 2 words, cleared first; a flag other than 0 afterwards: a device
// loop ran into its cap), the records of the components below cap in table (nullptr: none; room for min(cap, n) records).  scan: components_scan_words(n)
// words.  connectivity is 6, 18 or 26 (checked by the caller).  launch_components_clear_mask: occ = dist > clearance.  launch_components_home: words
// [0, n_words) of src -> dst, of the table's words (8 per record from word table_word on, table_cap records) only the records that were written.
size_t components_scan_words(uint32_t n);
void launch_components(hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, int32_t* label, int32_t* comp, uint32_t* scan,
        mon_lattice_component* table, uint32_t cap, uint32_t* meta);
void launch_components_clear_mask(hipStream_t s, uint32_t n, const float* dist, float clearance, uint8_t* occ);
void launch_components_home(hipStream_t s, const uint32_t* src, uint32_t* dst, uint32_t n_words, uint32_t table_word, uint32_t table_cap, const uint32_t* meta);
// Shortest-path cost fields (mon_shortest_paths, mon_scene_paths_lattice; kernels_paths.hip).  occ: the passable cells; mult: the per-cell multiplier or
// nullptr (none); flags: 2 * paths_tiles(g) bytes.  launch_paths_init: cost = +inf, 0 at the passable seeds (device array, every entry below n), the
// flags of sweep 0.  launch_paths_sweep: sweep number `sweep` (0, 1, ...: they alternate between the two rows of flags); *raised becomes 1 iff the sweep left
// work for the next one (the caller clears it).  launch_paths_finish: next (may be nullptr) on the untruncated cost, then cost_out (another array than
// cost) = cost cut at max_cost.  launch_paths_soft: the scene call's multiplier from a distance row.  connectivity is 6, 18 or 26 (checked by the caller).
uint32_t paths_tiles(const Lattice& g);
void launch_paths_init(hipStream_t s, const uint8_t* occ, const Lattice& g, const int32_t* seeds, uint32_t n_seeds, float* cost, uint8_t* flags);
void launch_paths_sweep(hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, const float* mult, float* cost, uint8_t* flags, uint32_t sweep,
        uint32_t* raised);
void launch_paths_finish(hipStream_t s, const uint8_t* occ, const Lattice& g, int connectivity, const float* mult, const float* cost, float max_cost,
        float* cost_out, int32_t* next);
void launch_paths_soft(hipStream_t s, uint32_t n, const float* dist, float soft_radius, float soft_weight, float* mult);
// Device-resident distance fields (mon_dist_field_*; kernels_clearance.hip).  DistFieldView: the cells D (device, [nz][ny][nx]) on their lattice g as the
// kernels take them; the wrappers form it.
// launch_field_sample: dist[n] and grad[n][3] (may be nullptr) at xyz[n][3].  launch_traj_score: the header's outputs of n_traj trajectories (device
// arrays; all but min_clear may be nullptr); n_samp = (n_way - 1) n_sub + 1; the launch fills in pad.  launch_field_max: out[0] = the largest of v[0 .. n),
// partial: kFieldMaxBlocks floats.
struct DistFieldView { const float* D; int nx, ny, nz; float o[3], s[3]; };
inline DistFieldView dist_field_view(const float* D, const Lattice& g) { return { D, g.nx, g.ny, g.nz, { g.origin[0], g.origin[1], g.origin[2] }, { g.step[0], g.step[1], g.step[2] } }; }
struct TrajScoreArgs { uint32_t n_traj, n_way, n_sub, n_samp, pad; float outside, margin, safe; float* min_clear; int32_t* first_hit; float* cost;
                       float* way_clear; float* way_grad; };
constexpr uint32_t kFieldMaxBlocks = 256;
void launch_field_sample(hipStream_t s, const float* D, const Lattice& g, const float* xyz, uint32_t n, float outside, float* dist, float* grad);
void launch_traj_score(hipStream_t s, const float* D, const Lattice& g, const float* spheres, uint32_t n_spheres, const float* ways, bool pose, TrajScoreArgs a);
void launch_field_max(hipStream_t s, const float* v, uint32_t n, float* partial, float* out);
// Scan matching against a distance field (mon_dist_field_match / _register; kernels_scan_match.hip).  launch_scan_match: rows[n_pose][32] = 21 A terms, 6 b
// terms, cost, n_inside, n_inlier (counts as exact floats), 0, 0 per pose -- or, normal false, rows[n_pose][4] = cost, n_inside, n_inlier, 0.  All arrays
// are the device's; points must be 16-byte aligned; pivots may be nullptr; scratch: scan_match_scratch(n, n_pose) floats.
struct ScanMatchArgs { const float* points; const float* poses; const float* pivots; uint32_t n, n_pose; float huber, outside; };
constexpr uint32_t kScanMatchChunk = 1024, kScanMatchFold = 64, kScanMatchRow = 32, kScanMatchLite = 4;
size_t scan_match_scratch(uint32_t n, uint32_t n_pose);
void launch_scan_match(hipStream_t s, const float* D, const Lattice& g, const ScanMatchArgs& a, bool normal, float* scratch, float* rows);
// launch_scan_fold: the part rows scratch[n_pose][n_in][32] of such a launch folded by k_scan_fold to rows[n_pose][width], columns first .. of each row.
void launch_scan_fold(hipStream_t s, float* scratch, uint32_t n_in, uint32_t n_pose, float* rows, uint32_t first, uint32_t width);
// Ray tracing against a distance field (mon_dist_field_trace / _beam_score; kernels_field_trace.hip).  launch_field_trace: n rays [n][6] (8-byte aligned)
// under n_pose poses (nullptr: one pose, world rays) marched by the header's rule; range, status, steps at [h * stride + ray], normal at 3 x that; status,
// steps and normal may be nullptr.  launch_beam_score: rows[n_pose][4] = cost, n_valid, n_hit (counts as exact floats), 0 from the ranges and statuses such a
// launch left at a stride that is a multiple of 4; range, status and measured 16-byte aligned; scratch: beam_score_scratch(n, n_pose) floats.
struct FieldTraceArgs { const float* rays; const float* poses; uint32_t n, n_pose, stride; float t_min, t_max, eps, step_min, relax, step_outside;
                        uint32_t max_steps; float* range; int32_t* status; int32_t* steps; float* normal; };
void launch_field_trace(hipStream_t s, const float* D, const Lattice& g, const FieldTraceArgs& a);
size_t beam_score_scratch(uint32_t n, uint32_t n_pose);
void launch_beam_score(hipStream_t s, const float* range, const int32_t* status, const float* measured, uint32_t n, uint32_t n_pose, uint32_t stride,
        float huber, float* scratch, float* rows);
// Pose refinement (mon_object_pose_loss / mon_object_refine_pose, kernels_pose.hip).  k_pose_rays: one record of 4 float4 per drawn ray from the pose in
// device memory (pose[16], world -> object); k_pose_grad<shape>: loss and position gradient, one partial row of 8 floats {g, x x g, loss, 0} per workgroup
// (pose_grad_grid of them); k_pose_update: the rows summed in a fixed order, x inv_n -> out[8 * it] = {loss, grad6, 0}, optionally the Adam step on pose.
// Counter-RNG streams of the drawn rays: sample jitter (key ray * 2S + k) and pixel draws (key ray), both keyed by (seed, iteration).
constexpr uint32_t kStreamPose = 4, kStreamPoseXY = 5, kStreamPoseHyp = 6;     // (6: mon_pose_hypotheses' draws, keyed (seed, hypothesis, 0..5))
constexpr uint32_t kPoseMaxGrid = 1024, kPoseMaxRays = 1u << 22;
struct PoseRayArgs {
    const mon_frame_bbox* boxes; const uint32_t* prefix;      // the boxes and the exclusive prefix sums of their areas
    uint32_t n_obs, n_rays, total, drawn, iteration; uint64_t seed;
    DatasetPtrs ds; Aabb aabb; uint32_t instance_id; const float* pose; float4* rec;
};
struct PoseGradArgs {
    const float4* rec; uint32_t n_rays;
    uint64_t seed; uint32_t stream, step;                       // jitter of sample k: rand01(seed, stream, step, base + k)
    float w_rgb, w_mask, w_depth, huber, inv_n;
    float* partials;
    float *dbg_x, *dbg_raw, *dbg_g;                             // mon_debug_pose_samples: [ray][2S][3 | 4 | 3], or nullptr
};
struct PoseGradArgsLW : PoseGradArgs { const float* level_w; };   // k_pose_grad<.., LW = true>: level l's term of g times level_w[l]
uint32_t pose_grad_grid(uint32_t n_rays);
void launch_pose_rays(hipStream_t s, const PoseRayArgs& a);
// level_w: nullptr = k_pose_grad<.., false>; else the device array of the nd.L level weights of this evaluation (k_pose_grad<.., true>)
void launch_pose_grad(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ObjectConst& oc, const uint16_t* params, uint16_t* frag_image,
        int build_image, const PoseGradArgs& p, const float* level_w);
void launch_pose_update(hipStream_t s, const float* partials, uint32_t n_parts, float inv_n, float* out, float* trace, uint32_t it, int step, float lr_t,
        float lr_r, float* pose, float* moments);
// Camera refinement against a scene of objects (mon_scene_pose_loss / mon_scene_refine_camera, kernels_scene_pose.hip).  Per chunk of `cap` rays:
// k_scene_pose_rays (targets, every object's ray record under the Twc in device memory) -> per object k_scene_pose_obj<.., BWD = false> (its sample lists, the
// scene render's EMIT format) -> k_scene_composite_grad (merge, loss, composite backward: {dL/dalpha, w} into every list slot, {G_rgb, l} per ray, loss
// partials per workgroup) -> per object k_scene_pose_obj<.., BWD = true> (MLP backward + position gradient, one partial row of 8 floats per workgroup);
// per evaluation k_scene_pose_update (rows -> grad6 in the camera frame, Adam, Twc <- Twc exp(delta^)).
constexpr uint32_t kSceneLossParts = 4096;
struct SceneObjConst { float Tow[16]; Aabb aabb; uint32_t instance_id; uint32_t pad; };
struct ScenePoseRayArgs {
    const mon_frame_bbox* boxes; const uint32_t* prefix;      // the boxes and the exclusive prefix sums of their areas
    uint32_t n_obs, n_rays, ray0, total, drawn, iteration; uint64_t seed;
    DatasetPtrs ds; const SceneObjConst* objs; uint32_t n_objs, cap; const float* pose;
    float4* rec; float* mstar; float4* ray;                   // [n_objs][cap][3], [n_objs][cap], [cap][3]
};
struct ScenePoseObjArgs {
    const float4* rec; uint32_t n_rays, ray0;                 // this object's records of the chunk; ray0 = the chunk's first ray (debug dump rows)
    uint64_t seed; uint32_t stream, step;                     // jitter of sample k: rand01(seed, stream, step, base + k)
    float* t; float4* attr; uint32_t* cnt;                    // this object's lists of the chunk [cap][64], counts [cap]
    const float2* gw; const float4* grow; const float4* ray;  // {dL/dalpha, w} [cap][64] of this object; per ray {G_rgb, l}; the rays' rows
    float inv_n; float* partials;
    float* dbg;                                               // mon_debug_scene_pose_samples: [ray][64][14] x_o, x_c, t, raw, dL/dx, or nullptr
    const float* level_w;                                     // nullptr, or the level weights of this evaluation (the object reads its first L)
};
struct SceneCompGradArgs {
    uint32_t n_rays, n_lists, cap;
    const float* t; const float4* attr; const uint32_t* cnt;  // the lists, as launch_scene_composite takes them
    const float* mstar; const float4* ray;                    // m*_j [n_lists][cap]; per ray {c*, d*} {dn, M*, ..} {..}
    float w_rgb, w_mask, w_depth, huber;
    float2* gw; float4* grow; float* loss_part;               // outputs; loss_part[workgroup]
    float* out_W; float* out_D;                               // mon_debug_scene_composite_grad: W [n_lists][cap], D [cap], or nullptr
};
struct ScenePoseUpdateArgs {
    const float* partials; uint32_t n_objs, n_rows, row_stride;   // object j's rows at j * row_stride * 8
    const float* loss_part; uint32_t n_loss_parts;
    const SceneObjConst* objs; float inv_n; float* out; uint32_t it; int step; float lr_t, lr_r; float* pose; float* moments;
};
void launch_scene_pose_rays(hipStream_t s, const ScenePoseRayArgs& a);
void launch_scene_pose_obj(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ObjectConst& oc, const uint16_t* params, uint16_t* frag_image,
        int build_image, int backward, uint32_t grid, const ScenePoseObjArgs& p);
uint32_t scene_comp_grad_grid(uint32_t n_rays);
void launch_scene_composite_grad(hipStream_t s, const SceneCompGradArgs& a);
void launch_scene_pose_update(hipStream_t s, const ScenePoseUpdateArgs& a);
// Batched pose scoring (mon_scene_pose_loss_batch, kernels_scene_score.hip).  A pass holds G hypotheses of n_per rays as G * n_per virtual rays
// v = g * n_per + r in the lists of one evaluation (cap >= G * n_per): k_scene_score_rays (n_rays = G * n_per, pose = every hypothesis's Twc, 16 floats each;
// ray0 unused) -> per object k_scene_pose_obj<.., false, false> over the virtual rays -> k_scene_composite_loss (grid (scene_comp_grad_grid(n_per), G), one
// loss partial per workgroup, hypothesis-major) -> k_scene_loss_reduce (one workgroup per hypothesis, k_scene_pose_update's order, out[g] = loss).
constexpr uint32_t kSceneScoreMaxPoses = 4096, kRelocMaxKeep = 16, kSceneScoreMaxRays = 16384;      // (rays: the chunk cap of the chain; a hypothesis is never split)
struct SceneScoreRayArgs : ScenePoseRayArgs { uint32_t n_per, h0; };      // rays per hypothesis; the pass's first hypothesis
void launch_scene_score_rays(hipStream_t s, const SceneScoreRayArgs& a);
void launch_scene_composite_loss(hipStream_t s, const SceneCompGradArgs& a, uint32_t n_per);
void launch_scene_loss_reduce(hipStream_t s, const float* loss_part, uint32_t n_hyp, uint32_t n_parts, float inv_n, float* out);
// Window refinement (mon_scene_window_loss / mon_scene_refine_window, kernels_scene_window.hip + the window kernels of kernels_scene_pose.hip).  A pass
// packs whole frames as virtual rays v = v0_f + r into the list workspace of one evaluation, at most kWindowPassRays of them, greedily in window order.  One
// row of the device table per frame; per pass k_scene_window_rays -> per object k_scene_pose_obj<.., false, false> over the virtual rays ->
// k_scene_window_composite (grid (max parts_f, frames)) -> per object k_scene_window_obj (grid (max gridc_f, frames)); per evaluation k_scene_window_update.
constexpr uint32_t kWindowMaxFrames = 32, kWindowPassRays = 16384;
struct SceneWinFrame {
    uint32_t pose;                                            // offset of its Twc in the pose array (floats)
    uint32_t box0, n_box, prefix0, total;                     // its boxes, its own exclusive prefix sums (n_box + 1 entries at prefix0), its pixel total
    uint32_t v0, n_rays; float inv_n;                         // its first virtual ray in its pass, N_f, 1 / N_f
    uint32_t gridc, row0, parts, lp0;                         // a single-frame call's backward grid and loss partials; its first partial row / loss partial
};
struct SceneWindowRayArgs : ScenePoseRayArgs { const SceneWinFrame* frames; uint32_t n_frames; };   // the pass's rows; n_rays = its virtual rays; pose = every Twc
struct SceneWindowUpdateArgs {
    const float* partials; uint32_t n_objs, row_stride;       // object j's rows at j * row_stride * 8, frame f's from row0_f on
    const float* loss_part; const SceneWinFrame* frames; uint32_t n_frames, n_fixed; int refine_objs;
    SceneObjConst* objs; float* poses; float* moments;        // moments [n_frames + n_objs][12]: the cameras, then the objects
    float* out; uint32_t out_stride, it; int step;            // out[out_stride * it] = {L, L_f [F], grad6_f [F][6], obj_grad6_j [K][6]}
    float lr_t, lr_r, lr_obj_t, lr_obj_r;
};
void launch_scene_window_rays(hipStream_t s, const SceneWindowRayArgs& a);
void launch_scene_window_composite(hipStream_t s, const SceneCompGradArgs& a, uint32_t grid, uint32_t n_frames, const SceneWinFrame* frames);
void launch_scene_window_obj(hipStream_t s, const LevelFast& lt, const NetDims& nd, const ObjectConst& oc, const uint16_t* params,
        uint16_t* frag_image, uint32_t grid, uint32_t n_frames, const SceneWinFrame* frames, const ScenePoseObjArgs& p);
void launch_scene_window_update(hipStream_t s, const SceneWindowUpdateArgs& a);
// inference on feature-planar level tiles (kernels_tilerender.hip): Render / RenderVideo, GetDensityOnGrid, mesh vertex colours
constexpr uint32_t kTileChunkJobs = 32768;          // rays (jobs of 2S = 64 samples) per chunk of the tile render
bool tile_render_supported(const LevelTable& lt, const NetDims& nd);
void launch_build_feat_image(hipStream_t s, const LevelFast& lf, const NetDims& nd, const uint16_t* params, uint16_t* image, uint32_t* zero_counter);
void launch_forward_frag_image(hipStream_t s, const NetDims& nd, const uint16_t* params, uint16_t* image);
void launch_render_rays_jobs(hipStream_t s, const Intrinsics& K, const ObjectConst& oc, mon_frame_bbox box, const Mat4& pose, int pose_is_Toc, uint32_t n_pix,
                             float* rec, uint32_t* count, uint32_t* next_count, float* rgb, float* depth, float* mask);
void launch_render_points(hipStream_t s, const ObjectConst& oc, const float* rec, const uint32_t* count, uint32_t job_base, uint32_t jobs_cap, float* x,
        const RenderSkipArgs& skip = RenderSkipArgs{});
// the render's live-sample lists: partitions of k_encode_feat and the slots each needs for a chunk of `cap` samples
uint32_t render_list_parts();
uint32_t render_list_spw(uint32_t cap);
void launch_grid_points4(hipStream_t s, float* x, int rx, int ry, int rz, uint32_t p0, uint32_t n);
void launch_mesh_warp4(hipStream_t s, const float* verts, float* x, uint32_t v0, uint32_t n, const Aabb& box);
void launch_encode_feat(hipStream_t s, const LevelFast& lf, const NetDims& nd, const uint16_t* image, const float* x, uint16_t* e, uint32_t cap,
                        uint32_t n_host, const uint32_t* count, uint32_t job_base, uint32_t jobs_cap, uint32_t spj,
                        const RenderSkipArgs& skip = RenderSkipArgs{});
void launch_tile_render(hipStream_t s, const NetDims& nd, const ObjectConst& oc, const uint16_t* frag_image, const float* rec, const uint32_t* count,
                        uint32_t job_base, uint32_t jobs_cap, const float* x, const uint16_t* e, uint32_t cap, uint32_t n_pix, float* rgb, float* depth,
                                float* mask, const RenderSkipArgs& skip = RenderSkipArgs{});
void launch_tile_points_mlp(hipStream_t s, const NetDims& nd, const uint16_t* frag_image, const uint16_t* e, uint32_t cap, uint32_t n_points, uint16_t* O);
void launch_candidates_and_frags(hipStream_t s, const BatchPtrs& b, const DatasetPtrs& ds, const ObjectConst& oc, const DevState* st, const uint16_t* params,
        const NetDims& nd, uint16_t* frag_image);
int selftest_mfma(int device, const uint16_t* A, const uint16_t* B, float* D);

// ---- host classes
struct Dataset {
    int device = 0; Intrinsics K{}; uint32_t max_frames = 0, n_frames = 0; bool use_depth = false;
    uint32_t* d_rgba = nullptr; float* d_depth = nullptr; float* d_poses = nullptr;
    std::vector<uint8_t> present;      // present[id]: frame id has been uploaded (a new id lands in memory no kernel reads yet)
    // pinned staging of one incoming frame; the device's high-priority stream (model.cpp InferShared)
    uint8_t* h_stage = nullptr; size_t stage_bytes = 0; void* upload = nullptr;
    DatasetPtrs ptrs() const { return DatasetPtrs{ d_rgba, d_depth, d_poses, K }; }
};

struct MeshState;   // mesh.cpp
struct InferState;  // model_internal.h: inference stream, published weight snapshots and the render workspace of their own

// Render skipping (mon_object_set_render_skip) of one side: the train stream's renders (Model) or the snapshot renders (InferState, inference stream).
// Each side has its own grids: a viewer renders while the object trains, and training's occupancy grid (d_occ) is another thing altogether.
struct RenderSkipSide {
    uint32_t* d_grid = nullptr; uint32_t* d_raw = nullptr;      // [kOccWords] dilated / before dilation
    uint32_t* d_stats = nullptr; uint32_t* h_stats = nullptr;   // the last render's counters (RenderSkipArgs::stats) on the device / pinned on the host
    bool built = false, pinned = false;                         // a grid exists / it is a caller's (mon_debug_set_render_grid) and never rebuilt
    uint64_t epoch = 0; float alpha = 0.f;                      // the weights stamp and min_alpha the grid was built for
    uint64_t builds = 0; bool active = false; uint64_t samples_in_box = 0, samples_live = 0;
};

// What an object's shape, config and the options at its creation allow: which buffers model_init allocates and therefore which training chains the enqueue
// code (train.cpp) CAN run.  Filled once by train_plan (model.cpp), a pure function; never changes.  What one iteration then takes among these is decided
// per enqueued iteration (step_choice, train.cpp).
struct PlanOptions { long backend, lds_encode; uint32_t big_switch; };      // the option values read at creation
struct TrainPlan {
    bool fused;             // the shape is one the fused kernels take (fused_supported); else the layer-at-a-time kernels, backend 0 by necessity
    bool fused_backend;     // ... and option backend did not ask for the layer-at-a-time kernels: the backend the object starts on, its inference on the fused kernels
    uint32_t lds_mask;      // fused: the levels k_grid_scatter covers (a prefix; d_de_soa, d_x_soa, d_gpart)
    bool lds_all;           // ... every level: the dense optimizer
    bool big_scatter;       // fused: levels beyond the LDS plan go through kernels_bigscatter.hip (d_big_ws, Model::big_switch)
    bool touched_flags;     // fused: chunk flags for the lazy optimizer (d_touched)
    bool level_tiles;       // level-tile encode (d_x_all, d_e_soa, d_half_tiles; fused: also B_alt, the second candidate set)
    // not fused: T-layout workspace of the MFMA layer kernels (kernels_layers.hip; d_layers_T) -- without it kernels_net.hip's one-sample-per-thread kernels run
    bool layer_ws;
    // not fused (the layer-at-a-time kernels), every level in the LDS plan: the grid backward of whole training steps goes through k_grid_scatter (d_de_soa,
    // d_x_soa, d_gpart)
    bool hybrid_scatter;
    bool occupancy;         // fused + cfg.occupancy_skip: the occupancy grid (d_occ, d_occ_tmp, d_frag_occ)
    // ... and, for the level-tile chain with the grid in use, live-sample lists for k_encode_tiles (LiveArgs; d_live_idx, d_live_cnt): a position block's 256
    // samples must lie in one of the encode's sample partitions, and a list -- at most ceil(blocks / n_parts) * 256 entries -- must fit the partition's spw slots
    bool live_lists;
    bool xorwow;            // the reference's XORWOW sample stream (d_xw*)
    bool lazy_ema;          // tables above 8 M parameters: the lazy optimizer and EMA (d_ema_step or chunk records)
    bool tile_render;       // the inference side may run on feature-planar level tiles (tile_render_supported)
    // published snapshots and a render workspace of their own (InferState).  Not in the XORWOW mode (one generator per Render, like the reference) nor for
    // tables above 8 M parameters (lazy EMA; 2 x 200 MB of snapshots): those render on the train stream
    bool inference_side;
};
TrainPlan train_plan(const mon_config& cfg, const LevelTable& lt, const NetDims& nd, uint32_t R, uint32_t S, bool lazy_ema, const PlanOptions& opt);

struct Model {
    TrainPlan plan{};
    MeshState* mesh = nullptr;
    InferState* infer = nullptr;                // mpInferenceStream (nerf_model.cu:1269): renders for viewers that never queue behind training
    Dataset* ds = nullptr; mon_config cfg{}; int device = 0;
    LevelTable lt{}; LevelFast lf{}; NetDims nd{}; ObjectConst oc{}; OptimConst opt{};
    uint32_t n_grid = 0, n_params = 0;
    hipStream_t train_stream = nullptr;      // mpTrainStream :1268; inference (render, mesh) runs on the same stream: the reference's mpInferenceStream is only
                                             // ever used from the object's own thread between training calls
    // level-tile encode: the second candidate set (cand_*, mask differ from B; everything else is shared); B and B_alt swap with the DevStates
    BatchPtrs B_alt{};
    // iteration i runs on one DevState and prepares the other for i + 1 (k_optimizer); swapped when an optimizer step is enqueued
    ParamPtrs P{}; BatchPtrs B{}; DevState* d_state = nullptr; DevState* d_state_next = nullptr;
    mon_frame_bbox* d_boxes = nullptr;
    uint32_t boxes_cap = 0, n_boxes = 0; uint32_t ws_samples = 0, ws_rays = 0;
    // fused backend
    // [512][fused_partial_cols + 64] fp32 dW partial rows of k_fused_train, accumulator layout (frag_layout.h acc_param)
    float* d_dw_partials = nullptr;
    uint16_t* d_de_soa = nullptr; float* d_x_soa = nullptr;       // compacted dL/dE rows [L][B] and positions [B] float4 for the scatter kernels
    // level-tile encode: positions [B] float4 of every sample, encoded features [L][B] half2 (nullptr: the fused kernel gathers)
    float* d_x_all = nullptr; uint16_t* d_e_soa = nullptr; uint16_t* d_half_tiles = nullptr;
    bool b0_tiles_current = false;            // layer-kernel shapes on the level-tile encode: the tile image matches the fp16 weights (k_optimizer keeps it so in whole steps)
    uint16_t* d_layers_T = nullptr;          // T-layout workspace of the MFMA layer kernels (shapes outside the fused kernels)
    uint16_t* d_gpart = nullptr; ScatterLevels scatter{};   // k_grid_scatter: partial tables, plan (the levels it covers: plan.lds_mask)
    // halves of ONE partial table: the grid parameters of the LDS-scattered levels (a prefix of the levels), not of the whole table
    uint32_t part_halves = 0;
    uint16_t* d_frag_train = nullptr; uint16_t* d_frag_render = nullptr;           // MFMA A-fragment images (training weights / inference weights)
    uint32_t n_bins = 16;                                         // ray bins of the compacted gradient rows (scatter_bins(R) unless the option caps it)
    uint32_t* d_ema_step = nullptr; uint8_t* d_touched = nullptr;                  // lazy EMA bookkeeping, chunk flags (ParamPtrs)
    // kernels_bigscatter.hip: workspace, switch point, launched in this train call
    uint8_t* d_big_ws = nullptr; uint32_t big_switch = 0; bool big_active = false;
    // occupancy grid (cfg.occupancy_skip)
    uint32_t *d_occ = nullptr, *d_occ_tmp = nullptr; uint16_t* d_frag_occ = nullptr; float occ_raw_threshold = 0.f;
    uint32_t occ_refreshed_iter = 0, occ_next_refresh = 0;
    bool occ_pinned = false;                                    // a caller's grid (mon_debug_set_train_occupancy): no scheduled refreshes
    uint32_t *d_live_idx = nullptr, *d_live_cnt = nullptr;      // live-sample lists of the level-tile chain (LiveArgs)
    // whole-crop render outputs: ONE grow-only buffer, rgb | depth | mask of the current crop back to back
    float *d_out_all = nullptr, *d_out_rgb = nullptr, *d_out_depth = nullptr, *d_out_mask = nullptr; size_t out_cap = 0;
    // pinned staging of a crop on its way to the caller's (pageable) buffers
    float* h_out = nullptr; size_t h_out_cap = 0;
    std::vector<void*> allocs;
    DevState h_state{}; DevState* h_state_pinned = nullptr; int backend = 0; bool profiling = false; int fused_dump = 0;
    bool ema_pending = false;   // large tables (plan.lazy_ema): EMA of untouched chunks is brought up to date on demand (k_ema_finalize)
    bool scatter_pending = false;   // a fused forward/backward was enqueued whose slot counter has not been reset by an optimizer step yet
    // XORWOW sample stream: lane states of the training generator (device), the two per-parity array sets, the iteration the fills have reached, the per-Render
    // generator xw_offset: values the training generator has produced
    void* d_xw_states = nullptr; float* d_xw = nullptr; uint32_t xw_filled = 0, xw_lanes = 0; int xw_flavour = 0; uint32_t enq_iter = 0; uint64_t xw_offset = 0;
    void* d_xw_render_states = nullptr; void* d_xw_render_init = nullptr; float* d_xw_render = nullptr; size_t xw_render_cap = 0;
    // NeRF_Model::Step schedule (option step_variant): per-ray sample counts / slots, the compacted positions
    uint32_t* d_step_counts = nullptr; float* d_step_pts = nullptr;
    // level-tile encode: used by the iteration being enqueued / the next batch's positions were written by the last k_optimizer / this train call runs the
    // gather chain (occupancy grid + few live samples)
    bool pre_active = false, points_ready = false, gathers_preferred = false;
    bool tile_counted = false;   // this object is counted in its device's tile workspace (freed with the device's last such object)
    std::atomic<int> rskip_on{ 0 }; std::atomic<float> rskip_alpha{ 1e-3f };      // render skipping: the switch (read once per render call)
    RenderSkipSide rskip;                                                             // ... and its train-stream side
    struct PoseWs* pose_ws[2] = { nullptr, nullptr };                                // pose refinement scratch per side (pose.cpp), made on first use 
    uint64_t weights_epoch = 0;  // process-wide unique stamp of the weights' current content (a new one after every train call / set_params / EMA catch-up):
                                 // the tile render's per-device workspace keeps its tile image while the stamp it was built for is current
    bool next_ready = false;     // fused backend: candidates + fragment image of the coming iteration were already produced by the last k_optimizer
    mon_profile prof{}; std::vector<hipEvent_t> ev_pool; std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_pending;
    // per-device training lanes (model.cpp): the lane and completion event of this object's last chunk
    struct TrainLanes* lanes = nullptr; int lane = -1; hipEvent_t lane_event = nullptr, switch_event = nullptr, sync_event = nullptr;
    // the object's private stream; train_stream is the one its work currently goes to (this one or a lane's)
    bool tail_marked = false; hipStream_t own_stream = nullptr;
    // (the state the captured pair of iterations starts on)
    hipGraphExec_t graph_exec = nullptr; int graph_backend = -1; const DevState* graph_state = nullptr; const void* graph_mask = nullptr;
};

// ---- the model layer's entry points (model.cpp, train.cpp, mesh.cpp, config.cpp, diag.cpp), as c_api.cpp, manager.cpp and diag.cpp call them
void set_error(const char* fmt, ...);      // the calling thread's mon_last_error text
const char* last_error();
int device_count(int* n);
int physical_device(int logical, int* phys_out);
void config_default(mon_config& c);
int config_from_json(const char* path, mon_config& c);
int stream_pool_reserve(int device, int n);
int dataset_create(int device, int H, int W, float fx, float fy, float cx, float cy, uint32_t max_frames, int use_depth, Dataset** out);
int dataset_add_frame(Dataset* d, uint32_t id, const uint8_t* rgb, int ch, int is_bgr, const uint8_t* inst, const float* depth, const float* Twc);
int dataset_update_poses(Dataset* d, uint32_t first, uint32_t n, const float* Twc16s);
int dataset_destroy(Dataset* d);
int model_create(Dataset* ds, const mon_config& cfg, int class_id, const float* Tow, const float* amin, const float* amax, Model** out);
int model_destroy(Model* m);
int model_add_boxes(Model& m, const mon_frame_bbox* boxes, size_t n);
int model_train(Model& m, int iters, float* loss, int stages);
int model_render(Model& m, mon_frame_bbox box, const float* pose16, int pose_is_Toc, float* rgb, float* depth, float* mask, int dst_on_device);
int model_density_grid(Model& m, int rx, int ry, int rz, float* out_host);
int model_get_params(Model& m, int which, void* dst, size_t bytes);
int model_set_params(Model& m, const float* master, size_t n);
int model_set_backend(Model& m, int backend);
int model_set_debug_dump(Model& m, int enable);
int model_debug_read(Model& m, int which, void* dst, size_t bytes);
int model_generate_mesh(Model& m, int res, float thresh, uint32_t* n_verts, uint32_t* n_indices);
int model_mesh_counts(Model& m, uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices);
int model_get_mesh(Model& m, float* verts, float* normals, uint8_t* colors, uint32_t* indices, float* normals_raw, float* colors_f32, int try_only);
int model_save_mesh(Model& m, const char* path);
int model_mesh_generation(Model& m, uint64_t* gen);
int model_copy_mesh(Model& m, uint32_t cap_verts, uint32_t cap_indices, float* verts, float* normals, uint8_t* colors, uint32_t* indices,
                    uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices, int try_only);
int marching_cubes_host(int device, const float* density, int rx, int ry, int rz, float thresh, const float* amin, const float* amax,
                        float* verts, float* normals_raw, uint32_t* indices, uint32_t cap_verts, uint32_t cap_indices, uint32_t* n_verts,
                                uint32_t* n_verts_real, uint32_t* n_indices);
int microbench(int device, int mode, int pattern, uint32_t n_entries, uint32_t n_ops, float* ms_out);
// What was prepared ahead of the next iteration goes stale for one of three reasons (train.cpp, where the flags live); graph_too: a captured pair of
// iterations goes as well
enum : unsigned { kStaleRays = 1u, kStaleWeights = 2u, kStaleOccupancy = 4u };
void model_mark_stale(Model& m, unsigned why, bool graph_too = false);
int ensure_ema_current(Model& m);
uint64_t next_weights_epoch();
int model_set_render_skip(Model& m, int enable, float min_alpha);
int model_render_skip_stats(Model& m, int side, mon_render_skip_stats* out);
int model_render_occupancy(Model& m, int side, int dilated, uint32_t* bits);
int model_debug_set_render_grid(Model& m, int side, const uint32_t* bits);
// Per-device workspace of the tile render, shared by the objects on the device; `side` 0: train-stream users (model_render, density lattice, mesh), 1: the
// inference stream.  A user holds `mu` from its first launch until its stream is synchronised.
struct TileWs {
    std::mutex mu;
    float* rec = nullptr; size_t rec_cap = 0;                   // job records of a crop: 12 floats per pixel
    uint32_t* counters = nullptr; uint32_t flip = 0;            // two job counters, used by alternate render calls (a call's ray kernel clears the next call's)
    float* x = nullptr; uint16_t* e = nullptr; uint16_t* O = nullptr; uint32_t cap = 0; int L_cap = 0;      // chunk buffers: positions, features, raw outputs
    uint16_t* image = nullptr; size_t image_cap = 0; uint16_t* frag = nullptr;      // feature-planar tile image + forward A fragments of the weights in use
    const void* key_params = nullptr; uint64_t key_epoch = ~0ull;
    // render skipping (RenderSkipArgs): two live words per job slot, the partitions' live-sample lists of one chunk, their counters for every chunk of a crop
    uint32_t *job_bits = nullptr, *live_idx = nullptr, *live_cnt = nullptr; size_t job_bits_cap = 0, live_cnt_cap = 0;
};
int tile_ws_get(Model& m, int side, size_t n_pix, TileWs** out);
// render skipping on the tile path: each job's live bits and the live-sample lists of a crop of n_pix pixels (caller holds ws.mu)
int tile_ws_skip_buffers(TileWs& ws, size_t n_pix);
// the weights `prm` (stamp `epoch`) as tile image + fragments in `ws` (rebuilt only when the stamp changed); caller holds ws.mu
void tile_ws_weights(Model& m, TileWs& ws, hipStream_t s, const uint16_t* prm, uint64_t epoch);
// ws.x holds n points -> ws.O (raw fp16 outputs [n][4]); caller holds ws.mu and has called tile_ws_weights
void tile_points_forward(Model& m, TileWs& ws, hipStream_t s, uint32_t n);
// ---- The boundary of the scene and pose routes.  Every entry to a route -- the C ABI, the online manager, a dump entry of the diagnostics
// library -- takes four steps: the route's <route>_check (every MON_ERR_ARG that can be judged without an object), the objects (scene_models from the
// caller's handles, the manager's pick), the route's <route>_objects_check (every MON_ERR_ARG that needs them), the route.  A schedule's pose_c2f_check is a
// call of its own: after the objects' check in the C ABI, before the manager picks its objects.  None of them does device work, and a route repeats none of
// them; its MON_ERR_STATE cases (an object outside the fused kernels, nothing published on side 1) are the route's own.
// scene_models: handles to models; MON_ERR_ARG for a NULL list, a count outside 1..kSceneMaxLists, a NULL element.  `what`: the message prefix.
int scene_models(const char* what, mon_object* const* objs, size_t n, std::vector<Model*>& ms);
// the objects of one call: the count again (the manager's lists come without handles), one device, one camera (not the ray cast), one dataset (the pose
// routes, which read a frame's pixels)
int scene_objects_check(const char* what, Model* const* ms, size_t n, bool camera = true, bool one_dataset = false);
// Lmax = the largest n_levels among the objects (the row length of their level weights) and, with a schedule, its table [iters][Lmax] (w(): nullptr without)
struct SceneLevels { int Lmax = 0; std::vector<float> table; const float* w() const { return table.empty() ? nullptr : table.data(); } };
SceneLevels scene_levels(Model* const* ms, size_t n, const mon_pose_c2f_params* c = nullptr, int iters = 0);
int level_weights_check(const char* what, const float* w, int n);                                 // n finite weights >= 0
// an in-out pose: `run` refines a copy of it in place, which goes back to the caller only when it succeeds
template <class F> int pose_inout(float* pose16, F run) {
    float pose[16]; std::memcpy(pose, pose16, 64);
    const int rc = run(pose);
    if (rc == MON_OK) std::memcpy(pose16, pose, 64);
    return rc;
}
// Scene render (mon_scene_render): side 0 the train-side weights, 1 the published snapshots; ids (may be nullptr) = the instance reported for each object;
// dump (mon_debug_scene_samples, may be nullptr) = object `list`'s sample lists of the whole rect, host arrays [pixel][kSceneListLen] (rgb x 3) + count [pixel]
struct SceneDump { uint32_t list; float* t; float* alpha; float* rgb; uint32_t* count; };
int scene_render_check(int side, mon_frame_bbox rect, const float* Twc16);      // the view; the caller's image and depth: scene_render_outputs_check
int scene_render_outputs_check(const float* rgb, const float* depth);
int scene_render(Model* const* ms, size_t n, int side, mon_frame_bbox rect, const float* Twc16, float* rgb, float* depth, float* opacity, int32_t* instance,
                 const int32_t* ids, const SceneDump* dump);
// Scene probe (mon_scene_probe): scene_render's conventions for side and ids (applied to both instance outputs).  dump (mon_debug_scene_probe_rays /
// mon_debug_scene_cast_rays, may be nullptr) = object k's ray rows per query, host array [n_q][10]: o[3], d[3], t0, t1, flag, dn (a row that missed the
// box: flag 0, dn, the rest 0); entry (the cast only) = its entry row [n_q].
struct SceneRaysDump { uint32_t k; float* rows; float* entry; };
int scene_probe_check(int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q, const float* rgb, const float* depth);
int scene_probe(Model* const* ms, size_t n, int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q, float* rgb, float* depth,
                float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance, const int32_t* ids, const SceneRaysDump* dump);
// Ray cast (mon_scene_cast): the probe's chain over world rays; the same conventions (its objects' check: no camera).
// scene_camera_rays (mon_camera_rays): the probe's world rays on the host, pixel_ray's world-frame branch.
int scene_cast_check(int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* rgb, const float* dist);
int scene_cast(Model* const* ms, size_t n, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, float* rgb, float* dist, float* opacity,
               int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance, const int32_t* ids, const SceneRaysDump* dump);
int scene_camera_rays(float fx, float fy, float cx, float cy, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                      mon_scene_ray* rays_out, float* dn_out);
// Point queries (mon_scene_query_points / mon_scene_query_lattice): the objects' check is the cast's (no camera); ids as scene_render's, applied to owner.
// ScenePoints: xyz = the world points [n][3], or nullptr: the lattice g (n = its points).  rows (mon_debug_scene_point_rows, may be
// nullptr) = object rows_k's rows of every point, host array [n][12].  scene_lattice_points (mon_lattice_points): the lattice's floats on the host.
// object_points (mon_object_query_points): the same kernel on unit-cube points of one object, its raw outputs [n][4].
struct ScenePoints { const float* xyz; size_t n; Lattice g; };
inline ScenePoints scene_point_list(const float* xyz, size_t n) { return { xyz, n, Lattice() }; }
inline ScenePoints scene_lattice(const float* origin3, const float* step3, int nx, int ny, int nz) { const Lattice g(origin3, step3, nx, ny, nz); return { nullptr, g.n(), g }; }
int scene_points_check(int side, const float* xyz, size_t n, const float* sigma);
int scene_lattice_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, const float* sigma);
int scene_points(Model* const* ms, size_t n, int side, const ScenePoints& q, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside,
                 const int32_t* ids, size_t rows_k, float* rows);
int scene_lattice_points(const float* origin3, const float* step3, int nx, int ny, int nz, float* xyz_out);
int object_points_check(int side, const float* unit_xyz, size_t n, const float* raw4);
int object_points(Model& m, int side, const float* unit_xyz, size_t n, float* raw4);
// Distance fields (mon_distance_transform, mon_scene_distance_lattice): distance_transform = the three passes and the finish on a host mask, in buffers
// of its own (MON_ERR_NO_DEVICE without a device, after its check).  scene_distance = the lattice query (q: scene_lattice's; the same objects' check and
// MON_ERR_STATE cases) with the mask !(sigma <= sigma_min), the transform and, with free_dist, the complement's transform behind it on the device; every
// output but dist may be nullptr; ids as scene_points', applied to nearest_owner.
int distance_transform_check(const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, const float* dist);
int distance_transform(int device, const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist, float* dist, int32_t* nearest);
int scene_distance_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist, const float* dist);
int scene_distance(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float max_dist, float* dist, int32_t* nearest,
                   int32_t* nearest_owner, float* free_dist, float* sigma, const int32_t* ids);
// Signed, sub-cell distance fields (mon_signed_distance_transform, mon_scene_signed_distance_lattice, mon_scene_signed_dist_field):
// signed_distance_transform = the nine passes and the finish on host values, in buffers of its own.  scene_signed_distance = the lattice query, the
// values (flags & MON_SIGNED_LOG: in log density) and the transform behind it on the device; every output but sdist may be nullptr; ids as scene_points',
// applied to nearest_owner.  scene_signed_dist_field keeps sdist in a handle (dist_field.cpp): nothing per cell goes home.
int signed_distance_transform_check(const float* val, float iso, int nx, int ny, int nz, const float* step3, float max_dist, const float* sdist);
int signed_distance_transform(int device, const float* val, float iso, int nx, int ny, int nz, const float* step3, float max_dist, float* sdist,
                              int32_t* nearest_edge);
int scene_signed_distance_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, uint32_t flags, float max_dist,
                                const float* sdist);
int scene_signed_distance(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, uint32_t flags, float max_dist, float* sdist,
                          int32_t* nearest_edge, int32_t* nearest_owner, float* sigma, float* val, float* iso_out, const int32_t* ids);
struct DistField;
int scene_signed_dist_field_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, uint32_t flags, float max_dist,
                                  const void* field_out);
int scene_signed_dist_field(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, uint32_t flags, float max_dist, DistField** out);
// Connected components (mon_label_components, mon_scene_components_lattice): label_components = the labelling of a host mask in buffers of its own
// (MON_ERR_NO_DEVICE without a device, after its check).  scene_components = the lattice query with the mask !(sigma <= sigma_min) (region 0) or, behind
// the untruncated distance transform of that mask, dist > clearance (region 1), and the labelling behind it on the device; every output but label may
// be nullptr (table needs n_components; dist: region 1 only); ids as scene_points', applied to owner.  A device loop that ran into its cap: MON_ERR_STATE.
int label_components_check(const uint8_t* mask, int nx, int ny, int nz, int connectivity, const int32_t* label, const mon_lattice_component* table,
                           const uint32_t* n_components);
int label_components(int device, const uint8_t* mask, int nx, int ny, int nz, int connectivity, int32_t* label, int32_t* comp, mon_lattice_component* table,
                     uint32_t cap, uint32_t* n_components);
int scene_components_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, int region, float clearance,
                           int connectivity, const int32_t* label, const mon_lattice_component* table, const uint32_t* n_components, const float* dist);
int scene_components(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, int region, float clearance, int connectivity,
                     int32_t* label, int32_t* comp, mon_lattice_component* table, uint32_t cap, uint32_t* n_components, float* dist, float* sigma,
                     int32_t* owner, const int32_t* ids);
// Shortest-path cost fields (mon_shortest_paths, mon_scene_paths_lattice, mon_lattice_path): shortest_paths = the field of a host mask in buffers of its own
// (MON_ERR_NO_DEVICE without a device, after its check).  scene_paths = the lattice query, the untruncated distance transform of !(sigma <= sigma_min), the
// mask dist > clearance, the multiplier (soft_weight > 0) and the field behind them on the device; every output but cost may be nullptr; ids as
// scene_points', applied to owner.  The sweeps are enqueued in batches of kPathsBatch with one 4-byte read-back each; more than n + 1 sweeps: MON_ERR_STATE.
// paths_last_stats: { sweeps enqueued, batches, sweeps that left work } of the process's latest field (mon_debug_paths_stats).  lattice_path: the walk
// along next, on the host.
int shortest_paths_check(const uint8_t* passable, int nx, int ny, int nz, const float* step3, int connectivity, const float* cell_cost, const int32_t* seeds,
                         size_t n_seeds, float max_cost, const float* cost);
int shortest_paths(int device, const uint8_t* passable, int nx, int ny, int nz, const float* step3, int connectivity, const float* cell_cost,
                   const int32_t* seeds, size_t n_seeds, float max_cost, float* cost, int32_t* next);
int scene_paths_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float clearance, float soft_radius,
                      float soft_weight, int connectivity, const int32_t* seeds, size_t n_seeds, float max_cost, const float* cost);
int scene_paths(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float clearance, float soft_radius, float soft_weight,
                int connectivity, const int32_t* seeds, size_t n_seeds, float max_cost, float* cost, int32_t* next, float* dist, float* sigma, int32_t* owner,
                const int32_t* ids);
void paths_last_stats(uint32_t out3[3]);
int lattice_path(const int32_t* next, size_t n_cells, int32_t start, int32_t* path, size_t cap, size_t* n_path);
// Device-resident distance fields (mon_dist_field_*; dist_field.cpp): a snapshot of a field in device memory of its own, asked at world points and along
// trajectories (the rule: include/mon_core.h).  DistField holds no reference to objects or to a manager; calls on one handle take turns on its mutex.
// The *_check judge what needs no device; dist_field_create uploads a host field; scene_dist_field runs scene_distance's chain (scene_field.cpp) and keeps
// dist on the device: nothing per cell goes home.  Every output of dist_field_score but min_clear may be nullptr, dist_field_sample's grad3 too.
struct DistField;
int dist_field_create_check(const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, const void* field_out);
int dist_field_create(int device, const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, DistField** out);
int scene_dist_field_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist, const void* field_out);
int scene_dist_field(Model* const* ms, size_t n, int side, const ScenePoints& q, float sigma_min, float max_dist, DistField** out);
int dist_field_adopt(int device, const Lattice& g, DistField** out);          // scene_field.cpp's way in: the handle with its buffer, still empty
void dist_field_free(DistField* f);
int dist_field_info(DistField* f, mon_dist_field_desc* info);
int dist_field_read(DistField* f, float* dist_out);
int dist_field_sample(DistField* f, const float* xyz, size_t n, float outside, float* dist_out, float* grad3_out);
int dist_field_score(DistField* f, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj, size_t n_way, size_t n_sub,
                     const mon_traj_score_params* p, float* min_clear, int32_t* first_hit, float* cost, float* way_clear, float* way_grad);
// Scan matching (dist_field.cpp; the rule: include/mon_core.h).  dist_field_match: cost and, where asked for, the counts and the normal equations of n points
// under H poses.  dist_field_register: every hypothesis refined by Levenberg-Marquardt in lockstep, one match launch and one read-back of 32 words per pose
// and round; the 6 x 6 solves and the pose updates are the host's, in double.
int dist_field_match(DistField* f, const float* points, size_t n, const float* poses16, size_t n_pose, const float* pivots, const mon_scan_match_params* p,
                     float* cost, int32_t* n_inside, int32_t* n_inlier, float* normal);
int dist_field_register_default(DistField* f, mon_register_params* p);
int dist_field_register(DistField* f, const float* points, size_t n, const float* poses16_in, size_t n_pose, const mon_register_params* p, float* poses16_out,
                        float* cost, int32_t* n_inside, int32_t* n_inlier, int32_t* evals, int32_t* status, int32_t* best);
// Ray tracing (dist_field.cpp; the rule: include/mon_core.h).  dist_field_trace: range and, where asked for, status, steps and the normal at the hit of n rays
// under H poses ([H][n]; poses16 nullptr: world rays, H == 1).  dist_field_beam_score: per pose the Huber cost of range - measured over the beams and the two
// counts, the ranges staying on the device.  One upload, the launches, one copy home and one synchronisation each.
int dist_field_trace_default(DistField* f, mon_trace_params* p);
int dist_field_trace(DistField* f, const float* rays, size_t n, const float* poses16, size_t n_pose, const mon_trace_params* p, float* range, int32_t* status,
                     int32_t* steps, float* normal3);
int dist_field_beam_score(DistField* f, const float* rays, size_t n, const float* measured, const float* poses16, size_t n_pose, const mon_trace_params* p,
                          const mon_beam_params* b, float* cost, int32_t* n_valid, int32_t* n_hit);
// Point gradients (mon_scene_query_gradients / _lattice_gradients, mon_object_query_gradients): the point queries' conventions, plus level_w (host, may be
// nullptr = all 1: Lmax floats, object j reads its first L_j; the *_check judges the first, scene_gradients_weights_check the rest once the objects are
// known) and select (host, [n] or nullptr: -1 or an index into ms).  rows (mon_debug_scene_gradient_rows) = object rows_k's rows, host array [n][16].
// scene_cast_normals (mon_scene_cast_normals): scene_cast, then scene_gradients at the hit points with select = the hit object; ids applied at the end.
int scene_gradients_check(int side, const float* xyz, size_t n, const float* level_w, const int32_t* select, size_t n_objs, const float* sigma,
                          const float* grad_log);
int scene_lattice_gradients_check(int side, const float* origin3, const float* step3, int nx, int ny, int nz, const float* level_w, const float* sigma,
                                  const float* grad_log);
int scene_gradients_weights_check(Model* const* ms, size_t n, const float* level_w);
int scene_gradients(Model* const* ms, size_t n, int side, const ScenePoints& q, const float* level_w, const int32_t* select, float* sigma, float* rgb,
                    int32_t* owner, float* owner_sigma, uint32_t* n_inside, float* grad_log, float* grad_sigma, float* normal, const int32_t* ids,
                    size_t rows_k, float* rows);
int object_gradients_check(int side, const float* unit_xyz, size_t n, const float* level_w, const float* grad_unit);
int object_gradients(Model& m, int side, const float* unit_xyz, size_t n, const float* level_w, float* raw4, float* grad_unit);
int scene_cast_normals_check(int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* level_w, const float* rgb, const float* dist,
                             const float* normal);
int scene_cast_normals(Model* const* ms, size_t n, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* level_w, float* rgb,
                       float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance, float* hit_xyz, float* normal,
                       float* grad_log, const int32_t* ids);
bool model_has_snapshot(Model& m);      // the object has an inference side and has published weights
// Pose refinement: iters < 0 = one evaluation (mon_object_pose_loss: loss, grad6, jitter / draws of `iteration`), else iters Adam steps from Tow16
// (mon_object_refine_pose: the final pose into pose_out, loss_trace[iters + 1] may be nullptr).  dump (mon_debug_pose_samples, may be nullptr): per drawn ray
// of the evaluation, host arrays [ray][2S] of positions (object frame, 3), raw outputs (4) and dL/dx (3); any of them may be nullptr.
// level_w (mon_object_pose_loss_levels / mon_object_refine_pose_c2f, may be nullptr): host weights [L] of the one evaluation, or [iters][L] of the steps.
struct PoseDump { float* x; float* raw; float* dldx; };
int pose_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p);     // (the boxes are the object's part)
int pose_refine(Model& m, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params& p, int iters,
                uint32_t iteration, float* pose_out, float* loss_trace, float* loss, float* grad6, const PoseDump* dump, const float* level_w = nullptr);
// Camera refinement against a scene of objects (mon_scene_pose_loss / mon_scene_refine_camera): pose_refine's conventions for iters, iteration, the outputs
// and level_w (rows of Lmax = the largest n_levels among the objects; object j reads its first L_j).  dump (mon_debug_scene_pose_samples, may be nullptr):
// object k's share per drawn ray, host arrays [ray][64][3 | 3 | 1 | 4 | 3] + count [ray].
struct ScenePoseDump { uint32_t k; float* x_o; float* x_c; float* t; float* raw; float* dldx; uint32_t* count; };
int scene_pose_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16, const mon_pose_refine_params* p);
int scene_pose_objects_check(Model* const* ms, size_t n, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p);
int scene_pose(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16, const mon_pose_refine_params& p, int iters,
               uint32_t iteration, float* pose_out, float* loss_trace, float* loss, float* grad6, const ScenePoseDump* dump, const float* level_w = nullptr);
uint32_t pose_n_rays(const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params& p);      // rays of one evaluation
// mon_scene_pose_loss_batch: losses[h] = scene_pose(.., Twc16s + 16 h, p, -1, iteration, ..)'s loss bit for bit, all in one enqueue with one synchronisation.
// The checks: scene_pose's, n_poses outside 1..kSceneScoreMaxPoses, more than kSceneScoreMaxRays rays per hypothesis.
int scene_pose_batch_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, size_t n_poses, const mon_pose_refine_params* p,
                           const float* losses);
int scene_pose_batch_objects_check(Model* const* ms, size_t n, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p);
int scene_pose_batch(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, size_t n_poses,
                     const mon_pose_refine_params& p, uint32_t iteration, float* losses);
// mon_scene_window_loss / mon_scene_refine_window (include/mon_core.h): iters < 0 = one evaluation at `iteration` (wp may be nullptr; level_w one row of
// Lmax or nullptr), else iters steps (level_w [iters][Lmax] or nullptr).  Tow16s nullptr = every object's own Tow.  Outputs may be nullptr; Twc16s_out /
// Tow16s_out receive only the poses that moved.  window_frames: mon_window_frames.  scene_window_objects_check: every frame's boxes as scene_pose takes
// them, the rays of a frame, a non-finite Tow16s.  model_set_pose: mon_object_set_pose.
int window_frames(const mon_frame_bbox* obs, size_t n_obs, uint32_t* frame_ids, size_t* n_frames);
int scene_window_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, const mon_pose_refine_params* p, const mon_window_params* w,
                       const float* Tow16s, bool refine);
int scene_window_objects_check(Model* const* ms, size_t n, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16s, const mon_pose_refine_params* p);
int scene_window(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s, const float* Tow16s,
                 const mon_pose_refine_params& p, const mon_window_params* wp, int iters, uint32_t iteration, const float* level_w, float* Twc16s_out,
                 float* Tow16s_out, float* loss_trace, float* frame_trace, float* loss, float* frame_loss, float* cam_grad6, float* obj_grad6);
int model_set_pose(Model& m, const float* Tow16);
// mon_scene_relocalise / mon_online_relocalise: the rule of include/mon_core.h over scene_pose_batch and scene_pose.  Its objects' check is
// scene_pose_objects_check; level_w: the table of the schedule every kept candidate is refined under (scene_levels), or nullptr.
int scene_reloc_check(int side, const mon_frame_bbox* obs, size_t n_obs, const float* cands, size_t n_cands, const mon_pose_refine_params* p,
                      const mon_reloc_params* r, const float* pose_out);
int scene_relocalise(Model* const* ms, size_t n, int side, const mon_frame_bbox* obs, size_t n_obs, const float* cands, size_t n_cands,
                     const mon_pose_refine_params& p, const float* level_w, const mon_reloc_params& r, float* pose_out, mon_reloc_result* result,
                     float* scores);
int pose_c2f_check(const mon_pose_c2f_params* c);                                                    // MON_ERR_ARG for a NULL or bad schedule
std::vector<float> pose_c2f_table(const mon_pose_c2f_params& c, int n_levels, int iters);          // [iters][n_levels]: mon_pose_c2f_weights of every step
// Checkpoints (mon_object_save / mon_object_load / mon_checkpoint_read_info).  boxes_out (may be nullptr): the box list the file holds,
// whether or not it was restored (the online manager's bookkeeping).
int checkpoint_read_info(const char* path, int verify, mon_checkpoint_info* out);
int model_save(Model& m, const char* path);
int model_load(Dataset* ds, const char* path, uint32_t flags, Model** out, std::vector<mon_frame_bbox>* boxes_out = nullptr);
// HIP-event time of the pack / unpack kernels of the calling thread's saves and loads (tools/checkpoint_timing.py through the diagnostics library):
// enable != 0 starts collecting (each kernel bracketed by events), *kernel_ms = the sum since the last call, then cleared
int checkpoint_timing(int enable, double* kernel_ms);
int model_publish_snapshot(Model& m);
int model_render_snapshot(Model& m, mon_frame_bbox box, const float* pose16, int pose_is_Toc, float* rgb, float* depth, float* mask, uint32_t* snapshot_step);
int level_table_build(const mon_config& c, LevelTable& lt, NetDims& nd, uint32_t& n_grid);
void level_fast_build(const LevelTable& lt, const NetDims& nd, LevelFast& lf);
void init_params_host(const mon_config& c, const NetDims& nd, uint32_t n_params, std::vector<float>& master);

}  // namespace mon

// opaque C handles of include/mon_core.h
struct mon_dataset { mon::Dataset* d; };
struct mon_object { mon::Model* m; };
struct mon_dist_field { mon::DistField* f; };
