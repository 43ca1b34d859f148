/* mon_core_diag.h -- C ABI of libmon_core_diag.so: diagnostics and test scaffolding of the MI355X Multi-Object-NeRF core.
 *
 * NOT part of the drop-in boundary (include/mon_core.h, libmon_core.so): nothing here is needed to run RO-MAP.  The library links against
 * libmon_core.so and looks into its objects (ro-map_amd/csrc/model.h) for the parity tests, the layout self-tests and the micro-benchmarks
 * that drove the design (profiles/r01_microbench.md). */
#ifndef MON_CORE_DIAG_H
#define MON_CORE_DIAG_H
#include "mon_core.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Copy an internal device buffer to the host; ids in ro-map_amd/csrc/model.h (MON_BUF_*). */
int mon_object_debug_read(mon_object* obj, int which, void* dst, size_t bytes);
/* Copy one uploaded frame of a dataset back to the host: rgba[H*W] packed r | g << 8 | b << 16 | instance << 24, depth[H*W] (NULL or a dataset without depth:
 * skipped), pose[16] (Twc, column-major).  The upload test compares what arrived with what was sent, frame by frame. */
int mon_dataset_debug_read(mon_dataset* ds, uint32_t frame, uint32_t* rgba, float* depth, float* pose16);
/* Diagnostic micro-benchmarks of scatter strategies (ro-map_amd/csrc/microbench.hip); *ms = best of 3 runs. */
int mon_microbench(int device, int mode, int pattern, uint32_t n_entries, uint32_t n_ops, float* ms);
/* Host-side check hook: corner index of the fused kernels' closed form (device_common.h:fast_grid_index) for level `level`
 * of configuration cfg; *size = entries of that level.  No device needed. */
int mon_debug_fast_index(const mon_config* cfg, int level, uint32_t x, uint32_t y, uint32_t z, uint32_t* index, uint32_t* size);
/* Layout of the MFMA A-fragment image of the fused kernels (ro-map_amd/csrc/frag_layout.h), both directions, for the layout test:
 * source[n_image] = MLP parameter index held by each image element (-1 = structural zero); slots[2 * n_mlp] = the (<= 2) image elements
 * each parameter feeds (-1 = none).  Either pointer may be NULL. */
int mon_debug_frag_layout(int encoded_width_padded, int n_neurons, int n_hidden_layers, int n_levels, int* source, int* slots, int* n_image, int* n_mlp);
/* Accumulator layout of k_fused_train's dW partial rows (frag_layout.h acc_param): param[n_cols] = MLP parameter index each column sums into
 * (-1 = pad column of a narrow encoding); the loss partial follows at column n_cols.  param may be NULL. */
int mon_debug_acc_layout(int encoded_width_padded, int n_neurons, int n_hidden_layers, int n_levels, int* param, int* n_cols);
/* MFMA fragment-layout self-test: D[32x32] = A[32x16] * B[16x32], fp16 in / fp32 out, through the lane mapping the fused kernels rely on. */
int mon_selftest_mfma(int device, const uint16_t* A, const uint16_t* B, float* D);
/* config.yaml key look-up of the sequence reader (cv::FileStorage semantics: exact key at line start); returns MON_ERR_IO when absent. */
int mon_debug_yaml_number(const char* text, const char* key, double* value);
/* Occupancy-grid bookkeeping of an object created with occupancy_skip (model.cpp maybe_refresh_occupancy): out[0] = iteration of the last refresh
 * (0 = none yet), out[1] = first iteration at or after which the next one is due. */
int mon_debug_occupancy_state(mon_object* obj, uint32_t out[2]);
/* Training's occupancy grid (64^3 bits, x fastest, 8192 words; bit n of word w = cell 32 w + n): `raw` before and `dilated` after the one-cell dilation (the
 * grid k_fused_train uses; before the first refresh or pin both are the warm-up's all-ones grid), the raw-density threshold, and the number of live-sample
 * lists of the level-tile chain (0: the object has none).  Any output may be NULL.  MON_ERR_STATE when the object has no grid. */
int mon_debug_occupancy_grid(mon_object* obj, uint32_t* raw, uint32_t* dilated, float* raw_threshold, uint32_t* n_parts);
/* Pins a caller-supplied training grid (8192 words) in place of the object's own, also before the warm-up: the grid is in use from the next iteration, the
 * positions already sampled for it are sampled again, and no scheduled refresh replaces it.  bits = NULL unpins: before the warm-up the all-ones grid
 * returns, afterwards a refresh is due at the next iteration.  MON_ERR_STATE when the object has no grid. */
int mon_debug_set_train_occupancy(mon_object* obj, const uint32_t* bits);

/* Tile render bookkeeping (ro-map_amd/csrc/kernels_tilerender.hip): jobs (rays that hit the object's box, 2S samples each) of the LAST crop rendered on the
 * object's device through the per-device workspace of `side` (0: train-stream renders, 1: the inference stream); what bench.py's evaluated-sample count is. */
int mon_debug_render_jobs(mon_object* obj, int side, uint32_t* jobs);

/* Render skipping (mon_object_set_render_skip): pins a caller-supplied grid (64^3 bits, x fastest, 8192 words) for `side` in place of the one the object
 * builds, until called again with bits = NULL.  The tests check the renders' cell look-up against geometry through it. */
int mon_debug_set_render_grid(mon_object* obj, int side, const uint32_t* bits);

/* Scene render (mon_scene_render), its two kernels one at a time.  mon_debug_scene_samples: object k's sample lists of the scene render of rect (the same
 * arguments), host arrays per pixel of the rect (row-major): t[64], alpha[64], rgb[64][3] and count (0: the ray missed the box; else 32 or 64, the slots
 * written).  Any output may be NULL.  mon_debug_scene_composite: the merge-composite kernel on caller lists, n_lists x n_rays lists of up to 64 samples,
 * ascending in t: t[n_lists][n_rays][64], alpha the same, rgb[n_lists][n_rays][64][3], count[n_lists][n_rays] (<= 64); dn[n_rays] = the camera ray norms
 * the depth is divided by.  Outputs as mon_scene_render's, instance = list index.  n_lists <= 256. */
int mon_debug_scene_samples(mon_object* const* objs, size_t n_objs, int side, mon_frame_bbox rect, const float* Twc16, size_t k, float* t, float* alpha,
                            float* rgb, uint32_t* count);
int mon_debug_scene_composite(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                              const float* dn, float* out_rgb, float* out_depth, float* out_opacity, int32_t* out_instance);

/* Scene probe (mon_scene_probe), its own two kernels one at a time.  mon_debug_scene_probe_rays: the ray rows k_scene_probe_rays writes for object k of that
 * probe call (the same arguments first), rows[n_q][10] = o[3], d[3] (object frame), t0, t1, flag (1: the ray hits k's box), dn = |camera ray|; a row that
 * misses the box holds flag 0, dn and zeros.  mon_debug_scene_probe_composite: k_scene_probe_composite on caller lists, the arguments of
 * mon_debug_scene_composite plus the two hit outputs (hit_instance = list index). */
int mon_debug_scene_probe_rays(mon_object* const* objs, size_t n_objs, int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                               size_t k, float* rows);
int mon_debug_scene_probe_composite(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                                    const float* dn, float* out_rgb, float* out_depth, float* out_opacity, int32_t* out_instance, float* out_hit_depth,
                                    int32_t* out_hit_instance);

/* Ray cast (mon_scene_cast), its own two kernels one at a time.  mon_debug_scene_cast_rays: the ray rows k_scene_cast_rays writes for object k of that cast
 * (the same arguments first), rows[n_rays][10] = o[3], d[3] (object frame), t0 = lo, t1 = hi, flag (1: object k contributes), dn = 1, and entry[n_rays] = the
 * entry row the composite reads (lo; 0 where flag is 0); a row with flag 0 holds zeros and dn.  mon_debug_scene_cast_composite: k_scene_cast_composite on
 * caller lists laid out as mon_debug_scene_composite's, plus entry[n_lists][n_rays] and the threshold; out_dist is not divided by anything
 * (hit_instance = list index). */
int mon_debug_scene_cast_rays(mon_object* const* objs, size_t n_objs, int side, const mon_scene_ray* rays, size_t n_rays, size_t k, float* rows, float* entry);
int mon_debug_scene_cast_composite(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                                   const float* entry, float hit_opacity, float* out_rgb, float* out_dist, float* out_opacity, int32_t* out_instance,
                                   float* out_hit_t, float* out_hit_sample_t, int32_t* out_hit_instance);

/* Point queries (mon_scene_query_points, the same arguments first): object k's row of every point as k_scene_points writes it, rows[n][12] = u[3] (the
 * point in k's unit cube), inside (0 / 1), raw4 (the network's raw outputs), sigma_k, r, g, b; a point outside k's box holds u, 0 and eight zeros.  The scene
 * call's outputs are, bit for bit, a fold of these rows over k: the fp32 sum of sigma_k in list order, the first largest sigma_k for the owner. */
int mon_debug_scene_point_rows(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, size_t k, float* rows);
/* Point gradients (mon_scene_query_gradients, the same arguments first, no select): object k's row of every point as k_scene_point_grads writes it,
 * rows[n][16] = mon_debug_scene_point_rows' twelve floats (the same bits), g_k[3] = the world gradient of k's log density there, and one 0; a point
 * outside k's box holds u, 0 and twelve zeros.  The scene call's outputs are, bit for bit, a fold of these rows over k. */
int mon_debug_scene_gradient_rows(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, const float* level_weights, size_t k,
                                  float* rows);

/* Pose refinement (mon_object_pose_loss, the same arguments): per drawn ray of that evaluation (rays_per_iter of them, or every pixel of every box in box
 * order), its 2S = 64 samples: x[ray][64][3] the positions in the object frame, raw[ray][64][4] the network's raw outputs, dldx[ray][64][3] = dL/dx_k in the
 * object frame (the 1/N of the mean included).  Samples not evaluated (a missed box, the second tile behind the early cut) hold 0 (x: the position it would
 * have, or 0 for a miss).  Any output may be NULL. */
int mon_debug_pose_samples(mon_object* obj, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p,
                           uint32_t iteration, float* x, float* raw, float* dldx);

/* Camera refinement against a scene (mon_scene_pose_loss, the same arguments first).  mon_debug_scene_pose_samples: object k's share of that evaluation, per
 * drawn ray: x_o[ray][64][3] the sample positions in k's frame, x_c[ray][64][3] in the camera frame (t x the unit camera ray), t[ray][64], raw[ray][64][4] the
 * network's raw outputs, dldx[ray][64][3] = dL/dx_o (object frame, the 1/N of the mean included) and count[ray] (0: the ray missed k's box; else 32 per
 * evaluated tile).  Samples not evaluated hold raw = dldx = 0 (and x = t = 0 for a miss).  Any output may be NULL.
 * mon_debug_scene_composite_grad: the merged composite's forward and backward (k_scene_composite_grad) on caller lists laid out as mon_debug_scene_composite's,
 * plus per-ray targets cstar[n_rays][3], mstar[n_lists][n_rays], dstar[n_rays], dn[n_rays] and the loss weights.  Outputs: l[n_rays], W[n_lists][n_rays],
 * D[n_rays], dalpha[n_lists][n_rays][64] = dL/dalpha and dc[n_lists][n_rays][64][3] = dL/dc of every sample (0 for slots not merged or behind the cut). */
int mon_debug_scene_pose_samples(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16,
                                 const mon_pose_refine_params* p, uint32_t iteration, const float* level_weights, size_t k, float* x_o, float* x_c, float* t,
                                 float* raw, float* dldx, uint32_t* count);
int mon_debug_scene_composite_grad(int device, uint32_t n_rays, uint32_t n_lists, const float* t, const float* alpha, const float* rgb, const uint32_t* count,
                                   const float* cstar, const float* mstar, const float* dstar, const float* dn, float w_rgb, float w_mask, float w_depth,
                                   float huber, float* out_l, float* out_W, float* out_D, float* out_dalpha, float* out_dc);
/* HIP-event time of the pack / unpack kernels of mon_object_save / mon_object_load calls made by this thread (tools/checkpoint_timing.py): enable != 0
 * starts collecting -- each kernel is bracketed by two events --, *kernel_ms (may be NULL) = the sum since the last call, which is then cleared. */
int mon_debug_checkpoint_timing(int enable, double* kernel_ms);
/* The sweeps of the process's latest shortest-path field (mon_shortest_paths, mon_scene_paths_lattice, mon_online_paths_lattice; tools/scene_paths_timing.py):
 * out3 = { sweeps enqueued, batches (one read-back each), sweeps that left work for the next one }. */
int mon_debug_paths_stats(uint32_t* out3);
/* k_encode_tiles' workgroup order (ro-map_amd/csrc/model.h enc_block_decode, the function the kernel calls): workgroup `block` of a grid row of 16 n_levels
 * workgroups walks partition *part (0..15) of level *level.  No device needed.  MON_ERR_ARG for n_levels outside 1..16 or block >= 16 n_levels. */
int mon_debug_encode_block(uint32_t block, int n_levels, uint32_t* level, uint32_t* part);

#ifdef __cplusplus
}
#endif
#endif
