/*
 * mon_core.h -- C ABI of libmon_core.so, the MI355X-native Multi-Object-NeRF core.
 *
 * This is the drop-in boundary for the one hot path of XiaoHan-Git/RO-MAP: the per-object NeRF
 * inside dependencies/Multi-Object-NeRF/Core (libMON.so).  The reference exposes a C++ ABI
 * (namespace nerf, Eigen / cv::Mat types); every entry point below cites the reference member it
 * replaces.  CORE = /root/reference/dependencies/Multi-Object-NeRF/Core.  The C++ shim that
 * reproduces the reference's class names on top of this ABI is shown in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns an int status
 * (MON_OK == 0); matrices are 4x4 float, column-major (Eigen::Matrix4f memory order); images are
 * row-major HxW.  A handle may be used from one thread at a time; different handles are
 * independent (the reference runs one std::thread per object, CORE/src/nerf_manager.cu:89,259).
 * There is NO CPU fallback: every compute entry point fails with MON_ERR_NO_DEVICE when no gfx950
 * device is visible.
 */
#ifndef MON_CORE_H
#define MON_CORE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MON_OK              0
#define MON_ERR_ARG         1   /* bad argument                                        */
#define MON_ERR_NO_DEVICE   2   /* no HIP device (reference: cerr + exit(0), nerf_manager.cu:21-25) */
#define MON_ERR_HIP         3   /* HIP runtime error (reference: CUDA_CHECK_THROW)     */
#define MON_ERR_IO          4   /* file / parse error                                  */
#define MON_ERR_STATE       5   /* call not valid in the current state                 */
#define MON_ERR_NO_RAYS     6   /* a training step found zero rays inside the 3-D box (reference: i % 0 UB, nerf_model.cu:287) */

/* Network / training configuration.  Fields follow CORE/configs/base.json (tcnn JSON schema) and
 * the compile-time constants of CORE/include/nerf_model.h:145,166,172-175 promoted to runtime. */
typedef struct mon_config {
    int32_t  n_levels;             /* encoding.n_levels (16)                                 */
    int32_t  n_features;           /* encoding.n_features_per_level; must be 2               */
    int32_t  log2_hashmap_size;    /* encoding.log2_hashmap_size (16)                        */
    int32_t  base_resolution;      /* encoding.base_resolution (16)                          */
    float    per_level_scale;      /* encoding.per_level_scale; tcnn default 2.0             */
    int32_t  n_neurons;            /* network.n_neurons: 16, 32, 64 or 128 (tcnn FullyFusedMLP) */
    int32_t  n_hidden_layers;      /* network.n_hidden_layers: 1 or 2; 3 or 4 up to 64 neurons */
    int32_t  rays_per_batch;       /* mnRaysPerBatch (4096); multiple of 64                  */
    int32_t  n_samples;            /* mnSampleNum (32); render uses 2x (mnRenderSampleNum)   */
    float    loss_scale;           /* mLoss_Scale (128)                                      */
    float    learning_rate;        /* optimizer...nested.nested.learning_rate (1e-2)         */
    float    beta1, beta2, epsilon, l2_reg;
    float    ema_decay;            /* optimizer.decay (0.95)                                 */
    int32_t  decay_start, decay_interval;
    float    decay_base;
    uint32_t param_seed;           /* m_seed (1337)                                          */
    /* rng_flags: "same inputs" mode for a comparison with the CUDA build; 0 (default) = this repo's own streams:
     *   bits 0-1   sample stream: 0 counter RNG keyed by sample_seed | 1 XORWOW in the reference's order of draws, cuRAND flavour
     *              (nerf_model.cu:1432,1434,1468 and :1781; default seed) | 2 the same with rocRAND's seeding / float map
     *   bit  4     parameter init in tcnn's generate_random_uniform element order (pcg32 draws interleaved per thread)
     *   bits 16-31 XORWOW lanes in units of 1024 (0 = 4: cuRAND's 4096 subsequences)   -- ro-map_amd/csrc/xorwow.h */
    uint32_t rng_flags;
    uint64_t sample_seed;          /* key of the counter RNG that replaces the cuRAND XORWOW stream by default */
    int32_t  use_depth;            /* NeRF_Model::mbUseDepth                                 */
    /* occupancy_skip: 0 (default, the reference's behaviour: every one of the 32 samples of a ray is evaluated) | 1: occupancy-grid skipping -- a 64^3 bit
     * grid over the object's box, refreshed from the training weights (every 32 iterations at first, every 512 later) after 256 warm-up iterations and
     * dilated by one cell; samples in empty cells are not evaluated (no table reads, no contribution, no gradient).  An approximation the reference does
     * not have: parity runs leave it off. */
    int32_t  occupancy_skip;
} mon_config;

/* CORE/include/common.h:18-23 (note: h before w). */
typedef struct mon_frame_bbox { uint32_t FrameId, x, y, h, w; } mon_frame_bbox;

typedef struct mon_dataset mon_dataset;   /* nerf::NeRF_Dataset, one per device (nerf_data.h:19-71)   */
typedef struct mon_object  mon_object;    /* nerf::NeRF + nerf::NeRF_Model (nerf.h:19-89, nerf_model.h:92-184) */

typedef struct mon_object_info {
    uint32_t n_params, n_mlp_params, n_grid_params, encoded_width;
    uint32_t train_step;           /* mnTrainingStep                                        */
    uint32_t n_boxes;              /* mnBbox                                                */
    uint32_t last_n_valid;         /* rays inside the 3-D box in the last batch             */
    int32_t  device;               /* mGPUid                                                */
    float    last_loss;            /* mfPerTrainLoss                                        */
    float    learning_rate;        /* after ExponentialDecay                                */
    int32_t  backend;              /* 0 unfused kernels, 1 fused MFMA kernel                */
    uint32_t skipped_batches;      /* iterations skipped because no ray hit the 3-D box     */
} mon_object_info;

/* Kernel classes timed with HIP events on the object's train stream when profiling is on. */
enum { MON_K_BATCH = 0, MON_K_FWDBWD = 1, MON_K_OPTIM = 2, MON_K_RENDER = 3, MON_K_SCATTER = 4, MON_K_REDUCE = 5, MON_K_ENCODE = 6 /* k_encode_tiles */,
       MON_K_POINTS = 7 /* k_sample_points */, MON_K_COUNT = 8 };
/* FWDBWD = k_fused_train alone (fused backend) or the unfused forward/backward kernel group; SCATTER = k_grid_scatter; REDUCE = k_reduce_partials. */
typedef struct mon_profile { double ms[MON_K_COUNT]; uint64_t launches[MON_K_COUNT]; } mon_profile;

const char* mon_last_error(void);                 /* thread-local message for the last non-OK status */
int mon_version(void);

/* NerfManager{Offline,Online}::Init -- device discovery (nerf_manager.cu:16-38, :136-158). */
int mon_device_count(int* n_devices);
/* Device numbering of everything below is LOGICAL.  Default: the physical HIP devices.  n > 0: n logical devices mapped round-robin onto the
 * physical ones (logical d -> physical d mod physical count), so the reference's object k -> device k mod nGPU placement with one dataset replica
 * per device (nerf.cu:27-33, nerf_manager.cu:44-55) can be driven -- oversubscribed -- on a box with fewer GPUs; 0 restores the default.  Call before
 * creating datasets / managers. */
int mon_set_logical_devices(int n);
/* the HIP device a logical device runs on (what a multi-device consumer groups objects by) */
int mon_physical_device(int logical_device, int* physical_device);

/* NeRF_Model::ReadNetworkConfig (nerf_model.cu:1272-1284): tcnn JSON with comments. */
int mon_config_default(mon_config* cfg);                       /* CORE/configs/base.json values */
int mon_config_from_json(const char* path, mon_config* cfg);

/* NerfManagerOnline::DatasetInit / NeRF_Dataset::InitDataToGPU (nerf_manager.cu:160-187, nerf_data.cu:237-271):
 * intrinsics + capacity for max_frames frames resident in HBM on `device`. */
int mon_dataset_create(int device, int H, int W, float fx, float fy, float cx, float cy,
                       uint32_t max_frames, int use_depth, mon_dataset** out);
/* NerfManagerOnline::NewFrameToDataset / NeRF_Dataset::FrameDataToGPU (nerf_manager.cu:189-218,
 * nerf_data.cu:273-339) and the per-image body of DataToGPU (nerf_data.cu:151-221).
 * rgb: HxWxchannels 8-bit (channels 3 or 4), is_bgr as delivered by cv::imread / the SLAM frontend;
 * instance: HxW 8-bit instance ids (0 = background); depth: HxW float metres (z-depth, 0 = none) or NULL;
 * Twc16: camera-to-world pose. */
int mon_dataset_add_frame(mon_dataset* ds, uint32_t frame_id, const uint8_t* rgb, int channels, int is_bgr,
                          const uint8_t* instance, const float* depth, const float* Twc16);
int mon_dataset_n_frames(const mon_dataset* ds, uint32_t* n);
int mon_dataset_destroy(mon_dataset* ds);

/* NerfManagerOnline::CreateNeRF / NeRF::SetAttributes + CreateModelOnline + ResetNetwork
 * (nerf_manager.cu:237-261, nerf.cu:155-185, nerf_model.cu:1259-1342) and NerfManagerOffline::CreateNeRF
 * (nerf_manager.cu:64-92).  class_id doubles as the instance id (nerf.cu:75,158).  The 1.1x/1.2x box
 * inflation of SetAttributes is the caller's business (the shim applies it); aabb is used as given. */
int mon_object_create(mon_dataset* ds, const mon_config* cfg, int class_id, const float* Tow16,
                      const float* aabb_min3, const float* aabb_max3, mon_object** out);
/* NeRF_Model::UpdateFrameIdAndBbox / UpdateFrameIdAndBboxOnline (nerf_model.cu:1609-1628): append. */
int mon_object_add_boxes(mon_object* obj, const mon_frame_bbox* boxes, size_t n);
/* NeRF_Model::Train_Step / Train_Step_Online (nerf_model.cu:1630-1699): `iters` iterations of
 * GenerateBatch -> Step_No_Compacted -> optimizer_step; returns after the train stream drained.
 * *loss (may be NULL) = mean per-ray loss of the last iteration (mfPerTrainLoss). */
int mon_object_train(mon_object* obj, int iters, float* loss);
/* NeRF_Model::Render (nerf_model.cu:1702-1830; pose_is_Toc=0, pose=Twc) and one pose of RenderVideo
 * (:1916-1976; pose_is_Toc=1).  Outputs box.h x box.w: rgb[3*h*w] float RGB, depth, mask; host
 * pointers unless dst_on_device != 0 (then device pointers on the object's device). */
int mon_object_render(mon_object* obj, mon_frame_bbox box, const float* pose16, int pose_is_Toc,
                      float* rgb, float* depth, float* mask, int dst_on_device);
/* The same render on the object's INFERENCE stream (mpInferenceStream, nerf_model.cu:1269) from the inference weights the training side
 * published last (at the end of a mon_object_train call / online training slice -- of every call of 64 or more iterations, otherwise when a
 * viewer has asked since the last publication or 10 ms have passed): callable from any thread WHILE another thread trains
 * the object -- no model lock, nothing queued behind training.  *snapshot_step (may be NULL) = optimizer steps the weights had.  Host
 * outputs.  MON_ERR_STATE before the first publication and for objects without an inference side (tables above 8 M parameters, unfused
 * backend): use mon_object_render under the caller's own serialisation there. */
int mon_object_render_snapshot(mon_object* obj, mon_frame_bbox box, const float* pose16, int pose_is_Toc,
                               float* rgb, float* depth, float* mask, uint32_t* snapshot_step);
/* Empty-space skipping for this object's renders (default off; the reference evaluates every sample).
 * enable != 0: before a render, a 64^3 grid over the object's box is built from the weights that render reads (EMA once training has run, the published
 * snapshot on the inference side).  The grid is cached per side and weights epoch, so a video's 60 views or a viewer's repeated crops of one snapshot
 * build it once.  A cell is live if it or one of its 26 neighbours has alpha >= min_alpha at the cell centre, with alpha = 1 - exp(-sigma * dt) and
 * dt = box diagonal / (2S).  A sample in a dead cell contributes exactly what a sample of alpha 0 contributes: no table reads, no MLP where a whole
 * 32-sample tile is dead; the next live sample's interval is unchanged.  min_alpha <= 0: every cell is live (bit-identical images).  min_alpha must be < 1.
 * Applies to mon_object_render, mon_object_render_snapshot and everything built on them (managers' test images, RenderVideo, mon_online_render); not to
 * density grids or meshes.  MON_ERR_STATE for objects outside the fused shapes (the layer-kernel backend).  The switch is read once per render call. */
int mon_object_set_render_skip(mon_object* obj, int enable, float min_alpha);
typedef struct mon_render_skip_stats {
    uint32_t active;           /* the last render of this side skipped (0: switch off or unsupported path)  */
    uint32_t live_cells;       /* set bits of the grid that render used                                     */
    uint64_t grid_builds;      /* grids built on this side so far                                           */
    uint64_t samples_in_box;   /* last render: rays that hit the box x 2S                                   */
    uint64_t samples_live;     /* last render: of those, samples in live cells                              */
} mon_render_skip_stats;
/* side 0: renders on the train stream (mon_object_render, the managers); 1: mon_object_render_snapshot (MON_ERR_STATE without an inference side) */
int mon_object_render_skip_stats(mon_object* obj, int side, mon_render_skip_stats* out);
/* The grid of the side's last skipping render: 64^3 bits, x fastest, 8192 words.  dilated = 0: before dilation.  MON_ERR_STATE before the first one. */
int mon_object_render_occupancy(mon_object* obj, int side, int dilated, uint32_t* bits);
/* Scene render: several objects of one device seen from one camera, composited in depth order (the reference has no such call; opt-in, new).
 * For every pixel ray of rect (x, y, w, h; FrameId ignored) under Twc16 (column-major), each object contributes exactly the samples its own render of
 * the same rect and pose takes: the same ray, the same 2S jittered distances t (its own sample_seed), the same alpha and colour, its render grid when
 * render skipping is on (a dead sample has alpha 0 and colour 0).  t is the distance along the unit world ray, so the samples of all objects the ray
 * hits are merged by t (ties: the lower index in objs) and composited front to back: w_i = alpha_i * T_i, T_0 = 1, T_{i+1} = T_i (1 - alpha_i);
 * the first sample with T_i < 1e-4 and everything behind it get weight 0.  Outputs, h*w each (rgb 3*h*w), host pointers:
 *   rgb      = sum w_i c_i + T_end (soft, white background, not binarised)
 *   depth    = sum w_i t_i / |camera ray| (z-depth, as mon_object_render) where opacity > 0.5, else 0
 *   opacity  = 1 - T_end                                                    (may be NULL)
 *   instance = index in objs of the object with the largest summed weight where opacity > 0.5, else -1   (may be NULL)
 * A pixel that hits no box: rgb 1, depth 0, opacity 0, instance -1.  With one object, on pixels where its own render has mask 1, rgb and depth are that
 * render's values and instance is 0.
 * side 0: the objects' train-side weights (EMA once trained), on the first object's train stream -- the caller serialises against the objects' training,
 *         as for mon_object_render;
 * side 1: each object's last published snapshot on the device's inference stream -- callable while the objects train, as mon_object_render_snapshot.
 * Render grids: each object's own cache of that side (built here when stale; counted in its grid_builds); the objects' skip statistics are left as they
 * were.  Returns:
 *   MON_ERR_ARG    objs or an element, Twc16, rgb or depth NULL; n_objs 0 or above 256; rect empty; side not 0 / 1; objects on different logical devices
 *                  or with different intrinsics
 *   MON_ERR_STATE  an object outside the fused shapes (the layer-kernel backend); an object in the XORWOW "same inputs" render mode (rng_flags
 *                  sample-stream bits); side 1 and an object without an inference side or with nothing published yet */
int mon_scene_render(mon_object* const* objs, size_t n_objs, int side, mon_frame_bbox rect, const float* Twc16,
                     float* rgb, float* depth, float* opacity, int32_t* instance);
/* Scene probe: what mon_scene_render returns, at a list of sub-pixel image points under one or several camera poses, in one enqueue, plus the depth at
 * which each ray is actually stopped (a feature-based front end's question: depth and object id at keypoints under a predicted pose; the reference has no
 * such call; opt-in, new).
 * Query i looks through pose Twc16s + 16 q[i].pose (column-major, camera to world) at image point (u, v) -- any finite position, inside the image or not.
 * For each object j its ray is the one mon_scene_render builds for a pixel at (u, v), intersected with j's box; its 2S = 64 samples are that render's, with
 * the jitter index key * 64 + k of j's own render stream; the same termination, render grid (when render skipping is on) and dead samples.  The lists are
 * merged and composited exactly as mon_scene_render does it.  Outputs per query, host pointers:
 *   rgb, depth, opacity, instance   as mon_scene_render defines them
 *   hit_depth    = t_i / |camera ray| of the first merged sample i with 1 - T_{i+1} > 0.5 (the transmittance the composite carries after it), else 0
 *   hit_instance = the index in objs of that sample's object, else -1
 * hit_depth is a sample distance, not interpolated inside the sample's interval (mon_scene_cast's hit_t is); unlike depth (sum w t) it does not smear across an occlusion edge.
 * Bit rule: a query with integer-valued u = x, v = y and key = (y - rect.y) * rect.w + (x - rect.x) returns in rgb, depth, opacity and instance the bits
 * mon_scene_render(objs, n_objs, side, rect, Twc, ...) returns for that pixel.  The six outputs of a query do not depend on the other queries of the call,
 * on its place in the list, on the number of poses or on how the list is cut into passes (16 384 queries each); no atomics: equal arguments, equal bits.
 * key: any stable per-keypoint number below 2^26, or the pixel index when the result is to be compared with a render.
 * Read-only, side as in mon_scene_render (0: the caller serialises against training; 1: the snapshots pinned once for the whole call, callable while the
 * objects train).  Nothing about any object changes beyond building a stale render grid, as the scene render does.  Returns:
 *   MON_ERR_ARG    objs or an element, Twc16s, q, rgb or depth NULL; n_objs 0 or above 256; n_poses outside 1..4096; n_q outside 1..2^22; a pose index
 *                  >= n_poses; a key >= 2^26; a non-finite u, v or pose matrix; side not 0 / 1; objects on different logical devices or with different
 *                  intrinsics -- all before any device work
 *   MON_ERR_STATE  as mon_scene_render */
typedef struct mon_scene_query { uint32_t pose; uint32_t key; float u, v; } mon_scene_query;   /* 16 bytes */
int mon_scene_probe(mon_object* const* objs, size_t n_objs, int side, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                    float* rgb, float* depth, float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance);
/* Ray cast: the object map asked along world rays by a consumer that is not a camera of the dataset -- a planner's line-of-sight check between two points,
 * a range sensor, a grasp query, the surface point along a map point's viewing ray (the reference has no such call; opt-in, new).  Forward only; the
 * normal at the hit: mon_scene_cast_normals below; queries at points rather than along rays: mon_scene_query_points below.
 * Ray i is x(t) = o + t d for 0 <= t <= t_max in the world frame; d must be unit (| |d|^2 - 1 | <= 1e-3, used as given: the device does not renormalise);
 * t_max > 0, +inf allowed.  For object j the ray is taken into j's frame (R_ow d, R_ow o + t_ow) and intersected with j's box at [t0, t1]; j contributes iff
 * the box is hit and lo < hi, lo = max(t0, 0), hi = min(t1, t_max).  Its 2S = 64 samples are the scene render's for a ray row {t0 = lo, t1 = hi}:
 * t_k = fma((hi - lo) / 64, k + u_k, lo) with the jitter index key * 64 + k of j's own render stream; alpha, colour, termination, render grid (when render
 * skipping is on) and dead samples as in mon_scene_render.  As there, the interval of an object's first sample is measured from t = 0 (the ray's origin),
 * not from lo: a caller who means the segment from a to b puts o = a, so that nothing in front of the segment is counted.  The lists are merged and
 * composited exactly as mon_scene_render does it.  Outputs per ray, host pointers (the last five may be NULL):
 *   rgb, opacity, instance   as mon_scene_render defines them
 *   dist          = sum w t where opacity > 0.5, else 0 (mon_scene_probe's depth without the division by |camera ray|)
 *   hit_sample_t, hit_instance = t_i and the index in objs of the first merged sample i with 1 - T_{i+1} > hit_opacity, else 0 and -1
 *   hit_t         = p + f (t_i - p): the crossing placed inside sample i's interval under the piecewise-constant density the composite assumes,
 *                   f = clamp(ln(T_i / (1 - hit_opacity)) / (-ln(1 - alpha_i)), 0, 1), f = 0 when 1 - alpha_i == 0; p = the previous sample's t in the same
 *                   object's list, or that object's lo for its first sample (never in front of the box); T_i = the merged transmittance in front of
 *                   sample i.  p <= hit_t <= hit_sample_t; 0 where there is no hit.
 * hit_opacity in (0, 0.999]: 0.5 is mon_scene_probe's rule; a planner takes about 0.1 for a conservative stop.
 * Bit rule: with rays = mon_camera_rays(the dataset's intrinsics, poses, q) (t_max = +inf, the queries' keys) and hit_opacity = 0.5, rgb, opacity, instance
 * and hit_instance are the bits of mon_scene_probe(q), and dist / dn, hit_sample_t / dn (fp32, dn = mon_camera_rays' dn_out) those of its depth and
 * hit_depth -- except on a ray that meets an object's box only behind its origin (t1 < 0): mon_scene_probe, like mon_scene_render, samples such an object
 * at negative t, here it is a miss (lo < hi fails) and the ray's outputs are those of the other objects.  A ray's outputs do not depend on the other rays of the call, on its place in the list or on how the list is cut into passes (16 384 rays
 * each); no atomics: equal arguments, equal bits.  One enqueue, one synchronisation.  Read-only, side as in mon_scene_render.  The objects need not share
 * a dataset or intrinsics: no camera is involved.
 * Axis-aligned rays: a direction component that is exactly 0 in an object's frame (straight down onto an object whose rotation is the identity) gives
 * infinite slab distances and the right answer: a miss when the origin lies outside that slab, no constraint from it when inside.  Only when the origin
 * also lies exactly in one of that slab's two planes (0 / 0) is the answer for that object unspecified between a miss and a ray that runs inside the face;
 * every output stays finite.
 * Returns:
 *   MON_ERR_ARG    objs or an element, rays, rgb or dist NULL; n_objs 0 or above 256; n_rays outside 1..2^22; a key >= 2^26; a non-finite o or d; a
 *                  non-unit d; t_max <= 0 or NaN; hit_opacity outside (0, 0.999]; side not 0 / 1; objects on different logical devices -- all before
 *                  any device work
 *   MON_ERR_STATE  as mon_scene_render */
typedef struct mon_scene_ray { float o[3]; float t_max; float d[3]; uint32_t key; } mon_scene_ray;   /* 32 bytes */
int mon_scene_cast(mon_object* const* objs, size_t n_objs, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity,
                   float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance);
/* Host only, no device: the world rays mon_scene_probe casts for the queries q under the camera-to-world poses Twc16s with the pinhole (fx, fy, cx, cy):
 * rays_out[i] = { o = the camera centre, t_max = +inf, d = R_wc (dc / |dc|) with dc = ((u - cx) / fx, (v - cy) / fy, 1), key = q[i].key } and, where
 * dn_out is not NULL, dn_out[i] = |dc| (a depth along the optical axis = a distance along the ray / dn).  The arithmetic is the device's, operation for
 * operation.  MON_ERR_ARG: Twc16s, q or rays_out NULL; n_poses or n_q 0; a pose index >= n_poses; a non-finite intrinsic, pose, u or v; fx or fy 0. */
int mon_camera_rays(float fx, float fy, float cx, float cy, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                    mon_scene_ray* rays_out, float* dn_out);
/* Point queries: the object map asked about a place instead of a ray -- is this voxel free, which object owns this point, how dense is the field over
 * this lattice (a planner's or a grasper's question; a ray costs 64 samples per answer, a point one; the reference has no such call; opt-in, new).  Forward
 * only; the field's derivative at the same points: mon_scene_query_gradients below.
 * A world point x goes into object j's frame as mon_scene_cast takes a ray origin there, q = R_ow x + t_ow, and into j's unit cube by the operation the
 * render applies to a sample point, u_a = (q_a - aabb_min_a) / (aabb_max_a - aabb_min_a); it is inside j iff 0 <= u_a <= 1 on all three axes.  For an
 * inside point the network is evaluated at u exactly as the render evaluates a sample, with the render's weights of that side; sigma_j = exp(o3),
 * c_j = logistic(o0..2), the render's two lines (sigma_j may be +inf for a saturated fp16 output; it is passed on as is).  Outside, sigma_j = 0.
 * Outputs per point, host pointers (all but sigma may be NULL):
 *   sigma       = the sum of sigma_j over the objects the point is inside, added in fp32 in the order of objs
 *   owner       = the index in objs of the object with the largest sigma_j among those (ties: the lower index), -1 when the point is inside none
 *   rgb         = the owner's colour, 0 0 0 without an owner
 *   owner_sigma = the owner's sigma_j, 0 without an owner
 *   n_inside    = the number of boxes the point lies in
 * sigma is a density per unit of WORLD length (Tow is rigid: lengths in an object's frame are world lengths): the opacity of a step of length l through
 * the point is 1 - exp(-sigma l), which is what a caller thresholds.
 * A point's outputs depend on that point and the objects alone: not on the other points, its place in the list, how the list is cut into passes (16 384
 * points each) or whether it came by list or by lattice; no atomics: equal arguments, equal bits.  One enqueue, one synchronisation.  Read-only; side as
 * in mon_scene_render (0: the caller serialises against training; 1: the snapshots, callable while the objects train).  The objects need only share a
 * device.  The sample count, render skipping and the XORWOW render mode play no part: nothing is sampled, skipped or jittered.
 * mon_scene_query_lattice: the same at the points p(i, j, k) = (fmaf(i, step[0], origin[0]), fmaf(j, step[1], origin[1]), fmaf(k, step[2], origin[2])),
 * 0 <= i < nx (fastest), j < ny, k < nz, formed on the device: nothing is uploaded but the six floats.  Output index (k * ny + j) * nx + i.
 * mon_lattice_points (host only, no device): those points exactly as the device forms them, xyz_out[nx * ny * nz][3]; mon_scene_query_points of them
 * returns the lattice call's bits.
 * mon_object_query_points: one object, points given in its unit cube (the coordinates its encoder takes): raw4[n][4] = the network's four raw fp16
 * outputs (o0..2 colour, o3 log density) widened to fp32, by the same kernel with the transform switched off.
 * Returns:
 *   MON_ERR_ARG    objs or an element, the points (origin3, step3) or sigma (raw4) NULL; n_objs 0 or above 256; n or nx * ny * nz outside 1..2^22; nx, ny
 *                  or nz below 1; a non-finite point, origin or step, or a lattice that leaves the finite floats; side not 0 / 1; objects on different
 *                  logical devices; mon_object_query_points: a point outside [0, 1]^3 -- all before any device work, the outputs untouched
 *   MON_ERR_STATE  an object outside the fused shapes (the layer-kernel backend); side 1 and an object with nothing published yet */
int mon_object_query_points(mon_object* obj, int side, const float* unit_xyz, size_t n, float* raw4);
int mon_scene_query_points(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n,
                           float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside);
int mon_scene_query_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                            float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside);
int mon_lattice_points(const float* origin3, const float* step3, int nx, int ny, int nz, float* xyz_out);
/* Point gradients and surface normals: the point queries with the field's derivative -- the surface normal at a grasp contact, the direction that takes a
 * path away from an object (the reference has no such call; opt-in, new, read-only; no existing call changes its bits).  Differencing point queries does
 * not give it: the finest cells of a base.json grid are about 2e-6 of the box and the raw log density is fp16, so a difference inside a cell measures
 * rounding.  The derivative here is analytic.
 * Per object j and point: the point goes into j's unit cube and is judged inside exactly as in mon_scene_query_points; the forward is that call's, so
 * raw4, sigma_j = exp(o3) and the colour are its values bit for bit.  The backward runs the pose routes' tile backward (dL/dO -> dL/dx) from the seed
 * dO = (0, 0, 0, 1), scaled by 2^5 into fp16 and unscaled exactly: it yields d o3 / d q, the gradient of j's raw log density.  Held at their forward values:
 * each level's hash-grid corners and the ReLU masks of the fp16 forward; only the trilinear weights are differentiated, which away from cell faces and
 * ReLU kinks is the field's derivative.  Level l's term is multiplied by level_weights[l] (NULL: every weight 1, the exact gradient of the field; object j
 * reads level_weights[0 .. L_j) of an array of Lmax = the largest n_levels among the objects).  g_obj = d o3 / d q per unit of object-frame length;
 * g_j = R_ow^T g_obj in fp32 (g_a = fmaf(R(2,a), g_obj2, fmaf(R(1,a), g_obj1, R(0,a) g_obj0))) is the world gradient of j's log density -- Tow is rigid, so
 * nothing is rescaled.  Outside j's box g_j = 0.
 * On fine grids the gradient of every level is dominated by the finest ones and is noise as a surface direction: for a NORMAL pass
 * a coarse window, level_weights[l] = 1 for the coarse levels and 0 above (mon_pose_c2f_weights forms such windows).
 * Outputs per point: the five of mon_scene_query_points with the same bits (sigma required, the others may be NULL), and
 *   grad_log[3]   (required) = g_j of the owner (of the selected object), 0 0 0 without one
 *   grad_sigma[3] (may be NULL) = sum over the objects the point is inside, in the order of objs, per component acc = fmaf(sigma_j, g_j, acc): the world
 *                 gradient of sigma.  A non-finite sigma_j is passed on as IEEE arithmetic gives it, as in sigma.
 *   normal[3]     (may be NULL) = -grad_log / |grad_log|, the direction of falling density, outward from a surface; |g| = sqrtf(fmaf(g2, g2, fmaf(g1, g1,
 *                 g0 g0))), one division per component.  0 0 0 without an owner, or when |g| is 0 or not finite (under- and overflow of the squares included).
 * select: NULL, or n int32.  -1 keeps the owner rule; k >= 0 makes object k the one reported in owner, rgb, owner_sigma, grad_log and normal if the point
 * lies in k's box, else those are reported as "no owner" (-1, zeros).  sigma, n_inside and grad_sigma do not depend on select.
 * Independence, sides, passes (16 384 points), "no atomics: equal arguments, equal bits", one enqueue and one synchronisation: as mon_scene_query_points.
 * mon_scene_query_lattice_gradients: the same over the lattice, formed on the device as mon_scene_query_lattice forms it; it takes no select.
 * mon_object_query_gradients: one object, unit-cube points, the transform off: raw4[n][4] (may be NULL) = mon_object_query_points' bits,
 * grad_unit[n][3] = d o3 / d u, the derivative per unit of the unit cube: the kernel's division by the extent is a division by 1, nothing is multiplied back.
 * Returns MON_ERR_ARG and MON_ERR_STATE as the point queries do, and MON_ERR_ARG for grad_log (grad_unit) NULL, a select value outside [-1, n_objs), a
 * level weight that is negative or not finite -- all before any device work, the outputs untouched.
 * mon_scene_cast_normals: the normal at a ray's hit, a host-side rule whose every step is a public call:
 *   1. mon_scene_cast (the same arguments and seven outputs);  2. for the rays with hit_instance >= 0, x_a = fmaf(hit_t, d_a, o_a) per axis in fp32;
 *   3. mon_scene_query_gradients at those points, compacted in ray order, with select = hit_instance;  4. hit_xyz = x, normal, grad_log scattered back.
 * A miss gets 0 0 0 in all three (hit_xyz and grad_log may be NULL).  Two enqueues and two synchronisations (one when no ray hits).  A hit point that fp32
 * rounding puts outside the hit object's box (a hit exactly on the box's entry face) gets normal and grad_log 0 while hit_instance stays.  Errors: those
 * of mon_scene_cast, a NULL normal, a bad level weight. */
int mon_object_query_gradients(mon_object* obj, int side, const float* unit_xyz, size_t n, const float* level_weights, float* raw4, float* grad_unit);
int mon_scene_query_gradients(mon_object* const* objs, size_t n_objs, int side, const float* world_xyz, size_t n, const float* level_weights,
                              const int32_t* select, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside,
                              float* grad_log, float* grad_sigma, float* normal);
int mon_scene_query_lattice_gradients(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                                      const float* level_weights, float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside,
                                      float* grad_log, float* grad_sigma, float* normal);
int mon_scene_cast_normals(mon_object* const* objs, size_t n_objs, int side, const mon_scene_ray* rays, size_t n_rays, float hit_opacity,
                           const float* level_weights, float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t,
                           int32_t* hit_instance, float* hit_xyz, float* normal, float* grad_log);
/* Distance fields: clearance over a lattice -- how far each cell is from the nearest occupied cell, which cell that is and which object it belongs to; the
 * quantity a path optimiser or a collision check works with (a Euclidean distance field of the voxblox / FIESTA kind; the reference has no such call;
 * opt-in, new, read-only; no existing call changes its bits).  Exact, not approximate: the result is the minimum over ALL occupied cells.
 * The lattice: nx x ny x nz cells, i fastest, cell (i, j, k) at index (k * ny + j) * nx + i; step3 = the spacing per axis, finite; a component may be
 * negative (only its square matters) or 0 (that axis then adds nothing to a distance).
 * The arithmetic, every operation a separately rounded fp32 one (nothing is contracted into an fma):
 *   a_x = (float)(i - i') * step[0], likewise a_y, a_z;   d2(cell, cell') = ((a_x * a_x) + (a_y * a_y)) + (a_z * a_z)
 *   d2(cell) = the least d2(cell, cell') over the occupied cells';   dist = sqrt(d2), the correctly rounded root.
 * It is computed axis by axis -- v1 = min over occupied i' of a_x^2; v2 = min over j' of fl(a_y^2 + v1(i, j', k)); v3 = min over k' of fl(a_z^2 +
 * v2(i, j, k')) -- which, rounding being monotone, is the minimum of the nested expression bit for bit.
 * nearest = the flat index of the occupied cell that gives it.  The rule: in each of the three minimisations the candidates are taken in ascending index
 * along that axis, a candidate replaces the best only when strictly smaller, and the site stored below a candidate is carried along.  Away from ties that
 * rounding itself creates this is the occupied cell with the lowest flat index among the nearest.  Without an occupied cell: dist = +inf, nearest = -1.
 * max_dist (above 0; +inf: no limit): where !(dist <= max_dist), dist = max_dist and nearest = -1; a cell at exactly max_dist keeps its site.
 * No atomics: equal arguments, equal bits; a cell's outputs depend on the mask, the shape and the steps alone.
 * mon_distance_transform: the transform of a host mask (occupied[nx * ny * nz], a cell counts iff its byte is not 0) on `device`, as mon_marching_cubes
 * serves density lattices; dist[nx * ny * nz]; nearest may be NULL.
 * mon_scene_distance_lattice: the object map's field over the lattice of mon_scene_query_lattice (the same points, sides, objects and passes).  A cell is
 * occupied iff !(sigma <= sigma_min), sigma that call's output bit for bit: a NaN or +inf sigma counts as occupied, the conservative reading for a planner.
 * sigma is a density per unit of world length: opacity a over a step of length l corresponds to sigma_min = -ln(1 - a) / l.  Mask, transform and owner
 * lookup run on the device behind the query; one copy home, one synchronisation.  Outputs per cell (all but dist may be NULL):
 *   dist          = the distance to the nearest occupied cell (0 on an occupied cell), truncated by max_dist
 *   nearest       = that cell's flat index, -1 without one
 *   nearest_owner = mon_scene_query_lattice's owner at that cell (an index into objs; -1 where the cell lies in no box, which a finite sigma_min >= 0
 *                   never marks occupied), -1 without a nearest cell
 *   free_dist     = the same transform of the complemented mask: the distance to the nearest FREE cell, 0 on a free cell, truncated by max_dist alike; a
 *                   signed field is dist - free_dist
 *   sigma         = mon_scene_query_lattice's sigma
 * Returns:
 *   MON_ERR_ARG    occupied, step3, origin3, dist, objs or an element NULL; nx, ny or nz below 1 or nx * ny * nz above 2^22; a non-finite step or origin
 *                  (the scene call: a lattice that leaves the finite floats); sigma_min negative or not finite; max_dist <= 0 or NaN; side not 0 / 1;
 *                  n_objs 0 or above 256; objects on different logical devices -- all before any device work, the outputs untouched
 *   MON_ERR_STATE  as mon_scene_query_lattice;   MON_ERR_NO_DEVICE  mon_distance_transform without a device */
int mon_distance_transform(int device, const uint8_t* occupied, int nx, int ny, int nz, const float* step3, float max_dist,
                           float* dist, int32_t* nearest);
int mon_scene_distance_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                               float sigma_min, float max_dist, float* dist, int32_t* nearest, int32_t* nearest_owner, float* free_dist, float* sigma);
/* Connected components: which cells of a lattice belong together -- the global question the local calls above leave open: is the goal reachable from the
 * start by a robot of radius r, which free pockets are sealed off, how many occupied blobs there are and how large each is (the reference has no such
 * call; opt-in, new, read-only; no existing call changes its bits).  Integers only, and the result has a unique definition:
 * The lattice is the distance calls': nx x ny x nz cells, i fastest, cell (i, j, k) at flat index (k * ny + j) * nx + i, nx * ny * nz in 1 .. 2^22.  A cell
 * is in the mask iff its byte is not 0.  Two mask cells are adjacent iff they differ by at most 1 in every coordinate and by at most m in the sum of the
 * absolute differences: connectivity 6 -> m = 1 (faces), 18 -> m = 2 (faces and edges), 26 -> m = 3 (faces, edges and corners).  Nothing wraps round the
 * border.  A component is an equivalence class of the transitive closure of adjacency.  Outputs:
 *   label[cell]   = the lowest flat index among the cells of its component (its representative: label[rep] == rep); -1 outside the mask
 *   comp[cell]    = the rank of its component when the components are ordered by ascending representative, 0 .. n_components - 1; -1 outside the mask
 *   n_components  = the number of components, the total even when cap is smaller (as mon_marching_cubes reports its counts)
 *   table[c]      = one record per component c < min(n_components, cap): its representative, its number of cells and its inclusive bounding box
 *                   lo <= (i, j, k) <= hi; the records from min(n_components, cap) on are not touched
 * The result is a function of the mask, the shape and the connectivity alone: equal arguments give equal bits, whatever computes them.
 * mon_label_components: the labelling of a host mask (mask[nx * ny * nz]) on `device`; comp, table and n_components may be NULL (table needs
 * n_components).
 * mon_scene_components_lattice: the object map's components over the lattice of mon_scene_query_lattice (the same points, sides, objects and passes).
 *   region 0, occupied matter: the mask is !(sigma <= sigma_min), sigma that call's output bit for bit -- mon_scene_distance_lattice's mask (a NaN or
 *     +inf sigma counts as occupied); clearance is ignored; dist must be NULL.  The table is the map's blobs: a main body and its floaters by size.
 *   region 1, traversable space: the mask is dist > clearance, dist being mon_scene_distance_lattice's dist for the same arguments with max_dist = +inf,
 *     bit for bit; clearance >= 0 and finite; clearance 0 gives exactly the free cells (under non-zero steps); a lattice without an occupied cell has
 *     dist = +inf everywhere and is one component.  Two cell centres can be joined by a lattice path (of the chosen connectivity) along which a sphere of
 *     radius clearance stays clear of every occupied cell centre iff their comp is equal and >= 0.
 *   dist (region 1 only), sigma and owner are those calls' rows (owner: mon_scene_query_lattice's, an index into objs or -1), each copied home only when
 *   asked for.  Mask, transform and labelling run on the device behind the query; one copy home, one synchronisation.
 * Returns:
 *   MON_ERR_ARG    everything mon_distance_transform / mon_scene_distance_lattice refuse for the arguments they share (mask, step3, origin3, objs or an
 *                  element NULL; the shape; a non-finite step or origin; sigma_min; side; n_objs; devices); label NULL; table without n_components;
 *                  connectivity not 6, 18 or 26; region not 0 or 1; region 1 with a negative or non-finite clearance; region 0 with dist -- all before
 *                  any device work, the outputs untouched
 *   MON_ERR_STATE  as mon_scene_query_lattice;   MON_ERR_NO_DEVICE  mon_label_components without a device */
typedef struct mon_lattice_component { int32_t rep; uint32_t cells; int32_t lo[3]; int32_t hi[3]; } mon_lattice_component;   /* 32 bytes */
int mon_label_components(int device, const uint8_t* mask, int nx, int ny, int nz, int connectivity,
                         int32_t* label, int32_t* comp, mon_lattice_component* table, uint32_t cap, uint32_t* n_components);
int mon_scene_components_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                                 float sigma_min, int region, float clearance, int connectivity,
                                 int32_t* label, int32_t* comp, mon_lattice_component* table, uint32_t cap, uint32_t* n_components,
                                 float* dist, float* sigma, int32_t* owner);
/* Shortest-path cost fields: how far the goal is through the space the robot may occupy, and which way to go -- the step a planner runs on the three
 * calls above after every publication (the reference has no such call; opt-in, new, read-only; no existing call changes its bits).  The field has a unique
 * definition in fp32:
 * Lattice.  The distance calls': nx x ny x nz cells, i fastest, cell (i, j, k) at flat index (k * ny + j) * nx + i, nx * ny * nz in 1 .. 2^22, step3 finite;
 *   a component of step3 may be negative or 0.
 * Graph.  A cell is passable iff its mask byte is not 0.  Two passable cells are adjacent under connectivity 6 / 18 / 26 exactly as in
 *   mon_label_components.  Nothing wraps round the border.  A diagonal move may pass between two blocked cells; the scene call's clearance is what keeps a
 *   robot off them.
 * Weights.  Every operation is a separately rounded fp32 one (fl), as in the distance rule.  For a move (di, dj, dk): a_x = (float)di * step3[0], a_y and
 *   a_z likewise; len = sqrtf(((a_x * a_x) + (a_y * a_y)) + (a_z * a_z)), the correctly rounded root: mon_distance_transform's dist between the two cells.
 *   Without cell_cost w(u, v) = len.  With cell_cost, a per-cell multiplier c that is finite and >= 0: w(u, v) = fl(len * fl(0.5f * fl(c[u] + c[v]))),
 *   symmetric in u and v.
 * Cost.  cost[v] = the least value of the left fold c_0 = 0, c_(i+1) = fl(c_i + w(p_i, p_(i+1))) over all walks p_0 .. p_k = v through passable cells that
 *   start at a seed; +inf without such a walk and on a cell outside the mask; 0 at a passable seed.  A seed on a cell outside the mask contributes nothing;
 *   duplicate seeds are allowed.  fp32 addition is monotone and fl(c + w) >= c for w >= 0, so this minimum is the fixed point that the
 *   relaxations cost[v] = min(cost[v], fl(cost[u] + w(u, v))) reach from 0 at the seeds and +inf elsewhere under any order, bit for bit: equal arguments
 *   give equal bits, whatever computes them.
 * max_cost.  > 0; +inf: no limit.  Where !(cost <= max_cost): cost = +inf and next = -1; a cell at exactly max_cost keeps its value.
 * next[v], the way to go: among the neighbours u of v, in ascending flat index, the first with cost[u] < cost[v] and fl(cost[u] + w(u, v)) == cost[v], taken
 *   on the untruncated field; -1 at seeds, on unreachable, truncated and masked-out cells, and where no such neighbour exists (only where a weight is 0 or
 *   absorbed by rounding, e.g. under a zero step).  Following next strictly lowers cost, so it ends: at a seed or at a -1.
 * mon_shortest_paths: the field of a host mask (passable[nx * ny * nz]) on `device`; cell_cost [nx * ny * nz] or NULL (1 everywhere: w = len); seeds
 *   [n_seeds] flat indices; next may be NULL.
 * mon_scene_paths_lattice: the object map's field over the lattice of mon_scene_query_lattice (the same points, sides, objects and passes).  Passable is
 *   dist > clearance, dist being mon_scene_distance_lattice's for the same arguments with max_dist = +inf, bit for bit: the mask of
 *   mon_scene_components_lattice's region 1.  soft_weight == 0: no multiplier, soft_radius is ignored.  soft_weight > 0:
 *   c[v] = fl(1 + fl(soft_weight * fl(fmaxf(0, fl(soft_radius - dist[v])) / soft_radius))): dearer near matter, 1 from soft_radius outward and where dist
 *   is +inf.  dist, sigma and owner are those calls' rows (owner: an index into objs or -1), each copied home only when asked for; all outputs but cost may
 *   be NULL.  Everything runs on the device behind the query with one copy home; the number of relaxation sweeps depends on the map, so the host reads one
 *   small word back per batch of sweeps.
 * mon_lattice_path (host only): the cells from start along next: path[0] = start, then next[start], ... up to the first -1; at most cap cells are written
 *   (path may be NULL when cap is 0); *n_path is the whole length even when cap is smaller.
 * Returns:
 *   MON_ERR_ARG    everything mon_distance_transform / mon_scene_distance_lattice and the components calls refuse for the arguments they share (mask, step3,
 *                  origin3, objs or an element NULL; the shape; a non-finite step or origin; sigma_min; side; n_objs; devices; connectivity not 6, 18 or 26);
 *                  cost or seeds NULL; n_seeds 0 or above 2^22; a seed outside 0 .. nx * ny * nz - 1; max_cost <= 0 or NaN; clearance or soft_weight
 *                  negative or not finite; soft_weight > 0 with soft_radius not finite or <= 0; mon_shortest_paths with a cell_cost entry negative or not
 *                  finite -- all before any device work, the outputs untouched.  mon_lattice_path: next or n_path NULL, start or an entry met on the walk
 *                  outside -1 .. n_cells - 1 (start: not -1), a walk longer than n_cells (a damaged array); path and n_path untouched
 *   MON_ERR_STATE  as mon_scene_query_lattice; also a field that did not settle within nx * ny * nz + 1 sweeps (Bellman-Ford cannot need more), the
 *                  outputs untouched;   MON_ERR_NO_DEVICE  mon_shortest_paths without a device, after its checks */
int mon_shortest_paths(int device, const uint8_t* passable, int nx, int ny, int nz, const float* step3, int connectivity,
                       const float* cell_cost, const int32_t* seeds, size_t n_seeds, float max_cost, float* cost, int32_t* next);
int mon_scene_paths_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                            float sigma_min, float clearance, float soft_radius, float soft_weight, int connectivity,
                            const int32_t* seeds, size_t n_seeds, float max_cost,
                            float* cost, int32_t* next, float* dist, float* sigma, int32_t* owner);
int mon_lattice_path(const int32_t* next, size_t n_cells, int32_t start, int32_t* path, size_t cap, size_t* n_path);
/* Device-resident distance fields and batched trajectory clearance: does this robot body, along these trajectories, stay clear of the map, by how much,
 * where does it first touch, and which way should it be pushed -- asked many times per map publication by a planner that samples trajectories (the
 * reference has no such call; opt-in, new, read-only; no existing call changes its bits).  A mon_dist_field is a SNAPSHOT of a distance field in device
 * memory of its own, 4 bytes per cell: it holds no reference to objects or to a manager, does not follow later training, and outlives the objects and the
 * manager it was made from; there is no cache to go stale.  Calls on one handle from several threads take turns on a mutex in the handle; different
 * handles are independent.  No atomics: equal arguments give equal bits.  Every operation below is one separately rounded fp32 operation (fl); nothing is
 * contracted.
 * Field.  D[nx * ny * nz], i fastest, cell (i, j, k) at flat index (k * ny + j) * nx + i and at world point o + (i, j, k) * s (origin3 o, step3 s),
 *   nx * ny * nz in 1 .. 2^22, every entry finite.  An axis with more than one cell has a finite step other than 0 (a negative one is fine); the step of
 *   an axis of one cell is ignored.
 * Sample of D at a world point p.  Per axis a with n_a > 1: g_a = fl(fl(p_a - o_a) / s_a); the point is inside on the axis iff 0 <= g_a <= (float)(n_a - 1)
 *   (a NaN fails); i_a = min((int)floorf(g_a), n_a - 2); f_a = fl(g_a - (float)i_a).  An axis with n_a == 1 is neither interpolated nor range-checked:
 *   i_a = 0, f_a = 0, its upper corner is the same cell and its gradient component is 0.  A point outside on any axis: d = outside, grad = 0.  Otherwise,
 *   with lerp(a, b, f) = fl(a + fl(f * fl(b - a))):
 *     along x  c_jk = lerp(D[i, j + dj, k + dk], D[i + 1, j + dj, k + dk], f_x)   (dj, dk in {0, 1}),     e_jk = fl(D[i + 1, ..] - D[i, ..])
 *     along y  c_k = lerp(c_0k, c_1k, f_y),   h_k = fl(c_1k - c_0k),   e_k = lerp(e_0k, e_1k, f_y)
 *     along z  d = lerp(c_0, c_1, f_z)
 *     grad_x = fl(lerp(e_0, e_1, f_z) / s_x),   grad_y = fl(lerp(h_0, h_1, f_z) / s_y),   grad_z = fl(fl(c_1 - c_0) / s_z)     (world units)
 * Body.  spheres[k] = { bx, by, bz, r } in the body frame, 1 <= n_spheres <= 32, offsets finite, r finite and >= 0.
 * Waypoints.  ways[n_traj][n_way][way_floats]; the values are not checked, a centre that is not finite is simply outside.
 *   way_floats 3: a position t; the centre of sphere b there is c = fl(t + b) per component (the body is not rotated).
 *   way_floats 16: a row-major 4 x 4 matrix M, the layout of Twc16, its last row ignored; c_x = fl(fl(fl(fl(M00 b_x) + fl(M01 b_y)) + fl(M02 b_z)) + M03),
 *     c_y and c_z likewise from rows 1 and 2.
 * Samples.  Each of the n_way - 1 segments gives n_sub samples and the last waypoint one more: n_samp = (n_way - 1) * n_sub + 1.  Sample q = w * n_sub + u
 *   (u < n_sub): for u == 0 the centre at waypoint w; otherwise fl(c_w + fl(tau * fl(c_(w+1) - c_w))) per component with tau = fl((float)u / (float)n_sub).
 *   1 <= n_way <= 256, 1 <= n_sub <= 16, 1 <= n_traj <= 65 536, n_traj * n_samp <= 2^24.
 * Outputs.  params = { outside, margin, safe }, all finite; clear(q, k) = fl(d - r_k), d the sample of D at the centre of sphere k at sample q.
 *   min_clear[t]       = the least clear over all q and k (every value is finite, so the order cannot matter)
 *   first_hit[t]       = the lowest q with some k where !(clear(q, k) > margin); -1 without one
 *   cost[t]            = the pairwise tree over pen(0 .. n_samp - 1): pad with +0 to the next power of two, then level by level v'[i] = fl(v[2 i] +
 *                        v[2 i + 1]) down to one value; pen(q) = the left fold over ascending k, from 0, of fl(h * h), h = fmaxf(0, fl(safe - clear(q, k)))
 *   way_clear[t][w]    = the least clear(w * n_sub, k) over k
 *   way_grad[t][w][3]  = the gradient of D at the centre of the lowest k that attains it; 0 0 0 when that centre is outside
 * mon_dist_field_create: uploads a host field to `device`, as mon_marching_cubes serves density lattices.
 * mon_scene_dist_field: mon_scene_distance_lattice's chain (the same sides, objects, points and passes) with dist kept in the handle's buffer: the handle's
 *   cells are that call's dist for the same arguments bit for bit, and nothing per cell is copied home.  max_dist must be FINITE here, so that every value
 *   lies in [0, max_dist].
 * mon_dist_field_info: shape, origin, step, logical device and the largest value held.  mon_dist_field_read: the cells, dist_out[nx * ny * nz].
 * mon_dist_field_sample: d (dist_out[n]) and grad (grad3_out[n][3], may be NULL) at xyz[n][3], 1 <= n <= 2^24; `outside` is returned as given.
 * mon_dist_field_score: every output but min_clear may be NULL.  ways and spheres are uploaded per call; the outputs come home with one synchronisation.
 * mon_dist_field_destroy: frees the handle and its device memory (NULL: nothing to do).
 * Returns:
 *   MON_ERR_ARG    field, dist, origin3, step3, objs or an element, xyz, dist_out, info, spheres, ways, params or min_clear NULL; the shape as the distance
 *                  calls refuse it; a field entry or an origin that is not finite; an axis of more than one cell with a step that is 0 or not finite (the
 *                  scene calls also refuse what mon_scene_distance_lattice refuses: any non-finite step, a lattice that leaves the finite floats,
 *                  sigma_min, side, n_objs, objects on different logical devices); max_dist not finite or <= 0; n 0 or above 2^24; n_spheres, n_way, n_sub,
 *                  n_traj or n_traj * n_samp outside their limits; way_floats not 3 or 16; a sphere that is not finite or has r < 0; a param that is not
 *                  finite -- all before any device work, the outputs and *field untouched
 *   MON_ERR_STATE  as mon_scene_query_lattice;   MON_ERR_NO_DEVICE  mon_dist_field_create without a device, after its checks */
typedef struct mon_dist_field mon_dist_field;
typedef struct mon_dist_field_desc { int32_t nx, ny, nz, device; float origin[3]; float step[3]; float max_value; } mon_dist_field_desc;   /* 44 bytes */
typedef struct mon_traj_score_params { float outside, margin, safe; } mon_traj_score_params;
int mon_dist_field_create(int device, const float* dist, int nx, int ny, int nz, const float* origin3, const float* step3, mon_dist_field** field);
int mon_scene_dist_field(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                         float sigma_min, float max_dist, mon_dist_field** field);
int mon_dist_field_info(mon_dist_field* field, mon_dist_field_desc* info);
int mon_dist_field_read(mon_dist_field* field, float* dist_out);
int mon_dist_field_sample(mon_dist_field* field, const float* xyz, size_t n, float outside, float* dist_out, float* grad3_out);
int mon_dist_field_score(mon_dist_field* field, const float* spheres, size_t n_spheres, const float* ways, int way_floats, size_t n_traj, size_t n_way,
                         size_t n_sub, const mon_traj_score_params* params, float* min_clear, int32_t* first_hit, float* cost, float* way_clear,
                         float* way_grad);
int mon_dist_field_destroy(mon_dist_field* field);
/* Signed, sub-cell distance fields: the distance to the SURFACE of the map's density, negative inside matter -- the field the consumers of a
 * mon_dist_field (sample, score, match, register, trace, beam_score) work best on.  The transform of a mask (mon_distance_transform) measures to cell
 * centres, carries the mask's half-cell ambiguity and has no inside; this one measures to the level set val = iso placed inside the lattice edges, and
 * gives a sign (the reference has no such call; opt-in, new, read-only; no existing call changes its bits).  Exact over its candidates, separable and
 * bit-reproducible as the distance transform is.  The lattice, the flat index flat(i, j, k) = (k * ny + j) * nx + i and step3 are
 * mon_distance_transform's.  Every operation is one separately rounded fp32 operation (fl); nothing is contracted.
 *   Inside.    inside(c) = !(val[c] <= iso): a NaN or +inf counts as inside, the conservative reading the mask takes.
 *   Crossing.  Edge (q, a) joins cell q to its neighbour q + e_a along axis a, both in the lattice.  It carries a crossing iff the two cells differ in
 *              inside.  With v0 = val[q], v1 = val[q + e_a]: f = fl(fl(iso - v0) / fl(v1 - v0)), an IEEE division; if !(f >= 0 && f <= 1) then f = 0.5
 *              (which arises from infinite and NaN values only).  The crossing lies at q + f e_a.
 *   Seed pass along a.  For cell p on a line of axis a: u_a(p) = the least fl(t t) over the crossing edges (q, a) of that line,
 *              t = fl(fl((float)(p_a - q_a) - f) * step[a]); candidates in ascending q, a strictly smaller one replaces; the site is 3 * flat(q) + a.
 *              Without a crossing on the line: +inf, site -1.  An axis of one cell has no edges.
 *   Two plain passes over the other two axes, in ascending axis order, each mon_distance_transform's minimisation from values:
 *              out(p) = the least fl(fl(fl((float)(p - q) * step)^2) + in(q)) over q, candidates in ascending q along the pass's axis, a strictly smaller
 *              one replaces, the site below a candidate is carried along.  That gives w_a; rounding being monotone, w_a is the minimum over ALL crossings
 *              of axis a of the nested expression (for a = x: fl(fl(t_x^2 + a_y^2) + a_z^2); for y: fl(fl(t_y^2 + a_x^2) + a_z^2); for z:
 *              fl(fl(t_z^2 + a_x^2) + a_y^2)), bit for bit.
 *   Combine.   d2 = w_x, then w_y, then w_z: a strictly smaller one replaces and brings its site.
 *   Finish.    d = sqrt(d2), the correctly rounded root.  Where !(d <= max_dist): d = max_dist and nearest_edge = -1 (a cell at exactly max_dist keeps
 *              its edge).  sdist = inside ? -d : d.  A lattice without a crossing gives -max_dist / +max_dist everywhere.
 * No atomics: equal arguments, equal bits; a cell's outputs depend on val, iso, the shape and the steps alone.  The crossings are points, not a surface
 * between them: near a convex edge of a box the field is off by up to about 0.9 cell; on a smooth surface by about 0.2 cell rms.
 * mon_signed_distance_transform: the transform of host values val[nx * ny * nz] on `device`; sdist[nx * ny * nz]; nearest_edge may be NULL.
 * mon_scene_signed_distance_lattice: the object map's field over the lattice of mon_scene_query_lattice (the same points, sides, objects and passes).
 *   inside = !(sigma <= sigma_min) on that call's sigma, bit for bit mon_scene_distance_lattice's mask, whatever the flags.  The interpolated values:
 *   without flags val = sigma and iso = sigma_min; with MON_SIGNED_LOG val = logf(sigma) and iso = logf(sigma_min), formed on the device by one function
 *   (a density is an exponential of the network's output, so a crossing placed linearly in sigma is biased towards the empty cell by about 0.2 cell;
 *   in log density it is not).  logf(0) = -inf gives f = 0.5, the right answer at a box face, where the density is cut; sigma_min = 0 is allowed.
 *   Outputs per cell (all but sdist may be NULL): sdist; nearest_edge; nearest_owner = mon_scene_query_lattice's owner at the INSIDE end of the nearest
 *   edge (-1 without an edge); sigma; val; and iso_out[1] -- val and iso_out bring home the values the device formed, so that
 *   mon_signed_distance_transform(val, iso_out[0]) reproduces sdist and nearest_edge wherever the side read from val agrees with the side read from sigma.
 * mon_scene_signed_dist_field: the same chain with sdist kept in a mon_dist_field, nothing per cell copied home; an ordinary handle, which every
 *   mon_dist_field_* call takes as it takes any other.  max_dist must be FINITE here, so that every value lies in [-max_dist, max_dist];
 *   mon_dist_field_info's max_value is the largest value, not the largest magnitude.
 * Returns:
 *   MON_ERR_ARG    what mon_distance_transform / mon_scene_distance_lattice / mon_scene_dist_field refuse for the arguments they share; val or sdist NULL;
 *                  iso NaN; a flag bit other than MON_SIGNED_LOG -- all before any device work, the outputs and *field untouched
 *   MON_ERR_STATE  as mon_scene_query_lattice;   MON_ERR_NO_DEVICE  mon_signed_distance_transform without a device */
#define MON_SIGNED_LOG 1u
int mon_signed_distance_transform(int device, const float* val, float iso, int nx, int ny, int nz, const float* step3, float max_dist,
                                  float* sdist, int32_t* nearest_edge);
int mon_scene_signed_distance_lattice(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                                      float sigma_min, uint32_t flags, float max_dist, float* sdist, int32_t* nearest_edge, int32_t* nearest_owner,
                                      float* sigma, float* val, float* iso_out);
int mon_scene_signed_dist_field(mon_object* const* objs, size_t n_objs, int side, const float* origin3, const float* step3, int nx, int ny, int nz,
                                float sigma_min, uint32_t flags, float max_dist, mon_dist_field** field);
/* Scan matching against a device-resident distance field: where is this scan in the map -- asked by a consumer that brings only geometry (a lidar, a depth
 * camera whose frames are not in a dataset, a second robot that loaded a saved map), where every other localisation call is photometric (the reference has no
 * such call; opt-in, new, read-only; no existing call changes its bits).  One batched evaluation serves a particle filter's likelihood-field weights (the
 * cost per pose) and a Gauss-Newton / Levenberg-Marquardt refinement (the cost and the 6 x 6 normal equations); the field is best a SIGNED distance
 * (mon_dist_field_create), whose zero set the scan's end points lie on.  Every operation below is one separately rounded fp32 operation (fl); nothing is
 * contracted.  No atomics: equal arguments give equal bits, and a pose's row does not depend on the other poses of the call.
 * Inputs.  points[n][3], the scan in the sensor or body frame; the values are not checked: a point that lands outside the lattice, or is not finite, is
 *   simply "outside".  poses16[H][16]: row-major 4 x 4 matrices, the layout of Twc16, the last row ignored, which map the points into the field's world;
 *   the twelve entries used are finite.  pivots[H][3], finite, or NULL for (0, 0, 0).  params = { huber, outside }: huber > 0, +inf is allowed; outside is
 *   finite.  1 <= n <= 2^20, 1 <= H <= 4 096, n * H <= 2^26.
 * Per pose h and point p.
 *   1. q = the centre formula of way_floats 16 above, applied to poses16[h] and points[p].
 *   2. (d, g) = the sample of D at q and its gradient, by the rule above.
 *   3. q outside: d = outside, every A and b term of the point is +0 (not computed), inside = 0.
 *   4. Otherwise a = fl(q - pivot) per component, and
 *        J = (g_x, g_y, g_z, fl(fl(a_y g_z) - fl(a_z g_y)), fl(fl(a_z g_x) - fl(a_x g_z)), fl(fl(a_x g_y) - fl(a_y g_x))),
 *      the derivative of d under pose <- Exp(v, w) about the pivot, translation first: R' = Exp(w) R, t' = Exp(w) (t - pivot) + pivot + v.
 *   5. m = |d|.  Where m <= huber: w = 1, rho = fl(d d), and the point is an inlier if it is inside.  Otherwise w = fl(huber / m) and
 *      rho = fl(huber * fl(fl(2 m) - huber)).
 *   6. A_ij = fl(fl(w J_i) J_j) for i <= j (21 terms, row-major upper triangle), b_i = fl(fl(w J_i) d) (6 terms), and rho (one term).  An outside point
 *      contributes its rho too, so a pose cannot lower its cost by leaving the lattice.
 * Sums.  Each of the 28 float sums of a pose is the pairwise tree over the points in ascending index: pad with +0 to the next power of two, then level by
 *   level v'[i] = fl(v[2 i] + v[2 i + 1]) down to one value; a result of -0 is returned as +0.  n_inside and n_inlier are integer counts.
 * mon_dist_field_match: cost[H]; n_inside[H] and n_inlier[H] (either may be NULL); normal[H][27] = the 21 A terms, then the 6 b terms (may be NULL: nothing
 *   of A and b is then computed -- the particle filter's case).  Points, poses and pivots are uploaded per call; the outputs come home with one
 *   synchronisation.
 * mon_register_default: huber = 2 x the largest |step| among the axes of more than one cell (1 without such an axis), outside = the handle's max_value,
 *   max_evals 30, lambda0 1e-3, lambda_up = lambda_down = 10, lambda_max 1e6, tol_trans = 1e-3 x that step, tol_rot 1e-4, min_inside 6.
 * mon_dist_field_register: every one of the H hypotheses poses16_in is refined by Levenberg-Marquardt, all in lockstep: the points are uploaded once; per
 *   round there is one match launch over the hypotheses still running and one read-back of 32 words per pose.  The pivot c of a hypothesis is its input pose
 *   applied to the centroid of the scan's finite points, and stays fixed.  The first round evaluates the input poses.  Then, per hypothesis: the host solves
 *   (A + lambda diag(A)) delta = -b in double by a Cholesky factorisation (a failed one counts as a rejected step), forms R' = Exp(w) R and
 *   t' = Exp(w) (t - c) + c + v with delta = (v, w), rounds to fp32 and has the candidate evaluated.  A step is accepted iff its cost is strictly lower;
 *   lambda is divided by lambda_down on acceptance and multiplied by lambda_up on rejection.  The host's double steps are not pinned bit for bit by this
 *   text, but equal calls give equal bits, and a hypothesis's result does not depend on the others.
 *   Outputs: poses16_out[H][16] (the last row is the input's) and cost[H]; and, each of which may be NULL: n_inside[H], n_inlier[H] (cost and counts are
 *   mon_dist_field_match's at the returned pose with the hypothesis's pivot, bit for bit), evals[H] (the match evaluations of that hypothesis, the first
 *   included), status[H] (0: an accepted step with |v| < tol_trans and |w| < tol_rot; 1: max_evals reached; 2: lambda above lambda_max; 3: fewer than
 *   min_inside points inside at the input pose, which is returned bit for bit) and *best (the index of the lowest cost among status != 3, ties to the
 *   lowest index; -1 without one).
 * Returns:
 *   MON_ERR_ARG    field, points, poses16, params, cost, poses16_in, poses16_out or p NULL; n, H or n * H outside their limits; a pose entry or a pivot
 *                  that is not finite; huber <= 0 or NaN; outside, a lambda parameter or a tolerance that is not finite; lambda0 <= 0, lambda_max <= 0 or
 *                  a tolerance < 0; lambda_up or lambda_down <= 1; max_evals < 1; min_inside < 0 -- all before any device work, the outputs untouched; the
 *                  handle is judged last */
typedef struct mon_scan_match_params { float huber, outside; } mon_scan_match_params;
typedef struct mon_register_params { float huber, outside; int32_t max_evals; float lambda0, lambda_up, lambda_down, lambda_max, tol_trans, tol_rot;
                                     int32_t min_inside; } mon_register_params;      /* 40 bytes */
int mon_dist_field_match(mon_dist_field* field, const float* points, size_t n, const float* poses16, size_t n_poses, const float* pivots,
                         const mon_scan_match_params* params, float* cost, int32_t* n_inside, int32_t* n_inlier, float* normal);
int mon_register_default(mon_dist_field* field, mon_register_params* p);
int mon_dist_field_register(mon_dist_field* field, const float* points, size_t n, const float* poses16_in, size_t n_poses, const mon_register_params* p,
                            float* poses16_out, float* cost, int32_t* n_inside, int32_t* n_inlier, int32_t* evals, int32_t* status, int32_t* best);
/* Ray tracing against a device-resident distance field: what range scan would a sensor at this pose see, is there a line of sight between two points, and
 * how well do predicted ranges under several thousand pose hypotheses agree with measured ones -- the forward direction of the scan matching above, for a
 * consumer that holds only a mon_dist_field (the reference has no such call; opt-in, new, read-only; no existing call changes its bits).  The rays are
 * sphere-traced: the sampled distance bounds the free way ahead.  The field is best a SIGNED distance (mon_dist_field_create).  Every operation below is one
 * separately rounded fp32 operation (fl); nothing is contracted.  No atomics: equal arguments give equal bits, and a ray's row does not depend on the other
 * rays or poses of the call.
 * Inputs.  rays[n][6] = origin o and direction u in the sensor frame; the values are not checked.  The direction is used as given and t is in units of its
 *   length: pass unit directions.  poses16[H][16] as in mon_dist_field_match: the twelve entries used are finite, the last row is ignored.  poses16 may be
 *   NULL: then n_poses must be 1 and the rays are world rays used as given, with no arithmetic.  1 <= n <= 2^20, 1 <= H <= 4 096; n * H <= 2^22 for
 *   mon_dist_field_trace, whose outputs are [H][n] and come home; n * H <= 2^24 for mon_dist_field_beam_score, which brings home H words per output.
 *   params = { t_min, t_max, eps, step_min, relax, step_outside, max_steps }: all finite, t_min <= t_max, step_min > 0, step_outside > 0, 0 < relax <= 1,
 *   1 <= max_steps <= 4 096.
 * Per pose h and ray r.
 *   1. a = the centre formula of way_floats 16 above applied to poses16[h] and o.  w_x = fl(fl(fl(M00 u_x) + fl(M01 u_y)) + fl(M02 u_z)), w_y and w_z
 *      likewise from rows 1 and 2: the translation is not added.
 *   2. point(t) = fl(a + fl(t * w)) per component.
 *   3. Start with t = t_min, k = 0, seen_inside = false.  Repeat:
 *        if !(t <= t_max): status 1 (passed), range = t_max; end.
 *        if k == max_steps: status 2 (out of steps), range = t; end.
 *        sample D at point(t) by the rule above: d; k += 1.
 *        outside the lattice, seen_inside set: status 3 (left: the lattice is convex), range = t_prev; end.
 *        outside, seen_inside clear: t = fl(t + step_outside) and continue; nothing is remembered as previous.
 *        inside: seen_inside = true.  If d <= eps: status 0 (hit); without a previous inside sample range = t, otherwise
 *          range = fl(t_prev + fl(fl(t - t_prev) * fl(fl(d_prev - eps) / fl(d_prev - d)))),
 *        the crossing of the level eps between the last two samples (both differences are positive, so nothing needs a clamp); end.
 *        Else t_prev = t, d_prev = d, t = fl(t + fmaxf(fl(relax * d), step_min)).
 *   4. steps = k.  normal3 = the gradient of D by the sample rule at point(range) on a hit; 0 0 0 on any other status or when that point is outside.
 *   Trilinear interpolation of a 1-Lipschitz field has a gradient norm of up to sqrt 3, so relax <= 0.57 cannot step through a surface; a larger relax is
 *   for fields known to be smoother.
 * mon_trace_default: with c the smallest |step| among the axes of more than one cell (1 without such an axis): t_min 0, t_max = sqrtf of the left fold over
 *   x, y, z of fl(e_a e_a), e_a = fl((float)(n_a - 1) * |s_a|) (the lattice's diagonal), eps = c / 8, step_min = c / 4, relax 0.5, step_outside = c / 2,
 *   max_steps 256.
 * mon_dist_field_trace: range[H][n]; status[H][n], steps[H][n] and normal3[H][n][3], each of which may be NULL (what was not asked for is neither computed
 *   beyond the march nor copied home).  Rays and poses are uploaded per call; the outputs come home with one synchronisation.
 * mon_dist_field_beam_score: measured[n], a NaN marks a beam without a return: its term is +0 and it is not valid.  Per pose and valid beam
 *   e = fl(range - measured), range exactly what mon_dist_field_trace returns for that pose and ray, whatever its status; rho and the Huber split on
 *   m = |e| are step 5 of the scan matching above with beam = { huber }.  cost[H] is ONE pairwise tree over the beams in ascending index, padded with +0 to
 *   a power of two; -0 is returned as +0.  n_valid[H] and n_hit[H] (the valid beams with status 0) are integer counts; either may be NULL.  The ranges stay
 *   on the device.
 * Returns:
 *   MON_ERR_ARG    field, rays, params, range, measured, beam or cost NULL; n, H or n * H outside their limits; poses16 NULL with H != 1; a used pose entry
 *                  that is not finite; t_min, t_max, eps, step_min, relax or step_outside not finite; t_min > t_max; step_min <= 0 or step_outside <= 0;
 *                  relax <= 0 or > 1; max_steps outside 1 .. 4 096; huber <= 0 or NaN (+inf is allowed) -- all before any device work, the outputs
 *                  untouched; the handle is judged last */
typedef struct mon_trace_params { float t_min, t_max, eps, step_min, relax, step_outside; int32_t max_steps; } mon_trace_params;   /* 28 bytes */
typedef struct mon_beam_params { float huber; } mon_beam_params;
int mon_trace_default(mon_dist_field* field, mon_trace_params* p);
int mon_dist_field_trace(mon_dist_field* field, const float* rays, size_t n, const float* poses16, size_t n_poses, const mon_trace_params* p,
                         float* range, int32_t* status, int32_t* steps, float* normal3);
int mon_dist_field_beam_score(mon_dist_field* field, const float* rays, size_t n, const float* measured, const float* poses16, size_t n_poses,
                              const mon_trace_params* p, const mon_beam_params* b, float* cost, int32_t* n_valid, int32_t* n_hit);
/* Object pose refinement through the trained field (iNeRF-style): align the object with observed frames by following the gradient of a photometric,
 * silhouette and depth error with respect to the 6-DoF pose Tow.
 * Objective.  obs names frames of the object's dataset (FrameId) and pixel boxes inside them; the target of a pixel is that frame's rgb c*, its instance map
 * m* = (instance == class_id) and its depth d* (0 where the dataset has none); the camera is the frame's Twc.  For each drawn pixel, the ray
 * mon_object_render builds for it under the Tow evaluated, intersected with the object's box, and its 2S = 64 jittered distances t_k -- rays_per_iter = 0:
 * the render's own jitter, so that at the object's own Tow the samples, alpha and colour of each box are those of mon_debug_scene_samples for that box;
 * rays_per_iter > 0: counter-RNG stream 4 keyed by (seed, iteration, ray * 2S + k), the pixels drawn uniformly over the union of the boxes' pixels by
 * stream 5 keyed by (seed, iteration, ray): with z that key's 64-bit mix (rand01's top 24 bits are z >> 40) and `total` the union's pixels (box b holds
 * [prefix[b], prefix[b + 1]), box order, then row-major), pixel p = ((z >> 40) total) >> 24 for total <= 2^24 and ((z >> 32) total) >> 32 above, so
 * that every pixel of a union of up to 2^28 can be drawn.  Alpha and colour as the render computes them (sigma = exp(o3), c = logistic(o0..2), alpha_k = 1 - exp(-sigma_k
 * dt_k), the first interval from 0, the early cut at T < 1e-4):
 *   w_k = alpha_k T_k, T_end what remains; r = sum_k w_k (c_k - c*) (the background counts as the target colour); O = 1 - T_end;
 *   D = sum_k w_k t_k / |camera ray|
 *   l = w_rgb m* |r|^2 / 3 + w_mask (O - m*)^2 + w_depth m* [d* > 0] Huber(D - d*),
 *   Huber(x) = x^2 / 2 for |x| <= depth_huber, else depth_huber (|x| - depth_huber / 2)
 *   L = mean of l over the drawn pixels (a ray that misses the box counts with O = D = r = 0)
 * grad6 = dL/dxi at xi = 0 for Tow(xi) = exp(xi^) Tow, xi = (rho, phi), translation first.  Sample positions move as x_k(xi) = exp(xi^) x_k; every t_k and
 * dt_k, the box intersection, the early cut and the hash-grid corners of each sample are held at their values at Tow -- only the trilinear weights inside the
 * cell are differentiated: dL/drho = sum_k g_k, dL/dphi = sum_k x_k x g_k, g_k = dL/dx_k in the object frame.
 * Refinement: Adam (0.9, 0.999, 1e-8) on the twist, lr_trans for rho and lr_rot for phi; each step Tow <- exp(delta^) Tow (closed-form SE(3) exponential,
 * fp32), the rotation re-orthonormalised.  Step i evaluates with iteration = i.  Every sample is evaluated: render skipping does not apply.
 * Defaults (mon_pose_refine_default; step sizes and step count measured on the synthetic scene): iters 100, rays_per_iter 4096,
 * lr_trans 2e-3, lr_rot 4e-3, w_rgb 1, w_mask 1, w_depth 1, depth_huber 0.05, seed 1.
 * (8-level grid at per-level scale 1.5, 5 degrees / 5 % of the box diagonal off: 0.12-0.15 degrees and <= 0.09 % after 100 steps; lr 1e-3 / 2e-3 over 200
 * steps and 5e-3 / 1e-2 over 100 were no better.  On base.json's 16-level grid the gradient does not point downhill on the pose's scale: DESIGN.md 3.4d.)
 * Read-only: nothing about the object changes (parameters, training state and RNG counters, render-skip caches and statistics, snapshot, mesh, its own Tow);
 * the pose goes back to the caller only.  side as in mon_scene_render: 0 the train-side weights (EMA once trained) on the train stream, the caller
 * serialises against training; 1 the published snapshot on the inference stream, callable while the object trains.  Each side has its own scratch.
 * Returns MON_ERR_ARG for NULL obj / obs / pose / params, n_obs 0, iters < 0, side not 0 / 1, rays_per_iter above 2^22, a FrameId the dataset does not hold,
 * a box empty or outside its frame, boxes holding more than 2^28 pixels together, more than 2^22 of them with rays_per_iter = 0 (checked before any device
 * work); MON_ERR_STATE for objects outside the fused shapes, the XORWOW render mode, and side 1
 * with nothing published. */
typedef struct mon_pose_refine_params {
    int      iters;          /* Adam steps of mon_object_refine_pose (>= 0)                                                                         */
    uint32_t rays_per_iter;  /* pixels drawn per evaluation, uniformly over the union of the boxes' pixels; 0 = every pixel of every box, in box order
                                then row-major (no randomness)                                                                                        */
    float    lr_trans;       /* Adam step size of the twist's translation part (object-frame units)                                                */
    float    lr_rot;         /* Adam step size of the twist's rotation part (radians)                                                               */
    float    w_rgb, w_mask, w_depth, depth_huber;   /* loss weights, Huber width of the depth term (metres)                                        */
    uint64_t seed;           /* pixel draws and sample jitter of rays_per_iter > 0                                                                  */
} mon_pose_refine_params;
int mon_pose_refine_default(mon_pose_refine_params* p);
/* One evaluation at pose Tow16 (column-major, world -> object, as mon_object_create's): loss and dL/dxi (grad6 = rho, phi; either may be NULL) */
int mon_object_pose_loss(mon_object* obj, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16, const mon_pose_refine_params* p,
                         uint32_t iteration, float* loss, float* grad6);
/* p->iters Adam steps from *Tow16_inout; writes the final pose back; loss_trace[iters + 1] (may be NULL): the loss before each step and at the end.  The
 * whole refinement is enqueued at once (the pose lives on the device between steps); the call returns when it is done. */
int mon_object_refine_pose(mon_object* obj, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p, float* Tow16_inout,
                           float* loss_trace);
/* Coarse-to-fine pose refinement: the objective L, its samples, alpha, colour, the early cut and the held hash-grid corners are exactly
 * those of mon_object_pose_loss; only the gradient is re-weighted by level.
 * Level-weighted gradient.  g_k = sum_l g_{k,l}, g_{k,l} = level l's term of dL/dx_k (dL/dE_l . dfeat_l/dx over the 8 corners, times the level's scale,
 * over the box extent).  For weights w_0..w_{L-1} >= 0: g_k(w) = sum_l w_l g_{k,l}, grad6(w) = (sum_k g_k(w), sum_k x_k x g_k(w)).  The loss does not depend
 * on w; every w_l = 1 gives grad6 of mon_object_pose_loss bit for bit, every w_l = 0 gives grad6 = 0.
 * Window (BARF; alpha in levels, level 0 the coarsest): w_l(alpha) = 0 for alpha <= l, (1 - cos(pi (alpha - l))) / 2 for l < alpha < l + 1, 1 for
 * alpha >= l + 1.
 * Schedule: step i of an iters-step refinement uses alpha(i) = level_start + (level_end - level_start) min(1, i / (ramp iters)); everything else is
 * mon_object_refine_pose's (Adam on the twist, Tow <- exp(delta^) Tow, Gram-Schmidt, loss_trace[i] the loss before step i and loss_trace[iters] at the
 * end; iters 0 takes no step).
 * C2F defaults (mon_pose_c2f_default; chosen by a sweep on base.json objects of the synthetic scene, profiles/r09_pose_c2f.md): level_start 4, level_end 5,
 * ramp 0.7.
 * (base.json, 500 or 2000 training iterations, 100 default steps: 5 degrees / 5 % and 15 degrees / 10 % of the box diagonal off end at 0.12-0.33 degrees and
 * <= 0.15 %, where plain mon_object_refine_pose drifts away; the floor is Adam's step, lr_rot = 0.23 degrees.)
 * Returns MON_ERR_ARG, before any device work, for a NULL c or level_weights, a non-finite parameter or weight, level_start < 0, level_end < level_start,
 * ramp outside (0, 1], a negative weight, and everything mon_object_pose_loss / mon_object_refine_pose reject; MON_ERR_STATE as they do.  Read-only. */
typedef struct mon_pose_c2f_params {
    float level_start;   /* alpha at step 0 (>= 0)                                                                                                   */
    float level_end;     /* alpha from the end of the ramp on (>= level_start; values >= L weight every level 1)                                     */
    float ramp;          /* fraction of p->iters over which alpha rises linearly, (0, 1]                                                             */
} mon_pose_c2f_params;
int mon_pose_c2f_default(mon_pose_c2f_params* c);
/* host-only: w[0..n_levels) of step `step` of an `iters`-step refinement (the window and schedule above); MON_ERR_ARG for iters < 1 or step outside
 * [0, iters) as well */
int mon_pose_c2f_weights(const mon_pose_c2f_params* c, int n_levels, int iters, int step, float* w);
/* mon_object_pose_loss with the level weights w[0..L) of the object (L = its n_levels) */
int mon_object_pose_loss_levels(mon_object* obj, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Tow16,
                                const mon_pose_refine_params* p, uint32_t iteration, const float* level_weights, float* loss, float* grad6);
/* mon_object_refine_pose with the schedule: step i uses mon_pose_c2f_weights(c, L, p->iters, i).  Still enqueued at once, one synchronisation. */
int mon_object_refine_pose_c2f(mon_object* obj, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p,
                               const mon_pose_c2f_params* c, float* Tow16_inout, float* loss_trace);
/* Camera pose refinement against a scene of object NeRFs (the reference has no such call; opt-in, new): given a frame of the dataset and a
 * predicted camera pose, follow the gradient of one photometric, silhouette and depth error of everything the object map holds with respect to Twc.
 * Inputs.  objs[0..K): objects of one logical device and one dataset (equal intrinsics), fused shapes only, K <= 256; each uses its own Tow and box.  obs:
 * boxes that all name the same FrameId.  A candidate camera pose Twc16 (column-major, camera -> world).  Targets of pixel (x, y) of that frame: colour c*,
 * instance id i*, depth d* (0 without depth); m*_j = [i* == class_id_j], M* = max_j m*_j.
 * Rays.  Pixels are drawn exactly as mon_object_pose_loss draws them (the union of the boxes, box order then row-major, stream 5 keyed (seed, iteration, ray),
 * the 24- / 32-bit rule; rays_per_iter = 0 takes every pixel).  The world ray is the one mon_object_render builds for that pixel under the candidate Twc.  Per
 * object j: the ray in j's frame under its Tow, its intersection with j's box, and 2S = 64 jittered distances t_{j,k} in [max(t0_j, 0), t1_j] --
 * rays_per_iter = 0: object j's own render jitter (sample_seed_j, stream 3, index q * 64 + k, q the pixel inside its box), so that at the dataset's own Twc
 * each object's t, alpha and colour for a box are those of mon_debug_scene_samples for that box as rect; rays_per_iter > 0: stream 4 keyed (seed, iteration,
 * ray * 64 + k), the same draw for every object.  Alpha and colour are the render's (sigma = exp(o3), c = logistic(o0..2), alpha = 1 - exp(-sigma dt), the
 * first interval from 0).  Each object evaluates its second 32-sample tile only if its own transmittance after the first is >= 1e-4.  Render skipping does not
 * apply.
 * Composite (mon_scene_render's).  All evaluated samples of the ray are merged by t; ties go to the lower index in objs, then the lower slot.  T_0 = 1,
 * w_i = alpha_i T_i, T_{i+1} = T_i (1 - alpha_i); the first merged sample with T_i < 1e-4 and everything behind it get weight 0.
 * Loss.  r = sum_i w_i (c_i - c*); W_j = sum_{i in j} w_i; D = sum_i w_i t_i / |camera ray|;
 *   l = w_rgb M* |r|^2 / 3 + w_mask sum_{j < K} (W_j - m*_j)^2 + w_depth M* [d* > 0] Huber(D - d*)
 *   L = mean of l over the drawn pixels (an object the ray misses has W_j = 0 and still counts in the mask sum).
 * With K = 1 this is mon_object_pose_loss's l term for term (W_0 = O, M* = m*).
 * Gradient.  grad6 = dL/dxi at xi = 0 for Twc(xi) = Twc exp(xi^) -- a camera-frame (right) perturbation, xi = (rho, phi), translation first.  A sample's
 * camera-frame position x_c = t (unit camera ray) is rigid; its object-frame position is x_o = Toc_j exp(xi^) x_c with Toc_j = Tow_j Twc.  Held at their
 * values at xi = 0: every t and dt, each box intersection, the merge order, both cuts and each sample's hash-grid corners; only the trilinear weights are
 * differentiated (mon_object_pose_loss's rule).  dL/drho = sum g_c, dL/dphi = sum x_c x g_c with g_c = R_oc,j^T g_o and g_o = dL/dx_o of the sample;
 * computed per object as G_j = (sum g_o, sum x_o x g_o) in the object frame and mapped with Toc_j = (R, p): grad_rho = sum_j R^T G_j,rho,
 * grad_phi = sum_j R^T (G_j,phi - p x G_j,rho), the sum over j in index order.  Composite backward in merged order, with
 * q_i = G_rgb . (c_i - c*) + G_D t_i + 2 w_mask (W_j(i) - m*_j(i)): dL/dsigma_i = dt_i (T_{i+1} q_i - sum_{n > i} w_n q_n), dL/dc_i = w_i G_rgb; there is no
 * separate T_end term (opacity enters only through the W_j).
 * Level weights (mon_object_pose_loss_levels's, by level index): object j uses level_weights[0..L_j); NULL = every weight 1.  Weights of 1 give the
 * unweighted result bit for bit, weights of 0 give grad6 = 0 exactly; the loss does not depend on them.
 * Refinement.  Adam (0.9, 0.999, 1e-8) on the twist, lr_trans / lr_rot; each step Twc <- Twc exp(delta^) in closed form, the rotation re-orthonormalised
 * (Gram-Schmidt).  Step i evaluates with iteration = i; loss_trace[i] (iters + 1 values, may be NULL) is the loss before step i, loss_trace[iters] the loss
 * at the end.  With a schedule c, step i uses mon_pose_c2f_weights(c, Lmax, iters, i), Lmax the largest n_levels in objs; c = NULL: plain.  The whole
 * refinement is enqueued at once (the pose lives on the device between steps), one synchronisation.  No atomics: equal arguments give equal bits.
 * Read-only.  Nothing about any object, the dataset or a manager changes (parameters, training state, RNG counters, render-skip caches and statistics,
 * snapshots, the objects' pose scratch, the dataset's stored pose): the pose goes back to the caller only, who calls mon_online_update_dataset to store it.
 * side as in mon_scene_render: 0 the train-side weights on the first object's train stream (the caller serialises against training), 1 the pinned snapshots
 * on the device's inference stream (callable while the objects train).
 * Returns MON_ERR_ARG, before any device work, for everything mon_object_pose_loss / mon_object_refine_pose / mon_object_refine_pose_c2f reject, n_objs 0 or
 * above 256, a NULL element of objs, boxes naming different FrameIds, objects on different logical devices, with different intrinsics or on different
 * datasets; MON_ERR_STATE for an object outside the fused shapes, the XORWOW render mode, and side 1 with nothing published. */
int mon_scene_pose_loss(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16,
                        const mon_pose_refine_params* p, uint32_t iteration, const float* level_weights /* NULL or Lmax */, float* loss, float* grad6);
int mon_scene_refine_camera(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p,
                            const mon_pose_c2f_params* c /* NULL: plain */, float* Twc16_inout, float* loss_trace);
/* ---- wide-basin relocalisation: many candidate camera poses scored in one enqueue, the best few refined.
 * mon_scene_pose_loss_batch.  losses[h] (n_poses floats) is, bit for bit, the loss mon_scene_pose_loss(objs, n_objs, side, obs, n_obs, Twc16s + 16 h, p,
 * iteration, NULL, &loss, NULL) returns -- for every h, whatever else the batch holds and wherever in it the pose stands.  Pixels and jitter are keyed by
 * (seed, iteration, ray), not by the pose: every hypothesis sees the same pixels and targets, only the rays differ.  Forward only: no gradient, no level
 * weights, no Adam step.  Read-only and `side` exactly as mon_scene_pose_loss (side 1 pins each object's snapshot once for the whole batch).  The call is
 * enqueued at once -- passes of floor(16384 / n) hypotheses of n rays each, K + 3 launches per pass for K objects, in the list workspace of one
 * evaluation -- with one synchronisation and one copy home of n_poses floats.  No atomics: equal arguments give equal bits.
 * Returns MON_ERR_ARG, before any device work, for n_poses outside 1..4096, a NULL Twc16s or losses, more than 16384 rays per hypothesis (rays_per_iter
 * above 16384, or rays_per_iter = 0 with boxes of more than 16384 pixels together: a hypothesis is never split across passes) and everything
 * mon_scene_pose_loss rejects; MON_ERR_STATE as that call. */
int mon_scene_pose_loss_batch(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s,
                              size_t n_poses, const mon_pose_refine_params* p, uint32_t iteration, float* losses /* n_poses */);
/* mon_pose_hypotheses (host only).  n candidate poses around Twc16, 16 floats each, column-major.  Hypothesis 0 is Twc16 bit for bit.  Hypothesis h >= 1:
 * u_k = the counter RNG's stream 6 keyed (seed, step = h, idx = k), k = 0..5; rho_i = max_trans (2 u_i - 1), i = 0..2; phi = max_rot_rad cbrt(u_3) e with e
 * the unit vector of z = 2 u_4 - 1 and azimuth 2 pi u_5 (uniform in the ball of radius max_rot_rad); D = [R(phi), c - R(phi) c + rho] with R by Rodrigues
 * and c = pivot_cam3, a point in the camera frame (NULL: the camera centre); Twc_h = Twc D.  A pure rotation leaves the pivot where it was, so objects
 * around the pivot stay in view.  Computed in double, rounded once to float.  MON_ERR_ARG for a NULL Twc16 or Twc16s_out, n = 0 or above 4096, and a
 * negative or non-finite max_rot_rad or max_trans. */
int mon_pose_hypotheses(const float* Twc16, const float* pivot_cam3 /* NULL: the camera centre */, float max_rot_rad, float max_trans, size_t n,
                        uint64_t seed, float* Twc16s_out /* 16 n */);
/* mon_scene_relocalise.  Candidate 0 is the caller's own guess.  The rule, every step a public call:
 *   1. ps = *p with rays_per_iter = r->score_rays.
 *   2. S = mon_scene_pose_loss_batch(candidates, ps, r->score_iteration); S goes to `scores` (n_candidates floats, may be NULL).
 *   3. The kept set: candidate 0, then the other candidates by ascending S (ties to the lower index, a non-finite S last), min(keep, n_candidates) in all.
 *   4. Each kept candidate is refined by what mon_scene_refine_camera(objs, .., p, c, pose, NULL) does from it, one after the other; bit for bit that call's.
 *   5. F = mon_scene_pose_loss_batch([refined_0 .. refined_{k-1}, start_0 .. start_{k-1}], ps, r->score_iteration).
 *   6. The entry of the lowest finite F wins (ties to the earlier entry); its pose goes to Twc16_out.  No finite F: candidate 0 as given, refined = 0, MON_OK.
 * So score_final <= F of candidate 0 as given and <= F of candidate 0 after plain mon_scene_refine_camera: by the common score the call is never worse than
 * local refinement from the caller's guess.  2 + min(keep, n_candidates) synchronisations (one per scoring round and per refinement).  Read-only as
 * mon_scene_refine_camera.  MON_ERR_ARG, before any device work, for NULL objs, obs, candidates, p, r or Twc16_out, n_candidates outside 1..4096,
 * score_rays outside 1..16384, keep outside 1..16, a bad schedule c and everything mon_scene_refine_camera rejects; MON_ERR_STATE as that call. */
typedef struct mon_reloc_params {
    uint32_t score_rays;       /* pixels drawn per hypothesis when scoring; 1..16384 */
    uint32_t keep;             /* hypotheses refined, 1..16; candidate 0 is always one of them */
    uint32_t score_iteration;  /* the iteration key of both scoring rounds */
} mon_reloc_params;
typedef struct mon_reloc_result {
    uint32_t best_candidate;   /* index into the candidates of the pose returned */
    uint32_t refined;          /* 1: its refined pose won, 0: the candidate as given */
    float    score_candidate0, score_best_candidate, score_final;   /* S[0], S[best_candidate], F of the pose returned */
} mon_reloc_result;
int mon_reloc_default(mon_reloc_params* r);     /* 256, 4, 0 */
int mon_scene_relocalise(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16_candidates,
                         size_t n_candidates, const mon_pose_refine_params* p, const mon_pose_c2f_params* c /* NULL: plain */, const mon_reloc_params* r,
                         float* Twc16_out, mon_reloc_result* result /* may be NULL */, float* scores /* n_candidates, may be NULL */);
/* ---- joint refinement of a window of camera poses and object poses (the reference has no such call; opt-in, new): the step a SLAM back
 * end takes between tracking and mapping -- a local window of keyframes and the objects they see, refined together.
 * Window.  obs may name several FrameIds; the boxes of one frame must be contiguous in obs.  The frames of the window are the distinct FrameIds in order of
 * first appearance ("window order"), F of them, 1 <= F <= 32; mon_window_frames (host only) returns that order.  Poses: Twc16s, F matrices in window order.
 * Objects: Tow16s, K matrices in objs order; NULL = each object's own Tow.
 * Objective.  For frame f, L_f and grad6_f are exactly what mon_scene_pose_loss(objs, .., the boxes of f, Twc_f, p, iteration, level_weights) defines: the
 * same pixel draw over the union of f's boxes keyed (seed, iteration, ray) with rays_per_iter counting per frame, the same per-object samples, merged
 * composite, both cuts and held quantities -- with Tow_j taken from Tow16s.  L = sum_f L_f, added in window order in fp32: a sum, not a mean, so each
 * camera's gradient is its single-frame gradient unscaled.
 * Gradients.  cam_grad6[6 f ..] = grad6_f.  obj_grad6[6 j ..] = sum_f G_{f,j}, added in window order, G_{f,j} = (sum g_o, sum x_o x g_o) / N_f in object
 * j's frame over the N_f rays of frame f: obj_grad6_j = dL/dxi at xi = 0 for Tow_j(xi) = exp(xi^) Tow_j, translation first (mon_object_pose_loss's
 * perturbation).  Held at their values at xi = 0 as there: every t and dt, the box intersections, the merge order, both cuts and the hash-grid corners.
 * Level weights act on both gradients exactly as in mon_scene_pose_loss (1: the unweighted bits; 0: both gradients exactly 0; the loss does not depend on
 * them).
 * Bit rule.  For every frame f, frame_loss[f] and cam_grad6[6 f ..] are bit for bit what mon_scene_pose_loss returns for that frame alone with the same
 * object poses -- whatever else the window holds, wherever the frame stands in it and however the frames are packed into passes.  No atomics anywhere:
 * equal arguments give equal bits.
 * Refinement (mon_scene_refine_window).  Adam (0.9, 0.999, 1e-8) on one twist per free camera and per object, moments per block.  Cameras: p->lr_trans /
 * p->lr_rot and Twc_f <- Twc_f exp(delta^), mon_scene_refine_camera's step.  Objects: w->lr_obj_trans / w->lr_obj_rot and Tow_j <- exp(delta^) Tow_j,
 * mon_object_refine_pose's step; Gram-Schmidt on both.  All gradients of a step are taken at the poses the step starts from, then everything moves at once.
 * Step i evaluates with iteration = i; with a schedule c it uses mon_pose_c2f_weights(c, Lmax, iters, i).  loss_trace[i] (iters + 1 values, may be NULL) is L
 * before step i, loss_trace[iters] L at the end; frame_trace[(iters + 1) * F] (may be NULL) holds the L_f, evaluation-major.  All poses live on the device
 * between steps; the whole call is enqueued at once -- passes of whole frames, at most 16384 rays each, filled greedily in window order, in the list
 * workspace of one mon_scene_pose_loss evaluation: passes x (2K + 2) + 1 launches per step -- with one synchronisation.
 * The first n_fixed_frames frames in window order keep their pose (anchors) and come back bit for bit as given.  refine_objects = 0: the objects keep Tow16s
 * and Tow16s_inout (which may then be NULL: each object's own Tow) comes back bit for bit as given.  refine_objects != 0 with n_fixed_frames = 0 is rejected:
 * the objective is invariant under one common motion of every camera and object, so nothing would hold the map in place.
 * Read-only, as mon_scene_refine_camera: nothing about any object, the dataset or a manager changes; the poses go back to the caller only, who stores them
 * with mon_online_update_dataset (cameras) and mon_object_set_pose / mon_online_set_object_pose (objects).  side 0 / 1 as in that call.
 * Returns MON_ERR_ARG, before any device work, for everything mon_scene_pose_loss / mon_scene_refine_camera reject per frame, non-contiguous frames, more
 * than 32 frames, more than 16384 rays in one frame (a frame is never split across passes), n_fixed_frames above F, non-finite or negative object step
 * sizes, refine_objects without a fixed frame or with a NULL Tow16s_inout, a non-finite Tow16s, a NULL Twc16s or w; MON_ERR_STATE as
 * mon_scene_refine_camera. */
typedef struct mon_window_params {
    uint32_t n_fixed_frames;  /* the first n frames in window order keep their pose (anchors); 0..F */
    int32_t  refine_objects;  /* 0: the objects keep Tow16s */
    float    lr_obj_trans, lr_obj_rot;   /* Adam step sizes of the object twists (object-frame units, radians) */
} mon_window_params;
int mon_window_default(mon_window_params* w);   /* 1, 1, 2e-3, 4e-3 (mon_pose_refine_default's steps) */
/* host only: the distinct FrameIds of obs in order of first appearance; MON_ERR_ARG for non-contiguous frames, more than 32 frames and NULL arguments */
int mon_window_frames(const mon_frame_bbox* obs, size_t n_obs, uint32_t* frame_ids_out /* cap 32 */, size_t* n_frames_out);
/* One evaluation.  Every output may be NULL: loss, frame_loss [F], cam_grad6 [6 F], obj_grad6 [6 K]. */
int mon_scene_window_loss(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16s /* 16 F */,
                          const float* Tow16s /* 16 K, or NULL */, const mon_pose_refine_params* p, uint32_t iteration,
                          const float* level_weights /* NULL or Lmax */, float* loss, float* frame_loss, float* cam_grad6, float* obj_grad6);
int mon_scene_refine_window(mon_object* const* objs, size_t n_objs, int side, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p,
                            const mon_pose_c2f_params* c /* NULL: plain */, const mon_window_params* w, float* Twc16s_inout /* 16 F */,
                            float* Tow16s_inout /* 16 K; NULL allowed only when refine_objects == 0 */, float* loss_trace /* iters + 1, may be NULL */,
                            float* frame_trace /* (iters + 1) F, may be NULL */);
/* Stores a new Tow (column-major, world -> object) in a trained object: replaces the object's pose and nothing else -- weights, optimizer state, counters,
 * the occupancy grid and the render-skip grids live in the object frame and stay.  What was built under the old pose is marked stale: the candidate rays
 * prepared for the coming iteration are generated again and a captured training graph is dropped; setting the pose the object already has therefore leaves
 * training bit for bit as it was.  An object holds one Tow for both sides.  The pose is replaced under the device's inference lock, which every side 1
 * call holds from start to end: a side 1 call running on another thread (a viewer's mon_online_render_scene, mon_online_refine_camera, ...) sees either
 * the old pose or the new one, never a mixture, and needs no care by the caller.  The price is latency, not correctness: this call waits until a side 1
 * call in flight on the device has ended (a 100-step mon_online_refine_window or a relocalisation may take tens of milliseconds), and
 * mon_online_set_object_pose holds the object's model lock while it waits, so that object's training slice stalls for as long (lock order everywhere: model
 * lock, then inference lock).  A back end that minds calls the setter between its own side 1 calls.
 * Between this call and the object's next publication a side 1 call uses
 * the NEW pose with the snapshot's weights as published -- consistent, since the weights are in the object frame; the next publication changes weights
 * only.  Against training the caller serialises, as for mon_object_render (mon_online_set_object_pose does it with the model lock).  mon_object_save
 * afterwards stores the new Tow.  MON_ERR_ARG for NULL arguments or a non-finite matrix; MON_ERR_STATE between stage-wise calls of
 * mon_object_train_stages. */
int mon_object_set_pose(mon_object* obj, const float* Tow16);
/* NeRF_Model::GetDensityOnGrid (nerf_model.cu:2007-2048): raw density channel on an rx*ry*rz lattice. */
int mon_object_density_grid(mon_object* obj, int rx, int ry, int rz, float* out_host);

/* ---- mesh extraction: NeRF_Model::GenerateMesh + TransCPUMesh (CORE/src/nerf_model.cu:1993-2095), MarchingCubes and
 * compute_mesh_1ring (CORE/src/marching_cubes.cu:478-509, 655-665), SaveMesh (nerf_model.cu:2181-2184 -> save_mesh :511-653).
 * res <= 0 selects the reference's 64 (marching_cubes.h:30); the reference's threshold is 2.0 on the PRE-activation density
 * (marching_cubes.h:31).  n_verts is rounded up to a multiple of 128 with all-zero padding vertices (marching_cubes.cu:496);
 * vertex / face numbering is deterministic here (lattice order), the reference's is atomicAdd order.
 * The result is kept with the object as CPUMeshData (CORE/include/common.h:32-41): verts / normals float[3n], colors u8[3n],
 * indices u32; get_mesh with try_lock_only != 0 behaves like DrawCPUMesh's try_lock (nerf.cu:486-490). */
int mon_object_generate_mesh(mon_object* obj, int res, float thresh, uint32_t* n_verts, uint32_t* n_indices);
int mon_object_mesh_counts(mon_object* obj, uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices);
int mon_object_get_mesh(mon_object* obj, float* verts, float* normals, uint8_t* colors, uint32_t* indices, int try_lock_only);
/* Counts + data under one hold of the mesh mutex, bounded by the caller's capacities (in vertices / indices): the form a viewer thread uses
 * while the object's thread trains and republishes the mesh (counts-then-get is only safe once the threads have ended).  MON_ERR_ARG with
 * the needed counts in n_* when a buffer is too small; MON_ERR_STATE when try_lock_only and the trainer holds the mesh, or no mesh yet. */
int mon_object_copy_mesh(mon_object* obj, uint32_t cap_verts, uint32_t cap_indices, float* verts, float* normals, uint8_t* colors, uint32_t* indices,
                         uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices, int try_lock_only);
/* lock-free: number of meshes published so far (0 = none); a viewer copies again only when it changed */
int mon_object_mesh_generation(mon_object* obj, uint64_t* generation);
int mon_object_get_mesh_raw(mon_object* obj, float* normals_raw, float* colors_f32);      /* un-normalised normals, float colours (parity tests) */
int mon_object_save_mesh(mon_object* obj, const char* path);                              /* ".ply" -> ASCII ply, anything else -> obj */
/* Marching cubes + normals on a caller-supplied lattice (x fastest); buffers may be NULL to query the counts. */
int mon_marching_cubes(int device, const float* density, int rx, int ry, int rz, float thresh, const float* aabb_min3, const float* aabb_max3,
                       float* verts, float* normals_raw, uint32_t* indices, uint32_t cap_verts, uint32_t cap_indices,
                       uint32_t* n_verts, uint32_t* n_verts_real, uint32_t* n_indices);

/* the configuration the object was created with (borrowed objects of the managers: base.json as read) */
int mon_object_get_config(mon_object* obj, mon_config* cfg);
int mon_object_info_get(mon_object* obj, mon_object_info* info);
/* Parameter I/O (the reference has none; needed for fixtures/checkpoints).
 * which: 0 fp32 master, 1 fp16 working copy, 2 fp16 EMA (inference) copy. */
int mon_object_get_params(mon_object* obj, int which, void* dst, size_t bytes);
int mon_object_set_params(mon_object* obj, const float* master, size_t n);
/* ---- Checkpoints (the reference has no save / load; opt-in, new): one object per file, little-endian, versioned, independent of how
 * the build lays the optimizer state out in device memory.  A saved object, loaded in another process onto any device, is the original bit for bit --
 * parameters, Adam moments and step counters, EMA (a pending lazy EMA stays pending), learning rate, counters, the training occupancy grid and its refresh
 * schedule, optionally the box list -- and training it further gives bit for bit what the uninterrupted object would have had.  Not stored: dataset frames
 * and poses, meshes, render-skip switch and grids, profiles, process-wide options (mon_set_option: set them as they were before loading).
 * Status codes of the three calls: MON_ERR_ARG a NULL argument, unknown flag bits; MON_ERR_IO unreadable, truncated, bad magic, newer version, any CRC
 * mismatch, sizes inconsistent with the config, invalid config; MON_ERR_STATE as listed per call. */
typedef struct mon_checkpoint_info {
    uint32_t version; mon_config cfg; int32_t class_id; float Tow[16], aabb_min[3], aabb_max[3];
    uint32_t n_params, n_mlp_params, n_grid_params, train_step, iter, n_boxes; int32_t backend;
    uint32_t has_occupancy, lazy_ema; uint64_t file_bytes;
} mon_checkpoint_info;
/* host only, no device: header, object block and section table checked (CRC, sizes against the file length, the config through mon_object_create's checks,
 * n_params recomputed).  verify != 0 also checks every section's CRC. */
int mon_checkpoint_read_info(const char* path, int verify, mon_checkpoint_info* out);
/* Writes <path>.tmp and renames it: a crash never leaves a truncated file under the final name.  Read-only: nothing about the object changes (parameters,
 * a pending lazy EMA, render-skip caches, snapshots, counters, the weights stamp).  Runs on the train stream; the caller serialises against training, as for
 * mon_object_render.  Streams through one pinned and one device staging buffer of at most 32 MB each.  MON_ERR_STATE: an object in the XORWOW "same inputs"
 * mode (its generator state is not stored), and between the stage-wise calls of mon_object_train_stages.  A grid pinned through
 * mon_debug_set_train_occupancy is saved as a grid; the pin is not. */
int mon_object_save(mon_object* obj, const char* path);
/* Everything mon_checkpoint_read_info(verify = 0) checks, the step-counter width and the box list (its CRC, and with MON_LOAD_BOXES every box against ds)
 * are judged before any device work; the object is then created on ds's device whichever device saved it and its state streamed in, each section's CRC
 * checked as it streams (a mismatch frees the half-built object: MON_ERR_IO).  Its derived images are rebuilt as mon_object_set_params does, the backend
 * restored and a snapshot published (from the EMA once a step has been taken).  *out = NULL on any failure.  flags: MON_LOAD_BOXES restores the box list (MON_ERR_STATE when ds lacks one of its frames or a box does not fit ds's images); without it
 * the object has no boxes -- it renders, meshes and refines, and trains once boxes are added.  use_depth follows mon_object_create's rule
 * (cfg.use_depth && the dataset's).  MON_ERR_STATE also for a file whose step-counter width (16 / 32 bits) is not this build's for that config. */
#define MON_LOAD_BOXES 1u
int mon_object_load(mon_dataset* ds, const char* path, uint32_t flags, mon_object** out);
/* Test hooks: split one iteration so intermediate buffers can be compared with the oracle.
 * stage bits: 1 GenerateBatch, 2 forward+backward, 4 optimizer_step(+step counter). */
int mon_object_train_stages(mon_object* obj, int stage_bits);
/* Backend selector for forward/backward: 0 = unfused reference kernels, 1 = fused MFMA kernel. */
int mon_object_set_backend(mon_object* obj, int backend);
int mon_object_set_profiling(mon_object* obj, int enable);
int mon_object_get_profile(mon_object* obj, mon_profile* out, int reset);
int mon_object_destroy(mon_object* obj);

/* ---- nerf::NerfManagerOffline (CORE/include/nerf_manager.h:21-50, CORE/src/nerf_manager.cu:9-131) without OpenCV/Eigen:
 * reads the reference's on-disk sequence layout (nerf_data.cu:27-121: config.yaml, img.txt, groundtruth.txt, rgb|depth|instance
 * PNGs) and object files (nerf.cu:58-118), one dataset replica per device, one thread per object, object k on device k mod nGPU,
 * 10 x 500 training iterations per object (nerf_manager.cu:89, nerf_model.cu:1635; MON_OFFLINE_OUTER / MON_OFFLINE_INNER override). */
typedef struct mon_offline mon_offline;
int mon_offline_create(const char* dataset_path, const char* network_config_file, int use_dense_depth, mon_offline** out);
int mon_offline_init(mon_offline* mgr);                                   /* Init()            */
/* The offline training schedule, process-wide, read by mon_offline_init: `outer` Train_Step calls of `inner` iterations per object (the reference hard-codes
 * 10 x 500: nerf_manager.cu:89, nerf_model.cu:1635; a mesh every 2nd outer step).  Both >= 1. */
int mon_offline_set_schedule(int outer, int inner);
int mon_offline_read_dataset(mon_offline* mgr);                           /* ReadDataset()     */
int mon_offline_create_nerf(mon_offline* mgr, const char* object_file);   /* CreateNeRF(file): starts the object's training thread */
int mon_offline_wait_threads_end(mon_offline* mgr);                       /* WaitThreadsEnd()  */
int mon_offline_n_objects(mon_offline* mgr, int* n);
int mon_offline_object_loss(mon_offline* mgr, int idx, float* loss, int* device);
/* test images for the first max_views (0 = all) training boxes of object idx: <out_dir>/<id>/test_{img,depth,mask}/<stamp>.png (nerf.cu:335-349) */
int mon_offline_render_test(mon_offline* mgr, int idx, const char* out_dir, int max_views);
/* the "Save Object Mesh" step of RenderTestImg alone (nerf.cu:397-403): <out_dir>/<id>/obj.ply if the object has a mesh; mon_offline_render_test includes it */
int mon_offline_save_mesh(mon_offline* mgr, int idx, const char* out_dir);
/* GetIntrinsics(), GetAllTwc() and, per object, GetObjTow() / GetBoundingBox() / GetFrameIdAndBBox() (MON/main.cpp:55,149-151,334-336: the viewer's inputs).
 * Buffers may be NULL to query the counts. */
int mon_offline_get_intrinsics(mon_offline* mgr, float* fx, float* fy, float* cx, float* cy, int* H, int* W);
int mon_offline_get_poses(mon_offline* mgr, float* Twc16s, size_t capacity_frames, size_t* n_frames);
int mon_offline_object_meta(mon_offline* mgr, int idx, int* class_id, float* Tow16, float* aabb_min3, float* aabb_max3, mon_frame_bbox* boxes,
        size_t capacity_boxes, size_t* n_boxes);
/* the timestamp string of the object's box_index-th observation (the test images' file names) */
int mon_offline_object_stamp(mon_offline* mgr, int idx, size_t box_index, char* buf, size_t capacity);
/* where the training thread saves <id>.ply (default "./output", nerf.cu:148; "" = do not save) */
int mon_offline_set_output_dir(mon_offline* mgr, const char* dir);
/* GetAllNeRF()[idx]: owned by the manager, do not destroy; only mon_object_copy_mesh(try_lock) is safe while its thread trains */
int mon_offline_object(mon_offline* mgr, int idx, mon_object** borrowed);
int mon_offline_destroy(mon_offline* mgr);
/* ---- nerf::NerfManagerOnline (CORE/include/nerf_manager.h:54-90, CORE/src/nerf_manager.cu:133-312) + the online half of nerf::NeRF
 * (nerf.cu:155-253, 406-448): per-object training thread sleeping on a condition variable, training gated on > 10 boxes,
 * per-object dataset mutex, finish protocol.  cv::Mat arguments become raw pointers (8-bit BGR(A), 8-bit instance, float depth). */
typedef struct mon_online mon_online;
int mon_online_create(const char* network_config_file, int use_sparse_depth, int train_step_iterations, mon_online** out);
int mon_online_init(mon_online* mgr);
int mon_online_dataset_init(mon_online* mgr, float fx, float fy, float cx, float cy, int H, int W, size_t imgs);
int mon_online_new_frame(mon_online* mgr, uint32_t img_id, const char* timestamp, const uint8_t* bgr, int channels, const uint8_t* instance,
                         const float* depth, const float* Twc16);                                   /* NewFrameToDataset */
/* CreateNeRF: 1.1x / 1.2x box inflation applied */
int mon_online_create_nerf(mon_online* mgr, int cls, const float* Tow16, const float* aabb_min3, const float* aabb_max3, size_t* idx_out);
int mon_online_update_nerf_bbox(mon_online* mgr, size_t idx, const mon_frame_bbox* boxes, size_t n, int train_step);                        /* UpdateNeRFBbox */
int mon_online_get_frame_idx(mon_online* mgr, const char* timestamp, int* idx);                     /* GetFrameIdx (-1 if unknown) */
/* NerfManagerOnline::UpdateDataset -> NeRF_Dataset::UpdateDataGPU (nerf_manager.cu:220-235, nerf_data.cu:341-353): the poses of frames
 * [cur_id - frame_num, cur_id) are replaced on every device (bundle adjustment moved them) while every object's training is excluded.
 * Twc16s: frame_num column-major 4x4.  The reference only calls it from commented-out code (LocalMapping.cc:1128-1150). */
int mon_online_update_dataset(mon_online* mgr, uint32_t cur_id, uint32_t frame_num, const float* Twc16s);
/* pose (Twc, column-major) the dataset holds for frame `frame_id` (NeRF::GetTwc reads these, nerf.cu:450-462) */
int mon_online_get_pose(mon_online* mgr, uint32_t frame_id, float* Twc16);
int mon_online_wait_threads_end(mon_online* mgr);                                                  /* WaitThreadsEnd: request finish + join */
int mon_online_object_info(mon_online* mgr, size_t idx, float* loss, int* train_calls, int* device, uint32_t* n_boxes);
/* one view of RenderNeRFsTest */
int mon_online_render(mon_online* mgr, size_t idx, mon_frame_bbox box, const float* Twc16, float* rgb, float* depth, float* mask);
/* mon_scene_render(side 1) of every object of the manager that has published weights (the others are left out; none: the background); instance = the
 * manager's object index.  A viewer's call: safe while the objects train.  MON_ERR_STATE when those objects span more than one device (a follow-up). */
int mon_online_render_scene(mon_online* mgr, mon_frame_bbox rect, const float* Twc16, float* rgb, float* depth, float* opacity, int32_t* instance);
/* mon_scene_probe(side 1) of every object of the manager that has published weights, chosen as mon_online_render_scene chooses them; both instance outputs
 * hold the manager's object indices.  A front end's call, safe while the objects train.  MON_ERR_STATE when no object has published yet or the objects
 * span more than one device. */
int mon_online_probe_scene(mon_online* mgr, const float* Twc16s, size_t n_poses, const mon_scene_query* q, size_t n_q,
                           float* rgb, float* depth, float* opacity, int32_t* instance, float* hit_depth, int32_t* hit_instance);
/* mon_scene_cast(side 1) of every object of the manager that has published weights, chosen as mon_online_render_scene chooses them; both instance outputs
 * hold the manager's object indices.  A planner's call, safe while the objects train.  MON_ERR_STATE when no object has published yet or the objects
 * span more than one device. */
int mon_online_cast_rays(mon_online* mgr, const mon_scene_ray* rays, size_t n_rays, float hit_opacity,
                         float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance);
/* mon_scene_query_points / mon_scene_query_lattice (side 1) of every object of the manager that has published weights, chosen as mon_online_render_scene
 * chooses them; owner holds the manager's object indices.  A planner's call, safe while the objects train.  MON_ERR_STATE when no object has published
 * yet or the objects span more than one device. */
int mon_online_query_points(mon_online* mgr, const float* world_xyz, size_t n,
                            float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside);
int mon_online_query_lattice(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz,
                             float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside);
/* mon_scene_distance_lattice (side 1) over the same objects, with the same refusals; nearest_owner holds the manager's object indices.  A planner's
 * call for the clearance field, safe while the objects train. */
int mon_online_distance_lattice(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist,
                                float* dist, int32_t* nearest, int32_t* nearest_owner, float* free_dist, float* sigma);
/* mon_scene_components_lattice (side 1) over the same objects, with the same refusals; owner holds the manager's object indices.  A planner's call for
 * reachability at a clearance and a mapper's for the blobs of the published map, safe while the objects train. */
int mon_online_components_lattice(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz,
                                  float sigma_min, int region, float clearance, int connectivity,
                                  int32_t* label, int32_t* comp, mon_lattice_component* table, uint32_t cap, uint32_t* n_components,
                                  float* dist, float* sigma, int32_t* owner);
/* mon_scene_paths_lattice (side 1) over the same objects, with the same refusals; owner holds the manager's object indices.  A planner's call for the cost
 * to its goal (seeds = the goal's cell) and the way there (mon_lattice_path from the robot's cell), safe while the objects train. */
int mon_online_paths_lattice(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz,
                             float sigma_min, float clearance, float soft_radius, float soft_weight, int connectivity,
                             const int32_t* seeds, size_t n_seeds, float max_cost,
                             float* cost, int32_t* next, float* dist, float* sigma, int32_t* owner);
/* mon_scene_dist_field (side 1) over the same objects, with the same refusals: the published map's clearance as a snapshot on the device, which a sampling
 * planner scores its trajectories against (mon_dist_field_score) until the next publication.  The handle is the caller's: it does not follow the manager's
 * training and stays valid after mon_online_destroy; mon_dist_field_destroy frees it. */
int mon_online_dist_field(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, float max_dist,
                          mon_dist_field** field);
/* mon_scene_signed_distance_lattice and mon_scene_signed_dist_field (side 1) over the same objects, with the same refusals; nearest_owner holds the
 * manager's object indices.  The published map's signed field for a scan matcher or a ray tracer, safe while the objects train; the handle is the caller's,
 * as mon_online_dist_field's. */
int mon_online_signed_distance_lattice(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, uint32_t flags,
                                       float max_dist, float* sdist, int32_t* nearest_edge, int32_t* nearest_owner, float* sigma, float* val,
                                       float* iso_out);
int mon_online_signed_dist_field(mon_online* mgr, const float* origin3, const float* step3, int nx, int ny, int nz, float sigma_min, uint32_t flags,
                                 float max_dist, mon_dist_field** field);
/* mon_scene_query_gradients / mon_scene_cast_normals (side 1) over the same objects, with the same refusals.  owner, instance and hit_instance hold the
 * manager's object indices, and so does select: -1, or the index of an object with published weights; any other value is MON_ERR_ARG.
 * mon_online_cast_normals picks the objects once for both steps of its rule.  There is no online lattice form of the gradients: a caller forms the lattice
 * with mon_lattice_points and passes it as a list. */
int mon_online_query_gradients(mon_online* mgr, const float* world_xyz, size_t n, const float* level_weights, const int32_t* select,
                               float* sigma, float* rgb, int32_t* owner, float* owner_sigma, uint32_t* n_inside,
                               float* grad_log, float* grad_sigma, float* normal);
int mon_online_cast_normals(mon_online* mgr, const mon_scene_ray* rays, size_t n_rays, float hit_opacity, const float* level_weights,
                            float* rgb, float* dist, float* opacity, int32_t* instance, float* hit_t, float* hit_sample_t, int32_t* hit_instance,
                            float* hit_xyz, float* normal, float* grad_log);
/* mon_object_refine_pose(side 1) of object idx: its published snapshot, on the inference stream -- safe while the manager trains it.  MON_ERR_STATE while
 * nothing of it has been published. */
int mon_online_refine_pose(mon_online* mgr, size_t idx, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p, float* Tow16_inout,
                           float* loss_trace);
/* mon_object_refine_pose_c2f(side 1) of object idx, as mon_online_refine_pose */
int mon_online_refine_pose_c2f(mon_online* mgr, size_t idx, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p,
                               const mon_pose_c2f_params* c, float* Tow16_inout, float* loss_trace);
/* mon_scene_refine_camera(side 1) over every object of the manager that has published weights: a frontend's call for a new frame (mon_online_new_frame ->
 * mon_online_refine_camera -> mon_online_update_dataset), safe while the objects train.  MON_ERR_STATE when no object has published yet or when those
 * objects span more than one device (as mon_online_render_scene). */
int mon_online_refine_camera(mon_online* mgr, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p, const mon_pose_c2f_params* c,
                             float* Twc16_inout, float* loss_trace);
/* mon_scene_relocalise(side 1) over every object of the manager that has published weights: a resumed session's call for a frame whose pose is only
 * roughly known (mon_online_load_map -> mon_online_new_frame -> mon_pose_hypotheses -> mon_online_relocalise -> mon_online_update_dataset), safe while the
 * objects train.  Nothing of the manager changes.  MON_ERR_STATE as mon_online_refine_camera. */
int mon_online_relocalise(mon_online* mgr, const mon_frame_bbox* obs, size_t n_obs, const float* Twc16_candidates, size_t n_candidates,
                          const mon_pose_refine_params* p, const mon_pose_c2f_params* c, const mon_reloc_params* r, float* Twc16_out,
                          mon_reloc_result* result, float* scores);
/* mon_scene_refine_window(side 1) over every object of the manager that has published weights, chosen as mon_online_refine_camera chooses them: a back
 * end's call for a local window of keyframes already in the dataset (mon_online_refine_window -> accept by the trace -> mon_online_update_dataset for the
 * cameras, mon_online_set_object_pose for the objects), safe while the objects train.  Tow16s_inout holds 16 floats per MANAGER object (n_objects of them, may
 * be NULL when refine_objects == 0): the starting pose of every object that takes part is read from it and its refined pose written back; the others keep
 * what the array held.  included[n_objects] (may be NULL) marks the objects that took part.  Nothing of the manager changes.  MON_ERR_ARG when n_objects is
 * not the manager's object count; MON_ERR_STATE as mon_online_refine_camera. */
int mon_online_refine_window(mon_online* mgr, const mon_frame_bbox* obs, size_t n_obs, const mon_pose_refine_params* p, const mon_pose_c2f_params* c,
                             const mon_window_params* w, float* Twc16s_inout, float* Tow16s_inout, size_t n_objects, uint8_t* included, float* loss_trace,
                             float* frame_trace);
/* mon_object_set_pose of object idx under its model lock (as mon_online_update_dataset takes it): safe while the object trains; the manager's own record of
 * the pose follows.  The snapshot side sees the new pose from the call on (one Tow per object, replaced under the device's inference lock: see
 * mon_object_set_pose), so side 1 calls of other threads need not be held back. */
int mon_online_set_object_pose(mon_online* mgr, size_t idx, const float* Tow16);
/* The object map as checkpoints: <dir>/map.txt, one line "index file class_id" per object, and one mon_object_save file per object next to it.  Each
 * object's model lock is taken in turn (as mon_online_update_dataset does), so the call is safe while the objects train and every file is one consistent
 * object; the map is NOT one global cut -- object 3 may be saved some training slices later than object 0. */
/* dir is created if missing (its parent must exist: MON_ERR_IO otherwise).  When an object's save fails, the files this call wrote are removed and an
 * earlier map.txt is left as it was.  mon_online_load_map reads map.txt in line order: the index column must count up from line to line and class_id must be
 * the file's own (MON_ERR_IO otherwise); the objects get the manager's next free indices. */
int mon_online_save_map(mon_online* mgr, const char* dir);
/* Valid after mon_online_dataset_init: appends the map's objects, each with its training thread, as mon_online_create_nerf does -- object k of the call on
 * device k mod nGPU continuing the manager's rotation, no box inflation (the file holds the box in use).  flags as mon_object_load: with MON_LOAD_BOXES the
 * boxes count as uploaded, so the "> 10 boxes" gate of training behaves as before the save (the frames they name must have been handed over with
 * mon_online_new_frame first).  *n_loaded (may be NULL) = objects appended; on an error the objects loaded before it stay. */
int mon_online_load_map(mon_online* mgr, const char* dir, uint32_t flags, size_t* n_loaded);
/* RenderNeRFsTest(out_path, idx, stamps, boxes, Twcs, radius) -> NeRF::RenderTestImg (nerf.cu:255-404): test images + test.txt +
 * train.txt + the 60-view 360-degree video (RenderVideo, nerf_model.cu:1832-1990) + obj.ply under <out_path>/<id>/ */
int mon_online_render_nerfs_test(mon_online* mgr, const char* out_path, size_t idx, const char* const* timestamps, const mon_frame_bbox* boxes,
                                 const float* Twcs16, size_t n, float radius);
int mon_generate_toc(float theta_deg, float phi_deg, float radius, float* Toc16);   /* NeRF_Model::GenerateToc, nerf_model.cu:2186-2205 */
/* DrawMesh(idx) reads this object's CPUMeshData through mon_object_copy_mesh(try_lock) */
int mon_online_object(mon_online* mgr, size_t idx, mon_object** borrowed);
int mon_online_destroy(mon_online* mgr);

/* PNG codec used for the sequence layout (8/16-bit, gray/RGB/RGBA in; gray/RGB out; 16-bit samples big-endian as in the file).
 * pixels may be NULL to query the header only. */
int mon_png_read(const char* path, int* width, int* height, int* channels, int* bit_depth, uint8_t* pixels, size_t capacity);
int mon_png_write(const char* path, int width, int height, int channels, int bit_depth, const uint8_t* pixels_big_endian);
/* A rendered crop as the reference stores it (nerf.cu:335-349: img.convertTo(CV_8UC3, 255), depth.convertTo(CV_16UC1, 20000), mask.convertTo(CV_8UC1, 255);
 * saturating, round half to even); mask / mask_path may be NULL (RenderVideo writes none). */
int mon_write_render_pngs(const char* img_path, const char* depth_path, const char* mask_path, uint32_t w, uint32_t h, const float* rgb, const float* depth,
        const float* mask);

/* Process-wide test and tuning switches (none is needed for normal operation; defaults are the product behaviour).  Read when an object is
 * created or a training call is enqueued -- set them before.  Nine names (round 6; the A/B switches whose losing setting only a measurement wanted --
 * record / array optimizer state, 16- / 32-bit step counters, chunk flags, lane chunk, slice length -- are variant builds now, model.h):
 *   "backend"            -1 auto, 0 layer-at-a-time kernels, 1 fused
 *   "use_graph"          1: replay an iteration pair as a hipGraph
 *   "big_switch"         gradient-carrying samples below which the large-table levels scatter with global atomics (0 = always atomics, 1 = always binned)
 *   "lds_encode"         forward hash-grid encode from LDS-resident level tiles (kernels_encode.hip): 1 = from 3072 rays per batch (default), 2 = always,
 *                        0 = never (gathers inside k_fused_train) -- bit-identical parameters either way
 *   "tile_render"        inference on feature-planar level tiles: 0 never, 1 crops of 4096 rays and more + point queries, 2 always -- bit-identical images
 *   "step_variant"       1: NeRF_Model::Step's sample-compaction schedule (nerf_model.cu:1504-1550) on the layer-at-a-time kernels -- the reference's own
 *                        "unavailable, for reference only" path, kept checkable; 0 = Step_No_Compacted, what both drivers train with
 *   "keep_zero_samples"  1: zero-gradient samples are scattered too -- the exactness test's A/B
 *   "train_lanes"        per-device training lanes (0 = every object on its own stream)
 *   "roctx"              1: roctx ranges per phase
 * Unknown names return MON_ERR_ARG. */
int mon_set_option(const char* name, long value);
int mon_get_option(const char* name, long* value);

/* Whole-device helpers used by bench.py. */
int mon_device_synchronize(int device);
/* hipMemGetInfo: sizing how many object NeRFs a device takes (measured: base.json 198 MB each incl. workspaces, T = 2^22 2.5 GB; + ~190 MB once per device
 * for the render workspace) */
int mon_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes);
/* Staged-execution companion (tests): the fused backend also writes its intermediate activations into the debug buffers (slower);
 * they are read back through libmon_core_diag.so (include/mon_core_diag.h).  enable = 1: on the gather chain (every level's grid gradient through
 * global atomics, readable as one table); 2: on the chain the object would run anyway (level tiles -> k_fused_train<PRE> -> k_grid_scatter). */
int mon_object_set_debug_dump(mon_object* obj, int enable);

#ifdef __cplusplus
}
#endif
#endif /* MON_CORE_H */
