"""ctypes binding of libmon_core.so.  Mirrors the reference's manager/object interface
(CORE/include/nerf_manager.h, nerf.h) one call per C-ABI entry point; no compute happens in Python and
there is no CPU fallback: every compute call raises MonError when the HIP library or a device is missing."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


class MonError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mon_core error %d: %s" % (code, msg)); self.code = code


class MonConfig(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("n_features", C.c_int32), ("log2_hashmap_size", C.c_int32), ("base_resolution", C.c_int32),
                ("per_level_scale", C.c_float), ("n_neurons", C.c_int32), ("n_hidden_layers", C.c_int32), ("rays_per_batch", C.c_int32),
                ("n_samples", C.c_int32), ("loss_scale", C.c_float), ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("epsilon", C.c_float), ("l2_reg", C.c_float), ("ema_decay", C.c_float), ("decay_start", C.c_int32), ("decay_interval", C.c_int32),
                ("decay_base", C.c_float), ("param_seed", C.c_uint32), ("rng_flags", C.c_uint32), ("sample_seed", C.c_uint64),
                ("use_depth", C.c_int32), ("occupancy_skip", C.c_int32)]


class MonBBox(C.Structure):
    _fields_ = [("FrameId", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("h", C.c_uint32), ("w", C.c_uint32)]


class MonInfo(C.Structure):
    _fields_ = [("n_params", C.c_uint32), ("n_mlp_params", C.c_uint32), ("n_grid_params", C.c_uint32), ("encoded_width", C.c_uint32),
                ("train_step", C.c_uint32), ("n_boxes", C.c_uint32), ("last_n_valid", C.c_uint32), ("device", C.c_int32),
                ("last_loss", C.c_float), ("learning_rate", C.c_float), ("backend", C.c_int32), ("skipped_batches", C.c_uint32)]


class MonRenderSkipStats(C.Structure):
    _fields_ = [("active", C.c_uint32), ("live_cells", C.c_uint32), ("grid_builds", C.c_uint64), ("samples_in_box", C.c_uint64),
                ("samples_live", C.c_uint64)]


class PoseRefineParams(C.Structure):
    """mon_pose_refine_params (include/mon_core.h): Adam steps, rays per evaluation (0 = every box pixel), step sizes, loss weights, Huber width, seed."""
    _fields_ = [("iters", C.c_int32), ("rays_per_iter", C.c_uint32), ("lr_trans", C.c_float), ("lr_rot", C.c_float), ("w_rgb", C.c_float),
                ("w_mask", C.c_float), ("w_depth", C.c_float), ("depth_huber", C.c_float), ("seed", C.c_uint64)]


class PoseC2FParams(C.Structure):
    """mon_pose_c2f_params (include/mon_core.h): the coarse-to-fine window's alpha (in levels) at step 0, after the ramp, and the ramp's share of the steps."""
    _fields_ = [("level_start", C.c_float), ("level_end", C.c_float), ("ramp", C.c_float)]


class RelocParams(C.Structure):
    """mon_reloc_params (include/mon_core.h): pixels drawn per hypothesis when scoring, hypotheses refined, the iteration key of both scoring rounds."""
    _fields_ = [("score_rays", C.c_uint32), ("keep", C.c_uint32), ("score_iteration", C.c_uint32)]


class WindowParams(C.Structure):
    """mon_window_params (include/mon_core.h): the anchors of a window refinement, whether the objects move, and the objects' Adam step sizes."""
    _fields_ = [("n_fixed_frames", C.c_uint32), ("refine_objects", C.c_int32), ("lr_obj_trans", C.c_float), ("lr_obj_rot", C.c_float)]


class SceneQuery(C.Structure):
    """mon_scene_query (include/mon_core.h): one probe query -- the pose it looks through, its jitter key, the image point (u, v)."""
    _fields_ = [("pose", C.c_uint32), ("key", C.c_uint32), ("u", C.c_float), ("v", C.c_float)]


SCENE_QUERY_DTYPE = np.dtype([("pose", np.uint32), ("key", np.uint32), ("u", np.float32), ("v", np.float32)])


class SceneRay(C.Structure):
    """mon_scene_ray (include/mon_core.h): one world ray of a cast -- origin, segment length, unit direction, jitter key."""
    _fields_ = [("o", C.c_float * 3), ("t_max", C.c_float), ("d", C.c_float * 3), ("key", C.c_uint32)]


SCENE_RAY_DTYPE = np.dtype([("o", np.float32, 3), ("t_max", np.float32), ("d", np.float32, 3), ("key", np.uint32)])
# mon_lattice_component (include/mon_core.h): one record of a component table, 32 bytes
LATTICE_COMPONENT_DTYPE = np.dtype([("rep", np.int32), ("cells", np.uint32), ("lo", np.int32, 3), ("hi", np.int32, 3)])


class DistFieldDesc(C.Structure):
    """mon_dist_field_desc (include/mon_core.h): what mon_dist_field_info reports of a field handle."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("device", C.c_int32), ("origin", C.c_float * 3), ("step", C.c_float * 3),
                ("max_value", C.c_float)]


class TrajScoreParams(C.Structure):
    """mon_traj_score_params (include/mon_core.h): the value of a sample outside the field, the hit margin, the clearance below which a sample costs."""
    _fields_ = [("outside", C.c_float), ("margin", C.c_float), ("safe", C.c_float)]


class ScanMatchParams(C.Structure):
    """mon_scan_match_params (include/mon_core.h): the Huber threshold on |d| (+inf: plain least squares) and the value of a point outside the field."""
    _fields_ = [("huber", C.c_float), ("outside", C.c_float)]


class RegisterParams(C.Structure):
    """mon_register_params (include/mon_core.h): ScanMatchParams, then the Levenberg-Marquardt schedule of mon_dist_field_register."""
    _fields_ = [("huber", C.c_float), ("outside", C.c_float), ("max_evals", C.c_int32), ("lambda0", C.c_float), ("lambda_up", C.c_float),
                ("lambda_down", C.c_float), ("lambda_max", C.c_float), ("tol_trans", C.c_float), ("tol_rot", C.c_float), ("min_inside", C.c_int32)]


class TraceParams(C.Structure):
    """mon_trace_params (include/mon_core.h): the march of mon_dist_field_trace: its range, the hit level, the least step, the step's share of the sampled
    distance, the step before the lattice is entered, and the step budget."""
    _fields_ = [("t_min", C.c_float), ("t_max", C.c_float), ("eps", C.c_float), ("step_min", C.c_float), ("relax", C.c_float), ("step_outside", C.c_float),
                ("max_steps", C.c_int32)]


class BeamParams(C.Structure):
    """mon_beam_params (include/mon_core.h): the Huber threshold on |range - measured| (+inf: plain least squares)."""
    _fields_ = [("huber", C.c_float)]


class RelocResult(C.Structure):
    """mon_reloc_result (include/mon_core.h): which candidate won, whether its refined pose did, and the scores S[0], S[best], F[winner]."""
    _fields_ = [("best_candidate", C.c_uint32), ("refined", C.c_uint32), ("score_candidate0", C.c_float), ("score_best_candidate", C.c_float),
                ("score_final", C.c_float)]


class CheckpointInfo(C.Structure):
    """mon_checkpoint_info (include/mon_core.h): what mon_checkpoint_read_info reports of a checkpoint file, host only."""
    _fields_ = [("version", C.c_uint32), ("cfg", MonConfig), ("class_id", C.c_int32), ("Tow", C.c_float * 16), ("aabb_min", C.c_float * 3),
                ("aabb_max", C.c_float * 3), ("n_params", C.c_uint32), ("n_mlp_params", C.c_uint32), ("n_grid_params", C.c_uint32),
                ("train_step", C.c_uint32), ("iter", C.c_uint32), ("n_boxes", C.c_uint32), ("backend", C.c_int32), ("has_occupancy", C.c_uint32),
                ("lazy_ema", C.c_uint32), ("file_bytes", C.c_uint64)]


MON_LOAD_BOXES = 1


def checkpoint_info(path, verify=True):
    """mon_checkpoint_read_info: the header, object block and section table of a checkpoint, checked on the host (no device); verify also checks every
    section's CRC.  Raises MonError (code 4) for anything damaged."""
    i = CheckpointInfo(); _check(lib().mon_checkpoint_read_info(os.fsencode(path), int(bool(verify)), C.byref(i))); return i


def checkpoint_timing(enable=True):
    """(diagnostics library) HIP-event milliseconds of the pack / unpack kernels of this thread's saves and loads since the last call; enable starts / stops."""
    ms = C.c_double(0); _check(diag_lib().mon_debug_checkpoint_timing(int(bool(enable)), C.byref(ms))); return ms.value


class MonProfile(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_uint64 * 8)]


K_BATCH, K_FWDBWD, K_OPTIM, K_RENDER = 0, 1, 2, 3

# every symbol include/mon_core.h declares (checked by tests/test_abi.py against the header text)
_SIGS = {
    "mon_last_error": (C.c_char_p, []),
    "mon_version": (C.c_int, []),
    "mon_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mon_set_logical_devices": (C.c_int, [C.c_int]),
    "mon_offline_set_schedule": (C.c_int, [C.c_int, C.c_int]),
    "mon_set_option": (C.c_int, [C.c_char_p, C.c_long]),
    "mon_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_long)]),
    "mon_config_default": (C.c_int, [C.POINTER(MonConfig)]),
    "mon_config_from_json": (C.c_int, [C.c_char_p, C.POINTER(MonConfig)]),
    "mon_dataset_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "mon_dataset_add_frame": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_dataset_n_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "mon_dataset_destroy": (C.c_int, [C.c_void_p]),
    "mon_object_create": (C.c_int, [C.c_void_p, C.POINTER(MonConfig), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mon_object_add_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mon_object_train": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "mon_object_render": (C.c_int, [C.c_void_p, MonBBox, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mon_object_render_snapshot": (C.c_int, [C.c_void_p, MonBBox, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]),
    "mon_object_density_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mon_object_info_get": (C.c_int, [C.c_void_p, C.POINTER(MonInfo)]),
    "mon_object_get_params": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "mon_object_set_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "mon_object_train_stages": (C.c_int, [C.c_void_p, C.c_int]),
    "mon_object_set_backend": (C.c_int, [C.c_void_p, C.c_int]),
    "mon_object_set_debug_dump": (C.c_int, [C.c_void_p, C.c_int]),
    "mon_object_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "mon_object_get_profile": (C.c_int, [C.c_void_p, C.POINTER(MonProfile), C.c_int]),
    "mon_object_destroy": (C.c_int, [C.c_void_p]),
    "mon_offline_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mon_offline_init": (C.c_int, [C.c_void_p]),
    "mon_offline_read_dataset": (C.c_int, [C.c_void_p]),
    "mon_offline_create_nerf": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mon_offline_wait_threads_end": (C.c_int, [C.c_void_p]),
    "mon_offline_n_objects": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mon_offline_object_loss": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "mon_offline_render_test": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int]),
    "mon_offline_save_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p]),
    "mon_offline_destroy": (C.c_int, [C.c_void_p]),
    "mon_object_generate_mesh": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mon_object_mesh_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mon_object_get_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "mon_device_mem_info": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "mon_object_mesh_generation": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mon_object_get_config": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mon_object_copy_mesh": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_int]),
    "mon_object_get_mesh_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_object_save_mesh": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mon_marching_cubes": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_uint32, C.c_uint32,
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mon_offline_get_intrinsics": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_float)] * 4 + [C.POINTER(C.c_int)] * 2),
    "mon_offline_get_poses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "mon_offline_object_meta": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
            C.POINTER(C.c_size_t)]),
    "mon_offline_set_output_dir": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mon_offline_object": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mon_online_object": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "mon_online_render_nerfs_test": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "mon_generate_toc": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "mon_online_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mon_online_init": (C.c_int, [C.c_void_p]),
    "mon_online_dataset_init": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_size_t]),
    "mon_online_new_frame": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_create_nerf": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]),
    "mon_online_update_nerf_bbox": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]),
    "mon_online_get_frame_idx": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    "mon_online_update_dataset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mon_online_get_pose": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "mon_online_wait_threads_end": (C.c_int, [C.c_void_p]),
    "mon_online_object_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "mon_online_render": (C.c_int, [C.c_void_p, C.c_size_t, MonBBox, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_destroy": (C.c_int, [C.c_void_p]),
    "mon_png_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]),
    "mon_png_write": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mon_write_render_pngs": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_physical_device": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "mon_offline_object_stamp": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_char_p, C.c_size_t]),
    "mon_device_synchronize": (C.c_int, [C.c_int]),
    "mon_object_set_render_skip": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "mon_object_render_skip_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(MonRenderSkipStats)]),
    "mon_object_render_occupancy": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "mon_scene_render": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, MonBBox, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_render_scene": (C.c_int, [C.c_void_p, MonBBox, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_probe": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_probe_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p]),
    "mon_scene_cast": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_cast_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p]),
    "mon_camera_rays": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mon_object_query_points": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mon_scene_query_points": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_query_lattice": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_lattice_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mon_online_query_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_query_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p]),
    "mon_distance_transform": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "mon_scene_distance_lattice": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_distance_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_label_components": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "mon_scene_components_lattice": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
            C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_components_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_shortest_paths": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p,
            C.c_void_p]),
    "mon_scene_paths_lattice": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
            C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_paths_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
            C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_lattice_path": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mon_dist_field_create": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mon_scene_dist_field": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
            C.POINTER(C.c_void_p)]),
    "mon_online_dist_field": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_void_p)]),
    "mon_signed_distance_transform": (C.c_int, [C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "mon_scene_signed_distance_lattice": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32,
            C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_signed_dist_field": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32,
            C.c_float, C.POINTER(C.c_void_p)]),
    "mon_online_signed_distance_lattice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_float,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_signed_dist_field": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint32, C.c_float,
            C.POINTER(C.c_void_p)]),
    "mon_dist_field_info": (C.c_int, [C.c_void_p, C.POINTER(DistFieldDesc)]),
    "mon_dist_field_read": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mon_dist_field_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p]),
    "mon_dist_field_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
            C.POINTER(TrajScoreParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_dist_field_destroy": (C.c_int, [C.c_void_p]),
    "mon_dist_field_match": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(ScanMatchParams), C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p]),
    "mon_register_default": (C.c_int, [C.c_void_p, C.POINTER(RegisterParams)]),
    "mon_dist_field_register": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(RegisterParams), C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_trace_default": (C.c_int, [C.c_void_p, C.POINTER(TraceParams)]),
    "mon_dist_field_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(TraceParams), C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p]),
    "mon_dist_field_beam_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TraceParams),
            C.POINTER(BeamParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_object_query_gradients": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_query_gradients": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_query_lattice_gradients": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_cast_normals": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_query_gradients": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_cast_normals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_pose_refine_default": (C.c_int, [C.POINTER(PoseRefineParams)]),
    "mon_object_pose_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(PoseRefineParams), C.c_uint32,
            C.POINTER(C.c_float), C.c_void_p]),
    "mon_object_refine_pose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.c_void_p, C.c_void_p]),
    "mon_online_refine_pose": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.c_void_p, C.c_void_p]),
    "mon_pose_c2f_default": (C.c_int, [C.POINTER(PoseC2FParams)]),
    "mon_pose_c2f_weights": (C.c_int, [C.POINTER(PoseC2FParams), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mon_object_pose_loss_levels": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(PoseRefineParams), C.c_uint32,
            C.c_void_p, C.POINTER(C.c_float), C.c_void_p]),
    "mon_object_refine_pose_c2f": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams),
            C.c_void_p, C.c_void_p]),
    "mon_online_refine_pose_c2f": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams),
            C.c_void_p, C.c_void_p]),
    "mon_scene_pose_loss": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(PoseRefineParams), C.c_uint32,
            C.c_void_p, C.POINTER(C.c_float), C.c_void_p]),
    "mon_scene_refine_camera": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams),
            C.c_void_p, C.c_void_p]),
    "mon_online_refine_camera": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams), C.c_void_p,
            C.c_void_p]),
    "mon_scene_pose_loss_batch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams),
            C.c_uint32, C.c_void_p]),
    "mon_pose_hypotheses": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_size_t, C.c_uint64, C.c_void_p]),
    "mon_reloc_default": (C.c_int, [C.POINTER(RelocParams)]),
    "mon_scene_relocalise": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams),
            C.POINTER(PoseC2FParams), C.POINTER(RelocParams), C.c_void_p, C.POINTER(RelocResult), C.c_void_p]),
    "mon_online_relocalise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams),
            C.POINTER(RelocParams), C.c_void_p, C.POINTER(RelocResult), C.c_void_p]),
    "mon_window_default": (C.c_int, [C.POINTER(WindowParams)]),
    "mon_window_frames": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]),
    "mon_scene_window_loss": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(PoseRefineParams),
            C.c_uint32, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_scene_refine_window": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams),
            C.POINTER(WindowParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_online_refine_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(PoseRefineParams), C.POINTER(PoseC2FParams),
            C.POINTER(WindowParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_object_set_pose": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mon_online_set_object_pose": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    "mon_checkpoint_read_info": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p]),
    "mon_object_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mon_object_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mon_online_save_map": (C.c_int, [C.c_void_p, C.c_char_p]),
    "mon_online_load_map": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_size_t)]),
}


# every symbol include/mon_core_diag.h declares (libmon_core_diag.so: diagnostics and test scaffolding, not the product)
_DIAG_SIGS = {
    "mon_object_debug_read": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "mon_dataset_debug_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_microbench": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "mon_debug_frag_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mon_debug_acc_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    "mon_debug_fast_index": (C.c_int, [C.POINTER(MonConfig), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mon_selftest_mfma": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_debug_yaml_number": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_double)]),
    "mon_debug_render_jobs": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]),
    "mon_debug_occupancy_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "mon_debug_occupancy_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    "mon_debug_set_train_occupancy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mon_debug_set_render_grid": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mon_debug_checkpoint_timing": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "mon_debug_paths_stats": (C.c_int, [C.c_void_p]),
    "mon_debug_encode_block": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mon_debug_scene_samples": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, MonBBox, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_debug_scene_composite": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_debug_scene_probe_rays": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "mon_debug_scene_probe_composite": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_debug_scene_cast_rays": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mon_debug_scene_cast_composite": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_debug_scene_point_rows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
    "mon_debug_scene_gradient_rows": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mon_debug_pose_samples": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(PoseRefineParams), C.c_uint32, C.c_void_p,
            C.c_void_p, C.c_void_p]),
    "mon_debug_scene_pose_samples": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(PoseRefineParams), C.c_uint32,
            C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_debug_scene_composite_grad": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def exported_symbols():
    return sorted(_SIGS)


# libmon_core_rccl.so (include/mon_core_rccl.h): the in-process gather-to-root over RCCL
_RCCL_SIGS = {
    "mon_gather_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mon_gather_destroy": (C.c_int, [C.c_void_p]),
    "mon_gather_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mon_gather_renders": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mon_gather_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "mon_gather_transport_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "mon_gather_set_transport": (C.c_int, [C.c_void_p, C.c_int]),
    "mon_gather_last_error": (C.c_char_p, []),
    "mon_offline_render_test_gathered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]),
}
_rccl_lib = None


def rccl_symbols():
    return sorted(_RCCL_SIGS)


def rccl_lib_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libmon_core_rccl.so")


def rccl_lib():
    """libmon_core_rccl.so next to libmon_core.so (the core is loaded first: the gather library resolves its symbols against it)."""
    global _rccl_lib
    if _rccl_lib is None:
        lib()
        L = C.CDLL(rccl_lib_path(), mode=C.RTLD_GLOBAL)
        for name, (res, args) in _RCCL_SIGS.items():
            f = getattr(L, name); f.restype = res; f.argtypes = args
        _rccl_lib = L
    return _rccl_lib


def gather_plan(object_device, n_pix, n_devices):
    d = np.ascontiguousarray(object_device, np.int32); p = np.ascontiguousarray(n_pix, np.uint32)
    per = np.zeros(n_devices, np.uint64); off = np.zeros(len(d), np.uint64)
    rc = rccl_lib().mon_gather_plan(_p(d), _p(p), len(d), int(n_devices), _p(per), _p(off))
    if rc:
        raise MonError(rc, "mon_gather_plan failed")
    return per, off


def _gather_error():
    return (rccl_lib().mon_gather_last_error() or b"").decode("utf-8", "replace")


class Gather:
    """mon_gather: single-process RCCL communicator over the visible devices + the gather-to-root of rendered crops."""

    def __init__(self, root_device=0):
        self.h = C.c_void_p()
        rc = rccl_lib().mon_gather_create(int(root_device), C.byref(self.h))
        if rc:
            raise MonError(rc, "mon_gather_create: " + _gather_error())

    AUTO, RCCL, PEER_COPY = 0, 1, 2

    def set_transport(self, transport):
        rc = rccl_lib().mon_gather_set_transport(self.h, int(transport))
        if rc:
            raise MonError(rc, "mon_gather_set_transport: " + _gather_error())

    def renders(self, objects, boxes, poses16, pose_is_Toc=False):
        n = len(objects); b = np.ascontiguousarray(boxes, np.uint32).reshape(n, 5); T = np.ascontiguousarray(poses16, np.float32).reshape(n, 16)
        oh = (C.c_void_p * n)(*[o.h for o in objects])
        rgb = [np.empty((int(q[3]), int(q[4]), 3), np.float32) for q in b]; dep = [np.empty((int(q[3]), int(q[4])), np.float32) for q in b]
        msk = [np.empty_like(d) for d in dep]
        pr = (C.c_void_p * n)(*[a.ctypes.data for a in rgb]); pd = (C.c_void_p * n)(*[a.ctypes.data for a in dep])
        pm = (C.c_void_p * n)(*[a.ctypes.data for a in msk])
        rc = rccl_lib().mon_gather_renders(self.h, oh, _p(b), _p(T), int(pose_is_Toc), n, pr, pd, pm)
        if rc:
            raise MonError(rc, "mon_gather_renders: " + _gather_error())
        return list(zip(rgb, dep, msk))

    def stats(self):
        a = C.c_uint64(0); b = C.c_uint64(0); s = C.c_int(0); ms = C.c_double(0)
        rccl_lib().mon_gather_stats(self.h, C.byref(a), C.byref(b), C.byref(s), C.byref(ms))
        nr = C.c_int(0); br = C.c_uint64(0); mr = C.c_int(0); bc = C.c_uint64(0); mc = C.c_int(0)
        rccl_lib().mon_gather_transport_stats(self.h, C.byref(nr), C.byref(br), C.byref(mr), C.byref(bc), C.byref(mc))
        return dict(bytes_over_links=a.value, bytes_on_root=b.value, sending_devices=s.value, transfer_ms=ms.value, n_ranks=nr.value, bytes_rccl=br.value,
                messages_rccl=mr.value, bytes_peer_copy=bc.value, messages_peer_copy=mc.value)

    def offline_render_test(self, manager, out_dir, max_views=0):
        rc = rccl_lib().mon_offline_render_test_gathered(self.h, manager.h, out_dir.encode(), int(max_views))
        if rc:
            raise MonError(rc, "mon_offline_render_test_gathered: " + _gather_error())

    def close(self):
        if self.h:
            rccl_lib().mon_gather_destroy(self.h); self.h = C.c_void_p()


def diag_symbols():
    return sorted(_DIAG_SIGS)


def lib_path():
    """In-tree library; MON_CORE_LIB points tooling at an instrumented / experimental build of the same sources (tools/variant_build.sh)."""
    return os.environ.get("MON_CORE_LIB") or os.path.join(_HERE, "libmon_core.so")


_lib = None


def lib():
    """Loads libmon_core.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise MonError(-1, "libmon_core.so not built (run python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(p)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name); fn.restype = res; fn.argtypes = args
        _lib = L
        # harness convenience (tools / tests that run in a subprocess): MON_OPTIONS="name=value,..." -> mon_set_option calls
        for kv in filter(None, os.environ.get("MON_OPTIONS", "").split(",")):
            k, v = kv.split("=")
            if k.strip() == "offline_schedule":          # "offline_schedule=OUTERxINNER"
                o, i = v.lower().split("x"); rc = L.mon_offline_set_schedule(int(o), int(i))
            else:
                rc = L.mon_set_option(k.strip().encode(), int(v))
            if rc != 0:
                raise MonError(rc, L.mon_last_error().decode("utf-8", "replace"))
    return _lib


_diag = None


def diag_lib_path():
    return os.path.join(os.path.dirname(lib_path()), "libmon_core_diag.so")


def diag_lib():
    """Loads libmon_core_diag.so (after libmon_core.so, which it links against)."""
    global _diag
    if _diag is None:
        lib()
        p = diag_lib_path()
        if not os.path.exists(p):
            raise MonError(-1, "libmon_core_diag.so not built")
        L = C.CDLL(p)
        for name, (res, args) in _DIAG_SIGS.items():
            fn = getattr(L, name); fn.restype = res; fn.argtypes = args
        _diag = L
    return _diag


def set_option(name, value):
    """Process-wide test / tuning switch (include/mon_core.h: mon_set_option)."""
    _check(lib().mon_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_long(0); _check(lib().mon_get_option(name.encode(), C.byref(v))); return v.value


def yaml_number(text, key):
    v = C.c_double(0); _check(diag_lib().mon_debug_yaml_number(text.encode(), key.encode(), C.byref(v))); return v.value


def _check(rc):
    if rc != 0:
        raise MonError(rc, lib().mon_last_error().decode("utf-8", "replace"))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    rc = lib().mon_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def set_offline_schedule(outer=10, inner=500):
    """NerfManagerOffline's outer x inner training iterations per object (reference: 10 x 500), read by Offline.init."""
    _check(lib().mon_offline_set_schedule(int(outer), int(inner)))


def set_logical_devices(n):
    """n logical devices mapped round-robin onto the physical GPUs (0 = the physical devices themselves)."""
    _check(lib().mon_set_logical_devices(int(n)))


def device_mem_info(device=0):
    """(free, total) bytes of device memory (hipMemGetInfo)."""
    f = C.c_size_t(0); t = C.c_size_t(0); _check(lib().mon_device_mem_info(int(device), C.byref(f), C.byref(t))); return f.value, t.value


def default_config(**kw):
    c = MonConfig(); _check(lib().mon_config_default(C.byref(c)))
    kw = dict(kw)
    # "same inputs" mode (mon_config.rng_flags): xorwow = 0 counter RNG | 1 cuRAND flavour | 2 rocRAND flavour, xorwow_lanes (multiple of 1024, default 4096),
    # tcnn_init_order
    rng = int(kw.pop("xorwow", 0)) | (int(bool(kw.pop("tcnn_init_order", 0))) << 4) | ((int(kw.pop("xorwow_lanes", 0)) // 1024) << 16)
    for k, v in kw.items():
        setattr(c, k, v)
    c.rng_flags |= rng
    return c


def config_from_json(path):
    c = MonConfig(); _check(lib().mon_config_from_json(path.encode(), C.byref(c))); return c


def selftest_mfma(A_h, B_h, device=0):
    A = np.ascontiguousarray(A_h, np.uint16); B = np.ascontiguousarray(B_h, np.uint16); D = np.empty((32, 32), np.float32)
    _check(diag_lib().mon_selftest_mfma(device, _p(A), _p(B), _p(D))); return D


def fast_index(cfg, level, x, y, z):
    i = C.c_uint32(0); n = C.c_uint32(0); _check(diag_lib().mon_debug_fast_index(C.byref(cfg), level, x, y, z, C.byref(i), C.byref(n))); return i.value, n.value


def microbench(mode, pattern, n_entries, n_ops, device=0):
    ms = C.c_float(0); _check(diag_lib().mon_microbench(device, mode, pattern, n_entries, n_ops, C.byref(ms))); return ms.value


class Dataset:
    """nerf::NeRF_Dataset on one device (frames resident in HBM)."""

    def __init__(self, device, H, W, fx, fy, cx, cy, max_frames, use_depth=False):
        self.h = C.c_void_p(); self.H, self.W = H, W
        _check(lib().mon_dataset_create(device, H, W, fx, fy, cx, cy, max_frames, int(use_depth), C.byref(self.h)))

    def add_frame(self, frame_id, rgb_u8, instance_u8, Twc16, depth=None, is_bgr=False):
        rgb = np.ascontiguousarray(rgb_u8, np.uint8); inst = np.ascontiguousarray(instance_u8, np.uint8)
        pose = np.ascontiguousarray(Twc16, np.float32); d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        assert rgb.shape[:2] == (self.H, self.W) and inst.shape == (self.H, self.W) and pose.size == 16
        _check(lib().mon_dataset_add_frame(self.h, frame_id, _p(rgb), rgb.shape[2], int(is_bgr), _p(inst), _p(d), _p(pose)))

    @property
    def n_frames(self):
        n = C.c_uint32(0); _check(lib().mon_dataset_n_frames(self.h, C.byref(n))); return n.value

    def debug_read(self, frame_id, with_depth=False):
        """(diagnostics library) what the device holds for one frame: packed rgba | instance << 24, depth or None, pose (Twc, column-major)."""
        rgba = np.empty((self.H, self.W), np.uint32); pose = np.empty(16, np.float32); dep = np.empty((self.H, self.W), np.float32) if with_depth else None
        _check(diag_lib().mon_dataset_debug_read(self.h, frame_id, _p(rgba), _p(dep), _p(pose)))
        return rgba, dep, pose

    def close(self):
        if self.h:
            lib().mon_dataset_destroy(self.h); self.h = None


# debug buffer ids (ro-map_amd/csrc/model.h MON_BUF_*): name -> (id, dtype, elements as f(R, B, info))
BUF = dict(master=0, half=1, ema=2, m1=3, m2=4, steps=5, gmlp=6, ggrid_h=9, pts=10, tdist=11, E=12, Hid=13, O=14, dO=15, dHid=16, dE=17,
           rgb_ray=18, depth_ray=19, mask_ray=20, loss_ray=21, ray_o=22, ray_d=23, ray_t0=24, ray_t1=25, target=26, target_depth=27, bgcol=28,
           ray_flag=29, ray_dn=31, mask=32, state=33, frag_train=34, frag_ref=35, x_all=36, e_soa=37, half_tiles=38, ggrid_f32=39, live_cnt=40)


class ObjectNeRF:
    """nerf::NeRF + nerf::NeRF_Model for one object."""

    def __init__(self, dataset, cfg, class_id, Tow16, aabb_min, aabb_max):
        self.h = C.c_void_p(); self.cfg = cfg; self.ds = dataset
        a, b, c = (np.ascontiguousarray(v, np.float32) for v in (Tow16, aabb_min, aabb_max))
        _check(lib().mon_object_create(dataset.h, C.byref(cfg), int(class_id), _p(a), _p(b), _p(c), C.byref(self.h)))
        self.R, self.S = cfg.rays_per_batch, cfg.n_samples

    def close(self):
        if self.h:
            lib().mon_object_destroy(self.h); self.h = None

    def add_boxes(self, boxes):
        b = np.ascontiguousarray(boxes, np.uint32).reshape(-1, 5)
        _check(lib().mon_object_add_boxes(self.h, _p(b), b.shape[0]))

    def save(self, path):
        """mon_object_save: the whole object -- parameters, optimizer state, EMA, counters, occupancy grid, boxes -- as one checkpoint file (written to
        <path>.tmp, then renamed).  Read-only; serialise against training as for render."""
        _check(lib().mon_object_save(self.h, os.fsencode(path)))

    @classmethod
    def load(cls, dataset, path, with_boxes=True):
        """mon_object_load: the saved object on `dataset`'s device, bit for bit; with_boxes restores the box list (the dataset must hold its frames)."""
        h = C.c_void_p()
        _check(lib().mon_object_load(dataset.h, os.fsencode(path), MON_LOAD_BOXES if with_boxes else 0, C.byref(h)))
        o = cls.__new__(cls); o.h = h; o.ds = dataset
        o.cfg = MonConfig(); _check(lib().mon_object_get_config(h, C.byref(o.cfg))); o.R, o.S = o.cfg.rays_per_batch, o.cfg.n_samples
        return o

    def train(self, iters):
        loss = C.c_float(0); _check(lib().mon_object_train(self.h, iters, C.byref(loss))); return loss.value

    def train_stages(self, bits):
        _check(lib().mon_object_train_stages(self.h, bits))

    def set_backend(self, backend):
        _check(lib().mon_object_set_backend(self.h, backend))

    def info(self):
        i = MonInfo(); _check(lib().mon_object_info_get(self.h, C.byref(i))); return i

    def render(self, box, pose16, pose_is_Toc=False):
        FrameId, x, y, h, w = (int(v) for v in box)
        rgb = np.empty((h, w, 3), np.float32); depth = np.empty((h, w), np.float32); mask = np.empty((h, w), np.float32)
        pose = np.ascontiguousarray(pose16, np.float32)
        _check(lib().mon_object_render(self.h, MonBBox(FrameId, x, y, h, w), _p(pose), int(pose_is_Toc), _p(rgb), _p(depth), _p(mask), 0))
        return rgb, depth, mask

    def render_snapshot(self, box, pose16, pose_is_Toc=False):
        """Viewer-side render from the last published inference weights on the inference stream (safe while another thread trains this object);
        returns (rgb, depth, mask, optimizer steps of the weights)."""
        FrameId, x, y, h, w = (int(v) for v in box)
        rgb = np.empty((h, w, 3), np.float32); depth = np.empty((h, w), np.float32); mask = np.empty((h, w), np.float32); st = C.c_uint32(0)
        pose = np.ascontiguousarray(pose16, np.float32)
        _check(lib().mon_object_render_snapshot(self.h, MonBBox(FrameId, x, y, h, w), _p(pose), int(pose_is_Toc), _p(rgb), _p(depth), _p(mask), C.byref(st)))
        return rgb, depth, mask, st.value

    def render_into(self, box, pose16, rgb_ptr, depth_ptr, mask_ptr, on_device, pose_is_Toc=False):
        """NeRF_Model::Render straight into caller-owned buffers given as raw addresses (3hw + hw + hw float32); `on_device`: they are
        HBM addresses of this object's device (e.g. a torch tensor's data_ptr() -- the final-render gather sends them over RCCL as they are)."""
        FrameId, x, y, h, w = (int(v) for v in box)
        pose = np.ascontiguousarray(pose16, np.float32)
        _check(lib().mon_object_render(self.h, MonBBox(FrameId, x, y, h, w), _p(pose), int(pose_is_Toc), C.c_void_p(int(rgb_ptr)), C.c_void_p(int(depth_ptr)),
                C.c_void_p(int(mask_ptr)), int(bool(on_device))))

    def generate_mesh(self, res=64, thresh=2.0):
        """GenerateMesh + TransCPUMesh (nerf_model.cu:1993-2095); returns (n_verts incl. padding, n_indices)."""
        nv = C.c_uint32(0); ni = C.c_uint32(0)
        _check(lib().mon_object_generate_mesh(self.h, int(res), float(thresh), C.byref(nv), C.byref(ni))); return nv.value, ni.value

    def get_mesh(self, try_lock=False, raw=False):
        """CPUMeshData (common.h:32-41) as a dict of numpy arrays.  Counts and data come from one hold of the mesh mutex
        (mon_object_copy_mesh), so this is safe from a viewer thread while the object's thread republishes the mesh."""
        nv = C.c_uint32(0); nr = C.c_uint32(0); ni = C.c_uint32(0)
        _check(lib().mon_object_mesh_counts(self.h, C.byref(nv), C.byref(nr), C.byref(ni)))
        for _ in range(8):
            cv, ci = nv.value, ni.value
            out = dict(verts=np.empty((cv, 3), np.float32), normals=np.empty((cv, 3), np.float32), colors=np.empty((cv, 3), np.uint8), indices=np.empty(ci,
                    np.uint32))
            rc = lib().mon_object_copy_mesh(self.h, cv, ci, _p(out["verts"]), _p(out["normals"]), _p(out["colors"]), _p(out["indices"]),
                                            C.byref(nv), C.byref(nr), C.byref(ni), int(try_lock))
            if rc == 1 and (nv.value > cv or ni.value > ci):
                continue                                            # the mesh grew in between: retry with the reported counts
            _check(rc); break
        else:
            raise MonError(1, "get_mesh: mesh kept growing")
        out = {k: (v[:nv.value] if k != "indices" else v[:ni.value]) for k, v in out.items()}; out["n_verts_real"] = nr.value
        if raw:
            out["normals_raw"] = np.empty((nv.value, 3), np.float32); out["colors_f32"] = np.empty((nv.value, 3), np.float32)
            _check(lib().mon_object_get_mesh_raw(self.h, _p(out["normals_raw"]), _p(out["colors_f32"])))
        return out

    def mesh_generation(self):
        g = C.c_uint64(0); _check(lib().mon_object_mesh_generation(self.h, C.byref(g))); return g.value

    def save_mesh(self, path):
        _check(lib().mon_object_save_mesh(self.h, path.encode()))

    def set_render_skip(self, enable, min_alpha=1e-3):
        """Empty-space skipping of this object's renders (default off): a 64^3 grid of the rendered weights, cells live where alpha >= min_alpha at a
        cell centre or a neighbour's; min_alpha <= 0 keeps every cell (bit-identical images)."""
        _check(lib().mon_object_set_render_skip(self.h, int(bool(enable)), float(min_alpha)))

    def render_skip_stats(self, side=0):
        """Side 0 (train-stream renders) or 1 (snapshot renders): dict of active, live_cells, grid_builds, samples_in_box, samples_live of the last render."""
        st = MonRenderSkipStats(); _check(lib().mon_object_render_skip_stats(self.h, int(side), C.byref(st)))
        return {f: int(getattr(st, f)) for f, _ in MonRenderSkipStats._fields_}

    def render_occupancy(self, side=0, dilated=True):
        """The grid of the side's last skipping render as a (64, 64, 64) bool array indexed [z, y, x]."""
        w = np.empty(8192, np.uint32); _check(lib().mon_object_render_occupancy(self.h, int(side), int(bool(dilated)), _p(w)))
        return np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool).reshape(64, 64, 64)

    def debug_set_render_grid(self, side, grid):
        """Pins a (64, 64, 64) bool grid [z, y, x] as the side's render grid (None: back to the object's own)."""
        if grid is None:
            _check(diag_lib().mon_debug_set_render_grid(self.h, int(side), None)); return
        w = np.packbits(np.ascontiguousarray(grid, bool).reshape(-1), bitorder="little").view(np.uint32)
        _check(diag_lib().mon_debug_set_render_grid(self.h, int(side), _p(w)))

    def density_grid(self, rx, ry, rz):
        out = np.empty(rx * ry * rz, np.float32); _check(lib().mon_object_density_grid(self.h, rx, ry, rz, _p(out))); return out

    def get_params(self, which=0):
        n = self.info().n_params
        out = np.empty(n, np.float32 if which == 0 else np.uint16)
        _check(lib().mon_object_get_params(self.h, which, _p(out), out.nbytes)); return out

    def set_params(self, master):
        m = np.ascontiguousarray(master, np.float32); _check(lib().mon_object_set_params(self.h, _p(m), m.size))

    def buffer(self, name):
        i = self.info(); R, B, n = self.R, self.R * self.S, i.n_params
        W, NH, Ep = self.cfg.n_neurons, self.cfg.n_hidden_layers, i.encoded_width
        shapes = dict(master=(np.float32, n), half=(np.uint16, n), ema=(np.uint16, n), m1=(np.float32, n), m2=(np.float32, n), steps=(np.uint32, n),
                      gmlp=(np.float32, i.n_mlp_params), ggrid_h=(np.uint16, i.n_grid_params), ggrid_f32=(np.float32, i.n_grid_params), pts=(np.float32, B * 3), tdist=(np.float32, B),
                      E=(np.uint16, B * Ep), Hid=(np.uint16, B * W * NH), O=(np.uint16, B * 4), dO=(np.uint16, B * 4), dHid=(np.uint16, B * W * NH),
                      dE=(np.uint16, B * Ep), rgb_ray=(np.float32, R * 3), depth_ray=(np.float32, R), mask_ray=(np.float32, R), loss_ray=(np.float32, R),
                      ray_o=(np.float32, R * 3), ray_d=(np.float32, R * 3), ray_t0=(np.float32, R), ray_t1=(np.float32, R), target=(np.float32, R * 3),
                      target_depth=(np.float32, R), bgcol=(np.float32, R * 3), ray_flag=(np.uint8, R), ray_dn=(np.float32, R), mask=(np.uint64, R // 64),
                      state=(np.uint32, 28 + 2 * 128 * 16), frag_train=(np.uint16, 64 * 512), frag_ref=(np.uint16, 64 * 512),
                      live_cnt=(np.uint32, 2 * 64 * 16), x_all=(np.float32, B * 4), e_soa=(np.uint16, B * 2 * self.cfg.n_levels), half_tiles=(np.uint16, i.n_grid_params))
        dt, cnt = shapes[name]; out = np.empty(cnt, dt)
        _check(diag_lib().mon_object_debug_read(self.h, BUF[name], _p(out), out.nbytes)); return out

    def occupancy_state(self):
        out = (C.c_uint32 * 2)(); _check(diag_lib().mon_debug_occupancy_state(self.h, out)); return int(out[0]), int(out[1])

    def occupancy_grid(self):
        """Training's occupancy grid: (raw bits, dilated bits, raw-density threshold, number of live-sample lists); 8192 words each, x fastest."""
        raw = np.empty(8192, np.uint32); dil = np.empty(8192, np.uint32); thr = C.c_float(0); n_parts = C.c_uint32(0)
        _check(diag_lib().mon_debug_occupancy_grid(self.h, _p(raw), _p(dil), C.byref(thr), C.byref(n_parts)))
        return raw, dil, float(thr.value), int(n_parts.value)

    def set_train_occupancy(self, bits):
        """Pins a training occupancy grid (8192 words) in place of the object's own; None unpins."""
        if bits is None:
            _check(diag_lib().mon_debug_set_train_occupancy(self.h, None)); return
        w = np.ascontiguousarray(bits, np.uint32); assert w.size == 8192
        _check(diag_lib().mon_debug_set_train_occupancy(self.h, _p(w)))

    def render_jobs(self, side=0):
        """Jobs (rays that hit the box) of the last crop the tile render evaluated on this object's device (side 0: train stream, 1: inference stream)."""
        n = C.c_uint32(0); _check(diag_lib().mon_debug_render_jobs(self.h, int(side), C.byref(n))); return n.value

    def pose_loss(self, obs, Tow16, params=None, side=0, iteration=0):
        """mon_object_pose_loss: (loss, grad6 = dL/d(rho, phi)) of pose Tow16 (column-major, world -> object) against the boxes obs [(FrameId, x, y, h, w)]."""
        b, prm = _pose_boxes(obs), _pose_params(params); pose = np.ascontiguousarray(Tow16, np.float32).reshape(16)
        loss = C.c_float(0); g = np.empty(6, np.float32)
        _check(lib().mon_object_pose_loss(self.h, int(side), _p(b), b.shape[0], _p(pose), C.byref(prm), int(iteration), C.byref(loss), _p(g)))
        return loss.value, g

    def refine_pose(self, obs, Tow16, params=None, side=0):
        """mon_object_refine_pose: params.iters Adam steps from Tow16; returns (refined Tow16, loss trace of iters + 1 values).  The object is not changed."""
        b, prm = _pose_boxes(obs), _pose_params(params); pose = np.array(Tow16, np.float32).reshape(16)
        trace = np.empty(prm.iters + 1, np.float32)
        _check(lib().mon_object_refine_pose(self.h, int(side), _p(b), b.shape[0], C.byref(prm), _p(pose), _p(trace)))
        return pose, trace

    def pose_loss_levels(self, obs, Tow16, level_weights, params=None, side=0, iteration=0):
        """mon_object_pose_loss_levels: pose_loss with level l's share of the position gradient scaled by level_weights[l] (one per level); the loss is
        pose_loss's."""
        b, prm = _pose_boxes(obs), _pose_params(params); pose = np.ascontiguousarray(Tow16, np.float32).reshape(16)
        w = np.ascontiguousarray(level_weights, np.float32).reshape(-1)
        if w.size != self.cfg.n_levels:
            raise ValueError("level_weights: %d values for %d levels" % (w.size, self.cfg.n_levels))
        loss = C.c_float(0); g = np.empty(6, np.float32)
        _check(lib().mon_object_pose_loss_levels(self.h, int(side), _p(b), b.shape[0], _p(pose), C.byref(prm), int(iteration), _p(w), C.byref(loss), _p(g)))
        return loss.value, g

    def set_pose(self, Tow16):
        """mon_object_set_pose: stores a new Tow (column-major) in the object; weights and training state stay."""
        T = np.ascontiguousarray(Tow16, np.float32).reshape(16); _check(lib().mon_object_set_pose(self.h, _p(T)))

    def refine_pose_c2f(self, obs, Tow16, params=None, c2f=None, side=0):
        """mon_object_refine_pose_c2f: refine_pose with the coarse-to-fine level schedule c2f (PoseC2FParams, a dict of overrides, or None = defaults)."""
        b, prm, c = _pose_boxes(obs), _pose_params(params), _c2f_params(c2f); pose = np.array(Tow16, np.float32).reshape(16)
        trace = np.empty(prm.iters + 1, np.float32)
        _check(lib().mon_object_refine_pose_c2f(self.h, int(side), _p(b), b.shape[0], C.byref(prm), C.byref(c), _p(pose), _p(trace)))
        return pose, trace

    def pose_samples(self, obs, Tow16, params=None, side=0, iteration=0):
        """mon_debug_pose_samples: per drawn ray of that evaluation, positions (n, 64, 3), raw outputs (n, 64, 4) and dL/dx (n, 64, 3), object frame."""
        b, prm = _pose_boxes(obs), _pose_params(params); pose = np.ascontiguousarray(Tow16, np.float32).reshape(16)
        n = int(prm.rays_per_iter) or int(sum(int(v[3]) * int(v[4]) for v in b))
        x = np.empty((n, 64, 3), np.float32); raw = np.empty((n, 64, 4), np.float32); g = np.empty((n, 64, 3), np.float32)
        _check(diag_lib().mon_debug_pose_samples(self.h, int(side), _p(b), b.shape[0], _p(pose), C.byref(prm), int(iteration), _p(x), _p(raw), _p(g)))
        return x, raw, g

    def set_debug_dump(self, on):
        _check(lib().mon_object_set_debug_dump(self.h, int(on)))

    def set_profiling(self, on):
        _check(lib().mon_object_set_profiling(self.h, int(on)))

    def profile(self, reset=True):
        p = MonProfile(); _check(lib().mon_object_get_profile(self.h, C.byref(p), int(reset)))
        return {"ms": list(p.ms), "launches": list(p.launches)}


def png_read(path):
    w, h, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _check(lib().mon_png_read(path.encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(d), None, 0))
    buf = np.empty(w.value * h.value * c.value * d.value // 8, np.uint8)
    _check(lib().mon_png_read(path.encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(d), _p(buf), buf.nbytes))
    if d.value == 16:
        return buf.view(">u2").astype(np.uint16).reshape(h.value, w.value, c.value)
    return buf.reshape(h.value, w.value, c.value)


def png_write(path, arr):
    a = np.asarray(arr)
    if a.ndim == 2:
        a = a[..., None]
    data = np.ascontiguousarray(a.astype(">u2") if a.dtype == np.uint16 else a.astype(np.uint8))
    _check(lib().mon_png_write(path.encode(), a.shape[1], a.shape[0], a.shape[2], 16 if arr.dtype == np.uint16 else 8, data.ctypes.data_as(C.c_void_p)))


class OfflineManager:
    """nerf::NerfManagerOffline: same call sequence as OfflineNeRF's main() (MON/main.cpp:322-340) minus the viewer."""

    def __init__(self, dataset_path, config_path, use_dense_depth=False):
        self.h = C.c_void_p()
        _check(lib().mon_offline_create(dataset_path.encode(), config_path.encode(), int(use_dense_depth), C.byref(self.h)))

    def init(self):
        _check(lib().mon_offline_init(self.h))

    def read_dataset(self):
        _check(lib().mon_offline_read_dataset(self.h))

    def create_nerf(self, object_file):
        _check(lib().mon_offline_create_nerf(self.h, object_file.encode()))

    def wait_threads_end(self):
        _check(lib().mon_offline_wait_threads_end(self.h))

    def n_objects(self):
        n = C.c_int(0); _check(lib().mon_offline_n_objects(self.h, C.byref(n))); return n.value

    def object_loss(self, idx):
        l = C.c_float(0); d = C.c_int(0); _check(lib().mon_offline_object_loss(self.h, idx, C.byref(l), C.byref(d))); return l.value, d.value

    def set_output_dir(self, path):
        _check(lib().mon_offline_set_output_dir(self.h, path.encode()))

    def intrinsics(self):
        f = [C.c_float(0) for _ in range(4)]; hw = [C.c_int(0), C.c_int(0)]
        _check(lib().mon_offline_get_intrinsics(self.h, *[C.byref(v) for v in f + hw])); return tuple(v.value for v in f + hw)

    def poses(self):
        n = C.c_size_t(0); _check(lib().mon_offline_get_poses(self.h, None, 0, C.byref(n)))
        T = np.empty((n.value, 16), np.float32); _check(lib().mon_offline_get_poses(self.h, _p(T), n.value, C.byref(n))); return T

    def object_meta(self, idx):
        n = C.c_size_t(0); cls = C.c_int(0); Tow = np.empty(16, np.float32); a0 = np.empty(3, np.float32); a1 = np.empty(3, np.float32)
        _check(lib().mon_offline_object_meta(self.h, idx, C.byref(cls), _p(Tow), _p(a0), _p(a1), None, 0, C.byref(n)))
        boxes = np.empty((n.value, 5), np.uint32)
        _check(lib().mon_offline_object_meta(self.h, idx, None, None, None, None, _p(boxes), n.value, C.byref(n)))
        return dict(cls=cls.value, Tow=Tow, aabb_min=a0, aabb_max=a1, boxes=boxes)

    def object(self, idx):
        """Borrowed handle of object idx (GetAllNeRF()[idx]); owned by the manager."""
        h = C.c_void_p(); _check(lib().mon_offline_object(self.h, idx, C.byref(h))); return _borrowed_object(h)

    def render_test(self, idx, out_dir, max_views=0):
        _check(lib().mon_offline_render_test(self.h, idx, out_dir.encode(), max_views))

    def close(self):
        if self.h:
            lib().mon_offline_destroy(self.h); self.h = None


class OnlineManager:
    """nerf::NerfManagerOnline as the SLAM frontend drives it (REF/src/System.cc:120-138, LocalMapping.cc:1122-1270)."""

    def __init__(self, config_path, use_sparse_depth=False, train_step_iterations=500):
        self.h = C.c_void_p()
        _check(lib().mon_online_create(config_path.encode(), int(use_sparse_depth), int(train_step_iterations), C.byref(self.h)))

    def init(self):
        _check(lib().mon_online_init(self.h))

    def dataset_init(self, fx, fy, cx, cy, H, W, imgs):
        _check(lib().mon_online_dataset_init(self.h, fx, fy, cx, cy, H, W, imgs))

    def new_frame(self, img_id, stamp, bgr_u8, instance_u8, Twc16, depth=None):
        bgr = np.ascontiguousarray(bgr_u8, np.uint8); inst = np.ascontiguousarray(instance_u8, np.uint8); pose = np.ascontiguousarray(Twc16, np.float32)
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        _check(lib().mon_online_new_frame(self.h, img_id, stamp.encode(), _p(bgr), bgr.shape[2], _p(inst), _p(d), _p(pose)))

    def create_nerf(self, cls, Tow16, aabb_min, aabb_max):
        a, b, c = (np.ascontiguousarray(v, np.float32) for v in (Tow16, aabb_min, aabb_max)); idx = C.c_size_t(0)
        _check(lib().mon_online_create_nerf(self.h, int(cls), _p(a), _p(b), _p(c), C.byref(idx))); return idx.value

    def update_nerf_bbox(self, idx, boxes, train_step):
        b = np.ascontiguousarray(boxes, np.uint32).reshape(-1, 5)
        _check(lib().mon_online_update_nerf_bbox(self.h, idx, _p(b), b.shape[0], int(train_step)))

    def update_dataset(self, cur_id, Twc16s):
        """UpdateDataset: poses of the len(Twc16s) frames before cur_id replaced on every device."""
        T = np.ascontiguousarray(Twc16s, np.float32).reshape(-1, 16); _check(lib().mon_online_update_dataset(self.h, int(cur_id), T.shape[0], _p(T)))

    def get_pose(self, frame_id):
        T = np.empty(16, np.float32); _check(lib().mon_online_get_pose(self.h, int(frame_id), _p(T))); return T

    def get_frame_idx(self, stamp):
        i = C.c_int(0); _check(lib().mon_online_get_frame_idx(self.h, stamp.encode(), C.byref(i))); return i.value

    def wait_threads_end(self):
        _check(lib().mon_online_wait_threads_end(self.h))

    def object(self, idx):
        h = C.c_void_p(); _check(lib().mon_online_object(self.h, idx, C.byref(h))); return _borrowed_object(h)

    def render_nerfs_test(self, out_path, idx, stamps, boxes, Twcs16, radius):
        b = np.ascontiguousarray(boxes, np.uint32).reshape(-1, 5); T = np.ascontiguousarray(Twcs16, np.float32).reshape(-1, 16)
        arr = (C.c_char_p * len(stamps))(*[s.encode() for s in stamps])
        _check(lib().mon_online_render_nerfs_test(self.h, out_path.encode(), idx, arr, _p(b), _p(T), len(stamps), float(radius)))

    def object_info(self, idx):
        l = C.c_float(0); t = C.c_int(0); d = C.c_int(0); n = C.c_uint32(0)
        _check(lib().mon_online_object_info(self.h, idx, C.byref(l), C.byref(t), C.byref(d), C.byref(n)))
        return dict(loss=l.value, train_calls=t.value, device=d.value, n_boxes=n.value)

    def render(self, idx, box, Twc16):
        FrameId, x, y, h, w = (int(v) for v in box)
        rgb = np.empty((h, w, 3), np.float32); depth = np.empty((h, w), np.float32); mask = np.empty((h, w), np.float32)
        pose = np.ascontiguousarray(Twc16, np.float32)
        _check(lib().mon_online_render(self.h, idx, MonBBox(FrameId, x, y, h, w), _p(pose), _p(rgb), _p(depth), _p(mask))); return rgb, depth, mask

    def render_scene(self, rect, Twc16):
        """mon_online_render_scene: every object with published weights composited in depth order (a viewer's call, safe while they train);
        returns (rgb, depth, opacity, instance = the manager's object index or -1)."""
        box, out = _scene_outputs(rect); pose = np.ascontiguousarray(Twc16, np.float32)
        _check(lib().mon_online_render_scene(self.h, box, _p(pose), *[_p(a) for a in out]))
        return out

    def probe_scene(self, queries, Twc16s):
        """mon_online_probe_scene: probe_scene on side 1 over every object with published weights (a front end's call, safe while they train); both
        instance outputs hold the manager's object indices."""
        q, poses, out = _probe_args(queries, Twc16s)
        _check(lib().mon_online_probe_scene(self.h, _p(poses), poses.shape[0], _p(q), q.shape[0], *[_p(a) for a in out]))
        return out

    def cast_rays(self, rays, hit_opacity=0.5):
        """mon_online_cast_rays: cast_scene on side 1 over every object with published weights (a planner's call, safe while they train); both instance
        outputs hold the manager's object indices."""
        r, out = _cast_args(rays)
        _check(lib().mon_online_cast_rays(self.h, _p(r), r.shape[0], float(hit_opacity), *[_p(a) for a in out]))
        return out

    def query_points(self, world_xyz):
        """mon_online_query_points: query_scene_points on side 1 over every object with published weights (safe while they train); owner holds the
        manager's object indices."""
        x = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3); out = _point_outputs(x.shape[0])
        _check(lib().mon_online_query_points(self.h, _p(x), x.shape[0], *[_p(a) for a in out]))
        return out

    def query_lattice(self, origin, step, shape):
        """mon_online_query_lattice: query_scene_lattice on side 1 over every object with published weights; owner holds the manager's object indices."""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _point_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0))
        _check(lib().mon_online_query_lattice(self.h, _p(o), _p(s), nx, ny, nz, *[_p(a) for a in out]))
        return out

    def distance_lattice(self, origin, step, shape, sigma_min, max_dist=np.inf, free=True):
        """mon_online_distance_lattice: scene_distance_lattice on side 1 over every object with published weights (safe while they train);
        nearest_owner holds the manager's object indices."""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _distance_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0), free)
        _check(lib().mon_online_distance_lattice(self.h, _p(o), _p(s), nx, ny, nz, float(sigma_min), float(max_dist), *[_p(a) for a in out]))
        return out

    def dist_field(self, origin, step, shape, sigma_min, max_dist):
        """mon_online_dist_field: scene_dist_field on side 1 over every object with published weights -> DistField, which does not follow later training and
        stays valid after the manager is gone"""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape); h = C.c_void_p()
        _check(lib().mon_online_dist_field(self.h, _p(o), _p(s), nx, ny, nz, float(sigma_min), float(max_dist), C.byref(h)))
        return DistField(h)

    def signed_distance_lattice(self, origin, step, shape, sigma_min, max_dist=np.inf, log=True):
        """mon_online_signed_distance_lattice: scene_signed_distance_lattice on side 1 over every object with published weights (safe while they train);
        nearest_owner holds the manager's object indices."""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _signed_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0))
        _check(lib().mon_online_signed_distance_lattice(self.h, _p(o), _p(s), nx, ny, nz, float(sigma_min), MON_SIGNED_LOG if log else 0, float(max_dist),
                                                        *[_p(a) for a in out]))
        return out[:5] + (float(out[5][0]),)

    def signed_dist_field(self, origin, step, shape, sigma_min, max_dist, log=True):
        """mon_online_signed_dist_field: scene_signed_dist_field on side 1 over every object with published weights -> DistField, which does not follow
        later training and stays valid after the manager is gone"""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape); h = C.c_void_p()
        _check(lib().mon_online_signed_dist_field(self.h, _p(o), _p(s), nx, ny, nz, float(sigma_min), MON_SIGNED_LOG if log else 0, float(max_dist),
                                                  C.byref(h)))
        return DistField(h)

    def components_lattice(self, origin, step, shape, sigma_min, region=0, clearance=0.0, connectivity=6, cap=None, rows=()):
        """mon_online_components_lattice: scene_components_lattice on side 1 over every object with published weights (safe while they train); the
        owner row holds the manager's object indices."""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape)
        return _components_call(lambda *a: lib().mon_online_components_lattice(self.h, _p(o), _p(s), nx, ny, nz, float(sigma_min), int(region),
                                                                                float(clearance), int(connectivity), *a),
                                max(nx, 0) * max(ny, 0) * max(nz, 0), cap, rows)

    def paths_lattice(self, origin, step, shape, sigma_min, seeds, clearance=0.0, soft_radius=0.0, soft_weight=0.0, connectivity=26, max_cost=np.inf,
                      rows=()):
        """mon_online_paths_lattice: scene_paths_lattice on side 1 over every object with published weights (safe while they train); the owner row
        holds the manager's object indices."""
        o, s, nx, ny, nz = _lattice_args(origin, step, shape)
        return _paths_call(lambda sd, ns, *a: lib().mon_online_paths_lattice(self.h, _p(o), _p(s), nx, ny, nz, float(sigma_min), float(clearance),
                                                                              float(soft_radius), float(soft_weight), int(connectivity), sd, ns,
                                                                              float(max_cost), *a),
                           max(nx, 0) * max(ny, 0) * max(nz, 0), seeds, rows)

    def query_gradients(self, world_xyz, level_weights=None, select=None):
        """mon_online_query_gradients: query_scene_gradients on side 1 over every object with published weights (safe while they train); owner and
        select hold the manager's object indices."""
        x = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3); out = _gradient_outputs(x.shape[0])
        w = _weights_arg(level_weights); s = _select_arg(select, x.shape[0])
        _check(lib().mon_online_query_gradients(self.h, _p(x), x.shape[0], _p(w), _p(s), *[_p(a) for a in out]))
        return out

    def cast_normals(self, rays, hit_opacity=0.5, level_weights=None):
        """mon_online_cast_normals: cast_scene_normals on side 1 over every object with published weights; the instance outputs hold the manager's
        object indices."""
        r, out = _cast_args(rays); out = out + _normal_outputs(r.shape[0]); w = _weights_arg(level_weights)
        _check(lib().mon_online_cast_normals(self.h, _p(r), r.shape[0], float(hit_opacity), _p(w), *[_p(a) for a in out]))
        return out

    def save_map(self, path):
        """mon_online_save_map: <path>/map.txt + one checkpoint per object, each under its own model lock (safe while they train; not one global cut)."""
        _check(lib().mon_online_save_map(self.h, os.fsencode(path)))

    def load_map(self, path, with_boxes=True):
        """mon_online_load_map (after dataset_init, and after new_frame of the frames the boxes name): appends the map's objects with their training
        threads; returns how many."""
        n = C.c_size_t(0); _check(lib().mon_online_load_map(self.h, os.fsencode(path), MON_LOAD_BOXES if with_boxes else 0, C.byref(n))); return n.value

    def refine_pose(self, idx, obs, Tow16, params=None):
        """mon_online_refine_pose: object idx's published snapshot, safe while the manager trains; returns (refined Tow16, loss trace)."""
        b, prm = _pose_boxes(obs), _pose_params(params); pose = np.array(Tow16, np.float32).reshape(16)
        trace = np.empty(prm.iters + 1, np.float32)
        _check(lib().mon_online_refine_pose(self.h, int(idx), _p(b), b.shape[0], C.byref(prm), _p(pose), _p(trace)))
        return pose, trace

    def refine_pose_c2f(self, idx, obs, Tow16, params=None, c2f=None):
        """mon_online_refine_pose_c2f: refine_pose with the coarse-to-fine level schedule, on object idx's published snapshot."""
        b, prm, c = _pose_boxes(obs), _pose_params(params), _c2f_params(c2f); pose = np.array(Tow16, np.float32).reshape(16)
        trace = np.empty(prm.iters + 1, np.float32)
        _check(lib().mon_online_refine_pose_c2f(self.h, int(idx), _p(b), b.shape[0], C.byref(prm), C.byref(c), _p(pose), _p(trace)))
        return pose, trace

    def refine_window(self, obs, Twc16s, Tow16s, params=None, c2f=None, window=None):
        """mon_online_refine_window: the window's camera poses Twc16s (F, 16) and the objects' poses Tow16s (one row of 16 per manager object) refined against every object with published weights, safe while they train.  Returns (Twc16s, Tow16s, included flags per
        manager object, loss trace, frame trace (iters + 1, F)); the manager is not changed."""
        b, prm, wp = _pose_boxes(obs), _pose_params(params), _window_params(window)
        F = len(window_frames(b)); Twc = np.array(Twc16s, np.float32).reshape(F, 16)
        Tow = np.array(Tow16s, np.float32).reshape(-1, 16); n = Tow.shape[0]
        c = None if c2f is None else _c2f_params(None if c2f is True else c2f)
        inc = np.zeros(n, np.uint8); trace = np.empty(prm.iters + 1, np.float32); ftrace = np.empty((prm.iters + 1, F), np.float32)
        _check(lib().mon_online_refine_window(self.h, _p(b), b.shape[0], C.byref(prm), None if c is None else C.byref(c), C.byref(wp), _p(Twc), _p(Tow), n,
                                              _p(inc), _p(trace), _p(ftrace)))
        return Twc, Tow, inc, trace, ftrace

    def set_object_pose(self, idx, Tow16):
        """mon_online_set_object_pose: stores a refined Tow in object idx under its model lock (safe while it trains)."""
        T = np.ascontiguousarray(Tow16, np.float32).reshape(16); _check(lib().mon_online_set_object_pose(self.h, int(idx), _p(T)))

    def refine_camera(self, obs, Twc16, params=None, c2f=None):
        """mon_online_refine_camera: the camera pose of one frame refined against every object with published weights, safe while they train; c2f as
        scene_refine_camera's.  Returns (refined Twc16, loss trace); the manager is not changed (update_dataset stores a pose)."""
        b, prm = _pose_boxes(obs), _pose_params(params); pose = np.array(Twc16, np.float32).reshape(16)
        c = None if c2f is None else _c2f_params(None if c2f is True else c2f)
        trace = np.empty(prm.iters + 1, np.float32)
        _check(lib().mon_online_refine_camera(self.h, _p(b), b.shape[0], C.byref(prm), None if c is None else C.byref(c), _p(pose), _p(trace)))
        return pose, trace

    def relocalise(self, obs, candidates, params=None, c2f=None, reloc=None):
        """mon_online_relocalise: scene_relocalise on side 1 over every object with published weights, safe while they train.  Returns (Twc16, RelocResult,
        scores); the manager is not changed (update_dataset stores a pose)."""
        b, prm, rp = _pose_boxes(obs), _pose_params(params), _reloc_params(reloc)
        cand = np.ascontiguousarray(candidates, np.float32).reshape(-1, 16)
        c = None if c2f is None else _c2f_params(None if c2f is True else c2f)
        pose = np.empty(16, np.float32); res = RelocResult(); scores = np.empty(cand.shape[0], np.float32)
        _check(lib().mon_online_relocalise(self.h, _p(b), b.shape[0], _p(cand), cand.shape[0], C.byref(prm), None if c is None else C.byref(c),
                                           C.byref(rp), _p(pose), C.byref(res), _p(scores)))
        return pose, res, scores

    def close(self):
        if self.h:
            lib().mon_online_destroy(self.h); self.h = None


def pose_refine_default(**overrides):
    """mon_pose_refine_default, then any field overridden by keyword."""
    p = PoseRefineParams(); _check(lib().mon_pose_refine_default(C.byref(p)))
    for k, v in overrides.items():
        if k not in dict(PoseRefineParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _pose_params(params):
    if params is None:
        return pose_refine_default()
    if isinstance(params, dict):
        return pose_refine_default(**params)
    return params


def pose_c2f_default(**overrides):
    """mon_pose_c2f_default, then any field overridden by keyword."""
    c = PoseC2FParams(); _check(lib().mon_pose_c2f_default(C.byref(c)))
    for k, v in overrides.items():
        if k not in dict(PoseC2FParams._fields_):
            raise KeyError(k)
        setattr(c, k, v)
    return c


def pose_c2f_weights(n_levels, iters, step, c2f=None):
    """mon_pose_c2f_weights: the level weights (n_levels float32) of step `step` of an `iters`-step coarse-to-fine refinement."""
    c = _c2f_params(c2f); w = np.empty(int(n_levels), np.float32)
    _check(lib().mon_pose_c2f_weights(C.byref(c), int(n_levels), int(iters), int(step), _p(w)))
    return w


def _c2f_params(c2f):
    if c2f is None:
        return pose_c2f_default()
    if isinstance(c2f, dict):
        return pose_c2f_default(**c2f)
    return c2f


def _pose_boxes(obs):
    return np.ascontiguousarray(obs, np.uint32).reshape(-1, 5)


def _scene_outputs(rect):
    FrameId, x, y, h, w = (int(v) for v in rect)
    return MonBBox(FrameId, x, y, h, w), (np.empty((h, w, 3), np.float32), np.empty((h, w), np.float32), np.empty((h, w), np.float32),
                                          np.empty((h, w), np.int32))


def _handles(objects):
    return (C.c_void_p * len(objects))(*[o.h for o in objects])


def render_scene(objects, rect, Twc16, side=0):
    """mon_scene_render: the objects (one device, one set of intrinsics) composited in depth order over rect = (FrameId, x, y, h, w) seen from Twc16;
    side 0 the train-side weights, 1 the published snapshots.  Returns (rgb HxWx3, depth HxW, opacity HxW, instance HxW int32: index into objects, -1)."""
    box, out = _scene_outputs(rect); pose = np.ascontiguousarray(Twc16, np.float32)
    _check(lib().mon_scene_render(_handles(objects), len(objects), int(side), box, _p(pose), *[_p(a) for a in out]))
    return out


def scene_queries(pose, key, u, v):
    """An array of mon_scene_query (SCENE_QUERY_DTYPE) from broadcastable pose indices, keys and image points."""
    pose, key, u, v = np.broadcast_arrays(np.asarray(pose), np.asarray(key), np.asarray(u), np.asarray(v))
    q = np.empty(pose.size, SCENE_QUERY_DTYPE)
    q["pose"] = pose.reshape(-1); q["key"] = key.reshape(-1); q["u"] = u.reshape(-1); q["v"] = v.reshape(-1)
    return q


def rect_queries(rect, pose=0):
    """Every pixel of rect = (FrameId, x, y, h, w) as a query, row-major, key = the pixel index: the queries whose probe equals render_scene of the rect."""
    _, x, y, h, w = (int(a) for a in rect)
    yy, xx = np.mgrid[0:h, 0:w]
    return scene_queries(pose, yy * w + xx, x + xx, y + yy)


def _probe_args(queries, Twc16s):
    q = np.ascontiguousarray(queries, SCENE_QUERY_DTYPE).reshape(-1); poses = np.ascontiguousarray(Twc16s, np.float32).reshape(-1, 16); n = q.shape[0]
    return q, poses, (np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.float32),
                      np.empty(n, np.int32))


def probe_scene(objects, queries, Twc16s, side=0):
    """mon_scene_probe: what render_scene returns at the queries' sub-pixel image points (SCENE_QUERY_DTYPE: pose index into Twc16s (n_poses, 16), key, u, v),
    plus the first-hit depth and object.  Returns (rgb (n, 3), depth, opacity, instance, hit_depth, hit_instance)."""
    q, poses, out = _probe_args(queries, Twc16s)
    _check(lib().mon_scene_probe(_handles(objects), len(objects), int(side), _p(poses), poses.shape[0], _p(q), q.shape[0], *[_p(a) for a in out]))
    return out


def scene_probe_rays(objects, queries, Twc16s, k, side=0):
    """mon_debug_scene_probe_rays: object k's ray rows of that probe, (n, 10) = o[3], d[3], t0, t1, flag, dn."""
    q, poses, _ = _probe_args(queries, Twc16s); rows = np.empty((q.shape[0], 10), np.float32)
    _check(diag_lib().mon_debug_scene_probe_rays(_handles(objects), len(objects), int(side), _p(poses), poses.shape[0], _p(q), q.shape[0], int(k), _p(rows)))
    return rows


def scene_probe_composite(t, alpha, rgb, count, dn, device=0):
    """mon_debug_scene_probe_composite: the probe's composite kernel on lists laid out as scene_composite's.  Returns (rgb (n_rays, 3), depth, opacity,
    instance, hit_depth, hit_instance)."""
    t = np.ascontiguousarray(t, np.float32); L, R = t.shape[:2]
    a = np.ascontiguousarray(alpha, np.float32).reshape(L, R, 64); c = np.ascontiguousarray(rgb, np.float32).reshape(L, R, 64, 3)
    n = np.ascontiguousarray(count, np.uint32).reshape(L, R); d = np.ascontiguousarray(dn, np.float32).reshape(R)
    out = (np.empty((R, 3), np.float32), np.empty(R, np.float32), np.empty(R, np.float32), np.empty(R, np.int32), np.empty(R, np.float32),
           np.empty(R, np.int32))
    _check(diag_lib().mon_debug_scene_probe_composite(int(device), R, L, _p(t), _p(a), _p(c), _p(n), _p(d), *[_p(o) for o in out]))
    return out


def scene_rays(o, d, t_max=np.inf, key=0):
    """An array of mon_scene_ray (SCENE_RAY_DTYPE) from origins (n, 3), unit directions (n, 3) and broadcastable segment lengths and keys."""
    o = np.asarray(o, np.float32).reshape(-1, 3); d = np.asarray(d, np.float32).reshape(-1, 3)
    r = np.empty(o.shape[0], SCENE_RAY_DTYPE)
    r["o"] = o; r["d"] = d; r["t_max"] = np.broadcast_to(np.asarray(t_max, np.float32), o.shape[:1]); r["key"] = np.broadcast_to(np.asarray(key), o.shape[:1])
    return r


def camera_rays(K, Twc16s, queries):
    """mon_camera_rays (host only): the world rays probe_scene casts for the queries under the pinhole K = (fx, fy, cx, cy).  Returns (rays, dn)."""
    q = np.ascontiguousarray(queries, SCENE_QUERY_DTYPE).reshape(-1); poses = np.ascontiguousarray(Twc16s, np.float32).reshape(-1, 16)
    rays = np.empty(q.shape[0], SCENE_RAY_DTYPE); dn = np.empty(q.shape[0], np.float32)
    _check(lib().mon_camera_rays(float(K[0]), float(K[1]), float(K[2]), float(K[3]), _p(poses), poses.shape[0], _p(q), q.shape[0], _p(rays), _p(dn)))
    return rays, dn


def _cast_args(rays):
    r = np.ascontiguousarray(rays, SCENE_RAY_DTYPE).reshape(-1); n = r.shape[0]
    return r, (np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.float32),
               np.empty(n, np.float32), np.empty(n, np.int32))


def cast_scene(objects, rays, hit_opacity=0.5, side=0):
    """mon_scene_cast: the object map along world rays (SCENE_RAY_DTYPE: o, t_max, d unit, key).  Returns (rgb (n, 3), dist, opacity, instance, hit_t,
    hit_sample_t, hit_instance): hit_t is the point at which 1 - T crosses hit_opacity, placed inside its sample's interval."""
    r, out = _cast_args(rays)
    _check(lib().mon_scene_cast(_handles(objects), len(objects), int(side), _p(r), r.shape[0], float(hit_opacity), *[_p(a) for a in out]))
    return out


def scene_cast_rays(objects, rays, k, side=0):
    """mon_debug_scene_cast_rays: object k's ray rows of that cast, (n, 10) = o[3], d[3], lo, hi, flag, dn = 1, and its entry row (n,)."""
    r, _ = _cast_args(rays); rows = np.empty((r.shape[0], 10), np.float32); entry = np.empty(r.shape[0], np.float32)
    _check(diag_lib().mon_debug_scene_cast_rays(_handles(objects), len(objects), int(side), _p(r), r.shape[0], int(k), _p(rows), _p(entry)))
    return rows, entry


def scene_cast_composite(t, alpha, rgb, count, entry, hit_opacity=0.5, device=0):
    """mon_debug_scene_cast_composite: the cast's composite kernel on lists laid out as scene_composite's, entry (n_lists, n_rays) = each list's box entry.
    Returns (rgb (n_rays, 3), dist, opacity, instance, hit_t, hit_sample_t, hit_instance)."""
    t = np.ascontiguousarray(t, np.float32); L, R = t.shape[:2]
    a = np.ascontiguousarray(alpha, np.float32).reshape(L, R, 64); c = np.ascontiguousarray(rgb, np.float32).reshape(L, R, 64, 3)
    n = np.ascontiguousarray(count, np.uint32).reshape(L, R); e = np.ascontiguousarray(entry, np.float32).reshape(L, R)
    out = (np.empty((R, 3), np.float32), np.empty(R, np.float32), np.empty(R, np.float32), np.empty(R, np.int32), np.empty(R, np.float32),
           np.empty(R, np.float32), np.empty(R, np.int32))
    _check(diag_lib().mon_debug_scene_cast_composite(int(device), R, L, _p(t), _p(a), _p(c), _p(n), _p(e), float(hit_opacity), *[_p(o) for o in out]))
    return out


def _point_outputs(n):
    return (np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.uint32))


def _lattice_args(origin, step, shape):
    o = np.ascontiguousarray(origin, np.float32).reshape(3); s = np.ascontiguousarray(step, np.float32).reshape(3)
    nx, ny, nz = (int(v) for v in shape)
    return o, s, nx, ny, nz


def query_object_points(obj, unit_xyz, side=0):
    """mon_object_query_points: the object's raw network outputs (n, 4) at points of its unit cube (the coordinates its encoder takes)."""
    x = np.ascontiguousarray(unit_xyz, np.float32).reshape(-1, 3); raw = np.empty((x.shape[0], 4), np.float32)
    _check(lib().mon_object_query_points(obj.h, int(side), _p(x), x.shape[0], _p(raw)))
    return raw


def query_scene_points(objects, world_xyz, side=0):
    """mon_scene_query_points: the object map at world points (n, 3).  Returns (sigma, rgb (n, 3), owner: index into objects or -1, owner_sigma, n_inside)."""
    x = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3); out = _point_outputs(x.shape[0])
    _check(lib().mon_scene_query_points(_handles(objects), len(objects), int(side), _p(x), x.shape[0], *[_p(a) for a in out]))
    return out


def query_scene_lattice(objects, origin, step, shape, side=0):
    """mon_scene_query_lattice: query_scene_points at the lattice origin + (i, j, k) * step, shape = (nx, ny, nz), i fastest, formed on the device."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _point_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0))
    _check(lib().mon_scene_query_lattice(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, *[_p(a) for a in out]))
    return out


def lattice_points(origin, step, shape):
    """mon_lattice_points (host only): the lattice's points (nx * ny * nz, 3) exactly as the device forms them."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); xyz = np.empty((max(nx, 0) * max(ny, 0) * max(nz, 0), 3), np.float32)
    _check(lib().mon_lattice_points(_p(o), _p(s), nx, ny, nz, _p(xyz)))
    return xyz


def _distance_outputs(n, free):
    return (np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32) if free else None, np.empty(n, np.float32))


def distance_transform(occupied, step, max_dist=np.inf, device=0, nearest=True):
    """mon_distance_transform: the exact Euclidean distance transform of a mask of shape (nz, ny, nx) (x fastest; a cell counts iff it is not 0) with
    spacing step = (sx, sy, sz).  Returns (dist, nearest), both of the mask's shape: the distance to the nearest occupied cell, truncated by max_dist,
    and that cell's flat index (-1: none); nearest=False passes NULL and returns (dist, None)."""
    m = np.ascontiguousarray(occupied); assert m.ndim == 3, "mask of shape (nz, ny, nx)"
    m = np.ascontiguousarray(m != 0, np.uint8); nz, ny, nx = m.shape
    s = np.ascontiguousarray(step, np.float32).reshape(3)
    dist = np.empty(m.shape, np.float32); near = np.empty(m.shape, np.int32) if nearest else None
    _check(lib().mon_distance_transform(int(device), _p(m), nx, ny, nz, _p(s), float(max_dist), _p(dist), _p(near)))
    return dist, near


def scene_distance_lattice(objects, origin, step, shape, sigma_min, max_dist=np.inf, side=0, free=True):
    """mon_scene_distance_lattice: the object map's distance field over the lattice of query_scene_lattice, a cell occupied iff not (sigma <= sigma_min).
    Returns (dist, nearest, nearest_owner, free_dist (None with free=False), sigma), each of nx * ny * nz elements."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _distance_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0), free)
    _check(lib().mon_scene_distance_lattice(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, float(sigma_min), float(max_dist),
                                            *[_p(a) for a in out]))
    return out


MON_SIGNED_LOG = 1


def _signed_outputs(n):
    return (np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32), np.empty(n, np.float32), np.empty(1, np.float32))


def signed_distance_transform(val, iso, step, max_dist=np.inf, device=0, nearest=True):
    """mon_signed_distance_transform: the signed, sub-cell distance transform of values of shape (nz, ny, nx) (x fastest) with spacing step = (sx, sy, sz):
    a cell is inside iff not (val <= iso), the surface crosses the lattice edges between cells of different sides at the linearly interpolated place.
    Returns (sdist, nearest_edge), both of val's shape: the distance to the nearest crossing, negative inside, truncated by max_dist, and that edge as
    3 * flat(lower cell) + axis (-1: none); nearest=False passes NULL and returns (sdist, None)."""
    v = np.ascontiguousarray(val, np.float32); assert v.ndim == 3, "values of shape (nz, ny, nx)"
    nz, ny, nx = v.shape; s = np.ascontiguousarray(step, np.float32).reshape(3)
    sdist = np.empty(v.shape, np.float32); near = np.empty(v.shape, np.int32) if nearest else None
    _check(lib().mon_signed_distance_transform(int(device), _p(v), float(iso), nx, ny, nz, _p(s), float(max_dist), _p(sdist), _p(near)))
    return sdist, near


def scene_signed_distance_lattice(objects, origin, step, shape, sigma_min, max_dist=np.inf, side=0, log=True):
    """mon_scene_signed_distance_lattice: the object map's signed, sub-cell distance field over the lattice of query_scene_lattice: inside iff
    not (sigma <= sigma_min); log: the crossings are placed in log density (MON_SIGNED_LOG), else in density.
    Returns (sdist, nearest_edge, nearest_owner, sigma, val, iso): five arrays of nx * ny * nz elements and the level the device formed."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _signed_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0))
    _check(lib().mon_scene_signed_distance_lattice(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, float(sigma_min),
                                                   MON_SIGNED_LOG if log else 0, float(max_dist), *[_p(a) for a in out]))
    return out[:5] + (float(out[5][0]),)


def edge_points(nearest_edge, val, iso, origin, step):
    """Host helper: the world point of each cell's nearest crossing, (.., 3) float64, NaN where nearest_edge is -1.  val: the values of shape
    (nz, ny, nx) the field was made from (scene_signed_distance_lattice's val), iso its level; the fraction along the edge is the header's f in fp32."""
    v = np.ascontiguousarray(val, np.float32); nz, ny, nx = v.shape; flat = v.reshape(-1)
    e = np.asarray(nearest_edge, np.int64); ok = e >= 0; ee = np.where(ok, e, 0)
    a = ee % 3; q = ee // 3; other = np.minimum(q + np.asarray([1, nx, nx * ny])[a], flat.size - 1)
    v0 = flat[q]; v1 = flat[other]
    with np.errstate(all="ignore"):
        f = (np.float32(iso) - v0) / (v1 - v0)
    f = np.where((f >= 0) & (f <= 1), f, np.float32(0.5)).astype(np.float64)
    ijk = np.stack([q % nx, (q // nx) % ny, q // (nx * ny)], -1).astype(np.float64) + f[..., None] * np.eye(3)[a]
    pts = np.asarray(origin, np.float64) + ijk * np.asarray(step, np.float64)
    pts[~ok] = np.nan
    return pts


def scene_signed_dist_field(objects, origin, step, shape, sigma_min, max_dist, side=0, log=True):
    """mon_scene_signed_dist_field: scene_signed_distance_lattice's sdist for the same arguments, kept on the device -> DistField (defined below)"""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); h = C.c_void_p()
    _check(lib().mon_scene_signed_dist_field(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, float(sigma_min),
                                             MON_SIGNED_LOG if log else 0, float(max_dist), C.byref(h)))
    return DistField(h)


class DistField:
    """A mon_dist_field: a snapshot of a distance field in device memory (include/mon_core.h).  Made by dist_field_create, scene_dist_field or
    OnlineManager.dist_field; it outlives the objects and the manager it came from.  close() (or the garbage collector) frees it."""

    def __init__(self, handle):
        self.h = handle

    def close(self):
        if self.h is not None and self.h.value:
            _check(lib().mon_dist_field_destroy(self.h))
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """mon_dist_field_info -> DistFieldDesc (nx, ny, nz, device, origin, step, max_value)"""
        d = DistFieldDesc(); _check(lib().mon_dist_field_info(self.h, C.byref(d))); return d

    def read(self):
        """mon_dist_field_read: the cells, of shape (nz, ny, nx)"""
        d = self.info(); out = np.empty((d.nz, d.ny, d.nx), np.float32)
        _check(lib().mon_dist_field_read(self.h, _p(out))); return out

    def sample(self, xyz, outside=0.0, grad=True):
        """mon_dist_field_sample at world points (n, 3) -> (dist (n,), grad (n, 3), or None with grad=False)"""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3); n = x.shape[0]
        dist = np.empty(n, np.float32); g = np.empty((n, 3), np.float32) if grad else None
        _check(lib().mon_dist_field_sample(self.h, _p(x), n, float(outside), _p(dist), _p(g)))
        return dist, g

    def score(self, spheres, ways, n_sub=1, outside=0.0, margin=0.0, safe=0.0, outputs=("first_hit", "cost", "way_clear", "way_grad")):
        """mon_dist_field_score.  spheres (n_spheres, 4) = (bx, by, bz, r); ways (n_traj, n_way, 3) positions or (n_traj, n_way, 16) / (n_traj, n_way, 4, 4)
        row-major matrices.  -> a dict with min_clear (n_traj,) and those of first_hit (n_traj,) int32, cost (n_traj,), way_clear (n_traj, n_way) and way_grad
        (n_traj, n_way, 3) that `outputs` names (the others are passed as NULL)."""
        assert set(outputs) <= {"first_hit", "cost", "way_clear", "way_grad"}, outputs
        b = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        w = np.ascontiguousarray(ways, np.float32); assert w.ndim in (3, 4), "ways of shape (n_traj, n_way, 3 | 16) or (n_traj, n_way, 4, 4)"
        n_traj, n_way = w.shape[:2]; w = w.reshape(n_traj, n_way, -1); wf = w.shape[2]
        prm = TrajScoreParams(float(outside), float(margin), float(safe))
        out = {"min_clear": np.empty(n_traj, np.float32),
               "first_hit": np.empty(n_traj, np.int32) if "first_hit" in outputs else None,
               "cost": np.empty(n_traj, np.float32) if "cost" in outputs else None,
               "way_clear": np.empty((n_traj, n_way), np.float32) if "way_clear" in outputs else None,
               "way_grad": np.empty((n_traj, n_way, 3), np.float32) if "way_grad" in outputs else None}
        _check(lib().mon_dist_field_score(self.h, _p(b), b.shape[0], _p(w), wf, n_traj, n_way, int(n_sub), C.byref(prm), _p(out["min_clear"]),
                                          _p(out["first_hit"]), _p(out["cost"]), _p(out["way_clear"]), _p(out["way_grad"])))
        return {k: v for k, v in out.items() if v is not None}

    def match(self, points, poses, pivots=None, huber=np.inf, outside=0.0, normal=True, counts=True):
        """mon_dist_field_match.  points (n, 3) in the body frame; poses (H, 16) or (H, 4, 4) row-major; pivots (H, 3) or None for the origin.  -> a dict
        with cost (H,) and, with counts, n_inside and n_inlier (H,) int32, and, with normal, A (H, 21) (row-major upper triangle) and b (H, 6)."""
        x = np.ascontiguousarray(points, np.float32).reshape(-1, 3); T = np.ascontiguousarray(poses, np.float32).reshape(-1, 16); H = T.shape[0]
        c = None if pivots is None else np.ascontiguousarray(pivots, np.float32).reshape(H, 3)
        prm = ScanMatchParams(float(huber), float(outside))
        cost = np.empty(H, np.float32); ni = np.empty(H, np.int32) if counts else None; nl = np.empty(H, np.int32) if counts else None
        nrm = np.empty((H, 27), np.float32) if normal else None
        _check(lib().mon_dist_field_match(self.h, _p(x), x.shape[0], _p(T), H, _p(c), C.byref(prm), _p(cost), _p(ni), _p(nl), _p(nrm)))
        out = {"cost": cost}
        if counts:
            out["n_inside"] = ni; out["n_inlier"] = nl
        if normal:
            out["A"] = nrm[:, :21].copy(); out["b"] = nrm[:, 21:].copy()
        return out

    def register_default(self):
        """mon_register_default -> RegisterParams for this field"""
        p = RegisterParams(); _check(lib().mon_register_default(self.h, C.byref(p))); return p

    def register(self, points, poses, params=None, **overrides):
        """mon_dist_field_register: every hypothesis of poses (H, 16) or (H, 4, 4) refined by Levenberg-Marquardt.  params: RegisterParams (default:
        register_default()), with `overrides` set on a copy.  -> a dict with poses (H, 4, 4), cost, n_inside, n_inlier, evals, status (H,) and best."""
        x = np.ascontiguousarray(points, np.float32).reshape(-1, 3); T = np.ascontiguousarray(poses, np.float32).reshape(-1, 16); H = T.shape[0]
        base = params if params is not None else self.register_default()
        prm = RegisterParams.from_buffer_copy(base)
        for k, v in overrides.items():
            assert k in dict(RegisterParams._fields_), k
            setattr(prm, k, v)
        out = {"poses": np.empty((H, 4, 4), np.float32), "cost": np.empty(H, np.float32), "n_inside": np.empty(H, np.int32), "n_inlier": np.empty(H, np.int32),
               "evals": np.empty(H, np.int32), "status": np.empty(H, np.int32)}
        best = C.c_int32(-2)
        _check(lib().mon_dist_field_register(self.h, _p(x), x.shape[0], _p(T), H, C.byref(prm), _p(out["poses"]), _p(out["cost"]), _p(out["n_inside"]),
                                             _p(out["n_inlier"]), _p(out["evals"]), _p(out["status"]), C.byref(best)))
        out["best"] = int(best.value)
        return out

    def trace_default(self):
        """mon_trace_default -> TraceParams for this field"""
        p = TraceParams(); _check(lib().mon_trace_default(self.h, C.byref(p))); return p

    def _trace_args(self, rays, poses, params):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        T = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        prm = TraceParams.from_buffer_copy(params if params is not None else self.trace_default())
        return r, T, (1 if T is None else T.shape[0]), prm

    def trace(self, rays, poses=None, params=None, normals=False, status=True, steps=True):
        """mon_dist_field_trace.  rays (n, 6) = origin and unit direction in the sensor frame; poses (H, 16) or (H, 4, 4) row-major, or None for world rays.
        params: TraceParams (default: trace_default()).  -> a dict with range (H, n) and, unless turned off, status and steps (H, n) int32 (status 0: hit,
        1: passed t_max, 2: out of steps, 3: left the lattice), and with normals normal (H, n, 3)."""
        r, T, H, prm = self._trace_args(rays, poses, params); n = r.shape[0]
        out = {"range": np.empty((H, n), np.float32), "status": np.empty((H, n), np.int32) if status else None,
               "steps": np.empty((H, n), np.int32) if steps else None, "normal": np.empty((H, n, 3), np.float32) if normals else None}
        _check(lib().mon_dist_field_trace(self.h, _p(r), n, _p(T), H, C.byref(prm), _p(out["range"]), _p(out["status"]), _p(out["steps"]), _p(out["normal"])))
        return {k: v for k, v in out.items() if v is not None}

    def beam_score(self, rays, measured, poses, params=None, huber=np.inf):
        """mon_dist_field_beam_score.  measured (n,): the measured range of every beam, NaN for a beam without a return; rays, poses and params as trace
        takes them.  -> a dict with cost (H,), the Huber cost of range - measured over the valid beams, and n_valid and n_hit (H,) int32."""
        r, T, H, prm = self._trace_args(rays, poses, params); n = r.shape[0]
        z = np.ascontiguousarray(measured, np.float32).reshape(-1); assert z.shape[0] == n, "one measured range per ray"
        b = BeamParams(float(huber))
        out = {"cost": np.empty(H, np.float32), "n_valid": np.empty(H, np.int32), "n_hit": np.empty(H, np.int32)}
        _check(lib().mon_dist_field_beam_score(self.h, _p(r), n, _p(z), _p(T), H, C.byref(prm), C.byref(b), _p(out["cost"]), _p(out["n_valid"]),
                                               _p(out["n_hit"])))
        return out

    def line_of_sight(self, a, b, params=None):
        """Is the segment from a to b free?  a, b (3,) or (m, 3) world points.  A host-side helper over trace: the unit direction and t_max = |b - a| are
        formed in float64 and rounded; one call per pair, since t_max is the call's.  -> bool, or (m,) bool: the ray passed t_max (status 1)."""
        a64 = np.asarray(a, np.float64).reshape(-1, 3); b64 = np.asarray(b, np.float64).reshape(-1, 3); assert a64.shape == b64.shape
        prm = TraceParams.from_buffer_copy(params if params is not None else self.trace_default())
        free = np.zeros(a64.shape[0], bool); t_min = prm.t_min
        for m in range(a64.shape[0]):
            v = b64[m] - a64[m]; length = float(np.linalg.norm(v))
            u = v / length if length > 0.0 else np.zeros(3)
            prm.t_max = length; prm.t_min = min(t_min, prm.t_max)
            got = self.trace(np.concatenate([a64[m], u]).astype(np.float32), None, prm, steps=False)
            free[m] = got["status"][0, 0] == 1
        return bool(free[0]) if np.ndim(a) == 1 else free


def dist_field_create(dist, origin, step, device=0):
    """mon_dist_field_create: a host field of shape (nz, ny, nx) (x fastest), cell (i, j, k) at origin + (i, j, k) * step, uploaded to `device` -> DistField"""
    d = np.ascontiguousarray(dist, np.float32); assert d.ndim == 3, "field of shape (nz, ny, nx)"
    nz, ny, nx = d.shape; o, s, _, _, _ = _lattice_args(origin, step, (nx, ny, nz)); h = C.c_void_p()
    _check(lib().mon_dist_field_create(int(device), _p(d), nx, ny, nz, _p(o), _p(s), C.byref(h)))
    return DistField(h)


def scene_dist_field(objects, origin, step, shape, sigma_min, max_dist, side=0):
    """mon_scene_dist_field: scene_distance_lattice's dist for the same arguments, kept on the device (nothing per cell comes home) -> DistField"""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); h = C.c_void_p()
    _check(lib().mon_scene_dist_field(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, float(sigma_min), float(max_dist), C.byref(h)))
    return DistField(h)


def _components_call(call, n, cap, rows):
    """call(label, comp, table, cap, n_components, dist, sigma, owner) with fresh arrays of n cells; cap None: room for every component (n records);
    rows: which of "dist", "sigma", "owner" to bring home.  -> (label, comp, table cut to the records written, n_components, {row: array})"""
    assert set(rows) <= {"dist", "sigma", "owner"}, rows
    cap = n if cap is None else int(cap)
    label = np.empty(n, np.int32); comp = np.empty(n, np.int32); table = np.empty(min(cap, n), LATTICE_COMPONENT_DTYPE); nc = C.c_uint32(0)
    opt = {k: np.empty(n, np.int32 if k == "owner" else np.float32) for k in rows}
    _check(call(_p(label), _p(comp), _p(table), cap, C.byref(nc), *[_p(opt.get(k)) for k in ("dist", "sigma", "owner")]))
    return label, comp, table[:min(nc.value, cap)], nc.value, opt


def label_components(mask, connectivity=6, device=0, cap=None):
    """mon_label_components: the connected components of a mask of shape (nz, ny, nx) (x fastest; a cell counts iff it is not 0) under 6-, 18- or
    26-connectivity.  Returns (label, comp, table, n_components): label and comp of the mask's shape (the lowest flat index of the cell's component and
    the component's rank by ascending representative; -1 outside the mask), table a structured array (LATTICE_COMPONENT_DTYPE: rep, cells, lo, hi) of
    the first min(n_components, cap) components (cap None: all of them), n_components the total."""
    m = np.ascontiguousarray(mask); assert m.ndim == 3, "mask of shape (nz, ny, nx)"
    m = np.ascontiguousarray(m != 0, np.uint8); nz, ny, nx = m.shape
    label, comp, table, nc, _ = _components_call(
        lambda lab, cmp_, tab, cap_, n_, *_: lib().mon_label_components(int(device), _p(m), nx, ny, nz, int(connectivity), lab, cmp_, tab, cap_, n_),
        m.size, cap, ())
    return label.reshape(m.shape), comp.reshape(m.shape), table, nc


def scene_components_lattice(objects, origin, step, shape, sigma_min, region=0, clearance=0.0, connectivity=6, side=0, cap=None, rows=()):
    """mon_scene_components_lattice: the object map's connected components over the lattice of query_scene_lattice.  region 0: the occupied cells,
    not (sigma <= sigma_min) -- the map's blobs; region 1: the cells a sphere of radius `clearance` may occupy, scene_distance_lattice's dist > clearance.
    Returns (label, comp, table, n_components, rows), the first two of nx * ny * nz elements, as label_components'; rows = {name: array} for the names
    asked for among "dist" (region 1 only), "sigma" and "owner"."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape)
    return _components_call(lambda *a: lib().mon_scene_components_lattice(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz,
                                                                          float(sigma_min), int(region), float(clearance), int(connectivity), *a),
                            max(nx, 0) * max(ny, 0) * max(nz, 0), cap, rows)


def _paths_call(call, n, seeds, rows):
    """call(seeds, n_seeds, cost, next, dist, sigma, owner) with fresh arrays of n cells; rows: which of "dist", "sigma", "owner" to bring home.
    -> (cost, next, {row: array})"""
    assert set(rows) <= {"dist", "sigma", "owner"}, rows
    sd = np.ascontiguousarray(seeds, np.int32).reshape(-1)
    cost = np.empty(n, np.float32); nxt = np.empty(n, np.int32)
    opt = {k: np.empty(n, np.int32 if k == "owner" else np.float32) for k in rows}
    _check(call(_p(sd), sd.size, _p(cost), _p(nxt), *[_p(opt.get(k)) for k in ("dist", "sigma", "owner")]))
    return cost, nxt, opt


def shortest_paths(mask, seeds, step, connectivity=26, cell_cost=None, max_cost=np.inf, device=0):
    """mon_shortest_paths: the shortest-path cost field of a mask of shape (nz, ny, nx) (x fastest; a cell is passable iff it is not 0) from the seeds (flat
    indices) with spacing step = (sx, sy, sz) under 6-, 18- or 26-connectivity; cell_cost: a per-cell multiplier of the mask's shape (None: 1).  Returns
    (cost, next), both of the mask's shape: the least fp32 fold of the move weights over all walks from a seed (+inf: unreachable, outside the mask or
    above max_cost) and the flat index of the neighbour to step to (-1: a seed, no way, or no strictly cheaper neighbour that explains the cost)."""
    m = np.ascontiguousarray(mask); assert m.ndim == 3, "mask of shape (nz, ny, nx)"
    m = np.ascontiguousarray(m != 0, np.uint8); nz, ny, nx = m.shape
    s = np.ascontiguousarray(step, np.float32).reshape(3)
    c = None if cell_cost is None else np.ascontiguousarray(cell_cost, np.float32)
    assert c is None or c.size == m.size, "cell_cost of the mask's shape"
    cost, nxt, _ = _paths_call(lambda sd, ns, co, nx_, *_: lib().mon_shortest_paths(int(device), _p(m), nx, ny, nz, _p(s), int(connectivity), _p(c), sd, ns,
                                                                                     float(max_cost), co, nx_), m.size, seeds, ())
    return cost.reshape(m.shape), nxt.reshape(m.shape)


def scene_paths_lattice(objects, origin, step, shape, sigma_min, seeds, clearance=0.0, soft_radius=0.0, soft_weight=0.0, connectivity=26, max_cost=np.inf,
                        side=0, rows=()):
    """mon_scene_paths_lattice: the object map's shortest-path cost field over the lattice of query_scene_lattice: passable where scene_distance_lattice's
    dist > clearance, a move dearer by up to 1 + soft_weight within soft_radius of matter.  Returns (cost, next, rows), the first two of nx * ny * nz
    elements, as shortest_paths'; rows = {name: array} for the names asked for among "dist", "sigma" and "owner"."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape)
    return _paths_call(lambda sd, ns, *a: lib().mon_scene_paths_lattice(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, float(sigma_min),
                                                                        float(clearance), float(soft_radius), float(soft_weight), int(connectivity), sd, ns,
                                                                        float(max_cost), *a),
                       max(nx, 0) * max(ny, 0) * max(nz, 0), seeds, rows)


def lattice_path(next, start):
    """mon_lattice_path: the flat indices from start along next (as shortest_paths returns it) to the first -1, start included."""
    nx_ = np.ascontiguousarray(next, np.int32).reshape(-1); n = C.c_size_t(0)
    _check(lib().mon_lattice_path(_p(nx_), nx_.size, int(start), None, 0, C.byref(n)))
    path = np.empty(n.value, np.int32)
    _check(lib().mon_lattice_path(_p(nx_), nx_.size, int(start), _p(path), path.size, C.byref(n)))
    return path


def paths_stats():
    """mon_debug_paths_stats: (sweeps enqueued, batches, sweeps that left work) of the process's latest shortest-path field."""
    out = np.zeros(3, np.uint32)
    _check(diag_lib().mon_debug_paths_stats(_p(out)))
    return tuple(int(v) for v in out)


def scene_point_rows(objects, world_xyz, k, side=0):
    """mon_debug_scene_point_rows: object k's row of every point of that query, (n, 12) = u[3], inside, raw4, sigma_k, r, g, b."""
    x = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3); rows = np.empty((x.shape[0], 12), np.float32)
    _check(diag_lib().mon_debug_scene_point_rows(_handles(objects), len(objects), int(side), _p(x), x.shape[0], int(k), _p(rows)))
    return rows


def _gradient_outputs(n):
    return _point_outputs(n) + (np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32))


def _weights_arg(level_weights):
    return None if level_weights is None else np.ascontiguousarray(level_weights, np.float32).reshape(-1)


def _select_arg(select, n):
    if select is None:
        return None
    s = np.ascontiguousarray(select, np.int32).reshape(-1)
    if s.shape[0] != n:
        raise ValueError("select holds %d values for %d points" % (s.shape[0], n))
    return s


def query_object_gradients(obj, unit_xyz, level_weights=None, side=0):
    """mon_object_query_gradients: (raw (n, 4), grad_unit (n, 3) = d raw3 / d u) at points of the object's unit cube; level_weights: n_levels floats."""
    x = np.ascontiguousarray(unit_xyz, np.float32).reshape(-1, 3); w = _weights_arg(level_weights)
    raw = np.empty((x.shape[0], 4), np.float32); g = np.empty((x.shape[0], 3), np.float32)
    _check(lib().mon_object_query_gradients(obj.h, int(side), _p(x), x.shape[0], _p(w), _p(raw), _p(g)))
    return raw, g


def query_scene_gradients(objects, world_xyz, level_weights=None, select=None, side=0):
    """mon_scene_query_gradients: query_scene_points' five outputs, then grad_log (n, 3) = the world gradient of the owner's (the selected object's) log
    density, grad_sigma (n, 3) = the world gradient of sigma, normal (n, 3) = -grad_log / |grad_log|.  level_weights: Lmax floats (None: all 1; a coarse
    window for normals); select: per point -1 (the owner rule) or the index of the object to report."""
    x = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3); out = _gradient_outputs(x.shape[0])
    w = _weights_arg(level_weights); s = _select_arg(select, x.shape[0])
    _check(lib().mon_scene_query_gradients(_handles(objects), len(objects), int(side), _p(x), x.shape[0], _p(w), _p(s), *[_p(a) for a in out]))
    return out


def query_scene_lattice_gradients(objects, origin, step, shape, level_weights=None, side=0):
    """mon_scene_query_lattice_gradients: query_scene_gradients (no select) over the lattice of query_scene_lattice, formed on the device."""
    o, s, nx, ny, nz = _lattice_args(origin, step, shape); out = _gradient_outputs(max(nx, 0) * max(ny, 0) * max(nz, 0)); w = _weights_arg(level_weights)
    _check(lib().mon_scene_query_lattice_gradients(_handles(objects), len(objects), int(side), _p(o), _p(s), nx, ny, nz, _p(w), *[_p(a) for a in out]))
    return out


def _normal_outputs(n):
    return (np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32))


def cast_scene_normals(objects, rays, hit_opacity=0.5, level_weights=None, side=0):
    """mon_scene_cast_normals: cast_scene's seven outputs, then hit_xyz (n, 3), normal (n, 3) and grad_log (n, 3) of the hit object at the hit point
    (0 0 0 for a miss)."""
    r, out = _cast_args(rays); out = out + _normal_outputs(r.shape[0]); w = _weights_arg(level_weights)
    _check(lib().mon_scene_cast_normals(_handles(objects), len(objects), int(side), _p(r), r.shape[0], float(hit_opacity), _p(w), *[_p(a) for a in out]))
    return out


def scene_gradient_rows(objects, world_xyz, k, level_weights=None, side=0):
    """mon_debug_scene_gradient_rows: object k's row of every point of that query, (n, 16) = scene_point_rows' twelve floats, g_k[3], 0."""
    x = np.ascontiguousarray(world_xyz, np.float32).reshape(-1, 3); rows = np.empty((x.shape[0], 16), np.float32); w = _weights_arg(level_weights)
    _check(diag_lib().mon_debug_scene_gradient_rows(_handles(objects), len(objects), int(side), _p(x), x.shape[0], _p(w), int(k), _p(rows)))
    return rows


def scene_samples(objects, rect, Twc16, k, side=0):
    """mon_debug_scene_samples: object k's sample lists of that scene render, per pixel: t (h, w, 64), alpha (h, w, 64), rgb (h, w, 64, 3), count (h, w)."""
    FrameId, x, y, h, w = (int(v) for v in rect); pose = np.ascontiguousarray(Twc16, np.float32)
    t = np.empty((h, w, 64), np.float32); a = np.empty_like(t); c = np.empty((h, w, 64, 3), np.float32); n = np.empty((h, w), np.uint32)
    _check(diag_lib().mon_debug_scene_samples(_handles(objects), len(objects), int(side), MonBBox(FrameId, x, y, h, w), _p(pose), int(k), _p(t), _p(a),
                                              _p(c), _p(n)))
    return t, a, c, n


def scene_composite(t, alpha, rgb, count, dn, device=0):
    """mon_debug_scene_composite: the merge-composite kernel on lists t / alpha (n_lists, n_rays, 64), rgb (n_lists, n_rays, 64, 3), count (n_lists,
    n_rays), dn (n_rays,).  Returns (rgb (n_rays, 3), depth, opacity, instance)."""
    t = np.ascontiguousarray(t, np.float32); L, R = t.shape[:2]
    a = np.ascontiguousarray(alpha, np.float32).reshape(L, R, 64); c = np.ascontiguousarray(rgb, np.float32).reshape(L, R, 64, 3)
    n = np.ascontiguousarray(count, np.uint32).reshape(L, R); d = np.ascontiguousarray(dn, np.float32).reshape(R)
    o_rgb = np.empty((R, 3), np.float32); o_d = np.empty(R, np.float32); o_o = np.empty(R, np.float32); o_i = np.empty(R, np.int32)
    _check(diag_lib().mon_debug_scene_composite(int(device), R, L, _p(t), _p(a), _p(c), _p(n), _p(d), _p(o_rgb), _p(o_d), _p(o_o), _p(o_i)))
    return o_rgb, o_d, o_o, o_i


def _scene_level_weights(objects, level_weights):
    if level_weights is None:
        return None
    w = np.ascontiguousarray(level_weights, np.float32).reshape(-1)
    if w.size != max(o.cfg.n_levels for o in objects):
        raise ValueError("level_weights: one weight per level of the finest object")
    return w


def scene_pose_loss(objects, obs, Twc16, params=None, side=0, iteration=0, level_weights=None):
    """mon_scene_pose_loss: (loss, grad6 = dL/d(rho, phi) of Twc exp(xi^)) of the camera pose Twc16 (column-major) against the boxes obs [(FrameId, x, y, h, w)]
    of one frame, through all the objects composited in depth order.  level_weights: None, or one weight per level of the finest object."""
    b, prm = _pose_boxes(obs), _pose_params(params); pose = np.ascontiguousarray(Twc16, np.float32).reshape(16)
    w = _scene_level_weights(objects, level_weights); loss = C.c_float(0); g = np.empty(6, np.float32)
    _check(lib().mon_scene_pose_loss(_handles(objects), len(objects), int(side), _p(b), b.shape[0], _p(pose), C.byref(prm), int(iteration), _p(w),
                                     C.byref(loss), _p(g)))
    return loss.value, g


def scene_refine_camera(objects, obs, Twc16, params=None, c2f=None, side=0):
    """mon_scene_refine_camera: params.iters Adam steps on the camera pose from Twc16.  c2f: None = plain, True = the default coarse-to-fine schedule, or
    PoseC2FParams / a dict of overrides.  Returns (refined Twc16, loss trace of iters + 1 values); nothing about the objects changes."""
    b, prm = _pose_boxes(obs), _pose_params(params); pose = np.array(Twc16, np.float32).reshape(16)
    c = None if c2f is None else _c2f_params(None if c2f is True else c2f)
    trace = np.empty(prm.iters + 1, np.float32)
    _check(lib().mon_scene_refine_camera(_handles(objects), len(objects), int(side), _p(b), b.shape[0], C.byref(prm), None if c is None else C.byref(c),
                                         _p(pose), _p(trace)))
    return pose, trace


def window_default(**overrides):
    """mon_window_default, then any field overridden by keyword."""
    w = WindowParams(); _check(lib().mon_window_default(C.byref(w)))
    for k, v in overrides.items():
        if k not in dict(WindowParams._fields_):
            raise KeyError(k)
        setattr(w, k, v)
    return w


def _window_params(window):
    if isinstance(window, WindowParams):
        return window
    return window_default(**(window or {}))


def window_frames(obs):
    """mon_window_frames (host only): the distinct FrameIds of obs [(FrameId, x, y, h, w)] in order of first appearance (uint32)."""
    b = _pose_boxes(obs); ids = np.zeros(32, np.uint32); n = C.c_size_t(0)
    _check(lib().mon_window_frames(_p(b), b.shape[0], _p(ids), C.byref(n)))
    return ids[:n.value].copy()


def scene_window_loss(objects, obs, Twc16s, Tow16s=None, params=None, side=0, iteration=0, level_weights=None):
    """mon_scene_window_loss: one evaluation of a window -- obs names F frames (each frame's boxes contiguous), Twc16s (F, 16) in window order, Tow16s (K, 16)
    or None = every object's own Tow.  Returns (L = sum of the frame losses, frame_loss (F,), cam_grad6 (F, 6), obj_grad6 (K, 6))."""
    b, prm = _pose_boxes(obs), _pose_params(params); F = len(window_frames(b)); K = len(objects)
    Twc = np.ascontiguousarray(Twc16s, np.float32).reshape(F, 16)
    Tow = None if Tow16s is None else np.ascontiguousarray(Tow16s, np.float32).reshape(K, 16)
    w = _scene_level_weights(objects, level_weights); loss = C.c_float(0)
    fl = np.empty(F, np.float32); cg = np.empty((F, 6), np.float32); og = np.empty((K, 6), np.float32)
    _check(lib().mon_scene_window_loss(_handles(objects), K, int(side), _p(b), b.shape[0], _p(Twc), _p(Tow), C.byref(prm), int(iteration), _p(w),
                                       C.byref(loss), _p(fl), _p(cg), _p(og)))
    return loss.value, fl, cg, og


def scene_refine_window(objects, obs, Twc16s, Tow16s=None, params=None, c2f=None, window=None, side=0):
    """mon_scene_refine_window: params.iters joint Adam steps on the window's free cameras and (window.refine_objects) the objects.  window: WindowParams, a
    dict of overrides of mon_window_default, or None.  Tow16s None = every object's own Tow (only with refine_objects = 0).  Returns (Twc16s (F, 16),
    Tow16s (K, 16) or None, loss trace (iters + 1,), frame trace (iters + 1, F)); nothing about the objects changes."""
    b, prm, wp = _pose_boxes(obs), _pose_params(params), _window_params(window); F = len(window_frames(b)); K = len(objects)
    Twc = np.array(Twc16s, np.float32).reshape(F, 16)
    Tow = None if Tow16s is None else np.array(Tow16s, np.float32).reshape(K, 16)
    c = None if c2f is None else _c2f_params(None if c2f is True else c2f)
    trace = np.empty(prm.iters + 1, np.float32); ftrace = np.empty((prm.iters + 1, F), np.float32)
    _check(lib().mon_scene_refine_window(_handles(objects), K, int(side), _p(b), b.shape[0], C.byref(prm), None if c is None else C.byref(c), C.byref(wp),
                                         _p(Twc), _p(Tow), _p(trace), _p(ftrace)))
    return Twc, Tow, trace, ftrace


def scene_pose_loss_batch(objects, obs, Twc16s, params=None, side=0, iteration=0):
    """mon_scene_pose_loss_batch: the scene_pose_loss of every pose of Twc16s (n, 16), bit for bit, in one enqueue.  Returns the n losses (float32)."""
    b, prm = _pose_boxes(obs), _pose_params(params); poses = np.ascontiguousarray(Twc16s, np.float32).reshape(-1, 16)
    losses = np.empty(poses.shape[0], np.float32)
    _check(lib().mon_scene_pose_loss_batch(_handles(objects), len(objects), int(side), _p(b), b.shape[0], _p(poses), poses.shape[0], C.byref(prm),
                                           int(iteration), _p(losses)))
    return losses


def pose_hypotheses(Twc16, n, max_rot, max_trans, pivot=None, seed=1):
    """mon_pose_hypotheses (host only): n candidate poses (n, 16) around Twc16 -- hypothesis 0 the pose itself, the others turned by at most max_rot
    radians about pivot (a point in the camera frame; None: the camera centre) and moved by at most max_trans per axis."""
    pose = np.ascontiguousarray(Twc16, np.float32).reshape(16); out = np.empty((int(n), 16), np.float32)
    pv = None if pivot is None else np.ascontiguousarray(pivot, np.float32).reshape(3)
    _check(lib().mon_pose_hypotheses(_p(pose), _p(pv), float(max_rot), float(max_trans), int(n), int(seed), _p(out)))
    return out


def reloc_default(**overrides):
    """mon_reloc_default, then any field overridden by keyword."""
    r = RelocParams(); _check(lib().mon_reloc_default(C.byref(r)))
    for k, v in overrides.items():
        if k not in dict(RelocParams._fields_):
            raise KeyError(k)
        setattr(r, k, v)
    return r


def _reloc_params(reloc):
    if reloc is None:
        return reloc_default()
    if isinstance(reloc, dict):
        return reloc_default(**reloc)
    return reloc


def scene_relocalise(objects, obs, candidates, params=None, c2f=None, reloc=None, side=0):
    """mon_scene_relocalise: every candidate (n, 16; candidate 0 the caller's own guess) scored in one batch, the best reloc.keep refined as
    scene_refine_camera refines them, the refined poses and their starts scored again, the lowest score returned.  Returns (Twc16, RelocResult, scores of
    the candidates); nothing about the objects changes."""
    b, prm, rp = _pose_boxes(obs), _pose_params(params), _reloc_params(reloc)
    cand = np.ascontiguousarray(candidates, np.float32).reshape(-1, 16)
    c = None if c2f is None else _c2f_params(None if c2f is True else c2f)
    pose = np.empty(16, np.float32); res = RelocResult(); scores = np.empty(cand.shape[0], np.float32)
    _check(lib().mon_scene_relocalise(_handles(objects), len(objects), int(side), _p(b), b.shape[0], _p(cand), cand.shape[0], C.byref(prm),
                                      None if c is None else C.byref(c), C.byref(rp), _p(pose), C.byref(res), _p(scores)))
    return pose, res, scores


def scene_pose_samples(objects, obs, Twc16, k, params=None, side=0, iteration=0, level_weights=None):
    """mon_debug_scene_pose_samples: object k's share of that evaluation per drawn ray: dict of x_o (n, 64, 3), x_c (n, 64, 3), t (n, 64), raw (n, 64, 4),
    dldx (n, 64, 3; object frame, 1/N included) and count (n,)."""
    b, prm = _pose_boxes(obs), _pose_params(params); pose = np.ascontiguousarray(Twc16, np.float32).reshape(16)
    n = int(prm.rays_per_iter) or int((b[:, 3].astype(np.int64) * b[:, 4]).sum())
    w = _scene_level_weights(objects, level_weights)
    o = dict(x_o=np.empty((n, 64, 3), np.float32), x_c=np.empty((n, 64, 3), np.float32), t=np.empty((n, 64), np.float32), raw=np.empty((n, 64, 4), np.float32),
             dldx=np.empty((n, 64, 3), np.float32), count=np.empty(n, np.uint32))
    _check(diag_lib().mon_debug_scene_pose_samples(_handles(objects), len(objects), int(side), _p(b), b.shape[0], _p(pose), C.byref(prm), int(iteration), _p(w),
                                                   int(k), _p(o["x_o"]), _p(o["x_c"]), _p(o["t"]), _p(o["raw"]), _p(o["dldx"]), _p(o["count"])))
    return o


def scene_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, w_rgb=1.0, w_mask=1.0, w_depth=1.0, huber=0.05, device=0):
    """mon_debug_scene_composite_grad: k_scene_composite_grad on lists laid out as scene_composite's, targets cstar (n_rays, 3), mstar (n_lists, n_rays),
    dstar (n_rays,), dn (n_rays,).  Returns dict of l (n_rays,), W (n_lists, n_rays), D (n_rays,), dalpha (n_lists, n_rays, 64), dc (n_lists, n_rays, 64, 3)."""
    t = np.ascontiguousarray(t, np.float32); L, R = t.shape[:2]
    a = np.ascontiguousarray(alpha, np.float32).reshape(L, R, 64); c = np.ascontiguousarray(rgb, np.float32).reshape(L, R, 64, 3)
    n = np.ascontiguousarray(count, np.uint32).reshape(L, R); d = np.ascontiguousarray(dn, np.float32).reshape(R)
    cs = np.ascontiguousarray(cstar, np.float32).reshape(R, 3); ms = np.ascontiguousarray(mstar, np.float32).reshape(L, R)
    dsr = np.ascontiguousarray(dstar, np.float32).reshape(R)
    o = dict(l=np.empty(R, np.float32), W=np.empty((L, R), np.float32), D=np.empty(R, np.float32), dalpha=np.empty((L, R, 64), np.float32),
             dc=np.empty((L, R, 64, 3), np.float32))
    _check(diag_lib().mon_debug_scene_composite_grad(int(device), R, L, _p(t), _p(a), _p(c), _p(n), _p(cs), _p(ms), _p(dsr), _p(d), float(w_rgb), float(w_mask),
                                                     float(w_depth), float(huber), _p(o["l"]), _p(o["W"]), _p(o["D"]), _p(o["dalpha"]), _p(o["dc"])))
    return o


def _borrowed_object(handle):
    o = ObjectNeRF.__new__(ObjectNeRF); o.h = handle; o.ds = None
    o.cfg = MonConfig(); _check(lib().mon_object_get_config(handle, C.byref(o.cfg))); o.R, o.S = o.cfg.rays_per_batch, o.cfg.n_samples
    o.close = lambda: None                     # the manager owns it
    return o


def marching_cubes(density, res3, thresh, aabb_min, aabb_max, device=0):
    """MarchingCubes + compute_mesh_1ring (marching_cubes.cu:478-509, 655-665) on a caller-supplied lattice (x fastest)."""
    rx, ry, rz = (int(v) for v in res3)
    d = np.ascontiguousarray(density, np.float32).reshape(-1); assert d.size == rx * ry * rz
    a0 = np.ascontiguousarray(aabb_min, np.float32); a1 = np.ascontiguousarray(aabb_max, np.float32)
    nv = C.c_uint32(0); nr = C.c_uint32(0); ni = C.c_uint32(0)
    _check(lib().mon_marching_cubes(device, _p(d), rx, ry, rz, float(thresh), _p(a0), _p(a1), None, None, None, 0, 0, C.byref(nv), C.byref(nr), C.byref(ni)))
    verts = np.empty((nv.value, 3), np.float32); nraw = np.empty((nv.value, 3), np.float32); idx = np.empty(ni.value, np.uint32)
    _check(lib().mon_marching_cubes(device, _p(d), rx, ry, rz, float(thresh), _p(a0), _p(a1), _p(verts), _p(nraw), _p(idx), nv.value, ni.value, C.byref(nv),
            C.byref(nr), C.byref(ni)))
    return dict(verts=verts, normals_raw=nraw, indices=idx, n_verts_real=nr.value)


def generate_toc(theta_deg, phi_deg, radius):
    T = np.empty(16, np.float32); _check(lib().mon_generate_toc(theta_deg, phi_deg, radius, _p(T))); return T


def acc_layout(epad, W, NH, L):
    """param[n_cols]: the MLP parameter each column of k_fused_train's dW partial rows sums into (frag_layout.h acc_param; -1 = pad column)."""
    nc = C.c_int(0)
    _check(diag_lib().mon_debug_acc_layout(epad, W, NH, L, None, C.byref(nc)))
    prm = np.empty(nc.value, np.int32)
    _check(diag_lib().mon_debug_acc_layout(epad, W, NH, L, _p(prm), C.byref(nc))); return prm


def frag_layout(epad, W, NH, L):
    """(source[n_image], slots[n_mlp, 2]) of the fused kernels' A-fragment image (frag_layout.h)."""
    ni = C.c_int(0); nm = C.c_int(0)
    _check(diag_lib().mon_debug_frag_layout(epad, W, NH, L, None, None, C.byref(ni), C.byref(nm)))
    src = np.empty(ni.value, np.int32); sl = np.empty((nm.value, 2), np.int32)
    _check(diag_lib().mon_debug_frag_layout(epad, W, NH, L, _p(src), _p(sl), C.byref(ni), C.byref(nm))); return src, sl
