"""ro-map_amd: MI355X-native Multi-Object-NeRF core for RO-MAP (host mirror + ctypes view of the C ABI).

The product is the C-ABI shared library `libmon_core.so` (include/mon_core.h); this Python package is a
thin ctypes view used by tests, bench.py and tools.  The directory name contains a hyphen, so load it
with `__graft_entry__.load_package()` (importlib) rather than `import`.
"""
from .binding import (MonConfig, MonBBox, MonError, Dataset, ObjectNeRF, default_config, config_from_json, device_count, lib, lib_path,  # noqa: F401
                      exported_symbols, BUF, selftest_mfma, microbench, fast_index, OfflineManager, OnlineManager, png_read, png_write, marching_cubes,
                              generate_toc, frag_layout, acc_layout, device_mem_info, set_logical_devices, set_offline_schedule, set_option, get_option, diag_lib, diag_lib_path,
                              diag_symbols, yaml_number, MonRenderSkipStats, render_scene, scene_samples, scene_composite, PoseRefineParams, pose_refine_default,
                      PoseC2FParams, pose_c2f_default, pose_c2f_weights, scene_pose_loss, scene_refine_camera, scene_pose_samples,
                      scene_composite_grad, RelocParams, RelocResult, reloc_default, scene_pose_loss_batch, pose_hypotheses, scene_relocalise,
                      SceneQuery, SCENE_QUERY_DTYPE, scene_queries, rect_queries, probe_scene, scene_probe_rays, scene_probe_composite,
                      SceneRay, SCENE_RAY_DTYPE, scene_rays, camera_rays, cast_scene, scene_cast_rays, scene_cast_composite,
                      query_object_points, query_scene_points, query_scene_lattice, lattice_points, scene_point_rows,
                      distance_transform, scene_distance_lattice,
                      signed_distance_transform, scene_signed_distance_lattice, scene_signed_dist_field, edge_points, MON_SIGNED_LOG,
                      label_components, scene_components_lattice, LATTICE_COMPONENT_DTYPE,
                      shortest_paths, scene_paths_lattice, lattice_path, paths_stats,
                      DistField, DistFieldDesc, TrajScoreParams, ScanMatchParams, RegisterParams, TraceParams, BeamParams, dist_field_create, scene_dist_field,
                      query_object_gradients, query_scene_gradients, query_scene_lattice_gradients, cast_scene_normals, scene_gradient_rows,
                      WindowParams, window_default, window_frames, scene_window_loss, scene_refine_window,
                      CheckpointInfo, checkpoint_info, checkpoint_timing, MON_LOAD_BOXES,
                      rccl_lib, rccl_lib_path, rccl_symbols, gather_plan, Gather)
