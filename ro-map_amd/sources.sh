# The sources of libmon_core.so, in csrc/: sourced by build.sh, tools/variant_build.sh and tests/tsan/build_and_run.sh.
SRCS=(config.cpp model.cpp train.cpp pose.cpp scene.cpp scene_field.cpp dist_field.cpp scene_pose.cpp checkpoint.cpp c_api.cpp manager.cpp png_io.cpp mesh.cpp kernels_batch.hip kernels_net.hip kernels_net_wide.hip
      kernels_net_deep.hip kernels_layers.hip kernels_composite.hip kernels_optim.hip kernels_fused.hip kernels_scatter.hip kernels_render.hip
      kernels_tilerender.hip kernels_encode.hip kernels_step.hip kernels_bigscatter.hip kernels_mesh.hip kernels_pose.hip kernels_scene_pose.hip
      kernels_scene_score.hip kernels_scene_window.hip kernels_scene_probe.hip
      kernels_scene_cast.hip kernels_scene_points.hip kernels_scene_gradients.hip kernels_distance.hip kernels_signed_distance.hip kernels_components.hip
      kernels_paths.hip kernels_clearance.hip kernels_scan_match.hip kernels_field_trace.hip)
