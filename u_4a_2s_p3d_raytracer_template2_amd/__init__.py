"""MI355X-native Whitted renderer for P3D .p3f scenes -- Python harness over the C-ABI.

The product is csrc/ (HIP kernels, C-ABI, C++ host layer).  This package is the thin ctypes
binding that tests/ and bench.py drive it through; it holds no rendering logic and has no CPU
fallback: importing `api` without a built libp3d_hip.so raises.
"""
from .api import (PathTracer, pt_debug_hash, pt_debug_hit_world, pt_debug_scatter, pt_debug_direct_lighting, ACCEL_BVH, ACCEL_GRID, ACCEL_NONE, Counters, DeviceScene, HostScene, P3DError,
                  build_native, debug_intersect, debug_powf, debug_rand, debug_sample_stream, debug_denoise, host_denoise, debug_denoise_variance, host_denoise_variance, debug_accumulate, host_accumulate, debug_accumulate_moving, host_accumulate_moving, debug_accumulate_variance, host_accumulate_variance, host_ao_segments, host_ao_resolve, host_indirect_resolve, host_path_next, host_path_add, debug_pow, debug_schlick_kr, debug_check_rcp, debug_check_rcp_len, device_count, host_bvh, lib, local_rows, Comm, comm_unique_id,
                  gather_all, tune_schedule, FEATURE_SCHLICK, orbit_eyes, host_tile_coverage)

__all__ = ["orbit_eyes", "PathTracer", "pt_debug_hash", "pt_debug_hit_world", "pt_debug_scatter", "pt_debug_direct_lighting", "ACCEL_BVH", "ACCEL_GRID", "ACCEL_NONE", "Counters", "DeviceScene", "HostScene", "P3DError",
           "build_native", "debug_intersect", "debug_powf", "debug_rand", "debug_sample_stream", "debug_denoise", "host_denoise", "debug_denoise_variance", "host_denoise_variance", "debug_accumulate", "host_accumulate", "debug_accumulate_moving", "host_accumulate_moving", "debug_accumulate_variance", "host_accumulate_variance", "host_ao_segments", "host_ao_resolve", "host_indirect_resolve", "host_path_next", "host_path_add", "debug_pow", "debug_schlick_kr", "debug_check_rcp", "debug_check_rcp_len", "device_count", "host_bvh", "lib", "local_rows", "Comm", "comm_unique_id",
           "gather_all", "tune_schedule", "FEATURE_SCHLICK", "host_tile_coverage"]
