"""gvom -- drop-in replacement for the reference module `gvom` on AMD MI355X (gfx950).

    import gvom
    m = gvom.Gvom(xy_resolution, z_resolution, xy_size, z_size, buffer_size, min_distance,
                  positive_obstacle_threshold, negative_obstacle_threshold,
                  slope_obstacle_threshold, robot_height, robot_radius,
                  ground_to_lidar_height, xy_eigen_dist, z_eigen_dist)
    m.process_pointcloud(pc, ego_position, transform)       # gvom_ros.py:109
    origin, positive, negative, roughness, visibility = m.combine_maps()   # gvom_ros.py:115

Same constructor (14 positional args, reference gvom.py:29-31), same methods, return types,
warning strings and ring-buffer attributes as the reference class
(/root/reference/scripts/gvom.py:12-410), so the reference's ROS node (gvom_ros.py) runs
against it unchanged.  All arithmetic happens in hand-written HIP kernels behind the C ABI
of include/gvom_hip.h, bound here with ctypes.  No PyTorch, no Numba.

There is NO CPU fallback: importing works anywhere, but constructing `Gvom` raises
`GvomBackendError` if libgvom_hip.so is missing or no gfx950 device is visible.
"""
import ctypes
import math
import os
import threading

import numpy as np

__all__ = ["Gvom", "GvomBackendError", "DeviceMaps", "DeviceMap", "DeviceArray", "DeviceVoxelCloud", "DeviceRays", "load_library",
           "library_path", "unproject_range_image"]

_HERE = os.path.dirname(os.path.abspath(__file__))

GVOM_OK, GVOM_EMPTY_CLOUD, GVOM_NO_OVERLAP, GVOM_EMPTY_BUFFER, GVOM_NO_DATA = 0, 1, 2, 3, 4
GVOM_ERR_INVALID = -1
GVOM_WHICH_FUSED = -1
MAP_HEIGHT, MAP_INFERRED, MAP_SLOPE_X, MAP_SLOPE_Y, MAP_ROUGHNESS, MAP_GUESSED = range(6)
BUF_HEIGHT_MAPS, BUF_FUSED_CELLS = 0, 3
N_STAGES = 5
STAGE_NAMES = ("trace", "encode", "min_height", "fuse", "map2d")


class GvomBackendError(RuntimeError):
    """The HIP backend is unavailable or a HIP call failed."""


class GvomParams(ctypes.Structure):
    _fields_ = [("xy_resolution", ctypes.c_double), ("z_resolution", ctypes.c_double),
                ("xy_size", ctypes.c_int32), ("z_size", ctypes.c_int32),
                ("buffer_size", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("min_distance", ctypes.c_double),
                ("positive_obstacle_threshold", ctypes.c_double),
                ("negative_obstacle_threshold", ctypes.c_double),
                ("slope_obstacle_threshold", ctypes.c_double),
                ("robot_height", ctypes.c_double), ("robot_radius", ctypes.c_double),
                ("ground_to_lidar_height", ctypes.c_double),
                ("xy_eigen_dist", ctypes.c_int32), ("z_eigen_dist", ctypes.c_int32)]


class GvomState(ctypes.Structure):
    _fields_ = [("buffer_index", ctypes.c_int32), ("last_buffer_index", ctypes.c_int32),
                ("has_combined", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("combined_cell_count", ctypes.c_int64),
                ("combined_origin", ctypes.c_double * 3), ("ego_position", ctypes.c_double * 3)]


class GvomScanStats(ctypes.Structure):
    _fields_ = [("points", ctypes.c_int64), ("cells", ctypes.c_int64),
                ("sum_hit", ctypes.c_int64), ("sum_total", ctypes.c_int64)]


def library_path():
    return os.environ.get("GVOM_HIP_LIBRARY", os.path.join(_HERE, "lib", "libgvom_hip.so"))


_lib = None
_lib_lock = threading.Lock()

# every symbol include/gvom_hip.h declares: (name, restype, argtypes)
_P, _I, _I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_DP = ctypes.POINTER(ctypes.c_double)
ABI = [
    ("gvom_create", _I, [ctypes.POINTER(GvomParams), _I, ctypes.POINTER(_P)]),
    ("gvom_create_sharded", _I, [ctypes.POINTER(GvomParams), _I, _I, _I, ctypes.POINTER(_P)]),
    ("gvom_destroy", None, [_P]),
    ("gvom_process_pointcloud", _I, [_P, _P, _I64, _I64, _I, _DP, _P]),
    ("gvom_process_pointcloud2", _I, [_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                       ctypes.c_int64, ctypes.c_int, _P, _P]),
    ("gvom_process_pointcloud_device", _I, [_P, _P, _I64, _I64, _I, _DP, _P]),
    ("gvom_sensor_model_set", _I, [_P, ctypes.c_int32, ctypes.c_int32, _P, _P, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    ("gvom_process_range_image", _I, [_P, _P, _I, _I, _I64, _P, _I, _DP, _P]),
    ("gvom_process_pointcloud_origins", _I, [_P, _P, _I, _I64, _I64, _I, _P, ctypes.c_int32, _P, _DP, _P]),
    ("gvom_process_range_image_origins", _I, [_P, _P, _I, _I, _I64, _P, _I, _DP, _P]),
    ("gvom_combine_maps", _I, [_P, _P, _P, _P, _P, _P]),
    ("gvom_output_buffer_alloc", _I, [_P, ctypes.POINTER(_P)]),
    ("gvom_output_buffer_free", _I, [_P, _P]),
    ("gvom_combine_maps_into", _I, [_P, _P, _P]),
    ("gvom_output_forget", _I, [_P, _P]),
    ("gvom_output_record", _I, [_P, _P, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)]),
    ("gvom_combine_occupancy_into", _I, [_P, _P, _P, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    ("gvom_shard_scan_local", _I, [_P, _P, _I, _I64, _I64, _I, _DP, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64),
                                   ctypes.POINTER(_I)]),
    ("gvom_shard_buffer", _I, [_P, _I, _I, ctypes.POINTER(_P), ctypes.POINTER(_I64)]),
    ("gvom_shard_recv_reserve", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_shard_scan_merge", _I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), _I]),
    ("gvom_shard_stats_counts", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_shard_stats_reserve", _I, [_P, ctypes.POINTER(_I64), _I]),
    ("gvom_combine_fuse", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_set_combined_cell_count", _I, [_P, _I64]),
    ("gvom_sync", _I, [_P]),
    ("gvom_device_buffer", _I, [_P, _I, ctypes.POINTER(_P), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_combine_map2d_into", _I, [_P, _P, _P]),
    ("gvom_comm_create", _I, [_I, _I, _I, ctypes.c_char_p, ctypes.POINTER(_P)]),
    ("gvom_comm_create2", _I, [_I, _I, _I, ctypes.c_char_p, _I, ctypes.POINTER(_P)]),
    ("gvom_comm_transport", _I, [_P]),
    ("gvom_comm_before_scan", _I, [_P]),
    ("gvom_comm_before_combine", _I, [_P]),
    ("gvom_comm_peer_async", _I, [_P]),
    ("gvom_comm_peer_stats", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_comm_peer_renewed", _I64, [_P]),
    ("gvom_comm_info", _I, [_P, ctypes.POINTER(_I64), ctypes.c_char_p, ctypes.c_size_t]),
    ("gvom_comm_wire_stats", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_comm_abort", _I, [_P]),
    ("gvom_shard_renew_region", _I, [_P, _I]),
    ("gvom_comm_destroy", None, [_P]),
    ("gvom_comm_exchange_host", _I, [_P, ctypes.POINTER(_I64), _I, ctypes.POINTER(_I64)]),
    ("gvom_comm_barrier", _I, [_P]),
    ("gvom_comm_exchange_scan", _I, [_P, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64),
                                     ctypes.POINTER(_I64)]),
    ("gvom_comm_exchange_stats", _I, [_P, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), _I]),
    ("gvom_comm_allgather_rows", _I, [_P, _P]),
    ("gvom_comm_process_pointcloud", _I, [_P, _P, _P, _I, ctypes.c_int64, ctypes.c_int64, _I, _P, _P, _P]),
    ("gvom_comm_combine_maps_into", _I, [_P, _P, _P, _P]),
    ("gvom_comm_rank", _I, [_P]),
    ("gvom_comm_world", _I, [_P]),
    ("gvom_comm_last_error", ctypes.c_char_p, [_P]),
    ("gvom_slot_filled", _I, [_P, _I]),
    ("gvom_get_state", _I, [_P, ctypes.POINTER(GvomState)]),
    ("gvom_get_scan_stats", _I, [_P, ctypes.POINTER(GvomScanStats)]),
    ("gvom_get_occupancy", _I, [_P, _P]),
    ("gvom_debug_voxel_map", _I, [_P, _P, _I64, ctypes.POINTER(_I64)]),
    ("gvom_debug_voxel_eigen", _I, [_P, _P, _P, _I64, ctypes.POINTER(_I64)]),
    ("gvom_read_rows", _I, [_P, _I, _P]),
    ("gvom_gather_metrics", _I, [_P, _I, _P, _I64, _P]),
    ("gvom_debug_height_map", _I, [_P, _P]),
    ("gvom_debug_inferred_height_map", _I, [_P, _P]),
    ("gvom_read_dense", _I, [_P, _I, _P, _P, _P, _P, _P, ctypes.POINTER(_I64)]),
    ("gvom_read_map2d", _I, [_P, _I, _P]),
    ("gvom_last_stage_ms", _I, [_P, ctypes.POINTER(ctypes.c_float * N_STAGES)]),
    ("gvom_combine_begin", _I, [_P, _P, _P]),
    ("gvom_combine_end", _I, [_P, _P]),
    ("gvom_combine_maps_device", _I, [_P, _P, ctypes.POINTER(_I64)]),
    ("gvom_device_map_export", _I, [_P, _I64, _I, _P, ctypes.POINTER(_P), ctypes.POINTER(_I64)]),
    ("gvom_device_map_release", _I, [_P, _I64, _P]),
    ("gvom_device_map_dlpack", _I, [_P, _I64, _I, _P, _I, ctypes.POINTER(_P)]),
    ("gvom_device_map_copy", _I, [_P, _I64, _I, _P]),
    ("gvom_device_product", _I, [_P, _I, _I64, ctypes.POINTER(_I64)]),
    ("gvom_device_product_export", _I, [_P, _I64, _I, _P, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_device_product_release", _I, [_P, _I64, _P]),
    ("gvom_device_product_dlpack", _I, [_P, _I64, _I, _P, _I, ctypes.POINTER(_P)]),
    ("gvom_device_product_copy", _I, [_P, _I64, _I, _P]),
    ("gvom_clearance", _I, [_P, _I64, _P, _P, _I, ctypes.c_double, ctypes.c_int32, _I, ctypes.POINTER(_I64)]),
    ("gvom_raycast", _I, [_P, _P, _I64, _P, _I64, _I, _I, _DP, ctypes.POINTER(_I64)]),
    ("gvom_cost_to_go", _I, [_P, _I64, _P, _P, _I, _P, _I64, ctypes.c_int32, ctypes.c_int32, _I, ctypes.POINTER(_I64),
                             ctypes.POINTER(_I64)]),
    ("gvom_footprint_set", _I, [_P, ctypes.c_int32, _P, _P]),
    ("gvom_score_rollouts", _I, [_P, _I64, _P, _P, _P, _I64, _I64, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_chassis_set", _I, [_P, _P, ctypes.c_int32, _P]),
    ("gvom_score_attitude", _I, [_P, _I64, _P, _P, _I64, _I64, _I, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_body_set", _I, [_P, _P, ctypes.c_int32]),
    ("gvom_score_body", _I, [_P, _I64, _P, ctypes.POINTER(_I64), _I64, _P, _P, _I64, _I64, _I, _I, ctypes.POINTER(_I64), ctypes.c_float,
                             ctypes.POINTER(_I64)]),
    ("gvom_score_alignments", _I, [_P, _P, _I64, _P, _I64, _I, _I, _P, ctypes.POINTER(_I64)]),
    ("gvom_frontiers", _I, [_P, _I64, _I64, _P, _P, _P, _I, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_score_viewpoints", _I, [_P, _P, _I64, _I, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _I, _P, ctypes.POINTER(_I64)]),
    ("gvom_primitives_set", _I, [_P, ctypes.c_int32, _P, _P]),
    ("gvom_pose_field", _I, [_P, _I64, _P, _I, _P, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_attitude_volume", _I, [_P, _I64, _P, _I, _I, ctypes.POINTER(_I64)]),
    ("gvom_pose_field_attitude", _I, [_P, _I64, _P, _I, _I64, ctypes.c_uint32, ctypes.c_int32, _P, _I64, ctypes.c_int32, ctypes.c_int32,
                                      ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_body_volume", _I, [_P, _I64, _P, ctypes.POINTER(_I64), _I64, _P, _I, _I, ctypes.POINTER(_I64), ctypes.c_float, ctypes.c_float,
                              ctypes.POINTER(_I64)]),
    ("gvom_pose_field_volumes", _I, [_P, _I64, _P, _I, _I64, ctypes.c_uint32, ctypes.c_int32, _I64, ctypes.c_uint32, ctypes.c_int32, _P, _I64,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_device_map_origin", _I, [_P, _I64, ctypes.POINTER(_I64)]),
    ("gvom_atlas_configure", _I, [_P, ctypes.c_int32, _I, ctypes.POINTER(_I64)]),
    ("gvom_atlas_integrate", _I, [_P, _I64, ctypes.POINTER(_P), _I, ctypes.POINTER(_I64)]),
    ("gvom_atlas_recall", _I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), _P]),
    ("gvom_atlas_extent", _I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_atlas_clear", _I, [_P]),
    ("gvom_atlas_counts", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_atlas_cost_to_go", _I, [_P, _P, ctypes.POINTER(_I64), _I64, ctypes.c_int32, ctypes.c_int32, _I, ctypes.POINTER(_I64),
                                   ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_atlas_field_window", _I, [_P, _I64, _I64, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_atlas_frontiers", _I, [_P, _I64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_configure", _I, [_P, ctypes.c_int32, ctypes.c_int32, _I, ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_integrate", _I, [_P]),
    ("gvom_voxel_atlas_clear", _I, [_P]),
    ("gvom_voxel_atlas_counts", _I, [_P, ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_box", _I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_changes", _I, [_P, _I, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_raycast", _I, [_P, _P, _I64, _P, _I64, _I, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_score_viewpoints", _I, [_P, _P, _I64, _I, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _I, ctypes.POINTER(_I64),
                                               ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_score_alignments", _I, [_P, _P, _I64, _P, _I64, _I, _I, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_voxel_atlas_distance_field", _I, [_P, ctypes.POINTER(_I64), ctypes.c_double, _I, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("gvom_voxel_distance_sample", _I, [_P, _I64, _P, _I64, _I, ctypes.POINTER(_I64)]),
    ("gvom_set_profiling", _I, [_P, _I]),
    ("gvom_host_timing", _I, [_P, ctypes.POINTER(ctypes.c_double * 8)]),
    ("gvom_set_tuning", _I, [_P, ctypes.c_char_p, _I]),
    ("gvom_get_tuning", _I, [_P, ctypes.c_char_p, ctypes.POINTER(_I)]),
    ("gvom_stream", _P, [_P]),
    ("gvom_alloc_generation", ctypes.c_uint64, [_P]),
    ("gvom_region_generation", ctypes.c_uint64, [_P, _I]),
    ("gvom_last_error", ctypes.c_char_p, [_P]),
    ("gvom_backend_info", _I, [ctypes.c_char_p, ctypes.c_size_t]),
    ("gvom_abi_version", _I, []),
]


ABI_VERSION = 10         # include/gvom_hip.h GVOM_ABI_VERSION this binding was written against


def load_library(path=None):
    """dlopen libgvom_hip.so and bind every C-ABI entry point.  Raises GvomBackendError."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or library_path()
        if not os.path.exists(p):
            raise GvomBackendError(
                "HIP backend not built: %s is missing. Run `make -C %s` (or "
                "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
                % (p, _HERE))
        try:
            L = ctypes.CDLL(p)
        except OSError as e:
            raise GvomBackendError("cannot load %s: %s" % (p, e))
        for name, res, args in ABI:
            try:
                f = getattr(L, name)
            except AttributeError:
                raise GvomBackendError("%s does not export %s" % (p, name))
            f.restype = res
            f.argtypes = args
        if L.gvom_abi_version() != ABI_VERSION:
            raise GvomBackendError("%s has C ABI version %d, this binding needs %d: rebuild it (`make -C %s`)"
                                   % (p, L.gvom_abi_version(), ABI_VERSION, _HERE))
        if path is None:
            _lib = L
        return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dev(p):
    """a raw device (or pinned host) address as the library takes it; None and 0 are the null pointer"""
    return ctypes.c_void_p(int(p)) if p else None


def _device_cloud(dtype, row_stride_bytes=None):
    """(dtype code, row stride in bytes) of a cloud in device memory: float32 is code 0, anything else is read as float64 (1);
    the rows are packed x, y, z unless a stride is given"""
    code = 0 if (dtype is np.float32 or np.dtype(dtype) == np.float32) else 1
    return code, row_stride_bytes or (12 if code == 0 else 24)


def _warn_scan(rc):
    """the reference's two warnings about a scan that changes nothing, for the return codes that stand for them"""
    if rc == GVOM_EMPTY_CLOUD:
        print("[WARNING] Processing an empty pointcloud, nothing will happen!")
    elif rc == GVOM_NO_OVERLAP:
        print("[WARNING] The pointcloud points don't overlap with any voxels, nothing will happen!")


def _warn_empty_ring():
    print("[WARNING] The map buffer is empty, nothing will happen!")


RANGE_U16, RANGE_U32, RANGE_F32 = 0, 1, 2                   # GVOM_RANGE_*
_RANGE_CODES = {np.dtype(np.uint16): RANGE_U16, np.dtype(np.uint32): RANGE_U32, np.dtype(np.float32): RANGE_F32}


def _range_code(dtype):
    try:
        return _RANGE_CODES[np.dtype(dtype)]
    except (KeyError, TypeError):
        raise ValueError("a range image is uint16, uint32 or float32, got %r" % (dtype,))


def _cloud_code(dtype):
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("cloud_dtype must be float32 or float64, got %r" % (dtype,))
    return 0 if dt == np.dtype(np.float32) else 1


def _column_poses(column_transforms, W):
    """[W, 4, 4] or [W, 3, 4] -> C-contiguous float64 [W, 12] (rows 0..2 of every matrix), or None"""
    if column_transforms is None:
        return None
    c = np.asarray(column_transforms, dtype=np.float64)
    if c.ndim != 3 or c.shape[0] != W or c.shape[1] not in (3, 4) or c.shape[2] != 4:
        raise ValueError("column_transforms must have shape (%d, 4, 4) or (%d, 3, 4), got %r" % (W, W, c.shape))
    return np.ascontiguousarray(c[:, :3, :]).reshape(W, 12)


def unproject_range_image(ranges, directions, offsets=None, range_scale=0.001, min_range=0.0, max_range=float("inf"),
                          column_transforms=None, cloud_dtype=np.float32, drop_invalid=False):
    """What Gvom.process_range_image scans, computed with numpy on the CPU: the [H*W, 3] cloud of `cloud_dtype` of a range
    image -- include/gvom_hip.h "range images", operation for operation, every one a float64 operation rounded once:

        r      = float64(raw) * range_scale
        valid  = raw != 0 and r finite and min_range <= r <= max_range
        p[k]   = r * dir[k] + off[k]                                              (multiply, then add)
        q[k]   = ((p[0]*C[w][k][0] + p[1]*C[w][k][1]) + p[2]*C[w][k][2]) + C[w][k][3]       (with column_transforms)
        xyz    = cloud_dtype(q)  where valid, else (NaN, NaN, NaN)                (ONE rounding, at the end)

    ranges [H, W] uint16 / uint32 / float32; directions [H, W, 3]; offsets [H, W, 3] or None (zeros); column_transforms
    [W, 4, 4] or [W, 3, 4] or None.  drop_invalid: the invalid pixels' rows removed, the order of the others kept (the cloud a
    node that filters its returns hands to process_pointcloud).  The library computes the same bits on the GPU."""
    raw = np.asarray(ranges)
    _range_code(raw.dtype)
    if raw.ndim != 2:
        raise ValueError("ranges must have shape (H, W), got %r" % (raw.shape,))
    H, W = raw.shape
    d = np.asarray(directions, dtype=np.float64)
    if d.shape != (H, W, 3):
        raise ValueError("directions must have shape (%d, %d, 3), got %r" % (H, W, d.shape))
    o = np.zeros((H, W, 3)) if offsets is None else np.asarray(offsets, dtype=np.float64)
    if o.shape != (H, W, 3):
        raise ValueError("offsets must have shape (%d, %d, 3), got %r" % (H, W, o.shape))
    _cloud_code(cloud_dtype)
    scale = np.float64(range_scale)
    with np.errstate(invalid="ignore", over="ignore"):
        r = raw.astype(np.float64) * scale
        valid = (raw != 0) & np.isfinite(r) & (np.float64(min_range) <= r) & (r <= np.float64(max_range))
        p = [r * d[:, :, k] + o[:, :, k] for k in range(3)]
        q = p
        if column_transforms is not None:
            C = _column_poses(column_transforms, W).reshape(W, 3, 4)
            q = [((p[0] * C[None, :, k, 0] + p[1] * C[None, :, k, 1]) + p[2] * C[None, :, k, 2]) + C[None, :, k, 3]
                 for k in range(3)]
        xyz = np.stack(q, axis=-1)
        xyz[~valid] = np.nan
        xyz = xyz.reshape(H * W, 3).astype(cloud_dtype)
    if drop_invalid:
        xyz = xyz[valid.reshape(-1)]
    return np.ascontiguousarray(xyz)


def column_origins(column_transforms, transform=None):
    """The ray origins of Gvom.process_range_image_origins: [W, 3] float64, row w = the translation of column
    w's pose taken through `transform` in the cloud transform's order of operations (include/gvom_hip.h "multi-origin scans"):

        t = C[w][:, 3];   O[w][k] = ((t[0]*tf[k][0] + t[1]*tf[k][1]) + t[2]*tf[k][2]) + tf[k][3]      (O[w] = t without a transform)

    so that process_range_image_origins(r, ego, tf, cols) is
    process_pointcloud_origins(unproject_range_image(r, <model>, column_transforms=cols), column_origins(cols, tf), ego, tf)."""
    c = np.asarray(column_transforms, dtype=np.float64)
    if c.ndim != 3 or c.shape[1] not in (3, 4) or c.shape[2] != 4:
        raise ValueError("column_transforms must have shape (W, 4, 4) or (W, 3, 4), got %r" % (c.shape,))
    t = np.ascontiguousarray(c[:, :3, 3])
    if transform is None:
        return t
    tf = np.asarray(transform, dtype=np.float64)
    if tf.shape != (4, 4):
        raise ValueError("transform must be 4x4")
    return np.stack([((t[:, 0] * tf[k, 0] + t[:, 1] * tf[k, 1]) + t[:, 2] * tf[k, 2]) + tf[k, 3] for k in range(3)], axis=-1)


def _origin_table(origins):
    """[K, 3] finite float64, 1 <= K <= 65536 (C-contiguous)"""
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.float64))
    if o.ndim != 2 or o.shape[1] != 3:
        raise ValueError("origins must have shape (K, 3), got %r" % (o.shape,))
    if not 1 <= o.shape[0] <= 65536:
        raise ValueError("origins: 1 <= K <= 65536, got K = %d" % o.shape[0])
    if not np.isfinite(o).all():
        raise ValueError("origins must be finite")
    return o


class _DeviceArrayView(object):
    """Stands in for the reference's numba device arrays: `.copy_to_host()` returns numpy."""

    def __init__(self, fetch):
        self._fetch = fetch

    def copy_to_host(self):
        return self._fetch()

    def __array__(self, dtype=None):
        a = self._fetch()
        return a if dtype is None else a.astype(dtype)


# ---- device-resident maps (Gvom.combine_maps_device) ------------------------------------------
DEVICE_MAP_NAMES = ("positive", "negative", "visibility", "roughness", "height_map", "inferred_height_map",
                    "x_slope_map", "y_slope_map", "guessed_height_delta")     # map index 0..8 of a set (include/gvom_hip.h)
_STREAM_NOSYNC = (1 << 64) - 1            # GVOM_STREAM_NOSYNC
_KDL_ROCM = 10
_DLTENSOR, _DLTENSOR_VERSIONED = b"dltensor", b"dltensor_versioned"    # (module constants: a capsule keeps a pointer to its name)
_DELETER_T = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
_capi = None


def _capsule_api():
    global _capi
    if _capi is None:
        api = ctypes.pythonapi
        api.PyCapsule_New.restype = ctypes.py_object
        api.PyCapsule_New.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
        api.PyCapsule_IsValid.restype = ctypes.c_int
        api.PyCapsule_IsValid.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        api.PyCapsule_GetPointer.restype = ctypes.c_void_p
        api.PyCapsule_GetPointer.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        _capi = api
    return _capi


def _capsule_destructor(name, deleter_offset):
    """PyCapsule destructor: a capsule nobody consumed (a consumer renames it "used_...") still holds an export -- its managed
    tensor's deleter (C code of the library) releases it."""
    def dtor(cap):
        api = _capsule_api()
        if api.PyCapsule_IsValid(cap, name):
            managed = api.PyCapsule_GetPointer(cap, name)
            fn = ctypes.c_void_p.from_address(managed + deleter_offset).value
            if fn:
                _DELETER_T(fn)(managed)
    return _DELETER_T(dtor)


# deleter offsets: DLManagedTensor {DLTensor (48 B), manager_ctx, deleter}; DLManagedTensorVersioned {version, manager_ctx, deleter, ...}
_DTOR_LEGACY = _capsule_destructor(_DLTENSOR, 56)
_DTOR_VERSIONED = _capsule_destructor(_DLTENSOR_VERSIONED, 16)


def _stream_arg(stream):
    """DLPack stream value -> the library's consumer stream: None = the null stream, an integer = a hipStream_t (torch on ROCm
    passes 0 for its default stream), -1 = no synchronisation."""
    if stream is None:
        return None
    s = int(stream)
    if s == -1:
        return ctypes.c_void_p(_STREAM_NOSYNC)
    if s < 0:
        raise ValueError("stream must be None, -1 or a hipStream_t, got %r" % (stream,))
    return ctypes.c_void_p(s) if s else None


def _dlpack_capsule(g, export, ident, part, what, stream, max_version, dl_device, copy):
    """__dlpack__ of a DeviceMap (what = "map") or a DeviceArray ("array") of the mapper g: one export of part `part` of the set
    `ident` through `export` (gvom_device_map_dlpack / gvom_device_product_dlpack), in a capsule whose destructor gives it back."""
    device = (_KDL_ROCM, g._device)
    if copy:
        raise BufferError("copy=True is not supported: the %s is shared in place" % what)
    if dl_device is not None and tuple(int(v) for v in dl_device) != device:
        raise BufferError("the %s lives on %r; no cross-device export" % (what, device))
    versioned = max_version is not None and int(max_version[0]) >= 1
    managed = ctypes.c_void_p()
    g._check(export(g._h, ident, part, _stream_arg(stream), 1 if versioned else 0, ctypes.byref(managed)))
    name, dtor = (_DLTENSOR_VERSIONED, _DTOR_VERSIONED) if versioned else (_DLTENSOR, _DTOR_LEGACY)
    return _capsule_api().PyCapsule_New(managed.value, name, ctypes.cast(dtor, ctypes.c_void_p))


class _WithRelease(object):
    """`with` support of everything that has a release()"""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()
        return False


class _Export(_WithRelease):
    """One export of a device set held by a Python object (`_owner`: the mapper, `_held`: not given back yet): given back once, by
    release() or on collection, through the entry point `_release_name` with the id the attribute `_id_name` holds."""
    _release_name = _id_name = None

    def release(self):
        if self.__dict__.get("_held"):
            self._held = False
            g = self._owner
            if g._h:
                g._check(getattr(g._lib, self._release_name)(g._h, getattr(self, self._id_name), ctypes.c_void_p(_STREAM_NOSYNC)))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class DeviceMap(object):
    """One map of a device map set: [x, y]-indexed, column-major in device memory (strides (1, xy) in elements).
    `__dlpack__` hands it to a GPU consumer without a copy (torch.from_dlpack); `copy_to_host()` returns numpy."""

    def __init__(self, maps, which):
        self._maps = maps
        self._which = which
        xy = maps._owner.xy_size
        self.shape = (xy, xy)
        self.dtype = np.dtype(np.int32) if which < 3 else np.dtype(np.float64)

    def __dlpack_device__(self):
        return (_KDL_ROCM, self._maps._owner._device)

    def __dlpack__(self, stream=None, max_version=None, dl_device=None, copy=None):
        g = self._maps._owner
        return _dlpack_capsule(g, g._lib.gvom_device_map_dlpack, self._maps.set_id, self._which, "map", stream, max_version, dl_device, copy)

    @property
    def ptr(self):
        """Device address of the map."""
        g = self._maps._owner
        p, st = ctypes.c_void_p(), (_I64 * 2)()
        nosync = ctypes.c_void_p(_STREAM_NOSYNC)
        g._check(g._lib.gvom_device_map_export(g._h, self._maps.set_id, self._which, nosync, ctypes.byref(p), st))
        g._check(g._lib.gvom_device_map_release(g._h, self._maps.set_id, nosync))
        return int(p.value)

    def copy_to_host(self):
        """numpy [x, y] (Fortran order), equal to what combine_maps returns / the attribute of the same name reads."""
        g = self._maps._owner
        out = np.empty(self.shape, self.dtype, order="F")
        g._check(g._lib.gvom_device_map_copy(g._h, self._maps.set_id, self._which, ctypes.c_void_p(out.ctypes.data)))
        return out

    def __array__(self, dtype=None):
        a = self.copy_to_host()
        return a if dtype is None else a.astype(dtype)


class DeviceMaps(_Export):
    """The result of Gvom.combine_maps_device(): the nine maps of one combine in device memory (one map set), as DeviceMap
    attributes named after the reference's (DEVICE_MAP_NAMES), `.origin` (f64[3], world), `.origin_cells` (the same corner as the
    three integer voxel indices the library counts it in) and `.set_id`.  A set an Atlas recalled also has `.stamps` (a DeviceArray,
    int32 [x, y]: the integrate that last wrote each cell, 0 = never) and `.recall_counts`.  It holds one export
    of the set -- the set is not reused while it lives -- given back by release(), by leaving a `with` block, or when it is
    collected.  Tensors taken through DLPack hold exports of their own and stay valid after release() (and after the mapper)."""
    _release_name, _id_name = "gvom_device_map_release", "set_id"

    def __init__(self, owner, set_id, origin):
        self._owner = owner
        self.set_id = set_id
        self.origin = origin
        p, st = ctypes.c_void_p(), (_I64 * 2)()
        owner._check(owner._lib.gvom_device_map_export(owner._h, set_id, 0, ctypes.c_void_p(_STREAM_NOSYNC), ctypes.byref(p), st))
        self._held = True
        cells = (_I64 * 3)()
        owner._check(owner._lib.gvom_device_map_origin(owner._h, set_id, cells))
        self.origin_cells = tuple(int(v) for v in cells)

    def __getattr__(self, name):
        if name in DEVICE_MAP_NAMES:
            return DeviceMap(self, DEVICE_MAP_NAMES.index(name))
        raise AttributeError(name)

    def release(self):
        """Gives the export back -- and, of a recalled set, the one its `.stamps` and `.recall_counts` share."""
        _Export.release(self)
        hold = self.__dict__.get("_recall_hold")
        if hold is not None:
            hold.release()

    def clearance(self, density_threshold=50, include_negative=True, max_distance=None):
        """Distance of every cell to the nearest hard obstacle of this set's positive / negative maps -- a cell is one iff
        positive > density_threshold or (include_negative and) negative > 0, the non-zero cells of the node's hard-obstacle grid
        -- as a DeviceClearance, computed on the GPU behind the combine that wrote the set; no host wait.  max_distance (metres):
        cells further than that from every obstacle read +inf / CLEARANCE_FAR, and the transform looks no further."""
        g = self._owner
        return g._clearance(self.set_id, None, None, 0, density_threshold, include_negative, max_distance)

    def score_attitude(self, poses, inferred_ground=True):
        """How the vehicle would sit on this set's ground at every pose of K candidate trajectories: pitch, roll and belly clearance
        from the `height` map (and, with inferred_ground, the `inferred height` map where the height is unknown), with the mapper's
        footprint table and chassis (Gvom.set_footprint, Gvom.set_chassis) -- a DeviceAttitude, computed on the GPU behind the
        combine that wrote the set; no host wait once the poses are up.  poses: (K, T, 3) = (x, y, yaw) in world metres and radians,
        ROUNDED TO float32.  include/gvom_hip.h "terrain attitude scoring" has the definition."""
        g = self._owner
        a = _rollout_poses(poses)
        return g._score_attitude(self.set_id, None, _ptr(a), a.shape[0], a.shape[1], 0, bool(inferred_ground), self.origin)

    def attitude_volume(self, inferred_ground=True):
        """How the vehicle would sit on this set's ground at EVERY state of the window -- the centre of each cell at each heading of
        the mapper's footprint table, with its chassis (Gvom.set_footprint, Gvom.set_chassis) -- a DeviceAttitudeVolume (status and
        tilt per state), computed on the GPU behind the combine that wrote the set; no host wait.  The ground is score_attitude()'s.
        DeviceCostField.pose_field(attitude=...) takes it into a pose field.  include/gvom_hip.h "attitude volumes" has the
        definition."""
        return self._owner._attitude_volume(self.set_id, None, 0, bool(inferred_ground))

    def cost_to_go(self, goals, goals_in_cells=False, inflation_radius=None, density_threshold=50, include_negative=True,
                   unknown="free", base=1, soft_weight=0, rough_weight=0, roughness_range=None, max_cost=None, max_rounds=0):
        """The navigation function of this set's maps towards `goals`: from every cell the cheapest 8-connected way to a goal
        (`.cost`) and the first step of it (`.direction`), as a DeviceCostField computed on the GPU behind the combine that wrote
        the set.  The call waits for the field.  goals: (G, 2) world metres (x, y) -- or window cells with goals_in_cells=True; a
        goal outside the window raises ValueError, one on a blocked cell seeds nothing.  A cell is blocked where positive >
        density_threshold, (include_negative and) negative > 0, within inflation_radius metres of such a cell (None: no
        inflation; as clearance()'s max_distance), or -- unknown="blocked" -- never observed.  Elsewhere it costs base +
        soft_weight * positive + (an int `unknown`: that much where never observed) + rough_weight * q, at most 65535, with q =
        0 .. 100 the roughness's place in roughness_range = (min, max).  max_cost: cells dearer than that read CTG_UNREACHED.
        max_rounds > 0 stops after that many rounds (`.converged` says whether the field is final).  include/gvom_hip.h
        "cost-to-go fields" has the definition."""
        g = self._owner
        cells = _ctg_goals(goals, g.xy_size, None if goals_in_cells else (g.xy_resolution, self.origin))
        params, flags = _ctg_params(g.xy_resolution, inflation_radius, density_threshold, include_negative, unknown, base, soft_weight,
                                    rough_weight, roughness_range)
        return g._cost_to_go(self.set_id, params, None, 0, cells, _ctg_max_cost(max_cost), _ctg_max_rounds(max_rounds), flags,
                             origin=self.origin)


# ---- device-resident 3-D products (Gvom.occupancy_grid_device and friends) ----------------------------------------
PRODUCT_OCCUPANCY, PRODUCT_VOXEL_CLOUD, PRODUCT_HEIGHT_CLOUD, PRODUCT_INFERRED_HEIGHT_CLOUD = 1, 2, 3, 4    # include/gvom_hip.h
PRODUCT_CLEARANCE = 5                     # GVOM_PRODUCT_CLEARANCE: made by gvom_clearance, not by gvom_device_product
PRODUCT_RAYCAST = 6                       # GVOM_PRODUCT_RAYCAST: made by gvom_raycast, not by gvom_device_product
PRODUCT_COSTFIELD = 7                     # GVOM_PRODUCT_COSTFIELD: made by gvom_cost_to_go, not by gvom_device_product
PRODUCT_ROLLOUTS = 10                     # GVOM_PRODUCT_ROLLOUTS: made by gvom_score_rollouts (kinds 8 and 9 are not assigned)
PRODUCT_ALIGNMENT = 12                    # GVOM_PRODUCT_ALIGNMENT: made by gvom_score_alignments (kind 11 is not assigned either)
PRODUCT_ATTITUDE = 14                     # GVOM_PRODUCT_ATTITUDE: made by gvom_score_attitude (kind 13 is not assigned)
PRODUCT_FRONTIERS = 16                    # GVOM_PRODUCT_FRONTIERS: made by gvom_frontiers (kind 15 is not assigned)
PRODUCT_VIEWPOINTS = 18                   # GVOM_PRODUCT_VIEWPOINTS: made by gvom_score_viewpoints (kind 17 is not assigned)
PRODUCT_POSEFIELD = 20                    # GVOM_PRODUCT_POSEFIELD: made by gvom_pose_field (kind 19 is not assigned)
PRODUCT_ATLAS_RECALL = 22                 # GVOM_PRODUCT_ATLAS_RECALL: made by gvom_atlas_recall, beside its map set (kind 21 is not assigned)
PRODUCT_ATLAS_EXTENT = 24                 # GVOM_PRODUCT_ATLAS_EXTENT: made by gvom_atlas_extent (kind 23 is not assigned)
PRODUCT_ATLAS_FIELD = 26                  # GVOM_PRODUCT_ATLAS_FIELD: made by gvom_atlas_cost_to_go (kind 25 is not assigned)
PRODUCT_ATLAS_FRONTIERS = 28              # GVOM_PRODUCT_ATLAS_FRONTIERS: made by gvom_atlas_frontiers (kind 27 is not assigned)
_ATTITUDE_BLOCKS = (1, 2, 3)              # (ATTITUDE_PITCH, ATTITUDE_ROLL, ATTITUDE_BELLY): the statuses a pose field blocks by default
PRODUCT_ATTITUDE_VOLUME = 30              # GVOM_PRODUCT_ATTITUDE_VOLUME: made by gvom_attitude_volume (kind 29 is not assigned)
PRODUCT_VOXEL_BOX = 32                    # GVOM_PRODUCT_VOXEL_BOX: made by gvom_voxel_atlas_box (kind 31 is not assigned)
PRODUCT_VOXEL_ATLAS_RAYS = 34             # GVOM_PRODUCT_VOXEL_ATLAS_RAYS: made by gvom_voxel_atlas_raycast (kind 33 is not assigned)
PRODUCT_VOXEL_ATLAS_VIEWPOINTS = 36       # GVOM_PRODUCT_VOXEL_ATLAS_VIEWPOINTS: made by gvom_voxel_atlas_score_viewpoints (kind 35 is not assigned)
PRODUCT_VOXEL_ATLAS_ALIGNMENT = 38        # GVOM_PRODUCT_VOXEL_ATLAS_ALIGNMENT: made by gvom_voxel_atlas_score_alignments (kind 37 is not assigned)
PRODUCT_VOXEL_DISTANCE = 40               # GVOM_PRODUCT_VOXEL_DISTANCE: made by gvom_voxel_atlas_distance_field (kind 39 is not assigned)
PRODUCT_VOXEL_DISTANCE_SAMPLES = 42       # GVOM_PRODUCT_VOXEL_DISTANCE_SAMPLES: made by gvom_voxel_distance_sample (kind 41 is not assigned)
PRODUCT_BODY = 44                         # GVOM_PRODUCT_BODY: made by gvom_score_body (kind 43 is not assigned)
PRODUCT_BODY_VOLUME = 46                  # GVOM_PRODUCT_BODY_VOLUME: made by gvom_body_volume (kind 45 is not assigned)
PRODUCT_VOXEL_CHANGES = 48                # GVOM_PRODUCT_VOXEL_CHANGES: made by gvom_voxel_atlas_changes (kind 47 is not assigned)
_BODY_BLOCKS = (1, 2)                    # (BODY_COLLISION, BODY_LEFT_BOX): the statuses a pose field blocks by default -- an unknown clearance is not a free one
# element type of part k of a product, by kind (what set_part() of csrc/gvom_setlayout.h gives as DLPack code and bits)
_PRODUCT_DTYPES = {PRODUCT_OCCUPANCY: (np.uint8,), PRODUCT_VOXEL_CLOUD: (np.float32, np.float32, np.int64),
                   PRODUCT_HEIGHT_CLOUD: (np.float32,), PRODUCT_INFERRED_HEIGHT_CLOUD: (np.float32,),
                   PRODUCT_CLEARANCE: (np.float32, np.int32), PRODUCT_RAYCAST: (np.int32, np.float32),
                   PRODUCT_COSTFIELD: (np.int32, np.uint8, np.uint16), PRODUCT_ROLLOUTS: (np.int32, np.uint16),
                   PRODUCT_ALIGNMENT: (np.int32, np.int32), PRODUCT_ATTITUDE: (np.int32, np.float32, np.uint8),
                   PRODUCT_FRONTIERS: (np.int32, np.int64, np.int32, np.int32), PRODUCT_VIEWPOINTS: (np.int32, np.int32),
                   PRODUCT_POSEFIELD: (np.int32, np.uint8, np.uint16), PRODUCT_ATLAS_RECALL: (np.int32, np.int32),
                   PRODUCT_ATLAS_EXTENT: (np.int32, np.int32, np.int32, np.float64, np.float64, np.int32),
                   PRODUCT_ATLAS_FIELD: (np.int32, np.uint8, np.uint16),
                   PRODUCT_ATLAS_FRONTIERS: (np.int32, np.int64, np.int32, np.int32),
                   PRODUCT_ATTITUDE_VOLUME: (np.uint8, np.uint8, np.int32),
                   PRODUCT_VOXEL_BOX: (np.uint8, np.int32), PRODUCT_VOXEL_ATLAS_RAYS: (np.int32, np.float32, np.int32),
                   PRODUCT_VOXEL_ATLAS_VIEWPOINTS: (np.int32, np.int32), PRODUCT_VOXEL_ATLAS_ALIGNMENT: (np.int32, np.int32),
                   PRODUCT_VOXEL_DISTANCE: (np.float32, np.int32), PRODUCT_VOXEL_DISTANCE_SAMPLES: (np.float32, np.int32),
                   PRODUCT_BODY: (np.int32, np.float32, np.uint8),
                   PRODUCT_BODY_VOLUME: (np.uint8, np.uint8, np.float32, np.int32),
                   PRODUCT_VOXEL_CHANGES: (np.int32, np.int64, np.int32, np.int32, np.int32, np.uint8, np.uint16)}
CLEARANCE_FAR = 2147483647                # GVOM_CLEARANCE_FAR: squared_cells where no obstacle is in reach
_CLEARANCE_NO_NEGATIVE = 1                # GVOM_CLEARANCE_NO_NEGATIVE


def _clearance_cap(max_distance, xy_resolution):
    """max_distance in metres -> max_cells2 of gvom_clearance: floor((max_distance / xy_resolution)^2); 0 (unbounded) for None,
    +inf and whatever does not fit int32.  ValueError for NaN, negative values and less than one cell."""
    if max_distance is None:
        return 0
    d = float(max_distance)
    if d != d or d < 0:
        raise ValueError("max_distance must be None or a distance >= 0 in metres, got %r" % (max_distance,))
    if d == float("inf"):
        return 0
    c = math.floor((d / float(xy_resolution)) ** 2)
    if c < 1:                                   # (the C ABI reads max_cells2 <= 0 as unbounded)
        raise ValueError("max_distance must be at least one cell (%r m), got %r" % (xy_resolution, max_distance))
    return 0 if c >= CLEARANCE_FAR else int(c)


def _clearance_threshold(density_threshold):
    t = float(density_threshold)
    if t != t:
        raise ValueError("density_threshold must be a number, got %r" % (density_threshold,))
    return t


class _ProductHold(_Export):
    """One export of a device product, held for as long as the Python object that shows it lives: the product's set is not
    reused meanwhile.  Given back by release() or on collection."""
    _release_name, _id_name = "gvom_device_product_release", "product_id"

    def __init__(self, owner, kind, product_id):
        self._owner, self.kind, self.product_id = owner, kind, product_id
        self.describe(0, hold=True)
        self._held = True

    def describe(self, part, hold=False):
        """(device address, shape, strides in elements) of a part; hold=True keeps the export it takes."""
        g = self._owner
        p, nd, sh, st = ctypes.c_void_p(), ctypes.c_int32(0), (_I64 * 3)(), (_I64 * 3)()
        nosync = ctypes.c_void_p(_STREAM_NOSYNC)
        g._check(g._lib.gvom_device_product_export(g._h, self.product_id, part, nosync, ctypes.byref(p), ctypes.byref(nd), sh, st))
        if not hold:
            g._check(g._lib.gvom_device_product_release(g._h, self.product_id, nosync))
        n = int(nd.value)
        return int(p.value), tuple(int(v) for v in sh[:n]), tuple(int(v) for v in st[:n])


class _ProductView(_WithRelease):
    """What the views of a device product share: the hold on its export (`_hold`; the views of one product share one), its
    `product_id`, and release() -- also at the end of a `with` block."""

    def __init__(self, hold):
        self._hold = hold
        self.product_id = hold.product_id

    def release(self):
        self._hold.release()


class DeviceArray(_ProductView):
    """One array of a device product in device memory, C-contiguous: the uint8 [x, y, z] occupancy grid, a float32 cloud, the
    int64 row count of a voxel cloud.  `__dlpack__` hands it to a GPU consumer without a copy (torch.from_dlpack), ordered
    behind the kernel that writes it on the consumer's stream; `copy_to_host()` returns numpy.  The product is a snapshot:
    later scans and combines do not change it.  The object holds one export of the product -- its memory is not reused while
    it lives -- given back by release(), by leaving a `with` block, or when it is collected (the parts of a DeviceVoxelCloud
    share the cloud's).  Tensors taken through DLPack hold exports of their own and stay valid after release() (and after the
    mapper)."""

    def __init__(self, hold, part=0):
        _ProductView.__init__(self, hold)
        self._part = part
        _, self.shape, self.strides = hold.describe(part)
        self.dtype = np.dtype(_PRODUCT_DTYPES[hold.kind][part])

    def __dlpack_device__(self):
        return (_KDL_ROCM, self._hold._owner._device)

    def __dlpack__(self, stream=None, max_version=None, dl_device=None, copy=None):
        g = self._hold._owner
        return _dlpack_capsule(g, g._lib.gvom_device_product_dlpack, self.product_id, self._part, "array", stream, max_version, dl_device, copy)

    @property
    def ptr(self):
        """Device address of the array."""
        return self._hold.describe(self._part)[0]

    def copy_to_host(self):
        """numpy array of `shape` and `dtype` (waits for the kernel that writes the product)."""
        g = self._hold._owner
        fortran = len(self.shape) == 2 and self.strides == (1, self.shape[0]) and self.shape[0] > 1     # (a clearance map: [x, y], x fastest)
        out = np.empty(self.shape, self.dtype, order="F" if fortran else "C")
        g._check(g._lib.gvom_device_product_copy(g._h, self.product_id, self._part, ctypes.c_void_p(out.ctypes.data)))
        return out

    def __array__(self, dtype=None):
        a = self.copy_to_host()
        return a if dtype is None else a.astype(dtype)


class _OnePartDLPack(object):
    """DLPack of a view of several arrays hands out ONE of them: the DeviceArray that the view's `_dlpack_part` names."""

    def __dlpack_device__(self):
        return getattr(self, self._dlpack_part).__dlpack_device__()

    def __dlpack__(self, stream=None, max_version=None, dl_device=None, copy=None):
        return getattr(self, self._dlpack_part).__dlpack__(stream=stream, max_version=max_version, dl_device=dl_device, copy=copy)


class DeviceVoxelCloud(_ProductView):
    """The result of Gvom.voxel_cloud_device(): `.rows` float32 [cap, 8] (the rows of make_debug_voxel_map, in unspecified
    order), `.eigenvalues` float32 [cap, 3] (row for row) and `.count` int64 [1] (rows the map has; those beyond cap are dropped),
    three DeviceArrays of one product.  copy_to_host() returns rows[:min(count, cap)] as numpy."""

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.rows, self.eigenvalues, self.count = (DeviceArray(hold, k) for k in range(3))

    def copy_to_host(self):
        n = min(int(self.count.copy_to_host()[0]), self.rows.shape[0])
        return self.rows.copy_to_host()[:n]

    def eigenvalues_to_host(self):
        n = min(int(self.count.copy_to_host()[0]), self.rows.shape[0])
        return self.eigenvalues.copy_to_host()[:n]


class DeviceClearance(_ProductView):
    """The result of DeviceMaps.clearance() / Gvom.clearance_of() / clearance_of_device(): `.distance` float32 [xy, xy], metres to
    the nearest hard obstacle (+inf where none is in reach), and `.squared_cells` int32 [xy, xy], the exact squared distance in
    cells (CLEARANCE_FAR there) -- two DeviceArrays of one product, [x, y]-indexed with strides (1, xy) like a DeviceMap.
    copy_to_host() returns (distance, squared_cells) as Fortran-ordered numpy [x, y]."""

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.distance, self.squared_cells = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.distance.copy_to_host(), self.squared_cells.copy_to_host()


RAY_CLEAR, RAY_OCCUPIED, RAY_UNKNOWN, RAY_LEFT_WINDOW, RAY_INVALID = range(5)       # GVOM_RAY_*: result[:, 0]
_RAY_UNKNOWN_BLOCKS, _RAY_CHECK_TARGET = 1, 2                                       # flags
RAYCAST_MAX_RAYS = 1 << 26


class DeviceRays(_ProductView):
    """The result of Gvom.raycast() / raycast_device(): `.result` int32 [n, 4] -- per ray {status (RAY_*), steps, voxel, unknown
    voxels passed} -- and `.position` float32 [n, 3], where the ray stopped in world metres (NaN where it did not stop at a
    voxel): two DeviceArrays of one product, row i = ray i.  `.origin`: the fused map's window origin in voxels; window voxel
    (x, y, z) = (voxel % xy, voxel // xy % xy, voxel // (xy * xy)) is world voxel origin + (x, y, z).  A snapshot: later scans
    and combines do not change it.  copy_to_host() returns (result, position) as numpy."""

    def __init__(self, hold, origin):
        _ProductView.__init__(self, hold)
        self.origin = origin
        self.result, self.position = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.result.copy_to_host(), self.position.copy_to_host()


CTG_UNREACHED = 2147483647                # GVOM_CTG_UNREACHED: cost where a cell is blocked, cut off, or dearer than max_cost
CTG_MAX_COST = 1 << 30                    # GVOM_CTG_MAX_COST
CTG_GOAL, CTG_UNSETTLED, CTG_NONE = 8, 254, 255          # GVOM_CTG_*: direction codes beside the eight steps 0 .. 7
CTG_STEPS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))   # (dx, dy) of direction code k
CTG_MAX_GOALS = 65536
_CTG_NO_NEGATIVE, _CTG_UNKNOWN_BLOCKS = 1, 2             # flags


class GvomCtgParams(ctypes.Structure):
    """gvom_ctg_params"""
    _fields_ = [("density_threshold", ctypes.c_double), ("min_roughness", ctypes.c_double), ("max_roughness", ctypes.c_double),
                ("inflation_cells2", ctypes.c_int32), ("base", ctypes.c_int32), ("soft_weight", ctypes.c_int32),
                ("unknown_cost", ctypes.c_int32), ("rough_weight", ctypes.c_int32)]


def world_to_cells(points, xy_resolution, origin):
    """(G, 2) world metres -> window cells of a map whose window corner is at `origin` (world metres, a multiple of the
    resolution): floor(p / xy_resolution) - round(origin / xy_resolution), per axis in float64."""
    p = np.asarray(points, np.float64)
    o = np.asarray(origin, np.float64)[:2]
    return (np.floor(p / float(xy_resolution)) - np.round(o / float(xy_resolution))).astype(np.int64)


def _ctg_goals(goals, xy_size, frame):
    """goals -> C-contiguous int32 (G, 2) window cells; frame = (xy_resolution, origin) for goals in world metres, None for cells"""
    a = np.asarray(goals)
    if a.ndim == 1 and a.shape[0] == 2:
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= CTG_MAX_GOALS:
        raise ValueError("goals must have shape (G, 2) with 1 <= G <= %d, got %r" % (CTG_MAX_GOALS, a.shape))
    if a.dtype.kind not in "iuf":
        raise ValueError("goals must be numbers, got dtype %s" % a.dtype)
    if a.dtype.kind == "f" and not np.isfinite(a).all():
        raise ValueError("goals must be finite")
    if frame is not None:
        a = world_to_cells(a, *frame)
    elif a.dtype.kind == "f":
        if (a != np.floor(a)).any():
            raise ValueError("goals in cells must be whole numbers")
        a = a.astype(np.int64)
    if ((a < 0) | (a >= xy_size)).any():
        bad = a[((a < 0) | (a >= xy_size)).any(axis=1)][0]
        raise ValueError("a goal lies outside the window: cell (%d, %d) of a %d x %d map" % (bad[0], bad[1], xy_size, xy_size))
    return np.ascontiguousarray(a, dtype=np.int32)


def _ctg_max_cost(max_cost):
    if max_cost is None:
        return 0
    if isinstance(max_cost, float) and max_cost != max_cost:
        raise ValueError("max_cost must be None or an integer in 1 .. 2**30, got %r" % (max_cost,))
    m = int(max_cost)
    if m != max_cost or not 1 <= m <= CTG_MAX_COST:
        raise ValueError("max_cost must be None or an integer in 1 .. 2**30, got %r" % (max_cost,))
    return m


def _ctg_max_rounds(max_rounds):
    r = int(max_rounds)
    if r != max_rounds or not 0 <= r < 2 ** 31:
        raise ValueError("max_rounds must be an integer >= 0 (0: until converged), got %r" % (max_rounds,))
    return r


def _ctg_weight(name, v, lo=0):
    hi = 65535 if lo == 0 else 2 ** 31 - 1
    try:
        ok = int(v) == v and lo <= int(v) <= hi
    except (TypeError, ValueError, OverflowError):       # (a NaN, an infinity, not a number)
        ok = False
    if not ok:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    return int(v)


def _ctg_params(xy_resolution, inflation_radius, density_threshold, include_negative, unknown, base, soft_weight, rough_weight,
                roughness_range):
    """the keyword arguments of DeviceMaps.cost_to_go -> (GvomCtgParams, flags); ValueError for what the library would refuse"""
    P = GvomCtgParams()
    P.density_threshold = _clearance_threshold(density_threshold)
    try:
        P.inflation_cells2 = _clearance_cap(inflation_radius, xy_resolution)
    except ValueError as e:
        raise ValueError(str(e).replace("max_distance", "inflation_radius"))
    flags = 0 if include_negative else _CTG_NO_NEGATIVE
    if unknown == "blocked":
        flags |= _CTG_UNKNOWN_BLOCKS
    elif unknown != "free":
        if isinstance(unknown, str):
            raise ValueError('unknown must be "free", "blocked" or an integer cost in 0 .. 65535, got %r' % (unknown,))
        P.unknown_cost = _ctg_weight("unknown", unknown)
    P.base = _ctg_weight("base", base, 1)
    P.soft_weight = _ctg_weight("soft_weight", soft_weight)
    P.rough_weight = _ctg_weight("rough_weight", rough_weight)
    if P.rough_weight:
        if roughness_range is None or len(roughness_range) != 2:
            raise ValueError("rough_weight > 0 needs roughness_range = (min, max)")
        lo, hi = float(roughness_range[0]), float(roughness_range[1])
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise ValueError("roughness_range must be finite with max > min, got %r" % (roughness_range,))
        P.min_roughness, P.max_roughness = lo, hi
    return P, flags


class DeviceCostField(_ProductView):
    """The result of DeviceMaps.cost_to_go() / Gvom.cost_to_go_of() / cost_to_go_of_device(): `.cost` int32 [xy, xy], the cheapest
    way from each cell to a goal (CTG_UNREACHED where there is none), `.direction` uint8 [xy, xy], the first step of it (code k
    = CTG_STEPS[k]; CTG_GOAL at a goal, CTG_NONE where unreached, CTG_UNSETTLED only in a field that is not final) and
    `.cell_cost` uint16 [xy, xy], the cost map the solver used (0 = blocked) -- three DeviceArrays of one product, [x, y]-indexed
    with strides (1, xy) like a DeviceMap.  `.converged`, `.rounds`, `.reached` (cells with a finite cost) and `.goals_seeded` (goals
    on unblocked cells) describe the solve; `.origin` is the window corner in world metres.  A snapshot: later scans and combines do not change it.  copy_to_host() returns (cost,
    direction, cell_cost) as Fortran-ordered numpy [x, y]."""

    def __init__(self, hold, info, origin=(0.0, 0.0)):
        _ProductView.__init__(self, hold)
        self.cost, self.direction, self.cell_cost = DeviceArray(hold, 0), DeviceArray(hold, 1), DeviceArray(hold, 2)
        self.converged, self.rounds, self.reached, self.goals_seeded = bool(info[0]), int(info[1]), int(info[2]), int(info[3])
        self.origin = np.array(origin, np.float64)          # the window corner in world metres (x, y[, z]): what score_rollouts places poses with
        self._host = None

    def score_rollouts(self, poses):
        """Scores K candidate trajectories against this field with the mapper's footprint table (Gvom.set_footprint): per pose the
        maximum of `.cell_cost` under the footprint turned to the pose's heading (0 where it touches a blocked cell or leaves the
        window), per rollout where it first collides, the cost up to there and `.cost` under the last free pose -- a DeviceRollouts,
        computed on the GPU behind the solve; no host wait once the poses are up.  poses: (K, T, 3) = (x, y, yaw) in world metres
        and radians, ROUNDED TO float32.  include/gvom_hip.h "rollout scoring" has the definition."""
        g = self._hold._owner
        a = _rollout_poses(poses)
        return g._score_rollouts(self.product_id, None, None, _ptr(a), a.shape[0], a.shape[1], 0, self.origin)

    def copy_to_host(self):
        return self.cost.copy_to_host(), self.direction.copy_to_host(), self.cell_cost.copy_to_host()

    def pose_field(self, goals, goals_in_cells=False, max_cost=None, max_rounds=0, attitude=None, attitude_blocks=_ATTITUDE_BLOCKS, tilt_weight=0,
                   body=None, body_blocks=_BODY_BLOCKS, squeeze_weight=0):
        """The heading-aware navigation function of this field's `.cell_cost` under the mapper's footprint table (Gvom.set_footprint;
        build THIS field without inflation: the footprint does that, per heading) and primitive table (Gvom.set_primitives): from
        every state (x, y, heading) the cheapest drive to a goal state that the primitives allow -- a DevicePoseField, computed on the
        GPU behind the solve that wrote this field.  The call waits for it.  goals: (G, 2) = (x, y) seeds every heading of the cell,
        (G, 3) = (x, y, yaw) only the heading rint(yaw * H / 2 pi) mod H (float32, the rollouts' rule); world metres -- or window
        cells with goals_in_cells=True; the yaw is radians either way.  A goal outside the window raises ValueError; a goal state
        the footprint blocks seeds nothing.  max_cost, max_rounds: as cost_to_go().  attitude: a DeviceAttitudeVolume of the same
        headings and window -- a state whose status is one of attitude_blocks (ATTITUDE_* codes) is
        blocked, every other state costs tilt_weight (0 .. 255) times its tilt more, at most 65535; without one
        the field is what it always was.  body: a DeviceBodyVolume of the same headings and window -- behind the attitude volume, a
        state whose status is one of body_blocks (BODY_* codes; by default a collision and a body outside the field's box: an unknown
        clearance is not a free one) is blocked, every other state costs squeeze_weight (0 .. 255) times its squeeze more.
        include/gvom_hip.h "pose fields", "attitude volumes" and "body volumes" have the definition."""
        g = self._hold._owner
        H = g._pose_headings()
        cells = _pose_goals(goals, g.xy_size, H, None if goals_in_cells else (g.xy_resolution, self.origin))
        return g._pose_field(self.product_id, None, 0, cells, _ctg_max_cost(max_cost), _ctg_max_rounds(max_rounds), self.origin,
                             _pose_attitude(attitude, attitude_blocks, tilt_weight), _pose_body(body, body_blocks, squeeze_weight))

    def frontiers(self, device_maps, min_cells=4, max_clusters=1024):
        """Where to explore next: the cells of this field that can be driven on (`.cell_cost` > 0), have been seen (`visibility` of
        device_maps, a DeviceMaps, > 0), can be reached (`.cost` < CTG_UNREACHED: seed the field AT the vehicle, the graph is
        undirected) and border never-seen ground, clustered under 8-connectivity on the GPU -- a DeviceFrontiers.  Clusters of fewer
        than min_cells cells are dropped; the rows of at most max_clusters clusters are kept, in ascending order of their least
        cell index.  The call waits for the labelling.  include/gvom_hip.h "frontier extraction" has the definition."""
        g = self._hold._owner
        if not isinstance(device_maps, DeviceMaps):
            raise ValueError("frontiers takes the DeviceMaps whose visibility it reads, got %r" % (type(device_maps).__name__,))
        return g._frontiers(self.product_id, device_maps.set_id, None, None, None, 0, min_cells, max_clusters, self.origin)

    def path_from(self, cell):
        """The cells from `cell` = (x, y) to a goal, both included, following `.direction` on a host copy (made once); None where
        the cell is unreached.  RuntimeError on CTG_UNSETTLED (a field that stopped before it converged)."""
        if self._host is None:
            self._host = self.direction.copy_to_host()
        d = self._host
        x, y = int(cell[0]), int(cell[1])
        if not (0 <= x < d.shape[0] and 0 <= y < d.shape[1]):
            raise ValueError("cell (%d, %d) lies outside the window" % (x, y))
        path = [(x, y)]
        for _ in range(d.size):
            k = int(d[x, y])
            if k == CTG_GOAL:
                return path
            if k == CTG_NONE:
                return None
            if k >= 8:
                raise RuntimeError("cell (%d, %d) is unsettled: the field stopped before it converged" % (x, y))
            x, y = x + CTG_STEPS[k][0], y + CTG_STEPS[k][1]
            path.append((x, y))
        raise RuntimeError("the directions do not lead to a goal")


# ---- rollout scoring (Gvom.set_footprint, DeviceCostField.score_rollouts and friends; include/gvom_hip.h "rollout scoring") ----
ROLLOUT_CLEAR, ROLLOUT_COLLISION, ROLLOUT_LEFT_WINDOW, ROLLOUT_INVALID = range(4)   # GVOM_ROLLOUT_*: summary[:, 0]
ROLLOUT_MAX_T = 4096
ROLLOUT_MAX_POSES = 1 << 26
FOOTPRINT_MAX_HEADINGS = 1024
FOOTPRINT_MAX_CELLS = 16384               # per heading
FOOTPRINT_MAX_TABLE = 1 << 22             # offsets of all headings together


def _box_distance(px, py, hx, hy):
    """distance of the points (px, py) from the axis-aligned box [-hx, hx] x [-hy, hy]"""
    return np.hypot(np.maximum(np.abs(px) - hx, 0.0), np.maximum(np.abs(py) - hy, 0.0))


def _footprint_table(masks, n):
    """boolean masks [H][dy + n][dx + n] -> (start int32 [H + 1], offsets int16 [total, 2]), the cells of a heading row by row"""
    start, offs = [0], []
    for m in masks:
        iy, ix = np.nonzero(m)                                          # (row-major: dy ascending, then dx)
        if iy.size < 1 or iy.size > FOOTPRINT_MAX_CELLS:
            raise ValueError("a footprint heading must have between 1 and %d cells, got %d" % (FOOTPRINT_MAX_CELLS, iy.size))
        offs.append(np.stack([ix - n, iy - n], axis=1))
        start.append(start[-1] + iy.size)
    if start[-1] > FOOTPRINT_MAX_TABLE:
        raise ValueError("a footprint table holds at most 2**22 offsets, got %d" % start[-1])
    return np.array(start, np.int32), np.ascontiguousarray(np.concatenate(offs), dtype=np.int16)


def rectangle_footprint(front, rear, half_width, xy_resolution, headings=64, margin=0.0):
    """The footprint table (start, offsets) of a rectangular vehicle for Gvom.set_footprint: heading h of `headings` turns the
    rectangle [-rear, front] x [-half_width, half_width] (metres, x forward) by 2 pi h / headings.  The cell offset (dx, dy)
    belongs to a heading iff the turned rectangle, grown by `margin` metres all round, meets the OPEN square of side 2 *
    xy_resolution centred at (dx, dy) * xy_resolution -- every cell the footprint can overlap wherever inside its cell the pose
    lies: the mask is conservative, and no cell of it is further than xy_resolution * sqrt(2) + margin from the rectangle.  Pure
    numpy in float64; sines and cosines are exact at quarter turns."""
    front, rear, hw, res, margin = float(front), float(rear), float(half_width), float(xy_resolution), float(margin)
    H = int(headings)
    if H != headings or not 1 <= H <= FOOTPRINT_MAX_HEADINGS:
        raise ValueError("headings must be an integer in 1 .. %d, got %r" % (FOOTPRINT_MAX_HEADINGS, headings))
    if not (math.isfinite(front) and math.isfinite(rear) and math.isfinite(hw) and front + rear >= 0 and hw >= 0):
        raise ValueError("front + rear and half_width must be finite and >= 0, got %r, %r, %r" % (front, rear, half_width))
    if not (math.isfinite(res) and res > 0):
        raise ValueError("xy_resolution must be a length > 0, got %r" % (xy_resolution,))
    if not (math.isfinite(margin) and margin >= 0):
        raise ValueError("margin must be a distance >= 0, got %r" % (margin,))
    n = int(math.ceil((math.hypot(max(abs(front), abs(rear)), hw) + margin) / res)) + 2
    if n > 32767:
        raise ValueError("the footprint reaches further than 32767 cells")
    if (2 * n + 1) ** 2 > 64 * FOOTPRINT_MAX_CELLS:
        raise ValueError("the footprint covers more than %d cells" % FOOTPRINT_MAX_CELLS)
    g = np.arange(-n, n + 1, dtype=np.float64) * res
    px, py = np.meshgrid(g, g)                                          # [dy + n][dx + n]: the squares' centres
    mx, hx = 0.5 * (front - rear), 0.5 * (front + rear)                 # the rectangle in its own frame: centre (mx, 0), half sizes (hx, hw)
    quarter = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
    masks = []
    for h in range(H):
        if (4 * h) % H == 0:
            c, s = quarter[(4 * h) // H]
        else:
            a = 2.0 * math.pi * h / H
            c, s = math.cos(a), math.sin(a)
        # corners in the world frame (body (bx, by) -> (c bx - s by, s bx + c by))
        body = [(front, hw), (front, -hw), (-rear, -hw), (-rear, hw)]
        cwx = np.array([c * bx - s * by for bx, by in body])
        cwy = np.array([s * bx + c * by for bx, by in body])
        # separating axes: the square's two (world x, y) and the rectangle's two (u = (c, s), v = (-s, c)); the square is open
        pu, pv = c * px + s * py, -s * px + c * py
        r = res * (abs(c) + abs(s))                                     # the square's half extent along u and along v
        hit = ((cwx.max() > px - res) & (px + res > cwx.min()) & (cwy.max() > py - res) & (py + res > cwy.min()) &
               (front > pu - r) & (pu + r > -rear) & (hw > pv - r) & (pv + r > -hw))
        if margin > 0.0:
            # apart, two convex polygons are closest at a corner of one of them: the rectangle's corners against the square (a box
            # in the world frame), the square's corners against the rectangle (a box in its own)
            d = np.full(px.shape, np.inf)
            for k in range(4):
                d = np.minimum(d, _box_distance(cwx[k] - px, cwy[k] - py, res, res))
            for sx, sy in ((1, 1), (1, -1), (-1, -1), (-1, 1)):
                qx, qy = px + sx * res, py + sy * res
                d = np.minimum(d, _box_distance(c * qx + s * qy - mx, -s * qx + c * qy, hx, hw))
            hit |= d < margin
        masks.append(hit)
    return _footprint_table(masks, n)


def disc_footprint(radius, xy_resolution):
    """The footprint table (start, offsets) of a disc of `radius` metres, one heading: the offsets whose open square of side 2 *
    xy_resolution the disc meets (the same conservative rule as rectangle_footprint)."""
    radius, res = float(radius), float(xy_resolution)
    if not (math.isfinite(radius) and radius >= 0):
        raise ValueError("radius must be a distance >= 0, got %r" % (radius,))
    if not (math.isfinite(res) and res > 0):
        raise ValueError("xy_resolution must be a length > 0, got %r" % (xy_resolution,))
    n = int(math.ceil(radius / res)) + 2
    if n > 32767 or (2 * n + 1) ** 2 > 64 * FOOTPRINT_MAX_CELLS:
        raise ValueError("the footprint covers more than %d cells" % FOOTPRINT_MAX_CELLS)
    g = np.arange(-n, n + 1, dtype=np.float64) * res
    px, py = np.meshgrid(g, g)
    hit = (_box_distance(px, py, res, res) < radius) | ((px == 0.0) & (py == 0.0))
    return _footprint_table([hit], n)


def _footprint_arrays(table):
    """(start, offsets) as the library takes them: C-contiguous int32 [H + 1] and int16 [total, 2]; ValueError for what it would refuse"""
    try:
        start, offsets = table
    except (TypeError, ValueError):
        raise ValueError("a footprint table is a pair (start, offsets)")
    st, of = np.asarray(start), np.asarray(offsets)
    if st.ndim != 1 or not 2 <= st.shape[0] <= FOOTPRINT_MAX_HEADINGS + 1 or st.dtype.kind not in "iu":
        raise ValueError("start must be integers of shape (H + 1,) with 1 <= H <= %d, got %r %s" % (FOOTPRINT_MAX_HEADINGS, st.shape, st.dtype))
    if of.ndim != 2 or of.shape[1] != 2 or of.dtype.kind not in "iu":
        raise ValueError("offsets must be integers of shape (total, 2), got %r %s" % (of.shape, of.dtype))
    st = st.astype(np.int64)
    m = np.diff(st)
    if st[0] != 0 or (m < 1).any() or (m > FOOTPRINT_MAX_CELLS).any():
        raise ValueError("start must begin at 0 and give every heading between 1 and %d cells" % FOOTPRINT_MAX_CELLS)
    if st[-1] != of.shape[0]:
        raise ValueError("start[-1] = %d, but there are %d offsets" % (st[-1], of.shape[0]))
    if st[-1] > FOOTPRINT_MAX_TABLE:
        raise ValueError("a footprint table holds at most 2**22 offsets, got %d" % st[-1])
    if of.size and (of.min() < -32768 or of.max() > 32767):
        raise ValueError("offsets must fit int16")
    return np.ascontiguousarray(st, dtype=np.int32), np.ascontiguousarray(of, dtype=np.int16)


def _rollout_shape(K, T):
    try:
        ok = int(K) == K and int(T) == T
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not 1 <= int(T) <= ROLLOUT_MAX_T or int(K) < 1:
        raise ValueError("rollouts need K >= 1 trajectories of 1 <= T <= %d poses, got K = %r, T = %r" % (ROLLOUT_MAX_T, K, T))
    if int(K) * int(T) > ROLLOUT_MAX_POSES:
        raise ValueError("at most 2**26 poses per call, got %d x %d" % (int(K), int(T)))
    return int(K), int(T)


def _rollout_poses(poses):
    """poses -> C-contiguous float32 (K, T, 3)"""
    a = np.asarray(poses)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("poses must have shape (K, T, 3) = (x, y, yaw), got %r" % (a.shape,))
    if a.dtype.kind not in "iuf":
        raise ValueError("poses must be numbers, got dtype %s" % a.dtype)
    _rollout_shape(a.shape[0], a.shape[1])
    return np.ascontiguousarray(a, dtype=np.float32)


def _rollout_origin(origin, xy_resolution):
    """the window corner in world metres -> round(origin / xy_resolution) per axis, as world_to_cells places points"""
    o = np.asarray(origin, np.float64).reshape(-1)
    if o.shape[0] < 2 or not np.isfinite(o[:2]).all():
        raise ValueError("origin must be (x, y) in finite world metres, got %r" % (origin,))
    c = np.round(o[:2] / float(xy_resolution))
    if (np.abs(c) > 2.0 ** 40).any():
        raise ValueError("origin lies beyond 2**40 cells: %r" % (origin,))
    return (_I64 * 2)(int(c[0]), int(c[1]))


class DeviceRollouts(_ProductView):
    """The result of DeviceCostField.score_rollouts() / Gvom.score_rollouts_of() / score_rollouts_of_device(): `.summary` int32
    [K, 4] -- per rollout {status (ROLLOUT_*), first blocked pose (T: none), path cost (the pose costs in front of it, summed),
    terminal (the cost-to-go under the last free pose; CTG_UNREACHED without one)} -- and `.pose_cost` uint16 [K, T], the maximum
    cell cost under the footprint at each pose (0 = blocked): two DeviceArrays of one product, row i = rollout i.  A snapshot: later
    scans, combines and set_footprint calls do not change it.  copy_to_host() returns (summary, pose_cost) as numpy."""

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.summary, self.pose_cost = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.summary.copy_to_host(), self.pose_cost.copy_to_host()


# ---- terrain attitude scoring (Gvom.set_chassis, DeviceMaps.score_attitude and friends; include/gvom_hip.h "terrain attitude scoring") ----
ATTITUDE_OK, ATTITUDE_PITCH, ATTITUDE_ROLL, ATTITUDE_BELLY, ATTITUDE_UNKNOWN_GROUND, ATTITUDE_LEFT_WINDOW, ATTITUDE_INVALID = range(7)   # GVOM_ATTITUDE_*
_ATTITUDE_INFERRED_GROUND = 1             # flags


class GvomChassis(ctypes.Structure):
    """gvom_chassis_t"""
    _fields_ = [("front_axle", ctypes.c_double), ("rear_axle", ctypes.c_double), ("track", ctypes.c_double), ("belly_height", ctypes.c_double),
                ("max_pitch", ctypes.c_float), ("max_roll", ctypes.c_float), ("min_clearance", ctypes.c_float)]


def _chassis_angle(name, a):
    """a limit angle in radians -> its tangent as float32; None: no limit (+inf)"""
    if a is None:
        return np.float32(np.inf)
    a = float(a)
    if not 0.0 <= a < math.pi / 2:
        raise ValueError("%s must be None or an angle in [0, pi / 2) radians, got %r" % (name, a))
    return np.float32(np.tan(a))


def chassis(front_axle, rear_axle, track, belly_height, max_pitch=None, max_roll=None, min_clearance=None):
    """The chassis for Gvom.set_chassis (a GvomChassis): the axles' body x in metres (x forward, front_axle > rear_axle), the track
    width, the belly's height above the wheels' contact plane; max_pitch / max_roll: limit angles in radians, stored as
    np.float32(np.tan(a)); min_clearance: the least belly clearance in metres.  None: no limit."""
    fa, ra, tr, bh = float(front_axle), float(rear_axle), float(track), float(belly_height)
    if not (math.isfinite(fa) and math.isfinite(ra) and math.isfinite(tr) and math.isfinite(bh)):
        raise ValueError("front_axle, rear_axle, track and belly_height must be finite, got %r, %r, %r, %r" % (front_axle, rear_axle, track, belly_height))
    if not fa > ra:
        raise ValueError("front_axle must lie in front of rear_axle, got %r <= %r" % (front_axle, rear_axle))
    if not tr > 0:
        raise ValueError("track must be a width > 0, got %r" % (track,))
    c = GvomChassis()
    c.front_axle, c.rear_axle, c.track, c.belly_height = fa, ra, tr, bh
    c.max_pitch, c.max_roll = _chassis_angle("max_pitch", max_pitch), _chassis_angle("max_roll", max_roll)
    mc = -math.inf if min_clearance is None else float(min_clearance)
    if mc != mc:
        raise ValueError("min_clearance must be None or a height in metres, got %r" % (min_clearance,))
    c.min_clearance = np.float32(mc)
    return c


def heading_cos_sin(headings):
    """float64 [H, 2] = (cos, sin) of 2 pi k / H, exact at quarter turns like rectangle_footprint's"""
    H = int(headings)
    a = 2.0 * np.pi * np.arange(H, dtype=np.float64) / H
    cs = np.stack([np.cos(a), np.sin(a)], axis=1)
    quarter = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))
    for k in range(H):
        if (4 * k) % H == 0:
            cs[k] = quarter[(4 * k) // H]
    return np.ascontiguousarray(cs)


class DeviceAttitude(_ProductView):
    """The result of DeviceMaps.score_attitude() / Gvom.score_attitude_of() / score_attitude_of_device(): `.summary` int32 [K, 5] --
    per rollout {status (ATTITUDE_*), first bad pose (T: none), the poses of the steepest pitch, the steepest roll and the lowest
    belly in front of it (-1 without one)} --, `.attitude` float32 [K, T, 3] {pitch tangent (nose up positive), roll tangent (left
    side up positive), belly clearance in metres} and `.status` uint8 [K, T]: three DeviceArrays of one product, row i = rollout i.
    A snapshot: later scans, combines, set_footprint and set_chassis calls do not change it.  copy_to_host() returns (summary,
    attitude, status) as numpy."""

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.summary, self.attitude, self.status = DeviceArray(hold, 0), DeviceArray(hold, 1), DeviceArray(hold, 2)

    def copy_to_host(self):
        return self.summary.copy_to_host(), self.attitude.copy_to_host(), self.status.copy_to_host()


# ---- body clearance scoring (Gvom.set_body, DeviceDistanceField.score_body and friends; include/gvom_hip.h "body clearance scoring") ----
BODY_OK, BODY_COLLISION, BODY_LEFT_BOX, BODY_UNKNOWN_GROUND, BODY_LEFT_WINDOW, BODY_INVALID = range(6)   # GVOM_BODY_*
BODY_MAX_SPHERES = 256


def _body_spheres(spheres):
    """spheres -> C-contiguous float32 (S, 4) = (bx, by, bz, r)"""
    a = np.asarray(spheres)
    if a.ndim != 2 or a.shape[1] != 4 or not 1 <= a.shape[0] <= BODY_MAX_SPHERES:
        raise ValueError("spheres must have shape (S, 4) = (bx, by, bz, r) with 1 <= S <= %d, got %r" % (BODY_MAX_SPHERES, a.shape))
    if a.dtype.kind not in "iuf":
        raise ValueError("spheres must be numbers, got dtype %s" % a.dtype)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all() or (a[:, 3] < 0).any():
        raise ValueError("spheres must be finite with radii >= 0")
    return a


def box_spheres(x0, x1, half_width, z0, z1, radius):
    """A body for Gvom.set_body: float32 (S, 4) spheres of one radius on a lattice whose union covers the box x0 .. x1 (body x,
    forward) by -half_width .. +half_width (body y) by z0 .. z1 (height above the wheels' contact plane).  Per axis the side is cut
    into the fewest equal parts of at most radius * 2 / sqrt(3) -- the side of the cube inscribed in a sphere -- and a centre stands
    in the middle of each part: the cuboids around the centres tile the box and every point of it lies within `radius` of a centre.
    The union reaches radius - part / 2 beyond a face, along the axis through a centre: at most `radius`, and at least
    radius * (1 - 1 / sqrt(3)) = 0.42 radius.  ValueError where the lattice would need more than 256 spheres: choose a larger
    radius."""
    lo = np.array([x0, -float(half_width), z0], np.float64)
    hi = np.array([x1, float(half_width), z1], np.float64)
    r = float(radius)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all() and math.isfinite(r) and r > 0):
        raise ValueError("box_spheres needs x0 < x1, half_width > 0, z0 < z1 and radius > 0, all finite")
    pitch = r * 2.0 / math.sqrt(3.0)
    n = np.maximum(1, np.ceil((hi - lo) / pitch - 1e-12)).astype(np.int64)
    if int(n.prod()) > BODY_MAX_SPHERES:
        raise ValueError("a box of %r m at radius %r needs %d spheres, more than %d" % ((hi - lo).tolist(), r, int(n.prod()), BODY_MAX_SPHERES))
    axes = [l + (np.arange(k, dtype=np.float64) + 0.5) * ((h - l) / k) for l, h, k in zip(lo, hi, n)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([g, np.full((g.shape[0], 1), r)], axis=1), dtype=np.float32)


class DeviceBodyClearance(_OnePartDLPack, _ProductView):
    """The result of DeviceDistanceField.score_body() / score_body_of() / Gvom.score_body_of() / score_body_of_device(): `.summary`
    int32 [K, 4] -- per rollout {status (BODY_*), first bad pose (T: none), the pose of the least clearance in front of it and that
    pose's tightest sphere (-1 without one)} --, `.clearance` float32 [K, T] -- the least of (field at the sphere's voxel - radius)
    over the body, metres, +inf where nothing is within the field's cap -- and `.status` uint8 [K, T, 2] {BODY_*, tightest sphere}:
    three DeviceArrays of one product, row i = rollout i.  A snapshot: later scans, combines, integrates, set_body and set_chassis
    calls do not change it.  DLPack hands over `.clearance`; copy_to_host() returns (summary, clearance, status) as numpy."""
    _dlpack_part = "clearance"

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.summary, self.clearance, self.status = DeviceArray(hold, 0), DeviceArray(hold, 1), DeviceArray(hold, 2)

    def copy_to_host(self):
        return self.summary.copy_to_host(), self.clearance.copy_to_host(), self.status.copy_to_host()


class _AttitudePlanes(DeviceArray):
    """One [H, xy, xy] volume of an attitude volume or a body volume, indexed [h, x, y] with strides (xy*xy, 1, xy) like a pose field's volumes.
    copy_to_host() returns numpy of the same indexing (a transposed view of the [h][y][x] copy)."""

    def copy_to_host(self):
        g = self._hold._owner
        raw = np.empty((self.shape[0], self.shape[2], self.shape[1]), self.dtype)
        g._check(g._lib.gvom_device_product_copy(g._h, self.product_id, self._part, ctypes.c_void_p(raw.ctypes.data)))
        return raw.transpose(0, 2, 1)


class DeviceAttitudeVolume(_OnePartDLPack, _ProductView):
    """The result of DeviceMaps.attitude_volume() / Gvom.attitude_volume_of() / attitude_volume_of_device(): `.status` uint8
    [H, xy, xy] -- ATTITUDE_* of the vehicle standing in the centre of cell (x, y) at heading h -- and `.tilt` uint8 [H, xy, xy] -- how
    much of the nearer of the pitch and the roll limit the state uses, 0 .. 100 percent (0 on unknown ground and outside the window)
    --, both indexed [h, x, y], and `.counts` int32 [8]: the states per status code 0 .. 6, then H.  Three DeviceArrays of one
    product; `__dlpack__` hands out `.status`.  A snapshot: later scans, combines, set_footprint and set_chassis calls do not change
    it.  copy_to_host() returns (status, tilt, counts) as numpy."""
    _dlpack_part = "status"

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.status, self.tilt, self.counts = _AttitudePlanes(hold, 0), _AttitudePlanes(hold, 1), DeviceArray(hold, 2)

    def copy_to_host(self):
        return self.status.copy_to_host(), self.tilt.copy_to_host(), self.counts.copy_to_host()


def _pose_volume(volume, blocks, weight, word, cls, maker, top, weight_word):
    """the keywords of one volume of the pose_field calls (word = "attitude" or "body") -> None, or (the volume's product id, block
    mask, weight)"""
    if volume is None:
        if weight != 0:
            raise ValueError("%s needs %s %s volume (%s=...)" % (weight_word, "an" if word[0] in "aeiou" else "a", word, word))
        return None
    if not isinstance(volume, cls):
        raise TypeError("%s must be a %s (%s), got %r" % (word, cls.__name__, maker, type(volume).__name__))
    mask = 0
    try:
        for b in blocks:
            if isinstance(b, bool) or int(b) != b or not 0 <= int(b) <= top:
                raise ValueError
            mask |= 1 << int(b)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s_blocks must be a sequence of %s_* codes 0 .. %d, got %r" % (word, word.upper(), top, blocks))
    try:
        ok = not isinstance(weight, bool) and int(weight) == weight and 0 <= int(weight) <= 255
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s must be an integer in 0 .. 255, got %r" % (weight_word, weight))
    return volume.product_id, mask, int(weight)


def _pose_attitude(attitude, attitude_blocks, tilt_weight):
    return _pose_volume(attitude, attitude_blocks, tilt_weight, "attitude", DeviceAttitudeVolume, "DeviceMaps.attitude_volume()", 6, "tilt_weight")


def _pose_body(body, body_blocks, squeeze_weight):
    return _pose_volume(body, body_blocks, squeeze_weight, "body", DeviceBodyVolume, "DeviceDistanceField.body_volume()", 5, "squeeze_weight")


class DeviceBodyVolume(_OnePartDLPack, _ProductView):
    """The result of DeviceDistanceField.body_volume() / body_volume_of() / Gvom.body_volume_of() / body_volume_of_device(): `.status`
    uint8 [H, xy, xy] -- BODY_* of the sphere body (Gvom.set_body) with the vehicle standing in the centre of cell (x, y) at heading h
    --, `.squeeze` uint8 [H, xy, xy] -- how much of the band between soft_margin and min_margin the state has used up, 0 .. 100 percent
    (0 outside the window, on unknown ground and outside the field's box) -- and `.clearance` float32 [H, xy, xy] -- the least of
    (field at the sphere's voxel - radius) over the body, metres, +inf where nothing is within the field's cap, 0 in those three cases
    --, all indexed [h, x, y], and `.counts` int32 [8]: the states per status code 0 .. 5, then H and S.  Four DeviceArrays of one
    product; `__dlpack__` hands out `.status`.  A snapshot: later scans, combines, integrates, set_footprint, set_chassis and set_body
    calls do not change it.  copy_to_host() returns (status, squeeze, clearance, counts) as numpy."""
    _dlpack_part = "status"

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.status, self.squeeze, self.clearance = _AttitudePlanes(hold, 0), _AttitudePlanes(hold, 1), _AttitudePlanes(hold, 2)
        self.counts = DeviceArray(hold, 3)

    def copy_to_host(self):
        return self.status.copy_to_host(), self.squeeze.copy_to_host(), self.clearance.copy_to_host(), self.counts.copy_to_host()


def _body_margins(min_margin, soft_margin):
    """the margins of the score_body and body_volume calls -> (min_margin, soft_margin) as float32-exact Python floats; soft_margin None: min_margin"""
    with np.errstate(over="ignore"):
        mm = float(np.float32(min_margin))
        sm = mm if soft_margin is None else float(np.float32(soft_margin))
    if not math.isfinite(mm):
        raise ValueError("min_margin must be a finite distance in metres, got %r" % (min_margin,))
    if not math.isfinite(sm):
        raise ValueError("soft_margin must be a finite distance in metres, got %r" % (soft_margin,))
    if sm < mm:
        raise ValueError("soft_margin must not be less than min_margin, got %r < %r" % (soft_margin, min_margin))
    return mm, sm


# ---- frontier extraction (DeviceCostField.frontiers, Gvom.frontiers_of and friends; include/gvom_hip.h "frontier extraction") ----
FRONTIER_MAX_CLUSTERS = 1 << 20
FRONTIER_NONE, FRONTIER_SMALL = -1, -2    # cluster map: no frontier cell; a frontier cell of a cluster below min_cells


def _frontier_limits(min_cells, max_clusters):
    try:
        ok = int(min_cells) == min_cells and int(max_clusters) == max_clusters
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not 1 <= int(min_cells) < 2 ** 31:
        raise ValueError("min_cells must be an integer >= 1, got %r" % (min_cells,))
    if not 1 <= int(max_clusters) <= FRONTIER_MAX_CLUSTERS:
        raise ValueError("max_clusters must be an integer in 1 .. 2**20, got %r" % (max_clusters,))
    return int(min_cells), int(max_clusters)


class DeviceFrontiers(_ProductView):
    """The result of DeviceCostField.frontiers() / Gvom.frontiers_of() / frontiers_of_device(): `.clusters` int32 [cap, 8] -- per kept
    cluster, in ascending label order, {label (its least cell index y * xy + x), cells, min x, min y, max x, max y, best cell (the
    member with the least cost to go, on ties the lowest index), best D} --, `.sums` int64 [cap, 2] {sum x, sum y} (the centroid is
    theirs divided by cells), `.cluster_map` int32 [xy, xy], [x, y]-indexed with strides (1, xy) like a DeviceMap (the cell's cluster
    rank, FRONTIER_NONE where it is no frontier cell, FRONTIER_SMALL where its cluster is below min_cells) and `.counts` int32 [4]
    {kept clusters, frontier cells, frontier cells in kept clusters, cap}: four DeviceArrays of one product.  Rows from
    min(n_clusters, cap) on are zero.  `.rounds`, `.n_clusters` (kept clusters, also those beyond cap), `.frontier_cells` and
    `.dropped` (clusters below min_cells) describe the call; `.origin` is the window corner in world metres.  A snapshot: later
    scans, combines and solves do not change it.  copy_to_host() returns (clusters, sums, cluster_map, counts) as numpy."""

    def __init__(self, hold, info, xy_resolution, origin=(0.0, 0.0)):
        _ProductView.__init__(self, hold)
        self.clusters, self.sums, self.cluster_map, self.counts = (DeviceArray(hold, k) for k in range(4))
        self.rounds, self.n_clusters, self.frontier_cells, self.dropped = int(info[0]), int(info[1]), int(info[2]), int(info[3])
        self.origin = np.array(origin, np.float64)
        self._res = float(xy_resolution)

    def copy_to_host(self):
        return self.clusters.copy_to_host(), self.sums.copy_to_host(), self.cluster_map.copy_to_host(), self.counts.copy_to_host()

    def goals(self, order="cost"):
        """Exploration goals on the host: (best, centroid, rows) -- float64 [n, 2] world metres (x, y) of the centre of each kept
        cluster's best cell and of its centroid, and the int64 [n] rows of `.clusters` they come from; n = min(n_clusters, cap).
        order="cost": the cheapest to reach first (best D ascending, then label); "size": the largest first (cells descending, then
        label)."""
        if order not in ("cost", "size"):
            raise ValueError('order must be "cost" or "size", got %r' % (order,))
        n = min(self.n_clusters, self.clusters.shape[0])
        rows, sums = self.clusters.copy_to_host()[:n].astype(np.int64), self.sums.copy_to_host()[:n]
        xy = self.cluster_map.shape[0]
        key = rows[:, 7] if order == "cost" else -rows[:, 1]
        pick = np.lexsort((rows[:, 0], key))
        oc = np.round(self.origin[:2] / self._res)
        best = np.stack([rows[:, 6] % xy, rows[:, 6] // xy], axis=1).astype(np.float64)
        centroid = sums.astype(np.float64) / np.maximum(rows[:, 1:2], 1)
        return ((best + oc + 0.5) * self._res)[pick], ((centroid + oc + 0.5) * self._res)[pick], pick


# ---- viewpoint scoring (Gvom.score_viewpoints and friends; include/gvom_hip.h "viewpoint scoring") ----
VIEWPOINT_MAX_POSES = 65536
VIEWPOINT_MAX_BEAMS = 1 << 22


def _viewpoint_poses(poses):
    """poses float64 (K, 4, 4), (K, 3, 4), (4, 4) or (3, 4) -> C-contiguous float64 (K, 3, 4): rows 0..2"""
    a = np.asarray(poses)
    if a.dtype != np.float64:
        raise TypeError("poses must be float64, got %s" % a.dtype)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] not in ((4, 4), (3, 4)) or a.shape[0] < 1:
        raise ValueError("poses must have shape (K, 4, 4) or (K, 3, 4) with K >= 1, or be one such matrix, got %r" % (a.shape,))
    return np.ascontiguousarray(a[:, :3, :])


def _viewpoint_options(K, max_range, beam_stride):
    try:
        ok = int(K) == K and not isinstance(K, bool)
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or not 1 <= int(K) <= VIEWPOINT_MAX_POSES:
        raise ValueError("viewpoint scoring needs 1 .. 65536 poses, got K = %r" % (K,))
    try:
        r = float(max_range)
    except (TypeError, ValueError):
        r = float("nan")
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("max_range must be finite and > 0, got %r" % (max_range,))
    try:
        sh, sw = beam_stride
        ok = int(sh) == sh and int(sw) == sw and 1 <= int(sh) < 2 ** 31 and 1 <= int(sw) < 2 ** 31
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("beam_stride must be two integers >= 1 (rows, columns), got %r" % (beam_stride,))
    return int(K), r, int(sh), int(sw)


def viewpoint_poses(points_xyz, yaws, sensor_to_body=None):
    """Candidate sensor poses for Gvom.score_viewpoints: float64 [len(points) * len(yaws), 4, 4], sensor to world.  Pose
    k = i * len(yaws) + j puts the BODY at points_xyz[i] (world metres; with the `best` of DeviceFrontiers.goals() and a sensor height:
    np.column_stack([best, np.full(len(best), z)])) turned by yaws[j] about the vertical: B = [[c, -s, 0, x], [s, c, 0, y],
    [0, 0, 1, z], [0, 0, 0, 1]] with c = math.cos(yaw), s = math.sin(yaw), and is B itself without sensor_to_body, else
    B.dot(sensor_to_body) (numpy's float64 matrix product of the two 4x4; sensor_to_body: the sensor's pose in the body frame).
    INDEX ORDER: the yaw is the fastest index."""
    pts = np.asarray(points_xyz, np.float64)
    if pts.ndim == 1:
        pts = pts[None]
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points_xyz must have shape (n, 3), got %r" % (pts.shape,))
    yw = np.asarray(yaws, np.float64).reshape(-1)
    S = None
    if sensor_to_body is not None:
        S = np.asarray(sensor_to_body, np.float64)
        if S.shape != (4, 4):
            raise ValueError("sensor_to_body must be a 4x4 matrix, got shape %r" % (S.shape,))
    if pts.shape[0] * yw.shape[0] > VIEWPOINT_MAX_POSES:
        raise ValueError("more than 65536 poses: %d" % (pts.shape[0] * yw.shape[0]))
    out = np.empty((pts.shape[0], yw.shape[0], 4, 4), np.float64)
    for i in range(pts.shape[0]):
        for j in range(yw.shape[0]):
            c, s = math.cos(float(yw[j])), math.sin(float(yw[j]))
            B = np.identity(4)
            B[0, 0], B[0, 1], B[1, 0], B[1, 1] = c, -s, s, c
            B[:3, 3] = pts[i]
            out[i, j] = B if S is None else B.dot(S)
    return out.reshape(-1, 4, 4)


class DeviceViewpoints(_ProductView):
    """The result of Gvom.score_viewpoints() / score_viewpoints_device(): `.rows` int32 [K, 8] -- per pose {status of the pose's own
    voxel (RAY_*), gain (DISTINCT never-observed voxels its beams examined), visits (the same with multiplicity), beams that ended
    RAY_OCCUPIED, RAY_CLEAR, RAY_LEFT_WINDOW, RAY_UNKNOWN, RAY_INVALID} -- and `.best` int32 [4] {best index (the lowest of the
    largest gain among the poses whose own voxel is observed free; -1 where there is none), its gain, K, beams per pose}: two
    DeviceArrays of one product, row k = pose k.  `.origin`: the fused map's window origin in voxels when the call was made.  A
    snapshot: later scans and combines do not change it.  copy_to_host() returns (rows, best) as numpy."""

    def __init__(self, hold, origin, poses=None):
        _ProductView.__init__(self, hold)
        self.origin = origin
        self._poses = poses
        self.rows, self.best = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.rows.copy_to_host(), self.best.copy_to_host()

    def best_pose(self):
        """(index, gain, pose) of the best viewpoint -- pose: float64 [3, 4], rows 0..2 of the matrix handed to score_viewpoints()
        (None on the device route, which keeps no host copy) --, or None where no pose lies in an observed-free voxel."""
        k, gain = (int(v) for v in self.best.copy_to_host()[:2])
        if k < 0:
            return None
        return k, gain, (None if self._poses is None else self._poses[k].copy())


# ---- pose fields (Gvom.set_primitives, DeviceCostField.pose_field and friends; include/gvom_hip.h "pose fields") ----
POSE_GOAL = 253                           # GVOM_POSE_GOAL: the action at a seeded state (beside CTG_NONE and CTG_UNSETTLED)
POSE_MAX_HEADINGS = 64
POSE_MAX_REACH = 4                        # |dx|, |dy| of a primitive, in cells
POSE_MAX_PRIMITIVES = 64                  # per heading
POSE_MAX_STATES = 1 << 28                 # headings * xy_size ** 2
_RO_FAR = 100000                          # csrc/gvom_rollouts.h RO_FAR: where pose_states puts a centre that is outside however far


def _primitive_arrays(table):
    """(start, prims) as the library takes them: C-contiguous int32 [H + 1] and int16 [total, 4]; ValueError for what it would refuse"""
    try:
        start, prims = table
    except (TypeError, ValueError):
        raise ValueError("a primitive table is a pair (start, prims)")
    st, pr = np.asarray(start), np.asarray(prims)
    if st.ndim != 1 or not 2 <= st.shape[0] <= POSE_MAX_HEADINGS + 1 or st.dtype.kind not in "iu":
        raise ValueError("start must be integers of shape (H + 1,) with 1 <= H <= %d, got %r %s" % (POSE_MAX_HEADINGS, st.shape, st.dtype))
    if pr.ndim != 2 or pr.shape[1] != 4 or pr.dtype.kind not in "iu":
        raise ValueError("prims must be integers of shape (total, 4) = (dx, dy, h_to, w), got %r %s" % (pr.shape, pr.dtype))
    st, pr = st.astype(np.int64), pr.astype(np.int64)
    H = st.shape[0] - 1
    m = np.diff(st)
    if st[0] != 0 or (m < 0).any() or (m > POSE_MAX_PRIMITIVES).any():
        raise ValueError("start must begin at 0 and give every heading at most %d primitives" % POSE_MAX_PRIMITIVES)
    if st[-1] != pr.shape[0]:
        raise ValueError("start[-1] = %d, but there are %d primitives" % (st[-1], pr.shape[0]))
    own = np.repeat(np.arange(H), m)
    bad = ((np.abs(pr[:, 0]) > POSE_MAX_REACH) | (np.abs(pr[:, 1]) > POSE_MAX_REACH) | (pr[:, 2] < 0) | (pr[:, 2] >= H) | (pr[:, 3] < 1) |
           (pr[:, 3] > 255) | ((pr[:, 0] == 0) & (pr[:, 1] == 0) & (pr[:, 2] == own)))
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError("primitive %d = %r of heading %d is outside the limits: |dx|, |dy| <= %d, 0 <= h_to < %d, 1 <= w <= 255, "
                         "not (0, 0, its own heading)" % (k, tuple(int(v) for v in pr[k]), own[k], POSE_MAX_REACH, H))
    return np.ascontiguousarray(st, dtype=np.int32), np.ascontiguousarray(pr, dtype=np.int16)


def arc_primitives(headings, min_turn_radius, xy_resolution, reach=3, reverse_weight=None):
    """The primitive table (start, prims) of a car-like vehicle for Gvom.set_primitives, by a constructive definition: per heading
    three forward primitives -- straight, left, right, in this order -- each an arc of length l = reach * xy_resolution.  A turn
    changes the heading by k = floor(l / min_turn_radius / (2 pi / headings)) bins, at most headings // 4 (ValueError where k is 0:
    the arc is too short to reach the next heading), that is by phi = k * 2 pi / headings on a radius l / phi >= min_turn_radius.
    The end cell is the rint of the arc's end point in cells (float64); w = max(1, rint(10 * the arc length, in cells, through the
    ROUNDED chord)) -- the chord itself for a straight primitive, chord * (phi / 2) / sin(phi / 2) for a turn.  reverse_weight = r adds
    the three mirrored reverse primitives (straight back, back with the wheels left: the heading turns right, back with the wheels
    right) behind them in the same order, w multiplied by r and clipped to 255.  For headings % 4 == 0 the first quarter is built and
    rotated for the rest: the table is exactly symmetric under quarter turns."""
    H = int(headings)
    if H != headings or not 4 <= H <= POSE_MAX_HEADINGS:
        raise ValueError("headings must be an integer in 4 .. %d, got %r" % (POSE_MAX_HEADINGS, headings))
    res, rad, n = float(xy_resolution), float(min_turn_radius), float(reach)
    if not (math.isfinite(res) and res > 0 and math.isfinite(rad) and rad > 0 and math.isfinite(n) and 0 < n <= POSE_MAX_REACH):
        raise ValueError("arc_primitives needs xy_resolution > 0, min_turn_radius > 0 and 0 < reach <= %d cells" % POSE_MAX_REACH)
    if reverse_weight is not None and not (math.isfinite(float(reverse_weight)) and float(reverse_weight) > 0):
        raise ValueError("reverse_weight must be None or a factor > 0, got %r" % (reverse_weight,))
    length = n * res
    step = 2.0 * math.pi / H
    k = int(math.floor(length / rad / step))
    if k == 0:
        raise ValueError("an arc of %g m on a radius of %g m does not reach the next of %d headings: raise reach or lower headings"
                         % (length, rad, H))
    k = min(k, H // 4)
    phi = k * step
    r = length / phi

    def one(h):
        th = h * step
        c, s = math.cos(th), math.sin(th)
        rows = []
        ends = ((length, 0.0, 0), (r * math.sin(phi), r * (1.0 - math.cos(phi)), k), (r * math.sin(phi), -r * (1.0 - math.cos(phi)), -k))
        for sign, factor in ((1.0, None), (-1.0, reverse_weight)):
            if sign < 0 and reverse_weight is None:
                break
            for ex, ey, dk in ends:
                ex, dk = sign * ex, int(sign) * dk                          # mirrored through the lateral axis: backing up turns the other way
                dx, dy = int(np.rint((c * ex - s * ey) / res)), int(np.rint((s * ex + c * ey) / res))
                chord = math.hypot(dx, dy)
                arc = chord if dk == 0 else chord * (phi / 2.0) / math.sin(phi / 2.0)
                w = max(1, int(np.rint(10.0 * arc)))
                if factor is not None:
                    w = max(1, int(np.rint(w * float(factor))))
                rows.append((dx, dy, (h + dk) % H, min(w, 255)))
        return rows

    per = []
    if H % 4 == 0:
        q = H // 4
        base = [one(h) for h in range(q)]
        for turn in range(4):
            for h in range(q):
                rows = base[h]
                for _ in range(turn):
                    rows = [(-dy, dx, (ht + q) % H, w) for dx, dy, ht, w in rows]
                per.append(rows)
    else:
        per = [one(h) for h in range(H)]
    start = np.concatenate([[0], np.cumsum([len(rows) for rows in per])]).astype(np.int32)
    prims = np.array([row for rows in per for row in rows], np.int16)
    return _primitive_arrays((start, prims))


def pose_states(poses, origin, xy_resolution, H):
    """The states of poses [..., 3] = (x, y, yaw) in world metres and radians, ROUNDED TO float32, with exactly the arithmetic the
    rollout kernels place a pose with (include/gvom_hip.h "rollout scoring", CENTRE / HEADING / INVALID): (states, valid) -- states
    int32 [..., 3] = (cx, cy, h), the centre in window cells of a map whose window corner is at `origin` and the heading bin of H;
    valid bool [...].  A centre may lie outside the window (test it against xy_size); one that is outside however far (a
    non-finite coordinate, |x / xy_resolution| >= 2**30) reads -100000, and a centre is clamped to +-100000.  An invalid pose has
    heading 0.  A torch consumer gathers a DevicePoseField's cost[h, cx, cy] with these as a rollout's terminal cost."""
    p = np.asarray(poses)
    if p.ndim < 1 or p.shape[-1] != 3 or p.dtype.kind not in "iuf":
        raise ValueError("poses must be numbers of shape (..., 3) = (x, y, yaw), got %r %s" % (p.shape, p.dtype))
    H = int(H)
    if H < 1:
        raise ValueError("H must be at least 1")
    p = p.astype(np.float32)
    oc = _rollout_origin(origin, xy_resolution)
    x, y, yaw = p[..., 0], p[..., 1], p[..., 2]
    out = np.zeros(p.shape[:-1] + (3,), np.int32)
    with np.errstate(all="ignore"):
        a = yaw * np.float32(H / 6.283185307179586476925286766559)       # one float32 multiply
        valid = (np.abs(x) < np.inf) & (np.abs(y) < np.inf) & (np.abs(yaw) < np.inf) & (np.abs(a) < np.float32(16777216.0))
        out[..., 2] = np.where(valid, np.rint(a), np.float32(0)).astype(np.int64) % H
        for k, v in enumerate((x, y)):
            q = v.astype(np.float64) / float(xy_resolution)
            near = np.abs(q) < 1073741824.0                               # (False for NaN)
            c = np.floor(np.where(near, q, 0.0)).astype(np.int64) - int(oc[k])
            out[..., k] = np.where(near, np.clip(c, -_RO_FAR, _RO_FAR), -_RO_FAR)
    return out, valid


def _pose_goals(goals, xy_size, H, frame):
    """goals -> C-contiguous int32 (G, 3) = (x, y, h) window cells and heading, h = -1 for a goal without a yaw; frame as _ctg_goals"""
    a = np.asarray(goals)
    if a.ndim == 1 and a.shape[0] in (2, 3):
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] not in (2, 3) or not 1 <= a.shape[0] <= CTG_MAX_GOALS:
        raise ValueError("goals must have shape (G, 2) or (G, 3) = (x, y[, yaw]) with 1 <= G <= %d, got %r" % (CTG_MAX_GOALS, a.shape))
    if a.dtype.kind not in "iuf":
        raise ValueError("goals must be numbers, got dtype %s" % a.dtype)
    cells = _ctg_goals(a[:, :2], xy_size, frame)
    out = np.full((a.shape[0], 3), -1, np.int32)
    out[:, :2] = cells
    if a.shape[1] == 3:
        yaw = a[:, 2].astype(np.float32)
        with np.errstate(all="ignore"):
            s = yaw * np.float32(H / 6.283185307179586476925286766559)
        if not (np.isfinite(yaw).all() and (np.abs(s) < np.float32(16777216.0)).all()):
            raise ValueError("a goal's yaw must be finite (and below 2**24 heading bins)")
        out[:, 2] = np.rint(s).astype(np.int64) % H
    return np.ascontiguousarray(out)


class _PoseVolume(DeviceArray):
    """One [H, xy, xy] volume of a pose field, indexed [h, x, y] with strides (xy*xy, 1, xy): every plane lies in memory like a
    DeviceCostField's maps.  copy_to_host() returns numpy of the same indexing (a transposed view of the [h][y][x] copy)."""

    def copy_to_host(self):
        g = self._hold._owner
        raw = np.empty((self.shape[0], self.shape[2], self.shape[1]), self.dtype)
        g._check(g._lib.gvom_device_product_copy(g._h, self.product_id, self._part, ctypes.c_void_p(raw.ctypes.data)))
        return raw.transpose(0, 2, 1)


class DevicePoseField(_ProductView):
    """The result of DeviceCostField.pose_field() / Gvom.pose_field_of() / pose_field_of_device(): `.cost` int32 [H, xy, xy], the
    cheapest drive from each state (heading, x, y) to a goal state under the mapper's footprint and primitive tables (CTG_UNREACHED
    where there is none), `.action` uint8 [H, xy, xy], the index of its first primitive within the heading's list (POSE_GOAL at a
    seeded state, CTG_NONE where unreached, CTG_UNSETTLED only in a field that is not final) and `.pose_cost` uint16 [H, xy, xy],
    the cost volume the solver used (0 = the footprint touches a blocked cell or leaves the window) -- three volumes of one product,
    indexed [h, x, y].  `.converged`, `.rounds`, `.reached` (states with a finite cost) and `.goals_seeded` (distinct states seeded)
    describe the solve; `.origin` is the window corner in world metres; `.primitives` the table it was made with.  A snapshot: later
    scans, combines, set_footprint and set_primitives calls do not change it.  copy_to_host() returns (cost, action, pose_cost)."""

    def __init__(self, hold, info, origin, primitives):
        _ProductView.__init__(self, hold)
        self.cost, self.action, self.pose_cost = _PoseVolume(hold, 0), _PoseVolume(hold, 1), _PoseVolume(hold, 2)
        self.converged, self.rounds, self.reached, self.goals_seeded = bool(info[0]), int(info[1]), int(info[2]), int(info[3])
        self.origin = np.array(origin, np.float64)
        self.primitives = primitives
        self._host = None

    def copy_to_host(self):
        return self.cost.copy_to_host(), self.action.copy_to_host(), self.pose_cost.copy_to_host()

    def path_from(self, x, y, h):
        """The states [(x, y, h), ...] from the given one to a seeded goal state, both included, following `.action` on a host copy
        (made once); None where the state is unreached.  RuntimeError on CTG_UNSETTLED (a field that stopped before it converged)."""
        if self._host is None:
            self._host = self.action.copy_to_host()
        a = self._host
        start, prims = self.primitives
        x, y, h = int(x), int(y), int(h)
        if not (0 <= h < a.shape[0] and 0 <= x < a.shape[1] and 0 <= y < a.shape[2]):
            raise ValueError("state (%d, %d, %d) lies outside the field" % (x, y, h))
        path = [(x, y, h)]
        for _ in range(a.size):
            k = int(a[h, x, y])
            if k == POSE_GOAL:
                return path
            if k == CTG_NONE:
                return None
            if k >= start[h + 1] - start[h]:
                raise RuntimeError("state (%d, %d, %d) is unsettled: the field stopped before it converged" % (x, y, h))
            dx, dy, ht, _w = (int(v) for v in prims[start[h] + k])
            x, y, h = x + dx, y + dy, ht
            path.append((x, y, h))
        raise RuntimeError("the actions do not lead to a goal")


ALIGN_MAX_POINTS = 1 << 20
ALIGN_MAX_CANDIDATES = 65536
ALIGN_MAX_PAIRS = 1 << 32
ALIGN_MAX_WEIGHT = 1024
ALIGN_DEFAULT_WEIGHTS = (2, 1, -1, 0, 0)  # {occupied, near, free, unknown, outside}


def _align_shape(n, K):
    try:
        ok = int(n) == n and int(K) == K
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or int(n) < 1 or int(K) < 1:
        raise ValueError("alignment scoring needs n >= 1 returns and K >= 1 candidates, got n = %r, K = %r" % (n, K))
    n, K = int(n), int(K)
    if n > ALIGN_MAX_POINTS or K > ALIGN_MAX_CANDIDATES or n * K > ALIGN_MAX_PAIRS:
        raise ValueError("at most 2**20 returns, 65536 candidates and 2**32 pairs per call, got %d x %d" % (n, K))
    return n, K


def _align_options(dilate, weights):
    if isinstance(dilate, bool):
        dilate = int(dilate)
    if dilate not in (0, 1) or int(dilate) != dilate:
        raise ValueError("dilate must be 0 or 1, got %r" % (dilate,))
    w = np.asarray(weights)
    if w.shape != (5,) or w.dtype.kind not in "iu":
        raise ValueError("weights must be five integers {occupied, near, free, unknown, outside}, got %r" % (weights,))
    if (np.abs(w.astype(np.int64)) > ALIGN_MAX_WEIGHT).any():
        raise ValueError("weights must lie in -1024 .. 1024, got %r" % (weights,))
    return int(dilate), (ctypes.c_int32 * 5)(*[int(v) for v in w])


def _align_cloud(cloud):
    """cloud float32 (n, 3) -> C-contiguous; other dtypes raise TypeError, nothing is cast"""
    c = np.asarray(cloud)
    if c.dtype != np.float32:
        raise TypeError("cloud must be float32, got %s" % c.dtype)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("cloud must have shape (n, 3), got %r" % (c.shape,))
    return np.ascontiguousarray(c)


def _ray_segments(origins, targets):
    """targets (n, 3), origins (3,), (1, 3) or (n, 3), of any float type -> C-contiguous float32 (K, 3) and (n, 3), K = 1 or n"""
    t = np.ascontiguousarray(np.asarray(targets), dtype=np.float32)
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError("targets must have shape (n, 3) with n >= 1, got %r" % (t.shape,))
    n = t.shape[0]
    if n > RAYCAST_MAX_RAYS:
        raise ValueError("at most 2**26 rays per call, got %d" % n)
    o = np.ascontiguousarray(np.asarray(origins), dtype=np.float32)
    if o.shape == (3,):
        o = o.reshape(1, 3)
    if o.shape not in ((1, 3), (n, 3)):
        raise ValueError("origins must have shape (3,), (1, 3) or (%d, 3), got %r" % (n, o.shape))
    return o, t


def _ray_flags(unknown_blocks, check_target=False):
    return (_RAY_UNKNOWN_BLOCKS if unknown_blocks else 0) | (_RAY_CHECK_TARGET if check_target else 0)


def _align_transforms(transforms):
    """transforms float64 (K, 4, 4) or (K, 3, 4) -> C-contiguous float64 (K, 3, 4): rows 0..2"""
    a = np.asarray(transforms)
    if a.dtype != np.float64:
        raise TypeError("transforms must be float64, got %s" % a.dtype)
    if a.ndim != 3 or a.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError("transforms must have shape (K, 4, 4) or (K, 3, 4), got %r" % (a.shape,))
    return np.ascontiguousarray(a[:, :3, :])


def pose_candidates(transform, xy_step, xy_steps, yaw_step, yaw_steps, z_step=0.0, z_steps=0, pivot=None):
    """Candidate poses around `transform` (4x4) for Gvom.score_alignments: float64 [K, 4, 4] with K = (2 z_steps + 1) *
    (2 yaw_steps + 1) * (2 xy_steps + 1)**2.  Candidate k is D_k @ transform, where D_k turns the world by a yaw of a * yaw_step
    about the vertical through `pivot` (world metres; default: the transform's translation) and then moves it by (i * xy_step,
    j * xy_step, l * z_step), with i, j in -xy_steps .. xy_steps, a in -yaw_steps .. yaw_steps, l in -z_steps .. z_steps.
    INDEX ORDER: k = ((l' * A + a') * N + j') * N + i' with N = 2 xy_steps + 1, A = 2 yaw_steps + 1 and primes the indices counted
    from 0 -- x offset fastest, then y offset, then yaw, then z offset; the centre index K // 2 is the all-zero offset, and that
    candidate is `transform` itself, bit for bit."""
    T = np.asarray(transform, np.float64)
    if T.shape != (4, 4):
        raise ValueError("transform must be a 4x4 matrix, got shape %r" % (T.shape,))
    for name, v in (("xy_steps", xy_steps), ("yaw_steps", yaw_steps), ("z_steps", z_steps)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError("%s must be a whole number >= 0, got %r" % (name, v))
    for name, v in (("xy_step", xy_step), ("yaw_step", yaw_step), ("z_step", z_step)):
        if not math.isfinite(float(v)):
            raise ValueError("%s must be finite, got %r" % (name, v))
    N, A, Z = 2 * int(xy_steps) + 1, 2 * int(yaw_steps) + 1, 2 * int(z_steps) + 1
    if N * N * A * Z > ALIGN_MAX_CANDIDATES:
        raise ValueError("more than 65536 candidates: %d" % (N * N * A * Z))
    c = T[:3, 3].copy() if pivot is None else np.asarray(pivot, np.float64).reshape(-1)[:3].copy()
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError("pivot must be (x, y, z) in finite world metres, got %r" % (pivot,))
    out = np.empty((Z, A, N, N, 4, 4), np.float64)
    for l in range(Z):
        for a in range(A):
            yaw = (a - int(yaw_steps)) * float(yaw_step)
            cs, sn = math.cos(yaw), math.sin(yaw)
            for j in range(N):
                for i in range(N):
                    off = ((i - int(xy_steps)) * float(xy_step), (j - int(xy_steps)) * float(xy_step), (l - int(z_steps)) * float(z_step))
                    if yaw == 0.0 and off == (0.0, 0.0, 0.0):
                        out[l, a, j, i] = T                               # the input itself: no arithmetic
                        continue
                    D = np.identity(4)
                    D[0, 0], D[0, 1], D[1, 0], D[1, 1] = cs, -sn, sn, cs
                    D[:3, 3] = c - D[:3, :3].dot(c) + off                 # turn about the pivot, then move
                    out[l, a, j, i] = D.dot(T)
    return out.reshape(-1, 4, 4)


class DeviceAlignments(_ProductView):
    """The result of Gvom.score_alignments() / score_alignments_device(): `.counts` int32 [K, 6] -- per candidate {score, returns
    that end in an occupied voxel, next to one (dilate=1 only), in a free one, in a never-observed one, outside the window} -- and
    `.best` int32 [4] {best index (the lowest of the best score), best score, n, K}: two DeviceArrays of one product, row k =
    candidate k.  `.origin`: the fused map's window origin in voxels when the call was made.  A snapshot: later scans and combines
    do not change it.  copy_to_host() returns (counts, best) as numpy."""

    def __init__(self, hold, origin):
        _ProductView.__init__(self, hold)
        self.origin = origin
        self.counts, self.best = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.counts.copy_to_host(), self.best.copy_to_host()


# ---- map atlas (Gvom.create_atlas; include/gvom_hip.h "map atlas") ----------------------------------------------------
ATLAS_MIN_CELLS, ATLAS_MAX_CELLS = 64, 4096
ATLAS_FOLLOW, ATLAS_FIXED = 0, 1          # GVOM_ATLAS_FOLLOW, GVOM_ATLAS_FIXED
ATLAS_EXTENT_NAMES = ("positive", "negative", "visibility", "roughness", "height_map", "stamp")    # part 0..5 of an extent export


def cells_of(points_xy, xy_resolution):
    """World metres -> the integer world cells the atlas counts in: floor(p / xy_resolution), int64, same shape."""
    p = np.asarray(points_xy, dtype=np.float64)
    if not np.isfinite(p).all():
        raise ValueError("points_xy must be finite")
    return np.floor(p / float(xy_resolution)).astype(np.int64)


def _atlas_cells(cells, xy_size):
    c = int(cells)
    if c != cells or c < ATLAS_MIN_CELLS or c > ATLAS_MAX_CELLS or c & (c - 1):
        raise ValueError("cells must be a power of two in %d .. %d, got %r" % (ATLAS_MIN_CELLS, ATLAS_MAX_CELLS, cells))
    if c < xy_size:
        raise ValueError("cells must be at least xy_size (%d), got %d" % (xy_size, c))
    return c


def _atlas_origin(origin_cells, what="origin_cells"):
    o = np.asarray(origin_cells)
    if o.shape != (2,) or o.dtype.kind not in "iu":
        raise ValueError("%s must be two integers (x, y) in world cells, got %r" % (what, origin_cells))
    if (np.abs(o.astype(np.int64)) > (1 << 40)).any():
        raise ValueError("%s lies beyond 2^40 cells" % what)
    return (_I64 * 2)(int(o[0]), int(o[1]))


def _atlas_maps(maps, xy_size):
    """nine [x, y] numpy maps in set order -> Fortran-ordered arrays of the set's dtypes (nothing is cast: bit patterns count)"""
    if len(maps) != 9:
        raise ValueError("maps must be the nine maps of a set (DEVICE_MAP_NAMES), got %d" % len(maps))
    out = []
    for k, m in enumerate(maps):
        a = np.asarray(m)
        want = np.int32 if k < 3 else np.float64
        if a.shape != (xy_size, xy_size):
            raise ValueError("%s must have shape (%d, %d), got %r" % (DEVICE_MAP_NAMES[k], xy_size, xy_size, a.shape))
        if a.dtype != want:
            raise TypeError("%s must be %s, got %s" % (DEVICE_MAP_NAMES[k], np.dtype(want), a.dtype))
        out.append(np.asfortranarray(a))
    return out


class DeviceAtlasExtent(_ProductView):
    """The result of Atlas.extent_device(): the whole extent unwrapped, six DeviceArrays of one product named as in
    ATLAS_EXTENT_NAMES, each [A, A], [x, y]-indexed with strides (1, A): cell (origin_cells[0] + x, origin_cells[1] + y) at [x, y]."""

    def __init__(self, hold, origin_cells):
        _ProductView.__init__(self, hold)
        self.origin_cells = origin_cells
        for k, name in enumerate(ATLAS_EXTENT_NAMES):
            setattr(self, name, DeviceArray(hold, k))

    def copy_to_host(self):
        return tuple(getattr(self, name).copy_to_host() for name in ATLAS_EXTENT_NAMES)


def _atlas_field_goals(goals, xy_resolution, extent_origin, cells):
    """goals -> C-contiguous int64 (G, 2) WORLD cells inside the extent; xy_resolution for goals in world metres (cells_of), None for
    cells.  ValueError for what gvom_atlas_cost_to_go would refuse; a goal outside the extent names the cell and the extent."""
    a = np.asarray(goals)
    if a.ndim == 1 and a.shape[0] == 2:
        a = a.reshape(1, 2)
    if a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= CTG_MAX_GOALS:
        raise ValueError("goals must have shape (G, 2) with 1 <= G <= %d, got %r" % (CTG_MAX_GOALS, a.shape))
    if a.dtype.kind not in "iuf":
        raise ValueError("goals must be numbers, got dtype %s" % a.dtype)
    if a.dtype.kind == "f" and not np.isfinite(a).all():
        raise ValueError("goals must be finite")
    if xy_resolution is not None:
        a = cells_of(a, xy_resolution)
    elif a.dtype.kind == "f":
        if (a != np.floor(a)).any():
            raise ValueError("goals in cells must be whole numbers")
    a = a.astype(np.int64)
    lo = np.array(extent_origin, np.int64)
    out = ((a < lo) | (a >= lo + cells)).any(axis=1)
    if out.any():
        bad = a[out][0]
        raise ValueError("a goal lies outside the extent: cell (%d, %d), extent [%d, %d) x [%d, %d)" % (
            bad[0], bad[1], lo[0], lo[0] + cells, lo[1], lo[1] + cells))
    return np.ascontiguousarray(a)


def _follow_directions(d, x, y, stop_at_border):
    """the cells from (x, y) down the direction codes of the [x, y] array d, both ends included; None from an unreached cell.  A
    step that leaves the array ends the path at the last cell inside (stop_at_border) or is an error."""
    path = [(x, y)]
    for _ in range(d.size):
        k = int(d[x, y])
        if k == CTG_GOAL:
            return path
        if k == CTG_NONE:
            return None
        if k >= 8:
            raise RuntimeError("cell (%d, %d) is unsettled: the field stopped before it converged" % (x, y))
        x, y = x + CTG_STEPS[k][0], y + CTG_STEPS[k][1]
        if not (0 <= x < d.shape[0] and 0 <= y < d.shape[1]):
            if stop_at_border:
                return path
            raise RuntimeError("the directions lead out of the field")
        path.append((x, y))
    raise RuntimeError("the directions do not lead to a goal")


class DeviceAtlasFieldWindow(DeviceCostField):
    """The result of DeviceAtlasField.window(): the part of an atlas field under a window, as a DeviceCostField -- score_rollouts(),
    frontiers() and pose_field() work on it as on any other.  `.origin` is the window corner in world metres, `.origin_cells` the same
    in world cells; `.converged`, `.rounds`, `.reached` and `.goals_seeded` are the FIELD's.  Cells outside the field's extent read
    CTG_UNREACHED / CTG_NONE / 0.  `.direction` is the field's: at the border a step may point out of the window."""

    def __init__(self, hold, info, origin, origin_cells):
        DeviceCostField.__init__(self, hold, info, origin)
        self.origin_cells = (int(origin_cells[0]), int(origin_cells[1]))

    def path_from(self, cell):
        """The part of the path from window cell (x, y) that lies inside the window: it ends at a goal, or at the last cell before
        the step that leaves the window (the global path goes on there: DeviceAtlasField.path_from).  None where unreached."""
        if self._host is None:
            self._host = self.direction.copy_to_host()
        x, y = int(cell[0]), int(cell[1])
        if not (0 <= x < self._host.shape[0] and 0 <= y < self._host.shape[1]):
            raise ValueError("cell (%d, %d) lies outside the window" % (x, y))
        return _follow_directions(self._host, x, y, True)


class DeviceAtlasFrontiers(DeviceFrontiers):
    """The result of DeviceAtlasField.frontiers(): a DeviceFrontiers over the field's WHOLE extent -- the same four DeviceArrays
    (`.cluster_map` is [A, A] with strides (1, A), A the field's side), the same info attributes and copy_to_host().  Labels, boxes and
    best cells are in the FIELD's frame: field cell (x, y) is world cell (origin_cells[0] + x, origin_cells[1] + y) and has the linear
    index y * A + x.  `.origin_cells` is the field's corner in world cells, `.origin` the same in world metres.  goals() returns world
    metres, goal_cells() world cells, which Atlas.cost_to_go(goals_in_cells=True) and DeviceAtlasField.path_from() take as they are."""

    def __init__(self, hold, info, xy_resolution, origin_cells):
        self.origin_cells = (int(origin_cells[0]), int(origin_cells[1]))
        DeviceFrontiers.__init__(self, hold, info, xy_resolution, np.array(self.origin_cells, np.float64) * float(xy_resolution))

    def _picked(self, order):
        """(rows int64 [n, 8], sums int64 [n, 2], pick): the kept rows on the host and their order"""
        if order not in ("cost", "size"):
            raise ValueError('order must be "cost" or "size", got %r' % (order,))
        n = min(self.n_clusters, self.clusters.shape[0])
        rows, sums = self.clusters.copy_to_host()[:n].astype(np.int64), self.sums.copy_to_host()[:n]
        key = rows[:, 7] if order == "cost" else -rows[:, 1]
        return rows, sums, np.lexsort((rows[:, 0], key))

    def goal_cells(self, order="cost"):
        """(best, rows): int64 [n, 2] WORLD cells (x, y) of each kept cluster's best cell, in the order of goals(), and the int64 [n]
        rows of `.clusters` they come from."""
        rows, _, pick = self._picked(order)
        A = self.cluster_map.shape[0]
        best = np.stack([rows[:, 6] % A, rows[:, 6] // A], axis=1) + np.array(self.origin_cells, np.int64)
        return best[pick], pick

    def goals(self, order="cost"):
        """DeviceFrontiers.goals() in world metres, computed from `.origin_cells` exactly (no float origin is rounded back to cells)."""
        rows, sums, pick = self._picked(order)
        A = self.cluster_map.shape[0]
        oc = np.array(self.origin_cells, np.float64)
        best = np.stack([rows[:, 6] % A, rows[:, 6] // A], axis=1).astype(np.float64)
        centroid = sums.astype(np.float64) / np.maximum(rows[:, 1:2], 1)
        return ((best + oc + 0.5) * self._res)[pick], ((centroid + oc + 0.5) * self._res)[pick], pick


class DeviceAtlasField(_ProductView):
    """The result of Atlas.cost_to_go(): the cost-to-go field of the atlas's whole extent -- `.cost` int32, `.direction` uint8 and
    `.cell_cost` uint16, each [A, A], three DeviceArrays of one product, [x, y]-indexed with strides (1, A): world cell
    (origin_cells[0] + x, origin_cells[1] + y) at [x, y], with the values of a DeviceCostField.  `.origin_cells` is the extent's
    corner when the field was made, `.origin` the same in world metres; `.converged`, `.rounds`, `.reached` and `.goals_seeded`
    describe the solve.  A snapshot: later integrates, moves of the extent, clear() and a new create_atlas() do not change it.
    copy_to_host() returns (cost, direction, cell_cost) as Fortran-ordered numpy [x, y]."""

    def __init__(self, hold, info, origin_cells, xy_resolution):
        _ProductView.__init__(self, hold)
        self.cost, self.direction, self.cell_cost = DeviceArray(hold, 0), DeviceArray(hold, 1), DeviceArray(hold, 2)
        self.converged, self.rounds, self.reached, self.goals_seeded = bool(info[0]), int(info[1]), int(info[2]), int(info[3])
        self.origin_cells = (int(origin_cells[0]), int(origin_cells[1]))
        self._res = float(xy_resolution)
        self.origin = np.array(self.origin_cells, np.float64) * self._res
        self._host = None

    def copy_to_host(self):
        return self.cost.copy_to_host(), self.direction.copy_to_host(), self.cell_cost.copy_to_host()

    def path_from(self, cell):
        """The WORLD cells from world cell `cell` = (x, y) to a goal, both included, following `.direction` on a host copy (made
        once); None where the cell is unreached.  RuntimeError on CTG_UNSETTLED (a field that stopped before it converged)."""
        if self._host is None:
            self._host = self.direction.copy_to_host()
        ox, oy = self.origin_cells
        x, y = int(cell[0]) - ox, int(cell[1]) - oy
        if not (0 <= x < self._host.shape[0] and 0 <= y < self._host.shape[1]):
            raise ValueError("cell (%d, %d) lies outside the field's extent" % (int(cell[0]), int(cell[1])))
        path = _follow_directions(self._host, x, y, False)
        return None if path is None else [(px + ox, py + oy) for px, py in path]

    def frontiers(self, min_cells=4, max_clusters=1024):
        """Where unexplored ground remains ANYWHERE this field reaches: DeviceCostField.frontiers() on the field's whole extent, with
        the atlas's visibility as it is now (seen: visibility > 0; never seen: <= 0; a cell outside the atlas's present extent is
        neither) -- a DeviceAtlasFrontiers whose clusters are not cut at window borders and whose best cells carry the global cost to
        go.  Seed the field AT the vehicle.  Neither the field's edge nor the atlas's is a frontier.  The call waits for the labelling.
        include/gvom_hip.h "atlas frontiers" has the definition."""
        g = self._hold._owner
        min_cells, max_clusters = _frontier_limits(min_cells, max_clusters)
        info, e = (_I64 * 4)(), (_I64 * 2)()
        hold = g._make_product(lambda pid: g._lib.gvom_atlas_frontiers(g._h, int(self.product_id), min_cells, max_clusters, pid, info, e),
                               PRODUCT_ATLAS_FRONTIERS, g._check_args)
        return DeviceAtlasFrontiers(hold, list(info), self._res, (int(e[0]), int(e[1])))

    def window(self, device_maps=None, origin_cells=None):
        """The part of this field under a window as a DeviceAtlasFieldWindow (a DeviceCostField): the window of a live DeviceMaps
        -- a combine's or a recall's --, or the one whose corner is origin_cells (integer world cells).  Cropped on the GPU behind
        the solve; no host wait.  Window cell (x, y) is world cell (corner + (x, y)); outside the field's extent it reads
        unreached.  The local planner's terminal cost: window(maps).score_rollouts(poses)."""
        g = self._hold._owner
        if (device_maps is None) == (origin_cells is None):
            raise ValueError("give device_maps or origin_cells, one of the two")
        if device_maps is not None:
            if not isinstance(device_maps, DeviceMaps):
                raise ValueError("window takes the DeviceMaps whose window it crops to, got %r" % (type(device_maps).__name__,))
            sid, org, cells, origin = int(device_maps.set_id), None, device_maps.origin_cells[:2], device_maps.origin
        else:
            org = _atlas_origin(origin_cells)
            sid, cells = -1, (int(org[0]), int(org[1]))
            origin = np.array(cells, np.float64) * self._res
        hold = g._make_product(lambda pid: g._lib.gvom_atlas_field_window(g._h, int(self.product_id), sid, org, pid), PRODUCT_COSTFIELD,
                               g._check_args)
        info = [self.converged, self.rounds, self.reached, self.goals_seeded]
        return DeviceAtlasFieldWindow(hold, info, origin, cells)


class Atlas(object):
    """The map atlas of a mapper (Gvom.create_atlas): a world-fixed, toroidally stored memory of the nine 2-D maps, `cells` x `cells`
    world cells of device memory (64 bytes each), that keeps what the rolling window forgets.  integrate() merges a combine's set
    into it on the GPU -- observed ground is never overwritten by an inference or by nothing --, recall() returns any window-sized
    part of it as an ordinary DeviceMaps, on which clearance(), cost_to_go(), score_attitude() and DeviceCostField.frontiers() work
    as on a combine's.  Only counts() waits for the GPU.  include/gvom_hip.h "map atlas" has the definition."""

    def __init__(self, owner, cells, follow, origin_cells):
        self._owner = owner
        self.cells = _atlas_cells(cells, owner.xy_size)
        self.follow = bool(follow)
        if not self.follow and origin_cells is None:
            raise ValueError("a fixed atlas needs origin_cells, the corner of its extent")
        org = None if origin_cells is None else _atlas_origin(origin_cells)
        owner._check_args(owner._lib.gvom_atlas_configure(owner._h, self.cells, ATLAS_FOLLOW if self.follow else ATLAS_FIXED, org))
        self.extent_origin = (0, 0) if org is None else (int(org[0]), int(org[1]))
        self.seq = 0
        self._last = None                       # the last integrated set's origin: the default of recall()

    def _integrated(self, origin):
        g = self._owner
        self._last = (int(origin[0]), int(origin[1]))
        self.seq += 1
        if self.follow:
            self.extent_origin = tuple(o + g.xy_size // 2 - self.cells // 2 for o in self._last)

    def integrate(self, device_maps):
        """Merges a live DeviceMaps (a combine's, or a recall's) into the atlas, behind the kernel that wrote it; no host wait."""
        g = self._owner
        g._check_args(g._lib.gvom_atlas_integrate(g._h, int(device_maps.set_id), None, 0, None))
        self._integrated(device_maps.origin_cells)

    def integrate_of(self, maps, origin_cells):
        """The same for nine numpy maps in set order (DEVICE_MAP_NAMES), [x, y] of shape (xy_size, xy_size), int32 / float64 as
        DeviceMap.copy_to_host() gives them, and the integer origin of their window.  The maps are copied to the device."""
        g = self._owner
        arrs = _atlas_maps(maps, g.xy_size)
        org = _atlas_origin(origin_cells)
        ptrs = (_P * 9)(*[a.ctypes.data for a in arrs])
        g._check_args(g._lib.gvom_atlas_integrate(g._h, -1, ptrs, 0, org))
        self._integrated(org)

    def integrate_of_device(self, ptrs, origin_cells):
        """The same for nine maps in device memory: raw device addresses in set order (cell (x, y) at [y*xy_size + x]); the data
        must be ready when the call is made."""
        g = self._owner
        if len(ptrs) != 9 or not all(ptrs):
            raise ValueError("ptrs must be nine device addresses, the maps of a set in order")
        org = _atlas_origin(origin_cells)
        g._check_args(g._lib.gvom_atlas_integrate(g._h, -1, (_P * 9)(*[int(p) for p in ptrs]), 1, org))
        self._integrated(org)

    def recall(self, origin_cells=None, center=None):
        """A window-sized part of the atlas as a DeviceMaps -- with `.stamps` and `.recall_counts` = DeviceArrays of int32 [x, y]
        and {cells of rank 2, of rank 1, outside the extent, seq} -- whose corner is origin_cells (integer world cells), or the
        window a scan with its ego at `center` (x, y in world metres) would have: floor(c / xy_resolution - xy_size / 2), the
        scan's own arithmetic.  Default: the last integrated set's origin.  Cells outside the extent read UNKNOWN.  No host wait."""
        g = self._owner
        if origin_cells is not None and center is not None:
            raise ValueError("give origin_cells or center, not both")
        if center is not None:
            c = np.asarray(center, dtype=np.float64)
            if c.shape != (2,) or not np.isfinite(c).all():
                raise ValueError("center must be two finite numbers (x, y) in metres, got %r" % (center,))
            origin_cells = [int(math.floor(v / g.xy_resolution - g.xy_size / 2.0)) for v in c]
        org = None if origin_cells is None else _atlas_origin(origin_cells)
        sid, pid, world = ctypes.c_int64(-1), ctypes.c_int64(-1), np.zeros(3, np.float64)
        g._check_args(g._lib.gvom_atlas_recall(g._h, org, ctypes.byref(sid), ctypes.byref(pid), _ptr(world)))
        maps = DeviceMaps(g, int(sid.value), world)
        hold = _ProductHold(g, PRODUCT_ATLAS_RECALL, int(pid.value))
        maps.stamps, maps.recall_counts = DeviceArray(hold, 0), DeviceArray(hold, 1)
        maps._recall_hold = hold
        return maps

    def extent_device(self):
        """The whole extent unwrapped, as a DeviceAtlasExtent (32 bytes per cell).  No host wait."""
        g = self._owner
        e = (_I64 * 2)()
        hold = g._make_product(lambda pid: g._lib.gvom_atlas_extent(g._h, pid, e), PRODUCT_ATLAS_EXTENT, g._check_args)
        return DeviceAtlasExtent(hold, (int(e[0]), int(e[1])))

    def cost_to_go(self, goals, goals_in_cells=False, inflation_radius=None, density_threshold=50, include_negative=True,
                   unknown="free", base=1, soft_weight=0, rough_weight=0, roughness_range=None, max_cost=None, max_rounds=0):
        """The navigation function of EVERYTHING the atlas holds towards `goals`: DeviceMaps.cost_to_go() on the whole extent, read
        from the atlas in place, as a DeviceAtlasField ([A, A]; its window() is the DeviceCostField a local planner scores
        rollouts against).  The call waits for the field.  goals: (G, 2) world metres (x, y), converted by cells_of -- or integer
        WORLD cells with goals_in_cells=True; a goal outside the extent raises ValueError, one on a blocked cell seeds nothing.
        The other keywords are DeviceMaps.cost_to_go()'s; never observed means visibility <= 0 here, and obstacles anywhere in the
        extent inflate.  The extent's opposite edges are not neighbours.  include/gvom_hip.h "atlas fields" has the definition."""
        g = self._owner
        cells = _atlas_field_goals(goals, None if goals_in_cells else g.xy_resolution, self.extent_origin, self.cells)
        params, flags = _ctg_params(g.xy_resolution, inflation_radius, density_threshold, include_negative, unknown, base, soft_weight,
                                    rough_weight, roughness_range)
        info, e = (_I64 * 4)(), (_I64 * 2)()
        hold = g._make_product(lambda pid: g._lib.gvom_atlas_cost_to_go(
            g._h, ctypes.byref(params), cells.ctypes.data_as(ctypes.POINTER(_I64)), cells.shape[0], _ctg_max_cost(max_cost),
            _ctg_max_rounds(max_rounds), flags, pid, info, e), PRODUCT_ATLAS_FIELD, g._check_args)
        return DeviceAtlasField(hold, list(info), (int(e[0]), int(e[1])), g.xy_resolution)

    def clear(self):
        """Every cell becomes UNKNOWN; the extent and seq stay."""
        g = self._owner
        g._check_args(g._lib.gvom_atlas_clear(g._h))

    def counts(self):
        """Waits for the GPU.  A dict: of the last integrate `written`, `kept`, `uninformative`, `outside`, `cleared`,
        `cleared_known`; of the atlas `known` (cells of rank >= 1) and `seq`."""
        g = self._owner
        out = (_I64 * 8)()
        g._check_args(g._lib.gvom_atlas_counts(g._h, out))
        names = ("written", "kept", "uninformative", "outside", "cleared", "cleared_known", "known", "seq")
        return dict(zip(names, (int(v) for v in out)))

    def release(self):
        """Frees the atlas's device memory."""
        g = self._owner
        if g._h:
            g._check_args(g._lib.gvom_atlas_configure(g._h, 0, 0, None))


# ---- voxel atlas (Gvom.create_voxel_atlas; include/gvom_hip.h "voxel atlas") ----------------------------------------------
VOXEL_NEVER, VOXEL_FREE, VOXEL_OCCUPIED = 0, 1, 2       # GVOM_VOXEL_*: the class codes of a DeviceVoxelBox
VOXEL_ATLAS_COUNTS = ("first_seen", "free_to_occupied", "occupied_to_free", "confirmed", "uninformative", "outside", "cleared",
                      "cleared_observed", "observed", "occupied", "seq")


def _voxel_atlas_sizes(cells, levels, xy_size, z_size):
    c = _atlas_cells(cells, xy_size)
    z = int(levels)
    if z != levels or z < 1 or z > c or z & (z - 1):
        raise ValueError("levels must be a power of two, at most cells (%d), got %r" % (c, levels))
    if z < z_size:
        raise ValueError("levels must be at least z_size (%d), got %d" % (z_size, z))
    if c * c * z > 1 << 32:
        raise ValueError("cells * cells * levels must not exceed 2**32, got %d" % (c * c * z))
    return c, z


def _voxel_origin(origin_voxels, what="origin_voxels", limit=None):
    o = np.asarray(origin_voxels)
    if o.shape != (3,) or o.dtype.kind not in "iu":
        raise ValueError("%s must be three integers (x, y, z) in world voxels, got %r" % (what, origin_voxels))
    if limit is not None and (np.abs(o.astype(np.int64)) >= limit).any():
        raise ValueError("%s lies at or beyond 2^30 voxels" % what)
    return (_I64 * 3)(int(o[0]), int(o[1]), int(o[2]))


class DeviceVoxelBox(_OnePartDLPack, _ProductView):
    """The result of VoxelAtlas.box(): `.classes` uint8 [xy, xy, z] in the occupancy grid's layout -- VOXEL_NEVER, VOXEL_FREE or
    VOXEL_OCCUPIED per voxel, VOXEL_NEVER outside the extent -- and `.counts` int32 [4] {occupied, free, voxels outside the extent,
    seq}: two DeviceArrays of one product.  `.origin_voxels`: the box's corner in world voxels.  `classes == VOXEL_OCCUPIED` is an
    occupancy grid of remembered space.  A snapshot.  DLPack hands over the class grid.  copy_to_host() returns (classes, counts)."""
    _dlpack_part = "classes"

    def __init__(self, hold, origin_voxels):
        _ProductView.__init__(self, hold)
        self.origin_voxels = origin_voxels
        self.classes, self.counts = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.classes.copy_to_host(), self.counts.copy_to_host()


CHANGE_APPEARED, CHANGE_VANISHED = 1, 2                 # GVOM_CHANGE_*: the codes of a DeviceVoxelChanges


def _change_mask(appeared, vanished):
    mask = (1 if appeared else 0) | (2 if vanished else 0)
    if mask == 0:
        raise ValueError("changes() needs appeared, vanished or both")
    return mask


class DeviceVoxelChanges(_OnePartDLPack, _ProductView):
    """The result of VoxelAtlas.changes(): what the current fused map contradicts of what the atlas remembers.  `.codes` uint8 [xy, xy, z]
    in the occupancy grid's layout -- CHANGE_APPEARED where the window is occupied and the atlas remembers free, CHANGE_VANISHED where the
    window is free and the atlas remembers occupied, 0 elsewhere --, `.column_counts` uint16 [2, xy, xy] (appeared / vanished voxels per
    column, [k, x, y]-indexed), `.cluster_map` int32 [xy, xy] (the rank of the column's cluster, FRONTIER_NONE where the column is not
    marked, FRONTIER_SMALL where its cluster is below min_cells), `.rows` int32 [cap, 8], `.sums` int64 [cap, 2] and `.voxels` int32
    [cap, 4] per kept cluster (include/gvom_hip.h "voxel atlas changes": parts 0, 1 and 4) and `.counts` int32 [8] {kept clusters, marked
    columns, marked columns in kept clusters, cap, appeared voxels, vanished voxels, window voxels outside the extent, seq}: seven
    DeviceArrays of one product.  `.origin_voxels`: the window's corner in world voxels; `.rounds`, `.n_clusters`, `.marked_columns` and
    `.dropped` describe the call.  A snapshot.  DLPack hands over the codes.  copy_to_host() returns (rows, sums, cluster_map, counts,
    voxels, codes, column_counts)."""
    _dlpack_part = "codes"

    def __init__(self, hold, origin_voxels, info, xy_resolution, z_resolution):
        _ProductView.__init__(self, hold)
        self.origin_voxels = origin_voxels
        self.rows, self.sums, self.cluster_map, self.counts, self.voxels, self.codes = (DeviceArray(hold, k) for k in range(6))
        self.column_counts = _PoseVolume(hold, 6)            # planes laid out like a pose field's: [k, x, y]-indexed
        self.rounds, self.n_clusters, self.marked_columns, self.dropped = int(info[0]), int(info[1]), int(info[2]), int(info[3])
        self._res = (float(xy_resolution), float(z_resolution))

    def copy_to_host(self):
        return tuple(a.copy_to_host() for a in (self.rows, self.sums, self.cluster_map, self.counts, self.voxels, self.codes, self.column_counts))

    def clusters(self):
        """The kept clusters on the host, n = min(n_clusters, cap) of them in ascending label order: a dict of arrays -- "label" int64
        [n], "columns" int64 [n], "appeared" and "vanished" int64 [n] (voxels), "box" int64 [n, 4] {min x, min y, max x, max y} in
        window columns, "levels" int64 [n, 2] {lowest, highest} window level of a counted voxel, and in world metres "centroid"
        float64 [n, 2], "nearest" float64 [n, 2] (the centre of the cluster's column nearest the vehicle), "nearest_distance" float64
        [n] (between column centres) and "z_range" float64 [n, 2] (bottom of the lowest, top of the highest level)."""
        n = min(self.n_clusters, self.rows.shape[0])
        rows, sums, vox = self.rows.copy_to_host()[:n].astype(np.int64), self.sums.copy_to_host()[:n], self.voxels.copy_to_host()[:n].astype(np.int64)
        xy = self.cluster_map.shape[0]
        res, zres = self._res
        W = np.array(self.origin_voxels, np.float64)
        near = np.stack([rows[:, 6] % xy, rows[:, 6] // xy], axis=1).astype(np.float64)
        centroid = sums.astype(np.float64) / np.maximum(rows[:, 1:2], 1)
        return {"label": rows[:, 0], "columns": rows[:, 1], "appeared": vox[:, 0], "vanished": vox[:, 1], "box": rows[:, 2:6], "levels": vox[:, 2:4],
                "centroid": (centroid + W[:2] + 0.5) * res, "nearest": (near + W[:2] + 0.5) * res,
                "nearest_distance": np.sqrt(rows[:, 7].astype(np.float64)) * res,
                "z_range": (vox[:, 2:4] + W[2] + np.array([0.0, 1.0])) * zres}


class DeviceAtlasRays(_ProductView):
    """The result of VoxelAtlas.raycast() / raycast_device(): `.result` int32 [n, 3] -- per ray {status (RAY_*; RAY_LEFT_WINDOW: it left
    the extent), steps, unknown voxels passed} --, `.position` float32 [n, 3], where the ray stopped in world metres (NaN where it did
    not stop at a voxel), and `.voxel` int32 [n, 3], the WORLD voxel of the stop ((0, 0, 0) where there is none): three DeviceArrays of
    one product, row i = ray i.  `.extent_origin`: the extent's corner in world voxels when the call was made.  A snapshot.
    copy_to_host() returns (result, position, voxel) as numpy."""

    def __init__(self, hold, extent_origin):
        _ProductView.__init__(self, hold)
        self.extent_origin = extent_origin
        self.result, self.position, self.voxel = DeviceArray(hold, 0), DeviceArray(hold, 1), DeviceArray(hold, 2)

    def copy_to_host(self):
        return self.result.copy_to_host(), self.position.copy_to_host(), self.voxel.copy_to_host()


class DeviceAtlasViewpoints(DeviceViewpoints):
    """The result of VoxelAtlas.score_viewpoints() / score_viewpoints_device(): a DeviceViewpoints whose beams were cast through the
    voxel atlas -- RAY_LEFT_WINDOW means "left the extent", the gain counts distinct never-observed WORLD voxels -- with best_pose().
    `.origin` and `.extent_origin`: the extent's corner in world voxels when the call was made."""

    def __init__(self, hold, extent_origin, poses=None):
        DeviceViewpoints.__init__(self, hold, np.array(extent_origin, np.float64), poses)
        self.extent_origin = extent_origin


class DeviceAtlasAlignments(DeviceAlignments):
    """The result of VoxelAtlas.score_alignments() / score_alignments_device(): a DeviceAlignments whose returns were classed by the
    voxel atlas -- "outside" means outside the box, "near" looks at remembered occupied voxels beyond the box's faces too.
    `.origin_voxels`: the box's corner in world voxels; `.origin` the same as float64."""

    def __init__(self, hold, origin_voxels):
        DeviceAlignments.__init__(self, hold, np.array(origin_voxels, np.float64))
        self.origin_voxels = origin_voxels


_DISTANCE_UNKNOWN_BLOCKS = 1              # GVOM_DISTANCE_UNKNOWN_BLOCKS
DISTANCE_MAX_POINTS = 1 << 26
DISTANCE_MAX_HALO = 32767                 # voxels a cap may reach on an axis


def distance_halo(max_distance, resolution):
    """The halo of a cap on an axis of `resolution` metres per voxel, as the library computes it: the largest h with
    fl64(a * (double)(h*h)) <= fl64(max_distance * max_distance), a = fl64(resolution * resolution) -- a source further away on that
    axis cannot be within the cap (include/gvom_hip.h "voxel distance field")."""
    a, cap2 = float(resolution) * float(resolution), float(max_distance) * float(max_distance)
    h = int(math.sqrt(cap2 / a))
    while a * float((h + 1) * (h + 1)) <= cap2:
        h += 1
    while h > 0 and a * float(h * h) > cap2:
        h -= 1
    return h


def _distance_cap(max_distance, xy_resolution, z_resolution):
    """max_distance of VoxelAtlas.distance_field() as a float: ValueError for NaN, infinite and non-positive values and for less
    than the finer of the two resolutions (a field that could only read 0 or +inf)."""
    try:
        d = float(max_distance)
    except (TypeError, ValueError):
        raise ValueError("max_distance must be a finite distance > 0 in metres, got %r" % (max_distance,))
    if d != d or d <= 0 or d == float("inf"):
        raise ValueError("max_distance must be a finite distance > 0 in metres, got %r" % (max_distance,))
    finer = min(float(xy_resolution), float(z_resolution))
    if d < finer:
        raise ValueError("max_distance must be at least one voxel of the finer resolution (%r m), got %r" % (finer, max_distance))
    return d


class DeviceDistanceSamples(_ProductView):
    """The result of DeviceDistanceField.sample() / sample_device(): `.distance` float32 [n], the field's value at the voxel of every
    point (NaN where the voxel lies outside the field's box or a coordinate is not finite), and `.counts` int32 [4] {points inside
    the box, of those finite, of those at 0, n}: two DeviceArrays of one product.  A snapshot.  copy_to_host() returns (distance,
    counts)."""

    def __init__(self, hold):
        _ProductView.__init__(self, hold)
        self.distance, self.counts = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.distance.copy_to_host(), self.counts.copy_to_host()


class DeviceDistanceField(_OnePartDLPack, _ProductView):
    """The result of VoxelAtlas.distance_field(): `.distance` float32 [xy, xy, z] in the class grid's layout -- metres from the
    voxel's centre to the centre of the nearest source voxel anywhere in the atlas's extent, 0 at a source, +inf beyond
    `.max_distance` -- and `.counts` int32 [4] {voxels at 0, voxels with a finite distance, voxels outside the extent, seq}: two
    DeviceArrays of one product.  `.origin_voxels`: the box's corner in world voxels; the field lines up voxel for voxel with
    VoxelAtlas.box() at the same origin.  A snapshot.  DLPack hands over `.distance`; copy_to_host() returns (distance, counts)."""
    _dlpack_part = "distance"

    def __init__(self, hold, origin_voxels, max_distance):
        _ProductView.__init__(self, hold)
        self.origin_voxels, self.max_distance = origin_voxels, max_distance
        self.distance, self.counts = DeviceArray(hold, 0), DeviceArray(hold, 1)

    def copy_to_host(self):
        return self.distance.copy_to_host(), self.counts.copy_to_host()

    def _sample(self, points_ptr, n, on_device):
        g = self._hold._owner
        n = int(n)
        if n < 1 or n > DISTANCE_MAX_POINTS:
            raise ValueError("between 1 and 2**26 points per call, got %d" % n)
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_distance_sample(g._h, self.product_id, points_ptr, n, int(on_device), pid),
                               PRODUCT_VOXEL_DISTANCE_SAMPLES, g._check_args)
        return DeviceDistanceSamples(hold)

    def score_body(self, device_maps, poses, min_margin=0.0, inferred_ground=True):
        """Where the mapper's body (Gvom.set_body) lies in this field once the vehicle sits on the ground of `device_maps` (a DeviceMaps:
        its `height` map and, with inferred_ground, its `inferred height` map) at every pose of K candidate trajectories, and how
        close it comes to a remembered obstacle: a DeviceBodyClearance, one kernel on the GPU behind the passes that wrote the field
        and the combine that wrote the set; no host wait once the poses are up.  poses: (K, T, 3) = (x, y, yaw) in world metres and
        radians, ROUNDED TO float32.  A pose collides where its clearance < min_margin (metres); a body is clear of every remembered
        voxel centre where the clearance is at least the voxel's half diagonal.  Needs set_footprint, set_chassis and set_body.
        include/gvom_hip.h "body clearance scoring" has the definition."""
        g = self._hold._owner
        a = _rollout_poses(poses)
        return g._score_body(self.product_id, None, None, device_maps.set_id, None, _ptr(a), a.shape[0], a.shape[1], 0, bool(inferred_ground),
                             device_maps.origin, min_margin)

    def score_body_of(self, ground, poses, origin=(0.0, 0.0), min_margin=0.0):
        """score_body() on a ground map of the caller's: a numpy [x, y] array of shape (xy_size, xy_size), heights in metres as
        Gvom.score_attitude_of takes them; origin: the window corner in world metres."""
        g = self._hold._owner
        gm = g._window_map("ground", ground, np.float64)
        a = _rollout_poses(poses)
        return g._score_body(self.product_id, None, None, -1, _ptr(gm), _ptr(a), a.shape[0], a.shape[1], 0, False, origin, min_margin)

    def body_volume(self, device_maps, min_margin=0.0, soft_margin=None, inferred_ground=True):
        """score_body() at EVERY state of the window -- the centre of each cell of `device_maps` (a DeviceMaps) at each heading of the
        mapper's footprint table -- without a pose array: a DeviceBodyVolume (status, squeeze and clearance per state), one kernel on
        the GPU behind the passes that wrote the field and the combine that wrote the set; no host wait.  A state collides where its
        clearance < min_margin; its squeeze says how much of the band from soft_margin (None: min_margin -- squeeze is 100 at a
        collision and 0 elsewhere) down to min_margin it has used up.  DeviceCostField.pose_field(body=...) takes it into a pose
        field.  Needs set_footprint, set_chassis and set_body.  include/gvom_hip.h "body volumes" has the definition."""
        g = self._hold._owner
        return g._body_volume(self.product_id, None, None, device_maps.set_id, None, 0, bool(inferred_ground), device_maps.origin, min_margin,
                              soft_margin)

    def body_volume_of(self, ground, origin=(0.0, 0.0), min_margin=0.0, soft_margin=None):
        """body_volume() on a ground map of the caller's: a numpy [x, y] array of shape (xy_size, xy_size), heights in metres as
        Gvom.score_attitude_of takes them; origin: the window corner in world metres."""
        g = self._hold._owner
        gm = g._window_map("ground", ground, np.float64)
        return g._body_volume(self.product_id, None, None, -1, _ptr(gm), 0, False, origin, min_margin, soft_margin)

    def sample(self, points):
        """The field at the voxels of world points float32 [n, 3] in metres -- floor(p / resolution) per axis, no interpolation: a
        DeviceDistanceSamples.  A body sphere of radius r at p is clear of every source where sample(p) >= r + the voxel's half
        diagonal.  Waits only for the upload of the points."""
        p = np.ascontiguousarray(np.asarray(points), dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError("points must have shape (n, 3) with n >= 1, got %r" % (p.shape,))
        return self._sample(_ptr(p), p.shape[0], 0)

    def sample_device(self, points_ptr, n):
        """The same for n points float32 [n, 3] in device memory.  Enqueues and returns: no host wait."""
        if not points_ptr:
            raise ValueError("points_ptr must be a device address")
        return self._sample(_dev(points_ptr), n, 1)


class VoxelAtlas(object):
    """The voxel atlas of a mapper (Gvom.create_voxel_atlas): a world-fixed, toroidally stored memory of the voxels' classes --
    never observed, observed free, occupied -- `cells` x `cells` x `levels` voxels at 2 bits each, that keeps what the rolling window
    forgets.  integrate() merges the current fused map into it on the GPU (what the window has observed wins; what it has not stays as
    it was known), raycast() and score_viewpoints() are Gvom.raycast() and Gvom.score_viewpoints() on the whole extent, box() returns any
    window-sized part as a class grid, score_alignments() is Gvom.score_alignments() against any such part.  Only counts() waits for
    the GPU (score_viewpoints_device() reads its poses back).
    include/gvom_hip.h "voxel atlas" has the definition."""

    def __init__(self, owner, cells, levels, follow, origin_voxels):
        self._owner = owner
        self.cells, self.levels = _voxel_atlas_sizes(cells, levels, owner.xy_size, owner.z_size)
        self.follow = bool(follow)
        if not self.follow and origin_voxels is None:
            raise ValueError("a fixed voxel atlas needs origin_voxels, the corner of its extent")
        org = None if origin_voxels is None else _voxel_origin(origin_voxels, limit=1 << 30)
        owner._check_args(owner._lib.gvom_voxel_atlas_configure(owner._h, self.cells, self.levels, ATLAS_FOLLOW if self.follow else ATLAS_FIXED, org))
        self.extent_origin = (0, 0, 0) if org is None else tuple(int(v) for v in org)
        self.seq = 0

    def integrate(self):
        """Merges the CURRENT fused map (the map of the most recently begun combine) into the atlas; no host wait.  False before the
        first combine (nothing was merged), else True."""
        g = self._owner
        if g._check_args(g._lib.gvom_voxel_atlas_integrate(g._h)) == GVOM_NO_DATA:
            return False
        self.seq += 1
        if self.follow:
            W = tuple(int(v) for v in g._state().combined_origin)
            sizes, sides = (g.xy_size, g.xy_size, g.z_size), (self.cells, self.cells, self.levels)
            self.extent_origin = tuple(w + n // 2 - s // 2 for w, n, s in zip(W, sizes, sides))
        return True

    def box(self, origin_voxels=None, center=None):
        """A window-sized part of the atlas as a DeviceVoxelBox whose corner is origin_voxels (integer world voxels), or the window a
        scan with its ego at `center` (x, y, z in world metres) would have: floor(c / resolution - size / 2) per axis, the scan's own
        arithmetic.  Default: the last integrated window (None before the first integrate).  Voxels outside the extent read VOXEL_NEVER.  None before
        the first combine.
        No host wait."""
        g = self._owner
        org = self._box_origin(origin_voxels, center)
        out = (_I64 * 3)()
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_atlas_box(g._h, org, pid, out), PRODUCT_VOXEL_BOX, g._check_args)
        return None if hold is None else DeviceVoxelBox(hold, tuple(int(v) for v in out))

    def changes(self, appeared=True, vanished=True, min_cells=2, max_clusters=1024):
        """What the CURRENT fused map contradicts of what the atlas remembers, BEFORE integrate() merges it: a DeviceVoxelChanges -- the
        voxels that are occupied now and remembered free (appeared) or free now and remembered occupied (vanished) as codes and per
        column, and the 8-connected clusters of the columns that hold one of the selected kinds, of at least min_cells columns, at most
        max_clusters of them summarised.  Read-only on the map and on the atlas; the intended loop is combine_maps_device(), changes(),
        integrate().  None before the first combine.  Waits for the labelling, like DeviceCostField.frontiers()."""
        g = self._owner
        mask = _change_mask(appeared, vanished)
        mc, cap = _frontier_limits(min_cells, max_clusters)
        out, info = (_I64 * 3)(), (_I64 * 4)()
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_atlas_changes(g._h, mask, mc, cap, pid, out, info), PRODUCT_VOXEL_CHANGES, g._check_args)
        return None if hold is None else DeviceVoxelChanges(hold, tuple(int(v) for v in out), info, g.xy_resolution, g.z_resolution)

    def distance_field(self, max_distance, origin_voxels=None, center=None, unknown_blocks=False):
        """The exact 3-D clearance of a window-sized part of the atlas, truncated at max_distance metres: a DeviceDistanceField whose
        `.distance` float32 [xy, xy, z] is, per voxel, the Euclidean distance in metres (xy_resolution in x and y, z_resolution in z,
        voxel centre to voxel centre) to the nearest remembered OCCUPIED voxel -- anywhere in the extent, not only in the box --, 0 at
        such a voxel and +inf where none lies within max_distance.  unknown_blocks=True: never-observed voxels are sources too,
        everything outside the extent among them.  The box as for box(): origin_voxels, or the window of a scan with its ego at
        `center`; default: the last integrated window.  None where box() returns None.  ValueError for a cap that is not a finite
        distance > 0 or lies below the finer of the two resolutions.  No host wait."""
        g = self._owner
        cap = _distance_cap(max_distance, g.xy_resolution, g.z_resolution)
        org = self._box_origin(origin_voxels, center)
        out = (_I64 * 3)()
        flags = _DISTANCE_UNKNOWN_BLOCKS if unknown_blocks else 0
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_atlas_distance_field(g._h, org, cap, flags, pid, out), PRODUCT_VOXEL_DISTANCE, g._check_args)
        return None if hold is None else DeviceDistanceField(hold, tuple(int(v) for v in out), cap)

    def _box_origin(self, origin_voxels, center):
        """the corner of a window-sized box as the library takes it: origin_voxels, or the window of a scan with its ego at `center`,
        or None (the last integrated window)"""
        g = self._owner
        if origin_voxels is not None and center is not None:
            raise ValueError("give origin_voxels or center, not both")
        if center is not None:
            c = np.asarray(center, dtype=np.float64)
            if c.shape != (3,) or not np.isfinite(c).all():
                raise ValueError("center must be three finite numbers (x, y, z) in metres, got %r" % (center,))
            res, size = (g.xy_resolution, g.xy_resolution, g.z_resolution), (g.xy_size, g.xy_size, g.z_size)
            origin_voxels = [int(math.floor(v / r - n / 2.0)) for v, r, n in zip(c, res, size)]
        return None if origin_voxels is None else _voxel_origin(origin_voxels)

    def _score_alignments(self, cloud_ptr, n, tf_ptr, K, on_device, dilate, weights, origin_voxels, center):
        g = self._owner
        dilate, w = _align_options(dilate, weights)
        n, K = _align_shape(n, K)
        org = self._box_origin(origin_voxels, center)
        out = (_I64 * 3)()
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_atlas_score_alignments(g._h, cloud_ptr, n, tf_ptr, K, int(on_device), dilate, w, org,
                                                                                    out, pid), PRODUCT_VOXEL_ATLAS_ALIGNMENT, g._check_args)
        return None if hold is None else DeviceAtlasAlignments(hold, tuple(int(v) for v in out))

    def score_alignments(self, cloud, transforms, dilate=0, weights=ALIGN_DEFAULT_WEIGHTS, origin_voxels=None, center=None):
        """Gvom.score_alignments() against the atlas -- relocalising on remembered space: the same cloud, candidates, dilate and
        weights, held against the window-sized box whose corner is origin_voxels or the window of a scan with its ego at `center`
        (both as in box(); default: the last integrated window).  A voxel's class is the atlas's: occupied, near (dilate=1: an
        occupied voxel anywhere in the extent within one voxel on every axis), free, never observed (also: outside the extent);
        "outside" is outside the box.  Returns a DeviceAtlasAlignments; None before the first combine and, without an origin, before
        the first integrate."""
        c = _align_cloud(cloud)
        t = _align_transforms(transforms)
        return self._score_alignments(_ptr(c), c.shape[0], _ptr(t), t.shape[0], 0, dilate, weights, origin_voxels, center)

    def score_alignments_device(self, cloud_ptr, n, transforms_ptr, K, dilate=0, weights=ALIGN_DEFAULT_WEIGHTS, origin_voxels=None, center=None):
        """The same for inputs in device memory, as Gvom.score_alignments_device().  Enqueues and returns: no host wait."""
        if not cloud_ptr or not transforms_ptr:
            raise ValueError("cloud_ptr and transforms_ptr must be device addresses")
        return self._score_alignments(_dev(cloud_ptr), n, _dev(transforms_ptr), K, 1, dilate, weights, origin_voxels, center)

    def _raycast(self, from_ptr, K, to_ptr, n, on_device, unknown_blocks, check_target):
        g = self._owner
        e = (_I64 * 3)()
        flags = _ray_flags(unknown_blocks, check_target)
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_atlas_raycast(g._h, from_ptr, int(K), to_ptr, int(n), int(on_device), flags, e, pid),
                               PRODUCT_VOXEL_ATLAS_RAYS, g._check_args)
        return None if hold is None else DeviceAtlasRays(hold, tuple(int(v) for v in e))

    def raycast(self, origins, targets, unknown_blocks=False, check_target=False):
        """Gvom.raycast() through the atlas: the same segments, flags and ray rule, with the extent in the window's place -- a ray
        stops at the first remembered occupied voxel, never-observed voxels count as unknown, RAY_LEFT_WINDOW means it left the
        extent.  Returns a DeviceAtlasRays; None before the first combine."""
        o, t = _ray_segments(origins, targets)
        return self._raycast(_ptr(o), o.shape[0], _ptr(t), t.shape[0], 0, unknown_blocks, check_target)

    def raycast_device(self, from_ptr, K, to_ptr, n, unknown_blocks=False, check_target=False):
        """The same for segments in device memory, as Gvom.raycast_device().  Enqueues and returns: no host wait."""
        if not from_ptr or not to_ptr:
            raise ValueError("from_ptr and to_ptr must be device addresses")
        return self._raycast(_dev(from_ptr), K, _dev(to_ptr), n, 1, unknown_blocks, check_target)

    def _score_viewpoints(self, poses_ptr, K, on_device, max_range, beam_stride, unknown_blocks, host_poses=None):
        g = self._owner
        K, r, sh, sw = _viewpoint_options(K, max_range, beam_stride)
        e = (_I64 * 3)()
        flags = _ray_flags(unknown_blocks)
        hold = g._make_product(lambda pid: g._lib.gvom_voxel_atlas_score_viewpoints(g._h, poses_ptr, K, int(on_device), r, sh, sw, flags, e, pid),
                               PRODUCT_VOXEL_ATLAS_VIEWPOINTS, g._check_args)
        return None if hold is None else DeviceAtlasViewpoints(hold, tuple(int(v) for v in e), host_poses)

    def score_viewpoints(self, poses, max_range, beam_stride=(1, 1), unknown_blocks=False):
        """Gvom.score_viewpoints() through the atlas: the same poses, sensor model, strides and flag; the gain of a pose is the number
        of DISTINCT never-observed world voxels its beams pass anywhere in the extent -- the last step of the exploration loop
        atlas field -> frontiers -> viewpoint_poses() -> score_viewpoints() -> best_pose() for goals outside the window.  Returns a
        DeviceAtlasViewpoints; None before the first combine."""
        t = _viewpoint_poses(poses)
        return self._score_viewpoints(_ptr(t), t.shape[0], 0, max_range, beam_stride, unknown_blocks, t)

    def score_viewpoints_device(self, poses_ptr, K, max_range, beam_stride=(1, 1), unknown_blocks=False):
        """The same for poses in device memory, as Gvom.score_viewpoints_device().  The library reads the poses back (K x 96 bytes):
        this route waits for the mapper's stream."""
        if not poses_ptr:
            raise ValueError("poses_ptr must be a device address")
        return self._score_viewpoints(_dev(poses_ptr), K, 1, max_range, beam_stride, unknown_blocks)

    def clear(self):
        """Every voxel becomes VOXEL_NEVER and the counters 0; the extent and seq stay."""
        g = self._owner
        g._check_args(g._lib.gvom_voxel_atlas_clear(g._h))

    def counts(self):
        """Waits for the GPU.  A dict (VOXEL_ATLAS_COUNTS): of the last integrate `first_seen`, `free_to_occupied`, `occupied_to_free`,
        `confirmed`, `uninformative`, `outside` (they sum to the window's voxels), `cleared` and `cleared_observed` (by the move); of the
        atlas `observed`, `occupied` and `seq`."""
        g = self._owner
        out = (_I64 * 11)()
        g._check_args(g._lib.gvom_voxel_atlas_counts(g._h, out))
        return dict(zip(VOXEL_ATLAS_COUNTS, (int(v) for v in out)))

    def release(self):
        """Frees the atlas's device memory."""
        g = self._owner
        if g._h:
            g._check_args(g._lib.gvom_voxel_atlas_configure(g._h, 0, 0, 0, None))


class _OutputPool(object):
    """Free pinned output buffers of one Gvom.  Outlives the Gvom if returned arrays do: a buffer that
    comes back after the mapper is gone is released at once (pinned host memory is not tied to the
    handle: hipHostFree works without it)."""

    def __init__(self):
        self.free = []
        self.closed = False

    def give_back(self, ptr):
        if not self.closed:
            self.free.append(ptr)           # recycled by the next combine_maps
        else:
            _host_free(ptr)


def _host_free(ptr):
    try:
        rt = ctypes.CDLL("libamdhip64.so")
        rt.hipHostFree.argtypes = [ctypes.c_void_p]
        rt.hipHostFree(ctypes.c_void_p(ptr))
    except Exception:
        pass


class _PinnedOutput(object):
    """One pinned, device-mapped output buffer of combine_maps.  The four returned numpy arrays
    are views whose base chain ends here; when the caller drops them all, the buffer goes back to
    the owning Gvom's pool (so every call still returns FRESH arrays, as the reference does) -- or is
    freed, if that Gvom no longer exists."""

    def __init__(self, owner_pool, ptr, nbytes):
        self._pool = owner_pool
        self.ptr = ptr
        self.__array_interface__ = {"data": (ptr, False), "shape": (nbytes,), "typestr": "|u1",
                                    "version": 3}

    def __del__(self):
        pool = self._pool
        if pool is not None:
            pool.give_back(self.ptr)


def _map_views(raw, xy):
    """(positive, negative, roughness, visibility) of the pinned output buffer `raw` (uint8) a combine writes: [xy, xy] views of it"""
    n2 = xy * xy
    # the library writes the maps in [y][x] memory order: seen through .T they are the reference's
    # [x, y]-indexed arrays in Fortran order (what gvom_ros.py's reshape(..., order='F') reads
    # without a copy), and the GPU writes them as contiguous runs without a transpose
    positive = np.ndarray((xy, xy), np.int32, raw, 0, (4, 4 * xy))
    negative = np.ndarray((xy, xy), np.int32, raw, 4 * n2, (4, 4 * xy))
    visibility = np.ndarray((xy, xy), np.int32, raw, 8 * n2, (4, 4 * xy))
    roughness = np.ndarray((xy, xy), np.float64, raw, 12 * n2, (8, 8 * xy))
    return positive, negative, roughness, visibility


def _occupancy_grids(raw, xy):
    """(hard, soft, certainty, negative, roughness) of the buffer an occupancy combine writes: five int8 [xy * xy] views of it"""
    n2 = xy * xy
    return tuple(raw[k * n2:(k + 1) * n2].view(np.int8) for k in range(5))


def transform_from_translation_rotation(translation, rotation):
    """4x4 matrix of a translation (x, y, z) and a quaternion (x, y, z, w): what the node builds with
    tf.TransformerROS.fromTranslationRotation (gvom_ros.py:105).  Restates tf.transformations
    (ROS geometry 1.13, not part of the reference checkout): translation_matrix @ quaternion_matrix,
    with quaternion_matrix's normalisation q *= sqrt(2 / q.q) and its near-zero quaternion -> identity."""
    q = np.array(rotation[:4], dtype=np.float64, copy=True)
    nq = np.dot(q, q)
    if nq < np.finfo(float).eps * 4.0:
        r = np.identity(4)
    else:
        q *= np.sqrt(2.0 / nq)
        q = np.outer(q, q)
        r = np.array(((1.0 - q[1, 1] - q[2, 2], q[0, 1] - q[2, 3], q[0, 2] + q[1, 3], 0.0),
                      (q[0, 1] + q[2, 3], 1.0 - q[0, 0] - q[2, 2], q[1, 2] - q[0, 3], 0.0),
                      (q[0, 2] - q[1, 3], q[1, 2] + q[0, 3], 1.0 - q[0, 0] - q[1, 1], 0.0),
                      (0.0, 0.0, 0.0, 1.0)), dtype=np.float64)
    t = np.identity(4)
    t[:3, 3] = translation[:3]
    return np.dot(t, r)


class _PendingMaps(object):
    """A combine begun with Gvom.combine_maps_async() / combine_maps_occupancy_async(); result() completes
    it (once)."""

    def __init__(self, owner, holder, occupancy=False):
        self._owner, self._holder, self._out, self._done = owner, holder, None, holder is None
        self._occupancy = occupancy

    def result(self):
        if not self._done:
            g = self._owner
            origin = np.zeros(3, np.float64)
            g._check(g._lib.gvom_combine_end(g._h, _ptr(origin)))
            views = _occupancy_grids if self._occupancy else _map_views
            self._out = (origin,) + views(np.asarray(self._holder), g.xy_size)
            self._done, self._holder = True, None
        return self._out

    def __del__(self):
        # a handle dropped without result(): end the combine so that the mapper accepts the next one
        try:
            if not self._done and self._owner._h:
                self._owner._lib.gvom_combine_end(self._owner._h, None)
        except Exception:
            pass


class Gvom(object):
    """A class to convert lidar pointclouds into a cost map (reference gvom.py:12-27).

    The 14 positional arguments are the reference's (gvom.py:29-31).  Keyword arguments of this implementation:
      device            HIP device of the map (default 0)
      voxel_statistics  the per-voxel mean / covariance path behind make_debug_voxel_map (gvom.py:159, 276-284, 363-378).
                        None (default): ON DEMAND -- it runs from the first scan on, as in the reference, for as long as somebody
                        reads it (make_debug_voxel_map, voxel_cloud_device, metrics_buffer, combined_metrics,
                        voxels_eigenvalues: the unchanged node does every tick, gvom_ros.py:171; read_dense, the returned maps
                        and the other debug products are not reads); the FOURTH combine in a row with no read before it
                        switches it off and merges no statistics (the scans then cost what the north-star path costs), a later
                        read returns None once and switches it on again for the scans that follow; the fused map has statistics
                        again once every filled ring slot was scanned with them -- restarted from the ring: a voxel only the
                        map from before knows has an all-zero row (count 0) until a scan reaches its neighbourhood.  A reader
                        of every fourth combine or fewer never gets data: pin them with True.  True: always.  False: never
                        (make_debug_voxel_map returns None).
      c_order           False (default): combine_maps returns the four maps as FORTRAN-ordered views of pinned host memory the
                        GPU has written -- same [x, y] indexing, shapes, dtypes and values as the reference's arrays; its
                        caller flattens them with order='F' (gvom_ros.py:141-162), which is then a no-copy reshape.  True:
                        C-contiguous arrays of their own, as the reference's copy_to_host() returns (gvom.py:352-354).
      numba_cuda_typing the types Numba infers for a REAL CUDA device where they differ from its simulator's (which the golden
                        fixtures were recorded under): ray_length = sqrt(float32) in float32, slope / ray_length in float32,
                        the loop bound from that float32 (gvom.py:1109-1114, 1127; profiles/numba_cuda_typing.txt, INTEGRATION.md
                        section 5).  cuda_f32_sqrt: the name this switch had before round 6."""

    def __init__(self, xy_resolution, z_resolution, xy_size, z_size, buffer_size, min_distance,
                 positive_obstacle_threshold, negative_obstacle_threshold, slope_obstacle_threshold,
                 robot_height, robot_radius, ground_to_lidar_height, xy_eigen_dist, z_eigen_dist,
                 device=0, voxel_statistics=None, numba_cuda_typing=False, c_order=False, _shard=None, _library=None, cuda_f32_sqrt=None):
        self.xy_resolution = xy_resolution
        self.z_resolution = z_resolution
        self.xy_size = xy_size
        self.z_size = z_size
        self.voxel_count = self.xy_size * self.xy_size * self.z_size
        self.min_distance = min_distance
        self.positive_obstacle_threshold = positive_obstacle_threshold
        self.negative_obstacle_threshold = negative_obstacle_threshold
        self.slope_obstacle_threshold = slope_obstacle_threshold
        self.robot_height = robot_height
        self.robot_radius = robot_radius
        self.ground_to_lidar_height = ground_to_lidar_height
        self.xy_eigen_dist = xy_eigen_dist
        self.z_eigen_dist = z_eigen_dist
        self.metrics_count = 10
        self.buffer_size = buffer_size
        self.threads_per_block = 256
        self.threads_per_block_3D = (8, 8, 4)
        self.threads_per_block_2D = (16, 16)
        self.blocks = math.ceil(self.voxel_count / self.threads_per_block)          # gvom.py:94
        self.ego_position = [0, 0, 0]
        # reference attributes that guard ITS buffers (gvom.py:65-67, 96) or hold a placeholder (gvom.py:54): inert here -- the
        # library serialises per handle with its own mutex -- but present, for callers that touch them
        self.semaphores = [threading.Semaphore() for _ in range(int(buffer_size))]
        self.ego_semaphore = threading.Semaphore()
        self.metrics = _DeviceArrayView(lambda: np.array([[3, 2]]))
        self._c_order = bool(c_order)
        self._device = int(device)
        if cuda_f32_sqrt is not None:
            numba_cuda_typing = bool(cuda_f32_sqrt)

        self._lib = load_library(_library)
        self._h = ctypes.c_void_p()
        stat_flags = 4 if (voxel_statistics is None and _shard is None) else (1 if voxel_statistics else 0)
        prm = GvomParams(float(xy_resolution), float(z_resolution), int(xy_size), int(z_size),
                         int(buffer_size), stat_flags | (2 if numba_cuda_typing else 0), float(min_distance),
                         float(positive_obstacle_threshold), float(negative_obstacle_threshold),
                         float(slope_obstacle_threshold), float(robot_height), float(robot_radius),
                         float(ground_to_lidar_height), int(xy_eigen_dist), int(z_eigen_dist))
        if _shard is None:
            rc = self._lib.gvom_create(ctypes.byref(prm), int(device), ctypes.byref(self._h))
        else:
            rc = self._lib.gvom_create_sharded(ctypes.byref(prm), int(device), int(_shard[0]),
                                               int(_shard[1]), ctypes.byref(self._h))
        self._out_pool = _OutputPool()      # free pinned output buffers (host pointers)
        if rc != GVOM_OK:
            info = ctypes.create_string_buffer(256)
            self._lib.gvom_backend_info(info, 256)
            self._h = ctypes.c_void_p()
            raise GvomBackendError("gvom_create failed with code %d (%s). There is no CPU fallback."
                                   % (rc, info.value.decode()))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                # idle buffers go now; those still referenced by live arrays are freed by the pool when
                # the last array of their call is collected
                pool = getattr(self, "_out_pool", None)
                if pool is not None:
                    pool.closed = True
                    for p in pool.free:
                        self._lib.gvom_output_buffer_free(h, _dev(p))
                    pool.free = []
                self._lib.gvom_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            raise GvomBackendError("libgvom_hip call failed (%d): %s"
                                   % (rc, self._lib.gvom_last_error(self._h).decode()))
        return rc

    @staticmethod
    def _prepare_cloud(pointcloud):
        """(array, n, row_stride_bytes, dtype_code).  float32/float64 rows of >= 3 columns are
        passed without a copy when C-contiguous in the last axis; anything else is converted to
        float64 (what ros_numpy delivers, gvom_ros.py:108)."""
        pc = pointcloud if isinstance(pointcloud, np.ndarray) else np.asarray(pointcloud)
        if pc.ndim != 2 or pc.shape[1] < 3:
            raise ValueError("pointcloud must have shape (N, >=3), got %r" % (pc.shape,))
        if pc.dtype not in (np.float32, np.float64):
            pc = pc.astype(np.float64)
        if pc.shape[0] > 0 and (pc.strides[1] != pc.itemsize or pc.strides[0] < 3 * pc.itemsize
                                or pc.strides[0] % pc.itemsize):
            pc = np.ascontiguousarray(pc)
        stride = pc.strides[0] if pc.shape[0] > 0 else 3 * pc.itemsize
        return pc, pc.shape[0], stride, (0 if pc.dtype == np.float32 else 1)

    def _scan_frame(self, ego_position, transform):
        """The frame arguments of a scan, as every scan route hands them to the library: (ego, tf) = ego_position as double[3]
        and `transform` as a C-contiguous float64 4x4 array, or None.  Keeps ego_position (the reference's attribute).  The
        library reads tf[0..11], so anything but a 4x4 matrix is refused here."""
        tf = None
        if transform is not None:
            tf = np.ascontiguousarray(np.asarray(transform, dtype=np.float64))
            if tf.shape != (4, 4):
                raise ValueError("transform must be 4x4")
        self.ego_position = ego_position
        return (ctypes.c_double * 3)(float(ego_position[0]), float(ego_position[1]), float(ego_position[2])), tf

    def process_pointcloud(self, pointcloud, ego_position, transform=None):
        """Imports a pointcloud, processes it into a voxel map then adds the map to the buffer
        (reference gvom.py:99-175).  Returns None."""
        pc, n, stride, code = self._prepare_cloud(pointcloud)
        ego, tf = self._scan_frame(ego_position, transform)
        _warn_scan(self._check(self._lib.gvom_process_pointcloud(self._h, _ptr(pc) if n else None, n,
                                                                 stride, code, ego, _ptr(tf))))
        return None

    def process_pointcloud_device(self, dev_ptr, n, dtype, ego_position, transform=None,
                                  row_stride_bytes=None):
        """Same as process_pointcloud for a cloud already resident in HBM (raw device pointer)."""
        code, stride = _device_cloud(dtype, row_stride_bytes)
        ego, tf = self._scan_frame(ego_position, transform)
        return self._check(self._lib.gvom_process_pointcloud_device(
            self._h, _dev(dev_ptr), int(n), int(stride), code, ego, _ptr(tf)))

    # ---- multi-origin scans: every return traced from its own sensor position (include/gvom_hip.h "multi-origin scans") ----
    def process_pointcloud_origins(self, pointcloud, origins, ego_position, transform=None, origin_index=None):
        """process_pointcloud with return i traced from origins[origin_index[i]] instead of from ego_position, which keeps
        every other role (it places the window).  origins [K, 3] world-frame sensor positions (`transform` is not applied to
        them), 1 <= K <= 65536; origin_index [N] integers below K, or None: return i belongs to origin i % K.  Returns None."""
        pc, n, stride, code = self._prepare_cloud(pointcloud)
        o = _origin_table(origins)
        idx = None
        if origin_index is not None:
            raw = np.asarray(origin_index)
            if raw.shape != (n,):
                raise ValueError("origin_index must have shape (%d,), got %r" % (n, raw.shape))
            if n and (raw.min() < 0 or raw.max() >= o.shape[0]):
                raise ValueError("origin_index entries must lie in [0, %d)" % o.shape[0])
            idx = np.ascontiguousarray(raw.astype(np.uint16))
        ego, tf = self._scan_frame(ego_position, transform)
        _warn_scan(self._check_args(self._lib.gvom_process_pointcloud_origins(
            self._h, _ptr(pc) if n else None, 0, n, stride, code, _ptr(o), o.shape[0], _ptr(idx), ego, _ptr(tf))))
        return None

    def process_pointcloud_origins_device(self, dev_ptr, n, dtype, origins, ego_position, transform=None,
                                          origin_index_ptr=None, row_stride_bytes=None):
        """process_pointcloud_origins for a cloud already resident in HBM.  origins: a HOST [K, 3] array; origin_index_ptr: a raw
        device pointer to n uint16, or None (i % K).  The device index cannot be checked by the host: a return whose index is
        not below K has no effect at all."""
        code, stride = _device_cloud(dtype, row_stride_bytes)
        o = _origin_table(origins)
        ego, tf = self._scan_frame(ego_position, transform)
        return self._check_args(self._lib.gvom_process_pointcloud_origins(
            self._h, _dev(dev_ptr), 1, int(n), int(stride), code, _ptr(o), o.shape[0], _dev(origin_index_ptr), ego, _ptr(tf)))

    def _check_args(self, rc):
        """_check, with GVOM_ERR_INVALID (-1) as the ValueError the binding's own argument checks raise"""
        if rc == GVOM_ERR_INVALID:
            raise ValueError("libgvom_hip: invalid argument: %s" % self._lib.gvom_last_error(self._h).decode())
        return self._check(rc)

    # ---- ingest side of the ROS node (reference gvom_ros.py:93-109) ----------
    def process_pointcloud2(self, data, n_points, point_step, offsets, ego_position, transform=None,
                            field_dtype=np.float32):
        """Scans the packed bytes of a sensor_msgs/PointCloud2 directly: `data` (bytes / buffer) holds
        n_points records of point_step bytes with little-endian x, y, z fields of `field_dtype`
        (float32 = PointField.FLOAT32, float64 = FLOAT64) at byte `offsets` (x, y, z).  Equivalent to
            pc = ros_numpy.point_cloud2.pointcloud2_to_xyz_array(msg)     # gvom_ros.py:108
            self.process_pointcloud(pc, ego_position, transform)          # gvom_ros.py:109
        (ros_numpy hands over a float64 array with the non-finite records removed; here FLOAT32
        fields are widened on the GPU and non-finite records have no effect on the map)."""
        buf = np.frombuffer(data, dtype=np.uint8)
        if buf.size < int(n_points) * int(point_step):
            raise ValueError("PointCloud2 data shorter than n_points * point_step")
        code = 0 if np.dtype(field_dtype) == np.float32 else 1
        ego, tf = self._scan_frame(ego_position, transform)
        _warn_scan(self._check(self._lib.gvom_process_pointcloud2(
            self._h, ctypes.c_void_p(buf.ctypes.data), int(n_points), int(point_step),
            int(offsets[0]), int(offsets[1]), int(offsets[2]), code, ego, _ptr(tf))))
        return None

    def process_pointcloud2_msg(self, msg, ego_position, transform=None):
        """process_pointcloud2 for a sensor_msgs/PointCloud2-like object (fields[].name/offset/datatype,
        point_step, row_step, width, height, data, is_bigendian)."""
        f = {fd.name: fd for fd in msg.fields}
        kinds = {f[k].datatype for k in "xyz"}
        if getattr(msg, "is_bigendian", False) or len(kinds) != 1 or not kinds <= {7, 8}:
            raise ValueError("x, y, z must be little-endian FLOAT32 (7) or FLOAT64 (8) fields of one type")
        if msg.height > 1 and msg.row_step != msg.width * msg.point_step:
            raise ValueError("row padding is not supported")
        return self.process_pointcloud2(msg.data, msg.width * msg.height, msg.point_step,
                                        (f["x"].offset, f["y"].offset, f["z"].offset), ego_position,
                                        transform, np.float32 if kinds == {7} else np.float64)

    # ---- range images: the scan as a spinning multi-beam lidar emits it (include/gvom_hip.h "range images") ----------
    def set_sensor_model(self, directions, offsets=None, range_scale=0.001, min_range=0.0, max_range=float("inf")):
        """The sensor's per-pixel lookup table, once (or whenever it changes): directions [H, W, 3] (unit vectors), offsets
        [H, W, 3] metres or None, range_scale metres per raw unit, the inclusive range gate.  The arrays are copied to the GPU."""
        d = np.ascontiguousarray(np.asarray(directions, dtype=np.float64))
        if d.ndim != 3 or d.shape[2] != 3 or d.shape[0] < 1 or d.shape[1] < 1:
            raise ValueError("directions must have shape (H, W, 3), got %r" % (d.shape,))
        o = None
        if offsets is not None:
            o = np.ascontiguousarray(np.asarray(offsets, dtype=np.float64))
            if o.shape != d.shape:
                raise ValueError("offsets must have the shape of directions %r, got %r" % (d.shape, o.shape))
        if not (float(range_scale) > 0.0 and math.isfinite(float(range_scale))):
            raise ValueError("range_scale must be finite and > 0")
        self._check(self._lib.gvom_sensor_model_set(self._h, d.shape[0], d.shape[1], _ptr(d), _ptr(o), float(range_scale),
                                                    float(min_range), float(max_range)))
        self._sensor_shape = (d.shape[0], d.shape[1])

    def _range_image_call(self, raw_ptr, on_device, rcode, stride, ego_position, transform, column_transforms, cloud_dtype,
                          trace_from_columns=False):
        if trace_from_columns and column_transforms is None:
            raise ValueError("process_range_image_origins needs column_transforms (the sensor's pose per column)")
        shape = getattr(self, "_sensor_shape", None)
        poses = _column_poses(column_transforms, shape[1]) if (column_transforms is not None and shape) else None
        ego, tf = self._scan_frame(ego_position, transform)
        if trace_from_columns:
            rc = self._check_args(self._lib.gvom_process_range_image_origins(self._h, raw_ptr, int(on_device), rcode, int(stride),
                                                                             _ptr(poses), _cloud_code(cloud_dtype), ego, _ptr(tf)))
        else:
            rc = self._check(self._lib.gvom_process_range_image(self._h, raw_ptr, int(on_device), rcode, int(stride), _ptr(poses),
                                                                _cloud_code(cloud_dtype), ego, _ptr(tf)))
        _warn_scan(rc)
        return None

    def process_range_image(self, ranges, ego_position, transform=None, column_transforms=None, cloud_dtype=np.float32):
        """process_pointcloud for a range image: `ranges` [H, W] uint16 / uint32 / float32 raw ranges of the sensor whose model
        set_sensor_model has handed over (0 = no return), any row stride; column_transforms [W, 4, 4] or [W, 3, 4]: one pose
        per column (the sweep's de-skew), applied before `transform`.  Equivalent to
            self.process_pointcloud(unproject_range_image(ranges, <the model>, column_transforms, cloud_dtype), ego_position, transform)
        with the unprojection done on the GPU and 2 or 4 bytes per pixel uploaded.  Returns None."""
        return self._range_image_host(ranges, ego_position, transform, column_transforms, cloud_dtype, False)

    def process_range_image_origins(self, ranges, ego_position, transform=None, column_transforms=None, cloud_dtype=np.float32):
        """process_range_image with every pixel's ray starting at its column's sensor position -- column_origins(
        column_transforms, transform) -- instead of at ego_position, as process_pointcloud_origins traces it.
        column_transforms is required.  Returns None."""
        return self._range_image_host(ranges, ego_position, transform, column_transforms, cloud_dtype, True)

    def _range_image_host(self, ranges, ego_position, transform, column_transforms, cloud_dtype, trace_from_columns):
        raw = ranges if isinstance(ranges, np.ndarray) else np.asarray(ranges)
        rcode = _range_code(raw.dtype)
        if raw.ndim != 2 or raw.shape[0] < 1 or raw.shape[1] < 1:
            raise ValueError("ranges must have shape (H, W), got %r" % (raw.shape,))
        shape = getattr(self, "_sensor_shape", None)
        if shape is not None and tuple(raw.shape) != shape:
            raise ValueError("ranges have shape %r, the sensor model %r" % (tuple(raw.shape), shape))
        if raw.strides[1] != raw.itemsize or raw.strides[0] < raw.shape[1] * raw.itemsize or raw.strides[0] % raw.itemsize:
            raise ValueError("ranges must be C-contiguous in the last axis with rows a whole number of elements apart")
        if shape is None and column_transforms is not None:
            _column_poses(column_transforms, raw.shape[1])
        return self._range_image_call(_ptr(raw), 0, rcode, raw.strides[0], ego_position, transform, column_transforms, cloud_dtype,
                                      trace_from_columns)

    def process_range_image_device(self, dev_ptr, range_dtype, ego_position, transform=None, column_transforms=None,
                                   cloud_dtype=np.float32, row_stride_bytes=None):
        """process_range_image for an image already resident in HBM (raw device pointer, the model's H x W pixels of
        `range_dtype`, rows row_stride_bytes apart; default: packed).  The data must be ready when the call is made."""
        return self._range_image_device(dev_ptr, range_dtype, ego_position, transform, column_transforms, cloud_dtype, row_stride_bytes,
                                        False)

    def process_range_image_origins_device(self, dev_ptr, range_dtype, ego_position, transform=None, column_transforms=None,
                                           cloud_dtype=np.float32, row_stride_bytes=None):
        """process_range_image_origins for an image already resident in HBM (see process_range_image_device)."""
        return self._range_image_device(dev_ptr, range_dtype, ego_position, transform, column_transforms, cloud_dtype, row_stride_bytes,
                                        True)

    def _range_image_device(self, dev_ptr, range_dtype, ego_position, transform, column_transforms, cloud_dtype, row_stride_bytes,
                            trace_from_columns):
        rcode = _range_code(range_dtype)
        shape = getattr(self, "_sensor_shape", None)
        stride = row_stride_bytes or ((shape[1] if shape else 0) * np.dtype(range_dtype).itemsize)
        return self._range_image_call(_dev(dev_ptr), 1, rcode, stride, ego_position, transform, column_transforms, cloud_dtype,
                                      trace_from_columns)

    def combine_maps(self):
        """Combines all maps in the buffer and processes the resultant map into 2D maps
        (reference gvom.py:177-354).  Returns None or (origin_world f64[3], positive i32[xy,xy],
        negative i32[xy,xy], roughness f64[xy,xy], visibility i32[xy,xy])."""
        if self._c_order:
            xy = self.xy_size
            origin = np.zeros(3, np.float64)
            positive, negative, visibility = (np.empty((xy, xy), np.int32) for _ in range(3))
            roughness = np.empty((xy, xy), np.float64)
            rc = self._check(self._lib.gvom_combine_maps(self._h, _ptr(origin), _ptr(positive), _ptr(negative), _ptr(roughness),
                                                         _ptr(visibility)))
            out = (origin, positive, negative, roughness, visibility)
        else:
            rc, out = self._combine_into(self._lib.gvom_combine_maps_into)
        if rc == GVOM_EMPTY_BUFFER:
            _warn_empty_ring()
            return None
        return out

    def combine_maps_device(self):
        """combine_maps() with the maps left in device memory (an extension, for consumers on the GPU): advances the fusion
        exactly like combine_maps() and returns None (empty ring, with the same warning) or a DeviceMaps -- nine maps, each
        shareable with torch.from_dlpack() without a copy.  Returns once the work is enqueued: no host wait."""
        origin = np.zeros(3, np.float64)
        sid = ctypes.c_int64(-1)
        rc = self._check(self._lib.gvom_combine_maps_device(self._h, _ptr(origin), ctypes.byref(sid)))
        if rc == GVOM_EMPTY_BUFFER:
            _warn_empty_ring()
            return None
        return DeviceMaps(self, int(sid.value), origin)

    def _output_buffer(self):
        """A pinned output buffer for one combine -- one the pool has free, else a new one -- in the holder that gives it back to the
        pool once the last view of it is dropped; `.ptr` is its host address."""
        if self._out_pool.free:
            ptr = self._out_pool.free.pop()
        else:
            p = ctypes.c_void_p()
            self._check(self._lib.gvom_output_buffer_alloc(self._h, ctypes.byref(p)))
            ptr = p.value
        return _PinnedOutput(self._out_pool, ptr, self.xy_size * self.xy_size * 20)

    def _combine_begin(self, occupancy):
        """the two *_async methods: `occupancy` is None for the four maps, the double[3] of thresholds for the five grids"""
        holder = self._output_buffer()
        rc = self._check(self._lib.gvom_combine_begin(self._h, _dev(holder.ptr), occupancy))
        if rc == GVOM_EMPTY_BUFFER:
            _warn_empty_ring()
            return _PendingMaps(self, None)
        return _PendingMaps(self, holder, occupancy=occupancy is not None)

    def combine_maps_async(self):
        """combine_maps() split in two (an extension; the reference's call is synchronous): enqueues the
        combine and returns a handle at once; `.result()` waits and returns what combine_maps() returns.
        Hand the next scan to process_pointcloud*() in between: its ray tracing runs on the GPU while the
        maps of this combine are written to host memory.  One combine may be pending at a time."""
        return self._combine_begin(None)

    def combine_maps_occupancy_async(self, density_threshold=50, min_roughness=-10, max_roughness=0):
        """combine_maps_occupancy() split like combine_maps_async(): `.result()` returns its tuple."""
        return self._combine_begin((ctypes.c_double * 3)(float(density_threshold), float(min_roughness), float(max_roughness)))

    def combine_maps_occupancy(self, density_threshold=50, min_roughness=-10, max_roughness=0):
        """combine_maps() fused with the post-processing the ROS node applies to its result
        (reference gvom_ros.py:141-165).  Advances the map exactly like
        combine_maps() and returns None (empty ring) or
            (origin_world f64[3], hard, soft, certainty, negative, roughness)
        where each grid is the int8[xy*xy] array the node assigns to nav_msgs/OccupancyGrid.data
        (x fastest, i.e. np.reshape(m, -1, order='F')).  Defaults = the node's ROS parameter
        defaults (gvom_ros.py:32-35).  5 bytes per cell cross PCIe instead of 20."""
        origin = np.zeros(3, np.float64)
        holder = self._output_buffer()
        rc = self._check(self._lib.gvom_combine_occupancy_into(
            self._h, _ptr(origin), _dev(holder.ptr), float(density_threshold),
            float(min_roughness), float(max_roughness)))
        if rc == GVOM_EMPTY_BUFFER:
            _warn_empty_ring()
            return None
        return (origin,) + _occupancy_grids(np.asarray(holder), self.xy_size)

    def _combine_into(self, entry_point):
        """Runs `entry_point(handle, origin, pinned_buffer)` and wraps the pinned buffer as the
        reference's return tuple.  The GPU writes the four maps straight into a pinned,
        device-mapped host buffer; the returned arrays are views of it (fresh per call: a buffer
        is reused only after every array of an earlier call has been garbage-collected)."""
        origin = np.zeros(3, np.float64)
        holder = self._output_buffer()
        # The views are built BEFORE the (blocking) call: k_encode is still running on the GPU when
        # combine_maps is entered, so this host work is hidden; after the call only the return is left.
        out = (origin,) + _map_views(np.asarray(holder), self.xy_size)
        rc = self._check(entry_point(self._h, _ptr(origin), _dev(holder.ptr)))
        if rc != GVOM_OK:
            return rc, None
        return GVOM_OK, out

    # ---- accessors / debug API (reference gvom.py:356-410) ------------------------------
    def get_map_as_occupancy_grid(self):
        out = np.empty((self.xy_size, self.xy_size, self.z_size), np.uint8)
        rc = self._check(self._lib.gvom_get_occupancy(self._h, _ptr(out)))
        if rc == GVOM_NO_DATA:
            raise AttributeError("'NoneType' object has no attribute 'copy_to_host'")  # as the reference
        return out.astype(bool)

    # ---- the same four, left in device memory (extensions; include/gvom_hip.h "device-resident 3-D products") ----
    def _make_product(self, call, kind, check=None):
        """What the four makers share: `call(product id, by reference)` runs the entry point; the hold on the product of `kind` it
        made, or None where it had no data."""
        pid = ctypes.c_int64(-1)
        rc = (check or self._check)(call(ctypes.byref(pid)))
        return None if rc == GVOM_NO_DATA else _ProductHold(self, kind, int(pid.value))

    def _device_product(self, kind, max_rows=0):
        return self._make_product(lambda pid: self._lib.gvom_device_product(self._h, kind, int(max_rows), pid), kind)

    def occupancy_grid_device(self):
        """get_map_as_occupancy_grid() left in device memory: a DeviceArray uint8 [xy, xy, z] (1 = occupied), a snapshot of the
        current fused map shareable with torch.from_dlpack() without a copy; None before the first combine.  Returns once the
        work is enqueued: no host wait."""
        hold = self._device_product(PRODUCT_OCCUPANCY)
        return None if hold is None else DeviceArray(hold)

    def voxel_cloud_device(self, max_rows=None):
        """make_debug_voxel_map() left in device memory: a DeviceVoxelCloud (rows, eigenvalues, row count) of at most max_rows
        rows (default: the fused cell count); None ("No data" before the first combine) under make_debug_voxel_map's conditions.
        Counts as a read of the per-voxel statistics: statistics on demand stay on while this is called."""
        return self._debug_cloud_device(PRODUCT_VOXEL_CLOUD, DeviceVoxelCloud, 0 if max_rows is None else max(int(max_rows), 1), True)

    def _debug_cloud_device(self, kind, view, max_rows=0, only_before_combine=False):
        """What the three debug-cloud makers share: `view` of the product of `kind`, or None and the reference's "No data" where the
        mapper has none (only_before_combine: said only before the first combine, as make_debug_voxel_map does)."""
        hold = self._device_product(kind, max_rows)
        if hold is None:
            if not (only_before_combine and self._state().has_combined):
                print("No data")
            return None
        return view(hold)

    def height_cloud_device(self):
        """make_debug_height_map() left in device memory: a DeviceArray float32 [xy*xy, 7]; None (and "No data") without 2-D maps."""
        return self._debug_cloud_device(PRODUCT_HEIGHT_CLOUD, DeviceArray)

    def inferred_height_cloud_device(self):
        """make_debug_inferred_height_map() left in device memory: a DeviceArray float32 [xy*xy, 3]; None (and "No data") without 2-D maps."""
        return self._debug_cloud_device(PRODUCT_INFERRED_HEIGHT_CLOUD, DeviceArray)

    def _window_map(self, name, m, dtype, bounds=None, optional=False, range_note=""):
        """An [x, y] map of the caller's over the window, as the library reads it: a Fortran-ordered (x fastest) array of `dtype`;
        None for an absent `optional` map.  bounds = (lo, hi): the map must hold finite whole numbers in lo .. hi; without
        bounds the values are cast as they are.  range_note: what the range message adds about the values."""
        if m is None:
            if optional:
                return None
            raise ValueError("%s must be an array" % name)
        a = np.asarray(m)
        if a.shape != (self.xy_size, self.xy_size):
            raise ValueError("%s must have shape (%d, %d), got %r" % (name, self.xy_size, self.xy_size, a.shape))
        if bounds is not None:
            if a.dtype.kind == "f" and not np.isfinite(a).all():
                raise ValueError("%s must be finite" % name)
            if a.dtype.kind not in "iuf" or (a.dtype.kind == "f" and (a != np.floor(a)).any()):
                raise ValueError("%s must hold whole numbers" % name)
            if a.size and (a.min() < bounds[0] or a.max() > bounds[1]):
                raise ValueError("%s must lie in %d .. %d%s" % (name, bounds[0], bounds[1], range_note))
        return np.asfortranarray(a, dtype=dtype)                        # x fastest

    # ---- obstacle clearance (an extension; include/gvom_hip.h "obstacle clearance") ----
    def _clearance(self, set_id, pos_ptr, neg_ptr, on_device, density_threshold, include_negative, max_distance):
        thr = _clearance_threshold(density_threshold)
        cap = _clearance_cap(max_distance, self.xy_resolution)
        flags = 0 if include_negative else _CLEARANCE_NO_NEGATIVE
        return DeviceClearance(self._make_product(lambda pid: self._lib.gvom_clearance(
            self._h, int(set_id), pos_ptr, neg_ptr, int(on_device), thr, cap, flags, pid), PRODUCT_CLEARANCE))

    def clearance_of(self, positive, negative=None, density_threshold=50, include_negative=True, max_distance=None):
        """DeviceMaps.clearance() of maps of the caller's: numpy [x, y] arrays of shape (xy_size, xy_size) in any memory order
        (negative may be None).  Needs no scan and no combine.  A convenience route: the maps are copied to the device."""
        pos = self._window_map("positive", positive, np.int32)
        neg = self._window_map("negative", negative, np.int32, optional=True)
        return self._clearance(-1, _ptr(pos), _ptr(neg), 0, density_threshold, include_negative, max_distance)

    def clearance_of_device(self, positive_ptr, negative_ptr=None, density_threshold=50, include_negative=True, max_distance=None):
        """The same for maps in device memory (raw device addresses of xy_size*xy_size int32, cell (x, y) at [y*xy_size + x]; the
        data must be ready when the call is made).  negative_ptr may be None."""
        if not positive_ptr:
            raise ValueError("positive_ptr must be a device address")
        return self._clearance(-1, _dev(positive_ptr), _dev(negative_ptr), 1, density_threshold, include_negative, max_distance)

    # ---- ray queries (an extension; include/gvom_hip.h "ray queries") ----
    def _raycast(self, from_ptr, K, to_ptr, n, on_device, unknown_blocks, check_target):
        org = (ctypes.c_double * 3)()
        flags = _ray_flags(unknown_blocks, check_target)
        hold = self._make_product(lambda pid: self._lib.gvom_raycast(self._h, from_ptr, int(K), to_ptr, int(n), int(on_device), flags,
                                                                     org, pid), PRODUCT_RAYCAST, self._check_args)
        return None if hold is None else DeviceRays(hold, np.array(list(org), np.float64))

    def raycast(self, origins, targets, unknown_blocks=False, check_target=False):
        """Walks the straight segments origins -> targets (world metres) through the current fused map on the GPU, with the
        mapper's own ray rule, and returns a DeviceRays: per ray whether it is RAY_CLEAR, stopped at an occupied voxel
        (RAY_OCCUPIED), at a never-observed one (RAY_UNKNOWN, only with unknown_blocks=True; otherwise such voxels are counted) or
        left the window (RAY_LEFT_WINDOW); rays with a non-finite coordinate are RAY_INVALID.  check_target=True also examines the
        voxel the target itself lies in.  targets: (n, 3); origins: (3,), (1, 3) or (n, 3).  Arrays of any float type are
        ROUNDED TO float32 (the library's input type; a float32 start and end are what makes the voxels walked exactly the ones
        a scan's ray marks).  None before the first combine.  A convenience route: the arrays are copied to the device; rays in
        a coherent order (neighbours pointing the same way) are faster."""
        o, t = _ray_segments(origins, targets)
        return self._raycast(_ptr(o), o.shape[0], _ptr(t), t.shape[0], 0, unknown_blocks, check_target)

    def raycast_device(self, from_ptr, K, to_ptr, n, unknown_blocks=False, check_target=False):
        """The same for segments in device memory: raw device addresses of K x 3 and n x 3 float32 (C-contiguous; K is 1 or n;
        the data must be ready when the call is made).  Enqueues and returns: no host wait."""
        if not from_ptr or not to_ptr:
            raise ValueError("from_ptr and to_ptr must be device addresses")
        return self._raycast(_dev(from_ptr), K, _dev(to_ptr), n, 1, unknown_blocks, check_target)

    # ---- cost-to-go fields (an extension; include/gvom_hip.h "cost-to-go fields") ----
    def _cost_to_go(self, set_id, params, cost_ptr, on_device, cells, max_cost, max_rounds, flags, origin=(0.0, 0.0)):
        info = (_I64 * 4)()
        hold = self._make_product(lambda pid: self._lib.gvom_cost_to_go(
            self._h, int(set_id), ctypes.byref(params) if params is not None else None, cost_ptr, int(on_device), _ptr(cells),
            cells.shape[0], max_cost, max_rounds, flags, pid, info), PRODUCT_COSTFIELD)
        return DeviceCostField(hold, list(info), origin)

    def cost_to_go_of(self, cost, goals, max_cost=None, max_rounds=0, origin=(0.0, 0.0)):
        """DeviceMaps.cost_to_go() of a cost map of the caller's: a numpy [x, y] array of shape (xy_size, xy_size) in any memory
        order, integers in 0 .. 65535 (0 = blocked); goals: (G, 2) window cells.  Needs no scan and no combine.  A convenience
        route: the map is copied to the device.  origin: the window corner in world metres, kept as the field's `.origin`."""
        # (np.asarray: a cost of None is held to the shape like any other value)
        c = self._window_map("cost", np.asarray(cost), np.int32, (0, 65535), range_note=" (0 = blocked)")
        cells = _ctg_goals(goals, self.xy_size, None)
        return self._cost_to_go(-1, None, _ptr(c), 0, cells, _ctg_max_cost(max_cost), _ctg_max_rounds(max_rounds), 0, origin=origin)

    def cost_to_go_of_device(self, cost_ptr, goals, max_cost=None, max_rounds=0, origin=(0.0, 0.0)):
        """The same for a cost map in device memory (the raw device address of xy_size*xy_size int32, cell (x, y) at
        [y*xy_size + x]; the data must be ready when the call is made).  Values outside 0 .. 65535 are clamped into the range."""
        if not cost_ptr:
            raise ValueError("cost_ptr must be a device address")
        cells = _ctg_goals(goals, self.xy_size, None)
        return self._cost_to_go(-1, None, _dev(cost_ptr), 1, cells, _ctg_max_cost(max_cost), _ctg_max_rounds(max_rounds), 0, origin=origin)

    # ---- rollout scoring (an extension; include/gvom_hip.h "rollout scoring") ----
    def set_footprint(self, table):
        """Sets the vehicle's footprint table for the score_rollouts calls: what rectangle_footprint() / disc_footprint() return, or
        raw (start, offsets) arrays -- start int32 (H + 1,), offsets int16 (total, 2) = (dx, dy) in cells, heading h owning
        offsets[start[h]:start[h + 1]].  Replaces a previous table; products made with it are unchanged."""
        st, of = _footprint_arrays(table)
        self._check(self._lib.gvom_footprint_set(self._h, st.shape[0] - 1, _ptr(st), _ptr(of)))
        self._footprint_headings = st.shape[0] - 1

    def _score_rollouts(self, field_id, cost_ptr, ctg_ptr, poses_ptr, K, T, on_device, origin):
        oc = _rollout_origin(origin, self.xy_resolution)
        return DeviceRollouts(self._make_product(lambda pid: self._lib.gvom_score_rollouts(
            self._h, int(field_id), cost_ptr, ctg_ptr, poses_ptr, int(K), int(T), int(on_device), oc, pid), PRODUCT_ROLLOUTS,
            self._check_args))

    def score_rollouts_of(self, cell_cost, poses, cost_to_go=None, origin=(0.0, 0.0)):
        """DeviceCostField.score_rollouts() against maps of the caller's: cell_cost a numpy [x, y] array of shape (xy_size, xy_size)
        in any memory order, whole numbers in 0 .. 65535 (0 = blocked); cost_to_go (optional) int32 of the same shape, the field
        the terminal column is read from; origin: the window corner in world metres.  Needs no scan and no combine.  A convenience
        route: maps and poses are copied to the device."""
        cc = self._window_map("cell_cost", cell_cost, np.uint16, (0, 65535))
        ctg = self._window_map("cost_to_go", cost_to_go, np.int32, (-2 ** 31, 2 ** 31 - 1), optional=True)
        p = _rollout_poses(poses)
        return self._score_rollouts(-1, _ptr(cc), _ptr(ctg), _ptr(p), p.shape[0], p.shape[1], 0, origin)

    def score_rollouts_of_device(self, cell_cost_ptr, poses_ptr, K, T, cost_to_go_ptr=None, origin=(0.0, 0.0)):
        """The same for maps and poses in device memory: raw device addresses of xy_size*xy_size uint16 (cell (x, y) at
        [y*xy_size + x]), K x T x 3 float32 (C-contiguous) and, optionally, xy_size*xy_size int32; the data must be ready when the
        call is made.  Enqueues and returns: no host wait."""
        if not cell_cost_ptr or not poses_ptr:
            raise ValueError("cell_cost_ptr and poses_ptr must be device addresses")
        K, T = _rollout_shape(K, T)
        return self._score_rollouts(-1, _dev(cell_cost_ptr), _dev(cost_to_go_ptr), _dev(poses_ptr), K, T, 1, origin)

    # ---- terrain attitude scoring (an extension; include/gvom_hip.h "terrain attitude scoring") ----
    def set_chassis(self, chassis):
        """Sets the vehicle's chassis (what chassis() returns) for the score_attitude calls, after set_footprint: the headings are
        the footprint table's, and `.cos_sin` -- float64 [H, 2], the (cos, sin) of each heading the library turns the wheels and the
        belly with -- is kept readable.  Replaces a previous chassis; products made with it are unchanged.  Set the chassis again
        after a set_footprint with another number of headings."""
        if not isinstance(chassis, GvomChassis):
            raise ValueError("set_chassis takes what chassis() returns, got %r" % (type(chassis).__name__,))
        H = getattr(self, "_footprint_headings", None)
        if H is None:
            raise ValueError("set_footprint comes first: the chassis takes its headings from the footprint table")
        cs = heading_cos_sin(H)
        self._check_args(self._lib.gvom_chassis_set(self._h, ctypes.byref(chassis), H, _ptr(cs)))
        self.cos_sin = cs

    def _score_attitude(self, set_id, ground_ptr, poses_ptr, K, T, on_device, inferred_ground, origin):
        oc = _rollout_origin(origin, self.xy_resolution)
        flags = _ATTITUDE_INFERRED_GROUND if inferred_ground else 0
        return DeviceAttitude(self._make_product(lambda pid: self._lib.gvom_score_attitude(
            self._h, int(set_id), ground_ptr, poses_ptr, int(K), int(T), int(on_device), flags, oc, pid), PRODUCT_ATTITUDE,
            self._check_args))

    def score_attitude_of(self, ground, poses, origin=(0.0, 0.0)):
        """DeviceMaps.score_attitude() against a ground map of the caller's: a numpy [x, y] array of shape (xy_size, xy_size) in any
        memory order, heights in metres cast to float64 as they are (NaN, infinities and values <= -1000 are unknown ground);
        origin: the window corner in world metres.  Needs no scan and no combine.  A convenience route: map and poses are copied
        to the device."""
        gm = self._window_map("ground", ground, np.float64)
        p = _rollout_poses(poses)
        return self._score_attitude(-1, _ptr(gm), _ptr(p), p.shape[0], p.shape[1], 0, False, origin)

    def score_attitude_of_device(self, ground_ptr, poses_ptr, K, T, origin=(0.0, 0.0)):
        """The same for a map and poses in device memory: raw device addresses of xy_size*xy_size float64 (cell (x, y) at
        [y*xy_size + x]) and K x T x 3 float32 (C-contiguous); the data must be ready when the call is made.  Enqueues and returns:
        no host wait."""
        if not ground_ptr or not poses_ptr:
            raise ValueError("ground_ptr and poses_ptr must be device addresses")
        K, T = _rollout_shape(K, T)
        return self._score_attitude(-1, _dev(ground_ptr), _dev(poses_ptr), K, T, 1, False, origin)

    # ---- body clearance scoring (an extension; include/gvom_hip.h "body clearance scoring") ----
    def set_body(self, spheres):
        """Sets the vehicle's body for the score_body calls: float32 (S, 4) = (bx, by, bz, r), 1 <= S <= 256 -- sphere centres in the
        chassis's body frame (x forward, y left, bz above the wheels' contact plane) and radii >= 0, in metres; box_spheres() makes
        one of a box.  Replaces a previous body; products made with it are unchanged."""
        a = _body_spheres(spheres)
        self._check_args(self._lib.gvom_body_set(self._h, _ptr(a), a.shape[0]))

    def _host_field(self, field):
        f = np.ascontiguousarray(np.asarray(field), dtype=np.float32)
        if f.shape != (self.xy_size, self.xy_size, self.z_size):
            raise ValueError("field must have shape (%d, %d, %d), got %r" % (self.xy_size, self.xy_size, self.z_size, f.shape))
        return f

    def _score_body(self, field_id, field_ptr, field_origin, set_id, ground_ptr, poses_ptr, K, T, on_device, inferred_ground, origin, min_margin):
        oc = _rollout_origin(origin, self.xy_resolution)
        flags = _ATTITUDE_INFERRED_GROUND if inferred_ground else 0
        mm, _ = _body_margins(min_margin, None)
        return DeviceBodyClearance(self._make_product(lambda pid: self._lib.gvom_score_body(
            self._h, int(field_id), field_ptr, field_origin, int(set_id), ground_ptr, poses_ptr, int(K), int(T), int(on_device), flags, oc,
            ctypes.c_float(mm), pid), PRODUCT_BODY, self._check_args))

    def score_body_of(self, field, field_origin_voxels, ground, poses, origin=(0.0, 0.0), min_margin=0.0):
        """DeviceDistanceField.score_body() with a field AND a ground map of the caller's: field a numpy float32 array of shape
        (xy_size, xy_size, z_size) in the class grid's layout, its corner at field_origin_voxels (three integers, world voxels);
        ground as score_attitude_of takes it; origin: the window corner in world metres.  Needs no scan and no combine.  A
        convenience route: field, map and poses are copied to the device."""
        f = self._host_field(field)
        gm = self._window_map("ground", ground, np.float64)
        p = _rollout_poses(poses)
        return self._score_body(-1, _ptr(f), _voxel_origin(field_origin_voxels, "field_origin_voxels"), -1, _ptr(gm), _ptr(p), p.shape[0],
                                p.shape[1], 0, False, origin, min_margin)

    def score_body_of_device(self, field_ptr, field_origin_voxels, ground_ptr, poses_ptr, K, T, origin=(0.0, 0.0), min_margin=0.0):
        """The same for a field, a map and poses in device memory: raw device addresses of xy_size*xy_size*z_size float32 ([x][y][z]),
        xy_size*xy_size float64 (cell (x, y) at [y*xy_size + x]) and K x T x 3 float32 (C-contiguous); the data must be ready when the
        call is made.  Enqueues and returns: no host wait."""
        if not field_ptr or not ground_ptr or not poses_ptr:
            raise ValueError("field_ptr, ground_ptr and poses_ptr must be device addresses")
        K, T = _rollout_shape(K, T)
        return self._score_body(-1, _dev(field_ptr), _voxel_origin(field_origin_voxels, "field_origin_voxels"), -1, _dev(ground_ptr),
                                _dev(poses_ptr), K, T, 1, False, origin, min_margin)

    # ---- body volumes (an extension; include/gvom_hip.h "body volumes") ----
    def _body_volume(self, field_id, field_ptr, field_origin, set_id, ground_ptr, on_device, inferred_ground, origin, min_margin, soft_margin):
        oc = _rollout_origin(origin, self.xy_resolution)
        flags = _ATTITUDE_INFERRED_GROUND if inferred_ground else 0
        mm, sm = _body_margins(min_margin, soft_margin)
        return DeviceBodyVolume(self._make_product(lambda pid: self._lib.gvom_body_volume(
            self._h, int(field_id), field_ptr, field_origin, int(set_id), ground_ptr, int(on_device), flags, oc, ctypes.c_float(mm),
            ctypes.c_float(sm), pid), PRODUCT_BODY_VOLUME, self._check_args))

    def body_volume_of(self, field, field_origin_voxels, ground, origin=(0.0, 0.0), min_margin=0.0, soft_margin=None):
        """DeviceDistanceField.body_volume() with a field AND a ground map of the caller's: field and field_origin_voxels as
        score_body_of takes them, ground as score_attitude_of takes it; origin: the window corner in world metres.  Needs no scan and
        no combine.  A convenience route: field and map are copied to the device."""
        f = self._host_field(field)
        gm = self._window_map("ground", ground, np.float64)
        return self._body_volume(-1, _ptr(f), _voxel_origin(field_origin_voxels, "field_origin_voxels"), -1, _ptr(gm), 0, False, origin,
                                 min_margin, soft_margin)

    def body_volume_of_device(self, field_ptr, field_origin_voxels, ground_ptr, origin=(0.0, 0.0), min_margin=0.0, soft_margin=None):
        """The same for a field and a map in device memory: raw device addresses of xy_size*xy_size*z_size float32 ([x][y][z]) and
        xy_size*xy_size float64 (cell (x, y) at [y*xy_size + x]); the data must be ready when the call is made.  Enqueues and returns:
        no host wait."""
        if not field_ptr or not ground_ptr:
            raise ValueError("field_ptr and ground_ptr must be device addresses")
        return self._body_volume(-1, _dev(field_ptr), _voxel_origin(field_origin_voxels, "field_origin_voxels"), -1, _dev(ground_ptr), 1,
                                 False, origin, min_margin, soft_margin)

    # ---- attitude volumes (an extension; include/gvom_hip.h "attitude volumes") ----
    def _attitude_volume(self, set_id, ground_ptr, on_device, inferred_ground):
        flags = _ATTITUDE_INFERRED_GROUND if inferred_ground else 0
        return DeviceAttitudeVolume(self._make_product(lambda pid: self._lib.gvom_attitude_volume(
            self._h, int(set_id), ground_ptr, int(on_device), flags, pid), PRODUCT_ATTITUDE_VOLUME, self._check_args))

    def attitude_volume_of(self, ground):
        """DeviceMaps.attitude_volume() of a ground map of the caller's: a numpy [x, y] array of shape (xy_size, xy_size) in any
        memory order, heights in metres cast to float64 as they are (NaN, infinities and values <= -1000 are unknown ground).  Needs
        no scan and no combine.  A convenience route: the map is copied to the device."""
        gm = self._window_map("ground", ground, np.float64)
        return self._attitude_volume(-1, _ptr(gm), 0, False)

    def attitude_volume_of_device(self, ground_ptr):
        """The same for a map in device memory: the raw device address of xy_size*xy_size float64 (cell (x, y) at [y*xy_size + x]);
        the data must be ready when the call is made.  Enqueues and returns: no host wait."""
        if not ground_ptr:
            raise ValueError("ground_ptr must be a device address")
        return self._attitude_volume(-1, _dev(ground_ptr), 1, False)

    # ---- frontier extraction (an extension; include/gvom_hip.h "frontier extraction") ----
    def _frontiers(self, field_id, set_id, cost_ptr, ctg_ptr, vis_ptr, on_device, min_cells, max_clusters, origin):
        min_cells, max_clusters = _frontier_limits(min_cells, max_clusters)
        info = (_I64 * 4)()
        hold = self._make_product(lambda pid: self._lib.gvom_frontiers(
            self._h, int(field_id), int(set_id), cost_ptr, ctg_ptr, vis_ptr, int(on_device), min_cells, max_clusters, pid, info),
            PRODUCT_FRONTIERS, self._check_args)
        return DeviceFrontiers(hold, list(info), self.xy_resolution, origin)

    def frontiers_of(self, cell_cost, visibility, cost_to_go=None, min_cells=4, max_clusters=1024, origin=(0.0, 0.0)):
        """DeviceCostField.frontiers() of maps of the caller's: cell_cost a numpy [x, y] array of shape (xy_size, xy_size) in any
        memory order, whole numbers in 0 .. 65535 (0 = blocked); visibility int32 of the same shape (> 0: seen); cost_to_go
        (optional) int32 of the same shape -- without it every seen, unblocked cell counts as reachable.  Needs no scan and no
        combine.  A convenience route: the maps are copied to the device.  origin: the window corner in world metres."""
        cc = self._window_map("cell_cost", cell_cost, np.uint16, (0, 65535))
        vis = self._window_map("visibility", visibility, np.int32, (-2 ** 31, 2 ** 31 - 1))
        ctg = self._window_map("cost_to_go", cost_to_go, np.int32, (-2 ** 31, 2 ** 31 - 1), optional=True)
        return self._frontiers(-1, -1, _ptr(cc), _ptr(ctg), _ptr(vis), 0, min_cells, max_clusters, origin)

    def frontiers_of_device(self, cell_cost_ptr, visibility_ptr, cost_to_go_ptr=None, min_cells=4, max_clusters=1024, origin=(0.0, 0.0)):
        """The same for maps in device memory: raw device addresses of xy_size*xy_size uint16, int32 and, optionally, int32 (cell
        (x, y) at [y*xy_size + x]); the data must be ready when the call is made."""
        if not cell_cost_ptr or not visibility_ptr:
            raise ValueError("cell_cost_ptr and visibility_ptr must be device addresses")
        return self._frontiers(-1, -1, _dev(cell_cost_ptr), _dev(cost_to_go_ptr), _dev(visibility_ptr), 1, min_cells, max_clusters, origin)

    # ---- viewpoint scoring (an extension; include/gvom_hip.h "viewpoint scoring") ----
    def _score_viewpoints(self, poses_ptr, K, on_device, max_range, beam_stride, unknown_blocks, host_poses=None):
        K, r, sh, sw = _viewpoint_options(K, max_range, beam_stride)
        org = (ctypes.c_double * 3)()
        flags = _ray_flags(unknown_blocks)
        hold = self._make_product(lambda pid: self._lib.gvom_score_viewpoints(self._h, poses_ptr, K, int(on_device), r, sh, sw, flags,
                                                                              org, pid), PRODUCT_VIEWPOINTS, self._check_args)
        return None if hold is None else DeviceViewpoints(hold, np.array(list(org), np.float64), host_poses)

    def score_viewpoints(self, poses, max_range, beam_stride=(1, 1), unknown_blocks=False):
        """Next-best-view scoring on the GPU: puts the sensor whose model set_sensor_model() holds at each of K poses and casts its
        beams, max_range metres long, through the current fused map with raycast()'s ray rule -- a DeviceViewpoints: per pose how
        many DISTINCT never-observed voxels the beams pass before they stop (gain), the same counted once per beam (visits), how the
        beams ended, whether the pose itself lies in an observed-free voxel, and the best such pose.  poses: float64 (K, 4, 4) or
        (K, 3, 4), sensor to world (viewpoint_poses() builds them from points and yaws), or one matrix; beam_stride = (rows,
        columns): every how-manyth beam of the model is cast; unknown_blocks=True: a beam stops at the first never-observed voxel.
        Every beam starts at the pose's translation.  Read-only: the map does not change.  None before the first combine.  A
        convenience route: the poses are copied to the device."""
        t = _viewpoint_poses(poses)
        return self._score_viewpoints(_ptr(t), t.shape[0], 0, max_range, beam_stride, unknown_blocks, t)

    def score_viewpoints_device(self, poses_ptr, K, max_range, beam_stride=(1, 1), unknown_blocks=False):
        """The same for poses in device memory: the raw device address of K x 3 x 4 float64 (rows 0..2 of each matrix,
        C-contiguous; the data must be ready when the call is made).  Enqueues and returns: no host wait."""
        if not poses_ptr:
            raise ValueError("poses_ptr must be a device address")
        return self._score_viewpoints(_dev(poses_ptr), K, 1, max_range, beam_stride, unknown_blocks)

    # ---- pose fields (an extension; include/gvom_hip.h "pose fields") ----
    def set_primitives(self, table):
        """Sets the vehicle's motion primitives for the pose_field calls: what arc_primitives() returns, or raw (start, prims) arrays
        -- start int32 (H + 1,), prims int16 (total, 4) = (dx, dy, h_to, w), heading h owning prims[start[h]:start[h + 1]]: from the
        state (x, y, h) to (x + dx, y + dy, h_to) at the price w * (pose cost at both ends).  H must be the footprint table's when a
        field is made.  Replaces a previous table; products made with it are unchanged."""
        st, pr = _primitive_arrays(table)
        self._check_args(self._lib.gvom_primitives_set(self._h, st.shape[0] - 1, _ptr(st), _ptr(pr)))
        self._primitives = (st, pr)

    def _pose_headings(self):
        if getattr(self, "_primitives", None) is None:
            raise ValueError("no primitive table is set (Gvom.set_primitives)")
        return self._primitives[0].shape[0] - 1

    def _pose_field(self, field_id, cost_ptr, on_device, cells, max_cost, max_rounds, origin, attitude=None, body=None):
        info = (_I64 * 4)()
        table = self._primitives
        if body is not None:
            a = attitude if attitude is not None else (-1, 0, 0)
            call = lambda pid: self._lib.gvom_pose_field_volumes(
                self._h, int(field_id), cost_ptr, int(on_device), a[0], a[1], a[2], body[0], body[1], body[2], _ptr(cells), cells.shape[0],
                max_cost, max_rounds, pid, info)
        elif attitude is None:
            call = lambda pid: self._lib.gvom_pose_field(
                self._h, int(field_id), cost_ptr, int(on_device), _ptr(cells), cells.shape[0], max_cost, max_rounds, pid, info)
        else:
            call = lambda pid: self._lib.gvom_pose_field_attitude(
                self._h, int(field_id), cost_ptr, int(on_device), attitude[0], attitude[1], attitude[2], _ptr(cells), cells.shape[0],
                max_cost, max_rounds, pid, info)
        hold = self._make_product(call, PRODUCT_POSEFIELD, self._check_args)
        return DevicePoseField(hold, list(info), origin, table)

    def pose_field_of(self, cost, goals, max_cost=None, max_rounds=0, origin=(0.0, 0.0), attitude=None, attitude_blocks=_ATTITUDE_BLOCKS, tilt_weight=0,
                      body=None, body_blocks=_BODY_BLOCKS, squeeze_weight=0):
        """DeviceCostField.pose_field() of a cost map of the caller's: a numpy [x, y] array of shape (xy_size, xy_size) in any memory
        order, integers in 0 .. 65535 (0 = blocked); goals: (G, 2) or (G, 3) = (x, y[, yaw]) in window cells and radians.  Needs no
        scan and no combine.  A convenience route: the map is copied to the device.  origin: kept as the field's `.origin`.
        attitude, attitude_blocks, tilt_weight, body, body_blocks, squeeze_weight: as DeviceCostField.pose_field()."""
        H = self._pose_headings()
        c = self._window_map("cost", np.asarray(cost), np.int32, (0, 65535), range_note=" (0 = blocked)")
        cells = _pose_goals(goals, self.xy_size, H, None)
        return self._pose_field(-1, _ptr(c), 0, cells, _ctg_max_cost(max_cost), _ctg_max_rounds(max_rounds), origin,
                                _pose_attitude(attitude, attitude_blocks, tilt_weight), _pose_body(body, body_blocks, squeeze_weight))

    def pose_field_of_device(self, cost_ptr, goals, max_cost=None, max_rounds=0, origin=(0.0, 0.0), attitude=None, attitude_blocks=_ATTITUDE_BLOCKS,
                             tilt_weight=0, body=None, body_blocks=_BODY_BLOCKS, squeeze_weight=0):
        """The same for a cost map in device memory (the raw device address of xy_size*xy_size int32, cell (x, y) at
        [y*xy_size + x]; the data must be ready when the call is made).  Values outside 0 .. 65535 are clamped into the range."""
        if not cost_ptr:
            raise ValueError("cost_ptr must be a device address")
        H = self._pose_headings()
        cells = _pose_goals(goals, self.xy_size, H, None)
        return self._pose_field(-1, _dev(cost_ptr), 1, cells, _ctg_max_cost(max_cost), _ctg_max_rounds(max_rounds), origin,
                                _pose_attitude(attitude, attitude_blocks, tilt_weight), _pose_body(body, body_blocks, squeeze_weight))

    # ---- map atlas (an extension; include/gvom_hip.h "map atlas") ----
    def create_atlas(self, cells, follow=True, origin_cells=None):
        """Configures the mapper's atlas -- one per mapper; a second call replaces the first -- and returns it: `cells` x `cells`
        world cells (a power of two in 64 .. 4096, at least xy_size; 64 bytes of device memory each).  follow=True: the extent
        re-centres on every integrated set and forgets what leaves it; follow=False: it stays at origin_cells (its corner, integer
        world cells) and sets outside it are skipped.  See Atlas."""
        return Atlas(self, cells, follow, origin_cells)

    # ---- voxel atlas (an extension; include/gvom_hip.h "voxel atlas") ----
    def create_voxel_atlas(self, cells, levels, follow=True, origin_voxels=None):
        """Configures the mapper's voxel atlas -- one per mapper; a second call replaces the first -- and returns it: `cells` x `cells`
        x `levels` world voxels at 2 bits each (cells a power of two in 64 .. 4096, at least xy_size; levels a power of two from z_size
        to cells; at most 2**32 voxels, 1 GiB).  follow=True: the extent re-centres on every integrated window, as the map atlas's does,
        and forgets what leaves it; follow=False: it stays at origin_voxels (its corner, integer world voxels).  See VoxelAtlas."""
        return VoxelAtlas(self, cells, levels, follow, origin_voxels)

    # ---- scan alignment scoring (an extension; include/gvom_hip.h "scan alignment scoring") ----
    def _score_alignments(self, cloud_ptr, n, tf_ptr, K, on_device, dilate, weights):
        dilate, w = _align_options(dilate, weights)
        n, K = _align_shape(n, K)
        hold = self._make_product(lambda pid: self._lib.gvom_score_alignments(self._h, cloud_ptr, n, tf_ptr, K, int(on_device), dilate,
                                                                              w, pid), PRODUCT_ALIGNMENT, self._check_args)
        return None if hold is None else DeviceAlignments(hold, np.array(list(self._state().combined_origin), np.float64))

    def score_alignments(self, cloud, transforms, dilate=0, weights=ALIGN_DEFAULT_WEIGHTS):
        """Holds a scan under K candidate poses against the current fused map on the GPU -- the inner loop of a correlative scan
        matcher -- and returns a DeviceAlignments: per candidate how many of the n returns end in an occupied voxel, next to one
        (dilate=1: within one voxel on every axis), in a free one, in a never-observed one and outside the window, the score
        sum(weights * counts) (weights: five integers in -1024 .. 1024 for {occupied, near, free, unknown, outside}), and the best
        candidate.  A return under a candidate is classed by the voxel process_pointcloud(cloud, ego, transform=candidate) would
        add its hit to (without the min_distance rejection).  cloud: float32 (n, 3) -- other dtypes raise TypeError, nothing is
        cast; transforms: float64 (K, 4, 4) or (K, 3, 4) (pose_candidates builds a grid of them; arbitrary matrices are accepted).
        Read-only: the map does not change.  None before the first combine.  A convenience route: the arrays are copied to the
        device."""
        c = _align_cloud(cloud)
        t = _align_transforms(transforms)
        return self._score_alignments(_ptr(c), c.shape[0], _ptr(t), t.shape[0], 0, dilate, weights)

    def score_alignments_device(self, cloud_ptr, n, transforms_ptr, K, dilate=0, weights=ALIGN_DEFAULT_WEIGHTS):
        """The same for inputs in device memory: raw device addresses of n x 3 float32 and K x 3 x 4 float64 (rows 0..2 of each
        candidate, C-contiguous; the data must be ready when the call is made).  Enqueues and returns: no host wait."""
        if not cloud_ptr or not transforms_ptr:
            raise ValueError("cloud_ptr and transforms_ptr must be device addresses")
        return self._score_alignments(_dev(cloud_ptr), n, _dev(transforms_ptr), K, 1, dilate, weights)

    def make_debug_voxel_map(self):
        """float32[Cc, 8] rows {x, y, z, hit/total, hit, l0-l1, l1-l2, l2} (reference gvom.py:363-378) while the mapper
        computes the per-voxel statistics (voxel_statistics: by default for as long as this is called); else None, which
        the reference's caller tolerates (gvom_ros.py:171-172) -- and which switches them on again for the scans that follow."""
        n = self.combined_cell_count_cpu
        if n is None:
            print("No data")
            return None
        out = np.empty((max(n, 1), 8), np.float32)
        rows = ctypes.c_int64(0)
        rc = self._check(self._lib.gvom_debug_voxel_map(self._h, _ptr(out), n, ctypes.byref(rows)))
        if rc == GVOM_NO_DATA:
            return None
        return out[:min(n, int(rows.value))]

    def _rows(self, which):
        rows = np.empty(self.voxel_count, np.int32)
        rc = self._check(self._lib.gvom_read_rows(self._h, int(which), _ptr(rows)))
        return None if rc == GVOM_NO_DATA else rows[rows >= 0]          # occupied voxels, in voxel order

    def _metrics(self, which, dtype):
        """(C, 10) statistics {mean xyz, covariance xx xy xz yy yz zz, count} of the occupied voxels of a
        ring slot (float64) or of the fused map (float32), rows in voxel order (row order is unspecified
        in the reference, gvom.py:1158); None without voxel statistics."""
        rows = self._rows(which)
        if rows is None:
            return None
        out = np.empty((rows.shape[0], 10), dtype)
        rc = self._check(self._lib.gvom_gather_metrics(self._h, int(which), _ptr(np.ascontiguousarray(rows)),
                                                       rows.shape[0], _ptr(out)))
        return None if rc == GVOM_NO_DATA else out

    @property
    def metrics_buffer(self):
        """reference attribute (gvom.py:62,166): per ring slot None or a device-array stand-in of (C, 10) float64"""
        out = []
        for i in range(self.buffer_size):
            if self._lib.gvom_slot_filled(self._h, i) != 1 or self._metrics(i, np.float64) is None:
                out.append(None)
            else:
                out.append(_DeviceArrayView(lambda i=i: self._metrics(i, np.float64)))
        return out

    @property
    def combined_metrics(self):
        """reference attribute (gvom.py:72,234): (Cc, 10) float32 of the fused map, rows in voxel order"""
        if not self._state().has_combined or self._metrics(GVOM_WHICH_FUSED, np.float32) is None:
            return None
        return _DeviceArrayView(lambda: self._metrics(GVOM_WHICH_FUSED, np.float32))

    last_combined_metrics = combined_metrics

    @property
    def voxels_eigenvalues(self):
        """reference attribute (gvom.py:83,281, set by make_debug_voxel_map): (Cc, 3) float32 eigenvalues
        l0 >= l1 >= l2 of the fused voxels' covariances, rows in voxel order"""
        n = self.combined_cell_count_cpu
        if n is None:
            return None
        out = np.empty((max(n, 1), 8), np.float32)
        eig = np.empty((max(n, 1), 3), np.float32)
        rows = ctypes.c_int64(0)
        rc = self._check(self._lib.gvom_debug_voxel_eigen(self._h, _ptr(out), _ptr(eig), n, ctypes.byref(rows)))
        if rc == GVOM_NO_DATA:
            return None
        k = min(n, int(rows.value))
        st = self._state()
        # voxel order: the rows carry their world coordinates (gvom.py:462-466)
        x = np.rint(out[:k, 0] / self.xy_resolution - st.combined_origin[0]).astype(np.int64)
        y = np.rint(out[:k, 1] / self.xy_resolution - st.combined_origin[1]).astype(np.int64)
        z = np.rint(out[:k, 2] / self.z_resolution - st.combined_origin[2]).astype(np.int64)
        order = np.argsort(x + y * self.xy_size + z * self.xy_size * self.xy_size, kind="stable")
        arr = np.ascontiguousarray(eig[:k][order])
        return _DeviceArrayView(lambda: arr.copy())

    def make_debug_height_map(self):
        out = np.empty((self.xy_size * self.xy_size, 7), np.float32)
        rc = self._check(self._lib.gvom_debug_height_map(self._h, _ptr(out)))
        if rc == GVOM_NO_DATA:
            print("No data")
            return None
        return out

    def make_debug_inferred_height_map(self):
        out = np.empty((self.xy_size * self.xy_size, 3), np.float32)
        rc = self._check(self._lib.gvom_debug_inferred_height_map(self._h, _ptr(out)))
        if rc == GVOM_NO_DATA:
            print("No data")
            return None
        return out

    # ---- ring-buffer / fused-map attributes of the reference object ------------------
    def _state(self):
        st = GvomState()
        self._check(self._lib.gvom_get_state(self._h, ctypes.byref(st)))
        return st

    @property
    def buffer_index(self):
        return int(self._state().buffer_index)

    @property
    def last_buffer_index(self):
        return int(self._state().last_buffer_index)

    @property
    def combined_cell_count_cpu(self):
        st = self._state()
        return int(st.combined_cell_count) if st.has_combined else None

    last_combined_cell_count_cpu = combined_cell_count_cpu

    def read_dense(self, which):
        """Test hook: (state, hit, total, min_h, origin, cell_count) dense arrays in the
        reference's voxel order for ring slot `which` or GVOM_WHICH_FUSED; None if empty."""
        V = self.voxel_count
        state = np.empty(V, np.int32); hit = np.empty(V, np.int32); total = np.empty(V, np.int32)
        minh = np.empty(V, np.float32); origin = np.zeros(3); cnt = ctypes.c_int64(0)
        rc = self._check(self._lib.gvom_read_dense(self._h, int(which), _ptr(state), _ptr(hit),
                                                   _ptr(total), _ptr(minh), _ptr(origin),
                                                   ctypes.byref(cnt)))
        if rc == GVOM_NO_DATA:
            return None
        return state, hit, total, minh, origin, int(cnt.value)

    def _compact(self, which):
        """Reference-shaped sparse form (index_map, hit[C], total[C], min_height) rebuilt from
        the dense test hook; rows numbered in voxel order (row order is unspecified in the
        reference, gvom.py:1158)."""
        d = self.read_dense(which)
        if d is None:
            return None
        state, hit, total, minh, origin, _ = d
        occ = state >= 0
        index_map = state.copy()
        index_map[occ] = np.arange(int(occ.sum()), dtype=np.int32)
        return index_map, hit[occ], total[occ], minh[occ], origin

    def _slot_views(self, field):
        out = []
        for i in range(self.buffer_size):
            if self._lib.gvom_slot_filled(self._h, i) != 1:
                out.append(None)
                continue

            def fetch(i=i, field=field):
                index_map, hit, total, minh, origin = self._compact(i)
                if field == 4:                       # gvom.py:1014: min_height has 3*C entries
                    return np.concatenate([minh, np.ones(2 * minh.shape[0], np.float32)])
                return (index_map, hit, total, minh, origin)[field]
            out.append(_DeviceArrayView(fetch))
        return out

    index_buffer = property(lambda self: self._slot_views(0))
    hit_count_buffer = property(lambda self: self._slot_views(1))
    total_count_buffer = property(lambda self: self._slot_views(2))
    min_height_buffer = property(lambda self: self._slot_views(4))

    @property
    def origin_buffer(self):
        out = []
        for i in range(self.buffer_size):
            if self._lib.gvom_slot_filled(self._h, i) != 1:
                out.append(None)
            else:
                out.append(_DeviceArrayView(lambda i=i: self.read_dense(i)[4]))
        return out

    def _fused_view(self, field):
        if not self._state().has_combined:
            return None
        return _DeviceArrayView(lambda: self._compact(GVOM_WHICH_FUSED)[field])

    combined_index_map = property(lambda self: self._fused_view(0))
    combined_hit_count = property(lambda self: self._fused_view(1))
    combined_total_count = property(lambda self: self._fused_view(2))
    combined_min_height = property(lambda self: self._fused_view(3))
    last_combined_index_map = combined_index_map
    last_combined_hit_count = combined_hit_count
    last_combined_total_count = combined_total_count
    last_combined_min_height = combined_min_height

    @property
    def combined_origin(self):
        st = self._state()
        if not st.has_combined:
            return None
        org = np.array(list(st.combined_origin), np.float64)
        return _DeviceArrayView(lambda: org.copy())

    last_combined_origin = combined_origin

    def _map2d(self, which):
        out = np.empty((self.xy_size, self.xy_size), np.float64)
        rc = self._check(self._lib.gvom_read_map2d(self._h, which, _ptr(out)))
        return None if rc == GVOM_NO_DATA else out

    def _map_view(self, which):
        if self._map2d(which) is None:
            return None
        return _DeviceArrayView(lambda: self._map2d(which))

    height_map = property(lambda self: self._map_view(MAP_HEIGHT))
    inferred_height_map = property(lambda self: self._map_view(MAP_INFERRED))
    x_slope_map = property(lambda self: self._map_view(MAP_SLOPE_X))
    y_slope_map = property(lambda self: self._map_view(MAP_SLOPE_Y))
    roughness_map = property(lambda self: self._map_view(MAP_ROUGHNESS))
    guessed_height_delta = property(lambda self: self._map_view(MAP_GUESSED))

    # ---- measurement helpers ----------------------------------------------------------
    def set_profiling(self, on):
        self._check(self._lib.gvom_set_profiling(self._h, 1 if on else 0))

    def last_stage_ms(self):
        ms = (ctypes.c_float * N_STAGES)()
        self._check(self._lib.gvom_last_stage_ms(self._h, ctypes.byref(ms)))
        return dict(zip(STAGE_NAMES, [float(v) for v in ms]))

    def forget(self, *arrays):
        """The caller has WRITTEN into maps combine_maps() returned.  The returned arrays are writable views of a pinned buffer
        that comes back to a later combine_maps() once they are all dropped, and the library stores only the runs of cells that
        changed since it last wrote that buffer (include/gvom_hip.h, gvom_output_forget) -- it must be the buffer's only writer.
        Call forget(array, ...) with any of the written arrays BEFORE dropping them (no argument: every buffer of this mapper),
        or switch the mechanism off: set_tuning("delta_out", 0).  A caller that only reads the maps, or copies them, has
        nothing to do."""
        if not arrays:
            self._check(self._lib.gvom_set_tuning(self._h, b"delta_out", -1))     # (-1: every record goes, the setting stays)
            return
        for a in arrays:
            base = a
            while getattr(base, "base", None) is not None:
                base = base.base
            ptr = getattr(base, "ptr", None)
            if ptr is None:
                ptr = np.asarray(a).__array_interface__["data"][0]
            self._check(self._lib.gvom_output_forget(self._h, _dev(ptr)))

    def output_record(self, array):
        """(bits uint8[n], generation) of the content record of the buffer behind a returned map (include/gvom_hip.h,
        gvom_output_record), or None when it has none.  For measurements and tests."""
        base = array
        while getattr(base, "base", None) is not None:
            base = base.base
        ptr = _dev(base.ptr)
        n, gen = ctypes.c_size_t(0), ctypes.c_uint64(0)
        if self._check(self._lib.gvom_output_record(self._h, ptr, None, 0, ctypes.byref(n), ctypes.byref(gen))) == GVOM_NO_DATA:
            return None
        bits = np.zeros(n.value, np.uint8)
        if self._check(self._lib.gvom_output_record(self._h, ptr, _ptr(bits), n.value, ctypes.byref(n), ctypes.byref(gen))) == GVOM_NO_DATA:
            return None
        return bits, int(gen.value)

    def set_tuning(self, name, value):
        """Performance knobs that never change a result: "segs", "period", "ep_row", "prio", "interleave", "eager", "delta_out"
        (include/gvom_hip.h).  "delta_out" 0: combine_maps() stores every cell every time -- for callers that write into the
        returned maps in place and do not call forget()."""
        self._check(self._lib.gvom_set_tuning(self._h, name.encode(), int(value)))

    def get_tuning(self, name):
        """The value the last scan ran with (what "automatic" resolved to)."""
        v = _I(0)
        self._check(self._lib.gvom_get_tuning(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def host_timing(self):
        us = (ctypes.c_double * 8)()
        self._check(self._lib.gvom_host_timing(self._h, ctypes.byref(us)))
        return dict(zip(("scan_launch", "scan_wait", "combine_launch", "combine_wait", "output_copy"),
                        [float(v) for v in us][:5]))

    def scan_stats(self):
        st = GvomScanStats()
        rc = self._check(self._lib.gvom_get_scan_stats(self._h, ctypes.byref(st)))
        if rc == GVOM_NO_DATA:
            return None
        return {"points": int(st.points), "cells": int(st.cells), "sum_hit": int(st.sum_hit),
                "sum_total": int(st.sum_total)}

    @staticmethod
    def backend_info():
        L = load_library()
        buf = ctypes.create_string_buffer(256)
        rc = L.gvom_backend_info(buf, 256)
        return rc, buf.value.decode()
