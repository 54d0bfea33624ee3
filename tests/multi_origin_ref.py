"""Shared by tests/test_multi_origin.py, tests/test_multi_origin_cpu.py and tests/_multi_origin_torch.py: the referee of a
multi-origin scan, built from the UNMODIFIED oracle, and the inputs of those tests.

The referee: oracle.OracleGvom.process_pointcloud with its one orc_point_2_map call replaced by one call per origin k, on the
sub-cloud index == k with ego = O[k], all of them onto the same hit / total arrays and with the window origin computed from
`ego` -- orc_point_2_map takes the ray origin and the window as separate arguments and ADDS into the arrays it is given.
Everything behind (row assignment, min-height, statistics, ring) is the parent's, on the whole cloud."""
import math

import numpy as np

import synth
from oracle import oracle

K = 5
N = 8192
GRIDS = {                                                  # (xy_resolution, z_resolution, xy_size, z_size): the smallest of each kind
    "p2": (0.4, 0.2, 64, 32),                              # power of two: integer lookup, the no-window-test step body runs
    "np2": (0.4, 0.2, 48, 20),                             # no power of two: window test in the loop, wrap by compare
    "tall": (0.4, 0.2, 16, 32),                            # taller than wide: the literal float64 lookup
}


def params(grid, buffer_size):
    return GRIDS[grid] + (buffer_size,) + synth.REF_TAIL


class MultiOriginOracle(oracle.OracleGvom):
    def process_pointcloud_origins(self, pointcloud, origins, ego_position, transform=None, origin_index=None):
        L, _p = oracle.lib(), oracle._p
        self.ego_position = ego_position
        point_count = pointcloud.shape[0]
        if point_count == 0:
            return
        pc = oracle._as_cloud(pointcloud)
        suf = "f32" if pc.dtype == np.float32 else "f64"
        O = np.ascontiguousarray(np.asarray(origins, np.float64))
        index = np.arange(point_count) % O.shape[0] if origin_index is None else np.asarray(origin_index)
        V = self.voxel_count
        tmp_hit = self._take_v(0)
        tmp_total = self._take_v(0)
        index_map = self._take_v(-1)
        origin = np.zeros(3)
        origin[0] = math.floor((ego_position[0] / self.xy_resolution) - self.xy_size / 2)
        origin[1] = math.floor((ego_position[1] / self.xy_resolution) - self.xy_size / 2)
        origin[2] = math.floor((ego_position[2] / self.z_resolution) - self.z_size / 2)
        if transform is not None:
            tf = np.ascontiguousarray(np.asarray(transform, np.float64))
            getattr(L, "orc_transform_pointcloud_" + suf)(_p(pc), point_count, pc.shape[1], _p(tf))
        L.orc_set_cuda_f32_sqrt(1 if self.cuda_f32_sqrt else 0)
        self.last_scan_updates = 0
        self.adds_per_origin = []
        for k in range(O.shape[0]):
            sub = np.ascontiguousarray(pc[index == k])
            if sub.shape[0] == 0:
                self.adds_per_origin.append(0)
                continue
            ego_k = np.ascontiguousarray(O[k])
            n = getattr(L, "orc_point_2_map_" + suf)(
                self.xy_resolution, self.z_resolution, self.xy_size, self.z_size, self.min_distance,
                _p(sub), sub.shape[0], sub.shape[1], _p(tmp_hit), _p(tmp_total), _p(ego_k), _p(origin))
            self.adds_per_origin.append(int(n))
            self.last_scan_updates += int(n)
        self.last_tmp_total = tmp_total.copy()
        cell_count = L.orc_assign_indices(_p(tmp_hit), _p(tmp_total), _p(index_map), V)
        if cell_count == 0:
            return
        hit = np.empty(cell_count, np.int32); total = np.empty(cell_count, np.int32)
        L.orc_move_data(_p(tmp_hit), _p(hit), _p(index_map), V)
        L.orc_move_data(_p(tmp_total), _p(total), _p(index_map), V)
        min_height = np.ones(cell_count * 3, np.float32)
        self.last_scan_points_in_grid = getattr(L, "orc_calculate_min_height_" + suf)(
            self.xy_resolution, self.z_resolution, self.xy_size, self.z_size, self.min_distance,
            _p(index_map), _p(pc), point_count, pc.shape[1], _p(min_height), _p(origin))
        metrics = None
        if self.voxel_statistics:
            metrics = np.zeros((cell_count, 10), np.float64)
            for ps in (0, 1):
                getattr(L, "orc_calculate_stats_" + suf)(
                    ps, self.xy_resolution, self.z_resolution, self.xy_size, self.z_size,
                    self.min_distance, _p(index_map), _p(pc), point_count, pc.shape[1], _p(metrics),
                    _p(origin), self.xy_eigen_dist, self.z_eigen_dist)
                L.orc_normalize_stats(ps, _p(metrics), cell_count)
        b = self.buffer_index
        self.metrics_buffer[b] = metrics
        self.index_buffer[b] = index_map
        self.hit_count_buffer[b] = hit
        self.total_count_buffer[b] = total
        self.min_height_buffer[b] = min_height
        self.origin_buffer[b] = origin
        self.last_buffer_index = b
        self.buffer_index += 1
        if self.buffer_index >= self.buffer_size:
            self.buffer_index = 0


def single_origin_total(prm, cloud, ego, transform=None):
    """`total` (dense) of the plain single-origin oracle scan of the same cloud: what a build that ignores the origins computes"""
    g = oracle.OracleGvom(*prm)
    pc = oracle._as_cloud(cloud)
    if transform is not None:
        pc = apply_transform(pc, transform)
    origin = [math.floor(ego[0] / prm[0] - prm[2] / 2), math.floor(ego[1] / prm[0] - prm[2] / 2), math.floor(ego[2] / prm[1] - prm[3] / 2)]
    return oracle.point_2_map(prm[0], prm[1], prm[2], prm[3], g.min_distance, pc, ego, origin)[1]


def apply_transform(cloud, tf):
    """the cloud transform in the reference's order of operations (gvom.py:1044-1052): float64, rounded to the cloud's type"""
    pc = np.asarray(cloud)
    tf = np.asarray(tf, np.float64)
    x, y, z = (pc[:, k].astype(np.float64) for k in range(3))
    out = np.stack([((x * tf[k, 0] + y * tf[k, 1]) + z * tf[k, 2]) + tf[k, 3] for k in range(3)], axis=-1)
    return np.ascontiguousarray(out.astype(pc.dtype))


def ego_of(scan):
    return (0.3 * scan + 0.05, -0.2 * scan, 0.04 * scan)


def transform_of(scan):
    """None for the even scans; a yaw + translation for the odd ones (the cloud is handed over in the sensor's frame)"""
    if scan % 2 == 0:
        return None
    return synth.sensor_transform(ego_of(scan), yaw=0.1 * scan)


def cloud_of(grid, scan, dtype):
    """8,192 returns in the WORLD frame of scan `scan`: a 16 x 512 lidar sweep of a scene of boxes (beam-major fans) on the even
    scans of the grids wide enough to hold one, uniformly random returns around the window otherwise"""
    xr, zr, xy, zs = GRIDS[grid]
    ego = ego_of(scan)
    if grid != "tall" and scan % 2 == 0:
        scene = synth.make_scene(2, extent=10.0)
        return synth.lidar_scan(scene, 16, 512, ego, 0.0, scan, dtype, elevations_deg=np.linspace(-24.0, 3.0, 16))
    wx, wz = xr * xy, zr * zs
    pc = synth.uniform_cloud(N, 100 + scan, (ego[0] - 0.6 * wx, ego[0] + 0.6 * wx), (ego[1] - 0.6 * wx, ego[1] + 0.6 * wx),
                             (ego[2] - 0.55 * wz, ego[2] + 0.55 * wz), np.float64)
    return np.ascontiguousarray(pc.astype(dtype))


def scan_inputs(grid, scan, dtype):
    """(cloud as handed over, origins [5, 3], explicit index [N], ego, transform).  The five origins: the ego itself; 0.45
    window widths off in x (the window's edge region: rays longer than half a window); a few decimetres off; 1.5 window widths
    off (outside the window: endpoints only); the exact world coordinates of one return of its own fifth (that ray takes no
    step).  The index assigns contiguous fifths."""
    xr, zr, xy, zs = GRIDS[grid]
    ego, tf = ego_of(scan), transform_of(scan)
    world = cloud_of(grid, scan, dtype)
    assert world.shape == (N, 3)
    index = (np.arange(N) * K // N).astype(np.uint16)
    handed = world
    if tf is not None:
        # the sensor-frame cloud whose transform the scan applies; the world coordinates the scan sees are apply_transform's
        inv = np.linalg.inv(tf)
        handed = np.ascontiguousarray((world.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(dtype))
        world = apply_transform(handed, tf)
    w = xr * xy
    own = np.nonzero(index == K - 1)[0]
    d = np.abs(world[own].astype(np.float64) - np.asarray(ego)).max(axis=1)
    j = own[np.argmin(np.where(d > 0.5, d, np.inf))]          # a return of the last fifth, well inside the window
    origins = np.array([ego,
                        (ego[0] + 0.45 * w, ego[1], ego[2]),
                        (ego[0] + 0.3, ego[1] - 0.2, ego[2] + 0.1),
                        (ego[0] + 1.5 * w, ego[1], ego[2]),
                        world[j].astype(np.float64)], np.float64)
    return handed, origins, index, ego, tf


def column_poses(W, k, travel=1.5):
    """tests/test_range_image.py's kind of column poses -- a slow yaw and a drift along x and z, one 4x4 per column -- with
    `travel` metres of motion per sweep, so that the origins span several voxels"""
    out = np.zeros((W, 4, 4))
    t = np.arange(W) / W
    a = 0.03 * t + 0.01 * k
    out[:, 0, 0] = np.cos(a); out[:, 0, 1] = -np.sin(a); out[:, 1, 0] = np.sin(a); out[:, 1, 1] = np.cos(a)
    out[:, 2, 2] = 1.0; out[:, 3, 3] = 1.0
    out[:, 0, 3] = travel * t; out[:, 2, 3] = -0.05 * t
    return out
