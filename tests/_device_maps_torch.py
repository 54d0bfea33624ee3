"""Child process of tests/test_device_maps.py: the cases with a torch consumer.  torch is imported FIRST, so that
libgvom_hip.so binds to the HIP runtime torch carries (one runtime in the process).  python _device_maps_torch.py CASE"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gc  # noqa: E402

import numpy as np  # noqa: E402

import gvom  # noqa: E402
import synth  # noqa: E402


def _m256(n_scans=1):
    params, scans = synth.config_inputs("m256", n_scans=n_scans)
    return gvom.Gvom(*params, voxel_statistics=False), scans


def case_zero_copy():
    g, scans = _m256()
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    xy = g.xy_size
    sets = g.get_tuning("device_map_sets")
    for name in gvom.DEVICE_MAP_NAMES:
        dm = getattr(m, name)
        want = dm.copy_to_host()
        tdt = torch.int32 if want.dtype == np.int32 else torch.float64
        assert dm.__dlpack_device__() == (10, 0)
        stream = torch.cuda.current_stream().cuda_stream
        for t in (torch.from_dlpack(dm), torch.from_dlpack(dm.__dlpack__(stream=stream))):    # versioned, legacy capsule
            assert t.device == torch.device("cuda:0") and t.dtype == tdt
            assert tuple(t.shape) == (xy, xy) and t.stride() == (1, xy)
            assert t.data_ptr() == dm.ptr
            assert np.array_equal(t.cpu().numpy(), want)
            del t
        cap = dm.__dlpack__(max_version=(1, 0))          # never consumed: its destructor gives the export back
        del cap
        for kw in ({"copy": True}, {"dl_device": (1, 0)}):
            try:
                dm.__dlpack__(**kw)
                raise AssertionError("accepted %r" % (kw,))
            except BufferError:
                pass
    torch.cuda.synchronize()
    m.release()
    g.process_pointcloud(*scans[0])
    g.combine_maps_device().release()                    # every export came back: the set is reused
    assert g.get_tuning("device_map_sets") == sets


def case_reuse_waits():
    g, scans = _m256(n_scans=4)
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    want = m.height_map.copy_to_host()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = torch.from_dlpack(m.height_map)
        torch.cuda._sleep(200_000_000)                    # the consumer is slow...
        clone = t.clone()
        del t                                             # ...and drops its tensor at once: the release is stream-ordered
    m.release()
    del m
    for pc, ego, tf in scans[1:]:                         # the set is free now: the next combines reuse it
        g.process_pointcloud(pc, ego, tf)
        g.combine_maps_device().release()
    side.synchronize()
    got = clone.cpu().numpy()
    assert not np.array_equal(want, g.height_map.copy_to_host())     # (the later combines wrote other maps)
    assert np.array_equal(got, want)


def case_pool():
    g, scans = _m256()
    for k in range(50):
        g.process_pointcloud(*scans[0])
        m = g.combine_maps_device()
        t = torch.from_dlpack(m.roughness)
        s = float(t.sum())
        del t
        m = None
        assert s == s
    assert 1 <= g.get_tuning("device_map_sets") <= 3
    held = []
    for k in range(8):
        g.process_pointcloud(*scans[0])
        held.append(g.combine_maps_device())
    assert g.get_tuning("device_map_sets") == 8
    g.process_pointcloud(*scans[0])
    try:
        g.combine_maps_device()
        raise AssertionError("a ninth set was handed out")
    except gvom.GvomBackendError as e:
        assert "device map sets" in str(e), e
    for m in held:
        m.release()
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    assert m is not None and g.get_tuning("device_map_sets") == 8
    m.release()


def case_outlives():
    g, scans = _m256()
    g.process_pointcloud(*scans[0])
    m = g.combine_maps_device()
    want = m.guessed_height_delta.copy_to_host()
    t = torch.from_dlpack(m.guessed_height_delta)
    m.release()
    del m, g
    gc.collect()
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), want)
    del t                                                 # the last release frees the orphaned set
    torch.cuda.synchronize()


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
