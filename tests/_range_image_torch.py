"""Child process of tests/test_range_image.py: range images that a torch tensor holds in HBM.  torch is imported FIRST, so that
libgvom_hip.so binds to the HIP runtime torch carries (one runtime in the process).  python _range_image_torch.py CASE"""
import os
import sys

import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402

import gvom  # noqa: E402
import synth  # noqa: E402


def case_device_input():
    """the image in device memory, rows 64 bytes longer than a row (the padding filled with ones: it must not be read as
    ranges), with and without column poses == the host route, map for map"""
    params = (0.4, 0.2, 64, 32, 2) + synth.REF_TAIL
    H, W = 16, 512
    scene = synth.make_scene(2, extent=10.0)
    el = np.linspace(-24.0, 3.0, H)
    for rdt, scale in ((np.uint16, 0.001), (np.uint32, 0.001), (np.float32, 1.0)):
        dev, host = gvom.Gvom(*params, voxel_statistics=False), gvom.Gvom(*params, voxel_statistics=False)
        for k in range(3):
            sensor = (0.5 * k, -0.3 * k, 0.05 * k)
            raw, dirs, offs = synth.range_image_scan(scene, H, W, sensor, 0.0, k, rdt, dropout=0.1, elevations_deg=el)
            if k == 0:
                dev.set_sensor_model(dirs, offs, scale)
                host.set_sensor_model(dirs, offs, scale)
            cols = None
            if k == 2:
                cols = np.tile(np.eye(4), (W, 1, 1))
                cols[:, 0, 3] = 0.3 * np.arange(W) / W
            pad = 64 // raw.itemsize
            padded = np.ones((H, W + pad), rdt)
            padded[:, :W] = raw
            t = torch.from_numpy(padded.view(np.uint8).reshape(-1)).cuda()
            torch.cuda.synchronize()                          # the data is ready when the call is made
            tf = synth.sensor_transform(sensor)
            dev.process_range_image_device(t.data_ptr(), rdt, sensor, tf, cols, np.float32, row_stride_bytes=padded.strides[0])
            host.process_range_image(padded[:, :W], sensor, tf, cols)          # (a strided view: the same row stride from the host)
            a, b = dev.read_dense(dev.last_buffer_index), host.read_dense(host.last_buffer_index)
            for u, v in zip(a[:5], b[:5]):
                assert np.array_equal(u, v)
            ma, mb = dev.combine_maps(), host.combine_maps()
            assert ma is not None and int((ma[1] != 0).sum() + (ma[4] != 0).sum()) > 0
            for u, v in zip(ma, mb):
                assert np.array_equal(np.asarray(u), np.asarray(v))
            del t
        # a packed image: the default row stride
        raw, dirs, offs = synth.range_image_scan(scene, H, W, (0.0, 0.0, 0.0), 0.0, 7, rdt, elevations_deg=el)
        t = torch.from_numpy(raw.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        dev.process_range_image_device(t.data_ptr(), rdt, (0.0, 0.0, 0.0))
        host.process_range_image(raw, (0.0, 0.0, 0.0))
        for u, v in zip(dev.combine_maps(), host.combine_maps()):
            assert np.array_equal(np.asarray(u), np.asarray(v))


if __name__ == "__main__":
    name = sys.argv[1]
    globals()["case_" + name]()
    print("CASE OK " + name)
