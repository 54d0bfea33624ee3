"""CPU-side checks of the drop-in boundary: libgvom_hip.so loads and exports every symbol
include/gvom_hip.h declares (no compute calls without a GPU); the Python class mirrors the
reference's surface and fails loudly -- never silently falls back -- when the GPU is absent."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gvom_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import ctypes
    import gvom
    path = gvom.library_path()
    assert os.path.exists(path), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = ctypes.CDLL(path)
    declared = _declared_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(L, name), "libgvom_hip.so does not export %s" % name
    bound = {n for n, _, _ in gvom.ABI}
    assert set(declared) == bound, (set(declared) ^ bound)
    import re
    header = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    declared_version = int(re.search(r"#define\s+GVOM_ABI_VERSION\s+(\d+)", header).group(1))
    assert gvom.load_library().gvom_abi_version() == declared_version == gvom.ABI_VERSION


def test_params_struct_layout_matches_header():
    import ctypes
    import gvom
    assert ctypes.sizeof(gvom.GvomParams) == 8 * 2 + 4 * 4 + 8 * 7 + 4 * 2
    assert gvom.GvomParams.min_distance.offset == 32
    assert ctypes.sizeof(gvom.GvomState) == 16 + 8 + 24 + 24


def test_constructor_signature_matches_reference():
    import gvom
    names = list(inspect.signature(gvom.Gvom.__init__).parameters)[1:15]
    assert names == ["xy_resolution", "z_resolution", "xy_size", "z_size", "buffer_size",
                     "min_distance", "positive_obstacle_threshold", "negative_obstacle_threshold",
                     "slope_obstacle_threshold", "robot_height", "robot_radius",
                     "ground_to_lidar_height", "xy_eigen_dist", "z_eigen_dist"]
    for m in ("process_pointcloud", "combine_maps", "get_map_as_occupancy_grid",
              "make_debug_voxel_map", "make_debug_height_map", "make_debug_inferred_height_map"):
        assert callable(getattr(gvom.Gvom, m))
    sig = inspect.signature(gvom.Gvom.process_pointcloud)
    assert list(sig.parameters)[1:] == ["pointcloud", "ego_position", "transform"]
    assert sig.parameters["transform"].default is None
    # keyword extensions come behind the reference's 14 and default to its behaviour: statistics for as long as somebody reads
    # them (None), Fortran-ordered views of the GPU's own output unless c_order is asked for
    extra = {p.name: p.default for p in list(inspect.signature(gvom.Gvom.__init__).parameters.values())[15:]}
    assert extra["voxel_statistics"] is None and extra["c_order"] is False and extra["device"] == 0
    # the reference object's remaining attributes (gvom.py:54, 65-67, 94, 96) are set by the constructor
    src = inspect.getsource(gvom.Gvom.__init__)
    for attr in ("self.semaphores", "self.ego_semaphore", "self.metrics", "self.blocks"):
        assert attr in src, attr


def test_test_hooks_live_in_the_test_library_only():
    """"epoch_bias", "churn" and the GVOM_TEST_IPC_REFUSE fault injector are documented in
    include/gvom_hip_test.h and compiled into lib/libgvom_hip_test.so (-DGVOM_TEST_HOOKS: the production sources + the hooks);
    the production library contains none of the three strings, exports exactly the same symbols, and its public header does
    not mention them."""
    pkg = os.path.join(ROOT, "g-vom_amd")
    build = subprocess.run(["make", "-j6", "-C", pkg, "lib/libgvom_hip.so", "lib/libgvom_hip_test.so"], capture_output=True, text=True, timeout=900)
    assert build.returncode == 0, build.stderr[-2000:]
    prod, test = os.path.join(pkg, "lib", "libgvom_hip.so"), os.path.join(pkg, "lib", "libgvom_hip_test.so")
    blob_p, blob_t = open(prod, "rb").read(), open(test, "rb").read()
    for hook in (b"GVOM_TEST_IPC_REFUSE", b"epoch_bias", b"churn"):
        assert hook not in blob_p, hook
        assert hook in blob_t, hook

    def exported(path):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
        return {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln and ln.split()[-1].startswith("gvom_")}
    assert exported(prod) == exported(test) and len(exported(prod)) >= 60
    public = open(os.path.join(ROOT, "include", "gvom_hip.h")).read()
    for word in ("GVOM_TEST_IPC_REFUSE", "epoch_bias", "\"churn\""):
        assert word not in public, word
    hooks = open(os.path.join(ROOT, "include", "gvom_hip_test.h")).read()
    for word in ("GVOM_TEST_IPC_REFUSE", "epoch_bias", "churn"):
        assert word in hooks


def test_identity_hashes_every_source_of_the_library():
    """tools/lib_identity.py takes its list from the Makefile (UNITS, HDR): every unit and header under csrc/ is in it -- a file
    left out would not change the source_sha256 stamped into the profile sidecars -- every listed file exists, and `make sources`
    prints the same list."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lib_identity", os.path.join(ROOT, "tools", "lib_identity.py"))
    lib_identity = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib_identity)
    pkg = os.path.join(ROOT, "g-vom_amd")
    listed = lib_identity.sources()
    assert len(listed) == len(set(listed))
    for rel in listed:
        assert os.path.isfile(os.path.join(pkg, rel)), rel
    on_disk = {"csrc/" + f for f in os.listdir(os.path.join(pkg, "csrc")) if f.endswith((".hip", ".h"))}
    assert on_disk and on_disk <= set(listed), sorted(on_disk - set(listed))
    assert {"../include/gvom_hip.h", "../include/gvom_hip_test.h", "Makefile"} <= set(listed)
    printed = subprocess.run(["make", "-s", "-C", pkg, "sources"], capture_output=True, text=True, check=True).stdout.split()
    assert printed == listed


def test_no_silent_cpu_fallback():
    """Without a GPU the product must refuse to run, not quietly compute on the CPU."""
    import gvom
    rc, info = gvom.Gvom.backend_info()
    if rc == 0:
        pytest.skip("a GPU is visible: %s" % info)
    with pytest.raises(gvom.GvomBackendError):
        gvom.Gvom(0.4, 0.4, 16, 8, 2, 1.0, 0.5, 0.5, 0.3, 2.0, 4.0, 1.0, 1, 1)
    with pytest.raises(gvom.GvomBackendError):
        gvom.load_library("/nonexistent/libgvom_hip.so")


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "g-vom_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.lower(), "%s mentions the oracle" % f


def test_synthetic_inputs_are_seeded_and_shaped():
    import synth
    params, scans = synth.config_inputs("c2")
    pc, ego, tf = scans[0]
    assert pc.shape == (131072, 3) and pc.dtype == np.float32 and tf is None
    params2, scans2 = synth.config_inputs("c2")
    assert np.array_equal(pc, scans2[0][0])
    assert np.isfinite(pc).all() and np.linalg.norm(pc, axis=1).max() <= 60.001
    p1, s1 = synth.config_inputs("c1")
    assert s1[0][0].shape == (50000, 3) and s1[0][0].dtype == np.float64


def test_hot_kernels_use_no_scratch_and_keep_their_occupancy():
    """The code objects inside the built library: the four hot kernels (every instantiation) must not touch scratch memory, and
    k_trace must fit 8 waves per SIMD (<= 64 VGPRs).  Round 4 lost 9 us of k_trace's 40 to an innocent-looking helper inlined
    into it -- 20 bytes of scratch, set up by every wave of the launch -- which no functional test can see."""
    import sys
    import gvom
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    if not os.path.exists(os.path.join(kernel_regs.LLVM, "clang-offload-bundler")):
        pytest.skip("no ROCm LLVM tools")
    kernels = kernel_regs.kernels(gvom.library_path())
    hot = {k: v for k, v in kernels.items() if any(n in k for n in ("7k_trace", "8k_encode", "7k_fuse4", "7k_fuse1", "6k_fuse", "7k_map2d"))}
    assert len(hot) >= 12, sorted(kernels)
    for k, v in hot.items():
        assert v["scratch"] == 0, (k, v)
        if "7k_trace" in k:
            assert v["vgpr"] <= 64, (k, v)
