"""The window's and the voxel atlas's walk queries check their arrays with one text (gvom._ray_segments, gvom._align_cloud): Gvom.raycast
and VoxelAtlas.raycast, Gvom.score_alignments and VoxelAtlas.score_alignments raise the same exception, type and message, for the same
bad arrays.  On the CPU: a Gvom and a VoxelAtlas made with __new__ (no handle) whose `_lib` is None -- a call into the library would be
an AttributeError, not the exception expected here."""
import numpy as np
import pytest


def _pair():
    import gvom
    g = gvom.Gvom.__new__(gvom.Gvom)
    g._lib, g._h = None, None
    a = gvom.VoxelAtlas.__new__(gvom.VoxelAtlas)
    a._owner = g
    return g, a


GOOD = np.zeros((4, 3), np.float32)
TF = np.zeros((2, 4, 4), np.float64)
RAYS = {   # bad (origins, targets) -> the exception
    "a dtype numpy cannot cast": ((np.zeros(3), np.array([["a", "b", "c"]])), ValueError),     # (numpy's own refusal: the binding casts every number)
    "a wrong rank": ((np.zeros(3), np.zeros(3)), ValueError),
    "zero rows": ((np.zeros(3), np.zeros((0, 3))), ValueError),
    "origins of a wrong shape": ((np.zeros((2, 3)), GOOD), ValueError),
}
CLOUDS = {  # bad cloud -> the exception
    "a wrong dtype": (np.zeros((4, 3), np.float64), TypeError),
    "a wrong rank": (np.zeros(3, np.float32), ValueError),
    "zero rows": (np.zeros((0, 3), np.float32), ValueError),
    "a wrong number of columns": (np.zeros((4, 2), np.float32), ValueError),
}


def _raised(call, kind):
    with pytest.raises(kind) as e:
        call()
    assert type(e.value) is kind
    return str(e.value)


@pytest.mark.parametrize("bad", list(RAYS))
def test_both_raycasts_refuse_the_same_arrays_alike(bad):
    g, a = _pair()
    (origins, targets), kind = RAYS[bad]
    msg = _raised(lambda: g.raycast(origins, targets), kind)
    assert msg and msg == _raised(lambda: a.raycast(origins, targets), kind)


@pytest.mark.parametrize("bad", list(CLOUDS))
def test_both_alignment_calls_refuse_the_same_arrays_alike(bad):
    g, a = _pair()
    cloud, kind = CLOUDS[bad]
    msg = _raised(lambda: g.score_alignments(cloud, TF), kind)
    assert msg and msg == _raised(lambda: a.score_alignments(cloud, TF), kind)
