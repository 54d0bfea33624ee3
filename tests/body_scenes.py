"""The scenes of the body clearance tests that go through REAL products (tests/test_body.py on the GPU, tests/test_body_cpu.py on the CPU
oracle): one scan each, then combine, integrate, distance field, body scoring.

  post   the 40 x 40 x 6 grid at 0.3 / 0.2 m of tests/test_voxel_distance.py (resolutions that round), posts on rolling ground, the ego low
         enough that the ground lies inside the window's six levels
  gate   48 x 48 x 16 at 0.25 / 0.2 m: flat ground at 0.1 m, a ramp of slope 0.3 in the lane 1 m <= y < 4 m that rises from x = -1 m to a
         plateau at x = 3 m, and a bar across the way -- one voxel thick at x = 2 m, over every y -- at the fixed height 2.1 m

The physical statement of the gate scene, held on the GPU's result and on the CPU oracle's alike (hold_statement):
  the low body passes under the bar on the flat approach, OK in every pose;
  the tall body collides there, with a top sphere tightest at the pose nearest the bar;
  on the ramp approach the low body collides nose-up where the untilted frame (sp = sr = 0, the same z0) says OK."""
import functools

import numpy as np

import attitude_ref as ar
import body_ref as br
import obstacle_scenes
import rollouts_ref as rr

SCENES = {"post": dict(res=0.3, zres=0.2, xy=40, zs=6, ego=(1.7, -2.9, -0.7)),
          "gate": dict(res=0.25, zres=0.2, xy=48, zs=16, ego=(0.0, 0.0, 1.0))}
HEADINGS = 16
CHASSIS = ar.make_chassis(0.7, -0.3, 0.6, 0.2)
CAP = 2.0                                                   # metres: the distance fields' max_distance
MIN_MARGIN = np.float32(0.15)
DISPLACED = (5, -3, 1)
BAR_X, BAR_Z, RAMP_SLOPE = 2.0, 2.1, 0.3
FLAT_Y, RAMP_Y = -2.0, 2.5                                  # the lanes of the two approaches
TOP_Z = 2.0                                                 # the tall body's top spheres


def _grid(x0, x1, y0, y1, step):
    x, y = np.meshgrid(np.arange(x0, x1, step), np.arange(y0, y1, step), indexing="ij")
    return x.ravel(), y.ravel()


def ground_height(x, y):
    """the gate scene's ground in metres"""
    on_ramp = (y >= 1.0) & (y < 4.0)
    return np.where(on_ramp, 0.1 + RAMP_SLOPE * np.clip(x + 1.0, 0.0, 4.0), 0.1)


@functools.lru_cache(maxsize=None)
def cloud(name):
    """the scene's one scan, float32 [N, 3]; shared, read-only"""
    S = SCENES[name]
    if name == "post":
        return obstacle_scenes.post_scene(3, S["xy"], S["res"], S["zres"], S["ego"], n_posts=40, ground_pts=6000)
    gx, gy = _grid(-5.6, 5.6, -5.6, 5.6, 0.06)
    bx, by = _grid(BAR_X + 0.02, BAR_X + 0.25, -5.6, 5.6, 0.04)
    pts = np.concatenate([np.stack([gx, gy, ground_height(gx, gy)], 1), np.stack([bx, by, np.full(bx.shape, BAR_Z)], 1)], 0)
    return np.ascontiguousarray(pts.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _bodies(name):
    import gvom
    if name == "post":                                      # six levels of 0.2 m: a body that fits between the ground and the window's top
        low = gvom.box_spheres(-0.3, 0.9, 0.3, 0.3, 0.5, 0.1)
        top = np.array([(bx, by, 0.7, 0.1) for bx in (0.0, 0.6) for by in (-0.2, 0.2)], np.float32)
    else:
        low = gvom.box_spheres(-0.3, 1.5, 0.3, 0.9, 1.2, 0.15)
        top = np.array([(bx, by, TOP_Z, 0.15) for bx in (0.0, 0.6, 1.2) for by in (-0.2, 0.2)], np.float32)
    return {"low": low, "tall": np.concatenate([low, top], 0)}


def bodies(name="gate"):
    """{"low", "tall"}: float32 [S, 4]; the tall body is the low one with a few top spheres behind it in the table"""
    return dict(_bodies(name))


@functools.lru_cache(maxsize=None)
def poses(name):
    """float32 [K, T, 3].  gate: rollout 0 drives the flat lane and rollout 1 the ramp lane, both along +x from x = -3 m a cell per pose
    through the gate; the others are arcs about the ego.  post: arcs about the ego."""
    S = SCENES[name]
    res, xy = S["res"], S["xy"]
    oc = tuple(int(np.floor(S["ego"][k] / res - xy / 2.0)) for k in range(2))
    centre = tuple(int(np.floor(S["ego"][k] / res)) - oc[k] for k in range(2))
    T = 24
    arcs = rr.arc_poses(30, T, xy, res, oc, 11, spread=xy / 4.0, centre=centre)
    if name == "gate":
        x = -3.0 + res * np.arange(T)
        for k, y in enumerate((FLAT_Y, RAMP_Y)):
            arcs[k] = np.stack([x, np.full(T, y), np.zeros(T)], 1).astype(np.float32)
    arcs[5, 7] = np.nan
    return arcs


def hold_statement(name, seen, untilted_low):
    """seen = {"low": (summary, clearance, pairs), "tall": ...} at the window's box with the inferred ground; untilted_low = the referee's
    result for the low body in the untilted frame.  The gate scene's three statements; the post scene only has to reach OK and COLLISION."""
    low, tall = seen["low"], seen["tall"]
    if name != "gate":
        assert (low[2][..., 0] == br.OK).sum() >= 20 and (tall[2][..., 0] == br.COLLISION).sum() >= 20
        return
    n_low = len(bodies()["low"])
    x = poses(name)[0, :, 0]
    # 1. the low body passes under the bar on the flat approach
    assert low[0][0].tolist()[:2] == [br.OK, len(x)], low[0][0].tolist()
    assert (low[1][0] >= MIN_MARGIN).all()
    # 2. the tall body collides there, a top sphere tightest, at the pose nearest the bar
    assert tall[0][0, 0] == br.COLLISION, tall[0][0].tolist()
    hit = np.nonzero(tall[2][0, :, 0] == br.COLLISION)[0]
    worst = int(np.argmin(tall[1][0]))
    assert tall[2][0, worst, 1] >= n_low and abs(float(x[worst]) + 0.6 - (BAR_X + 0.125)) <= 0.9, (worst, tall[2][0, worst].tolist())
    assert all(tall[2][0, t, 1] >= n_low for t in hit)
    # 3. on the ramp approach the low body collides nose-up where the untilted frame says OK
    first = int(low[0][1, 1])
    assert low[0][1, 0] == br.COLLISION and first < len(x), low[0][1].tolist()
    if untilted_low is not None:
        assert untilted_low[2][1, first, 0] == br.OK and untilted_low[0][1, 1] > first, (first, untilted_low[0][1].tolist())
