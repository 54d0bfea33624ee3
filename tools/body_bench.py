#!/usr/bin/env python3
"""What body clearance scoring (gvom_score_body: k_body) costs.  On m256 (256 x 256 x 256) and c4 (512 x 512 x 128) with an atlas of
1024 x 1024 x (256 | 128) voxels, after three bench scans and one integrate, against distance_field(2.0) at the window, with a car body of
box_spheres (S is recorded) and arcs from the ego a cell per pose, at K x T = 4096 x 64 and 16384 x 128 -- every loop in a fresh child
process, every child under a `timeout` of its own, and the first child that fails ends the run:

  events       HIP events on the handle's stream around one score_body() call (the map-set route: k_attitude_ground + k_body)
  kernels      k_body, k_attitude_ground and k_attitude alone from ONE rocprofv3 --kernel-trace --stats run of a child of its own
  composition  what a planner had to assemble before this call, as the yardstick: score_attitude(), the K x T x S sphere centres in
               torch from its tangents, sample_device(), torch reductions -- by the wall clock to the drained device; its statuses must
               equal the product's in every pose (torch rounds the centres to float32 on the way to sample_device(): the poses where
               that moved a sphere into another voxel are counted and left out of the comparison)
  attitude     score_attitude() at the same shapes, for scale
  step         scan + combine_maps_device() per step without a query, on this library and, with --parent LIB, on the parent commit's,
               alternating, --turns runs each (default three)
  resources    tools/kernel_regs.py: the new kernel, and registers, scratch, LDS and code size of every kernel outside the new unit on
               the parent and on this library (--resources alone: no GPU needed)

    tools/body_bench.py [--resources] [--parent LIB] [--configs m256,c4] [--turns N] [out.json]   (default: profiles/body_<lib sha8>.json)
"""
import json
import sys
import tempfile
import time

import benchkit as bk

CONFIGS = {"m256": 100, "c4": 40}                        # config: timed steps per repetition
SIDE = 1024
CAP = 2.0
SHAPES = ((4096, 64), (16384, 128))
CAR = dict(front=3.6, rear=1.0, half_width=1.1)            # metres: the footprint of tools/attitude_bench.py
CHASSIS = dict(front_axle=2.7, rear_axle=0.0, track=1.7, belly_height=0.25)
BODY = dict(x0=-1.0, x1=3.6, half_width=0.9, z0=1.0, z1=2.2, radius=0.45)     # metres: box_spheres of the car, its spheres clear of the ground voxels under it
HEADINGS = 64
MIN_MARGIN = 0.2
CHUNK = 256                                                # rollouts per chunk of the torch form
CHILD_TIMEOUT = 420                                        # seconds, per child process
TURNS = 3
KERNELS = ("k_body", "k_attitude_ground", "k_attitude")


def _levels(z_size):
    z = 1
    while z < z_size:
        z *= 2
    return z


def _poses(np, K, T, ego, res, seed=1):
    """K arcs of T poses from the ego, a cell a pose, float32 [K, T, 3]"""
    rng = np.random.default_rng(seed)
    th0 = rng.uniform(-np.pi, np.pi, K)
    curv = rng.uniform(-0.04, 0.04, K)
    th = th0[:, None] + curv[:, None] * np.arange(T)[None, :]
    x = ego[0] + np.cumsum(res * np.cos(th), axis=1)
    y = ego[1] + np.cumsum(res * np.sin(th), axis=1)
    return np.ascontiguousarray(np.stack([x, y, th], axis=2).astype(np.float32))


def _ready(np, gvom, g, dev):
    """three scans, one integrate, the field at the window, the vehicle: (map set, atlas, field, body)"""
    a = g.create_voxel_atlas(SIDE, _levels(g.z_size))
    for scan in dev:
        m = bk.scan_combine(np, g, scan)
    a.integrate()
    g.set_footprint(gvom.rectangle_footprint(CAR["front"], CAR["rear"], CAR["half_width"], g.xy_resolution, headings=HEADINGS))
    g.set_chassis(gvom.chassis(**CHASSIS))
    body = gvom.box_spheres(**BODY)
    g.set_body(body)
    return m, a, a.distance_field(CAP), body


def _composition(torch, g, gvom, m, f, tp, body_t, cs_t, K, T, am):
    """score_attitude, centres in torch, sample_device, torch reductions: (status uint8 [K, T], clearance float32 [K, T], poses whose
    float32 centres fell into another voxel than the float64 ones) -- the definition's arithmetic in torch (which may contract)"""
    att = g._score_attitude(m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin)
    ast = torch.from_dlpack(att.status)
    H = cs_t.shape[0]
    s = torch.tensor(H / (2.0 * 3.141592653589793), dtype=torch.float32, device=tp.device)
    status = torch.empty((K, T), dtype=torch.uint8, device=tp.device)
    clearance = torch.empty((K, T), dtype=torch.float32, device=tp.device)
    moved = torch.zeros((K, T), dtype=torch.bool, device=tp.device)
    res, zres = g.xy_resolution, g.z_resolution
    S = body_t.shape[0]
    bx, by, bz, br = body_t[:, 0].double(), body_t[:, 1].double(), body_t[:, 2].double(), body_t[:, 3]
    for k0 in range(0, K, CHUNK):
        p = tp[k0:k0 + CHUNK]
        n = p.shape[0]
        x, y = p[..., 0].double()[..., None], p[..., 1].double()[..., None]
        h = torch.remainder(torch.round(p[..., 2] * s).long(), H)
        c, sn = cs_t[h][..., 0:1], cs_t[h][..., 1:2]
        # (the attitude product stores the tangents as float32 and not z0: for the definition's float64 frame the composition gathers
        # the four wheel heights again; the product's statuses say where the wheels stand)
        sp, sr, z0 = (v[..., None] for v in _stance(torch, g, m, p, h, cs_t))
        lu, ln = torch.sqrt(1.0 + sp * sp), torch.sqrt((1.0 + sp * sp) + sr * sr)
        e1u, e1w = 1.0 / lu, sp / lu
        nu, nv, nw = -sp / ln, -sr / ln, 1.0 / ln
        e2u, e2v, e2w = nv * e1w, nw * e1u - nu * e1w, -(nv * e1u)
        q0 = z0 - sp * am
        Cu = (bx * e1u + by * e2u) + bz * nu
        Cv = by * e2v + bz * nv
        Z = ((bx * e1w + by * e2w) + bz * nw) + q0
        X, Y = x + (Cu * c - Cv * sn), y + (Cu * sn + Cv * c)
        pts64 = torch.stack([X, Y, Z], dim=-1)
        pts = pts64.float().contiguous()                          # the float32 round trip of the centres
        rr = torch.tensor([res, res, zres], dtype=torch.float64, device=tp.device)
        moved[k0:k0 + n] = (torch.floor(pts64 / rr) != torch.floor(pts.double() / rr)).any(dim=-1).any(dim=-1)
        smp = f.sample_device(pts.data_ptr(), n * T * S)
        d = torch.from_dlpack(smp.distance).view(n, T, S)
        outside = torch.isnan(d).any(dim=-1)                      # (a product's field holds no NaN: NaN is the sample's "outside the box")
        clr = (d - br).amin(dim=-1)
        st = torch.where(clr < MIN_MARGIN, 1, 0).to(torch.uint8)
        st[outside] = 2
        a = ast[k0:k0 + n]
        st[a == gvom.ATTITUDE_UNKNOWN_GROUND] = 3
        st[a == gvom.ATTITUDE_INVALID] = 5
        status[k0:k0 + n], clearance[k0:k0 + n] = st, torch.where(st >= 2, torch.zeros_like(clr), clr)
        smp.release()
    # LEFT_WINDOW: score_attitude walks the footprint, score_body only the wheels -- the composition cannot tell the two apart
    left = ast == gvom.ATTITUDE_LEFT_WINDOW
    att.release()
    return status, clearance, moved, left


def _stance(torch, g, m, p, h, cs_t):
    """(sp, sr, z0) of the four wheel heights, float64 [n, T]"""
    ch = CHASSIS
    half = ch["track"] / 2
    res, xy = g.xy_resolution, g.xy_size
    oc = [int(round(v / res)) for v in m.origin[:2]]
    hgt, inf_h = torch.from_dlpack(m.height_map), torch.from_dlpack(m.inferred_height_map)
    gflat = torch.where(hgt > -1000.0, hgt, inf_h).T.contiguous().view(-1)
    x, y = p[..., 0].double(), p[..., 1].double()
    c, s = cs_t[h][..., 0], cs_t[h][..., 1]
    z = []
    for a, b in ((ch["front_axle"], half), (ch["front_axle"], -half), (ch["rear_axle"], half), (ch["rear_axle"], -half)):
        wx = torch.floor((x + (a * c - b * s)) / res).long() - oc[0]
        wy = torch.floor((y + (a * s + b * c)) / res).long() - oc[1]
        z.append(gflat[wy.clamp(0, xy - 1) * xy + wx.clamp(0, xy - 1)])
    sp = (0.5 * (z[0] + z[1]) - 0.5 * (z[2] + z[3])) / (ch["front_axle"] - ch["rear_axle"])
    sr = (0.5 * (z[0] + z[2]) - 0.5 * (z[1] + z[3])) / ch["track"]
    return sp, sr, 0.25 * ((z[0] + z[1]) + (z[2] + z[3]))


def child_score(name, profiled):
    np, torch, gvom, g, dev = bk.setup(name)
    m, a, f, body = _ready(np, gvom, g, dev)
    ego = dev[2][1]
    res = g.xy_resolution
    stream = torch.cuda.ExternalStream(int(g._lib.gvom_stream(g._h)))
    body_t, cs_t = torch.from_numpy(body).cuda(), torch.from_numpy(g.cos_sin).cuda()
    am = 0.5 * (CHASSIS["front_axle"] + CHASSIS["rear_axle"])
    reps, results = 20, []
    for K, T in SHAPES:
        tp = torch.from_numpy(_poses(np, K, T, ego, res)).cuda()
        torch.cuda.synchronize()
        body_call = lambda: g._score_body(f.product_id, None, None, m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin, MIN_MARGIN)
        att_call = lambda: g._score_attitude(m.set_id, None, gvom._dev(tp.data_ptr()), K, T, 1, True, m.origin)
        if profiled:                                           # under rocprofv3: `reps` launches per call, in this order
            for call in (body_call, att_call):
                for _ in range(reps):
                    call().release()
                bk.sync(g)
            continue
        out = {"xy": g.xy_size, "z": g.z_size, "K": K, "T": T, "S": int(body.shape[0])}
        out["score_body (events on the handle's stream)"] = bk.timed_events(torch, stream, lambda: body_call().release(), reps, warm=3)[0]
        out["score_attitude (events on the handle's stream)"] = bk.timed_events(torch, stream, lambda: att_call().release(), reps, warm=3)[0]
        out["score_body_call_us"] = bk.timed(g, lambda: body_call().release(), reps, digits=2)
        r = body_call()
        summary, clr, pairs = r.copy_to_host()
        r.release()
        out["pose_status_counts"] = np.bincount(pairs[..., 0].ravel(), minlength=6).tolist()
        out["rollout_status_counts"] = np.bincount(summary[:, 0], minlength=6).tolist()
        st, cl, moved, left = (v.cpu().numpy() for v in _composition(torch, g, gvom, m, f, tp, body_t, cs_t, K, T, am))
        judged = ~moved & ~left & (pairs[..., 0] != 4)
        same = st[judged] == pairs[..., 0][judged]
        torch.cuda.synchronize()
        tus = []
        for rep in range(3):
            t0 = time.perf_counter()
            _composition(torch, g, gvom, m, f, tp, body_t, cs_t, K, T, am)
            torch.cuda.synchronize()
            bk.sync(g)
            tus.append(round((time.perf_counter() - t0) * 1e6, 1))
        out["composition"] = {"statuses_equal": bool(same.all()), "statuses_that_differ": int((~same).sum()), "poses_judged": int(judged.sum()),
                              "poses_left_out (a float32 centre in another voxel)": int(moved.sum()),
                              "poses_left_out (LEFT_WINDOW by the footprint or the wheels)": int((left | (pairs[..., 0] == 4)).sum()),
                              "us": tus, "us_median": bk.median(tus), "chunk_rollouts": CHUNK, "intermediate_bytes": K * T * int(body.shape[0]) * 12}
        results.append(out)
    return {"calls": reps, "order": ["score_body", "score_attitude"]} if profiled else {"scoring": results}


def child_step(name, steps):
    np, torch, gvom, g, dev = bk.setup(name)

    def step(k):
        bk.scan_combine(np, g, dev[k % 3]).release()
    return bk.step_loop(g, step, steps, warm=min(10, steps))


def main():
    if bk.child(sys.argv[1:], {"score": lambda a: child_score(a[0], a[1] == "1"), "step": lambda a: child_step(a[0], int(a[1]))}):
        return
    args = bk.read_args(sys.argv[1:], configs=CONFIGS, turns=TURNS)
    parent = args["parent"]
    spawn = lambda mode, a, **kw: bk.spawn(__file__, mode, a, CHILD_TIMEOUT, **kw)
    report, configs = bk.product_report(
        "body", args, {"side": SIDE, "cap_m": CAP, "shapes": [list(s) for s in SHAPES], "body_box_metres": BODY, "chassis": CHASSIS,
                       "headings": HEADINGS, "min_margin_m": MIN_MARGIN}, lambda k: "k_body" in k,
        ["the other form of the kernel (lanes over the spheres of one pose, a shuffle minimum per pose): only one pose per lane is built",
         "bodies of other sizes than the car's", "the pointer routes and the host route", "other depths than 4 gathers in flight",
         "shuffled poses", "the step with a body query per step"])
    if configs is None:
        return
    for name in args["configs"]:
        steps = CONFIGS[name]
        res = spawn("score", (name, 0))
        configs[name] = res
        report.save()
        with tempfile.TemporaryDirectory() as d:                             # the kernels alone: one kernel trace of a child of its own
            spawn("score", (name, 1), profile_dir=d, stats=True)
            res["kernels (rocprofv3 --kernel-trace --stats of a child of its own: both shapes together)"] = bk.kernel_stats(d, KERNELS)
        report.save()
        runs = bk.alternate(args["turns"], {"parent_without": parent and (lambda: spawn("step", (name, steps), lib=parent)),
                                            "without": lambda: spawn("step", (name, steps))})
        step = bk.spreads(runs)
        res["step: scan + combine_maps_device, no query"] = bk.against_parent(step, "without", "parent_without", "without_")
        report.save()
    print(json.dumps(report.out, indent=1))


if __name__ == "__main__":
    main()
