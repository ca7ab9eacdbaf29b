"""User scenarios at the ABI's limits (helper of test_limit_scenarios.py / test_gpu_limit_scenarios.py).

The eleven limit paths' waypoints come from tests/golden/limits_probe.npz (chosen and recorded by
tests/golden/make_limits_golden.py, next to the reference's fit and probes of them); the package's
QPMIPath fits them, and the circle sets, spawn rectangles and probe points are generated here from
seeded generators.  The CPU tests assert from the oracle alone that these shapes reach the code they
are meant for; the GPU tests then run exactly the same scenarios, actions and points.

Test infrastructure: imports nothing that needs a device.
"""
from __future__ import annotations

import os
import re
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = ["w3_arc", "w3_line", "w3_tiny", "w3_dust", "w3_long", "w4_zig", "w5_zig", "w15_zig", "w16_zig", "w16_arc",
         "w16_long"]
COUNTS = [0, 1, 2, 3, 4, 5, 63, 64]
KINDS = ["uniform", "mixed"]
# (path, circles, radii) of the single-scenario GPU runs; the first eight are the grouped map's scenarios
PAIRINGS = [("w3_arc", 0, "uniform"), ("w3_line", 1, "uniform"), ("w3_tiny", 2, "uniform"), ("w4_zig", 3, "uniform"),
            ("w5_zig", 4, "uniform"), ("w5_zig", 5, "mixed"), ("w15_zig", 63, "uniform"), ("w16_zig", 64, "uniform"),
            ("w16_arc", 64, "mixed"), ("w3_long", 4, "mixed"), ("w16_long", 64, "uniform")]
RESET_CACHE_PAIRINGS = [("w3_tiny", 2, "uniform"), ("w16_zig", 64, "uniform")]
N_SINGLE, N_GROUPED, N_POOL, STEPS = 448, 1001, 1024, 120   # envs and steps of the GPU rollouts
POOL = 64
UNIFORM_R = 25.0

_cache = {}


def fixture():
    if "npz" not in _cache:
        _cache["npz"] = np.load(os.path.join(HERE, "golden", "limits_probe.npz"), allow_pickle=False)
    return _cache["npz"]


def bt_k():
    """BT_K, the recorded steps of a golden-march table, read from csrc/d2d_device.h."""
    import drone2d_amd

    hdr = open(os.path.join(os.path.dirname(drone2d_amd.__file__), "csrc", "d2d_device.h")).read()
    m = re.search(r"^constexpr int BT_K_MAX = (\d+);", hdr, re.M)
    assert m and re.search(r"^constexpr int BT_K = BT_K_MAX;", hdr, re.M)
    return int(m.group(1))


def path(name):
    from drone2d_amd.scenarios import QPMIPath

    if ("path", name) not in _cache:
        _cache["path", name] = QPMIPath(fixture()[f"{name}/wps"])
    return _cache["path", name]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def spawn_rect(name):
    """(xmin, xmax, ymin, ymax): 300 x 300 px around the path's start, reaching 100 px along +x (all
    limit paths head that way), so envs spawn on both sides of the start and fly into the circles."""
    x0, y0 = (float(v) for v in fixture()[f"{name}/wps"][0])
    return (x0 - 200.0, x0 + 100.0, y0 - 150.0, y0 + 150.0)


def circles(name, count, kind):
    """[count, 3] (x, y, r), all near the path's start, where the envs spawn and fly.
    Up to 5 circles: a jittered ring of radius 110 px around the spawn rectangle's centre, inside the
    rectangle, so every circle is the nearest, the second and the third for some spawn.
    63 and 64 circles: centres scattered around the path (path(u) for u up to 700 px, +- 150 px; around
    the start for the short paths), at least 120 px off the spawn rectangle's centre, and the LAST index
    on that centre: the nearest circle for the spawns around it, the one a truncated table loses."""
    if count == 0:
        return np.zeros((0, 3))
    rng = _rng("circles", name, count, kind)
    p = path(name)
    xmin, xmax, ymin, ymax = spawn_rect(name)
    ctr = np.array([0.5 * (xmin + xmax), 0.5 * (ymin + ymax)])
    if count <= 5:
        a = rng.uniform(0.0, 2.0 * np.pi) + 2.0 * np.pi * np.arange(count) / count
        out = ctr + 110.0 * np.stack([np.cos(a), np.sin(a)], -1) + rng.uniform(-20.0, 20.0, (count, 2))
    else:
        reach = min(float(p.length), 700.0)
        out = []
        while len(out) < count:
            c = np.asarray(p(rng.uniform(0.0, reach))) + rng.uniform(-150.0, 150.0, 2)
            if reach < 300.0:
                c = c + rng.uniform(-250.0, 250.0, 2)
            if np.hypot(*(c - ctr)) >= 120.0:
                out.append(c)
        out = np.array(out)
        out[-1] = ctr
    r = np.full(count, UNIFORM_R) if kind == "uniform" else rng.uniform(10.0, 40.0, count)
    return np.concatenate([out, r[:, None]], 1)


def scenario(name, count=0, kind="uniform", drop_last=False):
    from drone2d_amd.scenarios import Scenario

    c = circles(name, count, kind)
    if drop_last:
        c = c[:-1]
    return Scenario(f"{name}_{count}{kind[0]}", np.asarray(fixture()[f"{name}/wps"]), path(name), c, spawn_rect(name))


def actions(tag, n, steps=STEPS):
    """float32 [steps, n, 2], U(-1, 1): the actions of the rollout named tag, on the CPU and on the GPU."""
    return _rng("actions", tag, n, steps).uniform(-1.0, 1.0, (steps, n, 2)).astype(np.float32)


def grouped_map():
    """The grouped-map run: N_GROUPED envs over the first eight pairings with a ragged map -- scenario 5
    has 3 envs, scenario 6 none, and (1001 envs, uneven shares) groups straddle two scenarios."""
    rng = _rng("grouped")
    es = rng.choice(8, size=N_GROUPED, p=[0.25, 0.2, 0.15, 0.15, 0.1, 0.0, 0.0, 0.15]).astype(np.int32)
    es[[5, 500, 1000]] = 5
    return [scenario(*p) for p in PAIRINGS[:8]], es


def pool_scenarios():
    """POOL scenarios for d2d_refresh_pool: the pairings cycled (the library takes 3-waypoint paths in
    pool mode like any other), so the lanes of one wave hold different n_wps and n_circles."""
    return [scenario(*PAIRINGS[k % len(PAIRINGS)]) for k in range(POOL)]


def pool_kwargs():
    """The curriculum-pool handle whose pool the limit scenarios replace (short episodes: many resets)."""
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, scenario="stage_5", mode="curriculum", curriculum_pool=POOL, curriculum_seed=9,
                n_steps=40)


POOL_SEED, POOL_STEPS_BEFORE, POOL_STEPS_AFTER = 23, 5, 100


def rollouts():
    """tag -> (scenarios, n_envs, env_scenario or None, seed, config overrides, steps): every static-map
    rollout a GPU test runs, so the CPU tests can run the same in the oracle."""
    out = {}
    for p in PAIRINGS:
        out["single/%s-%d-%s" % p] = ([scenario(*p)], N_SINGLE, None, 31, {}, STEPS)
    scns, es = grouped_map()
    out["grouped"] = (scns, N_GROUPED, es, 32, {}, STEPS)
    for p in RESET_CACHE_PAIRINGS:
        out["cache/%s-%d-%s" % p] = ([scenario(*p)], 512, None, 33, {"n_steps": 3}, 30)
    return out


def oracle_batch(scns, n, env_scenario, over, auto_reset=True):
    import oracle
    from drone2d_amd.config import ENV_TRAIN_CONFIG, make_cfg

    cfg = make_cfg(dict(ENV_TRAIN_CONFIG, **over), auto_reset=auto_reset)
    es = np.arange(n) % len(scns) if env_scenario is None else env_scenario
    return oracle.OracleBatch(cfg, [s.to_c() for s in scns], n, env_scenario=es)


def end_points(name, n_each=48):
    """Points behind the start along the start tangent and beyond the end along the end tangent, from
    0.5 px to 2 000 px off the search bounds' points path(-10) and path(L + 10), on the tangent and a
    little beside it."""
    import oracle

    sc = scenario(name).to_c()
    L = float(path(name).length)
    rng = _rng("ends", name)
    out = []
    for u0, sign in ((-10.0, -1.0), (L + 10.0, 1.0)):
        p0 = np.array(oracle.path_eval(sc, u0))
        tg = sign * (np.array(oracle.path_eval(sc, u0 + 1e-3)) - np.array(oracle.path_eval(sc, u0 - 1e-3)))
        tg /= np.hypot(*tg)
        nm = np.array([-tg[1], tg[0]])
        d = np.geomspace(0.5, 2000.0, n_each)
        side = np.where(np.arange(n_each) % 4 == 3, rng.uniform(-0.5, 0.5, n_each), 0.0) * d
        out.append(p0 + d[:, None] * tg + side[:, None] * nm)
    return np.concatenate(out)


def far_points(name):
    """Points from which the search marches down to an end and stays there.  From four waypoints on,
    path(u < 0) blends in the LAST quadratic (Python's x_params[-1]): a 10-unit stub far from the start, which
    a local search reaches only if the distance falls all the way along the path and the stub is nearer than
    the start.  So: far behind the stub path(-5) against the path's overall direction (3 000 and 10 000 px, a
    fan of +-60 degrees), and the mirror image beyond path(L + 5)."""
    import oracle

    sc = scenario(name).to_c()
    wps = fixture()[f"{name}/wps"]
    L = float(path(name).length)
    t = (wps[-1] - wps[0]) / np.hypot(*(wps[-1] - wps[0]))
    out = []
    for u0, sign, wp in ((-5.0, -1.0, wps[0]), (L + 5.0, 1.0, wps[-1])):
        q = np.array(oracle.path_eval(sc, u0))
        for D in (3000.0, 10000.0):
            for phi in np.deg2rad(np.linspace(-60.0, 60.0, 7)):
                c, s = np.cos(phi), np.sin(phi)
                out.append(q + sign * D * np.array([c * t[0] - s * t[1], s * t[0] + c * t[1]]))
        # a long path's stub lies far beside its start (16 zigzag waypoints: 200 times the zigzag's height):
        # from beside the stub's side of the end waypoint, so far out that the way along the path is mostly
        # towards the point
        w = q - wp
        for D in (2.0, 5.0):
            for f in (0.6, 0.8, 1.0):
                out.append(wp + f * w + sign * (D * np.hypot(*w) + 3000.0) * t)
    return np.array(out)


def grid_points(name, per):
    """The `per` points of the GPU closest-point test on one path: the fixture's points, end_points,
    far_points, four points inside every knot interval, a 12 x 12 grid 600 px around the waypoints' bounding
    box, and points within +-40 px of the path."""
    assert per >= 512
    wps = fixture()[f"{name}/wps"]
    L = float(path(name).length)
    rng = _rng("grid", name)
    lo, hi = wps.min(0) - 600.0, wps.max(0) + 600.0
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 12), np.linspace(lo[1], hi[1], 12))
    # four points per knot interval, off the path by a hundredth of the interval's length
    us = np.asarray(path(name).us)
    ui = (us[:-1, None] + np.diff(us)[:, None] * np.array([0.2, 0.4, 0.6, 0.8])[None, :]).ravel()
    off = 0.01 * np.repeat(np.diff(us), 4)[:, None] * rng.uniform(-1.0, 1.0, (len(ui), 2))
    on = np.array([path(name)(x) for x in ui]) + off
    head = np.concatenate([fixture()[f"{name}/pts"], end_points(name), far_points(name), on,
                           np.stack([gx, gy], -1).reshape(-1, 2)])
    u = rng.uniform(-10.0, L + 10.0, per - len(head))
    near = np.array([path(name)(x) for x in u]) + rng.uniform(-40.0, 40.0, (len(u), 2))
    return np.concatenate([head, near])


def states_at(pts):
    """(state [NSTATE, n], istate [NISTATE, n]): drones at rest at pts, level (motors at frame -+ 40)."""
    from drone2d_amd import abi

    n = len(pts)
    st = np.zeros((abi.NSTATE, n))
    st[0], st[1] = pts[:, 0], pts[:, 1]
    st[6], st[7] = pts[:, 0] - 40.0, pts[:, 1]
    st[12], st[13] = pts[:, 0] + 40.0, pts[:, 1]
    return st, np.zeros((abi.NISTATE, n), np.int32)
