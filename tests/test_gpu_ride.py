"""Table followers riding K1's continuation loop (BT_RIDE, bt_finish_join) -- needs an MI355X.

Under the early start the path wave re-checks steps [1, E) of the golden-march table and resumes its
deviating lanes at once.  The lanes that followed [1, E) now ride that loop: they run brent_step from
the snapshot before step E for at least R passes, the other wave re-checks [E + R, len) only, and at
the join a rider jumps along the table only if its state equals the table's snapshot bit for bit.
That code runs only when there are more workgroups than CUs, so every test here uses corridor, the
env-ordered layout and 64 x (CU count + 1) envs.

1. crafted points, one step, bitwise against the oracle, every class of lane present;
2. crafted 64-lane groups (riders alone / early lanes done before pass R / long after it / first
   deviations at E, E + R - 1 and E + R side by side / no rider), bitwise, and the same twice: the
   moment of the join depends on timing, the result must not;
3. a teacher-forced run with auto-reset against the oracle;
4. the constants below against the header.
"""
import os
import re
import sys

import numpy as np
import pytest

from parity_util import compare_step, make_pair
from test_gpu_early_start import _assert_bitwise, _cfgkw, _n_envs, _step_points

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

E = 16          # BT_EARLY
R = 15          # BT_RIDE (csrc/d2d_device.h; test_constants_match_kernel)


def test_constants_match_kernel():
    import drone2d_amd

    hdr = open(os.path.join(os.path.dirname(drone2d_amd.__file__), "csrc", "d2d_device.h")).read()
    for name, val in (("D2D_BT_EARLY", E), ("D2D_BT_RIDE", R)):
        m = re.search(r"^#define %s (\d+)$" % name, hdr, re.M)
        assert m and int(m.group(1)) == val, name


@pytest.fixture(scope="module")
def points():
    """Crafted points on corridor, classified on the CPU by the scipy restatement of
    tools/brent_lanes.py: pts [m, 2], kind, dev, cont (continuation steps), kind_len.  A grid, points
    near the path, and fans around the two extrapolated ends (where the table marches converge: the
    later a search leaves its march, the closer its point lies to the end's normal)."""
    import brent_lanes as bl
    import oracle
    from drone2d_amd.env import build_scenarios

    scn = build_scenarios(_cfgkw())[0]
    sc = scn.to_c()
    L = float(scn.path.length)
    rng = np.random.default_rng(23)
    g = np.linspace(-600.0, 1900.0, 40)
    grid = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    u = rng.uniform(-10.0, L + 10.0, 1024)
    near = np.array([scn.path(x) for x in u]) + rng.normal(0.0, 40.0, (len(u), 2))
    fans = []
    for ue in (-10.0, L + 10.0):
        p0 = np.array(oracle.path_eval(sc, ue))
        tg = np.array(oracle.path_eval(sc, ue + 1e-3)) - np.array(oracle.path_eval(sc, ue - 1e-3))
        tg /= np.hypot(*tg)
        nm = np.array([-tg[1], tg[0]])
        # along the tangent from 1e-4 to 30 on both sides (geometric: each decade moves dev by ~5)
        b = np.geomspace(1e-4, 30.0, 60)
        b = np.concatenate([-b, b])
        a, b = np.meshgrid(np.linspace(-300.0, 300.0, 21), b)
        fans.append(p0 + a.reshape(-1, 1) * nm + b.reshape(-1, 1) * tg)
    pts = np.concatenate([grid, near, *fans])
    kind_len = [bl.forced_len(L, 0), bl.forced_len(L, 1)]
    cls = np.array([bl.classify(sc, L, kind_len, x, y) for x, y in pts])
    return dict(pts=pts, kind=cls[:, 0], dev=cls[:, 1], cont=cls[:, 2], kind_len=kind_len)


def _classes(P):
    kind, dev = P["kind"], P["dev"]
    whole = dev == np.array(P["kind_len"])[kind]
    return {"whole0": whole & (kind == 0), "whole1": whole & (kind == 1), "early": ~whole & (dev < E),
            "ride": ~whole & (dev >= E) & (dev < E + R), "late": ~whole & (dev >= E + R)}, whole


def test_crafted_points_bitwise(d2, points):
    """Every class of lane -- whole table followed (both kinds), first deviation below E, in
    [E, E + R) (the lane leaves the table while riding), in [E + R, len) (found by the other wave) --
    in one step, bit for bit the oracle's closest and lookahead points and path error."""
    cls, _ = _classes(points)
    for name, m in cls.items():
        print(name, int(m.sum()))
        assert m.any(), name
    n = _n_envs()
    # every class in every part of the batch: one point of each first, then the whole set in turn
    first = np.array([np.flatnonzero(m)[0] for m in cls.values()])
    order = np.concatenate([first, np.arange(n - len(first)) % len(points["pts"])])
    outs, ref = _step_points(d2, points["pts"][order])
    _assert_bitwise(outs[0], ref)


def test_lane_arrangements_bitwise(d2, points):
    """64-lane groups that take each way through the loop and the join, bit for bit the oracle's, and
    the same on a second run from the same state."""
    cls, whole = _classes(points)
    dev, cont = points["dev"], points["cont"]
    early = cls["early"]
    w = np.flatnonzero(whole)
    ei = np.flatnonzero(early)
    assert len(w) >= 64 and len(ei) >= 64
    short = ei[cont[ei] < R]            # continuation over before pass R
    long_ = ei[cont[ei] >= R + 8]       # ... well after it
    assert len(short) and len(long_)
    side = []
    for k in (E, E + R - 1, E + R):
        at = np.flatnonzero(~whole & (dev == k))
        assert len(at), k
        side.append(at[0])

    def group(special):
        special = np.asarray(special, int)
        return np.concatenate([special, w[:64 - len(special)]])

    groups = [
        group([]),                                   # no early lane: the riders alone hold the loop for R passes
        group(short[:3]),                            # the early lanes are done before pass R
        group([long_[np.argmax(cont[long_])], short[0]]),  # ... and well after pass R
        group(side),                                 # first deviations at E, E + R - 1, E + R side by side
        ei[:64],                                     # every lane early: no rider
    ]
    order = np.concatenate(groups)
    g = [order[64 * k:64 * k + 64] for k in range(5)]
    assert whole[g[0]].all()
    assert early[g[1]].sum() == 3 and cont[g[1]][early[g[1]]].max() < R and whole[g[1]].sum() == 61
    assert cont[g[2]][early[g[2]]].max() >= R + 8 and whole[g[2]].sum() == 62
    assert {E, E + R - 1, E + R} <= set(dev[g[3]][~whole[g[3]]]) and whole[g[3]].sum() == 61
    assert early[g[4]].all()
    n = _n_envs()
    rest = np.arange(n - len(order)) % len(points["pts"])
    pts = points["pts"][np.concatenate([order, rest])]
    outs, ref = _step_points(d2, pts)
    _assert_bitwise(outs[0], ref)
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_teacher_forced(d2):
    """30 steps of U(-1, 1) actions with auto-reset against the oracle, teacher-forced every step, at
    parity_util's tolerances; obs 19..22 bit for bit."""
    n = _n_envs()
    venv, orc = make_pair(d2, n, ["corridor"], seed=77, kwargs=_cfgkw())
    assert venv.group_layout() is None
    seen = {}
    gpu_step = venv.step

    def step(act):  # compare_step's GPU step, its observation kept for the bitwise check
        out = gpu_step(act)
        seen["obs"] = out[0]
        return out

    venv.step = step
    rng = np.random.default_rng(3)
    for t in range(30):
        compare_step(venv, orc, rng.uniform(-1, 1, (n, 2)).astype(np.float32))
        np.testing.assert_array_equal(seen["obs"].cpu().numpy()[:, 19:23], orc.obs[:, 19:23])
    venv.close()
