"""K1's early start of the Brent continuation (bt_finish_join) -- needs an MI355X.

At full load the path wave re-checks only steps [1, E) of the golden-march table, resumes the lanes
that deviate there at once, and the lanes that deviate in the other wave's part [E, len) join the
running loop.  That code runs only when there are more workgroups than CUs, so every test here uses
one scenario, the env-ordered layout and 64 x (CU count + 1) envs.

1. crafted points, one step, bitwise against the oracle, every class of lane present;
2. crafted 64-lane groups (no join / dry loop before the join / E - 1, E, E + 1 side by side / join
   after the early loop has ended / all early), bitwise, and the same twice: the moment of the join
   depends on timing, the result must not;
3. teacher-forced runs with auto-reset against the oracle.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

from parity_util import OBS_ATOL, compare_step, make_pair

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

E = 16          # BT_EARLY (csrc/d2d_device.h; test_constant_matches_kernel)
SPLIT = 22      # the split by halves the early start replaces: max(4, (42 + 3) // 2)


def _cfgkw(scenario="corridor", **over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, scenario=scenario, **over)


def _n_envs():
    return 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)


def test_constant_matches_kernel():
    import drone2d_amd

    hdr = os.path.join(os.path.dirname(drone2d_amd.__file__), "csrc", "d2d_device.h")
    m = re.search(r"^#define D2D_BT_EARLY (\d+)$", open(hdr).read(), re.M)
    assert m and int(m.group(1)) == E


@pytest.fixture(scope="module")
def points(d2):
    """The crafted points on corridor, classified on the CPU by the scipy restatement of
    tools/brent_lanes.py: pts [m, 2], kind, dev, cont (continuation steps), kind_len."""
    import brent_lanes as bl
    import oracle
    from drone2d_amd.env import build_scenarios

    scn = build_scenarios(_cfgkw())[0]
    sc = scn.to_c()
    L = float(scn.path.length)
    rng = np.random.default_rng(11)
    g = np.linspace(-600.0, 1900.0, 64)
    grid = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    u = rng.uniform(-10.0, L + 10.0, 2048)
    near = np.array([scn.path(x) for x in u]) + rng.normal(0.0, 40.0, (len(u), 2))
    fans = []
    for ue in (-10.0, L + 10.0):  # the extrapolated ends, where the table marches converge
        p0 = np.array(oracle.path_eval(sc, ue))
        tg = np.array(oracle.path_eval(sc, ue + 1e-3)) - np.array(oracle.path_eval(sc, ue - 1e-3))
        tg /= np.hypot(*tg)
        nm = np.array([-tg[1], tg[0]])
        a, b = np.meshgrid(np.linspace(-300.0, 300.0, 41), np.linspace(-0.5, 0.5, 21))
        fans.append(p0 + a.reshape(-1, 1) * nm + b.reshape(-1, 1) * tg)
    pts = np.concatenate([grid, near, *fans])
    kind_len = [bl.forced_len(L, 0), bl.forced_len(L, 1)]
    cls = np.array([bl.classify(sc, L, kind_len, x, y) for x, y in pts])
    return dict(pts=pts, kind=cls[:, 0], dev=cls[:, 1], cont=cls[:, 2], kind_len=kind_len)


def _classes(P):
    kind, dev, cont = P["kind"], P["dev"], P["cont"]
    whole = dev == np.array(P["kind_len"])[kind]
    return {"whole0": whole & (kind == 0), "whole1": whole & (kind == 1), "early": ~whole & (dev < E),
            "mid": ~whole & (dev >= E) & (dev < SPLIT), "late": ~whole & (dev >= SPLIT)}, whole, cont


def _step_points(d2, pts):
    """One step of n corridor envs placed at pts (at rest, zero action: the searches run from pts):
    the GPU's (obs, path error) twice from the same state, and the oracle's."""
    from drone2d_amd import abi

    n = len(pts)
    venv, orc = make_pair(d2, n, ["corridor"], seed=5, kwargs=_cfgkw(), auto_reset=False)
    assert venv.group_layout() is None  # env-ordered: the ungrouped kernel
    st = np.zeros((abi.NSTATE, n))
    st[0], st[1] = pts[:, 0], pts[:, 1]
    st[6], st[7] = pts[:, 0] - 40.0, pts[:, 1]
    st[12], st[13] = pts[:, 0] + 40.0, pts[:, 1]
    ist = np.zeros((abi.NISTATE, n), np.int32)
    act = np.zeros((n, 2), np.float32)
    outs = []
    for _ in range(2):
        venv.set_state(torch.as_tensor(st), torch.as_tensor(ist))
        obs = venv.step(torch.as_tensor(act, device=venv.device))[0].cpu().numpy()
        outs.append((obs, venv.get_state()[0].cpu().numpy()[abi.S_PATH_ERR]))
    orc.set_state(st, ist)
    o_obs = orc.step(act)[0].copy()
    o_err = orc.get_state()[0][abi.S_PATH_ERR].copy()
    venv.close()
    return outs, (o_obs, o_err)


def _assert_bitwise(out, ref):
    (obs, err), (o_obs, o_err) = out, ref
    np.testing.assert_array_equal(obs[:, 19:23], o_obs[:, 19:23])
    np.testing.assert_array_equal(err, o_err)
    np.testing.assert_allclose(obs, o_obs, rtol=0, atol=OBS_ATOL)


def test_crafted_points_bitwise(d2, points):
    """Every class of lane -- whole table followed (both kinds), first deviation below E, in [E, 22)
    (today's first half), at 22 or later -- in one step, bit for bit the oracle's closest and
    lookahead points and path error."""
    cls, _, _ = _classes(points)
    for name, m in cls.items():
        print(name, int(m.sum()))
        assert m.any(), name
    n = _n_envs()
    pts = points["pts"][np.arange(n) % len(points["pts"])]
    outs, ref = _step_points(d2, pts)
    _assert_bitwise(outs[0], ref)


def test_lane_arrangements_bitwise(d2, points):
    """64-lane groups that take each way through the join, bit for bit the oracle's, and the same
    on a second run from the same state."""
    cls, whole, cont = _classes(points)
    dev = points["dev"]
    ix = {k: np.flatnonzero(v) for k, v in cls.items()}
    w = np.flatnonzero(whole)
    latecomers = np.flatnonzero(~whole & (dev >= E))
    for k in (E - 1, E, E + 1):
        assert (~whole & (dev == k)).any(), k
    assert len(w) >= 64 and len(ix["early"]) >= 64 and len(latecomers)

    def group(special):
        return np.concatenate([special, w[:64 - len(special)]])

    short_early = ix["early"][np.argmin(cont[ix["early"]])]
    long_late = latecomers[np.argmax(cont[latecomers])]
    groups = [
        group(np.array([], int)),                                       # no continuation, no join
        group(latecomers[:1]),                                          # the loop is dry before the join
        group(np.array([np.flatnonzero(~whole & (dev == k))[0] for k in (E - 1, E, E + 1)])),
        group(np.array([short_early, long_late])),                      # the join after the early loop ended
        ix["early"][:64],                                               # every lane deviates early
    ]
    order = np.concatenate(groups)
    early = ~whole & (dev < E)
    g = [order[64 * k:64 * k + 64] for k in range(5)]
    assert whole[g[0]].all()
    assert whole[g[1]].sum() == 63 and (dev[g[1]][~whole[g[1]]] >= E).all()
    assert {E - 1, E, E + 1} <= set(dev[g[2]][~whole[g[2]]])
    assert early[g[3]].sum() == 1 and (~whole[g[3]] & ~early[g[3]]).sum() == 1
    assert cont[g[3]][early[g[3]]][0] == cont[early].min() and cont[g[3]].max() == cont[latecomers].max()
    assert early[g[4]].all()
    n = _n_envs()
    rest = np.arange(n - len(order)) % len(points["pts"])
    pts = points["pts"][np.concatenate([order, rest])]
    outs, ref = _step_points(d2, pts)
    _assert_bitwise(outs[0], ref)
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("scn", ["corridor", "S_corridor"])
def test_teacher_forced(d2, scn):
    """40 steps of U(-1, 1) actions with auto-reset against the oracle, teacher-forced every step,
    within test_vs_oracle_teacher_forced's tolerances (parity_util); obs 19..22 bit for bit."""
    n = _n_envs()
    venv, orc = make_pair(d2, n, [scn], seed=99, kwargs=_cfgkw())
    assert venv.group_layout() is None
    seen = {}
    gpu_step = venv.step

    def step(act):  # compare_step's GPU step, its observation kept for the bitwise check
        out = gpu_step(act)
        seen["obs"] = out[0]
        return out

    venv.step = step
    rng = np.random.default_rng(1)
    for t in range(40):
        compare_step(venv, orc, rng.uniform(-1, 1, (n, 2)).astype(np.float32))
        np.testing.assert_array_equal(seen["obs"].cpu().numpy()[:, 19:23], orc.obs[:, 19:23])
    venv.close()
