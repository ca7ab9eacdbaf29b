"""libd2d_disturb.so on an MI355X: both calls against ``disturb.HostDisturber`` (bit for bit from the same
draws; the Philox uniforms exactly and the normals within the bound the eval library's noise is held to),
shard invariance, and the disturbed closed loops of ``evaluate_policy``, ``EvalLoop`` and ``sweep``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bank_util import make_policies

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BASE, STEPS, SEED = 130, 1000, 20, 0xDEADBEEF12345678
ODD = 77  # the env given a level outside the table
# the bound tests/test_gpu_eval.py::test_philox_noise_matches_host holds the eval library's normals to: r <= 5.9
# times the float32 rounding of 2 pi u1 (<= 4e-7) and a few ulp of cosf / logf is under 1e-5
NORMAL_ATOL = 2e-5


def _test_kw(**over):
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, **over)


def _levels():
    from drone2d_amd.disturb import Disturbance

    return [Disturbance(),
            Disturbance(obs_sigma=0.05, act_sigma=0.1, sensor_dropout=0.3, motor_gain=(0.7, 1.0), act_delay=8),
            Disturbance(obs_sigma=0.2, sensor_dropout=0.5, motor_gain=(1.0, 0.5), act_delay=3)]


def _level_map(n=N):
    lv = (np.arange(n) % 3).astype(np.int32)
    lv[ODD] = 7
    return lv


def _inputs(t, n=N):
    """Step t's observation and action rows (float32, with -0.0, inf and NaN rows among them) and draws."""
    rng = np.random.default_rng(100 + t)
    obs = rng.standard_normal((n, 27)).astype(np.float32)
    act = rng.uniform(-1.2, 1.2, (n, 2)).astype(np.float32)
    obs[3 * (t % 5)] = -0.0
    obs[3 * (t % 5) + 1, ::3] = np.inf
    obs[3 * (t % 5) + 2, 1::3] = np.nan
    act[t % 7] = -0.0
    z_obs = rng.standard_normal((n, 27)).astype(np.float32)
    u = rng.random((n, 3)).astype(np.float32)
    z_act = rng.standard_normal((n, 2)).astype(np.float32)
    return obs, act, z_obs, u, z_act


def _eq(dev: torch.Tensor, host: np.ndarray) -> bool:
    return torch.equal(dev.cpu().contiguous().view(torch.int32), torch.from_numpy(np.ascontiguousarray(host)).view(torch.int32))


@pytest.fixture(scope="module")
def policies(d2):
    return make_policies()


@pytest.mark.parametrize("channels", [None, (0, 1, 6, 9, 13, 26)])
def test_given_draws_bit_for_bit(d2, channels):
    """20 steps of both calls from supplied draws equal the NumPy twin on the uint32 views: outputs, history
    and returned draws, over levels mixing every stage beside an all-neutral one; the env without a level
    is untouched."""
    from drone2d_amd import disturb as D

    kw = dict(env_id_base=BASE, seed=SEED, obs_channels=channels, noise="given", keep_draws=True)
    dev = D.Disturber(N, _levels(), _level_map(), device="cuda", **kw)
    host = D.HostDisturber(N, _levels(), _level_map(), **kw)
    changed = 0
    for t in range(STEPS):
        obs, act, z_obs, u, z_act = _inputs(t)
        obs_d, act_d = torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda()
        out = dev.obs(obs_d, t, z=torch.from_numpy(z_obs).cuda(), u=torch.from_numpy(u).cuda())
        want = host.obs(obs, t, z=z_obs, u=u)
        assert _eq(out, want), t
        assert _eq(obs_d, obs)  # the input is not modified
        assert _eq(dev.z_obs, host.z_obs) and _eq(dev.u_drop, host.u_drop), t
        assert _eq(out[ODD], obs[ODD]) and _eq(out[0::3][:25], obs[0::3][:25])  # no level; the neutral level
        assert dev.act(act_d, t, z=torch.from_numpy(z_act).cuda()) is act_d
        a = act.copy()
        host.act(a, t, z=z_act)
        assert _eq(act_d, a), t
        assert _eq(dev.hist, host.hist) and _eq(dev.z_act, host.z_act), t
        assert _eq(act_d[ODD], act[ODD]) and _eq(act_d[0::3][:25], act[0::3][:25])
        changed += int((a != act).any(1).sum())
    assert changed > STEPS * 80  # the two disturbed levels did move their rows
    assert float(dev.hist[:, ODD].abs().max()) == 0.0


def test_philox_draws(d2):
    """Mode 2: the returned uniforms are the twin's exactly, the returned normals are the float64 Box-Muller of
    the same uniforms within the eval library's bound, and from the device's own draws everything downstream
    is the twin's bit for bit (every dropout decision among it)."""
    from drone2d_amd import disturb as D

    levels, lv = _levels(), _level_map()
    kw = dict(env_id_base=BASE, seed=SEED)
    dev = D.Disturber(N, levels, lv, device="cuda", keep_draws=True, **kw)
    twin = D.HostDisturber(N, levels, lv, keep_draws=True, **kw)
    given = D.HostDisturber(N, levels, lv, noise="given", **kw)
    g = np.arange(BASE, BASE + N)
    table = np.stack([d.row() for d in levels])[np.where(lv < 3, lv, 0)]
    has = lv < 3
    worst, dropped = 0.0, 0

    def bm64(w, k):
        u0, u1 = D.uniforms(w[k]).astype(np.float64), D.uniforms(w[k + 1]).astype(np.float64)
        r, a = np.sqrt(-2.0 * np.log(u0)), 2.0 * np.pi * u1
        return r * np.cos(a), r * np.sin(a)

    for t in range(STEPS):
        obs, act, *_ = _inputs(t)
        out = dev.obs(torch.from_numpy(obs).cuda(), t)
        z_dev, u_dev = dev.z_obs.cpu().numpy(), dev.u_drop.cpu().numpy()
        twin.obs(obs, t)
        assert np.array_equal(u_dev.view(np.uint32), twin.u_drop.view(np.uint32)), t
        assert np.array_equal(u_dev != 0, np.repeat((has & (table[:, 2] != 0))[:, None], 3, 1))
        z64 = np.zeros((N, 28))
        for b in range(7):
            w = D.philox_words(SEED, g, t, D.TAG_OBS, b)
            z64[:, 4 * b], z64[:, 4 * b + 1] = bm64(w, 0)
            z64[:, 4 * b + 2], z64[:, 4 * b + 3] = bm64(w, 2)
        on = has & (table[:, 0] != 0)
        z64 = np.where(on[:, None], z64[:, :27], 0.0)
        worst = max(worst, float(np.abs(z_dev - z64).max()))
        assert (z_dev[on] != 0).all() and (z_dev[~on] == 0).all()
        want = given.obs(obs, t, z=z_dev, u=u_dev)
        assert _eq(out, want), t
        dropped += int((want[:, 8:17:3] == 1).sum())
        act_d = torch.from_numpy(act).cuda()
        dev.act(act_d, t)
        za = dev.z_act.cpu().numpy()
        a64 = np.stack(bm64(D.philox_words(SEED, g, t, D.TAG_ACT, 0), 0), -1)
        on = has & (table[:, 1] != 0)
        worst = max(worst, float(np.abs(za - np.where(on[:, None], a64, 0.0)).max()))
        a = act.copy()
        given.act(a, t, z=za)
        assert _eq(act_d, a) and _eq(dev.hist, given.hist), t
    print(f"philox normals: max |device - float64 Box-Muller| {worst:.3g} (bound {NORMAL_ATOL})")
    assert worst <= NORMAL_ATOL
    assert dropped > 100


def test_shards_give_the_rows_of_the_whole(d2):
    from drone2d_amd import disturb as D

    levels, lv = _levels(), _level_map()
    whole = D.Disturber(N, levels, lv, device="cuda", env_id_base=BASE, seed=SEED)
    parts = [D.Disturber(65, levels, lv[:65], device="cuda", env_id_base=BASE, seed=SEED),
             D.Disturber(65, levels, lv[65:], device="cuda", env_id_base=BASE + 65, seed=SEED)]
    other = D.Disturber(N, levels, lv, device="cuda", env_id_base=BASE + 1, seed=SEED)
    for t in range(12):
        obs, act, *_ = _inputs(t)
        obs, act = torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda()
        o = whole.obs(obs, t).clone()
        a = whole.act(act.clone(), t)
        os_ = torch.cat([p.obs(obs[k * 65:(k + 1) * 65].contiguous(), t) for k, p in enumerate(parts)])
        as_ = torch.cat([p.act(act[k * 65:(k + 1) * 65].clone(), t) for k, p in enumerate(parts)])
        assert torch.equal(o.view(torch.int32), os_.view(torch.int32)), t
        assert torch.equal(a.view(torch.int32), as_.view(torch.int32)), t
        assert not torch.equal(o.view(torch.int32), other.obs(obs, t).view(torch.int32))


def test_contradictory_arguments_launch_nothing(d2):
    from drone2d_amd import disturb as D

    dev = D.Disturber(N, _levels(), _level_map(), device="cuda", env_id_base=BASE, seed=SEED)
    obs, act, *_ = _inputs(0)
    obs, act = torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda()
    out = dev.obs(obs, 0).clone()
    dev.act(act, 0)
    torch.cuda.synchronize()
    before = (dev.obs_out.clone(), act.clone(), dev.hist.clone())
    base = D.D2DDisturbArgs.from_buffer_copy(dev._args)
    for field, value in (("n", 0), ("t", -1), ("n_levels", 0), ("noise_mode", 3), ("noise_mode", 1), ("env_id_base", -1), ("env_id_base", 2 ** 32 - N + 1), ("params", None), ("env_level", None)):
        b = D.D2DDisturbArgs.from_buffer_copy(base)
        setattr(b, field, value)
        assert dev._lib.d2d_disturb_obs(C.byref(b), None) == 1, field
        assert dev._lib.d2d_disturb_act(C.byref(b), None) == 1, field
    for field, value in (("obs_in", None), ("obs_out", None), ("obs_out", base.obs_in), ("obs_mask", 1 << 27)):
        b = D.D2DDisturbArgs.from_buffer_copy(base)
        setattr(b, field, value)
        assert dev._lib.d2d_disturb_obs(C.byref(b), None) == 1, field
    for field, value in (("act", None), ("hist", None), ("act", base.act + 4)):
        b = D.D2DDisturbArgs.from_buffer_copy(base)
        setattr(b, field, value)
        assert dev._lib.d2d_disturb_act(C.byref(b), None) == 1, field
    assert dev._lib.d2d_disturb_obs(None, None) == 1 and dev._lib.d2d_disturb_act(None, None) == 1
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), before[0].view(torch.int32))
    for now, was in zip((dev.obs_out, act, dev.hist), before):
        assert torch.equal(now.view(torch.int32), was.view(torch.int32))
    with pytest.raises(ValueError):
        dev.obs(obs[:100].contiguous(), 0)
    with pytest.raises(ValueError):
        dev.act(act.double(), 0)
    with pytest.raises(ValueError):
        dev.obs(obs, 0, z=obs)  # draws are taken with noise="given" only


# ------------------------------------------------------------------------------------------- the closed loops
def _same(m, ref):
    assert set(m) == set(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            assert m[k].dtype == v.dtype and m[k].shape == v.shape, k
            assert np.array_equal(np.ascontiguousarray(m[k]).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k
        else:
            assert m[k] == v, k


def _corridor(d2, n, seed, **kw):
    return d2.Drone2dVecEnv(n, seed=seed, with_info=True, **_test_kw(scenario="corridor"), **kw)


def test_neutral_evaluation_is_the_plain_one(d2, policies):
    """The split record / act sequence against the fused call: 256 corridor envs, every key bit for bit."""
    from drone2d_amd import evaluate
    from drone2d_amd.disturb import Disturbance

    res = []
    for disturb in (None, Disturbance()):
        venv = _corridor(d2, 256, 11)
        res.append(evaluate.evaluate_policy(venv, policies["shipped"], seed=11, flight_paths=True, keep_actions=True,
                                            disturb=disturb))
        venv.close()
    assert res[0]["unfinished"] == 0 and res[0]["successes"] > 0
    _same(res[1], res[0])


def test_recorder_sees_the_true_flight(d2, policies):
    """obs_sigma = 0.05: the recorded positions are the env's own obs[:, 6:8] of every step and ``actions`` are
    what reached ``venv.step``, against the same seeds stepped by hand with ``Disturber`` + ``evaluate.act``."""
    from drone2d_amd import evaluate
    from drone2d_amd.disturb import Disturbance, Disturber

    n, seed, pol = 96, 4, policies["shipped"]
    level = Disturbance(obs_sigma=0.05, act_sigma=0.05, act_delay=1)
    venv = _corridor(d2, n, seed, env_id_offset=640)
    m = evaluate.evaluate_policy(venv, pol, seed=seed, flight_paths=True, keep_actions=True, disturb=level)
    venv.close()
    assert m["unfinished"] == 0
    T = m["actions"].shape[0]
    assert T >= int(m["time_spent"].max())
    venv = _corridor(d2, n, seed, env_id_offset=640)
    d = Disturber(n, level, device=venv.device, env_id_base=640, seed=seed)
    obs = venv.reset(seed=seed)
    xy = np.full((T, n, 2), np.nan, np.float32)
    first = np.full(n, -1)
    applied, seen = [], []
    for t in range(T):
        seen_t = d.obs(obs, t)
        if t < 3:
            seen.append(bool(torch.equal(seen_t, obs)))
        a = evaluate.act(pol, seen_t, seed=seed, t=t, env_id_base=640)
        d.act(a, t)
        applied.append(a.clone())
        obs, _, term, trunc, _ = venv.step(a)
        done = (term | trunc).bool()
        pos = torch.where(done[:, None], venv.terminal_obs[:, 6:8], obs[:, 6:8]).cpu().numpy()
        live = first < 0
        xy[t, live] = pos[live]
        first[live & done.cpu().numpy()] = t
    venv.close()
    assert seen == [False] * 3  # the policy did not see the truth
    assert np.array_equal(m["actions"].view(np.uint32), torch.stack(applied).cpu().numpy().view(np.uint32))
    assert np.array_equal(m["time_spent"], first + 1)
    w, h = m["screen"]
    steps = int(m["time_spent"].max())
    tr = xy[:steps].astype(np.float64)
    want = np.stack([(tr[..., 0] + 1.0) * w / 2.0, h - (tr[..., 1] + 1.0) * h / 2.0], -1)
    np.testing.assert_array_equal(m["flight_xy"], want)
    # and the eager EvalLoop flies the same, run after run
    venv = _corridor(d2, n, seed, env_id_offset=640)
    loop = evaluate.EvalLoop(venv, pol, graph=False, flight_paths=True, disturb=level)
    for _ in range(2):
        fin, rows, pos, nobs, *_ = loop.run(seed)
        _same(evaluate._records(venv, fin, rows, pos, nobs), {k: v for k, v in m.items() if k != "actions"})
    venv.close()


P, S, L, R = 2, 2, 3, 32
SCN = ["corridor", "large"]


@pytest.fixture(scope="module")
def level_sweep(d2, policies):
    from drone2d_amd import evaluate
    from drone2d_amd.disturb import Disturbance

    levels = [Disturbance(), Disturbance(obs_sigma=0.05, name="noisy"),
              Disturbance(motor_gain=(0.8, 1.0), act_delay=4, sensor_dropout=0.2, name="worn")]
    bank = evaluate.PolicyBank([policies["shipped"], policies["perturbed"]], names=["shipped", "perturbed"])
    return bank, levels, evaluate.sweep(bank, SCN, R, seed=9, flight_paths=True, disturb=levels)


def test_sweep_level_axis(d2, level_sweep):
    """2 policies x 2 scenarios x 3 levels x 32 runs in one batch: a cell equals ``evaluate_policies`` on a batch
    of its 32 global env ids built by hand, and the neutral cells are the plain sweep's envs of the same ids."""
    from drone2d_amd import evaluate
    from drone2d_amd.disturb import Disturber

    bank, levels, res = level_sweep
    assert list(res) == ["shipped", "perturbed"]
    for per_scn in res.values():
        assert list(per_scn) == SCN
        for per_level in per_scn.values():
            assert list(per_level) == ["level_0", "noisy", "worn"]
            assert all(m["successes"] + m["fails"] + m["unfinished"] == R for m in per_level.values())
    ep, es, el = evaluate.sweep_layout(P, S, R, L)
    for p, s, k in ((1, 1, 2), (0, 1, 1)):
        ids = np.flatnonzero((ep == p) & (es == s) & (el == k))
        off = int(ids[0])
        assert np.array_equal(ids, np.arange(off, off + R)) and off == ((p * S + s) * L + k) * R
        venv = d2.Drone2dVecEnv(R, seed=9, with_info=True, env_scenario=np.full(R, s, np.int32), env_id_offset=off,
                                **_test_kw(scenario=SCN))
        d = Disturber(R, levels[k], device=venv.device, env_id_base=off, seed=9)
        by_hand = evaluate.evaluate_policies(venv, bank, np.full(R, p, np.int32), seed=9, flight_paths=True, disturb=d)
        venv.close()
        _same(res[bank.names[p]][SCN[s]][levels[k].name], by_hand[p])
    # the plain sweep of L R runs: cell (p, s) holds the ids of the level sweep's cell (p, s), level 0 first
    plain = evaluate.sweep(bank, SCN, L * R, seed=9)
    differs = 0
    for name in bank.names:
        for scn in SCN:
            cell, ref = res[name][scn], plain[name][scn]
            assert ref["unfinished"] == 0 and all(m["unfinished"] == 0 for m in cell.values())
            for k in ("time_spent", "rewards", "apes", "collisions"):
                assert np.array_equal(cell["level_0"][k].view(np.uint8), ref[k][:R].view(np.uint8)), (name, scn, k)
            differs += sum(not np.array_equal(cell[lv]["rewards"], ref["rewards"][j * R:(j + 1) * R])
                           for j, lv in ((1, "noisy"), (2, "worn")))
    assert differs == 2 * P * S  # the disturbed cells are other flights


def test_graph_with_disturb_is_refused(d2, policies):
    from drone2d_amd import evaluate
    from drone2d_amd.disturb import Disturbance

    venv = _corridor(d2, 8, 1)
    bank = evaluate.PolicyBank([policies["shipped"]])
    with pytest.raises(ValueError, match="graph=True with disturb"):
        evaluate.evaluate_policy(venv, policies["shipped"], graph=True, disturb=Disturbance())
    with pytest.raises(ValueError, match="graph=True with disturb"):
        evaluate.evaluate_policies(venv, bank, np.zeros(8, np.int32), graph=True, disturb=Disturbance())
    with pytest.raises(ValueError, match="graph=True with disturb"):
        evaluate.EvalLoop(venv, policies["shipped"], graph=True, disturb=Disturbance())
    with pytest.raises(ValueError, match="graph=True with disturb"):
        evaluate.sweep(bank, ["corridor"], 4, graph=True, disturb=[Disturbance()])
    venv.close()


_OFF = """
import sys
sys.path.insert(0, {repo!r})
sys.path.insert(0, {tests!r})
import drone2d_amd as d2
from drone2d_amd import evaluate
from drone2d_amd.config import ENV_TEST_CONFIG
from bank_util import make_policies
venv = d2.Drone2dVecEnv(64, seed=1, with_info=True, **dict(ENV_TEST_CONFIG, scenario="corridor"))
m = evaluate.evaluate_policy(venv, make_policies()["shipped"], seed=1, max_steps=8)
venv.close()
maps = open("/proc/self/maps").read()
print("eval", "libd2d_eval.so" in maps, "disturb", "libd2d_disturb.so" in maps, "module", "drone2d_amd.disturb" in sys.modules)
"""


def test_off_means_off(d2):
    """A plain evaluation in a fresh process neither imports the module nor loads the library."""
    r = subprocess.run([sys.executable, "-c", _OFF.format(repo=REPO, tests=os.path.join(REPO, "tests"))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "eval True disturb False module False"
