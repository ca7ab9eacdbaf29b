"""The step kernels against the oracle on user scenarios at the ABI's limits -- needs an MI355X.

3-, 4-, 5-, 15- and 16-waypoint paths from 0.017 px to 64 000 px long with 0..5, 63 and 64 circles
(tests/limit_scenarios.py; tests/test_limit_scenarios.py proves on the CPU that these scenarios, points and
rollouts reach the code they are meant for: every knot interval, marches that outlive and undercut the
recorded golden-march table, the last circle of a full table, every slot of a small uniform set):

1. one scenario staged in LDS, one test per pairing, teacher-forced with auto-reset;
2. a ragged grouped map over eight of them;
3. the pool path (tables read per lane from global memory) after d2d_refresh_pool with the limit scenarios;
4. the closest-point search from crafted points on all eleven paths, one step, bit for bit, at the
   small-batch launch and with more workgroups than CUs;
5. the reset cache on two of them with 3-step episodes;
6. refused uploads, after which the handle steps on in parity.

Tolerances are parity_util's.
"""
import numpy as np
import pytest
import torch

import limit_scenarios as ls
from parity_util import OBS_ATOL, compare_step, make_pair

pytestmark = pytest.mark.gpu


def _cfgkw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _teacher_forced(d2, tag):
    scns, n, es, seed, over, steps = ls.rollouts()[tag]
    venv, orc = make_pair(d2, n, scns, seed=seed, kwargs=_cfgkw(**over), env_scenario=es)
    act = ls.actions(tag, n, steps)
    dones, worst = 0, 0.0
    for t in range(steps):
        worst = max(worst, compare_step(venv, orc, act[t]))
        dones += int(orc.term.sum())
    print(tag, "episodes finished", dones, "max |obs diff| %.3g" % worst)
    return venv, dones


@pytest.mark.parametrize("pairing", ls.PAIRINGS, ids=lambda p: "%s-%d-%s" % p)
def test_single_scenario_staged(d2, pairing):
    """One scenario, 448 envs = 7 workgroups (the three-way re-check), 120 steps with auto-reset."""
    venv, dones = _teacher_forced(d2, "single/%s-%d-%s" % pairing)
    assert venv.group_layout() is None and venv.num_envs == 448
    assert dones > 50
    venv.close()


def test_grouped_map(d2):
    """1 001 envs on a ragged map over eight limit scenarios: one with 3 envs, one with none, groups that
    straddle two scenarios."""
    venv, dones = _teacher_forced(d2, "grouped")
    _, gs = venv.group_layout()
    assert (gs < -1).any()  # a group straddling two scenarios
    assert dones > 50
    venv.close()


def test_pool_path(d2):
    """A curriculum-pool handle whose pool d2d_refresh_pool replaces by the limit scenarios, 3-waypoint paths
    included: lanes of one wave read tables of different n_wps and n_circles from global memory."""
    import oracle
    from drone2d_amd import abi
    from drone2d_amd.config import make_cfg

    kw, n = ls.pool_kwargs(), ls.N_POOL
    venv = d2.Drone2dVecEnv(n, seed=ls.POOL_SEED, **kw)
    assert venv.cfg.scn_pool == 1 and len(venv.scenarios) == ls.POOL
    cfg = make_cfg(dict(kw))
    cfg.scn_pool = 1
    orc = oracle.OracleBatch(cfg, [s.to_c() for s in venv.scenarios], n, env_scenario=venv.env_scenario)
    np.testing.assert_allclose(venv.reset().cpu().numpy(), orc.reset(ls.POOL_SEED), rtol=0, atol=OBS_ATOL)
    act = ls.actions("pool", n, ls.POOL_STEPS_BEFORE + ls.POOL_STEPS_AFTER)
    for t in range(ls.POOL_STEPS_BEFORE):
        compare_step(venv, orc, act[t])
    pool = [s.to_c() for s in ls.pool_scenarios()]
    venv._check(venv._lib.d2d_refresh_pool(venv._h, (abi.D2DScn * len(pool))(*pool), len(pool)), "d2d_refresh_pool")
    assert orc.refresh_pool(pool) == 0
    resets, worst, seen = 0, 0.0, set()
    for t in range(ls.POOL_STEPS_BEFORE, len(act)):
        worst = max(worst, compare_step(venv, orc, act[t]))
        resets += int(orc.term.sum())
        es = venv.get_env_scenarios().cpu().numpy()
        np.testing.assert_array_equal(es, orc.get_env_scenarios())
        seen |= set(es[es >= ls.POOL].tolist())
    print("pool: resets after the refresh", resets, "entries drawn", len(seen), "max |obs diff| %.3g" % worst)
    assert resets >= 200 and len(seen) == ls.POOL
    venv.close()


@pytest.mark.parametrize("many", [False, True], ids=["per512", "over_cus"])
def test_closest_point_bitwise(d2, many):
    """All eleven paths, one step from the crafted points (limit_scenarios.grid_points: behind the start,
    beyond the end, inside every knot interval, a grid, near the path): obs 19..22 and the path error bit
    for bit the oracle's.  per = 512: 88 workgroups, the speculative small-batch launch; otherwise more
    workgroups than the device has CUs, the launch without the re-check variants' idle waves."""
    from drone2d_amd import abi

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    per = 64 * (n_cu // len(ls.PATHS) + 1) if many else 512
    per = max(per, 512)
    n = per * len(ls.PATHS)
    assert (n // 64 > n_cu) == many
    scns = [ls.scenario(name) for name in ls.PATHS]
    venv, orc = make_pair(d2, n, scns, seed=5, kwargs=_cfgkw(), env_scenario=np.repeat(np.arange(len(scns)), per),
                          auto_reset=False)
    pts = np.concatenate([ls.grid_points(name, per) for name in ls.PATHS])
    st, ist = ls.states_at(pts)
    venv.set_state(torch.as_tensor(st), torch.as_tensor(ist))
    orc.set_state(st, ist)
    act = np.zeros((n, 2), np.float32)
    obs = venv.step(torch.as_tensor(act, device=venv.device))[0].cpu().numpy()
    o_obs = orc.step(act, nthreads=8)[0]
    err = venv.get_state()[0].cpu().numpy()[abi.S_PATH_ERR]
    o_err = orc.get_state()[0][abi.S_PATH_ERR]
    bad = np.flatnonzero((obs[:, 19:23] != o_obs[:, 19:23]).any(axis=1) | (err != o_err))
    print("per", per, "envs", n, "mismatching envs", len(bad), [ls.PATHS[k] for k in np.unique(bad // per)],
          "max |obs diff| %.3g" % float(np.max(np.abs(obs - o_obs))))
    np.testing.assert_array_equal(obs[:, 19:23], o_obs[:, 19:23])
    np.testing.assert_array_equal(err, o_err)
    np.testing.assert_allclose(obs, o_obs, rtol=0, atol=OBS_ATOL)
    venv.close()


@pytest.mark.parametrize("pairing", ls.RESET_CACHE_PAIRINGS, ids=lambda p: "%s-%d-%s" % p)
def test_reset_cache_short_episodes(d2, pairing):
    """3-step episodes: cached and synchronous reset observations both occur."""
    venv, dones = _teacher_forced(d2, "cache/%s-%d-%s" % pairing)
    assert dones >= 9 * venv.num_envs
    venv.close()


def test_refusals_leave_handle_usable(d2):
    """d2d_set_scenarios refuses 2 and 17 waypoints, 65 circles and a last-segment window that reaches back
    past us[n_wps-3], each with D2D_E_ARG and its message; the handle keeps its scenario and steps on."""
    from drone2d_amd import abi
    from drone2d_amd._native import NativeError, check

    tag = "single/%s-%d-%s" % ls.PAIRINGS[4]
    scns, n, es, seed, over, steps = ls.rollouts()[tag]
    venv, orc = make_pair(d2, n, scns, seed=seed, kwargs=_cfgkw(**over))
    act = ls.actions(tag, n, steps)
    for t in range(10):
        compare_step(venv, orc, act[t])

    def bad(**kw):
        c = ls.scenario("w16_zig", 64, "uniform").to_c()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    window = ls.scenario("w5_zig", 4, "uniform").to_c()
    window.us[window.n_wps - 3] = window.us[window.n_wps - 2] - 0.001
    cases = [(bad(n_wps=2), r"n_wps out of range \[3, D2D_MAX_WPS\]"),
             (bad(n_wps=abi.MAX_WPS + 1), r"n_wps out of range \[3, D2D_MAX_WPS\]"),
             (bad(n_circles=abi.MAX_CIRCLES + 1), r"n_circles out of range \[0, D2D_MAX_CIRCLES\]"),
             (window, r"us\[n_wps-2\] - us\[n_wps-3\] must exceed 0.001")]
    for k, (c, msg) in enumerate(cases):
        rc = venv._lib.d2d_set_scenarios(venv._h, (abi.D2DScn * 1)(c), 1, None)
        assert rc == 1  # D2D_E_ARG
        with pytest.raises(NativeError, match=msg):
            check(rc, "d2d_set_scenarios", venv._lib)
        for t in range(10 + 5 * k, 15 + 5 * k):
            compare_step(venv, orc, act[t])
    venv.close()
