"""User scenarios at the ABI's limits, CPU side: the checker pinned, and the GPU tests' coverage proven.

tests/test_gpu_limit_scenarios.py runs the step kernels on 3-, 4-, 5-, 15- and 16-waypoint paths from
0.017 px to 64 000 px long with 0..5, 63 and 64 circles (tests/limit_scenarios.py).  Here, without a
device:

1. the package's QPMIPath fit of the limit paths equals the reference's (tests/golden/limits_probe.npz);
2. the oracle's path evaluation and closest-point search meet the reference's on them, under the rules
   of test_oracle_golden.py::test_path_eval_and_closest_point;
3. the coverage conditions, from the oracle and the helper alone: the points, scenarios and rollouts of
   the GPU tests do reach every knot interval, marches longer and shorter than the recorded table, the
   last circle of a full table, every slot of the small uniform sets, and enough finished episodes;
4. scenario_to_c refuses 2 and 17 waypoints and 65 circles.
"""
import functools

import numpy as np
import pytest

import limit_scenarios as ls


def _c(name):
    return ls.scenario(name).to_c()


# ---------------------------------------------------------------------------------------- the checker
@pytest.mark.parametrize("name", ls.PATHS)
def test_path_fit(d2, name):
    g, p = ls.fixture(), ls.path(name)
    np.testing.assert_array_equal(np.asarray(p.us), g[f"{name}/us"])
    np.testing.assert_array_equal(np.asarray(p.x_params), g[f"{name}/x_params"])
    np.testing.assert_array_equal(np.asarray(p.y_params), g[f"{name}/y_params"])
    n = len(g[f"{name}/wps"])
    assert n == int(name[1:name.index("_")]) and g[f"{name}/x_params"].shape == (n - 2, 3)


def test_limit_path_lengths(d2):
    """The shapes the fixture is meant to hold (ISSUE: L ~ 1 000, ~ 1, ~ 0.02, >= 6e4, >= 2e4; collinear)."""
    L = {n: float(ls.path(n).length) for n in ls.PATHS}
    assert 900 < L["w3_arc"] < 1100 and 0.9 < L["w3_tiny"] < 1.1 and 0.015 < L["w3_dust"] < 0.025
    assert L["w3_long"] >= 6e4 and L["w16_long"] >= 2e4
    for n in ("w3_tiny", "w3_dust"):
        us = ls.path(n).us
        assert us[1] - us[0] > 0.001
    pl = ls.path("w3_line")
    assert abs(pl.x_params[0][0]) < 1e-12 and abs(pl.y_params[0][0]) < 1e-12


@pytest.mark.parametrize("name", ls.PATHS)
def test_path_eval_and_closest_point(oracle_mod, d2, name):
    """As test_oracle_golden.py::test_path_eval_and_closest_point, on the limit paths: >= 99 % of the
    evaluations and closest-u results bitwise equal (the reference's u**2 is glibc pow(u, 2.0), the oracle's
    u*u), every one within 4 ulp / xtol, 1 < nf < 500."""
    scn, g = _c(name), ls.fixture()
    exact = total = 0
    for u, xy in zip(g[f"{name}/u"], g[f"{name}/xy"]):
        x, y = oracle_mod.path_eval(scn, u)
        np.testing.assert_allclose([x, y], xy, rtol=4e-16 * 4, atol=1e-12)
        exact += (x, y) == (xy[0], xy[1])
        total += 1
    L = scn.us[scn.n_wps - 1]
    for p, cu, cxy, lxy in zip(g[f"{name}/pts"], g[f"{name}/closest_u"], g[f"{name}/closest_xy"],
                               g[f"{name}/lookahead_xy"]):
        u, nf = oracle_mod.closest_u(scn, p[0], p[1])
        assert abs(u - cu) <= 1e-6, (p, u, cu)
        assert 1 < nf < 500
        ula = L if u + 220 > L else u + 220
        np.testing.assert_allclose(oracle_mod.path_eval(scn, u), cxy, atol=1e-6)
        np.testing.assert_allclose(oracle_mod.path_eval(scn, ula), lxy, atol=1e-6)
        exact += u == cu
        total += 1
    print(name, "bitwise", exact, "of", total)
    assert exact >= 0.99 * total, (exact, total)


# ------------------------------------------------------------------------------ coverage: closest point
@functools.lru_cache(maxsize=None)
def _searched(name):
    """(u, nf) of the oracle's closest-point search from every point of the GPU grid test (per = 512)."""
    import oracle

    sc = _c(name)
    return np.array([oracle.closest_u(sc, x, y) for x, y in ls.grid_points(name, 512)]).T


@pytest.mark.parametrize("name", ls.PATHS)
def test_grid_points_reach_every_interval(oracle_mod, d2, name):
    u, _ = _searched(name)
    us = np.asarray(ls.path(name).us)
    inside = (u >= us[0]) & (u <= us[-1])
    iv = np.searchsorted(us, u[inside], side="left") - 1      # u in (us[k], us[k + 1]] -> k
    assert set(range(len(us) - 1)) <= set(iv.tolist()), sorted(set(iv.tolist()))
    assert (u < us[0]).any() and (u > us[-1]).any()


def test_marches_outlive_and_undercut_the_table(oracle_mod, d2):
    K = ls.bt_k()
    u, nf = _searched("w3_long")
    m = u < -10 + 1e-5
    print("BT_K", K, "w3_long nf behind the start", sorted(set(nf[m].astype(int))), "all", nf.min(), nf.max())
    assert (m & (nf >= K + 3)).sum() >= 8
    u, nf = _searched("w16_long")
    print("w16_long nf", nf.min(), nf.max())
    assert (nf >= K + 3).sum() >= 8
    for name in ("w3_tiny", "w3_dust"):
        u, nf = _searched(name)
        print(name, "nf", nf.min(), nf.max())
        assert (nf <= 40).sum() >= 8


# ------------------------------------------------------------------------------------ coverage: rollouts
def _run(scns, n, es, seed, over, steps, tag, keep_states=False):
    orc = ls.oracle_batch(scns, n, es, over)
    obs0 = orc.reset(seed)
    act = ls.actions(tag, n, steps)
    terms, xy = [], [orc.get_state()[0][:2].copy()] if keep_states else []
    for t in range(steps):
        terms.append(orc.step(act[t], nthreads=4)[2])
        if keep_states:
            xy.append(orc.get_state()[0][:2].copy())
    orc.close()
    return obs0, np.array(terms), xy


@functools.lru_cache(maxsize=None)
def _rollout(tag):
    return _run(*ls.rollouts()[tag], tag, keep_states=True)


@pytest.mark.parametrize("tag", sorted(ls.rollouts()))
def test_rollouts_finish_episodes(oracle_mod, d2, tag):
    n = ls.rollouts()[tag][1]
    dones = int(_rollout(tag)[1].sum())
    print(tag, "episodes finished", dones)
    assert dones >= (9 * n if tag.startswith("cache/") else 50)


def test_pool_rollout_finishes_episodes(oracle_mod, d2):
    """The pool run of the GPU test in the oracle alone: after the refresh at least 200 resets draw from the
    limit scenarios (indices in the second pool half), among them scenarios of every waypoint count."""
    import oracle
    from drone2d_amd.config import make_cfg
    from drone2d_amd.env import build_scenarios

    kw = ls.pool_kwargs()
    cfg = make_cfg(dict(kw))
    cfg.scn_pool = 1
    n = ls.N_POOL
    orc = oracle.OracleBatch(cfg, [s.to_c() for s in build_scenarios(kw)], n, env_scenario=np.arange(n) % ls.POOL)
    orc.reset(ls.POOL_SEED)
    act = ls.actions("pool", n, ls.POOL_STEPS_BEFORE + ls.POOL_STEPS_AFTER)
    for t in range(ls.POOL_STEPS_BEFORE):
        orc.step(act[t], nthreads=4)
    pool = ls.pool_scenarios()
    assert min(len(s.path.us) for s in pool) == 3 and max(len(s.path.us) for s in pool) == 16
    assert orc.refresh_pool([s.to_c() for s in pool]) == 0
    resets, seen = 0, set()
    for t in range(ls.POOL_STEPS_BEFORE, len(act)):
        resets += int(orc.step(act[t], nthreads=4)[2].sum())
        es = orc.get_env_scenarios()
        seen |= set(es[es >= ls.POOL].tolist())
    print("resets after the refresh", resets, "pool entries drawn", len(seen))
    assert resets >= 200 and len(seen) == ls.POOL
    orc.close()


def _edge_distances(scn, xy):
    """[n_envs, n_circles]: get_obstacle_distances -- min over the frame's unrotated corners (+-50, +-5)."""
    c = scn.circles
    d = [np.hypot(xy[0][:, None] + vx - c[None, :, 0], xy[1][:, None] + vy - c[None, :, 1])
         for vx, vy in ((50.0, -5.0), (50.0, 5.0), (-50.0, 5.0), (-50.0, -5.0))]
    return np.min(d, axis=0) - c[None, :, 2]


@pytest.mark.parametrize("pairing", [p for p in ls.PAIRINGS if p[1] in (2, 3, 4) and p[2] == "uniform"],
                         ids=lambda p: "%s-%d-%s" % p)
def test_small_uniform_sets_fill_every_slot(oracle_mod, d2, pairing):
    """Every circle index is the nearest, the second and (from 3 circles on) the third for some env over the
    run -- sensor_pos' top-4 shortcut with empty slots sees every arrangement."""
    scn = ls.scenario(*pairing)
    count = pairing[1]
    seen = np.zeros((min(3, count), count), bool)
    for xy in _rollout("single/%s-%d-%s" % pairing)[2]:
        order = np.argsort(_edge_distances(scn, xy), axis=1, kind="stable")
        for rank in range(seen.shape[0]):
            seen[rank, np.unique(order[:, rank])] = True
    assert seen.all(), seen


@pytest.mark.parametrize("pairing", [p for p in ls.PAIRINGS if p[1] >= 63], ids=lambda p: "%s-%d-%s" % p)
def test_last_circle_decides(oracle_mod, d2, pairing):
    """Full and nearly full circle tables: without the last circle the same run senses other circles at
    reset in >= 10 % of the envs and ends different episodes."""
    tag = "single/%s-%d-%s" % pairing
    scns, n, es, seed, over, steps = ls.rollouts()[tag]
    obs0, term, _ = _rollout(tag)
    cut = ls.scenario(*pairing, drop_last=True)
    assert len(cut.circles) == pairing[1] - 1 and np.array_equal(cut.circles, scns[0].circles[:-1])
    obs0_c, term_c, _ = _run([cut], n, es, seed, over, steps, tag)
    differ = (obs0[:, 8:17] != obs0_c[:, 8:17]).any(axis=1).mean()
    print(tag, "reset obs[8:17] differ in %.1f %% of the envs" % (100 * differ),
          "term differs in", int((term != term_c).sum()), "env-steps")
    assert differ >= 0.10
    assert (term != term_c).any()


# --------------------------------------------------------------------------------------------- refusals
def test_scenario_to_c_refusals(d2):
    from drone2d_amd.scenarios import QPMIPath, Scenario, scenario_to_c

    def scn(n_wps, n_circles):
        wps = np.array([[100.0 + 60.0 * i, 500.0 + 40.0 * (i % 2)] for i in range(n_wps)])
        circ = np.array([[300.0 + 10.0 * k, 400.0, 20.0] for k in range(n_circles)]).reshape(-1, 3)
        return Scenario("x", wps, QPMIPath(wps), circ, (50.0, 150.0, 400.0, 600.0))

    for nw, nc in ((3, 0), (16, 64)):
        c = scenario_to_c(scn(nw, nc))
        assert (c.n_wps, c.n_circles) == (nw, nc)
    with pytest.raises(ValueError, match="2 waypoints"):
        scenario_to_c(scn(2, 0))
    with pytest.raises(ValueError, match="17 waypoints"):
        scenario_to_c(scn(17, 0))
    with pytest.raises(ValueError, match="65 circles"):
        scenario_to_c(scn(4, 65))
