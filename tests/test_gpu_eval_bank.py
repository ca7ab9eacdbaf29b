"""The policy bank (d2d_eval_step_bank) on an MI355X: every comparison is with the single-policy path
(``evaluate.act`` / ``evaluate_policy``) and bitwise -- both sides are the same fmaf chains."""
import ctypes as C
import csv
import os

import numpy as np
import pytest
import torch

from bank_util import blocks, make_policies

pytestmark = pytest.mark.gpu
KW = dict(seed=77, t=5)


def _test_kw(**over):
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, **over)


@pytest.fixture(scope="module")
def policies(d2):
    return make_policies()


@pytest.fixture(scope="module")
def bank(d2, policies):
    from drone2d_amd import evaluate

    return evaluate.PolicyBank(list(policies.values()), names=list(policies))


@pytest.fixture(scope="module")
def obs_pool(d2):
    """As tests/test_gpu_eval.py: 1000 observation rows of a short random-action corridor rollout and
    1000 rows of 3 * randn, interleaved (so the first n rows hold both kinds); on the device, never modified."""
    venv = d2.Drone2dVecEnv(250, seed=2, **_test_kw(scenario="corridor"))
    g = torch.Generator(device="cuda").manual_seed(3)
    obs = venv.reset(seed=2)
    real = []
    for t in range(40):
        obs = venv.step(torch.rand(250, 2, device="cuda", generator=g) * 2 - 1)[0]
        if t % 10 == 9:
            real.append(obs.clone())
    real = torch.cat(real).cpu()
    venv.close()
    wide = 3.0 * torch.randn(1000, 27, generator=torch.Generator().manual_seed(4))
    return torch.stack([real, wide], 1).reshape(2000, 27).cuda()


def _mode_kw(mode, n):
    if mode == 0:
        return dict(deterministic=True)
    if mode == 1:
        return dict(noise=torch.randn(n, 2, generator=torch.Generator().manual_seed(n)).cuda())
    return {}


def _maps(n):
    last = np.zeros(n, np.int32)
    last[-1] = 2
    return {"all policy 1, two unused": np.ones(n, np.int32), "blocks of 64": blocks(n, 64),
            "blocks of 100": blocks(n, 100), "blocks of 20": blocks(n, 20), "i % 3": blocks(n, 1),
            "the last row alone": last}


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_act_bank_is_the_single_policy_act_bitwise(d2, policies, bank, obs_pool, n, mode):
    """act_bank(...)[map == p] == evaluate.act(policy p, ...)[map == p], actions and noise_out, over
    uniform chunks, chunks straddling two policies, three policies in a chunk and a policy that owns
    only the last row of the last, partial chunk; and a bank of one policy."""
    from drone2d_amd import evaluate

    obs = obs_pool[:n]
    kw = dict(KW, env_id_base=0, return_noise=True, **_mode_kw(mode, n))
    solo = [evaluate.act(ac, obs, **kw) for ac in policies.values()]
    if n > 1:
        assert not torch.equal(solo[0][0], solo[1][0]) and not torch.equal(solo[1][0], solo[2][0])
    for name, m in _maps(n).items():
        a, z = evaluate.act_bank(bank, obs, m, **kw)
        assert a.shape == (n, 2) and a.dtype == torch.float32
        for p in range(3):
            rows = torch.from_numpy(m == p).cuda()
            assert torch.equal(a[rows], solo[p][0][rows]), (name, p)
            assert torch.equal(z[rows], solo[p][1][rows]), (name, p)
    for p, ac in enumerate(policies.values()):  # P = 1
        a, z = evaluate.act_bank([ac], obs, np.zeros(n, np.int64), **kw)
        assert torch.equal(a, solo[p][0]) and torch.equal(z, solo[p][1]), p


def test_chunk_walk_past_the_grid_cap(d2, policies, bank, obs_pool):
    """65 536 + 70 rows in blocks of 4 100: more chunks than workgroups, so a workgroup takes a second
    chunk (of another policy than its first)."""
    from drone2d_amd import evaluate

    n = 65536 + 70
    obs = obs_pool.repeat((n + 1999) // 2000, 1)[:n].contiguous()
    m = blocks(n, 4100)
    a = evaluate.act_bank(bank, obs, m, **KW)
    for p, ac in enumerate(policies.values()):
        rows = torch.from_numpy(m == p).cuda()
        assert int(rows.sum()) > 20000
        assert torch.equal(a[rows], evaluate.act(ac, obs, **KW)[rows]), p


SCN7 = ["perpendicular", "parallel", "S_parallel", "corridor", "S_corridor", "large", "impossible"]
RUNS, LOOP_SEED = 24, 5
REC = ("time_spent", "rewards", "apes", "collisions")


def _loop_venv(d2, n=504, off=0, es=None):
    return d2.Drone2dVecEnv(n, seed=LOOP_SEED, with_info=True, env_scenario=es, env_id_offset=off, **_test_kw(scenario=SCN7))


@pytest.fixture(scope="module")
def closed_loop(d2, bank):
    """evaluate_policies on 3 policies x 7 test scenarios x 24 runs, computed once."""
    from drone2d_amd import evaluate

    ep, es = evaluate.sweep_layout(3, 7, RUNS)
    venv = _loop_venv(d2, es=es)
    res = evaluate.evaluate_policies(venv, bank, ep, split=es, seed=LOOP_SEED, flight_paths=True, keep_actions=True)
    venv.close()
    return ep, es, res


def test_closed_loop_flies_each_policys_own_episodes(d2, policies, closed_loop):
    """Policy p's envs in the bank's batch fly what evaluate_policy flies them under policy p alone on an
    identically built batch: records, flight paths and actions at the same env indices."""
    from drone2d_amd import evaluate

    ep, es, res = closed_loop
    assert sorted(res) == [(p, s) for p in range(3) for s in range(7)]
    for p, ac in enumerate(policies.values()):
        venv = _loop_venv(d2, es=es)
        solo = evaluate.evaluate_policy(venv, ac, seed=LOOP_SEED, flight_paths=True, keep_actions=True)
        venv.close()
        assert solo["unfinished"] == 0 and len(solo["time_spent"]) == 504  # record j is env j
        for s in range(7):
            m = res[(p, s)]
            idx = np.flatnonzero((ep == p) & (es == s))
            assert m["unfinished"] == 0 and len(idx) == RUNS == m["successes"] + m["fails"]
            for k in REC:
                np.testing.assert_array_equal(m[k], solo[k][idx], err_msg=f"{k} {p} {s}")
            T = int(m["time_spent"].max())
            assert m["flight_xy"].shape == (T, RUNS, 2)
            np.testing.assert_array_equal(m["flight_xy"], solo["flight_xy"][:T, idx])
            assert np.isnan(solo["flight_xy"][T:, idx]).all()
            steps = min(m["actions"].shape[0], solo["actions"].shape[0])
            assert steps >= T and m["actions"].shape[1:] == (RUNS, 2)
            np.testing.assert_array_equal(m["actions"][:steps], solo["actions"][:steps, idx])
    # the policies fly different episodes: the bank did not hand every env the same actor
    assert not np.array_equal(res[(0, 3)]["time_spent"], res[(1, 3)]["time_spent"])
    assert not np.array_equal(res[(1, 3)]["time_spent"], res[(2, 3)]["time_spent"])


def test_shards_of_the_map_fly_the_unsharded_episodes(d2, bank, closed_loop):
    """Two 252-env batches (env_id_offset 0 and 252), each with its slice of the map: concatenated,
    the records of every (policy, scenario) pair are the unsharded run's."""
    from drone2d_amd import evaluate

    ep, es, whole = closed_loop
    parts = []
    for off in (0, 252):
        venv = _loop_venv(d2, n=252, off=off, es=es[off:off + 252])
        parts.append(evaluate.evaluate_policies(venv, bank, ep[off:off + 252], split=es[off:off + 252], seed=LOOP_SEED,
                                                flight_paths=True))
        venv.close()
    assert set(parts[0]) | set(parts[1]) == set(whole) and set(parts[0]) & set(parts[1])  # policy 1 is split
    for key, ref in whole.items():
        ms = [p[key] for p in parts if key in p]
        assert sum(m["unfinished"] for m in ms) == 0
        assert sum(m["successes"] for m in ms) == ref["successes"] and sum(m["fails"] for m in ms) == ref["fails"]
        for k in REC:
            np.testing.assert_array_equal(np.concatenate([m[k] for m in ms]), ref[k], err_msg=f"{k} {key}")
        T = ref["flight_xy"].shape[0]
        fl = []
        for m in ms:
            f = np.full((T, m["flight_xy"].shape[1], 2), np.nan)
            f[:m["flight_xy"].shape[0]] = m["flight_xy"]
            fl.append(f)
        np.testing.assert_array_equal(np.concatenate(fl, 1), ref["flight_xy"])


def test_bank_loop_captures_into_a_graph(d2, bank):
    """16 x (d2d_eval_step_bank, d2d_step) captured and replayed == the same 16 steps issued eagerly
    (one chain, no parallel branches)."""
    from drone2d_amd import abi, evaluate

    lib = evaluate.load()
    n, T = 256, 16
    ep = torch.from_numpy(blocks(n, 100)).cuda()
    cb = bank.c_bank(ep)
    out = []
    for graph in (False, True):
        venv = d2.Drone2dVecEnv(n, seed=4, with_info=True, **_test_kw(scenario="corridor"))
        fin = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rows = torch.zeros(n, abi.INFO_DIM, device="cuda")
        rem = torch.full((1,), n, dtype=torch.int32, device="cuda")
        act_env = torch.empty(n, 2, device="cuda")
        obs0 = venv.reset(seed=4)

        def body():
            a = evaluate.D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, noise_mode=evaluate.NOISE_PHILOX, seed=4,
                                         act_env=act_env.data_ptr())
            obs = obs0
            st = torch.cuda.current_stream().cuda_stream
            for t in range(T + 1):
                a.t, a.act, a.obs = t, int(t < T), obs.data_ptr()
                evaluate._step_bank(lib, a, cb, st)
                if t == T:
                    break
                obs, _, term, trunc, info = venv.step(act_env)
                a.prev_term, a.prev_trunc, a.prev_info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
                a.finished, a.rows, a.remaining = fin.data_ptr(), rows.data_ptr(), rem.data_ptr()
            return obs

        def rewind():
            venv.reset(seed=4)
            fin.zero_()
            rows.zero_()
            rem.fill_(n)

        body()  # both arms: a first pass issued eagerly (library warm-up)
        rewind()
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                obs = body()
            g.replay()
        else:
            obs = body()
        torch.cuda.synchronize()
        out.append((obs.clone(), fin.clone(), rows.clone(), rem.clone(), act_env.clone()))
        venv.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert int(out[0][3]) == n - int(out[0][1].sum())
    assert float(out[0][4].abs().max()) <= 1.0


def test_bank_step_refuses_contradictory_arguments(d2, bank):
    """Every contradiction of include/d2d_eval.h returns hipErrorInvalidValue (1) and launches nothing:
    act_env keeps its sentinel."""
    from drone2d_amd import abi, evaluate

    lib = evaluate.load()
    n = 70
    obs = torch.zeros(n, 27, device="cuda")
    ep = torch.from_numpy(blocks(n, 20)).cuda()
    act_env = torch.full((n, 2), 7.0, device="cuda")
    noise = torch.zeros(n, 2, device="cuda")
    other = torch.zeros(64 * 64, device="cuda")
    byte = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def args(**over):
        kw = dict(n=n, t=1, info_dim=abi.INFO_DIM, act=1, noise_mode=evaluate.NOISE_PHILOX, seed=1, obs=obs.data_ptr(),
                  act_env=act_env.data_ptr())
        kw.update(over)
        return evaluate.D2DEvalStepArgs(**kw)

    def bank_rec(**over):
        kw = dict(n_policies=3, params=bank.params.data_ptr(), env_policy=ep.data_ptr())
        kw.update(over)
        return evaluate.D2DEvalBank(**kw)

    def call(a, b):
        rc = lib.d2d_eval_step_bank(C.byref(a), C.byref(b) if b is not None else None, 0)
        torch.cuda.synchronize()
        return rc

    bad = [("bank NULL", args(), None), ("P = 0", args(), bank_rec(n_policies=0)), ("P < 0", args(), bank_rec(n_policies=-1)),
           ("params NULL", args(), bank_rec(params=None)), ("env_policy NULL", args(), bank_rec(env_policy=None))]
    bad += [(f"{k} given", args(**{k: other.data_ptr()}), bank_rec())
            for k in ("w1", "b1", "w2", "b2", "w3", "b3", "log_std")]
    bad += [("n = 0", args(n=0), bank_rec()), ("t < 0", args(t=-1), bank_rec()),
            ("neither half", args(act=0), bank_rec()), ("obs NULL", args(obs=None), bank_rec()),
            ("noise mode 3", args(noise_mode=3), bank_rec()), ("noise mode -1", args(noise_mode=-1), bank_rec()),
            ("mode 1 without noise", args(noise_mode=evaluate.NOISE_GIVEN), bank_rec()),
            ("env_id_base < 0", args(env_id_base=-1), bank_rec()),
            ("ids past 2^32", args(env_id_base=2 ** 32 - n + 1), bank_rec()),
            ("half a record half", args(prev_trunc=byte.data_ptr()), bank_rec()),
            ("record half without rows", args(prev_term=byte.data_ptr(), prev_trunc=byte.data_ptr()), bank_rec())]
    for what, a, b in bad:
        assert call(a, b) == 1, what
        assert bool((act_env == 7.0).all()), what
    assert lib.d2d_eval_bank_version() == evaluate.BANK_VERSION == 1
    assert lib.d2d_eval_abi_version() == evaluate.ABI_VERSION == 1
    # the same arguments without the contradiction launch and write every row
    assert call(args(noise_mode=evaluate.NOISE_GIVEN, noise=noise.data_ptr()), bank_rec()) == 0
    assert bool((act_env.abs() <= 1.0).all())
    # record only (act == 0): the bank's pointers are not read
    act_env.fill_(7.0)
    term = torch.ones(n, dtype=torch.uint8, device="cuda")
    info = torch.arange(n * abi.INFO_DIM, dtype=torch.float32, device="cuda").reshape(n, abi.INFO_DIM)
    fin = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(n, abi.INFO_DIM, device="cuda")
    rem = torch.full((1,), n, dtype=torch.int32, device="cuda")
    a = args(act=0, obs=None, act_env=None, prev_term=term.data_ptr(), prev_trunc=byte.data_ptr(), prev_info=info.data_ptr(),
             finished=fin.data_ptr(), rows=rows.data_ptr(), remaining=rem.data_ptr())
    assert call(a, bank_rec(params=None, env_policy=None)) == 0
    assert int(rem) == 0 and bool(fin.all()) and torch.equal(rows, info) and bool((act_env == 7.0).all())


def test_sweep_returns_the_batch_split_by_agent_and_scenario(d2, policies, tmp_path):
    """sweep on 2 policies x {corridor, large} x 64 runs == evaluate_policies on the sweep_layout batch;
    write_selection: one row per pair, its rates harness.summary's."""
    from drone2d_amd import evaluate, harness

    scns = ["corridor", "large"]
    b2 = evaluate.PolicyBank([policies["shipped"], policies["perturbed"]], names=["shipped", "perturbed"])
    res = evaluate.sweep(b2, scns, 64, seed=9)
    assert list(res) == ["shipped", "perturbed"] and all(list(v) == scns for v in res.values())
    ep, es = evaluate.sweep_layout(2, 2, 64)
    venv = d2.Drone2dVecEnv(256, seed=9, with_info=True, env_scenario=es, **_test_kw(scenario=scns))
    ref = evaluate.evaluate_policies(venv, b2, ep, split=es, seed=9)
    venv.close()
    for p, name in enumerate(b2.names):
        for s, scn in enumerate(scns):
            m, r = res[name][scn], ref[(p, s)]
            assert set(m) == set(r) and m["unfinished"] == 0 and m["successes"] + m["fails"] == 64
            for k, v in r.items():
                if isinstance(v, np.ndarray):
                    np.testing.assert_array_equal(m[k], v, err_msg=k)
                else:
                    assert m[k] == v, k
    with pytest.raises(ValueError):
        evaluate.sweep(b2, ["corridor", "stage_3"], 4)
    rows = harness.write_selection(res, str(tmp_path))
    assert [r[:3] for r in rows] == [(a, s, 64) for a in b2.names for s in scns]
    with open(tmp_path / "selection.csv", newline="") as f:
        lines = list(csv.reader(f))[1:]
    assert len(lines) == 4 and os.path.exists(tmp_path / "selection.json")
    for line, r in zip(lines, rows):
        s = harness.summary(res[r[0]][r[1]])
        assert r[3:] == (s["Success rate"], s["Collision rate"], s["Average APE"], s["Average flight time"])
        assert [float(v) for v in line[3:]] == list(r[3:])
    assert rows[0][3] > rows[2][3]  # the shipped agent beats a random actor on corridor
