"""``PPO.learn(evaluation=...)`` on an MI355X: the schedule, every row of ``evaluations.npz`` and the
record's ``eval/*`` against ``evaluate.sweep`` of that step's checkpoint, ``best_model.zip``, the training
side left alone, and a resumed run continuing the file -- with the update and the evaluation both
eager and both replayed as HIP graphs."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N, T, UPDATES = 1024, 8, 4
PER = N * T
SCN = ("corridor", "parallel")
RUNS, SEED = 8, 3


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _cfg(graph):
    from drone2d_amd.ppo import PPOConfig

    cfg = PPOConfig.gpu_defaults(n_steps=T, batch_size=2048, n_epochs=2)
    cfg.graph = graph
    return cfg


def _evaluation(d, graph):
    from drone2d_amd.ppo import Evaluation

    return Evaluation(eval_freq=2 * PER, scenarios=SCN, runs=RUNS, seed=SEED, graph=graph, log_path=str(d / "logs"),
                      best_model_save_path=str(d / "best"))


def _state(algo):
    torch.cuda.synchronize()
    return {k: v.detach().clone() if isinstance(v, torch.Tensor) else v
            for k, v in dict(algo.policy.state_dict(), **algo._stepper.state()).items()}


def _learn(d2, d, graph, evaluate=True, updates=UPDATES):
    from drone2d_amd.ppo import PPO, Checkpoint

    venv = d2.Drone2dVecEnv(N, seed=1, **_train_kw(scenario="corridor"))
    algo = PPO(venv, _cfg(graph), seed=0)
    hist = algo.learn(updates * PER, evaluation=_evaluation(d, graph) if evaluate else None,
                      checkpoint=Checkpoint(2 * PER, str(d / "ck")))
    state = _state(algo)
    captures = algo._ev_run.loop.captures if evaluate else None
    algo.close_evaluation()
    venv.close()
    return hist, state, captures


@pytest.fixture(scope="module", params=[False, True], ids=["eager", "graphs"])
def run(d2, request, tmp_path_factory):
    """One 4-update run with an evaluation every 2 updates and the checkpoints of the same steps, and the
    sweeps of those checkpoints computed afterwards; shared, never modified."""
    from drone2d_amd import evaluate

    graph = request.param
    d = tmp_path_factory.mktemp("graphs" if graph else "eager")
    hist, state, captures = _learn(d2, d, graph)
    sweeps = {}
    for step in (2 * PER, 4 * PER):
        bank = evaluate.PolicyBank([str(d / "ck" / f"rl_model_{step}_steps.zip")])
        sweeps[step] = evaluate.sweep(bank, SCN, RUNS, seed=SEED, deterministic=True)[bank.names[0]]
    return SimpleNamespace(dir=d, graph=graph, hist=hist, state=state, sweeps=sweeps, captures=captures)


def test_evaluations_follow_the_schedule(run):
    assert [h["timesteps"] for h in run.hist] == [PER * k for k in range(1, UPDATES + 1)]
    assert [h["timesteps"] for h in run.hist if "eval/mean_reward" in h] == [2 * PER, 4 * PER]
    assert sorted(os.listdir(run.dir / "ck")) == sorted(f"rl_model_{s}_steps.zip" for s in (2 * PER, 4 * PER))
    assert run.captures == (1 if run.graph else 0)  # one captured segment served both evaluations


def test_npz_rows_equal_a_sweep_of_that_checkpoint(run):
    f = np.load(run.dir / "logs" / "evaluations.npz")
    assert f["timesteps"].tolist() == [2 * PER, 4 * PER] and f["scenarios"].tolist() == list(SCN)
    for e, step in enumerate((2 * PER, 4 * PER)):
        for s, name in enumerate(SCN):
            m, sl = run.sweeps[step][name], slice(s * RUNS, (s + 1) * RUNS)
            assert m["unfinished"] == 0
            np.testing.assert_array_equal(f["results"][e][sl], m["rewards"], err_msg=name)
            np.testing.assert_array_equal(f["ep_lengths"][e][sl], m["time_spent"], err_msg=name)
            np.testing.assert_array_equal(f["collisions"][e][sl], m["collisions"], err_msg=name)
            assert int(f["successes"][e][sl].sum()) == m["successes"]
        assert len(set(f["ep_lengths"][e].tolist())) > 1  # not one episode flown sixteen times


def test_record_equals_the_summary_of_that_sweep(run):
    from drone2d_amd import harness

    f = np.load(run.dir / "logs" / "evaluations.npz")
    best = None
    for e, step in enumerate((2 * PER, 4 * PER)):
        h = next(h for h in run.hist if h["timesteps"] == step)
        parts = [run.sweeps[step][name] for name in SCN]
        whole = {k: sum(p[k] for p in parts) for k in ("successes", "fails")}
        whole.update({k: np.concatenate([p[k] for p in parts]) for k in ("collisions", "apes", "time_spent", "rewards")})
        s = harness.summary(whole)
        assert h["eval/mean_reward"] == float(np.mean(whole["rewards"])) == f["metric"][e]
        assert h["eval/mean_ep_length"] == s["Average flight time"]
        assert h["eval/success_rate"] == s["Success rate"] and h["eval/collision_rate"] == s["Collision rate"]
        assert h["eval/average_ape"] == s["Average APE"]
        for name, p in zip(SCN, parts):
            assert h[f"eval/{name}/success_rate"] == harness.summary(p)["Success rate"]
            assert h[f"eval/{name}/mean_reward"] == float(np.mean(p["rewards"]))
        best = h["eval/mean_reward"] if best is None or h["eval/mean_reward"] > best else best
        assert h["eval/best"] == best and h["eval/seconds"] > 0


def test_best_model_is_the_checkpoint_with_the_greater_metric(run):
    from drone2d_amd.agent_io import read_agent

    m = np.load(run.dir / "logs" / "evaluations.npz")["metric"]
    step = 4 * PER if m[1] > m[0] else 2 * PER  # strictly greater: the first stays on a tie
    best = read_agent(str(run.dir / "best" / "best_model.zip"))
    ck = read_agent(str(run.dir / "ck" / f"rl_model_{step}_steps.zip"))
    assert best[0]["num_timesteps"] == step
    assert set(best[1]["policy.pth"]) == set(ck[1]["policy.pth"])
    for k, v in ck[1]["policy.pth"].items():
        assert torch.equal(best[1]["policy.pth"][k], v), k


def test_training_is_the_run_without_evaluation(d2, run, tmp_path):
    """Parameters, Adam moments and step counter after 4 updates, with and without the evaluations, at
    test_resume_on_hip_matches_uninterrupted_run's bound (rtol 1e-4 / atol 1e-5)."""
    hist, state, _ = _learn(d2, tmp_path, run.graph, evaluate=False)
    assert not any(k.startswith("eval/") for h in hist for k in h)
    assert not os.path.exists(tmp_path / "logs") and not os.path.exists(tmp_path / "best")
    assert set(state) == set(run.state)
    bitwise = True
    for k, v in state.items():
        if isinstance(v, torch.Tensor):
            torch.testing.assert_close(v, run.state[k], rtol=1e-4, atol=1e-5, msg=k)
            bitwise = bitwise and torch.equal(v, run.state[k])
        else:
            assert v == run.state[k], k
    print(f"with / without evaluation ({'graphs' if run.graph else 'eager'}): bitwise equal = {bitwise}")


def test_resumed_run_continues_the_file(d2, run, tmp_path):
    """2 updates, then ``PPO.load`` of that step's checkpoint into a new batch and 2 more under a new
    ``Evaluation`` of the same protocol: the file is continued (its first row kept bit for bit, the
    uninterrupted run's timesteps), and ``best_model.zip`` is replaced only by a strictly better score."""
    from drone2d_amd.agent_io import read_agent
    from drone2d_amd.ppo import PPO, Checkpoint

    _learn(d2, tmp_path, run.graph, updates=2)
    npz = tmp_path / "logs" / "evaluations.npz"
    first = {k: v.copy() for k, v in np.load(npz).items()}
    assert first["timesteps"].tolist() == [2 * PER]
    assert read_agent(str(tmp_path / "best" / "best_model.zip"))[0]["num_timesteps"] == 2 * PER
    venv = d2.Drone2dVecEnv(N, seed=1, **_train_kw(scenario="corridor"))
    algo = PPO.load(str(tmp_path / "ck" / f"rl_model_{2 * PER}_steps.zip"), venv)
    hist = algo.learn(UPDATES * PER, evaluation=_evaluation(tmp_path, run.graph),
                      checkpoint=Checkpoint(2 * PER, str(tmp_path / "ck")))
    algo.close_evaluation()
    venv.close()
    f = np.load(npz)
    whole = np.load(run.dir / "logs" / "evaluations.npz")
    assert set(f.files) == set(whole.files) and f["timesteps"].tolist() == whole["timesteps"].tolist()
    for k in ("results", "ep_lengths", "successes", "collisions", "metric"):
        assert f[k].shape == whole[k].shape and f[k].dtype == whole[k].dtype
        np.testing.assert_array_equal(f[k][0], first[k][0], err_msg=k)
    m = f["metric"]
    assert hist[-1]["eval/best"] == max(m[0], m[1])  # the best before the resume was restored from the file
    step = 4 * PER if m[1] > m[0] else 2 * PER
    assert read_agent(str(tmp_path / "best" / "best_model.zip"))[0]["num_timesteps"] == step
