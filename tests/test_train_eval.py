"""Evaluating while training (``ppo.Evaluation``, ``PPO.learn(evaluation=...)``) on the CPU: the oracle
backend as training and eval batch through ``venv_factory``, and a scripted stub batch where the test
is about which score wins.  The schedule, ``evaluations.npz``, the metrics, SB3's strict ``>`` and the
NaN rule, the protocol-mismatch and multi-rank refusals, the logs, and that the training side is left
alone."""
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle_backend import OracleVecBackend

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 16, 8            # training envs, rollout length: 128 timesteps per update
PER = N * T
SCN = ("corridor", "parallel")
RUNS = 8


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _eval_kw():
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, n_steps=60)  # time-up within 61 steps


class RewindableOracle(OracleVecBackend):
    """The oracle batch with the ``get_state`` / ``set_state`` an eval batch needs."""

    def get_state(self):
        return self.orc.get_state()

    def set_state(self, st, ist):
        self.orc.set_state(st, ist)


def _factory(made=None):
    def make(num_envs, env_scenario, seed, **kw):
        be = RewindableOracle(num_envs, seed=seed, env_scenario=env_scenario, **kw)
        if made is not None:
            made.append(be)
        return be

    return make


def _algo(seed=0):
    from drone2d_amd.ppo import PPO, PPOConfig

    be = OracleVecBackend(N, seed=3, **_train_kw(scenario="corridor"))
    return PPO(be, PPOConfig(n_steps=T, batch_size=64, n_epochs=1), seed=seed, device="cpu"), be


def _evaluation(**over):
    from drone2d_amd.ppo import Evaluation

    kw = dict(eval_freq=PER, scenarios=SCN, runs=RUNS, seed=5, env_kwargs=_eval_kw(), venv_factory=_factory())
    kw.update(over)
    return Evaluation(**kw)


class ScriptedBatch:
    """A batch whose every episode ends at its first step; evaluation k (the k-th reset) returns
    ``rewards[k]`` for every env and succeeds on the first ``round(successes[k] * n)`` envs."""

    def __init__(self, num_envs, rewards, successes):
        self.num_envs, self.device = int(num_envs), torch.device("cpu")
        self.kwargs = {"n_steps": 4, "screensize_x": 1300, "screensize_y": 1300}
        self.scenarios = [SimpleNamespace(circles=[])]
        self.cfg = SimpleNamespace(env_id_base=0)
        self.rewards, self.successes, self.k = rewards, successes, -1

    def reset(self, seed=None, mask=None):
        self.k += 1
        return torch.zeros(self.num_envs, 27)

    def step(self, actions):
        from drone2d_amd import abi

        n = self.num_envs
        info = torch.zeros(n, abi.INFO_DIM)
        info[:, abi.INFO_STEPS] = 1
        info[:, abi.INFO_TOTREW] = self.rewards[self.k]
        info[:, abi.INFO_CAUSE] = abi.END_TIMEUP
        info[:round(self.successes[self.k] * n), abi.INFO_CAUSE] = abi.END_REACH
        done = torch.ones(n, dtype=torch.bool)
        return torch.zeros(n, 27), torch.zeros(n), done, torch.zeros(n, dtype=torch.bool), info

    @property
    def terminal_obs(self):
        return torch.zeros(self.num_envs, 27)

    def get_state(self):
        return None, None

    def set_state(self, st, ist):
        pass

    def close(self):
        pass


def _scripted(rewards, successes=None):
    successes = successes if successes is not None else [0.0] * len(rewards)
    return lambda num_envs, env_scenario, seed, **kw: ScriptedBatch(num_envs, rewards, successes)


def _best_step(path):
    from drone2d_amd.agent_io import read_agent

    return int(read_agent(os.path.join(path, "best_model.zip"))[0]["num_timesteps"])


@pytest.fixture(scope="module")
def run(d2, tmp_path_factory):
    """One 6-update run with an ``eval_freq`` that is no multiple of the rollout size, a logger and a
    checkpoint; shared, never modified."""
    from drone2d_amd.ppo import Checkpoint
    from drone2d_amd.trainlog import ScalarLog

    d = tmp_path_factory.mktemp("run")
    algo, be = _algo()
    made = []
    ev = _evaluation(eval_freq=300, log_path=str(d / "logs"), best_model_save_path=str(d / "best"),
                     venv_factory=_factory(made))
    with ScalarLog(str(d / "logs")) as logger:
        hist = algo.learn(6 * PER, evaluation=ev, logger=logger, checkpoint=Checkpoint(300, str(d / "ck")))
        paths = (logger.csv_path, logger.event_path)
    algo.close_evaluation()
    be.close()
    return SimpleNamespace(dir=d, hist=hist, made=made, params=[p.detach().clone() for p in algo.policy.parameters()],
                           csv=paths[0], events=paths[1])


def test_schedule_follows_crossings_of_eval_freq(run):
    """eval_freq 300 over updates of 128 timesteps: 384 crosses 300, 640 crosses 600; 768 crosses nothing."""
    got = [h["timesteps"] for h in run.hist if "eval/mean_reward" in h]
    assert [h["timesteps"] for h in run.hist] == [PER * k for k in range(1, 7)]
    assert got == [384, 640]
    assert len(run.made) == 1  # one eval batch for the whole learn call
    assert sorted(os.listdir(run.dir / "ck")) == ["rl_model_384_steps.zip", "rl_model_640_steps.zip"]
    for h in run.hist:
        assert ("eval/seconds" in h) == (h["timesteps"] in got)


def test_record_keys(run):
    h = next(h for h in run.hist if "eval/mean_reward" in h)
    want = {"eval/mean_reward", "eval/mean_ep_length", "eval/success_rate", "eval/collision_rate", "eval/average_ape",
            "eval/seconds", "eval/best"} | {f"eval/{s}/{k}" for s in SCN for k in ("success_rate", "mean_reward")}
    assert {k for k in h if k.startswith("eval/")} == want
    assert h["eval/seconds"] > 0 and 1 <= h["eval/mean_ep_length"] <= 61
    assert 0.0 <= h["eval/success_rate"] <= 1.0
    bests = [h["eval/best"] for h in run.hist if "eval/best" in h]
    means = [h["eval/mean_reward"] for h in run.hist if "eval/best" in h]
    assert bests == [means[0], max(means)]


def test_npz_keys_shapes_dtypes(run):
    f = np.load(run.dir / "logs" / "evaluations.npz")
    n = len(SCN) * RUNS
    assert set(f.files) == {"timesteps", "results", "ep_lengths", "successes", "collisions", "scenarios", "metric",
                            "metric_name"}
    assert f["timesteps"].tolist() == [384, 640] and f["timesteps"].dtype == np.int64
    for k, dt in (("results", np.float64), ("ep_lengths", np.int64), ("successes", np.bool_), ("collisions", np.int64)):
        assert f[k].shape == (2, n) and f[k].dtype == dt, k
    assert f["scenarios"].tolist() == list(SCN) and str(f["metric_name"]) == "mean_reward"
    assert f["metric"].shape == (2,) and f["metric"].dtype == np.float64
    ev = [h for h in run.hist if "eval/mean_reward" in h]
    for e, h in enumerate(ev):
        assert f["metric"][e] == h["eval/mean_reward"] == float(np.mean(f["results"][e]))
        assert h["eval/mean_ep_length"] == float(np.mean(f["ep_lengths"][e]))
        assert h["eval/success_rate"] == float(np.mean(f["successes"][e]))
        assert h["eval/corridor/success_rate"] == float(np.mean(f["successes"][e][:RUNS]))
        assert h["eval/parallel/mean_reward"] == float(np.mean(f["results"][e][RUNS:]))
    assert np.all(f["ep_lengths"] >= 1) and np.all(f["ep_lengths"] <= 61)


def test_npz_row_is_an_evaluation_of_that_checkpoint(run):
    """Row e == a fresh evaluation, on a fresh batch, of the checkpoint saved at that step."""
    from drone2d_amd import harness
    from drone2d_amd.evaluate import as_mlp_actor, sweep_layout
    from drone2d_amd.ppo import ActorCritic
    from drone2d_amd.train_eval import episode_arrays

    f = np.load(run.dir / "logs" / "evaluations.npz")
    es = sweep_layout(1, len(SCN), RUNS)[1]
    for e, step in enumerate((384, 640)):
        ac = ActorCritic.from_sb3_zip(str(run.dir / "ck" / f"rl_model_{step}_steps.zip"))
        be = OracleVecBackend(len(es), seed=5, env_scenario=es, **dict(_eval_kw(), scenario=list(SCN)))
        raw = harness.run_first_episodes(be, as_mlp_actor(ac), deterministic=True, seed=5, records=False)
        be.close()
        ref = episode_arrays(raw["finished"], raw["rows"])
        for k, v in ref.items():
            np.testing.assert_array_equal(f[k][e], v, err_msg=k)


def test_best_model_is_the_better_checkpoint(run):
    from drone2d_amd.agent_io import read_agent

    f = np.load(run.dir / "logs" / "evaluations.npz")
    step = 640 if f["metric"][1] > f["metric"][0] else 384
    best = read_agent(str(run.dir / "best" / "best_model.zip"))
    ck = read_agent(str(run.dir / "ck" / f"rl_model_{step}_steps.zip"))
    assert best[0]["num_timesteps"] == step
    for k, v in ck[1]["policy.pth"].items():
        assert torch.equal(best[1]["policy.pth"][k], v), k


def test_logs_carry_eval_columns(run):
    from test_monitor import _read_events

    from drone2d_amd import trainlog

    rows = trainlog.read_progress(run.csv)
    assert len(rows) == 6
    for row in rows:
        has = {k for k in row if k.startswith("eval/")}
        assert bool(has) == (row["step"] in (384, 640)), row["step"]  # empty cells elsewhere
        if has:
            assert {"eval/mean_reward", "eval/best", "eval/corridor/success_rate"} <= has
    header = open(run.csv).readline()
    assert "eval/mean_reward" in header and "eval/parallel/mean_reward" in header
    events = _read_events(run.events, trainlog.masked_crc)
    tagged = [step for step, vals in events[1:] if "eval/mean_reward" in vals]
    assert tagged == [384, 640]
    h = next(h for h in run.hist if h["timesteps"] == 384)
    vals = dict(events[1:])[384]
    assert vals["eval/success_rate"] == np.float32(h["eval/success_rate"])


def test_training_is_left_alone_and_none_writes_what_it_did(d2, run, tmp_path):
    """The same run with ``evaluation=None``: the same parameters, bit for bit; records without ``eval/``
    keys; the files of a run with a logger and a checkpoint and nothing else."""
    from drone2d_amd.ppo import Checkpoint
    from drone2d_amd.trainlog import ScalarLog

    algo, be = _algo()
    with ScalarLog(str(tmp_path / "logs")) as logger:
        hist = algo.learn(6 * PER, evaluation=None, logger=logger, checkpoint=Checkpoint(300, str(tmp_path / "ck")))
    be.close()
    for a, b in zip(algo.policy.parameters(), run.params):
        assert torch.equal(a.detach(), b)
    assert algo._ev_run is None
    timing = {"rollout_s", "train_s", "env_steps_per_s"}
    for h, g in zip(hist, run.hist):
        assert not any(k.startswith("eval/") for k in h)
        assert set(h) == {k for k in g if not k.startswith("eval/")}
        for k in set(h) - timing:
            assert h[k] == g[k] or (math.isnan(h[k]) and math.isnan(g[k])), k
    assert sorted(os.listdir(tmp_path)) == ["ck", "logs"]
    assert sorted(os.listdir(tmp_path / "ck")) == ["rl_model_384_steps.zip", "rl_model_640_steps.zip"]
    logs = sorted(os.listdir(tmp_path / "logs"))
    assert len(logs) == 2 and logs[1] == "progress.csv" and logs[0].startswith("events.out.tfevents.")
    assert "eval/" not in open(tmp_path / "logs" / "progress.csv").read()


def test_strict_greater_and_nan_never_wins(d2, tmp_path):
    """Scores 1, 1, NaN, 2, 1.5: saved at the first, not at the tie, not at the NaN, at the 2, not after."""
    scores = [1.0, 1.0, float("nan"), 2.0, 1.5]
    algo, be = _algo()
    ev = _evaluation(venv_factory=_scripted(scores), best_model_save_path=str(tmp_path), log_path=str(tmp_path))
    saved, bests = [], []
    for u in range(5):
        h = algo.learn((u + 1) * PER, evaluation=ev)[-1]  # one learn call per update: the run is kept
        saved.append(_best_step(str(tmp_path)))
        bests.append(h["eval/best"])
        assert h["eval/mean_reward"] == scores[u] or (u == 2 and math.isnan(h["eval/mean_reward"]))
    be.close()
    assert saved == [PER, PER, PER, 4 * PER, 4 * PER]
    assert bests == [1.0, 1.0, 1.0, 2.0, 2.0]
    m = np.load(tmp_path / "evaluations.npz")["metric"]
    assert m[[0, 1, 3, 4]].tolist() == [1.0, 1.0, 2.0, 1.5] and math.isnan(m[2])


def test_metric_selects_what_best_means(d2, tmp_path):
    rewards, succ = [1.0, 2.0], [0.5, 0.25]
    steps = {}
    for metric in ("mean_reward", "success_rate"):
        algo, be = _algo()
        d = str(tmp_path / metric)
        hist = algo.learn(2 * PER, evaluation=_evaluation(venv_factory=_scripted(rewards, succ), metric=metric,
                                                          best_model_save_path=d))
        be.close()
        steps[metric] = _best_step(d)
        assert [h["eval/success_rate"] for h in hist] == succ and [h["eval/mean_reward"] for h in hist] == rewards
        assert hist[-1]["eval/best"] == (2.0 if metric == "mean_reward" else 0.5)
    assert steps == {"mean_reward": 2 * PER, "success_rate": PER}
    with pytest.raises(ValueError):
        _algo()[0].learn(PER, evaluation=_evaluation(metric="median_reward"))


def test_resumed_file_is_continued_and_best_restored(d2, tmp_path):
    """A second ``learn`` with a new ``Evaluation`` of the same protocol continues the file and does not
    replace a better ``best_model.zip``; another protocol raises."""
    d = str(tmp_path)
    algo, be = _algo()
    algo.learn(2 * PER, evaluation=_evaluation(venv_factory=_scripted([3.0, 1.0]), log_path=d, best_model_save_path=d))
    assert _best_step(d) == PER
    h = algo.learn(4 * PER, evaluation=_evaluation(venv_factory=_scripted([2.0, 2.5]), log_path=d,
                                                   best_model_save_path=d))
    assert _best_step(d) == PER and [x["eval/best"] for x in h] == [3.0, 3.0]
    f = np.load(os.path.join(d, "evaluations.npz"))
    assert f["timesteps"].tolist() == [PER * k for k in (1, 2, 3, 4)] and f["metric"].tolist() == [3.0, 1.0, 2.0, 2.5]
    for other in (dict(runs=RUNS + 1), dict(scenarios=("corridor", "large")), dict(metric="success_rate")):
        with pytest.raises(ValueError, match="protocol"):
            algo.learn(5 * PER, evaluation=_evaluation(venv_factory=_scripted([0.0]), log_path=d, **other))
    assert algo.num_timesteps == 4 * PER  # refused before anything ran
    be.close()


def test_refusals(d2):
    from drone2d_amd.ppo import Evaluation

    algo, be = _algo()
    algo.world = 2  # a faked world size
    with pytest.raises(ValueError, match="more than one rank"):
        algo.learn(PER, evaluation=_evaluation())
    algo.world = 1
    with pytest.raises(ValueError, match="static scenarios"):
        algo.learn(PER, evaluation=_evaluation(scenarios=("corridor", "stage_2")))
    with pytest.raises(ValueError, match="venv_factory"):  # the default eval batch is a HIP one
        algo.learn(PER, evaluation=Evaluation(PER, scenarios=SCN, runs=2))
    assert algo.num_timesteps == PER  # (the last refusal came at the first evaluation, after one update)
    be.close()
    assert Evaluation(1).deterministic is True and Evaluation(1).runs == 16 and Evaluation(1).graph is None


def test_graph_argument_is_refused_off_the_device(d2):
    from drone2d_amd import evaluate
    from drone2d_amd.ppo import ActorCritic

    be = OracleVecBackend(4, seed=1, **dict(_eval_kw(), scenario="corridor"))
    with pytest.raises(ValueError, match="HIP"):
        evaluate.evaluate_policy(be, ActorCritic(), graph=True)
    with pytest.raises(ValueError, match="HIP"):
        evaluate.evaluate_policies(be, [ActorCritic()], np.zeros(4, np.int32), graph=True)
    with pytest.raises(ValueError, match="HIP"):
        evaluate.EvalLoop(be, ActorCritic())
    be.close()
    assert {"d2d_eval_seq_version", "d2d_eval_step_seq"} <= set(evaluate.SIGNATURES) and evaluate.SEQ_VERSION == 1


def test_command_line_lists_the_flags():
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train_ppo.py"), "--help"], capture_output=True,
                         text=True, check=True).stdout
    for flag in ("--eval-freq", "--eval-runs", "--eval-scenarios", "--eval-metric"):
        assert flag in out, flag
