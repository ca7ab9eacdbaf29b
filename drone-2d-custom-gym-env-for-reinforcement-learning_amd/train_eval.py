"""In-training evaluation: what ``PPO.learn(evaluation=...)`` runs (``ppo.Evaluation`` is SB3's
``EvalCallback``).  ``EvaluationRun`` joins the parts that exist -- ``evaluate.sweep_layout`` (the
mixed-scenario batch), ``evaluate.EvalLoop`` (the closed test loop, replayable), ``harness.summary``,
``PPO.save`` -- and keeps ``evaluations.npz`` and ``best_model.zip``.

The eval batch is a second env batch of its own, built at the first evaluation and kept with its
``EvalLoop`` for the whole ``learn`` call; nothing of the training side (the training batch, the
rollout noise generator, the shuffle counter, ``_predict_t``, PPO's graphs) is touched.
"""
from __future__ import annotations

import math
import os
import time

import numpy as np

# Evaluation.graph=None on a one-rank HIP run: replay the eval loop as a captured graph only if that
# measured faster than the eager loop at 896 envs (DESIGN.md "The replayed loop": the replayed arm's
# median below the eager arm's minimum over 5 rounds; profiles/eval/eval_graph_probe.json).
GRAPH_PAYS = False

NPZ_NAME = "evaluations.npz"
METRICS = ("mean_reward", "success_rate")


def scenario_names(scenarios) -> list:
    """The names of an ``Evaluation``'s scenarios, refusing what ``evaluate.sweep`` refuses."""
    from .config import CURRICULUM_STAGES

    scenarios = [scenarios] if isinstance(scenarios, str) else list(scenarios)
    if not scenarios or any(isinstance(s, str) and s in CURRICULUM_STAGES for s in scenarios):
        raise ValueError("Evaluation takes static scenarios (names or Scenario objects), at least one")
    names = [s if isinstance(s, str) else s.name for s in scenarios]
    if len(set(names)) != len(names):
        raise ValueError("Evaluation: scenario names must be unique")
    return names


def episode_arrays(fin, rows) -> dict:
    """Per-env arrays, in env order, of the recorder's output: ``results`` (the episode return, NaN for
    an env that did not finish), ``ep_lengths`` (0 then), ``successes`` and ``collisions``."""
    from .env import info_dicts

    n = len(fin)
    out = {"results": np.full(n, np.nan, np.float64), "ep_lengths": np.zeros(n, np.int64),
           "successes": np.zeros(n, bool), "collisions": np.zeros(n, np.int64)}
    for i in np.flatnonzero(fin):
        d = info_dicts(rows[i])
        out["results"][i], out["ep_lengths"][i] = d["total_reward"], d["env_steps"]
        out["successes"][i], out["collisions"][i] = d["n_successful_runs"] == 1, d["n_collisions"]
    return out


def eval_scalars(venv, fin, rows, nobs, env_scenario, names) -> dict:
    """The ``eval/*`` entries of a record (without ``eval/seconds`` and ``eval/best``): the numbers of
    ``harness.summary`` over the whole batch and per scenario."""
    from . import harness
    from .evaluate import _records

    def mean(x):
        return float(np.mean(x)) if len(x) else float("nan")

    m = _records(venv, fin, rows, None, nobs)
    s = harness.summary(m)
    out = {"eval/mean_reward": mean(m["rewards"]), "eval/mean_ep_length": s["Average flight time"],
           "eval/success_rate": s["Success rate"], "eval/collision_rate": s["Collision rate"],
           "eval/average_ape": s["Average APE"]}
    for k, name in enumerate(names):
        idx = np.flatnonzero(env_scenario == k)
        mk = _records(venv, fin[idx], rows[idx], None, nobs)
        out[f"eval/{name}/success_rate"] = harness.summary(mk)["Success rate"]
        out[f"eval/{name}/mean_reward"] = mean(mk["rewards"])
    return out


class EvaluationRun:
    """One ``learn`` call's evaluation state: the eval batch and its loop (built at the first
    evaluation), the arrays of ``evaluations.npz`` and the best metric so far."""

    def __init__(self, ev, algo):
        if ev.eval_freq < 1 or ev.runs < 1:
            raise ValueError("Evaluation: eval_freq and runs must be at least 1")
        if ev.metric not in METRICS:
            raise ValueError(f"Evaluation.metric must be one of {METRICS}")
        self.ev = ev
        self.names = scenario_names(ev.scenarios)
        self.n = len(self.names) * int(ev.runs)
        self.venv = self.loop = self._snap = None
        self.best = None  # the best metric so far (None: no evaluation with a number yet)
        self.data = {"timesteps": np.zeros(0, np.int64), "results": np.zeros((0, self.n), np.float64),
                     "ep_lengths": np.zeros((0, self.n), np.int64), "successes": np.zeros((0, self.n), bool),
                     "collisions": np.zeros((0, self.n), np.int64), "metric": np.zeros(0, np.float64)}
        self.npz_path = os.path.join(ev.log_path, NPZ_NAME) if ev.log_path is not None else None
        if self.npz_path is not None and os.path.exists(self.npz_path):
            self._continue_file()

    def _continue_file(self):
        with np.load(self.npz_path) as f:
            old = {k: f[k] for k in f.files}
        same = (set(self.data) | {"scenarios", "metric_name"}) <= set(old) and \
            [str(s) for s in old["scenarios"]] == self.names and old["results"].ndim == 2 and \
            old["results"].shape[1] == self.n and str(old["metric_name"]) == self.ev.metric
        if not same:
            raise ValueError(f"{self.npz_path} was written under another evaluation protocol (scenarios, runs or "
                             "metric differ): continuing it would mix the two; move it away or use another log_path")
        self.data = {k: old[k].astype(v.dtype) for k, v in self.data.items()}
        good = self.data["metric"][~np.isnan(self.data["metric"])]
        if len(good):
            self.best = float(good.max())

    def due(self, before: int, after: int) -> bool:
        return after // self.ev.eval_freq > before // self.ev.eval_freq

    def _build(self, algo):
        from .config import ENV_TEST_CONFIG
        from .env import Drone2dVecEnv, is_curriculum
        from .evaluate import EvalLoop, sweep_layout

        ev = self.ev
        kw = dict(ENV_TEST_CONFIG if ev.env_kwargs is None else ev.env_kwargs, scenario=list(ev.scenarios))
        if is_curriculum(kw):
            raise ValueError("Evaluation takes static scenarios (names or Scenario objects), at least one")
        self.es = sweep_layout(1, len(self.names), ev.runs)[1]
        if ev.venv_factory is not None:
            self.venv = ev.venv_factory(self.n, self.es, ev.seed, **kw)
            if not (hasattr(self.venv, "get_state") and hasattr(self.venv, "set_state")):
                raise ValueError("Evaluation.venv_factory must return a batch with get_state / set_state: every "
                                 "evaluation rewinds the batch to the state the first one found")
        elif algo.device.type != "cuda":
            raise ValueError("Evaluation on the CPU needs a venv_factory: the default eval batch is a HIP "
                             "Drone2dVecEnv on the PPO's device")
        else:
            self.venv = Drone2dVecEnv(self.n, device=algo.device, seed=ev.seed, with_info=True, env_scenario=self.es,
                                      **kw)
        if isinstance(self.venv, Drone2dVecEnv):
            graph = GRAPH_PAYS if ev.graph is None else bool(ev.graph)
            self.loop = EvalLoop(self.venv, algo.policy, deterministic=ev.deterministic, graph=graph)

    def fly(self, algo) -> tuple:
        """(finished, rows, n_obstacles) of one evaluation of ``algo``'s current policy."""
        from . import harness
        from .evaluate import as_mlp_actor

        if self.venv is None:
            self._build(algo)
        if self.loop is not None:
            fin, rows, _, nobs, _, _ = self.loop.run(self.ev.seed)
            return fin, rows, nobs
        # another backend: the same rewind as EvalLoop's (the episode counters key the spawn draws)
        if self._snap is None:
            self._snap = self.venv.get_state()
        else:
            self.venv.set_state(*self._snap)
        raw = harness.run_first_episodes(self.venv, as_mlp_actor(algo.policy), deterministic=self.ev.deterministic,
                                         seed=self.ev.seed, records=False, gather=False)
        return raw["finished"], raw["rows"], raw["n_obstacles"]

    def __call__(self, algo) -> dict:
        """Evaluate, extend ``evaluations.npz``, save ``best_model.zip`` on a strictly better metric;
        returns the record's ``eval/*`` entries."""
        ev = self.ev
        t0 = time.perf_counter()
        fin, rows, nobs = self.fly(algo)
        out = eval_scalars(self.venv, fin, rows, nobs, self.es, self.names)
        out["eval/seconds"] = time.perf_counter() - t0
        metric = float(out["eval/" + ev.metric])
        per_env = episode_arrays(fin, rows)
        d = self.data
        d["timesteps"] = np.append(d["timesteps"], np.int64(algo.num_timesteps))
        d["metric"] = np.append(d["metric"], metric)
        for k, v in per_env.items():
            d[k] = np.concatenate([d[k], v[None]])
        if self.npz_path is not None:
            os.makedirs(os.path.dirname(self.npz_path) or ".", exist_ok=True)
            tmp = self.npz_path + ".tmp.npz"
            np.savez(tmp, scenarios=np.array(self.names), metric_name=np.array(ev.metric), **d)
            os.replace(tmp, self.npz_path)
        # SB3's `>`: the first of equal scores stays; a NaN compares false and never wins
        if not math.isnan(metric) and (self.best is None or metric > self.best):
            self.best = metric
            if ev.best_model_save_path is not None:
                os.makedirs(ev.best_model_save_path, exist_ok=True)
                algo.save(os.path.join(ev.best_model_save_path, "best_model.zip"))
        out["eval/best"] = self.best if self.best is not None else float("nan")
        return out

    def close(self):
        if self.venv is not None and hasattr(self.venv, "close"):
            self.venv.close()
        self.venv = self.loop = None


__all__ = ["EvaluationRun", "GRAPH_PAYS", "episode_arrays", "eval_scalars", "scenario_names"]
