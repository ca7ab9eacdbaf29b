"""PPO end-to-end on the device: the rollout, GAE and the clipped-surrogate
update all stay on the GPU next to the HIP env batch, with no per-env Python objects.

The reference trains with Stable-Baselines3 2.1 ``PPO("MlpPolicy", env)`` over 14 SubprocVecEnv
workers (main.py:181-210; hyperparameters in ``ppo_agents/PFCA_see_3_obs_17_90.zip:data``: n_steps
2048, batch_size 64, n_epochs 10, gamma 0.99, gae_lambda 0.95, clip_range 0.2, ent_coef 0.01
(rl_config.py:7), vf_coef 0.5, max_grad_norm 0.5, lr 3e-4).  SB3 is not installed in this image;
this module restates the parts of SB3 2.1 that a training run executes, in the same order:

* ``ActorCritic`` (policy.py): SB3's ``MlpPolicy`` for a Box action space.
* ``collect_rollouts`` (SB3 ``OnPolicyAlgorithm.collect_rollouts``): Gaussian actions, clipped to
  the action space only for the env; the stored actions and log-probabilities are the unclipped
  ones; rewards of time-limit truncations are bootstrapped with V(terminal obs) (the reference
  never truncates: time-up is terminal, so this path is idle by default).
* ``compute_returns_and_advantage`` (SB3 ``RolloutBuffer``): GAE(lambda) with episode starts.
* ``train`` (SB3 ``PPO.train``): shuffled minibatches, per-minibatch advantage normalisation,
  clipped surrogate, MSE value loss, entropy bonus, grad-norm clipping, Adam(eps=1e-5); with
  ``PPOConfig.control`` also SB3's learning-rate / clip-range schedules (linear), ``clip_range_vf``,
  ``approx_kl`` and the ``target_kl`` early stop, read from and decided in a device-resident
  ``ControlBlock`` so that they work inside the captured update (DESIGN.md "PPO control").  One
  minibatch step is a stepper's (ppo_step.py: ``ManualStep``, or ``AutogradStep`` for ``manual=False``).
* ``PPOConfig.norm_reward`` (SB3 ``VecNormalize(norm_obs=False, norm_reward=True)``): the rollout records
  rewards divided by the running standard deviation of the discounted returns (normalize.py,
  libd2d_norm.so; DESIGN.md "Reward normalisation"); episode statistics and logs stay raw.

* ``Evaluation`` (SB3 ``EvalCallback``): ``learn(evaluation=...)`` flies the current policy on the test
  scenarios every ``eval_freq`` steps in an env batch of its own, logs ``eval/*`` and keeps
  ``evaluations.npz`` and ``best_model.zip`` (train_eval.py; DESIGN.md "The replayed loop").

At 65 536 envs a 2 048-step rollout would hold 134 M transitions, so GPU-scale runs shorten
n_steps and enlarge batch_size (``PPOConfig.gpu_defaults``); the update rule is unchanged.  With
``torch.distributed`` initialised (one process per GPU, each with its env shard,
``drone2d_amd.shard``), gradients are averaged over ranks before each optimiser step (RCCL).

Agent files (``PPO.save`` / ``PPO.load`` / ``ActorCritic.from_sb3_zip``, ``Checkpoint``): agent_io.py; the
binding of libd2d_ppo.so (``ppo_native``): ppo_native.py.  Their names are importable from here as before.
"""
from __future__ import annotations

import dataclasses
import math
import os
import time
from dataclasses import dataclass

import torch
import torch.distributed as dist

from .agent_io import (AGENT_FORMAT_VERSION, AGENT_MEMBERS, _to_arrays, _to_tensors,  # noqa: F401  (re-exports)
                       read_agent, write_agent)
from .config import TEST_SCENARIOS
from .policy import _HALF_LOG_2PI, ActorCritic  # noqa: F401
from .ppo_native import PPO_CTL_VERSION, D2DPPOCtl, D2DPPORollout, _ok, ppo_native  # noqa: F401
from .ppo_step import STAT_KEYS, AutogradStep, ControlBlock, ManualStep  # noqa: F401


@dataclass
class PPOConfig:
    n_steps: int = 2048
    batch_size: int = 64
    n_epochs: int = 10
    learning_rate: float = 3e-4
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    ent_coef: float = 0.01          # rl_config.py:7
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    normalize_advantage: bool = True
    graph: bool = True              # GPU, one rank: the minibatch update replayed as one HIP graph
    manual: bool = True             # MLP backward + Adam written out over flat buffers (ManualStep)
    # PPO control (include/d2d_ppo.h "PPO control"); None = off.  Setting any of the four selects the
    # control path: the update reads its coefficients from a device-resident control block, records
    # approx_kl and can stop early on its own, also inside a captured HIP graph.
    learning_rate_end: float | None = None  # linear schedule: x = end + (start - end) * progress_remaining
    clip_range_end: float | None = None
    clip_range_vf: float | None = None      # SB3 clip_range_vf: the value prediction clipped around old_values
    target_kl: float | None = None          # SB3 target_kl; float("inf"): never stops, approx_kl logged only
    # Reward normalisation (normalize.py, include/d2d_norm.h): SB3's VecNormalize(norm_obs=False,
    # norm_reward=True, gamma=gamma, clip_reward=clip_reward, epsilon=norm_epsilon) inside the rollout.
    # An agent file carries these three keys only when norm_reward is on (NORM_KEYS).
    norm_reward: bool = False
    clip_reward: float = 10.0
    norm_epsilon: float = 1e-8

    def __post_init__(self):
        for name in ("learning_rate", "clip_range"):
            if callable(getattr(self, name)):
                raise TypeError(f"PPOConfig.{name} is a callable: a schedule cannot be stored in an agent file; "
                                f"give the start value as {name} and the final one as {name}_end (linear in SB3's "
                                "progress_remaining)")

    @property
    def control(self) -> bool:
        return any(x is not None for x in (self.learning_rate_end, self.clip_range_end, self.clip_range_vf,
                                           self.target_kl))

    def coefs(self, progress_remaining: float = 1.0) -> tuple:
        """(lr, clip_range, clip_range_vf or -1.0, KL limit = 1.5 * target_kl or +inf) of an update at
        SB3's ``progress_remaining`` (1 at the start of a run, 0 at its end)."""
        def lin(start, end):
            return start if end is None else end + (start - end) * progress_remaining

        return (float(lin(self.learning_rate, self.learning_rate_end)), float(lin(self.clip_range, self.clip_range_end)),
                -1.0 if self.clip_range_vf is None else float(self.clip_range_vf),
                math.inf if self.target_kl is None else 1.5 * float(self.target_kl))

    @classmethod
    def gpu_defaults(cls, **over) -> "PPOConfig":
        """Short rollouts over many envs (65 536 x 16 = 1 M samples per update), big minibatches."""
        return cls(**dict(dict(n_steps=16, batch_size=32768), **over))


NORM_KEYS = ("norm_reward", "clip_reward", "norm_epsilon")


@dataclass
class Checkpoint:
    """``PPO.learn(checkpoint=...)``: save ``<save_path>/<name_prefix>_<num_timesteps>_steps.zip`` whenever
    ``num_timesteps`` crosses a multiple of ``save_freq`` -- SB3's CheckpointCallback file names, which
    the reference reads back as its curriculum clock (main.py:161-177, drone_2d_env.py:76-86)."""
    save_freq: int
    save_path: str
    name_prefix: str = "rl_model"


@dataclass
class Evaluation:
    """``PPO.learn(evaluation=...)``: SB3's ``EvalCallback``.  After the update whose ``num_timesteps``
    crosses a multiple of ``eval_freq`` the current policy flies ``runs`` first episodes on each of
    ``scenarios`` -- one batch of S x ``runs`` envs, scenario-major (``evaluate.sweep_layout(1, S, runs)``), a
    second env batch of its own -- and the update's record gains ``eval/mean_reward``,
    ``eval/mean_ep_length`` (SB3's two), ``eval/success_rate``, ``eval/collision_rate``,
    ``eval/average_ape`` (``harness.summary``'s numbers), ``eval/seconds``, ``eval/best`` and per scenario
    ``eval/<scenario>/success_rate`` and ``eval/<scenario>/mean_reward``.

    ``<log_path>/evaluations.npz`` holds SB3's ``timesteps`` [E], ``results`` [E, S runs] (episode returns
    in env order) and ``ep_lengths`` [E, S runs], and ``successes``, ``collisions`` (same shape),
    ``scenarios`` (the S names), ``metric`` [E] and ``metric_name``; it is rewritten after every
    evaluation.  A file found when ``learn`` starts is continued when its scenarios, runs and metric
    are this protocol's (the best metric so far is restored from it, so a resumed run does not
    overwrite a better ``best_model.zip``); otherwise ``learn`` raises.  ``<best_model_save_path>/
    best_model.zip`` is ``PPO.save`` whenever ``metric`` is strictly greater than the best so far (SB3's
    ``>``: the first of equal scores stays; a NaN never wins).

    Deviations from SB3, on purpose: (1) SB3 evaluates in mid-rollout, whenever its step counter hits
    ``eval_freq``; here the evaluation runs after the update, as ``checkpoint`` does, so the policy
    evaluated is the one a checkpoint of that step holds.  (2) SB3 lets its eval env run on from one
    evaluation to the next; here every evaluation resets the eval batch to the same ``seed``, so
    successive evaluations face the same spawn draws and differ by the policy alone.

    ``graph``: fly the eval loop as a replayed HIP graph (``evaluate.EvalLoop``); None: what measured
    faster (``train_eval.GRAPH_PAYS``).  One rank only: ``learn`` raises with more."""
    eval_freq: int                               # num_timesteps (this rank's), Checkpoint.save_freq's unit
    scenarios: tuple = TEST_SCENARIOS            # static scenario names or Scenario objects
    runs: int = 16                               # episodes per scenario; n_eval_episodes = S * runs
    deterministic: bool = True                   # SB3's default
    seed: int = 0
    metric: str = "mean_reward"                  # or "success_rate"; larger is better
    log_path: str | None = None                  # <log_path>/evaluations.npz
    best_model_save_path: str | None = None      # <path>/best_model.zip
    env_kwargs: dict | None = None               # default ENV_TEST_CONFIG
    graph: bool | None = None
    venv_factory: object = None                  # (num_envs, env_scenario, seed, **kw) -> batch; None: Drone2dVecEnv


def compute_gae(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """SB3 ``RolloutBuffer.compute_returns_and_advantage``: tensors [T, N] (episode_starts[t] = the
    env started a new episode at step t), last_* [N]; returns (advantages, returns)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last_gae = torch.zeros_like(last_values)
    for step in reversed(range(T)):
        if step == T - 1:
            next_non_terminal = 1.0 - last_dones.to(rewards.dtype)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1].to(rewards.dtype)
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae = delta + gamma * gae_lambda * next_non_terminal * last_gae
        adv[step] = last_gae
    return adv, adv + values


class PPO:
    """PPO on a batched env with Drone2dVecEnv's tensor interface (``reset() -> obs``,
    ``step(actions) -> (obs, reward, terminated, truncated, info)``, ``terminal_obs``)."""

    def __init__(self, venv, config: PPOConfig | None = None, policy: ActorCritic | None = None, seed: int = 0,
                 device=None):
        self.venv = venv
        self.cfg = config or PPOConfig()
        self.seed = int(seed)
        self.device = torch.device(device) if device is not None else torch.device(venv.device)
        torch.manual_seed(seed)
        self.policy = (policy or ActorCritic()).to(self.device)
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.use_graph = bool(self.cfg.graph and self.device.type == "cuda" and self.world == 1)
        if self.cfg.norm_reward and self.world > 1:
            raise ValueError("norm_reward=True with more than one rank: every rank would keep the running statistics "
                             "of its own env shard and scale its rewards differently, and an all-reduced rms is not "
                             "built")
        if self.world > 1:
            # one policy on every rank: rank 0's initial parameters; each rank its own noise stream
            for p in self.policy.parameters():
                dist.broadcast(p.data, 0)
        # one minibatch step (ppo_step.py); `manual` / `opt`: the ManualStep / the torch optimiser, or None
        self._stepper = (ManualStep(self.policy, self.cfg, self.device) if self.cfg.manual else
                         AutogradStep(self.policy, self.cfg, self.device, capturable=self.use_graph))
        self.manual = self._stepper if self.cfg.manual else None
        self.opt = getattr(self._stepper, "opt", None)
        rank = dist.get_rank() if self.world > 1 else 0
        self.gen = torch.Generator(device=self.device).manual_seed(seed + 1_000_003 * rank)
        self.n_envs = int(venv.num_envs)
        self.num_timesteps = 0
        # the rollout lands in fixed buffers (a captured update reads them at fixed addresses)
        M = self.cfg.n_steps * self.n_envs
        dev = self.device
        self._flat = (torch.empty(M, 27, device=dev), torch.empty(M, 2, device=dev), torch.empty(M, device=dev),
                      torch.empty(M, device=dev), torch.empty(M, device=dev))
        # PPO control: SB3's progress_remaining (learn() sets it after every rollout; a caller of train()
        # may set it), and the stepper's control block, whose tail holds the statistics, so an update's
        # record is one transfer
        self.progress_remaining = 1.0
        self._ctl = self._stepper.ctl
        self._acc = self._ctl.acc() if self._ctl is not None else {k: torch.zeros((), device=dev) for k in STAT_KEYS}
        self._graph = None
        self._gidx = None
        self._ro = None          # rollout buffers (_alloc_rollout)
        self._ro_graph = None    # the captured rollout (GPU)
        self._ro_warm = False
        self._ro_gen = None      # the env's generation the rollout graph was captured against
        # the libd2d_ppo.so path (GPU, ManualStep): the epochs' shuffles from d2d_ppo_permute (a device
        # counter keys them, so the whole update -- shuffles and every minibatch step -- replays as one
        # HIP graph) and the rollout as one fused launch per step (d2d_ppo_rollout_step)
        self._hip = self._stepper.lib is not None
        self._perm = None
        self._perm_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self._perm_seed = (seed * 0x9E3779B97F4A7C15 + rank * 0xD1B54A32D192ED03 + 1) % (1 << 64)
        self._upd_warm = False
        self._adv_ws = None      # every minibatch's advantage-statistics partials (_train_body_hip)
        self._fused = None       # decided at the first rollout (_alloc_rollout)
        self._predict_t = 0      # predict()'s call counter: the Philox step index of its noise
        self._predict_gen = None
        self._ev_run = None      # learn(evaluation=...)'s EvaluationRun: the eval batch and its loop
        self.monitor = None      # an EpisodeMonitor (set_monitor / learn(monitor=...)); None: off
        self.normalizer = None   # a RewardNormalizer (cfg.norm_reward); None: the rollout records raw rewards
        if self.cfg.norm_reward:
            from .normalize import RewardNormalizer

            self.normalizer = RewardNormalizer(venv, self.cfg.gamma, self.cfg.clip_reward, self.cfg.norm_epsilon,
                                               device=getattr(venv, "device", self.device))

    # ------------------------------------------------------------------ rollout
    def _alloc_rollout(self):
        from .env import Drone2dVecEnv

        T, N, dev = self.cfg.n_steps, self.n_envs, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        # time-limit truncations are bootstrapped with V(terminal obs); the reference never truncates
        self._truncates = bool(getattr(getattr(self.venv, "cfg", None), "timeup_truncates", 1))
        # the fused rollout: the HIP env batch (with _truncates its step is d2d_ppo_rollout_step_tb)
        self._fused = bool(self._hip and isinstance(self.venv, Drone2dVecEnv))
        self._ro = {"val": torch.empty(T, N, device=dev), "rew": torch.empty(T, N, device=dev),
                    "done": torch.empty(T, N, dtype=torch.bool, device=dev),
                    "start0": torch.empty(N, dtype=torch.bool, device=dev),
                    "noise": torch.empty(T, N, 2, device=dev), "fin": torch.zeros((), **f64),
                    "ret": torch.zeros((), **f64)}
        if self._fused:
            self._ro["act_env"] = torch.empty(N, 2, device=dev)
            self._ro["stats"] = torch.zeros(T, (N + 63) // 64, 2, **f64)
            self._ro["obs_cur"] = None
        else:
            self._ro.update(obs=torch.empty(T + 1, N, 27, device=dev), act=torch.empty(T, N, 2, device=dev),
                            logp=torch.empty(T, N, device=dev))

    def _set_first_obs(self, obs):
        if self._fused:
            self._ro["obs_cur"] = obs  # the env's output tensor; the fused step reads it in place
        else:
            self._ro["obs"][0].copy_(obs.to(self.device))
        self._ro["start0"].fill_(True)

    def set_monitor(self, monitor=True):
        """Attach an ``EpisodeMonitor`` (``True``: a new one for the env batch) or detach it (``None`` /
        ``False``).  The rollout then digests every env step's outputs with one ``monitor.step`` and ends
        with one ``monitor.flush``; the record gains ``monitor/*`` and ``train/explained_variance``.  A
        monitor attached to a batch in mid-flight (after ``PPO.load``, or between two ``learn`` calls)
        starts with ``live=0``: the episodes under way are counted as skipped, not logged with partial
        sums.  A captured rollout is dropped and captured again on the usual schedule."""
        if monitor is True:
            if self.monitor is not None:
                return self.monitor
            from .monitor import EpisodeMonitor

            monitor = EpisodeMonitor(self.venv, getattr(self.venv, "device", self.device))
        elif monitor is False:
            monitor = None
        if monitor is self.monitor:
            return monitor
        if monitor is not None and monitor.n != self.n_envs:
            raise ValueError(f"the monitor is for {monitor.n} envs, the batch has {self.n_envs}")
        self.monitor = monitor
        self._ro_graph = None
        self._ro_warm = False
        if monitor is not None and self._ro is not None:
            monitor.reset(live=False)  # (a fresh run resets it with the envs, in collect_rollouts)
        return monitor

    def _reset_envs(self):
        obs = self.venv.reset()
        if self.monitor is not None:
            self.monitor.reset()
        if self.normalizer is not None:
            self.normalizer.reset()  # the discounted returns start over; the running statistics stay
        return obs

    @torch.no_grad()
    def _rollout_body_fused(self):
        """_rollout_body as T + 1 libd2d_ppo.so launches around the T env steps: step t's launch runs
        both MLPs on the env's observation tensor, samples and stores the action, log-density and
        value, copies the observations into the flat buffer and records step t-1's reward / done /
        episode statistics; the last one adds the bootstrap value and GAE (d2d_ppo_rollout_step).  With
        ``_truncates`` the launch is d2d_ppo_rollout_step_tb, which also reads step t-1's terminal
        observations and adds gamma V(terminal obs) to the recorded reward of the envs that truncated --
        after the normaliser has rewritten the reward, SB3's order around a VecNormalize."""
        from . import abi

        R, T, N, lib = self._ro, self.cfg.n_steps, self.n_envs, self.manual.lib
        st = self.manual._stream()
        wptr = self.manual.weight_ptrs()
        obs_buf, act_buf, logp_buf, adv_buf, ret_buf = self._flat
        ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
        r = D2DPPORollout(n=N, T=T, info_dim=abi.INFO_DIM, info_totrew=abi.INFO_TOTREW, gamma=self.cfg.gamma,
                          gae_lambda_gamma=self.cfg.gamma * self.cfg.gae_lambda,
                          log_std=ptr(self.policy.log_std), obs_buf=ptr(obs_buf), act_buf=ptr(act_buf),
                          logp_buf=ptr(logp_buf), val_buf=ptr(R["val"]), rew_buf=ptr(R["rew"]),
                          done_buf=ptr(R["done"]), start0=ptr(R["start0"]), act_env=ptr(R["act_env"]),
                          adv_buf=ptr(adv_buf), ret_buf=ptr(ret_buf), stats=ptr(R["stats"]))
        obs, tobs = R["obs_cur"], None
        for t in range(T + 1):
            r.t = t
            r.obs = ptr(obs)
            r.noise = ptr(R["noise"][t]) if t < T else None
            if self._truncates:
                _ok(lib.d2d_ppo_rollout_step_tb(r, ptr(tobs), wptr, st), "d2d_ppo_rollout_step_tb")
            else:
                _ok(lib.d2d_ppo_rollout_step(r, wptr, st), "d2d_ppo_rollout_step")  # (passed by reference: argtypes)
            if t < T:
                obs, rew, term, trunc, info = self.venv.step(R["act_env"])
                if self.monitor is not None:
                    self.monitor.step(term, trunc, info)
                if self.normalizer is not None:  # (the monitor and the episode statistics read info: raw)
                    rew = self.normalizer.step(rew, term, trunc)
                r.prev_rew, r.prev_term, r.prev_trunc, r.prev_info = ptr(rew), ptr(term), ptr(trunc), ptr(info)
                tobs = self.venv.terminal_obs  # of this step: double-buffered like the other outputs
        if self.monitor is not None:
            self.monitor.flush()
        R["obs_cur"] = obs  # T even: the same double-buffer slot as at the start
        R["fin"].copy_(R["stats"][..., 0].sum())
        R["ret"].copy_(R["stats"][..., 1].sum())

    @torch.no_grad()
    def _rollout_body(self):
        """n_steps policy + env steps into the rollout buffers, then GAE into the flat buffers.
        Reads obs[0], start0 and noise; leaves the next rollout's obs[0] / start0 in place.  No host
        synchronisation: on a GPU the whole body is one captured HIP graph."""
        from . import abi

        R, pol, T, dev = self._ro, self.policy, self.cfg.n_steps, self.device
        std = pol.log_std.exp()
        for t in range(T):
            mean, value = pol(R["obs"][t])
            actions = mean + std * R["noise"][t]
            logp = pol.log_prob(mean, actions)
            # SB3 clips to the Box bounds for the env only; the buffer keeps the unclipped action
            new_obs, rew, term, trunc, info = self.venv.step(actions.clamp(-1.0, 1.0))
            if self.monitor is not None:
                self.monitor.step(term, trunc, info)
            if self.normalizer is not None:
                # before the truncation bootstrap below, the order SB3's PPO gets around a VecNormalize
                rew = self.normalizer.step(rew, term, trunc)
            rew = rew.to(dev).float()
            trunc = trunc.to(dev)
            done = term.to(dev) | trunc
            if self._truncates:
                tv = pol.predict_values(self.venv.terminal_obs.to(dev))
                rew = torch.where(trunc, rew + self.cfg.gamma * tv, rew)
            R["obs"][t + 1].copy_(new_obs)
            R["act"][t].copy_(actions)
            R["logp"][t].copy_(logp)
            R["val"][t].copy_(value)
            R["rew"][t].copy_(rew)
            R["done"][t].copy_(done)
            if info is not None:
                R["fin"] += done.sum()
                R["ret"] += torch.where(done, info[:, abi.INFO_TOTREW].to(dev).double(), 0.0).sum()
        last_values = pol.predict_values(R["obs"][T])
        starts = torch.cat([R["start0"][None], R["done"][:-1]])
        adv, ret = compute_gae(R["rew"], R["val"], starts, last_values, R["done"][T - 1], self.cfg.gamma,
                               self.cfg.gae_lambda)
        N = self.n_envs
        for dst, src in zip(self._flat, (R["obs"][:T].reshape(T * N, 27), R["act"].reshape(T * N, 2),
                                         R["logp"].reshape(-1), adv.reshape(-1), ret.reshape(-1))):
            dst.copy_(src)
        R["obs"][0].copy_(R["obs"][T])
        R["start0"].copy_(R["done"][T - 1])
        if self.monitor is not None:
            self.monitor.flush()

    def collect_rollouts(self) -> dict:
        T, N = self.cfg.n_steps, self.n_envs
        gen = getattr(self.venv, "generation", None)
        if self._ro is not None and gen != self._ro_gen:
            # the env re-allocated its scenario tables (set_curriculum / set_scenarios): a captured
            # rollout would replay against freed memory, and the envs were reset -- drop the graph
            # and start the next rollout from a reset
            self._ro_graph = None
            self._ro_warm = False
            self._set_first_obs(self._reset_envs())
        self._ro_gen = gen
        if self._ro is None:
            self._alloc_rollout()
            self._set_first_obs(self._reset_envs())
        R = self._ro
        body = self._rollout_body_fused if self._fused else self._rollout_body
        R["fin"].zero_()
        R["ret"].zero_()
        torch.randn(R["noise"].shape, generator=self.gen, device=self.device, out=R["noise"])
        # capture only whole fill periods: d2d_step launches the reset-cache fill after every 16th
        # step, decided on the host, so a graph of another length would bake in a fill on every
        # replay or on none (still correct through the synchronous reset path, but slower)
        graph_ok = self.cfg.graph and self.device.type == "cuda" and T % 16 == 0
        if graph_ok and self._ro_graph is None and self._ro_warm:
            # second rollout: capture (the first one ran eagerly: library and allocator warm-up);
            # T even, so the env's double-buffered outputs are back at their start after a replay
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            self._ro_graph = g
        if self._ro_graph is not None:
            self._ro_graph.replay()
        else:
            body()
            self._ro_warm = True
        self.num_timesteps += T * N
        if self.monitor is None and self.normalizer is None:
            f, r = float(R["fin"]), float(R["ret"])
            return {"episodes": f, "mean_return": r / f if f else float("nan")}
        # fin, ret, the normaliser's variance, the explained variance and the flushed vector packed on the
        # device and read with one copy, where fin and ret were read before
        pack = [R["fin"].reshape(1), R["ret"].reshape(1)]
        if self.normalizer is not None:
            pack.append(self.normalizer.rms[1:2].to(self.device))
        if self.monitor is not None:
            pack += [self._explained_variance().to(torch.float64).reshape(1), self.monitor.out.to(self.device)]
        host = torch.cat(pack).cpu()
        f, r = float(host[0]), float(host[1])
        out = {"episodes": f, "mean_return": r / f if f else float("nan")}
        at = 2
        if self.normalizer is not None:
            var = float(host[at])
            at += 1
        if self.monitor is not None:
            out.update({"monitor/" + k: v for k, v in self.monitor.scalars(host[at + 1:]).items()})
            out["train/explained_variance"] = float(host[at])
        if self.normalizer is not None:
            # what a reward is divided by after this rollout, and the running variance of the returns
            out["norm/reward_scale"] = math.sqrt(var + self.normalizer.epsilon) if var == var else float("nan")
            out["norm/return_var"] = var
        return out

    @torch.no_grad()
    def _explained_variance(self) -> torch.Tensor:
        """SB3's ``explained_variance(values, returns)`` over the rollout buffer, before the update:
        1 - Var(returns - values) / Var(returns) (NaN when the returns do not vary)."""
        val, ret = self._ro["val"].reshape(-1), self._flat[4]
        var_y = torch.var(ret, unbiased=False)
        return torch.where(var_y == 0, torch.full_like(var_y, float("nan")),
                           1.0 - torch.var(ret - val, unbiased=False) / var_y)

    # ------------------------------------------------------------------ update
    def _minibatch(self, idx: torch.Tensor, zero_grad: bool = True, adv_ws=None):
        """One SB3 PPO gradient step on rollout samples ``idx`` (statistics accumulated on device)."""
        self._stepper.step(idx, self._rollout_data(), self._acc, self.world, adv_ws, zero_grad)

    def _rollout_data(self) -> tuple:
        """The steppers' rollout tuple; on the control path with the rollout's stored values (SB3's
        ``old_values``: the buffer the rollout wrote, in the flat buffers' sample order)."""
        return self._flat if self._ctl is None else self._flat + (self._ro["val"].reshape(-1),)

    def _capture(self):
        """Record one full-size minibatch step as a HIP graph: forward, backward, grad clipping and
        the (capturable) Adam step replay with no per-kernel launches from Python."""
        self._gidx = torch.zeros(self.cfg.batch_size, dtype=torch.long, device=self.device)
        saved = {k: v.clone() for k, v in self._acc.items()}
        self.opt.zero_grad(set_to_none=True)  # (AutogradStep's: ManualStep on a GPU takes _train_body_hip)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._minibatch(self._gidx, zero_grad=False)
        for k, v in saved.items():  # capture does not execute: nothing to undo, but keep the sums exact
            self._acc[k].copy_(v)
        self._graph = g

    def _train_body_hip(self):
        """One update on the libd2d_ppo.so path: the n_epochs shuffles in one launch
        (d2d_ppo_permute), then every minibatch step; nothing waits for the host, so on one rank the
        whole update is captured and replayed as one HIP graph."""
        M, bs, E = self._flat[0].shape[0], self.cfg.batch_size, self.cfg.n_epochs
        if self._ctl is not None:
            self.manual.reset_control()  # the update's first node
        for v in self._acc.values():
            v.zero_()
        lib, st = self.manual.lib, self.manual._stream()
        _ok(lib.d2d_ppo_permute(M, E, self._perm_seed, self._perm_ctr.data_ptr(), self._perm.data_ptr(), st),
            "d2d_ppo_permute")
        # the advantage statistics of every minibatch of the update in one launch: 64-row partials over
        # the whole shuffle; minibatch boundaries fall on partial boundaries when M and bs are multiples
        # of 64, so each minibatch reads its own slice (otherwise each minibatch computes its own)
        ws = None
        if self.manual.fused and self.cfg.normalize_advantage and M % 64 == 0 and bs % 64 == 0:
            if self._adv_ws is None:
                self._adv_ws = torch.zeros(E * M // 64, 2, dtype=torch.float64, device=self.device)
            _ok(lib.d2d_ppo_adv_stats(E * M, self._perm.data_ptr(), self._flat[3].data_ptr(),
                                      self._adv_ws.data_ptr(), st), "d2d_ppo_adv_stats")
            ws = self._adv_ws
        for e in range(E):
            for s in range(0, M, bs):
                n = min(s + bs, M) - s
                aw = ws[(e * M + s) // 64:].data_ptr() if (ws is not None and n > 1) else None
                self._minibatch(self._perm[e * M + s:e * M + s + n], adv_ws=aw)

    def train(self) -> dict:
        """One update on the last rollout.  On the control path (``cfg.control``) the coefficients of
        ``cfg.coefs(self.progress_remaining)`` are written to the control block first -- one small copy,
        outside the captured graph, which reads them from memory on every replay -- and the record
        gains ``approx_kl``, ``n_minibatches``, ``early_stop``, ``learning_rate``, ``clip_range`` and
        (when on) ``clip_range_vf``; the four means are over the recorded minibatches."""
        M, bs = self._flat[0].shape[0], self.cfg.batch_size
        ctl = self._ctl
        if ctl is not None:
            ctl.set(*self.cfg.coefs(self.progress_remaining))
            self._stepper.set_lr(ctl.coef[0])
        if self._hip:
            if self._perm is None:
                self._perm = torch.empty(self.cfg.n_epochs * M, dtype=torch.int64, device=self.device)
            if self.use_graph and self._graph is None and self._upd_warm:
                # second update: capture the whole update (the first ran eagerly: kernels loaded, every
                # minibatch size's work buffers allocated)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._train_body_hip()
                self._graph = g
            if self._graph is not None:
                self._graph.replay()
            else:
                self._train_body_hip()
                self._upd_warm = True
            n_upd = self.cfg.n_epochs * -(-M // bs)
            # (control: the statistics and the counters in one transfer)
            return ctl.read() if ctl is not None else {k: float(v) / n_upd for k, v in self._acc.items()}
        if ctl is not None:
            self._stepper.reset_control()
        for v in self._acc.values():
            v.zero_()
        n_upd = 0
        warm = 0
        for _ in range(self.cfg.n_epochs):
            # (a stopped update still draws every epoch's shuffle: the generator's state after an
            # update does not depend on whether it stopped)
            perm = torch.randperm(M, device=self.device, generator=self.gen)
            for s in range(0, M, bs):
                if ctl is not None and ctl.stopped():
                    break
                idx = perm[s:s + bs]
                if self.use_graph and idx.numel() == bs and ctl is None:
                    if self._graph is None and warm >= 3:
                        # capture after a few eager steps (lazy optimiser state, allocator warm-up)
                        torch.cuda.synchronize(self.device)
                        self._capture()
                    if self._graph is not None:
                        self._gidx.copy_(idx)
                        self._graph.replay()
                        n_upd += 1
                        continue
                    warm += 1
                self._minibatch(idx)
                n_upd += 1
        return ctl.read() if ctl is not None else {k: float(v) / max(n_upd, 1) for k, v in self._acc.items()}

    def learn(self, total_timesteps: int, log=None, checkpoint: Checkpoint | None = None, monitor=None,
              logger=None, schedule_timesteps: int | None = None, evaluation: Evaluation | None = None) -> list[dict]:
        """Alternate rollouts and updates until ``total_timesteps`` env steps (this rank);
        ``checkpoint``: save the agent whenever ``num_timesteps`` crosses a multiple of its
        ``save_freq`` (after the update, so a resumed run continues with the next rollout).
        ``monitor``: ``True`` or an ``EpisodeMonitor`` -- ``set_monitor`` it first (``None``: leave
        things as they are; off unless one was set).  ``logger``: a ``trainlog.ScalarLog`` (anything
        with ``log(record)``) that gets every record after ``log``.  After each rollout and before its
        update, ``progress_remaining = 1 - num_timesteps / total_timesteps`` (SB3's
        ``OnPolicyAlgorithm.learn``; not below 0 when the last rollout overshoots), which the schedules
        ``learning_rate_end`` / ``clip_range_end`` read; ``schedule_timesteps``: the schedule's horizon
        when it is not this call's ``total_timesteps`` (a run driven by several ``learn`` calls).
        ``evaluation``: an ``Evaluation`` -- the policy is flown on test scenarios after the update whose
        ``num_timesteps`` crosses a multiple of its ``eval_freq`` (before that update's checkpoint), and
        that update's record gains ``eval/*``; the eval batch is built at the first evaluation and kept (also
        for a later ``learn`` call with the same object; ``close_evaluation`` drops it).  None: nothing
        is launched or written for it."""
        horizon = float(schedule_timesteps if schedule_timesteps is not None else total_timesteps)
        if monitor is not None:
            self.set_monitor(monitor)
        ev_run = None
        if evaluation is not None:
            if self.world > 1:
                raise ValueError("evaluation=... with more than one rank: every rank would fly the whole eval batch "
                                 "and keep files of its own, and an evaluation sharded over the ranks is not built")
            from .train_eval import EvaluationRun

            # a run driven by several learn calls with one Evaluation object keeps its eval batch, its
            # captured loop and its best metric from call to call
            if self._ev_run is None or self._ev_run.ev is not evaluation:
                self.close_evaluation()
                self._ev_run = EvaluationRun(evaluation, self)
            ev_run = self._ev_run
        return self._learn(total_timesteps, horizon, log, checkpoint, logger, ev_run)

    def close_evaluation(self):
        """Drop the eval batch a ``learn(evaluation=...)`` built (it is otherwise kept for the next
        ``learn`` call with the same ``Evaluation`` object, and closed with this object)."""
        if self._ev_run is not None:
            self._ev_run.close()
        self._ev_run = None

    def _learn(self, total_timesteps, horizon, log, checkpoint, logger, ev_run) -> list[dict]:
        hist = []
        while self.num_timesteps < total_timesteps:
            before = self.num_timesteps
            t0 = time.perf_counter()
            ro = self.collect_rollouts()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            t1 = time.perf_counter()
            self.progress_remaining = max(0.0, 1.0 - self.num_timesteps / horizon)
            tr = self.train()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            t2 = time.perf_counter()
            rec = dict(ro, **tr, timesteps=self.num_timesteps, rollout_s=t1 - t0, train_s=t2 - t1,
                       env_steps_per_s=self.cfg.n_steps * self.n_envs / (t2 - t0))
            if ev_run is not None and ev_run.due(before, self.num_timesteps):
                rec.update(ev_run(self))
            hist.append(rec)
            if log:
                log(rec)
            if logger is not None:
                logger.log(rec)
            if checkpoint is not None and self.num_timesteps // checkpoint.save_freq > before // checkpoint.save_freq:
                os.makedirs(checkpoint.save_path, exist_ok=True)
                self.save(os.path.join(checkpoint.save_path,
                                       f"{checkpoint.name_prefix}_{self.num_timesteps}_steps.zip"))
        return hist

    # ------------------------------------------------------------------ predict / save / load
    @torch.no_grad()
    def predict(self, obs, deterministic: bool = False) -> torch.Tensor:
        """The clipped actions for ``obs`` [n, 27] (SB3 ``model.predict``; stochastic by default, as the
        reference calls it).  On a HIP device the evaluation library's act half (``evaluate.act``): call
        k's noise for row i is the Philox draw of (seed, i, k); on the CPU the same in torch."""
        x = torch.as_tensor(obs, dtype=torch.float32).to(self.device).reshape(-1, 27)
        if self.device.type == "cuda":
            from . import evaluate

            a = evaluate.act(self.policy, x, deterministic=deterministic, seed=self.seed, t=self._predict_t)
        else:
            a = self.policy(x)[0]
            if not deterministic:
                if self._predict_gen is None:
                    self._predict_gen = torch.Generator(device=self.device).manual_seed(self.seed + 7)
                a = a + self.policy.log_std.exp() * torch.randn(a.shape, generator=self._predict_gen)
            a = a.clamp(-1.0, 1.0)
        if not deterministic:
            self._predict_t += 1
        return a

    def _train_state(self) -> dict:
        ts = {"gen": self.gen.get_state(), "perm_ctr": self._perm_ctr, **self._stepper.state()}
        if self._ro is not None:
            ts["last_obs"] = self._ro["obs_cur"] if self._fused else self._ro["obs"][0]
            ts["start0"] = self._ro["start0"]
        return _to_tensors(ts)

    def save(self, path: str) -> str:
        """Write the agent as a zip laid out like SB3's: ``policy.pth`` (the policy's state_dict under
        SB3's names), ``train_state.pth`` (Adam moments and step counter, the rollout noise generator,
        the shuffle counter, the rollout's carried observations and episode starts), ``env_state.pth``
        (``venv.state_dict()``, when the batch has one) and ``data.json`` (format version, PPOConfig,
        num_timesteps, n_envs, seed).  With ``norm_reward`` also ``reward_norm.pth`` (the normaliser's
        ``rms`` and ``ret``); without it the file has neither that member nor the config's NORM_KEYS, so
        it is the file earlier versions wrote and read.  Tensors and JSON only."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        members = {"policy.pth": _to_tensors(dict(self.policy.state_dict())), "train_state.pth": self._train_state()}
        if hasattr(self.venv, "state_dict"):
            members["env_state.pth"] = _to_tensors(self.venv.state_dict())
        if self.normalizer is not None:
            sd = self.normalizer.state_dict()
            members["reward_norm.pth"] = {"rms": sd["rms"], "ret": sd["ret"]}
        config = dataclasses.asdict(self.cfg)
        if not self.cfg.norm_reward:
            for k in NORM_KEYS:
                del config[k]
        data = {"format_version": AGENT_FORMAT_VERSION, "config": config,
                "num_timesteps": int(self.num_timesteps), "n_envs": self.n_envs, "seed": self.seed}
        return write_agent(path, data, members)

    @classmethod
    def load(cls, path: str, venv, device=None, restore_env: bool = True) -> "PPO":
        """The agent of ``save``'s file on ``venv``, ready to go on learning where the saved run
        stopped: policy, optimiser state, noise generator and shuffle counter, ``num_timesteps``, the env
        batch's state (``restore_env``, when the file has one and ``venv`` can take it) and the
        rollout's carried observations, so the next ``collect_rollouts`` continues the running episodes
        instead of resetting them.  The first rollout and update after a load run eagerly and the HIP
        graphs are captured again on the usual schedule (a captured rollout reads the env's own
        observation tensor at a fixed address, which the restored observations are not in)."""
        data, members = read_agent(path)
        ts = members["train_state.pth"]
        if int(venv.num_envs) != int(data["n_envs"]):
            raise ValueError(f"{path}: saved with {data['n_envs']} envs, the batch has {venv.num_envs}")
        algo = cls(venv, PPOConfig(**data["config"]), seed=int(data["seed"]), device=device)
        algo.policy.load_state_dict(members["policy.pth"])  # in place: ManualStep's flat buffer holds the parameters
        try:
            algo._stepper.load_state(ts)
        except ValueError as e:  # (the file's optimiser state is the other stepper's)
            raise ValueError(f"{path}: {e}") from None
        algo.gen.set_state(ts["gen"])
        algo._perm_ctr.copy_(ts["perm_ctr"])
        algo.num_timesteps = int(data["num_timesteps"])
        if algo.normalizer is not None:
            if "reward_norm.pth" not in members:
                raise ValueError(f"{path}: saved with norm_reward but without reward_norm.pth")
            algo.normalizer.load_state_dict(members["reward_norm.pth"])
        if restore_env and "env_state.pth" in members and hasattr(venv, "load_state_dict"):
            venv.load_state_dict(_to_arrays(members["env_state.pth"]))
        if "last_obs" in ts:
            algo._alloc_rollout()
            last_obs = ts["last_obs"].to(algo.device)
            if algo._fused:
                algo._ro["obs_cur"] = last_obs.contiguous()
            else:
                algo._ro["obs"][0].copy_(last_obs)
            algo._ro["start0"].copy_(ts["start0"])
            # collect_rollouts resets the envs when the batch's generation is not the one it last saw
            algo._ro_gen = getattr(venv, "generation", None)
        return algo


__all__ = ["PPOConfig", "Checkpoint", "Evaluation", "ActorCritic", "ManualStep", "PPO", "compute_gae"]
