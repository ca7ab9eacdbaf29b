#!/usr/bin/env python3
"""PPO training end-to-end on one MI355X (GPU box): the HIP env batch + drone2d_amd.ppo.

    python tools/train_ppo.py [--envs 65536] [--updates 30] [--scenario corridor | --curriculum]
                              [--save AGENT.zip] [--checkpoint-every STEPS] [--resume AGENT.zip]
                              [--log-dir DIR [--no-tensorboard]]
                              [--lr-end LR] [--clip-range-end C] [--clip-range-vf C] [--target-kl KL]
                              [--norm-reward [--clip-reward X]] [--timeup-truncates [--episode-steps K]]
                              [--eval-freq STEPS [--eval-runs R] [--eval-scenarios a,b,...] [--eval-metric M]]

One JSON line per update (timesteps, mean finished-episode return, losses, env-steps/s including
the policy forward passes and the PPO update) into gpurun_out/ppo.jsonl and on stdout.
``--curriculum`` trains as the reference does (mode='train': a fresh curriculum scenario per
reset, stage by the global step count, drone_2d_env.py:76-86 / 324-372), with the pool refreshed
(and the stage advanced) every ``--refresh`` updates.
``--save`` writes the trained agent (``PPO.save``; ``tools/test_agent.py`` tests it), ``--checkpoint-every``
also ``<dir of --save, or ppo_agents/ in the working directory>/rl_model_<steps>_steps.zip`` whenever the step count crosses
a multiple of STEPS (the reference's checkpoint names), ``--resume`` continues a saved run: policy,
optimiser, noise streams and the env batch as they were (same --envs, --n-steps, --batch as saved).
``--log-dir`` attaches the episode monitor (drone2d_amd.monitor) and writes ``progress.csv``, a TensorBoard
event file, ``env_train_config.txt`` and ``rl_config.txt`` there (drone2d_amd.trainlog; the reference's
``tensorboard_log="logs"`` + ``TensorboardLogger``, main.py:192-208).
``--lr-end`` / ``--clip-range-end`` (linear schedules over the run's ``--updates``), ``--clip-range-vf`` and
``--target-kl`` (``inf``: log approx_kl only) select PPO's control path (PPOConfig; DESIGN.md "PPO control").
``--norm-reward`` normalises the rewards the rollout records as SB3's ``VecNormalize(norm_obs=False, norm_reward=True)``
does, clipped at ``--clip-reward`` (default 10; DESIGN.md "Reward normalisation"); the logs keep the raw returns.
``--timeup-truncates`` builds the batch with ``timeup_truncates=True``: the time-up is a truncation, and the rollout adds
``gamma V(terminal obs)`` to a truncated step's reward inside its fused step (DESIGN.md "Truncation bootstrap");
``--episode-steps`` sets the env's time limit (the config's ``n_steps``, 1 100 by default).
``--eval-freq`` flies the current policy on the test scenarios (``--eval-scenarios``, default all seven; ``--eval-runs``
episodes each) after the update that crosses a multiple of STEPS (``ppo.Evaluation``, SB3's EvalCallback): ``eval/*`` in the
record and the logs, ``best_model.zip`` (by ``--eval-metric``) beside ``--save`` or else in ``--log-dir``, ``evaluations.npz`` in
``--log-dir``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--n-steps", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--scenario", default="corridor")
    ap.add_argument("--curriculum", action="store_true")
    ap.add_argument("--pool", type=int, default=4096, help="curriculum pool size; 0: the fresh curriculum")
    ap.add_argument("--refresh", type=int, default=100, help="updates between curriculum pool refreshes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-graph", action="store_true", help="eager minibatch updates (A/B against the HIP graph)")
    ap.add_argument("--autograd", action="store_true", help="autograd + torch Adam update (A/B against ManualStep)")
    ap.add_argument("--save", default=None, metavar="PATH", help="write the trained agent here (PPO.save)")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="STEPS",
                    help="also save rl_model_<steps>_steps.zip every STEPS env steps")
    ap.add_argument("--resume", default=None, metavar="PATH", help="continue the run saved in this agent file")
    ap.add_argument("--log-dir", default=None, metavar="DIR",
                    help="monitor the episodes on the device and write progress.csv, a TensorBoard event file and "
                         "the two config files here")
    ap.add_argument("--no-tensorboard", action="store_true", help="with --log-dir: progress.csv only")
    ap.add_argument("--lr-end", type=float, default=None, help="learning rate at the end of the run (linear schedule)")
    ap.add_argument("--clip-range-end", type=float, default=None, help="clip range at the end of the run")
    ap.add_argument("--clip-range-vf", type=float, default=None, help="SB3 clip_range_vf")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="SB3 target_kl: stop an update when a minibatch's approx_kl exceeds 1.5 x this (inf: log only)")
    ap.add_argument("--norm-reward", action="store_true",
                    help="normalise the rollout's rewards by the running std of the discounted returns (VecNormalize)")
    ap.add_argument("--clip-reward", type=float, default=10.0, metavar="X", help="with --norm-reward: clip at +-X")
    ap.add_argument("--timeup-truncates", action="store_true",
                    help="report the time-up as a truncation and bootstrap it with the value of the terminal observation")
    ap.add_argument("--episode-steps", type=int, default=None, metavar="K", help="the env's time limit (config n_steps)")
    ap.add_argument("--eval-freq", type=int, default=0, metavar="STEPS",
                    help="evaluate on the test scenarios every STEPS env steps (after the update that crosses them)")
    ap.add_argument("--eval-runs", type=int, default=16, metavar="R", help="with --eval-freq: episodes per scenario")
    ap.add_argument("--eval-scenarios", default=None, metavar="a,b,...",
                    help="with --eval-freq: the scenarios (default: the seven test scenarios)")
    ap.add_argument("--eval-metric", default="mean_reward", choices=("mean_reward", "success_rate"),
                    help="with --eval-freq: what best_model.zip is the best by")
    a = ap.parse_args()

    import torch

    import drone2d_amd as d2
    from drone2d_amd.config import ENV_TRAIN_CONFIG
    from drone2d_amd.config import TEST_SCENARIOS
    from drone2d_amd.ppo import PPO, Checkpoint, Evaluation, PPOConfig

    torch.cuda.set_device(0)
    kw = dict(ENV_TRAIN_CONFIG, scenario=a.scenario)
    if a.curriculum:
        kw.update(mode="curriculum", scenario="curriculum", sim_num=0, curriculum_seed=a.seed)
        if a.pool > 0:  # a host-generated pool; --pool 0: every reset on a fresh device-generated scenario
            kw["curriculum_pool"] = a.pool
    if a.episode_steps is not None:
        kw["n_steps"] = a.episode_steps
    venv = d2.Drone2dVecEnv(a.envs, seed=a.seed, timeup_truncates=a.timeup_truncates, **kw)
    cfg = PPOConfig.gpu_defaults(n_steps=a.n_steps, batch_size=a.batch, n_epochs=a.epochs,
                                 learning_rate_end=a.lr_end, clip_range_end=a.clip_range_end,
                                 clip_range_vf=a.clip_range_vf, target_kl=a.target_kl, norm_reward=a.norm_reward,
                                 clip_reward=a.clip_reward)
    cfg.graph = not a.no_graph
    cfg.manual = not a.autograd
    # a resumed run takes its configuration, seed and env state from the file
    algo = PPO.load(a.resume, venv) if a.resume else PPO(venv, cfg, seed=a.seed)
    ckpt = None
    if a.checkpoint_every > 0:
        ck_dir = os.path.dirname(os.path.abspath(a.save)) if a.save else "ppo_agents"
        ckpt = Checkpoint(a.checkpoint_every, ck_dir)
    evaluation = None
    if a.eval_freq > 0:
        best_dir = os.path.dirname(os.path.abspath(a.save)) if a.save else a.log_dir
        evaluation = Evaluation(a.eval_freq, scenarios=tuple(a.eval_scenarios.split(",")) if a.eval_scenarios else
                                TEST_SCENARIOS, runs=a.eval_runs, seed=a.seed, metric=a.eval_metric, log_path=a.log_dir,
                                best_model_save_path=best_dir)
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    tag = ("_eager" if a.no_graph else "") + ("_autograd" if a.autograd else "") + ("_norm" if a.norm_reward else "") + \
          ("_trunc" if a.timeup_truncates else "")
    out = open(os.path.join(REPO, "gpurun_out", f"ppo{tag}.jsonl"), "w")
    logger = None
    if a.log_dir:
        import dataclasses

        from drone2d_amd.trainlog import ScalarLog

        logger = ScalarLog(a.log_dir, tensorboard=not a.no_tensorboard)
        logger.write_configs(kw, dataclasses.asdict(algo.cfg))
        algo.set_monitor(True)
    t0, steps0 = time.perf_counter(), algo.num_timesteps
    horizon = steps0 + a.updates * algo.cfg.n_steps * a.envs  # the schedules run over this call's updates
    for u in range(a.updates):
        if a.curriculum and a.pool > 0 and u and u % a.refresh == 0:
            # the reference's stage clock is the global step count (checkpoint names, :76-86)
            venv.refresh_curriculum(sim_num=algo.num_timesteps)
        rec = algo.learn(algo.num_timesteps + algo.cfg.n_steps * a.envs, checkpoint=ckpt, logger=logger,
                         schedule_timesteps=horizon, evaluation=evaluation)[-1]
        rec.update(update=u, wall_s=time.perf_counter() - t0)
        line = json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in rec.items()})
        print(line, flush=True)
        out.write(line + "\n")
    total = (algo.num_timesteps - steps0) / (time.perf_counter() - t0)
    if logger is not None:
        logger.close()
    print(json.dumps({"envs": a.envs, "updates": a.updates, "timesteps": algo.num_timesteps, "graph": algo.use_graph, "manual": algo.cfg.manual,
                      "env_steps_per_s_incl_learning": total}), flush=True)
    if a.save:
        print(json.dumps({"saved": algo.save(a.save)}), flush=True)
    venv.close()


if __name__ == "__main__":
    main()
