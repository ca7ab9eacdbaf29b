#!/usr/bin/env python
"""Times the evaluation loop eager against replayed as a captured HIP graph: a record for DESIGN.md
"The replayed loop" and the measurement ``train_eval.GRAPH_PAYS`` is set from, not a gate.

Arms, on identically built batches (one batch per arm, kept over the rounds), each a whole evaluation to
the last env's first episode end, the host clock around the call (it ends in a read-back):
  eager   evaluate_policy(graph=False): one d2d_eval_step + one d2d_step per env step, launched from Python
  graph   evaluate_policy(graph=True): a throw-away EvalLoop -- warm segment, capture, replays, tail
  loop    EvalLoop.run on a loop kept over the rounds (what PPO.learn(evaluation=...) flies): replays only
Sizes: 896 envs (the seven test scenarios x 128 runs, deterministic, the shipped agent) and 65 536
corridor envs.  One warm run per arm, then --reps rounds alternating the arms; seconds and us per env
step (steps = the longest episode) as median (min - max).  ``graph_pays``: at 896 envs the graph arm's
median below the eager arm's minimum.

With --train: tools/train_ppo.py at 65 536 envs, 30 updates, without and with --eval-freq set to every 5
updates, each in a process of its own; ``eval/seconds`` next to ``rollout_s + train_s``.

    python tools/eval_graph_probe.py [--reps 5] [--train] [--out profiles/eval/eval_graph_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
AGENT = os.path.join(REPO, "tests", "golden", "agent_17_90.npz")


def _stat(v) -> dict:
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def time_arms(runs: dict, reps: int) -> dict:
    """Each arm once warm, then ``reps`` rounds alternating the arms; every run returns its env steps."""
    import torch

    for run in runs.values():
        run()
    sec, us = {k: [] for k in runs}, {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = run()
            dt = time.perf_counter() - t0
            sec[k].append(dt)
            us[k].append(dt * 1e6 / steps)
    return {k: {"seconds": _stat(sec[k]), "us_per_env_step": _stat(us[k]), "env_steps": steps} for k in runs}


def train_record(updates: int = 30, every: int = 5, envs: int = 65536, n_steps: int = 16) -> dict:
    out = {}
    for arm, extra in (("plain", []), ("evaluating", ["--eval-freq", str(every * envs * n_steps)])):
        cmd = [sys.executable, os.path.join(REPO, "tools", "train_ppo.py"), "--envs", str(envs), "--updates",
               str(updates), "--n-steps", str(n_steps), *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode:
            raise SystemExit(f"train_ppo.py failed ({p.returncode}):\n{p.stderr[-2000:]}")
        recs = [json.loads(line) for line in p.stdout.splitlines() if line.startswith('{"episodes"')]
        ev = [r["eval/seconds"] for r in recs if "eval/seconds" in r]
        out[arm] = {"updates": len(recs), "rollout_plus_train_s": float(sum(r["rollout_s"] + r["train_s"] for r in recs)),
                    "rollout_plus_train_s_per_update": _stat([r["rollout_s"] + r["train_s"] for r in recs[2:]]),
                    "wall_s": recs[-1]["wall_s"], "evaluations": len(ev), "eval_seconds": ev,
                    "eval_success_rate": [r["eval/success_rate"] for r in recs if "eval/seconds" in r]}
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="896,65536")
    ap.add_argument("--train", action="store_true", help="also the train_ppo.py record (two child processes)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval", "eval_graph_probe.json"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("eval_graph_probe needs a HIP device")
    import drone2d_amd as d2
    from drone2d_amd import evaluate
    from drone2d_amd.config import ENV_TEST_CONFIG, TEST_SCENARIOS
    from drone2d_amd.ppo import ActorCritic

    torch.cuda.set_device(0)
    pol = ActorCritic.from_agent_npz(AGENT).cuda()
    record = {"reps": args.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        if n == 896:
            es = evaluate.sweep_layout(1, len(TEST_SCENARIOS), 128)[1]
            kw, det = dict(ENV_TEST_CONFIG, scenario=list(TEST_SCENARIOS)), True
        else:
            es, kw, det = None, dict(ENV_TEST_CONFIG, scenario="corridor"), False
        venvs = {k: d2.Drone2dVecEnv(n, seed=0, with_info=True, env_scenario=es, **kw) for k in ("eager", "graph", "loop")}
        loop = evaluate.EvalLoop(venvs["loop"], pol, deterministic=det, graph=True)

        def steps_of(m):
            return int(m["time_spent"].max())

        def run_loop():
            fin, rows, _, nobs, _, _ = loop.run(0)
            return steps_of(evaluate._records(venvs["loop"], fin, rows, None, nobs))

        runs = {"eager": lambda: steps_of(evaluate.evaluate_policy(venvs["eager"], pol, deterministic=det, seed=0)),
                "graph": lambda: steps_of(evaluate.evaluate_policy(venvs["graph"], pol, deterministic=det, seed=0,
                                                                   graph=True)),
                "loop": run_loop}
        res = time_arms(runs, args.reps)
        res["captures_of_the_kept_loop"] = loop.captures
        if n == 896:
            res["graph_pays"] = bool(res["graph"]["seconds"]["median"] < res["eager"]["seconds"]["min"])
            res["kept_loop_pays"] = bool(res["loop"]["seconds"]["median"] < res["eager"]["seconds"]["min"])
        for v in venvs.values():
            v.close()
        record["sizes"][str(n)] = res
        print(json.dumps({"envs": n, **res}), flush=True)
    if args.train:
        record["train_65536x30"] = train_record()
        print(json.dumps(record["train_65536x30"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
