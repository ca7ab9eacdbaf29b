#!/usr/bin/env python3
"""The measurements of DESIGN.md "PPO control" (one MI355X; a record, the only bar is on `train`'s
default path).

    python tools/ppo_control_probe.py train [--parent-tree DIR [--parent-control]] [--norm-reward] [--runs 5] [--updates 30]
    python tools/ppo_control_probe.py stop  [--rounds 7]

``train``: DESIGN.md "Monitor"'s protocol -- ``tools/train_ppo.py``, 65 536 corridor envs, 30 updates, a
fresh process per run, the median env-steps/s over the updates after the graph captures (update >= 3)
-- for this tree's default path, this tree with ``--target-kl inf`` (the control path, never stopping)
and, with ``--parent-tree``, the parent commit's built tree (``--parent-control``: that tree with
``--target-kl inf`` as well), alternating in one call.  ``--norm-reward`` (DESIGN.md "Reward normalisation"):
the control arm is replaced by this tree with ``--norm-reward``, and the rollout's seconds are kept too.
``stop``: one captured update of the headline configuration (320 minibatch steps) that runs in full
against one that stops at its first minibatch (``target_kl = -1``), the same graph replayed.
Results: ``profiles/ppo_control/<mode>_probe.json`` (``--out``).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("parent", "parent_control", "default", "control", "norm")


def _train_run(tree: str, a, extra=()) -> dict:
    cmd = [sys.executable, os.path.join(tree, "tools", "train_ppo.py"), "--envs", str(a.envs), "--updates",
           str(a.updates), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr[-3000:]}")
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    upd = [x for x in recs if "update" in x]
    steady = [x["env_steps_per_s"] for x in upd if x["update"] >= 3]
    out = {"whole_run": recs[-1]["env_steps_per_s_incl_learning"], "steady_median": statistics.median(steady),
           "train_s_median": statistics.median(x["train_s"] for x in upd if x["update"] >= 3),
           "rollout_s_median": statistics.median(x["rollout_s"] for x in upd if x["update"] >= 3)}
    if "approx_kl" in upd[-1]:
        out["last_approx_kl"], out["last_n_minibatches"] = upd[-1]["approx_kl"], upd[-1]["n_minibatches"]
    return out


def train_probe(a) -> dict:
    out = {"envs": a.envs, "updates": a.updates, "runs": a.runs, "default": [], "control": [], "parent": [],
           "parent_control": [], "norm": []}
    _train_run(REPO, a)  # a first run nobody counts: the box's caches
    for k in range(a.runs):
        if a.parent_tree:
            out["parent"].append(_train_run(os.path.abspath(a.parent_tree), a))
        if a.parent_tree and a.parent_control:
            out["parent_control"].append(_train_run(os.path.abspath(a.parent_tree), a, ("--target-kl", "inf")))
        out["default"].append(_train_run(REPO, a))
        if a.norm_reward:
            out["norm"].append(_train_run(REPO, a, ("--norm-reward",)))
        else:
            out["control"].append(_train_run(REPO, a, ("--target-kl", "inf")))
        print(json.dumps({"run": k, **{n: out[n][-1] for n in ARMS if out[n]}}), flush=True)
    for key in ("whole_run", "steady_median", "train_s_median", "rollout_s_median"):
        out[key] = {}
        for n in ARMS:
            v = [x[key] for x in out[n]]
            if v:
                out[key].update({n + "_median": statistics.median(v), n + "_min": min(v), n + "_max": max(v)})
        for n in ("control", "norm"):
            if out[n]:
                out[key][n + "_over_default"] = out[key][n + "_median"] / out[key]["default_median"]
        if a.parent_tree:
            out[key]["default_inside_parent_spread"] = (out[key]["parent_min"] <= out[key]["default_median"]
                                                        <= out[key]["parent_max"])
        if out["parent_control"]:
            out[key]["control_inside_parent_spread"] = (out[key]["parent_control_min"] <= out[key]["control_median"]
                                                        <= out[key]["parent_control_max"])
    return out


def stop_probe(a) -> dict:
    import torch

    sys.path.insert(0, REPO)
    import drone2d_amd as d2
    from drone2d_amd.config import ENV_TRAIN_CONFIG
    from drone2d_amd.ppo import PPO, PPOConfig

    torch.cuda.set_device(0)
    venv = d2.Drone2dVecEnv(a.envs, seed=0, **dict(ENV_TRAIN_CONFIG, scenario="corridor"))
    algo = PPO(venv, PPOConfig.gpu_defaults(target_kl=float("inf")), seed=0)
    for _ in range(3):  # eager, capture, replay
        algo.collect_rollouts()
        algo.train()
    assert algo._graph is not None
    full, stopped, recs = [], [], {}
    for _ in range(a.rounds):
        for name, tkl, ts in (("full", float("inf"), full), ("stopped", -1.0, stopped)):
            algo.cfg.target_kl = tkl
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            recs[name] = algo.train()  # ends with the record's device-to-host copy
            ts.append(time.perf_counter() - t0)
    venv.close()
    assert recs["stopped"]["n_minibatches"] == 1 and recs["stopped"]["early_stop"] == 1
    assert recs["full"]["early_stop"] == 0
    n = recs["full"]["n_minibatches"]
    res = {"envs": a.envs, "planned_minibatches": n, "rounds": a.rounds,
           "full_s": {"median": statistics.median(full), "min": min(full), "max": max(full)},
           "stopped_s": {"median": statistics.median(stopped), "min": min(stopped), "max": max(stopped)}}
    res["skipped_minibatch_us"] = 1e6 * res["stopped_s"]["median"] / n
    res["full_minibatch_us"] = 1e6 * res["full_s"]["median"] / n
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["train", "stop"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-control", action="store_true", help="also run the parent tree with --target-kl inf")
    ap.add_argument("--norm-reward", action="store_true", help="train: this tree with --norm-reward in place of the control arm")
    ap.add_argument("--out", default=None, help="result file (default: profiles/ppo_control/<mode>_probe.json)")
    a = ap.parse_args()
    res = train_probe(a) if a.mode == "train" else stop_probe(a)
    path = a.out or os.path.join(REPO, "profiles", "ppo_control", f"{a.mode}_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
