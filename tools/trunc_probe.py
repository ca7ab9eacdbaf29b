#!/usr/bin/env python3
"""The measurements of DESIGN.md "Truncation bootstrap" (one MI355X; a record, the only bar is on the
default path).

    python tools/trunc_probe.py [--parent-tree DIR] [--rounds 3] [--updates 30] [--episode-steps 64]

DESIGN.md "Monitor"'s protocol -- ``tools/train_ppo.py``, 65 536 corridor envs, 16-step rollouts, 30
updates, a fresh process per run, medians over the updates after the graph captures (update >= 3) -- for
these arms, alternating in one call:

    default        this tree, no flag (time-up is terminal: d2d_ppo_rollout_step)
    trunc          this tree, --timeup-truncates (d2d_ppo_rollout_step_tb)
    default_short  this tree, --episode-steps K
    trunc_short    this tree, --timeup-truncates --episode-steps K: time-ups inside the timed window
    parent, parent_trunc, parent_trunc_short   with --parent-tree: the parent commit's built tree; its
                   tool has no flag, so its truncating runs go through this file's ``--shim`` mode, which
                   runs that tree's tools/train_ppo.py with the batch built with timeup_truncates=True (the
                   parent then takes the torch rollout)

With the default 1 100-step limit no env times out within 30 x 16 steps, so ``trunc`` measures the new
instantiation with the second pass never taken, ``trunc_short`` (K = 64: every env times out in every
fourth rollout at the latest) with it taken.  Results: ``profiles/trunc_bootstrap/train_probe.json`` (``--out``).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("whole_run", "steady_median", "train_s_median", "rollout_s_median")


def shim(tree: str, episode_steps: int, argv: list):
    """A tree's tools/train_ppo.py with every Drone2dVecEnv built truncating (and, with episode_steps > 0,
    with that time limit)."""
    import runpy

    sys.path.insert(0, tree)
    import drone2d_amd as d2

    real = d2.Drone2dVecEnv

    def make(*a, **kw):
        kw["timeup_truncates"] = True
        if episode_steps > 0:
            kw["n_steps"] = episode_steps
        return real(*a, **kw)

    d2.Drone2dVecEnv = make
    tool = os.path.join(tree, "tools", "train_ppo.py")
    sys.argv = [tool, *argv]
    runpy.run_path(tool, run_name="__main__")


def _run(tree: str, a, extra=(), shim_steps=None) -> dict:
    base = ["--envs", str(a.envs), "--updates", str(a.updates), "--n-steps", "16"]
    if shim_steps is None:
        cmd = [sys.executable, os.path.join(tree, "tools", "train_ppo.py"), *base, *extra]
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--shim", tree, "--shim-steps", str(shim_steps), "--", *base]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr[-3000:]}")
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    upd = [x for x in recs if "update" in x and x["update"] >= 3]
    return {"whole_run": recs[-1]["env_steps_per_s_incl_learning"],
            "steady_median": statistics.median(x["env_steps_per_s"] for x in upd),
            "train_s_median": statistics.median(x["train_s"] for x in upd),
            "rollout_s_median": statistics.median(x["rollout_s"] for x in upd),
            "episodes": sum(x["episodes"] for x in upd)}


def probe(a) -> dict:
    K = str(a.episode_steps)
    arms = {"default": (REPO, (), None), "trunc": (REPO, ("--timeup-truncates",), None),
            "default_short": (REPO, ("--episode-steps", K), None),
            "trunc_short": (REPO, ("--timeup-truncates", "--episode-steps", K), None)}
    if a.parent_tree:
        p = os.path.abspath(a.parent_tree)
        arms = {"parent": (p, (), None), "parent_trunc": (p, (), 0), "parent_trunc_short": (p, (), a.episode_steps),
                **arms}
    out = {"envs": a.envs, "updates": a.updates, "rounds": a.rounds, "episode_steps": a.episode_steps,
           "runs": {n: [] for n in arms}}
    _run(REPO, a)  # a first run nobody counts: the box's caches
    for k in range(a.rounds):
        for n, (tree, extra, steps) in arms.items():
            out["runs"][n].append(_run(tree, a, extra, steps))
        print(json.dumps({"round": k, **{n: out["runs"][n][-1] for n in arms}}), flush=True)
    for key in KEYS:
        out[key] = {}
        for n in arms:
            v = [x[key] for x in out["runs"][n]]
            out[key].update({n + "_median": statistics.median(v), n + "_min": min(v), n + "_max": max(v)})
        out[key]["trunc_over_default"] = out[key]["trunc_median"] / out[key]["default_median"]
        out[key]["trunc_short_over_default_short"] = out[key]["trunc_short_median"] / out[key]["default_short_median"]
        if a.parent_tree:
            out[key]["trunc_over_parent_trunc"] = out[key]["trunc_median"] / out[key]["parent_trunc_median"]
            out[key]["trunc_short_over_parent_trunc_short"] = (out[key]["trunc_short_median"] /
                                                               out[key]["parent_trunc_short_median"])
            out[key]["default_inside_parent_spread"] = (out[key]["parent_min"] <= out[key]["default_median"]
                                                        <= out[key]["parent_max"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--episode-steps", type=int, default=64)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None, help="result file (default: profiles/trunc_bootstrap/train_probe.json)")
    ap.add_argument("--shim", default=None, metavar="TREE", help="(internal) run TREE's train_ppo.py on a truncating batch")
    ap.add_argument("--shim-steps", type=int, default=0)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_args()
    if a.shim:
        return shim(os.path.abspath(a.shim), a.shim_steps, a.rest)
    res = probe(a)
    path = a.out or os.path.join(REPO, "profiles", "trunc_bootstrap", "train_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in KEYS}), flush=True)


if __name__ == "__main__":
    main()
