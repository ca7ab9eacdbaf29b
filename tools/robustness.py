#!/usr/bin/env python3
"""How much disturbance saved agents can take: one robustness curve per agent and scenario, GPU box.

    python tools/robustness.py A.zip [B.zip ... | CHECKPOINT_DIR] [--scenarios corridor,large] [--runs 1000]
                               --obs-sigma 0 0.01 0.02 0.05 | --act-sigma ... | --sensor-dropout ... |
                               --act-delay 0 2 4 8 | --motor-gain-left 1 0.9 0.8 | --motor-gain-right ...
                               [--seed 0] [--deterministic] [--out DIR]

One parameter is swept per call: the option that is given several values.  The others are held at the single
value they are given (default: the nominal world).  Every agent flies every scenario under every level in
ONE batch of agents x scenarios x levels x ``--runs`` envs (``evaluate.sweep(..., disturb=levels)``: the policy
bank and two small disturbance launches per env step); every (agent, scenario, level, run) is an env of its
own, with its own spawn and noise draws.  The agents are zips and / or directories of checkpoints, as
tools/sweep_agents.py takes them.  Writes ``robustness.csv`` / ``robustness.json``
(``harness.write_robustness``) under ``--out`` (default Tests/) and prints one JSON line per row.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# option -> (its neutral value, its type)
PARAMS = {"obs_sigma": (0.0, float), "act_sigma": (0.0, float), "sensor_dropout": (0.0, float),
          "act_delay": (0, int), "motor_gain_left": (1.0, float), "motor_gain_right": (1.0, float)}


def levels_from(a) -> list:
    """The levels the options name: the swept option's values, the others held."""
    from drone2d_amd.disturb import Disturbance

    swept = [k for k in PARAMS if len(getattr(a, k)) > 1]
    if len(swept) > 1:
        raise SystemExit("one swept parameter per call: " + ", ".join("--" + k.replace("_", "-") for k in swept) +
                         " all have several values")
    key = swept[0] if swept else None
    out = []
    for v in (getattr(a, key) if key else [None]):
        p = {k: (v if k == key else getattr(a, k)[0]) for k in PARAMS}
        out.append(Disturbance(p["obs_sigma"], p["act_sigma"], p["sensor_dropout"],
                               (p["motor_gain_left"], p["motor_gain_right"]), p["act_delay"],
                               name=f"{key}={v}" if key else "held"))
    return out


def main():
    from sweep_agents import agent_paths

    from drone2d_amd.config import TEST_SCENARIOS

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("agents", nargs="+", help="agent zips and / or directories of checkpoint zips")
    ap.add_argument("--scenarios", default=",".join(TEST_SCENARIOS))
    ap.add_argument("--runs", type=int, default=1000, help="runs per (agent, scenario, level)")
    for k, (neutral, kind) in PARAMS.items():
        ap.add_argument("--" + k.replace("_", "-"), type=kind, nargs="+", default=[neutral], metavar="V",
                        help=f"one value to hold, several to sweep (default {neutral})")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        levels = levels_from(a)
    except ValueError as e:
        raise SystemExit(str(e))

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("robustness needs a HIP device")
    from drone2d_amd import evaluate, harness

    torch.cuda.set_device(0)
    paths = agent_paths(a.agents)
    names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    if len(set(names)) != len(names):
        raise SystemExit("agent file names must differ: they name the rows")
    t0 = time.perf_counter()
    bank = evaluate.PolicyBank(paths, names=names, device=torch.device("cuda", 0))
    res = evaluate.sweep(bank, a.scenarios.split(","), a.runs, seed=a.seed, deterministic=a.deterministic, disturb=levels)
    seconds = round(time.perf_counter() - t0, 3)
    for row in harness.write_robustness(a.out or "Tests", res, levels):
        print(json.dumps(dict(zip(harness.ROBUSTNESS_COLUMNS, row), sweep_seconds=seconds)), flush=True)


if __name__ == "__main__":
    main()
