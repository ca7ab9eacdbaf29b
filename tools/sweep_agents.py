#!/usr/bin/env python3
"""Test several saved agents on the test scenarios in one batch (choosing a checkpoint), GPU box.

    python tools/sweep_agents.py A.zip B.zip ... | CHECKPOINT_DIR [--scenarios corridor,large] [--envs 1000]
                                 [--seed 0] [--deterministic] [--flight-paths] [--maps [GRID]] [--out DIR]

The many-agent companion of tools/test_agent.py, with its options.  The agents are zips (as test_agent.py
takes them) and / or directories of ``rl_model_<steps>_steps.zip`` checkpoints, each taken in step order.
All agents fly every scenario in ONE batch of agents x scenarios x ``--envs`` envs (``evaluate.sweep``: one
launch of the policy bank per env step); every (agent, scenario, run) is an env of its own, with its own
spawn and noise draws.  Every agent's per-scenario files -- what test_agent.py writes
(``harness.write_results``) -- go to ``--out``/<agent file name>/<scenario>/ (default
Tests/<agent file name>/<scenario>/, where test_agent.py puts them by default) and the agent-by-scenario
table to ``selection.csv`` / ``selection.json`` under ``--out`` (default Tests/).  One JSON line per
(agent, scenario).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def checkpoint_zips(directory: str) -> list:
    """The ``<prefix>_<steps>_steps.zip`` files of ``directory``, in step order."""
    found = []
    for f in os.listdir(directory):
        m = re.fullmatch(r".*_(\d+)_steps\.zip", f)
        if m:
            found.append((int(m.group(1)), f))
    if not found:
        raise SystemExit(f"{directory}: no <prefix>_<steps>_steps.zip files")
    return [os.path.join(directory, f) for _, f in sorted(found)]


def agent_paths(args: list) -> list:
    """The zips the command line names: a directory stands for its checkpoints."""
    return [p for a in args for p in (checkpoint_zips(a) if os.path.isdir(a) else [a])]


def main():
    from drone2d_amd.config import TEST_SCENARIOS

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("agents", nargs="+", help="agent zips and / or directories of checkpoint zips")
    ap.add_argument("--scenarios", default=",".join(TEST_SCENARIOS))
    ap.add_argument("--envs", type=int, default=1000, help="runs per (agent, scenario)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--flight-paths", action="store_true")
    ap.add_argument("--maps", type=int, nargs="?", const=64, default=None, metavar="GRID",
                    help="bin every (agent, scenario)'s episodes into arena maps of GRID x GRID cells (default 64)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--graph", action="store_true", help="replay the sweep's loop as a captured HIP graph (same results)")
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("sweep_agents needs a HIP device")
    from drone2d_amd import evaluate, harness

    torch.cuda.set_device(0)
    paths = agent_paths(a.agents)
    names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    if len(set(names)) != len(names):
        raise SystemExit("agent file names must differ: they name the output directories")
    scns = a.scenarios.split(",")
    out_root = a.out or "Tests"
    t0 = time.perf_counter()
    bank = evaluate.PolicyBank(paths, names=names, device=torch.device("cuda", 0))
    res = evaluate.sweep(bank, scns, a.envs, seed=a.seed, deterministic=a.deterministic, flight_paths=a.flight_paths,
                         graph=a.graph, maps=a.maps)
    seconds = round(time.perf_counter() - t0, 3)
    for name, path in zip(names, paths):
        for scn in scns:
            m = res[name][scn]
            s = harness.write_results(m, os.path.join(out_root, name, scn), scn, name, os.path.abspath(path))
            print(json.dumps(dict(s, agent=name, scenario=scn, unfinished=m["unfinished"], sweep_seconds=seconds)),
                  flush=True)
    harness.write_selection(res, out_root)


if __name__ == "__main__":
    main()
