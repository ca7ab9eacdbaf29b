#!/usr/bin/env python3
"""Test a saved agent on the test scenarios and draw its arena maps, GPU box.

    python tools/map_agent.py AGENT.zip [--maps GRID] [--scenarios corridor,large] [--envs 1000] [--seed 0]
                              [--deterministic] [--flight-paths] [--out DIR]

tools/test_agent.py with the arena maps switched on: the same agent files, the same loop
(``evaluate_policy``, one batch of ``--envs`` first episodes per scenario), the same per-scenario files in
the same places (``--out``, default Tests/<agent file name>/<scenario>/), and next to them ``maps.npz``
(the six planes and their ``outside`` counters, GRID x GRID cells, default 64) and the pictures
``plots/<scenario>_density.png``, ``_spawn_success.png`` and ``_crashes.png``: where the agent flies, its
success rate by spawn cell, and where it crashes.  The maps are binned on the device while the episodes
fly (``drone2d_amd.heatmap``); every other file is byte for byte what test_agent.py writes.  One JSON line
per scenario.
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
    from drone2d_amd.config import TEST_SCENARIOS

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("agent")
    ap.add_argument("--maps", type=int, default=64, metavar="GRID", help="cells a side (1 .. 256)")
    ap.add_argument("--scenarios", default=",".join(TEST_SCENARIOS))
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--flight-paths", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("map_agent needs a HIP device")
    import drone2d_amd as d2
    from drone2d_amd import harness
    from drone2d_amd.config import ENV_TEST_CONFIG
    from drone2d_amd.evaluate import evaluate_policy
    from drone2d_amd.ppo import ActorCritic

    torch.cuda.set_device(0)
    policy = ActorCritic.from_sb3_zip(a.agent).cuda()
    name = os.path.splitext(os.path.basename(a.agent))[0]
    out_dir = a.out or os.path.join("Tests", name)
    for scn in a.scenarios.split(","):
        t0 = time.perf_counter()
        venv = d2.Drone2dVecEnv(a.envs, seed=a.seed, with_info=True, **dict(ENV_TEST_CONFIG, scenario=scn))
        m = evaluate_policy(venv, policy, deterministic=a.deterministic, seed=a.seed, flight_paths=a.flight_paths,
                            maps=a.maps)
        venv.close()
        s = harness.write_results(m, os.path.join(out_dir, scn), scn, name, os.path.abspath(a.agent))
        r = m["maps"]
        print(json.dumps(dict(s, scenario=scn, unfinished=m["unfinished"], grid=a.maps,
                              steps_binned=int(r["planes"][0].sum()) + int(r["outside"][0]),
                              seconds=round(time.perf_counter() - t0, 3))), flush=True)


if __name__ == "__main__":
    main()
