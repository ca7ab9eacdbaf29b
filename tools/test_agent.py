#!/usr/bin/env python3
"""Test a saved agent on the test scenarios (the reference's ``mode == "test"``, main.py:220-327), GPU box.

    python tools/test_agent.py AGENT.zip [--scenarios corridor,large] [--envs 1000] [--seed 0]
                               [--deterministic] [--flight-paths] [--out DIR]

AGENT.zip: a file written by ``PPO.save`` / ``tools/train_ppo.py --save`` or by SB3's ``PPO.save`` (any zip
with a ``policy.pth``).  Every scenario runs ``--envs`` first episodes in one batch through
``evaluate_policy`` (stochastic actions by default, as the reference's ``model.predict(obs)``) and
writes the reference's per-scenario files (``<scenario>_<agent>_results.txt``, collisions / rewards /
apes / time_spent ``.npy``; with ``--flight-paths`` the ``flight_paths`` JSON and the overview plot)
under ``--out`` (default Tests/<agent file name>/ in the working directory, the reference's layout), one
directory per scenario.  One JSON line per scenario.
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
    ap.add_argument("--scenarios", default=",".join(TEST_SCENARIOS))
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--flight-paths", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("test_agent needs a HIP device")
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
        m = evaluate_policy(venv, policy, deterministic=a.deterministic, seed=a.seed, flight_paths=a.flight_paths)
        venv.close()
        s = harness.write_results(m, os.path.join(out_dir, scn), scn, name, os.path.abspath(a.agent))
        print(json.dumps(dict(s, scenario=scn, unfinished=m["unfinished"], seconds=round(time.perf_counter() - t0, 3))),
              flush=True)


if __name__ == "__main__":
    main()
