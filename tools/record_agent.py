#!/usr/bin/env python3
"""Test a saved agent and record its flights as GIFs: ``tools/test_agent.py`` with ``--gif``, GPU box.

    python tools/record_agent.py AGENT.zip [every option of tools/test_agent.py]
                                 [--gif K [--gif-size N] [--gif-hud]]

One command for the reference's whole test mode (main.py:220-327): it runs ``tools/test_agent.py``'s own
``main()`` on the command line it was given (results.txt, the ``.npy`` arrays, ``--flight-paths``; that tool's
parser, defaults and output, not restated here) and then, with ``--gif K`` (default 0: nothing more happens and
nothing new is loaded), records the first episode of K envs per scenario through ``harness.record_gifs``:
``<out>/Gifs/<agent>/<scenario>.gif`` (``<scenario>_<k>.gif`` for K > 1), every second frame, 30 fps, rendered
at ``--gif-size`` (default 256) and encoded on the device, with the text overlay, arcs and shades under
``--gif-hud``.  One more JSON line per scenario.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, TOOLS)
sys.path.insert(0, os.path.dirname(TOOLS))


def main():
    import test_agent  # tools/test_agent.py
    from drone2d_amd.config import TEST_SCENARIOS

    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--gif", type=int, default=0, metavar="K")
    ap.add_argument("--gif-size", type=int, default=256)
    ap.add_argument("--gif-hud", action="store_true")
    g, rest = ap.parse_known_args()
    if "-h" in rest or "--help" in rest:
        print(__doc__)
    sys.argv = [sys.argv[0], *rest]
    test_agent.main()
    if g.gif < 1:
        return
    # what the GIFs share with the test run, read off the same command line
    sh = argparse.ArgumentParser(add_help=False)
    sh.add_argument("agent")
    sh.add_argument("--scenarios", default=",".join(TEST_SCENARIOS))
    sh.add_argument("--seed", type=int, default=0)
    sh.add_argument("--deterministic", action="store_true")
    sh.add_argument("--out", default=None)
    a, _ = sh.parse_known_args(rest)

    import drone2d_amd as d2
    from drone2d_amd import harness
    from drone2d_amd.config import ENV_TEST_CONFIG
    from drone2d_amd.ppo import ActorCritic

    policy = ActorCritic.from_sb3_zip(a.agent).cuda()
    name = os.path.splitext(os.path.basename(a.agent))[0]
    out_dir = a.out or os.path.join("Tests", name)
    for scn in a.scenarios.split(","):
        t0 = time.perf_counter()
        venv = d2.Drone2dVecEnv(g.gif, seed=a.seed, with_info=True, **dict(ENV_TEST_CONFIG, scenario=scn))
        gifs = harness.record_gifs(venv, policy, out_dir, scn, name, env_ids=range(g.gif), seed=a.seed,
                                   deterministic=a.deterministic, size=g.gif_size, hud=g.gif_hud)
        venv.close()
        print(json.dumps({"scenario": scn, "gifs": gifs, "bytes": [os.path.getsize(p) for p in gifs],
                          "seconds": round(time.perf_counter() - t0, 3)}), flush=True)


if __name__ == "__main__":
    main()
