#!/usr/bin/env python3
"""What the arena maps cost per env step of the eager evaluation loop on one MI355X (a record, no
threshold; results: profiles/heat/; DESIGN.md "Arena maps").

    python tools/heat_probe.py [--envs 4096 65536] [--steps 200] [--rounds 5] [--grid 64]

Per batch size (corridor, the shipped agent, stochastic actions): the eager loop of ``evaluate_policy``
(``evaluate._fly``, ``--steps`` env steps, the end-of-run read-back included) without maps, with
``maps=GRID`` and with ``flight_paths=True``: one warm run, then ``--rounds`` runs each, the variants
interleaved, reported as median (min - max) microseconds per env step, with the peak device memory each
variant adds over the batch itself.  Then the step kernel alone: HIP events around ``--calls``
back-to-back ``d2d_heat_step`` calls on the table path and on the global path, on two inputs: the outputs
of the first env step after a reset (every env still inside the spawn rectangle, which covers some 470
cells of a 64 x 64 grid) and the same outputs with every position moved into one cell (the most contended
input there is).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
AGENT = os.path.join(REPO, "tests", "golden", "agent_17_90.npz")


def _stat(v) -> dict:
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def probe(n: int, a) -> dict:
    import torch

    import drone2d_amd as d2
    from drone2d_amd import evaluate, heatmap
    from drone2d_amd.config import ENV_TEST_CONFIG
    from drone2d_amd.ppo import ActorCritic

    policy = ActorCritic.from_agent_npz(AGENT).cuda()
    venv = d2.Drone2dVecEnv(n, seed=0, with_info=True, **dict(ENV_TEST_CONFIG, scenario="corridor"))
    ws = evaluate.actor_tensors(policy, venv.device)
    S = a.steps

    def loop(variant):
        am = heatmap.ArenaMaps(venv, a.grid, cap=S) if variant == "maps" else None
        # a quarter-length plain run first, untimed: every timed loop then starts right after the same work
        # (the previous variant ends in a read-back of its own size, during which the device idles)
        evaluate._fly(venv, ws, None, False, 0, max(S // 4, 1), None, False, S + 1, "philox", False)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        evaluate._fly(venv, ws, None, False, 0, S, None, variant == "flight_paths", S + 1, "philox", False, maps=am)
        if am is not None:
            am.counts()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt * 1e6 / S, torch.cuda.max_memory_allocated() - base

    variants = ("plain", "maps", "flight_paths")
    times = {v: [] for v in variants}
    mem = {}
    for r in range(a.rounds + 1):  # (round 0 warms)
        for v in variants:
            us, extra = loop(v)
            mem[v] = extra
            if r:
                times[v].append(us)

    # the kernel alone, on the first step's outputs and on the same with every env in one cell
    kernel = {}
    obs0 = venv.reset(seed=0)
    act = torch.zeros(n, 2, device=venv.device)
    obs, _, term, trunc, info = venv.step(act)
    hot = obs.clone()
    hot[:, 6:8] = hot[0, 6:8].clone()
    inputs = (("spawn", obs), ("one_cell", hot))
    for name, path, x in [(f"{p}_{i}", path, x) for p, path in (("table", heatmap.PATH_LDS), ("global", heatmap.PATH_GLOBAL))
                          for i, x in inputs]:
        obs = x
        am = heatmap.ArenaMaps(venv, a.grid, cap=a.calls * (a.rounds + 2), path=path)
        am.begin(obs0)
        runs = []
        for r in range(a.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.calls):
                am.step(obs, term, trunc, venv.terminal_obs, info)
            e1.record()
            torch.cuda.synchronize()
            if r:
                runs.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        c = am.counts()["planes"][0, heatmap.VISIT]
        kernel[name] = {"us_per_call": _stat(runs), "cells_hit": int((c > 0).sum())}
        am.close()
    venv.close()
    return {"envs": n, "steps": S, "grid": a.grid, "loop_us_per_env_step": {v: _stat(times[v]) for v in variants},
            "peak_device_bytes_added": mem, "d2d_heat_step": kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--out", default=None, help="result file (default: profiles/heat/heat_probe.json)")
    a = ap.parse_args()

    import torch

    torch.cuda.set_device(0)
    res = {"rounds": a.rounds, "calls": a.calls, "device": torch.cuda.get_device_name(0),
           "sizes": [probe(n, a) for n in a.envs]}
    path = a.out or os.path.join(REPO, "profiles", "heat", "heat_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
