#!/usr/bin/env python3
"""What reward normalisation costs per env step on one MI355X (a record, no threshold; results:
profiles/norm/; DESIGN.md "Reward normalisation").

    python tools/norm_probe.py [--envs 1000 65536] [--calls 200] [--rounds 5]

Per batch size: corridor, the batch flown ``--warm`` random steps with the normaliser attached, then HIP
events around ``--calls`` back-to-back ``d2d_norm_step`` calls (two launches each) on one real step's
outputs, ``training = 1`` and ``training = 0`` alternating: one warm round, then ``--rounds`` rounds,
reported as median (min - max) microseconds per call.  The algorithmic bytes per env-step are counted
from the shapes.  (The train-level numbers: ``tools/ppo_control_probe.py train --norm-reward``.)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# per env and step, training: rew read twice (each launch), ret read and written, then written again
# at episode ends only; term and trunc read; rew_out written
BYTES_PER_ENV_STEP = 4 + 8 + 8 + 4 + 1 + 1 + 4


def probe(n: int, a) -> dict:
    import torch

    import drone2d_amd as d2
    from drone2d_amd.config import ENV_TRAIN_CONFIG
    from drone2d_amd.normalize import RewardNormalizer

    venv = d2.Drone2dVecEnv(n, seed=0, **dict(ENV_TRAIN_CONFIG, scenario="corridor"))
    nz = RewardNormalizer(venv, 0.99)
    g = torch.Generator(device="cuda").manual_seed(0)
    venv.reset(seed=0)
    for _ in range(a.warm):
        _, rew, term, trunc, _ = venv.step(torch.rand(n, 2, device="cuda", generator=g) * 2 - 1)
        nz.step(rew, term, trunc)
    scale = float(nz.scale())

    def timed(training):
        nz.training = training
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            nz.step(rew, term, trunc)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls  # us per call

    on, off = [], []
    for r in range(a.rounds + 1):  # (round 0 warms)
        x, y = timed(True), timed(False)
        if r:
            on.append(x)
            off.append(y)
    venv.close()
    med = statistics.median(on)
    stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}  # noqa: E731
    return {"envs": n, "n_blocks": nz.n_blocks, "reward_scale_after_warm": scale,
            "d2d_norm_step_training_us": stat(on), "d2d_norm_step_eval_us": stat(off),
            "bytes_per_env_step": BYTES_PER_ENV_STEP, "bytes_per_call": BYTES_PER_ENV_STEP * n,
            "achieved_bytes_per_s": BYTES_PER_ENV_STEP * n / (med * 1e-6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[1000, 65536])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=64, help="env steps flown before the measured step")
    ap.add_argument("--out", default=None, help="result file (default: profiles/norm/kernel_probe.json)")
    a = ap.parse_args()

    import torch

    torch.cuda.set_device(0)
    res = {"calls": a.calls, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "launches_per_call": {"training": 2, "eval": 1}, "sizes": [probe(n, a) for n in a.envs]}
    path = a.out or os.path.join(REPO, "profiles", "norm", "kernel_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
