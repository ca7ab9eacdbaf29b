#!/usr/bin/env python3
"""What a disturbed evaluation costs per env step of the eager loop on one MI355X (a record, no threshold;
results: profiles/disturb/; DESIGN.md "Disturbances").

    python tools/disturb_probe.py [--envs 65536] [--steps 200] [--rounds 5] [--calls 200] [--draws 1048576]

Per batch size (corridor, the shipped agent, stochastic actions): the eager loop of ``evaluate_policy``
(``evaluate._fly``, ``--steps`` env steps, the end-of-run read-back included) without ``disturb``, with a
neutral ``Disturbance`` (the two launches and the split evaluation call, nothing to compute) and with every
stage on: one warm round, then ``--rounds`` runs each, the arms interleaved, reported as median (min - max)
microseconds per env step.  Then the two kernels alone: HIP events around ``--calls`` back-to-back calls of
``d2d_disturb_obs`` and of ``d2d_disturb_act``, neutral and with every stage on.  Then the normals: the
largest absolute difference between the device's Box-Muller and a float64 one over ``--draws`` draws of the
same uniforms.
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


def _all_on():
    from drone2d_amd.disturb import Disturbance

    return Disturbance(obs_sigma=0.02, act_sigma=0.05, sensor_dropout=0.1, motor_gain=(0.9, 1.0), act_delay=4)


def probe(n: int, a) -> dict:
    import torch

    import drone2d_amd as d2
    from drone2d_amd import evaluate
    from drone2d_amd.config import ENV_TEST_CONFIG
    from drone2d_amd.disturb import Disturbance, Disturber
    from drone2d_amd.ppo import ActorCritic

    policy = ActorCritic.from_agent_npz(AGENT).cuda()
    venv = d2.Drone2dVecEnv(n, seed=0, with_info=True, **dict(ENV_TEST_CONFIG, scenario="corridor"))
    ws = evaluate.actor_tensors(policy, venv.device)
    S = a.steps
    arms = {"plain": None, "neutral": Disturber(n, Disturbance(), device=venv.device),
            "all_stages": Disturber(n, _all_on(), device=venv.device)}

    def loop(arm):
        d = arms[arm]
        # a quarter-length plain run first, untimed: every timed loop then starts right after the same work
        evaluate._fly(venv, ws, None, False, 0, max(S // 4, 1), None, False, S + 1, "philox", False)
        torch.cuda.synchronize()
        if d is not None:
            d.reset()
        t0 = time.perf_counter()
        evaluate._fly(venv, ws, None, False, 0, S, None, False, S + 1, "philox", False, disturb=d)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / S

    times = {k: [] for k in arms}
    for r in range(a.rounds + 1):  # (round 0 warms)
        for k in arms:
            us = loop(k)
            if r:
                times[k].append(us)

    kernel = {}
    obs = venv.reset(seed=0)
    act = torch.rand(n, 2, device=venv.device) * 2 - 1
    for arm in ("neutral", "all_stages"):
        d = arms[arm]
        for call in ("obs", "act"):
            runs = []
            for r in range(a.rounds + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for t in range(a.calls):
                    d.obs(obs, t) if call == "obs" else d.act(act, t)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    runs.append(e0.elapsed_time(e1) * 1e3 / a.calls)
            kernel[f"d2d_disturb_{call}_{arm}"] = {"us_per_call": _stat(runs)}
    venv.close()
    return {"envs": n, "steps": S, "loop_us_per_env_step": {k: _stat(v) for k, v in times.items()}, "kernels": kernel}


def normals(draws: int) -> dict:
    """The device's normals against a float64 Box-Muller of the same uniforms: ``draws`` of them, the sensor
    stream's 28 per env (27 channels and the 28th through the actuator stream's pair)."""
    import numpy as np
    import torch

    from drone2d_amd import disturb as D

    n = (draws + 26) // 27
    seed = 0x0123456789ABCDEF
    d = D.Disturber(n, D.Disturbance(obs_sigma=1.0, act_sigma=1.0), device="cuda", seed=seed, keep_draws=True)
    d.obs(torch.zeros(n, 27, device="cuda"), 5)
    d.act(torch.zeros(n, 2, device="cuda"), 5)
    z_obs, z_act = d.z_obs.cpu().numpy().astype(np.float64), d.z_act.cpu().numpy().astype(np.float64)
    g = np.arange(n)

    def bm64(w, k):
        u0, u1 = D.uniforms(w[k]).astype(np.float64), D.uniforms(w[k + 1]).astype(np.float64)
        r, ang = np.sqrt(-2.0 * np.log(u0)), 2.0 * np.pi * u1
        return r * np.cos(ang), r * np.sin(ang)

    worst, worst_host = 0.0, 0.0
    host = D.HostDisturber(n, D.Disturbance(obs_sigma=1.0), seed=seed).obs_normals(5).astype(np.float64)
    for b in range(7):
        w = D.philox_words(seed, g, 5, D.TAG_OBS, b)
        ref = np.stack([*bm64(w, 0), *bm64(w, 2)], -1)[:, :min(4, 27 - 4 * b)]
        worst = max(worst, float(np.abs(z_obs[:, 4 * b:4 * b + 4] - ref).max()))
        worst_host = max(worst_host, float(np.abs(z_obs[:, 4 * b:4 * b + 4] - host[:, 4 * b:4 * b + 4]).max()))
    ref = np.stack(bm64(D.philox_words(seed, g, 5, D.TAG_ACT, 0), 0), -1)
    worst = max(worst, float(np.abs(z_act - ref).max()))
    return {"draws": int(z_obs.size + z_act.size), "max_abs_device_minus_float64": worst,
            "max_abs_device_minus_numpy_twin": worst_host, "largest_abs_normal": float(np.abs(z_obs).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[65536])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--draws", type=int, default=1 << 20)
    ap.add_argument("--out", default=None, help="result file (default: profiles/disturb/disturb_probe.json)")
    a = ap.parse_args()

    import torch

    torch.cuda.set_device(0)
    res = {"rounds": a.rounds, "calls": a.calls, "device": torch.cuda.get_device_name(0),
           "sizes": [probe(n, a) for n in a.envs], "normals": normals(a.draws)}
    path = a.out or os.path.join(REPO, "profiles", "disturb", "disturb_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
