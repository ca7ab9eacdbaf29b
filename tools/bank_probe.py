#!/usr/bin/env python
"""Times the policy bank on the device: a record for DESIGN.md "Policy bank", not a gate.

Launch alone (HIP events around --calls back-to-back launches, record + act halves on a real env step's
outputs, stochastic), at 1 000 and 65 536 rows, after one warm round, median (min - max) of --reps rounds
that alternate the arms:
  eval_step        d2d_eval_step, one policy (the kernel the bank is measured against)
  bank_p1          d2d_eval_step_bank, P = 1
  bank_aligned     P = 16 in blocks that are multiples of 64 rows (every chunk uniform)
  bank_blocks      P = 16 in blocks that are no multiple of 64 (sweep_layout's case: one mixed chunk per boundary)
  bank_mod16       P = 16 as i % 16 (16 passes per chunk: the worst case)
and, with --deal (needs --build-deal first), at --deal-rows rows (more chunks than workgroups), the
bank_blocks map under both chunk-to-workgroup deals: the product's and the build with the other one.

The sweep: 16 policies x 7 test scenarios x --runs runs, wall time of one ``evaluate.sweep`` call against
the 112 (agent, scenario) loops of tools/test_agent.py at ``--envs`` = runs, each with its own
``Drone2dVecEnv`` and ``evaluate_policy``; both arms include batch construction and record decoding.

    python tools/bank_probe.py [--reps 5] [--calls 200] [--runs 128] [--deal] [--out profiles/eval/bank_probe.json]
    python tools/bank_probe.py --build-deal      # no device needed
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
AGENT = os.path.join(REPO, "tests", "golden", "agent_17_90.npz")
DEAL_LIB = os.path.join(REPO, "tools", "_abl", "libd2d_eval_deal.so")


DEALS = {0: "stride", 1: "ranges"}


def product_deal() -> int:
    """The product's chunk-to-workgroup deal: the source's default D2D_EVAL_BANK_DEAL."""
    import re

    import drone2d_amd  # noqa: F401
    from drone2d_amd import _build

    return int(re.search(r"#define D2D_EVAL_BANK_DEAL (\d)", open(_build.EVAL_SRC).read()).group(1))


def build_deal() -> str:
    """The library with the other chunk-to-workgroup deal (-DD2D_EVAL_BANK_DEAL=0 when the product's is 1)."""
    import subprocess

    from drone2d_amd import _build

    product = product_deal()
    os.makedirs(os.path.dirname(DEAL_LIB), exist_ok=True)
    subprocess.run([_build.hipcc(), *_build.PPO_FLAGS, f"-DD2D_EVAL_BANK_DEAL={1 - product}", "-I",
                    os.path.join(REPO, "include"), _build.EVAL_SRC, "-o", DEAL_LIB], check=True)
    return DEAL_LIB


def stats(v) -> dict:
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def make_policies(n: int) -> list:
    """The shipped agent, the perturbed and the fresh policy of the tests, then perturbations of the shipped one."""
    import torch

    from drone2d_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pert = ActorCritic()
    with torch.no_grad():
        pert.log_std.copy_(torch.tensor([-0.4, 0.3]))
        pert.action_net.weight.mul_(20.0)
    torch.manual_seed(1)
    out = [ActorCritic.from_agent_npz(AGENT), pert, ActorCritic()]
    g = torch.Generator().manual_seed(2)
    while len(out) < n:
        ac = ActorCritic.from_agent_npz(AGENT)
        with torch.no_grad():
            for p in ac.mlp_extractor.policy_net.parameters():
                p.add_(0.02 * torch.randn(p.shape, generator=g))
        out.append(ac)
    return out[:n]


def launch_us(n: int, arms: dict, reps: int, calls: int) -> dict:
    """``arms``: name -> (lib, map or None, P).  Record + act halves on the outputs of a real env step."""
    import torch

    import drone2d_amd as d2
    from drone2d_amd import abi, evaluate
    from drone2d_amd.config import ENV_TEST_CONFIG

    venv = d2.Drone2dVecEnv(n, seed=0, with_info=True, **dict(ENV_TEST_CONFIG, scenario="corridor"))
    dev = venv.device
    policies = make_policies(16)
    bank = evaluate.PolicyBank(policies, device=dev)
    ws = evaluate.actor_tensors(policies[0], dev)
    act_env = torch.zeros(n, 2, device=dev)
    venv.reset(seed=0)
    obs, _, term, trunc, info = venv.step(act_env)
    fin = torch.zeros(n, dtype=torch.uint8, device=dev)
    rows = torch.zeros(n, abi.INFO_DIM, device=dev)
    rem = torch.full((1,), n, dtype=torch.int32, device=dev)

    def args():
        return evaluate.D2DEvalStepArgs(n=n, t=1, info_dim=abi.INFO_DIM, act=1, noise_mode=evaluate.NOISE_PHILOX, seed=1,
                                        obs=obs.data_ptr(), act_env=act_env.data_ptr(), prev_term=term.data_ptr(),
                                        prev_trunc=trunc.data_ptr(), prev_info=info.data_ptr(), finished=fin.data_ptr(),
                                        rows=rows.data_ptr(), remaining=rem.data_ptr())

    runs, keep = {}, []
    for name, (lib, m, P) in arms.items():
        a = args()
        if m is None:
            evaluate._weights_into(a, ws)
            runs[name] = lambda lib=lib, a=a, st=0: evaluate._step(lib, a, st)
        else:
            ep = torch.from_numpy(np.ascontiguousarray(m, np.int32)).to(dev)
            cb = evaluate.D2DEvalBank(n_policies=P, params=bank.params.data_ptr(), env_policy=ep.data_ptr())
            keep.append((ep, cb))
            runs[name] = lambda lib=lib, a=a, cb=cb, st=0: evaluate._step_bank(lib, a, cb, st)
    st = torch.cuda.current_stream(dev).cuda_stream
    res = {k: [] for k in runs}
    for r in range(reps + 1):  # the first round is the warm-up
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                run(st=st)
            e1.record()
            e1.synchronize()
            if r:
                res[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    venv.close()
    return {k: dict(stats(v), unit="us per launch", calls=calls) for k, v in res.items()}


def blocks(n: int, size: int, P: int = 16) -> np.ndarray:
    return ((np.arange(n) // size) % P).astype(np.int32)


def maps(n: int) -> dict:
    aligned = max(64, (n // 16) // 64 * 64)
    size = -(-n // 16)
    if size % 64 == 0:
        size += 4
    return {"bank_aligned": blocks(n, aligned), "bank_blocks": blocks(n, size), "bank_mod16": blocks(n, 1)}


def sweep_seconds(reps: int, runs: int) -> dict:
    import torch

    import drone2d_amd as d2
    from drone2d_amd import evaluate
    from drone2d_amd.config import ENV_TEST_CONFIG, TEST_SCENARIOS

    dev = torch.device("cuda", 0)
    policies = [p.to(dev) for p in make_policies(16)]
    scns = list(TEST_SCENARIOS)

    def one_sweep():
        bank = evaluate.PolicyBank(policies, device=dev)
        res = evaluate.sweep(bank, scns, runs, seed=0)
        return sum(len(m["time_spent"]) for per in res.values() for m in per.values())

    def loops():
        done = 0
        for pol in policies:
            for scn in scns:
                venv = d2.Drone2dVecEnv(runs, seed=0, with_info=True, **dict(ENV_TEST_CONFIG, scenario=scn))
                m = evaluate.evaluate_policy(venv, pol, seed=0)
                venv.close()
                done += len(m["time_spent"])
        return done

    arms = {"one_sweep": one_sweep, "loops_112": loops}
    res = {k: [] for k in arms}
    episodes = {}
    for r in range(reps + 1):  # the first round is the warm-up
        for k, run in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            episodes[k] = run()
            torch.cuda.synchronize()
            if r:
                res[k].append(time.perf_counter() - t0)
    return {k: dict(stats(v), unit="s per sweep", episodes=episodes[k]) for k, v in res.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sizes", default="1000,65536")
    ap.add_argument("--runs", type=int, default=128)
    ap.add_argument("--deal", action="store_true", help="also time the build with the other chunk deal")
    ap.add_argument("--deal-rows", type=int, default=262144)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--build-deal", action="store_true", help="compile the other-deal build and exit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval", "bank_probe.json"))
    a = ap.parse_args()
    if a.build_deal:
        print("built", build_deal())
        return

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bank_probe needs a HIP device")
    from drone2d_amd import evaluate

    torch.cuda.set_device(0)
    lib = evaluate.load()
    record = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "launch": {}}
    for n in (int(s) for s in a.sizes.split(",")):
        arms = {"eval_step": (lib, None, 1), "bank_p1": (lib, np.zeros(n, np.int32), 1)}
        arms.update({k: (lib, m, 16) for k, m in maps(n).items()})
        record["launch"][str(n)] = launch_us(n, arms, a.reps, a.calls)
        print(json.dumps({"rows": n, **record["launch"][str(n)]}), flush=True)
    if a.deal:
        other = evaluate.bind(DEAL_LIB)
        n = a.deal_rows
        m = maps(n)["bank_blocks"]
        pd = product_deal()
        record["deal"] = {"rows": n, "product_deal": DEALS[pd], "other_deal_is": DEALS[1 - pd],
                          **launch_us(n, {"product": (lib, m, 16), "other_deal": (other, m, 16)}, a.reps, a.calls)}
        print(json.dumps(record["deal"]), flush=True)
    if not a.no_sweep:
        record["sweep"] = dict(sweep_seconds(a.reps, a.runs), policies=16, scenarios=7, runs=a.runs)
        print(json.dumps(record["sweep"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
