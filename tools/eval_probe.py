#!/usr/bin/env python
"""Times evaluation per env step on the device: a record for DESIGN.md "Evaluation", not a gate.

At 1 000 and 65 536 corridor envs with the shipped agent, stochastic, a fixed 256 steps (no early
stop), after one warm run, median of --reps runs, the arms alternating (host clock around a run that
ends in a read-back):
  fused        evaluate_policy(noise="philox"): one d2d_eval_step + one d2d_step per env step
  torch        harness.run_first_episodes, batch_invariant=False (torch GEMMs, randn, where / mask ops)
  torch_fixed  harness.run_first_episodes, batch_invariant=True (the sharding-exact path; 1 000 envs only)
and the d2d_eval_step launch alone (record + act halves on a real step's outputs) from HIP events.
Every arm's run includes the reset and the host's decoding of the finished episodes' records, the same
code in all arms; ``records_tail`` is that decoding timed alone (same number of finished episodes),
per step, to read the arms' differences against.
One JSON line per size on stdout and the whole record in --out; needs a HIP device (no fallback).

    python tools/eval_probe.py [--reps 5] [--steps 256] [--out profiles/eval/eval_probe.json] [--valu]
    python tools/eval_probe.py --build-valu      # no device needed

``--build-valu`` compiles a diagnostic build of the library whose hidden layers are plain fmaf loops
(tools/patches/eval_actor_valu.patch applied to a copy of the sources) into tools/_abl/; ``--valu`` also
times that build's launch, alternating with the product's, and checks that its actions are the
product's bit for bit (both are k-ordered fmaf chains).
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


def per_step_us(runs: dict, steps: int, reps: int) -> dict:
    """Each arm once warm (libraries loaded, allocator filled), then ``reps`` rounds that alternate
    the arms, so a change in the machine's load falls on all of them."""
    import torch

    for run in runs.values():
        run()
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            us[k].append((time.perf_counter() - t0) * 1e6 / steps)
    return {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))}
            for k, v in us.items()}


VALU_LIB = os.path.join(REPO, "tools", "_abl", "libd2d_eval_valu.so")


def build_valu() -> str:
    import shutil
    import subprocess
    import tempfile

    import drone2d_amd  # noqa: F401
    from drone2d_amd import _build

    tmp = tempfile.mkdtemp(prefix="d2d_eval_var_")
    try:
        pkg = os.path.basename(_build.PKG_DIR)
        shutil.copytree(os.path.join(_build.PKG_DIR, "csrc"), os.path.join(tmp, pkg, "csrc"))
        subprocess.run(["patch", "-s", "-p1", "-d", tmp, "-i",
                        os.path.join(REPO, "tools", "patches", "eval_actor_valu.patch")], check=True)
        os.makedirs(os.path.dirname(VALU_LIB), exist_ok=True)
        subprocess.run([_build.hipcc(), *_build.PPO_FLAGS, "-I", os.path.join(REPO, "include"),
                        os.path.join(tmp, os.path.relpath(_build.EVAL_SRC, REPO)), "-o", VALU_LIB], check=True)
    finally:
        shutil.rmtree(tmp)
    return VALU_LIB


def kernel_us(venv, policy, libs: dict, calls: int = 200) -> dict:
    """d2d_eval_step alone, both halves, on the outputs of a real env step: HIP events around
    ``calls`` back-to-back launches, the builds in ``libs`` alternating."""
    import torch

    from drone2d_amd import abi, evaluate

    dev, n = venv.device, venv.num_envs
    ws = evaluate.actor_tensors(policy, dev)
    act_env = torch.zeros(n, 2, device=dev)
    venv.reset(seed=0)
    obs, _, term, trunc, info = venv.step(act_env)
    fin = torch.zeros(n, dtype=torch.uint8, device=dev)
    rows = torch.zeros(n, abi.INFO_DIM, device=dev)
    rem = torch.full((1,), n, dtype=torch.int32, device=dev)
    a = evaluate.D2DEvalStepArgs(n=n, t=1, info_dim=abi.INFO_DIM, act=1, noise_mode=evaluate.NOISE_PHILOX, seed=1,
                                 obs=obs.data_ptr(), act_env=act_env.data_ptr(), prev_term=term.data_ptr(),
                                 prev_trunc=trunc.data_ptr(), prev_info=info.data_ptr(), finished=fin.data_ptr(),
                                 rows=rows.data_ptr(), remaining=rem.data_ptr())
    evaluate._weights_into(a, ws)
    st = torch.cuda.current_stream(dev).cuda_stream
    res = {k: [] for k in libs}
    acts = {}
    for r in range(6):  # the first round is the warm-up
        for k, lib in libs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                evaluate._step(lib, a, st)
            e1.record()
            e1.synchronize()
            if r:
                res[k].append(e0.elapsed_time(e1) * 1e3 / calls)
            acts[k] = act_env.clone()
    out = {k: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v)), "calls": calls}
           for k, v in res.items()}
    for k in acts:
        out[k]["actions_equal_product"] = bool(torch.equal(acts[k], acts["product"]))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--sizes", default="1000,65536")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval", "eval_probe.json"))
    ap.add_argument("--build-valu", action="store_true", help="compile the fmaf-loop diagnostic build and exit")
    ap.add_argument("--valu", action="store_true", help="also time the fmaf-loop diagnostic build's launch")
    args = ap.parse_args()
    if args.build_valu:
        print("built", build_valu())
        return

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("eval_probe needs a HIP device")
    import drone2d_amd as d2
    from drone2d_amd import evaluate, harness
    from drone2d_amd.config import ENV_TEST_CONFIG
    from drone2d_amd.evaluate import _records, evaluate_policy

    torch.cuda.set_device(0)
    libs = {"product": evaluate.load()}
    if args.valu:
        libs["valu"] = evaluate.bind(VALU_LIB)
    never = 1 << 30  # check_every: no read-back, no early stop
    record = {"steps": args.steps, "reps": args.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for n in (int(s) for s in args.sizes.split(",")):
        venv = d2.Drone2dVecEnv(n, seed=0, with_info=True, **dict(ENV_TEST_CONFIG, scenario="corridor"))
        pol = harness.MlpActor.from_npz(AGENT).to(venv.device)
        fixed = harness.MlpActor.from_npz(AGENT, batch_invariant=True).to(venv.device)
        kw = dict(seed=0, max_steps=args.steps, check_every=never)
        runs = {"fused": lambda: evaluate_policy(venv, pol, **kw),
                "torch": lambda: harness.run_first_episodes(venv, pol, **kw)}
        if n <= 1000:
            runs["torch_fixed"] = lambda: harness.run_first_episodes(venv, fixed, **kw)
        res = per_step_us(runs, args.steps, args.reps)
        res["d2d_eval_step_kernel"] = kernel_us(venv, pol, libs)
        m = evaluate_policy(venv, pol, seed=0, max_steps=args.steps, check_every=never)
        k = len(m["time_spent"])
        fin, rows = np.arange(n) < k, np.zeros((n, d2.abi.INFO_DIM), np.float32)
        t0 = time.perf_counter()
        _records(venv, fin, rows, None, 0)
        res["records_tail"] = {"finished": k, "us_per_step": (time.perf_counter() - t0) * 1e6 / args.steps}
        venv.close()
        record["sizes"][str(n)] = res
        print(json.dumps({"envs": n, **res}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
