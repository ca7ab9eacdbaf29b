#!/usr/bin/env python3
"""What the episode monitor costs on one MI355X (a record, no threshold; results: profiles/monitor/).

    python tools/monitor_probe.py kernel [--envs 65536] [--calls 200] [--rounds 5]
    python tools/monitor_probe.py train  [--runs 5] [--updates 30] [--parent-tree DIR]

``kernel``: corridor, ``--envs`` envs flown ``--warm`` random steps so that episodes end at their usual
rate; then HIP events around ``--calls`` back-to-back ``d2d_monitor_step`` launches on one real step's
outputs, against a torch restatement of the same digest (kept here only), the two alternating for
``--rounds`` rounds; medians.  The algorithmic bytes per env-step are counted from the shapes.

``train``: ``tools/train_ppo.py`` as a fresh child process, without and with ``--log-dir``, alternating
``--runs`` times, and once from ``--parent-tree`` (a checkout of the parent commit with its libraries
built) without ``--log-dir``; env-steps/s of each run (the whole run, and the median over the updates
after the graphs were captured).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# per env and step: the info row, term, trunc, run and minclr read; run and minclr written
# (live is touched at episode ends only, the partial rows once per workgroup)
BYTES_PER_ENV_STEP = 12 * 4 + 1 + 1 + 6 * 8 + 4 + 6 * 8 + 4


def _torch_digest(term, trunc, info, run, minclr, live, acc):
    """The digest of include/d2d_monitor.h in torch ops (any summation order)."""
    import torch

    from drone2d_amd import abi
    from drone2d_amd import monitor as M

    run += info[:, :6].t().double()
    torch.minimum(minclr, info[:, abi.INFO_DCLOSE], out=minclr)
    done = term | trunc
    dep = done & live.bool()
    cause = info[:, abi.INFO_CAUSE].to(torch.int32)
    c1, c2, c4, c5 = ((cause & b) != 0 for b in (1, 2, 4, 8))
    fin = torch.isfinite(minclr)
    one = torch.ones_like(minclr, dtype=torch.float64)
    cols = [one, c2.double(), (c1 | c4 | c5).double(), (c1 & ~c2 & ~c4 & ~c5).double(), c4.double(), c5.double(),
            info[:, abi.INFO_STEPS].double(), info[:, abi.INFO_TOTREW].double(), info[:, abi.INFO_APE].double(),
            *run, *info[:, :6].t().double(), info[:, abi.INFO_REWARD].double(),
            torch.where(fin, minclr.double(), 0.0), fin.double()]
    m = torch.stack(cols, 1)
    acc[:M.SKIPPED] += torch.where(dep[:, None], m, 0.0).sum(0)
    acc[M.SKIPPED] += (done & ~dep).sum()
    run.masked_fill_(done[None], 0.0)
    minclr.masked_fill_(done, float("inf"))
    live.masked_fill_(done, 1)


def kernel_probe(a) -> dict:
    import torch

    import drone2d_amd as d2
    from drone2d_amd import monitor as M
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    torch.cuda.set_device(0)
    n = a.envs
    venv = d2.Drone2dVecEnv(n, seed=0, **dict(ENV_TRAIN_CONFIG, scenario="corridor"))
    mon = M.EpisodeMonitor(venv)
    g = torch.Generator(device="cuda").manual_seed(0)
    venv.reset(seed=0)
    for _ in range(a.warm):
        _, _, term, trunc, info = venv.step(torch.rand(n, 2, device="cuda", generator=g) * 2 - 1)
        mon.step(term, trunc, info)
    done_rate = float((term | trunc).float().mean())
    t_run, t_min, t_live = mon.run.clone(), mon.minclr.clone(), mon.live.clone()
    t_acc = torch.zeros(M.K, dtype=torch.float64, device="cuda")
    # one call of each on the same state: the same episodes
    mon.flush()
    mon.step(term, trunc, info)
    _torch_digest(term, trunc, info, t_run, t_min, t_live, t_acc)
    dev_vec, tor_vec = mon.flush().cpu(), t_acc.cpu()
    same_counts = bool(torch.equal(dev_vec[[0, 1, 2, 3, 4, 5, 6, 23, 24]], tor_vec[[0, 1, 2, 3, 4, 5, 6, 23, 24]]))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()  # warm
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls  # us per call

    dev_us, tor_us = [], []
    for _ in range(a.rounds):
        dev_us.append(timed(lambda: mon.step(term, trunc, info)))
        tor_us.append(timed(lambda: _torch_digest(term, trunc, info, t_run, t_min, t_live, t_acc)))
    venv.close()
    med = statistics.median(dev_us)
    nbytes = BYTES_PER_ENV_STEP * n
    return {"envs": n, "calls": a.calls, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
            "done_rate_of_the_step": done_rate, "counts_equal_torch": same_counts, "n_blocks": mon.n_blocks,
            "d2d_monitor_step_us": {"median": med, "min": min(dev_us), "max": max(dev_us)},
            "torch_digest_us": {"median": statistics.median(tor_us), "min": min(tor_us), "max": max(tor_us)},
            "bytes_per_env_step": BYTES_PER_ENV_STEP, "bytes_per_call": nbytes,
            "achieved_bytes_per_s": nbytes / (med * 1e-6),
            "bound": "memory traffic; the call's working set (bytes_per_call) is re-read by back-to-back calls, so it "
                     "is served by the L2 / Infinity Cache rather than HBM, and at this size launch latency is a "
                     "large share of the call"}


def _train_run(tree: str, a, log_dir: str | None) -> dict:
    cmd = [sys.executable, os.path.join(tree, "tools", "train_ppo.py"), "--envs", str(a.envs), "--updates",
           str(a.updates)]
    if log_dir:
        cmd += ["--log-dir", log_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}: exit {r.returncode}\n{r.stderr[-3000:]}")
    recs = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    upd = [x for x in recs if "update" in x]
    steady = [x["env_steps_per_s"] for x in upd if x["update"] >= 3]
    return {"whole_run": recs[-1]["env_steps_per_s_incl_learning"], "steady_median": statistics.median(steady)}


def train_probe(a) -> dict:
    out = {"envs": a.envs, "updates": a.updates, "runs": a.runs, "off": [], "on": []}
    with tempfile.TemporaryDirectory() as tmp:
        _train_run(REPO, a, None)  # a first run nobody counts: the box's caches
        for k in range(a.runs):
            out["off"].append(_train_run(REPO, a, None))
            out["on"].append(_train_run(REPO, a, os.path.join(tmp, f"logs{k}")))
            print(json.dumps({"run": k, "off": out["off"][-1], "on": out["on"][-1]}), flush=True)
        if a.parent_tree:
            out["parent_off"] = _train_run(os.path.abspath(a.parent_tree), a, None)
        files = sorted(os.listdir(os.path.join(tmp, "logs0")))
    out["log_dir_files"] = [f if not f.startswith("events.out.tfevents.") else "events.out.tfevents.*" for f in files]
    for key in ("whole_run", "steady_median"):
        off, on = [x[key] for x in out["off"]], [x[key] for x in out["on"]]
        out[key] = {"off_median": statistics.median(off), "off_min": min(off), "off_max": max(off),
                    "on_median": statistics.median(on), "on_min": min(on), "on_max": max(on),
                    "on_over_off": statistics.median(on) / statistics.median(off)}
        if a.parent_tree:
            out[key]["parent_off"] = out["parent_off"][key]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "train"])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=64, help="kernel: env steps flown before the measured step")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None, help="result file (default: profiles/monitor/<mode>_probe.json)")
    a = ap.parse_args()
    res = kernel_probe(a) if a.mode == "kernel" else train_probe(a)
    path = a.out or os.path.join(REPO, "profiles", "monitor", f"{a.mode}_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
