#!/usr/bin/env python
"""Times the GIF encoder (libd2d_gif.so) and the recording loop: a record for DESIGN.md "Recording", not a gate.

  encode_K    ``GifEncoder.add`` on the frames of a real corridor flight (K envs under the shipped agent, --frames
              steps, 256 x 256, HUD off): HIP events around one call (two launches), warm, median over the delta
              frames; the first (whole) frame apart; bytes per frame against raw RGB.  K = 1 and K = 16.
              The split by kernel comes from running this tool under ``rocprofv3 --kernel-trace --stats``.
  record      the wall time of ``record_episodes`` for one corridor episode at 256 x 256, every second frame,
              against the only path there was before: the same loop (the same act call, a render only for a
              kept frame, the episode's length known beforehand) with ``.cpu()`` on every kept frame, then
              ``render.save_gif`` where Pillow is installed (else the transfers alone).
One JSON line per workload; needs a HIP device (no fallback).

    python tools/gif_probe.py [--frames 64] [--size 256]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AGENT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "agent_17_90.npz")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("gif_probe needs a HIP device")
    import drone2d_amd as d2
    from drone2d_amd import evaluate, harness
    from drone2d_amd import gif as G
    from drone2d_amd import render as R
    from drone2d_amd.config import ENV_TEST_CONFIG

    dev = torch.device("cuda", 0)
    policy = harness.MlpActor.from_npz(AGENT).to(dev)
    kw = dict(ENV_TEST_CONFIG, scenario="corridor")
    size, seed = args.size, args.seed

    def ev_us(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for k in (1, 16):
        venv = d2.Drone2dVecEnv(k, seed=seed, with_info=True, **kw)
        obs = venv.reset(seed=seed)
        frames = [venv.render(range(k), size=size)]
        for t in range(args.frames - 1):
            obs = venv.step(evaluate.act(policy, obs, seed=seed, t=t, env_id_base=int(venv.cfg.env_id_base)))[0]
            frames.append(venv.render(range(k), size=size))
        venv.close()
        enc = G.GifEncoder(dev, k, size, G.Palette.model(), flush_every=args.frames)
        for f in frames:  # warm
            enc.add(f)
        enc.finish()
        first, later = [], []
        for rep in range(3):
            for t, f in enumerate(frames):
                (later if t else first).append(ev_us(lambda: enc.add(f)))
            files = enc.finish()
        n_bytes = sum(map(len, files)) / (k * len(frames))
        print(json.dumps({"workload": f"encode_{k}x{size}x{size}", "frames": len(frames),
                          "delta_frame_call_us": {"median": float(np.median(later)), "min": float(min(later)),
                                                  "max": float(max(later))},
                          "first_frame_call_us": {"median": float(np.median(first))},
                          "delta_frame_us_per_stream": float(np.median(later)) / k,
                          "bytes_per_frame": n_bytes, "raw_rgb_bytes_per_frame": size * size * 3,
                          "ratio": size * size * 3 / n_bytes}), flush=True)
        enc.close()

    # one corridor episode, every second frame
    def fresh():
        return d2.Drone2dVecEnv(1, seed=seed, with_info=True, **kw)

    venv = fresh()
    G.record_episodes(venv, policy, [0], seed=seed, size=size, max_steps=32)  # warm
    venv.close()
    venv = fresh()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = G.record_episodes(venv, policy, [0], seed=seed, size=size)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    venv.close()

    # the host path flies the same loop -- the same act call, a render only where a frame is kept, no other
    # wait for the device -- and differs in how a kept frame leaves: as pixels, .cpu().  The episode's length
    # is taken from evaluate_policy beforehand, so that neither loop asks the device for it every step.
    venv = fresh()
    steps = int(evaluate.evaluate_policy(venv, policy, seed=seed)["time_spent"][0])
    venv.close()
    venv = fresh()
    base = int(venv.cfg.env_id_base)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    obs = venv.reset(seed=seed)
    host = [venv.render([0], size=size).cpu()]
    for t in range(steps - 1):
        obs = venv.step(evaluate.act(policy, obs, seed=seed, t=t, env_id_base=base))[0]
        if (t + 1) % 2 == 0:
            host.append(venv.render([0], size=size).cpu())
    torch.cuda.synchronize()
    t_xfer = time.perf_counter() - t0
    t = steps
    t_pil, pil_bytes = None, None
    try:
        import PIL  # noqa: F401

        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "flight.gif")
            t0 = time.perf_counter()
            R.save_gif(torch.cat(host), p, fps=33)
            t_pil = time.perf_counter() - t0
            pil_bytes = os.path.getsize(p)
    except ImportError:
        pass
    venv.close()
    assert len(host) == int(rec.frames[0]), (len(host), rec.frames)
    print(json.dumps({"workload": f"record_corridor_{size}", "episode_steps": t, "frames": int(rec.frames[0]),
                      "device_path_s": t_dev, "file_bytes": len(rec.gifs[0]),
                      "host_path_render_cpu_s": t_xfer, "host_path_save_gif_s": t_pil, "host_path_file_bytes": pil_bytes,
                      "host_path_bytes_moved": len(host) * size * size * 3}), flush=True)


if __name__ == "__main__":
    main()
