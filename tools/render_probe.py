#!/usr/bin/env python
"""Times the renderer (libd2d_render.so) on the device: a record for DESIGN.md "Rendering", not a gate.

Three workloads, each timed warm with HIP events around one library call (its launches: setup + raster,
for the plot also the id clear and the scatter), median over --reps calls:
  frames   64 frames of 256 x 256 on S_corridor (58 circles), with obs, actions and a 64-point trail
  full     one 1300 x 1300 frame
  plot     the overview plot of 20 000 corridor-like paths (up to 1100 points) at 1300 x 1300
For each: the time, the written-bytes rate (the picture's bytes over the time) and the host twin's time
on the same inputs.  One JSON line per workload; needs a HIP device (no fallback).

    python tools/render_probe.py [--reps 30] [--no-host]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps: int, warmup: int = 5) -> dict:
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return {"median_us": float(np.median(ms) * 1e3), "min_us": float(ms.min() * 1e3), "max_us": float(ms.max() * 1e3)}


def frame_inputs(k: int, trail_cap: int, seed: int):
    import drone2d_amd  # noqa: F401
    from drone2d_amd.scenarios import create_test_scenario

    rng = np.random.default_rng(seed)
    scn = create_test_scenario("S_corridor", 1300, 1300)
    st = np.zeros((32, k))
    st[0], st[1] = rng.uniform(100, 1200, k), rng.uniform(300, 1000, k)
    st[2] = rng.uniform(-0.7, 0.7, k)
    st[3], st[4] = rng.uniform(-200, 200, k), rng.uniform(-200, 200, k)
    for b, sgn in ((6, -1.0), (12, 1.0)):
        st[b], st[b + 1], st[b + 2] = st[0] + sgn * 40 * np.cos(st[2]), st[1] + sgn * 40 * np.sin(st[2]), st[2]
    obs = rng.uniform(-0.8, 0.8, (k, 27)).astype(np.float32)
    act = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
    trail = (np.stack([st[0], st[1]], 1)[:, None, :] + np.cumsum(rng.uniform(-8, 8, (k, trail_cap, 2)), 1)[:, ::-1])
    return [scn] * k, st, obs, act, trail.astype(np.float32), np.full(k, trail_cap, np.int32)


def plot_inputs(n_paths: int, max_len: int, seed: int):
    rng = np.random.default_rng(seed)
    steps = rng.normal(0, 0.6, (max_len, n_paths, 2))
    steps[..., 0] += 0.9  # left to right along the corridor, about 1 px per step
    xy = np.cumsum(steps, 0) + np.stack([rng.uniform(60, 250, n_paths), rng.uniform(500, 800, n_paths)], 1)[None]
    lens = rng.integers(200, max_len + 1, n_paths).astype(np.int32)
    return xy.astype(np.float32), lens, rng.integers(0, 256, (n_paths, 3)).astype(np.uint8)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30, help="timed calls per workload (at least 20)")
    ap.add_argument("--no-host", action="store_true", help="skip the host twin's times")
    ap.add_argument("--paths", type=int, default=20000)
    args = ap.parse_args()
    reps = max(20, args.reps)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("render_probe needs a HIP device")
    import drone2d_amd  # noqa: F401
    from drone2d_amd import render as R
    from drone2d_amd.scenarios import create_test_scenario

    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    r = R.Renderer(dev, max_frames=64, max_trail=64)

    def host_ms(fn):
        if args.no_host:
            return None
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    for name, k, size in (("frames_64x256x256", 64, 256), ("frame_1x1300x1300", 1, 1300)):
        scns, st, obs, act, trail, tl = frame_inputs(k, 64, seed=k)
        scn_d, dev_in = r.scn_tensor(scns), [t(a) for a in (st, obs, act, trail, tl)]
        out = torch.empty((k, size, size, 3), dtype=torch.uint8, device=dev)
        res = timed(lambda: r.render(scn_d, *dev_in, size=size, out=out), reps)
        same = bool((out.cpu().numpy() == R.render_host(scns, st, obs, act, trail, tl, size=size)).all())
        res.update(workload=name, bytes_written=int(out.numel()), equals_host_twin=same,
                   written_GBps=out.numel() / (res["median_us"] * 1e-6) / 1e9,
                   host_twin_ms=host_ms(lambda: R.render_host(scns, st, obs, act, trail, tl, size=size)))
        print(json.dumps(res), flush=True)

    scn = create_test_scenario("corridor", 1300, 1300)
    xy, lens, rgb = plot_inputs(args.paths, 1100, seed=3)
    scn_d, dev_in = r.scn_tensor([scn]), [t(a) for a in (xy, lens, rgb)]
    out = torch.empty((1300, 1300, 3), dtype=torch.uint8, device=dev)
    res = timed(lambda: r.plot_paths(scn_d, *dev_in, size=1300, out=out), reps)
    res.update(workload=f"plot_{args.paths}_paths_1300x1300", bytes_written=int(out.numel()),
               path_segments=int(np.maximum(lens - 1, 0).sum()),
               written_GBps=out.numel() / (res["median_us"] * 1e-6) / 1e9)
    if not args.no_host:
        t0 = time.perf_counter()
        want = R.plot_paths_host(scn, xy, lens, rgb, size=1300)
        res.update(host_twin_ms=(time.perf_counter() - t0) * 1e3, equals_host_twin=bool((out.cpu().numpy() == want).all()))
    print(json.dumps(res), flush=True)
    r.close()


if __name__ == "__main__":
    main()
