#!/usr/bin/env python
"""Times the HUD renderer (libd2d_hud.so) against the plain renderer in the same run: a record for
DESIGN.md "Rendering", not a gate.

render_probe.py's method (HIP events around one library call, warm, median over --reps calls) on its two
frame workloads -- 64 frames of 256 x 256 on S_corridor with 64-point trails, and one 1300 x 1300 frame:
  plain      d2dr_render                       (the yardstick of this run)
  hud_clear  d2dh_render, the three new bits clear (the shared tile walk over the extended list)
  hud_all    d2dh_render with text, arcs and 32 shades per frame
and the shade recorder, d2dh_shade_update for 16 of 65 536 envs.  One JSON line per workload with the
three medians and their ratios to `plain`; needs a HIP device (no fallback).

    python tools/hud_probe.py [--reps 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from render_probe import frame_inputs, timed  # noqa: E402

SHADES = 32


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30, help="timed calls per workload (at least 20)")
    args = ap.parse_args()
    reps = max(20, args.reps)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("hud_probe needs a HIP device")
    import drone2d_amd  # noqa: F401
    from drone2d_amd import hud as H
    from drone2d_amd import render as R

    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    base = R.Renderer(dev, max_frames=64, max_trail=64)
    hud = H.HudRenderer(dev, max_frames=64, max_trail=64, max_shades=SHADES)

    for name, k, size in (("frames_64x256x256", 64, 256), ("frame_1x1300x1300", 1, 1300)):
        scns, st, obs, act, trail, tl = frame_inputs(k, 64, seed=k)
        rng = np.random.default_rng(k + 100)
        info = rng.standard_normal((k, 12)).astype(np.float32)
        poses = np.stack([rng.uniform(100, 1200, (k, SHADES)), rng.uniform(300, 1000, (k, SHADES)),
                          rng.uniform(-0.7, 0.7, (k, SHADES))], -1)
        count = np.full(k, SHADES, np.int32)
        scn_d, dev_in = base.scn_tensor(scns), [t(a) for a in (st, obs, act, trail, tl)]
        info_d, shades_d = t(info), (t(poses), t(count))
        out = torch.empty((k, size, size, 3), dtype=torch.uint8, device=dev)
        res = {"workload": name}
        res["plain"] = timed(lambda: base.render(scn_d, *dev_in, size=size, out=out), reps)
        plain = out.clone()
        res["hud_clear"] = timed(lambda: hud.render(scn_d, *dev_in, info_d, shades_d, size=size, layers=R.L_ALL, out=out),
                                 reps)
        res["clear_equals_plain"] = bool(torch.equal(out, plain))
        res["hud_all"] = timed(lambda: hud.render(scn_d, *dev_in, info_d, shades_d, size=size, layers=H.L_ALL, out=out),
                               reps)
        res["all_equals_host_twin"] = bool((out.cpu().numpy() == H.render_host(
            scns, st, obs, act, trail, tl, info, (poses, count), size=size, layers=H.L_ALL)).all())
        res["clear_over_plain"] = res["hud_clear"]["median_us"] / res["plain"]["median_us"]
        res["all_over_plain"] = res["hud_all"]["median_us"] / res["plain"]["median_us"]
        print(json.dumps(res), flush=True)

    n, k = 65536, 16
    rng = np.random.default_rng(1)
    state = t(rng.uniform(100, 1200, (32, n)))
    ids = t(np.sort(rng.choice(n, k, replace=False)).astype(np.int32))
    term, trunc = t((rng.random(n) < 0.01).astype(np.uint8)), t(np.zeros(n, np.uint8))
    poses = torch.zeros(k, SHADES, 3, dtype=torch.float64, device=dev)
    count = torch.zeros(k, dtype=torch.int32, device=dev)
    last = torch.zeros(k, 2, dtype=torch.float64, device=dev)
    lib = H.load()

    def update():
        H.check(lib.d2dh_shade_update(dev.index, k, ids.data_ptr(), n, state.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                                      75.0, SHADES, poses.data_ptr(), count.data_ptr(), last.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream), "d2dh_shade_update")

    res = {"workload": f"shade_update_{k}_of_{n}", "update": timed(update, reps)}
    print(json.dumps(res), flush=True)
    base.close()
    hud.close()


if __name__ == "__main__":
    main()
