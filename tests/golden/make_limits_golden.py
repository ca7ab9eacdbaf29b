#!/usr/bin/env python3
"""Path fixture for user scenarios at the ABI's limits, from the reference's own Python.

Run ONLY where the reference is present (like make_golden.py, whose import helper and shims this uses):

    python tests/golden/make_limits_golden.py

Executed from the reference, unmodified: ``predef_path.py`` -- the QPMI2D fit, ``__call__``,
``get_closest_u`` (scipy ``fminbound``), ``get_closest_position`` and ``get_lookahead_point``.

The waypoints of the eleven limit paths are chosen here and recorded in the fixture;
tests/limit_scenarios.py builds its scenarios from the recorded waypoints, so this file, the CPU
tests and the GPU tests all read the same geometry.

Writes tests/golden/limits_probe.npz (float64 arrays only, allow_pickle=False).  Per path NAME:
  NAME/wps, NAME/us, NAME/x_params, NAME/y_params   waypoints and the reference's fit
  NAME/u, NAME/xy          QPMI2D.__call__ on u in [-10, L + 10]: a uniform draw, both bounds, dense
                           around every knot and around us[-2] - 0.001
  NAME/pts                 points: behind the start along the start tangent, beyond the end, within
                           +-40 px of the path, a coarse grid
  NAME/closest_u, NAME/closest_xy, NAME/lookahead_xy   get_closest_u / _position / lookahead (220)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

LOOKAHEAD = 220
N_UNIFORM, N_BEHIND, N_BEYOND, N_NEAR, GRID = 80, 16, 12, 60, 7


def _zig(n, x0, y0, dx, dy):
    return np.array([[x0 + dx * i, y0 + (dy if i % 2 else 0.0)] for i in range(n)], dtype=np.float64)


def limit_waypoints():
    """name -> waypoints [n, 2]."""
    ang = np.deg2rad(np.linspace(200.0, -20.0, 16))
    return {
        "w3_arc": np.array([[200.0, 300.0], [600.0, 700.0], [1100.0, 800.0]]),
        "w3_line": np.array([[200.0, 400.0], [600.0, 600.0], [1100.0, 850.0]]),
        "w3_tiny": np.array([[600.0, 650.0], [600.5, 650.25], [601.0, 650.125]]),
        "w3_dust": np.array([[650.0, 650.0], [650.0078125, 650.00390625], [650.015625, 650.0]]),
        "w3_long": np.array([[100.0, 600.0], [30100.0, 10600.0], [62100.0, 5600.0]]),
        "w4_zig": _zig(4, 200.0, 500.0, 300.0, 200.0),
        "w5_zig": _zig(5, 150.0, 600.0, 250.0, 200.0),
        "w15_zig": _zig(15, 100.0, 600.0, 80.0, 80.0),
        "w16_zig": _zig(16, 90.0, 550.0, 75.0, 100.0),
        "w16_arc": np.stack([650.0 + 450.0 * np.cos(ang), 500.0 + 450.0 * np.sin(ang)], -1),
        "w16_long": _zig(16, 100.0, 400.0, 2000.0, 600.0),
    }


def probe_us(path, rng):
    us, L = np.asarray(path.us, dtype=np.float64), float(path.length)
    gap = float(np.min(np.diff(us)))
    m = max(2, int(np.ceil(40 / len(us))))
    off = np.geomspace(1e-9, 0.45 * gap, m)
    off = np.concatenate([[0.0], off, -off])
    knots = (us[:, None] + off[None, :]).ravel()
    w = np.array([0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-4, -1e-4, 5e-4, -5e-4])
    window = us[-2] - 0.001 + w * min(1.0, gap)
    # (the uniform draws on a 2^-10 grid and the points on a 2^-5 px grid: the file compresses better)
    u = np.concatenate([np.round(rng.uniform(-10.0, L + 10.0, N_UNIFORM) * 1024.0) / 1024.0, [-10.0, L + 10.0], knots,
                        window])
    return np.clip(u, -10.0, L + 10.0)


def probe_points(path, rng):
    wps, L = np.asarray(path.waypoints, dtype=np.float64), float(path.length)

    def end(u0, sign):  # the search bound's point and the unit tangent there, pointing out of the path
        p0 = np.asarray(path(u0))
        tg = sign * (np.asarray(path(u0 + 1e-3)) - np.asarray(path(u0 - 1e-3)))
        return p0, tg / np.hypot(*tg)

    p0, t0 = end(-10.0, -1.0)
    behind = p0 + np.geomspace(0.5, 2000.0, N_BEHIND)[:, None] * t0
    p1, t1 = end(L + 10.0, 1.0)
    beyond = p1 + np.geomspace(0.5, 2000.0, N_BEYOND)[:, None] * t1
    u = rng.uniform(-10.0, L + 10.0, N_NEAR)
    near = np.array([path(float(x)) for x in u]) + rng.uniform(-40.0, 40.0, (N_NEAR, 2))
    lo, hi = wps.min(0) - 600.0, wps.max(0) + 600.0
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], GRID), np.linspace(lo[1], hi[1], GRID))
    grid = np.stack([gx, gy], -1).reshape(-1, 2)
    return np.round(np.concatenate([behind, beyond, near, grid]) * 32.0) / 32.0


def main():
    _, pp, _, _, _ = _import_reference()
    out = {}
    for k, (name, wps) in enumerate(limit_waypoints().items()):
        rng = np.random.default_rng(100 + k)
        path = pp.QPMI2D(wps)
        u = probe_us(path, rng)
        pts = probe_points(path, rng)
        out[f"{name}/wps"] = np.asarray(wps, dtype=np.float64)
        out[f"{name}/us"] = np.asarray(path.us, dtype=np.float64)
        out[f"{name}/x_params"] = np.asarray(path.x_params, dtype=np.float64)
        out[f"{name}/y_params"] = np.asarray(path.y_params, dtype=np.float64)
        out[f"{name}/u"] = u
        out[f"{name}/xy"] = np.array([path(float(x)) for x in u])
        out[f"{name}/pts"] = pts
        out[f"{name}/closest_u"] = np.array([path.get_closest_u([float(p[0]), float(p[1])]) for p in pts])
        out[f"{name}/closest_xy"] = np.array([path.get_closest_position([float(p[0]), float(p[1])]) for p in pts])
        out[f"{name}/lookahead_xy"] = np.array([path.get_lookahead_point([float(p[0]), float(p[1])], LOOKAHEAD)
                                                for p in pts])
        print(name, "L = %.6g" % float(path.length), "u", len(u), "pts", len(pts))
    assert all(v.dtype == np.float64 for v in out.values())
    dst = os.path.join(HERE, "limits_probe.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
