"""libd2d_render.so (include/d2d_render.h): the picture model against an independent rasteriser and
known answers (CPU, through the library's host twins), and the device kernels byte for byte against
those twins (GPU)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, SCENARIOS

SW = SH = 1300.0
BG = (243, 243, 243)
BLACK, BLUE, LA, RED, GREEN = (0, 0, 0), (0, 0, 255), (0, 150, 150), (255, 0, 0), (0, 255, 0)
OBST, BODY, MOTOR, GREY, TRAIL = (188, 72, 72), (66, 135, 245), (33, 93, 191), (179, 179, 179), (16, 19, 97)


@pytest.fixture(scope="module")
def R(d2):
    from drone2d_amd import _build, render

    _build.build_render()
    return render


def make_scenario(wps, circles=(), spawn=(50.0, 300.0, 150.0, 1000.0), name="crafted"):
    from drone2d_amd.scenarios import QPMIPath, Scenario

    wps = np.asarray(wps, np.float64)
    return Scenario(name, wps, QPMIPath(wps), np.asarray(circles, np.float64).reshape(-1, 3), tuple(spawn))


def pose_state(k, poses):
    """fp64 state [32, k]: frame at (x, y, angle) with velocity (vx, vy); the motors at -+40 along the
    frame with slightly different angles (the bodies' own poses are what is drawn)."""
    st = np.zeros((32, k))
    for i, (x, y, a, vx, vy) in enumerate(poses):
        st[0:6, i] = (x, y, a, vx, vy, 0.2)
        st[6:12, i] = (x - 40 * math.cos(a), y - 40 * math.sin(a), a + 0.05, vx, vy, 0.0)
        st[12:18, i] = (x + 40 * math.cos(a), y + 40 * math.sin(a), a - 0.04, vx, vy, 0.0)
    return st


# ---------------------------------------------------------------- an independent rasteriser (numpy fp64)
class RefRaster:
    """The picture model of include/d2d_render.h written out in numpy fp64, calling none of the
    library's code.  ``margin`` is each pixel's least |distance| to any primitive's edge."""

    def __init__(self, H, W, sw=SW, sh=SH):
        self.px, self.py = sw / W, sh / H
        self.X = ((np.arange(W) + 0.5) * sw / W)[None, :].repeat(H, 0)
        self.Y = (sh - (np.arange(H) + 0.5) * sh / H)[:, None].repeat(W, 1)
        self.img = np.empty((H, W, 3), np.uint8)
        self.img[:] = BG
        self.margin = np.full((H, W), np.inf)

    def _paint(self, covered, dist, colour):
        self.img[covered] = colour
        self.margin = np.minimum(self.margin, np.abs(dist))

    def circle(self, c, r, colour, dot=False):
        r = max(r, self.px) if dot else r
        dx, dy = self.X - c[0], self.Y - c[1]
        self._paint(dx * dx + dy * dy <= r * r, np.hypot(dx, dy) - r, colour)

    def capsule(self, a, b, w, colour):
        hw = max(w / 2, 0.75 * self.px)
        d = np.array([b[0] - a[0], b[1] - a[1]], np.float64)
        l2 = d @ d
        wx, wy = self.X - a[0], self.Y - a[1]
        t = np.clip((wx * d[0] + wy * d[1]) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(wx)
        ex, ey = wx - t * d[0], wy - t * d[1]
        self._paint(ex * ex + ey * ey <= hw * hw, np.hypot(ex, ey) - hw, colour)

    def box(self, c, ang, hx, hy, colour):
        dx, dy = self.X - c[0], self.Y - c[1]
        u = dx * np.cos(ang) + dy * np.sin(ang)
        v = -dx * np.sin(ang) + dy * np.cos(ang)
        self._paint((np.abs(u) <= hx) & (np.abs(v) <= hy), np.maximum(np.abs(u) - hx, np.abs(v) - hy), colour)


def ref_frame(scn, st, obs, act, trail, H, W):
    """One frame, all layers, in painter's order (the issue's section 2)."""
    r = RefRaster(H, W)
    us = scn.path.us
    pts = [scn.path(u) for u in np.linspace(us[0], us[-1], 100)]
    for a, b in zip(pts[:-1], pts[1:]):
        r.capsule(a, b, 1, BLACK)
    r.circle(scn.path(us[0]), 5, BLACK, dot=True)
    r.circle(scn.wps[-1], 5, BLACK, dot=True)
    x0, x1, y0, y1 = scn.spawn
    for a, b in (((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0))):
        r.capsule(a, b, 2, BLACK)
    p = st[0:2]
    if obs is not None:
        r.circle(((obs[19] + 1.0) * SW / 2, (obs[20] + 1.0) * SH / 2), 5, BLUE, dot=True)
        la = ((obs[21] + 1.0) * SW / 2, (obs[22] + 1.0) * SH / 2)
        r.capsule(p, la, 4, LA)
        r.circle(la, 5, LA, dot=True)
    r.capsule(p, p + st[3:5], 4, RED)
    if len(scn.circles):
        verts = np.array([(sx * 50.0, sy * 5.0) for sx in (-1, 1) for sy in (-1, 1)])
        d = [min(np.hypot(*(v + p - c[:2])) for v in verts) - c[2] for c in scn.circles]
        r.capsule(p, scn.circles[int(np.argmin(d))][:2], 4, GREEN)  # argmin: lowest index on ties
    for c in scn.circles:
        r.circle(c[:2], c[2], OBST)
    r.box(st[0:2], st[2], 50, 5, BODY)
    r.box(st[6:8], st[8], 10, 10, MOTOR)
    r.box(st[12:14], st[14], 10, 10, MOTOR)
    if act is not None:
        c, s = math.cos(st[2]), math.sin(st[2])
        local = lambda lx, ly: (p[0] + c * lx - s * ly, p[1] + s * lx + c * ly)  # noqa: E731
        for k, lx in enumerate((-40.0, 40.0)):
            r.capsule(local(lx, 0), local(lx, 50.0), 4, GREY)
            r.capsule(local(lx, 0), local(lx, (float(act[k]) / 2 + 0.5) * 1000 * 0.05), 4, RED)
    r.circle(scn.wps[-1], 5, RED, dot=True)
    if trail is not None and len(trail) >= 2:
        for a, b in zip(trail[:-1], trail[1:]):
            r.capsule(a, b, 1, TRAIL)
    return r.img, r.margin


POSE = (431.3, 668.9, 0.3, 61.0, -34.0)
OBS = np.zeros(27, np.float32)
OBS[19:23] = (-0.31, 0.07, -0.22, 0.12)
ACT = np.array([0.4, -0.6], np.float32)
TRAIL_PTS = np.array([[300.2, 610.1], [340.7, 640.3], [371.9, 652.2], [401.4, 661.8], [431.3, 668.9]], np.float32)


@pytest.mark.parametrize("size,allowed", [(96, 9), (128, 16)])
def test_twin_matches_independent_rasteriser(R, size, allowed):
    """Each of the 7 test scenarios with a fixed pose, obs, action and trail: the host twin's frame
    equals the numpy fp64 rasteriser's at every pixel farther than 0.01 world px from every primitive
    edge, and those excluded pixels are at most 0.1 % of the frame."""
    from drone2d_amd.scenarios import create_test_scenario

    scns = [create_test_scenario(s, 1300, 1300) for s in SCENARIOS]
    k = len(scns)
    st = pose_state(k, [POSE] * k)
    got = R.render_host(scns, st, np.tile(OBS, (k, 1)), np.tile(ACT, (k, 1)), np.tile(TRAIL_PTS, (k, 1, 1)),
                        np.full(k, len(TRAIL_PTS), np.int32), size=size)
    for i, scn in enumerate(scns):
        ref, margin = ref_frame(scn, st[:, i], OBS.astype(np.float64), ACT, TRAIL_PTS.astype(np.float64), size, size)
        near = margin < 0.01
        diff = (got[i] != ref).any(-1)
        print(f"{scn.name} {size}x{size}: {int(near.sum())} pixels within 0.01 px of an edge, "
              f"{int(diff.sum())} differing, {int((diff & ~near).sum())} of them away from an edge")
        assert int(near.sum()) <= allowed, scn.name
        assert not (diff & ~near).any(), scn.name
        assert len({tuple(c) for c in ref.reshape(-1, 3)}) >= 7  # the frame is not trivially empty


def pix(x, y, H=1300, W=1300):
    return int((SH - y) / (SH / H)), int(x / (SW / W))


@pytest.fixture(scope="module")
def crafted(R):
    """Two full-size frames with known answers: the drone at (400.5, 700.5), level, flying right at 200 px/s
    through an obstacle of radius 20 at (500.5, 700.5); the target (wp_last) inside a second obstacle.
    Frame 0 without force vectors (act NULL), frame 1 with."""
    wps = [(100.0, 200.0), (600.0, 400.0), (1100.5, 1000.5)]
    scn = make_scenario(wps, [(500.5, 700.5, 20.0), (1100.5, 1000.5, 50.0)])
    st = pose_state(1, [(400.5, 700.5, 0.0, 200.0, 0.0)])
    st[8, 0] = st[14, 0] = 0.0  # motors level too
    obs = np.zeros((1, 27), np.float32)
    obs[0, 19:23] = (2 * 400.5 / SW - 1, 2 * 1000.5 / SH - 1, 2 * 400.5 / SW - 1, 2 * 900.5 / SH - 1)  # straight up
    f0 = R.render_host([scn], st, obs, None, size=1300)[0]
    f1 = R.render_host([scn], st, obs, np.array([[1.0, -1.0]], np.float32), size=1300)[0]
    return f0, f1


def test_layer_order_known_answers(crafted):
    f0, f1 = crafted
    at = lambda f, x, y: tuple(int(v) for v in f[pix(x, y)])  # noqa: E731
    # the target dot over an obstacle, the obstacle around it
    assert at(f0, 1100.5, 1000.5) == RED and at(f0, 1100.5, 1003.5) == RED
    assert at(f0, 1100.5, 1030.5) == OBST and at(f0, 1100.5, 1060.5) == BG
    # a motor over the frame; the frame beside it
    assert at(f0, 445.5, 703.5) == MOTOR and at(f0, 355.5, 697.5) == MOTOR
    assert at(f0, 410.5, 703.5) == BODY and at(f0, 425.5, 704.5) == BODY
    assert at(f0, 445.5, 708.5) == MOTOR and at(f0, 425.5, 708.5) == BG
    # the obstacles over the velocity line (and over the line to the nearest obstacle); the line beyond it
    assert at(f0, 500.5, 700.5) == OBST and at(f0, 515.5, 700.5) == OBST
    assert at(f0, 560.5, 700.5) == RED and at(f0, 600.5, 701.5) == RED and at(f0, 610.5, 700.5) == BG
    assert at(f0, 465.5, 700.5) == GREEN  # the nearest-obstacle line lies over the velocity line
    # the lookahead line and dots (straight up from the drone), under the drone at its root
    assert at(f0, 400.5, 800.5) == LA and at(f0, 400.5, 900.5) == LA and at(f0, 400.5, 1000.5) == BLUE
    assert at(f0, 400.5, 702.5) == BODY
    # the path's start dot, the spawn rectangle's corner, the background elsewhere
    assert at(f0, 100.5, 200.5) == BLACK and at(f0, 50.5, 150.5) == BLACK and at(f0, 300.5, 999.5) == BLACK
    assert at(f0, 10.5, 10.5) == BG and at(f0, 1290.5, 1290.5) == BG and at(f0, 800.5, 100.5) == BG
    # force vectors over the drone: left full (F 0.05 = 50: all red), right zero (grey, a red dot at its root)
    assert at(f1, 360.5, 730.5) == RED and at(f1, 360.5, 700.5) == RED and at(f1, 360.5, 751.5) == RED
    assert at(f1, 440.5, 730.5) == GREY and at(f1, 440.5, 700.5) == RED and at(f1, 440.5, 753.5) == BG
    assert at(f1, 445.5, 703.5) == MOTOR


def _curvy(n):
    rng = np.random.default_rng(n)
    t = np.linspace(0.0, 1.0, n)
    return np.stack([100 + 1100 * t, 650 + 300 * np.sin(5 * t) + rng.uniform(-40, 40, n)], 1)


@pytest.mark.parametrize("n_wps", [3, 16])
def test_path_samples(R, n_wps):
    """The 100 samples of the path layer against scenarios.QPMIPath.__call__: a 3-waypoint path (one
    quadratic, never the blend branch) and a 16-waypoint one (D2D_MAX_WPS)."""
    scn = make_scenario(_curvy(n_wps))
    got = R.path_samples(scn)
    us = scn.path.us
    ref = np.array([scn.path(u) for u in np.linspace(us[0], us[-1], 100)])
    err = np.abs(got - ref).max()
    print(f"{n_wps} waypoints: max |sample - QPMIPath| = {err:.3g} px")
    assert err <= 1e-9
    np.testing.assert_allclose(got[-1], scn.wps[-1], atol=1e-6)


def test_plot_twin(R):
    """Overlapping paths: the highest index wins; paths of 0, 1 and 2 points draw nothing; the colour bar
    rows carry red_blue_grad's values; a NULL scenario gives a blank background."""
    L, P = 40, 6
    xy = np.zeros((L, P, 2), np.float32)
    xs = np.linspace(150.5, 1000.5, L)
    for m in range(P):
        xy[:, m, 0] = xs
        xy[:, m, 1] = 300.5 if m in (0, 1, 2) else 500.5 + 100 * (m - 3)  # 0, 1, 2 on one line
    rgb = np.array([(10, 20, 30), (40, 50, 60), (70, 80, 90), (1, 2, 3), (4, 5, 6), (7, 8, 9)], np.uint8)
    lens = np.array([L, L, 30, 0, 1, 2], np.int32)
    img = R.plot_paths_host(None, xy, lens, rgb, size=1300)
    at = lambda x, y: tuple(int(v) for v in img[pix(x, y)])  # noqa: E731
    assert at(xs[10], 300.5) == (70, 80, 90)                 # three paths: index 2 wins ...
    assert at(xs[35], 300.5) == (40, 50, 60)                 # ... where it has ended, index 1
    for m in (3, 4, 5):
        assert at(xs[0], 500.5 + 100 * (m - 3)) == BG        # 0, 1, 2 points draw nothing
    assert at(xs[10], 302.5) == BG and at(50.5, 300.5) == BG
    colours = {tuple(c) for c in img.reshape(-1, 3)}
    assert not colours & {(1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 20, 30)}  # path 0 lies wholly under path 1
    # colour bar: rows i = 0..99 at y = 900 + i from x = 1200 to 1250, half-width 0.75: the last covering row wins
    for r in range(1300):
        yc = SH - (r + 0.5)
        rows = [i for i in range(100) if abs(yc - (900 + i)) <= 0.75]
        want = R.red_blue_grad(max(rows) / 100) if rows else BG
        assert tuple(int(v) for v in img[r, 1225]) == want, r
        assert tuple(int(v) for v in img[r, 1195]) == BG and tuple(int(v) for v in img[r, 1255]) == BG
    assert R.red_blue_grad(0.0) == (255, 0, 0) and R.red_blue_grad(0.25) == (255, 0, 127)
    assert R.red_blue_grad(0.5) == (255, 0, 255) and R.red_blue_grad(1.0) == (0, 0, 255)
    # with a scenario: its path and obstacles under the flight paths, no spawn rectangle
    scn = make_scenario([(100.0, 200.0), (600.0, 400.0), (1100.5, 1000.5)], [(500.5, 300.5, 20.0)])
    img2 = R.plot_paths_host(scn, xy, lens, rgb, size=1300)
    assert tuple(img2[pix(500.5, 310.5)]) == OBST and tuple(img2[pix(500.5, 300.5)]) != OBST
    assert tuple(img2[pix(100.5, 200.5)]) == BLACK and tuple(img2[pix(50.5, 500.5)]) == BG
    # no path at all: the library draws nothing and the wrapper returns the background
    none = R.plot_paths_host(scn, xy[:, :0], lens[:0], rgb[:0], size=64)
    assert (none == 243).all()


def test_struct_sizes_and_constants(R, tmp_path):
    from drone2d_amd import abi

    hdr = os.path.join(REPO, "include", "d2d_render.h")
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void){",
            'printf("d2dr_view %zu\\n", sizeof(d2dr_view));', 'printf("d2d_scn %zu\\n", sizeof(d2d_scn));']
    for fname, _ in R.D2DRView._fields_:
        prog.append(f'printf("d2dr_view.{fname} %zu\\n", offsetof(d2dr_view, {fname}));')
    consts = {"D2DR_ABI_VERSION": R.ABI_VERSION, "D2DR_MIN_SIZE": R.MIN_SIZE, "D2DR_MAX_SIZE": R.MAX_SIZE,
              "D2DR_PATH_SAMPLES": R.PATH_SAMPLES, "D2DR_BAR_ROWS": R.BAR_ROWS, "D2DR_L_PATH": R.L_PATH,
              "D2DR_L_GUIDES": R.L_GUIDES, "D2DR_L_OBSTACLES": R.L_OBSTACLES, "D2DR_L_DRONE": R.L_DRONE,
              "D2DR_L_FORCES": R.L_FORCES, "D2DR_L_TRAIL": R.L_TRAIL, "D2DR_L_ALL": R.L_ALL, "D2DR_OK": R.E_OK,
              "D2DR_E_ARG": R.E_ARG, "D2DR_E_HIP": R.E_HIP, "D2DR_E_NOMEM": R.E_NOMEM}
    for k in consts:
        prog.append(f'printf("{k} %d\\n", (int){k});')
    prog.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(c)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                check=True).stdout.splitlines())
    assert int(out["d2dr_view"]) == C.sizeof(R.D2DRView) and int(out["d2d_scn"]) == C.sizeof(abi.D2DScn)
    for fname, _ in R.D2DRView._fields_:
        assert int(out[f"d2dr_view.{fname}"]) == getattr(R.D2DRView, fname).offset, fname
    for k, v in consts.items():
        assert int(out[k]) == v, k
    # the library exports every entry point the header declares, and the binding declares each
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    fns = sorted(set(re.findall(r"\b(d2dr_[a-z_]+)\s*\(", src)))
    lib = R.load()
    assert len(fns) == 9 and lib.d2dr_abi_version() == 1
    for f in fns:
        assert hasattr(lib, f) and f in R.SIGNATURES, f


def test_render_host_code_sanitized(tmp_path):
    """csrc/render/d2d_raster.h (primitive construction, coverage predicate, the CPU twins) as a stand-alone
    program under the address and undefined-behaviour sanitizers: tests/render_host_main.cpp lists the
    cases.  Nothing is preloaded and nothing sanitized is loaded into Python."""
    from drone2d_amd import _build

    exe = tmp_path / "render_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(_build.PKG_DIR, "csrc"),
                    os.path.join(REPO, "tests", "render_host_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_render_headers_are_build_dependencies(d2):
    """tests/test_build.py's render counterpart: every header d2d_render.hip includes is on the render
    library's dependency list, and the env library's list does not grow by them."""
    from drone2d_amd import _build

    deps = {os.path.normpath(p) for p in _build.RENDER_HDRS}
    todo, seen = [_build.RENDER_SRC], set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for line in open(f):
            m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
            if m:
                inc = os.path.normpath(os.path.join(os.path.dirname(f), m.group(1)))
                assert inc in deps, f"{inc} (included by {f}) is not in the render build's dependency list"
                todo.append(inc)
    assert len(seen) == 5  # d2d_render.hip, d2d_raster.h, d2d_pmath.h, d2d_render.h, drone2d.h
    assert not any("render" in os.path.basename(p) or "raster" in os.path.basename(p) for p in _build.env_headers())
    assert _build.HIPCC_FLAGS.count("-ffp-contract=off") == 1  # the host/device identity depends on it


def test_save_gif_needs_pillow(R, tmp_path):
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="Pillow"):
            R.save_gif(frames, str(tmp_path / "a.gif"))
    else:
        R.save_gif(frames, str(tmp_path / "a.gif"))
        assert open(tmp_path / "a.gif", "rb").read(6) in (b"GIF87a", b"GIF89a")


# ================================================================ GPU: device == host twin, byte for byte
CANARY = 4096


def _inputs(names, k, seed, trail_cap=24):
    """K frames cycling over the named scenarios with seeded random poses, obs, actions and trails."""
    from drone2d_amd.scenarios import create_test_scenario, free_flight

    def scen(n):
        if n == "wps3":
            return make_scenario(_curvy(3), [(600.0, 600.0, 45.0)])
        if n == "wps16":
            return make_scenario(_curvy(16), [(300.0 + 40 * i, 800.0, 12.0) for i in range(10)])
        if n.endswith("_free"):
            return free_flight(create_test_scenario(n[:-5], 1300, 1300))
        return create_test_scenario(n, 1300, 1300)

    base = [scen(n) for n in names]
    rng = np.random.default_rng(seed)
    scns = [base[i % len(base)] for i in range(k)]
    poses = [(rng.uniform(50, 1250), rng.uniform(50, 1250), rng.uniform(-1.5, 1.5), rng.uniform(-300, 300),
              rng.uniform(-300, 300)) for _ in range(k)]
    st = pose_state(k, poses)
    obs = rng.uniform(-1, 1, (k, 27)).astype(np.float32)
    act = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
    trail = np.cumsum(rng.uniform(-30, 30, (k, trail_cap, 2)), 1).astype(np.float32) + 650
    tl = rng.integers(0, trail_cap + 1, k).astype(np.int32)
    tl[0] = trail_cap
    return scns, st, obs, act, trail, tl


@pytest.fixture(scope="module")
def renderer(R):
    import torch

    r = R.Renderer(torch.device("cuda", 0), max_frames=128, max_trail=24)
    yield r
    r.close()


def _device_vs_host(R, renderer, scns, st, obs, act, trail, tl, size, layers=None):
    """Render on the device into a buffer with 4 KiB canaries on both sides; compare with the twin."""
    import torch

    layers = R.L_ALL if layers is None else layers
    h, w = R._size(size)
    k = len(scns)
    n = k * h * w * 3
    flat = torch.full((CANARY + n + CANARY,), 0xA5, dtype=torch.uint8, device=renderer.device)
    out = flat[CANARY:CANARY + n].view(k, h, w, 3)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    renderer.render(renderer.scn_tensor(scns), t(st), t(obs), t(act), t(trail), t(tl), size=size, layers=layers, out=out)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:CANARY] == 0xA5).all() and (got[CANARY + n:] == 0xA5).all(), "canary overwritten"
    want = R.render_host(scns, st, obs, act, trail, tl, size=size, layers=layers)
    frame = got[CANARY:CANARY + n].reshape(k, h, w, 3)
    bad = int((frame != want).any(-1).sum())
    assert bad == 0, f"{bad} pixels differ between device and host twin"
    return frame


ALL_SCN = ["S_corridor", "large", "corridor_free", "wps3", "wps16"]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [64, (96, 160), (70, 50), 8])
@pytest.mark.parametrize("k", [1, 3, 67])
def test_device_equals_twin(R, renderer, size, k):
    """Sizes 64x64, 96x160, 50 wide x 70 high (row bytes no multiple of 4, partial tiles on both edges) and
    8x8; 1, 3 and 67 frames (more than one wave of frames); S_corridor (58 circles), large (one r = 260
    circle over many tiles), corridor_free (no circles), the 3- and the 16-waypoint path."""
    frame = _device_vs_host(R, renderer, *_inputs(ALL_SCN, k, seed=k), size=size)
    assert len({tuple(c) for c in frame.reshape(-1, 3)}) >= (3 if size == 8 else 6)


@pytest.mark.gpu
def test_device_equals_twin_full_size(R, renderer):
    """One 1300x1300 frame (the reference's screen)."""
    _device_vs_host(R, renderer, *_inputs(["S_corridor"], 1, seed=5), size=1300)


@pytest.mark.gpu
def test_device_equals_twin_edge_states(R, renderer):
    """The stand-alone program's states: NaN, +-inf and +-1e300 in every state field, a drone wholly outside
    the screen, a zero-length velocity; and the same values in obs, act and trail."""
    bads = [np.nan, np.inf, -np.inf, 1e300, -1e300]
    scns, st, obs, act, trail, tl = _inputs(ALL_SCN, 18 * len(bads) + 2, seed=9)
    for j, bad in enumerate(bads):
        for f in range(18):
            st[f, 18 * j + f] = bad
    k = st.shape[1]
    st[:, k - 2] = pose_state(1, [(5000.0, -4000.0, -1.2, 10.0, 10.0)])[:, 0]
    st[:, k - 1] = pose_state(1, [(700.0, 300.0, 0.0, 0.0, 0.0)])[:, 0]
    _device_vs_host(R, renderer, scns, st, obs, act, trail, tl, size=64)
    for bad in bads:
        k = 4
        scns, st, obs, act, trail, tl = _inputs(ALL_SCN, k, seed=10)
        with np.errstate(over="ignore"):
            o2, a2, t2 = (np.full_like(a, bad) for a in (obs, act, trail))
        _device_vs_host(R, renderer, scns, st, o2, a2, t2, np.full(k, 24, np.int32), size=(70, 50))
        _device_vs_host(R, renderer, scns, np.full_like(st, bad), obs, act, trail, tl, size=(70, 50))


@pytest.mark.gpu
def test_device_equals_twin_null_inputs_and_layers(R, renderer):
    """NULL obs, act and trail, each alone and all together; every layer-mask bit alone, and none."""
    scns, st, obs, act, trail, tl = _inputs(ALL_SCN, 5, seed=11)
    for m in range(8):
        _device_vs_host(R, renderer, scns, st, None if m & 1 else obs, None if m & 2 else act,
                        None if m & 4 else trail, None if m & 4 else tl, size=(70, 50))
    seen = set()
    for bit in (R.L_PATH, R.L_GUIDES, R.L_OBSTACLES, R.L_DRONE, R.L_FORCES, R.L_TRAIL):
        f = _device_vs_host(R, renderer, scns, st, obs, act, trail, tl, size=96, layers=bit)
        seen.add(f.tobytes())
    assert len(seen) == 6
    assert (_device_vs_host(R, renderer, scns, st, obs, act, trail, tl, size=96, layers=0) == 243).all()
    import torch

    empty = renderer.render(renderer.scn_tensor(scns)[:0], torch.zeros(32, 0, dtype=torch.float64), size=64)
    assert tuple(empty.shape) == (0, 64, 64, 3)  # n_frames = 0: OK, nothing launched


def _plot_inputs(n_paths, max_len, seed):
    rng = np.random.default_rng(seed)
    steps = rng.uniform(-6, 6, (max_len, n_paths, 2))
    steps[..., 0] += 1.0
    xy = (np.cumsum(steps, 0) + rng.uniform(300, 500, (1, n_paths, 2))).astype(np.float32)
    xy[:, : max(1, n_paths // 2)] = xy[:, :1]  # the first half of the paths run through the same pixels
    lens = rng.integers(0, max_len + 1, n_paths).astype(np.int32)
    lens[0] = max_len
    rgb = rng.integers(0, 256, (n_paths, 3)).astype(np.uint8)
    return xy, lens, rgb


@pytest.mark.gpu
@pytest.mark.parametrize("n_paths", [1, 5, 100])
def test_plot_device_equals_twin(R, renderer, n_paths):
    """The plot for 1, 5 and 100 paths of up to 1100 points, several of them through the same pixels: two
    device runs are bitwise equal to each other and to the twin."""
    import torch
    from drone2d_amd.scenarios import create_test_scenario

    scn = create_test_scenario("corridor", 1300, 1300)
    xy, lens, rgb = _plot_inputs(n_paths, 1100, seed=n_paths)
    for size, rec in ((256, scn), ((200, 300), None)):
        h, w = R._size(size)
        n = h * w * 3
        runs = []
        for _ in range(2):
            flat = torch.full((CANARY + n + CANARY,), 0xA5, dtype=torch.uint8, device=renderer.device)
            renderer.plot_paths(renderer.scn_tensor([rec]) if rec is not None else None, torch.from_numpy(xy),
                                torch.from_numpy(lens), torch.from_numpy(rgb), size=size,
                                out=flat[CANARY:CANARY + n].view(h, w, 3))
            torch.cuda.synchronize()
            got = flat.cpu().numpy()
            assert (got[:CANARY] == 0xA5).all() and (got[CANARY + n:] == 0xA5).all(), "canary overwritten"
            runs.append(got[CANARY:CANARY + n].reshape(h, w, 3))
        want = R.plot_paths_host(rec, xy, lens, rgb, size=size)
        assert (runs[0] == runs[1]).all() and (runs[0] == want).all()
        assert tuple(rgb[0]) in {tuple(c) for c in want.reshape(-1, 3)} or n_paths > 1


@pytest.mark.gpu
def test_capacity_errors_leave_out_untouched(R):
    import torch

    dev = torch.device("cuda", 0)
    small = R.Renderer(dev, max_frames=2, max_trail=4, max_width=64, max_height=32)
    try:
        scns, st, obs, act, trail, tl = _inputs(["corridor"], 3, seed=1, trail_cap=4)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        cases = [dict(k=3, size=(32, 64)),      # more frames than max_frames
                 dict(k=2, size=(32, 65)),      # wider than max_width
                 dict(k=2, size=(33, 64)),      # higher than max_height
                 dict(k=2, size=(4, 64)),       # below the smallest picture
                 dict(k=2, size=(32, 4096))]    # above the largest
        for c in cases:
            k, (h, w) = c["k"], c["size"]
            out = torch.full((k, h, w, 3), 0x5A, dtype=torch.uint8, device=dev)
            with pytest.raises(R.RenderError, match="code 1"):
                small.render(small.scn_tensor(scns[:k]), t(st[:, :k]), t(obs[:k]), t(act[:k]), t(trail[:k]), t(tl[:k]),
                             size=(h, w), out=out)
            torch.cuda.synchronize()
            assert (out == 0x5A).all()
        xy, lens, rgb = _plot_inputs(3, 10, seed=2)
        out = torch.full((33, 64, 3), 0x5A, dtype=torch.uint8, device=dev)
        with pytest.raises(R.RenderError, match="code 1"):
            small.plot_paths(None, t(xy), t(lens), t(rgb), size=(33, 64), out=out)
        torch.cuda.synchronize()
        assert (out == 0x5A).all()
        with pytest.raises(ValueError):  # a trail longer than max_trail does not fit the ctx: refused, not cut
            small.render(small.scn_tensor(scns[:2]), t(st[:, :2]), t(obs[:2]), t(act[:2]),
                         torch.zeros(2, 9, 2), t(tl[:2]), size=32)
        ok = small.render(small.scn_tensor(scns[:2]), t(st[:, :2]), t(obs[:2]), t(act[:2]), t(trail[:2]), t(tl[:2]),
                          size=(32, 64))
        assert (ok.cpu().numpy() == R.render_host(scns[:2], st[:, :2], obs[:2], act[:2], trail[:2], tl[:2],
                                                  size=(32, 64))).all()
    finally:
        small.close()
    with pytest.raises(R.RenderError, match="code 1"):
        R.Renderer(dev, max_frames=0)
