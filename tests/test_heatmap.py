"""Arena maps on the CPU: heatmap.py's NumPy twin of libd2d_heat.so against brute force, against the
host build of csrc/heat/d2d_heat_core.h, and in the closed loop on the oracle backend.  Everything is
integer (or one of three single float32 operations), so every comparison is equality."""
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
F = np.float32
GRIDS = (1, 3, 64, 256)


# ------------------------------------------------------------------------------------------ references
def cell_ref(o, G):
    """include/d2d_heat.h's cell function, one float32 operation at a time on NumPy scalars."""
    o = F(o)
    if not (F(-1.0) <= o and o < F(1.0)):
        return -1
    u = F(F(o + F(1.0)) * F(0.5))
    return min(int(F(u * F(G))), G - 1)


def cell2_ref(ox, oy, gx, gy):
    cx, cy = cell_ref(ox, gx), cell_ref(oy, gy)
    return -1 if cx < 0 or cy < 0 else (gy - 1 - cy) * gx + cx


def class_ref(cause):
    c1, c2, c4, c5 = bool(cause & 1), bool(cause & 2), bool(cause & 4), bool(cause & 8)
    return 0 if c2 else (1 if c1 and not c4 and not c5 else 2)


def cell_inputs(G):
    """-1 and its neighbours, 1 - 2^-24, 1, every cell border 2k/G - 1 with its neighbours, NaN, +-inf."""
    v = [F(-1.0), F(1.0) - F(2.0 ** -24), F(1.0), F(0.0), F(np.nan), F(np.inf), F(-np.inf)]
    v += [F(2.0 * k / G - 1.0) for k in range(G + 1)]
    v = np.array(v, F)
    fin = v[np.isfinite(v)]
    return np.concatenate([v, np.nextafter(fin, F(np.inf)), np.nextafter(fin, F(-np.inf))]).astype(F)


@pytest.fixture(scope="module")
def hm(d2):
    from drone2d_amd import heatmap

    return heatmap


# ---------------------------------------------------------------------------------------- 1. the cell function
@pytest.mark.parametrize("G", GRIDS)
def test_cell_function(hm, G):
    o = cell_inputs(G)
    got = hm.cell(o, G)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, [cell_ref(x, G) for x in o])
    inside = (o >= -1) & (o < 1)
    assert (got[~inside] == -1).all() and (got[inside] >= 0).all() and (got[inside] < G).all()
    order = np.argsort(o[inside], kind="stable")
    assert (np.diff(got[inside][order]) >= 0).all()  # monotone in o
    assert hm.cell(F(1.0) - F(2.0 ** -24), G)[()] == G - 1 and hm.cell(F(-1.0), G)[()] == 0
    if G & (G - 1) == 0:
        # borders of a power-of-two grid are float32 values: cell k starts exactly there, and 2^-23 below
        # it (the resolution of o + 1 in [1, 2); a closer neighbour of a border below 0 rounds onto it)
        k = np.arange(G)
        b = (2.0 * k / G - 1.0).astype(F)
        np.testing.assert_array_equal(hm.cell(b, G), k)
        np.testing.assert_array_equal(hm.cell(b[1:] - F(2.0 ** -23), G), k[1:] - 1)


def test_cell2_rows_and_outside(hm):
    # row 0 is the top of the picture: the largest y; outside in either axis is outside
    assert hm.cell2(F(-1.0), F(0.99), 5, 3)[()] == 0 and hm.cell2(F(0.99), F(-1.0), 5, 3)[()] == 2 * 5 + 4
    for bad in (F(1.0), F(-1.5), F(np.nan), F(np.inf)):
        assert hm.cell2(bad, F(0.0), 5, 3)[()] == -1 and hm.cell2(F(0.0), bad, 5, 3)[()] == -1
    rng = np.random.default_rng(0)
    xy = rng.uniform(-1.1, 1.1, (200, 2)).astype(F)
    np.testing.assert_array_equal(hm.cell2(xy[:, 0], xy[:, 1], 5, 3), [cell2_ref(x, y, 5, 3) for x, y in xy])


def test_outcome_class_every_cause(hm):
    np.testing.assert_array_equal(hm.outcome_class(np.arange(16)), [class_ref(c) for c in range(16)])


# ------------------------------------------------------------------------------- 4. level, ramp and blend
def level_cases():
    peaks = (1, 2, 7, 255, 65025, 70_000_000, 2 ** 32 - 1)
    out = []
    for p in peaks:
        cs = sorted({0, 1, 2, p // 3, p // 2, p - 1, p} | {min(p, c) for c in (3, 10, 1000, 10 ** 6)})
        out += [(c, p) for c in cs if 0 <= c <= p]
    return out + [(0, 0)]


def test_isqrt_level_ramp_blend(hm):
    v = np.arange(65026, dtype=np.uint64)
    np.testing.assert_array_equal(hm.isqrt(v), [math.isqrt(int(x)) for x in v])
    big = [2 ** 32 - 1, 2 ** 32, (2 ** 32 - 1) * 65025, 2 ** 63, 2 ** 64 - 1]
    np.testing.assert_array_equal(hm.isqrt(np.array(big, np.uint64)), [math.isqrt(x) for x in big])
    for peak in (1, 7, 1000, 70_000_000):
        c = np.unique(np.r_[np.arange(min(peak, 3000) + 1), np.linspace(0, peak, 500).astype(np.int64)])
        lv = hm.level(c, peak)
        assert (np.diff(lv) >= 0).all() and lv[0] == 0 and lv[-1] == 255 and (lv[1:] >= 1).all()
        np.testing.assert_array_equal(lv[1:], [max(1, math.isqrt(int(x) * 65025 // peak)) for x in c[1:]])
    assert hm.level(1, 70_000_000)[0] == 1 and hm.level(5, 0)[0] == 0
    for den in (1, 3, 100, 2 ** 32 - 1):
        assert hm.rate_level(0, den)[0] == 0 and hm.rate_level(den, den)[0] == 255
        num = np.linspace(0, den, 50).astype(np.uint64)
        assert (np.diff(hm.rate_level(num, np.full(50, den, np.uint64))) >= 0).all()
    assert hm.rate_level(1, 2)[0] == 128 and hm.rate_level(1, 3)[0] == 85
    # the rate colours are render.red_blue_grad at level / 255
    from drone2d_amd.render import red_blue_grad

    # (in exact arithmetic: 510 f = 2 level is an integer, which red_blue_grad's float product 510.0 * (level /
    # 255.0) can miss from below by one rounding, so its truncation may sit one step under the exact value)
    exact = [(255, 0, 2 * lv) if 2 * lv < 255 else (2 * (255 - lv), 0, 255) for lv in range(256)]
    np.testing.assert_array_equal(hm.RATE_COLOURS, exact)
    floats = np.array([red_blue_grad(lv / 255.0) for lv in range(256)], np.int64)
    d = hm.RATE_COLOURS.astype(np.int64) - floats
    assert ((d == 0) | (d == 1)).all()
    np.testing.assert_array_equal(hm.RATE_COLOURS[[0, 255]], [red_blue_grad(0.0), red_blue_grad(1.0)])
    assert hm.RAMP.shape == (256, 3) and tuple(hm.RAMP[0]) == tuple(hm.ANCHORS[0]) and tuple(hm.RAMP[255]) == tuple(hm.ANCHORS[4])
    bg, col = np.arange(256), np.arange(256)[::-1]
    np.testing.assert_array_equal(hm.blend(bg, col, 0), bg)
    np.testing.assert_array_equal(hm.blend(bg, col, 255), col)
    np.testing.assert_array_equal(hm.blend(bg, col, 100), [(int(b) * 155 + int(c) * 100 + 127) // 255 for b, c in zip(bg, col)])
    # den < min_count is transparent, alpha 0 returns the background, alpha 255 the colour
    planes = np.zeros((1, 6, 1, 2), np.uint32)
    planes[0, hm.SPAWN, 0] = (4, 2)
    planes[0, hm.SPAWN_SUCCESS, 0] = (4, 0)
    back = np.full((1, 2, 3), 9, np.uint8)
    img = hm.images_host(planes, back, "spawn_success", alpha=255, min_count=3)
    np.testing.assert_array_equal(img[0, 0], [[0, 0, 255], [9, 9, 9]])
    np.testing.assert_array_equal(hm.images_host(planes, back, "spawn_success", alpha=255, min_count=1)[0, 0],
                                  [[0, 0, 255], [255, 0, 0]])
    np.testing.assert_array_equal(hm.images_host(planes, back, "spawn", alpha=0)[0], back)


# ------------------------------------------------------------------- 2. the host build of the core header
def test_heat_core_host_build_sanitized(hm, tmp_path):
    """csrc/heat/d2d_heat_core.h compiled as plain C into tests/heat_host_main.c under the address and
    undefined-behaviour sanitizers: its cell, class, isqrt, level, rate level, ramp, rate colour and blend
    equal the twin's on the cases of the tests above.  Nothing sanitized is loaded into Python."""
    from drone2d_amd import _build

    exe = tmp_path / "heat_host"
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", os.path.join(_build.PKG_DIR, "csrc"),
                    os.path.join(HERE, "heat_host_main.c"), "-o", str(exe)], check=True)
    lines, want = [], []

    def case(text, value):
        lines.append(text)
        want.append(" ".join(str(int(x)) for x in np.atleast_1d(value)))

    for G in GRIDS:
        o = cell_inputs(G)
        for x, c in zip(o, hm.cell(o, G)):
            case(f"c {int(x.view(np.uint32)):x} {G}", c)
    rng = np.random.default_rng(1)
    xy = np.r_[rng.uniform(-1.1, 1.1, (64, 2)).astype(F), np.array([[np.nan, 0], [0, np.inf], [1, 1], [-1, -1]], F)]
    for (x, y), c in zip(xy, hm.cell2(xy[:, 0], xy[:, 1], 5, 3)):
        case(f"p {int(x.view(np.uint32)):x} {int(y.view(np.uint32)):x} 5 3", c)
    for cause in range(16):
        case(f"k {cause}", hm.outcome_class(cause))
    for v in list(range(0, 65026, 97)) + [65025, 2 ** 32, (2 ** 32 - 1) * 65025, 2 ** 64 - 1]:
        case(f"q {v}", hm.isqrt(np.uint64(v)))
    for c, p in level_cases():
        case(f"l {c} {p}", hm.level(c, p))
    for num, den in ((0, 1), (1, 1), (1, 2), (1, 3), (2, 3), (0, 2 ** 32 - 1), (2 ** 32 - 1, 2 ** 32 - 1), (7, 9)):
        case(f"r {num} {den}", hm.rate_level(num, den))
    for lv in range(256):
        case(f"m {lv}", hm.RAMP[lv])
        case(f"t {lv}", hm.RATE_COLOURS[lv])
    for bg, col, a in ((0, 255, 0), (0, 255, 255), (9, 200, 100), (255, 0, 1), (255, 255, 254), (17, 3, 128)):
        case(f"b {bg} {col} {a}", hm.blend(bg, col, a))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert not bad, bad[:10]


def test_heat_headers_are_build_dependencies(hm):
    """Every header d2d_heat.hip includes is on the library's dependency list (a stale .so is rebuilt)."""
    import re

    from drone2d_amd import _build

    src = open(_build.HEAT_SRC).read()
    names = set(re.findall(r'#include "([^"]+)"', src))
    names |= set(re.findall(r'#include "([^"]+)"', open(os.path.join(_build.PKG_DIR, "csrc", "heat", "d2d_heat_core.h")).read()))
    assert {os.path.basename(n) for n in names} == {os.path.basename(p) for p in _build.HEAT_HDRS}
    assert all(os.path.exists(p) for p in _build.HEAT_HDRS)
    assert "-ffp-contract=off" in _build.HIPCC_FLAGS


# --------------------------------------------------------------------------- 3. HostMaps.step vs brute force
N, T, GROUPS, GY, GX = 7, 9, 3, 3, 5
NEVER, OUTSIDE_SPAWN = 5, 6


def synthetic_episodes():
    """Nine steps of seven envs: positions in and around the arena, env 6 spawned outside, env 5 never
    done; the six first episodes end with causes 2, 1, 4, 8, 3 and 5, and the later episodes of the same
    envs (which the maps must ignore) with the other nine combinations."""
    rng = np.random.default_rng(5)
    obs0 = rng.uniform(-1, 1, (N, 27)).astype(F)
    obs0[OUTSIDE_SPAWN, 6:8] = (F(1.25), F(0.0))
    obs = rng.uniform(-1.15, 1.15, (T, N, 27)).astype(F)
    tobs = rng.uniform(-1.15, 1.15, (T, N, 27)).astype(F)
    obs[1, 0, 6], tobs[3, 1, 7] = F(np.nan), F(1.0)
    term, trunc = np.zeros((T, N), bool), np.zeros((T, N), bool)
    info = np.zeros((T, N, 12), F)
    first = {0: (2, 2), 1: (3, 1), 2: (0, 4), 3: (8, 8), 4: (4, 3), 6: (5, 5)}  # env: (step, cause)
    later = [6, 7, 9, 10, 11, 12, 13, 14, 15]
    for i, (t, cause) in first.items():
        (trunc if cause == 4 else term)[t, i] = True
        info[t, i, 8], info[t, i, 7] = cause, t + 1
    for cause, (t, i) in zip(later, [(4, 0), (6, 0), (8, 0), (5, 1), (7, 1), (2, 2), (4, 2), (6, 4), (7, 6)]):
        term[t, i] = True
        info[t, i, 8], info[t, i, 7] = cause, 2
    group = np.array([0, 1, 2, 2, 1, 0, 1], np.int32)  # not contiguous
    return obs0, obs, tobs, term, trunc, info, group, first


def brute_force(obs0, obs, tobs, term, trunc, info, group):
    planes = np.zeros((GROUPS, 6, GY * GX), np.uint32)
    outside = np.zeros((GROUPS, 6), np.uint32)

    def put(g, plane, c):
        if c < 0:
            outside[g, plane] += 1
        else:
            planes[g, plane, c] += 1

    alive = [True] * N
    spawn = [cell2_ref(obs0[i, 6], obs0[i, 7], GX, GY) for i in range(N)]
    history = []
    for t in range(T):
        for i in range(N):
            if not alive[i]:
                continue
            done = bool(term[t, i] or trunc[t, i])
            src = tobs if done else obs
            c = cell2_ref(src[t, i, 6], src[t, i, 7], GX, GY)
            g = int(group[i])
            put(g, 0, c)
            if done:
                k = class_ref(int(info[t, i, 8]))
                put(g, 1, spawn[i])
                if k == 0:
                    put(g, 2, spawn[i])
                if k == 1:
                    put(g, 3, spawn[i])
                    put(g, 4, c)
                if k == 2:
                    put(g, 5, c)
                alive[i] = False
        history.append((planes.reshape(GROUPS, 6, GY, GX).copy(), outside.copy(), list(alive)))
    return history, spawn


def test_host_maps_step_against_brute_force(hm):
    obs0, obs, tobs, term, trunc, info, group, first = synthetic_episodes()
    history, spawn = brute_force(obs0, obs, tobs, term, trunc, info, group)
    m = hm.HostMaps(N, (GY, GX), group, GROUPS)
    m.begin(obs0)
    np.testing.assert_array_equal(m.spawn_cell, spawn)
    assert m.spawn_cell[OUTSIDE_SPAWN] == -1
    for t in range(T):
        m.step(obs[t], term[t], trunc[t], tobs[t], info[t])
        c = m.counts()
        np.testing.assert_array_equal(c["planes"], history[t][0])
        np.testing.assert_array_equal(c["outside"], history[t][1])
        np.testing.assert_array_equal(m.alive != 0, history[t][2])
    planes, outside = c["planes"].astype(np.int64), c["outside"].astype(np.int64)
    lens = np.array([first[i][0] + 1 if i in first else T for i in range(N)])
    for g in range(GROUPS):
        in_g = group == g
        assert planes[g, hm.VISIT].sum() + outside[g, hm.VISIT] == lens[in_g].sum()
        assert planes[g, hm.SPAWN].sum() + outside[g, hm.SPAWN] == sum(1 for i in first if group[i] == g)
    assert (planes[:, hm.SPAWN_SUCCESS] + planes[:, hm.SPAWN_COLLISION] <= planes[:, hm.SPAWN]).all()
    assert outside[:, hm.VISIT].sum() > 0 and outside[1, hm.SPAWN] == 1 and m.alive[NEVER] == 1
    assert planes[:, hm.END_COLLISION].sum() + outside[:, hm.END_COLLISION].sum() == 1  # cause 1 alone
    assert planes[:, hm.END_OTHER].sum() + outside[:, hm.END_OTHER].sum() == 3          # causes 4, 8, 5

    # the batch form over the same episodes as a recorded flight buffer
    xy = np.full((T, N, 2), np.nan, F)
    rows = np.zeros((N, 12), F)
    finished = np.zeros(N, bool)
    for i in range(N):
        for t in range(lens[i]):
            done = term[t, i] or trunc[t, i]
            xy[t, i] = (tobs if done else obs)[t, i, 6:8]
        if i in first:
            finished[i], rows[i] = True, info[first[i][0], i]
    f = hm.from_flight(obs0[:, 6:8], xy, finished, rows, group, GROUPS, (GY, GX))
    np.testing.assert_array_equal(f["planes"], c["planes"])
    np.testing.assert_array_equal(f["outside"], c["outside"])
    m.clear()
    assert not m.counts()["planes"].any() and not m.counts()["outside"].any()


def test_refusals_on_the_host(hm):
    for grid in (0, 257, (3, 0), (300, 4), "x"):
        with pytest.raises(ValueError):
            hm.HostMaps(4, grid)
    with pytest.raises(ValueError, match="env_group"):
        hm.HostMaps(4, 8, [0, 1, 2, 3], 3)
    with pytest.raises(ValueError, match="env_group"):
        hm.HostMaps(4, 8, [0, -1, 0, 0], 2)
    with pytest.raises(ValueError, match="2\\^32"):
        hm.HostMaps(65536, 8, cap=65536)
    hm.HostMaps(65536, 8, cap=65535)
    with pytest.raises(ValueError, match="HIP"):
        hm.ArenaMaps(4, 8, device="cpu")


# ------------------------------------------------------------------------- 5. images against brute force
def images_brute(planes, bg, mode, pa, pb, alpha, min_count, ramp, rate_colours):
    G, _, gy, gx = planes.shape
    shared = bg.ndim == 3
    h, w = bg.shape[-3], bg.shape[-2]
    out = np.empty((G, h, w, 3), np.uint8)
    for g in range(G):
        peak = int(planes[g, pa].max())
        for y in range(h):
            for x in range(w):
                cy, cx = y * gy // h, x * gx // w
                b = bg[y, x] if shared else bg[g, y, x]
                a = int(planes[g, pa, cy, cx])
                if mode == 0:
                    lv = 0 if a == 0 or peak == 0 else max(1, math.isqrt(a * 65025 // peak))
                    paint, col = lv > 0, ramp[lv]
                else:
                    den = int(planes[g, pb, cy, cx])
                    paint = den >= max(min_count, 1)
                    col = rate_colours[(510 * a + den) // (2 * den)] if paint else None
                out[g, y, x] = [(int(b[k]) * (255 - alpha) + int(col[k]) * alpha + 127) // 255 for k in range(3)] \
                    if paint else b
    return out


def image_planes(G, gy, gx, seed=3):
    """Planes with empty cells, a peak-0 VISIT plane in the last group and SPAWN_SUCCESS <= SPAWN."""
    rng = np.random.default_rng(seed)
    planes = rng.integers(0, 50, (G, 6, gy, gx)).astype(np.uint32)
    planes[:, :, 0, 0] = 0
    planes[0, 0].flat[-1] = 70_000_000
    planes[G - 1, 0] = 0
    planes[:, 2] = np.minimum(planes[:, 2], planes[:, 1])
    return planes


def test_host_images_against_brute_force(hm):
    G, gy, gx, h, w = 2, 3, 5, 37, 53
    planes = image_planes(G, gy, gx)
    rng = np.random.default_rng(4)
    shared = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    per_group = rng.integers(0, 256, (G, h, w, 3)).astype(np.uint8)
    m = hm.HostMaps(4, (gy, gx), n_groups=G)
    m.planes[...] = planes
    for bg in (shared, per_group):
        for which, alpha, mc in (("density", 200, 1), (hm.VISIT, 255, 1), ("spawn_success", 180, 1),
                                 ((hm.SPAWN_SUCCESS, hm.SPAWN), 255, 20)):
            mode, pa, pb = hm.picture(which)
            want = images_brute(planes, bg, mode, pa, pb, alpha, mc, hm.RAMP, hm.RATE_COLOURS)
            got = m.images(bg, which, alpha=alpha, min_count=mc)
            assert got.dtype == np.uint8 and got.shape == (G, h, w, 3)
            np.testing.assert_array_equal(got, want)
    # the peak-0 plane leaves its background untouched
    np.testing.assert_array_equal(m.images(per_group, "density")[G - 1], per_group[G - 1])
    with pytest.raises(ValueError):
        m.images(per_group[:1], "density")
    with pytest.raises(ValueError):
        hm.picture("nonsense")


# ------------------------------------------------------------------ 6. the closed loop on the oracle backend
class _Tap:
    """An oracle batch that also feeds every reset and step to a ``HostMaps``, step by step."""

    def __init__(self, be, maps):
        self._be, self._maps = be, maps

    def __getattr__(self, name):
        return getattr(self._be, name)

    def reset(self, *a, **kw):
        obs = self._be.reset(*a, **kw)
        self._maps.begin(obs)
        return obs

    def step(self, actions):
        out = self._be.step(actions)
        self._maps.step(out[0], out[2], out[3], self._be.terminal_obs, out[4])
        return out


def test_closed_loop_on_oracle_backend(hm):
    from oracle_backend import OracleVecBackend

    from drone2d_amd import evaluate, harness
    from drone2d_amd.config import ENV_TEST_CONFIG

    n, kw = 8, dict(ENV_TEST_CONFIG, scenario="corridor")
    pol = harness.MlpActor.from_npz(os.path.join(GOLD, "agent_17_90.npz"))
    be = OracleVecBackend(n, seed=3, **kw)
    stepwise = hm.HostMaps(n, 8)
    m = evaluate.evaluate_policy(_Tap(be, stepwise), pol, seed=3, flight_paths=True, maps=8)
    be.close()
    be2 = OracleVecBackend(n, seed=3, **kw)
    bare = evaluate.evaluate_policy(be2, pol, seed=3, flight_paths=True)
    be2.close()
    assert set(m) == set(bare) | {"maps"} and m["unfinished"] == 0
    for k in bare:
        np.testing.assert_array_equal(np.asarray(m[k]), np.asarray(bare[k]), err_msg=k)
    r = m["maps"]
    assert r["planes"].shape == (6, 8, 8) and r["planes"].dtype == np.uint32 and r["outside"].shape == (6,)
    f = hm.from_flight(r["spawn_obs"], r["flight_obs"], r["finished"], r["rows"], None, 1, 8)
    np.testing.assert_array_equal(r["planes"], f["planes"][0])
    np.testing.assert_array_equal(r["outside"], f["outside"][0])
    again = hm.from_result(m)
    np.testing.assert_array_equal(again["planes"], r["planes"])
    # the step-by-step twin saw the same episodes
    c = stepwise.counts()
    np.testing.assert_array_equal(c["planes"][0], r["planes"])
    np.testing.assert_array_equal(c["outside"][0], r["outside"])
    assert int(r["planes"][hm.VISIT].sum()) + int(r["outside"][hm.VISIT]) == int(m["time_spent"].sum())
    assert int(r["planes"][hm.SPAWN].sum()) + int(r["outside"][hm.SPAWN]) == n
    assert int(r["planes"][hm.SPAWN_SUCCESS].sum()) == m["successes"]
    # per-policy groups through the bank on the same backend
    be3 = OracleVecBackend(n, seed=3, **kw)
    res = evaluate.evaluate_policies(be3, [pol, pol], np.arange(n) % 2, seed=3, flight_paths=True, maps=(4, 8))
    be3.close()
    for p, rp in enumerate(res):
        assert rp["maps"]["planes"].shape == (6, 4, 8)
        np.testing.assert_array_equal(rp["maps"]["planes"], hm.from_result(rp)["planes"])
        assert int(rp["maps"]["planes"][hm.SPAWN].sum()) + int(rp["maps"]["outside"][hm.SPAWN]) == n // 2


def test_maps_refused_with_two_ranks(hm, monkeypatch):
    from drone2d_amd import evaluate, harness

    monkeypatch.setattr(harness, "_dist_world", lambda: (None, 0, 2))
    with pytest.raises(ValueError, match="rank"):
        evaluate.evaluate_policy(object(), None, maps=8)
    with pytest.raises(ValueError, match="rank"):
        evaluate.evaluate_policies(object(), None, None, maps=8)


def test_write_results_writes_maps_npz(hm, tmp_path, monkeypatch):
    import torch

    from drone2d_amd import harness

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # the pictures need a device; the npz does not
    planes = image_planes(1, 4, 4)[0]
    m = {"collisions": np.zeros(2, np.int64), "rewards": np.ones(2), "apes": np.ones(2), "time_spent": np.ones(2, np.int64),
         "successes": 2, "fails": 0, "unfinished": 0, "maps": {"planes": planes, "outside": np.arange(6, dtype=np.uint32)}}
    harness.write_results(m, str(tmp_path), "corridor", "17", "agent")
    with np.load(tmp_path / "maps.npz") as z:
        np.testing.assert_array_equal(z["planes"], planes)
        np.testing.assert_array_equal(z["outside"], np.arange(6))
