"""Arena maps on an MI355X: libd2d_heat.so against heatmap.py's NumPy twin -- the step kernel plane for
plane on both aggregation paths, the pictures, the closed loops of ``evaluate_policy`` (eager, replayed,
``EvalLoop``) and ``sweep`` against ``from_flight`` of their own flight buffers, and the refusals.  The
counts are integers: every comparison is equality."""
import os

import numpy as np
import pytest
import torch

from test_heatmap import image_planes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
AGENT = os.path.join(HERE, "golden", "agent_17_90.npz")
F = np.float32


def _test_kw(**over):
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, **over)


@pytest.fixture(scope="module")
def hm(d2):
    from drone2d_amd import heatmap

    return heatmap


@pytest.fixture(scope="module")
def policy(d2):
    from drone2d_amd.ppo import ActorCritic

    return ActorCritic.from_agent_npz(AGENT).cuda()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _positions(rng, shape, gx, gy):
    """Observation rows whose [6:8] mix cell interiors, exact cell borders, the arena's edges, outside, NaN and inf."""
    obs = rng.uniform(-1, 1, shape + (27,)).astype(F)
    xy = rng.uniform(-1.05, 1.05, shape + (2,)).astype(F)
    kind = rng.integers(0, 10, shape)
    xy[kind == 0, 0] = (2.0 * rng.integers(0, gx + 1, int((kind == 0).sum())) / gx - 1.0).astype(F)
    xy[kind == 1, 1] = (2.0 * rng.integers(0, gy + 1, int((kind == 1).sum())) / gy - 1.0).astype(F)
    special = np.array([-1.0, 1.0, 1.0 - 2.0 ** -24, np.nan, np.inf, -np.inf, 1.5, np.nextafter(F(-1), F(-2))], F)
    xy[kind == 2, 0] = special[rng.integers(0, len(special), int((kind == 2).sum()))]
    xy[kind == 3, 1] = special[rng.integers(0, len(special), int((kind == 3).sum()))]
    obs[..., 6:8] = xy
    return obs


def _same_counts(dev, host):
    d, h = dev.counts(), host.counts()
    assert d["planes"].dtype == np.uint32 and d["planes"].shape == h["planes"].shape
    np.testing.assert_array_equal(d["planes"], h["planes"])
    np.testing.assert_array_equal(d["outside"], h["outside"])


def _drive(hm, n, T, grid, group, n_groups, path, seed, p_done=0.12, hot=False):
    """A device map and its twin over T synthetic steps; yields after every step."""
    gy, gx = hm.parse_grid(grid)
    rng = np.random.default_rng(seed)
    dev = hm.ArenaMaps(n, grid, group, n_groups, device="cuda", cap=T, path=path)
    host = hm.HostMaps(n, grid, group, n_groups, cap=T)
    obs0 = _positions(rng, (n,), gx, gy)
    if hot:
        obs0[:, 6:8] = (F(0.3), F(-0.2))
    dev.begin(_dev(obs0))
    host.begin(obs0)
    for t in range(T):
        obs, tobs = _positions(rng, (n,), gx, gy), _positions(rng, (n,), gx, gy)
        if hot:
            obs[:, 6:8] = tobs[:, 6:8] = (F(0.3), F(-0.2))
        term = rng.random(n) < p_done
        trunc = rng.random(n) < p_done / 3
        info = np.zeros((n, 12), F)
        info[:, 8] = rng.integers(1, 16, n)
        info[:, 7] = t + 1
        dev.step(_dev(obs), _dev(term), _dev(trunc), _dev(tobs), _dev(info))
        host.step(obs, term, trunc, tobs, info)
        yield dev, host
    dev.close()


# ------------------------------------------------------------------------------ 1. the step kernel vs the twin
@pytest.mark.parametrize("path", [0, 1, 2])
def test_step_kernel_matches_twin_after_every_step(hm, path):
    """n = 130 (two waves and two lanes), groups of 1, 64 and 65 envs (a border inside a wave), grid 8 x 8."""
    n = 130
    group = np.r_[np.zeros(1), np.ones(64), np.full(65, 2)].astype(np.int32)
    steps = 0
    for dev, host in _drive(hm, n, 12, 8, group, 3, path, seed=11):
        _same_counts(dev, host)
        np.testing.assert_array_equal(dev.alive.cpu().numpy(), host.alive)
        np.testing.assert_array_equal(dev.spawn_cell.cpu().numpy(), host.spawn_cell)
        steps += 1
    c = host.counts()
    assert steps == 12 and c["outside"].sum() > 0 and (c["planes"].sum(axis=(0, 2, 3)) > 0).all()
    assert 0 < host.alive.sum() < n  # some envs ended their first episode, some are still flying


# ------------------------------------------------------------------------------------ 2. contention and paths
@pytest.mark.parametrize("path", [0, 1, 2])
def test_every_env_in_one_cell(hm, path):
    n = 4096
    for dev, host in _drive(hm, n, 3, 64, None, None, path, seed=12, hot=True):
        _same_counts(dev, host)
    c = host.counts()
    assert np.count_nonzero(c["planes"][0, hm.VISIT]) == 1 and c["planes"][0, hm.VISIT].max() > 2 * n


@pytest.mark.parametrize("grid", [1, 64, 256, (256, 3)])
def test_random_cells_noncontiguous_groups(hm, grid):
    """env_group = i % 5; 256 x 256 is beyond the LDS table's grids (the wave-combined global path)."""
    n = 4096
    group = (np.arange(n) % 5).astype(np.int32)
    runs = []
    for _ in range(2):
        for dev, host in _drive(hm, n, 4, grid, group, 5, 0, seed=13):
            last = dev.counts()
        np.testing.assert_array_equal(last["planes"], host.counts()["planes"])
        np.testing.assert_array_equal(last["outside"], host.counts()["outside"])
        runs.append(last)
    np.testing.assert_array_equal(runs[0]["planes"], runs[1]["planes"])
    np.testing.assert_array_equal(runs[0]["outside"], runs[1]["outside"])


def test_table_is_emptied_between_chunks(hm):
    """More envs than four passes of the 256 workgroups on random cells of a 128 x 128 grid under the table
    path: some workgroups walk five 256-env chunks whose keys hardly repeat (about 950 new keys each while
    most envs end their episode), so their table passes 3 071 keys and is emptied before the fifth."""
    n = 4 * 256 * 256 + 256 * 40 + 7
    group = (np.arange(n) % 3).astype(np.int32)
    for dev, host in _drive(hm, n, 2, 128, group, 3, 1, seed=14, p_done=0.9):
        _same_counts(dev, host)
    dev2 = hm.ArenaMaps(4, 8, device="cuda")
    dev2.clear()
    assert not dev2.counts()["planes"].any()


# --------------------------------------------------------------------------------------------- 3. the pictures
@pytest.mark.parametrize("gy,gx,h,w", [(8, 8, 37, 53), (64, 64, 256, 256)])
def test_images_match_twin(hm, gy, gx, h, w):
    G = 3
    planes = image_planes(G, gy, gx)
    rng = np.random.default_rng(6)
    shared = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    per_group = rng.integers(0, 256, (G, h, w, 3)).astype(np.uint8)
    dev = hm.ArenaMaps(4, (gy, gx), n_groups=G, device="cuda")
    dev.planes.copy_(_dev(planes.view(np.int32)))
    for bg in (shared, per_group):
        for which, alpha, mc in (("density", 200, 1), ("crashes", 255, 1), ("spawn_success", 180, 1),
                                 ((hm.SPAWN_SUCCESS, hm.SPAWN), 255, 20), (hm.SPAWN, 0, 1)):
            got = dev.images(_dev(bg), which, alpha=alpha, min_count=mc)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (G, h, w, 3)
            np.testing.assert_array_equal(got.cpu().numpy(), hm.images_host(planes, bg, which, alpha, mc))
    out = dev.images(per_group, "density").cpu().numpy()  # (a NumPy background is moved to the device)
    np.testing.assert_array_equal(out[G - 1], per_group[G - 1])  # the peak-0 plane paints nothing
    np.testing.assert_array_equal(hm.paint(planes, shared, "density").cpu().numpy(), hm.images_host(planes, shared))
    dev.close()


# ---------------------------------------------------------------------------------------- 4. evaluate_policy
def _same_but_maps(m, ref):
    assert set(m) == set(ref) | {"maps"}
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(m[k], v, err_msg=k)  # NaN == NaN here
        else:
            assert m[k] == v, k


def _planes_equal_flight(hm, m, grid):
    r = m["maps"]
    gy, gx = hm.parse_grid(grid)
    assert r["planes"].shape == (6, gy, gx) and r["planes"].dtype == np.uint32
    f = hm.from_result(m)
    np.testing.assert_array_equal(r["planes"], f["planes"])
    np.testing.assert_array_equal(r["outside"], f["outside"])
    assert int(r["planes"][hm.VISIT].sum()) + int(r["outside"][hm.VISIT]) == int(m["time_spent"].sum())
    assert int(r["planes"][hm.SPAWN_SUCCESS].sum()) + int(r["outside"][hm.SPAWN_SUCCESS]) == m["successes"]


def test_evaluate_policy_maps(d2, hm, policy):
    from drone2d_amd import evaluate

    n, kw = 256, _test_kw(scenario="corridor")

    def fly(**ev):
        venv = d2.Drone2dVecEnv(n, seed=6, with_info=True, **kw)
        m = evaluate.evaluate_policy(venv, policy, seed=6, flight_paths=True, **ev)
        venv.close()
        return m

    bare, eager, replayed = fly(), fly(maps=16), fly(maps=16, graph=True)
    assert bare["unfinished"] == 0
    for m in (eager, replayed):
        _same_but_maps(m, bare)
        _planes_equal_flight(hm, m, 16)
    np.testing.assert_array_equal(replayed["maps"]["planes"], eager["maps"]["planes"])
    assert eager["maps"]["planes"][hm.VISIT].max() > 0

    venv = d2.Drone2dVecEnv(n, seed=6, with_info=True, **kw)
    loop = evaluate.EvalLoop(venv, policy, flight_paths=True, graph=True, maps=16)
    for _ in range(2):
        fin, rows, xy, nobs, _, _ = loop.run(6)
        c = loop.maps.counts()
        np.testing.assert_array_equal(c["planes"][0], eager["maps"]["planes"])
        np.testing.assert_array_equal(c["outside"][0], eager["maps"]["outside"])
    assert loop.captures == 1
    venv.close()


# -------------------------------------------------------------------------------------------------- 5. sweep
def test_sweep_maps(d2, hm, policy):
    from drone2d_amd import evaluate
    from drone2d_amd.ppo import ActorCritic

    torch.manual_seed(1)
    other = ActorCritic().cuda()
    bank = evaluate.PolicyBank([policy, other], names=["shipped", "fresh"], device="cuda")
    scns = ["corridor", "large"]
    res = evaluate.sweep(bank, scns, 8, seed=9, flight_paths=True, maps=16)
    bare = evaluate.sweep(bank, scns, 8, seed=9, flight_paths=True)
    seen = []
    for name in bank.names:
        for scn in scns:
            m = res[name][scn]
            _same_but_maps(m, bare[name][scn])
            _planes_equal_flight(hm, m, 16)
            assert int(m["maps"]["planes"][hm.SPAWN].sum()) + int(m["maps"]["outside"][hm.SPAWN]) == 8
            seen.append(m["maps"]["planes"])
    assert any(not np.array_equal(seen[0], s) for s in seen[1:])


def test_write_results_draws_the_maps(d2, hm, policy, tmp_path):
    from drone2d_amd import evaluate, harness

    venv = d2.Drone2dVecEnv(64, seed=2, with_info=True, **_test_kw(scenario="corridor"))
    m = evaluate.evaluate_policy(venv, policy, seed=2, maps=32)
    venv.close()
    harness.write_results(m, str(tmp_path), "corridor", "17", "agent")
    with np.load(tmp_path / "maps.npz") as z:
        np.testing.assert_array_equal(z["planes"], m["maps"]["planes"])
    for name in ("density", "spawn_success", "crashes"):
        assert (tmp_path / "plots" / f"corridor_{name}.png").stat().st_size > 1000
    assert not (tmp_path / "plots" / "corridor.png").exists()  # no flight paths were asked for
    pics = harness.plot_maps(m, "corridor", size=128)
    bg = harness.plot_background("corridor", size=128).cpu().numpy()
    want = hm.images_host(m["maps"]["planes"][None], bg, "density")[0]
    np.testing.assert_array_equal(pics["density"], want)
    assert (pics["density"] != bg).any()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(d2, hm, policy, monkeypatch):
    import ctypes as C

    from drone2d_amd import evaluate, harness

    for grid in (0, 257, (8, 0)):
        with pytest.raises(ValueError, match="grid"):
            hm.ArenaMaps(16, grid, device="cuda")
    with pytest.raises(ValueError, match="env_group"):
        hm.ArenaMaps(4, 8, [0, 1, 2, 3], 3, device="cuda")
    with pytest.raises(ValueError, match="2\\^32"):
        hm.ArenaMaps(65536, 8, device="cuda", cap=65536)
    # the library checks its arguments too, and launches nothing
    am = hm.ArenaMaps(16, 8, device="cuda")
    rng = np.random.default_rng(0)
    obs, tobs = _dev(_positions(rng, (16,), 8, 8)), _dev(_positions(rng, (16,), 8, 8))
    done, info = _dev(np.ones(16, bool)), _dev(np.full((16, 12), 1, F))
    am.begin(obs)
    am.step(obs, done, done, tobs, info)  # (a valid call: every pointer of the record is set)
    before = am.counts()
    am.alive.fill_(1)
    a = hm.D2DHeatArgs.from_buffer_copy(am._args)
    for field, value in (("gx", 0), ("gy", 257), ("n", 0), ("n_groups", 0), ("obs_dim", 26), ("path", 3), ("planes", None)):
        b = hm.D2DHeatArgs.from_buffer_copy(a)
        setattr(b, field, value)
        assert am._lib.d2d_heat_step(C.byref(b), None) == 1, field
    torch.cuda.synchronize()
    np.testing.assert_array_equal(am.counts()["planes"], before["planes"])
    venv = d2.Drone2dVecEnv(8, seed=1, with_info=True, **_test_kw(scenario="corridor"))
    with pytest.raises(ValueError, match="grid"):
        evaluate.evaluate_policy(venv, policy, maps=0)
    monkeypatch.setattr(harness, "_dist_world", lambda: (None, 0, 2))
    with pytest.raises(ValueError, match="rank"):
        evaluate.evaluate_policy(venv, policy, maps=8)
    with pytest.raises(ValueError, match="rank"):
        evaluate.sweep([policy], ["corridor"], 2, maps=8)
    venv.close()
