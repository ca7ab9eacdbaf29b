"""libd2d_monitor.so on an MI355X: the device digest against its NumPy twin bit for bit (synthetic rows,
every batch-size edge and the strided walk; real env outputs), captured into a HIP graph, inside
``PPO``'s fused rollout, and its argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 50


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _synthetic(n, seed=0):
    """50 steps of hand-rolled outputs for n envs: random done masks (p = 0.15), every cause combination,
    inf / NaN collision-avoidance terms, +inf clearances; and a random initial ``live``.  The sums must
    depend on the order of addition, or a comparison of bits says nothing about the order (float64
    sums of N(0, 3) float32 values are exact in any order): the APE and the return of every done row, and
    the path-progression term of 6 % of all rows (it reaches the episode sums), are +-m 2^e with a 24-bit
    m in [1, 2) and e uniform in 0..60, so nearly every addition rounds, differently in another order."""
    rng = np.random.default_rng(1000 * seed + n)
    info = rng.normal(0.0, 3.0, (STEPS, n, 12)).astype(np.float32)
    ca = info[:, :, 0]
    u = rng.random((STEPS, n))
    ca[u < 0.01] = np.inf
    ca[(u >= 0.01) & (u < 0.02)] = -np.inf
    ca[(u >= 0.02) & (u < 0.03)] = np.nan
    d = np.abs(info[:, :, 6]) * 50
    d[rng.random((STEPS, n)) < 0.3] = np.inf
    info[:, :, 6] = d
    info[:, :, 7] = rng.integers(1, 1101, (STEPS, n))
    done = rng.random((STEPS, n)) < 0.15
    info[:, :, 8] = np.where(done, rng.integers(1, 16, (STEPS, n)), 0)
    term = done & (rng.random((STEPS, n)) < 0.8)
    trunc = done & ~term
    live = (rng.random(n) < 0.8).astype(np.uint8)
    for col, where in ((9, done), (10, done), (2, rng.random((STEPS, n)) < 0.06)):
        wide = rng.uniform(1.0, 2.0, (STEPS, n)) * 2.0 ** rng.integers(0, 61, (STEPS, n))
        wide *= rng.choice([-1.0, 1.0], (STEPS, n))
        info[:, :, col][where] = wide.astype(np.float32)[where]
    return term, trunc, info, live


def _twin_run(n, n_blocks, data):
    """The twin's two flushed vectors for ``data``, and the twin."""
    from drone2d_amd.monitor import monitor_host

    term, trunc, info, live = data
    twin = monitor_host(n, n_blocks)
    twin.live[:] = live
    want = []
    for t in range(STEPS):
        twin.step(term[t], trunc[t], info[t])
        if t in (STEPS // 2, STEPS - 1):
            want.append(twin.flush())
    return want, twin


def _bits(vecs):
    return np.array(vecs).view(np.int64)


def _reorder(data, group, sub):
    """``data`` with the envs of every full ``group`` rearranged: its ``sub``-sized pieces in reverse
    order.  (64, 1) reverses the lanes of each wave, (256, 64) the waves of each chunk: the same
    episodes, deposited in another order."""
    term, trunc, info, live = data
    n = len(live)
    perm = np.arange(n)
    for s in range(0, n - n % group, group):
        perm[s:s + group] = perm[s:s + group].reshape(group // sub, sub)[::-1].ravel()
    return term[:, perm], trunc[:, perm], info[:, perm], live[perm]


def check_order_sensitive(n):
    """The inputs of the device comparison distinguish summation orders: on the twin, the same episodes
    with the lanes of every wave reversed, with the waves of every chunk reversed, or walked with
    another ``n_blocks`` (another association of the chunk sums) give other bits.  So a device that
    added lanes, waves, chunks or rows in another order than include/d2d_monitor.h states, or with
    atomics, could not match the twin on them.  (Called here before the device is compared, and by
    tests/test_monitor.py, which needs no GPU.)"""
    data = _synthetic(n)
    base = _bits(_twin_run(n, None, data)[0])
    lanes = _bits(_twin_run(n, None, _reorder(data, 64, 1))[0])
    assert not np.array_equal(base, lanes)
    assert np.array_equal(base[:, :7], lanes[:, :7])  # the same episodes: counts and lengths agree
    if n >= 256:
        waves = _bits(_twin_run(n, None, _reorder(data, 256, 64))[0])
        assert not np.array_equal(base, waves) and np.array_equal(base[:, :7], waves[:, :7])
    if n == 1000:  # four chunks: n_blocks 1, 2 and 4 associate their sums differently
        walks = [_bits(_twin_run(n, nb, data)[0]).tobytes() for nb in (1, 2, None)]
        assert len(set(walks)) == 3


@pytest.mark.parametrize("n", [64, 65, 255, 256, 257, 1000])
def test_synthetic_rows_are_order_sensitive(d2, n):
    check_order_sensitive(n)


def _device_run(n, n_blocks, data):
    from drone2d_amd.monitor import EpisodeMonitor

    term, trunc, info, live = data
    mon = EpisodeMonitor(n, DEV, n_blocks)
    mon.live.copy_(torch.from_numpy(live))
    t_d, r_d, i_d = (torch.from_numpy(x).to(DEV) for x in (term, trunc, info))
    outs = []
    for t in range(STEPS):
        mon.step(t_d[t], r_d[t], i_d[t])
        if t in (STEPS // 2, STEPS - 1):
            outs.append(mon.flush().cpu().numpy().copy())
    state = (mon.run.cpu().numpy(), mon.minclr.cpu().numpy(), mon.live.cpu().numpy(), mon.part.cpu().numpy())
    return outs, state, mon.n_blocks


@pytest.mark.parametrize("n_blocks", [1, 2, None])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_device_matches_twin_bit_for_bit(d2, n, n_blocks):
    data = _synthetic(n)
    outs, state, nb = _device_run(n, n_blocks, data)
    want, twin = _twin_run(n, n_blocks, data)
    assert twin.n_blocks == nb
    for got, w in zip(outs, want):
        assert np.array_equal(got.view(np.int64), w.view(np.int64)), (got, w)
    assert want[0][0] > 0 or n < 8  # episodes were deposited ...
    assert (want[0][24] + want[1][24] > 0) or n < 64  # ... and skipped
    if n >= 255:
        assert np.isnan(want[0]).any()  # the specials reached the sums (+inf and -inf meet there)
    # the state left behind (a NaN's sign is the adder's own: compare NaN as NaN)
    assert np.array_equal(state[0], twin.run, equal_nan=True)
    assert np.array_equal(state[1], twin.minclr) and np.array_equal(state[2], twin.live)
    assert not state[3].any()
    # run to run
    outs2, state2, _ = _device_run(n, n_blocks, data)
    for a, b in zip(outs, outs2):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(state[0].view(np.int64), state2[0].view(np.int64))


def _real(d2, n, steps, std, **kw):
    """A real batch's outputs through the device monitor and, copied back, through the twin."""
    from drone2d_amd.config import TEST_SCENARIOS
    from drone2d_amd.monitor import EpisodeMonitor, monitor_host

    venv = d2.Drone2dVecEnv(n, seed=9, **_train_kw(scenario=list(TEST_SCENARIOS), **kw))
    mon, twin = EpisodeMonitor(venv), monitor_host(n)
    assert mon.hip and mon.n_blocks == twin.n_blocks
    g = torch.Generator(device=DEV).manual_seed(1)
    venv.reset(seed=9)
    got, want = [], []
    for t in range(steps):
        a = (torch.randn(n, 2, device=DEV, generator=g) * std).clamp(-1.0, 1.0)
        _, _, term, trunc, info = venv.step(a)
        mon.step(term, trunc, info)
        twin.step(term.cpu().numpy(), trunc.cpu().numpy(), info.cpu().numpy())
        if t % 100 == 99 or t == steps - 1:
            got.append(mon.flush().cpu().numpy().copy())
            want.append(twin.flush())
    stats = venv.episode_stats().cpu().numpy()
    venv.close()
    return np.array(got), np.array(want), stats


@pytest.mark.parametrize("n,steps,std,kw", [(448, 300, 0.5, {}), (64, 120, 0.25, {"n_steps": 40})],
                         ids=["448x300", "64_timeups"])
def test_real_outputs_match_twin_and_episode_stats(d2, n, steps, std, kw):
    from drone2d_amd import abi
    from drone2d_amd import monitor as M

    got, want, stats = _real(d2, n, steps, std, **kw)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    v = got.sum(0)
    assert v[M.EPISODES] == stats[abi.ST_EPISODES] > 0 and v[M.SKIPPED] == 0
    assert v[M.SUCCESS] == stats[abi.ST_SUCCESS] and v[M.FAIL] == stats[abi.ST_FAIL]
    assert v[M.COLLISION] == stats[abi.ST_COLLISION] and v[M.LEN] == stats[abi.ST_LEN]
    if kw:
        assert v[M.TIMEUP] > 0
    else:
        assert v[M.AA] > 0 and v[M.COLLISION] > 0


def test_monitor_in_a_captured_graph(d2):
    """A 16-step (venv.step, monitor.step) loop plus the flush, captured and replayed, gives the eager
    loop's bits.  Both batches fly the same 64 steps; the second one's last 16 are a graph replay."""
    from drone2d_amd.monitor import EpisodeMonitor

    n, T = 512, 16
    acts = (torch.rand(4 * T, n, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)) * 2 - 1)

    def block(venv, mon, k):
        for t in range(T):
            _, _, term, trunc, info = venv.step(acts[k * T + t])
            mon.step(term, trunc, info)
        return mon.flush()

    def fly(graph_last):
        venv = d2.Drone2dVecEnv(n, seed=4, **_train_kw(scenario="corridor"))
        mon = EpisodeMonitor(venv)
        venv.reset(seed=4)
        mon.reset()
        outs = [block(venv, mon, k).cpu().numpy().copy() for k in range(3)]
        if graph_last:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                block(venv, mon, 3)
            g.replay()
            outs.append(mon.out.cpu().numpy().copy())
        else:
            outs.append(block(venv, mon, 3).cpu().numpy().copy())
        torch.cuda.synchronize()
        venv.close()
        return np.array(outs)

    eager, graphed = fly(False), fly(True)
    assert eager[3][0] > 0, "no episode ended in the captured block"
    assert np.array_equal(eager.view(np.int64), graphed.view(np.int64))


def test_ppo_fused_rollout_with_monitor(d2):
    """Three updates on 256 corridor envs (eager, capture, replay), with and without the monitor: the
    same parameters bit for bit, and the monitor's episode count is the rollout's own."""
    from drone2d_amd.ppo import PPO, PPOConfig

    def run(monitor):
        venv = d2.Drone2dVecEnv(256, seed=5, **_train_kw(scenario="corridor"))
        algo = PPO(venv, PPOConfig.gpu_defaults(n_steps=16, batch_size=1024, n_epochs=2), seed=1)
        hist = algo.learn(3 * 16 * 256, monitor=monitor)
        assert algo._fused and algo._ro_graph is not None and algo._graph is not None
        flat = torch.cat([p.detach().reshape(-1) for p in algo.policy.parameters()]).cpu()
        venv.close()
        return flat, hist

    p0, h0 = run(None)
    p1, h1 = run(True)
    assert torch.equal(p0, p1)
    assert len(h1) == 3 and sum(r["episodes"] for r in h1) > 0
    for a, b in zip(h0, h1):
        assert a["episodes"] == b["episodes"] == b["monitor/episodes"] and b["monitor/skipped"] == 0
        assert a["policy_loss"] == b["policy_loss"] and a["value_loss"] == b["value_loss"]
        assert "monitor/episodes" not in a and np.isfinite(b["train/explained_variance"])


def test_argument_errors_launch_nothing(d2):
    from drone2d_amd import monitor as M

    n = 300
    term, trunc, info, _ = _synthetic(n)
    mon = M.EpisodeMonitor(n, DEV)
    lib = M.load()
    t_d, r_d = torch.from_numpy(term[0] | True).to(DEV), torch.from_numpy(trunc[0]).to(DEV)
    pad = torch.zeros(n * 12 + 4, dtype=torch.float32, device=DEV)
    pad[1:1 + n * 12] = torch.from_numpy(info[0]).reshape(-1).to(DEV)
    i_d = torch.from_numpy(info[0]).to(DEV)

    def args(**over):
        a = M.D2DMonitorStepArgs(n=n, info_dim=12, n_blocks=mon.n_blocks, term=t_d.data_ptr(), trunc=r_d.data_ptr(),
                                 info=i_d.data_ptr(), run=mon.run.data_ptr(), minclr=mon.minclr.data_ptr(),
                                 live=mon.live.data_ptr(), part=mon.part.data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    stream = torch.cuda.current_stream().cuda_stream
    assert i_d.data_ptr() % 16 == 0 and (pad.data_ptr() + 4) % 16 != 0
    for bad in (dict(info_dim=11), dict(info=pad.data_ptr() + 4), dict(n_blocks=0), dict(n_blocks=1025), dict(n=0),
                dict(run=None)):
        assert lib.d2d_monitor_step(C.byref(args(**bad)), stream) == 1, bad
    assert lib.d2d_monitor_flush(mon.part.data_ptr(), 0, mon.out.data_ptr(), stream) == 1
    assert lib.d2d_monitor_reset(n, mon.run.data_ptr(), mon.minclr.data_ptr(), mon.live.data_ptr(), 2, stream) == 1
    torch.cuda.synchronize()
    # every env's row said "done": a launch would have deposited and rewritten the state
    assert not mon.run.any() and not mon.part.any() and torch.isinf(mon.minclr).all()
    with pytest.raises(M.MonitorError):
        mon.step(t_d, r_d, i_d[:, :11].contiguous())
    assert lib.d2d_monitor_step(C.byref(args()), stream) == 0
    torch.cuda.synchronize()
    assert mon.flush().cpu()[M.EPISODES] == n
