"""libd2d_norm.so on an MI355X: the device against its NumPy twin bit for bit (order-sensitive rewards,
every batch-size edge and the strided walk, ``training = 0``), captured into a HIP graph, its argument
checks, and inside ``PPO``'s fused rollout."""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _dev(data):
    return tuple(torch.from_numpy(x).to(DEV) for x in data)


@pytest.fixture(scope="module")
def twins():
    """The twin's runs over the order-sensitive data, computed once per (n, n_blocks)."""
    cache = {}

    def get(n, n_blocks):
        if (n, n_blocks) not in cache:
            data = U.order_sensitive(n)
            cache[n, n_blocks] = (data, U.twin_run(data, n_blocks))
        return cache[n, n_blocks]

    return get


@pytest.mark.parametrize("n_blocks", [1, 3])
@pytest.mark.parametrize("n", U.SIZES)
def test_device_matches_twin_bit_for_bit(d2, twins, n, n_blocks):
    """``rew_out``, ``ret`` and ``rms`` after each of six steps, then a ``training = 0`` step.  (1 000
    envs on 3 workgroups: one workgroup walks two chunks; on 1: four.)"""
    from drone2d_amd.normalize import RewardNormalizer

    data, want = twins(n, n_blocks)
    rew, term, trunc = _dev(data)
    nz = RewardNormalizer(n, U.GAMMA, device=DEV, n_blocks=n_blocks)
    assert nz.hip
    for t in range(U.STEPS):
        out = nz.step(rew[t], term[t], trunc[t])
        o, ret, rms = (torch.from_numpy(x) for x in want[t])
        assert torch.equal(out.cpu(), o), t
        assert torch.equal(nz.ret.cpu(), ret), t
        assert torch.equal(nz.rms.cpu(), rms), (t, nz.rms.cpu().tolist(), rms.tolist())
    assert int(nz.ticket) == 0
    nz.training = False
    out = nz.step(rew[0], term[0] | True, trunc[0])
    w = U.twin_run(tuple(x[:1] for x in data), n_blocks, training=False, ret0=want[-1][1], rms0=want[-1][2])[0]
    assert torch.equal(out.cpu(), torch.from_numpy(w[0]))
    assert torch.equal(nz.ret.cpu(), torch.from_numpy(want[-1][1])) and torch.equal(nz.rms.cpu(), torch.from_numpy(want[-1][2]))
    assert float(nz.scale()) == float(np.sqrt(want[-1][2][1] + 1e-8))
    nz.reset()
    assert not nz.ret.any() and torch.equal(nz.rms.cpu(), torch.from_numpy(want[-1][2]))
    nz.reset(stats=True)
    assert nz.rms.cpu().tolist() == [0.0, 1.0, 1e-4]


def test_specials_agree_with_the_twin(d2):
    """An inf and a NaN reward: ``rms`` and ``rew_out`` are non-finite where the twin's are."""
    from drone2d_amd.normalize import RewardNormalizer

    n = 300
    data = U.realistic(n)
    data[0][2, 17] = np.inf
    data[0][4, 100] = np.nan
    want = U.twin_run(data)
    rew, term, trunc = _dev(data)
    nz = RewardNormalizer(n, U.GAMMA, device=DEV)
    for t in range(U.STEPS):
        out = nz.step(rew[t], term[t], trunc[t]).cpu().numpy()
        rms = nz.rms.cpu().numpy()
        for got, w in ((out, want[t][0]), (rms, want[t][2])):
            assert np.array_equal(np.isnan(got), np.isnan(w)) and np.array_equal(np.isinf(got), np.isinf(w)), t
        if t < 2:
            assert np.array_equal(out, want[t][0]) and np.array_equal(rms, want[t][2])
    assert not np.isfinite(rms[:2]).any()


def test_six_steps_in_a_captured_graph(d2, twins):
    """Six steps captured as a HIP graph and replayed twice equal twelve eager steps bit for bit."""
    from drone2d_amd.normalize import RewardNormalizer

    n = 1000
    data, _ = twins(n, None)
    rew, term, trunc = _dev(data)

    def six(nz, outs):
        for t in range(U.STEPS):
            outs[t].copy_(nz.step(rew[t], term[t], trunc[t]))

    eager, e_out = RewardNormalizer(n, U.GAMMA, device=DEV), torch.zeros(2, U.STEPS, n, device=DEV)
    six(eager, e_out[0])
    six(eager, e_out[1])
    nz, g_out = RewardNormalizer(n, U.GAMMA, device=DEV), torch.zeros(2, U.STEPS, n, device=DEV)
    buf = torch.zeros(U.STEPS, n, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        six(nz, buf)
    assert nz.rms.cpu().tolist() == [0.0, 1.0, 1e-4]  # (capturing ran nothing)
    for k in range(2):
        g.replay()
        g_out[k].copy_(buf)
    torch.cuda.synchronize()
    assert torch.equal(g_out, e_out) and torch.equal(nz.ret, eager.ret) and torch.equal(nz.rms, eager.rms)
    assert float(nz.rms[2]) == pytest.approx(1e-4 + 12 * n, rel=1e-12) and int(nz.ticket) == 0  # (twelve additions of n)


def test_argument_errors_launch_nothing(d2):
    from drone2d_amd import normalize as N

    n = 300
    nz = N.RewardNormalizer(n, U.GAMMA, device=DEV)
    lib = N.load()
    rew = torch.full((n,), 2.0, device=DEV)
    done = torch.zeros(n, dtype=torch.uint8, device=DEV)
    nz.out.fill_(777.0)  # the canary: a launch would rewrite it, ret and rms
    odd = torch.zeros(2 * n + 2, dtype=torch.float32, device=DEV)

    def args(**over):
        a = N.D2DNormStepArgs(n=n, n_blocks=nz.n_blocks, training=1, gamma=U.GAMMA, clip=10.0, epsilon=1e-8,
                              rew=rew.data_ptr(), term=done.data_ptr(), trunc=done.data_ptr(), rew_out=nz.out.data_ptr(),
                              ret=nz.ret.data_ptr(), rms=nz.rms.data_ptr(), part=nz.part.data_ptr(),
                              ticket=nz.ticket.data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    stream = torch.cuda.current_stream().cuda_stream
    assert nz.ret.data_ptr() % 8 == 0 and (odd.data_ptr() + 4) % 8 != 0
    for bad in (dict(n=0), dict(n=-5), dict(n_blocks=0), dict(n_blocks=1025), dict(rew=None), dict(rew_out=None),
                dict(rms=None), dict(ret=None), dict(term=None), dict(trunc=None), dict(part=None), dict(ticket=None),
                dict(training=2), dict(clip=-1.0), dict(epsilon=float("nan")), dict(ret=odd.data_ptr() + 4)):
        assert lib.d2d_norm_step(C.byref(args(**bad)), stream) == 1, bad
    assert lib.d2d_norm_step(None, stream) == 1
    assert lib.d2d_norm_reset(0, nz.ret.data_ptr(), nz.rms.data_ptr(), stream) == 1
    assert lib.d2d_norm_reset(n, None, nz.rms.data_ptr(), stream) == 1
    torch.cuda.synchronize()
    assert (nz.out == 777.0).all() and not nz.ret.any() and nz.rms.cpu().tolist() == [0.0, 1.0, 1e-4]
    assert not nz.part.any() and int(nz.ticket) == 0
    with pytest.raises(ValueError):
        nz.step(rew[:-1], done, done)
    with pytest.raises(ValueError):
        nz.step(rew.double(), done, done)
    # training = 0 needs neither the state nor the masks
    assert lib.d2d_norm_step(C.byref(args(training=0, ret=None, term=None, trunc=None, part=None, ticket=None)), stream) == 0
    assert lib.d2d_norm_step(C.byref(args()), stream) == 0
    torch.cuda.synchronize()
    assert (nz.ret == 2.0).all() and float(nz.rms[2]) == 1e-4 + n and not (nz.out == 777.0).any()


def test_ppo_fused_rollout_with_norm_reward(d2):
    """Three rollouts on 256 corridor envs x 16 steps with ``norm_reward=True`` and the monitor attached:
    the first eager, the second captured and replayed, the third a replay.  ``_ro["rew"]`` and the
    normaliser's ``rms`` / ``ret`` equal, bit for bit, the twin fed with the raw rewards of an identically
    built batch that replays the same clipped actions; the rollout's episode statistics and the monitor
    report that batch's raw returns."""
    from drone2d_amd import abi
    from drone2d_amd.normalize import RMS_INIT, reward_norm_host
    from drone2d_amd.ppo import PPO, PPOConfig

    N, T = 256, 16
    venv = d2.Drone2dVecEnv(N, seed=5, **_train_kw(scenario="corridor"))
    raw = d2.Drone2dVecEnv(N, seed=5, **_train_kw(scenario="corridor"))
    algo = PPO(venv, PPOConfig.gpu_defaults(n_steps=T, batch_size=1024, n_epochs=2, norm_reward=True), seed=1)
    algo.set_monitor(True)
    assert algo.normalizer.hip
    raw.reset()
    ret, rms = np.zeros(N), np.array(RMS_INIT)
    episodes = 0
    for k in range(3):
        rec = algo.collect_rollouts()
        assert algo._fused and (algo._ro_graph is not None) == (k > 0)
        acts = algo._flat[1].reshape(T, N, 2).clamp(-1.0, 1.0)
        want = np.zeros((T, N), np.float32)
        fin, tot = 0, 0.0
        for t in range(T):
            _, rew, term, trunc, info = raw.step(acts[t].contiguous())
            rew, term, trunc, info = (x.cpu().numpy() for x in (rew, term, trunc, info))
            want[t] = reward_norm_host(rew, term, trunc, ret, rms, algo.cfg.gamma, 10.0, 1e-8)
            done = (term | trunc) != 0
            fin += int(done.sum())
            tot += float(info[done, abi.INFO_TOTREW].astype(np.float64).sum())
        assert torch.equal(algo._ro["rew"].cpu(), torch.from_numpy(want)), k
        assert torch.equal(algo.normalizer.rms.cpu(), torch.from_numpy(rms)), k
        assert torch.equal(algo.normalizer.ret.cpu(), torch.from_numpy(ret)), k
        assert rec["episodes"] == fin == rec["monitor/episodes"] and rec["monitor/skipped"] == 0
        if fin:
            assert rec["mean_return"] == pytest.approx(tot / fin, rel=1e-9)
            assert rec["monitor/rollout/ep_rew_mean"] == pytest.approx(tot / fin, rel=1e-9)
        assert rec["norm/return_var"] == rms[1] and rec["norm/reward_scale"] == float(np.sqrt(rms[1] + 1e-8))
        episodes += fin
        algo.train()
    assert episodes > 0 and rms[2] == pytest.approx(1e-4 + 3 * T * N, rel=1e-12)
    venv.close()
    raw.close()
