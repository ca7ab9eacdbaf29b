"""Reward normalisation without a GPU: ``reward_norm_host`` (the NumPy twin of libd2d_norm.so,
include/d2d_norm.h) against the float64 restatement of SB3's VecNormalize in tests/norm_ref.py, its
summation order, ``RewardNormalizer`` on CPU tensors, ``PPO(norm_reward=True)`` on the oracle backend
(the recorded rewards, GAE, save / resume, the agent file with the option off) and the build list."""
import json
import os
import re
import zipfile

import numpy as np
import pytest
import torch

import norm_util as U
from norm_ref import VecNormalizeReward
from oracle_backend import OracleVecBackend

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# PPOConfig's fields before reward normalisation: the "config" of an agent file of the parent's format
PARENT_CONFIG_KEYS = ["n_steps", "batch_size", "n_epochs", "learning_rate", "gamma", "gae_lambda", "clip_range", "ent_coef",
                      "vf_coef", "max_grad_norm", "normalize_advantage", "graph", "manual", "learning_rate_end",
                      "clip_range_end", "clip_range_vf", "target_kl"]
NORM_KEYS = ["norm_reward", "clip_reward", "norm_epsilon"]

# The largest relative difference between the twin and norm_ref over tests/norm_util.realistic, every n of
# SIZES, seeds 0..3, measured when this test was written: 4.05e-16 (n = 65, seed 2; 2.74e-16 on seed 0,
# which the test uses).  It does not grow with n on these data.  The assertion allows 16 x that.
MEASURED_REL = 4.05e-16


def _rel(a, b, scale=None):
    s = np.abs(b) if scale is None else scale
    return float(np.max(np.where(a == b, 0.0, np.abs(a - b) / s)))


@pytest.mark.parametrize("n", U.SIZES)
def test_twin_matches_sb3_restatement(d2, n):
    """Six steps of realistic rewards.  ``rms`` and ``ret``: within min(16 x the measured difference, the
    derived cap 8 n 2^-53 (1 + bm^2 / bv)) relative -- var, count and ret against their own size, the
    mean against sqrt(var + mean^2), the size of the returns it averages.  The cap: a sum of n float64
    terms in any order is off by at most about n 2^-53 sum|x|; the shifted moments (the twin) and
    np.mean / np.var (the reference) each carry one such error, bv = S2 / n - bm^2 loses a factor
    (1 + bm^2 / bv) to cancellation, and the factor 8 covers the two sums, their squares and the
    handful of operations of update_from_moments.  With |bm| <= sqrt(bv), checked at every step, the
    cap stays within 16 n 2^-53.  For n = 1 the batch variance is exactly 0 on both sides (the condition
    cannot hold and nothing cancels): the cap is 16 n 2^-53 itself.  ``rew_out``: one float32 rounding of
    nearly equal doubles, so within 2^-23 relative."""
    data = U.realistic(n)
    twin = U.twin_run(data)
    ref = VecNormalizeReward(n, U.GAMMA)
    worst = 0.0
    for t in range(U.STEPS):
        old_mean = float(ref.ret_rms.mean)
        want = ref.step(data[0][t], data[1][t] | data[2][t])
        out, ret, rms = twin[t]
        if n > 1:
            # the batch moments of this step, from the reference's side (ret before the done rows are zeroed:
            # the twin's ret after the step agrees with it off the done rows, so rebuild it from the rewards)
            full = (twin[t - 1][1] * U.GAMMA if t else np.zeros(n)) + data[0][t].astype(np.float64)
            bm, bv = np.mean(full) - old_mean, np.var(full)
            assert abs(bm) <= np.sqrt(bv), f"step {t}: |bm| {abs(bm):.3g} > sqrt(bv) {np.sqrt(bv):.3g}: choose other data"
            cap = 8 * n * 2.0 ** -53 * (1 + bm * bm / bv)
            assert cap <= 16 * n * 2.0 ** -53
        else:
            cap = 16 * n * 2.0 ** -53
        tol = min(16 * MEASURED_REL, cap)
        r = ref.rms
        diffs = (_rel(rms[0], r[0], np.sqrt(r[1] + r[0] ** 2)), _rel(rms[1], r[1]), _rel(rms[2], r[2]),
                 _rel(ret, ref.returns, np.maximum(np.abs(ref.returns), 1e-300)))
        worst = max(worst, *diffs)
        assert max(diffs) <= tol, (t, diffs, tol)
        assert not ret[data[1][t] | data[2][t]].any()  # the done rows' returns start over
        assert out.dtype == np.float32
        np.testing.assert_allclose(out.astype(np.float64), want, rtol=2.0 ** -23, atol=0)
    print(f"n = {n}: largest relative difference twin vs norm_ref {worst:.3g} (asserted at {min(16 * MEASURED_REL, cap):.3g})")


def test_training_off_leaves_state_and_inf_poisons(d2):
    """``training=0``: only the scaling, with the stored variance; ``rms`` and ``ret`` untouched.  An inf
    reward leaves ``rms`` non-finite in the twin and in the reference alike, and both stay so."""
    from drone2d_amd.normalize import reward_norm_host

    n = 300
    data = U.realistic(n)
    warm = U.twin_run(data)
    _, ret0, rms0 = warm[-1]
    ret, rms = ret0.copy(), rms0.copy()
    out = reward_norm_host(data[0][0], data[1][0] | True, data[2][0], ret, rms, U.GAMMA, training=False)
    assert np.array_equal(ret.view(np.int64), ret0.view(np.int64)) and np.array_equal(rms.view(np.int64), rms0.view(np.int64))
    want = np.clip(data[0][0].astype(np.float64) / np.sqrt(rms0[1] + 1e-8), -10.0, 10.0).astype(np.float32)
    assert np.array_equal(out, want)
    out = reward_norm_host(data[0][0], data[1][0], data[2][0], ret, rms, U.GAMMA, clip=1.0, training=False)
    assert np.array_equal(out, np.clip(want, -1.0, 1.0)) and (out == 1.0).any() and (out == -1.0).any()

    rew = data[0].copy()
    rew[2, 17] = np.inf
    rew[4, 100] = np.nan
    twin = U.twin_run((rew, data[1], data[2]))
    ref = VecNormalizeReward(n, U.GAMMA)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(U.STEPS):
            want = ref.step(rew[t], data[1][t] | data[2][t]).astype(np.float32)
            out, _, rms = twin[t]
            assert np.array_equal(np.isnan(rms), np.isnan(ref.rms)) and np.array_equal(np.isinf(rms), np.isinf(ref.rms)), t
            assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isinf(out), np.isinf(want)), t
            assert np.isfinite(rms).all() == (t < 2)


def _rms_bits(data, n_blocks=None):
    return np.array([r for _, _, r in U.twin_run(data, n_blocks)]).view(np.int64)


@pytest.mark.parametrize("n", [64, 65, 255, 256, 257, 1000])
def test_summation_order_is_pinned(d2, n):
    """On the order-sensitive data the twin's ``rms`` bits change when the lanes of every wave are
    rearranged and (from one full chunk on) when the waves of every chunk are reversed: the same returns,
    added in another order.  So a device that added lanes or waves otherwise than include/d2d_norm.h
    states could not match the twin on these data (tests/test_gpu_reward_norm.py).  Data on which a
    rearrangement changes no bit would prove nothing: that fails here.

    The lanes are permuted at random, not reversed: the shuffle-down tree adds lanes l and l + s, and
    under a reversal of all 64 lanes the same pairs meet at every stage, so the tree's sum is the same
    bits for any data (checked below: a lane-by-lane ascending adder would not pass that)."""
    data = U.order_sensitive(n)
    base = _rms_bits(data)
    assert np.array_equal(base, _rms_bits(U.reorder(data, 64, 1)))  # the tree's own symmetry
    lanes = _rms_bits(U.permute_lanes(data))
    assert not np.array_equal(base[:, :2], lanes[:, :2])
    assert np.array_equal(base[:, 2], lanes[:, 2])  # the counts agree: the same batches
    np.testing.assert_allclose(lanes.view(np.float64), base.view(np.float64), rtol=1e-9)  # the same numbers otherwise
    if n >= 256:
        waves = _rms_bits(U.reorder(data, 256, 64))
        assert not np.array_equal(base[:, :2], waves[:, :2])
        np.testing.assert_allclose(waves.view(np.float64), base.view(np.float64), rtol=1e-9)
    if n == 1000:  # four chunks: one, two and three rows associate the chunk sums differently
        assert len({_rms_bits(data, nb).tobytes() for nb in (1, 2, 3)}) == 3


def test_twin_order_on_hand_made_returns(d2):
    """The tree inside a wave, waves 0..3, the chunk walk and the fold, each told from another order by
    a sum that is 0 one way and 1 the other (S1 of the first step: ret = rew, running mean 0)."""
    from drone2d_amd.normalize import chunk_sums, fold_sums

    big = 2.0 ** 60

    def s1(n, n_blocks, where):
        d = np.zeros(n)
        for i, x in where.items():
            d[i] = x
        return float(fold_sums(chunk_sums(d), n_blocks))

    # the tree: stage s = 32 adds lane 32 to lane 0 first, so (big + -big) + 1; ascending lanes would give 0
    assert s1(64, 1, {0: big, 1: 1.0, 32: -big}) == 1.0
    assert s1(64, 1, {0: big, 32: 1.0, 1: -big}) == 0.0
    assert s1(256, 1, {0: big, 70: 1.0, 130: -big}) == 0.0        # waves 0, 1, 2 in order
    assert s1(256, 1, {0: big, 70: -big, 130: 1.0}) == 1.0
    assert s1(600, 1, {0: big, 300: 1.0, 599: -big}) == 0.0       # one row walks chunks 0, 1, 2
    assert s1(600, 2, {0: big, 300: 1.0, 599: -big}) == 1.0       # rows {0, 2} and {1}: (big - big) + 1
    assert s1(600, 3, {0: big, 300: 1.0, 599: -big}) == 0.0       # rows 0, 1, 2 in fold order


def test_normalizer_on_cpu_tensors(d2):
    from drone2d_amd.normalize import RMS_INIT, RewardNormalizer, default_blocks

    n = 300
    data = U.realistic(n)
    want = U.twin_run(data)
    nz = RewardNormalizer(n, U.GAMMA, device="cpu")
    assert not nz.hip and nz.n_blocks == default_blocks(n) == 2 and nz.training
    for t in range(U.STEPS):
        out = nz.step(*(torch.from_numpy(x[t]) for x in data))
        assert out.dtype == torch.float32 and np.array_equal(out.numpy(), want[t][0])
    assert np.array_equal(nz.ret.numpy(), want[-1][1]) and np.array_equal(nz.rms.numpy(), want[-1][2])
    assert float(nz.scale()) == float(np.sqrt(want[-1][2][1] + 1e-8))
    sd = nz.state_dict()
    assert set(sd) == {"rms", "ret", "gamma", "clip", "epsilon"}
    other = RewardNormalizer(n, 0.5, clip=1.0, device="cpu")
    other.load_state_dict(sd)
    assert torch.equal(other.rms, nz.rms) and torch.equal(other.ret, nz.ret) and other.gamma == U.GAMMA and other.clip == 10.0
    nz.training = False
    out = nz.step(*(torch.from_numpy(x[0]) for x in data))
    assert torch.equal(nz.rms, other.rms) and torch.equal(nz.ret, other.ret)
    assert np.array_equal(out.numpy(), U.twin_run(tuple(x[:1] for x in data), training=False, ret0=want[-1][1],
                                                  rms0=want[-1][2])[0][0])
    nz.reset()
    assert not nz.ret.any() and torch.equal(nz.rms, other.rms)
    nz.reset(stats=True)
    assert nz.rms.tolist() == list(RMS_INIT)
    with pytest.raises(ValueError):
        RewardNormalizer(8, 0.99, n_blocks=1025, device="cpu")
    with pytest.raises(ValueError):
        RewardNormalizer(0, 0.99, device="cpu")
    with pytest.raises(ValueError):
        other.load_state_dict({"rms": sd["rms"], "ret": sd["ret"][:10]})


def test_step_args_struct_matches_header(d2, tmp_path):
    """The ctypes mirror against a compiled probe of include/d2d_norm.h (size, offsets, constants)."""
    import ctypes as C
    import subprocess

    from drone2d_amd import normalize as N

    fields = [f for f, _ in N.D2DNormStepArgs._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "d2d_norm.h"\nint main(void){'
                   'printf("%zu %d %d %d", sizeof(d2d_norm_step_args), D2D_NORM_ABI_VERSION, D2D_NORM_CHUNK, D2D_NORM_MAX_BLOCKS);'
                   + "".join(f'printf(" %zu", offsetof(d2d_norm_step_args, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [C.sizeof(N.D2DNormStepArgs), N.ABI_VERSION, N.CHUNK, N.MAX_BLOCKS]
    assert got[4:] == [getattr(N.D2DNormStepArgs, f).offset for f in fields]


def test_norm_headers_are_build_dependencies(d2):
    """Every header d2d_norm.hip includes is on the new build's dependency list, and the env library's
    list did not grow by them."""
    from drone2d_amd import _build

    deps = {os.path.normpath(p) for p in _build.NORM_HDRS}
    todo, seen = [_build.NORM_SRC], set()
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for line in open(f):
            m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
            if m:
                inc = os.path.normpath(os.path.join(os.path.dirname(f), m.group(1)))
                if not os.path.exists(inc):  # not beside the including file: under include/ (-I)
                    inc = os.path.normpath(os.path.join(REPO, "include", m.group(1)))
                assert inc in deps, f"{inc} (included by {f}) is not in the norm build's dependency list"
                todo.append(inc)
    assert {os.path.basename(p) for p in seen} == {"d2d_norm.hip", "d2d_norm.h"}
    assert not any("norm" in os.path.basename(p) for p in _build.env_headers())
    assert len(_build.env_headers()) == len(_build.HDRS)
    assert _build.HIPCC_FLAGS.count("-ffp-contract=off") == 1  # the host/device identity depends on it
    assert os.path.exists(_build.NORM_OUT), "build() did not make libd2d_norm.so"


# ------------------------------------------------------------------------------------------------ PPO
def _kw():
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, scenario="corridor")


def _algo(be, norm=True, seed=0, **over):
    from drone2d_amd.ppo import PPO, PPOConfig

    return PPO(be, PPOConfig(n_steps=8, batch_size=64, n_epochs=2, norm_reward=norm, **over), seed=seed, device="cpu")


def test_ppo_records_the_twins_rewards_and_their_gae(d2):
    """Two rollouts (an update between them) with ``norm_reward=True`` on 32 corridor envs of the oracle
    backend: ``_ro["rew"]`` equals bit for bit the twin fed with the raw rewards -- those of a second,
    identically built batch that replays the rollout's clipped actions -- and the advantages in ``_flat``
    are ``compute_gae`` of those rewards.  The rollout's episode statistics stay raw."""
    from drone2d_amd import abi
    from drone2d_amd.normalize import RMS_INIT, reward_norm_host
    from drone2d_amd.ppo import compute_gae

    N, T = 32, 8
    be, raw = OracleVecBackend(N, seed=3, **_kw()), OracleVecBackend(N, seed=3, **_kw())
    algo = _algo(be)
    assert algo.normalizer is not None and not algo.normalizer.hip
    raw.reset()
    ret, rms = np.zeros(N), np.array(RMS_INIT)
    start0 = torch.ones(N, dtype=torch.bool)
    finished = ret_sum = 0.0
    for k in range(2):
        rec = algo.collect_rollouts()
        R = algo._ro
        want = np.zeros((T, N), np.float32)
        fin = tot = 0.0
        for t in range(T):
            _, rew, term, trunc, info = raw.step(R["act"][t].clamp(-1.0, 1.0))
            want[t] = reward_norm_host(rew.numpy(), term.numpy(), trunc.numpy(), ret, rms, algo.cfg.gamma, 10.0, 1e-8)
            done = (term | trunc).numpy()
            assert np.array_equal(done, R["done"][t].numpy())
            fin += done.sum()
            tot += info.numpy()[done, abi.INFO_TOTREW].astype(np.float64).sum()
        assert np.array_equal(R["rew"].numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(algo.normalizer.rms.numpy(), rms) and np.array_equal(algo.normalizer.ret.numpy(), ret)
        assert not np.array_equal(want, np.clip(want, -0.5, 0.5))  # (not a degenerate all-small signal)
        with torch.no_grad():
            last_values = algo.policy.predict_values(R["obs"][T])
        starts = torch.cat([start0[None], R["done"][:-1]])
        adv, returns = compute_gae(torch.from_numpy(want), R["val"], starts, last_values, R["done"][T - 1],
                                   algo.cfg.gamma, algo.cfg.gae_lambda)
        assert torch.equal(algo._flat[3], adv.reshape(-1)) and torch.equal(algo._flat[4], returns.reshape(-1))
        start0 = R["done"][T - 1].clone()
        # the record: raw episode statistics, and the normaliser's two scalars
        assert rec["episodes"] == fin and (fin == 0 or rec["mean_return"] == pytest.approx(tot / fin, rel=1e-12))
        assert rec["norm/return_var"] == rms[1] and rec["norm/reward_scale"] == float(np.sqrt(rms[1] + 1e-8))
        finished += fin
        ret_sum += tot
        algo.train()
    be.close()
    raw.close()


def test_ppo_norm_off_records_and_files_are_the_parents(d2, tmp_path):
    """With the option off: no normaliser, no ``norm/*`` record keys, ``data.json`` holds none of the new
    config keys (its config is exactly the parent's key list, in order) and the zip has no
    ``reward_norm.pth``; such a file -- the parent's format -- loads, with normalisation off.  With it
    on, keys and member are there."""
    from drone2d_amd.ppo import PPO

    be = OracleVecBackend(32, seed=3, **_kw())
    off = _algo(be, norm=False)
    hist = off.learn(256)
    assert off.normalizer is None and not any(k.startswith("norm/") for k in hist[0])
    path = off.save(str(tmp_path / "off.zip"))
    with zipfile.ZipFile(path) as z:
        assert set(z.namelist()) == {"data.json", "policy.pth", "train_state.pth"}
        data = json.loads(z.read("data.json"))
    assert list(data["config"]) == PARENT_CONFIG_KEYS and not set(NORM_KEYS) & set(data["config"])
    back = PPO.load(path, be, device="cpu")
    assert back.normalizer is None and back.cfg == off.cfg and back.cfg.norm_reward is False
    back.learn(512)

    on = _algo(be, norm=True, clip_reward=5.0)
    hist = on.learn(256)
    assert {"norm/reward_scale", "norm/return_var"} <= set(hist[0])
    from drone2d_amd import trainlog

    logged = trainlog.record_scalars(hist[0])  # what ScalarLog writes: the two keys under their own names
    assert logged["norm/reward_scale"] == hist[0]["norm/reward_scale"] > 0
    assert logged["norm/return_var"] == hist[0]["norm/return_var"]
    path = on.save(str(tmp_path / "on.zip"))
    with zipfile.ZipFile(path) as z:
        assert set(z.namelist()) == {"data.json", "policy.pth", "train_state.pth", "reward_norm.pth"}
        data = json.loads(z.read("data.json"))
    assert list(data["config"]) == PARENT_CONFIG_KEYS + NORM_KEYS
    assert data["config"]["norm_reward"] is True and data["config"]["clip_reward"] == 5.0
    back = PPO.load(path, be, device="cpu")
    assert back.cfg == on.cfg and torch.equal(back.normalizer.rms, on.normalizer.rms)
    assert torch.equal(back.normalizer.ret, on.normalizer.ret) and back.normalizer.clip == 5.0
    be.close()


def test_ppo_norm_resume_is_exact(d2, tmp_path):
    """4 updates in one go == 2 updates, save, load into a new batch, 2 more: parameters, Adam state,
    ``rms`` and ``ret``.  (The oracle backend's state is not in the file: the new batch is brought to the
    saved run's state by a run of its own; the agent -- normaliser included -- comes from the file.)"""
    from drone2d_amd.ppo import PPO

    be_a, be_b, be_c = (OracleVecBackend(32, seed=3, **_kw()) for _ in range(3))
    a = _algo(be_a)
    a.learn(4 * 256)
    b0 = _algo(be_b)
    b0.learn(2 * 256)
    path = b0.save(str(tmp_path / "b.zip"))
    _algo(be_c).learn(2 * 256)
    c = PPO.load(path, be_c, device="cpu")
    assert c.normalizer is not None and c.normalizer is not b0.normalizer
    assert torch.equal(c.normalizer.rms, b0.normalizer.rms) and torch.equal(c.normalizer.ret, b0.normalizer.ret)
    assert c.normalizer.ret.any() and float(c.normalizer.rms[2]) == pytest.approx(1e-4 + 2 * 8 * 32, rel=1e-12)
    hist = c.learn(4 * 256)
    assert len(hist) == 2 and a.num_timesteps == c.num_timesteps == 1024
    for (k, p), q in zip(a.policy.state_dict().items(), c.policy.state_dict().values()):
        assert torch.equal(p, q), k
    assert torch.equal(a.manual.m, c.manual.m) and torch.equal(a.manual.v, c.manual.v) and torch.equal(a.manual.t, c.manual.t)
    assert torch.equal(a.normalizer.rms, c.normalizer.rms) and torch.equal(a.normalizer.ret, c.normalizer.ret)
    # and it is not the run without normalisation
    d = _algo(OracleVecBackend(32, seed=3, **_kw()), norm=False)
    d.learn(4 * 256)
    assert not torch.equal(a.manual.m, d.manual.m)
    for be in (be_a, be_b, be_c, d.venv):
        be.close()


def test_ppo_reset_keeps_the_statistics(d2):
    from drone2d_amd.ppo import PPO  # noqa: F401

    be = OracleVecBackend(32, seed=3, **_kw())
    algo = _algo(be)
    algo.learn(256)
    rms = algo.normalizer.rms.clone()
    assert algo.normalizer.ret.any()
    algo._reset_envs()
    assert not algo.normalizer.ret.any() and torch.equal(algo.normalizer.rms, rms)
    be.close()


def test_ppo_norm_reward_refuses_several_ranks(d2, monkeypatch):
    from drone2d_amd import ppo

    monkeypatch.setattr(ppo.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(ppo.dist, "get_world_size", lambda: 2)
    be = OracleVecBackend(8, seed=3, **_kw())
    with pytest.raises(ValueError, match="rank"):
        _algo(be)
    be.close()
