"""The time-limit bootstrap without a GPU: SB3's rule on the torch rollout (the semantics
d2d_ppo_rollout_step_tb is tested against in tests/test_gpu_trunc_bootstrap.py), and the ctypes
mirror of the new entry point against include/d2d_ppo.h."""
import ctypes as C
import os
import re

import numpy as np
import torch

from oracle_backend import OracleVecBackend

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def test_torch_rollout_bootstraps_truncations_as_sb3_does(d2):
    """SB3 2.1 ``collect_rollouts``: ``rewards[idx] += gamma * predict_values(terminal_observation)``
    where ``TimeLimit.truncated``.  The torch ``_rollout_body`` on 32 oracle envs that time out every 4
    steps: ``R["rew"]`` is the raw reward of an identically built batch that replays the clipped
    actions, plus ``gamma * V(terminal_obs)`` on the truncated rows, and bit for bit the raw reward on
    the others."""
    from drone2d_amd.ppo import PPO, PPOConfig

    N, T = 32, 8
    kw = _kw(scenario="large_free", n_steps=4)
    be = OracleVecBackend(N, seed=3, timeup_truncates=True, **kw)
    raw = OracleVecBackend(N, seed=3, timeup_truncates=True, **kw)
    algo = PPO(be, PPOConfig(n_steps=T, batch_size=64, n_epochs=2), seed=0, device="cpu")
    raw.reset()
    for k in range(2):
        algo.collect_rollouts()
        assert algo._truncates and not algo._fused
        R = algo._ro
        n_trunc = 0
        for t in range(T):
            _, rew, term, trunc, _ = raw.step(R["act"][t].clamp(-1.0, 1.0))
            assert not (term & trunc).any()
            assert torch.equal(R["done"][t], term | trunc)
            with torch.no_grad():
                tv = algo.policy.predict_values(raw.terminal_obs)
            want = torch.where(trunc, rew + algo.cfg.gamma * tv, rew)
            assert torch.equal(R["rew"][t], want), (k, t)
            assert torch.equal(R["rew"][t][~trunc], rew[~trunc])
            if trunc.any():
                assert not torch.equal(R["rew"][t][trunc], rew[trunc])  # (the bootstrap is not a no-op)
            n_trunc += int(trunc.sum())
        assert n_trunc >= N  # every env timed out at least once per rollout
        algo.train()
    be.close()
    raw.close()


def _header():
    with open(os.path.join(REPO, "include", "d2d_ppo.h")) as f:
        return f.read()


def test_header_and_ctypes_agree():
    from drone2d_amd import ppo_native as P

    h = _header()
    assert int(re.search(r"#define\s+D2D_PPO_TB_VERSION\s+(\d+)", h).group(1)) == P.PPO_TB_VERSION
    assert re.search(r"int32_t\s+d2d_ppo_tb_version\(void\);", h)
    m = re.search(r"int32_t\s+d2d_ppo_rollout_step_tb\(([^;]*)\);", h)
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    res, args = P.SIGNATURES["d2d_ppo_rollout_step_tb"]
    assert res is C.c_int32 and len(args) == len(params) == 4
    assert args[0] is C.POINTER(P.D2DPPORollout) and all(a is C.c_void_p for a in args[1:])
    assert P.SIGNATURES["d2d_ppo_tb_version"] == (C.c_int32, [])
    # additive: the step it extends, the struct and the ABI version are the parent's
    assert P.SIGNATURES["d2d_ppo_rollout_step"] == (C.c_int32, [C.POINTER(P.D2DPPORollout), C.c_void_p, C.c_void_p])
    assert int(re.search(r"#define\s+D2D_PPO_ABI_VERSION\s+(\d+)", h).group(1)) == P.ABI_VERSION == 6
    assert "not done here" not in h


def test_library_exports_the_entry_point():
    """The library cross-compiled for gfx950 by ``build()`` exports both symbols and holds the second
    instantiation of the step's kernel."""
    from drone2d_amd import _build

    with open(_build.PPO_OUT, "rb") as f:
        blob = f.read()
    assert np.frombuffer(blob[:4], np.uint8).tolist() == [0x7F, 0x45, 0x4C, 0x46]
    for sym in (b"d2d_ppo_rollout_step_tb", b"d2d_ppo_tb_version", b"rollout_step_tb_kernel", b"gfx950"):
        assert sym in blob, sym
