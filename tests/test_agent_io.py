"""Agent files and the evaluation front end without a GPU: save / load / resume / checkpoint of
``ppo.PPO`` on the CPU oracle backend, ``ActorCritic.from_sb3_zip``, ``MlpActor.from_policy``,
``evaluate_policy``'s delegation to the torch loop, and the host restatement of the evaluation
library's Philox policy noise (the formula the GPU tests compare the device against)."""
import io
import json
import os
import zipfile

import numpy as np
import torch

from oracle_backend import OracleVecBackend

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SB3_NAMES = {"log_std", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"} | {
    f"mlp_extractor.{net}.{k}.{p}" for net in ("policy_net", "value_net") for k in (0, 2) for p in ("weight", "bias")}


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _algo(be, seed=0):
    from drone2d_amd.ppo import PPO, PPOConfig

    return PPO(be, PPOConfig(n_steps=8, batch_size=64, n_epochs=2), seed=seed, device="cpu")


def _members(path):
    with zipfile.ZipFile(path) as z:
        return {n: z.read(n) for n in z.namelist()}


def test_save_load_round_trip(d2, tmp_path):
    from drone2d_amd.harness import MlpActor
    from drone2d_amd.ppo import PPO, ActorCritic

    be = OracleVecBackend(32, seed=3, **_train_kw(scenario="corridor"))
    algo = _algo(be)
    algo.learn(8 * 32)
    path = algo.save(str(tmp_path / "agent.zip"))
    mem = _members(path)
    # the oracle backend has no state_dict: no env member
    assert set(mem) == {"data.json", "policy.pth", "train_state.pth"}
    data = json.loads(mem["data.json"])
    assert set(data) == {"format_version", "config", "num_timesteps", "n_envs", "seed"}
    assert data["num_timesteps"] == 256 and data["n_envs"] == 32 and data["seed"] == 0
    assert data["config"]["n_steps"] == 8 and data["config"]["batch_size"] == 64
    loaded = {n: torch.load(io.BytesIO(b), weights_only=True) for n, b in mem.items() if n.endswith(".pth")}
    assert set(loaded["policy.pth"]) == SB3_NAMES
    assert {"m", "v", "t", "gen", "perm_ctr", "last_obs", "start0"} <= set(loaded["train_state.pth"])
    sd = algo.policy.state_dict()

    ac = ActorCritic.from_sb3_zip(path)
    assert set(ac.state_dict()) == SB3_NAMES
    for k, v in ac.state_dict().items():
        assert torch.equal(v, sd[k]), k
    obs = torch.randn(50, 27)
    with torch.no_grad():
        assert torch.equal(MlpActor.from_policy(ac)(obs), ac(obs)[0])
        assert torch.equal(MlpActor.from_policy(ac).log_std, ac.log_std)

    back = PPO.load(path, be, device="cpu")
    for k, v in back.policy.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert back.num_timesteps == 256 and back.cfg == algo.cfg and back.seed == 0
    for a, b in ((back.manual.m, algo.manual.m), (back.manual.v, algo.manual.v), (back.manual.t, algo.manual.t)):
        assert torch.equal(a, b)
    assert torch.equal(back.gen.get_state(), algo.gen.get_state())
    be.close()


def test_from_sb3_zip_actor_only_and_errors(d2, tmp_path):
    """A zip whose policy.pth holds the actor alone loads (fresh value net); one without policy.pth or
    with a missing actor tensor is refused."""
    import pytest

    from drone2d_amd.ppo import ActorCritic

    ref = ActorCritic.from_agent_npz(os.path.join(GOLD, "agent_17_90.npz"))
    actor = {k: v for k, v in ref.state_dict().items() if "value_net" not in k}

    def write(name, sd):
        p = str(tmp_path / name)
        with zipfile.ZipFile(p, "w") as z:
            if sd is not None:
                buf = io.BytesIO()
                torch.save(sd, buf)
                z.writestr("policy.pth", buf.getvalue())
            z.writestr("data", "{}")
        return p

    ac = ActorCritic.from_sb3_zip(write("actor.zip", actor))
    for k, v in actor.items():
        assert torch.equal(ac.state_dict()[k], v), k
    with pytest.raises(ValueError):
        ActorCritic.from_sb3_zip(write("none.zip", None))
    del actor["action_net.bias"]
    with pytest.raises(ValueError):
        ActorCritic.from_sb3_zip(write("short.zip", actor))


def test_resume_is_exact(d2, tmp_path):
    """3 updates in one go == 1 update, save, load onto the same running backend, 2 more."""
    from drone2d_amd.ppo import PPO

    be_a = OracleVecBackend(32, seed=3, **_train_kw(scenario="corridor"))
    a = _algo(be_a)
    a.learn(3 * 256)
    be_b = OracleVecBackend(32, seed=3, **_train_kw(scenario="corridor"))
    b0 = _algo(be_b)
    b0.learn(256)
    path = b0.save(str(tmp_path / "b.zip"))
    del b0
    b = PPO.load(path, be_b, device="cpu")
    hist = b.learn(3 * 256)
    assert len(hist) == 2 and a.num_timesteps == b.num_timesteps == 768
    for (k, p), q in zip(a.policy.state_dict().items(), b.policy.state_dict().values()):
        assert torch.equal(p, q), k
    assert torch.equal(a.manual.m, b.manual.m) and torch.equal(a.manual.v, b.manual.v)
    assert torch.equal(a.manual.t, b.manual.t)
    be_a.close()
    be_b.close()


def test_resume_is_exact_torch_optimiser(d2, tmp_path):
    """The same with ``manual=False``: the torch optimiser's state is what the file carries."""
    from drone2d_amd.ppo import PPO, PPOConfig

    cfg = PPOConfig(n_steps=8, batch_size=64, n_epochs=2, manual=False)
    be_a = OracleVecBackend(32, seed=3, **_train_kw(scenario="corridor"))
    a = PPO(be_a, cfg, seed=1, device="cpu")
    a.learn(2 * 256)
    be_b = OracleVecBackend(32, seed=3, **_train_kw(scenario="corridor"))
    b0 = PPO(be_b, cfg, seed=1, device="cpu")
    b0.learn(256)
    b = PPO.load(b0.save(str(tmp_path / "b.zip")), be_b, device="cpu")
    b.learn(2 * 256)
    for (k, p), q in zip(a.policy.state_dict().items(), b.policy.state_dict().values()):
        assert torch.equal(p, q), k
    sa, sb = a.opt.state_dict()["state"], b.opt.state_dict()["state"]
    for i in sa:
        for k in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(torch.as_tensor(sa[i][k]), torch.as_tensor(sb[i][k])), (i, k)
    be_a.close()
    be_b.close()


def test_checkpoint_files(d2, tmp_path):
    from drone2d_amd.ppo import PPO, Checkpoint

    be = OracleVecBackend(32, seed=3, **_train_kw(scenario="corridor"))
    algo = _algo(be)
    ck = str(tmp_path / "ck")
    algo.learn(3 * 256, checkpoint=Checkpoint(256, ck, "rl_model"))
    assert sorted(os.listdir(ck)) == sorted(f"rl_model_{k}_steps.zip" for k in (256, 512, 768))
    for k in (256, 512, 768):
        back = PPO.load(os.path.join(ck, f"rl_model_{k}_steps.zip"), be, device="cpu")
        assert back.num_timesteps == k
    for p, q in zip(back.policy.parameters(), algo.policy.parameters()):
        assert torch.equal(p, q)
    # a save_freq the rollouts step over: one file per crossing, none in between
    ck2 = str(tmp_path / "ck2")
    _algo(be).learn(3 * 256, checkpoint=Checkpoint(500, ck2))
    assert sorted(os.listdir(ck2)) == ["rl_model_512_steps.zip"]
    be.close()


def test_predict_cpu(d2):
    be = OracleVecBackend(8, seed=3, **_train_kw(scenario="corridor"))
    algo = _algo(be)
    obs = torch.randn(8, 27)
    with torch.no_grad():
        mean = algo.policy(obs)[0].clamp(-1, 1)
    assert torch.equal(algo.predict(obs, deterministic=True), mean)
    a1, a2 = algo.predict(obs), algo.predict(obs)
    assert a1.shape == (8, 2) and float(a1.abs().max()) <= 1.0
    assert not torch.equal(a1, mean) and not torch.equal(a1, a2)  # stochastic by default, a new draw per call
    be.close()


def test_evaluate_policy_delegates_on_oracle_backend(d2):
    from drone2d_amd import harness
    from drone2d_amd.config import ENV_TEST_CONFIG
    from drone2d_amd.evaluate import evaluate_policy
    from drone2d_amd.ppo import ActorCritic

    path = os.path.join(GOLD, "agent_17_90.npz")
    kw = dict(ENV_TEST_CONFIG, scenario="corridor")
    be = OracleVecBackend(12, seed=3, **kw)
    ref = harness.run_first_episodes(be, harness.MlpActor.from_npz(path), seed=3, flight_paths=True)
    be.close()
    for pol in (harness.MlpActor.from_npz(path), ActorCritic.from_agent_npz(path)):
        be = OracleVecBackend(12, seed=3, **kw)
        m = evaluate_policy(be, pol, seed=3, flight_paths=True)
        be.close()
        assert set(m) == set(ref) and m["unfinished"] == 0
        for k, v in ref.items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(m[k], v, err_msg=k)
            else:
                assert m[k] == v, k


def test_philox_noise_host(d2, oracle_mod):
    """The host restatement of noise mode 2: its Philox words are the oracle's, and 200 000 draws have
    mean and standard deviation within 4 standard errors of N(0, 1)'s."""
    from drone2d_amd import evaluate

    seed = 0x1234_5678_9ABC_DEF0
    key = (seed & 0xFFFFFFFF, seed >> 32)
    f = np.float32
    for g, t in ((0, 0), (1, 0), (999, 1100), (65535, 7), (2 ** 32 - 1, 2 ** 31)):
        w = oracle_mod.philox((g, t, evaluate.NOISE_TAG, 0), key)
        assert [int(x) for x in evaluate._philox4x32(np.array([[g], [t], [evaluate.NOISE_TAG], [0]], np.uint64), key)[:, 0]] == w
        u0 = (f(w[0] >> 8) + f(0.5)) * f(2.0 ** -24)
        u1 = (f(w[1] >> 8) + f(0.5)) * f(2.0 ** -24)
        r = np.sqrt(f(-2.0) * np.log(u0))
        a = f(2.0 * np.pi) * u1
        z = evaluate.philox_noise_host(seed, [g], t)[0]
        assert z.dtype == np.float32 and z[0] == f(r * np.cos(a)) and z[1] == f(r * np.sin(a))
    z = np.concatenate([evaluate.philox_noise_host(seed, np.arange(50_000), t) for t in (0, 1)]).astype(np.float64)
    assert z.shape == (100_000, 2)  # 200 000 draws
    n = z.size
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 4 / np.sqrt(n)
    assert abs(z.std() - 1.0) < 4 / np.sqrt(2 * n)  # se of a normal sample's standard deviation
    assert abs(np.mean(z[:, 0] * z[:, 1])) < 4 / np.sqrt(n / 2)  # the pair is uncorrelated
    # streams at different steps and under different seeds differ
    assert not np.array_equal(evaluate.philox_noise_host(seed, np.arange(8), 0), evaluate.philox_noise_host(seed, np.arange(8), 1))
    assert not np.array_equal(evaluate.philox_noise_host(seed, np.arange(8), 0), evaluate.philox_noise_host(seed + 1, np.arange(8), 0))


def test_eval_args_struct_matches_header(d2):
    """The ctypes struct has the header's fields in the header's order (a layout slip would make the
    kernel read the wrong pointers)."""
    import re

    from drone2d_amd import evaluate

    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "d2d_eval.h")).read()
    body = hdr[hdr.index("typedef struct d2d_eval_step_args {"):hdr.index("} d2d_eval_step_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+);", body)
    assert names == [f[0] for f in evaluate.D2DEvalStepArgs._fields_]
    assert f"#define D2D_EVAL_ABI_VERSION {evaluate.ABI_VERSION}" in hdr
    assert f"0x{evaluate.NOISE_TAG:08X}u".lower() in hdr.lower()
    import ctypes as C

    assert C.sizeof(evaluate.D2DEvalStepArgs) == 6 * 4 + 2 * 8 + 19 * 8
