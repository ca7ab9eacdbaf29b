"""PPO control (include/d2d_ppo.h "PPO control", DESIGN.md "PPO control"): learning-rate / clip-range
schedules, SB3's clip_range_vf, approx_kl and the target_kl early stop, read from and decided in a
device-resident control block so that all of it works inside the captured update.

CPU: the schedules, the two torch paths (ManualStep on CPU tensors, autograd) against a float64
restatement of SB3's train loop, stop-before-any-step, agent files, logs, two gloo ranks.  GPU: the
control kernels against the default path (bit for bit when neutral), against torch, and the captured
update against the eager one and against hand-issued steps."""
import csv
import ctypes as C
import json
import math
import os
import socket
import subprocess
import types
import zipfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import REPO
from oracle_backend import OracleVecBackend

STATS = ("policy_loss", "value_loss", "entropy", "clip_fraction")
CONTROL_KEYS = ("approx_kl", "n_minibatches", "early_stop", "learning_rate", "clip_range", "clip_range_vf")
INF = float("inf")


def _kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _cpu_algo(be=None, seed=0, **over):
    from drone2d_amd.ppo import PPO, PPOConfig

    be = be or OracleVecBackend(32, seed=3, **_kw(scenario="corridor"))
    return PPO(be, PPOConfig(**dict(dict(n_steps=8, batch_size=64, n_epochs=2), **over)), seed=seed, device="cpu"), be


def _f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------- CPU
def test_control_block_matches_header(tmp_path, d2):
    """ppo.D2DPPOCtl mirrors include/d2d_ppo.h's d2d_ppo_ctl word for word."""
    from drone2d_amd.ppo import PPO_CTL_VERSION, ControlBlock, D2DPPOCtl

    hdr = os.path.join(REPO, "include", "d2d_ppo.h")
    prog = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{hdr}"', "int main(void){",
            'printf("size %zu\\n", sizeof(d2d_ppo_ctl));', 'printf("version %d\\n", (int)D2D_PPO_CTL_VERSION);']
    prog += [f'printf("{f} %zu\\n", offsetof(d2d_ppo_ctl, {f}));' for f, _ in D2DPPOCtl._fields_]
    prog.append("return 0;}")
    src = tmp_path / "ctl.c"
    src.write_text("\n".join(prog))
    subprocess.run(["gcc", "-o", str(tmp_path / "ctl"), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "ctl")], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(D2DPPOCtl) == 4 * ControlBlock.WORDS == 32
    assert int(out["version"]) == PPO_CTL_VERSION
    for i, (f, _) in enumerate(D2DPPOCtl._fields_):
        assert int(out[f]) == getattr(D2DPPOCtl, f).offset == 4 * i, f
    names = [f for f, _ in D2DPPOCtl._fields_]
    for f in ("lr", "clip", "clip_vf", "kl_limit", "stop", "count", "kl_sum", "kl_last"):
        assert names.index(f) == getattr(ControlBlock, f.upper())


def test_defaults_leave_the_control_path_off(d2):
    from drone2d_amd.ppo import PPOConfig

    cfg = PPOConfig()
    assert not cfg.control and cfg.coefs(0.3) == (cfg.learning_rate, cfg.clip_range, -1.0, INF)
    for over in (dict(learning_rate_end=1e-5), dict(clip_range_end=0.1), dict(clip_range_vf=0.2), dict(target_kl=INF)):
        assert PPOConfig(**over).control
    algo, be = _cpu_algo()
    assert algo._ctl is None and algo.manual.ctl is None
    rec = algo.learn(256)[0]
    assert not any(k in rec for k in CONTROL_KEYS)
    be.close()


def test_schedules_follow_progress_remaining(d2):
    """Over a 4-update learn the recorded learning_rate and clip_range are linear in SB3's
    progress_remaining (set after each rollout, before its update) and end at the _end values."""
    from drone2d_amd.ppo import PPOConfig

    lr0, lr1, c0, c1 = 3e-4, 1e-5, 0.2, 0.05
    for manual in (True, False):
        algo, be = _cpu_algo(learning_rate=lr0, learning_rate_end=lr1, clip_range=c0, clip_range_end=c1, manual=manual)
        assert algo.progress_remaining == 1.0
        hist = algo.learn(4 * 256)
        assert len(hist) == 4
        for u, h in enumerate(hist):
            pr = 1.0 - (u + 1) * 256 / (4 * 256)
            assert h["learning_rate"] == _f32(lr1 + (lr0 - lr1) * pr), (u, h["learning_rate"])
            assert h["clip_range"] == _f32(c1 + (c0 - c1) * pr), (u, h["clip_range"])
            assert "clip_range_vf" not in h and h["early_stop"] == 0 and h["n_minibatches"] == 8
            assert np.isfinite(h["approx_kl"])
        assert hist[-1]["learning_rate"] == _f32(lr1) and hist[-1]["clip_range"] == _f32(c1)
        assert algo.progress_remaining == 0.0
        # train() on its own reads algo.progress_remaining
        algo.collect_rollouts()
        algo.progress_remaining = 0.5
        assert algo.train()["learning_rate"] == _f32(lr1 + (lr0 - lr1) * 0.5)
        be.close()
    for name in ("learning_rate", "clip_range"):
        with pytest.raises(TypeError, match=name + "_end"):
            PPOConfig(**{name: lambda p: 3e-4 * p})


def _band_problem(M, n_mb, c_vf=0.25, seed=1):
    """A policy away from its init, M samples in n_mb equal minibatches and old values around the
    value clip band.  Minibatch k's old log-probs are off by noise of scale (0.1, 0.2, 0.4, 0.4, ...)[k]
    (one minibatch: 0.3, as tests/test_ppo.py has it), so its KL is about scale^2 / 2 whatever the steps
    before it did.  Every 16th sample's observation is
    zero: with zero hidden biases its value is the output bias 0.5 exactly, in float32 and float64
    alike, and its old value sits exactly on the lower (0.25) or upper (0.75) bound of the band around
    it, or well outside; the other samples' old values are spread below, inside and above the band."""
    from drone2d_amd.ppo import ActorCritic

    torch.manual_seed(0)
    ref = ActorCritic()
    with torch.no_grad():
        ref.log_std.copy_(torch.tensor([-0.3, 0.2]))
        ref.action_net.weight.mul_(30.0)
        ref.value_net.bias.fill_(0.5)
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(M, 27, generator=g) * 0.5
    zero = torch.arange(0, M, 16)
    X[zero] = 0.0
    A = torch.randn(M, 2, generator=g)
    ADV = torch.randn(M, generator=g)
    R = torch.randn(M, generator=g) * 3
    bs = M // n_mb
    scale = torch.tensor([0.3] if n_mb == 1 else [0.1, 0.2] + [0.4] * (n_mb - 2)).repeat_interleave(bs)
    with torch.no_grad():
        mean, V = ref(X)
        OL = ref.log_prob(mean, A) + torch.randn(M, generator=g) * scale
        assert torch.equal(V[zero], torch.full((len(zero),), 0.5))
        # old = V - d: d in the band's units, cycling below / inside / above
        d = torch.tensor([-2.0, -0.5, 0.0, 0.5, 2.0, -1.3, 0.9, 1.1])[torch.arange(M) % 8] * c_vf
        OV = V - d + torch.randn(M, generator=g) * 0.01
        OV[zero] = torch.tensor([0.25, 0.75, 0.25 - 0.5, 0.75 + 0.5])[torch.arange(len(zero)) % 4]
    return ref, (X, A, OL, ADV, R, OV)


def _restatement(ref, data, minibatches, cfg, lr, c, c_vf, target_kl, steps=True):
    """SB3 2.1 PPO.train's loop in float64: loss, record statistics, approx_kl, break, step."""
    pol = type(ref)().double()
    pol.load_state_dict({k: v.double() for k, v in ref.state_dict().items()})
    X, A, OL, ADV, R, OV = (t.double() for t in data)
    opt = torch.optim.Adam(pol.parameters(), lr=lr, eps=1e-5)
    out = {k: [] for k in STATS + ("approx_kl",)}
    grads, stop = [], False
    for idx in minibatches:
        values, logp, ent = pol.evaluate_actions(X[idx], A[idx])
        adv = ADV[idx]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        log_ratio = logp - OL[idx]
        ratio = torch.exp(log_ratio)
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
        values_pred = values if c_vf is None else OV[idx] + torch.clamp(values - OV[idx], -c_vf, c_vf)
        vl = torch.nn.functional.mse_loss(R[idx], values_pred)
        loss = pl + cfg.ent_coef * (-ent.mean()) + cfg.vf_coef * vl
        out["policy_loss"].append(pl.item())
        out["value_loss"].append(vl.item())
        out["entropy"].append(ent.mean().item())
        out["clip_fraction"].append(((ratio - 1).abs() > c).double().mean().item())
        with torch.no_grad():
            kl = ((ratio - 1) - log_ratio).mean().item()
        out["approx_kl"].append(kl)
        opt.zero_grad()
        loss.backward()
        grads.append([p.grad.clone() for p in pol.parameters()])
        if target_kl is not None and kl > 1.5 * target_kl:
            stop = True
            break
        if not steps:
            break
        torch.nn.utils.clip_grad_norm_(list(pol.parameters()), cfg.max_grad_norm)
        opt.step()
    return pol, out, grads, stop


def _check_stats(rec, ref_out):
    n = len(ref_out["approx_kl"])
    close = torch.testing.assert_close
    t = lambda x: torch.tensor(x, dtype=torch.float64)  # noqa: E731
    mean = lambda k: t(sum(ref_out[k]) / n)  # noqa: E731
    close(t(rec["policy_loss"]), mean("policy_loss"), rtol=1e-5, atol=1e-7)
    close(t(rec["value_loss"]), mean("value_loss"), rtol=1e-5, atol=1e-6)
    close(t(rec["entropy"]), mean("entropy"), rtol=1e-6, atol=1e-6)
    close(t(rec["clip_fraction"]), mean("clip_fraction"), rtol=0, atol=1e-7)
    close(t(rec["approx_kl"]), mean("approx_kl"), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("manual", [True, False], ids=["manual", "autograd"])
def test_torch_paths_match_sb3_restatement(d2, manual):
    """ManualStep on CPU tensors and the autograd path against the float64 restatement, on the same
    four minibatches, with clip_range_vf on and old values below / inside / exactly on / above the band.
    The KLs are about 0.005, 0.02, 0.08, 0.08 and the limit 1.5 * 0.03, so all three stop at the third
    minibatch: its statistics count, its step is not taken."""
    from drone2d_amd.ppo import PPO, PPOConfig

    M, n_mb, c_vf, tkl = 256, 4, 0.25, 0.03
    ref, data = _band_problem(M, n_mb, c_vf)
    cfg = PPOConfig(n_steps=8, batch_size=M // n_mb, n_epochs=1, clip_range_vf=c_vf, target_kl=tkl, manual=manual)
    algo = PPO(types.SimpleNamespace(num_envs=M // 8, device="cpu"), cfg, policy=ref.__class__(), seed=0, device="cpu")
    algo.policy.load_state_dict(ref.state_dict())  # in place: ManualStep's flat buffer holds the parameters
    algo._alloc_rollout()
    # minibatch k = the k-th block of samples (its KL scale), in a shuffled order inside the block
    g = torch.Generator().manual_seed(5)
    mbs = [k * (M // n_mb) + torch.randperm(M // n_mb, generator=g) for k in range(n_mb)]
    for dst, src in zip(algo._flat, data[:5]):
        dst.copy_(src)
    algo._ro["val"].reshape(-1).copy_(data[5])
    pol64, out, grads, stop = _restatement(ref, data, mbs, cfg, cfg.learning_rate, cfg.clip_range, c_vf, tkl)
    assert stop and len(out["approx_kl"]) == 3 and 1.5 * out["approx_kl"][1] < 1.5 * tkl < out["approx_kl"][2] / 1.5
    ctl = algo._ctl
    ctl.set(*cfg.coefs())
    ctl.reset()
    for k, idx in enumerate(mbs):
        if manual:
            with torch.no_grad():
                algo.manual.grad(idx, algo._rollout_data(), algo._acc)
                if k < len(grads):
                    for (name, p), gr in zip(algo.policy.named_parameters(), grads[k]):
                        torch.testing.assert_close(p.grad.double(), gr, rtol=2e-4, atol=1e-7, msg=f"{name} mb {k}")
                algo.manual.apply()
        else:
            algo._minibatch(idx)
            if k == 2:  # (a minibatch that stepped has had its .grad clipped in place; the stopping one has not)
                for (name, p), gr in zip(algo.policy.named_parameters(), grads[k]):
                    torch.testing.assert_close(p.grad.double(), gr, rtol=2e-4, atol=1e-7, msg=f"{name} mb {k}")
        assert ctl.stopped() == (k >= 2)
    rec = ctl.read()
    assert rec["n_minibatches"] == 3 and rec["early_stop"] == 1 and rec["clip_range_vf"] == c_vf
    _check_stats(rec, out)
    for (name, p), q in zip(algo.policy.named_parameters(), pol64.parameters()):
        torch.testing.assert_close(p.detach().double(), q.detach(), rtol=1e-4, atol=1e-6, msg=name)
    t = algo.manual.t if manual else next(iter(algo.opt.state.values()))["step"]
    assert float(t) == 2.0


def _state(algo):
    return [x.detach().clone() for x in (algo.manual.P, algo.manual.m, algo.manual.v, algo.manual.t)]


def test_stop_before_any_step(d2):
    """target_kl = -1: the first minibatch's KL (about 0) exceeds the limit, so the update records that
    minibatch and changes nothing; with the limit lifted the next update trains (the flag was reset)."""
    algo, be = _cpu_algo(target_kl=-1.0)
    twin, be2 = _cpu_algo(target_kl=INF)
    for a in (algo, twin):
        a.collect_rollouts()
    before = _state(algo)
    gen = algo.gen.get_state()
    rec = algo.train()
    for a, b in zip(before, _state(algo)):
        assert torch.equal(a, b)
    assert rec["n_minibatches"] == 1 and rec["early_stop"] == 1
    # the twin's first minibatch, by hand
    twin._ctl.set(*twin.cfg.coefs())
    twin._ctl.reset()
    for v in twin._acc.values():
        v.zero_()
    perm = torch.randperm(256, generator=twin.gen)
    twin._minibatch(perm[:64])
    one = twin._ctl.read()
    for k in STATS + ("approx_kl",):
        assert rec[k] == one[k], k
    # a stopped update has drawn all its shuffles
    g2 = torch.Generator().manual_seed(0)
    g2.set_state(gen)
    for _ in range(algo.cfg.n_epochs):
        torch.randperm(256, generator=g2)
    assert torch.equal(g2.get_state(), algo.gen.get_state())
    algo.collect_rollouts()
    algo.cfg.target_kl = INF
    rec = algo.train()
    assert rec["n_minibatches"] == 8 and rec["early_stop"] == 0
    assert not torch.equal(before[0], algo.manual.P) and float(algo.manual.t) == 8.0
    be.close()
    be2.close()


def test_agent_files_carry_the_control_fields(d2, tmp_path):
    from drone2d_amd.ppo import AGENT_FORMAT_VERSION, PPO, Checkpoint

    over = dict(learning_rate_end=1e-5, clip_range_end=0.05, clip_range_vf=0.3, target_kl=INF)
    full, be_a = _cpu_algo(**over)
    # the uninterrupted run leaves a checkpoint after its second update; the other run is that file resumed
    lrs = [h["learning_rate"] for h in full.learn(4 * 256, checkpoint=Checkpoint(512, str(tmp_path)))]
    path = str(tmp_path / "rl_model_512_steps.zip")
    part, be_b = _cpu_algo(**over)
    part.learn(2 * 256, schedule_timesteps=4 * 256)  # (brings the resumed run's backend to the same state)
    with zipfile.ZipFile(path) as z:
        data = json.loads(z.read("data.json"))
    assert set(data) == {"format_version", "config", "num_timesteps", "n_envs", "seed"}
    assert data["format_version"] == AGENT_FORMAT_VERSION == 1
    for k, v in over.items():
        assert data["config"][k] == v
    back = PPO.load(path, be_b, device="cpu")
    assert back.cfg == part.cfg and back.cfg.target_kl == INF and back._ctl is not None
    # resumed with the same total_timesteps: the schedule continues from num_timesteps
    hist = back.learn(4 * 256)
    assert [h["learning_rate"] for h in hist] == lrs[2:] and len(lrs) == 4
    for p, q in zip(full.policy.parameters(), back.policy.parameters()):
        assert torch.equal(p, q)
    # a file written before the fields existed
    old = str(tmp_path / "old.zip")
    with zipfile.ZipFile(path) as z, zipfile.ZipFile(old, "w") as o:
        for n in z.namelist():
            b = z.read(n)
            if n == "data.json":
                d = json.loads(b)
                for k in over:
                    del d["config"][k]
                b = json.dumps(d)
            o.writestr(n, b)
    legacy = PPO.load(old, be_b, device="cpu")
    assert not legacy.cfg.control and legacy._ctl is None and legacy.cfg.n_steps == 8
    be_a.close()
    be_b.close()


def test_scalar_log_writes_the_control_keys_only_when_present(d2, tmp_path):
    from drone2d_amd.trainlog import ScalarLog, read_progress

    base = {"episodes": 2.0, "mean_return": 1.5, "policy_loss": 0.1, "value_loss": 0.2, "entropy": 2.8,
            "clip_fraction": 0.0, "timesteps": 256, "env_steps_per_s": 10.0}
    with ScalarLog(str(tmp_path / "plain"), tensorboard=False) as log:
        log.log(base)
    with open(tmp_path / "plain" / "progress.csv", newline="") as f:
        header = next(csv.reader(f))
    assert header == ["step", "train/policy_loss", "train/value_loss", "train/entropy", "train/clip_fraction",
                      "rollout/episodes", "rollout/ep_rew_mean", "time/fps", "time/total_timesteps", "time/episodes"]
    ctl = dict(base, approx_kl=0.01, n_minibatches=5, early_stop=1, learning_rate=3e-4, clip_range=0.2,
               clip_range_vf=0.25)
    with ScalarLog(str(tmp_path / "ctl")) as log:
        log.log(ctl)
        ev = log.event_path
    row = read_progress(str(tmp_path / "ctl" / "progress.csv"))[0]
    for k in CONTROL_KEYS:
        assert row["train/" + k] == float(ctl[k]), k
    data = open(ev, "rb").read()
    for k in CONTROL_KEYS:
        assert b"train/" + k.encode() in data


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out_dir, manual):
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import drone2d_amd  # noqa: F401
    from drone2d_amd import shard
    from drone2d_amd.ppo import PPO, PPOConfig
    from oracle_backend import OracleVecBackend as Backend

    shard.init_process_group_from_env("gloo")
    off, cnt = shard.shard_range(64, world, rank)
    be = Backend(cnt, seed=5, env_id_offset=off, **_kw(scenario="corridor"))
    cfg = PPOConfig(n_steps=8, batch_size=64, n_epochs=10, learning_rate=3e-3, target_kl=2e-3, manual=manual)
    algo = PPO(be, cfg, seed=rank, device="cpu")
    hist = algo.learn(2 * 8 * cnt)
    flat = torch.cat([p.detach().reshape(-1) for p in algo.policy.parameters()])
    torch.save({"params": flat, "n": [h["n_minibatches"] for h in hist], "stop": [h["early_stop"] for h in hist],
                "kl": [h["approx_kl"] for h in hist]}, os.path.join(out_dir, f"ctl_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
    be.close()


@pytest.mark.parametrize("manual", [True, False], ids=["manual", "autograd"])
def test_two_ranks_stop_at_the_same_minibatch(tmp_path, d2, manual):
    """Two gloo ranks with different shards: the KL rides behind the gradient in its collective and the
    decision is taken on the rank mean, so both ranks stop at the same minibatch -- midway through the
    40 planned -- and end with one policy, although their own KLs differ."""
    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, str(tmp_path), manual)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    a, b = (torch.load(os.path.join(tmp_path, f"ctl_{r}.pt"), weights_only=True) for r in range(world))
    assert a["n"] == b["n"] and a["stop"] == b["stop"] == [1, 1]
    assert all(1 < n < 40 for n in a["n"]), a["n"]
    assert a["kl"] != b["kl"]
    assert torch.equal(a["params"], b["params"])


# ---------------------------------------------------------------------------------------------- GPU
N_ENVS, N_STEPS, BS, EPOCHS = 256, 8, 512, 2
M_ALL, N_MB = N_ENVS * N_STEPS, EPOCHS * (N_ENVS * N_STEPS // BS)


def _gpu_algo(d2, graph=True, seed=0, env_seed=1, **over):
    from drone2d_amd.ppo import PPO, PPOConfig

    venv = d2.Drone2dVecEnv(N_ENVS, seed=env_seed, **_kw(scenario="corridor"))
    cfg = PPOConfig(n_steps=N_STEPS, batch_size=BS, n_epochs=EPOCHS, graph=graph, **over)
    algo = PPO(venv, cfg, seed=seed)
    assert algo._hip and algo.manual.fused and algo.use_graph == graph
    return algo, venv


def _update(algo):
    algo.collect_rollouts()
    rec = algo.train()
    torch.cuda.synchronize()
    return rec


@pytest.mark.gpu
def test_neutral_control_equals_default_path(d2):
    """target_kl = inf and schedules that end where they start: the control kernels (the second
    instantiation of the fused gradient, the control reduce and Adam) compute what the default ones
    do, bit for bit, over an eager, a capturing and a replaying update."""
    runs = []
    for over in ({}, dict(target_kl=INF, learning_rate_end=3e-4, clip_range_end=0.2)):
        algo, venv = _gpu_algo(d2, learning_rate=3e-4, clip_range=0.2, **over)
        assert (algo._ctl is not None) == bool(over)
        recs = []
        for u in range(3):
            rec = _update(algo)
            recs.append((rec, _state(algo)))
        assert algo._graph is not None
        runs.append(recs)
        venv.close()
    for (ra, sa), (rb, sb) in zip(*runs):
        for x, y in zip(sa, sb):
            assert torch.equal(x, y)
        for k in STATS:
            assert ra[k] == rb[k], k
        assert rb["n_minibatches"] == N_MB and rb["early_stop"] == 0 and rb["approx_kl"] >= -1e-7
    assert float(runs[1][-1][1][3]) == 3 * N_MB


def _fused_sizes():
    from drone2d_amd.ppo import ppo_native

    lib = ppo_native()
    cap = lib.d2d_ppo_fused_rows(1 << 24)  # the most rows (workgroups per net) the launch uses
    m = 64 * cap + 100
    assert lib.d2d_ppo_fused_rows(m) == cap and m > 64 * lib.d2d_ppo_fused_rows(m)
    return {"one_chunk": 64, "ragged": 1000, "multi_chunk": m}


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["one_chunk", "ragged", "multi_chunk"])
def test_control_head_and_gradient_match_torch(d2, size):
    """One minibatch through d2d_ppo_fused_grad_ctl + d2d_ppo_grad_reduce_ctl with clip_range_vf on and
    old values below / inside / exactly on / above the band: G, the statistics and approx_kl against the
    float64 restatement (multi_chunk: more than 64 * d2d_ppo_fused_rows(m) samples, so a workgroup
    walks more than one chunk)."""
    from drone2d_amd.ppo import ActorCritic, ManualStep, PPOConfig

    M, c_vf = _fused_sizes()[size], 0.25
    ref, data = _band_problem(M, 1, c_vf)
    cfg = PPOConfig(clip_range_vf=c_vf, target_kl=INF)
    _, out, grads, _ = _restatement(ref, data, [torch.arange(M)], cfg, cfg.learning_rate, cfg.clip_range, c_vf, None,
                                    steps=False)
    man = ActorCritic()
    man.load_state_dict(ref.state_dict())
    man = man.to("cuda")
    step = ManualStep(man, cfg, "cuda")
    assert step.lib is not None and step.fused and step.ctl is not None
    g = torch.Generator().manual_seed(9)
    perm = torch.randperm(M, generator=g)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(M)
    rollout = tuple(t[inv].contiguous().to("cuda") for t in data)  # row inv[i] -> sample i
    acc = step.ctl.acc()
    with torch.no_grad():
        step.reset_control()
        step.grad(perm.to("cuda"), rollout, acc)
        torch.cuda.synchronize()
        for (name, p), gr in zip(man.named_parameters(), grads[0]):
            torch.testing.assert_close(p.grad.cpu().double(), gr, rtol=2e-4, atol=1e-7, msg=name)
    rec = step.ctl.read()
    assert rec["n_minibatches"] == 1 and rec["early_stop"] == 0 and rec["clip_range_vf"] == c_vf
    _check_stats(rec, out)
    assert 0.05 < out["clip_fraction"][0] < 0.95 and out["approx_kl"][0] > 1e-3


@pytest.mark.gpu
def test_stop_at_the_first_minibatch_on_the_device(d2):
    """target_kl = -1 through an eager, a capturing and a replaying update: each records its first
    minibatch and leaves the parameters, the moments and t bit-identical; the statistics are those of
    that minibatch alone; with the limit lifted the same graph trains again."""
    from drone2d_amd.ppo import ActorCritic, ManualStep, PPOConfig

    algo, venv = _gpu_algo(d2, target_kl=-1.0)
    start = _state(algo)
    for u in range(3):
        rec = _update(algo)
        assert rec["n_minibatches"] == 1 and rec["early_stop"] == 1, (u, rec)
        for a, b in zip(start, _state(algo)):
            assert torch.equal(a, b)
        # the first minibatch alone: an eager control step on a copy of the policy
        pol = ActorCritic()
        pol.load_state_dict(algo.policy.state_dict())
        one = ManualStep(pol.to("cuda"), PPOConfig(target_kl=INF), "cuda")
        with torch.no_grad():
            one.grad(algo._perm[:BS], algo._rollout_data(), one.ctl.acc())
        alone = one.ctl.read()
        for k in STATS + ("approx_kl",):
            torch.testing.assert_close(torch.tensor(rec[k]), torch.tensor(alone[k]), rtol=1e-6, atol=1e-7, msg=k)
        assert int(algo._perm_ctr) == (u + 1) * EPOCHS  # a stopped update has drawn all its shuffles
    assert algo._graph is not None
    algo.cfg.target_kl = INF
    rec = _update(algo)
    assert rec["n_minibatches"] == N_MB and rec["early_stop"] == 0
    assert not torch.equal(start[0], algo.manual.P) and float(algo.manual.t) == N_MB
    venv.close()


# (learning_rate, PPO seed) candidates for the midway stop, in the order they are tried: the test needs a
# second-epoch minibatch whose KL is at least twice every earlier one's, which depends on the run
# (measured on an MI355X: (3e-3, 2) gives KL_4 = 3.3 x max(KL_0..3); the others 2.0 - 2.2 x)
MIDWAY_CANDIDATES = ((3e-3, 2), (2e-3, 1), (1e-3, 5), (1e-3, 2), (2e-3, 2), (1e-3, 4))


def _probe_midway(d2, lr, seed):
    """Update 0 as usual, then update 1 by hand on a no-stop run: the shuffles, the reset and one eager
    ManualStep.step per minibatch on algo._perm's slices; returns the per-minibatch KLs and the
    optimiser state after each step."""
    from drone2d_amd.ppo import ControlBlock, _ok

    algo, venv = _gpu_algo(d2, graph=False, seed=seed, learning_rate=lr, target_kl=INF)
    _update(algo)
    algo.collect_rollouts()
    man, st = algo.manual, algo.manual._stream()
    _ok(man.lib.d2d_ppo_permute(M_ALL, EPOCHS, algo._perm_seed, algo._perm_ctr.data_ptr(), algo._perm.data_ptr(), st),
        "d2d_ppo_permute")
    man.set_coefs()
    man.reset_control()
    kls, states = [], []
    with torch.no_grad():
        for k in range(N_MB):
            man.step(algo._perm[k * BS:(k + 1) * BS], algo._rollout_data(), algo._acc)
            kls.append(float(man.ctl.buf[ControlBlock.KL_LAST]))
            states.append(_state(algo))
    venv.close()
    return kls, states


def _midway_choice(kls):
    """The first second-epoch minibatch j whose KL is at least twice max(KL_0..j-1), and the limit
    between them (their geometric mean); None if there is none."""
    for j in range(N_MB // EPOCHS, N_MB):
        prev = max(kls[:j])
        if prev > 0 and kls[j] >= 2 * prev:
            return j, math.sqrt(kls[j] * prev)
    return None


@pytest.mark.gpu
def test_midway_stop_graph_equals_eager_equals_by_hand(d2):
    """A target_kl between KL_j and every earlier minibatch's KL (j in the second epoch, a factor of
    two apart so that rounding cannot move the stop): the captured update stops at j, ends bit-identical
    to the eager control run, and both equal exactly j hand-issued ManualStep.step calls."""
    found = None
    for lr, seed in MIDWAY_CANDIDATES:
        kls, states = _probe_midway(d2, lr, seed)
        print("midway probe", lr, seed, ["%.3e" % k for k in kls])
        choice = _midway_choice(kls)
        if choice is not None:
            found = (lr, seed, kls, states, *choice)
            break
    assert found is not None, "no second-epoch minibatch with KL_j >= 2 max(KL_0..j-1) at any candidate"
    lr, seed, kls, states, j, limit = found
    assert j >= N_MB // EPOCHS and max(kls[:j]) < limit < kls[j]
    finals = []
    for graph in (False, True):
        algo, venv = _gpu_algo(d2, graph=graph, seed=seed, learning_rate=lr, target_kl=INF)
        _update(algo)  # update 0: no limit, eager in both runs
        algo.cfg.target_kl = limit / 1.5
        rec = _update(algo)  # graph: captured here and replayed
        assert (algo._graph is not None) == graph
        assert rec["n_minibatches"] == j + 1 and rec["early_stop"] == 1, (graph, rec, kls)
        torch.testing.assert_close(torch.tensor(rec["approx_kl"]), torch.tensor(sum(kls[:j + 1]) / (j + 1)),
                                   rtol=1e-5, atol=1e-9)
        finals.append(_state(algo))
        venv.close()
    for a, b, c in zip(finals[0], finals[1], states[j - 1]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert float(finals[1][3]) == N_MB + j


@pytest.mark.gpu
def test_schedules_under_replay(d2):
    """learning_rate_end = 0 over a 4-update learn: the captured run reads lr from memory, so after
    every update it is bit-identical to the graph=False run; the last update (progress_remaining 0, lr
    0) leaves the parameters as they are while t advances by the full minibatch count."""
    snaps = []
    for graph in (True, False):
        algo, venv = _gpu_algo(d2, graph=graph, learning_rate=3e-4, learning_rate_end=0.0)
        run = []
        hist = algo.learn(4 * M_ALL, log=lambda rec: run.append(_state(algo)))  # noqa: B023
        assert (algo._graph is not None) == graph and len(hist) == 4
        assert [h["learning_rate"] for h in hist] == [_f32(3e-4 * (1 - (u + 1) / 4)) for u in range(4)]
        assert all(h["n_minibatches"] == N_MB for h in hist)
        snaps.append(run)
        venv.close()
    for sa, sb in zip(*snaps):
        for x, y in zip(sa, sb):
            assert torch.equal(x, y)
    g = snaps[0]
    assert not torch.equal(g[1][0], g[2][0])
    assert torch.equal(g[2][0], g[3][0]) and float(g[3][3]) - float(g[2][3]) == N_MB == 8
