"""d2d_ppo_rollout_step_tb on an MI355X: the time-limit bootstrap inside the fused rollout step against
the kernel's own value head (bit for bit), against the torch restatement (the value head's float
tolerance), and end to end inside ``PPO`` on a batch that times out every five steps -- eager,
captured, replayed, and resumed from a saved agent."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1  # hipErrorInvalidValue
OUTS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "done_buf", "start0", "act_env", "adv_buf",
        "ret_buf", "stats")


def _ptr(x):
    return x.data_ptr() if x is not None else None


class _Bufs:
    """One set of rollout buffers (NaN / zero canaries) and the ABI struct over them."""

    def __init__(self, n, T, log_std, gamma, gae_lambda):
        from drone2d_amd import abi
        from drone2d_amd.ppo import D2DPPORollout

        f = lambda *sh: torch.full(sh, float("nan"), device=DEV)  # noqa: E731
        self.obs_buf, self.act_buf, self.logp_buf, self.val_buf = f(T, n, 27), f(T, n, 2), f(T, n), f(T, n)
        self.rew_buf, self.adv_buf, self.ret_buf, self.act_env = f(T, n), f(T, n), f(T, n), f(n, 2)
        self.done_buf = torch.zeros(T, n, dtype=torch.bool, device=DEV)
        self.start0 = torch.ones(n, dtype=torch.bool, device=DEV)
        self.stats = torch.zeros(T, (n + 63) // 64, 2, dtype=torch.float64, device=DEV)
        self.r = D2DPPORollout(n=n, T=T, info_dim=abi.INFO_DIM, info_totrew=abi.INFO_TOTREW, gamma=gamma,
                               gae_lambda_gamma=gamma * gae_lambda, log_std=_ptr(log_std),
                               **{k: _ptr(getattr(self, k)) for k in OUTS})

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in OUTS}


def _same(a, b):
    """torch.equal with NaN == NaN (the canaries): the same bits."""
    if a.dtype.is_floating_point:
        return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))
    return torch.equal(a, b)


def _kernel_values(lib, wptr, log_std, rows):
    """The value the rollout step's value head gives each row of ``rows`` [m][27]: the existing
    d2d_ppo_rollout_step at t = 0 with the rows as observations, ``val_buf`` read back."""
    m = rows.shape[0]
    b = _Bufs(m, 1, log_std, 0.99, 0.95)
    rows = rows.contiguous()
    noise = torch.zeros(m, 2, device=DEV)
    b.r.t, b.r.obs, b.r.noise = 0, _ptr(rows), _ptr(noise)
    assert lib.d2d_ppo_rollout_step(C.byref(b.r), wptr, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return b.val_buf[0].clone()


def _trunc_pattern(n, T):
    """Which envs truncated at steps 0 .. T-1.  n = 229 (four workgroups of 64 envs, the last ragged):
    step 0 -- workgroup 0 none, workgroup 1 exactly one (lane 63), workgroup 2 all 64, workgroup 3 a few
    with the last valid row; step 1 -- another pattern (one in a first tile, a whole second tile, an
    empty workgroup, the last row).  Other n: the last row, at every step."""
    tr = torch.zeros(T, n, dtype=torch.bool)
    if n == 64 * 3 + 37:
        tr[0, 127] = True
        tr[0, 128:192] = True
        tr[0, [195, 200, 228]] = True
        tr[1, 0] = True
        tr[1, 160:192] = True
        tr[1, 228] = True
    else:
        tr[:, n - 1] = True
    return tr.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(n):
    """Inputs and runs shared by the tests below, computed once per n: T = 2 steps through the new
    entry point, through the old one, and through the new one with prev_term_obs = NULL."""
    from drone2d_amd import abi
    from drone2d_amd.ppo import ActorCritic, ManualStep, PPOConfig

    torch.manual_seed(0)
    pol = ActorCritic()
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([-0.4, 0.3]))
        pol.action_net.weight.mul_(60.0)  # actions beyond [-1, 1]: the clip is exercised
    pol = pol.cuda()
    cfg = PPOConfig()
    man = ManualStep(pol, cfg, DEV)
    lib, wptr, st = man.lib, man.weight_ptrs(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=DEV).manual_seed(1)
    T = 2
    obs = torch.rand(T + 1, n, 27, device=DEV, generator=g) * 2 - 1
    noise = torch.randn(T, n, 2, device=DEV, generator=g)
    rews = torch.randn(T, n, device=DEV, generator=g)
    truncs = _trunc_pattern(n, T)
    terms = (torch.rand(T, n, device=DEV, generator=g) < 0.2) & ~truncs
    info = torch.randn(T, n, abi.INFO_DIM, device=DEV, generator=g)
    # terminal observations: random on the truncated rows, NaN on every other row
    tobs = torch.where(truncs[..., None], torch.rand(T, n, 27, device=DEV, generator=g) * 2 - 1,
                       torch.full((), float("nan"), device=DEV))
    assert int(torch.isnan(tobs).any(-1).sum()) == T * n - int(truncs.sum())
    V = torch.stack([_kernel_values(lib, wptr, pol.log_std, torch.nan_to_num(tobs[t], nan=0.0)) for t in range(T)])
    last_v = _kernel_values(lib, wptr, pol.log_std, obs[T])

    def run(entry, with_tobs):
        b = _Bufs(n, T, pol.log_std, cfg.gamma, cfg.gae_lambda)
        for t in range(T + 1):
            b.r.t, b.r.obs, b.r.noise = t, _ptr(obs[t]), _ptr(noise[t]) if t < T else None
            if t > 0:
                b.r.prev_rew, b.r.prev_term, b.r.prev_trunc, b.r.prev_info = (
                    _ptr(rews[t - 1]), _ptr(terms[t - 1]), _ptr(truncs[t - 1]), _ptr(info[t - 1]))
            if entry == "tb":
                rc = lib.d2d_ppo_rollout_step_tb(C.byref(b.r), _ptr(tobs[t - 1]) if with_tobs and t > 0 else None, wptr, st)
            else:
                rc = lib.d2d_ppo_rollout_step(C.byref(b.r), wptr, st)
            assert rc == 0
        torch.cuda.synchronize()
        return b

    return dict(pol=pol, cfg=cfg, lib=lib, wptr=wptr, st=st, n=n, T=T, obs=obs, noise=noise, rews=rews, truncs=truncs,
                terms=terms, info=info, tobs=tobs, V=V, last_v=last_v, new=run("tb", True), old=run("old", False),
                null=run("tb", False))


@pytest.mark.parametrize("n", [64 * 3 + 37, 1, 65])
def test_abi_matches_the_kernels_own_value_head_bit_for_bit(d2, n):
    """On truncated rows ``rew_buf`` is ``prev_rew + gamma32 * V`` in float32 with V from the step's own
    value head (the existing entry point on the same 27 floats, at other rows of another batch size); on
    every other row it is ``prev_rew``, bit for bit, though those rows' terminal observations are NaN.
    Everything else the step writes is the old entry point's; GAE is ``compute_gae`` of the kernel's own
    rewards and values."""
    from drone2d_amd.ppo import compute_gae

    c = _case(n)
    new, old, T, cfg = c["new"], c["old"], c["T"], c["cfg"]
    truncs, terms, rews, V = c["truncs"], c["terms"], c["rews"], c["V"]
    assert not (truncs & terms).any() and terms.any() == (n > 1) and truncs[:, n - 1].all()
    gamma32 = torch.tensor(cfg.gamma, dtype=torch.float32, device=DEV)
    want = torch.where(truncs, rews + gamma32 * V, rews)
    print(f"n={n}: truncated rows {int(truncs.sum())}, max |gamma V| {float((gamma32 * V)[truncs].abs().max()):.4g}")
    assert torch.equal(new.rew_buf[truncs], want[truncs])
    assert torch.equal(new.rew_buf[~truncs], rews[~truncs])
    assert not torch.isnan(new.rew_buf).any()
    assert not torch.equal(new.rew_buf[truncs], rews[truncs])  # (the bootstrap is not a no-op)
    assert torch.equal(old.rew_buf, rews)
    for k in ("done_buf", "stats", "start0", "act_buf", "logp_buf", "val_buf", "obs_buf", "act_env"):
        assert torch.equal(getattr(new, k), getattr(old, k)), k
    assert torch.equal(new.done_buf, terms | truncs)
    # GAE on the kernel's own rewards and values
    dones = terms | truncs
    starts = torch.cat([torch.ones(1, n, dtype=torch.bool, device=DEV), dones[:-1]])
    adv_ref, ret_ref = compute_gae(new.rew_buf, new.val_buf, starts, c["last_v"], dones[T - 1], cfg.gamma,
                                   cfg.gae_lambda)
    assert not torch.isnan(new.adv_buf).any() and not torch.isnan(new.ret_buf).any()
    torch.testing.assert_close(new.adv_buf, adv_ref, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(new.ret_buf, ret_ref, rtol=1e-5, atol=2e-5)
    d = dones[T - 1]  # the bootstrap value of the last observation drops out: torch's bits
    assert d[n - 1] and torch.equal(new.adv_buf[:, d], adv_ref[:, d]) and torch.equal(new.ret_buf[:, d], ret_ref[:, d])
    # prev_term_obs = NULL: the old entry point, everywhere
    for k in OUTS:
        assert _same(getattr(c["null"], k), getattr(old, k)), k


def test_argument_errors_launch_nothing(d2):
    c = _case(65)
    lib, wptr, st, n, T = c["lib"], c["wptr"], c["st"], c["n"], c["T"]
    b = _Bufs(n, T, c["pol"].log_std, c["cfg"].gamma, c["cfg"].gae_lambda)
    before = b.snapshot()
    tobs = torch.nan_to_num(c["tobs"][0], nan=0.0)

    def args(t, **over):
        r = b.r
        r.t, r.obs, r.noise = t, _ptr(c["obs"][min(max(t, 0), T)]), _ptr(c["noise"][min(max(t, 0), T - 1)])
        r.prev_rew, r.prev_term, r.prev_trunc, r.prev_info = (_ptr(c["rews"][0]), _ptr(c["terms"][0]),
                                                             _ptr(c["truncs"][0]), _ptr(c["info"][0]))
        saved = {k: getattr(r, k) for k in over}
        for k, v in over.items():
            setattr(r, k, v)
        return r, saved

    for t, bad in ((1, dict(obs=None)), (1, dict(prev_trunc=None)), (1, dict(prev_rew=None)), (1, dict(rew_buf=None)),
                   (1, dict(stats=None)), (1, dict(noise=None)), (1, dict(T=0)), (3, {}), (-1, {}),
                   (1, dict(info_totrew=99)), (2, dict(adv_buf=None)), (2, dict(start0=None)), (0, dict(val_buf=None))):
        for p in (_ptr(tobs), None):
            r, saved = args(t, **bad)
            assert lib.d2d_ppo_rollout_step_tb(C.byref(r), p, wptr, st) == INVALID, (t, bad)
            for k, v in saved.items():
                setattr(r, k, v)
    r, _ = args(1)
    assert lib.d2d_ppo_rollout_step_tb(None, _ptr(tobs), wptr, st) == INVALID
    assert lib.d2d_ppo_rollout_step_tb(C.byref(r), _ptr(tobs), None, st) == INVALID
    torch.cuda.synchronize()
    for k, v in before.items():
        assert _same(getattr(b, k), v), k
    assert lib.d2d_ppo_tb_version() == 1


def test_value_matches_the_torch_restatement(d2):
    """V of the truncated rows against ``predict_values`` of the same terminal observations, within the
    project's bound for this kernel's value head (tests/test_ppo.py test_rollout_step_matches_torch)."""
    c = _case(64 * 3 + 37)
    truncs, tobs, pol = c["truncs"], c["tobs"], c["pol"]
    with torch.no_grad():
        ref = pol.predict_values(tobs[truncs])
    assert not torch.isnan(ref).any() and int(truncs.sum()) == 68 + 34
    print(f"max |V - predict_values| {float((c['V'][truncs] - ref).abs().max()):.3g}")
    torch.testing.assert_close(c["V"][truncs], ref, rtol=1e-5, atol=2e-5)


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


@pytest.mark.parametrize("norm_reward", [False, True])
def test_ppo_fused_rollout_bootstraps_truncations(d2, tmp_path, norm_reward):
    """Three rollouts (eager, captured, replayed) of 256 envs x 16 steps on a batch whose episodes time
    out every 5 steps: the rollout is the fused one, and ``_ro["rew"]`` equals bit for bit the reward of
    an identically built batch that replays the clipped actions (through the normaliser's twin with
    ``norm_reward``), plus ``gamma32 * V(terminal_obs)`` on truncated rows, V from the kernel's own value
    head under that rollout's policy.  Then a saved agent resumes on the fused path with the same
    rollout as the uninterrupted run."""
    from drone2d_amd import abi
    from drone2d_amd.normalize import RMS_INIT, reward_norm_host
    from drone2d_amd.ppo import PPO, PPOConfig

    N, T = 256, 16
    kw = _train_kw(scenario="large_free", n_steps=5)
    mk = lambda seed: d2.Drone2dVecEnv(N, seed=seed, timeup_truncates=True, **kw)  # noqa: E731
    venv, raw = mk(5), mk(5)
    algo = PPO(venv, PPOConfig.gpu_defaults(n_steps=T, batch_size=1024, n_epochs=2, norm_reward=norm_reward), seed=1)
    raw.reset()
    ret, rms = np.zeros(N), np.array(RMS_INIT)
    gamma32 = torch.tensor(algo.cfg.gamma, dtype=torch.float32, device=DEV)
    for k in range(3):
        rec = algo.collect_rollouts()
        assert algo._truncates and algo._fused and (algo._ro_graph is not None) == (k > 0)
        acts = algo._flat[1].reshape(T, N, 2).clamp(-1.0, 1.0)
        rews = torch.zeros(T, N, device=DEV)
        truncs = torch.zeros(T, N, dtype=torch.bool, device=DEV)
        tobs = torch.zeros(T, N, 27, device=DEV)
        fin, tot = 0, 0.0
        for t in range(T):
            _, rew, term, trunc, info = raw.step(acts[t].contiguous())
            truncs[t] = trunc != 0
            tobs[t] = torch.where(truncs[t][:, None], raw.terminal_obs, 0.0)
            assert not ((term != 0) & truncs[t]).any()
            if norm_reward:
                rews[t] = torch.from_numpy(reward_norm_host(rew.cpu().numpy(), term.cpu().numpy(), trunc.cpu().numpy(),
                                                            ret, rms, algo.cfg.gamma, 10.0, 1e-8)).to(DEV)
            else:
                rews[t] = rew
            done = ((term != 0) | truncs[t]).cpu().numpy()
            assert torch.equal(algo._ro["done"][t].cpu(), torch.from_numpy(done)), (k, t)
            fin += int(done.sum())
            tot += float(info.cpu().numpy()[done, abi.INFO_TOTREW].astype(np.float64).sum())
        V = _kernel_values(algo.manual.lib, algo.manual.weight_ptrs(), algo.policy.log_std,
                           tobs.reshape(T * N, 27)).reshape(T, N)
        want = torch.where(truncs, rews + gamma32 * V, rews)
        n_trunc, quiet = int(truncs.sum()), int((~truncs.any(1)).sum())
        print(f"rollout {k}: truncated rows {n_trunc}, steps with none {quiet}, episodes {fin}")
        assert n_trunc >= 3 * N and quiet > 0
        assert torch.equal(algo._ro["rew"], want), k
        assert not torch.equal(algo._ro["rew"][truncs], rews[truncs])
        if norm_reward:
            assert torch.equal(algo.normalizer.rms.cpu(), torch.from_numpy(rms)), k
        assert rec["episodes"] == fin and fin >= n_trunc
        assert rec["mean_return"] == pytest.approx(tot / fin, rel=1e-9)
        algo.train()
    # save, then the uninterrupted run's next rollout against a loaded agent's on a fresh truncating batch
    path = algo.save(str(tmp_path / "agent.zip"))
    algo.collect_rollouts()
    flat = [x.clone() for x in algo._flat]
    fresh = mk(77)
    back = PPO.load(path, fresh)
    assert back._truncates and back._fused and back._ro["obs_cur"] is not None
    back.collect_rollouts()
    assert back._fused and back._ro_graph is None
    for a, b in zip(flat, back._flat):
        assert torch.equal(a, b)
    assert torch.equal(algo._ro["rew"], back._ro["rew"])
    for v in (venv, raw, fresh):
        v.close()
