"""The fused evaluation step (libd2d_eval.so) and the agent files on an MI355X: the actor against
torch, bitwise row invariance, the Philox policy noise against its host restatement, the recorder
against ``harness.run_first_episodes``, sharding, the closed loop against the reference's published
rates, resuming a saved PPO run on a HIP batch, and ``PPO.predict``."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
AGENT = os.path.join(HERE, "golden", "agent_17_90.npz")


def _test_kw(**over):
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, **over)


def _train_kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


@pytest.fixture(scope="module")
def policies(d2):
    """'shipped': the reference's agent 17_90; 'perturbed': a random ActorCritic away from its init
    (log_std != 0, a larger action head: the clip is exercised)."""
    from drone2d_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pert = ActorCritic()
    with torch.no_grad():
        pert.log_std.copy_(torch.tensor([-0.4, 0.3]))
        pert.action_net.weight.mul_(20.0)
        pert.action_net.bias.copy_(torch.tensor([0.2, -0.1]))
        for lin in (pert.mlp_extractor.policy_net[0], pert.mlp_extractor.policy_net[2]):
            lin.bias.copy_(torch.randn(64) * 0.3)
    return {"shipped": ActorCritic.from_agent_npz(AGENT), "perturbed": pert}


@pytest.fixture(scope="module")
def obs_pool(d2):
    """1000 observation rows of a short rollout (random actions, corridor) and 1000 rows of 3 * randn
    (tanh saturates); CPU float32, never modified."""
    venv = d2.Drone2dVecEnv(250, seed=2, **_test_kw(scenario="corridor"))
    g = torch.Generator(device="cuda").manual_seed(3)
    obs = venv.reset(seed=2)
    real = []
    for t in range(40):
        obs = venv.step(torch.rand(250, 2, device="cuda", generator=g) * 2 - 1)[0]
        if t % 10 == 9:
            real.append(obs.clone())
    real = torch.cat(real).cpu()
    venv.close()
    wide = 3.0 * torch.randn(1000, 27, generator=torch.Generator().manual_seed(4))
    return {"real": real, "wide": wide}


def _ref_actions(ac, obs, z, dtype):
    """clip(mean + exp(log_std) z, -1, 1) in torch on the CPU, in ``dtype``."""
    import copy

    m = copy.deepcopy(ac).to(dtype)
    with torch.no_grad():
        a = m(obs.to(dtype))[0]
        if z is not None:
            a = a + m.log_std.exp() * z.to(dtype)
        return a.clamp(-1.0, 1.0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("which", ["shipped", "perturbed"])
def test_actor_matches_torch(d2, policies, obs_pool, which, n):
    """The act half (modes 0 and 1) against a float64 torch evaluation at rtol 1e-5 / atol 2e-5, the
    project's bound for this forward (test_rollout_step_matches_torch); where torch's own float32
    forward misses that bound on an element, the element's bound is twice torch-float32's error."""
    from drone2d_amd import evaluate

    ac = policies[which]
    zg = torch.randn(n, 2, generator=torch.Generator().manual_seed(n))
    for kind in ("real", "wide"):
        obs = obs_pool[kind][:n]
        for mode, z in ((0, None), (1, zg)):
            got = evaluate.act(ac, obs.cuda(), deterministic=mode == 0, noise=z.cuda() if z is not None else None)
            assert got.shape == (n, 2) and got.dtype == torch.float32
            got = got.cpu().double()
            a64 = _ref_actions(ac, obs, z, torch.float64)
            e32 = (_ref_actions(ac, obs, z, torch.float32).double() - a64).abs()
            err = (got - a64).abs()
            bound = 2e-5 + 1e-5 * a64.abs()
            tol = torch.where(e32 > bound, 2.0 * e32, bound)
            print(f"actor {which} n={n} {kind} mode {mode}: max |hip - f64| {float(err.max()):.3g}, "
                  f"max |torch f32 - f64| {float(e32.max()):.3g}, rows past the bound in torch f32: "
                  f"{int((e32 > bound).any(1).sum())}, clipped {float((a64.abs() >= 1).double().mean()):.2f}")
            assert bool((err <= tol).all()), (which, n, kind, mode, float(err.max()))


@pytest.mark.parametrize("mode", [0, 2])
def test_row_invariance_bitwise(d2, policies, obs_pool, mode):
    """1000 rows in one call == the same rows as [0:333] and [333:1000] (env_id_base moved along) ==
    single-row calls (63 padding rows beside them), bit for bit."""
    from drone2d_amd import evaluate

    obs = torch.cat([obs_pool["real"][:500], obs_pool["wide"][:500]]).cuda()
    for ac in policies.values():
        kw = dict(deterministic=mode == 0, seed=77, t=5)
        full = evaluate.act(ac, obs, env_id_base=0, **kw)
        parts = torch.cat([evaluate.act(ac, obs[:333], env_id_base=0, **kw),
                           evaluate.act(ac, obs[333:], env_id_base=333, **kw)])
        assert torch.equal(full, parts)
        for r in (0, 332, 333, 999):
            one = evaluate.act(ac, obs[r:r + 1], env_id_base=r, **kw)
            assert torch.equal(one[0], full[r]), r
        if mode == 2:  # the noise did something, and another step's or seed's draw is another draw
            assert not torch.equal(full, evaluate.act(ac, obs, deterministic=True))
            assert not torch.equal(full, evaluate.act(ac, obs, env_id_base=0, deterministic=False, seed=77, t=6))
            assert not torch.equal(full, evaluate.act(ac, obs, env_id_base=0, deterministic=False, seed=78, t=5))


def test_philox_noise_matches_host(d2, policies, obs_pool):
    """noise_out of mode 2 against the NumPy restatement (tests/test_agent_io.py pins that one): atol
    2e-5 -- r <= 5.9 times the float32 rounding of 2 pi u1 (<= 4e-7) and a few ulp of cosf / logf is
    under 1e-5."""
    from drone2d_amd import evaluate

    obs = obs_pool["real"][:1000].cuda()
    ac = policies["shipped"]
    seen = {}
    for seed in (0, 0xDEADBEEF12345678):
        for t in (0, 1, 1100):
            a, z = evaluate.act(ac, obs, seed=seed, t=t, return_noise=True)
            ref = evaluate.philox_noise_host(seed, np.arange(1000), t)
            d = np.abs(z.cpu().numpy().astype(np.float64) - ref.astype(np.float64))
            print(f"philox seed {seed:#x} t {t}: max |device - host| {d.max():.3g}")
            assert d.max() <= 2e-5, (seed, t, d.max())
            seen[(seed, t)] = z.cpu()
            # a shard's rows are the global batch's rows
            _, zs = evaluate.act(ac, obs[:300], seed=seed, t=t, env_id_base=700, return_noise=True)
            assert torch.equal(zs.cpu(), seen[(seed, t)][700:])
            # and the action is clip(mean + exp(log_std) z) of that z
            a1 = evaluate.act(ac, obs, noise=z)
            assert torch.equal(a, a1)
    keys = list(seen)
    for i, k in enumerate(keys):
        for k2 in keys[i + 1:]:
            assert not torch.equal(seen[k], seen[k2]), (k, k2)


def test_eval_step_refuses_contradictory_arguments(d2):
    from drone2d_amd import evaluate

    lib = evaluate.load()
    bad = evaluate.D2DEvalStepArgs(n=0, act=1)
    with pytest.raises(evaluate.EvalError):
        evaluate._step(lib, bad, 0)
    with pytest.raises(evaluate.EvalError):  # neither half asked for
        evaluate._step(lib, evaluate.D2DEvalStepArgs(n=8, act=0), 0)


class _Replay:
    """A stub policy for ``run_first_episodes``: replays recorded actions, zeros past the end."""

    def __init__(self, actions):
        self.actions, self.k = actions, 0

    def to(self, device):
        return self

    def act(self, obs, deterministic=False, generator=None, noise=None):
        k, self.k = self.k, self.k + 1
        return self.actions[k] if k < len(self.actions) else torch.zeros_like(self.actions[0])


def _same(m, ref):
    assert set(m) == set(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(m[k], v, err_msg=k)  # NaN == NaN here
        else:
            assert m[k] == v, k


def test_recorder_is_exact(d2):
    """evaluate_policy's records against run_first_episodes fed the very same actions."""
    from drone2d_amd import harness
    from drone2d_amd.evaluate import evaluate_policy

    pol = harness.MlpActor.from_npz(AGENT)
    kw = _test_kw(scenario="corridor")
    venv = d2.Drone2dVecEnv(1000, seed=5, with_info=True, **kw)
    m = evaluate_policy(venv, pol, seed=5, flight_paths=True, keep_actions=True)
    venv.close()
    assert m["unfinished"] == 0 and m["successes"] + m["fails"] == 1000
    actions = torch.from_numpy(m.pop("actions")).cuda()
    assert actions.shape[1:] == (1000, 2) and actions.shape[0] >= int(m["time_spent"].max())
    assert float(actions.abs().max()) <= 1.0
    venv = d2.Drone2dVecEnv(1000, seed=5, with_info=True, **kw)
    ref = harness.run_first_episodes(venv, _Replay(actions), seed=5, flight_paths=True)
    venv.close()
    assert ref["unfinished"] == 0
    _same(m, ref)


def test_sharded_batches_fly_the_unsharded_episodes(d2):
    from drone2d_amd import harness
    from drone2d_amd.evaluate import evaluate_policy

    pol = harness.MlpActor.from_npz(AGENT)
    kw = _test_kw(scenario="corridor")

    def run(n, off):
        venv = d2.Drone2dVecEnv(n, seed=9, with_info=True, env_id_offset=off, **kw)
        m = evaluate_policy(venv, pol, seed=9, flight_paths=True, noise="philox")
        venv.close()
        assert m["unfinished"] == 0
        return m

    whole, parts = run(512, 0), [run(256, 0), run(256, 256)]
    assert whole["successes"] == sum(p["successes"] for p in parts)
    assert whole["fails"] == sum(p["fails"] for p in parts)
    for k in ("collisions", "apes", "time_spent", "rewards"):
        np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts]), err_msg=k)
    T = whole["flight_xy"].shape[0]
    fl = []
    for p in parts:
        f = np.full((T, 256, 2), np.nan)
        f[:p["flight_xy"].shape[0]] = p["flight_xy"]
        fl.append(f)
    np.testing.assert_array_equal(whole["flight_xy"], np.concatenate(fl, 1))
    assert len(set(whole["time_spent"].tolist())) > 10  # not one episode flown 512 times


def test_closed_loop_success_rate(d2):
    """test_agent_success_rate_matches_reference's criterion on corridor, through evaluate_policy."""
    from drone2d_amd import harness
    from drone2d_amd.evaluate import evaluate_policy
    from drone2d_amd.ppo import ActorCritic

    ref = json.load(open(os.path.join(HERE, "golden", "agent_17_90_results.json")))["results"]["corridor"]
    venv = d2.Drone2dVecEnv(1000, seed=5, with_info=True, **_test_kw(scenario="corridor"))
    m = evaluate_policy(venv, ActorCritic.from_agent_npz(AGENT), seed=5)
    venv.close()
    s = harness.summary(m)
    assert m["unfinished"] == 0 and s["Successes"] + s["Fails"] == 1000
    p, q = s["Success rate"], ref["Success rate"]
    se = math.sqrt(max(q * (1 - q), 0.0099) / 100 + max(p * (1 - p), 0.0099) / 1000)
    assert abs(p - q) < 4 * se, (p, q)
    c, cq = s["Collision rate"], ref["Collision rate"]
    sec = math.sqrt(max(cq * (1 - cq), 0.0099) / 100 + max(c * (1 - c), 0.0099) / 1000)
    assert abs(c - cq) < 4 * sec, (c, cq)


def test_eval_loop_captures_into_a_graph(d2):
    """16 x (d2d_eval_step, d2d_step) captured and replayed == the same 16 steps issued eagerly."""
    from drone2d_amd import abi, evaluate, harness

    lib = evaluate.load()
    pol = harness.MlpActor.from_npz(AGENT)
    ws = evaluate.actor_tensors(pol, torch.device("cuda", torch.cuda.current_device()))
    n, T = 256, 16
    out = []
    for graph in (False, True):
        venv = d2.Drone2dVecEnv(n, seed=4, with_info=True, **_test_kw(scenario="corridor"))
        fin = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rows = torch.zeros(n, abi.INFO_DIM, device="cuda")
        rem = torch.full((1,), n, dtype=torch.int32, device="cuda")
        act_env = torch.empty(n, 2, device="cuda")
        obs0 = venv.reset(seed=4)

        def body():
            a = evaluate.D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, noise_mode=evaluate.NOISE_PHILOX, seed=4,
                                         act_env=act_env.data_ptr())
            evaluate._weights_into(a, ws)
            obs = obs0
            st = torch.cuda.current_stream().cuda_stream
            for t in range(T + 1):
                a.t, a.act, a.obs = t, int(t < T), obs.data_ptr()
                evaluate._step(lib, a, st)
                if t == T:
                    break
                obs, _, term, trunc, info = venv.step(act_env)
                a.prev_term, a.prev_trunc, a.prev_info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
                a.finished, a.rows, a.remaining = fin.data_ptr(), rows.data_ptr(), rem.data_ptr()
            return obs

        def rewind():
            venv.reset(seed=4)
            fin.zero_()
            rows.zero_()
            rem.fill_(n)

        body()  # both arms: a first pass issued eagerly (library warm-up, as PPO's rollout graph has it)
        rewind()
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                obs = body()
            g.replay()
        else:
            obs = body()
        torch.cuda.synchronize()
        out.append((obs.clone(), fin.clone(), rows.clone(), rem.clone(), act_env.clone()))
        venv.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert int(out[0][3]) == n - int(out[0][1].sum())


def _ppo_cfg(graph, n_steps=8):
    from drone2d_amd.ppo import PPOConfig

    cfg = PPOConfig.gpu_defaults(n_steps=n_steps, batch_size=2048, n_epochs=2)
    cfg.graph = graph
    return cfg


def test_resume_on_hip_matches_uninterrupted_run(d2, tmp_path):
    """4 updates == 2 updates, save, load into a new batch, 2 more (eager in both arms)."""
    from drone2d_amd.ppo import PPO

    n, per = 1024, 8 * 1024
    kw = _train_kw(scenario="corridor")
    va = d2.Drone2dVecEnv(n, seed=1, **kw)
    a = PPO(va, _ppo_cfg(False), seed=0)
    a.learn(4 * per)
    vb = d2.Drone2dVecEnv(n, seed=1, **kw)
    b0 = PPO(vb, _ppo_cfg(False), seed=0)
    b0.learn(2 * per)
    path = b0.save(str(tmp_path / "agent.zip"))
    import zipfile

    assert set(zipfile.ZipFile(path).namelist()) == {"data.json", "policy.pth", "train_state.pth", "env_state.pth"}
    vc = d2.Drone2dVecEnv(n, seed=123, **kw)
    b = PPO.load(path, vc)
    assert b.num_timesteps == 2 * per and b.device.type == "cuda"
    hist = b.learn(4 * per)
    assert len(hist) == 2 and a.num_timesteps == b.num_timesteps
    bitwise = all(torch.equal(p, q) for p, q in zip(a.policy.parameters(), b.policy.parameters()))
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.policy.parameters(), b.policy.parameters()))
    print(f"resume on HIP: parameters bitwise equal: {bitwise}, max |diff| {worst:.3g}")
    for (k, p), q in zip(a.policy.state_dict().items(), b.policy.state_dict().values()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-5, msg=k)
    for v in (va, vb, vc):
        v.close()


@pytest.mark.parametrize("scn", ["corridor", "fresh_curriculum"])
def test_load_restores_the_env_batch(d2, tmp_path, scn):
    from drone2d_amd.ppo import PPO

    n = 1024
    kw = _train_kw(scenario="corridor") if scn == "corridor" else _train_kw(mode="curriculum", scenario="curriculum",
                                                                            sim_num=2_500_000)
    va = d2.Drone2dVecEnv(n, seed=6, **kw)
    a = PPO(va, _ppo_cfg(False), seed=0)
    a.learn(3 * 8 * n)
    path = a.save(str(tmp_path / "agent.zip"))
    saved = [t.clone() for t in va.get_state()]
    vb = d2.Drone2dVecEnv(n, seed=77, **kw)
    b = PPO.load(path, vb)
    for s, t in zip(saved, vb.get_state()):
        assert torch.equal(s, t)
    assert vb.seed_value == va.seed_value
    assert torch.equal(b._ro["obs_cur"], a._ro["obs_cur"]) and torch.equal(b._ro["start0"], a._ro["start0"])
    assert b._ro_gen == vb.generation  # the next rollout continues instead of resetting
    act = torch.rand(n, 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 2 - 1
    oa, ra, ta = va.step(act)[:3]
    ob, rb, tb = vb.step(act)[:3]
    assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(ta, tb)
    va.close()
    vb.close()


@pytest.mark.parametrize("n_steps", [8, 16])
def test_resume_with_graphs_recaptures(d2, tmp_path, n_steps):
    """graph=True: after a load the first rollout and update run eagerly and the graphs are captured
    again (the rollout's only for whole reset-cache fill periods, n_steps % 16 == 0)."""
    from drone2d_amd.ppo import PPO

    n, per = 1024, n_steps * 1024
    kw = _train_kw(scenario="corridor")
    va = d2.Drone2dVecEnv(n, seed=1, **kw)
    a = PPO(va, _ppo_cfg(True, n_steps), seed=0)
    a.learn(2 * per)
    path = a.save(str(tmp_path / "agent.zip"))
    va.close()
    vb = d2.Drone2dVecEnv(n, seed=1, **kw)
    b = PPO.load(path, vb)
    assert b.use_graph and b._graph is None and b._ro_graph is None
    hist = b.learn(5 * per)
    assert len(hist) == 3
    for h in hist:
        for k in ("policy_loss", "value_loss", "entropy", "clip_fraction"):
            assert np.isfinite(h[k]), (k, h)
    assert b._graph is not None
    assert (b._ro_graph is not None) == (n_steps % 16 == 0)
    vb.close()


def test_predict_is_the_act_half(d2):
    from drone2d_amd import evaluate
    from drone2d_amd.ppo import PPO, ActorCritic

    venv = d2.Drone2dVecEnv(300, seed=2, **_test_kw(scenario="corridor"))
    algo = PPO(venv, _ppo_cfg(False), policy=ActorCritic.from_agent_npz(AGENT), seed=11)
    obs = venv.reset(seed=2)
    a0, a1 = algo.predict(obs), algo.predict(obs)
    assert torch.equal(a0, evaluate.act(algo.policy, obs, seed=11, t=0))
    assert torch.equal(a1, evaluate.act(algo.policy, obs, seed=11, t=1))
    assert not torch.equal(a0, a1)
    det = algo.predict(obs, deterministic=True)
    assert torch.equal(det, evaluate.act(algo.policy, obs, deterministic=True))
    assert torch.equal(det, algo.predict(obs.cpu().numpy(), deterministic=True))
    venv.close()
