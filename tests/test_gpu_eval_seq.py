"""The sequenced evaluation step (``d2d_eval_step_seq``: the call index in device memory) and the loop
replayed as a captured HIP graph on an MI355X: the step against the by-value step for the same ``t``,
its argument checks, a captured segment replayed against eager by-value iterations, the closed loops
``evaluate_policy(graph=True)`` / ``evaluate_policies(graph=True)`` against their eager selves, and
``EvalLoop``.  Everything here is an equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
AGENT = os.path.join(HERE, "golden", "agent_17_90.npz")
CAP = 7          # flight_cap of the step tests
SENT = -7.25     # what untouched outputs hold


def _test_kw(**over):
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, **over)


@pytest.fixture(scope="module")
def policies(d2):
    """Three actors on the device: the shipped agent and two random ones away from their init."""
    from drone2d_amd.ppo import ActorCritic

    out = [ActorCritic.from_agent_npz(AGENT)]
    for k in (1, 2):
        torch.manual_seed(k)
        p = ActorCritic()
        with torch.no_grad():
            p.log_std.copy_(torch.tensor([-0.4, 0.3]) * k)
            p.action_net.weight.mul_(10.0 * k)
        out.append(p)
    return [p.cuda() for p in out]


@pytest.fixture(scope="module")
def stepped(d2):
    """n -> the outputs of one real env step of n corridor envs under random actions (the step, among
    the first 80, at which most envs ended an episode), cloned and never modified."""
    cache = {}

    def get(n):
        if n not in cache:
            venv = d2.Drone2dVecEnv(n, seed=2, with_info=True, **_test_kw(scenario="corridor"))
            g = torch.Generator(device="cuda").manual_seed(3)
            venv.reset(seed=2)
            best = None
            for _ in range(80):
                obs, _, term, trunc, info = venv.step(torch.rand(n, 2, device="cuda", generator=g) * 2 - 1)
                k = int((term | trunc).sum())
                if best is None or k > best[0]:
                    best = (k, dict(obs=obs.clone(), term=term.clone(), trunc=trunc.clone(), info=info.clone(),
                                    tobs=venv.terminal_obs.clone()))
            venv.close()
            cache[n] = best[1]
        return cache[n]

    return get


def _call(kind, t, data, mode, ws=None, bank=None, record=True, flight=True):
    """One step of ``kind`` ('value' or 'seq') at call index ``t`` over ``data``; every output, and the
    return code.  ``flight`` has two rows more than ``CAP``; every third env (1, 4, ...) has already finished."""
    from drone2d_amd import abi, evaluate

    lib = evaluate.load()
    n = int(data["obs"].shape[0])
    out = dict(act_env=torch.full((n, 2), SENT, device="cuda"), noise_out=torch.full((n, 2), SENT, device="cuda"),
               rows=torch.full((n, abi.INFO_DIM), SENT, device="cuda"),
               finished=(torch.arange(n, device="cuda") % 3 == 1).to(torch.uint8),
               remaining=torch.full((1,), n, dtype=torch.int32, device="cuda"),
               flight=torch.full((CAP + 2, n, 2), float("nan"), device="cuda"),
               t_dev=torch.full((1,), t, dtype=torch.int32, device="cuda"))
    a = evaluate.D2DEvalStepArgs(n=n, t=t if kind == "value" else 0, info_dim=abi.INFO_DIM, act=1, noise_mode=mode,
                                 flight_cap=CAP, env_id_base=11, seed=77, obs=data["obs"].data_ptr(),
                                 act_env=out["act_env"].data_ptr(), noise_out=out["noise_out"].data_ptr())
    if ws is not None:
        evaluate._weights_into(a, ws)
    if record:
        a.prev_term, a.prev_trunc = data["term"].data_ptr(), data["trunc"].data_ptr()
        a.prev_info, a.prev_term_obs = data["info"].data_ptr(), data["tobs"].data_ptr()
        a.finished, a.rows, a.remaining = out["finished"].data_ptr(), out["rows"].data_ptr(), out["remaining"].data_ptr()
        if flight:
            a.flight = out["flight"].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    if kind == "seq":
        rc = lib.d2d_eval_step_seq(C.byref(a), C.byref(bank) if bank is not None else None, out["t_dev"].data_ptr(), st)
    elif bank is not None:
        rc = lib.d2d_eval_step_bank(C.byref(a), C.byref(bank), st)
    else:
        rc = lib.d2d_eval_step(C.byref(a), st)
    torch.cuda.synchronize()
    return rc, out


OUTPUTS = ("act_env", "noise_out", "rows", "finished", "remaining", "flight")


def _same_outputs(got, ref, what):
    for k in OUTPUTS:
        a, b = got[k], ref[k]
        if a.is_floating_point():  # NaN == NaN: compare the bits
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), (what, k)


def _check_seq_against_value(data, mode, t, ws=None, bank=None):
    """The sequenced step at *t_dev = t against the by-value step at args.t = t.  t = 0: the by-value
    call gets no record half (the sequenced one is given it and must skip it); t = CAP + 1: the by-value
    call, which refuses that t with flight, gets no flight (the sequenced one must do all but that)."""
    rc, got = _call("seq", t, data, mode, ws, bank)
    assert rc == 0
    rc, ref = _call("value", t, data, mode, ws, bank, record=t >= 1, flight=t <= CAP)
    assert rc == 0
    _same_outputs(got, ref, (t, mode))
    assert int(got["t_dev"]) == t + 1
    nan = torch.isnan(got["flight"])
    assert bool(nan[CAP:].all())  # nothing from row flight_cap on is ever written
    if 1 <= t <= CAP:
        written = ~nan.all(-1)
        n = int(got["finished"].numel())
        was = torch.arange(n, device="cuda") % 3 == 1
        assert torch.equal(written[t - 1], ~was) and int(written.sum()) == int((~was).sum())  # row t - 1 alone
        fresh = (data["term"] | data["trunc"]) & ~was
        assert int(got["remaining"]) == n - int(fresh.sum())  # the record half ran
    else:
        assert bool(nan.all())
    return got


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_seq_step_equals_by_value_step(d2, policies, stepped, n, mode):
    from drone2d_amd import evaluate

    data = stepped(n)
    ws = evaluate.actor_tensors(policies[1], torch.device("cuda", torch.cuda.current_device()))
    seen = []
    for t in (0, 1, 5, CAP, CAP + 1):
        got = _check_seq_against_value(data, mode, t, ws=ws)
        assert float(got["act_env"].abs().max()) <= 1.0
        seen.append(got["noise_out"].clone())
    if mode == 2:  # the index reached the Philox counter: another t, another draw
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    rc, _ = _call("value", CAP + 1, data, mode, ws)
    assert rc == 1  # (the by-value call does refuse that t with flight)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_seq_step_with_a_bank_equals_bank_step(d2, policies, stepped, n, mode):
    from drone2d_amd import evaluate

    data = stepped(n)
    bank = evaluate.PolicyBank(policies, device="cuda")
    for ep in (torch.arange(n) % 3, torch.arange(n) // 100):
        ep = ep.to(torch.int32).cuda()
        cb = bank.c_bank(ep)
        for t in (0, 1, 5, CAP, CAP + 1):
            got = _check_seq_against_value(data, mode, t, bank=cb)
        # bank invariance carries over: a row is the single-actor sequenced step's row under its policy
        for p in range(3):
            rows = torch.nonzero(ep == p).squeeze(1)
            if len(rows):
                _, one = _call("seq", CAP + 1, data, mode, ws=bank.tensors(p))
                assert torch.equal(got["act_env"][rows], one["act_env"][rows]), p


def test_seq_step_refuses_contradictory_arguments(d2, policies, stepped):
    """Each refusal returns hipErrorInvalidValue (1) and launches nothing: the outputs keep their sentinel
    and the index stays."""
    from drone2d_amd import abi, evaluate

    lib = evaluate.load()
    assert lib.d2d_eval_seq_version() == evaluate.SEQ_VERSION == 1
    assert lib.d2d_eval_abi_version() == 1 and lib.d2d_eval_bank_version() == 1
    data = stepped(65)
    n = 65
    ws = evaluate.actor_tensors(policies[0], torch.device("cuda", torch.cuda.current_device()))
    bank = evaluate.PolicyBank(policies, device="cuda")
    cb = bank.c_bank((torch.arange(n) % 3).to(torch.int32).cuda())
    act_env = torch.full((n, 2), SENT, device="cuda")
    rows = torch.full((n, abi.INFO_DIM), SENT, device="cuda")
    fin = torch.zeros(n, dtype=torch.uint8, device="cuda")
    rem = torch.full((1,), n, dtype=torch.int32, device="cuda")
    flight = torch.full((CAP, n, 2), float("nan"), device="cuda")
    t_dev = torch.full((1,), 3, dtype=torch.int32, device="cuda")

    def args(**over):
        a = evaluate.D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, act=1, noise_mode=2, flight_cap=CAP, seed=1,
                                     obs=data["obs"].data_ptr(), act_env=act_env.data_ptr(),
                                     prev_term=data["term"].data_ptr(), prev_trunc=data["trunc"].data_ptr(),
                                     prev_info=data["info"].data_ptr(), prev_term_obs=data["tobs"].data_ptr(),
                                     finished=fin.data_ptr(), rows=rows.data_ptr(), remaining=rem.data_ptr(),
                                     flight=flight.data_ptr())
        evaluate._weights_into(a, ws)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def seq(a, bank=None, t=t_dev.data_ptr()):
        return lib.d2d_eval_step_seq(C.byref(a), C.byref(bank) if bank is not None else None, t, 0)

    bad = [seq(args(t=1)), seq(args(t=-1)),                     # the index is not the struct's to give
           seq(args(), t=None),                                  # no index
           lib.d2d_eval_step_seq(None, None, t_dev.data_ptr(), 0),
           seq(args(n=0)), seq(args(act=0, prev_term=None, prev_trunc=None, prev_info=None)),  # d2d_eval_step's
           seq(args(prev_trunc=None)), seq(args(act_env=None)), seq(args(w2=None)), seq(args(noise_mode=3)),
           seq(args(noise_mode=1)), seq(args(prev_term_obs=None)), seq(args(flight_cap=-1)),
           seq(args(env_id_base=-1)),
           seq(args(), bank=cb),                                 # a bank and an actor of its own
           seq(args(w1=None, b1=None, w2=None, b2=None, w3=None, b3=None, log_std=None),
               bank=evaluate.D2DEvalBank(n_policies=0, params=cb.params, env_policy=cb.env_policy))]
    torch.cuda.synchronize()
    assert bad == [1] * len(bad)
    assert bool((act_env == SENT).all()) and bool((rows == SENT).all()) and bool(torch.isnan(flight).all())
    assert int(fin.sum()) == 0 and int(rem) == n and int(t_dev) == 3
    assert seq(args()) == 0  # and the same arguments without a contradiction run
    torch.cuda.synchronize()
    assert int(t_dev) == 4 and not bool((act_env == SENT).any())
    assert int(rem) == n - int((data["term"] | data["trunc"]).sum()) == n - int(fin.sum())
    assert not bool(torch.isnan(flight[2]).any()) and bool(torch.isnan(flight[:2]).all())


def test_captured_segment_replays_with_the_index_moving(d2):
    """A 4-iteration segment of (d2d_eval_step_seq, d2d_step) captured once and replayed three times ==
    12 eager iterations of the by-value step on an identically built batch.  A frozen ``t`` would repeat
    steps 0-3's noise and write flight rows 0-2 only."""
    from drone2d_amd import abi, evaluate, harness

    lib = evaluate.load()
    ws = evaluate.actor_tensors(harness.MlpActor.from_npz(AGENT), torch.device("cuda", torch.cuda.current_device()))
    n, K, R, cap = 256, 4, 3, 20
    out = []
    for graph in (False, True):
        venv = d2.Drone2dVecEnv(n, seed=4, with_info=True, **_test_kw(scenario="corridor"))
        fin = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rows = torch.zeros(n, abi.INFO_DIM, device="cuda")
        rem = torch.full((1,), n, dtype=torch.int32, device="cuda")
        act_env = torch.empty(n, 2, device="cuda")
        flight = torch.full((cap, n, 2), float("nan"), device="cuda")
        t_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        a = evaluate.D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, act=1, noise_mode=evaluate.NOISE_PHILOX, seed=4,
                                     flight_cap=cap, act_env=act_env.data_ptr())
        evaluate._weights_into(a, ws)
        state = {"obs": venv.reset(seed=4)}

        def iterate(t):
            a.obs = state["obs"].data_ptr()
            st = torch.cuda.current_stream().cuda_stream
            if graph:
                evaluate._step_seq(lib, a, None, t_dev.data_ptr(), st)
            else:
                a.t = t
                evaluate._step(lib, a, st)
            state["obs"], _, term, trunc, info = venv.step(act_env)
            a.prev_term, a.prev_trunc, a.prev_info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
            a.prev_term_obs = venv.terminal_obs.data_ptr()
            a.finished, a.rows, a.remaining, a.flight = fin.data_ptr(), rows.data_ptr(), rem.data_ptr(), flight.data_ptr()

        def rewind():
            state["obs"] = venv.reset(seed=4)
            fin.zero_()
            rows.zero_()
            rem.fill_(n)
            flight.fill_(float("nan"))
            t_dev.zero_()
            if not graph:  # the by-value step at t = 0 takes no record half
                for k in ("prev_term", "prev_trunc", "prev_info", "prev_term_obs", "finished", "rows", "remaining",
                          "flight"):
                    setattr(a, k, None)

        # both arms: K iterations issued eagerly first (the library's kernels loaded; K is even, so the
        # env's double-buffered outputs, and with them `a`, are back at their first parity), then a rewind
        for t in range(K):
            iterate(t)
        rewind()
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):  # iteration 0 holds the record half's pointers and skips it at t = 0
                for t in range(K):
                    iterate(t)
            for _ in range(R):
                g.replay()
        else:
            for t in range(K * R):
                iterate(t)
        torch.cuda.synchronize()
        out.append(dict(obs=state["obs"].clone(), finished=fin, rows=rows, remaining=rem, act_env=act_env,
                        flight=flight, t=int(t_dev)))
        venv.close()
    eager, replayed = out
    assert replayed["t"] == K * R
    for k in ("obs", "finished", "rows", "remaining", "act_env"):
        assert torch.equal(eager[k], replayed[k]), k
    assert torch.equal(eager["flight"].view(torch.int32), replayed["flight"].view(torch.int32))
    written = ~torch.isnan(eager["flight"]).all(-1).all(-1)
    assert written.tolist() == [True] * (K * R - 1) + [False] * (cap - K * R + 1)


def _same(m, ref):
    assert set(m) == set(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(m[k], v, err_msg=k)  # NaN == NaN here
        else:
            assert m[k] == v, k


def _both_arms(d2, policy, n, kw, env_scenario=None, **ev):
    from drone2d_amd.evaluate import evaluate_policy

    res = []
    for graph in (False, True):
        venv = d2.Drone2dVecEnv(n, seed=6, with_info=True, env_scenario=env_scenario, **kw)
        res.append(evaluate_policy(venv, policy, seed=6, flight_paths=True, graph=graph, **ev))
        venv.close()
    _same(res[1], res[0])
    return res[0]


@pytest.mark.parametrize("check_every", [16, 6, 5])
@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_closed_loop_replayed_equals_eager_on_corridor(d2, policies, n, deterministic, check_every):
    m = _both_arms(d2, policies[0], n, _test_kw(scenario="corridor"), deterministic=deterministic,
                   check_every=check_every)
    assert m["unfinished"] == 0 and m["successes"] + m["fails"] == n


@pytest.mark.parametrize("check_every", [16, 6, 5])
@pytest.mark.parametrize("deterministic", [True, False])
def test_closed_loop_replayed_equals_eager_on_seven_scenarios(d2, policies, deterministic, check_every):
    from drone2d_amd.config import TEST_SCENARIOS
    from drone2d_amd.evaluate import sweep_layout

    es = sweep_layout(1, len(TEST_SCENARIOS), 8)[1]
    m = _both_arms(d2, policies[0], len(es), _test_kw(scenario=list(TEST_SCENARIOS)), env_scenario=es,
                   deterministic=deterministic, check_every=check_every)
    assert m["unfinished"] == 0


@pytest.mark.parametrize("check_every", [16, 6, 5])
@pytest.mark.parametrize("deterministic", [True, False])
def test_closed_loop_with_a_cap_that_leaves_envs_unfinished(d2, policies, deterministic, check_every):
    """max_steps = 40: the tail is shorter than a segment and some envs have not finished."""
    m = _both_arms(d2, policies[0], 300, _test_kw(scenario="corridor"), deterministic=deterministic,
                   check_every=check_every, max_steps=40)
    assert 0 < m["unfinished"] <= 300  # (on the eager arm: _both_arms returns it)


def test_bank_loop_replayed_equals_eager(d2, policies):
    from drone2d_amd.config import TEST_SCENARIOS
    from drone2d_amd.evaluate import PolicyBank, evaluate_policies, sweep_layout

    bank = PolicyBank(policies, device="cuda")
    ep, es = sweep_layout(3, len(TEST_SCENARIOS), 8)
    res = []
    for graph in (False, True):
        venv = d2.Drone2dVecEnv(len(ep), seed=6, with_info=True, env_scenario=es,
                                **_test_kw(scenario=list(TEST_SCENARIOS)))
        res.append(evaluate_policies(venv, bank, ep, split=es, seed=6, flight_paths=True, graph=graph))
        venv.close()
    assert set(res[0]) == set(res[1]) and len(res[0]) == 3 * len(TEST_SCENARIOS)
    for key, ref in res[0].items():
        _same(res[1][key], ref)


def test_graph_refusals(d2, policies, monkeypatch):
    from drone2d_amd import evaluate, harness

    venv = d2.Drone2dVecEnv(8, seed=1, with_info=True, **_test_kw(scenario="corridor"))
    with pytest.raises(ValueError, match="torch"):
        evaluate.evaluate_policy(venv, policies[0], noise="torch", graph=True)
    with pytest.raises(ValueError, match="keep_actions"):
        evaluate.evaluate_policy(venv, policies[0], keep_actions=True, graph=True)
    with pytest.raises(ValueError, match="HIP"):
        evaluate.evaluate_policy(object(), policies[0], graph=True)
    monkeypatch.setattr(harness, "_dist_world", lambda: (None, 0, 2))
    with pytest.raises(ValueError, match="more than one rank"):
        evaluate.evaluate_policy(venv, policies[0], graph=True)
    with pytest.raises(ValueError, match="more than one rank"):
        evaluate.evaluate_policies(venv, policies, np.zeros(8, np.int32), graph=True)
    venv.close()


def test_eval_loop_reads_live_weights_and_recaptures_when_they_move(d2):
    from drone2d_amd import evaluate
    from drone2d_amd.ppo import ActorCritic

    policy = ActorCritic.from_agent_npz(AGENT).cuda()
    kw = _test_kw(scenario="corridor")
    n = 130

    def fresh():
        venv = d2.Drone2dVecEnv(n, seed=8, with_info=True, **kw)
        m = evaluate.evaluate_policy(venv, policy, seed=8, flight_paths=True)
        venv.close()
        return m

    def run(loop):
        fin, rows, xy, nobs, _, _ = loop.run(8)
        return evaluate._records(loop.venv, fin, rows, xy, nobs)

    venv = d2.Drone2dVecEnv(n, seed=8, with_info=True, **kw)
    loop = evaluate.EvalLoop(venv, policy, flight_paths=True, graph=True)
    first, again = run(loop), run(loop)
    _same(again, first)
    _same(first, fresh())
    assert loop.captures == 1
    with torch.no_grad():  # in place: the replay must read the new values through the old addresses
        for p in policy.mlp_extractor.policy_net.parameters():
            p.mul_(0.9)
        policy.action_net.bias.add_(0.05)
    moved = run(loop)
    assert loop.captures == 1
    _same(moved, fresh())
    assert not np.array_equal(moved["rewards"], first["rewards"])
    with torch.no_grad():  # new storage: the loop notices and captures again
        w = policy.mlp_extractor.policy_net[2].weight
        w.data = (w.data * 1.05).clone()
    _same(run(loop), fresh())
    assert loop.captures == 2
    venv.close()
