"""The PPO update library (csrc/d2d_ppo.hip behind ppo.ManualStep / ppo.PPO) against float64
references and at its edges: Adam from carried and preloaded states, the hand-written tanh point by
point, the minibatch gradient with saturated units and extreme ratios, a whole ``PPO.train()``, the
rollout step's GAE bit for bit, and the shuffles at every small size.

The references, the error measure (relative L2 per buffer against float64; parameters on the
per-step update) and the bound (8 x the error of ManualStep on CPU tensors on the same inputs, at
least one float32 epsilon) are tests/ppo_ref.py.  The unmarked tests run without a device: they check
the references' own pieces and that every listed mutant of the float32 restatement fails the bound on
these inputs by a wide margin, so that passing it means something."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import ppo_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
AGENT = os.path.join(HERE, "golden", "agent_17_90.npz")
INF = float("inf")
MAX_NORM = 0.5
HIP_INVALID = 1  # hipErrorInvalidValue


def _kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _worst(rows, key):
    return max(r[key] for r in rows)


# ================================================================================= 0. self-checks (CPU)
def test_error_measure_and_bound():
    assert R.rel_l2([1.0, 2.0], [1.0, 2.0]) == 0.0 and R.rel_l2([0.0], [0.0]) == 0.0
    assert R.rel_l2([1e-3], [0.0]) == INF and R.rel_l2([float("nan")], [1.0]) == INF
    assert abs(R.rel_l2([3.0, 4.0 + 5e-6], [3.0, 4.0]) - 1e-6) < 1e-12
    assert R.bound(0.0) == 8 * R.EPS32 and R.bound(1e-6) == 8e-6
    # ulp32: the spacing of float32 at 1, just below 1, at 0.25 and in the subnormal range
    assert list(R.ulp32(np.array([1.0, 0.999, 0.25, 1e-42]))) == [2.0 ** -23, 2.0 ** -24, 2.0 ** -25, 2.0 ** -149]


def test_adam64_is_torch_adam_from_a_preloaded_state():
    """Adam64 from (step 3000, m, v) continues a torch.optim.Adam run exactly: 7 steps from scratch equal
    4 steps, a state hand-over and 3 more; and its bias corrections are the float64 ones."""
    gs = R.adam_gradients(50, 7, MAX_NORM, seed=3)
    p0 = torch.randn(50, generator=torch.Generator().manual_seed(0))
    a = R.Adam64(p0, 0.05, MAX_NORM)
    for g in gs:
        a.step(g)
    b = R.Adam64(p0, 0.05, MAX_NORM)
    for g in gs[:4]:
        b.step(g)
    c = R.Adam64(b.p, 0.05, MAX_NORM, step=4, exp_avg=b.m, exp_avg_sq=b.v)
    for g in gs[4:]:
        c.step(g)
    assert torch.equal(a.p, c.p) and torch.equal(a.m, c.m) and torch.equal(a.v, c.v) and a.t == c.t == 7.0
    # one step from t = 3000 by hand
    p, m, v = (x.double() for x in R.adam_warm_state(50, 3000))
    d = R.Adam64(p, 0.05, MAX_NORM, 3000, m, v)
    g = gs[1].double()  # norm 0.999 max_norm: not clipped
    dp, gc = d.step(gs[1])
    assert torch.equal(gc, g) and d.t == 3001.0
    m1, v1 = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
    want = -0.05 / (1 - 0.9 ** 3001) * m1 / (v1.sqrt() / math.sqrt(1 - 0.999 ** 3001) + 1e-5)
    assert R.rel_l2(dp, want) < 1e-12 and R.rel_l2(d.m, m1) < 1e-15 and R.rel_l2(d.v, v1) < 1e-15


def test_gradient_schedule_takes_both_sides_of_the_clip():
    for n in (1, 63, 12101):
        gs = R.adam_gradients(n, 10, MAX_NORM)
        norms = [float(torch.linalg.vector_norm(g)) for g in gs]  # float32 norms, as ManualStep takes them
        for k, x in enumerate(norms):
            lo, hi = ((40.0, 60.0), (0.4994, 0.4996), (0.5004, 0.5006), (0.9e-9, 1.1e-9), (0.0, 0.0))[k % 5]
            assert lo <= x <= hi, (n, k, x)


def test_adam_mutants_fail_the_bound():
    """The comparison of section 1 on the CPU (n = 12101, 20 carried steps from t = 0, lr = 0.05): the
    float32 restatement written out again (ppo_ref.adam32) is bit-identical to ManualStep.apply, and each
    mutant of it exceeds the bound (8 x ManualStep's own error, per buffer and step) by at least 100 x
    on some buffer at some step.

    Measured: ManualStep's error per step: delta p 3.6e-6 .. 9.8e-6, m1 3.6e-7 .. 5.7e-7, m2 8.1e-7 ..
    1.2e-6, clipped gradient 0 .. 7.4e-7.  Worst error / bound per mutant: no_clamp 5.2e11, t_off_by_one
    9.5e3, eps_in_sqrt 2.1e4, bc2_no_sqrt 3.3e4, eps_1e-8 5.2e3, eps_over_bc2s 1.0e4."""
    n, lr = 12101, 0.05
    floor = R.adam_errors(lambda st, g: R.manual_apply(st, lr, MAX_NORM), n, 0, lr, MAX_NORM)
    same = R.adam_errors(lambda st, g: R.adam32(st, lr, MAX_NORM), n, 0, lr, MAX_NORM)
    assert floor == same and all(r["t_ok"] for r in floor)
    keys = ("dp", "m1", "m2", "g")
    print("adam float32 floor:", {k: (min(r[k] for r in floor), _worst(floor, k)) for k in keys})
    for mut in R.ADAM_MUTANTS:
        rows = R.adam_errors(lambda st, g: R.adam32(st, lr, MAX_NORM, mut), n, 0, lr, MAX_NORM)  # noqa: B023
        ratio = max(r[k] / R.bound(f[k]) for r, f in zip(rows, floor) for k in keys)
        print(f"adam mutant {mut}: worst error / bound {ratio:.3g}")
        assert ratio >= 100.0, (mut, ratio)


def test_gae_recursion_matches_compute_gae():
    from drone2d_amd.ppo import compute_gae

    rng = np.random.default_rng(0)
    T, N = 9, 6
    r, v, d, lv = rng.normal(size=(T, N)), rng.normal(size=(T, N)), rng.random((T, N)) < 0.2, rng.normal(size=N)
    starts = np.concatenate([np.ones((1, N), bool), d[:-1]])
    adv, ret = compute_gae(*(torch.as_tensor(x) for x in (r, v, starts, lv, d[-1])), 0.99, 0.95)
    a64, r64 = R.gae_per_env64(r, v, d, lv, 0.99, 0.95)
    assert np.abs(adv.numpy() - a64).max() < 1e-12 and np.abs(ret.numpy() - r64).max() < 1e-12


# ------------------------------------------------------------------------- section 3's inputs (CPU)
GRAD_MS = (1, 2, 63, 65, 129, 1000)
GRAD_CASES = [(M, norm) for M in GRAD_MS for norm in (True, False)]
C_VF = 0.25


@functools.lru_cache(maxsize=None)
def _obs_rows():
    """tests/test_gpu_eval.py's obs_pool recipe on the CPU env batch: 1000 rows of a short random-action
    corridor rollout, then 1000 rows of 3 * randn."""
    from drone2d_amd.config import ENV_TEST_CONFIG
    from oracle_backend import OracleVecBackend

    be = OracleVecBackend(250, seed=2, **dict(ENV_TEST_CONFIG, scenario="corridor"))
    g = torch.Generator().manual_seed(3)
    obs = be.reset(seed=2)
    real = []
    for t in range(40):
        obs = be.step(torch.rand(250, 2, generator=g) * 2 - 1)[0]
        if t % 10 == 9:
            real.append(obs.clone())
    be.close()
    wide = 3.0 * torch.randn(1000, 27, generator=torch.Generator().manual_seed(4))
    return torch.cat(real + [wide]).float()


@functools.lru_cache(maxsize=None)
def _grad_problem(kind):
    """(policy, float32 data (obs, act, old logp, adv, ret, old values), {M: index list}) of section 3.
    The M = 1000 minibatch mixes real and wide rows and starts with the 32 special rows: 16 with
    log_ratio = +-20 and advantages +-1.5, 16 whose advantage is the minibatch mean (normalises to a
    tiny |a|); the smaller minibatches come from the other 1000 rows."""
    from drone2d_amd.ppo import ActorCritic

    torch.manual_seed(5)
    if kind == "shipped":
        pol = ActorCritic.from_agent_npz(AGENT)
        scale = ((pol.mlp_extractor.value_net, 3.0),)
    else:
        pol = ActorCritic()
        scale = ((pol.mlp_extractor.policy_net, 4.0), (pol.mlp_extractor.value_net, 4.0))
    with torch.no_grad():
        for net, s in scale:
            net[0].weight.mul_(s)
            net[2].weight.mul_(s)
        pol.log_std.copy_(torch.tensor([-2.5, 0.7]))
        pol.value_net.bias.fill_(0.5)
    X = _obs_rows()
    n = X.shape[0]
    g = torch.Generator().manual_seed(6)
    p64 = R.policy64(pol)
    with torch.no_grad():
        mean, V = p64(X.double())
        A = (mean + p64.log_std.exp() * torch.randn(n, 2, generator=g, dtype=torch.float64)).float()
        logp = p64.log_prob(mean, A.double())
        OL = (logp + torch.randn(n, generator=g, dtype=torch.float64)).float()
        ADV = torch.randn(n, generator=g)
        RET = torch.randn(n, generator=g) * 3
        d = torch.tensor([-2.0, -0.5, 0.0, 0.5, 2.0, -1.3, 0.9, 1.1])[torch.arange(n) % 8] * C_VF
        OV = (V - d + torch.randn(n, generator=g, dtype=torch.float64) * 0.01).float()
    perm = torch.cat([torch.randperm(1000, generator=g)[:500], 1000 + torch.randperm(1000, generator=g)[:500]])
    big = perm[torch.randperm(1000, generator=g)]
    rest = torch.tensor(sorted(set(range(n)) - set(big.tolist())))
    rest = rest[torch.randperm(len(rest), generator=g)]
    sp = big[:16]
    sign_lr = torch.tensor([1.0, 1.0, -1.0, -1.0]).repeat(4)
    sign_a = torch.tensor([1.0, -1.0, 1.0, -1.0]).repeat(4)
    OL[sp] = (logp[sp] - 20.0 * sign_lr.double()).float()
    ADV[sp] = 1.5 * sign_a
    others = torch.cat([big[:16], big[32:]])
    ADV[big[16:32]] = ADV[others].double().mean().float()
    idx = {M: (big if M == 1000 else rest[:M]).clone() for M in GRAD_MS}
    return pol, (X, A, OL, ADV, RET, OV), idx


def _grad_cfg(norm, ctl):
    from drone2d_amd.ppo import PPOConfig

    return PPOConfig(normalize_advantage=norm, clip_range_vf=C_VF if ctl else None)


@functools.lru_cache(maxsize=None)
def _grad_reference(kind, M, norm, ctl):
    """(float64 gradients, float64 statistics, ManualStep-on-CPU's errors against them: the floor)."""
    pol, data, idx = _grad_problem(kind)
    cfg = _grad_cfg(norm, ctl)
    p64 = R.policy64(pol)
    g64, s64 = R.grads64(p64, tuple(t.double() for t in data), idx[M], cfg, cfg.clip_range, C_VF if ctl else None, norm)
    return g64, s64, _grad_run(kind, M, norm, ctl, "cpu", None, g64, s64)


def _floor_spread(kind, M, norm, ctl=False):
    """Information only, never a bound: the restatement's error per buffer over N_ORDERS orders of the
    same minibatch (the given one and fixed shuffles of it), as {buffer: largest / order-0 error}.  The
    restatement's rounding depends on the order of its sums (and on the host's BLAS), most on sums with
    cancellation: a bias gradient, the policy loss of normalised advantages."""
    g64, s64, floor = _grad_reference(kind, M, norm, ctl)
    runs = [_grad_run(kind, M, norm, ctl, "cpu", None, g64, s64, order) for order in range(1, N_ORDERS)]
    return {k: max([floor[k]] + [r[k] for r in runs]) / floor[k] for k in floor if floor[k] > 0}


N_ORDERS = 6


def _reorder(ix, order):
    """Order 0 is ``ix`` itself, order k > 0 a fixed shuffle of it."""
    if order == 0:
        return ix
    return ix[torch.randperm(len(ix), generator=torch.Generator().manual_seed(order))]


def _grad_run(kind, M, norm, ctl, device, variant, g64, s64, order=0):
    """One ``ManualStep.grad`` on ``device`` (variant: None = CPU restatement, a GRAD_MUTANTS name, or
    'fused' / 'ctl' / 'separate' on the GPU); its errors against the float64 reference."""
    pol, data, idx = _grad_problem(kind)
    cfg = _grad_cfg(norm, ctl)
    man = R.clone_policy(pol, device)
    names = [k for k, _ in man.named_parameters()]
    if device == "cpu":
        step = R.mutant_step(man, cfg, variant)
    else:
        from drone2d_amd.ppo import ManualStep

        step = ManualStep(man, cfg, device)
        assert step.lib is not None and step.fused and (step.ctl is not None) == ctl
        step.fused = variant != "separate"
    rollout = tuple(t.to(device) for t in (data if ctl else data[:5]))
    acc = step.ctl.acc() if ctl else R.new_acc(device)
    with torch.no_grad():
        if ctl:
            step.reset_control()
        step.grad(_reorder(idx[M], order).to(device), rollout, acc)
    if device != "cpu":
        torch.cuda.synchronize()
    kl = None
    if ctl:
        rec = step.ctl.read()
        assert rec["n_minibatches"] == 1 and rec["early_stop"] == 0
        kl = rec["approx_kl"]
    return R.grad_errors(step, man, names, g64, s64, acc, kl)


@pytest.mark.parametrize("kind", ["shipped", "fresh"])
def test_gradient_inputs_saturate_and_clip(kind):
    """Section 3's conditions on the float64 reference: between 10 % and 90 % of the hidden activations
    of the M = 1000 minibatch have |h| > 0.999, the clip fraction is inside (0.05, 0.95), the 16 extreme
    rows have ratios e^+-20 with both advantage signs and finite gradients, and 16 rows normalise to a
    tiny advantage."""
    pol, data, idx = _grad_problem(kind)
    p64 = R.policy64(pol)
    X, A, OL, ADV, RET, OV = (t.double() for t in data)
    big = idx[1000]
    with torch.no_grad():
        hs = []
        for net in (p64.mlp_extractor.policy_net, p64.mlp_extractor.value_net):
            h1 = net[1](net[0](X[big]))
            hs += [h1, net[3](net[2](h1))]
        frac = float((torch.cat(hs).abs() > 0.999).double().mean())
        per = [float((h.abs() > 0.999).double().mean()) for h in hs]
        mean, _ = p64(X[big])
        lr = p64.log_prob(mean, A[big]) - OL[big]
        a = (ADV[big] - ADV[big].mean()) / (ADV[big].std() + 1e-8)
    print(f"{kind}: saturated fraction {frac:.3f} (h1p, h2p, h1v, h2v: {per})")
    assert 0.10 < frac < 0.90, frac
    g64, s64, _ = _grad_reference(kind, 1000, True, False)
    print(f"{kind}: clip_fraction {s64['clip_fraction']:.3f}")
    assert 0.05 < s64["clip_fraction"] < 0.95
    assert all(bool(torch.isfinite(g).all()) for g in g64)
    assert torch.allclose(lr[:16].abs(), torch.full((16,), 20.0, dtype=torch.float64), atol=1e-5)
    assert sorted({(int(torch.sign(x)), int(torch.sign(y))) for x, y in zip(lr[:16], a[:16])}) == \
        [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    assert float(a[16:32].abs().max()) < 1e-6 < float(a[32:].abs().median())
    assert sorted(set(idx[1].tolist()) & set(big.tolist())) == []


@pytest.mark.parametrize("ctl", [False, True], ids=["default", "ctl"])
def test_mutant_head_without_a_mutation_is_manual_step(ctl):
    """ppo_ref.mutant_step's written-out loss head with no error switched on gives ManualStep's bits:
    every gradient, statistic and (control path) the KL, normalised and raw, M = 1 included."""
    pol, data, idx = _grad_problem("shipped")
    for M, norm in ((1, True), (65, True), (65, False), (1000, True)):
        cfg = _grad_cfg(norm, ctl)
        out = []
        for variant in (None, R.HEAD_COPY):
            man = R.clone_policy(pol)
            step = R.mutant_step(man, cfg, variant)
            acc = step.ctl.acc() if ctl else R.new_acc()
            with torch.no_grad():
                if ctl:
                    step.reset_control()
                step.grad(idx[M], data if ctl else data[:5], acc)
            out.append((step.G.clone(), {k: v.clone() for k, v in acc.items()},
                        step.ctl.buf.clone() if ctl else None))
        (ga, aa, ca), (gb, ab, cb) = out
        assert torch.equal(ga, gb), (M, norm)
        assert all(torch.equal(aa[k], ab[k]) for k in aa), (M, norm)
        assert not ctl or torch.equal(ca, cb)


@pytest.mark.parametrize("kind", ["shipped", "fresh"])
def test_gradient_mutants_fail_the_bound(kind):
    """Each mutant of the float32 restatement (ManualStep on CPU tensors with one error switched on),
    through section 3's comparison on section 3's inputs, exceeds the bound by at least 10 x on some
    buffer of some case (M, normalize); the unmutated restatement is the bound's own calibrator.

    Measured (worst error / bound over the cases, shipped / fresh): s1_lt_s2 2.6e4 / 2.2e5 (at the small
    minibatches: with the e^20 rows in, the M = 1000 policy gradient is theirs), clip_on_ratio 2.1e5 /
    2.1e5, one_minus_h 8.8e6 / 1.1e7, no_ent_coef 5.5e3 / 2.2e5, biased_std 1.5e5 / 4.3e5.  ManualStep's own
    error (the floor) per gradient tensor: 1.0e-8 .. 3.5e-5 / 1.4e-8 .. 1.5e-6.  Printed as information
    only: over six orders of the same minibatch the floor of a sum with cancellation (the policy loss
    at M = 129) varies 14- to 18-fold."""
    floors = []
    for M, norm in GRAD_CASES:
        floors.append(_grad_reference(kind, M, norm, False)[2])
    vals = [v for f in floors for k, v in f.items() if k not in R.STATS]
    print(f"{kind}: float32 floor per gradient tensor {min(vals):.3g} .. {max(vals):.3g}")
    spread = max((r, k, c) for c in GRAD_CASES if c[0] > 2 for k, r in _floor_spread(kind, *c).items())
    print(f"{kind}: (information) the floor over {N_ORDERS} orders of a minibatch, largest / given order: "
          f"{spread[0]:.3g} ({spread[1]} at {spread[2]})")
    for mut in R.GRAD_MUTANTS:
        worst, where = 0.0, None
        for (M, norm), floor in zip(GRAD_CASES, floors):
            g64, s64, _ = _grad_reference(kind, M, norm, False)
            err = _grad_run(kind, M, norm, False, "cpu", mut, g64, s64)
            for k, e in err.items():
                r = e / R.bound(floor[k])
                if r > worst:
                    worst, where = r, (M, norm, k)
        print(f"{kind} gradient mutant {mut}: worst error / bound {worst:.3g} at {where}")
        assert worst >= 10.0, (mut, worst, where)


# ======================================================================= 1. d2d_ppo_adam / _adam_ctl
ADAM_NS = (1, 63, 64, 65, 1023, 1024, 1025, 12101, 16384)


def _dev_adam(lib, st, lr, cb=None):
    n = st.P.numel()
    args = (n, st.P.data_ptr(), st.G.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), st.t.data_ptr())
    if cb is None:
        return lib.d2d_ppo_adam(*args, lr, R.BETA1, R.BETA2, R.ADAM_EPS, MAX_NORM, _stream())
    return lib.d2d_ppo_adam_ctl(*args, R.BETA1, R.BETA2, R.ADAM_EPS, MAX_NORM, cb.ptr(), _stream())


@pytest.mark.gpu
@pytest.mark.parametrize("n", ADAM_NS)
def test_adam_kernels_match_float64_over_carried_steps(d2, n):
    """d2d_ppo_adam over 20 carried steps of the clip-straddling gradient schedule, at lr 0.05 and 3e-4,
    from t0 = 0 and from preloaded states at t0 = 3000 and 200000 (both corrections exactly 1): after
    every step delta p, m1, m2 and the gradient clipped in place are within 8 x ManualStep-on-CPU's
    error of torch.optim.Adam in float64, and *t is exactly t0 + k.  d2d_ppo_adam_ctl with lr in the
    block and kl_limit = +inf gives the same bits and leaves stop at 0.

    Measured on an MI355X (worst over t0 and the steps, float32 floor / device): n = 12101, lr 0.05:
    delta p 9.8e-6 / 9.8e-6, m1 6.7e-7 / 8.8e-8, m2 1.4e-6 / 2.8e-7, clipped gradient 7.4e-7 / 2.7e-8; at lr
    3e-4 delta p 3.7e-4 / 3.7e-4 (the rounding of p itself).  Worst device / max(floor, eps) over every n:
    2.75 (n = 1, delta p).  Before the kernel took torch's float(1 - beta) as the moments' weight
    (it used 1 - float(beta)), m2 was 1.29e-5 off at every n and step: 10 to 100 x the bound."""
    from drone2d_amd.ppo import ControlBlock, ppo_native

    lib = ppo_native()
    worst, bad = {}, []
    for lr in (0.05, 3e-4):
        for t0 in (0, 3000, 200000):
            p, m, v = R.adam_warm_state(n, t0, seed=n)
            cpu, ref = R.adam_state(p, m, v, t0), R.Adam64(p, lr, MAX_NORM, t0, m, v)
            dev, dev_c = R.adam_state(p, m, v, t0, "cuda"), R.adam_state(p, m, v, t0, "cuda")
            cb = ControlBlock("cuda")
            cb.set(lr, 0.2, -1.0, INF)
            for k, g in enumerate(R.adam_gradients(n, 20, MAX_NORM, seed=n)):
                before = {"cpu": cpu.P.double().clone(), "dev": dev.P.double().cpu()}
                for st in (cpu, dev, dev_c):
                    st.G.copy_(g)
                R.manual_apply(cpu, lr, MAX_NORM)
                assert _dev_adam(lib, dev, lr) == 0 and _dev_adam(lib, dev_c, lr, cb) == 0
                torch.cuda.synchronize()
                dp, gc = ref.step(g)
                for key, got_d, got_c, want in (("dp", dev.P.double().cpu() - before["dev"],
                                                 cpu.P.double() - before["cpu"], dp), ("m1", dev.m, cpu.m, ref.m),
                                                ("m2", dev.v, cpu.v, ref.v), ("g", dev.G, cpu.G, gc)):
                    e_dev, e_cpu = R.rel_l2(got_d, want), R.rel_l2(got_c, want)
                    w = worst.setdefault((lr, key), [0.0, 0.0, 0.0])
                    w[0], w[1], w[2] = max(w[0], e_cpu), max(w[1], e_dev), max(w[2], e_dev / R.bound(e_cpu) * R.FACTOR)
                    if not e_dev <= R.bound(e_cpu):
                        bad.append((lr, t0, k, key, e_dev, e_cpu))
                assert float(dev.t) == t0 + k + 1 == ref.t
                for a, b in ((dev.P, dev_c.P), (dev.m, dev_c.m), (dev.v, dev_c.v), (dev.G, dev_c.G), (dev.t, dev_c.t)):
                    assert torch.equal(a, b), (n, lr, t0, k)
            assert int(cb.ibuf[ControlBlock.STOP]) == 0
    for (lr, key), (e_cpu, e_dev, ratio) in worst.items():
        print(f"adam n={n} lr={lr} {key}: float32 floor {e_cpu:.3g}, device {e_dev:.3g}, "
              f"worst device / max(floor, eps) {ratio:.3g}")
    assert not bad, (n, len(bad), bad[:4])


@pytest.mark.gpu
def test_adam_exact_properties(d2):
    """lr = 0 leaves p bit for bit while m1, m2 and t advance; n = 16385 is refused with
    hipErrorInvalidValue and touches nothing (both entry points); n = 0 returns 0; a NULL control block
    is refused."""
    from drone2d_amd.ppo import ControlBlock, ppo_native

    lib = ppo_native()
    cb = ControlBlock("cuda")
    cb.set(0.0, 0.2, -1.0, INF)
    n = 12101
    p, m, v = R.adam_warm_state(n, 3000)
    g = R.adam_gradients(n, 1, MAX_NORM)[0]
    for use_cb in (None, cb):
        st = R.adam_state(p, m, v, 3000, "cuda")
        st.G.copy_(g)
        assert _dev_adam(lib, st, 0.0, use_cb) == 0
        torch.cuda.synchronize()
        assert torch.equal(st.P.cpu(), p) and float(st.t) == 3001.0
        assert not torch.equal(st.m.cpu(), m) and not torch.equal(st.v.cpu(), v)
        ref = R.Adam64(p, 0.0, MAX_NORM, 3000, m, v)
        ref.step(g)
        assert R.rel_l2(st.m, ref.m) < 4 * R.EPS32 and R.rel_l2(st.v, ref.v) < 4 * R.EPS32
    n = 16385
    p, m, v = R.adam_warm_state(n, 3000)
    for use_cb in (None, cb):
        st = R.adam_state(p, m, v, 3000, "cuda")
        st.G.copy_(torch.ones(n))
        assert _dev_adam(lib, st, 0.05, use_cb) == HIP_INVALID
        torch.cuda.synchronize()
        assert torch.equal(st.P.cpu(), p) and torch.equal(st.m.cpu(), m) and torch.equal(st.v.cpu(), v)
        assert torch.equal(st.G.cpu(), torch.ones(n)) and float(st.t) == 3000.0
    st = R.adam_state(p, m, v, 3000, "cuda")
    assert lib.d2d_ppo_adam(0, st.P.data_ptr(), st.G.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), st.t.data_ptr(),
                            0.05, R.BETA1, R.BETA2, R.ADAM_EPS, MAX_NORM, _stream()) == 0
    assert lib.d2d_ppo_adam_ctl(64, st.P.data_ptr(), st.G.data_ptr(), st.m.data_ptr(), st.v.data_ptr(),
                                st.t.data_ptr(), R.BETA1, R.BETA2, R.ADAM_EPS, MAX_NORM, None, _stream()) == HIP_INVALID
    torch.cuda.synchronize()
    assert torch.equal(st.P.cpu(), p) and float(st.t) == 3000.0
    assert int(cb.ibuf[ControlBlock.STOP]) == 0


# =================================================================================== 2. ftanh
# Measured on an MI355X over the 262 144 points of the test below: 3.146 ulp.  The assertion is twice
# the measured maximum, rounded up to a power of two.
FTANH_ULP_BOUND = 8.0


@pytest.mark.gpu
def test_ftanh_point_by_point(d2):
    """d2d_ppo_mlp_forward's h1 with W1[j][0] = +-2^(j % 8 - 4) (policy net +, value net -), every other
    W1 entry and b1 zero and observation rows (v_i, 0, ...): the pre-activation is v_i 2^(j % 8 - 4)
    exactly, so h1 holds ftanh at 4096 x 64 points -- a log sweep 1e-30 .. 1e4 of both signs, +-0, a
    subnormal, 0.25 and its float neighbours at every scale, 1000 points in [0.2, 0.3], 1000 in [-9, 9],
    +-1e30, +-inf -- against torch.tanh in float64.  Exact: odd symmetry bit for bit (rows i and
    i + 2048; the value net's h1 is the policy net's negated), |y| <= 1, y = +-1 for |x| >= 1e4,
    ftanh(+-0) = +-0, no NaN.  Then h2 and the output layer of the same launch, layer by layer against
    float64 from the device's own input to that layer (more than a fifth of the h2 units sit at +-1).

    Measured on an MI355X: maximum 3.146 ulp (at x = 0.5210862, the exp2 / rcp branch); Taylor branch
    0.947 ulp; |x| in [0.2, 0.3] 2.587 ulp; 0.25 and its two neighbours at every scale 1.206 ulp; the
    subnormal input exact.  The assertion is 8 ulp = twice the maximum rounded up to a power of two;
    "a few ulp" in the kernel's comment holds.  Output layer: error at most 0.042 of the allowance."""
    from drone2d_amd.ppo import ActorCritic, ManualStep, PPOConfig, ppo_native

    lib = ppo_native()
    vpos = R.ftanh_points()
    v = torch.cat([vpos, -vpos])
    m = v.numel()
    assert m == 4096
    scale = 2.0 ** (torch.arange(64) % 8 - 4).double()
    g = torch.Generator().manual_seed(8)
    pol = ActorCritic()
    with torch.no_grad():
        for p in pol.parameters():
            p.zero_()
        pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
        pn[0].weight[:, 0] = scale.float()
        vn[0].weight[:, 0] = -scale.float()
        for net, head in ((pn, pol.action_net), (vn, pol.value_net)):
            net[2].weight.copy_(torch.randn(64, 64, generator=g) * 2.0)
            net[2].bias.copy_(torch.randn(64, generator=g) * 0.1)
            head.weight.copy_(torch.randn(head.weight.shape, generator=g))
            head.bias.copy_(torch.randn(head.bias.shape, generator=g))
    cpu = R.clone_policy(pol)
    man = ManualStep(pol.cuda(), PPOConfig(), "cuda")
    obs = torch.zeros(m, 27)
    obs[:, 0] = v
    obs = obs.cuda()
    idx = torch.arange(m, device="cuda")
    e = lambda *sh: torch.full(sh, float("nan"), device="cuda")  # noqa: E731
    bufs = [e(m, 64), e(m, 64), e(m, 2), e(m, 64), e(m, 64), e(m, 64), e(m, 64), e(m, 1), e(m, 64), e(m, 64)]
    bptr = (C.c_void_p * 10)(*[b.data_ptr() for b in bufs])
    assert lib.d2d_ppo_mlp_forward(m, idx.data_ptr(), obs.data_ptr(), man.weight_ptrs(), bptr, None, _stream()) == 0
    torch.cuda.synchronize()
    h1p, h2p, mean, _, _, h1v, h2v, val, _, _ = (b.cpu() for b in bufs)
    x = v.double()[:, None] * scale[None, :]
    assert torch.equal(x.float().double(), x)  # every pre-activation is a float32 value
    ref = torch.tanh(x)
    # the measured part
    ulps = ((h1p.double() - ref).abs() / torch.as_tensor(R.ulp32(ref.numpy()))).numpy()
    ax = x.abs().numpy()
    near = (ax >= 0.2) & (ax <= 0.3)
    exact_near = np.isin(ax.astype(np.float32), np.array([np.nextafter(np.float32(0.25), np.float32(0)),
                                                           np.float32(0.25),
                                                           np.nextafter(np.float32(0.25), np.float32(1))]))
    sub = (ax > 0) & (ax < 2.0 ** -126)
    assert int(exact_near.sum()) >= 2 * 3 * 8 and int(near.sum()) > 2000 and int(sub.sum()) > 0
    where = np.unravel_index(np.argmax(np.where(sub, 0.0, ulps)), ulps.shape)
    print(f"ftanh: max error {ulps[~sub].max():.3f} ulp at x = {x.numpy()[where]!r}; Taylor branch (|x| < 0.25) "
          f"{ulps[(ax < 0.25) & ~sub].max():.3f}, exp branch {ulps[ax >= 0.25].max():.3f}, |x| in [0.2, 0.3] "
          f"{ulps[near].max():.3f}, at 0.25 and its neighbours {ulps[exact_near].max():.3f}, subnormal inputs "
          f"{ulps[sub].max():.3f}")
    # exact properties
    assert not bool(torch.isnan(h1p).any()) and not bool(torch.isnan(h1v).any())
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    # (a zero input row reaches ftanh as +0 whatever its sign: the accumulator starts at +0 and
    # +0 + -0 = +0, so ftanh(-0) cannot be reached through the forward; both zero rows must give +0)
    zero = x == 0.0
    nz = ~zero[:2048]
    assert torch.equal(bits(h1p[2048:][nz]), bits((-h1p[:2048])[nz]))
    assert torch.equal(bits(h1v[~zero]), bits((-h1p)[~zero]))
    assert int(zero.sum()) == 128 and torch.equal(bits(h1p[zero]), torch.zeros(128, dtype=torch.int32))
    assert torch.equal(bits(h1v[zero]), torch.zeros(128, dtype=torch.int32))
    assert float(h1p.abs().max()) <= 1.0
    big = x.abs() >= 1e4
    assert int(big.sum()) > 500 and torch.equal(h1p[big].double(), torch.sign(x[big]))
    assert ulps[~sub].max() <= FTANH_ULP_BOUND
    assert ulps[sub].max() <= FTANH_ULP_BOUND
    # h2 and the outputs, layer by layer: a 64-term float32 dot product plus bias in any order is within
    # 65 u sum |w h| of the exact one (u = eps / 2)
    u = R.EPS32 / 2
    n_sat = 0
    for net, head, h1, h2, out in ((cpu.mlp_extractor.policy_net, cpu.action_net, h1p, h2p, mean),
                                   (cpu.mlp_extractor.value_net, cpu.value_net, h1v, h2v, val)):
        W2, b2, W3, b3 = (t.detach().double() for t in (net[2].weight, net[2].bias, head.weight, head.bias))
        pre = h1.double() @ W2.t() + b2
        slack = 65 * u * (h1.double().abs() @ W2.abs().t() + b2.abs())
        want = torch.tanh(pre)
        tol = FTANH_ULP_BOUND * torch.as_tensor(R.ulp32(want.numpy())) + (1 - want * want + 2 * slack) * slack
        assert bool(((h2.double() - want).abs() <= tol).all())
        n_sat += int((h2.abs() == 1.0).sum())
        want = h2.double() @ W3.t() + b3
        tol = 65 * u * (h2.double().abs() @ W3.abs().t() + b3.abs())
        err = (out.double() - want).abs()
        print(f"output layer: max |out - float64| {float(err.max()):.3g}, max error / allowance "
              f"{float((err / tol).max()):.3g}")
        assert bool((err <= tol).all())
    assert n_sat > 0.2 * 2 * m * 64  # h2 units at exactly +-1


# ======================================================================= 3. the minibatch gradient
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["fused", "ctl", "separate"])
@pytest.mark.parametrize("kind", ["shipped", "fresh"])
def test_gradient_matches_float64_autograd(d2, kind, variant):
    """ManualStep.grad on the device -- the fused launch, the fused control variant with clip_range_vf =
    0.25, the separate kernels -- on saturated policies (the shipped agent with its value net's hidden
    weights x 3; a fresh init with all hidden weights x 4), real and 3 * randn observations, log_std =
    (-2.5, 0.7), old log-probs off by randn, 16 rows at ratios e^+-20 and 16 at a normalised advantage of
    about 0; M in {1, 2, 63, 65, 129, 1000}, advantages normalised and raw (M = 1: never normalised, as
    SB3): every parameter's gradient and every statistic within 8 x ManualStep-on-CPU's error of float64
    autograd.

    Measured on an MI355X (worst device error / max(floor, eps), where 8 is allowed): fresh policy 3.4
    (fused; value_loss at M = 1: 4.1e-7 against 5.2e-8), 1.7 (ctl), 7.3 (separate; the same, 8.7e-7);
    shipped policy 7.8 (fused, ctl: action_net.bias at M = 63, normalised, 4.9e-6 against a floor of
    6.3e-7) and 7.7 (separate: the same tensor at M = 1000, raw, 5.0e-6 against 6.5e-7).  That tensor --
    two numbers, a sum over the samples with cancellation, at sigma = e^-2.5 carried by a few samples --
    is what this test found: with the action mean a float32 sum and the log-density in float32 the
    kernels gave 1.25e-5 (fused) and 7.9e-6 (separate) for it, 20 x and 12 x the floor.  The forward's h1
    and h2 were as close to float64 as the CPU's (9e-8 and 1.3e-7 both), but the mean was 1.5e-7 off
    against the CPU's 8.9e-8, and the float64 loss head on that mean alone already gave 7.7e-6.  The
    gradient kernels now take the mean as a double sum over h2 and z, the log-density and the normalised
    advantage in double.  The margin that is left is small, and the floor is one evaluation of the
    restatement: it depends on the host's BLAS."""
    ctl = variant == "ctl"
    worst, fails = (0.0, None), []
    for M, norm in GRAD_CASES:
        g64, s64, floor = _grad_reference(kind, M, norm, ctl)
        err = _grad_run(kind, M, norm, ctl, "cuda", variant, g64, s64)
        bad = {k: (e, floor[k]) for k, e in err.items() if not e <= R.bound(floor[k])}
        r, k = max((e / R.bound(floor[k]) * R.FACTOR, k) for k, e in err.items())
        if r > worst[0]:
            worst = (r, (M, norm, k, err[k], floor[k]))
        gk = [k for k in err if k not in R.STATS and k != "approx_kl"]
        print(f"grad {kind} {variant} M={M} normalize={norm}: floor {max(floor[k] for k in gk):.3g}, device "
              f"{max(err[k] for k in gk):.3g}, worst device / max(floor, eps) {r:.3g} ({k})")
        if bad:
            fails.append((M, norm, bad))
    print(f"grad {kind} {variant}: worst ratio {worst}")
    assert not fails, (kind, variant, fails)


# ============================================================================ 4. a whole PPO.train()
def _train_against_float64(d2, bs, graph, **over):
    from drone2d_amd.ppo import PPO, ActorCritic, ManualStep, PPOConfig

    n_envs, T, E = 256, 8, 2
    M = n_envs * T
    venv = d2.Drone2dVecEnv(n_envs, seed=1, **_kw(scenario="corridor"))
    cfg = PPOConfig(n_steps=T, batch_size=bs, n_epochs=E, graph=graph, **over)
    algo = PPO(venv, cfg, seed=0)
    assert algo._hip and algo.manual.fused and algo.use_graph == graph
    if graph:  # the first update runs eagerly; the second is captured and replayed
        algo.collect_rollouts()
        algo.train()
    algo.collect_rollouts()
    torch.cuda.synchronize()
    man = algo.manual
    P0, m0, v0, t0 = man.P.cpu().clone(), man.m.cpu().clone(), man.v.cpu().clone(), float(man.t)
    data = tuple(t.cpu().clone() for t in algo._rollout_data())
    rec = algo.train()
    torch.cuda.synchronize()
    assert (algo._graph is not None) == graph
    perm = algo._perm.cpu().clone()
    P1, m1, v1, t1 = man.P.cpu().clone(), man.m.cpu().clone(), man.v.cpu().clone(), float(man.t)
    venv.close()
    mbs = [perm[e * M + s:e * M + min(s + bs, M)] for e in range(E) for s in range(0, M, bs)]
    for e in range(E):
        assert torch.equal(torch.sort(perm[e * M:(e + 1) * M]).values, torch.arange(M))
    n_mb = len(mbs)
    assert t0 == (n_mb if graph else 0) and t1 == t0 + n_mb
    # float64: SB3's loop from the snapshot
    lr, clip, clip_vf, _ = cfg.coefs(1.0)
    p64 = ActorCritic().double()
    sizes = [p.numel() for p in p64.parameters()]
    with torch.no_grad():
        for p, x in zip(p64.parameters(), torch.split(P0.double(), sizes)):
            p.copy_(x.view_as(p))
    stats, (P64, m64, v64, t64) = R.train64(p64, tuple(t.double() for t in data), mbs, cfg, lr, clip,
                                            clip_vf if clip_vf >= 0 else None, True, m0, v0, t0)
    assert t64 == t1
    # the float32 restatement: ManualStep on CPU tensors from the same snapshot, the same index lists
    # (and, as information only, its errors over other orders of each minibatch's samples)
    keys = R.STATS + (("approx_kl",) if cfg.control else ())
    want = {k: sum(s[k] for s in stats) / n_mb for k in keys}
    refs = dict({"dP": P64 - P0.double(), "m": m64, "v": v64}, **want)
    floor, spread = None, dict.fromkeys(refs, 0.0)
    for order in range(N_ORDERS):
        cpu = ManualStep(ActorCritic(), cfg, "cpu")
        for dst, src in ((cpu.P, P0), (cpu.m, m0), (cpu.v, v0), (cpu.t, torch.tensor(t0))):
            dst.copy_(src)
        acc = cpu.ctl.acc() if cpu.ctl is not None else R.new_acc()
        with torch.no_grad():
            if cpu.ctl is not None:
                cpu.reset_control()
            for idx in mbs:
                cpu.step(_reorder(idx, order), data, acc)
        assert float(cpu.t) == t1
        rec32 = cpu.ctl.read() if cpu.ctl is not None else {k: float(a) / n_mb for k, a in acc.items()}
        got = dict({"dP": cpu.P.double() - P0.double(), "m": cpu.m, "v": cpu.v}, **{k: rec32[k] for k in keys})
        errs = {k: R.rel_l2(got[k], refs[k]) for k in refs}
        floor = errs if order == 0 else floor
        spread = {k: max(spread[k], errs[k]) for k in refs}
    dev = dict({"dP": P1.double() - P0.double(), "m": m1, "v": v1}, **{k: rec[k] for k in keys})
    bad = {}
    for k in refs:
        e_dev, e_cpu = R.rel_l2(dev[k], refs[k]), floor[k]
        print(f"train bs={bs} graph={graph} {k}: float32 floor {e_cpu:.3g}, device {e_dev:.3g}, device / "
              f"max(floor, eps) {e_dev / R.bound(e_cpu) * R.FACTOR:.3g}  (floor over {N_ORDERS} orders up to "
              f"{spread[k]:.3g})")
        if not e_dev <= R.bound(e_cpu):
            bad[k] = (e_dev, e_cpu)
    if cfg.control:
        assert rec["n_minibatches"] == n_mb and rec["early_stop"] == 0
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("bs", [512, 768, 500])
def test_train_matches_float64(d2, bs, graph):
    """One whole PPO.train() on a 256-env x 8-step rollout (2048 samples, 2 epochs), eager and as the
    captured and replayed graph, replayed from a snapshot through SB3's loop in float64 and through
    ManualStep on the CPU over the minibatch index lists read back from the device: P - P_before, m, v
    and the four statistics means within 8 x the CPU restatement's error, t advanced by exactly the
    number of minibatches.  bs = 512: the up-front advantage statistics sliced per minibatch; 768:
    minibatches of 768, 768, 512, so the ragged slice and the next epoch's offset; 500: no multiple of
    64, so each minibatch computes its own statistics.

    Measured on an MI355X (float32 floor / device, over the six runs): P - P_before 9.9e-6 .. 1.2e-5 /
    the same to three digits; m 2.2e-7 .. 5.8e-7 / 2.1e-7 .. 5.8e-7; v 2.2e-7 .. 5.1e-7 / 1.7e-7 .. 5.2e-7;
    policy_loss 1.9e-6 .. 3.8e-5 / 2.6e-6 .. 1.2e-5; value_loss 1.1e-7 .. 3.0e-7 / 9.3e-8 .. 3.0e-7; worst
    device / max(floor, eps) 2.7 (policy_loss at bs = 500, eager: 5.0e-6 against 1.9e-6); on the control
    path approx_kl 2.6e-5 / 6.0e-5 (2.3 x).  Found by this test: v was 6.4e-6 .. 1.3e-5 off, 20 to 35 x
    the floor, until d2d_ppo_adam took torch's weight for the moments; and policy_loss at bs = 500 was
    2.1e-5 off, 11 x, while the kernels rounded the minibatch's advantage mean to float."""
    _train_against_float64(d2, bs, graph)


@pytest.mark.gpu
def test_control_train_matches_float64(d2):
    """The same on the control path (target_kl = inf, clip_range_vf = 0.25, captured): also approx_kl."""
    _train_against_float64(d2, 768, True, target_kl=INF, clip_range_vf=C_VF)


# ============================================================================= 5. the rollout's GAE
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 129])
@pytest.mark.parametrize("T", [1, 2, 33])
def test_rollout_gae_bitwise_and_against_float64(d2, T, n):
    """d2d_ppo_rollout_step driven for T + 1 launches with done patterns never / always / p = 0.2 and
    once with prev_info = NULL.  The value net has zero hidden biases and step T sees all-zero
    observations, so the bootstrap value is the output bias 0.5 in every precision: adv_buf and ret_buf
    equal compute_gae in float32 on the CPU bit for bit for every env (the kernel's stated property),
    and agree with the per-env float64 recursion at rtol 1e-5 / atol 2e-5; start0 is the last step's
    dones; the episode counts are right and, without info, the return sums exactly 0."""
    from drone2d_amd import abi
    from drone2d_amd.ppo import ActorCritic, D2DPPORollout, ManualStep, PPOConfig, compute_gae

    torch.manual_seed(0)
    pol = ActorCritic()
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([-0.4, 0.3]))
        pol.value_net.weight.mul_(3.0)
        pol.value_net.bias.fill_(0.5)
    pol = pol.cuda()
    man = ManualStep(pol, PPOConfig(), "cuda")
    cfg = PPOConfig()
    ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
    f = lambda *sh, dt=torch.float32: torch.full(sh, float("nan"), device="cuda").to(dt)  # noqa: E731
    for pattern, with_info in (("never", True), ("always", True), ("p=0.2", True), ("p=0.2", False)):
        g = torch.Generator().manual_seed(100 * T + n)
        obs = (torch.rand(T, n, 27, generator=g) * 2 - 1).cuda()
        noise = torch.randn(T, n, 2, generator=g).cuda()
        rews = torch.randn(T, n, generator=g).cuda()
        p_done = {"never": 0.0, "always": 1.0, "p=0.2": 0.2}[pattern]
        terms = (torch.rand(T, n, generator=g) < p_done * 0.8).cuda()
        truncs = (torch.rand(T, n, generator=g) < p_done).cuda() if pattern != "p=0.2" else \
            (torch.rand(T, n, generator=g) < 0.05).cuda()
        info = torch.randn(T, n, abi.INFO_DIM, generator=g).cuda()
        obs_buf, act_buf, logp_buf, val_buf, rew_buf = f(T, n, 27), f(T, n, 2), f(T, n), f(T, n), f(T, n)
        adv_buf, ret_buf, act_env = f(T, n), f(T, n), f(n, 2)
        done_buf = torch.zeros(T, n, dtype=torch.bool, device="cuda")
        start0 = torch.ones(n, dtype=torch.bool, device="cuda")
        stats = torch.full((T, (n + 63) // 64, 2), float("nan"), dtype=torch.float64, device="cuda")
        r = D2DPPORollout(n=n, T=T, info_dim=abi.INFO_DIM, info_totrew=abi.INFO_TOTREW, gamma=cfg.gamma,
                          gae_lambda_gamma=cfg.gamma * cfg.gae_lambda, log_std=ptr(pol.log_std), obs_buf=ptr(obs_buf),
                          act_buf=ptr(act_buf), logp_buf=ptr(logp_buf), val_buf=ptr(val_buf), rew_buf=ptr(rew_buf),
                          done_buf=ptr(done_buf), start0=ptr(start0), act_env=ptr(act_env), adv_buf=ptr(adv_buf),
                          ret_buf=ptr(ret_buf), stats=ptr(stats))
        zeros = torch.zeros(n, 27, device="cuda")
        for t in range(T + 1):
            r.t, r.obs, r.noise = t, ptr(obs[t] if t < T else zeros), ptr(noise[t]) if t < T else None
            if t > 0:
                r.prev_rew, r.prev_term, r.prev_trunc = ptr(rews[t - 1]), ptr(terms[t - 1]), ptr(truncs[t - 1])
                r.prev_info = ptr(info[t - 1]) if with_info else None
            assert man.lib.d2d_ppo_rollout_step(C.byref(r), man.weight_ptrs(), _stream()) == 0
        torch.cuda.synchronize()
        dones = (terms | truncs).cpu()
        assert {"never": not dones.any(), "always": dones.all(), "p=0.2": True}[pattern]
        assert torch.equal(rew_buf.cpu(), rews.cpu()) and torch.equal(done_buf.cpu(), dones)
        assert torch.equal(obs_buf.cpu(), obs.cpu()) and torch.equal(start0.cpu(), dones[T - 1])
        ep = stats.sum(1).cpu()
        assert torch.equal(ep[:, 0], dones.sum(1).double())
        if with_info:
            want = torch.where(dones, info.cpu()[..., abi.INFO_TOTREW].double(), 0.0).sum(1)
            torch.testing.assert_close(ep[:, 1], want, rtol=1e-12, atol=1e-9)
        else:
            assert torch.equal(stats[..., 1].cpu(), torch.zeros(T, (n + 63) // 64, dtype=torch.float64))
        # the values of steps 0 .. T-1 are the device's (checked against float64 below, loosely: the
        # forward has its own tests); the bootstrap value is exactly 0.5
        vals = val_buf.cpu()
        with torch.no_grad():
            v64 = R.policy64(pol)(obs.cpu().double())[1]
        torch.testing.assert_close(vals.double(), v64, rtol=1e-5, atol=2e-5)
        last_v = torch.full((n,), 0.5)
        starts = torch.cat([torch.ones(1, n, dtype=torch.bool), dones[:-1]])
        adv32, ret32 = compute_gae(rews.cpu(), vals, starts, last_v, dones[T - 1], cfg.gamma, cfg.gae_lambda)
        assert adv32.dtype == torch.float32
        assert torch.equal(adv_buf.cpu(), adv32) and torch.equal(ret_buf.cpu(), ret32), (pattern, with_info)
        a64, r64 = R.gae_per_env64(rews.cpu().numpy(), vals.numpy(), dones.numpy(), last_v.numpy(), cfg.gamma,
                                   cfg.gae_lambda)
        np.testing.assert_allclose(adv32.numpy(), a64, rtol=1e-5, atol=2e-5)  # the float32 recursion itself
        np.testing.assert_allclose(adv_buf.cpu().numpy(), a64, rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(ret_buf.cpu().numpy(), r64, rtol=1e-5, atol=2e-5)


# ================================================================================= 6. the shuffles
@pytest.mark.gpu
def test_permute_is_a_bijection_at_every_small_size(d2):
    """d2d_ppo_permute for every n in 1 .. 130 and 2^k - 1, 2^k, 2^k + 1 up to k = 12, two epochs each:
    every row is a bijection of [0, n) (odd and even bit splits of the Feistel network, bits 0 and 1)."""
    from drone2d_amd.ppo import ppo_native

    lib = ppo_native()
    ns = sorted(set(range(1, 131)) | {2 ** k + d for k in range(13) for d in (-1, 0, 1) if 2 ** k + d >= 1})
    assert 4097 in ns and 1 in ns and 2 in ns
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = []
    for n in ns:
        out = torch.full((2 * n,), -1, dtype=torch.int64, device="cuda")
        assert lib.d2d_ppo_permute(n, 2, 99, ctr.data_ptr(), out.data_ptr(), _stream()) == 0
        outs.append(out)
    torch.cuda.synchronize()
    assert int(ctr) == 2 * len(ns)
    for n, out in zip(ns, outs):
        rows = out.cpu().reshape(2, n)
        for e in range(2):
            assert torch.equal(torch.sort(rows[e]).values, torch.arange(n)), (n, e)
