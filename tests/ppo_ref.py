"""Float64 references, the error measure and the bound for the PPO library's tests
(tests/test_gpu_ppo_reference.py), and float32 mutants that show the bound can tell a wrong kernel
from a right one.

Test infrastructure: the references restate SB3 2.1 ``PPO.train`` (loss, ``clip_grad_norm_``,
``torch.optim.Adam(eps=1e-5)``) and ``RolloutBuffer.compute_returns_and_advantage`` in float64 with
autograd and torch's own optimiser; nothing here calls the HIP library.

Error measure: the relative L2 error of a buffer against its float64 reference (``rel_l2``); for
parameters it is taken on the per-step update ``p_after - p_before`` differenced in float64.  Bound:
eight times the same error of the project's float32 torch restatement (``ManualStep`` on CPU tensors,
same inputs), where an error below one float32 epsilon counts as one epsilon (``bound``): the factor is
there for differences of a few ulp (powf, sqrtf, division, summation order), so the allowance is never
less than a few ulp of the buffer, also when the restatement happens to round a buffer exactly."""
from __future__ import annotations

import math
import types

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
STATS = ("policy_loss", "value_loss", "entropy", "clip_fraction")
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-5
FACTOR = 8.0


def rel_l2(x, ref) -> float:
    """||x - ref|| / ||ref|| in float64 (0 / 0 = 0, d / 0 = inf); a NaN anywhere gives inf."""
    as64 = lambda a: (a.detach().cpu().double() if isinstance(a, torch.Tensor)  # noqa: E731
                      else torch.as_tensor(a, dtype=torch.float64)).reshape(-1)
    x, ref = as64(x), as64(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    d, n = float(torch.linalg.vector_norm(x - ref)), float(torch.linalg.vector_norm(ref))
    if not math.isfinite(d):
        return math.inf
    if n == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / n


def bound(floor_err: float) -> float:
    """The device's allowance given the float32 restatement's error on the same buffer."""
    return FACTOR * max(floor_err, EPS32)


# ------------------------------------------------------------------------------------------- Adam
class Adam64:
    """``clip_grad_norm_`` + ``torch.optim.Adam(eps=1e-5)`` on one float64 vector, from a preloaded
    state (``step``, ``exp_avg``, ``exp_avg_sq``)."""

    def __init__(self, p, lr, max_norm, step=0, exp_avg=None, exp_avg_sq=None):
        self.p = torch.nn.Parameter(torch.as_tensor(p).detach().cpu().double().clone())
        self.max_norm = max_norm
        self.opt = torch.optim.Adam([self.p], lr=lr, betas=(BETA1, BETA2), eps=ADAM_EPS)
        z = torch.zeros_like(self.p.data)
        self.opt.state[self.p] = {
            "step": torch.tensor(float(step)),
            "exp_avg": z.clone() if exp_avg is None else torch.as_tensor(exp_avg).detach().cpu().double().clone(),
            "exp_avg_sq": z.clone() if exp_avg_sq is None else torch.as_tensor(exp_avg_sq).detach().cpu().double().clone()}

    def step(self, g32):
        """One step on the float32 gradient values ``g32``; returns (delta p, clipped gradient)."""
        before = self.p.detach().clone()
        self.p.grad = torch.as_tensor(g32).detach().cpu().double().clone()
        torch.nn.utils.clip_grad_norm_([self.p], self.max_norm)
        self.opt.step()
        return self.p.detach() - before, self.p.grad.clone()

    @property
    def m(self):
        return self.opt.state[self.p]["exp_avg"]

    @property
    def v(self):
        return self.opt.state[self.p]["exp_avg_sq"]

    @property
    def t(self):
        return float(self.opt.state[self.p]["step"])


ADAM_MUTANTS = ("no_clamp", "t_off_by_one", "eps_in_sqrt", "bc2_no_sqrt", "eps_1e-8", "eps_over_bc2s")


def adam_state(p, m=None, v=None, t=0.0, device="cpu"):
    """The fields ``ManualStep.apply`` works on: flat float32 P, G, m, v and the step counter t."""
    p = torch.as_tensor(p, dtype=torch.float32).to(device).clone()
    z = torch.zeros_like(p)
    return types.SimpleNamespace(P=p, G=z.clone(), m=z.clone() if m is None else m.float().to(device).clone(),
                                 v=z.clone() if v is None else v.float().to(device).clone(),
                                 t=torch.tensor(float(t), device=device), ctl=None, lib=None)


def manual_apply(st, lr, max_norm):
    """``ManualStep.apply`` itself (the project's float32 torch restatement) on a bare state."""
    from drone2d_amd.ppo import ManualStep, PPOConfig

    st.cfg = PPOConfig(learning_rate=lr, max_grad_norm=max_norm)
    ManualStep.apply(st)


def adam32(st, lr, max_norm, mutant=None):
    """``ManualStep.apply``'s float32 torch ops written out again, with one error switched on by
    ``mutant``; ``mutant=None`` is bit-identical to ``manual_apply`` (asserted by the self-check)."""
    assert mutant is None or mutant in ADAM_MUTANTS, mutant
    b1, b2, eps = BETA1, BETA2, ADAM_EPS
    G = st.G
    coef = max_norm / (torch.linalg.vector_norm(G) + 1e-6)
    if mutant != "no_clamp":
        coef = torch.clamp(coef, max=1.0)
    G.mul_(coef)
    st.t.add_(1.0)
    st.m.lerp_(G, 1.0 - b1)
    st.v.mul_(b2).addcmul_(G, G, value=1.0 - b2)
    bc1 = 1.0 - torch.pow(b1, st.t + 1.0 if mutant == "t_off_by_one" else st.t)
    bc2 = 1.0 - torch.pow(b2, st.t)
    bc2s = bc2 if mutant == "bc2_no_sqrt" else torch.sqrt(bc2)
    if mutant == "eps_1e-8":
        eps = 1e-8
    if mutant == "eps_in_sqrt":
        den = torch.sqrt(st.v / (bc2s * bc2s) + eps)
    elif mutant == "eps_over_bc2s":
        den = (st.v.sqrt() + eps) / bc2s
    else:
        den = st.v.sqrt() / bc2s + eps
    st.P.sub_(st.m * (lr / bc1) / den)


def adam_gradients(n, steps, max_norm, seed=0):
    """The gradient schedule, cycling per step: norm >> max_norm, 0.999 max_norm, 1.001 max_norm,
    about 1e-9, the zero vector.  Element magnitudes spread over three decades, so that sqrt(v) of some
    elements is near Adam's eps.  Float32 tensors (their float32 norm is the target within 1e-7)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(steps):
        x = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** (-3.0 * torch.rand(n, generator=g,
                                                                                          dtype=torch.float64))
        target = (100.0 * max_norm, 0.999 * max_norm, 1.001 * max_norm, 1e-9, 0.0)[k % 5]
        out.append((x * (target / float(torch.linalg.vector_norm(x)))).float())
    return out


def adam_warm_state(n, t0, seed=0):
    """(p, m1, m2) float32: random parameters, random first moments, random non-negative second
    moments (zero moments at t0 = 0, as a fresh optimiser has them)."""
    g = torch.Generator().manual_seed(1000 + seed)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 3e-3
    v = (torch.randn(n, generator=g) * 3e-3) ** 2
    if t0 == 0:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, m, v


def adam_errors(stepper, n, t0, lr, max_norm, steps=20, seed=0):
    """Run ``stepper(st, g)`` (one in-place step of a float32 Adam on state ``st`` with gradient ``g``
    loaded into ``st.G``) for ``steps`` carried steps next to ``Adam64``; per step the relative L2
    errors of (delta p, m1, m2, clipped gradient) and whether t came back as exactly t0 + k."""
    p, m, v = adam_warm_state(n, t0, seed)
    st = adam_state(p, m, v, t0)
    ref = Adam64(p, lr, max_norm, t0, m, v)
    rows = []
    for k, g in enumerate(adam_gradients(n, steps, max_norm, seed)):
        before = st.P.double().clone()
        st.G.copy_(g)
        stepper(st, g)
        dp, gc = ref.step(g)
        rows.append({"dp": rel_l2(st.P.double() - before, dp), "m1": rel_l2(st.m, ref.m), "m2": rel_l2(st.v, ref.v),
                     "g": rel_l2(st.G, gc), "t_ok": float(st.t) == t0 + k + 1 == ref.t})
    return rows


# ------------------------------------------------------------------------------ loss and gradient
def policy64(pol):
    """A float64 copy of an ``ActorCritic``."""
    out = type(pol)().double()
    out.load_state_dict({k: v.detach().cpu().double() for k, v in pol.state_dict().items()})
    return out


def loss64(pol, data, idx, cfg, clip, clip_vf=None, normalize=True):
    """SB3 2.1 ``PPO.train``'s loss of minibatch ``idx`` in float64: (loss, statistics incl.
    approx_kl).  ``data`` = float64 (obs, actions, old log-probs, advantages, returns[, old values]);
    advantages are normalised when ``normalize`` and the minibatch has more than one sample."""
    X, A, OL, ADV, R = data[:5]
    values, logp, ent = pol.evaluate_actions(X[idx], A[idx])
    adv = ADV[idx]
    if normalize and len(idx) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    log_ratio = logp - OL[idx]
    ratio = torch.exp(log_ratio)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    if clip_vf is not None:
        ov = data[5][idx]
        values = ov + torch.clamp(values - ov, -clip_vf, clip_vf)
    vl = torch.nn.functional.mse_loss(R[idx], values)
    loss = pl + cfg.ent_coef * (-ent.mean()) + cfg.vf_coef * vl
    with torch.no_grad():
        stats = {"policy_loss": pl.item(), "value_loss": vl.item(), "entropy": ent.mean().item(),
                 "clip_fraction": ((ratio - 1).abs() > clip).double().mean().item(),
                 "approx_kl": ((ratio - 1) - log_ratio).mean().item()}
    return loss, stats


def grads64(pol, data, idx, cfg, clip, clip_vf=None, normalize=True):
    """Autograd's gradients of ``loss64`` per parameter (the order of ``pol.parameters()``)."""
    for p in pol.parameters():
        p.grad = None
    loss, stats = loss64(pol, data, idx, cfg, clip, clip_vf, normalize)
    loss.backward()
    return [p.grad.clone() for p in pol.parameters()], stats


def train64(pol, data, minibatches, cfg, lr, clip, clip_vf=None, normalize=True, m=None, v=None, t=0):
    """SB3's minibatch loop in float64 over the index lists ``minibatches`` from a preloaded optimiser
    state (flat ``m``, ``v`` in ``pol.parameters()`` order, step ``t``); returns the per-minibatch
    statistics and the flat (P, m, v, t) afterwards."""
    params = list(pol.parameters())
    opt = torch.optim.Adam(params, lr=lr, betas=(BETA1, BETA2), eps=ADAM_EPS)
    sizes = [p.numel() for p in params]
    n = sum(sizes)
    ms = torch.split(torch.zeros(n, dtype=torch.float64) if m is None else m.detach().cpu().double(), sizes)
    vs = torch.split(torch.zeros(n, dtype=torch.float64) if v is None else v.detach().cpu().double(), sizes)
    for p, a, b in zip(params, ms, vs):
        opt.state[p] = {"step": torch.tensor(float(t)), "exp_avg": a.clone().view_as(p),
                        "exp_avg_sq": b.clone().view_as(p)}
    out = []
    for idx in minibatches:
        opt.zero_grad()
        loss, stats = loss64(pol, data, idx, cfg, clip, clip_vf, normalize)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, cfg.max_grad_norm)
        opt.step()
        out.append(stats)
    flat = lambda xs: torch.cat([x.detach().reshape(-1) for x in xs])  # noqa: E731
    return out, (flat(params), flat([opt.state[p]["exp_avg"] for p in params]),
                 flat([opt.state[p]["exp_avg_sq"] for p in params]), float(opt.state[params[0]]["step"]))


HEAD_COPY = "head_copy"
GRAD_MUTANTS = ("s1_lt_s2", "clip_on_ratio", "one_minus_h", "no_ent_coef", "biased_std")


def mutant_step(policy, cfg, mutant=None):
    """``ManualStep`` on CPU tensors with one error switched on: the loss head (``_head_torch`` written
    out again) or the tanh derivative.  ``mutant=None`` is ``ManualStep`` itself; ``HEAD_COPY`` installs
    the written-out head with no error switched on, which must give ``ManualStep``'s bits (asserted by a
    self-check, so that a mutant fails for its mutation and not because the copy has drifted)."""
    from drone2d_amd.ppo import _HALF_LOG_2PI, ManualStep

    assert mutant is None or mutant == HEAD_COPY or mutant in GRAD_MUTANTS, mutant
    step = ManualStep(policy, cfg, "cpu")
    if mutant is None:
        return step
    if mutant == "one_minus_h":
        step._tanh_grad_torch = lambda h, g: g.mul_(1.0 - h)
        return step

    def head(mean, V, A, OL, ADV, R, acc, OV=None):
        ls = step.pol.log_std
        M, c, cv = mean.shape[0], cfg.clip_range, -1.0
        if step.ctl is not None:
            c, cv = step.ctl.coef[1], step.ctl.coef[2]
        isig = torch.exp(-ls)
        z = (A - mean) * isig
        logp = (-0.5 * z * z - ls - _HALF_LOG_2PI).sum(1)
        adv = ADV
        if cfg.normalize_advantage and M > 1:
            adv = (ADV - ADV.mean()) / (ADV.std(unbiased=mutant != "biased_std") + 1e-8)
        ratio = torch.exp(logp - OL)
        s1 = adv * ratio
        s2 = adv * torch.clamp(ratio, 1 - c, 1 + c)
        pl = -torch.minimum(s1, s2).mean()
        err = R - V
        vl = (err * err).mean()
        take = (s1 < s2) if mutant == "s1_lt_s2" else (s1 <= s2)
        g_lp = torch.where(take, adv, 0.0) * ratio * (-1.0 / M)
        gz = g_lp[:, None] * z
        g_V = err * (-2.0 * cfg.vf_coef / M)
        if cv >= 0.0:
            d = V - OV
            err = R - (OV + torch.clamp(d, -cv, cv))
            vl = (err * err).mean()
            g_V = torch.where(d.abs() <= cv, err * (-2.0 * cfg.vf_coef / M), 0.0)
        torch.sum(gz * z - g_lp[:, None], 0, out=ls.grad)
        if mutant != "no_ent_coef":
            ls.grad.sub_(cfg.ent_coef)
        acc["policy_loss"] += pl
        acc["value_loss"] += vl
        acc["entropy"] += (0.5 + _HALF_LOG_2PI + ls).sum()
        acc["clip_fraction"] += ((ratio if mutant == "clip_on_ratio" else ratio - 1).abs() > c).float().mean()
        if step.ctl is not None:
            step.ctl.record(((ratio - 1) - (logp - OL)).mean())
        return gz * isig, g_V

    step._head_torch = head
    return step


def clone_policy(pol, device="cpu"):
    out = type(pol)()
    out.load_state_dict(pol.state_dict())
    return out.to(device)


def new_acc(device="cpu"):
    return {k: torch.zeros((), device=device) for k in STATS}


def grad_errors(step, pol, names, ref_grads, ref_stats, acc, kl=None):
    """Relative L2 errors of a step's gradients (per parameter tensor) and statistics against the
    float64 reference: {name: error}."""
    out = {n: rel_l2(p.grad, g) for n, p, g in zip(names, pol.parameters(), ref_grads)}
    for k in STATS:
        out[k] = rel_l2(acc[k], ref_stats[k])
    if kl is not None:
        out["approx_kl"] = rel_l2(kl, ref_stats["approx_kl"])
    return out


# --------------------------------------------------------------------------------------------- GAE
def gae_per_env64(rew, val, done, last_value, gamma, lam):
    """SB3's GAE recursion env by env in Python floats (the recursion of
    tests/test_ppo.py::test_gae_matches_per_env_recursion): ``rew``, ``val``, ``done`` [T, N]
    (done[t]: step t ended the episode), ``last_value`` [N]; returns float64 (adv, ret) [T, N]."""
    rew, val, done = (np.asarray(x, dtype=np.float64) for x in (rew, val, done))
    lv = np.asarray(last_value, dtype=np.float64)
    T, N = rew.shape
    adv = np.zeros((T, N))
    for n in range(N):
        gae = 0.0
        for t in reversed(range(T)):
            nv = lv[n] if t == T - 1 else val[t + 1, n]
            nt = 1.0 - done[t, n]
            gae = (rew[t, n] + gamma * nv * nt - val[t, n]) + gamma * lam * nt * gae
            adv[t, n] = gae
    return adv, adv + val


# ------------------------------------------------------------------------------------------- ftanh
def ulp32(ref64):
    """The float32 spacing at |ref| (float64 array), with the normal range's smallest spacing below it."""
    a = np.abs(np.asarray(ref64, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -126.0) - 23.0)


def ftanh_points():
    """2048 non-negative float32 values v (the other 2048 rows are their negatives): +0, a subnormal,
    0.25 and its two neighbours times 2^-3 .. 2^4 (so every column's scale 2^(j % 8 - 4) meets them),
    1000 uniform in [0.2, 0.3], 500 in [0, 9], 1e30, inf, and a log sweep 1e-30 .. 1e4."""
    g = torch.Generator().manual_seed(7)
    q = np.float32(0.25)
    near = [np.nextafter(q, np.float32(0)), q, np.nextafter(q, np.float32(1))]
    pts = [0.0, 2.0 ** -140] + [float(x) * 2.0 ** s for x in near for s in range(-3, 5)]
    pts += (0.2 + 0.1 * torch.rand(1000, generator=g, dtype=torch.float64)).tolist()
    pts += (9.0 * torch.rand(500, generator=g, dtype=torch.float64)).tolist()
    pts += [1e30, math.inf]
    n_sweep = 2048 - len(pts)
    pts += np.logspace(-30, 4, n_sweep).tolist()
    v = torch.tensor(pts, dtype=torch.float64).float()
    assert v.shape == (2048,)
    return v
