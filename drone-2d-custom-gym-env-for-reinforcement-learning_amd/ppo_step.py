"""One SB3 PPO minibatch step behind one interface, ``step(idx, rollout, acc, world, adv_ws, zero_grad)``,
``reset_control()``, ``ctl`` (a ``ControlBlock`` or ``None``), ``set_lr(lr)``, ``state()`` / ``load_state(ts)`` (the
optimiser's entries of ``train_state.pth``): ``ManualStep`` (libd2d_ppo.so, or torch ops) and ``AutogradStep``."""
from __future__ import annotations

import ctypes as C
import math
import os

import torch
import torch.distributed as dist

from .policy import _HALF_LOG_2PI
from .ppo_native import D2DPPOCtl, _ok, ppo_native

STAT_KEYS = ("policy_loss", "value_loss", "entropy", "clip_fraction")


class ControlBlock:
    """The device-resident control block of one update (include/d2d_ppo.h ``d2d_ppo_ctl``) and, behind
    it in the same 12-float tensor, the four loss statistics, so one transfer brings everything an
    update's record needs.  The host writes the coefficients (``set``: one stream-ordered copy, outside
    any graph); the update's kernels -- or, on the torch paths, ``record`` / ``decide`` -- do the rest."""
    WORDS = C.sizeof(D2DPPOCtl) // 4
    LR, CLIP, CLIP_VF, KL_LIMIT, STOP, COUNT, KL_SUM, KL_LAST = range(8)

    def __init__(self, device):
        self.buf = torch.zeros(self.WORDS + len(STAT_KEYS), device=device)
        self.ibuf = self.buf.view(torch.int32)
        self.coef = None  # the host's copy of (lr, clip, clip_vf, kl_limit)
        self.set(0.0, 0.0, -1.0, math.inf)

    def ptr(self) -> int:
        return self.buf.data_ptr()

    def acc(self) -> dict:
        return {k: self.buf[self.WORDS + i] for i, k in enumerate(STAT_KEYS)}

    def set(self, lr: float, clip: float, clip_vf: float, kl_limit: float):
        host = torch.tensor([lr, clip, clip_vf, kl_limit], dtype=torch.float32)
        self.coef = tuple(float(x) for x in (lr, clip, clip_vf, kl_limit))
        self.buf[:4].copy_(host, non_blocking=True)

    def read(self) -> dict:
        """The update's record entries (one device-to-host copy): the four means over the recorded
        minibatches, approx_kl, n_minibatches, early_stop and the coefficients the update used."""
        h = self.buf.detach().cpu()
        hi = h.view(torch.int32)
        n = int(hi[self.COUNT])
        out = {k: float(h[self.WORDS + i]) / max(n, 1) for i, k in enumerate(STAT_KEYS)}
        out.update(approx_kl=float(h[self.KL_SUM]) / max(n, 1), n_minibatches=n, early_stop=int(hi[self.STOP]),
                   learning_rate=float(h[self.LR]), clip_range=float(h[self.CLIP]))
        if float(h[self.CLIP_VF]) >= 0.0:
            out["clip_range_vf"] = float(h[self.CLIP_VF])
        return out

    def kl_last(self) -> torch.Tensor:  # a one-float view: it rides behind the gradients in _rank_mean
        return self.buf[self.KL_LAST:self.KL_LAST + 1]

    # the torch paths' halves of the *_ctl kernels (CPU ManualStep, autograd)
    def reset(self):
        self.buf[self.STOP:self.WORDS].zero_()

    def stopped(self) -> bool:
        return bool(self.ibuf[self.STOP])

    def record(self, kl: torch.Tensor):
        self.ibuf[self.COUNT] += 1
        self.buf[self.KL_LAST] = kl
        self.buf[self.KL_SUM] += kl

    def decide(self) -> bool:
        """SB3's check, after the statistics: True (and the stop flag set) when the last KL exceeds
        the limit, so the caller must not step."""
        if float(self.buf[self.KL_LAST]) > self.coef[3]:
            self.ibuf[self.STOP] = 1
            return True
        return False


def _rank_mean(grads, world: int, extra=None):
    """Data-parallel PPO: the mean over the ranks of ``grads`` in one all-reduce (RCCL) -- a list of tensors,
    flattened and scattered back, or one flat buffer, reduced in place, whose last slot is free when ``extra`` is
    given: a one-float tensor that travels behind the gradients (the minibatch KL: one decision on every rank)."""
    flat = grads
    if not isinstance(grads, torch.Tensor):
        flat = torch.cat([g.reshape(-1) for g in grads] + ([extra] if extra is not None else []))
    elif extra is not None:
        flat[-1:].copy_(extra)
    dist.all_reduce(flat)
    flat.div_(world)
    if flat is not grads:
        o = 0
        for g in grads:
            k = g.numel()
            g.copy_(flat[o:o + k].view_as(g))
            o += k
    if extra is not None:
        extra.copy_(flat[-1:])


def _wgrad(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, rows: int = 512):
    """out = a^T b for a [M, p], b [M, q] (a weight gradient: the sum over the minibatch's samples).
    With K = M in the tens of thousands and a tiny p x q output, one GEMM runs on a handful of
    workgroups; split the sample axis into M / rows chunks (one batched GEMM) and add them up."""
    M = a.shape[0]
    if M % rows or M < 4 * rows:
        torch.mm(a.t(), b, out=out)
        return
    S = M // rows
    torch.sum(torch.bmm(a.reshape(S, rows, a.shape[1]).transpose(1, 2), b.reshape(S, rows, b.shape[1])), 0, out=out)


class ManualStep:
    """One SB3 PPO minibatch step (loss, gradient, clipping and Adam) with the backward pass of the two
    27-64-64 tanh MLPs written out instead of recorded by autograd, over flat parameter / gradient /
    Adam-moment buffers (the module's parameters become views of them), and nothing that waits for the
    host -- the whole step captures into one HIP graph.  On a GPU it is seven libd2d_ppo.so launches
    (advantage statistics, both MLPs forward with four threads per sample and net, loss head + backward to
    the hidden-layer gradients, all weight / bias gradients + their reduce, log_std's gradient and the
    statistics, clip + Adam) instead of ~190 autograd / optimiser kernels; on the CPU the same math in torch
    ops (split-K weight gradients).

    Gradients of the loss (SB3 PPO.train, stable_baselines3/ppo/ppo.py 2.1):
      ratio = exp(logp - old_logp), s1 = adv ratio, s2 = adv clamp(ratio, 1 - c, 1 + c)
      d(-mean min(s1, s2)) / d logp_i = -adv_i [s1_i <= s2_i] ratio_i / M   (ties: autograd splits
        the gradient between the two equal branches, whose derivatives are then both adv_i)
      d logp / d mean = z / sigma, d logp / d log_std = z^2 - 1 (z = (a - mean) / sigma);
      entropy bonus: d(-ent_coef mean H) / d log_std = -ent_coef; value: vf_coef * -2 (R - V) / M.
    Adam as torch.optim.Adam (lerp first moment, bias corrections, eps outside the square root).

    With ``cfg.control`` the step takes its learning rate, clip range and value clip range from the
    control block ``ctl`` (``set_coefs``), the rollout tuple has a sixth entry (the stored values),
    ``grad`` also records approx_kl, and ``apply`` is SB3's target_kl check before the optimiser step:
    once a minibatch's KL exceeds the limit neither it nor any later ``step`` of the update
    (until ``reset_control``) changes anything.  On a GPU these are the ``*_ctl`` entry points of
    libd2d_ppo.so, which read the block on the device, so the sequence captures into a HIP graph."""

    def __init__(self, policy, cfg, device):
        self.pol, self.cfg = policy, cfg
        params = list(policy.parameters())
        n = sum(p.numel() for p in params)
        self.P = torch.zeros(n, device=device)
        self.ctl = ControlBlock(device) if cfg.control else None
        # control: one float behind G, where the minibatch KL rides in the gradient's collective (apply, world > 1)
        self.Gx = torch.zeros(n + (self.ctl is not None), device=device)
        self.G = self.Gx[:n]
        if self.ctl is not None:
            self.set_coefs()
        self.m = torch.zeros(n, device=device)
        self.v = torch.zeros(n, device=device)
        self.t = torch.zeros((), device=device)
        # the fused element-wise kernels on a GPU (libd2d_ppo.so, loud if missing); torch ops on CPU
        self.lib = ppo_native() if torch.device(device).type == "cuda" else None
        self._bufs = {}  # minibatch size -> (work buffers, partial rows) of the HIP path
        # D2D_PPO_FUSED=1 (default): forward + backward + weight gradients in one launch
        # (d2d_ppo_fused_grad) + the reduce; 0: the separate kernels (forward, backward, wgrad + reduce)
        self.fused = self.lib is not None and os.environ.get("D2D_PPO_FUSED", "1") == "1"
        if self.ctl is not None and self.lib is not None and not self.fused:
            raise RuntimeError("the PPO control path (learning_rate_end, clip_range_end, clip_range_vf, target_kl) "
                               "has no separate-kernel variant: unset D2D_PPO_FUSED=0")
        o = 0
        for p in params:
            k = p.numel()
            self.P[o:o + k].copy_(p.data.reshape(-1))
            p.data = self.P[o:o + k].view_as(p)
            p.grad = self.G[o:o + k].view_as(p)
            o += k

    @torch.no_grad()
    def step(self, idx, rollout, acc: dict, world: int = 1, adv_ws=None, zero_grad: bool = True):
        """(``zero_grad`` is ``AutogradStep``'s: ``grad`` overwrites ``G``.)"""
        self.grad(idx, rollout, acc, adv_ws)
        self.apply(world)

    def set_coefs(self, progress_remaining: float = 1.0):
        """Write this update's coefficients (``cfg.coefs``) into the control block."""
        self.ctl.set(*self.cfg.coefs(progress_remaining))

    def set_lr(self, lr: float):
        pass  # the step reads its learning rate from the control block

    def state(self) -> dict:
        return {"m": self.m, "v": self.v, "t": self.t}

    def load_state(self, ts: dict):
        if "m" not in ts:
            raise ValueError("saved with the torch optimiser, config.manual says ManualStep")
        for k, x in self.state().items():
            x.copy_(ts[k])

    def reset_control(self):
        """The first step of an update: clear the stop flag, the count and the KL sums."""
        if self.lib is not None:
            _ok(self.lib.d2d_ppo_ctl_reset(self.ctl.ptr(), self._stream()), "d2d_ppo_ctl_reset")
        else:
            self.ctl.reset()

    def grad(self, idx, rollout, acc: dict, adv_ws=None):
        """The loss gradient of minibatch ``idx`` of ``rollout`` = (obs, actions, old log-probs,
        advantages, returns[, old values: the control path]) into ``G``; statistics added to ``acc``."""
        if self.ctl is not None and len(rollout) < 6:
            raise ValueError("the control path needs the rollout's stored values as rollout[5]")
        if self.lib is None:
            self._grad_torch(idx, rollout, acc)
        elif self.fused:
            self._grad_fused(idx, rollout, acc, adv_ws)
        else:
            self._grad_hip(idx, rollout[:5], acc)

    def _grad_torch(self, idx, rollout, acc):
        """The CPU path: both MLPs forward, ``_head_torch``, the backward pass, all in torch ops."""
        if self.ctl is not None and self.ctl.stopped():
            return
        p1, p2, p3, v1, v2, v3 = self._linears()
        obs_all, act_all, ol_all, adv_all, ret_all = rollout[:5]
        X = obs_all[idx]
        # forward (nn.Linear = addmm)
        h1p = torch.tanh(torch.addmm(p1.bias, X, p1.weight.t()))
        h2p = torch.tanh(torch.addmm(p2.bias, h1p, p2.weight.t()))
        mean = torch.addmm(p3.bias, h2p, p3.weight.t())
        h1v = torch.tanh(torch.addmm(v1.bias, X, v1.weight.t()))
        h2v = torch.tanh(torch.addmm(v2.bias, h1v, v2.weight.t()))
        V = torch.addmm(v3.bias, h2v, v3.weight.t()).squeeze(1)
        g_mean, g_V = self._head_torch(mean, V, act_all[idx], ol_all[idx], adv_all[idx], ret_all[idx], acc,
                                       rollout[5][idx] if self.ctl is not None else None)
        tg = self._tanh_grad_torch
        # backward: the layer-output gradients, then every weight / bias gradient
        g2p = tg(h2p, torch.mm(g_mean, p3.weight))
        g2v = tg(h2v, g_V[:, None] * v3.weight)
        g1p = tg(h1p, torch.mm(g2p, p2.weight))
        g1v = tg(h1v, torch.mm(g2v, v2.weight))
        for a, b, lin in ((g_mean, h2p, p3), (g_V[:, None], h2v, v3), (g2p, h1p, p2), (g2v, h1v, v2), (g1p, X, p1),
                          (g1v, X, v1)):
            _wgrad(a, b, lin.weight.grad)
            torch.sum(a, 0, out=lin.bias.grad)

    def _grad_hip(self, idx, rollout, acc):
        """libd2d_ppo.so, the separate kernels: advantage statistics, both MLPs forward (four threads per sample
        and net), loss head + backward to the hidden-layer gradients, all weight / bias gradients, log_std's."""
        cfg, pol, lib, st = self.cfg, self.pol, self.lib, self._stream()
        obs_all, act_all, ol_all, adv_all, ret_all = rollout
        M, dev = idx.numel(), self.P.device
        if M not in self._bufs:
            # one set of work buffers per minibatch size, kept for the handle's life: a captured graph
            # holds the full-size set's addresses while a ragged last minibatch runs eagerly on its own
            e = lambda *sh: torch.empty(*sh, device=dev)  # noqa: E731
            hb = {"h1p": e(M, 64), "h2p": e(M, 64), "mean": e(M, 2), "g1p": e(M, 64), "g2p": e(M, 64),
                  "h1v": e(M, 64), "h2v": e(M, 64), "val": e(M, 1), "g1v": e(M, 64), "g2v": e(M, 64),
                  "xg": e(M, 27), "gm": e(M, 2), "gv": e(M, 1),
                  "ws": torch.zeros((M + 63) // 64, 2, dtype=torch.float64, device=dev)}  # D2D_PPO_HEAD_BLOCK rows each
            prow = lib.d2d_ppo_mlp_partial_rows(M)
            hb["partial"] = torch.zeros(prow, 5, device=dev)
            hb["wpart"] = e(lib.d2d_ppo_wgrad_chunks(M) * self.G.numel())  # weight-gradient partial rows
            self._bufs[M] = (hb, prow)
        hb, prow = self._bufs[M]
        p1, p2, p3, v1, v2, v3 = self._linears()
        wptr = self.weight_ptrs()
        bptr = (C.c_void_p * 10)(*[hb[k].data_ptr() for k in ("h1p", "h2p", "mean", "g1p", "g2p",
                                                              "h1v", "h2v", "val", "g1v", "g2v")])
        gptr = (C.c_void_p * 2)(hb["gm"].data_ptr(), hb["gv"].data_ptr())
        norm = int(cfg.normalize_advantage and M > 1)
        # the forward launch also writes the advantage statistics' partials when they are needed
        _ok(lib.d2d_ppo_mlp_forward_adv(M, idx.data_ptr(), obs_all.data_ptr(), adv_all.data_ptr() if norm else None,
                                        wptr, bptr, hb["xg"].data_ptr(), hb["ws"].data_ptr(), st),
            "d2d_ppo_mlp_forward_adv")
        _ok(lib.d2d_ppo_mlp_backward(M, idx.data_ptr(), act_all.data_ptr(), ol_all.data_ptr(), adv_all.data_ptr(),
                                     ret_all.data_ptr(), pol.log_std.data_ptr(), hb["ws"].data_ptr(), norm,
                                     cfg.clip_range, cfg.vf_coef, wptr, bptr, gptr, hb["partial"].data_ptr(), st),
            "d2d_ppo_mlp_backward")
        # all six weight / bias gradients in one launch (+ its reduce) into G; the head's finish (log-std gradient,
        # loss statistics) rides on the reduce's launch
        A = [hb[k] for k in ("gm", "gv", "g2p", "g2v", "g1p", "g1v")]
        B = [hb[k] for k in ("h2p", "h2v", "h1p", "h1v", "xg", "xg")]
        lins, n = (p3, v3, p2, v2, p1, v1), 6
        row_len = self.G.numel()  # all of G: log_std's slots (no problem covers them) are rewritten after
        assert hb["wpart"].numel() >= lib.d2d_ppo_wgrad_chunks(M) * row_len
        for a, b in zip(A, B):
            assert a.stride(1) == 1 and b.stride(1) == 1 and a.shape[0] == b.shape[0] == M
        ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
        ints = lambda v: (C.c_int32 * n)(*v)  # noqa: E731
        _ok(lib.d2d_ppo_wgrad_head(M, n, ptrs(A), ints(a.stride(0) for a in A), ptrs(B), ints(b.stride(0) for b in B),
                                   ints(a.shape[1] for a in A), ints(b.shape[1] for b in B),
                                   ints(self._off(lin.weight.grad) for lin in lins),
                                   ints(self._off(lin.bias.grad) for lin in lins), row_len, hb["wpart"].data_ptr(),
                                   self.G.data_ptr(), prow, hb["partial"].data_ptr(), *self._finish_args(acc), st),
            "d2d_ppo_wgrad_head")

    def _finish_args(self, acc: dict) -> tuple:
        """What finishes the loss head in a reduce launch (log_std, ent_coef, its gradient, the statistics)."""
        ls = self.pol.log_std
        return (ls.data_ptr(), self.cfg.ent_coef, ls.grad.data_ptr(), acc["policy_loss"].data_ptr(),
                acc["value_loss"].data_ptr(), acc["entropy"].data_ptr(), acc["clip_fraction"].data_ptr())

    def _grad_fused(self, idx, rollout, acc, adv_ws=None):
        """libd2d_ppo.so, two launches (+ the advantage statistics unless ``adv_ws`` points at this
        minibatch's precomputed d2d_ppo_adv_stats partials): d2d_ppo_fused_grad (both MLPs forward,
        the loss head, the backward and every weight / bias gradient, per-sample state on chip) and
        d2d_ppo_grad_reduce (the workgroups' rows into G, log_std's gradient, statistics)."""
        cfg, pol, lib, st = self.cfg, self.pol, self.lib, self._stream()
        M, dev, n = idx.numel(), self.P.device, self.G.numel()
        key = ("fused", M)
        if key not in self._bufs:
            rows = lib.d2d_ppo_fused_rows(M)
            self._bufs[key] = {"rows": rows, "wpart": torch.empty(rows * n, device=dev),
                               "hpart": torch.empty(2 * rows * (5 if self.ctl is None else 6), device=dev),
                               "ws": torch.zeros((M + 63) // 64, 2, dtype=torch.float64, device=dev)}
        b = self._bufs[key]
        offsets = (C.c_int32 * 12)(*[self._off(g) for lin in self._linears() for g in (lin.weight.grad, lin.bias.grad)])
        norm = int(cfg.normalize_advantage and M > 1)
        ws = adv_ws if adv_ws is not None else b["ws"].data_ptr()
        if norm and adv_ws is None:
            _ok(lib.d2d_ppo_adv_stats(M, idx.data_ptr(), rollout[3].data_ptr(), ws, st), "d2d_ppo_adv_stats")
        data = (M, idx.data_ptr(), *[x.data_ptr() for x in rollout[:5]])
        out = (self.weight_ptrs(), offsets, n, b["wpart"].data_ptr(), b["hpart"].data_ptr())
        reduce = (b["rows"], n, b["wpart"].data_ptr(), self.G.data_ptr(), 2 * b["rows"], b["hpart"].data_ptr(), M,
                  *self._finish_args(acc))
        ls = pol.log_std.data_ptr()
        if self.ctl is not None:
            # the control variants: clip / clip_vf / the stop flag from the block, KL into it
            ctl = self.ctl.ptr()
            _ok(lib.d2d_ppo_fused_grad_ctl(*data, rollout[5].data_ptr(), ls, ws, norm, cfg.vf_coef, *out, ctl, st),
                "d2d_ppo_fused_grad_ctl")
            _ok(lib.d2d_ppo_grad_reduce_ctl(*reduce, ctl, st), "d2d_ppo_grad_reduce_ctl")
        else:
            _ok(lib.d2d_ppo_fused_grad(*data, ls, ws, norm, cfg.clip_range, cfg.vf_coef, *out, st), "d2d_ppo_fused_grad")
            _ok(lib.d2d_ppo_grad_reduce(*reduce, st), "d2d_ppo_grad_reduce")

    def weight_ptrs(self):
        """The 12 weight / bias device pointers of include/d2d_ppo.h (policy net, then value net);
        views of the flat parameter buffer, so the addresses never change."""
        return (C.c_void_p * 12)(*[w.data_ptr() for lin in self._linears() for w in (lin.weight, lin.bias)])

    def _linears(self) -> tuple:
        pol = self.pol
        pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
        return (pn[0], pn[2], pol.action_net, vn[0], vn[2], pol.value_net)

    @staticmethod
    def _tanh_grad_torch(h, g):
        return g.mul_(1.0 - h * h)

    def _off(self, grad: torch.Tensor) -> int:  # a parameter's gradient as an offset into G, in floats
        return (grad.data_ptr() - self.G.data_ptr()) // 4

    def _stream(self):
        return torch.cuda.current_stream(self.P.device).cuda_stream

    def _head_torch(self, mean, V, A, OL, ADV, R, acc, OV=None):
        cfg, ls = self.cfg, self.pol.log_std
        M = mean.shape[0]
        c, cv = (cfg.clip_range, -1.0) if self.ctl is None else self.ctl.coef[1:3]
        isig = torch.exp(-ls)
        z = (A - mean) * isig
        logp = (-0.5 * z * z - ls - _HALF_LOG_2PI).sum(1)
        adv = ADV
        if cfg.normalize_advantage and M > 1:
            adv = (ADV - ADV.mean()) / (ADV.std() + 1e-8)
        ratio = torch.exp(logp - OL)
        s1 = adv * ratio
        s2 = adv * torch.clamp(ratio, 1 - c, 1 + c)
        pl = -torch.minimum(s1, s2).mean()
        err = R - V
        vl = (err * err).mean()
        g_lp = torch.where(s1 <= s2, adv, 0.0) * ratio * (-1.0 / M)  # d loss / d logp
        gz = g_lp[:, None] * z
        g_mean = gz * isig
        g_V = err * (-2.0 * cfg.vf_coef / M)
        if cv >= 0.0:
            # SB3 clip_range_vf: the prediction clipped around the stored value; torch.clamp's gradient
            # passes on the closed interval
            d = V - OV
            err = R - (OV + torch.clamp(d, -cv, cv))
            vl = (err * err).mean()
            g_V = torch.where(d.abs() <= cv, err * (-2.0 * cfg.vf_coef / M), 0.0)
        torch.sum(gz * z - g_lp[:, None], 0, out=ls.grad)
        ls.grad.sub_(cfg.ent_coef)
        acc["policy_loss"] += pl
        acc["value_loss"] += vl
        acc["entropy"] += (0.5 + _HALF_LOG_2PI + ls).sum()
        acc["clip_fraction"] += ((ratio - 1).abs() > c).float().mean()
        if self.ctl is not None:
            self.ctl.record(((ratio - 1) - (logp - OL)).mean())
        return g_mean, g_V

    def apply(self, world: int = 1):
        """Rank-mean of ``G`` (RCCL), clip_grad_norm_, Adam step on ``P``.  Control path: SB3's
        target_kl check first, on the rank mean of the minibatch KL, which travels behind ``G`` in the
        same collective so that every rank takes the same decision."""
        if world > 1:
            _rank_mean(self.Gx, world, None if self.ctl is None else self.ctl.kl_last())
        # (through the class: apply also works on any object with the fields P, G, m, v, t, cfg, ctl, lib)
        (ManualStep._adam_hip if self.lib is not None else ManualStep._adam_torch)(self)

    def _adam_hip(self):
        cfg = self.cfg
        args = (self.G.numel(), self.P.data_ptr(), self.G.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                self.t.data_ptr())
        if self.ctl is not None:  # the learning rate, the KL check and the stop flag: the block's, on the device
            _ok(self.lib.d2d_ppo_adam_ctl(*args, 0.9, 0.999, 1e-5, cfg.max_grad_norm, self.ctl.ptr(), self._stream()),
                "d2d_ppo_adam_ctl")
        else:
            _ok(self.lib.d2d_ppo_adam(*args, cfg.learning_rate, 0.9, 0.999, 1e-5, cfg.max_grad_norm, self._stream()),
                "d2d_ppo_adam")

    def _adam_torch(self):
        cfg, G = self.cfg, self.G
        lr = cfg.learning_rate
        if self.ctl is not None:
            if self.ctl.stopped() or self.ctl.decide():
                return
            lr = self.ctl.coef[0]
        # clip_grad_norm_(max_grad_norm): scale by min(1, max / (||g|| + 1e-6))
        G.mul_(torch.clamp(cfg.max_grad_norm / (torch.linalg.vector_norm(G) + 1e-6), max=1.0))
        # Adam(lr, betas (0.9, 0.999), eps 1e-5)
        b1, b2, eps = 0.9, 0.999, 1e-5
        self.t.add_(1.0)
        self.m.lerp_(G, 1.0 - b1)
        self.v.mul_(b2).addcmul_(G, G, value=1.0 - b2)
        bc1 = 1.0 - torch.pow(b1, self.t)
        bc2s = torch.sqrt(1.0 - torch.pow(b2, self.t))
        self.P.sub_(self.m * (lr / bc1) / (self.v.sqrt() / bc2s + eps))


class AutogradStep:
    """The same minibatch step recorded by autograd and applied by ``torch.optim.Adam`` (which it owns:
    ``opt``), in SB3 ``PPO.train``'s order: loss, backward, statistics, approx_kl, rank mean, the
    target_kl check, and only then clip and step.  The backward pass runs before the check, so that a
    multi-rank run can send the KL behind the gradients in their one collective; a stopped minibatch's
    gradients are simply not applied.  Without ``cfg.control`` there is no block (``ctl`` is ``None``), no
    KL and no check, and the statistics are added after the step."""
    lib = None  # torch ops on every device

    def __init__(self, policy, cfg, device, capturable: bool = False):
        self.pol, self.cfg = policy, cfg
        self.opt = torch.optim.Adam(policy.parameters(), lr=cfg.learning_rate, eps=1e-5, capturable=capturable)
        self.ctl = ControlBlock(device) if cfg.control else None

    def reset_control(self):
        self.ctl.reset()

    def set_lr(self, lr: float):
        for grp in self.opt.param_groups:
            grp["lr"] = lr

    def state(self) -> dict:
        return {"opt": self.opt.state_dict()}

    def load_state(self, ts: dict):
        self.opt.load_state_dict(ts["opt"])

    @torch.no_grad()
    def _stats(self, acc: dict, pl, vl, el, ratio, log_ratio, c: float):
        acc["policy_loss"] += pl
        acc["value_loss"] += vl
        acc["entropy"] -= el
        acc["clip_fraction"] += ((ratio - 1).abs() > c).float().mean()
        if self.ctl is not None:
            self.ctl.record(((ratio - 1) - log_ratio).mean())

    def step(self, idx, rollout, acc: dict, world: int = 1, adv_ws=None, zero_grad: bool = True):
        """``zero_grad=False``: the form a per-minibatch graph capture records, where backward writes
        fresh gradients (``PPO._capture``).  (``adv_ws`` is ``ManualStep``'s.)"""
        cfg, ctl = self.cfg, self.ctl
        if ctl is not None and ctl.stopped():
            return
        c, cv = (cfg.clip_range, -1.0) if ctl is None else ctl.coef[1:3]
        obs, act, old_logp, adv_all, ret = rollout[:5]
        params = list(self.pol.parameters())
        values, logp, entropy = self.pol.evaluate_actions(obs[idx], act[idx])
        adv = adv_all[idx]
        if cfg.normalize_advantage and idx.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        log_ratio = logp - old_logp[idx]
        ratio = torch.exp(log_ratio)
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
        if cv >= 0.0:
            ov = rollout[5][idx]
            values = ov + torch.clamp(values - ov, -cv, cv)
        vl = torch.nn.functional.mse_loss(ret[idx], values)
        el = -entropy.mean()
        loss = pl + cfg.ent_coef * el + cfg.vf_coef * vl
        if zero_grad:
            self.opt.zero_grad(set_to_none=False)
        loss.backward()
        if ctl is not None:
            self._stats(acc, pl, vl, el, ratio, log_ratio, c)
        if world > 1:
            _rank_mean([p.grad for p in params], world, None if ctl is None else ctl.kl_last())
        if ctl is not None and ctl.decide():
            return
        torch.nn.utils.clip_grad_norm_(params, cfg.max_grad_norm)
        self.opt.step()
        if ctl is None:
            self._stats(acc, pl, vl, el, ratio, log_ratio, c)
