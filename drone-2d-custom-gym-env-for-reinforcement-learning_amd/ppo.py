"""PPO end-to-end on the device: the rollout, GAE and the clipped-surrogate
update all stay on the GPU next to the HIP env batch, with no per-env Python objects.

The reference trains with Stable-Baselines3 2.1 ``PPO("MlpPolicy", env)`` over 14 SubprocVecEnv
workers (main.py:181-210; hyperparameters in ``ppo_agents/PFCA_see_3_obs_17_90.zip:data``: n_steps
2048, batch_size 64, n_epochs 10, gamma 0.99, gae_lambda 0.95, clip_range 0.2, ent_coef 0.01
(rl_config.py:7), vf_coef 0.5, max_grad_norm 0.5, lr 3e-4).  SB3 is not installed in this image;
this module restates the parts of SB3 2.1 that a training run executes, in the same order:

* ``ActorCritic``: SB3's ``MlpPolicy`` for a Box action space -- separate policy and value MLPs
  27-64-64 (tanh), ``action_net`` 64->2, ``value_net`` 64->1, state-independent ``log_std``
  (init 0), orthogonal init (gains sqrt(2) / 0.01 / 1, zero biases).  Parameter names follow SB3's
  state_dict, so a ``policy.pth`` from an SB3 zip loads into it.
* ``collect_rollouts`` (SB3 ``OnPolicyAlgorithm.collect_rollouts``): Gaussian actions, clipped to
  the action space only for the env; the stored actions and log-probabilities are the unclipped
  ones; rewards of time-limit truncations are bootstrapped with V(terminal obs) (the reference
  never truncates: time-up is terminal, so this path is idle by default).
* ``compute_returns_and_advantage`` (SB3 ``RolloutBuffer``): GAE(lambda) with episode starts.
* ``train`` (SB3 ``PPO.train``): shuffled minibatches, per-minibatch advantage normalisation,
  clipped surrogate, MSE value loss, entropy bonus, grad-norm clipping, Adam(eps=1e-5); with
  ``PPOConfig.control`` also SB3's learning-rate / clip-range schedules (linear), ``clip_range_vf``,
  ``approx_kl`` and the ``target_kl`` early stop, read from and decided in a device-resident
  ``ControlBlock`` so that they work inside the captured update (DESIGN.md "PPO control").

At 65 536 envs a 2 048-step rollout would hold 134 M transitions, so GPU-scale runs shorten
n_steps and enlarge batch_size (``PPOConfig.gpu_defaults``); the update rule is unchanged.  With
``torch.distributed`` initialised (one process per GPU, each with its env shard,
``drone2d_amd.shard``), gradients are averaged over ranks before each optimiser step (RCCL).

Agent files (``PPO.save`` / ``PPO.load`` / ``ActorCritic.from_sb3_zip``, ``Checkpoint``): a zip laid out
like SB3's -- ``policy.pth`` is the policy's state_dict under SB3's names -- whose other members carry
what a resumed run needs (optimiser moments, noise generator, the rollout's carried observations, the
env batch's state).  Every member holds tensors or JSON only (``torch.load(weights_only=True)``).
"""
from __future__ import annotations

import dataclasses
import io
import json
import math
import os
import time
import zipfile
from dataclasses import dataclass

import numpy as np
import torch
import torch.distributed as dist
from torch import nn


@dataclass
class PPOConfig:
    n_steps: int = 2048
    batch_size: int = 64
    n_epochs: int = 10
    learning_rate: float = 3e-4
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_range: float = 0.2
    ent_coef: float = 0.01          # rl_config.py:7
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    normalize_advantage: bool = True
    graph: bool = True              # GPU, one rank: the minibatch update replayed as one HIP graph
    manual: bool = True             # MLP backward + Adam written out over flat buffers (ManualStep)
    # PPO control (include/d2d_ppo.h "PPO control"); None = off.  Setting any of the four selects the
    # control path: the update reads its coefficients from a device-resident control block, records
    # approx_kl and can stop early on its own, also inside a captured HIP graph.
    learning_rate_end: float | None = None  # linear schedule: x = end + (start - end) * progress_remaining
    clip_range_end: float | None = None
    clip_range_vf: float | None = None      # SB3 clip_range_vf: the value prediction clipped around old_values
    target_kl: float | None = None          # SB3 target_kl; float("inf"): never stops, approx_kl logged only

    def __post_init__(self):
        for name in ("learning_rate", "clip_range"):
            if callable(getattr(self, name)):
                raise TypeError(f"PPOConfig.{name} is a callable: a schedule cannot be stored in an agent file; "
                                f"give the start value as {name} and the final one as {name}_end (linear in SB3's "
                                "progress_remaining)")

    @property
    def control(self) -> bool:
        return any(x is not None for x in (self.learning_rate_end, self.clip_range_end, self.clip_range_vf,
                                           self.target_kl))

    def coefs(self, progress_remaining: float = 1.0) -> tuple:
        """(lr, clip_range, clip_range_vf or -1.0, KL limit = 1.5 * target_kl or +inf) of an update at
        SB3's ``progress_remaining`` (1 at the start of a run, 0 at its end)."""
        def lin(start, end):
            return start if end is None else end + (start - end) * progress_remaining

        return (float(lin(self.learning_rate, self.learning_rate_end)), float(lin(self.clip_range, self.clip_range_end)),
                -1.0 if self.clip_range_vf is None else float(self.clip_range_vf),
                math.inf if self.target_kl is None else 1.5 * float(self.target_kl))

    @classmethod
    def gpu_defaults(cls, **over) -> "PPOConfig":
        """Short rollouts over many envs (65 536 x 16 = 1 M samples per update), big minibatches."""
        return cls(**dict(dict(n_steps=16, batch_size=32768), **over))


@dataclass
class Checkpoint:
    """``PPO.learn(checkpoint=...)``: save ``<save_path>/<name_prefix>_<num_timesteps>_steps.zip`` whenever
    ``num_timesteps`` crosses a multiple of ``save_freq`` -- SB3's CheckpointCallback file names, which
    the reference reads back as its curriculum clock (main.py:161-177, drone_2d_env.py:76-86)."""
    save_freq: int
    save_path: str
    name_prefix: str = "rl_model"


AGENT_FORMAT_VERSION = 1
AGENT_MEMBERS = ("data.json", "policy.pth", "train_state.pth", "env_state.pth")

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _zip_tensors(z: zipfile.ZipFile, name: str) -> dict:
    return torch.load(io.BytesIO(z.read(name)), map_location="cpu", weights_only=True)


def _to_tensors(x):
    """A checkpoint value with every NumPy array as a tensor (so the member loads weights_only)."""
    if isinstance(x, dict):
        return {k: _to_tensors(v) for k, v in x.items()}
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x))
    return x


def _to_arrays(sd: dict) -> dict:
    """An ``env_state.pth`` member as ``Drone2dVecEnv.load_state_dict`` takes it: the nested tables
    (curriculum pool, fresh-curriculum recipes) back as NumPy arrays, the state tensors as they are."""
    return {k: ({kk: (vv.numpy() if isinstance(vv, torch.Tensor) else vv) for kk, vv in v.items()}
                if isinstance(v, dict) else v) for k, v in sd.items()}


class ActorCritic(nn.Module):
    """SB3 2.1 ``MlpPolicy`` (net_arch pi=[64, 64], vf=[64, 64], tanh) for obs 27 -> action 2."""

    def __init__(self, obs_dim: int = 27, act_dim: int = 2, hidden: int = 64, log_std_init: float = 0.0):
        super().__init__()
        self.mlp_extractor = nn.Module()
        self.mlp_extractor.policy_net = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(),
                                                      nn.Linear(hidden, hidden), nn.Tanh())
        self.mlp_extractor.value_net = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(),
                                                     nn.Linear(hidden, hidden), nn.Tanh())
        self.action_net = nn.Linear(hidden, act_dim)
        self.value_net = nn.Linear(hidden, 1)
        self.log_std = nn.Parameter(torch.ones(act_dim) * log_std_init)
        # ActorCriticPolicy._build, ortho_init=True
        for mod, gain in ((self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01), (self.value_net, 1.0)):
            for m in mod.modules():
                if isinstance(m, nn.Linear):
                    nn.init.orthogonal_(m.weight, gain=gain)
                    m.bias.data.fill_(0.0)

    def forward(self, obs: torch.Tensor):
        mean = self.action_net(self.mlp_extractor.policy_net(obs))
        value = self.value_net(self.mlp_extractor.value_net(obs)).squeeze(-1)
        return mean, value

    def dist(self, mean: torch.Tensor) -> torch.distributions.Normal:
        return torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp(), validate_args=False)

    def log_prob(self, mean: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        """Diagonal-Gaussian log density summed over the action dims (SB3 DiagGaussianDistribution),
        written out so it captures into a HIP graph (torch.distributions validates on the host)."""
        z = (actions - mean) * torch.exp(-self.log_std)
        return (-0.5 * z * z - self.log_std - _HALF_LOG_2PI).sum(-1)

    def entropy(self, n: int) -> torch.Tensor:
        return (0.5 + _HALF_LOG_2PI + self.log_std).sum().expand(n)

    def evaluate_actions(self, obs: torch.Tensor, actions: torch.Tensor):
        mean, value = self(obs)
        return value, self.log_prob(mean, actions), self.entropy(obs.shape[0])

    @torch.no_grad()
    def predict_values(self, obs: torch.Tensor) -> torch.Tensor:
        return self(obs)[1]

    @classmethod
    def from_agent_npz(cls, path: str) -> "ActorCritic":
        """The actor of a shipped agent (tests/golden/agent_17_90.npz: SB3 names with '.' -> '_');
        the value net keeps its fresh init (the fixture holds the actor only)."""
        m = cls()
        with np.load(path, allow_pickle=False) as z:
            sd = {k: torch.as_tensor(z[k]) for k in z.files}
        names = {n.replace(".", "_"): n for n in m.state_dict()}
        m.load_state_dict({names[k]: v for k, v in sd.items()}, strict=False)
        return m

    @classmethod
    def from_sb3_zip(cls, path: str) -> "ActorCritic":
        """The policy of an agent zip: ``policy.pth`` of a file written by ``PPO.save`` or by SB3's
        ``PPO.save`` (the reference's ``ppo_agents/*.zip``).  The actor must be complete; the value
        net is loaded when the file has one, and keeps its fresh init otherwise."""
        with zipfile.ZipFile(path) as z:
            if "policy.pth" not in z.namelist():
                raise ValueError(f"{path}: no policy.pth member")
            sd = _zip_tensors(z, "policy.pth")
        m = cls()
        own = m.state_dict()
        actor = [k for k in own if k.startswith(("mlp_extractor.policy_net.", "action_net.", "log_std"))]
        missing = [k for k in actor if k not in sd]
        if missing:
            raise ValueError(f"{path}: policy.pth lacks {missing}")
        bad = [k for k in own if k in sd and tuple(sd[k].shape) != tuple(own[k].shape)]
        if bad:
            raise ValueError(f"{path}: policy.pth is not an MlpPolicy 27-64-64 (shape of {bad})")
        m.load_state_dict({k: v.float() for k, v in sd.items() if k in own}, strict=False)
        return m


_PPO_LIB = None

import ctypes as _C  # noqa: E402


class D2DPPORollout(_C.Structure):
    """include/d2d_ppo.h ``d2d_ppo_rollout`` (one fused rollout step, ABI v4)."""
    _fields_ = [(k, _C.c_int32) for k in ("n", "t", "T", "info_dim", "info_totrew")] + \
               [("gamma", _C.c_float), ("gae_lambda_gamma", _C.c_float), ("pad", _C.c_int32)] + \
               [(k, _C.c_void_p) for k in ("obs", "noise", "log_std", "prev_rew", "prev_term", "prev_trunc",
                                           "prev_info", "obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf",
                                           "done_buf", "start0", "act_env", "adv_buf", "ret_buf", "stats")]


class D2DPPOCtl(_C.Structure):
    """include/d2d_ppo.h ``d2d_ppo_ctl``: the control block's eight words (``ControlBlock.buf[:8]``)."""
    _fields_ = [(k, _C.c_float) for k in ("lr", "clip", "clip_vf", "kl_limit")] + \
               [("stop", _C.c_int32), ("count", _C.c_int32), ("kl_sum", _C.c_float), ("kl_last", _C.c_float)]


PPO_CTL_VERSION = 1
_STAT_KEYS = ("policy_loss", "value_loss", "entropy", "clip_fraction")


class ControlBlock:
    """The device-resident control block of one update (include/d2d_ppo.h ``d2d_ppo_ctl``) and, behind
    it in the same 12-float tensor, the four loss statistics, so one transfer brings everything an
    update's record needs.  The host writes the coefficients (``set``: one stream-ordered copy, outside
    any graph); the update's kernels -- or, on the torch paths, ``record`` / ``decide`` -- do the rest."""
    WORDS = _C.sizeof(D2DPPOCtl) // 4
    LR, CLIP, CLIP_VF, KL_LIMIT, STOP, COUNT, KL_SUM, KL_LAST = range(8)

    def __init__(self, device):
        self.buf = torch.zeros(self.WORDS + len(_STAT_KEYS), device=device)
        self.ibuf = self.buf.view(torch.int32)
        self.coef = None  # the host's copy of (lr, clip, clip_vf, kl_limit)
        self.set(0.0, 0.0, -1.0, math.inf)

    def ptr(self) -> int:
        return self.buf.data_ptr()

    def acc(self) -> dict:
        return {k: self.buf[self.WORDS + i] for i, k in enumerate(_STAT_KEYS)}

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
        out = {k: float(h[self.WORDS + i]) / max(n, 1) for i, k in enumerate(_STAT_KEYS)}
        out.update(approx_kl=float(h[self.KL_SUM]) / max(n, 1), n_minibatches=n, early_stop=int(hi[self.STOP]),
                   learning_rate=float(h[self.LR]), clip_range=float(h[self.CLIP]))
        if float(h[self.CLIP_VF]) >= 0.0:
            out["clip_range_vf"] = float(h[self.CLIP_VF])
        return out

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


def ppo_native():
    """ctypes binding of libd2d_ppo.so (include/d2d_ppo.h), loaded once; no fallback on a GPU."""
    global _PPO_LIB
    if _PPO_LIB is None:
        import ctypes as C
        import os

        from . import _native  # noqa: F401  (torch owns the HIP runtime first)

        path = os.environ.get("D2D_PPO_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib",
                                                             "libd2d_ppo.so")  # (env: A/B builds, tools/)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: the HIP extension is not built "
                               "(run `python -c 'import __graft_entry__ as g; g.build()'`)")
        lib = C.CDLL(path)
        vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
        sig = {
            "d2d_ppo_abi_version": [],
            "d2d_ppo_adv_stats": [i32, vp, vp, vp, vp],
            "d2d_ppo_head_finish": [i32, i32, vp, vp, f32, vp, vp, vp, vp, vp, vp],
            "d2d_ppo_adam": [i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, vp],
            "d2d_ppo_wgrad": [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp],
            "d2d_ppo_wgrad_head": [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp,
                                   i32, vp, vp, f32, vp, vp, vp, vp, vp, vp],
            "d2d_ppo_wgrad_chunks": [i32],
            "d2d_ppo_mlp_forward": [i32, vp, vp, vp, vp, vp, vp],
            "d2d_ppo_mlp_forward_adv": [i32, vp, vp, vp, vp, vp, vp, vp, vp],
            "d2d_ppo_mlp_backward": [i32, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, vp, vp, vp, vp, vp],
            "d2d_ppo_mlp_partial_rows": [i32],
            "d2d_ppo_permute": [i64, i32, C.c_uint64, vp, vp, vp],
            "d2d_ppo_rollout_step": [C.POINTER(D2DPPORollout), vp, vp],
            "d2d_ppo_fused_rows": [i32],
            "d2d_ppo_fused_grad": [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32, vp, vp, i32, vp, vp, vp],
            "d2d_ppo_grad_reduce": [i32, i32, vp, vp, i32, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp],
            # the control path (additive to ABI v6; versioned by d2d_ppo_ctl_version)
            "d2d_ppo_ctl_version": [],
            "d2d_ppo_ctl_reset": [vp, vp],
            "d2d_ppo_fused_grad_ctl": [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, vp, vp, i32, vp, vp, vp, vp],
            "d2d_ppo_grad_reduce_ctl": [i32, i32, vp, vp, i32, vp, i32, vp, f32, vp, vp, vp, vp, vp, vp, vp],
            "d2d_ppo_adam_ctl": [i32, vp, vp, vp, vp, vp, f32, f32, f32, f32, vp, vp],
        }
        for name, args in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = C.c_int32, args
        if lib.d2d_ppo_abi_version() != 6:
            raise RuntimeError("libd2d_ppo.so ABI mismatch")
        if lib.d2d_ppo_ctl_version() != PPO_CTL_VERSION:
            raise RuntimeError("libd2d_ppo.so control-block version mismatch")
        _PPO_LIB = lib
    return _PPO_LIB


def _ok(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError {rc}")


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
    """One SB3 PPO minibatch step (``PPO._minibatch``'s loss, gradient, clipping and Adam) with the
    backward pass of the two 27-64-64 tanh MLPs written out instead of recorded by autograd, over
    flat parameter / gradient / Adam-moment buffers (the module's parameters become views of them),
    and nothing that waits for the host -- the whole step captures into one HIP graph.  On a GPU
    it is seven libd2d_ppo.so launches (advantage statistics, both MLPs forward with four threads per
    sample and net, loss head + backward to the hidden-layer gradients, all weight / bias gradients
    + their reduce, log_std's gradient and the statistics, clip + Adam) instead of ~190 autograd /
    optimiser kernels; on the CPU the same math in torch ops (split-K weight gradients).

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

    def __init__(self, policy: ActorCritic, cfg: PPOConfig, device):
        self.pol, self.cfg = policy, cfg
        params = list(policy.parameters())
        n = sum(p.numel() for p in params)
        self.P = torch.zeros(n, device=device)
        self.ctl = ControlBlock(device) if cfg.control else None
        if self.ctl is not None:
            # one float behind G: the minibatch KL rides in the gradient's collective (apply, world > 1)
            self.Gx = torch.zeros(n + 1, device=device)
            self.G = self.Gx[:n]
            self.set_coefs()
        else:
            self.G = torch.zeros(n, device=device)
        self.m = torch.zeros(n, device=device)
        self.v = torch.zeros(n, device=device)
        self.t = torch.zeros((), device=device)
        # the fused element-wise kernels on a GPU (libd2d_ppo.so, loud if missing); torch ops on CPU
        self.lib = ppo_native() if torch.device(device).type == "cuda" else None
        self._bufs = {}  # minibatch size -> (work buffers, partial rows) of the HIP path
        import os

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

    def step(self, idx, rollout, acc: dict, world: int = 1, adv_ws=None):
        self.grad(idx, rollout, acc, adv_ws)
        self.apply(world)

    def set_coefs(self, progress_remaining: float = 1.0):
        """Write this update's coefficients (``cfg.coefs``) into the control block."""
        self.ctl.set(*self.cfg.coefs(progress_remaining))

    def reset_control(self):
        """The first step of an update: clear the stop flag, the count and the KL sums."""
        if self.lib is not None:
            _ok(self.lib.d2d_ppo_ctl_reset(self.ctl.ptr(), self._stream()), "d2d_ppo_ctl_reset")
        else:
            self.ctl.reset()

    def grad(self, idx, rollout, acc: dict, adv_ws=None):
        """The loss gradient of minibatch ``idx`` of ``rollout`` = (obs, actions, old log-probs,
        advantages, returns[, old values: the control path]) into ``G``; statistics added to ``acc``."""
        cfg, pol = self.cfg, self.pol
        pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
        W1p, W2p, W1v, W2v = pn[0].weight, pn[2].weight, vn[0].weight, vn[2].weight
        W3p, W3v, ls = pol.action_net.weight, pol.value_net.weight, pol.log_std
        if self.ctl is not None and len(rollout) < 6:
            raise ValueError("the control path needs the rollout's stored values as rollout[5]")
        obs_all, act_all, ol_all, adv_all, ret_all = rollout[:5]
        if self.lib is not None:
            if self.fused:
                self._grad_fused(idx, rollout, acc, adv_ws)
            else:
                self._grad_hip(idx, rollout[:5], acc)
            return
        if self.ctl is not None and self.ctl.stopped():
            return
        X = obs_all[idx]
        M, c = X.shape[0], cfg.clip_range
        # forward (nn.Linear = addmm)
        h1p = torch.tanh(torch.addmm(pn[0].bias, X, W1p.t()))
        h2p = torch.tanh(torch.addmm(pn[2].bias, h1p, W2p.t()))
        mean = torch.addmm(pol.action_net.bias, h2p, W3p.t())
        h1v = torch.tanh(torch.addmm(vn[0].bias, X, W1v.t()))
        h2v = torch.tanh(torch.addmm(vn[2].bias, h1v, W2v.t()))
        V = torch.addmm(pol.value_net.bias, h2v, W3v.t()).squeeze(1)
        g_mean, g_V = self._head_torch(mean, V, act_all[idx], ol_all[idx], adv_all[idx], ret_all[idx], acc,
                                       rollout[5][idx] if self.ctl is not None else None)
        tg = self._tanh_grad_torch
        # backward: the layer-output gradients, then every weight / bias gradient
        g2p = tg(h2p, torch.mm(g_mean, W3p))
        g2v = tg(h2v, g_V[:, None] * W3v)
        g1p = tg(h1p, torch.mm(g2p, W2p))
        g1v = tg(h1v, torch.mm(g2v, W2v))
        layers = ((g_mean, h2p, pol.action_net), (g_V[:, None], h2v, pol.value_net), (g2p, h1p, pn[2]),
                  (g2v, h1v, vn[2]), (g1p, X, pn[0]), (g1v, X, vn[0]))
        for a, b, lin in layers:
            _wgrad(a, b, lin.weight.grad)
            torch.sum(a, 0, out=lin.bias.grad)

    def _grad_hip(self, idx, rollout, acc):
        """libd2d_ppo.so: advantage statistics, both MLPs forward (four threads per sample and net),
        loss head + backward to the hidden-layer gradients, all weight / bias gradients, log_std's."""
        import ctypes as C

        cfg, pol, lib, st = self.cfg, self.pol, self.lib, self._stream()
        obs_all, act_all, ol_all, adv_all, ret_all = rollout
        M, dev = idx.numel(), self.P.device
        nb = (M + 63) // 64  # D2D_PPO_HEAD_BLOCK rows per advantage partial
        if M not in self._bufs:
            # one set of work buffers per minibatch size, kept for the handle's life: a captured graph
            # holds the full-size set's addresses while a ragged last minibatch runs eagerly on its own
            e = lambda *sh: torch.empty(*sh, device=dev)  # noqa: E731
            hb = {"h1p": e(M, 64), "h2p": e(M, 64), "mean": e(M, 2), "g1p": e(M, 64), "g2p": e(M, 64),
                  "h1v": e(M, 64), "h2v": e(M, 64), "val": e(M, 1), "g1v": e(M, 64), "g2v": e(M, 64),
                  "xg": e(M, 27), "gm": e(M, 2), "gv": e(M, 1),
                  "ws": torch.zeros(nb, 2, dtype=torch.float64, device=dev)}
            prow = lib.d2d_ppo_mlp_partial_rows(M)
            hb["partial"] = torch.zeros(prow, 5, device=dev)
            hb["wpart"] = e(lib.d2d_ppo_wgrad_chunks(M) * self.G.numel())  # weight-gradient partial rows
            self._bufs[M] = (hb, prow)
        hb, prow = self._bufs[M]
        pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
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
        layers = ((hb["gm"], hb["h2p"], pol.action_net), (hb["gv"], hb["h2v"], pol.value_net),
                  (hb["g2p"], hb["h1p"], pn[2]), (hb["g2v"], hb["h1v"], vn[2]), (hb["g1p"], hb["xg"], pn[0]),
                  (hb["g1v"], hb["xg"], vn[0]))
        ls = pol.log_std
        # the head's finish (log-std gradient, loss statistics) rides on the gradient reduce's launch
        head = (prow, hb["partial"].data_ptr(), ls.data_ptr(), cfg.ent_coef, ls.grad.data_ptr(),
                acc["policy_loss"].data_ptr(), acc["value_loss"].data_ptr(), acc["entropy"].data_ptr(),
                acc["clip_fraction"].data_ptr())
        self._wgrad_hip(M, layers, hb["wpart"], head)

    def _grad_fused(self, idx, rollout, acc, adv_ws=None):
        """libd2d_ppo.so, two launches (+ the advantage statistics unless ``adv_ws`` points at this
        minibatch's precomputed d2d_ppo_adv_stats partials): d2d_ppo_fused_grad (both MLPs forward,
        the loss head, the backward and every weight / bias gradient, per-sample state on chip) and
        d2d_ppo_grad_reduce (the workgroups' rows into G, log_std's gradient, statistics)."""
        import ctypes as C

        cfg, pol, lib, st = self.cfg, self.pol, self.lib, self._stream()
        obs_all, act_all, ol_all, adv_all, ret_all = rollout[:5]
        M, dev = idx.numel(), self.P.device
        key = ("fused", M)
        if key not in self._bufs:
            rows = lib.d2d_ppo_fused_rows(M)
            nb = (M + 63) // 64
            self._bufs[key] = {"rows": rows, "wpart": torch.empty(rows * self.G.numel(), device=dev),
                               "hpart": torch.empty(2 * rows * (5 if self.ctl is None else 6), device=dev),
                               "ws": torch.zeros(nb, 2, dtype=torch.float64, device=dev)}
        b = self._bufs[key]
        pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
        base = self.G.data_ptr()
        layers = (pn[0], pn[2], pol.action_net, vn[0], vn[2], pol.value_net)
        offs = []
        for k in range(2):
            for lin in layers[3 * k:3 * k + 3]:
                offs += [(lin.weight.grad.data_ptr() - base) // 4, (lin.bias.grad.data_ptr() - base) // 4]
        offsets = (C.c_int32 * 12)(*offs)
        norm = int(cfg.normalize_advantage and M > 1)
        ws = adv_ws if adv_ws is not None else b["ws"].data_ptr()
        if norm and adv_ws is None:
            _ok(lib.d2d_ppo_adv_stats(M, idx.data_ptr(), adv_all.data_ptr(), ws, st), "d2d_ppo_adv_stats")
        ls = pol.log_std
        if self.ctl is not None:
            # the control variants: clip / clip_vf / the stop flag from the block, KL into it
            ov, ctl = rollout[5], self.ctl.ptr()
            _ok(lib.d2d_ppo_fused_grad_ctl(M, idx.data_ptr(), obs_all.data_ptr(), act_all.data_ptr(), ol_all.data_ptr(),
                                           adv_all.data_ptr(), ret_all.data_ptr(), ov.data_ptr(), ls.data_ptr(), ws,
                                           norm, cfg.vf_coef, self.weight_ptrs(), offsets, self.G.numel(),
                                           b["wpart"].data_ptr(), b["hpart"].data_ptr(), ctl, st),
                "d2d_ppo_fused_grad_ctl")
            _ok(lib.d2d_ppo_grad_reduce_ctl(b["rows"], self.G.numel(), b["wpart"].data_ptr(), base, 2 * b["rows"],
                                            b["hpart"].data_ptr(), M, ls.data_ptr(), cfg.ent_coef, ls.grad.data_ptr(),
                                            acc["policy_loss"].data_ptr(), acc["value_loss"].data_ptr(),
                                            acc["entropy"].data_ptr(), acc["clip_fraction"].data_ptr(), ctl, st),
                "d2d_ppo_grad_reduce_ctl")
            return
        _ok(lib.d2d_ppo_fused_grad(M, idx.data_ptr(), obs_all.data_ptr(), act_all.data_ptr(), ol_all.data_ptr(),
                                   adv_all.data_ptr(), ret_all.data_ptr(), pol.log_std.data_ptr(), ws,
                                   norm, cfg.clip_range, cfg.vf_coef, self.weight_ptrs(), offsets, self.G.numel(),
                                   b["wpart"].data_ptr(), b["hpart"].data_ptr(), st), "d2d_ppo_fused_grad")
        _ok(lib.d2d_ppo_grad_reduce(b["rows"], self.G.numel(), b["wpart"].data_ptr(), base, 2 * b["rows"],
                                    b["hpart"].data_ptr(), M, ls.data_ptr(), cfg.ent_coef, ls.grad.data_ptr(),
                                    acc["policy_loss"].data_ptr(), acc["value_loss"].data_ptr(),
                                    acc["entropy"].data_ptr(), acc["clip_fraction"].data_ptr(), st),
            "d2d_ppo_grad_reduce")

    def weight_ptrs(self):
        """The 12 weight / bias device pointers of include/d2d_ppo.h (policy net, then value net);
        views of the flat parameter buffer, so the addresses never change."""
        import ctypes as C

        pol = self.pol
        pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
        ws = [pn[0].weight, pn[0].bias, pn[2].weight, pn[2].bias, pol.action_net.weight, pol.action_net.bias,
              vn[0].weight, vn[0].bias, vn[2].weight, vn[2].bias, pol.value_net.weight, pol.value_net.bias]
        return (C.c_void_p * 12)(*[w.data_ptr() for w in ws])

    @staticmethod
    def _tanh_grad_torch(h, g):
        return g.mul_(1.0 - h * h)

    def _wgrad_hip(self, M, layers, wpart, head=None):
        """All six weight / bias gradients in one libd2d_ppo.so launch (+ its reduce) into G; with
        `head` (d2d_ppo_head_finish's arguments after m) the reduce launch also finishes the head."""
        import ctypes as C

        row_len = self.G.numel()  # all of G: log_std's slots (no problem covers them) are rewritten after
        assert wpart.numel() >= self.lib.d2d_ppo_wgrad_chunks(M) * row_len
        n = len(layers)
        base = self.G.data_ptr()
        arr = lambda ty, v: (ty * n)(*v)  # noqa: E731
        a_p = arr(C.c_void_p, [a.data_ptr() for a, _, _ in layers])
        b_p = arr(C.c_void_p, [b.data_ptr() for _, b, _ in layers])
        lda = arr(C.c_int32, [a.stride(0) for a, _, _ in layers])
        ldb = arr(C.c_int32, [b.stride(0) for _, b, _ in layers])
        pp = arr(C.c_int32, [a.shape[1] for a, _, _ in layers])
        qq = arr(C.c_int32, [b.shape[1] for _, b, _ in layers])
        wo = arr(C.c_int32, [(lin.weight.grad.data_ptr() - base) // 4 for _, _, lin in layers])
        bo = arr(C.c_int32, [(lin.bias.grad.data_ptr() - base) // 4 for _, _, lin in layers])
        for a, b, _ in layers:
            assert a.stride(1) == 1 and b.stride(1) == 1 and a.shape[0] == b.shape[0] == M
        if head is None:
            _ok(self.lib.d2d_ppo_wgrad(M, n, a_p, lda, b_p, ldb, pp, qq, wo, bo, row_len, wpart.data_ptr(), base,
                                       self._stream()), "d2d_ppo_wgrad")
        else:
            _ok(self.lib.d2d_ppo_wgrad_head(M, n, a_p, lda, b_p, ldb, pp, qq, wo, bo, row_len, wpart.data_ptr(), base,
                                            *head, self._stream()), "d2d_ppo_wgrad_head")

    def _stream(self):
        return torch.cuda.current_stream(self.P.device).cuda_stream

    def _head_torch(self, mean, V, A, OL, ADV, R, acc, OV=None):
        cfg, ls = self.cfg, self.pol.log_std
        M, c = mean.shape[0], cfg.clip_range
        cv = -1.0
        if self.ctl is not None:
            c, cv = self.ctl.coef[1], self.ctl.coef[2]
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
        cfg, G = self.cfg, self.G
        lr = cfg.learning_rate
        if self.ctl is not None:
            kl_last = self.ctl.buf[ControlBlock.KL_LAST:ControlBlock.KL_LAST + 1]
            if world > 1:
                self.Gx[-1:].copy_(kl_last)
                dist.all_reduce(self.Gx)
                self.Gx.div_(world)
                kl_last.copy_(self.Gx[-1:])
            if self.lib is not None:
                _ok(self.lib.d2d_ppo_adam_ctl(G.numel(), self.P.data_ptr(), G.data_ptr(), self.m.data_ptr(),
                                              self.v.data_ptr(), self.t.data_ptr(), 0.9, 0.999, 1e-5,
                                              cfg.max_grad_norm, self.ctl.ptr(), self._stream()), "d2d_ppo_adam_ctl")
                return
            if self.ctl.stopped() or self.ctl.decide():
                return
            lr = self.ctl.coef[0]
        elif world > 1:
            dist.all_reduce(G)  # data-parallel PPO: mean gradient over the ranks (RCCL)
            G.div_(world)
        if self.lib is not None:
            _ok(self.lib.d2d_ppo_adam(G.numel(), self.P.data_ptr(), G.data_ptr(), self.m.data_ptr(),
                                      self.v.data_ptr(), self.t.data_ptr(), cfg.learning_rate, 0.9, 0.999, 1e-5,
                                      cfg.max_grad_norm, self._stream()), "d2d_ppo_adam")
            return
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


def compute_gae(rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
    """SB3 ``RolloutBuffer.compute_returns_and_advantage``: tensors [T, N] (episode_starts[t] = the
    env started a new episode at step t), last_* [N]; returns (advantages, returns)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last_gae = torch.zeros_like(last_values)
    for step in reversed(range(T)):
        if step == T - 1:
            next_non_terminal = 1.0 - last_dones.to(rewards.dtype)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - episode_starts[step + 1].to(rewards.dtype)
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae = delta + gamma * gae_lambda * next_non_terminal * last_gae
        adv[step] = last_gae
    return adv, adv + values


class PPO:
    """PPO on a batched env with Drone2dVecEnv's tensor interface (``reset() -> obs``,
    ``step(actions) -> (obs, reward, terminated, truncated, info)``, ``terminal_obs``)."""

    def __init__(self, venv, config: PPOConfig | None = None, policy: ActorCritic | None = None, seed: int = 0,
                 device=None):
        self.venv = venv
        self.cfg = config or PPOConfig()
        self.seed = int(seed)
        self.device = torch.device(device) if device is not None else torch.device(venv.device)
        torch.manual_seed(seed)
        self.policy = (policy or ActorCritic()).to(self.device)
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.use_graph = bool(self.cfg.graph and self.device.type == "cuda" and self.world == 1)
        if self.world > 1:
            # one policy on every rank: rank 0's initial parameters; each rank its own noise stream
            for p in self.policy.parameters():
                dist.broadcast(p.data, 0)
        self.manual = ManualStep(self.policy, self.cfg, self.device) if self.cfg.manual else None
        self.opt = None if self.manual else torch.optim.Adam(self.policy.parameters(), lr=self.cfg.learning_rate,
                                                             eps=1e-5, capturable=self.use_graph)
        rank = dist.get_rank() if self.world > 1 else 0
        self.gen = torch.Generator(device=self.device).manual_seed(seed + 1_000_003 * rank)
        self.n_envs = int(venv.num_envs)
        self.num_timesteps = 0
        # the rollout lands in fixed buffers (a captured update reads them at fixed addresses)
        M = self.cfg.n_steps * self.n_envs
        dev = self.device
        self._flat = (torch.empty(M, 27, device=dev), torch.empty(M, 2, device=dev), torch.empty(M, device=dev),
                      torch.empty(M, device=dev), torch.empty(M, device=dev))
        z = torch.zeros((), device=dev)
        self._acc = {"policy_loss": z.clone(), "value_loss": z.clone(), "entropy": z.clone(),
                     "clip_fraction": z.clone()}
        # PPO control: SB3's progress_remaining (learn() sets it after every rollout; a caller of train()
        # may set it), and the control block -- ManualStep's, or one of this object's for the autograd
        # path -- whose tail holds the statistics, so an update's record is one transfer
        self.progress_remaining = 1.0
        self._ctl = None
        if self.cfg.control:
            self._ctl = self.manual.ctl if self.manual is not None else ControlBlock(dev)
            self._acc = self._ctl.acc()
        self._graph = None
        self._gidx = None
        self._ro = None          # rollout buffers (_alloc_rollout)
        self._ro_graph = None    # the captured rollout (GPU)
        self._ro_warm = False
        self._ro_gen = None      # the env's generation the rollout graph was captured against
        # the libd2d_ppo.so path (GPU, ManualStep): the epochs' shuffles from d2d_ppo_permute (a device
        # counter keys them, so the whole update -- shuffles and every minibatch step -- replays as one
        # HIP graph) and the rollout as one fused launch per step (d2d_ppo_rollout_step)
        self._hip = self.manual is not None and self.manual.lib is not None
        self._perm = None
        self._perm_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        self._perm_seed = (seed * 0x9E3779B97F4A7C15 + rank * 0xD1B54A32D192ED03 + 1) % (1 << 64)
        self._upd_warm = False
        self._adv_ws = None      # every minibatch's advantage-statistics partials (_train_body_hip)
        self._fused = None       # decided at the first rollout (_alloc_rollout)
        self._predict_t = 0      # predict()'s call counter: the Philox step index of its noise
        self._predict_gen = None
        self.monitor = None      # an EpisodeMonitor (set_monitor / learn(monitor=...)); None: off

    # ------------------------------------------------------------------ rollout
    def _alloc_rollout(self):
        from .env import Drone2dVecEnv

        T, N, dev = self.cfg.n_steps, self.n_envs, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        # time-limit truncations are bootstrapped with V(terminal obs); the reference never truncates
        self._truncates = bool(getattr(getattr(self.venv, "cfg", None), "timeup_truncates", 1))
        # the fused rollout: the HIP env batch, no truncation bootstrap (its extra value pass stays in torch)
        self._fused = bool(self._hip and isinstance(self.venv, Drone2dVecEnv) and not self._truncates)
        self._ro = {"val": torch.empty(T, N, device=dev), "rew": torch.empty(T, N, device=dev),
                    "done": torch.empty(T, N, dtype=torch.bool, device=dev),
                    "start0": torch.empty(N, dtype=torch.bool, device=dev),
                    "noise": torch.empty(T, N, 2, device=dev), "fin": torch.zeros((), **f64),
                    "ret": torch.zeros((), **f64)}
        if self._fused:
            self._ro["act_env"] = torch.empty(N, 2, device=dev)
            self._ro["stats"] = torch.zeros(T, (N + 63) // 64, 2, **f64)
            self._ro["obs_cur"] = None
        else:
            self._ro.update(obs=torch.empty(T + 1, N, 27, device=dev), act=torch.empty(T, N, 2, device=dev),
                            logp=torch.empty(T, N, device=dev))

    def _set_first_obs(self, obs):
        if self._fused:
            self._ro["obs_cur"] = obs  # the env's output tensor; the fused step reads it in place
        else:
            self._ro["obs"][0].copy_(obs.to(self.device))
        self._ro["start0"].fill_(True)

    def set_monitor(self, monitor=True):
        """Attach an ``EpisodeMonitor`` (``True``: a new one for the env batch) or detach it (``None`` /
        ``False``).  The rollout then digests every env step's outputs with one ``monitor.step`` and ends
        with one ``monitor.flush``; the record gains ``monitor/*`` and ``train/explained_variance``.  A
        monitor attached to a batch in mid-flight (after ``PPO.load``, or between two ``learn`` calls)
        starts with ``live=0``: the episodes under way are counted as skipped, not logged with partial
        sums.  A captured rollout is dropped and captured again on the usual schedule."""
        if monitor is True:
            if self.monitor is not None:
                return self.monitor
            from .monitor import EpisodeMonitor

            monitor = EpisodeMonitor(self.venv, getattr(self.venv, "device", self.device))
        elif monitor is False:
            monitor = None
        if monitor is self.monitor:
            return monitor
        if monitor is not None and monitor.n != self.n_envs:
            raise ValueError(f"the monitor is for {monitor.n} envs, the batch has {self.n_envs}")
        self.monitor = monitor
        self._ro_graph = None
        self._ro_warm = False
        if monitor is not None and self._ro is not None:
            monitor.reset(live=False)  # (a fresh run resets it with the envs, in collect_rollouts)
        return monitor

    def _reset_envs(self):
        obs = self.venv.reset()
        if self.monitor is not None:
            self.monitor.reset()
        return obs

    @torch.no_grad()
    def _rollout_body_fused(self):
        """_rollout_body as T + 1 libd2d_ppo.so launches around the T env steps: step t's launch runs
        both MLPs on the env's observation tensor, samples and stores the action, log-density and
        value, copies the observations into the flat buffer and records step t-1's reward / done /
        episode statistics; the last one adds the bootstrap value and GAE (d2d_ppo_rollout_step)."""
        import ctypes as C

        from . import abi

        R, T, N, lib = self._ro, self.cfg.n_steps, self.n_envs, self.manual.lib
        st = self.manual._stream()
        wptr = self.manual.weight_ptrs()
        obs_buf, act_buf, logp_buf, adv_buf, ret_buf = self._flat
        ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
        r = D2DPPORollout(n=N, T=T, info_dim=abi.INFO_DIM, info_totrew=abi.INFO_TOTREW, gamma=self.cfg.gamma,
                          gae_lambda_gamma=self.cfg.gamma * self.cfg.gae_lambda,
                          log_std=ptr(self.policy.log_std), obs_buf=ptr(obs_buf), act_buf=ptr(act_buf),
                          logp_buf=ptr(logp_buf), val_buf=ptr(R["val"]), rew_buf=ptr(R["rew"]),
                          done_buf=ptr(R["done"]), start0=ptr(R["start0"]), act_env=ptr(R["act_env"]),
                          adv_buf=ptr(adv_buf), ret_buf=ptr(ret_buf), stats=ptr(R["stats"]))
        obs = R["obs_cur"]
        for t in range(T + 1):
            r.t = t
            r.obs = ptr(obs)
            r.noise = ptr(R["noise"][t]) if t < T else None
            _ok(lib.d2d_ppo_rollout_step(C.byref(r), wptr, st), "d2d_ppo_rollout_step")
            if t < T:
                obs, rew, term, trunc, info = self.venv.step(R["act_env"])
                if self.monitor is not None:
                    self.monitor.step(term, trunc, info)
                r.prev_rew, r.prev_term, r.prev_trunc, r.prev_info = ptr(rew), ptr(term), ptr(trunc), ptr(info)
        if self.monitor is not None:
            self.monitor.flush()
        R["obs_cur"] = obs  # T even: the same double-buffer slot as at the start
        R["fin"].copy_(R["stats"][..., 0].sum())
        R["ret"].copy_(R["stats"][..., 1].sum())

    @torch.no_grad()
    def _rollout_body(self):
        """n_steps policy + env steps into the rollout buffers, then GAE into the flat buffers.
        Reads obs[0], start0 and noise; leaves the next rollout's obs[0] / start0 in place.  No host
        synchronisation: on a GPU the whole body is one captured HIP graph."""
        from . import abi

        R, pol, T, dev = self._ro, self.policy, self.cfg.n_steps, self.device
        std = pol.log_std.exp()
        for t in range(T):
            mean, value = pol(R["obs"][t])
            actions = mean + std * R["noise"][t]
            logp = pol.log_prob(mean, actions)
            # SB3 clips to the Box bounds for the env only; the buffer keeps the unclipped action
            new_obs, rew, term, trunc, info = self.venv.step(actions.clamp(-1.0, 1.0))
            if self.monitor is not None:
                self.monitor.step(term, trunc, info)
            rew = rew.to(dev).float()
            trunc = trunc.to(dev)
            done = term.to(dev) | trunc
            if self._truncates:
                tv = pol.predict_values(self.venv.terminal_obs.to(dev))
                rew = torch.where(trunc, rew + self.cfg.gamma * tv, rew)
            R["obs"][t + 1].copy_(new_obs)
            R["act"][t].copy_(actions)
            R["logp"][t].copy_(logp)
            R["val"][t].copy_(value)
            R["rew"][t].copy_(rew)
            R["done"][t].copy_(done)
            if info is not None:
                R["fin"] += done.sum()
                R["ret"] += torch.where(done, info[:, abi.INFO_TOTREW].to(dev).double(), 0.0).sum()
        last_values = pol.predict_values(R["obs"][T])
        starts = torch.cat([R["start0"][None], R["done"][:-1]])
        adv, ret = compute_gae(R["rew"], R["val"], starts, last_values, R["done"][T - 1], self.cfg.gamma,
                               self.cfg.gae_lambda)
        N = self.n_envs
        for dst, src in zip(self._flat, (R["obs"][:T].reshape(T * N, 27), R["act"].reshape(T * N, 2),
                                         R["logp"].reshape(-1), adv.reshape(-1), ret.reshape(-1))):
            dst.copy_(src)
        R["obs"][0].copy_(R["obs"][T])
        R["start0"].copy_(R["done"][T - 1])
        if self.monitor is not None:
            self.monitor.flush()

    def collect_rollouts(self) -> dict:
        T, N = self.cfg.n_steps, self.n_envs
        gen = getattr(self.venv, "generation", None)
        if self._ro is not None and gen != self._ro_gen:
            # the env re-allocated its scenario tables (set_curriculum / set_scenarios): a captured
            # rollout would replay against freed memory, and the envs were reset -- drop the graph
            # and start the next rollout from a reset
            self._ro_graph = None
            self._ro_warm = False
            self._set_first_obs(self._reset_envs())
        self._ro_gen = gen
        if self._ro is None:
            self._alloc_rollout()
            self._set_first_obs(self._reset_envs())
        R = self._ro
        body = self._rollout_body_fused if self._fused else self._rollout_body
        R["fin"].zero_()
        R["ret"].zero_()
        torch.randn(R["noise"].shape, generator=self.gen, device=self.device, out=R["noise"])
        # capture only whole fill periods: d2d_step launches the reset-cache fill after every 16th
        # step, decided on the host, so a graph of another length would bake in a fill on every
        # replay or on none (still correct through the synchronous reset path, but slower)
        graph_ok = self.cfg.graph and self.device.type == "cuda" and T % 16 == 0
        if graph_ok and self._ro_graph is None and self._ro_warm:
            # second rollout: capture (the first one ran eagerly: library and allocator warm-up);
            # T even, so the env's double-buffered outputs are back at their start after a replay
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            self._ro_graph = g
        if self._ro_graph is not None:
            self._ro_graph.replay()
        else:
            body()
            self._ro_warm = True
        self.num_timesteps += T * N
        if self.monitor is None:
            f, r = float(R["fin"]), float(R["ret"])
            return {"episodes": f, "mean_return": r / f if f else float("nan")}
        # fin, ret, the explained variance and the flushed vector packed on the device and read with
        # one copy, where fin and ret were read before
        ev = self._explained_variance().to(torch.float64)
        host = torch.cat([R["fin"].reshape(1), R["ret"].reshape(1), ev.reshape(1),
                          self.monitor.out.to(self.device)]).cpu()
        f, r = float(host[0]), float(host[1])
        out = {"episodes": f, "mean_return": r / f if f else float("nan")}
        out.update({"monitor/" + k: v for k, v in self.monitor.scalars(host[3:]).items()})
        out["train/explained_variance"] = float(host[2])
        return out

    @torch.no_grad()
    def _explained_variance(self) -> torch.Tensor:
        """SB3's ``explained_variance(values, returns)`` over the rollout buffer, before the update:
        1 - Var(returns - values) / Var(returns) (NaN when the returns do not vary)."""
        val, ret = self._ro["val"].reshape(-1), self._flat[4]
        var_y = torch.var(ret, unbiased=False)
        return torch.where(var_y == 0, torch.full_like(var_y, float("nan")),
                           1.0 - torch.var(ret - val, unbiased=False) / var_y)

    # ------------------------------------------------------------------ update
    def _minibatch(self, idx: torch.Tensor, zero_grad: bool = True, adv_ws=None):
        """One SB3 PPO gradient step on rollout samples ``idx`` (statistics accumulated on device)."""
        obs, act, old_logp, adv_all, ret = self._flat
        if self.manual is not None:
            with torch.no_grad():
                self.manual.step(idx, self._rollout_data(), self._acc, self.world, adv_ws)
            return
        if self._ctl is not None:
            self._minibatch_control(idx)
            return
        c = self.cfg.clip_range
        params = list(self.policy.parameters())
        values, logp, entropy = self.policy.evaluate_actions(obs[idx], act[idx])
        adv = adv_all[idx]
        if self.cfg.normalize_advantage and idx.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(logp - old_logp[idx])
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
        vl = torch.nn.functional.mse_loss(ret[idx], values)
        el = -entropy.mean()
        loss = pl + self.cfg.ent_coef * el + self.cfg.vf_coef * vl
        if zero_grad:
            self.opt.zero_grad(set_to_none=False)
        loss.backward()
        if self.world > 1:
            # data-parallel PPO: average the gradients over the ranks (RCCL all-reduce)
            flat = torch.cat([p.grad.reshape(-1) for p in params])
            dist.all_reduce(flat)
            flat /= self.world
            o = 0
            for p in params:
                k = p.numel()
                p.grad.copy_(flat[o:o + k].view_as(p))
                o += k
        torch.nn.utils.clip_grad_norm_(params, self.cfg.max_grad_norm)
        self.opt.step()
        with torch.no_grad():
            self._acc["policy_loss"] += pl
            self._acc["value_loss"] += vl
            self._acc["entropy"] -= el
            self._acc["clip_fraction"] += ((ratio - 1).abs() > c).float().mean()

    def _rollout_data(self) -> tuple:
        """ManualStep's rollout tuple; on the control path with the rollout's stored values (SB3's
        ``old_values``: the buffer the rollout wrote, in the flat buffers' sample order)."""
        if self._ctl is None:
            return self._flat
        return self._flat + (self._ro["val"].reshape(-1),)

    def _minibatch_control(self, idx: torch.Tensor):
        """``_minibatch``'s autograd branch on the control path, in SB3 ``PPO.train``'s order: loss (with
        ``clip_range_vf``), statistics, approx_kl, the target_kl check, and only then the step.  The
        backward pass runs before the check, so that a multi-rank run can send the KL behind the
        gradients in their one collective; a stopped minibatch's gradients are simply not applied."""
        ctl = self._ctl
        if ctl.stopped():
            return
        _, c, cv, _ = ctl.coef
        obs, act, old_logp, adv_all, ret = self._flat
        params = list(self.policy.parameters())
        values, logp, entropy = self.policy.evaluate_actions(obs[idx], act[idx])
        adv = adv_all[idx]
        if self.cfg.normalize_advantage and idx.numel() > 1:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        log_ratio = logp - old_logp[idx]
        ratio = torch.exp(log_ratio)
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - c, 1 + c)).mean()
        if cv >= 0.0:
            ov = self._ro["val"].reshape(-1)[idx]
            values = ov + torch.clamp(values - ov, -cv, cv)
        vl = torch.nn.functional.mse_loss(ret[idx], values)
        el = -entropy.mean()
        loss = pl + self.cfg.ent_coef * el + self.cfg.vf_coef * vl
        self.opt.zero_grad(set_to_none=False)
        loss.backward()
        with torch.no_grad():
            self._acc["policy_loss"] += pl
            self._acc["value_loss"] += vl
            self._acc["entropy"] -= el
            self._acc["clip_fraction"] += ((ratio - 1).abs() > c).float().mean()
            ctl.record(((ratio - 1) - log_ratio).mean())
            if self.world > 1:
                kl_last = ctl.buf[ControlBlock.KL_LAST:ControlBlock.KL_LAST + 1]
                flat = torch.cat([p.grad.reshape(-1) for p in params] + [kl_last])
                dist.all_reduce(flat)
                flat /= self.world
                o = 0
                for p in params:
                    k = p.numel()
                    p.grad.copy_(flat[o:o + k].view_as(p))
                    o += k
                kl_last.copy_(flat[o:])
        if ctl.decide():
            return
        torch.nn.utils.clip_grad_norm_(params, self.cfg.max_grad_norm)
        self.opt.step()

    def _capture(self):
        """Record one full-size minibatch step as a HIP graph: forward, backward, grad clipping and
        the (capturable) Adam step replay with no per-kernel launches from Python."""
        bs = self.cfg.batch_size
        self._gidx = torch.zeros(bs, dtype=torch.long, device=self.device)
        saved = {k: v.clone() for k, v in self._acc.items()}
        if self.opt is not None:
            self.opt.zero_grad(set_to_none=True)  # backward inside the capture writes fresh gradients
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._minibatch(self._gidx, zero_grad=False)
        for k, v in saved.items():  # capture does not execute: nothing to undo, but keep the sums exact
            self._acc[k].copy_(v)
        self._graph = g

    def _train_body_hip(self):
        """One update on the libd2d_ppo.so path: the n_epochs shuffles in one launch
        (d2d_ppo_permute), then every minibatch step; nothing waits for the host, so on one rank the
        whole update is captured and replayed as one HIP graph."""
        M, bs, E = self._flat[0].shape[0], self.cfg.batch_size, self.cfg.n_epochs
        if self._ctl is not None:
            self.manual.reset_control()  # the update's first node
        for v in self._acc.values():
            v.zero_()
        lib, st = self.manual.lib, self.manual._stream()
        _ok(lib.d2d_ppo_permute(M, E, self._perm_seed, self._perm_ctr.data_ptr(), self._perm.data_ptr(), st),
            "d2d_ppo_permute")
        # the advantage statistics of every minibatch of the update in one launch: 64-row partials over
        # the whole shuffle; minibatch boundaries fall on partial boundaries when M and bs are multiples
        # of 64, so each minibatch reads its own slice (otherwise each minibatch computes its own)
        ws = None
        if self.manual.fused and self.cfg.normalize_advantage and M % 64 == 0 and bs % 64 == 0:
            if self._adv_ws is None:
                self._adv_ws = torch.zeros(E * M // 64, 2, dtype=torch.float64, device=self.device)
            _ok(lib.d2d_ppo_adv_stats(E * M, self._perm.data_ptr(), self._flat[3].data_ptr(),
                                      self._adv_ws.data_ptr(), st), "d2d_ppo_adv_stats")
            ws = self._adv_ws
        for e in range(E):
            for s in range(0, M, bs):
                n = min(s + bs, M) - s
                aw = ws[(e * M + s) // 64:].data_ptr() if (ws is not None and n > 1) else None
                self._minibatch(self._perm[e * M + s:e * M + s + n], adv_ws=aw)

    def train(self) -> dict:
        """One update on the last rollout.  On the control path (``cfg.control``) the coefficients of
        ``cfg.coefs(self.progress_remaining)`` are written to the control block first -- one small copy,
        outside the captured graph, which reads them from memory on every replay -- and the record
        gains ``approx_kl``, ``n_minibatches``, ``early_stop``, ``learning_rate``, ``clip_range`` and
        (when on) ``clip_range_vf``; the four means are over the recorded minibatches."""
        M, bs = self._flat[0].shape[0], self.cfg.batch_size
        ctl = self._ctl
        if ctl is not None:
            ctl.set(*self.cfg.coefs(self.progress_remaining))
            if self.opt is not None:
                for grp in self.opt.param_groups:
                    grp["lr"] = ctl.coef[0]
        if self._hip:
            if self._perm is None:
                self._perm = torch.empty(self.cfg.n_epochs * M, dtype=torch.int64, device=self.device)
            if self.use_graph and self._graph is None and self._upd_warm:
                # second update: capture the whole update (the first ran eagerly: kernels loaded, every
                # minibatch size's work buffers allocated)
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._train_body_hip()
                self._graph = g
            if self._graph is not None:
                self._graph.replay()
            else:
                self._train_body_hip()
                self._upd_warm = True
            if ctl is not None:
                return ctl.read()  # the statistics and the counters in one transfer
            n_upd = self.cfg.n_epochs * -(-M // bs)
            return {k: float(v) / n_upd for k, v in self._acc.items()}
        if ctl is not None:
            ctl.reset()
        for v in self._acc.values():
            v.zero_()
        n_upd = 0
        warm = 0
        for _ in range(self.cfg.n_epochs):
            # (a stopped update still draws every epoch's shuffle: the generator's state after an
            # update does not depend on whether it stopped)
            perm = torch.randperm(M, device=self.device, generator=self.gen)
            for s in range(0, M, bs):
                if ctl is not None and ctl.stopped():
                    break
                idx = perm[s:s + bs]
                if self.use_graph and idx.numel() == bs and ctl is None:
                    if self._graph is None and warm >= 3:
                        # capture after a few eager steps (lazy optimiser state, allocator warm-up)
                        torch.cuda.synchronize(self.device)
                        self._capture()
                    if self._graph is not None:
                        self._gidx.copy_(idx)
                        self._graph.replay()
                        n_upd += 1
                        continue
                    warm += 1
                self._minibatch(idx)
                n_upd += 1
        if ctl is not None:
            return ctl.read()
        return {k: float(v) / max(n_upd, 1) for k, v in self._acc.items()}

    def learn(self, total_timesteps: int, log=None, checkpoint: Checkpoint | None = None, monitor=None,
              logger=None, schedule_timesteps: int | None = None) -> list[dict]:
        """Alternate rollouts and updates until ``total_timesteps`` env steps (this rank);
        ``checkpoint``: save the agent whenever ``num_timesteps`` crosses a multiple of its
        ``save_freq`` (after the update, so a resumed run continues with the next rollout).
        ``monitor``: ``True`` or an ``EpisodeMonitor`` -- ``set_monitor`` it first (``None``: leave
        things as they are; off unless one was set).  ``logger``: a ``trainlog.ScalarLog`` (anything
        with ``log(record)``) that gets every record after ``log``.  After each rollout and before its
        update, ``progress_remaining = 1 - num_timesteps / total_timesteps`` (SB3's
        ``OnPolicyAlgorithm.learn``; not below 0 when the last rollout overshoots), which the schedules
        ``learning_rate_end`` / ``clip_range_end`` read; ``schedule_timesteps``: the schedule's horizon
        when it is not this call's ``total_timesteps`` (a run driven by several ``learn`` calls)."""
        horizon = float(schedule_timesteps if schedule_timesteps is not None else total_timesteps)
        if monitor is not None:
            self.set_monitor(monitor)
        hist = []
        while self.num_timesteps < total_timesteps:
            before = self.num_timesteps
            t0 = time.perf_counter()
            ro = self.collect_rollouts()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            t1 = time.perf_counter()
            self.progress_remaining = max(0.0, 1.0 - self.num_timesteps / horizon)
            tr = self.train()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            t2 = time.perf_counter()
            rec = dict(ro, **tr, timesteps=self.num_timesteps, rollout_s=t1 - t0, train_s=t2 - t1,
                       env_steps_per_s=self.cfg.n_steps * self.n_envs / (t2 - t0))
            hist.append(rec)
            if log:
                log(rec)
            if logger is not None:
                logger.log(rec)
            if checkpoint is not None and self.num_timesteps // checkpoint.save_freq > before // checkpoint.save_freq:
                os.makedirs(checkpoint.save_path, exist_ok=True)
                self.save(os.path.join(checkpoint.save_path,
                                       f"{checkpoint.name_prefix}_{self.num_timesteps}_steps.zip"))
        return hist

    # ------------------------------------------------------------------ predict / save / load
    @torch.no_grad()
    def predict(self, obs, deterministic: bool = False) -> torch.Tensor:
        """The clipped actions for ``obs`` [n, 27] (SB3 ``model.predict``; stochastic by default, as the
        reference calls it).  On a HIP device the evaluation library's act half (``evaluate.act``): call
        k's noise for row i is the Philox draw of (seed, i, k); on the CPU the same in torch."""
        x = torch.as_tensor(obs, dtype=torch.float32).to(self.device).reshape(-1, 27)
        if self.device.type == "cuda":
            from . import evaluate

            a = evaluate.act(self.policy, x, deterministic=deterministic, seed=self.seed, t=self._predict_t)
        else:
            a = self.policy(x)[0]
            if not deterministic:
                if self._predict_gen is None:
                    self._predict_gen = torch.Generator(device=self.device).manual_seed(self.seed + 7)
                a = a + self.policy.log_std.exp() * torch.randn(a.shape, generator=self._predict_gen)
            a = a.clamp(-1.0, 1.0)
        if not deterministic:
            self._predict_t += 1
        return a

    def _train_state(self) -> dict:
        ts = {"gen": self.gen.get_state(), "perm_ctr": self._perm_ctr}
        if self.manual is not None:
            ts.update(m=self.manual.m, v=self.manual.v, t=self.manual.t)
        else:
            ts["opt"] = self.opt.state_dict()
        if self._ro is not None:
            ts["last_obs"] = self._ro["obs_cur"] if self._fused else self._ro["obs"][0]
            ts["start0"] = self._ro["start0"]
        return _to_tensors(ts)

    def save(self, path: str) -> str:
        """Write the agent as a zip laid out like SB3's: ``policy.pth`` (the policy's state_dict under
        SB3's names), ``train_state.pth`` (Adam moments and step counter, the rollout noise generator,
        the shuffle counter, the rollout's carried observations and episode starts), ``env_state.pth``
        (``venv.state_dict()``, when the batch has one) and ``data.json`` (format version, PPOConfig,
        num_timesteps, n_envs, seed).  Tensors and JSON only."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        members = {"policy.pth": _to_tensors(dict(self.policy.state_dict())), "train_state.pth": self._train_state()}
        if hasattr(self.venv, "state_dict"):
            members["env_state.pth"] = _to_tensors(self.venv.state_dict())
        data = {"format_version": AGENT_FORMAT_VERSION, "config": dataclasses.asdict(self.cfg),
                "num_timesteps": int(self.num_timesteps), "n_envs": self.n_envs, "seed": self.seed}
        d = os.path.dirname(os.path.abspath(path))
        os.makedirs(d, exist_ok=True)
        tmp = path + ".part"
        with zipfile.ZipFile(tmp, "w", zipfile.ZIP_STORED) as z:
            z.writestr("data.json", json.dumps(data, indent=1))
            for name, obj in members.items():
                buf = io.BytesIO()
                torch.save(obj, buf)
                z.writestr(name, buf.getvalue())
        os.replace(tmp, path)
        return path

    @classmethod
    def load(cls, path: str, venv, device=None, restore_env: bool = True) -> "PPO":
        """The agent of ``save``'s file on ``venv``, ready to go on learning where the saved run
        stopped: policy, optimiser state, noise generator and shuffle counter, ``num_timesteps``, the env
        batch's state (``restore_env``, when the file has one and ``venv`` can take it) and the
        rollout's carried observations, so the next ``collect_rollouts`` continues the running episodes
        instead of resetting them.  The first rollout and update after a load run eagerly and the HIP
        graphs are captured again on the usual schedule (a captured rollout reads the env's own
        observation tensor at a fixed address, which the restored observations are not in)."""
        with zipfile.ZipFile(path) as z:
            names = set(z.namelist())
            data = json.loads(z.read("data.json"))
            if data.get("format_version") != AGENT_FORMAT_VERSION:
                raise ValueError(f"{path}: agent format {data.get('format_version')}, expected {AGENT_FORMAT_VERSION}")
            policy_sd = _zip_tensors(z, "policy.pth")
            ts = _zip_tensors(z, "train_state.pth")
            env_sd = _zip_tensors(z, "env_state.pth") if "env_state.pth" in names else None
        if int(venv.num_envs) != int(data["n_envs"]):
            raise ValueError(f"{path}: saved with {data['n_envs']} envs, the batch has {venv.num_envs}")
        algo = cls(venv, PPOConfig(**data["config"]), seed=int(data["seed"]), device=device)
        algo.policy.load_state_dict(policy_sd)  # in place: ManualStep's flat buffer holds the parameters
        if algo.manual is not None:
            if "m" not in ts:
                raise ValueError(f"{path}: saved with the torch optimiser, config.manual says ManualStep")
            algo.manual.m.copy_(ts["m"])
            algo.manual.v.copy_(ts["v"])
            algo.manual.t.copy_(ts["t"])
        else:
            algo.opt.load_state_dict(ts["opt"])
        algo.gen.set_state(ts["gen"])
        algo._perm_ctr.copy_(ts["perm_ctr"])
        algo.num_timesteps = int(data["num_timesteps"])
        if restore_env and env_sd is not None and hasattr(venv, "load_state_dict"):
            venv.load_state_dict(_to_arrays(env_sd))
        if "last_obs" in ts:
            algo._alloc_rollout()
            last_obs = ts["last_obs"].to(algo.device)
            if algo._fused:
                algo._ro["obs_cur"] = last_obs.contiguous()
            else:
                algo._ro["obs"][0].copy_(last_obs)
            algo._ro["start0"].copy_(ts["start0"])
            # collect_rollouts resets the envs when the batch's generation is not the one it last saw
            algo._ro_gen = getattr(venv, "generation", None)
        return algo


__all__ = ["PPOConfig", "Checkpoint", "ActorCritic", "ManualStep", "PPO", "compute_gae"]
