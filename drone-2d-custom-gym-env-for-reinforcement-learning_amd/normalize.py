"""Reward normalisation in the rollout: the reward half of Stable-Baselines3 2.1's
``VecNormalize(venv, norm_obs=False, norm_reward=True, gamma=...)`` -- a discounted return per env, a
``RunningMeanStd`` of those returns, every reward divided by the running standard deviation and clipped
-- done on the device by ``libd2d_norm.so`` (include/d2d_norm.h) with one call per env step.

``RewardNormalizer.step`` takes a step's ``rew`` / ``term`` / ``trunc`` and returns the normalised
rewards.  On HIP tensors every call goes to the library (a missing library is an error, there is no
fallback); on CPU tensors (the oracle backend of the tests) the same arithmetic runs in
``reward_norm_host``, a NumPy twin that evaluates the header's expressions and adds in the header's
order, so both give the same bits on finite inputs.  Observations are not normalised (the env already
maps them into Box(-1, 1); DESIGN.md "Out of scope").
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

ABI_VERSION = 1
CHUNK = 256
MAX_BLOCKS = 1024
RMS_INIT = (0.0, 1.0, 1e-4)  # SB3 RunningMeanStd(epsilon=1e-4): mean, var, count
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_norm.so")

_VP = C.c_void_p
_I32 = C.c_int32


class D2DNormStepArgs(C.Structure):
    """include/d2d_norm.h ``d2d_norm_step_args``."""
    _fields_ = [(k, _I32) for k in ("n", "n_blocks", "training", "pad")] + \
               [(k, C.c_double) for k in ("gamma", "clip", "epsilon")] + \
               [(k, _VP) for k in ("rew", "term", "trunc", "rew_out", "ret", "rms", "part", "ticket")]


class NormError(RuntimeError):
    pass


SIGNATURES = {
    "d2d_norm_abi_version": (_I32, []),
    "d2d_norm_step": (_I32, [C.POINTER(D2DNormStepArgs), _VP]),
    "d2d_norm_reset": (_I32, [_I32, _VP, _VP, _VP]),
}

_lib = None


def bind(path: str) -> C.CDLL:
    """The library at ``path`` with its signatures set and its ABI version checked."""
    from . import _native

    return _native.bind(path, SIGNATURES, "d2d_norm_abi_version", ABI_VERSION, NormError)


def load() -> C.CDLL:
    """Load (once) the normalisation library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            from ._build import build_norm

            build_norm()
        _lib = bind(LIB_PATH)
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc:
        raise NormError(f"{what}: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


def default_blocks(n: int) -> int:
    return max(1, min((int(n) + CHUNK - 1) // CHUNK, MAX_BLOCKS))


# ---------------------------------------------------------------------------------------------- host twin
def chunk_sums(d: np.ndarray) -> np.ndarray:
    """The header's chunk sums of ``d`` [n] float64: envs padded with +0.0 to whole chunks, the
    shuffle-down tree inside every wave, then waves 0, 1, 2, 3 in order.  Returns [chunks]."""
    n = d.shape[0]
    chunks = (n - 1) // CHUNK + 1
    v = np.zeros(chunks * CHUNK, np.float64)
    v[:n] = d
    v = v.reshape(chunks, CHUNK // 64, 64)
    for s in (32, 16, 8, 4, 2, 1):
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
    w = v[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def fold_sums(cs: np.ndarray, n_blocks: int) -> np.float64:
    """Workgroup b adds chunks b, b + n_blocks, ... to its row in walk order from +0.0; the fold adds
    the rows in ascending order from +0.0."""
    part = np.zeros(n_blocks, np.float64)
    for k in range(0, len(cs), n_blocks):
        seg = cs[k:k + n_blocks]
        part[:len(seg)] = part[:len(seg)] + seg
    s = np.float64(0.0)
    for b in range(n_blocks):
        s = s + part[b]
    return s


def reward_norm_host(rew, term, trunc, ret: np.ndarray, rms: np.ndarray, gamma: float, clip: float = 10.0,
                     epsilon: float = 1e-8, n_blocks: int | None = None, training: bool = True) -> np.ndarray:
    """``d2d_norm_step`` on NumPy arrays: ``ret`` [n] and ``rms`` [3] float64 updated in place (left alone
    with ``training=False``), the normalised rewards [n] float32 returned.  The same expressions in the
    same order as include/d2d_norm.h, each one IEEE operation at a time."""
    f8 = np.float64
    rew = np.asarray(rew, np.float32)
    n = rew.shape[0]
    if ret.shape != (n,) or rms.shape != (3,) or ret.dtype != f8 or rms.dtype != f8:
        raise ValueError("ret must be [n] and rms [3], float64")
    n_blocks = default_blocks(n) if n_blocks is None else int(n_blocks)
    if n < 1 or not 1 <= n_blocks <= MAX_BLOCKS:
        raise ValueError("need n >= 1 and 1 <= n_blocks <= 1024")
    gamma, clip, epsilon = f8(gamma), f8(clip), f8(epsilon)
    r64 = rew.astype(f8)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        var = rms[1]
        if training:
            ret[:] = ret * gamma + r64
            mean, count = rms[0], rms[2]
            d = ret - mean
            S1, S2 = fold_sums(chunk_sums(d), n_blocks), fold_sums(chunk_sums(d * d), n_blocks)
            nn = f8(n)
            bm = S1 / nn
            bv = S2 / nn - bm * bm
            if bv < 0.0:
                bv = f8(0.0)
            tot = count + nn
            M2 = var * count + bv * nn + bm * bm * count * nn / tot
            mean = mean + bm * nn / tot
            var = M2 / tot
            rms[:] = (mean, var, tot)
        x = r64 / np.sqrt(var + epsilon)
        x = np.where(x < -clip, -clip, x)
        x = np.where(x > clip, clip, x)
        out = x.astype(np.float32)
    if training:
        done = (np.asarray(term).astype(np.uint8) | np.asarray(trunc).astype(np.uint8)) != 0
        ret[done] = 0.0
    return out


# ---------------------------------------------------------------------------------------- the normaliser
class RewardNormalizer:
    """SB3's ``VecNormalize(norm_obs=False, norm_reward=True, gamma=gamma, clip_reward=clip,
    epsilon=epsilon)`` for a batch of ``n`` envs (``venv_or_n``: the batch, or n) on ``device`` (default:
    the batch's), with ``n_blocks`` workgroups (default: one per 256 envs, at most 1 024).  ``training``
    (default True): update the statistics with every step; False: scale with the stored ones."""

    def __init__(self, venv_or_n, gamma: float, clip: float = 10.0, epsilon: float = 1e-8, device=None,
                 n_blocks: int | None = None):
        n = venv_or_n if isinstance(venv_or_n, (int, np.integer)) else venv_or_n.num_envs
        if device is None:
            device = getattr(venv_or_n, "device", "cpu")
        self.n = int(n)
        self.gamma, self.clip, self.epsilon = float(gamma), float(clip), float(epsilon)
        self.device = torch.device(device)
        self.n_blocks = default_blocks(self.n) if n_blocks is None else int(n_blocks)
        if self.n < 1 or not 1 <= self.n_blocks <= MAX_BLOCKS:
            raise ValueError("need n >= 1 and 1 <= n_blocks <= 1024")
        if not (self.clip >= 0.0 and self.epsilon >= 0.0 and self.gamma == self.gamma):
            raise ValueError("need clip >= 0, epsilon >= 0 and a gamma that is a number")
        self.training = True
        self.hip = self.device.type == "cuda"
        if self.hip and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self.ret = torch.zeros(self.n, dtype=torch.float64, device=dev)
        self.rms = torch.tensor(RMS_INIT, dtype=torch.float64, device=dev)
        if self.hip:
            self._lib = load()
            self.part = torch.zeros(self.n_blocks, 2, dtype=torch.float64, device=dev)
            self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
            self.out = torch.zeros(self.n, dtype=torch.float32, device=dev)
            self._args = D2DNormStepArgs(n=self.n, n_blocks=self.n_blocks, rew_out=self.out.data_ptr(),
                                         ret=self.ret.data_ptr(), rms=self.rms.data_ptr(),
                                         part=self.part.data_ptr(), ticket=self.ticket.data_ptr())

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def step(self, rew: torch.Tensor, term: torch.Tensor, trunc: torch.Tensor) -> torch.Tensor:
        """One env step's rewards [n] float32 normalised (``term`` / ``trunc`` [n] bool or uint8 end the
        envs' discounted returns).  On a HIP device the result is the normaliser's own ``out`` tensor,
        rewritten by the next step; the call is stream-ordered and waits for nothing."""
        if not self.hip:
            if rew.is_cuda or term.is_cuda:
                raise ValueError("a CPU normaliser was handed HIP tensors")
            out = reward_norm_host(rew.detach().numpy(), term.numpy(), trunc.numpy(), self.ret.numpy(), self.rms.numpy(),
                                   self.gamma, self.clip, self.epsilon, self.n_blocks, self.training)
            return torch.from_numpy(out)
        if rew.device != self.device or rew.dtype != torch.float32 or rew.numel() != self.n or not rew.is_contiguous():
            raise ValueError(f"rew must be a contiguous float32 [n] tensor on {self.device}")
        for t, nm in ((term, "term"), (trunc, "trunc")):
            if t.device != self.device or t.element_size() != 1 or t.numel() != self.n or not t.is_contiguous():
                raise ValueError(f"{nm} must be a contiguous one-byte [n] tensor on {self.device}")
        a = self._args
        a.training = 1 if self.training else 0
        a.gamma, a.clip, a.epsilon = self.gamma, self.clip, self.epsilon
        a.rew, a.term, a.trunc = rew.data_ptr(), term.data_ptr(), trunc.data_ptr()
        _ok(self._lib.d2d_norm_step(C.byref(a), self._stream()), "d2d_norm_step")
        return self.out

    def reset(self, stats: bool = False) -> None:
        """The envs were reset: their discounted returns start over.  ``stats=True`` also puts the
        running statistics back to SB3's start, (mean, var, count) = (0, 1, 1e-4)."""
        if self.hip:
            _ok(self._lib.d2d_norm_reset(self.n, self.ret.data_ptr(), self.rms.data_ptr() if stats else None,
                                         self._stream()), "d2d_norm_reset")
        else:
            self.ret.zero_()
            if stats:
                self.rms.copy_(torch.tensor(RMS_INIT, dtype=torch.float64))

    def scale(self) -> torch.Tensor:
        """sqrt(var + epsilon), what ``training=False`` divides by: a scalar tensor on the device."""
        return torch.sqrt(self.rms[1] + self.epsilon)

    def state_dict(self) -> dict:
        return {"rms": self.rms.detach().cpu().clone(), "ret": self.ret.detach().cpu().clone(), "gamma": self.gamma,
                "clip": self.clip, "epsilon": self.epsilon}

    def load_state_dict(self, sd: dict) -> None:
        """Statistics, returns and, where the dict has them, the three settings.  Copied in place: a
        captured HIP graph that holds the buffers' addresses stays valid."""
        ret, rms = torch.as_tensor(sd["ret"], dtype=torch.float64), torch.as_tensor(sd["rms"], dtype=torch.float64)
        if ret.shape != (self.n,) or rms.shape != (3,):
            raise ValueError(f"the saved normaliser is for {ret.numel()} envs, this one for {self.n}")
        self.ret.copy_(ret)
        self.rms.copy_(rms)
        for k in ("gamma", "clip", "epsilon"):
            if k in sd:
                setattr(self, k, float(sd[k]))


__all__ = ["RewardNormalizer", "reward_norm_host", "chunk_sums", "fold_sums", "load", "bind", "NormError",
           "D2DNormStepArgs", "RMS_INIT", "default_blocks"]
