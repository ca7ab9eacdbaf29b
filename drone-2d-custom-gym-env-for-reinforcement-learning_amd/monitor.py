"""The episode monitor of a training run: what the reference's ``TensorboardLogger`` callback collects
(tensorboardlogger.py:49-110) plus the per-term breakdown of every finished episode's return, digested
on the device by ``libd2d_monitor.so`` (include/d2d_monitor.h) with one small launch per env step.

``EpisodeMonitor.step`` takes a step's ``term`` / ``trunc`` / ``info`` outputs, ``flush`` returns the
``K`` sums over the episodes that ended since the last flush, ``scalars`` turns them into named means
and rates.  On HIP tensors every call goes to the library (a missing library is an error, there is no
fallback); on CPU tensors (the oracle backend of the tests) the same digest runs in ``monitor_host``,
a NumPy twin that adds in exactly the order the header states, so both give the same bits.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import abi

ABI_VERSION = 1
TERMS = 6
CHUNK = 256
MAX_BLOCKS = 1024
# columns (D2D_MON_*)
EPISODES, SUCCESS, FAIL, COLLISION, TIMEUP, AA, LEN, TOTREW, APE = range(9)
RUN, LAST, LAST_REWARD, MINCLR, MINCLR_N, SKIPPED, K = 9, 15, 21, 22, 23, 24, 25
# the six reward terms, in info-row order (D2D_INFO_CA .. D2D_INFO_AA)
TERM_NAMES = ("collision_avoidance", "path_adherence", "path_progression", "collision", "reach_end",
              "agressive_alpha")
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_monitor.so")
_CANONICAL_NAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]

_VP = C.c_void_p


class D2DMonitorStepArgs(C.Structure):
    """include/d2d_monitor.h ``d2d_monitor_step_args``."""
    _fields_ = [(k, C.c_int32) for k in ("n", "info_dim", "n_blocks", "pad")] + \
               [(k, _VP) for k in ("term", "trunc", "info", "run", "minclr", "live", "part")]


class MonitorError(RuntimeError):
    pass


_I32 = C.c_int32
SIGNATURES = {
    "d2d_monitor_abi_version": (_I32, []),
    "d2d_monitor_step": (_I32, [C.POINTER(D2DMonitorStepArgs), _VP]),
    "d2d_monitor_flush": (_I32, [_VP, _I32, _VP, _VP]),
    "d2d_monitor_reset": (_I32, [_I32, _VP, _VP, _VP, _I32, _VP]),
}

_lib = None


def bind(path: str) -> C.CDLL:
    """The library at ``path`` with its signatures set and its ABI version checked."""
    from . import _native

    return _native.bind(path, SIGNATURES, "d2d_monitor_abi_version", ABI_VERSION, MonitorError)


def load() -> C.CDLL:
    """Load (once) the monitor library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            from ._build import build_monitor

            build_monitor()
        _lib = bind(LIB_PATH)
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc:
        raise MonitorError(f"{what}: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


def default_blocks(n: int) -> int:
    return max(1, min((int(n) + CHUNK - 1) // CHUNK, MAX_BLOCKS))


# ---------------------------------------------------------------------------------------------- host twin
def event_vectors(info: np.ndarray, run: np.ndarray, minclr: np.ndarray, live: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """The deposit vectors [len(idx), K] of the envs ``idx`` whose episode ends with this step's rows
    (``run`` / ``minclr`` already hold this step): the columns of include/d2d_monitor.h."""
    rows = info[idx]
    v = np.zeros((len(idx), K), np.float64)
    lv = live[idx] != 0
    cause = rows[:, abi.INFO_CAUSE].astype(np.int32)
    c1, c2 = (cause & abi.END_COLLISION) != 0, (cause & abi.END_REACH) != 0
    c4, c5 = (cause & abi.END_TIMEUP) != 0, (cause & abi.END_AA) != 0
    v[:, EPISODES] = 1.0
    v[:, SUCCESS] = c2
    v[:, FAIL] = c1 | c4 | c5
    v[:, COLLISION] = c1 & ~c2 & ~c4 & ~c5
    v[:, TIMEUP] = c4
    v[:, AA] = c5
    v[:, LEN] = rows[:, abi.INFO_STEPS]
    v[:, TOTREW] = rows[:, abi.INFO_TOTREW]
    v[:, APE] = rows[:, abi.INFO_APE]
    v[:, RUN:RUN + TERMS] = run[:, idx].T
    v[:, LAST:LAST + TERMS] = rows[:, :TERMS]
    v[:, LAST_REWARD] = rows[:, abi.INFO_REWARD]
    m = minclr[idx]
    fin = np.isfinite(m)
    v[:, MINCLR] = np.where(fin, m, np.float32(0.0))
    v[:, MINCLR_N] = fin
    v[~lv] = 0.0
    v[~lv, SKIPPED] = 1.0
    return v


def monitor_host_step(term, trunc, info, run, minclr, live, part):
    """``d2d_monitor_step`` on NumPy arrays, in place, adding in the header's order.  Returns the step's
    events, which the device never materialises: (env indices, their vectors [., K]) or None."""
    n, n_blocks = run.shape[1], part.shape[0]
    info = np.asarray(info, np.float32)
    if info.shape != (n, abi.INFO_DIM):
        raise ValueError("info must be [n, 12] float32")
    done = (np.asarray(term).astype(np.uint8) | np.asarray(trunc).astype(np.uint8)) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        run += info[:, :TERMS].T.astype(np.float64)
        d = info[:, abi.INFO_DCLOSE]
        np.copyto(minclr, d, where=d < minclr)
        idx = np.flatnonzero(done)
        if not len(idx):
            return None
        vec = event_vectors(info, run, minclr, live, idx)
        wave = idx // 64  # global wave index: ascending idx = ascending (chunk, wave, lane)
        chunk_sum = {}
        # waves in ascending order; within one, lanes in ascending order
        starts = np.flatnonzero(np.r_[True, wave[1:] != wave[:-1]])
        ends = np.r_[starts[1:], len(idx)]
        for s, e in zip(starts, ends):
            acc = np.zeros(K, np.float64)
            for j in range(s, e):
                acc = acc + vec[j]
            c = int(wave[s]) // (CHUNK // 64)
            chunk_sum[c] = chunk_sum.get(c, np.zeros(K, np.float64)) + acc
        # every row takes its chunks in walk order; rows are independent of each other
        for c in sorted(chunk_sum):
            b = c % n_blocks
            part[b] = part[b] + chunk_sum[c]
    run[:, idx] = 0.0
    minclr[idx] = np.inf
    live[idx] = 1
    return idx, vec


def monitor_host_flush(part: np.ndarray) -> np.ndarray:
    """``d2d_monitor_flush``: rows added in ascending order from +0.0, NaN canonicalised, ``part`` zeroed."""
    out = np.zeros(K, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(part.shape[0]):
            out = out + part[b]
    part[...] = 0.0
    out[np.isnan(out)] = _CANONICAL_NAN
    return out


class monitor_host:
    """The NumPy twin of the library: the same state, the same calls, the same bits."""

    def __init__(self, n: int, n_blocks: int | None = None):
        self.n = int(n)
        self.n_blocks = default_blocks(n) if n_blocks is None else int(n_blocks)
        if self.n <= 0 or not 1 <= self.n_blocks <= MAX_BLOCKS:
            raise ValueError("need n > 0 and 1 <= n_blocks <= 1024")
        self.run = np.zeros((TERMS, self.n), np.float64)
        self.minclr = np.full(self.n, np.inf, np.float32)
        self.live = np.ones(self.n, np.uint8)
        self.part = np.zeros((self.n_blocks, K), np.float64)

    def reset(self, live: bool = True) -> None:
        self.run[...] = 0.0
        self.minclr[...] = np.inf
        self.live[...] = 1 if live else 0

    def step(self, term, trunc, info):
        return monitor_host_step(term, trunc, info, self.run, self.minclr, self.live, self.part)

    def flush(self) -> np.ndarray:
        return monitor_host_flush(self.part)


# ---------------------------------------------------------------------------------------------- the monitor
def scalars(vec) -> dict:
    """Named means and rates of a flushed vector: the reference logger's ``episodes/*`` (here the mean
    of the terminal step's value over every episode of the window), ``rollout/*`` and ``return/<term>``
    (the mean episode sum of each reward term), plus the counts ``episodes`` and ``skipped``.  A window
    without an episode gives NaN means."""
    v = np.asarray(vec.detach().cpu() if isinstance(vec, torch.Tensor) else vec, np.float64)
    n = float(v[EPISODES])
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = lambda x: float(x / n) if n else float("nan")  # noqa: E731
        out = {"episodes": n, "skipped": float(v[SKIPPED]),
               "episodes/avg_reward": mean(v[LAST_REWARD]), "episodes/avg_length": mean(v[LEN])}
        last_names = ("collision_avoidance_reward", "path_adherence_reward", "path_progression_reward",
                      "collision_reward", "reach_end_reward", "agressive_alpha_reward")
        for f, name in enumerate(last_names):
            out[f"episodes/avg_{name}"] = mean(v[LAST + f])
        out.update({"rollout/ep_rew_mean": mean(v[TOTREW]), "rollout/ep_len_mean": mean(v[LEN]),
                    "rollout/success_rate": mean(v[SUCCESS]), "rollout/collision_rate": mean(v[COLLISION]),
                    "rollout/timeup_rate": mean(v[TIMEUP]), "rollout/aa_rate": mean(v[AA]),
                    "rollout/ape_mean": mean(v[APE]),
                    "rollout/min_clearance_mean": float(v[MINCLR] / v[MINCLR_N]) if v[MINCLR_N] else float("nan")})
        for f, name in enumerate(TERM_NAMES):
            out[f"return/{name}"] = mean(v[RUN + f])
    return out


class EpisodeMonitor:
    """The monitor's buffers for a batch of ``n`` envs (``venv_or_n``: the batch, or n) on ``device``
    (default: the batch's), with ``n_blocks`` partial rows (default: one per 256 envs, at most 1 024)."""

    def __init__(self, venv_or_n, device=None, n_blocks: int | None = None):
        n = venv_or_n if isinstance(venv_or_n, (int, np.integer)) else venv_or_n.num_envs
        if device is None:
            device = getattr(venv_or_n, "device", "cpu")
        self.n = int(n)
        self.device = torch.device(device)
        self.n_blocks = default_blocks(self.n) if n_blocks is None else int(n_blocks)
        self.hip = self.device.type == "cuda"
        if self.hip and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.hip:
            self._lib = load()
            dev = self.device
            self.run = torch.zeros(TERMS, self.n, dtype=torch.float64, device=dev)
            self.minclr = torch.full((self.n,), float("inf"), dtype=torch.float32, device=dev)
            self.live = torch.ones(self.n, dtype=torch.uint8, device=dev)
            self.part = torch.zeros(self.n_blocks, K, dtype=torch.float64, device=dev)
            self.out = torch.zeros(K, dtype=torch.float64, device=dev)
            self._args = D2DMonitorStepArgs(n=self.n, info_dim=abi.INFO_DIM, n_blocks=self.n_blocks,
                                            run=self.run.data_ptr(), minclr=self.minclr.data_ptr(),
                                            live=self.live.data_ptr(), part=self.part.data_ptr())
        else:
            self._host = monitor_host(self.n, self.n_blocks)
            self.out = torch.zeros(K, dtype=torch.float64)

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def step(self, term: torch.Tensor, trunc: torch.Tensor, info: torch.Tensor) -> None:
        """Digest one env step's outputs (``term`` / ``trunc`` [n] bool or uint8, ``info`` [n, 12] float32)."""
        if info is None:
            raise ValueError("the monitor needs the env's info rows (with_info=True)")
        if not self.hip:
            if term.is_cuda or info.is_cuda:
                raise ValueError("a CPU monitor was handed HIP tensors")
            self._host.step(term.numpy(), trunc.numpy(), info.numpy())
            return
        for t, nm in ((term, "term"), (trunc, "trunc")):
            if t.device != self.device or t.element_size() != 1 or t.numel() != self.n or not t.is_contiguous():
                raise ValueError(f"{nm} must be a contiguous one-byte [n] tensor on {self.device}")
        if info.device != self.device or info.dtype != torch.float32 or info.dim() != 2 or info.shape[0] != self.n \
                or not info.is_contiguous():
            raise ValueError(f"info must be a contiguous float32 [n, {abi.INFO_DIM}] tensor on {self.device}")
        a = self._args
        a.info_dim = int(info.shape[1])
        a.term, a.trunc, a.info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
        _ok(self._lib.d2d_monitor_step(C.byref(a), self._stream()), "d2d_monitor_step")

    def flush(self, reduce: bool = False) -> torch.Tensor:
        """The sums [K] over the episodes that ended since the last flush (the monitor's own ``out``
        tensor, rewritten by the next flush; on a HIP device the call is stream-ordered and waits for
        nothing).  ``reduce``: SUM over the ranks of an initialised ``torch.distributed`` group, as
        ``shard.allreduce_stats`` reduces the statistics vector."""
        if self.hip:
            _ok(self._lib.d2d_monitor_flush(self.part.data_ptr(), self.n_blocks, self.out.data_ptr(), self._stream()),
                "d2d_monitor_flush")
        else:
            self.out.copy_(torch.from_numpy(self._host.flush()))
        if reduce:
            from .shard import allreduce_stats

            allreduce_stats(self.out)
        return self.out

    def reset(self, live: bool = True) -> None:
        """Forget the episodes under way.  ``live=True`` after a reset of every env; ``live=False`` when
        attaching to a batch in mid-flight: its running episodes are counted as skipped when they end."""
        if self.hip:
            _ok(self._lib.d2d_monitor_reset(self.n, self.run.data_ptr(), self.minclr.data_ptr(), self.live.data_ptr(),
                                            1 if live else 0, self._stream()), "d2d_monitor_reset")
        else:
            self._host.reset(live)

    scalars = staticmethod(scalars)


__all__ = ["EpisodeMonitor", "monitor_host", "monitor_host_step", "monitor_host_flush", "scalars", "load", "bind",
           "MonitorError", "D2DMonitorStepArgs", "K", "TERM_NAMES"]
