"""Disturbed evaluation: what a controller can lose before it fails.  Sensor noise and obstacle-sensor
dropout on the observations the policy sees, actuator noise, lag and motor loss on the actions the env
gets, applied on the device by ``libd2d_disturb.so`` (include/d2d_disturb.h) with one small launch each.

The disturbance is a level axis of the batch: env i flies under ``levels[env_level[i]]``, the way it acts
under policy ``env_policy[i]`` of a policy bank, so a whole robustness curve is one closed loop
(``evaluate.sweep(..., disturb=[...])``).  The draws of global env g at step t are Philox draws keyed by
(seed, g, t), so shards of a batch fly the unsharded batch.

``Disturber`` owns the device buffers and is usable on its own around ``Drone2dVecEnv.step``::

    d = Disturber(venv.num_envs, Disturbance(obs_sigma=0.02, act_delay=2), device=venv.device, seed=0)
    obs = venv.reset(seed=0)
    for t in range(steps):
        a = evaluate.act(policy, d.obs(obs, t), seed=0, t=t)   # the policy sees the disturbed observations
        obs, rew, term, trunc, info = venv.step(d.act(a, t))   # the env gets the disturbed actions

``HostDisturber`` is its NumPy twin with the same interface: the same float32 operations in the same
order.  From the same draws (``noise="given"``) it is the device's result bit for bit; with Philox draws
everything integer (the words, the uniforms, the dropout decisions) is exact and the normals agree as
closely as ``evaluate.philox_noise_host`` agrees with the evaluation library (NumPy's float32 log / cos /
sin are not the device's).  On a HIP device every call goes to the library (a missing library is an error,
there is no fallback).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import abi

ABI_VERSION = 1
OBS_DIM, ACT_DIM = abi.OBS_DIM, abi.ACT_DIM
N_PARAMS = 8
MAX_DELAY = 8
HIST_ROWS = MAX_DELAY + 1
SLOTS, SLOT0 = 3, 8
OBS_BLOCKS = 7
TAG_OBS, TAG_DROP, TAG_ACT = 0x44530000, 0x44530001, 0x44530002
P_OBS_SIGMA, P_ACT_SIGMA, P_DROPOUT, P_GAIN_L, P_GAIN_R, P_DELAY = range(6)
NOISE_NONE, NOISE_GIVEN, NOISE_PHILOX = 0, 1, 2
_MODES = {"none": NOISE_NONE, "given": NOISE_GIVEN, "philox": NOISE_PHILOX}
ALL_CHANNELS = (1 << OBS_DIM) - 1
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_disturb.so")

_VP = C.c_void_p
_F = np.float32


class D2DDisturbArgs(C.Structure):
    """include/d2d_disturb.h ``d2d_disturb_args``."""
    _fields_ = [(k, C.c_int32) for k in ("n", "t", "n_levels", "noise_mode")] + \
               [("obs_mask", C.c_uint32), ("pad", C.c_int32), ("env_id_base", C.c_int64), ("seed", C.c_uint64)] + \
               [(k, _VP) for k in ("params", "env_level", "obs_in", "obs_out", "z_obs", "u_drop", "z_obs_out",
                                   "u_drop_out", "act", "hist", "z_act", "z_act_out")]


class DisturbError(RuntimeError):
    pass


SIGNATURES = {
    "d2d_disturb_abi_version": (C.c_int32, []),
    "d2d_disturb_obs": (C.c_int32, [C.POINTER(D2DDisturbArgs), _VP]),
    "d2d_disturb_act": (C.c_int32, [C.POINTER(D2DDisturbArgs), _VP]),
}

_lib = None


def bind(path: str) -> C.CDLL:
    """The library at ``path`` with its signatures set and its ABI version checked."""
    from . import _native

    return _native.bind(path, SIGNATURES, "d2d_disturb_abi_version", ABI_VERSION, DisturbError)


def load() -> C.CDLL:
    """Load (once) the disturbance library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            from ._build import build_disturb

            build_disturb()
        _lib = bind(LIB_PATH)
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc:
        raise DisturbError(f"{what}: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


class Disturbance:
    """One disturbance level.  ``obs_sigma``: standard deviation of the sensor noise added to the
    observation channels; ``act_sigma``: of the actuator noise added to both actions (then clipped);
    ``sensor_dropout``: the probability, per step and obstacle slot, that the slot reads "nothing seen";
    ``motor_gain`` (left, right): the fraction of its thrust each motor delivers; ``act_delay``: env steps
    between choosing an action and applying it (0 .. 8).  The defaults are the nominal world.  ``name``
    labels the level in a sweep's results."""

    __slots__ = ("obs_sigma", "act_sigma", "sensor_dropout", "motor_gain", "act_delay", "name")

    def __init__(self, obs_sigma: float = 0.0, act_sigma: float = 0.0, sensor_dropout: float = 0.0,
                 motor_gain=(1.0, 1.0), act_delay: int = 0, name: str | None = None):
        def number(v, what):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"{what} must be a finite number, not {v!r}")
            return float(v)

        self.obs_sigma = number(obs_sigma, "obs_sigma")
        self.act_sigma = number(act_sigma, "act_sigma")
        self.sensor_dropout = number(sensor_dropout, "sensor_dropout")
        if self.obs_sigma < 0.0 or self.act_sigma < 0.0:
            raise ValueError("obs_sigma and act_sigma must be >= 0")
        if not 0.0 <= self.sensor_dropout <= 1.0:
            raise ValueError("sensor_dropout must lie in [0, 1]")
        try:
            gl, gr = motor_gain
        except (TypeError, ValueError):
            raise ValueError("motor_gain must be a pair (left, right)") from None
        self.motor_gain = (number(gl, "motor_gain"), number(gr, "motor_gain"))
        if min(self.motor_gain) < 0.0:
            raise ValueError("motor_gain must be >= 0")
        if isinstance(act_delay, bool) or not isinstance(act_delay, (int, np.integer)):
            raise ValueError(f"act_delay must be an integer, not {act_delay!r}")
        if not 0 <= int(act_delay) <= MAX_DELAY:
            raise ValueError(f"act_delay must lie in [0, {MAX_DELAY}]")
        self.act_delay = int(act_delay)
        self.name = None if name is None else str(name)

    def row(self) -> np.ndarray:
        """The level's row of the parameter table: float32 [8] (include/d2d_disturb.h)."""
        return np.array([self.obs_sigma, self.act_sigma, self.sensor_dropout, self.motor_gain[0], self.motor_gain[1],
                         self.act_delay, 0.0, 0.0], _F)

    def is_neutral(self) -> bool:
        return bool((self.row() == Disturbance().row()).all())

    def as_dict(self) -> dict:
        return {"obs_sigma": self.obs_sigma, "act_sigma": self.act_sigma, "sensor_dropout": self.sensor_dropout,
                "motor_gain_left": self.motor_gain[0], "motor_gain_right": self.motor_gain[1],
                "act_delay": self.act_delay}

    def __repr__(self) -> str:
        return "Disturbance(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + \
            (f", name={self.name!r})" if self.name is not None else ")")


def level_names(levels) -> list:
    """One unique name per level: its own, or ``level_<k>``."""
    names = [d.name if d.name is not None else f"level_{k}" for k, d in enumerate(levels)]
    if len(set(names)) != len(names):
        raise ValueError("disturbance level names must be unique")
    return names


def _levels(levels) -> list:
    levels = [levels] if isinstance(levels, Disturbance) else list(levels)
    if not levels or not all(isinstance(d, Disturbance) for d in levels):
        raise ValueError("levels must be a Disturbance or a non-empty list of them")
    return levels


def channel_mask(obs_channels) -> int:
    """``obs_channels`` (None: all 27; else channel indices) as the batch-wide bit mask."""
    if obs_channels is None:
        return ALL_CHANNELS
    mask = 0
    for c in obs_channels:
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < OBS_DIM:
            raise ValueError(f"obs_channels must be channel indices in [0, {OBS_DIM}), not {c!r}")
        mask |= 1 << int(c)
    return mask


class _Base:
    """What ``Disturber`` and ``HostDisturber`` share: the table, the map and the arguments' checks."""

    def __init__(self, n, levels, env_level, env_id_base, seed, obs_channels, noise, keep_draws):
        self.n = int(n)
        if self.n < 1:
            raise ValueError("a disturber needs at least one env")
        self.levels = _levels(levels)
        self.names = level_names(self.levels)
        self.table = np.stack([d.row() for d in self.levels])  # float32 [L, 8]
        if env_level is None:
            env_level = np.zeros(self.n, np.int32)
        el = env_level.detach().cpu().numpy() if isinstance(env_level, torch.Tensor) else np.asarray(env_level)
        if el.dtype.kind not in "iu" or el.shape != (self.n,):
            raise ValueError(f"env_level must be an integer array of shape [{self.n}]")
        # (a level outside [0, L) is allowed: that env is skipped, as the library documents)
        self.level_map = np.ascontiguousarray(el, dtype=np.int32)
        self.env_id_base = int(env_id_base)
        if self.env_id_base < 0 or self.env_id_base + self.n > 2 ** 32:
            raise ValueError("env_id_base + n must fit the 32-bit Philox counter word")
        self.seed = int(seed) & (2 ** 64 - 1)
        self.mask = channel_mask(obs_channels)
        if noise not in _MODES:
            raise ValueError("noise must be 'philox', 'given' or 'none'")
        self.noise = noise
        self.mode = _MODES[noise]
        self.keep_draws = bool(keep_draws)
        self.t = 0
        self.z_obs = self.u_drop = self.z_act = None  # the draws of the last calls, with keep_draws

    @property
    def n_levels(self) -> int:
        return len(self.levels)

    def reset(self) -> None:
        """Rewind to step 0: the start of a flight.  (The history needs no clearing: step t reads rows
        written at steps max(t - 8, 0) .. t.)"""
        self.t = 0

    def _step(self, t) -> int:
        t = self.t if t is None else int(t)
        if t < 0 or t >= 2 ** 31:
            raise ValueError("t must lie in [0, 2^31)")
        return t


class Disturber(_Base):
    """The device side: ``params`` [L, 8], ``env_level`` [n], the action history ``hist`` [9, n, 2] and the
    disturbed-observation buffer, on ``device``.

    ``levels``: a ``Disturbance`` or a list; ``env_level``: the level of each env (default all 0; an env
    with a level outside [0, L) is left undisturbed); ``env_id_base``: the global id of env 0 (a shard's
    ``venv.cfg.env_id_base``); ``seed``: the Philox key; ``obs_channels``: the channels that take sensor noise
    (default all); ``noise``: "philox", "given" (``obs`` and ``act`` take the draws) or "none" (no draw is
    made: only lag and motor loss run).  ``keep_draws``: ``z_obs`` [n, 27], ``u_drop`` [n, 3] and ``z_act``
    [n, 2] hold the draws of the last calls (0 where none was used).

    ``obs(obs, t)`` returns the disturbed observations (the loop's own buffer, overwritten by the next
    call; ``obs`` is not modified); ``act(act, t)`` disturbs ``act`` in place and returns it.  ``t``
    defaults to a counter that ``act`` moves on and ``reset`` rewinds."""

    def __init__(self, n, levels, env_level=None, *, device, env_id_base: int = 0, seed: int = 0, obs_channels=None,
                 noise: str = "philox", keep_draws: bool = False):
        super().__init__(n, levels, env_level, env_id_base, seed, obs_channels, noise, keep_draws)
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("Disturber runs on a HIP device; HostDisturber is its CPU twin")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._lib = load()
        f32 = dict(dtype=torch.float32, device=device)
        self.params = torch.from_numpy(self.table).to(device)
        self.env_level = torch.from_numpy(self.level_map).to(device)
        self.hist = torch.zeros(HIST_ROWS, self.n, ACT_DIM, **f32)
        self.obs_out = torch.empty(self.n, OBS_DIM, **f32)
        if self.keep_draws:
            self.z_obs = torch.zeros(self.n, OBS_DIM, **f32)
            self.u_drop = torch.zeros(self.n, SLOTS, **f32)
            self.z_act = torch.zeros(self.n, ACT_DIM, **f32)
        self._args = D2DDisturbArgs(n=self.n, n_levels=self.n_levels, noise_mode=self.mode, obs_mask=self.mask,
                                    env_id_base=self.env_id_base, params=self.params.data_ptr(),
                                    env_level=self.env_level.data_ptr(), obs_out=self.obs_out.data_ptr(),
                                    hist=self.hist.data_ptr())
        if self.keep_draws:
            self._args.z_obs_out, self._args.u_drop_out = self.z_obs.data_ptr(), self.u_drop.data_ptr()
            self._args.z_act_out = self.z_act.data_ptr()

    def _given(self, x, shape, what):
        if self.mode != NOISE_GIVEN:
            if x is not None:
                raise ValueError(f"{what} is taken with noise='given' only")
            return None
        if x is None:
            raise ValueError(f"noise='given' needs {what}")
        x = x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(x.shape) != shape:
            raise ValueError(f"{what} must be {list(shape)}")
        return x

    def _tensor(self, x, shape, what):
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != torch.float32 or \
                tuple(x.shape) != shape or not x.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 tensor {list(shape)} on {self.device}")
        return x

    @torch.no_grad()
    def obs(self, obs: torch.Tensor, t: int | None = None, *, z: torch.Tensor | None = None,
            u: torch.Tensor | None = None) -> torch.Tensor:
        a = self._args
        x = self._tensor(obs, (self.n, OBS_DIM), "obs")
        z = self._given(z, (self.n, OBS_DIM), "z")
        u = self._given(u, (self.n, SLOTS), "u")
        a.t, a.seed, a.obs_in = self._step(t), self.seed, x.data_ptr()
        a.z_obs, a.u_drop = (z.data_ptr(), u.data_ptr()) if z is not None else (None, None)
        with torch.cuda.device(self.device):
            _ok(self._lib.d2d_disturb_obs(C.byref(a), torch.cuda.current_stream(self.device).cuda_stream),
                "d2d_disturb_obs")
        return self.obs_out

    @torch.no_grad()
    def act(self, act: torch.Tensor, t: int | None = None, *, z: torch.Tensor | None = None) -> torch.Tensor:
        a = self._args
        x = self._tensor(act, (self.n, ACT_DIM), "act")
        z = self._given(z, (self.n, ACT_DIM), "z")
        a.t, a.seed, a.act = self._step(t), self.seed, x.data_ptr()
        a.z_act = z.data_ptr() if z is not None else None
        with torch.cuda.device(self.device):
            _ok(self._lib.d2d_disturb_act(C.byref(a), torch.cuda.current_stream(self.device).cuda_stream),
                "d2d_disturb_act")
        self.t = a.t + 1
        return act


# --------------------------------------------------------------------------- the NumPy twin
def philox_words(seed: int, g, t: int, tag: int, block: int = 0) -> np.ndarray:
    """Philox4x32-10 of counter (g, t, tag, block) under key (seed lo, seed hi): uint64 [4, len(g)]."""
    from .evaluate import _philox4x32

    g = np.asarray(g, np.uint64).reshape(-1)
    return _philox4x32(np.stack([g, np.full_like(g, t), np.full_like(g, tag), np.full_like(g, block)]),
                       (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def uniforms(w) -> np.ndarray:
    """include/d2d_eval.h's uniform of Philox words: ((w >> 8) + 0.5) * 2^-24 in float32, in (0, 1]."""
    return ((np.asarray(w, np.uint64) >> np.uint64(8)).astype(_F) + _F(0.5)) * _F(2.0 ** -24)


def box_muller(u0, u1) -> tuple:
    """include/d2d_eval.h's Box-Muller in float32 (``evaluate.philox_noise_host``'s lines)."""
    r = np.sqrt(_F(-2.0) * np.log(np.asarray(u0, _F)))
    a = _F(6.28318530717958647692) * np.asarray(u1, _F)
    return (r * np.cos(a)).astype(_F), (r * np.sin(a)).astype(_F)


def _clip1(x):
    return np.fmin(np.fmax(x, _F(-1.0)), _F(1.0))  # fminf(fmaxf(x, -1), 1)


class HostDisturber(_Base):
    """``Disturber`` in NumPy: the same interface over float32 arrays (or CPU tensors, which come back as
    tensors), the same operations in the header's order."""

    def __init__(self, n, levels, env_level=None, *, device="cpu", env_id_base: int = 0, seed: int = 0,
                 obs_channels=None, noise: str = "philox", keep_draws: bool = False):
        super().__init__(n, levels, env_level, env_id_base, seed, obs_channels, noise, keep_draws)
        self.device = torch.device("cpu")
        self.hist = np.zeros((HIST_ROWS, self.n, ACT_DIM), _F)
        self._valid = (self.level_map >= 0) & (self.level_map < self.n_levels)
        self._row = self.table[np.where(self._valid, self.level_map, 0)]  # [n, 8]; masked by _valid where used
        self._g = np.arange(self.env_id_base, self.env_id_base + self.n, dtype=np.uint64)
        self._channels = np.array([(self.mask >> c) & 1 for c in range(OBS_DIM)], bool)

    def _param(self, k):
        return self._row[:, k].astype(_F)

    def _given(self, x, shape, what):
        if self.mode != NOISE_GIVEN:
            if x is not None:
                raise ValueError(f"{what} is taken with noise='given' only")
            return None
        if x is None:
            raise ValueError(f"noise='given' needs {what}")
        x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=_F)
        if x.shape != shape:
            raise ValueError(f"{what} must be {list(shape)}")
        return x

    def obs_normals(self, t: int) -> np.ndarray:
        """The sensor-noise normals of step ``t`` in mode "philox": float32 [n, 27] (every channel's)."""
        z = np.zeros((self.n, 4 * OBS_BLOCKS), _F)
        for b in range(OBS_BLOCKS):
            u = uniforms(philox_words(self.seed, self._g, t, TAG_OBS, b))
            z[:, 4 * b], z[:, 4 * b + 1] = box_muller(u[0], u[1])
            z[:, 4 * b + 2], z[:, 4 * b + 3] = box_muller(u[2], u[3])
        return z[:, :OBS_DIM]

    def drop_uniforms(self, t: int) -> np.ndarray:
        """The dropout uniforms of step ``t`` in mode "philox": float32 [n, 3]."""
        return uniforms(philox_words(self.seed, self._g, t, TAG_DROP, 0))[:SLOTS].T.copy()

    def act_normals(self, t: int) -> np.ndarray:
        """The actuator-noise normals of step ``t`` in mode "philox": float32 [n, 2]."""
        u = uniforms(philox_words(self.seed, self._g, t, TAG_ACT, 0))
        return np.stack(box_muller(u[0], u[1]), -1)

    def obs(self, obs, t: int | None = None, *, z=None, u=None):
        t = self._step(t)
        as_tensor = isinstance(obs, torch.Tensor)
        x = np.array(obs.detach().cpu().numpy() if as_tensor else obs, dtype=_F)  # a copy: obs is not modified
        if x.shape != (self.n, OBS_DIM):
            raise ValueError(f"obs must be [{self.n}, {OBS_DIM}]")
        z = self._given(z, (self.n, OBS_DIM), "z")
        u = self._given(u, (self.n, SLOTS), "u")
        random = self.mode != NOISE_NONE
        sigma, p = self._param(P_OBS_SIGMA), self._param(P_DROPOUT)
        # 1. sensor noise, where it is on: x + sigma z, one multiplication and one addition in float32
        noisy = (self._valid & (sigma != 0) & random)[:, None] & self._channels[None, :]
        zs = np.zeros((self.n, OBS_DIM), _F)
        if noisy.any():
            zs = np.where(noisy, z if self.mode == NOISE_GIVEN else self.obs_normals(t), _F(0.0)).astype(_F)
            with np.errstate(invalid="ignore", over="ignore"):
                x = np.where(noisy, x + sigma[:, None] * zs, x)
        # 2. dropout, after the noise
        dropping = self._valid & (p != 0) & random
        us = np.zeros((self.n, SLOTS), _F)
        if dropping.any():
            us = np.where(dropping[:, None], u if self.mode == NOISE_GIVEN else self.drop_uniforms(t), _F(0.0)).astype(_F)
            drop = dropping[:, None] & (us < p[:, None])
            for j in range(SLOTS):
                c = SLOT0 + 3 * j
                x[:, c:c + 3] = np.where(drop[:, j:j + 1], np.array([1.0, 0.0, 0.0], _F), x[:, c:c + 3])
        if self.keep_draws:
            self.z_obs, self.u_drop = zs, us
        return torch.from_numpy(x) if as_tensor else x

    def act(self, act, t: int | None = None, *, z=None):
        t = self._step(t)
        as_tensor = isinstance(act, torch.Tensor)
        out = act.detach().numpy() if as_tensor else act  # in place
        if not isinstance(out, np.ndarray) or out.dtype != _F or out.shape != (self.n, ACT_DIM):
            raise ValueError(f"act must be a float32 array [{self.n}, {ACT_DIM}] (it is disturbed in place)")
        z = self._given(z, (self.n, ACT_DIM), "z")
        v = self._valid
        sigma = self._param(P_ACT_SIGMA)
        delay = np.clip(self._param(P_DELAY), 0, MAX_DELAY).astype(np.int64)
        a = out.copy()
        # 1. actuator noise
        noisy = v & (sigma != 0) & (self.mode != NOISE_NONE)
        zs = np.zeros((self.n, ACT_DIM), _F)
        if noisy.any():
            zs = np.where(noisy[:, None], z if self.mode == NOISE_GIVEN else self.act_normals(t), _F(0.0)).astype(_F)
            with np.errstate(invalid="ignore", over="ignore"):
                a = np.where(noisy[:, None], _clip1(a + sigma[:, None] * zs), a)
        # 2. lag: the row is always written (for an env with a level)
        cur = t % HIST_ROWS
        self.hist[cur] = np.where(v[:, None], a, self.hist[cur])
        src = np.maximum(t - delay, 0) % HIST_ROWS
        a = np.where((v & (delay != 0))[:, None], self.hist[src, np.arange(self.n)], a)
        # 3. motor loss, per motor
        for k, pk in ((0, P_GAIN_L), (1, P_GAIN_R)):
            g = self._param(pk)
            with np.errstate(invalid="ignore", over="ignore"):
                lost = _clip1((a[:, k] + _F(1.0)) * g - _F(1.0))
            a[:, k] = np.where(v & (g != 1), lost, a[:, k])
        out[...] = a
        if self.keep_draws:
            self.z_act = zs
        self.t = t + 1
        return act


def make_disturber(disturb, venv, seed: int, env_level=None):
    """``disturb`` (None, a ``Disturbance``, a list of them with ``env_level``, or a ready ``Disturber`` /
    ``HostDisturber``) as None or a disturber for the batch ``venv``: on its device (the NumPy twin for a
    batch on the CPU), keyed by ``seed`` and the batch's ``env_id_base``, rewound."""
    if disturb is None:
        return None
    n = int(venv.num_envs)
    host = torch.device(venv.device).type != "cuda"
    if isinstance(disturb, _Base):
        if disturb.n != n or isinstance(disturb, HostDisturber) != host:
            raise ValueError("the disturber was not built for this batch (its size or its device differ)")
        d = disturb
    else:
        base = int(getattr(venv.cfg, "env_id_base", 0))
        kw = dict(env_id_base=base, seed=seed)
        d = HostDisturber(n, disturb, env_level, **kw) if host else Disturber(n, disturb, env_level, device=venv.device, **kw)
    d.reset()
    return d


__all__ = ["Disturbance", "Disturber", "HostDisturber", "DisturbError", "D2DDisturbArgs", "make_disturber", "load",
           "bind", "level_names", "channel_mask", "philox_words", "uniforms", "box_muller", "MAX_DELAY", "HIST_ROWS",
           "TAG_OBS", "TAG_DROP", "TAG_ACT"]
