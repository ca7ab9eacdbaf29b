"""Arena maps: histograms over the arena of where a batch's first episodes fly, where they end and which
spawn positions they fail from, accumulated on the device by ``libd2d_heat.so`` (include/d2d_heat.h) with
one small launch per env step.

``ArenaMaps`` owns the device buffers: ``begin`` after the reset, ``step`` after every ``venv.step``,
``counts`` for the planes, ``images`` for the pictures.  ``HostMaps`` is its NumPy twin with the same
methods, ``from_flight`` the twin's batch form over a recorded flight buffer.  The counts are integers
and the arithmetic is csrc/heat/d2d_heat_core.h restated operation for operation, so device and twin
agree byte for byte.  On a HIP device every call goes to the library (a missing library is an error,
there is no fallback).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import abi

ABI_VERSION = 1
PLANES = 6
VISIT, SPAWN, SPAWN_SUCCESS, SPAWN_COLLISION, END_COLLISION, END_OTHER = range(PLANES)
PLANE_NAMES = ("visit", "spawn", "spawn_success", "spawn_collision", "end_collision", "end_other")
MAX_GRID = 256
MAX_GROUPS = 4096
PATH_AUTO, PATH_LDS, PATH_GLOBAL = 0, 1, 2
DENSITY, RATE = 0, 1
SUCCESS, COLLIDED, OTHER = 0, 1, 2
# the pictures harness.write_results draws: a plane (density) or (numerator, denominator) (rate)
PICTURES = {"density": VISIT, "spawn_success": (SPAWN_SUCCESS, SPAWN), "crashes": END_COLLISION}
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_heat.so")

_VP = C.c_void_p
_I32 = C.c_int32


class D2DHeatArgs(C.Structure):
    """include/d2d_heat.h ``d2d_heat_args``."""
    _fields_ = [(k, _I32) for k in ("n", "n_groups", "gx", "gy", "obs_dim", "info_dim", "path", "pad")] + \
               [(k, _VP) for k in ("obs", "terminal_obs", "term", "trunc", "info", "env_group", "alive", "spawn_cell",
                                   "planes", "outside")]


class D2DHeatColourArgs(C.Structure):
    """include/d2d_heat.h ``d2d_heat_colour_args``."""
    _fields_ = [(k, _I32) for k in ("n_groups", "gx", "gy", "h", "w", "mode", "plane_a", "plane_b", "alpha",
                                    "bg_shared")] + [("min_count", C.c_uint32), ("pad", _I32)] + \
               [(k, _VP) for k in ("planes", "bg", "out", "peak")]


class HeatError(RuntimeError):
    pass


SIGNATURES = {
    "d2d_heat_abi_version": (_I32, []),
    "d2d_heat_begin": (_I32, [C.POINTER(D2DHeatArgs), _VP, _VP]),
    "d2d_heat_step": (_I32, [C.POINTER(D2DHeatArgs), _VP]),
    "d2d_heat_clear": (_I32, [C.POINTER(D2DHeatArgs), _VP]),
    "d2d_heat_colour": (_I32, [C.POINTER(D2DHeatColourArgs), _VP]),
}

_lib = None


def bind(path: str) -> C.CDLL:
    """The library at ``path`` with its signatures set and its ABI version checked."""
    from . import _native

    return _native.bind(path, SIGNATURES, "d2d_heat_abi_version", ABI_VERSION, HeatError)


def load() -> C.CDLL:
    """Load (once) the arena-map library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            from ._build import build_heat

            build_heat()
        _lib = bind(LIB_PATH)
    return _lib


def _ok(rc: int, what: str) -> None:
    if rc:
        raise HeatError(f"{what}: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


# ------------------------------------------------------------------------- d2d_heat_core.h, restated in NumPy
_F = np.float32


def cell(o, G: int) -> np.ndarray:
    """``d2d_heat_cell``: the cell of float32 observation values on an axis of ``G`` cells, -1 outside."""
    o = np.asarray(o, _F)
    with np.errstate(invalid="ignore"):
        inside = (_F(-1.0) <= o) & (o < _F(1.0))
        u = (np.where(inside, o, _F(0.0)) + _F(1.0)) * _F(0.5)
        c = np.minimum((u * _F(G)).astype(np.int32), np.int32(G - 1))
    return np.where(inside, c, np.int32(-1)).astype(np.int32)


def cell2(ox, oy, Gx: int, Gy: int) -> np.ndarray:
    """``d2d_heat_cell2``: row * Gx + column (row 0 on top), -1 when either axis is outside."""
    cx, cy = cell(ox, Gx), cell(oy, Gy)
    return np.where((cx < 0) | (cy < 0), np.int32(-1), (Gy - 1 - cy) * Gx + cx).astype(np.int32)


def outcome_class(cause) -> np.ndarray:
    """``d2d_heat_class`` of the D2D_END_* bitmask: SUCCESS, COLLIDED or OTHER."""
    c = np.asarray(cause).astype(np.int32)
    collided = ((c & abi.END_COLLISION) != 0) & ((c & (abi.END_TIMEUP | abi.END_AA)) == 0)
    return np.where((c & abi.END_REACH) != 0, SUCCESS, np.where(collided, COLLIDED, OTHER)).astype(np.int32)


def isqrt(v) -> np.ndarray:
    """``d2d_heat_isqrt``: floor(sqrt(v)) of uint64 values, bit by bit."""
    v = np.array(v, np.uint64, ndmin=1)
    r = np.zeros_like(v)
    for shift in range(62, -1, -2):
        bit = np.uint64(1) << np.uint64(shift)
        t = r + bit
        ge = v >= t
        v = np.where(ge, v - t, v)
        r = np.where(ge, (r >> np.uint64(1)) + bit, r >> np.uint64(1))
    return r.astype(np.uint32)


def level(c, peak) -> np.ndarray:
    """``d2d_heat_level``: 0 for an empty cell, else max(1, isqrt(c * 65025 / peak))."""
    c = np.array(c, np.uint64, ndmin=1)
    peak = np.broadcast_to(np.asarray(peak, np.uint64), c.shape)
    lv = isqrt(c * np.uint64(65025) // np.maximum(peak, np.uint64(1))).astype(np.int64)
    return np.where((c == 0) | (peak == 0), 0, np.clip(lv, 1, 255)).astype(np.int32)


def rate_level(num, den) -> np.ndarray:
    """``d2d_heat_rate_level``: round(255 num / den), for den > 0."""
    num, den = np.array(num, np.uint64, ndmin=1), np.array(den, np.uint64, ndmin=1)
    lv = (np.uint64(510) * num + den) // (np.uint64(2) * np.maximum(den, np.uint64(1)))
    return np.minimum(lv, np.uint64(255)).astype(np.int32)


def _mix(a, b, f):
    return (a * (255 - f) + b * f + 127) // 255


ANCHORS = np.array([[13, 8, 135], [126, 3, 168], [204, 71, 120], [248, 149, 64], [240, 249, 33]], np.int64)


def _ramp() -> np.ndarray:
    p = 4 * np.arange(256, dtype=np.int64)
    s = np.minimum(p // 255, len(ANCHORS) - 2)
    f = (p - 255 * s)[:, None]
    return _mix(ANCHORS[s], ANCHORS[s + 1], f).astype(np.uint8)


def _rate_colours() -> np.ndarray:
    lv = np.arange(256, dtype=np.int64)
    low = 2 * lv < 255
    return np.stack([np.where(low, 255, 2 * (255 - lv)), np.zeros_like(lv), np.where(low, 2 * lv, 255)], -1).astype(np.uint8)


RAMP = _ramp()                  # ``d2d_heat_ramp``, uint8 [256, 3]
RATE_COLOURS = _rate_colours()  # ``d2d_heat_rate_colour``, uint8 [256, 3]


def blend(bg, colour, alpha: int) -> np.ndarray:
    """``d2d_heat_blend``: (bg (255 - a) + colour a + 127) / 255 per channel."""
    return _mix(np.asarray(bg, np.int64), np.asarray(colour, np.int64), int(alpha)).astype(np.uint8)


# --------------------------------------------------------------------------------------------- arguments
def parse_grid(grid) -> tuple:
    """``grid`` (an int, or (Gy, Gx)) as (Gy, Gx), each 1 .. 256, or a ``ValueError``."""
    if isinstance(grid, (int, np.integer)) and not isinstance(grid, bool):
        gy = gx = int(grid)
    else:
        try:
            gy, gx = (int(g) for g in grid)
        except (TypeError, ValueError):
            raise ValueError("grid must be an int or (Gy, Gx)") from None
    if not (1 <= gy <= MAX_GRID and 1 <= gx <= MAX_GRID):
        raise ValueError(f"grid sizes must lie in 1 .. {MAX_GRID}, got ({gy}, {gx})")
    return gy, gx


def check_groups(env_group, n: int, n_groups) -> tuple:
    """(env_group as a contiguous int32 array [n] or None, n_groups), every id in [0, n_groups), or a
    ``ValueError``: the library trusts the ids, so a map outside the planes is refused on the host."""
    if env_group is None:
        n_groups = 1 if n_groups is None else int(n_groups)
        eg = None
    else:
        eg = env_group.detach().cpu().numpy() if isinstance(env_group, torch.Tensor) else np.asarray(env_group)
        if eg.dtype.kind not in "iu" or eg.shape != (n,):
            raise ValueError(f"env_group must be an integer array of shape [{n}]")
        if n_groups is None:
            n_groups = int(eg.max()) + 1 if n else 1
        n_groups = int(n_groups)
        if n and (int(eg.min()) < 0 or int(eg.max()) >= n_groups):
            raise ValueError(f"env_group values must lie in [0, {n_groups})")
        eg = np.ascontiguousarray(eg, dtype=np.int32)
    if not 1 <= n_groups <= MAX_GROUPS:
        raise ValueError(f"n_groups must lie in 1 .. {MAX_GROUPS}")
    return eg, n_groups


def check_capacity(n: int, cap) -> None:
    """No plane can wrap while n x cap < 2^32 (``cap``: the most steps an env deposits; None: unchecked)."""
    if n <= 0 or n > 2 ** 30:
        raise ValueError("need 0 < n <= 2^30 envs")
    if cap is not None and int(n) * int(cap) >= 2 ** 32:
        raise ValueError(f"n x cap = {int(n) * int(cap)} >= 2^32: a uint32 plane could wrap")


def _batch(venv_or_n, cap):
    if isinstance(venv_or_n, (int, np.integer)):
        return int(venv_or_n), cap
    if cap is None and "n_steps" in getattr(venv_or_n, "kwargs", {}):
        cap = int(venv_or_n.kwargs["n_steps"]) + 1
    return int(venv_or_n.num_envs), cap


def picture(which) -> tuple:
    """(mode, plane_a, plane_b) of ``which``: a picture name of ``PICTURES``, a plane (its index or its
    name in ``PLANE_NAMES``) for its density, or a pair (numerator, denominator) of planes for a rate."""
    def plane(p):
        if isinstance(p, str):
            if p.lower() not in PLANE_NAMES:
                raise ValueError(f"unknown plane {p!r}: one of {PLANE_NAMES}")
            return PLANE_NAMES.index(p.lower())
        if not 0 <= int(p) < PLANES:
            raise ValueError(f"plane index {p} outside 0 .. {PLANES - 1}")
        return int(p)

    if isinstance(which, str) and which in PICTURES:
        which = PICTURES[which]
    if isinstance(which, (tuple, list)):
        if len(which) != 2:
            raise ValueError("a rate picture is a pair (numerator plane, denominator plane)")
        return RATE, plane(which[0]), plane(which[1])
    return DENSITY, plane(which), 0


def _check_paint(alpha, min_count) -> tuple:
    alpha, min_count = int(alpha), int(min_count)
    if not 0 <= alpha <= 255:
        raise ValueError("alpha must lie in 0 .. 255")
    if not 0 <= min_count < 2 ** 32:
        raise ValueError("min_count must lie in 0 .. 2^32 - 1")
    return alpha, min_count


def _bg_shape(shape, n_groups: int) -> tuple:
    """(shared, H, W) of a background of ``shape``: [H, W, 3] or [n_groups, H, W, 3]."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 3 and shape[2] == 3:
        shared, (h, w) = True, shape[:2]
    elif len(shape) == 4 and shape[0] == n_groups and shape[3] == 3:
        shared, (h, w) = False, shape[1:3]
    else:
        raise ValueError(f"backgrounds must be uint8 [H, W, 3] or [{n_groups}, H, W, 3]")
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("frame sizes must lie in 1 .. 16384")
    return shared, h, w


# ------------------------------------------------------------------------------------------------ host twin
def images_host(planes: np.ndarray, backgrounds, which="density", alpha: int = 200, min_count: int = 1) -> np.ndarray:
    """``d2d_heat_colour`` on NumPy arrays: ``planes`` uint32 [G, 6, Gy, Gx] painted over ``backgrounds``
    (uint8 [H, W, 3] shared, or [G, H, W, 3]); uint8 [G, H, W, 3]."""
    planes = np.asarray(planes, np.uint32)
    G, _, gy, gx = planes.shape
    bg = np.asarray(backgrounds, np.uint8)
    shared, h, w = _bg_shape(bg.shape, G)
    mode, pa, pb = picture(which)
    alpha, min_count = _check_paint(alpha, min_count)
    cy = (np.arange(h, dtype=np.int64) * gy) // h
    cx = (np.arange(w, dtype=np.int64) * gx) // w
    out = np.empty((G, h, w, 3), np.uint8)
    for g in range(G):
        a = planes[g, pa][cy[:, None], cx[None, :]]
        base = bg if shared else bg[g]
        if mode == DENSITY:
            lv = level(a.reshape(-1), planes[g, pa].max()).reshape(h, w)
            paint, colour = lv > 0, RAMP[lv]
        else:
            den = planes[g, pb][cy[:, None], cx[None, :]]
            paint = den >= max(min_count, 1)
            lv = rate_level(a.reshape(-1), np.maximum(den.reshape(-1), 1)).reshape(h, w)
            colour = RATE_COLOURS[lv]
        out[g] = np.where(paint[..., None], blend(base, colour, alpha), base)
    return out


class HostMaps:
    """The NumPy twin of ``ArenaMaps``: the same state, the same calls, the same bytes."""

    def __init__(self, venv_or_n, grid=64, env_group=None, n_groups=None, cap=None):
        self.n, cap = _batch(venv_or_n, cap)
        check_capacity(self.n, cap)
        self.gy, self.gx = parse_grid(grid)
        self.env_group, self.n_groups = check_groups(env_group, self.n, n_groups)
        self._group = self.env_group if self.env_group is not None else np.zeros(self.n, np.int32)
        self.planes = np.zeros((self.n_groups, PLANES, self.gy, self.gx), np.uint32)
        self.outside = np.zeros((self.n_groups, PLANES), np.uint32)
        self.alive = np.zeros(self.n, np.uint8)
        self.spawn_cell = np.full(self.n, -1, np.int32)
        self.spawn_obs = np.zeros((self.n, 2), np.float32)

    @staticmethod
    def _np(t, dtype=None):
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return a if dtype is None else a.astype(dtype, copy=False)

    def begin(self, obs) -> None:
        obs = self._np(obs, np.float32)
        self.alive[...] = 1
        self.spawn_obs = obs[:, 6:8].copy()
        self.spawn_cell[...] = cell2(obs[:, 6], obs[:, 7], self.gx, self.gy)

    def _deposit(self, plane: int, envs: np.ndarray, cells: np.ndarray) -> None:
        g = self._group[envs]
        inside = cells >= 0
        flat = self.planes.reshape(self.n_groups, PLANES, -1)
        np.add.at(flat, (g[inside], plane, cells[inside]), np.uint32(1))
        np.add.at(self.outside, (g[~inside], plane), np.uint32(1))

    def step(self, obs, term, trunc, terminal_obs, info) -> None:
        obs, tobs = self._np(obs, np.float32), self._np(terminal_obs, np.float32)
        info = self._np(info, np.float32)
        done = (self._np(term).astype(np.uint8) | self._np(trunc).astype(np.uint8)) != 0
        live = self.alive != 0
        xy = np.where(done[:, None], tobs[:, 6:8], obs[:, 6:8])
        c = cell2(xy[:, 0], xy[:, 1], self.gx, self.gy)
        idx = np.flatnonzero(live)
        self._deposit(VISIT, idx, c[idx])
        end = np.flatnonzero(live & done)
        cls = outcome_class(info[end, abi.INFO_CAUSE])
        self._deposit(SPAWN, end, self.spawn_cell[end])
        for k, plane in ((SUCCESS, SPAWN_SUCCESS), (COLLIDED, SPAWN_COLLISION)):
            self._deposit(plane, end[cls == k], self.spawn_cell[end[cls == k]])
        for k, plane in ((COLLIDED, END_COLLISION), (OTHER, END_OTHER)):
            self._deposit(plane, end[cls == k], c[end[cls == k]])
        self.alive[end] = 0

    def counts(self) -> dict:
        return {"planes": self.planes.copy(), "outside": self.outside.copy()}

    def clear(self) -> None:
        self.planes[...] = 0
        self.outside[...] = 0

    def images(self, backgrounds, which="density", alpha: int = 200, min_count: int = 1) -> np.ndarray:
        return images_host(self.planes, self._np(backgrounds, np.uint8), which, alpha, min_count)

    def close(self) -> None:
        pass


def from_flight(spawn_xy, xy, finished, rows, env_group=None, n_groups=None, grid=64) -> dict:
    """The planes of a recorded flight buffer, ``HostMaps`` in batch form: ``spawn_xy`` float32 [n, 2]
    (the reset observation's [6:8]), ``xy`` float32 [T, n, 2] (the recorder's raw observation values, one
    row per env step, NaN past each episode's end), ``finished`` bool [n], ``rows`` [n, 12] (the
    finished episodes' info rows).  A finished env flew ``rows[:, INFO_STEPS]`` steps, an unfinished one
    all ``T``.  Returns ``{"planes": uint32 [G, 6, Gy, Gx], "outside": uint32 [G, 6]}``."""
    spawn_xy, xy = np.asarray(spawn_xy, np.float32), np.asarray(xy, np.float32)
    finished, rows = np.asarray(finished).astype(bool), np.asarray(rows, np.float32)
    T, n = int(xy.shape[0]), int(xy.shape[1])
    if xy.shape != (T, n, 2) or spawn_xy.shape != (n, 2) or finished.shape != (n,) or rows.shape != (n, abi.INFO_DIM):
        raise ValueError("from_flight: spawn_xy [n, 2], xy [T, n, 2], finished [n], rows [n, 12]")
    m = HostMaps(max(n, 1), grid, env_group if n else None, n_groups)
    if n == 0:
        return m.counts()
    lens = np.where(finished, np.clip(rows[:, abi.INFO_STEPS].astype(np.int64), 0, T), T)
    flown = np.arange(T)[:, None] < lens[None, :]
    t_idx, envs = np.nonzero(flown)
    m._deposit(VISIT, envs, cell2(xy[t_idx, envs, 0], xy[t_idx, envs, 1], m.gx, m.gy))
    end = np.flatnonzero(finished & (lens > 0))
    spawn = cell2(spawn_xy[end, 0], spawn_xy[end, 1], m.gx, m.gy)
    last = xy[lens[end] - 1, end]
    c = cell2(last[:, 0], last[:, 1], m.gx, m.gy)
    cls = outcome_class(rows[end, abi.INFO_CAUSE])
    m._deposit(SPAWN, end, spawn)
    for k, plane in ((SUCCESS, SPAWN_SUCCESS), (COLLIDED, SPAWN_COLLISION)):
        m._deposit(plane, end[cls == k], spawn[cls == k])
    for k, plane in ((COLLIDED, END_COLLISION), (OTHER, END_OTHER)):
        m._deposit(plane, end[cls == k], c[cls == k])
    return m.counts()


def from_result(m: dict) -> dict:
    """``from_flight`` over the raw recorder buffers a result dict of ``evaluate_policy(...,
    flight_paths=True, maps=...)`` carries under ``m["maps"]``: what its planes must equal."""
    r = m["maps"]
    if "flight_obs" not in r:
        raise ValueError("the result carries no flight buffer: evaluate with flight_paths=True and maps")
    c = from_flight(r["spawn_obs"], r["flight_obs"], r["finished"], r["rows"], None, 1, r["planes"].shape[1:])
    return {"planes": c["planes"][0], "outside": c["outside"][0]}


# ---------------------------------------------------------------------------------------------- the device
class ArenaMaps:
    """The arena maps of a batch of ``n`` envs (``venv_or_n``: the batch, or n) on a HIP ``device``
    (default: the batch's): ``grid`` an int or (Gy, Gx), ``env_group`` an int array [n] of group ids
    (default: one group), ``n_groups`` (default: the largest id + 1), ``cap`` the most steps an env can
    deposit (default: the batch's ``n_steps`` + 1; n x cap >= 2^32 is refused).  ``path``: the
    aggregation path of include/d2d_heat.h (``PATH_AUTO`` chooses by the grid's size)."""

    def __init__(self, venv_or_n, grid=64, env_group=None, n_groups=None, device=None, cap=None, path: int = PATH_AUTO):
        self.n, cap = _batch(venv_or_n, cap)
        check_capacity(self.n, cap)
        self.gy, self.gx = parse_grid(grid)
        eg, self.n_groups = check_groups(env_group, self.n, n_groups)
        if path not in (PATH_AUTO, PATH_LDS, PATH_GLOBAL):
            raise ValueError("path must be PATH_AUTO, PATH_LDS or PATH_GLOBAL")
        if device is None:
            device = getattr(venv_or_n, "device", None)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ArenaMaps runs on a HIP device; HostMaps is its NumPy twin")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = load()
        dev = self.device
        # (torch has no uint32 arithmetic: the planes are int32 tensors whose bytes are the uint32 counts)
        self.planes = torch.zeros(self.n_groups, PLANES, self.gy, self.gx, dtype=torch.int32, device=dev)
        self.outside = torch.zeros(self.n_groups, PLANES, dtype=torch.int32, device=dev)
        self.alive = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.spawn_cell = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        self.spawn_obs = torch.zeros(self.n, 2, dtype=torch.float32, device=dev)
        self.env_group = torch.from_numpy(eg).to(dev) if eg is not None else None  # (a copy: checked once)
        self._peak = torch.zeros(self.n_groups, dtype=torch.int32, device=dev)
        self._checked = set()  # step's argument sets that passed its checks
        self._args = D2DHeatArgs(n=self.n, n_groups=self.n_groups, gx=self.gx, gy=self.gy, obs_dim=abi.OBS_DIM,
                                 info_dim=abi.INFO_DIM, path=int(path),
                                 env_group=self.env_group.data_ptr() if eg is not None else None,
                                 alive=self.alive.data_ptr(), spawn_cell=self.spawn_cell.data_ptr(),
                                 planes=self.planes.data_ptr(), outside=self.outside.data_ptr())

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _rows(self, t: torch.Tensor, name: str, width: int) -> torch.Tensor:
        if t.device != self.device or t.dtype != torch.float32 or tuple(t.shape) != (self.n, width) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 [n, {width}] tensor on {self.device}")
        return t

    def begin(self, obs: torch.Tensor) -> None:
        """After the reset of every env: ``alive`` = 1, ``spawn_cell`` from ``obs`` [n, 27]."""
        self._rows(obs, "obs", abi.OBS_DIM)
        self.spawn_obs.copy_(obs[:, 6:8])
        _ok(self._lib.d2d_heat_begin(C.byref(self._args), obs.data_ptr(), self._stream()), "d2d_heat_begin")

    def step(self, obs, term, trunc, terminal_obs, info) -> None:
        """Digest one env step's outputs: one launch, stream-ordered, capturable."""
        if info is None:
            raise ValueError("the maps need the env's info rows (with_info=True)")
        # the env's outputs are double-buffered: a set of buffers (address and size in bytes of each) that
        # was checked once is not checked again, which matters where the loop is bound by the host
        key = tuple((t.data_ptr(), t.numel() * t.element_size()) for t in (obs, term, trunc, terminal_obs, info))
        if key not in self._checked:
            self._rows(obs, "obs", abi.OBS_DIM)
            self._rows(terminal_obs, "terminal_obs", abi.OBS_DIM)
            self._rows(info, "info", abi.INFO_DIM)
            for t, nm in ((term, "term"), (trunc, "trunc")):
                if t.device != self.device or t.element_size() != 1 or t.numel() != self.n or not t.is_contiguous():
                    raise ValueError(f"{nm} must be a contiguous one-byte [n] tensor on {self.device}")
            if len(self._checked) < 64:
                self._checked.add(key)
        a = self._args
        a.obs, a.terminal_obs, a.info = obs.data_ptr(), terminal_obs.data_ptr(), info.data_ptr()
        a.term, a.trunc = term.data_ptr(), trunc.data_ptr()
        _ok(self._lib.d2d_heat_step(C.byref(a), self._stream()), "d2d_heat_step")

    def clear(self) -> None:
        _ok(self._lib.d2d_heat_clear(C.byref(self._args), self._stream()), "d2d_heat_clear")

    def counts(self) -> dict:
        """``{"planes": uint32 [G, 6, Gy, Gx], "outside": uint32 [G, 6]}`` as NumPy (waits for the stream)."""
        return {"planes": self.planes.cpu().numpy().view(np.uint32), "outside": self.outside.cpu().numpy().view(np.uint32)}

    def images(self, backgrounds, which="density", alpha: int = 200, min_count: int = 1) -> torch.Tensor:
        """The planes painted over ``backgrounds`` (uint8 [H, W, 3] shared, or [G, H, W, 3]; a tensor or an
        array): uint8 [G, H, W, 3] on the device.  ``which``: see ``picture``."""
        return paint(self.planes, backgrounds, which, alpha, min_count, _peak=self._peak)

    def close(self) -> None:
        self.planes = self.outside = self.alive = self.spawn_cell = self.env_group = self._peak = None


def paint(planes, backgrounds, which="density", alpha: int = 200, min_count: int = 1, device=None, _peak=None):
    """``d2d_heat_colour``: ``planes`` ([G, 6, Gy, Gx]: a device tensor, or uint32 counts as NumPy, moved
    to ``device``) painted over ``backgrounds``; uint8 [G, H, W, 3] on the device."""
    if not isinstance(planes, torch.Tensor):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        planes = torch.from_numpy(np.ascontiguousarray(planes, np.uint32).view(np.int32)).to(device)
    if not planes.is_cuda or planes.dtype != torch.int32 or planes.dim() != 4 or planes.shape[1] != PLANES \
            or not planes.is_contiguous():
        raise ValueError("planes must be a contiguous int32 [G, 6, Gy, Gx] tensor on a HIP device")
    dev = planes.device
    G, _, gy, gx = (int(s) for s in planes.shape)
    parse_grid((gy, gx))
    bg = backgrounds if isinstance(backgrounds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(backgrounds))
    if bg.dtype != torch.uint8:
        raise ValueError("backgrounds must be uint8")
    shared, h, w = _bg_shape(bg.shape, G)
    bg = bg.to(dev).contiguous()
    mode, pa, pb = picture(which)
    alpha, min_count = _check_paint(alpha, min_count)
    lib = load()
    with torch.cuda.device(dev):
        out = torch.empty(G, h, w, 3, dtype=torch.uint8, device=dev)
        peak = _peak if _peak is not None else torch.zeros(G, dtype=torch.int32, device=dev)
        a = D2DHeatColourArgs(n_groups=G, gx=gx, gy=gy, h=h, w=w, mode=mode, plane_a=pa, plane_b=pb, alpha=alpha,
                              bg_shared=int(shared), min_count=min_count, planes=planes.data_ptr(),
                              bg=bg.data_ptr(), out=out.data_ptr(), peak=peak.data_ptr())
        _ok(lib.d2d_heat_colour(C.byref(a), torch.cuda.current_stream(dev).cuda_stream), "d2d_heat_colour")
    return out


__all__ = ["ArenaMaps", "HostMaps", "from_flight", "from_result", "images_host", "paint", "picture", "cell", "cell2",
           "outcome_class", "isqrt", "level", "rate_level", "blend", "RAMP", "RATE_COLOURS", "parse_grid", "check_groups",
           "check_capacity", "load", "bind", "HeatError", "D2DHeatArgs", "D2DHeatColourArgs", "PLANES", "PLANE_NAMES",
           "PICTURES", "VISIT", "SPAWN", "SPAWN_SUCCESS", "SPAWN_COLLISION", "END_COLLISION", "END_OTHER"]
