"""ctypes binding of ``libd2d_hud.so`` (include/d2d_hud.h): frames with the reference's "watch the agent
fly" extras -- the six lines of reward terms, the arcs that show which angle each guide line stands
for, and the shades (ghost drones) along the flight.

The library builds an extended primitive list around the renderer's own (``drone2d_amd.render``) and
rasterises it with the same tile walk; with none of ``L_TEXT`` / ``L_ARCS`` / ``L_SHADE`` set it returns
the renderer's bytes.  ``render_host`` and ``shade_update_host`` are CPU twins (the same code compiled
for the host, byte-identical results, no GPU needed); ``shade_update_np`` restates the recorder in NumPy.
There is no fallback from the device to the twins: ``HudRenderer`` draws on the device or fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi
from . import render as R
from .render import D2DRView, _np, _p, _size, make_view, scn_array

ABI_VERSION = 1
L_TEXT, L_ARCS, L_SHADE = 64, 128, 256
L_ALL = 511
ARC_SEGS = 32
TEXT_LINES, LINE_CHARS = 6, 40
MAX_SHADES = 4096
SHADE_FRAME_RGB, SHADE_MOTOR_RGB, TEXT_RED_RGB = (205, 222, 250), (170, 195, 235), (150, 0, 0)
E_OK, E_ARG, E_HIP, E_NOMEM = 0, 1, 2, 4
# (label, info field) of the six text lines; the last one is drawn in TEXT_RED_RGB, the others black
TEXT_FIELDS = (("Total reward: ", abi.INFO_REWARD), ("Collision avoidance: ", abi.INFO_CA),
               ("Path adherence: ", abi.INFO_PA), ("Path progression: ", abi.INFO_PP),
               ("Aggressive alpha: ", abi.INFO_AA), ("Closest obs dist: ", abi.INFO_DCLOSE))

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_hud.so")

_VP = C.c_void_p
_VIEW = C.POINTER(D2DRView)
_I = C.c_int32
SIGNATURES = {
    "d2dh_abi_version": (_I, []),
    "d2dh_last_error": (C.c_char_p, []),
    "d2dh_create": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_VP)]),
    "d2dh_destroy": (None, [_VP]),
    "d2dh_render": (_I, [_VP, _VIEW, _I, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "d2dh_shade_update": (_I, [_I, _I, _VP, _I, _VP, _VP, _VP, C.c_double, _I, _VP, _VP, _VP, _VP]),
    "d2dh_render_host": (_I, [_VIEW, _I, _VP, _VP, _VP, _VP, _VP, _VP, _I, _VP, _VP, _VP, _I, _VP]),
    "d2dh_shade_update_host": (_I, [_I, _VP, _I, _VP, _VP, _VP, C.c_double, _I, _VP, _VP, _VP]),
    "d2dh_format_host": (_I, [C.c_float, C.c_char_p]),
    "d2dh_glyph_host": (_I, [_I, _VP]),
}

_lib = None


class HudError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (once) the HUD library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from ._build import build_hud

        build_hud()
    from . import _native

    _lib = _native.bind(LIB_PATH, SIGNATURES, "d2dh_abi_version", ABI_VERSION, HudError)
    return _lib


def check(code: int, what: str) -> None:
    if code != E_OK:
        raise HudError(f"{what} failed (code {code}): {load().d2dh_last_error().decode()}")


def format_value(v) -> str:
    """The text the overlay prints for an info value: ``str(round(float(v), 2))``, computed by the library."""
    buf = C.create_string_buffer(16)
    check(load().d2dh_format_host(C.c_float(float(np.float32(v))), buf), "d2dh_format_host")
    return buf.value.decode()


def glyph(ch) -> np.ndarray:
    """uint8 [7, 5]: the font's bitmap of a character (a str of length 1 or a byte value)."""
    rows = np.zeros(7, np.uint8)
    check(load().d2dh_glyph_host(ord(ch) if isinstance(ch, str) else int(ch), _p(rows)), "d2dh_glyph_host")
    return (rows[:, None] >> np.arange(4, -1, -1)[None, :]) & 1


def text_scale(height: int) -> int:
    return max(1, int(height) // 512)


def _shade_args(shades, k: int):
    if shades is None:
        return None, None, 0
    poses, count = shades
    poses, count = _np(poses, np.float64), _np(count, np.int32)
    if poses.ndim != 3 or poses.shape[0] != k or poses.shape[2] != 3 or poses.shape[1] < 1 or count.shape != (k,):
        raise ValueError("shades must be (poses [K, S, 3], count [K]) with S >= 1")
    return poses, count, int(poses.shape[1])


# ------------------------------------------------------------------------------------------ CPU twins
def render_host(records, state, obs=None, act=None, trail=None, trail_len=None, info=None, shades=None, *, size=256,
                screen=(1300, 1300), layers: int = L_ALL) -> np.ndarray:
    """The CPU twin of ``HudRenderer.render``: ``render.render_host``'s arguments, then ``info`` float32
    [K, 12] (the env's info table; None: no text) and ``shades`` = (poses float64 [K, S, 3] of (x, y,
    frame angle), count int32 [K]) or None."""
    lib = load()
    recs = scn_array(records)
    k = len(recs)
    st = _np(state, np.float64)
    if st.shape != (abi.NSTATE, k):
        raise ValueError(f"state must have shape [{abi.NSTATE}, {k}]")
    ob, ac = _np(obs, np.float32), _np(act, np.float32)
    tr, tl = _np(trail, np.float32), _np(trail_len, np.int32)
    nf = _np(info, np.float32)
    if ob is not None and ob.shape != (k, abi.OBS_DIM) or ac is not None and ac.shape != (k, abi.ACT_DIM):
        raise ValueError("obs must be [K, 27] and act [K, 2]")
    if tr is not None and (tr.ndim != 3 or tr.shape[0] != k or tr.shape[2] != 2 or tl is None or tl.shape != (k,)):
        raise ValueError("trail must be [K, T, 2] with trail_len [K]")
    if nf is not None and nf.shape != (k, abi.INFO_DIM):
        raise ValueError(f"info must be [K, {abi.INFO_DIM}]")
    sp, sc, ms = _shade_args(shades, k)
    view = make_view(size, screen, layers)
    out = np.zeros((k, view.height, view.width, 3), np.uint8)
    check(lib.d2dh_render_host(C.byref(view), k, C.cast(recs, _VP), _p(st), _p(ob), _p(ac), _p(tr), _p(tl),
                               tr.shape[1] if tr is not None else 0, _p(nf), _p(sp), _p(sc), ms, _p(out)),
          "d2dh_render_host")
    return out


def _flags(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a).astype(np.uint8))


def shade_update_host(env_ids, state, term, trunc, distance, poses, count, last) -> None:
    """The CPU twin of the recorder's kernel: updates ``poses`` float64 [K, S, 3], ``count`` int32 [K] and
    ``last`` float64 [K, 2] in place from the batch's ``state`` float64 [32, N]; ``term`` / ``trunc``
    [N] are the step's flags, both None for "after reset"."""
    ids = _np(env_ids, np.int32)
    st = _np(state, np.float64)
    for a, dt in ((poses, np.float64), (count, np.int32), (last, np.float64)):
        if a.dtype != dt or not a.flags.c_contiguous:
            raise ValueError("poses, count and last must be contiguous float64 / int32 / float64 arrays")
    k = int(ids.shape[0])
    if poses.shape[0] != k or poses.ndim != 3 or poses.shape[2] != 3 or count.shape != (k,) or last.shape != (k, 2):
        raise ValueError("poses must be [K, S, 3], count [K] and last [K, 2]")
    te, tu = _flags(term), _flags(trunc)
    check(load().d2dh_shade_update_host(k, _p(ids), int(st.shape[1]), _p(st), _p(te), _p(tu), float(distance),
                                        int(poses.shape[1]), _p(poses), _p(count), _p(last)), "d2dh_shade_update_host")


def shade_update_np(env_ids, state, term, trunc, distance, poses, count, last) -> None:
    """``shade_update_host`` restated in NumPy (the same comparisons on the same float64 values)."""
    ids = np.asarray(env_ids, np.int64)
    x, y, a = state[0, ids], state[1, ids], state[2, ids]
    cap = poses.shape[1]
    if term is None:
        restart = np.ones(len(ids), bool)
    else:
        restart = np.asarray(term, bool)[ids] | np.asarray(trunc, bool)[ids]
    far = (np.abs(x - last[:, 0]) > distance) | (np.abs(y - last[:, 1]) > distance)
    n = np.where(restart, 0, count)
    for k in np.flatnonzero(restart | far):
        if n[k] < cap:
            poses[k, n[k]] = (x[k], y[k], a[k])
        last[k] = (x[k], y[k])
        count[k] = n[k] + 1


# ------------------------------------------------------------------------------------------ device
class HudRenderer:
    """Owns one ``d2dh`` ctx on a HIP device: all device workspace is allocated here, and ``render``
    neither allocates (beyond the output tensor) nor synchronises.  Capacities are fixed at
    construction; exceeding one raises."""

    def __init__(self, device, max_frames: int = 16, max_trail: int = 0, max_shades: int = 32,
                 max_width: int = R.MAX_SIZE, max_height: int = R.MAX_SIZE):
        import torch

        self._lib = load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("HudRenderer draws on a HIP device only (device='cuda[:k]'); the CPU twin is render_host")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_frames, self.max_trail, self.max_shades = int(max_frames), int(max_trail), int(max_shades)
        self.max_width, self.max_height = int(max_width), int(max_height)
        h = _VP()
        check(self._lib.d2dh_create(self.device.index, self.max_frames, self.max_trail, self.max_shades,
                                    self.max_width, self.max_height, C.byref(h)), "d2dh_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            import torch

            torch.cuda.synchronize(self.device)
            self._lib.d2dh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    scn_tensor = R.Renderer.scn_tensor  # ABI records as a device uint8 tensor [K, sizeof(d2d_scn)]

    def render(self, scn, state, obs=None, act=None, trail=None, trail_len=None, info=None, shades=None, *, size=256,
               screen=(1300, 1300), layers: int = L_ALL, out=None):
        """uint8 [K, H, W, 3] on the device.  ``Renderer.render``'s arguments, then ``info`` float32
        [K, 12] and ``shades`` = (poses float64 [K, max_shades, 3], count int32 [K]), each optional."""
        import torch

        k = int(scn.shape[0])
        dev = self.device

        def prep(t, dtype, shape, name):
            if t is None:
                return None
            t = t.to(device=dev, dtype=dtype).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
            return t

        scn = prep(scn, torch.uint8, (k, C.sizeof(abi.D2DScn)), "scn")
        state = prep(state, torch.float64, (abi.NSTATE, k), "state")
        obs = prep(obs, torch.float32, (k, abi.OBS_DIM), "obs")
        act = prep(act, torch.float32, (k, abi.ACT_DIM), "act")
        trail = prep(trail, torch.float32, (k, self.max_trail, 2), "trail")
        trail_len = prep(trail_len, torch.int32, (k,), "trail_len")
        info = prep(info, torch.float32, (k, abi.INFO_DIM), "info")
        sp = sc = None
        if shades is not None:
            sp = prep(shades[0], torch.float64, (k, self.max_shades, 3), "shade poses")
            sc = prep(shades[1], torch.int32, (k,), "shade count")
        view = make_view(size, screen, layers)
        if out is None:
            out = torch.empty((k, view.height, view.width, 3), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (k, view.height, view.width, 3) or not out.is_contiguous() \
                or out.device != dev:
            raise ValueError("out must be a contiguous uint8 [K, H, W, 3] tensor on the renderer's device")
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        stream = _VP(torch.cuda.current_stream(dev).cuda_stream)
        check(self._lib.d2dh_render(self._h, C.byref(view), k, p(scn), p(state), p(obs), p(act), p(trail), p(trail_len),
                                    p(info), p(sp), p(sc), p(out), stream), "d2dh_render")
        self._keep = (scn, state, obs, act, trail, trail_len, info, sp, sc)  # alive until the kernels have read them
        return out


class ShadeRecorder:
    """The shade lists of the envs ``env_ids`` of a batch, kept as the reference keeps its own
    (drone_2d_env.py:397, :416-419): a shade at spawn, another after a step whenever the drone has moved
    more than ``distance`` along x or y from the last one; an env that finished starts a new list with
    its new spawn pose.  Call ``restart()`` after ``reset`` and ``update()`` after each ``step``.

    On a HIP batch the buffers live on its device and one kernel launch updates them
    (``d2dh_shade_update``); a batch whose ``get_state`` returns host arrays goes through the CPU twin.
    ``poses`` [K, capacity, 3] float64 (x, y, frame angle), ``count`` [K] int32 (keeps counting past
    ``capacity``; poses beyond it are not stored)."""

    def __init__(self, venv, env_ids, distance: float = 75.0, capacity: int = 32):
        self.venv = venv
        ids = np.asarray(list(env_ids) if not isinstance(env_ids, np.ndarray) else env_ids, np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= venv.num_envs):
            raise ValueError(f"env_ids out of range for a batch of {venv.num_envs} envs")
        if not 1 <= int(capacity) <= MAX_SHADES:
            raise ValueError(f"capacity must be 1..{MAX_SHADES}")
        if not float(distance) >= 0.0:
            raise ValueError("distance must not be negative")
        self.env_ids = ids.astype(np.int32)
        self.distance, self.capacity = float(distance), int(capacity)
        k = len(ids)
        dev = getattr(venv, "device", None)
        self.on_device = dev is not None and getattr(dev, "type", "cpu") == "cuda"
        if self.on_device:
            import torch

            self._lib = load()
            self.device = dev
            self._ids = torch.from_numpy(self.env_ids).to(dev)
            self.poses = torch.zeros(k, self.capacity, 3, dtype=torch.float64, device=dev)
            self.count = torch.zeros(k, dtype=torch.int32, device=dev)
            self.last = torch.zeros(k, 2, dtype=torch.float64, device=dev)
        else:
            self.poses = np.zeros((k, self.capacity, 3), np.float64)
            self.count = np.zeros(k, np.int32)
            self.last = np.zeros((k, 2), np.float64)
        self.restart()

    def _step(self, term, trunc):
        st = self.venv.get_state()[0]
        if not self.on_device:
            shade_update_host(self.env_ids, np.asarray(st), term, trunc, self.distance, self.poses, self.count, self.last)
            return
        import torch

        if term is not None:
            term = term.to(device=self.device).contiguous().view(torch.uint8)
            trunc = trunc.to(device=self.device).contiguous().view(torch.uint8)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        stream = _VP(torch.cuda.current_stream(self.device).cuda_stream)
        check(self._lib.d2dh_shade_update(self.device.index, len(self.env_ids), p(self._ids), self.venv.num_envs, p(st),
                                          p(term), p(trunc), self.distance, self.capacity, p(self.poses), p(self.count),
                                          p(self.last), stream), "d2dh_shade_update")
        self._keep = (st, term, trunc)

    def restart(self):
        """After ``reset``: every tracked env's list becomes its spawn pose alone."""
        self._step(None, None)

    def update(self, term=None, trunc=None):
        """After ``step``: ``term`` / ``trunc`` default to the flags of the batch's last step."""
        if term is None or trunc is None:
            b = self.venv._bufs[self.venv._k]
            term, trunc = b["term"], b["trunc"]
        self._step(term, trunc)

    def shades(self):
        return self.poses, self.count


__all__ = ["HudRenderer", "HudError", "ShadeRecorder", "render_host", "shade_update_host", "shade_update_np",
           "format_value", "glyph", "text_scale", "L_TEXT", "L_ARCS", "L_SHADE", "L_ALL", "TEXT_FIELDS"]
