"""ctypes binding of ``libd2d_gif.so`` (include/d2d_gif.h): device frames into finished GIF89a bytes on the
device, and the loop that records episodes with it.

K streams (one GIF each) are encoded side by side; one ``GifEncoder.add`` takes one frame per stream and
costs two kernel launches: RGB -> palette index and the delta against the stream's canvas, then LZW and
the chunk's framing.  Only the compressed chunks cross to the host, every ``flush_every`` calls.
``HostEncoder`` / ``encode_host`` go over the CPU twin (the same code compiled for the host, the same
bytes, no GPU needed).  There is no fallback from one to the other: ``GifEncoder`` encodes on the device
or fails, and ``record_episodes`` takes a HIP batch only.  Needs neither Pillow nor anything beyond numpy
(and torch for the device half).
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from .render import _np, _p, _size

ABI_VERSION = 1
MAX_COLOURS = 255
SEGMENTS = 64
MIN_SIZE, MAX_SIZE = 8, 2048
MAX_STREAMS = 4096
FILE_HEADER_MAX = 800
MODEL_COLOURS = 14
TRAILER = b"\x3b"
E_OK, E_ARG, E_HIP, E_NOMEM = 0, 1, 2, 4

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_gif.so")

_VP = C.c_void_p
_I = C.c_int32
_L = C.c_int64
SIGNATURES = {
    "d2dg_abi_version": (_I, []),
    "d2dg_last_error": (C.c_char_p, []),
    "d2dg_dict_cap": (_I, []),
    "d2dg_frame_cap": (_L, [_I, _I]),
    "d2dg_create": (_I, [_I, _I, _I, _I, _VP, _I, C.POINTER(_VP)]),
    "d2dg_destroy": (None, [_VP]),
    "d2dg_restart": (_I, [_VP, _VP]),
    "d2dg_encode": (_I, [_VP, _I, _I, _I, _VP, _VP, _I, _VP, _L, _VP, _VP, _VP]),
    "d2dg_encode_host": (_I, [_I, _I, _I, _VP, _I, _VP, _VP, _I, _VP, _VP, _VP, _L, _VP, _VP, _VP]),
    "d2dg_file_header_host": (_I, [_I, _I, _VP, _I, _I, _VP, _I, C.POINTER(_I)]),
    "d2dg_model_palette": (_I, [_VP]),
}

_lib = None


class GifError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (once) the GIF library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from ._build import build_gif

        build_gif()
    from . import _native

    _lib = _native.bind(LIB_PATH, SIGNATURES, "d2dg_abi_version", ABI_VERSION, GifError)
    return _lib


def check(code: int, what: str) -> None:
    if code != E_OK:
        raise GifError(f"{what} failed (code {code}): {load().d2dg_last_error().decode()}")


def dict_cap() -> int:
    """The dictionary cap the library was compiled with (D2DG_DICT_CAP)."""
    return int(load().d2dg_dict_cap())


def frame_cap(size) -> int:
    """``d2dg_frame_cap``: the most bytes one frame chunk of an (H, W) stream can take."""
    h, w = _size(size)
    cap = int(load().d2dg_frame_cap(w, h))
    if cap <= 0:
        raise ValueError(f"picture {w} x {h}: width and height must be {MIN_SIZE}..{MAX_SIZE}")
    return cap


class Palette:
    """1..255 colours, uint8 [n, 3]; index n is the transparent index of the files."""

    def __init__(self, colours):
        c = np.ascontiguousarray(colours, dtype=np.uint8)
        if c.ndim != 2 or c.shape[1] != 3:
            raise ValueError("a palette is uint8 [n, 3]")
        if not 1 <= len(c) <= MAX_COLOURS:
            raise ValueError(f"a palette holds 1..{MAX_COLOURS} colours, got {len(c)}")
        self.colours = c

    def __len__(self) -> int:
        return len(self.colours)

    @property
    def bits(self) -> int:
        """The global colour table has 2^bits entries: the colours and the transparent index."""
        return max(1, int(len(self)).bit_length())

    @property
    def min_code_size(self) -> int:
        return max(2, self.bits)

    @classmethod
    def model(cls) -> "Palette":
        """The 14 colours the renderer and its HUD draw with (``d2dg_model_palette``'s order): frames of
        ``venv.render`` hold no other."""
        out = np.zeros((MODEL_COLOURS, 3), np.uint8)
        check(load().d2dg_model_palette(_p(out)), "d2dg_model_palette")
        return cls(out)

    @classmethod
    def scan(cls, frames) -> "Palette":
        """The distinct colours of ``frames`` [..., 3], sorted by packed value r << 16 | g << 8 | b;
        ``ValueError`` when there are more than 255."""
        if hasattr(frames, "cpu"):
            frames = frames.cpu().numpy()
        f = np.asarray(frames, np.uint8).reshape(-1, 3).astype(np.uint32)
        packed = np.unique(f[:, 0] << 16 | f[:, 1] << 8 | f[:, 2])
        if len(packed) > MAX_COLOURS:
            raise ValueError(f"{len(packed)} distinct colours: a palette holds at most {MAX_COLOURS} "
                             f"(Palette.uniform() takes any picture)")
        return cls(np.stack([packed >> 16, (packed >> 8) & 255, packed & 255], -1).astype(np.uint8))

    @classmethod
    def uniform(cls) -> "Palette":
        """A fixed 6 x 7 x 6 colour cube (252 colours; red-major, then green, then blue; levels
        round(255 i / (n - 1))) for pictures that are not the renderer's."""
        lv = lambda n: np.round(255.0 * np.arange(n) / (n - 1)).astype(np.uint8)  # noqa: E731
        r, g, b = np.meshgrid(lv(6), lv(7), lv(6), indexing="ij")
        return cls(np.stack([r.ravel(), g.ravel(), b.ravel()], -1))


def _palette(p) -> Palette:
    return p if isinstance(p, Palette) else Palette(p)


def file_header(size, palette, loop: int = 0) -> bytes:
    """``d2dg_file_header_host``: signature, logical screen, global colour table, NETSCAPE2.0 loop block
    (``loop`` None: no block)."""
    h, w = _size(size)
    pal = _palette(palette)
    out = np.zeros(FILE_HEADER_MAX, np.uint8)
    n = _I(0)
    check(load().d2dg_file_header_host(w, h, _p(pal.colours), len(pal), -1 if loop is None else int(loop), _p(out),
                                       len(out), C.byref(n)), "d2dg_file_header_host")
    return out[:n.value].tobytes()


# ------------------------------------------------------------------------------------------ CPU twin
class HostEncoder:
    """``GifEncoder`` over the CPU twin: ``add`` takes uint8 [K, H, W, 3] host frames.  It keeps what the
    device ctx keeps (canvases, "has a frame" flags) as host arrays, and for the tests ``chunk_lens`` (one
    int32 [K] per call) and ``mid_clears`` (Clear codes written inside segments, per stream)."""

    def __init__(self, n_streams: int, size, palette, loop: int = 0):
        self._lib = load()
        self.n_streams = int(n_streams)
        self.h, self.w = _size(size)
        self.palette = _palette(palette)
        self.loop = loop
        self.cap = frame_cap((self.h, self.w))
        k = self.n_streams
        self.canvas = np.zeros((k, self.h, self.w), np.uint8)
        self.has_frame = np.zeros(k, np.uint8)
        self.inexact = np.zeros(k, np.int32)
        self.mid_clears = np.zeros(k, np.int32)
        self.chunk_lens = []
        self._chunk = np.zeros((k, self.cap), np.uint8)
        self._parts = [[] for _ in range(k)]

    def add(self, frames, active=None, delay_cs: int = 3) -> None:
        f = _np(frames, np.uint8)
        k = self.n_streams
        if f.shape != (k, self.h, self.w, 3):
            raise ValueError(f"frames must be uint8 [{k}, {self.h}, {self.w}, 3], got {list(f.shape)}")
        act = None if active is None else np.ascontiguousarray(np.asarray(active).astype(np.uint8))
        if act is not None and act.shape != (k,):
            raise ValueError(f"active must be [{k}]")
        lens = np.zeros(k, np.int32)
        check(self._lib.d2dg_encode_host(k, self.w, self.h, _p(self.palette.colours), len(self.palette), _p(f), _p(act),
                                         int(delay_cs), _p(self.canvas), _p(self.has_frame), _p(self._chunk), self.cap,
                                         _p(lens), _p(self.inexact), _p(self.mid_clears)), "d2dg_encode_host")
        self.chunk_lens.append(lens)
        for s in range(k):
            if lens[s]:
                self._parts[s].append(self._chunk[s, :lens[s]].tobytes())

    def finish(self) -> list:
        """One finished file per stream; the encoder then begins new ones."""
        head = file_header((self.h, self.w), self.palette, self.loop)
        out = [head + b"".join(p) + TRAILER for p in self._parts]
        self._parts = [[] for _ in range(self.n_streams)]
        self.has_frame[:] = 0
        return out


def encode_host(frames, palette, active=None, delay_cs: int = 3, loop: int = 0) -> list:
    """Frames uint8 [T, K, H, W, 3] (``active`` bool [T, K] or None) through the CPU twin: K files."""
    f = np.asarray(frames, np.uint8)
    if f.ndim != 5 or f.shape[4] != 3:
        raise ValueError("frames must be [T, K, H, W, 3]")
    enc = HostEncoder(f.shape[1], f.shape[2:4], palette, loop)
    for t in range(f.shape[0]):
        enc.add(f[t], None if active is None else np.asarray(active)[t], delay_cs)
    return enc.finish()


# ------------------------------------------------------------------------------------------ device
class GifEncoder:
    """Owns one ``d2dg`` ctx on a HIP device and a chunk arena of ``flush_every`` calls: uint8
    [flush_every, K, frame_cap] with the lengths int32 [flush_every, K].  ``add`` launches two kernels on
    the current stream and neither allocates nor synchronises; the arena is read back (lengths, then the
    bytes up to the longest chunk) when ``flush_every`` calls have collected and in ``finish``.  All
    streams share the size and the palette given here."""

    def __init__(self, device, n_streams: int, size, palette, loop: int = 0, flush_every: int = 16):
        import torch

        self._lib = load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GifEncoder encodes on a HIP device only (device='cuda[:k]'); the CPU twin is HostEncoder")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_streams, self.flush_every = int(n_streams), int(flush_every)
        if self.flush_every < 1:
            raise ValueError("flush_every must be at least 1")
        self.h, self.w = _size(size)
        self.palette = _palette(palette)
        self.loop = loop
        self.cap = frame_cap((self.h, self.w))
        h = _VP()
        check(self._lib.d2dg_create(self.device.index, self.n_streams, self.w, self.h, _p(self.palette.colours),
                                    len(self.palette), C.byref(h)), "d2dg_create")
        self._h = h
        k = self.n_streams
        self._arena = torch.empty((self.flush_every, k, self.cap), dtype=torch.uint8, device=self.device)
        self._lens = torch.zeros((self.flush_every, k), dtype=torch.int32, device=self.device)
        self._inexact = torch.zeros(k, dtype=torch.int32, device=self.device)
        self._pending = 0
        self._keep = []
        self._parts = [[] for _ in range(k)]

    def close(self):
        if getattr(self, "_h", None):
            import torch

            torch.cuda.synchronize(self.device)
            self._lib.d2dg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _stream(self):
        import torch

        return _VP(torch.cuda.current_stream(self.device).cuda_stream)

    def add(self, frames, active=None, delay_cs: int = 3) -> None:
        """One frame per stream: ``frames`` uint8 [K, H, W, 3] on the device; ``active`` a device bool /
        uint8 tensor [K] or None (all).  No host synchronisation, except that the call which finds the
        arena full reads it back first.  The encoder holds ``frames`` and ``active`` only until the next
        flush: ``add`` calls captured in a graph must take tensors made OUTSIDE the capture and kept by
        the caller for as long as the graph is replayed (a tensor made inside belongs to the capture's
        pool, and nothing here keeps it alive)."""
        import torch

        k = self.n_streams
        if self._pending == self.flush_every:
            self.flush()
        if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.device == self.device
                and tuple(frames.shape) == (k, self.h, self.w, 3)):
            raise ValueError(f"frames must be a uint8 [{k}, {self.h}, {self.w}, 3] tensor on {self.device}")
        frames = frames.contiguous()
        if active is not None:
            if not (isinstance(active, torch.Tensor) and active.device == self.device and tuple(active.shape) == (k,)
                    and active.dtype in (torch.bool, torch.uint8)):
                raise ValueError(f"active must be a bool or uint8 [{k}] tensor on {self.device}")
            active = active.contiguous().view(torch.uint8)
        slot = self._pending
        check(self._lib.d2dg_encode(self._h, k, self.w, self.h, frames.data_ptr(),
                                    active.data_ptr() if active is not None else None, int(delay_cs),
                                    self._arena[slot].data_ptr(), self.cap, self._lens[slot].data_ptr(),
                                    self._inexact.data_ptr(), self._stream()), "d2dg_encode")
        self._keep.append((frames, active))  # alive until the kernels have read them
        self._pending += 1

    def flush(self, calls: int | None = None) -> None:
        """Read the collected chunks back (synchronises).  ``calls``: how many arena slots hold chunks
        (default: the ``add`` calls since the last flush; a replayed capture of ``add`` calls says so here)."""
        n = self._pending if calls is None else int(calls)
        if not 0 <= n <= self.flush_every:
            raise ValueError(f"calls must be 0..{self.flush_every}")
        if n:
            lens = self._lens[:n].cpu().numpy()
            longest = int(lens.max())
            data = self._arena[:n, :, :longest].cpu().numpy() if longest else None
            for c in range(n):
                for s in np.flatnonzero(lens[c]):
                    self._parts[s].append(data[c, s, :lens[c, s]].tobytes())
        self._pending = 0
        self._keep = []

    @property
    def inexact(self) -> np.ndarray:
        """int32 [K]: pixels that took a nearest colour, per stream, since the last ``finish`` (synchronises)."""
        return self._inexact.cpu().numpy()

    def finish(self) -> list:
        """One finished file (``bytes``) per stream; the encoder then begins new ones."""
        self.flush()
        head = file_header((self.h, self.w), self.palette, self.loop)
        out = [head + b"".join(p) + TRAILER for p in self._parts]
        self._parts = [[] for _ in range(self.n_streams)]
        self.last_inexact = self.inexact
        self._inexact.zero_()
        check(self._lib.d2dg_restart(self._h, self._stream()), "d2dg_restart")
        return out

    def save(self, paths) -> list:
        """``finish()`` written to ``paths`` (one per stream)."""
        paths = [os.fspath(p) for p in paths]
        if len(paths) != self.n_streams:
            raise ValueError(f"save needs {self.n_streams} paths")
        files = self.finish()
        for p, b in zip(paths, files):
            d = os.path.dirname(p)
            if d:
                os.makedirs(d, exist_ok=True)
            with open(p, "wb") as f:
                f.write(b)
        return files


# ------------------------------------------------------------------------------------------ recording
Recording = namedtuple("Recording", "gifs frames inexact env_ids")


def record_episodes(venv, policy, env_ids=None, *, seed: int = 0, deterministic: bool = False, size=256, every: int = 2,
                    delay_cs: int = 3, hud: bool = False, max_steps: int | None = None, check_every: int = 16) -> Recording:
    """Fly ``venv`` (a HIP ``Drone2dVecEnv``) under ``policy`` as ``evaluate.evaluate_policy`` does --
    ``venv.reset(seed)``, then per step ``evaluate.act(policy, obs, seed=seed, t=t,
    env_id_base=venv.cfg.env_id_base)`` (its rows are batch-invariant bit for bit) and ``venv.step`` -- and
    record the first episode of each of ``env_ids`` (default: the first min(num_envs, 16)) as a GIF, encoded
    on the device: the reference's per-scenario animation (main.py:266-295: every second frame, 30 fps).

    An episode of T steps gives T pictures: the reset frame and the frame after every step that does not
    end it; every ``every``-th of them is kept, ceil(T / every) frames of ``delay_cs`` / 100 s each.  The
    env resets itself inside the step kernel, so the TERMINAL state is never visible: the frame after an
    episode's last step would show the next episode's spawn, and is not recorded.

    ``hud``: the frames carry the text overlay, the angle arcs and the shades of a ``hud.ShadeRecorder``
    (the batch needs ``with_info=True``).  Nothing waits for the device except the encoder's read-back every
    16 frames and one "all done" flag every ``check_every`` steps.  Returns ``Recording(gifs, frames,
    inexact, env_ids)``: the files (``bytes``) per env, how many frames each holds, how many of its pixels
    were not one of ``Palette.model()``'s colours (0 for the renderer's pictures), and the env ids."""
    import torch

    from . import evaluate
    from .env import Drone2dVecEnv

    if not isinstance(venv, Drone2dVecEnv):
        raise ValueError("record_episodes needs a HIP Drone2dVecEnv: frames and files are made on the device")
    if int(every) < 1:
        raise ValueError("every must be at least 1")
    ids = venv._render_ids(env_ids)
    k = len(ids)
    if k == 0:
        return Recording([], np.zeros(0, np.int64), np.zeros(0, np.int32), ids.numpy())
    dev = venv.device
    cap = int(max_steps) if max_steps is not None else int(venv.kwargs["n_steps"]) + 1
    with torch.cuda.device(dev):
        enc = GifEncoder(dev, k, size, Palette.model())
        try:
            obs = venv.reset(seed=seed)
            shades = None
            if hud:
                from .hud import ShadeRecorder

                shades = ShadeRecorder(venv, ids.numpy())  # (its constructor takes the spawn poses)
            ids_dev = ids.to(dev)
            alive = torch.ones(k, dtype=torch.bool, device=dev)   # the first episode is still running
            kept = torch.zeros(k, dtype=torch.int32, device=dev)

            def picture():
                enc.add(venv.render(ids, size=size, text=hud, arcs=hud, shades=shades), alive, delay_cs)
                kept.add_(alive.to(torch.int32))

            picture()
            for t in range(cap):
                a = evaluate.act(policy, obs, deterministic=deterministic, seed=seed, t=t,
                                 env_id_base=int(venv.cfg.env_id_base))
                obs, _, term, trunc, _ = venv.step(a)
                alive &= ~(term | trunc)[ids_dev]
                if shades is not None:
                    shades.update(term, trunc)
                # the picture after step t + 1 is picture t + 1 of every env still in its first episode: which
                # steps are kept is known here, and the others are neither drawn nor encoded
                if (t + 1) % int(every) == 0:
                    picture()
                if (t + 1) % int(check_every) == 0 and not bool(alive.any()):
                    break
            inexact = enc.inexact
            return Recording(enc.finish(), kept.cpu().numpy().astype(np.int64), inexact, ids.numpy())
        finally:
            enc.close()


__all__ = ["Palette", "GifEncoder", "HostEncoder", "GifError", "encode_host", "record_episodes", "Recording", "file_header",
           "frame_cap", "dict_cap", "load", "TRAILER"]
