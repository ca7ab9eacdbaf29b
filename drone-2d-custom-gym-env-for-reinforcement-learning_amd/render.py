"""ctypes binding of ``libd2d_render.so`` (include/d2d_render.h) and the ``Renderer`` that owns its ctx.

The library draws frames of many envs at once into a device tensor, and the overview plot of a
scenario's flight paths; its picture model (pixel centres, three primitive kinds, last primitive
wins, no anti-aliasing) is described in the header and in INTEGRATION.md.  ``render_host`` /
``plot_paths_host`` are its CPU twins: the same code compiled for the host, byte-identical pictures,
no GPU needed.  There is no fallback from one to the other: ``Renderer`` draws on the device or fails.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

ABI_VERSION = 1
MIN_SIZE, MAX_SIZE = 8, 2048
PATH_SAMPLES = 100
BAR_ROWS = 100
L_PATH, L_GUIDES, L_OBSTACLES, L_DRONE, L_FORCES, L_TRAIL = 1, 2, 4, 8, 16, 32
L_ALL = 63
BACKGROUND = (243, 243, 243)
E_OK, E_ARG, E_HIP, E_NOMEM = 0, 1, 2, 4

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_render.so")


class D2DRView(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("screen_w", C.c_double), ("screen_h", C.c_double),
                ("layers", C.c_uint32), ("pad", C.c_uint32)]


_VP = C.c_void_p
_VIEW = C.POINTER(D2DRView)
SIGNATURES = {
    "d2dr_abi_version": (C.c_int32, []),
    "d2dr_last_error": (C.c_char_p, []),
    "d2dr_create": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_VP)]),
    "d2dr_destroy": (None, [_VP]),
    "d2dr_render": (C.c_int32, [_VP, _VIEW, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "d2dr_plot_paths": (C.c_int32, [_VP, _VIEW, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP, _VP]),
    "d2dr_render_host": (C.c_int32, [_VIEW, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP]),
    "d2dr_plot_paths_host": (C.c_int32, [_VIEW, _VP, _VP, _VP, _VP, C.c_int32, C.c_int32, _VP]),
    "d2dr_path_samples_host": (C.c_int32, [_VP, _VP]),
}

_lib = None


class RenderError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (once) the render library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from ._build import build_render

        build_render()
    from . import _native

    _lib = _native.bind(LIB_PATH, SIGNATURES, "d2dr_abi_version", ABI_VERSION, RenderError)
    return _lib


def check(code: int, what: str) -> None:
    if code != E_OK:
        raise RenderError(f"{what} failed (code {code}): {load().d2dr_last_error().decode()}")


def _size(size) -> tuple:
    h, w = (size, size) if isinstance(size, (int, np.integer)) else size
    return int(h), int(w)


def make_view(size, screen, layers: int = L_ALL) -> D2DRView:
    """``size``: an int or (H, W); ``screen``: the world extent (screensize_x, screensize_y)."""
    h, w = _size(size)
    return D2DRView(w, h, float(screen[0]), float(screen[1]), int(layers), 0)


def scn_array(records) -> "C.Array":
    """A contiguous ``D2DScn`` array from Scenario objects / ABI records."""
    recs = [r if isinstance(r, abi.D2DScn) else r.to_c() for r in records]
    return (abi.D2DScn * len(recs))(*recs)


def _np(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _p(a):
    return None if a is None else a.ctypes.data_as(_VP)


# ------------------------------------------------------------------------------------------ CPU twins
def render_host(records, state, obs=None, act=None, trail=None, trail_len=None, *, size=256, screen=(1300, 1300),
                layers: int = L_ALL) -> np.ndarray:
    """The CPU twin of ``Renderer.render``: uint8 [K, H, W, 3] from K ABI records, the fp64 state
    [32, K] (d2d_get_state's layout), obs [K, 27], act [K, 2], trail [K, T, 2] + trail_len [K]."""
    lib = load()
    recs = scn_array(records)
    k = len(recs)
    st = _np(state, np.float64)
    if st.shape != (abi.NSTATE, k):
        raise ValueError(f"state must have shape [{abi.NSTATE}, {k}]")
    ob, ac = _np(obs, np.float32), _np(act, np.float32)
    tr, tl = _np(trail, np.float32), _np(trail_len, np.int32)
    if ob is not None and ob.shape != (k, abi.OBS_DIM) or ac is not None and ac.shape != (k, abi.ACT_DIM):
        raise ValueError("obs must be [K, 27] and act [K, 2]")
    if tr is not None and (tr.ndim != 3 or tr.shape[0] != k or tr.shape[2] != 2 or tl is None or tl.shape != (k,)):
        raise ValueError("trail must be [K, T, 2] with trail_len [K]")
    view = make_view(size, screen, layers)
    out = np.zeros((k, view.height, view.width, 3), np.uint8)
    check(lib.d2dr_render_host(C.byref(view), k, C.cast(recs, _VP), _p(st), _p(ob), _p(ac), _p(tr), _p(tl),
                               tr.shape[1] if tr is not None else 0, _p(out)), "d2dr_render_host")
    return out


def plot_paths_host(record, xy, lens, rgb, *, size=256, screen=(1300, 1300)) -> np.ndarray:
    """The CPU twin of ``Renderer.plot_paths``: uint8 [H, W, 3]; xy [max_len, n_paths, 2] world
    positions, lens [n_paths], rgb [n_paths, 3]; ``record`` None gives a blank background."""
    lib = load()
    xy = _np(xy, np.float32)
    lens, rgb = _np(lens, np.int32), _np(rgb, np.uint8)
    n = int(lens.shape[0])
    if xy.ndim != 3 or xy.shape[1:] != (n, 2) or rgb.shape != (n, 3):
        raise ValueError("xy must be [max_len, n_paths, 2], lens [n_paths], rgb [n_paths, 3]")
    rec = scn_array([record]) if record is not None else None
    view = make_view(size, screen)
    out = np.empty((view.height, view.width, 3), np.uint8)
    out[:] = BACKGROUND  # what stays when there is no path at all (the library then draws nothing)
    check(lib.d2dr_plot_paths_host(C.byref(view), C.cast(rec, _VP) if rec is not None else None, _p(xy), _p(lens),
                                   _p(rgb), n, int(xy.shape[0]), _p(out)), "d2dr_plot_paths_host")
    return out


def path_samples(record) -> np.ndarray:
    """The 100 samples of the path layer, fp64 [100, 2] world positions."""
    rec = scn_array([record])
    out = np.zeros((PATH_SAMPLES, 2), np.float64)
    check(load().d2dr_path_samples_host(C.cast(rec, _VP), _p(out)), "d2dr_path_samples_host")
    return out


def red_blue_grad(f: float) -> tuple:
    """main.py:18-31 as bytes: red (low) to blue (high) through magenta."""
    if f < 0.5:
        return (255, 0, int(min(max(510.0 * f, 0.0), 255.0)))
    return (int(min(max(510.0 * (1.0 - f), 0.0), 255.0)), 0, 255)


def tile_images(frames: np.ndarray) -> np.ndarray:
    """[K, H, W, 3] -> one image of ceil(sqrt(K)) columns (SB3's tile_images layout), background-filled."""
    k, h, w, _ = frames.shape
    cols = int(np.ceil(np.sqrt(k)))
    rows = int(np.ceil(k / cols))
    out = np.empty((rows * h, cols * w, 3), np.uint8)
    out[:] = BACKGROUND
    for i in range(k):
        r, c = divmod(i, cols)
        out[r * h:(r + 1) * h, c * w:(c + 1) * w] = frames[i]
    return out


def write_png(path: str, img: np.ndarray) -> None:
    """An 8-bit RGB PNG of uint8 [H, W, 3], with the standard library's zlib only."""
    import struct
    import zlib

    img = np.ascontiguousarray(img, np.uint8)
    h, w, ch = img.shape
    if ch != 3:
        raise ValueError("write_png takes an [H, W, 3] image")

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = np.zeros((h, 1 + 3 * w), np.uint8)  # filter type 0 in front of every row
    raw[:, 1:] = img.reshape(h, 3 * w)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def save_gif(frames, path: str, fps: int = 60) -> None:
    """Frames [T, H, W, 3] (uint8, numpy or a torch tensor) as an animated GIF; needs Pillow."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("save_gif needs Pillow (PIL), which is not installed; the frames themselves need nothing "
                          "beyond numpy") from e
    if hasattr(frames, "cpu"):
        frames = frames.cpu().numpy()
    ims = [Image.fromarray(np.ascontiguousarray(f, np.uint8)) for f in frames]
    if not ims:
        raise ValueError("save_gif needs at least one frame")
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=max(1, round(1000 / fps)), loop=0)


# ------------------------------------------------------------------------------------------ device
class Renderer:
    """Owns one ``d2dr`` ctx on a HIP device: all device workspace is allocated here, and the render
    calls neither allocate (beyond the output tensor) nor synchronise.  Capacities are fixed at
    construction; exceeding one raises ``RenderError``."""

    def __init__(self, device, max_frames: int = 16, max_trail: int = 0, max_width: int = MAX_SIZE,
                 max_height: int = MAX_SIZE):
        import torch

        self._lib = load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("Renderer draws on a HIP device only (device='cuda[:k]'); the CPU twins are "
                             "render_host / plot_paths_host")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_frames, self.max_trail = int(max_frames), int(max_trail)
        self.max_width, self.max_height = int(max_width), int(max_height)
        h = _VP()
        check(self._lib.d2dr_create(self.device.index, self.max_frames, self.max_trail, self.max_width,
                                    self.max_height, C.byref(h)), "d2dr_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            import torch

            torch.cuda.synchronize(self.device)
            self._lib.d2dr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _stream(self):
        import torch

        return _VP(torch.cuda.current_stream(self.device).cuda_stream)

    def scn_tensor(self, records):
        """ABI records (or Scenario objects) as a device uint8 tensor [K, sizeof(d2d_scn)]."""
        import torch

        recs = scn_array(records)
        host = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).reshape(len(recs), C.sizeof(abi.D2DScn))
        return host.to(self.device)

    def render(self, scn, state, obs=None, act=None, trail=None, trail_len=None, *, size=256, screen=(1300, 1300),
               layers: int = L_ALL, out=None):
        """uint8 [K, H, W, 3] on the device.  ``scn``: device uint8 [K, sizeof(d2d_scn)] (``scn_tensor``);
        ``state`` float64 [32, K]; ``obs`` float32 [K, 27], ``act`` float32 [K, 2], ``trail`` float32
        [K, max_trail, 2] with ``trail_len`` int32 [K] (each optional)."""
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
        view = make_view(size, screen, layers)
        if out is None:
            out = torch.empty((k, view.height, view.width, 3), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (k, view.height, view.width, 3) or not out.is_contiguous() \
                or out.device != dev:
            raise ValueError("out must be a contiguous uint8 [K, H, W, 3] tensor on the renderer's device")
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(self._lib.d2dr_render(self._h, C.byref(view), k, p(scn), p(state), p(obs), p(act), p(trail), p(trail_len),
                                    p(out), self._stream()), "d2dr_render")
        self._keep = (scn, state, obs, act, trail, trail_len)  # alive until the kernels have read them
        return out

    def plot_paths(self, scn, xy, lens, rgb, *, size=256, screen=(1300, 1300), out=None):
        """The overview plot, uint8 [H, W, 3] on the device.  ``scn``: device uint8 [1, sizeof(d2d_scn)]
        or None (blank background); ``xy`` float32 [max_len, n_paths, 2] world positions, ``lens``
        int32 [n_paths], ``rgb`` uint8 [n_paths, 3]."""
        import torch

        dev = self.device
        xy = xy.to(device=dev, dtype=torch.float32).contiguous()
        lens = lens.to(device=dev, dtype=torch.int32).contiguous()
        rgb = rgb.to(device=dev, dtype=torch.uint8).contiguous()
        n = int(lens.shape[0])
        if xy.dim() != 3 or tuple(xy.shape[1:]) != (n, 2) or tuple(rgb.shape) != (n, 3):
            raise ValueError("xy must be [max_len, n_paths, 2], lens [n_paths], rgb [n_paths, 3]")
        if scn is not None:
            scn = scn.to(device=dev, dtype=torch.uint8).contiguous()
            if tuple(scn.shape) != (1, C.sizeof(abi.D2DScn)):
                raise ValueError("scn must be one ABI record")
        view = make_view(size, screen)
        if out is None:
            out = torch.empty((view.height, view.width, 3), dtype=torch.uint8, device=dev)
            if n == 0:
                out[:] = torch.tensor(BACKGROUND, dtype=torch.uint8, device=dev)  # the library draws nothing
        elif out.dtype != torch.uint8 or tuple(out.shape) != (view.height, view.width, 3) or not out.is_contiguous() \
                or out.device != dev:
            raise ValueError("out must be a contiguous uint8 [H, W, 3] tensor on the renderer's device")
        check(self._lib.d2dr_plot_paths(self._h, C.byref(view), scn.data_ptr() if scn is not None else None,
                                        xy.data_ptr(), lens.data_ptr(), rgb.data_ptr(), n, int(xy.shape[0]),
                                        out.data_ptr(), self._stream()), "d2dr_plot_paths")
        self._keep = (scn, xy, lens, rgb)
        return out


__all__ = ["Renderer", "RenderError", "render_host", "plot_paths_host", "path_samples", "red_blue_grad", "tile_images",
           "write_png", "save_gif", "make_view", "scn_array", "D2DRView", "L_ALL", "L_PATH", "L_GUIDES", "L_OBSTACLES",
           "L_DRONE", "L_FORCES", "L_TRAIL"]
