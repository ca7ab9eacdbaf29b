"""Build the HIP extension in-tree (hipcc, gfx950) -- used by ``__graft_entry__.build()``."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
SRC = os.path.join(PKG_DIR, "csrc", "d2d_hip.hip")


def env_headers() -> list:
    """Every header the env library's source can include: all of csrc/*.h (globbed, so a new header
    cannot be forgotten) and the public ABI header."""
    return sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.h"))) + [os.path.join(REPO, "include", "drone2d.h")]


HDRS = env_headers()
OUT = os.path.join(PKG_DIR, "_lib", "libdrone2d_hip.so")
# the same source with -DD2D_EXACT_TRIG=1: sin / cos / atan2 from d2d_pmath.h and the reference's
# bearing sequence (Drone2dVecEnv(exact_trig=True); bit-identical to the oracle's exact build)
EXACT_OUT = os.path.join(PKG_DIR, "_lib", "libdrone2d_hip_exact.so")
# the PPO update's fused element-wise kernels (include/d2d_ppo.h)
PPO_SRC = os.path.join(PKG_DIR, "csrc", "d2d_ppo.hip")
PPO_HDRS = [os.path.join(REPO, "include", "d2d_ppo.h")]
PPO_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_ppo.so")
# the renderer (include/d2d_render.h): a library of its own, under csrc/render/ so that env_headers()'
# glob of csrc/*.h does not make the env library rebuild with it
RENDER_SRC = os.path.join(PKG_DIR, "csrc", "render", "d2d_render.hip")
RENDER_HDRS = [os.path.join(PKG_DIR, "csrc", "render", "d2d_raster.h"), os.path.join(PKG_DIR, "csrc", "d2d_pmath.h"),
               os.path.join(REPO, "include", "d2d_render.h"), os.path.join(REPO, "include", "drone2d.h")]
RENDER_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_render.so")
# the text overlay, angle arcs and drone shades (include/d2d_hud.h): a library beside the renderer, built
# around the renderer's own headers (the primitive list and the tile walk of d2d_raster.h)
HUD_SRC = os.path.join(PKG_DIR, "csrc", "hud", "d2d_hud.hip")
HUD_HDRS = [os.path.join(PKG_DIR, "csrc", "hud", "d2d_hud_core.h"), os.path.join(PKG_DIR, "csrc", "hud", "d2d_font.h"),
            os.path.join(REPO, "include", "d2d_hud.h"), *RENDER_HDRS]
HUD_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_hud.so")
# the GIF encoder (include/d2d_gif.h), a library beside the renderer under csrc/gif/; it takes the colour
# constants of the renderer's and the HUD's headers and nothing else of them
GIF_SRC = os.path.join(PKG_DIR, "csrc", "gif", "d2d_gif.hip")
GIF_HDRS = [os.path.join(PKG_DIR, "csrc", "gif", "d2d_gif_core.h"), os.path.join(REPO, "include", "d2d_gif.h"), *HUD_HDRS]
GIF_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_gif.so")
# the fused evaluation step (include/d2d_eval.h), a library of its own under csrc/eval/
EVAL_SRC = os.path.join(PKG_DIR, "csrc", "eval", "d2d_eval.hip")
EVAL_HDRS = [os.path.join(PKG_DIR, "csrc", "eval", "d2d_eval_math.h"), os.path.join(REPO, "include", "d2d_eval.h")]
EVAL_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_eval.so")
# the episode monitor (include/d2d_monitor.h), a library of its own under csrc/monitor/
MONITOR_SRC = os.path.join(PKG_DIR, "csrc", "monitor", "d2d_monitor.hip")
MONITOR_HDRS = [os.path.join(REPO, "include", "d2d_monitor.h"), os.path.join(REPO, "include", "drone2d.h")]
MONITOR_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_monitor.so")
# reward normalisation (include/d2d_norm.h), a library of its own under csrc/norm/
NORM_SRC = os.path.join(PKG_DIR, "csrc", "norm", "d2d_norm.hip")
NORM_HDRS = [os.path.join(REPO, "include", "d2d_norm.h")]
NORM_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_norm.so")
# the arena maps (include/d2d_heat.h), a library of its own under csrc/heat/
HEAT_SRC = os.path.join(PKG_DIR, "csrc", "heat", "d2d_heat.hip")
HEAT_HDRS = [os.path.join(PKG_DIR, "csrc", "heat", "d2d_heat_core.h"), os.path.join(REPO, "include", "d2d_heat.h"),
             os.path.join(REPO, "include", "drone2d.h")]
HEAT_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_heat.so")
# disturbed evaluation (include/d2d_disturb.h), a library of its own under csrc/disturb/
DISTURB_SRC = os.path.join(PKG_DIR, "csrc", "disturb", "d2d_disturb.hip")
DISTURB_HDRS = [os.path.join(REPO, "include", "d2d_disturb.h")]
DISTURB_OUT = os.path.join(PKG_DIR, "_lib", "libd2d_disturb.so")

# -ffp-contract=off: the kernels follow the reference's NumPy evaluation order (explicit fma() only
# where NumPy/OpenBLAS fuses); no fast-math: IEEE inf/NaN semantics are part of the contract.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
               "-fno-fast-math", "-Wall", "-Werror"]


def hipcc() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def needs_build(out: str = OUT, src: str = SRC, hdrs=None) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(p) > t for p in [src, *(env_headers() if hdrs is None else hdrs)])


# the PPO update is float32 training arithmetic with no reference rounding to follow: FMAs contracted
# within an expression (-ffp-contract=on, which honours `#pragma clang fp contract(off)`: the rollout's
# GAE recursion keeps torch's operation-by-operation rounding; "fast" fuses across statements in the
# backend whatever the pragma says)
PPO_FLAGS = [f if f != "-ffp-contract=off" else "-ffp-contract=on" for f in HIPCC_FLAGS]


def _compile(src: str, out: str, verbose: bool, flags=None):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".tmp"
    cmd = [hipcc(), *(flags or HIPCC_FLAGS), "-I", os.path.join(REPO, "include"), src, "-o", tmp]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)


def build_exact(force: bool = False, verbose: bool = False) -> str:
    """The exact-trig build (libdrone2d_hip_exact.so), compiled only when asked for: by
    ``build(exact=True)`` (``__graft_entry__.build()``, which the tests rely on) or by the first
    ``Drone2dVecEnv(exact_trig=True)`` that finds it missing."""
    if force or needs_build(EXACT_OUT):
        _compile(SRC, EXACT_OUT, verbose, HIPCC_FLAGS + ["-DD2D_EXACT_TRIG=1"])
    return EXACT_OUT


def build_render(force: bool = False, verbose: bool = False) -> str:
    """The renderer (libd2d_render.so), with the env's flags: -ffp-contract=off is what makes its host
    twins and its kernels round alike.  Compiled by ``build()`` or by the first ``render()`` that
    finds it missing."""
    if force or needs_build(RENDER_OUT, RENDER_SRC, RENDER_HDRS):
        _compile(RENDER_SRC, RENDER_OUT, verbose)
    return RENDER_OUT


def build_hud(force: bool = False, verbose: bool = False) -> str:
    """The HUD renderer (libd2d_hud.so), with the renderer's flags (-ffp-contract=off: host twins and
    kernels round alike).  Compiled by ``build()`` or by the first HUD frame that finds it missing."""
    if force or needs_build(HUD_OUT, HUD_SRC, HUD_HDRS):
        _compile(HUD_SRC, HUD_OUT, verbose)
    return HUD_OUT


def build_gif(force: bool = False, verbose: bool = False) -> str:
    """The GIF encoder (libd2d_gif.so), with the env's flags (integer code: the host twin and the kernels
    give the same bytes whatever the flags).  Compiled by ``build()`` or by the first use of
    ``drone2d_amd.gif`` that finds it missing."""
    if force or needs_build(GIF_OUT, GIF_SRC, GIF_HDRS):
        _compile(GIF_SRC, GIF_OUT, verbose)
    return GIF_OUT


def build_eval(force: bool = False, verbose: bool = False) -> str:
    """The evaluation step (libd2d_eval.so), with the PPO library's flags (float32 arithmetic, FMAs
    contracted within an expression).  Compiled by ``build()`` or by the first evaluation that finds
    it missing."""
    if force or needs_build(EVAL_OUT, EVAL_SRC, EVAL_HDRS):
        _compile(EVAL_SRC, EVAL_OUT, verbose, PPO_FLAGS)
    return EVAL_OUT


def build_monitor(force: bool = False, verbose: bool = False) -> str:
    """The episode monitor (libd2d_monitor.so), with the env's flags (-ffp-contract=off: its sums are
    plain IEEE additions in the order include/d2d_monitor.h states, which the host twin repeats).
    Compiled by ``build()`` or by the first ``EpisodeMonitor`` on a HIP device that finds it missing."""
    if force or needs_build(MONITOR_OUT, MONITOR_SRC, MONITOR_HDRS):
        _compile(MONITOR_SRC, MONITOR_OUT, verbose)
    return MONITOR_OUT


def build_norm(force: bool = False, verbose: bool = False) -> str:
    """Reward normalisation (libd2d_norm.so), with the env's flags (-ffp-contract=off: its float64
    expressions and sums are plain IEEE operations in the order include/d2d_norm.h states, which the
    host twin repeats).  Compiled by ``build()`` or by the first ``RewardNormalizer`` on a HIP device
    that finds it missing."""
    if force or needs_build(NORM_OUT, NORM_SRC, NORM_HDRS):
        _compile(NORM_SRC, NORM_OUT, verbose)
    return NORM_OUT


def build_heat(force: bool = False, verbose: bool = False) -> str:
    """The arena maps (libd2d_heat.so), with the env's flags (-ffp-contract=off: the cell function's
    float32 operations round one by one, as the host twin's do; everything else is integer).  Compiled
    by ``build()`` or by the first ``heatmap.ArenaMaps`` on a HIP device that finds it missing."""
    if force or needs_build(HEAT_OUT, HEAT_SRC, HEAT_HDRS):
        _compile(HEAT_SRC, HEAT_OUT, verbose)
    return HEAT_OUT


def build_disturb(force: bool = False, verbose: bool = False) -> str:
    """Disturbed evaluation (libd2d_disturb.so), with the env's flags (-ffp-contract=off: its float32
    operations round one by one in the order include/d2d_disturb.h states, which the host twin repeats).
    Compiled by ``build()`` or by the first ``disturb.Disturber`` on a HIP device that finds it missing."""
    if force or needs_build(DISTURB_OUT, DISTURB_SRC, DISTURB_HDRS):
        _compile(DISTURB_SRC, DISTURB_OUT, verbose)
    return DISTURB_OUT


def build(force: bool = False, verbose: bool = False, exact: bool = False) -> str:
    """The in-tree libraries: the env (libdrone2d_hip.so: every mode, one scenario layout), the PPO
    update kernels (libd2d_ppo.so), the renderer (libd2d_render.so), its HUD (libd2d_hud.so) and the GIF encoder (libd2d_gif.so), the evaluation step
    (libd2d_eval.so), the episode monitor (libd2d_monitor.so), reward normalisation (libd2d_norm.so),
    the arena maps (libd2d_heat.so), disturbed evaluation (libd2d_disturb.so) and, with ``exact``, the env's
    exact-trig build."""
    stale = os.path.join(PKG_DIR, "_lib", "libdrone2d_hip_rm.so")  # rounds 1-3's second layout build
    if os.path.exists(stale):
        os.remove(stale)
    if force or needs_build():
        _compile(SRC, OUT, verbose)
    if exact:
        build_exact(force, verbose)
    if force or needs_build(PPO_OUT, PPO_SRC, PPO_HDRS):
        _compile(PPO_SRC, PPO_OUT, verbose, PPO_FLAGS)
    build_render(force, verbose)
    build_hud(force, verbose)
    build_gif(force, verbose)
    build_eval(force, verbose)
    build_monitor(force, verbose)
    build_norm(force, verbose)
    build_heat(force, verbose)
    build_disturb(force, verbose)
    return OUT
