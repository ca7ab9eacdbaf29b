"""ctypes mirror of include/d2d_ppo.h and the binding of libd2d_ppo.so (the PPO update and rollout
kernels, csrc/d2d_ppo.hip).  No auto-build and no fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

from . import _native


class D2DPPORollout(C.Structure):
    """include/d2d_ppo.h ``d2d_ppo_rollout`` (one fused rollout step, ABI v4)."""
    _fields_ = [(k, C.c_int32) for k in ("n", "t", "T", "info_dim", "info_totrew")] + \
               [("gamma", C.c_float), ("gae_lambda_gamma", C.c_float), ("pad", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("obs", "noise", "log_std", "prev_rew", "prev_term", "prev_trunc",
                                          "prev_info", "obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf",
                                          "done_buf", "start0", "act_env", "adv_buf", "ret_buf", "stats")]


class D2DPPOCtl(C.Structure):
    """include/d2d_ppo.h ``d2d_ppo_ctl``: the control block's eight words (``ControlBlock.buf[:8]``)."""
    _fields_ = [(k, C.c_float) for k in ("lr", "clip", "clip_vf", "kl_limit")] + \
               [("stop", C.c_int32), ("count", C.c_int32), ("kl_sum", C.c_float), ("kl_last", C.c_float)]


ABI_VERSION = 6
PPO_CTL_VERSION = 1
PPO_TB_VERSION = 1

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
# every entry point returns a hipError_t: name -> (restype, argtypes)
SIGNATURES = {name: (C.c_int32, args) for name, args in {
    "d2d_ppo_abi_version": [],
    "d2d_ppo_adv_stats": [_i32, _vp, _vp, _vp, _vp],
    "d2d_ppo_head_finish": [_i32, _i32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp],
    "d2d_ppo_adam": [_i32, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _vp],
    "d2d_ppo_wgrad": [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "d2d_ppo_wgrad_head": [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                           _i32, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp],
    "d2d_ppo_wgrad_chunks": [_i32],
    "d2d_ppo_mlp_forward": [_i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "d2d_ppo_mlp_forward_adv": [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "d2d_ppo_mlp_backward": [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp],
    "d2d_ppo_mlp_partial_rows": [_i32],
    "d2d_ppo_permute": [_i64, _i32, C.c_uint64, _vp, _vp, _vp],
    "d2d_ppo_rollout_step": [C.POINTER(D2DPPORollout), _vp, _vp],
    "d2d_ppo_fused_rows": [_i32],
    "d2d_ppo_fused_grad": [_i32, *[_vp] * 8, _i32, _f32, _f32, _vp, _vp, _i32, _vp, _vp, _vp],
    "d2d_ppo_grad_reduce": [_i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp],
    # the control path (additive to ABI v6; versioned by d2d_ppo_ctl_version)
    "d2d_ppo_ctl_version": [],
    "d2d_ppo_ctl_reset": [_vp, _vp],
    "d2d_ppo_fused_grad_ctl": [_i32, *[_vp] * 9, _i32, _f32, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "d2d_ppo_grad_reduce_ctl": [_i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "d2d_ppo_adam_ctl": [_i32, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _vp, _vp],
    # the rollout step with the time-limit bootstrap (additive to ABI v6; versioned by d2d_ppo_tb_version)
    "d2d_ppo_tb_version": [],
    "d2d_ppo_rollout_step_tb": [C.POINTER(D2DPPORollout), _vp, _vp, _vp],
}.items()}

_PPO_LIB = None


def ppo_native():
    """ctypes binding of libd2d_ppo.so (include/d2d_ppo.h), loaded once; no fallback on a GPU."""
    global _PPO_LIB
    if _PPO_LIB is None:
        path = os.environ.get("D2D_PPO_LIB") or os.path.join(_native.LIB_DIR, "libd2d_ppo.so")  # (env: A/B builds)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: the HIP extension is not built "
                               "(run `python -c 'import __graft_entry__ as g; g.build()'`)")
        lib = _native.bind(path, SIGNATURES, "d2d_ppo_abi_version", ABI_VERSION, RuntimeError,
                           "libd2d_ppo.so ABI mismatch")
        _native.check_version(lib, path, "d2d_ppo_ctl_version", PPO_CTL_VERSION, RuntimeError,
                              "libd2d_ppo.so control-block version mismatch")
        _native.check_version(lib, path, "d2d_ppo_tb_version", PPO_TB_VERSION, RuntimeError,
                              "libd2d_ppo.so truncation-bootstrap version mismatch")
        _PPO_LIB = lib
    return _PPO_LIB


def _ok(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError {rc}")
