"""Evaluation on the device: the reference's ``mode == "test"`` loop (main.py:220-288) with the policy
side of every step -- the actor, its noise, the clip and the first-episode recorder -- in one launch of
``libd2d_eval.so`` (include/d2d_eval.h) next to the env's own step kernel.

``evaluate_policy`` returns what ``harness.run_first_episodes`` returns (``harness.summary``,
``write_results`` and ``plot_flight_paths`` take it unchanged).  The policy noise of global env g at
step t is a Philox draw keyed by (seed, g, t) and the actor's arithmetic is row-invariant, so a batch
sharded over ranks or split into smaller batches flies, bit for bit, the episodes of the unsharded one.
There is no fallback on a HIP batch: a missing library is an error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import abi

ABI_VERSION = 1
NOISE_NONE, NOISE_GIVEN, NOISE_PHILOX = 0, 1, 2
NOISE_TAG = 0x45560000
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_eval.so")

_VP = C.c_void_p


class D2DEvalStepArgs(C.Structure):
    """include/d2d_eval.h ``d2d_eval_step_args``."""
    _fields_ = [(k, C.c_int32) for k in ("n", "t", "info_dim", "act", "noise_mode", "flight_cap")] + \
               [("env_id_base", C.c_int64), ("seed", C.c_uint64)] + \
               [(k, _VP) for k in ("obs", "w1", "b1", "w2", "b2", "w3", "b3", "log_std", "noise", "noise_out", "act_env",
                                   "prev_term", "prev_trunc", "prev_info", "prev_term_obs", "finished", "rows",
                                   "flight", "remaining")]


class EvalError(RuntimeError):
    pass


SIGNATURES = {
    "d2d_eval_abi_version": (C.c_int32, []),
    "d2d_eval_step": (C.c_int32, [C.POINTER(D2DEvalStepArgs), _VP]),
}

_lib = None


def bind(path: str) -> C.CDLL:
    """The library at ``path`` with its signatures set and its ABI version checked."""
    from . import _native

    return _native.bind(path, SIGNATURES, "d2d_eval_abi_version", ABI_VERSION, EvalError)


def load() -> C.CDLL:
    """Load (once) the evaluation library; a first use that finds it missing builds it (hipcc)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            from ._build import build_eval

            build_eval()
        _lib = bind(LIB_PATH)
    return _lib


def _step(lib, args: D2DEvalStepArgs, stream: int) -> None:
    rc = lib.d2d_eval_step(C.byref(args), stream)
    if rc:
        raise EvalError(f"d2d_eval_step: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


def _actor_critic(policy):
    """The ``ActorCritic`` behind a ``ppo.PPO``, or the policy itself."""
    return policy.policy if hasattr(policy, "collect_rollouts") else policy


def actor_tensors(policy, device) -> tuple:
    """(W1, b1, W2, b2, W3, b3, log_std) of an ``ActorCritic``, a ``harness.MlpActor`` or a
    ``ppo.PPO``: float32, contiguous, on ``device`` (no copy when they already are)."""
    p = _actor_critic(policy)
    if hasattr(p, "mlp_extractor"):
        pn = p.mlp_extractor.policy_net
        ts = (pn[0].weight, pn[0].bias, pn[2].weight, pn[2].bias, p.action_net.weight, p.action_net.bias, p.log_std)
    elif hasattr(p, "l0"):
        ts = (p.l0.weight, p.l0.bias, p.l1.weight, p.l1.bias, p.out.weight, p.out.bias, p.log_std)
    else:
        raise TypeError(f"cannot evaluate a {type(policy).__name__}: expected ActorCritic, MlpActor or PPO")
    out = tuple(t.detach().to(device=device, dtype=torch.float32).contiguous() for t in ts)
    shapes = ((64, 27), (64,), (64, 64), (64,), (2, 64), (2,), (2,))
    if tuple(tuple(t.shape) for t in out) != shapes:
        raise ValueError("the evaluation step runs SB3's MlpPolicy actor 27-64-64-2 only")
    return out


def _weights_into(args: D2DEvalStepArgs, ws: tuple) -> None:
    for k, t in zip(("w1", "b1", "w2", "b2", "w3", "b3", "log_std"), ws):
        setattr(args, k, t.data_ptr())


def as_mlp_actor(policy, batch_invariant: bool = False):
    """``policy`` as the ``harness.MlpActor`` the torch loop takes."""
    from .harness import MlpActor

    p = _actor_critic(policy)
    return p if isinstance(p, MlpActor) else MlpActor.from_policy(p, batch_invariant=batch_invariant)


@torch.no_grad()
def act(policy, obs: torch.Tensor, *, deterministic: bool = False, seed: int = 0, t: int = 0, env_id_base: int = 0,
        noise: torch.Tensor | None = None, return_noise: bool = False):
    """The act half alone on a HIP tensor ``obs`` [n, 27]: clip(mean + exp(log_std) z, -1, 1) [n, 2],
    with z = 0 (``deterministic``), ``noise`` [n, 2], or the Philox draw of (seed, env_id_base + i, t).
    ``return_noise``: also the z that was used."""
    if not obs.is_cuda:
        raise ValueError("evaluate.act runs on a HIP device; use the policy's torch forward on the CPU")
    lib = load()
    dev = obs.device
    x = obs.detach().to(torch.float32).contiguous()
    n = int(x.shape[0])
    if x.dim() != 2 or x.shape[1] != abi.OBS_DIM:
        raise ValueError("obs must be [n, 27]")
    out = torch.empty(n, abi.ACT_DIM, dtype=torch.float32, device=dev)
    if n == 0:
        return (out, out.clone()) if return_noise else out
    ws = actor_tensors(policy, dev)
    a = D2DEvalStepArgs(n=n, t=int(t), info_dim=abi.INFO_DIM, act=1, env_id_base=int(env_id_base),
                        seed=int(seed) & (2 ** 64 - 1), obs=x.data_ptr(), act_env=out.data_ptr())
    _weights_into(a, ws)
    z = None
    if deterministic:
        a.noise_mode = NOISE_NONE
    elif noise is not None:
        z = noise.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(z.shape) != (n, abi.ACT_DIM):
            raise ValueError("noise must be [n, 2]")
        a.noise_mode, a.noise = NOISE_GIVEN, z.data_ptr()
    else:
        a.noise_mode = NOISE_PHILOX
    zo = None
    if return_noise:
        zo = torch.zeros(n, abi.ACT_DIM, dtype=torch.float32, device=dev)
        a.noise_out = zo.data_ptr()
    with torch.cuda.device(dev):
        _step(lib, a, torch.cuda.current_stream(dev).cuda_stream)
    return (out, zo) if return_noise else out


def philox_noise_host(seed: int, g, t: int) -> np.ndarray:
    """The host restatement of the library's noise mode 2 (include/d2d_eval.h): float32 [len(g), 2]
    for global env ids ``g`` at step ``t``.  NumPy's float32 log / cos / sin are not the device's, so
    this agrees with the device to a few ulp of r <= 5.9, not bit for bit."""
    g = np.asarray(g, np.uint64).reshape(-1)
    w = _philox4x32(np.stack([g, np.full_like(g, t), np.full_like(g, NOISE_TAG), np.zeros_like(g)]),
                    (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    f = np.float32
    u0 = ((w[0] >> np.uint64(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    u1 = ((w[1] >> np.uint64(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    r = np.sqrt(f(-2.0) * np.log(u0))
    a = f(6.28318530717958647692) * u1
    return np.stack([r * np.cos(a), r * np.sin(a)], -1).astype(f)


def _philox4x32(ctr: np.ndarray, key: tuple) -> np.ndarray:
    """Philox4x32-10 over columns of ``ctr`` (uint64 [4, m] holding 32-bit words): uint64 [4, m]."""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & m32 for c in ctr)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3])


def _records(venv, fin, rows_np, xy_np, nobs) -> dict:
    """The result dict of ``harness.run_first_episodes`` from the recorder's arrays."""
    from .env import info_dicts

    idx = np.flatnonzero(fin)
    recs = [info_dicts(r, nobs) for r in rows_np[idx]]
    out = {
        "successes": int(sum(d["n_successful_runs"] == 1 for d in recs)),
        "fails": int(sum(d["n_failed_runs"] == 1 for d in recs)),
        "collisions": np.array([d["n_collisions"] for d in recs], np.int64),
        "apes": np.array([d["APE"] for d in recs], np.float64),
        "time_spent": np.array([d["env_steps"] for d in recs], np.int64),
        "rewards": np.array([d["total_reward"] for d in recs], np.float64),
        "unfinished": int(len(fin) - len(recs)),
    }
    if xy_np is not None:
        steps = int(out["time_spent"].max()) if len(recs) else 0
        w, h = float(venv.kwargs["screensize_x"]), float(venv.kwargs["screensize_y"])
        xy = xy_np[:steps, idx].astype(np.float64)  # [steps, finished envs, 2]
        fl = np.stack([(xy[..., 0] + 1.0) * w / 2.0, h - (xy[..., 1] + 1.0) * h / 2.0], -1)
        fl[np.arange(steps)[:, None] >= out["time_spent"][None, :]] = np.nan  # after each episode's end
        out["flight_xy"] = fl
        out["screen"] = (w, h)
    return out


@torch.no_grad()
def evaluate_policy(venv, policy, *, deterministic: bool = False, seed: int = 0, max_steps: int | None = None,
                    n_obstacles: int | None = None, flight_paths: bool = False, check_every: int = 16,
                    noise: str = "philox", keep_actions: bool = False) -> dict:
    """Step ``venv`` under ``policy`` (an ``ActorCritic``, a ``harness.MlpActor`` or a ``ppo.PPO``)
    until every env has finished its first episode; the result dict of
    ``harness.run_first_episodes`` (+ ``actions`` [steps, n, 2] with ``keep_actions``: this rank's).

    Per env step: one ``d2d_eval_step`` (the recorder over the previous step's outputs, the actor on
    the env's observation tensor, the noise, the clip), then ``venv.step`` on its action tensor;
    nothing waits for the device except the read-back of the unfinished-env counter every
    ``check_every`` steps.  After the last env step one record-only call digests its outputs.

    ``noise``: "philox" -- env g's draw at step t comes from (seed, g, t) on the device, g counted from
    ``venv.cfg.env_id_base``, so shards of one batch (``env_id_offset``, ``shard.make_shard_venv``)
    fly the unsharded batch's episodes; "torch" -- a seeded ``torch.randn`` of the global batch per step,
    as ``run_first_episodes`` draws it.  With ``torch.distributed`` initialised rank 0 gathers every
    rank's records in global env order, as ``run_first_episodes`` does.

    A batch that is not a HIP ``Drone2dVecEnv`` (the CPU oracle backend of the tests) goes through
    ``harness.run_first_episodes``."""
    from . import harness
    from .env import Drone2dVecEnv

    if noise not in ("philox", "torch"):
        raise ValueError("noise must be 'philox' or 'torch'")
    if not isinstance(venv, Drone2dVecEnv):
        if keep_actions:
            raise ValueError("keep_actions needs a HIP batch")
        return harness.run_first_episodes(venv, as_mlp_actor(policy), deterministic=deterministic, seed=seed,
                                          max_steps=max_steps, n_obstacles=n_obstacles, flight_paths=flight_paths,
                                          check_every=check_every)
    if not venv.with_info:
        raise ValueError("evaluate_policy needs the env's info rows (with_info=True)")
    lib = load()
    dev = venv.device
    dist, rank, world = harness._dist_world()
    n = int(venv.num_envs)
    base = int(venv.cfg.env_id_base)
    offset = base if world > 1 else 0
    n_total = n
    if world > 1:
        counts = [None] * world
        dist.all_gather_object(counts, n)
        n_total = int(sum(counts))
    cap = int(max_steps) if max_steps is not None else int(venv.kwargs["n_steps"]) + 1
    # (info_dicts ignores it; a fresh-curriculum batch has no static scenario to count obstacles of)
    nobs = n_obstacles if n_obstacles is not None else (len(venv.scenarios[0].circles) if venv.scenarios else 0)
    ws = actor_tensors(policy, dev)
    with torch.cuda.device(dev):
        obs = venv.reset(seed=seed)
        finished = torch.zeros(n, dtype=torch.uint8, device=dev)
        rows = torch.zeros(n, abi.INFO_DIM, dtype=torch.float32, device=dev)
        remaining = torch.full((1,), n, dtype=torch.int32, device=dev)
        act_env = torch.empty(n, abi.ACT_DIM, dtype=torch.float32, device=dev)
        pos = torch.full((cap, n, 2), float("nan"), dtype=torch.float32, device=dev) if flight_paths else None
        a = D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, flight_cap=cap, env_id_base=base,
                            seed=int(seed) & (2 ** 64 - 1), act_env=act_env.data_ptr())
        _weights_into(a, ws)
        gen = z = None
        if deterministic:
            a.noise_mode = NOISE_NONE
        elif noise == "philox":
            a.noise_mode = NOISE_PHILOX
        else:
            a.noise_mode = NOISE_GIVEN
            gen = torch.Generator(device=dev).manual_seed(seed)
        actions = []
        stream = torch.cuda.current_stream(dev).cuda_stream
        for t in range(cap + 1):
            last = t == cap
            a.t, a.act, a.obs = t, 0 if last else 1, obs.data_ptr()
            if gen is not None and not last:
                z = torch.randn((n_total, 2), device=dev, dtype=torch.float32, generator=gen)[offset:offset + n]
                z = z.contiguous()
                a.noise = z.data_ptr()
            _step(lib, a, stream)
            if keep_actions and not last:
                actions.append(act_env.clone())
            if last or (t and t % check_every == 0 and int(remaining.item()) == 0):
                break
            # the env's outputs are double-buffered: this step's set stays valid through the next call
            obs, _, term, trunc, info = venv.step(act_env)
            a.prev_term, a.prev_trunc, a.prev_info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
            a.prev_term_obs = venv.terminal_obs.data_ptr()
            a.finished, a.rows, a.remaining = finished.data_ptr(), rows.data_ptr(), remaining.data_ptr()
            a.flight = pos.data_ptr() if pos is not None else None
        steps = t
        fin = finished.cpu().numpy().astype(bool)
        rows_np = rows.cpu().numpy()
        xy_np = pos.cpu().numpy() if pos is not None else None
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, (offset, fin, rows_np, xy_np))
        parts.sort(key=lambda p: p[0])
        fin = np.concatenate([p[1] for p in parts])
        rows_np = np.concatenate([p[2] for p in parts])
        if xy_np is not None:
            T = max(p[3].shape[0] for p in parts)
            xy_np = np.concatenate([p[3][:T] for p in parts], 1)
    out = _records(venv, fin, rows_np, xy_np, nobs)
    if keep_actions:
        # the call that found every env finished had already written the next step's actions: drop them
        out["actions"] = (torch.stack(actions[:steps]) if steps else torch.empty(0, n, 2, device=dev)).cpu().numpy()
    return out


__all__ = ["evaluate_policy", "act", "actor_tensors", "as_mlp_actor", "philox_noise_host", "load", "bind", "EvalError",
           "D2DEvalStepArgs"]
