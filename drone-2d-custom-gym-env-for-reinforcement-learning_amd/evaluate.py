"""Evaluation on the device: the reference's ``mode == "test"`` loop (main.py:220-288) with the policy
side of every step -- the actor, its noise, the clip and the first-episode recorder -- in one launch of
``libd2d_eval.so`` (include/d2d_eval.h) next to the env's own step kernel.

``evaluate_policy`` returns what ``harness.run_first_episodes`` returns (``harness.summary``,
``write_results`` and ``plot_flight_paths`` take it unchanged).  The policy noise of global env g at
step t is a Philox draw keyed by (seed, g, t) and the actor's arithmetic is row-invariant, so a batch
sharded over ranks or split into smaller batches flies, bit for bit, the episodes of the unsharded one.
There is no fallback on a HIP batch: a missing library is an error.

``graph=True`` (``EvalLoop``) flies the same loop as one captured segment of (``d2d_eval_step_seq``,
``venv.step``) iterations replayed: the sequenced step reads its call index from device memory, so the
index moves on from replay to replay.  The results are the eager loop's bit for bit; whether it is
faster is measured in DESIGN.md "The replayed loop".
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
BANK_VERSION = 1
SEQ_VERSION = 1
BANK_STRIDE = 6084  # floats per policy in a bank: W1, b1, W2, b2, W3, b3, log_std (include/d2d_eval.h)
_BANK_SHAPES = ((64, 27), (64,), (64, 64), (64,), (2, 64), (2,), (2,))
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libd2d_eval.so")

_VP = C.c_void_p


class D2DEvalStepArgs(C.Structure):
    """include/d2d_eval.h ``d2d_eval_step_args``."""
    _fields_ = [(k, C.c_int32) for k in ("n", "t", "info_dim", "act", "noise_mode", "flight_cap")] + \
               [("env_id_base", C.c_int64), ("seed", C.c_uint64)] + \
               [(k, _VP) for k in ("obs", "w1", "b1", "w2", "b2", "w3", "b3", "log_std", "noise", "noise_out", "act_env",
                                   "prev_term", "prev_trunc", "prev_info", "prev_term_obs", "finished", "rows",
                                   "flight", "remaining")]


class D2DEvalBank(C.Structure):
    """include/d2d_eval.h ``d2d_eval_bank``."""
    _fields_ = [("n_policies", C.c_int32), ("pad", C.c_int32), ("params", _VP), ("env_policy", _VP)]


class EvalError(RuntimeError):
    pass


SIGNATURES = {
    "d2d_eval_abi_version": (C.c_int32, []),
    "d2d_eval_step": (C.c_int32, [C.POINTER(D2DEvalStepArgs), _VP]),
    "d2d_eval_bank_version": (C.c_int32, []),
    "d2d_eval_step_bank": (C.c_int32, [C.POINTER(D2DEvalStepArgs), C.POINTER(D2DEvalBank), _VP]),
    "d2d_eval_seq_version": (C.c_int32, []),
    "d2d_eval_step_seq": (C.c_int32, [C.POINTER(D2DEvalStepArgs), C.POINTER(D2DEvalBank), _VP, _VP]),
}

_lib = None


def bind(path: str) -> C.CDLL:
    """The library at ``path`` with its signatures set and its ABI, bank and sequenced-step versions checked."""
    from . import _native

    lib = _native.bind(path, SIGNATURES, "d2d_eval_abi_version", ABI_VERSION, EvalError)
    _native.check_version(lib, path, "d2d_eval_bank_version", BANK_VERSION, EvalError, None)
    _native.check_version(lib, path, "d2d_eval_seq_version", SEQ_VERSION, EvalError, None)
    return lib


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


def _step_bank(lib, args: D2DEvalStepArgs, bank: D2DEvalBank, stream: int) -> None:
    rc = lib.d2d_eval_step_bank(C.byref(args), C.byref(bank), stream)
    if rc:
        raise EvalError(f"d2d_eval_step_bank: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


def _step_seq(lib, args: D2DEvalStepArgs, bank: D2DEvalBank | None, t_dev: int, stream: int) -> None:
    """``d2d_eval_step_seq``: the call index is the device int32 at ``t_dev``; two launches."""
    rc = lib.d2d_eval_step_seq(C.byref(args), C.byref(bank) if bank is not None else None, t_dev, stream)
    if rc:
        raise EvalError(f"d2d_eval_step_seq: hipError {rc}" + (" (contradictory arguments)" if rc == 1 else ""))


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
    if tuple(tuple(t.shape) for t in out) != _BANK_SHAPES:
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
    return _act(obs, lambda dev: actor_tensors(policy, dev), None, None, deterministic, seed, t, env_id_base, noise,
                return_noise)


def _act(obs, weights, bank, env_policy, deterministic, seed, t, env_id_base, noise, return_noise):
    """``act`` under one actor (``weights(device)`` -> its seven tensors) or under a ``PolicyBank``
    with its env -> policy map."""
    if not obs.is_cuda:
        raise ValueError("evaluate.act runs on a HIP device; use the policy's torch forward on the CPU")
    lib = load()
    dev = obs.device
    x = obs.detach().to(torch.float32).contiguous()
    n = int(x.shape[0])
    if x.dim() != 2 or x.shape[1] != abi.OBS_DIM:
        raise ValueError("obs must be [n, 27]")
    out = torch.empty(n, abi.ACT_DIM, dtype=torch.float32, device=dev)
    if bank is not None:
        bank = bank.to(dev)
        ep = torch.from_numpy(check_env_policy(env_policy, n, bank.n_policies)).to(dev)
    if n == 0:
        return (out, out.clone()) if return_noise else out
    a = D2DEvalStepArgs(n=n, t=int(t), info_dim=abi.INFO_DIM, act=1, env_id_base=int(env_id_base),
                        seed=int(seed) & (2 ** 64 - 1), obs=x.data_ptr(), act_env=out.data_ptr())
    if bank is None:
        ws = weights(dev)
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
        stream = torch.cuda.current_stream(dev).cuda_stream
        if bank is None:
            _step(lib, a, stream)
        else:
            _step_bank(lib, a, bank.c_bank(ep), stream)
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


def _check_maps(maps):
    """``maps`` (None, a grid size or (Gy, Gx)) as None or (Gy, Gx); with more than one rank a ``ValueError``."""
    if maps is None:
        return None
    from . import harness, heatmap

    grid = heatmap.parse_grid(maps)
    if harness._dist_world()[2] > 1:
        raise ValueError("maps with more than one rank: summing the shards' planes is not built; evaluate on one rank")
    return grid


def _group_maps(counts: dict, g: int, idx, spawn_obs, fin, rows_np, xy_np) -> dict:
    """The ``"maps"`` entry of a result dict: group ``g``'s planes [6, Gy, Gx] and ``outside`` [6], the
    reset positions of its envs ``idx`` and, with a flight buffer, what ``heatmap.from_result`` recomputes
    the planes from (the recorder's raw buffer, not trimmed: an unfinished env flew all of it)."""
    out = {"planes": counts["planes"][g], "outside": counts["outside"][g], "spawn_obs": spawn_obs[idx]}
    if xy_np is not None:
        # (a group that is the whole batch takes the buffer itself: a fancy index would copy all of it)
        whole = len(idx) == xy_np.shape[1]
        out.update(flight_obs=xy_np if whole else xy_np[:, idx], finished=fin[idx], rows=rows_np[idx])
    return out


def _host_maps(grid, raw: dict, env_group, n_groups: int) -> dict:
    """The planes of a batch flown by ``harness.run_first_episodes`` (``records=False``, with its flight buffer)."""
    from . import heatmap

    return heatmap.from_flight(raw["spawn_xy"], raw["xy"], raw["finished"], raw["rows"], env_group, n_groups, grid)


@torch.no_grad()
def evaluate_policy(venv, policy, *, deterministic: bool = False, seed: int = 0, max_steps: int | None = None,
                    n_obstacles: int | None = None, flight_paths: bool = False, check_every: int = 16,
                    noise: str = "philox", keep_actions: bool = False, graph: bool = False, maps=None,
                    disturb=None) -> dict:
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

    ``graph``: replay the loop as a captured HIP graph (a throw-away ``EvalLoop``): the same result
    dict, bit for bit.  It needs a HIP batch, ``noise="philox"``, ``keep_actions=False`` and one rank.

    ``maps`` (a grid size or (Gy, Gx)): also bin the episodes into arena maps while they fly
    (``heatmap.ArenaMaps``, one more launch per env step); the result gains ``"maps"``: ``planes`` uint32
    [6, Gy, Gx], ``outside`` [6], the reset positions ``spawn_obs`` and, with ``flight_paths``, the
    recorder's raw buffers (``heatmap.from_result`` recomputes the planes from them).  Every other key is
    what it is without ``maps``.  One rank only.

    ``disturb`` (a ``disturb.Disturbance``, or a ``disturb.Disturber`` built for this batch): fly a
    disturbed world -- the policy sees ``Disturber.obs`` of the observations and the env gets
    ``Disturber.act`` of the actions, two more launches per env step, and the one evaluation call becomes a
    record-only call on the true observations and an act-only call on the disturbed ones.  The recorder,
    ``flight_paths`` and ``maps`` see the true flight; ``actions`` are the applied ones.  Not with ``graph``.

    A batch that is not a HIP ``Drone2dVecEnv`` (the CPU oracle backend of the tests) goes through
    ``harness.run_first_episodes`` (and its maps through ``heatmap.from_flight`` of the flight buffer)."""
    from . import harness
    from .env import Drone2dVecEnv

    if noise not in ("philox", "torch"):
        raise ValueError("noise must be 'philox' or 'torch'")
    if graph:
        _check_graph(venv, noise, keep_actions, disturb)
    grid = _check_maps(maps)
    n = int(venv.num_envs)
    if disturb is not None:
        from .disturb import make_disturber

        disturb = make_disturber(disturb, venv, seed)
    if not isinstance(venv, Drone2dVecEnv):
        if keep_actions:
            raise ValueError("keep_actions needs a HIP batch")
        kw = dict(deterministic=deterministic, seed=seed, max_steps=max_steps, n_obstacles=n_obstacles,
                  check_every=check_every)
        if disturb is not None:
            kw["disturb"] = disturb
        if grid is None:
            return harness.run_first_episodes(venv, as_mlp_actor(policy), flight_paths=flight_paths, **kw)
        raw = harness.run_first_episodes(venv, as_mlp_actor(policy), flight_paths=True, records=False, **kw)
        xy_np = raw["xy"] if flight_paths else None
        out = _records(venv, raw["finished"], raw["rows"], xy_np, raw["n_obstacles"])
        out["maps"] = _group_maps(_host_maps(grid, raw, None, 1), 0, np.arange(n), raw["spawn_xy"], raw["finished"],
                                  raw["rows"], xy_np)
        return out
    am = None
    if grid is not None:
        from . import heatmap

        am = heatmap.ArenaMaps(venv, grid, cap=max_steps)
    fin, rows_np, xy_np, nobs, actions, _ = _fly(venv, actor_tensors(policy, venv.device), None, deterministic, seed,
                                                 max_steps, n_obstacles, flight_paths, check_every, noise, keep_actions,
                                                 graph=graph, maps=am, disturb=disturb)
    out = _records(venv, fin, rows_np, xy_np, nobs)
    if keep_actions:
        out["actions"] = actions
    if am is not None:
        out["maps"] = _group_maps(am.counts(), 0, np.arange(n), am.spawn_obs.cpu().numpy(), fin, rows_np, xy_np)
        am.close()
    return out


def _check_graph(venv, noise, keep_actions, disturb=None) -> None:
    """What ``graph=True`` cannot do, as a ``ValueError``."""
    from . import harness
    from .env import Drone2dVecEnv

    if disturb is not None:
        raise ValueError("graph=True with disturb: the replayed loop takes its step index from device memory and the "
                         "disturbance calls take it by value; fly the disturbed loop eagerly")
    if not isinstance(venv, Drone2dVecEnv):
        raise ValueError("graph=True needs a HIP Drone2dVecEnv: the replayed loop is the device's")
    if noise != "philox":
        raise ValueError("graph=True with noise='torch': a host draw per step cannot be captured; use noise='philox'")
    if keep_actions:
        raise ValueError("graph=True with keep_actions=True: the replayed loop keeps no per-step copies")
    if harness._dist_world()[2] > 1:
        raise ValueError("graph=True with more than one rank: the gather of the records stays eager and the replayed "
                         "loop is built for one rank")


def _fly(venv, ws, bank, deterministic, seed, max_steps, n_obstacles, flight_paths, check_every, noise, keep_actions,
         extra=(), graph=False, maps=None, disturb=None):
    """The closed loop of ``evaluate_policy`` on a HIP batch under one actor (``ws``, its seven tensors)
    or a policy bank (``bank``: a ``D2DEvalBank`` whose tensors the caller keeps alive): the recorder's
    arrays over the whole batch in global env order (gathered over the ranks, and with them the
    per-env arrays in ``extra``), the obstacle count, and this rank's actions [steps, n, 2].  ``maps``: a
    ``heatmap.ArenaMaps`` of this batch, cleared, begun after the reset and stepped after every env step.
    ``disturb``: a ``disturb.Disturber`` of this batch, rewound; the actions are then the applied ones."""
    from . import harness

    if not venv.with_info:
        raise ValueError("evaluate_policy needs the env's info rows (with_info=True)")
    if graph:
        _check_graph(venv, noise, keep_actions, disturb)
        loop = EvalLoop(venv, None, deterministic=deterministic, flight_paths=flight_paths, check_every=check_every,
                        graph=True, max_steps=max_steps, n_obstacles=n_obstacles, _actor=(ws, bank), _maps=maps)
        return loop.run(seed, extra=extra)
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
    step = (lambda a, st: _step(lib, a, st)) if bank is None else (lambda a, st: _step_bank(lib, a, bank, st))
    with torch.cuda.device(dev):
        obs = venv.reset(seed=seed)
        if maps is not None:
            maps.clear()
            maps.begin(obs)
        finished = torch.zeros(n, dtype=torch.uint8, device=dev)
        rows = torch.zeros(n, abi.INFO_DIM, dtype=torch.float32, device=dev)
        remaining = torch.full((1,), n, dtype=torch.int32, device=dev)
        act_env = torch.empty(n, abi.ACT_DIM, dtype=torch.float32, device=dev)
        pos = torch.full((cap, n, 2), float("nan"), dtype=torch.float32, device=dev) if flight_paths else None
        a = D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, flight_cap=cap, env_id_base=base,
                            seed=int(seed) & (2 ** 64 - 1), act_env=act_env.data_ptr())
        if bank is None:
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
            if disturb is None:
                step(a, stream)
            else:
                _disturbed_step(step, a, stream, disturb, obs, act_env, t, last)
            if keep_actions and not last:
                actions.append(act_env.clone())
            if last or (t and t % check_every == 0 and int(remaining.item()) == 0):
                break
            # the env's outputs are double-buffered: this step's set stays valid through the next call
            obs, _, term, trunc, info = venv.step(act_env)
            if maps is not None:
                maps.step(obs, term, trunc, venv.terminal_obs, info)
            a.prev_term, a.prev_trunc, a.prev_info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
            a.prev_term_obs = venv.terminal_obs.data_ptr()
            a.finished, a.rows, a.remaining = finished.data_ptr(), rows.data_ptr(), remaining.data_ptr()
            a.flight = pos.data_ptr() if pos is not None else None
        steps = t
        fin = finished.cpu().numpy().astype(bool)
        rows_np = rows.cpu().numpy()
        xy_np = pos.cpu().numpy() if pos is not None else None
    extra = tuple(np.asarray(e) for e in extra)
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, (offset, fin, rows_np, xy_np, extra))
        parts.sort(key=lambda p: p[0])
        fin = np.concatenate([p[1] for p in parts])
        rows_np = np.concatenate([p[2] for p in parts])
        if xy_np is not None:
            T = max(p[3].shape[0] for p in parts)
            xy_np = np.concatenate([p[3][:T] for p in parts], 1)
        extra = tuple(np.concatenate([p[4][k] for p in parts]) for k in range(len(extra)))
    if keep_actions:
        # the call that found every env finished had already written the next step's actions: drop them
        actions = (torch.stack(actions[:steps]) if steps else torch.empty(0, n, 2, device=dev)).cpu().numpy()
    return fin, rows_np, xy_np, nobs, actions, extra


_RECORD_FIELDS = ("prev_term", "prev_trunc", "prev_info", "prev_term_obs", "finished", "rows", "flight", "remaining")


def _disturbed_step(step, a: D2DEvalStepArgs, stream: int, disturb, obs, act_env, t: int, last: bool) -> None:
    """One policy step of ``_fly`` under a ``disturb.Disturber``, in place of its one evaluation call: the
    record half alone on the true observations (from step 1 on: ``a`` holds the previous env step's
    outputs), then -- unless this is the call after the last env step -- the disturbed observations, the act
    half alone on them, and the disturbance of the actions it wrote.  ``a`` comes back as it was given."""
    if t >= 1:
        a.act = 0
        step(a, stream)
    if last:
        return
    record = [getattr(a, k) for k in _RECORD_FIELDS]
    for k in _RECORD_FIELDS:
        setattr(a, k, None)
    a.act, a.obs = 1, disturb.obs(obs, t).data_ptr()
    step(a, stream)
    disturb.act(act_env, t)
    a.obs = obs.data_ptr()
    for k, v in zip(_RECORD_FIELDS, record):
        setattr(a, k, v)


class EvalLoop:
    """The closed loop of ``evaluate_policy`` / ``evaluate_policies`` kept for many evaluations of one
    batch: it owns the recorder's buffers, the device call index ``t_dev`` of ``d2d_eval_step_seq`` and,
    with ``graph``, one captured segment of ``K`` iterations of (``d2d_eval_step_seq``, ``venv.step``),
    ``K`` = ``check_every`` rounded up to even (the env's outputs are double-buffered: an even segment
    ends on the buffer parity it began on, so it can be replayed back to back).

    ``policy_or_bank``: one policy (``env_policy`` None) or a ``PolicyBank`` / list of policies with
    the env -> policy map.  ``run(seed)`` rewinds -- the env's episode counters put back to what the
    first run found (``set_state``: they key the spawn draws), ``venv.reset(seed)``, buffers cleared,
    ``t_dev`` zeroed -- flies, and returns ``_fly``'s arrays, bit for bit those of the eager by-value
    loop on a batch in the first run's state:

      step 0 eagerly (no record half); on the first run one segment eagerly (library warm-up), then the
      capture; replays, each followed by a read-back of ``remaining``, until it is 0 or fewer than K
      steps are left before the cap; the tail and the record-only call eagerly.

    The segment holds the actor's tensors by address and ``actor_tensors`` makes no copy of float32
    device parameters, so a replay reads the live weights; ``run`` recaptures when one of the seven
    addresses (the bank's one), the seed (the env step takes it by value) or the env's ``generation``
    is not what the segment was captured with.  ``graph=False``: every run is ``_fly``'s eager loop.

    ``maps`` (a grid size or (Gy, Gx)): the loop owns a ``heatmap.ArenaMaps`` (``self.maps``; one group,
    or one per policy of the bank): every ``run`` clears it and begins it eagerly after the reset, and its
    step call follows every env step, inside the captured segment too; ``self.maps.counts()`` after a
    run are that run's planes.

    ``disturb`` (``graph=False`` only): as in ``evaluate_policy``; a ``Disturbance`` becomes a ``Disturber`` the
    loop keeps (``self.disturb``), keyed anew by every run's seed."""

    def __init__(self, venv, policy_or_bank, env_policy=None, *, deterministic: bool = False,
                 flight_paths: bool = False, check_every: int = 16, graph: bool = True, max_steps: int | None = None,
                 n_obstacles: int | None = None, maps=None, disturb=None, _actor=None, _maps=None):
        from .env import Drone2dVecEnv

        if graph:
            _check_graph(venv, "philox", False, disturb)
        elif not isinstance(venv, Drone2dVecEnv):
            raise ValueError("EvalLoop needs a HIP Drone2dVecEnv")
        self.disturb = self._own_disturb = None
        if disturb is not None:
            from .disturb import Disturbance, make_disturber

            self.disturb = make_disturber(disturb, venv, 0)
            self._own_disturb = isinstance(disturb, Disturbance)  # then its key follows run's seed
        if not venv.with_info:
            raise ValueError("evaluate_policy needs the env's info rows (with_info=True)")
        if int(check_every) < 1:
            raise ValueError("check_every must be at least 1")
        self.venv, self.graph = venv, bool(graph)
        self.deterministic, self.flight_paths, self.check_every = bool(deterministic), bool(flight_paths), int(check_every)
        self.max_steps, self.n_obstacles = max_steps, n_obstacles
        self.policy = self.bank = self._ep = None
        self._fixed = _actor  # _fly's (ws, c_bank): tensors the caller keeps alive
        if _actor is None:
            if env_policy is None:
                self.policy = policy_or_bank
            else:
                self.bank = _as_bank(policy_or_bank).to(venv.device)
                self._ep = torch.from_numpy(check_env_policy(env_policy, int(venv.num_envs),
                                                             self.bank.n_policies)).to(venv.device)
        self.maps = _maps  # _fly's ArenaMaps, or the loop's own
        grid = _check_maps(maps)
        if grid is not None and _maps is None:
            from . import heatmap

            groups = self._ep.cpu().numpy() if self._ep is not None else None
            self.maps = heatmap.ArenaMaps(venv, grid, groups, self.bank.n_policies if self.bank is not None else None,
                                          cap=max_steps)
        self.K = self.check_every + (self.check_every & 1)
        self.captures = 0       # segments captured so far (1 after any number of runs of unmoved weights)
        self._g = None
        self._key = None        # what the segment was captured with
        self._bufs = None
        self._k0 = None
        self._snap = None       # the env's state before the first run's reset

    def _actor(self):
        """(ws, c_bank, key): the seven tensors or the bank record, and the addresses a capture bakes in."""
        if self._fixed is not None:
            ws, cb = self._fixed
        elif self.bank is not None:
            ws, cb = None, self.bank.c_bank(self._ep)
        else:
            ws, cb = actor_tensors(self.policy, self.venv.device), None
        key = tuple(t.data_ptr() for t in ws) if ws is not None else (cb.params, cb.env_policy, cb.n_policies)
        return ws, cb, key

    def _alloc(self, cap):
        n, dev = int(self.venv.num_envs), self.venv.device
        self._bufs = dict(
            finished=torch.zeros(n, dtype=torch.uint8, device=dev),
            rows=torch.zeros(n, abi.INFO_DIM, dtype=torch.float32, device=dev),
            remaining=torch.full((1,), n, dtype=torch.int32, device=dev),
            act_env=torch.empty(n, abi.ACT_DIM, dtype=torch.float32, device=dev),
            t_dev=torch.zeros(1, dtype=torch.int32, device=dev),
            pos=torch.full((cap, n, 2), float("nan"), dtype=torch.float32, device=dev) if self.flight_paths else None)

    @torch.no_grad()
    def run(self, seed: int = 0, extra=()):
        venv = self.venv
        ws, cb, key = self._actor()
        # the env's episode counters key its spawn draws and a reset moves them on: put them back to
        # where the first run found them, so that every run flies the first run's episodes
        if self._snap is None:
            self._snap = venv.get_state()
        else:
            venv.set_state(*self._snap)
        if not self.graph:
            if self.disturb is not None:
                self.disturb.reset()
                if self._own_disturb:
                    self.disturb.seed = int(seed) & (2 ** 64 - 1)
            return _fly(venv, ws, cb, self.deterministic, seed, self.max_steps, self.n_obstacles, self.flight_paths,
                        self.check_every, "philox", False, extra, maps=self.maps, disturb=self.disturb)
        lib = load()
        dev = venv.device
        n = int(venv.num_envs)
        cap = int(self.max_steps) if self.max_steps is not None else int(venv.kwargs["n_steps"]) + 1
        nobs = self.n_obstacles if self.n_obstacles is not None else (
            len(venv.scenarios[0].circles) if venv.scenarios else 0)
        K = self.K
        with torch.cuda.device(dev):
            if self._bufs is None:
                self._alloc(cap)
                self._k0 = venv._k  # the output-buffer parity every run starts on (the segment's addresses)
            B = self._bufs
            key = (key, int(seed), venv.generation)
            if key != self._key:
                self._g = None
            self._ws = ws  # (alive while the segment points at them)
            venv._k = self._k0
            obs = venv.reset(seed=seed)
            hm = self.maps
            if hm is not None:
                hm.clear()
                hm.begin(obs)
            B["finished"].zero_()
            B["rows"].zero_()
            B["remaining"].fill_(n)
            B["t_dev"].zero_()
            if B["pos"] is not None:
                B["pos"].fill_(float("nan"))
            a = D2DEvalStepArgs(n=n, info_dim=abi.INFO_DIM, flight_cap=cap, env_id_base=int(venv.cfg.env_id_base),
                                seed=int(seed) & (2 ** 64 - 1), act_env=B["act_env"].data_ptr(), act=1,
                                noise_mode=NOISE_NONE if self.deterministic else NOISE_PHILOX, obs=obs.data_ptr())
            if ws is not None:
                _weights_into(a, ws)
            t_dev = B["t_dev"].data_ptr()

            def env_step():
                # the env's outputs are double-buffered: this step's set stays valid through the next call
                o, _, term, trunc, info = venv.step(B["act_env"])
                if hm is not None:
                    hm.step(o, term, trunc, venv.terminal_obs, info)
                a.obs = o.data_ptr()
                a.prev_term, a.prev_trunc, a.prev_info = term.data_ptr(), trunc.data_ptr(), info.data_ptr()
                a.prev_term_obs = venv.terminal_obs.data_ptr()
                a.finished, a.rows, a.remaining = B["finished"].data_ptr(), B["rows"].data_ptr(), B["remaining"].data_ptr()
                a.flight = B["pos"].data_ptr() if B["pos"] is not None else None

            def segment():
                for _ in range(K):
                    _step_seq(lib, a, cb, t_dev, torch.cuda.current_stream(dev).cuda_stream)
                    env_step()

            # step 0: no record half (the prev_* pointers are still NULL)
            _step_seq(lib, a, cb, t_dev, torch.cuda.current_stream(dev).cuda_stream)
            env_step()
            done = 1  # env steps taken = the next call's index
            left = n
            if self._g is None and done + K <= cap:
                segment()  # eagerly first: the library's kernels loaded before the capture
                done += K
                torch.cuda.synchronize(dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    segment()  # (recorded, not run; K is even, so `a` is back at this parity's pointers)
                self._g, self._key = g, key
                self.captures += 1
                left = int(B["remaining"].item())
            while left and done + K <= cap:
                self._g.replay()
                done += K
                left = int(B["remaining"].item())
            if left:
                while done < cap:  # the tail: fewer than K steps before the cap
                    _step_seq(lib, a, cb, t_dev, torch.cuda.current_stream(dev).cuda_stream)
                    env_step()
                    done += 1
            a.act = 0  # the record-only call over the last env step's outputs
            _step_seq(lib, a, cb, t_dev, torch.cuda.current_stream(dev).cuda_stream)
            fin = B["finished"].cpu().numpy().astype(bool)
            rows_np = B["rows"].cpu().numpy()
            xy_np = B["pos"].cpu().numpy() if B["pos"] is not None else None
        return fin, rows_np, xy_np, nobs, [], tuple(np.asarray(e) for e in extra)


# ---------------------------------------------------------------- the policy bank: many agents in one batch
class PolicyBank:
    """P actors packed for ``d2d_eval_step_bank``: ``params`` float32 [P, 6084], policy p's row holding
    W1, b1, W2, b2, W3, b3, log_std in the header's order.  ``policies``: each an ``ActorCritic``, a
    ``harness.MlpActor``, a ``ppo.PPO`` or the path of an agent zip (``ActorCritic.from_sb3_zip``);
    ``names``: one per policy, unique (default: a zip's file name without its extension, else
    ``policy_<p>``); ``device``: default the current HIP device, the CPU without one."""

    def __init__(self, policies, names=None, device=None):
        from .policy import ActorCritic

        policies = list(policies)
        if not policies:
            raise ValueError("a policy bank needs at least one policy")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        if names is None:
            names = [os.path.splitext(os.path.basename(os.fspath(p)))[0] if isinstance(p, (str, os.PathLike))
                     else f"policy_{k}" for k, p in enumerate(policies)]
        self.names = [str(s) for s in names]
        if len(self.names) != len(policies) or len(set(self.names)) != len(policies):
            raise ValueError("names must be one unique name per policy")
        rows = []
        for p in policies:
            if isinstance(p, (str, os.PathLike)):
                p = ActorCritic.from_sb3_zip(os.fspath(p))
            rows.append(torch.cat([t.reshape(-1) for t in actor_tensors(p, "cpu")]))
        self.params = torch.stack(rows).to(device).contiguous()
        assert self.params.shape[1] == BANK_STRIDE

    @property
    def n_policies(self) -> int:
        return int(self.params.shape[0])

    @property
    def device(self) -> torch.device:
        return self.params.device

    def __len__(self) -> int:
        return self.n_policies

    def to(self, device) -> "PolicyBank":
        """This bank on ``device`` (itself when it already is there)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.params.device:
            return self
        other = object.__new__(PolicyBank)
        other.names, other.params = self.names, self.params.to(device)
        return other

    def tensors(self, p: int) -> tuple:
        """(W1, b1, W2, b2, W3, b3, log_std) of policy ``p``: views of its row of ``params``."""
        row, out, o = self.params[p], [], 0
        for shape in _BANK_SHAPES:
            k = int(np.prod(shape))
            out.append(row[o:o + k].view(shape))
            o += k
        return tuple(out)

    def mlp_actor(self, p: int, batch_invariant: bool = False):
        """Policy ``p`` as a ``harness.MlpActor`` (a copy, on the CPU)."""
        from .harness import MlpActor

        keys = ("mlp_extractor_policy_net_0_weight", "mlp_extractor_policy_net_0_bias",
                "mlp_extractor_policy_net_2_weight", "mlp_extractor_policy_net_2_bias", "action_net_weight",
                "action_net_bias", "log_std")
        return MlpActor({k: t.cpu().numpy() for k, t in zip(keys, self.tensors(p))}, batch_invariant=batch_invariant)

    def c_bank(self, env_policy: torch.Tensor) -> D2DEvalBank:
        """The ABI record over ``params`` and an int32 map on the bank's device (the caller keeps both alive)."""
        assert env_policy.dtype == torch.int32 and env_policy.device == self.params.device and env_policy.is_contiguous()
        return D2DEvalBank(n_policies=self.n_policies, params=self.params.data_ptr(), env_policy=env_policy.data_ptr())


def _as_bank(bank) -> PolicyBank:
    return bank if isinstance(bank, PolicyBank) else PolicyBank(bank)


def check_env_policy(env_policy, n: int, n_policies: int) -> np.ndarray:
    """``env_policy`` as a contiguous int32 array [n] with every value in [0, P), or a ``ValueError``:
    the library skips an env whose id is outside the bank, so such a map is refused on the host."""
    ep = env_policy.detach().cpu().numpy() if isinstance(env_policy, torch.Tensor) else np.asarray(env_policy)
    if ep.dtype.kind not in "iu":
        raise ValueError("env_policy must be an integer array")
    if ep.shape != (n,):
        raise ValueError(f"env_policy must have shape [{n}]")
    if n and (int(ep.min()) < 0 or int(ep.max()) >= n_policies):
        raise ValueError(f"env_policy values must lie in [0, {n_policies})")
    return np.ascontiguousarray(ep, dtype=np.int32)


@torch.no_grad()
def act_bank(bank, obs: torch.Tensor, env_policy, *, deterministic: bool = False, seed: int = 0, t: int = 0,
             env_id_base: int = 0, noise: torch.Tensor | None = None, return_noise: bool = False):
    """``act`` with env i under policy ``env_policy[i]`` of ``bank``, one launch: row i is, bit for bit,
    row i of ``act(policy env_policy[i], obs, ...)``."""
    return _act(obs, None, _as_bank(bank), env_policy, deterministic, seed, t, env_id_base, noise, return_noise)


class BankActor(torch.nn.Module):
    """The bank for the torch loop (``harness.run_first_episodes``): ``act`` applies each policy's
    ``MlpActor`` to that policy's rows and scatters the results back.  The actors are
    ``batch_invariant``, so a row's action does not depend on how many rows share its policy."""

    def __init__(self, bank: PolicyBank, env_policy):
        super().__init__()
        self.actors = torch.nn.ModuleList(bank.mlp_actor(p, batch_invariant=True) for p in range(bank.n_policies))
        ep = torch.from_numpy(check_env_policy(env_policy, len(env_policy), bank.n_policies)).long()
        self.register_buffer("env_policy", ep)

    @torch.no_grad()
    def act(self, obs: torch.Tensor, deterministic: bool = False, generator: torch.Generator | None = None,
            noise: torch.Tensor | None = None):
        if not deterministic and noise is None:
            noise = torch.randn((obs.shape[0], 2), device=obs.device, dtype=obs.dtype, generator=generator)
        out = torch.empty(obs.shape[0], 2, dtype=obs.dtype, device=obs.device)
        for p, actor in enumerate(self.actors):
            idx = torch.nonzero(self.env_policy == p).squeeze(1)
            if len(idx):
                out[idx] = actor.act(obs[idx], deterministic=deterministic, noise=None if deterministic else noise[idx])
        return out


@torch.no_grad()
def evaluate_policies(venv, bank, env_policy, *, split=None, deterministic: bool = False, seed: int = 0,
                      max_steps: int | None = None, n_obstacles: int | None = None, flight_paths: bool = False,
                      check_every: int = 16, noise: str = "philox", keep_actions: bool = False, graph: bool = False,
                      maps=None, disturb=None):
    """``evaluate_policy`` for a batch whose envs belong to different agents: env i flies under policy
    ``env_policy[i]`` of ``bank`` (a ``PolicyBank`` or a list of policies), one ``d2d_eval_step_bank``
    per env step.  Returns one result dict per policy (a list), each what ``evaluate_policy`` returns,
    built from that policy's envs in env order: ``flight_xy`` trimmed to their longest episode,
    ``actions`` their columns.  ``split``: an int array [n] of labels (a scenario index, say); the
    result is then a dict keyed (policy, label) over the pairs the batch holds.

    Env i's episode is, bit for bit, the one ``evaluate_policy`` flies it under its policy alone in the
    same batch: the actor is row-invariant across the bank, and noise and spawns are keyed by global
    env id.  Under ``torch.distributed`` every rank passes its shard's slice of the map (and of
    ``split``); the records are gathered in global env order and split afterwards.  A batch that is not
    a HIP ``Drone2dVecEnv`` goes through ``harness.run_first_episodes`` under a ``BankActor``.
    ``graph``: as in ``evaluate_policy``.  ``maps``: as in ``evaluate_policy``, one group of planes per
    result: per policy, or per (policy, label) pair with ``split``.  ``disturb``: as in ``evaluate_policy``; a
    ``Disturber`` built for the batch carries the env -> level map (``sweep`` builds one)."""
    from . import harness
    from .env import Drone2dVecEnv

    if noise not in ("philox", "torch"):
        raise ValueError("noise must be 'philox' or 'torch'")
    if graph:
        _check_graph(venv, noise, keep_actions, disturb)
    grid = _check_maps(maps)
    bank = _as_bank(bank)
    n = int(venv.num_envs)
    dkw = {}
    if disturb is not None:
        from .disturb import make_disturber

        dkw["disturb"] = make_disturber(disturb, venv, seed)
    ep = check_env_policy(env_policy, n, bank.n_policies)
    labels = None
    if split is not None:
        labels = split.detach().cpu().numpy() if isinstance(split, torch.Tensor) else np.asarray(split)
        if labels.dtype.kind not in "iu" or labels.shape != (n,):
            raise ValueError(f"split must be an integer array of shape [{n}]")
    extra = (ep,) if labels is None else (ep, labels)
    # one group of planes per result (with maps there is one rank: the local arrays are the batch's)
    pairs = sorted(set(zip(ep.tolist(), labels.tolist()))) if labels is not None else None
    groups = n_groups = None
    if grid is not None:
        if pairs is None:
            groups, n_groups = ep, bank.n_policies
        else:
            where = {ps: g for g, ps in enumerate(pairs)}
            groups = np.array([where[ps] for ps in zip(ep.tolist(), labels.tolist())], np.int32).reshape(n)
            n_groups = max(len(pairs), 1)
    actions = counts = spawn_obs = None
    if not isinstance(venv, Drone2dVecEnv):
        if keep_actions:
            raise ValueError("keep_actions needs a HIP batch")
        raw = harness.run_first_episodes(venv, BankActor(bank, ep), deterministic=deterministic, seed=seed,
                                         max_steps=max_steps, n_obstacles=n_obstacles,
                                         flight_paths=flight_paths or grid is not None, check_every=check_every,
                                         records=False, extra=extra, **dkw)
        fin, rows_np, nobs, extra = raw["finished"], raw["rows"], raw["n_obstacles"], raw["extra"]
        xy_np = raw["xy"] if flight_paths else None
        if grid is not None:
            counts, spawn_obs = _host_maps(grid, raw, groups, n_groups), raw["spawn_xy"]
    else:
        bank = bank.to(venv.device)
        ep_dev = torch.from_numpy(ep).to(venv.device)
        am = None
        if grid is not None:
            from . import heatmap

            am = heatmap.ArenaMaps(venv, grid, groups, n_groups, cap=max_steps)
        fin, rows_np, xy_np, nobs, actions, extra = _fly(venv, None, bank.c_bank(ep_dev), deterministic, seed, max_steps,
                                                         n_obstacles, flight_paths, check_every, noise, keep_actions,
                                                         extra, graph=graph, maps=am, **dkw)
        if am is not None:
            counts, spawn_obs = am.counts(), am.spawn_obs.cpu().numpy()
            am.close()
    g_ep, g_labels = extra[0], (extra[1] if labels is not None else None)

    def subset(mask, local_mask, group):
        idx = np.flatnonzero(mask)
        out = _records(venv, fin[idx], rows_np[idx], xy_np[:, idx] if xy_np is not None else None, nobs)
        if keep_actions:
            out["actions"] = actions[:, np.flatnonzero(local_mask)]
        if counts is not None:
            out["maps"] = _group_maps(counts, group, idx, spawn_obs, fin, rows_np, xy_np)
        return out

    if labels is None:
        return [subset(g_ep == p, ep == p, p) for p in range(bank.n_policies)]
    g_pairs = sorted(set(zip(g_ep.tolist(), g_labels.tolist())))
    return {(p, s): subset((g_ep == p) & (g_labels == s), (ep == p) & (labels == s), g)
            for g, (p, s) in enumerate(g_pairs)}


def sweep_layout(n_policies: int, n_scenarios: int, runs: int, levels: int = 1) -> tuple:
    """(env_policy, env_scenario), int32 [P S R] each, of a sweep batch: policy-major, then scenario,
    then run.  A policy's envs are contiguous, so at most one 64-env chunk per policy boundary holds
    two policies.  With ``levels`` = L > 1 (a disturbed sweep) the batch is [P S L R] -- policy, scenario,
    level, run -- and the tuple gains a third array, env_level."""
    P, S, R, L = int(n_policies), int(n_scenarios), int(runs), int(levels)
    if P < 1 or S < 1 or R < 1 or L < 1:
        raise ValueError("sweep_layout needs at least one policy, one scenario, one level and one run")
    if L == 1:
        return (np.repeat(np.arange(P, dtype=np.int32), S * R),
                np.tile(np.repeat(np.arange(S, dtype=np.int32), R), P))
    return (np.repeat(np.arange(P, dtype=np.int32), S * L * R),
            np.tile(np.repeat(np.arange(S, dtype=np.int32), L * R), P),
            np.tile(np.repeat(np.arange(L, dtype=np.int32), R), P * S))


def sweep(bank, scenarios, runs: int, *, seed: int = 0, deterministic: bool = False, flight_paths: bool = False,
          env_kwargs: dict | None = None, graph: bool = False, maps=None, disturb=None) -> dict:
    """Every agent of ``bank`` on every scenario, ``runs`` first episodes each, as one batch of
    P S R envs (``sweep_layout``) in one closed loop: {agent name: {scenario name: result dict}}.
    ``scenarios``: names of static scenarios or ``Scenario`` objects (a curriculum stage is refused:
    pass a fresh-curriculum batch to ``evaluate_policies``); ``env_kwargs``: default ``ENV_TEST_CONFIG``.
    Every (agent, scenario, run) is an env of its own global id, so its spawn and noise draws are its own.
    ``graph``: as in ``evaluate_policy``.  ``maps``: as in ``evaluate_policy``, one group of planes per
    (agent, scenario).

    ``disturb`` (a list of ``disturb.Disturbance``): the level axis -- the batch is P S L R envs, agents x
    scenarios x levels x runs, env i under level ``env_level[i]`` of ``sweep_layout``, still one closed loop,
    and the result is {agent name: {scenario name: {level name: result dict}}} (``disturb.level_names``).
    With maps: one group of planes per (agent, scenario, level).  Not with ``graph``."""
    from .config import CURRICULUM_STAGES, ENV_TEST_CONFIG
    from .env import Drone2dVecEnv, is_curriculum

    bank = _as_bank(bank)
    scenarios = [scenarios] if isinstance(scenarios, str) else list(scenarios)
    kw = dict(ENV_TEST_CONFIG if env_kwargs is None else env_kwargs, scenario=scenarios)
    if not scenarios or any(isinstance(s, str) and s in CURRICULUM_STAGES for s in scenarios) or is_curriculum(kw):
        raise ValueError("sweep takes static scenarios (names or Scenario objects), at least one")
    names = [s if isinstance(s, str) else s.name for s in scenarios]
    if len(set(names)) != len(names):
        raise ValueError("sweep: scenario names must be unique")
    if disturb is not None:
        return _sweep_levels(bank, kw, names, runs, seed, deterministic, flight_paths, graph, maps, disturb)
    ep, es = sweep_layout(bank.n_policies, len(scenarios), runs)
    _check_maps(maps)
    if not bank.device.type == "cuda":
        raise ValueError("sweep runs on a HIP device: build the bank there")
    venv = Drone2dVecEnv(len(ep), device=bank.device, seed=seed, with_info=True, env_scenario=es, **kw)
    try:
        res = evaluate_policies(venv, bank, ep, split=es, deterministic=deterministic, seed=seed,
                                flight_paths=flight_paths, graph=graph, maps=maps)
    finally:
        venv.close()
    return {bank.names[p]: {names[s]: res[(p, s)] for s in range(len(names))} for p in range(bank.n_policies)}


def _sweep_levels(bank, kw, names, runs, seed, deterministic, flight_paths, graph, maps, disturb) -> dict:
    """``sweep`` with the level axis: the labels the batch is split by are scenario * L + level."""
    from .disturb import Disturber, _levels, level_names
    from .env import Drone2dVecEnv

    if graph:
        _check_graph(None, "philox", False, disturb)  # (refused before a batch is built for it)
    levels = _levels(disturb)
    lnames, L = level_names(levels), len(levels)
    lay = sweep_layout(bank.n_policies, len(names), runs, L)
    ep, es = lay[:2]
    el = lay[2] if L > 1 else np.zeros(len(ep), np.int32)
    _check_maps(maps)
    if not bank.device.type == "cuda":
        raise ValueError("sweep runs on a HIP device: build the bank there")
    venv = Drone2dVecEnv(len(ep), device=bank.device, seed=seed, with_info=True, env_scenario=es, **kw)
    try:
        d = Disturber(len(ep), levels, el, device=venv.device, env_id_base=int(venv.cfg.env_id_base), seed=seed)
        res = evaluate_policies(venv, bank, ep, split=es * L + el, deterministic=deterministic, seed=seed,
                                flight_paths=flight_paths, maps=maps, disturb=d)
    finally:
        venv.close()
    return {bank.names[p]: {names[s]: {lnames[k]: res[(p, s * L + k)] for k in range(L)} for s in range(len(names))}
            for p in range(bank.n_policies)}


__all__ = ["evaluate_policy", "act", "actor_tensors", "as_mlp_actor", "philox_noise_host", "load", "bind", "EvalError",
           "D2DEvalStepArgs", "D2DEvalBank", "PolicyBank", "BankActor", "act_bank", "evaluate_policies", "sweep_layout",
           "sweep", "check_env_policy", "EvalLoop"]
