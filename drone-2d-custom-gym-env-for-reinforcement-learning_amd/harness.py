"""Test harness on the batched env: the reference's ``mode == "test"`` loop
(main.py:242-327) -- run a policy until every env finishes its first episode, then report the same
metrics and files (``results.txt`` lines, ``apes/collisions/rewards/time_spent.npy``) -- with all
envs of a scenario stepping in one batch instead of 100 sequential runs.

``MlpActor`` is SB3's default ``MlpPolicy`` actor (27-64-64-2, tanh; policy_kwargs {} in the
shipped agents), loaded from the float32 weights extracted from an agent zip
(tests/golden/make_agent_fixture.py).  ``model.predict(obs)`` in the reference is stochastic
(deterministic=False): a = clip(mean + exp(log_std) * N(0, 1), -1, 1).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import abi
from .env import info_dicts


class MlpActor(torch.nn.Module):
    """SB3 MlpPolicy actor.  ``batch_invariant=True`` evaluates every linear layer as a fixed-order
    sum of element-wise products (bias + x_0 w_0 + x_1 w_1 + ...): each env's action is then a
    function of its own observation alone, bit for bit independent of the batch it sits in, so a
    run sharded over ranks reproduces one unsharded batch exactly (a GEMM may pick a different
    kernel -- and summation order -- for a different batch size)."""

    def __init__(self, w: dict, batch_invariant: bool = False):
        super().__init__()
        t = {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in w.items()}
        self.l0 = torch.nn.Linear(27, 64)
        self.l1 = torch.nn.Linear(64, 64)
        self.out = torch.nn.Linear(64, 2)
        self.batch_invariant = batch_invariant
        with torch.no_grad():
            self.l0.weight.copy_(t["mlp_extractor_policy_net_0_weight"])
            self.l0.bias.copy_(t["mlp_extractor_policy_net_0_bias"])
            self.l1.weight.copy_(t["mlp_extractor_policy_net_2_weight"])
            self.l1.bias.copy_(t["mlp_extractor_policy_net_2_bias"])
            self.out.weight.copy_(t["action_net_weight"])
            self.out.bias.copy_(t["action_net_bias"])
        self.register_buffer("log_std", t["log_std"].clone())

    @classmethod
    def from_npz(cls, path: str, batch_invariant: bool = False) -> "MlpActor":
        with np.load(path, allow_pickle=False) as z:
            return cls({k: z[k] for k in z.files}, batch_invariant=batch_invariant)

    @classmethod
    def from_policy(cls, actor_critic, batch_invariant: bool = False) -> "MlpActor":
        """The actor of a ``ppo.ActorCritic`` (a copy of its policy net, ``action_net`` and ``log_std``):
        a policy trained here through the torch loop."""
        keep = ("mlp_extractor.policy_net.", "action_net.", "log_std")
        sd = {k.replace(".", "_"): v.detach().cpu().numpy() for k, v in actor_critic.state_dict().items()
              if k.startswith(keep)}
        return cls(sd, batch_invariant=batch_invariant)

    @staticmethod
    def _lin_fixed(x: torch.Tensor, lin: torch.nn.Linear) -> torch.Tensor:
        y = lin.bias.expand(x.shape[0], -1).clone()
        w = lin.weight.t()  # [in, out]
        for k in range(w.shape[0]):
            y = y + x[:, k:k + 1] * w[k]
        return y

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        if self.batch_invariant:
            h = torch.tanh(self._lin_fixed(obs, self.l0))
            h = torch.tanh(self._lin_fixed(h, self.l1))
            return self._lin_fixed(h, self.out)
        return self.out(torch.tanh(self.l1(torch.tanh(self.l0(obs)))))

    @torch.no_grad()
    def act(self, obs: torch.Tensor, deterministic: bool = False, generator: torch.Generator | None = None,
            noise: torch.Tensor | None = None):
        """a = clip(mean + exp(log_std) * N(0, 1), -1, 1); ``noise`` supplies the N(0, 1) draws
        (the harness passes each shard its block of one global draw)."""
        mean = self(obs)
        if not deterministic:
            if noise is None:
                noise = torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)
            mean = mean + torch.exp(self.log_std) * noise
        return torch.clamp(mean, -1.0, 1.0)


def _dist_world():
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


def run_first_episodes(venv, policy: MlpActor, *, deterministic: bool = False, seed: int = 0,
                       max_steps: int | None = None, n_obstacles: int | None = None,
                       flight_paths: bool = False, check_every: int = 16, gather: bool = True,
                       policy_device=None, records: bool = True, extra=(), disturb=None) -> dict:
    """Step ``venv`` (with info rows) under ``policy`` until every env has finished its first
    episode; per-episode records as the reference's test loop keeps them (main.py:273-281).

    ``flight_paths``: also return ``flight_xy`` [steps, episodes, 2] (NaN past each episode's
    end; ``flight_path_lists`` turns it into the JSON value), each episode's
    ``info['flight_path']`` -- the frame position
    after every step as (x, screen_height - y), one entry per env step including the last
    (drone_2d_env.py:409-415, 984-986; saved as JSON by main.py:307-308).  The positions are decoded
    from the observation (obs[6:8] = 2p/(W,H) - 1, the terminal observation on the last step), so
    they carry the float32 observation's rounding (<= 1e-4 px at 1300 px) where the reference
    records the fp64 body position; the buffer stays on the device (8 B per env-step) until the
    episodes are done.

    The loop never waits on the device per step: finished episodes' info rows are kept by a
    masked select on the device and the "all done" test reads back one flag every
    ``check_every`` steps.

    Sharded (torch.distributed initialised, world > 1, every rank passing its shard of one global
    batch: ``shard.make_shard_venv``): each rank steps its own envs; the policy noise of global env
    i at step t is entry i of one global N(0, 1) draw per step (the same generator on every rank),
    so the episodes are those of one unsharded batch; at the end rank 0 gathers every rank's
    records in global env order (``gather``) and the returned dict covers the whole batch (other
    ranks get their own shard's).  Use a ``batch_invariant`` policy for bit-identical actions.

    ``policy_device``: where the policy and its noise run (default: the env's device).  The
    parity tests pass "cpu" for the HIP batch and the CPU oracle alike, so both see the same
    actions for the same observations (a GPU tanh or N(0, 1) stream is not the CPU one).

    ``records=False``: instead of the result dict, what it is built from, over the whole (gathered)
    batch in global env order -- ``finished`` bool [n], ``rows`` [n, INFO_DIM], ``xy`` [cap, n, 2] or
    None, ``n_obstacles``, ``spawn_xy`` float32 [n, 2] (the reset observation's [6:8]), and ``extra``: the
    caller's per-env arrays, gathered alike -- for a caller that splits the batch into several result
    sets (``evaluate.evaluate_policies``) or bins it into arena maps (``heatmap.from_flight``).

    ``disturb`` (a ``disturb.Disturbance``, or a ``disturb.Disturber`` / ``HostDisturber`` built for this
    batch): the policy sees ``disturb.obs`` of the observations and the env gets ``disturb.act`` of the
    actions; the records and the flight paths are the true flight's."""
    if disturb is not None:
        from .disturb import make_disturber

        disturb = make_disturber(disturb, venv, seed)
    dev = venv.device
    pdev = torch.device(policy_device) if policy_device is not None else dev
    dist, rank, world = _dist_world()
    gen = torch.Generator(device=pdev).manual_seed(seed)
    policy = policy.to(pdev)
    obs = venv.reset(seed=seed)
    spawn_np = obs[:, 6:8].cpu().numpy().copy() if not records else None
    n = venv.num_envs
    offset = int(getattr(venv.cfg, "env_id_base", 0)) if world > 1 else 0
    n_total = n
    if world > 1:
        counts = [None] * world
        dist.all_gather_object(counts, n)
        n_total = int(sum(counts))
    finished = torch.zeros(n, dtype=torch.bool, device=dev)
    rows = torch.zeros(n, abi.INFO_DIM, dtype=torch.float32, device=dev)
    cap = max_steps if max_steps is not None else int(venv.kwargs["n_steps"]) + 1
    nobs = n_obstacles if n_obstacles is not None else len(venv.scenarios[0].circles)
    pos = torch.full((cap, n, 2), float("nan"), dtype=torch.float32, device=dev) if flight_paths else None
    for t in range(cap):
        noise = None
        if not deterministic:
            noise = torch.randn((n_total, 2), device=pdev, dtype=torch.float32, generator=gen)[offset:offset + n]
        if disturb is None:
            a = policy.act(obs.to(pdev), deterministic=deterministic, noise=noise)
        else:
            a = policy.act(disturb.obs(obs, t).to(pdev), deterministic=deterministic, noise=noise)
            a = disturb.act(a.to(dev).contiguous(), t)
        obs, rew, term, trunc, info = venv.step(a)
        done = term | trunc
        new = done & ~finished
        rows = torch.where(new[:, None], info.to(dev), rows)
        if pos is not None:
            xy = torch.where(done[:, None], venv.terminal_obs[:, 6:8].to(dev), obs[:, 6:8])
            pos[t] = torch.where(finished[:, None], pos[t], xy)
        finished |= done
        if (t + 1) % check_every == 0 and bool(finished.all()):
            break
    fin = finished.cpu().numpy()
    rows_np = rows.cpu().numpy()
    xy_np = pos.cpu().numpy() if pos is not None else None
    extra = tuple(np.asarray(e) for e in extra)
    if world > 1 and gather:
        parts = [None] * world
        dist.all_gather_object(parts, (offset, fin, rows_np, xy_np, extra, spawn_np))
        parts.sort(key=lambda p: p[0])
        fin = np.concatenate([p[1] for p in parts])
        rows_np = np.concatenate([p[2] for p in parts])
        if xy_np is not None:
            T = max(p[3].shape[0] for p in parts)
            xy_np = np.concatenate([p[3][:T] for p in parts], 1)
        extra = tuple(np.concatenate([p[4][k] for p in parts]) for k in range(len(extra)))
        if spawn_np is not None:
            spawn_np = np.concatenate([p[5] for p in parts])
    if not records:
        return {"finished": fin, "rows": rows_np, "xy": xy_np, "n_obstacles": nobs, "extra": extra,
                "spawn_xy": spawn_np}
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


def write_results_rank0(m: dict, out_dir: str, scenario: str, agent_nr: str, agent_path: str):
    """``write_results`` on rank 0 only (a gathered ``run_first_episodes`` result); other ranks
    return None.  Without a process group it is ``write_results``."""
    _, rank, _ = _dist_world()
    return write_results(m, out_dir, scenario, agent_nr, agent_path) if rank == 0 else None


def flight_path_lists(m: dict) -> list:
    """``m["flight_xy"]`` as the reference's ``flight_paths`` JSON value: one list of [x, y] per
    episode, ``env_steps`` entries long (main.py:278, 307-308)."""
    fl = m["flight_xy"]
    return [fl[:T, j].tolist() for j, T in enumerate(m["time_spent"])]


def flight_path_colours(m: dict) -> np.ndarray:
    """uint8 [episodes, 3], main.py:374-383: red for a collided episode (and for a single episode),
    else ``red_blue_grad`` of the min-max-normalised total reward."""
    from .render import red_blue_grad

    rew = np.asarray(m["rewards"], np.float64)
    n = len(rew)
    rgb = np.zeros((n, 3), np.uint8)
    if n == 0:
        return rgb
    lo, hi = float(rew.min()), float(rew.max())
    for i in range(n):
        if m["collisions"][i] == 1 or n == 1 or not hi > lo:
            rgb[i] = (255, 0, 0)
        else:
            rgb[i] = red_blue_grad((rew[i] - lo) / (hi - lo))
    return rgb


def plot_inputs(m: dict):
    """What the plot is drawn from: (xy float32 [steps, episodes, 2] world positions, lengths int32
    [episodes], rgb uint8 [episodes, 3]) of a ``run_first_episodes(..., flight_paths=True)`` result."""
    fl = np.asarray(m["flight_xy"], np.float64)
    h = float(m.get("screen", (1300.0, 1300.0))[1])
    xy = np.nan_to_num(np.stack([fl[..., 0], h - fl[..., 1]], -1), nan=0.0).astype(np.float32)
    return xy, np.asarray(m["time_spent"], np.int32), flight_path_colours(m)


def _plot_scenario(venv_or_scenario, screen):
    from .config import TEST_SCENARIOS
    from .scenarios import Scenario, create_test_scenario

    s = venv_or_scenario
    if s is None or isinstance(s, (Scenario, abi.D2DScn)):
        return s
    if isinstance(s, str):  # a test scenario's name; 'stage_k' and the like have no fixed picture
        return create_test_scenario(s, int(screen[0]), int(screen[1])) if s in TEST_SCENARIOS else None
    return s.scenarios[0] if getattr(s, "scenarios", None) else None  # a batch: its (first) scenario


def plot_flight_paths(m: dict, venv_or_scenario=None, size=None, device=None) -> np.ndarray:
    """The reference's overview plot (main.py:329-389) of a ``run_first_episodes(..., flight_paths=True)``
    result, drawn on the device by libd2d_render.so: uint8 [H, W, 3].  ``venv_or_scenario``: the batch
    the episodes ran on, a Scenario / ABI record, a test scenario's name, or None for a blank
    background (the reference's 'stage_k' case); ``size``: an int or (H, W), default the screen."""
    from . import render as R

    screen = m.get("screen", (1300.0, 1300.0))
    if size is None:
        size = (int(screen[1]), int(screen[0]))
    dev = device if device is not None else getattr(venv_or_scenario, "device", None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    xy, lens, rgb = plot_inputs(m)
    rec = _plot_scenario(venv_or_scenario, screen)
    r = R.Renderer(dev, max_frames=1)
    try:
        img = r.plot_paths(r.scn_tensor([rec]) if rec is not None else None, torch.from_numpy(xy),
                           torch.from_numpy(lens), torch.from_numpy(rgb), size=size, screen=screen)
        return img.cpu().numpy()
    finally:
        r.close()


def plot_background(venv_or_scenario=None, size=None, screen=(1300.0, 1300.0), device=None) -> torch.Tensor:
    """The picture ``plot_flight_paths`` draws its paths on (the scenario; blank for None or a curriculum
    stage), without a path: uint8 [H, W, 3] on the device."""
    from . import render as R

    if size is None:
        size = (int(screen[1]), int(screen[0]))
    dev = device if device is not None else getattr(venv_or_scenario, "device", None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    rec = _plot_scenario(venv_or_scenario, screen)
    r = R.Renderer(dev, max_frames=1)
    try:
        # one path of no points: the renderer draws the scenario and no segment
        return r.plot_paths(r.scn_tensor([rec]) if rec is not None else None, torch.zeros(1, 1, 2),
                            torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.uint8), size=size,
                            screen=screen).clone()
    finally:
        r.close()


def plot_maps(m: dict, venv_or_scenario=None, size=None, device=None, alpha: int = 200, min_count: int = 1) -> dict:
    """The arena-map pictures of a result that carries ``"maps"``, painted on the device by libd2d_heat.so
    over ``plot_background``: {"density", "spawn_success", "crashes"} -> uint8 [H, W, 3]
    (``heatmap.PICTURES``: where the episodes flew, the success rate by spawn cell, where they crashed)."""
    from . import heatmap

    screen = m.get("screen", (1300.0, 1300.0))
    bg = plot_background(venv_or_scenario, size, screen, device)
    planes = np.asarray(m["maps"]["planes"], np.uint32)[None]
    return {name: heatmap.paint(planes, bg, name, alpha, min_count, device=bg.device)[0].cpu().numpy()
            for name in heatmap.PICTURES}


def summary(m: dict) -> dict:
    """The numbers of the reference's results.txt (main.py:318-325)."""
    runs = m["successes"] + m["fails"]
    col = int(m["collisions"].sum())
    return {"Successes": m["successes"], "Fails": m["fails"], "Collisions": col,
            "Success rate": m["successes"] / max(runs, 1), "Collision rate": col / max(runs, 1),
            "Average APE": float(np.mean(m["apes"])) if len(m["apes"]) else float("nan"),
            "Average flight time": float(np.mean(m["time_spent"])) if len(m["time_spent"]) else float("nan")}


def write_results(m: dict, out_dir: str, scenario: str, agent_nr: str, agent_path: str):
    """The reference's per-scenario files: results.txt + collisions/rewards/apes/time_spent .npy
    (+ the ``flight_paths`` JSON when ``m`` carries them, and then, with a HIP device to draw it on,
    the overview plot ``plots/<scenario>.png``), main.py:307-389.  When ``m`` carries arena maps
    (``evaluate_policy(..., maps=...)``): ``maps.npz`` (``planes``, ``outside``) and, with a HIP device,
    ``plots/<scenario>_density.png``, ``_spawn_success.png`` and ``_crashes.png`` (``plot_maps``)."""
    os.makedirs(out_dir, exist_ok=True)
    for k in ("collisions", "rewards", "apes", "time_spent"):
        np.save(os.path.join(out_dir, f"{k}.npy"), m[k])
    if "flight_xy" in m:
        with open(os.path.join(out_dir, "flight_paths"), "w") as f:
            json.dump(flight_path_lists(m), f)
        if torch.cuda.is_available():  # the overview plot, main.py:329-389 (drawn on the device)
            from .render import write_png

            os.makedirs(os.path.join(out_dir, "plots"), exist_ok=True)
            write_png(os.path.join(out_dir, "plots", f"{scenario}.png"), plot_flight_paths(m, scenario))
    if "maps" in m:
        np.savez(os.path.join(out_dir, "maps.npz"), planes=m["maps"]["planes"], outside=m["maps"]["outside"])
        if torch.cuda.is_available():
            from .render import write_png

            os.makedirs(os.path.join(out_dir, "plots"), exist_ok=True)
            for name, img in plot_maps(m, scenario).items():
                write_png(os.path.join(out_dir, "plots", f"{scenario}_{name}.png"), img)
    s = summary(m)
    with open(os.path.join(out_dir, f"{scenario}_{agent_nr}_results.txt"), "w") as f:
        for k in ("Successes", "Fails", "Collisions", "Success rate", "Collision rate", "Average APE",
                  "Average flight time"):
            f.write(f"{k}: {s[k]}\n")
        f.write(f"Agent path: {agent_path}\n")
    return s


SELECTION_COLUMNS = ("agent", "scenario", "episodes", "success_rate", "collision_rate", "average_ape",
                     "average_flight_time")


def selection_table(results: dict) -> list:
    """The agent-by-scenario table a checkpoint is picked from (the reference keeps it by hand in
    barplots.py): one row (agent, scenario, episodes, success rate, collision rate, average APE,
    average flight time) per pair of ``results`` = {agent: {scenario: result dict}} (``evaluate.sweep``),
    in its order; the numbers are ``summary``'s (NaN averages for a pair with no finished episode)."""
    rows = []
    for agent, per_scn in results.items():
        for scn, m in per_scn.items():
            s = summary(m)
            rows.append((agent, scn, s["Successes"] + s["Fails"], s["Success rate"], s["Collision rate"],
                         s["Average APE"], s["Average flight time"]))
    return rows


def write_selection(results: dict, out_dir: str) -> list:
    """``selection_table(results)`` as ``selection.csv`` (a header line, floats by ``repr``) and
    ``selection.json`` (a list of objects; NaN written as null) under ``out_dir``; returns the rows."""
    import csv

    rows = selection_table(results)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "selection.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SELECTION_COLUMNS)
        for r in rows:
            w.writerow([repr(float(v)) if isinstance(v, float) else v for v in r])
    with open(os.path.join(out_dir, "selection.json"), "w") as f:
        json.dump([{k: (None if isinstance(v, float) and v != v else v) for k, v in zip(SELECTION_COLUMNS, r)}
                   for r in rows], f, indent=1)
    return rows


ROBUSTNESS_COLUMNS = ("agent", "scenario", "level", "obs_sigma", "act_sigma", "sensor_dropout", "motor_gain_left",
                      "motor_gain_right", "act_delay", "episodes", "success_rate", "collision_rate", "average_ape",
                      "average_flight_time")


def robustness_table(results: dict, levels) -> list:
    """One row (``ROBUSTNESS_COLUMNS``) per (agent, scenario, level) of ``results`` = {agent: {scenario:
    {level name: result dict}}} (``evaluate.sweep(..., disturb=levels)``), in its order: the level's
    parameters and ``summary``'s headline numbers."""
    from .disturb import level_names

    levels = list(levels)
    by_name = dict(zip(level_names(levels), levels))
    rows = []
    for agent, per_scn in results.items():
        for scn, per_level in per_scn.items():
            for name, m in per_level.items():
                s, d = summary(m), by_name[name].as_dict()
                rows.append((agent, scn, name, d["obs_sigma"], d["act_sigma"], d["sensor_dropout"], d["motor_gain_left"],
                             d["motor_gain_right"], d["act_delay"], s["Successes"] + s["Fails"], s["Success rate"],
                             s["Collision rate"], s["Average APE"], s["Average flight time"]))
    return rows


def write_robustness(out_dir: str, results: dict, levels) -> list:
    """``robustness_table(results, levels)`` as ``robustness.csv`` (a header line, floats by ``repr``) and
    ``robustness.json`` (a list of objects; NaN written as null) under ``out_dir``; returns the rows."""
    import csv

    rows = robustness_table(results, levels)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "robustness.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(ROBUSTNESS_COLUMNS)
        for r in rows:
            w.writerow([repr(float(v)) if isinstance(v, float) else v for v in r])
    with open(os.path.join(out_dir, "robustness.json"), "w") as f:
        json.dump([{k: (None if isinstance(v, float) and v != v else v) for k, v in zip(ROBUSTNESS_COLUMNS, r)}
                   for r in rows], f, indent=1)
    return rows


def save_gif(frames, path: str, fps: int = 60) -> None:
    """Frames [T, H, W, 3] as an animated GIF (the reference's per-scenario GIF, main.py:283-300);
    needs Pillow and raises ImportError without it."""
    from .render import save_gif as _save

    _save(frames, path, fps)


def record_gifs(venv, policy, out_dir: str, scenario: str, agent: str, env_ids=(0,), **kw) -> list:
    """The reference's per-scenario animation (main.py:266-295, ``Gifs/<agent>/<scenario>.gif``), recorded
    and encoded on the device by ``gif.record_episodes`` (its keyword arguments pass through): the first
    episode of each of ``env_ids`` of the HIP batch ``venv`` under ``policy``.  One env writes
    ``<out_dir>/Gifs/<agent>/<scenario>.gif``, several write ``<scenario>_<k>.gif``, k counting ``env_ids``.
    Needs no Pillow; returns the paths."""
    from . import gif

    rec = gif.record_episodes(venv, policy, env_ids, **kw)
    d = os.path.join(out_dir, "Gifs", str(agent))
    os.makedirs(d, exist_ok=True)
    names = [f"{scenario}.gif"] if len(rec.gifs) == 1 else [f"{scenario}_{k}.gif" for k in range(len(rec.gifs))]
    paths = [os.path.join(d, name) for name in names]
    for p, b in zip(paths, rec.gifs):
        with open(p, "wb") as f:
            f.write(b)
    return paths


__all__ = ["MlpActor", "run_first_episodes", "flight_path_lists", "summary", "write_results", "record_gifs",
           "write_results_rank0", "plot_flight_paths", "plot_inputs", "plot_background", "plot_maps", "flight_path_colours", "save_gif",
           "selection_table", "write_selection", "SELECTION_COLUMNS", "robustness_table", "write_robustness",
           "ROBUSTNESS_COLUMNS"]
