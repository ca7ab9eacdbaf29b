"""Python facade over the HIP library: the reference's ``Drone2dEnv`` surface, batched.

``Drone2dVecEnv``  N envs on one GPU; tensor fast path (torch-ROCm tensors in, out).
``Drone2dEnv``     one env with the reference's gym-0.21 API (drone_2d_env.py:22-1023):
                   ``reset() -> obs``, ``step(a) -> (obs, reward, done, info)``.

Both take the reference's kwargs dict (rl_config.py:10-44, read at drone_2d_env.py:34-66).
Every step runs ``d2d_step`` (libdrone2d_hip.so) on the caller's current HIP stream; there is no
CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Sequence

import numpy as np
import torch

from . import abi
from ._native import check, load
from .config import CURRICULUM_STAGES, SCENARIO_STEP_COST, TEST_SCENARIOS, make_cfg
from .scenarios import Scenario, create_test_scenario, free_flight

INFO_KEYS = ("reward", "collision_avoidance_reward", "path_adherence", "path_progression", "collision_reward",
             "reach_end_reward", "agressive_alpha_reward", "dist_closest_obs", "env_steps")


class Box:
    """Duck-typed ``gym.spaces.Box`` (gym/gymnasium are used when importable)."""

    def __init__(self, low, high, dtype=np.float32):
        self.low = np.asarray(low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype)
        self.shape = self.low.shape
        self.dtype = np.dtype(dtype)

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


def _make_box(low, high):
    for mod in ("gymnasium", "gym"):
        try:
            spaces = __import__(mod + ".spaces", fromlist=["Box"])
            return spaces.Box(low=np.asarray(low, np.float32), high=np.asarray(high, np.float32), dtype=np.float32)
        except Exception:  # noqa: BLE001 -- optional dependency
            continue
    return Box(low, high)


def build_scenarios(kwargs: dict) -> list[Scenario]:
    """Scenario list for ``mode='test'``: one name, a list of names, or Scenario objects."""
    W, H = kwargs["screensize_x"], kwargs["screensize_y"]
    spec = kwargs["scenario"]
    if is_curriculum(kwargs):
        # a pool of curriculum resets (drone2d_amd.curriculum); the kernel draws one per episode
        from .curriculum import curriculum_pool, stage_for_sim_num

        if spec in CURRICULUM_STAGES:
            stage, chance = spec, None
        else:
            stage, chance = stage_for_sim_num(int(kwargs.get("sim_num", 0)))
        return curriculum_pool(stage, kwargs, int(kwargs.get("curriculum_pool") or 1024),
                               seed=int(kwargs.get("curriculum_seed", 0)), spawn_chance=chance)
    if isinstance(spec, (str, Scenario)):
        spec = [spec]
    out = []
    for s in spec:
        if isinstance(s, Scenario):
            out.append(s)
        elif s in TEST_SCENARIOS:
            out.append(create_test_scenario(s, W, H))
        elif isinstance(s, str) and s.endswith("_free") and s[:-5] in TEST_SCENARIOS:
            out.append(free_flight(create_test_scenario(s[:-5], W, H)))
        else:
            raise ValueError(f"unknown scenario {s!r}")
    return out


def is_curriculum(kwargs: dict) -> bool:
    """mode='curriculum' or an explicit stage_k scenario (drone_2d_env.py:75-86, 199-215)."""
    spec = kwargs.get("scenario")
    return kwargs.get("mode") == "curriculum" or (isinstance(spec, str) and spec in CURRICULUM_STAGES)


def is_fresh_curriculum(kwargs: dict) -> bool:
    """Curriculum episodes on scenarios generated on the device, one per reset (the default; the
    reference's behaviour).  ``curriculum_pool=P`` selects the host-generated pool of P instead."""
    return is_curriculum(kwargs) and kwargs.get("curriculum_pool") is None


def make_curriculum(kwargs: dict, envs_total: int) -> abi.D2DCurriculum:
    """The device generator's parameters from the reference kwargs: stage from scenario='stage_k'
    (else the sim_num schedule from ``sim_num``), n_wps, path_segment_length, random_path_spawn,
    spawn_corners (rl_config.py:10-44)."""
    c = abi.D2DCurriculum()
    spec = kwargs.get("scenario")
    c.stage = int(spec[-1]) if isinstance(spec, str) and spec in CURRICULUM_STAGES else 0
    c.n_wps = int(kwargs["n_wps"])
    c.segment_length = float(kwargs["path_segment_length"])
    c.random_path_spawn = 1 if kwargs.get("random_path_spawn", True) is True else 0
    lo, hi = kwargs.get("spawn_corners", (1, 4))
    c.corner_lo, c.corner_hi = int(lo), int(hi)
    c.sim_num0 = float(kwargs.get("sim_num", 0))
    c.envs_total = float(envs_total)
    return c


class Drone2dVecEnv:
    """``num_envs`` independent Drone2dEnv copies stepping together on one GPU.

    Parameters mirror the reference kwargs; ``kwargs['scenario']`` may also be a list of scenario
    names / Scenario objects (mixed batches, BASELINE config 5) or '<name>_free' (no obstacles,
    config 2).  Extra knobs:
      env_scenario    int array [num_envs] mapping env -> scenario index (default: i % n_scenarios)
      env_id_offset   global id of env 0 (multi-GPU shards keep per-env RNG streams global)
      auto_reset      SB3 VecEnv semantics (done envs are reset inside the step kernel)
      timeup_truncates  report time-up as truncation instead of termination (reference: False)
    Curriculum (``mode='curriculum'`` or ``scenario='stage_k'``), two forms:
      fresh (default)  every reset runs on a scenario generated on the device for that episode
                       alone (d2d_set_curriculum): the reference's behaviour.  The stage is
                       explicit or follows the reference's sim_num schedule with
                       sim_num = kwargs['sim_num'] + steps x ``envs_total`` (all ranks' envs;
                       default num_envs), advanced on the device with no host call.
      pool             ``kwargs['curriculum_pool'] = P``: P reference-identical resets generated
                       on the host from ``kwargs['curriculum_seed']`` (drone2d_amd.curriculum);
                       every episode draws one entry; ``refresh_curriculum`` swaps in a new pool.
    ``set_curriculum(stage=..., sim_num=...)`` switches the stage / schedule and resets all envs.
    """

    def __init__(self, num_envs: int, device=None, seed: int = 0, *,
                 env_scenario: Sequence[int] | None = None, auto_reset: bool = True,
                 timeup_truncates: bool = False, with_info: bool = True, env_id_offset: int = 0,
                 native_lib: str | None = None, envs_total: int | None = None, exact_trig: bool = False,
                 **kwargs):
        self.kwargs = dict(kwargs)
        self.fresh = is_fresh_curriculum(self.kwargs)
        # exact_trig: the library build whose sin / cos / atan2 are d2d_pmath.h's restatements and whose
        # bearings follow the reference's atan2 -> ssa -> sincos sequence; its states and observations
        # are bit-identical to the CPU oracle's exact build, so closed loops match it episode for
        # episode (default: the faster build, a few ulp apart).  native_lib: an alternative build of
        # the same source (diagnostic A/B builds only).
        self.exact_trig = bool(exact_trig)
        if exact_trig:
            if native_lib is not None:
                raise ValueError("exact_trig selects the exact-trig library build; do not also pass native_lib")
            from ._native import EXACT_LIB_PATH

            if not os.path.exists(EXACT_LIB_PATH):  # built on first use (hipcc, ~1 min)
                from ._build import build_exact

                build_exact()
            native_lib = EXACT_LIB_PATH
        self._lib = load(native_lib)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("Drone2dVecEnv runs on a HIP device only (device='cuda[:k]')")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.cfg = make_cfg(self.kwargs, auto_reset=auto_reset, timeup_truncates=timeup_truncates,
                            env_id_base=env_id_offset)
        self.envs_total = int(envs_total) if envs_total is not None else self.num_envs
        self.scenarios = [] if self.fresh else build_scenarios(self.kwargs)
        # curriculum: every reset draws a fresh device-generated scenario (2) or a pool entry (1)
        self.cfg.scn_pool = (2 if self.fresh else 1) if is_curriculum(self.kwargs) else 0
        self.seed_value = int(seed)
        self.with_info = with_info
        self.action_space = _make_box(-np.ones(2), np.ones(2))
        self.observation_space = _make_box(-np.ones(27), np.ones(27))

        h = C.c_void_p()
        self._check(self._lib.d2d_create(C.byref(self.cfg), self.num_envs, self.device.index, C.byref(h)), "d2d_create")
        self._h = h
        self._upload_scenarios(env_scenario)

        N, dev = self.num_envs, self.device
        # double-buffered outputs: the tensors returned by step k stay valid during step k+1
        self._bufs = [dict(obs=torch.empty(N, abi.OBS_DIM, dtype=torch.float32, device=dev),
                           rew=torch.empty(N, dtype=torch.float32, device=dev),
                           term=torch.empty(N, dtype=torch.bool, device=dev),   # written as 0/1 bytes
                           trunc=torch.empty(N, dtype=torch.bool, device=dev),
                           info=torch.empty(N, abi.INFO_DIM, dtype=torch.float32, device=dev),
                           tobs=torch.zeros(N, abi.OBS_DIM, dtype=torch.float32, device=dev))
                      for _ in range(2)]
        self._k = 0
        self._stats = torch.zeros(abi.NSTATS, dtype=torch.float64, device=dev)
        # step()'s host path: the output pointers of both buffer sets as plain ints (ctypes converts
        # them for the c_void_p parameters) and the raw current-stream query, so an eager step costs
        # one ctypes call and a few attribute reads on the host (tools/eager_probe.py)
        self._bufp = [tuple(b[k].data_ptr() if (k != "info" or with_info) else None
                            for k in ("obs", "rew", "term", "trunc", "info", "tobs")) for b in self._bufs]
        self._act_shape = (N, abi.ACT_DIM)
        self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)

    # ------------------------------------------------------------------ plumbing
    def _check(self, code: int, what: str) -> None:
        check(code, what, self._lib)  # the error text of this handle's library

    def _upload_scenarios(self, env_scenario=None):
        self._render_table = None  # render()'s device copy of the static scenario table
        if self.fresh:
            self.curriculum = make_curriculum(self.kwargs, self.envs_total)
            self.env_scenario = 2 * np.arange(self.num_envs, dtype=np.int32)
            self._check(self._lib.d2d_set_curriculum(self._h, C.byref(self.curriculum)), "d2d_set_curriculum")
            return
        n_scn = len(self.scenarios)
        arr = (abi.D2DScn * n_scn)(*[s.to_c() for s in self.scenarios])
        if env_scenario is None:
            env_scenario = np.arange(self.num_envs) % n_scn
        es = np.ascontiguousarray(np.asarray(env_scenario, dtype=np.int32))
        if es.shape != (self.num_envs,):
            raise ValueError("env_scenario must have shape [num_envs]")
        self.env_scenario = es  # in curriculum mode: the initial map only (resets redraw on device)
        self._check(self._lib.d2d_set_scenarios(self._h, arr, n_scn, es.ctypes.data_as(C.POINTER(C.c_int32))),
              "d2d_set_scenarios")
        if not self.cfg.scn_pool and n_scn > 1:  # step costs: the grouped layout's co-residency balance
            cost = (C.c_double * n_scn)(*[SCENARIO_STEP_COST.get(s.name.removesuffix("_free"), 32.0)
                                          for s in self.scenarios])
            self._check(self._lib.d2d_set_scenario_costs(self._h, cost, n_scn), "d2d_set_scenario_costs")

    def set_curriculum(self, stage: str | None = None, sim_num: int | None = None, pool: int | None = None,
                       seed: int | None = None) -> torch.Tensor:
        """Regenerate the curriculum pool (explicit ``stage`` or the reference's ``sim_num``
        schedule), upload it and reset every env; returns the reset observations.  Fresh
        curriculum: the schedule restarts at ``sim_num`` (the device step clock is zeroed, so
        sim_num = sim_num + steps taken from here x envs_total); with neither ``stage`` nor
        ``sim_num`` (e.g. ``seed=`` only) it continues from the progress the clock holds."""
        if not self.cfg.scn_pool:
            raise ValueError("set_curriculum needs an env created in curriculum mode (mode='curriculum')")
        if pool is not None and self.fresh:
            raise ValueError("set_curriculum(pool=...) on a fresh-curriculum env: the library and its scenario "
                             "slots are fixed at construction; build the env with curriculum_pool=P instead")
        if stage is not None:
            self.kwargs["scenario"] = stage
        elif sim_num is not None:
            self.kwargs["scenario"] = "curriculum"
            self.kwargs["sim_num"] = int(sim_num)
        elif self.fresh and self.kwargs.get("scenario") not in CURRICULUM_STAGES:
            # neither given, and the stage follows the sim_num schedule (scenario 'curriculum' or any
            # non-stage scenario with mode='curriculum', drone_2d_env.py:324-334 -- the test
            # make_curriculum uses to pick stage 0): the schedule carries on where the device clock
            # has it (the library zeroes the clock, so sim_num0 takes the progress: sim_num + clock x
            # envs_total)
            clock = self.fresh_recipes()[2]
            self.kwargs["sim_num"] = int(self.kwargs.get("sim_num", 0)) + clock * self.envs_total
        self.kwargs["mode"] = "curriculum"
        if pool is not None and not self.fresh:
            self.kwargs["curriculum_pool"] = int(pool)
        if seed is not None:
            self.kwargs["curriculum_seed"] = int(seed)
        self.scenarios = [] if self.fresh else build_scenarios(self.kwargs)
        torch.cuda.synchronize(self.device)
        self._upload_scenarios()
        return self.reset()

    def refresh_curriculum(self, seed: int | None = None, stage: str | None = None, sim_num: int | None = None):
        """Replace the curriculum pool by a fresh draw of the same size WITHOUT stopping the running
        episodes (``d2d_refresh_pool``): resets from now on draw from the new pool, episodes that
        started earlier finish on their own scenarios.  ``seed`` defaults to the previous pool seed
        + 1; ``stage`` / ``sim_num`` optionally move the curriculum on (the reference applies a new
        stage at each env's next reset, drone_2d_env.py:76-86).  Refresh at most once per
        ``n_steps`` steps (the library refuses while an env still runs an episode from the pool
        before the previous refresh)."""
        if self.cfg.scn_pool != 1:
            raise ValueError("refresh_curriculum needs a curriculum pool (mode='curriculum', curriculum_pool=P); "
                             "the fresh curriculum generates every episode's scenario itself")
        kw = dict(self.kwargs, mode="curriculum")
        if stage is not None:
            kw["scenario"] = stage
        elif sim_num is not None:
            kw["scenario"] = "curriculum"
            kw["sim_num"] = int(sim_num)
        kw["curriculum_seed"] = int(seed) if seed is not None else int(kw.get("curriculum_seed", 0)) + 1
        scns = build_scenarios(kw)
        arr = (abi.D2DScn * len(scns))(*[s.to_c() for s in scns])
        self._check(self._lib.d2d_refresh_pool(self._h, arr, len(scns)), "d2d_refresh_pool")
        self.kwargs, self.scenarios = kw, scns

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def close(self):
        for name in ("_renderer", "_hud_renderer"):
            r = getattr(self, name, None)
            if r is not None:
                r.close()
                setattr(self, name, None)
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._lib.d2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ------------------------------------------------------------------ API
    def reset(self, seed: int | None = None, mask: torch.Tensor | None = None) -> torch.Tensor:
        """Reset all envs (or those with ``mask`` set); returns obs [N, 27] float32."""
        sv = int(seed) if seed is not None else self.seed_value
        b = self._bufs[self._k]
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        self._check(self._lib.d2d_reset(self._h, self._ptr(m), C.c_uint64(sv & (2 ** 64 - 1)),
                                  self._ptr(b["obs"]), self._stream()), "d2d_reset")
        # only a reset the library accepted installs the seed (a refused masked fresh-curriculum
        # reset with a new seed leaves the library on the old one, and so must state_dict())
        self.seed_value = sv
        return b["obs"]

    def _prep_actions(self, actions) -> torch.Tensor:
        if not isinstance(actions, torch.Tensor):
            actions = torch.as_tensor(np.asarray(actions, dtype=np.float32))
        a = actions.to(device=self.device, dtype=torch.float32).reshape(self.num_envs, abi.ACT_DIM).contiguous()
        return a

    def step(self, actions):
        """Tensor fast path: returns (obs, reward, terminated, truncated, info) device tensors.

        ``obs`` rows of finished envs already hold the reset observation (auto-reset); their
        pre-reset observation is in ``self.terminal_obs``.  ``info`` is the float32 [N, 12] table
        of include/drone2d.h (D2D_INFO_*), or None when ``with_info=False``.
        """
        a = actions
        if not (type(a) is torch.Tensor and a.dtype is torch.float32 and a.is_cuda and a.shape == self._act_shape
                and a.get_device() == self.device.index and a.is_contiguous()):
            a = self._prep_actions(actions)
        self._k ^= 1
        k = self._k
        st = self._raw_stream(self.device.index) if self._raw_stream else self._stream()
        rc = self._lib.d2d_step(self._h, a.data_ptr(), *self._bufp[k], st)
        if rc:
            self._check(rc, "d2d_step")
        self._last_actions = a  # keep alive until the kernel has consumed it
        b = self._bufs[k]
        return b["obs"], b["rew"], b["term"], b["trunc"], (b["info"] if self.with_info else None)

    @property
    def terminal_obs(self) -> torch.Tensor:
        return self._bufs[self._k]["tobs"]

    def get_state(self):
        st = torch.empty(abi.NSTATE, self.num_envs, dtype=torch.float64, device=self.device)
        ist = torch.empty(abi.NISTATE, self.num_envs, dtype=torch.int32, device=self.device)
        self._check(self._lib.d2d_get_state(self._h, self._ptr(st), self._ptr(ist), self._stream()), "d2d_get_state")
        return st, ist

    def set_state(self, state: torch.Tensor | None, istate: torch.Tensor | None = None):
        st = None if state is None else state.to(self.device, torch.float64).contiguous()
        ist = None if istate is None else istate.to(self.device, torch.int32).contiguous()
        self._check(self._lib.d2d_set_state(self._h, self._ptr(st), self._ptr(ist), self._stream()), "d2d_set_state")
        self._keep = (st, ist)

    def get_env_scenarios(self) -> torch.Tensor:
        """int32 [N]: each env's current scenario index (in curriculum pool mode every reset redraws it)."""
        es = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._check(self._lib.d2d_get_env_scenarios(self._h, self._ptr(es), self._stream()), "d2d_get_env_scenarios")
        return es

    def set_env_scenarios(self, env_scn: torch.Tensor):
        """Restore the per-env scenario indices of a checkpoint (curriculum pool mode only)."""
        es = torch.as_tensor(env_scn).to(self.device, torch.int32).contiguous()
        if es.shape != (self.num_envs,):
            raise ValueError("env_scn must have shape [num_envs]")
        self._check(self._lib.d2d_set_env_scenarios(self._h, self._ptr(es), self._stream()), "d2d_set_env_scenarios")

    def group_layout(self):
        """The slot layout in use (include/drone2d.h d2d_get_group_layout): (slot_env [ns] int32,
        group_scn [groups] int32), or None for the identity layout (one scenario / pool modes)."""
        ng = (self.num_envs + 63) // 64
        se = np.zeros(ng * 64, np.int32)
        gs = np.zeros(ng, np.int32)
        k = self._lib.d2d_get_group_layout(self._h, se.ctypes.data_as(C.c_void_p), gs.ctypes.data_as(C.c_void_p))
        if k < 0:
            self._check(k, "d2d_get_group_layout")
        return (se, gs) if k > 0 else None

    @property
    def generation(self) -> int:
        """Changes whenever the library re-allocates what a captured step graph points at
        (set_scenarios / set_curriculum): holders of a captured graph re-capture it."""
        return int(self._lib.d2d_generation(self._h))


    def scenario_table(self, first: int = 0, count: int | None = None):
        """ABI records (abi.D2DScn array) of scenario-table slots [first, first + count): the pool's two
        halves, or in the fresh curriculum env i's slots 2 i, 2 i + 1 (the oracle replays them)."""
        total = 2 * self.num_envs if self.fresh else 2 * len(self.scenarios)
        count = total - first if count is None else count
        out = (abi.D2DScn * count)()
        self._check(self._lib.d2d_get_scenario_table(self._h, first, count, out), "d2d_get_scenario_table")
        return out

    def fresh_recipes(self):
        """Fresh curriculum: (keys int32[2n], clocks int64[2n], clock) -- every scenario slot's episode
        key and generation clock, and the step clock (what a checkpoint needs to regenerate them)."""
        k = np.zeros(2 * self.num_envs, np.int32)
        c = np.zeros(2 * self.num_envs, np.int64)
        t = C.c_int64()
        self._check(self._lib.d2d_fresh_recipes(self._h, k.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                          C.byref(t), 0), "d2d_fresh_recipes")
        return k, c, int(t.value)

    def state_dict(self) -> dict:
        """Checkpoint of the running batch: physics/bookkeeping state, per-env scenario indices and
        the spawn seed (the reference has no resume path).  Curriculum pool:
        both pool halves' scenarios and which half resets draw from; fresh curriculum: every
        scenario slot's recipe (episode key, clock) and the step clock."""
        st, ist = self.get_state()
        sd = {"state": st, "istate": ist, "env_scn": self.get_env_scenarios(), "seed": self.seed_value}
        if self.cfg.scn_pool == 1:
            base, valid = C.c_int32(), C.c_int32()
            self._check(self._lib.d2d_pool_state(self._h, C.byref(base), C.byref(valid)), "d2d_pool_state")
            recs = self.scenario_table()
            sd["pool"] = {"records": np.frombuffer(bytes(recs), np.uint8).copy(), "active_base": int(base.value),
                          "valid_mask": int(valid.value), "size": len(self.scenarios)}
        elif self.cfg.scn_pool == 2:
            k, c, t = self.fresh_recipes()
            sd["fresh"] = {"keys": k, "clocks": c, "clock": t}
        return sd

    def load_state_dict(self, sd: dict):
        """Restore a ``state_dict()`` into a batch built with the same kwargs: episodes continue
        exactly where they were (pool mode: on the saved pool, whatever this batch's own pool is)."""
        self.seed_value = int(sd["seed"])
        self.reset()  # installs the seed for later auto-resets; the state is overwritten below
        if self.cfg.scn_pool == 1:
            pool = sd.get("pool")
            if pool is None:
                raise ValueError("pool-mode checkpoint without its pool (saved by an older version)")
            if int(pool["size"]) != len(self.scenarios):
                raise ValueError("checkpoint pool size differs from this batch's curriculum_pool")
            recs = (abi.D2DScn * (2 * int(pool["size"]))).from_buffer_copy(np.asarray(pool["records"]).tobytes())
            self._check(self._lib.d2d_restore_pool(self._h, recs, len(recs), int(pool["active_base"]),
                                             int(pool["valid_mask"])), "d2d_restore_pool")
            self.set_env_scenarios(sd["env_scn"])
        elif self.cfg.scn_pool == 2:
            f = sd["fresh"]
            k = np.ascontiguousarray(f["keys"], np.int32)
            c = np.ascontiguousarray(f["clocks"], np.int64)
            if k.shape != (2 * self.num_envs,):
                raise ValueError("checkpoint has a different number of envs")
            t = C.c_int64(int(f["clock"]))
            self._check(self._lib.d2d_fresh_recipes(self._h, k.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                              C.byref(t), 1), "d2d_fresh_recipes")
        elif not torch.equal(torch.as_tensor(sd["env_scn"]).cpu(), self.get_env_scenarios().cpu()):
            raise ValueError("checkpoint env -> scenario map differs from this batch's (static map)")
        self.set_state(sd["state"], sd["istate"])

    # ------------------------------------------------------------------ rendering
    def _render_ids(self, env_ids) -> torch.Tensor:
        if env_ids is None:
            env_ids = range(min(self.num_envs, 16))
        ids = torch.as_tensor(list(env_ids) if not isinstance(env_ids, (torch.Tensor, np.ndarray)) else env_ids)
        ids = ids.to(torch.int64).reshape(-1).cpu()
        if len(ids) and (int(ids.min()) < 0 or int(ids.max()) >= self.num_envs):
            raise ValueError("env_ids out of range")
        return ids

    def render_scenarios(self, env_ids=None, istate: torch.Tensor | None = None):
        """The ABI record (abi.D2DScn array) of the scenario each of ``env_ids`` is running now -- what
        ``render`` draws: the static map's entry; in curriculum pool mode the table slot
        ``get_env_scenarios`` names; in the fresh curriculum the slot of the running episode,
        2 i + ((episode - 1) & 1) (csrc/d2d_kernels.h fresh_slot)."""
        ids = self._render_ids(env_ids).numpy()
        if not self.cfg.scn_pool:
            return (abi.D2DScn * len(ids))(*[self.scenarios[int(self.env_scenario[i])].to_c() for i in ids])
        if self.fresh:
            ist = self.get_state()[1] if istate is None else istate
            ep = ist[abi.I_EPISODE].cpu().numpy()[ids]
            slots = 2 * ids + ((ep - 1) & 1)
        else:
            slots = self.get_env_scenarios().cpu().numpy()[ids]
        if not len(slots):
            return (abi.D2DScn * 0)()
        lo, hi = int(slots.min()), int(slots.max())
        table = self.scenario_table(lo, hi - lo + 1)
        return (abi.D2DScn * len(ids))(*[table[int(k) - lo] for k in slots])

    def render(self, env_ids=None, size=256, layers: int | None = None, trails=None, text: bool = False,
               arcs: bool = False, shades=None) -> torch.Tensor:
        """Frames of the envs ``env_ids`` (default: the first min(num_envs, 16)) as they are now:
        uint8 [K, H, W, 3] on the env's device, drawn by libd2d_render.so (drone2d_amd.render has the
        picture model).  ``size``: an int or (H, W); ``layers``: a mask of render.L_* (default all);
        ``trails``: (xy float32 [K, T, 2] world positions, length int32 [K]) or None.  Each frame shows
        the env's running scenario, its state, its current observation's closest and lookahead points
        and the last action's forces.  The renderer and its library are created on first use.
        ``text``: the six lines of reward terms from the last step's info table; ``arcs``: the angle
        arcs of the three guide lines; ``shades``: a ``hud.ShadeRecorder`` over the same ``env_ids`` or a
        (poses float64 [K, S, 3], count int32 [K]) pair.  Any of the three goes through libd2d_hud.so
        (drone2d_amd.hud); with all at their defaults nothing of it is loaded."""
        from . import render as R

        if text or arcs or shades is not None:
            return self._render_hud(env_ids, size, layers, trails, bool(text), bool(arcs), shades)

        ids = self._render_ids(env_ids)
        k = len(ids)
        h, w = R._size(size)
        if k == 0:
            return torch.empty((0, h, w, 3), dtype=torch.uint8, device=self.device)
        tr, tl = self._render_trails(trails, k)
        need_trail = int(tr.shape[1]) if tr is not None else 0
        r = getattr(self, "_renderer", None)
        if r is None or r.max_frames < k or r.max_trail < need_trail:
            caps = (max(k, 16, r.max_frames if r else 0), max(need_trail, r.max_trail if r else 0))
            if r is not None:
                r.close()
            r = self._renderer = R.Renderer(self.device, max_frames=caps[0], max_trail=caps[1])
        tr = self._pad_rows(tr, r.max_trail)  # the library's trail rows are max_trail long
        return r.render(*self._render_inputs(r, ids), tr, tl, size=(h, w), screen=(self.cfg.screen_w, self.cfg.screen_h),
                        layers=R.L_ALL if layers is None else int(layers))

    @staticmethod
    def _render_trails(trails, k: int):
        if trails is None:
            return None, None
        tr, tl = trails
        tr = torch.as_tensor(tr, dtype=torch.float32)
        tl = torch.as_tensor(tl, dtype=torch.int32)
        if tr.dim() != 3 or tuple(tr.shape[::2]) != (k, 2) or tuple(tl.shape) != (k,):
            raise ValueError("trails must be (xy [K, T, 2], length [K])")
        return tr, tl

    @staticmethod
    def _pad_rows(t, n: int):
        """[K, m, c] -> [K, n, c], zero-filled (None stays None)."""
        if t is None or t.shape[1] >= n:
            return t
        return torch.cat([t, t.new_zeros(t.shape[0], n - t.shape[1], t.shape[2])], 1)

    def _render_inputs(self, r, ids):
        """What a frame of each of ``ids`` is drawn from, on the device: the running scenario's record,
        the state columns, the current observation and the last action (None before the first step)."""
        st, ist = self.get_state()
        dids = ids.to(self.device)
        if not self.cfg.scn_pool:
            if self._render_table is None:
                self._render_table = r.scn_tensor(self.scenarios)
            scn = self._render_table[torch.as_tensor(self.env_scenario, dtype=torch.int64)[ids].to(self.device)]
        else:
            scn = r.scn_tensor(self.render_scenarios(ids, ist))
        act = getattr(self, "_last_actions", None)
        return scn, st[:, dids], self._bufs[self._k]["obs"][dids], act[dids] if act is not None else None

    def _render_hud(self, env_ids, size, layers, trails, text, arcs, shades) -> torch.Tensor:
        """``render`` with the text overlay, the arcs or the shades: the same inputs, and the info
        table's rows and the shade lists, through ``hud.HudRenderer``."""
        from . import hud as H
        from . import render as R

        if text and not self.with_info:
            raise ValueError("render(text=True) prints the step's info table: the env needs with_info=True")
        ids = self._render_ids(env_ids)
        k = len(ids)
        h, w = R._size(size)
        if k == 0:
            return torch.empty((0, h, w, 3), dtype=torch.uint8, device=self.device)
        tr, tl = self._render_trails(trails, k)
        sp = sc = None
        if shades is not None:
            if isinstance(shades, H.ShadeRecorder):
                if not np.array_equal(shades.env_ids, ids.numpy()):
                    raise ValueError("the ShadeRecorder tracks other env_ids than render was asked for")
                shades = shades.shades()
            sp = torch.as_tensor(shades[0], dtype=torch.float64)
            sc = torch.as_tensor(shades[1], dtype=torch.int32)
            if sp.dim() != 3 or tuple(sp.shape[::2]) != (k, 3) or sp.shape[1] < 1 or tuple(sc.shape) != (k,):
                raise ValueError("shades must be a ShadeRecorder or (poses [K, S, 3], count [K])")
        need_trail = int(tr.shape[1]) if tr is not None else 0
        need_shades = int(sp.shape[1]) if sp is not None else 0
        r = getattr(self, "_hud_renderer", None)
        if r is None or r.max_frames < k or r.max_trail < need_trail or r.max_shades < need_shades:
            caps = (max(k, 16, r.max_frames if r else 0), max(need_trail, r.max_trail if r else 0),
                    max(need_shades, r.max_shades if r else 0))
            if r is not None:
                r.close()
            r = self._hud_renderer = H.HudRenderer(self.device, max_frames=caps[0], max_trail=caps[1], max_shades=caps[2])
        tr = self._pad_rows(tr, r.max_trail)  # the library's rows are max_trail / max_shades long
        if sp is not None and need_shades < r.max_shades:
            sp = self._pad_rows(sp, r.max_shades)
            sc = sc.clamp(max=need_shades)  # a count beyond the caller's capacity must not reach into the padding
        mask = (R.L_ALL if layers is None else int(layers)) & R.L_ALL
        mask |= (H.L_TEXT if text else 0) | (H.L_ARCS if arcs else 0) | (H.L_SHADE if sp is not None else 0)
        info = self._bufs[self._k]["info"][ids.to(self.device)] if text else None
        return r.render(*self._render_inputs(r, ids), tr, tl, info, (sp, sc) if sp is not None else None, size=(h, w),
                        screen=(self.cfg.screen_w, self.cfg.screen_h), layers=mask)

    def episode_stats(self, clear: bool = True) -> torch.Tensor:
        """float64 [8]: (sum return, episodes, successes, fails, collisions, sum APE, sum len, 0)."""
        self._check(self._lib.d2d_episode_stats(self._h, self._ptr(self._stats), 1 if clear else 0, self._stream()),
              "d2d_episode_stats")
        return self._stats


def info_dicts(info_row: np.ndarray, n_obstacles: int | None = None) -> dict:
    """Rebuild the reference's ``info`` dict (drone_2d_env.py:575-613) from one info row.

    ``dist_closest_obs`` is taken as the kernel wrote it: +inf for an obstacle-free scenario
    (drone_2d_env.py:587), so it is right for every env even in curriculum pool mode, where the
    scenario changes at every reset.  ``n_obstacles`` is accepted for compatibility and unused.
    """
    cause = int(info_row[abi.INFO_CAUSE])
    d = {
        "reward": float(info_row[abi.INFO_REWARD]),
        "collision_avoidance_reward": float(info_row[abi.INFO_CA]),
        "path_adherence": float(info_row[abi.INFO_PA]),
        "path_progression": float(info_row[abi.INFO_PP]),
        "collision_reward": float(info_row[abi.INFO_COLL]),
        "reach_end_reward": float(info_row[abi.INFO_REACH]),
        "agressive_alpha_reward": float(info_row[abi.INFO_AA]),
        "env_steps": int(info_row[abi.INFO_STEPS]),
        "dist_closest_obs": float(info_row[abi.INFO_DCLOSE]),
        "APE": 0, "total_reward": 0, "n_collisions": 0, "n_successful_runs": 0, "n_failed_runs": 0,
        "flight_path": 0,
    }
    if cause:
        c1, c2 = bool(cause & abi.END_COLLISION), bool(cause & abi.END_REACH)
        c4, c5 = bool(cause & abi.END_TIMEUP), bool(cause & abi.END_AA)
        # the same overwrite order as drone_2d_env.py:595-610
        if c1:
            d["n_collisions"], d["n_failed_runs"] = 1, 1
        if c2:
            d["n_collisions"], d["n_successful_runs"] = 0, 1
        if c4:
            d["n_collisions"], d["n_failed_runs"] = 0, 1
        if c5:
            d["n_collisions"], d["n_failed_runs"] = 0, 1
        d["APE"] = float(info_row[abi.INFO_APE])
        d["total_reward"] = float(info_row[abi.INFO_TOTREW])
    return d


class Drone2dEnv:
    """Single environment with the reference's gym-0.21 API (``reset() -> obs``,
    ``step(a) -> (obs, reward, done, info)``), backed by a 1-env HIP batch.

    Differences, all deliberate: observations are float32 values returned as a float64 array
    (the reference builds float64 from the same expressions); the spawn draw comes from the
    library's Philox stream instead of Python's unseeded ``random``; ``render`` draws
    ``rgb_array`` frames with the project's own picture model (drone2d_amd.render) and opens no
    window.  ``render(mode="rgb_array", hud=True)`` adds what ``render_text`` / ``render_shade`` /
    ``shade_distance`` switch on in the reference, and the angle arcs (drone2d_amd.hud); without
    ``hud`` those keys are ignored, as ``render_sim`` always is.
    """

    metadata = {"render.modes": ["rgb_array"]}

    def __init__(self, **kwargs):
        self.kwargs = dict(kwargs)
        self._venv = Drone2dVecEnv(1, seed=int(kwargs.get("seed", 0)), auto_reset=False,
                                   **{k: v for k, v in kwargs.items() if k != "seed"})
        self.action_space = self._venv.action_space
        self.observation_space = self._venv.observation_space
        self.flight_path = []
        self._done = False
        self._shades = None  # render(hud=True)'s one-env recorder, kept from construction when render_shade is set
        self.reset()  # the reference spawns in __init__ (drone_2d_env.py:144)
        if self.kwargs.get("render_shade"):
            from .hud import ShadeRecorder

            self._shades = ShadeRecorder(self._venv, [0], distance=float(self.kwargs.get("shade_distance", 75)))

    def seed(self, seed=None):
        if seed is not None:
            self._venv.seed_value = int(seed)
        return [self._venv.seed_value]

    def reset(self):
        obs = self._venv.reset()
        self._done = False
        self.flight_path = []
        if self._shades is not None:
            self._shades.restart()
        return obs[0].double().cpu().numpy()

    def step(self, action):
        a = torch.as_tensor(np.asarray(action, dtype=np.float32)).reshape(1, 2)
        obs, rew, term, trunc, info = self._venv.step(a)
        if self._shades is not None:
            self._shades.update(torch.zeros_like(term), torch.zeros_like(trunc))  # no auto-reset here: never a restart
        o = obs[0].double().cpu().numpy()
        r = float(rew[0].item())
        done = bool(term[0].item() or trunc[0].item()) or self._done  # self.done is sticky (:594)
        d = info_dicts(info[0].cpu().numpy())
        if self.kwargs.get("render_path"):
            st, _ = self._venv.get_state()
            x, y = float(st[0, 0]), float(st[1, 0])
            self.flight_path.append((x, float(self.kwargs["screensize_y"]) - y))
            if done:
                d["flight_path"] = list(self.flight_path)
        self._done = done
        return o, r, done, d

    def render(self, mode="human", close=False, hud=False):
        """``mode="rgb_array"``: the frame at the screen size, uint8 [screensize_y, screensize_x, 3],
        with the flight path so far as the trail when ``render_path`` is set.  ``"human"``: None (no
        window is opened).  ``hud=True``: the angle arcs, the text overlay when ``render_text`` is set
        (once a step has filled the info table) and the shades when ``render_shade`` is."""
        if mode != "rgb_array":
            return None
        H, W = int(self.kwargs["screensize_y"]), int(self.kwargs["screensize_x"])
        trails = None
        if self.kwargs.get("render_path"):
            cap = int(self.kwargs["n_steps"]) + 1
            xy = np.zeros((1, cap, 2), np.float32)
            fp = np.asarray(self.flight_path[-cap:], np.float64).reshape(-1, 2)  # (x, screen_height - y)
            xy[0, :len(fp), 0] = fp[:, 0]
            xy[0, :len(fp), 1] = float(self.kwargs["screensize_y"]) - fp[:, 1]
            trails = (xy, np.array([len(fp)], np.int32))
        if not hud:
            return self._venv.render([0], size=(H, W), trails=trails)[0].cpu().numpy()
        text = bool(self.kwargs.get("render_text")) and hasattr(self._venv, "_last_actions")
        return self._venv.render([0], size=(H, W), trails=trails, text=text, arcs=True,
                                 shades=self._shades)[0].cpu().numpy()

    def close(self):
        self._venv.close()
