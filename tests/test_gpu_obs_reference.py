"""The HIP kernels' observation, reward, end causes and info against the 50-digit evaluation of the
reference's sequence, at float32 resolution and within eight times the float64 restatement's own error
(tests/obs_ref.py) -- needs an MI355X.

Step route: every case is one env of a batch (``auto_reset=False``, ``set_state``, one ``step``,
``get_state``); the returned float64 state is what the kernel observed, and truth, restatement and floors
are evaluated there.  Reset route: scenarios whose spawn rectangle is a point, and the shipped scenarios'
spawn draws, through ``reset()``.  Checked: every float32 output inside ``[RN32(truth - m), RN32(truth + m)]``,
state columns 30 and 31 within ``m``, every decision equal to the truth's (all decided at the observed
states), and that a case's bits do not depend on the batch size, the lane, the wave's other lanes, or on
whether its observation is handed out by the step, as ``terminal_obs``, from the reset cache or by ``reset``.
"""
import functools

import numpy as np
import pytest
import torch

import obs_ref as R

pytestmark = pytest.mark.gpu

EXACT_FAMILIES = ("bearing_axes", "big_angle", "coincident", "tiny_vector", "reward_thresholds")


class HipEnv:
    """Drone2dVecEnv behind obs_ref.run_batch's interface (NumPy in and out)."""

    def __init__(self, d2, n, scns, env_scenario, cfgkey, exact=False, auto_reset=False):
        self.v = d2.Drone2dVecEnv(n, env_scenario=env_scenario, auto_reset=auto_reset, exact_trig=exact,
                                  **dict(R.cfg_kwargs(cfgkey), scenario=list(scns)))

    def reset(self, seed, mask=None):
        m = None if mask is None else torch.as_tensor(np.asarray(mask, np.uint8))
        return self.v.reset(seed=seed, mask=m).cpu().numpy().copy()

    def set_state(self, st, ist):
        self.v.set_state(torch.as_tensor(st), torch.as_tensor(ist))

    def step(self, act):
        return tuple(x.cpu().numpy().copy() for x in self.v.step(torch.as_tensor(act, device=self.v.device)))

    def terminal_obs(self):
        return self.v.terminal_obs.cpu().numpy().copy()

    def get_state(self):
        st, ist = self.v.get_state()
        return st.cpu().numpy(), ist.cpu().numpy()

    def close(self):
        self.v.close()


class PoolEnv(HipEnv):
    """A curriculum-pool handle whose pool d2d_refresh_pool replaces by the case scenarios: every lane reads
    its scenario's tables from global memory."""

    def __init__(self, d2, n, scns, env_scenario, cfgkey, exact=False, auto_reset=False):
        from drone2d_amd import abi

        kw = dict(R.cfg_kwargs(cfgkey), scenario="stage_5", mode="curriculum", curriculum_pool=len(scns), curriculum_seed=9)
        self.v = d2.Drone2dVecEnv(n, seed=R.SEED, auto_reset=auto_reset, exact_trig=exact, **kw)
        assert self.v.cfg.scn_pool == 1 and len(self.v.scenarios) == len(scns)
        self.v.reset(seed=R.SEED)
        pool = [s.to_c() for s in scns]
        # (the package offers no call that uploads a pool of one's own; as test_gpu_limit_scenarios.py does)
        self.v._check(self.v._lib.d2d_refresh_pool(self.v._h, (abi.D2DScn * len(pool))(*pool), len(pool)), "d2d_refresh_pool")
        self.es = torch.as_tensor(np.asarray(env_scenario, np.int32) + len(scns))   # the half the refresh filled

    def reset(self, seed, mask=None):
        assert mask is None
        return None

    def set_state(self, st, ist):
        self.v.set_env_scenarios(self.es)
        super().set_state(st, ist)
        assert (self.v.get_env_scenarios().cpu() == self.es).all()


@pytest.fixture(scope="module")
def make(d2):
    return functools.partial(HipEnv, d2)


def _run(make_env, keep=lambda c: True, per_scenario=False, **kw):
    """{case index: Out} of the cases ``keep`` selects, in batches (obs_ref.batches)."""
    cases = R.cases()
    outs = {}
    for idx in R.batches(keep, per_scenario):
        for i, o in zip(idx, R.run_batch(make_env, [cases[i] for i in idx], mixed=not per_scenario or cases[idx[0]].route == "reset", **kw)):
            outs[i] = o
    return outs


def _check(outs):
    """Every output of the cases run within the bound at the states observed, every decision the truth's,
    every case decided; families are run whole (a floor is the maximum over all of a family's cases)."""
    cases = R.cases()
    ran = {cases[i].family for i in outs}
    assert all(i in outs for i, c in enumerate(cases) if c.family in ran)
    idx = sorted(outs)
    evals = [R.eval_at(i, outs[i]) for i in idx]
    floors = R.floors_of([cases[i] for i in idx], evals)
    chk = R.Check(floors)
    und = []
    for i, ev in zip(idx, evals):
        R.compare(chk, i, outs[i])
        u = R.undecided(cases[i], ev, floors)
        if u:
            und.append((cases[i].family, cases[i].note, u))
    print(R.describe(floors))
    print(chk.summary())
    assert not und, und[:5]
    assert not chk.bad, chk.bad[:10]
    return chk


@pytest.fixture(scope="module")
def identity(make):
    """Every case once, default build: the step route one batch per scenario (the single-scenario kernel),
    the reset route one batch."""
    return _run(make, per_scenario=True)


def test_families_within_bound(identity):
    assert len(identity) == len(R.cases())
    chk = _check(identity)
    assert set(chk.worst) == {c.family for c in R.cases()}


def test_exact_trig_build(d2):
    """The build that follows the reference's atan2 -> ssa -> sincos sequence everywhere, on the families
    where the two builds differ."""
    chk = _check(_run(functools.partial(HipEnv, d2), lambda c: c.family in EXACT_FAMILIES, per_scenario=True, exact=True))
    assert set(chk.worst) == set(EXACT_FAMILIES)


def test_mixed_scenario_map(d2, make, identity):
    """All step-route cases in one batch under a mixed env -> scenario map (the grouped kernel), and through a
    curriculum-pool handle whose pool the case scenarios replace (per-lane tables in global memory)."""
    step = lambda c: c.route == "step"   # noqa: E731
    grouped = _run(make, step)
    assert len(R.batches(step)) == 2     # ENV_TRAIN_CONFIG, and the two cases with use_lambda off
    _check(grouped)
    pool = _run(functools.partial(PoolEnv, d2), step)
    _check(pool)
    # (a measurement, no assertion: these are other kernels than the single-scenario one)
    for name, outs in (("grouped", grouped), ("pool", pool)):
        print(name, "cases whose bits differ from the single-scenario batches':",
              sum(not R.same_bits(outs[i], identity[i]) for i in outs), "of", len(outs))


def _largest_step_batch():
    idx = max((b for b in R.batches(lambda c: c.route == "step" and c.cfgkey == "train", per_scenario=True)), key=len)
    assert len(idx) > 65
    return idx


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_size(make, identity, n):
    """The first n cases of the largest single-scenario batch: a ragged last workgroup changes no bit."""
    cases = R.cases()
    idx = _largest_step_batch()[:n]
    for i, o in zip(idx, R.run_batch(make, [cases[i] for i in idx], mixed=False)):
        assert R.same_bits(o, identity[i]), (cases[i].family, cases[i].note)


def test_permuted_lanes(make, identity):
    cases = R.cases()
    rng = np.random.default_rng(5)
    for idx in R.batches(lambda c: c.route == "step", per_scenario=True):
        perm = [idx[k] for k in rng.permutation(len(idx))]
        for i, o in zip(perm, R.run_batch(make, [cases[i] for i in perm], mixed=False)):
            assert R.same_bits(o, identity[i]), (cases[i].family, cases[i].note)


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_one_lane_in_need(make, identity, lane):
    """Each nearest3 case alone at ``lane`` in a wave of resting rigs far from every circle: the lane that needs
    the top-4 insertion (the wave-uniform skip) or the square root's fix-up (a vertex on a centre) is the
    only one of its wave."""
    cases = R.cases()
    ran = 0
    for idx in R.batches(lambda c: c.family == "nearest3", per_scenario=True):
        assert len(idx) <= 7
        pad = R.pad_case(cases[idx[0]].scn)
        cs = []
        for i in idx:
            wave = [pad] * 64
            wave[lane] = cases[i]
            cs += wave
        outs = R.run_batch(make, cs, mixed=False)
        for k, i in enumerate(idx):
            assert R.same_bits(outs[64 * k + lane], identity[i]), (cases[i].note, lane)
            ran += 1
        pads = [o for k, o in enumerate(outs) if k % 64 != lane]
        assert all(R.same_bits(o, pads[0]) for o in pads)
    assert ran == sum(c.family == "nearest3" for c in cases)


def test_terminal_and_reset_obs(make, identity):
    """With auto_reset, ``terminal_obs`` of every case that ends is the auto_reset=False observation bit for
    bit; the observation returned in its place (the reset cache's) is within the bound at the state
    ``get_state()`` reports; and a masked ``reset`` of the same envs of a handle without auto_reset gives
    the same bits."""
    cases = R.cases()
    idx = [i for i, c in enumerate(cases) if c.route == "step" and c.cfgkey == "train"]
    cs = [cases[i] for i in idx]
    used = sorted({c.scn for c in cs})
    es = np.array([used.index(c.scn) for c in cs], np.int32)
    scns = [R.scenarios()[s] for s in used]
    res = {}
    for auto in (True, False):
        env = make(len(cs), scns, es, "train", auto_reset=auto)
        try:
            env.reset(R.SEED)
            R.set_cases(env, cs)
            outs = R.step_outs(env, cs)
            tobs = env.terminal_obs() if auto else None
            robs = None
            if not auto:
                ended = np.array([o.term or o.trunc for o in outs])
                robs = env.reset(R.SEED, mask=ended)
                st, ist = env.get_state()
                for k, o in enumerate(outs):
                    o.st, o.ist = st[:, k].copy(), ist[:, k].copy()
            res[auto] = (outs, tobs, robs)
        finally:
            env.close()
    (a_outs, a_tobs, _), (m_outs, _, m_robs) = res[True], res[False]
    ended = [k for k, i in enumerate(idx) if R.eval_at(i, identity[i]).cause != 0]
    assert len(ended) >= 40
    reset_cases, reset_outs = [], []
    for k in ended:
        i = idx[k]
        assert a_outs[k].term and m_outs[k].term, cases[i].note
        assert a_tobs[k].tobytes() == m_outs[k].obs.tobytes(), cases[i].note
        assert np.float32(a_outs[k].rew).tobytes() == np.float32(m_outs[k].rew).tobytes(), cases[i].note
        # the observation handed out in the terminal one's place, and the masked reset's
        assert a_outs[k].obs.tobytes() == m_robs[k].tobytes(), cases[i].note
        assert a_outs[k].st.tobytes() == m_outs[k].st.tobytes() and (a_outs[k].ist == m_outs[k].ist).all(), cases[i].note
        reset_cases.append(R.Case(family="auto_reset", note="after " + cases[i].note, route="reset", scn=cases[i].scn,
                                  cfgkey="train", view=cases[i].view, cfg=cases[i].cfg))
        reset_outs.append(a_outs[k])
    for k, i in enumerate(idx):
        if k not in ended:
            assert a_outs[k].obs.tobytes() == m_outs[k].obs.tobytes(), cases[i].note
    evals = [R.evaluate(c, o.st, R.closest_u(c.scn, o.st[0], o.st[1])) for c, o in zip(reset_cases, reset_outs)]
    floors = R.floors_of(reset_cases, evals)
    chk = R.Check(floors)
    for c, o, ev in zip(reset_cases, reset_outs, evals):
        for j in range(R.OBS_DIM):
            chk.f32(c, ev, j, o.obs[j], "reset obs")
        chk.equal(c, "flags", int(o.ist[1]), ev.flags)
        chk.equal(c, "t", int(o.ist[0]), 0)
        assert not R.undecided(c, ev, floors), c.note
    print(chk.summary())
    assert not chk.bad, chk.bad[:10]
