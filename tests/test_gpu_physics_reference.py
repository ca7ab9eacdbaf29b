"""The HIP step kernels' physics against the 50-digit evaluation of Chipmunk's sequence, within eight
times the unfused float64 restatement's own error (tests/physics_ref.py) -- needs an MI355X.

Every case of every family is one env of a batch (``auto_reset=False``, ``set_state``, one ``step``,
``get_state``); a batch holds the cases of one scenario (the single-scenario kernel) or all of them
under a mixed ``env_scenario`` map (the grouped kernel, same physics body).  Checked: the family error
per column group against ``bound(floor)``; the contact flag against the truth's; and that a case's result
does not depend, bit for bit, on the batch size or on the lane and wave it runs in -- including waves
in which exactly one lane has a circle in reach of ``frame_hits``' wave-uniform skip, and one with none.
"""
import numpy as np
import pytest
import torch

import physics_ref as R

pytestmark = pytest.mark.gpu


def _run_batch(d2, scenario, env_scenario, idx, exact=False):
    """Step the cases ``idx`` once as one batch; (post [n, 30] float64, contact flag [n])."""
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    cases = R.cases()
    n = len(idx)
    venv = d2.Drone2dVecEnv(n, env_scenario=env_scenario, auto_reset=False, exact_trig=exact,
                            **dict(ENV_TRAIN_CONFIG, scenario=scenario))
    try:
        venv.reset(seed=0)
        st = torch.as_tensor(np.ascontiguousarray(np.stack([cases[i].pre for i in idx]).T))
        venv.set_state(st, torch.zeros(3, n, dtype=torch.int32))
        venv.step(torch.as_tensor(np.stack([cases[i].act for i in idx]).astype(np.float32)))
        st2, ist2 = venv.get_state()
        return st2.cpu().numpy().T[:, :R.NPHYS].copy(), (ist2[1].cpu().numpy() & 1).astype(bool)
    finally:
        venv.close()


def _run_layout(d2, layout, exact=False):
    """``layout``: [(scenario index, [case index, ...])], one single-scenario batch each."""
    return [_run_batch(d2, R.SCENARIOS[s], None, idx, exact) for s, idx in layout if idx]


def _by_scenario(keep=lambda c: True):
    cases = R.cases()
    return [(s, [i for i, c in enumerate(cases) if c.scn == s and keep(c)]) for s in range(len(R.SCENARIOS))]


def _per_case(layout, results):
    """{case index: (post row, flag)} of a layout in which every case appears once."""
    out = {}
    for (_, idx), (post, flag) in zip([b for b in layout if b[1]], results):
        for k, i in enumerate(idx):
            assert i not in out
            out[i] = (post[k], bool(flag[k]))
    return out


def _check(per_case):
    """Family errors within bound(floor) and contact flags equal to the truth's, for the cases run."""
    cases, T, floors = R.cases(), R.truth(), R.floors()
    posts = [None if (i not in per_case or c.flag_only) else per_case[i][0] for i, c in enumerate(cases)]
    errs = R.family_errors(cases, posts, T.post, T.num)
    print(R.describe(errs, floors))
    # a family is either run whole or not at all: its floor is the maximum over all of its cases
    ran = {c.family for i, c in enumerate(cases) if i in per_case}
    assert all((i in per_case) for i, c in enumerate(cases) if c.family in ran)
    assert not R.violations(errs, floors)
    wrong = [getattr(cases[i], "note", cases[i].family) for i in per_case
             if T.decided[i] and per_case[i][1] != T.flag[i]]
    assert not wrong, wrong
    return errs


@pytest.fixture(scope="module")
def identity(d2):
    """Every case once, in order, one batch per scenario, default build."""
    layout = _by_scenario()
    return _per_case(layout, _run_layout(d2, layout))


def _assert_same_bits(per_case, identity):
    cases = R.cases()
    for i, (post, flag) in per_case.items():
        assert post.tobytes() == identity[i][0].tobytes(), (i, cases[i].family)
        assert flag == identity[i][1], (i, cases[i].family)


def test_families_within_bound(identity):
    assert len(identity) == len(R.cases())
    errs = _check(identity)
    assert set(errs) == set(R.floors())


def test_exact_trig_build(d2):
    """The build that takes the sincos branch only, on the families it differs on."""
    layout = _by_scenario(lambda c: c.family.startswith("golden/") or c.family == "motor_small")
    errs = _check(_per_case(layout, _run_layout(d2, layout, exact=True)))
    assert "motor_small" in errs and len(errs) == 8


def test_mixed_scenario_map(d2):
    """All cases in one batch under a mixed env -> scenario map: the grouped kernel."""
    cases = R.cases()
    idx = list(range(len(cases)))
    post, flag = _run_batch(d2, list(R.SCENARIOS), np.array([c.scn for c in cases], np.int32), idx)
    _check({i: (post[i], bool(flag[i])) for i in idx})


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_batch_size(d2, identity, n):
    """The first n cases of the largest batches: a ragged last workgroup changes no case's result."""
    for s, idx in _by_scenario():
        if R.SCENARIOS[s] in ("large", "corridor"):
            assert len(idx) > 65
            post, flag = _run_batch(d2, R.SCENARIOS[s], None, idx[:n])
            _assert_same_bits({i: (post[k], bool(flag[k])) for k, i in enumerate(idx[:n])}, identity)


def test_permuted_lanes(d2, identity):
    rng = np.random.default_rng(5)
    layout = [(s, [idx[k] for k in rng.permutation(len(idx))]) for s, idx in _by_scenario()]
    per_case = _per_case(layout, _run_layout(d2, layout))
    assert len(per_case) == len(R.cases())
    _assert_same_bits(per_case, identity)


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_one_lane_near_a_circle(d2, identity, lane):
    """Each contact case alone in a wave of resting rigs out of every circle's reach, at ``lane``; the
    last wave has no lane in reach at all.  The contact flags are the truth's, and neither the contact
    cases nor the padding differ by a bit from the full batches' results."""
    cases, T = R.cases(), R.truth()
    pad = next(i for i, c in enumerate(cases) if getattr(c, "pad", False))
    for name in ("large", "corridor"):
        s = R.SCENARIOS.index(name)
        contact = [i for i, c in enumerate(cases) if c.family == "contact" and c.scn == s]
        assert len(contact) >= 20
        idx = []
        for i in contact:
            wave = [pad] * 64
            wave[lane] = i
            idx += wave
        idx += [pad] * 64
        post, flag = _run_batch(d2, name, None, idx)
        for k, i in enumerate(idx):
            assert post[k].tobytes() == identity[i][0].tobytes(), (k, i)
            assert bool(flag[k]) == identity[i][1] == T.flag[i], (k, getattr(cases[i], "note", "pad"))
