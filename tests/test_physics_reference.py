"""Pin the physics step to an unfused restatement of Chipmunk's sequence and to a 50-digit evaluation
of it (tests/physics_ref.py); no GPU.

1. the unfused float64 restatement equals the physics columns of both golden fixtures bit for bit, so
   physics_ref is tied to the fixtures and through them to tests/golden/ref_shims.py;
2. the C oracle (both builds) stays within ``bound(floor)`` of the truth on every case family and
   column group, where the floor is the unfused restatement's own error there; its contact flag equals
   the truth's;
3. five wrong steps switched on inside the restatement each exceed that bound on some family, and the
   right step with the kernel's series for the motors' sin / cos does not.
"""
import ctypes as C
import math

import numpy as np
import pytest

import physics_ref as R
from conftest import load_golden


# ---------------------------------------------------------------------------- 1. fixtures, bitwise
@pytest.mark.parametrize("which", ["traj", "crafted"])
def test_unfused_equals_golden_bitwise(which):
    """Every row: ``pre``, ``act`` and the float32 thrust give columns 0..29 of ``post`` exactly.  The step
    after a spawn is taken like every other, with ``curr_dt = 1/60`` (make_golden.set_state): the cached
    impulses are zero there, so ``dt_coef`` = 1 applies the same zeros as Chipmunk's 0."""
    g = load_golden(which)
    pre, act, want = g["pre"], g["act"], g["post"]
    assert len(pre) >= 1000
    bad = []
    for k in range(len(pre)):
        fL, fR = R.thrust(act[k])
        post, _ = R.step(pre[k], fL, fR, float, math.sin, math.cos)
        if np.asarray(post, np.float64).tobytes() != np.ascontiguousarray(want[k][:R.NPHYS]).tobytes():
            bad.append(k)
    assert not bad, (len(bad), bad[:10])


def test_truth_contact_flag_equals_golden(golden_crafted):
    """The 50-digit contact predicate on the post-update pose gives the recorded collision bit."""
    g = golden_crafted
    num = R.mp_number()
    pre, act, scn, pre_i, post_i = g["pre"], g["act"], g["scn"], g["pre_i"], g["post_i"]
    assert not pre_i[:, 1].any() and post_i[:, 1].sum() > 50
    bad = []
    for k in range(len(pre)):
        fL, fR = R.thrust(act[k])
        _, pose = R.step(pre[k], fL, fR, num.N, num.sin, num.cos, positions_only=True)
        if R.touches(pose, R.circles_of(int(scn[k])), num.N) != bool(post_i[k, 1]):
            bad.append(k)
    assert not bad, bad[:10]


def test_scenario_circles_are_the_library_s(scenarios_c):
    """physics_ref reads the circles from scenarios.npz; the library's scenarios hold the same."""
    for si, scn in enumerate(scenarios_c):
        got = [(scn.cx[k], scn.cy[k], scn.cr[k]) for k in range(scn.n_circles)]
        assert got == R.circles_of(si)


# ---------------------------------------------------------------------------- families
def test_family_sizes_and_contact_cap():
    cases, T = R.cases(), R.truth()
    count = {}
    for c in cases:
        count[c.family] = count.get(c.family, 0) + 1
    assert max(count.values()) <= 64 and len(cases) <= 400, count
    contact = [(c, f, d) for c, f, d in zip(cases, T.flag, T.decided) if c.family == "contact"]
    left_out = sum(not d for _, _, d in contact)
    assert left_out <= 0.1 * len(contact), (left_out, len(contact))
    for c, f, _ in contact:
        assert not c.pre[18:30].any()
        if "/skip/" in c.note:
            assert f is False, c.note            # at the skip's threshold there is no contact
        else:
            assert f == c.note.endswith(("-0.001", "-1e-06", "-1e-09")), (c.note, f)  # delta < 0: contact
    # the pre-step flag of every case is 0, and no other family's case sits on the contact threshold
    assert all(T.decided), [i for i, d in enumerate(T.decided) if not d]


def test_motor_offsets_on_both_sides_of_the_switch():
    """motor_small stays on the series side of the kernel's switch (|d| < 1e-2 after the update),
    motor_large has the threshold itself and its neighbours on the sincos side."""
    def ds(family):
        out = []
        for c in R.cases():
            if c.family == family:
                post, _ = R.step(c.pre, 0.0, 0.0, float, math.sin, math.cos, positions_only=False)
                out += [post[8] - post[2], post[14] - post[2]]
        return out

    small, large = ds("motor_small"), ds("motor_large")
    assert all(abs(d) < 1e-2 for d in small)
    assert float(np.nextafter(1e-2, 0.0)) in small and 0.0 in small
    assert {1e-2, float(np.nextafter(1e-2, 1.0)), -0.010000001} <= set(large)


# ---------------------------------------------------------------------------- 2. the oracle
def _oracle_posts(oracle_mod, scenarios_c, ref_cfg, exact):
    lib = oracle_mod.load(exact)
    posts, flags = [], []
    for c in R.cases():
        fL, fR = R.thrust(c.act)
        st = np.array(c.pre, dtype=np.float64)
        hit = lib.d2dcpu_physics_step(C.byref(ref_cfg), C.byref(scenarios_c[c.scn]), C.c_void_p(st.ctypes.data),
                                      fL, fR, 0)
        posts.append(None if c.flag_only else st[:R.NPHYS].copy())
        flags.append(bool(hit))
    return posts, flags


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
def test_oracle_within_bound(oracle_mod, scenarios_c, ref_cfg, exact):
    cases, T, floors = R.cases(), R.truth(), R.floors()
    posts, flags = _oracle_posts(oracle_mod, scenarios_c, ref_cfg, exact)
    errs = R.family_errors(cases, posts, T.post, T.num)
    assert set(errs) == set(floors)
    print(R.describe(errs, floors))
    assert not R.violations(errs, floors)
    wrong = [i for i, c in enumerate(cases) if T.decided[i] and flags[i] != T.flag[i]]
    assert not wrong, [getattr(cases[i], "note", cases[i].family) for i in wrong]


# ---------------------------------------------------------------------------- 3. mutants
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_exceeds_bound(mutant):
    cases, T, floors = R.cases(), R.truth(), R.floors()
    errs = R.family_errors(cases, R.unfused(mutant=mutant)[0], T.post, T.num)
    assert R.violations(errs, floors), mutant


def test_kernel_series_within_bound():
    """The right step with the motors' sin / cos from the kernel's addition formula and series."""
    cases, T, floors = R.cases(), R.truth(), R.floors()
    errs = R.family_errors(cases, R.unfused(motor_series=True)[0], T.post, T.num)
    assert not R.violations(errs, floors)


def test_measure_and_bound():
    num = R.mp_number()
    t = [num.N(0.5)] * R.NPHYS
    x = [0.5] * R.NPHYS
    assert set(R.group_errors(x, t, num).values()) == {0.0}
    x[3] = 0.5 + 2.0 ** -30
    e = R.group_errors(x, t, num)
    assert e["vel"] == 2.0 ** -30 and e["pos"] == 0.0       # |truth| < 1: absolute
    t[4] = num.N(4.0)
    assert R.group_errors(x, t, num)["vel"] == 3.5 / 4.0     # relative to the group's largest |truth|
    x[5] = math.nan
    assert R.group_errors(x, t, num)["w"] == math.inf
    assert R.bound(0.0) == 8 * 2.0 ** -52 and R.bound(1e-12) == 8e-12
    assert R.violations({"f": {"pos": math.inf}}, {"f": {"pos": 1.0}})
