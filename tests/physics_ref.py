"""One ``cpSpaceStep(1/60)`` of the drone rig written once over a number type, the error measure and
the bound for the physics-step tests (tests/test_physics_reference.py, tests/test_gpu_physics_reference.py),
the case families they run, and mutants that show the bound can tell a wrong step from a right one.

Test infrastructure: nothing here calls the HIP library or the C oracle.

``step`` restates Chipmunk2D 7's step for exactly the configuration Drone.py builds (3 dynamic bodies,
6 pivots in ``space.add`` order, ``error_bias = 0``, warm start with ``dt_coef = 1``, 10 sweeps, gravity
(0, -1000), damping 1, thrust at local (-+40, 0)), one operation at a time and in the order
``tests/golden/ref_shims.py``'s ``Space.step`` performs them: nothing is fused, ``jAcc`` is applied as
the round-trip difference ``jAcc_new - jAcc_old`` and the ``+ 0.0`` terms stay.  Two instantiations:

* ``N = float`` with ``math.sin`` / ``math.cos`` (not NumPy's, which may dispatch to other routines), the
  *unfused float64* restatement; it equals the golden vectors' physics columns bit for bit (asserted by
  the CPU tests);
* ``mp_number()``: ``mpmath`` at 50 digits, the *truth* for the same float64 inputs (state, thrust, and
  the double constants dt, masses, box sizes and anchors the C library is handed).

Error measure, per case and column group: ``max_i |x_i - truth_i| / max(1, max_i |truth_i|)`` with the
difference taken in mpmath; a NaN gives infinity; a family's error is the maximum over its cases.
Bound: ``FACTOR`` = 8 times the unfused restatement's error on the same family and group, where an error
below one float64 epsilon counts as one epsilon (tests/ppo_ref.py's convention: the factor is for a few
ulp of difference in trig, division and contraction; the floor is for a group the restatement happens to
round exactly).  The code under test never sets its own bound.

Families (``cases``; each homogeneous, so that a hard case does not set the floor for an easy one; at most
64 cases each and 400 in all): ``golden/<scenario>`` (every 5th row of crafted.npz, one family per
scenario), ``motor_small`` / ``motor_large`` (motor angle offsets d on either side of the kernel's switch
between the series and sincos at |d| = 1e-2), ``big_angle`` (unwrapped angles up to 1e6 + 0.25: argument
reduction), ``thrust`` (the float32 action mapping's corners), ``strained`` (displaced motors, large
jAcc, speeds and spins), ``rest`` (the first step after a reset) and ``contact`` (contact flag only:
box-to-circle distances r + delta down to 1e-9, and centre offsets at frame_hits' skip threshold)."""
from __future__ import annotations

import math
import os
import types

import numpy as np

NPHYS = 30                      # state columns 0..29; 30 (path_error) and 31 (total_reward) are not physics
GROUPS = {
    "pos": [0, 1, 6, 7, 12, 13],
    "ang": [2, 8, 14],
    "vel": [3, 4, 9, 10, 15, 16],
    "w": [5, 11, 17],
    "j": list(range(18, 30)),
}
FACTOR = 8.0
EPS64 = 2.0 ** -52
MUTANTS = ("det_inv", "nine_sweeps", "right_first", "bias_pre_update", "motor_trig_from_frame")
FORCE_SCALE = 1000              # drone_2d_env.py:150

# Drone(x, y, angle, height 20, width 100, masses 0.2 / 0.4 / 0.4): frame box (100, 10), motor boxes (20, 20)
_MASS = (0.2, 0.4, 0.4)
_BOX = ((100.0, 10.0), (20.0, 20.0), (20.0, 20.0))
FRAME_HX, FRAME_HY = 50.0, 5.0
DRONE_R = 40.0                  # width / 2 - height / 2
# pivots in space.add order: (motor body, anchor x on the motor, anchor x on the frame); anchor y = 0
_JOINTS = ((1, -7.0, -47.0), (1, 0.0, -40.0), (1, 7.0, -33.0), (2, -7.0, 33.0), (2, 0.0, 40.0), (2, 7.0, 47.0))


# ------------------------------------------------------------------------------------ number types
def mp_number(dps: int = 50):
    """An mpmath context of its own (the global ``mpmath.mp`` keeps its precision)."""
    import mpmath

    ctx = mpmath.mp.clone()
    ctx.dps = dps
    return types.SimpleNamespace(N=ctx.mpf, sin=ctx.sin, cos=ctx.cos, ctx=ctx)


def thrust(act):
    """drone_2d_env.py:400-401 on SB3's float32 action: ``(a / 2 + 0.5) * force_scale`` stays float32."""
    a = np.asarray(act, dtype=np.float32)
    f = (a / np.float32(2) + np.float32(0.5)) * np.float32(FORCE_SCALE)
    assert f.dtype == np.float32
    return float(f[0]), float(f[1])


# ------------------------------------------------------------------------------------ the step
def _moment_box(N, mass, size):
    # cpMomentForPoly over cpBoxShapeNew2's vertices (r,b), (r,t), (l,t), (l,b), offset 0
    hw, hh = N(size[0]) / N(2.0), N(size[1]) / N(2.0)
    v = [(hw, -hh), (hw, hh), (-hw, hh), (-hw, -hh)]
    s1 = s2 = N(0.0)
    for i in range(4):
        v1x, v1y = v[i][0] + N(0.0), v[i][1] + N(0.0)
        v2x, v2y = v[(i + 1) % 4][0] + N(0.0), v[(i + 1) % 4][1] + N(0.0)
        a = v2x * v1y - v2y * v1x
        b = (v1x * v1x + v1y * v1y) + (v1x * v2x + v1y * v2y) + (v2x * v2x + v2y * v2y)
        s1 = s1 + a * b
        s2 = s2 + a
    return (N(mass) * s1) / (N(6.0) * s2)


class _Body:
    __slots__ = ("px", "py", "a", "vx", "vy", "w", "c", "s", "fx", "fy", "t", "m_inv", "i_inv")


def _tvect(c, s, vx, vy):
    return c * vx + (-s) * vy, s * vx + c * vy


def _tpoint(N, c, s, px, py, vx, vy):
    tx = px - (N(0.0) * c - N(0.0) * s)
    ty = py - (N(0.0) * s + N(0.0) * c)
    return c * vx + (-s) * vy + tx, s * vx + c * vy + ty


def _apply(b, jx, jy, rx, ry):
    b.vx = b.vx + jx * b.m_inv
    b.vy = b.vy + jy * b.m_inv
    b.w = b.w + b.i_inv * (rx * jy - ry * jx)


def _kernel_series(N, c0, s0, d):
    """sin / cos(frame + d) by the addition formula with d's series (csrc/d2d_device.h, |d| < 1e-2),
    every operation separate."""
    d2 = d * d
    sd = d * (d2 * (d2 * (d2 * (N(-1.0) / N(5040.0)) + N(1.0) / N(120.0)) + N(-1.0) / N(6.0)) + N(1.0))
    cdm1 = d2 * (d2 * (d2 * (d2 * (N(1.0) / N(40320.0)) + N(-1.0) / N(720.0)) + N(1.0) / N(24.0)) + N(-0.5))
    return s0 * cdm1 + (c0 * sd + s0), c0 * cdm1 + ((-s0) * sd + c0)


def step(state32, fL, fR, N, sin, cos, mutant=None, motor_series=False, positions_only=False):
    """One step from the float64 state ``state32`` (columns 0..29 are read) with thrusts ``fL``, ``fR``.

    Returns ``(post, pose)``: the 30 physics columns as ``N`` values and the frame's post-update pose
    ``(px, py, cos, sin)`` the contact test runs on.  ``mutant`` switches one error on (``MUTANTS``);
    ``motor_series`` takes the motors' sin / cos by the kernel's series where ``|d| < 1e-2``;
    ``positions_only`` stops after the position update (``post`` is then None)."""
    assert mutant is None or mutant in MUTANTS, mutant
    zero, one = N(0.0), N(1.0)
    dt = N(1.0 / 60)
    B = []
    for bi in range(3):
        b = _Body()
        b.px, b.py, b.a, b.vx, b.vy, b.w = (N(float(state32[6 * bi + q])) for q in range(6))
        b.c, b.s = cos(b.a), sin(b.a)
        b.fx = b.fy = b.t = zero
        b.m_inv = one / N(_MASS[bi])
        b.i_inv = one / _moment_box(N, _MASS[bi], _BOX[bi])
        B.append(b)
    jacc = [[N(float(state32[18 + 2 * k])), N(float(state32[19 + 2 * k]))] for k in range(6)]
    F = B[0]
    # drone_2d_env.py:403-404: cpBodyApplyForceAtLocalPoint((0, f), (-+40, 0)) on the frame, left then right
    for f, lx in ((N(float(fL)), N(-DRONE_R)), (N(float(fR)), N(DRONE_R))):
        fwx, fwy = _tvect(F.c, F.s, zero, f)
        wpx, wpy = _tpoint(N, F.c, F.s, F.px, F.py, lx, zero)
        cgx, cgy = _tpoint(N, F.c, F.s, F.px, F.py, zero, zero)
        F.fx = F.fx + fwx
        F.fy = F.fy + fwy
        rx, ry = wpx - cgx, wpy - cgy
        F.t = F.t + (rx * fwy - ry * fwx)
    pre_pos = [(b.px, b.py) for b in B]
    # cpBodyUpdatePosition (v_bias = w_bias = 0), cpBodySetAngle
    for b in B:
        b.px = b.px + (b.vx + zero) * dt
        b.py = b.py + (b.vy + zero) * dt
        b.a = b.a + (b.w + zero) * dt
        b.c, b.s = cos(b.a), sin(b.a)
    for b in B[1:]:
        d = b.a - F.a
        if mutant == "motor_trig_from_frame" and abs(d) < 1e-6:
            b.c, b.s = F.c, F.s
        elif motor_series and abs(d) < 1e-2:
            b.s, b.c = _kernel_series(N, F.c, F.s, d)
    pose = (F.px, F.py, F.c, F.s)
    if positions_only:
        return None, pose
    # PivotJoint preStep
    order = (3, 4, 5, 0, 1, 2) if mutant == "right_first" else (0, 1, 2, 3, 4, 5)
    J = {}
    for k in order:
        m, ax, bx = _JOINTS[k]
        a, b = B[m], F
        r1x, r1y = _tvect(a.c, a.s, N(ax) - zero, zero - zero)
        r2x, r2y = _tvect(b.c, b.s, N(bx) - zero, zero - zero)
        m_sum = a.m_inv + b.m_inv
        k11, k12, k21, k22 = m_sum, zero, zero, m_sum
        r1xsq = r1x * r1x * a.i_inv
        r1ysq = r1y * r1y * a.i_inv
        r1nxy = -r1x * r1y * a.i_inv
        k11 = k11 + r1ysq
        k12 = k12 + r1nxy
        k21 = k21 + r1nxy
        k22 = k22 + r1xsq
        r2xsq = r2x * r2x * b.i_inv
        r2ysq = r2y * r2y * b.i_inv
        r2nxy = -r2x * r2y * b.i_inv
        k11 = k11 + r2ysq
        k12 = k12 + r2nxy
        k21 = k21 + r2nxy
        k22 = k22 + r2xsq
        det = k11 * k22 - k12 * k21
        det_inv = one / det
        if mutant == "det_inv":
            det_inv = det_inv * N(1.0 + 1e-10)
        kinv = (k22 * det_inv, -k12 * det_inv, -k21 * det_inv, k11 * det_inv)
        if mutant == "bias_pre_update":
            (apx, apy), (bpx, bpy) = pre_pos[m], pre_pos[0]
        else:
            apx, apy, bpx, bpy = a.px, a.py, b.px, b.py
        dx = (bpx + r2x) - (apx + r1x)
        dy = (bpy + r2y) - (apy + r1y)
        coef = -(one - zero) / dt   # bias_coef = 1 - error_bias ** dt with error_bias = 0
        J[k] = (a, r1x, r1y, r2x, r2y, kinv, dx * coef, dy * coef)
    # cpBodyUpdateVelocity: gravity (0, -1000), damping ** dt = 1
    damping = one
    for b in B:
        b.vx = b.vx * damping + (zero + b.fx * b.m_inv) * dt
        b.vy = b.vy * damping + (N(-1000.0) + b.fy * b.m_inv) * dt
        b.w = b.w * damping + b.t * b.i_inv * dt
    # applyCachedImpulse, dt_coef = 1
    for k in order:
        a, r1x, r1y, r2x, r2y = J[k][:5]
        jx, jy = jacc[k][0] * one, jacc[k][1] * one
        _apply(a, -jx, -jy, r1x, r1y)
        _apply(F, jx, jy, r2x, r2y)
    # applyImpulse, Space.iterations = 10
    for _ in range(9 if mutant == "nine_sweeps" else 10):
        for k in order:
            a, r1x, r1y, r2x, r2y, (ka, kb, kc, kd), bx, by = J[k]
            v1x = a.vx + (-r1y) * a.w
            v1y = a.vy + r1x * a.w
            v2x = F.vx + (-r2y) * F.w
            v2y = F.vy + r2x * F.w
            vrx = v2x - v1x
            vry = v2y - v1y
            ux = bx - vrx
            uy = by - vry
            jx = ux * ka + uy * kb
            jy = ux * kc + uy * kd
            ox, oy = jacc[k]
            jacc[k] = [ox + jx, oy + jy]   # the clamp to max_force * dt = inf is the identity
            jx, jy = jacc[k][0] - ox, jacc[k][1] - oy
            _apply(a, -jx, -jy, r1x, r1y)
            _apply(F, jx, jy, r2x, r2y)
    post = []
    for b in B:
        post += [b.px, b.py, b.a, b.vx, b.vy, b.w]
    for k in range(6):
        post += jacc[k]
    return post, pose


def contact_margin(pose, circle, N):
    """``dist^2 - r^2`` of the frame box (+-50, +-5) at ``pose`` to the circle's centre, in the operation
    order of ref_shims' ``Space._box_circle_touch``; contact iff it is <= 0."""
    px, py, c, s = pose
    cx, cy, r = (N(float(v)) for v in circle)
    hx, hy = N(FRAME_HX), N(FRAME_HY)
    dx = cx - px
    dy = cy - py
    lx = dx * c + dy * s
    ly = -dx * s + dy * c
    qx = min(max(lx, -hx), hx)
    qy = min(max(ly, -hy), hy)
    ex = lx - qx
    ey = ly - qy
    return (ex * ex + ey * ey) - r * r, r * r


def touches(pose, circles, N) -> bool:
    return any(contact_margin(pose, c, N)[0] <= 0 for c in circles)


# ------------------------------------------------------------------------------------ error, bound
def group_errors(x, truth, num) -> dict:
    """{group: max_i |x_i - truth_i| / max(1, max_i |truth_i|)} of one case; ``x`` are floats (or ``N``
    values), ``truth`` the mpmath step's values; the difference is taken in mpmath; a NaN gives inf."""
    out = {}
    for g, cols in GROUPS.items():
        scale = max(num.N(1.0), max(abs(truth[c]) for c in cols))
        worst = 0.0
        for c in cols:
            xc = x[c]
            if isinstance(xc, (float, np.floating)) and not math.isfinite(xc):
                worst = math.inf
                break
            worst = max(worst, float(abs(num.N(xc) - truth[c]) / scale))
        out[g] = worst
    return out


def family_errors(cases, posts, truths, num) -> dict:
    """{family: {group: max over the family's cases}} for per-case results ``posts`` (None: not run)."""
    out = {}
    for case, x, t in zip(cases, posts, truths):
        if x is None or t is None:
            continue
        e = group_errors(x, t, num)
        f = out.setdefault(case.family, dict.fromkeys(GROUPS, 0.0))
        for g in GROUPS:
            f[g] = max(f[g], e[g])
    return out


def bound(floor_err: float) -> float:
    """The allowance given the unfused restatement's error on the same family and group."""
    return FACTOR * max(floor_err, EPS64)


def violations(errs: dict, floors: dict) -> list:
    """[(family, group, error, bound)] where ``errs`` exceeds ``bound(floors)``."""
    return [(f, g, e, bound(floors[f][g])) for f, ge in errs.items() for g, e in ge.items()
            if not e <= bound(floors[f][g])]


def describe(errs: dict, floors: dict) -> str:
    """One line per family: ``group error/floor`` (what the tests print before they assert)."""
    return "\n".join(f"{f:22s} " + "  ".join(f"{g} {e:.2e}/{floors[f][g]:.2e}" for g, e in ge.items())
                     for f, ge in errs.items())


# ------------------------------------------------------------------------------------ case families
SCENARIOS = ["perpendicular", "parallel", "S_parallel", "corridor", "S_corridor", "large", "impossible"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONTACT_DELTAS = (1e-3, -1e-3, 1e-6, -1e-6, 1e-9, -1e-9)
SKIP_REACH = 51.25              # frame_hits' wave-uniform skip: |offset| >= r + 51.25 on an axis


class Case(types.SimpleNamespace):
    """family, scn (index into SCENARIOS), pre (float64[32]), act (float32[2]); contact cases: physics
    columns are not compared (``flag_only``)."""


def rig(x, y, th, vx=0.0, vy=0.0, w=0.0, dL=0.0, dR=0.0, off=((0.0, 0.0), (0.0, 0.0)), dv=None, jacc=None):
    """A state with the motors at the rigid offsets -+40 along the body axis (plus ``off`` px), motor
    angles ``th + d``, rigid-body motor velocities (plus ``dv`` rows of (vx, vy, w)) and ``jacc``."""
    s = np.zeros(32)
    s[0:6] = [x, y, th, vx, vy, w]
    for bi, sign, d in ((1, -1.0, dL), (2, 1.0, dR)):
        rx, ry = sign * 40.0 * math.cos(th), sign * 40.0 * math.sin(th)
        ox, oy = off[bi - 1]
        s[6 * bi:6 * bi + 6] = [x + rx + ox, y + ry + oy, th + d, vx - ry * w, vy + rx * w, w]
        if dv is not None:
            s[6 * bi + 3:6 * bi + 6] += dv[bi - 1]
    if jacc is not None:
        s[18:30] = jacc
    return s


def _golden_cases():
    g = np.load(os.path.join(GOLDEN, "crafted.npz"), allow_pickle=False)
    return [Case(family="golden/" + SCENARIOS[int(g["scn"][k])], scn=int(g["scn"][k]), pre=g["pre"][k].copy(),
                 act=g["act"][k].copy(), flag_only=False) for k in range(0, len(g["rew"]), 5)]


def _circles(name):
    return np.load(os.path.join(GOLDEN, "scenarios.npz"), allow_pickle=False)[f"{name}/circles"]


def pad_state():
    """A rig at rest out of every circle's reach in every test scenario (no lane of a wave of these has
    a circle to test)."""
    return rig(-3000.0, -3000.0, 0.0)


def _contact_cases():
    """Frame poses whose post-update box-to-circle distance is r + delta, nearest feature a face, an
    edge end or a corner -- also a corner pointing at the circle along the x axis, where the centre
    offset on that axis is r + 50.249 + delta: the farthest offset with a contact, which frame_hits'
    skip must not cut off; and poses whose centre offset on one axis is within 1e-9 of the skip's reach."""
    num = mp_number()
    N, ctx = num.N, num.ctx
    dt = 1.0 / 60
    cases = []
    for name in ("large", "corridor"):
        circ = _circles(name)
        scn = SCENARIOS.index(name)
        # the circle to approach and the direction (seen from it) the frame comes from: no other circle
        # is near there, whatever the frame's orientation (every point of the box is within 50.25 of
        # its centre, which stays within 10 of the probe point)
        ci, phi0 = {"large": (0, 2.2), "corridor": (0, math.pi)}[name]
        cx, cy, r = (float(v) for v in circ[ci])
        probe = (cx + (r + 55.0) * math.cos(phi0), cy + (r + 55.0) * math.sin(phi0))
        clear = min([math.hypot(probe[0] - ox, probe[1] - oy) - orr for oi, (ox, oy, orr) in enumerate(circ)
                     if oi != ci], default=math.inf)
        assert clear > 100.0, (name, clear)
        k = 0
        for feature in ("face", "edge_end", "corner", "corner_on_axis"):
            for delta in CONTACT_DELTAS:
                # the circle's centre in the frame's coordinates, at distance r + delta from the box
                if feature == "face":
                    lx, ly = N(12.5 * (k % 3 - 1)), -(N(5.0) + N(r) + N(delta))
                elif feature == "edge_end":
                    lx, ly = -(N(50.0) + N(r) + N(delta)), N(4.999)
                elif feature == "corner":
                    q = N(0.7 + 0.1 * (k % 3))
                    lx = -(N(50.0) + (N(r) + N(delta)) * ctx.cos(q))
                    ly = -(N(5.0) + (N(r) + N(delta)) * ctx.sin(q))
                else:   # on the box's diagonal through the corner (-50, -5)
                    diag = ctx.sqrt(N(50.0) * N(50.0) + N(5.0) * N(5.0))
                    lx = -(N(50.0) + (N(r) + N(delta)) * N(50.0) / diag)
                    ly = -(N(5.0) + (N(r) + N(delta)) * N(5.0) / diag)
                # the orientation that puts the frame in direction phi of the circle: p - c = -R(th) l
                phi = math.pi if feature == "corner_on_axis" else phi0 + 0.05 * (k % 3 - 1)
                th = phi - math.atan2(-float(ly), -float(lx))
                vx, vy, w = 35.0 * (k % 5 - 2), -20.0 * (k % 3 - 1), 0.0
                c, s = ctx.cos(N(th)), ctx.sin(N(th))
                px = float(N(cx) - (c * lx - s * ly))
                py = float(N(cy) - (s * lx + c * ly))
                pre = rig(px - vx * dt, py - vy * dt, th, vx, vy, w)
                cases.append(Case(family="contact", scn=scn, pre=pre, act=np.zeros(2, np.float32), flag_only=True,
                                  note=f"{name}/{feature}/{delta:+g}"))
                k += 1
        for axis in (0, 1):
            for eps in (1e-9, -1e-9):
                off = [37.0, -23.0]
                off[axis] = (r + SKIP_REACH + eps) * (1 if axis == 0 else -1)
                pre = rig(cx - off[0], cy - off[1], 0.4 if axis == 0 else -1.1)
                cases.append(Case(family="contact", scn=scn, pre=pre, act=np.zeros(2, np.float32), flag_only=True,
                                  note=f"{name}/skip/axis{axis}/{eps:+g}"))
    return cases


def _series_side(th, s):
    """Where the sum th + d rounded a motor's offset up to 1e-2, the nearest angle below it."""
    for col in (8, 14):
        while abs(s[col] - th) >= 1e-2:
            s[col] = np.nextafter(s[col], th)
    return s


def _synthetic_cases():
    rng = np.random.default_rng(20260)
    cases = []

    def add(family, pre, act=(0.0, 0.0)):
        cases.append(Case(family=family, scn=len(cases) % len(SCENARIOS), pre=np.asarray(pre, np.float64),
                          act=np.asarray(act, np.float32), flag_only=False))

    below = float(np.nextafter(1e-2, 0.0))
    small = [0.0, 1e-12, -1e-12, 1e-7, -1e-7, 3e-5, -3e-5, 1e-3, -1e-3, 5e-3, -5e-3, 9.9e-3, -9.9e-3, below]
    for ti, th in enumerate((0.0, 0.3, -1.2, 2.9)):
        for i, dL in enumerate(small):
            dR = small[(i + 5 + ti) % len(small)]
            # th = 0 with no spin: d = motor angle - frame angle is exactly the listed value after the update
            w = 0.0 if th == 0.0 or below in (dL, dR) else 0.05 * (i % 3 - 1)
            add("motor_small", _series_side(th, rig(400.0 + 30 * i, 900.0 - 20 * ti, th, 3.0 * (i % 4 - 1.5), -2.0 * (i % 3), w, dL, dR,
                                   jacc=rng.normal(0.0, 1.0, 12))), rng.uniform(-1, 1, 2))
    large = [1e-2, float(np.nextafter(1e-2, 1.0)), -0.010000001, 0.02, -0.02, 0.5, -0.5, 3.0, -3.0]
    for ti, th in enumerate((0.0, -1.2)):
        for i, dL in enumerate(large):
            # the other motor sits just on the other side of the switch or well inside it
            dR = (below, -9.9e-3, large[(i + 4) % len(large)])[(i + ti) % 3]
            if i % 2:
                dL, dR = dR, dL
            add("motor_large", rig(500.0 + 25 * i, 700.0 + 40 * ti, th, 2.0 * (i % 3 - 1), 1.5 * (i % 4), 0.0, dL, dR,
                                   jacc=rng.normal(0.0, 1.0, 12)), rng.uniform(-1, 1, 2))
    for i, mag in enumerate((10.0, 1e3, 1e5, 1e6 + 0.25)):
        for sign in (1.0, -1.0):
            for q in range(2):
                dL, dR = ((7e-4, -2e-4), (-9.5e-4, 1e-3))[q]
                add("big_angle", rig(300.0 + 90 * i, 500.0 + 60 * q, sign * mag, 20.0 * (q - 0.5), -15.0, 0.4 * sign * (q + 1),
                                     dL, dR, jacc=rng.normal(0.0, 2.0, 12)), rng.uniform(-1, 1, 2))
    f32 = [np.float32(0.1), np.float32(-1.0 / 3.0), np.float32(0.99999994), np.float32(-0.99999994), np.float32(1e-7)]
    acts = [(a, b) for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)]
    acts += [(f32[i], f32[(i + 2) % 5]) for i in range(5)]
    for i, act in enumerate(acts):
        add("thrust", rig(650.0, 300.0 + 10 * i, 0.6 - 0.1 * (i % 4), 40.0, -60.0, 1.5, 2e-4, -3e-4,
                          jacc=rng.normal(0.0, 3.0, 12)), act)
    for i in range(18):
        px = (0.05, 1.0, 5.0)[i % 3]
        ang = rng.uniform(-math.pi, math.pi, 2)
        off = tuple((px * math.cos(a), px * math.sin(a)) for a in ang)
        sp = (5.0, 120.0, 500.0)[(i // 3) % 3]
        jm = (3.0, 60.0, 300.0)[(i // 6) % 3]
        dv = [np.array([rng.uniform(-1, 1) * 0.02 * sp, rng.uniform(-1, 1) * 0.02 * sp, rng.uniform(-1, 1) * 0.5])
              for _ in range(2)]
        add("strained", rig(rng.uniform(100, 1200), rng.uniform(100, 1200), rng.uniform(-1.7, 1.7),
                            sp * math.cos(i), sp * math.sin(i), (2.0, 12.0, 30.0)[i % 3] * (-1) ** i,
                            rng.normal(0, 0.01), rng.normal(0, 0.01), off, dv, rng.uniform(-1, 1, 12) * jm),
            rng.uniform(-1, 1, 2))
    # the first step after a reset: recorded spawn states (all velocities and jAcc zero), and the padding state
    g = np.load(os.path.join(GOLDEN, "traj.npz"), allow_pickle=False)
    idx = np.nonzero(g["is_reset"] == 1)[0]
    seen = set()
    for k in idx:
        if int(g["scn"][k]) in seen:
            continue
        seen.add(int(g["scn"][k]))
        s = g["reset_state"][k].copy()
        assert np.all(s[[3, 4, 5, 9, 10, 11, 15, 16, 17]] == 0) and np.all(s[18:30] == 0)
        cases.append(Case(family="rest", scn=int(g["scn"][k]), pre=s, act=rng.uniform(-1, 1, 2).astype(np.float32),
                          flag_only=False))
    for th in (0.0, 0.7, -2.0):
        add("rest", rig(200.0, 1100.0, th), rng.uniform(-1, 1, 2))
    cases.append(Case(family="rest", scn=0, pre=pad_state(), act=np.zeros(2, np.float32), flag_only=False, pad=True))
    return cases


_cache = {}


def cases():
    """Every case of every family, in a fixed order (built once per process)."""
    if "cases" not in _cache:
        cs = _golden_cases() + _synthetic_cases() + _contact_cases()
        count = {}
        for c in cs:
            count[c.family] = count.get(c.family, 0) + 1
        assert max(count.values()) <= 64 and len(cs) <= 400, count
        _cache["cases"] = cs
    return _cache["cases"]


def circles_of(scn: int):
    if ("circles", scn) not in _cache:
        _cache["circles", scn] = [tuple(float(v) for v in c) for c in _circles(SCENARIOS[scn])]
    return _cache["circles", scn]


def truth():
    """The mpmath step of every case, once per process: a SimpleNamespace with ``num``; ``post`` (per
    case, None for flag-only cases); ``flag`` (the contact predicate on the post-update pose; the
    pre-step collided flag of every case is 0); ``decided`` (False where |dist^2 - r^2| <= 1e-12 r^2
    for some circle: such a case is left out of flag comparisons)."""
    if "truth" not in _cache:
        num = mp_number()
        post, flag, decided = [], [], []
        for c in cases():
            fL, fR = thrust(c.act)
            p, pose = step(c.pre, fL, fR, num.N, num.sin, num.cos, positions_only=c.flag_only)
            post.append(p)
            margins = [contact_margin(pose, circ, num.N) for circ in circles_of(c.scn)]
            flag.append(any(m <= 0 for m, _ in margins))
            decided.append(all(abs(m) > num.N(1e-12) * rr for m, rr in margins))
        _cache["truth"] = types.SimpleNamespace(num=num, post=post, flag=flag, decided=decided)
    return _cache["truth"]


def unfused(mutant=None, motor_series=False):
    """The float restatement of every case: (posts, flags)."""
    posts, flags = [], []
    for c in cases():
        fL, fR = thrust(c.act)
        p, pose = step(c.pre, fL, fR, float, math.sin, math.cos, mutant=mutant, motor_series=motor_series,
                       positions_only=c.flag_only)
        posts.append(p)
        flags.append(touches(pose, circles_of(c.scn), float))
    return posts, flags


def floors() -> dict:
    """{family: {group: the unfused restatement's error}}: what ``bound`` is taken of."""
    if "floors" not in _cache:
        t = truth()
        _cache["floors"] = family_errors(cases(), unfused()[0], t.post, t.num)
    return _cache["floors"]
