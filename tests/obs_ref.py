"""``get_observation`` and the reward / end conditions of ``step`` written once over a number type, the
error measure and the bound for the observation tests (tests/test_obs_reference.py,
tests/test_gpu_obs_reference.py), the case families they run, and mutants that show the bound can tell a
wrong observation or reward from a right one.

Test infrastructure: nothing here calls the HIP library; the C oracle is called for ``closest_u`` alone (the
closest-point search is a discrete procedure held bit for bit elsewhere; ``u`` is an input here), and for its
``path_eval`` where the case families place a frame relative to a path point.

``observe`` restates drone_2d_env.py:631-771 with transformations.py's ``ssa`` / ``R_w_b`` and
``get_obstacle_distances``; ``reward`` restates :422-578.  One operation at a time, in the reference's
order: ``m1to1`` / ``invm1to1`` round trips, ``obs[17] * pi``, ``(atan2 + 2 pi) % 2 pi``, the row form of
``np.matmul(R_w_b, d)``.  Two instantiations:

* ``float_number()``: Python floats with NumPy's sin / cos / arctan2 (the reference's) -- the *float64 restatement*; it is anchored
  to the golden vectors' ``obs``, ``rew`` and info columns (tests/test_obs_reference.py);
* ``mp_number()``: mpmath at 50 digits -- the *truth* for the same float64 inputs (state, scenario tables,
  configuration, ``u`` and the double constants pi, 11.7, 1330 ...).  mpmath has no signed zero: where both
  arguments of an ``atan2`` are exactly zero the truth takes the IEEE result for the sign bits the float64
  restatement had there (its ``atan2`` calls are recorded on a tape the truth reads in step).

Measure.  The device hands out float32 (obs, reward, info) and two float64 values (state columns 30 and
31).  A float32 value ``o`` passes iff ``RN32(truth - m) <= o <= RN32(truth + m)``: it is the float32
rounding of some number within ``m`` of the truth (one final rounding is what the kernel does, so its half
ulp is derived, not measured).  A float64 value passes iff ``|o - truth| <= m``.
``m = FACTOR * max(floor, EPS64 * max(1, |truth|))`` with ``FACTOR`` = 8 and ``floor`` the float64
restatement's own error against the truth on the same family and output group (``GROUPS``), evaluated at the
same states.  The code under test never sets its bound.

Decisions (which three circles and in which order, LA lock, lookahead clamp, ``d < danger_range``, the
lambda floor, AA band / angle, reach-end, time-up, collision) are compared as decisions.  A case is *decided*
when the truth's margin to every threshold it depends on exceeds ``m`` of the group the quantity decodes
from (an exact tie between two circles' distances is decided: lowest index first).  No case may be undecided.

Routes.  *step*: ``set_state``, one ``step``, ``get_state``: the returned float64 state is what the kernel
observed, so the physics drops out.  *reset*: a scenario whose spawn rectangle is a point (``xmin == xmax``
...) or a shipped scenario's spawn draw; ``reset()`` runs the reset kernel's single-lane ``observe``.
"""
from __future__ import annotations

import math
import os
import types
from fractions import Fraction

import numpy as np

import physics_ref as P

FACTOR = 8.0
EPS64 = 2.0 ** -52
OBS_DIM = 27
# value vector of a case: obs 0..26, then reward, PA, PP, CA, AA, path distance
V_REW, V_PA, V_PP, V_CA, V_AA, V_DIST = 27, 28, 29, 30, 31, 32
GROUPS = {
    "linear": [0, 1, 2, 4, 5, 6, 7],
    "alpha": [3],
    "obst_dist": [8, 11, 14],
    "obst_bear": [9, 10, 12, 13, 15, 16],
    "vel_bear": [17, 18],
    "path_pts": [19, 20, 21, 22],
    "path_bear": [23, 24, 25, 26],
    "reward": [V_REW],
    "terms": [V_PA, V_PP, V_CA, V_AA],
    "path_dist": [V_DIST],
}
GROUP_OF = {i: g for g, idx in GROUPS.items() for i in idx}
SUBTLE = ("rsqrt32", "diag32", "pi32", "la_clamp")
STRUCTURAL = ("rot_verts", "centre_rank", "no_minus_pi", "no_lambda_floor", "lock_not_sticky", "aa_alpha")
MUTANTS = SUBTLE + STRUCTURAL
FLAG_COLLIDED, FLAG_LA_LOCK = 1, 2
END_COLLISION, END_REACH, END_TIMEUP, END_AA = 1, 2, 4, 8
VEL_MAX = 1330.0


# ------------------------------------------------------------------------------------ number types
def _fma(a, b, c):
    """Correctly rounded a * b + c of floats (the conversion of a Fraction to float rounds correctly)."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    r = Fraction(a) * Fraction(b) + Fraction(c)
    if r == 0:
        p = a * b
        return p + c   # the sign of an exact zero: IEEE's sum of the two signed terms
    return float(r)


def _pymod(a, b):
    """Python / NumPy float modulo for b > 0."""
    m = math.fmod(a, b)
    if m != 0.0:
        if m < 0.0:
            m += b
    else:
        m = math.copysign(0.0, b)
    return m


def float_number():
    """Python floats; sin / cos / atan2 are NumPy's, which the reference calls (np.arctan2 is an AVX-512
    routine an ulp from libm's in ~8 % of arguments where the CPU has it -- with ``math.atan2`` only 96 % of
    the golden bearings match bit for bit, with NumPy's all of them; np.sin / np.cos equal libm's)."""
    return types.SimpleNamespace(N=float, sin=lambda v: float(np.sin(v)), cos=lambda v: float(np.cos(v)),
                                 sqrt=math.sqrt, atan2=lambda y, x: float(np.arctan2(y, x)), fma=_fma,
                                 mod=_pymod, pi=math.pi, exact=False)


def mp_number(dps: int = 50):
    num = P.mp_number(dps)
    ctx = num.ctx

    def atan2(y, x, hint=(0.0, 0.0)):
        if y == 0 and x == 0:
            hy, hx = (math.copysign(1.0, float(h)) for h in hint)
            return ctx.mpf(0) if hx > 0 else hy * ctx.pi
        if y == 0 and x < 0:
            return math.copysign(1.0, float(hint[0])) * ctx.pi
        return ctx.atan2(y, x)

    def mod(a, b):
        return a - b * ctx.floor(a / b)

    num.sqrt, num.atan2, num.mod, num.fma, num.exact = ctx.sqrt, atan2, mod, (lambda a, b, c: a * b + c), True
    num.pi = ctx.mpf(math.pi)    # np.pi, the double: the reference's constant is an input like any other
    return num


class _Atan2:
    """atan2 of a number type with the signed-zero tape: the float run records its arguments in call
    order, the truth's run reads them as the signs of its exact zeros."""

    def __init__(self, num, tape):
        self.num, self.tape, self.k = num, tape, 0

    def __call__(self, y, x):
        if not self.num.exact:
            self.tape.append((y, x))
            return self.num.atan2(y, x)
        hint = self.tape[self.k]
        self.k += 1
        return self.num.atan2(y, x, hint)


# ------------------------------------------------------------------------------------ scenario view
def scn_view(c):
    """The fields of a D2DScn as Python floats."""
    n, nc = int(c.n_wps), int(c.n_circles)
    return types.SimpleNamespace(
        n_wps=n, n_circles=nc, us=[float(c.us[i]) for i in range(n)],
        xa=[float(v) for v in c.xa[:n - 2]], xb=[float(v) for v in c.xb[:n - 2]], xc=[float(v) for v in c.xc[:n - 2]],
        ya=[float(v) for v in c.ya[:n - 2]], yb=[float(v) for v in c.yb[:n - 2]], yc=[float(v) for v in c.yc[:n - 2]],
        cx=[float(v) for v in c.cx[:nc]], cy=[float(v) for v in c.cy[:nc]], cr=[float(v) for v in c.cr[:nc]],
        wlx=float(c.wp_last_x), wly=float(c.wp_last_y))


def _u_index(S, u):
    n = 0
    while n < S.n_wps - 1:
        if u <= S.us[n + 1]:
            break
        n += 1
    return n


def path_eval(S, u, N, un=None):
    """QPMI2D.__call__ (predef_path.py:88-142) at the float ``u``; the branch is taken on the float.
    ``un``: the value the quadratics are evaluated at, where it is not N(u) (the truth's exact
    ``u + lookahead``: the float sum's rounding, half an ulp of u, is part of the restatement's error)."""
    us, nw = S.us, S.n_wps
    nseg = nw - 2
    un = N(u) if un is None else un

    def quad(k):
        return (N(S.xa[k]) * un ** 2 + N(S.xb[k]) * un + N(S.xc[k]),
                N(S.ya[k]) * un ** 2 + N(S.yb[k]) * un + N(S.yc[k]))

    if us[0] <= u <= us[1]:
        return quad(0)
    if (us[nw - 2] - 0.001 <= u <= us[nw - 1]) or _u_index(S, u) == nw - 1:
        return quad(nseg - 1)
    n = _u_index(S, u)
    den = N(us[n + 1]) - N(us[n])
    mu_r = (un - N(us[n])) / den
    mu_f = (N(us[n + 1]) - un) / den
    x1, y1 = quad(n - 1 if n >= 1 else n - 1 + nseg)
    x2, y2 = quad(n)
    return mu_r * x2 + mu_f * x1, mu_r * y2 + mu_f * y1


# ------------------------------------------------------------------------------------ observe, reward
def _clip(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def _f32(x):
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def observe(st, S, cfg, flags, u, num, tape, mutant=None):
    """obs[27] as ``num.N`` values, the new flags, and the decisions [(name, outcome, margin, group)] with
    the margin in units of the group's observation entries (None: an exact tie, decided by index)."""
    assert mutant is None or mutant in MUTANTS, mutant
    N, sin, cos, sqrt = num.N, num.sin, num.cos, num.sqrt
    at2 = _Atan2(num, tape)
    PI, TWO_PI = num.pi, N(2.0) * num.pi
    W, H = N(float(cfg.screen_w)), N(float(cfg.screen_h))
    zero, one, two = N(0.0), N(1.0), N(2.0)
    x, y, al, vx, vy, w = (N(float(st[i])) for i in range(6))
    dec = []

    def m1to1(v, lo, hi):
        return two * (v - lo) / (hi - lo) - one

    def ssa(a):
        return num.mod(a + PI, TWO_PI) - PI

    def unit32(dy, dx, sa, ca):
        # the rsqrt32 mutant: the rotated unit vector through a float32 reciprocal square root
        ir = N(_f32(1.0 / math.sqrt(float(dy) * float(dy) + float(dx) * float(dx))))
        ux, uy = dx * ir, dy * ir
        return uy * ca - ux * sa, ux * ca + uy * sa

    obs = [zero] * OBS_DIM
    vmax = N(VEL_MAX)
    obs[0] = m1to1(vx, -vmax, vmax)
    obs[1] = m1to1(vy, -vmax, vmax)
    obs[2] = _clip(w / N(11.7), -one, one)
    obs[3] = al / PI
    wlx, wly = N(S.wlx), N(S.wly)
    obs[4] = m1to1(wlx - x, zero, W)
    obs[5] = m1to1(wly - y, zero, H)
    obs[6] = m1to1(x, zero, W)
    obs[7] = m1to1(y, zero, H)
    for j in range(3):
        obs[8 + 3 * j], obs[9 + 3 * j], obs[10 + 3 * j] = one, zero, zero
    sal, cal = sin(al), cos(al)
    if S.n_circles > 0:
        verts = [(50.0, -5.0), (50.0, 5.0), (-50.0, 5.0), (-50.0, -5.0)]
        dist = []
        for i in range(S.n_circles):
            cx, cy, cr = N(S.cx[i]), N(S.cy[i]), N(S.cr[i])
            dmin = None
            for bx, by in verts:
                if mutant == "rot_verts":
                    bx, by = cal * N(bx) - sal * N(by), sal * N(bx) + cal * N(by)
                ex, ey = (N(bx) + x) - cx, (N(by) + y) - cy
                d = sqrt(ex ** 2 + ey ** 2) - cr   # Vec2d.get_distance: ** 2 is libm's pow on floats
                if dmin is None or d < dmin:
                    dmin = d
            dist.append(dmin)
        key = dist
        if mutant == "centre_rank":
            key = [sqrt((x - N(S.cx[i])) * (x - N(S.cx[i])) + (y - N(S.cy[i])) * (y - N(S.cy[i]))) for i in range(S.n_circles)]
        order = sorted(range(S.n_circles), key=lambda i: key[i])   # stable: equal keys keep index order
        kk = min(3, S.n_circles)
        diag = sqrt(W * W + H * H)
        if mutant == "diag32":
            diag = N(_f32(diag))
        for r in range(min(kk, S.n_circles - 1)):   # ranks r / r + 1, the last one against the first left out
            gap = dist[order[r + 1]] - dist[order[r]]
            dec.append(("rank%d%d" % (r + 1, r + 2), (order[r], order[r + 1]),
                        None if gap == 0 else two * gap / diag, "obst_dist"))
        for j in range(kk):
            i = order[j]
            obs[8 + 3 * j] = m1to1(dist[i], zero, diag)
            dy, dx = y - N(S.cy[i]), x - N(S.cx[i])
            if mutant == "rsqrt32" and (float(dy) != 0.0 or float(dx) != 0.0):
                s_, c_ = unit32(dy, dx, sal, cal)
                obs[9 + 3 * j], obs[10 + 3 * j] = -s_, -c_
                continue
            ang = at2(dy, dx)
            ang = ssa(ang - al - (zero if mutant == "no_minus_pi" else PI))
            obs[9 + 3 * j], obs[10 + 3 * j] = sin(ang), cos(ang)
    if mutant == "rsqrt32" and (float(vy) != 0.0 or float(vx) != 0.0):
        obs[17], obs[18] = unit32(vy, vx, sal, cal)
    else:
        vab = ssa(at2(vy, vx) - al)
        obs[17], obs[18] = sin(vab), cos(vab)
    cpx, cpy = path_eval(S, u, N)
    obs[19] = m1to1(cpx, zero, W)
    obs[20] = m1to1(cpy, zero, H)
    L = S.us[S.n_wps - 1]
    look = N(float(cfg.lookahead))
    Lc = N(L) - N(1e-4) if mutant == "la_clamp" else N(L)
    over = N(u) + look - Lc
    dec.append(("la_clamp", bool(over > 0), abs(over) / max(one, abs(Lc)), None))
    if over > 0:
        ula = float(Lc) if mutant == "la_clamp" else L
    else:
        ula = u + float(cfg.lookahead)   # the reference's float sum; its rounding is the search's to carry
    lax, lay = path_eval(S, ula, N, N(u) + look if (num.exact and not over > 0) else None)
    ten = N(10.0)
    ax_, ay_ = abs(lax - wlx), abs(lay - wly)
    near = ax_ < ten and ay_ < ten
    # the condition flips when the nearer-to-10 of the deciding axes crosses
    if near:
        marg = min(ten - ax_, ten - ay_)
    else:
        marg = max(ax_ - ten if ax_ >= ten else zero, ay_ - ten if ay_ >= ten else zero)
    dec.append(("la_near", bool(near), two * marg / W, "path_pts"))
    if mutant == "lock_not_sticky":
        flags &= ~FLAG_LA_LOCK
    if near:
        flags |= FLAG_LA_LOCK
    if flags & FLAG_LA_LOCK:
        lax, lay = wlx, wly
    obs[21] = m1to1(lax, zero, W)
    obs[22] = m1to1(lay, zero, H)
    for k, (px_, py_) in ((23, (lax, lay)), (25, (cpx, cpy))):
        dx, dy = px_ - x, py_ - y
        if mutant == "rsqrt32" and (float(dy) != 0.0 or float(dx) != 0.0):
            obs[k], obs[k + 1] = unit32(dy, dx, zero, one)
            continue
        bx = num.fma(cal, dx, (-sal) * dy)
        by = num.fma(sal, dx, cal * dy)
        a = ssa(at2(by, bx) - al)
        obs[k], obs[k + 1] = sin(a), cos(a)
    return obs, flags, dec


def reward(obs, S, cfg, collided, t, num, tape, mutant=None):
    """(values [reward, PA, PP, CA, AA, path distance], end cause bits, decisions) from ``obs``."""
    N, sin, cos, sqrt = num.N, num.sin, num.cos, num.sqrt
    at2 = _Atan2(num, tape)
    PI, TWO_PI = num.pi, N(2.0) * num.pi
    W, H = N(float(cfg.screen_w)), N(float(cfg.screen_h))
    zero, one, two = N(0.0), N(1.0), N(2.0)
    dec = []

    def inv(v, lo, hi):
        return (v + one) * (hi - lo) / two + lo

    def ang(s, c):
        return num.mod(at2(s, c) + TWO_PI, TWO_PI)

    vmax = N(VEL_MAX)
    vxd, vyd = inv(obs[0], -vmax, vmax), inv(obs[1], -vmax, vmax)
    alpha = obs[3] * (N(_f32(math.pi)) if mutant == "pi32" else PI)
    tdx, tdy = inv(obs[4], zero, W), inv(obs[5], zero, H)
    pxd, pyd = inv(obs[6], zero, W), inv(obs[7], zero, H)
    vel_ang = ang(obs[17] * PI, obs[18] * PI)
    cpx, cpy = inv(obs[19], zero, W), inv(obs[20], zero, H)
    la_ang = ang(obs[23], obs[24])
    lpa, lca, ca = one, one, zero
    if S.n_circles > 0:
        diag = sqrt(W * W + H * H)
        if mutant == "diag32":
            diag = N(_f32(diag))
        d = inv(obs[8], zero, diag)
        oa = ang(obs[9], obs[10])
        adiff = abs((num.mod(oa - vel_ang + PI, TWO_PI) - PI) * (N(180.0) / PI))
        Rr, A, k = N(float(cfg.danger_range)), N(float(cfg.danger_angle)), N(float(cfg.abs_inv_ca_min_rew))
        dec.append(("danger", bool(d < Rr), two * abs(d - Rr) / diag, "obst_dist"))
        if d < Rr and cfg.use_lambda:
            lpa = (d / Rr) / two
            fl = N(0.10)
            dec.append(("lambda_floor", bool(lpa < fl), two * abs(lpa - fl) * two * Rr / diag, "obst_dist"))
            if lpa < fl and mutant != "no_lambda_floor":
                lpa = fl
            lca = one - lpa
        if d < Rr:
            rr = -(((Rr + k * Rr) / (d + k * Rr)) - one)
            ar = -(((A + k * A) / (adiff + k * A)) - one)
            if ar > 0:
                ar = zero
            if rr > 0:
                rr = zero
            ca = rr + ar
    ex, ey = cpx - pxd, cpy - pyd
    dist = sqrt(num.fma(ey, ey, ex * ex))
    edge = N(float(cfg.pa_band_edge))
    pa = -(two * (_clip(dist, zero, edge) / edge) - one) * N(float(cfg.pa_scale))
    vel = sqrt(vxd ** 2 + vyd ** 2)
    sv = vel * N(float(cfg.pp_vel_scale))
    vla = abs(num.mod(la_ang - vel_ang + PI, TWO_PI) - PI)
    pp = _clip(cos(vla) * sv, N(float(cfg.pp_rew_min)), N(float(cfg.pp_rew_max)))
    coll, cause = zero, 0
    if collided:
        coll = N(float(cfg.rew_collision))
        cause |= END_COLLISION
    reach = zero
    rad = N(float(cfg.reach_end_radius))
    inx, iny = abs(tdx) < rad, abs(tdy) < rad
    if inx and iny:
        marg = min(rad - abs(tdx), rad - abs(tdy))
    else:
        marg = max(abs(tdx) - rad if not inx else zero, abs(tdy) - rad if not iny else zero)
    dec.append(("reach", bool(inx and iny), two * marg / W, "linear"))
    if inx and iny:
        cause |= END_REACH
        reach = N(float(cfg.rew_reach_end))
    aa = zero
    band, angle = N(float(cfg.aa_band)), N(float(cfg.aa_angle))
    dec.append(("aa_band", (bool(alpha > band), bool(alpha < -band)), abs(abs(alpha) - band) / PI, "alpha"))
    dec.append(("aa_angle", bool(abs(alpha) >= angle), abs(abs(alpha) - angle) / PI, "alpha"))
    f = (lambda a: a) if mutant == "aa_alpha" else sin
    if alpha > band:
        aa = -f(alpha)
    if alpha < -band:
        aa = f(alpha)
    if abs(alpha) >= angle:
        aa = N(float(cfg.rew_aa))
        cause |= END_AA
    if t == int(cfg.n_steps):
        cause |= END_TIMEUP
    rew = aa + pa * lpa + pp + coll + ca * lca + reach
    return [rew, pa * lpa, pp, ca * lca, aa, dist], cause, dec


# ------------------------------------------------------------------------------------ measure, bound
_F32_MAX = Fraction(float(np.finfo(np.float32).max))
_F32_OVER = _F32_MAX + Fraction(2) ** 103    # half an ulp above the largest float32: rounds to infinity


def to_fraction(v) -> Fraction:
    if isinstance(v, Fraction):
        return v
    if isinstance(v, (float, int, np.floating)):
        return Fraction(float(v))
    sign, man, exp, _ = v._mpf_   # an mpmath mpf: (-1)^sign * man * 2^exp, exactly
    fr = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return -fr if sign else fr


def rn32(v) -> np.float32:
    """The float32 nearest ``v`` (ties to even, overflow to infinity), with no double rounding."""
    fr = to_fraction(v)
    if fr == 0:
        return np.float32(0.0)
    if abs(fr) >= _F32_OVER:
        return np.float32(math.copysign(math.inf, fr))
    with np.errstate(over="ignore", under="ignore"):
        c = np.float32(float(fr))
    if not np.isfinite(c):
        c = np.float32(math.copysign(float(_F32_MAX), fr))
    with np.errstate(over="ignore"):
        cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    cands = [k for k in cands if np.isfinite(k)]
    return min(cands, key=lambda k: (abs(Fraction(float(k)) - fr), int(np.float32(k).view(np.uint32)) & 1))


def allowance(floor_err: float, truth) -> float:
    """m = FACTOR * max(floor, EPS64 * max(1, |truth|))."""
    return FACTOR * max(floor_err, EPS64 * max(1.0, abs(float(truth))))


def within32(o, truth, m) -> bool:
    t = to_fraction(truth)
    mm = Fraction(m)
    o = np.float32(o)
    return bool(np.isfinite(o)) and rn32(t - mm) <= o <= rn32(t + mm)


def within64(o, truth, m) -> bool:
    return math.isfinite(float(o)) and abs(to_fraction(float(o)) - to_fraction(truth)) <= Fraction(m)


def needed32(o, truth) -> Fraction:
    """The smallest m for which the float32 value ``o`` is within the bracket of ``truth``: 0 where
    o = RN32(truth), else the truth's distance to the rounding boundary between o and its neighbour
    on the truth's side."""
    o = np.float32(o)
    t = to_fraction(truth)
    if o == rn32(t):
        return Fraction(0)
    if not np.isfinite(o):
        return Fraction(10) ** 30
    nb = np.nextafter(o, np.float32(math.copysign(math.inf, t - Fraction(float(o)))))
    edge = (Fraction(float(o)) + Fraction(float(nb))) / 2 if np.isfinite(nb) else _F32_OVER
    return abs(t - edge)


def err64(o, truth) -> float:
    o = float(o)
    return math.inf if not math.isfinite(o) else float(abs(to_fraction(o) - to_fraction(truth)))


# ------------------------------------------------------------------------------------ evaluation
class Eval(types.SimpleNamespace):
    """Of one case at one observed state: truth / rest (value vectors, mpmath and float), flags and end
    causes of both, the truth's decisions and the restatement's, ``collided`` (the truth's contact test)."""


def _contact(st, circles, num):
    a = num.N(float(st[2]))
    pose = (num.N(float(st[0])), num.N(float(st[1])), num.cos(a), num.sin(a))
    margins = [P.contact_margin(pose, c, num.N) for c in circles]
    hit = any(m <= 0 for m, _ in margins)
    decided = all(abs(float(m)) > 1e-12 * float(rr) for m, rr in margins)
    return hit, decided


def evaluate_one(st, S, cfg, flags_in, t_after, u, num, tape, with_reward, mutant=None):
    obs, fl, dec = observe(st, S, cfg, int(flags_in), u, num, tape, mutant)
    n_bearings = len(tape)      # (float run) the tape so far: the arguments of the bearings' atan2
    vals, cause = list(obs), 0
    if with_reward:
        circles = list(zip(S.cx, S.cy, S.cr))
        hit, hit_decided = _contact(st, circles, num)
        collided = hit or bool(flags_in & FLAG_COLLIDED)
        if collided:
            fl |= FLAG_COLLIDED
        r, cause, dec2 = reward(obs, S, cfg, collided, t_after, num, tape, mutant)
        vals += r
        dec = dec + dec2 + [("collision", collided, None if hit_decided or (flags_in & FLAG_COLLIDED) else 0.0, None)]
    return vals, fl, cause, dec, n_bearings


_mp = {}


def truth_number():
    if "num" not in _mp:
        _mp["num"] = mp_number()
    return _mp["num"]


def evaluate(case, st, u, mutant=None, want_truth=True):
    """Eval of ``case`` at the observed float64 state ``st`` (32 columns) with closest-point parameter
    ``u``.  Step route: flags and t are the case's pre-step ones (t + 1 is the step's clock)."""
    S, cfg = case.view, case.cfg
    step = case.route == "step"
    fl_in, t_after = (case.flags, case.t + 1) if step else (0, 0)
    tape = []
    rv, rfl, rcause, rdec, nb = evaluate_one(st, S, cfg, fl_in, t_after, u, float_number(), tape, step, mutant)
    ev = Eval(rest=rv, rest_flags=rfl, rest_cause=rcause, rest_dec=rdec, branch=[rel_dir_branch(y, x) for y, x in tape[:nb]])
    if want_truth:
        tv, tfl, tcause, tdec, _ = evaluate_one(st, S, cfg, fl_in, t_after, u, truth_number(), tape, step)
        ev.truth, ev.flags, ev.cause, ev.dec = tv, tfl, tcause, tdec
    return ev


def rel_dir_branch(y, x) -> str:
    """Which way csrc/d2d_device.h's rel_dir goes for the direction vector (x, y) in the default build: 'fast'
    (the rotated unit vector), or the reference sequence for a 'zero', 'tiny' (r2 <= 1e-200) or 'huge'
    (r2 >= 1e300) vector.  (The path bearings' vectors are recorded after R_w_b: the same length to an ulp.)"""
    r2 = y * y + x * x
    if r2 > 1e-200 and r2 < 1e300:
        return "fast"
    return "zero" if r2 == 0.0 else ("tiny" if r2 <= 1e-200 else "huge")


def floors_of(cases, evals) -> dict:
    """{family: {group: max |restatement - truth|}} over the cases' entries of each group."""
    out = {}
    for c, ev in zip(cases, evals):
        f = out.setdefault(c.family, dict.fromkeys(GROUPS, 0.0))
        for i, (r, t) in enumerate(zip(ev.rest, ev.truth)):
            g = GROUP_OF[i]
            f[g] = max(f[g], err64(r, t))
    return out


def undecided(case, ev, floors) -> list:
    """The decisions of the case whose margin does not exceed m of the quantity's group, and those the
    restatement takes differently from the truth."""
    bad = []
    fl = floors[case.family]
    rest = {d[0]: d[1] for d in ev.rest_dec}
    for name, outcome, margin, group in ev.dec:
        if rest.get(name) != outcome:
            bad.append((name, "restatement differs", outcome, rest.get(name)))
        if margin is None:
            continue
        m = FACTOR * max(fl[group], EPS64) if group else FACTOR * EPS64
        if not float(margin) > m:
            bad.append((name, outcome, float(margin), m))
    if ev.rest_flags != ev.flags or ev.rest_cause != ev.cause:
        bad.append(("flags/cause", ev.rest_flags, ev.flags, ev.rest_cause, ev.cause))
    return bad


def describe(floors: dict, worst: dict | None = None) -> str:
    """One line per family: ``group floor`` or ``group worst/m`` (what the tests print before they assert)."""
    lines = []
    for f, ge in floors.items():
        if worst is None:
            lines.append(f"{f:22s} " + "  ".join(f"{g} {e:.1e}" for g, e in ge.items()))
        else:
            lines.append(f"{f:22s} " + "  ".join(f"{g} {worst[f][g]:.2f}" for g in ge if g in worst.get(f, {})))
    return "\n".join(lines)


class Check:
    """Accumulates the comparison of implementations' outputs with the truth: worst error per family and
    group in units of m, violations, the share of float32 entries that are not RN32(truth)."""

    def __init__(self, floors):
        self.floors, self.worst, self.bad = floors, {}, []
        self.n32 = self.off32 = 0

    def _note(self, case, i, ratio, what):
        g = GROUP_OF[i]
        w = self.worst.setdefault(case.family, {})
        w[g] = max(w.get(g, 0.0), ratio)
        if not ratio <= 1.0:
            self.bad.append((case.family, case.note, what, i, ratio))

    def f32(self, case, ev, i, o, what="f32"):
        m = allowance(self.floors[case.family][GROUP_OF[i]], ev.truth[i])
        ratio = float(needed32(o, ev.truth[i]) / Fraction(m)) if np.isfinite(np.float32(o)) else math.inf
        if not within32(o, ev.truth[i], m):
            ratio = max(ratio, 1.0 + 1e-9)
        self.n32 += 1
        self.off32 += int(np.float32(o) != rn32(ev.truth[i]))
        self._note(case, i, ratio, what)

    def f64(self, case, ev, i, o, what="f64"):
        m = allowance(self.floors[case.family][GROUP_OF[i]], ev.truth[i])
        self._note(case, i, err64(o, ev.truth[i]) / m, what)

    def equal(self, case, name, got, want):
        if got != want:
            self.bad.append((case.family, case.note, name, got, want))

    def summary(self) -> str:
        share = self.off32 / max(1, self.n32)
        top = max((r for w in self.worst.values() for r in w.values()), default=0.0)
        return describe(self.floors, self.worst) + f"\nworst error / m over all families and groups: {top:.4f}" \
            + f"\nfloat32 entries != RN32(truth): {self.off32}/{self.n32} = {share:.4%}"


# ------------------------------------------------------------------------------------ scenarios
SCENARIOS = list(P.SCENARIOS)   # the seven shipped ones first; the tests' own scenarios follow
SEED = 11                       # of every reset
DT = 1.0 / 60
_cache = {}


def _line(name, wps, circles=(), spawn=None, angle=None, last=None):
    """A straight three-waypoint path along an axis whose quadratic is exact (a = 0, b = 0 or 1), so a path
    point is evaluated without rounding in every number type."""
    from drone2d_amd.scenarios import QPMIPath, Scenario

    wps = np.asarray(wps, np.float64)
    path = QPMIPath(wps)
    d = wps[-1] - wps[0]
    assert len(wps) == 3 and (d[0] == 0.0) != (d[1] == 0.0) and d.sum() > 0
    along = 0 if d[1] == 0.0 else 1
    xp, yp = np.array([0.0, 0.0, wps[0][0]]), np.array([0.0, 0.0, wps[0][1]])
    (xp if along == 0 else yp)[1] = 1.0
    path.x_params, path.y_params = [xp], [yp]
    if last is not None:    # the target (wp_last_x, wp_last_y) is a field of its own: off the path's end
        wps = np.concatenate([wps[:-1], np.asarray([last], np.float64)])
    if spawn is None:
        sp, ang = (wps[0][0] - 50.0, wps[0][0] + 50.0, wps[0][1] - 50.0, wps[0][1] + 50.0), (-0.3, 0.3)
    else:
        sp, ang = (spawn[0], spawn[0], spawn[1], spawn[1]), (angle, angle)
    return Scenario(name, wps, path, np.asarray(circles, np.float64).reshape(-1, 3), sp, ang)


HLINE = [(200.0, 650.0), (650.0, 650.0), (1100.0, 650.0)]
VLINE = [(650.0, 200.0), (650.0, 650.0), (650.0, 1100.0)]
ORIGIN_LINE = [(-900.0, 0.0), (-450.0, 0.0), (0.0, 0.0)]
C0 = (600.0, 400.0, 20.0)       # the circle of the "line" scenario
TIE = [(450.0, 400.0, 20.0), (750.0, 400.0, 20.0), (600.0, 580.0, 20.0), (600.0, 220.0, 20.0), (1200.0, 1200.0, 20.0)]
ODD = (100.0, 1200.0, 35.0)     # a far circle of another radius: the scenario has no uniform radius
# spawn points of the reset route's own scenarios: (family, note, path, circles, (x, y), angle)
_POINTS = (
    [("coincident", "on centre a=%g" % a, HLINE, [(600.0, 500.0, 30.0)], (600.0, 500.0), a) for a in (0.0, 0.2, -0.7)]
    + [("coincident", "on last waypoint a=%g" % a, HLINE, [C0], (1100.0, 650.0), a) for a in (0.0, 0.2, -0.7, 2.5, -2.5)]
    + [("coincident", "on the path a=%g" % a, HLINE, [C0], (600.0, 650.0), a) for a in (0.0, 0.2, -2.5)]
    + [("tiny_vector", "at (%g, %g)" % p, ORIGIN_LINE, [(0.0, 0.0, 30.0)], p, 0.2)
       for p in ((1e-100, 0.0), (1e-101, 0.0), (1e-99, 0.0), (1e-90, 1e-95), (1e-110, 1e-105), (0.0, 1e-100),
                 (-1e-100, 0.0), (7e-101, 7.2e-101), (7e-101, 7.1e-101))])
RESET_LANES = 8                 # spawn draws per shipped scenario in the ``reset`` family


def scenarios():
    """[Scenario]: the shipped seven, then the tests' own (``scn_index`` finds one by name)."""
    if "scn" not in _cache:
        import limit_scenarios as ls
        from drone2d_amd.scenarios import create_test_scenario

        out = [create_test_scenario(s, 1300, 1300) for s in P.SCENARIOS]
        out += [_line("line", HLINE, [C0]), _line("vline", VLINE), _line("tie", HLINE, TIE),
                _line("tie_m", HLINE, TIE + [ODD]), _line("tie23", HLINE, TIE[1:]), _line("tie23_m", HLINE, TIE[1:] + [ODD]),
                _line("inside", HLINE, [(600.0, 400.0, 100.0)]), _line("far", HLINE, [(3000.0, 100.0, 10.0)]),
                _line("vertex", HLINE, [(600.0, 400.0, 30.0)]), _line("vertex_m", HLINE, [(600.0, 400.0, 30.0), ODD]),
                _line("allend", HLINE, [(1100.0, 650.0, 60.0)]), _line("detached", HLINE, [C0], last=(1100.0, 665.0))]
        for p in list(ls.PAIRINGS[:9]) + [("w4_zig", 3, "mixed")]:
            s = ls.scenario(*p)
            s.name = "lim_" + s.name
            out.append(s)
        for k, (_, _, wps, circles, pt, a) in enumerate(_POINTS):
            out.append(_line("pt%d" % k, wps, circles, pt, a))
        _cache["scn"] = out
        _cache["scn_c"] = [s.to_c() for s in out]
        _cache["view"] = [scn_view(c) for c in _cache["scn_c"]]
    return _cache["scn"]


def scn_index(name):
    return [s.name for s in scenarios()].index(name)


def cfg_of(key):
    """'train': ENV_TRAIN_CONFIG; 'nolambda': use_Lambda off."""
    from drone2d_amd.config import ENV_TRAIN_CONFIG, make_cfg

    if ("cfg", key) not in _cache:
        _cache["cfg", key] = make_cfg(dict(ENV_TRAIN_CONFIG, use_Lambda=(key != "nolambda")), auto_reset=False)
    return _cache["cfg", key]


def cfg_kwargs(key):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, use_Lambda=(key != "nolambda"))


def closest_u(scn, x, y):
    import oracle

    scenarios()
    return oracle.closest_u(_cache["scn_c"][scn], float(x), float(y))[0]


# ------------------------------------------------------------------------------------ cases
class Case(types.SimpleNamespace):
    """family, note, route ('step' / 'reset'), scn (index into scenarios()), cfgkey, and for the step route
    pre (float64[32], columns 30 and 31 zero), flags, t, act (float32[2]); view and cfg are filled in."""


def rest_at(x, y, th):
    """A rig at rest: one step leaves the frame's position and angle exactly where they are."""
    return P.rig(x, y, th)


def pre_for(x, y, th, vx, vy, w, act=(0.0, 0.0), tol=1e-11):
    """The state before a step after which the frame is at (x, y, th) with velocity (vx, vy, w), to a few
    ulp, by fixed-point iteration on the unfused float64 physics restatement."""
    fL, fR = P.thrust(act)
    target = (x, y, th, vx, vy, w)
    guess = [x - vx * DT, y - vy * DT, th - w * DT, vx, vy, w]
    for _ in range(80):
        post, _pose = P.step(P.rig(*guess), fL, fR, float, math.sin, math.cos)
        if all(abs(t - p) <= 1e-14 * max(1.0, abs(t)) for t, p in zip(target, post[:6])):
            break
        guess = [g + (t - p) for g, t, p in zip(guess, target, post[:6])]
    post, _pose = P.step(P.rig(*guess), fL, fR, float, math.sin, math.cos)
    assert all(abs(t - p) <= tol * max(1.0, abs(t)) for t, p in zip(target, post[:6])), (target, post[:6])
    return P.rig(*guess)


def _scan(scn, f, x0, y0, tx, ty, targets, h=1e-9, n=3000):
    """Frame positions (x0, y0) + k h (tx, ty), |k| <= n, whose ``f(u)`` (u the oracle's closest-point
    parameter there) comes nearest each target: the search's result has a tolerance of 1e-6 in u, so a
    value of u to 1e-9 is found, not computed."""
    rows = []
    for k in range(-n, n + 1):
        x, y = x0 + k * h * tx, y0 + k * h * ty
        rows.append((f(closest_u(scn, x, y)), x, y))
    return [min(rows, key=lambda r: abs(r[0] - t))[1:] for t in targets]


def _build_cases():
    import limit_scenarios as ls

    scenarios()
    cs = []
    zero_act = np.zeros(2, np.float32)

    def add(family, note, scn, pre, flags=0, t=0, cfgkey="train", act=zero_act):
        pre = np.array(pre, np.float64)
        pre[30:32] = 0.0
        cs.append(Case(family=family, note=note, route="step", scn=scn if isinstance(scn, int) else scn_index(scn),
                       cfgkey=cfgkey, pre=pre, flags=int(flags), t=int(t), act=np.asarray(act, np.float32)))

    # golden/<scenario>: every 5th crafted row
    g = np.load(os.path.join(P.GOLDEN, "crafted.npz"), allow_pickle=False)
    for k in range(0, len(g["rew"]), 5):
        si = int(g["scn"][k])
        add("golden/" + SCENARIOS[si], "row %d" % k, si, g["pre"][k], int(g["pre_i"][k, 1]) | (int(g["pre_i"][k, 2]) << 1),
            int(g["pre_i"][k, 0]), act=g["act"][k])

    # bearing_axes ------------------------------------------------------------------------------
    fam = "bearing_axes"
    cx, cy = C0[0], C0[1]
    dirs = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    for ex, ey in dirs:     # the obstacle's direction on the axes and diagonals (exact offsets)
        add(fam, "obstacle dir (%d, %d)" % (ex, ey), "line", rest_at(cx + 200.0 * ex, cy + 200.0 * ey, 0.3))
    px, py = cx + 160.0, cy + 120.0
    a0 = math.atan2(py - cy, px - cx)   # ssa's argument (atan2 - al - pi) + pi wraps where atan2 = al
    for tag, al in (("-1e-9", a0 - 1e-9), ("+1e-9", a0 + 1e-9), ("-1e-12", a0 - 1e-12), ("+1e-12", a0 + 1e-12),
                    ("-ulp", np.nextafter(a0, -4.0)), ("+ulp", np.nextafter(a0, 4.0)), ("0", a0)):
        add(fam, "obstacle wrap al = atan2 %s" % tag, "line", rest_at(px, py, float(al)))
    for ex, ey in dirs:     # the velocity's direction (to the physics step's rounding)
        n = math.hypot(ex, ey)
        add(fam, "velocity dir (%d, %d)" % (ex, ey), "line", pre_for(300.0, 900.0, 0.3, 200.0 * ex / n, 200.0 * ey / n, 0.0))
    for tag, dl in (("-1e-9", -1e-9), ("+1e-9", 1e-9)):    # ssa(atan2(vy, vx) - al) wraps where the difference is pi
        add(fam, "velocity wrap %s" % tag, "line", pre_for(300.0, 900.0, 2.0 - math.pi + dl, 200.0 * math.cos(2.0), 200.0 * math.sin(2.0), 0.0))
    wlx, wly = HLINE[-1]
    for ex, ey in dirs:     # the lookahead point's direction: the lock preset, the point is the last waypoint
        add(fam, "lookahead dir (%d, %d)" % (-ex, -ey), "line", rest_at(wlx + 100.0 * ex, wly + 100.0 * ey, 0.3), FLAG_LA_LOCK)
    for tag, dy in (("+1e-9", 1e-7), ("-1e-9", -1e-7), ("+1e-12", 1e-10), ("-1e-12", -1e-10),
                    ("+ulp", float(np.spacing(wly))), ("-ulp", -float(np.spacing(wly)))):
        # the direction to the point is pi -+ dy / 100: either side of ssa's wrap at atan2(R d) - al = -pi
        add(fam, "lookahead wrap %s" % tag, "line", rest_at(wlx + 100.0, wly + dy, 0.3), FLAG_LA_LOCK)
    for note, x, y in (("above", 600.0, 680.0), ("below", 600.0, 620.0), ("behind the start", 150.0, 650.0),
                       ("beyond the end", 1150.0, 650.0)):   # the closest point's direction on the axes
        add(fam, "closest point " + note, "line", rest_at(x, y, -0.4))
    # the search is bounded to [-10, L + 10]: a frame behind the start or beyond the end sees the clamped points
    # (190, 650) and (1110, 650) (less the search's 1e-6 in u, along the path: the offset across it is exact)
    for ex, ey, x0 in ((-1, 1, 190.0), (-1, -1, 190.0), (1, 1, 1110.0), (1, -1, 1110.0)):
        add(fam, "closest point diagonal (%d, %d)" % (-ex, -ey), "line", rest_at(x0 + 40.0 * ex, 650.0 + 40.0 * ey, -0.4))
    for tag, dy in (("+1e-9", 4e-8), ("-1e-9", -4e-8), ("+1e-12", 4e-11), ("-1e-12", -4e-11),
                    ("+ulp", float(np.spacing(650.0))), ("-ulp", -float(np.spacing(650.0)))):
        # beyond the end the direction to the point is pi -+ dy / 40: either side of ssa's wrap
        add(fam, "closest point wrap %s" % tag, "line", rest_at(1150.0, 650.0 + dy, -0.4))
    # big_angle: the same bearings at unwrapped frame angles (argument reduction sets another floor)
    for k, mag in enumerate((10.0, 1e3, 1e5, 1e6 + 0.25)):
        for sign in (1.0, -1.0):
            add("big_angle", "al = %+g" % (sign * mag), "line", pre_for(cx + 150.0 + 10 * k, cy + 170.0, sign * mag, 60.0, -35.0 * sign, 0.0, tol=1e-7))

    # nearest3 ----------------------------------------------------------------------------------
    fam = "nearest3"
    for p in list(ls.PAIRINGS[:9]) + [("w4_zig", 3, "mixed")]:
        name = "lim_%s_%d%s" % (p[0], p[1], p[2][0])
        xmin, xmax, ymin, ymax = ls.spawn_rect(p[0])
        for ox, oy in ((0.0, 0.0), (60.0, -40.0)):
            add(fam, "%s at +(%g, %g)" % (name, ox, oy), name, rest_at(0.5 * (xmin + xmax) + ox, 0.5 * (ymin + ymax) + oy, 0.2))
    for name in ("tie", "tie_m", "tie23", "tie23_m"):
        add(fam, name + " exact", name, rest_at(600.0, 400.0, 0.1))
    for rel in (1e-12, 1e-9):      # the frame a little towards one of the tied pair: a relative gap of about rel
        for sign in (1.0, -1.0):
            add(fam, "tie near %+g" % (sign * rel), "tie", rest_at(600.0 + sign * rel * 40.0, 400.0, 0.1))
    add(fam, "inside a circle", "inside", rest_at(610.0, 400.0, 0.1))
    add(fam, "farther than the diagonal", "far", rest_at(100.0, 100.0, 0.1))
    for sign in (1.0, -1.0):       # the nearest vertex switches between x = +50 and -50, y = +5 and -5
        add(fam, "x vertex switch %+g" % sign, "line", rest_at(cx + sign * 1e-6, cy - 70.0, 0.1))
        add(fam, "y vertex switch %+g" % sign, "line", rest_at(cx - 120.0, cy + sign * 1e-6, 0.1))
    for name in ("vertex", "vertex_m"):   # the vertex (50, -5) + p exactly on the centre: q = 0
        add(fam, name + " on the centre", name, rest_at(550.0, 405.0, 0.1))

    # lookahead ---------------------------------------------------------------------------------
    fam = "lookahead"
    import oracle
    look = 220.0
    for name in ("line", "vline", "lim_w3_arc_0u", "S_corridor", "lim_w16_zig_64u"):
        si = scn_index(name)
        sc = _cache["scn_c"][si]
        L = _cache["view"][si].us[-1]
        u0 = L - look
        p0 = np.array(oracle.path_eval(sc, u0))
        tg = np.array(oracle.path_eval(sc, u0 + 1e-3)) - np.array(oracle.path_eval(sc, u0 - 1e-3))
        tg /= np.hypot(*tg)
        for off in (30.0, -30.0, 8.0, -8.0):
            q = p0 + off * np.array([-tg[1], tg[0]])
            for _ in range(12):     # off the path the parameter does not advance one for one: home in first
                q = q - ((closest_u(si, q[0], q[1]) + look) - L) * tg
            if abs((closest_u(si, q[0], q[1]) + look) - L) < 1e-6:
                break
        for (x, y), tag in zip(_scan(si, lambda u: (u + look) - L, q[0], q[1], tg[0], tg[1], (1e-9, -1e-9)), ("+", "-")):
            add(fam, "%s: u + lookahead %s 1e-9 of L" % (name, tag), si, rest_at(x, y, 0.2))
        for f in (0.1, 0.5, 0.9):     # along the path, off it by 25 px
            p = np.array(oracle.path_eval(sc, f * L)) + np.array([7.0, 24.0])
            add(fam, "%s at %.1f L" % (name, f), si, rest_at(p[0], p[1], 0.2))
        p = np.array(oracle.path_eval(sc, 0.05 * L)) + np.array([5.0, -20.0])
        add(fam, "%s: lock preset far from the end" % name, si, rest_at(p[0], p[1], 0.2), FLAG_LA_LOCK)
    # a target 15 px off the path's end: the lookahead point never locks, so the clamp at L shows in obs 21, 22
    si = scn_index("detached")
    pts = _scan(si, lambda u: (u + look) - 900.0, 880.0, 680.0, 1.0, 0.0, (1e-9, -1e-9))
    for (x, y), note in zip(pts + [(1000.0, 680.0), (1150.0, 640.0)], ("+1e-9 of L", "-1e-9 of L", "120 past L", "270 past L")):
        add(fam, "detached target: u + lookahead " + note, si, rest_at(x, y, 0.2))
    for name, axis in (("line", 0), ("vline", 1)):   # the lookahead point 10 -+ eps from the last waypoint on one axis
        si = scn_index(name)
        wl = np.array(HLINE[-1] if axis == 0 else VLINE[-1])
        start = (HLINE if axis == 0 else VLINE)[0][axis]
        t = np.eye(2)[axis]
        q = wl - (10.0 + look) * t + 30.0 * np.eye(2)[1 - axis]
        eps = (1e-6, -1e-6, 1e-9, -1e-9)
        pts = _scan(si, lambda u: (wl[axis] - (start + (u + look))) - 10.0, q[0], q[1], t[0], t[1], eps, h=1e-9, n=3000)
        for (x, y), e in zip(pts, eps):
            add(fam, "%s: lookahead point at 10 %+g px" % (name, e), si, rest_at(x, y, 0.2))

    # reward_thresholds -------------------------------------------------------------------------
    fam = "reward_thresholds"
    deltas = (1e-6, -1e-6, 1e-9, -1e-9)

    def x_for_d(T):     # the frame's x, right of C0 at its height, at vertex distance T from the circle
        return cx + 50.0 + math.sqrt((T + C0[2]) ** 2 - 25.0)

    for thr, what in ((150.0, "danger_range"), (30.0, "0.2 danger_range")):
        for dl in deltas:
            add(fam, "d at %s %+g" % (what, dl), "line", rest_at(x_for_d(thr * (1.0 + dl)), cy, 0.1))
    for thr, what in ((math.pi / 4, "aa_band"), (math.pi / 2, "aa_angle")):
        for sign in (1.0, -1.0):
            for dl in deltas:
                add(fam, "alpha at %+g %s %+g" % (sign, what, dl), "line", rest_at(300.0, 800.0, sign * thr * (1.0 + dl)))
    for dl in deltas:
        add(fam, "target dx at reach_end_radius %+g" % dl, "line", rest_at(wlx - 20.0 * (1.0 + dl), wly + 3.0, 0.1))
    for dl in deltas:
        add(fam, "target dy at reach_end_radius %+g" % dl, "line", rest_at(wlx + 3.0, wly + 20.0 * (1.0 + dl), 0.1))
        add(fam, "target dx, dy at reach_end_radius %+g" % dl, "line",
            rest_at(wlx + 20.0 * (1.0 + dl), wly - 20.0 * (1.0 + dl), 0.1))
    for dl in deltas:
        add(fam, "path distance at pa_band_edge %+g" % dl, "line", rest_at(500.0, 650.0 + 40.0 * (1.0 + dl), 0.1))
    for top, what in ((31.25, "PP max"), (-12.5, "PP min")):   # along (against) the lookahead direction +x
        for dl in deltas:
            add(fam, "%s %+g" % (what, dl), "line", pre_for(400.0, 650.0, 0.1, top * (1.0 + dl), 0.0, 0.0))
    fx = cx + 120.0      # 50.2 px from C0, which lies at world bearing pi from the frame
    for deg, what in ((0.0, "0"), (20.0, "danger_angle"), (180.0, "180")):
        for dl in deltas:
            th = math.radians(deg) * (1.0 + dl) if deg else dl
            add(fam, "adiff at %s %+g" % (what, dl), "line", pre_for(fx, cy, 0.0, 100.0 * math.cos(math.pi - th), 100.0 * math.sin(math.pi - th), 0.0))
    for T in (50.0, 20.0):
        add(fam, "use_lambda off, d = %g" % T, "line", rest_at(x_for_d(T), cy, 0.1), cfgkey="nolambda")
    add(fam, "t == n_steps", "line", rest_at(300.0, 800.0, 0.1), t=1099)
    add(fam, "collision, reach-end and AA together", "allend", rest_at(wlx + 2.0, wly - 1.0, 2.0))

    # saturation --------------------------------------------------------------------------------
    fam = "saturation"
    for sign in (1.0, -1.0):
        for dl in deltas:
            add(fam, "w / 11.7 at %+g %+g" % (sign, dl), "line", pre_for(300.0, 800.0, 0.1, 5.0, -3.0, sign * 11.7 * (1.0 + dl)))
    for vx, vy in ((2000.0, -1500.0), (-3000.0, 100.0), (0.0, 1400.0)):
        add(fam, "speed (%g, %g) above VEL_MAX" % (vx, vy), "line", pre_for(300.0, 800.0, 0.1, vx, vy, 0.0))

    # the reset route ----------------------------------------------------------------------------
    first_pt = scn_index("pt0")
    for k, (family, note, *_rest) in enumerate(_POINTS):
        cs.append(Case(family=family, note=note, route="reset", scn=first_pt + k, cfgkey="train"))
    for si in range(len(P.SCENARIOS)):
        for k in range(RESET_LANES):
            cs.append(Case(family="reset", note="%s draw %d" % (SCENARIOS[si], k), route="reset", scn=si, cfgkey="train"))
    for c in cs:
        c.view, c.cfg = _cache["view"][c.scn], cfg_of(c.cfgkey)
    count = {}
    for c in cs:
        count[c.family] = count.get(c.family, 0) + 1
    assert max(count.values()) <= 64 and len(cs) <= 500, (count, len(cs))
    return cs


def cases():
    """Every case of every family, in a fixed order (built once per process)."""
    if "cases" not in _cache:
        _cache["cases"] = _build_cases()
    return _cache["cases"]


# ------------------------------------------------------------------------------------ running cases
class Out(types.SimpleNamespace):
    """What an implementation returned for a case: obs (float32[27]), st (float64[32]), ist (int32[3]); the
    step route also rew, term, trunc, info (float32[12])."""


def run_batch(make_env, cs, mixed=True, **kw):
    """Run the cases ``cs`` (all of one route and configuration) as one batch and return [Out] in their
    order.  ``make_env(n, scenario list, env_scenario, cfgkey, **kw)`` gives an object with ``reset(seed)``,
    ``set_state``, ``step``, ``get_state`` and ``close`` over NumPy arrays (``st`` [32, n], ``ist`` [3, n])."""
    route, cfgkey = cs[0].route, cs[0].cfgkey
    assert all(c.route == route and c.cfgkey == cfgkey for c in cs) and len(cs) <= 500
    used = sorted({c.scn for c in cs})
    assert mixed or len(used) == 1
    env = make_env(len(cs), [scenarios()[s] for s in used], np.array([used.index(c.scn) for c in cs], np.int32), cfgkey, **kw)
    try:
        obs0 = env.reset(SEED)
        if route == "reset":
            st, ist = env.get_state()
            return [Out(obs=obs0[k].copy(), st=st[:, k].copy(), ist=ist[:, k].copy()) for k in range(len(cs))]
        set_cases(env, cs)
        return step_outs(env, cs)
    finally:
        env.close()


def set_cases(env, cs):
    ist = np.zeros((3, len(cs)), np.int32)
    ist[0], ist[1] = [c.t for c in cs], [c.flags for c in cs]
    env.set_state(np.ascontiguousarray(np.stack([c.pre for c in cs]).T), ist)


def step_outs(env, cs):
    obs, rew, term, trunc, info = env.step(np.stack([c.act for c in cs]).astype(np.float32))
    st, ist = env.get_state()
    return [Out(obs=obs[k].copy(), rew=rew[k], term=bool(term[k]), trunc=bool(trunc[k]), info=info[k].copy(),
                st=st[:, k].copy(), ist=ist[:, k].copy()) for k in range(len(cs))]


def pad_case(scn, cfgkey="train"):
    """A rig at rest far from every circle of every scenario here: fills the other lanes of a wave."""
    scenarios()
    return Case(family="pad", note="pad", route="step", scn=scn, cfgkey=cfgkey, pre=P.pad_state(), flags=0, t=0,
                act=np.zeros(2, np.float32), view=_cache["view"][scn], cfg=cfg_of(cfgkey))


def same_bits(a, b) -> bool:
    """obs, reward and state columns 30 and 31 of two Outs of the step route, bit for bit."""
    return (a.obs.tobytes() == b.obs.tobytes() and np.float32(a.rew).tobytes() == np.float32(b.rew).tobytes()
            and a.st[30:32].tobytes() == b.st[30:32].tobytes())


def batches(keep=lambda c: True, per_scenario=False):
    """The case indices grouped into batches: by route and configuration, and by scenario too for the step
    route when ``per_scenario`` (the single-scenario kernel); the reset route is always one batch, its
    spawn draws belong to its lanes."""
    out = {}
    for i, c in enumerate(cases()):
        if keep(c):
            key = (c.route, c.cfgkey, c.scn if (per_scenario and c.route == "step") else -1)
            out.setdefault(key, []).append(i)
    return list(out.values())


_evals = {}


def eval_at(i, out):
    """The (memoised) evaluation of case i at the state an implementation observed."""
    c = cases()[i]
    key = (i, out.st[:6].tobytes())
    if key not in _evals:
        _evals[key] = evaluate(c, out.st, closest_u(c.scn, out.st[0], out.st[1]))
    return _evals[key]


INFO_CA, INFO_PA, INFO_PP, INFO_COLL, INFO_REACH, INFO_AA = 0, 1, 2, 3, 4, 5
INFO_STEPS, INFO_CAUSE, INFO_REWARD = 7, 8, 11


def compare(check, i, out, obs64=None):
    """Hold one case's outputs to the truth at the state it observed.  ``obs64``: a float64 observation of
    the same state (the oracle's ``observe_state``), held by the float64 rule."""
    c = cases()[i]
    ev = eval_at(i, out)
    for k in range(OBS_DIM):
        check.f32(c, ev, k, out.obs[k], "obs")
        if obs64 is not None:
            check.f64(c, ev, k, obs64[k], "obs64")
    check.equal(c, "flags", int(out.ist[1]), ev.flags)
    if c.route == "reset":
        check.equal(c, "t", int(out.ist[0]), 0)
        return ev
    check.f32(c, ev, V_REW, out.rew, "reward")
    check.f32(c, ev, V_REW, out.info[INFO_REWARD], "info reward")
    check.f64(c, ev, V_REW, out.st[31], "state 31")
    check.f64(c, ev, V_DIST, out.st[30], "state 30")
    for v, col in ((V_PA, INFO_PA), (V_PP, INFO_PP), (V_CA, INFO_CA), (V_AA, INFO_AA)):
        check.f32(c, ev, v, out.info[col], "info %d" % col)
    cfg = c.cfg
    check.equal(c, "info collision", float(out.info[INFO_COLL]), float(cfg.rew_collision) if ev.cause & END_COLLISION else 0.0)
    check.equal(c, "info reach", float(out.info[INFO_REACH]), float(cfg.rew_reach_end) if ev.cause & END_REACH else 0.0)
    check.equal(c, "info cause", int(out.info[INFO_CAUSE]), ev.cause)
    check.equal(c, "info steps", int(out.info[INFO_STEPS]), c.t + 1)
    check.equal(c, "terminated", out.term, ev.cause != 0)
    check.equal(c, "truncated", out.trunc, False)
    check.equal(c, "t", int(out.ist[0]), c.t + 1)
    return ev
