#!/usr/bin/env python3
"""CPU analysis of the Brent searches a K1 path wave runs (no GPU): steady-state lane positions
from the C oracle (the bench's workload: random U(-1,1) actions, auto-reset, W warmup steps), then
per search scipy's fminbound step sequence (_optimize.py:2251-2398) with its decisions logged:

  kind / dev   the golden-march table kind and the first step whose decision differs (the search
               resumes brent_step there: the "continuation")
  decisions    per continuation step: parabolic or golden, new probe better (le) or worse

and per wave of 64 consecutive slots: lanes in continuation, max / sum of continuation steps, so
lane utilisation and packing alternatives can be priced before writing kernel code.

    python tools/brent_lanes.py [--scenario corridor] [--envs 4096] [--warmup 300] [--early 7 10 13 16]
                                [--ride 6 9 12 15 18]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "oracle")]

GOLD = 0.3819660112501051
SQRT_EPS = 1.4832396974191326e-08


def fminbound_log(f, x1, x2, xatol=1e-6, maxfun=500):
    a, b = x1, x2
    fulc = a + GOLD * (b - a)
    nfc = xf = fulc
    rat = e = 0.0
    x = xf
    fx = f(x)
    num = 1
    ffulc = fnfc = fx
    xm = 0.5 * (a + b)
    tol1 = SQRT_EPS * abs(xf) + xatol / 3.0
    tol2 = 2.0 * tol1
    log = []  # (par, le, plain worse, speculation possible before the step) per step
    while abs(xf - xm) > (tol2 - 0.5 * (b - a)):
        spec_ok = (nfc != xf) and (fulc != xf) and (fulc != nfc)
        golden = True
        par = False
        if abs(e) > tol1:
            golden = False
            r = (xf - nfc) * (fx - ffulc)
            q = (xf - fulc) * (fx - fnfc)
            p = (xf - fulc) * q - (xf - nfc) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            r = e
            e = rat
            if (abs(p) < abs(0.5 * q * r)) and (p > q * (a - xf)) and (p < q * (b - xf)):
                rat = (p + 0.0) / q
                x = xf + rat
                par = True
                if ((x - a) < tol2) or ((b - x) < tol2):
                    si = np.sign(xm - xf) + ((xm - xf) == 0)
                    rat = tol1 * si
            else:
                golden = True
        if golden:
            e = (a - xf) if xf >= xm else (b - xf)
            rat = GOLD * e
        si = np.sign(rat) + (rat == 0)
        x = xf + si * max(abs(rat), tol1)
        fu = f(x)
        num += 1
        le = fu <= fx
        plain_worse = (not le) and not (fu <= fnfc) and not (fu <= ffulc)
        if le:
            if x >= xf:
                a = xf
            else:
                b = xf
            fulc, ffulc = nfc, fnfc
            nfc, fnfc = xf, fx
            xf, fx = x, fu
        else:
            if x < xf:
                a = x
            else:
                b = x
            if (fu <= fnfc) or (nfc == xf):
                fulc, ffulc = nfc, fnfc
                nfc, fnfc = x, fu
            elif (fu <= ffulc) or (fulc == xf) or (fulc == nfc):
                fulc, ffulc = x, fu
        if log:  # the previous step's "better" speculation held iff it was better and this step is golden
            log[-1] = log[-1][:4] + (log[-1][1] and not par,)
        log.append((par, le, plain_worse, spec_ok, False))
        xm = 0.5 * (a + b)
        tol1 = SQRT_EPS * abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        if num >= maxfun:
            break
    return xf, log


def table_dev(log, kind_len):
    """kind (step 0: better -> 1, worse -> 0) and the first step k >= 1 whose decision is not
    'golden, better' (the table's), capped at the table length."""
    kind = 1 if log and log[0][1] else 0
    n = kind_len[kind]
    for k in range(1, min(len(log), n)):
        par, le = log[k][:2]
        if par or not le:
            return kind, k
    return kind, min(len(log), n)


def forced_len(L, kind):
    """Length of the golden-march table of `kind` for a path of length L: the forced march (kind 0:
    step 0 worse, then every step better; kind 1: every step better), capped at the table's 48 steps."""
    a, bb = -10.0, L + 10.0
    fulc = a + GOLD * (bb - a)
    xf = nfc = fulc
    e = 0.0
    k = 0
    xm = 0.5 * (a + bb)
    tol1 = SQRT_EPS * abs(xf) + 1e-6 / 3.0
    while abs(xf - xm) > (2 * tol1 - 0.5 * (bb - a)) and k < 48:
        e = (a - xf) if xf >= xm else (bb - xf)
        rat = GOLD * e
        x = xf + (np.sign(rat) + (rat == 0)) * max(abs(rat), tol1)
        le = not (kind == 0 and k == 0)
        if le:
            if x >= xf:
                a = xf
            else:
                bb = xf
            xf = x
        else:
            if x < xf:
                a = x
            else:
                bb = x
        k += 1
        xm = 0.5 * (a + bb)
        tol1 = SQRT_EPS * abs(xf) + 1e-6 / 3.0
    return k


def dist_to(sc, p):
    """Distance from point p to the path of the C scenario `sc` as a function of u (the oracle's path)."""
    import oracle

    def f(u):
        x, y = oracle.path_eval(sc, u)
        dx, dy = x - p[0], y - p[1]
        return math.sqrt(dx * dx + dy * dy)
    return f


def classify(sc, L, kind_len, px, py):
    """(kind, dev, continuation steps) of the search from (px, py): dev == kind_len[kind] and no
    continuation when the search follows its whole table."""
    _, log = fminbound_log(dist_to(sc, (px, py)), -10.0, L + 10.0)
    kind, dev = table_dev(log, kind_len)
    return kind, dev, max(0, len(log) - dev)


def up3(k):
    return 3 * ((k + 2) // 3)


def early_model(kind, dev, cont, kind_len, E, recheck_cost):
    """The path wave's chain per wave of 64 lanes, as (re-check steps, continuation steps) on the
    critical lane and their sum with a re-check step priced at `recheck_cost` continuation steps.
    E = 0: today's split by halves (the path wave re-checks [1, split), waits for the other wave's
    [split, len) -- 3 window distances, then passes of 3 -- and only then resumes any lane).
    E > 0: the path wave re-checks [1, E) and resumes its early deviators at once; the lanes that
    deviate in the other wave's [E, len) start when both waves are done."""
    out = []
    split = max(4, (kind_len[0] + 3) // 2) if E == 0 else E
    for w in range(len(kind) // 64):
        k, d, c = (x[64 * w:64 * w + 64] for x in (kind, dev, cont))
        ln = np.array(kind_len)[k]
        own = up3(int(np.minimum(d, np.minimum(split, ln)).max()) - 1)   # W2's passes run to the last lane
        other = 3 + up3(int(np.maximum(ln - split, 0).max()))
        if E == 0:
            r, s = max(own, other), int(c.max())
        else:
            early = (d < np.minimum(split, ln)) & (c > 0)
            late = ~early & (c > 0)
            ce = int(c[early].max()) if early.any() else 0
            cl = int(c[late].max()) if late.any() else 0
            a = (own, ce)
            b = (max(own, other), cl) if late.any() else (0, 0)
            r, s = max(a, b, key=lambda x: x[0] * recheck_cost + x[1])
        out.append((r, s, r * recheck_cost + s))
    return np.array(out, float)


def early_report(kind, dev, cont, kind_len, Es, recheck_cost):
    """What `--early` prints: where the continuing lanes deviate and what an early start would buy."""
    kind, dev, cont = (np.asarray(x) for x in (kind, dev, cont))
    going = cont > 0
    hist = np.bincount(dev[going], minlength=max(kind_len) + 1)
    waves = cont.reshape(-1, 64)
    longest = waves.argmax(1) + 64 * np.arange(len(waves))
    longest = longest[waves.max(1) > 0]
    res = {"table_len": list(kind_len), "split_today": max(4, (kind_len[0] + 3) // 2), "recheck_cost": recheck_cost,
           "cont_lane_frac": float(going.mean()),
           "dev_hist_continuing": {int(k): int(v) for k, v in enumerate(hist) if v},
           "dev_of_wave_longest_lane": {int(k): int(v) for k, v in enumerate(np.bincount(dev[longest])) if v},
           "wave_cont_max_mean": float(waves.max(1).mean()), "cont_max": int(cont.max()), "early": {}}
    for E in Es:
        cls = {"dev<E": going & (dev < E), "dev>=E": going & (dev >= E)}
        m0, m = early_model(kind, dev, cont, kind_len, 0, recheck_cost), early_model(kind, dev, cont, kind_len, E,
                                                                                       recheck_cost)
        res["early"][int(E)] = {
            "frac_continuing_below_E": float((dev[going] < E).mean()) if going.any() else 0.0,
            "cont_by_class": {k: {"lanes": int(v.sum()), "mean": float(cont[v].mean()) if v.any() else 0.0,
                                  "max": int(cont[v].max()) if v.any() else 0} for k, v in cls.items()},
            "chain_today": {"recheck": float(m0[:, 0].mean()), "cont": float(m0[:, 1].mean()),
                            "sum_mean": float(m0[:, 2].mean()), "sum_max": float(m0[:, 2].max())},
            "chain_E": {"recheck": float(m[:, 0].mean()), "cont": float(m[:, 1].mean()),
                        "sum_mean": float(m[:, 2].mean()), "sum_max": float(m[:, 2].max())},
            "gain_mean": float(1.0 - m[:, 2].mean() / m0[:, 2].mean()),
            "gain_slowest_wave": float(1.0 - m[:, 2].max() / m0[:, 2].max()),
        }
    return res


def ride_report(kind, dev, cont, kind_len, E, Rs, recheck_cost, step_valu=150.0, check_valu=45.0):
    """What `--ride` prints.  Under the early start (E) the lanes that followed [1, E) sit switched off
    in the path wave's continuation loop; as riders they run brent_step from the snapshot before step E
    in every pass, and the other wave re-checks [E + R, len) only.  Per wave of 64 lanes:

      natural loop   the passes the loop runs today: the longest continuation among the lanes that
                     deviate below E (0: the wave has none and only waits for the other wave)
      added passes   max(0, R - natural loop) when the wave has a rider: passes run for the riders alone
      saved steps    the other wave's re-check steps dropped, in its passes of three

    and the wave's chain in continuation steps (a re-check step priced at `recheck_cost`): the first
    loop, then the lanes that start at the join -- today every lane that deviates at or past E, after
    the other wave's [E, len); with riders only those at or past E + R (a rider that deviates in
    [E, E + R) has been stepping since pass 0 and needs dev - E + cont passes in all)."""
    kind, dev, cont = (np.asarray(x) for x in (kind, dev, cont))
    nw = len(kind) // 64
    lens = np.array(kind_len)[kind]
    early = (dev < np.minimum(E, lens)) & (cont > 0)
    rider = ~(dev < np.minimum(E, lens)) & (lens > E)
    W = lambda x: x[:64 * nw].reshape(nw, 64)
    nat = np.where(W(early), W(cont), 0).max(1)
    has_rider = W(rider).any(1)
    own = up3(E - 1) * recheck_cost
    res = {"E": E, "waves": nw, "rider_lane_frac": float(rider.mean()), "waves_with_rider": float(has_rider.mean()),
           "natural_loop": {"mean": float(nat.mean()), "zero_frac": float((nat == 0).mean()),
                            "quantiles": {str(q): float(np.quantile(nat, q / 100.0)) for q in (5, 10, 25, 50, 75, 90, 100)},
                            "hist": {int(k): int(v) for k, v in enumerate(np.bincount(nat)) if v}},
           "step_valu": step_valu, "check_valu": check_valu, "ride": {}}
    for R in [0] + [r for r in Rs if r > 0]:
        other = np.array([3 + up3(int(max(l.max() - E - R, 0))) if l.max() > E + R else 0 for l in W(lens)], float)
        other0 = np.array([3 + up3(int(max(l.max() - E, 0))) if l.max() > E else 0 for l in W(lens)], float)
        added = np.where(has_rider, np.maximum(0, R - nat), 0) if R else np.zeros(nw)
        loop = nat + added
        # the lanes that continue but not from below E start at the join: the loop has ended and the
        # other wave, which runs beside the path wave's own part, has raised its flag
        mid = W(~early & (cont > 0) & (dev < E + R)) if R else np.zeros((nw, 64), bool)
        late = W(~early & (cont > 0)) & ~mid
        mid_end = own + np.where(mid, W(dev) - E + W(cont), 0).max(1)
        flag = other * recheck_cost
        join = np.maximum(own + loop, flag)
        late_end = np.where(late.any(1), join + np.where(late, W(cont), 0).max(1), 0)
        chain = np.maximum(np.maximum(join, mid_end), late_end)  # (the wave always waits for the flag)
        res["ride"][int(R)] = {
            "waves_loop_shorter_than_R": float((has_rider & (nat < R)).mean()),
            "added_passes_mean": float(added.mean()), "added_passes_total": int(added.sum()),
            "saved_steps_mean": float((other0 - other).mean()),
            "valu_per_wave_pair": float((added * step_valu - (other0 - other) * check_valu).mean()),
            "chain_mean": float(chain.mean()), "chain_p90": float(np.quantile(chain, 0.9)), "chain_max": float(chain.max()),
        }
    return res


def spec_iterations(steps, mode="worse"):
    """Wave-loop passes a lane needs for `steps` (log entries) when every pass evaluates the step's
    probe AND, speculatively, the next step's probe under the assumption that this step's new probe
    is "plain worse" (not better, no nfc / fulc update: the next probe then depends on the bracket
    alone); a pass whose assumption holds completes two steps."""
    it = k = 0
    prev_better = False
    while k < len(steps):
        par, le, pw, ok, bg = steps[k]
        it += 1
        w_hit = ok and pw
        b_hit = bg
        if mode == "worse":
            hit = w_hit
        elif mode == "better":
            hit = b_hit
        elif mode == "predict":   # the previous step's outcome picks the speculation
            hit = b_hit if prev_better else w_hit
        else:                     # both (three probes per pass)
            hit = w_hit or b_hit
        hit = hit and k + 1 < len(steps)
        prev_better = steps[k + 1][1] if hit else le
        k += 2 if hit else 1
    return it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenario", default="corridor")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--early", type=int, nargs="+", metavar="E", default=None,
                    help="early start of the continuation: the dev histogram of the continuing lanes, the dev of "
                         "each wave's longest lane, continuation length by dev class and the modelled chain for "
                         "today's split and for each E")
    ap.add_argument("--ride", type=int, nargs="+", metavar="R", default=None,
                    help="table followers riding the continuation loop (early start at --ride-early): each "
                         "wave's natural loop length, and for each R the passes riders add where it is shorter "
                         "than R, the re-check steps the other wave drops and the modelled chain")
    ap.add_argument("--ride-early", type=int, default=16, help="E of --ride (BT_EARLY)")
    ap.add_argument("--recheck-cost", type=float, default=0.125,
                    help="a table re-check step in continuation steps (~45 VALU against a 1.65-2.0 k cycle brent_step)")
    args = ap.parse_args()

    import oracle

    import drone2d_amd  # noqa: F401
    from drone2d_amd.config import ENV_TRAIN_CONFIG, make_cfg
    from drone2d_amd.env import build_scenarios

    kw = dict(ENV_TRAIN_CONFIG, scenario=args.scenario)
    scn = build_scenarios(kw)[0]
    sc = scn.to_c()
    b = oracle.OracleBatch(make_cfg(dict(kw)), [sc], args.envs)
    b.reset(12345)
    rng = np.random.default_rng(1000)
    for _ in range(args.warmup):
        b.step(rng.uniform(-1, 1, (args.envs, 2)).astype(np.float32), nthreads=8)
    st, _ = b.get_state()
    px, py = st[0], st[1]
    L = float(scn.path.length)

    kind_len = [forced_len(L, 0), forced_len(L, 1)]
    rows = []
    for i in range(args.envs):
        _, log = fminbound_log(dist_to(sc, (px[i], py[i])), -10.0, L + 10.0)
        kind, dev = table_dev(log, kind_len)
        cont = log[dev:] if dev < len(log) else []
        # trailing run of golden-worse steps in the continuation
        tail = 0
        for par, le, *_ in reversed(cont):
            if par or le:
                break
            tail += 1
        rows.append(dict(n=len(log), kind=kind, dev=dev, cont=len(cont), tail=tail,
                         par=sum(x[0] for x in cont), gw=sum((not x[0]) and (not x[1]) for x in cont),
                         **{f"cont_{m}": spec_iterations(cont, m) for m in ("worse", "better", "predict", "both")},
                         **{f"full_{m}": spec_iterations(log, m) for m in ("worse", "better", "predict", "both")}))
    C = np.array([r["cont"] for r in rows])
    T = np.array([r["tail"] for r in rows])
    waves = C.reshape(-1, 64)
    tails = T.reshape(-1, 64)
    lanes = (waves > 0).sum(1)
    wmax = waves.max(1)
    wsum = waves.sum(1)
    # alternatives (wave-steps of continuation per 64 envs)
    pair_max = np.maximum(waves[0::2].max(1), waves[1::2].max(1))  # two waves pooled -> one (if <= 64 lanes)
    pooled_ok = (lanes[0::2] + lanes[1::2]) <= 64
    # pooled with refill (lanes pull the next search when done): ~max(longest, ceil(sum / 64))
    refill = np.maximum(pair_max, np.ceil((wsum[0::2] + wsum[1::2]) / 64.0))
    notail = (waves - tails).max(1)
    res = {
        "scenario": args.scenario, "envs": args.envs, "warmup": args.warmup, "table_len": kind_len,
        "steps_mean": float(np.mean([r["n"] for r in rows])), "steps_max": int(max(r["n"] for r in rows)),
        "kind0_frac": float(np.mean([r["kind"] == 0 for r in rows])),
        "dev_mean": float(np.mean([r["dev"] for r in rows])),
        "cont_lane_frac": float((C > 0).mean()), "cont_mean_active": float(C[C > 0].mean()) if (C > 0).any() else 0.0,
        "wave_cont_max_mean": float(wmax.mean()), "wave_cont_lanes_mean": float(lanes.mean()),
        "lane_util": float(wsum.sum() / (64.0 * wmax.sum())),
        "pooled_two_waves_wave_steps_per_64": float(pair_max.mean() / 2), "pooled_fits_64_frac": float(pooled_ok.mean()),
        "pooled_refill_wave_steps_per_64": float(refill.mean() / 2),
        "tail_mean_active": float(T[C > 0].mean()) if (C > 0).any() else 0.0,
        "wave_max_without_golden_tail": float(notail.mean()),
        "par_frac_of_cont": float(sum(r["par"] for r in rows) / max(1, C.sum())),
        "golden_worse_frac_of_cont": float(sum(r["gw"] for r in rows) / max(1, C.sum())),
        # speculative next-probe evaluation (spec_iterations): wave-max passes of the continuation
        # (tables) and of the whole search (no tables: the fresh curriculum's plain search)
        "wave_full_max_mean": float(np.array([r["n"] for r in rows]).reshape(-1, 64).max(1).mean()),
        **{f"wave_{p}_max_spec_{m}": float(np.array([r[f"{p}_{m}"] for r in rows]).reshape(-1, 64).max(1).mean())
           for p in ("cont", "full") for m in ("worse", "better", "predict", "both")},
    }
    if args.early:
        res["early_start"] = early_report([r["kind"] for r in rows], [r["dev"] for r in rows], C, kind_len, args.early,
                                          args.recheck_cost)
    if args.ride:
        res["ride"] = ride_report([r["kind"] for r in rows], [r["dev"] for r in rows], C, kind_len, args.ride_early,
                                  args.ride, args.recheck_cost)
    print(json.dumps(res, indent=1))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
