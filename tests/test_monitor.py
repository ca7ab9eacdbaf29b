"""The episode monitor and the training logs without a GPU: ``monitor_host`` (the NumPy twin of
libd2d_monitor.so, include/d2d_monitor.h) on hand-made rows and on an oracle-backend rollout against
``episode_stats()``, ``PPO.learn(monitor=...)`` on the oracle backend, and ``trainlog``'s writers."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from oracle_backend import OracleVecBackend

INF, NAN = float("inf"), float("nan")
CANONICAL_NAN = 0x7FF8000000000000


def _row(terms=(0, 0, 0, 0, 0, 0), dclose=INF, steps=0, cause=0, ape=0.0, totrew=0.0, reward=0.0):
    return list(terms) + [dclose, steps, cause, ape, totrew, reward]


def _step(mon, rows, done):
    info = np.array(rows, np.float32)
    d = np.array(done, np.uint8)
    return mon.step(d, np.zeros_like(d), info)


def test_twin_every_cause_combination_and_a_skipped_episode(d2):
    """One step, 16 envs: env i < 15 ends with cause bits i + 1 (all 15 combinations of collision 1,
    reach 2, time-up 4, aggressive alpha 8); env 15 ends an episode the monitor did not see start."""
    from drone2d_amd import monitor as M

    mon = M.monitor_host(16)
    mon.live[15] = 0
    rows = []
    for i in range(16):
        c = i + 1 if i < 15 else 1
        rows.append(_row((0.5, -0.25, 1.0, -2.0 if c & 1 else 0.0, 4.0 if c & 2 else 0.0, -0.5 if c & 8 else 0.0),
                         dclose=10 + i, steps=100 + i, cause=c, ape=2.0, totrew=i, reward=0.125))
    _step(mon, rows, [1] * 16)
    v = mon.flush()
    assert v[M.EPISODES] == 15 and v[M.SKIPPED] == 1
    # the overwrite order of drone_2d_env.py:595-610: success = reach (2 3 6 7 10 11 14 15); fail = any of
    # collision / time-up / AA (all but cause 2); a collision counts only when nothing overwrote it (cause 1)
    assert v[M.SUCCESS] == 8 and v[M.FAIL] == 14 and v[M.COLLISION] == 1
    assert v[M.TIMEUP] == 8 and v[M.AA] == 8
    assert v[M.LEN] == 1605 and v[M.TOTREW] == 105 and v[M.APE] == 30
    want = [7.5, -3.75, 15.0, -16.0, 32.0, -4.0]  # 15 episodes; 8 odd causes, 8 with bit 2, 8 with bit 8
    assert list(v[M.RUN:M.RUN + 6]) == want and list(v[M.LAST:M.LAST + 6]) == want
    assert v[M.LAST_REWARD] == 1.875 and v[M.MINCLR] == 255 and v[M.MINCLR_N] == 15
    # the skipped env deposited nothing and is live from now on
    assert mon.live.all() and not mon.run.any() and np.isinf(mon.minclr).all()
    assert not mon.flush().any()


def test_twin_two_episodes_of_one_env_in_one_window(d2):
    from drone2d_amd import monitor as M

    mon = M.monitor_host(2)
    _step(mon, [_row((1, 0, 0, 0, 0, 0), dclose=5), _row((0, 2, 0, 0, 0, 0))], [0, 0])
    ev = _step(mon, [_row((0.5, 0, 0, 0, 0, 0), dclose=3, steps=2, cause=8, ape=0.25, totrew=1.5, reward=0.5),
                     _row((0, 2, 0, 0, 0, 0))], [1, 0])
    assert list(ev[0]) == [0] and ev[1][0, M.RUN] == 1.5
    _step(mon, [_row((0.25, 0, 0, 0, 0, 0), dclose=7, steps=1, cause=2, ape=0.5, totrew=0.25, reward=0.25),
                _row((0, 2, 0, 0, 0, 0), steps=3, cause=4, ape=1.0, totrew=6.0, reward=2.0)], [1, 1])
    v = mon.flush()
    assert v[M.EPISODES] == 3 and v[M.SUCCESS] == 1 and v[M.FAIL] == 2 and v[M.COLLISION] == 0
    assert v[M.TIMEUP] == 1 and v[M.AA] == 1 and v[M.SKIPPED] == 0
    assert v[M.LEN] == 6 and v[M.TOTREW] == 7.75 and v[M.APE] == 1.75
    assert v[M.RUN] == 1.75 and v[M.RUN + 1] == 6.0           # episode sums: 1.5, 0.25 | 6
    assert v[M.LAST] == 0.75 and v[M.LAST + 1] == 2.0         # terminal steps: 0.5, 0.25 | 2
    assert v[M.LAST_REWARD] == 2.75
    assert v[M.MINCLR] == 10 and v[M.MINCLR_N] == 2           # min(5, 3), 7; env 1 never saw an obstacle


def test_twin_inf_and_nan_rows(d2):
    """IEEE specials pass through; a NaN comes out of flush as the canonical quiet NaN, whatever its
    sign (x86 gives inf - inf the sign bit); a NaN clearance is ignored."""
    from drone2d_amd import monitor as M

    mon = M.monitor_host(3)
    _step(mon, [_row((-INF, 0, 0, 0, 0, 0), dclose=NAN), _row((1, 0, 0, 0, 0, 0)), _row((0, -INF, 0, 0, 0, 0))],
          [0, 0, 0])
    _step(mon, [_row((INF, 1, 0, 0, 0, 0), dclose=4, steps=2, cause=1, totrew=NAN),
                _row((1, 0, 0, 0, 0, 0), steps=2, cause=1, totrew=2), _row((0, 0, 0, 0, 0, 0), steps=2, cause=8)],
          [1, 1, 1])
    v = mon.flush()
    bits = v.view(np.int64)
    assert v[M.EPISODES] == 3
    assert bits[M.RUN] == CANONICAL_NAN and bits[M.TOTREW] == CANONICAL_NAN   # -inf + inf (+ 2); NaN + 2
    assert v[M.LAST] == INF and v[M.RUN + 1] == -INF and v[M.LAST + 1] == 1.0
    assert v[M.MINCLR] == 4 and v[M.MINCLR_N] == 1
    assert np.isfinite(np.delete(v, [M.RUN, M.TOTREW, M.LAST, M.RUN + 1])).all()


def test_twin_summation_order(d2):
    """Ascending lanes within a wave, then waves, then the row's chunks in walk order, then rows: each
    pair below gives 0 in the stated order and 1 in the other."""
    from drone2d_amd import monitor as M

    big = 2.0 ** 60

    def run(n, n_blocks, where):
        mon = M.monitor_host(n, n_blocks)
        rows = [_row() for _ in range(n)]
        done = [0] * n
        for i, x in where.items():
            rows[i] = _row(cause=1, steps=1, totrew=0.0, ape=x)
            done[i] = 1
        # float32 holds 2^60 and 1 exactly
        _step(mon, rows, done)
        return mon.flush()[M.APE]

    assert run(64, 1, {3: big, 17: 1.0, 40: -big}) == 0.0          # lanes: (big + 1) - big
    assert run(64, 1, {3: big, 17: -big, 40: 1.0}) == 1.0
    assert run(256, 1, {0: big, 70: 1.0, 130: -big}) == 0.0        # waves 0, 1, 2 of one chunk
    assert run(256, 1, {0: big, 70: -big, 130: 1.0}) == 1.0
    assert run(600, 1, {0: big, 300: 1.0, 599: -big}) == 0.0       # one row walks chunks 0, 1, 2
    assert run(600, 2, {0: big, 300: 1.0, 599: -big}) == 1.0       # rows {0, 2} and {1}: (big - big) + 1
    assert run(600, 3, {0: big, 300: 1.0, 599: -big}) == 0.0       # rows 0, 1, 2 in flush order


@pytest.mark.parametrize("n", [64, 65, 255, 256, 257, 1000])
def test_gpu_synthetic_rows_are_order_sensitive(d2, n):
    """The synthetic rows that tests/test_gpu_monitor.py compares the device on tell summation orders
    apart (lanes, waves, the chunk walk): checked on the twin, so without a GPU too."""
    import test_gpu_monitor as G

    G.check_order_sensitive(n)


def test_monitor_arguments(d2):
    from drone2d_amd import monitor as M

    with pytest.raises(ValueError):
        M.monitor_host(8, 0)
    with pytest.raises(ValueError):
        M.monitor_host(8, 1025)
    mon = M.EpisodeMonitor(8, "cpu")
    assert mon.n_blocks == 1 and M.default_blocks(257) == 2 and M.default_blocks(10 ** 6) == 1024
    with pytest.raises(ValueError):
        mon.step(torch.zeros(8, dtype=torch.bool), torch.zeros(8, dtype=torch.bool), torch.zeros(8, 11))
    with pytest.raises(ValueError):
        mon.step(torch.zeros(8, dtype=torch.bool), torch.zeros(8, dtype=torch.bool), None)


def test_step_args_struct_matches_header(d2, tmp_path):
    """The ctypes mirror against a compiled probe of include/d2d_monitor.h (sizes, offsets, K)."""
    import ctypes as C
    import subprocess

    from drone2d_amd import monitor as M

    cc = "gcc"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in M.D2DMonitorStepArgs._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "d2d_monitor.h"\n#include "drone2d.h"\nint main(void){'
                   'printf("%zu %d %d %d %d %d %d", sizeof(d2d_monitor_step_args), D2D_MON_K, D2D_MON_RUN, D2D_MON_LAST,'
                   ' D2D_MON_SKIPPED, D2D_MON_ABI_VERSION, D2D_INFO_DIM);'
                   + "".join(f'printf(" %zu", offsetof(d2d_monitor_step_args, {f}));' for f in fields) + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:7] == [C.sizeof(M.D2DMonitorStepArgs), M.K, M.RUN, M.LAST, M.SKIPPED, M.ABI_VERSION, 12]
    assert got[7:] == [getattr(M.D2DMonitorStepArgs, f).offset for f in fields]


# ------------------------------------------------------------------------------------- oracle rollout
N_ENVS, STEPS = 448, 1500


@pytest.fixture(scope="module")
def rollout(d2):
    """448 envs over the 7 test scenarios on the C oracle, clipped N(0, 0.25^2) actions, 1 500 steps,
    digested by an ``EpisodeMonitor`` on CPU tensors and flushed every 250 steps.  Kept: the sum of the
    flushes, every event vector, each episode's sum of |f32 term| over its steps (accumulated here, not
    by the monitor), the cause bits read from the info rows, and the env's own ``episode_stats()``."""
    from drone2d_amd import abi
    from drone2d_amd import monitor as M
    from drone2d_amd.config import ENV_TRAIN_CONFIG, TEST_SCENARIOS

    be = OracleVecBackend(N_ENVS, seed=7, **dict(ENV_TRAIN_CONFIG, scenario=list(TEST_SCENARIOS)))
    mon = M.EpisodeMonitor(be)
    assert not mon.hip
    be.reset()
    rng = np.random.default_rng(5)
    total = np.zeros(M.K)
    absrun = np.zeros(N_ENVS)
    events, abssum, causes = [], [], np.zeros(4, np.int64)
    for t in range(STEPS):
        a = np.clip(rng.normal(0.0, 0.25, (N_ENVS, 2)), -1.0, 1.0).astype(np.float32)
        _, _, term, trunc, info = be.step(torch.from_numpy(a))
        rows = info.numpy()
        absrun += np.abs(rows[:, :6].astype(np.float64)).sum(1)
        ev = mon._host.step(term.numpy(), trunc.numpy(), rows)
        if ev is not None:
            idx, vec = ev
            events.append(vec)
            abssum.append(absrun[idx].copy())
            absrun[idx] = 0.0
            c = rows[idx, abi.INFO_CAUSE].astype(np.int64)
            causes += [int(((c >> k) & 1).sum()) for k in range(4)]
        if t % 250 == 249:
            total += mon.flush().numpy()
    stats = be.episode_stats(clear=False).numpy().copy()
    be.close()
    return {"total": total, "events": np.concatenate(events), "abssum": np.concatenate(abssum), "causes": causes,
            "stats": stats}


def test_oracle_rollout_counts_equal_episode_stats(d2, rollout):
    """Counts and the length sum equal the env's accumulators exactly.  The return and APE sums: the
    monitor adds float32-rounded info values, the env float64 ones, so each term is off by at most
    2^-24 |x|; 2^-23 sum |x| leaves room for the float64 additions."""
    from drone2d_amd import abi
    from drone2d_amd import monitor as M

    v, st, ev = rollout["total"], rollout["stats"], rollout["events"]
    print("causes (collision, reach, time-up, AA):", rollout["causes"], "episodes:", v[M.EPISODES])
    assert (rollout["causes"] > 0).all(), "the rollout must hold every end cause"
    assert v[M.SKIPPED] == 0
    assert v[M.EPISODES] == st[abi.ST_EPISODES] == len(ev) and v[M.EPISODES] > 1000
    assert v[M.SUCCESS] == st[abi.ST_SUCCESS] and v[M.FAIL] == st[abi.ST_FAIL]
    assert v[M.COLLISION] == st[abi.ST_COLLISION] and v[M.LEN] == st[abi.ST_LEN]
    assert v[M.TIMEUP] == rollout["causes"][2] and v[M.AA] == rollout["causes"][3]
    for col, ref in ((M.TOTREW, abi.ST_RETURN), (M.APE, abi.ST_APE)):
        bound = 2.0 ** -23 * np.abs(ev[:, col]).sum()
        print("column", col, "monitor", v[col], "env", st[ref], "diff", abs(v[col] - st[ref]), "bound", bound)
        assert abs(v[col] - st[ref]) <= bound
    # the flushed sums are the events' sums (another order: float64 rounding only)
    np.testing.assert_allclose(v, ev.sum(0), rtol=1e-12)


def test_oracle_rollout_per_episode_terms_add_up(d2, rollout):
    """Every episode's six term sums add up to its INFO_TOTREW within 2^-23 (sum |terms| + |total|),
    sum |terms| over the episode's steps and terms: the env adds the float64 terms, the info row holds
    each rounded to float32 (error <= 2^-24 |term|), and the total itself is rounded once
    (<= 2^-24 |total|); the factor two covers the float64 additions."""
    from drone2d_amd import monitor as M

    ev, ab = rollout["events"], rollout["abssum"]
    got = ev[:, M.RUN:M.RUN + 6].sum(1)
    diff = np.abs(got - ev[:, M.TOTREW])
    bound = 2.0 ** -23 * (ab + np.abs(ev[:, M.TOTREW]))
    worst = int(np.argmax(diff / bound))
    print(f"{len(ev)} episodes, longest {ev[:, M.LEN].max():.0f}; worst |diff| {diff.max():.3g}, "
          f"worst diff / bound {diff[worst] / bound[worst]:.3g}")
    assert np.isfinite(got).all() and (diff <= bound).all()
    assert ev[:, M.LEN].max() >= 1000  # a time-up or a long flight is among them


# ------------------------------------------------------------------------------------------------ PPO
def _kw():
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, scenario="corridor")


def _ppo(be, seed=0):
    from drone2d_amd.ppo import PPO, PPOConfig

    return PPO(be, PPOConfig(n_steps=64, batch_size=256, n_epochs=2), seed=seed, device="cpu")


TIMING_KEYS = {"rollout_s", "train_s", "env_steps_per_s"}


def test_ppo_monitor_changes_nothing_and_adds_its_keys(d2, tmp_path):
    """Two updates with and without the monitor: parameters and Adam moments identical, the earlier
    record keys with the same values; then save + load: the first rollout's in-flight episodes are
    skipped, not deposited, so episodes + skipped is the rollout's finished-episode count."""
    from drone2d_amd.ppo import PPO

    be_a, be_b = (OracleVecBackend(32, seed=3, **_kw()) for _ in range(2))
    a, b = _ppo(be_a), _ppo(be_b)
    ha = a.learn(2 * 64 * 32)
    hb = b.learn(2 * 64 * 32, monitor=True)
    assert len(ha) == len(hb) == 2
    for (k, p), q in zip(a.policy.state_dict().items(), b.policy.state_dict().values()):
        assert torch.equal(p, q), k
    assert torch.equal(a.manual.m, b.manual.m) and torch.equal(a.manual.v, b.manual.v)
    assert torch.equal(a.manual.t, b.manual.t)
    for ra, rb in zip(ha, hb):
        assert set(ra) <= set(rb)
        for k, v in ra.items():
            if k not in TIMING_KEYS:
                assert rb[k] == v or (math.isnan(v) and math.isnan(rb[k])), k
        new = set(rb) - set(ra)
        assert "train/explained_variance" in new and all(k.startswith(("monitor/", "train/")) for k in new)
        assert rb["monitor/episodes"] == rb["episodes"] and rb["monitor/skipped"] == 0
        assert rb["monitor/rollout/ep_rew_mean"] == pytest.approx(rb["mean_return"], rel=1e-6)
        assert rb["train/explained_variance"] <= 1.0
    assert sum(r["episodes"] for r in hb) > 0
    path = b.save(str(tmp_path / "b.zip"))
    c = PPO.load(path, be_b, device="cpu")
    assert c.monitor is None
    rec = c.learn(3 * 64 * 32, monitor=True)[0]
    assert rec["monitor/episodes"] + rec["monitor/skipped"] == rec["episodes"]
    assert rec["monitor/skipped"] > 0  # 32 envs were in mid-episode; a 64-step rollout ends some of them
    be_a.close()
    be_b.close()


# --------------------------------------------------------------------------------------------- writers
def _read_varint(buf, o):
    n = s = 0
    while True:
        b = buf[o]
        o += 1
        n |= (b & 0x7F) << s
        s += 7
        if not b & 0x80:
            return n, o


def _fields(buf):
    """(field number, wire type, value) of one protobuf message."""
    o, out = 0, []
    while o < len(buf):
        key, o = _read_varint(buf, o)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, o = _read_varint(buf, o)
        elif wt == 1:
            v, o = buf[o:o + 8], o + 8
        elif wt == 2:
            n, o = _read_varint(buf, o)
            v, o = buf[o:o + n], o + n
        elif wt == 5:
            v, o = buf[o:o + 4], o + 4
        else:
            raise AssertionError(f"wire type {wt}")
        out.append((f, wt, v))
    return out


def _read_events(path, masked_crc):
    """The event file back as [(step, {tag: float32 value} or file_version)]; every CRC checked."""
    data = open(path, "rb").read()
    o, out = 0, []
    while o < len(data):
        head = data[o:o + 8]
        (n,) = struct.unpack("<Q", head)
        assert struct.unpack("<I", data[o + 8:o + 12])[0] == masked_crc(head)
        body = data[o + 12:o + 12 + n]
        assert struct.unpack("<I", data[o + 12 + n:o + 16 + n])[0] == masked_crc(body)
        o += 16 + n
        step, vals = 0, {}
        for f, wt, v in _fields(body):
            if f == 1:
                assert wt == 1 and struct.unpack("<d", v)[0] > 1.6e9  # wall time
            elif f == 2:
                step = v
            elif f == 3:
                vals = v.decode()
            elif f == 5:
                for _, _, val in _fields(v):
                    d = {ff: vv for ff, _, vv in _fields(val)}
                    vals[d[1].decode()] = struct.unpack("<f", d[2])[0]
        out.append((step, vals))
    return out


def test_crc32c_known_answer(d2):
    from drone2d_amd import trainlog

    assert trainlog.crc32c(b"123456789") == 0xE3069283
    assert trainlog.crc32c(b"") == 0
    assert trainlog.masked_crc(b"123456789") == (((0xE3069283 >> 15) | (0xE3069283 << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def test_scalar_log_files_round_trip(d2, tmp_path):
    from drone2d_amd import monitor as M
    from drone2d_amd import trainlog

    vec = np.zeros(M.K)
    vec[[M.EPISODES, M.SUCCESS, M.FAIL, M.COLLISION, M.AA, M.LEN, M.TOTREW]] = [4, 1, 3, 1, 2, 200, -50]
    vec[M.RUN:M.RUN + 6] = [-4, 8, 12, -30, 10, -2]
    vec[M.LAST:M.LAST + 6] = [-1, 0.5, 0.25, -30, 10, -2]
    vec[[M.LAST_REWARD, M.MINCLR, M.MINCLR_N]] = [-22.25, 90, 3]
    sc = M.scalars(vec)
    assert sc["episodes"] == 4 and sc["rollout/success_rate"] == 0.25 and sc["rollout/collision_rate"] == 0.25
    assert sc["rollout/aa_rate"] == 0.5 and sc["rollout/timeup_rate"] == 0 and sc["rollout/ep_len_mean"] == 50
    assert sc["rollout/ep_rew_mean"] == -12.5 and sc["rollout/min_clearance_mean"] == 30
    assert sc["return/path_progression"] == 3 and sc["episodes/avg_collision_reward"] == -7.5
    assert sc["episodes/avg_reward"] == -5.5625 and sc["episodes/avg_length"] == 50
    assert math.isnan(M.scalars(np.zeros(M.K))["rollout/ep_rew_mean"])

    recs = []
    for u in range(3):
        rec = {"episodes": 4.0, "mean_return": -12.5, "policy_loss": 0.01 * u, "value_loss": 3.0, "entropy": 2.8,
               "clip_fraction": 0.125, "timesteps": 1000 * (u + 1), "rollout_s": 0.1, "train_s": 0.2,
               "env_steps_per_s": 1e6 / 3}
        if u:  # the first record has no monitor keys: the CSV header grows
            rec.update({"monitor/" + k: v for k, v in sc.items()}, **{"train/explained_variance": -0.5})
        recs.append(rec)
    with trainlog.ScalarLog(str(tmp_path / "logs")) as log:
        log.write_configs({"scenario": "corridor"}, {"ent_coef": 0.01})
        for rec in recs:
            log.log(rec)
        ev_path, csv_path = log.event_path, log.csv_path
    assert os.path.basename(ev_path).startswith("events.out.tfevents.")
    assert open(tmp_path / "logs" / "env_train_config.txt").read() == str({"scenario": "corridor"})
    assert open(tmp_path / "logs" / "rl_config.txt").read() == str({"ent_coef": 0.01})

    want = [trainlog.record_scalars(r, 4.0 * (u + 1)) for u, r in enumerate(recs)]
    reference_keys = {"time/episodes", "episodes/avg_reward", "episodes/avg_length", "episodes/avg_collision_reward",
                      "episodes/avg_collision_avoidance_reward", "episodes/avg_path_adherence_reward",
                      "episodes/avg_path_progression_reward", "episodes/avg_reach_end_reward",
                      "episodes/avg_agressive_alpha_reward"}
    assert reference_keys <= set(want[1])
    assert {"rollout/ep_rew_mean", "rollout/ep_len_mean", "rollout/success_rate", "rollout/collision_rate",
            "rollout/timeup_rate", "rollout/aa_rate", "rollout/ape_mean", "rollout/min_clearance_mean",
            "return/collision_avoidance", "train/policy_loss", "train/explained_variance", "time/fps",
            "time/total_timesteps"} <= set(want[1])
    assert want[2]["time/episodes"] == 12 and want[0]["rollout/ep_rew_mean"] == -12.5

    events = _read_events(ev_path, trainlog.masked_crc)
    assert events[0] == (0, "brain.Event:2") and len(events) == 4
    for (step, vals), w, rec in zip(events[1:], want, recs):
        assert step == rec["timesteps"] and set(vals) == set(w)
        for k, x in w.items():
            f32 = struct.unpack("<f", struct.pack("<f", x))[0]
            assert vals[k] == f32 or (math.isnan(vals[k]) and math.isnan(f32)), k

    rows = trainlog.read_progress(csv_path)
    assert len(rows) == 3
    for row, w, rec in zip(rows, want, recs):
        assert row.pop("step") == rec["timesteps"]
        assert set(row) == set(w)
        for k, x in w.items():
            assert row[k] == x or (math.isnan(row[k]) and math.isnan(x)), k

    with trainlog.ScalarLog(str(tmp_path / "plain"), tensorboard=False) as log:
        log.log(recs[0])
    assert sorted(os.listdir(tmp_path / "plain")) == ["progress.csv"]

    # a window without an episode: its NaN means are empty cells and are left out of the event
    empty = dict(recs[1], episodes=0.0, mean_return=NAN)
    empty.update({"monitor/" + k: v for k, v in M.scalars(np.zeros(M.K)).items()})
    with trainlog.ScalarLog(str(tmp_path / "empty")) as log:
        log.log(empty)
        log.log(recs[2])
        ev_path, csv_path = log.event_path, log.csv_path
    events = _read_events(ev_path, trainlog.masked_crc)
    rows = trainlog.read_progress(csv_path)
    for vals in (events[1][1], rows[0]):
        assert "rollout/ep_rew_mean" not in vals and "return/collision" not in vals
        assert vals["rollout/episodes"] == 0 and vals["time/episodes"] == 0 and "train/value_loss" in vals
        assert not any(math.isnan(v) for v in vals.values())
    assert rows[1]["rollout/ep_rew_mean"] == -12.5 and events[2][1]["rollout/ep_rew_mean"] == -12.5
