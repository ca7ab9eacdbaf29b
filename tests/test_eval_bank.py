"""The policy bank without a GPU: the ``d2d_eval_bank`` struct against the header, ``PolicyBank`` packing,
``sweep_layout``, the host's refusal of a bad env -> policy map, ``evaluate_policies`` on the CPU oracle
backend (``BankActor`` through ``harness.run_first_episodes``; one process and two gloo ranks) and the
selection table."""
import csv
import ctypes as C
import json
import os
import pickle
import re
import socket

import numpy as np
import pytest
import torch

from bank_util import AGENT, make_policies
from oracle_backend import OracleVecBackend

HERE = os.path.dirname(os.path.abspath(__file__))
SCN = ["corridor", "large"]
P, S, R, MAX_STEPS, SEED = 3, 2, 4, 80, 3


def _kw():
    from drone2d_amd.config import ENV_TEST_CONFIG

    return dict(ENV_TEST_CONFIG, scenario=SCN)


def _same(m, ref):
    assert set(m) == set(ref)
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(m[k], v, err_msg=k)  # NaN == NaN here
        else:
            assert m[k] == v, k


def test_bank_struct_matches_header(d2):
    """The ctypes struct has the header's fields in the header's order, 24 bytes, and the stride and
    version constants are the header's."""
    from drone2d_amd import evaluate

    hdr = open(os.path.join(HERE, "..", "include", "d2d_eval.h")).read()
    body = hdr[hdr.index("typedef struct d2d_eval_bank {"):hdr.index("} d2d_eval_bank;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+);", body)
    assert names == [f[0] for f in evaluate.D2DEvalBank._fields_] == ["n_policies", "pad", "params", "env_policy"]
    assert C.sizeof(evaluate.D2DEvalBank) == 24
    assert evaluate.D2DEvalBank.params.offset == 8 and evaluate.D2DEvalBank.env_policy.offset == 16
    assert re.search(rf"#define D2D_EVAL_BANK_STRIDE\s+{evaluate.BANK_STRIDE}\b", hdr)
    assert re.search(rf"#define D2D_EVAL_BANK_VERSION\s+{evaluate.BANK_VERSION}\b", hdr)
    assert evaluate.BANK_STRIDE == 64 * 27 + 64 + 64 * 64 + 64 + 2 * 64 + 2 + 2 == 6084
    assert {"d2d_eval_bank_version", "d2d_eval_step_bank"} <= set(evaluate.SIGNATURES)
    # the old entry point and struct are what they were
    assert f"#define D2D_EVAL_ABI_VERSION {evaluate.ABI_VERSION}" in hdr and evaluate.ABI_VERSION == 1
    assert C.sizeof(evaluate.D2DEvalStepArgs) == 6 * 4 + 2 * 8 + 19 * 8


def test_policy_bank_packing(d2, tmp_path):
    """Every slice of the [P, 6084] tensor equals ``actor_tensors`` of its policy, whatever the policy
    was given as; a 27-32-32-2 actor is refused."""
    from drone2d_amd import agent_io, evaluate, harness
    from drone2d_amd.ppo import PPO, ActorCritic, PPOConfig

    pol = make_policies()
    be = OracleVecBackend(8, seed=3, **dict(_kw(), scenario="corridor"))
    algo = PPO(be, PPOConfig(n_steps=8, batch_size=64, n_epochs=1), policy=pol["perturbed"], seed=0, device="cpu")
    saved = algo.save(str(tmp_path / "rl_model_64_steps.zip"))
    be.close()
    written = agent_io.write_agent(str(tmp_path / "fresh.zip"), {"format_version": agent_io.AGENT_FORMAT_VERSION},
                                   {"policy.pth": pol["fresh"].state_dict(), "train_state.pth": {}})
    entries = [pol["fresh"], harness.MlpActor.from_npz(AGENT), saved, written, ActorCritic.from_agent_npz(AGENT), algo]
    expect = [pol["fresh"], pol["shipped"], pol["perturbed"], pol["fresh"], pol["shipped"], pol["perturbed"]]
    bank = evaluate.PolicyBank(entries, device="cpu")
    assert bank.params.shape == (6, evaluate.BANK_STRIDE) and bank.params.dtype == torch.float32
    assert bank.params.is_contiguous() and bank.n_policies == len(bank) == 6
    assert bank.names == ["policy_0", "policy_1", "rl_model_64_steps", "fresh", "policy_4", "policy_5"]
    for p, ref in enumerate(expect):
        want = evaluate.actor_tensors(ref, "cpu")
        got = bank.tensors(p)
        assert len(got) == 7
        for g, w in zip(got, want):
            assert g.shape == w.shape and torch.equal(g, w)
        # the header's order: the row is the seven tensors laid end to end
        assert torch.equal(bank.params[p], torch.cat([w.reshape(-1) for w in want]))
        # views, not copies
        assert got[0].data_ptr() == bank.params[p].data_ptr()
    assert not torch.equal(bank.params[0], bank.params[1])
    named = evaluate.PolicyBank([pol["fresh"], pol["shipped"]], names=["a", "b"], device="cpu")
    assert named.names == ["a", "b"]
    actor = named.mlp_actor(1, batch_invariant=True)
    obs = torch.randn(5, 27, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        assert torch.equal(actor(obs), harness.MlpActor.from_npz(AGENT, batch_invariant=True)(obs))
    with pytest.raises(ValueError, match="27-64-64-2"):
        evaluate.PolicyBank([pol["fresh"], ActorCritic(hidden=32)], device="cpu")
    with pytest.raises(ValueError):
        evaluate.PolicyBank([pol["fresh"], pol["shipped"]], names=["a", "a"], device="cpu")
    with pytest.raises(ValueError):
        evaluate.PolicyBank([], device="cpu")


def test_sweep_layout(d2):
    from drone2d_amd.evaluate import sweep_layout

    for p, s, r in ((3, 7, 24), (1, 1, 1), (16, 7, 128), (2, 2, 64)):
        ep, es = sweep_layout(p, s, r)
        assert ep.shape == es.shape == (p * s * r,) and ep.dtype == es.dtype == np.int32
        pairs, counts = np.unique(np.stack([ep, es], 1), axis=0, return_counts=True)
        assert len(pairs) == p * s and (counts == r).all()  # every (policy, scenario) pair exactly `runs` times
        assert (np.diff(ep) >= 0).all() and (np.bincount(ep) == s * r).all()  # policy blocks contiguous
        blk = es.reshape(p, s * r)
        assert (blk == blk[0]).all() and (np.diff(blk[0]) >= 0).all()  # then scenario, then run
    with pytest.raises(ValueError):
        sweep_layout(0, 1, 1)


def test_env_policy_is_checked_on_the_host(d2):
    """Wrong length, a negative id, id = P and a float map each raise ValueError before any step."""
    from drone2d_amd import evaluate

    bank = evaluate.PolicyBank(list(make_policies().values()), device="cpu")

    class NeverStepped(OracleVecBackend):
        def reset(self, *a, **k):
            raise AssertionError("the map is checked before the batch is touched")

    be = NeverStepped(6, seed=1, **_kw())
    good = np.array([0, 1, 2, 0, 1, 2])
    for bad in (good[:5], np.append(good, 0), np.array([0, 1, -1, 0, 1, 2]), np.array([0, 1, 3, 0, 1, 2]),
                good.astype(np.float32), good.reshape(2, 3)):
        with pytest.raises(ValueError):
            evaluate.evaluate_policies(be, bank, bad)
        with pytest.raises(ValueError):
            evaluate.check_env_policy(bad, 6, 3)
    with pytest.raises(ValueError):
        evaluate.evaluate_policies(be, bank, good, split=np.zeros(5, np.int64))
    be.close()
    ok = evaluate.check_env_policy(torch.tensor([2, 0, 1]), 3, 3)
    assert ok.dtype == np.int32 and ok.tolist() == [2, 0, 1]
    with pytest.raises(ValueError):
        evaluate.BankActor(bank, [0, 3])


def _bank_run(rank=0, world=1):
    """evaluate_policies on this rank's shard of the 3 x 2 x 4 oracle batch."""
    from drone2d_amd import evaluate, shard

    bank = evaluate.PolicyBank(list(make_policies().values()), names=["shipped", "perturbed", "fresh"], device="cpu")
    ep, es = evaluate.sweep_layout(P, S, R)
    off, cnt = shard.shard_range(P * S * R, world, rank)
    be = OracleVecBackend(cnt, seed=SEED, env_scenario=es[off:off + cnt], env_id_offset=off, **_kw())
    res = evaluate.evaluate_policies(be, bank, ep[off:off + cnt], split=es[off:off + cnt], seed=SEED,
                                     max_steps=MAX_STEPS, flight_paths=True)
    be.close()
    return res


@pytest.fixture(scope="module")
def bank_results(d2):
    return _bank_run()


def test_bank_actor_on_oracle_backend(d2, bank_results):
    """The split results equal the records of run_first_episodes under each policy alone
    (batch_invariant), at that policy's env indices, bit for bit."""
    from drone2d_amd import evaluate, harness

    ep, es = evaluate.sweep_layout(P, S, R)
    assert sorted(bank_results) == [(p, s) for p in range(P) for s in range(S)]
    finished = 0
    for p, pol in enumerate(make_policies().values()):
        be = OracleVecBackend(P * S * R, seed=SEED, env_scenario=es, **_kw())
        raw = harness.run_first_episodes(be, evaluate.as_mlp_actor(pol, batch_invariant=True), seed=SEED,
                                         max_steps=MAX_STEPS, flight_paths=True, records=False)
        for s in range(S):
            idx = np.flatnonzero((ep == p) & (es == s))
            ref = evaluate._records(be, raw["finished"][idx], raw["rows"][idx], raw["xy"][:, idx], raw["n_obstacles"])
            _same(bank_results[(p, s)], ref)
            assert ref["unfinished"] + len(ref["time_spent"]) == R
            finished += len(ref["time_spent"])
        be.close()
    assert finished > 0  # some episodes ended within max_steps: the records are not all empty
    # without a split: one dict per policy, the same episodes
    be = OracleVecBackend(P * S * R, seed=SEED, env_scenario=es, **_kw())
    per_policy = evaluate.evaluate_policies(be, list(make_policies().values()), ep, seed=SEED, max_steps=MAX_STEPS)
    be.close()
    assert isinstance(per_policy, list) and len(per_policy) == P
    for p, m in enumerate(per_policy):
        np.testing.assert_array_equal(m["time_spent"], np.concatenate([bank_results[(p, s)]["time_spent"]
                                                                       for s in range(S)]))
        assert m["unfinished"] == sum(bank_results[(p, s)]["unfinished"] for s in range(S))


def _worker(rank, world, port, out_dir):
    import sys

    for p in (HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist

    import drone2d_amd  # noqa: F401
    from drone2d_amd import shard

    shard.init_process_group_from_env("gloo")
    res = _bank_run(rank, world)
    if rank == 0:
        with open(os.path.join(out_dir, "rank0.pkl"), "wb") as f:
            pickle.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_bank_matches_one_process(d2, bank_results, tmp_path):
    """Every rank passes its slice of the map; rank 0's gathered, split results are the one-process run's."""
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    with open(tmp_path / "rank0.pkl", "rb") as f:
        got = pickle.load(f)
    assert sorted(got) == sorted(bank_results)
    for k, ref in bank_results.items():
        _same(got[k], ref)


def _synthetic(successes, fails, collisions, apes, times):
    return {"successes": successes, "fails": fails, "collisions": np.array(collisions, np.int64),
            "apes": np.array(apes, np.float64), "time_spent": np.array(times, np.int64),
            "rewards": np.zeros(len(times)), "unfinished": 0}


def test_selection_table_and_files(d2, tmp_path):
    from drone2d_amd import harness

    results = {"rl_model_100_steps": {"corridor": _synthetic(3, 1, [0, 1, 0, 0], [1.0, 2.0, 3.0, 6.0], [10, 20, 30, 40]),
                                      "large": _synthetic(0, 0, [], [], [])},
               "rl_model_200_steps": {"corridor": _synthetic(1, 1, [1, 1], [0.5, 1.5], [7, 9]),
                                      "large": _synthetic(2, 0, [0, 0], [4.0, 4.0], [100, 300])}}
    rows = harness.selection_table(results)
    assert [r[:3] for r in rows] == [("rl_model_100_steps", "corridor", 4), ("rl_model_100_steps", "large", 0),
                                     ("rl_model_200_steps", "corridor", 2), ("rl_model_200_steps", "large", 2)]
    for r in rows:
        s = harness.summary(results[r[0]][r[1]])
        want = (s["Success rate"], s["Collision rate"], s["Average APE"], s["Average flight time"])
        np.testing.assert_array_equal(np.array(r[3:], np.float64), np.array(want, np.float64))  # NaN == NaN
    assert rows[0][3:] == (0.75, 0.25, 3.0, 25.0)
    assert rows[1][3] == 0.0 and rows[1][4] == 0.0 and np.isnan(rows[1][5]) and np.isnan(rows[1][6])
    written = harness.write_selection(results, str(tmp_path / "sel"))
    assert len(written) == 4 and written[0] == rows[0] and written[3] == rows[3]
    with open(tmp_path / "sel" / "selection.csv", newline="") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == harness.SELECTION_COLUMNS and len(lines) == 5
    for line, r in zip(lines[1:], rows):
        assert line[:2] == list(r[:2]) and int(line[2]) == r[2]
        np.testing.assert_array_equal(np.array([float(v) for v in line[3:]]), np.array(r[3:], np.float64))
    back = json.load(open(tmp_path / "sel" / "selection.json"))
    assert [tuple(d) for d in back] == [harness.SELECTION_COLUMNS] * 4
    assert back[0] == dict(zip(harness.SELECTION_COLUMNS, rows[0]))
    assert back[1]["episodes"] == 0 and back[1]["average_ape"] is None and back[1]["average_flight_time"] is None
