"""The episode monitor over two ranks on CPU (gloo, world size 2, the C oracle as each rank's env
shard, as in test_multi_rank.py): ``flush(reduce=True)`` SUM-reduces the flushed vector, and the result
is the unsharded batch's -- the counts exactly, the float columns to the rounding of another order."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

N_TOTAL = 301          # odd on purpose: uneven shards
STEPS = 120
SCN = ["corridor", "S_corridor", "large", "parallel", "perpendicular", "S_parallel", "impossible"]


def _kw():
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, scenario=SCN)


def _actions():
    return np.random.default_rng(11).uniform(-1, 1, (STEPS, N_TOTAL, 2)).astype(np.float32)


def _run(backend, acts, reduce):
    """Step, digest, flush once in the middle and once at the end; (sum of the two flushes, events)."""
    from drone2d_amd.monitor import K, EpisodeMonitor

    mon = EpisodeMonitor(backend)
    backend.reset()
    total, events = torch.zeros(K, dtype=torch.float64), []
    for t in range(STEPS):
        _, _, term, trunc, info = backend.step(torch.from_numpy(acts[t]))
        ev = mon._host.step(term.numpy(), trunc.numpy(), info.numpy())
        if ev is not None:
            events.append(ev[1])
        if t in (STEPS // 2, STEPS - 1):
            total += mon.flush(reduce=reduce)
    return total, np.concatenate(events)


def _worker(rank, world, port, out_dir):
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import drone2d_amd  # noqa: F401
    from drone2d_amd import shard
    from oracle_backend import OracleVecBackend

    shard.init_process_group_from_env("gloo")
    off, cnt = shard.shard_range(N_TOTAL, world, rank)
    es = shard.shard_env_scenario(shard.global_env_scenario(N_TOTAL, len(SCN)), off, cnt)
    be = OracleVecBackend(cnt, seed=21, env_scenario=es, env_id_offset=off, **_kw())
    total, _ = _run(be, _actions()[:, off:off + cnt], reduce=True)
    torch.save(total, os.path.join(out_dir, f"monitor_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
    be.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_reduced_monitor_matches_single_batch(tmp_path, d2):
    from drone2d_amd import abi
    from drone2d_amd import monitor as M
    from oracle_backend import OracleVecBackend

    world = 2
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    got = [torch.load(os.path.join(tmp_path, f"monitor_{r}.pt"), weights_only=True).numpy() for r in range(world)]
    assert np.array_equal(got[0], got[1])  # every rank holds the reduced vector

    single = OracleVecBackend(N_TOTAL, seed=21, **_kw())
    want, events = _run(single, _actions(), reduce=False)
    stats = single.episode_stats().numpy()
    single.close()
    want = want.numpy()
    counts = [M.EPISODES, M.SUCCESS, M.FAIL, M.COLLISION, M.TIMEUP, M.AA, M.LEN, M.MINCLR_N, M.SKIPPED]
    np.testing.assert_array_equal(got[0][counts], want[counts])
    assert want[M.EPISODES] == stats[abi.ST_EPISODES] == len(events) and want[M.EPISODES] > 100
    # the same float32-derived terms in another order: within the bound of the rollout tests, 2^-23 sum |x|
    bound = 2.0 ** -23 * np.abs(events).sum(0)
    assert np.isfinite(want).all() and (np.abs(got[0] - want) <= bound).all()
