"""libd2d_gif.so on the device: the kernels' bytes against the CPU twin's on the cases of tests/test_gif.py,
many streams at once, run-to-run identity, ``add`` inside a captured graph, and ``record_episodes`` against
``evaluate_policy`` and ``venv.render``."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gif import (COLOUR_COUNTS, case_any_colours, case_boxes, case_colours, case_nearest, case_noise,
                      case_one_colour, case_small, case_streams, case_sub_blocks, decode_gif, distinct_palette, parse_gif)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(d2):
    from drone2d_amd import gif

    return gif


def device_files(G, frames, palette, active=None, flush_every=16, runs=1):
    """Frames uint8 [T, K, H, W, 3] through a ``GifEncoder``: (files, inexact [K]) of each of ``runs`` passes
    over the same encoder (a later pass starts from the workspace the earlier one left)."""
    import torch

    dev = torch.device("cuda", 0)
    T, K = frames.shape[:2]
    enc = G.GifEncoder(dev, K, frames.shape[2:4], palette, flush_every=flush_every)
    fd = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    ad = torch.from_numpy(np.ascontiguousarray(active)).to(dev) if active is not None else None
    out = []
    for _ in range(runs):
        for t in range(T):
            enc.add(fd[t], None if ad is None else ad[t])
        inexact = enc.inexact
        out.append((enc.finish(), inexact))
    enc.close()
    return out


def same_as_twin(G, frames, palette, active=None, **kw):
    want = G.HostEncoder(frames.shape[1], frames.shape[2:4], palette)
    for t in range(frames.shape[0]):
        want.add(frames[t], None if active is None else active[t])
    want_inexact, want_files = want.inexact.copy(), want.finish()
    for files, inexact in device_files(G, frames, palette, active, **kw):
        assert inexact.tolist() == want_inexact.tolist()
        for k, (a, b) in enumerate(zip(files, want_files)):
            assert a == b, f"stream {k}: device {len(a)} bytes, twin {len(b)} bytes, first difference at " \
                           f"{next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))}"
    return want_files


def test_round_trip_cases_equal_the_twin(G):
    """Every case of tests/test_gif.py 1. but the large noise: 8 x 8, 37 x 53, the changed boxes, one colour,
    every colour count, the sub-block boundaries.  Two passes each: the second finds used dictionaries."""
    cases = [case_small(G, 8, 8), case_small(G, 37, 53), case_boxes()[:2], case_one_colour()]
    cases += [case_colours(n) for n in COLOUR_COUNTS]
    found, pal = case_sub_blocks(G)
    cases += [(idx, pal) for idx in found.values()]
    for idx, colours in cases:
        pal = G.Palette(colours)
        same_as_twin(G, pal.colours[idx][:, None], pal, runs=2)


def test_noise_beyond_the_dictionary_equals_the_twin(G):
    """255-colour noise at 512 x 512 (Clears inside every segment; the longest chunk the bound allows for)."""
    idx, colours = case_noise()
    pal = G.Palette(colours)
    files = same_as_twin(G, pal.colours[idx][:, None], pal)
    assert max(f["chunk_len"] for f in parse_gif(files[0])["frames"]) <= G.frame_cap(512)


def test_palettes_and_streams_equal_the_twin(G):
    """The nearest rule and its count, the uniform cube on arbitrary colours, and K = 3 under a changing
    ``active`` mask with a flush inside the sequence."""
    f, colours, want = case_nearest()
    same_as_twin(G, np.stack([f, f])[:, None], G.Palette(colours))
    same_as_twin(G, case_any_colours()[None], G.Palette.uniform())
    frames, colours, active = case_streams()
    files = same_as_twin(G, frames, G.Palette(colours), active, flush_every=3)
    for k in range(3):
        assert (decode_gif(files[k]) == frames[active[:, k], k]).all()


def test_many_streams(G):
    """K = max_streams = 80 (more one-wave workgroups than a CU holds at once) of 24 x 40 pixels, 5 frames,
    a random ``active`` mask: every stream's bytes are the twin's, which are those of that stream alone
    (tests/test_gif.py); and two passes give the same bytes."""
    rng = np.random.default_rng(8)
    K, T = 80, 5
    colours = distinct_palette(14, seed=2)
    idx = rng.integers(0, 14, (T, K, 24, 40)).astype(np.uint8)
    idx[2:] = idx[1]
    idx[2:, :, 3:17, 8:30] = rng.integers(0, 14, (T - 2, K, 14, 22))
    active = rng.random((T, K)) < 0.7
    active[0] = True
    same_as_twin(G, colours[idx], G.Palette(colours), active, runs=2)


def test_capacities_are_refused(G):
    """A ctx used beyond ``max_streams``, beyond its largest picture, with a chunk row shorter than the bound,
    and with another size while its GIFs are running: each is D2DG_E_ARG, nothing is launched and ``len`` keeps
    its bytes.  After ``d2dg_restart`` the other size is accepted."""
    import ctypes as C

    import torch

    dev = torch.device("cuda", 0)
    lib = G.load()
    enc = G.GifEncoder(dev, 2, (16, 24), G.Palette.model())  # ctx: 2 streams of up to 24 wide x 16 high
    cap = G.frame_cap((24, 24))
    frames = torch.zeros(3, 24, 24, 3, dtype=torch.uint8, device=dev)
    chunk = torch.zeros(3, cap, dtype=torch.uint8, device=dev)
    lens = torch.full((3,), -7, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def encode(k, w, h, row=cap):
        return lib.d2dg_encode(enc._h, k, w, h, frames.data_ptr(), None, 3, chunk.data_ptr(), row, lens.data_ptr(), None,
                               stream)

    assert encode(2, 24, 16) == G.E_OK
    torch.cuda.synchronize(dev)
    first = lens.cpu().tolist()
    assert first[0] > 20 and first[1] > 20 and first[2] == -7
    lens.fill_(-7)
    for args, msg in (((3, 24, 16), "n_streams 3 exceeds the ctx capacity 2"), ((2, 25, 16), "exceeds the ctx capacity 24 x 16"),
                      ((2, 24, 17), "exceeds the ctx capacity 24 x 16"), ((2, 16, 16), "the running GIFs are 24 x 16"),
                      ((2, 24, 16, G.frame_cap((16, 24)) - 1), "d2dg_frame_cap")):
        assert encode(*args) == G.E_ARG and msg in lib.d2dg_last_error().decode(), (args, lib.d2dg_last_error())
    torch.cuda.synchronize(dev)
    assert lens.cpu().tolist() == [-7, -7, -7] and int(chunk[2].max()) == 0
    with pytest.raises(ValueError):
        enc.add(frames[:2])  # the binding checks the shape itself
    assert lib.d2dg_restart(enc._h, stream) == G.E_OK
    assert encode(2, 16, 16) == G.E_OK  # new GIFs, another size
    torch.cuda.synchronize(dev)
    assert min(lens.cpu().tolist()[:2]) > 20
    enc.close()


def test_add_in_a_captured_graph(G):
    """16 ``add`` calls (one arena's worth) captured in a ``torch.cuda.graph`` and replayed: a call that
    synchronised or allocated outside the graph's pool would fail the capture.  The replay's files are the
    eager calls'."""
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    colours = distinct_palette(7, seed=1)
    T, K = 16, 3
    idx = rng.integers(0, 7, (T, K, 20, 33)).astype(np.uint8)
    idx[1:] = idx[0]
    idx[1:, :, 5:12, 4:25] = rng.integers(0, 7, (T - 1, K, 7, 21))
    active = rng.random((T, K)) < 0.8
    frames = torch.from_numpy(colours[idx]).to(dev)
    act = torch.from_numpy(active).to(dev)
    enc = G.GifEncoder(dev, K, (20, 33), G.Palette(colours), flush_every=T)
    for t in range(T):  # eagerly first: the library's kernels are loaded before the capture
        enc.add(frames[t], act[t])
    eager = enc.finish()
    assert eager == G.encode_host(colours[idx], G.Palette(colours), active)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(T):
            enc.add(frames[t], act[t])  # (recorded, not run)
    g.replay()
    assert enc.finish() == eager
    g.replay()  # the restart in finish() is ordered before it: first frames again
    enc.flush(T)
    assert enc.finish() == eager
    enc.close()


def _venv(d2, n, seed):
    from drone2d_amd.config import ENV_TEST_CONFIG

    return d2.Drone2dVecEnv(n, seed=seed, with_info=True, **dict(ENV_TEST_CONFIG, scenario="corridor"))


@pytest.mark.parametrize("deterministic", [False, True])
def test_record_episodes(d2, G, deterministic):
    """64 corridor envs under the shipped agent at 64 x 64, every second picture: each env's frame count is
    ceil(time_spent / 2) of ``evaluate_policy`` on an equally built batch with the same seed; no pixel was
    off the model palette; the decoded first and last frames are ``venv.render`` of the states they were
    taken from (a third equally built batch, flown again to each env's last kept picture)."""
    import torch

    from drone2d_amd import evaluate, harness

    n, seed, every, size = 64, 5, 2, 64
    policy = harness.MlpActor.from_npz(os.path.join(GOLDEN, "agent_17_90.npz")).to(torch.device("cuda", 0))
    venv = _venv(d2, n, seed)
    rec = G.record_episodes(venv, policy, range(n), seed=seed, deterministic=deterministic, size=size, every=every)
    venv.close()
    venv = _venv(d2, n, seed)
    m = evaluate.evaluate_policy(venv, policy, deterministic=deterministic, seed=seed)
    venv.close()
    assert m["unfinished"] == 0
    T = np.asarray(m["time_spent"])
    print(f"deterministic={deterministic}: episodes of {T.min()}..{T.max()} steps, files of "
          f"{min(map(len, rec.gifs))}..{max(map(len, rec.gifs))} bytes")
    assert rec.frames.tolist() == (-(-T // every)).tolist()
    assert rec.inexact.tolist() == [0] * n and rec.env_ids.tolist() == list(range(n))
    parsed = [parse_gif(b) for b in rec.gifs]
    assert [len(g["frames"]) for g in parsed] == rec.frames.tolist()
    assert all(f["delay"] == 3 for g in parsed for f in g["frames"])

    # fly again; env i's last kept picture shows the state after last[i] steps
    last = (rec.frames - 1) * every
    check = sorted({0, n - 1, int(np.argmin(T)), int(np.argmax(T)), 17, 40})
    venv = _venv(d2, n, seed)
    obs = venv.reset(seed=seed)
    first = venv.render(range(n), size=size).cpu().numpy()
    shown = {i: first[i] for i in check if last[i] == 0}
    for t in range(int(last[check].max())):
        a = evaluate.act(policy, obs, deterministic=deterministic, seed=seed, t=t, env_id_base=int(venv.cfg.env_id_base))
        obs = venv.step(a)[0]
        due = [i for i in check if last[i] == t + 1]
        if due:
            pics = venv.render(due, size=size).cpu().numpy()
            shown.update(zip(due, pics))
    venv.close()
    for i in check:
        frames = decode_gif(rec.gifs[i])
        assert len(frames) == rec.frames[i]
        assert (frames[0] == first[i]).all(), f"env {i}: first frame"
        assert (frames[-1] == shown[i]).all(), f"env {i}: last frame"
    for i in range(n):  # every file's first image is the whole reset picture
        f0 = parsed[i]["frames"][0]
        assert (f0["w"], f0["h"], f0["transparent"]) == (size, size, None)


def test_record_gifs_writes_the_files(d2, G, tmp_path):
    """``harness.record_gifs``: Gifs/<agent>/<scenario>.gif for one env, <scenario>_<k>.gif for several; with the
    HUD on the frames differ from the plain ones and still hold the model palette's colours only."""
    import torch

    from drone2d_amd import harness

    policy = harness.MlpActor.from_npz(os.path.join(GOLDEN, "agent_17_90.npz")).to(torch.device("cuda", 0))
    venv = _venv(d2, 4, 2)
    one = harness.record_gifs(venv, policy, str(tmp_path), "corridor", "17", env_ids=[1], seed=2, size=48, max_steps=40)
    assert one == [os.path.join(str(tmp_path), "Gifs", "17", "corridor.gif")]
    venv.close()
    venv = _venv(d2, 4, 2)
    three = harness.record_gifs(venv, policy, str(tmp_path), "corridor", "17", env_ids=[0, 1, 3], seed=2, size=48,
                                max_steps=40, hud=True)
    venv.close()
    assert [os.path.basename(p) for p in three] == ["corridor_0.gif", "corridor_1.gif", "corridor_2.gif"]
    plain = decode_gif(open(one[0], "rb").read())
    hud = decode_gif(open(three[1], "rb").read())
    # the same flight: at most the reset picture and every second one of 40 steps
    assert plain.shape == hud.shape and plain.shape[1:] == (48, 48, 3) and 2 <= len(plain) <= 21
    assert (plain[-1] != hud[-1]).any()
    model = {tuple(c) for c in G.Palette.model().colours.tolist()}
    assert {tuple(c) for c in np.unique(hud.reshape(-1, 3), axis=0).tolist()} <= model
