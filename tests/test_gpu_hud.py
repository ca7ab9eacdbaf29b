"""libd2d_hud.so on the device: the kernels byte for byte against the CPU twins, the layers-off identity with
libd2d_render.so's kernels, the shade recorder against its NumPy twin over auto-resets, and the HUD through
Drone2dEnv / Drone2dVecEnv."""
import numpy as np
import pytest

from conftest import SCENARIOS
from test_hud import pose_state, text_raster

pytestmark = pytest.mark.gpu

CANARY = 4096
TRAIL_CAP, SHADE_CAP = 24, 6


@pytest.fixture(scope="module")
def H(d2):
    from drone2d_amd import hud

    return hud


@pytest.fixture(scope="module")
def R(d2):
    from drone2d_amd import render

    return render


@pytest.fixture(scope="module")
def hud_renderer(H):
    import torch

    r = H.HudRenderer(torch.device("cuda", 0), max_frames=8, max_trail=TRAIL_CAP, max_shades=SHADE_CAP)
    yield r
    r.close()


@pytest.fixture(scope="module")
def inputs():
    """Three frames of a mixed batch -- S_corridor (58 circles), large, corridor without obstacles -- with
    seeded poses, obs, actions, trails, info rows and shades (one list past its capacity, one empty)."""
    from drone2d_amd.scenarios import create_test_scenario, free_flight

    scns = [create_test_scenario("S_corridor", 1300, 1300), create_test_scenario("large", 1300, 1300),
            free_flight(create_test_scenario("corridor", 1300, 1300))]
    k = len(scns)
    rng = np.random.default_rng(12)
    st = pose_state([(rng.uniform(150, 1150), rng.uniform(150, 1150), rng.uniform(-1.5, 1.5), rng.uniform(-300, 300),
                      rng.uniform(-300, 300)) for _ in range(k)])
    obs = rng.uniform(-1, 1, (k, 27)).astype(np.float32)
    act = rng.uniform(-1, 1, (k, 2)).astype(np.float32)
    trail = (np.cumsum(rng.uniform(-30, 30, (k, TRAIL_CAP, 2)), 1) + 650).astype(np.float32)
    tl = np.array([TRAIL_CAP, 7, 1], np.int32)
    info = rng.standard_normal((k, 12)).astype(np.float32) * np.float32(3.0)
    info[2, 6] = np.inf  # dist_closest_obs of an obstacle-free scenario
    poses = np.stack([rng.uniform(100, 1200, (k, SHADE_CAP)), rng.uniform(100, 1200, (k, SHADE_CAP)),
                      rng.uniform(-1.5, 1.5, (k, SHADE_CAP))], -1)
    count = np.array([SHADE_CAP + 3, 2, 0], np.int32)
    return scns, st, obs, act, trail, tl, info, (poses, count)


def _device_vs_host(H, r, inp, size, layers, frames=slice(None)):
    """Render on the device into a buffer with 4 KiB canaries on both sides; compare with the twin."""
    import torch

    scns, st, obs, act, trail, tl, info, (poses, count) = inp
    scns = scns[frames]
    st, obs, act, trail, tl, info = st[:, frames], obs[frames], act[frames], trail[frames], tl[frames], info[frames]
    poses, count = poses[frames], count[frames]
    h, w = H._size(size)
    k = len(scns)
    n = k * h * w * 3
    flat = torch.full((CANARY + n + CANARY,), 0xA5, dtype=torch.uint8, device=r.device)
    out = flat[CANARY:CANARY + n].view(k, h, w, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    r.render(r.scn_tensor(scns), t(st), t(obs), t(act), t(trail), t(tl), t(info), (t(poses), t(count)), size=size,
             layers=layers, out=out)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert (got[:CANARY] == 0xA5).all() and (got[CANARY + n:] == 0xA5).all(), "canary overwritten"
    want = H.render_host(scns, st, obs, act, trail, tl, info, (poses, count), size=size, layers=layers)
    frame = got[CANARY:CANARY + n].reshape(k, h, w, 3)
    bad = int((frame != want).any(-1).sum())
    assert bad == 0, f"{bad} pixels differ between device and host twin"
    return frame


@pytest.mark.parametrize("size", [8, (61, 97), 256])
def test_device_equals_twin(H, hud_renderer, inputs, size):
    """8 x 8, 97 wide x 61 high (row bytes no multiple of 4, partial tiles on both edges) and 256 x 256; all
    layers on, and each new bit alone."""
    seen = set()
    for layers in (H.L_ALL, H.L_TEXT, H.L_ARCS, H.L_SHADE):
        seen.add(_device_vs_host(H, hud_renderer, inputs, size, layers).tobytes())
    assert len(seen) == 4


@pytest.mark.parametrize("size", [1300, 2048])
def test_device_equals_twin_full_size(H, hud_renderer, inputs, size):
    """One frame at the reference's screen size (text scale 2) and at the largest picture (scale 4)."""
    f = _device_vs_host(H, hud_renderer, inputs, size, H.L_ALL, frames=slice(0, 1))
    packed = np.unique(f[..., 0].astype(np.uint32) << 16 | f[..., 1].astype(np.uint32) << 8 | f[..., 2])
    for r, g, b in ((0, 0, 0), (150, 0, 0), H.SHADE_FRAME_RGB, (0, 255, 0), (0, 150, 150)):  # text, shades, arcs
        assert (r << 16 | g << 8 | b) in packed


def test_new_bits_clear_equals_the_renderer_on_the_device(H, R, hud_renderer, inputs):
    """d2dh_render with the three bits clear == d2dr_render for the same inputs, both on the device."""
    import torch

    scns, st, obs, act, trail, tl, info, (poses, count) = inputs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    base = R.Renderer(hud_renderer.device, max_frames=8, max_trail=TRAIL_CAP)
    try:
        scn = base.scn_tensor(scns)
        for size in ((61, 97), 256):
            for layers in (R.L_ALL, R.L_GUIDES, R.L_TRAIL | R.L_DRONE):
                want = base.render(scn, t(st), t(obs), t(act), t(trail), t(tl), size=size, layers=layers)
                got = hud_renderer.render(scn, t(st), t(obs), t(act), t(trail), t(tl), t(info), (t(poses), t(count)),
                                          size=size, layers=layers)
                assert torch.equal(got, want)
                bare = hud_renderer.render(scn, t(st), t(obs), t(act), t(trail), t(tl), size=size, layers=layers)
                assert torch.equal(bare, want)
        empty = hud_renderer.render(scn[:0], torch.zeros(32, 0, dtype=torch.float64), size=64)
        assert tuple(empty.shape) == (0, 64, 64, 3)  # n_frames = 0: OK, nothing launched
        with pytest.raises(H.HudError, match="code 1"):  # more frames than the ctx holds
            hud_renderer.render(scn[[0] * 9], t(st[:, [0] * 9]), size=64)
    finally:
        base.close()


def _kw(**over):
    from drone2d_amd.config import ENV_TRAIN_CONFIG

    return dict(ENV_TRAIN_CONFIG, **over)


def test_shade_recorder_on_the_device(d2, H):
    """192 envs (three workgroups of the step kernel) with a 60-step time limit, so every env restarts three
    times in 200 steps of seeded random actions; 5 tracked ids including the first and the last env; distance
    20 and capacity 4, so lists overflow.  The device buffers equal the NumPy twin's bit for bit every 50 steps."""
    import torch

    n, ids = 192, [0, 63, 64, 130, 191]
    venv = d2.Drone2dVecEnv(n, seed=5, **_kw(scenario=list(SCENARIOS), n_steps=60))
    venv.reset()
    rec = H.ShadeRecorder(venv, ids, distance=20.0, capacity=4)
    poses, count, last = np.zeros((5, 4, 3)), np.zeros(5, np.int32), np.zeros((5, 2))
    H.shade_update_np(ids, venv.get_state()[0].cpu().numpy(), None, None, 20.0, poses, count, last)
    g = torch.Generator(device=venv.device).manual_seed(9)
    restarted = np.zeros(5, bool)
    overflowed = appended = False
    for step in range(1, 201):
        _, _, term, trunc, _ = venv.step(torch.rand(n, 2, device=venv.device, generator=g) * 2 - 1)
        rec.update()
        te, tu = term.cpu().numpy(), trunc.cpu().numpy()
        H.shade_update_np(ids, venv.get_state()[0].cpu().numpy(), te, tu, 20.0, poses, count, last)
        restarted |= (te | tu)[ids]
        appended |= bool((count > 1).any())
        overflowed |= bool((count > 4).any())
        if step % 50 == 0:
            assert rec.poses.cpu().numpy().tobytes() == poses.tobytes(), step
            assert rec.count.cpu().numpy().tobytes() == count.tobytes(), step
            assert rec.last.cpu().numpy().tobytes() == last.tobytes(), step
    print(f"restarted {restarted}, appended {appended}, overflowed {overflowed}, count {count}")
    assert restarted.all() and appended and overflowed
    rec.restart()
    assert (rec.count.cpu().numpy() == 1).all()
    with pytest.raises(ValueError):
        H.ShadeRecorder(venv, [0, n])
    # the recorder's lists as the frames' shades
    frames = venv.render(ids, size=64, shades=rec)
    assert tuple(frames.shape) == (5, 64, 64, 3)
    with pytest.raises(ValueError):
        venv.render([0, 1], size=64, shades=rec)
    venv.close()


def test_single_env_hud(d2, H, R):
    """Drone2dEnv.render(mode="rgb_array", hud=True) after a few steps of the test config: the text block's first
    line is the env's own info["reward"] through the NumPy rasteriser (and the whole block the info table's);
    the picture equals the twin on the env's state, info and recorded shades; hud=False is today's picture."""
    from drone2d_amd.config import ENV_TEST_CONFIG

    env = d2.Drone2dEnv(**dict(ENV_TEST_CONFIG, scenario="corridor"))
    first = env.render(mode="rgb_array", hud=True)  # before any step: no text yet
    assert first.shape == (1300, 1300, 3) and (first[:16, :200] == 243).all()
    for _ in range(5):
        _, _, _, info = env.step(np.array([0.6, 0.5], np.float32))
    img = env.render(mode="rgb_array", hud=True)
    assert img.shape == (1300, 1300, 3) and img.dtype == np.uint8
    s = H.text_scale(1300)
    line = "Total reward: " + str(round(info["reward"], 2))
    want = np.full((7 * s, 6 * s * len(line) + 6 * s, 3), 243, np.uint8)
    for j, ch in enumerate(line):
        g = np.kron(H.glyph(ch), np.ones((s, s), np.uint8)).astype(bool)
        want[:, 6 * s * j:6 * s * j + 5 * s][g] = 0
    assert (img[:7 * s, :want.shape[1]] == want).all()
    venv = env._venv
    row = venv._bufs[venv._k]["info"][0].cpu().numpy()
    assert (img[:7 * s, :300 * s] == text_raster(H, row, 1300, 1300)[:7 * s, :300 * s]).all()
    st = venv.get_state()[0].cpu().numpy()
    cap = int(env.kwargs["n_steps"]) + 1
    xy = np.zeros((1, cap, 2), np.float32)
    fp = np.asarray(env.flight_path, np.float64)
    xy[0, :len(fp), 0], xy[0, :len(fp), 1] = fp[:, 0], 1300.0 - fp[:, 1]
    tl = np.array([len(fp)], np.int32)
    obs, act = venv._bufs[venv._k]["obs"].cpu().numpy(), venv._last_actions.cpu().numpy()
    poses, count = env._shades.poses.cpu().numpy(), env._shades.count.cpu().numpy()
    assert count[0] >= 1 and (poses[0, 0, :2] != st[0:2, 0]).any()  # the spawn pose, not the current one
    twin = H.render_host([venv.scenarios[0]], st, obs, act, xy, tl, row[None], (poses, count), size=1300)[0]
    assert (img == twin).all()
    plain = env.render(mode="rgb_array")
    assert (plain == R.render_host([venv.scenarios[0]], st, obs, act, xy, tl, size=1300)[0]).all()
    assert (plain != img).any()
    env.reset()
    assert int(env._shades.count.cpu().numpy()[0]) == 1
    env.close()
    # an env without info rows cannot print them
    v = d2.Drone2dVecEnv(2, seed=1, with_info=False, **_kw(scenario="parallel"))
    v.reset()
    with pytest.raises(ValueError):
        v.render(size=64, text=True)
    assert tuple(v.render(size=64, arcs=True).shape) == (2, 64, 64, 3)
    v.close()


def test_sb3_get_images_hud(d2):
    from drone2d_amd.sb3 import SB3VecEnv

    v = SB3VecEnv(3, seed=1, **_kw(scenario="parallel"))
    v.reset()
    plain = v.get_images()
    assert len(v.get_images(hud=True)) == len(plain) == 3  # before a step: the arcs, no text yet
    v.step(np.zeros((3, 2), np.float32))
    plain, imgs = v.get_images(), v.get_images(hud=True)
    assert len(imgs) == 3 and all(im.shape == (256, 256, 3) and im.dtype == np.uint8 for im in imgs)
    assert all((a[:7] != b[:7]).any() for a, b in zip(plain, imgs))  # the first text line
    v.close()


def test_hud_rendering_does_not_disturb_stepping(d2, H):
    """Two identical 64-env batches take 20 steps, one of them recording shades and rendering HUD frames every
    step: obs, reward and state are bitwise equal afterwards."""
    import torch

    n = 64
    a = d2.Drone2dVecEnv(n, seed=7, **_kw(scenario=list(SCENARIOS)))
    b = d2.Drone2dVecEnv(n, seed=7, **_kw(scenario=list(SCENARIOS)))
    oa, ob = a.reset(), b.reset()
    ids = list(range(0, n, 5))
    rec = H.ShadeRecorder(b, ids, distance=10.0)
    g = torch.Generator(device=a.device).manual_seed(3)
    for _ in range(20):
        act = torch.rand(n, 2, device=a.device, generator=g) * 2 - 1
        oa, ra, *_ = a.step(act)
        ob, rb, *_ = b.step(act.clone())
        rec.update()
        b.render(ids, size=64, text=True, arcs=True, shades=rec)
    assert torch.equal(oa, ob) and torch.equal(ra, rb)
    (sa, ia), (sb, ib) = a.get_state(), b.get_state()
    assert torch.equal(sa, sb) and torch.equal(ia, ib)
    assert int(rec.count.max()) > 1
    a.close()
    b.close()
