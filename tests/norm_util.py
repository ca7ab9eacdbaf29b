"""Shared inputs of the reward-normalisation tests (tests/test_reward_norm.py, tests/test_gpu_reward_norm.py):
six steps of rewards and done masks for n envs, and runs of the NumPy twin over them.  Never shipped."""
import numpy as np

STEPS = 6
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
GAMMA = 0.99


def realistic(n, seed=0):
    """Rewards as the env gives them: N(0.5, 1.5) per step, a done row (p = 0.15) adds +30 or -50.
    Returns (rew [STEPS, n] float32, term, trunc [STEPS, n] bool)."""
    rng = np.random.default_rng(7000 * seed + n)
    rew = rng.normal(0.5, 1.5, (STEPS, n))
    done = rng.random((STEPS, n)) < 0.15
    rew = rew + np.where(done, rng.choice([30.0, -50.0], (STEPS, n)), 0.0)
    term = done & (rng.random((STEPS, n)) < 0.8)
    return rew.astype(np.float32), term, done & ~term


def order_sensitive(n, seed=0):
    """``realistic`` with a third of the rewards replaced by +-m 2^e, m a 24-bit value in [1, 2) and e
    uniform in 0..20: float64 sums of such returns (and of their squares) round at nearly every
    addition, differently in another order, so equal bits mean the same order of addition."""
    rew, term, trunc = realistic(n, seed)
    rng = np.random.default_rng(9000 * seed + n)
    wide = rng.uniform(1.0, 2.0, (STEPS, n)) * 2.0 ** rng.integers(0, 21, (STEPS, n)) * rng.choice([-1.0, 1.0], (STEPS, n))
    where = rng.random((STEPS, n)) < 1.0 / 3.0
    rew[where] = wide.astype(np.float32)[where]
    return rew, term, trunc


def reorder(data, group, sub):
    """``data`` with the envs of every full ``group`` rearranged: its ``sub``-sized pieces in reverse
    order.  (64, 1) reverses the lanes of each wave, (256, 64) the waves of each chunk."""
    n = data[0].shape[1]
    perm = np.arange(n)
    for s in range(0, n - n % group, group):
        perm[s:s + group] = perm[s:s + group].reshape(group // sub, sub)[::-1].ravel()
    return tuple(x[:, perm] for x in data)


def permute_lanes(data):
    """``data`` with the lanes of every full wave in another order (one fixed random permutation of the
    64 lanes).  The shuffle-down tree adds lanes l and l + s, so it is blind to a reversal or a rotation
    of the 64 lanes (the same pairs meet at every stage, and a + b = b + a); a random permutation makes
    other lanes meet."""
    n = data[0].shape[1]
    lanes = np.random.default_rng(64).permutation(64)
    perm = np.arange(n)
    for s in range(0, n - n % 64, 64):
        perm[s:s + 64] = perm[s:s + 64][lanes]
    return tuple(x[:, perm] for x in data)


def twin_run(data, n_blocks=None, training=True, clip=10.0, epsilon=1e-8, ret0=None, rms0=None):
    """The twin over ``data``: per step (rew_out, ret, rms) copies."""
    from drone2d_amd.normalize import RMS_INIT, reward_norm_host

    rew, term, trunc = data
    n = rew.shape[1]
    ret = np.zeros(n) if ret0 is None else np.array(ret0, np.float64)
    rms = np.array(RMS_INIT if rms0 is None else rms0, np.float64)
    out = []
    for t in range(rew.shape[0]):
        o = reward_norm_host(rew[t], term[t], trunc[t], ret, rms, GAMMA, clip, epsilon, n_blocks, training)
        out.append((o, ret.copy(), rms.copy()))
    return out
