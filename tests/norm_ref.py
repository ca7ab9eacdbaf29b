"""Test reference: the reward path of Stable-Baselines3 2.1's ``VecNormalize`` restated in float64 NumPy
(``common/running_mean_std.py`` and ``common/vec_env/vec_normalize.py``), written from SB3's source and
independently of ``drone2d_amd.normalize``.  Never shipped."""
import numpy as np


class RunningMeanStd:
    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = epsilon

    def update(self, arr):
        batch_mean = np.mean(arr, axis=0)
        batch_var = np.var(arr, axis=0)
        batch_count = arr.shape[0]
        self.update_from_moments(batch_mean, batch_var, batch_count)

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        m_2 = m_a + m_b + np.square(delta) * self.count * batch_count / (self.count + batch_count)
        new_var = m_2 / (self.count + batch_count)
        new_count = batch_count + self.count
        self.mean = new_mean
        self.var = new_var
        self.count = new_count


class VecNormalizeReward:
    """``VecNormalize(venv, norm_obs=False, norm_reward=True)``: what ``step_wait`` does to the rewards."""

    def __init__(self, n, gamma=0.99, clip_reward=10.0, epsilon=1e-8):
        self.ret_rms = RunningMeanStd(shape=())
        self.returns = np.zeros(n, np.float64)
        self.gamma, self.clip_reward, self.epsilon = gamma, clip_reward, epsilon
        self.training = True

    def step(self, rewards, dones):
        rewards = np.asarray(rewards, np.float64)
        if self.training:
            self.returns = self.returns * self.gamma + rewards
            self.ret_rms.update(self.returns)
        out = np.clip(rewards / np.sqrt(self.ret_rms.var + self.epsilon), -self.clip_reward, self.clip_reward)
        self.returns[np.asarray(dones, bool)] = 0
        return out

    @property
    def rms(self):
        return np.array([self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count], np.float64)
