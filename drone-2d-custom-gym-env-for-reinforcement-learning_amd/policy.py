"""SB3 2.1's ``MlpPolicy`` for a Box action space: separate 27-64-64 tanh policy and value MLPs, state-independent
``log_std``, orthogonal init; parameter names as in SB3's state_dict, so an SB3 zip's ``policy.pth`` loads into it."""
from __future__ import annotations

import math
import zipfile

import numpy as np
import torch
from torch import nn

from .agent_io import _zip_tensors

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class ActorCritic(nn.Module):
    """SB3 2.1 ``MlpPolicy`` (net_arch pi=[64, 64], vf=[64, 64], tanh) for obs 27 -> action 2."""

    def __init__(self, obs_dim: int = 27, act_dim: int = 2, hidden: int = 64, log_std_init: float = 0.0):
        super().__init__()
        self.mlp_extractor = nn.Module()
        self.mlp_extractor.policy_net = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(),
                                                      nn.Linear(hidden, hidden), nn.Tanh())
        self.mlp_extractor.value_net = nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(),
                                                     nn.Linear(hidden, hidden), nn.Tanh())
        self.action_net = nn.Linear(hidden, act_dim)
        self.value_net = nn.Linear(hidden, 1)
        self.log_std = nn.Parameter(torch.ones(act_dim) * log_std_init)
        # ActorCriticPolicy._build, ortho_init=True
        for mod, gain in ((self.mlp_extractor, math.sqrt(2)), (self.action_net, 0.01), (self.value_net, 1.0)):
            for m in mod.modules():
                if isinstance(m, nn.Linear):
                    nn.init.orthogonal_(m.weight, gain=gain)
                    m.bias.data.fill_(0.0)

    def forward(self, obs: torch.Tensor):
        mean = self.action_net(self.mlp_extractor.policy_net(obs))
        value = self.value_net(self.mlp_extractor.value_net(obs)).squeeze(-1)
        return mean, value

    def dist(self, mean: torch.Tensor) -> torch.distributions.Normal:
        return torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp(), validate_args=False)

    def log_prob(self, mean: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        """Diagonal-Gaussian log density summed over the action dims (SB3 DiagGaussianDistribution),
        written out so it captures into a HIP graph (torch.distributions validates on the host)."""
        z = (actions - mean) * torch.exp(-self.log_std)
        return (-0.5 * z * z - self.log_std - _HALF_LOG_2PI).sum(-1)

    def entropy(self, n: int) -> torch.Tensor:
        return (0.5 + _HALF_LOG_2PI + self.log_std).sum().expand(n)

    def evaluate_actions(self, obs: torch.Tensor, actions: torch.Tensor):
        mean, value = self(obs)
        return value, self.log_prob(mean, actions), self.entropy(obs.shape[0])

    @torch.no_grad()
    def predict_values(self, obs: torch.Tensor) -> torch.Tensor:
        return self(obs)[1]

    @classmethod
    def from_agent_npz(cls, path: str) -> "ActorCritic":
        """The actor of a shipped agent (tests/golden/agent_17_90.npz: SB3 names with '.' -> '_');
        the value net keeps its fresh init (the fixture holds the actor only)."""
        m = cls()
        with np.load(path, allow_pickle=False) as z:
            sd = {k: torch.as_tensor(z[k]) for k in z.files}
        names = {n.replace(".", "_"): n for n in m.state_dict()}
        m.load_state_dict({names[k]: v for k, v in sd.items()}, strict=False)
        return m

    @classmethod
    def from_sb3_zip(cls, path: str) -> "ActorCritic":
        """The policy of an agent zip: ``policy.pth`` of a file written by ``PPO.save`` or by SB3's
        ``PPO.save`` (the reference's ``ppo_agents/*.zip``).  The actor must be complete; the value
        net is loaded when the file has one, and keeps its fresh init otherwise."""
        with zipfile.ZipFile(path) as z:
            if "policy.pth" not in z.namelist():
                raise ValueError(f"{path}: no policy.pth member")
            sd = _zip_tensors(z, "policy.pth")
        m = cls()
        own = m.state_dict()
        actor = [k for k in own if k.startswith(("mlp_extractor.policy_net.", "action_net.", "log_std"))]
        missing = [k for k in actor if k not in sd]
        if missing:
            raise ValueError(f"{path}: policy.pth lacks {missing}")
        bad = [k for k in own if k in sd and tuple(sd[k].shape) != tuple(own[k].shape)]
        if bad:
            raise ValueError(f"{path}: policy.pth is not an MlpPolicy 27-64-64 (shape of {bad})")
        m.load_state_dict({k: v.float() for k, v in sd.items() if k in own}, strict=False)
        return m
