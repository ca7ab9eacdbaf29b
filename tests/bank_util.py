"""Shared by tests/test_eval_bank.py and tests/test_gpu_eval_bank.py: the three policies of the policy-bank
tests and env -> policy maps."""
import os

import numpy as np
import torch

AGENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agent_17_90.npz")


def make_policies() -> dict:
    """'shipped': the reference's agent 17_90; 'perturbed': as tests/test_gpu_eval.py builds it (a random
    ActorCritic away from its init: log_std != 0, a larger action head); 'fresh': ActorCritic() under
    torch.manual_seed(1)."""
    from drone2d_amd.ppo import ActorCritic

    torch.manual_seed(0)
    pert = ActorCritic()
    with torch.no_grad():
        pert.log_std.copy_(torch.tensor([-0.4, 0.3]))
        pert.action_net.weight.mul_(20.0)
        pert.action_net.bias.copy_(torch.tensor([0.2, -0.1]))
        for lin in (pert.mlp_extractor.policy_net[0], pert.mlp_extractor.policy_net[2]):
            lin.bias.copy_(torch.randn(64) * 0.3)
    torch.manual_seed(1)
    fresh = ActorCritic()
    return {"shipped": ActorCritic.from_agent_npz(AGENT), "perturbed": pert, "fresh": fresh}


def blocks(n: int, size: int, n_policies: int = 3) -> np.ndarray:
    """Env i -> policy (i // size) % P: contiguous blocks of ``size`` envs."""
    return ((np.arange(n) // size) % n_policies).astype(np.int32)
