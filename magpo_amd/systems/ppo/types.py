"""Pytree surface of the PPO systems (recurrent and feed-forward) on torch tensors (mava/systems/ppo/types.py).

Same names and fields as the reference NamedTuples.  Leaves are device tensors with a leading group axis (the reference's update-batch
axis); parameters are the networks' named views (magpo_amd/params.py: actor_named_views), optimiser states the flat optax-adam triple."""
from __future__ import annotations

from typing import Any, Dict, NamedTuple

import torch


class Params(NamedTuple):
    actor_params: Dict[str, torch.Tensor]
    critic_params: Dict[str, torch.Tensor]


class OptStates(NamedTuple):
    actor_opt_state: Dict[str, Any]      # optax adam: count, mu, nu (flat buffers)
    critic_opt_state: Dict[str, Any]


class HiddenStates(NamedTuple):
    policy_hidden_state: torch.Tensor    # [groups, N * A, 128]
    critic_hidden_state: torch.Tensor


class LearnerState(NamedTuple):
    """State of the feed-forward systems (ff_ippo / ff_mappo)."""
    params: Params
    opt_states: OptStates
    key: Any
    env_state: Any
    timestep: Any                        # agents_view, step_count[, action_mask]
    dones: torch.Tensor                  # [groups, N] u8: timestep.last(), repeated over the agents inside the kernels


class PPOTransition(NamedTuple):
    done: torch.Tensor
    action: torch.Tensor
    value: torch.Tensor
    reward: torch.Tensor
    log_prob: torch.Tensor
    obs: Any


class RNNLearnerState(NamedTuple):
    params: Params
    opt_states: OptStates
    key: Any
    env_state: Any
    timestep: Any                        # agents_view, step_count[, action_mask]
    dones: torch.Tensor                  # [groups, N] u8: timestep.last(), repeated over the agents inside the kernels
    hstates: HiddenStates


class RNNPPOTransition(NamedTuple):
    done: torch.Tensor
    action: torch.Tensor
    value: torch.Tensor
    reward: torch.Tensor
    log_prob: torch.Tensor
    obs: Any
    hstates: HiddenStates
