"""Pytree surface of the Sable system on torch tensors (mava/systems/sable/types.py, mava/systems/ppo/types.py: PPOTransition).

Same names and fields as the reference NamedTuples.  Leaves are device tensors with a leading group axis (the reference's update-batch
axis); the hidden states use the logical [embed_dim / n_head, embed_dim / n_head] head-state layout of ``GPOLearnerState``
(magpo_amd.sable.sable_hstates_logical)."""
from __future__ import annotations

from typing import Any, Callable, Dict, NamedTuple

import torch


class SableNetworkConfig(NamedTuple):
    n_block: int
    n_head: int
    embed_dim: int


class HiddenStates(NamedTuple):
    encoder: torch.Tensor            # [groups, n_block, n_head, N, hs, hs]
    decoder_self_retn: torch.Tensor
    decoder_cross_retn: torch.Tensor


class RecLearnerState(NamedTuple):
    params: Dict[str, torch.Tensor]
    opt_states: Dict[str, Any]       # optax adam: count, mu, nu (flat buffers)
    key: Any
    env_state: Any
    timestep: Any                    # agents_view, step_count, [action_mask,] last ([groups, N] u8: timestep.last())
    hstates: HiddenStates


class FFLearnerState(NamedTuple):     # ff_sable: nothing is carried between env steps but the env itself
    params: Dict[str, torch.Tensor]
    opt_states: Dict[str, Any]
    key: Any
    env_state: Any
    timestep: Any                    # agents_view, step_count, [action_mask,] last


class Transition(NamedTuple):        # PPOTransition
    done: torch.Tensor
    action: torch.Tensor
    value: torch.Tensor
    reward: torch.Tensor
    log_prob: torch.Tensor
    obs: Any


LearnerState = RecLearnerState
ActorApply = Callable[..., Any]      # SableGuider.get_actions
LearnerApply = Callable[..., Any]    # SableGuider.apply
