"""Pytree surface of the Q-learning systems on torch tensors (mava/systems/q_learning/types.py): same names and fields as the reference's
NamedTuples.  Leaves are device tensors with a leading group axis (the reference's update-batch axis); parameters are the network's named
views, the optimiser state the flat optax-adam triple, the buffer state the device ring's tensors with its two counters."""
from __future__ import annotations

from typing import Any, Dict, NamedTuple

import torch


class Transition(NamedTuple):
    obs: Any
    action: torch.Tensor
    reward: torch.Tensor
    terminal: torch.Tensor
    term_or_trunc: torch.Tensor
    next_obs: Any                        # real_next_obs: the observation before the auto-reset (auto_reset_wrapper.py:52-83)


class QNetParams(NamedTuple):
    online: Dict[str, torch.Tensor]
    target: Dict[str, torch.Tensor]


class QMIXParams(NamedTuple):
    online: Dict[str, torch.Tensor]
    target: Dict[str, torch.Tensor]
    mixer_online: Dict[str, torch.Tensor]
    mixer_target: Dict[str, torch.Tensor]


class ActionSelectionState(NamedTuple):
    online_params: Dict[str, torch.Tensor]
    hidden_state: torch.Tensor
    time_steps: Any
    key: Any


class ActionState(NamedTuple):
    action_selection_state: ActionSelectionState
    env_state: Any
    buffer_state: Any
    obs: Any
    terminal: torch.Tensor
    term_or_trunc: torch.Tensor


class LearnerState(NamedTuple):
    obs: Any                             # agents_view, step_count[, action_mask] of every group
    terminal: torch.Tensor               # [groups, N] u8
    term_or_trunc: torch.Tensor          # [groups, N] u8
    hidden_state: torch.Tensor           # [groups, N * A, 128]
    env_state: Any
    time_steps: torch.Tensor             # [groups] i32: env steps taken (drives epsilon)
    train_steps: torch.Tensor            # [groups] i32: training epochs done
    opt_state: Dict[str, Any]            # optax adam: count, mu, nu (flat buffers)
    buffer_state: Dict[str, Any]         # experience (the ring's fields), current_index, filled: [groups, ...]
    params: QNetParams
    key: Any                             # [groups, 2] uint32


class TrainState(NamedTuple):
    buffer_state: Any
    params: QNetParams
    opt_state: Dict[str, Any]
    train_steps: Any
    key: Any
