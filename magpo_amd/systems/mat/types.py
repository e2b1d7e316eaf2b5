"""Pytree surface of the MAT system on torch tensors (mava/systems/mat/types.py).

``LearnerState`` is the memoryless Sable system's (magpo_amd/systems/sable/types.py: FFLearnerState -- params, optimiser state, key,
env_state, timestep): MAT carries nothing else between env steps, and one state type keeps one checkpoint format.  Its second field is
named ``opt_states`` as there (the reference's MAT state calls it ``opt_state``)."""
from __future__ import annotations

from typing import Any, Callable, NamedTuple

from magpo_amd.systems.sable.types import FFLearnerState, Transition  # noqa: F401  (PPOTransition)

LearnerState = FFLearnerState


class MATNetworkConfig(NamedTuple):
    n_block: int
    n_head: int
    embed_dim: int
    use_swiglu: bool
    use_rmsnorm: bool


ActorApply = Callable[..., Any]      # MatNetwork.get_actions
LearnerApply = Callable[..., Any]    # MatNetwork.apply
