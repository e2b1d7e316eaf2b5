"""What rec_ppo.py (rec_ippo / rec_mappo) and ff_ppo.py (ff_ippo / ff_mappo) share: the config's SystemConfig and the critic's, the owner
checks of ``get_learner_fn``, the centralised critic's input shape and the learner-state fields both have (Params, OptStates, key and the
rollout state).  rec_ppo.py adds its hidden states and the ``recurrent_chunk_size`` checks, ff_ppo.py its torso rule and action-space check.
"""
from __future__ import annotations

import dataclasses

from magpo_amd.critic import global_state_ld
from magpo_amd.learner import SystemConfig, obs_row_stride
from magpo_amd.optim import ClipAdam
from magpo_amd.ppo_learner import raw_features
from magpo_amd.systems.common import (_owner, _system_config, as_dict, load_opt_state, load_rollout_state, snapshot_opt_state,
                                      snapshot_rollout_state)
from magpo_amd.systems.ppo.types import OptStates, Params


def system_config(config) -> SystemConfig:
    """The learner's settings from a PPO config tree (no ``clip_gpo`` / ``alpha``: MAGPO's keys, never read here)."""
    return _system_config(config, clip_gpo=SystemConfig.clip_gpo, alpha=SystemConfig.alpha)


def critic_system_config(sysc: SystemConfig, config) -> SystemConfig:
    """``sysc`` with ``system.critic_lr`` as its rate: ClipAdam reads its rate as actor_lr."""
    return dataclasses.replace(sysc, actor_lr=float(config.system.critic_lr))


def critic_input(env, centralised: bool):
    """(features, row stride) of the rows the critic reads: agents_view rows, or for a centralised critic observation.global_state, the raw
    views of all agents (environments.make checked the width; global_state_ld names the 128-input limit)."""
    cfg = env.cfg
    if centralised:
        return cfg.num_agents * raw_features(cfg), global_state_ld(cfg.num_agents, raw_features(cfg))
    return env.obs_dim, obs_row_stride(cfg.obs_dim)


def owners(apply_fns, update_fns, actor_cls, critic_cls, an_actor: str):
    """(actor, critic, actor optimiser, critic optimiser) that own ``apply_fns`` = (actor_apply_fn, critic_apply_fn) and ``update_fns`` =
    (actor_update_fn, critic_update_fn): bound ``apply`` methods of ``actor_cls`` / ``critic_cls`` (a subclass of it) and ``ClipAdam.update``
    of their optimisers, in this order, or the errors of common._owner.  ``an_actor``: the actor class with its article, for the message."""
    actor_apply_fn, critic_apply_fn = apply_fns
    actor_update_fn, critic_update_fn = update_fns
    critic = _owner(critic_apply_fn, critic_cls, "apply", "apply_fns[1] (critic_apply_fn)")
    actor = _owner(actor_apply_fn, actor_cls, "apply", "apply_fns[0] (actor_apply_fn)")
    if isinstance(actor, critic_cls):
        raise TypeError(f"get_learner_fn: apply_fns[0] (actor_apply_fn) must belong to {an_actor}, not to the critic")
    a_opt = _owner(actor_update_fn, ClipAdam, "update", "update_fns[0] (actor_update_fn)")
    c_opt = _owner(critic_update_fn, ClipAdam, "update", "update_fns[1] (critic_update_fn)")
    if a_opt.net is not actor or c_opt.net is not critic:
        raise ValueError("update_fns must be the update functions of the optimisers of (actor, critic), in this order")
    return actor, critic, a_opt, c_opt


def snapshot_shared(learner):
    """(params, opt_states, key, env_state, timestep, dones) of the learner as independent copies: the leading fields of LearnerState and
    RNNLearnerState alike; leaves carry a leading group axis."""
    params = Params({k: v.clone() for k, v in learner.actor.named.items()}, {k: v.clone() for k, v in learner.critic.named.items()})
    opts = OptStates(snapshot_opt_state(learner.a_opt), snapshot_opt_state(learner.c_opt))
    return (params, opts, learner.groups[0].key.copy(), *snapshot_rollout_state(learner.groups))


def load_shared(learner, state) -> None:
    """Inverse of ``snapshot_shared``: those fields of ``state`` into the learner's (static, graph-captured) buffers."""
    params, opts = as_dict(state.params), as_dict(state.opt_states)
    learner.actor.load_named(params["actor_params"])
    learner.critic.load_named(params["critic_params"])
    load_opt_state(learner.a_opt, opts["actor_opt_state"])
    load_opt_state(learner.c_opt, opts["critic_opt_state"])
    load_rollout_state(learner.groups, state.key, state.env_state, state.timestep, state.dones)
