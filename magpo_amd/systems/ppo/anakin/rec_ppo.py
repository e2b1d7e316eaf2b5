"""The one implementation behind the two recurrent PPO systems, rec_ippo and rec_mappo (mava/systems/ppo/anakin/rec_ippo.py, rec_mappo.py).

The two reference files differ in three places only: ``centralised_critic`` of the critic network (rec_mappo.py:429), ``add_global_state``
of the env factory (:558) and the system name (:540).  ``make_system(name, centralised)`` returns the reference's public functions for one
of them; rec_ippo.py / rec_mappo.py bind them at module level under the reference's names.  The bodies drive the HIP kernels
(magpo_amd.ppo_learner.PpoLearner); the experiment loop, the learner loop and the shared parts of the learner state are the ones every
system uses (magpo_amd/systems/common.py).
"""
from __future__ import annotations

import dataclasses
import sys
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.actor import GruActor
from magpo_amd.config import compose
from magpo_amd.critic import GruCritic, global_state_ld
from magpo_amd.learner import SystemConfig, host_split, obs_row_stride, prng_key
from magpo_amd.optim import ClipAdam
from magpo_amd.ppo_learner import LOSS_NAMES, PpoLearner, check_chunk_size, raw_features
from magpo_amd.systems.common import (_owner, _system_config, as_dict, load_opt_state, load_rollout_state, make_learner_fn, network_torsos,
                                      setup_learner, snapshot_opt_state, snapshot_rollout_state, start_experiment,
                                      train_and_evaluate_gru_actor)
from magpo_amd.systems.ppo.types import HiddenStates, OptStates, Params, RNNLearnerState
from magpo_amd.utils import make_env as environments


def system_config(config) -> SystemConfig:
    """The learner's settings from a rec_ippo / rec_mappo config tree (no ``clip_gpo`` / ``alpha``: MAGPO's keys, never read here)."""
    return _system_config(config, clip_gpo=SystemConfig.clip_gpo, alpha=SystemConfig.alpha)


def _snapshot_state(learner: PpoLearner) -> RNNLearnerState:
    """RNNLearnerState of the learner as an independent COPY (rec_mappo.py:353-361); leaves carry a leading group axis."""
    gs = learner.groups
    params = Params({k: v.clone() for k, v in learner.actor.named.items()}, {k: v.clone() for k, v in learner.critic.named.items()})
    return RNNLearnerState(params, OptStates(snapshot_opt_state(learner.a_opt), snapshot_opt_state(learner.c_opt)), gs[0].key.copy(),
                           *snapshot_rollout_state(gs),
                           HiddenStates(torch.stack([g.policy_h[0] for g in gs]), torch.stack([g.critic_h[0] for g in gs])))


def load_learner_state(learner: PpoLearner, state: RNNLearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    params, opts, hst = as_dict(state.params), as_dict(state.opt_states), as_dict(state.hstates)
    learner.actor.load_named(params["actor_params"])
    learner.critic.load_named(params["critic_params"])
    load_opt_state(learner.a_opt, opts["actor_opt_state"])
    load_opt_state(learner.c_opt, opts["critic_opt_state"])
    load_rollout_state(learner.groups, state.key, state.env_state, state.timestep, state.dones)
    for gi, grp in enumerate(learner.groups):
        grp.policy_h[0].copy_(hst["policy_hidden_state"][gi])
        grp.critic_h[0].copy_(hst["critic_hidden_state"][gi])


def make_system(name: str, centralised: bool) -> SimpleNamespace:
    """The reference's public functions of ``rec_ippo`` (``centralised`` False) or ``rec_mappo`` (True)."""

    def get_learner_fn(env, apply_fns, update_fns, config):
        """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps (rec_mappo.py:60-394).

            apply_fns  = (actor_apply_fn, critic_apply_fn)       rec_mappo.py:67
            update_fns = (actor_update_fn, critic_update_fn)     rec_mappo.py:68

        Under the rule of rec_sable.get_learner_fn: the callables must be the bound methods ``GruActor.apply`` / ``GruCritic.apply`` and
        ``ClipAdam.update`` of the objects that own the device buffers (or thin functools.wraps / functools.partial adaptors around them),
        and the loop CALLS exactly what it is given; anything else raises the ``TypeError`` of common._owner."""
        actor_apply_fn, critic_apply_fn = apply_fns
        actor_update_fn, critic_update_fn = update_fns
        critic = _owner(critic_apply_fn, GruCritic, "apply", "apply_fns[1] (critic_apply_fn)")
        actor = _owner(actor_apply_fn, GruActor, "apply", "apply_fns[0] (actor_apply_fn)")
        if isinstance(actor, GruCritic):
            raise TypeError("get_learner_fn: apply_fns[0] (actor_apply_fn) must belong to a GruActor, not to the critic")
        a_opt = _owner(actor_update_fn, ClipAdam, "update", "update_fns[0] (actor_update_fn)")
        c_opt = _owner(critic_update_fn, ClipAdam, "update", "update_fns[1] (critic_update_fn)")
        if a_opt.net is not actor or c_opt.net is not critic:
            raise ValueError("update_fns must be the update functions of the optimisers of (actor, critic), in this order")
        check_chunk_size(config.system.get("recurrent_chunk_size"), int(config.system.rollout_length))
        _, world = mdist.rank_world()
        learner = PpoLearner(env.cfg, int(config.arch.num_envs), a_opt.sys, actor.dev, centralised=centralised,
                             num_groups=int(config.system.update_batch_size), actor=actor, critic=critic, optims=(a_opt, c_opt),
                             apply_fns=tuple(apply_fns), update_fns=tuple(update_fns))
        grad_sync = mdist.make_grad_sync(world)   # the four pmeans of rec_mappo.py:252-266: one all-reduce of [actor | critic | loss scalars]
        return make_learner_fn(learner, config, grad_sync, _snapshot_state, load_learner_state, list(LOSS_NAMES))

    def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
        """Initialise learner_fn, networks, optimisers, environments and states (rec_mappo.py:397-535)."""
        key, actor_net_key, critic_net_key = keys
        config.system.num_agents = env.num_agents
        if int(config.network.hidden_state_dim) != 128:
            raise NotImplementedError("HIP kernels support hidden_state_dim=128")
        check_chunk_size(config.system.get("recurrent_chunk_size"), int(config.system.rollout_length))
        device = device or torch.device("cuda", torch.cuda.current_device())
        cfg, sysc = env.cfg, system_config(config)
        csys = dataclasses.replace(sysc, actor_lr=float(config.system.critic_lr))   # ClipAdam reads its rate as actor_lr
        obs_ld = obs_row_stride(cfg.obs_dim)
        a_pre, a_post = network_torsos(config, "actor_network")
        c_pre, c_post = network_torsos(config, "critic_network")
        if centralised:   # observation.global_state: the raw views of all agents (environments.make checked the width)
            cF = cfg.num_agents * raw_features(cfg)
            cld = global_state_ld(cfg.num_agents, raw_features(cfg))
        else:
            cF, cld = env.obs_dim, obs_ld
        # parameters = what flax creates from actor_net_key / critic_net_key (rec_mappo.py:463-466; UNPINNED restatement, magpo_amd/params.py)
        actor_network = GruActor(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_ld, seed=np.asarray(actor_net_key, np.uint32),
                                 pre_torso=a_pre, post_torso=a_post)
        critic_network = GruCritic(cfg.num_agents, cF, device, centralised=centralised, obs_ld=cld, seed=np.asarray(critic_net_key, np.uint32),
                                   tuning=actor_network.tuning, pre_torso=c_pre, post_torso=c_post)
        actor_optim, critic_optim = ClipAdam(actor_network, sysc), ClipAdam(critic_network, csys)
        apply_fns = (actor_network.apply, critic_network.apply)
        update_fns = (actor_optim.update, critic_optim.update)
        learn = get_learner_fn(env, apply_fns, update_fns, config)
        return learn, actor_network, setup_learner(learn, key, _snapshot_state, rank, world)

    def run_experiment(_config) -> float:
        """Runs experiment (rec_mappo.py:538-677)."""
        config, rank, world, device = start_experiment(_config, name)
        # recurrent_chunk_size (rec_mappo.py:545-555): null means the rollout length
        check_chunk_size(config.system.get("recurrent_chunk_size"), int(config.system.rollout_length))
        if config.system.get("recurrent_chunk_size") is None:
            config.system.recurrent_chunk_size = config.system.rollout_length
        assert config.arch.num_envs % config.system.num_minibatches == 0, "Number of envs must be divisibile by number of minibatches."

        env, eval_env = environments.make(config, add_global_state=centralised)
        ks = host_split(prng_key(int(config.system.seed)), 4)
        key, key_e, actor_net_key, critic_net_key = ks[0], ks[1], ks[2], ks[3]
        learn, actor_network, learner_state = learner_setup(env, (key, actor_net_key, critic_net_key), config, device, rank, world)
        return train_and_evaluate_gru_actor(config, env, eval_env, learn, actor_network, learner_state, key, key_e, device, rank, world)

    def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
        """Experiment entry point (rec_mappo.py:680-693): compose configs/default/<system>.yaml + CLI overrides."""
        cfg = compose(name, sys.argv[1:] if overrides is None else overrides)
        perf = run_experiment(cfg)
        print(f"Recurrent {'MAPPO' if centralised else 'IPPO'} experiment completed")
        return perf

    return SimpleNamespace(get_learner_fn=get_learner_fn, learner_setup=learner_setup, run_experiment=run_experiment,
                           hydra_entry_point=hydra_entry_point)
