"""The one implementation behind the two recurrent PPO systems, rec_ippo and rec_mappo (mava/systems/ppo/anakin/rec_ippo.py, rec_mappo.py).

The two reference files differ in three places only: ``centralised_critic`` of the critic network (rec_mappo.py:429), ``add_global_state``
of the env factory (:558) and the system name (:540).  ``make_system(name, centralised)`` returns the reference's public functions for one
of them; rec_ippo.py / rec_mappo.py bind them at module level under the reference's names.  The bodies drive the HIP kernels
(magpo_amd.ppo_learner.PpoLearner); the experiment loop, the learner loop and the shared parts of the learner state are the ones every
system uses (magpo_amd/systems/common.py).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.actor import GruActor
from magpo_amd.critic import GruCritic
from magpo_amd.learner import host_split, obs_row_stride, prng_key
from magpo_amd.optim import ClipAdam
from magpo_amd.ppo_learner import LOSS_NAMES, PpoLearner, check_chunk_size
from magpo_amd.systems.common import (as_dict, entry_point, make_learner_fn, network_torsos, setup_learner, start_experiment,
                                      train_and_evaluate_actor)
from magpo_amd.systems.ppo.anakin.ppo_common import critic_input, critic_system_config, load_shared, owners, snapshot_shared, system_config  # noqa: F401
from magpo_amd.systems.ppo.types import HiddenStates, RNNLearnerState
from magpo_amd.utils import make_env as environments


def _snapshot_state(learner: PpoLearner) -> RNNLearnerState:
    """RNNLearnerState of the learner as an independent COPY (rec_mappo.py:353-361); leaves carry a leading group axis."""
    gs = learner.groups
    return RNNLearnerState(*snapshot_shared(learner),
                           HiddenStates(torch.stack([g.policy_h[0] for g in gs]), torch.stack([g.critic_h[0] for g in gs])))


def load_learner_state(learner: PpoLearner, state: RNNLearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    hst = as_dict(state.hstates)
    load_shared(learner, state)
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
        actor, critic, a_opt, c_opt = owners(apply_fns, update_fns, GruActor, GruCritic, "a GruActor")
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
        csys = critic_system_config(sysc, config)
        obs_ld = obs_row_stride(cfg.obs_dim)
        a_pre, a_post = network_torsos(config, "actor_network")
        c_pre, c_post = network_torsos(config, "critic_network")
        cF, cld = critic_input(env, centralised)
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
        return train_and_evaluate_actor(config, env, eval_env, learn, actor_network, learner_state, key, key_e, device, rank, world)

    def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
        """Experiment entry point (rec_mappo.py:680-693): compose configs/default/<system>.yaml + CLI overrides."""
        return entry_point(name, run_experiment, f"Recurrent {'MAPPO' if centralised else 'IPPO'} experiment completed", overrides)

    return SimpleNamespace(get_learner_fn=get_learner_fn, learner_setup=learner_setup, run_experiment=run_experiment,
                           hydra_entry_point=hydra_entry_point)
