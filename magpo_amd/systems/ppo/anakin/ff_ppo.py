"""The one implementation behind the two feed-forward PPO systems, ff_ippo and ff_mappo (mava/systems/ppo/anakin/ff_ippo.py, ff_mappo.py).

As with the recurrent pair the two reference files differ in ``centralised_critic`` of the critic network, ``add_global_state`` of the env
factory and the system name.  ``make_system(name, centralised)`` returns the reference's public functions for one of them; ff_ippo.py /
ff_mappo.py bind them at module level under the reference's names.  The bodies drive the HIP kernels (magpo_amd.ff_ppo_learner.FfPpoLearner);
the experiment loop, the learner loop and the shared parts of the learner state are the ones every system uses (magpo_amd/systems/common.py).

Supported: discrete action spaces; MLPTorso pre-torsos inside magpo_amd.torso.TorsoSpec; for ff_mappo a global state of at most 128 inputs.
Anything else raises NotImplementedError at set-up.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.ff_nets import FF_DEFAULT_TORSO, FfActor, FfCritic
from magpo_amd.ff_ppo_learner import FfPpoLearner
from magpo_amd.learner import host_split, obs_row_stride, prng_key
from magpo_amd.optim import ClipAdam
from magpo_amd.ppo_learner import LOSS_NAMES
from magpo_amd.systems import common
from magpo_amd.systems.common import entry_point, make_learner_fn, setup_learner, start_experiment, train_and_evaluate_actor
from magpo_amd.systems.ppo.anakin.ppo_common import critic_input, critic_system_config, load_shared, owners, snapshot_shared, system_config  # noqa: F401
from magpo_amd.systems.ppo.types import LearnerState
from magpo_amd.torso import torso_from_config
from magpo_amd.utils import make_env as environments


def network_torso(config, which: str):
    """The TorsoSpec of ``network.actor_network.pre_torso`` / ``network.critic_network.pre_torso`` (ff_mappo.py:297-302 instantiate them as
    MLPTorso); feed-forward networks have no post-torso.  What the HIP kernels do not cover raises NotImplementedError (magpo_amd/torso.py)."""
    node = config.network.get(which)
    if node is None or "pre_torso" not in node:
        return FF_DEFAULT_TORSO
    if "post_torso" in node:
        raise NotImplementedError(f"network.{which}.post_torso: the feed-forward networks of ff_ippo / ff_mappo have a pre_torso only (configs/network/mlp.yaml)")
    return torso_from_config(node.pre_torso)


def check_action_space(config) -> None:
    """Discrete actions only (the masked categorical head); the reference's continuous head (TanhTransformedDistribution) is not built."""
    common.check_action_space(config, "ff_ippo / ff_mappo support discrete action spaces only (DiscreteActionHead)",
                              "; continuous actions are not implemented")


def _snapshot_state(learner: FfPpoLearner) -> LearnerState:
    """LearnerState of the learner as an independent COPY (ff_mappo.py:264); leaves carry a leading group axis."""
    return LearnerState(*snapshot_shared(learner))


def load_learner_state(learner: FfPpoLearner, state: LearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    load_shared(learner, state)


def make_system(name: str, centralised: bool) -> SimpleNamespace:
    """The reference's public functions of ``ff_ippo`` (``centralised`` False) or ``ff_mappo`` (True)."""

    def get_learner_fn(env, apply_fns, update_fns, config):
        """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps (ff_mappo.py:45-296).

            apply_fns  = (actor_apply_fn, critic_apply_fn)       ff_mappo.py:52
            update_fns = (actor_update_fn, critic_update_fn)     ff_mappo.py:53

        Under the rule of rec_sable.get_learner_fn: the callables must be the bound methods ``FfActor.apply`` / ``FfCritic.apply`` and
        ``ClipAdam.update`` of the objects that own the device buffers (or thin functools.wraps / functools.partial adaptors around them),
        and the loop CALLS exactly what it is given; anything else raises the ``TypeError`` of common._owner."""
        actor, critic, a_opt, c_opt = owners(apply_fns, update_fns, FfActor, FfCritic, "an FfActor")
        _, world = mdist.rank_world()
        learner = FfPpoLearner(env.cfg, int(config.arch.num_envs), a_opt.sys, actor.dev, centralised=centralised,
                               num_groups=int(config.system.update_batch_size), actor=actor, critic=critic, optims=(a_opt, c_opt),
                               apply_fns=tuple(apply_fns), update_fns=tuple(update_fns))
        grad_sync = mdist.make_grad_sync(world)   # the four pmeans of ff_mappo.py:192-206: one all-reduce of [actor | critic | loss scalars]
        return make_learner_fn(learner, config, grad_sync, _snapshot_state, load_learner_state, list(LOSS_NAMES))

    def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
        """Initialise learner_fn, networks, optimisers, environments and states (ff_mappo.py:278-380)."""
        key, actor_net_key, critic_net_key = keys
        config.system.num_agents = env.num_agents
        check_action_space(config)
        device = device or torch.device("cuda", torch.cuda.current_device())
        cfg, sysc = env.cfg, system_config(config)
        csys = critic_system_config(sysc, config)
        obs_ld = obs_row_stride(cfg.obs_dim)
        a_torso, c_torso = network_torso(config, "actor_network"), network_torso(config, "critic_network")
        cF, cld = critic_input(env, centralised)
        # parameters = what flax creates from actor_net_key / critic_net_key (ff_mappo.py:311-312; UNPINNED restatement, magpo_amd/params.py)
        actor_network = FfActor(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_ld, seed=np.asarray(actor_net_key, np.uint32),
                                torso=a_torso)
        critic_network = FfCritic(cfg.num_agents, cF, device, centralised=centralised, obs_ld=cld, seed=np.asarray(critic_net_key, np.uint32),
                                  tuning=actor_network.tuning, torso=c_torso)
        actor_optim, critic_optim = ClipAdam(actor_network, sysc), ClipAdam(critic_network, csys)
        apply_fns = (actor_network.apply, critic_network.apply)
        update_fns = (actor_optim.update, critic_optim.update)
        learn = get_learner_fn(env, apply_fns, update_fns, config)
        return learn, actor_network, setup_learner(learn, key, _snapshot_state, rank, world)

    def run_experiment(_config) -> float:
        """Runs experiment (ff_mappo.py:383-510)."""
        config, rank, world, device = start_experiment(_config, name)
        if int(config.system.get("micro_batches", 1) or 1) != 1:
            raise NotImplementedError("system.micro_batches is not supported by ff_ippo / ff_mappo")
        env, eval_env = environments.make(config, add_global_state=centralised)
        ks = host_split(prng_key(int(config.system.seed)), 4)
        key, key_e, actor_net_key, critic_net_key = ks[0], ks[1], ks[2], ks[3]
        learn, actor_network, learner_state = learner_setup(env, (key, actor_net_key, critic_net_key), config, device, rank, world)
        return train_and_evaluate_actor(config, env, eval_env, learn, actor_network, learner_state, key, key_e, device, rank, world)

    def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
        """Experiment entry point (ff_mappo.py:513-526): compose configs/default/<system>.yaml + CLI overrides."""
        return entry_point(name, run_experiment, f"{'MAPPO' if centralised else 'IPPO'} experiment completed", overrides)

    return SimpleNamespace(get_learner_fn=get_learner_fn, learner_setup=learner_setup, run_experiment=run_experiment,
                           hydra_entry_point=hydra_entry_point)
