"""Multi-Agent Transformer system entry point on MI355X -- drop-in for mava/systems/mat/anakin/mat.py: an encoder-decoder transformer over
the agents of one time step, acting autoregressively over the agents, trained with PPO on shuffled single steps.

Same public names and call contract as the reference system file:
    hydra_entry_point / main(overrides)      mat.py:546-560
    run_experiment(config) -> float          mat.py:407-543   (eval_act_fn :425-443: make_mat_eval_act_fn)
    learner_setup(env, keys, config) -> (learn, actor_network, init_learner_state)        mat.py:310-404
    get_learner_fn(env, apply_fns, update_fn, config) -> LearnerFn                        mat.py:56-307
The learner is the memoryless Sable system's (mat.py:82-283 is ff_sable.py:83-283 with another network): FfSableLearner given a
MatNetwork, behind the learner-function, state and experiment code of systems/sable/anakin/ff_sable.py and systems/common.py.

Supported: discrete action spaces, all five environments, embed_dim 64, n_head 1 / 2 / 4, any n_block; ``use_rmsnorm``, ``use_swiglu``
and ``system.normalise_value_targets`` true raise NotImplementedError.

    python -m magpo_amd.systems.mat.anakin.mat env=coordsum env/scenario=3x30-50 arch.num_envs=64
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from magpo_amd.evaluator import sable_eval_act_fn
from magpo_amd.learner import host_split, obs_row_stride, prng_key
from magpo_amd.mat import MatNetwork, check_net_config
from magpo_amd.optim import ClipAdam
from magpo_amd.systems import common
from magpo_amd.systems.common import _owner, entry_point, setup_learner, start_experiment, train_and_evaluate
from magpo_amd.systems.mat.types import LearnerState, MATNetworkConfig, Transition  # noqa: F401
from magpo_amd.systems.sable.anakin import ff_sable
from magpo_amd.systems.sable.anakin.ff_sable import _snapshot_state, load_learner_state, system_config  # noqa: F401
from magpo_amd.types import ExperimentOutput  # noqa: F401
from magpo_amd.utils import make_env as environments


def network_config(config) -> MATNetworkConfig:
    """``config.network`` (configs/network/transformer.yaml) as the reference's MATNetworkConfig; what the kernels do not evaluate raises."""
    n = config.network
    nc = MATNetworkConfig(int(n.n_block), int(n.n_head), int(n.embed_dim), bool(n.get("use_swiglu", False)), bool(n.get("use_rmsnorm", False)))
    check_net_config(nc.embed_dim, nc.n_head, nc.n_block, nc.use_rmsnorm, nc.use_swiglu)
    return nc


def check_system(config) -> None:
    common.check_action_space(config, "mat supports discrete action spaces only")
    if bool(config.system.get("normalise_value_targets", False)):
        raise NotImplementedError("system.normalise_value_targets=true is not supported")
    if int(config.system.get("micro_batches", 1) or 1) != 1:
        raise NotImplementedError("system.micro_batches is not supported by mat")


def get_learner_fn(env, apply_fns, update_fn, config):
    """Returns ``learn(learner_state) -> ExperimentOutput`` (mat.py:56-307): ff_sable's learner function around a MatNetwork.
    apply_fns = (actor_action_select_fn, actor_apply_fn) must be the bound methods ``MatNetwork.act`` and ``MatNetwork.apply`` of one
    network and update_fn ``ClipAdam.update`` of its optimiser (see ff_sable.get_learner_fn)."""
    return ff_sable.learner_fn_for(MatNetwork, env, apply_fns, update_fn, config)


def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
    """Initialise learner_fn, network, optimiser, environments and states (mat.py:310-404)."""
    key, actor_net_key = keys
    config.system.num_agents = env.num_agents
    check_system(config)
    nc = network_config(config)
    device = device or torch.device("cuda", torch.cuda.current_device())
    cfg = env.cfg
    # parameters = what flax creates from actor_net_key (mat.py:353; magpo_amd/params.py: init_mat_from_key)
    actor_network = MatNetwork(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_row_stride(cfg.obs_dim), embed_dim=nc.embed_dim,
                               n_head=nc.n_head, n_block=nc.n_block, use_rmsnorm=nc.use_rmsnorm, use_swiglu=nc.use_swiglu,
                               seed=np.asarray(actor_net_key, np.uint32))
    optim = ClipAdam(actor_network, system_config(config))
    learn = get_learner_fn(env, (actor_network.act, actor_network.apply), optim.update, config)   # mat.py:357-362
    return learn, actor_network, setup_learner(learn, key, _snapshot_state, rank, world)


def make_mat_eval_act_fn(actor_apply_fn: Callable) -> Callable:
    """``EvalActFn(params, timestep, key, actor_state) -> (action, {})`` that executes the network itself (mat.py:425-443): the action
    is always SAMPLED from ``key``.  ``actor_apply_fn``: ``MatNetwork.act`` of the network that evaluates (its own object, so that loading
    the evaluated parameters does not touch the learner's)."""
    return sable_eval_act_fn(_owner(actor_apply_fn, MatNetwork, "act", "actor_apply_fn"), actor_apply_fn, stateful=False)


def run_experiment(_config) -> float:
    """Runs experiment (mat.py:407-543)."""
    config, rank, world, device = start_experiment(_config, "mat")
    env, eval_env = environments.make(config)
    ks = host_split(prng_key(int(config.system.seed)), 3)
    key, key_e, actor_net_key = ks[0], ks[1], ks[2]
    learn, actor_network, learner_state = learner_setup(env, (key, actor_net_key), config, device, rank, world)
    eval_net = actor_network.twin()   # the evaluator runs the network on its own batch of envs, with the pre-interval parameters
    return train_and_evaluate(config, env, eval_env, learn, learner_state, make_mat_eval_act_fn(eval_net.act), key, key_e, device, rank, world,
                              init_act_state=lambda batch: {}, eval_params=lambda state: state.params)


def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
    """Experiment entry point (mat.py:546-560): compose configs/default/mat.yaml + CLI overrides."""
    return entry_point("mat", run_experiment, "MAT experiment completed", overrides)


if __name__ == "__main__":
    hydra_entry_point()
