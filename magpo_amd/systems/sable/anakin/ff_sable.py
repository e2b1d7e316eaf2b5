"""Memoryless Sable system entry point on MI355X -- drop-in for mava/systems/sable/anakin/ff_sable.py: Sable with retention over the
agents of one time step only (no hidden states, no decay, no timestep positional encoding), trained with PPO on shuffled single steps.

Same public names and call contract as the reference system file:
    hydra_entry_point / main(overrides)      ff_sable.py:559-573
    run_experiment(config) -> float          ff_sable.py:458-556   (make_ff_sable_act_fn :475-486)
    learner_setup(env, keys, config) -> (learn, sable_execution_fn, init_learner_state)   ff_sable.py:324-455
    get_learner_fn(env, apply_fns, update_fn, config) -> LearnerFn                        ff_sable.py:52-321
The bodies drive the HIP kernels (magpo_amd.ff_sable_learner.FfSableLearner); the experiment loop, the learner loop and the shared parts
of the learner state are the ones every system uses (magpo_amd/systems/common.py).

Supported: discrete action spaces, all five environments, ``memory_config.agents_chunk_size`` null (full retention over the team).

    python -m magpo_amd.systems.sable.anakin.ff_sable env=coordsum env/scenario=3x30-50 arch.num_envs=64
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.evaluator import sable_eval_act_fn
from magpo_amd.ff_sable_learner import LOSS_NAMES, FfSableLearner
from magpo_amd.learner import SystemConfig, host_split, obs_row_stride, prng_key
from magpo_amd.optim import ClipAdam
from magpo_amd.sable import SableGuider
from magpo_amd.systems import common
from magpo_amd.systems.common import (_owner, _system_config, entry_point, load_opt_state, load_rollout_state, make_learner_fn, setup_learner,
                                      snapshot_opt_state, snapshot_rollout_state, start_experiment, train_and_evaluate)
from magpo_amd.systems.sable.types import FFLearnerState, Transition  # noqa: F401
from magpo_amd.types import ExperimentOutput  # noqa: F401
from magpo_amd.utils import make_env as environments

LearnerState = FFLearnerState


def system_config(config) -> SystemConfig:
    """The learner's settings from an ff_sable config tree (no ``clip_gpo`` / ``alpha``: MAGPO's keys, never read here)."""
    return _system_config(config, clip_gpo=SystemConfig.clip_gpo, alpha=SystemConfig.alpha)


def check_action_space(config) -> None:
    """Discrete actions only; the reference's continuous head is not built."""
    common.check_action_space(config, "ff_sable supports discrete action spaces only")


def configure_memory(config, num_agents: int) -> None:
    """What learner_setup writes into ``network.memory_config`` (ff_sable.py:339-350): a dummy decay factor of 1, the chunk size = the
    number of agents, no timestep positional encoding.  ``agents_chunk_size`` other than null would evaluate the team in chunks of agents
    with a carried state -- the thing the stateless team kernels exist to avoid -- and is not built."""
    mc = config.network.memory_config
    if mc.type != "ff_sable":
        raise NotImplementedError("memory_config.type must be ff_sable")
    mc.decay_scaling_factor = 1.0
    if mc.get("agents_chunk_size"):
        raise NotImplementedError(f"network.memory_config.agents_chunk_size={mc.agents_chunk_size}: only null (full retention over the "
                                  "team in one chunk) is supported; chunks of agents need a carried retention state")
    mc.chunk_size = int(num_agents)
    mc.timestep_positional_encoding = False


def _snapshot_state(learner: FfSableLearner) -> FFLearnerState:
    """LearnerState of the learner as an independent COPY (ff_sable.py:284-290); leaves carry a leading group axis.  ``timestep`` holds
    what the next rollout reads of the reference's TimeStep: the observation and ``last``."""
    gs = learner.groups
    params = {k: v.clone() for k, v in learner.guider.named.items()}
    env_state, timestep, timestep_last = snapshot_rollout_state(gs)
    timestep["last"] = timestep_last
    return FFLearnerState(params, snapshot_opt_state(learner.g_opt), gs[0].key.copy(), env_state, timestep)


def load_learner_state(learner: FfSableLearner, state: FFLearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    learner.guider.load_named(state.params)
    load_opt_state(learner.g_opt, state.opt_states)
    load_rollout_state(learner.groups, state.key, state.env_state, state.timestep, state.timestep["last"])


def get_learner_fn(env, apply_fns, update_fn, config):
    """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps (ff_sable.py:52-321).

        apply_fns = (sable_action_select_fn, sable_apply_fn)     ff_sable.py:61   (execution / training)
        update_fn = the optimiser's update function              ff_sable.py:55

    Under the rule of rec_sable.get_learner_fn: the callables must be the bound methods ``SableGuider.act`` (the stateless acting chain) or
    ``SableGuider.act_team_fused`` (the same step in one launch),
    ``SableGuider.apply`` and ``ClipAdam.update`` of the objects that own the device buffers (or thin functools.wraps / functools.partial
    adaptors around them), and the loop CALLS exactly what it is given; anything else raises the ``TypeError`` of common._owner."""
    return learner_fn_for(SableGuider, env, apply_fns, update_fn, config)


def learner_fn_for(net_cls, env, apply_fns, update_fn, config):
    """``get_learner_fn`` for the memoryless network class ``net_cls`` (SableGuider; magpo_amd.mat.MatNetwork for the mat system, whose
    learner is this one, mava/systems/mat/anakin/mat.py:82-283)."""
    sable_action_select_fn, sable_apply_fn = apply_fns
    guider = _owner(sable_apply_fn, net_cls, "apply", "apply_fns[1] (sable_apply_fn)")
    if _owner(sable_action_select_fn, net_cls, "act", "apply_fns[0] (sable_action_select_fn)") is not guider:
        raise ValueError("the execution and the training function must belong to one Sable network")
    optim = _owner(update_fn, ClipAdam, "update", "update_fn")
    _, world = mdist.rank_world()
    learner = FfSableLearner(env.cfg, int(config.arch.num_envs), optim.sys, guider.dev, num_groups=int(config.system.update_batch_size),
                             guider=guider, optim=optim, apply_fns=tuple(apply_fns), update_fn=update_fn)
    grad_sync = mdist.make_grad_sync(world)   # the two pmeans of ff_sable.py:226-228: one all-reduce of [gradients | 4 loss scalars]
    return make_learner_fn(learner, config, grad_sync, _snapshot_state, load_learner_state, list(LOSS_NAMES))


def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
    """Initialise learner_fn, network, optimiser, environments and states (ff_sable.py:324-455)."""
    key, net_key = keys
    config.system.num_agents = env.num_agents
    check_action_space(config)
    if int(config.system.get("micro_batches", 1) or 1) != 1:
        raise NotImplementedError("system.micro_batches is not supported by ff_sable")
    configure_memory(config, env.num_agents)
    nc = config.network.net_config
    if int(nc.embed_dim) not in (16, 32, 64, 128) or int(nc.n_head) not in (1, 2, 4):
        raise NotImplementedError("HIP kernels support embed_dim in {16,32,64,128}, n_head in {1,2,4} (any n_block)")
    device = device or torch.device("cuda", torch.cuda.current_device())
    cfg, sysc = env.cfg, system_config(config)
    # parameters = what flax creates from net_key (ff_sable.py:378-384; magpo_amd/params.py): the parameter tree is rec_sable's
    sable_network = SableGuider(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_row_stride(cfg.obs_dim), embed_dim=int(nc.embed_dim),
                                n_head=int(nc.n_head), n_block=int(nc.n_block), memory_type="ff_sable", max_pos=cfg.time_limit + 1,
                                seed=np.asarray(net_key, np.uint32))
    optim = ClipAdam(sable_network, sysc)
    apply_fns = (sable_network.act, sable_network.apply)   # execution function, training function (ff_sable.py:396-401)
    # the rollout's action-select function follows Tuning.ff_sable_fused_act: the one-launch step, or the chain that is returned as the
    # execution function either way
    learn = get_learner_fn(env, (acting_fn(sable_network), apply_fns[1]), optim.update, config)
    return learn, apply_fns[0], setup_learner(learn, key, _snapshot_state, rank, world)


def acting_fn(net: SableGuider) -> Callable:
    """The acting step of a memoryless network under its tuning: ``act_team_fused`` (magpo_ff_sable_act, one launch) with
    ``Tuning.ff_sable_fused_act`` on, else the kernel-by-kernel chain ``act``."""
    return net.act_team_fused if net.tuning.ff_sable_fused_act else net.act


def make_ff_sable_eval_act_fn(actor_apply_fn: Callable) -> Callable:
    """``EvalActFn(params, timestep, key, actor_state) -> (action, {})`` that executes the Sable network itself, statelessly
    (ff_sable.py:475-486).  ``actor_apply_fn``: ``SableGuider.act`` or ``.act_team_fused`` (see ``acting_fn``) of the network that evaluates (its own object, so that loading the
    evaluated parameters does not touch the learner's).  As in the reference the action is always SAMPLED from ``key``.  Parameters are
    loaded when a DIFFERENT dict object arrives than the last one (see rec_sable.make_rec_sable_act_fn)."""
    net = _owner(actor_apply_fn, SableGuider, "act", "actor_apply_fn")
    if not net.ff:
        raise ValueError("make_ff_sable_eval_act_fn needs a SableGuider with memory_type='ff_sable'")
    return sable_eval_act_fn(net, actor_apply_fn, stateful=False)


def run_experiment(_config) -> float:
    """Runs experiment (ff_sable.py:458-556)."""
    config, rank, world, device = start_experiment(_config, "ff_sable")
    env, eval_env = environments.make(config)
    ks = host_split(prng_key(int(config.system.seed)), 3)
    key, key_e, net_key = ks[0], ks[1], ks[2]
    learn, sable_execution_fn, learner_state = learner_setup(env, (key, net_key), config, device, rank, world)

    # the evaluator runs the Sable network on its own batch of envs, with the pre-interval parameters: a second network object
    eval_net = learn.learner.guider.twin()
    return train_and_evaluate(config, env, eval_env, learn, learner_state, make_ff_sable_eval_act_fn(acting_fn(eval_net)), key, key_e, device, rank, world,
                              init_act_state=lambda batch: {}, eval_params=lambda state: state.params)


def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
    """Experiment entry point (ff_sable.py:559-573): compose configs/default/ff_sable.yaml + CLI overrides."""
    return entry_point("ff_sable", run_experiment, "FF Sable experiment completed", overrides)


if __name__ == "__main__":
    hydra_entry_point()
