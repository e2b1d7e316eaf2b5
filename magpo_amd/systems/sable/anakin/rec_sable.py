"""Sable system entry point on MI355X -- drop-in for mava/systems/sable/anakin/rec_sable.py: the guider of MAGPO trained alone with PPO.

Same public names and call contract as the reference system file:
    hydra_entry_point / main(overrides)      rec_sable.py:623-636
    run_experiment(config) -> float          rec_sable.py:481-620   (make_rec_sable_act_fn :498-513)
    learner_setup(env, keys, config) -> (learn, sable_execution_fn, init_learner_state)   rec_sable.py:351-478
    get_learner_fn(env, apply_fns, update_fn, config) -> LearnerFn                        rec_sable.py:53-348
The bodies drive the HIP kernels (magpo_amd.sable_learner.SableLearner); the experiment loop, the learner loop and the state layout
helpers are the ones every system uses (magpo_amd/systems/common.py, magpo_amd/sable.py).

    python -m magpo_amd.systems.sable.anakin.rec_sable env=coordsum env/scenario=3x30-50 arch.num_envs=64
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.evaluator import sable_eval_act_fn
from magpo_amd.learner import SystemConfig, host_split, obs_row_stride, prng_key
from magpo_amd.optim import ClipAdam
from magpo_amd.sable import SableGuider, load_sable_hstates, sable_hstates_logical
from magpo_amd.sable_learner import LOSS_NAMES, SableLearner
from magpo_amd.systems.common import (_owner, _system_config, as_dict, entry_point, load_opt_state, load_rollout_state, make_learner_fn,
                                      setup_learner, snapshot_opt_state, snapshot_rollout_state, start_experiment, train_and_evaluate)
from magpo_amd.systems.sable.types import HiddenStates, LearnerState, Transition  # noqa: F401
from magpo_amd.types import ExperimentOutput  # noqa: F401
from magpo_amd.utils import make_env as environments


def system_config(config) -> SystemConfig:
    """The learner's settings from a rec_sable config tree: it has no ``clip_gpo`` / ``alpha`` (MAGPO's keys, which rec_magpo requires and
    this system never reads), so they take SystemConfig's defaults."""
    return _system_config(config, clip_gpo=SystemConfig.clip_gpo, alpha=SystemConfig.alpha)


def _snapshot_state(learner: SableLearner) -> LearnerState:
    """LearnerState of the learner as an independent COPY (rec_sable.py:309-316); leaves carry a leading group axis.  ``timestep``
    holds what the next rollout reads of the reference's TimeStep: the observation and ``last`` (= timestep.last(), the done flag
    the first transition records, rec_sable.py:112)."""
    gs, gd = learner.groups, learner.guider
    params = {k: v.clone() for k, v in gd.named.items()}
    hs = HiddenStates(*[torch.stack([sable_hstates_logical(gd, g.sable_hs[i]) for g in gs]) for i in range(3)])
    env_state, timestep, timestep_last = snapshot_rollout_state(gs)
    timestep["last"] = timestep_last
    return LearnerState(params, snapshot_opt_state(learner.g_opt), gs[0].key.copy(), env_state, timestep, hs)


def load_learner_state(learner: SableLearner, state: LearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    learner.guider.load_named(state.params)
    load_opt_state(learner.g_opt, state.opt_states)
    hst = as_dict(state.hstates)
    sable = (hst["encoder"], hst["decoder_self_retn"], hst["decoder_cross_retn"])
    load_rollout_state(learner.groups, state.key, state.env_state, state.timestep, state.timestep["last"])
    for gi, grp in enumerate(learner.groups):
        for i in range(3):
            load_sable_hstates(learner.guider, grp.sable_hs[i], sable[i][gi])


def get_learner_fn(env, apply_fns, update_fn, config):
    """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps (rec_sable.py:53-348).

        apply_fns = (sable_action_select_fn, sable_apply_fn)     rec_sable.py:62   (execution / training)
        update_fn = the optimiser's update function              rec_sable.py:56

    As in the MAGPO system the callables must be methods of the objects that own the device buffers -- ``SableGuider.get_actions``,
    ``SableGuider.apply`` and ``ClipAdam.update``, or thin ``functools.wraps`` / ``functools.partial`` adaptors around them -- and the
    loop CALLS exactly what it is given; anything else raises the ``TypeError`` of common._owner.  State in, state out: a state
    other than the last one produced is loaded into the buffers first, so ``learn`` is a function of its argument."""
    sable_action_select_fn, sable_apply_fn = apply_fns
    guider = _owner(sable_apply_fn, SableGuider, "apply", "apply_fns[1] (sable_apply_fn)")
    if _owner(sable_action_select_fn, SableGuider, "get_actions", "apply_fns[0] (sable_action_select_fn)") is not guider:
        raise ValueError("the execution and the training function must belong to one Sable network")
    optim = _owner(update_fn, ClipAdam, "update", "update_fn")
    _, world = mdist.rank_world()
    learner = SableLearner(env.cfg, int(config.arch.num_envs), optim.sys, guider.dev, num_groups=int(config.system.update_batch_size),
                           guider=guider, optim=optim, apply_fns=tuple(apply_fns), update_fn=update_fn)
    grad_sync = mdist.make_grad_sync(world)   # the two pmeans of rec_sable.py:242-244: one all-reduce of [gradients | 4 loss scalars]
    return make_learner_fn(learner, config, grad_sync, _snapshot_state, load_learner_state, list(LOSS_NAMES))


def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
    """Initialise learner_fn, network, optimiser, environments and states (rec_sable.py:351-478)."""
    key, net_key = keys
    config.system.num_agents = env.num_agents
    nc, mc = config.network.net_config, config.network.memory_config
    # chunk size: a memory / speed knob of the reference's chunkwise evaluation with no effect on the function (see rec_magpo.learner_setup)
    if mc.timestep_chunk_size:
        mc.chunk_size = int(mc.timestep_chunk_size) * env.num_agents
    else:
        mc.chunk_size = config.system.rollout_length * env.num_agents
    if mc.type != "rec_sable":
        raise NotImplementedError("memory_config.type must be rec_sable")
    if int(nc.embed_dim) not in (16, 32, 64, 128) or int(nc.n_head) not in (1, 2, 4):
        raise NotImplementedError("HIP kernels support embed_dim in {16,32,64,128}, n_head in {1,2,4} (any n_block)")
    device = device or torch.device("cuda", torch.cuda.current_device())
    cfg, sysc = env.cfg, system_config(config)
    # parameters = what flax creates from net_key (rec_sable.py:403-409; magpo_amd/params.py)
    sable_network = SableGuider(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_row_stride(cfg.obs_dim), embed_dim=int(nc.embed_dim),
                                n_head=int(nc.n_head), n_block=int(nc.n_block), decay_scaling_factor=float(mc.decay_scaling_factor),
                                use_pe=bool(mc.timestep_positional_encoding), max_pos=cfg.time_limit + 1, seed=np.asarray(net_key, np.uint32))
    optim = ClipAdam(sable_network, sysc)
    apply_fns = (sable_network.get_actions, sable_network.apply)   # execution function, training function (rec_sable.py:413-416)
    learn = get_learner_fn(env, apply_fns, optim.update, config)
    return learn, apply_fns[0], setup_learner(learn, key, _snapshot_state, rank, world)


def get_init_hidden_state(sable_network: SableGuider, batch_size: int) -> torch.Tensor:
    """Zero Sable hidden states of the evaluator's act function for ``batch_size`` envs: the three retention states (encoder, decoder
    self, decoder cross) stacked in one tensor [3, n_block, n_tile, batch, 64, 64] -- the device layout, so that an evaluation step
    converts nothing (the evaluator clones and carries it as one leaf)."""
    return torch.zeros(3, sable_network.nb, sable_network.ntile, batch_size, 64, 64, device=sable_network.dev)


def make_rec_sable_act_fn(actor_apply_fn: Callable) -> Callable:
    """``EvalActFn(params, timestep, key, actor_state) -> (action, actor_state)`` that executes the Sable network itself
    (rec_sable.py:498-513).  ``actor_apply_fn``: ``SableGuider.get_actions`` of the network that evaluates (its own object, so that
    loading the evaluated parameters does not touch the learner's); ``actor_state`` = {"hidden_state": get_init_hidden_state(...)} for
    the evaluator's own env batch.  As in the reference the action is always SAMPLED from ``key`` (get_actions has no greedy mode:
    ``arch.evaluation_greedy`` does not apply to this act function) and the hidden state is carried through an episode end unchanged
    (the evaluator reads the metrics of every env's first terminal step only).
    The hidden state is advanced in place and handed back: the caller's tensor is the carried state (get_eval_fn clones its initial
    state once per episode loop).  Parameters are loaded when a DIFFERENT dict object arrives than the last one: a caller that rewrites
    the tensors of the same dict in place and passes it again evaluates the previously loaded weights -- pass a new dict (a learner
    state snapshot is one) or ``net.named`` itself."""
    net = _owner(actor_apply_fn, SableGuider, "get_actions", "actor_apply_fn")
    return sable_eval_act_fn(net, actor_apply_fn, stateful=True)


def run_experiment(_config) -> float:
    """Runs experiment (rec_sable.py:481-620)."""
    config, rank, world, device = start_experiment(_config, "rec_sable")
    env, eval_env = environments.make(config)
    ks = host_split(prng_key(int(config.system.seed)), 3)
    key, key_e, net_key = ks[0], ks[1], ks[2]
    learn, sable_execution_fn, learner_state = learner_setup(env, (key, net_key), config, device, rank, world)

    # the evaluator runs the Sable network on its own batch of envs, with the pre-interval parameters: a second network object
    eval_net = learn.learner.guider.twin()
    eval_act_fn = make_rec_sable_act_fn(eval_net.get_actions)
    return train_and_evaluate(config, env, eval_env, learn, learner_state, eval_act_fn, key, key_e, device, rank, world,
                              init_act_state=lambda batch: {"hidden_state": get_init_hidden_state(eval_net, batch)},
                              eval_params=lambda state: state.params)


def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
    """Experiment entry point (rec_sable.py:623-636): compose configs/default/rec_sable.yaml + CLI overrides."""
    return entry_point("rec_sable", run_experiment, "Rec Sable experiment completed", overrides)


if __name__ == "__main__":
    hydra_entry_point()
