"""MAGPO system entry point on MI355X -- drop-in for mava/systems/gpo/anakin/rec_magpo.py.

Same public names and call contract as the reference system file:
    hydra_entry_point / main(overrides)      rec_magpo.py:818-831
    run_experiment(config) -> float          rec_magpo.py:688-815
    learner_setup(env, keys, config) -> (learn, actor_network, init_learner_state)   rec_magpo.py:533-685
    get_learner_fn(env, apply_fns, update_fn, config) -> LearnerFn                   rec_magpo.py:91-530
The bodies drive the HIP kernels (magpo_amd.learner.MagpoLearner); there is no JAX, no XLA, no Triton.

    python -m magpo_amd.systems.gpo.anakin.rec_magpo env=coordsum env/scenario=8x15-100 arch.num_envs=64

Multi-GPU: launch one process per GPU with torch.distributed.run; ``n_devices`` = world size, each rank owns
``update_batch_size`` groups of ``arch.num_envs`` envs, gradients are averaged with one RCCL all-reduce.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.actor import GruActor
from magpo_amd.learner import MagpoLearner, host_split, obs_row_stride, prng_key
from magpo_amd.optim import ClipAdam
from magpo_amd.sable import SableGuider, load_sable_hstates, sable_hstates_logical
from magpo_amd.systems.common import (_owner, _system_config, as_dict, entry_point, load_opt_state, load_rollout_state, make_learner_fn,
                                      network_torsos, setup_learner, snapshot_opt_state, snapshot_rollout_state, start_experiment,
                                      train_and_evaluate_actor)
from magpo_amd.tuning import Tuning
from magpo_amd.types import GPOLearnerState, HiddenStates, OptStates, Params, SableHiddenStates
from magpo_amd.utils import make_env as environments

LearnerState = GPOLearnerState


def _snapshot_state(learner: MagpoLearner) -> GPOLearnerState:
    """LearnerState of the learner as an independent COPY (rec_magpo.py:488-497): the state a caller holds stays readable
    and re-usable after later learn() calls (the harness evaluates the pre-interval parameters, rec_magpo.py:770, SURVEY
    B12; a checkpoint of it can be resumed).  Leaves carry a leading group axis (the reference's update-batch axis)."""
    gs = learner.groups
    params = Params({k: v.clone() for k, v in learner.guider.named.items()}, {k: v.clone() for k, v in learner.actor.named.items()})
    opt = OptStates(snapshot_opt_state(learner.g_opt), snapshot_opt_state(learner.a_opt))
    # The state carries the reference's [embed_dim / n_head, embed_dim / n_head] head states (sable_hstates_logical)
    gd = learner.guider
    hs = HiddenStates(SableHiddenStates(*[torch.stack([sable_hstates_logical(gd, g.sable_hs[i]) for g in gs]) for i in range(3)]),
                      torch.stack([g.policy_h[g.cur] for g in gs]))
    return GPOLearnerState(params, opt, gs[0].key.copy(), *snapshot_rollout_state(gs), hs)


def load_learner_state(learner: MagpoLearner, state: GPOLearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    params, opt, hst = as_dict(state.params), as_dict(state.opt_states), as_dict(state.hstates)
    learner.guider.load_named(params["guider_params"])
    learner.actor.load_named(params["actor_params"])
    load_opt_state(learner.g_opt, opt["guider_opt_state"])
    load_opt_state(learner.a_opt, opt["actor_opt_state"])
    sable = as_dict(hst["sable_hidden_state"])
    sable = (sable["encoder"], sable["decoder_self_retn"], sable["decoder_cross_retn"])
    load_rollout_state(learner.groups, state.key, state.env_state, state.timestep, state.dones)
    for gi, grp in enumerate(learner.groups):
        for i in range(3):
            load_sable_hstates(learner.guider, grp.sable_hs[i], sable[i][gi])
        grp.policy_h[grp.cur].copy_(hst["policy_hidden_state"][gi])


def get_learner_fn(env, apply_fns, update_fn, config):
    """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps
    (rec_magpo.py:91-530).  Same contract as the reference:

        apply_fns = (sable_action_select_fn, sable_apply_fn, actor_apply_fn)     rec_magpo.py:99   (execution / training / training)
        update_fn = (sable_update_fn, actor_update_fn)                           rec_magpo.py:100  (the two optimisers' update functions)

    In the reference these are pure functions of parameter pytrees.  Here the parameters, activations and optimiser moments live in device
    buffers OWNED by objects (``SableGuider``, ``GruActor``, ``ClipAdam``), and a hand-written backward pairs every training forward, so
    the five callables must be methods of such objects: ``SableGuider.get_actions`` / ``SableGuider.apply`` / ``GruActor.apply`` and
    ``ClipAdam.update``, either the bound methods themselves or thin adaptors around them that expose the method as ``__wrapped__``
    (``functools.wraps``) or ``func`` (``functools.partial``).  The loop CALLS exactly the callables it is given (rollout ->
    ``sable_action_select_fn``, minibatch forward -> ``sable_apply_fn`` / ``actor_apply_fn``, optimiser step -> the update functions) and
    reaches the owners' buffers / backward passes through them; anything else raises a ``TypeError`` that says so (``_owner``).
    ``env``: the MarlEnv whose batched kernels the rollout steps.

    State in, state out: the learner's device buffers are a cache of the last state it produced.  When ``learner_state``
    is that state (the normal host loop, rec_magpo.py:754,792) nothing is copied; any other state (an older one, a restored
    checkpoint) is loaded into the buffers first, so ``learn`` is a function of its argument."""
    sable_action_select_fn, sable_apply_fn, actor_apply_fn = apply_fns
    sable_update_fn, actor_update_fn = update_fn
    guider = _owner(sable_apply_fn, SableGuider, "apply", "apply_fns[1] (sable_apply_fn)")
    actor = _owner(actor_apply_fn, GruActor, "apply", "apply_fns[2] (actor_apply_fn)")
    if _owner(sable_action_select_fn, SableGuider, "get_actions", "apply_fns[0] (sable_action_select_fn)") is not guider:
        raise ValueError("the execution and the training function must belong to one Sable network")
    g_opt = _owner(sable_update_fn, ClipAdam, "update", "update_fn[0] (sable_update_fn)")
    a_opt = _owner(actor_update_fn, ClipAdam, "update", "update_fn[1] (actor_update_fn)")
    rank, world = mdist.rank_world()
    U = int(config.system.update_batch_size)
    learner = MagpoLearner(env.cfg, int(config.arch.num_envs), g_opt.sys, guider.dev, num_groups=U, guider=guider, actor=actor, optims=(g_opt, a_opt),
                           apply_fns=tuple(apply_fns), update_fns=tuple(update_fn))
    grad_sync = mdist.make_grad_sync(world)   # the pmean over ("batch", "device") of rec_magpo.py:395-409: one all-reduce of the flat buffer

    return make_learner_fn(learner, config, grad_sync, _snapshot_state, load_learner_state,
                           ["total_loss", "value_loss", "actor_loss", "guider_loss", "kl_loss", "entropy"])


def actor_torsos(config):
    """(pre, post) TorsoSpecs of ``network.actor_network`` (rec_magpo.py:570-571 instantiates them as MLPTorso); what the HIP
    kernels do not cover raises NotImplementedError (magpo_amd/torso.py)."""
    return network_torsos(config, "actor_network")


def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
    """Initialise learner_fn, networks, optimiser, environments and states (rec_magpo.py:533-685)."""
    key, actor_net_key, net_key = keys
    config.system.num_agents = env.num_agents
    nc, mc = config.network.net_config, config.network.memory_config
    # memory_config.timestep_chunk_size only changes HOW the reference evaluates the chunkwise retention (smaller chunks with a
    # carried state, rec_magpo.py:552-557); the function is the same for every chunk size (recurrent == chunkwise, tested in
    # tests/test_oracle_networks.py).  The HIP kernel always walks 64-token tiles with the state on chip, so the key is honoured
    # as a pure memory/speed knob with no effect here.
    if mc.timestep_chunk_size:
        mc.chunk_size = int(mc.timestep_chunk_size) * env.num_agents
    else:
        mc.chunk_size = config.system.rollout_length * env.num_agents
    if mc.type != "rec_sable":
        raise NotImplementedError("memory_config.type must be rec_sable")
    if int(nc.embed_dim) not in (16, 32, 64, 128) or int(nc.n_head) not in (1, 2, 4) or int(config.network.hidden_state_dim) != 128:
        raise NotImplementedError("HIP kernels support embed_dim in {16,32,64,128}, n_head in {1,2,4}, hidden_state_dim=128 (any n_block)")
    pre_torso, post_torso = actor_torsos(config)
    device = device or torch.device("cuda", torch.cuda.current_device())
    # networks (rec_magpo.py:559-579), optimisers (:581-589) -- objects that own their kernels' device buffers
    cfg, sysc = env.cfg, _system_config(config)
    # parameters = what flax creates from net_key / actor_net_key (rec_magpo.py:598-604,623; magpo_amd/params.py, UNPINNED restatement)
    obs_ld = obs_row_stride(cfg.obs_dim)   # floats between the rows the env kernels write; env.obs_dim = the features the networks read (add_agent_id)
    g_seed, a_seed = np.asarray(net_key, np.uint32), np.asarray(actor_net_key, np.uint32)
    tuning = Tuning.from_env()   # ONE object shared by both networks (tuning.py)
    if tuning.legacy_init:   # A/B only: the torch-generator initialisation of rounds 1-3 (same distributions, other draws)
        g_seed = int(net_key[1]) & 0x7FFFFFFF
        a_seed = g_seed + 1
    sable_network = SableGuider(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_ld, embed_dim=int(nc.embed_dim), n_head=int(nc.n_head),
                                n_block=int(nc.n_block), decay_scaling_factor=float(mc.decay_scaling_factor),
                                use_pe=bool(mc.timestep_positional_encoding), max_pos=cfg.time_limit + 1, seed=g_seed, tuning=tuning)
    actor_network = GruActor(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_ld, seed=a_seed, tuning=tuning,
                             pre_torso=pre_torso, post_torso=post_torso)
    guider_optim, actor_optim = ClipAdam(sable_network, sysc), ClipAdam(actor_network, sysc)
    # Pack apply and update functions (rec_magpo.py:624-632)
    apply_fns = (sable_network.get_actions, sable_network.apply, actor_network.apply)
    update_fns = (guider_optim.update, actor_optim.update)
    learn = get_learner_fn(env, apply_fns, update_fns, config)
    return learn, actor_network, setup_learner(learn, key, _snapshot_state, rank, world)


def run_experiment(_config) -> float:
    """Runs experiment (rec_magpo.py:688-815)."""
    config, rank, world, device = start_experiment(_config, "rec_magpo")
    env, eval_env = environments.make(config)
    ks = host_split(prng_key(int(config.system.seed)), 4)
    key, key_e, actor_net_key, net_key = ks[0], ks[1], ks[2], ks[3]
    learn, actor_network, learner_state = learner_setup(env, (key, actor_net_key, net_key), config, device, rank, world)
    return train_and_evaluate_actor(config, env, eval_env, learn, actor_network, learner_state, key, key_e, device, rank, world)


def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
    """Experiment entry point (rec_magpo.py:818-831): compose configs/default/rec_magpo.yaml + CLI overrides."""
    return entry_point("rec_magpo", run_experiment, "MAGPO experiment completed", overrides)


if __name__ == "__main__":
    hydra_entry_point()
