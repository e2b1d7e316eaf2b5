"""rec_iql: recurrent independent double-Q learning with a device replay buffer (mava/systems/q_learning/anakin/rec_iql.py).

The reference's public functions under their names.  The bodies drive the HIP kernels (magpo_amd.q_learner.QLearner, csrc/qlearn.hip);
the experiment loop, ``learn(state)`` and the checkpointer are the ones every system uses (magpo_amd/systems/common.py).  The learner state is
the reference's ``LearnerState`` (systems/q_learning/types.py): the buffer tensors and both counters are part of it, so a run resumed from a
checkpoint continues bit-identically.

Supported envs: CoordSum and Level-Based Foraging, whose step kernels write real_next_obs; the others raise NotImplementedError at set-up.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.envs import host_split, obs_row_stride, prng_key
from magpo_amd.evaluator import make_q_eval_act_fn
from magpo_amd.optim import ClipAdam
from magpo_amd.q_learner import LOSS_NAMES, QLearner, QSystemConfig, check_q_limits, epsilon
from magpo_amd.q_net import GruQNetwork
from magpo_amd.systems.common import (_owner, as_dict, check_action_space, entry_point, load_opt_state, load_rollout_state, make_learner_fn,
                                      network_torsos, setup_learner, snapshot_opt_state, snapshot_rollout_state, start_experiment,
                                      train_and_evaluate, zero_gru_state)
from magpo_amd.systems.q_learning.types import LearnerState, QNetParams
from magpo_amd.utils import make_env as environments

NAME = "rec_iql"


def system_config(config) -> QSystemConfig:
    s = config.system
    return QSystemConfig(rollout_length=int(s.rollout_length), epochs=int(s.epochs), buffer_size=int(s.buffer_size), min_buffer_size=int(s.min_buffer_size),
                         sample_batch_size=int(s.sample_batch_size), sample_sequence_length=int(s.sample_sequence_length), q_lr=float(s.q_lr),
                         max_grad_norm=float(s.max_grad_norm), hard_update=bool(s.hard_update), update_period=int(s.update_period), tau=float(s.tau),
                         gamma=float(s.gamma), eps_min=float(s.eps_min), eps_decay=float(s.eps_decay), micro_batches=int(s.get("micro_batches", 1) or 1),
                         lr_num_updates=int(s.num_updates) if s.get("num_updates") else 1000)


def check_supported(env_cfg, config, name: str = NAME) -> None:
    """What rec_iql (or the system ``name`` built on it) refuses, before any device work."""
    check_action_space(config, f"{name} supports discrete action spaces only")
    if int(config.network.hidden_state_dim) != 128:
        raise NotImplementedError("HIP kernels support hidden_state_dim=128")
    check_q_limits(env_cfg, int(config.system.sample_sequence_length), int(config.system.buffer_size), config.system.get("micro_batches", 1), name,
                   env_name=config.env.env_name)


def _snapshot_state(learner: QLearner) -> LearnerState:
    """LearnerState of the learner as an independent COPY (rec_iql.py:464-476); leaves carry a leading group axis."""
    gs = learner.groups
    st = lambda f: torch.stack([f(g) for g in gs])
    env_state, obs, term_or_trunc = snapshot_rollout_state(gs)
    buffer_state = dict(experience={k: st(lambda g: g.ring[k]) for k, v in gs[0].ring.items() if v is not None},
                        current_index=st(lambda g: g.cursor[0]), filled=st(lambda g: g.filled[0]))
    params = QNetParams({k: v.clone() for k, v in learner.q_net.named.items()}, {k: v.clone() for k, v in learner.target_net.named.items()})
    return LearnerState(obs, st(lambda g: g.term[0]), term_or_trunc, st(lambda g: g.h[0]), env_state, st(lambda g: g.t_dev[0]),
                        torch.full((len(gs),), learner.t_train, dtype=torch.int32, device=learner.dev), snapshot_opt_state(learner.q_opt), buffer_state,
                        params, np.stack([g.key for g in gs]).astype(np.uint32))


def load_learner_state(learner: QLearner, state: LearnerState) -> None:
    """Inverse of ``_snapshot_state``: write every leaf of ``state`` into the learner's (static, graph-captured) buffers."""
    params, buf = as_dict(state.params), state.buffer_state
    keys = np.asarray(state.key, np.uint32).reshape(-1, 2)     # one key per group
    load_rollout_state(learner.groups, keys, state.env_state, state.obs, state.term_or_trunc)
    learner.q_net.load_named(params["online"])
    learner.target_net.load_named(params["target"])
    load_opt_state(learner.q_opt, state.opt_state)
    for gi, g in enumerate(learner.groups):
        g.term[0].copy_(state.terminal[gi])
        g.h[0].copy_(state.hidden_state[gi])
        for k, v in g.ring.items():
            if v is not None:
                v.copy_(buf["experience"][k][gi])
        g.cursor[0].copy_(buf["current_index"][gi]); g.filled[0].copy_(buf["filled"][gi])
        g.t_dev[0].copy_(state.time_steps[gi])
        g.t = int(state.time_steps[gi])
        g.adds = g.t // learner.N            # one stored step per env step of the group
        if (g.adds % g.S, min(g.adds, g.S)) != (int(buf["current_index"][gi]), int(buf["filled"][gi])):
            raise ValueError("learner state: the buffer's counters do not belong to its time_steps")
    learner.t_train = int(state.train_steps[0])
    learner.t_train_dev.fill_(learner.t_train)


def get_learner_fn(env, q_apply_fn, q_update_fn, config):
    """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps (rec_iql.py:200-489).
    ``q_apply_fn`` must be the bound method ``GruQNetwork.apply`` and ``q_update_fn`` the bound ``ClipAdam.update`` of the objects that own the
    device buffers (or thin functools adaptors around them); anything else raises the ``TypeError`` of common._owner."""
    q_net = _owner(q_apply_fn, GruQNetwork, "apply", "q_apply_fn")
    q_opt = _owner(q_update_fn, ClipAdam, "update", "q_update_fn")
    if q_opt.net is not q_net:
        raise ValueError("q_update_fn must be the update function of the optimiser of q_apply_fn's network")
    check_supported(env.cfg, config)
    _, world = mdist.rank_world()
    learner = QLearner(env.cfg, int(config.arch.num_envs), q_opt.sys, q_net.dev, num_groups=int(config.system.update_batch_size), q_net=q_net, optim=q_opt)
    return make_learner_fn(learner, config, mdist.make_grad_sync(world), _snapshot_state, load_learner_state, list(LOSS_NAMES))


def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
    """Initialise learner_fn, network, optimiser, environments, buffer and states (rec_iql.py:59-197)."""
    key, q_key = keys
    config.system.num_agents = env.num_agents
    check_supported(env.cfg, config)
    device = device or torch.device("cuda", torch.cuda.current_device())
    cfg, sysc = env.cfg, system_config(config)
    pre, post = network_torsos(config, "q_network")
    # parameters = what flax creates from q_key, online and target alike (rec_iql.py:113-114; UNPINNED restatement, magpo_amd/params.py)
    q_network = GruQNetwork(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_row_stride(cfg.obs_dim), seed=np.asarray(q_key, np.uint32),
                            pre_torso=pre, post_torso=post)
    q_optim = ClipAdam(q_network, sysc)
    learn = get_learner_fn(env, q_network.apply, q_optim.update, config)
    return learn, q_network, setup_learner(learn, key, _snapshot_state, rank, world)


def run_q_experiment(_config, name: str, add_global_state: bool, learner_setup: Callable) -> float:
    """``run_experiment`` of rec_iql (rec_iql.py:492-618) and rec_qmix (rec_qmix.py:550-680): they differ in the name, in ``add_global_state``
    of the env factory and in the module's ``learner_setup``.  Evaluation acts greedily on the online Q network's ``twin()``."""
    config, rank, world, device = start_experiment(_config, name)
    env, eval_env = environments.make(config, add_global_state=add_global_state)
    ks = host_split(prng_key(int(config.system.seed)), 2)    # key, q_key = split(key) (:86)
    key, q_key = ks[0], ks[1]
    learn, _, learner_state = learner_setup(env, (key, q_key), config, device, rank, world)
    ks = host_split(learn.learner.setup_key, 2)              # key, eval_key = split(key) (:514)
    key, key_e = ks[0], ks[1]
    eval_net = learn.learner.q_net.twin()
    s = config.system
    # num_updates update steps of rollout_length env steps like every Anakin system here (check_total_timesteps)
    return train_and_evaluate(config, env, eval_env, learn, learner_state, make_q_eval_act_fn(eval_net, config), key, key_e, device, rank, world,
                              init_act_state=zero_gru_state(env, device), eval_params=lambda state: state.params.online,
                              misc_metrics=lambda t: {"epsilon": epsilon(t, float(s.eps_min), float(s.eps_decay))})


def run_experiment(_config) -> float:
    """Runs experiment (rec_iql.py:492-618)."""
    return run_q_experiment(_config, NAME, False, learner_setup)


def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
    """Experiment entry point (rec_iql.py:621-637): compose configs/default/rec_iql.yaml + CLI overrides."""
    return entry_point(NAME, run_experiment, "IDQN experiment completed", overrides)


if __name__ == "__main__":
    hydra_entry_point()
