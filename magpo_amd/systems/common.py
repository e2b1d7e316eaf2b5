"""What the ten system entry files share: reading the config tree, the refusals several of them state (``check_action_space``), the check
that get_learner_fn's callables belong to objects that own device buffers, ``learn(state)`` around a learner object, the parts of a learner
state every system has (rollout state of the env groups, optimiser state), the first and last lines of ``learner_setup`` /
``run_experiment``, the experiment loop and ``hydra_entry_point``'s body.  Each system file keeps what is its own:

    gpo/anakin/rec_magpo.py                 guider and GRU actor, both optimisers, Sable and policy hidden states, GPOLearnerState
    sable/anakin/rec_sable.py, ff_sable.py  the Sable network and its memory settings, (rec) the retention states, the act function that
                                            executes the network itself (body: evaluator.sable_eval_act_fn)
    ppo/anakin/rec_ppo.py, ff_ppo.py        behind rec_ippo / rec_mappo and ff_ippo / ff_mappo; what the pairs share is ppo/anakin/ppo_common.py:
                                            rec adds hidden states and recurrent_chunk_size, ff its torso rule and action-space check
    q_learning/anakin/rec_iql.py            Q network, replay ring and counters in the state, the run_experiment body of both Q systems
    q_learning/anakin/rec_qmix.py           the mixer: its settings, parameters and Adam moments next to rec_iql's
"""
from __future__ import annotations

import copy
import os
import sys
import time
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.actor import GruActor
from magpo_amd.anakin import SystemConfig
from magpo_amd.config import compose
from magpo_amd.envs import host_split
from magpo_amd.evaluator import get_eval_fn, get_num_eval_envs, make_ff_eval_act_fn, make_rec_eval_act_fn
from magpo_amd.torso import DEFAULT_TORSO, torso_from_config
from magpo_amd.types import ExperimentOutput
from magpo_amd.utils.checkpointing import Checkpointer, latest_valid_checkpoint, load_checkpoint, restore_learner_state
from magpo_amd.utils.config import check_total_timesteps
from magpo_amd.utils.logger import LogEvent, MavaLogger


def _system_config(config, clip_gpo=None, alpha=None) -> SystemConfig:
    """``clip_gpo`` / ``alpha``: given by a system whose config tree has no such keys (rec_sable, which never reads them); rec_magpo's are required."""
    s = config.system
    return SystemConfig(rollout_length=int(s.rollout_length), ppo_epochs=int(s.ppo_epochs), num_minibatches=int(s.num_minibatches),
                        gamma=float(s.gamma), gae_lambda=float(s.gae_lambda), clip_eps=float(s.clip_eps), ent_coef=float(s.ent_coef),
                        vf_coef=float(s.vf_coef), max_grad_norm=float(s.max_grad_norm), clip_gpo=float(s.clip_gpo if clip_gpo is None else clip_gpo),
                        alpha=float(s.alpha if alpha is None else alpha), actor_lr=float(s.actor_lr), decay_learning_rates=bool(s.get("decay_learning_rates", False)),
                        lr_num_updates=int(s.num_updates) if s.get("num_updates") else 1000, micro_batches=int(s.get("micro_batches", 1) or 1))


def network_torsos(config, which: str):
    """(pre, post) TorsoSpecs of ``network.actor_network`` / ``network.critic_network`` (rec_magpo.py:570-571, rec_mappo.py:412-417
    instantiate them as MLPTorso); what the HIP kernels do not cover raises NotImplementedError (magpo_amd/torso.py)."""
    node = config.network.get(which)
    if node is None:
        return DEFAULT_TORSO, DEFAULT_TORSO
    return (torso_from_config(node.pre_torso) if "pre_torso" in node else DEFAULT_TORSO,
            torso_from_config(node.post_torso) if "post_torso" in node else DEFAULT_TORSO)


def check_action_space(config, label: str, tail: str = "") -> None:
    """Discrete actions only (the masked categorical head, the eps-greedy selector); the reference's continuous heads are not built.
    ``label`` / ``tail``: the calling system's words in front of and behind the refused value."""
    kw = config.env.get("kwargs")
    action_type = "Discrete" if kw is None else str(kw.get("action_type", "Discrete"))
    if action_type.lower() != "discrete":
        raise NotImplementedError(f"{label}, got env.kwargs.action_type={action_type}{tail}")


def _owner(fn, cls, method: str, what: str):
    """The object whose device buffers ``fn`` acts on: ``fn`` must be the bound method ``cls.<method>`` or a thin adaptor around it
    (``functools.partial(...).func`` / ``functools.wraps(...).__wrapped__`` chains are followed)."""
    f, seen = fn, 0
    while not hasattr(f, "__self__") and seen < 8:
        f = getattr(f, "__wrapped__", None) or getattr(f, "func", None)
        seen += 1
        if f is None:
            break
    obj = getattr(f, "__self__", None)
    names = {method} | ({"act_fused"} if method == "get_actions" else {"train_fwd", "seq_fwd"} if method == "apply" else
                        {"act_team_fused"} if method == "act" else set())   # (act_team_fused: the one-launch form of a memoryless network's act)
    if not isinstance(obj, cls) or getattr(f, "__name__", None) not in names:
        raise TypeError(
            f"get_learner_fn: {what} must be the bound method {cls.__name__}.{method} of a network / optimiser object (or a functools.wraps / "
            f"functools.partial adaptor around it), got {fn!r}.  Unlike the reference's pure functions of parameter pytrees, the HIP path keeps "
            "parameters, activations and optimiser moments in device buffers owned by these objects and pairs each forward with a "
            "hand-written backward, so a free function cannot stand in for them.")
    return obj


# ---------------------------------------------------------------------- the parts of a learner state every system has
def snapshot_rollout_state(groups):
    """(env_state, timestep, dones) of the env groups as independent copies with a leading group axis (the reference's update-batch
    axis): what the next rollout reads of the env state and of the last TimeStep."""
    env_state = {f: torch.stack([getattr(g.env, f) for g in groups]) for f in groups[0].env.state_fields}
    timestep = dict(agents_view=torch.stack([g.traj["obs"][0] for g in groups]), step_count=torch.stack([g.traj["step_count"][0] for g in groups]))
    if groups[0].traj["mask"] is not None:
        timestep["action_mask"] = torch.stack([g.traj["mask"][0] for g in groups])
    return env_state, timestep, torch.stack([g.traj["done"][0] for g in groups])


def load_rollout_state(groups, key, env_state, timestep, dones) -> None:
    """Inverse of ``snapshot_rollout_state``, into the groups' (static, graph-captured) buffers.  ``key``: one key [2], of which every group
    takes a copy, or a table [groups, 2] with every group's own (the Q learner's groups carry different keys)."""
    if dones.shape[0] != len(groups):
        raise ValueError(f"learner state holds {dones.shape[0]} env groups, the learner {len(groups)}")
    keys = np.asarray(key, dtype=np.uint32)
    for gi, grp in enumerate(groups):
        for f in grp.env.state_fields:
            getattr(grp.env, f).copy_(env_state[f][gi])
        grp.traj["obs"][0].copy_(timestep["agents_view"][gi])
        if grp.traj["mask"] is not None:
            grp.traj["mask"][0].copy_(timestep["action_mask"][gi])
        grp.traj["step_count"][0].copy_(timestep["step_count"][gi])
        grp.traj["done"][0].copy_(dones[gi])
        grp.key = (keys if keys.ndim == 1 else keys[gi]).copy()


def snapshot_opt_state(opt) -> Dict[str, Any]:
    """optax's adam state of a ClipAdam as a copy: count, mu, nu."""
    return dict(count=opt.count, mu=opt.mu.clone(), nu=opt.nu.clone())


def load_opt_state(opt, state) -> None:
    opt.mu.copy_(state["mu"]); opt.nu.copy_(state["nu"]); opt.count = int(state["count"])


def as_dict(x):
    """A state node as a dict: it is a NamedTuple when the learner made it and a plain dict when a caller rebuilt it."""
    return x if isinstance(x, dict) else x._asdict()


# ---------------------------------------------------------------------- learn(state)
def make_learner_fn(learner, config, grad_sync, snapshot, load, loss_names):
    """``learn(learner_state) -> ExperimentOutput`` around a learner object: ``config.system.num_updates_per_eval`` update steps, the
    per-step episode metrics and the loss table under ``loss_names`` (the first columns of the learner's loss scalars).  ``snapshot`` /
    ``load`` turn the learner's device buffers into the system's LearnerState and back.  """
    def learner_fn(learner_state) -> ExperimentOutput:
        if learner_state is not getattr(learner, "_live_state", None):
            load(learner, learner_state)
        n_up = int(config.system.num_updates_per_eval)
        # linear_scedule reads config.system.num_updates when the learner is traced, i.e. at the first learn() call -- AFTER
        # check_total_timesteps has rewritten it on the same config object (mava/utils/training.py:37-43; rec_magpo.py:581 vs :717)
        learner.sys.lr_num_updates = int(config.system.num_updates)
        ep: Dict[str, List[np.ndarray]] = {"episode_return": [], "episode_length": [], "is_terminal_step": []}
        train = []
        for _ in range(n_up):
            losses = learner.update_step(grad_sync)
            train.append(losses)
            for k in ep:
                ep[k].append(torch.stack([g.metrics[k] for g in learner.groups]).cpu().numpy())
        tl = torch.stack(train).cpu().numpy()  # (updates, P, M, n_loss)
        train_metrics = {n: tl[..., i] for i, n in enumerate(loss_names)}
        episode_metrics = {k: np.stack(v) for k, v in ep.items()}
        episode_metrics["is_terminal_step"] = episode_metrics["is_terminal_step"].astype(bool)
        learner._live_state = snapshot(learner)
        return ExperimentOutput(learner._live_state, episode_metrics, train_metrics)

    learner_fn.learner = learner
    return learner_fn


def setup_learner(learn, key, snapshot, rank: int, world: int):
    """The end of every learner_setup: reset the envs of this rank's ``update_batch_size`` groups out of ``world`` x that many and take
    the first learner state.  Returns it."""
    learner = learn.learner
    U = len(learner.groups)
    learner.setup(key, n_groups=world * U, group=rank * U)
    learner._live_state = snapshot(learner)
    return learner._live_state


# ---------------------------------------------------------------------- run_experiment
def start_experiment(_config, system_name: str):
    """The beginning of every run_experiment: name the system for the logger, copy the config, join the job, pick the GPU.
    Returns (config, rank, world, device)."""
    _config.logger.system_name = system_name
    config = copy.deepcopy(_config)
    rank, world, local = mdist.init_from_env()
    torch.cuda.set_device(local)
    return config, rank, world, torch.device("cuda", local)


def entry_point(name: str, run_experiment, done_message: str, overrides: Optional[List[str]] = None) -> float:
    """The body of every ``hydra_entry_point``: compose configs/default/<name>.yaml + CLI overrides, run, print the system's last line."""
    cfg = compose(name, sys.argv[1:] if overrides is None else overrides)
    perf = run_experiment(cfg)
    print(done_message)
    return perf


def zero_gru_state(env, device):
    """``init_act_state`` of an evaluator whose network carries a GRU state: {"hidden_state": zeros [batch * A, 128]}."""
    return lambda batch: {"hidden_state": torch.zeros(batch * env.num_agents, 128, device=device)}


def train_and_evaluate_actor(config, env, eval_env, learn, actor_network, learner_state, key, key_e, device, rank, world) -> float:
    """``train_and_evaluate`` for a system whose evaluated policy is a GruActor (rec_magpo, rec_ippo, rec_mappo) or an FfActor (ff_ippo,
    ff_mappo): the evaluator runs the actor's ``twin()`` on its own batch of envs, with the pre-interval ``params.actor_params``; a
    feed-forward actor's state is ``{}``."""
    eval_actor = actor_network.twin()
    if isinstance(eval_actor, GruActor):
        act_fn, init_act_state = make_rec_eval_act_fn(eval_actor, config), zero_gru_state(env, device)
    else:
        act_fn, init_act_state = make_ff_eval_act_fn(eval_actor, config), lambda batch: {}
    return train_and_evaluate(config, env, eval_env, learn, learner_state, act_fn, key, key_e, device, rank, world, init_act_state=init_act_state,
                              eval_params=lambda state: state.params.actor_params)


train_and_evaluate_gru_actor = train_and_evaluate_ff_actor = train_and_evaluate_actor   # (the names from before the two were one)


def train_and_evaluate(config, env, eval_env, learn, learner_state, eval_act_fn, key, key_e, device, rank, world, *, init_act_state, eval_params,
                       misc_metrics=None) -> float:
    """The experiment loop both systems run after their set-up (rec_magpo.py:702-815, rec_sable.py:518-620): evaluator, timestep
    bookkeeping, logger, checkpoint save / resume, ``num_evaluation`` x (learn, evaluate the pre-interval parameters), absolute metric.
    ``init_act_state(batch)``: the evaluator's initial actor state for ``batch`` envs; ``eval_params(learner_state)``: the parameter
    dict the act function evaluates; ``misc_metrics(t)``: what a system logs under MISC next to the timestep (rec_iql's epsilon)."""
    n_devices = world
    evaluator = get_eval_fn(eval_env, eval_act_fn, config, absolute_metric=False, device=device, n_devices=n_devices)

    config = check_total_timesteps(config, n_devices)
    assert config.system.num_updates > config.arch.num_evaluation, \
        "Number of updates per evaluation must be less than total number of updates."
    config.system.num_updates_per_eval = config.system.num_updates // config.arch.num_evaluation
    steps_per_rollout = (n_devices * config.system.num_updates_per_eval * config.system.rollout_length
                         * config.system.update_batch_size * config.arch.num_envs)
    logger = MavaLogger(config) if rank == 0 else None
    # every rank saves: rank 0 the full state, the others their own rollout state (their envs, keys and hidden states differ)
    save_checkpoint = bool(config.logger.checkpointing.save_model)
    if save_checkpoint:
        sa = config.logger.checkpointing.save_args.to_container()
        if world > 1 and not sa.get("checkpoint_uid"):   # one directory for all ranks
            sa["checkpoint_uid"] = mdist.broadcast_object(time.strftime("%Y%m%d%H%M%S"))
        checkpointer = Checkpointer(metadata=config.to_container(), model_name=config.logger.system_name,
                                    base_path=config.logger.base_exp_path, rank=rank, world=world, **sa)
    if bool(config.logger.checkpointing.load_model):
        # Resume from the latest loadable checkpoint of load_args.checkpoint_uid (the reference saves the full learner state,
        # checkpointing.py:108-145, but rec_magpo.py never reads it back: this closes the loop for long sweeps).  Rank-aware:
        # parameters / optimiser state from rank 0's file, env state / keys / hidden states from the rank's own file.
        la = config.logger.checkpointing.load_args
        cdir = os.path.join(config.logger.base_exp_path, la.rel_dir, config.logger.system_name, str(la.checkpoint_uid))
        latest = latest_valid_checkpoint(cdir, rank, world)
        learner_state, _ = restore_learner_state(latest, device, rank, world)
        resume = load_checkpoint(latest).get("extras") or {}
    else:
        resume = {}
    eval_batch = get_num_eval_envs(config, absolute_metric=False, n_devices=n_devices)
    eval_hs = init_act_state(eval_batch)

    max_episode_return = -np.inf
    best_params = None
    eval_metrics: Dict[str, Any] = {}
    start_eval = 0
    if resume:   # a checkpoint written by this loop: continue the evaluation counter, the evaluator's key chain and the best-params record
        start_eval = int(resume["eval_step"]) + 1
        key_e = np.asarray(resume["key_e"], np.uint32)
        max_episode_return = float(resume["max_episode_return"])
        best_params = None if resume["best_params"] is None else {k: v.to(device) for k, v in resume["best_params"].items()}
    for eval_step in range(start_eval, int(config.arch.num_evaluation)):
        start = time.time()
        learner_output = learn(learner_state)
        torch.cuda.synchronize()
        elapsed = time.time() - start
        t = int(steps_per_rollout * (eval_step + 1))
        em = learner_output.episode_metrics
        term = em["is_terminal_step"]
        ep_completed = bool(term.any())
        if logger:
            logger.log({"timestep": t, **(misc_metrics(t) if misc_metrics is not None else {})}, t, eval_step, LogEvent.MISC)
            if ep_completed:
                logger.log({"episode_return": em["episode_return"][term], "episode_length": em["episode_length"][term],
                            "steps_per_second": steps_per_rollout / elapsed}, t, eval_step, LogEvent.ACT)
            logger.log(learner_output.train_metrics, t, eval_step, LogEvent.TRAIN)
        # evaluate the PRE-interval actor parameters, as the reference does (rec_magpo.py:770)
        trained_params = eval_params(learner_state)
        ks = host_split(key_e, n_devices + 1)
        key_e, eval_key = ks[0], ks[1 + rank]
        eval_metrics = evaluator(trained_params, eval_key, eval_hs)
        if logger:
            logger.log(eval_metrics, t, eval_step, LogEvent.EVAL)
        episode_return = float(np.mean(eval_metrics["episode_return"]))
        if config.arch.absolute_metric and max_episode_return <= episode_return:
            best_params = {k: v.clone() for k, v in trained_params.items()}
            max_episode_return = episode_return
        if save_checkpoint:  # rec_magpo.py:779-785 (+ what run_experiment itself needs to continue: its loop state)
            mdist.barrier()
            checkpointer.save(timestep=t, unreplicated_learner_state=learner_output.learner_state, episode_return=episode_return,
                              extras=dict(eval_step=eval_step, key_e=key_e.copy(), max_episode_return=max_episode_return,
                                          best_params=None if best_params is None else {k: v.cpu() for k, v in best_params.items()}))
            mdist.barrier()      # every rank's file of this timestep is on disk: only now may older checkpoints go
            checkpointer.prune()
        learner_state = learner_output.learner_state

    eval_performance = float(np.mean(eval_metrics[config.env.eval_metric])) if eval_metrics else float("nan")
    if config.arch.absolute_metric:
        eb = get_num_eval_envs(config, absolute_metric=True, n_devices=n_devices)
        abs_hs = init_act_state(eb)
        abs_eval = get_eval_fn(eval_env, eval_act_fn, config, absolute_metric=True, device=device, n_devices=n_devices)
        abs_key = host_split(key, n_devices)[rank]
        m = abs_eval(best_params, abs_key, abs_hs)
        if logger:
            logger.log(m, int(steps_per_rollout * config.arch.num_evaluation), int(config.arch.num_evaluation) - 1, LogEvent.ABSOLUTE)
    if logger:
        logger.stop()
    return eval_performance
