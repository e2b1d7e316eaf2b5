"""rec_qmix: recurrent QMIX, double-Q learning on a monotonic mixture of the agents' values (mava/systems/q_learning/anakin/rec_qmix.py).

The reference's public functions under their names.  The bodies drive the HIP kernels (magpo_amd.qmix_learner.QmixLearner, csrc/qmix.hip,
csrc/qlearn.hip); the experiment loop, ``learn(state)`` and the checkpointer are the ones every system uses.  The learner state is rec_iql's
``LearnerState`` with ``QMIXParams`` as its parameters and the mixer's Adam moments next to the network's in ``opt_state``, so a run resumed
from a checkpoint continues bit-identically.  Evaluation acts greedily on the online Q network; the mixer takes no part in acting.

Supported: what rec_iql supports (CoordSum and Level-Based Foraging), a global state of num_agents * raw features <= 128 inputs,
``qmix_embed_dim`` 32 or 64 with num_agents * qmix_embed_dim <= 512, ``hyper_hidden_dim`` 64 and ``QMixingNetwork`` as the mixer.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from magpo_amd import distributed as mdist
from magpo_amd.envs import obs_row_stride
from magpo_amd.optim import ClipAdam
from magpo_amd.ppo_learner import raw_features
from magpo_amd.q_net import GruQNetwork
from magpo_amd.qmix_learner import LOSS_NAMES, QmixLearner, adam_alone
from magpo_amd.qmix_net import QMixer, check_mixer_shape
from magpo_amd.systems.common import _owner, as_dict, entry_point, make_learner_fn, network_torsos, setup_learner
from magpo_amd.systems.q_learning.anakin import rec_iql
from magpo_amd.systems.q_learning.anakin.rec_iql import system_config
from magpo_amd.systems.q_learning.types import LearnerState, QMIXParams

NAME = "rec_qmix"
MIXER_TARGET = "mava.networks.base.QMixingNetwork"


def mixer_settings(config):
    """(embed_dim, hyper_hidden_dim, norm_env_states) of ``system.qmix_embed_dim`` and ``network.mixer_network``."""
    mx = config.network.get("mixer_network")
    hyper = 64 if mx is None else int(mx.get("hyper_hidden_dim", 64))
    norm = True if mx is None else bool(mx.get("norm_env_states", True))
    return int(config.system.qmix_embed_dim), hyper, norm


def check_supported(env_cfg, config) -> None:
    """What rec_qmix refuses, before any device work: what rec_iql refuses, and what the mixer kernels do not serve."""
    rec_iql.check_supported(env_cfg, config, NAME)
    mx = config.network.get("mixer_network")
    target = MIXER_TARGET if mx is None else str(mx.get("_target_", MIXER_TARGET))
    if target != MIXER_TARGET:
        raise NotImplementedError(f"rec_qmix: network.mixer_network._target_ must be {MIXER_TARGET}, got {target}")
    from magpo_amd.critic import global_state_ld
    global_state_ld(env_cfg.num_agents, raw_features(env_cfg))     # names the 128-input limit of the global state
    E, hyper, _ = mixer_settings(config)
    check_mixer_shape(env_cfg.num_agents, E, env_cfg.num_agents * raw_features(env_cfg), hyper)


def _snapshot_state(learner: QmixLearner) -> LearnerState:
    st = rec_iql._snapshot_state(learner)
    clone = lambda named: {k: v.clone() for k, v in named.items()}
    params = QMIXParams(st.params.online, st.params.target, clone(learner.mixer.named), clone(learner.mixer_target.named))
    opt = dict(st.opt_state, mixer_mu=learner.mix_opt.mu.clone(), mixer_nu=learner.mix_opt.nu.clone())
    return st._replace(params=params, opt_state=opt)


def load_learner_state(learner: QmixLearner, state: LearnerState) -> None:
    rec_iql.load_learner_state(learner, state)
    params = as_dict(state.params)
    learner.mixer.load_named(params["mixer_online"])
    learner.mixer_target.load_named(params["mixer_target"])
    learner.mix_opt.mu.copy_(state.opt_state["mixer_mu"]); learner.mix_opt.nu.copy_(state.opt_state["mixer_nu"])
    learner.mix_opt.count = int(state.opt_state["count"])


def get_learner_fn(env, apply_fns, update_fns, config):
    """Returns ``learn(learner_state) -> ExperimentOutput``: ``config.system.num_updates_per_eval`` update steps (rec_qmix.py:233-547).
    ``apply_fns`` = (GruQNetwork.apply, QMixer.apply) and ``update_fns`` = (ClipAdam.update of the network, of the mixer), bound methods of the
    objects that own the device buffers (or thin functools adaptors around them); anything else raises the ``TypeError`` of common._owner."""
    q_apply_fn, mixer_apply_fn = apply_fns
    q_update_fn, mixer_update_fn = update_fns
    q_net = _owner(q_apply_fn, GruQNetwork, "apply", "q_apply_fn")
    mixer = _owner(mixer_apply_fn, QMixer, "apply", "mixer_apply_fn")
    q_opt = _owner(q_update_fn, ClipAdam, "update", "q_update_fn")
    mix_opt = _owner(mixer_update_fn, ClipAdam, "update", "mixer_update_fn")
    if q_opt.net is not q_net or mix_opt.net is not mixer:
        raise ValueError("the update functions must belong to the optimisers of q_apply_fn's network and mixer_apply_fn's mixer")
    check_supported(env.cfg, config)
    _, world = mdist.rank_world()
    learner = QmixLearner(env.cfg, int(config.arch.num_envs), q_opt.sys, q_net.dev, num_groups=int(config.system.update_batch_size), q_net=q_net, optim=q_opt,
                          mixer=mixer, mixer_optim=mix_opt)
    return make_learner_fn(learner, config, mdist.make_grad_sync(world), _snapshot_state, load_learner_state, list(LOSS_NAMES))


def learner_setup(env, keys, config, device=None, rank: int = 0, world: int = 1):
    """Initialise learner_fn, networks, optimisers, environments, buffer and states (rec_qmix.py:59-230)."""
    key, q_key = keys
    config.system.num_agents = env.num_agents
    check_supported(env.cfg, config)
    device = device or torch.device("cuda", torch.cuda.current_device())
    cfg, sysc = env.cfg, system_config(config)
    pre, post = network_torsos(config, "q_network")
    q_key = np.asarray(q_key, np.uint32)
    # the Q network and the mixer, online and target, are all created from q_key (rec_qmix.py:115-116, :144-145)
    q_network = GruQNetwork(cfg.num_agents, cfg.num_actions, env.obs_dim, device, obs_ld=obs_row_stride(cfg.obs_dim), seed=q_key, pre_torso=pre, post_torso=post)
    E, _, norm = mixer_settings(config)
    mixer = QMixer(cfg.num_agents, E, raw_features(cfg), device, id_cols=cfg.num_agents, norm_env_states=norm, seed=q_key)
    learn = get_learner_fn(env, (q_network.apply, mixer.apply), (adam_alone(q_network, sysc).update, adam_alone(mixer, sysc).update), config)
    return learn, (q_network, mixer), setup_learner(learn, key, _snapshot_state, rank, world)


def run_experiment(_config) -> float:
    """Runs experiment (rec_qmix.py:550-680)."""
    return rec_iql.run_q_experiment(_config, NAME, True, learner_setup)


def hydra_entry_point(overrides: Optional[List[str]] = None) -> float:
    """Experiment entry point (rec_qmix.py:683-699): compose configs/default/rec_qmix.yaml + CLI overrides."""
    return entry_point(NAME, run_experiment, "QMIX experiment completed", overrides)


if __name__ == "__main__":
    hydra_entry_point()
