"""Anakin evaluator (mava/evaluator.py:66-208) on the device kernels: sampled (or greedy) GRU-actor episodes on
non-auto-reset envs for time_limit + 1 steps, metrics taken at the first done of every env.

``pi.sample(seed=key)`` goes through TFP's categorical sampler in the reference; here it is the same
gumbel-argmax kernel as the rollout with the gumbel tensor laid out row-major over (env, agent, action)
-- PARITY UNPINNED against TFP's internal layout."""
from __future__ import annotations

import math
import time
import warnings
from typing import Callable, Dict, Optional

import numpy as np
import torch

from ._lib import lib
from .actor import GruActor
from .envs import agent_sample_keys, host_split


def get_num_eval_envs(config, absolute_metric: bool, n_devices: int = 1) -> int:
    n_parallel = config.arch.num_envs * n_devices
    episodes = config.arch.num_absolute_metric_eval_episodes if absolute_metric else config.arch.num_eval_episodes
    if episodes <= n_parallel:
        return math.ceil(episodes / n_devices)
    return config.arch.num_envs


# ---------------------------------------------------------------------- what the act functions share
def _load_params(net, loaded, params) -> None:
    """Load ``params`` into ``net`` when a DIFFERENT dict object arrives than the last one loaded (``net.named`` itself never needs loading)."""
    if params is not None and params is not net.named and params is not loaded["params"]:
        net.load_named(params)
        loaded["params"] = params


def _view_and_mask(net, timestep):
    """(agents_view [N, A, F] with its rows checked to be ``net.Fld`` floats apart, action mask as contiguous uint8 or None)."""
    view, mask = timestep.observation.agents_view, timestep.observation.action_mask
    if view.stride(2) != 1 or view.stride(1) != net.Fld or view.stride(0) != view.shape[1] * net.Fld:
        raise ValueError(f"agents_view rows must be {net.Fld} floats apart (got strides {tuple(view.stride())})")
    return view, None if mask is None else mask.to(torch.uint8).contiguous()


def _swap_hidden(actor_state):
    """(h_in, h_out) of a recurrent step: the carried ``hidden_state`` and the ``_spare`` tensor the step writes (a new one when the state
    has none of that shape yet); the step's actor state is {"hidden_state": h_out, "_spare": h_in}."""
    h_in = actor_state["hidden_state"]
    h_out = actor_state.get("_spare")
    if h_out is None or h_out.shape != h_in.shape or h_out.data_ptr() == h_in.data_ptr():
        h_out = torch.empty_like(h_in)
    return h_in, h_out


def _mode_or_sample(L, logits, mask, key, greedy: bool, N: int, A: int, K: int) -> torch.Tensor:
    """Actions [N, A] int32 from logit rows [N * A, 64]: ``pi.mode()`` of the masked categorical (heads.py:56-63: illegal logits -> finfo.min)
    or one magpo_sample_categorical draw over the whole batch from ``key``."""
    action = torch.empty(N, A, dtype=torch.int32, device=logits.device)
    if greedy:
        lg = logits[:, :K]
        if mask is not None:
            lg = torch.where(mask.view(N * A, K) != 0, lg, torch.full_like(lg, torch.finfo(torch.float32).min))
        action.copy_(lg.argmax(-1).view(N, A))
    else:
        key = np.asarray(key, dtype=np.uint32).reshape(2)
        logp = torch.empty(N * A, device=logits.device)
        L.call("magpo_sample_categorical", logits, 64, mask, 0 if mask is None else K, int(key[0]), int(key[1]), None, action, 1,
               logp, 1, None, 0, None, 0, N * A, K, torch.cuda.current_stream().cuda_stream)
    return action


def make_rec_eval_act_fn(actor_apply_fn: GruActor, config) -> Callable:
    """Makes ``EvalActFn(params, timestep, key, actor_state) -> (action, actor_state)`` for a recurrent actor (evaluator.py:50-63,
    188-208).  ``actor_apply_fn`` is the object that owns the actor's kernels (the reference passes ``actor_network.apply``);
    ``timestep`` is the env's TimeStep (observation.agents_view [N, A, F], observation.action_mask [N, A, K], ``last()`` [N]),
    ``key`` one PRNG key ([2] uint32), ``actor_state`` = {"hidden_state": [N * A, 128]}."""
    actor = actor_apply_fn
    greedy = bool(config.arch.evaluation_greedy)
    L = lib()
    loaded = {"params": None}

    def eval_act_fn(params: Dict[str, torch.Tensor], timestep, key: np.ndarray, actor_state):
        _load_params(actor, loaded, params)
        view, mask = _view_and_mask(actor, timestep)
        last_done = timestep.last().to(torch.uint8)          # repeated over the agents inside the kernel (evaluator.py:200)
        h_in, h_out = _swap_hidden(actor_state)
        logits = actor.step(view, h_in, last_done, h_out, want_logits=True)
        return _mode_or_sample(L, logits, mask, key, greedy, view.shape[0], view.shape[1], actor.K), {"hidden_state": h_out, "_spare": h_in}

    return eval_act_fn


def make_ff_eval_act_fn(actor_apply_fn, config) -> Callable:
    """Makes ``EvalActFn(params, timestep, key, actor_state) -> (action, actor_state)`` for a feed-forward actor (evaluator.py:174-185).
    ``actor_apply_fn`` is the ``FfActor`` that owns the kernels; the action is the mode of the masked categorical with
    ``arch.evaluation_greedy``, else one sample over the whole [N, A] batch from ``key``; the actor state is ``{}`` in and out."""
    actor = actor_apply_fn
    greedy = bool(config.arch.evaluation_greedy)
    L = lib()
    loaded = {"params": None}

    def eval_act_fn(params: Dict[str, torch.Tensor], timestep, key: np.ndarray, actor_state):
        _load_params(actor, loaded, params)
        view, mask = _view_and_mask(actor, timestep)
        return _mode_or_sample(L, actor.logits(view), mask, key, greedy, view.shape[0], view.shape[1], actor.K), {}

    return eval_act_fn


def make_q_eval_act_fn(q_apply_fn, config) -> Callable:
    """Makes ``EvalActFn(params, timestep, key, actor_state) -> (action, actor_state)`` for a recurrent Q network (rec_iql.py:516-529):
    ``q_apply_fn`` is the ``GruQNetwork`` that owns the kernels.  The eps-greedy distribution is built with its default eps = 0, so the sample is
    the masked greedy action whatever ``key`` is (magpo_eps_greedy_sample with a null step counter); the GRU state is carried in
    ``actor_state["hidden_state"]`` [N * A, 128]."""
    net = q_apply_fn
    L = lib()
    loaded = {"params": None}

    def eval_act_fn(params: Dict[str, torch.Tensor], timestep, key: np.ndarray, actor_state):
        _load_params(net, loaded, params)
        view, mask = _view_and_mask(net, timestep)
        N, A = view.shape[0], view.shape[1]
        h_in, h_out = _swap_hidden(actor_state)
        q = net.step(view, h_in, timestep.last().to(torch.uint8), h_out)
        action = torch.empty(N, A, dtype=torch.int32, device=view.device)
        key = np.asarray(key, dtype=np.uint32).reshape(2)
        L.call("magpo_eps_greedy_sample", q, 64, mask, int(key[0]), int(key[1]), None, None, 0.0, 1.0, action, None, N * A, net.K,
               torch.cuda.current_stream().cuda_stream)
        return action, {"hidden_state": h_out, "_spare": h_in}

    return eval_act_fn


def sable_eval_act_fn(net, actor_apply_fn: Callable, stateful: bool) -> Callable:
    """The body of the two act functions that execute a Sable network itself, rec_sable.make_rec_sable_act_fn (``stateful``) and
    ff_sable.make_ff_sable_eval_act_fn (see their docstrings): ``net`` owns ``actor_apply_fn``; the kernel's inputs and outputs are
    allocated once per batch size (the acting kernel caches its pointer tables), the action is sampled from the per-agent keys of ``key``.
    ``stateful``: ``actor_state["hidden_state"]`` (the three retention states in one tensor) is advanced IN PLACE and handed back;
    otherwise the actor state is ``{}`` in and out."""
    loaded = {"params": None}
    bufs: Dict[int, Dict[str, torch.Tensor]] = {}

    def eval_act_fn(params: Optional[Dict[str, torch.Tensor]], timestep, key: np.ndarray, actor_state):
        _load_params(net, loaded, params)
        ob = timestep.observation
        view, N, A = ob.agents_view, ob.agents_view.shape[0], net.A
        io = bufs.get(N)
        if io is None:
            dev = view.device
            io = bufs[N] = dict(obs=torch.zeros(N, A, net.Fld, device=dev), pos=torch.empty(N, dtype=torch.int32, device=dev),
                                mask=torch.empty(N, A, net.K, dtype=torch.uint8, device=dev), action=torch.empty(N, A, dtype=torch.int32, device=dev),
                                logp=torch.empty(N, A, device=dev), value=torch.empty(N, A, device=dev))
        io["obs"][..., :view.shape[2]].copy_(view)
        io["pos"].copy_(ob.step_count[:, 0] if ob.step_count.dim() == 2 else ob.step_count)
        mask = None if ob.action_mask is None else io["mask"].copy_(ob.action_mask)
        _, keys = agent_sample_keys(key, A)   # key, sample_key = split(key) per agent inside get_actions (decode.py:141)
        if not stateful:
            actor_apply_fn(io["obs"], io["pos"], None, keys, io["action"], io["logp"], io["value"], mask=mask)
            return io["action"].clone(), {}
        hs = actor_state["hidden_state"]   # advanced IN PLACE (the acting kernel updates the states where they are)
        actor_apply_fn(io["obs"], io["pos"], (hs[0], hs[1], hs[2]), keys, io["action"], io["logp"], io["value"], mask=mask, tag=f"eval{N}")
        return io["action"].clone(), {"hidden_state": hs}

    return eval_act_fn


def get_eval_fn(env, act_fn: Callable, config, absolute_metric: bool, device=None, n_devices: int = 1):
    """``EvalFn(params, key, init_act_state) -> metrics`` (evaluator.py:66-185) over the MarlEnv contract: ``env.reset(keys)``,
    then ``time_limit + 1`` times ``act_fn(params, timestep, act_key, actor_state)`` and ``env.step(env_state, action)``; the
    metrics are those of every env's FIRST terminal step.  ``n_devices`` = number of ranks (the reference's jax.device_count())."""
    episodes = config.arch.num_absolute_metric_eval_episodes if absolute_metric else config.arch.num_eval_episodes
    n_envs = get_num_eval_envs(config, absolute_metric, n_devices)
    n_parallel = n_envs * n_devices
    loops = math.ceil(episodes / n_parallel)
    if episodes % n_parallel:
        warnings.warn(f"Number of evaluation episodes ({episodes}) is not divisible by num_envs * num_devices "
                      f"({n_parallel}); running {loops * n_parallel} episodes.", stacklevel=2)
    if device is not None and getattr(env, "device", None) is None:
        env.device = device
    L = lib()

    def eval_fn(params, key: np.ndarray, init_act_state) -> Dict[str, np.ndarray]:
        rets, lens = [], []
        for _ in range(loops):   # _episode (evaluator.py:125-148)
            ks = host_split(key, 2)
            key, reset_key = ks[0], ks[1]
            dev = env._dev()
            kd = torch.from_numpy(reset_key.view(np.int32).copy()).to(dev)
            reset_keys = torch.empty(n_envs, 2, dtype=torch.int32, device=dev)
            L.call("magpo_threefry_split", kd, reset_keys, n_envs, torch.cuda.current_stream().cuda_stream)
            env_state, ts = env.reset(reset_keys)
            actor_state = {k: v.clone() for k, v in init_act_state.items()}   # {"hidden_state": ...}, or {} for a feed-forward actor
            got = torch.zeros(n_envs, dtype=torch.bool, device=dev)
            ep_ret = torch.zeros(n_envs, device=dev)
            ep_len = torch.zeros(n_envs, dtype=torch.int32, device=dev)
            step_key = key   # the scan's carried key is discarded by _episode (evaluator.py:140,150): loop 2 continues from ``key``
            for _t in range(env.time_limit + 1):   # _env_step (evaluator.py:113-123)
                ks = host_split(step_key, 2)
                step_key, act_key = ks[0], ks[1]
                action, actor_state = act_fn(params, ts, act_key, actor_state)
                env_state, ts = env.step(env_state, action)
                m = ts.extras["episode_metrics"]
                first = ts.last() & ~got
                ep_ret = torch.where(first, m["episode_return"], ep_ret)
                ep_len = torch.where(first, m["episode_length"], ep_len)
                got |= first
            rets.append(ep_ret.cpu().numpy())
            lens.append(ep_len.cpu().numpy())
        return {"episode_return": np.concatenate(rets), "episode_length": np.concatenate(lens)}

    def timed_eval_fn(params, key, init_act_state):
        t0 = time.time()
        metrics = eval_fn(params, key, init_act_state)
        torch.cuda.synchronize()
        metrics["steps_per_second"] = float(np.sum(metrics["episode_length"])) / (time.time() - t0)
        return metrics

    return timed_eval_fn
