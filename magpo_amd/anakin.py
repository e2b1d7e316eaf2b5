"""What every Anakin learner here shares, whichever networks it trains: env groups, the rollout's eager / warm-up / capture / replay
state machine, the minibatch gather and the group dispatch of one optimisation step.

``MagpoLearner`` (learner.py; ``SableLearner`` derives from it) and ``PpoLearner`` (ppo_learner.py) derive from ``AnakinLearner`` and
supply what depends on their networks:

  _reset_states(g)          zero the hidden states of one group at set-up
  _rollout_keys(g)          advance g.key over one rollout and fill the host key table g.keys_host
  _rollout_body(g, keys)    T acting steps + bootstrap value + GAE on the current stream; ``keys`` is g.keys_host when the body runs
                            eagerly (keys passed by value) and g.keys_dev when it is captured (the replayed graph reads the table)
  _mb_buffers(R, nseq)      the per-minibatch buffers next to the gathered rows (loss gradients, start-state row indices, ...)
  minibatch_grads / apply_grads / update   the minibatch, the optimiser steps and the epoch loop (they call ``_optimise``)
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from ._lib import lib
from .envs import host_split, make_env_batch, net_obs, obs_row_stride, prng_key


@dataclass
class SystemConfig:
    rollout_length: int = 128
    ppo_epochs: int = 4
    num_minibatches: int = 2
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_eps: float = 0.2
    ent_coef: float = 0.01
    vf_coef: float = 0.5
    max_grad_norm: float = 0.5
    clip_gpo: float = 1.5
    alpha: float = 1.0
    actor_lr: float = 2.5e-4
    # make_learning_rate (mava/utils/training.py:20-64): linear decay lr * (1 - (count // (ppo_epochs * num_minibatches)) / num_updates)
    # with the optimiser step count BEFORE the step; lr_num_updates is config.system.num_updates as the schedule reads it when the learner
    # is TRACED (first learn() call), i.e. the value check_total_timesteps derived: the system file refreshes it on every learn() call
    decay_learning_rates: bool = False
    lr_num_updates: int = 1000
    # not a reference key: every minibatch is trained in this many equal slabs of sequences whose gradients are accumulated before the
    # ONE optimiser step (same gradient up to fp32 summation order; advantage statistics stay those of the whole minibatch).
    # Activations in HBM scale with the slab, so large teams run at the reference's num_minibatches within the memory of one GPU.
    micro_batches: int = 1


def split_setup_keys(L, dev, st, key: np.ndarray, total: int):
    """learner_setup's key layout (rec_magpo.py:642-660 = rec_mappo.py:495-513): split(key, total) on the device; row 0 is split once more on
    the host into (set-up key, the ONE step key every group shares).  Returns (device keys [total, 2] i32, set-up key, step key)."""
    kd = torch.from_numpy(np.ascontiguousarray(key, np.uint32).view(np.int32)).to(dev)
    allk = torch.empty(total, 2, dtype=torch.int32, device=dev)
    L.call("magpo_threefry_split", kd, allk, total, st)
    ks = host_split(allk[0].cpu().numpy().view(np.uint32), 2)
    return allk, ks[0], ks[1]


def setup_env_groups(L, dev, st, groups, key: np.ndarray, N: int, n_groups: int, group: int) -> np.ndarray:
    """What every system's set-up does with its env groups (objects with ``env``, ``traj`` and ``key``): reset keys are rows 1.. of
    split(key, n_groups * N + 1) laid out row-major over (group, env), ``group`` = global index of the first local group; slot 0 of the
    trajectory takes the reset observation and done = 0; ONE step key is shared by every group.  Returns the set-up key."""
    if group < 0 or group + len(groups) > n_groups:   # (a short key table would send the env-reset kernel out of bounds)
        raise ValueError(f"setup: this learner holds {len(groups)} env group(s) starting at group {group}, but the job has n_groups={n_groups}")
    allk, setup_key, step_key = split_setup_keys(L, dev, st, key, n_groups * N + 1)
    for gi, g in enumerate(groups):
        env_keys = allk[1 + (group + gi) * N: 1 + (group + gi + 1) * N].contiguous()
        g.env.reset(env_keys, g.traj["obs"][0], g.traj["step_count"][0], None if g.traj["mask"] is None else g.traj["mask"][0])
        g.traj["done"][0].zero_()
        g.key = step_key.copy()
    return setup_key


def jax_permutation(L, dev, st, key: np.ndarray, n: int) -> torch.Tensor:
    """jax.random.permutation(key, n) on the device: rounds of a stable sort by 32 random bits."""
    rounds = int(math.ceil(3 * math.log(max(1, n)) / math.log(2 ** 32 - 1)))
    x = torch.arange(n, dtype=torch.int32, device=dev)
    bits = torch.empty(n, dtype=torch.int32, device=dev)
    for _ in range(rounds):
        ks = host_split(key, 2)
        key, sub = ks[0], ks[1]
        kd = torch.from_numpy(sub.view(np.int32).copy()).to(dev)
        L.call("magpo_threefry_random_bits", kd, bits, n, st)
        order = torch.sort(bits.to(torch.int64) & 0xFFFFFFFF, stable=True).indices
        x = x[order]
    return x.contiguous()


class AdvStats:
    """The [mean, 1 / (std + eps)] pair a loss kernel normalises the advantages of a minibatch with (rec_magpo.py:283,356; rec_sable.py:199;
    rec_mappo.py:193), per group when several groups train as one batch of sequences.  Owns its small device buffers."""

    def __init__(self, L, dev):
        self.L, self.dev = L, dev
        self.one = torch.zeros(2, dtype=torch.float32, device=dev)
        self.per_group = None
        self.ident = None

    def __call__(self, m, U: int, adv_stats: Optional[torch.Tensor], ws64: torch.Tensor, st) -> torch.Tensor:
        R = m["R"]
        R1 = R // U
        if U == 1:
            if adv_stats is None:
                self.L.call("magpo_adv_moments", m["adv"], R, ws64, self.one, st)
            return self.one if adv_stats is None else adv_stats[0]
        # per-group statistics, applied in place with the loss kernel's own expression (adv - mean) * rstd; identity stats after
        if self.per_group is None or self.per_group.shape[0] != U:
            self.per_group = torch.zeros(U, 2, device=self.dev)
            self.ident = torch.tensor([0.0, 1.0], device=self.dev)
        su = self.per_group if adv_stats is None else adv_stats
        if adv_stats is None:
            for u in range(U):
                self.L.call("magpo_adv_moments", m["adv"][u * R1:(u + 1) * R1], R1, ws64, su[u], st)
        a2 = m["adv"].view(U, R1)
        a2.sub_(su[:, 0:1]).mul_(su[:, 1:2])
        return self.ident


class Group:
    """Rollout state of one group, the reference's (device, update-batch) replica of ``N`` envs (rec_magpo.py:519, :648-653): envs,
    trajectory, episode metrics, bootstrap value, PRNG key, the key table of one rollout (``key_shape`` per env step: on the host for
    an eager rollout, on the device for a captured one) and the rollout graph.  All groups of a process share the parameters and the
    training workspaces; the systems' groups add their hidden states."""

    def __init__(self, env_cfg, N: int, T: int, device, key_shape):
        A, F = env_cfg.num_agents, obs_row_stride(env_cfg.obs_dim)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=device)
        self.env = make_env_batch(env_cfg, N, device)
        self.traj = dict(obs=f32(T + 1, N, A, F), step_count=i32(T + 1, N), done=u8(T + 1, N), action=i32(T, N, A), value=f32(T, N, A),
                         reward=f32(T, N, A), log_prob=f32(T, N, A), adv=f32(T, N, A), targets=f32(T, N, A))
        # action masks (Observation.action_mask) only for envs that have illegal actions; None = every action legal
        self.traj["mask"] = u8(T + 1, N, A, env_cfg.num_actions) if env_cfg.has_mask else None
        self.metrics = dict(episode_return=f32(T, N), episode_length=i32(T, N), is_terminal_step=u8(T, N))
        self.last_val = f32(N, A)
        self.key = prng_key(0)
        self.keys_host = np.zeros((T, *key_shape, 2), np.uint32)
        self.keys_dev = torch.zeros(T, *key_shape, 2, dtype=torch.int32, device=device)
        self.cur = 0   # which of two double-buffered hidden states holds the carried one; 0 between rollouts (static graph arguments)
        self.graph, self.graph_failed, self.warmed = None, False, False


class AnakinLearner:
    n_loss: int           # loss scalars behind the gradients in the all-reduce message
    use_graph = True      # replay the whole rollout as one HIP graph (removes ~11K host launches per MAGPO rollout)
    batch_groups = True   # update_batch_size > 1: the minibatches of all local groups train as one batch of sequences
    groups: List[Group]
    grad_all: torch.Tensor              # [gradients of every network | loss scalars]: one all-reduce message
    grad_acc: Optional[torch.Tensor]    # num_groups > 1: the sum over groups when they train one after another
    loss_out: torch.Tensor

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device):
        self.env_cfg, self.N, self.sys, self.dev = env_cfg, num_envs, sys, device
        self.A, self.K, self.T = env_cfg.num_agents, env_cfg.num_actions, sys.rollout_length
        self.F, self.obs_off = net_obs(env_cfg)   # what the networks read: the whole row with the AgentIDWrapper's one-hot id, or the part behind it
        self.Fld = obs_row_stride(env_cfg.obs_dim)   # floats between rows as the env kernels write them
        if num_envs % sys.num_minibatches:
            raise ValueError("num_envs must be divisible by num_minibatches")
        self.L = lib()
        self.ws64 = torch.zeros(8 * 1024, dtype=torch.float64, device=device)
        self.gnorm = torch.zeros(2, dtype=torch.float32, device=device)
        self._adv = AdvStats(self.L, device)
        self._mb: Dict[str, torch.Tensor] = {}

    # group-0 shortcuts (single-group callers and the parity tests)
    env = property(lambda self: self.groups[0].env)
    traj = property(lambda self: self.groups[0].traj)
    metrics = property(lambda self: self.groups[0].metrics)
    key = property(lambda self: self.groups[0].key)

    def _st(self):
        return torch.cuda.current_stream().cuda_stream

    def _net_view(self, obs: torch.Tensor) -> torch.Tensor:
        """The part of the observation rows the networks read (net_obs): same rows, same stride, pointer behind the one-hot id."""
        return obs if self.obs_off == 0 else obs[..., self.obs_off:]

    # ------------------------------------------------------------------ setup (rec_magpo.py:642-660 = rec_mappo.py:495-513)
    def setup(self, key: np.ndarray, n_groups: int = 1, group: int = 0):
        """``n_groups`` = total number of groups in the job (ranks x local groups), ``group`` = global index of this process's first
        group.  Reset keys are rows 1.. of split(key, n_groups*N + 1) laid out row-major over (group, env); ONE step key is shared by
        every group (rec_magpo.py:660-671); every hidden state starts at zero."""
        self.setup_key = setup_env_groups(self.L, self.dev, self._st(), self.groups, key, self.N, n_groups, group)
        for g in self.groups:
            self._reset_states(g)

    # ------------------------------------------------------------------ rollout
    def rollout(self):
        """One rollout per group, one group after the other: eagerly, or (``use_graph``) eagerly once so that every workspace exists,
        then captured as one HIP graph and replayed from then on with only the key table uploaded."""
        for g in self.groups:
            self._rollout_keys(g)
            if not self.use_graph or g.graph_failed:
                self._rollout_body(g, g.keys_host)
            elif g.graph is not None:
                self._upload_keys(g)
                g.graph.replay()
            elif not g.warmed:
                self._rollout_body(g, g.keys_host)
                g.warmed = True
            else:
                self._upload_keys(g)
                self._capture(g)

    def _upload_keys(self, g: Group):
        # pageable source: the runtime stages the few KB immediately, so the host table can be reused right away
        g.keys_dev.copy_(torch.from_numpy(g.keys_host.view(np.int32).copy()))

    def _capture(self, g: Group):
        cur0 = g.cur
        try:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._rollout_body(g, g.keys_dev)
            g.graph = graph
            graph.replay()
        except Exception as e:  # capture is an optimisation: never let it change results
            warnings.warn(f"HIP graph capture of the rollout failed ({e!r}); running eagerly")
            g.graph, g.graph_failed, g.cur = None, True, cur0
            torch.cuda.synchronize()
            self._rollout_body(g, g.keys_host)

    def _carry_over(self):
        """Slot T of the trajectory becomes slot 0 of the next rollout."""
        for g in self.groups:
            tr = g.traj
            tr["obs"][0].copy_(tr["obs"][self.T]); tr["step_count"][0].copy_(tr["step_count"][self.T]); tr["done"][0].copy_(tr["done"][self.T])
            if tr["mask"] is not None:
                tr["mask"][0].copy_(tr["mask"][self.T])

    # ------------------------------------------------------------------ shuffles (jax.random.permutation)
    def _permutation(self, key: np.ndarray, n: int) -> torch.Tensor:
        return jax_permutation(self.L, self.dev, self._st(), key, n)

    # ------------------------------------------------------------------ one minibatch (rec_magpo.py:441-462)
    def _gather(self, groups: List[int], env_idx: torch.Tensor, agent_perm: torch.Tensor, shape=None):
        """Minibatch rows (j, t, a') of the listed groups, group after group, in sequence-major order.  ``h0idx`` (where the system's
        ``_mb_buffers`` has one): the rows of the sequences' GRU start states in the start states of all groups, stacked.  ``shape`` =
        (T, N) the time-major trajectory buffers are read as (default: as they are; a feed-forward learner gathers single steps, (1, T N))."""
        T, N = (self.T, self.N) if shape is None else shape
        A, F, K = self.A, self.Fld, self.K   # (observation rows are copied with their padding)
        mb, U = env_idx.numel(), len(groups)
        R1 = mb * T * A
        R = U * R1
        m = self._mb
        if m.get("R") != R:
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
            i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=self.dev)
            m.update(R=R, obs=f32(R, F), action=i32(R), prev=i32(R), pos=i32(R), done=torch.empty(U * mb, T, dtype=torch.uint8, device=self.dev),
                     value=f32(R), logp=f32(R), adv=f32(R), targets=f32(R),
                     mask=torch.empty(R, K, dtype=torch.uint8, device=self.dev) if self.env_cfg.has_mask else None, **self._mb_buffers(R, U * mb))
        for u, gi in enumerate(groups):
            tr = self.groups[gi].traj
            r = slice(u * R1, (u + 1) * R1)
            h0 = None if m["h0idx"] is None else m["h0idx"][u * mb * A:(u + 1) * mb * A]
            self.L.call("magpo_gather_minibatch", tr["obs"], tr["action"], tr["step_count"], tr["done"], tr["mask"], tr["value"], tr["log_prob"],
                        tr["adv"], tr["targets"], env_idx, agent_perm, m["obs"][r], m["action"][r], m["prev"][r], m["pos"][r],
                        m["done"][u * mb:(u + 1) * mb], None if m["mask"] is None else m["mask"][r], m["value"][r], m["logp"][r], m["adv"][r],
                        m["targets"][r], h0, T, N, A, F, K, mb, self._st())
            if gi and h0 is not None:
                h0.add_(gi * N * A)
        return m

    # ------------------------------------------------------------------ one optimisation step (rec_magpo.py:395-420 = rec_mappo.py:250-277)
    def _optimise(self, grads: Callable, grad_sync: Optional[Callable], row: torch.Tensor):
        """``grads(group)`` leaves the gradient of one minibatch of ``group`` (an index, or a list of groups that train as one batch of
        sequences) in grad_all.  Mean over the local groups, ``grad_sync`` (the all-reduce over ranks; returns what is left to scale by),
        the optimiser steps, and the loss scalars of the step into ``row``."""
        U = len(self.groups)
        scale = 1.0
        if U == 1:
            grads(0)
        elif self.batch_groups:   # all local groups as one batch of sequences: the row mean IS the pmean over "batch"
            grads(list(range(U)))
        else:  # group by group: accumulate, the 1/U goes into grad_scale
            self.grad_acc.zero_()
            for gi in range(U):
                grads(gi)
                self.grad_acc.add_(self.grad_all)
            self.grad_all.copy_(self.grad_acc)
            scale = 1.0 / U
        scale *= grad_sync(self) if grad_sync is not None else 1.0
        self.apply_grads(scale)
        self._loss_row(row)
        row.mul_(scale)

    def _loss_row(self, row: torch.Tensor):
        row.copy_(self.loss_out)

    def update_step(self, grad_sync=None):
        """One ``_update_step`` (rec_magpo.py:106-499, rec_mappo.py:70-362): rollout + GAE + training."""
        self.rollout()
        losses = self.update(grad_sync)
        self._carry_over()
        return losses
