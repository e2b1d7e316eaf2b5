"""Recurrent double-Q learner on the MI355X kernels: rec_iql (mava/systems/q_learning/anakin/rec_iql.py:210-478).

One update step is an act-train loop (:429-478):

  rollout   new_key, act_key, train_key = split(key, 3) (:447); per env step new_key, explore_key = split(key) (:227), the Q network advances ONE
            step (GruQNetwork.step), magpo_eps_greedy_sample draws the actions from explore_key with eps formed in the kernel from the device
            env-step counter, the env kernel steps with real_next_obs, and magpo_replay_add stores the transition (obs, action, reward,
            terminal, term_or_trunc, real_next_obs) in the group's device ring.  The counter advances by num_envs per env step.  The rollout is
            one HIP graph per group like the other learners'; a failed capture falls back to eager and never changes results.
  epoch     next_key, buff_key = split(key) (:409); windows of sample_sequence_length steps are drawn uniformly (indices on the host from the
            threefry host entry points, one small upload), magpo_replay_gather lays their L - 1 aligned rows out as GruActor.seq_fwd reads
            them, the target network and the online network unroll over next_obs and the online network over obs, all from zero hidden
            states; magpo_q_td_loss gives the loss scalars and dQ, seq_bwd the gradient; mean over the local groups, ``grad_sync``, clip + Adam
            (q_lr, eps 1e-5, max_grad_norm) and magpo_target_update.  ``t_train`` counts epochs.

DEVIATION (the empty buffer): the reference trains from the very first update, when the buffer holds fewer steps than one window and what it
samples hangs on randint over an empty range.  Here the epochs of an update step are skipped until every group's ring holds at least
max(min_buffer_size, sample_sequence_length) steps: zero loss rows, no optimiser step, ``t_train`` does not advance; the keys are still split.
UNPINNED: the trajectory buffer (flashbax), Categorical(probs).sample (tfp) and the target updates (optax) are restated from memory; see
tests/iql_ref.py.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from ._lib import lib
from .anakin import AnakinLearner, Group
from .envs import ENV_BATCHES, host_split
from .optim import ClipAdam
from .q_net import GruQNetwork
from .tuning import Tuning

LOSS_NAMES = ("q_loss", "mean_q", "mean_target")   # loss_info of rec_iql.py:322-326
log = logging.getLogger(__name__)


@dataclass
class QSystemConfig:
    rollout_length: int = 2
    epochs: int = 2
    buffer_size: int = 1000
    min_buffer_size: int = 32
    sample_batch_size: int = 32
    sample_sequence_length: int = 32
    q_lr: float = 3e-4
    max_grad_norm: float = 10.0
    hard_update: bool = False
    update_period: int = 200
    tau: float = 0.01
    gamma: float = 0.99
    eps_min: float = 0.05
    eps_decay: float = 1e5
    micro_batches: int = 1
    # what AnakinLearner / ClipAdam read of every system's settings
    num_minibatches: int = 1
    ppo_epochs: int = 1
    decay_learning_rates: bool = False
    lr_num_updates: int = 1000

    @property
    def actor_lr(self) -> float:   # ClipAdam reads its rate under this name
        return self.q_lr


def epsilon(t: int, eps_min: float, eps_decay: float) -> float:
    """max(eps_min, 1 - (t / eps_decay) * (1 - eps_min)) in float32 in that order: what magpo_eps_greedy_sample forms from its counter."""
    f = np.float32
    return float(np.maximum(f(eps_min), f(f(1) - f(f(f(t) / f(eps_decay)) * f(f(1) - f(eps_min))))))


def _host_bits(key: np.ndarray, n: int) -> np.ndarray:
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty(n, np.uint32)
    lib().raw("magpo_random_bits_host")(key.ctypes.data, n, out.ctypes.data)
    return out


def host_randint(key: np.ndarray, n: int, span: int) -> np.ndarray:
    """jax.random.randint(key, (n,), 0, span) on the host from the threefry host entry points (exact; uint32 arithmetic)."""
    ks = host_split(key, 2)
    hi, lo = _host_bits(ks[0], n).astype(np.uint64), _host_bits(ks[1], n).astype(np.uint64)
    span = np.uint64(max(1, int(span)))
    m32 = np.uint64(0xFFFFFFFF)
    mult = np.uint64(1 << 16) % span
    mult = ((mult * mult) & m32) % span
    off = (((hi % span) * mult) & m32) + (lo % span) & m32
    return (off % span).astype(np.int32)


def sample_window_indices(key: np.ndarray, B: int, L: int, N: int, S: int, cursor: int, filled: int):
    """Uniform windows of L steps (UNPINNED restatement of flashbax's sampler, tests/iql_ref.py): key_batch, key_time = split(key); env row
    by randint(key_batch, B, 0, N); start by randint(key_time, B, 0, filled - L + 1) counted from the oldest stored step, so that no
    window straddles the write cursor.  Returns (env_idx [B], start [B]) int32."""
    n_valid = filled - L + 1
    if n_valid < 1:
        raise ValueError("the ring holds fewer steps than one window")
    ks = host_split(key, 2)
    oldest = cursor if filled == S else 0
    return host_randint(ks[0], B, N), ((oldest + host_randint(ks[1], B, n_valid)) % S).astype(np.int32)


class QGroup(Group):
    """A group of the Q learner: anakin.Group (envs, the rollout's observation slots, key table of explore keys) + the hidden state, the
    terminal flags, the env step's discount / real_next_obs outputs, the device ring with its two counters and the env-step counter."""

    def __init__(self, env_cfg, N: int, T: int, S: int, device):
        super().__init__(env_cfg, N, T, device, key_shape=())
        A, K, F = env_cfg.num_agents, env_cfg.num_actions, self.traj["obs"].shape[-1]
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)
        u8, i32 = torch.uint8, torch.int32
        self.h = [z(N * A, 128) for _ in range(2)]     # double-buffered; [0] holds the carried state between rollouts
        self.term = z(T + 1, N, dt=u8)                 # terminal flag of the observation in the same slot (1 - discount)
        self.discount, self.real_obs = z(N, A), z(N, A, F)
        has_mask = self.traj["mask"] is not None
        self.real_mask = z(N, A, K, dt=u8) if has_mask else None
        self.ring = dict(obs=z(N, S, A, F), mask=z(N, S, A, K, dt=u8) if has_mask else None, action=z(N, S, A, dt=i32), reward=z(N, S, A),
                         terminal=z(N, S, dt=u8), term_or_trunc=z(N, S, dt=u8), next_obs=z(N, S, A, F),
                         next_mask=z(N, S, A, K, dt=u8) if has_mask else None)
        self.cursor, self.filled, self.t_dev = z(1, dt=i32), z(1, dt=i32), z(1, dt=i32)
        self.adds = 0          # env steps stored so far: the host's copy of what cursor / filled hold (cursor = adds % S, filled = min(adds, S))
        self.t = 0             # env-step counter time_steps: the host's copy of t_dev
        self.S = S
        self.train_key = self.key.copy()

    def ring_fields(self):
        r = self.ring
        return (r["obs"], r["mask"], r["action"], r["reward"], r["terminal"], r["term_or_trunc"], r["next_obs"], r["next_mask"])

    def ring_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.ring.values() if t is not None)


def check_q_limits(env_cfg, L: int, S: int, micro_batches, system_name: str, env_name: Optional[str] = None) -> None:
    """What the Q learners' kernels serve, stated once for QLearner and for the systems' ``check_supported`` (which names the config's
    ``env_name`` too): no micro-batches, an env kernel that writes real_next_obs, windows of 2 <= L <= S steps, narrow rows."""
    if int(micro_batches or 1) != 1:
        raise NotImplementedError(f"system.micro_batches is not supported by {system_name}")
    if not ENV_BATCHES[type(env_cfg)].has_real_obs:
        cls = type(env_cfg).__name__
        if env_name is None:
            raise NotImplementedError(f"{system_name} on {cls}: the env kernel does not write real_next_obs (CoordSum and Level-Based Foraging do)")
        raise NotImplementedError(f"{system_name} on {env_name} ({cls}): the env kernel does not write real_next_obs; CoordSum and Level-Based Foraging do")
    if L < 2 or L > S:
        raise NotImplementedError(f"{system_name}: need 2 <= sample_sequence_length <= buffer_size, got {L} and {S}")
    if env_cfg.num_actions > 32 or env_cfg.obs_dim > 128:
        raise NotImplementedError("obs_dim <= 128 and action_dim <= 32 required")


class QLearner(AnakinLearner):
    n_loss = 3
    SYSTEMS = "rec_iql"

    def __init__(self, env_cfg, num_envs: int, sys: QSystemConfig, device, *, net_seed=0, wgrad_groups: int = 512, num_groups: int = 1, tuning=None,
                 q_net: Optional[GruQNetwork] = None, optim: Optional[ClipAdam] = None, torso=(None, None)):
        """``q_net`` / ``optim``: the online network and its ClipAdam built by the caller (learner_setup); by default the learner builds its own
        from ``net_seed`` (an int, a PRNG key or None) and the torso specs.  The target network is a second object of the same layout."""
        if not hasattr(env_cfg, "num_actions") or getattr(env_cfg, "continuous", False):
            raise NotImplementedError(f"{self.SYSTEMS}: discrete actions only")
        S = int(sys.buffer_size)
        check_q_limits(env_cfg, int(sys.sample_sequence_length), S, getattr(sys, "micro_batches", 1), self.SYSTEMS)
        super().__init__(env_cfg, num_envs, sys, device)
        self.tuning = tuning if tuning is not None else (q_net.tuning if q_net is not None else Tuning.from_env())
        A, K, F = self.A, self.K, self.F
        if q_net is None:
            q_net = GruQNetwork(A, K, F, device, wgrad_groups=wgrad_groups, seed=net_seed, tuning=self.tuning, obs_ld=self.Fld, pre_torso=torso[0],
                                post_torso=torso[1])
        if q_net.F != F or q_net.Fld != self.Fld or q_net.K != K:
            raise ValueError(f"network built for {q_net.F} features (row stride {q_net.Fld}) and {q_net.K} actions; this system needs {F} "
                             f"({self.Fld}) and {K}")
        self.q_net = q_net
        self.target_net = GruQNetwork(A, K, F, device, wgrad_groups=wgrad_groups, seed=None, tuning=self.tuning, obs_ld=self.Fld,
                                      pre_torso=q_net.pre_spec, post_torso=q_net.post_spec)
        self.sync_target()     # q_net.init(q_key, ...) twice (rec_iql.py:113-114): equal parameters, separate buffers
        n = q_net.P.numel
        self.grad_all = torch.zeros(n + 16, dtype=torch.float32, device=device)   # [gradients | loss scalars]: one all-reduce message
        self.grad_acc = None
        q_net.bind_grads(self.grad_all[:n])
        self.loss_out = self.grad_all[n:n + self.n_loss]
        self.q_opt = optim if optim is not None else ClipAdam(q_net, sys)
        assert self.q_opt.net is q_net
        self.groups: List[QGroup] = [QGroup(env_cfg, num_envs, self.T, S, device) for _ in range(num_groups)]
        log.info(self.SYSTEMS + ": replay ring of %d steps x %d envs per group: %.2f MiB", S, num_envs, self.groups[0].ring_bytes() / 2 ** 20)
        self.t_train = 0
        self.t_train_dev = torch.zeros(1, dtype=torch.int32, device=device)
        self._idx_host = None

    def sync_target(self):
        self.target_net.P.flat.copy_(self.q_net.P.flat)
        self.target_net.refresh()

    # ------------------------------------------------------------------ setup (rec_iql.py:155-195)
    def setup(self, key: np.ndarray, n_groups: int = 1, group: int = 0):
        """key, reset_key = split(key); env keys = split(reset_key, n_groups * N) laid out row-major over (group, env); the groups' learner
        keys = split(key, n_groups).  Hidden states, counters and rings start at zero; terminal / term_or_trunc of the reset step are 0."""
        U, N = len(self.groups), self.N
        if group < 0 or group + U > n_groups:
            raise ValueError(f"setup: this learner holds {U} env group(s) starting at group {group}, but the job has n_groups={n_groups}")
        ks = host_split(key, 2)
        first_keys = host_split(ks[0], n_groups)
        kd = torch.from_numpy(ks[1].view(np.int32).copy()).to(self.dev)
        allk = torch.empty(n_groups * N, 2, dtype=torch.int32, device=self.dev)
        self.L.call("magpo_threefry_split", kd, allk, n_groups * N, self._st())
        for gi, g in enumerate(self.groups):
            tr = g.traj
            g.env.reset(allk[(group + gi) * N:(group + gi + 1) * N].contiguous(), tr["obs"][0], tr["step_count"][0], None if tr["mask"] is None else tr["mask"][0])
            tr["done"][0].zero_(); g.term[0].zero_(); g.h[0].zero_()
            for t in g.ring_fields() + (g.cursor, g.filled, g.t_dev):
                if t is not None:
                    t.zero_()
            g.adds = g.t = 0
            g.key = first_keys[group + gi].copy()
        self.t_train = 0
        self.t_train_dev.zero_()
        self.setup_key = ks[0]

    def _reset_states(self, g):   # (setup above does it)
        g.h[0].zero_()

    # ------------------------------------------------------------------ rollout (rec_iql.py:210-278, :447-456)
    def _rollout_keys(self, g: QGroup):
        """new_key, act_key, train_key = split(key, 3); per env step key, explore_key = split(key).  Runs once per rollout and group, so the
        host's copies of the device counters advance here."""
        ks = host_split(g.key, 3)
        g.key, key, g.train_key = ks[0], ks[1], ks[2]
        for t in range(self.T):
            k2 = host_split(key, 2)
            key, g.keys_host[t] = k2[0], k2[1]
        g.adds += self.T
        g.t += self.T * self.N

    def _rollout_body(self, g: QGroup, ekeys):
        L, st, T, N, A, K, s = self.L, self._st(), self.T, self.N, self.A, self.K, self.sys
        tr = g.traj
        cur, on_dev = 0, torch.is_tensor(ekeys)
        for t in range(T):
            mk = None if tr["mask"] is None else tr["mask"][t]
            q = self.q_net.step(self._net_view(tr["obs"][t]), g.h[cur], tr["done"][t], g.h[1 - cur])
            cur = 1 - cur
            k0, k1 = (0, 0) if on_dev else (int(ekeys[t][0]), int(ekeys[t][1]))
            L.call("magpo_eps_greedy_sample", q, 64, mk, k0, k1, ekeys[t] if on_dev else None, g.t_dev, s.eps_min, s.eps_decay, tr["action"][t], None,
                   N * A, K, st)
            g.env.step(tr["action"][t], tr["reward"][t], tr["done"][t + 1], tr["obs"][t + 1], tr["step_count"][t + 1], g.metrics["episode_return"][t],
                       g.metrics["episode_length"][t], g.metrics["is_terminal_step"][t], mask=None if mk is None else tr["mask"][t + 1],
                       discount=g.discount, real_obs=g.real_obs, real_mask=g.real_mask)
            self._before_add(g, t)
            L.call("magpo_replay_add", *g.ring_fields(), g.cursor, g.filled, N, g.S, A, self.Fld, K, tr["obs"][t], self.Fld, mk, tr["action"][t],
                   tr["reward"][t], g.term[t], tr["done"][t], g.real_obs, self.Fld, g.real_mask, st)
            g.term[t + 1].copy_(g.discount[:, 0] == 0)     # next_terminal = 1 - discount (:264)
            g.t_dev.add_(N)                                # t + num_envs (:233)
        if cur != 0:  # keep the buffer roles identical from rollout to rollout (static graph arguments)
            g.h[0].copy_(g.h[1])

    def _before_add(self, g: QGroup, t: int):
        """What a derived system does to the env step in slot t before it is stored (rec_qmix: the team reward); nothing here."""

    def _carry_over(self):
        super()._carry_over()
        for g in self.groups:
            g.term[0].copy_(g.term[self.T])

    # ------------------------------------------------------------------ training (rec_iql.py:299-422)
    def ready(self) -> bool:
        """Whether every local group's ring can be sampled (the deviation in the module docstring); known on the host."""
        need = max(int(self.sys.min_buffer_size), int(self.sys.sample_sequence_length))
        return all(min(g.adds, g.S) >= need for g in self.groups)

    def _mb_buffers(self, R: int, nseq: int):
        return {}

    def _train_rows(self, U: int):
        """The stacked training rows of U groups (allocated once)."""
        s, A, K, F = self.sys, self.A, self.K, self.Fld
        B, T = int(s.sample_batch_size), int(s.sample_sequence_length) - 1
        R = U * B * T * A
        m = self._mb
        if m.get("R") != R:
            e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=self.dev)
            u8 = torch.uint8
            m.clear()
            m.update(R=R, obs=e(R, F), next_obs=e(R, F), action=e(R, dt=torch.int32), reward=e(R), tot=e(U * B, T, dt=u8), next_tot=e(U * B, T, dt=u8),
                     next_terminal=e(U * B, T, dt=u8), next_mask=e(R, K, dt=u8) if self.env_cfg.has_mask else None, qn_online=e(R, 64), dq=e(R, 64),
                     idx=torch.zeros(U, 2, B, dtype=torch.int32, device=self.dev), h0=torch.zeros(U * B * A, 128, device=self.dev),
                     h0idx=torch.arange(U * B * A, dtype=torch.int32, device=self.dev))
        return m

    def epoch_grads(self, group=0):
        """Sample, gather, the three unrolls, loss and backward for one epoch; the gradient lands in q_net.grads, the scalars in loss_out."""
        s, A, K = self.sys, self.A, self.K
        groups = [group] if isinstance(group, int) else list(group)
        U, B, L_ = len(groups), int(s.sample_batch_size), int(s.sample_sequence_length)
        T = L_ - 1
        m = self._train_rows(U)
        R, R1, st = m["R"], B * T * A, self._st()
        idx = np.empty((U, 2, B), np.int32)
        for u, gi in enumerate(groups):
            g = self.groups[gi]
            idx[u, 0], idx[u, 1] = sample_window_indices(g.buff_key, B, L_, self.N, g.S, g.adds % g.S, min(g.adds, g.S))
        self._idx_host = idx
        m["idx"].copy_(torch.from_numpy(idx))
        for u, gi in enumerate(groups):
            g = self.groups[gi]
            r, q = slice(u * R1, (u + 1) * R1), slice(u * B, (u + 1) * B)
            self.L.call("magpo_replay_gather", *g.ring_fields(), self.N, g.S, A, self.Fld, K, m["idx"][u, 0], m["idx"][u, 1], B, L_, m["obs"][r], self.Fld,
                        m["tot"][q], m["action"][r], m["reward"][r], m["next_obs"][r], self.Fld, None if m["next_mask"] is None else m["next_mask"][r],
                        m["next_tot"][q], m["next_terminal"][q], st)
        nseq = U * B
        next_view, obs_view = self._net_view(m["next_obs"]), self._net_view(m["obs"])
        qn_target = self.target_net.seq_fwd(next_view, m["next_tot"], m["h0"], m["h0idx"], nseq, T)
        m["qn_online"].copy_(self.q_net.seq_fwd(next_view, m["next_tot"], m["h0"], m["h0idx"], nseq, T))   # (the next unroll reuses the workspace)
        q = self.q_net.seq_fwd(obs_view, m["tot"], m["h0"], m["h0idx"], nseq, T)
        self.L.call("magpo_q_td_loss", q, m["qn_online"], qn_target, 64, m["action"], m["next_mask"], m["reward"], m["next_terminal"], s.gamma, m["dq"], 64,
                    self.ws64, self.loss_out, R, K, A, st)
        self.q_net.seq_bwd(m["dq"])

    def apply_grads(self, grad_scale: float = 1.0):
        """clip_by_global_norm + adam on the online parameters, then the target update with t_train before its increment (rec_iql.py:386-396)."""
        s = self.sys
        self.last_lr = self.q_opt.update(grad_scale, self.ws64, self.gnorm[0:1])
        n = self.q_net.P.numel
        self.L.call("magpo_target_update", self.q_net.P.flat, self.target_net.P.flat, n, 1 if s.hard_update else 0, s.tau, self.t_train_dev,
                    int(s.update_period), self._st())
        self.target_net.refresh()
        self.t_train += 1
        self.t_train_dev.add_(1)

    def update(self, grad_sync: Optional[Callable[["QLearner"], float]] = None) -> torch.Tensor:
        """``epochs`` training steps; returns the loss table [epochs, 1, 3] (device) in the order of LOSS_NAMES (zero rows while skipped)."""
        s = self.sys
        losses = torch.zeros(int(s.epochs), 1, self.n_loss, device=self.dev)
        ready = self.ready()
        for e in range(int(s.epochs)):
            for g in self.groups:
                ks = host_split(g.train_key, 2)      # next_key, buff_key = split(key) (:409)
                g.train_key, g.buff_key = ks[0], ks[1]
            if ready:
                self._optimise(self.epoch_grads, grad_sync, losses[e, 0])
        return losses
