"""QMIX learner on the MI355X kernels: rec_qmix (mava/systems/q_learning/anakin/rec_qmix.py:233-533) on top of ``QLearner``.

  rollout   rec_iql's act loop; the stored reward is the team mean over agents (rec_qmix.py:287), written into every agent column of the
            step by ``magpo_team_reward`` in front of ``magpo_replay_add``, so the ring keeps rec_iql's layout.
  epoch     ``magpo_replay_gather_seq`` lays out all L stored steps of the sampled windows.  The reference unrolls the online network twice
            (rec_qmix.py:388 for the next greedy actions, :344 inside the loss) and the target network once, every time from a zero hidden
            state over rows of the same windows; here ONE online unroll over the L steps serves both (its steps 0 .. L-2 are the loss's Q
            values, its steps 1 .. L-1 select the next actions, with the same bits), so an epoch is two unrolls of L steps where rec_iql's is
            three of L - 1.  The target mixer (``magpo_qmix_fwd``, double-Q column selection inside the launch) mixes the target network's
            values of steps 1 .. L-1, the online mixer the taken actions' values of steps 0 .. L-2; ``magpo_qmix_td_loss`` gives dq_tot and
            the eight loss scalars, ``magpo_qmix_bwd`` the mixer gradients and the 64-wide Q-gradient rows ``seq_bwd`` takes (rows of step
            L - 1 stay zero).  Network gradients, mixer gradients and the loss scalars share one all-reduce message.
  optimiser optax.adam(q_lr) alone (rec_qmix.py:151-153): eps 1e-8, no clipping -- ``system.max_grad_norm`` is never read.  Without a global
            norm Adam is element-wise, so one ClipAdam per parameter buffer (max_norm = inf) equals one over the pair bit for bit.
            ``magpo_target_update`` runs once per buffer.

The ``ready()`` deviation of rec_iql (no training until the ring can be sampled) is kept.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .optim import ClipAdam
from .ppo_learner import raw_features
from .q_learner import QLearner, QSystemConfig, sample_window_indices
from .qmix_net import QMixer

LOSS_NAMES = ("q_loss", "mean_q", "max_q_error", "min_q_error", "mean_target", "mean_reward_t0", "mean_next_qval", "done")   # rec_qmix.py:361-367, :423-425


def adam_alone(net, sys) -> ClipAdam:
    """optax.adam(q_lr) (rec_qmix.py:151-153) on one parameter buffer."""
    return ClipAdam(net, sys, eps=1e-8, max_norm=math.inf)


class QmixLearner(QLearner):
    n_loss = 8
    SYSTEMS = "rec_qmix"

    def __init__(self, env_cfg, num_envs: int, sys: QSystemConfig, device, *, embed_dim: int = 32, norm_env_states: bool = True, mixer: Optional[QMixer] = None,
                 mixer_optim: Optional[ClipAdam] = None, mixer_seed=None, optim: Optional[ClipAdam] = None, **kw):
        """``mixer`` / ``mixer_optim``: the online mixer and its optimiser built by the caller (learner_setup); by default the learner builds its
        own from ``mixer_seed``.  The target mixer is a second object of the same layout.  Everything else as ``QLearner``."""
        super().__init__(env_cfg, num_envs, sys, device, optim=optim, **kw)
        A = self.A
        if mixer is None:
            mixer = QMixer(A, embed_dim, raw_features(env_cfg), device, id_cols=A, norm_env_states=norm_env_states, seed=mixer_seed)
        if (mixer.A, mixer.F_raw, mixer.id_cols) != (A, raw_features(env_cfg), A):
            raise ValueError(f"mixer built for {mixer.A} agents x {mixer.F_raw} raw features behind {mixer.id_cols} id columns; this system needs "
                             f"{A} x {raw_features(env_cfg)} behind {A}")
        self.mixer = mixer
        self.mixer_target = QMixer(A, mixer.E, mixer.F_raw, device, id_cols=mixer.id_cols, norm_env_states=mixer.norm)
        self.sync_target()
        n, nm = self.q_net.P.numel, mixer.P.numel
        self.grad_all = torch.zeros(n + nm + 16, dtype=torch.float32, device=device)   # [network | mixer | loss scalars]: one all-reduce message
        self.q_net.bind_grads(self.grad_all[:n])
        mixer.bind_grads(self.grad_all[n:n + nm])
        self.loss_out = self.grad_all[n + nm:n + nm + self.n_loss]
        if optim is None:
            self.q_opt = adam_alone(self.q_net, sys)
        self.mix_opt = mixer_optim if mixer_optim is not None else adam_alone(mixer, sys)
        assert self.mix_opt.net is mixer

    def sync_target(self):
        super().sync_target()
        if getattr(self, "mixer_target", None) is not None:   # (QLearner's constructor syncs before the mixers exist)
            self.mixer_target.P.flat.copy_(self.mixer.P.flat)

    def _before_add(self, g, t: int):
        r = g.traj["reward"][t]
        self.L.call("magpo_team_reward", r, r, self.N, self.A, self._st())

    def _train_rows(self, U: int):
        s, A, K, F = self.sys, self.A, self.K, self.Fld
        B, L_ = int(s.sample_batch_size), int(s.sample_sequence_length)
        R, Rm = U * B * L_ * A, U * B * (L_ - 1)
        m = self._mb
        if m.get("R") != R:
            e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=self.dev)
            m.clear()
            m.update(R=R, Rm=Rm, obs=e(R, F), mask=e(R, K, dt=torch.uint8) if self.env_cfg.has_mask else None, tot=e(U * B, L_, dt=torch.uint8),
                     action=e(Rm * A, dt=torch.int32), reward=e(Rm), q_tot=e(Rm), next_q_tot=e(Rm), dq_tot=e(Rm),
                     dq=torch.zeros(R, 64, device=self.dev),   # rows of step L - 1 are never written: they stay zero
                     idx=torch.zeros(U, 2, B, dtype=torch.int32, device=self.dev), h0=torch.zeros(U * B * A, 128, device=self.dev),
                     h0idx=torch.arange(U * B * A, dtype=torch.int32, device=self.dev))
        return m

    def epoch_grads(self, group=0):
        """Sample, gather, the two unrolls, both mixers, loss and backward for one epoch; the gradients land in q_net.grads / mixer.grads, the
        scalars in loss_out."""
        s, A, K = self.sys, self.A, self.K
        groups = [group] if isinstance(group, int) else list(group)
        U, B, L_ = len(groups), int(s.sample_batch_size), int(s.sample_sequence_length)
        m = self._train_rows(U)
        Rm, st = m["Rm"], self._st()
        idx = np.empty((U, 2, B), np.int32)
        for u, gi in enumerate(groups):
            g = self.groups[gi]
            idx[u, 0], idx[u, 1] = sample_window_indices(g.buff_key, B, L_, self.N, g.S, g.adds % g.S, min(g.adds, g.S))
        self._idx_host = idx
        m["idx"].copy_(torch.from_numpy(idx))
        R1, T = B * L_ * A, L_ - 1
        for u, gi in enumerate(groups):
            g = self.groups[gi]
            r, q = slice(u * R1, (u + 1) * R1), slice(u * B, (u + 1) * B)
            self.L.call("magpo_replay_gather_seq", *g.ring_fields(), self.N, g.S, A, self.Fld, K, m["idx"][u, 0], m["idx"][u, 1], B, L_, m["obs"][r], self.Fld,
                        None if m["mask"] is None else m["mask"][r], m["tot"][q], m["action"][u * B * T * A:(u + 1) * B * T * A], m["reward"][u * B * T:(u + 1) * B * T], st)
        nseq = U * B
        obs_view = self._net_view(m["obs"])
        q_target = self.target_net.seq_fwd(obs_view, m["tot"], m["h0"], m["h0idx"], nseq, L_)
        q_all = self.q_net.seq_fwd(obs_view, m["tot"], m["h0"], m["h0idx"], nseq, L_)
        self.mixer_target.apply(m["obs"], self.Fld, Rm, q_target, q_online=q_all, mask=m["mask"], K=K, steps=(T, L_, 1), out=m["next_q_tot"])
        self.mixer.apply(m["obs"], self.Fld, Rm, q_all, index=m["action"], K=K, steps=(T, L_, 0), train=True, out=m["q_tot"])
        self.L.call("magpo_qmix_td_loss", m["q_tot"], m["next_q_tot"], m["reward"], m["tot"], L_, s.gamma, m["dq_tot"], self.ws64, self.loss_out, Rm, U, st)
        self.mixer.bwd(m["dq_tot"], dq64=m["dq"])
        self.q_net.seq_bwd(m["dq"])

    def apply_grads(self, grad_scale: float = 1.0):
        """adam on both online parameter buffers, then both target updates with t_train before its increment (rec_qmix.py:430-449)."""
        s = self.sys
        self.last_lr = self.q_opt.update(grad_scale, self.ws64, self.gnorm[0:1])
        self.mix_opt.update(grad_scale, self.ws64, self.gnorm[1:2])
        for online, target in ((self.q_net, self.target_net), (self.mixer, self.mixer_target)):
            self.L.call("magpo_target_update", online.P.flat, target.P.flat, online.P.numel, 1 if s.hard_update else 0, s.tau, self.t_train_dev,
                        int(s.update_period), self._st())
        self.target_net.refresh()
        self.t_train += 1
        self.t_train_dev.add_(1)
