"""Recurrent PPO learner on the MI355X kernels: rec_ippo / rec_mappo (mava/systems/ppo/anakin/rec_mappo.py:70-362).

A GRU actor and a GRU critic (magpo_amd/actor.py, critic.py) trained with PPO.  One update step is

  rollout   per env step (rec_mappo.py:92-144): key, policy_key = split(key); both networks advance ONE step (critic.step_pair: the two
            GRU cells in one launch); ONE categorical sample over the whole [N, A] batch from policy_key; env step.  Stored per step:
            last_done, action, value, reward, log_prob, obs.  The hidden states of both networks at rollout start are the chunk's
            start state.  Then the bootstrap value from one critic step (:155-162) and magpo_gae (:164-166).  The rollout is captured
            as one HIP graph like MagpoLearner's; a failed capture falls back to eager and never changes results.
  epoch     key, shuffle_key, entropy_key = split(key, 3) (:296); the N sequences are permuted with shuffle_key and cut into
            num_minibatches slices (:311-321); entropy_key is carried and never consumed for discrete actions (:235,293).
  minibatch both networks run their training scan from the stored start states; advantages normalised per minibatch and per group (:193);
            magpo_ppo_loss_fwd_bwd on the actor's logits and the critic's values (:176-232, the same terms); its dlogits drive
            actor.seq_bwd, its dvalue -- already scaled by vf_coef -- critic.seq_bwd; one all-reduce message
            [actor grads | critic grads | loss scalars]; two clip + Adam steps (actor_lr, critic_lr; :268-277).

``system.recurrent_chunk_size`` must be null or rollout_length: see ``check_chunk_size``.  For a centralised critic (rec_mappo) the
critic reads observation.global_state rows built by magpo_global_state from the stored observation rows (never stored themselves).
"""
from __future__ import annotations

import dataclasses
from typing import Callable, List, Optional

import torch

from .actor import GruActor
from .anakin import AnakinLearner, Group, SystemConfig
from .critic import GruCritic, global_state_ld, step_pair
from .envs import host_split
from .optim import ClipAdam
from .tuning import Tuning

LOSS_NAMES = ("total_loss", "value_loss", "actor_loss", "entropy")   # the reference's loss_info keys (rec_mappo.py:286-291)


def check_chunk_size(chunk, rollout_length: int) -> None:
    """system.recurrent_chunk_size: null or rollout_length (the eight tuned ippo / mappo rows use 128 = their rollout length)."""
    if chunk is None or int(chunk) == int(rollout_length):
        return
    raise NotImplementedError(
        f"system.recurrent_chunk_size={chunk} with rollout_length={rollout_length}: only null or rollout_length is supported.  With more than "
        "one chunk the reference's reshape (rec_mappo.py:300-310: x.reshape(chunk_size, num_envs * num_chunks, ...) of a time-major batch) "
        "interleaves time steps of different envs into one sequence; that layout is not restated here.")


def raw_features(env_cfg) -> int:
    """Width of one raw agent view: the stored observation row without the AgentIDWrapper's one-hot id (taken before it, make_env.py:90-104)."""
    return int(env_cfg.obs_dim) - int(env_cfg.num_agents)


class PpoGroup(Group):
    """A group of the PPO learner: anakin.Group + both hidden states; its key table holds the policy_key of every env step."""

    def __init__(self, env_cfg, N: int, T: int, device):
        super().__init__(env_cfg, N, T, device, key_shape=())
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        self.policy_h = [f32(N * env_cfg.num_agents, 128) for _ in range(2)]   # double-buffered; [0] holds the carried state between rollouts
        self.critic_h = [f32(N * env_cfg.num_agents, 128) for _ in range(2)]
        self.policy_h0 = self.critic_h0 = None                 # views of the learner's stacked start states


class PpoBase(AnakinLearner):
    """What the recurrent and the feed-forward PPO learner (ff_ppo_learner.FfPpoLearner) share: an actor and a critic with one optimiser each,
    the critic's input rows, the key chain of a rollout, the epoch loop, the two optimiser steps and the logged loss row.  The subclass
    supplies its networks, ``_shuffle_n`` (how many items an epoch permutes) and ``minibatch_grads(idx, group)``."""
    n_loss = 4
    SYSTEMS = "rec_ippo / rec_mappo"

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device, *, centralised: bool, tuning):
        super().__init__(env_cfg, num_envs, sys, device)
        self.tuning = tuning
        self.centralised = bool(centralised)
        if int(getattr(sys, "micro_batches", 1) or 1) != 1:
            raise NotImplementedError(f"system.micro_batches is not supported by {self.SYSTEMS}")
        # what the critic reads: agents_view rows, or global-state rows of num_agents * raw features (zero-padded to gs_ld)
        self.F_raw = raw_features(env_cfg)
        if self.centralised:
            self.gs_ld = global_state_ld(self.A, self.F_raw)    # raises beyond 128 inputs
            self.cF, self.cld = self.A * self.F_raw, self.gs_ld
        else:
            self.gs_ld = 0
            self.cF, self.cld = self.F, self.Fld

    def _bind_networks(self, actor, critic, sys: SystemConfig, critic_lr, optims, apply_fns, update_fns, num_groups: int):
        """Check the networks against the system, lay their gradients into one all-reduce message, build / take the optimisers and the four
        callables of get_learner_fn."""
        F, cF, cld, device = self.F, self.cF, self.cld, self.dev
        if actor.F != F or actor.Fld != self.Fld or critic.F != cF or critic.Fld != cld or critic.centralised != self.centralised:
            raise ValueError(f"networks built for {actor.F} / {critic.F} input features with row strides {actor.Fld} / {critic.Fld}; this system "
                             f"needs {F} / {cF} with row strides {self.Fld} / {cld} (centralised critic: {self.centralised})")
        self.actor, self.critic = actor, critic
        # one contiguous buffer [actor grads | critic grads | loss scalars] = one all-reduce message (rec_mappo.py:250-266)
        an, cn = actor.P.numel, critic.P.numel
        self.grad_all = torch.zeros(an + cn + 16, dtype=torch.float32, device=device)
        self.grad_acc = torch.zeros_like(self.grad_all) if num_groups > 1 else None
        actor.bind_grads(self.grad_all[:an])
        critic.bind_grads(self.grad_all[an:an + cn])
        self.loss_out = self.grad_all[an + cn:an + cn + self.n_loss]   # k_ppo_loss_final: [total, surrogate, entropy, value_loss]
        if optims is None:
            csys = dataclasses.replace(sys, actor_lr=float(sys.actor_lr if critic_lr is None else critic_lr))   # ClipAdam reads its rate as actor_lr
            optims = (ClipAdam(actor, sys), ClipAdam(critic, csys))
        self.a_opt, self.c_opt = optims
        assert self.a_opt.net is actor and self.c_opt.net is critic
        self.actor_apply_fn, self.critic_apply_fn = apply_fns if apply_fns is not None else (actor.apply, critic.apply)
        self.actor_update_fn, self.critic_update_fn = update_fns if update_fns is not None else (self.a_opt.update, self.c_opt.update)
        self._ident_perm = torch.arange(self.A, dtype=torch.int32, device=device)   # PPO does not permute agents
        self._gs_step = torch.zeros(self.N, self.A, self.gs_ld, device=device) if self.centralised else None

    def _critic_rows(self, obs_rows: torch.Tensor, n_env: int, out: Optional[torch.Tensor]) -> torch.Tensor:
        """The critic's input rows for ``n_env`` x A stored observation rows: the rows themselves, or their global state in ``out``."""
        if not self.centralised:
            return self._net_view(obs_rows)
        self.L.call("magpo_global_state", obs_rows, self.Fld, self.A, self.F_raw, out, self.gs_ld, n_env, self.A, self._st())
        return out

    def _rollout_keys(self, g: Group):
        """Host key chain of one rollout: key, policy_key = split(key) per env step (rec_mappo.py:106 = ff_mappo.py:83)."""
        key = g.key
        for t in range(self.T):
            ks = host_split(key, 2)
            key, g.keys_host[t] = ks[0], ks[1]
        g.key = key

    def apply_grads(self, grad_scale: float = 1.0):
        """Two optax chains clip_by_global_norm + adam (rec_mappo.py:435-442, :268-277)."""
        self.c_opt.sys.lr_num_updates = self.sys.lr_num_updates
        self.last_lr = self.actor_update_fn(grad_scale, self.ws64, self.gnorm[0:1])
        self.critic_update_fn(grad_scale, self.ws64, self.gnorm[1:2])

    def _shuffle_n(self) -> int:
        """Items one epoch permutes and cuts into num_minibatches slices."""
        raise NotImplementedError

    # ------------------------------------------------------------------ update (rec_mappo.py:168-350)
    def update(self, grad_sync: Optional[Callable[["PpoBase"], float]] = None) -> torch.Tensor:
        """ppo_epochs x num_minibatches optimisation steps; returns the loss table [P, M, 4] (device) in the order of LOSS_NAMES with the
        reference's logging quirk (rec_mappo.py:282-291): ``actor_loss`` is the actor's TOTAL (surrogate - ent_coef * entropy),
        ``value_loss`` the unscaled one, ``total_loss`` = actor total + vf_coef * value_loss."""
        s, n = self.sys, self._shuffle_n()
        M = s.num_minibatches
        mbs = n // M
        losses = torch.zeros(s.ppo_epochs, M, self.n_loss, device=self.dev)
        for e in range(s.ppo_epochs):
            ks = host_split(self.groups[0].key, 3)    # every group holds the same key => one permutation serves all groups
            kb, ke = ks[1], ks[2]
            for g in self.groups:
                g.key = ks[0].copy()
            batch_perm = self._permutation(kb, n)
            for mi in range(M):
                ke = host_split(ke, 2)[1]  # key, entropy_key = split(key); entropy_key is what the scan carries (:235,293), unused for discrete actions
                idx = batch_perm[mi * mbs:(mi + 1) * mbs].contiguous()
                self._optimise(lambda group: self.minibatch_grads(idx, group), grad_sync, losses[e, mi])
        return losses

    def _loss_row(self, row: torch.Tensor):
        """loss_out [total, surrogate, entropy, value_loss] in the order and with the quirk ``update`` documents."""
        lo = self.loss_out
        row[0].copy_(lo[0]); row[1].copy_(lo[3]); row[3].copy_(lo[2])
        torch.sub(lo[1], lo[2], alpha=self.sys.ent_coef, out=row[2])


class PpoLearner(PpoBase):
    """The groups' rollouts are never replayed side by side as MagpoLearner.rollout does: the acting step's workspaces inside the two
    networks and ``_gs_step`` are shared by all groups, so AnakinLearner.rollout's order, one group after the other on one stream, is
    what keeps them apart."""

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device, *, centralised: bool, critic_lr: Optional[float] = None,
                 net_seed: Optional[int] = 0, wgrad_groups: int = 512, num_groups: int = 1, tuning=None, actor: Optional[GruActor] = None,
                 critic: Optional[GruCritic] = None, optims=None, apply_fns=None, update_fns=None, actor_torso=(None, None),
                 critic_torso=(None, None)):
        """``centralised``: rec_mappo (the critic reads global-state rows) or rec_ippo (agents_view rows).  ``actor`` / ``critic`` /
        ``optims`` = (actor ClipAdam, critic ClipAdam): objects built by the caller (learner_setup); by default the learner builds its
        own from ``net_seed`` and the torso specs.  ``apply_fns`` = (actor_apply_fn, critic_apply_fn), ``update_fns`` =
        (actor_update_fn, critic_update_fn) (rec_mappo.py:67-68): the callables the minibatch CALLS for the two training forwards and the
        two optimiser steps -- by default the bound methods of the objects above."""
        super().__init__(env_cfg, num_envs, sys, device, centralised=centralised,
                         tuning=tuning if tuning is not None else (actor.tuning if actor is not None else Tuning.from_env()))
        A, K, F = self.A, self.K, self.F
        if actor is None:
            actor = GruActor(A, K, F, device, wgrad_groups=wgrad_groups, seed=net_seed, tuning=self.tuning, obs_ld=self.Fld,
                             pre_torso=actor_torso[0], post_torso=actor_torso[1])
        if critic is None:
            critic = GruCritic(A, self.cF, device, centralised=self.centralised, wgrad_groups=wgrad_groups, seed=None if net_seed is None else net_seed + 1,
                               tuning=self.tuning, obs_ld=self.cld, pre_torso=critic_torso[0], post_torso=critic_torso[1])
        self._bind_networks(actor, critic, sys, critic_lr, optims, apply_fns, update_fns, num_groups)
        self.groups: List[PpoGroup] = [PpoGroup(env_cfg, num_envs, self.T, device) for _ in range(num_groups)]
        U_, N_ = num_groups, num_envs
        self._policy_h0 = torch.zeros(U_ * N_ * A, 128, device=device)   # rollout-start states of all groups, stacked (h0 + h0_idx of the scans)
        self._critic_h0 = torch.zeros(U_ * N_ * A, 128, device=device)
        for gi, g in enumerate(self.groups):
            g.policy_h0 = self._policy_h0[gi * N_ * A:(gi + 1) * N_ * A]
            g.critic_h0 = self._critic_h0[gi * N_ * A:(gi + 1) * N_ * A]

    def _shuffle_n(self) -> int:
        return self.N   # the N sequences (rec_mappo.py:311-321)

    def _reset_states(self, g: PpoGroup):
        """Both hidden states start at zero (ScannedRNN.initialize_carry, rec_mappo.py:455-460)."""
        g.policy_h[0].zero_()
        g.critic_h[0].zero_()

    # ------------------------------------------------------------------ rollout (rec_mappo.py:92-166)
    def _rollout_body(self, g: PpoGroup, pkeys):
        """T acting steps, the bootstrap value and GAE, all on the current stream (no parallel branches in the captured graph).  The
        carried hidden states are in policy_h[0] / critic_h[0] before and after (T is even or odd: the last state is copied back)."""
        L, st, T, N, A = self.L, self._st(), self.T, self.N, self.A
        tr = g.traj
        g.policy_h0.copy_(g.policy_h[0])
        g.critic_h0.copy_(g.critic_h[0])
        cur, on_dev = 0, torch.is_tensor(pkeys)
        for t in range(T):
            obs_a = self._net_view(tr["obs"][t])
            obs_c = self._critic_rows(tr["obs"][t], N, self._gs_step)
            mk = None if tr["mask"] is None else tr["mask"][t]
            step_pair(self.actor, self.critic, obs_a, obs_c, tr["done"][t], g.policy_h[cur], g.policy_h[1 - cur], g.critic_h[cur], g.critic_h[1 - cur],
                      key=None if on_dev else pkeys[t], key_dev=pkeys[t] if on_dev else None, mask=mk,
                      action=tr["action"][t], log_prob=tr["log_prob"][t], value=tr["value"][t])
            cur = 1 - cur
            g.env.step(tr["action"][t], tr["reward"][t], tr["done"][t + 1], tr["obs"][t + 1], tr["step_count"][t + 1],
                       g.metrics["episode_return"][t], g.metrics["episode_length"][t], g.metrics["is_terminal_step"][t],
                       mask=None if tr["mask"] is None else tr["mask"][t + 1])
        if cur != 0:  # keep the buffer roles identical from rollout to rollout (static graph arguments)
            g.policy_h[0].copy_(g.policy_h[1])
            g.critic_h[0].copy_(g.critic_h[1])
        # bootstrap value: one critic step whose new hidden state is discarded (rec_mappo.py:159)
        val = self.critic.step(self._critic_rows(tr["obs"][T], N, self._gs_step), g.critic_h[0], tr["done"][T], g.critic_h[1])
        g.last_val.view(-1).copy_(val)
        L.call("magpo_gae", tr["reward"], tr["value"], tr["done"], g.last_val, tr["done"][T], tr["adv"], tr["targets"], T, N, A,
               self.sys.gamma, self.sys.gae_lambda, st)

    # ------------------------------------------------------------------ one minibatch (rec_mappo.py:171-293)
    def _mb_buffers(self, R: int, nseq: int):
        """Loss gradients of the logits and the values, the start-state rows of both GRUs, the critic's global-state rows."""
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        return dict(da=f32(R, 64), dv=f32(R), h0idx=torch.empty(nseq * self.A, dtype=torch.int32, device=self.dev),
                    gs=f32(R, self.gs_ld) if self.centralised else None)

    def minibatch_grads(self, env_idx: torch.Tensor, group=0):
        """Forward + loss + backward of both networks for one minibatch; gradients land in actor.grads / critic.grads, the loss scalars in
        self.loss_out (all inside self.grad_all).  ``group``: one group index, or a list of groups that train as ONE batch of sequences
        (the loss is a mean over rows, so the batch gradient is the mean of the groups' gradients: the pmean over "batch",
        rec_mappo.py:252-262); the advantage normalisation stays per group (:193 inside the vmap)."""
        s, T, K = self.sys, self.T, self.K
        groups = [group] if isinstance(group, int) else list(group)
        U = len(groups)
        m = self._gather(groups, env_idx, self._ident_perm)
        R, nseq = m["R"], U * env_idx.numel()
        logits = self.actor_apply_fn(self._net_view(m["obs"]), m["done"], self._policy_h0, m["h0idx"], nseq, T)
        value = self.critic_apply_fn(self._critic_rows(m["obs"], nseq * T, m["gs"]), m["done"], self._critic_h0, m["h0idx"], nseq, T)
        stats = self._adv(m, U, None, self.ws64, self._st())
        self.L.call("magpo_ppo_loss_fwd_bwd", logits, 64, m["mask"], m["action"], m["logp"], m["value"], value, m["adv"], m["targets"], stats,
                    m["da"], 64, m["dv"], self.ws64, self.loss_out, R, K, s.clip_eps, s.ent_coef, s.vf_coef, self._st())
        self.actor.seq_bwd(m["da"])
        self.critic.seq_bwd(m["dv"])    # dvalue is d(vf_coef * value_loss): the critic's total loss (rec_mappo.py:231)
