"""Feed-forward PPO learner on the MI355X kernels: ff_ippo / ff_mappo (mava/systems/ppo/anakin/ff_mappo.py:56-265).

A feed-forward actor and critic (magpo_amd/ff_nets.py) trained with PPO.  One update step is

  rollout   per env step (ff_mappo.py:76-99): key, policy_key = split(key); ONE launch takes the observation rows through both networks
            (ff_nets.act_pair -> magpo_mlp_act_step), ONE categorical sample over the whole [N, A] batch from policy_key; env step.  Stored per
            step: last_done, action, value, reward, log_prob, obs.  There are no hidden states.  Then the bootstrap value (:108) and magpo_gae
            (:110-112).  The rollout is captured as one HIP graph like every learner's; a failed capture falls back to eager.
  epoch     key, shuffle_key, entropy_key = split(key, 3) (:235); ONE permutation of rollout_length x num_envs items (:238-246) cut into
            num_minibatches slices.  merge_leading_dims(x, 2) of a time-major batch makes item t * N + n, which is how the [T][N] trajectory
            buffers lie in memory, so magpo_gather_minibatch read with T = 1, N = T * N gathers such items (tests/test_ff_ppo_system.py checks
            the order against the restatement).
  minibatch both training forwards; advantages normalised per minibatch and per group (:136); magpo_ppo_loss_fwd_bwd (:122-172, the terms of
            the recurrent systems); actor.bwd(dlogits), critic.bwd(dvalue); one all-reduce message [actor grads | critic grads | loss scalars];
            two clip + Adam steps (actor_lr, critic_lr; :209-217); the logged losses carry the quirk of :222-231.

What it shares with the recurrent learner (the critic's rows, the key chain, the epoch loop, the optimiser steps, the loss row) is
ppo_learner.PpoBase.  For a centralised critic (ff_mappo) the critic reads observation.global_state rows built by magpo_global_state.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .anakin import Group, SystemConfig
from .ff_nets import FfActor, FfCritic, act_pair
from .ppo_learner import PpoBase
from .tuning import Tuning


class FfPpoLearner(PpoBase):
    """As with PpoLearner the groups' rollouts run one after the other on one stream: the acting workspaces inside the networks and
    ``_gs_step`` are shared by all groups."""
    SYSTEMS = "ff_ippo / ff_mappo"

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device, *, centralised: bool, critic_lr: Optional[float] = None,
                 net_seed: Optional[int] = 0, wgrad_groups: int = 512, num_groups: int = 1, tuning=None, actor: Optional[FfActor] = None,
                 critic: Optional[FfCritic] = None, optims=None, apply_fns=None, update_fns=None, actor_torso=None, critic_torso=None):
        """Arguments as PpoLearner's; ``actor_torso`` / ``critic_torso``: one TorsoSpec each (these networks have only a pre-torso)."""
        super().__init__(env_cfg, num_envs, sys, device, centralised=centralised,
                         tuning=tuning if tuning is not None else (actor.tuning if actor is not None else Tuning.from_env()))
        if (self.T * num_envs) % sys.num_minibatches:
            raise ValueError("rollout_length * num_envs must be divisible by num_minibatches")
        if actor is None:
            actor = FfActor(self.A, self.K, self.F, device, wgrad_groups=wgrad_groups, seed=net_seed, tuning=self.tuning, obs_ld=self.Fld, torso=actor_torso)
        if critic is None:
            critic = FfCritic(self.A, self.cF, device, centralised=self.centralised, wgrad_groups=wgrad_groups,
                              seed=None if net_seed is None else net_seed + 1, tuning=self.tuning, obs_ld=self.cld, torso=critic_torso)
        self._bind_networks(actor, critic, sys, critic_lr, optims, apply_fns, update_fns, num_groups)
        self.groups: List[Group] = [Group(env_cfg, num_envs, self.T, device, key_shape=()) for _ in range(num_groups)]

    def _reset_states(self, g: Group):
        """Nothing is carried between env steps but the env itself."""

    def _shuffle_n(self) -> int:
        return self.T * self.N   # batch_size = rollout_length * num_envs (ff_mappo.py:238)

    # ------------------------------------------------------------------ rollout (ff_mappo.py:76-112)
    def _rollout_body(self, g: Group, pkeys):
        """T acting steps, the bootstrap value and GAE, all on the current stream (no parallel branches in the captured graph)."""
        T, N, A = self.T, self.N, self.A
        tr = g.traj
        on_dev = torch.is_tensor(pkeys)
        for t in range(T):
            obs_a = self._net_view(tr["obs"][t])
            obs_c = self._critic_rows(tr["obs"][t], N, self._gs_step)
            act_pair(self.actor, self.critic, obs_a, obs_c, key=None if on_dev else pkeys[t], key_dev=pkeys[t] if on_dev else None,
                     mask=None if tr["mask"] is None else tr["mask"][t], action=tr["action"][t], log_prob=tr["log_prob"][t], value=tr["value"][t])
            g.env.step(tr["action"][t], tr["reward"][t], tr["done"][t + 1], tr["obs"][t + 1], tr["step_count"][t + 1],
                       g.metrics["episode_return"][t], g.metrics["episode_length"][t], g.metrics["is_terminal_step"][t],
                       mask=None if tr["mask"] is None else tr["mask"][t + 1])
        self.critic.values(self._critic_rows(tr["obs"][T], N, self._gs_step), out=g.last_val)   # ff_mappo.py:108
        self.L.call("magpo_gae", tr["reward"], tr["value"], tr["done"], g.last_val, tr["done"][T], tr["adv"], tr["targets"], T, N, A,
                    self.sys.gamma, self.sys.gae_lambda, self._st())

    # ------------------------------------------------------------------ one minibatch (ff_mappo.py:117-232)
    def _mb_buffers(self, R: int, nseq: int):
        """Loss gradients of the logits and the values, the critic's global-state rows; no start states."""
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        return dict(da=f32(R, 64), dv=f32(R), h0idx=None, gs=f32(R, self.gs_ld) if self.centralised else None)

    def minibatch_grads(self, item_idx: torch.Tensor, group=0):
        """Forward + loss + backward of both networks for one minibatch of items t * N + n (``item_idx`` int32); gradients land in
        actor.grads / critic.grads, the loss scalars in self.loss_out (all inside self.grad_all).  ``group``: one group index, or a list of
        groups that train as ONE batch (the loss is a mean over rows, so the batch gradient is the mean of the groups' gradients: the pmean
        over "batch", ff_mappo.py:192-202); the advantage normalisation stays per group (:136 inside the vmap)."""
        s, K = self.sys, self.K
        groups = [group] if isinstance(group, int) else list(group)
        U = len(groups)
        m = self._gather(groups, item_idx, self._ident_perm, shape=(1, self.T * self.N))
        R, items = m["R"], U * item_idx.numel()
        logits = self.actor_apply_fn(self._net_view(m["obs"]))
        value = self.critic_apply_fn(self._critic_rows(m["obs"], items, m["gs"]))
        stats = self._adv(m, U, None, self.ws64, self._st())
        self.L.call("magpo_ppo_loss_fwd_bwd", logits, 64, m["mask"], m["action"], m["logp"], m["value"], value, m["adv"], m["targets"], stats,
                    m["da"], 64, m["dv"], self.ws64, self.loss_out, R, K, s.clip_eps, s.ent_coef, s.vf_coef, self._st())
        self.actor.bwd(m["da"])
        self.critic.bwd(m["dv"])    # dvalue is d(vf_coef * value_loss): the critic's total loss (ff_mappo.py:171)
