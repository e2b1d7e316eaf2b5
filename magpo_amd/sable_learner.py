"""Guider-only PPO learner on the MI355X kernels: the Sable system (mava/systems/sable/anakin/rec_sable.py:53-350).

``rec_sable`` is ``rec_magpo`` without the GRU actor: the same rollout (one acting launch per env step, Sable states read as zero where
``timestep.last()``, one more acting call with its own key for the bootstrap value), the same GAE, the same shuffles (batch permutation,
agent permutation, the cumulative ``prev_hstates`` permutation of quirk B19: rec_sable.py:272,298), one all-reduce of
``[gradients | 4 loss scalars]`` and one clip + Adam step per minibatch.  All of that is ``MagpoLearner``'s code (learner.py), run with
``has_actor = False``; what this module adds is the minibatch: Sable training forward -> PPO loss (csrc/rl.hip: k_ppo_loss) -> Sable backward.
``system.micro_batches`` works as for MAGPO (it lives in the shared update loop).
"""
from __future__ import annotations

from typing import Optional

import torch

from .learner import MagpoLearner, SystemConfig  # noqa: F401

LOSS_NAMES = ("total_loss", "actor_loss", "entropy", "value_loss")   # order of k_ppo_loss_final


class SableLearner(MagpoLearner):
    has_actor = False
    n_loss = 4

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device, *, guider=None, optim=None, apply_fns=None, update_fn=None, **kw):
        """``guider`` / ``optim``: the SableGuider and its ClipAdam built by the caller (rec_sable.learner_setup); ``apply_fns`` =
        (sable_action_select_fn, sable_apply_fn) and ``update_fn`` as get_learner_fn receives them (rec_sable.py:55-56).  Every other
        keyword is MagpoLearner's (net_seed, n_block, n_head, embed_dim, num_groups, tuning, ...)."""
        super().__init__(env_cfg, num_envs, sys, device, guider=guider, optims=None if optim is None else (optim, None),
                         apply_fns=None if apply_fns is None else (*apply_fns, None),
                         update_fns=None if update_fn is None else (update_fn, None), **kw)

    def minibatch_grads(self, env_idx: torch.Tensor, agent_perm: torch.Tensor, group=0, hs_idx: Optional[torch.Tensor] = None,
                        adv_stats: Optional[torch.Tensor] = None):
        """Forward + PPO loss + backward of the Sable network for one minibatch (_loss_fn, rec_sable.py:177-226); arguments as
        MagpoLearner.minibatch_grads.  Gradients land in guider.grads, [total, actor_loss, entropy, value_loss] in self.loss_out."""
        s, T = self.sys, self.T
        m, hidx, U, gcl, _ = self._minibatch_inputs(env_idx, agent_perm, group, hs_idx)
        logits, value = self.sable_apply_fn(self._net_view(m["obs"]), m["prev"], m["pos"], m["done"], self._prev_hs, hidx, U * env_idx.numel(), T,
                                            classes=gcl)
        stats = self._minibatch_stats(m, U, adv_stats)
        self.L.call("magpo_ppo_loss_fwd_bwd", logits, 64, m["mask"], m["action"], m["logp"], m["value"], value, m["adv"], m["targets"], stats,
                    m["dg"], 64, m["dv"], self.ws64, self.loss_out, m["R"], self.K, s.clip_eps, s.ent_coef, s.vf_coef, self._st())
        self.guider.train_bwd(m["dg"], m["dv"])

    def apply_grads(self, grad_scale: float = 1.0):
        """optax clip_by_global_norm + adam + apply_updates (rec_sable.py:247-248): the one update function."""
        self.last_lr = self.sable_update_fn(grad_scale, self.ws64, self.gnorm[0:1])
