"""Memoryless Sable learner on the MI355X kernels: the ff_sable system (mava/systems/sable/anakin/ff_sable.py:56-320).

Sable with retention over the agents of ONE time step: no hidden states, no decay, no timestep positional encoding
(``SableGuider(memory_type="ff_sable")``: every retention op is a stateless team kernel, csrc/team_retention.hip).  One update step is

  rollout   per env step (ff_sable.py:83-114): key, policy_key = split(key); the acting chain of the network on the observation alone
            (inside it key, sample_key = split(key) per agent, decode.py:141); env step.  Stored per step: action, value, reward, log_prob,
            obs, and ``done = timestep.last()`` of the step itself (:103) -- slot t + 1 of the trajectory's done flags, which is how
            magpo_gae reads them ("the observation of step t + 1 starts an episode"): the GAE of :135-155 without a next_done carry.
            Then the bootstrap value from one more acting call with its own key (:123-128).  The rollout is captured as one HIP graph on
            one stream like every learner's; a failed capture falls back to eager.
  epoch     key, batch_shuffle_key, agent_shuffle_key, entropy_key = split(key, 4) (:247); ONE permutation of rollout_length x num_envs
            items (:250-254: merge_leading_dims of a time-major batch makes item t * N + n, which is how the [T][N] trajectory buffers lie
            in memory, so magpo_gather_minibatch read as a (1, T N) trajectory gathers such items), then ONE agent permutation on the agent
            axis (:257-258), cut into num_minibatches slices (:261-264).
  minibatch the training forward on items x A token rows (nseq = items, T = 1); advantages normalised per minibatch and per group (:190);
            magpo_ppo_loss_fwd_bwd (:187-217); the hand-written backward; one all-reduce of [gradients | 4 loss scalars]; one clip + Adam.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

from .anakin import AnakinLearner, Group, SystemConfig
from .envs import agent_sample_keys, host_split
from .optim import ClipAdam
from .params import FlatParams, guider_layout
from .sable import SableGuider
from .tuning import Tuning

LOSS_NAMES = ("total_loss", "actor_loss", "entropy", "value_loss")   # order of k_ppo_loss_final


class FfSableLearner(AnakinLearner):
    """The groups' rollouts run one after the other on one stream: the acting workspaces inside the network are shared by all groups."""
    n_loss = 4

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device, *, net_seed: Optional[int] = 0, wgrad_groups: int = 512,
                 num_groups: int = 1, n_block: int = 1, n_head: int = 1, embed_dim: int = 64, tuning=None,
                 guider: Optional[SableGuider] = None, optim: Optional[ClipAdam] = None, apply_fns=None, update_fn=None):
        """``guider`` / ``optim``: the SableGuider (memory_type "ff_sable") and its ClipAdam built by the caller (ff_sable.learner_setup);
        by default the learner builds its own.  ``apply_fns`` = (sable_action_select_fn, sable_apply_fn) and ``update_fn`` as
        get_learner_fn receives them (ff_sable.py:54-55): by default ``guider.act`` (``guider.act_team_fused`` with
        ``Tuning.ff_sable_fused_act`` on), ``guider.apply`` and ``optim.update``."""
        super().__init__(env_cfg, num_envs, sys, device)
        if int(getattr(sys, "micro_batches", 1) or 1) != 1:
            raise NotImplementedError("system.micro_batches is not supported by ff_sable")
        if (self.T * num_envs) % sys.num_minibatches:
            raise ValueError("rollout_length * num_envs must be divisible by num_minibatches")
        self.tuning = tuning if tuning is not None else (guider.tuning if guider is not None else Tuning.from_env())
        A, K, F = self.A, self.K, self.F
        # the size of the parameter layout: the given network's own (a SableGuider, or another memoryless network with the same methods:
        # magpo_amd.mat.MatNetwork), else that of the SableGuider built below
        gn = guider.P.numel if guider is not None else FlatParams(guider_layout(int(embed_dim), F, K, int(n_block), int(n_head)), "cpu").numel
        # one contiguous buffer [gradients | loss scalars] = one all-reduce message (ff_sable.py:226-228)
        self.grad_all = torch.zeros(gn + 16, dtype=torch.float32, device=device)
        self.grad_acc = torch.zeros_like(self.grad_all) if num_groups > 1 else None
        if guider is None:
            guider = SableGuider(A, K, F, device, memory_type="ff_sable", max_pos=env_cfg.time_limit + 1, wgrad_groups=wgrad_groups,
                                 n_block=int(n_block), n_head=int(n_head), embed_dim=int(embed_dim), seed=net_seed, grads=self.grad_all[:gn],
                                 tuning=self.tuning, obs_ld=self.Fld)
        else:
            guider.bind_grads(self.grad_all[:gn])
        if not guider.ff:
            raise ValueError("FfSableLearner needs a SableGuider with memory_type='ff_sable'")
        if guider.F != F or guider.Fld != self.Fld:
            raise ValueError(f"network built for {guider.F} observation features with row stride {guider.Fld}, the env provides {F} with row "
                             f"stride {self.Fld}")
        self.guider = guider
        self.g_opt = optim if optim is not None else ClipAdam(guider, sys)
        assert self.g_opt.net is guider
        # acting step: one magpo_ff_sable_act launch (Tuning.ff_sable_fused_act) or the kernel-by-kernel chain; the caller's functions win
        if apply_fns is None:
            apply_fns = (guider.act_team_fused if self.tuning.ff_sable_fused_act else guider.act, guider.apply)
        self.sable_action_select_fn, self.sable_apply_fn = apply_fns
        self.sable_update_fn = update_fn if update_fn is not None else self.g_opt.update
        self.loss_out = self.grad_all[gn:gn + self.n_loss]
        # the key table of a rollout holds the A sample keys of every env step
        self.groups: List[Group] = [Group(env_cfg, num_envs, self.T, device, key_shape=(A,)) for _ in range(num_groups)]

    last_val = property(lambda self: self.groups[0].last_val)

    def _reset_states(self, g: Group):
        """Nothing is carried between env steps but the env itself."""

    # ------------------------------------------------------------------ rollout (ff_sable.py:83-160)
    def _rollout_keys(self, g: Group):
        """Host key chain of one rollout: key, policy_key = split(key) per env step (:90); inside get_actions key, sample_key = split(key)
        per agent (decode.py:141); one more split for the bootstrap value (:123; a value needs no sample)."""
        key = g.key
        for t in range(self.T):
            ks = host_split(key, 2)
            key, g.keys_host[t] = ks[0], agent_sample_keys(ks[1], self.A)[1]
        g.key = host_split(key, 2)[0]

    def _rollout_body(self, g: Group, skeys):
        """T acting steps, the bootstrap value and GAE, all on the current stream (no parallel branches in the captured graph)."""
        T, N, A = self.T, self.N, self.A
        tr, act = g.traj, self.sable_action_select_fn
        for t in range(T):
            mk = None if tr["mask"] is None else tr["mask"][t]
            act(self._net_view(tr["obs"][t]), tr["step_count"][t], None, skeys[t], tr["action"][t], tr["log_prob"][t], tr["value"][t], mask=mk)
            g.env.step(tr["action"][t], tr["reward"][t], tr["done"][t + 1], tr["obs"][t + 1], tr["step_count"][t + 1],
                       g.metrics["episode_return"][t], g.metrics["episode_length"][t], g.metrics["is_terminal_step"][t],
                       mask=None if tr["mask"] is None else tr["mask"][t + 1])
        act(self._net_view(tr["obs"][T]), tr["step_count"][T], None, None, None, None, g.last_val, value_only=True)
        self.L.call("magpo_gae", tr["reward"], tr["value"], tr["done"], g.last_val, tr["done"][T], tr["adv"], tr["targets"], T, N, A,
                    self.sys.gamma, self.sys.gae_lambda, self._st())

    # ------------------------------------------------------------------ one minibatch (ff_sable.py:165-242)
    def _mb_buffers(self, R: int, nseq: int):
        """Loss gradients of the logits and the values; no start states."""
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        return dict(dg=f32(R, 64), dv=f32(R), h0idx=None)

    def minibatch_grads(self, item_idx: torch.Tensor, agent_perm: torch.Tensor, group=0):
        """Forward + PPO loss + backward for one minibatch of items t * N + n (``item_idx`` int32) with their agents in ``agent_perm``
        order; gradients land in guider.grads, [total, actor_loss, entropy, value_loss] in self.loss_out (all inside self.grad_all).
        ``group``: one group index, or a list of groups that train as ONE batch (the loss is a mean over rows, so the batch gradient is
        the mean of the groups' gradients: the pmean over "batch", :226); the advantage normalisation stays per group (:190 in the vmap)."""
        s = self.sys
        groups = [group] if isinstance(group, int) else list(group)
        U = len(groups)
        m = self._gather(groups, item_idx, agent_perm, shape=(1, self.T * self.N))
        items = U * item_idx.numel()
        logits, value = self.sable_apply_fn(self._net_view(m["obs"]), m["prev"], m["pos"], m["done"], None, None, items, 1)
        stats = self._adv(m, U, None, self.ws64, self._st())
        self.L.call("magpo_ppo_loss_fwd_bwd", logits, 64, m["mask"], m["action"], m["logp"], m["value"], value, m["adv"], m["targets"], stats,
                    m["dg"], 64, m["dv"], self.ws64, self.loss_out, m["R"], self.K, s.clip_eps, s.ent_coef, s.vf_coef, self._st())
        self.guider.train_bwd(m["dg"], m["dv"])

    def apply_grads(self, grad_scale: float = 1.0):
        """optax clip_by_global_norm + adam + apply_updates (ff_sable.py:231-232): the one update function."""
        self.last_lr = self.sable_update_fn(grad_scale, self.ws64, self.gnorm[0:1])

    # ------------------------------------------------------------------ update (ff_sable.py:162-283)
    def update(self, grad_sync: Optional[Callable[["FfSableLearner"], float]] = None) -> torch.Tensor:
        """ppo_epochs x num_minibatches optimisation steps; returns the loss table [P, M, 4] (device) in the order of LOSS_NAMES."""
        s, n = self.sys, self.T * self.N
        M = s.num_minibatches
        mbs = n // M
        losses = torch.zeros(s.ppo_epochs, M, self.n_loss, device=self.dev)
        for e in range(s.ppo_epochs):
            ks = host_split(self.groups[0].key, 4)    # every group holds the same key => one pair of permutations serves all groups
            kb, ka, ke = ks[1], ks[2], ks[3]
            for g in self.groups:
                g.key = ks[0].copy()
            batch_perm = self._permutation(kb, n)
            agent_perm = self._permutation(ka, self.A)
            for mi in range(M):
                ke = host_split(ke, 2)[0]  # key, entropy_key = split(key) (:220): unused for discrete actions
                idx = batch_perm[mi * mbs:(mi + 1) * mbs].contiguous()
                self._optimise(lambda group: self.minibatch_grads(idx, agent_perm, group), grad_sync, losses[e, mi])
        return losses
