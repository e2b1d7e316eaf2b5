"""MAGPO Anakin learner on the MI355X kernels: rollout -> GAE -> epochs x minibatches -> clip+Adam.

Host-side mirror of ``get_learner_fn`` (mava/systems/gpo/anakin/rec_magpo.py:91-530).  One instance is
one *group* (the reference's (device, update-batch) replica of ``num_envs`` envs); groups are
independent except for the mean of the gradients (rec_magpo.py:395-409), which the caller injects
through ``grad_sync`` (an RCCL all-reduce over xGMI in the multi-GPU launcher).

Data layout in HBM (no physical shuffle of activations; the minibatch gather moves only per-token
scalars, rec_magpo.py:441-462 becomes index arithmetic):
  trajectory  obs[T+1,N,A,F] f32, step_count[T+1,N] i32, done[T+1,N] u8 (slot t = "obs at step t starts an
              episode"), action/value/log_prob/reward/adv/targets [T,N,A]
  states      3 x [N,64,64] fp32 retention states, policy hidden [N*A,128]
  minibatch   rows (j, t, a') sequence-major, R = mb*T*A

Groups, set-up, the rollout's graph capture, the gather and the group dispatch of an optimisation step are AnakinLearner's (anakin.py).
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

from ._lib import lib  # noqa: F401
from .actor import GruActor
# what every learner shares lives in anakin.py, the environments in envs.py; their names are re-exported here for the callers that
# import them from the learner
from .anakin import AdvStats, AnakinLearner, Group, SystemConfig, jax_permutation, setup_env_groups, split_setup_keys  # noqa: F401
from .envs import (ConnectorEnvBatch, CoordSumConfig, CoordSumEnvBatch, LbfConfig, LbfEnvBatch, MpeConfig, MpeEnvBatch, RwareConfig,  # noqa: F401
                   RwareEnvBatch, VectorConnectorConfig, agent_sample_keys, host_split, make_env_batch, net_obs, obs_row_stride, prng_key)
from .optim import ClipAdam
from .params import FlatParams, actor_layout, guider_layout
from .sable import SableGuider
from .tuning import Tuning


class EnvGroup(Group):
    """A group of the MAGPO / Sable learner: anakin.Group + retention / GRU states; its key table holds the A sample keys of every step."""

    def __init__(self, env_cfg, N: int, T: int, device, n_block: int = 1, n_tile: int = 1, policy: bool = True):
        super().__init__(env_cfg, N, T, device, key_shape=(env_cfg.num_agents,))
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
        # (encoder, decoder self, decoder cross) retention states as 64 x 64 tiles: one (zero-padded) tile per head, or the four blocks of
        # the one 128-wide head (SableGuider.ntile)
        self.sable_hs = tuple(f32(n_block, n_tile, N, 64, 64) for _ in range(3))
        # GRU actor hidden states (double-buffered); a guider-only system has none
        self.policy_h = [f32(N * env_cfg.num_agents, 128) for _ in range(2)] if policy else None
        self.prev_sable_hs = self.policy_h0 = None   # rollout-start copies: views of the learner's stacked start states
        self.skeys_host, self.skeys_dev = self.keys_host, self.keys_dev   # the tables under the names of what they hold


class MagpoLearner(AnakinLearner):
    # What a guider-only system (sable_learner.SableLearner) turns off: the GRU actor with its hidden states, carry, training pass and
    # optimiser.  Everything else -- env groups, rollout body, HIP-graph capture, gather, shuffles, micro-batches, update loop -- is shared.
    has_actor = True
    n_loss = 9      # loss scalars behind the gradients in the all-reduce message (k_loss_final)

    def __init__(self, env_cfg, num_envs: int, sys: SystemConfig, device, *, net_seed: Optional[int] = 0,
                 decay_scaling_factor: float = 0.8, use_pe: bool = True, wgrad_groups: int = 512, num_groups: int = 1,
                 n_block: int = 1, n_head: int = 1, embed_dim: int = 64, tuning=None, guider: Optional[SableGuider] = None,
                 actor: Optional[GruActor] = None, optims=None, apply_fns=None, update_fns=None, actor_torso=(None, None)):
        """``guider`` / ``actor`` / ``optims`` = (guider ClipAdam, actor ClipAdam): networks and optimisers built by the caller
        (rec_magpo.learner_setup hands them to get_learner_fn as its apply / update functions); by default the learner builds its own.
        ``apply_fns`` = (sable_action_select_fn, sable_apply_fn, actor_apply_fn), ``update_fns`` = (sable_update_fn, actor_update_fn)
        (rec_magpo.py:99-100): the callables the loop CALLS for acting, the two training forwards and the two optimiser steps --
        by default the bound methods of the objects above; get_learner_fn passes on what it was given (thin adaptors included).
        ``actor_torso`` = (pre, post) TorsoSpecs of the actor the learner builds itself (None: the default [128] relu torso)."""
        super().__init__(env_cfg, num_envs, sys, device)
        self.tuning = tuning if tuning is not None else (guider.tuning if guider is not None else Tuning.from_env())   # ONE object shared by both networks (tuning.py)
        A, K, F = self.A, self.K, self.F
        # one contiguous buffer [guider grads | actor grads | loss scalars] = one all-reduce message (rec_magpo.py:395-409)
        if guider is not None:
            n_block, n_head, embed_dim = guider.nb, guider.nh, guider.EL
        self.nb, self.nh = int(n_block), int(n_head)
        gn = FlatParams(guider_layout(int(embed_dim), F, K, self.nb, self.nh), "cpu").numel
        an = 0 if not self.has_actor else actor.P.numel if actor is not None else FlatParams(actor_layout(F, 128, K, *actor_torso), "cpu").numel
        self.grad_all = torch.zeros(gn + an + 16, dtype=torch.float32, device=device)
        self.grad_acc = torch.zeros_like(self.grad_all) if num_groups > 1 else None
        self.grad_mu = torch.zeros_like(self.grad_all) if sys.micro_batches > 1 else None
        if guider is None:
            guider = SableGuider(A, K, F, device, decay_scaling_factor=decay_scaling_factor, use_pe=use_pe,
                                 max_pos=env_cfg.time_limit + 1, wgrad_groups=wgrad_groups, n_block=self.nb, n_head=self.nh, embed_dim=int(embed_dim),
                                 seed=None if net_seed is None else net_seed, grads=self.grad_all[:gn], tuning=self.tuning, obs_ld=self.Fld)
        else:
            guider.bind_grads(self.grad_all[:gn])
        if not self.has_actor:
            actor = None
        elif actor is None:
            actor = GruActor(A, K, F, device, wgrad_groups=wgrad_groups, seed=None if net_seed is None else net_seed + 1,
                             grads=self.grad_all[gn:gn + an], tuning=self.tuning, obs_ld=self.Fld, pre_torso=actor_torso[0],
                             post_torso=actor_torso[1])
        else:
            actor.bind_grads(self.grad_all[gn:gn + an])
        nets = [n for n in (guider, actor) if n is not None]
        if any(n.F != F or n.Fld != self.Fld for n in nets):
            raise ValueError(f"networks built for {' / '.join(str(n.F) for n in nets)} observation features with row stride "
                             f"{' / '.join(str(n.Fld) for n in nets)}, the env provides {F} with row stride {self.Fld}")
        self.guider, self.actor = guider, actor
        self.g_opt, self.a_opt = optims if optims is not None else (ClipAdam(guider, sys), ClipAdam(actor, sys) if actor is not None else None)
        assert self.g_opt.net is guider and (self.a_opt is None or self.a_opt.net is actor)
        self.sable_action_select_fn, self.sable_apply_fn, self.actor_apply_fn = apply_fns if apply_fns is not None else \
            (guider.get_actions, guider.apply, actor.apply if actor is not None else None)
        self.sable_update_fn, self.actor_update_fn = update_fns if update_fns is not None else \
            (self.g_opt.update, self.a_opt.update if self.a_opt is not None else None)
        self.loss_out = self.grad_all[gn + an:gn + an + self.n_loss]
        self.nt = self.guider.ntile
        self.groups: List[EnvGroup] = [EnvGroup(env_cfg, num_envs, self.T, device, self.nb, self.nt, policy=self.has_actor)
                                       for _ in range(num_groups)]
        # rollout-start states of all groups in ONE tensor each (group g = envs g*N .. g*N + N - 1), so that the minibatches of all
        # local groups train as one batch of sequences (update(): the groups differ only in their advantage statistics)
        U_, N_ = num_groups, num_envs
        self._prev_hs = tuple(torch.zeros(self.nb, self.nt, U_ * N_, 64, 64, device=device) for _ in range(3))
        self._policy_h0 = torch.zeros(U_ * N_ * A, 128, device=device) if self.has_actor else None
        for gi, g in enumerate(self.groups):
            g.prev_sable_hs = tuple(t[:, :, gi * N_:(gi + 1) * N_] for t in self._prev_hs)
            if self.has_actor:
                g.policy_h0 = self._policy_h0[gi * N_ * A:(gi + 1) * N_ * A]
        # First-layer class tables (csrc/classtab.hip): a wrapped CoordSum token is one of A*maxval*npos distinct inputs, so the
        # layers in front of the GRU / of the first retention run on the distinct rows only.  MAGPO_CLASS_TABLES=0 = dense path.
        # (the tables are read in place by the 64-wide fused kernels: a 128-wide net takes the dense first layers)
        # (... and need the one-hot id in the network input: the class rows are [id | target])
        self.class_tables = env_cfg.class_tables and self.tuning.class_tables and int(embed_dim) <= 64 and self.obs_off == 0
        self._cls = None
        # the actor's forward / backward run on a second HIP stream next to the guider's (independent until the loss)
        self.overlap_actor = False  # opt-in (bench.py --overlap): ~3 %, but per-kernel timings then include contention
        self._actor_stream = torch.cuda.Stream(device=device) if torch.device(device).type == "cuda" else None

    # the optimiser state (optax adam: count, mu, nu) lives in the two ClipAdam objects; the parity tests read it under these names
    g_mu = property(lambda self: self.g_opt.mu)
    g_nu = property(lambda self: self.g_opt.nu)
    a_mu = property(lambda self: self.a_opt.mu)
    a_nu = property(lambda self: self.a_opt.nu)
    g_count = property(lambda self: self.g_opt.count)

    # more group-0 shortcuts (AnakinLearner has env, traj, metrics and key)
    sable_hs = property(lambda self: self.groups[0].sable_hs)
    policy_h = property(lambda self: self.groups[0].policy_h)
    last_val = property(lambda self: self.groups[0].last_val)
    _cur = property(lambda self: self.groups[0].cur)

    def _reset_states(self, g: EnvGroup):
        for h in g.sable_hs:
            h.zero_()
        if self.has_actor:
            g.policy_h[0].zero_()
        g.cur = 0

    # ------------------------------------------------------------------ rollout (rec_magpo.py:126-212)
    overlap_actor_step = False  # (measured slower: the acting kernel already fills every wave slot) actor hidden-state carry on a side stream beside the guider's acting kernel
    batched_actor_carry = True  # actor hidden-state carry as ONE scan over the finished trajectory (not T single steps)
    fused_act = True  # one launch per env step for the whole Sable acting step (csrc/act_fused_kernel.hpp)

    def rollout(self):
        if len(self.groups) > 1 and self.use_graph and self.fused_act and self.A <= 8 and self.class_tables and self.batched_actor_carry \
                and all(g.graph is not None for g in self.groups):
            # the groups' rollouts are independent: replay their graphs side by side (at small num_envs a rollout is a latency
            # chain that leaves most of the chip idle)
            main = torch.cuda.current_stream()
            for g in self.groups:
                self._rollout_keys(g)
                self._upload_keys(g)
            for gi, g in enumerate(self.groups):
                st = self._group_stream(gi)
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    g.graph.replay()
            for gi in range(len(self.groups)):
                main.wait_stream(self._group_stream(gi))
            return
        super().rollout()

    def _group_stream(self, gi: int):
        if not hasattr(self, "_gstreams"):
            self._gstreams = {}
        if gi not in self._gstreams:
            self._gstreams[gi] = torch.cuda.Stream(device=self.dev)
        return self._gstreams[gi]

    def _rollout_keys(self, g: EnvGroup):
        """Host key chain of one rollout (pure function of the carried key): key, policy_key = split(key) per env
        step (rec_magpo.py:135); inside get_actions key, sample_key = split(key) per agent (decode.py:141); one
        more split for the bootstrap value (:202).  The A sample keys per step go to a device table."""
        T, A = self.T, self.A
        tab = g.skeys_host
        key = g.key
        for t in range(T):
            ks = host_split(key, 2)
            key, tab[t] = ks[0], agent_sample_keys(ks[1], A)[1]
        g.key = host_split(key, 2)[0]

    def _rollout_body(self, g: EnvGroup, skeys):
        L, st, T, N, A = self.L, self._st(), self.T, self.N, self.A
        tr = g.traj
        for d, s in zip(g.prev_sable_hs, g.sable_hs):
            d.copy_(s)
        if self.has_actor:
            g.policy_h0.copy_(g.policy_h[g.cur])
        main = torch.cuda.current_stream()
        side = self._actor_stream if self.overlap_actor_step and self.has_actor else None
        fused = self.fused_act
        gtag = str(self.groups.index(g))
        act = (lambda *a, **k: self.sable_action_select_fn(*a, tag=gtag, **k)) if fused else self.guider.act

        def zero_done(done):
            for k in range(self.nb):
                for h in range(self.nt):
                    L.call("magpo_zero_states_where_done", g.sable_hs[0][k][h], g.sable_hs[1][k][h], g.sable_hs[2][k][h], done, N, st)

        for t in range(T):
            obs, pos, done_prev = self._net_view(tr["obs"][t]), tr["step_count"][t], tr["done"][t]
            if self.has_actor and not self.batched_actor_carry:
                # the actor's hidden-state carry is a pure function of (obs, done); per step it can run on a side stream
                h_in, h_out = g.policy_h[g.cur], g.policy_h[1 - g.cur]
                if side is not None:
                    side.wait_stream(main)
                    with torch.cuda.stream(side):
                        self.actor.step(obs, h_in, done_prev, h_out)
                else:
                    self.actor.step(obs, h_in, done_prev, h_out)
                g.cur = 1 - g.cur
            mk = None if tr["mask"] is None else tr["mask"][t]
            if fused:   # states of envs whose episode just ended read as zero inside the kernel (rec_magpo.py:164-169); the decoder-state
                # update of a step is deferred to the next launch (each state read + written once per step, csrc/act_fused.hip)
                act(obs, pos, g.sable_hs, skeys[t], tr["action"][t], tr["log_prob"][t], tr["value"][t], done=done_prev, mask=mk,
                    pending=t > 0, flush=False, precand=t > 0, defer=True)
            else:
                act(obs, pos, g.sable_hs, skeys[t], tr["action"][t], tr["log_prob"][t], tr["value"][t], mask=mk)
            g.env.step(tr["action"][t], tr["reward"][t], tr["done"][t + 1], tr["obs"][t + 1], tr["step_count"][t + 1],
                       g.metrics["episode_return"][t], g.metrics["episode_length"][t], g.metrics["is_terminal_step"][t],
                       mask=None if tr["mask"] is None else tr["mask"][t + 1])
            if not fused:
                zero_done(tr["done"][t + 1])
        if side is not None:
            main.wait_stream(side)
        if self.has_actor and self.batched_actor_carry:   # one scan over the finished trajectory instead of T single steps (same result)
            ccl = None
            if self.class_tables:   # input side of the GRU on the A*maxval distinct (agent, target) rows
                if getattr(g, "traj_cls", None) is None:
                    g.traj_cls = torch.empty(T * N * A, dtype=torch.int32, device=self.dev)
                L.call("magpo_coordsum_classes", tr["obs"], self.F, None, None, A, self.env_cfg.maxval, 1, g.traj_cls, None, T * N * A, st)
                ccl = (self._class_rows()["obs_act"], g.traj_cls)
            self.actor.carry(self._net_view(tr["obs"][:T]), g.policy_h[g.cur], tr["done"][:T], g.policy_h[1 - g.cur], classes=ccl, tag=gtag)
            g.cur = 1 - g.cur
        if g.cur != 0:  # keep the buffer roles identical from rollout to rollout (static graph arguments)
            g.policy_h[0].copy_(g.policy_h[1])
            g.cur = 0
        if fused:   # bootstrap value (encoder states of just-ended episodes read as zero) + the last step's pending decoder-state update
            act(self._net_view(tr["obs"][T]), tr["step_count"][T], g.sable_hs, None, None, None, g.last_val, value_only=True, done=tr["done"][T], pending=True, flush=True, precand=True)
            zero_done(tr["done"][T])
        else:
            act(self._net_view(tr["obs"][T]), tr["step_count"][T], g.sable_hs, None, None, None, g.last_val, value_only=True)
        L.call("magpo_gae", tr["reward"], tr["value"], tr["done"], g.last_val, tr["done"][T], tr["adv"], tr["targets"], T, N, A,
               self.sys.gamma, self.sys.gae_lambda, st)

    # ------------------------------------------------------------------ one minibatch (rec_magpo.py:217-435)
    def _mb_buffers(self, R: int, nseq: int):
        """Loss gradients of the guider's logits, the actor's logits and the values; the start-state rows of the GRU actor."""
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
        return dict(dg=f32(R, 64), da=f32(R, 64) if self.has_actor else None, dv=f32(R),
                    h0idx=torch.empty(nseq * self.A, dtype=torch.int32, device=self.dev) if self.has_actor else None)

    def _class_rows(self):
        """Distinct first-layer inputs of wrapped CoordSum tokens, in class order (built once)."""
        if self._cls is None:
            A, K, mv, npos = self.A, self.K, self.env_cfg.maxval, self.env_cfg.time_limit + 1
            Ce, Cd = A * mv * npos, (K + 1) * npos
            c = dict(Ce=Ce, Cd=Cd, Ca=A * mv, npos=npos, obs_enc=torch.empty(Ce, self.F, device=self.dev),
                     pos_enc=torch.empty(Ce, dtype=torch.int32, device=self.dev), prev_dec=torch.empty(Cd, dtype=torch.int32, device=self.dev),
                     pos_dec=torch.empty(Cd, dtype=torch.int32, device=self.dev))
            self.L.call("magpo_coordsum_class_rows", A, mv, npos, K, c["obs_enc"], c["pos_enc"], c["prev_dec"], c["pos_dec"], self._st())
            if self.has_actor:
                c["obs_act"] = c["obs_enc"][::npos].contiguous()     # actor class (agent, target) = encoder class // npos
            c["zero"] = torch.zeros(1, dtype=torch.int64, device=self.dev)
            self._cls = c
        return self._cls

    def _classes(self, m):
        """Class index of every minibatch row and the stable row order per class (one sort per network side; the actor's
        classes are a coarsening of the encoder's, so it shares that order)."""
        c = self._class_rows()
        R = m["R"]
        if m.get("cls_R") != R:
            m.update(cls_R=R, cls_enc=torch.empty(R, dtype=torch.int32, device=self.dev), cls_dec=torch.empty(R, dtype=torch.int32, device=self.dev))
        self.L.call("magpo_coordsum_classes", m["obs"], self.F, m["prev"], m["pos"], self.A, self.env_cfg.maxval, c["npos"],
                    m["cls_enc"], m["cls_dec"], R, self._st())
        out = {}
        for side, C in (("enc", c["Ce"]), ("dec", c["Cd"])):
            cls = m["cls_" + side]
            vals, order = torch.sort(cls, stable=True)
            # class boundaries in the sorted order without a host synchronisation (torch.bincount sizes its output on the host)
            if ("bounds_" + side) not in c:
                c["bounds_" + side] = torch.arange(C + 1, dtype=torch.int32, device=self.dev)
            offsets = torch.searchsorted(vals, c["bounds_" + side])
            out[side] = (cls, order, offsets)
        if not self.has_actor:
            return out
        cls_act = torch.div(m["cls_enc"], c["npos"], rounding_mode="floor").to(torch.int32)
        out["act"] = (c["obs_act"], cls_act, out["enc"][1], out["enc"][2][::c["npos"]].contiguous())
        return out

    def _minibatch_adv_stats(self, group, env_idx: torch.Tensor) -> torch.Tensor:
        """(mean, 1 / (std + eps)) of the advantages of the minibatch's envs per group [U, 2] (rec_magpo.py:283,356): what
        minibatch_grads computes from its gathered rows, here for the WHOLE minibatch ahead of its micro-batches."""
        groups = [group] if isinstance(group, int) else list(group)
        out = torch.zeros(len(groups), 2, device=self.dev)
        for u, gi in enumerate(groups):
            sel = self.groups[gi].traj["adv"][:, env_idx.long(), :].contiguous()
            self.L.call("magpo_adv_moments", sel, sel.numel(), self.ws64, out[u], self._st())
        return out

    def minibatch_grads(self, env_idx: torch.Tensor, agent_perm: torch.Tensor, group=0, hs_idx: Optional[torch.Tensor] = None,
                        adv_stats: Optional[torch.Tensor] = None):
        """Forward + loss + backward of both networks for one minibatch; gradients land in guider.grads / actor.grads, loss
        scalars in self.loss_out (all inside self.grad_all, on device).  ``group``: one group index, or a list of groups that
        train as ONE batch of sequences -- every group uses the same env / agent permutation and the loss is a mean
        over rows, so the batch gradient is the unweighted mean of the groups' gradients (the pmean over the "batch" axis,
        rec_magpo.py:395-397); only the advantage normalisation stays per group (rec_magpo.py:283,356).
        ``hs_idx`` [mb]: env whose rollout-start Sable states sequence j trains on (quirk B19: in the reference
        it differs from ``env_idx`` after the first PPO epoch); default = ``env_idx``.  ``adv_stats`` [U, 2]: advantage statistics to
        use instead of those of the rows at hand (micro-batches: the statistics of the whole minibatch)."""
        s, T, K = self.sys, self.T, self.K
        m, hidx, U, gcl, acl = self._minibatch_inputs(env_idx, agent_perm, group, hs_idx)
        R, nseq = m["R"], U * env_idx.numel()
        side = self._actor_stream if self.overlap_actor else None
        main = torch.cuda.current_stream()
        if side is not None:
            side.wait_stream(main)  # minibatch gather (and the previous optimiser step) are complete for the actor
            with torch.cuda.stream(side):
                a_logits = self.actor_apply_fn(self._net_view(m["obs"]), m["done"], self._policy_h0, m["h0idx"], nseq, T, classes=acl)
        g_logits, value = self.sable_apply_fn(self._net_view(m["obs"]), m["prev"], m["pos"], m["done"], self._prev_hs, hidx, nseq, T, classes=gcl)
        if side is not None:
            main.wait_stream(side)
        else:
            a_logits = self.actor_apply_fn(self._net_view(m["obs"]), m["done"], self._policy_h0, m["h0idx"], nseq, T, classes=acl)
        st = self._st()
        stats = self._minibatch_stats(m, U, adv_stats)
        self.L.call("magpo_loss_fwd_bwd", g_logits, 64, a_logits, 64, m["mask"], m["action"], m["logp"], m["value"], value, m["adv"], m["targets"],
                    stats, m["dg"], 64, m["da"], 64, m["dv"], self.ws64, self.loss_out, R, K, s.clip_eps, s.clip_gpo,
                    s.ent_coef, s.vf_coef, s.alpha, st)
        if side is not None:
            side.wait_stream(main)  # loss gradients are ready
            with torch.cuda.stream(side):
                self.actor.seq_bwd(m["da"])
        self.guider.train_bwd(m["dg"], m["dv"])
        if side is not None:
            main.wait_stream(side)
        else:
            self.actor.seq_bwd(m["da"])

    def _minibatch_inputs(self, env_idx: torch.Tensor, agent_perm: torch.Tensor, group, hs_idx: Optional[torch.Tensor]):
        """What every system's minibatch starts from: the gathered rows, the start-state rows of their sequences, the number of groups
        in the batch and the (guider, actor) class tables."""
        groups = [group] if isinstance(group, int) else list(group)
        U = len(groups)
        m = self._gather(groups, env_idx, agent_perm)
        hidx = env_idx if hs_idx is None else hs_idx
        if U > 1 or groups[0]:
            hidx = torch.cat([hidx + gi * self.N for gi in groups])
        cl = self._classes(m) if self.class_tables else None
        acl = None if cl is None or not self.has_actor else cl["act"]
        gcl = None if cl is None else dict(rows=(self._cls["obs_enc"], self._cls["pos_enc"], self._cls["prev_dec"], self._cls["pos_dec"]),
                                           enc=cl["enc"], dec=cl["dec"])
        return m, hidx, U, gcl, acl

    def _minibatch_stats(self, m, U: int, adv_stats: Optional[torch.Tensor]) -> torch.Tensor:
        """The [mean, 1 / (std + eps)] pair the loss kernel normalises the advantages with (AdvStats)."""
        return self._adv(m, U, adv_stats, self.ws64, self._st())

    def apply_grads(self, grad_scale: float = 1.0):
        """optax clip_by_global_norm + adam + apply_updates on both flat buffers (rec_magpo.py:412-420): the two update functions."""
        self.sable_update_fn(grad_scale, self.ws64, self.gnorm[0:1])
        self.last_lr = self.actor_update_fn(grad_scale, self.ws64, self.gnorm[1:2])

    # ------------------------------------------------------------------ update (rec_magpo.py:214-487)
    def update(self, grad_sync: Optional[Callable[["MagpoLearner"], float]] = None) -> torch.Tensor:
        """ppo_epochs x num_minibatches optimisation steps; returns the loss table [P, M, n_loss] (device), already
        averaged over groups (and ranks when grad_sync all-reduces)."""
        s, N, A = self.sys, self.N, self.A
        M = s.num_minibatches
        mbs = N // M
        losses = torch.zeros(s.ppo_epochs, M, self.n_loss, device=self.dev)
        # Quirk B19 (rec_magpo.py:437,447,471): the reference shuffles prev_hstates by batch_perm and carries the SHUFFLED
        # arrays into the next epoch, so epoch e reads state row hs_idx_e[i] = hs_idx_{e-1}[batch_perm_e[i]] for
        # sequence i while the trajectory is gathered by batch_perm_e alone.  Only the index is composed; the 48 KiB
        # states never move.
        hs_idx = None
        mu = max(1, int(s.micro_batches))
        if mu > 1 and mbs % mu:
            raise ValueError(f"micro_batches={mu} must divide the minibatch of {mbs} envs")

        def grads(idx, group, hidx):
            """Gradients of one minibatch into grad_all: in one pass, or as the mean over ``micro_batches`` equal slabs."""
            if mu == 1:
                self.minibatch_grads(idx, agent_perm, group, hidx)
                return
            stats = self._minibatch_adv_stats(group, idx)
            step = mbs // mu
            self.grad_mu.zero_()
            for j in range(mu):
                self.minibatch_grads(idx[j * step:(j + 1) * step].contiguous(), agent_perm, group, hidx[j * step:(j + 1) * step].contiguous(),
                                     adv_stats=stats)
                self.grad_mu.add_(self.grad_all)
            self.grad_all.copy_(self.grad_mu).mul_(1.0 / mu)

        for e in range(s.ppo_epochs):
            # every group holds the same key => one permutation serves all groups
            ks = host_split(self.groups[0].key, 4)
            kb, ka, ke = ks[1], ks[2], ks[3]
            for g in self.groups:
                g.key = ks[0].copy()
            batch_perm = self._permutation(kb, N)
            agent_perm = self._permutation(ka, A)
            hs_idx = batch_perm if hs_idx is None else hs_idx[batch_perm.long()].contiguous()
            for mi in range(M):
                ke = host_split(ke, 2)[0]  # key, entropy_key = split(key): unused for discrete actions (:373)
                idx = batch_perm[mi * mbs:(mi + 1) * mbs].contiguous()
                hidx = hs_idx[mi * mbs:(mi + 1) * mbs].contiguous()
                self._optimise(lambda group: grads(idx, group, hidx), grad_sync, losses[e, mi])
        return losses
