"""Decentralised GRU actor (RecurrentActor, mava/networks/base.py:152-184) on the MI355X kernels.

pre-torso MLPTorso (default Dense(F->128)+ReLU) -> scanned GRU(128) with done-resets -> post-torso MLPTorso (default
Dense(128->128)+ReLU) -> Dense(D_post->K) logits (masked categorical head, heads.py:26-63).  The torsos follow
``network.actor_network.{pre,post}_torso`` (magpo_amd/torso.py): 1-3 layers of width 64-256, relu / tanh, optional
LayerNorm (magpo_ln_act_fwd / _bwd after the dense layer).  ``step`` pushes the carry during
the rollout (rec_magpo.py:146-159) and serves the evaluator; ``seq_fwd`` / ``seq_bwd`` are the
training forward and the hand-derived BPTT backward.
"""
from __future__ import annotations

from typing import Optional

import contextlib

import torch

from .netbase import TorsoNet
from .params import actor_layout, actor_named_views, init_actor, init_actor_from_key
from .torso import DEFAULT_TORSO, TorsoSpec, layer_name
from .tuning import Tuning

H = 128


class GruActor(TorsoNet):
    LINEAR_VARIANT = "actor_linear_variant"

    def __init__(self, n_agents: int, action_dim: int, obs_dim: int, device, *, hidden: int = 128, wgrad_groups: int = 512,
                 seed: Optional[int] = None, grads: Optional[torch.Tensor] = None, tuning: Optional[Tuning] = None, obs_ld: Optional[int] = None,
                 pre_torso: Optional[TorsoSpec] = None, post_torso: Optional[TorsoSpec] = None):
        if hidden != 128:
            raise NotImplementedError("gfx950 GRU kernels: hidden_state_dim = 128 only")
        if obs_dim > 128 or action_dim > 32:
            raise NotImplementedError("obs_dim <= 128 and action_dim <= 32 required")
        super().__init__(obs_dim, device, wgrad_groups, tuning, obs_ld)   # (wide observations: the pre-torso runs on the MFMA dense kernel)
        self.A, self.K = n_agents, action_dim
        self.pre_spec = pre_torso if pre_torso is not None else DEFAULT_TORSO
        self.post_spec = post_torso if post_torso is not None else DEFAULT_TORSO
        self.Dpre, self.Dpost = self.pre_spec.width, self.post_spec.width
        self._set_first_layer(self.pre_spec)
        self._bind_params(actor_layout(obs_dim, H, action_dim, self.pre_spec, self.post_spec), actor_named_views, grads)
        self._init_params(seed, init_actor_from_key, init_actor)   # (a key: rec_magpo.py:623)
        shapes = [(H, 3 * H), (self.Dpre, 3 * H), (self.Dpost, self.K)]   # every (KIN, NOUT) of a weight gradient
        for spec, din in ((self.pre_spec, self.KP), (self.post_spec, H)):
            for d in spec.layer_sizes:
                shapes.append((din, d))
                din = d
        self._size_wgrad_ws(shapes)
        self.refresh()

    def _twin_kw(self):
        return dict(wgrad_groups=self.G, tuning=self.tuning, obs_ld=self.Fld, pre_torso=self.pre_spec, post_torso=self.post_spec)

    def twin(self):
        """A second network of the same class, shape, row stride and torsos on the same device, sharing this one's ``Tuning`` object, with
        buffers of its own and uninitialised parameters (``load_named`` fills them): what an evaluator acts with, so that loading the
        evaluated parameters does not touch the learner's.  (A network built without ``tuning`` holds ``Tuning.from_env()`` of the same
        process environment, so sharing the object gives a system's evaluation network the values a fresh default would have.)"""
        return type(self)(self.A, self.K, self.F, self.dev, **self._twin_kw())

    def refresh(self):
        v = self.v
        self._tp("wi", v["gru.wi"]); self._tp("wh", v["gru.wh"])
        for prefix, spec in (("pre", self.pre_spec), ("post", self.post_spec)):
            for i in range(1 if prefix == "pre" else 0, len(spec.layer_sizes)):
                n = layer_name(prefix, i)
                self._tp(n, v[n + ".kernel"])
        self._refresh_first_and_head(self.pre_spec, self.Dpost)
        # W_i with its gate columns in the order of the backward scan's gradient matrix (n | r | z), see seq_bwd
        if "wi_nrz" not in self.wt:
            self.wt["wi_nrz"] = torch.empty(self.Dpre, 3 * H, device=self.dev)
        self._cols_nrz(v["gru.wi"], self.wt["wi_nrz"], self.Dpre, inverse=True)

    def _cols_nrz(self, src, dst, rows, inverse=False):
        """[rows, 3H] matrices, gate column blocks (n | r | z) -> (r | z | n) (inverse: the other way), on the current stream."""
        L, st = self.L, self._st()
        if inverse:
            L.call("magpo_copy_rows", src[:, 2 * H:], 3 * H, dst, 3 * H, rows, H, st)
            L.call("magpo_copy_rows", src, 3 * H, dst[:, H:], 3 * H, rows, 2 * H, st)
        else:
            L.call("magpo_copy_rows", src, 3 * H, dst[:, 2 * H:], 3 * H, rows, H, st)
            L.call("magpo_copy_rows", src[:, H:], 3 * H, dst, 3 * H, rows, 2 * H, st)

    def pre_torso(self, obs, obs_ld, R, ctx):
        """Pre-torso on R observation rows (stride obs_ld) -> its layer records; the output (GRU input) is recs[-1][3], [R, D_pre]."""
        return self._torso_fwd("pre", self.pre_spec, obs, obs_ld, R, ctx)

    def post_torso_logits(self, hs, R, ctx, logits):
        """Post-torso on the hidden states hs [R,128] and the logit head into logits [R,64] (K valid columns)."""
        recs = self._torso_fwd("post", self.post_spec, hs, H, R, ctx)
        self.lin(recs[-1][3], self.Dpost, self.wt["head"], self.v["head.bias"], logits, 64, R, self.Dpost, self.K)
        return recs

    def _wgrad_nrz(self, emb, dg, R, gw, dW, db):
        """dW_i, db_i from dg's columns 0..3H (gate blocks n | r | z) into W_i's order, on the weight-gradient stream."""
        D = self.Dpre
        side = self._wgrad_side()
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            st = self._st()
            self.L.call("magpo_wgrad", emb, D, dg, 4 * H, R, D, D, 3 * H, gw[:D], gw[D], self.wg_ws, self._groups(R), 1.0, 0, self.tuning.wgrad_variant, st)
            self._cols_nrz(gw[:D], dW, D)
            self._cols_nrz(gw[D:], db.view(1, 3 * H), 1)

    # one step for N envs: returns new hidden [N*A,128]; logits [N*A,64] if want_logits
    def step(self, obs, h_in, reset_env, h_out, want_logits: bool = False):
        """obs [N,A,F] f32, h_in / h_out [N*A,128], reset_env [N] u8 (reset-before-step flag per env)."""
        L, st, A, F, v, b = self.L, self._st(), self.A, self.F, self.v, self.b
        N = obs.shape[0]
        R = N * A
        xi = b.get("s_xi", (R, 3 * H))
        emb = self.pre_torso(obs, self.Fld, R, "s_")[-1][3]
        self.lin(emb, self.Dpre, self.wt["wi"], v["gru.bi"], xi, 3 * H, R, self.Dpre, 3 * H)
        L.call("magpo_gru_scan_fwd", xi, self.wt["wh"], v["gru.hn.bias"], h_in, None, reset_env, h_out, None, None, N, 1, A, None, 0, self.tuning.gru_block_rows, st)
        if not want_logits:
            return None
        logits = b.get("s_logits", (R, 64), zero=True)
        self.post_torso_logits(h_out, R, "s_", logits)
        return logits

    def carry(self, obs_tm, h_in, reset_tm, h_out, classes=None, tag=""):
        """Hidden-state carry over a whole rollout at once: obs_tm [T,N,A,F] (time-major trajectory), reset_tm [T,N] u8
        reset-before-step flags, h_in / h_out [N*A,128].  Same result as T calls of :meth:`step` (ScannedRNN, base.py:121-149):
        the carry depends on (obs, done) only, never on the sampled actions.  ``classes`` = (obs_tab [C,F], cls [T*N*A] i32):
        the input side on the distinct rows only (csrc/classtab.hip)."""
        L, st, A, F, v, b = self.L, self._st(), self.A, self.F, self.v, self.b
        T, N = obs_tm.shape[0], obs_tm.shape[1]
        R = T * N * A
        if classes is not None:
            _, xi_tab = self.input_table(classes[0], "r" + tag)
            L.call("magpo_gru_carry", xi_tab, self.wt["wh"], v["gru.hn.bias"], h_in, reset_tm, h_out, N, T, A, classes[1], self.tuning.gru_block_rows, st)
            return
        xi = b.get("c_xi", (R, 3 * H))
        emb = self.pre_torso(obs_tm, self.Fld, R, "c_")[-1][3]
        self.lin(emb, self.Dpre, self.wt["wi"], v["gru.bi"], xi, 3 * H, R, self.Dpre, 3 * H)
        L.call("magpo_gru_carry", xi, self.wt["wh"], v["gru.hn.bias"], h_in, reset_tm, h_out, N, T, A, None, self.tuning.gru_block_rows, st)

    def input_table(self, obs_tab: torch.Tensor, tag: str = ""):
        """xi of every distinct observation row: pre-torso + GRU input projection on obs_tab [C,F] -> [C,384] (the rows of a
        minibatch then take their xi by class index; see csrc/classtab.hip).  Returns (pre-torso layer records, xi table)."""
        v, b = self.v, self.b
        C = obs_tab.shape[0]
        xi_tab = b.get("c_xitab" + tag, (C, 3 * H))
        recs = self.pre_torso(obs_tab, self.F, C, "c_tab" + tag + "_")
        self.lin(recs[-1][3], self.Dpre, self.wt["wi"], v["gru.bi"], xi_tab, 3 * H, C, self.Dpre, 3 * H)
        return recs, xi_tab

    def seq_fwd(self, obs, dones, h0, h0_idx, nseq: int, T: int, classes=None):
        """obs [R,F] rows (seq, t, agent); dones [nseq,T] u8 resets; h0 [*,128] gathered through h0_idx [nseq*A].
        ``classes`` (optional) = (obs_tab [C,F], cls [R] i32, order [R] i64, offsets [C+1] i64): the rows' observations are
        obs_tab[cls]; the input side of the GRU is then evaluated on the C distinct rows only.
        Returns raw logits [R,64] (K valid columns)."""
        L, st, A, F, v, b = self.L, self._st(), self.A, self.F, self.v, self.b
        R = nseq * T * A
        hs = b.get("t_hs", (R, H))
        gates = b.get("t_gates", (R, 4 * H)); hprev = b.get("t_hprev", (R, H))
        logits = b.get("t_logits", (R, 64), zero=True)
        if classes is not None:   # the scan reads xi rows straight from the (L2-resident) class table
            pre, xi = self.input_table(classes[0])
            xi_cls = classes[1]
        else:
            xi = b.get("t_xi", (R, 3 * H))
            xi_cls = None
            pre = self.pre_torso(obs, self.Fld, R, "t_")
            self.lin(pre[-1][3], self.Dpre, self.wt["wi"], v["gru.bi"], xi, 3 * H, R, self.Dpre, 3 * H)
        L.call("magpo_gru_scan_fwd", xi, self.wt["wh"], v["gru.hn.bias"], h0, h0_idx, dones, hs, gates, hprev, nseq, T, A, xi_cls, self.tuning.gru_split_bf16, self.tuning.gru_block_rows, st)
        post = self.post_torso_logits(hs, R, "t_", logits)
        self._saved = dict(obs=obs, dones=dones, nseq=nseq, T=T, R=R, classes=classes, pre=pre, post=post)
        return logits

    def seq_bwd(self, dlogits):
        """dlogits [R,64] (columns >= K zero); fills self.grads."""
        L, st, A, F, K, v, gv, b = self.L, self._st(), self.A, self.F, self.K, self.v, self.gv, self.b
        sv = self._saved
        R, nseq, T, obs, dones = sv["R"], sv["nseq"], sv["T"], sv["obs"], sv["dones"]
        post, pre, Dq, Dp = sv["post"], sv["pre"], self.Dpost, self.Dpre
        dy = b.get("g_post_dy", (R, Dq))
        # dy = dlogits @ W_head^T, masked by the last post-torso layer's activation (fused epilogue: act 4 / 6 take it as the mask argument).
        # A ReLU layer without LayerNorm of width 64 / 128: head gradient and dy from one pass (dense_bwd; the layer's output is X and the mask)
        last = post[-1]
        if last[4] is None and self.post_spec.act(len(post) - 1) == 1:
            self.dense_bwd(last[3], Dq, dlogits, 64, v["head.kernel"], dy, Dq, R, Dq, K, gv["head.kernel"], gv["head.bias"], act=4, mask=last[3],
                           lin_W=self.wt["head_nat_pad"], lin_K=64)
        else:
            self.wgrad(last[3], Dq, dlogits, 64, R, Dq, K, gv["head.kernel"], gv["head.bias"])
            self._dx(dlogits, 64, self.wt["head_nat_pad"], 64, Dq, R, dy, self.post_spec, len(post) - 1, last)
        dz0 = self._torso_bwd("post", self.post_spec, post, dy)
        dhs = b.get("g_dhs", (R, H))
        self.lin(dz0, self.post_spec.layer_sizes[0], v["post.kernel"], None, dhs, H, R, self.post_spec.layer_sizes[0], H)
        # one gradient matrix for both projections (include/magpo.h): dg = (dn_in | dr | dz | dn_hid); the hidden side is its columns
        # H..4H in W_h's own gate order, the input side its columns 0..3H in the order (n | r | z)
        dg = b.get("g_dg", (R, 4 * H))
        nblk = (nseq * A + 63) // 64
        slab = b.get("g_slab", (nblk, H))
        L.call("magpo_gru_scan_bwd", b.t["t_gates"], b.t["t_hprev"], dones, dhs, v["gru.wh"], dg, slab, nseq, T, A, self.tuning.gru_split_bf16, self.tuning.gru_block_rows, st)
        self.reduce(slab, gv["gru.hn.bias"])
        self.wgrad(b.t["t_hprev"], H, dg[:, H:], 4 * H, R, H, 3 * H, gv["gru.wh"])
        if sv["classes"] is not None:
            # input side on the class table: S[c] = sum of the rows of class c, gate blocks back into W_i's order on the C rows, then the
            # layers' backward on C rows
            obs, _, order, offsets = sv["classes"]
            C = obs.shape[0]
            part = b.get("g_cpart", (L.call("magpo_class_sum_slots", C), C, 3 * H))
            s_nrz = b.get("g_dxic_nrz", (C, 3 * H)); dxi = b.get("g_dxic", (C, 3 * H))
            L.call("magpo_class_sum", dg, 4 * H, order, offsets, C, 3 * H, part, s_nrz, st)
            self._cols_nrz(s_nrz, dxi, C)
            emb, R = pre[-1][3], C
            self.wgrad(emb, Dp, dxi, 3 * H, R, Dp, 3 * H, gv["gru.wi"], gv["gru.bi"])
            ldx, wi_t = 3 * H, v["gru.wi"]
        else:
            # per token row: weight gradient with its gate blocks in dg's order, put back into W_i's order on the [D_pre, 3H] result; the dX
            # GEMM contracts over the gates in dg's order against the equally permuted copy of W_i
            emb = pre[-1][3]
            gw = b.get("g_gwi_nrz", (Dp + 1, 3 * H))
            self._wgrad_nrz(emb, dg, R, gw, gv["gru.wi"], gv["gru.bi"])
            dxi, ldx, wi_t = dg, 4 * H, self.wt["wi_nrz"]
        demb = b.get("g_demb", (R, Dp))
        # dX of the GRU input projection, masked by the last pre-torso layer's activation (the small first layer applies its ReLU mask itself)
        if len(pre) == 1 and self.small_first:
            self.lin(dxi, ldx, wi_t, None, demb, Dp, R, 3 * H, Dp)
        else:
            self._dx(dxi, ldx, wi_t, 3 * H, Dp, R, demb, self.pre_spec, len(pre) - 1, pre[-1])
        d0 = self._torso_bwd("pre", self.pre_spec, pre, demb)
        if self.small_first:   # Dense(F->128)+ReLU weight gradient on the raw observation rows
            self._small_first_wgrad(obs, pre[0][3], d0, R)
        self._join_wgrad()


GruActor.apply = GruActor.seq_fwd   # actor_network.apply (rec_magpo.py:631): the scanned training forward (its backward: seq_bwd)
