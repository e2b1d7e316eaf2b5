"""Multi-Agent Transformer on the MI355X kernels: autoregressive acting and the teacher-forced training forward / backward.

Host-side composition of the C-ABI kernels (include/magpo.h); mirrors ``MultiAgentTransformer.get_actions``
(mava/networks/mat_network.py:266-279 with discrete_autoregressive_act, networks/utils/mat/decode.py:90-124) and
``MultiAgentTransformer.__call__`` (:247-264 with discrete_parallel_act, decode.py:33-58).  The backward pass is hand-derived (no
autograd): it walks the forward graph in reverse, one kernel per node.

A time step's A agents are one team of A consecutive token rows.  Every attention is magpo_team_attention_* (csrc/team_attention.hip):
softmax over the agents of a team per head; the forward keeps one log-sum-exp per row and head, the backward recomputes the weights from
it.  Every LayerNorm is magpo_resln_* (residual + flax LayerNorm; act 2: LayerNorm(gelu(.)) for the heads and the embeddings; nf = F: the
observation encoder's LayerNorm over the F raw features inside a zero-padded row).  Dense layers, GELU inside the MLP (magpo_linear act 2),
sampling and the loss are the kernels every other network uses.

Acting is the encoder once and A decoder iterations; iteration i computes row i only, from the k | v rows j <= i of every block that the
earlier iterations left in place (ntok = i + 1, ret_from = i).  Both decoder attentions are causal, so row j of a block's input never
depends on a later agent and the cached rows are exactly what the whole-sequence decoder of decode.py:104 recomputes every iteration.

Supported (anything else raises NotImplementedError naming the key): embed_dim 64, n_head 1 / 2 / 4, any n_block, at most 32 agents,
discrete actions with action_dim <= 31, obs_dim <= 128, LayerNorm (use_rmsnorm false) and the Dense-GELU-Dense MLP (use_swiglu false).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .netbase import NetBase
from .params import init_mat, init_mat_from_key, mat_layout, mat_named_views
from .tuning import Tuning

E = 64      # embed_dim: the row width of every activation
LW = 64     # logit rows (K <= 31 valid columns)


def check_net_config(embed_dim: int = 64, n_head: int = 1, n_block: int = 1, use_rmsnorm: bool = False, use_swiglu: bool = False) -> None:
    """The network settings of configs/network/transformer.yaml that the kernels evaluate."""
    if use_rmsnorm:
        raise NotImplementedError("network.use_rmsnorm=true: the MAT kernels evaluate flax LayerNorm only")
    if use_swiglu:
        raise NotImplementedError("network.use_swiglu=true: the MAT kernels evaluate the Dense-GELU-Dense MLP only")
    if int(embed_dim) != 64:
        raise NotImplementedError(f"network.embed_dim={embed_dim}: the MAT kernels are built for embed_dim 64")
    if int(n_head) not in (1, 2, 4):
        raise NotImplementedError(f"network.n_head={n_head}: heads of 16, 32 or 64 channels only (n_head 1, 2 or 4)")
    if int(n_block) < 1:
        raise NotImplementedError(f"network.n_block={n_block}: at least one block")


class MatNetwork(NetBase):
    ff = True   # memoryless: nothing is carried between env steps (what FfSableLearner asks of its network)

    def __init__(self, n_agents: int, action_dim: int, obs_dim: int, device, *, embed_dim: int = 64, n_head: int = 1, n_block: int = 1,
                 use_rmsnorm: bool = False, use_swiglu: bool = False, wgrad_groups: int = 512, seed=None, grads: Optional[torch.Tensor] = None,
                 tuning: Optional[Tuning] = None, obs_ld: Optional[int] = None):
        check_net_config(embed_dim, n_head, n_block, use_rmsnorm, use_swiglu)
        if n_agents < 1 or n_agents > 32:
            raise NotImplementedError(f"num_agents={n_agents}: a team is at most the 32 rows of one attention tile")
        if obs_dim > 128 or action_dim > 31:
            raise NotImplementedError("obs_dim <= 128 and action_dim <= 31 required")
        self.nb, self.nh, self.EL, self.E = int(n_block), int(n_head), E, E
        self.hs = E // self.nh
        super().__init__(obs_dim, device, wgrad_groups, tuning, obs_ld)
        self.A, self.K = n_agents, action_dim
        self.KP = 128 if self.wide else 64   # the observation rows as a zero-padded operand of the first Dense layer
        self._bind_params(mat_layout(E, obs_dim, action_dim, self.nb), lambda views: mat_named_views(views, E), grads)
        self._init_params(seed, init_mat_from_key, init_mat)
        self.wg_ws = torch.empty(max(self.L.call("magpo_wgrad_workspace_floats", k, n, self.G) for k, n in
                                     ((E, 3 * E), (E, 2 * E), (E, E), (self.KP, E))), device=device)
        self.refresh()

    def twin(self):
        """A second network of the same shape and row stride on the same device, sharing this one's ``Tuning`` object, with buffers of its
        own and uninitialised parameters."""
        return type(self)(self.A, self.K, self.F, self.dev, n_head=self.nh, n_block=self.nb, wgrad_groups=self.G, tuning=self.tuning, obs_ld=self.Fld)

    # ------------------------------------------------------------------ derived weight copies
    def _blocks(self):
        """(name prefix of the block's parameters, key prefix of its derived copies and buffers, attention names) of every block."""
        out = [(f"encoder.blocks.layers_{b}.", f"e{b}", ("attn",)) for b in range(self.nb)]
        return out + [(f"decoder.cross_attention_block_{b}.", f"d{b}", ("attn1", "attn2")) for b in range(self.nb)]

    def refresh(self):
        """Rebuild the transposed (forward-GEMM) weight copies after a parameter update, in place on the calling stream."""
        v, F, KP = self.v, self.F, self.KP
        for name, shape in (("wobs", (E, KP)), ("wobs_nat_pad", (KP, E)), ("ln0.scale", (KP,)), ("ln0.bias", (KP,))):
            if name not in self.wt:
                self.wt[name] = torch.zeros(*shape, device=self.dev)
        self.wt["wobs"][:, :F].copy_(v["encoder.obs_encoder.layers_1.kernel"].t())
        self.wt["wobs_nat_pad"][:F].copy_(v["encoder.obs_encoder.layers_1.kernel"])
        self.wt["ln0.scale"][:F].copy_(v["encoder.obs_encoder.layers_0.scale"])
        self.wt["ln0.bias"][:F].copy_(v["encoder.obs_encoder.layers_0.bias"])
        for p, key, attns in self._blocks():
            for a in attns:
                if a == "attn2":
                    self._tp(f"{key}.{a}.q", v[p + "attn2.query.kernel"])
                    self._tp(f"{key}.{a}.kv", v[p + "attn2.w_kv"])
                else:
                    self._tp(f"{key}.{a}.qkv", v[p + f"{a}.w_qkv"])
                self._tp(f"{key}.{a}.proj", v[p + f"{a}.proj.kernel"])
            self._tp(f"{key}.mlp0", v[p + "mlp.layers_0.kernel"])
            self._tp(f"{key}.mlp2", v[p + "mlp.layers_2.kernel"])
        for side in ("encoder", "decoder"):
            self._tp(f"{side}.h0", v[side + ".head.layers_0.kernel"])
            h1t = self._tp(f"{side}.h1", v[side + ".head.layers_3.kernel"], LW)   # [64 (columns padded)][E]
            self._tp(f"{side}.h1_nat_pad", h1t, E)                                   # [E][64]: natural W padded to 64 columns

    # ------------------------------------------------------------------ pieces shared by acting and training
    def _resln(self, a, lda, y, ldy, name, out, ldout, R, act=0):
        v = self.v
        self.L.call("magpo_resln_fwd", a, lda, y, ldy, v[name + ".scale"], v[name + ".bias"], out, ldout, R, E, E, act, self._st())

    def _attn(self, q, ldq, k, ldk, vv, ldv, y, lse, nteams, ntok, ret_from, masked):
        self.L.call("magpo_team_attention_fwd", q, ldq, k, ldk, vv, ldv, y, E, lse, nteams, self.A, ntok, ret_from, masked, self.hs, self.nh, self._st())

    def _mlp_ln(self, p, key, x, ldx, ln, out, R, g):
        """out = LayerNorm(x + Dense(gelu(Dense(x)))) (mat_network.py:39-45, 66, 137); keeps h and the MLP output for the backward."""
        v = self.v
        h, m = g(key + ".h"), g(key + ".m")
        self.lin(x, ldx, self.wt[key + ".mlp0"], v[p + "mlp.layers_0.bias"], h, E, R, E, E, act=2)
        self.lin(h, E, self.wt[key + ".mlp2"], v[p + "mlp.layers_2.bias"], m, E, R, E, E)
        self._resln(x, ldx, m, E, p + ln, out, E, R)

    def _head(self, side, x, ldx, out, ldout, nout, R, g):
        """Dense -> gelu -> LayerNorm -> Dense(nout) (mat_network.py:95-102, 186-193)."""
        v = self.v
        hp, hn = g(side + ".hp"), g(side + ".hn")
        self.lin(x, ldx, self.wt[side + ".h0"], v[side + ".head.layers_0.bias"], hp, E, R, E, E)
        self._resln(None, 0, hp, E, side + ".head.layers_2", hn, E, R, act=2)
        self.lin(hn, E, self.wt[side + ".h1"], v[side + ".head.layers_3.bias"], out, ldout, R, E, nout)

    def _encoder(self, obs, value_out, R, g):
        """Encoder.__call__ (mat_network.py:104-111) on R = teams x A rows: writes the values, returns the representation."""
        L, st, v, KP, A = self.L, self._st(), self.v, self.KP, self.A
        if self.wide:
            xp = obs   # rows already 128 floats apart
        else:
            xp = g("xp", KP)
            L.call("magpo_small_operand", 2, obs, self.Fld, self.F, None, None, 0, xp, R, st)
        on, z0 = g("on", KP), g("z0")
        L.call("magpo_resln_fwd", None, 0, xp, KP, self.wt["ln0.scale"], self.wt["ln0.bias"], on, KP, R, KP, self.F, 0, st)
        self.lin(on, KP, self.wt["wobs"], v["encoder.obs_encoder.layers_1.bias"], z0, E, R, KP, E)
        x = g("e.x0")
        self._resln(None, 0, z0, E, "encoder.ln", x, E, R, act=2)
        for b in range(self.nb):
            p, key = f"encoder.blocks.layers_{b}.", f"e{b}"
            qkv, att, pr, x1, x2 = g(key + ".qkv", 3 * E), g(key + ".att"), g(key + ".pr"), g(key + ".x1"), g(f"e.x{b + 1}")
            self.lin(x, E, self.wt[key + ".attn.qkv"], v[p + "attn.b_qkv"], qkv, 3 * E, R, E, 3 * E)
            self._attn(qkv, 3 * E, qkv[:, E:], 3 * E, qkv[:, 2 * E:], 3 * E, att, g(key + ".lse", self.nh), R // A, A, 0, 0)
            self.lin(att, E, self.wt[key + ".attn.proj"], v[p + "attn.proj.bias"], pr, E, R, E, E)
            self._resln(x, E, pr, E, p + "ln1", x1, E, R)
            self._mlp_ln(p, key, x1, E, "ln2", x2, R, g)
            x = x2
        self._head("encoder", x, E, value_out, 1, 1, R, g)
        return x

    def _decoder_block(self, b, x, ldx, rep, ldrep, q2, row, step, R, nteams, ntok, ret_from, g, gk):
        """DecodeBlock.__call__ (mat_network.py:134-138) on R rows x (stride ldx) -> the block's output [R, E].  The q | k | v rows and the
        attention outputs live in the buffers ``gk`` of nteams x A rows: this call's R rows are the rows ``row``, ``row + step``, ... of
        them (acting: agent ``row`` of every team, step = A; training: every row, step = 1), and the attentions produce rows
        ret_from <= i < ntok of every team."""
        v = self.v
        p, key = f"decoder.cross_attention_block_{b}.", f"d{b}"
        qkv1, kv2, a1, a2 = gk(key + ".qkv1", 3 * E), gk(key + ".kv2", 2 * E), gk(key + ".a1"), gk(key + ".a2")
        lse1, lse2 = gk(key + ".lse1", self.nh), gk(key + ".lse2", self.nh)
        p1, x1, p2, x2, x3 = g(key + ".p1"), g(key + ".x1"), g(key + ".p2"), g(key + ".x2"), g(f"d.x{b + 1}")
        self.lin(x, ldx, self.wt[key + ".attn1.qkv"], v[p + "attn1.b_qkv"], qkv1[row:], step * 3 * E, R, E, 3 * E)
        self._attn(qkv1, 3 * E, qkv1[:, E:], 3 * E, qkv1[:, 2 * E:], 3 * E, a1, lse1, nteams, ntok, ret_from, 1)
        self.lin(a1[row:], step * E, self.wt[key + ".attn1.proj"], v[p + "attn1.proj.bias"], p1, E, R, E, E)
        self._resln(x, ldx, p1, E, p + "ln1", x1, E, R)
        self.lin(x1, E, self.wt[key + ".attn2.kv"], v[p + "attn2.b_kv"], kv2[row:], step * 2 * E, R, E, 2 * E)
        self._attn(q2, E, kv2, 2 * E, kv2[:, E:], 2 * E, a2, lse2, nteams, ntok, ret_from, 1)
        self.lin(a2[row:], step * E, self.wt[key + ".attn2.proj"], v[p + "attn2.proj.bias"], p2, E, R, E, E)
        self._resln(rep, ldrep, p2, E, p + "ln2", x2, E, R)
        self._mlp_ln(p, key, x2, E, "ln3", x3, R, g)
        return x3

    def _cross_queries(self, rep, R, g):
        """The cross-attention queries of every decoder block, for all rows at once (query = the encoder representation)."""
        out = []
        for b in range(self.nb):
            p, key = f"decoder.cross_attention_block_{b}.", f"d{b}"
            q2 = g(key + ".q2")
            self.lin(rep, E, self.wt[key + ".attn2.q"], self.v[p + "attn2.query.bias"], q2, E, R, E, E)
            out.append(q2)
        return out

    # ------------------------------------------------------------------ acting
    def _sample_keys_arg(self, sample_keys, value_only=False):
        """``sample_keys`` [A, 2] uint32 as (host array or None, device table or None): see SableGuider._sample_keys_arg."""
        if torch.is_tensor(sample_keys):
            return None, sample_keys
        if value_only:
            return None, None
        return np.ascontiguousarray(np.asarray(sample_keys, dtype=np.uint32).reshape(self.A, 2)), None

    def act(self, obs, pos, states, sample_keys, action_out, logp_out, value_out, mask=None, value_only=False):
        """One env step for N envs (MultiAgentTransformer.get_actions): obs [N, A, Fld] f32; ``pos`` (step counts) and ``states`` are not
        read (no positional encoding, no memory); sample_keys = [A, 2] uint32 (host array: keys by value; device tensor: static arguments
        for graph replay).  Writes action [N, A] i32, logp [N, A], value [N, A]."""
        L, st, A, K, v = self.L, self._st(), self.A, self.K, self.v
        N = obs.shape[0]
        R = N * A
        g = lambda n, w=E: self.b.get("a_" + n, (R, w))
        rep = self._encoder(obs, value_out, R, g)
        if value_only:
            return
        gn = lambda n, w=E: self.b.get("ai_" + n, (N, w))
        q2 = self._cross_queries(rep, R, g)
        prev = self.b.get("a_prev", (A, N), torch.int32, zero=True)   # agent-major: row i = the table rows agent i embeds (0: start token)
        za, logits = gn("za"), self.b.get("ai_logits", (N, LW), zero=True)
        keys, kdev = self._sample_keys_arg(sample_keys)
        for i in range(A):
            L.call("magpo_gather_rows", v["decoder.action_encoder.layers_0.kernel"], E, prev[i], za, E, N, E, st)
            x = gn("d.x0")
            self._resln(None, 0, za, E, "decoder.ln", x, E, N, act=2)
            for b in range(self.nb):
                x = self._decoder_block(b, x, E, rep[i:], A * E, q2[b], i, A, N, N, i + 1, i, gn, g)
            self._head("decoder", x, E, logits, LW, K, N, gn)
            k0, k1 = (0, 0) if keys is None else (int(keys[i][0]), int(keys[i][1]))
            L.call("magpo_sample_categorical", logits, LW, None if mask is None else mask[:, i], (A * K if mask is not None else 0),
                   k0, k1, None if kdev is None else kdev[i], action_out[:, i:], A, logp_out[:, i:], A, prev[i + 1] if i + 1 < A else None, 1, None, 0, N, K, st)

    get_actions = act   # partial(actor_network.apply, method="get_actions") (mat.py:357-360)

    # ------------------------------------------------------------------ training forward
    def apply(self, obs, prev_idx, pos, dones, s0, seq_env, nseq: int, T: int = 1):
        """The teacher-forced parallel pass on nseq x A rows (MultiAgentTransformer.__call__): obs [R, Fld], prev_idx [R] (0 = start token,
        action + 1 otherwise: the row of the K + 1 one-hot); pos, dones, s0, seq_env are not read.  Returns (logits [R, 64] raw with K valid
        columns, value [R])."""
        if T != 1:
            raise ValueError("MAT trains on single time steps (T = 1)")
        L, st, v, A = self.L, self._st(), self.v, self.A
        R = nseq * A
        g = lambda n, w=E: self.b.get("t_" + n, (R, w))
        self._saved = dict(obs=obs, prev_idx=prev_idx, R=R, nseq=nseq)
        value = self.b.get("t_value", (R,))
        logits = self.b.get("t_logits", (R, LW), zero=True)
        rep = self._encoder(obs, value, R, g)
        q2 = self._cross_queries(rep, R, g)
        za, x = g("za"), g("d.x0")
        L.call("magpo_gather_rows", v["decoder.action_encoder.layers_0.kernel"], E, prev_idx, za, E, R, E, st)
        self._resln(None, 0, za, E, "decoder.ln", x, E, R, act=2)
        for b in range(self.nb):
            x = self._decoder_block(b, x, E, rep, E, q2[b], 0, 1, R, nseq, A, 0, g, g)
        self._head("decoder", x, E, logits, LW, self.K, R, g)
        return logits, value

    train_fwd = apply

    # ------------------------------------------------------------------ training backward
    def _slabs(self, R, W=E):
        """The per-workgroup slabs of a LayerNorm's scale and bias gradients over R rows of W floats."""
        grid = self.L.call("magpo_row_grid", R)
        return self.b.get(f"s_scale{W}", (grid, W)), self.b.get(f"s_bias{W}", (grid, W))

    def _resln_bwd(self, a, y, name, d0, d1, dsum, R, act=0):
        """Backward of :meth:`_resln` on [R, E] rows: dsum = d(a + y) (act 2: dy) of d0 [+ d1]; fills the LayerNorm's scale / bias gradients."""
        sa, sb = self._slabs(R)
        self.L.call("magpo_resln_bwd", a, 0 if a is None else E, y, E, self.v[name + ".scale"], d0, E, d1, 0 if d1 is None else E, dsum, E,
                    sa, sb, R, E, E, act, self._st())
        self.reduce(sa, self.gv[name + ".scale"])
        self.reduce(sb, self.gv[name + ".bias"])

    def _dense_bwd(self, X, dY, name, dX, R):
        """Backward of an E -> E Dense layer ``name`` (.kernel, .bias)."""
        self.dense_bwd(X, E, dY, E, self.v[name + ".kernel"], dX, E, R, E, E, self.gv[name + ".kernel"], self.gv[name + ".bias"])

    def _mlp_ln_bwd(self, p, key, x, ln, d0, d1, R, t, g):
        """Backward of :meth:`_mlp_ln`: returns (dA, dB) with d(x) = dA + dB."""
        v = self.v
        dsum, dh, z, dxm = g(key + ".dsum_m"), g("dh"), g("z"), g(key + ".dxm")
        self._resln_bwd(x, t(key + ".m"), p + ln, d0, d1, dsum, R)
        self._dense_bwd(t(key + ".h"), dsum, p + "mlp.layers_2", dh, R)
        self.lin(x, E, self.wt[key + ".mlp0"], v[p + "mlp.layers_0.bias"], z, E, R, E, E)   # the pre-activation again: gelu'(z)
        self.L.call("magpo_gelu_bwd", z, E, dh, E, dh, E, R, E, self._st())
        self._dense_bwd(x, dh, p + "mlp.layers_0", dxm, R)
        return dsum, dxm

    def _fused_proj_bwd(self, X, dY, wname, bname, width, dX, R):
        """Backward of a fused projection [E, width] (width 2E / 3E): weight and bias gradient, dX = dY W^T."""
        self.wgrad(X, E, dY, width, R, E, width, self.gv[wname], self.gv[bname])
        self.lin(dY, width, self.v[wname], None, dX, E, R, width, E)

    def _head_bwd(self, side, x, dout, ldd, nout, dx, R, t, g):
        """Backward of :meth:`_head`: dout [R, ldd] with ``nout`` valid columns -> dx [R, E]."""
        v, gv = self.v, self.gv
        dhn, dhp = g("dhn"), g("dhp")
        self.dense_bwd(t(side + ".hn"), E, dout, ldd, v[side + ".head.layers_3.kernel"], dhn, E, R, E, nout, gv[side + ".head.layers_3.kernel"],
                       gv[side + ".head.layers_3.bias"], lin_W=self.wt[side + ".h1_nat_pad"], lin_K=LW)
        self._resln_bwd(None, t(side + ".hp"), side + ".head.layers_2", dhn, None, dhp, R, act=2)
        self._dense_bwd(x, dhp, side + ".head.layers_0", dx, R)

    def _attn_bwd(self, q, ldq, k, ldk, vv, ldv, lse, dy, dq, lddq, dk, lddk, dv, lddv, nteams, masked):
        self.L.call("magpo_team_attention_bwd", q, ldq, k, ldk, vv, ldv, lse, dy, E, dq, lddq, dk, lddk, dv, lddv, nteams, self.A, masked,
                    self.hs, self.nh, self._st())

    def train_bwd(self, dlogits, dvalue):
        """dlogits [R, 64] (columns >= K zero), dvalue [R]; fills self.grads (every entry written exactly once)."""
        L, st, v, gv, b, nb, KP, F = self.L, self._st(), self.v, self.gv, self.b, self.nb, self.KP, self.F
        sv = self._saved
        R, nseq = sv["R"], sv["nseq"]
        t = lambda n: b.t["t_" + n]
        g = lambda n, w=E: b.get("g_" + n, (R, w))
        # ---- logit head
        dx = g("dx_head")
        self._head_bwd("decoder", t(f"d.x{nb}"), dlogits, LW, self.K, dx, R, t, g)
        # ---- decoder blocks, last to first; the gradient of a block's output is d0 [+ d1]
        d0, d1 = dx, None
        drep = None   # running sum of d(rep) over the blocks: cross-attention query path + residual path
        for k in reversed(range(nb)):
            p, key = f"decoder.cross_attention_block_{k}.", f"d{k}"
            x_in = t(f"d.x{k}")
            dsum3, dxm = self._mlp_ln_bwd(p, key, t(key + ".x2"), "ln3", d0, d1, R, t, g)
            dsum2 = g(key + ".dsum2")
            self._resln_bwd(t("e.x%d" % nb), t(key + ".p2"), p + "ln2", dsum3, dxm, dsum2, R)
            da, dq2, dkv2, dx1 = g("da"), g("dq2"), g("dkv2", 2 * E), g("dx1")
            self._dense_bwd(t(key + ".a2"), dsum2, p + "attn2.proj", da, R)
            kv2 = t(key + ".kv2")
            self._attn_bwd(t(key + ".q2"), E, kv2, 2 * E, kv2[:, E:], 2 * E, t(key + ".lse2"), da, dq2, E, dkv2, 2 * E, dkv2[:, E:], 2 * E, nseq, 1)
            drq = g(key + ".drq")
            self._dense_bwd(t("e.x%d" % nb), dq2, p + "attn2.query", drq, R)
            self._fused_proj_bwd(t(key + ".x1"), dkv2, p + "attn2.w_kv", p + "attn2.b_kv", 2 * E, dx1, R)
            if drep is None:
                drep = g("drep")
                L.call("magpo_copy_rows", dsum2, E, drep, E, R, E, st)
            else:
                self.add_(drep, dsum2)
            self.add_(drep, drq)
            dsum1, dqkv1, dxq = g(key + ".dsum1"), g("dqkv", 3 * E), g(key + ".dxq")
            self._resln_bwd(x_in, t(key + ".p1"), p + "ln1", dx1, None, dsum1, R)
            self._dense_bwd(t(key + ".a1"), dsum1, p + "attn1.proj", da, R)
            qkv1 = t(key + ".qkv1")
            self._attn_bwd(qkv1, 3 * E, qkv1[:, E:], 3 * E, qkv1[:, 2 * E:], 3 * E, t(key + ".lse1"), da, dqkv1, 3 * E, dqkv1[:, E:], 3 * E,
                           dqkv1[:, 2 * E:], 3 * E, nseq, 1)
            self._fused_proj_bwd(x_in, dqkv1, p + "attn1.w_qkv", p + "attn1.b_qkv", 3 * E, dxq, R)
            d0, d1 = dsum1, dxq
        # ---- action embedding: x0 = LayerNorm(gelu(W_act[prev])); the table's gradient is one-hot^T dza
        dza, oh = g("dza"), g("onehot")
        self._resln_bwd(None, t("za"), "decoder.ln", d0, d1, dza, R, act=2)
        L.call("magpo_small_operand", 1, None, 0, 0, None, sv["prev_idx"], 1, oh, R, st)
        self.wgrad(oh, E, dza, E, R, E, E, gv["decoder.action_encoder.layers_0.kernel"], None, krows=self.K + 1)
        # ---- value head
        dl = b.get("g_dvalue_rows", (R, LW), zero=True)   # columns 1.. stay zero
        L.call("magpo_copy_rows", dvalue, 1, dl, LW, R, 1, st)
        drep_v = g("drep_v")
        self._head_bwd("encoder", t(f"e.x{nb}"), dl, LW, 1, drep_v, R, t, g)
        # ---- encoder blocks, last to first; d(rep) = value head + the decoder blocks' sums
        d0, d1 = drep_v, drep
        for k in reversed(range(nb)):
            p, key = f"encoder.blocks.layers_{k}.", f"e{k}"
            x_in = t(f"e.x{k}")
            dsumB, dxm = self._mlp_ln_bwd(p, key, t(key + ".x1"), "ln2", d0, d1, R, t, g)
            dsumA, da, dqkv, dxq = g(key + ".dsumA"), g("da"), g("dqkv", 3 * E), g(key + ".dxq")
            self._resln_bwd(x_in, t(key + ".pr"), p + "ln1", dsumB, dxm, dsumA, R)
            self._dense_bwd(t(key + ".att"), dsumA, p + "attn.proj", da, R)
            qkv = t(key + ".qkv")
            self._attn_bwd(qkv, 3 * E, qkv[:, E:], 3 * E, qkv[:, 2 * E:], 3 * E, t(key + ".lse"), da, dqkv, 3 * E, dqkv[:, E:], 3 * E,
                           dqkv[:, 2 * E:], 3 * E, nseq, 0)
            self._fused_proj_bwd(x_in, dqkv, p + "attn.w_qkv", p + "attn.b_qkv", 3 * E, dxq, R)
            d0, d1 = dsumA, dxq
        # ---- observation encoder: x0 = LayerNorm(gelu(z0)), z0 = LayerNorm_F(obs) W + b
        dz0, don, dxp = g("dz0"), g("don", KP), g("dxp", KP)
        self._resln_bwd(None, t("z0"), "encoder.ln", d0, d1, dz0, R, act=2)
        self.wgrad(t("on"), KP, dz0, E, R, KP, E, gv["encoder.obs_encoder.layers_1.kernel"], gv["encoder.obs_encoder.layers_1.bias"], krows=F)
        self.lin(dz0, E, self.wt["wobs_nat_pad"], None, don, KP, R, E, KP)
        xp = sv["obs"] if self.wide else t("xp")
        sa, sb = self._slabs(R, KP)
        L.call("magpo_resln_bwd", None, 0, xp, KP, self.wt["ln0.scale"], don, KP, None, 0, dxp, KP, sa, sb, R, KP, F, 0, st)
        self.reduce(sa, gv["encoder.obs_encoder.layers_0.scale"], P=F, stride=KP)
        self.reduce(sb, gv["encoder.obs_encoder.layers_0.bias"], P=F, stride=KP)
        self._join_wgrad()

    def add_(self, dst, src):
        self.L.call("magpo_add_inplace", dst, src, dst.numel(), self._st())

    def _wgrad_side(self):
        return None   # every weight gradient on the calling stream: the d(rep) sums are accumulated in place
