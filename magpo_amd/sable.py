"""Sable guider on the MI355X kernels: recurrent acting and chunkwise training forward/backward.

Host-side composition of the C-ABI kernels (include/magpo.h); mirrors ``SableNetwork.get_actions``
(mava/networks/sable_network.py:443-482) and ``SableNetwork.__call__`` (:412-441).  The backward pass
is hand-derived (no autograd): it walks the forward graph in reverse, one kernel per node.

Supported configuration (asserted): embed_dim 16 / 32 / 64 / 128, n_head 1 / 2 / 4, any n_block, discrete actions, one chunk
per rollout, SwiGLU weights at their zero init (then the FFN branch and its gradients are exactly 0,
SURVEY B5 -- verified on the host at construction / load time).

Widths.  ``EL`` = the reference's embed_dim; ``E`` = width of the device network: 64 (EL <= 64: narrower nets run embedded, see
params.WidthEmbedding) or 128.  The fused kernels (csrc/seg_fused.hip, csrc/act_fused.hip, first-layer class tables read in place)
exist for E = 64; an E = 128 network is composed kernel by kernel: dense layers on k_linear_lds<128 | 256 | 384,*>, row kernels at 32
lanes per row (csrc/rowops.hip), retention on the 64-wide tile kernels -- n_head 2 / 4 have 64- / 32-wide heads (real tiles); the
one 128-wide head of n_head = 1 is evaluated blockwise, r[:, J] = sum_I ret(q[:, I], k[:, I], v[:, J]) over the 64-column halves
I, J with the 128 x 128 state kept as four 64 x 64 tiles S[I][J] (exact: retention is bilinear in (q.k) and v).
"""
from __future__ import annotations

import math
from functools import partial
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .netbase import NetBase, _Bufs  # noqa: F401  (_Bufs stays importable from this module)
from .params import FlatParams, WidthEmbedding, guider_layout, guider_named_views, init_guider, init_guider_from_key
from .tuning import Tuning

E = 64      # width of the fused (64-wide) kernel family, of a retention state tile and of a logit row
TILE = 64   # retention states live in 64 x 64 tiles on the device
LW = 64     # logit rows (K <= 31 valid columns)


def decay_kappas(n_head: int, scaling: float):
    """sable_network.py:366-369 / retention.py:231-234 in float32: one kappa per head."""
    k = 1.0 - np.exp(np.linspace(np.log(np.float32(1 / 32)), np.log(np.float32(1 / 512)), n_head, dtype=np.float32))
    return [float(x) for x in (k.astype(np.float32) * np.float32(scaling)).astype(np.float32)]


class SableGuider(NetBase):
    def __init__(self, n_agents: int, action_dim: int, obs_dim: int, device, *, embed_dim: int = 64, n_head: int = 1,
                 n_block: int = 1, decay_scaling_factor: float = 0.8, use_pe: bool = True, max_pos: int = 101,
                 wgrad_groups: int = 512, seed: Optional[int] = None, grads: Optional[torch.Tensor] = None,
                 tuning: Optional[Tuning] = None, obs_ld: Optional[int] = None, memory_type: str = "rec_sable"):
        if memory_type not in ("rec_sable", "ff_sable"):
            raise NotImplementedError(f"memory_type must be rec_sable or ff_sable, got {memory_type!r}")
        # ff_sable (mava/systems/sable/anakin/ff_sable.py): retention over the agents of ONE time step on zero hidden states -- no decay
        # (:341), no timestep positional encoding (:350; an all-zero pe table makes the existing kernels add exactly 0), no state buffers:
        # every retention op is a team kernel (csrc/team_retention.hip)
        self.memory_type, self.ff = memory_type, memory_type == "ff_sable"
        if self.ff:
            decay_scaling_factor, use_pe = 1.0, False
        self.decay_scaling_factor, self.use_pe = float(decay_scaling_factor), bool(use_pe)
        if embed_dim not in (16, 32, 64, 128) or n_head not in (1, 2, 4) or n_block < 1 or embed_dim % n_head or 64 // n_head // n_head < 4:
            raise NotImplementedError("gfx950 Sable kernels: embed_dim in {16, 32, 64, 128} (nets narrower than 64 run embedded in the 64-wide "
                                      "kernels, params.WidthEmbedding) and n_head in {1, 2, 4} (SURVEY 8f rank 3)")
        self.nb, self.nh = int(n_block), int(n_head)
        self.EL = int(embed_dim)        # logical embed_dim (what the optimiser, checkpoints and the reference see)
        self.E = E = 128 if self.EL == 128 else 64   # width of the device network
        self.hs = E // self.nh          # head width of the device network
        self.gs = self.hs // self.nh    # flax GroupNorm(num_groups=n_head) on (token*head, hs) rows: hs / n_head channels per group
        # retention state tiles [n_block, ntile, N, 64, 64]: one per head, or the four 64 x 64 blocks (I, J) of the one 128-wide head
        self.blockwise = self.hs > TILE
        self.ntile = 4 if self.blockwise else self.nh
        if obs_dim > 128 or action_dim > 31:
            raise NotImplementedError("obs_dim <= 128 and action_dim <= 31 required")
        super().__init__(obs_dim, device, wgrad_groups, tuning, obs_ld)
        self.A, self.K = n_agents, action_dim
        self.kappas = [1.0] * self.nh if self.ff else decay_kappas(self.nh, decay_scaling_factor)
        self.kappa = self.kappas[0]
        # P / grads: the LOGICAL parameters (optimiser, all-reduce, checkpoints); PD / grads_D: what the kernels read and write.
        # For embed_dim = 64 they are the same buffers.
        if self.EL == E:
            self.emb = None
        else:
            self.emb = WidthEmbedding(self.EL, obs_dim, action_dim, self.nb, self.nh, device)
            self.PD = FlatParams(guider_layout(E, obs_dim, action_dim, self.nb, self.nh), device)
            self.grads_D = torch.zeros_like(self.PD.flat)
        self._bind_params(guider_layout(self.EL, obs_dim, action_dim, self.nb, self.nh), lambda views: guider_named_views(views, self.EL, self.nh), grads)
        if self.emb is None:
            self.PD = self.P
        else:
            self.v = self.PD.views()
        self._init_params(seed, lambda named, key: init_guider_from_key(named, key, self.EL, self.nh),   # (a key: rec_magpo.py:598-604)
                          lambda named, s: init_guider(named, s, self.EL))
        self.npos = max_pos
        self.pe = torch.zeros(max_pos, E, device=device)
        if use_pe:
            if self.emb is None:
                self.L.call("magpo_pe_table", self.pe, max_pos, E, self._st())
            else:   # positional_encoding.py:24-60 at the logical width, every feature duplicated like the activations
                pe_l = torch.zeros(max_pos, self.EL, device=device)
                self.L.call("magpo_pe_table", pe_l, max_pos, self.EL, self._st())
                self.pe.copy_(self.emb.expand_rows(pe_l))
        assert not self.ff or (not use_pe and self.kappas == [1.0] * self.nh)   # what magpo_ff_sable_act relies on: pe stays all-zero, no decay
        self.wa: Dict[str, torch.Tensor] = {}   # fragment-major copies of self.wt for the fused acting kernel: refresh() keeps both current
        self.fused_segments = self.nh == 1 and E == 64   # token-local parts between retention ops as single launches (csrc/seg_fused.hip)
        self.wg_ws = torch.empty(self.L.call("magpo_wgrad_workspace_floats", E, 4 * E, self.G), device=device)
        self.refresh()

    # ------------------------------------------------------------------ plumbing
    def twin(self):
        """A second network of the same shape, row stride and memory settings on the same device, sharing this one's ``Tuning`` object, with
        buffers of its own and uninitialised parameters (see GruActor.twin)."""
        return type(self)(self.A, self.K, self.F, self.dev, embed_dim=self.EL, n_head=self.nh, n_block=self.nb, decay_scaling_factor=self.decay_scaling_factor,
                          use_pe=self.use_pe, max_pos=self.npos, wgrad_groups=self.G, tuning=self.tuning, obs_ld=self.Fld, memory_type=self.memory_type)

    def bind_grads(self, grads: torch.Tensor) -> None:
        """The LOGICAL gradient buffer; the kernels write ``grads_D`` -- the same buffer, or the embedded network's own, which train_bwd
        folds into ``grads``."""
        super().bind_grads(grads)
        if self.emb is None:
            self.grads_D = grads
        else:
            self.gv = self.PD.views(self.grads_D)

    def check_ffn_zero(self):
        for n, v in self.v.items():
            if ".ffn." in n and bool(v.any().item()):
                raise NotImplementedError("non-zero SwiGLU weights: the FFN branch is not evaluated by the HIP path")

    _check_loaded = check_ffn_zero   # load_named's hook

    def refresh(self):
        """Rebuild the device parameters (embed_dim < 64), the transposed (forward-GEMM) weight copies and the acting kernel's
        fragment-major copies of those after a parameter update.  Every copy is written in place on the calling stream, so work queued
        behind it -- a captured rollout included -- reads the new weights and never writes them."""
        if self.emb is not None:
            self.emb.expand(self.P.flat, self.PD.flat)
        v, E = self.v, self.E
        if self.wide:   # W_obs [F, 64] as [64][128] (forward) and [128][64] (dOn = dz W_obs^T), zero beyond F
            for name, shape in (("wobs", (E, 128)), ("wobs_nat_pad", (128, E))):
                if name not in self.wt:
                    self.wt[name] = torch.zeros(*shape, device=self.dev)
            self.wt["wobs"][:, :self.F].copy_(v["enc.obs.dense.kernel"].t())
            self.wt["wobs_nat_pad"][:self.F].copy_(v["enc.obs.dense.kernel"])
        self._tp("vh0", v["enc.head.dense0.kernel"])
        self._tp("h0", v["dec.head.dense0.kernel"])
        for b in range(self.nb):
            e, d = f"enc.block{b}.", f"dec.block{b}."
            for key, name in [(f"qkvg{b}", e + "retn.w_qkvg"), (f"wo{b}", e + "retn.w_o"), (f"qkvg1{b}", d + "retn1.w_qkvg"),
                              (f"wo1{b}", d + "retn1.w_o"), (f"q2{b}", d + "retn2.w_q"), (f"kvg2{b}", d + "retn2.w_kvg"),
                              (f"wo2{b}", d + "retn2.w_o")]:
                self._tp(key, v[name])
        h1t = self._tp("h1", v["dec.head.dense1.kernel"], LW)        # [64 (K padded)][E]
        self._tp("h1_nat_pad", h1t, E)                                # [E][64]: natural W padded to 64 columns
        if E > 64:   # dX = dY W^T with KIN = 4 E = 512 runs as two K-halves (k_linear_lds<256,*>): contiguous copies of the row halves
            for bk in range(self.nb):
                for name in (f"enc.block{bk}.retn.w_qkvg", f"dec.block{bk}.retn1.w_qkvg"):
                    W = v[name]
                    for half in (0, 1):
                        key = f"{name}.nat{half}"
                        if key not in self.wt:
                            self.wt[key] = torch.empty(E, 2 * E, device=self.dev)
                        self.wt[key].copy_(W[:, half * 2 * E:(half + 1) * 2 * E])
        self.build_act_weights()

    def _act_weight_names(self):
        names = ["vh0", "h0", "h1"]
        for b in range(self.nb):
            names += [f"qkvg{b}", f"wo{b}", f"qkvg1{b}", f"wo1{b}", f"q2{b}", f"kvg2{b}", f"wo2{b}"]
        return names

    def build_act_weights(self):
        """Fragment-major copies of the transposed weights for the fused acting kernel (csrc/fm_rows.hpp: wfrag<true>):
        Wf[g][gk][lane = m + 16 kq][4] = Wt[16 g + m][16 gk + 4 kq .. + 3], so that a wave's weight-fragment load is 1 KB contiguous.
        In-place copies into persistent buffers (static pointers for the captured rollouts, which only read them); the last step of
        :meth:`refresh`, so they exist from construction on and change whenever the transposed copies do."""
        if self.E != 64:
            return
        for name in self._act_weight_names():
            t = self.wt[name]
            d = self.wa.get(name)
            if d is None:
                d = self.wa[name] = torch.empty_like(t)
            self.L.call("magpo_act_weight_layout", t, d, t.shape[0], self._st())

    def _wgrad_side(self):
        # (with n_block > 1 the d(obs_rep) sums are accumulated in place, so the side stream is not used)
        return super()._wgrad_side() if self.nb == 1 else None

    def lin_dx_qkvg(self, dY, name, dX, R):
        """dX [R, E] = dY [R, 4E] W^T for a fused q|k|v|g projection ``name`` ([E, 4E]): one launch up to KIN = 256, two K-halves + add for E = 128."""
        E = self.E
        if E == 64:
            self.lin(dY, 4 * E, self.v[name], None, dX, E, R, 4 * E, E)
            return
        tmp = self.b.get("g_dx_half", (R, E))
        self.lin(dY, 4 * E, self.wt[name + ".nat0"], None, dX, E, R, 2 * E, E)
        self.lin(dY[:, 2 * E:], 4 * E, self.wt[name + ".nat1"], None, tmp, E, R, 2 * E, E)
        self.add_(dX, tmp)

    def add_(self, dst, src):
        self.L.call("magpo_add_inplace", dst, src, dst.numel(), self._st())

    # ------------------------------------------------------------------ acting (recurrent form)
    def _pro(self, pro, a, lda, y, ldy_in, s1, s2, use_pe, pos, pos_stride, W, idx, idx_stride, out, ldout, outpe, ldoutpe,
             Wt, bias, Y, ldy, R, NOUT):
        """Dense layer behind a row-wise op: pro 1 embed-action, 2 embed-observation, 3 residual + norm(s), 4 gelu + norm; the dense input is
        the row (+ pe when ``use_pe``); ``out`` / ``outpe`` (optional) receive the row / the row + pe.  E = 64: one launch with the row op in
        the prologue of the GEMM (csrc/linear.hip: k_linear_pro); E = 128: row kernel + k_linear_lds<128,*>."""
        E = self.E
        if E == 64:
            self.L.call("magpo_linear_pro", pro, a, lda, y, ldy_in, s1, s2, self.pe, pos, pos_stride, self.npos, 1 if use_pe else 0,
                        W, idx, idx_stride, self.v["enc.obs.norm.scale"], self.F, out, ldout, outpe, ldoutpe, Wt, bias, Y, ldy, R, NOUT,
                        self._st())
            return
        L, st, b = self.L, self._st(), self.b
        if out is None:
            out, ldout = b.get("p_row", (R, E)), E
        need_pe = use_pe or outpe is not None or pro in (1, 2)
        if need_pe and outpe is None:
            outpe, ldoutpe = b.get("p_rowpe", (R, E)), E
        if pro == 1:
            L.call("magpo_embed_fwd", 1, None, 0, 0, None, W, idx, idx_stride, s1, self.pe, pos, pos_stride, self.npos, None, 0, out, ldout,
                   outpe, ldoutpe, R, E, st)
        elif pro == 2:
            L.call("magpo_embed_fwd", 0, a, lda, self.F, self.v["enc.obs.norm.scale"], W, None, 0, s1, self.pe, pos, pos_stride, self.npos, None, 0,
                   out, ldout, outpe, ldoutpe, R, E, st)
        elif pro == 3:
            L.call("magpo_resnorm_fwd", a, lda, y, ldy_in, s1, s2, self.pe, pos, pos_stride, self.npos, out, ldout, outpe if need_pe else None,
                   ldoutpe if need_pe else 0, R, E, st)
        else:
            L.call("magpo_headmid_fwd", a, lda, s1, out, ldout, None, None, None, 0, R, E, st)
        if use_pe:
            self.lin(outpe, ldoutpe, Wt, bias, Y, ldy, R, E, NOUT)
        else:
            self.lin(out, ldout, Wt, bias, Y, ldy, R, E, NOUT)

    # ------------------------------------------------------------------ retention helpers (per state tile)
    def _tiles(self):
        """State tiles of one retention layer as (tile, q / k column offset, v / r column offset, width, kappa, first_v, first_qk): one per
        head, or -- one 128-wide head -- the four 64 x 64 blocks S[I][J] (q, k columns of half I meet v, r columns of half J).  Results for
        the v / r columns add over I and those for the q / k columns over J: ``first_v`` / ``first_qk`` say whether the tile is the first
        to write them (one tile per head: always)."""
        if self.blockwise:
            return [(2 * i + j, TILE * i, TILE * j, TILE, self.kappas[0], i == 0, j == 0) for i in (0, 1) for j in (0, 1)]
        return [(h, h * self.hs, h * self.hs, self.hs, self.kappas[h], True, True) for h in range(self.nh)]

    def add_rows(self, dst, ldd, src, lds, R, W):
        self.L.call("magpo_add_rows", dst, ldd, src, lds, R, W, self._st())

    def _tile_launch(self, launch, R, *outs):
        """One tile's ``launch(dst, ld, ...)`` with a (dst, ld) pair per entry (dst, ld, first, temporary's name) of ``outs``: the first
        tile to write these columns writes them in place, a later one goes to the [R, 64] temporary, which is then added."""
        tgt = [(dst, ld) if first else (self.b.get(tmp, (R, TILE)), TILE) for dst, ld, first, tmp in outs]
        launch(*(x for t in tgt for x in t))
        for (dst, ld, first, _), (t, _) in zip(outs, tgt):
            if not first:
                self.add_rows(dst, ld, t, TILE, R, TILE)

    def _ret_rec(self, S, q, ldq, k, ldk, v, ldv, env_rows, u, ldu, N, ntok, ret_from, write, gp, ldg, gamma, beta):
        """Acting: retention + GroupNorm / swish gate for every state tile; S [ntile, N, 64, 64].  Rows: token a of env e at e * env_rows + a;
        written are the rows ret_from <= a < ntok of every env.  ff_sable: the same rows from the stateless team kernel (S, write unused;
        the rows of an env are consecutive; the decoder asks for its newest token only, so the causal mask is implied by ntok)."""
        L, E, A, st = self.L, self.E, self.A, self._st()
        R = u.shape[0]
        if self.ff:   # (``post`` / ``gs``: the fused GroupNorm + gate epilogue and its group size; none and 0 for a block of the 128-wide head)
            assert env_rows == A
            masked = 0 if ret_from == 0 else 1
            launch = lambda ti, kap, w, qkv, post, gs, out, ldo: L.call("magpo_team_retention_fwd", *qkv, out, ldo, N, A, ntok, ret_from, masked, w,
                                                                        *post, gs, st)
        else:
            launch = lambda ti, kap, w, qkv, post, gs, out, ldo: L.call("magpo_retention_recurrent", S[ti], *qkv, env_rows, out, ldo, N, ntok, ret_from,
                                                                        kap, write, *post, w, gs or w, st)
        raw = self.b.get("rr_raw", (R, E)) if self.blockwise else None
        for ti, oq, ov, w, kap, first_v, _ in self._tiles():
            qkv = (q[:, oq:], ldq, k[:, oq:], ldk, v[:, ov:], ldv)
            if raw is None:   # the kernel's fused epilogue covers a whole head
                launch(ti, kap, w, qkv, (gp[:, ov:], ldg, gamma, beta), self.gs, u[:, ov:], ldu)
            else:             # (rows outside [ret_from, ntok) hold stale values: never read)
                self._tile_launch(partial(launch, ti, kap, w, qkv, (None, 0, None, None), 0), R, (raw[:, ov:], E, first_v, "rr_tmp"))
        if raw is not None:
            for a in range(ret_from, ntok):   # GroupNorm + swish gate on the 128-wide rows of token a of every env
                L.call("magpo_retpost_fwd", raw[a:], env_rows * E, gp[a:], env_rows * ldg, gamma, beta, u[a:], env_rows * ldu, N, self.hs, self.gs, E, st)

    def _ret_fwd(self, q, ldq, k, ldk, v, ldv, r, s0, seq_env, dones, name, nseq, T, masked, rows=None):
        """Training forward: r [R, E] for every state tile; keeps the chunk states ``t_{name}_{tile}`` for the backward.  ``rows`` (i32 [R],
        optional): q | k | v are row tables and token row r reads table row rows[r] (csrc/classtab.hip).  ff_sable: stateless retention
        over teams of A consecutive rows (csrc/team_retention.hip) -- no t_* state buffers, no s0, no dones."""
        L, b, E, A, st = self.L, self.b, self.E, self.A, self._st()
        if self.ff:
            assert T == 1 and rows is None
            launch = lambda ti, kap, w, qkv, out, ldo: L.call("magpo_team_retention_fwd", *qkv, out, ldo, nseq, A, A, 0, masked, w, None, 0, None, None, 0, st)
        else:
            ct = self.tuning.ret_chunk_tokens
            nch = L.call("magpo_retention_num_chunks", T, A, ct)
            launch = lambda ti, kap, w, qkv, out, ldo: L.call("magpo_retention_chunk_fwd", *qkv, out, ldo, s0[ti], seq_env, dones,
                                                              b.get(f"t_{name}_{ti}", (nseq, nch, TILE, TILE)), None, nseq, T, A, masked, kap, w, rows, ct, st)
        for ti, oq, ov, w, kap, first_v, _ in self._tiles():
            qkv = (q[:, oq:], ldq, k[:, oq:], ldk, v[:, ov:], ldv)
            self._tile_launch(partial(launch, ti, kap, w, qkv), nseq * T * A, (r[:, ov:], E, first_v, "rf_tmp"))

    def _ret_bwd(self, q, ldq, k, ldk, v, ldv, dr, dq, lddq, dk, lddk, dv, lddv, dones, name, nseq, T, masked, rows=None):
        """Training backward of :meth:`_ret_fwd`: dq, dk, dv from dr [R, E]."""
        L, b, E, A, st = self.L, self.b, self.E, self.A, self._st()
        if self.ff:
            assert T == 1 and rows is None
            launch = lambda ti, kap, w, io, *d: L.call("magpo_team_retention_bwd", *io, *d, nseq, A, masked, w, st)
        else:
            ct = self.tuning.ret_chunk_tokens
            launch = lambda ti, kap, w, io, *d: L.call("magpo_retention_chunk_bwd", *io, *d, dones, b.t[f"t_{name}_{ti}"], nseq, T, A, masked, kap, w,
                                                       rows, ct, st)
        for ti, oq, ov, w, kap, first_v, first_qk in self._tiles():
            io = (q[:, oq:], ldq, k[:, oq:], ldk, v[:, ov:], ldv, dr[:, ov:], E)
            # block (I, J) of the 128-wide head: dq_I, dk_I add over J; dv_J adds over I
            self._tile_launch(partial(launch, ti, kap, w, io), nseq * T * A, (dq[:, oq:], lddq, first_qk, "rb_tq"), (dk[:, oq:], lddk, first_qk, "rb_tk"),
                              (dv[:, ov:], lddv, first_v, "rb_tv"))

    def act(self, obs, pos, states, sample_keys, action_out, logp_out, value_out, mask=None, value_only=False):
        """One env step for N envs (SableNetwork.get_actions, sable_network.py:443-482).  obs [N,A,F] f32, pos [N] i32
        (step_count), states = (S_enc, S_d1, S_d2) each [n_block, N, 64, 64] updated in place, sample_keys = [A,2]
        uint32 (host array: keys by value; device tensor: static arguments for graph replay).
        Writes action [N,A] i32, logp [N,A], value [N,A].  Row-wise ops are fused into the prologue of the dense layer
        that follows them and the GroupNorm + swish gate into the recurrent retention kernel."""
        L, st, A, K, F, nb, E = self.L, self._st(), self.A, self.K, self.F, self.nb, self.E
        N = obs.shape[0]
        R = N * A
        v, b = self.v, self.b
        xn = b.get("a_xn", (R, E)); qkvg = b.get("a_qkvg", (R, 4 * E)); u = b.get("a_u", (R, E)); y = b.get("a_y", (R, E))
        rep = b.get("a_rep", (R, E)); reppe = b.get("a_reppe", (R, E)); hv = b.get("a_hv", (R, E))
        if self.ff:   # memoryless: ``states`` is not read (pass None)
            s_enc = s_d1 = s_d2 = [None] * nb
        else:
            s_enc, s_d1, s_d2 = states
        if value_only and not self.ff:  # bootstrap value (rec_magpo.py:202-208): states must not change
            s_enc = b.get("a_senc_tmp", tuple(s_enc.shape)).copy_(s_enc)
        pos_tok = b.get("a_pos", (R,), torch.int32)
        pos_tok.view(N, A).copy_(pos.view(N, 1).expand(N, A))
        # encoder over the A tokens of this timestep (act_encoder_fn, encode.py:58-84)
        for blk in range(nb):
            e = f"enc.block{blk}."
            if blk == 0:
                self._pro(2, obs, self.Fld, None, 0, v["enc.ln.scale"], None, True, pos_tok, 1, v["enc.obs.dense.kernel"], None, 0, xn, E, None, 0,
                          self.wt["qkvg0"], None, qkvg, 4 * E, R, 4 * E)
            else:  # x = ln(rep of the previous block) (shared self.ln, sable_network.py:150)
                self._pro(3, rep, E, None, 0, v["enc.ln.scale"], None, True, pos_tok, 1, None, None, 0, xn, E, None, 0,
                          self.wt[f"qkvg{blk}"], None, qkvg, 4 * E, R, 4 * E)
            self._ret_rec(s_enc[blk], qkvg, 4 * E, qkvg[:, E:], 4 * E, qkvg[:, 2 * E:], 4 * E, A, u, E, N, A, 0, 1,
                          qkvg[:, 3 * E:], 4 * E, v[e + "retn.gn.scale"], v[e + "retn.gn.bias"])
            self.lin(u, E, self.wt[f"wo{blk}"], None, y, E, R, E, E)
            if blk == nb - 1:
                self._pro(3, xn, E, y, E, v[e + "ln1.scale"], v[e + "ln2.scale"], False, pos_tok, 1, None, None, 0, rep, E, reppe, E,
                          self.wt["vh0"], v["enc.head.dense0.bias"], hv, E, R, E)
            else:
                L.call("magpo_resnorm_fwd", xn, E, y, E, v[e + "ln1.scale"], v[e + "ln2.scale"], None, None, 0, 0, rep, E, None, 0, R, E, st)
        L.call("magpo_headmid_fwd", hv, E, v["enc.head.norm.scale"], None, 0, v["enc.head.dense1.kernel"],
               v["enc.head.dense1.bias"], value_out, 1, R, E, st)
        if value_only:
            return
        # autoregressive decoder (decode.py:111-153): one token per env per iteration.  Per-agent projections stay
        # resident ([N, A, .]) so that a retention state is read once per agent and written once per step.
        prev = b.get("a_prev", (N, A), torch.int32, zero=True)
        xa = b.get("d_xa", (N, E)); y1 = b.get("d_y1", (N, E)); y2 = b.get("d_y2", (N, E)); xo = b.get("d_xo", (N, E))
        xope = b.get("d_xope", (N, E))
        hp = b.get("d_hp", (N, E)); logits = b.get("d_logits", (N, LW), zero=True)
        qkvg1 = [b.get(f"d_qkvg1_{k}", (R, 4 * E)) for k in range(nb)]
        q2 = [b.get(f"d_q2_{k}", (R, E)) for k in range(nb)]
        kvg2 = [b.get(f"d_kvg2_{k}", (R, 3 * E)) for k in range(nb)]
        u1 = b.get("d_u1", (R, E)); u2 = b.get("d_u2", (R, E))
        keys, kdev = self._sample_keys_arg(sample_keys)
        for blk in range(nb):   # cross-retention queries of all agents at once
            self.lin(reppe, E, self.wt[f"q2{blk}"], None, q2[blk], E, R, E, E)
        for i in range(A):
            last = 1 if i == A - 1 else 0
            for blk in range(nb):
                d = f"dec.block{blk}."
                if blk == 0:
                    self._pro(1, None, 0, None, 0, v["dec.ln.scale"], None, True, pos, 1, v["dec.act.kernel"], prev[:, i:], A, xa, E, None, 0,
                              self.wt["qkvg10"], None, qkvg1[0][i:], A * 4 * E, N, 4 * E)
                    xin = xa
                else:  # block input = previous block's output x (xo); key = query = value = x + pe (xope)
                    self.lin(xope, E, self.wt[f"qkvg1{blk}"], None, qkvg1[blk][i:], A * 4 * E, N, E, 4 * E)
                    xin = xo
                self._ret_rec(s_d1[blk], qkvg1[blk], 4 * E, qkvg1[blk][:, E:], 4 * E, qkvg1[blk][:, 2 * E:], 4 * E, A, u1, E, N, i + 1, i, last,
                              qkvg1[blk][:, 3 * E:], 4 * E, v[d + "retn1.gn.scale"], v[d + "retn1.gn.bias"])
                self.lin(u1[i:], A * E, self.wt[f"wo1{blk}"], None, y1, E, N, E, E)
                self._pro(3, xin, E, y1, E, v[d + "ln1.scale"], None, True, pos, 1, None, None, 0, None, 0, None, 0,
                          self.wt[f"kvg2{blk}"], None, kvg2[blk][i:], A * 3 * E, N, 3 * E)
                self._ret_rec(s_d2[blk], q2[blk], E, kvg2[blk], 3 * E, kvg2[blk][:, E:], 3 * E, A, u2, E, N, i + 1, i, last,
                              kvg2[blk][:, 2 * E:], 3 * E, v[d + "retn2.gn.scale"], v[d + "retn2.gn.bias"])
                self.lin(u2[i:], A * E, self.wt[f"wo2{blk}"], None, y2, E, N, E, E)
                if blk == nb - 1:
                    self._pro(3, rep[i:], A * E, y2, E, v[d + "ln2.scale"], v[d + "ln3.scale"], False, pos, 1, None, None, 0,
                              None, 0, None, 0, self.wt["h0"], v["dec.head.dense0.bias"], hp, E, N, E)
                else:
                    L.call("magpo_resnorm_fwd", rep[i:], A * E, y2, E, v[d + "ln2.scale"], v[d + "ln3.scale"], self.pe, pos, 1, self.npos,
                           xo, E, xope, E, N, E, st)
            self._pro(4, hp, E, None, 0, v["dec.head.norm.scale"], None, False, pos, 1, None, None, 0, None, 0, None, 0,
                      self.wt["h1"], v["dec.head.dense1.bias"], logits, LW, N, K)
            k0, k1 = (0, 0) if keys is None else (int(keys[i][0]), int(keys[i][1]))
            L.call("magpo_sample_categorical", logits, LW, None if mask is None else mask[:, i], (A * K if mask is not None else 0),
                   k0, k1, None if kdev is None else kdev[i], action_out[:, i:], A, logp_out[:, i:], A, prev[:, i + 1:] if i + 1 < A else None, A, None, 0, N, K, st)

    def _sample_keys_arg(self, sample_keys, value_only=False):
        """``sample_keys`` [A, 2] uint32 as (host array or None, device table or None): a device tensor goes to the kernels as it is (static
        arguments for HIP-graph replay), host keys go by value; ``value_only`` samples nothing and needs none."""
        if torch.is_tensor(sample_keys):
            return None, sample_keys
        if value_only:
            return None, None
        return np.ascontiguousarray(np.asarray(sample_keys, dtype=np.uint32).reshape(self.A, 2)), None

    def _head_params(self, w):
        """The 15 embedding / head entries the one-launch acting kernels' tables share, in the order of include/magpo.h; ``w``: the weight
        copies the kernel reads (``wa`` fragment-major, ``wt`` transposed)."""
        v = self.v
        return [v["enc.obs.norm.scale"], v["enc.obs.dense.kernel"], v["enc.ln.scale"], v["dec.act.kernel"], v["dec.ln.scale"],
                w["vh0"], v["enc.head.dense0.bias"], v["enc.head.norm.scale"], v["enc.head.dense1.kernel"], v["enc.head.dense1.bias"],
                w["h0"], v["dec.head.dense0.bias"], v["dec.head.norm.scale"], w["h1"], v["dec.head.dense1.bias"]]

    def _block_params(self, k, w):
        """The 18 per-block entries of the same tables for block ``k``, in header order."""
        v, e, d = self.v, f"enc.block{k}.", f"dec.block{k}."
        return [w[f"qkvg{k}"], w[f"wo{k}"], v[e + "ln1.scale"], v[e + "ln2.scale"], v[e + "retn.gn.scale"], v[e + "retn.gn.bias"],
                w[f"qkvg1{k}"], w[f"wo1{k}"], v[d + "ln1.scale"], v[d + "retn1.gn.scale"], v[d + "retn1.gn.bias"],
                w[f"q2{k}"], w[f"kvg2{k}"], w[f"wo2{k}"], v[d + "ln2.scale"], v[d + "ln3.scale"], v[d + "retn2.gn.scale"], v[d + "retn2.gn.bias"]]

    def act_fused(self, obs, pos, states, sample_keys, action_out, logp_out, value_out, mask=None, value_only=False, done=None, tag="",
                  pending=False, flush=True, precand=False, defer=False):
        """Same contract as :meth:`act`, ONE launch per env step (csrc/act_fused_kernel.hpp: k_sable_act): a wave carries 4 - 16 envs
        through encoder, the A decoder iterations and the sampling.  states [n_block, n_head, N, 64, 64].  ``done`` [N] u8
        (optional): envs whose episode ended on the previous step -- their carried states are read as zero
        (rec_magpo.py:164-169), which replaces a separate zeroing pass between steps.
        ``pending`` / ``flush``: the kernel defers a step's decoder-state update to the next launch so that every state is read and
        written once per step (include/magpo.h).  The defaults {False, True} are a stand-alone step (states settled on return); a
        rollout passes pending = (t > 0), flush = False and ends with a launch that has flush = True (the bootstrap-value launch).
        The scratch rows that carry the pending k | v rows belong to ``tag``.
        ``defer`` / ``precand`` (include/magpo.h): inside a rollout half of the workgroups run the block-0 candidate pre-pass of the NEXT
        step at the end of the launch (defer) and skip it in the next one (precand), so that they stream states while the others decode."""
        A, K, F, nb, nh = self.A, self.K, self.F, self.nb, self.nh
        if self.ff:
            raise NotImplementedError("ff_sable has no retention state to carry: its one-launch acting step is SableGuider.act_team_fused "
                                      "(magpo_ff_sable_act), the kernel-by-kernel chain is SableGuider.act")
        if A > 8 or self.E != 64:   # token staging registers / 64-wide register rows of the fused kernel: larger teams take the kernel-by-kernel path (states settled on return)
            if done is not None:
                for k in range(nb):
                    for h in range(self.ntile):
                        self.L.call("magpo_zero_states_where_done", states[0][k][h], states[1][k][h], states[2][k][h], done, obs.shape[0], self._st())
            return self.act(obs, pos, states, sample_keys, action_out, logp_out, value_out, mask=mask, value_only=value_only)
        N = obs.shape[0]
        R = N * A
        b = self.b
        s_enc, s_d1, s_d2 = states   # value_only (bootstrap value, rec_magpo.py:202-208): the kernel writes no state
        keys, kdev = self._sample_keys_arg(sample_keys, value_only)
        args = (obs, pos, mask, kdev, s_enc, s_d1, s_d2, action_out, logp_out, value_out, done)

        def table():   # the global pointers, then 21 per block (everything beside ``args``: parameters, weight copies, scratch of (tag, N))
            g = lambda n, w=E, rows=R: b.get(f"f{tag}_" + n, (rows, w))   # scratch per caller tag (env groups may act concurrently)
            glob = [obs, pos, mask, kdev, *self._head_params(self.wa),
                    self.pe, s_enc, s_d1, s_d2,
                    g("xn"), done, g("qkvg", 4 * E), g("u"), g("y"), g("rep"), g("reppe"), g("hv"),
                    g("xa", E, N), g("kin1", E, N), g("y1", E, N), g("c", E, N), g("cpe", E, N), g("y2", E, N), g("xo", E, N),
                    g("xope", E, N), g("hp", E, N), g("hn", E, N), g("logits", E, N), g("u1"), g("u2"),
                    b.get(f"f{tag}_prev", (N, A), torch.int32, zero=True), action_out, logp_out, value_out,
                    b.get(f"f{tag}_ptab", (N, (K + 2) * E)) if nh == 1 else None]
            blk = []
            for k in range(nb):
                blk += self._block_params(k, self.wa) + [g(f"qkvg1_{k}", 4 * E), g(f"q2_{k}"), g(f"kvg2_{k}", 4 * E)]   # kvg2 rows: [k | v | - | P2] (ld 256)
            return glob + blk

        tab = self.ptr_table(("act", tag, N) + tuple(None if t is None else t.data_ptr() for t in args), table)
        gp, bp = tab[:tab.size - 21 * nb], tab[tab.size - 21 * nb:]
        dims = np.array([N, A, K, F, nb, nh, self.hs, self.gs, self.npos, 1 if value_only else 0, self.Fld, self.tuning.act_envs_per_wave,
                         1 if pending else 0, 1 if flush else 0, 1 if precand else 0, 1 if defer else 0], dtype=np.int32)
        kap = np.array((self.kappas + [0.0] * 4)[:4], dtype=np.float32)
        self.L.call("magpo_sable_act", dims.ctypes.data, kap.ctypes.data, None if keys is None else keys.ctypes.data,
                    gp.ctypes.data, int(gp.size), bp.ctypes.data, int(bp.size), self._st())

    def team_fused_supported(self) -> bool:
        """The shape set of magpo_ff_sable_act: 64-wide rows (embed_dim 16 / 32 embedded), at most 8 agents and 4 blocks."""
        return self.ff and self.E == 64 and self.A <= 8 and self.nb <= 4

    def act_team_fused(self, obs, pos, states, sample_keys, action_out, logp_out, value_out, mask=None, value_only=False):
        """:meth:`act` of a memoryless network (memory_type "ff_sable") in ONE launch per env step (csrc/ff_sable_act.hip: a workgroup
        carries 32 envs through encoder, value head, the A decoder iterations and the sampling).  Same contract as :meth:`act`;
        ``states`` is ignored (pass None) and ``pos`` is not read (no timestep positional encoding).  Networks outside the kernel's shape
        set (embed_dim 128, more than 8 agents or 4 blocks) take the kernel-by-kernel chain."""
        if not self.ff:
            raise ValueError("act_team_fused is the acting step of a memoryless network (memory_type='ff_sable'); a recurrent one acts "
                             "through act_fused")
        if not self.team_fused_supported():
            return self.act(obs, pos, states, sample_keys, action_out, logp_out, value_out, mask=mask, value_only=value_only)
        A, K, nb = self.A, self.K, self.nb
        N = obs.shape[0]
        keys, kdev = self._sample_keys_arg(sample_keys, value_only)
        need = 32 * ((N + 31) // 32) * A * (384 + 256 * nb)
        args = (obs, mask, kdev, action_out, logp_out, value_out)

        def table():   # 22 global pointers, then 18 per block (include/magpo.h)
            glob = [obs, mask, kdev, *self._head_params(self.wt), self.b.get(f"tf_scratch{need}", (need,)), action_out, logp_out, value_out]
            return glob + [t for k in range(nb) for t in self._block_params(k, self.wt)]

        tab = self.ptr_table(("act_team", N) + tuple(None if t is None else t.data_ptr() for t in args), table)
        gp, bp = tab[:22], tab[22:]
        dims = np.array([N, A, K, self.F, nb, self.nh, self.hs, self.gs, 1 if value_only else 0, self.Fld], dtype=np.int32)
        self.L.call("magpo_ff_sable_act", dims.ctypes.data, None if keys is None else keys.ctypes.data, gp.ctypes.data, int(gp.size),
                    bp.ctypes.data, int(bp.size), need, self._st())

    # the reference's names for the two apply functions of the Sable network (rec_magpo.py:624-628)
    get_actions = act_fused        # partial(sable_network.apply, method="get_actions"): execution  (apply = train_fwd: end of the file)

    # ------------------------------------------------------------------ post-retention segment (contract of magpo_seg_post / magpo_seg_bwd)
    def _seg_fwd(self, tail, key, pfx, r, gp, ldg, res, s1, s2, pos, o, ope, R, w0_t=None, b0=None, out0=None, ld0=0, hs=None, hw=None,
                 hb1=None, value=None, q2_t=(), q2=(), hn=None, w1_t=None, b1=None, logits=None, rows=None):
        """Token-local part between two retention ops, for the retention layer ``pfx`` (parameters) / ``key`` (W_o^T copy, workspaces):
        u = swish(gp) * GroupNorm(r); y = u W_o; o = rms(res + y) s1 [-> rms s2]; ope = o + pe[pos]; then the tail (include/magpo.h:
        1 value head + cross-retention queries, 2 the k | v | g projection, 3 logit head, 0 none).  One launch (csrc/seg_fused.hip)
        with ``fused_segments`` -- u and y are then not stored: the fused backward recomputes them -- else kernel by kernel."""
        v, E = self.v, self.E
        gamma, beta, wo_t = v[pfx + "gn.scale"], v[pfx + "gn.bias"], self.wt["wo" + key]
        if self.fused_segments:
            q2_t, q2 = list(q2_t) + [None] * (4 - len(q2_t)), list(q2) + [None] * (4 - len(q2))
            tab = [r, gp, gamma, beta, wo_t, res, s1, s2, self.pe, pos, None, None, o, ope, w0_t, b0, out0, hs, hw, hb1, value, *q2_t, *q2,
                   hn, w1_t, b1, logits, rows]
            ptrs = self.ptr_table(("seg_post",) + tuple(None if t is None else t.data_ptr() for t in tab), tab)
            dims = np.array([tail, self.K, self.npos, ldg, ld0, sum(1 for t in q2 if t is not None)], dtype=np.int32)
            self.L.call("magpo_seg_post", dims.ctypes.data, R, ptrs.ctypes.data, int(ptrs.size), self._st())
            return
        assert rows is None, "class tables are read in place by the fused segment kernels only"
        L, st = self.L, self._st()
        u, y = self.b.get("t_u" + key, (R, E)), self.b.get("t_y" + key, (R, E))   # kept for the backward
        L.call("magpo_retpost_fwd", r, E, gp, ldg, gamma, beta, u, E, R, self.hs, self.gs, E, st)
        self.lin(u, E, wo_t, None, y, E, R, E, E)
        pe = (self.pe, pos, 1, self.npos) if ope is not None else (None, None, 0, 0)
        L.call("magpo_resnorm_fwd", res, E, y, E, s1, s2, *pe, o, 0 if o is None else E, ope, 0 if ope is None else E, R, E, st)
        if tail == 2:
            self.lin(ope, E, w0_t, b0, out0, ld0, R, E, ld0)
        elif tail:
            self.lin(o, E, w0_t, b0, out0, ld0, R, E, E)
            if tail == 1:
                L.call("magpo_headmid_fwd", out0, ld0, hs, None, 0, hw, hb1, value, 1, R, E, st)
                for wq, q in zip(q2_t, q2):
                    self.lin(ope, E, wq, None, q, E, R, E, E)
            else:
                L.call("magpo_headmid_fwd", out0, ld0, hs, hn, E, None, None, None, 0, R, E, st)
                self.lin(hn, E, w1_t, b1, logits, LW, R, E, self.K)

    def _seg_bwd(self, key, pfx, a, s1, s2, d0, d1, d2, r, gp, ldg, dsum, dr, dgp, lddg, R, g_s1, g_s2, rows=None):
        """Backward of the front of :meth:`_seg_fwd` (a = its ``res``): dsum = d(res + y) of the incoming d0 [+ d1 + d2] through the
        RMSNorm(s), the W_o gradient u^T dsum, du = dsum W_o^T, (dr, dgp) through GroupNorm + gate, and the parameter-gradient rows of
        s1 [, s2], gamma, beta.  One launch + slab reductions (csrc/seg_fused.hip: k_seg_bwd) with ``fused_segments``, else kernel
        by kernel on the u and y the composed forward kept."""
        v, gv, b, E = self.v, self.gv, self.b, self.E
        gamma, beta, wo_nat, g_wo = v[pfx + "gn.scale"], v[pfx + "gn.bias"], v[pfx + "w_o"], gv[pfx + "w_o"]
        if self.fused_segments:
            G = self.L.call("magpo_seg_bwd_grid", R)
            sl = [b.get(f"sb_{i}", (G, E)) for i in range(4)]
            sl_wo = b.get("sb_wo", (G, E * E))
            tab = [a, None, s1, s2, d0, d1, d2, wo_nat, r, gp, gamma, beta, dsum, dr, dgp, sl[0], sl[1] if s2 is not None else None, sl[2], sl[3],
                   rows, self.wt["wo" + key], sl_wo]
            ptrs = self.ptr_table(("seg_bwd",) + tuple(None if t is None else t.data_ptr() for t in tab), tab)
            self.L.call("magpo_seg_bwd", R, ldg, lddg, ptrs.ctypes.data, int(ptrs.size), self._st())
            self.reduce(sl[0], g_s1)
            if s2 is not None:
                self.reduce(sl[1], g_s2)
            self.reduce(sl[2], gv[pfx + "gn.scale"]); self.reduce(sl[3], gv[pfx + "gn.bias"])
            self.reduce(sl_wo, g_wo)
            return
        assert rows is None, "class tables are read in place by the fused segment kernels only"
        L, st = self.L, self._st()
        grid = L.call("magpo_row_grid", R)
        sa, sb, du = b.get("s_a", (grid, E)), b.get("s_b", (grid, E)), b.get("g_du", (R, E))
        ld = lambda d: 0 if d is None else E
        L.call("magpo_resnorm_bwd", a, E, b.t["t_y" + key], E, s1, s2, d0, E, d1, ld(d1), d2, ld(d2), dsum, E, sa, sb if s2 is not None else None,
               R, E, st)
        self.reduce(sa, g_s1)
        if s2 is not None:
            self.reduce(sb, g_s2)
        self.wgrad(b.t["t_u" + key], E, dsum, E, R, E, E, g_wo)
        self.lin(dsum, E, wo_nat, None, du, E, R, E, E)
        L.call("magpo_retpost_bwd", r, E, gp, ldg, gamma, beta, du, E, dr, E, dgp, lddg, sa, sb, R, self.hs, self.gs, E, st)
        for h in range(self.nh):   # scale / bias [hs] are shared by the heads: fold the per-column slabs
            self.reduce(sa[:, h * self.hs:], gv[pfx + "gn.scale"], P=self.hs, stride=E, accumulate=h > 0)
            self.reduce(sb[:, h * self.hs:], gv[pfx + "gn.bias"], P=self.hs, stride=E, accumulate=h > 0)

    def _class_fwd(self, side):
        """Block 0 of ``side`` ("enc" / "dec") on its class table: the embedding and the first q|k|v|g projection on the C distinct input
        rows; unless the block's consumers read the tables through the class index (``direct``), both are gathered by class into the
        per-token buffers.  Returns (block input [C, E], q|k|v|g [C, 4E]); ``_class_bwd`` is the backward."""
        L, st, b, v, E, F, sv = self.L, self._st(), self.b, self.v, self.E, self.F, self._saved
        rows = sv["classes"]["rows"]
        if side == "enc":   # observation embedding: names of x, x + pe and the projection (= its weight copy's)
            (inp, pos_c), (x, xpe, proj) = rows[:2], ("xn0", "kin0", "qkvg0")
            embed = (0, inp, F, F, v["enc.obs.norm.scale"], v["enc.obs.dense.kernel"], None, 0, v["enc.ln.scale"])
        else:               # action embedding
            (inp, pos_c), (x, xpe, proj) = rows[2:], ("x0", "xpe0", "qkvg10")
            embed = (1, None, 0, 0, None, v["dec.act.kernel"], inp, 1, v["dec.ln.scale"])
        C, R = inp.shape[0], sv["R"]
        x_c, xpe_c, qkvg_c = b.get("c_" + x, (C, E)), b.get("c_" + xpe, (C, E)), b.get("c_" + proj, (C, 4 * E))
        L.call("magpo_embed_fwd", *embed, self.pe, pos_c, 1, self.npos, None, 0, x_c, E, xpe_c, E, C, E, st)
        self.lin(xpe_c, E, self.wt[proj], None, qkvg_c, 4 * E, C, E, 4 * E)
        if not sv["direct"]:   # per-token copies for the unfused segment kernels; the fused ones read the tables through the class index
            cls = sv["classes"][side][0]
            L.call("magpo_gather_rows", x_c, E, cls, b.get("t_" + x, (R, E)), E, R, E, st)
            L.call("magpo_gather_rows", qkvg_c, 4 * E, cls, b.get("t_" + proj, (R, 4 * E)), 4 * E, R, 4 * E, st)
        return x_c, qkvg_c

    def _obs_embed_bwd(self, d0, d1, obs, ldo, R, grid, sfx, accumulate):
        """Backward of the observation embedding on R rows of ``obs`` (stride ldo) from the gradient d0 + d1 at its output, with the three
        parameter gradients from the slabs ``s_{a,w,d}{sfx}`` of ``grid`` rows (enc.ln.scale: shared by the blocks, hence ``accumulate``)."""
        b, v, gv, E, F = self.b, self.v, self.gv, self.E, self.F
        sa, sw, sd = b.get("s_a" + sfx, (grid, E)), b.get("s_w" + sfx, (grid, 32 * E)), b.get("s_d" + sfx, (grid, 32))
        self.L.call("magpo_embed_bwd", 0, None, 0, d0, E, d1, E, None, 0, v["enc.ln.scale"], None, 0, sa, sw, F,
                    obs, ldo, F, v["enc.obs.norm.scale"], v["enc.obs.dense.kernel"], sd, None, 0, R, E, self._st())
        self.reduce(sa, gv["enc.ln.scale"], accumulate=accumulate)
        self.reduce(sd, gv["enc.obs.norm.scale"], P=F, stride=32)
        self.reduce(sw, gv["enc.obs.dense.kernel"], P=F * E, stride=32 * E)

    def _class_bwd(self, side, dqkvg, dsum, kin_c, wname):
        """Block 0 of ``side`` ("enc" / "dec") on its class table: the per-class sums of both gradient paths into the block input, then on
        the C class rows the weight gradient of the q|k|v|g projection ``wname`` (input rows ``kin_c``) and its dX.
        Returns (d(input) residual path [C, E], d(input) projection path [C, E], C)."""
        L, st, b, E, cl = self.L, self._st(), self.b, self.E, self._saved["classes"]
        _, order, offsets = cl[side]
        i = 0 if side == "enc" else 1
        C = cl["rows"][2 * i].shape[0]
        dq_c, ds_c, dkin_c = b.get(f"gc_dqkvg{i}", (C, 4 * E)), b.get(f"gc_dsum{i}", (C, E)), b.get(f"gc_dkin{i}", (C, E))
        part = b.get("gc_part_" + side[0], (L.call("magpo_class_sum_slots", C), C, 4 * E))
        L.call("magpo_class_sum", dqkvg, 4 * E, order, offsets, C, 4 * E, part, dq_c, st)
        L.call("magpo_class_sum", dsum, E, order, offsets, C, E, part, ds_c, st)
        self.wgrad(kin_c, E, dq_c, 4 * E, C, E, 4 * E, self.gv[wname])
        self.lin_dx_qkvg(dq_c, wname, dkin_c, C)
        return ds_c, dkin_c, C

    # ------------------------------------------------------------------ training forward (chunkwise form)
    def train_fwd(self, obs, prev_idx, pos, dones, s0, seq_env, nseq: int, T: int, classes=None):
        """obs [R,F], prev_idx [R] (0 = start token, a+1 otherwise), pos [R] step counts, dones [nseq,T] u8,
        s0 = three [n_block, N, 64, 64] rollout-start states indexed through seq_env [nseq].
        ``classes`` (optional, csrc/classtab.hip) = dict(rows=(obs_enc [Ce,F], pos_enc [Ce], prev_dec [Cd], pos_dec [Cd]),
        enc=(cls, order, offsets), dec=(cls, order, offsets)): the embeddings and the first q|k|v|g projections of encoder
        and decoder are then evaluated on the distinct input rows only and gathered by class.
        Returns (logits [R,64] raw with K valid columns, value [R])."""
        L, st, A, K, F, v, b, nb, E = self.L, self._st(), self.A, self.K, self.F, self.v, self.b, self.nb, self.E
        R = nseq * T * A
        if self.ff:   # items of one time step: no start states, no dones, dense first layers
            if T != 1 or classes is not None:
                raise ValueError("ff_sable trains on single time steps (T = 1) without class tables")
            s0 = ((None,) * nb,) * 3
        g = lambda n, w=E: b.get("t_" + n, (R, w))
        direct = classes is not None and self.fused_segments   # block-0 consumers read the class tables through the class index
        self._saved = dict(obs=obs, prev_idx=prev_idx, pos=pos, dones=dones, nseq=nseq, T=T, R=R, classes=classes, direct=direct)
        rep, reppe, hv, value = g("rep"), g("reppe"), g("hv"), b.get("t_value", (R,))
        logits = b.get("t_logits", (R, LW), zero=True)
        # ---- encoder
        if classes is not None:   # embedding + first projection on the Ce distinct (agent, target, step) rows, gathered by class
            xn_c, qkvg_c = self._class_fwd("enc")
        elif self.wide:   # obs_encoder + ln on padded rows: RMSNorm_F -> Dense on the MFMA kernel -> GELU + RMSNorm (sable_network.py:93-101,132)
            on, z0 = b.get("t_on", (R, 128)), g("z0")
            L.call("magpo_obsnorm_fwd", obs, self.Fld, F, v["enc.obs.norm.scale"], on, R, st)
            self.lin(on, 128, self.wt["wobs"], None, z0, E, R, 128, E)
            L.call("magpo_headmid_fwd", z0, E, v["enc.ln.scale"], g("xn0"), E, None, None, None, 0, R, E, st)
            L.call("magpo_add_pe", g("xn0"), E, self.pe, pos, 1, self.npos, g("kin0"), E, R, E, st)
        else:
            L.call("magpo_embed_fwd", 0, obs, self.Fld, F, v["enc.obs.norm.scale"], v["enc.obs.dense.kernel"], None, 0, v["enc.ln.scale"],
                   self.pe, pos, 1, self.npos, None, 0, g("xn0"), E, g("kin0"), E, R, E, st)   # z is recomputed by the backward
        for k in range(nb):
            e = f"enc.block{k}."
            rows = classes["enc"][0] if direct and k == 0 else None
            if rows is not None:
                xn, qkvg = xn_c, qkvg_c
            else:
                xn, qkvg = g(f"xn{k}"), g(f"qkvg{k}", 4 * E)
            r = g(f"r{k}")
            if k > 0 or classes is None:
                self.lin(g(f"kin{k}"), E, self.wt[f"qkvg{k}"], None, qkvg, 4 * E, R, E, 4 * E)
            self._ret_fwd(qkvg, 4 * E, qkvg[:, E:], 4 * E, qkvg[:, 2 * E:], 4 * E, r, s0[0][k], seq_env, dones, f"st_e{k}", nseq, T, 0, rows=rows)
            if k == nb - 1:   # GroupNorm + gate, W_o, residual + norms, then the value head and the cross-retention queries of every decoder block
                self._seg_fwd(1, f"{k}", e + "retn.", r, qkvg[:, 3 * E:], 4 * E, xn, v[e + "ln1.scale"], v[e + "ln2.scale"], pos, rep, reppe, R,
                              w0_t=self.wt["vh0"], b0=v["enc.head.dense0.bias"], out0=hv, ld0=E, hs=v["enc.head.norm.scale"],
                              hw=v["enc.head.dense1.kernel"], hb1=v["enc.head.dense1.bias"], value=value,
                              q2_t=[self.wt[f"q2{j}"] for j in range(nb)], q2=[g(f"q2{j}") for j in range(nb)], rows=rows)
            else:
                repb = g(f"repb{k}")
                self._seg_fwd(0, f"{k}", e + "retn.", r, qkvg[:, 3 * E:], 4 * E, xn, v[e + "ln1.scale"], v[e + "ln2.scale"], pos, repb, None, R,
                              rows=rows)
                L.call("magpo_resnorm_fwd", repb, E, None, 0, v["enc.ln.scale"], None, self.pe, pos, 1, self.npos,
                       g(f"xn{k + 1}"), E, g(f"kin{k + 1}"), E, R, E, st)
        # ---- decoder
        if classes is not None:   # action embedding + first projection on the Cd distinct (previous action, step) rows
            x_c, qkvg1_c = self._class_fwd("dec")
        else:
            L.call("magpo_embed_fwd", 1, None, 0, 0, None, v["dec.act.kernel"], prev_idx, 1, v["dec.ln.scale"], self.pe, pos, 1, self.npos,
                   None, 0, g("x0"), E, g("xpe0"), E, R, E, st)   # za = W_act[prev] is gathered again by the backward
        for k in range(nb):
            d = f"dec.block{k}."
            rows = classes["dec"][0] if direct and k == 0 else None
            if rows is not None:
                x, qkvg1 = x_c, qkvg1_c
            else:
                x, qkvg1 = g(f"x{k}"), g(f"qkvg1{k}", 4 * E)
            r1, cpe, q2, kvg2, r2 = g(f"r1{k}"), g(f"cpe{k}"), g(f"q2{k}"), g(f"kvg2{k}", 3 * E), g(f"r2{k}")
            if k > 0 or classes is None:
                self.lin(g(f"xpe{k}"), E, self.wt[f"qkvg1{k}"], None, qkvg1, 4 * E, R, E, 4 * E)
            self._ret_fwd(qkvg1, 4 * E, qkvg1[:, E:], 4 * E, qkvg1[:, 2 * E:], 4 * E, r1, s0[1][k], seq_env, dones, f"st_1{k}", nseq, T, 1, rows=rows)
            # after the self-retention: gate, W_o, residual + norm + pe (only c + pe is consumed) and the k | v | g projection of the cross-retention
            self._seg_fwd(2, f"1{k}", d + "retn1.", r1, qkvg1[:, 3 * E:], 4 * E, x, v[d + "ln1.scale"], None, pos, None, cpe, R,
                          w0_t=self.wt[f"kvg2{k}"], out0=kvg2, ld0=3 * E, rows=rows)
            self._ret_fwd(q2, E, kvg2, 3 * E, kvg2[:, E:], 3 * E, r2, s0[2][k], seq_env, dones, f"st_2{k}", nseq, T, 1)
            if k == nb - 1:   # ... and after the cross-retention of the last block the logit head
                self._seg_fwd(3, f"2{k}", d + "retn2.", r2, kvg2[:, 2 * E:], 3 * E, rep, v[d + "ln2.scale"], v[d + "ln3.scale"], pos, g(f"x{nb}"), None, R,
                              w0_t=self.wt["h0"], b0=v["dec.head.dense0.bias"], out0=g("hp"), ld0=E, hs=v["dec.head.norm.scale"], hn=g("hn"),
                              w1_t=self.wt["h1"], b1=v["dec.head.dense1.bias"], logits=logits)
            else:
                self._seg_fwd(0, f"2{k}", d + "retn2.", r2, kvg2[:, 2 * E:], 3 * E, rep, v[d + "ln2.scale"], v[d + "ln3.scale"], pos,
                              g(f"x{k + 1}"), g(f"xpe{k + 1}"), R)
        return logits, value

    # ------------------------------------------------------------------ training backward
    def train_bwd(self, dlogits, dvalue):
        """dlogits [R,64] (columns >= K zero), dvalue [R]; fills self.grads (every entry written exactly once, the
        shared encoder ln scale accumulates over blocks)."""
        L, st, A, K, F, v, gv, b, nb, E = self.L, self._st(), self.A, self.K, self.F, self.v, self.gv, self.b, self.nb, self.E
        sv = self._saved
        R, nseq, T = sv["R"], sv["nseq"], sv["T"]
        obs, prev_idx, pos, dones = sv["obs"], sv["prev_idx"], sv["pos"], sv["dones"]
        cl, Rd = sv["classes"], R
        t = lambda n: b.t["t_" + n]
        g = lambda n, w=E: b.get("g_" + n, (R, w))
        grid = L.call("magpo_row_grid", R)
        slab = lambda n, w=E: b.get("s_" + n, (grid, w))
        # ---- logit head
        dhn = g("dhn")
        self.dense_bwd(t("hn"), E, dlogits, LW, v["dec.head.dense1.kernel"], dhn, E, R, E, K, gv["dec.head.dense1.kernel"], gv["dec.head.dense1.bias"],
                       lin_W=self.wt["h1_nat_pad"], lin_K=LW)
        dhp = g("dhp_l")
        L.call("magpo_headmid_bwd", t("hp"), E, v["dec.head.norm.scale"], dhn, E, None, None, 0, dhp, E, slab("a"), None, None, R, E, st)
        self.reduce(slab("a"), gv["dec.head.norm.scale"])
        dout = g("dout")
        self.dense_bwd(t(f"x{nb}"), E, dhp, E, v["dec.head.dense0.kernel"], dout, E, R, E, E, gv["dec.head.dense0.kernel"], gv["dec.head.dense0.bias"])
        # ---- decoder blocks, last to first.  incoming gradient of block k's output x_{k+1}: (din0 [+ din1])
        din0, din1 = dout, None
        drep_q, drep_r = None, None      # running sums of d(obs_rep): cross-retention query path / residual path
        for k in reversed(range(nb)):
            d = f"dec.block{k}."
            dsum2 = g(f"dsum2_{k}")
            dr2 = g("dr"); dq2 = g(f"dq2_{k}"); dkvg2 = g(f"dkvg2_{k}", 3 * E)
            kvg2 = t(f"kvg2{k}")
            self._seg_bwd(f"2{k}", d + "retn2.", t("rep"), v[d + "ln2.scale"], v[d + "ln3.scale"], din0, din1, None, t(f"r2{k}"),
                          kvg2[:, 2 * E:], 3 * E, dsum2, dr2, dkvg2[:, 2 * E:], 3 * E, R, gv[d + "ln2.scale"], gv[d + "ln3.scale"])
            self._ret_bwd(t(f"q2{k}"), E, kvg2, 3 * E, kvg2[:, E:], 3 * E, dr2, dq2, E, dkvg2, 3 * E, dkvg2[:, E:], 3 * E, dones,
                          f"st_2{k}", nseq, T, 1)
            dreppe = g(f"dreppe_{k}"); dcpe = g("dcpe")
            # (the same predicate NetBase.dense_bwd routes on, asked here as well because the pair's launches of the two projections
            # interleave below the threshold -- the two places must stay in step)
            if self._dense_bwd_fused(R, E, E):
                self.dense_bwd(t("reppe"), E, dq2, E, v[d + "retn2.w_q"], dreppe, E, R, E, E, gv[d + "retn2.w_q"])
                self.wgrad(t(f"cpe{k}"), E, dkvg2, 3 * E, R, E, 3 * E, gv[d + "retn2.w_kvg"])
            else:   # both weight gradients first (the side stream's order), then both dX
                self.wgrad(t("reppe"), E, dq2, E, R, E, E, gv[d + "retn2.w_q"])
                self.wgrad(t(f"cpe{k}"), E, dkvg2, 3 * E, R, E, 3 * E, gv[d + "retn2.w_kvg"])
                self.lin(dq2, E, v[d + "retn2.w_q"], None, dreppe, E, R, E, E)
            self.lin(dkvg2, 3 * E, v[d + "retn2.w_kvg"], None, dcpe, E, R, 3 * E, E)
            if drep_q is None:
                drep_q, drep_r = dreppe, dsum2
            else:
                self.add_(drep_q, dreppe); self.add_(drep_r, dsum2)
            # self-retention: c = rms(x_k + y1) * ln1
            dsum1 = g(f"dsum1_{k}")
            dr1 = g("dr"); dqkvg1 = g(f"dqkvg1_{k}", 4 * E)
            rows = cl["dec"][0] if sv["direct"] and k == 0 else None
            qkvg1, xk = (b.t["c_qkvg10"], b.t["c_x0"]) if rows is not None else (t(f"qkvg1{k}"), t(f"x{k}"))
            self._seg_bwd(f"1{k}", d + "retn1.", xk, v[d + "ln1.scale"], None, dcpe, None, None, t(f"r1{k}"), qkvg1[:, 3 * E:], 4 * E,
                          dsum1, dr1, dqkvg1[:, 3 * E:], 4 * E, R, gv[d + "ln1.scale"], None, rows=rows)
            self._ret_bwd(qkvg1, 4 * E, qkvg1[:, E:], 4 * E, qkvg1[:, 2 * E:], 4 * E, dr1, dqkvg1, 4 * E, dqkvg1[:, E:], 4 * E,
                          dqkvg1[:, 2 * E:], 4 * E, dones, f"st_1{k}", nseq, T, 1, rows=rows)
            if k == 0 and cl is not None:   # block 0 on the class table: per-class sums of both gradient paths, then Cd rows
                din0, din1, Rd = self._class_bwd("dec", dqkvg1, dsum1, b.t["c_xpe0"], d + "retn1.w_qkvg")
                prev_idx = cl["rows"][2]
                break
            self.wgrad(t(f"xpe{k}"), E, dqkvg1, 4 * E, R, E, 4 * E, gv[d + "retn1.w_qkvg"])
            dkin1 = g(f"dkin1_{k}")
            self.lin_dx_qkvg(dqkvg1, d + "retn1.w_qkvg", dkin1, R)
            din0, din1 = dsum1, dkin1      # gradient of x_k (block input): residual path + key/query/value path
        gridd = L.call("magpo_row_grid", Rd)
        sa_d, sw_d = b.get("s_a_d", (gridd, E)), b.get("s_w_d", (gridd, 32 * E))
        L.call("magpo_embed_bwd", 1, None, 0, din0, E, din1, E, None, 0, v["dec.ln.scale"], None, 0, sa_d, sw_d,
               K + 1, None, 0, 0, None, v["dec.act.kernel"], None, prev_idx, 1, Rd, E, st)
        self.reduce(sa_d, gv["dec.ln.scale"])
        self.reduce(sw_d, gv["dec.act.kernel"], P=(K + 1) * E, stride=32 * E)
        # ---- value head
        dhv = g("dhv")
        L.call("magpo_headmid_bwd", t("hv"), E, v["enc.head.norm.scale"], None, 0, v["enc.head.dense1.kernel"], dvalue, 1, dhv, E,
               slab("a"), slab("b"), slab("c", 1), R, E, st)
        self.reduce(slab("a"), gv["enc.head.norm.scale"]); self.reduce(slab("b"), gv["enc.head.dense1.kernel"])
        self.reduce(slab("c", 1), gv["enc.head.dense1.bias"], P=1, stride=1)
        drep_v = g("dout")
        self.dense_bwd(t("rep"), E, dhv, E, v["enc.head.dense0.kernel"], drep_v, E, R, E, E, gv["enc.head.dense0.kernel"], gv["enc.head.dense0.bias"])
        # ---- encoder blocks, last to first; d(rep) = value head + cross-retention queries + decoder residuals
        e0, e1, e2 = drep_v, drep_q, drep_r
        first_ln = True
        for k in reversed(range(nb)):
            e = f"enc.block{k}."
            dsum0 = g(f"dsum0_{k}")
            dr = g("dr"); dqkvg = g(f"dqkvg_{k}", 4 * E)
            rows = cl["enc"][0] if sv["direct"] and k == 0 else None
            qkvg, xnk = (b.t["c_qkvg0"], b.t["c_xn0"]) if rows is not None else (t(f"qkvg{k}"), t(f"xn{k}"))
            self._seg_bwd(f"{k}", e + "retn.", xnk, v[e + "ln1.scale"], v[e + "ln2.scale"], e0, e1, e2, t(f"r{k}"), qkvg[:, 3 * E:], 4 * E,
                          dsum0, dr, dqkvg[:, 3 * E:], 4 * E, R, gv[e + "ln1.scale"], gv[e + "ln2.scale"], rows=rows)
            self._ret_bwd(qkvg, 4 * E, qkvg[:, E:], 4 * E, qkvg[:, 2 * E:], 4 * E, dr, dqkvg, 4 * E, dqkvg[:, E:], 4 * E, dqkvg[:, 2 * E:], 4 * E,
                          dones, f"st_e{k}", nseq, T, 0, rows=rows)
            if k == 0 and cl is not None:
                ds_c, dkin, Ce = self._class_bwd("enc", dqkvg, dsum0, b.t["c_kin0"], e + "retn.w_qkvg")
                self._obs_embed_bwd(ds_c, dkin, cl["rows"][0], F, Ce, L.call("magpo_row_grid", Ce), "_e", not first_ln)
                break
            self.wgrad(t(f"kin{k}"), E, dqkvg, 4 * E, R, E, 4 * E, gv[e + "retn.w_qkvg"])
            dkin = g(f"dkin_{k}")
            self.lin_dx_qkvg(dqkvg, e + "retn.w_qkvg", dkin, R)
            if k > 0:  # xn_k = rms(rep_{k-1}) * enc.ln (shared scale): d(rep_{k-1})
                drepb = g(f"drepb_{k}")
                L.call("magpo_resnorm_bwd", t(f"repb{k - 1}"), E, None, 0, v["enc.ln.scale"], None, dsum0, E, dkin, E, None, 0, drepb, E,
                       slab("a"), None, R, E, st)
                self.reduce(slab("a"), gv["enc.ln.scale"], accumulate=not first_ln)
                first_ln = False
                e0, e1, e2 = drepb, None, None
            elif self.wide:
                dxn, dz, don = g("dxn0"), g("dz0"), b.get("g_don", (R, 128))
                L.call("magpo_copy_rows", dsum0, E, dxn, E, R, E, st)
                self.add_(dxn, dkin)
                L.call("magpo_headmid_bwd", t("z0"), E, v["enc.ln.scale"], dxn, E, None, None, 0, dz, E, slab("a"), None, None, R, E, st)
                self.reduce(slab("a"), gv["enc.ln.scale"], accumulate=not first_ln)
                self.wgrad(b.t["t_on"], 128, dz, E, R, 128, E, gv["enc.obs.dense.kernel"], krows=F)
                self.lin(dz, E, self.wt["wobs_nat_pad"], None, don, 128, R, E, 128)
                so = b.get("s_obsn", (L.call("magpo_obsnorm_grid", R), 128))
                L.call("magpo_obsnorm_bwd", obs, self.Fld, F, don, so, R, st)
                self.reduce(so, gv["enc.obs.norm.scale"], P=F, stride=128)
            else:
                self._obs_embed_bwd(dsum0, dkin, obs, self.Fld, R, grid, "", not first_ln)
        self._join_wgrad()
        if self.emb is not None:   # gradient of a logical parameter = sum over its tied device copies
            self.emb.fold(self.grads_D, self.grads)


SableGuider.apply = SableGuider.train_fwd   # sable_network.apply: the chunkwise training forward (its backward: train_bwd)


# the layout of the retention states in a learner state (systems/gpo/anakin/rec_magpo.py, systems/sable/anakin/rec_sable.py)
def sable_hstates_logical(gd: SableGuider, t: torch.Tensor) -> torch.Tensor:
    """Device retention states [n_block, ntile, N, 64, 64] -> the reference's [n_block, n_head, N, hs, hs] head states
    (get_init_hstates.py:20-43).  On the device a head state sits in a zero-padded 64 x 64 tile, and a narrow net (embed_dim < 64,
    params.WidthEmbedding) keeps logical entry (i, j) at device rows m i (q / k live in the first copy) and columns m j .. m j + m - 1
    (v is duplicated), m = 64 / embed_dim.  The one 128-wide head of embed_dim 128 / n_head 1 lives in four 64 x 64 tiles S[I][J] (tile 2 I + J)."""
    hw, m = gd.hs, max(1, 64 // gd.EL)
    if gd.blockwise:
        return torch.cat([torch.cat([t[:, 0], t[:, 1]], -1), torch.cat([t[:, 2], t[:, 3]], -1)], -2).unsqueeze(1)
    return t[..., :hw:m, :hw:m]


def load_sable_hstates(gd: SableGuider, dst: torch.Tensor, logical: torch.Tensor) -> None:
    """Inverse of ``sable_hstates_logical``: write the logical head states into the device tiles ``dst``."""
    hw, m = gd.hs, max(1, 64 // gd.EL)
    dst.zero_()
    if gd.blockwise:   # [n_block, 1, N, 128, 128] -> tiles (I, J)
        full = logical[:, 0]
        for ti in range(4):
            dst[:, ti].copy_(full[..., 64 * (ti // 2):64 * (ti // 2) + 64, 64 * (ti % 2):64 * (ti % 2) + 64])
        return
    for c in range(m):   # rows m i, every column copy
        dst[..., :hw:m, c:hw:m].copy_(logical)
