"""Host-side plumbing shared by the networks (SableGuider, GruActor, FfActor): named workspaces, transposed weight copies, the dense-layer
and weight-gradient launches with the optional side stream, slab reductions and cached device-pointer tables; ``TorsoNet`` adds the forward
and backward of one MLPTorso for the networks that have one (GruActor / GruCritic, FfActor / FfCritic), the rule for their first layer and the
derived copies of first layer and head.  ``ParamBinding`` is the flat parameter / gradient buffer with its named views, shared with QMixer."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ._lib import lib
from .params import FlatParams
from .torso import layer_name
from .tuning import Tuning


class _Bufs:
    def __init__(self, device):
        self.device = device
        self.t: Dict[str, torch.Tensor] = {}

    def get(self, name, shape, dtype=torch.float32, zero=False):
        t = self.t.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=self.device)
            self.t[name] = t
        return t


class ParamBinding:
    """One flat parameter buffer ``P`` and one flat gradient buffer ``grads`` with views by layout name (``v`` / ``gv``) and by the reference's
    names (``named`` / ``named_grads``: what the optimiser, the checkpoints and ``load_named`` see).  The class supplies ``dev`` and ``refresh``."""

    def _bind_params(self, layout, named_views=None, grads: Optional[torch.Tensor] = None) -> None:
        """``named_views``: views by layout name -> views by reference name (default: the same names).  ``grads``: a buffer to bind, else
        one of its own."""
        self._named_views = named_views or dict
        self.P = FlatParams(layout, self.dev)
        self.v = self.P.views()
        self.named = self._named_views(self.v)
        self.bind_grads(torch.zeros_like(self.P.flat) if grads is None else grads)

    def bind_grads(self, grads: torch.Tensor) -> None:
        """Make ``grads`` (flat, P.numel floats, e.g. a slice of the learner's all-reduce message) the gradient buffer."""
        assert grads.numel() == self.P.numel
        self.grads = grads
        self.gv = self.P.views(grads)
        self.named_grads = self._named_views(self.gv)

    def _init_params(self, seed, from_key, from_seed) -> None:
        """``seed``: None (parameters are loaded later), a PRNG key ([2] uint32: ``from_key(named, key)``, the parameters flax creates from
        it) or an int (``from_seed(named, seed)``, torch generator)."""
        if isinstance(seed, np.ndarray):
            from_key(self.named, seed)
        elif seed is not None:
            from_seed(self.named, seed)

    def _check_loaded(self) -> None:
        """Hook of ``load_named``: refuse parameters the kernels do not evaluate."""

    def load_named(self, params) -> None:
        with torch.no_grad():
            for n, v in self.named.items():
                v.copy_(params[n].to(self.dev, torch.float32).reshape(v.shape))
        self._check_loaded()
        self.refresh()


class NetBase(ParamBinding):
    LINEAR_VARIANT = "linear_variant"   # the Tuning field that picks this network's magpo_linear variant
    MAX_TABLES = 4096                   # cached pointer tables: all are dropped beyond this many

    def __init__(self, obs_dim: int, device, wgrad_groups: int, tuning: Optional[Tuning], obs_ld: Optional[int]):
        self.tuning = tuning if tuning is not None else Tuning.from_env()   # per-call kernel knobs (tuning.py); the library keeps none
        self.F = obs_dim
        # observation rows: F floats apart for small observations (row kernels), padded to 128 for wide ones (obs_dim > 32, e.g.
        # Robot Warehouse: the observation-side first layer then runs on the MFMA dense kernels, csrc/wideobs.hip)
        self.wide = obs_dim > 32
        self.Fld = 128 if self.wide else obs_dim      # floats between observation rows
        if obs_ld is not None and int(obs_ld) != self.Fld:   # rows wider than the features read (system.add_agent_id: False, envs.net_obs)
            if self.wide or int(obs_ld) < obs_dim:
                raise ValueError(f"obs_ld={obs_ld} with obs_dim={obs_dim}: a separate row stride is supported for narrow observations only")
            self.Fld = int(obs_ld)
        self.dev = device
        self.L = lib()
        self.G = wgrad_groups
        self.wt: Dict[str, torch.Tensor] = {}
        self.b = _Bufs(device)
        self._tabs: Dict[tuple, np.ndarray] = {}
        # weight-gradient GEMMs run on a side stream: they are off the critical path of the backward chain
        self.wgrad_stream = torch.cuda.Stream(device=device) if torch.device(device).type == "cuda" else None
        self.overlap_wgrad = False  # opt-in (bench.py --overlap): ~0.5 %, but per-kernel timings then include contention

    def _st(self):
        return torch.cuda.current_stream().cuda_stream

    def _tp(self, name, W, npad=None):
        K_, N_ = W.shape
        npad = npad or (N_ + 31) // 32 * 32
        t = self.wt.get(name)
        if t is None:
            t = torch.zeros(npad, K_, device=self.dev)
            self.wt[name] = t
        self.L.call("magpo_transpose_pad", W, t, K_, N_, npad, self._st())
        return t

    def lin(self, X, ldx, Wt, bias, Y, ldy, R, KIN, NOUT, act=0, mask=None):
        self.L.call("magpo_linear", X, ldx, Wt, bias, Y, ldy, mask, R, KIN, NOUT, act, getattr(self.tuning, self.LINEAR_VARIANT), self._st())

    def _groups(self, R):
        """Row slabs of a split weight gradient: no more than one per 256 rows (small minibatches: fewer partials to reduce)."""
        return max(1, min(self.G, R // 256))

    def _wgrad_side(self):
        """The stream weight gradients are queued on beside the backward chain, or None: on the calling stream."""
        return self.wgrad_stream if self.overlap_wgrad else None

    def wgrad(self, X, ldx, dY, ldy, R, KIN, NOUT, dW, db=None, krows=None):
        """dW = X^T dY.  With overlap_wgrad the GEMM is queued on the side stream behind everything the calling stream
        has queued so far (so X and dY are complete); the caller must not overwrite dY before its backward joins."""
        side = self._wgrad_side()
        if side is None:
            self.L.call("magpo_wgrad", X, ldx, dY, ldy, R, KIN, krows or KIN, NOUT, dW, db, self.wg_ws, self._groups(R), 1.0, 0, self.tuning.wgrad_variant, self._st())
            return
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.L.call("magpo_wgrad", X, ldx, dY, ldy, R, KIN, krows or KIN, NOUT, dW, db, self.wg_ws, self._groups(R), 1.0, 0, self.tuning.wgrad_variant, self._st())

    def _dense_bwd_fused(self, R, KIN, NOUT, act=0):
        """Whether ``dense_bwd`` serves this layer with the one-launch kernel: a shape magpo_dense_bwd takes, and a minibatch of at least
        ``tuning.dense_bwd_min_rows`` rows (below it the launch sequence is the pair's, unchanged)."""
        return KIN in (64, 128) and 1 <= NOUT <= 64 and act in (0, 4) and R >= self.tuning.dense_bwd_min_rows

    def dense_bwd(self, X, ldx, dY, ldy, W_nat, dX, lddx, R, KIN, NOUT, dW, db=None, act=0, mask=None, lin_W=None, lin_K=None):
        """Backward of a narrow dense layer: dW [KIN, NOUT] (+ db) = X^T dY and dX [R, KIN] = dY W_nat^T (act 4: masked by ``mask`` > 0, which
        may be X).  ``mask`` has dX's row stride ``lddx`` (magpo_linear's convention for act 4, which the pair below relies on; with
        mask = X that means ldx == lddx, and the kernel then reads the mask from its X tile).  One magpo_dense_bwd launch (csrc/linear.hip:
        k_dense_bwd) when the shape is one it serves and the minibatch has at least ``tuning.dense_bwd_min_rows`` rows; on the calling
        stream even with overlap_wgrad, because dX is on the critical path.  Otherwise the pair ``wgrad`` then ``lin``; ``lin_W`` /
        ``lin_K``: the weight image and contraction width of that GEMM where they are not W_nat / NOUT (a zero-padded copy)."""
        if self._dense_bwd_fused(R, KIN, NOUT, act):
            # with overlap_wgrad the side stream's weight gradients may still be folding their slabs out of wg_ws while this launch runs on
            # the calling stream: it then gets a slab workspace of its own (sized for the largest shape served, allocated on first use)
            ws = self.wg_ws if self._wgrad_side() is None else self.b.get("dense_ws", (self.L.call("magpo_wgrad_workspace_floats", 128, 64, self.G),))
            self.L.call("magpo_dense_bwd", X, ldx, dY, ldy, W_nat, mask, lddx if mask is not None else 0, dX, lddx, R, KIN, NOUT, dW, db,
                        ws, self._groups(R), act, self._st())
            return
        self.wgrad(X, ldx, dY, ldy, R, KIN, NOUT, dW, db)
        self.lin(dY, ldy, W_nat if lin_W is None else lin_W, None, dX, lddx, R, lin_K or NOUT, KIN, act=act, mask=mask)

    def _join_wgrad(self):
        """End of a backward: the calling stream waits for the weight gradients queued on the side stream."""
        if self.overlap_wgrad and self.wgrad_stream is not None:
            torch.cuda.current_stream().wait_stream(self.wgrad_stream)

    def reduce(self, slab, out, P=None, stride=None, accumulate=False):
        self.L.call("magpo_reduce_slabs", slab, out, slab.shape[0], P or slab.shape[1], stride or slab.shape[1], 1.0, 1 if accumulate else 0, self._st())

    def ptr_table(self, key, tensors) -> np.ndarray:
        """Host table (uint64) of the device pointers of ``tensors`` (None = NULL), cached under ``key``; ``tensors`` is the list, or a
        callable that builds it when the key is new.  The key must name every pointer in the table."""
        tab = self._tabs.get(key)
        if tab is None:
            if len(self._tabs) > self.MAX_TABLES:
                self._tabs.clear()
            tab = self._tabs[key] = np.array([0 if t is None else t.data_ptr() for t in (tensors() if callable(tensors) else tensors)],
                                             dtype=np.uint64)
        return tab


class TorsoNet(NetBase):
    """NetBase + the MLPTorso forward / backward (magpo_amd/torso.py) on the dense, LayerNorm and small-input kernels.  The network supplies
    ``v`` / ``gv`` (parameter and gradient views named by ``layer_name``) and the further transposed copies in ``wt`` (its ``refresh``).  For
    its ``pre`` torso (the one that reads observation rows) ``small_first`` and ``KP``: the first layer on narrow observations is served by the
    small-input kernels when it is Dense(F->128)+ReLU without LayerNorm; any other first layer reads the observations as a zero-padded
    [R][64] operand (magpo_small_operand) through magpo_linear / magpo_wgrad."""

    def _set_first_layer(self, spec) -> None:
        """``small_first`` / ``KP`` (columns of the first layer's padded operand) from the torso ``spec`` that reads the observation rows."""
        self.small_first = not self.wide and spec.layer_sizes[0] == 128 and spec.act(0) == 1 and not spec.use_layer_norm
        self.KP = 128 if self.wide else 64

    def _size_wgrad_ws(self, shapes) -> None:
        """The weight-gradient workspace for ``shapes``: every (KIN, NOUT) of a weight gradient of this network."""
        self.wg_ws = torch.empty(max(self.L.call("magpo_wgrad_workspace_floats", k, n, self.G) for k, n in shapes), device=self.dev)

    def _refresh_first_and_head(self, first_spec, head_in_width) -> None:
        """Derived copies at both ends: W_pre [F, D0] as [D0][KP] with zero columns beyond F (unless ``small_first``), and the head as
        [64][D] (forward) and [D][64] (natural, padded to 64 columns: dX of the head)."""
        v = self.v
        if not self.small_first:
            if "pre" not in self.wt:
                self.wt["pre"] = torch.zeros(first_spec.layer_sizes[0], self.KP, device=self.dev)
            self.wt["pre"][:, :self.F].copy_(v["pre.kernel"].t())
        ht = self._tp("head", v["head.kernel"], 64)
        self._tp("head_nat_pad", ht, head_in_width)

    def _torso_fwd(self, prefix, spec, X, ldx, R, ctx):
        """One MLPTorso (torsos.py:36-47) on R rows of X (stride ldx; the pre-torso's X are observation rows of F features).  Buffers are
        named by ``ctx`` so that the rollout, the carry and the training forward keep their own.  Returns one record per layer:
        (input, input stride, KIN, output y [R, width], (xhat, rstd) of the LayerNorm or None)."""
        L, st, v, b = self.L, self._st(), self.v, self.b
        recs = []
        kin = ldx if prefix == "post" else None
        for i, d in enumerate(spec.layer_sizes):
            n = layer_name(prefix, i)
            y = b.get(f"{ctx}{n}.y", (R, d))
            Wt = self.wt.get(n)
            if prefix == "pre" and i == 0:
                if self.small_first:
                    L.call("magpo_small_linear", X, ldx, self.F, v["pre.kernel"], v["pre.bias"], y, d, d, R, 1, st)
                    recs.append((X, ldx, None, y, None))
                    X, ldx, kin = y, d, d
                    continue
                if not self.wide:   # observation rows as a zero-padded [R][64] operand
                    xp = b.get(f"{ctx}pre.xp", (R, 64))
                    L.call("magpo_small_operand", 2, X, ldx, self.F, None, None, 0, xp, R, st)
                    X, ldx = xp, 64
                kin, Wt = self.KP, self.wt["pre"]
            if spec.use_layer_norm:
                z = b.get(f"{ctx}{n}.z", (R, d)); xh = b.get(f"{ctx}{n}.xh", (R, d)); rs = b.get(f"{ctx}{n}.rs", (R,))
                self.lin(X, ldx, Wt, v[n + ".bias"], z, d, R, kin, d)
                L.call("magpo_ln_act_fwd", z, d, v[n + ".ln.bias"], y, d, xh, d, rs, R, d, spec.act(i), st)
                recs.append((X, ldx, kin, y, (xh, rs)))
            else:
                self.lin(X, ldx, Wt, v[n + ".bias"], y, d, R, kin, d, act=spec.act(i))
                recs.append((X, ldx, kin, y, None))
            X, ldx, kin = y, d, d
        return recs

    def _torso_bwd(self, prefix, spec, recs, dy):
        """Backward through one torso.  ``dy`` = gradient at the last layer's output, already multiplied by that layer's activation
        derivative when the layer has no LayerNorm (the GEMM that produced it fused the mask: act 4 / 6).  Fills the layers' parameter
        gradients; returns the gradient at layer 0's pre-activation (the small first layer: at its output, unmasked)."""
        L, st, gv, v, b = self.L, self._st(), self.gv, self.v, self.b
        R = dy.shape[0]
        for i in range(len(spec.layer_sizes) - 1, -1, -1):
            n = layer_name(prefix, i)
            d = spec.layer_sizes[i]
            X, ldx, kin, y, ln = recs[i]
            if prefix == "pre" and i == 0 and self.small_first:
                return dy
            if ln is not None:   # LayerNorm + activation backward on the rows; the LayerNorm bias gradient from per-workgroup slabs
                dz = b.get(f"g_{prefix}{i}.dz", (R, d))
                grid = L.call("magpo_row_grid", R)
                slab = b.get(f"g_{prefix}{i}.slab", (grid, d))
                L.call("magpo_ln_act_bwd", dy, d, y, d, ln[0], d, ln[1], dz, d, slab, R, d, spec.act(i), st)
                self.reduce(slab, gv[n + ".ln.bias"])
            else:
                dz = dy
            krows = self.F if (prefix == "pre" and i == 0) else None
            self.wgrad(X, ldx, dz, d, R, kin, d, gv[n + ".kernel"], gv[n + ".bias"], krows=krows)
            if i == 0:
                return dz
            dy = b.get(f"g_{prefix}{i - 1}.dy", (R, spec.layer_sizes[i - 1]))
            self._dx(dz, d, v[n + ".kernel"], d, spec.layer_sizes[i - 1], R, dy, spec, i - 1, recs[i - 1])
        return dy

    def _dx(self, dsrc, ldsrc, W_nat, KIN, NOUT, R, dst, spec, j, rec):
        """dst = dsrc W^T (W in its natural [NOUT, KIN] layout), times the activation derivative of layer j of ``spec`` when that
        layer has no LayerNorm (fused epilogue: act 4 ReLU mask / act 6 tanh, its output as the mask argument)."""
        act, M = 0, None
        if rec[4] is None and spec.act(j):
            act, M = (4 if spec.act(j) == 1 else 6), rec[3]
        self.lin(dsrc, ldsrc, W_nat, None, dst, NOUT, R, KIN, NOUT, act=act, mask=M)

    def _small_first_wgrad(self, obs, emb0, d0, R):
        """Dense(F->128)+ReLU weight gradient on the raw observation rows: ``emb0`` the layer's output, ``d0`` the gradient there (unmasked)."""
        L, b, gv, F, Hh = self.L, self.b, self.gv, self.F, 128
        grid = L.call("magpo_row_grid", R)
        sw = b.get("g_slabw", (grid, 33 * Hh))
        L.call("magpo_small_relu_wgrad", obs, self.Fld, F, emb0, d0, sw, R, self._st())
        self.reduce(sw, gv["pre.kernel"], P=F * Hh, stride=33 * Hh)
        self.reduce(sw[:, 32 * Hh:], gv["pre.bias"], P=Hh, stride=33 * Hh)
