"""Feed-forward actor and critic (FeedForwardActor / FeedForwardValueNet, mava/networks/base.py:38-88) on the MI355X kernels, and the paired
acting step of feed-forward PPO (ff_ippo / ff_mappo).

``FfActor``: MLPTorso -> Dense(K) logits (masked categorical head, heads.py:26-63).  ``FfCritic``: MLPTorso -> Dense(1, orthogonal(1.0)),
squeezed; ``centralised`` only changes what the rows ARE (``observation.global_state`` rows from ``magpo_global_state`` instead of
``agents_view`` rows).  These networks have one torso, ``network.{actor,critic}_network.pre_torso`` (magpo_amd/torso.py: 1-3 layers of width
64-256, relu / tanh, optional LayerNorm; the default is configs/network/mlp.yaml's [128, 128] relu).  Parameters live in one flat buffer
(params.ff_layout) with ``named`` / ``named_grads`` / ``load_named`` / ``refresh`` / ``bind_grads`` as GruActor has them, so ClipAdam, the
checkpointing and the ``_owner`` rule of get_learner_fn work unchanged.  ``apply`` is the training forward, ``bwd`` its hand-written backward;
both are the torso code GruActor uses (netbase.TorsoNet).

``act_pair`` is the acting step (ff_mappo.py:75-100): ONE ``magpo_mlp_act_step`` launch takes the observation rows through torso and head of both
networks with the activations in LDS (csrc/mlp_step.hip), then one categorical sample over the whole [N, A] batch.  With
``Tuning.ff_fused_step`` off (MAGPO_FF_FUSED_STEP=0) it is the composed chain of dense kernels per network.  The kernel has no LayerNorm: when
either network's torso has ``use_layer_norm`` the step takes the composed chain, silently.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .netbase import TorsoNet
from .params import ff_layout, init_ff, init_ff_from_key
from .torso import ACT_CODES, TorsoSpec, layer_name
from .tuning import Tuning

FF_DEFAULT_TORSO = TorsoSpec((128, 128))   # configs/network/mlp.yaml = the reference's mlp.yaml


class FfActor(TorsoNet):
    LINEAR_VARIANT = "actor_linear_variant"
    HEAD_PATH, HEAD_GAIN = ("action_head", "Dense_0"), 0.01   # flax path and orthogonal gain of the head (heads.py:53)

    def __init__(self, n_agents: int, action_dim: int, obs_dim: int, device, *, wgrad_groups: int = 512, seed=None,
                 grads: Optional[torch.Tensor] = None, tuning: Optional[Tuning] = None, obs_ld: Optional[int] = None, torso: Optional[TorsoSpec] = None):
        """``seed``: None (parameters are loaded later), an int (torch generator) or a PRNG key ([2] uint32: the parameters flax creates
        from actor_net_key / critic_net_key, params.init_ff_from_key, UNPINNED)."""
        if obs_dim > 128 or action_dim > 32:
            raise NotImplementedError("obs_dim <= 128 and action_dim <= 32 required")
        super().__init__(obs_dim, device, wgrad_groups, tuning, obs_ld)
        self.A, self.K = n_agents, action_dim
        self.spec = torso if torso is not None else FF_DEFAULT_TORSO
        self.D = self.spec.width
        self._set_first_layer(self.spec)
        self._bind_params(ff_layout(obs_dim, action_dim, self.spec), grads=grads)   # the layout's names are the reference's
        self._init_params(seed, lambda named, key: init_ff_from_key(named, key, self.HEAD_PATH, self.HEAD_GAIN),
                          lambda named, s: init_ff(named, s, self.HEAD_GAIN))
        shapes, din = [(self.D, self.K)], self.KP
        for d in self.spec.layer_sizes:
            shapes.append((din, d))
            din = d
        self._size_wgrad_ws(shapes)
        self.refresh()

    def _twin_kw(self):
        return dict(wgrad_groups=self.G, tuning=self.tuning, obs_ld=self.Fld, torso=self.spec)

    def twin(self):
        """A second network of the same class, shape, row stride and torso on the same device, sharing this one's ``Tuning`` object, with
        buffers of its own and uninitialised parameters (see GruActor.twin)."""
        return type(self)(self.A, self.K, self.F, self.dev, **self._twin_kw())

    def refresh(self):
        """Derived weight copies: the transposed layers of magpo_linear, which are also the images magpo_mlp_act_step reads."""
        for i in range(1, len(self.spec.layer_sizes)):
            self._tp(layer_name("pre", i), self.v[layer_name("pre", i) + ".kernel"])
        self._refresh_first_and_head(self.spec, self.D)

    # ------------------------------------------------------------------ composed forward (training, and acting with the fused step off)
    def _rows(self, obs) -> int:
        return obs.numel() // obs.shape[-1]

    def _fwd(self, obs, ctx: str):
        """Torso and head on the rows of ``obs`` (stride Fld) -> (layer records, logits [R, 64] with K valid columns)."""
        R = self._rows(obs)
        logits = self.b.get(ctx + "logits", (R, 64), zero=True)
        recs = self._torso_fwd("pre", self.spec, obs, self.Fld, R, ctx)
        self.lin(recs[-1][3], self.D, self.wt["head"], self.v["head.bias"], logits, 64, R, self.D, self.K)
        return recs, logits

    def apply(self, obs):
        """actor_network.apply (ff_mappo.py:131): raw logits [R, 64] (K valid columns) of the observation rows; its backward: ``bwd``."""
        recs, logits = self._fwd(obs, "t_")
        self._saved = dict(obs=obs, R=self._rows(obs), recs=recs)
        return logits

    def bwd(self, dlogits):
        """dlogits [R, 64] (columns >= K zero); fills self.grads."""
        sv, gv, D = self._saved, self.gv, self.D
        recs, R = sv["recs"], sv["R"]
        self.wgrad(recs[-1][3], D, dlogits, 64, R, D, self.K, gv["head.kernel"], gv["head.bias"])
        dy = self.b.get("g_dy", (R, D))
        # dy = dlogits @ W_head^T, masked by the last layer's activation (the small first layer applies its ReLU mask itself)
        if len(recs) == 1 and self.small_first:
            self.lin(dlogits, 64, self.wt["head_nat_pad"], None, dy, D, R, 64, D)
        else:
            self._dx(dlogits, 64, self.wt["head_nat_pad"], 64, D, R, dy, self.spec, len(recs) - 1, recs[-1])
        d0 = self._torso_bwd("pre", self.spec, recs, dy)
        if self.small_first:
            self._small_first_wgrad(sv["obs"], recs[0][3], d0, R)
        self._join_wgrad()

    # ------------------------------------------------------------------ acting
    def fusable(self) -> bool:
        """magpo_mlp_act_step covers this torso (it has no LayerNorm)."""
        return not self.spec.use_layer_norm

    def step_tables(self, X, Y, ldy: int):
        """This network's part of magpo_mlp_act_step's tables (include/magpo.h): (dims [10], tensors [10])."""
        s, v = self.spec, self.v
        w = list(s.layer_sizes) + [0] * (3 - len(s.layer_sizes))
        dims = [self.F, self.Fld, len(s.layer_sizes), *w, ACT_CODES[s.activation], int(s.activate_final), self.K, ldy]
        t = [X, v["pre.kernel"] if self.small_first else self.wt["pre"], v["pre.bias"]]
        for i in (1, 2):
            n = layer_name("pre", i)
            t += [self.wt[n], v[n + ".bias"]] if i < len(s.layer_sizes) else [None, None]
        return dims, t + [self.wt["head"], v["head.bias"], Y]

    def logits(self, obs, fused: Optional[bool] = None):
        """Acting forward on the rows of ``obs`` -> logits [R, 64] (a workspace of this object): one magpo_mlp_act_step launch, or the
        composed chain (``fused`` False, or a LayerNorm torso)."""
        fused = self.tuning.ff_fused_step if fused is None else fused
        if fused and self.fusable():
            out = self.b.get("s_logits", (self._rows(obs), 64), zero=True)
            mlp_act_step((self,), (obs,), (out,), (64,))
            return out
        return self._fwd(obs, "s_")[1]


class FfCritic(FfActor):
    """``apply`` / ``bwd`` / ``values`` over value rows: the one-column head of the actor's machinery."""
    HEAD_PATH, HEAD_GAIN = ("Dense_0",), 1.0     # the value head at the module's own scope, orthogonal(1.0) (base.py:86)

    def __init__(self, n_agents: int, obs_dim: int, device, *, centralised: bool = False, wgrad_groups: int = 512, seed=None,
                 grads: Optional[torch.Tensor] = None, tuning=None, obs_ld: Optional[int] = None, torso: Optional[TorsoSpec] = None):
        """``obs_dim`` / ``obs_ld``: features and row stride of the rows the network reads -- agents_view rows, or for ``centralised`` the
        global-state rows (num_agents * raw features, stride critic.global_state_ld)."""
        self.centralised = bool(centralised)
        super().__init__(n_agents, 1, obs_dim, device, wgrad_groups=wgrad_groups, seed=seed, grads=grads, tuning=tuning, obs_ld=obs_ld, torso=torso)

    def twin(self):
        return type(self)(self.A, self.F, self.dev, centralised=self.centralised, **self._twin_kw())

    def _values(self, logits, name):
        R = logits.shape[0]
        val = self.b.get(name, (R,))
        self.L.call("magpo_copy_rows", logits, 64, val, 1, R, 1, self._st())
        return val

    def apply(self, obs):
        """critic_network.apply (ff_mappo.py:160): the values [R] of the rows; its backward: ``bwd``."""
        return self._values(super().apply(obs), "t_value")

    def bwd(self, dvalue):
        """dvalue [R] = dL/dvalue; fills self.grads."""
        R = dvalue.shape[0]
        dl = self.b.get("g_dvalue_rows", (R, 64), zero=True)   # columns 1.. stay zero
        self.L.call("magpo_copy_rows", dvalue, 1, dl, 64, R, 1, self._st())
        super().bwd(dl)

    def values(self, obs, out: Optional[torch.Tensor] = None, fused: Optional[bool] = None):
        """Acting forward -> the values [R], into ``out`` (R floats) or a workspace of this object.  Fused: magpo_mlp_act_step with
        NOUT = 1, ldy = 1 writes the value vector directly."""
        R = self._rows(obs)
        fused = self.tuning.ff_fused_step if fused is None else fused
        if fused and self.fusable():
            val = self.b.get("s_value", (R,)) if out is None else out
            mlp_act_step((self,), (obs,), (val,), (1,))
            return val
        val = self._values(self._fwd(obs, "s_")[1], "s_value")
        if out is not None:
            out.view(-1).copy_(val)
        return val


def mlp_act_step(nets, xs, ys, ldys):
    """One ``magpo_mlp_act_step`` launch on the current stream: ys[k] = head_k(torso_k(xs[k])) for one or two FfActor / FfCritic objects.  The
    pointer table is cached under its pointers (NetBase.ptr_table), so a captured rollout has static arguments."""
    first = nets[0]
    R = first._rows(xs[0])
    dims, tab = [len(nets)], []
    for n, x, y, ldy in zip(nets, xs, ys, ldys):
        d, t = n.step_tables(x, y, ldy)
        dims += d
        tab += t
    ptrs = first.ptr_table(("mlp_step",) + tuple(0 if t is None else t.data_ptr() for t in tab), tab)
    dims = np.array(dims, dtype=np.int32)
    first.L.call("magpo_mlp_act_step", dims.ctypes.data, ptrs.ctypes.data, int(ptrs.size), R, first._st())


def act_pair(actor: FfActor, critic: FfCritic, obs_a, obs_c, *, key=None, key_dev=None, mask=None, action=None, log_prob=None, value=None,
             fused: Optional[bool] = None):
    """The acting step of feed-forward PPO for N envs (ff_mappo.py:75-100).  obs_a [N, A, F] actor rows, obs_c critic rows (agents_view, or
    global-state rows for a centralised critic).  Fused (default: actor.tuning.ff_fused_step, and no LayerNorm torso): ONE launch for both
    networks, the values written straight into ``value`` [N, A]; else the composed chain of each network.  Then ONE categorical sample over
    the whole [N, A] batch from ``key`` ([2] uint32 on the host) or ``key_dev`` (device, for a captured rollout) into action / log_prob
    [N, A].  Returns (logits [N * A, 64], values [N * A])."""
    R = actor._rows(obs_a)
    fused = actor.tuning.ff_fused_step if fused is None else fused
    if fused and actor.fusable() and critic.fusable():
        logits = actor.b.get("s_logits", (R, 64), zero=True)
        val = critic.b.get("s_value", (R,)) if value is None else value
        mlp_act_step((actor, critic), (obs_a, obs_c), (logits, val), (64, 1))
    else:
        logits = actor.logits(obs_a, fused=False)
        val = critic.values(obs_c, out=value, fused=False)
    if action is not None:
        k0, k1 = (0, 0) if key_dev is not None else (int(key[0]), int(key[1]))
        actor.L.call("magpo_sample_categorical", logits, 64, mask, 0 if mask is None else actor.K, k0, k1, key_dev, action, 1, log_prob, 1,
                     None, 0, None, 0, R, actor.K, actor._st())
    return logits, val
