"""Recurrent critic (RecurrentValueNet, mava/networks/base.py:187-226) on the MI355X kernels, and the paired acting step of recurrent PPO.

pre-torso MLPTorso -> scanned GRU(128) with done-resets -> post-torso MLPTorso -> Dense(1, orthogonal(1.0)), squeezed.  The network is
``GruActor`` with a one-column head: the parameter layout is ``actor_layout(F, 128, 1, pre, post)``, the torsos follow
``network.critic_network.{pre_torso,post_torso}`` (magpo_amd/torso.py), the training scan and its hand-written backward are the actor's.
``centralised=True`` (rec_mappo.py:425-430) only changes what the rows ARE: the caller passes ``observation.global_state`` rows
(``magpo_global_state``: the raw views of all agents, tiled to every agent) instead of ``agents_view`` rows.

``step_pair`` is the acting step of rec_ippo / rec_mappo (rec_mappo.py:106-124): both pre-torsos, ONE ``magpo_gru_cell_step`` launch for the
two GRU cells (csrc/gru_step.hip; no xi buffer), both post-torsos and heads, one categorical sample over the whole [N, A] batch.  With
``Tuning.ppo_fused_step`` off it is the composed ``step`` of each network instead.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .actor import H, GruActor
from .params import _orth, _param_key, _trunc_normal
from .torso import TorsoSpec, layer_name

GS_MAX = 128   # inputs of the centralised critic: A * F_raw <= 128 (one padded row of the dense kernels)


def global_state_ld(n_agents: int, raw_features: int) -> int:
    """Row stride of the global-state rows ``magpo_global_state`` writes for this team: 64 for narrow rows (<= 32 features: the small-input
    kernels), else 128 (the padded rows of the MFMA first layer).  Raises for teams whose concatenated views do not fit."""
    F = int(n_agents) * int(raw_features)
    if F > GS_MAX:
        raise NotImplementedError(f"centralised critic: the global state has num_agents * raw features = {n_agents} * {raw_features} = {F} inputs; "
                                  f"the gfx950 first layer reads at most {GS_MAX} (rec_ippo has no such limit)")
    return 128 if F > 32 else 64


def init_critic_from_key(named, critic_net_key: np.ndarray) -> None:
    """The RecurrentValueNet parameters flax creates from ``critic_net_key`` (rec_mappo.py:465), in the manner of params.init_actor_from_key:
    pre_torso / post_torso Dense_<i> orthogonal(sqrt 2), ScannedRNN_0/GRUCell_0 (lecun-normal input kernels, orthogonal recurrent kernels),
    and the value head at the module's own scope, flax path ("Dense_0",), orthogonal(1.0) (base.py:224).  UNPINNED like the actor's
    (the samplers and flax's key derivation are restated from memory, oracle/prng.py)."""
    import math
    s2 = math.sqrt(2.0)
    key = lambda path, c: _param_key(critic_net_key, path, c)
    with torch.no_grad():
        def put(name, arr):
            named[name].copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(named[name].shape))
        for v in named.values():
            v.zero_()
        for prefix, scope in (("pre", "pre_torso"), ("post", "post_torso")):
            i = 0
            while layer_name(prefix, i) + ".kernel" in named:
                n = layer_name(prefix, i) + ".kernel"
                put(n, _orth(key((scope, f"Dense_{i}"), 1), tuple(named[n].shape), s2))
                i += 1
        D, Hh = named["gru.ir.kernel"].shape
        cell = ("ScannedRNN_0", "GRUCell_0")
        std = np.float32(np.sqrt(np.float32(1.0) / np.float32(D))) / np.float32(0.87962566103423978)
        for g in ("ir", "iz", "in"):
            put(f"gru.{g}.kernel", _trunc_normal(key(cell + (g,), 1), (D, Hh)) * std)
        for g in ("hr", "hz", "hn"):
            put(f"gru.{g}.kernel", _orth(key(cell + (g,), 1), (Hh, Hh), 1.0))
        put("head.kernel", _orth(key(("Dense_0",), 1), (named["head.kernel"].shape[0], 1), 1.0))


class GruCritic(GruActor):
    """``step`` / ``seq_fwd`` / ``seq_bwd`` over value rows: the one-column head of the actor's machinery.  ``named`` / ``named_grads`` /
    ``load_named`` / ``refresh`` / ``bind_grads`` are the actor's."""

    def __init__(self, n_agents: int, obs_dim: int, device, *, centralised: bool = False, hidden: int = 128, wgrad_groups: int = 512,
                 seed=None, grads: Optional[torch.Tensor] = None, tuning=None, obs_ld: Optional[int] = None,
                 pre_torso: Optional[TorsoSpec] = None, post_torso: Optional[TorsoSpec] = None):
        """``obs_dim`` / ``obs_ld``: features and row stride of the rows the network reads -- agents_view rows, or for ``centralised`` the
        global-state rows (num_agents * raw features, stride global_state_ld).  ``seed``: an int (torch generator) or critic_net_key."""
        self.centralised = bool(centralised)
        key = seed if isinstance(seed, np.ndarray) else None
        super().__init__(n_agents, 1, obs_dim, device, hidden=hidden, wgrad_groups=wgrad_groups, seed=None if key is not None else seed,
                         grads=grads, tuning=tuning, obs_ld=obs_ld, pre_torso=pre_torso, post_torso=post_torso)
        if key is not None:
            init_critic_from_key(self.named, key)
            self.refresh()
        elif seed is not None:   # Dense(1, orthogonal(1.0)): the actor's initialiser scales its head by 0.01
            with torch.no_grad():
                self.v["head.kernel"].mul_(100.0)
            self.refresh()

    def twin(self):
        return type(self)(self.A, self.F, self.dev, centralised=self.centralised, **self._twin_kw())

    def _values(self, logits, R, name):
        val = self.b.get(name, (R,))
        self.L.call("magpo_copy_rows", logits, 64, val, 1, R, 1, self._st())
        return val

    def step(self, obs, h_in, reset_env, h_out, want_value: bool = True, fused: Optional[bool] = None):
        """One step for N envs (rows as GruActor.step); returns the values [N * A] (a workspace of this object).  ``fused`` (default:
        tuning.ppo_fused_step): the GRU cell through magpo_gru_cell_step, else GruActor.step's composed chain."""
        if self.tuning.ppo_fused_step if fused is None else fused:
            R = obs.shape[0] * self.A
            emb = self.pre_torso(obs, self.Fld, R, "s_")[-1][3]
            gru_cell_step((self,), (emb,), (h_in,), reset_env, (h_out,), self.A)
            return self.head_values(h_out, R) if want_value else None
        logits = super().step(obs, h_in, reset_env, h_out, want_logits=want_value)
        return None if logits is None else self._values(logits, logits.shape[0], "s_value")

    def head_values(self, h, R):
        """Post-torso and value head on hidden states h [R, 128] -> values [R] (the tail of a step whose cell ran elsewhere)."""
        logits = self.b.get("s_logits", (R, 64), zero=True)
        self.post_torso_logits(h, R, "s_", logits)
        return self._values(logits, R, "s_value")

    def seq_fwd(self, obs, dones, h0, h0_idx, nseq: int, T: int, classes=None):
        """Arguments as GruActor.seq_fwd; returns the values [R]."""
        logits = super().seq_fwd(obs, dones, h0, h0_idx, nseq, T, classes=classes)
        return self._values(logits, logits.shape[0], "t_value")

    def seq_bwd(self, dvalue):
        """dvalue [R] = dL/dvalue; fills self.grads."""
        R = dvalue.shape[0]
        dl = self.b.get("g_dvalue_rows", (R, 64), zero=True)   # columns 1.. stay zero
        self.L.call("magpo_copy_rows", dvalue, 1, dl, 64, R, 1, self._st())
        super().seq_bwd(dl)


GruCritic.apply = GruCritic.seq_fwd   # critic_network.apply (rec_mappo.py:469): the scanned training forward (its backward: seq_bwd)


def gru_cell_step(nets, embs, h_ins, reset_env, h_outs, A: int):
    """One ``magpo_gru_cell_step`` launch for the GRU cells of ``nets`` (one or two GruActor / GruCritic objects) on the current stream:
    h_outs[k] = GRUCell_k(h_ins[k] zeroed where reset, embs[k]); embs[k] [R, D_pre of network k]."""
    first = nets[0]
    R = embs[0].shape[0]
    tab = []
    for n, e, hi, ho in zip(nets, embs, h_ins, h_outs):
        tab += [e, n.wt["wi"], n.v["gru.bi"], n.wt["wh"], n.v["gru.hn.bias"], hi, ho]
    ptrs = first.ptr_table(("cell_step",) + tuple(t.data_ptr() for t in tab), tab)
    dims = np.array([len(nets), nets[0].Dpre, nets[-1].Dpre], dtype=np.int32)
    first.L.call("magpo_gru_cell_step", dims.ctypes.data, ptrs.ctypes.data, int(ptrs.size), reset_env, R, A, first._st())


def step_pair(actor: GruActor, critic: GruCritic, obs_a, obs_c, reset_env, ha_in, ha_out, hc_in, hc_out, *, key=None, key_dev=None, mask=None,
              action=None, log_prob=None, value=None, fused: Optional[bool] = None):
    """The acting step of recurrent PPO for N envs (rec_mappo.py:106-124).  obs_a [N, A, F] actor rows, obs_c critic rows (agents_view, or
    global-state rows for a centralised critic), reset_env [N] u8, hidden states [N * A, 128] in / out per network.  In order, all on the
    current stream: both pre-torsos, one launch for both GRU cells, both post-torsos and heads, then ONE categorical sample over the whole
    [N, A] batch from ``key`` ([2] uint32 on the host) or ``key_dev`` (device, for a captured rollout) into action / log_prob [N, A];
    the values go to ``value`` [N, A].  ``fused`` (default: actor.tuning.ppo_fused_step) False = the composed ``step`` of each network.
    Returns (logits [N * A, 64], values [N * A])."""
    N, A = obs_a.shape[0], actor.A
    R = N * A
    fused = actor.tuning.ppo_fused_step if fused is None else fused
    if fused:
        emb_a = actor.pre_torso(obs_a, actor.Fld, R, "s_")[-1][3]
        emb_c = critic.pre_torso(obs_c, critic.Fld, R, "s_")[-1][3]
        gru_cell_step((actor, critic), (emb_a, emb_c), (ha_in, hc_in), reset_env, (ha_out, hc_out), A)
        logits = actor.b.get("s_logits", (R, 64), zero=True)
        actor.post_torso_logits(ha_out, R, "s_", logits)
        val = critic.head_values(hc_out, R)
    else:
        logits = actor.step(obs_a, ha_in, reset_env, ha_out, want_logits=True)
        val = critic.step(obs_c, hc_in, reset_env, hc_out, fused=False)
    if value is not None:
        value.view(-1).copy_(val)
    if action is not None:
        k0, k1 = (0, 0) if key_dev is not None else (int(key[0]), int(key[1]))
        actor.L.call("magpo_sample_categorical", logits, 64, mask, 0 if mask is None else actor.K, k0, k1, key_dev, action, 1, log_prob, 1,
                     None, 0, None, 0, R, actor.K, actor._st())
    return logits, val
