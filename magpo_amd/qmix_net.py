"""QMIX's monotonic mixing network (QMixingNetwork, mava/networks/base.py:276-343) on the fused mixer kernels (csrc/qmix.hip).

One flat parameter buffer (``FlatParams``) with the reference's parameter paths as names; ``apply`` is ONE ``magpo_qmix_fwd`` launch, ``bwd``
one ``magpo_qmix_bwd`` launch plus the slab fold.  The global state is never built: the kernels read it from the team's observation rows
(the raw agent views behind the ``id_cols`` leading agent-id columns, the layout of ``magpo_global_state``).
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from ._lib import lib
from .netbase import ParamBinding
from .params import _orth, _orthogonal, _param_key

HYPER_HIDDEN = 64
EMBED_DIMS = (32, 64)
G_MAX = 128
# the entries in the order of the kernels' offset table (include/magpo.h)
ENTRIES = ("hyper_w1/Dense_0", "hyper_w1/Dense_1", "hyper_b1/Dense_0", "hyper_w2/Dense_0", "hyper_w2/Dense_1", "hyper_b2/Dense_0", "hyper_b2/Dense_1")


def mixer_layout(A: int, E: int, G: int) -> "OrderedDict[str, tuple]":
    s: "OrderedDict[str, tuple]" = OrderedDict()
    for name, (din, dout) in zip(ENTRIES, ((G, HYPER_HIDDEN), (HYPER_HIDDEN, A * E), (G, E), (G, HYPER_HIDDEN), (HYPER_HIDDEN, E), (G, E), (E, 1))):
        s[name + "/kernel"] = (din, dout)
        s[name + "/bias"] = (dout,)
    s["layer_norm/scale"] = (G,)
    s["layer_norm/bias"] = (G,)
    return s


def check_mixer_shape(A: int, E: int, G: int, hyper_hidden: int = HYPER_HIDDEN) -> None:
    """What the mixer kernels serve; anything else raises NotImplementedError."""
    if int(hyper_hidden) != HYPER_HIDDEN:
        raise NotImplementedError(f"QMIX mixer: hyper_hidden_dim = {HYPER_HIDDEN} only, got {hyper_hidden}")
    if int(E) not in EMBED_DIMS:
        raise NotImplementedError(f"QMIX mixer: qmix_embed_dim must be one of {EMBED_DIMS}, got {E}")
    if A < 1 or A * E > 512:
        raise NotImplementedError(f"QMIX mixer: num_agents * qmix_embed_dim = {A} * {E} exceeds 512")
    if G < 1 or G > G_MAX:
        raise NotImplementedError(f"QMIX mixer: the global state has {G} inputs; the kernels read at most {G_MAX}")


def _init_mixer(named: Dict[str, torch.Tensor], kernel) -> None:
    """Every Dense kernel from ``kernel(name, view)`` (orthogonal(sqrt 2)), zero biases, LayerNorm scale 1 / bias 0."""
    with torch.no_grad():
        for n, v in named.items():
            if n.endswith("/kernel"):
                v.copy_(kernel(n, v))
            else:
                v.fill_(1.0 if n == "layer_norm/scale" else 0.0)


def init_mixer_from_key(named: Dict[str, torch.Tensor], key: np.ndarray) -> None:
    """The QMixingNetwork parameters flax creates from ``key`` (rec_qmix.py:144-145), in the manner of params.init_actor_from_key: every
    Dense kernel from the key of its module path.  UNPINNED like the other initialisers."""
    _init_mixer(named, lambda n, v: torch.from_numpy(np.ascontiguousarray(
        _orth(_param_key(key, tuple(n.split("/")[:-1]), 1), tuple(v.shape), math.sqrt(2.0)))))


def init_mixer(named: Dict[str, torch.Tensor], seed: int) -> None:
    """The same distributions from a torch generator."""
    gen = torch.Generator().manual_seed(int(seed))
    _init_mixer(named, lambda n, v: _orthogonal(gen, tuple(v.shape), math.sqrt(2.0)))


class QMixer(ParamBinding):
    def __init__(self, n_agents: int, embed_dim: int, raw_features: int, device, *, id_cols: int = 0, norm_env_states: bool = True,
                 hyper_hidden: int = HYPER_HIDDEN, seed=None, grads: Optional[torch.Tensor] = None):
        """``raw_features``: width of one raw agent view (G = n_agents * raw_features state inputs); ``id_cols``: leading columns of every
        observation row the state skips.  ``seed``: a PRNG key (the parameters flax creates from it), an int (torch generator) or None."""
        A, E, G = int(n_agents), int(embed_dim), int(n_agents) * int(raw_features)
        check_mixer_shape(A, E, G, hyper_hidden)
        self.A, self.E, self.G, self.F_raw, self.id_cols, self.norm = A, E, G, int(raw_features), int(id_cols), bool(norm_env_states)
        self.dev, self.L = device, lib()
        self._bind_params(mixer_layout(A, E, G), grads=grads)   # the layout's names are the reference's parameter paths
        names = [e + s for e in ENTRIES for s in ("/kernel", "/bias")] + ["layer_norm/scale", "layer_norm/bias"]
        self.offs = np.array([self.P.offsets[n] for n in names], dtype=np.int64)
        self.SV = int(self.L.raw("magpo_qmix_save_floats")(E, G))
        self._buf: Dict[str, torch.Tensor] = {}
        self._saved = None
        self._init_params(seed, init_mixer_from_key, init_mixer)

    def refresh(self) -> None:
        """The kernels read the parameter buffer itself: nothing is derived from it."""

    def _st(self):
        return torch.cuda.current_stream().cuda_stream

    def _get(self, name, shape):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._buf[name] = torch.empty(*shape, dtype=torch.float32, device=self.dev)
        return t

    def _dims(self, Tm, Ts, t_off, mode, K):
        return np.array([self.A, self.E, self.G, self.F_raw, self.id_cols, int(self.norm), Tm, Ts, t_off, mode, K], dtype=np.int32)

    def apply(self, obs, obs_ld: int, R: int, q, *, q_online=None, index=None, mask=None, K: int = 0, ldq: int = 64, steps=(1, 1, 0), train: bool = False,
              out: Optional[torch.Tensor] = None, tag: str = ""):
        """q_tot [R] of R rows.  ``obs``: the teams' observation rows (stride obs_ld); ``steps`` = (Tm, Ts, t_off): row r is step r % Tm of
        sequence r / Tm and reads team (r / Tm) Ts + r % Tm + t_off.  ``q`` [R, A] (mode 0), or Q rows [teams A, ldq] with ``index`` [R, A] i32 (the
        taken actions: mode 1) or ``q_online`` rows (+ ``mask``) whose greedy action selects the column (double-Q: mode 2).  ``train`` saves
        what ``bwd`` needs."""
        mode = 0 if (index is None and q_online is None) else (1 if index is not None else 2)
        Tm, Ts, t_off = steps
        dims = self._dims(Tm, Ts, t_off, mode, K)
        q_tot = out if out is not None else self._get(tag + "q_tot", (R,))
        q_used = self._get(tag + "q_used", (R, self.A))
        save = self._get(tag + "save", (R, self.SV)) if train else None
        self.L.call("magpo_qmix_fwd", dims.ctypes.data, 11, self.P.flat, self.offs.ctypes.data, 16, obs, obs_ld, q, q_online, ldq, index, mask, q_tot, q_used,
                    save, R, self._st())
        if train:
            self._saved = dict(dims=dims, R=R, save=save, q_used=q_used, index=index)
        return q_tot

    def bwd(self, dq_tot, dq: Optional[torch.Tensor] = None, dq64: Optional[torch.Tensor] = None):
        """From dq_tot [R]: the parameter gradients into ``grads``; ``dq`` [R, A] and / or the scatter ``dq64`` (64-wide Q-gradient rows in the
        layout of the forward's Q rows: dq in the taken action's column, zero in the row's other columns)."""
        sv = self._saved
        R = sv["R"]
        nb = int(self.L.raw("magpo_qmix_bwd_grid")(R))
        slab = self._get("slab", (nb, self.P.numel))
        self.L.call("magpo_qmix_bwd", sv["dims"].ctypes.data, 11, self.P.flat, self.offs.ctypes.data, 16, self.P.numel, sv["save"], sv["q_used"], dq_tot, dq,
                    dq64, 64, sv["index"] if dq64 is not None else None, slab, self.grads, R, self._st())
