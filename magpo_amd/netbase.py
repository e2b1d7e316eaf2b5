"""Host-side plumbing shared by the two networks (SableGuider, GruActor): named workspaces, transposed weight copies, the dense-layer
and weight-gradient launches with the optional side stream, slab reductions and cached device-pointer tables."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ._lib import lib
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


class NetBase:
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
