"""Helpers shared by the primitive-kernel GPU modules: guarded output buffers and printed, bounded comparisons."""
import numpy as np
import torch

from tests import kernel_refs as kr

DEV = "cuda"
PAD = 64            # guard rows before and after every output buffer
SENT = -777.0       # what the guard rows (and the columns between strided rows) hold
UNSET_INT = -123456789   # pre-fill of integer outputs (float outputs: NaN)


def dev(x):
    return None if x is None else x.to(DEV).contiguous()


class Guard:
    """An output buffer of R rows x W columns (row stride ld >= W) inside one allocation with PAD rows before and after it.  The owned
    block is pre-filled with NaN, everything else with the sentinel: after the call `check` wants no NaN left in the block and every
    other element unchanged.  All of it stays inside the allocation, so an overrun of up to PAD rows is seen, not suffered."""

    def __init__(self, R, W, ld=None, dtype=torch.float32, fill=None):
        ld = ld or W
        self.unset = fill is None
        if fill is None:
            fill = float("nan") if dtype.is_floating_point else UNSET_INT
        self.R, self.W = R, W
        self.full = torch.full((R + 2 * PAD, ld), SENT, device=DEV, dtype=dtype)
        self.rows = self.full[PAD:PAD + R]          # data_ptr() of this view = first owned row
        self.rows[:, :W] = fill

    def data_ptr(self):
        return self.rows.data_ptr()

    @property
    def out(self):
        return self.rows[:, :self.W]

    def check(self, what, defined=None):
        """defined: boolean mask [R] (or [R, W]) of the elements the call must have written; default all."""
        o = self.out
        if self.unset:
            nan = torch.isnan(o) if o.is_floating_point() else o == UNSET_INT
            if defined is not None:
                nan = nan & (defined if defined.dim() == 2 else defined[:, None]).to(DEV)
            assert not bool(nan.any()), f"{what}: {int(nan.sum())} elements of the output were never written"
        t = self.full.clone()
        t[PAD:PAD + self.R, :self.W] = SENT
        bad = t != SENT
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the owned block were overwritten"


def transpose_pad(L, st, W):
    """Wt [N padded to 32][K] = W[K][N]^T on the device, the weight layout of magpo_linear."""
    K, N = W.shape
    Np = (N + 31) // 32 * 32
    Wt = torch.empty(Np, K, device=DEV)
    L.call("magpo_transpose_pad", W, Wt, K, N, Np, st)
    return Wt


def ptr_table(tensors):
    return np.array([0 if t is None else t.data_ptr() for t in tensors], dtype=np.uint64)


def check(what, got, ref, bound):
    """Print the figure, then assert it: the whole output of a run is the measurement."""
    err = kr.max_err(got, ref)
    print(f"CHECK {what}: err {err:.3e} bound {bound:.3e} ref {ref.detach().abs().max().item():.3e}")
    assert err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e}"
    return err


def check_local(what, got, ref):
    return check(what, got, ref, kr.local_bound(ref))


def check_local_bwd(what, got, ref):
    return check(what, got, ref, kr.local_bound(ref, 1e-4, 1e-5))


def check_sum(what, got, ref64, ref32):
    """Sum over rows: max(project bound, 4 x the plain fp32 restatement's own error); prints reference error, kernel error and ratio."""
    e32 = kr.max_err(ref32, ref64)
    err = kr.max_err(got, ref64)
    bound = kr.sum_bound(ref64, ref32)
    print(f"SUMERR {what}: fp32-torch err {e32:.3e} kernel err {err:.3e} ratio {err / max(e32, 1e-300):.2f} bound {bound:.3e} "
          f"ref {ref64.abs().max().item():.3e}")
    assert err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e} (fp32 torch: {e32:.3e})"
    return err


def reduce_slabs(L, st, slab, G, P, stride, out=None):
    out = torch.empty(P, device=DEV) if out is None else out
    L.call("magpo_reduce_slabs", slab, out, G, P, stride, 1.0, 0, st)
    return out


def _count_calls(L, counts, fn):
    """Run fn() with every ABI call counted by name."""
    orig = L.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return orig(name, *a)
    L.call = counting
    try:
        return fn()
    finally:
        del L.call
