"""magpo_seg_post (tails 0-3) and magpo_seg_bwd (csrc/seg_fused.hip) against the fp64 references of tests/kernel_refs.py, at the row
counts where their 16-row tiles, shadow rows and grid-stride loops change behaviour, inside guarded buffers."""
import itertools

import numpy as np
import pytest
import torch

from tests import kernel_refs as kr
from tests.gpu_util import DEV, Guard, check_local, check_local_bwd, check_sum, dev, ptr_table, reduce_slabs

pytestmark = pytest.mark.gpu
E = 64
NPOS = 101
SMALL_R = (1, 15, 16, 17, 1000)
BIG_R = (16 * 1024 + 5, 3 * 16384 + 7)   # first grid-stride pass with a ragged last tile; three passes


@pytest.fixture(scope="module")
def pe(L, stream):
    t = torch.empty(NPOS, E, device=DEV)
    L.call("magpo_pe_table", t, NPOS, E, stream)
    return t.cpu()


def _wide(t, ld):
    """t [C, 64] as the last 64 columns of rows of ld floats (the g part of a q|k|v|g row)."""
    if ld == E:
        return dev(t)
    buf = torch.full((t.shape[0], ld), 1e30, device=DEV)
    buf[:, ld - E:] = t.to(DEV)
    return buf[:, ld - E:]


def run_seg_post(L, st, tail, c, K=20, given=True, ldg=E, ld0=None):
    """One magpo_seg_post call on the case dict; returns the guarded outputs by name.  given: the nullable outputs y / o / ope are passed."""
    R = c["r"].shape[0]
    keep = dict(r=dev(c["r"]), gp=_wide(c["gp"], ldg), gamma=dev(c["gamma"]), beta=dev(c["beta"]), wo_t=dev(c["wo"].T), res=dev(c["res"]),
                s1=dev(c["s1"]), s2=dev(c["s2"]), pe=dev(c["pe"]), pos=dev(c["pos"]), rows=dev(c.get("rows")))
    out = dict(u=Guard(R, E))
    if given:
        out.update(y=Guard(R, E), o=Guard(R, E), ope=Guard(R, E))
    q2w = c.get("q2w", []) if tail == 1 else []
    w0_t = b0 = hs = hw = hb1 = w1_t = b1 = None
    if tail in (1, 3):
        w0_t, b0, hs = dev(c["w0"].T), dev(c["b0"]), dev(c["hs"])
        out["out0"] = Guard(R, E, ld0 or E)
    if tail == 1:
        hw, hb1 = dev(c["hw"]), dev(c["hb1"])
        out["value"] = Guard(R, 1)
        for k in range(len(q2w)):
            out[f"q2_{k}"] = Guard(R, E)
    if tail == 2:
        w0_t = dev(c["w0"].T)
        out["out0"] = Guard(R, 3 * E, ld0 or 3 * E)
    if tail == 3:
        w1 = torch.zeros(E, E)
        w1[:K] = c["w1"].T
        w1_t, b1 = dev(w1), dev(c["b1"])
        out.update(hn=Guard(R, E), logits=Guard(R, E))
    q2_t = [dev(w.T) for w in q2w] + [None] * (4 - len(q2w))
    q2 = [out.get(f"q2_{k}") for k in range(4)]
    tab = [keep["r"], keep["gp"], keep["gamma"], keep["beta"], keep["wo_t"], keep["res"], keep["s1"], keep["s2"], keep["pe"], keep["pos"],
           out["u"], out.get("y"), out.get("o"), out.get("ope"), w0_t, b0, out.get("out0"), hs, hw, hb1, out.get("value"), *q2_t, *q2,
           out.get("hn"), w1_t, b1, out.get("logits"), keep["rows"]]
    ptrs = ptr_table(tab)
    dims = np.array([tail, K, NPOS, ldg, out["out0"].full.shape[1] if "out0" in out else 0, len(q2w)], dtype=np.int32)
    L.call("magpo_seg_post", dims.ctypes.data, R, ptrs.ctypes.data, int(ptrs.size), st)
    torch.cuda.synchronize()
    return out


def check_seg_post(L, st, tail, c, K=20, given=True, ldg=E, ld0=None, what=""):
    out = run_seg_post(L, st, tail, c, K, given, ldg, ld0)
    ref = kr.seg_post(tail, c)
    for name, g in out.items():
        g.check(f"{what} {name}")
        check_local(f"seg_post {what} {name}", g.out.reshape(ref[name].shape) if name == "value" else g.out, ref[name])
    if tail == 3:
        assert bool((out["logits"].out[:, K:] == 0).all()), "logit columns beyond K must be zero"
    return out


TAILS = [(0, 20, 0), (1, 20, 0), (1, 20, 1), (1, 20, 4), (2, 20, 0), (3, 1, 0), (3, 5, 0), (3, 31, 0), (3, 64, 0)]


@pytest.mark.parametrize("s2,rows,given", list(itertools.product((True, False), repeat=3)))
@pytest.mark.parametrize("tail,K,nq2", TAILS)
def test_seg_post(L, stream, pe, tail, K, nq2, s2, rows, given):
    """Every tail and every output it defines, with / without the second norm, the row table (gp / res tables of fewer rows, gp as the last
    64 columns of 256-float rows) and the nullable outputs, at 1, 15, 16, 17 and 1000 rows."""
    for R in SMALL_R:
        c = kr.seg_case(R, 1000 * tail + 10 * K + R, tail=tail, K=K, nq2=nq2, s2=s2, rows=rows, pe=pe)
        check_seg_post(L, stream, tail, c, K, given, ldg=256 if rows else E, ld0=(256 if tail == 2 else 128) if rows else None,
                       what=f"tail{tail} K{K} nq2={nq2} s2={s2} rows={rows} given={given} R={R}")


@pytest.mark.parametrize("R", BIG_R)
@pytest.mark.parametrize("tail,K,nq2,s2,rows", [(1, 20, 4, True, True), (3, 31, 0, False, False)])
def test_seg_post_grid_stride(L, stream, pe, tail, K, nq2, s2, rows, R):
    """More than 1024 16-row tiles: the prefetching grid-stride loop, its clamped look-ahead and the ragged last tile."""
    c = kr.seg_case(R, 77 + tail, tail=tail, K=K, nq2=nq2, s2=s2, rows=rows, pe=pe)
    check_seg_post(L, stream, tail, c, K, True, ldg=256 if rows else E, what=f"tail{tail} R={R}")


def test_seg_post_rejects_bad_arguments(L, stream, pe):
    c = kr.seg_case(16, 5, pe=pe)
    keep = [dev(c[n]) for n in ("r", "gp", "gamma", "beta")] + [dev(c["wo"].T), dev(c["res"]), dev(c["s1"]), dev(c["s2"]), dev(c["pe"]), dev(c["pos"])]
    u = Guard(16, E)
    ptrs = ptr_table(keep + [u] + [None] * 23)
    good = [0, 20, NPOS, E, 0, 0]
    for i, v in ((0, 4), (0, -1), (1, 0), (1, 65), (5, 5), (5, -1)):
        dims = np.array(good, dtype=np.int32)
        dims[i] = v
        with pytest.raises(ValueError):
            L.call("magpo_seg_post", dims.ctypes.data, 16, ptrs.ctypes.data, 34, stream)
    with pytest.raises(ValueError):
        L.call("magpo_seg_post", np.array(good, dtype=np.int32).ctypes.data, 16, ptrs.ctypes.data, 33, stream)
    with pytest.raises(ValueError):
        L.call("magpo_seg_bwd", 16, E, E, ptrs.ctypes.data, 20, stream)
    torch.cuda.synchronize()
    u.check("rejected calls write nothing", defined=torch.zeros(16, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------- backward
def run_seg_bwd(L, st, c, y=None, recompute=True, use_d1=True, use_d2=True, ldg=E, lddg=E):
    """One magpo_seg_bwd call + the four slab reductions.  y: device tensor [R, 64] (what seg_post wrote) or None; recompute: pass W_o^T."""
    R = c["r"].shape[0]
    G = L.call("magpo_seg_bwd_grid", R)
    assert G == min(1024, (R + 15) // 16)
    keep = dict(a=dev(c["res"]), s1=dev(c["s1"]), s2=dev(c["s2"]), d0=dev(c["d0"]), d1=dev(c["d1"]) if use_d1 else None,
                d2=dev(c["d2"]) if use_d2 else None, wo=dev(c["wo"]), r=dev(c["r"]), gp=_wide(c["gp"], ldg), gamma=dev(c["gamma"]),
                beta=dev(c["beta"]), rows=dev(c.get("rows")), wo_t=dev(c["wo"].T) if recompute else None)
    out = dict(dsum=Guard(R, E), dr=Guard(R, E), dgp=Guard(R, E, lddg), slab_s1=Guard(G, E), slab_ga=Guard(G, E), slab_be=Guard(G, E))
    if c["s2"] is not None:
        out["slab_s2"] = Guard(G, E)
    tab = [keep["a"], y, keep["s1"], keep["s2"], keep["d0"], keep["d1"], keep["d2"], keep["wo"], keep["r"], keep["gp"], keep["gamma"], keep["beta"],
           out["dsum"], out["dr"], out["dgp"], out["slab_s1"], out.get("slab_s2"), out["slab_ga"], out["slab_be"], keep["rows"], keep["wo_t"]]
    ptrs = ptr_table(tab)
    L.call("magpo_seg_bwd", R, ldg, lddg, ptrs.ctypes.data, int(ptrs.size), st)
    for n, red in (("slab_s1", "ds1"), ("slab_s2", "ds2"), ("slab_ga", "dgamma"), ("slab_be", "dbeta")):
        if n in out:
            out[red] = reduce_slabs(L, st, out[n], G, E, E)
    torch.cuda.synchronize()
    return out


def check_seg_bwd(out, c, use_d1=True, use_d2=True, presum=False, what=""):
    ref, r32 = kr.seg_bwd(c, torch.float64, use_d1, use_d2, presum), kr.seg_bwd(c, torch.float32, use_d1, use_d2, presum)
    for n in ("dsum", "dr", "dgp", "slab_s1", "slab_s2", "slab_ga", "slab_be"):
        if n in out:
            out[n].check(f"{what} {n}")
    for n in ("dsum", "dr", "dgp"):
        check_local_bwd(f"seg_bwd {what} {n}", out[n].out, ref[n])
    for n in ("ds1", "ds2", "dgamma", "dbeta"):
        if ref[n] is not None:
            check_sum(f"seg_bwd {what} {n}", out[n], ref[n], r32[n])


def _same_bits(a, b, what):
    for n in a:
        x, y = (a[n].out, b[n].out) if isinstance(a[n], Guard) else (a[n], b[n])
        assert torch.equal(x, y), f"{what}: {n} differs in {int((x != y).sum())} elements"


@pytest.mark.parametrize("s2,rows,dd", list(itertools.product((True, False), (True, False), ((True, True), (False, False), (True, False)))))
def test_seg_bwd(L, stream, pe, s2, rows, dd):
    """dsum, dr, dgp and the four reduced parameter-gradient rows against autograd of the fp64 forward, in the product's form (y recomputed
    from W_o^T) and given the y that seg_post wrote -- which the source claims are the same bits."""
    for R in SMALL_R:
        c = kr.seg_case(R, 4000 + R, s2=s2, rows=rows, pe=pe)
        ldg = 256 if rows else E
        what = f"s2={s2} rows={rows} d1,d2={dd} R={R}"
        y = run_seg_post(L, stream, 0, c, ldg=ldg)["y"].out.contiguous()
        rec = run_seg_bwd(L, stream, c, None, True, dd[0], dd[1], ldg, ldg)
        check_seg_bwd(rec, c, dd[0], dd[1], what=what)
        giv = run_seg_bwd(L, stream, c, y, False, dd[0], dd[1], ldg, ldg)
        check_seg_bwd(giv, c, dd[0], dd[1], what=what + " y given")
        _same_bits(rec, giv, f"recomputed y against stored y, {what}")


@pytest.mark.parametrize("R", (17, 1000))
def test_seg_bwd_presummed_input(L, stream, pe, R):
    """Neither y nor W_o^T: `a` already is the sum res + y (the third form the kernel's arguments allow)."""
    c = kr.seg_case(R, 4500 + R, pe=pe)
    y = run_seg_post(L, stream, 0, c)["y"].out.cpu()
    c2 = dict(c, res=c["res"] + y)
    check_seg_bwd(run_seg_bwd(L, stream, c2, None, False), c2, presum=True, what=f"presum R={R}")


@pytest.mark.parametrize("R", BIG_R)
@pytest.mark.parametrize("s2,rows", [(True, True), (False, False)])
def test_seg_bwd_grid_stride(L, stream, pe, s2, rows, R):
    """1024 waves walking more than 1024 tiles: per-wave sums over several tiles, shadow rows of the ragged last tile kept out of them."""
    c = kr.seg_case(R, 4700 + (R & 15), s2=s2, rows=rows, pe=pe)
    ldg = 256 if rows else E
    rec = run_seg_bwd(L, stream, c, None, True, True, False, ldg, ldg)
    check_seg_bwd(rec, c, True, False, what=f"s2={s2} rows={rows} R={R}")
    y = run_seg_post(L, stream, 0, c, ldg=ldg)["y"].out.contiguous()
    _same_bits(rec, run_seg_bwd(L, stream, c, y, False, True, False, ldg, ldg), f"recomputed y against stored y, R={R}")


@pytest.mark.parametrize("tail,nq2,R", [(0, 0, 1000), (1, 4, 1000), (2, 0, 17), (3, 0, 1000), (1, 1, BIG_R[0])])
def test_rows_table_equals_pregathered_call(L, stream, pe, tail, nq2, R):
    """With `rows` the kernels read gp / res through the table: the same bits as the call on inputs gathered beforehand."""
    c = kr.seg_case(R, 4900 + tail, tail=tail, K=20, nq2=nq2, rows=True, pe=pe)
    g = dict(c, gp=c["gp"][c["rows"].long()], res=c["res"][c["rows"].long()], rows=None)
    _same_bits(run_seg_post(L, stream, tail, c, ldg=256), run_seg_post(L, stream, tail, g), f"seg_post tail {tail}")
    _same_bits(run_seg_bwd(L, stream, c, ldg=256), run_seg_bwd(L, stream, g), "seg_bwd")
