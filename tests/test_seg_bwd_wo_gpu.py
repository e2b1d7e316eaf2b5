"""The W_o weight gradient that magpo_seg_bwd forms itself (22-pointer table, slot 21 = per-workgroup [64 in][64 out] slabs of u^T dsum,
csrc/seg_fused.hip) against fp64 and against the three-launch path it replaces (magpo_seg_post writing u, magpo_seg_bwd with 21 pointers,
magpo_wgrad on u and dsum); and magpo_seg_post with u = NULL.

Bound of the fused dW_o: its max-abs error against fp64 may be at most twice that of the replaced path on the same inputs (another fp32
summation tree) plus 1e-7 max|dW_o|; a layout or masking mistake is an O(1) relative error."""
import functools

import numpy as np
import pytest
import torch

from tests import kernel_refs as kr
from tests import test_segment_kernels_gpu as sk
from tests.gpu_util import DEV, Guard, dev, ptr_table, reduce_slabs

pytestmark = pytest.mark.gpu
E = 64
ROWS = (1, 15, 16, 17, 1000, 16 * 1024 * 2 + 5)   # the last: every wave walks more than one tile, and the last tile is ragged
# the argument combinations SableGuider.train_bwd issues: (s2, d1, d2, row stride of gp and dgp)
SITES = dict(enc=(True, True, True, 256),        # encoder block: both norms, three incoming gradients, g of a q|k|v|g row
             dec1=(False, False, False, 256),    # decoder self-retention: one norm, one incoming gradient
             dec2=(True, False, False, 192),     # decoder cross-retention of the last block: g of a k|v|g row
             dec2mid=(True, True, False, 192))   # ... of an inner block (residual + projection paths)


@pytest.fixture(scope="module")
def pe(L, stream):
    t = torch.empty(sk.NPOS, E, device=DEV)
    L.call("magpo_pe_table", t, sk.NPOS, E, stream)
    return t.cpu()


def _seed(site, rows, R):
    return 9000 + 100 * list(SITES).index(site) + 50 * int(rows) + (R % 47)


@functools.lru_cache(maxsize=None)
def _reference(site, rows, R):
    """(case, fp64 dW_o = u^T dsum): u by GroupNorm + swish, dsum by the backward of the RMSNorm chain, on the case's own fp32 inputs."""
    s2, d1, d2, _ = SITES[site]
    c = kr.seg_case(R, _seed(site, rows, R), s2=s2, rows=rows)
    g = lambda n: c[n].double()
    gp = g("gp")[c["rows"].long()] if rows else g("gp")
    u = kr.onets.swish(gp) * kr.onets.groupnorm_rows(g("r"), g("gamma"), g("beta"), 1)
    dsum = kr.seg_bwd(c, torch.float64, d1, d2)["dsum"]
    return c, u.T @ dsum


def run_fused(L, st, c, use_d1, use_d2, ld, with_slab=True, nptrs=22):
    """One magpo_seg_bwd call with the 22-pointer table + the slab reductions; dW_o is the reduced slab."""
    R = c["r"].shape[0]
    G = L.call("magpo_seg_bwd_grid", R)
    keep = [dev(c["res"]), None, dev(c["s1"]), dev(c["s2"]), dev(c["d0"]), dev(c["d1"]) if use_d1 else None, dev(c["d2"]) if use_d2 else None,
            dev(c["wo"]), dev(c["r"]), sk._wide(c["gp"], ld), dev(c["gamma"]), dev(c["beta"])]
    out = dict(dsum=Guard(R, E), dr=Guard(R, E), dgp=Guard(R, E, ld), slab_s1=Guard(G, E), slab_ga=Guard(G, E), slab_be=Guard(G, E))
    if c["s2"] is not None:
        out["slab_s2"] = Guard(G, E)
    if with_slab:
        out["slab_wo"] = Guard(G, E * E)
    tail = [dev(c.get("rows")), dev(c["wo"].T.contiguous())]
    tab = keep + [out["dsum"], out["dr"], out["dgp"], out["slab_s1"], out.get("slab_s2"), out["slab_ga"], out["slab_be"]] + tail + [out.get("slab_wo")]
    ptrs = ptr_table(tab[:nptrs])
    L.call("magpo_seg_bwd", R, ld, ld, ptrs.ctypes.data, int(ptrs.size), st)
    for n, red in (("slab_s1", "ds1"), ("slab_s2", "ds2"), ("slab_ga", "dgamma"), ("slab_be", "dbeta")):
        if n in out:
            out[red] = reduce_slabs(L, st, out[n], G, E, E)
    if with_slab:
        out["dwo"] = reduce_slabs(L, st, out["slab_wo"], G, E * E, E * E).reshape(E, E)
    torch.cuda.synchronize()
    return out


def run_replaced(L, st, c, use_d1, use_d2, ld):
    """The path the fused gradient replaces: seg_post writes u, seg_bwd (21 pointers) writes dsum, magpo_wgrad multiplies them."""
    R = c["r"].shape[0]
    u = sk.run_seg_post(L, st, 0, c, ldg=ld)["u"].out.contiguous()
    out = sk.run_seg_bwd(L, st, c, None, True, use_d1, use_d2, ld, ld)
    G = max(1, min(512, R // 256))   # SableGuider._groups at the default wgrad_groups
    ws = torch.empty(L.call("magpo_wgrad_workspace_floats", E, E, G), device=DEV)
    dW = torch.full((E, E), float("nan"), device=DEV)
    L.call("magpo_wgrad", u, E, out["dsum"].out.contiguous(), E, R, E, E, E, dW, None, ws, G, 1.0, 0, 0, st)
    torch.cuda.synchronize()
    out["dwo"] = dW
    return out


_runs = {}


def runs(L, st, site, rows, R):
    """Every launch the tests of one case look at, made once: replaced path, 21-pointer call, 22-pointer call twice."""
    key = (site, rows, R)
    if key not in _runs:
        c, _ = _reference(site, rows, R)
        _, d1, d2, ld = SITES[site]
        _runs[key] = dict(old=run_replaced(L, st, c, d1, d2, ld), new=run_fused(L, st, c, d1, d2, ld), again=run_fused(L, st, c, d1, d2, ld))
    return _runs[key]


CASES = [(site, rows, R) for site in ("enc", "dec1", "dec2") for rows in (False, True) for R in ROWS] + [("dec2mid", False, 1000), ("dec2mid", True, ROWS[-1])]


@pytest.mark.parametrize("site,rows,R", CASES)
def test_dwo_against_fp64_and_replaced_path(L, stream, site, rows, R):
    _, ref = _reference(site, rows, R)
    rr = runs(L, stream, site, rows, R)
    rr["new"]["slab_wo"].check(f"{site} rows={rows} R={R} slab_wo")
    e_old, e_new = kr.max_err(rr["old"]["dwo"], ref), kr.max_err(rr["new"]["dwo"], ref)
    bound = 2.0 * e_old + 1e-7 * ref.abs().max().item()
    print(f"DWO {site} rows={rows} R={R}: replaced-path err {e_old:.3e} fused err {e_new:.3e} bound {bound:.3e} max|dW| {ref.abs().max().item():.3e}")
    assert e_new <= bound, f"fused dW_o error {e_new:.3e} > 2 x {e_old:.3e} + 1e-7 x {ref.abs().max().item():.3e}"


@pytest.mark.parametrize("site,rows,R", CASES)
def test_other_outputs_same_bits_as_21_pointer_call(L, stream, site, rows, R):
    """Both calls are kernels of this build that read W_o from its LDS image, so this shows that forming dW_o disturbs nothing else -- not that
    the image gives the register path's bits: that is test_segment_kernels_gpu's recomputed-against-stored-y comparison (y given = register path)."""
    rr = runs(L, stream, site, rows, R)
    for n in ("dsum", "dr", "dgp", "slab_s1", "slab_s2", "slab_ga", "slab_be"):
        if n in rr["old"]:
            rr["new"][n].check(f"{site} rows={rows} R={R} {n}")
            x, y = rr["new"][n].out, rr["old"][n].out
            assert torch.equal(x, y), f"{n} differs from the 21-pointer call in {int((x != y).sum())} elements"


@pytest.mark.parametrize("site,rows,R", CASES)
def test_two_launches_same_bits(L, stream, site, rows, R):
    rr = runs(L, stream, site, rows, R)
    assert torch.equal(rr["new"]["slab_wo"].out, rr["again"]["slab_wo"].out), "slabs differ between two launches"
    assert torch.equal(rr["new"]["dwo"], rr["again"]["dwo"]), "reduced dW_o differs between two launches"


def test_null_slab_equals_21_pointer_call(L, stream):
    """Slot 21 present but NULL is the 21-pointer call."""
    c, _ = _reference("enc", True, 1000)
    a, b = run_fused(L, stream, c, True, True, 256, with_slab=False), run_fused(L, stream, c, True, True, 256, with_slab=False, nptrs=21)
    for n in a:
        x, y = (a[n].out, b[n].out) if isinstance(a[n], Guard) else (a[n], b[n])
        assert torch.equal(x, y), n


def test_rejects_bad_tables(L, stream):
    c, _ = _reference("enc", False, 16)
    keep = [dev(c["res"]), None, dev(c["s1"]), dev(c["s2"]), dev(c["d0"]), None, None, dev(c["wo"]), dev(c["r"]), dev(c["gp"]), dev(c["gamma"]), dev(c["beta"])]
    outs = [Guard(16, E) for _ in range(3)] + [Guard(1, E) for _ in range(4)]
    slab = Guard(1, E * E)
    wo_t = dev(c["wo"].T.contiguous())
    full = keep + outs + [None, wo_t, slab, None]
    for n in (20, 23):
        with pytest.raises(ValueError):
            L.call("magpo_seg_bwd", 16, E, E, ptr_table(full).ctypes.data, n, stream)
    no_wot = ptr_table(keep + outs + [None, None, slab])
    with pytest.raises(ValueError):
        L.call("magpo_seg_bwd", 16, E, E, no_wot.ctypes.data, 22, stream)
    torch.cuda.synchronize()
    for g in outs + [slab]:
        g.check("rejected calls write nothing", defined=torch.zeros(g.R, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------- seg_post without u
def _post(L, st, tail, c, K, with_u, ldg):
    """magpo_seg_post with every output of the tail given; u given or NULL."""
    R = c["r"].shape[0]
    keep = [dev(c["r"]), sk._wide(c["gp"], ldg), dev(c["gamma"]), dev(c["beta"]), dev(c["wo"].T.contiguous()), dev(c["res"]), dev(c["s1"]), dev(c["s2"]),
            dev(c["pe"]), dev(c["pos"])]
    out = dict(y=Guard(R, E), o=Guard(R, E), ope=Guard(R, E))
    if with_u:
        out["u"] = Guard(R, E)
    q2w = c.get("q2w", []) if tail == 1 else []
    w0_t = b0 = hs = hw = hb1 = w1_t = b1 = None
    if tail in (1, 3):
        w0_t, b0, hs = dev(c["w0"].T.contiguous()), dev(c["b0"]), dev(c["hs"])
        out["out0"] = Guard(R, E)
    if tail == 1:
        hw, hb1 = dev(c["hw"]), dev(c["hb1"])
        out["value"] = Guard(R, 1)
        for k in range(len(q2w)):
            out[f"q2_{k}"] = Guard(R, E)
    if tail == 2:
        w0_t = dev(c["w0"].T.contiguous())
        out["out0"] = Guard(R, 3 * E)
    if tail == 3:
        w1 = torch.zeros(E, E)
        w1[:K] = c["w1"].T
        w1_t, b1 = dev(w1), dev(c["b1"])
        out.update(hn=Guard(R, E), logits=Guard(R, E))
    q2_t = [dev(w.T.contiguous()) for w in q2w] + [None] * (4 - len(q2w))
    tab = keep + [out.get("u"), out["y"], out["o"], out["ope"], w0_t, b0, out.get("out0"), hs, hw, hb1, out.get("value"), *q2_t,
                  *[out.get(f"q2_{k}") for k in range(4)], out.get("hn"), w1_t, b1, out.get("logits"), dev(c.get("rows"))]
    ptrs = ptr_table(tab)
    dims = np.array([tail, K, sk.NPOS, ldg, out["out0"].full.shape[1] if "out0" in out else 0, len(q2w)], dtype=np.int32)
    L.call("magpo_seg_post", dims.ctypes.data, R, ptrs.ctypes.data, int(ptrs.size), st)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("tail,nq2,rows", [(1, 2, True), (2, 0, False), (3, 0, False), (0, 0, True)])
def test_seg_post_without_u_same_bits(L, stream, pe, tail, nq2, rows):
    for R in (1, 17, 1000, 16 * 1024 + 5):
        c = kr.seg_case(R, 9900 + 10 * tail + (R % 7), tail=tail, K=20, nq2=nq2, rows=rows, pe=pe)
        ldg = 256 if rows else E
        a, b = _post(L, stream, tail, c, 20, True, ldg), _post(L, stream, tail, c, 20, False, ldg)
        for n, g in b.items():
            g.check(f"tail {tail} R={R} {n} (u = NULL)")
            assert torch.equal(g.out, a[n].out), f"tail {tail} R={R}: {n} differs when u is not stored"
