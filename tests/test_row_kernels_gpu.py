"""Row kernels that only whole-learner runs reached: wide observations (csrc/wideobs.hip), the small first-layer helpers
(csrc/rowops.hip), the CoordSum class ids / tables (csrc/coordsum.hip) and the elementwise / row-copy helpers."""
import pytest
import torch

from tests import kernel_refs as kr
from tests.gpu_util import DEV, SENT, Guard, check_local, check_sum, dev, reduce_slabs

pytestmark = pytest.mark.gpu
D = torch.float64
NPOS = 101


# ------------------------------------------------------------------------------------------------ wide observations
GRID_CAP_R = 8 * 2048 * 2 + 13     # more than 2048 blocks of 8 rows: the grid stops growing, every block takes a third row group


def test_obsnorm_grid(L):
    for R in (1, 7, 8, 9, 5003, 8 * 2048, GRID_CAP_R, 10 * GRID_CAP_R):
        assert L.call("magpo_obsnorm_grid", R) == min(2048, (R + 7) // 8)


@pytest.mark.parametrize("ldo", [128, 160])
@pytest.mark.parametrize("F", [1, 33, 75, 127, 128])
def test_obsnorm_fwd_bwd(L, stream, F, ldo):
    """Rows of ldo floats with garbage behind the F features; `on` is NaN before the call: columns F..127 come back exactly zero.  The s_obs
    gradient is reduced the way the host does it (the first F columns of 128-wide slabs)."""
    for R in (1, 7, 8, 9, 5003, GRID_CAP_R):
        if R == GRID_CAP_R and (F, ldo) not in ((75, 160), (128, 128)):
            continue
        c = kr.obsnorm_case(R, F, ldo, 13 * F + ldo + R)
        what = f"F={F} ldo={ldo} R={R}"
        on = Guard(R, 128)
        L.call("magpo_obsnorm_fwd", dev(c["obs"]), ldo, F, dev(c["s_obs"]), on, R, stream)
        torch.cuda.synchronize()
        on.check(f"obsnorm_fwd {what}")
        check_local(f"obsnorm_fwd {what}", on.out, kr.obsnorm_fwd(c["obs"].to(D), F, c["s_obs"].to(D)))
        assert bool((on.out[:, F:] == 0).all()), f"{what}: columns F..127 must be exactly zero"
        G = L.call("magpo_obsnorm_grid", R)
        slab = Guard(G, 128)
        L.call("magpo_obsnorm_bwd", dev(c["obs"]), ldo, F, dev(c["don"]), slab, R, stream)
        ds = torch.full((128,), SENT, device=DEV)
        reduce_slabs(L, stream, slab, G, F, 128, ds)
        torch.cuda.synchronize()
        slab.check(f"obsnorm_bwd {what}")
        assert bool((ds[F:] == SENT).all())
        check_sum(f"obsnorm_bwd {what} ds_obs", ds[:F], kr.obsnorm_bwd(c["obs"].to(D), F, c["s_obs"].to(D), c["don"].to(D)),
                  kr.obsnorm_bwd(c["obs"], F, c["s_obs"], c["don"]))


def test_obsnorm_rejects_bad_arguments(L, stream):
    c = kr.obsnorm_case(8, 5, 128, 1)
    on = Guard(8, 128)
    for F, ldo in ((0, 128), (129, 160), (5, 124), (5, 130)):
        with pytest.raises(ValueError):
            L.call("magpo_obsnorm_fwd", dev(c["obs"]), ldo, F, dev(c["s_obs"]), on, 8, stream)
        with pytest.raises(ValueError):
            L.call("magpo_obsnorm_bwd", dev(c["obs"]), ldo, F, dev(c["don"]), on, 8, stream)
    torch.cuda.synchronize()
    on.check("rejected calls write nothing", defined=torch.zeros(8, dtype=torch.bool))


@pytest.mark.parametrize("pos_stride", [1, 3])
@pytest.mark.parametrize("E", [64, 128])
def test_add_pe(L, stream, E, pos_stride):
    """out = x + pe[clamp(pos)]: one fp32 addition per element, so bit-equal to the same expression; strided x / out / pos."""
    pe = torch.empty(NPOS, E, device=DEV)
    L.call("magpo_pe_table", pe, NPOS, E, stream)
    for R in (1, 63, 1000):
        g = torch.Generator().manual_seed(R + E)
        x = torch.randn(R, E + 8, generator=g).to(DEV)
        pos = torch.full((R, pos_stride), 10 ** 6, dtype=torch.int32)
        pos[:, 0] = torch.randint(-3, NPOS + 3, (R,), generator=g, dtype=torch.int32)
        out = Guard(R, E, E + 4)
        L.call("magpo_add_pe", x, E + 8, pe, dev(pos), pos_stride, NPOS, out, E + 4, R, E, stream)
        torch.cuda.synchronize()
        out.check(f"add_pe E={E} R={R}")
        assert torch.equal(out.out, x[:, :E] + pe[kr.clamp_pos(pos[:, 0], NPOS).to(DEV)])
    with pytest.raises(ValueError):
        L.call("magpo_add_pe", x, E + 8, pe, dev(pos), pos_stride, NPOS, out, E + 4, R, 96, stream)


# ------------------------------------------------------------------------------------------------ small first layers
@pytest.mark.parametrize("F", [1, 8, 9, 16, 17, 32])
def test_small_relu_wgrad(L, stream, F):
    """All three instances (F <= 8 / 16 / 32) on both sides of each seam; slabs [grid][33][128]: rows 0..F-1 = dW, row 32 = db (rows F..31
    are not the kernel's to write), reduced as the host reduces them."""
    for R in (1, 255, 5003, 16 * 2048 * 2 + 77):
        c = kr.small_relu_wgrad_case(R, F, F + 3, 50 * F + (R & 255))
        what = f"small_relu_wgrad F={F} R={R}"
        grid = L.call("magpo_row_grid", R)
        slab = Guard(grid, 33 * 128)
        L.call("magpo_small_relu_wgrad", dev(c["X"]), F + 3, F, dev(c["Yact"]), dev(c["dY"]), slab, R, stream)
        dW = reduce_slabs(L, stream, slab, grid, F * 128, 33 * 128)
        db = reduce_slabs(L, stream, slab.rows[:, 32 * 128:], grid, 128, 33 * 128)
        torch.cuda.synchronize()
        written = torch.zeros(grid, 33, 128, dtype=torch.bool)
        written[:, :F] = True
        written[:, 32] = True
        slab.check(what, defined=written.reshape(grid, 33 * 128))
        assert bool(torch.isnan(slab.out.reshape(grid, 33, 128)[:, F:32]).all()), f"{what}: slab rows F..31 are not written"
        (rW, rb), (fW, fb) = kr.small_relu_wgrad(c["X"].to(D), F, c["Yact"].to(D), c["dY"].to(D)), kr.small_relu_wgrad(c["X"], F, c["Yact"], c["dY"])
        check_sum(f"{what} dW", dW.reshape(F, 128), rW, fW)
        check_sum(f"{what} db", db, rb, fb)
    with pytest.raises(ValueError):
        L.call("magpo_small_relu_wgrad", dev(c["X"]), F + 3, 33, dev(c["Yact"]), dev(c["dY"]), slab, R, stream)
    with pytest.raises(ValueError):
        L.call("magpo_small_relu_wgrad", dev(c["X"]), F + 3, 0, dev(c["Yact"]), dev(c["dY"]), slab, R, stream)


@pytest.mark.parametrize("F", [1, 5, 33, 64])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_small_operand(L, stream, mode, F):
    """mode 2 (raw observations, the actor's first layer), 0 (normalised observations) and 1 (one-hot of an index): [R][64], zero beyond F."""
    for R in (1, 1000):
        g = torch.Generator().manual_seed(R + F + mode)
        obs = torch.full((R, F + 3), 1e30)
        obs[:, :F] = torch.randn(R, F, generator=g)
        s = 1 + 0.1 * torch.randn(F, generator=g)
        idx = torch.full((R, 2), 10 ** 6, dtype=torch.int32)
        idx[:, 0] = torch.randint(0, 64, (R,), generator=g, dtype=torch.int32)
        out = Guard(R, 64)
        L.call("magpo_small_operand", mode, dev(obs), F + 3, F, dev(s), dev(idx), 2, out, R, stream)
        torch.cuda.synchronize()
        out.check(f"small_operand mode={mode} F={F} R={R}")
        if mode == 0:
            check_local(f"small_operand mode 0 F={F} R={R}", out.out, kr.small_operand(0, obs.to(D), F, s.to(D)))
            assert bool((out.out[:, F:] == 0).all())
        else:
            assert torch.equal(out.out.cpu(), kr.small_operand(mode, obs, F, idx=idx[:, 0]))
    with pytest.raises(ValueError):
        L.call("magpo_small_operand", mode, dev(obs), F + 3, 65, dev(s), dev(idx), 2, out, R, stream)


# ------------------------------------------------------------------------------------------------ CoordSum input classes
@pytest.mark.parametrize("A,K,maxval,npos,N", [(4, 20, 60, 101, 333), (3, 10, 30, 7, 1), (8, 15, 100, 1, 515), (2, 3, 5, 4, 129)])
def test_coordsum_classes_and_class_rows(L, stream, A, K, maxval, npos, N):
    """Integer-exact against the header's formulas on tokens of the oracle env, and the defining property of the tables: looking a row's
    class up in them gives the row back (positions clamped), for every row."""
    obs, prev, pos = kr.coordsum_case(A, K, maxval, N, npos, 3 * A + N)
    R, F = obs.shape
    enc, dec = Guard(R, 1, dtype=torch.int32), Guard(R, 1, dtype=torch.int32)
    L.call("magpo_coordsum_classes", dev(obs), F, dev(prev), dev(pos), A, maxval, npos, enc, dec, R, stream)
    enc1 = Guard(R, 1, dtype=torch.int32)
    L.call("magpo_coordsum_classes", dev(obs), F, None, None, A, maxval, 1, enc1, None, R, stream)   # the actor's form
    Ce, Cd = A * maxval * npos, (K + 1) * npos
    obs_tab, pos_enc = Guard(Ce, F), Guard(Ce, 1, dtype=torch.int32)
    prev_dec, pos_dec = Guard(Cd, 1, dtype=torch.int32), Guard(Cd, 1, dtype=torch.int32)
    L.call("magpo_coordsum_class_rows", A, maxval, npos, K, obs_tab, pos_enc, prev_dec, pos_dec, stream)
    torch.cuda.synchronize()
    for n, g in dict(enc=enc, dec=dec, enc1=enc1, obs_tab=obs_tab, pos_enc=pos_enc, prev_dec=prev_dec, pos_dec=pos_dec).items():
        g.check(f"coordsum {n}")
    renc, rdec = kr.coordsum_classes(obs, prev, pos, A, maxval, npos)
    e, d = enc.out[:, 0].cpu().long(), dec.out[:, 0].cpu().long()
    assert torch.equal(e, renc) and torch.equal(d, rdec)
    assert torch.equal(enc1.out[:, 0].cpu().long(), kr.coordsum_classes(obs, None, None, A, maxval, 1)[0]) and torch.equal(enc1.out[:, 0].cpu().long(), e // npos)
    for got, ref in zip((obs_tab, pos_enc, prev_dec, pos_dec), kr.coordsum_class_rows(A, maxval, npos, K)):
        assert torch.equal(got.out.cpu().reshape(ref.shape).to(ref.dtype), ref)
    pc = kr.clamp_pos(pos, npos)
    assert torch.equal(obs_tab.out.cpu()[e], obs) and torch.equal(pos_enc.out.cpu()[e, 0].long(), pc)
    assert torch.equal(prev_dec.out.cpu()[d, 0], prev) and torch.equal(pos_dec.out.cpu()[d, 0].long(), pc)
    for badF in (A, A + 2):
        with pytest.raises(ValueError):
            L.call("magpo_coordsum_classes", dev(obs), badF, dev(prev), dev(pos), A, maxval, npos, enc, dec, R, stream)


# ------------------------------------------------------------------------------------------------ elementwise and row helpers
@pytest.mark.parametrize("n", [4, 1020, (1 << 20) + 4])
def test_relu_bwd_and_add_inplace(L, stream, n):
    """One fp32 operation per element: bit-equal to the same expression.  Both take whole float4s: n a multiple of 4."""
    g = torch.Generator().manual_seed(n)
    act, dy = torch.relu(torch.randn(n, generator=g)).to(DEV), torch.randn(n, generator=g).to(DEV)
    dx = Guard(n // 4, 4)
    L.call("magpo_relu_bwd", act, dy, dx, n, stream)
    torch.cuda.synchronize()
    dx.check("relu_bwd")
    ref = torch.where(act > 0, dy, torch.zeros_like(dy))
    assert torch.equal(dx.out.reshape(n), ref)
    inp = Guard(n // 4, 4)
    inp.rows.copy_(dy.reshape(n // 4, 4))
    L.call("magpo_relu_bwd", act, inp, inp, n, stream)   # in place
    torch.cuda.synchronize()
    inp.check("relu_bwd in place")
    assert torch.equal(inp.out.reshape(n), ref)
    dst = Guard(n // 4, 4)
    dst.rows.copy_(act.reshape(n // 4, 4))
    L.call("magpo_add_inplace", dst, dy, n, stream)
    torch.cuda.synchronize()
    dst.check("add_inplace")
    assert torch.equal(dst.out.reshape(n), act + dy)
    for bad in (n + 1, n + 2):
        with pytest.raises(ValueError):
            L.call("magpo_relu_bwd", act, dy, dx, bad, stream)
        with pytest.raises(ValueError):
            L.call("magpo_add_inplace", dst, dy, bad, stream)


@pytest.mark.parametrize("W", [4, 64, 128])
def test_add_rows(L, stream, W):
    for R in (1, 1000):
        g = torch.Generator().manual_seed(R + W)
        d0, src = torch.randn(R, W, generator=g).to(DEV), torch.full((R, W + 8), 1e30, device=DEV)
        src[:, :W] = torch.randn(R, W, generator=g).to(DEV)
        dst = Guard(R, W, W + 4)
        dst.rows[:, :W] = d0
        L.call("magpo_add_rows", dst, W + 4, src, W + 8, R, W, stream)
        torch.cuda.synchronize()
        dst.check(f"add_rows W={W} R={R}")
        assert torch.equal(dst.out, d0 + src[:, :W])
    for w, ldd, lds in ((W + 2, W + 4, W + 8), (W, W + 5, W + 8), (W, W + 4, W + 7), (0, W + 4, W + 8)):
        with pytest.raises(ValueError):
            L.call("magpo_add_rows", dst, ldd, src, lds, R, w, stream)


@pytest.mark.parametrize("W", [1, 5, 128, 256])
def test_copy_rows(L, stream, W):
    """Any width (scalar copies): a column block of wider rows into a column block of other rows."""
    for R in (1, 1000):
        g = torch.Generator().manual_seed(R + W)
        src = torch.randn(R, W + 7, generator=g).to(DEV)
        dst = Guard(R, W, W + 3)
        L.call("magpo_copy_rows", src[:, 2:], W + 7, dst, W + 3, R, W, stream)
        torch.cuda.synchronize()
        dst.check(f"copy_rows W={W} R={R}")
        assert torch.equal(dst.out, src[:, 2:2 + W])
