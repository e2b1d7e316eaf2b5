"""The Multi-Agent Transformer's row kernels (csrc/rowops.hip: magpo_resln_fwd / _bwd, magpo_gelu_bwd) against fp64 autograd of the
restatement (tests/mat_ref.py: flax LayerNorm with scale and bias, epsilon 1e-6, mat_network.py:65-66, 80, 85, 99).

Accuracy bar, per case and per output (tests/test_team_attention_gpu.py's): max error against fp64 <= max(2 x the error of the same
formula evaluated by torch in fp32 on the CPU on the same inputs, 2^-24 x max|reference|).  Every case prints one MATROWS line; one run's
lines are kept as profiles/mat_rows_errors.txt."""
import pytest
import torch

from tests import mat_ref as mr
from tests.gpu_util import DEV, Guard, reduce_slabs

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
ROWS = (1, 63, 64, 257)   # one row; the last row block short by one row, exactly full, and one row into the 17th workgroup


@pytest.fixture(scope="module")
def L():
    from magpo_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def err(a, ref):
    return (a.double() - ref.double()).abs().max().item()


def reference(a, y, scale, bias, dout, nf, act, dt):
    """(out, d(a + y) or dy, dscale, dbias) in ``dt``; statistics over the first nf columns, the columns beyond leave as bias."""
    a, y, scale, bias, dout = (None if t is None else t.to(dt) for t in (a, y, scale, bias, dout))
    y = y.clone().requires_grad_(True)
    scale, bias = scale.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    E = y.shape[1]
    head = mr.resln(None if a is None else a[:, :nf], y[:, :nf], scale[:nf], bias[:nf], act)
    out = torch.cat([head, bias[nf:].expand(y.shape[0], E - nf)], dim=1)
    dy, ds, db = torch.autograd.grad((out * dout).sum(), [y, scale, bias])
    return out.detach(), dy, ds, db


def strided(t, ld, fill=5.0e3):
    """Rows of t inside a wider device buffer of row stride ld."""
    buf = torch.full((t.shape[0], ld), fill, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def run_case(L, R, E, nf, act, with_a, tag):
    g = torch.Generator().manual_seed(97 * R + E + 7 * nf + act + (1 if with_a else 0))
    y, dout = torch.randn(R, E, generator=g) * 1.5 + 0.3, torch.randn(R, E, generator=g)
    a = torch.randn(R, E, generator=g) if with_a else None
    scale, bias = 1.0 + 0.3 * torch.randn(E, generator=g), 0.3 * torch.randn(E, generator=g)
    if nf < E:   # a zero-padded row: nothing but zeros (and no scale) beyond the nf features
        y[:, nf:] = 0.0
        scale[nf:] = 0.0
        if a is not None:
            a[:, nf:] = 0.0
    w64 = reference(a, y, scale, bias, dout, nf, act, torch.float64)
    w32 = reference(a, y, scale, bias, dout, nf, act, torch.float32)
    ad, yd, dd = (None if a is None else strided(a, E + 8)), strided(y, E + 4), strided(dout, E + 12)
    sd, bd = scale.to(DEV), bias.to(DEV)
    out, dsum = Guard(R, E, E + 4), Guard(R, E, E + 8)
    L.call("magpo_resln_fwd", ad, E + 8 if with_a else 0, yd, E + 4, sd, bd, out, E + 4, R, E, nf, act, st())
    grid = L.call("magpo_row_grid", R)
    bits = []
    for _ in range(2):   # the slab fold is deterministic: two runs give the same bits
        ss, sb = Guard(grid, E), Guard(grid, E)
        L.call("magpo_resln_bwd", ad, E + 8 if with_a else 0, yd, E + 4, sd, dd, E + 12, None, 0, dsum, E + 8, ss, sb, R, E, nf, act, st())
        ds, db = reduce_slabs(L, st(), ss, grid, E, E), reduce_slabs(L, st(), sb, grid, E, E)
        torch.cuda.synchronize()
        for n, gd in (("out", out), ("dsum", dsum), ("slab_scale", ss), ("slab_bias", sb)):
            gd.check(f"{n} {tag}")
        bits.append((dsum.out.clone(), ds.clone(), db.clone()))
    assert all(torch.equal(x, z) for x, z in zip(*bits)), f"{tag}: two backward runs differ"
    got = (out.out.cpu(), dsum.out.cpu(), ds.cpu(), db.cpu())
    figs, bad = [], []
    for n, gt, w, f in zip(("out", "dsum", "dscale", "dbias"), got, w64, w32):
        if nf < E and n == "dscale":
            gt, w, f = gt[:nf], w[:nf], f[:nf]   # (the scale of a padding column multiplies xhat = 0: its gradient is 0 either way)
        e, e32 = err(gt, w), err(f, w)
        bound = max(2.0 * e32, U24 * w.abs().max().item())
        figs.append(f"{n} {e:.3e}/{e32:.3e}/{bound:.3e}")
        if not e <= bound:
            bad.append(n)
    print(f"MATROWS {tag}: err/fp32-torch-err/bound " + " ".join(figs))
    assert not bad, f"{tag}: {bad} above the bar ({figs})"


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("R", ROWS)
def test_resln_against_fp64(L, R, with_a):
    """out = LayerNorm(a + y) * scale + bias on strided rows of 64 floats, with and without a."""
    run_case(L, R, 64, 64, 0, with_a, f"resln R={R} a={int(with_a)}")


@pytest.mark.parametrize("R,E,nf,act", [(63, 64, 64, 2), (257, 64, 64, 2), (257, 64, 4, 0), (63, 64, 23, 0), (257, 128, 71, 0), (64, 128, 128, 0)])
def test_resln_variants_against_fp64(L, R, E, nf, act):
    """act 2: LayerNorm(gelu(y)) (the heads and the embeddings); nf < E: the observation encoder's LayerNorm over nf raw features inside a
    zero-padded row of 64 or 128 floats."""
    run_case(L, R, E, nf, act, False, f"resln R={R} E={E} nf={nf} act={act}")


def test_resln_adds_the_second_gradient(L):
    """d0 + d1 is the incoming gradient: the same bits as one buffer holding their fp32 sum."""
    R, E = 63, 64
    g = torch.Generator().manual_seed(5)
    y, d0, d1 = (torch.randn(R, E, generator=g).to(DEV) for _ in range(3))
    scale = (1.0 + 0.3 * torch.randn(E, generator=g)).to(DEV)
    grid = L.call("magpo_row_grid", R)
    outs = []
    for da, db in ((d0, d1), (d0 + d1, None)):
        dsum, ss, sb = Guard(R, E), Guard(grid, E), Guard(grid, E)
        L.call("magpo_resln_bwd", None, 0, y, E, scale, da, E, db, 0 if db is None else E, dsum, E, ss, sb, R, E, E, 0, st())
        torch.cuda.synchronize()
        outs.append((dsum.out.clone(), ss.out.clone(), sb.out.clone()))
    assert all(torch.equal(x, z) for x, z in zip(*outs))


@pytest.mark.parametrize("R,E", [(1, 64), (63, 64), (257, 64), (64, 128)])
def test_gelu_bwd_against_fp64(L, R, E):
    g = torch.Generator().manual_seed(R + E)
    z, dy = torch.randn(R, E, generator=g) * 2.0, torch.randn(R, E, generator=g)
    want = {}
    for dt in (torch.float64, torch.float32):
        zz = z.to(dt).requires_grad_(True)
        want[dt], = torch.autograd.grad((torch.nn.functional.gelu(zz, approximate="tanh") * dy.to(dt)).sum(), [zz])
    dz = Guard(R, E, E + 4)
    L.call("magpo_gelu_bwd", strided(z, E + 8), E + 8, strided(dy, E + 4), E + 4, dz, E + 4, R, E, st())
    torch.cuda.synchronize()
    dz.check(f"gelu_bwd R{R} E{E}")
    e, e32 = err(dz.out.cpu(), want[torch.float64]), err(want[torch.float32], want[torch.float64])
    bound = max(2.0 * e32, U24 * want[torch.float64].abs().max().item())
    print(f"MATROWS gelu_bwd R={R} E={E}: err/fp32-torch-err/bound dz {e:.3e}/{e32:.3e}/{bound:.3e}")
    assert e <= bound


def test_entry_points_reject_bad_arguments(L):
    b, s = torch.zeros(16, 64, device=DEV), torch.ones(64, device=DEV)
    ok_f = [b, 64, b, 64, s, s, b, 64, 16, 64, 64, 0]
    ok_b = [b, 64, b, 64, s, b, 64, b, 64, b, 64, b, b, 16, 64, 64, 0]
    ok_g = [b, 64, b, 64, b, 64, 16, 64]
    L.call("magpo_resln_fwd", *ok_f, st())
    L.call("magpo_resln_bwd", *ok_b, st())
    L.call("magpo_gelu_bwd", *ok_g, st())

    def bad(name, base, changes):
        a = list(base)
        for i, x in changes.items():
            a[i] = x
        with pytest.raises(ValueError):
            L.call(name, *a, st())
    for ch in ({2: None}, {4: None}, {5: None}, {6: None}, {1: 66}, {3: 66}, {7: 66}, {3: 60}, {8: -1}, {9: 48}, {10: 0}, {10: 65}, {11: 1}, {11: 2}):
        bad("magpo_resln_fwd", ok_f, ch)           # ({11: 2}: gelu with a residual)
    for ch in ({2: None}, {4: None}, {5: None}, {9: None}, {11: None}, {12: None}, {1: 66}, {3: 66}, {6: 66}, {8: 66}, {10: 66}, {14: 48}, {15: 0},
               {15: 65}, {16: 3}, {16: 2}):
        bad("magpo_resln_bwd", ok_b, ch)
    for ch in ({0: None}, {2: None}, {4: None}, {1: 66}, {3: 60}, {5: 66}, {6: -1}, {7: 32}):
        bad("magpo_gelu_bwd", ok_g, ch)
    torch.cuda.synchronize()
