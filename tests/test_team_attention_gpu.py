"""The team softmax-attention kernels (csrc/team_attention.hip: magpo_team_attention_fwd / _bwd) against fp64 autograd of the restatement
(tests/mat_ref.py: attention.py:59-72 between the projections).

Accuracy bar, per case and per output: max error against fp64 <= max(2 x the error of the same formula evaluated by torch in fp32 on the
CPU on the same inputs, 2^-24 x max|reference|) -- the factor 2 is for the different summation order and exp of two correct fp32
evaluations, the floor is one fp32 rounding of the largest result.  Every case prints one TEAMATT line; one run's lines are kept as
profiles/mat_team_attention_errors.txt.

The kernels sum in fp64 and round every output once, so they sit at the floor.

Layout of every case: two heads; q in a tensor of its own with a row stride of its own, k and v side by side in the rows of one wider
buffer (the cross-attention's shape: q from the encoder representation, k | v from the decoder stream); what lies between the operands is
5e3 and must never reach a result; outputs in guarded, strided buffers."""
import pytest
import torch

from tests import mat_ref as mr
from tests.gpu_util import DEV, Guard

pytestmark = pytest.mark.gpu

NH = 2
U24 = 2.0 ** -24
NTEAMS = (1, 7, 33)   # 33: more than one workgroup of floor(64 / A) teams for every A > 1, the last one partly filled


@pytest.fixture(scope="module")
def L():
    from magpo_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def heads(t, hs):
    """[nteams, A, NH * hs] -> [nteams * NH, A, hs]"""
    n, A, _ = t.shape
    return t.reshape(n, A, NH, hs).permute(0, 2, 1, 3).reshape(n * NH, A, hs)


def unheads(t, n):
    _, A, hs = t.shape
    return t.reshape(n, NH, A, hs).permute(0, 2, 1, 3).reshape(n, A, NH * hs)


_inputs = {}


def inputs(A, hs, nteams, qscale=1.0):
    """fp32 q, k, v, dy [nteams, A, NH hs] (seeded, shared, never changed) and per mask the fp64 reference and the fp32 restatement:
    (y, lse [nteams, A, NH], dq, dk, dv)."""
    key = (A, hs, nteams, qscale)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 * A + 10 * hs + nteams)
        q, k, v, dy = (torch.randn(nteams, A, NH * hs, generator=g) for _ in range(4))
        q = q * qscale
        ref = {}
        for masked in (0, 1):
            for dt in (torch.float64, torch.float32):
                qh, kh, vh, dh = (heads(t.to(dt), hs) for t in (q, k, v, dy))
                y, lse = mr.attention(qh, kh, vh, masked)
                grads = mr.attention_bwd(qh, kh, vh, dh, masked)
                lse = lse.reshape(nteams, NH, A).permute(0, 2, 1)
                ref[masked, dt] = (unheads(y, nteams), lse, *(unheads(t, nteams) for t in grads))
        _inputs[key] = (q, k, v, dy, ref)
    return _inputs[key]


def operands(q, k, v, hs):
    """Device operands: q rows ldq = NH hs + 12 apart in a tensor of their own; k | v in one buffer of rows 2 NH hs + 4 wide."""
    R, W = q.shape[0] * q.shape[1], NH * hs
    qb = torch.full((R, W + 12), 5.0e3, device=DEV)
    kv = torch.full((R, 2 * W + 4), 5.0e3, device=DEV)
    qb[:, :W] = q.reshape(R, W).to(DEV)
    kv[:, :W] = k.reshape(R, W).to(DEV)
    kv[:, W:2 * W] = v.reshape(R, W).to(DEV)
    return qb, W + 12, kv, 2 * W + 4, kv[:, W:], 2 * W + 4


def run(L, A, hs, masked, nteams, q, k, v, dy):
    R, W = nteams * A, NH * hs
    qd, ldq, kd, ldk, vd, ldv = operands(q, k, v, hs)
    y, lse = Guard(R, W, W + 4), Guard(R, NH, NH)
    L.call("magpo_team_attention_fwd", qd, ldq, kd, ldk, vd, ldv, y, W + 4, lse, nteams, A, A, 0, masked, hs, NH, st())
    dyd = torch.full((R, W + 8), 5.0e3, device=DEV)
    dyd[:, :W] = dy.reshape(R, W).to(DEV)
    dq, dk, dv = Guard(R, W, W + 4), Guard(R, W, W + 8), Guard(R, W, W)
    L.call("magpo_team_attention_bwd", qd, ldq, kd, ldk, vd, ldv, lse, dyd, W + 8, dq, W + 4, dk, W + 8, dv, W, nteams, A, masked, hs, NH, st())
    torch.cuda.synchronize()
    for n, gd in (("y", y), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        gd.check(f"{n} A{A} hs{hs} m{masked} n{nteams}")
    return [gd.out.cpu().reshape(nteams, A, -1) for gd in (y, lse, dq, dk, dv)]


def err(a, ref):
    return (a.double() - ref.double()).abs().max().item()


def compare(tag, got, ref64, ref32):
    figs, bad = [], []
    for n, g, w, f in zip(("y", "lse", "dq", "dk", "dv"), got, ref64, ref32):
        e, e32 = err(g, w), err(f, w)
        bound = max(2.0 * e32, U24 * w.abs().max().item())
        figs.append(f"{n} {e:.3e}/{e32:.3e}/{bound:.3e}")
        if not e <= bound:
            bad.append(n)
    print(f"TEAMATT {tag}: err/fp32-torch-err/bound " + " ".join(figs))
    return [f"{tag}: {bad} above the bar ({figs})"] if bad else []


@pytest.mark.parametrize("hs", [16, 32, 64])
@pytest.mark.parametrize("A", [1, 2, 3, 5, 8, 32])
def test_forward_and_backward_against_fp64(L, A, hs):
    failed = []   # every figure is printed before the first one is asserted
    for nteams in NTEAMS:
        q, k, v, dy, ref = inputs(A, hs, nteams)
        for masked in (0, 1):
            got = run(L, A, hs, masked, nteams, q, k, v, dy)
            failed += compare(f"A={A} hs={hs} masked={masked} nteams={nteams}", got, ref[masked, torch.float64], ref[masked, torch.float32])
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("A,hs", [(5, 32), (8, 64)])
def test_large_scores_need_the_max_subtraction(L, A, hs):
    """q scaled so that the scores reach +-60: exp(60) squared overflows fp32, so a kernel that does not subtract the row maximum (or that
    lets a masked score into it) returns inf / NaN here."""
    nteams = 7
    q, k, v, dy, _ = inputs(A, hs, nteams)
    s = (heads(q.double(), hs) @ heads(k.double(), hs).transpose(1, 2)).abs().max().item() / hs ** 0.5
    q, k, v, dy, ref = inputs(A, hs, nteams, qscale=60.0 / s)
    smax = (heads(q.double(), hs) @ heads(k.double(), hs).transpose(1, 2)).abs().max().item() / hs ** 0.5
    assert 59.0 < smax < 61.0
    failed = []
    for masked in (0, 1):
        got = run(L, A, hs, masked, nteams, q, k, v, dy)
        assert all(bool(torch.isfinite(g).all()) for g in got)
        failed += compare(f"scores+-60 A={A} hs={hs} masked={masked} nteams={nteams}", got, ref[masked, torch.float64], ref[masked, torch.float32])
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("A", [3, 8])
def test_acting_form_rows_equal_the_full_call(L, A):
    """Every decoder iteration (ntok, ret_from) = (i + 1, i): only row i of every team is produced, from the k / v rows j <= i (the rows
    behind them hold NaN: not written yet while acting), and it is the row of the full masked call."""
    hs, nteams = 32, 9
    R, W = nteams * A, NH * hs
    q, k, v, dy, ref = inputs(A, hs, nteams)
    full = run(L, A, hs, 1, nteams, q, k, v, dy)
    w64, w32 = ref[1, torch.float64], ref[1, torch.float32]
    failed = []
    for i in range(A):
        kn, vn = k.clone(), v.clone()
        kn[:, i + 1:] = float("nan")
        vn[:, i + 1:] = float("nan")
        qd, ldq, kd, ldk, vd, ldv = operands(q, kn, vn, hs)
        y, lse = Guard(R, W, W + 4), Guard(R, NH, NH)
        L.call("magpo_team_attention_fwd", qd, ldq, kd, ldk, vd, ldv, y, W + 4, lse, nteams, A, i + 1, i, 1, hs, NH, st())
        torch.cuda.synchronize()
        produced = torch.zeros(nteams, A, dtype=torch.bool)
        produced[:, i] = True
        y.check(f"acting y A{A} i{i}", defined=produced.reshape(R))
        lse.check(f"acting lse A{A} i{i}", defined=produced.reshape(R))
        gy, gl = y.out.cpu().reshape(nteams, A, W), lse.out.cpu().reshape(nteams, A, NH)
        assert bool(torch.isnan(gy[~produced]).all()) and bool(torch.isnan(gl[~produced]).all()), "a row outside [ret_from, ntok) was written"
        for n, g, fl, a64, a32 in (("y", gy, full[0], w64[0], w32[0]), ("lse", gl, full[1], w64[1], w32[1])):
            e, ef, e32 = err(g[:, i], a64[:, i]), err(g[:, i], fl[:, i]), err(a32[:, i], a64[:, i])
            bound = max(2.0 * e32, U24 * a64[:, i].abs().max().item())
            print(f"TEAMATT-ACT A={A} ntok={i + 1} ret_from={i} {n}: err {e:.3e} against-full-call {ef:.3e} fp32-torch-err {e32:.3e} bound {bound:.3e}")
            if not (e <= bound and ef <= bound):
                failed.append(f"A={A} ntok={i + 1} {n}: err {e:.3e} against-full-call {ef:.3e} bound {bound:.3e}")
    assert not failed, "\n".join(failed)


def test_entry_points_reject_bad_arguments(L):
    b = torch.zeros(64, 64, device=DEV)
    l = torch.zeros(64, 2, device=DEV)
    ok_f = [b, 64, b, 64, b, 64, b, 64, l, 2, 4, 4, 0, 1, 32, 2]
    ok_b = [b, 64, b, 64, b, 64, l, b, 64, b, 64, b, 64, b, 64, 2, 4, 1, 32, 2]
    L.call("magpo_team_attention_fwd", *ok_f, st())
    L.call("magpo_team_attention_bwd", *ok_b, st())
    L.call("magpo_team_attention_fwd", *[0 if i == 9 else x for i, x in enumerate(ok_f)], st())   # no teams: nothing to do

    def bad(name, base, changes):
        a = list(base)
        for i, x in changes.items():
            a[i] = x
        with pytest.raises(ValueError):
            L.call(name, *a, st())
    for i in (0, 2, 4, 6, 8):                    # null operands / outputs
        bad("magpo_team_attention_fwd", ok_f, {i: None})
    for i in (1, 3, 5, 7):                       # strides: not a multiple of 4, narrower than the heads
        bad("magpo_team_attention_fwd", ok_f, {i: 66})
        bad("magpo_team_attention_fwd", ok_f, {i: 60})
    for ch in ({9: -1}, {10: 0}, {10: 33}, {14: 48}, {14: 0}, {14: 8}, {15: 0}, {11: 0}, {11: 5}, {12: -1}, {12: 4}, {11: 2, 12: 2}):
        bad("magpo_team_attention_fwd", ok_f, ch)
    for i in (0, 2, 4, 6, 7, 9, 11, 13):
        bad("magpo_team_attention_bwd", ok_b, {i: None})
    for i in (1, 3, 5, 8, 10, 12, 14):
        bad("magpo_team_attention_bwd", ok_b, {i: 66})
    for ch in ({15: -1}, {16: 0}, {16: 33}, {18: 48}, {19: 0}):
        bad("magpo_team_attention_bwd", ok_b, ch)
    torch.cuda.synchronize()
