"""The stateless team-retention kernels (csrc/team_retention.hip: magpo_team_retention_fwd / _bwd) against the fp64 restatement of the ff
retention (tests/ff_sable_ref.py).

Accuracy bar, per case and per output: max error against fp64 <= max(1.25 x the error of magpo_retention_chunk_fwd / _bwd on the same
inputs run as T = 1 sequences with kappa = 1, zero start states and no done flag, 2^-24 x max|reference|) -- 1.25 x the predecessor
kernel's error is the project's bar, the floor is one fp32 rounding of the result.  tests/test_ff_sable_system.py shows in fp64
that the chunk kernels so run compute the same function.  Head widths the chunk kernels do not take (not a multiple of 4) are held to the
a priori bound of an fp32 evaluation in any summation order (ff_sable_ref.retention_error_bound).  Every case prints one TEAMRET line; one
run's lines are kept as profiles/ff_sable_team_retention_errors.txt."""
import pytest
import torch

from tests import ff_sable_ref as fs
from tests.gpu_util import DEV, Guard

pytestmark = pytest.mark.gpu

E4 = 256          # the guider's row: [q | k | v | g], 4 x 64 floats
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    from magpo_amd._lib import lib
    return lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def nteams_of(A):
    tpt = 32 // A
    return sorted({1, tpt + 1, 67} | ({tpt - 1} if tpt - 1 >= 1 else set()))


_inputs = {}


def inputs(A, hs, nteams):
    """fp32 q, k, v, dr [nteams, A, hs] of one shape (seeded; shared by the cases of that shape and never changed) and their fp64
    references for masked 0 / 1: (r, dq, dk, dv)."""
    key = (A, hs, nteams)
    if key not in _inputs:
        g = torch.Generator().manual_seed(1000 * A + 10 * hs + nteams)
        q, k, v, dr = (torch.randn(nteams, A, hs, generator=g) for _ in range(4))
        ref = {}
        for masked in (0, 1):
            q64, k64, v64, d64 = (t.double() for t in (q, k, v, dr))
            ref[masked] = (fs.ff_retention(q64, k64, v64, masked), *fs.ff_retention_bwd(q64, k64, v64, d64, masked))
        _inputs[key] = (q, k, v, dr, ref)
    return _inputs[key]


def lay(layout, R, hs, q, k, v):
    """Device operands (q, ldq, k, ldk, v, ldv): tight rows of hs floats, or the guider's 4E-strided row [q | k | v | g]."""
    if layout == "tight":
        return q.reshape(R, hs).to(DEV).contiguous(), hs, k.reshape(R, hs).to(DEV).contiguous(), hs, v.reshape(R, hs).to(DEV).contiguous(), hs
    row = torch.full((R, E4), 5.0e3, device=DEV)   # what lies between the operands must never be read into a result
    for i, t in enumerate((q, k, v)):
        row[:, 64 * i:64 * i + hs] = t.reshape(R, hs).to(DEV)
    return row, E4, row[:, 64:], E4, row[:, 128:], E4


def run_team(L, A, hs, masked, nteams, layout, q, k, v, dr):
    R = nteams * A
    ldo = hs if layout == "tight" else E4
    qd, ldq, kd, ldk, vd, ldv = lay(layout, R, hs, q, k, v)
    r = Guard(R, hs, ldo if layout == "tight" else 64)
    L.call("magpo_team_retention_fwd", qd, ldq, kd, ldk, vd, ldv, r, r.full.shape[1], nteams, A, A, 0, masked, hs, None, 0, None, None, 0, st())
    drd = dr.reshape(R, hs).to(DEV).contiguous()
    dq, dk, dv = (Guard(R, hs, ldo) for _ in range(3))
    L.call("magpo_team_retention_bwd", qd, ldq, kd, ldk, vd, ldv, drd, hs, dq, ldo, dk, ldo, dv, ldo, nteams, A, masked, hs, st())
    torch.cuda.synchronize()
    for n, gd in (("r", r), ("dq", dq), ("dk", dk), ("dv", dv)):
        gd.check(f"{n} A{A} hs{hs} m{masked} n{nteams} {layout}")
    return [gd.out.cpu().reshape(nteams, A, hs) for gd in (r, dq, dk, dv)]


def run_chunk(L, A, hs, masked, nteams, q, k, v, dr):
    """The chunk kernels on the same inputs as T = 1 sequences: kappa 1, zero start states (s0 null), no done flag."""
    R = nteams * A
    qd, kd, vd, drd = (t.reshape(R, hs).to(DEV).contiguous() for t in (q, k, v, dr))
    nch = L.call("magpo_retention_num_chunks", 1, A, 0)
    states = torch.zeros(nteams, nch, 64, 64, device=DEV)
    dones = torch.zeros(nteams, 1, dtype=torch.uint8, device=DEV)
    r, dq, dk, dv = (torch.zeros(R, hs, device=DEV) for _ in range(4))
    L.call("magpo_retention_chunk_fwd", qd, hs, kd, hs, vd, hs, r, hs, None, None, dones, states, None, nteams, 1, A, masked, 1.0, hs, None, 0, st())
    L.call("magpo_retention_chunk_bwd", qd, hs, kd, hs, vd, hs, drd, hs, dq, hs, dk, hs, dv, hs, dones, states, nteams, 1, A, masked, 1.0, hs, None, 0,
           st())
    torch.cuda.synchronize()
    return [t.cpu().reshape(nteams, A, hs) for t in (r, dq, dk, dv)]


def err(a, ref):
    return (a.double() - ref).abs().max().item()


@pytest.mark.parametrize("hs", [16, 32, 64])
@pytest.mark.parametrize("A", [1, 2, 3, 5, 8, 11, 32])
def test_forward_and_backward_against_fp64(L, A, hs):
    for nteams in nteams_of(A):
        q, k, v, dr, ref = inputs(A, hs, nteams)
        assert nteams * A <= 2144
        for masked in (0, 1):
            chunk = run_chunk(L, A, hs, masked, nteams, q, k, v, dr)
            for layout in ("tight", "strided"):
                got = run_team(L, A, hs, masked, nteams, layout, q, k, v, dr)
                figs, bad = [], []
                for n, g, c, w in zip(("r", "dq", "dk", "dv"), got, chunk, ref[masked]):
                    e, ec = err(g, w), err(c, w)
                    bound = max(1.25 * ec, U24 * w.abs().max().item())
                    figs.append(f"{n} {e:.3e}/{ec:.3e}/{bound:.3e}")
                    if e > bound:
                        bad.append(n)
                print(f"TEAMRET A={A} hs={hs} masked={masked} nteams={nteams} {layout}: err/chunk-err/bound " + " ".join(figs))
                assert not bad, f"A={A} hs={hs} masked={masked} nteams={nteams} {layout}: {bad} above the bar ({figs})"


@pytest.mark.parametrize("A,hs,nteams", [(3, 20, 11), (5, 7, 9), (4, 1, 10), (32, 63, 3), (6, 44, 67)])
def test_head_widths_the_chunk_kernels_do_not_take(L, A, hs, nteams):
    """hs not a multiple of 8 (a zero-filled half fragment) or of 4 (scalar operand loads), tight rows at a stride that is a multiple of
    4: every element within the a priori fp32 bound of its own sum."""
    g = torch.Generator().manual_seed(7 * A + hs)
    q, k, v, dr = (torch.randn(nteams, A, hs, generator=g) for _ in range(4))
    R, ld = nteams * A, (hs + 3) // 4 * 4
    pad = lambda t: torch.nn.functional.pad(t.reshape(R, hs), (0, ld - hs), value=3.0e3).to(DEV).contiguous()
    qd, kd, vd, dd = pad(q), pad(k), pad(v), pad(dr)
    for masked in (0, 1):
        r, dq, dk, dv = (Guard(R, hs, ld) for _ in range(4))
        L.call("magpo_team_retention_fwd", qd, ld, kd, ld, vd, ld, r, ld, nteams, A, A, 0, masked, hs, None, 0, None, None, 0, st())
        L.call("magpo_team_retention_bwd", qd, ld, kd, ld, vd, ld, dd, ld, dq, ld, dk, ld, dv, ld, nteams, A, masked, hs, st())
        torch.cuda.synchronize()
        q64, k64, v64, d64 = (t.double() for t in (q, k, v, dr))
        want = (fs.ff_retention(q64, k64, v64, masked), *fs.ff_retention_bwd(q64, k64, v64, d64, masked))
        aq, ak, av, ad = (t.abs() for t in (q64, k64, v64, d64))
        M = fs.team_mask(A, masked)
        c = (hs + A + 2) * U24     # nested dot products of hs and at most A terms
        bounds = (c * ((aq @ ak.transpose(1, 2)) * M) @ av, c * ((ad @ av.transpose(1, 2)) * M) @ ak,
                  c * ((ad @ av.transpose(1, 2)) * M).transpose(1, 2) @ aq, c * ((aq @ ak.transpose(1, 2)) * M).transpose(1, 2) @ ad)
        for n, gd, w, b in zip(("r", "dq", "dk", "dv"), (r, dq, dk, dv), want, bounds):
            gd.check(f"{n} A{A} hs{hs} m{masked}")
            d = (gd.out.cpu().double().reshape(nteams, A, hs) - w).abs()
            print(f"TEAMRET-ODD A={A} hs={hs} masked={masked} nteams={nteams} {n}: err {d.max().item():.3e} worst err/bound {(d / b.clamp_min(1e-300)).max().item():.3f}")
            assert bool((d <= b + 1e-300).all()), (n, A, hs, masked)


def _recurrent(L, q, ldq, k, ldk, v, ldv, out, ldo, N, A, ntok, ret_from, hs, gp, ldg, gamma, beta, gs):
    S = torch.zeros(N, 64, 64, device=DEV)
    L.call("magpo_retention_recurrent", S, q, ldq, k, ldk, v, ldv, A, out, ldo, N, ntok, ret_from, 1.0, 0, gp, ldg, gamma, beta, hs, gs, st())
    assert float(S.abs().max()) == 0.0


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("A,hs,gs,N", [(3, 64, 64, 13), (8, 64, 64, 5), (3, 32, 16, 11), (8, 16, 4, 9)])
def test_acting_form_against_the_recurrent_kernel(L, A, hs, gs, N, epilogue):
    """ntok / ret_from of every decoder iteration (ntok = i + 1, ret_from = i) and of the encoder (ntok = A, ret_from = 0), with and
    without the fused GroupNorm + swish-gate epilogue, in the acting chain's strided layout, next to magpo_retention_recurrent on zero
    states with decay 1 (which writes no state here); both against fp64.  The two kernels associate the sum differently (the recurrent one
    builds sum_j k_j^T v_j first), so neither is held to the other: each is held to the a priori bound of an fp32 evaluation.
    Raw rows: d = (hs + A + 2) u sum_j M_ij (|q_i| . |k_j|) |v_j|, u = 2^-24 (ff_sable_ref.retention_error_bound).
    Epilogue rows, out = swish(g) (y gamma + beta), y = (x - mean) rstd over a group: to first order |dy_i| <= rstd D (2 + |y_i|) for
    |dx| <= D on the group (the mean moves by at most D, the variance term by |y_i| mean|y| D rstd and mean|y| <= 1), so
    |d out_i| <= |swish(g_i) gamma_i| rstd D (2 + |y_i|) + 8 u |swish(g_i)| (|y_i gamma_i| + |beta_i|) for the epilogue's own roundings.
    Rows outside [ret_from, ntok) are not written."""
    from oracle import networks as onets
    g = torch.Generator().manual_seed(31 * A + hs + gs)
    R = N * A
    q, k, v, gpre = (torch.randn(N, A, hs, generator=g) for _ in range(4))
    gamma, beta = torch.randn(hs, generator=g), torch.randn(hs, generator=g)
    row = torch.full((R, E4), 4.0e3, device=DEV)
    for i, t in enumerate((q, k, v, gpre)):
        row[:, 64 * i:64 * i + hs] = t.reshape(R, hs).to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    nh = hs // gs
    forms = [(A, 0, 0)] + [(i + 1, i, 1) for i in range(A)]
    full = row
    for ntok, ret_from, masked in forms:
        row = full.clone()
        row.view(N, A, E4)[:, ntok:] = float("nan")   # the rows of agents >= ntok are not written yet while acting: never read
        out = Guard(R, hs, 64)
        ref_out = torch.full((R, 64), float("nan"), device=DEV)
        ep = (row[:, 192:], E4, gd, bd, gs) if epilogue else (None, 0, None, None, 0)
        L.call("magpo_team_retention_fwd", row, E4, row[:, 64:], E4, row[:, 128:], E4, out, 64, N, A, ntok, ret_from, masked, hs, *ep, st())
        _recurrent(L, row, E4, row[:, 64:], E4, row[:, 128:], E4, ref_out, 64, N, A, ntok, ret_from, hs,
                   row[:, 192:] if epilogue else None, E4 if epilogue else 0, gd if epilogue else None, bd if epilogue else None, gs if epilogue else hs)
        torch.cuda.synchronize()
        produced = torch.zeros(N, A, dtype=torch.bool)
        produced[:, ret_from:ntok] = True
        out.check(f"acting A{A} hs{hs} ntok{ntok}", defined=produced.reshape(R))
        got = out.out.cpu().reshape(N, A, hs)
        assert bool(torch.isnan(got[~produced]).all()), "a row outside [ret_from, ntok) was written"
        rec = ref_out[:, :hs].cpu().reshape(N, A, hs)
        q64, k64, v64 = q.double(), k.double(), v.double()
        raw = fs.ff_retention_partial(q64, k64, v64, bool(masked), ntok, ret_from)
        sel = produced
        if not epilogue:
            bound = fs.retention_error_bound(q[:, :ntok], k[:, :ntok], v[:, :ntok], bool(masked))[:, ret_from:ntok]
            for name, x in (("team", got), ("recurrent", rec)):
                d = (x.double()[:, ret_from:ntok] - raw[:, ret_from:ntok]).abs()
                print(f"TEAMRET-ACT A={A} hs={hs} ntok={ntok} ret_from={ret_from} {name}: err {d.max().item():.3e} worst err/bound {(d / bound.clamp_min(1e-300)).max().item():.3f}")
                assert bool((d <= bound + 1e-300).all()), (name, ntok)
            continue
        x = raw[sel].reshape(-1, nh, gs)
        D = fs.retention_error_bound(q[:, :ntok], k[:, :ntok], v[:, :ntok], bool(masked))[:, ret_from:ntok].reshape(-1, nh, gs).amax(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + 1e-6)
        y = ((x - x.mean(-1, keepdim=True)) * rstd).reshape(-1, hs)
        assert (y - onets.groupnorm_rows(raw[sel].reshape(-1, hs), torch.ones(hs, dtype=torch.float64), torch.zeros(hs, dtype=torch.float64), nh)).abs().max() < 1e-9
        sw = onets.swish(gpre.double()[sel].reshape(-1, hs))
        ga, be = gamma.double(), beta.double()
        want = sw * (y * ga + be)
        bound = (sw * ga).abs() * (rstd * D).expand(-1, nh, gs).reshape(-1, hs) * (2 + y.abs()) + 8 * U24 * sw.abs() * ((y * ga).abs() + be.abs())
        for name, o in (("team", got), ("recurrent", rec)):
            d = (o[sel].reshape(-1, hs).double() - want).abs()
            print(f"TEAMRET-ACT A={A} hs={hs} gs={gs} ntok={ntok} ret_from={ret_from} epilogue {name}: err {d.max().item():.3e} worst err/bound {(d / bound.clamp_min(1e-300)).max().item():.3f}")
            assert bool((d <= bound + 1e-300).all()), (name, ntok)


def test_entry_points_reject_bad_arguments(L):
    b = torch.zeros(64, 64, device=DEV)
    ok_f = [b, 64, b, 64, b, 64, b, 64, 2, 4, 4, 0, 1, 64, None, 0, None, None, 0]
    ok_b = [b, 64, b, 64, b, 64, b, 64, b, 64, b, 64, b, 64, 2, 4, 1, 64]
    L.call("magpo_team_retention_fwd", *ok_f, st())
    L.call("magpo_team_retention_bwd", *ok_b, st())
    L.call("magpo_team_retention_fwd", *[0 if i == 8 else x for i, x in enumerate(ok_f)], st())   # no teams: nothing to do

    def bad(name, base, changes):
        a = list(base)
        for i, x in changes.items():
            a[i] = x
        with pytest.raises(ValueError):
            L.call(name, *a, st())
    for i in (0, 2, 4, 6):                       # null operands / output
        bad("magpo_team_retention_fwd", ok_f, {i: None})
    for i in (1, 3, 5, 7):                       # strides not multiples of 4
        bad("magpo_team_retention_fwd", ok_f, {i: 66})
    for ch in ({8: -1}, {9: 0}, {9: 33}, {13: 0}, {13: 65}, {10: 0}, {10: 5}, {11: -1}, {11: 4}, {10: 2, 11: 2}):
        bad("magpo_team_retention_fwd", ok_f, ch)
    g = torch.ones(64, device=DEV)
    L.call("magpo_team_retention_fwd", *ok_f[:14], b, 64, g, g, 64, st())
    for ch in ({16: None}, {17: None}, {15: 66}, {18: 0}, {18: 48}, {18: 128}):   # epilogue: gamma / beta, gate stride, group size
        bad("magpo_team_retention_fwd", ok_f[:14] + [b, 64, g, g, 64], ch)
    for i in (0, 2, 4, 6, 8, 10, 12):
        bad("magpo_team_retention_bwd", ok_b, {i: None})
    for i in (1, 3, 5, 7, 9, 11, 13):
        bad("magpo_team_retention_bwd", ok_b, {i: 30})
    for ch in ({14: -1}, {15: 0}, {15: 33}, {17: 0}, {17: 65}):
        bad("magpo_team_retention_bwd", ok_b, ch)
    torch.cuda.synchronize()
