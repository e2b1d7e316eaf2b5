"""The RL-side kernels (csrc/rl.hip, csrc/optim.hip) and the slab reduction at production strides, edge shapes and loss kinks: fused
MAGPO loss, categorical sampling, GAE, advantage moments, clip + Adam, minibatch gather, k_reduce_slabs, and the accumulate / krows /
swish arguments of magpo_wgrad / magpo_linear.  References and case builders are in tests/kernel_refs.py (checked on the CPU by
tests/test_kernel_refs.py); every output sits in a Guard, every comparison prints its figure before it asserts.

Near-kink rows (loss): the clipped surrogates have kinks, and a row within rounding of one can take the other branch in fp32.  Rows of
the fp64 reference within kr.KINK = 1e-5 of a kink (kr.loss_near_kink) are left out of the dg / da / dv comparison, nothing else; the CPU
module caps them at 0.1 % of the rows of a case with R >= 1000 and at none below.  kl_loss = mean(kl * [|d| > log clip_gpo]) jumps at its
kink, so loss[0], loss[4] and loss[7] get the slack sum(kl over near-kink rows) / R, printed with each case."""
import math

import numpy as np
import pytest
import torch

from oracle import learner as olearn
from oracle import networks as onets
from oracle import prng as oprng
from tests import kernel_refs as kr
from tests.gpu_util import DEV, PAD, UNSET_INT, Guard, check, check_sum, dev, transpose_pad

pytestmark = pytest.mark.gpu
D = torch.float64
S = kr.SYSC
U8 = torch.uint8


def _sync():
    torch.cuda.synchronize()


class ByteGuard:
    """Guard for unsigned-char outputs (the float sentinel of gpu_util.Guard does not fit a byte): owned rows pre-filled with 7, PAD rows
    of 165 before and after; the kernels under test write 0 / 1."""
    UNSET, SENT = 7, 165

    def __init__(self, R, W):
        self.R, self.W = R, W
        self.full = torch.full((R + 2 * PAD, W), self.SENT, device=DEV, dtype=U8)
        self.out = self.full[PAD:PAD + R]
        self.out[:] = self.UNSET

    def data_ptr(self):
        return self.out.data_ptr()

    def check(self, what, written=True):
        assert bool((self.full[:PAD] == self.SENT).all()) and bool((self.full[PAD + self.R:] == self.SENT).all()), f"{what}: written outside the owned block"
        left = int((self.out == self.UNSET).sum())
        assert left == (0 if written else self.R * self.W), f"{what}: {left} elements still unset"


# ================================================================================================ magpo_loss_fwd_bwd
FILLS = {"zero": 0.0, "1e30": 1e30, "nan": float("nan")}


def _run_loss(L, stream, c, fill, what, strides=None):
    """One adv_moments + loss call on the case with `fill` in the input columns >= K.  Returns the guarded outputs after their checks."""
    R, K = c["R"], c["K"]
    ldg, lda, lddg, lddda = strides or c["strides"]

    def padded(x, ld):
        t = torch.full((R, ld), fill)
        t[:, :K] = x
        return dev(t)
    stats = Guard(1, 2)
    ws = Guard(1024, 8, dtype=D, fill=0.0)            # exactly the 8 * 1024 doubles the header asks for
    L.call("magpo_adv_moments", dev(c["adv"]), R, ws, stats, stream)
    dg, da, dv, lo = Guard(R, min(lddg, 64), lddg), Guard(R, min(lddda, 64), lddda), Guard(R, 1), Guard(1, 9)
    L.call("magpo_loss_fwd_bwd", padded(c["gl"], ldg), ldg, padded(c["al"], lda), lda, dev(c["legal"].to(U8)) if c["masked"] else None,
           dev(c["action"].int()), dev(c["old"]), dev(c["vold"]), dev(c["value"]), dev(c["adv"]), dev(c["tgt"]), stats.out, dg, lddg, da, lddda,
           dv, ws, lo, R, K, S.clip_eps, S.clip_gpo, S.ent_coef, S.vf_coef, S.alpha, stream)
    _sync()
    for g, n in ((stats, "adv_stats"), (ws, "workspace"), (dg, "dg"), (da, "da"), (dv, "dvalue"), (lo, "loss_out")):
        g.check(f"{what} {n}")
    return dict(dg=dg, da=da, dv=dv, lo=lo)


def _check_loss(what, c, r64, r32, out):
    R, K, legal = c["R"], c["K"], c["legal"]
    near = kr.loss_near_kink(r64)
    ok = ~near
    slack = float(r64["kl"][near].sum()) / R
    print(f"LOSSKINK {what}: near-kink rows {int(near.sum())} / {R} left out of dg / da / dv, kl slack {slack:.3e}")
    lo = out["lo"].out[0].cpu().double()
    fails = []
    for j, name in enumerate(kr.LOSS_NAMES):
        ref = r64["loss"][j].item()
        e32, err = abs(r32["loss"][j].item() - ref), abs(lo[j].item() - ref)
        sl = slack if j in kr.LOSS_KL_SLACK else 0.0
        bound = max(kr.loss_scalar_bound(r64, j), 4.0 * e32) + sl
        print(f"LOSSERR {what} {name}: fp32-torch err {e32:.3e} kernel err {err:.3e} ratio {err / max(e32, 1e-300):.2f} bound {bound:.3e} "
              f"kink slack {sl:.3e} ref {ref:.3e}")
        if not err <= bound:
            fails.append(f"{name}: err {err:.3e} > bound {bound:.3e}")
    for n in ("dg", "da", "dv"):
        got = (out[n].out[:, :K] if n != "dv" else out[n].out[:, 0]).cpu()
        ref, ref32 = r64[n][ok], r32[n][ok]
        if ref.numel() == 0:
            continue
        e32, err = kr.max_err(ref32, ref), kr.max_err(got[ok], ref)
        bound = max(kr.loss_grad_bound(r64, n, ok), 4.0 * e32)
        print(f"LOSSERR {what} {n}: fp32-torch err {e32:.3e} kernel err {err:.3e} ratio {err / max(e32, 1e-300):.2f} bound {bound:.3e} "
              f"kink slack 0 ref {ref.abs().max().item():.3e}")
        if not err <= bound:
            fails.append(f"{n}: err {err:.3e} > bound {bound:.3e}")
    assert not fails, f"{what}: {fails}"
    # exact zeros: illegal columns, the columns K .. min(ld, 64) of the gradient rows, and every column of a row with one legal action
    one = (legal.sum(1) == 1).to(DEV)
    for n in ("dg", "da"):
        o = out[n].out
        assert bool((o[:, K:] == 0).all()), f"{what} {n}: columns >= K must be exactly 0"
        assert bool((o[:, :K][~legal.to(DEV)] == 0).all()), f"{what} {n}: illegal columns must be exactly 0"
        assert bool((o[one] == 0).all()), f"{what} {n}: a row with one legal action has no gradient"


@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("i", range(len(kr.LOSS_MATRIX)), ids=[kr.loss_case_id(i) for i in range(len(kr.LOSS_MATRIX))])
def test_loss_matrix(L, stream, i, fill):
    """The matrix of kr.LOSS_MATRIX (how it is chosen: kr._loss_matrix) x what the input columns >= K hold.  The fills 1e30 and NaN must
    give the zero-filled run's loss scalars and gradients bit for bit: the vector branch loads those columns and has to discard them."""
    c, r64, r32 = kr.loss_matrix_case(i)
    what = f"{c['name']} fill={fill}"
    out = _run_loss(L, stream, c, FILLS[fill], what)
    _check_loss(what, c, r64, r32, out)
    if fill != "zero":
        base = _run_loss(L, stream, c, 0.0, what + " (zero-filled run)")
        for n in ("lo", "dg", "da", "dv"):
            assert torch.equal(out[n].full, base[n].full), f"{what}: {n} differs from the zero-filled run"


@pytest.mark.parametrize("strides", ["s64", "tight"])
def test_loss_single_legal_rows_only(L, stream, strides):
    """Every row has one legal action: log-prob 0 there, so entropy, both KL terms and all logit gradients are exactly 0, the guider ratio
    is exp(-old) and the value loss is untouched by the mask."""
    R, K = 1500, 20
    c = kr.loss_case(R, K, 77, mask_p=0.6, one_legal=1.0)
    assert bool((c["legal"].sum(1) == 1).all())
    r64, r32 = kr.loss_ref(c), kr.loss_ref(c, torch.float32)
    assert int(kr.loss_near_kink(r64).sum()) <= 1
    what = f"single-legal-only {strides}"
    out = _run_loss(L, stream, c, 1e30, what, kr.loss_strides(strides, K))
    _check_loss(what, c, r64, r32, out)
    lo = out["lo"].out[0].cpu()
    assert lo[4].item() == 0 and lo[5].item() == 0 and lo[6].item() == 0, lo
    assert bool((out["dg"].out == 0).all()) and bool((out["da"].out == 0).all())


def test_loss_rejects_bad_arguments(L, stream):
    """Everything rl.hip rejects on the host before any launch: K > 64, K above a stride, a gradient stride that is no multiple of 4,
    clip_gpo <= 0.  Nothing is written."""
    R, K = 8, 20
    c = kr.loss_case(R, K, 1)
    x = dev(torch.zeros(R + 2, 72))
    stats = dev(torch.tensor([0.0, 1.0]))
    ws = Guard(1024, 8, dtype=D, fill=0.0)
    dg, da, dv, lo = Guard(R, 72), Guard(R, 72), Guard(R, 1), Guard(1, 9)
    vec = [dev(c[n]) for n in ("old", "vold", "value", "adv", "tgt")]
    for K_, strides, gpo in ((65, (72, 72, 72, 72), 1.5), (20, (16, 64, 64, 64), 1.5), (20, (64, 16, 64, 64), 1.5), (20, (64, 64, 16, 64), 1.5),
                             (20, (64, 64, 64, 16), 1.5), (20, (64, 64, 22, 64), 1.5), (20, (64, 64, 64, 30), 1.5), (20, (64, 64, 64, 64), 0.0),
                             (20, (64, 64, 64, 64), -1.0)):
        with pytest.raises(ValueError):
            L.call("magpo_loss_fwd_bwd", x, strides[0], x, strides[1], None, dev(c["action"].int()), vec[0], vec[1], vec[2], vec[3], vec[4], stats,
                   dg, strides[2], da, strides[3], dv, ws, lo, R, K_, S.clip_eps, gpo, S.ent_coef, S.vf_coef, S.alpha, stream)
    _sync()
    for g, n in ((dg, 72), (da, 72), (dv, 1), (lo, 9)):
        g.check("rejected calls write nothing", defined=torch.zeros(g.R, dtype=torch.bool))
        assert bool(torch.isnan(g.out).all())
    ws.check("rejected calls write nothing")
    assert bool((ws.out == 0).all())


# ================================================================================================ magpo_sample_categorical
SAMPLE_N = (1, 127, 128, 129, 70001)


@pytest.mark.parametrize("mask", [None, "mask", "single"])
@pytest.mark.parametrize("K", [1, 2, 5, 20, 33, 64])
def test_sample_categorical_matrix(L, stream, K, mask):
    """K x mask x N around the 128-thread block edge, in the learner's layout: mask [N][A][K] addressed with mask_stride = A * K from the
    agent's own offset, outputs strided into [N][A] buffers.  Log-probs against the fp64 masked log-softmax, actions bit-exact against
    the oracle's sampler on the device's own log-probs; key_dev, lp_all = NULL and next_idx = NULL change nothing else."""
    A, ag = 3, 2
    key = oprng.split(oprng.prng_key(70 + K), 3)[1]
    key_dev = dev(torch.from_numpy(key.view(np.int32).copy()))
    for N in SAMPLE_N:
        what = f"sample K={K} mask={mask} N={N}"
        ld, lp_ld = K + 3, K + 1
        c = kr.sample_case(N, K, ld, 1000 * K + N, mask, A)
        lp64, legal = kr.sample_lp_ref(c)
        md = None if mask is None else dev(c["legal"].to(U8))
        margs = (None, 0) if mask is None else (md[:, ag], A * K)
        logits = dev(c["logits"])
        runs = []
        for mode in ("value", "key_dev", "no_optional"):
            act, lp, nxt = Guard(N, A, dtype=torch.int32), Guard(N, A), Guard(N, A, dtype=torch.int32)
            lpall = Guard(N, K, lp_ld)
            k0, k1, kd = (int(key[0]), int(key[1]), None) if mode != "key_dev" else (0, 0, key_dev)
            opt = (nxt.out[:, ag - 1:], A, lpall, lp_ld) if mode != "no_optional" else (None, 0, None, 0)
            L.call("magpo_sample_categorical", logits, ld, margs[0], margs[1], k0, k1, kd, act.out[:, ag:], A, lp.out[:, ag:], A, *opt, N, K, stream)
            _sync()
            col = torch.zeros(N, A, dtype=torch.bool)
            col[:, ag] = True
            ncol = torch.zeros(N, A, dtype=torch.bool)
            ncol[:, ag - 1] = mode != "no_optional"
            act.check(what + " action", col); lp.check(what + " logp", col); nxt.check(what + " next_idx", ncol)
            lpall.check(what + " lp_all", torch.full((N,), mode != "no_optional"))
            # every other column of the [N][A] buffers is untouched
            assert bool((act.out[:, :ag] == UNSET_INT).all()) and bool(torch.isnan(lp.out[:, :ag]).all())
            assert bool((nxt.out[~ncol.to(DEV)] == UNSET_INT).all())
            if mode == "no_optional":
                assert bool(torch.isnan(lpall.out).all())
            runs.append((act.out[:, ag].cpu(), lp.out[:, ag].cpu(), nxt.out[:, ag - 1].cpu(), lpall.out.cpu()))
        a, lpa, nx, lpd = runs[0]
        zero = torch.zeros_like(lp64)
        check(what + " log-softmax (legal entries)", torch.where(legal, lpd.double(), zero), torch.where(legal, lp64, zero), kr.local_bound(torch.where(legal, lp64, zero), 1e-5, 1e-6))
        assert bool((lpd[~legal] < -1e30).all())
        ref_a = torch.from_numpy(oprng.categorical(key, lpd.numpy()[:, None, :])[:, 0])
        assert torch.equal(a, ref_a), f"{what}: sampled action indices must be bit-exact"
        assert torch.equal(nx, ref_a + 1)
        assert torch.equal(lpa, lpd.gather(1, ref_a.long()[:, None])[:, 0]), f"{what}: logp must be the gathered lp_all entry"
        assert bool(legal.gather(1, a.long()[:, None]).all()), f"{what}: an illegal action was returned"
        one = legal.sum(1) == 1
        assert torch.equal(a[one].long(), legal[one].int().argmax(1)) and bool((lpa[one] == 0).all())
        for other, mode in ((runs[1], "key_dev"), (runs[2], "no_optional")):
            assert torch.equal(other[0], a) and torch.equal(other[1], lpa), f"{what}: {mode} changes the sample"
        assert torch.equal(runs[1][2], nx) and torch.equal(runs[1][3], lpd)


def test_sample_rejects_oversized_counter(L, stream):
    """N * K >= 2^32 would wrap the 32-bit gumbel counter: rejected on the host, nothing launched."""
    act, lp = Guard(4, 1, dtype=torch.int32), Guard(4, 1)
    with pytest.raises(ValueError):
        L.call("magpo_sample_categorical", dev(torch.zeros(4, 64)), 64, None, 0, 1, 2, None, act, 1, lp, 1, None, 0, None, 0, 1 << 26, 64, stream)
    _sync()
    act.check("rejected", torch.zeros(4, dtype=torch.bool)); lp.check("rejected", torch.zeros(4, dtype=torch.bool))
    assert bool((act.out == UNSET_INT).all()) and bool(torch.isnan(lp.out).all())


# ================================================================================================ magpo_gae
def _run_gae(L, stream, c, gamma, lam, what):
    T, N, A = c["T"], c["N"], c["A"]
    adv, tg = Guard(T, N * A), Guard(T, N * A)
    L.call("magpo_gae", dev(c["reward"]), dev(c["value"]), dev(c["done"].to(U8)), dev(c["last_val"]), dev(c["last_done"].to(U8)), adv, tg,
           T, N, A, gamma, lam, stream)
    _sync()
    adv.check(what + " adv"); tg.check(what + " targets")
    return adv.out.cpu().reshape(T, N, A), tg.out.cpu().reshape(T, N, A)


def _check_gae(what, got, c, gamma, lam):
    r64, r32 = kr.gae_ref(c, gamma, lam), kr.gae_ref(c, gamma, lam, torch.float32)
    for n, g, a, b in zip(("adv", "targets"), got, r64, r32):
        check(f"{what} {n} (fp32-torch err {kr.max_err(b, a):.3e})", g, a, kr.gae_bound(a, b))


@pytest.mark.parametrize("T,N,A,ci,done", kr.gae_matrix())
def test_gae_matrix(L, stream, T, N, A, ci, done):
    """T at the scan's tile edges, sequence counts on both sides of the dispatch boundary (N * A < 8192 and T >= 16: k_gae_scan, else
    k_gae), the four coefficient pairs and five done patterns of kr.gae_matrix."""
    gamma, lam = kr.GAE_COEF[ci]
    c = kr.gae_case(T, N, A, 7 * T + N, done)
    what = f"gae T={T} N={N} A={A} gamma={gamma} lambda={lam} done={done} ({'scan' if N * A < 8192 and T >= 16 else 'serial'})"
    _check_gae(what, _run_gae(L, stream, c, gamma, lam, what), c, gamma, lam)


@pytest.mark.parametrize("T", [16, 65, 129])
@pytest.mark.parametrize("ci", [0, 1])
def test_gae_scan_and_serial_on_the_same_data(L, stream, T, ci):
    """8193 sequences run the serial kernel, the first 8191 of them the scan kernel: each faces fp64, and their common sequences agree
    within the same bound (neither is the other's reference)."""
    gamma, lam = kr.GAE_COEF[ci]
    full = kr.gae_case(T, 8193, 1, 900 + T, "random")
    cut = dict(full, N=8191, **{n: full[n][:, :8191].contiguous() for n in ("reward", "value", "done")}, last_val=full["last_val"][:8191].contiguous(),
               last_done=full["last_done"][:8191].contiguous())
    serial = _run_gae(L, stream, full, gamma, lam, f"gae serial T={T}")
    scan = _run_gae(L, stream, cut, gamma, lam, f"gae scan T={T}")
    _check_gae(f"gae serial 8193 T={T} ci={ci}", serial, full, gamma, lam)
    _check_gae(f"gae scan 8191 T={T} ci={ci}", scan, cut, gamma, lam)
    r64, r32 = kr.gae_ref(cut, gamma, lam), kr.gae_ref(cut, gamma, lam, torch.float32)
    for n, a, b, x, y in zip(("adv", "targets"), scan, serial, r64, r32):
        check(f"gae scan vs serial T={T} ci={ci} {n}", a, b[:, :8191], kr.gae_bound(x, y))


# ================================================================================================ magpo_adv_moments
MOMENT_N = (1, 2, 255, 256, 257, 1024 * 256 + 3)


def _moments(L, stream, x, what):
    ws, out = Guard(1024, 2, dtype=D, fill=0.0), Guard(1, 2)     # exactly the 2 * 1024 doubles the header asks for
    L.call("magpo_adv_moments", dev(x), x.numel(), ws, out, stream)
    _sync()
    ws.check(what); out.check(what)
    return out.out[0].cpu()


@pytest.mark.parametrize("n", MOMENT_N)
def test_adv_moments(L, stream, n):
    for kind in ("normal", "100+-0.1"):
        x = kr.adv_moments_input(kind, n, n)
        mean, rstd = kr.adv_moments_ref(x.double())
        got = _moments(L, stream, x, f"adv_moments {kind} n={n}")
        check(f"adv_moments {kind} n={n} mean", got[0], mean, 1e-7 + 1e-6 * abs(mean.item()))
        if n > 1:
            check(f"adv_moments {kind} n={n} rstd", got[1], rstd, 1e-5 * rstd.item())
        else:   # one element: the std is exactly 0
            assert got[1].item() == (torch.tensor(1.0) / torch.tensor(1e-8)).item()
    got = _moments(L, stream, torch.zeros(n), f"adv_moments zeros n={n}")
    assert got[0].item() == 0 and got[1].item() == (torch.tensor(1.0) / torch.tensor(1e-8)).item(), got
    # a non-zero constant: the mean is exact, and what the loss consumes, (x - mean) * rstd, is exactly 0 (rstd itself depends on the rounding
    # of E[x^2] - mean^2 and is not asserted beyond finite and positive)
    x = kr.adv_moments_input("const1.3", n, n)
    got = _moments(L, stream, x, f"adv_moments const n={n}")
    assert got[0].item() == x[0].item() and math.isfinite(got[1].item()) and got[1].item() > 0, got
    assert bool(((x - got[0]) * got[1] == 0).all())
    # recorded, not asserted: mean / std = 1e6 costs the one-pass formula about (mean / std)^2 2^-53 of the variance; advantages never look like this
    x = kr.adv_moments_input("1000+-1e-3", n, n)
    if n > 1:
        mean, rstd = kr.adv_moments_ref(x.double())
        got = _moments(L, stream, x, f"adv_moments 1000+-1e-3 n={n}")
        r32 = kr.adv_moments_ref(x)[1].item()
        print(f"RECORD adv_moments 1000+-1e-3 n={n}: rstd rel err {abs(got[1].item() - rstd.item()) / rstd.item():.3e} (not asserted; two-pass fp32 torch "
              f"{abs(r32 - rstd.item()) / rstd.item():.3e}), mean err {abs(got[0].item() - mean.item()):.3e}")


# ================================================================================================ magpo_clip_adam
ADAM_N = (1, 255, 257, 5000, 1024 * 256 + 77)
MAX_NORM, LR, B1, B2, EPS = 0.5, 2.5e-4, 0.9, 0.999, 1e-5
B1F, B2F = float(np.float32(B1)), float(np.float32(B2))     # what the float arguments of the entry point hold


def _filled(t):
    g = Guard(t.numel(), 1, fill=0.0)
    g.out[:, 0] = t.to(DEV)
    return g


@pytest.mark.parametrize("grad_scale", [1.0, 0.5, 0.25])
@pytest.mark.parametrize("n", ADAM_N)
def test_clip_adam_five_steps(L, stream, n, grad_scale):
    """Five steps of clip + Adam against olearn.clip_adam_step in fp64, asserting mu, nu, params and gnorm at every step.  Scenarios: far
    below and far above the clip threshold, a norm of max_norm (1 -+ 1e-3) (no exact tie: the reference's norm is fp64), and a zero
    gradient in the middle of a run.  Bounds: params and gnorm as in test_kernels_gpu.py::test_clip_adam; mu is two fp32 products and a
    sum per step (plus a quotient and a product when clipped) and the decay keeps old error from growing: 1e-6 of its largest entry;
    nu squares the gradient, which doubles its relative error: 2e-6 (the fp32 restatement is checked against both on the CPU).
    The reference runs with the decay rates the C ABI can carry, float32(0.9) and float32(0.999): the entry point takes them as floats,
    and 1 - b2 amplifies the rounding of b2 (1.3e-8 relative) by b2 / (1 - b2) = 999, so against b2 = 0.999 in double every entry of nu is
    off by the same factor 1 - 1.29e-5.  That factor cancels in nu / bc2 (the host derives bc2 from the same float), so params do not see
    it; it is printed (RECORD line), not asserted."""
    for name, (p0, grads) in kr.adam_scenarios(n, 12 + n, MAX_NORM).items():
        p = {"w": p0}
        opt = olearn.adam_init({"w": p["w"].double()})
        p64 = {"w": p["w"].double()}
        pdbl, optdbl = p64, opt     # the same run with b1 = 0.9, b2 = 0.999 in double: for the record only
        pd, md, vd = _filled(p["w"]), _filled(torch.zeros(n)), _filled(torch.zeros(n))
        ws, gn = Guard(1024, 1, dtype=D, fill=0.0), Guard(1, 1)
        for step in range(1, 6):
            gr = grads[step - 1]
            before = (pd.out.clone(), md.out.clone(), vd.out.clone())
            p64, opt, gnorm = olearn.clip_adam_step(p64, {"w": gr.double()}, opt, LR, MAX_NORM, B1F, B2F)
            pdbl, optdbl, _ = olearn.clip_adam_step(pdbl, {"w": gr.double()}, optdbl, LR, MAX_NORM)
            if name.startswith("just"):
                assert (gnorm.item() < MAX_NORM) == (name == "just-below") and abs(gnorm.item() / MAX_NORM - 1) < 1.1e-3
            bc1 = float(np.float32(1) - np.float32(B1) ** np.float32(step)); bc2 = float(np.float32(1) - np.float32(B2) ** np.float32(step))
            L.call("magpo_clip_adam", pd, dev(gr / grad_scale), md, vd, n, grad_scale, MAX_NORM, LR, B1, B2, EPS, bc1, bc2, ws, gn, stream)
            _sync()
            what = f"clip_adam n={n} scale={grad_scale} {name} step {step}"
            for gd in (pd, md, vd, ws, gn):
                gd.check(what)
            check(what + " gnorm", gn.out[0, 0], gnorm, 1e-6 * gnorm.item())
            check(what + " params", pd.out[:, 0], p64["w"], kr.local_bound(p64["w"], 1e-6, 1e-7))
            check(what + " mu", md.out[:, 0], opt["mu"]["w"], kr.ADAM_MU_RTOL * opt["mu"]["w"].abs().max().item() + 1e-30)
            check(what + " nu", vd.out[:, 0], opt["nu"]["w"], kr.ADAM_NU_RTOL * opt["nu"]["w"].abs().max().item() + 1e-30)
            if step == 5 and grad_scale == 1.0:
                nud = optdbl["nu"]["w"]
                print(f"RECORD {what}: nu against b2 = 0.999 in double: rel err {kr.max_err(vd.out[:, 0], nud) / nud.abs().max().item():.3e} (not asserted), "
                      f"params {kr.max_err(pd.out[:, 0], pdbl['w']):.3e}")
            if not bool(gr.any()):   # zero gradient: gnorm 0, the moments only decay (one fp32 product each)
                assert gn.out.item() == 0
                assert torch.equal(md.out, before[1] * B1) and torch.equal(vd.out, before[2] * B2)


def test_clip_adam_zero_gradient_from_a_fresh_state(L, stream):
    n = 5000
    p = torch.randn(n, generator=torch.Generator().manual_seed(3))
    pd, md, vd = _filled(p), _filled(torch.zeros(n)), _filled(torch.zeros(n))
    ws, gn = Guard(1024, 1, dtype=D, fill=0.0), Guard(1, 1)
    L.call("magpo_clip_adam", pd, dev(torch.zeros(n)), md, vd, n, 0.5, MAX_NORM, LR, B1, B2, EPS, 0.1, 0.001, ws, gn, stream)
    _sync()
    for gd in (pd, md, vd, ws, gn):
        gd.check("clip_adam zero gradient")
    assert torch.equal(pd.out[:, 0].cpu(), p) and bool((md.out == 0).all()) and bool((vd.out == 0).all()) and gn.out.item() == 0


# ================================================================================================ magpo_gather_minibatch
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("T,N,A,F,K,mb", [(6, 10, 4, 5, 20, 5), (1, 4, 1, 1, 3, 4), (3, 40, 8, 75, 5, 13), (5, 6, 3, 75, 20, 6), (1, 300, 1, 5, 64, 300),
                                          (7, 9, 1, 1, 1, 2)])
def test_gather_minibatch_every_output(L, stream, T, N, A, F, K, mb, masked):
    """Every output against the take / transpose / reshape route of rec_magpo.py:441-462; the float fields are distinct per field, so a
    swap shows.  A = 1, T = 1, mb = N, the wide F of Connector / MPE observations, more rows than one block."""
    c = kr.gather_case(T, N, A, F, K, mb, 13 + T + N, masked)
    ref = kr.gather_ref(c)
    R = mb * T * A
    i32 = torch.int32
    o = dict(obs=Guard(R, F), action=Guard(R, 1, dtype=i32), prev=Guard(R, 1, dtype=i32), pos=Guard(R, 1, dtype=i32), done=ByteGuard(mb * T, 1),
             mask=ByteGuard(R, K), value=Guard(R, 1), logp=Guard(R, 1), adv=Guard(R, 1), targets=Guard(R, 1), h0idx=Guard(mb * A, 1, dtype=i32))
    L.call("magpo_gather_minibatch", dev(c["obs"]), dev(c["action"]), dev(c["stepcount"]), dev(c["done"]), dev(c["mask"]), dev(c["value"]), dev(c["logp"]),
           dev(c["adv"]), dev(c["targets"]), dev(c["env_idx"]), dev(c["agent_perm"]), o["obs"], o["action"], o["prev"], o["pos"], o["done"], o["mask"],
           o["value"], o["logp"], o["adv"], o["targets"], o["h0idx"], T, N, A, F, K, mb, stream)
    _sync()
    what = f"gather T={T} N={N} A={A} F={F} K={K} mb={mb} masked={masked}"
    for n, gd in o.items():
        if n == "mask" and not masked:
            gd.check(f"{what} {n} (no mask given: o_mask stays untouched)", written=False)
            continue
        gd.check(f"{what} {n}")
        got, want = gd.out.cpu(), ref[n]
        assert torch.equal(got.reshape(want.shape), want), f"{what}: {n} differs"


# ================================================================================================ magpo_reduce_slabs, magpo_wgrad, magpo_linear
@pytest.mark.parametrize("G", [1, 15, 16, 17, 48, 49, 63, 64, 65, 200, 1024])
def test_reduce_slabs_arms(L, stream, G):
    """out = (accumulate ? out : 0) + scale * sum_g slab[g]: the four-way unrolled arm (g + 48 < G), its 16-step tail, P around the
    64-column block, strided slabs, and the product's accumulate = 1.  Two runs are bit-identical."""
    for P in (1, 63, 64, 65, 5000):
        for stride in (P, P + 12):
            g = torch.Generator().manual_seed(G * 7 + P)
            slab = torch.randn(G, stride, generator=g)
            before = torch.randn(P, generator=g)
            sd = dev(slab)
            for scale in (1.0, 0.5):
                for acc in (0, 1):
                    what = f"reduce_slabs G={G} P={P} stride={stride} scale={scale} accumulate={acc}"
                    outs = []
                    for _ in range(2):
                        out = Guard(1, P, fill=0.0 if acc else None)
                        if acc:
                            out.out[0] = before.to(DEV)
                        L.call("magpo_reduce_slabs", sd, out, G, P, stride, scale, acc, stream)
                        _sync()
                        out.check(what)
                        outs.append(out.out[0].clone())
                    assert torch.equal(outs[0], outs[1]), f"{what}: two runs differ"
                    check_sum(what, outs[0], kr.reduce_slabs_ref(slab.double(), P, before.double(), scale, acc), kr.reduce_slabs_ref(slab, P, before, scale, acc))


@pytest.mark.parametrize("KIN,NOUT,R,G", [(64, 64, 1000, 7), (128, 384, 64 * 256 + 37, 200)])
def test_wgrad_accumulate(L, stream, KIN, NOUT, R, G):
    """accumulate = 1 onto a non-zero dW / db: out = before + scale * X^T dY (split kernel and whole-matrix kernel)."""
    g = torch.Generator().manual_seed(21)
    X, dY = torch.randn(R, KIN, generator=g) * 0.1, torch.randn(R, NOUT, generator=g) * 0.1
    W0, b0 = torch.randn(KIN, NOUT, generator=g), torch.randn(NOUT, generator=g)
    ws = torch.empty(L.call("magpo_wgrad_workspace_floats", KIN, NOUT, G), device=DEV)
    dW, db = Guard(KIN, NOUT, fill=0.0), Guard(1, NOUT, fill=0.0)
    dW.out[:], db.out[0] = W0.to(DEV), b0.to(DEV)
    L.call("magpo_wgrad", dev(X), KIN, dev(dY), NOUT, R, KIN, KIN, NOUT, dW, db, ws, G, 0.5, 1, 0, stream)
    _sync()
    dW.check("wgrad accumulate dW"); db.check("wgrad accumulate db")
    f = lambda dt: (W0.to(dt) + 0.5 * (X.to(dt).T @ dY.to(dt)), b0.to(dt) + 0.5 * dY.to(dt).sum(0))
    (w64, b64), (w32, b32) = f(D), f(torch.float32)
    check_sum(f"wgrad accumulate {KIN}x{NOUT} dW", dW.out, w64, w32); check_sum(f"wgrad accumulate {KIN}x{NOUT} db", db.out[0], b64, b32)


@pytest.mark.parametrize("KIN,NOUT,R,G,krows", [(64, 20, 500, 7, 5), (64, 256, 16384, 256, 33)])
def test_wgrad_krows(L, stream, KIN, NOUT, R, G, krows):
    """krows < KIN: only the first krows rows of dW are written (the guard rows behind them are what rows krows .. KIN would be), on one
    split-kernel and one whole-matrix shape; db is complete."""
    g = torch.Generator().manual_seed(22)
    X, dY = torch.randn(R, KIN, generator=g) * 0.1, torch.randn(R, NOUT, generator=g) * 0.1
    ws = torch.empty(L.call("magpo_wgrad_workspace_floats", KIN, NOUT, G), device=DEV)
    dW, db = Guard(krows, NOUT), Guard(1, NOUT)
    L.call("magpo_wgrad", dev(X), KIN, dev(dY), NOUT, R, KIN, krows, NOUT, dW, db, ws, G, 1.0, 0, 0, stream)
    _sync()
    dW.check("wgrad krows dW"); db.check("wgrad krows db")
    f = lambda dt: ((X.to(dt).T @ dY.to(dt))[:krows], dY.to(dt).sum(0))
    (w64, b64), (w32, b32) = f(D), f(torch.float32)
    check_sum(f"wgrad krows={krows} {KIN}x{NOUT} dW", dW.out, w64, w32); check_sum(f"wgrad krows={krows} {KIN}x{NOUT} db", db.out[0], b64, b32)


@pytest.mark.parametrize("KIN,NOUT,R", [(64, 64, 203), (128, 100, 65), (64, 256, 130), (256, 64, 77)])
def test_linear_swish(L, stream, KIN, NOUT, R):
    """act = 3: Y = swish(X W + b) on the shared-tile kernels."""
    g = torch.Generator().manual_seed(23)
    X, W, b = torch.randn(R, KIN, generator=g), torch.randn(KIN, NOUT, generator=g) / math.sqrt(KIN), torch.randn(NOUT, generator=g)
    Wt = transpose_pad(L, stream, dev(W))
    ld = kr.ceil4(NOUT)
    Y = Guard(R, NOUT, ld)
    L.call("magpo_linear", dev(X), KIN, Wt, dev(b), Y, ld, None, R, KIN, NOUT, 3, 0, stream)
    _sync()
    Y.check("linear swish Y")
    ref = X.double() @ W.double() + b.double()
    check(f"linear swish {KIN}x{NOUT} R={R} Y", Y.out, onets.swish(ref), kr.local_bound(onets.swish(ref)))
