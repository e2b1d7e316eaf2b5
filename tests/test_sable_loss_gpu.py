"""magpo_ppo_loss_fwd_bwd (csrc/rl.hip: k_ppo_loss), the PPO loss of the guider-only system, against tests/sable_ref.ppo_loss_ref in fp64
at R in {1, 255, 256, 257, 1500} x K in {2, 5, 20, 64}, masked and unmasked, strides 64 and tight, with 0 / 1e30 / NaN behind the K valid
input columns.  Every output sits in a Guard; every comparison prints its figure before it asserts.

Error bars (the rule of tests/test_rl_kernels_gpu.py::_check_loss): per scalar and per gradient max(model bound, 4 x the error of the
plain fp32 torch restatement against fp64), model bounds kr.loss_scalar_bound / kr.loss_grad_bound.  Rows of the fp64 reference within
kr.KINK of a kink (ratio at 1 +- clip_eps, value difference at +- clip_eps, equal value-loss branches) are left out of the GRADIENT
comparison only; at most 2 % of a case's rows (asserted here and, on the reference alone, in tests/test_sable_system.py).  The loss
scalars are continuous at every kink and are compared on all rows.  The dedicated kink case puts rows on every kink and enumerates the
one-sided gradients there."""
import pytest
import torch

from tests import kernel_refs as kr
from tests import sable_ref as sr
from tests.gpu_util import DEV, Guard, dev

pytestmark = pytest.mark.gpu
D = torch.float64
S = kr.SYSC
U8 = torch.uint8
FILLS = {"zero": 0.0, "1e30": 1e30, "nan": float("nan")}


def _run(L, stream, c, fill, what, strides=None):
    """One adv_moments + PPO loss call on the case with `fill` in the input columns >= K; the guarded outputs after their checks."""
    R, K = c["R"], c["K"]
    ld, lddl = strides or c["strides"]
    logits = torch.full((R, ld), fill)
    logits[:, :K] = c["gl"]
    stats = Guard(1, 2)
    ws = Guard(1024, 8, dtype=D, fill=0.0)            # exactly the 8 * 1024 doubles the header asks for
    L.call("magpo_adv_moments", dev(c["adv"]), R, ws, stats, stream)
    dl, dv, lo = Guard(R, min(lddl, 64), lddl), Guard(R, 1), Guard(1, 4)
    L.call("magpo_ppo_loss_fwd_bwd", dev(logits), ld, dev(c["legal"].to(U8)) if c["masked"] else None, dev(c["action"].int()), dev(c["old"]),
           dev(c["vold"]), dev(c["value"]), dev(c["adv"]), dev(c["tgt"]), stats.out, dl, lddl, dv, ws, lo, R, K, S.clip_eps, S.ent_coef,
           S.vf_coef, stream)
    torch.cuda.synchronize()
    for g, n in ((stats, "adv_stats"), (ws, "workspace"), (dl, "dlogits"), (dv, "dvalue"), (lo, "loss_out")):
        g.check(f"{what} {n}")
    return dict(dl=dl, dv=dv, lo=lo)


def _check_scalars(what, r64, r32, out):
    lo = out["lo"].out[0].cpu().double()
    fails = []
    for j, name in enumerate(sr.PPO_LOSS_NAMES):
        ref = r64["loss"][j].item()
        e32, err = abs(r32["loss"][j].item() - ref), abs(lo[j].item() - ref)
        bound = max(kr.loss_scalar_bound(r64, j), 4.0 * e32)
        print(f"PPOLOSSERR {what} {name}: fp32-torch err {e32:.3e} kernel err {err:.3e} ratio {err / max(e32, 1e-300):.2f} bound {bound:.3e} ref {ref:.3e}")
        if not err <= bound:
            fails.append(f"{name}: err {err:.3e} > bound {bound:.3e}")
    return fails


def _check_zeros(what, c, out):
    """Exact zeros: illegal columns, the columns K .. min(lddl, 64), and every column of a row with one legal action."""
    K, legal, o = c["K"], c["legal"], out["dl"].out
    assert bool((o[:, K:] == 0).all()), f"{what}: columns >= K must be exactly 0"
    assert bool((o[:, :K][~legal.to(DEV)] == 0).all()), f"{what}: illegal columns must be exactly 0"
    assert bool((o[(legal.sum(1) == 1).to(DEV)] == 0).all()), f"{what}: a row with one legal action has no gradient"


def _check(what, c, r64, r32, out):
    R, K = c["R"], c["K"]
    near = sr.ppo_near_kink(r64)
    ok = ~near
    print(f"PPOLOSSKINK {what}: near-kink rows {int(near.sum())} / {R} left out of dlogits / dvalue")
    assert int(near.sum()) <= 0.02 * R
    fails = _check_scalars(what, r64, r32, out)
    for n in ("dl", "dv"):
        got = (out[n].out[:, :K] if n == "dl" else out[n].out[:, 0]).cpu()
        ref, ref32 = r64[n][ok], r32[n][ok]
        if ref.numel() == 0:
            continue
        e32, err = kr.max_err(ref32, ref), kr.max_err(got[ok], ref)
        bound = max(kr.loss_grad_bound(r64, n, ok), 4.0 * e32)
        print(f"PPOLOSSERR {what} {n}: fp32-torch err {e32:.3e} kernel err {err:.3e} ratio {err / max(e32, 1e-300):.2f} bound {bound:.3e} "
              f"ref {ref.abs().max().item():.3e}")
        if not err <= bound:
            fails.append(f"{n}: err {err:.3e} > bound {bound:.3e}")
    assert not fails, f"{what}: {fails}"
    _check_zeros(what, c, out)


@pytest.mark.parametrize("i", range(len(sr.PPO_MATRIX)), ids=[sr.ppo_case_id(i) for i in range(len(sr.PPO_MATRIX))])
def test_ppo_loss_matrix(L, stream, i):
    """Every case with zeros behind the K valid input columns against fp64, then with 1e30 and NaN there: bit for bit the zero-filled
    result (the vector branch loads those columns and has to discard them; the tight strides have no such columns and repeat the run)."""
    c, r64, r32 = sr.ppo_matrix_case(i)
    base = _run(L, stream, c, 0.0, c["name"])
    _check(c["name"], c, r64, r32, base)
    for fill in ("1e30", "nan"):
        out = _run(L, stream, c, FILLS[fill], f"{c['name']} fill={fill}")
        for n in ("lo", "dl", "dv"):
            assert torch.equal(out[n].full, base[n].full), f"{c['name']} fill={fill}: {n} differs from the zero-filled run"


@pytest.mark.parametrize("strides", ["s64", "tight"])
def test_ppo_loss_single_legal_rows_only(L, stream, strides):
    """Every row has one legal action: log-prob 0 there, so the entropy and all logit gradients are exactly 0, the ratio is exp(-old) and
    the value loss is untouched by the mask."""
    R, K = 1500, 20
    c = sr.ppo_case(R, K, 77, mask_p=0.6, one_legal=1.0)
    assert bool((c["legal"].sum(1) == 1).all())
    r64, r32 = sr.ppo_loss_ref(c), sr.ppo_loss_ref(c, torch.float32)
    what = f"ppo single-legal-only {strides}"
    out = _run(L, stream, c, 1e30, what, sr.ppo_strides(strides, K))
    _check(what, c, r64, r32, out)
    assert out["lo"].out[0, 2].item() == 0, out["lo"].out
    assert bool((out["dl"].out == 0).all())


def test_ppo_loss_on_the_kinks(L, stream):
    """Rows ON every kink (sr.ppo_kink_case).  Loss scalars: continuous there, compared as everywhere.  Gradients: the rows off the kinks
    as everywhere; a row on a kink must carry one of the enumerated one-sided gradients (sr.ppo_kink_candidates), within the same bound."""
    c, groups = sr.ppo_kink_case()
    c["strides"] = (64, 64)
    r64, r32 = sr.ppo_loss_ref(c), sr.ppo_loss_ref(c, torch.float32)
    out = _run(L, stream, c, 0.0, "ppo kinks")
    fails = _check_scalars("ppo kinks", r64, r32, out)
    assert not fails, fails
    _check_zeros("ppo kinks", c, out)
    on = sr.ppo_near_kink(r64)
    off = ~on
    got_dl, got_dv = out["dl"].out[:, :c["K"]].cpu().double(), out["dv"].out[:, 0].cpu().double()
    b_dl = max(kr.loss_grad_bound(r64, "dl", off), 4.0 * kr.max_err(r32["dl"][off], r64["dl"][off]))
    b_dv = max(kr.loss_grad_bound(r64, "dv", off), 4.0 * kr.max_err(r32["dv"][off], r64["dv"][off]))
    e_dl, e_dv = kr.max_err(got_dl[off], r64["dl"][off]), kr.max_err(got_dv[off], r64["dv"][off])
    print(f"PPOLOSSERR ppo kinks (rows off the kinks) dl: kernel err {e_dl:.3e} bound {b_dl:.3e}; dv: kernel err {e_dv:.3e} bound {b_dv:.3e}")
    assert e_dl <= b_dl and e_dv <= b_dv
    cand_dl, cand_dv = sr.ppo_kink_candidates(c, r64)
    taken = {}
    for name, sl in groups.items():
        rows = torch.arange(c["R"])[sl]
        assert bool(on[rows].all()), name
        d_dl = (cand_dl[:, rows] - got_dl[rows][None]).abs().amax(2)      # [candidate, row]
        d_dv = (cand_dv[:, rows] - got_dv[rows][None]).abs()
        taken[name] = (d_dl.argmin(0).bincount(minlength=3).tolist(), d_dv.argmin(0).bincount(minlength=6).tolist())
        print(f"PPOLOSSKINK {name}: worst distance to the nearest one-sided gradient dl {d_dl.min(0).values.max().item():.3e} (bound {b_dl:.3e}) "
              f"dv {d_dv.min(0).values.max().item():.3e} (bound {b_dv:.3e}); candidates taken dl {taken[name][0]} dv {taken[name][1]}")
        assert float(d_dl.min(0).values.max()) <= b_dl, name
        assert float(d_dv.min(0).values.max()) <= b_dv, name


def test_magpo_loss_at_equal_logits_gives_the_ppo_gradients(L, stream):
    """magpo_loss_fwd_bwd with a_logits = g_logits: dg and dvalue are the PPO kernel's (the log-ratio is 0, so no KL mask and
    clipped_ratio == ratio), each within its bound of fp64 and of the other."""
    for i in (sr.PPO_MATRIX.index((1500, 20, True, "s64")), sr.PPO_MATRIX.index((257, 5, False, "s64"))):
        c, r64, r32 = sr.ppo_matrix_case(i)
        R, K = c["R"], c["K"]
        ppo = _run(L, stream, c, 0.0, c["name"])
        logits = torch.zeros(R, 64)
        logits[:, :K] = c["gl"]
        stats, ws = Guard(1, 2), Guard(1024, 8, dtype=D, fill=0.0)
        L.call("magpo_adv_moments", dev(c["adv"]), R, ws, stats, stream)
        dg, da, dv, lo = Guard(R, 64), Guard(R, 64), Guard(R, 1), Guard(1, 9)
        ld = dev(logits)
        L.call("magpo_loss_fwd_bwd", ld, 64, ld, 64, dev(c["legal"].to(U8)) if c["masked"] else None, dev(c["action"].int()), dev(c["old"]),
               dev(c["vold"]), dev(c["value"]), dev(c["adv"]), dev(c["tgt"]), stats.out, dg, 64, da, 64, dv, ws, lo, R, K, S.clip_eps, S.clip_gpo,
               S.ent_coef, S.vf_coef, S.alpha, stream)
        torch.cuda.synchronize()
        ok = ~sr.ppo_near_kink(r64)
        for n, got, other in (("dl", dg.out[:, :K].cpu(), ppo["dl"].out[:, :K].cpu()), ("dv", dv.out[:, 0].cpu(), ppo["dv"].out[:, 0].cpu())):
            bound = max(kr.loss_grad_bound(r64, n, ok), 4.0 * kr.max_err(r32[n][ok], r64[n][ok]))
            e_ref, e_other = kr.max_err(got[ok], r64[n][ok]), kr.max_err(got[ok], other[ok].double())
            print(f"PPOLOSSERR {c['name']} magpo-loss-at-equal-logits {n}: err vs fp64 {e_ref:.3e}, vs the PPO kernel {e_other:.3e}, bound {bound:.3e}")
            assert e_ref <= bound and e_other <= bound
        # the guider scalars of the MAGPO loss are the PPO scalars: guider_loss = actor_loss, entropy, value_loss
        m, p = lo.out[0].cpu().double(), ppo["lo"].out[0].cpu().double()
        for a, b, j in ((m[3], p[1], 1), (m[5], p[2], 2), (m[1], p[3], 3)):
            assert abs(a.item() - b.item()) <= kr.loss_scalar_bound(r64, j) * 2, (j, a, b)
        assert m[4].item() == 0      # no row is outside the GPO clip at equal logits


def test_ppo_loss_rejects_bad_arguments(L, stream):
    """Everything the host rejects before any launch: K > 64, K above a stride, a gradient stride that is no multiple of 4, no rows (R = 0: a mean
    over nothing).  Nothing is written."""
    R, K = 8, 20
    c = sr.ppo_case(R, K, 1)
    x = dev(torch.zeros(R + 2, 72))
    stats = dev(torch.tensor([0.0, 1.0]))
    ws = Guard(1024, 8, dtype=D, fill=0.0)
    dl, dv, lo = Guard(R, 72), Guard(R, 1), Guard(1, 4)
    vec = [dev(c[n]) for n in ("old", "vold", "value", "adv", "tgt")]
    for R_, K_, ld, lddl in ((R, 65, 72, 72), (R, 20, 16, 64), (R, 20, 64, 16), (R, 20, 64, 22), (R, 20, 64, 30), (R, 3, 64, 2), (0, 20, 64, 64)):
        with pytest.raises(ValueError):
            L.call("magpo_ppo_loss_fwd_bwd", x, ld, None, dev(c["action"].int()), vec[0], vec[1], vec[2], vec[3], vec[4], stats, dl, lddl, dv, ws, lo,
                   R_, K_, S.clip_eps, S.ent_coef, S.vf_coef, stream)
        torch.cuda.synchronize()
        for g in (dl, dv, lo):
            g.check("a rejected call writes nothing", defined=torch.zeros(g.R, dtype=torch.bool))
            assert bool(torch.isnan(g.out).all())
        ws.check("a rejected call writes nothing")
        assert bool((ws.out == 0).all())
