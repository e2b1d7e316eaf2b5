"""The fp64 references of tests/kernel_refs.py checked on the CPU: against a second route through oracle.networks where one exists, and
their plain fp32 restatement against every tolerance of the GPU modules with a margin of 2 (so a GPU failure is the kernel's)."""
import pytest
import torch

from oracle import networks as onets
from tests import kernel_refs as kr

D = torch.float64


def _close(a, b, tol=1e-12):
    assert kr.max_err(a, b) <= tol * max(1.0, b.abs().max().item()), kr.max_err(a, b)


@pytest.mark.parametrize("s2", [True, False])
def test_seg_post_tail3_equals_oracle_decoder_tail(s2):
    """msr_recurrent with w_q = w_g = I, w_v = 0 and an identity state returns (swish(key) * GroupNorm(query)) w_o: the oracle's own
    retention epilogue; the rest of the decoder block (sable_network.py:214-215 with zero FFN weights) and _logit_head follow."""
    R, K = 50, 7
    c = kr.seg_case(R, 1, tail=3, K=K, s2=s2)
    eye = torch.eye(64, dtype=D)
    p = {"w_q": eye[None], "w_k": eye[None], "w_v": torch.zeros(1, 64, 64, dtype=D), "w_g": eye, "w_o": c["wo"].to(D),
         "gn.scale": c["gamma"].to(D), "gn.bias": c["beta"].to(D)}
    y, _ = onets.msr_recurrent(p, "", c["gp"].to(D)[:, None], c["r"].to(D)[:, None], c["r"].to(D)[:, None],
                               eye[None, None].expand(R, 1, 64, 64), None, nh=1, use_pe=False)
    x = onets.rmsnorm(c["res"].to(D) + y[:, 0], c["s1"].to(D))
    if s2:
        x = onets.rmsnorm(x, c["s2"].to(D))
    hp = {"dec.head.dense0.kernel": c["w0"].to(D), "dec.head.dense0.bias": c["b0"].to(D), "dec.head.norm.scale": c["hs"].to(D),
          "dec.head.dense1.kernel": c["w1"].to(D), "dec.head.dense1.bias": c["b1"].to(D)}
    ref = kr.seg_post(3, c)
    _close(ref["y"], y[:, 0]); _close(ref["o"], x); _close(ref["logits"][:, :K], onets._logit_head(hp, x))
    assert ref["logits"][:, K:].abs().max().item() == 0
    _close(ref["ope"], x + c["pe"].to(D)[c["pos"].long().clamp(0, 100)])


def test_seg_post_tail1_equals_oracle_value_head():
    c = kr.seg_case(40, 2, tail=1, nq2=4)
    ref = kr.seg_post(1, c)
    h = onets.rmsnorm(onets.gelu(ref["out0"]), c["hs"].to(D))
    _close(ref["value"], h @ c["hw"].to(D) + c["hb1"].to(D))
    for k in range(4):
        _close(ref[f"q2_{k}"], ref["ope"] @ c["q2w"][k].to(D))


@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_seg_rows_table_equals_gather_then_dense(tail):
    c = kr.seg_case(100, 3 + tail, tail=tail, nq2=2, rows=True)
    g = dict(c, gp=c["gp"][c["rows"].long()], res=c["res"][c["rows"].long()], rows=None)
    a, b = kr.seg_post(tail, c), kr.seg_post(tail, g)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    a, b = kr.seg_bwd(c), kr.seg_bwd(g)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_seg_bwd_presum_value_equals_sum():
    """presum mode: the forward value is that of the sum given as `res`; gradients of r / gp still flow through y = u W_o."""
    c = kr.seg_case(30, 9)
    y = kr.seg_post(0, c)["y"].float()
    a, b = kr.seg_bwd(c), kr.seg_bwd(dict(c, res=c["res"] + y), presum=True)
    for k in a:
        assert kr.max_err(a[k], b[k]) <= 1e-5 * max(1.0, a[k].abs().max().item()), k   # (y rounded to fp32)


@pytest.mark.parametrize("nh", [1, 4])
def test_retention_recurrent_equals_msr_recurrent(nh):
    """One head (and four heads of 16 channels, groups of 4): identity projections, decay 1, gate input = the key."""
    N, ntok, E = 5, 6, 64
    hs = E // nh
    g = torch.Generator().manual_seed(4)
    x = {n: torch.randn(N, ntok, E, generator=g, dtype=D) for n in "qkv"}
    S = torch.randn(N, nh, hs, hs, generator=g, dtype=D)
    gamma, beta = 1 + 0.1 * torch.randn(hs, generator=g, dtype=D), 0.1 * torch.randn(hs, generator=g, dtype=D)
    proj = torch.stack([torch.eye(E, dtype=D)[:, h * hs:(h + 1) * hs] for h in range(nh)])
    p = {"w_q": proj, "w_k": proj, "w_v": proj, "w_g": torch.eye(E, dtype=D), "w_o": torch.eye(E, dtype=D), "gn.scale": gamma, "gn.bias": beta}
    out, newh = onets.msr_recurrent(p, "", x["k"], x["q"], x["v"], S, None, nh=nh, use_pe=False)
    for h in range(nh):
        sl = slice(h * hs, (h + 1) * hs)
        Sn, r = kr.retention_recurrent(S[:, h], x["q"][..., sl], x["k"][..., sl], x["v"][..., sl], 1.0, 0, x["k"][..., sl], gamma, beta, hs // nh)
        _close(Sn, newh[:, h]); _close(r, out[..., sl])
    # ret_from only selects the returned tokens
    _, r2 = kr.retention_recurrent(S[:, 0], x["q"][..., :hs], x["k"][..., :hs], x["v"][..., :hs], 0.7, 3)
    _, r0 = kr.retention_recurrent(S[:, 0], x["q"][..., :hs], x["k"][..., :hs], x["v"][..., :hs], 0.7, 0)
    assert torch.equal(r2, r0[:, 3:])


def test_retention_padded_state():
    c = kr.retention_case(3, 5, 16, 5)
    Sn = kr.retention_padded_state(c, 0.8, 16)
    k, v = torch.zeros(3, 5, 64, dtype=D), torch.zeros(3, 5, 64, dtype=D)
    k[..., :16], v[..., :16] = c["k"], c["v"]
    _close(Sn, 0.8 * c["S"].to(D) + k.transpose(1, 2) @ v)


@pytest.mark.parametrize("pro", [1, 2, 3, 4])
def test_linear_pro_equals_oracle_pieces(pro):
    c = kr.linear_pro_case(pro, 60, 20, 10 + pro)
    row, outpe, Y = kr.linear_pro(pro, c, True)
    if pro == 2:
        x = c["a"][:, :5].to(D)
        x = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * c["s_obs"].to(D)
        _close(row, onets.rmsnorm(onets.gelu(x @ c["W"].to(D)), c["s1"].to(D)))
    if pro == 3:
        _close(row, onets.rmsnorm(onets.rmsnorm(c["a"].to(D) + c["y"].to(D), c["s1"].to(D)), c["s2"].to(D)))
    _close(outpe - row, c["pe"].to(D)[c["pos"].long().clamp(0, 100)], 1e-9)
    _close(Y, outpe @ c["Wd"].to(D) + c["bias"].to(D))
    _close(kr.linear_pro(pro, c, False)[2], row @ c["Wd"].to(D) + c["bias"].to(D))


def test_obsnorm_bwd_equals_header_formula():
    c = kr.obsnorm_case(200, 75, 160, 6)
    obs, don = c["obs"].to(D), c["don"].to(D)
    x = obs[:, :75]
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6)
    _close(kr.obsnorm_bwd(obs, 75, c["s_obs"].to(D), don), (don[:, :75] * x * rstd).sum(0))
    on = kr.obsnorm_fwd(obs, 75, c["s_obs"].to(D))
    assert on[:, 75:].abs().max().item() == 0 and torch.isfinite(on).all()


def test_small_relu_wgrad_equals_autograd():
    g = torch.Generator().manual_seed(7)
    X, dY = torch.randn(300, 9, generator=g, dtype=D), torch.randn(300, 128, generator=g, dtype=D)
    W = torch.randn(9, 128, generator=g, dtype=D).requires_grad_(True); b = torch.randn(128, generator=g, dtype=D).requires_grad_(True)
    Y = torch.relu(X @ W + b)
    (Y * dY).sum().backward()
    dW, db = kr.small_relu_wgrad(X, 9, Y.detach(), dY)
    _close(dW, W.grad); _close(db, b.grad)


def test_small_operand_modes():
    g = torch.Generator().manual_seed(8)
    obs = torch.randn(20, 12, generator=g); s = 1 + 0.1 * torch.randn(5, generator=g); idx = torch.randint(0, 64, (20,), generator=g)
    assert torch.equal(kr.small_operand(2, obs, 5)[:, :5], obs[:, :5]) and kr.small_operand(2, obs, 5)[:, 5:].abs().max() == 0
    assert torch.equal(kr.small_operand(0, obs, 5, s)[:, :5], onets.rmsnorm(obs[:, :5], s))
    oh = kr.small_operand(1, None, 0, idx=idx)
    assert oh.shape == (20, 64) and torch.equal(oh.argmax(1), idx) and oh.sum().item() == 20


@pytest.mark.parametrize("A,K,maxval,npos", [(4, 20, 60, 101), (3, 10, 30, 7), (8, 15, 100, 1)])
def test_coordsum_class_tables_reproduce_the_rows(A, K, maxval, npos):
    obs, prev, pos = kr.coordsum_case(A, K, maxval, 50, npos, 9)
    assert obs[:, :A].sum(1).eq(1).all() and obs[:, A].max() < maxval
    enc, dec = kr.coordsum_classes(obs, prev, pos, A, maxval, npos)
    obs_tab, pos_enc, prev_dec, pos_dec = kr.coordsum_class_rows(A, maxval, npos, K)
    pc = pos.long().clamp(0, npos - 1)
    assert torch.equal(obs_tab[enc], obs) and torch.equal(pos_enc[enc], pc)
    assert torch.equal(prev_dec[dec], prev.long()) and torch.equal(pos_dec[dec], pc)
    enc1, dec1 = kr.coordsum_classes(obs, None, None, A, maxval, 1)
    assert dec1 is None and torch.equal(enc1, enc // npos)


# ---- the plain fp32 restatement passes every token-local tolerance of the GPU modules with a margin of 2
def _margin(ref64, ref32, rtol=2e-5, atol=2e-6, what=""):
    err, bound = kr.max_err(ref32, ref64), kr.local_bound(ref64, rtol, atol)
    assert 2 * err <= bound, f"{what}: fp32 restatement error {err:.3e} against bound {bound:.3e}"


@pytest.mark.parametrize("tail,K,nq2", [(0, 1, 0), (1, 1, 4), (2, 1, 0), (3, 1, 0), (3, 31, 0), (3, 64, 0)])
@pytest.mark.parametrize("R", [17, 1000, 3 * 16384 + 7])
def test_fp32_margin_seg(tail, K, nq2, R):
    if R > 1000 and (tail, K) not in ((1, 1), (3, 31)):
        R = 1000 + tail   # the big row counts run for the two combinations the GPU module runs them for
    for s2, rows in ((True, False), (False, True)):
        c = kr.seg_case(R, 100 + tail, tail=tail, K=K, nq2=nq2, s2=s2, rows=rows)
        a, b = kr.seg_post(tail, c), kr.seg_post(tail, c, torch.float32)
        for k in a:
            _margin(a[k], b[k], what=f"seg_post {k}")
        a, b = kr.seg_bwd(c), kr.seg_bwd(c, torch.float32)
        for k in ("dsum", "dr", "dgp"):
            _margin(a[k], b[k], 1e-4, 1e-5, f"seg_bwd {k}")


@pytest.mark.parametrize("hs,gs", [(16, 4), (16, 16), (32, 4), (32, 16), (32, 32), (64, 4), (64, 16), (64, 64)])
@pytest.mark.parametrize("ntok", [1, 2, 8, 16, 17, 23, 32])
def test_fp32_margin_retention(ntok, hs, gs):
    c = kr.retention_case(37, ntok, hs, 1000 + ntok)
    f = lambda dt, gate: kr.retention_recurrent(c["S"][:, :hs, :hs].to(dt), c["q"].to(dt), c["k"].to(dt), c["v"].to(dt), 0.775, 0,
                                                *((c["gp"].to(dt), c["gamma"].to(dt), c["beta"].to(dt), gs) if gate else ()))
    for gate in (False, True):
        (S64, r64), (S32, r32) = f(D, gate), f(torch.float32, gate)
        _margin(S64, S32, what="state"); _margin(r64, r32, what=f"ret gate={gate}")


@pytest.mark.parametrize("pro", [1, 2, 3, 4])
@pytest.mark.parametrize("NOUT", [20, 256])
def test_fp32_margin_linear_pro(pro, NOUT):
    c = kr.linear_pro_case(pro, 1000, NOUT, 50 + pro)
    c32 = {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    for use_pe in (True, False):
        for a, b, what in zip(kr.linear_pro(pro, c, use_pe), kr.linear_pro(pro, c32, use_pe, torch.float32), ("row", "outpe", "Y")):
            _margin(a, b, what=what)


@pytest.mark.parametrize("F", [1, 33, 75, 127, 128])
def test_fp32_margin_obsnorm(F):
    c = kr.obsnorm_case(5003, F, 160, 20 + F)
    _margin(kr.obsnorm_fwd(c["obs"].to(D), F, c["s_obs"].to(D)), kr.obsnorm_fwd(c["obs"], F, c["s_obs"]), what="on")


# ================================================================================================ RL-side kernels (tests/test_rl_kernels_gpu.py)
import math

import numpy as np

from oracle import learner as olearn
from oracle import prng as oprng

LOSS_IDS = [kr.loss_case_id(i) for i in range(len(kr.LOSS_MATRIX))]


def test_loss_matrix_covers_what_it_must():
    """Every value of every dimension, every valid pair of two dimensions, and the grid-stride row count at production strides with K = 20
    and K = 64."""
    M = kr.LOSS_MATRIX
    assert len(set(M)) == len(M)
    assert {c[0] for c in M} == {"s64", "s32", "tight", "mixed", "s72"}
    assert {c[1] for c in M} == {1, 2, 5, 6, 20, 31, 32, 33, 63, 64}
    assert {c[2] for c in M} == {1, 3, 15, 16, 17, 1500, kr.GRID_STRIDE_R}
    assert {c[3] for c in M} == set(kr.LOSS_MASKS) and {c[4] for c in M} == set(kr.LOSS_DISTS)
    for K in (20, 64):
        assert any(c[:3] == ("s64", K, kr.GRID_STRIDE_R) for c in M)
    have = {(i, c[i], j, c[j]) for c in M for i in range(5) for j in range(i + 1, 5)}
    for s in ("s64", "s32", "tight", "mixed", "s72"):
        for K in (1, 2, 5, 6, 20, 31, 32, 33, 63, 64):
            assert ((0, s, 1, K) in have) == (K <= min(kr.loss_strides(s, K))), (s, K)
        for R in (1, 3, 15, 16, 17, 1500):
            assert (0, s, 2, R) in have
    for K in (1, 2, 5, 6, 20, 31, 32, 33, 63, 64):
        for R in (1, 3, 15, 16, 17, 1500):
            assert (1, K, 2, R) in have
        for m in kr.LOSS_MASKS:
            assert (1, K, 3, m) in have
        for d in kr.LOSS_DISTS:
            assert (1, K, 4, d) in have
    for d in kr.LOSS_DISTS:
        for m in kr.LOSS_MASKS:
            assert ("s64", 20, 1500, m, d) in M
    assert kr.loss_strides("tight", 5) == (5, 5, 8, 8) and kr.loss_strides("tight", 64) == (64, 64, 64, 64)


@pytest.mark.parametrize("i", range(len(kr.LOSS_MATRIX)), ids=LOSS_IDS)
def test_loss_case(i):
    """Per case of the matrix: the exclusion cap (a condition on the case, not a measurement), no crossing rows, the branch populations,
    the structure of the masked reference, and the fp32 restatement inside every bound of the GPU test with a margin of 2."""
    c, r64, r32 = kr.loss_matrix_case(i)
    R, K = c["R"], c["K"]
    near = kr.loss_near_kink(r64)
    nnear = int(near.sum())
    cap = int(R * 1e-3) if R >= 1000 else 0
    assert nnear <= cap, f"{nnear} rows of {R} within {kr.KINK} of a kink (cap {cap}): give the case another seed (LOSS_SEED_BUMP)"
    assert int(kr.loss_crossings(r64, c).sum()) == 0, "a row where branches with different gradients cross: give the case another seed"
    slack = float(r64["kl"][near].sum()) / R
    print(f"LOSSCASE {c['name']}: near-kink rows {nnear} / {R}, kl slack {slack:.3e}")
    # inputs: the stored old log-prob is within the 0.1 noise of the guider's; illegal logits are ILLEGAL; exp(a_logp - old) stays small
    legal = c["legal"]
    assert bool((c["gl"][~legal] == kr.ILLEGAL).all()) and bool((c["al"][~legal] == kr.ILLEGAL).all())
    assert bool(legal.gather(1, c["action"][:, None]).all())
    assert r64["ra"].max().item() < 1e3 and r64["ratio"].max().item() < 2
    if c["dist"] == "constadv" or R == 1:
        assert bool((r64["A_"] == 0).all()) and bool((r32["A_"] == 0).all())
        # with a zero advantage the guider gradient is that of the KL and entropy terms alone
        gl = c["gl"].double().requires_grad_(True)
        glp, alp = onets.masked_log_softmax(gl, legal), onets.masked_log_softmax(c["al"].double(), legal)
        pr = glp.exp()
        ent = -torch.where(pr == 0, torch.zeros_like(pr), pr * glp).sum(-1)
        kmask = (r64["d"].abs() > math.log(kr.SYSC.clip_gpo)).double()
        (g,) = torch.autograd.grad((olearn._kl(glp, alp) * kmask).mean() - kr.SYSC.ent_coef * ent.mean(), [gl])
        _close(r64["dg"], g, 1e-15)
    elif R >= 1500 and K >= 2:
        pops = kr.loss_populations(r64)
        print(f"LOSSCASE {c['name']}: populations {pops}")
        assert min(pops.values()) > 0, pops
    # masked structure of the reference: gradients exactly 0 at illegal actions; a row with one legal action has log-prob 0, entropy 0
    # and no gradient at all
    for r in (r64, r32):
        assert bool((r["dg"][~legal] == 0).all()) and bool((r["da"][~legal] == 0).all())
    one = legal.sum(1) == 1
    if bool(one.any()):
        assert r64["g_logp"][one].abs().max().item() == 0 and r64["a_logp"][one].abs().max().item() == 0
        assert r64["ent"][one].abs().max().item() == 0 and r64["kl"][one].abs().max().item() == 0
        assert r64["dg"][one].abs().max().item() == 0 and r64["da"][one].abs().max().item() == 0
    if kr.LOSS_MATRIX[i][3] == "single" and R >= 1500 and K >= 20:   # (a small K has more such rows from the random mask alone)
        assert 0.1 * R <= int(one.sum()) <= 0.2 * R, int(one.sum())
    # fp32 restatement against the bounds of the GPU test, margin 2
    ok = ~near
    for n in ("dg", "da", "dv"):
        err, bound = kr.max_err(r32[n][ok], r64[n][ok]), kr.loss_grad_bound(r64, n, ok)
        assert 2 * err <= bound, f"{n}: fp32 restatement error {err:.3e} against bound {bound:.3e}"
    for j, name in enumerate(kr.LOSS_NAMES):
        err = abs(r32["loss"][j].item() - r64["loss"][j].item())
        bound = kr.loss_scalar_bound(r64, j) + (slack if j in kr.LOSS_KL_SLACK else 0.0)
        assert 2 * err <= bound, f"{name}: fp32 restatement error {err:.3e} against bound {bound:.3e}"


def test_loss_ref_scalars_add_up():
    c, r, _ = kr.loss_matrix_case(next(i for i, m in enumerate(kr.LOSS_MATRIX) if m == ("s64", 20, 1500, "single", "base")))
    s, l = kr.SYSC, r["loss"]
    _close(l[7], l[3] + l[4] - s.ent_coef * l[5] + s.vf_coef * l[1]); _close(l[8], s.alpha * l[2] + l[6]); _close(l[0], l[7] + l[8])
    ld = math.log(s.clip_gpo)
    _close(l[4], (r["kl"] * (r["d"].abs() > ld)).mean()); _close(l[6], olearn._kl(*(onets.masked_log_softmax(c[n].double(), c["legal"]) for n in ("gl", "al"))).mean())
    assert l[4].item() > 0


# ---- sampling
@pytest.mark.parametrize("K", [1, 2, 5, 20, 33, 64])
@pytest.mark.parametrize("mask", [None, "mask", "single"])
def test_sample_reference(K, mask):
    """The fp32 log-softmax is inside the GPU bound with margin 2; the oracle's sampler on masked log-probs never returns an illegal action
    and returns the only legal one of a single-legal row, whose log-prob is exactly 0."""
    c = kr.sample_case(1000, K, K + 3, 40 + K, mask, A=3)
    lp64, legal = kr.sample_lp_ref(c)
    lp32, _ = kr.sample_lp_ref(c, torch.float32)
    finite = legal
    _margin(torch.where(finite, lp64, torch.zeros_like(lp64)), torch.where(finite, lp32.double(), torch.zeros_like(lp64)), 1e-5, 1e-6, "log-softmax")
    a = torch.from_numpy(oprng.categorical(oprng.prng_key(5), lp32.numpy()[:, None, :])[:, 0]).long()
    assert bool(legal.gather(1, a[:, None]).all())
    one = legal.sum(1) == 1
    if mask == "single" and K >= 20:
        assert 100 <= int(one.sum()) <= 200
    assert bool((lp32.gather(1, a[:, None])[:, 0][one] == 0).all()) and torch.equal(a[one], legal[one].int().argmax(1))


# ---- GAE
@pytest.mark.parametrize("T,N,A,ci,done", kr.gae_matrix())
def test_gae_fp32_margin(T, N, A, ci, done):
    c = kr.gae_case(T, N, A, 7 * T + N, done)
    gamma, lam = kr.GAE_COEF[ci]
    for a, b in zip(kr.gae_ref(c, gamma, lam), kr.gae_ref(c, gamma, lam, torch.float32)):
        _margin(a, b, 1e-5, 1e-5, "gae")
    if done == "always":   # every step is the last of its episode: adv = reward - value
        _close(kr.gae_ref(c, gamma, lam)[0], c["reward"].double() - c["value"].double())


def test_gae_matrix_covers_what_it_must():
    M = kr.gae_matrix()
    assert {m[0] for m in M} == {1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 200}
    assert {m[1] * m[2] for m in M} >= {1, 7, 8191, 8192, 8193} and {m[2] for m in M} == {1, 3, 8}
    assert {(m[3], m[4]) for m in M} == {(i, d) for i in range(4) for d in kr.GAE_DONE}


# ---- advantage moments
@pytest.mark.parametrize("kind", ["normal", "100+-0.1"])
@pytest.mark.parametrize("n", [2, 255, 256, 257, 1024 * 256 + 3])
def test_adv_moments_one_pass_formula(kind, n):
    """The kernel's formula (double-precision sums, E[x^2] - mean^2) against the two-pass fp64 reference: inside the GPU bounds, margin 2."""
    x = kr.adv_moments_input(kind, n, n).double()
    mean, rstd = kr.adv_moments_ref(x)
    m1 = x.sum() / n
    r1 = 1 / (torch.sqrt(((x * x).sum() / n - m1 * m1).clamp(min=0)).float() + np.float32(1e-8))
    assert 2 * abs(m1.float().item() - mean.item()) <= 1e-7 + 1e-6 * abs(mean.item())
    assert 2 * abs(r1.item() - rstd.item()) <= 1e-5 * rstd.item()


# ---- optimiser
def test_clip_adam_reference_zero_gradient():
    p = {"w": torch.randn(100, dtype=D)}
    opt = dict(count=3, mu={"w": torch.randn(100, dtype=D)}, nu={"w": torch.rand(100, dtype=D)})
    p2, opt2, gn = olearn.clip_adam_step(p, {"w": torch.zeros(100, dtype=D)}, opt, 2.5e-4, 0.5)
    assert gn.item() == 0 and torch.equal(opt2["mu"]["w"], 0.9 * opt["mu"]["w"]) and torch.equal(opt2["nu"]["w"], 0.999 * opt["nu"]["w"])


@pytest.mark.parametrize("n", [1, 257, 5000])
def test_clip_adam_fp32_margin(n):
    """olearn.clip_adam_step in fp32 against fp64 over the five steps of every scenario: inside the GPU bounds with margin 2.  Both run
    with the decay rates as the C ABI carries them (floats): rounding 0.999 to fp32 moves 1 - b2, and with it every entry of nu, by
    1.29e-5 relative, which is the ABI's and not the arithmetic's."""
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert abs((1 - b2) / (1 - 0.999) - 1 + 1.29e-5) < 1e-7 and abs((1 - b1) / (1 - 0.9) - 1) < 3e-7
    for name, (p0, grads) in kr.adam_scenarios(n, 12 + n, 0.5).items():
        st = {dt: ({"w": p0.to(dt)}, olearn.adam_init({"w": p0.to(dt)})) for dt in (D, torch.float32)}
        for gr in grads:
            gn = {}
            for dt in st:
                p, opt, gn[dt] = olearn.clip_adam_step(st[dt][0], {"w": gr.to(dt)}, st[dt][1], 2.5e-4, 0.5, b1, b2)
                st[dt] = (p, opt)
            (p64, o64), (p32, o32) = st[D], st[torch.float32]
            if name.startswith("just"):
                assert (gn[D].item() < 0.5) == (gn[torch.float32].item() < 0.5) == (name == "just-below")
            _margin(p64["w"], p32["w"], 1e-6, 1e-7, f"{name} params")
            assert 2 * kr.max_err(o32["mu"]["w"], o64["mu"]["w"]) <= kr.ADAM_MU_RTOL * o64["mu"]["w"].abs().max().item() + 1e-30, name
            assert 2 * kr.max_err(o32["nu"]["w"], o64["nu"]["w"]) <= kr.ADAM_NU_RTOL * o64["nu"]["w"].abs().max().item() + 1e-30, name


# ---- minibatch gather
@pytest.mark.parametrize("T,N,A,F,K,mb", [(6, 10, 4, 5, 20, 5), (1, 4, 1, 1, 3, 4), (3, 40, 8, 75, 5, 13), (7, 9, 1, 1, 1, 2)])
def test_gather_ref_equals_index_arithmetic(T, N, A, F, K, mb):
    """The take / transpose / reshape route of the reference against the kernel's documented row formula, element by element."""
    c = kr.gather_case(T, N, A, F, K, mb, 3)
    ref = kr.gather_ref(c)
    for j in range(mb):
        for t in range(T):
            for a in range(A):
                r, e, ag = (j * T + t) * A + a, int(c["env_idx"][j]), int(c["agent_perm"][a])
                assert torch.equal(ref["obs"][r], c["obs"][t, e, ag]) and torch.equal(ref["mask"][r], c["mask"][t, e, ag])
                for n in ("action", "value", "logp", "adv", "targets"):
                    assert ref[n][r] == c[n][t, e, ag]
                assert ref["prev"][r] == (0 if a == 0 else c["action"][t, e, int(c["agent_perm"][a - 1])] + 1)
                assert ref["pos"][r] == c["stepcount"][t, e] and ref["done"][j * T + t] == c["done"][t, e]
                assert ref["h0idx"][j * A + a] == e * A + ag
    # the four float fields cannot be confused
    assert ref["value"].max() < 15 < ref["logp"].min() and ref["logp"].max() < 25 < ref["adv"].min() and ref["adv"].max() < 35 < ref["targets"].min()
