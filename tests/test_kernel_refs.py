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
