"""The kernel-by-kernel acting primitives -- magpo_retention_recurrent (both LDS instances, fused GroupNorm + gate epilogue),
magpo_linear_pro (prologues 1-4) and magpo_zero_states_where_done -- against the fp64 references of tests/kernel_refs.py."""
import itertools

import pytest
import torch

from tests import kernel_refs as kr
from tests.gpu_util import DEV, SENT, Guard, check_local, dev

pytestmark = pytest.mark.gpu
E = 64
NPOS = 101
DECAY = 0.775
PREFILL = 5.0      # what the output rows hold before a retention call (rows the call does not return must keep it)
HEADS = [(16, 4), (16, 16), (32, 4), (32, 16), (32, 32), (64, 4), (64, 16), (64, 64)]
NTOKS = [1, 2, 8, 16, 17, 23, 32]


@pytest.fixture(scope="module")
def pe(L, stream):
    t = torch.empty(NPOS, E, device=DEV)
    L.call("magpo_pe_table", t, NPOS, E, stream)
    return t.cpu()


# ------------------------------------------------------------------------------------------------ recurrent retention
def run_ret(L, st, c, hs, gs, ret_from, write, gate, stride):
    """q | k | v | g as column-offset views of 256-float rows (the second head's columns when hs < 64), token a of env e in row
    e * stride + a; the rows between the envs' tokens hold garbage on the input side and the sentinel on the output side."""
    nenv, ntok = c["q"].shape[:2]
    off = hs if hs < 64 else 0
    X = torch.full((nenv, stride, 256), 1e30)
    for i, n in enumerate(("q", "k", "v", "gp")):
        X[:, :ntok, 64 * i + off:64 * i + off + hs] = c[n]
    X = X.reshape(nenv * stride, 256).to(DEV)
    S = Guard(nenv, 4096)
    S.rows.copy_(c["S"].reshape(nenv, 4096))
    r = Guard(nenv * stride, hs, 128, fill=PREFILL)
    gam, bet = dev(c["gamma"]), dev(c["beta"])
    L.call("magpo_retention_recurrent", S, X[:, off:], 256, X[:, 64 + off:], 256, X[:, 128 + off:], 256, stride, r, 128, nenv, ntok, ret_from,
           DECAY, write, X[:, 192 + off:] if gate else None, 256 if gate else 0, gam if gate else None, bet if gate else None, hs, gs, st)
    torch.cuda.synchronize()
    return S, r


def check_ret(L, st, c, hs, gs, ret_from, write, gate, stride, what):
    nenv, ntok = c["q"].shape[:2]
    S, r = run_ret(L, st, c, hs, gs, ret_from, write, gate, stride)
    D = torch.float64
    _, ref = kr.retention_recurrent(c["S"][:, :hs, :hs].to(D), c["q"].to(D), c["k"].to(D), c["v"].to(D), DECAY, ret_from,
                                    *((c["gp"].to(D), c["gamma"].to(D), c["beta"].to(D), gs) if gate else ()))
    S.check(f"{what} state"); r.check(f"{what} ret")
    got = r.out.reshape(nenv, stride, hs)
    check_local(f"ret_recurrent {what} ret", got[:, ret_from:ntok], ref)
    assert bool((got[:, :ret_from] == PREFILL).all()), f"{what}: tokens below ret_from were written"
    assert bool((got[:, ntok:] == PREFILL).all()), f"{what}: rows between the envs' tokens were written"
    if write:
        check_local(f"ret_recurrent {what} state", S.out.reshape(nenv, 64, 64), kr.retention_padded_state(c, DECAY, hs))
    else:
        assert torch.equal(S.out.cpu(), c["S"].reshape(nenv, 4096)), f"{what}: the state must stay bit-unchanged without write_state"


@pytest.mark.parametrize("ntok", NTOKS)
def test_retention_recurrent_shapes(L, stream, ntok):
    """Both instances (up to 16 / 17-32 tokens), every head width / group size, first / middle / last returned token, with and without
    the state write and the gate epilogue; env stride equal to and larger than ntok alternates over the cases (both for every ntok)."""
    n = 0
    for (hs, gs), ret_from, write, gate in itertools.product(HEADS, sorted({0, ntok // 2, ntok - 1}), (0, 1), (False, True)):
        c = kr.retention_case(37, ntok, hs, 100 * ntok + hs + gs)
        stride = ntok + (3 if n % 2 else 0)
        n += 1
        check_ret(L, stream, c, hs, gs, ret_from, write, gate, stride, f"ntok={ntok} hs={hs} gs={gs} from={ret_from} write={write} gate={gate} stride={stride}")


@pytest.mark.parametrize("nenv", [1, 1030])
@pytest.mark.parametrize("ntok", NTOKS)
def test_retention_recurrent_env_counts(L, stream, ntok, nenv):
    hs, gs = HEADS[NTOKS.index(ntok) % len(HEADS)]
    c = kr.retention_case(nenv, ntok, hs, 7 * ntok + nenv)
    for write, gate, stride in ((1, True, ntok + 5), (0, False, ntok)):
        check_ret(L, stream, c, hs, gs, ntok // 2, write, gate, stride, f"nenv={nenv} ntok={ntok} hs={hs} gs={gs} write={write} gate={gate}")


@pytest.mark.parametrize("gate", [False, True])
def test_retention_recurrent_instance_seam(L, stream, gate):
    """A 17-token call (56 KiB instance) whose last token has k = v = 0 gives the state and the first 16 outputs of the 16-token call
    (28 KiB instance): two kernels, so within the forward tolerance, not bitwise."""
    c17 = kr.retention_case(37, 17, 64, 99)
    c17["k"][:, 16] = 0
    c17["v"][:, 16] = 0
    c16 = {n: (t[:, :16].contiguous() if n in ("q", "k", "v", "gp") else t) for n, t in c17.items()}
    S17, r17 = run_ret(L, stream, c17, 64, 16, 0, 1, gate, 17)
    S16, r16 = run_ret(L, stream, c16, 64, 16, 0, 1, gate, 16)
    check_local("instance seam state", S17.out, S16.out)
    check_local("instance seam ret", r17.out.reshape(37, 17, 64)[:, :16], r16.out.reshape(37, 16, 64))


def test_retention_recurrent_rejects_bad_arguments(L, stream):
    c = kr.retention_case(2, 4, 64, 1)
    S, q, r = dev(c["S"]), dev(c["q"].reshape(8, 64)), torch.full((8, 64), SENT, device=DEV)
    for ntok, ret_from, hs, gs in ((0, 0, 64, 64), (33, 0, 64, 64), (4, 4, 64, 64), (4, -1, 64, 64), (4, 0, 66, 2), (4, 0, 68, 4),
                                   (4, 0, 0, 1), (4, 0, 64, 3), (4, 0, 16, 32), (4, 0, 64, 0)):
        with pytest.raises(ValueError):
            L.call("magpo_retention_recurrent", S, q, 64, q, 64, q, 64, 4, r, 64, 2, ntok, ret_from, DECAY, 0, None, 0, None, None, hs, gs, stream)
    torch.cuda.synchronize()
    assert bool((r == SENT).all())


# ------------------------------------------------------------------------------------------------ state zeroing
@pytest.mark.parametrize("nenv", [1, 5, 4097])
def test_zero_states_where_done(L, stream, nenv):
    g = torch.Generator().manual_seed(nenv)
    done = torch.rand(nenv, generator=g) < 0.4
    if nenv == 1:
        done[:] = True
    src = [torch.randn(nenv, 4096, generator=g) for _ in range(3)]
    for flip in ((False, True) if nenv == 1 else (False,)):   # nenv = 1: the done env, then the live one
        d = done ^ flip
        bufs = [Guard(nenv, 4096) for _ in range(3)]
        for b, s in zip(bufs, src):
            b.rows.copy_(s)
        L.call("magpo_zero_states_where_done", bufs[0], bufs[1], bufs[2], dev(d.to(torch.uint8)), nenv, stream)
        torch.cuda.synchronize()
        for i, (b, s) in enumerate(zip(bufs, src)):
            b.check(f"state {i}")
            out = b.out.cpu()
            assert bool((out[d] == 0).all()), f"state {i}: done envs must be exactly zero"
            assert torch.equal(out[~d], s[~d]), f"state {i}: live envs must be bit-unchanged"


# ------------------------------------------------------------------------------------------------ prologue-fused dense layer
def run_linear_pro(L, st, pro, c, NOUT, use_pe, given, pos_stride=1):
    R = c["pos"].shape[0]
    Wt = torch.zeros((NOUT + 31) // 32 * 32, E)
    Wt[:NOUT] = c["Wd"].T
    pos = torch.full((R, pos_stride), 10 ** 6, dtype=torch.int32)
    pos[:, 0] = c["pos"]
    k = {n: dev(c.get(n)) for n in ("a", "y", "s1", "s2", "pe", "W", "idx", "s_obs", "bias")}
    k.update(Wt=dev(Wt), pos=dev(pos))
    out = dict(Y=Guard(R, NOUT, NOUT + 4))
    if given:
        out.update(out=Guard(R, E), outpe=Guard(R, E, 128))
    lda = 0 if c.get("a") is None else c["a"].shape[1]
    L.call("magpo_linear_pro", pro, k["a"], lda, k["y"], E, k["s1"], k["s2"], k["pe"], k["pos"], pos_stride, NPOS, 1 if use_pe else 0, k["W"],
           k["idx"], 1, k["s_obs"], c["F"], out.get("out"), E, out.get("outpe"), 128, k["Wt"], k["bias"], out["Y"], NOUT + 4, R, NOUT, st)
    torch.cuda.synchronize()
    return out, k


def run_unfused(L, st, pro, c, k, NOUT, use_pe, pos_stride):
    """The composition the E = 128 host path uses (sable.py:_pro): row kernel, then magpo_linear."""
    R = c["pos"].shape[0]
    out, outpe = Guard(R, E), Guard(R, E)
    if pro == 1:
        L.call("magpo_embed_fwd", 1, None, 0, 0, None, k["W"], k["idx"], 1, k["s1"], k["pe"], k["pos"], pos_stride, NPOS, None, 0, out, E, outpe, E, R, E, st)
    elif pro == 2:
        L.call("magpo_embed_fwd", 0, k["a"], c["a"].shape[1], c["F"], k["s_obs"], k["W"], None, 0, k["s1"], k["pe"], k["pos"], pos_stride, NPOS, None, 0,
               out, E, outpe, E, R, E, st)
    elif pro == 3:
        L.call("magpo_resnorm_fwd", k["a"], E, k["y"], E, k["s1"], k["s2"], k["pe"], k["pos"], pos_stride, NPOS, out, E, outpe, E, R, E, st)
    else:
        L.call("magpo_headmid_fwd", k["a"], E, k["s1"], out, E, None, None, None, 0, R, E, st)
        L.call("magpo_add_pe", out, E, k["pe"], k["pos"], pos_stride, NPOS, outpe, E, R, E, st)
    Y = Guard(R, NOUT, NOUT + 4)
    L.call("magpo_linear", outpe if use_pe else out, E, k["Wt"], k["bias"], Y, NOUT + 4, None, R, E, NOUT, 0, 0, st)
    torch.cuda.synchronize()
    return dict(out=out, outpe=outpe, Y=Y)


def check_linear_pro(L, st, pe, pro, R, NOUT, use_pe, given, variant=0):
    c = kr.linear_pro_case(pro, R, NOUT, 31 * pro + NOUT + R, pe=pe, s2=variant == 0, y=variant != 2)
    what = f"pro{pro} R={R} NOUT={NOUT} pe={use_pe} given={given} v{variant}"
    pos_stride = 2 if use_pe else 1
    out, k = run_linear_pro(L, st, pro, c, NOUT, use_pe, given, pos_stride)
    ref = dict(zip(("out", "outpe", "Y"), kr.linear_pro(pro, c, use_pe)))
    unf = run_unfused(L, st, pro, c, k, NOUT, use_pe, pos_stride)
    for n, g in out.items():
        g.check(f"{what} {n}")
        check_local(f"linear_pro {what} {n}", g.out, ref[n])
        unf[n].check(f"{what} unfused {n}")
        check_local(f"linear_pro {what} {n} against the unfused path", g.out, unf[n].out.cpu().double())


@pytest.mark.parametrize("use_pe,given", [(0, True), (1, True), (0, False), (1, False)])
@pytest.mark.parametrize("NOUT", [20, 64, 192, 256])
@pytest.mark.parametrize("pro", [1, 2, 3, 4])
def test_linear_pro(L, stream, pe, pro, NOUT, use_pe, given):
    """One, three and four column groups and a ragged one; 32-row tiles: one row, one short of a tile, one over, many."""
    for R in (1, 31, 33, 1000):
        check_linear_pro(L, stream, pe, pro, R, NOUT, use_pe, given)
    if pro == 3:   # without the second norm; without the addend (plain norm)
        check_linear_pro(L, stream, pe, 3, 33, NOUT, use_pe, given, variant=1)
        check_linear_pro(L, stream, pe, 3, 33, NOUT, use_pe, given, variant=2)


@pytest.mark.parametrize("pro,R,NOUT", [(1, 32 * 2048 + 9, 64), (3, 32 * 2048 + 9, 20), (2, 32 * 512 + 45, 256), (4, 32 * 512 + 45, 256),
                                        (3, 32 * 2048 + 9, 192)])
def test_linear_pro_grid_stride(L, stream, pe, pro, R, NOUT):
    """More 32-row tiles than walkers: 2048 one-wave blocks (NOUT <= 64), 682 three-wave blocks, 512 four-wave blocks."""
    check_linear_pro(L, stream, pe, pro, R, NOUT, 1, True)


def test_linear_pro_rejects_bad_arguments(L, stream, pe):
    c = kr.linear_pro_case(4, 8, 64, 3, pe=pe)
    Y = Guard(8, 64)
    for pro, NOUT in ((0, 64), (5, 64), (4, 0), (4, -3)):
        with pytest.raises(ValueError):
            L.call("magpo_linear_pro", pro, dev(c["a"]), E, None, 0, dev(c["s1"]), None, dev(c["pe"]), dev(c["pos"]), 1, NPOS, 0, None, None, 0, None, 0,
                   None, 0, None, 0, dev(c["Wd"].T), dev(c["bias"]), Y, 64, 8, NOUT, stream)
    torch.cuda.synchronize()
    Y.check("rejected calls write nothing", defined=torch.zeros(8, dtype=torch.bool))
