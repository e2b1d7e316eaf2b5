"""magpo_dense_bwd (csrc/linear.hip: k_dense_bwd -- dW, db and dX of a narrow dense layer from one pass over X and dY) against fp64 and against
the pair it replaces (magpo_wgrad + magpo_linear) on the same inputs, at production strides (dY rows 64 wide with 20 valid columns, dY as a
column window of a [R, 192] matrix, X / dX rows wider than KIN), with NaN in the unused columns of dY, guard rows and columns around every
output, twice for the same bits; then at guider / actor level: one minibatch with the threshold ``Tuning.dense_bwd_min_rows`` at 0 against
one with the default.

Criterion for every output (the bound of tests/test_seg_bwd_wo_gpu.py): max error against fp64 <= 2 x the pair's max error against the same
reference + 1e-7 x max|reference|.  The kernel sums the pair's terms in the pair's order, so on top of that bound its outputs equal the
pair's element for element (test_same_values_as_the_pair).  Each run prints its figures (``DENSEBWD ...``); profiles/dense_bwd_errors.txt is the table
scripts/summarize_dense_bwd_errors.py makes of that output (per shape, row count and output: the maximum over the runs)."""
import pytest
import torch

from tests import kernel_refs as kr
from tests.gpu_util import DEV, Guard, _count_calls

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (64, 20), (64, 33), (128, 20), (128, 64), (64, 1)]
ROWS = [1, 63, 64, 65, 257, 16448, 16451]     # one tile, ragged last tile, many full tiles, ragged large
MODES = ["none", "mask_x", "mask_sep"]        # act 0; act 4 with mask = X; act 4 with a separate mask


def _layout(NOUT):
    """(row width of the matrix dY lives in, its first column): 64-wide rows for the K = 20 heads, a column window of a [R, 192] matrix for
    64 columns (the cross-retention gradient), otherwise NOUT rounded up to 4 plus one more float4 of unused columns."""
    if NOUT == 20:
        return 64, 0
    if NOUT == 64:
        return 192, 64
    return (NOUT + 3) // 4 * 4 + 4, 0


_cases = {}


def case(KIN, NOUT, R):
    """Inputs and fp64 references of one shape, made once and left unchanged."""
    key = (KIN, NOUT, R)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(1000 * KIN + 10 * NOUT + R % 997)
    ld = KIN + 8
    X = torch.randn(R, KIN, generator=g)
    X[::5] = -X[::5].abs()                    # whole rows <= 0: with mask = X their dX rows are exactly 0
    dY = torch.randn(R, NOUT, generator=g)
    W = torch.randn(KIN, NOUT, generator=g) / NOUT ** 0.5
    M = torch.randn(R, KIN, generator=g)
    M[1::7] = -M[1::7].abs()
    M[2::7] = 0.0
    wy, c0 = _layout(NOUT)
    Xs = torch.full((R, ld), float("nan")); Xs[:, :KIN] = X
    Ms = torch.full((R, ld), float("nan")); Ms[:, :KIN] = M
    Yfull = torch.full((R, wy), float("nan")); Yfull[:, c0:c0 + NOUT] = dY
    if NOUT == 64:                            # the neighbouring windows of the [R, 192] matrix hold other gradients, not NaN
        Yfull[:, :64] = 3.0; Yfull[:, 128:] = -5.0
    Yzero = Yfull.clone(); Yzero[torch.isnan(Yzero)] = 0.0
    Yclean = torch.zeros(R, 64); Yclean[:, :NOUT] = dY        # the pair's dX GEMM contracts over 64 columns: zeros beyond NOUT, as in production
    Wpad = torch.zeros(KIN, 64); Wpad[:, :NOUT] = W
    Xd, dYd, Wd = X.double(), dY.double(), W.double()
    dx = dYd @ Wd.t()
    ref = dict(dW=Xd.t() @ dYd, db=dYd.sum(0, keepdim=True), none=dx, mask_x=torch.where(Xd > 0, dx, torch.zeros_like(dx)),
               mask_sep=torch.where(M.double() > 0, dx, torch.zeros_like(dx)))
    c = dict(KIN=KIN, NOUT=NOUT, R=R, ld=ld, wy=wy, c0=c0, X=Xs.to(DEV), M=Ms.to(DEV), Y=Yfull.to(DEV), Yzero=Yzero.to(DEV), Yclean=Yclean.to(DEV),
             W=W.to(DEV).contiguous(), Wpad=Wpad.to(DEV), ref=ref, Xneg=(X <= 0).all(1), Mneg=(M <= 0).all(1))
    _cases[key] = c
    return c


def run_new(L, st, c, G, bias, mode, Y=None):
    KIN, NOUT, R, ld = c["KIN"], c["NOUT"], c["R"], c["ld"]
    Y = c["Y"] if Y is None else Y
    dX, dW, db = Guard(R, KIN, ld), Guard(KIN, NOUT), Guard(1, NOUT)
    ws = torch.full((L.call("magpo_wgrad_workspace_floats", KIN, NOUT, G),), float("nan"), device=DEV)
    mask = None if mode == "none" else (c["X"] if mode == "mask_x" else c["M"])
    rc = L.call("magpo_dense_bwd", c["X"], ld, Y[:, c["c0"]:], c["wy"], c["W"], mask, ld if mask is not None else 0, dX, ld, R, KIN, NOUT,
                dW, db if bias else None, ws, G, 0 if mode == "none" else 4, st)
    assert rc == 0
    torch.cuda.synchronize()
    return dict(dX=dX, dW=dW, db=db if bias else None)


def run_pair(L, st, c, G, mode):
    """Today's two launches on the same inputs: magpo_wgrad, then magpo_linear with the natural weights padded to 64 columns."""
    KIN, NOUT, R, ld = c["KIN"], c["NOUT"], c["R"], c["ld"]
    dX = torch.full((R, ld), float("nan"), device=DEV)
    dW, db = torch.empty(KIN, NOUT, device=DEV), torch.empty(1, NOUT, device=DEV)
    ws = torch.empty(L.call("magpo_wgrad_workspace_floats", KIN, NOUT, G), device=DEV)
    L.call("magpo_wgrad", c["X"], ld, c["Yclean"], 64, R, KIN, KIN, NOUT, dW, db, ws, G, 1.0, 0, 0, st)
    mask = None if mode == "none" else (c["X"] if mode == "mask_x" else c["M"])
    L.call("magpo_linear", c["Yclean"], 64, c["Wpad"], None, dX, ld, mask, R, 64, KIN, 0 if mode == "none" else 4, 0, st)
    torch.cuda.synchronize()
    return dict(dX=dX[:, :KIN], dW=dW, db=db)


def _bounded(tag, new, old, ref):
    e_new, e_old, scale = kr.max_err(new, ref), kr.max_err(old, ref), ref.abs().max().item()
    bound = 2.0 * e_old + 1e-7 * scale
    print(f"DENSEBWD {tag}: pair err {e_old:.3e} fused err {e_new:.3e} ratio {e_new / max(e_old, 1e-300):.2f} bound {bound:.3e} max|ref| {scale:.3e}")
    assert e_new <= bound, f"{tag}: fused error {e_new:.3e} > 2 x {e_old:.3e} + 1e-7 x {scale:.3e}"


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("KIN,NOUT", SHAPES)
def test_against_fp64_and_the_pair(L, stream, KIN, NOUT, R):
    c = case(KIN, NOUT, R)
    for mode in MODES:
        for G in (1, 4):
            old = run_pair(L, stream, c, G, mode)
            for bias in (True, False):
                tag = f"{KIN}x{NOUT} R={R} G={G} bias={int(bias)} {mode}"
                new = run_new(L, stream, c, G, bias, mode)
                for n in ("dX", "dW", "db"):
                    if new[n] is not None:
                        new[n].check(f"{tag} {n}")                       # everything written, guard rows / columns untouched
                        assert bool(torch.isfinite(new[n].out).all()), f"{tag}: {n} is not finite"
                _bounded(f"{tag} dX", new["dX"].out, old["dX"], c["ref"][mode])
                _bounded(f"{tag} dW", new["dW"].out, old["dW"], c["ref"]["dW"])
                if bias:
                    _bounded(f"{tag} db", new["db"].out, old["db"], c["ref"]["db"])
                if mode != "none":                                      # rows whose mask is <= 0 everywhere: exactly 0
                    neg = (c["Xneg"] if mode == "mask_x" else c["Mneg"]).to(DEV)
                    assert bool(neg.any()) or R < 5
                    assert bool((new["dX"].out[neg] == 0).all()), f"{tag}: dX rows under an all-non-positive mask are not exactly 0"


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("KIN,NOUT", SHAPES)
def test_same_bits_twice_and_unused_columns_ignored(L, stream, KIN, NOUT, R):
    """Two launches give the same bits (fixed-order slab reduction, no atomics), and so does a launch whose unused dY columns hold zeros
    instead of NaN: those columns are never used."""
    c = case(KIN, NOUT, R)
    for mode, G in (("none", 4), ("mask_x", 1), ("mask_sep", 4)):
        a, b, z = run_new(L, stream, c, G, True, mode), run_new(L, stream, c, G, True, mode), run_new(L, stream, c, G, True, mode, Y=c["Yzero"])
        for n in ("dX", "dW", "db"):
            assert torch.equal(a[n].out, b[n].out), f"{KIN}x{NOUT} R={R} {mode}: {n} differs between two launches"
            assert torch.equal(a[n].out, z[n].out), f"{KIN}x{NOUT} R={R} {mode}: {n} depends on the columns >= NOUT of dY"


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("KIN,NOUT", SHAPES)
def test_same_values_as_the_pair(L, stream, KIN, NOUT, R):
    """Every sum of the kernel runs over the pair's terms in the pair's order (tiles per slab, rows per MFMA step, bias column sums per tile,
    the dX contraction over 64 columns with the padding's zeros): dW, db and dX compare equal to magpo_wgrad + magpo_linear element for
    element, so routing a layer to the kernel changes no result."""
    c = case(KIN, NOUT, R)
    for mode, G in (("none", 1), ("mask_x", 4), ("mask_sep", 4)):
        new, old = run_new(L, stream, c, G, True, mode), run_pair(L, stream, c, G, mode)
        for n in ("dX", "dW", "db"):
            d = (new[n].out != old[n])
            assert not bool(d.any()), f"{KIN}x{NOUT} R={R} G={G} {mode}: {n} differs from the pair in {int(d.sum())} elements"


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    print(f"DENSEBWD learner {what}: max err {err:.3e} (ref scale {ref:.3e})")
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


@pytest.mark.parametrize("A,K,N,T,nb", [(4, 20, 12, 16, 1), (3, 10, 7, 9, 2)])
def test_guider_and_actor_fused_equal_the_pair(L, A, K, N, T, nb):
    """One rollout and one minibatch_grads of the same learner, once with every narrow pair on magpo_dense_bwd (threshold 0) and once with
    the default threshold (these minibatches are far below it: the pair, launch for launch): same actions, losses and gradients within the
    bars of test_learner_gpu.py::test_fused_segments_equal_kernel_composition.  The fused path makes 4 + nb calls per minibatch (logit head
    dense1 / dense0, value head dense0, one cross-retention w_q per block, the actor head), each replacing one magpo_wgrad and one
    magpo_linear; with the default threshold it is never called."""
    from magpo_amd.learner import CoordSumConfig, MagpoLearner, SystemConfig, host_split, prng_key
    from magpo_amd.tuning import Tuning
    sysc = SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=1)
    key = host_split(prng_key(21), 4)[0]
    ls = []
    for min_rows in (None, 0):
        t = Tuning()
        if min_rows is not None:
            t.dense_bwd_min_rows = min_rows
        l = MagpoLearner(CoordSumConfig(A, K, 7, 3 * K), N, sysc, "cuda", net_seed=3, wgrad_groups=4, n_block=nb, tuning=t)
        assert l.guider.tuning is t and l.actor.tuning is t
        l.use_graph = False
        l.setup(key)
        l.rollout()
        env_idx = torch.arange(N, device="cuda", dtype=torch.int32)
        agent_perm = torch.arange(A, device="cuda", dtype=torch.int32)
        counts = {}
        _count_calls(L, counts, lambda: l.minibatch_grads(env_idx, agent_perm))
        torch.cuda.synchronize()
        ls.append((l, counts))
    (a, ca), (b, cb) = ls
    assert a.guider.tuning.dense_bwd_min_rows == 16384
    assert torch.equal(a.traj["action"], b.traj["action"])
    nf = 4 + nb
    print(f"DENSEBWD learner calls nb={nb}: default {ca.get('magpo_dense_bwd', 0)} dense_bwd / {ca['magpo_wgrad']} wgrad / {ca['magpo_linear']} linear; "
          f"threshold 0: {cb.get('magpo_dense_bwd', 0)} / {cb['magpo_wgrad']} / {cb['magpo_linear']}")
    assert ca.get("magpo_dense_bwd", 0) == 0 and cb.get("magpo_dense_bwd", 0) == nf
    assert ca["magpo_wgrad"] == cb["magpo_wgrad"] + nf and ca["magpo_linear"] == cb["magpo_linear"] + nf
    # the default path launch for launch: the counts of the commit before magpo_dense_bwd for this minibatch (recorded there with _count_calls)
    assert (ca["magpo_wgrad"], ca["magpo_linear"]) == {1: (11, 15), 2: (15, 21)}[nb]
    assert {n: v for n, v in ca.items() if n not in ("magpo_wgrad", "magpo_linear")} == \
           {n: v for n, v in cb.items() if n not in ("magpo_wgrad", "magpo_linear", "magpo_dense_bwd")}
    close(b.loss_out, a.loss_out, 1e-5, 1e-6, "losses")
    ga, gb = a.guider.grads, b.guider.grads
    scale = float(ga.abs().max())
    err = float((ga - gb).abs().max())
    print(f"DENSEBWD learner guider gradients: max err {err:.3e} (scale {scale:.3e})")
    assert err <= 2e-5 * scale + 1e-7, "guider gradients differ between magpo_dense_bwd and the pair"
    close(b.actor.grads, a.actor.grads, 1e-5, 1e-7, "actor gradients")


@pytest.mark.parametrize("A,K,N,T,nb", [(4, 20, 12, 16, 1), (3, 10, 7, 9, 2)])
def test_overlap_wgrad_gives_the_same_gradients(L, A, K, N, T, nb):
    """``overlap_wgrad``: the remaining weight gradients run on the side stream while magpo_dense_bwd runs on the calling stream.  Both
    write slabs and fold them, so the fused launch has a workspace of its own there (NetBase.dense_bwd); sharing ``wg_ws`` across the two
    streams would give gradients that depend on timing.  Three minibatch passes with overlap against one without: equal element for element."""
    from magpo_amd.learner import CoordSumConfig, MagpoLearner, SystemConfig, host_split, prng_key
    from magpo_amd.tuning import Tuning
    sysc = SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=1)
    key = host_split(prng_key(21), 4)[0]
    env_idx = torch.arange(N, device="cuda", dtype=torch.int32)
    agent_perm = torch.arange(A, device="cuda", dtype=torch.int32)
    grads = []
    for overlap in (False, True):
        t = Tuning()
        t.dense_bwd_min_rows = 0
        l = MagpoLearner(CoordSumConfig(A, K, 7, 3 * K), N, sysc, "cuda", net_seed=3, wgrad_groups=4, n_block=nb, tuning=t)
        l.use_graph = False
        l.guider.overlap_wgrad = l.actor.overlap_wgrad = overlap
        l.setup(key)
        l.rollout()
        for rep in range(3 if overlap else 1):
            counts = {}
            _count_calls(L, counts, lambda: l.minibatch_grads(env_idx, agent_perm))
            torch.cuda.synchronize()
            assert counts.get("magpo_dense_bwd", 0) == 4 + nb
            grads.append((l.guider.grads.clone(), l.actor.grads.clone(), l.loss_out.clone()))
        if overlap:
            for net in (l.guider, l.actor):   # (the guider keeps its weight gradients on the calling stream when it has several blocks)
                if net._wgrad_side() is not None:
                    assert "dense_ws" in net.b.t and net.b.t["dense_ws"].data_ptr() != net.wg_ws.data_ptr()
                else:
                    assert net is l.guider and nb > 1 and "dense_ws" not in net.b.t
        else:
            assert "dense_ws" not in l.guider.b.t and "dense_ws" not in l.actor.b.t     # no second workspace without overlap
    ref = grads[0]
    for i, g in enumerate(grads[1:]):
        for what, x, y in zip(("guider gradients", "actor gradients", "losses"), g, ref):
            d = x != y
            assert not bool(d.any()), f"overlap pass {i}: {what} differ from the one-stream pass in {int(d.sum())} elements"
