"""The one-launch acting step of the memoryless Sable (csrc/ff_sable_act.hip: "magpo_ff_sable_act", SableGuider.act_team_fused) against the
fp64 restatement (oracle.networks.sable_get_actions on zero hidden states with the ff configuration, tests/ff_sable_act_cases.py) and
against the kernel-by-kernel chain SableGuider.act on the same inputs.

Bars, per case: sampled actions bit-exact on every row (tests/test_ff_sable_act_cases.py shows that no case has a Gumbel near-tie); value
and log-prob within 1e-4 relative + 1e-6 of the restatement (the bar of tests/test_ff_sable_learner_gpu.py for this path), and no worse than
max(1.25 x the chain's error on the same inputs, 2^-24 x max|reference|) -- the project's bar for a kernel that replaces another
(DESIGN 4n / 4p).  Every case prints one FFACT line.  Outputs sit between sentinel rows; observation rows carry huge finite values in the
columns >= F, which any read would turn into inf / nan.

The second bar is why the kernel evaluates its heads, norm statistics and retention dot products in double (csrc/ff_sable_act.hip): with
fp32 heads it sat at the chain's 1 - 3 ulp of the output, where one ulp on the worst element is more than 25 %.  Recorded on an MI355X, error
against fp64 as a fraction of the chain's: value 0.29 - 1.0, log-prob 0.34 - 1.0 over the eight cases."""
import numpy as np
import pytest
import torch

from tests import ff_sable_act_cases as fc
from tests.gpu_util import DEV, Guard, _count_calls, ptr_table

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24
HUGE = 3.0e38


def _guider(cid, memory_type="ff_sable"):
    from magpo_amd.sable import SableGuider
    c, x = fc.CASES[cid], fc.make_inputs(cid)
    g = SableGuider(c["A"], c["K"], c["F"], DEV, embed_dim=c["E"], n_head=c["nh"], n_block=c["nb"], memory_type=memory_type, max_pos=4,
                    wgrad_groups=4, obs_ld=c["ld"])
    g.load_named(x["gp"])
    assert g.Fld == c["ld"] and g.team_fused_supported()
    return g, x


def _device_inputs(cid, x, pad=HUGE):
    c = fc.CASES[cid]
    N, A, F = c["N"], c["A"], c["F"]
    obs = torch.full((N, A, c["ld"]), pad, device=DEV)
    obs[..., :F] = x["obs"].to(DEV)
    mask = x["mask"].to(torch.uint8).to(DEV).contiguous() if c["mask"] else None
    pos = torch.zeros(N, dtype=torch.int32, device=DEV)
    return obs, pos, mask, fc.sample_keys(x["key"], A)


def _guards(N, A):
    return Guard(N, A, dtype=torch.int32), Guard(N, A), Guard(N, A)


def _err(got, ref):
    return (got.detach().cpu().double() - ref.double()).abs().max().item()


@pytest.mark.parametrize("cid", sorted(fc.CASES))
def test_parity_with_the_fp64_restatement_and_the_chain(cid):
    c = fc.CASES[cid]
    N, A = c["N"], c["A"]
    g, x = _guider(cid)
    obs, pos, mask, keys = _device_inputs(cid, x)
    ra, rlp, rv, _ = fc.reference(cid)
    ac, lc, vc = (torch.empty(N, A, dtype=torch.int32, device=DEV), torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV))
    g.act(obs, pos, None, keys, ac, lc, vc, mask=mask)
    ga, gl, gv = _guards(N, A)
    counts = {}
    _count_calls(g.L, counts, lambda: g.act_team_fused(obs, pos, None, keys, ga.rows, gl.rows, gv.rows, mask=mask))
    torch.cuda.synchronize()
    assert counts == {"magpo_ff_sable_act": 1}, counts
    for n, gd in (("action", ga), ("logp", gl), ("value", gv)):
        gd.check(f"{cid} {n}")
    figs, bad = [], []
    for n, got, chain, ref in (("value", gv.out, vc, rv), ("logp", gl.out, lc, rlp)):
        e, ec, scale = _err(got, ref), _err(chain, ref), ref.abs().max().item()
        bound = max(1.25 * ec, U24 * scale)
        figs.append(f"{n} {e:.3e}/{ec:.3e}/{bound:.3e} (ref {scale:.3e})")
        if e > 1e-6 + 1e-4 * scale:
            bad.append(n + " over 1e-4 + 1e-6")
        if e > bound:
            bad.append(n + " over max(1.25 x chain, one rounding)")
    same = np.array_equal(ga.out.cpu().numpy(), ra.numpy())
    print(f"FFACT {cid}: fused/chain/bound {'; '.join(figs)}; actions {'equal' if same else 'DIFFER'}")
    assert same, f"{cid}: sampled actions differ from the restatement"
    assert np.array_equal(ac.cpu().numpy(), ra.numpy()), f"{cid}: the chain's actions differ from the restatement"
    assert not bad, (cid, bad, figs)
    if c["mask"]:   # never an illegal action; the forced rows: the one legal action with log-prob exactly 0
        assert bool(torch.gather(mask, -1, ga.out.long().unsqueeze(-1)).all())
        for n, i in ((0, A - 1), (N - 1, 0)):
            assert int(ga.out[n, i]) == c["K"] - 1 and float(gl.out[n, i]) == 0.0
    if c["ld"] > c["F"]:   # the columns >= F of an observation row are never read: other padding, same bits
        obs2, _, _, _ = _device_inputs(cid, x, pad=-1.5e30)
        a2, l2, v2 = _guards(N, A)
        g.act_team_fused(obs2, pos, None, keys, a2.rows, l2.rows, v2.rows, mask=mask)
        assert torch.equal(a2.out, ga.out) and torch.equal(l2.out, gl.out) and torch.equal(v2.out, gv.out)


def _hand_built_tables(g, obs, mask, kdev, scratch, action, logp, value):
    """The 22 + 18 n_block pointers of include/magpo.h, slot by slot, from the guider's parameter views and transposed weight copies."""
    v, wt = g.v, g.wt
    glob = [obs, mask, kdev, v["enc.obs.norm.scale"], v["enc.obs.dense.kernel"], v["enc.ln.scale"], v["dec.act.kernel"], v["dec.ln.scale"],
            wt["vh0"], v["enc.head.dense0.bias"], v["enc.head.norm.scale"], v["enc.head.dense1.kernel"], v["enc.head.dense1.bias"],
            wt["h0"], v["dec.head.dense0.bias"], v["dec.head.norm.scale"], wt["h1"], v["dec.head.dense1.bias"], scratch, action, logp, value]
    blk = []
    for k in range(g.nb):
        e, d = f"enc.block{k}.", f"dec.block{k}."
        blk += [wt[f"qkvg{k}"], wt[f"wo{k}"], v[e + "ln1.scale"], v[e + "ln2.scale"], v[e + "retn.gn.scale"], v[e + "retn.gn.bias"],
                wt[f"qkvg1{k}"], wt[f"wo1{k}"], v[d + "ln1.scale"], v[d + "retn1.gn.scale"], v[d + "retn1.gn.bias"],
                wt[f"q2{k}"], wt[f"kvg2{k}"], wt[f"wo2{k}"], v[d + "ln2.scale"], v[d + "ln3.scale"], v[d + "retn2.gn.scale"], v[d + "retn2.gn.bias"]]
    return ptr_table(glob), ptr_table(blk)


@pytest.mark.parametrize("cid", ["A2-N31-64.2.2-K31-F3-ld7-mask", "A5-N45-64.1.4-K5-F9"])
def test_entry_point_by_name_keys_by_value_and_by_table_and_repeated_launches(cid):
    """magpo_ff_sable_act called by name on a hand-built table gives act_team_fused's bits; host keys by value give the bits of a device
    key table; two consecutive launches give identical bits (no atomics, and the scratch rows of one launch do not leak into the next)."""
    c = fc.CASES[cid]
    N, A, nb = c["N"], c["A"], c["nb"]
    g, x = _guider(cid)
    obs, pos, mask, keys = _device_inputs(cid, x)
    wa, wl, wv = _guards(N, A)
    g.act_team_fused(obs, pos, None, keys, wa.rows, wl.rows, wv.rows, mask=mask)
    need = 32 * ((N + 31) // 32) * A * (384 + 256 * nb)
    scratch = torch.full((need + 64,), float("nan"), device=DEV)    # (a launch must not depend on what the scratch held)
    dims = np.array([N, A, c["K"], c["F"], nb, c["nh"], g.hs, g.gs, 0, c["ld"]], dtype=np.int32)
    kdev = torch.from_numpy(keys.view(np.int32).copy()).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for by_value in (True, False, False):
        ga, gl, gv = _guards(N, A)
        gp, bp = _hand_built_tables(g, obs, mask, None if by_value else kdev, scratch, ga.rows, gl.rows, gv.rows)
        g.L.call("magpo_ff_sable_act", dims.ctypes.data, keys.ctypes.data if by_value else None, gp.ctypes.data, int(gp.size), bp.ctypes.data,
                 int(bp.size), need, st)
        torch.cuda.synchronize()
        for n, gd in (("action", ga), ("logp", gl), ("value", gv)):
            gd.check(f"{cid} {n}")
        outs.append((ga.out.clone(), gl.out.clone(), gv.out.clone()))
    assert bool(torch.isnan(scratch[need:]).all()), "the kernel wrote behind the scratch it was given"
    for o in outs:
        for got, want in zip(o, (wa.out, wl.out, wv.out)):
            assert torch.equal(got, want)


def test_value_only_writes_the_values_and_nothing_else():
    cid = "A4-N33-64.1.1-K10-F5"
    c = fc.CASES[cid]
    N, A = c["N"], c["A"]
    g, x = _guider(cid)
    obs, pos, mask, keys = _device_inputs(cid, x)
    fa, fl, fv = _guards(N, A)
    g.act_team_fused(obs, pos, None, keys, fa.rows, fl.rows, fv.rows)
    gv = Guard(N, A)
    g.act_team_fused(obs, pos, None, None, None, None, gv.rows, value_only=True)
    torch.cuda.synchronize()
    gv.check("value_only value")
    assert torch.equal(gv.out, fv.out)
    # by name, with sentinel-filled action / logp buffers in the table: untouched
    sa, sl, sv = Guard(N, A, dtype=torch.int32, fill=-5), Guard(N, A, fill=-5.0), Guard(N, A)
    need = 32 * ((N + 31) // 32) * A * 640
    gp, bp = _hand_built_tables(g, obs, None, None, torch.empty(need, device=DEV), sa.rows, sl.rows, sv.rows)
    dims = np.array([N, A, c["K"], c["F"], 1, 1, 64, 64, 1, c["ld"]], dtype=np.int32)
    g.L.call("magpo_ff_sable_act", dims.ctypes.data, None, gp.ctypes.data, 22, bp.ctypes.data, 18, need, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sv.check("value_only value (by name)")
    assert torch.equal(sv.out, fv.out)
    assert bool((sa.out == -5).all()) and bool((sl.out == -5.0).all())
    sa.check("value_only action"); sl.check("value_only logp")


def test_graph_replay_equals_the_eager_call():
    cid = "A8-N33-32.2.2-K7-F12-mask"
    c = fc.CASES[cid]
    N, A = c["N"], c["A"]
    g, x = _guider(cid)
    obs, pos, mask, keys = _device_inputs(cid, x)
    kdev = torch.from_numpy(keys.view(np.int32).copy()).to(DEV)
    ea, el, ev = _guards(N, A)
    g.act_team_fused(obs, pos, None, kdev, ea.rows, el.rows, ev.rows, mask=mask)
    torch.cuda.synchronize()
    ra, rl, rv = _guards(N, A)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g.act_team_fused(obs, pos, None, kdev, ra.rows, rl.rows, rv.rows, mask=mask)
    graph.replay()
    torch.cuda.synchronize()
    for n, got, want in (("action", ra, ea), ("logp", rl, el), ("value", rv, ev)):
        got.check(f"replay {n}")
        assert torch.equal(got.out, want.out), n


def _small_net(A, E, memory_type="ff_sable", nb=1):
    from magpo_amd.sable import SableGuider
    K, F, N = 5, A + 1, 3
    g = SableGuider(A, K, F, DEV, embed_dim=E, n_block=nb, memory_type=memory_type, max_pos=4, wgrad_groups=4, seed=3)
    gen = torch.Generator().manual_seed(A + E)
    obs = torch.randn(N, A, F, generator=gen).to(DEV)
    keys = fc.sample_keys(np.array([1, 2], np.uint32), A)
    return g, obs, torch.zeros(N, dtype=torch.int32, device=DEV), keys, N


@pytest.mark.parametrize("A, E, nb", [(3, 128, 1), (9, 64, 1), (2, 64, 5)])
def test_shapes_outside_the_set_take_the_chain(A, E, nb):
    g, obs, pos, keys, N = _small_net(A, E, nb=nb)
    assert not g.team_fused_supported()
    outs = []
    for fn in (g.act, g.act_team_fused):
        a, l, v = torch.empty(N, A, dtype=torch.int32, device=DEV), torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
        counts = {}
        _count_calls(g.L, counts, lambda: fn(obs, pos, None, keys, a, l, v))
        assert counts.get("magpo_ff_sable_act", 0) == 0 and counts.get("magpo_team_retention_fwd", 0) > 0, counts
        outs.append((a, l, v))
    torch.cuda.synchronize()
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_a_recurrent_network_is_refused():
    g, obs, pos, keys, N = _small_net(3, 64, memory_type="rec_sable")
    with pytest.raises(ValueError, match="ff_sable"):
        g.act_team_fused(obs, pos, None, keys, None, None, None)
    ff, *_ = _small_net(3, 64)
    with pytest.raises(NotImplementedError, match="act_team_fused"):
        ff.act_fused(None, None, None, None, None, None, None)
