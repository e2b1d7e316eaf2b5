"""The acting-step primitives of recurrent PPO (csrc/gru_step.hip): ``magpo_gru_cell_step`` against the fp64 GRU cell, with the existing
composed path (magpo_linear for xi + a T = 1 magpo_gru_scan_fwd) on the same inputs as the yardstick, and ``magpo_global_state`` bit for bit
against torch indexing.

Bar of the cell step, for every shape, width configuration, network and reset pattern: max |fused - fp64| <= 1.25 x max |composed - fp64| on
the same inputs (1.25 x is the factor this project allows between two fp32 summation orders).  The kernel sums the same products in the
composed step's own order (csrc/gru_step.hip), so every case also prints how many of its outputs differ from the composed step's.  Every
figure is printed before it is asserted.  Outputs sit in Guards (rows beyond R, and everything around the buffers, keep their sentinel)."""
import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, Guard, dev, ptr_table, transpose_pad

pytestmark = pytest.mark.gpu
H = 128
SHAPES = [(1, 1), (63, 3), (65, 3), (130, 5), (256, 4)]     # (65, 3): env 21 lies across the 64-row tile boundary
WIDTHS = [(64,), (128,), (192,), (256,), (128, 256), (192, 64)]   # one network, and two networks of different D
_NETS = {}


def _net(L, stream, D, seed):
    """Random GRU cell of input width D: natural-layout fp64 weights and the device copies in the kernels' layouts."""
    if (D, seed) not in _NETS:
        g = torch.Generator().manual_seed(1000 * seed + D)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        p = dict(Wi=(rn(D, 3 * H) / D ** 0.5).float(), bi=(0.1 * rn(3 * H)).float(), Wh=(rn(H, 3 * H) / H ** 0.5).float(), bhn=(0.1 * rn(H)).float())
        d = {k: dev(v) for k, v in p.items()}
        d["Wit"], d["Wht"] = transpose_pad(L, stream, d["Wi"]), transpose_pad(L, stream, d["Wh"])
        _NETS[(D, seed)] = (p, d)
    return _NETS[(D, seed)]


def _cell64(p, h, x, reset_rows):
    """flax GRUCell in fp64 on the reset-applied state (the recurrence in the header of csrc/gru.hip)."""
    Wi, bi, Wh, bhn = (p[k].double() for k in ("Wi", "bi", "Wh", "bhn"))
    h = torch.where(reset_rows[:, None], torch.zeros_like(h), h).double()
    xi, hh = x.double() @ Wi + bi, h @ Wh
    r = torch.sigmoid(xi[:, :H] + hh[:, :H])
    z = torch.sigmoid(xi[:, H:2 * H] + hh[:, H:2 * H])
    n = torch.tanh(xi[:, 2 * H:] + r * (hh[:, 2 * H:] + bhn))
    return (1.0 - z) * n + z * h


def _resets(kind, nenv, gen):
    if kind == "none":
        return torch.zeros(nenv, dtype=torch.uint8)
    if kind == "all":
        return torch.ones(nenv, dtype=torch.uint8)
    r = (torch.rand(nenv, generator=gen) < 0.5).to(torch.uint8)
    if nenv > 1:
        r[0], r[-1] = 1, 0
    return r


def _composed(L, stream, d, D, emb, h_in, reset, R, A):
    """GruActor.step's chain on the same inputs; the scan works on whole envs, so the rows are padded up to one."""
    nenv = (R + A - 1) // A
    Rp = nenv * A
    e = torch.zeros(Rp, D, device=DEV); e[:R] = emb
    hi = torch.zeros(Rp, H, device=DEV); hi[:R] = h_in
    xi = torch.empty(Rp, 3 * H, device=DEV)
    ho = Guard(Rp, H)
    L.call("magpo_linear", e, D, d["Wit"], d["bi"], xi, 3 * H, None, Rp, D, 3 * H, 0, 0, stream)
    L.call("magpo_gru_scan_fwd", xi, d["Wht"], d["bhn"], hi, None, reset, ho, None, None, nenv, 1, A, None, 0, 0, stream)
    torch.cuda.synchronize()
    ho.check("composed step")
    return ho.out[:R].cpu()


def _fused(L, stream, nets, embs, h_ins, reset, R, A, alias=False):
    outs, tab = [], []
    for (p, d), e, hi in zip(nets, embs, h_ins):
        ho = Guard(R, H)
        if alias:   # h_out IS h_in: the buffer starts as the state
            ho.out.copy_(hi)
            ho.unset = False
        outs.append(ho)
        tab += [e, d["Wit"], d["bi"], d["Wht"], d["bhn"], ho if alias else hi, ho]
    ptrs = ptr_table(tab)
    dims = np.array([len(nets), embs[0].shape[1], embs[-1].shape[1]], dtype=np.int32)
    L.call("magpo_gru_cell_step", dims.ctypes.data, ptrs.ctypes.data, int(ptrs.size), reset, R, A, stream)
    torch.cuda.synchronize()
    for k, ho in enumerate(outs):
        ho.check(f"fused step, network {k}")
    return [ho.out.cpu() for ho in outs]


@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "D" + "x".join(map(str, w)))
@pytest.mark.parametrize("R,A", SHAPES)
def test_cell_step_against_fp64_and_the_composed_step(L, stream, R, A, widths):
    gen = torch.Generator().manual_seed(7 * R + A + sum(widths))
    nenv = (R + A - 1) // A
    nets = [_net(L, stream, D, k) for k, D in enumerate(widths)]
    embs = [torch.randn(R, D, generator=gen) for D in widths]
    h_ins = [torch.tanh(torch.randn(R, H, generator=gen)) for _ in widths]
    embs_d, h_d = [dev(e) for e in embs], [dev(h) for h in h_ins]
    keep = [t.clone() for t in embs_d + h_d]
    for kind in ("none", "all", "mixed"):
        reset = _resets(kind, nenv, gen)
        reset_rows = reset.bool().repeat_interleave(A)[:R]
        reset_d = dev(reset)
        got = _fused(L, stream, nets, embs_d, h_d, reset_d, R, A)
        assert all(torch.equal(a, b) for a, b in zip(keep, embs_d + h_d)), "an input buffer was written"
        aliased = _fused(L, stream, nets, embs_d, h_d, reset_d, R, A, alias=True)
        for k, ((p, d), D) in enumerate(zip(nets, widths)):
            ref = _cell64(p, h_ins[k], embs[k], reset_rows)
            comp = _composed(L, stream, d, D, embs_d[k], h_d[k], reset_d, R, A)
            e_f = (got[k].double() - ref).abs().max().item()
            e_c = (comp.double() - ref).abs().max().item()
            print(f"CELLSTEP R={R} A={A} D={D} net={k}/{len(widths)} reset={kind}: fused err {e_f:.3e} composed err {e_c:.3e} ratio {e_f / e_c:.2f} "
                  f"outputs that differ from the composed step's {int((got[k] != comp).sum())}")
            assert e_c < 5e-6, "the yardstick itself is off"
            assert e_f <= 1.25 * e_c, f"fused {e_f:.3e} > 1.25 x composed {e_c:.3e}"
            assert torch.equal(aliased[k], got[k]), "h_out aliasing h_in changed the result"
            if kind == "all":   # nothing of h_in may reach the output
                other = _fused(L, stream, nets, embs_d, [torch.zeros_like(h) for h in h_d], reset_d, R, A)
                assert torch.equal(other[k], got[k])


def test_cell_step_rejects_bad_arguments_before_any_launch(L, stream):
    R, A, D = 8, 2, 64
    p, d = _net(L, stream, D, 0)
    emb, h_in = dev(torch.randn(R, D)), dev(torch.randn(R, H))
    reset = dev(torch.zeros(R // A, dtype=torch.uint8))
    ho = Guard(R, H)
    tab = [emb, d["Wit"], d["bi"], d["Wht"], d["bhn"], h_in, ho]
    good = ptr_table(tab)
    two = ptr_table(tab + tab)

    def call(dims, ptrs, nptrs, rst, R_, A_):
        dims = None if dims is None else np.array(dims, dtype=np.int32)
        with pytest.raises(ValueError):
            L.call("magpo_gru_cell_step", None if dims is None else dims.ctypes.data, None if ptrs is None else ptrs.ctypes.data, nptrs, rst, R_, A_, stream)

    call([1, D, 0], good, 7, reset, 0, A)          # R < 1
    call([1, D, 0], good, 7, reset, R, 0)          # A < 1
    for bad_d in (0, 32, 96, 320):
        call([1, bad_d, 0], good, 7, reset, R, A)  # D outside the set
    call([2, D, 96], two, 14, reset, R, A)         # ... of the second network
    for nn in (0, 3):
        call([nn, D, D], good, 7, reset, R, A)     # nnets
    call([1, D, 0], good, 6, reset, R, A)          # table size
    call([2, D, D], good, 7, reset, R, A)
    call([1, D, 0], good, 7, None, R, A)           # null reset flags
    call([1, D, 0], None, 7, reset, R, A)          # null table
    call(None, good, 7, reset, R, A)               # null dims
    for j in range(7):                             # a null pointer in the table
        bad = good.copy(); bad[j] = 0
        call([1, D, 0], bad, 7, reset, R, A)
    torch.cuda.synchronize()
    ho.check("rejected calls", torch.zeros(R, dtype=torch.bool))
    assert bool(torch.isnan(ho.out).all()), "a rejected call launched"


@pytest.mark.parametrize("ld", [64, 128])
@pytest.mark.parametrize("A", [2, 5, 8])
@pytest.mark.parametrize("with_ids", [False, True])
def test_global_state_is_the_concatenated_raw_views(L, stream, A, ld, with_ids):
    N, F_raw = 37, ld // 8            # A = 8 fills the row exactly; A = 2, 5 leave zero columns
    id_cols = A if with_ids else 0
    ldo = id_cols + F_raw + 3         # rows wider than what is read
    obs = torch.randn(N, A, ldo)
    out = Guard(N * A, ld)
    L.call("magpo_global_state", dev(obs), ldo, id_cols, F_raw, out, ld, N, A, stream)
    torch.cuda.synchronize()
    out.check("global_state")
    ref = torch.zeros(N, A, ld)
    ref[:, :, :A * F_raw] = obs[:, :, id_cols:id_cols + F_raw].reshape(N, 1, A * F_raw)   # concat over agents, tiled to every agent
    assert torch.equal(out.out.cpu(), ref.reshape(N * A, ld))


def test_global_state_rejects_bad_arguments(L, stream):
    obs, out = dev(torch.zeros(4, 2, 8)), Guard(8, 64)
    for args in ((8, 0, 8, out, 32, 4, 2),      # ld outside {64, 128}
                 (8, 0, 8, out, 64, 4, 9),      # A * F_raw > ld
                 (8, 4, 8, out, 64, 4, 2),      # id_cols + F_raw > ldo
                 (8, 0, 0, out, 64, 4, 2), (8, 0, 8, out, 64, 0, 2), (8, 0, 8, out, 64, 4, 0), (8, -1, 8, out, 64, 4, 2),
                 (8, 0, 8, None, 64, 4, 2)):
        with pytest.raises(ValueError):
            L.call("magpo_global_state", obs, *args, stream)
    with pytest.raises(ValueError):
        L.call("magpo_global_state", None, 8, 0, 8, out, 64, 4, 2, stream)
    torch.cuda.synchronize()
    out.check("rejected calls", torch.zeros(8, dtype=torch.bool))
    assert bool(torch.isnan(out.out).all())
