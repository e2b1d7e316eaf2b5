"""The acting-step kernel of feed-forward PPO (csrc/mlp_step.hip): ``magpo_mlp_act_step`` against the fp64 MLP, with the composed chain of
the existing kernels on the same inputs as the yardstick (magpo_small_linear, or magpo_small_operand + magpo_linear, for the first layer;
magpo_linear per further layer and for the head; magpo_copy_rows for a value vector).

Bar, for every case and every R: max |fused - fp64| <= 1.25 x max |composed - fp64| (1.25 x is the factor this project allows between two
fp32 summation orders).  The kernel sums every product chain in the composed kernels' own order, so every line also prints how many outputs
differ from the composed chain's.  The yardstick itself: its error over the R values of a case (same weights, 259 rows in all) is at most
4 x that of plain fp32 torch on those inputs -- taken over all rows of the case, because a single output (R = 1, NOUT = 1) has no
meaningful error ratio against another summation order.  Every figure is printed on an ``MLPSTEP`` line before it is asserted.  Outputs sit
in Guards; input columns >= F and input rows >= R hold NaN in every fused call."""
import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, Guard, dev, ptr_table, transpose_pad

pytestmark = pytest.mark.gpu

RS = (1, 63, 65, 130)
INPUTS = [(7, 7), (32, 32), (20, 64), (33, 128), (128, 128)]      # (F, ldx)
HEADS = [(5, 64), (32, 64), (1, 1)]                               # (NOUT, ldy)
# (widths, activation, activate_final): the four of the issue, and three more so that every width is a first, a middle and a last layer
TORSOS = [((128, 128), "relu", True), ((64,), "tanh", True), ((256, 192, 64), "relu", True), ((192, 256), "tanh", False),
          ((64, 256, 192), "tanh", True), ((192, 64, 128), "relu", True), ((128, 128, 256), "relu", False)]
ACT = {"relu": 1, "tanh": 5}
XROWS = 130 + 70     # rows of every input buffer: the largest R and a tile's worth of NaN rows behind it
_NETS = {}


class Net:
    """Random MLP + head: natural-layout weights (host, fp32 values) and the device images magpo_mlp_act_step documents."""

    def __init__(self, L, stream, F, ldx, widths, act, final, nout, ldy, seed):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        self.F, self.ldx, self.widths, self.act, self.final, self.nout, self.ldy = F, ldx, tuple(widths), ACT[act], bool(final), nout, ldy
        self.W, self.b = [], []
        kin = F
        for w in widths:
            self.W.append((rn(kin, w) / kin ** 0.5).float())     # N(0, 1 / fan_in): outputs O(1)
            self.b.append((0.1 * rn(w)).float())
            kin = w
        self.Wh, self.bh = (rn(kin, nout) / kin ** 0.5).float(), (0.1 * rn(nout)).float()
        self.small = F <= 32 and widths[0] == 128 and self.layer_act(0) == 1
        self.KP = 64 if F <= 32 else 128
        self.dW, self.db = [], [dev(b) for b in self.b]
        for i, W in enumerate(self.W):
            if i == 0 and self.small:
                self.dW.append(dev(W))
            elif i == 0:
                Wp = torch.zeros(self.KP, widths[0]); Wp[:F] = W
                self.dW.append(transpose_pad(L, stream, dev(Wp)))
            else:
                self.dW.append(transpose_pad(L, stream, dev(W)))
        self.dW0_nat = dev(self.W[0])
        self.dWh, self.dbh = transpose_pad(L, stream, dev(self.Wh)), dev(self.bh)
        # inputs: XROWS rows, the same for every R; NaN in the columns >= F
        self.x = torch.randn(XROWS, F, generator=g)
        xb = torch.full((XROWS, ldx), float("nan")); xb[:, :F] = self.x
        self.x_clean = dev(torch.nan_to_num(xb, nan=0.0))     # what the composed chain reads (zero padding, as the env kernels write it)
        self.x_nan_cols = dev(xb)

    def layer_act(self, i):
        return self.act if (i < len(self.widths) - 1 or self.final) else 0

    def dims(self):
        w = list(self.widths) + [0] * (3 - len(self.widths))
        return [self.F, self.ldx, len(self.widths), *w, self.act, int(self.final), self.nout, self.ldy]

    def ptrs(self, X, Y):
        t = [X]
        for i in range(3):
            t += [self.dW[i], self.db[i]] if i < len(self.widths) else [None, None]
        return t + [self.dWh, self.dbh, Y]

    def ref(self, R, dtype):
        y = self.x[:R].to(dtype)
        for i, (W, b) in enumerate(zip(self.W, self.b)):
            y = y @ W.to(dtype) + b.to(dtype)
            a = self.layer_act(i)
            y = torch.relu(y) if a == 1 else torch.tanh(y) if a == 5 else y
        return y @ self.Wh.to(dtype) + self.bh.to(dtype)

    def x_for(self, R):
        """The input buffer of a fused call on R rows: NaN in the columns >= F and in every row >= R."""
        xb = self.x_nan_cols.clone()
        xb[R:] = float("nan")
        return xb

    def composed(self, L, stream, R):
        """The chain FfActor / FfCritic run with the fused step off (TorsoNet._torso_fwd, the head, the value copy)."""
        X, ldx, kin = self.x_clean, self.ldx, None
        for i, d in enumerate(self.widths):
            y = torch.empty(R, d, device=DEV)
            if i == 0 and self.small:
                L.call("magpo_small_linear", X, ldx, self.F, self.dW0_nat, self.db[0], y, d, d, R, 1, stream)
            else:
                if i == 0 and self.F <= 32:
                    xp = torch.empty(R, 64, device=DEV)
                    L.call("magpo_small_operand", 2, X, ldx, self.F, None, None, 0, xp, R, stream)
                    X, ldx = xp, 64
                if i == 0:
                    kin = self.KP
                L.call("magpo_linear", X, ldx, self.dW[i], self.db[i], y, d, None, R, kin, d, self.layer_act(i), 0, stream)
            X, ldx, kin = y, d, d
        logits = torch.zeros(R, 64, device=DEV)
        L.call("magpo_linear", X, ldx, self.dWh, self.dbh, logits, 64, None, R, kin, self.nout, 0, 0, stream)
        if self.ldy == 1:
            out = Guard(R, 1)
            L.call("magpo_copy_rows", logits, 64, out, 1, R, 1, stream)
            torch.cuda.synchronize()
            out.check("composed value copy")
            return out.out.cpu()
        torch.cuda.synchronize()
        return logits[:, :self.nout].cpu()


def _net(L, stream, ti, ii, hi):
    key = (ti, ii, hi)
    if key not in _NETS:
        (F, ldx), (widths, act, final), (nout, ldy) = INPUTS[ii], TORSOS[ti], HEADS[hi]
        _NETS[key] = Net(L, stream, F, ldx, widths, act, final, nout, ldy, seed=100 * ti + 10 * ii + hi + 1)
    return _NETS[key]


def _fused(L, stream, nets, R, xs=None, keep_guards=False):
    """One launch for ``nets`` on R rows; returns the outputs (host) after the Guard checks."""
    xs = [n.x_for(R) for n in nets] if xs is None else xs
    before = [x.clone() for x in xs]
    outs = [Guard(R, n.nout, n.ldy) for n in nets]
    tab, dims = [], [len(nets)]
    for n, x, o in zip(nets, xs, outs):
        tab += n.ptrs(x, o)
        dims += n.dims()
    ptrs, dims = ptr_table(tab), np.array(dims, dtype=np.int32)
    L.call("magpo_mlp_act_step", dims.ctypes.data, ptrs.ctypes.data, int(ptrs.size), R, stream)
    torch.cuda.synchronize()
    for k, (o, x, b) in enumerate(zip(outs, xs, before)):
        o.check(f"fused step, network {k}")     # every owned element written, guard rows and the columns between rows untouched
        assert torch.equal(x.view(torch.int32), b.view(torch.int32)), "an input buffer was written"
    return outs if keep_guards else [o.out.cpu() for o in outs]


@pytest.mark.parametrize("ii", range(len(INPUTS)), ids=lambda i: "F%dld%d" % INPUTS[i])
@pytest.mark.parametrize("ti", range(len(TORSOS)), ids=lambda i: "x".join(map(str, TORSOS[i][0])) + TORSOS[i][1] + ("" if TORSOS[i][2] else "nofinal"))
def test_step_against_fp64_and_the_composed_chain(L, stream, ti, ii):
    hi = (ti + ii) % len(HEADS)
    n = _net(L, stream, ti, ii, hi)
    ec_all = e32_all = 0.0
    for R in RS:
        ref = n.ref(R, torch.float64)
        got = _fused(L, stream, [n], R)[0]
        comp = n.composed(L, stream, R)
        e_f = (got.double() - ref).abs().max().item()
        e_c = (comp.double() - ref).abs().max().item()
        e_32 = (n.ref(R, torch.float32).double() - ref).abs().max().item()
        ec_all, e32_all = max(ec_all, e_c), max(e32_all, e_32)
        print(f"MLPSTEP R={R} F={n.F} ldx={n.ldx} torso={n.widths} act={n.act} final={int(n.final)} head=({n.nout},{n.ldy}) small={int(n.small)}: "
              f"fused err {e_f:.3e} composed err {e_c:.3e} ratio {e_f / max(e_c, 1e-300):.2f} fp32-torch err {e_32:.3e} "
              f"outputs that differ from the composed chain's {int((got != comp).sum())} of {got.numel()}")
        assert e_f <= 1.25 * e_c, f"fused {e_f:.3e} > 1.25 x composed {e_c:.3e}"
    print(f"MLPSTEP yardstick F={n.F} ldx={n.ldx} torso={n.widths} act={n.act} head=({n.nout},{n.ldy}): composed err {ec_all:.3e} fp32-torch err {e32_all:.3e} "
          f"ratio {ec_all / max(e32_all, 1e-300):.2f}")
    assert ec_all <= 4.0 * e32_all, "the yardstick itself is off"


PAIRS = [((0, 0, 0), (2, 3, 2)),     # default actor on 7-float rows | three-layer critic on 128-stride rows, value vector
         ((1, 2, 1), (3, 4, 2)),     # one layer tanh on global-state rows | two layers without final activation
         ((4, 1, 0), (0, 2, 2)),     # the wider network first
         ((5, 3, 1), (6, 1, 0))]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "-".join("".join(map(str, k)) for k in p))
def test_two_networks_in_one_launch_equal_their_single_launches(L, stream, pair):
    nets = [_net(L, stream, *k) for k in pair]
    for R in RS:
        both = _fused(L, stream, nets, R)
        for k, n in enumerate(nets):
            alone = _fused(L, stream, [n], R)[0]
            same = torch.equal(both[k].view(torch.int32), alone.view(torch.int32))
            print(f"MLPSTEP pair R={R} network {k} torso={n.widths} F={n.F} head=({n.nout},{n.ldy}): bit-equal to its single launch {same}")
            assert same
            ref = n.ref(R, torch.float64)
            assert (both[k].double() - ref).abs().max().item() < 1e-4    # and it is the network's own result, not the other's


@pytest.mark.parametrize("key", [(0, 0, 0), (2, 2, 2), (3, 3, 1), (1, 1, 0)], ids=lambda k: "".join(map(str, k)))
def test_nan_outside_the_read_region_changes_nothing(L, stream, key):
    """Columns >= F and rows >= R are never read: NaN there (every fused call of this module) gives the bits that zeros give; the input
    buffers are unchanged and everything outside columns 0..NOUT-1 of rows 0..R-1 keeps its sentinel (_fused asserts both)."""
    n = _net(L, stream, *key)
    for R in RS:
        clean = n.x_clean.clone()
        clean[R:] = 0.0
        a = _fused(L, stream, [n], R, xs=[clean])[0]
        b = _fused(L, stream, [n], R)[0]
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        print(f"MLPSTEP nan R={R} F={n.F} ldx={n.ldx} torso={n.widths}: NaN padding leaves every output bit unchanged {same}")
        assert same and not bool(torch.isnan(b).any())


def test_step_rejects_bad_arguments_before_any_launch(L, stream):
    R = 8
    n = _net(L, stream, 2, 2, 0)     # three layers: every pointer slot is used
    x = n.x_for(R)
    out = Guard(R, n.nout, n.ldy)
    good_d, good_p = [1] + n.dims(), ptr_table(n.ptrs(x, out))
    two_d, two_p = [2] + n.dims() + n.dims(), ptr_table(n.ptrs(x, out) + n.ptrs(x, out))

    def call(dims, ptrs, nptrs, R_=R):
        d = None if dims is None else np.array(dims, dtype=np.int32)
        with pytest.raises(ValueError):
            L.call("magpo_mlp_act_step", None if d is None else d.ctypes.data, None if ptrs is None else ptrs.ctypes.data, nptrs, R_, stream)

    def with_(i, v, base=good_d):
        d = list(base); d[i] = v
        return d

    # dims: [nnets, F, ldx, layers, w0, w1, w2, act, final, NOUT, ldy]
    call(good_d, good_p, 10, 0)                      # R < 1
    call(good_d, good_p, 10, -3)
    for nn in (0, 3):
        call(with_(0, nn), good_p, 10)               # nnets
    call(good_d, good_p, 9)                          # table size
    call(good_d, good_p, 20)
    call(two_d, two_p, 10)
    for nl in (0, 4):
        call(with_(3, nl), good_p, 10)               # layer count
    for slot in (4, 5, 6):
        for w in (0, 32, 96, 320):
            call(with_(slot, w), good_p, 10)         # a width outside the set
    call(with_(11 + 4, 96, two_d), two_p, 20)        # ... of the second network
    for F in (0, 129, n.ldx + 1):
        call(with_(1, F), good_p, 10)                # F out of range, or ldx < F
    call(with_(2, n.F - 1), good_p, 10)
    for nout in (0, 33, n.ldy + 1):
        call(with_(9, nout), good_p, 10)             # NOUT out of range, or ldy < NOUT
    call(with_(10, n.nout - 1), good_p, 10)
    for act in (0, 2, 3, 4, 6, -1):
        call(with_(7, act), good_p, 10)              # unknown activation code
    call(with_(8, 2), good_p, 10)                    # activate_final is a flag
    call(None, good_p, 10)                           # null tables
    call(good_d, None, 10)
    for j in range(10):                              # a null pointer in a used slot
        bad = good_p.copy(); bad[j] = 0
        call(good_d, bad, 10)
    torch.cuda.synchronize()
    out.check("rejected calls", torch.zeros(R, dtype=torch.bool))
    assert bool(torch.isnan(out.out).all()), "a rejected call launched"
