"""The QMIX kernels (csrc/qmix.hip, csrc/qlearn.hip) against the fp64 restatement (tests/qmix_ref.py): the mixer's forward and backward at
shapes around the 16-row tile and the parameter limits, its kinks, monotonicity and bit-stability, the column-selection modes with the
64-wide scatter, the sequence gather bit for bit against numpy, the TD loss, and the argument checks.  Bounds as tests/test_q_learner_gpu.py:
values 1e-4 absolute at O(1) magnitudes, gradients 2e-3 x max|reference|."""
import numpy as np
import pytest
import torch

from tests import iql_ref
from tests import qmix_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _close(got, want, bound, what):
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    err = (got - want).abs().max().item()
    print(f"CHECK {what}: err {err:.3e} bound {bound:.3e} ref {want.abs().max().item():.3e}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _params(seed, A, E, G):
    """The restatement's parameters with the two hypernetwork output layers scaled so that q_tot stays O(1) (the value bound is absolute)."""
    p = ref.mixer_init(seed, A, E, G)
    for n in ("hyper_w1/Dense_1", "hyper_w2/Dense_1"):
        p[n + "/kernel"] = p[n + "/kernel"] * 0.05
    return p


def _inputs(seed, A, F_raw, id_cols, R, ld_extra=3):
    g = torch.Generator().manual_seed(seed)
    ld = id_cols + F_raw + ld_extra
    return torch.randn(R * A, ld, generator=g), torch.randn(R, A, generator=g), torch.randn(R, generator=g)


def _mixer(p, A, E, F_raw, id_cols, norm):
    from magpo_amd.qmix_net import QMixer
    mx = QMixer(A, E, F_raw, DEV, id_cols=id_cols, norm_env_states=norm)
    mx.load_named(p)
    return mx


def _reference(p, obs, q, dq_tot, A, E, F_raw, id_cols, norm):
    """fp64 q_tot and the gradients of sum(q_tot * dq_tot) with respect to q and every parameter."""
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    q64 = q.double().requires_grad_(True)
    s = ref.global_state(obs.double().view(-1, A, obs.shape[1])[..., :id_cols + F_raw], id_cols)
    q_tot = ref.mixer_apply(p64, q64, s, E, norm)
    grads = torch.autograd.grad((q_tot * dq_tot.double()).sum(), [q64] + list(p64.values()), allow_unused=True)
    gp = {k: (torch.zeros_like(v) if g_ is None else g_) for (k, v), g_ in zip(p64.items(), grads[1:])}
    return q_tot.detach(), grads[0], gp


def _run(mx, obs, q, dq_tot, R):
    q_tot = mx.apply(obs.to(DEV), obs.shape[1], R, q.to(DEV).contiguous(), train=True)
    dq = torch.empty(R, mx.A, device=DEV)
    mx.bwd(dq_tot.to(DEV), dq=dq)
    return q_tot.clone(), dq, {k: v.clone() for k, v in mx.named_grads.items()}


# (A, E, F_raw, id_cols, R, norm): every A in {1, 2, 3, 8}, E in {32, 64}, G = A F_raw in {5, 18, 128}, id_cols in {0, A}, R in {1, 63, 65, 257}
# around the 16-row tile, both norm settings; A E = 512 and G = 128 are the limits; R = 2065 = 130 tiles makes workgroups fold a second tile
# into their slab (the grid stops at 128)
CASES = [(1, 32, 5, 0, 1, True), (2, 64, 9, 2, 63, True), (3, 32, 6, 3, 65, False), (8, 64, 16, 8, 257, True), (8, 32, 16, 0, 65, True),
         (3, 64, 6, 0, 257, False), (2, 32, 64, 2, 63, False), (1, 64, 5, 1, 257, True), (2, 32, 9, 2, 2065, True)]


@pytest.mark.parametrize("A,E,F_raw,id_cols,R,norm", CASES)
def test_mixer_forward_and_backward_match_fp64(A, E, F_raw, id_cols, R, norm):
    G = A * F_raw
    p = _params(11 + A + E, A, E, G)
    obs, q, dq_tot = _inputs(R + G, A, F_raw, id_cols, R)
    want_q, want_dq, want_g = _reference(p, obs, q, dq_tot, A, E, F_raw, id_cols, norm)
    mx = _mixer(p, A, E, F_raw, id_cols, norm)
    q_tot, dq, grads = _run(mx, obs, q, dq_tot, R)
    tag = f"A{A} E{E} G{G} id{id_cols} R{R} norm{int(norm)}"
    _close(q_tot, want_q, 1e-4, f"{tag} q_tot")
    _close(dq, want_dq, 2e-3 * want_dq.abs().max().item(), f"{tag} dq")
    for n, gv in grads.items():
        want = want_g[n].reshape(gv.shape)
        if not norm and n.startswith("layer_norm"):
            assert not gv.any(), n
            continue
        _close(gv, want, 2e-3 * max(want.abs().max().item(), 1e-30), f"{tag} grad {n}")
    assert torch.isfinite(mx.grads).all() and not mx.grads[mx.P.offsets["hyper_b2/Dense_1/bias"] + 1: mx.P.offsets["layer_norm/scale"]].any(), "padding must be zero"
    # the backward twice: equal bits
    _, dq2, grads2 = _run(mx, obs, q, dq_tot, R)
    assert torch.equal(dq, dq2) and all(torch.equal(grads[n], grads2[n]) for n in grads), "two runs must give the same bits"
    # eval mode (nothing saved) gives the training mode's values
    assert torch.equal(mx.apply(obs.to(DEV), obs.shape[1], R, q.to(DEV).contiguous(), tag="eval_"), q_tot)


def test_workspace_sizes():
    """The two sizing entry points, and that QMixer sizes its buffers by them."""
    from magpo_amd._lib import lib
    save, grid = lib().raw("magpo_qmix_save_floats"), lib().raw("magpo_qmix_bwd_grid")
    assert [save(E, G) for E, G in ((32, 5), (64, 18), (64, 128))] == [128 + 64 + 8 + 4, 128 + 128 + 20 + 4, 128 + 128 + 128 + 4]
    assert [grid(R) for R in (1, 16, 17, 2048, 2049, 10 ** 6)] == [1, 1, 2, 128, 128, 128]      # one workgroup per 16-row tile, at most 128
    A, E, F_raw, R = 2, 32, 9, 40
    mx = _mixer(_params(1, A, E, A * F_raw), A, E, F_raw, A, True)
    _run(mx, *_inputs(1, A, F_raw, A, R), R)
    assert mx._saved["save"].shape == (R, save(E, A * F_raw)) and mx._buf["slab"].shape == (grid(R), mx.P.numel)


def test_mixer_is_monotonic_in_every_agent_value():
    A, E, F_raw, R = 3, 32, 6, 65
    mx = _mixer(_params(4, A, E, A * F_raw), A, E, F_raw, A, True)
    obs, q, _ = _inputs(9, A, F_raw, A, R)
    obs, q = obs.to(DEV), q.to(DEV)
    base = mx.apply(obs, obs.shape[1], R, q).clone()
    g = torch.Generator().manual_seed(2)
    for a in range(A):
        up = q.clone()
        up[:, a] += torch.rand(R, generator=g).to(DEV) * 3.0
        assert (mx.apply(obs, obs.shape[1], R, up.contiguous()) >= base).all(), f"raising agent {a}'s value lowered q_tot"


def test_mixer_kinks():
    A, E, F_raw, R = 2, 32, 9, 40
    G = A * F_raw
    # |0|: the last layer of hyper_w1 and its bias zeroed -> w1 = 0: no gradient into that hypernetwork, q_tot independent of q
    p = _params(6, A, E, G)
    p["hyper_w1/Dense_1/kernel"].zero_(); p["hyper_w1/Dense_1/bias"].zero_()
    obs, q, dq_tot = _inputs(5, A, F_raw, A, R)
    mx = _mixer(p, A, E, F_raw, A, True)
    q_tot, dq, grads = _run(mx, obs, q, dq_tot, R)
    for n in ("hyper_w1/Dense_1/kernel", "hyper_w1/Dense_1/bias", "hyper_w1/Dense_0/kernel", "hyper_w1/Dense_0/bias"):
        assert not grads[n].any(), f"sign(0) = 0: {n} must have no gradient"
    assert not dq.any()
    assert torch.equal(mx.apply(obs.to(DEV), obs.shape[1], R, (q * 7 + 1).to(DEV).contiguous(), tag="k_"), q_tot)
    want_q, _, want_g = _reference(p, obs, q, dq_tot, A, E, F_raw, A, True)
    _close(q_tot, want_q, 1e-4, "|0| q_tot")
    for n in ("hyper_b1/Dense_0/kernel", "hyper_w2/Dense_1/kernel", "layer_norm/scale"):
        _close(grads[n], want_g[n], 2e-3 * want_g[n].abs().max().item(), f"|0| grad {n}")
    # elu at 0: b1 = 0 and one row with q = 0 -> that row's pre-activations are exactly 0, where elu' = 1
    p = _params(7, A, E, G)
    p["hyper_b1/Dense_0/kernel"].zero_(); p["hyper_b1/Dense_0/bias"].zero_()
    q[3] = 0.0
    mx = _mixer(p, A, E, F_raw, A, True)
    q_tot, dq, grads = _run(mx, obs, q, dq_tot, R)
    assert not mx._saved["save"][3, 128 + E:128 + 2 * E].any(), "the row's hidden must be exactly 0"
    want_q, want_dq, want_g = _reference(p, obs, q, dq_tot, A, E, F_raw, A, True)
    assert want_dq[3].abs().min() > 0
    _close(dq[3], want_dq[3], 2e-3 * want_dq.abs().max().item(), "elu(0) dq of the kink row")
    _close(dq, want_dq, 2e-3 * want_dq.abs().max().item(), "elu(0) dq")
    for n, gv in grads.items():
        _close(gv, want_g[n].reshape(gv.shape), 2e-3 * max(want_g[n].abs().max().item(), 1e-30), f"elu(0) grad {n}")


@pytest.mark.parametrize("has_mask", [True, False])
def test_column_selection_modes_and_the_scatter(has_mask):
    """Mode 1 (taken actions, steps 0 .. L-2) and mode 2 (double-Q selection, steps 1 .. L-1) on 64-wide Q rows of B windows of L steps, and
    the backward's scatter into 64-wide gradient rows."""
    A, E, F_raw, K, B, L_ = 3, 32, 6, 5, 7, 4
    T, G = L_ - 1, A * F_raw
    Rm, rows = B * T, B * L_ * A
    g = torch.Generator().manual_seed(8)
    obs = torch.randn(rows, A + F_raw, generator=g)
    qo, qt = torch.zeros(rows, 64), torch.zeros(rows, 64)
    qo[:, :K], qt[:, :K] = torch.randn(rows, K, generator=g), torch.randn(rows, K, generator=g)
    mask = (torch.rand(rows, K, generator=g) < 0.6).to(torch.uint8)
    mask[torch.arange(rows), torch.randint(0, K, (rows,), generator=g)] = 1
    action = torch.randint(0, K, (Rm, A), generator=g).to(torch.int32)
    dq_tot = torch.randn(Rm, generator=g)
    p = _params(3, A, E, G)
    mx = _mixer(p, A, E, F_raw, A, True)
    d = lambda x: x.to(DEV).contiguous()
    # the restatement on explicit slices
    o5 = obs.view(B, L_, A, -1)
    m5 = mask.view(B, L_, A, K) if has_mask else None
    qo5, qt5 = qo.view(B, L_, A, 64)[..., :K].double(), qt.view(B, L_, A, 64)[..., :K].double()
    next_a = torch.from_numpy(iql_ref.greedy_action(qo5[:, 1:].numpy(), None if m5 is None else m5[:, 1:].numpy())).long()
    next_q = torch.gather(qt5[:, 1:], -1, next_a[..., None])[..., 0].reshape(Rm, A)
    q_sel = torch.gather(qo5[:, :-1], -1, action.view(B, T, A).long()[..., None])[..., 0].reshape(Rm, A)
    p64 = {k: v.double() for k, v in p.items()}
    want_next = ref.mixer_apply(p64, next_q, ref.global_state(o5[:, 1:].double(), A).reshape(Rm, G), E)
    qs = q_sel.clone().requires_grad_(True)
    want_tot = ref.mixer_apply(p64, qs, ref.global_state(o5[:, :-1].double(), A).reshape(Rm, G), E)
    want_dq, = torch.autograd.grad((want_tot * dq_tot.double()).sum(), qs)
    nxt = mx.apply(d(obs), obs.shape[1], Rm, d(qt), q_online=d(qo), mask=d(mask) if has_mask else None, K=K, steps=(T, L_, 1), tag="n_").clone()
    _close(nxt, want_next, 1e-4, "double-Q q_tot")
    assert torch.equal(mx._buf["n_q_used"].cpu(), next_q.float()), "the selected target values must be the restatement's, bit for bit"
    tot = mx.apply(d(obs), obs.shape[1], Rm, d(qo), index=d(action), K=K, steps=(T, L_, 0), train=True)
    _close(tot, want_tot.detach(), 1e-4, "taken-action q_tot")
    dq64 = torch.full((rows, 64), 7.0, device=DEV)
    dq = torch.empty(Rm, A, device=DEV)
    mx.bwd(d(dq_tot), dq=dq, dq64=dq64)
    _close(dq, want_dq, 2e-3 * want_dq.abs().max().item(), "taken-action dq")
    got = dq64.cpu().view(B, L_, A, 64)
    assert (got[:, -1] == 7.0).all(), "rows of step L - 1 are not the mixer's to write"
    want64 = torch.zeros(B, T, A, 64)
    want64.scatter_(-1, action.view(B, T, A, 1).long(), dq.cpu().view(B, T, A, 1))
    assert torch.equal(got[:, :-1], want64), "dq in the taken action's column, zero elsewhere"


# ----------------------------------------------------------------------------- sequence gather and team reward
@pytest.mark.parametrize("adds", [5, 8, 11], ids=["before-wrap", "exactly-full", "after-wrap"])
@pytest.mark.parametrize("has_mask", [True, False])
def test_replay_gather_seq_bit_for_bit(adds, has_mask):
    from magpo_amd._lib import lib
    from oracle import prng
    N, S, A, F, K, B, L_ = 3, 8, 2, 5, 4, 6, 4
    ring = iql_ref.Ring(N, S, A, F, K, has_mask)
    rng = np.random.default_rng(adds)
    for _ in range(adds):
        ring.add(obs=rng.standard_normal((N, A, F)).astype(np.float32), mask=rng.integers(0, 2, (N, A, K)), action=rng.integers(0, K, (N, A)),
                 reward=ref.team_reward(rng.standard_normal((N, A))), terminal=rng.integers(0, 2, N), term_or_trunc=rng.integers(0, 2, N),
                 next_obs=rng.standard_normal((N, A, F)).astype(np.float32), next_mask=rng.integers(0, 2, (N, A, K)))
    env_idx, start = ring.sample_indices(prng.prng_key(adds), B, L_)
    assert adds <= S or (start + L_ > S).any(), "a sampled window must cross the end of the ring"
    win = ring.gather(env_idx, start, L_)
    t = lambda k: None if ring.data[k] is None else torch.from_numpy(ring.data[k]).to(DEV)
    fields = [t(k) for k in ("obs", "mask", "action", "reward", "terminal", "term_or_trunc", "next_obs", "next_mask")]
    ldo = F + 3
    o_obs = torch.full((B * L_ * A, ldo), -9.0, device=DEV)
    o_mask = torch.zeros(B * L_ * A, K, dtype=torch.uint8, device=DEV) if has_mask else None
    o_tot = torch.zeros(B, L_, dtype=torch.uint8, device=DEV)
    o_act = torch.zeros(B, L_ - 1, A, dtype=torch.int32, device=DEV)
    o_rew = torch.zeros(B, L_ - 1, device=DEV)
    lib().call("magpo_replay_gather_seq", *fields, N, S, A, F, K, torch.from_numpy(env_idx).to(DEV), torch.from_numpy(start).to(DEV), B, L_, o_obs, ldo, o_mask,
               o_tot, o_act, o_rew, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(o_obs.cpu().numpy()[:, :F].reshape(B, L_, A, F), win["obs"]) and (o_obs[:, F:] == -9.0).all()
    if has_mask:
        assert np.array_equal(o_mask.cpu().numpy().reshape(B, L_, A, K), win["mask"])
    assert np.array_equal(o_tot.cpu().numpy(), win["term_or_trunc"])
    assert np.array_equal(o_act.cpu().numpy(), win["action"][:, :-1])
    assert np.array_equal(o_rew.cpu().numpy(), win["reward"][:, :-1, 0])


def test_team_reward_bit_for_bit():
    from magpo_amd._lib import lib
    for N, A in ((1, 1), (5, 3), (300, 8)):
        r = np.random.default_rng(N).standard_normal((N, A)).astype(np.float32)
        d = torch.from_numpy(r).to(DEV)
        lib().call("magpo_team_reward", d, d, N, A, torch.cuda.current_stream().cuda_stream)
        assert np.array_equal(d.cpu().numpy(), ref.team_reward(r))


# ----------------------------------------------------------------------------- TD loss
@pytest.mark.parametrize("U", [1, 2])
def test_td_loss_matches_restatement(U):
    from magpo_amd._lib import lib
    B, L_, gamma = 5, 4, 0.99
    T = L_ - 1
    R = U * B * T
    g = torch.Generator().manual_seed(U)
    q, nq, rew = torch.randn(U * B, T, generator=g), torch.randn(U * B, T, generator=g), torch.randn(U * B, T, generator=g)
    tot = (torch.rand(U * B, L_, generator=g) < 0.3).to(torch.uint8)
    tot[1, 2] = 1     # step 2 of window 1 ends by truncation: term_or_trunc = 1 while terminal = 0 -- the bootstrap of row (1, 1) is cut all the same
    terminal = torch.zeros_like(tot)
    dq = torch.empty(R, device=DEV)
    out = torch.zeros(8, device=DEV)
    ws = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)
    lib().call("magpo_qmix_td_loss", q.to(DEV), nq.to(DEV), rew.to(DEV), tot.to(DEV), L_, gamma, dq, ws, out, R, U, torch.cuda.current_stream().cuda_stream)
    f = np.float32
    done = tot[:, 1:].numpy().astype(np.float32)
    target = (rew.numpy() + ((f(1) - done) * f(gamma)).astype(f) * nq.numpy()).astype(f)
    want_dq = (f(f(2.0) / f(R)) * (q.numpy() - target).astype(f)).astype(f)
    assert np.array_equal(dq.cpu().numpy().reshape(U * B, T), want_dq), "dq_tot: every operation rounded to fp32 in the stated order"
    assert target[1, 1] == rew.numpy()[1, 1] and terminal[1, 2] == 0, "truncation must cut the bootstrap"
    infos = [ref.td_loss(q[u * B:(u + 1) * B].double(), nq[u * B:(u + 1) * B].double(), rew[u * B:(u + 1) * B].double(), tot[u * B:(u + 1) * B], gamma)[1] for u in range(U)]
    got = out.cpu().numpy()
    for i, name in enumerate(ref.LOSS_NAMES):
        want = sum(float(info[name]) for info in infos) / U     # pmean over the groups
        print(f"CHECK td_loss U{U} {name}: got {got[i]:.6f} want {want:.6f}")
        assert abs(got[i] - want) <= 1e-3, (name, got[i], want)


# ----------------------------------------------------------------------------- argument checks: rejected with null pointers
def test_invalid_arguments_are_rejected_before_a_pointer_is_touched():
    from magpo_amd._lib import lib
    L, st = lib(), 0
    offs = np.arange(16, dtype=np.int64) * 4096
    good = [2, 32, 18, 9, 2, 1, 1, 1, 0, 0, 0]     # A, E, G, F_raw, id_cols, norm, Tm, Ts, t_off, mode, K

    def fwd(dims, R=4, ndims=11, noffs=16, offs=offs, ldo=64):
        d = np.array(dims, np.int32)
        L.call("magpo_qmix_fwd", d.ctypes.data, ndims, None, offs.ctypes.data, noffs, None, ldo, None, None, 64, None, None, None, None, None, R, st)

    def bwd(dims, R=4, P=1 << 20, offs=offs):
        d = np.array(dims, np.int32)
        L.call("magpo_qmix_bwd", d.ctypes.data, 11, None, offs.ctypes.data, 16, P, None, None, None, None, None, 64, None, None, None, R, st)

    def alt(**kw):
        names = ["A", "E", "G", "F_raw", "id_cols", "norm", "Tm", "Ts", "t_off", "mode", "K"]
        return [kw.get(n, v) for n, v in zip(names, good)]

    bad_dims = [alt(E=16), alt(E=48), alt(A=0, G=0), alt(A=17, G=17 * 9), alt(E=64, A=9, G=81), alt(G=19), alt(F_raw=0, G=0), alt(A=2, F_raw=65, G=130),
                alt(id_cols=-1), alt(norm=2), alt(Tm=0), alt(Tm=3, Ts=2), alt(Tm=2, Ts=3, t_off=2), alt(mode=3), alt(mode=1, K=0), alt(mode=2, K=33)]
    for dims in bad_dims:
        for call in (fwd, bwd):
            with pytest.raises(ValueError):
                call(dims)
    for call in (fwd, bwd):
        with pytest.raises(ValueError):
            call(good, R=0)
        with pytest.raises(ValueError):
            call(good, offs=offs + 1)       # offsets must be multiples of 4 floats
        with pytest.raises(ValueError):
            call(good)                      # valid shape, NULL pointers
    with pytest.raises(ValueError):
        fwd(good, ndims=10)
    with pytest.raises(ValueError):
        fwd(good, noffs=15)
    with pytest.raises(ValueError):
        fwd(good, ldo=10)                   # the row stride must cover id_cols + F_raw
    with pytest.raises(ValueError):
        bwd(good, P=4096)                   # an entry outside the buffer
    for L_, U, R in ((1, 1, 4), (4, 0, 6), (4, 1025, 3 * 1025), (4, 2, 9), (4, 1, 4), (4, 1, 0), (4, 1, 6)):     # the last one: valid shape, NULL pointers
        with pytest.raises(ValueError):
            L.call("magpo_qmix_td_loss", None, None, None, None, L_, 0.99, None, None, None, R, U, st)
    for B, L_, S in ((0, 4, 8), (2, 1, 8), (2, 9, 8), (2, 4, 8)):      # the last one: valid shape, NULL pointers
        with pytest.raises(ValueError):
            L.call("magpo_replay_gather_seq", None, None, None, None, None, None, None, None, 3, S, 2, 5, 4, None, None, B, L_, None, 5, None, None, None, None, st)
    for N, A in ((0, 2), (2, 0), (2, 2)):
        with pytest.raises(ValueError):
            L.call("magpo_team_reward", None, None, N, A, st)
