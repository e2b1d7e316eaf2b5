"""The Q-learning kernels (csrc/qlearn.hip) and the env kernels' real_next_obs against their restatement (tests/iql_ref.py, oracle envs):
sampling, ring copies, target update and env outputs bit for bit; the TD loss against float64 on the same float32 inputs."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import coordsum as ocs
from oracle import lbf as olbf
from oracle import prng as oprng
from tests import iql_ref as ref
from tests.gpu_util import DEV, PAD, Guard, check

pytestmark = pytest.mark.gpu

I32, U8 = torch.int32, torch.uint8


class ByteGuard:
    """tests.gpu_util.Guard for uint8 outputs (its sentinel does not fit a byte): R x W owned bytes pre-filled with 9 between guard rows of 200."""

    def __init__(self, R, W):
        self.R = R
        self.full = torch.full((R + 2 * PAD, W), 200, device=DEV, dtype=torch.uint8)
        self.rows = self.out = self.full[PAD:PAD + R]
        self.rows.fill_(9)

    def check(self, what):
        assert not bool((self.out == 9).any()), f"{what}: elements of the output were never written"
        t = self.full.clone()
        t[PAD:PAD + self.R] = 200
        assert bool((t == 200).all()), f"{what}: elements outside the owned block were overwritten"


def _key_words(key):
    return int(key[0]), int(key[1])


def _dev_int(v):
    return torch.tensor([v], dtype=I32, device=DEV)


# ----------------------------------------------------------------------------- magpo_eps_greedy_sample
EPS_MIN, EPS_DECAY = 0.05, 1000.0
# (eps_min, t or None) -> eps 1, 0.05, 0 and the null counter
EPS_CASES = [(EPS_MIN, 0), (EPS_MIN, 1000), (EPS_MIN, 5000), (0.0, 1000), (EPS_MIN, None)]


def _q_rows(R, K, seed, masked):
    rng = np.random.default_rng(seed)
    q = np.full((R, 64), np.nan, np.float32)
    q[:, :K] = rng.standard_normal((R, K)).astype(np.float32)
    if not masked:
        return q, None
    m = rng.random((R, K)) < 0.6
    m[np.arange(R), rng.integers(0, K, R)] = True           # one legal action at least
    m[0] = False; m[0, K - 1] = True                        # a single legal action
    top = np.argmax(q[:, :K], axis=1)
    for r in range(1, R, 2):                                # the largest Q illegal
        if m[r].sum() > 1 or not m[r, top[r]]:
            m[r, top[r]] = False
        if not m[r].any():
            m[r, (top[r] + 1) % K] = True
    if R > 2:
        q[2, :K] = 0.25                                     # exactly equal Q values: the first legal one wins
    return q, m.astype(np.uint8)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("K", [2, 6, 20, 32])
@pytest.mark.parametrize("R", [1, 63, 65, 130])
def test_eps_greedy_sample_matches_restatement(L, stream, R, K, masked):
    q, m = _q_rows(R, K, 100 * R + K, masked)
    qd = torch.from_numpy(q).to(DEV)
    md = None if m is None else torch.from_numpy(m).to(DEV)
    key = oprng.split(oprng.prng_key(7 * R + K), 2)[1]
    kd = torch.from_numpy(key.view(np.int32).copy()).to(DEV)
    for eps_min, t in EPS_CASES:
        eps = np.float32(0.0) if t is None else ref.epsilon(t, eps_min, EPS_DECAY)
        want_a, want_g = ref.eps_greedy_sample(key, q[:, :K], m, eps)
        for on_dev in (False, True):
            act, gr = Guard(R, 1, dtype=I32), Guard(R, 1, dtype=I32)
            k0, k1 = (0, 0) if on_dev else _key_words(key)
            L.call("magpo_eps_greedy_sample", qd, 64, md, k0, k1, kd if on_dev else None, None if t is None else _dev_int(t), eps_min, EPS_DECAY,
                   act, gr, R, K, stream)
            act.check("action"); gr.check("greedy")
            assert np.array_equal(act.out[:, 0].cpu().numpy(), want_a), (eps_min, t, on_dev)
            assert np.array_equal(gr.out[:, 0].cpu().numpy(), want_g), (eps_min, t, on_dev)
        if m is not None:
            assert m[np.arange(R), want_a].all(), "a sampled action is illegal"
        if float(eps) == 0.0:   # the masked greedy action whatever the key
            assert np.array_equal(want_a, want_g)
            other = Guard(R, 1, dtype=I32)
            L.call("magpo_eps_greedy_sample", qd, 64, md, 123, 456, None, None if t is None else _dev_int(t), eps_min, EPS_DECAY, other, None, R, K, stream)
            assert np.array_equal(other.out[:, 0].cpu().numpy(), want_g)
    if R >= 63 and K >= 6:
        a1, _ = ref.eps_greedy_sample(key, q[:, :K], m, np.float32(1.0))
        assert (a1 != ref.greedy_action(q[:, :K], m)).any(), "eps = 1 must explore"


def test_eps_greedy_sample_rejects_bad_arguments(L, stream):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for args in [(p, 64, None, 0, 0, None, None, 0.05, 10.0, p, None, 4, 33),      # K > 32
                 (p, 64, None, 0, 0, None, None, 0.05, 10.0, p, None, 4, 0),       # K < 1
                 (p, 4, None, 0, 0, None, None, 0.05, 10.0, p, None, 4, 6),        # ld < K
                 (None, 64, None, 0, 0, None, None, 0.05, 10.0, p, None, 4, 6),    # no Q rows
                 (p, 64, None, 0, 0, None, None, 0.05, 10.0, None, None, 4, 6),    # no output
                 (p, 64, None, 0, 0, None, p, 0.05, 0.0, p, None, 4, 6),           # eps_decay = 0 with a counter
                 (p, 64, None, 0, 0, None, p, 1.5, 10.0, p, None, 4, 6)]:          # eps_min > 1
        with pytest.raises(ValueError):
            L.call("magpo_eps_greedy_sample", *args, stream)


# ----------------------------------------------------------------------------- magpo_replay_add / magpo_replay_gather
S_, LW, N_, A_ = 8, 4, 3, 2


class DevRing:
    def __init__(self, N, S, A, F, K, has_mask):
        z = lambda shape, dt: torch.zeros(N, S, *shape, dtype=dt, device=DEV)
        self.dims = (N, S, A, F, K)
        self.obs, self.next_obs = z((A, F), torch.float32), z((A, F), torch.float32)
        self.mask, self.next_mask = (z((A, K), U8), z((A, K), U8)) if has_mask else (None, None)
        self.action, self.reward = z((A,), I32), z((A,), torch.float32)
        self.terminal, self.tot = z((), U8), z((), U8)
        self.cursor, self.filled = _dev_int(0), _dev_int(0)

    def fields(self):
        return (self.obs, self.mask, self.action, self.reward, self.terminal, self.tot, self.next_obs, self.next_mask)

    def add(self, L, stream, step, ld):
        L.call("magpo_replay_add", *self.fields(), self.cursor, self.filled, *self.dims, step["obs"], ld, step["mask"], step["action"], step["reward"],
               step["terminal"], step["term_or_trunc"], step["next_obs"], ld, step["next_mask"], stream)

    def equals(self, r: ref.Ring):
        names = dict(obs=self.obs, mask=self.mask, action=self.action, reward=self.reward, terminal=self.terminal, term_or_trunc=self.tot,
                     next_obs=self.next_obs, next_mask=self.next_mask)
        for k, v in names.items():
            if v is not None:
                assert np.array_equal(v.cpu().numpy(), r.data[k]), k
        assert (int(self.cursor), int(self.filled)) == (r.cursor, r.filled)


def _steps(n_steps, N, A, F, K, ld, has_mask, seed):
    """Host steps (dense) and their device copies with row stride ld >= F (the gap holds a sentinel)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_steps):
        h = dict(obs=rng.standard_normal((N, A, F)).astype(np.float32), next_obs=rng.standard_normal((N, A, F)).astype(np.float32),
                 mask=(rng.random((N, A, K)) < 0.5).astype(np.uint8) if has_mask else None,
                 next_mask=(rng.random((N, A, K)) < 0.5).astype(np.uint8) if has_mask else None,
                 action=rng.integers(0, K, (N, A)).astype(np.int32), reward=rng.standard_normal((N, A)).astype(np.float32),
                 terminal=(rng.random(N) < 0.3).astype(np.uint8), term_or_trunc=(rng.random(N) < 0.5).astype(np.uint8))
        d = {}
        for k, v in h.items():
            if v is None:
                d[k] = None
            elif k in ("obs", "next_obs"):
                t = torch.full((N, A, ld), -777.0, device=DEV)
                t[..., :F] = torch.from_numpy(v).to(DEV)
                d[k] = t
            else:
                d[k] = torch.from_numpy(v).to(DEV)
        out.append((h, d))
    return out


@pytest.mark.parametrize("has_mask,F,K,ld", [(True, 14, 6, 14), (False, 3, 10, 5)], ids=["lbf-like", "coordsum-like"])
def test_replay_add_and_gather_are_exact_copies(L, stream, has_mask, F, K, ld):
    B, U = 5, 2
    rings = [ref.Ring(N_, S_, A_, F, K, has_mask) for _ in range(U)]
    drings = [DevRing(N_, S_, A_, F, K, has_mask) for _ in range(U)]
    steps = [_steps(10, N_, A_, F, K, ld, has_mask, 31 + u) for u in range(U)]
    for i in range(10):                      # ten adds: the ring of 8 wraps
        for u in range(U):
            h, d = steps[u][i]
            rings[u].add(**h)
            drings[u].add(L, stream, d, ld)
            drings[u].equals(rings[u])       # contents, cursor and filled after every add
    assert rings[0].cursor == 2 and rings[0].filled == S_
    # B = 5 windows with a repeated env row and one that wraps past the ring's end; two groups stacked
    env_idx, start = np.array([2, 0, 2, 1, 0], np.int32), np.array([2, 6, 3, 4, 7], np.int32)
    T = LW - 1
    R1 = B * T * A_
    old = 64
    o_obs, o_nobs = Guard(U * R1, F, ld=old), Guard(U * R1, F, ld=old)
    o_act, o_rew = Guard(U * R1, 1, dtype=I32), Guard(U * R1, 1)
    o_nmask = ByteGuard(U * R1, K) if has_mask else None
    o_tot, o_ntot, o_nterm = (ByteGuard(U * B, T) for _ in range(3))
    ei, sd = torch.from_numpy(env_idx).to(DEV), torch.from_numpy(start).to(DEV)
    for u in range(U):
        r, s = slice(u * R1, (u + 1) * R1), slice(u * B, (u + 1) * B)
        L.call("magpo_replay_gather", *drings[u].fields(), N_, S_, A_, F, K, ei, sd, B, LW, o_obs.rows[r], old, o_tot.rows[s], o_act.rows[r], o_rew.rows[r],
               o_nobs.rows[r], old, None if o_nmask is None else o_nmask.rows[r], o_ntot.rows[s], o_nterm.rows[s], stream)
    for g in (o_obs, o_nobs, o_act, o_rew, o_tot, o_ntot, o_nterm) + ((o_nmask,) if has_mask else ()):
        g.check("gather output")
    for u in range(U):
        rows = ref.training_rows(rings[u].gather(env_idx, start, LW))
        r, s = slice(u * R1, (u + 1) * R1), slice(u * B, (u + 1) * B)
        assert np.array_equal(o_obs.out[r].cpu().numpy(), rows["obs"].reshape(R1, F))
        assert np.array_equal(o_nobs.out[r].cpu().numpy(), rows["next_obs"].reshape(R1, F))
        assert np.array_equal(o_act.out[r, 0].cpu().numpy(), rows["action"].reshape(R1))
        assert np.array_equal(o_rew.out[r, 0].cpu().numpy(), rows["reward"].reshape(R1))
        assert np.array_equal(o_tot.out[s].cpu().numpy(), rows["term_or_trunc"])
        assert np.array_equal(o_ntot.out[s].cpu().numpy(), rows["next_term_or_trunc"])
        assert np.array_equal(o_nterm.out[s].cpu().numpy(), rows["next_terminal"])
        if has_mask:
            assert np.array_equal(o_nmask.out[r].cpu().numpy(), rows["next_mask"].reshape(R1, K))
    assert not np.array_equal(rings[0].data["obs"], rings[1].data["obs"])


def test_replay_add_graph_replay_equals_eager(L, stream):
    F, K, ld = 14, 6, 14
    (h0, d0), (h1, d1) = _steps(2, N_, A_, F, K, ld, True, 77)
    eager, graphed = DevRing(N_, S_, A_, F, K, True), DevRing(N_, S_, A_, F, K, True)
    for ring in (eager, graphed):          # start at slot 7, so that the two adds wrap the cursor
        ring.cursor.fill_(7); ring.filled.fill_(7)
    eager.add(L, stream, d0, ld); eager.add(L, stream, d1, ld)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream().cuda_stream
        graphed.add(L, st, d0, ld); graphed.add(L, st, d1, ld)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager.fields() + (eager.cursor, eager.filled), graphed.fields() + (graphed.cursor, graphed.filled)):
        assert torch.equal(a, b)
    assert (int(graphed.cursor), int(graphed.filled)) == (1, 8)


def test_replay_rejects_bad_arguments(L, stream):
    r = DevRing(N_, S_, A_, 3, 4, False)
    ei = torch.zeros(2, dtype=I32, device=DEV)
    with pytest.raises(ValueError):   # L > buffer_size
        L.call("magpo_replay_gather", *r.fields(), N_, S_, A_, 3, 4, ei, ei, 2, S_ + 1, r.obs, 3, r.tot, r.action, r.reward, r.obs, 3, None, r.tot, r.tot, stream)
    with pytest.raises(ValueError):   # L < 2
        L.call("magpo_replay_gather", *r.fields(), N_, S_, A_, 3, 4, ei, ei, 2, 1, r.obs, 3, r.tot, r.action, r.reward, r.obs, 3, None, r.tot, r.tot, stream)
    with pytest.raises(ValueError):   # no cursor
        L.call("magpo_replay_add", *r.fields(), None, r.filled, N_, S_, A_, 3, 4, r.obs, 3, None, r.action, r.reward, r.tot, r.tot, r.obs, 3, None, stream)
    with pytest.raises(ValueError):   # row stride < F
        L.call("magpo_replay_add", *r.fields(), r.cursor, r.filled, N_, S_, A_, 3, 4, r.obs, 2, None, r.action, r.reward, r.tot, r.tot, r.obs, 3, None, stream)


# ----------------------------------------------------------------------------- magpo_q_td_loss
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("K", [2, 20])
@pytest.mark.parametrize("R,A", [(1, 1), (65, 1), (4 * 3 * 2, 2)])
def test_q_td_loss_matches_fp64(L, stream, R, A, K, masked):
    rng = np.random.default_rng(R * 10 + K)
    mk = lambda: torch.from_numpy(rng.standard_normal((R, 64)).astype(np.float32))
    q, qo, qt = mk(), mk(), mk()
    action = torch.from_numpy(rng.integers(0, K, R).astype(np.int32))
    reward = torch.from_numpy(rng.standard_normal(R).astype(np.float32))
    term = torch.from_numpy((rng.random(R // A) < 0.4).astype(np.uint8))
    term[0] = 1                                                    # rows with next_terminal = 1
    mask = None
    if masked:
        m = rng.random((R, K)) < 0.6
        best = qo[:, :K].argmax(1).numpy()
        m[np.arange(R), best] = False                              # every row's best next action is illegal
        m[np.arange(R), (best + 1) % K] = True
        mask = torch.from_numpy(m.astype(np.uint8))
    gamma = 0.99
    q64 = q[:, :K].double().requires_grad_(True)
    loss, mean_q, mean_t, _, next_a = ref.td_loss(q64, qo[:, :K].double(), qt[:, :K].double(), action, mask, reward.double(),
                                                  term.double().repeat_interleave(A), gamma)
    (dq_ref,) = torch.autograd.grad(loss, q64)
    if masked:
        assert bool(mask[torch.arange(R), next_a].all()) and not bool((next_a == qo[:, :K].argmax(1)).any())
    outs = []
    for _ in range(2):
        dq = Guard(R, 64)
        ws = torch.zeros(8 * 1024, dtype=torch.float64, device=DEV)
        lo = torch.full((3,), float("nan"), device=DEV)
        L.call("magpo_q_td_loss", q.to(DEV), qo.to(DEV), qt.to(DEV), 64, action.to(DEV), None if mask is None else mask.to(DEV), reward.to(DEV),
               term.to(DEV), gamma, dq, 64, ws, lo, R, K, A, stream)
        dq.check("dq")
        outs.append((dq.out.clone(), lo.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls must give the same bits"
    dq_d, lo_d = outs[0]
    check("dq", dq_d[:, :K].cpu(), dq_ref, 1e-5 * dq_ref.abs().max().item())
    untouched = torch.ones(R, 64, dtype=torch.bool)
    untouched[torch.arange(R), action.long()] = False
    assert bool((dq_d.cpu()[untouched] == 0).all()), "columns other than the action's must be exactly 0"
    for name, got, want in zip(("q_loss", "mean_q", "mean_target"), lo_d.cpu().tolist(), (loss.item(), mean_q.item(), mean_t.item())):
        print(f"CHECK {name}: got {got:.9e} want {want:.9e} rel {abs(got - want) / abs(want):.3e}")
        assert abs(got - want) <= 1e-5 * abs(want), (name, got, want)


def test_q_td_loss_rejects_bad_arguments(L, stream):
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    good = [p, p, p, 64, p, None, p, p, 0.99, p, 64, p, p, 4, 6, 2]
    for i, v in [(13, 0), (13, 5), (14, 33), (3, 4), (10, 62), (0, None), (11, None)]:   # R < 1, R % A, K > 32, ld < K, lddq % 4, NULL q, NULL workspace
        bad = list(good)
        bad[i] = v
        with pytest.raises(ValueError):
            L.call("magpo_q_td_loss", *bad, stream)


# ----------------------------------------------------------------------------- magpo_target_update
@pytest.mark.parametrize("n", [1, 1023, 4097])
def test_target_update_incremental_is_exact(L, stream, n):
    rng = np.random.default_rng(n)
    online, target = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    tau = 0.005
    od = torch.from_numpy(online).to(DEV)
    tg = Guard(1, n)
    tg.out.copy_(torch.from_numpy(target).to(DEV))
    L.call("magpo_target_update", od, tg, n, 0, tau, None, 1, stream)
    tg.check("target")
    assert np.array_equal(tg.out[0].cpu().numpy(), ref.target_update(online, target, 0, tau, 0, 1))
    assert np.array_equal(od.cpu().numpy(), online)


@pytest.mark.parametrize("t_train,copies", [(0, True), (1, False), (200, True)])
def test_target_update_periodic(L, stream, t_train, copies):
    n, period = 1023, 200
    rng = np.random.default_rng(5)
    online, target = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    tg = torch.from_numpy(target).to(DEV)
    L.call("magpo_target_update", torch.from_numpy(online).to(DEV), tg, n, 1, 0.0, _dev_int(t_train), period, stream)
    want = ref.target_update(online, target, 1, 0.0, t_train, period)
    assert np.array_equal(tg.cpu().numpy(), want) and np.array_equal(want, online if copies else target)
    with pytest.raises(ValueError):
        L.call("magpo_target_update", tg, tg, n, 1, 0.0, None, period, stream)
    with pytest.raises(ValueError):
        L.call("magpo_target_update", tg, tg, n, 2, 0.0, None, period, stream)


# ----------------------------------------------------------------------------- real_next_obs of the env kernels
def _env_buffers(N, A, F, K):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    return dict(obs=z(N, A, F), obs_step=z(N, dt=I32), mask=z(N, A, K, dt=U8), reward=z(N, A), discount=z(N, A), done=z(N, dt=U8),
                m_ret=z(N), m_len=z(N, dt=I32), m_term=z(N, dt=U8), real_obs=torch.full((N, A, F), float("nan"), device=DEV),
                real_mask=torch.full((N, A, K), 9, dtype=U8, device=DEV))


def _step_both(env, plain, b, pb, actions, use_mask):
    """Step ``env`` through the real_obs entry point and its twin ``plain`` through the plain one; every shared output must agree."""
    a = torch.from_numpy(actions).to(DEV)
    env.step(a, b["reward"], b["done"], b["obs"], b["obs_step"], b["m_ret"], b["m_len"], b["m_term"], mask=b["mask"] if use_mask else None,
             discount=b["discount"], real_obs=b["real_obs"], real_mask=b["real_mask"] if use_mask else None)
    plain.step(a, pb["reward"], pb["done"], pb["obs"], pb["obs_step"], pb["m_ret"], pb["m_len"], pb["m_term"], mask=pb["mask"] if use_mask else None,
               discount=pb["discount"])
    for k in ("reward", "discount", "done", "obs", "obs_step", "m_ret", "m_len", "m_term") + (("mask",) if use_mask else ()):
        assert torch.equal(b[k], pb[k]), k
    for f in env.state_fields:
        assert torch.equal(getattr(env, f), getattr(plain, f)), f


def test_coordsum_step_real_obs_matches_oracle(L, stream):
    from magpo_amd.envs import CoordSumConfig, CoordSumEnvBatch
    A, K, TL, maxval, N = 2, 4, 6, 7, 9
    spec, cfg = ocs.CoordSumSpec(A, K, TL, maxval), CoordSumConfig(A, K, TL, maxval)
    keys = oprng.split(oprng.prng_key(5), N)
    st, ts = ocs.reset(spec, keys)
    env, plain = CoordSumEnvBatch(cfg, N, DEV), CoordSumEnvBatch(cfg, N, DEV)
    b, pb = _env_buffers(N, A, A + 1, K), _env_buffers(N, A, A + 1, K)
    kd = torch.from_numpy(keys.view(np.int32)).to(DEV)
    env.reset(kd, b["obs"], b["obs_step"]); plain.reset(kd, pb["obs"], pb["obs_step"])
    rng = np.random.default_rng(1)
    ends = 0
    for t in range(2 * TL + 1):
        a = rng.integers(0, K, (N, A)).astype(np.int32)
        st, ts, real = ref.step_with_real_obs(ocs, spec, st, a)
        _step_both(env, plain, b, pb, a, False)
        assert np.array_equal(b["obs"].cpu().numpy(), ts["observation"]["agents_view"].astype(np.float32)), t
        assert np.array_equal(b["real_obs"].cpu().numpy(), real["agents_view"].astype(np.float32)), t
        done = ts["step_type"] == ocs.STEP_LAST
        assert np.array_equal(b["done"].cpu().numpy().astype(bool), done)
        same = torch.equal(b["real_obs"], b["obs"])
        assert same or done.any()
        ends += int(done.sum())
    assert ends >= 2 * N
    # a null real_obs through the new entry point = the plain step
    L.call("magpo_coordsum_step_real_obs", *env._args(), torch.from_numpy(a).to(DEV), A, b["reward"], b["discount"], b["done"], b["obs"], b["obs_step"],
           b["m_ret"], b["m_len"], b["m_term"], 1, None, stream)
    plain.step(torch.from_numpy(a).to(DEV), pb["reward"], pb["done"], pb["obs"], pb["obs_step"], pb["m_ret"], pb["m_len"], pb["m_term"], discount=pb["discount"])
    assert torch.equal(b["obs"], pb["obs"]) and torch.equal(env.record, plain.record) and torch.equal(env.key, plain.key)


def test_lbf_step_real_obs_matches_oracle(L, stream):
    from magpo_amd.envs import LbfConfig, LbfEnvBatch
    args = (5, 5, 2, 2, 2, False, 5)       # 5 x 5 grid, 2 agents, 2 food, time limit 5: truncations and terminations
    spec, cfg = olbf.LbfSpec(*args), LbfConfig(*args)
    N, A, K, F = 40, 2, 6, cfg.obs_dim
    keys = oprng.split(oprng.prng_key(11), N)
    st, ts = olbf.reset(spec, keys)
    env, plain = LbfEnvBatch(cfg, N, DEV), LbfEnvBatch(cfg, N, DEV)
    b, pb = _env_buffers(N, A, F, K), _env_buffers(N, A, F, K)
    kd = torch.from_numpy(keys.view(np.int32)).to(DEV)
    env.reset(kd, b["obs"], b["obs_step"], b["mask"]); plain.reset(kd, pb["obs"], pb["obs_step"], pb["mask"])
    rng = np.random.default_rng(2)
    terminated = truncated = 0
    for t in range(16):
        m = ts["observation"]["action_mask"]
        a = np.zeros((N, A), np.int32)
        for n in range(N):
            for i in range(A):
                a[n, i] = 5 if (m[n, i, 5] and rng.random() < 0.8) else rng.choice(np.nonzero(m[n, i])[0])
        st, ts, real = ref.step_with_real_obs(olbf, spec, st, a)
        _step_both(env, plain, b, pb, a, True)
        assert np.array_equal(b["obs"].cpu().numpy(), ts["observation"]["agents_view"]), t
        assert np.array_equal(b["mask"].cpu().numpy().astype(bool), ts["observation"]["action_mask"]), t
        assert np.array_equal(b["real_obs"].cpu().numpy(), real["agents_view"]), t
        assert np.array_equal(b["real_mask"].cpu().numpy().astype(bool), real["action_mask"]), t
        done = ts["step_type"] == olbf.STEP_LAST
        term = ts["discount"][:, 0] == 0
        terminated += int(term.sum()); truncated += int((done & ~term).sum())
        keep = torch.from_numpy(~done).to(DEV)
        assert torch.equal(b["real_obs"][keep], b["obs"][keep]) and torch.equal(b["real_mask"][keep], b["mask"][keep])
    assert terminated > 0 and truncated > 0, (terminated, truncated)
    with pytest.raises(ValueError):   # one of the two real outputs alone
        L.call("magpo_lbf_step_real_obs", *env._args(), torch.from_numpy(a).to(DEV), A, b["reward"], b["discount"], b["done"], b["obs"], b["obs_step"],
               b["mask"], b["m_ret"], b["m_len"], b["m_term"], 1, b["real_obs"], None, stream)
    # both null = the plain step
    L.call("magpo_lbf_step_real_obs", *env._args(), torch.from_numpy(a).to(DEV), A, b["reward"], b["discount"], b["done"], b["obs"], b["obs_step"],
           b["mask"], b["m_ret"], b["m_len"], b["m_term"], 1, None, None, stream)
    plain.step(torch.from_numpy(a).to(DEV), pb["reward"], pb["done"], pb["obs"], pb["obs_step"], pb["m_ret"], pb["m_len"], pb["m_term"], mask=pb["mask"],
               discount=pb["discount"])
    assert torch.equal(b["obs"], pb["obs"]) and torch.equal(b["mask"], pb["mask"]) and torch.equal(env.agent_pos, plain.agent_pos)


def test_other_envs_refuse_real_obs():
    from magpo_amd.envs import MpeConfig, make_env_batch
    env = make_env_batch(MpeConfig(), 2, DEV)
    with pytest.raises(NotImplementedError, match="MpeConfig"):
        env.step(None, None, None, None, None, None, None, None, real_obs=torch.zeros(1, device=DEV))
