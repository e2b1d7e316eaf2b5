"""Plain torch references of the primitive HIP kernels, one function per operation, written from the header comments of
include/magpo.h and the formulas at the top of each csrc/*.hip file.

Every function computes in the dtype of its inputs: the GPU tests call them in fp64 (the reference) and once more in fp32 (the plain
restatement whose own error against fp64 sizes the bound of sums over many rows, `sum_bound`).  Backward references are
torch.autograd on the forward; shared formulas come from oracle.networks.  The case builders (`*_case`) make the fp32 inputs both the
CPU module (tests/test_kernel_refs.py) and the GPU modules use, so the margins checked on the CPU are those of the GPU cases.
"""
import torch

from oracle import networks as onets

E = 64          # row width of the fused segment kernels
WP = 128        # padded observation width of the wide-observation kernels


# ----------------------------------------------------------------------------- tolerances
def local_bound(ref, rtol=2e-5, atol=2e-6):
    """Token-local outputs: the bound of close() in tests/test_kernels_gpu.py."""
    return atol + rtol * ref.detach().abs().max().item()


def max_err(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def sum_bound(ref64, ref32):
    """Sums over R rows: max(the project's 1e-4 / 1e-5 bound, 4 x the error of the same sum in plain fp32 torch)."""
    return max(local_bound(ref64, 1e-4, 1e-5), 4.0 * max_err(ref32, ref64))


def to(dtype, *ts):
    return tuple(None if t is None else (t.to(dtype) if t.is_floating_point() else t) for t in ts)


def clamp_pos(pos, npos):
    return pos.long().clamp(0, npos - 1)


# ----------------------------------------------------------------------------- fused segments (csrc/seg_fused.hip)
def seg_front(r, gp, gamma, beta, wo, res, s1, s2, pe, pos, rows=None):
    """u = swish(g) * GroupNorm(r) ; y = u W_o ; o = rms(res + y) s1 [-> rms s2] ; ope = o + pe[clamp(pos)].  With `rows`, gp and res
    are row tables and token row i reads table row rows[i]."""
    if rows is not None:
        gp, res = gp[rows.long()], res[rows.long()]
    u = onets.swish(gp) * onets.groupnorm_rows(r, gamma, beta, 1)
    y = u @ wo
    o = onets.rmsnorm(res + y, s1)
    if s2 is not None:
        o = onets.rmsnorm(o, s2)
    ope = o + pe[clamp_pos(pos, pe.shape[0])]
    return u, y, o, ope


def seg_post(tail, c, dtype=torch.float64):
    """All outputs of magpo_seg_post for the case dict `c` (seg_case): u y o ope + the tail's."""
    g = lambda n: None if c.get(n) is None else (c[n].to(dtype) if c[n].is_floating_point() else c[n])
    u, y, o, ope = seg_front(g("r"), g("gp"), g("gamma"), g("beta"), g("wo"), g("res"), g("s1"), g("s2"), g("pe"), c["pos"], c.get("rows"))
    out = dict(u=u, y=y, o=o, ope=ope)
    if tail == 1:
        p = {"enc.head.dense0.kernel": g("w0"), "enc.head.dense0.bias": g("b0"), "enc.head.norm.scale": g("hs"),
             "enc.head.dense1.kernel": g("hw")[:, None], "enc.head.dense1.bias": g("hb1")}
        out["out0"] = o @ p["enc.head.dense0.kernel"] + p["enc.head.dense0.bias"]
        out["value"] = onets._value_head(p, o)[:, 0]
        for k, wq in enumerate(c["q2w"]):
            out[f"q2_{k}"] = ope @ wq.to(dtype)
    elif tail == 2:
        out["out0"] = ope @ g("w0")
    elif tail == 3:
        p = {"dec.head.dense0.kernel": g("w0"), "dec.head.dense0.bias": g("b0"), "dec.head.norm.scale": g("hs"),
             "dec.head.dense1.kernel": g("w1"), "dec.head.dense1.bias": g("b1")}
        out["out0"] = o @ p["dec.head.dense0.kernel"] + p["dec.head.dense0.bias"]
        out["hn"] = onets.rmsnorm(onets.gelu(out["out0"]), p["dec.head.norm.scale"])
        lg = onets._logit_head(p, o)
        out["logits"] = torch.cat([lg, torch.zeros(lg.shape[0], E - lg.shape[1], dtype=dtype)], dim=1)   # 64-wide rows, zero beyond K
    return out


def seg_case(R, seed, tail=0, K=20, nq2=0, s2=True, rows=False, npos=101, pe=None):
    """fp32 inputs of one seg_post / seg_bwd case.  Parameters of order 1, scales near 1.  With rows: gp / res are tables of C < R rows."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    C = max(1, min(R - 1, 37)) if rows else R
    c = dict(r=rn(R, E), gp=rn(C, E), res=rn(C, E), gamma=1 + 0.1 * rn(E), beta=0.1 * rn(E), wo=rn(E, E) / 8, s1=1 + 0.1 * rn(E),
             s2=(1 + 0.1 * rn(E)) if s2 else None)
    # positions: mostly in range, some below 0 and some >= npos (the kernels clamp)
    c["pos"] = torch.randint(-3, npos + 3, (R,), generator=g, dtype=torch.int32)
    c["rows"] = torch.randint(0, C, (R,), generator=g, dtype=torch.int32) if rows else None
    c["pe"] = pe if pe is not None else onets.positional_encoding(torch.arange(npos), E, torch.float32)
    if tail in (1, 3):
        c.update(w0=rn(E, E) / 8, b0=0.1 * rn(E), hs=1 + 0.1 * rn(E))
    if tail == 1:
        c.update(hw=rn(E) / 8, hb1=rn(1), q2w=[rn(E, E) / 8 for _ in range(nq2)])
    if tail == 2:
        c.update(w0=rn(E, 3 * E) / 8)
    if tail == 3:
        c.update(w1=rn(E, K) / 8, b1=0.1 * rn(K))
    # incoming gradients of the backward
    c.update(d0=rn(R, E), d1=rn(R, E), d2=rn(R, E))
    return c


def seg_bwd(c, dtype=torch.float64, use_d1=True, use_d2=True, presum=False):
    """Backward of the front by autograd: loss = sum(o * (d0 + d1 + d2)).  Returns dsum = d loss / d (res + y), dr, dgp (per token row)
    and the parameter gradients ds1, ds2, dgamma, dbeta.  presum: `res` already holds res + y (the kernel is given neither y nor W_o^T),
    the gradient still flows through y = u W_o into r and gp."""
    g = lambda n: None if c.get(n) is None else c[n].detach().to(dtype).clone()   # fresh leaves: the case's own tensors stay untouched
    r, gp_t, res_t = g("r").requires_grad_(True), g("gp"), g("res")
    gamma, beta, s1 = g("gamma").requires_grad_(True), g("beta").requires_grad_(True), g("s1").requires_grad_(True)
    s2 = None if c.get("s2") is None else g("s2").requires_grad_(True)
    rows = c.get("rows")
    gp = (gp_t[rows.long()] if rows is not None else gp_t).clone().requires_grad_(True)
    res = (res_t[rows.long()] if rows is not None else res_t).clone().requires_grad_(True)
    u = onets.swish(gp) * onets.groupnorm_rows(r, gamma, beta, 1)
    y = u @ g("wo")
    x = res + ((y - y.detach()) if presum else y)
    o = onets.rmsnorm(x, s1)
    if s2 is not None:
        o = onets.rmsnorm(o, s2)
    d = g("d0") + (g("d1") if use_d1 else 0) + (g("d2") if use_d2 else 0)
    (o * d).sum().backward()
    return dict(dsum=res.grad, dr=r.grad, dgp=gp.grad, ds1=s1.grad, ds2=None if s2 is None else s2.grad, dgamma=gamma.grad, dbeta=beta.grad)


# ----------------------------------------------------------------------------- recurrent retention (csrc/retention.hip)
def retention_recurrent(S, q, k, v, decay, ret_from, gp=None, gamma=None, beta=None, gs=None):
    """S [N, hs, hs], q / k / v (/ gp) [N, ntok, hs]:  S' = decay S + sum_b k_b^T v_b over all ntok tokens of the call,
    r_a = q_a S' for ret_from <= a < ntok; epilogue (gp given): swish(gp) * GroupNorm(r) over groups of gs channels.
    Returns (S', r [N, ntok - ret_from, hs])."""
    Sn = decay * S + k.transpose(1, 2) @ v
    r = q[:, ret_from:] @ Sn
    if gp is not None:
        hs = q.shape[-1]
        r = onets.swish(gp[:, ret_from:]) * onets.groupnorm_rows(r.reshape(-1, hs), gamma, beta, hs // gs).reshape(r.shape)
    return Sn, r


def retention_case(nenv, ntok, hs, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(S=rn(nenv, 64, 64), q=rn(nenv, ntok, hs), k=rn(nenv, ntok, hs), v=rn(nenv, ntok, hs), gp=rn(nenv, ntok, hs),
                gamma=1 + 0.1 * rn(hs), beta=0.1 * rn(hs))


def retention_padded_state(c, decay, hs, dtype=torch.float64):
    """The 64 x 64 state tile after a write: the hs x hs corner follows the recurrence, the padding only decays (k, v are zero there)."""
    S = c["S"].to(dtype)
    Sn = decay * S
    Sn[:, :hs, :hs] = retention_recurrent(S[:, :hs, :hs], c["q"].to(dtype), c["k"].to(dtype), c["v"].to(dtype), decay, 0)[0]
    return Sn


# ----------------------------------------------------------------------------- prologue-fused dense layer (csrc/linear.hip: k_linear_pro)
def linear_pro(pro, c, use_pe, dtype=torch.float64):
    """row = pro 1: rms(gelu(W_act[idx])) s1; 2: rms(gelu(rms_F(obs) s_obs @ W_obs)) s1; 3: rms(a + y) s1 [-> rms s2]; 4: rms(gelu(a)) s1.
    outpe = row + pe[clamp(pos)];  Y = (use_pe ? outpe : row) @ Wd + bias.  Returns (row, outpe, Y)."""
    g = lambda n: None if c.get(n) is None else c[n].to(dtype)
    if pro == 1:
        row = onets.rmsnorm(onets.gelu(g("W")[c["idx"].long()]), g("s1"))
    elif pro == 2:
        p = {"enc.obs.norm.scale": g("s_obs"), "enc.obs.dense.kernel": g("W")}
        row = onets.rmsnorm(onets._obs_encoder(p, g("a")[:, :c["F"]]), g("s1"))
    elif pro == 3:
        row = onets.rmsnorm(g("a") + g("y") if c.get("y") is not None else g("a"), g("s1"))
        if c.get("s2") is not None:
            row = onets.rmsnorm(row, g("s2"))
    else:
        row = onets.rmsnorm(onets.gelu(g("a")), g("s1"))
    outpe = row + g("pe")[clamp_pos(c["pos"], c["pe"].shape[0])]
    return row, outpe, (outpe if use_pe else row) @ g("Wd") + g("bias")


def linear_pro_case(pro, R, NOUT, seed, npos=101, pe=None, K=20, F=5, ldo=8, s2=True, y=True):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = dict(s1=1 + 0.1 * rn(E), Wd=rn(E, NOUT) / 8, bias=0.1 * rn(NOUT), F=F,
             pos=torch.randint(-3, npos + 3, (R,), generator=g, dtype=torch.int32),
             pe=pe if pe is not None else onets.positional_encoding(torch.arange(npos), E, torch.float32))
    if pro == 1:
        c.update(W=rn(K + 1, E) * 0.5, idx=torch.randint(0, K + 1, (R,), generator=g, dtype=torch.int32))
    elif pro == 2:
        obs = torch.full((R, ldo), 1e30)             # the floats behind the F features are not the kernel's to read
        obs[:, :F] = torch.randint(0, 60, (R, F), generator=g).float()
        c.update(a=obs, s_obs=1 + 0.1 * rn(F), W=rn(F, E) * 0.5)
    elif pro == 3:
        c.update(a=rn(R, E), y=rn(R, E) if y else None, s2=(1 + 0.1 * rn(E)) if s2 else None)
    else:
        c.update(a=rn(R, E))
    return c


# ----------------------------------------------------------------------------- wide observations (csrc/wideobs.hip)
def obsnorm_fwd(obs, F, s_obs):
    """on [R, 128] = RMSNorm over the first F features * s_obs, columns F..127 zero."""
    on = torch.zeros(obs.shape[0], WP, dtype=obs.dtype)
    on[:, :F] = onets.rmsnorm(obs[:, :F], s_obs)
    return on


def obsnorm_bwd(obs, F, s_obs, don):
    """gradient of s_obs for the incoming gradient don [R, 128] (autograd of obsnorm_fwd)."""
    s = s_obs.detach().clone().requires_grad_(True)
    (obsnorm_fwd(obs, F, s) * don).sum().backward()
    return s.grad


def obsnorm_case(R, F, ldo, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.full((R, ldo), 3e18)                 # garbage behind the F features: must not influence anything
    obs[:, :F] = torch.randn(R, F, generator=g)
    return dict(obs=obs, s_obs=1 + 0.1 * torch.randn(F, generator=g), don=torch.randn(R, WP, generator=g))


def add_pe(x, pe, pos):
    return x + pe[clamp_pos(pos, pe.shape[0])]


# ----------------------------------------------------------------------------- small first layers (csrc/rowops.hip)
def small_relu_wgrad(X, F, Yact, dY):
    """dW [F, 128] = X^T (dY * [Yact > 0]), db [128] = column sums of dY * [Yact > 0]."""
    gm = dY * (Yact > 0).to(dY.dtype)
    return X[:, :F].T @ gm, gm.sum(0)


def small_relu_wgrad_case(R, F, ldx, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.full((R, ldx), 1e30)
    X[:, :F] = torch.randn(R, F, generator=g)
    return dict(X=X, Yact=torch.relu(torch.randn(R, 128, generator=g)), dY=torch.randn(R, 128, generator=g))


def small_operand(mode, obs, F, s_obs=None, idx=None):
    """[R, 64] left operand of the small weight-gradient GEMMs: 0 = rms_F(obs) * s_obs, 1 = one-hot(idx), 2 = raw obs; zero beyond F."""
    R = obs.shape[0] if obs is not None else idx.shape[0]
    out = torch.zeros(R, 64, dtype=obs.dtype if obs is not None else torch.float32)
    if mode == 0:
        out[:, :F] = onets.rmsnorm(obs[:, :F], s_obs)
    elif mode == 1:
        out = torch.nn.functional.one_hot(idx.long(), 64).to(out.dtype)
    else:
        out[:, :F] = obs[:, :F]
    return out


# ----------------------------------------------------------------------------- CoordSum input classes (csrc/coordsum.hip)
def coordsum_classes(obs, prev, pos, A, maxval, npos):
    """cls_enc = ((agent * maxval + target) * npos + pos), cls_dec = prev * npos + pos; obs rows [one-hot agent id | target]."""
    agent = obs[:, :A].argmax(dim=1)
    target = obs[:, A].long().clamp(0, maxval - 1)
    p = clamp_pos(pos, npos) if pos is not None else torch.zeros_like(agent)
    enc = (agent * maxval + target) * npos + p
    dec = None if prev is None else prev.long() * npos + p
    return enc, dec


def coordsum_class_rows(A, maxval, npos, K):
    """The distinct rows in class order: obs_tab [A maxval npos][A + 1], pos_enc, prev_dec / pos_dec [(K + 1) npos]."""
    ce = torch.arange(A * maxval * npos)
    obs_tab = torch.zeros(ce.numel(), A + 1)
    obs_tab[ce, ce // npos // maxval] = 1.0
    obs_tab[:, A] = ((ce // npos) % maxval).float()
    cd = torch.arange((K + 1) * npos)
    return obs_tab, ce % npos, cd // npos, cd % npos


def coordsum_case(A, K, maxval, N, npos, seed):
    """Wrapped CoordSum tokens from the oracle env: obs rows [N * A][A + 1] (dense), plus previous actions and positions per row;
    positions include values below 0 and >= npos."""
    import numpy as np

    from oracle import coordsum as ocs
    from oracle import prng as oprng
    spec = ocs.CoordSumSpec(A, K, 100, maxval)
    state, ts = ocs.reset(spec, oprng.split(oprng.prng_key(seed), N))
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 101, (N,), generator=g).numpy()
    view = ocs.make_obs(spec, state["target"][np.arange(N), t], t.astype(np.int32))["agents_view"]
    obs = torch.from_numpy(view.reshape(N * A, A + 1).astype(np.float32))
    prev = torch.randint(0, K + 1, (N * A,), generator=g, dtype=torch.int32)
    pos = torch.randint(-2, npos + 2, (N * A,), generator=g, dtype=torch.int32)
    return obs, prev, pos
