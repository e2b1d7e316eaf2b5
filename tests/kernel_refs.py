"""Plain torch references of the primitive HIP kernels, one function per operation, written from the header comments of
include/magpo.h and the formulas at the top of each csrc/*.hip file.

Every function computes in the dtype of its inputs: the GPU tests call them in fp64 (the reference) and once more in fp32 (the plain
restatement whose own error against fp64 sizes the bound of sums over many rows, `sum_bound`).  Backward references are
torch.autograd on the forward; shared formulas come from oracle.networks.  The case builders (`*_case`) make the fp32 inputs both the
CPU module (tests/test_kernel_refs.py) and the GPU modules use, so the margins checked on the CPU are those of the GPU cases.
"""
import math

import torch

from oracle import learner as olearn
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


# ----------------------------------------------------------------------------- RL-side kernels (csrc/rl.hip, csrc/optim.hip)
SYSC = olearn.SystemCfg()       # clip_eps 0.2, clip_gpo 1.5, ent_coef 0.01, vf_coef 0.5, alpha 1: what the learner passes
KINK = 1e-5                     # a row closer than this to a kink of a clipped surrogate (fp64 reference) may take the other branch in fp32
ILLEGAL = 1e4                   # logit of every illegal action in the inputs: a kernel that forgets the mask fails loudly
LOSS_NAMES = ("total", "value_loss", "actor_loss", "guider_loss", "kl_loss", "entropy", "actor_kl", "total_guider", "total_actor")
LOSS_KL_SLACK = (0, 4, 7)       # the scalars that contain kl_loss = mean(kl * [|d| > log clip_gpo]), discontinuous at that kink
GRID_STRIDE_R = 16 * 1024 * 2 + 5   # k_magpo_loss: 1024 blocks of 16 rows, two full grid-stride passes and a ragged third


def ceil4(k):
    return (k + 3) // 4 * 4


def loss_strides(kind, K):
    """(ldg, lda, lddg, lddda): s64 is the learner's; tight: logits rows of exactly K floats, gradient rows of ceil4(K) (the entry point
    wants gradient strides in multiples of 4); mixed: the vector loads off, one gradient row wide; s72: vector loads on odd strides."""
    return {"s64": (64, 64, 64, 64), "s32": (32, 32, 32, 32), "tight": (K, K, ceil4(K), ceil4(K)), "mixed": (64, 32, 32, 64),
            "s72": (72, 68, 68, 72)}[kind]


LOSS_DISTS = {"base": {}, "peaked": dict(scale=30.0, spread=1.0), "off+30": dict(offset=30.0), "off-30": dict(offset=-30.0),
              "constadv": dict(const_adv=True)}
LOSS_MASKS = {"nomask": {}, "mask": dict(mask_p=0.6), "single": dict(mask_p=0.6, one_legal=0.15)}


def loss_case(R, K, seed, scale=0.7, spread=0.6, offset=0.0, mask_p=None, one_legal=0.0, const_adv=False):
    """fp32 inputs of one magpo_loss_fwd_bwd case.  Guider logits N(offset, scale), actor logits = guider + N(0, spread); value within
    0.3 of the old value (clip_eps 0.2: both value branches); old log-prob = the fp64 guider log-prob + N(0, 0.1), stored as fp32 so every
    dtype and the kernel read the same number.  mask_p: keep probability of the action mask (one random action always legal), one_legal:
    fraction of rows with exactly one legal action; illegal logits are ILLEGAL in both tensors.  const_adv: all advantages 0.75 (sums of
    it are exact in fp32 and fp64, so the mean is exact, the std 0 and the normalised advantage exactly 0 in every dtype)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    gl = rn(R, K) * scale + offset
    al = gl + rn(R, K) * spread
    legal = torch.ones(R, K, dtype=torch.bool)
    if mask_p is not None:
        legal = torch.rand(R, K, generator=g) < mask_p
        keep = torch.randint(0, K, (R,), generator=g)
        legal[torch.arange(R), keep] = True
        single = torch.rand(R, generator=g) < one_legal
        legal[single] = False
        legal[single, keep[single]] = True
        gl = torch.where(legal, gl, torch.full_like(gl, ILLEGAL))
        al = torch.where(legal, al, torch.full_like(al, ILLEGAL))
    action = torch.multinomial(legal.float(), 1, generator=g)[:, 0]
    vold, dvn, tgt, adv = (rn(R) for _ in range(4))
    value = vold + 0.3 * dvn
    if const_adv:
        adv = torch.full((R,), 0.75)
    noise = 0.1 * rn(R)
    g_logp = onets.masked_log_softmax(gl.double(), legal).gather(1, action[:, None])[:, 0]
    return dict(R=R, K=K, gl=gl, al=al, legal=legal, masked=mask_p is not None, action=action, value=value, vold=vold, tgt=tgt, adv=adv,
                old=(g_logp + noise.double()).float())


def loss_ref(c, dtype=torch.float64):
    """oracle.learner.guider_loss / actor_loss on the case, gradients by autograd.  Returns loss [9] in the order of k_loss_final
    (LOSS_NAMES), the gradients dg / da [R, K] and dv [R], and per row: d = g_logp - a_logp, cr (the guider's clipped-difference ratio
    before the eps clip), ra (the actor's ratio), vd = value - old value, kl (guider || actor) and A_ (the normalised advantage)."""
    gl, al, v = (c[n].to(dtype).requires_grad_(True) for n in ("gl", "al", "value"))
    legal, action = c["legal"], c["action"]
    glp, alp = onets.masked_log_softmax(gl, legal), onets.masked_log_softmax(al, legal)
    g_logp, a_logp = glp.gather(1, action[:, None])[:, 0], alp.gather(1, action[:, None])[:, 0]
    pr = glp.exp()
    ent = -torch.where(pr == 0, torch.zeros_like(pr), pr * glp).sum(-1)
    mb = dict(log_prob=c["old"].to(dtype), adv=c["adv"].to(dtype), value=c["vold"].to(dtype), targets=c["tgt"].to(dtype))
    tg, gi = olearn.guider_loss(SYSC, v, g_logp, ent, glp, alp, a_logp, mb)
    ta, ai = olearn.actor_loss(SYSC, glp, alp, a_logp, mb)
    dg, dv = torch.autograd.grad(tg, [gl, v], retain_graph=True)
    (da,) = torch.autograd.grad(ta, [al])
    loss = torch.stack([tg + ta, gi["value_loss"], ai["actor_loss"], gi["guider_loss"], gi["kl_loss"], gi["entropy"], ai["actor_kl"], tg, ta]).detach()
    with torch.no_grad():
        ld = math.log(SYSC.clip_gpo)
        d = g_logp - a_logp
        adv = mb["adv"]
        out = dict(loss=loss, dg=dg, da=da, dv=dv, d=d, cr=torch.exp(d.clamp(-ld, ld) + a_logp - mb["log_prob"]), ra=torch.exp(a_logp - mb["log_prob"]),
                   vd=v - mb["value"], kl=olearn._kl(glp, alp), A_=(adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8),
                   ratio=torch.exp(g_logp - mb["log_prob"]), g_logp=g_logp, a_logp=a_logp, ent=ent)
    return {k: t.detach() for k, t in out.items()}


def loss_near_kink(ref, m=KINK):
    """Rows [R] (of the fp64 reference) within m of a kink of a clipped surrogate: | |d| - log clip_gpo |, | cr - (1 +- eps) |,
    | ra - (1 +- eps) |, | |v - v_old| - eps |."""
    ld, eps = math.log(SYSC.clip_gpo), SYSC.clip_eps
    near = (ref["d"].abs() - ld).abs() < m
    for r in (ref["cr"], ref["ra"]):
        near |= ((r - (1 - eps)).abs() < m) | ((r - (1 + eps)).abs() < m)
    return near | ((ref["vd"].abs() - eps).abs() < m)


def loss_crossings(ref, c, m=KINK):
    """Rows where two branches with DIFFERENT gradients cross away from the kinks above: the guider's min(l1, l2) with a clipped l2 and
    ratio = the clipped value, and the value loss's max(e1, e2) with a clipped value and the target midway.  Not excluded from anything:
    the cases are chosen to have none (asserted on the CPU)."""
    ld, eps = math.log(SYSC.clip_gpo), SYSC.clip_eps
    crc = ref["cr"].clamp(1 - eps, 1 + eps)
    l2_clipped = (ref["d"].abs() > ld) | (ref["cr"] < 1 - eps) | (ref["cr"] > 1 + eps)
    cross_pg = l2_clipped & ((ref["ratio"] - crc).abs() < m) & (ref["A_"] != 0)
    v, vo, tgt = c["value"].double(), c["vold"].double(), c["tgt"].double()
    vcl = vo + (v - vo).clamp(-eps, eps)
    cross_v = ((v - vo).abs() > eps) & (((v - tgt) ** 2 - (vcl - tgt) ** 2).abs() < m)
    return (cross_pg | cross_v) & ~loss_near_kink(ref, m)


def loss_populations(ref):
    """Row counts of every branch of the three clipped surrogates, split by the sign of the advantage where it selects the gradient."""
    ld, eps = math.log(SYSC.clip_gpo), SYSC.clip_eps
    pos, neg = ref["A_"] > 0, ref["A_"] < 0
    pops = {"d_lo": ref["d"] < -ld, "d_hi": ref["d"] > ld, "v_clipped": ref["vd"].abs() > eps, "v_unclipped": ref["vd"].abs() < eps}
    for n, r in (("cr", ref["cr"]), ("ra", ref["ra"])):
        for side, sel in (("lo", r < 1 - eps), ("hi", r > 1 + eps)):
            pops[f"{n}_{side}_A+"], pops[f"{n}_{side}_A-"] = sel & pos, sel & neg
    return {k: int(v.sum()) for k, v in pops.items()}


def loss_scalar_bound(ref64, i):
    """The bound of today's test on a loss scalar: 2e-5 relative + 1e-6."""
    return 1e-6 + 2e-5 * abs(ref64["loss"][i].item())


def loss_grad_bound(ref64, name, rows):
    """The bound of today's test on a gradient: 2e-4 of the largest reference entry + 1e-9 (over the compared rows)."""
    return 1e-9 + 2e-4 * (ref64[name][rows].abs().max().item() if bool(rows.any()) else 0.0)


def _loss_matrix():
    """The case matrix of magpo_loss_fwd_bwd: a pairwise cover of strides x K x R x mask x distribution, chosen greedily and
    deterministically: among all valid combinations (K <= every stride) in lexicographic order, repeatedly the one that covers the most
    value pairs not yet covered, first one on ties, until every valid pair of values of two different dimensions appears in a case.  The
    peaked and offset distributions run with R >= 1500 only: they put logits of magnitude 30 to 100 into fp32 (ulp 2e-6 to 8e-6), and with
    a handful of rows the largest gradient entry of a peaked row is the residue of a cancellation (p (log p + entropy) at p ~ 1, 1e-5 and
    below), so the relative bounds have nothing to hold on to: the plain fp32 restatement misses them there by itself.  Then
    the two grid-stride cases (production strides, K = 20 and K = 64) and the production shape for every distribution and mask."""
    import itertools
    dims = [("s64", "s32", "tight", "mixed", "s72"), (1, 2, 5, 6, 20, 31, 32, 33, 63, 64), (1, 3, 15, 16, 17, 1500),
            tuple(LOSS_MASKS), tuple(LOSS_DISTS)]
    valid = lambda c: c[1] <= min(loss_strides(c[0], c[1])) and (c[2] >= 1500 or c[4] in ("base", "constadv"))
    combos = [c for c in itertools.product(*dims) if valid(c)]
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(5) for j in range(i + 1, 5)}
    todo = set().union(*(pairs(c) for c in combos))
    chosen = []
    while todo:
        best = max(combos, key=lambda c: len(pairs(c) & todo))    # max() keeps the first of equals
        chosen.append(best)
        todo -= pairs(best)
    chosen += [("s64", K, GRID_STRIDE_R, m, "base") for K, m in ((20, "single"), (64, "nomask"))]
    chosen += [("s64", 20, 1500, m, d) for d in LOSS_DISTS for m in LOSS_MASKS if ("s64", 20, 1500, m, d) not in chosen]
    return chosen


# seeds: 1000 + index in the matrix; a case whose fp64 reference has a row near a kink (R < 1000) or more than 0.1 % such rows, or a
# crossing row (loss_crossings), gets the next seed that has none: listed here, asserted in tests/test_kernel_refs.py
LOSS_SEED_BUMP = {14: 2, 15: 1, 24: 1, 43: 1, 53: 1, 61: 1, 74: 1, 80: 1, 82: 22, 83: 10, 84: 1, 86: 1, 93: 1, 96: 2}
LOSS_MATRIX = _loss_matrix()


def loss_case_id(i):
    s, K, R, m, d = LOSS_MATRIX[i]
    return f"{i}-{s}-K{K}-R{R}-{m}-{d}"


_loss_cache = {}


def loss_matrix_case(i):
    """(case, fp64 reference, fp32 restatement) of matrix entry i, computed once per process."""
    if i not in _loss_cache:
        s, K, R, m, d = LOSS_MATRIX[i]
        c = loss_case(R, K, 1000 + i + LOSS_SEED_BUMP.get(i, 0), **LOSS_MASKS[m], **LOSS_DISTS[d])
        c.update(strides=loss_strides(s, K), dist=d, name=loss_case_id(i))
        if R > 1500:
            return c, loss_ref(c), loss_ref(c, torch.float32)     # big cases are not kept
        _loss_cache[i] = (c, loss_ref(c), loss_ref(c, torch.float32))
    return _loss_cache[i]


# ---- categorical sampling (k_sample)
def sample_case(N, K, ld, seed, mask=None, A=1):
    """Logits [N, ld] with 1e30 behind the K valid columns; mask kinds as LOSS_MASKS, laid out [N][A][K] as the learner's (each agent its own
    random mask; the sampled agent is A - 1), illegal logits ILLEGAL."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.full((N, ld), 1e30)
    logits[:, :K] = torch.randn(N, K, generator=g) * 2
    legal = None
    if mask is not None:
        kw = LOSS_MASKS[mask]
        legal = torch.rand(N, A, K, generator=g) < kw["mask_p"]
        keep = torch.randint(0, K, (N, A), generator=g)
        legal.scatter_(2, keep[..., None], True)
        single = torch.rand(N, A, generator=g) < kw.get("one_legal", 0.0)
        legal[single] = False
        legal.scatter_(2, keep[..., None], True)
        logits[:, :K] = torch.where(legal[:, A - 1], logits[:, :K], torch.full((N, K), ILLEGAL))
    return dict(N=N, K=K, ld=ld, A=A, logits=logits, legal=legal)


def sample_lp_ref(c, dtype=torch.float64):
    x = c["logits"][:, :c["K"]].to(dtype)
    legal = torch.ones_like(x, dtype=torch.bool) if c["legal"] is None else c["legal"][:, c["A"] - 1]
    return onets.masked_log_softmax(x, legal), legal


# ---- GAE (k_gae, k_gae_scan)
GAE_DONE = ("never", "always", "last_step", "last_done", "random")
GAE_COEF = ((0.99, 0.95), (1.0, 1.0), (0.99, 0.0), (0.0, 0.95))


def gae_case(T, N, A, seed, done="random"):
    g = torch.Generator().manual_seed(seed)
    c = dict(T=T, N=N, A=A, reward=torch.randn(T, N, A, generator=g), value=torch.randn(T, N, A, generator=g), last_val=torch.randn(N, A, generator=g))
    d, ld = torch.rand(T, N, generator=g) < 0.1, torch.rand(N, generator=g) < 0.3
    if done != "random":
        d, ld = torch.zeros_like(d), torch.zeros_like(ld)
    if done == "always":
        d[:], ld[:] = True, True
    elif done == "last_step":
        d[T - 1] = True
    elif done == "last_done":
        ld[:] = True
    c.update(done=d, last_done=ld)
    return c


def gae_ref(c, gamma, lam, dtype=torch.float64):
    T, N, A = c["T"], c["N"], c["A"]
    return olearn.calculate_gae(c["reward"].to(dtype), c["value"].to(dtype), c["done"][:, :, None].expand(T, N, A), c["last_val"].to(dtype),
                                c["last_done"][:, None].expand(N, A), gamma, lam)


def gae_bound(ref64, ref32):
    """Today's bound (1e-5 relative + 1e-5), or 4 x the serial fp32 restatement's own error where that is larger."""
    return max(local_bound(ref64, 1e-5, 1e-5), 4.0 * max_err(ref32, ref64))


def gae_matrix():
    """(T, N, A, coefficient index, done pattern): every T with 1, 7 and 21 = 7 x 3 sequences, every sequence count around the dispatch
    boundary 8192 with a few small T on both sides of T = 16; coefficients and done patterns rotate with the case number (4 and 5 are
    coprime: all 20 combinations appear), plus the worst case for rounding (T = 200, gamma = lambda = 1, never done) by name."""
    shapes = [(T, N, A) for T in (1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 200) for N, A in ((1, 1), (7, 1), (7, 3), (5, 8))]
    shapes += [(T, N, A) for N, A in ((8191, 1), (1024, 8), (2731, 3)) for T in (1, 15, 16, 17, 65)]
    cases = [(T, N, A, i % 4, GAE_DONE[i % 5]) for i, (T, N, A) in enumerate(shapes)]
    return cases + [(200, 7, 3, 1, "never"), (129, 1, 1, 1, "never"), (64, 7, 1, 1, "last_done"), (16, 8191, 1, 1, "never")]


# ---- advantage moments (k_moments_partial / k_moments_final)
def adv_moments_ref(x):
    """[mean, 1 / (std + 1e-8)], population std, in the dtype of x."""
    return x.mean(), 1 / (x.std(unbiased=False) + 1e-8)


def adv_moments_input(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g)
    return {"normal": z, "100+-0.1": 100 + 0.1 * z, "zeros": torch.zeros(n), "const1.3": torch.full((n,), 1.3), "1000+-1e-3": 1000 + 1e-3 * z}[kind]


# ---- minibatch gather (k_gather_minibatch)
def gather_case(T, N, A, F, K, mb, seed, masked=True):
    """Every float field is drawn separately and offset by its own constant (value 10.., logp 20.., adv 30.., targets 40..), so a kernel that
    swaps two of them cannot pass."""
    g = torch.Generator().manual_seed(seed)
    c = dict(T=T, N=N, A=A, F=F, K=K, mb=mb, obs=torch.randn(T, N, A, F, generator=g), action=torch.randint(0, K, (T, N, A), generator=g, dtype=torch.int32),
             stepcount=torch.randint(0, 100, (T, N), generator=g, dtype=torch.int32), done=(torch.rand(T, N, generator=g) < 0.3).to(torch.uint8),
             mask=(torch.rand(T, N, A, K, generator=g) < 0.6).to(torch.uint8) if masked else None)
    for i, n in enumerate(("value", "logp", "adv", "targets")):
        c[n] = 10.0 * (i + 1) + torch.randn(T, N, A, generator=g)
    perm = torch.randperm(N, generator=g).int()
    start = (N - mb) // 2
    c.update(env_idx=perm[start:start + mb].contiguous(), agent_perm=torch.randperm(A, generator=g).int())
    return c


def gather_ref(c):
    """rec_magpo.py:441-462 on the selected envs: take envs, take agents, time-major -> env-major, rows (j, t, a')."""
    T, A, mb, K = c["T"], c["A"], c["mb"], c["K"]
    e, ap = c["env_idx"].long(), c["agent_perm"].long()

    def prep(x):
        x = x.index_select(1, e).index_select(2, ap).transpose(0, 1)
        return x.reshape(mb * T * A, *x.shape[3:])
    out = {n: prep(c[n]) for n in ("obs", "action", "value", "logp", "adv", "targets")}
    if c["mask"] is not None:
        out["mask"] = prep(c["mask"])
    out["prev"] = onets.shifted_actions(out["action"].reshape(mb, T * A), K, A, torch.float32).argmax(-1).int().reshape(-1)
    out["pos"] = c["stepcount"].index_select(1, e).T[:, :, None].expand(mb, T, A).reshape(-1)
    out["done"] = c["done"].index_select(1, e).T.reshape(-1)
    out["h0idx"] = (c["env_idx"][:, None] * A + c["agent_perm"][None, :]).reshape(-1)
    return out


# ---- slab reduction (k_reduce_slabs)
def reduce_slabs_ref(slab, P, before, scale, accumulate):
    """out = (accumulate ? before : 0) + scale * sum_g slab[g, :P]: scale multiplies the slab sum, not the old value."""
    s = scale * slab[:, :P].sum(0)
    return before + s if accumulate else s


# ---- clip + Adam (csrc/optim.hip)
ADAM_MU_RTOL, ADAM_NU_RTOL = 1e-6, 2e-6     # of the largest entry: see tests/test_rl_kernels_gpu.py::test_clip_adam_five_steps


def adam_scenarios(n, seed, max_norm):
    """name -> (fp32 parameters, five fp32 gradients): far below / far above the clip threshold, a norm of max_norm (1 -+ 1e-3), and zero
    gradients in the middle and at the end of a run."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, generator=g).double()
    unit = z / z.norm()
    sc = {"small": [1e-3 * z] * 5, "large": [3.0 * z] * 5, "just-below": [unit * max_norm * (1 - 1e-3)] * 5,
          "just-above": [unit * max_norm * (1 + 1e-3)] * 5, "zero-mid": [z * 0.01, z * 0.01, z * 0, z * 0.01, z * 0]}
    return {k: (torch.randn(n, generator=g), [x.float() for x in v]) for k, v in sc.items()}
