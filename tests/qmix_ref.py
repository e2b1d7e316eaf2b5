"""CPU restatement of rec_qmix (mava/systems/q_learning/anakin/rec_qmix.py:233-533), for the tests only: the monotonic mixing network
(QMixingNetwork, networks/base.py:276-343; autograd gives the reference gradients), the team reward, the slicing of the L stored steps of a
window, the eight loss scalars, optax.adam without clipping and the learner loop.  Built on tests/iql_ref.py (acting, ring, sampler, envs) by
import; the product never imports it.

UNPINNED (restated, not compared with JAX): what tests/iql_ref.py lists, and the team reward's summation order: the agents' rewards are added
sequentially a = 0 .. A-1 in float32 and the sum divided by float32(A).
"""
import numpy as np
import torch
import torch.nn.functional as Fn

from oracle import prng
from tests import iql_ref
from tests.iql_ref import F32, FMIN

ENTRIES = ("hyper_w1/Dense_0", "hyper_w1/Dense_1", "hyper_b1/Dense_0", "hyper_w2/Dense_0", "hyper_w2/Dense_1", "hyper_b2/Dense_0", "hyper_b2/Dense_1")
LOSS_NAMES = ("q_loss", "mean_q", "max_q_error", "min_q_error", "mean_target", "mean_reward_t0", "mean_next_qval", "done")


# ----------------------------------------------------------------------------- the mixer (base.py:276-343)
def mixer_shapes(A, E, G, hyper=64):
    dims = ((G, hyper), (hyper, A * E), (G, E), (G, hyper), (hyper, E), (G, E), (E, 1))
    s = {}
    for n, (i, o) in zip(ENTRIES, dims):
        s[n + "/kernel"], s[n + "/bias"] = (i, o), (o,)
    s["layer_norm/scale"], s["layer_norm/bias"] = (G,), (G,)
    return s


def mixer_init(seed, A, E, G, bias_std=0.1):
    """float32 parameters: orthogonal(sqrt 2) kernels as the reference's, but random biases and LayerNorm scale / bias, so that every
    gradient is exercised."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for n, shp in mixer_shapes(A, E, G).items():
        if n.endswith("/kernel"):
            a = torch.randn(max(shp), min(shp), generator=g, dtype=torch.float64)
            q, r = torch.linalg.qr(a)
            q = q * torch.sign(torch.diagonal(r))[None]
            p[n] = (np.sqrt(2.0) * (q.T if shp[0] < shp[1] else q)).float().contiguous()
        elif n == "layer_norm/scale":
            p[n] = (1.0 + bias_std * torch.randn(shp, generator=g)).float()
        else:
            p[n] = (bias_std * torch.randn(shp, generator=g)).float()
    return p


def global_state(obs, id_cols):
    """observation.global_state of one team: obs [..., A, F] -> [..., A (F - id_cols)], the raw agent views side by side."""
    return obs[..., id_cols:].reshape(*obs.shape[:-2], -1)


def mixer_apply(p, q, s, E, norm=True):
    """q [..., A], s [..., G] -> q_tot [...]."""
    A = q.shape[-1]
    if norm:   # flax LayerNorm: eps 1e-6, fast variance clamped at 0
        mean = s.mean(-1, keepdim=True)
        var = torch.clamp((s * s).mean(-1, keepdim=True) - mean * mean, min=0.0)
        x = (s - mean) * torch.rsqrt(var + 1e-6) * p["layer_norm/scale"] + p["layer_norm/bias"]
    else:
        x = s
    dense = lambda n, v: v @ p[n + "/kernel"] + p[n + "/bias"]
    w1 = torch.abs(dense("hyper_w1/Dense_1", torch.relu(dense("hyper_w1/Dense_0", x)))).reshape(*q.shape[:-1], A, E)
    b1 = dense("hyper_b1/Dense_0", x)
    hidden = Fn.elu((q[..., None, :] @ w1)[..., 0, :] + b1)
    w2 = torch.abs(dense("hyper_w2/Dense_1", torch.relu(dense("hyper_w2/Dense_0", x))))
    b2 = dense("hyper_b2/Dense_1", torch.relu(dense("hyper_b2/Dense_0", x)))[..., 0]
    return (hidden * w2).sum(-1) + b2


# ----------------------------------------------------------------------------- reward, slicing, loss (rec_qmix.py:287, :377-425)
def team_reward(reward):
    """jnp.mean(reward, axis=-1) of [N, A] float32, in every agent column (UNPINNED order: sequential sum, then / A)."""
    r = np.asarray(reward, F32)
    s = np.zeros(r.shape[0], F32)
    for a in range(r.shape[1]):
        s = (s + r[:, a]).astype(F32)
    return np.repeat((s / F32(r.shape[1])).astype(F32)[:, None], r.shape[1], axis=1)


def sequence_rows(win):
    """What update_q reads of windows [B][L] (rec_qmix.py:377-395): all L obs / masks / term_or_trunc, the first L - 1 actions and rewards."""
    return dict(obs=win["obs"], mask=win["mask"], term_or_trunc=win["term_or_trunc"], action=win["action"][:, :-1], reward=win["reward"][:, :-1, 0])


def td_loss(q_tot, next_q_tot, reward, tot_full, gamma):
    """q_tot / next_q_tot / reward [B, L-1], tot_full [B, L] -> (loss, info dict of 0-d tensors, target)."""
    next_done = tot_full[:, 1:].to(q_tot.dtype)
    target = (reward + (1.0 - next_done) * gamma * next_q_tot).detach()
    err = q_tot - target
    loss = (err ** 2).mean()
    e2 = (err.abs() ** 2).detach()
    info = dict(q_loss=loss.detach(), mean_q=q_tot.mean().detach(), max_q_error=e2.max(), min_q_error=e2.min(), mean_target=target.mean(),
                mean_reward_t0=reward.mean(), mean_next_qval=next_q_tot.mean(), done=tot_full.to(q_tot.dtype).mean())
    return loss, info, target


def adam_step(params, grads, opt, lr, b1=0.9, b2=0.999, eps=1e-8):
    """optax.adam(lr) + apply_updates (rec_qmix.py:151-153, :430-433): no clipping."""
    from oracle import learner as olearn
    new_p, new_opt, _ = olearn.clip_adam_step(params, grads, opt, lr, float("inf"), b1, b2, eps)
    return new_p, new_opt


# ----------------------------------------------------------------------------- learner (rec_qmix.py:233-533)
class QmixOracleLearner(iql_ref.IqlOracleLearner):
    """rec_qmix on the CPU: rec_iql's restated rollout with the team reward stored, and QMIX's training step."""

    def __init__(self, spec, num_envs, sys, params, torsos, env, mixer_params, embed_dim, id_cols, norm=True, **kw):
        super().__init__(spec, num_envs, sys, params, torsos, env, **kw)
        dt = self.dtype
        self.E, self.id_cols, self.norm = embed_dim, id_cols, norm
        self.mixer = {k: v.clone().to(dt) for k, v in mixer_params.items()}
        self.mixer_target = {k: v.clone().to(dt) for k, v in mixer_params.items()}
        self.opt_mixer = self.olearn.adam_init(self.mixer)

    def setup(self, key):
        super().setup(key)
        for g in self.groups:
            add = g.ring.add
            g.ring.add = lambda _add=add, **step: _add(**{**step, "reward": team_reward(step["reward"])})   # rec_qmix.py:287

    def group_loss(self, online, mixer, g, env_idx, start):
        s, A, dt = self.sys, self.A, self.dtype
        win = g.ring.gather(env_idx, start, s.sample_sequence_length)
        rows = sequence_rows(win)
        tm = lambda x: torch.from_numpy(np.ascontiguousarray(np.swapaxes(x, 0, 1)))      # (B, L, ...) -> (L, B, ...)
        B = len(env_idx)
        h0 = torch.zeros(B, A, 128, dtype=dt)
        obs = tm(rows["obs"]).to(dt)                                                       # (L, B, A, F)
        resets = tm(rows["term_or_trunc"]).bool()[..., None].expand(-1, -1, A)
        with torch.no_grad():
            _, q_target = iql_ref.q_apply(self.target, h0, obs, resets, self.pre, self.post)
        _, q_all = iql_ref.q_apply(online, h0, obs, resets, self.pre, self.post)          # one unroll serves :388 and :344 (same rows, zero carry)
        mask = None if rows["mask"] is None else tm(rows["mask"])
        qn = q_all[1:].detach()
        qm = qn if mask is None else torch.where(mask[1:].bool(), qn, torch.full_like(qn, float(FMIN)))
        next_a = torch.argmax(qm, dim=-1)
        next_q = torch.gather(q_target[1:], -1, next_a[..., None])[..., 0]                # (L-1, B, A)
        q_sel = torch.gather(q_all[:-1], -1, tm(rows["action"]).long()[..., None])[..., 0]
        state = global_state(obs, self.id_cols)                                            # (L, B, G)
        with torch.no_grad():
            next_q_tot = mixer_apply(self.mixer_target, next_q, state[1:], self.E, self.norm)
        q_tot = mixer_apply(mixer, q_sel, state[:-1], self.E, self.norm)
        bt = lambda x: x.transpose(0, 1)                                                   # (L-1, B) -> (B, L-1)
        loss, info, target = td_loss(bt(q_tot), bt(next_q_tot), torch.from_numpy(rows["reward"]).to(dt), torch.from_numpy(rows["term_or_trunc"]), s.gamma)
        return loss, info, dict(q=q_all.detach(), qn_online=qn, next_mask=None if mask is None else mask[1:], rows=rows, terminal=win["terminal"], q_tot=bt(q_tot).detach(),
                                next_q_tot=bt(next_q_tot), q_sel=q_sel.detach(), next_q=next_q)

    def train(self):
        s, infos = self.sys, []
        ready = self.ready()
        for _ in range(s.epochs):
            for g in self.groups:
                ks = prng.split(g.train_key, 2)                                              # :466
                g.train_key, g.buff_key = ks[0], ks[1]
            if not ready:
                infos.append(None)
                continue
            online = {k: v.detach().clone().requires_grad_(True) for k, v in self.online.items()}
            mixer = {k: v.detach().clone().requires_grad_(True) for k, v in self.mixer.items()}
            total, info_sum, details, idxs = 0.0, None, [], []
            for g in self.groups:
                env_idx, start = g.ring.sample_indices(g.buff_key, s.sample_batch_size, s.sample_sequence_length)
                loss, info, det = self.group_loss(online, mixer, g, env_idx, start)
                total = total + loss / self.U                                                # pmean over "batch" (:429)
                info_sum = {k: v / self.U for k, v in info.items()} if info_sum is None else {k: info_sum[k] + v / self.U for k, v in info.items()}
                details.append(det); idxs.append((env_idx, start))
            leaves = list(online.values()) + list(mixer.values())
            gl = [torch.zeros_like(p) if g_ is None else g_ for p, g_ in zip(leaves, torch.autograd.grad(total, leaves, allow_unused=True))]
            grads, mgrads = dict(zip(online, gl[:len(online)])), dict(zip(mixer, gl[len(online):]))
            self.online, self.opt = adam_step(self.online, grads, self.opt, s.q_lr)
            self.mixer, self.opt_mixer = adam_step(self.mixer, mgrads, self.opt_mixer, s.q_lr)
            with torch.no_grad():
                for src, name in ((self.online, "target"), (self.mixer, "mixer_target")):
                    tgt = getattr(self, name)
                    if s.hard_update:                                                        # :436-449, t_train before its increment
                        if self.t_train % s.update_period == 0:
                            setattr(self, name, {k: v.clone() for k, v in src.items()})
                    elif self.dtype == torch.float32:
                        setattr(self, name, {k: torch.from_numpy(iql_ref.target_update(src[k].numpy(), tgt[k].numpy(), 0, s.tau, 0, 1)) for k in src})
                    else:
                        setattr(self, name, {k: s.tau * src[k] + (1.0 - s.tau) * tgt[k] for k in src})
            self.t_train += 1
            info = {k: float(v) for k, v in info_sum.items()}
            infos.append(info)
            self.train_log.append(dict(idx=idxs, info=info, grads=grads, mixer_grads=mgrads, details=details))
        return infos


# ----------------------------------------------------------------------------- the parity cases of tests/test_qmix_learner_gpu.py
# iql_ref.PARITY_CASES' two envs; 4 envs, rollout_length 2, epochs 2, ring 8, L = 4, B = 4, 8 update steps.
PARITY_EMBED = 32
MIXER_GAIN = 0.15     # on the two hypernetwork output kernels: orthogonal(sqrt 2) leaves q_tot at several tens, where the absolute bounds on the loss scalars are below fp32 resolution
PARITY_SEED = 3
PARITY_SEED_BUMP = {}   # (env, variant) -> seed increment, where the fp64 restatement has a near tie at PARITY_SEED (tests/test_qmix_system.py)


def parity_case(case, variant, dtype=torch.float32):
    return make_case(case, dtype, seed=PARITY_SEED + PARITY_SEED_BUMP.get((case[0], variant), 0), **iql_ref.PARITY_VARIANTS[variant])


def make_case(case, dtype=torch.float32, num_groups=1, seed=PARITY_SEED, **sys_over):
    """(oracle learner after setup, env config of the product, dict of what the device learner needs) of one parity case."""
    il, cfg, info = iql_ref.make_case(case, dtype, num_groups=num_groups, seed=seed, **sys_over)
    A, F = info["A"], info["F"]
    mixer_params = mixer_init(31, A, PARITY_EMBED, A * (F - A))
    for n in ("hyper_w1/Dense_1/kernel", "hyper_w2/Dense_1/kernel"):
        mixer_params[n] = mixer_params[n] * MIXER_GAIN
    ol = QmixOracleLearner(il.spec, il.N, il.sys, info["params"], (il.pre, il.post), il.env, mixer_params, PARITY_EMBED, A, dtype=dtype,
                           num_groups=num_groups, has_mask=il.has_mask)
    ol.setup(info["key"])
    return ol, cfg, dict(info, mixer_params=mixer_params, E=PARITY_EMBED)
