"""CPU restatement of the recurrent Q-learning system (mava/systems/q_learning/anakin/rec_iql.py:210-478), for the tests only: the
eps-greedy distribution (networks/distributions.py:94-138), the Q network (RecQNetwork, networks/base.py:229-273), the stored transition
with real_next_obs, the trajectory buffer, the double-Q TD loss and the target update.  Built on tests/ppo_ref.py (torso, scanned_rnn,
init_named), oracle.prng, oracle.learner.clip_adam_step and oracle.coordsum / oracle.lbf; the product never imports it.

UNPINNED (restated from memory: flashbax, tfp and optax are not part of the reference tree):
  * flashbax's trajectory buffer: ``add`` writes one step per env at the write cursor of a time ring; ``sample`` draws
    key_batch, key_time = split(key), the env row by randint(key_batch, B, 0, N) and the window start by randint(key_time, B, 0, n_valid)
    over the valid starts counted from the OLDEST stored step, so that a window never straddles the write cursor;
  * tfp's Categorical(probs).sample: Gumbel-argmax on log(probs), the noise laid out row-major (counter r K + k), log and gumbel rounded once
    from float64 (oracle.prng.bits_to_gumbel);
  * optax.incremental_update (tau * new + (1 - tau) * old) and optax.periodic_update (copy when steps % period == 0).
Whatever is fixed here the device path reproduces bit for bit (tests/test_qlearn_kernels_gpu.py).
"""
import numpy as np
import torch

from oracle import prng
from tests import ppo_ref

F32 = np.float32
FMIN = np.finfo(np.float32).min


# ----------------------------------------------------------------------------- acting (rec_iql.py:210-236, distributions.py:94-138)
def epsilon(t, eps_min, eps_decay):
    """max(eps_min, 1 - (t / eps_decay) * (1 - eps_min)), every operation rounded to float32 in that order."""
    t, eps_min, eps_decay = F32(t), F32(eps_min), F32(eps_decay)
    return np.maximum(eps_min, F32(F32(1.0) - F32(F32(t / eps_decay) * F32(F32(1.0) - eps_min))))


def greedy_action(q, mask=None):
    """argmax over the legal actions, first maximum wins (jnp.argmax of where(mask, q, finfo.min))."""
    q = np.asarray(q)
    if mask is not None:
        q = np.where(np.asarray(mask, bool), q, q.dtype.type(FMIN))
    return np.argmax(q, axis=-1).astype(np.int32)


def top2_gap(q, mask=None):
    """Gap between the two best legal values of every row [..., K] (inf for a row with one legal action)."""
    q = np.asarray(q, np.float64)
    if mask is not None:
        q = np.where(np.asarray(mask, bool), q, -np.inf)
    v = np.sort(q, axis=-1)
    return np.where(np.isfinite(v[..., -2]), v[..., -1] - v[..., -2], np.inf) if q.shape[-1] > 1 else np.full(q.shape[:-1], np.inf)


def eps_greedy_probs(q, mask, eps):
    """MaskedEpsGreedyDistribution's probs in float32: eps * mask / n_avail + (1 - eps) * onehot(greedy)."""
    q = np.asarray(q, F32)
    K = q.shape[-1]
    m = np.ones(q.shape, bool) if mask is None else np.asarray(mask, bool)
    eps = F32(eps)
    uni = (m.astype(F32) / m.sum(-1, keepdims=True).astype(F32)).astype(F32)
    onehot = (np.arange(K) == greedy_action(q, m)[..., None]).astype(F32)
    return ((eps * uni).astype(F32) + (F32(F32(1.0) - eps) * onehot).astype(F32)).astype(F32)


def perturbed_log_probs(key, probs):
    """log(probs) + gumbel, the values whose argmax is the sample ([R, K] float32; -inf where probs = 0)."""
    p = np.asarray(probs, F32).reshape(-1, probs.shape[-1])
    with np.errstate(divide="ignore"):
        lp = np.log(p.astype(np.float64)).astype(F32)
    g = prng.bits_to_gumbel(prng.random_bits(key, p.size)).reshape(p.shape)
    return (g + lp).astype(F32).reshape(probs.shape)


def eps_greedy_sample(key, q, mask, eps):
    """MaskedEpsGreedyDistribution(q, eps, mask).sample(seed=key) over rows [..., K] -> (action, greedy action) int32."""
    probs = eps_greedy_probs(q, mask, eps)
    return np.argmax(perturbed_log_probs(key, probs), axis=-1).astype(np.int32), greedy_action(np.asarray(q, F32), mask)


def q_apply(p, hidden, obs, done, pre, post):
    """RecQNetwork.get_q_values (base.py:247-262): obs (T, N, A, F), done (T, N, A) bool -> (hidden, q (T, N, A, K))."""
    h, ys = ppo_ref.scanned_rnn(p, hidden, ppo_ref.torso(p, "pre", obs.to(hidden.dtype), pre), done)
    return h, ppo_ref.torso(p, "post", ys, post) @ p["head.kernel"] + p["head.bias"]


# ----------------------------------------------------------------------------- trajectory buffer (UNPINNED: flashbax)
class Ring:
    """Time ring [N][S] per field of the Transition (q_learning/types.py) plus the action masks of obs / next_obs."""

    def __init__(self, N, S, A, F, K, has_mask=True):
        self.N, self.S, self.cursor, self.filled = N, S, 0, 0
        z = lambda shape, dt: np.zeros((N, S, *shape), dt)
        self.data = dict(obs=z((A, F), F32), mask=z((A, K), np.uint8) if has_mask else None, action=z((A,), np.int32), reward=z((A,), F32),
                         terminal=z((), np.uint8), term_or_trunc=z((), np.uint8), next_obs=z((A, F), F32),
                         next_mask=z((A, K), np.uint8) if has_mask else None)

    def add(self, **step):
        for k, v in self.data.items():
            if v is not None:
                v[:, self.cursor] = np.asarray(step[k]).astype(v.dtype)
        self.cursor = (self.cursor + 1) % self.S
        self.filled = min(self.filled + 1, self.S)

    def sample_indices(self, key, B, L):
        return sample_indices(key, B, L, self.N, self.S, self.cursor, self.filled)

    def gather(self, env_idx, start, L):
        """Windows [B][L] per field (None for absent masks)."""
        t = (np.asarray(start)[:, None] + np.arange(L)[None]) % self.S
        return {k: None if v is None else v[np.asarray(env_idx)[:, None], t] for k, v in self.data.items()}


def sample_indices(key, B, L, N, S, cursor, filled):
    """(env_idx [B], start [B]) int32 of the uniformly sampled windows; needs filled >= L."""
    n_valid = filled - L + 1
    if n_valid < 1:
        raise ValueError("the ring holds fewer steps than one window")
    ks = prng.split(key, 2)
    env_idx = prng.randint(ks[0], B, 0, N)
    oldest = cursor if filled == S else 0
    start = (oldest + prng.randint(ks[1], B, 0, n_valid)) % S
    return env_idx.astype(np.int32), start.astype(np.int32)


def training_rows(win):
    """rec_iql.py:335-350: the L - 1 aligned rows of every window [B][L]."""
    d = {k: None if v is None else v[:, :-1] for k, v in win.items()}
    n = {k: None if v is None else v[:, 1:] for k, v in win.items()}
    return dict(obs=d["obs"], term_or_trunc=d["term_or_trunc"], action=d["action"], reward=d["reward"], next_obs=d["next_obs"],
                next_mask=d["next_mask"], next_term_or_trunc=n["term_or_trunc"], next_terminal=n["terminal"])


# ----------------------------------------------------------------------------- loss (rec_iql.py:366-377, :299-328)
def td_loss(q, qn_online, qn_target, action, next_mask, reward, next_terminal, gamma):
    """Torch tensors of any float dtype: q / qn_* [..., K], action / reward [...], next_terminal broadcastable to [...].
    Returns (q_loss, mean_q, mean_target, target, next_action); q_loss is differentiable in q."""
    qm = qn_online if next_mask is None else torch.where(next_mask.bool(), qn_online, torch.full_like(qn_online, float(FMIN)))
    next_a = torch.argmax(qm, dim=-1)   # (torch.argmax returns the first maximum on the CPU)
    next_q = torch.gather(qn_target, -1, next_a[..., None])[..., 0]
    target = (reward + (1.0 - next_terminal.to(q.dtype)) * gamma * next_q).detach()
    q_sel = torch.gather(q, -1, action.long()[..., None])[..., 0]
    return ((q_sel - target) ** 2).mean(), q_sel.mean(), target.mean(), target, next_a


def target_update(online, target, mode, tau, t_train, period):
    """optax.incremental_update (mode 0) in float32 in the order tau * new + (1 - tau) * old, or optax.periodic_update (mode 1)."""
    o, t = np.asarray(online, F32), np.asarray(target, F32)
    if mode == 0:
        tau = F32(tau)
        return ((tau * o).astype(F32) + (F32(F32(1.0) - tau) * t).astype(F32)).astype(F32)
    return o.copy() if t_train % period == 0 else t.copy()


# ----------------------------------------------------------------------------- real_next_obs (auto_reset_wrapper.py:52-83)
def step_with_real_obs(env, spec, state, actions):
    """(new state, timestep, real observation dict): the state itself stepped with auto_reset=True, a copy with auto_reset=False for the
    observation before the auto-reset."""
    copy = {k: np.array(v, copy=True) for k, v in state.items()}
    _, real = env.step(spec, copy, actions, auto_reset=False)
    new_state, ts = env.step(spec, state, actions, auto_reset=True)
    return new_state, ts, real["observation"]


# ----------------------------------------------------------------------------- learner (rec_iql.py:210-478)
class _GroupState:
    pass


class IqlOracleLearner:
    """rec_iql on the CPU with ``num_groups`` groups (the reference's update-batch axis) that share parameters and optimiser.  ``sys``: anything
    with the fields of magpo_amd.q_learner.QSystemConfig.  Training epochs are skipped until every ring holds max(min_buffer_size,
    sample_sequence_length) steps (the product's stated deviation: the keys are still split, t_train does not advance)."""

    def __init__(self, spec, num_envs, sys, params, torsos, env, dtype=torch.float32, num_groups=1, has_mask=True):
        from oracle import learner as olearn
        self.olearn = olearn
        self.spec, self.N, self.sys, self.env, self.dtype, self.U, self.has_mask = spec, num_envs, sys, env, dtype, num_groups, has_mask
        self.pre, self.post = torsos
        self.online = {k: v.clone().to(dtype) for k, v in params.items()}
        self.target = {k: v.clone().to(dtype) for k, v in params.items()}
        self.opt = olearn.adam_init(self.online)
        self.t_train = 0
        self.log = []          # per env step and group: dict(key, q, mask, eps, action)
        self.train_log = []    # per trained epoch: dict(env_idx, start, info, grads, q, qn_online, next_mask)

    def setup(self, key):
        """rec_iql.py:155-195: key, reset_key = split(key); env keys = split(reset_key, U N); learner keys = split(key, U)."""
        N, A, K = self.N, self.spec.num_agents, self.spec.num_actions if hasattr(self.spec, "num_actions") else 6
        ks = prng.split(key, 2)
        env_keys, first = prng.split(ks[1], self.U * N), prng.split(ks[0], self.U)
        self.groups = []
        for u in range(self.U):
            g = _GroupState()
            g.env_state, g.timestep = self.env.reset(self.spec, env_keys[u * N:(u + 1) * N])
            g.key = first[u]
            g.terminal, g.tot = np.zeros(N, bool), np.zeros(N, bool)
            g.hidden = torch.zeros(N, A, 128, dtype=self.dtype)
            g.t = 0
            g.ring = Ring(N, self.sys.buffer_size, A, g.timestep["observation"]["agents_view"].shape[-1], K, self.has_mask)
            self.groups.append(g)
        self.A, self.K = A, K

    @torch.no_grad()
    def rollout(self):
        s, A = self.sys, self.A
        metrics = []
        for g in self.groups:
            ks = prng.split(g.key, 3)                                                        # :447
            g.key, key, g.train_key = ks[0], ks[1], ks[2]
            gm = {k: [] for k in ("episode_return", "episode_length", "is_terminal_step")}
            for _ in range(s.rollout_length):
                ob = g.timestep["observation"]
                obs = np.asarray(ob["agents_view"], F32)
                mask = ob["action_mask"] if self.has_mask else None
                eps = epsilon(g.t, s.eps_min, s.eps_decay)                                   # :216-218
                tot = torch.from_numpy(np.repeat(g.tot[:, None], A, axis=1))
                g.hidden, q = q_apply(self.online, g.hidden, torch.from_numpy(obs)[None], tot[None], self.pre, self.post)
                q = q[0]
                ks = prng.split(key, 2)                                                      # :227
                key, explore_key = ks[0], ks[1]
                action, _ = eps_greedy_sample(explore_key, q.to(torch.float32).numpy(), mask, eps)
                self.log.append(dict(key=explore_key, q=q.clone(), mask=mask, eps=eps, action=action))
                g.env_state, g.timestep, real = step_with_real_obs(self.env, self.spec, g.env_state, action)
                g.ring.add(obs=obs, mask=mask, action=action, reward=g.timestep["reward"], terminal=g.terminal, term_or_trunc=g.tot,
                           next_obs=np.asarray(real["agents_view"], F32), next_mask=real["action_mask"] if self.has_mask else None)
                g.terminal = g.timestep["discount"][:, 0] == 0                               # :264
                g.tot = g.timestep["step_type"] == 2                                         # :265 (STEP_LAST)
                g.t += self.N                                                                # :233
                for k in gm:
                    gm[k].append(g.timestep["episode_metrics"][k].copy())
            metrics.append({k: np.stack(v) for k, v in gm.items()})
        return metrics

    def ready(self):
        need = max(self.sys.min_buffer_size, self.sys.sample_sequence_length)
        return all(g.ring.filled >= need for g in self.groups)

    def group_loss(self, online, g, env_idx, start):
        """update_q's loss of one group's sampled windows (rec_iql.py:330-381): returns (loss, info dict, detail dict)."""
        s, A, dt = self.sys, self.A, self.dtype
        rows = training_rows(g.ring.gather(env_idx, start, s.sample_sequence_length))

        def tm(x, d=None):                                                                   # (B, T, ...) -> (T, B, ...)
            t = torch.from_numpy(np.ascontiguousarray(np.swapaxes(x, 0, 1)))
            return t if d is None else t.to(d)
        B = len(env_idx)
        h0 = torch.zeros(B, A, 128, dtype=dt)
        rep = lambda f: tm(f).bool()[..., None].expand(-1, -1, A)
        with torch.no_grad():
            _, qn_online = q_apply(self.online, h0, tm(rows["next_obs"], dt), rep(rows["next_term_or_trunc"]), self.pre, self.post)
            _, qn_target = q_apply(self.target, h0, tm(rows["next_obs"], dt), rep(rows["next_term_or_trunc"]), self.pre, self.post)
        _, q = q_apply(online, h0, tm(rows["obs"], dt), rep(rows["term_or_trunc"]), self.pre, self.post)
        nmask = None if rows["next_mask"] is None else tm(rows["next_mask"])
        loss, mean_q, mean_t, target, next_a = td_loss(q, qn_online, qn_target, tm(rows["action"]), nmask, tm(rows["reward"], dt),
                                                       tm(rows["next_terminal"], dt)[..., None], s.gamma)
        return loss, dict(q_loss=loss, mean_q=mean_q, mean_target=mean_t), dict(q=q.detach(), qn_online=qn_online, next_mask=nmask, rows=rows)

    def train(self):
        """``epochs`` x train (rec_iql.py:403-422); returns the per-epoch loss_info (None for a skipped epoch)."""
        s, infos = self.sys, []
        ready = self.ready()
        for _ in range(s.epochs):
            for g in self.groups:
                ks = prng.split(g.train_key, 2)                                              # :409
                g.train_key, g.buff_key = ks[0], ks[1]
            if not ready:
                infos.append(None)
                continue
            online = {k: v.detach().clone().requires_grad_(True) for k, v in self.online.items()}
            total, info_sum, details, idxs = 0.0, None, [], []
            for g in self.groups:
                env_idx, start = g.ring.sample_indices(g.buff_key, s.sample_batch_size, s.sample_sequence_length)
                loss, info, det = self.group_loss(online, g, env_idx, start)
                total = total + loss / self.U                                                # pmean over "batch" (:385)
                info_sum = {k: v.detach() / self.U for k, v in info.items()} if info_sum is None else \
                    {k: info_sum[k] + v.detach() / self.U for k, v in info.items()}
                details.append(det); idxs.append((env_idx, start))
            grads = dict(zip(online, torch.autograd.grad(total, list(online.values()), allow_unused=True)))
            grads = {k: torch.zeros_like(online[k]) if v is None else v for k, v in grads.items()}
            self.online, self.opt, _ = self.olearn.clip_adam_step(self.online, grads, self.opt, s.q_lr, s.max_grad_norm)
            with torch.no_grad():
                if s.hard_update:                                                            # :389-396, t_train before its increment
                    if self.t_train % s.update_period == 0:
                        self.target = {k: v.clone() for k, v in self.online.items()}
                elif self.dtype == torch.float32:
                    self.target = {k: torch.from_numpy(target_update(self.online[k].numpy(), self.target[k].numpy(), 0, s.tau, 0, 1)) for k in self.online}
                else:
                    self.target = {k: s.tau * self.online[k] + (1.0 - s.tau) * self.target[k] for k in self.online}
            self.t_train += 1
            info = {k: float(v) for k, v in info_sum.items()}
            infos.append(info)
            self.train_log.append(dict(idx=idxs, info=info, grads=grads, details=details))
        return infos

    def update_step(self):
        metrics = self.rollout()
        return metrics, self.train()


# ----------------------------------------------------------------------------- the parity cases of tests/test_q_learner_gpu.py
# (env, env args); coordsum args = (A, K, time_limit, maxval), lbf = LbfSpec's.  4 envs, rollout_length 2, epochs 2, ring 8, L = 4, B = 4.
PARITY_CASES = [("coordsum", (2, 4, 6, 7)), ("lbf", (5, 5, 2, 2, 2, False, 5))]
PARITY_N, PARITY_SEED, PARITY_STEPS = 4, 3, 8     # 8 update steps x 2 env steps: the ring of 8 wraps, episodes of 5 / 6 steps end inside windows
HEAD_GAIN = 1.0                                   # (orthogonal(0.01) leaves the Q values of an untrained head too close together for a tie-free check)


PARITY_VARIANTS = {"soft": dict(), "hard": dict(hard_update=True), "two-groups": dict(num_groups=2)}
PARITY_SEED_BUMP = {("coordsum", "two-groups"): 1}   # (env, variant) -> seed increment, where the fp64 restatement has a near tie at PARITY_SEED (tests/test_iql_system.py)


def parity_case(case, variant, dtype=torch.float32):
    return make_case(case, dtype, seed=PARITY_SEED + PARITY_SEED_BUMP.get((case[0], variant), 0), **PARITY_VARIANTS[variant])


def parity_sys(**over):
    from magpo_amd.q_learner import QSystemConfig
    kw = dict(rollout_length=2, epochs=2, buffer_size=8, min_buffer_size=4, sample_batch_size=4, sample_sequence_length=4, q_lr=3e-4, max_grad_norm=10.0,
              hard_update=False, update_period=3, tau=0.01, gamma=0.99, eps_min=0.05, eps_decay=40.0)
    kw.update(over)
    return QSystemConfig(**kw)


def make_case(case, dtype=torch.float32, num_groups=1, seed=PARITY_SEED, **sys_over):
    """(oracle learner after setup, env config of the product, dict of what the device learner needs) of one parity case."""
    from magpo_amd.envs import CoordSumConfig, LbfConfig
    from magpo_amd.torso import DEFAULT_TORSO
    from oracle import coordsum as cs
    from oracle import lbf as olbf
    env, args = case
    if env == "coordsum":
        spec, cfg, mod, has_mask = cs.CoordSumSpec(*args), CoordSumConfig(*args), cs, False
        A, K, F = args[0], args[1], args[0] + 1
    else:
        spec, cfg, mod, has_mask = olbf.LbfSpec(*args), LbfConfig(*args), olbf, True
        A, K, F = spec.num_agents, 6, spec.obs_dim
    params = ppo_ref.init_named(21, F, K, DEFAULT_TORSO, DEFAULT_TORSO, HEAD_GAIN)
    sys = parity_sys(**sys_over)
    ol = IqlOracleLearner(spec, PARITY_N, sys, params, (DEFAULT_TORSO, DEFAULT_TORSO), mod, dtype=dtype, num_groups=num_groups, has_mask=has_mask)
    key = prng.split(prng.prng_key(seed), 4)[0]
    ol.setup(key)
    return ol, cfg, dict(key=key, params=params, sys=sys, A=A, K=K, F=F, N=PARITY_N)
