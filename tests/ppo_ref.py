"""CPU restatement of the recurrent PPO systems (mava/systems/ppo/anakin/rec_mappo.py, rec_ippo.py), for the tests only: the critic
network (RecurrentValueNet, base.py:187-226), observation.global_state (wrappers/matrax.py:128-131, jumanji.py:61-67) and the learner of
rec_mappo.py:70-362 -- rollout, key chain, whole-batch sampling, GAE, shuffle, both losses, the logging quirk and two optimisers.  rec_ippo.py
is the same file with ``centralised_critic=False`` (its critic reads agents_view) and no global state.  Built on oracle.networks
(gru_cell, masked_log_softmax), oracle.prng and oracle.learner (calculate_gae, clip_adam_step); the product never imports it.

Parameters are dicts name -> tensor with the names of magpo_amd.params.actor_layout (torso layer i: ``pre`` / ``pre1`` / ``pre2``
``.kernel`` / ``.bias`` / ``.ln.bias``), so any torso the product supports can be restated; the critic's head is ``head.kernel`` [D, 1]."""
import numpy as np
import torch

from oracle import coordsum as cs
from oracle import learner as olearn
from oracle import networks as nets
from oracle import prng

LOSS_NAMES = ("total_loss", "value_loss", "actor_loss", "entropy")   # loss_info of rec_mappo.py:286-291


# ----------------------------------------------------------------------------- networks
def torso(p, prefix, x, spec):
    """MLPTorso (torsos.py:24-47): Dense -> LayerNorm(use_scale=False) if use_layer_norm -> activation (not on the last layer unless
    activate_final).  ``spec``: anything with layer_sizes / activation / use_layer_norm / activate_final (magpo_amd.torso.TorsoSpec)."""
    n = len(spec.layer_sizes)
    for i in range(n):
        name = prefix if i == 0 else f"{prefix}{i}"
        x = x @ p[name + ".kernel"] + p[name + ".bias"]
        if spec.use_layer_norm:   # flax LayerNorm(use_scale=False): eps 1e-6, fast variance E[x^2] - E[x]^2 clamped at 0, bias only
            mean = x.mean(-1, keepdim=True)
            var = torch.clamp((x * x).mean(-1, keepdim=True) - mean * mean, min=0.0)
            x = (x - mean) * torch.rsqrt(var + 1e-6) + p[name + ".ln.bias"]
        if i < n - 1 or spec.activate_final:
            x = torch.relu(x) if spec.activation == "relu" else torch.tanh(x)
    return x


def scanned_rnn(p, hidden, emb, done):
    """ScannedRNN (base.py:121-142): hidden (N, A, H); emb (T, N, A, D); done (T, N, A) bool -> (last hidden, per-step hidden)."""
    outs, h = [], hidden
    for t in range(emb.shape[0]):
        h = torch.where(done[t][..., None], torch.zeros_like(h), h)
        h = nets.gru_cell(p, h, emb[t])
        outs.append(h)
    return h, torch.stack(outs, dim=0)


def actor_apply(p, hidden, obs, done, mask, pre, post):
    """RecurrentActor.__call__ (base.py:161-184) for any torso: -> (hidden, normalised masked log-probs (T, N, A, K))."""
    h, ys = scanned_rnn(p, hidden, torso(p, "pre", obs.to(hidden.dtype), pre), done)
    logits = torso(p, "post", ys, post) @ p["head.kernel"] + p["head.bias"]
    return h, nets.masked_log_softmax(logits, mask)


def critic_apply(p, hidden, obs, done, pre, post):
    """RecurrentValueNet.__call__ (base.py:196-226): ``obs`` = agents_view or global_state rows (T, N, A, F) -> (hidden, value (T, N, A))."""
    h, ys = scanned_rnn(p, hidden, torso(p, "pre", obs.to(hidden.dtype), pre), done)
    value = torso(p, "post", ys, post) @ p["head.kernel"] + p["head.bias"]
    return h, value.squeeze(-1)


def global_state(agents_view, num_agents: int, id_cols: int):
    """observation.global_state from wrapped agents_view rows (..., A, F): the raw views (behind the ``id_cols`` one-hot columns the
    AgentIDWrapper put in front, make_env.py:90-104) of all agents concatenated (matrax.py:128-131: jnp.concatenate(obs, axis=0)) and tiled
    to every agent (jnp.tile(global_obs, (num_agents, 1)))."""
    raw = agents_view[..., id_cols:]
    flat = raw.reshape(*raw.shape[:-2], 1, num_agents * raw.shape[-1])
    return flat.expand(*raw.shape[:-2], num_agents, flat.shape[-1])


# ----------------------------------------------------------------------------- learner (rec_mappo.py:70-362)
class PpoOracleLearner:
    """Single-group recurrent PPO learner on the CPU."""

    def __init__(self, spec, num_envs, sys, actor_params, critic_params, *, centralised, critic_lr=None, torsos=None, dtype=torch.float32, env=cs):
        """``torsos`` = (actor pre, actor post, critic pre, critic post) TorsoSpec-likes; ``env``: oracle.coordsum or oracle.lbf."""
        from magpo_amd.torso import DEFAULT_TORSO
        self.spec, self.N, self.sys, self.dtype, self.env, self.centralised = spec, num_envs, sys, dtype, env, centralised
        self.torsos = torsos or (DEFAULT_TORSO,) * 4
        self.ap = {k: v.clone().to(dtype) for k, v in actor_params.items()}
        self.cp = {k: v.clone().to(dtype) for k, v in critic_params.items()}
        self.a_opt, self.c_opt = olearn.adam_init(self.ap), olearn.adam_init(self.cp)
        self.critic_lr = sys.actor_lr if critic_lr is None else critic_lr

    def setup(self, key):
        """learner_setup PRNG layout (rec_mappo.py:495-513): env keys = split(key, N + 1)[1:], then key, step_key = split(key)."""
        N, A = self.N, self.spec.num_agents
        ks = prng.split(key, N + 1)
        self.env_state, self.timestep = self.env.reset(self.spec, ks[1:])
        self.key = prng.split(ks[0], 2)[1]
        self.dones = np.zeros((N, A), bool)
        self.policy_h = torch.zeros(N, A, self.sys.hidden, dtype=self.dtype)    # ScannedRNN.initialize_carry (:455-460)
        self.critic_h = torch.zeros(N, A, self.sys.hidden, dtype=self.dtype)

    def critic_obs(self, agents_view):
        A = self.spec.num_agents
        return global_state(agents_view, A, A) if self.centralised else agents_view

    @torch.no_grad()
    def rollout(self, T=None):
        """_env_step x T (rec_mappo.py:92-149), the bootstrap value (:155-162) and GAE (:164-166)."""
        sys, spec = self.sys, self.spec
        T = T or sys.rollout_length
        traj = {k: [] for k in ("done", "action", "value", "reward", "log_prob", "obs", "mask", "lp_all")}
        metrics = {k: [] for k in ("episode_return", "episode_length", "is_terminal_step")}
        self.policy_h0, self.critic_h0 = self.policy_h.clone(), self.critic_h.clone()       # traj_batch.hstates[0] (:138,186,220)
        a_pre, a_post, c_pre, c_post = self.torsos
        for _ in range(T):
            ks = prng.split(self.key, 2)                                                     # :106
            self.key, policy_key = ks[0], ks[1]
            ob = self.timestep["observation"]
            obs, mask = torch.from_numpy(ob["agents_view"]), torch.from_numpy(ob["action_mask"]).bool()
            last_done = torch.from_numpy(self.dones)
            self.policy_h, lp = actor_apply(self.ap, self.policy_h, obs[None], last_done[None], mask[None], a_pre, a_post)      # :113-115
            self.critic_h, value = critic_apply(self.cp, self.critic_h, self.critic_obs(obs)[None], last_done[None], c_pre, c_post)   # :116-118
            lp, value = lp[0], value[0]
            # actor_policy.sample(seed=policy_key): ONE draw over the whole (1, N, A, K) batch (:121)
            action = torch.from_numpy(prng.categorical(policy_key, lp.to(torch.float32).numpy()))
            logp = torch.gather(lp, -1, action.long()[..., None])[..., 0]                    # :122
            self.env_state, self.timestep = self.env.step(spec, self.env_state, action.numpy(), auto_reset=True)               # :127
            done = self.timestep["step_type"] == cs.STEP_LAST
            self.dones = np.repeat(done[:, None], spec.num_agents, axis=1)                   # :129
            for k, x in (("done", last_done), ("action", action), ("value", value), ("reward", torch.from_numpy(self.timestep["reward"]).to(self.dtype)),
                         ("log_prob", logp), ("obs", obs), ("mask", mask), ("lp_all", lp)):
                traj[k].append(x)
            for k in metrics:
                metrics[k].append(self.timestep["episode_metrics"][k].copy())
        obs = torch.from_numpy(self.timestep["observation"]["agents_view"])
        last_done = torch.from_numpy(self.dones)
        _, last_val = critic_apply(self.cp, self.critic_h, self.critic_obs(obs)[None], last_done[None], c_pre, c_post)          # :159
        last_val = last_val[0]
        traj = {k: torch.stack(v, dim=0) for k, v in traj.items()}
        traj["adv"], traj["targets"] = olearn.calculate_gae(traj["reward"], traj["value"], traj["done"], last_val, last_done, sys.gamma, sys.gae_lambda)
        self.traj, self.last_val = traj, last_val
        return {k: np.stack(v, axis=0) for k, v in metrics.items()}

    def make_minibatches(self, perm):
        """rec_mappo.py:299-321 with one recurrent chunk (recurrent_chunk_size = rollout_length): take the env axis by the permutation,
        split it into num_minibatches slices; fields stay time-major (T, N / M, A, ...).  The start states are traj_batch.hstates[0]."""
        M = self.sys.num_minibatches
        bp = torch.from_numpy(perm.astype(np.int64))
        fields = {k: self.traj[k].index_select(1, bp) for k in ("done", "action", "value", "log_prob", "obs", "mask", "adv", "targets")}
        fields["policy_h0"], fields["critic_h0"] = self.policy_h0.index_select(0, bp)[None], self.critic_h0.index_select(0, bp)[None]
        n = self.N // M
        return [{k: v[:, m * n:(m + 1) * n] for k, v in fields.items()} for m in range(M)]

    def actor_loss(self, params, mb):
        """_actor_loss_fn (rec_mappo.py:176-209)."""
        s = self.sys
        _, lp = actor_apply(params, mb["policy_h0"][0], mb["obs"], mb["done"], mb["mask"], self.torsos[0], self.torsos[1])
        logp = torch.gather(lp, -1, mb["action"].long()[..., None])[..., 0]
        ratio = torch.exp(logp - mb["log_prob"])
        gae = mb["adv"]
        gae = (gae - gae.mean()) / (gae.std(unbiased=False) + 1e-8)                         # :193
        actor = -torch.minimum(ratio * gae, torch.clamp(ratio, 1.0 - s.clip_eps, 1.0 + s.clip_eps) * gae).mean()
        pr = lp.exp()
        entropy = (-torch.where(pr == 0, torch.zeros_like(pr), pr * lp).sum(-1)).mean()
        return actor - s.ent_coef * entropy, (actor, entropy), logp

    def critic_loss(self, params, mb):
        """_critic_loss_fn (rec_mappo.py:211-232)."""
        s = self.sys
        _, value = critic_apply(params, mb["critic_h0"][0], self.critic_obs(mb["obs"]), mb["done"], self.torsos[2], self.torsos[3])
        vclip = mb["value"] + (value - mb["value"]).clamp(-s.clip_eps, s.clip_eps)
        vl = 0.5 * torch.maximum((value - mb["targets"]) ** 2, (vclip - mb["targets"]) ** 2).mean()
        return s.vf_coef * vl, vl, value

    def minibatch_grads(self, mb):
        ap = {k: v.detach().clone().requires_grad_(True) for k, v in self.ap.items()}
        cp = {k: v.detach().clone().requires_grad_(True) for k, v in self.cp.items()}
        a_total, (_, entropy), logp = self.actor_loss(ap, mb)
        c_total, vl, value = self.critic_loss(cp, mb)
        ga = dict(zip(ap, torch.autograd.grad(a_total, list(ap.values()), allow_unused=True)))
        gc = dict(zip(cp, torch.autograd.grad(c_total, list(cp.values()), allow_unused=True)))
        ga = {k: torch.zeros_like(ap[k]) if g is None else g for k, g in ga.items()}
        gc = {k: torch.zeros_like(cp[k]) if g is None else g for k, g in gc.items()}
        # the logging quirk (rec_mappo.py:282-291): actor_loss_info = (total, (actor_loss, entropy)) is unpacked as ``actor_loss, (_, entropy)``,
        # so the logged "actor_loss" is the actor's TOTAL; value_loss_info = (vf_coef * vl, vl) -> "value_loss" is the unscaled one
        info = {k: float(v.detach()) for k, v in dict(total_loss=a_total + c_total, value_loss=vl, actor_loss=a_total, entropy=entropy).items()}
        return ga, gc, info, dict(value=value.detach(), log_prob=logp.detach())

    def _lr(self, base, count):
        s = self.sys
        if not s.decay_learning_rates:
            return base
        return base * (1.0 - (count // (s.ppo_epochs * s.num_minibatches)) / s.lr_num_updates)

    def update(self, grad_hook=None):
        """_update_epoch x ppo_epochs (rec_mappo.py:168-350).  Returns the loss_info of every minibatch and the permutations used."""
        s, infos, perms = self.sys, [], []
        for _ in range(s.ppo_epochs):
            ks = prng.split(self.key, 3)                                                     # :296
            self.key, shuffle_key, entropy_key = ks[0], ks[1], ks[2]
            perm = prng.permutation(shuffle_key, self.N)                                     # :311
            perms.append(perm)
            for mb in self.make_minibatches(perm):
                entropy_key = prng.split(entropy_key, 2)[1]                                  # :235,293: carried, unused for discrete actions
                ga, gc, info, _ = self.minibatch_grads(mb)
                if grad_hook is not None:
                    ga, gc = grad_hook(ga, gc)
                self.ap, self.a_opt, _ = olearn.clip_adam_step(self.ap, ga, self.a_opt, self._lr(s.actor_lr, self.a_opt["count"]), s.max_grad_norm)
                self.cp, self.c_opt, _ = olearn.clip_adam_step(self.cp, gc, self.c_opt, self._lr(self.critic_lr, self.c_opt["count"]), s.max_grad_norm)
                infos.append(info)
        return infos, perms

    def update_step(self):
        metrics = self.rollout()
        infos, _ = self.update()
        return metrics, infos


def gumbel_near_ties(policy_key, lp_all, tol=1e-4):
    """Number of samples whose top two perturbed log-probs g + lp are closer than ``tol`` (a draw that fp32 rounding could flip), with the
    noise recomputed from the key as jax.random.categorical lays it out (row-major over lp_all.shape)."""
    lp = np.asarray(lp_all, np.float64)
    g = prng.bits_to_gumbel(prng.random_bits(policy_key, lp.size)).reshape(lp.shape).astype(np.float64)
    v = np.sort(g + lp, axis=-1)
    return int(((v[..., -1] - v[..., -2]) < tol).sum()) if lp.shape[-1] > 1 else 0


# ----------------------------------------------------------------------------- the parity cases of tests/test_ppo_learner_gpu.py
# (system, env, env args, N, T, torso, episode ends inside the rollouts); coordsum args = (A, K, time_limit, maxval), lbf = LbfSpec's.
# "noend": time limit 100 > 3 T, so non-zero hidden states are carried across the three update steps.
LN_TANH = dict(layer_sizes=(64, 128), activation="tanh", use_layer_norm=True, activate_final=True)
_ENVS = [("coordsum", (2, 10, 5, 15), 8, 8, None, True), ("coordsum", (2, 10, 100, 15), 8, 16, None, False),
         ("coordsum", (3, 30, 6, 50), 8, 8, None, True), ("coordsum", (3, 30, 100, 50), 8, 16, None, False),
         ("coordsum", (5, 20, 5, 80), 8, 8, None, True), ("coordsum", (5, 20, 100, 80), 8, 16, None, False),
         ("coordsum", (3, 10, 6, 30), 8, 8, LN_TANH, True), ("lbf", (8, 8, 2, 2, 2, True, 6), 8, 8, None, True)]
PARITY_CASES = [(system, *e) for system in ("rec_ippo", "rec_mappo") for e in _ENVS]
PARITY_SEED = 42
PARITY_SEED_BUMP = {"rec_ippo-coordsum-A3-T8-lntanh": 1, "rec_mappo-coordsum-A3-T8": 1, "rec_mappo-coordsum-A3-T8-lntanh": 1}   # case id -> seed increment, where the fp64 restatement has a Gumbel near-tie at PARITY_SEED (tests/test_ppo_system.py)
PARITY_EPOCHS, PARITY_MINIBATCHES = 2, 2


def case_id(c):
    system, env, args, N, T, torso_kw, ends = c
    A = args[0] if env == "coordsum" else args[2]
    return f"{system}-{env}-A{A}-T{T}{'-lntanh' if torso_kw else ''}{'' if ends else '-noend'}"


def init_named(seed, F, K, pre, post, head_gain, bias_std=0.05):
    """Parameters under the names of magpo_amd.params.actor_layout for the torsos (pre, post): the project's initialiser (orthogonal torsos,
    lecun-normal / orthogonal GRU kernels, orthogonal head of gain ``head_gain``) with small random biases, so that every bias gradient is
    exercised."""
    from magpo_amd.params import FlatParams, actor_layout, actor_named_views, init_actor
    P = FlatParams(actor_layout(F, 128, K, pre, post), "cpu")
    named = actor_named_views(P.views())
    init_actor(named, seed)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        named["head.kernel"].mul_(head_gain / 0.01)
        for n, v in named.items():
            if n.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * bias_std)
    return {k: v.clone() for k, v in named.items()}


def make_case(c, dtype=torch.float32):
    """(oracle learner after setup, env config of the product, dict of what the device learner needs) of one parity case."""
    from magpo_amd.envs import CoordSumConfig, LbfConfig
    from magpo_amd.torso import DEFAULT_TORSO, TorsoSpec
    from oracle import lbf as olbf
    system, env, args, N, T, torso_kw, ends = c
    if env == "coordsum":
        spec, cfg, mod = cs.CoordSumSpec(*args), CoordSumConfig(*args), cs
        A, K, F = args[0], args[1], args[0] + 1
    else:
        spec, cfg, mod = olbf.LbfSpec(*args), LbfConfig(*args), olbf
        A, K, F = spec.num_agents, 6, spec.obs_dim
    centralised = system == "rec_mappo"
    ts = TorsoSpec(**torso_kw) if torso_kw else DEFAULT_TORSO
    cF = A * (F - A) if centralised else F
    ap = init_named(11, F, K, ts, ts, 0.3 if env == "lbf" else 0.01)     # (masked envs: logits with a visible spread)
    cp = init_named(12, cF, 1, ts, ts, 1.0)
    sys = olearn.SystemCfg(rollout_length=T, ppo_epochs=PARITY_EPOCHS, num_minibatches=PARITY_MINIBATCHES, actor_lr=2.5e-4)
    ol = PpoOracleLearner(spec, N, sys, ap, cp, centralised=centralised, critic_lr=5e-4, torsos=(ts, ts, ts, ts), dtype=dtype, env=mod)
    key = prng.split(prng.prng_key(PARITY_SEED + PARITY_SEED_BUMP.get(case_id(c), 0)), 4)[0]
    ol.setup(key)
    return ol, cfg, dict(key=key, ap=ap, cp=cp, torso=ts, centralised=centralised, A=A, K=K, F=F, N=N, T=T, critic_lr=5e-4)
