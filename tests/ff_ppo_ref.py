"""CPU restatement of the feed-forward PPO systems (mava/systems/ppo/anakin/ff_mappo.py, ff_ippo.py), for the tests only: the networks
(FeedForwardActor / FeedForwardValueNet, base.py:38-88) and the learner of ff_mappo.py:56-265 -- rollout with its key chain, whole-batch
sampling, GAE, the flat shuffle over rollout_length x num_envs items, both losses through autograd, the logging quirk and two optax
clip + Adam chains.  ff_ippo.py is the same file with ``centralised_critic=False`` (its critic reads agents_view) and no global state.
Built on tests/ppo_ref.py (MLPTorso, global state, the losses' owner class), oracle.networks, oracle.prng and oracle.learner; the product never
imports it.

Parameters are dicts name -> tensor with the names of magpo_amd.params.ff_layout (torso layer i: ``pre`` / ``pre1`` / ``pre2`` ``.kernel`` /
``.bias`` / ``.ln.bias``; ``head.kernel`` [D, K], the critic's [D, 1])."""
import numpy as np
import torch

from oracle import coordsum as cs
from oracle import learner as olearn
from oracle import networks as nets
from oracle import prng
from tests import ppo_ref as pr

LOSS_NAMES = pr.LOSS_NAMES   # loss_info of ff_mappo.py:226-231: the same keys and the same quirk as rec_mappo's


# ----------------------------------------------------------------------------- networks
def actor_apply(p, obs, mask, spec):
    """FeedForwardActor.__call__ (base.py:50-57): torso -> action head; normalised masked log-probs (..., K)."""
    x = pr.torso(p, "pre", obs.to(p["head.kernel"].dtype), spec)
    return nets.masked_log_softmax(x @ p["head.kernel"] + p["head.bias"], mask)


def critic_apply(p, obs, spec):
    """FeedForwardValueNet.__call__ (base.py:73-88): ``obs`` = agents_view or global_state rows (..., F) -> value (...)."""
    x = pr.torso(p, "pre", obs.to(p["head.kernel"].dtype), spec)
    return (x @ p["head.kernel"] + p["head.bias"]).squeeze(-1)


def merge_leading_dims(x, n):
    """mava/utils/jax_utils.py: reshape the first ``n`` axes into one."""
    return x.reshape(-1, *x.shape[n:])


# ----------------------------------------------------------------------------- learner (ff_mappo.py:56-265)
class FfPpoOracleLearner(pr.PpoOracleLearner):
    """Single-group feed-forward PPO learner on the CPU.  From the recurrent restatement it keeps ``critic_obs``, ``minibatch_grads`` (which
    calls the two loss functions below), ``_lr`` and ``update_step``."""

    def __init__(self, spec, num_envs, sys, actor_params, critic_params, *, centralised, critic_lr=None, torsos=None, dtype=torch.float32, env=cs):
        """``torsos`` = (actor torso, critic torso) TorsoSpec-likes."""
        from magpo_amd.ff_nets import FF_DEFAULT_TORSO
        super().__init__(spec, num_envs, sys, actor_params, critic_params, centralised=centralised, critic_lr=critic_lr, dtype=dtype, env=env)
        self.torsos = torsos or (FF_DEFAULT_TORSO,) * 2

    def setup(self, key):
        """learner_setup PRNG layout (ff_mappo.py:340-358): env keys = split(key, N + 1)[1:], then key, step_key = split(key)."""
        N, A = self.N, self.spec.num_agents
        ks = prng.split(key, N + 1)
        self.env_state, self.timestep = self.env.reset(self.spec, ks[1:])
        self.key = prng.split(ks[0], 2)[1]
        self.dones = np.zeros((N, A), bool)

    @torch.no_grad()
    def rollout(self, T=None):
        """_env_step x T (ff_mappo.py:76-104), the bootstrap value (:108) and GAE (:110-112)."""
        sys, spec = self.sys, self.spec
        T = T or sys.rollout_length
        traj = {k: [] for k in ("done", "action", "value", "reward", "log_prob", "obs", "mask", "lp_all")}
        metrics = {k: [] for k in ("episode_return", "episode_length", "is_terminal_step")}
        for _ in range(T):
            ks = prng.split(self.key, 2)                                                     # :83
            self.key, policy_key = ks[0], ks[1]
            ob = self.timestep["observation"]
            obs, mask = torch.from_numpy(ob["agents_view"]), torch.from_numpy(ob["action_mask"]).bool()
            last_done = torch.from_numpy(self.dones)
            lp = actor_apply(self.ap, obs, mask, self.torsos[0])                             # :84
            value = critic_apply(self.cp, self.critic_obs(obs), self.torsos[1])              # :85
            action = torch.from_numpy(prng.categorical(policy_key, lp.to(torch.float32).numpy()))   # :86: ONE draw over the (N, A, K) batch
            logp = torch.gather(lp, -1, action.long()[..., None])[..., 0]                    # :87
            self.env_state, self.timestep = self.env.step(spec, self.env_state, action.numpy(), auto_reset=True)   # :90
            done = self.timestep["step_type"] == cs.STEP_LAST
            self.dones = np.repeat(done[:, None], spec.num_agents, axis=1)                   # :92
            for k, x in (("done", last_done), ("action", action), ("value", value), ("reward", torch.from_numpy(self.timestep["reward"]).to(self.dtype)),
                         ("log_prob", logp), ("obs", obs), ("mask", mask), ("lp_all", lp)):
                traj[k].append(x)
            for k in metrics:
                metrics[k].append(self.timestep["episode_metrics"][k].copy())
        obs = torch.from_numpy(self.timestep["observation"]["agents_view"])
        last_done = torch.from_numpy(self.dones)
        last_val = critic_apply(self.cp, self.critic_obs(obs), self.torsos[1])               # :108
        traj = {k: torch.stack(v, dim=0) for k, v in traj.items()}
        traj["adv"], traj["targets"] = olearn.calculate_gae(traj["reward"], traj["value"], traj["done"], last_val, last_done, sys.gamma, sys.gae_lambda)
        self.traj, self.last_val = traj, last_val
        return {k: np.stack(v, axis=0) for k, v in metrics.items()}

    def make_minibatches(self, perm):
        """ff_mappo.py:238-246: merge_leading_dims(x, 2) of the time-major batch, take by the permutation of rollout_length * num_envs items,
        reshape into num_minibatches slices; fields are (items, A, ...)."""
        M = self.sys.num_minibatches
        bp = torch.from_numpy(perm.astype(np.int64))
        fields = {k: merge_leading_dims(self.traj[k], 2).index_select(0, bp) for k in ("done", "action", "value", "log_prob", "obs", "mask", "adv", "targets")}
        return [{k: v.reshape(M, -1, *v.shape[1:])[m] for k, v in fields.items()} for m in range(M)]

    def actor_loss(self, params, mb):
        """_actor_loss_fn (ff_mappo.py:122-152)."""
        s = self.sys
        lp = actor_apply(params, mb["obs"], mb["mask"], self.torsos[0])
        logp = torch.gather(lp, -1, mb["action"].long()[..., None])[..., 0]
        ratio = torch.exp(logp - mb["log_prob"])
        gae = mb["adv"]
        gae = (gae - gae.mean()) / (gae.std(unbiased=False) + 1e-8)                         # :136
        actor = -torch.minimum(ratio * gae, torch.clamp(ratio, 1.0 - s.clip_eps, 1.0 + s.clip_eps) * gae).mean()
        pr_ = lp.exp()
        entropy = (-torch.where(pr_ == 0, torch.zeros_like(pr_), pr_ * lp).sum(-1)).mean()
        return actor - s.ent_coef * entropy, (actor, entropy), logp

    def critic_loss(self, params, mb):
        """_critic_loss_fn (ff_mappo.py:154-172)."""
        s = self.sys
        value = critic_apply(params, self.critic_obs(mb["obs"]), self.torsos[1])
        vclip = mb["value"] + (value - mb["value"]).clamp(-s.clip_eps, s.clip_eps)
        vl = 0.5 * torch.maximum((value - mb["targets"]) ** 2, (vclip - mb["targets"]) ** 2).mean()
        return s.vf_coef * vl, vl, value

    def update(self, grad_hook=None):
        """_update_epoch x ppo_epochs (ff_mappo.py:114-261).  Returns the loss_info of every minibatch and the permutations used."""
        s, infos, perms = self.sys, [], []
        n_items = self.traj["action"].shape[0] * self.N                                      # :238
        for _ in range(s.ppo_epochs):
            ks = prng.split(self.key, 3)                                                     # :235
            self.key, shuffle_key, entropy_key = ks[0], ks[1], ks[2]
            perm = prng.permutation(shuffle_key, n_items)                                    # :239
            perms.append(perm)
            for mb in self.make_minibatches(perm):
                entropy_key = prng.split(entropy_key, 2)[1]                                  # :175,232: carried, unused for discrete actions
                ga, gc, info, _ = self.minibatch_grads(mb)
                if grad_hook is not None:
                    ga, gc = grad_hook(ga, gc)
                self.ap, self.a_opt, _ = olearn.clip_adam_step(self.ap, ga, self.a_opt, self._lr(s.actor_lr, self.a_opt["count"]), s.max_grad_norm)
                self.cp, self.c_opt, _ = olearn.clip_adam_step(self.cp, gc, self.c_opt, self._lr(self.critic_lr, self.c_opt["count"]), s.max_grad_norm)
                infos.append(info)
        return infos, perms


# ----------------------------------------------------------------------------- the parity cases of tests/test_ff_ppo_learner_gpu.py
# (system, env, env args, N, T, torso, episode ends inside the rollouts); coordsum args = (A, K, time_limit, maxval), lbf = LbfSpec's.
TANH_WIDE = dict(layer_sizes=(64, 192), activation="tanh", use_layer_norm=False, activate_final=True)   # no small first layer: the padded operand
LN_TANH = pr.LN_TANH                                                                                     # LayerNorm: the composed chain
_ENVS = [("coordsum", (2, 10, 5, 15), 8, 8, None, True), ("coordsum", (3, 30, 100, 50), 8, 8, None, False),
         ("coordsum", (3, 10, 6, 30), 8, 8, TANH_WIDE, True), ("lbf", (8, 8, 2, 2, 2, True, 6), 8, 8, None, True)]
PARITY_CASES = [(system, *e) for system in ("ff_ippo", "ff_mappo") for e in _ENVS]
LN_CASES = [(system, "coordsum", (3, 10, 6, 30), 8, 8, LN_TANH, True) for system in ("ff_ippo", "ff_mappo")]   # two update steps on the composed chain
PARITY_SEED = 42
PARITY_SEED_BUMP = {}   # case id -> seed increment, where the fp64 restatement has a Gumbel near-tie at PARITY_SEED (tests/test_ff_ppo_system.py)
PARITY_EPOCHS, PARITY_MINIBATCHES = 2, 2


def case_id(c):
    system, env, args, N, T, torso_kw, ends = c
    A = args[0] if env == "coordsum" else args[2]
    torso = "" if not torso_kw else "-lntanh" if torso_kw.get("use_layer_norm") else "-tanh"
    return f"{system}-{env}-A{A}-T{T}{torso}{'' if ends else '-noend'}"


def init_named(seed, F, K, torso, head_gain, bias_std=0.05):
    """Parameters under the names of magpo_amd.params.ff_layout: the project's initialiser (orthogonal torso, orthogonal head of gain
    ``head_gain``) with small random biases, so that every bias gradient is exercised."""
    from magpo_amd.params import FlatParams, ff_layout, init_ff
    named = FlatParams(ff_layout(F, K, torso), "cpu").views()
    init_ff(named, seed, head_gain)
    g = torch.Generator().manual_seed(seed + 77)
    with torch.no_grad():
        for n, v in named.items():
            if n.endswith("bias"):
                v.copy_(torch.randn(v.shape, generator=g) * bias_std)
    return {k: v.clone() for k, v in named.items()}


def make_case(c, dtype=torch.float32):
    """(oracle learner after setup, env config of the product, dict of what the device learner needs) of one parity case."""
    from magpo_amd.envs import CoordSumConfig, LbfConfig
    from magpo_amd.ff_nets import FF_DEFAULT_TORSO
    from magpo_amd.torso import TorsoSpec
    from oracle import lbf as olbf
    system, env, args, N, T, torso_kw, ends = c
    if env == "coordsum":
        spec, cfg, mod = cs.CoordSumSpec(*args), CoordSumConfig(*args), cs
        A, K, F = args[0], args[1], args[0] + 1
    else:
        spec, cfg, mod = olbf.LbfSpec(*args), LbfConfig(*args), olbf
        A, K, F = spec.num_agents, 6, spec.obs_dim
    centralised = system == "ff_mappo"
    ts = TorsoSpec(**torso_kw) if torso_kw else FF_DEFAULT_TORSO
    cF = A * (F - A) if centralised else F
    ap = init_named(11, F, K, ts, 0.3 if env == "lbf" else 0.01)     # (masked envs: logits with a visible spread)
    cp = init_named(12, cF, 1, ts, 1.0)
    sys = olearn.SystemCfg(rollout_length=T, ppo_epochs=PARITY_EPOCHS, num_minibatches=PARITY_MINIBATCHES, actor_lr=2.5e-4)
    ol = FfPpoOracleLearner(spec, N, sys, ap, cp, centralised=centralised, critic_lr=5e-4, torsos=(ts, ts), dtype=dtype, env=mod)
    key = prng.split(prng.prng_key(PARITY_SEED + PARITY_SEED_BUMP.get(case_id(c), 0)), 4)[0]
    ol.setup(key)
    return ol, cfg, dict(key=key, ap=ap, cp=cp, torso=ts, centralised=centralised, A=A, K=K, F=F, N=N, T=T, critic_lr=5e-4)
