"""The feed-forward PPO systems on the GPU (magpo_amd/ff_ppo_learner.py, ff_nets.py, systems/ppo/anakin/ff_*.py) against their CPU restatement
(tests/ff_ppo_ref.py) on identical seeds, parameters and PRNG keys, with the project's bars (tests/test_ppo_learner_gpu.py): sampled actions
and env state bit-exact in every rollout, values and log-probs <= 1e-4, adv / targets 1e-4 / 2e-5, every parameter gradient of both networks
<= 2e-3 of the tensor's max, loss scalars 1e-3, parameters <= 3e-5 per update step.

Sampled actions are compared for exact equality: tests/test_ff_ppo_system.py shows that the fp64 restatement has no Gumbel near-tie (top two
perturbed log-probs within 1e-4) at any of these seeds and shapes, so fp32 rounding cannot flip a draw; a mismatch reports whether the
recomputed noise puts it at a near-tie."""
import os

import numpy as np
import pytest
import torch

from oracle import prng as oprng
from tests import ff_ppo_ref as fr
from tests.gpu_util import _count_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


def _device_learner(cfg, info, **kw):
    from magpo_amd.ff_ppo_learner import FfPpoLearner
    from magpo_amd.learner import SystemConfig
    sysc = SystemConfig(rollout_length=info["T"], ppo_epochs=fr.PARITY_EPOCHS, num_minibatches=fr.PARITY_MINIBATCHES, actor_lr=2.5e-4)
    ts = info["torso"]
    dl = FfPpoLearner(cfg, info["N"], sysc, DEV, centralised=info["centralised"], critic_lr=info["critic_lr"], net_seed=None, wgrad_groups=4,
                      actor_torso=ts, critic_torso=ts, **kw)
    dl.actor.load_named(info["ap"])
    dl.critic.load_named(info["cp"])
    dl.setup(info["key"])
    return dl


def _rollout_parity(ol, dl, what):
    T_ = dl.T
    key0 = ol.key.copy()
    om = ol.rollout()
    dl.rollout()
    tr, otr = dl.traj, ol.traj
    da, oa = tr["action"].cpu().numpy(), otr["action"].numpy()
    if not np.array_equal(da, oa):
        t = int(np.argwhere((da != oa).reshape(T_, -1).any(1))[0, 0])
        key = key0
        for _ in range(t + 1):
            ks = oprng.split(key, 2)
            key, pk = ks[0], ks[1]
        ties = fr.pr.gumbel_near_ties(pk, otr["lp_all"][t].numpy())
        raise AssertionError(f"{what}: sampled actions differ, first at step {t} ({int((da[t] != oa[t]).sum())} samples; {ties} near-ties in that draw)")
    assert np.array_equal(tr["obs"][:T_].cpu().numpy(), otr["obs"].numpy().astype(np.float32)), what
    assert np.array_equal(tr["done"][:T_].cpu().numpy().astype(bool), otr["done"][:, :, 0].numpy()), what
    assert np.array_equal(tr["reward"].cpu().numpy(), otr["reward"].numpy()), what
    if tr["mask"] is not None:
        assert np.array_equal(tr["mask"][:T_].cpu().numpy().astype(bool), otr["mask"].numpy()), what
        assert bool(torch.gather(tr["mask"][:T_], -1, tr["action"].long().unsqueeze(-1)).all()), "an illegal action was sampled"
    compared = 0
    for f in dl.env.state_fields:     # env state bit-exact, where the oracle carries the field under the same name and shape
        a, b = getattr(dl.env, f).cpu().numpy(), np.asarray(ol.env_state.get(f, ()))
        if a.shape != b.shape:
            continue
        if a.dtype == np.int32 and b.dtype == np.uint32:    # PRNG keys
            a = a.view(np.uint32)
        assert np.array_equal(a, b), (what, f)
        compared += 1
    assert compared >= 2, f"{what}: no env state field compared"
    close(tr["value"], otr["value"], 1e-4, 1e-6, f"{what}: value")
    close(tr["log_prob"], otr["log_prob"], 1e-4, 1e-6, f"{what}: log_prob")
    close(dl.groups[0].last_val, ol.last_val, 1e-4, 1e-6, f"{what}: last_val")
    close(tr["adv"], otr["adv"], 1e-4, 2e-5, f"{what}: adv")
    close(tr["targets"], otr["targets"], 1e-4, 2e-5, f"{what}: targets")
    for k in ("episode_return", "episode_length"):
        assert np.array_equal(dl.metrics[k].cpu().numpy(), om[k]), (what, k)
    assert np.array_equal(dl.key, ol.key), what
    return om


def _sync_oracle(ol, dl):
    """The oracle takes over the device's parameters and Adam moments: each further step is compared from a common starting point; the
    drift up to there is bounded first."""
    for net, opt, p, o in ((dl.actor, dl.a_opt, ol.ap, ol.a_opt), (dl.critic, dl.c_opt, ol.cp, ol.c_opt)):
        drift = max((v.cpu() - p[n].reshape(v.shape)).abs().max().item() for n, v in net.named.items())
        assert drift <= 3e-5, f"parameter drift: {drift:.2e}"
        mn, nn = net.P.views(opt.mu), net.P.views(opt.nu)
        for n in p:
            p[n] = net.named[n].detach().cpu().reshape(p[n].shape).clone()
            o["mu"][n] = mn[n].detach().cpu().reshape(p[n].shape).clone()
            o["nu"][n] = nn[n].detach().cpu().reshape(p[n].shape).clone()


def _three_steps(case, steps=(1, 2, 3)):
    ol, cfg, info = fr.make_case(case)
    dl = _device_learner(cfg, info)
    N, ends, n_items = info["N"], case[-1], info["T"] * info["N"]
    ended = False
    for step in steps:
        what = f"{fr.case_id(case)} update step {step}"
        if step > 1:
            _sync_oracle(ol, dl)
        om = _rollout_parity(ol, dl, what)
        ended |= bool(om["is_terminal_step"].any())
        if step == 1:   # one minibatch: losses and gradients (hand-written backward against the restatement's autograd)
            ks = oprng.split(ol.key, 3)
            bp = oprng.permutation(ks[1], n_items)
            bpd = dl._permutation(ks[1], n_items)
            assert np.array_equal(bpd.cpu().numpy(), bp)
            ga, gc, oinfo, inter = ol.minibatch_grads(ol.make_minibatches(bp)[1])
            dl.minibatch_grads(bpd[n_items // 2:].contiguous())
            lo = dl.loss_out.cpu()     # [total, surrogate, entropy, value_loss]
            close(lo[0], torch.tensor(oinfo["total_loss"]), 1e-3, 2e-6, "total_loss")
            close(lo[1] - dl.sys.ent_coef * lo[2], torch.tensor(oinfo["actor_loss"]), 1e-3, 2e-6, "actor_loss (the actor's total)")
            close(lo[2], torch.tensor(oinfo["entropy"]), 1e-3, 2e-6, "entropy")
            close(lo[3], torch.tensor(oinfo["value_loss"]), 1e-3, 2e-6, "value_loss")
            close(dl.critic.b.t["t_value"].view(n_items // 2, info["A"]), inter["value"], 1e-4, 1e-6, "train value")   # rows are (item, agent) on both sides
            for net, gg in ((dl.actor, ga), (dl.critic, gc)):
                for n, g in net.named_grads.items():
                    scale = max(gg[n].abs().max().item(), 1e-6)
                    close(g / scale, gg[n].reshape(g.shape) / scale, 0, 2e-3, f"grad {n}")
        oinfos, _ = ol.update()
        losses = dl.update().cpu()
        dl._carry_over()
        assert np.array_equal(dl.key, ol.key)
        assert losses.shape == (fr.PARITY_EPOCHS, fr.PARITY_MINIBATCHES, 4)
        for net, p in ((dl.actor, ol.ap), (dl.critic, ol.cp)):
            for n, v in net.named.items():
                close(v, p[n].reshape(v.shape), 0, 3e-5, f"param {n} ({what})")
        for i, k in enumerate(fr.LOSS_NAMES):
            close(losses[0, 0, i], torch.tensor(oinfos[0][k]), 1e-3, 2e-6, f"logged {k}")
        assert dl.a_opt.count == dl.c_opt.count == ol.a_opt["count"] == 4 * step
    return dl, ended


@pytest.mark.parametrize("case", fr.PARITY_CASES, ids=fr.case_id)
def test_three_update_steps_against_the_restatement(case):
    dl, ended = _three_steps(case)
    assert ended == case[-1], "episode ends inside the rollouts: not what the case is for"
    assert dl.actor.tuning.ff_fused_step and dl.actor.fusable() and dl.critic.fusable()
    assert dl.groups[0].graph is not None, "the rollouts of steps 2 and 3 should have been a HIP-graph capture / replay"


@pytest.mark.parametrize("case", fr.LN_CASES, ids=fr.case_id)
def test_layer_norm_torso_trains_and_acts_on_the_composed_chain(case):
    """use_layer_norm: the kernel has no LayerNorm, so the acting step is the composed chain (no magpo_mlp_act_step launch), silently; the
    learner still matches the restatement."""
    from magpo_amd._lib import lib
    counts = {}
    dl, _ = _count_calls(lib(), counts, lambda: _three_steps(case, steps=(1, 2)))
    assert dl.actor.spec.use_layer_norm and not dl.actor.fusable() and dl.actor.tuning.ff_fused_step
    assert counts.get("magpo_mlp_act_step", 0) == 0 and counts.get("magpo_ln_act_fwd", 0) > 0 and counts.get("magpo_ln_act_bwd", 0) > 0


def _coordsum_learner(N=8, seed=4, num_groups=1, fused=True, use_graph=True, centralised=True, args=(3, 10, 5, 30), P=1, M=1):
    from magpo_amd.ff_ppo_learner import FfPpoLearner
    from magpo_amd.learner import CoordSumConfig, SystemConfig
    from magpo_amd.tuning import Tuning
    t = Tuning()
    t.ff_fused_step = fused
    l = FfPpoLearner(CoordSumConfig(*args), N, SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=M), DEV, centralised=centralised,
                     net_seed=seed, wgrad_groups=4, num_groups=num_groups, tuning=t)
    l.use_graph = use_graph
    return l


@pytest.mark.parametrize("centralised", [False, True], ids=["ippo", "mappo"])
def test_fused_acting_step_against_the_composed_one(centralised):
    """ff_fused_step on and off: the same actions over three rollouts, values and log-probs within 1e-4; T + 1 magpo_mlp_act_step launches per
    rollout on the fused path (T paired steps + the bootstrap value) and none on the composed one."""
    from magpo_amd.learner import host_split, prng_key
    key = host_split(prng_key(5), 3)[0]
    fused = _coordsum_learner(fused=True, use_graph=False, centralised=centralised)
    comp = _coordsum_learner(fused=False, use_graph=False, centralised=centralised)
    assert fused.actor.tuning.ff_fused_step and not comp.actor.tuning.ff_fused_step
    for l in (fused, comp):
        l.setup(key)
    for it in range(3):
        cf, cc = {}, {}
        _count_calls(fused.L, cf, fused.rollout)
        _count_calls(comp.L, cc, comp.rollout)
        assert cf.get("magpo_mlp_act_step", 0) == T + 1 and cc.get("magpo_mlp_act_step", 0) == 0, (cf, cc)
        assert cf.get("magpo_linear", 0) == 0 and cf.get("magpo_small_linear", 0) == 0 and cc.get("magpo_linear", 0) > 0
        assert torch.equal(fused.traj["action"], comp.traj["action"]), it
        close(fused.traj["value"], comp.traj["value"], 1e-4, 1e-6, "value")
        close(fused.traj["log_prob"], comp.traj["log_prob"], 1e-4, 1e-6, "log_prob")
        close(fused.groups[0].last_val, comp.groups[0].last_val, 1e-4, 1e-6, "last_val")
        assert float(fused.traj["value"].abs().max()) > 0
        for l in (fused, comp):
            l._carry_over()


@pytest.mark.parametrize("num_groups", [1, 2])
def test_graph_replay_equals_eager_rollout(num_groups):
    from magpo_amd.learner import host_split, prng_key
    key = host_split(prng_key(5), 3)[0]
    ls = [_coordsum_learner(num_groups=num_groups, use_graph=g) for g in (False, True)]
    for l in ls:
        l.setup(key, n_groups=num_groups)
    eager, graphed = ls
    for it in range(4):
        for l in ls:
            l.update_step()
        assert all(g.graph is not None for g in graphed.groups) or it < 1
        for gi, (ge, gg) in enumerate(zip(eager.groups, graphed.groups)):
            for k in ("action", "value", "log_prob", "reward", "adv"):
                assert torch.equal(ge.traj[k], gg.traj[k]), (it, gi, k)
            assert np.array_equal(ge.key, gg.key)
        assert torch.equal(eager.actor.P.flat, graphed.actor.P.flat) and torch.equal(eager.critic.P.flat, graphed.critic.P.flat), it
    assert bool(eager.groups[0].traj["done"].any())
    assert not any(g.graph_failed for g in graphed.groups) and all(g.graph is None for g in eager.groups)


def test_two_groups_share_parameters_and_average_gradients():
    """update_batch_size = 2: two env groups, one parameter set, gradient = mean over the groups (the pmean over "batch", ff_mappo.py:192-202)."""
    from magpo_amd.learner import host_split, prng_key
    key = host_split(prng_key(1), 3)[0]
    two = _coordsum_learner(N=4, seed=3, num_groups=2, args=(3, 10, 6, 30))
    two.setup(key, n_groups=2, group=0)
    singles = []
    for gi in range(2):
        s = _coordsum_learner(N=4, seed=3, args=(3, 10, 6, 30))
        s.setup(key, n_groups=2, group=gi)
        singles.append(s)
    two.rollout()
    for gi, s in enumerate(singles):
        s.rollout()
        assert torch.equal(s.traj["action"], two.groups[gi].traj["action"])
    assert not torch.equal(two.groups[0].traj["obs"], two.groups[1].traj["obs"])
    bp = two._permutation(host_split(two.key, 3)[1], T * 4)
    grads = []
    for s in singles:
        s.minibatch_grads(bp)
        grads.append(s.grad_all.clone())
    two.update()
    singles[0].grad_all.copy_(grads[0] + grads[1])
    singles[0].apply_grads(0.5)
    assert torch.allclose(two.actor.P.flat, singles[0].actor.P.flat, atol=2e-6)
    assert torch.allclose(two.critic.P.flat, singles[0].critic.P.flat, atol=2e-6)
    assert float((grads[0] + grads[1]).abs().max()) > 0


def _small_cfg(system, tmp_path, seed, extra=()):
    from magpo_amd.config import compose
    return compose(system, ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=6", "arch.num_evaluation=2", "arch.num_eval_episodes=6",
                            "system.total_timesteps=~", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=2",
                            "system.update_batch_size=2", "env.kwargs.time_limit=5", f"system.seed={seed}", "system.critic_lr=5e-4",
                            f"logger.base_exp_path={tmp_path}/", *extra])


def _system(name):
    from magpo_amd.systems.ppo.anakin import ff_ippo, ff_mappo
    return {"ff_ippo": ff_ippo, "ff_mappo": ff_mappo}[name]


def _setup(system, cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg, add_global_state=system == "ff_mappo")
    ks = host_split(prng_key(int(cfg.system.seed)), 4)
    learn, actor_network, state = _system(system).learner_setup(env, (ks[0], ks[2], ks[3]), cfg, torch.device(DEV))
    cfg = check_total_timesteps(cfg, 1)
    cfg.system.num_updates_per_eval = 1
    return learn, actor_network, state


def _flat(state):
    out = []
    for p in state.params:
        out += [p[k] for k in sorted(p)]
    for o in state.opt_states:
        out += [o["mu"], o["nu"]]
    out += [state.dones, state.timestep["agents_view"], state.timestep["step_count"], *[state.env_state[k] for k in sorted(state.env_state)]]
    return [t.detach().cpu() for t in out]


@pytest.mark.parametrize("system", ["ff_ippo", "ff_mappo"])
def test_learn_is_a_function_of_its_state_and_checkpoints_resume(system, tmp_path):
    from magpo_amd.ff_nets import FfActor
    from magpo_amd.systems.ppo.types import LearnerState
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    learn, actor_network, s0 = _setup(system, _small_cfg(system, tmp_path, 42))
    assert actor_network is learn.learner.actor and isinstance(actor_network, FfActor) and isinstance(s0, LearnerState)
    assert learn.learner.centralised == (system == "ff_mappo") and learn.learner.c_opt.sys.actor_lr == 5e-4 and learn.learner.a_opt.sys.actor_lr == 2.5e-4
    assert s0.dones.shape == (2, 6) and set(s0.params.actor_params) == {"pre.kernel", "pre.bias", "pre1.kernel", "pre1.bias", "head.kernel", "head.bias"}
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    ck = Checkpointer(system, base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == set(fr.LOSS_NAMES) and out3.train_metrics["entropy"].shape == (1, 2, 2)
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(system, _small_cfg(system, tmp_path, 7))
    assert not torch.equal(t0.params.actor_params["head.kernel"], s0.params.actor_params["head.kernel"])   # another seed, other parameters
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", system, "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, LearnerState)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key)
    assert r3.opt_states.critic_opt_state["count"] == s3.opt_states.critic_opt_state["count"] == 12
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
def test_eval_act_fn_on_the_trained_actor_equals_the_restated_one(greedy, tmp_path):
    """make_ff_eval_act_fn on the actor ff_mappo.learner_setup built and trained for one interval: the actions of one evaluator step equal the
    restatement's on the same timestep and key (mode, or one categorical sample over the whole batch); the actor state is {} in and out."""
    from magpo_amd.evaluator import make_ff_eval_act_fn
    from magpo_amd.ff_nets import FfActor
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg("ff_mappo", tmp_path, 11, ["arch.num_envs=4", "system.update_batch_size=1", f"arch.evaluation_greedy={greedy}"])
    learn, actor_network, state = _setup("ff_mappo", cfg)
    state = learn(state).learner_state
    env, eval_env = environments.make(cfg, add_global_state=True)
    eval_env.device = torch.device(DEV)
    A, K = env.num_agents, env.action_dim
    ap = {k: v.cpu().clone() for k, v in state.params.actor_params.items()}
    # a head with a visible spread (the trained one is still close to its orthogonal(0.01) start): neither the mode nor the sample is trivial
    ap["head.kernel"] = torch.randn(ap["head.kernel"].shape, generator=torch.Generator().manual_seed(5)) * 0.5
    from magpo_amd.learner import obs_row_stride
    eval_actor = FfActor(A, K, env.obs_dim, DEV, obs_ld=obs_row_stride(env.cfg.obs_dim), torso=actor_network.spec)
    act = make_ff_eval_act_fn(eval_actor, cfg)
    n = 5
    keys = torch.from_numpy(oprng.split(oprng.prng_key(23), n).view(np.int32).copy()).to(DEV)
    _, ts = eval_env.reset(keys)
    key = oprng.split(oprng.prng_key(29), 2)[1]
    action, actor_state = act({k: v.cuda() for k, v in ap.items()}, ts, key, {})
    assert actor_state == {} and action.shape == (n, A) and action.dtype == torch.int32
    obs = ts.observation.agents_view.cpu()[..., :env.obs_dim]
    mask = ts.observation.action_mask
    mask = torch.ones(n, A, K, dtype=torch.bool) if mask is None else mask.cpu().bool()
    lp = fr.actor_apply({k: v.double() for k, v in ap.items()}, obs.double(), mask, actor_network.spec)
    if greedy:
        top2 = torch.topk(lp, 2, dim=-1).values
        assert float((top2[..., 0] - top2[..., 1]).min()) > 1e-4, "the mode hangs on rounding: pick another key"
        want = lp.argmax(-1).numpy()
    else:
        assert fr.pr.gumbel_near_ties(key, lp.numpy()) == 0, "a draw hangs on rounding: pick another key"
        want = oprng.categorical(key, lp.to(torch.float32).numpy())
    assert np.array_equal(action.cpu().numpy(), want)
    assert len(np.unique(want)) > 1


@pytest.mark.parametrize("system", ["ff_ippo", "ff_mappo"])
def test_hydra_entry_point_trains_and_evaluates(system, tmp_path):
    perf = _system(system).hydra_entry_point(["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=8", "arch.num_evaluation=2", "arch.num_eval_episodes=8",
                                              "arch.absolute_metric=False", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=1",
                                              "env.kwargs.time_limit=6", f"logger.base_exp_path={tmp_path}/", "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", system)
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]


def test_get_learner_fn_calls_what_it_is_given_and_rejects_foreign_callables(tmp_path):
    import functools
    from magpo_amd.ff_nets import FfActor, FfCritic
    from magpo_amd.learner import host_split, obs_row_stride, prng_key
    from magpo_amd.optim import ClipAdam
    from magpo_amd.systems.ppo.anakin import ff_ippo, ff_ppo
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg("ff_ippo", tmp_path, 3, ["system.update_batch_size=1"])
    env, _ = environments.make(cfg)
    ld = obs_row_stride(env.cfg.obs_dim)
    actor = FfActor(env.num_agents, env.action_dim, env.obs_dim, DEV, obs_ld=ld, seed=1)
    critic = FfCritic(env.num_agents, env.obs_dim, DEV, obs_ld=ld, seed=2, tuning=actor.tuning)
    sysc = ff_ppo.system_config(cfg)
    a_opt, c_opt = ClipAdam(actor, sysc), ClipAdam(critic, sysc)
    calls = {"actor": 0, "critic": 0, "a_update": 0, "c_update": 0}

    def counted(fn, name):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    learn = ff_ippo.get_learner_fn(env, (counted(actor.apply, "actor"), counted(critic.apply, "critic")),
                                   (counted(a_opt.update, "a_update"), counted(c_opt.update, "c_update")), cfg)
    learn.learner.use_graph = False
    learn.learner.setup(host_split(prng_key(3), 3)[0])
    learn.learner.update_step()
    assert calls == {"actor": 4, "critic": 4, "a_update": 4, "c_update": 4}, calls
    good_a, good_u = (actor.apply, critic.apply), (a_opt.update, c_opt.update)
    for bad_apply, bad_update in (((lambda *a, **k: None, critic.apply), good_u), ((actor.apply, torch.relu), good_u),
                                  ((critic.apply, critic.apply), good_u), (good_a, (a_opt.update, lambda *a: None))):
        with pytest.raises(TypeError):
            ff_ippo.get_learner_fn(env, bad_apply, bad_update, cfg)
    with pytest.raises(ValueError):     # the optimisers of (actor, critic), in this order
        ff_ippo.get_learner_fn(env, good_a, (c_opt.update, a_opt.update), cfg)
