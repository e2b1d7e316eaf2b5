"""The recurrent PPO systems on the GPU (magpo_amd/ppo_learner.py, critic.py, systems/ppo/anakin) against their CPU restatement
(tests/ppo_ref.py) on identical seeds, parameters and PRNG keys, with the project's bars (tests/test_sable_learner_gpu.py): sampled actions
and env state bit-exact in every rollout, both carried hidden states, values and log-probs <= 1e-4, adv / targets 1e-4 / 2e-5, every
parameter gradient of both networks <= 2e-3 of the tensor's max, loss scalars 1e-3, parameters <= 3e-5 per update step.

Sampled actions are compared for exact equality: tests/test_ppo_system.py shows that the fp64 restatement has no Gumbel near-tie (top two
perturbed log-probs within 1e-4) at any of these seeds and shapes, so fp32 rounding cannot flip a draw; a mismatch reports whether the
recomputed noise puts it at a near-tie."""
import os

import numpy as np
import pytest
import torch

from oracle import coordsum as ocs
from oracle import evaluator as oeval
from oracle import prng as oprng
from tests import ppo_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


def _device_learner(cfg, info, **kw):
    from magpo_amd.learner import SystemConfig
    from magpo_amd.ppo_learner import PpoLearner
    sysc = SystemConfig(rollout_length=info["T"], ppo_epochs=pr.PARITY_EPOCHS, num_minibatches=pr.PARITY_MINIBATCHES, actor_lr=2.5e-4)
    ts = info["torso"]
    dl = PpoLearner(cfg, info["N"], sysc, DEV, centralised=info["centralised"], critic_lr=info["critic_lr"], net_seed=None, wgrad_groups=4,
                    actor_torso=(ts, ts), critic_torso=(ts, ts), **kw)
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
        ties = pr.gumbel_near_ties(pk, otr["lp_all"][t].numpy())
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
    g = dl.groups[0]
    close(g.policy_h[0], ol.policy_h, 1e-4, 1e-6, f"{what}: carried policy hidden state")
    close(g.critic_h[0], ol.critic_h, 1e-4, 1e-6, f"{what}: carried critic hidden state")
    close(g.policy_h0, ol.policy_h0, 1e-4, 1e-6, f"{what}: rollout-start policy hidden state")
    close(g.critic_h0, ol.critic_h0, 1e-4, 1e-6, f"{what}: rollout-start critic hidden state")
    close(tr["value"], otr["value"], 1e-4, 1e-6, f"{what}: value")
    close(tr["log_prob"], otr["log_prob"], 1e-4, 1e-6, f"{what}: log_prob")
    close(g.last_val, ol.last_val, 1e-4, 1e-6, f"{what}: last_val")
    close(tr["adv"], otr["adv"], 1e-4, 2e-5, f"{what}: adv")
    close(tr["targets"], otr["targets"], 1e-4, 2e-5, f"{what}: targets")
    for k in ("episode_return", "episode_length"):
        assert np.array_equal(dl.metrics[k].cpu().numpy(), om[k]), (what, k)
    assert np.array_equal(dl.key, ol.key), what
    return om


def _sync_oracle(ol, dl):
    """The oracle takes over the device's parameters and Adam moments: each further step is compared from a common starting point; the
    drift up to there is bounded first."""
    from magpo_amd.params import actor_named_views
    for net, opt, p, o in ((dl.actor, dl.a_opt, ol.ap, ol.a_opt), (dl.critic, dl.c_opt, ol.cp, ol.c_opt)):
        drift = max((v.cpu() - p[n].reshape(v.shape)).abs().max().item() for n, v in net.named.items())
        assert drift <= 3e-5, f"parameter drift: {drift:.2e}"
        mn, nn = actor_named_views(net.P.views(opt.mu)), actor_named_views(net.P.views(opt.nu))
        for n in p:
            p[n] = net.named[n].detach().cpu().reshape(p[n].shape).clone()
            o["mu"][n] = mn[n].detach().cpu().reshape(p[n].shape).clone()
            o["nu"][n] = nn[n].detach().cpu().reshape(p[n].shape).clone()


@pytest.mark.parametrize("case", pr.PARITY_CASES, ids=pr.case_id)
def test_three_update_steps_against_the_restatement(case):
    ol, cfg, info = pr.make_case(case)
    dl = _device_learner(cfg, info)
    N, ends = info["N"], case[-1]
    ended = False
    for step in (1, 2, 3):
        what = f"{pr.case_id(case)} update step {step}"
        if step > 1:
            _sync_oracle(ol, dl)
        om = _rollout_parity(ol, dl, what)
        ended |= bool(om["is_terminal_step"].any())
        if step > 1 and not ends:
            assert float(ol.policy_h0.abs().max()) > 0 and float(dl.groups[0].critic_h0.abs().max()) > 0, "rollout-start states must be non-zero"
        if step == 1:   # one minibatch: losses and gradients (hand-written backward against the restatement's autograd)
            ks = oprng.split(ol.key, 3)
            bp = oprng.permutation(ks[1], N)
            bpd = dl._permutation(ks[1], N)
            assert np.array_equal(bpd.cpu().numpy(), bp)
            ga, gc, oinfo, inter = ol.minibatch_grads(ol.make_minibatches(bp)[1])
            dl.minibatch_grads(bpd[N // 2:].contiguous())
            lo = dl.loss_out.cpu()     # [total, surrogate, entropy, value_loss]
            close(lo[0], torch.tensor(oinfo["total_loss"]), 1e-3, 2e-6, "total_loss")
            close(lo[1] - dl.sys.ent_coef * lo[2], torch.tensor(oinfo["actor_loss"]), 1e-3, 2e-6, "actor_loss (the actor's total)")
            close(lo[2], torch.tensor(oinfo["entropy"]), 1e-3, 2e-6, "entropy")
            close(lo[3], torch.tensor(oinfo["value_loss"]), 1e-3, 2e-6, "value_loss")
            # device rows are (sequence, t, agent); the restatement's fields are time-major (t, sequence, agent)
            mb, A = N // 2, info["A"]
            close(dl.critic.b.t["t_value"].view(mb, dl.T, A), inter["value"].transpose(0, 1), 1e-4, 1e-6, "train value")
            for net, gg in ((dl.actor, ga), (dl.critic, gc)):
                for n, g in net.named_grads.items():
                    scale = max(gg[n].abs().max().item(), 1e-6)
                    close(g / scale, gg[n].reshape(g.shape) / scale, 0, 2e-3, f"grad {n}")
        oinfos, _ = ol.update()
        losses = dl.update().cpu()
        dl._carry_over()
        assert np.array_equal(dl.key, ol.key)
        assert losses.shape == (pr.PARITY_EPOCHS, pr.PARITY_MINIBATCHES, 4)
        for net, p in ((dl.actor, ol.ap), (dl.critic, ol.cp)):
            for n, v in net.named.items():
                close(v, p[n].reshape(v.shape), 0, 3e-5, f"param {n} ({what})")
        for i, k in enumerate(pr.LOSS_NAMES):
            close(losses[0, 0, i], torch.tensor(oinfos[0][k]), 1e-3, 2e-6, f"logged {k}")
        assert dl.a_opt.count == dl.c_opt.count == ol.a_opt["count"] == 4 * step
    assert ended == ends, "episode ends inside the rollouts: not what the case is for"
    assert dl.groups[0].graph is not None, "the rollouts of steps 2 and 3 should have been a HIP-graph capture / replay"


def _coordsum_learner(N=8, seed=4, num_groups=1, fused=True, use_graph=True, centralised=True, args=(3, 10, 5, 30), P=1, M=1):
    from magpo_amd.learner import CoordSumConfig, SystemConfig
    from magpo_amd.ppo_learner import PpoLearner
    from magpo_amd.tuning import Tuning
    t = Tuning()
    t.ppo_fused_step = fused
    l = PpoLearner(CoordSumConfig(*args), N, SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=M), DEV, centralised=centralised,
                   net_seed=seed, wgrad_groups=4, num_groups=num_groups, tuning=t)
    l.use_graph = use_graph
    return l


def test_fused_acting_step_against_the_composed_one():
    """ppo_fused_step on and off: the same actions over three rollouts, hidden states within 1e-4 (two fp32 summation orders)."""
    from magpo_amd.learner import host_split, prng_key
    key = host_split(prng_key(5), 3)[0]
    fused, comp = _coordsum_learner(fused=True, use_graph=False), _coordsum_learner(fused=False, use_graph=False)
    assert fused.actor.tuning.ppo_fused_step and not comp.actor.tuning.ppo_fused_step
    calls = {"cell": 0}
    orig = fused.L.call

    def counting(name, *a):
        calls["cell"] += name == "magpo_gru_cell_step"
        return orig(name, *a)
    for l in (fused, comp):
        l.setup(key)
    for it in range(3):
        fused.L.call = counting
        try:
            fused.rollout()
        finally:
            del fused.L.call
        n_fused = calls["cell"]
        comp.L.call = counting
        try:
            comp.rollout()
        finally:
            del comp.L.call
        assert calls["cell"] == n_fused == (it + 1) * (T + 1), "T paired steps + the bootstrap critic step, and none on the composed path"
        assert torch.equal(fused.traj["action"], comp.traj["action"]), it
        for a, b in ((fused.groups[0].policy_h[0], comp.groups[0].policy_h[0]), (fused.groups[0].critic_h[0], comp.groups[0].critic_h[0])):
            close(a, b, 1e-4, 1e-6, "hidden state")
            assert float(a.abs().max()) > 0
        close(fused.traj["value"], comp.traj["value"], 1e-4, 1e-6, "value")
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
            assert torch.equal(ge.policy_h[0], gg.policy_h[0]) and torch.equal(ge.critic_h[0], gg.critic_h[0])
            assert np.array_equal(ge.key, gg.key)
        assert torch.equal(eager.actor.P.flat, graphed.actor.P.flat) and torch.equal(eager.critic.P.flat, graphed.critic.P.flat), it
    assert bool(eager.groups[0].traj["done"].any())
    assert not any(g.graph_failed for g in graphed.groups) and all(g.graph is None for g in eager.groups)


def test_two_groups_share_parameters_and_average_gradients():
    """update_batch_size = 2: two env groups, one parameter set, gradient = mean over the groups (the pmean over "batch", rec_mappo.py:252-262)."""
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
    bp = two._permutation(host_split(two.key, 3)[1], 4)
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
    from magpo_amd.systems.ppo.anakin import rec_ippo, rec_mappo
    return {"rec_ippo": rec_ippo, "rec_mappo": rec_mappo}[name]


def _setup(system, cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg, add_global_state=system == "rec_mappo")
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
    out += [*state.hstates, state.dones, state.timestep["agents_view"], state.timestep["step_count"], *[state.env_state[k] for k in sorted(state.env_state)]]
    return [t.detach().cpu() for t in out]


@pytest.mark.parametrize("system", ["rec_ippo", "rec_mappo"])
def test_learn_is_a_function_of_its_state_and_checkpoints_resume(system, tmp_path):
    from magpo_amd.systems.ppo.types import RNNLearnerState
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    learn, actor_network, s0 = _setup(system, _small_cfg(system, tmp_path, 42))
    assert actor_network is learn.learner.actor and isinstance(s0, RNNLearnerState)
    assert learn.learner.centralised == (system == "rec_mappo") and learn.learner.c_opt.sys.actor_lr == 5e-4 and learn.learner.a_opt.sys.actor_lr == 2.5e-4
    assert s0.hstates.critic_hidden_state.shape == (2, 18, 128) and s0.dones.shape == (2, 6)
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    ck = Checkpointer(system, base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == set(pr.LOSS_NAMES) and out3.train_metrics["entropy"].shape == (1, 2, 2)
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(system, _small_cfg(system, tmp_path, 7))
    assert not torch.equal(t0.params.actor_params["head.kernel"], s0.params.actor_params["head.kernel"])   # another seed, other parameters
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", system, "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, RNNLearnerState)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key)
    assert r3.opt_states.critic_opt_state["count"] == s3.opt_states.critic_opt_state["count"] == 12
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


def test_evaluator_on_the_trained_actor_equals_the_restated_one(tmp_path):
    """make_rec_eval_act_fn (as it is) on the actor rec_mappo.learner_setup built: per-episode arrays bit-equal to oracle.evaluator."""
    import warnings
    from magpo_amd.actor import GruActor
    from magpo_amd.evaluator import get_eval_fn, get_num_eval_envs, make_rec_eval_act_fn
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg("rec_mappo", tmp_path, 11, ["arch.num_envs=4", "arch.num_eval_episodes=8", "system.update_batch_size=1"])
    learn, actor_network, state = _setup("rec_mappo", cfg)
    env, eval_env = environments.make(cfg, add_global_state=True)
    A, K = env.num_agents, env.action_dim
    ap = {k: v.cpu().clone() for k, v in state.params.actor_params.items()}
    ap["head.kernel"] = ap["head.kernel"] * 60          # a head with a visible spread: sampling is not uniform
    eval_actor = GruActor(A, K, env.obs_dim, DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        evaluator = get_eval_fn(eval_env, make_rec_eval_act_fn(eval_actor, cfg), cfg, absolute_metric=False, device=DEV)
    n = get_num_eval_envs(cfg, False)
    key = oprng.split(oprng.prng_key(23), 3)[1]
    got = evaluator({k: v.cuda() for k, v in ap.items()}, key, {"hidden_state": torch.zeros(n * A, 128, device=DEV)})
    want = oeval.evaluate(ocs.CoordSumSpec(A, K, 5, env.cfg.maxval), ap, key, 4, 8)
    assert np.array_equal(got["episode_length"], want["episode_length"])
    assert np.array_equal(got["episode_return"], want["episode_return"]), (got["episode_return"], want["episode_return"])


@pytest.mark.parametrize("system", ["rec_ippo", "rec_mappo"])
def test_hydra_entry_point_trains_and_evaluates(system, tmp_path):
    perf = _system(system).hydra_entry_point(["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=8", "arch.num_evaluation=2", "arch.num_eval_episodes=8",
                                              "arch.absolute_metric=False", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=1",
                                              f"system.recurrent_chunk_size={T}", "env.kwargs.time_limit=6", f"logger.base_exp_path={tmp_path}/",
                                              "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", system)
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]
    with pytest.raises(NotImplementedError, match="interleaves"):
        _system(system).hydra_entry_point(["env=coordsum", "env/scenario=3x10-30", f"system.rollout_length={T}", "system.recurrent_chunk_size=4",
                                           f"logger.base_exp_path={tmp_path}/"])


def test_get_learner_fn_calls_what_it_is_given_and_rejects_foreign_callables(tmp_path):
    import functools
    from magpo_amd.actor import GruActor
    from magpo_amd.critic import GruCritic
    from magpo_amd.learner import host_split, obs_row_stride, prng_key
    from magpo_amd.optim import ClipAdam
    from magpo_amd.systems.ppo.anakin import rec_ippo, rec_ppo
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg("rec_ippo", tmp_path, 3, ["system.update_batch_size=1"])
    env, _ = environments.make(cfg)
    ld = obs_row_stride(env.cfg.obs_dim)
    actor = GruActor(env.num_agents, env.action_dim, env.obs_dim, DEV, obs_ld=ld, seed=1)
    critic = GruCritic(env.num_agents, env.obs_dim, DEV, obs_ld=ld, seed=2, tuning=actor.tuning)
    sysc = rec_ppo.system_config(cfg)
    a_opt, c_opt = ClipAdam(actor, sysc), ClipAdam(critic, sysc)
    calls = {"actor": 0, "critic": 0, "a_update": 0, "c_update": 0}

    def counted(fn, name):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    learn = rec_ippo.get_learner_fn(env, (counted(actor.apply, "actor"), counted(critic.apply, "critic")),
                                    (counted(a_opt.update, "a_update"), counted(c_opt.update, "c_update")), cfg)
    learn.learner.use_graph = False
    learn.learner.setup(host_split(prng_key(3), 3)[0])
    learn.learner.update_step()
    assert calls == {"actor": 4, "critic": 4, "a_update": 4, "c_update": 4}, calls
    good_a, good_u = (actor.apply, critic.apply), (a_opt.update, c_opt.update)
    for bad_apply, bad_update in (((lambda *a, **k: None, critic.apply), good_u), ((actor.apply, torch.relu), good_u),
                                  ((critic.apply, critic.apply), good_u), (good_a, (a_opt.update, lambda *a: None))):
        with pytest.raises(TypeError):
            rec_ippo.get_learner_fn(env, bad_apply, bad_update, cfg)
    with pytest.raises(ValueError):     # the optimisers of (actor, critic), in this order
        rec_ippo.get_learner_fn(env, good_a, (c_opt.update, a_opt.update), cfg)


def _tuned_rows():
    import csv
    return list(csv.DictReader(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_params.csv"))))


@pytest.mark.parametrize("row", range(8))
def test_tuned_rows_start_on_the_hip_path(row, tmp_path):
    """Every ippo / mappo row of tests/golden/ppo_params.csv with its tuned values (rollout_length 128 = recurrent_chunk_size, 64 envs, 8 epochs,
    the config's update_batch_size): set-up and one update step."""
    from magpo_amd.config import compose
    r = _tuned_rows()[row]
    system = "rec_" + r["system_name"]
    scen = {"3x10": "3x10-30", "3x30": "3x30-50", "5x20": "5x20-80", "8x15": "8x15-100"}[r["task"]]
    cfg = compose(system, ["env=coordsum", f"env/scenario={scen}", f"logger.base_exp_path={tmp_path}/"] + [
        f"system.{k}={r[k]}" for k in ("num_minibatches", "max_grad_norm", "ppo_epochs", "clip_eps", "recurrent_chunk_size", "ent_coef", "critic_lr",
                                       "actor_lr", "num_updates")] + [f"arch.num_envs={r['num_envs']}", f"arch.num_evaluation={r['num_evaluation']}"])
    learn, _, s0 = _setup(system, cfg)
    lr = learn.learner
    assert lr.T == 128 and lr.N == 64 and len(lr.groups) == 2 and lr.sys.ppo_epochs == 8 and lr.c_opt.sys.actor_lr == float(r["critic_lr"])
    out = learn(s0)
    tl = out.train_metrics["total_loss"]
    assert np.isfinite(tl).all() and tl.shape == (1, 8, int(r["num_minibatches"]))
