"""The memoryless Sable system on the GPU (magpo_amd/ff_sable_learner.py, systems/sable/anakin/ff_sable.py) against its CPU restatement
(tests/ff_sable_ref.py: FfSableOracleLearner) on identical seeds, parameters and PRNG keys, in the manner and with the bars of
tests/test_sable_learner_gpu.py / test_ff_ppo_learner_gpu.py: sampled actions, observations, dones, rewards, env state and keys bit-exact in
every rollout, values and log-probs <= 1e-4, every parameter gradient <= 2e-3 of the tensor's max, parameters <= 3e-5 per update step.
tests/test_ff_sable_system.py shows that none of the seeds used here has a Gumbel near-tie."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import prng as oprng
from tests import ff_sable_ref as fs
from tests.gpu_util import _count_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8
HERE = os.path.dirname(os.path.abspath(__file__))


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


def _mk(case):
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.learner import SystemConfig
    ol, cfg, info = fs.make_case(case)
    sysc = SystemConfig(rollout_length=info["T"], ppo_epochs=fs.PARITY_EPOCHS, num_minibatches=fs.PARITY_MINIBATCHES)
    dl = FfSableLearner(cfg, info["N"], sysc, DEV, net_seed=None, wgrad_groups=4, n_block=info["nb"], n_head=info["nh"], embed_dim=info["E"])
    dl.guider.load_named(info["gp"])
    dl.setup(info["key"])
    return ol, dl, info


def _rollout_parity(ol, dl, what):
    om = ol.rollout()
    dl.rollout()
    tr, otr = dl.traj, ol.traj
    assert np.array_equal(tr["action"].cpu().numpy(), otr["action"].numpy()), f"{what}: sampled actions differ"
    assert np.array_equal(tr["obs"][:T].cpu().numpy(), otr["obs"].numpy().astype(np.float32)), what
    # done = timestep.last() of the step itself (ff_sable.py:103): slot t + 1 of the device's flags
    assert np.array_equal(tr["done"][1:T + 1].cpu().numpy().astype(bool), otr["done"][:, :, 0].numpy()), what
    assert np.array_equal(tr["reward"].cpu().numpy(), otr["reward"].numpy()), what
    assert np.array_equal(tr["step_count"][:T].cpu().numpy(), otr["step_count"][:, :, 0].numpy()), what
    if tr["mask"] is not None:
        assert np.array_equal(tr["mask"][:T].cpu().numpy().astype(bool), otr["mask"].numpy()), what
        assert bool(torch.gather(tr["mask"][:T], -1, tr["action"].long().unsqueeze(-1)).all()), "an illegal action was sampled"
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
    close(dl.last_val, ol.last_val, 1e-4, 1e-6, f"{what}: last_val")
    close(tr["adv"], otr["adv"], 1e-4, 2e-5, f"{what}: adv")
    close(tr["targets"], otr["targets"], 1e-4, 2e-5, f"{what}: targets")
    for k in ("episode_return", "episode_length"):
        assert np.array_equal(dl.metrics[k].cpu().numpy(), om[k]), (what, k)
    assert np.array_equal(dl.key, ol.key), what
    return om


def _sync_oracle(ol, dl, E, nh):
    """The oracle takes over the device's parameters and Adam moments (each further step is compared from a common starting point; the
    drift up to there is bounded separately)."""
    from magpo_amd.params import guider_named_views
    drift = max((v.cpu() - ol.gp[n].reshape(v.shape)).abs().max().item() for n, v in dl.guider.named.items())
    assert drift <= 3e-5, f"parameter drift: {drift:.2e}"
    mn, nn = guider_named_views(dl.guider.P.views(dl.g_opt.mu), E, nh), guider_named_views(dl.guider.P.views(dl.g_opt.nu), E, nh)
    for n in ol.gp:
        ol.gp[n] = dl.guider.named[n].detach().cpu().reshape(ol.gp[n].shape).clone()
        ol.g_opt["mu"][n] = mn[n].detach().cpu().reshape(ol.gp[n].shape).clone()
        ol.g_opt["nu"][n] = nn[n].detach().cpu().reshape(ol.gp[n].shape).clone()


@pytest.mark.parametrize("case", fs.PARITY_CASES, ids=fs.case_id)
def test_three_update_steps_against_the_restatement(case):
    from magpo_amd._lib import lib
    ol, dl, info = _mk(case)
    N, A, E, nh, ends = info["N"], info["A"], info["E"], info["nh"], case[-1]
    ended = False
    counts = {}
    for step in (1, 2, 3):
        what = f"update step {step}"
        if step > 1:
            _sync_oracle(ol, dl, E, nh)
        om = _count_calls(lib(), counts, lambda: _rollout_parity(ol, dl, what)) if step == 1 else _rollout_parity(ol, dl, what)
        ended |= bool(om["is_terminal_step"].any())
        if step == 1:   # one minibatch: losses and gradients (hand-written backward against the restatement's autograd)
            ks = oprng.split(ol.key, 4)
            bp, apm = oprng.permutation(ks[1], T * N), oprng.permutation(ks[2], A)
            bpd, apd = dl._permutation(ks[1], T * N), dl._permutation(ks[2], A)
            assert np.array_equal(bpd.cpu().numpy(), bp) and np.array_equal(apd.cpu().numpy(), apm)
            gg, oinfo, inter = ol.minibatch_grads(ol.make_minibatches(bp, apm)[1])
            _count_calls(lib(), counts, lambda: dl.minibatch_grads(bpd[T * N // 2:].contiguous(), apd))
            lo = dl.loss_out.cpu()
            for i, k in enumerate(("total_loss", "actor_loss", "entropy", "value_loss")):
                close(lo[i], torch.tensor(oinfo[k]), 1e-3, 2e-6, k)
            close(dl.guider.b.t["t_value"], inter["value"], 1e-4, 1e-6, "train value")
            for n, g in dl.guider.named_grads.items():
                scale = max(gg[n].abs().max().item(), 1e-6)
                close(g / scale, gg[n].reshape(g.shape) / scale, 0, 2e-3, f"grad {n}")
        oinfos, _ = ol.update()
        losses = dl.update().cpu()
        dl._carry_over()
        assert np.array_equal(dl.key, ol.key)
        assert losses.shape == (2, 2, 4)
        for n, v in dl.guider.named.items():
            close(v, ol.gp[n].reshape(v.shape), 0, 3e-5, f"param {n} ({what})")
        close(losses[-1, -1, 3], torch.tensor(oinfos[-1]["value_loss"]), 5e-3, 1e-5, "final value loss")
        assert dl.g_opt.count == ol.g_opt["count"] == 4 * step
    assert ended == ends, "episode ends inside the rollouts: not what the case is for"
    assert dl.groups[0].graph is not None, "the rollouts of steps 2 and 3 should have been a HIP-graph capture / replay"
    # stateless: the team kernels and none of the state-carrying retention entry points; no chunk-entry state buffer was ever allocated
    assert counts.get("magpo_team_retention_fwd", 0) > 0 and counts.get("magpo_team_retention_bwd", 0) > 0
    for n in ("retention_chunk_fwd", "retention_chunk_bwd", "retention_recurrent", "zero_states_where_done", "sable_act"):
        assert counts.get("magpo_" + n, 0) == 0, (n, counts)
    assert not [k for k in dl.guider.b.t if k.startswith("t_st_")]
    assert float(dl.guider.pe.abs().max()) == 0.0 and dl.guider.kappas == [1.0] * nh
    with pytest.raises(NotImplementedError):
        dl.guider.act_fused(None, None, None, None, None, None, None)


def _coordsum_learner(N=8, seed=4, num_groups=1, use_graph=True, args=(3, 10, 5, 30), P=1, M=1, **kw):
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.learner import CoordSumConfig, SystemConfig
    l = FfSableLearner(CoordSumConfig(*args), N, SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=M), DEV, net_seed=seed, wgrad_groups=4,
                       num_groups=num_groups, **kw)
    l.use_graph = use_graph
    return l


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
        assert torch.equal(eager.guider.P.flat, graphed.guider.P.flat), it
    assert bool(eager.groups[0].traj["done"].any())
    assert not any(g.graph_failed for g in graphed.groups) and all(g.graph is None for g in eager.groups)


def test_two_groups_share_parameters_and_average_gradients():
    """update_batch_size = 2: two env groups, one parameter set, gradient = mean over the groups (the pmean over "batch", ff_sable.py:226)."""
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
    ks = host_split(two.key, 4)
    bp, ap = two._permutation(ks[1], T * 4), two._permutation(ks[2], 3)
    grads = []
    for s in singles:
        s.minibatch_grads(bp, ap)
        grads.append(s.grad_all.clone())
    losses = two.update()
    singles[0].grad_all.copy_(grads[0] + grads[1])
    singles[0].apply_grads(0.5)
    assert torch.allclose(two.guider.P.flat, singles[0].guider.P.flat, atol=2e-6)
    assert torch.allclose(losses[0, 0], ((grads[0] + grads[1]) / 2)[-16:-12], rtol=1e-4, atol=1e-6)   # the loss scalars ride behind the gradients
    assert float((grads[0] + grads[1]).abs().max()) > 0


def test_micro_batches_raise():
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.learner import CoordSumConfig, SystemConfig
    with pytest.raises(NotImplementedError, match="micro_batches"):
        FfSableLearner(CoordSumConfig(3, 10, 5, 30), 8, SystemConfig(rollout_length=T, micro_batches=2), DEV)


def _small_cfg(tmp_path, seed, extra=()):
    from magpo_amd.config import compose
    return compose("ff_sable", ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=6", "arch.num_evaluation=2", "arch.num_eval_episodes=6",
                                "system.total_timesteps=~", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=2",
                                "system.update_batch_size=2", "env.kwargs.time_limit=5", f"system.seed={seed}", f"logger.base_exp_path={tmp_path}/",
                                *extra])


def _setup(cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.systems.sable.anakin import ff_sable
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg)
    ks = host_split(prng_key(int(cfg.system.seed)), 3)
    learn, execution_fn, state = ff_sable.learner_setup(env, (ks[0], ks[2]), cfg, torch.device(DEV))
    cfg = check_total_timesteps(cfg, 1)
    cfg.system.num_updates_per_eval = 1
    return learn, execution_fn, state


def _flat(state):
    out = [state.params[k] for k in sorted(state.params)] + [state.opt_states["mu"], state.opt_states["nu"], state.timestep["last"],
                                                             state.timestep["agents_view"], state.timestep["step_count"],
                                                             *[state.env_state[k] for k in sorted(state.env_state)]]
    return [t.detach().cpu() for t in out]


def test_learn_is_a_function_of_its_state_and_checkpoints_resume(tmp_path):
    """State in, state out: an OLD state passed again gives the same successor, and a checkpoint restored into a learner set up from
    another seed continues bit-identically to the uninterrupted run.  The state has no hidden states."""
    from magpo_amd.systems.sable.types import FFLearnerState
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    cfg = _small_cfg(tmp_path, 42)
    learn, execution_fn, s0 = _setup(cfg)
    mc = cfg.network.memory_config
    assert mc.decay_scaling_factor == 1.0 and mc.chunk_size == 3 and mc.timestep_positional_encoding is False
    assert execution_fn.__self__ is learn.learner.guider and execution_fn.__name__ == "act" and isinstance(s0, FFLearnerState)
    assert s0._fields == ("params", "opt_states", "key", "env_state", "timestep") and s0.timestep["last"].shape == (2, 6)
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    ck = Checkpointer("ff_sable", base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == {"total_loss", "actor_loss", "entropy", "value_loss"} and out3.train_metrics["entropy"].shape == (1, 2, 2)
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(_small_cfg(tmp_path, 7))
    assert not torch.equal(_flat(t0)[0], _flat(s0)[0])
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", "ff_sable", "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, FFLearnerState)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key)
    assert r3.opt_states["count"] == s3.opt_states["count"] == 12
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


def test_eval_act_fn_equals_the_restated_network():
    """make_ff_sable_eval_act_fn: the actions of one evaluator step equal sable_get_actions of the restatement on zero states with the
    same timestep and key; the actor state is {} in and out."""
    from magpo_amd.config import compose
    from magpo_amd.sable import SableGuider
    from magpo_amd.systems.sable.anakin import ff_sable
    from magpo_amd.utils import make_env as environments
    from oracle import networks as onets
    cfg = compose("ff_sable", ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=4", "env.kwargs.time_limit=6"])
    env, eval_env = environments.make(cfg)
    eval_env.device = torch.device(DEV)
    A, K = env.num_agents, env.action_dim
    gp = onets.init_guider_params(17, 64, A + 1, K)
    gp["dec.head.dense1.kernel"] = gp["dec.head.dense1.kernel"] * 60     # a head with a visible spread: sampling is not uniform
    net = SableGuider(A, K, A + 1, DEV, memory_type="ff_sable", max_pos=7)
    act = ff_sable.make_ff_sable_eval_act_fn(net.act)
    n = 5
    keys = torch.from_numpy(oprng.split(oprng.prng_key(23), n).view(np.int32).copy()).to(DEV)
    _, ts = eval_env.reset(keys)
    key = oprng.split(oprng.prng_key(29), 2)[1]
    action, actor_state = act({k: v.cuda() for k, v in gp.items()}, ts, key, {})
    assert actor_state == {} and action.shape == (n, A) and action.dtype == torch.int32
    ob = ts.observation
    scfg = fs.ff_cfg(A, K, A + 1)
    p64 = {k: v.double() for k, v in gp.items()}
    obs = ob.agents_view.cpu()[..., :A + 1]
    mask = torch.ones(n, A, K, dtype=torch.bool) if ob.action_mask is None else ob.action_mask.cpu().bool()
    sc = ob.step_count.cpu()
    sc = sc if sc.dim() == 2 else sc[:, None].expand(n, A)
    want, _, _, _, lp = onets.sable_get_actions(p64, scfg, obs.double(), mask, sc, onets.init_sable_hstates(n, scfg, torch.float64), key)
    # a draw of agent i + 1 depends on the action of agent i, so the near-tie count is taken along the fp64 trajectory
    assert fs.gumbel_near_ties(key, lp.numpy()) == 0, "a draw hangs on rounding: pick another key"
    assert np.array_equal(action.cpu().numpy(), want.numpy())
    assert len(np.unique(want.numpy())) > 1
    with pytest.raises(TypeError):
        ff_sable.make_ff_sable_eval_act_fn(lambda *a, **k: None)
    with pytest.raises(ValueError):
        ff_sable.make_ff_sable_eval_act_fn(SableGuider(A, K, A + 1, DEV, max_pos=7).act)


def test_hydra_entry_point_trains_and_evaluates(tmp_path):
    from magpo_amd.systems.sable.anakin import ff_sable
    perf = ff_sable.hydra_entry_point(["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=8", "arch.num_evaluation=2", "arch.num_eval_episodes=8",
                                       "arch.absolute_metric=False", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=1",
                                       "env.kwargs.time_limit=6", f"logger.base_exp_path={tmp_path}/", "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", "ff_sable")
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]


def test_get_learner_fn_calls_what_it_is_given_and_rejects_foreign_callables(tmp_path):
    import functools
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.optim import ClipAdam
    from magpo_amd.sable import SableGuider
    from magpo_amd.systems.sable.anakin import ff_sable
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg(tmp_path, 3, ["system.update_batch_size=1"])
    env, _ = environments.make(cfg)
    net = SableGuider(env.num_agents, env.action_dim, env.obs_dim, DEV, memory_type="ff_sable", max_pos=env.cfg.time_limit + 1, seed=1)
    opt = ClipAdam(net, ff_sable.system_config(cfg))
    calls = {"act": 0, "apply": 0, "update": 0}

    def counted(fn, name):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    learn = ff_sable.get_learner_fn(env, (counted(net.act, "act"), counted(net.apply, "apply")), counted(opt.update, "update"), cfg)
    learn.learner.use_graph = False
    learn.learner.setup(host_split(prng_key(3), 3)[0])
    learn.learner.update_step()
    assert calls == {"act": T + 1, "apply": 4, "update": 4}, calls
    for bad_apply, bad_update in (((lambda *a, **k: None, net.apply), opt.update), ((net.act, torch.relu), opt.update),
                                  ((net.get_actions, net.apply), opt.update), ((net.act, net.apply), lambda *a: None)):
        with pytest.raises(TypeError):
            ff_sable.get_learner_fn(env, bad_apply, bad_update, cfg)
    rec = SableGuider(env.num_agents, env.action_dim, env.obs_dim, DEV, max_pos=env.cfg.time_limit + 1, seed=2)
    with pytest.raises(ValueError):     # a recurrent network: the learner refuses it
        ff_sable.get_learner_fn(env, (rec.act, rec.apply), ClipAdam(rec, ff_sable.system_config(cfg)).update, cfg)


# ------------------------------------------------------------------------------------------------ rec_sable is untouched
REC_CASES = {"64.1.1": dict(args=(3, 10, 5, 30), N=8, nb=1, nh=1, E=64), "128.1.1": dict(args=(3, 10, 5, 30), N=8, nb=1, nh=1, E=128),
             "64.2.2": dict(args=(4, 20, 5, 60), N=8, nb=2, nh=2, E=64)}


def rec_sable_call_counts(name):
    """ABI calls, by name, of one eager update step (T = 8, 1 epoch x 2 minibatches) of a rec_sable learner of REC_CASES[name]."""
    from magpo_amd._lib import lib
    from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key
    from magpo_amd.sable_learner import SableLearner
    c = REC_CASES[name]
    l = SableLearner(CoordSumConfig(*c["args"]), c["N"], SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=2), DEV, net_seed=4, wgrad_groups=4,
                     n_block=c["nb"], n_head=c["nh"], embed_dim=c["E"])
    l.use_graph = False
    l.setup(host_split(prng_key(5), 3)[0])
    counts = {}
    _count_calls(lib(), counts, l.update_step)
    torch.cuda.synchronize()
    return counts


@pytest.mark.parametrize("name", sorted(REC_CASES))
def test_rec_sable_makes_the_abi_calls_of_the_parent_commit(name):
    """A rec_sable learner built beside an ff_sable one (which has run first) makes exactly the ABI calls, by name and count, that the
    commit before ff_sable made for the same update step: tests/golden/rec_sable_abi_calls.json was recorded there with this function."""
    ff = _coordsum_learner(N=8, P=1, M=2, embed_dim=REC_CASES[name]["E"])
    ff.setup(oprng.split(oprng.prng_key(5), 3)[0])
    ff.update_step()
    want = json.load(open(os.path.join(HERE, "golden", "rec_sable_abi_calls.json")))[name]
    got = rec_sable_call_counts(name)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    assert not [k for k in got if "team_retention" in k]
