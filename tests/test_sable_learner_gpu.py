"""The guider-only Sable system on the GPU (magpo_amd/sable_learner.py, systems/sable/anakin/rec_sable.py) against its CPU restatement
(tests/sable_ref.py: SableOracleLearner, evaluate_sable) on identical seeds, parameters and PRNG keys, with the project's bars:
sampled actions and env state bit-exact in every rollout, values and log-probs <= 1e-4, every parameter gradient <= 2e-3 of the tensor's
max, parameters <= 3e-5 per update step."""
import os

import numpy as np
import pytest
import torch

from oracle import coordsum as ocs
from oracle import lbf as olbf
from oracle import learner as olearn
from oracle import networks as onets
from oracle import prng as oprng
from tests import sable_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


def _mk(env, args, N, nb=1, nh=1, E=64, P=2, M=2, seed=42, head_scale=1.0):
    """(oracle, device) learners of one case.  env "coordsum": args = (A, K, time_limit, maxval); "lbf": the LbfSpec arguments."""
    from magpo_amd.learner import CoordSumConfig, LbfConfig, SystemConfig
    from magpo_amd.sable_learner import SableLearner
    if env == "coordsum":
        spec, cfg, mod = ocs.CoordSumSpec(*args), CoordSumConfig(*args), ocs
        A, K, F = args[0], args[1], args[0] + 1
    else:
        spec, cfg, mod = olbf.LbfSpec(*args), LbfConfig(*args), olbf
        A, K, F = spec.num_agents, 6, spec.obs_dim
    scfg = onets.SableCfg(A, K, F, embed_dim=E, n_block=nb, n_head=nh)
    gp = onets.init_guider_params(1, E, F, K, nb=nb, nh=nh)
    gp["dec.head.dense1.kernel"] = gp["dec.head.dense1.kernel"] * head_scale   # (masked envs: logits with a visible spread)
    kw = dict(rollout_length=T, ppo_epochs=P, num_minibatches=M)
    ol = sr.SableOracleLearner(spec, N, olearn.SystemCfg(**kw), scfg, gp, env=mod)
    key = oprng.split(oprng.prng_key(seed), 3)[0]
    ol.setup(key)
    dl = SableLearner(cfg, N, SystemConfig(**kw), DEV, net_seed=None, wgrad_groups=4, n_block=nb, n_head=nh, embed_dim=E)
    dl.guider.load_named(gp)
    dl.setup(key)
    return ol, dl


def _state_parity(ol, dl, E, nh, what):
    """Carried retention states after a rollout against the oracle's (layout [N, nh, nb, hs, hs]), as tests/test_learner_gpu.py compares
    them: device head states sit in zero-padded 64 x 64 tiles, a net narrower than 64 carries every feature m = 64 / E times, the one
    128-wide head of 128 / 1 lives in four tiles (index 2 I + J)."""
    for d, o in zip(dl.sable_hs, ol.sable_hs):
        if E == 128 and nh == 1:
            full = torch.cat([torch.cat([d[:, 0], d[:, 1]], -1), torch.cat([d[:, 2], d[:, 3]], -1)], -2)   # [nb, N, 128, 128]
            close(full, o[:, 0].permute(1, 0, 2, 3), 1e-4, 1e-6, f"{what}: sable state (128-wide head)")
            continue
        hs, m = max(E, 64) // nh, max(1, 64 // E)
        close(d[:, :, :, :hs:m, :hs:m], o.permute(2, 1, 0, 3, 4), 1e-4, 1e-6, f"{what}: sable state")
        assert float(d[:, :, :, hs:, :].abs().max() if hs < 64 else 0.0) == 0.0, what


def _rollout_parity(ol, dl, what):
    om = ol.rollout()
    dl.rollout()
    tr, otr = dl.traj, ol.traj
    assert np.array_equal(tr["action"].cpu().numpy(), otr["action"].numpy()), f"{what}: sampled actions differ"
    assert np.array_equal(tr["obs"][:T].cpu().numpy(), otr["obs"].numpy().astype(np.float32)), what
    assert np.array_equal(tr["done"][:T].cpu().numpy().astype(bool), otr["done"][:, :, 0].numpy()), what
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
    """The oracle takes over the device's parameters and Adam moments (test_learner_gpu.py: each further step is compared from a common
    starting point; the drift up to there is bounded separately)."""
    from magpo_amd.params import guider_named_views
    drift = max((v.cpu() - ol.gp[n].reshape(v.shape)).abs().max().item() for n, v in dl.guider.named.items())
    assert drift <= 3e-5, f"parameter drift: {drift:.2e}"
    mn, nn = guider_named_views(dl.guider.P.views(dl.g_mu), E, nh), guider_named_views(dl.guider.P.views(dl.g_nu), E, nh)
    for n in ol.gp:
        ol.gp[n] = dl.guider.named[n].detach().cpu().reshape(ol.gp[n].shape).clone()
        ol.g_opt["mu"][n] = mn[n].detach().cpu().reshape(ol.gp[n].shape).clone()
        ol.g_opt["nu"][n] = nn[n].detach().cpu().reshape(ol.gp[n].shape).clone()


CASES = [  # env, args, N, nb, nh, E, episode end inside a rollout
    ("coordsum", (2, 10, 5, 15), 8, 1, 1, 64, True),
    ("coordsum", (3, 30, 6, 50), 6, 3, 2, 128, True),      # the tuned 3x30 row: 128 / 2 / 3
    ("coordsum", (4, 20, 5, 60), 4, 1, 1, 64, True),
    ("coordsum", (5, 20, 100, 80), 4, 1, 1, 64, False),    # no episode end in three rollouts: non-zero states carried across update steps
    ("lbf", (8, 8, 2, 2, 2, True, 6), 8, 1, 1, 64, True),
]


@pytest.mark.parametrize("env,args,N,nb,nh,E,ends", CASES, ids=[f"{c[0]}-A{c[1][0] if c[0] == 'coordsum' else c[1][2]}-{c[5]}.{c[4]}.{c[3]}{'' if c[6] else '-noend'}" for c in CASES])
def test_three_update_steps_against_the_oracle(env, args, N, nb, nh, E, ends):
    ol, dl = _mk(env, args, N, nb=nb, nh=nh, E=E, head_scale=30.0 if env == "lbf" else 1.0)
    ended = False
    for step in (1, 2, 3):
        what = f"update step {step}"
        if step > 1:
            _sync_oracle(ol, dl, E, nh)
        om = _rollout_parity(ol, dl, what)
        _state_parity(ol, dl, E, nh, what)
        ended |= bool(om["is_terminal_step"].any())
        if step > 1 and not ends:
            for o, d in zip(ol.prev_sable_hs, dl.groups[0].prev_sable_hs):
                assert float(o.abs().max()) > 0 and float(d.abs().max()) > 0, "rollout-start states must be non-zero"
        if step == 1:   # one minibatch: losses and gradients (hand-written backward against the oracle's autograd)
            ks = oprng.split(ol.key, 4)
            bp, apm = oprng.permutation(ks[1], N), oprng.permutation(ks[2], ol.spec.num_agents)
            bpd, apd = dl._permutation(ks[1], N), dl._permutation(ks[2], ol.spec.num_agents)
            assert np.array_equal(bpd.cpu().numpy(), bp) and np.array_equal(apd.cpu().numpy(), apm)
            gg, info, inter = ol.minibatch_grads(ol.make_minibatches(bp, apm)[1])
            dl.minibatch_grads(bpd[N // 2:].contiguous(), apd)
            lo = dl.loss_out.cpu()
            for i, k in enumerate(("total_loss", "actor_loss", "entropy", "value_loss")):
                close(lo[i], torch.tensor(info[k]), 1e-3, 2e-6, k)
            close(dl.guider.b.t["t_value"], inter["value"], 1e-4, 1e-6, "train value")
            for n, g in dl.guider.named_grads.items():
                scale = max(gg[n].abs().max().item(), 1e-6)
                close(g / scale, gg[n].reshape(g.shape) / scale, 0, 2e-3, f"grad {n}")
        oinfos = ol.update()
        losses = dl.update().cpu()
        dl._carry_over()
        assert np.array_equal(dl.key, ol.key)
        assert losses.shape == (2, 2, 4)
        for n, v in dl.guider.named.items():
            close(v, ol.gp[n].reshape(v.shape), 0, 3e-5, f"param {n} ({what})")
        close(losses[-1, -1, 3], torch.tensor(oinfos[-1]["value_loss"]), 5e-3, 1e-5, "final value loss")
        assert dl.g_count == ol.g_opt["count"] == 4 * step
    assert ended == ends, "episode ends inside the rollouts: not what the case is for"
    if not ends:
        assert all(float(h.abs().max()) > 0 for h in dl.sable_hs)
    assert dl.groups[0].graph is not None, "the rollouts of steps 2 and 3 should have been a HIP-graph capture / replay"
    assert dl.actor is None and dl.groups[0].policy_h is None


@pytest.mark.parametrize("num_groups", [1, 2])
def test_graph_replay_equals_eager_rollout(num_groups):
    from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key
    from magpo_amd.sable_learner import SableLearner
    sysc = SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=1)
    key = host_split(prng_key(5), 3)[0]
    ls = []
    for use_graph in (False, True):
        l = SableLearner(CoordSumConfig(3, 10, 5, 30), 8, sysc, DEV, net_seed=4, wgrad_groups=4, num_groups=num_groups)
        l.use_graph = use_graph
        l.setup(key, n_groups=num_groups)
        ls.append(l)
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
    """update_batch_size = 2: two env groups, one parameter set, gradient = mean over the groups (the pmean over "batch", rec_sable.py:242)."""
    from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key
    from magpo_amd.sable_learner import SableLearner
    sysc = SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=1)
    cfg = CoordSumConfig(3, 10, 6, 30)
    key = host_split(prng_key(1), 3)[0]
    two = SableLearner(cfg, 4, sysc, DEV, net_seed=3, wgrad_groups=4, num_groups=2)
    two.setup(key, n_groups=2, group=0)
    singles = []
    for gi in range(2):
        s = SableLearner(cfg, 4, sysc, DEV, net_seed=3, wgrad_groups=4)
        s.setup(key, n_groups=2, group=gi)
        singles.append(s)
    two.rollout()
    for gi, s in enumerate(singles):
        s.rollout()
        assert torch.equal(s.traj["action"], two.groups[gi].traj["action"])
    assert not torch.equal(two.groups[0].traj["obs"], two.groups[1].traj["obs"])
    ks = host_split(two.key, 4)
    bp, ap = two._permutation(ks[1], 4), two._permutation(ks[2], 3)
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


def test_micro_batches_give_the_update_of_one_pass():
    """system.micro_batches = 2: every minibatch in two slabs with accumulated gradients and the advantage statistics of the whole
    minibatch -- the update of micro_batches = 1 up to the fp32 summation order.  Bars: rollouts bit-equal (same parameters going in);
    after one update step (P x M = 4 Adam steps) parameters within 3e-5, the project's per-step bar; loss table within 1e-4 relative."""
    from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key
    from magpo_amd.sable_learner import SableLearner
    key = host_split(prng_key(9), 3)[0]
    ls = []
    for mu in (1, 2):
        l = SableLearner(CoordSumConfig(3, 10, 5, 30), 8, SystemConfig(rollout_length=T, ppo_epochs=2, num_minibatches=2, micro_batches=mu), DEV,
                         net_seed=6, wgrad_groups=4)
        l.setup(key)
        ls.append(l)
    one, two = ls
    p0 = one.guider.P.flat.clone()
    lo1, lo2 = one.update_step(), two.update_step()
    for k in ("action", "value", "log_prob", "adv"):
        assert torch.equal(one.traj[k], two.traj[k]), k
    assert bool(one.traj["done"].any()) and float(lo1.abs().max()) > 0
    close(lo2, lo1, 1e-4, 1e-6, "loss table")
    close(two.guider.P.flat, one.guider.P.flat, 0, 3e-5, "parameters")
    assert float((one.guider.P.flat - p0).abs().max()) > 1e-4, "the update must have moved the parameters"
    bad = SableLearner(CoordSumConfig(3, 10, 5, 30), 6, SystemConfig(rollout_length=T, num_minibatches=2, micro_batches=2), DEV, net_seed=6)
    bad.setup(key)
    with pytest.raises(ValueError):     # a minibatch of 3 envs in 2 slabs
        bad.update_step()


def _small_cfg(tmp_path, seed, extra=()):
    from magpo_amd.config import compose
    return compose("rec_sable", ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=6", "arch.num_evaluation=2", "arch.num_eval_episodes=6",
                                 "system.total_timesteps=~", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=2",
                                 "system.update_batch_size=2", "env.kwargs.time_limit=5", f"system.seed={seed}", f"logger.base_exp_path={tmp_path}/",
                                 *extra])


def _setup(cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.systems.sable.anakin import rec_sable
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg)
    ks = host_split(prng_key(int(cfg.system.seed)), 3)
    learn, execution_fn, state = rec_sable.learner_setup(env, (ks[0], ks[2]), cfg, torch.device(DEV))
    cfg = check_total_timesteps(cfg, 1)
    cfg.system.num_updates_per_eval = 1
    return learn, execution_fn, state


def _flat(state):
    out = [state.params[k] for k in sorted(state.params)] + [state.opt_states["mu"], state.opt_states["nu"], *state.hstates,
                                                             state.timestep["last"], state.timestep["agents_view"], state.timestep["step_count"],
                                                             *[state.env_state[k] for k in sorted(state.env_state)]]
    return [t.detach().cpu() for t in out]


def test_learn_is_a_function_of_its_state_and_checkpoints_resume(tmp_path):
    """State in, state out: an OLD state passed again gives the same successor, and a checkpoint restored into a learner set up from
    another seed continues bit-identically to the uninterrupted run."""
    from magpo_amd.systems.sable.types import LearnerState
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    learn, execution_fn, s0 = _setup(_small_cfg(tmp_path, 42))
    assert execution_fn.__self__ is learn.learner.guider and isinstance(s0, LearnerState)
    assert s0.hstates.encoder.shape == (2, 1, 1, 6, 64, 64) and s0.timestep["last"].shape == (2, 6)
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    ck = Checkpointer("rec_sable", base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == {"total_loss", "actor_loss", "entropy", "value_loss"} and out3.train_metrics["entropy"].shape == (1, 2, 2)
    assert float(s2.hstates.encoder.abs().max()) > 0
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(_small_cfg(tmp_path, 7))
    assert not torch.equal(_flat(t0)[0], _flat(s0)[0])
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", "rec_sable", "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, LearnerState)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key)
    assert r3.opt_states["count"] == s3.opt_states["count"] == 12
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


@pytest.mark.parametrize("scenario,TL,num_envs,episodes,nb,nh,E", [("3x10-30", 6, 4, 8, 1, 1, 64), ("3x30-50", 5, 3, 6, 3, 2, 128)])
def test_evaluator_with_the_sable_act_function(scenario, TL, num_envs, episodes, nb, nh, E):
    """get_eval_fn (as it is) with make_rec_sable_act_fn on the evaluator's own env batch: per-episode return and length arrays bit-equal
    to the restated evaluator over two episode loops.  evaluation_greedy is set and changes nothing: get_actions always samples."""
    import warnings
    from magpo_amd.config import compose
    from magpo_amd.evaluator import get_eval_fn, get_num_eval_envs
    from magpo_amd.sable import SableGuider
    from magpo_amd.systems.sable.anakin import rec_sable
    from magpo_amd.utils import make_env as environments
    cfg = compose("rec_sable", ["env=coordsum", f"env/scenario={scenario}", f"arch.num_envs={num_envs}", f"arch.num_eval_episodes={episodes}",
                                f"env.kwargs.time_limit={TL}", "arch.evaluation_greedy=True"])
    env, eval_env = environments.make(cfg)
    A, K = env.num_agents, env.action_dim
    gp = onets.init_guider_params(17, E, A + 1, K, nb=nb, nh=nh)
    gp["dec.head.dense1.kernel"] = gp["dec.head.dense1.kernel"] * 60     # a head with a visible spread: sampling is not uniform
    net = SableGuider(A, K, A + 1, DEV, embed_dim=E, n_head=nh, n_block=nb, max_pos=TL + 1)
    act_fn = rec_sable.make_rec_sable_act_fn(net.get_actions)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        evaluator = get_eval_fn(eval_env, act_fn, cfg, absolute_metric=False, device=DEV)
    n = get_num_eval_envs(cfg, False)
    assert episodes == 2 * n
    key = oprng.split(oprng.prng_key(23), 3)[1]
    init = {"hidden_state": rec_sable.get_init_hidden_state(net, n)}
    got = evaluator({k: v.cuda() for k, v in gp.items()}, key, init)
    assert float(init["hidden_state"].abs().max()) == 0, "the evaluator's initial state must stay untouched"
    spec = ocs.CoordSumSpec(A, K, TL, env.cfg.maxval)
    want = sr.evaluate_sable(spec, onets.SableCfg(A, K, A + 1, embed_dim=E, n_block=nb, n_head=nh), gp, key, num_envs, episodes)
    assert np.array_equal(got["episode_length"], want["episode_length"])
    assert np.array_equal(got["episode_return"], want["episode_return"]), (got["episode_return"], want["episode_return"])
    assert got["episode_return"].shape == (episodes,)
    with pytest.raises(TypeError):
        rec_sable.make_rec_sable_act_fn(lambda *a, **k: None)


def test_hydra_entry_point_trains_and_evaluates(tmp_path):
    from magpo_amd.systems.sable.anakin import rec_sable
    perf = rec_sable.hydra_entry_point(["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=8", "arch.num_evaluation=2", "arch.num_eval_episodes=8",
                                        "arch.absolute_metric=False", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=1",
                                        "env.kwargs.time_limit=6", f"logger.base_exp_path={tmp_path}/", "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", "rec_sable")
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]


def test_get_learner_fn_calls_what_it_is_given_and_rejects_foreign_callables(tmp_path):
    import functools
    from magpo_amd.optim import ClipAdam
    from magpo_amd.sable import SableGuider
    from magpo_amd.systems.sable.anakin import rec_sable
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg(tmp_path, 3, ["system.update_batch_size=1"])
    env, _ = environments.make(cfg)
    net = SableGuider(env.num_agents, env.action_dim, env.obs_dim, DEV, max_pos=env.cfg.time_limit + 1, seed=1)
    opt = ClipAdam(net, rec_sable.system_config(cfg))
    calls = {"act": 0, "apply": 0, "update": 0}

    def counted(fn, name):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper
    learn = rec_sable.get_learner_fn(env, (counted(net.get_actions, "act"), counted(net.apply, "apply")), counted(opt.update, "update"), cfg)
    learn.learner.use_graph = False
    from magpo_amd.learner import host_split, prng_key
    learn.learner.setup(host_split(prng_key(3), 3)[0])
    learn.learner.update_step()
    assert calls == {"act": T + 1, "apply": 4, "update": 4}, calls
    for bad_apply, bad_update in (((lambda *a, **k: None, net.apply), opt.update), ((net.get_actions, torch.relu), opt.update),
                                  ((net.get_actions, net.apply), lambda *a: None)):
        with pytest.raises(TypeError):
            rec_sable.get_learner_fn(env, bad_apply, bad_update, cfg)
    other = SableGuider(env.num_agents, env.action_dim, env.obs_dim, DEV, max_pos=env.cfg.time_limit + 1, seed=2)
    with pytest.raises(ValueError):
        rec_sable.get_learner_fn(env, (other.get_actions, net.apply), opt.update, cfg)
