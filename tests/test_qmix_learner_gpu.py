"""rec_qmix on the GPU (magpo_amd/qmix_learner.py) against its restatement (tests/qmix_ref.py) over enough update steps that the ring wraps and
episodes end inside sampled windows: actions, env state, ring contents and sampled indices bit for bit; Q values, both gradient sets, loss
scalars and all four parameter sets within the tolerances of tests/test_q_learner_gpu.py.  tests/test_qmix_system.py shows that the fp64
restatement has no near tie at these seeds, so fp32 rounding cannot flip an index."""
import os

import numpy as np
import pytest
import torch

from tests import iql_ref
from tests import qmix_ref as ref
from tests.test_q_learner_gpu import ENV_FIELDS, _close, _ring_equal

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_learner(cfg, info, num_groups, use_graph=True):
    from magpo_amd.qmix_learner import QmixLearner
    dl = QmixLearner(cfg, info["N"], info["sys"], DEV, embed_dim=info["E"], net_seed=None, wgrad_groups=4, num_groups=num_groups)
    dl.use_graph = use_graph
    dl.q_net.load_named(info["params"])
    dl.mixer.load_named(info["mixer_params"])
    dl.sync_target()
    dl.setup(info["key"], n_groups=num_groups)
    return dl


@pytest.mark.parametrize("variant", list(iql_ref.PARITY_VARIANTS))
@pytest.mark.parametrize("case", iql_ref.PARITY_CASES, ids=[c[0] for c in iql_ref.PARITY_CASES])
def test_qmix_learner_matches_restatement(case, variant):
    ol, cfg, info = ref.parity_case(case, variant)
    U, T, K, A = ol.U, info["sys"].rollout_length, info["K"], info["A"]
    dl = _device_learner(cfg, info, U)
    assert dl.q_opt.eps == dl.mix_opt.eps == 1e-8 and dl.q_opt.max_norm == dl.mix_opt.max_norm == float("inf")
    skipped = trained = ends = 0
    for step in range(iql_ref.PARITY_STEPS):
        n_log = len(ol.log)
        metrics, infos = ol.update_step()
        losses = dl.update_step().cpu().numpy()
        tag = (case[0], variant, step)
        for u, (g, og) in enumerate(zip(dl.groups, ol.groups)):
            acts = np.stack([e["action"] for e in ol.log[n_log + u * T: n_log + (u + 1) * T]])
            assert np.array_equal(g.traj["action"].cpu().numpy(), acts), (tag, "actions")
            for dev_f, ora_f in ENV_FIELDS[case[0]]:
                got = getattr(g.env, dev_f).cpu().numpy()
                assert np.array_equal(got.view(np.uint32) if dev_f == "key" else got, og.env_state[ora_f]), (tag, dev_f)
            assert np.array_equal(g.traj["obs"][0].cpu().numpy(), og.timestep["observation"]["agents_view"].astype(np.float32)), tag
            assert np.array_equal(g.term[0].cpu().numpy().astype(bool), og.terminal) and np.array_equal(g.traj["done"][0].cpu().numpy().astype(bool), og.tot)
            assert np.array_equal(g.key, og.key) and np.array_equal(g.train_key, og.train_key), tag
            _ring_equal(g, og, tag)      # (the reward ring holds the team mean in every agent column, bit for bit)
            _close(g.h[0], og.hidden.reshape(-1, 128), 1e-4, f"{tag} hidden state")
            ends += int(metrics[u]["is_terminal_step"].sum())
        for e, info_e in enumerate(infos):
            if info_e is None:      # the skipped-training phase: zero loss rows, no optimiser step, t_train stays
                skipped += 1
                assert not losses[e].any() and dl.t_train == 0 and dl.q_opt.count == 0 and dl.mix_opt.count == 0
                continue
            trained += 1
            for i, name in enumerate(ref.LOSS_NAMES):
                print(f"CHECK {tag} epoch {e} {name}: got {losses[e, 0, i]:.6f} want {info_e[name]:.6f}")
                assert abs(losses[e, 0, i] - info_e[name]) <= 1e-3, (tag, name, losses[e, 0, i], info_e[name])
        assert dl.t_train == ol.t_train == int(dl.t_train_dev) == dl.q_opt.count == dl.mix_opt.count
        if infos[-1] is not None:
            last = ol.train_log[-1]
            for u in range(U):
                assert np.array_equal(dl._idx_host[u, 0], last["idx"][u][0]) and np.array_equal(dl._idx_host[u, 1], last["idx"][u][1]), (tag, "sampled indices")
            m = dl._mb
            q_ref = torch.cat([d["q"].transpose(0, 1).reshape(-1, K) for d in last["details"]])       # (L, B, A, K) -> rows (b, t, a)
            _close(dl.q_net.b.t["t_logits"][:, :K], q_ref, 1e-4, f"{tag} online Q values")
            _close(m["q_tot"], torch.cat([d["q_tot"].reshape(-1) for d in last["details"]]), 1e-4, f"{tag} q_tot")
            _close(m["next_q_tot"], torch.cat([d["next_q_tot"].reshape(-1) for d in last["details"]]), 1e-4, f"{tag} next q_tot")
            for net, want_g, what in ((dl.q_net, last["grads"], "grad"), (dl.mixer, last["mixer_grads"], "mixer grad")):
                for n, gv in net.named_grads.items():
                    want = want_g[n].reshape(gv.shape)
                    _close(gv, want, 2e-3 * max(want.abs().max().item(), 1e-30), f"{tag} {what} {n}")
        for net, want_p, what in ((dl.q_net, ol.online, "online"), (dl.target_net, ol.target, "target"), (dl.mixer, ol.mixer, "mixer online"),
                                  (dl.mixer_target, ol.mixer_target, "mixer target")):
            for n, v in net.named.items():
                _close(v, want_p[n].reshape(v.shape), 3e-5 * (step + 1), f"{tag} {what} {n}")
    assert skipped == 2 and trained == 2 * iql_ref.PARITY_STEPS - 2 and ends > 0
    assert all(g.graph is not None for g in dl.groups), "the rollout must have been captured and replayed"
    for a, b in ((dl.q_net, dl.target_net), (dl.mixer, dl.mixer_target)):
        assert any(not torch.equal(x, y) for x, y in zip(a.named.values(), b.named.values())), "online and target parameters must have moved apart"


@pytest.mark.parametrize("case", iql_ref.PARITY_CASES, ids=[c[0] for c in iql_ref.PARITY_CASES])
def test_graph_replay_equals_eager_bit_for_bit(case):
    _, cfg, info = ref.parity_case(case, "two-groups")
    a, b = _device_learner(cfg, info, 2, use_graph=True), _device_learner(cfg, info, 2, use_graph=False)
    for _ in range(5):
        la, lb = a.update_step(), b.update_step()
        assert torch.equal(la, lb)
    assert all(g.graph is not None for g in a.groups) and all(g.graph is None for g in b.groups)
    for ga, gb in zip(a.groups, b.groups):
        for k, v in ga.ring.items():
            assert v is None or torch.equal(v, gb.ring[k]), k
        assert torch.equal(ga.h[0], gb.h[0]) and torch.equal(ga.cursor, gb.cursor) and torch.equal(ga.t_dev, gb.t_dev) and np.array_equal(ga.key, gb.key)
    assert torch.equal(a.q_net.P.flat, b.q_net.P.flat) and torch.equal(a.target_net.P.flat, b.target_net.P.flat)
    assert torch.equal(a.mixer.P.flat, b.mixer.P.flat) and torch.equal(a.mixer_target.P.flat, b.mixer_target.P.flat)


# ----------------------------------------------------------------------------- the system around the learner
SMALL = ["arch.num_envs=4", "arch.num_evaluation=2", "arch.num_eval_episodes=4", "arch.absolute_metric=True", "arch.num_absolute_metric_eval_episodes=4",
         "system.num_updates=8", "system.rollout_length=2", "system.epochs=2", "system.buffer_size=8", "system.min_buffer_size=4", "system.sample_batch_size=4",
         "system.sample_sequence_length=4", "env.kwargs.time_limit=5"]


def _small_cfg(tmp_path, seed, extra=()):
    from magpo_amd.config import compose
    return compose("rec_qmix", ["env=lbf", "env/scenario=8x8-2p-2f-coop", *SMALL, "system.total_timesteps=~", "system.eps_decay=40", "system.update_period=3",
                                f"system.seed={seed}", f"logger.base_exp_path={tmp_path}/", *extra])


def _setup(cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.systems.q_learning.anakin import rec_qmix
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg, add_global_state=True)
    ks = host_split(prng_key(int(cfg.system.seed)), 2)
    learn, nets, state = rec_qmix.learner_setup(env, (ks[0], ks[1]), cfg, torch.device(DEV))
    cfg = check_total_timesteps(cfg, 1)
    cfg.system.num_updates_per_eval = 2
    return learn, nets, state


def _flat(state):
    out = []
    for p in (state.params.online, state.params.target, state.params.mixer_online, state.params.mixer_target):
        out += [p[k] for k in sorted(p)]
    out += [state.opt_state[k] for k in ("mu", "nu", "mixer_mu", "mixer_nu")]
    out += [state.hidden_state, state.terminal, state.term_or_trunc, state.time_steps, state.train_steps]
    out += [state.obs[k] for k in sorted(state.obs)] + [state.env_state[k] for k in sorted(state.env_state)]
    out += [state.buffer_state["experience"][k] for k in sorted(state.buffer_state["experience"])]
    out += [state.buffer_state["current_index"], state.buffer_state["filled"]]
    return [t.detach().cpu() for t in out]


def test_learn_is_a_function_of_its_state_and_checkpoints_resume(tmp_path):
    from magpo_amd.systems.q_learning.types import LearnerState, QMIXParams
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    learn, (q_network, mixer), s0 = _setup(_small_cfg(tmp_path, 42, ["system.update_batch_size=2"]))
    assert q_network is learn.learner.q_net and mixer is learn.learner.mixer and isinstance(s0, LearnerState) and isinstance(s0.params, QMIXParams)
    assert all(torch.equal(s0.params.mixer_online[k], s0.params.mixer_target[k]) for k in s0.params.mixer_online)
    assert s0.params.mixer_online["layer_norm/scale"].eq(1).all() and not s0.params.mixer_online["hyper_w1/Dense_0/bias"].any()
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    assert s2.time_steps.tolist() == [32, 32] and s2.train_steps.tolist() == [6, 6] and s2.buffer_state["filled"].tolist() == [8, 8]
    ck = Checkpointer("rec_qmix", base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == set(ref.LOSS_NAMES) and out3.train_metrics["q_loss"].shape == (2, 2, 1)
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(_small_cfg(tmp_path, 7, ["system.update_batch_size=2"]))
    assert not torch.equal(t0.params.mixer_online["hyper_w1/Dense_0/kernel"], s0.params.mixer_online["hyper_w1/Dense_0/kernel"])
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", "rec_qmix", "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, LearnerState) and isinstance(restored.params, QMIXParams)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key) and r3.opt_state["count"] == s3.opt_state["count"] == 10
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


def test_hydra_entry_point_trains_and_evaluates(tmp_path):
    from magpo_amd.systems.q_learning.anakin import rec_qmix
    perf = rec_qmix.hydra_entry_point(["env=lbf", "env/scenario=8x8-2p-2f-coop", *SMALL, f"logger.base_exp_path={tmp_path}/", "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", "rec_qmix")
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]
    with pytest.raises(NotImplementedError, match="global state has .* 142 inputs"):      # (Robot Warehouse: refused when the envs are made)
        rec_qmix.hydra_entry_point(["env=rware", f"logger.base_exp_path={tmp_path}/"])
    with pytest.raises(NotImplementedError, match="real_next_obs"):
        rec_qmix.hydra_entry_point(["env=mpe", "env.kwargs.action_type=Discrete", f"logger.base_exp_path={tmp_path}/"])


def test_get_learner_fn_rejects_foreign_callables(tmp_path):
    from magpo_amd.q_net import GruQNetwork
    from magpo_amd.qmix_learner import adam_alone
    from magpo_amd.qmix_net import QMixer
    from magpo_amd.systems.q_learning.anakin import rec_qmix
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg(tmp_path, 3)
    env, _ = environments.make(cfg, add_global_state=True)
    net = GruQNetwork(env.num_agents, env.action_dim, env.obs_dim, DEV, seed=1)
    mixer = QMixer(env.num_agents, 32, env.obs_dim - env.num_agents, DEV, id_cols=env.num_agents, seed=1)
    sysc = rec_qmix.system_config(cfg)
    opt, mopt = adam_alone(net, sysc), adam_alone(mixer, sysc)
    with pytest.raises(TypeError):
        rec_qmix.get_learner_fn(env, (lambda *a: None, mixer.apply), (opt.update, mopt.update), cfg)
    with pytest.raises(TypeError):
        rec_qmix.get_learner_fn(env, (net.apply, torch.relu), (opt.update, mopt.update), cfg)
    with pytest.raises(TypeError):
        rec_qmix.get_learner_fn(env, (net.apply, mixer.apply), (opt.update, torch.relu), cfg)
    other = QMixer(env.num_agents, 32, env.obs_dim - env.num_agents, DEV, id_cols=env.num_agents, seed=2)
    with pytest.raises(ValueError):
        rec_qmix.get_learner_fn(env, (net.apply, other.apply), (opt.update, mopt.update), cfg)
    learner = rec_qmix.get_learner_fn(env, (net.apply, mixer.apply), (opt.update, mopt.update), cfg).learner
    assert learner.q_net is net and learner.mixer is mixer
