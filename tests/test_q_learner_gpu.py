"""rec_iql on the GPU (magpo_amd/q_learner.py) against its restatement (tests/iql_ref.py) over enough update steps that the ring wraps and
episodes end inside sampled windows: actions, env state, ring contents and sampled indices bit for bit; hidden states, gradients, loss scalars
and both parameter sets within the tolerances of tests/test_ppo_learner_gpu.py for the same network kernels.  tests/test_iql_system.py shows
that the fp64 restatement has no near tie at these seeds, so fp32 rounding cannot flip an index."""
import os

import numpy as np
import pytest
import torch

from tests import iql_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENV_FIELDS = {"coordsum": (("step_count", "step_count"), ("target", "target"), ("record", "record"), ("key", "key")),
              "lbf": (("agent_pos", "agent_pos"), ("agent_level", "agent_level"), ("food_pos", "food_pos"), ("food_level", "food_level"),
                      ("step_count", "step_count"), ("key", "key"))}


def _device_learner(cfg, info, num_groups, use_graph=True):
    from magpo_amd.q_learner import QLearner
    dl = QLearner(cfg, info["N"], info["sys"], DEV, net_seed=None, wgrad_groups=4, num_groups=num_groups)
    dl.use_graph = use_graph
    dl.q_net.load_named(info["params"])
    dl.sync_target()
    dl.setup(info["key"], n_groups=num_groups)
    return dl


def _close(got, want, bound, what):
    got, want = got.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    err = (got - want).abs().max().item()
    print(f"CHECK {what}: err {err:.3e} bound {bound:.3e} ref {want.abs().max().item():.3e}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _ring_equal(g, og, tag):
    names = dict(obs="obs", mask="mask", action="action", reward="reward", terminal="terminal", term_or_trunc="term_or_trunc", next_obs="next_obs",
                 next_mask="next_mask")
    for k, rk in names.items():
        if g.ring[k] is not None:
            assert np.array_equal(g.ring[k].cpu().numpy(), og.ring.data[rk]), (tag, k)
    assert (int(g.cursor), int(g.filled), g.adds % g.S, min(g.adds, g.S)) == (og.ring.cursor, og.ring.filled, og.ring.cursor, og.ring.filled), tag
    assert int(g.t_dev) == og.t == g.t, tag


@pytest.mark.parametrize("variant", list(ref.PARITY_VARIANTS))
@pytest.mark.parametrize("case", ref.PARITY_CASES, ids=[c[0] for c in ref.PARITY_CASES])
def test_q_learner_matches_restatement(case, variant):
    ol, cfg, info = ref.parity_case(case, variant)
    U, T, s = ol.U, info["sys"].rollout_length, info["sys"]
    dl = _device_learner(cfg, info, U)
    skipped = trained = ends = 0
    for step in range(ref.PARITY_STEPS):
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
            _ring_equal(g, og, tag)
            _close(g.h[0], og.hidden.reshape(-1, 128), 1e-4, f"{tag} hidden state")
            for k in ("episode_return", "episode_length"):
                assert np.array_equal(g.metrics[k].cpu().numpy(), metrics[u][k]), (tag, k)
            ends += int(metrics[u]["is_terminal_step"].sum())
        for e, info_e in enumerate(infos):
            if info_e is None:      # the skipped-training phase: zero loss rows, no optimiser step, t_train stays
                skipped += 1
                assert not losses[e].any() and dl.t_train == 0 and dl.q_opt.count == 0
                continue
            trained += 1
            for i, name in enumerate(("q_loss", "mean_q", "mean_target")):
                assert abs(losses[e, 0, i] - info_e[name]) <= 1e-3, (tag, name, losses[e, 0, i], info_e[name])
        assert dl.t_train == ol.t_train == int(dl.t_train_dev) == dl.q_opt.count
        if infos[-1] is not None:
            last = ol.train_log[-1]
            for u in range(U):
                assert np.array_equal(dl._idx_host[u, 0], last["idx"][u][0]) and np.array_equal(dl._idx_host[u, 1], last["idx"][u][1]), (tag, "sampled indices")
            m = dl._mb
            q_ref = torch.cat([d["q"].transpose(0, 1).reshape(-1, info["K"]) for d in last["details"]])       # (T, B, A, K) -> rows (b, t, a)
            _close(dl.q_net.b.t["t_logits"][:, :info["K"]], q_ref, 1e-4, f"{tag} online Q values")
            _close(m["qn_online"][:, :info["K"]], torch.cat([d["qn_online"].transpose(0, 1).reshape(-1, info["K"]) for d in last["details"]]), 1e-4,
                   f"{tag} online next Q values")
            for n, gv in dl.q_net.named_grads.items():
                want = last["grads"][n].reshape(gv.shape)
                _close(gv, want, 2e-3 * max(want.abs().max().item(), 1e-30), f"{tag} grad {n}")
        for n, v in dl.q_net.named.items():
            _close(v, ol.online[n].reshape(v.shape), 3e-5 * (step + 1), f"{tag} online {n}")
        for n, v in dl.target_net.named.items():
            _close(v, ol.target[n].reshape(v.shape), 3e-5 * (step + 1), f"{tag} target {n}")
    assert skipped == 2 and trained == 2 * ref.PARITY_STEPS - 2 and ends > 0
    assert all(g.graph is not None for g in dl.groups), "the rollout must have been captured and replayed"
    differs = any(not torch.equal(a, b) for a, b in zip(dl.q_net.named.values(), dl.target_net.named.values()))
    assert differs, "online and target parameters must have moved apart"


@pytest.mark.parametrize("case", ref.PARITY_CASES, ids=[c[0] for c in ref.PARITY_CASES])
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


# ----------------------------------------------------------------------------- the system around the learner
def _small_cfg(tmp_path, seed, extra=()):
    from magpo_amd.config import compose
    return compose("rec_iql", ["env=lbf", "env/scenario=8x8-2p-2f-coop", "arch.num_envs=4", "arch.num_evaluation=2", "arch.num_eval_episodes=4",
                               "arch.absolute_metric=True", "arch.num_absolute_metric_eval_episodes=4", "system.total_timesteps=~", "system.num_updates=8",
                               "system.buffer_size=8", "system.min_buffer_size=4", "system.sample_batch_size=4", "system.sample_sequence_length=4",
                               "system.eps_decay=40", "env.kwargs.time_limit=5", f"system.seed={seed}", f"logger.base_exp_path={tmp_path}/", *extra])


def _setup(cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.systems.q_learning.anakin import rec_iql
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg)
    ks = host_split(prng_key(int(cfg.system.seed)), 2)
    learn, q_network, state = rec_iql.learner_setup(env, (ks[0], ks[1]), cfg, torch.device(DEV))
    cfg = check_total_timesteps(cfg, 1)
    cfg.system.num_updates_per_eval = 2
    return learn, q_network, state


def _flat(state):
    out = [state.params.online[k] for k in sorted(state.params.online)] + [state.params.target[k] for k in sorted(state.params.target)]
    out += [state.opt_state["mu"], state.opt_state["nu"], state.hidden_state, state.terminal, state.term_or_trunc, state.time_steps, state.train_steps]
    out += [state.obs[k] for k in sorted(state.obs)] + [state.env_state[k] for k in sorted(state.env_state)]
    out += [state.buffer_state["experience"][k] for k in sorted(state.buffer_state["experience"])]
    out += [state.buffer_state["current_index"], state.buffer_state["filled"]]
    return [t.detach().cpu() for t in out]


def test_learn_is_a_function_of_its_state_and_checkpoints_resume(tmp_path):
    from magpo_amd.systems.q_learning.types import LearnerState
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    learn, q_network, s0 = _setup(_small_cfg(tmp_path, 42, ["system.update_batch_size=2"]))
    assert q_network is learn.learner.q_net and isinstance(s0, LearnerState)
    assert s0.hidden_state.shape == (2, 8, 128) and s0.buffer_state["experience"]["obs"].shape[:3] == (2, 4, 8) and s0.key.shape == (2, 2)
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    assert s2.time_steps.tolist() == [32, 32] and s2.train_steps.tolist() == [6, 6] and s2.buffer_state["filled"].tolist() == [8, 8]
    ck = Checkpointer("rec_iql", base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == {"q_loss", "mean_q", "mean_target"} and out3.train_metrics["q_loss"].shape == (2, 2, 1)
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(_small_cfg(tmp_path, 7, ["system.update_batch_size=2"]))
    assert not torch.equal(t0.params.online["head.kernel"], s0.params.online["head.kernel"])
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", "rec_iql", "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, LearnerState)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key) and r3.opt_state["count"] == s3.opt_state["count"] == 10
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


def test_groups_with_different_keys_round_trip_through_snapshot_and_load(tmp_path):
    """common.load_rollout_state with a [groups, 2] key table (the Q learner keeps one key per group; the other systems pass one key for
    all): every group gets its own row back, as a copy, and a single key still goes to every group."""
    from magpo_amd.systems.common import load_rollout_state
    from magpo_amd.systems.q_learning.anakin import rec_iql
    learn, _, s0 = _setup(_small_cfg(tmp_path, 11, ["system.update_batch_size=2"]))
    learner = learn.learner
    assert s0.key.shape == (2, 2) and not np.array_equal(s0.key[0], s0.key[1])      # setup gave the groups different keys
    s1 = learn(s0).learner_state
    assert not np.array_equal(s1.key[0], s1.key[1]) and not np.array_equal(s1.key, s0.key)
    rec_iql.load_learner_state(learner, s0)
    for gi, g in enumerate(learner.groups):
        assert g.key.dtype == np.uint32 and np.array_equal(g.key, s0.key[gi]) and not np.shares_memory(g.key, s0.key)
    back = rec_iql._snapshot_state(learner)
    assert np.array_equal(back.key, s0.key)
    for a, b in zip(_flat(back), _flat(s0)):
        assert torch.equal(a, b)
    swapped = s0._replace(key=s0.key[::-1].copy())                                    # the rows follow the group axis, not a fixed order
    rec_iql.load_learner_state(learner, swapped)
    assert np.array_equal(learner.groups[0].key, s0.key[1]) and np.array_equal(learner.groups[1].key, s0.key[0])
    load_rollout_state(learner.groups, s0.key[1], s0.env_state, s0.obs, s0.term_or_trunc)   # one key: a copy for every group
    assert all(np.array_equal(g.key, s0.key[1]) for g in learner.groups) and not np.shares_memory(learner.groups[0].key, learner.groups[1].key)


@pytest.mark.parametrize("env", ["lbf", "coordsum"])
def test_hydra_entry_point_trains_and_evaluates(env, tmp_path):
    from magpo_amd.systems.q_learning.anakin import rec_iql
    scen = ["env=lbf", "env/scenario=8x8-2p-2f-coop"] if env == "lbf" else ["env=coordsum", "env/scenario=3x10-30"]
    perf = rec_iql.hydra_entry_point(scen + ["arch.num_envs=4", "arch.num_evaluation=2", "arch.num_eval_episodes=4", "arch.absolute_metric=True",
                                             "arch.num_absolute_metric_eval_episodes=4", "system.num_updates=8", "system.buffer_size=8",
                                             "system.min_buffer_size=4", "system.sample_batch_size=4", "system.sample_sequence_length=4",
                                             "env.kwargs.time_limit=5", f"logger.base_exp_path={tmp_path}/", "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", "rec_iql")
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]
    with pytest.raises(NotImplementedError, match="real_next_obs"):
        rec_iql.hydra_entry_point(["env=rware", f"logger.base_exp_path={tmp_path}/"])


def test_get_learner_fn_rejects_foreign_callables(tmp_path):
    from magpo_amd.optim import ClipAdam
    from magpo_amd.q_net import GruQNetwork
    from magpo_amd.systems.q_learning.anakin import rec_iql
    from magpo_amd.utils import make_env as environments
    cfg = _small_cfg(tmp_path, 3)
    env, _ = environments.make(cfg)
    net = GruQNetwork(env.num_agents, env.action_dim, env.obs_dim, DEV, seed=1)
    opt = ClipAdam(net, rec_iql.system_config(cfg))
    with pytest.raises(TypeError):
        rec_iql.get_learner_fn(env, lambda *a: None, opt.update, cfg)
    with pytest.raises(TypeError):
        rec_iql.get_learner_fn(env, net.apply, torch.relu, cfg)
    other = GruQNetwork(env.num_agents, env.action_dim, env.obs_dim, DEV, seed=2)
    with pytest.raises(ValueError):
        rec_iql.get_learner_fn(env, other.apply, opt.update, cfg)
    assert rec_iql.get_learner_fn(env, net.apply, opt.update, cfg).learner.q_net is net
