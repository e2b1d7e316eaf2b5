"""rec_qmix without a GPU: configs against the reference's values (and the stated deviations), exported names and types, what raises at
set-up, the restated pieces (tests/qmix_ref.py) and the near-tie count of every seed and shape the GPU parity test uses (zero: neither a
greedy selection nor an eps-greedy sample then hangs on fp32 rounding)."""
import numpy as np
import pytest
import torch

from oracle import prng
from tests import iql_ref
from tests import qmix_ref as ref

MLP = dict(_target_="mava.networks.torsos.MLPTorso", layer_sizes=[128], use_layer_norm=False, activation="relu")
# mava/configs/system/q_learning/rec_qmix.yaml
SYSTEM_DEFAULTS = dict(total_timesteps=None, num_updates=10000, seed=42, add_agent_id=True, min_buffer_size=32, update_batch_size=1, rollout_length=8,
                       epochs=4, buffer_size=1000, sample_batch_size=128, sample_sequence_length=20, q_lr=3e-5, max_grad_norm=10, hard_update=True,
                       update_period=200, tau=0.01, gamma=0.99, eps_min=0.05, eps_decay=1e5, qmix_embed_dim=32)
# mava/configs/network/qmix_rnn.yaml, with the deviation: hidden_state_dim and the torsos 128 wide where the reference has 256
NETWORK_DEFAULTS = dict(hidden_state_dim=128, q_network=dict(pre_torso=MLP, post_torso=MLP),
                        mixer_network=dict(_target_="mava.networks.base.QMixingNetwork", hyper_hidden_dim=64, norm_env_states=True))


def test_config_tree_and_defaults():
    from magpo_amd.config import compose
    cfg = compose("rec_qmix")
    assert set(cfg.to_container()) == {"logger", "arch", "system", "network", "env"}
    assert cfg.system.to_container() == SYSTEM_DEFAULTS
    assert cfg.network.to_container() == NETWORK_DEFAULTS
    assert cfg.network.hidden_state_dim == 128 and cfg.network.q_network.pre_torso.layer_sizes == [128]   # deviation: the reference has 256
    assert cfg.env.env_name == "LevelBasedForaging"      # deviation: the reference's default env is smax
    assert "mixer_network" not in compose("rec_iql").network.to_container()     # configs/network/q_rnn.yaml stays as it is


def test_exported_names_and_type_fields():
    from magpo_amd.qmix_learner import LOSS_NAMES
    from magpo_amd.systems.q_learning import types as t
    from magpo_amd.systems.q_learning.anakin import rec_qmix
    for n in ("get_learner_fn", "learner_setup", "run_experiment", "hydra_entry_point"):
        assert callable(getattr(rec_qmix, n)), n
    assert t.QMIXParams._fields == ("online", "target", "mixer_online", "mixer_target")
    assert t.QNetParams._fields == ("online", "target")
    assert LOSS_NAMES == ref.LOSS_NAMES


BIG_TEAM = ["env/scenario=8x8-2p-2f-coop", "env.scenario.task_config.num_agents=6"]    # 6 agents x 24 raw features = 144 state inputs


@pytest.mark.parametrize("overrides,match", [(["env=rware"], "real_next_obs"), (["env=vector-connector"], "real_next_obs"),
                                             (["+system.micro_batches=2"], "micro_batches"),
                                             (["CONTINUOUS"], "discrete action"),
                                             (["system.sample_sequence_length=9", "system.buffer_size=8"], "sample_sequence_length"),
                                             (["system.sample_sequence_length=1"], "sample_sequence_length"),
                                             (["network.hidden_state_dim=64"], "hidden_state_dim"),
                                             (BIG_TEAM, "144"),
                                             (["system.qmix_embed_dim=16"], "qmix_embed_dim"),
                                             (["system.qmix_embed_dim=48"], "qmix_embed_dim"),
                                             (["network.mixer_network.hyper_hidden_dim=32"], "hyper_hidden_dim"),
                                             (["network.mixer_network._target_=mava.networks.base.VDNMixer"], "QMixingNetwork")])
def test_unsupported_settings_raise_before_any_device_work(overrides, match):
    from magpo_amd.config import compose
    from magpo_amd.systems.q_learning.anakin import rec_qmix
    from magpo_amd.utils import make_env as environments
    continuous = overrides == ["CONTINUOUS"]       # (the env factories refuse the key themselves: set it behind them)
    cfg = compose("rec_qmix", [] if continuous else overrides)
    env, _ = environments.make(cfg)
    if continuous:
        cfg.env.kwargs.action_type = "Continuous"
    with pytest.raises(NotImplementedError, match=match):
        rec_qmix.check_supported(env.cfg, cfg)
    with pytest.raises(NotImplementedError, match=match):     # learner_setup refuses before it builds a network
        rec_qmix.learner_setup(env, (prng.prng_key(0), prng.prng_key(1)), cfg, device="cpu")
    if overrides is BIG_TEAM:
        with pytest.raises(NotImplementedError, match=match):
            environments.make(cfg, add_global_state=True)


def test_mixer_shape_limits():
    from magpo_amd.qmix_net import check_mixer_shape, mixer_layout
    check_mixer_shape(1, 32, 1); check_mixer_shape(8, 64, 128); check_mixer_shape(16, 32, 128)
    for bad in ((0, 32, 4), (9, 64, 9), (17, 32, 17), (2, 32, 0), (2, 32, 129), (2, 16, 4)):
        with pytest.raises(NotImplementedError):
            check_mixer_shape(*bad)
    assert {k: tuple(v) for k, v in mixer_layout(3, 32, 18).items()} == ref.mixer_shapes(3, 32, 18)


# ----------------------------------------------------------------------------- the restated pieces
def test_mixer_restatement_is_monotonic_and_matches_a_loop():
    A, E, G = 3, 32, 7
    p = {k: v.double() for k, v in ref.mixer_init(5, A, E, G).items()}
    g = torch.Generator().manual_seed(1)
    q, s = torch.randn(6, A, generator=g, dtype=torch.float64), torch.randn(6, G, generator=g, dtype=torch.float64)
    base = ref.mixer_apply(p, q, s, E)
    for a in range(A):
        up = q.clone(); up[:, a] += 0.5
        assert (ref.mixer_apply(p, up, s, E) >= base).all()
    # one row by hand
    x = (s[0] - s[0].mean()) / torch.sqrt(s[0].var(unbiased=False) + 1e-6) * p["layer_norm/scale"] + p["layer_norm/bias"]
    d = lambda n, v: v @ p[n + "/kernel"] + p[n + "/bias"]
    w1 = d("hyper_w1/Dense_1", torch.relu(d("hyper_w1/Dense_0", x))).abs().reshape(A, E)
    hid = torch.nn.functional.elu(q[0] @ w1 + d("hyper_b1/Dense_0", x))
    want = hid @ d("hyper_w2/Dense_1", torch.relu(d("hyper_w2/Dense_0", x))).abs() + d("hyper_b2/Dense_1", torch.relu(d("hyper_b2/Dense_0", x)))[0]
    assert abs(float(base[0] - want)) < 1e-9


def test_team_reward_and_loss_scalars():
    r = np.array([[0.1, 0.2, 0.7], [1.0, 0.0, 0.0]], np.float32)
    t = ref.team_reward(r)
    f = np.float32
    assert t.shape == r.shape and t[0, 0] == f(f(f(f(0.1) + f(0.2)) + f(0.7)) / f(3)) and (t[:, 0:1] == t).all()
    q, nq = torch.tensor([[1.0, 2.0]], dtype=torch.float64), torch.tensor([[0.5, 4.0]], dtype=torch.float64)
    rew, tot = torch.tensor([[1.0, 0.0]], dtype=torch.float64), torch.tensor([[0, 0, 1]], dtype=torch.uint8)
    loss, info, target = ref.td_loss(q, nq, rew, tot, 0.5)
    assert target.tolist() == [[1.25, 0.0]]          # the bootstrap is cut where term_or_trunc of the NEXT step is set
    assert float(loss) == pytest.approx((0.25 ** 2 + 4.0) / 2) and float(info["max_q_error"]) == 4.0 and float(info["min_q_error"]) == 0.0625
    assert float(info["done"]) == pytest.approx(1 / 3) and float(info["mean_next_qval"]) == 2.25 and float(info["mean_reward_t0"]) == 0.5


# ----------------------------------------------------------------------------- no near ties at the GPU parity test's seeds and shapes
@pytest.mark.parametrize("variant", list(iql_ref.PARITY_VARIANTS))
@pytest.mark.parametrize("case", iql_ref.PARITY_CASES, ids=[c[0] for c in iql_ref.PARITY_CASES])
def test_parity_seeds_have_no_near_ties(case, variant):
    """The fp64 restatement over the update steps of tests/test_qmix_learner_gpu.py: no acting step and no double-Q selection whose two best
    legal Q values are closer than 1e-4, no eps-greedy sample whose two best perturbed log-probabilities are closer than 1e-4; the ring wraps,
    episodes end inside sampled windows, and some sampled step has term_or_trunc = 1 with terminal = 0 (QMIX's bootstrap rule)."""
    ol, _, info = ref.parity_case(case, variant, torch.float64)
    ended, infos_all = 0, []
    for _ in range(iql_ref.PARITY_STEPS):
        metrics, infos = ol.update_step()
        ended += sum(int(m["is_terminal_step"].sum()) for m in metrics)
        infos_all += infos
    assert infos_all[:2] == [None, None] and all(i is not None for i in infos_all[2:])
    assert ended > 0 and all(g.ring.filled == 8 and g.ring.cursor == 0 for g in ol.groups)      # 16 adds into a ring of 8: wrapped
    explored = 0
    for e in ol.log:
        q = e["q"].numpy()
        assert iql_ref.top2_gap(q, e["mask"]).min() >= 1e-4, "acting step: near tie of the two best legal Q values"
        v = np.sort(iql_ref.perturbed_log_probs(e["key"], iql_ref.eps_greedy_probs(q.astype(np.float32), e["mask"], e["eps"])).astype(np.float64), axis=-1)
        finite = np.isfinite(v[..., -2])
        assert ((v[..., -1] - v[..., -2])[finite] >= 1e-4).all(), "eps-greedy sample: near tie of the two best perturbed log-probabilities"
        explored += int((e["action"] != iql_ref.greedy_action(q, e["mask"])).sum())
    assert explored > 0, "eps must make some action non-greedy"
    ends_inside = truncated_only = 0
    for tl in ol.train_log:
        for det, (env_idx, start), g in zip(tl["details"], tl["idx"], ol.groups):
            assert iql_ref.top2_gap(det["qn_online"].numpy(), None if det["next_mask"] is None else det["next_mask"].numpy()).min() >= 1e-4, \
                "double-Q selection: near tie"
            tot = det["rows"]["term_or_trunc"]
            ends_inside += int(tot[:, 1:].sum())
            truncated_only += int(((tot[:, 1:] == 1) & (det["terminal"][:, 1:] == 0)).sum())
    assert ends_inside > 0, "sampled windows must contain episode ends"
    if case[0] == "lbf":   # (CoordSum has no truncation: every episode end there sets discount = 0, so only LBF's time limit can show the rule)
        assert truncated_only > 0, "a sampled next step must have term_or_trunc = 1 and terminal = 0"
    else:
        assert truncated_only == 0
