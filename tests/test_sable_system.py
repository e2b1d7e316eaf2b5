"""The guider-only Sable system (magpo_amd/systems/sable/anakin/rec_sable.py) on the CPU: its config tree and public names, and the
restatement the GPU tests compare against (tests/sable_ref.py) checked against finite differences, against oracle/ and against
independent formulations."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from oracle import coordsum as ocs
from oracle import learner as olearn
from oracle import networks as onets
from oracle import prng as oprng
from tests import kernel_refs as kr
from tests import sable_ref as sr

D = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ configs and names
def test_compose_rec_sable_key_tree_and_defaults():
    """configs/default/rec_sable.yaml composes logger / arch / system / network / env like rec_magpo; the system and network groups carry
    the reference's keys and default values (mava/configs/system/sable/rec_sable.yaml, network/rec_retention.yaml), overrides apply."""
    from magpo_amd.config import compose
    c = compose("rec_sable", ["env=coordsum"])
    assert set(c.keys()) == {"logger", "arch", "system", "network", "env"}
    s = c.system.to_container()
    s.pop("micro_batches")   # not a reference key (documented in the yaml)
    assert s == dict(total_timesteps=None, num_updates=1000, seed=42, add_agent_id=True, actor_lr=2.5e-4, update_batch_size=2, rollout_length=128,
                     ppo_epochs=4, num_minibatches=2, gamma=0.99, gae_lambda=0.95, clip_eps=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5,
                     decay_learning_rates=False)
    assert c.network.to_container() == dict(net_config=dict(n_block=1, embed_dim=64, n_head=1),
                                            memory_config=dict(type="rec_sable", decay_scaling_factor=0.8, timestep_positional_encoding=True,
                                                               timestep_chunk_size=None))
    assert c.env.env_name == "CoordSum" and compose("rec_sable").env.env_name == compose("rec_magpo").env.env_name
    c = compose("rec_sable", ["env=coordsum", "env/scenario=3x30-50", "network.net_config.embed_dim=128", "network.net_config.n_head=2",
                              "network.net_config.n_block=3", "system.ppo_epochs=10", "system.micro_batches=2", "arch.num_envs=64"])
    assert (c.network.net_config.embed_dim, c.network.net_config.n_head, c.network.net_config.n_block) == (128, 2, 3)
    assert c.system.ppo_epochs == 10 and c.system.micro_batches == 2 and c.arch.num_envs == 64
    with pytest.raises(KeyError):
        compose("rec_sable", ["system.clip_gpo=2.0"])   # a MAGPO key: not part of this system


def test_module_exports_the_reference_names():
    from magpo_amd.systems.sable import types as st
    from magpo_amd.systems.sable.anakin import rec_sable
    for n in ("get_learner_fn", "learner_setup", "run_experiment", "hydra_entry_point", "make_rec_sable_act_fn", "LearnerState", "Transition",
              "HiddenStates"):
        assert hasattr(rec_sable, n), n
    assert st.LearnerState._fields == ("params", "opt_states", "key", "env_state", "timestep", "hstates")
    assert st.HiddenStates._fields == ("encoder", "decoder_self_retn", "decoder_cross_retn")
    assert st.Transition._fields == ("done", "action", "value", "reward", "log_prob", "obs")
    assert rec_sable.LearnerState is st.RecLearnerState
    from magpo_amd.sable_learner import SableLearner
    from magpo_amd.learner import MagpoLearner
    # one rollout body, one gather, one capture: the Sable learner overrides the minibatch and the optimiser step only
    for shared in ("_rollout_body", "_capture", "_gather", "rollout", "update", "_permutation", "_rollout_keys"):
        assert getattr(SableLearner, shared) is getattr(MagpoLearner, shared), shared


def test_system_config_reads_a_sable_config():
    from magpo_amd.config import compose
    from magpo_amd.systems.common import _system_config
    from magpo_amd.systems.sable.anakin.rec_sable import system_config
    cfg = compose("rec_sable", ["env=coordsum", "system.micro_batches=4", "system.ent_coef=0.001"])
    s = system_config(cfg)
    assert s.micro_batches == 4 and s.ent_coef == 0.001 and s.rollout_length == 128 and not s.decay_learning_rates
    with pytest.raises((AttributeError, KeyError)):     # MAGPO's own reader still requires MAGPO's keys
        _system_config(cfg)


def test_tuned_sable_rows_build_a_sable_cfg():
    """The four tuned sable rows for CoordSum (experiment_data/params.csv:57-60, copied to tests/golden/sable_params.csv): every net is
    one the oracle network and the HIP guider's parameter layout accept."""
    from magpo_amd.params import FlatParams, guider_layout
    rows = list(csv.DictReader(open(os.path.join(HERE, "golden", "sable_params.csv"))))
    assert [(int(r["n_embd"]), int(r["n_head"]), int(r["n_block"])) for r in rows] == [(64, 1, 2), (128, 2, 3), (128, 4, 3), (32, 2, 1)]
    teams = {"3x10": (3, 10), "3x30": (3, 30), "5x20": (5, 20), "8x15": (8, 15)}
    for r in rows:
        assert r["system_name"] == "sable" and r["env_name"] == "coordsum"
        A, K = teams[r["task"]]
        E, nh, nb = int(r["n_embd"]), int(r["n_head"]), int(r["n_block"])
        cfg = onets.SableCfg(A, K, A + 1, embed_dim=E, n_block=nb, n_head=nh, decay_scaling_factor=float(r["decay_scaling_factor"]))
        assert (cfg.E, cfg.nh, cfg.nb) == (E, nh, nb) and len(cfg.kappas) == nh and E in (16, 32, 64, 128) and nh in (1, 2, 4) and E % nh == 0
        shapes = onets.guider_param_shapes(E, A + 1, K, nh=nh, nb=nb)
        assert {k: tuple(v.shape) for k, v in onets.init_guider_params(1, E, A + 1, K, nb=nb, nh=nh).items()} == shapes
        assert FlatParams(guider_layout(E, A + 1, K, nb, nh), "cpu").numel > 0


# ------------------------------------------------------------------------------------------------ the loss restatement
@pytest.mark.parametrize("masked", [False, True])
def test_ppo_loss_ref_against_finite_differences(masked):
    """Autograd gradients of ppo_loss_ref against central differences of its own total loss in fp64 (advantage statistics are inputs of
    the loss, not functions of the logits, so every entry is a local derivative)."""
    c = sr.ppo_case(12, 5, 11, **(dict(mask_p=0.6, one_legal=0.2) if masked else {}))
    ref = sr.ppo_loss_ref(c)
    assert not bool(sr.ppo_near_kink(ref, 1e-3).any())
    h = 1e-6
    for name, key, grad in (("gl", "dl", ref["dl"]), ("value", "dv", ref["dv"])):
        base = c[name].double()
        fd = torch.zeros_like(base)
        for i in range(base.numel()):
            for sgn in (1, -1):
                x = base.clone().reshape(-1)
                x[i] += sgn * h
                fd.reshape(-1)[i] += sgn * sr.ppo_loss_ref(dict(c, **{name: x.reshape(base.shape)}))["loss"][0] / (2 * h)
        if name == "gl":
            fd = torch.where(c["legal"], fd, torch.zeros_like(fd))   # an illegal logit is replaced by the mask value: no derivative
        assert kr.max_err(grad, fd) <= 1e-8, (name, kr.max_err(grad, fd))
    one = c["legal"].sum(1) == 1
    assert bool((ref["dl"][one] == 0).all()) and bool((ref["ent"][one] == 0).all())


@pytest.mark.parametrize("masked", [False, True])
def test_ppo_loss_ref_equals_the_oracle_guider_loss_at_equal_logits(masked):
    """oracle.learner.guider_loss with actor logits = guider logits: the log-ratio is 0, so the KL mask is 0 and clipped_ratio == ratio,
    which leaves the PPO loss.  Same total and the same logit / value gradients to 1e-12 in fp64 -- this ties the restatement to oracle/."""
    c = sr.ppo_case(300, 20, 12, **(dict(mask_p=0.6, one_legal=0.15) if masked else {}))
    ref = sr.ppo_loss_ref(c)
    gl, v = c["gl"].double().requires_grad_(True), c["value"].double().requires_grad_(True)
    glp = onets.masked_log_softmax(gl, c["legal"])
    g_logp = glp.gather(1, c["action"][:, None])[:, 0]
    pr = glp.exp()
    ent = -torch.where(pr == 0, torch.zeros_like(pr), pr * glp).sum(-1)
    mb = dict(log_prob=c["old"].double(), adv=c["adv"].double(), value=c["vold"].double(), targets=c["tgt"].double())
    total, info = olearn.guider_loss(kr.SYSC, v, g_logp, ent, glp, glp.detach(), g_logp.detach(), mb)
    dl, dv = torch.autograd.grad(total, [gl, v])
    assert float(info["kl_loss"].detach()) == 0.0
    assert abs(float(total.detach()) - float(ref["loss"][0])) <= 1e-12
    for a, b in ((info["guider_loss"], ref["loss"][1]), (info["entropy"], ref["loss"][2]), (info["value_loss"], ref["loss"][3])):
        assert abs(float(a.detach()) - float(b)) <= 1e-12
    assert kr.max_err(dl, ref["dl"]) <= 1e-12 and kr.max_err(dv, ref["dv"]) <= 1e-12


@pytest.mark.parametrize("i", range(len(sr.PPO_MATRIX)), ids=[sr.ppo_case_id(i) for i in range(len(sr.PPO_MATRIX))])
def test_ppo_matrix_cases_keep_their_rows(i):
    """At most 2 % of a case's rows are within KINK of a kink in the fp64 reference (they are left out of the GPU gradient comparison)."""
    c, r64, _ = sr.ppo_matrix_case(i)
    near = int(sr.ppo_near_kink(r64).sum())
    assert near <= 0.02 * c["R"], f"{c['name']}: {near} of {c['R']} rows near a kink: give the case another seed (PPO_SEED_BUMP)"


def test_ppo_kink_case_sits_on_every_kink():
    c, groups = sr.ppo_kink_case()
    ref = sr.ppo_loss_ref(c)
    eps = kr.SYSC.clip_eps
    assert float((ref["ratio"][groups["ratio_hi"]] - (1 + eps)).abs().max()) < 2e-7
    assert float((ref["ratio"][groups["ratio_lo"]] - (1 - eps)).abs().max()) < 2e-7
    e32 = torch.tensor(eps, dtype=torch.float32)
    assert bool((c["value"][groups["v_hi"]] - c["vold"][groups["v_hi"]] == e32).all())
    assert bool((c["value"][groups["v_lo"]] - c["vold"][groups["v_lo"]] == -e32).all())
    assert float((ref["e1"] - ref["e2"])[groups["v_equal"]].abs().max()) < 1e-7 and bool((ref["vd"][groups["v_equal"]] > eps).all())
    on = torch.zeros(c["R"], dtype=torch.bool)
    for sl in groups.values():
        on[sl] = True
    assert bool(sr.ppo_near_kink(ref)[on].all())
    # the other rows are ordinary ones, and the reference's own gradient is one of the enumerated candidates on every kink row
    assert int(sr.ppo_near_kink(ref)[~on].sum()) == 0
    dl, dv = sr.ppo_kink_candidates(c, ref)
    rows = torch.arange(c["R"])[on]
    for r in rows:
        assert float((dl[:, r] - ref["dl"][r]).abs().amax(1).min()) <= 1e-12, int(r)
        assert float((dv[:, r] - ref["dv"][r]).abs().min()) <= 1e-12, int(r)


# ------------------------------------------------------------------------------------------------ the learner restatement
def _oracle(A=3, K=10, TL=5, maxval=30, N=6, T=8, P=3, M=2, nb=1, nh=1, E=64, seed=3):
    spec = ocs.CoordSumSpec(A, K, TL, maxval)
    scfg = onets.SableCfg(A, K, A + 1, embed_dim=E, n_block=nb, n_head=nh)
    osys = olearn.SystemCfg(rollout_length=T, ppo_epochs=P, num_minibatches=M)
    ol = sr.SableOracleLearner(spec, N, osys, scfg, onets.init_guider_params(1, E, A + 1, K, nb=nb, nh=nh))
    ol.setup(oprng.split(oprng.prng_key(seed), 3)[0])
    return ol


def test_oracle_learner_gae_against_the_quadratic_sum():
    ol = _oracle()
    m = ol.rollout()
    assert m["is_terminal_step"].any(), "an episode must end inside the rollout"
    tr = ol.traj
    adv, tgt = sr.gae_quadratic(tr["reward"].double(), tr["value"].double(), tr["done"], ol.last_val.double(), torch.from_numpy(ol.dones),
                                ol.sys.gamma, ol.sys.gae_lambda)
    assert kr.max_err(tr["adv"], adv) <= 1e-5 and kr.max_err(tr["targets"], tgt) <= 1e-5
    # the states of envs whose episode ended on the last step are zero, the others are not
    ended = torch.from_numpy(ol.dones[:, 0])
    for h in ol.sable_hs:
        assert float(h[ended].abs().max() if bool(ended.any()) else 0.0) == 0.0 and float(h[~ended].abs().max()) > 0


def test_oracle_learner_carries_the_shuffled_states_across_epochs():
    """Quirk B19 (rec_sable.py:272,298): the states a minibatch trains on are the ORIGINAL rollout-start states taken by the composed
    index hs_idx_e = hs_idx_{e-1}[perm_e], while the trajectory is taken by perm_e alone."""
    ol = _oracle(P=3)
    ol.rollout()
    ol.rollout()      # second rollout: non-zero, distinct rollout-start states
    assert float(ol.prev_sable_hs[0].abs().max()) > 0
    key, perms, prev = ol.key, [], None
    for e in range(3):
        ks = oprng.split(key, 4)
        key = ks[0]
        bp, ap = oprng.permutation(ks[1], ol.N), oprng.permutation(ks[2], ol.spec.num_agents)
        perms.append(bp)
        mbs = ol.make_minibatches(bp, ap, prev)
        prev = ol._epoch_prev_hs
        idx = sr.compose_b19(perms)[-1]
        for h, orig in zip(prev, ol.prev_sable_hs):
            assert torch.equal(h, orig[torch.from_numpy(idx.astype(np.int64))]), e
        got = torch.cat([mb["prev_hs"][0] for mb in mbs])
        assert torch.equal(got, ol.prev_sable_hs[0][torch.from_numpy(idx.astype(np.int64))])
        obs = torch.cat([mb["obs"] for mb in mbs])      # trajectory: this epoch's permutation alone
        want = ol.traj["obs"].index_select(1, torch.from_numpy(bp.astype(np.int64))).index_select(2, torch.from_numpy(ap.astype(np.int64)))
        assert torch.equal(obs, want.transpose(0, 1).reshape(obs.shape))
    assert not np.array_equal(sr.compose_b19(perms)[1], perms[1]), "the composed index must differ from the epoch's permutation"


def test_oracle_learner_update_moves_the_parameters_and_keeps_the_key_chain():
    ol = _oracle(P=2)
    ol.rollout()
    key = ol.key
    before = {k: v.clone() for k, v in ol.gp.items()}
    infos = ol.update()
    assert len(infos) == 4 and set(infos[0]) == {"total_loss", "actor_loss", "entropy", "value_loss"}
    for _ in range(2):
        key = oprng.split(key, 4)[0]
    assert np.array_equal(ol.key, key) and ol.g_opt["count"] == 4
    assert any(not torch.equal(v, before[k]) for k, v in ol.gp.items())
    i = infos[0]
    assert i["total_loss"] == pytest.approx(i["actor_loss"] - ol.sys.ent_coef * i["entropy"] + ol.sys.vf_coef * i["value_loss"], abs=1e-6)
