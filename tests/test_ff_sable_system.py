"""The memoryless Sable system (magpo_amd/systems/sable/anakin/ff_sable.py) without a GPU: its config tree against the reference's values,
what learner_setup writes into the memory config and what raises, the item and agent order of the shuffle against the restatement, the
restated ff retention against the recurrent system's retention in fp64 (the yardstick of tests/test_team_retention_gpu.py), and the Gumbel
near-tie count of every seed and shape the GPU parity test uses."""
import numpy as np
import pytest
import torch

from oracle import networks as onets
from oracle import prng
from tests import ff_sable_ref as fs

D = torch.float64


# ------------------------------------------------------------------------------------------------ configs and names
def test_compose_ff_sable_key_tree_and_defaults():
    """configs/default/ff_sable.yaml composes logger / arch / system / network / env; the system and network groups carry the reference's
    keys and values (mava/configs/system/sable/ff_sable.yaml, network/ff_retention.yaml)."""
    from magpo_amd.config import compose
    c = compose("ff_sable", ["env=coordsum"])
    assert set(c.keys()) == {"logger", "arch", "system", "network", "env"}
    assert c.system.to_container() == dict(total_timesteps=None, num_updates=1000, seed=42, add_agent_id=True, actor_lr=2.5e-4, update_batch_size=2,
                                           rollout_length=128, ppo_epochs=4, num_minibatches=2, gamma=0.99, gae_lambda=0.95, clip_eps=0.2,
                                           ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, decay_learning_rates=False)
    assert c.network.to_container() == dict(net_config=dict(n_block=1, embed_dim=64, n_head=1),
                                            memory_config=dict(type="ff_sable", agents_chunk_size=None))
    assert c.env.env_name == "CoordSum" and compose("ff_sable").env.env_name == compose("rec_sable").env.env_name


def test_memory_config_as_learner_setup_writes_it():
    """ff_sable.py:339-350: kappa scaling 1, chunk size = num_agents, timestep positional encoding off."""
    from magpo_amd.config import compose
    from magpo_amd.systems.sable.anakin import ff_sable
    c = compose("ff_sable", ["env=coordsum"])
    ff_sable.configure_memory(c, 4)
    mc = c.network.memory_config
    assert mc.decay_scaling_factor == 1.0 and mc.chunk_size == 4 and mc.timestep_positional_encoding is False and mc.type == "ff_sable"
    s = ff_sable.system_config(c)
    assert s.rollout_length == 128 and s.micro_batches == 1 and s.num_minibatches == 2


def test_agents_chunk_size_and_micro_batches_raise():
    from magpo_amd.config import compose
    from magpo_amd.systems.sable.anakin import ff_sable
    c = compose("ff_sable", ["env=coordsum", "network.memory_config.agents_chunk_size=2"])
    with pytest.raises(NotImplementedError, match="agents_chunk_size"):
        ff_sable.configure_memory(c, 4)
    c = compose("ff_sable", ["env=coordsum", "network=rec_retention"])
    with pytest.raises(NotImplementedError, match="ff_sable"):
        ff_sable.configure_memory(c, 4)

    class Env:   # learner_setup reads nothing else before it checks the system keys
        num_agents = 4
    c = compose("ff_sable", ["env=coordsum", "+system.micro_batches=2"])
    with pytest.raises(NotImplementedError, match="micro_batches"):
        ff_sable.learner_setup(Env(), (prng.prng_key(0), prng.prng_key(1)), c, device="cpu")
    c = compose("ff_sable", ["env=coordsum", "+env.kwargs.action_type=Continuous"])
    with pytest.raises(NotImplementedError, match="discrete"):
        ff_sable.learner_setup(Env(), (prng.prng_key(0), prng.prng_key(1)), c, device="cpu")


def test_module_exports_the_reference_names():
    from magpo_amd.systems.sable import types as st
    from magpo_amd.systems.sable.anakin import ff_sable
    for n in ("get_learner_fn", "learner_setup", "run_experiment", "hydra_entry_point", "make_ff_sable_eval_act_fn", "LearnerState", "Transition"):
        assert hasattr(ff_sable, n), n
    assert st.FFLearnerState._fields == ("params", "opt_states", "key", "env_state", "timestep")
    assert ff_sable.LearnerState is st.FFLearnerState and st.LearnerState is st.RecLearnerState


# ------------------------------------------------------------------------------------------------ the shuffle
def test_item_and_agent_shuffle_order_against_the_restatement():
    """What FfSableLearner.update gathers: items t * N + n of the time-major buffers by ONE permutation of T * N, agents by ONE permutation
    of A, cut into num_minibatches slices -- written out by index against FfSableOracleLearner.make_minibatches, and the key chain of an
    epoch (split 4: key, items, agents, entropy)."""
    ol, _, info = fs.make_case(fs.PARITY_CASES[1])
    T_, N_, A_ = info["T"], info["N"], info["A"]
    ol.rollout()
    key0 = ol.key.copy()
    infos, perms = ol.update()
    assert len(infos) == fs.PARITY_EPOCHS * fs.PARITY_MINIBATCHES
    key = key0
    for perm, agent_perm in perms:
        ks = prng.split(key, 4)
        key = ks[0]
        assert np.array_equal(perm, prng.permutation(ks[1], T_ * N_)) and np.array_equal(agent_perm, prng.permutation(ks[2], A_))
        assert sorted(perm.tolist()) == list(range(T_ * N_)) and sorted(agent_perm.tolist()) == list(range(A_))
    assert np.array_equal(key, ol.key)
    perm, agent_perm = perms[0]
    mbs = ol.make_minibatches(perm, agent_perm)
    per = T_ * N_ // fs.PARITY_MINIBATCHES
    for m, mb in enumerate(mbs):
        idx = perm[m * per:(m + 1) * per]
        for k in ("action", "obs", "adv", "done", "step_count"):
            want = torch.stack([ol.traj[k][i // N_, i % N_][agent_perm.astype(np.int64)] for i in idx.tolist()])
            assert torch.equal(mb[k], want), (m, k)
        assert all(float(h.abs().max()) == 0 for h in mb["prev_hs"]) and mb["prev_hs"][0].shape[0] == per


def test_ff_gae_equals_the_slot_form():
    """The GAE of ff_sable.py:135-155 on the flag of the step itself = oracle.learner.calculate_gae on flags shifted by one slot (done[t] =
    "the observation of step t starts an episode", last_done = the flag of the last step): the form magpo_gae evaluates."""
    from oracle import learner as olearn
    g = torch.Generator().manual_seed(3)
    T_, N_, A_ = 9, 5, 3
    reward, value, last_val = (torch.randn(*s, generator=g, dtype=D) for s in ((T_, N_, A_), (T_, N_, A_), (N_, A_)))
    done = (torch.rand(T_, N_, 1, generator=g) < 0.3).expand(T_, N_, A_)
    slot = torch.cat([torch.zeros(1, N_, A_, dtype=torch.bool), done[:-1]])
    a1, t1 = fs.ff_gae(reward, value, done, last_val, 0.99, 0.95)
    a2, t2 = olearn.calculate_gae(reward, value, slot, last_val, done[-1], 0.99, 0.95)
    assert torch.equal(a1, a2) and torch.equal(t1, t2) and bool(done.any())


# ------------------------------------------------------------------------------------------------ the retention restatement
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A,hs", [(1, 16), (3, 32), (5, 64), (8, 16), (32, 64)])
def test_ff_retention_equals_rec_retention_at_one_step(A, hs, masked):
    """fp64: the ff retention (retention.py:79-84, 94-99) = the recurrent system's chunkwise retention (:86-99) with T = 1, kappa = 1, a
    zero state and no done flag; and on a zero state with ANY kappa, which is why the oracle network restates ff_sable.  So the chunk
    kernels run as T = 1 sequences are the right yardstick for the team kernels."""
    g = torch.Generator().manual_seed(100 * A + hs + masked)
    B = 7
    q, k, v = (torch.randn(B, A, hs, generator=g, dtype=D) for _ in range(3))
    want = fs.ff_retention(q, k, v, masked)
    dones = torch.zeros(B, A, dtype=torch.bool)
    z = torch.zeros(B, hs, hs, dtype=D)
    for kappa in (1.0, 0.8):
        got = fs.rec_retention(q, k, v, z, dones, A, kappa, masked, )
        assert torch.equal(got, want), (kappa, (got - want).abs().max())
    # the restated backward against autograd
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    dr = torch.randn(B, A, hs, generator=g, dtype=D)
    gq, gk, gv = torch.autograd.grad((fs.ff_retention(qa, ka, va, masked) * dr).sum(), [qa, ka, va])
    for got, ref in zip(fs.ff_retention_bwd(q, k, v, dr, masked), (gq, gk, gv)):
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    # the acting form: row i of decoder iteration i (ntok = i + 1, ret_from = i) is row i of the causal product
    causal = fs.ff_retention(q, k, v, True)
    for i in range(A):
        part = fs.ff_retention_partial(q, k, v, True, i + 1, i)
        assert (part[:, i] - causal[:, i]).abs().max().item() <= 1e-12 * max(1.0, causal.abs().max().item())
        assert bool(torch.isnan(part[:, :i]).all()) and bool(torch.isnan(part[:, i + 1:]).all())


def test_oracle_network_on_zero_states_is_the_ff_network():
    """sable_train on (items, A) sequences with zero states: independent of the decay factor and of the done flags' absence, and its
    encoder retention is the unmasked, its decoder retention the causal ff retention (checked through msr_chunk's pre-GroupNorm output)."""
    A, K, F, B = 3, 5, 4, 6
    p = {k: v.double() for k, v in onets.init_guider_params(3, 64, F, K).items()}
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(B, A, F, generator=g, dtype=D)
    action = torch.randint(0, K, (B, A), generator=g)
    mask = torch.ones(B, A, K, dtype=torch.bool)
    sc = torch.randint(0, 5, (B, 1), generator=g).expand(B, A)
    dones = torch.zeros(B, A, dtype=torch.bool)
    outs = []
    for scaling in (1.0, 0.8):
        cfg = onets.SableCfg(A, K, F, decay_scaling_factor=scaling, use_pe=False)
        outs.append(onets.sable_train(p, cfg, obs, action, mask, sc, onets.init_sable_hstates(B, cfg, D), dones))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    cfg = fs.ff_cfg(A, K, F)
    x = torch.randn(B, A, 64, generator=g, dtype=D)
    for masked in (False, True):
        _, _, ret = onets.msr_chunk(p, "enc.block0.retn.", x, x, x, torch.zeros(B, 1, 64, 64, dtype=D), dones, sc, n_agents=A, nh=1, masked=masked,
                                    kappas=cfg.kappas, use_pe=False)
        w = p["enc.block0.retn.w_q"][0], p["enc.block0.retn.w_k"][0], p["enc.block0.retn.w_v"][0]
        assert torch.equal(ret, fs.ff_retention(x @ w[0], x @ w[1], x @ w[2], masked))


# ------------------------------------------------------------------------------------------------ parity seeds
@pytest.mark.parametrize("case", fs.PARITY_CASES, ids=fs.case_id)
def test_parity_seeds_have_no_gumbel_near_ties(case):
    """Three update steps of the fp64 restatement at the seeds and shapes of the GPU parity test: no sample's top two perturbed log-probs
    are closer than 1e-4, so fp32 rounding cannot change a sampled action; episodes end where the case says."""
    ol, _, info = fs.make_case(case, torch.float64)
    ended = False
    for _ in range(3):
        metrics = ol.rollout()
        ended |= bool(metrics["is_terminal_step"].any())
        for t in range(info["T"]):
            assert fs.gumbel_near_ties(ol.sample_keys[t], ol.traj["lp_all"][t].numpy()) == 0, (fs.case_id(case), t)
        infos, _ = ol.update()
        assert len(infos) == fs.PARITY_EPOCHS * fs.PARITY_MINIBATCHES
    assert ended == case[-1]
