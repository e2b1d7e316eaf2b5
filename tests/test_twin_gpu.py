"""``twin()`` of the network classes: a second object of the same class, shape, row stride and torso / memory settings on the same device,
holding the same ``Tuning`` object, with storage of its own; once it has the first network's parameters, one acting step on the same input
gives bit-equal output (same kernels, same arguments).  Smallest shapes the constructors take: 3 agents, 5 actions, 4-feature rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
A, K, F, N = 3, 5, 4, 6


def _build(kind):
    from magpo_amd.actor import GruActor
    from magpo_amd.critic import GruCritic, global_state_ld
    from magpo_amd.ff_nets import FfActor, FfCritic
    from magpo_amd.q_net import GruQNetwork
    from magpo_amd.sable import SableGuider
    from magpo_amd.torso import TorsoSpec
    from magpo_amd.tuning import Tuning
    tuning = Tuning()
    torso = TorsoSpec((64, 128), activation="tanh")
    if kind == "gru_actor":
        return GruActor(A, K, F, DEV, seed=1, tuning=tuning, pre_torso=torso)
    if kind == "gru_critic":
        return GruCritic(A, F, DEV, seed=2, tuning=tuning, post_torso=torso)
    if kind == "gru_critic_centralised":      # global-state rows: 3 agents x 1 raw feature, 64 floats apart
        return GruCritic(A, A * 1, DEV, centralised=True, obs_ld=global_state_ld(A, 1), seed=3, tuning=tuning)
    if kind == "gru_q":
        return GruQNetwork(A, K, F, DEV, seed=4, tuning=tuning, wgrad_groups=8)
    if kind == "ff_actor":
        return FfActor(A, K, F, DEV, seed=5, tuning=tuning, torso=torso)
    if kind == "ff_critic":
        return FfCritic(A, F, DEV, seed=6, tuning=tuning, obs_ld=8)
    sable = dict(embed_dim=16, n_head=1, n_block=1, max_pos=7, seed=7, tuning=tuning)
    if kind == "sable_rec":
        return SableGuider(A, K, F, DEV, decay_scaling_factor=0.5, use_pe=False, **sable)
    return SableGuider(A, K, F, DEV, memory_type="ff_sable", **sable)


def _act(net, kind, g):
    """One acting step of ``net`` on inputs drawn from the generator ``g``; every output as a fresh tensor."""
    obs = torch.randn(N, A, net.Fld, generator=g).to(DEV)
    reset = (torch.rand(N, generator=g) < 0.3).to(torch.uint8).to(DEV)
    h_in = torch.randn(N * A, 128, generator=g).to(DEV)
    if kind.startswith("sable"):
        pos = torch.randint(0, 7, (N,), generator=g, dtype=torch.int32).to(DEV)
        keys = np.arange(2 * A, dtype=np.uint32).reshape(A, 2) + 11
        out = [torch.zeros(N, A, dtype=torch.int32, device=DEV), torch.zeros(N, A, device=DEV), torch.zeros(N, A, device=DEV)]
        states = None if net.ff else tuple(torch.randn(net.nb, net.ntile, N, 64, 64, generator=g).to(DEV) for _ in range(3))
        (net.act if net.ff else net.get_actions)(obs, pos, states, keys, *out)
        return out + list(states or ())
    if kind.startswith("ff"):
        return [(net.values(obs) if kind == "ff_critic" else net.logits(obs)).clone()]
    h_out = torch.empty_like(h_in)
    if kind.startswith("gru_critic"):
        return [net.step(obs, h_in, reset, h_out).clone(), h_out]
    return [net.step(obs, h_in, reset, h_out, want_logits=True).clone(), h_out]


@pytest.mark.parametrize("kind", ["gru_actor", "gru_critic", "gru_critic_centralised", "gru_q", "ff_actor", "ff_critic", "sable_rec", "sable_ff"])
def test_twin_has_the_layout_and_settings_and_acts_bit_equal_on_loaded_parameters(kind):
    net = _build(kind)
    twin = net.twin()
    assert type(twin) is type(net) and twin is not net and twin.tuning is net.tuning and twin.dev == net.dev
    assert list(twin.P.shapes.items()) == list(net.P.shapes.items()) and twin.P.offsets == net.P.offsets and twin.P.numel == net.P.numel
    assert (twin.A, twin.K, twin.F, twin.Fld, twin.G) == (net.A, net.K, net.F, net.Fld, net.G)
    for name in ("pre_spec", "post_spec", "spec", "centralised", "memory_type", "EL", "nh", "nb", "npos", "kappas", "use_pe", "decay_scaling_factor"):
        assert hasattr(twin, name) == hasattr(net, name) and getattr(twin, name, None) == getattr(net, name, None), name
    if kind == "sable_rec":
        assert net.kappas != [1.0] and not bool(net.pe.any()) and torch.equal(twin.pe, net.pe)      # the memory settings given above, not defaults
    assert twin.P.flat.data_ptr() != net.P.flat.data_ptr() and twin.grads.data_ptr() != net.grads.data_ptr()
    assert bool(net.P.flat.any()) and not bool(twin.P.flat.any())          # parameters of its own, not initialised
    twin.load_named(net.named)
    assert torch.equal(twin.P.flat, net.P.flat)
    got, want = _act(twin, kind, torch.Generator().manual_seed(3)), _act(net, kind, torch.Generator().manual_seed(3))
    assert len(got) == len(want) >= 1
    for a, b in zip(got, want):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b) and bool(torch.isfinite(b.float()).all())
    assert all(bool(t.any()) for t in want[1:] or want)     # (a sampled action table may be all zero; what is behind it is not)


# ---------------------------------------------------------------------------------------------------------------- bind_grads
BA, BK, BF, BNSEQ, BT = 2, 3, 5, 2, 2     # the smallest shape every training forward accepts: 2 sequences x 2 steps x 2 agents


def _bind_case(kind):
    """(net, run): ``run()`` is one training forward / backward on fixed inputs, which fills ``net.grads``."""
    from magpo_amd.actor import GruActor
    from magpo_amd.critic import GruCritic
    from magpo_amd.ff_nets import FfActor
    from magpo_amd.qmix_net import QMixer
    from magpo_amd.sable import SableGuider
    from magpo_amd.tuning import Tuning
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    if kind == "qmixer":       # R = 4 rows, A = 2, E = 32, 3 raw features per agent
        net, R = QMixer(BA, 32, 3, DEV, seed=6), 4
        obs, q, dq_tot, dq = rnd(R * BA, 3), rnd(R, BA), rnd(R), torch.empty(R, BA, device=DEV)

        def run():
            net.apply(obs, 3, R, q, train=True)
            net.bwd(dq_tot, dq=dq)
        return net, run
    R = BNSEQ * BT * BA
    obs, dvalue, dlogits = rnd(R, BF), rnd(R), torch.zeros(R, 64, device=DEV)
    dlogits[:, :BK] = rnd(R, BK)
    dones = (torch.rand(BNSEQ, BT, generator=g) < 0.3).to(torch.uint8).to(DEV)
    if kind == "ff_actor":
        net = FfActor(BA, BK, BF, DEV, seed=6, tuning=Tuning(), wgrad_groups=4)
        return net, lambda: (net.apply(obs), net.bwd(dlogits))
    if kind in ("gru_actor", "gru_critic"):
        net = GruActor(BA, BK, BF, DEV, seed=6, tuning=Tuning(), wgrad_groups=4) if kind == "gru_actor" else \
            GruCritic(BA, BF, DEV, seed=6, tuning=Tuning(), wgrad_groups=4)
        h0, h0_idx = rnd(BNSEQ * BA, 128), torch.arange(BNSEQ * BA, dtype=torch.int32, device=DEV)
        return net, lambda: (net.seq_fwd(obs, dones, h0, h0_idx, BNSEQ, BT), net.seq_bwd(dlogits if kind == "gru_actor" else dvalue))
    net = SableGuider(BA, BK, BF, DEV, embed_dim=int(kind[len("sable"):]), max_pos=4, seed=6, tuning=Tuning(), wgrad_groups=4)
    prev = torch.randint(0, BK + 1, (R,), generator=g, dtype=torch.int32).to(DEV)
    pos = torch.randint(0, 4, (R,), generator=g, dtype=torch.int32).to(DEV)
    s0 = tuple(0.1 * rnd(net.nb, net.ntile, BNSEQ, 64, 64) for _ in range(3))
    seq_env = torch.arange(BNSEQ, dtype=torch.int32, device=DEV)
    return net, lambda: (net.train_fwd(obs, prev, pos, dones, s0, seq_env, BNSEQ, BT), net.train_bwd(dlogits, dvalue))


@pytest.mark.parametrize("kind", ["gru_actor", "gru_critic", "ff_actor", "sable64", "sable32", "qmixer"])
def test_bind_grads_sends_the_next_backward_to_the_new_buffer_and_leaves_the_old_one(kind):
    """After ``bind_grads`` the same forward / backward writes the same gradients, bit for bit (no atomics in these kernels), into the new
    buffer -- pre-filled with NaN, so an entry the backward left to the old buffer would show -- and not one element of the old buffer,
    which holds NaN as its sentinel.  sable32 is the embedded network: the kernels write ``grads_D``, a buffer of the device width that
    stays the network's own, and ``emb.fold`` must land in the new logical buffer.

    "Every entry" is every entry a backward writes.  None writes the padding behind an entry (entries start at multiples of 4 floats), and
    the guider's none writes the gradients of the SwiGLU weights: the HIP path keeps those weights at their zero init
    (SableGuider.check_ffn_zero), their gradients are exactly 0 and stay what the buffer held -- the learners bind zero-filled buffers."""
    net, run = _bind_case(kind)
    run()
    torch.cuda.synchronize()
    first, old = net.grads.clone(), net.grads
    written = torch.zeros(net.P.numel, dtype=torch.bool, device=DEV)
    for n, v in net.P.views(written).items():
        v.fill_(".ffn." not in n)
    new = torch.full_like(first, float("nan"))
    net.bind_grads(new)
    old.fill_(float("nan"))
    lo, hi = new.data_ptr(), new.data_ptr() + 4 * new.numel()
    assert net.grads is new and all(lo <= v.data_ptr() < hi and v.untyped_storage().data_ptr() == new.untyped_storage().data_ptr()
                                    for v in net.named_grads.values())
    run()
    torch.cuda.synchronize()
    nan_new, nan_old = int(torch.isnan(new[written]).sum()), int(torch.isnan(old).sum())
    print(f"BINDGRADS {kind}: {int(written.sum())} of {new.numel()} entries written by a backward; NaN left among them {nan_new}; "
          f"old buffer still NaN in {nan_old} of {old.numel()}; bit-equal {torch.equal(new[written], first[written])}")
    assert torch.equal(new[written], first[written])
    assert nan_new == 0
    assert nan_old == old.numel()
