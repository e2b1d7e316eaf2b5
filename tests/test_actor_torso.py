"""The actor's torso configuration (network.actor_network.{pre,post}_torso -> MLPTorso, mava/networks/torsos.py:24-47) on the host:
parsing and validation, parameter layout and names, and the from-key initialisation."""
import numpy as np
import pytest
import torch

from magpo_amd.params import FlatParams, actor_layout, actor_named_views, init_actor, init_actor_from_key
from magpo_amd.torso import DEFAULT_TORSO, TorsoSpec, torso_from_config
from oracle import prng as oprng

MLP = "mava.networks.torsos.MLPTorso"


def _node(**kw):
    d = {"_target_": MLP, "layer_sizes": [128], "use_layer_norm": False, "activation": "relu"}
    d.update(kw)
    return d


@pytest.mark.parametrize("kw,want", [
    ({}, TorsoSpec((128,), "relu", False, True)),
    ({"layer_sizes": [256, 128], "activation": "tanh", "use_layer_norm": True}, TorsoSpec((256, 128), "tanh", True, True)),
    ({"layer_sizes": [64, 192, 256], "activate_final": False}, TorsoSpec((64, 192, 256), "relu", False, False)),
])
def test_supported_specs_parse(kw, want):
    assert torso_from_config(_node(**kw)) == want


@pytest.mark.parametrize("kw", [
    {"_target_": "mava.networks.torsos.CNNTorso"},
    {"layer_sizes": [100]},
    {"layer_sizes": [512]},
    {"layer_sizes": [128, 128, 128, 128]},
    {"layer_sizes": []},
    {"activation": "gelu"},
])
def test_unsupported_specs_raise(kw):
    with pytest.raises(NotImplementedError):
        torso_from_config(_node(**kw))


def _cfg(overrides):
    from magpo_amd.config import compose
    return compose("rec_magpo", ["env=coordsum", "env/scenario=3x10-30", *overrides])


def test_config_keys_reach_the_actor_and_unsupported_ones_raise():
    from magpo_amd.systems.gpo.anakin.rec_magpo import actor_torsos, learner_setup
    assert actor_torsos(_cfg([])) == (DEFAULT_TORSO, DEFAULT_TORSO)
    pre, post = actor_torsos(_cfg(["network.actor_network.pre_torso.layer_sizes=[256,128]", "network.actor_network.pre_torso.use_layer_norm=True",
                                   "network.actor_network.pre_torso.activation=tanh", "network.actor_network.post_torso.layer_sizes=[64]",
                                   "+network.actor_network.post_torso.activate_final=False"]))
    assert pre == TorsoSpec((256, 128), "tanh", True, True) and post == TorsoSpec((64,), "relu", False, False)
    with pytest.raises(NotImplementedError):
        actor_torsos(_cfg(["network.actor_network.pre_torso.layer_sizes=[96]"]))
    # hidden_state_dim other than 128 keeps raising (before any device work)
    with pytest.raises(NotImplementedError):
        learner_setup(_Env(), (None, None, None), _cfg(["network.hidden_state_dim=256"]), device="cpu")


class _Env:
    """Just enough of an env for learner_setup to reach its configuration checks."""
    num_agents = 3


def test_default_layout_is_unchanged():
    want = [("pre.kernel", (11, 128)), ("pre.bias", (128,)), ("gru.wi", (128, 384)), ("gru.bi", (384,)), ("gru.wh", (128, 384)),
            ("gru.hn.bias", (128,)), ("post.kernel", (128, 128)), ("post.bias", (128,)), ("head.kernel", (128, 5)), ("head.bias", (5,))]
    assert list(actor_layout(11, 128, 5).items()) == want
    assert list(actor_layout(11, 128, 5, DEFAULT_TORSO, DEFAULT_TORSO).items()) == want


def test_layout_and_names_follow_the_torso():
    pre, post = TorsoSpec((256, 128), "tanh", True), TorsoSpec((64, 192, 128))
    s = actor_layout(7, 128, 4, pre, post)
    assert list(s.items()) == [
        ("pre.kernel", (7, 256)), ("pre.bias", (256,)), ("pre.ln.bias", (256,)),
        ("pre1.kernel", (256, 128)), ("pre1.bias", (128,)), ("pre1.ln.bias", (128,)),
        ("gru.wi", (128, 384)), ("gru.bi", (384,)), ("gru.wh", (128, 384)), ("gru.hn.bias", (128,)),
        ("post.kernel", (128, 64)), ("post.bias", (64,)), ("post1.kernel", (64, 192)), ("post1.bias", (192,)),
        ("post2.kernel", (192, 128)), ("post2.bias", (128,)), ("head.kernel", (128, 4)), ("head.bias", (4,))]
    s = actor_layout(7, 128, 4, TorsoSpec((64,)), TorsoSpec((256,)))
    assert s["gru.wi"] == (64, 384) and s["head.kernel"] == (256, 4)
    P = FlatParams(s, "cpu")
    named = actor_named_views(P.views())
    assert named["gru.ir.kernel"].shape == (64, 128) and named["gru.hn.kernel"].shape == (128, 128)
    assert all(P.offsets[n] % 4 == 0 for n in s)
    init_actor(named, 3)   # torch-generator initialisation: every entry finite, LayerNorm / Dense biases zero
    assert all(torch.isfinite(v).all() for v in named.values())


def _restated(key, F, K, pre, post, H=128):
    """MLPTorso's @nn.compact body names its children Dense_0, LayerNorm_0, Dense_1, ...: Dense kernels orthogonal(sqrt 2), Dense and
    LayerNorm(use_scale=False) biases zero; GRUCell input kernels lecun-normal over the GRU input width (flax defaults)."""
    k = lambda path: oprng.flax_param_key(key, path, 1)
    out = {}
    for prefix, scope, spec, din in (("pre", "pre_torso", pre, F), ("post", "post_torso", post, H)):
        for i, d in enumerate(spec.layer_sizes):
            n = prefix if i == 0 else f"{prefix}{i}"
            out[n + ".kernel"] = oprng.init_orthogonal(k((scope, f"Dense_{i}")), (din, d), np.sqrt(2))
            out[n + ".bias"] = np.zeros(d, np.float32)
            if spec.use_layer_norm:
                out[n + ".ln.bias"] = np.zeros(d, np.float32)
            din = d
    cell = ("ScannedRNN_0", "GRUCell_0")
    for g in ("ir", "iz", "in"):
        out[f"gru.{g}.kernel"] = oprng.init_lecun_normal(k(cell + (g,)), (pre.width, H))
        out[f"gru.{g}.bias"] = np.zeros(H, np.float32)
    for g in ("hr", "hz", "hn"):
        out[f"gru.{g}.kernel"] = oprng.init_orthogonal(k(cell + (g,)), (H, H), 1.0)
    out["gru.hn.bias"] = np.zeros(H, np.float32)
    out["head.kernel"] = oprng.init_orthogonal(k(("action_head", "Dense_0")), (post.width, K), 0.01)
    out["head.bias"] = np.zeros(K, np.float32)
    return out


@pytest.mark.parametrize("pre,post", [(TorsoSpec((256, 128), "tanh", True), TorsoSpec((128, 64), use_layer_norm=True)),
                                      (TorsoSpec((64,)), TorsoSpec((128, 128)))])
def test_init_from_key_matches_restatement(pre, post):
    key = oprng.split(oprng.prng_key(11), 4)[2]
    F, K = 6, 5
    P = FlatParams(actor_layout(F, 128, K, pre, post), "cpu")
    named = actor_named_views(P.views())
    P.flat.fill_(7.0)
    init_actor_from_key(named, key)
    want = _restated(key, F, K, pre, post)
    assert set(want) == set(named)
    for n, v in named.items():
        assert np.array_equal(v.numpy(), want[n]), n
