"""Without a GPU: the seeds of the ff_sable acting-step parity cases have no Gumbel near-tie in the fp64 reference (so the GPU module may ask
for bit-exact actions of every row), the tuning switch parses, the header declares the entry point and the generated binding carries it,
and the entry point rejects shapes outside its set before any launch."""
import ctypes

import numpy as np
import pytest

from magpo_amd import _lib
from tests import ff_sable_act_cases as fc
from tests import ff_sable_ref as fs


@pytest.mark.parametrize("cid", sorted(fc.CASES))
def test_case_seeds_have_no_gumbel_near_ties(cid):
    """A draw of agent i + 1 depends on agent i's action, so the count is taken along the fp64 trajectory; a seed with a near-tie gets an
    entry in ff_sable_act_cases.SEED_BUMP."""
    x = fc.make_inputs(cid)
    a, lp, v, lp_all = fc.reference(cid)
    assert fs.gumbel_near_ties(x["key"], lp_all.numpy()) == 0, f"{cid}: a draw hangs on rounding: bump the seed"
    c = fc.CASES[cid]
    assert a.shape == (c["N"], c["A"]) and bool(np.isfinite(lp.numpy()).all()) and bool(np.isfinite(v.numpy()).all())
    if c["mask"]:   # the forced rows: one legal action, log-prob 0
        assert bool(x["mask"].gather(-1, a.long()[..., None]).all())
        for n, i in ((0, c["A"] - 1), (c["N"] - 1, 0)):
            assert int(a[n, i]) == c["K"] - 1 and abs(float(lp[n, i])) < 1e-12
    if c["A"] > 1 and c["K"] > 2 and c["N"] > 4:
        assert len(np.unique(a.numpy())) > 1, "the policy has no visible spread"


def test_cases_cover_the_shape_set():
    cs = list(fc.CASES.values())
    assert {c["A"] for c in cs} >= {1, 2, 3, 4, 5, 8}
    assert {c["N"] for c in cs} >= {1, fc.ENVS - 1, fc.ENVS, fc.ENVS + 1} and any(c["N"] > fc.ENVS + 1 and c["N"] % fc.ENVS for c in cs)
    assert {(c["nh"], c["nb"]) for c in cs} >= {(1, 1), (2, 2), (4, 1), (1, 4)}
    assert {c["E"] for c in cs} >= {16, 32, 64} and {c["K"] for c in cs} >= {2, 31}
    assert {(c["F"], c["ld"]) for c in cs} >= {(3, 3), (128, 128)} and any(c["ld"] % 4 for c in cs)
    assert {c["mask"] for c in cs} == {True, False} and any(c.get("act_scale", 1.0) > 1.0 for c in cs)


def test_autoregressive_case_depends_on_the_previous_action():
    """In the autoregression case the log-probs of agent i change visibly when agent i - 1's action is replaced."""
    import torch
    from oracle import networks as nets
    cid = "A3-N5-64.1.1-K8-F4-autoregressive"
    x = fc.make_inputs(cid)
    a, _, _, lp_all = fc.reference(cid)
    cfg, N = x["cfg"], a.shape[0]
    forced = (a + 1) % cfg.K
    p64 = {k: v.double() for k, v in x["gp"].items()}
    with torch.no_grad():
        _, _, _, _, lp2 = nets.sable_get_actions(p64, cfg, x["obs"].double(), x["mask"], torch.zeros(N, cfg.A, dtype=torch.int32),
                                                 nets.init_sable_hstates(N, cfg, torch.float64), x["key"], forced_actions=forced)
    assert float((lp2[:, 1:] - lp_all[:, 1:]).abs().max()) > 1e-2 and float((lp2[:, 0] - lp_all[:, 0]).abs().max()) == 0.0


def test_tuning_switch_parses():
    from magpo_amd.tuning import Tuning
    assert Tuning.from_env({"MAGPO_FF_SABLE_FUSED_ACT": "0"}).ff_sable_fused_act is False
    assert Tuning.from_env({"MAGPO_FF_SABLE_FUSED_ACT": "1"}).ff_sable_fused_act is True
    assert Tuning.from_env({}).ff_sable_fused_act == Tuning().ff_sable_fused_act
    assert Tuning.from_env({"MAGPO_FF_SABLE_FUSED_ACT": "1"}).ff_fused_step == Tuning().ff_fused_step


def test_header_declares_the_entry_point_and_the_binding_carries_it():
    ret, params = _lib.parse_header()["magpo_ff_sable_act"]
    assert ret == "int"
    assert [n for _, n in params] == ["dims_host", "keys_host", "ptrs_host", "nptrs", "blk_ptrs_host", "nblk_ptrs", "scratch_floats", "stream"]
    assert [_lib._ctype(t) for t, _ in params] == [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return _lib.lib()


def _call(built, dims, nptrs=22, nblk=None, scratch=None, keys=True, null_slot=None):
    """magpo_ff_sable_act on host stand-ins for the device pointers: every rejection happens before a pointer is touched."""
    N, A, nb = dims[0], dims[1], dims[4]
    buf = (ctypes.c_float * 4)()
    gp = np.full(max(nptrs, 1), ctypes.addressof(buf), dtype=np.uint64)
    if null_slot is not None:
        gp[null_slot] = 0
    bp = np.full(max(18 * nb if nblk is None else nblk, 1), ctypes.addressof(buf), dtype=np.uint64)
    d = np.array(dims, dtype=np.int32)
    k = np.zeros((8, 2), np.uint32)
    need = 32 * ((max(N, 1) + 31) // 32) * max(A, 1) * (384 + 256 * max(nb, 1))
    return built.call("magpo_ff_sable_act", d.ctypes.data, k.ctypes.data if keys else None, gp.ctypes.data, nptrs, bp.ctypes.data,
                      18 * nb if nblk is None else nblk, need if scratch is None else scratch, None)


GOOD = [8, 4, 10, 5, 1, 1, 64, 64, 0, 5]   # N, A, K, F, n_block, n_head, hs, gs, value_only, obs_ld


@pytest.mark.parametrize("change, match", [
    ({1: 9}, "A <= 8"), ({4: 5}, "n_block <= 4"), ({5: 3}, "n_head"), ({2: 32}, "K <= 31"), ({0: 0}, "N must be"), ({1: 0}, "A <= 8"),
    ({3: 129, 9: 129}, "F <= 128"), ({9: 4}, "obs_ld"), ({6: 32}, "n_head"), ({5: 2, 6: 32, 7: 32}, "n_head"),
])
def test_entry_point_rejects_shapes_outside_its_set(built, change, match):
    dims = list(GOOD)
    for i, v in change.items():
        dims[i] = v
    with pytest.raises(ValueError, match=match):
        _call(built, dims)
    assert built.last_error().startswith("magpo_ff_sable_act:")


def test_entry_point_rejects_bad_tables(built):
    with pytest.raises(ValueError, match="table size"):
        _call(built, GOOD, nptrs=21)
    with pytest.raises(ValueError, match="table size"):
        _call(built, GOOD, nblk=17)
    with pytest.raises(ValueError, match="scratch"):
        _call(built, GOOD, scratch=32 * 4 * 640 - 1)
    with pytest.raises(ValueError, match="null pointer"):
        _call(built, GOOD, null_slot=18)
    with pytest.raises(ValueError, match="null pointer"):
        _call(built, GOOD, null_slot=19)           # action_out is required unless value_only
    with pytest.raises(ValueError, match="keys"):
        _call(built, GOOD, keys=False, null_slot=2)
