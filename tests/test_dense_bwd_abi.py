"""magpo_dense_bwd without a GPU: every unsupported argument combination is refused with MAGPO_EINVAL (ValueError) before a pointer is touched
(null pointers, or a host buffer standing in for the mask as in test_abi::test_linear_validates_mask_and_width_before_any_launch), and the
host-side threshold that routes a layer to it has its documented default and no environment variable."""
import ctypes

import pytest

from magpo_amd import _lib


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return _lib.lib()


def _args(**kw):
    """(X, ldx, dY, ldy, W, mask, ldmask, dX, lddx, R, KIN, NOUT, dW, db, workspace, G, act, stream) of a valid 64 x 64 call, with overrides."""
    a = dict(X=None, ldx=64, dY=None, ldy=64, W=None, mask=None, ldmask=0, dX=None, lddx=64, R=1, KIN=64, NOUT=64, dW=None, db=None, ws=None, G=1,
             act=0, stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return tuple(a.values())


BUF = (ctypes.c_float * 4)()
HOST = ctypes.addressof(BUF)

REJECTED = [
    ("KIN", dict(KIN=32, ldx=32, lddx=32)), ("KIN", dict(KIN=192, ldx=192, lddx=192)), ("KIN", dict(KIN=0)), ("KIN", dict(KIN=96, ldx=96, lddx=96)),
    ("NOUT", dict(NOUT=0)), ("NOUT", dict(NOUT=-3)), ("NOUT", dict(NOUT=65, ldy=68)), ("NOUT", dict(NOUT=128, ldy=128)),
    ("multiples of 4", dict(ldx=66)), ("multiples of 4", dict(ldy=66)), ("multiples of 4", dict(lddx=70)),
    ("multiples of 4", dict(ldx=60)), ("multiples of 4", dict(lddx=32)), ("multiples of 4", dict(NOUT=20, ldy=16)),
    ("act", dict(act=1)), ("act", dict(act=6, mask=HOST, ldmask=64)), ("act", dict(act=-1)), ("act", dict(act=5)),
    ("mask", dict(act=4)), ("mask", dict(act=0, mask=HOST, ldmask=64)),
    ("ldmask", dict(act=4, mask=HOST, ldmask=66)), ("ldmask", dict(act=4, mask=HOST, ldmask=32)),
    ("16-byte aligned", dict(X=4096 + 4)), ("16-byte aligned", dict(dY=4096 + 8)), ("16-byte aligned", dict(X=4096, dY=8192 + 12)),
    ("R must", dict(R=0)), ("R must", dict(R=-5)), ("R must", dict(R=2 ** 31)), ("R must", dict(G=0)),
]


@pytest.mark.parametrize("match,override", REJECTED)
def test_rejected_before_any_pointer_is_touched(built, match, override):
    with pytest.raises(ValueError, match=match):
        built.call("magpo_dense_bwd", *_args(**override))


def test_threshold_default_and_no_environment_variable():
    from magpo_amd.tuning import Tuning
    assert Tuning().dense_bwd_min_rows == 16384
    assert Tuning.from_env({}) == Tuning()
    # no variable moves it: whatever the environment holds, the field keeps its default
    e = {k: "0" for k in ("MAGPO_DENSE_BWD_MIN_ROWS", "MAGPO_DENSE_BWD", "MAGPO_DENSE_BWD_ROWS")}
    assert Tuning.from_env(e).dense_bwd_min_rows == 16384
    src = open(__import__("magpo_amd.tuning", fromlist=["x"]).__file__).read()
    assert "MAGPO_DENSE" not in src
