"""td7f_select_seq's argument checks (include/exo_amd.h), reached in plan-only
mode (td7f_probe): the entry validates its arguments and its LDS plan and
returns before anything is launched, so the descriptors here carry made-up
addresses and the test needs no GPU.  Shapes: the default networks
(TD7_multi_agent.py:61-140 at zs 300 / encoder 300 / actor 320)."""
import ctypes

import pytest

from exo_amd import _native as nat
from exo_amd.fused import KD, PREC, _ks

EINVAL = -22
FAKE = 0x10000  # never dereferenced: nothing launches under td7f_probe


def _lin(n_out, n_in, prec):
    thin = n_out <= 16
    return nat.TD7FLin(FAKE, None, FAKE, n_out, n_in, _ks(n_in, KD.get(prec, 32)), 0, FAKE if thin else None,
                       n_in if thin else 0)


def _nets(prec, S=80, A=7, Z=300, He=300, Ha=320):
    enc = (nat.TD7FLin * 3)(_lin(He, S, prec), _lin(He, He, prec), _lin(Z, He, prec))
    actor = (nat.TD7FLin * 4)(_lin(Ha, S, prec), _lin(Ha, Ha + Z, prec), _lin(Ha, Ha, prec), _lin(A, Ha, prec))
    return enc, actor


def _call(prec, seq=FAKE, t=FAKE, Lmax=347, mode=0, zimg=None, n=38, sigma=FAKE, ticket=FAKE, obs=FAKE, out=FAKE,
          rt=0, wg_cap=0, noise=True):
    enc, actor = _nets(prec)
    act = (ctypes.c_int32 * 3)(1, 1, 1)
    nz = nat.TD7FNoise(1, 2, 0, None, ticket, sigma, 1e-3, 0.15, 0.75, 0, None, None)
    return nat.lib().td7f_select_seq(prec, act, enc, actor, obs, n, ctypes.byref(nz) if noise else None, seq, t, Lmax,
                                     out, wg_cap, rt, zimg, mode, None)


@pytest.fixture
def probe():
    lib = nat.lib()
    lib.td7f_probe(1)
    try:
        yield
    finally:
        lib.td7f_probe(0)


@pytest.mark.parametrize("precision", ["bf16", "fp16", "fp32"])
def test_valid_plans(probe, precision):
    p = PREC[precision]
    assert _call(p) == 0
    assert _call(p, mode=2, zimg=FAKE) == 0
    assert _call(p, wg_cap=2, rt=1) == 0
    assert _call(p, n=8200) == 0
    if precision != "fp32":
        assert _call(p, rt=2) == 0 and _call(p, rt=2, mode=2, zimg=FAKE) == 0


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_refusals(probe, precision):
    p = PREC[precision]
    assert _call(p, seq=None) == EINVAL
    assert _call(p, t=None) == EINVAL
    assert _call(p, Lmax=0) == EINVAL
    assert _call(p, Lmax=-3) == EINVAL
    assert _call(p, mode=1, zimg=FAKE) == EINVAL  # the zs half takes no noise: td7f_select_part serves it
    assert _call(p, mode=3, zimg=FAKE) == EINVAL
    assert _call(p, mode=-1) == EINVAL
    assert _call(p, mode=2, zimg=None) == EINVAL  # the actor half without its zs image
    # td7f_select's own cases
    assert _call(p, n=0) == EINVAL
    assert _call(p, obs=None) == EINVAL
    assert _call(p, out=None) == EINVAL
    assert _call(p, noise=False) == EINVAL
    assert _call(p, rt=3) == EINVAL
    assert _call(p, wg_cap=-1) == EINVAL
    assert _call(7) == EINVAL
    # the state the ticket's holder writes
    assert _call(p, sigma=None) == EINVAL
    assert _call(p, ticket=None) == EINVAL
