"""The fused TD7 gradient passes keep the recorded bits at the edges of their
VALU stretches.

The stretches between the GEMMs of td7f_critic / td7f_actor / td7f_encoder
(AvgL1Norm backward, the thin heads' gradient operands, the Q head's rank-1
dX, the loss and tanh' blocks) were rescheduled without changing a value, a
summation order or a rounding, so every buffer the passes write must equal
the former build's bit for bit -- no tolerance.

tests/golden/td7f_edge_bits.npz was recorded by tools/td7f_edge_fixture.py
with the library of the last commit before that change (ae2dc15), on an
MI355X; the test runs the same function.  Cases (the tool's docstring has the
rows): default widths and every width 240, bf16 / fp16 / fp32, B = 1 (one live
row) and B = 17 (a row tile with one live row; rows whose q0 / l0 pre-norm
output is exactly zero -- norm_bwd's m < eps arm in the critic and both actor
backward passes; a row with TD error exactly 0 for head 0; a row with
|d| = 3e-38, whose 16-bit dq is subnormal or zero), plus the TD3+BC actor
phases.  The fixture keeps one SHA-256 per array (dtype, shape and bytes).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("td7f_edge_fixture", os.path.join(REPO, "tools", "td7f_edge_fixture.py"))
fx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fx)


@pytest.fixture(scope="module")
def golden():
    with np.load(fx.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("setname,precision,B", fx.CASES)
def test_gradient_passes_keep_the_recorded_bits_at_the_edges(setname, precision, B, golden):
    res = fx.run_case(setname, precision, B)
    key = f"{setname}/{precision}/{B}"
    names, sha = fx.digests(res)
    assert list(names) == list(golden[key + "/names"])
    bad = [str(n) for n, g, w in zip(names, sha, golden[key + "/sha"]) if not np.array_equal(g, w)]
    assert not bad, f"{len(bad)} of {len(names)} recorded arrays differ: {bad[:12]}"
