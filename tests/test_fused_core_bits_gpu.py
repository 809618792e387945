"""Every fused TD7 pass equals the recorded build bit for bit.

The GEMM core of csrc/td7_fused.h gives each wave whole-K output tiles; its
sums keep the order of the former split of the k-steps over two wave groups
(two accumulator chains per tile, over [0, kA) and [kA, ks), added once), so
every pass must reproduce the former build's bits exactly -- no tolerance.

tests/golden/td7f_core_bits.npz was recorded by tools/td7f_core_fixture.py at
the last commit with the two-k-group core (e6f47b1), on an MI355X; the test runs
the same function (run_case: select at 16 / 32 rows per workgroup and its
split halves, target_a + target_b, fixed, encoder, critic phase 0 and phases
1 + 2, actor a / b / c, and the weight-gradient launches they feed) and
compares the raw bits of every buffer a pass writes.  Arrays of at most 2 KiB
are kept whole, larger ones as the SHA-256 of their bytes plus their first 64
elements (64 KiB whole, as first planned, would put the six cases' 48 KiB
fp32 activations well past the 1 MB a fixture may take; the hash compares
every byte all the same).

Cases: B = 40 (two full row tiles and a ragged one) x {default widths: 5
tiles per wave, 5 / 10 / 20 / 30 k-steps, the former second group empty at 5;
every width 240: 4 tiles per wave, 15 and 25 k-steps, the former splits 10 / 5
and 15 / 10} x {bf16, fp16, fp32 (twice the k-steps)}.

Regenerating (after a toolchain change that legitimately moves bits, e.g. a
new libm tanhf / expf in the epilogues): check out a commit known good under
the old toolchain, build it with the new one, run
`python tools/td7f_core_fixture.py` on the GPU and commit the .npz it writes;
the test at that commit must pass before any later commit is judged by it.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("td7f_core_fixture", os.path.join(REPO, "tools", "td7f_core_fixture.py"))
fx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fx)


@pytest.fixture(scope="module")
def golden():
    with np.load(fx.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("setname,precision", fx.CASES)
def test_fused_passes_keep_the_recorded_bits(setname, precision, golden):
    res = fx.run_case(setname, precision)
    prefix = f"{setname}/{precision}/"
    want = {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}
    got = {}
    for name, arr in res.items():
        for suffix, v in fx.digest(arr).items():
            got[name + suffix] = v
    assert set(got) == set(want)
    bad = []
    for k in sorted(want):
        g, w = got[k], want[k]
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            bad.append(k)
    assert not bad, f"{len(bad)} of {len(want)} recorded arrays differ: {bad[:12]}"
