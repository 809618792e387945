"""bench.py's command line: a plain run does the headline measurement alone,
`--steps` sets the timed steps, `--dump-outputs` writes the last timed step's
outputs, and the same arguments give the same outputs in another process."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5"]  # configs[1]: 4,096 envs
# what only --full measures or checks
FULL_ONLY = ("cpu_baseline", "roofline", "td7_variants", "sync_rounds", "reference_schedule", "weights_finite",
             "critic_gemm_roofline", "fused_critic_roofline", "reset_kernel_ms", "env_kernel_env_steps_per_sec")


def _run(dump):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *ARGS, "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump_a")
    return _run(d), d


def test_plain_run_prints_the_headline_line_alone(first):
    res, d = first
    assert res["steps"] == 20 and res["warmup"] == 5 and res["full"] is False
    assert res["unit"] == "env-steps/s" and res["higher_is_better"] is True and res["dtype"] == "f64 sim + bf16 TD7"
    assert res["ms_per_step"] > 0
    # async episodes: every timed step steps every env, so the value is the window's own rate
    assert res["value"] == pytest.approx(4096 * 20 / (20 * res["ms_per_step"] * 1e-3), rel=1e-9)
    assert res["measured_round"] is None
    assert not [k for k in FULL_ONLY if k in res]


def test_dump_outputs_are_the_last_steps_arrays(first):
    _, d = first
    shapes = {"obs": (4096, 80), "reward": (4096,), "done": (4096,), "info": (4096, 40)}
    files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}
    assert sorted(files) == sorted([*shapes, "actor", "critic", "encoder"])
    for n, a in files.items():
        assert a.dtype in (np.float32, np.float64), n
        assert np.isfinite(a).all(), n
        if n in shapes:
            assert a.shape == shapes[n], n
    assert set(np.unique(files["done"])) <= {0.0, 1.0}
    assert np.abs(files["obs"]).max() > 0 and np.abs(files["actor"]).max() > 0
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(d, "*.npy"))) <= 64 * 2 ** 20


def test_same_arguments_same_outputs(first, tmp_path):
    """Seeded inputs: another process with the same arguments starts from the
    same weights, env draws and RNG streams.  The kernels sum in a fixed
    order (their only atomics are integer tickets) and the graph's parallel
    branches touch disjoint data, so the last step's env outputs and the
    weights must be equal bit for bit."""
    _, d = first
    _run(tmp_path)
    for f in glob.glob(os.path.join(d, "*.npy")):
        np.testing.assert_array_equal(np.load(f), np.load(os.path.join(tmp_path, os.path.basename(f))),
                                      err_msg=os.path.basename(f))
