"""The host-only parts of exo_amd.Collector (no GPU): per-policy argument
broadcasting and validation (fused.per_policy), the sigma-schedule bound
(collect.check_sigma_schedule), the replay strata (collect.default_strata) and
the segment / motion / env-argument layout it shares with Evaluator
(evaluate.segment_layout), compared with the expressions Evaluator's
constructor held before the two shared it."""
import numpy as np
import pytest

from exo_amd.collect import check_sigma_schedule, default_strata
from exo_amd.evaluate import segment_layout
from exo_amd.fused import MULTI_NOISE_TAG0, per_policy


def test_per_policy_broadcasts_and_validates():
    assert per_policy(0.25, 3, "sigma") == [0.25, 0.25, 0.25]
    assert per_policy([0.1, 0.0, 2], 3, "sigma") == [0.1, 0.0, 2.0]
    assert per_policy(np.float32(0.5), 1, "clip") == [0.5]
    for bad in ([0.1, 0.2], [[0.1, 0.2, 0.3]], [], -0.1, [0.1, -1e-9, 0.1], float("nan"), [0.1, float("inf"), 0.1]):
        with pytest.raises(ValueError, match="sigma"):
            per_policy(bad, 3, "sigma")
    with pytest.raises(ValueError, match="Collector: clip"):
        per_policy(-1, 2, "clip", "Collector")
    assert MULTI_NOISE_TAG0 > 3  # clear of the learner's (1, 2) and the replay's (3) streams


def test_sigma_schedule_bound():
    check_sigma_schedule([0.1, 0.3], [1e-3, 0.0], 100)
    check_sigma_schedule([0.2], [1e-3], 200)          # ends at 0 (up to the product's rounding)
    check_sigma_schedule([0.0, 0.0], [0.0, 0.0], 10 ** 9)
    check_sigma_schedule([0.1], [1.0], 0)
    with pytest.raises(ValueError, match="policy 0.*below 0"):
        check_sigma_schedule([0.1, 0.3], [1e-3, 0.0], 101)
    with pytest.raises(ValueError, match="policy 1"):
        check_sigma_schedule([0.1, 0.0], [0.0, 1e-12], 1)
    # a policy without envs never advances
    check_sigma_schedule([0.1, 0.3], [1e-3, 0.0], 500, counts=[0, 4])
    with pytest.raises(ValueError, match="below 0"):
        check_sigma_schedule([0.1, 0.3], [1e-3, 0.0], 500, counts=[1, 4])
    with pytest.raises(ValueError, match="steps"):
        check_sigma_schedule([0.1], [0.0], -1)


def _evaluator_layout(counts, env_kwargs, per_policy_env_kwargs):
    """what Evaluator computes for these counts (its constructor's expressions)"""
    seg = [0] + [int(v) for v in np.cumsum(counts)]
    kw = dict(env_kwargs or {})
    if per_policy_env_kwargs is not None:
        for name in per_policy_env_kwargs[0]:
            vals = [np.asarray(d[name], dtype=np.float64) for d in per_policy_env_kwargs]
            kw[name] = np.concatenate([np.broadcast_to(v, (c,) + v.shape) for v, c in zip(vals, counts)], axis=0)
    motions = np.concatenate([np.arange(c) % 8 for c in counts]).astype(np.int64)
    return seg, motions, kw


@pytest.mark.parametrize("counts", [[9, 14], [3, 0, 17, 8], [800] * 15, [1]])
def test_segment_layout_is_the_evaluators(counts):
    K = len(counts)
    rng = np.random.default_rng(K)
    per = [dict(tremor_sequence=rng.integers(0, 2, 7), max_force_elbow=20.0 + p) for p in range(K)]
    seg, motions, kw = segment_layout(K, counts, dict(dr_actuator_range=0.03), per, "Collector")
    wseg, wmotions, wkw = _evaluator_layout(counts, dict(dr_actuator_range=0.03), per)
    assert seg == wseg and seg[-1] == sum(counts)
    np.testing.assert_array_equal(motions, wmotions)
    assert motions.dtype == np.int64 and set(kw) == set(wkw) == {"dr_actuator_range", "tremor_sequence",
                                                                 "max_force_elbow"}
    assert kw["dr_actuator_range"] == 0.03
    for name in ("tremor_sequence", "max_force_elbow"):
        np.testing.assert_array_equal(kw[name], wkw[name])
    assert kw["tremor_sequence"].shape == (sum(counts), 7) and kw["max_force_elbow"].shape == (sum(counts),)
    for p in range(K):  # env i of a segment: motion i % 8, policy p's arguments
        a, b = seg[p], seg[p + 1]
        np.testing.assert_array_equal(motions[a:b], np.arange(b - a) % 8)
        assert (kw["max_force_elbow"][a:b] == 20.0 + p).all()
    st = default_strata(motions, 8)
    assert st.dtype == np.int32
    np.testing.assert_array_equal(st, motions % 8)
    np.testing.assert_array_equal(default_strata(motions, 3), (motions % 8) % 3)


def test_segment_layout_scalar_count_and_errors():
    seg, motions, kw = segment_layout(3, 5)
    assert seg == [0, 5, 10, 15] and kw == {}
    np.testing.assert_array_equal(motions, np.tile(np.arange(5), 3))
    for bad in ([4, 4], [4, -1, 4], [0, 0, 0]):
        with pytest.raises(ValueError, match="Collector: envs_per_policy"):
            segment_layout(3, bad, owner="Collector")
    with pytest.raises(ValueError, match="must hold 3 dicts"):
        segment_layout(3, 4, per_policy_env_kwargs=[{}, {}])
    with pytest.raises(ValueError, match="not given for every policy"):
        segment_layout(2, 4, per_policy_env_kwargs=[dict(max_force_elbow=1.0), {}])
