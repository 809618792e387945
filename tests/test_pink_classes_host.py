"""exo_amd.pink.length_classes / sequence_reference on the host: the per-class
tables td7f_pink_advance reads and the fp64 reference of one episode's
coloured-noise block (TD7_multi_agent_Pink_noise.py:203-228)."""
import numpy as np
import pytest

from exo_amd import pink

LENGTHS = [232, 347, 232, 8, 3]


@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_length_classes_against_spectrum_scale(beta):
    len_cls, cls_len, cls_scale, cls_norm = pink.length_classes(np.array(LENGTHS), beta)
    # the distinct lengths, each once, in increasing order
    assert cls_len.tolist() == [3, 8, 232, 347] and cls_len.dtype == np.int32
    assert len_cls.tolist() == [2, 3, 2, 1, 0] and len_cls.dtype == np.int32
    nf_max = 347 // 2 + 1
    assert cls_scale.shape == (4, nf_max) and cls_scale.dtype == np.float32
    assert cls_norm.shape == (4,) and cls_norm.dtype == np.float32
    for c, n in enumerate(cls_len):
        scale, sigma = pink._spectrum_scale(beta, int(n))
        nf = int(n) // 2 + 1
        assert scale.size == nf
        np.testing.assert_array_equal(cls_scale[c, :nf], scale.astype(np.float32))
        assert not cls_scale[c, nf:].any()
        assert cls_norm[c] == np.float32(1.0 / (int(n) * sigma))
    for i, n in enumerate(LENGTHS):
        assert cls_len[len_cls[i]] == n


def test_length_classes_refuses_what_has_no_spectrum():
    with pytest.raises(ValueError):
        pink.length_classes(np.array([232, 1]))
    with pytest.raises(ValueError):
        pink.length_classes(np.array([], dtype=np.int64))
    with pytest.raises(ValueError):
        pink.length_classes(np.array([232.0, 8.0]))


@pytest.mark.parametrize("n", [2, 3, 8, 17, 232, 347])
def test_sequence_reference_is_the_powerlaw_route(n):
    """the draws powerlaw_psd_gaussian makes, then buf / max|buf| * sigma"""
    beta, sigma, A = 1.0, 0.3, 7
    scale, _ = pink._spectrum_scale(beta, n)
    rng = np.random.default_rng(5)
    sr = rng.normal(scale=scale, size=(A, scale.size))
    si = rng.normal(scale=scale, size=(A, scale.size))
    buf = pink.powerlaw_psd_gaussian(beta, (A, n), rng=np.random.default_rng(5))
    want = buf / np.abs(buf).max() * sigma
    got = pink.sequence_reference(sr, si, beta, n, sigma)
    assert got.shape == (A, n)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    assert abs(np.abs(got).max() - sigma) <= 1e-15
    # the inputs are left alone; a zero spectrum gives a zero block
    assert si[0, 0] != 0
    assert not pink.sequence_reference(sr * 0, si * 0, beta, n, sigma).any()
