"""td7f_pink_advance / exo_amd.fused.PinkNoise on the MI355X: one coloured
noise sequence per env, generated on the device by a direct inverse real DFT in
fp32 (TD7_multi_agent_Pink_noise.py:203-228 per env).

The reference is pink.sequence_reference (numpy irfft in fp64, peak
normalisation, times sigma) on the very spectra the kernel used: the ones the
test feeds, or the ones the kernel reports (spec_out) in Philox mode.

The bound is the fp32 summation and twiddle error of the direct DFT, computed
from those spectra.  With nf = n // 2 + 1 and, per column,
    S = cls_norm * (|sr_0| + sum_k w_k (|sr_k| + |si_k|)),  w_k = 2 (1 at Nyquist),
E = (nf + 16) * 2^-23 * max_columns S bounds the error of an unnormalised x,
and tol = 2 sigma E / peak + 4 * 2^-24 sigma that of x * (sigma / peak): the
errors of x and of the peak, then the roundings of the gain and the product.
Columns t >= n_r of a row are never read by the select launch and are not
asserted on.

Policies are the stand-ins of test_select_multi_noise_gpu.py (they only give
the set its size and action width here).
"""
import ctypes

import numpy as np
import pytest
import torch

from test_select_multi_gpu import _agent, _bits, _policy_set

pytestmark = pytest.mark.gpu

BETA = 1.0
A = 7
# the smallest, even and odd, and the shortest and longest motion; every class in both policies
LENGTHS = np.array([2, 3, 8, 17, 232, 347, 232, 347, 232, 17, 8, 3, 2])
SEG = [0, 7, 13]
SIGMA = [0.3, 0.05]
EINVAL = -22


def _set(K):
    return _policy_set([_agent("bf16", "default", k) for k in range(K)])


def _pink(ps, seg=SEG, lengths=LENGTHS, sigma=SIGMA, **kw):
    from exo_amd.fused import PinkNoise
    return PinkNoise(ps, seg, lengths, sigma, beta=BETA, **kw)


def _policy_of(seg, r):
    return max(p for p in range(len(seg) - 1) if seg[p] <= r)


def _check_rows(pn, spec, rows, seg=SEG, sigma=SIGMA, peak_out=None):
    """rows of pn.seq against sequence_reference of spec [n, A, nf_max, 2] within the bound of the docstring"""
    from exo_amd import pink
    seq = pn.seq.cpu().numpy().astype(np.float64)
    spec = spec.cpu().numpy().astype(np.float64)
    norm = pn.cls_norm.cpu().numpy().astype(np.float64)
    len_cls = pn.len_cls.cpu().numpy()
    worst = 0.0
    for r in rows:
        n = int(pn.lengths_host[r])
        nf = n // 2 + 1
        sg = float(np.float32(sigma[_policy_of(seg, r)]))
        sr, si = spec[r, :, :nf, 0], spec[r, :, :nf, 1]
        want = pink.sequence_reference(sr, si, BETA, n, sg)  # [A, n]
        peak = np.abs(pink.irfft_reference(sr, si, BETA, n)).max()
        w = np.full(nf, 2.0)
        w[0] = 0.0
        if n % 2 == 0:
            w[-1] = 1.0
        S = norm[len_cls[r]] * (np.abs(sr[:, 0]) + ((np.abs(sr) + np.abs(si)) * w).sum(1))
        E = (nf + 16) * 2.0 ** -23 * S.max()
        tol = 2 * sg * E / peak + 4 * 2.0 ** -24 * sg
        err = np.abs(seq[r, :n, :].T - want).max()
        worst = max(worst, err / tol)
        print(f"row {r} n {n}: err {err:.3g} tol {tol:.3g} ratio {err / tol:.3g}")
        assert err <= tol, f"row {r} (n = {n})"
        if peak_out is not None:
            assert abs(float(peak_out[r]) - peak) <= E, f"peak of row {r}"
    return worst


def _given_spectrum(pn, seed):
    """Gaussian spectra with the classes' amplitudes, fp32 [n, A, nf_max, 2]"""
    sc = pn.cls_scale.cpu().numpy()[pn.len_cls.cpu().numpy()]  # [n, nf_max], zero beyond each row's nf
    z = np.random.default_rng(seed).normal(size=(pn.n, A, pn.nf_max, 2))
    return torch.as_tensor((z * sc[:, None, :, None]).astype(np.float32)).to("cuda")


def test_given_spectra_against_the_reference():
    ps = _set(2)
    pn = _pink(ps)
    ones = torch.ones(pn.n, dtype=torch.bool, device="cuda")
    spec = _given_spectrum(pn, 3)
    pn.advance(ones, ones, spectrum=spec)
    torch.cuda.synchronize()
    assert pn.epi.tolist() == [1] * pn.n and pn.t.tolist() == [0] * pn.n
    _check_rows(pn, spec, range(pn.n))
    # a zero spectrum: peak 0, gain 0
    pn.advance(ones, ones, spectrum=torch.zeros_like(spec))
    torch.cuda.synchronize()
    for r in range(pn.n):
        assert not bool(pn.seq[r, :int(LENGTHS[r])].any())


def test_philox_spectra_feed_back_and_are_standard_normal():
    ps = _set(2)
    pn = _pink(ps)
    ones = torch.ones(pn.n, dtype=torch.bool, device="cuda")
    so = torch.full((pn.n, A, pn.nf_max, 2), float("nan"), device="cuda")
    po = torch.full((pn.n,), float("nan"), device="cuda")
    first = pn.seq.clone()
    pn.advance(ones, ones, spec_out=so, peak_out=po)
    torch.cuda.synchronize()
    po_h = po.cpu().numpy().astype(np.float64)
    _check_rows(pn, torch.nan_to_num(so), range(pn.n), peak_out=po_h)
    seq = pn.seq.cpu().numpy().astype(np.float64)
    sc = pn.cls_scale.cpu().numpy().astype(np.float64)[pn.len_cls.cpu().numpy()]
    so_h = so.cpu().numpy().astype(np.float64)
    zs = []
    for r in range(pn.n):
        n = int(LENGTHS[r])
        nf = n // 2 + 1
        sg = float(np.float32(SIGMA[_policy_of(SEG, r)]))
        # the table's own peak is sigma: the peak element is peak * (sigma / peak), two roundings
        assert abs(np.abs(seq[r, :n]).max() - sg) <= 2 * 2.0 ** -24 * sg
        # written exactly where drawn
        assert np.isfinite(so_h[r, :, :nf]).all() and np.isnan(so_h[r, :, nf:]).all()
        zs.append((so_h[r, :, :nf] / sc[r, None, :nf, None]).reshape(-1))
        assert not np.array_equal(seq[r, :n], first[r, :n].cpu().numpy())  # another episode, other draws
    z = np.concatenate(zs)
    N = z.size
    print(f"N {N} mean {z.mean():.4g} var {z.var():.4g}")
    assert abs(z.mean()) <= 6 / np.sqrt(N)
    assert abs(z.var() - 1.0) <= 6 * np.sqrt(2.0 / N)


def test_masks():
    ps = _set(2)
    pn = _pink(ps)
    n = pn.n
    seq0, t0, e0 = pn.seq.clone(), pn.t.clone(), pn.epi.clone()
    done = torch.zeros(n, dtype=torch.bool, device="cuda")
    stepped = torch.zeros(n, dtype=torch.bool, device="cuda")
    done[[1, 5, 9]] = True
    stepped[[0, 5, 6, 12]] = True
    for k in range(2):  # the second launch: t counted on from 1, another episode again
        before = pn.seq.clone()
        pn.advance(stepped, done)
        torch.cuda.synchronize()
        for r in range(n):
            L = int(LENGTHS[r])
            if bool(done[r]):
                assert int(pn.t[r]) == 0 and int(pn.epi[r]) == k + 1
                assert not torch.equal(_bits(pn.seq[r, :L]), _bits(before[r, :L])), f"row {r} kept its episode"
                assert bool(torch.isfinite(pn.seq[r, :L]).all())
                assert torch.equal(_bits(pn.seq[r, L:]), _bits(seq0[r, L:]))  # never written
            else:
                assert torch.equal(_bits(pn.seq[r]), _bits(seq0[r])), f"row {r} changed"
                assert int(pn.epi[r]) == int(e0[r])
                assert int(pn.t[r]) == int(t0[r]) + (k + 1 if bool(stepped[r]) else 0)


def test_segment_independence():
    """the same policy (tag, sigma) in two layouts: bit-identical rows.  The
    layouts hold an empty segment and a 5-row one (a ragged tile of the select launch)."""
    ps = _set(3)
    rng = np.random.default_rng(9)
    big = rng.choice([2, 3, 8, 17, 232, 347], size=33)
    big[:2] = (347, 2)
    small = rng.choice([8, 17, 232], size=5)
    T = [0x1234, 0x1235, 0x1236]
    a = _pink(ps, [0, 5, 5, 38], np.concatenate([small, big]), [0.1, 0.2, 0.3], tags=T)
    # (policy: 5 rows, none, 33 rows) and (33 rows, 5 rows, none)
    b = _pink(ps, [0, 33, 38, 38], np.concatenate([big, small]), [0.3, 0.1, 0.2], tags=[T[2], T[0], T[1]])
    ones = torch.ones(38, dtype=torch.bool, device="cuda")
    for k in range(2):
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.seq[5:38]), _bits(b.seq[0:33])), f"episode {k}: the 33-row policy"
        assert torch.equal(_bits(a.seq[0:5]), _bits(b.seq[33:38])), f"episode {k}: the 5-row policy"
        assert bool(a.seq[5, :347].abs().max() > 0)
        a.advance(ones, ones)
        b.advance(ones, ones)
    # and the rows of one policy differ from each other and from the other policy's
    assert not torch.equal(_bits(a.seq[5, :2]), _bits(a.seq[6, :2]))


def test_argument_errors_launch_nothing():
    from exo_amd import _native as nat
    from exo_amd.fused import PinkNoise
    ps = _set(2)
    with pytest.raises(ValueError, match="lengths"):
        PinkNoise(ps, SEG, LENGTHS[:-1], SIGMA)
    with pytest.raises(ValueError, match="at least 2"):
        PinkNoise(ps, SEG, np.where(LENGTHS == 17, 1, LENGTHS), SIGMA)
    with pytest.raises(ValueError, match="sigma"):
        PinkNoise(ps, SEG, LENGTHS, [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="seg"):
        PinkNoise(ps, [0, 7, 10, 13], LENGTHS, SIGMA)
    pn = _pink(ps)
    torch.cuda.synchronize()
    seq0, t0, e0 = pn.seq.clone(), pn.t.clone(), pn.epi.clone()
    ones = torch.ones(pn.n, dtype=torch.bool, device="cuda")
    with pytest.raises(ValueError, match="stepped"):
        pn.advance(ones[:-1], ones)
    with pytest.raises(ValueError, match="done"):
        pn.advance(ones, ones.float())
    with pytest.raises(ValueError, match="spectrum"):
        pn.advance(ones, ones, spectrum=torch.zeros((pn.n, A, pn.nf_max), device="cuda"))
    with pytest.raises(ValueError, match="peak_out"):
        pn.advance(ones, ones, peak_out=torch.zeros((pn.n + 1,), device="cuda"))

    def call(npol=2, seg=SEG, n=pn.n, a=A, lmax=pn.Lmax, cls=None, done=ones, rows=pn.rows, table=pn.table):
        cls = list(pn.cls_len_host) if cls is None else cls
        rc = nat.lib().td7f_pink_advance(npol, (ctypes.c_int32 * len(seg))(*seg), n, a, lmax, len(cls),
                                         (ctypes.c_int32 * len(cls))(*cls), nat.ptr(ones), nat.ptr(done),
                                         nat.ptr(pn.t), nat.ptr(pn.epi), nat.ptr(pn.seq), nat.ptr(pn.len_cls),
                                         nat.ptr(pn.cls_len), nat.ptr(pn.cls_norm), nat.ptr(pn.cls_scale), rows,
                                         nat.ptr(table), nat.ptr(pn.seg_dev), None, None, None,
                                         nat.stream_ptr(pn.dev))
        torch.cuda.synchronize()
        return rc

    assert call(seg=[0, 7, 12]) == EINVAL          # seg does not end at n
    assert call(seg=[0, 9, 7, 13], npol=3) == EINVAL
    assert call(a=9) == EINVAL                     # wider than the LDS spectrum
    assert call(lmax=1) == EINVAL
    assert call(cls=[2, 3, 8, 17, 232, 348]) == EINVAL  # a class longer than the table's rows
    assert call(cls=[1, 3, 8, 17, 232, 347]) == EINVAL
    assert call(done=None) == EINVAL
    assert call(rows=None) == EINVAL
    assert call(table=None) == EINVAL
    assert call(lmax=20000, cls=[2]) == EINVAL     # the images do not fit the LDS
    nat.lib().td7f_probe(1)
    try:
        assert call() == 0                         # plan-only: valid, nothing launched
    finally:
        nat.lib().td7f_probe(0)
    assert torch.equal(_bits(pn.seq), _bits(seq0)) and torch.equal(pn.t, t0) and torch.equal(pn.epi, e0)
    # a PinkNoise of another set's size, or of another layout
    out = torch.full((pn.n, A), float("nan"), device="cuda")
    obs = torch.zeros((pn.n, 80), device="cuda")
    with pytest.raises(ValueError, match="PinkNoise"):
        _set(3).act(obs, [0, 7, 13, 13], out=out, noise=pn)
    with pytest.raises(ValueError, match="PinkNoise"):
        ps.act(obs, [0, 6, 13], out=out, noise=pn)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
