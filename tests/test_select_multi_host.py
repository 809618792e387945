"""exo_amd.fused.multi_tiles: the tile plan of td7f_select_multi (one launch,
policy p on the rows [seg[p], seg[p+1])).  A workgroup streams one policy's
weights, so a tile may not cross a segment boundary; every row is in exactly
one tile.  Host only (numpy)."""
import numpy as np
import pytest

from exo_amd.fused import multi_tiles


def _check(seg, rows=16):
    seg = np.asarray(seg, dtype=np.int64)
    t = multi_tiles(seg, rows)
    assert t.dtype == np.int32 and t.ndim == 2 and t.shape[1] == 3
    lens = np.diff(seg)
    assert len(t) == int((-(-lens // rows)).sum())          # sum(ceil(len / rows))
    n = int(seg[-1])
    owner = np.repeat(np.arange(len(lens)), lens)           # the policy of every row
    seen = np.zeros(n, dtype=np.int64)
    for p, r0, r1 in t:
        assert 0 <= r0 < r1 <= n and r1 - r0 <= rows        # no empty tile, none longer than `rows`
        assert seg[p] <= r0 and r1 <= seg[p + 1]            # inside policy p's segment
        assert np.all(owner[r0:r1] == p)                    # its policy owns its rows
        assert (r0 - seg[p]) % rows == 0                    # cut from the segment's first row
        assert r1 - r0 == rows or r1 == seg[p + 1]          # only a segment's last tile is ragged
        seen[r0:r1] += 1
    assert np.all(seen == 1)                                # [0, n) exactly once
    if len(t):                                              # in row order: blockIdx.x order is the rows' order
        assert np.all(np.diff(t[:, 1]) > 0)
    return t


def test_hand_cases():
    np.testing.assert_array_equal(_check([0, 37]), [[0, 0, 16], [0, 16, 32], [0, 32, 37]])
    np.testing.assert_array_equal(_check([0, 5, 5, 40, 57]),
                                  [[0, 0, 5], [2, 5, 21], [2, 21, 37], [2, 37, 40], [3, 40, 56], [3, 56, 57]])
    np.testing.assert_array_equal(_check([0, 16, 32]), [[0, 0, 16], [1, 16, 32]])
    np.testing.assert_array_equal(_check([0, 1, 2, 3]), [[0, 0, 1], [1, 1, 2], [2, 2, 3]])
    np.testing.assert_array_equal(_check([0, 0, 0, 17, 17]), [[2, 0, 16], [2, 16, 17]])
    np.testing.assert_array_equal(_check([0, 5], rows=2), [[0, 0, 2], [0, 2, 4], [0, 4, 5]])
    t = _check(np.arange(16) * 800)  # the 15 x 800-env evaluation
    assert len(t) == 15 * 50


def test_empty_segments_give_no_tiles():
    for seg in ([0, 0], [0, 0, 0, 0]):
        t = multi_tiles(seg)
        assert t.shape == (0, 3) and t.dtype == np.int32
    t = _check([0, 0, 20, 20, 20, 21])
    assert set(t[:, 0]) == {1, 4}


def test_random_segs():
    rng = np.random.default_rng(5)
    for k in range(300):
        npol = int(rng.integers(1, 20))
        lens = rng.integers(0, 70, npol)
        lens[rng.uniform(size=npol) < 0.2] = 0
        if k % 3 == 0:
            lens = lens * 16 // max(int(rng.integers(1, 4)), 1)
        _check(np.concatenate([[0], np.cumsum(lens)]), rows=16 if k % 5 else int(rng.integers(1, 40)))


@pytest.mark.parametrize("seg", [[1, 5], [0, 5, 4], [0, -1], [0], [], [[0, 4]], [0.0, 4.0], [0, 2 ** 31]])
def test_bad_seg_raises(seg):
    with pytest.raises(ValueError):
        multi_tiles(seg)


def test_bad_rows_raises():
    with pytest.raises(ValueError):
        multi_tiles([0, 4], rows=0)
