"""numpy fp32 models of what csrc/lap.hip computes for a sum tree, shared by the
view and source-column tests: the pairwise tree, prefix_sum, the descent (the
rule before and after the `left > 0` term), and the per-stratum rings of
add_batch with a source column."""
import numpy as np

F = np.float32


def cap_of(capacity):
    cap = 1
    while cap < capacity:
        cap <<= 1
    return cap


def build_tree(leaves, cap):
    """T[cap + i] = leaves[i], every internal node T[2n] + T[2n + 1] in fp32, T[0] = 0."""
    T = np.zeros(2 * cap, dtype=F)
    T[cap:cap + len(leaves)] = np.asarray(leaves, dtype=F)
    w = cap
    while w > 1:
        w >>= 1
        T[w:2 * w] = T[2 * w:4 * w:2] + T[2 * w + 1:4 * w:2]
    return T


def prefix_sum(T, cap, sz):
    """Sum of the leaves [0, sz): the walk towards leaf sz adding every left sibling."""
    if sz >= cap:
        return F(T[1])
    levels = cap.bit_length() - 1
    acc = F(0)
    for j in range(levels):
        lv = levels - 1 - j
        x = T[2 * ((1 << j) | (sz >> (lv + 1)))]
        acc = F(acc + (x if (sz >> lv) & 1 else F(0)))
    return acc


def descend(T, cap, val, amended=True):
    val, node = F(val), 1
    while node < cap:
        left, right = T[2 * node], T[2 * node + 1]
        go_left = (val <= left and left > 0) or right <= 0 if amended else (val <= left or right <= 0)
        if go_left:
            node = 2 * node
        else:
            val = F(val - left)
            node = 2 * node + 1
    return node - cap


def sample_index(T, cap, sz, u, amended=True):
    """lap_sample for one uniform u (fp32)."""
    i = descend(T, cap, F(u) * prefix_sum(T, cap, sz), amended)
    if i >= sz:
        i = sz - 1 if sz > 0 else 0
    return i


def searchsorted_left(leaves, u):
    """The reference's index: searchsorted_left(cumsum(leaves), u * sum(leaves)),
    leaves integer-valued (every sum exact in fp32)."""
    c = np.cumsum(np.asarray(leaves, dtype=np.float64))
    return int(np.searchsorted(c, float(F(u) * F(c[-1])), side="left"))


def view_leaves(base_leaves, source, size, keep, inherit):
    """One stratum's view leaves: base leaf (inherit) or 1 where slot < size and source in keep."""
    source = np.asarray(source)
    kept = (np.arange(len(source)) < size) & np.isin(source, list(keep)) & (source >= 0)
    vals = np.asarray(base_leaves, dtype=F) if inherit else np.ones(len(source), dtype=F)
    return np.where(kept, vals, F(0)).astype(F), kept


def make_calls(seed, E, S, A, calls, n, probs, K, bad_stratum=None):
    """`calls` add_batch calls of n rows as numpy arrays: strata drawn with
    `probs`, about 4 in 5 rows active, sources 0..K-1; bad_stratum: the
    stratum given to row 3 of every call (out of range)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(calls):
        strata = rng.choice(E, size=n, p=probs).astype(np.int32)
        if bad_stratum is not None:
            strata[3] = bad_stratum
        out.append(dict(state=rng.normal(0, 1, (n, S)).astype(F), action=rng.uniform(-1, 1, (n, A)).astype(F),
                        next_state=rng.normal(0, 1, (n, S)).astype(F), reward=rng.uniform(-2, 3, n).astype(F),
                        done=rng.uniform(0, 1, n) < 0.1, strata=strata, active=rng.uniform(0, 1, n) < 0.8,
                        source=rng.integers(0, K, n).astype(np.int32)))
    return out


class Rings:
    """add_batch's rings: row i of a call goes to the next slot of stratum
    strata[i] when active[i] and the stratum is in range, in row order.
    row[s, slot] = the global number of the row stored there (-1: empty),
    source[s, slot] = its source (-1: untagged)."""

    def __init__(self, E, C):
        self.E, self.C = E, C
        self.ptr = np.zeros(E, dtype=np.int64)
        self.size = np.zeros(E, dtype=np.int64)
        self.row = np.full((E, C), -1, dtype=np.int64)
        self.source = np.full((E, C), -1, dtype=np.int32)
        self.rows_seen = 0

    def add_batch(self, strata, active=None, source=None):
        n = len(strata)
        for i in range(n):
            s = int(strata[i])
            if (active is None or active[i]) and 0 <= s < self.E:
                p = self.ptr[s]
                self.row[s, p] = self.rows_seen + i
                self.source[s, p] = -1 if source is None else source[i]
                self.ptr[s] = (p + 1) % self.C
                self.size[s] = min(self.size[s] + 1, self.C)
        self.rows_seen += n
