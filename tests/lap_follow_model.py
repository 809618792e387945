"""numpy fp32 model of live views (LAP.view(..., live=True), lap_views_follow)
on top of lap_view_model.Rings / build_tree: per view the leaves, max_priority
and kept of every stratum.  on_insert gives the slots an add_batch wrote the
view's max_priority (kept source) or 0; on_update is lap_update on the view:
the last duplicate's priority per slot, max_priority raised to the largest."""
import numpy as np

from lap_view_model import F, Rings, build_tree, cap_of, view_leaves


class View:
    def __init__(self, E, C, keep):
        self.keep = sorted(int(k) for k in keep)
        self.leaves = np.zeros((E, C), dtype=F)
        self.maxp = F(1)
        self.lost = 0  # kept rows that a foreign or untagged row replaced

    @property
    def kept(self):
        return (self.leaves > 0).sum(1)

    def ready(self):
        return bool((self.kept > 0).all())


class Follow:
    """A buffer of E rings of C slots and its live views, one per entry of keeps."""

    def __init__(self, E, C, keeps):
        self.E, self.C, self.cap = E, C, cap_of(C)
        self.rings = Rings(E, C)
        self.views = [View(E, C, k) for k in keeps]
        self.wraps = np.zeros(E, dtype=np.int64)     # inserts whose span crossed the ring end
        self.idle = 0                                # (call, stratum) pairs that inserted nothing

    def attach(self, keep, base_leaves=None):
        """One more view, built from the rings as they are now (lap_view_build):
        leaf 1 per kept row, or with base_leaves [E, C] (inherit=True) the
        base's leaf and max_priority their maximum -- 1 when no row is kept.
        Returns its index."""
        v = View(self.E, self.C, keep)
        for s in range(self.E):
            vals = np.ones(self.C, dtype=F) if base_leaves is None else base_leaves[s]
            v.leaves[s] = view_leaves(vals, self.rings.source[s], self.rings.size[s], v.keep, True)[0]
        if base_leaves is not None and (v.leaves > 0).any():
            v.maxp = F(v.leaves.max())
        self.views.append(v)
        return len(self.views) - 1

    def add_batch(self, strata, active=None, source=None):
        """Rings.add_batch, then on_insert for the slots it wrote."""
        ptr0 = self.rings.ptr.copy()
        count = np.zeros(self.E, dtype=np.int64)
        written = []  # (stratum, slot, source) in row order
        for i in range(len(strata)):
            s = int(strata[i])
            if (active is None or active[i]) and 0 <= s < self.E:
                written.append((s, int((ptr0[s] + count[s]) % self.C), -1 if source is None else int(source[i])))
                count[s] += 1
        assert count.max(initial=0) <= self.C, "one add_batch must not wrap a ring onto itself"
        self.rings.add_batch(strata, active, source)
        for s in range(self.E):
            assert self.rings.ptr[s] == (ptr0[s] + count[s]) % self.C
            self.idle += count[s] == 0
            self.wraps[s] += 0 < count[s] and ptr0[s] + count[s] > self.C
        self.on_insert(written)
        return written

    def on_insert(self, written):
        for v in self.views:
            for s, slot, src in written:
                new = v.maxp if src in v.keep else F(0)
                v.lost += bool(v.leaves[s, slot] > 0 and new == 0)
                v.leaves[s, slot] = new

    def on_update(self, k, idx, prio):
        """lap_update on view k: idx, prio [E, B]; the last duplicate wins."""
        v = self.views[k]
        prio = np.asarray(prio, dtype=F)
        for s in range(self.E):
            for b in range(idx.shape[1]):
                v.leaves[s, idx[s, b]] = prio[s, b]
        v.maxp = max(v.maxp, F(prio.max()))

    def reset(self):
        self.rings = Rings(self.E, self.C)
        for v in self.views:
            v.leaves[:] = 0
            v.maxp = F(1)

    def tree(self, k):
        """View k's trees, [E, 2 cap]."""
        return np.stack([build_tree(self.views[k].leaves[s], self.cap) for s in range(self.E)])
