"""LAP prioritised replay on the GPU (reference: Agent/TD7_buffer_multi_agent.py).

Storage is fp32 on the device ([strata, max_size + 1, dim]; the extra row per
stratum absorbs writes of inactive envs so batched inserts need no host sync),
priorities are per-stratum sum trees updated and sampled by the HIP kernels in
csrc/lap.hip.  The reference stores float64 numpy arrays and converts every
sampled batch to float32 on the way to the device (:105-111); storing float32
gives the same training inputs.

Two insert paths:
* add(...)       -- one transition, the reference's exact pointer semantics
                    (ptr advances when count % num_envs == 0 BEFORE count is
                    incremented, :59-63);
* add_batch(...) -- one vectorised env step: a ring per stratum, one slot per
                    active env-step (documented divergence);
* add_batch_ref(...) -- one vectorised env step as the training script's
                    per-env add loop (Exoskeleton_agent_train.py:139-142): the
                    reference's shared pointer, kept on the device
                    (lap_store_batch_ref), so a vectorised run fills the buffer
                    slot for slot like the script's sequential adds.
"""
import ctypes
import os

import numpy as np
import torch

from . import _native as nat


class LAP:
    def __init__(self, state_dim, action_dim, device, num_envs, max_size=1e6, batch_size=64, max_action=1,
                 normalize_actions=True, prioritized=True):
        if not prioritized:
            raise NotImplementedError("only the prioritized LAP buffer of the TD7 agent is implemented")
        self.device = nat.require_gpu(device)
        self.max_size = int(max_size)
        self.max_action = max_action
        self.batch_size = int(batch_size)
        self.num_envs = int(num_envs)
        self.state_dim, self.action_dim = state_dim, action_dim
        self.normalize_actions = max_action if normalize_actions else 1
        self.prioritized = True
        E, C = self.num_envs, self.max_size
        if C > 1 << 24:  # csrc/lap.hip prefix_sum walks at most 24 levels
            raise ValueError(f"LAP: max_size {C} above 2^24 rows per stratum")
        f32 = dict(device=self.device, dtype=torch.float32)
        self.state = torch.zeros((E, C + 1, state_dim), **f32)
        self.action = torch.zeros((E, C + 1, action_dim), **f32)
        self.next_state = torch.zeros((E, C + 1, state_dim), **f32)
        self.reward = torch.zeros((E, C + 1, 1), **f32)
        self.not_done = torch.zeros((E, C + 1, 1), **f32)
        cap = 1
        while cap < C:
            cap <<= 1
        self._tree = torch.zeros((E, 2 * cap), **f32)
        self._maxp = torch.ones((1,), **f32)
        self._desc = nat.LapTreeDesc(self._tree.data_ptr(), self._maxp.data_ptr(), E, C, cap)
        self._cap = cap
        # reference pointer semantics (single add)
        self.ptr = 0
        self.count = 0
        self.size = 0
        # per-stratum rings (batched add), device-resident
        i32 = dict(device=self.device, dtype=torch.int32)
        self.ptr_s = torch.zeros((E,), **i32)
        self.size_s = torch.zeros((E,), **i32)
        self._row0 = (torch.arange(E, device=self.device, dtype=torch.int64) * (C + 1))
        self.ind = None
        # reference pointer of add_batch_ref: int64 {ptr, count, size} on the device
        self.ref_state = torch.zeros((3,), dtype=torch.int64, device=self.device)
        self._ref_ws = None
        self.ref_insert_fused = os.environ.get("EXO_REF_INSERT_FUSED", "1") != "0"
        self._u = torch.empty((E, self.batch_size), **f32)
        # sample() draws its uniforms in the kernel (EXO_DEVICE_RNG=0: torch.rand + lap_sample_gather)
        from .ops import DeviceRNG
        self.device_rng = os.environ.get("EXO_DEVICE_RNG", "1") != "0"
        self._rng = DeviceRNG(self.device, 3)
        self._idx = torch.empty((E, self.batch_size), **i32)
        self._store = nat.LapStorageDesc(self.state.data_ptr(), self.action.data_ptr(), self.next_state.data_ptr(),
                                         self.reward.data_ptr(), self.not_done.data_ptr(), state_dim, action_dim,
                                         self.ptr_s.data_ptr(), self.size_s.data_ptr())
        B = E * self.batch_size  # sampled batch, written in place by lap_sample_gather (static for HIP graphs)
        # state and next_state adjacent in one [2, B, dim] buffer: the learner's
        # paired passes over both read it as one tensor (ops.pair_rows), no stack / cat
        sn = torch.empty((2, B, state_dim), **f32)
        self._batch = (sn[0], torch.empty((B, action_dim), **f32), sn[1], torch.empty((B, 1), **f32),
                       torch.empty((B, 1), **f32))
        self._row_ws = None
        self.source = None  # the behaviour-policy column (enable_sources)
        # live views (view(..., live=True)): the attached views, their lap_view_entry
        # table on the device (allocated once: captured inserts keep its pointer),
        # live_generation bumped by every attach / detach (a captured insert holds
        # the number of views: Collector re-records when it moved) and
        # insert_epoch bumped by every insert (a view's pending draw is stale then)
        self._live = []
        self._live_table = None
        self.live_generation = 0
        self.insert_epoch = 0
        self._init_tree()

    def _stream(self):
        return nat.stream_ptr(self.device)

    def _init_tree(self):
        nat.check(nat.lib().lap_init(ctypes.byref(self._desc), self._stream()), "lap_init")

    # --------------------------------------------------------------- views
    @property
    def priority(self):
        """[E, max_size] view of the tree leaves (the reference's self.priority)."""
        return self._tree[:, self._cap:self._cap + self.max_size]

    @property
    def max_priority(self):
        return float(self._maxp)

    @property
    def totals(self):
        return self._tree[:, 1]

    # ---------------------------------------------------------------- adds
    def add(self, state, action, next_state, reward, done, tremor_num):
        """Agent/TD7_buffer_multi_agent.py:49-63."""
        self._no_sources("add")
        s, p = int(tremor_num), self.ptr
        dev = self.device
        self.state[s, p] = torch.as_tensor(np.asarray(state, dtype=np.float32), device=dev)
        self.action[s, p] = torch.as_tensor(np.asarray(action, dtype=np.float32) / self.normalize_actions, device=dev)
        self.next_state[s, p] = torch.as_tensor(np.asarray(next_state, dtype=np.float32), device=dev)
        self.reward[s, p] = float(reward)
        self.not_done[s, p] = 1.0 - float(done)
        st = torch.tensor([s], dtype=torch.int32, device=dev)
        sl = torch.tensor([p], dtype=torch.int32, device=dev)
        nat.check(nat.lib().lap_add(ctypes.byref(self._desc), nat.ptr(st), nat.ptr(sl), 1, self._stream()), "lap_add")
        if self.count % self.num_envs == 0:
            self.ptr = (self.ptr + 1) % self.max_size
            self.size = min(self.size + 1, self.max_size)
        self.count += 1
        self.size_s.fill_(self.size)

    def _step_args(self, state, action, next_state, reward, done, strata, active):
        """One env step's tensors as the insert kernels read them: contiguous
        float32 rows, done and active as uint8 (a bool or uint8 mask is viewed,
        not copied: an in-place mask stays the caller's), strata as int32."""
        n = state.shape[0]

        def f32(t, shape):
            t = t.to(device=self.device, dtype=torch.float32).reshape(shape)
            return t if t.is_contiguous() else t.contiguous()

        def u8(t):
            return t if t.dtype == torch.uint8 else (t.view(torch.uint8) if t.dtype == torch.bool
                                                     else t.to(torch.uint8))

        st = f32(state, (n, self.state_dim))
        nx = f32(next_state, (n, self.state_dim))
        ac = f32(action, (n, self.action_dim))
        rw = f32(reward, (n,))
        dn = u8(done).reshape(n).contiguous()
        sr = (strata if strata.dtype == torch.int32 else strata.to(torch.int32)).contiguous()
        act = None if active is None else u8(active).contiguous()
        return st, ac, nx, rw, dn, sr, act

    # ------------------------------------------- the behaviour-policy column
    def enable_sources(self):
        """Allocate self.source, int32 [E, max_size + 1] filled with -1: the
        behaviour policy of every stored row (-1 = untagged), written by
        add_batch(source=...).  Call it eagerly, before any graph capture;
        idempotent.  Rows already stored stay untagged."""
        if self.source is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LAP.enable_sources: run once eagerly before graph capture")
            self.source = torch.full((self.num_envs, self.max_size + 1), -1, dtype=torch.int32, device=self.device)
        return self.source

    def _no_sources(self, what):
        if self.source is not None:
            raise ValueError(f"LAP.{what}: not on a buffer with a source column (add_batch / load_dataset only)")

    def source_counts(self, K):
        """Stored rows per source id and stratum: int64 [E, K + 1] on the
        device, column K the untagged rows (lap_source_counts, one kernel; ids
        >= K are not counted)."""
        if self.source is None:
            raise ValueError("LAP.source_counts: no source column (enable_sources)")
        out = torch.empty((self.num_envs, int(K) + 1), dtype=torch.int64, device=self.device)
        nat.check(nat.lib().lap_source_counts(ctypes.byref(self._desc), ctypes.byref(self._store),
                                              nat.ptr(self.source), int(K), nat.ptr(out), self._stream()),
                  "lap_source_counts")
        return out

    def view(self, keep, inherit=False, batch_size=None, live=False):
        """A LapView of the rows whose source is in `keep` (see LapView).
        live=True: the view follows this buffer's later inserts (one more
        launch per add_batch while any view is attached) until view.detach();
        the column is enabled if needed and strata may still be empty.  At
        most MAX_LIVE_VIEWS (64) views are attached to one buffer at a time
        (their device table is allocated once): ValueError beyond that."""
        return LapView(self, keep, inherit=inherit, batch_size=batch_size, live=live)

    # ------------------------------------------------------------ live views
    MAX_LIVE_VIEWS = 64

    def _live_check(self, what, attach):
        """The one check of every attach (before anything is built) and detach."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what}: attach and detach live views eagerly, not during graph capture")
        if attach and len(self._live) >= self.MAX_LIVE_VIEWS:
            raise ValueError(f"{what}: at most {self.MAX_LIVE_VIEWS} live views per buffer")

    def _set_live(self, views):
        """self._live = views: the device table rewritten, the generation bumped."""
        self._live = list(views)
        if self._live_table is None:
            self._live_table = torch.zeros((self.MAX_LIVE_VIEWS * ctypes.sizeof(nat.LapViewEntry),), dtype=torch.uint8,
                                           device=self.device)
        rows = (nat.LapViewEntry * self.MAX_LIVE_VIEWS)()  # the entries past the last view stay zero: skipped
        for k, v in enumerate(self._live):
            rows[k] = nat.LapViewEntry(v._tree.data_ptr(), v._maxp.data_ptr(), v._keep.data_ptr(), v._keep.numel(),
                                       v.kept.data_ptr())
        host = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8)
        self._live_table.copy_(host)  # stream-ordered after the inserts issued so far
        self.live_generation += 1

    def note_insert(self):
        """One more insert happened on the device without a call of add_batch:
        a captured add_batch was replayed (Collector's step graphs)."""
        self.insert_epoch += 1

    def _inserted(self, n, source):
        """After add_batch's two launches: the live views follow (lap_views_follow)."""
        self.insert_epoch += 1
        if self._live:
            nat.check(nat.lib().lap_views_follow(ctypes.byref(self._desc), ctypes.byref(self._store),
                                                 nat.ptr(self._row_ws), nat.ptr(source), n,
                                                 nat.ptr(self._live_table), len(self._live), self._stream()),
                      "lap_views_follow")

    def add_batch(self, state, action, next_state, reward, done, strata, active=None, source=None):
        """One vectorised env step: row i goes to stratum strata[i] (int32 [N]) if
        active[i] (bool/uint8 [N], default all) -- lap_store_batch, two kernels
        (and lap_views_follow, a third, while live views are attached), no
        host synchronisation.  source (int32 [N] on the device, values >= 0):
        the behaviour policy of every row, into self.source by the row-copy
        launch (lap_store_batch_src, the same two kernels; the column is
        enabled if needed); without it a buffer that has the column records -1."""
        n = state.shape[0]
        if self._row_ws is None or self._row_ws.numel() < n:
            self._row_ws = torch.empty((n,), dtype=torch.int32, device=self.device)
        st, ac, nx, rw, dn, sr, act = self._step_args(state, action, next_state, reward, done, strata, active)
        if source is not None or self.source is not None:
            self.enable_sources()
            if source is not None:
                if source.dtype != torch.int32 or source.device != self.device or source.numel() != n:
                    raise ValueError(f"add_batch: source must be int32 [{n}] on {self.device}")
                source = source.reshape(n).contiguous()
            nat.check(nat.lib().lap_store_batch_src(ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(st),
                                                    nat.ptr(ac), nat.ptr(nx), nat.ptr(rw), nat.ptr(dn), nat.ptr(sr),
                                                    nat.ptr(act), float(self.normalize_actions), n,
                                                    nat.ptr(self._row_ws), nat.ptr(source), nat.ptr(self.source),
                                                    self._stream()), "lap_store_batch_src")
            self._inserted(n, source)
            return
        nat.check(nat.lib().lap_store_batch(ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(st),
                                            nat.ptr(ac), nat.ptr(nx), nat.ptr(rw), nat.ptr(dn), nat.ptr(sr),
                                            nat.ptr(act), float(self.normalize_actions), n, nat.ptr(self._row_ws),
                                            self._stream()), "lap_store_batch")
        self.insert_epoch += 1

    # ------------------------------------------------------ datasets (offline)
    def load_dataset(self, state, action, next_state, reward, done, strata, chunk=65536, source=None):
        """A dataset of transitions (numpy or torch, host or device; row i to
        stratum strata[i]) through add_batch in row order: ring semantics per
        stratum (a stratum given more rows than max_size keeps the newest),
        priority max_priority, actions divided by normalize_actions.  Chunks
        hold at most `chunk` rows and at most max_size rows of one stratum
        (one add_batch call must not wrap a ring onto itself).  ValueError if
        a stratum is empty afterwards: sample() draws batch_size rows from
        every stratum.  One host read of the ring sizes at the end.  source
        (int [n], values >= 0; export_dataset's key of a buffer with the
        column): the rows' behaviour policies, into self.source."""
        cpu = lambda t: torch.as_tensor(t)  # noqa: E731
        sr = cpu(strata).to(torch.int64).reshape(-1).cpu()
        n = sr.numel()
        if n and (int(sr.min()) < 0 or int(sr.max()) >= self.num_envs):
            raise ValueError(f"load_dataset: strata outside 0..{self.num_envs - 1}")
        cols = [cpu(state).reshape(n, self.state_dim), cpu(action).reshape(n, self.action_dim),
                cpu(next_state).reshape(n, self.state_dim), cpu(reward).reshape(n), cpu(done).reshape(n)]
        cols[4] = cols[4].to(torch.uint8) if cols[4].dtype != torch.bool else cols[4]
        if source is not None:
            source = cpu(source).reshape(n).to(torch.int32)
        for lo, hi in self._dataset_chunks(sr, int(chunk)):
            s, a, s2, r, d = (c[lo:hi].to(self.device) for c in cols)
            self.add_batch(s, a, s2, r, d, sr[lo:hi].to(device=self.device, dtype=torch.int32),
                           source=None if source is None else source[lo:hi].to(self.device))
        empty = (self.size_s == 0).nonzero().reshape(-1).tolist()
        if empty:
            raise ValueError(f"load_dataset: no rows for strata {empty} (every stratum is sampled)")

    def _dataset_chunks(self, strata, chunk):
        """[lo, hi) row ranges of load_dataset: <= chunk rows, <= max_size rows of one stratum."""
        n, C = strata.numel(), self.max_size
        if n == 0:
            return []
        # rank of every row inside its stratum, in row order
        rank = torch.zeros(n, dtype=torch.int64)
        for s in range(self.num_envs):
            m = strata == s
            rank[m] = torch.arange(int(m.sum()))
        out, lo = [], 0
        base = torch.zeros(self.num_envs, dtype=torch.int64)  # ranks at the chunk's start
        while lo < n:
            hi = min(lo + max(chunk, 1), n)
            over = (rank[lo:hi] - base[strata[lo:hi]] >= C).nonzero()
            if over.numel():
                hi = lo + int(over[0])
            out.append((lo, hi))
            base.scatter_reduce_(0, strata[lo:hi], rank[lo:hi] + 1, "amax")
            lo = hi
        return out

    def export_dataset(self):
        """The rows the per-stratum rings hold, oldest first per stratum (after
        a wrap too), as CPU tensors: state, action (de-normalised), next_state,
        reward [n], done [n] (uint8), strata [n] (int32), and source [n] (int32)
        when the buffer has the column.  load_dataset(**it) into a fresh
        buffer of the same capacity holds the same rows."""
        C = self.max_size
        size, ptr = self.size_s.cpu().tolist(), self.ptr_s.cpu().tolist()
        rows, strata = [], []
        for s in range(self.num_envs):
            slots = (ptr[s] - size[s] + torch.arange(size[s], dtype=torch.int64)) % C
            rows.append(s * (C + 1) + slots)
            strata.append(torch.full((size[s],), s, dtype=torch.int32))
        rows = torch.cat(rows).to(self.device)
        take = lambda t: t.reshape(-1, t.shape[-1]).index_select(0, rows).cpu()  # noqa: E731
        out = dict(state=take(self.state), action=take(self.action) * self.normalize_actions,
                   next_state=take(self.next_state), reward=take(self.reward).reshape(-1),
                   done=(1.0 - take(self.not_done).reshape(-1)).to(torch.uint8), strata=torch.cat(strata))
        if self.source is not None:  # int32 [n], -1 = untagged
            out["source"] = self.source.reshape(-1).index_select(0, rows).cpu()
        return out

    def add_batch_ref(self, state, action, next_state, reward, done, strata, active=None, advance=None):
        """LAP.add (:49-63) for every active row in row order -- the training
        script's per-env loop over one vectorised step -- with the reference's
        shared pointer (ref_state, device-resident): env 0's first transition
        one slot behind the others, a done env's slot re-used by the next adds,
        one shared sampling size.  One kernel (lap_store_batch_ref_fused, r04;
        EXO_REF_INSERT_FUSED=0: the three launches of lap_store_batch_ref), no
        host synchronisation.  advance = (table, k, count, score): the
        trainer's mask advance in the same launch (lap_store_batch_ref_fused_adv;
        `active` is then advanced in place, the rewards added into score)."""
        self._no_sources("add_batch_ref")
        n = state.shape[0]
        if self._ref_ws is None or self._ref_ws.numel() < 3 * n:
            # zeroed: its first word is the fused launch's ticket (left zero)
            self._ref_ws = torch.zeros((3 * n,), dtype=torch.int32, device=self.device)
        st, ac, nx, rw, dn, sr, act = self._step_args(state, action, next_state, reward, done, strata, active)
        if advance is not None:
            if not self.ref_insert_fused or act is None or act.data_ptr() != active.data_ptr():
                raise ValueError("add_batch_ref(advance=...): the fused insert and an in-place uint8/bool mask only")
            table, k, count, score = advance
            nat.check(nat.lib().lap_store_batch_ref_fused_adv(
                ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(self.ref_state), nat.ptr(st),
                nat.ptr(ac), nat.ptr(nx), nat.ptr(rw), nat.ptr(dn), nat.ptr(sr), nat.ptr(act),
                float(self.normalize_actions), n, nat.ptr(self._ref_ws), nat.ptr(table), table.shape[0], nat.ptr(k),
                nat.ptr(count), nat.ptr(score), self._stream()), "lap_store_batch_ref_fused_adv")
            return
        fn = "lap_store_batch_ref_fused" if self.ref_insert_fused else "lap_store_batch_ref"
        nat.check(getattr(nat.lib(), fn)(ctypes.byref(self._desc), ctypes.byref(self._store),
                                         nat.ptr(self.ref_state), nat.ptr(st), nat.ptr(ac), nat.ptr(nx),
                                         nat.ptr(rw), nat.ptr(dn), nat.ptr(sr), nat.ptr(act),
                                         float(self.normalize_actions), n, nat.ptr(self._ref_ws),
                                         self._stream()), fn)

    # ----------------------------------------------- planned reference inserts
    # (lap_ref_plan / lap_ref_step / lap_ref_commit, csrc/lap.hip): a whole
    # synchronous episode round of add_batch_ref calls planned at its start --
    # the steps' envs come from a fixed mask table -- so a step is one
    # elementwise launch and the tree is updated once, at ref_commit.  Bit
    # for bit the per-step inserts' rows, leaves, sums, pointer and sizes,
    # provided nothing reads the tree between ref_plan and ref_commit.
    def ref_plan(self, table, strata, offs, total, plan):
        """plan[k][e] (int32 [rows][n]) for the mask table rows (uint8/bool
        [rows][n]); offs: int64 device [rows], the adds before each row."""
        self._no_sources("ref_plan")
        rows, n = table.shape
        if getattr(self, "_ref_add_ws", None) is None or self._ref_add_ws.numel() < max(int(total), 1):
            self._ref_add_ws = torch.empty((max(int(total), 1),), dtype=torch.int32, device=self.device)
        tb = table.view(torch.uint8) if table.dtype == torch.bool else table
        sr = (strata if strata.dtype == torch.int32 else strata.to(torch.int32)).contiguous()
        nat.check(nat.lib().lap_ref_plan(ctypes.byref(self._desc), nat.ptr(self.ref_state), nat.ptr(tb), rows, n,
                                         nat.ptr(sr), nat.ptr(offs), int(total), nat.ptr(self._ref_add_ws),
                                         nat.ptr(plan), self._stream()), "lap_ref_plan")

    def ref_step(self, plan, table, kk, par, state, action, next_state, reward, done, strata, active,
                 k_dev=None, count=None, counts_table=None, score=None):
        """One step of a planned round (see ref_plan): the transitions to their
        planned slots, score += reward where active, the next mask in place."""
        self._no_sources("ref_step")
        rows, n = plan.shape
        tb = table.view(torch.uint8) if table.dtype == torch.bool else table
        dn = done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)
        act = active.view(torch.uint8) if active.dtype == torch.bool else active
        nat.check(nat.lib().lap_ref_step(
            ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(plan), rows, n, nat.ptr(kk), int(par),
            nat.ptr(k_dev), nat.ptr(strata), nat.ptr(state.contiguous()), nat.ptr(action.contiguous()),
            nat.ptr(next_state.contiguous()), nat.ptr(reward.contiguous()), nat.ptr(dn.contiguous()),
            float(self.normalize_actions), nat.ptr(tb), nat.ptr(act), nat.ptr(count), nat.ptr(counts_table),
            nat.ptr(score), self._stream()), "lap_ref_step")

    def ref_commit(self, plan, strata, total):
        """The end of a planned round: leaves, the round's span, the pointer."""
        self._no_sources("ref_commit")
        rows, n = plan.shape
        nat.check(nat.lib().lap_ref_commit(ctypes.byref(self._desc), ctypes.byref(self._store),
                                           nat.ptr(self.ref_state), nat.ptr(plan), rows, n, nat.ptr(strata),
                                           int(total), self._stream()), "lap_ref_commit")

    def ref_pointer(self):
        """(ptr, count, size) of add_batch_ref (host sync)."""
        return tuple(int(v) for v in self.ref_state.cpu())

    # ------------------------------------------------------------- sample
    def _slot(self, slot):
        """Batch buffers of sample(slot=...): the vectorised trainer samples the
        next iteration's batch into the other slot while this one is in use."""
        if slot is None:
            return self._batch, self._idx
        if not hasattr(self, "_slots"):
            self._slots = {}
        if slot not in self._slots:
            f32 = dict(device=self.device, dtype=torch.float32)
            B, (S, A) = self._batch[0].shape[0], (self._batch[0].shape[1], self._batch[1].shape[1])
            sn = torch.empty((2, B, S), **f32)
            self._slots[slot] = ((sn[0], torch.empty((B, A), **f32), sn[1], torch.empty((B, 1), **f32),
                                  torch.empty((B, 1), **f32)), torch.empty_like(self._idx))
        return self._slots[slot]

    def sample(self, slot=None):
        """Agent/TD7_buffer_multi_agent.py:65-111: batch_size rows from every
        stratum, stratum-major, as float32 device tensors (lap_sample_gather:
        descent + gather in one kernel; the returned tensors are reused by the
        next call with the same slot).  self.ind = the sampled indices."""
        batch, idx = self._slot(slot)
        if self.device_rng:
            # the uniforms drawn inside the kernel (ops.DeviceRNG): no generator launch
            r = self._rng
            nat.check(nat.lib().lap_sample_gather_rng(ctypes.byref(self._desc), ctypes.byref(self._store), r.seed,
                                                      r.tag, r.counter_ptr, r.ticket_ptr, self.batch_size,
                                                      nat.ptr(idx), *[nat.ptr(t) for t in batch],
                                                      self._stream()), "lap_sample_gather_rng")
        else:
            self._u.uniform_()
            nat.check(nat.lib().lap_sample_gather(ctypes.byref(self._desc), ctypes.byref(self._store),
                                                  nat.ptr(self._u), self.batch_size, nat.ptr(idx),
                                                  *[nat.ptr(t) for t in batch], self._stream()),
                      "lap_sample_gather")
        self.ind = idx
        return batch

    def sample_indices(self, u):
        """Indices for given uniforms u [E, batch] (parity hook)."""
        u = u.to(device=self.device, dtype=torch.float32).contiguous()
        idx = torch.empty(u.shape, dtype=torch.int32, device=self.device)
        nat.check(nat.lib().lap_sample(ctypes.byref(self._desc), nat.ptr(u), nat.ptr(self.size_s), u.shape[1],
                                       nat.ptr(idx), self._stream()), "lap_sample")
        return idx

    def update_priority(self, priority, ind=None):
        """:113-117 (max_priority stays on the device)."""
        ind = self.ind if ind is None else ind
        pr = priority.detach().to(torch.float32).reshape(-1).contiguous()
        assert pr.numel() == ind.numel()
        nat.check(nat.lib().lap_update(ctypes.byref(self._desc), nat.ptr(ind), nat.ptr(pr), ind.shape[1],
                                       self._stream()), "lap_update")

    # LAP.update_priority + the next sample as one launch (lap_update_sample_rng,
    # r04); EXO_LAP_FUSED=0: the two launches
    fuse_update_sample = os.environ.get("EXO_LAP_FUSED", "1") != "0"

    def update_priority_and_sample(self, priority, ind=None, slot=None, before_gather=None):
        """update_priority(priority, ind) then sample(slot), the same values; one
        launch with the device RNG (the sampled batch in the slot's buffers,
        self.ind = its indices).  before_gather (a callable, r05): two launches
        instead -- the update and the indices, then before_gather() (the caller's
        stream waits), then the rows gathered (lap_update_sample_idx +
        lap_gather_rows, bit-identical)."""
        ind = self.ind if ind is None else ind
        if not (self.device_rng and self.fuse_update_sample and self.batch_size <= 1024):
            self.update_priority(priority, ind)
            if before_gather is not None:
                before_gather()
            return self.sample(slot)
        pr = priority.detach().to(torch.float32).reshape(-1).contiguous()
        assert pr.numel() == ind.numel()
        batch, idx = self._slot(slot)
        r = self._rng
        if before_gather is not None:
            nat.check(nat.lib().lap_update_sample_idx(ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(ind),
                                                      nat.ptr(pr), ind.shape[1], r.seed, r.tag, r.counter_ptr,
                                                      r.ticket_ptr, nat.ptr(idx), self._stream()),
                      "lap_update_sample_idx")
            before_gather()
            nat.check(nat.lib().lap_gather_rows(ctypes.byref(self._desc), ctypes.byref(self._store), ind.shape[1],
                                                nat.ptr(idx), *[nat.ptr(t) for t in batch], self._stream()),
                      "lap_gather_rows")
            self.ind = idx
            return batch
        nat.check(nat.lib().lap_update_sample_rng(ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(ind),
                                                  nat.ptr(pr), ind.shape[1], r.seed, r.tag, r.counter_ptr,
                                                  r.ticket_ptr, nat.ptr(idx), *[nat.ptr(t) for t in batch],
                                                  self._stream()), "lap_update_sample_rng")
        self.ind = idx
        return batch

    def update_priority_and_sample_td(self, td, alpha, min_priority, ind, slot, prio_out=None):
        """update_priority_and_sample with the priorities computed in the launch
        from the critic pass's |td| [B, 2] (lap_update_sample_td): the same
        values as td7f_wgrad's, so the update needs only the critic pass."""
        if not (self.device_rng and self.batch_size <= 1024):
            raise RuntimeError("update_priority_and_sample_td: the device RNG and batch <= 1024 only")
        batch, idx = self._slot(slot)
        r = self._rng
        nat.check(nat.lib().lap_update_sample_td(ctypes.byref(self._desc), ctypes.byref(self._store), nat.ptr(ind),
                                                 nat.ptr(td), float(alpha), float(min_priority), nat.ptr(prio_out),
                                                 ind.shape[1], r.seed, r.tag, r.counter_ptr, r.ticket_ptr,
                                                 nat.ptr(idx), *[nat.ptr(t) for t in batch], self._stream()),
                  "lap_update_sample_td")
        self.ind = idx
        return batch

    def reset_max_priority(self):
        nat.check(nat.lib().lap_reset_max(ctypes.byref(self._desc), self._stream()), "lap_reset_max")

    def reset_buffer(self):
        """:122-139"""
        self.ptr = self.count = self.size = 0
        for t in (self.state, self.action, self.next_state, self.reward, self.not_done):
            t.zero_()
        self.ptr_s.zero_()
        self.size_s.zero_()
        self.ref_state.zero_()
        if self.source is not None:
            self.source.fill_(-1)
        self._init_tree()
        self.insert_epoch += 1
        for v in self._live:  # every attached view empty again: zero trees, kept 0, max_priority 1
            v._init_tree()
            v.kept.zero_()


class LapView(LAP):
    """LAP.view(keep, inherit=False, batch_size=None): the rows of `base`
    whose source id is in `keep`, as a replay of their own for the learner
    (Agent.use_replay, OfflineTrainer).  The view shares the base's row
    tensors, source column and ring state (ptr_s / size_s) -- no row is copied
    -- and owns a second set of sum trees (lap_view_build: the leaf of a
    foreign or untagged row is 0, so no descent reaches it), its max_priority,
    DeviceRNG stream, batch slots and ind.  sample, sample_indices,
    update_priority, update_priority_and_sample(_td), reset_max_priority,
    priority, max_priority and totals are LAP's, on the view's trees; the
    base's priorities are neither read (inherit=False: every kept row starts at
    priority 1, max_priority 1; inherit=True: at the base's leaf, max_priority
    their maximum) nor written afterwards.

    live=False: the view is a snapshot of the base at view() / rebuild(): rows
    inserted into the base afterwards are not in it (a wrapped ring may even
    overwrite a kept row with a foreign one).  rebuild() runs the build again
    from the base as it is then, which also discards the view's learned
    priorities.  ValueError if a stratum keeps no row (one host read of
    source_counts): sample() draws from every stratum.

    live=True: the view is attached to the base and follows its inserts.
    Every add_batch / load_dataset of the base issues one more launch
    (lap_views_follow, for all attached views together) that touches only the
    leaves the insert wrote: a new kept row enters at the view's own
    max_priority (LAP's rule for add; for inherit=True views too -- the base's
    leaf is read by the build only), a foreign or untagged row gets 0, which
    also removes a kept row the ring evicted.  The priorities the learner has
    written to the other rows stay.  The view may be taken from an empty or
    partly filled buffer (the column is enabled if needed): self.kept (int32
    [E], on the device) counts the rows with a positive leaf per stratum and
    ready() -- one host read -- says whether every stratum keeps one; sample
    only then.  kept moves with inserts only: priorities written to a live view
    must be > 0 (TD7's are, min_priority ** alpha at least), a 0 would hide the
    row while kept still counts it.  A view that keeps no row when it is built
    starts at max_priority 1, with inherit=True too (the inherit build's
    maximum over no leaf is replaced by LAP's initial value).
    If reset_max_priority runs on a view that keeps no row its
    max_priority is 0 until the next update_priority, and rows inserted
    meanwhile are not reachable.  base.reset_buffer() empties the attached
    views with it.  detach() ends the following: the view is a snapshot from
    then on.  Attach and detach eagerly, never during graph capture; a captured
    add_batch holds the number of attached views (Collector re-records its
    step graphs when base.live_generation moved).

    A draw made before an insert may name a slot that now holds another row:
    `stale` is true when the base has taken rows since this view last sampled,
    and update_priority / update_priority_and_sample(_td) raise ValueError for
    the view's own index buffer of such a draw (writing a priority there could
    make a foreign row reachable).  Sample again instead; dropping a pending
    draw is harmless, its rows keep their priorities.

    Inserts, reset_buffer and load_dataset raise on a view."""

    def __init__(self, base, keep, inherit=False, batch_size=None, live=False):
        if isinstance(base, LapView):
            raise ValueError("LAP.view: take the view from the base buffer")
        if live:
            base._live_check("LAP.view(live=True)", attach=True)  # before anything is built
            base.enable_sources()
        if base.source is None:
            raise ValueError("LAP.view: the buffer has no source column (enable_sources / add_batch(source=...))")
        keep = sorted({int(k) for k in keep})
        if not keep or keep[0] < 0:
            raise ValueError("LAP.view: keep must list source ids >= 0")
        self.base, self.keep, self.inherit = base, keep, bool(inherit)
        for name in ("device", "max_size", "max_action", "num_envs", "state_dim", "action_dim", "normalize_actions",
                     "prioritized", "state", "action", "next_state", "reward", "not_done", "ptr_s", "size_s", "source",
                     "_store", "_cap", "device_rng"):
            setattr(self, name, getattr(base, name))
        self.batch_size = int(batch_size if batch_size is not None else base.batch_size)
        E, C, cap = self.num_envs, self.max_size, self._cap
        f32 = dict(device=self.device, dtype=torch.float32)
        i32 = dict(device=self.device, dtype=torch.int32)
        self._tree = torch.zeros((E, 2 * cap), **f32)
        self._maxp = torch.ones((1,), **f32)
        self._desc = nat.LapTreeDesc(self._tree.data_ptr(), self._maxp.data_ptr(), E, C, cap)
        table = torch.zeros(keep[-1] + 1, dtype=torch.uint8)
        table[keep] = 1
        self._keep = table.to(self.device)
        self.ind = None
        self._u = torch.empty((E, self.batch_size), **f32)
        from .ops import DeviceRNG
        self._rng = DeviceRNG(self.device, 3)
        self._idx = torch.empty((E, self.batch_size), **i32)
        B = E * self.batch_size
        sn = torch.empty((2, B, self.state_dim), **f32)
        self._batch = (sn[0], torch.empty((B, self.action_dim), **f32), sn[1], torch.empty((B, 1), **f32),
                       torch.empty((B, 1), **f32))
        self.kept = torch.zeros((E,), **i32)  # rows with a positive leaf, per stratum
        self.live = bool(live)
        self._drawn = {}   # index buffer -> the base's insert epoch at its draw (live views)
        self._seen = None  # the insert epoch at the last draw
        self.rebuild()
        if self.live:
            base._set_live(base._live + [self])

    def rebuild(self):
        """Build the view's trees again from the base as it is now (kept with
        them); a live view stays attached."""
        counts = self.base.source_counts(self._keep.numel())[:, :-1].cpu()
        kept = counts[:, self.keep].sum(1)
        empty = (kept == 0).nonzero().reshape(-1).tolist()
        if empty and not self.live:
            raise ValueError(f"LAP.view: no rows of sources {self.keep} in strata {empty} (every stratum is sampled)")
        self.kept.copy_(kept.to(torch.int32))
        nat.check(nat.lib().lap_view_build(ctypes.byref(self._desc), ctypes.byref(self.base._desc),
                                           ctypes.byref(self._store), nat.ptr(self.source), nat.ptr(self._keep),
                                           self._keep.numel(), int(self.inherit), self._stream()), "lap_view_build")
        if self.inherit and int(kept.sum()) == 0:
            # the inherit build leaves max_priority = the largest kept leaf, 0 when no
            # row is kept yet (a live view of an empty buffer): LAP's initial 1 instead,
            # or every row that enters later would get the leaf 0
            self._maxp.fill_(1.0)
        return self

    def ready(self):
        """Every stratum keeps at least one row (one host read of self.kept)."""
        return bool((self.kept > 0).all())

    def detach(self):
        """End the following: the view is a snapshot of the base from now on."""
        if self.live:
            self.base._live_check("LapView.detach", attach=False)
            self.base._set_live([v for v in self.base._live if v is not self])
            self.live = False
            self._drawn, self._seen = {}, None
        return self

    # ------------------------------------------------------ pending draws
    @property
    def stale(self):
        """The base has taken rows since this live view last sampled."""
        return self.live and self._seen is not None and self._seen != self.base.insert_epoch

    def note_draw(self, slot=None):
        """The batch slot was drawn into just now without a call of sample():
        a captured update_priority_and_sample was replayed (OfflineTrainer)."""
        self._note(self._slot(slot)[1])

    def _note(self, idx):
        if self.live:
            self._seen = self._drawn[idx.data_ptr()] = self.base.insert_epoch

    def _fresh(self, ind, what):
        ind = self.ind if ind is None else ind
        if self.live and ind is not None and self._drawn.get(ind.data_ptr(), self.base.insert_epoch) != \
                self.base.insert_epoch:
            raise ValueError(f"LapView.{what}: the base has taken rows since these indices were drawn (the slots may "
                             "hold other rows now): sample() again")
        return ind

    def sample(self, slot=None):
        batch = super().sample(slot)
        self._note(self.ind)
        return batch

    def update_priority(self, priority, ind=None):
        super().update_priority(priority, self._fresh(ind, "update_priority"))

    def update_priority_and_sample(self, priority, ind=None, slot=None, before_gather=None):
        batch = super().update_priority_and_sample(priority, self._fresh(ind, "update_priority_and_sample"), slot,
                                                   before_gather)
        self._note(self.ind)
        return batch

    def update_priority_and_sample_td(self, td, alpha, min_priority, ind, slot, prio_out=None):
        batch = super().update_priority_and_sample_td(td, alpha, min_priority,
                                                      self._fresh(ind, "update_priority_and_sample_td"), slot,
                                                      prio_out)
        self._note(self.ind)
        return batch

    def _not_on_a_view(self, *a, **k):
        raise ValueError("LapView: a view is read-only storage (insert into, reset or load the base buffer, "
                         "then rebuild())")

    add = add_batch = add_batch_ref = ref_plan = ref_step = ref_commit = _not_on_a_view
    load_dataset = reset_buffer = enable_sources = view = _not_on_a_view
