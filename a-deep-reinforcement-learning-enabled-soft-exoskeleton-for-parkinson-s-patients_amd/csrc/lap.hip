// lap.hip -- LAP prioritised replay (Agent/TD7_buffer_multi_agent.py) as
// per-stratum binary sum trees on gfx950.
//
// The reference keeps one priority row per env ("stratum", :41) and samples
// batch_size indices from every row with torch.cumsum + torch.searchsorted
// (:75-78): O(size) work and a host sync per row per training step.  Here
// every stratum owns a complete binary tree over `cap` (power of two) leaves,
// tree[s][1] is the row total and leaf i lives at tree[s][cap + i].  The
// caller owns the memory (torch tensors) and describes it with lap_tree_desc:
//   sample : one lane per draw descends log2(cap) levels,
//   update : leaves are written (last duplicate wins, like the reference's CPU
//            index_put at :115), then the touched ancestors are recomputed
//            level by level inside one workgroup per stratum (deterministic:
//            a parent is always left + right of final children),
//   max    : max_priority lives in device memory (no host sync, :116, :120).
// For integer-valued priorities the descent returns exactly
// searchsorted_left(cumsum(p), u * sum(p)).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "lap_chain.h"
#include "philox.h"
#include "exo_amd.h"

namespace {

constexpr int UPD_THREADS = 1024;

__device__ __forceinline__ float *stratum_tree(float *tree, int s, int cap) { return tree + (size_t)s * 2 * cap; }

// Recompute the ancestors of the n leaves slot[0..n) of one stratum, bottom-up,
// one level per barrier.  The lower levels work in global memory; once every
// parent of a level is below TOPN/2 the top of the tree (nodes [1, TOPN), the
// parents and their children) is staged in LDS and the remaining levels (12 of
// the 18 of a 250k-slot stratum) run there -- one L2 round trip per level
// fewer -- and the recomputed nodes [1, TOPN/2) are written back.  The same
// additions in the same order: the sums are bit-identical.
constexpr int TOPN = 8192;
// top: the caller's LDS array of NTOP floats; on return (true) it holds the
// final nodes [1, min(NTOP, 2 cap)) (false: no level was staged, T holds them).
// The staging loads are all issued before their LDS stores (one round trip).
template <int NTOP = TOPN>
__device__ bool propagate_top(float *T, int cap, int levels, const int32_t *slot, int n, float *top) {
    int lv = 1;
    for (; lv <= levels && ((2 * cap) >> lv) > NTOP / 2; ++lv) {
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            const int node = (cap + slot[k]) >> lv;
            T[node] = T[2 * node] + T[2 * node + 1];
        }
    }
    __syncthreads();
    if (lv > levels) return false;
    const int lim = min(NTOP, 2 * cap);
    if (blockDim.x == UPD_THREADS) {
        constexpr int PER = NTOP / UPD_THREADS;
        float v[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + j * UPD_THREADS;
            v[j] = i < lim ? T[i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = threadIdx.x + j * UPD_THREADS;
            if (i < lim) top[i] = v[j];
        }
    } else {
        for (int i = threadIdx.x; i < lim; i += blockDim.x) top[i] = T[i];
    }
    for (; lv <= levels; ++lv) {
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += blockDim.x) {
            const int node = (cap + slot[k]) >> lv;
            top[node] = top[2 * node] + top[2 * node + 1];
        }
    }
    __syncthreads();
    const int wb = min(NTOP / 2, cap);
    for (int i = 1 + threadIdx.x; i < wb; i += blockDim.x) T[i] = top[i];
    __syncthreads();
    return true;
}
__device__ void propagate(float *T, int cap, int levels, const int32_t *slot, int n) {
    __shared__ float top[TOPN];
    propagate_top(T, cap, levels, slot, n, top);
}

// The same recomputation for the leaves of a ring span: `count` consecutive
// slots from `first`, wrapping at `capacity` (all of them once count reaches
// it).  The ancestors of a contiguous leaf range at one level are a contiguous
// node range, so each level is a loop over (at most two) node ranges instead
// of a per-slot list; the nodes recomputed, and every sum, are the ones
// propagate computes for the same slots.
__device__ void propagate_span(float *T, int cap, int levels, int capacity, int first, int count) {
    __shared__ float top[TOPN];
    if (count <= 0) return;
    int a0 = first, e0 = first + count, a1 = 0, e1 = 0;  // [a0, e0) and [a1, e1)
    if (count >= capacity) {
        a0 = 0;
        e0 = capacity;
    } else if (e0 > capacity) {
        e1 = e0 - capacity;
        e0 = capacity;
    }
    int lv = 1;
    for (; lv <= levels && ((2 * cap) >> lv) > TOPN / 2; ++lv) {
        __syncthreads();
        const int lo0 = (cap + a0) >> lv, n0 = ((cap + e0 - 1) >> lv) - lo0 + 1;
        const int lo1 = (cap + a1) >> lv, n1 = e1 > a1 ? ((cap + e1 - 1) >> lv) - lo1 + 1 : 0;
        for (int k = threadIdx.x; k < n0 + n1; k += blockDim.x) {
            const int node = k < n0 ? lo0 + k : lo1 + k - n0;
            T[node] = T[2 * node] + T[2 * node + 1];
        }
    }
    __syncthreads();
    if (lv > levels) return;
    const int lim = min(TOPN, 2 * cap);
    for (int i = threadIdx.x; i < lim; i += blockDim.x) top[i] = T[i];
    for (; lv <= levels; ++lv) {
        __syncthreads();
        const int lo0 = (cap + a0) >> lv, n0 = ((cap + e0 - 1) >> lv) - lo0 + 1;
        const int lo1 = (cap + a1) >> lv, n1 = e1 > a1 ? ((cap + e1 - 1) >> lv) - lo1 + 1 : 0;
        for (int k = threadIdx.x; k < n0 + n1; k += blockDim.x) {
            const int node = k < n0 ? lo0 + k : lo1 + k - n0;
            top[node] = top[2 * node] + top[2 * node + 1];
        }
    }
    __syncthreads();
    const int wb = min(TOPN / 2, cap);
    for (int i = 1 + threadIdx.x; i < wb; i += blockDim.x) T[i] = top[i];
    __syncthreads();
}

// propagate_span for a span that does not wrap and holds at most SPAN_LDS - 2
// leaves, every level in LDS: the span's nodes of one level are a contiguous
// range [lo, hi] whose children are [lo & ~1, hi | 1] of the level below --
// the span's own recomputed nodes plus at most one unchanged sibling at each
// end.  The siblings of every level are outside the span, so nothing in this
// launch writes them: all of them are loaded up front (one round trip), the
// span's leaves once, and then each level is one barrier of LDS work whose
// results also go to the tree (stores nothing waits for).  The same operands
// in the same order as propagate_span: bit-identical.  Returns false (nothing
// done) when the span does not qualify.
constexpr int SPAN_LDS = 4096;
constexpr int SPAN_LEVELS = 32;
__device__ bool propagate_span_lds(float *T, int cap, int levels, int capacity, int first, int count,
                                   float *buf /* 2 SPAN_LDS */, float *edge /* 2 SPAN_LEVELS */) {
    const int a = cap + first, e = cap + first + count - 1;  // leaf nodes [a, e]
    if (count <= 0 || first + count > capacity || count > SPAN_LDS - 2 || levels >= SPAN_LEVELS) return false;
    // edge[2 lv], edge[2 lv + 1]: the unchanged left / right sibling at level lv
    // (the children of level lv + 1's range), when that range needs one
    const int t = threadIdx.x;
    if (t < 2 * levels) {
        const int lv = t >> 1, right = t & 1;
        const int lo = a >> lv, hi = e >> lv;
        if (!right && (lo & 1)) edge[t] = T[lo - 1];
        if (right && !(hi & 1)) edge[t] = T[hi + 1];
    }
    float *A = buf, *B = buf + SPAN_LDS;
    // level 0: A[c - (a & ~1)] for c in [a & ~1, e | 1]
    {
        const int base = a & ~1;
        for (int c = a + t; c <= e; c += blockDim.x) A[c - base] = T[c];
    }
    __syncthreads();
    if (t == 0) {
        if (a & 1) A[0] = edge[0];
        if (!(e & 1)) A[(e | 1) - (a & ~1)] = edge[1];
    }
    for (int lv = 1; lv <= levels; ++lv) {
        __syncthreads();
        const int lo = a >> lv, hi = e >> lv, cbase = (a >> (lv - 1)) & ~1, nbase = lo & ~1;
        for (int node = lo + t; node <= hi; node += blockDim.x) {
            const int c = 2 * node - cbase;
            const float v = A[c] + A[c + 1];
            T[node] = v;
            B[node - nbase] = v;
        }
        if (t == 0 && lv < levels) {
            if (lo & 1) B[0] = edge[2 * lv];
            if (!(hi & 1)) B[(hi | 1) - nbase] = edge[2 * lv + 1];
        }
        float *tmp = A;
        A = B;
        B = tmp;
    }
    __syncthreads();
    return true;
}

// LAP.add: new items get max_priority (:56-57).  The items of this block's
// stratum are gathered in chunks of ADD_CHUNK into LDS, their leaves written,
// then their ancestors recomputed.
constexpr int ADD_CHUNK = 4096;
__global__ __launch_bounds__(UPD_THREADS) void lap_add_kernel(float *tree, const float *maxp, int cap, int levels,
                                                              int capacity, const int32_t *stratum,
                                                              const int32_t *slot, int n) {
    const int s = blockIdx.x;
    float *T = stratum_tree(tree, s, cap);
    __shared__ int32_t mine[ADD_CHUNK];
    __shared__ int count;
    const float p = *maxp;
    for (int base = 0; base < n; base += ADD_CHUNK) {
        if (threadIdx.x == 0) count = 0;
        __syncthreads();
        const int end = min(n, base + ADD_CHUNK);
        for (int k = base + threadIdx.x; k < end; k += blockDim.x) {
            if (stratum[k] != s) continue;
            const int sl = slot[k];
            if (sl < 0 || sl >= capacity) continue;
            T[cap + sl] = p;
            mine[atomicAdd(&count, 1)] = sl;
        }
        __syncthreads();
        propagate(T, cap, levels, mine, count);
    }
}

// Sum of the leaves [0, sz) of one stratum's tree: the reference samples
// against cumsum(priority[i, :size]) (:76-77), and with its single-add pointer
// quirk (:59-61) strata 1..E-1 hold their newest transition at slot == size,
// outside that prefix -- so the draw is scaled by the prefix total, not the
// root.  One root-to-leaf walk towards leaf sz adding every left sibling.
// The walk's nodes depend on sz alone (step j visits (1 << j) | sz >> (levels
// - j)): every addend is loaded first, independently, and then added in the
// walk's order (an unset bit adds +0: the same sum) -- one memory round trip
// instead of one per level.  at(node): the tree accessor.
constexpr int MAXLV = 24;  // levels of a stratum tree (capacity <= 2^24)
template <class At>
__device__ __forceinline__ float prefix_sum(At at, int cap, int levels, int sz) {
    if (sz >= cap) return at(1);
    float v[MAXLV];
#pragma unroll
    for (int j = 0; j < MAXLV; ++j) {
        v[j] = 0.0f;
        if (j < levels) {
            const int lv = levels - 1 - j;
            const float x = at(2 * ((1 << j) | (sz >> (lv + 1))));
            v[j] = ((sz >> lv) & 1) ? x : 0.0f;
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXLV; ++j)
        if (j < levels) acc += v[j];
    return acc;
}
__device__ __forceinline__ float prefix_total(const float *T, int cap, int levels, int sz) {
    return prefix_sum([T](int n) { return T[n]; }, cap, levels, sz);
}

__device__ __forceinline__ float sel4(int r, float a, float b, float c, float d) {
    return r == 0 ? a : r == 1 ? b : r == 2 ? c : d;
}

// The descent from `node` at level lv to a leaf: at every level go left when
// val <= left and the left subtree is not empty (or the right one is), else
// subtract left and go right.  The `left > 0` term matters only for val == 0
// over an empty left subtree: a buffer's own tree has none left of a filled
// slot (the same leaf as without the term), a view's tree (lap_view_build)
// has them wherever the leading rows are foreign, and the walk must not end
// on a zero leaf there.  The LDS levels of lap_update_sample apply the same
// rule.  The children of the next (up to) three levels are read together --
// 2 + 4 + 8 nodes at 2n, 4n, 8n -- and the three choices made from registers:
// the same comparisons and subtractions as the one-level walk, a third of its
// dependent memory round trips.  Returns the leaf node.
template <class At>
__device__ __forceinline__ int descend_from(At at, float val, int node, int lv, int levels) {
    while (lv < levels) {
        const int k = levels - lv >= 3 ? 3 : levels - lv;
        const int n1 = 2 * node, n2 = 4 * node, n3 = 8 * node;
        const float a0 = at(n1), a1 = at(n1 + 1);
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
        float c4 = 0.f, c5 = 0.f, c6 = 0.f, c7 = 0.f;
        if (k >= 2) b0 = at(n2), b1 = at(n2 + 1), b2 = at(n2 + 2), b3 = at(n2 + 3);
        if (k >= 3) {
            c0 = at(n3), c1 = at(n3 + 1), c2 = at(n3 + 2), c3 = at(n3 + 3);
            c4 = at(n3 + 4), c5 = at(n3 + 5), c6 = at(n3 + 6), c7 = at(n3 + 7);
        }
        int r;
        if ((val <= a0 && a0 > 0.0f) || a1 <= 0.0f) {
            r = 0;
        } else {
            val -= a0;
            r = 1;
        }
        if (k >= 2) {
            const float l = r ? b2 : b0, rt = r ? b3 : b1;
            if ((val <= l && l > 0.0f) || rt <= 0.0f) {
                r = 2 * r;
            } else {
                val -= l;
                r = 2 * r + 1;
            }
            if (k >= 3) {
                const float l3 = sel4(r, c0, c2, c4, c6), r3 = sel4(r, c1, c3, c5, c7);
                if ((val <= l3 && l3 > 0.0f) || r3 <= 0.0f) {
                    r = 2 * r;
                } else {
                    val -= l3;
                    r = 2 * r + 1;
                }
            }
        }
        node = (node << k) + r;
        lv += k;
    }
    return node;
}

// LAP.sample (:75-78): idx = searchsorted_left(cumsum(p[:size]), u * total)
__global__ void lap_sample_kernel(const float *tree, int cap, int levels, const float *u, const int32_t *size,
                                  int batch, int32_t *idx) {
    const int s = blockIdx.y;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const float *T = tree + (size_t)s * 2 * cap;
    const int sz = size[s];
    const float val = u[(size_t)s * batch + b] * prefix_total(T, cap, levels, sz);
    const int node = descend_from([T](int n) { return T[n]; }, val, 1, 0, levels);
    int i = node - cap;
    if (i >= sz) i = sz > 0 ? sz - 1 : 0;
    idx[(size_t)s * batch + b] = i;
}

// TdPrio (lap_update_sample_td): the priorities computed in the update from the
// critic pass's |td| of both heads, prio = max(|td0|, |td1|, min_priority)^alpha
// (TD7_multi_agent.py:259, the expression td7f_wgrad evaluates), so the update
// need not wait for the weight-gradient launch; written to `out` if non-null.
struct TdPrio {
    const float *td;  // [B][2]; nullptr: the priorities are given (prio)
    float alpha, minp;
    float *out;
};

// LAP.update_priority's leaf pass for stratum s (:113-117): the batch's indices
// I staged in LDS (li, UPD_THREADS of them at a time), a leaf written by the
// last of its duplicates, priorities P or tp's.  Returns the thread's running
// maximum of the batch's priorities.
__device__ __forceinline__ float update_leaves(float *T, int cap, const int32_t *I, int batch, const TdPrio &tp,
                                               const float *P, int s, int32_t *li) {
    float mx = 0.0f;
    for (int b0 = 0; b0 < batch; b0 += UPD_THREADS) { // the batch's indices staged in LDS
        const int nb = min(UPD_THREADS, batch - b0);
        __syncthreads();
        if ((int)threadIdx.x < nb) li[threadIdx.x] = I[b0 + threadIdx.x];
        __syncthreads();
        const int b = b0 + threadIdx.x;
        if (b < batch) {
            const int me = li[threadIdx.x];
            bool last = true; // a later duplicate overwrites this one
            for (int k = threadIdx.x + 1; k < nb; ++k) last &= (li[k] != me);
            for (int b2 = b0 + nb; b2 < batch; ++b2) last &= (I[b2] != me);
            float pb;
            if (tp.td) {
                const long d = (long)s * batch + b;
                pb = powf(fmaxf(fmaxf(tp.td[2 * d], tp.td[2 * d + 1]), tp.minp), tp.alpha);
                if (tp.out) tp.out[d] = pb;
            } else {
                pb = P[b];
            }
            if (last) T[cap + me] = pb;
            mx = fmaxf(mx, pb);
        }
    }
    return mx;
}

// The workgroup's maximum into *maxp, in two steps with a barrier of the
// caller's between them (propagate*'s, where there is one): every wave's
// maximum to red[], then thread 0's atomic.
__device__ __forceinline__ float wave_max_to(float *red, float mx) {
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    return mx;
}
__device__ __forceinline__ void block_max_to(float *maxp, float mx, const float *red) {
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) mx = fmaxf(mx, red[w]);
        // priorities are >= min_priority^alpha > 0 (leaves >= 0): int order == float order
        atomicMax(reinterpret_cast<int *>(maxp), __float_as_int(mx));
    }
}

// LAP.update_priority (:113-117)
__global__ __launch_bounds__(UPD_THREADS) void lap_update_kernel(float *tree, float *maxp, int cap, int levels,
                                                                 const int32_t *idx, const float *prio,
                                                                 int batch) {
    const int s = blockIdx.x;
    float *T = stratum_tree(tree, s, cap);
    const int32_t *I = idx + (size_t)s * batch;
    __shared__ float red[UPD_THREADS / 64];
    __shared__ int32_t li[UPD_THREADS];
    float mx = update_leaves(T, cap, I, batch, TdPrio{nullptr, 0.f, 0.f, nullptr}, prio + (size_t)s * batch, s, li);
    mx = wave_max_to(red, mx);
    propagate(T, cap, levels, I, batch);
    block_max_to(maxp, mx, red);
}

// LAP.reset_max_priority (:119-120): max over every leaf of every stratum.
// maxp is zeroed by the launcher first; leaves are >= 0 so int order works.
__global__ void lap_reset_max_kernel(const float *tree, float *maxp, int cap, int n_strata) {
    __shared__ float red[16];
    float mx = 0.0f;
    const size_t total = (size_t)n_strata * cap;
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (size_t)gridDim.x * blockDim.x) {
        const size_t s = k / cap, i = k % cap;
        mx = fmaxf(mx, tree[s * 2 * cap + cap + i]);
    }
    mx = wave_max_to(red, mx);
    __syncthreads();
    block_max_to(maxp, mx, red);
}

__global__ void lap_totals_kernel(const float *tree, int cap, int n_strata, float *out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_strata) out[s] = tree[(size_t)s * 2 * cap + 1];
}

__global__ void lap_init_kernel(float *maxp) { *maxp = 1.0f; } // max_priority = 1 (:42)


// ---------------------------------------------------------------- batched store
// LAP.add for every env of one vectorised step (:49-63 per row): the rows of
// stratum s go to consecutive ring slots starting at ptr[s], in env order.
// Phase 1 (one workgroup per stratum): block scan of "row i is active and in
// stratum s" -> slot of every row (the trash row `capacity` for inactive ones),
// new leaves = max_priority, ring pointer and size; the stratum's new slots are
// one ring span, whose ancestors are recomputed once after the last chunk
// (propagate_span; r03d: a propagate per 4,096-row chunk made the 65,536-env
// store 158 us).
// Phase 2 (many workgroups): one wavefront per row copies its transition.
constexpr int STORE_CHUNK = UPD_THREADS * 4;

// The calling thread's exclusive prefix of v over the UPD_THREADS-thread
// workgroup (wave __shfl_up ladder, the waves' sums in wsum[UPD_THREADS / 64],
// thread 0's serial pass over them), and the workgroup's total through `total`
// (from *total_lds, into a register before returning).  Two barriers; a caller
// that scans again keeps a barrier of its own before the next call, which
// overwrites wsum and *total_lds.
__device__ __forceinline__ int block_scan_excl(int v, int *wsum, int *total_lds, int &total) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int k = 0; k < UPD_THREADS / 64; ++k) {
            const int w = wsum[k];
            wsum[k] = acc;
            acc += w;
        }
        *total_lds = acc;
    }
    __syncthreads();
    total = *total_lds;
    return wsum[wv] + incl - v;
}

template <int RANK_RPT>
__global__ __launch_bounds__(UPD_THREADS) void lap_store_rank_kernel(float *tree, const float *maxp, int cap,
                                                                     int levels, int capacity, int32_t *ring_ptr,
                                                                     int32_t *ring_size, const int32_t *strata,
                                                                     const uint8_t *active, int n, int32_t *row_of) {
    const int s = blockIdx.x, t = threadIdx.x;
    float *T = stratum_tree(tree, s, cap);
    __shared__ int wsum[UPD_THREADS / 64];
    __shared__ int chunk_total;
    const float p = *maxp;
    const int ptr0 = ring_ptr[s];
    const int row0 = s * (capacity + 1);
    int offset = 0; // rows of this stratum placed by earlier chunks
    // RANK_RPT consecutive rows per thread (their strata kept in registers):
    // 16 above 16,384 envs -- 4 chunks of 16,384 rows at 65,536 envs instead of
    // 16 of 4,096, each chunk paying a load latency and two barriers -- and 4
    // below (one chunk at 4,096 envs either way; 16 serial rows per thread
    // measured 16.2 vs 15.0 us there, profiles/r03d_raw/lap2)
    for (int base = 0; base < n; base += RANK_RPT * UPD_THREADS) {
        int st[RANK_RPT], cnt = 0;
        bool f[RANK_RPT];
#pragma unroll
        for (int k = 0; k < RANK_RPT; ++k) {
            const int i = base + RANK_RPT * t + k;
            st[k] = i < n ? strata[i] : -1;
            f[k] = i < n && (!active || active[i]);
        }
#pragma unroll
        for (int k = 0; k < RANK_RPT; ++k) {
            f[k] = f[k] && st[k] == s;
            cnt += f[k];
        }
        int total;
        int rank = offset + block_scan_excl(cnt, wsum, &chunk_total, total);
#pragma unroll
        for (int k = 0; k < RANK_RPT; ++k) {
            const int i = base + RANK_RPT * t + k;
            if (i >= n) continue;
            if (s == 0 && (st[k] < 0 || st[k] >= (int)gridDim.x)) row_of[i] = -1; // no stratum
            if (st[k] != s) continue;
            if (f[k]) {
                const int slot = (ptr0 + rank) % capacity;
                row_of[i] = row0 + slot;
                T[cap + slot] = p;
                ++rank;
            } else {
                row_of[i] = row0 + capacity; // inactive env: the trash row
            }
        }
        __syncthreads();
        offset += total;
    }
    propagate_span(T, cap, levels, capacity, ptr0, offset);
    if (t == 0) {
        ring_ptr[s] = (ptr0 + offset) % capacity;
        ring_size[s] = min(ring_size[s] + offset, capacity);
    }
}

// LAP.add with the reference's SHARED pointer (:49-63), called for every
// active env of one vectorised step in env order -- what the training script's
// per-env loop does (Exoskeleton_agent_train.py:139-142).  The c-th add writes
// slot ptr0 + #{multiples of E in [count0, c)} of its stratum (the pointer
// advances after an add whose count is a multiple of E = num_envs, :59-61), so
// env 0's first transition sits one slot behind the others and, when envs are
// done, two adds of one stratum can land in the same slot -- the later one
// wins, as the reference's overwrite.  One workgroup: a block scan ranks the
// active rows (rank_row[r] = the stratum of rank r), every active row checks
// the next E-1 ranks for a same-stratum, same-slot successor (two counts share
// a slot only if no multiple of E lies between them), winners get slot_of /
// row_of, losers and inactive rows -1.  ref = {ptr, count, size}; every
// stratum's size = size (the reference samples every row against the one
// shared size, :76).
__device__ __forceinline__ long long mult_below(long long x, int E) { return (x + E - 1) / E; }

// The shared pointer's slot for an add whose count c has mr = mult_below(c, E),
// from the pointer ptr0 at count0 (m0 = mult_below(count0, E)).
__device__ __forceinline__ int ref_slot(long long ptr0, long long m0, long long mr, int capacity) {
    long long v = ptr0 + (mr - m0); // ptr0 < capacity, mr - m0 <= n / E + 1
    if (v >= capacity) v -= capacity;
    if (v >= capacity) v %= capacity;
    return (int)v;
}

// {ptr, count, size} after n_act more adds
struct RefState {
    long long ptr, count, size;
};
__device__ __forceinline__ RefState ref_advance(long long ptr0, long long count0, long long size0, long long n_act,
                                                int E, int capacity) {
    const long long adv = mult_below(count0 + n_act, E) - mult_below(count0, E);
    return {(ptr0 + adv) % capacity, count0 + n_act, min(size0 + adv, (long long)capacity)};
}

__global__ __launch_bounds__(UPD_THREADS) void lap_store_ref_slots_kernel(int capacity, int E, long long *ref,
                                                                          int32_t *ring_size,
                                                                          const int32_t *strata,
                                                                          const uint8_t *active, int n,
                                                                          int32_t *rank_row, int32_t *slot_of,
                                                                          int32_t *row_of) {
    const int t = threadIdx.x;
    __shared__ int wsum[UPD_THREADS / 64];
    __shared__ int chunk_total;
    const long long ptr0 = ref[0], count0 = ref[1], size0 = ref[2];
    const long long m0 = mult_below(count0, E);
    int offset = 0;
    for (int base = 0; base < n; base += STORE_CHUNK) {
        int f[4], cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + 4 * t + k;
            f[k] = (i < n && strata[i] >= 0 && strata[i] < E && (!active || active[i])) ? 1 : 0;
            cnt += f[k];
        }
        int total;
        int rank = offset + block_scan_excl(cnt, wsum, &chunk_total, total);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + 4 * t + k;
            if (i >= n) continue;
            if (f[k]) {
                rank_row[rank] = strata[i]; // the stratum of each rank (the winner pass reads it)
                row_of[i] = rank;           // the rank, until the winner pass below
                ++rank;
            } else {
                row_of[i] = -1;
                slot_of[i] = -1;
            }
        }
        offset += total;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    const int n_act = offset;
    for (int i = t; i < n; i += blockDim.x) {
        const int r = row_of[i];
        if (r < 0) continue;
        const long long mr = mult_below(count0 + r, E);
        const int s = strata[i];
        bool win = true;
        // ranks r < q share r's slot while count0 + q <= mr E (ceil((count0 + q) / E) == mr):
        // one 64-bit product instead of a 64-bit division per candidate, and the
        // candidate's stratum read directly (one load, not rank -> row -> stratum)
        const long long qend = mr * E - count0;
        const int qmax = (int)min((long long)min(r + E, n_act) - 1, qend);
        for (int q = r + 1; q <= qmax; ++q) win &= rank_row[q] != s;
        const int slot = ref_slot(ptr0, m0, mr, capacity);
        slot_of[i] = win ? slot : -1;
        row_of[i] = win ? s * (capacity + 1) + slot : -1;
    }
    __syncthreads();
    const RefState nx = ref_advance(ptr0, count0, size0, n_act, E, capacity);
    for (int s = t; s < E; s += blockDim.x) ring_size[s] = (int32_t)nx.size;
    if (t == 0) {
        ref[0] = nx.ptr;
        ref[1] = nx.count;
        ref[2] = nx.size;
    }
}

// r04: lap_store_batch_ref as ONE launch (the three
// launches above cost ~28 us per 4,096-env step of the reference schedule).
// Grid (E strata) x (K copy parts), 1024 threads.  Every workgroup ranks the
// active rows (the same block scan, chunks of STORE_CHUNK rows) and keeps, for
// ITS stratum, the rows in rank order (LDS).  The winner test needs no rank ->
// stratum table: a row loses iff the next active row of the SAME stratum
// shares its slot (the c-th add's slot depends only on ceil((count0 + c) / E),
// so same-slot ranks are consecutive and all lie within [r, mr E - count0]).
// Part 0 writes the winners' leaves (max_priority) and recomputes the span
// [ptr0, last slot] of its stratum (propagate_span: nodes whose children did
// not change are recomputed to the same sum); every part copies the winners
// with stratum-row index = part (mod K).  The last workgroup out (ticket
// ws[0]) advances the shared pointer and the strata's sampling size.
// Bit-identical to the three launches (tests/test_lap_gpu.py).
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// One env step's transitions as the store kernels receive them: row i of
// state / next_state [n][state_dim], action [n][action_dim] (stored divided by
// action_scale), reward [n], done [n] (stored as not_done = 1 - done).
struct Rows {
    const float *state, *action, *next_state, *reward;
    const uint8_t *done;
    float action_scale;
};

// The rows are whole float4s, 16-byte aligned, in the storage and in the
// caller's state / next_state arrays a, b (the copies' float4 path).
__host__ __device__ __forceinline__ bool rows_vec(const lap_storage_desc &st, const float *a, const float *b) {
    return (st.state_dim & 3) == 0 &&
           ((reinterpret_cast<uintptr_t>(st.state) | reinterpret_cast<uintptr_t>(st.next_state) |
             reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

// The transitions in.*[ri[j]] for j = j0, j0 + step, ... < m of stratum s to the
// slots sl[j] (< 0: skipped), item by item over the nt threads t.
template <bool VEC>
__device__ __forceinline__ void copy_rows(const lap_storage_desc &st, const Rows &in, const int32_t *ri,
                                          const int32_t *sl, int s, int capacity, int j0, int step, int m, int t,
                                          int nt) {
    const int sd = st.state_dim, ad = st.action_dim;
    const int sdv = VEC ? sd / 4 : sd;        // state items per row (float4 or float)
    const int per = 2 * sdv + ad + 2;         // state, next_state, action, reward, not_done
    const int nrows = j0 < m ? (m - j0 + step - 1) / step : 0;
    const int items = nrows * per;
    constexpr int U = 4;  // items in flight per thread: loads first, then stores
    for (int it0 = t; it0 < items; it0 += U * nt) {
        float4 v[U];
        long dst[U];
        int kind[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int it = it0 + u * nt;
            kind[u] = -1;
            if (it >= items) continue;
            const int q = it / per, c = it - q * per, j = j0 + q * step;
            const int slot = sl[j];
            if (slot < 0) continue;
            const long r = (long)s * (capacity + 1) + slot;
            const long i = ri[j];
            if (c < 2 * sdv) {
                const bool nx = c >= sdv;
                const int e = nx ? c - sdv : c;
                const float *src = (nx ? in.next_state : in.state) + i * sd;
                if (VEC) {
                    v[u] = ld4(src + 4 * e);
                    dst[u] = r * sd + 4 * e;
                } else {
                    v[u].x = src[e];
                    dst[u] = r * sd + e;
                }
                kind[u] = nx ? 1 : 0;
            } else if (c < 2 * sdv + ad) {
                const int e = c - 2 * sdv;
                v[u].x = in.action[i * ad + e] / in.action_scale;
                dst[u] = r * ad + e;
                kind[u] = 2;
            } else if (c == 2 * sdv + ad) {
                v[u].x = in.reward[i];
                dst[u] = r;
                kind[u] = 3;
            } else {
                v[u].x = 1.0f - (in.done[i] ? 1.0f : 0.0f);
                dst[u] = r;
                kind[u] = 4;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            switch (kind[u]) {
            case 0:
                if (VEC) st4(st.state + dst[u], v[u]); else st.state[dst[u]] = v[u].x;
                break;
            case 1:
                if (VEC) st4(st.next_state + dst[u], v[u]); else st.next_state[dst[u]] = v[u].x;
                break;
            case 2: st.action[dst[u]] = v[u].x; break;
            case 3: st.reward[dst[u]] = v[u].x; break;
            case 4: st.not_done[dst[u]] = v[u].x; break;
            default: break;
            }
        }
    }
}

// The training loop's per-step mask advance, optionally done by the insert's
// last workgroup out (lap_store_batch_ref_fused_adv): every workgroup has read
// the step's mask by then.  exo_active_advance_score's arithmetic: score +=
// reward where the step's mask is set, k = min(k + 1, rows - 1), mask = table
// row k, count = its population.
struct MaskAdvance {
    const uint8_t *table;  // nullptr: no advance
    int rows;
    long long *k;
    uint8_t *active;
    int32_t *count;
    double *score;         // nullptr: no score
};

template <bool VEC>
__global__ __launch_bounds__(UPD_THREADS) void lap_store_ref_fused_kernel(
    float *tree, const float *maxp, int cap, int levels, int capacity, int E, long long *ref, int32_t *ring_size,
    lap_storage_desc st, Rows in, const int32_t *strata, const uint8_t *active, int n, uint32_t *ticket,
    MaskAdvance adv) {
    const int s = blockIdx.x, part = blockIdx.y, K = gridDim.y;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __shared__ int wsum[UPD_THREADS / 64];
    __shared__ int chunk_total;  // (active rows) | (rows of stratum s) << 16
    __shared__ int32_t rk[STORE_CHUNK], ri[STORE_CHUNK], sl[STORE_CHUNK];
    __shared__ int carry_r, carry_i, carry_J, carry_slot;  // the chunk's last row of stratum s, decided later
    float *T = stratum_tree(tree, s, cap);
    // K > 1: part 0 writes the leaves and propagates, parts 1..K-1 copy the rows
    // (copy part of stratum-row j: 1 + j mod (K - 1)); K == 1: part 0 does both
    const int KC = K > 1 ? K - 1 : 1, cpart = K > 1 ? part - 1 : 0;
    const long long ptr0 = ref[0], count0 = ref[1], size0 = ref[2];
    const long long m0 = mult_below(count0, E);
    const float p = *maxp;
    auto slot_of = [&](long long r) { return ref_slot(ptr0, m0, mult_below(count0 + r, E), capacity); };
    if (t == 0) carry_r = -1;
    int offset = 0, soff = 0;  // active rows / stratum-s rows before this chunk
    for (int base = 0; base < n; base += STORE_CHUNK) {
        int cnt = 0, gcnt = 0;
        bool f[4], g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = base + 4 * t + k;
            const int sk = i < n ? strata[i] : -1;
            f[k] = i < n && sk >= 0 && sk < E && (!active || active[i]);
            g[k] = f[k] && sk == s;
            cnt += f[k];
            gcnt += g[k];
        }
        // block-wide exclusive scan of (cnt, gcnt) packed in one int (each <= STORE_CHUNK < 2^16)
        int total;
        const int ex = block_scan_excl(cnt | (gcnt << 16), wsum, &chunk_total, total);
        int rank = offset + (ex & 0xFFFF), j = ex >> 16;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (g[k]) {
                rk[j] = rank;
                ri[j] = base + 4 * t + k;
                ++j;
            }
            rank += f[k];
        }
        __syncthreads();
        const int m = total >> 16;
        // the previous chunk's last row of stratum s: its successor is rk[0]
        if (t == 0) {
            carry_slot = -1;
            if (carry_r >= 0 && m > 0) {
                const long long mr = mult_below(count0 + carry_r, E);
                if ((long long)rk[0] > mr * E - count0) {  // no same-slot successor: a winner
                    carry_slot = slot_of(carry_r);
                    if (part == 0) T[cap + carry_slot] = p;
                }
                carry_r = -1;
            }
        }
        __syncthreads();
        if (carry_slot >= 0 && wv == 0 && carry_J % KC == cpart)
            copy_rows<VEC>(st, in, &carry_i, &carry_slot, s, capacity, 0, 1, 1, lane, 64);
        __syncthreads();  // the loop below sets the next carry: wave 0 must be done reading this one
        for (int jj = t; jj < m; jj += UPD_THREADS) {
            const int r = rk[jj];
            if (jj + 1 == m) {  // successor unknown until a later chunk (or none: a winner)
                carry_r = r;
                carry_i = ri[jj];
                carry_J = soff + jj;
                sl[jj] = -1;
                continue;
            }
            const long long mr = mult_below(count0 + r, E);
            const bool win = (long long)rk[jj + 1] > mr * E - count0;
            const int slot = win ? slot_of(r) : -1;
            sl[jj] = slot;
            if (win && part == 0) T[cap + slot] = p;
        }
        __syncthreads();
        // this part's share of the chunk's winners: stratum-row index = cpart (mod KC)
        if (cpart >= 0) {
            const int j0 = ((cpart - soff) % KC + KC) % KC;
            copy_rows<VEC>(st, in, ri, sl, s, capacity, j0, KC, m, t, UPD_THREADS);
        }
        offset += total & 0xFFFF;
        soff += m;
        __syncthreads();
    }
    // the last row of stratum s has no successor: a winner
    if (t == 0) {
        carry_slot = -1;
        if (carry_r >= 0) {
            carry_slot = slot_of(carry_r);
            if (part == 0) T[cap + carry_slot] = p;
        }
    }
    __syncthreads();
    if (carry_slot >= 0 && wv == 0 && carry_J % KC == cpart)
        copy_rows<VEC>(st, in, &carry_i, &carry_slot, s, capacity, 0, 1, 1, lane, 64);
    const int n_act = offset;
    if (part == 0 && n_act > 0) {
        __shared__ float span_buf[2 * SPAN_LDS], span_edge[2 * SPAN_LEVELS];
        __syncthreads();
        const long long last = mult_below(count0 + n_act - 1, E) - m0;  // slots ptr0 .. ptr0 + last
        const int cnt = (int)min(last + 1, (long long)capacity);
        if (!propagate_span_lds(T, cap, levels, capacity, (int)ptr0, cnt, span_buf, span_edge))
            propagate_span(T, cap, levels, capacity, (int)ptr0, cnt);
    }
    __syncthreads();
    __shared__ int last;
    if (t == 0) {  // ref and the mask were read (and used) before this add: no fence needed
        last = atomicAdd(ticket, 1u) == (uint32_t)(E * K - 1);  // every workgroup has read them
        if (last) {
            const RefState nx = ref_advance(ptr0, count0, size0, n_act, E, capacity);
            for (int q = 0; q < E; ++q) ring_size[q] = (int32_t)nx.size;
            ref[0] = nx.ptr;
            ref[1] = nx.count;
            ref[2] = nx.size;
            *ticket = 0u;
        }
    }
    __syncthreads();
    if (!last || !adv.table) return;
    const long long k0 = *adv.k;
    const long long kk = k0 + 1 < adv.rows ? k0 + 1 : adv.rows - 1;
    int c = 0;
    for (int e = t; e < n; e += UPD_THREADS) {
        const uint8_t v = adv.table[(size_t)kk * n + e];
        if (adv.score) adv.score[e] += adv.active[e] ? (double)in.reward[e] : 0.0;
        adv.active[e] = v;
        c += v != 0;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int wc[UPD_THREADS / 64];
    if (lane == 0) wc[wv] = c;
    __syncthreads();
    if (t == 0) {
        *adv.k = kk;
        if (adv.count) {
            int tot = 0;
            for (int w = 0; w < UPD_THREADS / 64; ++w) tot += wc[w];
            *adv.count = tot;
        }
    }
}

// One wavefront copies transition i of `in` to storage row r.
__device__ __forceinline__ void store_row_wave(const lap_storage_desc &st, const Rows &in, long r, long i, int lane) {
    const int sd = st.state_dim, ad = st.action_dim;
    for (int k = lane; k < sd; k += 64) {
        st.state[r * sd + k] = in.state[i * sd + k];
        st.next_state[r * sd + k] = in.next_state[i * sd + k];
    }
    for (int k = lane; k < ad; k += 64) st.action[r * ad + k] = in.action[i * ad + k] / in.action_scale;
    if (lane == 0) {
        st.reward[r] = in.reward[i];
        st.not_done[r] = 1.0f - (in.done[i] ? 1.0f : 0.0f);
    }
}

__global__ __launch_bounds__(256) void lap_store_copy_kernel(lap_storage_desc st, Rows in, int n,
                                                             const int32_t *row_of) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const long r = row_of[i];
    if (r < 0) return;
    store_row_wave(st, in, r, i, lane);
}

// The five arrays a sampled batch is gathered into, row d = s * batch + b.
struct Outs {
    float *state, *action, *next_state, *reward, *not_done;
};

// LAP.sample (:65-111) with the gather: one wavefront per draw descends the
// tree (every lane the same path, reads broadcast) and copies the row.
__device__ __forceinline__ void sample_descend(const float *tree, int cap, int levels, int capacity, float ud,
                                               const int32_t *size, int batch, int d, int lane, int32_t *idx,
                                               const lap_storage_desc &st, const Outs &o) {
    const int s = d / batch;
    const float *T = tree + (size_t)s * 2 * cap;
    const int sz = size[s];
    const float val = ud * prefix_total(T, cap, levels, sz);
    const int node = descend_from([T](int n) { return T[n]; }, val, 1, 0, levels);
    int i = node - cap;
    if (i >= sz) i = sz > 0 ? sz - 1 : 0;
    if (lane == 0) idx[d] = i;
    const long r = (long)s * (capacity + 1) + i;
    const int sd = st.state_dim, ad = st.action_dim;
    for (int k = lane; k < sd; k += 64) {
        o.state[(long)d * sd + k] = st.state[r * sd + k];
        o.next_state[(long)d * sd + k] = st.next_state[r * sd + k];
    }
    for (int k = lane; k < ad; k += 64) o.action[(long)d * ad + k] = st.action[r * ad + k];
    if (lane == 0) {
        o.reward[d] = st.reward[r];
        o.not_done[d] = st.not_done[r];
    }
}

// rng != nullptr: u[d] is drawn in the kernel (Philox block d of this call,
// word 0 -> [0, 1)); the device call counter advances once per launch (the
// last workgroup out, as td7_adam_step's step count).
struct SampleRng {
    uint64_t seed;
    uint32_t tag;
    unsigned long long *counter;
    uint32_t *ticket;
};
// The call counter's advance, by one thread of every workgroup after the
// workgroup's last use of `call` (= *rng.counter, read before its barrier):
// the last workgroup out writes call + 1 and leaves the ticket zero.
__device__ __forceinline__ void rng_ticket(const SampleRng &rng, unsigned long long call) {
    if (atomicAdd(rng.ticket, 1u) == gridDim.x - 1) {
        *rng.counter = call + 1ull;
        *rng.ticket = 0u;
    }
}

__global__ __launch_bounds__(256) void lap_sample_gather_kernel(const float *tree, int cap, int levels, int capacity,
                                                                const float *u, const int32_t *size, int batch,
                                                                int total, int32_t *idx, lap_storage_desc st,
                                                                Outs o, SampleRng rng) {
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (rng.counter) {
        const unsigned long long call = *rng.counter;
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            rng_ticket(rng, call);
        }
        if (d >= total) return;
        uint32_t r[4];
        philox_block(rng.seed, rng.tag, call, (uint32_t)d, r);
        sample_descend(tree, cap, levels, capacity, u01_open_hi(r[0]), size, batch, d, lane, idx, st, o);
        return;
    }
    if (d >= total) return;
    sample_descend(tree, cap, levels, capacity, u[d], size, batch, d, lane, idx, st, o);
}


// The top of a stratum tree lap_update_sample stages in LDS (r05 A/B at the
// bench's shape, tools/lap_bench.py: 32,768 nodes -- 128 KB, 3 global levels
// left instead of 6 -- 23.9 us per launch against 21.8 with 8,192: staging
// 128 KB costs more than the three level sweeps it saves)
#ifndef LAP_TOPN_US
#define LAP_TOPN_US 8192
#endif
constexpr int TOPN_US = LAP_TOPN_US;

// ---------------------------------------------------------------- planned reference inserts
// The reference schedule's rollout inserts (lap_store_batch_ref_fused_adv per
// step: 18.5 us of its ~80 us per 4,096-env step, r05 lap_bench) planned for
// a whole episode round at its start (r05).  Which envs run at each step of
// a synchronous round is fixed by the motion lengths (the trainer's mask
// table), so the shared pointer's slot of every add of the round -- and
// which adds a later same-slot add of the same stratum overwrites -- follow
// from the pointer at the round start alone: lap_ref_plan writes
// plan[k][e] = the slot env e's step-k transition lands in (-1: inactive or
// overwritten).  A step is then one elementwise launch (lap_ref_step: the
// row copies, the scores, the next mask) with no scan, ticket or tree work,
// and lap_ref_commit writes the round's leaves (max_priority: constant over a
// rollout, nothing trains during it), recomputes the round's ring span once
// and advances the pointer and sizes.  The same rows, leaves, sums, pointer
// and sizes as the per-step inserts: a slot written twice in a round is
// written by the later add either way, an ancestor's last recomputation sees
// its children's final values either way.

// pass 1: rank of every active env within its step (block scan per step row),
// add index c = offs[k] + rank, stratum_of_add[c]; plan[k][e] = c or -1
__global__ __launch_bounds__(UPD_THREADS) void lap_ref_plan_scan_kernel(const uint8_t *table, int n,
                                                                        const int32_t *strata, int E,
                                                                        const long long *offs, int32_t *add_s,
                                                                        int32_t *plan) {
    const int k = blockIdx.x, t = threadIdx.x;
    __shared__ int wsum[UPD_THREADS / 64];
    __shared__ int chunk_total;
    const uint8_t *A = table + (size_t)k * n;
    int32_t *P = plan + (size_t)k * n;
    long long offset = offs[k];
    for (int base = 0; base < n; base += STORE_CHUNK) {
        int f[4], sk[4], cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + 4 * t + j;
            sk[j] = i < n ? strata[i] : -1;
            f[j] = (i < n && sk[j] >= 0 && sk[j] < E && A[i]) ? 1 : 0;
            cnt += f[j];
        }
        int total;
        long long c = offset + block_scan_excl(cnt, wsum, &chunk_total, total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = base + 4 * t + j;
            if (i >= n) continue;
            if (f[j]) {
                add_s[c] = sk[j];
                P[i] = (int32_t)c;
                ++c;
            } else {
                P[i] = -1;
            }
        }
        offset += total;
        __syncthreads();
    }
}

// pass 2: add c -> its slot, or -1 when a later add of its slot group (the
// adds sharing ceil((count0 + c) / E)) has the same stratum
__global__ __launch_bounds__(256) void lap_ref_plan_slots_kernel(int32_t *plan, long long entries,
                                                                 const int32_t *add_s, long long total,
                                                                 const long long *ref, int E, int capacity) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= entries) return;
    const int c = plan[i];
    if (c < 0) return;
    const long long ptr0 = ref[0], count0 = ref[1];
    const long long m0 = mult_below(count0, E), mr = mult_below(count0 + c, E);
    const long long qend = min(mr * E - count0, total - 1);
    const int s = add_s[c];
    bool win = true;
    for (long long q = c + 1; q <= qend; ++q) win &= add_s[q] != s;
    plan[i] = win ? ref_slot(ptr0, m0, mr, capacity) : -1;
}

// one step of the planned round: env e's transition to its slot, the episode
// score (:144) and the next mask -- one wavefront per env, 4 per workgroup.
// The step index lives in kk[par] (the trainers' observation parity); the
// launch writes k + 1 to kk[par ^ 1] (and *k_dev), so no workgroup reads a
// counter another one advances.
__global__ __launch_bounds__(256) void lap_ref_step_kernel(lap_storage_desc st, const int32_t *plan, int rows, int n,
                                                           long long *kk, int par, long long *k_dev,
                                                           const int32_t *strata, int capacity, Rows in,
                                                           const uint8_t *table, uint8_t *active, int32_t *count,
                                                           const int32_t *counts_table, double *score) {
    const long long k = kk[par];
    const long long k1 = k + 1 < rows ? k + 1 : rows - 1;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        kk[par ^ 1] = k1;
        if (k_dev) *k_dev = k1;
        if (count) *count = counts_table[k1];
    }
    if (e >= n) return;
    const int slot = k < rows ? plan[(size_t)k * n + e] : -1;
    if (slot >= 0) store_row_wave(st, in, (long)strata[e] * (capacity + 1) + slot, e, lane);
    if (lane == 0) {
        if (score) score[e] += active[e] ? (double)in.reward[e] : 0.0;
        active[e] = table[(size_t)k1 * n + e];
    }
}

// the round's leaves (max_priority) at every planned slot
__global__ __launch_bounds__(256) void lap_ref_commit_leaves_kernel(const int32_t *plan, long long entries, int n,
                                                                    const int32_t *strata, float *tree, int cap,
                                                                    const float *maxp) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= entries) return;
    const int slot = plan[i];
    if (slot < 0) return;
    stratum_tree(tree, strata[i % n], cap)[cap + slot] = *maxp;
}

// the round's ring span recomputed per stratum (one workgroup each)
__global__ __launch_bounds__(UPD_THREADS) void lap_ref_commit_tree_kernel(float *tree, int cap, int levels,
                                                                          int capacity, const long long *ref,
                                                                          long long total, int E) {
    const long long ptr0 = ref[0], count0 = ref[1];
    if (total <= 0) return;
    // the round's adds land in slots ptr0 .. ptr0 + last: the last add's slot
    // is ptr0 + adv (not ptr0 + adv - 1) unless count0 + total - 1 is a
    // multiple of E -- the same span as the per-step insert's (:959)
    const long long last = mult_below(count0 + total - 1, E) - mult_below(count0, E);
    propagate_span(stratum_tree(tree, blockIdx.x, cap), cap, levels, capacity, (int)ptr0,
                   (int)min(last + 1, (long long)capacity));
}

// the pointer and sizes after the round
__global__ void lap_ref_commit_ref_kernel(long long *ref, long long total, int E, int capacity, int32_t *ring_size) {
    const RefState nx = ref_advance(ref[0], ref[1], ref[2], total, E, capacity);
    for (int s = 0; s < E; ++s) ring_size[s] = (int32_t)nx.size;
    ref[0] = nx.ptr;
    ref[1] = nx.count;
    ref[2] = nx.size;
}

// The sampled rows gathered by their own launch (r05): lap_update_sample's
// stratum workgroups stop at the indices, and DRAWS draws per 256-thread
// workgroup here copy state, next_state (float4 where aligned), action,
// reward and not_done -- 64 workgroups for the bench's 8 x 128 batch instead
// of the 8 that ran the update (9.7 of its 24.7 us, r05g).
constexpr int GATHER_DRAWS = 16;

// The storage row of a draw and the batch row d it is gathered into.
struct Draw {
    long d, row;
};

// gather: (draw, item) over the nt threads t, `count` draws with draw_of(q) =
// the q-th one's Draw; items = state, next_state (float4 where the rows are
// 16-byte aligned), action, reward, not_done; GU items per thread loaded
// before any is stored (the stores may alias the loads as far as the compiler
// knows: item by item, every load would wait for the previous store -- r04
// first cut, 54 us per launch)
template <int GU, class DrawOf>
__device__ __forceinline__ void gather_rows(const lap_storage_desc &st, const Outs &o, int count, int t, int nt,
                                            DrawOf draw_of) {
    const int sd = st.state_dim, ad = st.action_dim;
    const bool v4 = rows_vec(st, o.state, o.next_state);
    const int sv = v4 ? sd / 4 : sd, per = 2 * sv + ad + 2;
    const int items = count * per;
    for (int it0 = t; it0 < items; it0 += GU * nt) {
        float4 v[GU];
        float *dst[GU];
        bool wide[GU];
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            const int it = it0 + u * nt;
            dst[u] = nullptr;
            wide[u] = false;
            if (it >= items) continue;
            const int q = it / per, c = it - q * per;
            const Draw w = draw_of(q);
            const long d = w.d, row = w.row;
            if (c < 2 * sv) {
                const bool nx = c >= sv;
                const int e = nx ? c - sv : c;
                const float *src = (nx ? st.next_state : st.state) + row * sd;
                float *out = (nx ? o.next_state : o.state) + d * sd;
                if (v4) {
                    v[u] = ld4(src + 4 * e);
                    dst[u] = out + 4 * e;
                    wide[u] = true;
                } else {
                    v[u].x = src[e];
                    dst[u] = out + e;
                }
            } else if (c < 2 * sv + ad) {
                const int e = c - 2 * sv;
                v[u].x = st.action[row * ad + e];
                dst[u] = o.action + d * ad + e;
            } else if (c == 2 * sv + ad) {
                v[u].x = st.reward[row];
                dst[u] = o.reward + d;
            } else {
                v[u].x = st.not_done[row];
                dst[u] = o.not_done + d;
            }
        }
#pragma unroll
        for (int u = 0; u < GU; ++u) {
            if (!dst[u]) continue;
            if (wide[u]) st4(dst[u], v[u]);
            else *dst[u] = v[u].x;
        }
    }
}

__global__ __launch_bounds__(256) void lap_gather_kernel(lap_storage_desc st, int capacity, const int32_t *idx,
                                                         int batch, int total, Outs o) {
    const int d0 = blockIdx.x * GATHER_DRAWS;
    gather_rows<4>(st, o, min(GATHER_DRAWS, total - d0), threadIdx.x, 256, [=](int q) {
        const long d = d0 + q;
        return Draw{d, (long)(d / batch) * (capacity + 1) + idx[d]};
    });
}

// LAP.update_priority (:113-117) and the NEXT LAP.sample (:65-111) as ONE
// launch (r04: lap_update_kernel + lap_sample_gather_kernel were 32 us plus a
// queue hand-off at the end of every critic-only iteration).  One workgroup
// per stratum: the update exactly as lap_update_kernel (last duplicate wins,
// level-synchronous ancestors, the max_priority atomic), whose staged top
// levels stay in LDS; then the stratum's `batch` draws (Philox block d =
// s * batch + b of call *counter, as lap_sample_gather_kernel) descend with
// the nodes below TOPN read from LDS, and the workgroup gathers their rows.
// The same sums and comparisons: bit-identical to the two launches.
// tp (lap_update_sample_td): the priorities computed here, see TdPrio.

// lap_update_sample's own gather (EXO_LAP_GATHER_SPLIT=0): the rows pick[0 .. batch)
// of stratum s, by the whole workgroup.
__device__ __forceinline__ void gather_picked(const lap_storage_desc &st, const Outs &o, int capacity, int s,
                                              int batch, const int32_t *pick) {
    gather_rows<8>(st, o, min(batch, UPD_THREADS), threadIdx.x, UPD_THREADS, [=](int b) {
        return Draw{(long)s * batch + b, (long)s * (capacity + 1) + pick[b]};
    });
}

__global__ __launch_bounds__(UPD_THREADS) void lap_update_sample_kernel(float *tree, float *maxp, int cap, int levels,
                                                                        int capacity, const int32_t *idx_in,
                                                                        const float *prio, int batch,
                                                                        const int32_t *size, lap_storage_desc st,
                                                                        SampleRng rng, int32_t *idx_out, Outs o,
                                                                        TdPrio tp, bool gather) {
    const int s = blockIdx.x;
    float *T = stratum_tree(tree, s, cap);
    const int32_t *I = idx_in + (size_t)s * batch;
    __shared__ float red[UPD_THREADS / 64];
    __shared__ int32_t li[UPD_THREADS];
    __shared__ float top[TOPN_US];
    __shared__ int32_t pick[UPD_THREADS];
    const unsigned long long call = *rng.counter;  // read before any workgroup can take the ticket
    float mx = update_leaves(T, cap, I, batch, tp, prio + (size_t)s * batch, s, li);
    mx = wave_max_to(red, mx);
    const bool staged = propagate_top<TOPN_US>(T, cap, levels, I, batch, top);
    block_max_to(maxp, mx, red);
    // ---- the next batch of this stratum
    const int lim = staged ? min(TOPN_US, 2 * cap) : 0;
    auto node_at = [&](int node) { return node < lim ? top[node] : T[node]; };
    const int sz = size[s];
    const float tot = prefix_sum(node_at, cap, levels, sz);
    for (int b = threadIdx.x; b < batch; b += UPD_THREADS) {
        const int d = s * batch + b;
        uint32_t r[4];
        philox_block(rng.seed, rng.tag, call, (uint32_t)d, r);
        float val = u01_open_hi(r[0]) * tot;
        // the staged top levels from LDS one level at a time, the rest (below
        // TOPN) three levels per round trip
        int node = 1, lv = 0;
        for (; lv < levels && 2 * node + 1 < lim; ++lv) {
            const float left = top[2 * node], right = top[2 * node + 1];
            if ((val <= left && left > 0.0f) || right <= 0.0f) {
                node = 2 * node;
            } else {
                val -= left;
                node = 2 * node + 1;
            }
        }
        node = descend_from([T](int n) { return T[n]; }, val, node, lv, levels);
        int i = node - cap;
        if (i >= sz) i = sz > 0 ? sz - 1 : 0;
        idx_out[d] = i;
        if (b < UPD_THREADS) pick[b] = i;
    }
    __syncthreads();
    if (gather) {  // (else the rows follow in lap_gather_kernel)
        gather_picked(st, o, capacity, s, batch, pick);
        __syncthreads();
    }
    if (threadIdx.x == 0) rng_ticket(rng, call);  // `call` was read (and used) before this add: no fence needed
}

// lap_update_sample_kernel with its dependent global-memory round trips
// collapsed (batch <= CHAIN_MAXB; EXO_LAP_CHAIN=0 or a larger batch: the kernel
// above).  That kernel waits for memory about 20 times in a row at the
// bench's shape (cap 2^18, G = 6 levels below the staged top): the counter
// and indices, the priorities, two trips for each global level (the index
// re-read, then the children; every level's barrier also waits for the
// level's stores), the staging, the sizes, the prefix walk, two for the
// descent and the ticket; the 12 LDS levels re-read their index from global
// memory as well.  Here, from the start to the idx_out store, a thread waits
// for memory 4 times, and once more for the ticket -- 5 dependent trips:
//   1. everything that depends on nothing, in one batch: the call counter,
//      size[s], the draw's index (kept in a register from here on), its
//      priority (or |td| pair) and the staged top of the tree (8 loads);
//   2. the siblings of the draw's G global ancestors (lap_chain.h) and the
//      prefix walk's G addends below the staged top (the siblings of leaf
//      size[s]'s ancestors: thread `batch` loads them as if leaf size[s]
//      were its draw), as soon as the index and the size are there.
//      While they fly the workgroup finds the superseded duplicates and the
//      chain partners in LDS.  The G levels are then G LDS-only barriers; the
//      sums also go to the tree, stores nothing waits for.  A prefix addend
//      this update changes is taken from the chain (leaf size[s] is one more
//      row of the partner table), and the level-G values patch the staged
//      top: both were loaded before this launch changed them;
//   3., 4. the descent below the staged top, three levels per trip, after a
//      barrier that finds the chain's stores long complete;
//   5. the tail: the ticket's atomic, after the idx_out store.
// What the phase stamps showed (profiles/lap_chain/README.md): neither kernel
// is a pure latency chain.  Trip 2 is bound by the CU's rate of missed lines
// (batch x G scattered 64-byte lines, about 6 cycles each), and the rest by
// the instructions the two waves that hold the draws execute once each -- so
// work those waves need not do is kept off them: the partner scan is spread
// over the workgroup four slots per LDS read, the uniforms are drawn by waves
// of other SIMDs, the batch maximum is reduced by the last wave.
// The same operands in the same order as lap_update_kernel's level sweeps and
// lap_sample_gather_kernel's walks: every node, index and row bit-identical
// (tests/test_lap_chain_host.py, tests/test_lap_update_sample_chain_gpu.py).
// idx_in may be idx_out (the caller's previous batch in the same slot): the
// index is read once, at the start, by the thread that later writes it.
constexpr int CHAIN_MAXB = 256;  // batch bound: LDS, and 1,024 threads give each table row >= 2 scanning threads
constexpr int CHAIN_MAXG = 12;   // global levels (cap 2^24 under an 8,192-node top)
constexpr int CHAIN_ROW = CHAIN_MAXB + 1;  // the draws and leaf size[s]
constexpr int CHAIN_TOPLV = 12;            // at most this many levels in the staged top
static_assert((2 << CHAIN_TOPLV) >= TOPN_US, "CHAIN_TOPLV: the staged top's levels");
constexpr int CHAIN_PAD = 0x40000000;      // li[] padding: no slot's duplicate or partner (slots are < 2^24)
constexpr int CHAIN_RNG0 = 640;            // the threads that draw the uniforms (waves on other SIMDs than the draws')

// A workgroup barrier for LDS traffic alone: __syncthreads() would also wait
// for the wave's global stores and, with them, for every load in flight.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(UPD_THREADS) void lap_update_sample_chain_kernel(
    float *tree, float *maxp, int cap, int levels, int capacity, const int32_t *idx_in,
    const float *__restrict__ prio, int batch, const int32_t *__restrict__ size, lap_storage_desc st, SampleRng rng,
    int32_t *idx_out, Outs o, TdPrio tp, bool gather) {
    const int s = blockIdx.x, t = threadIdx.x;
    float *T = stratum_tree(tree, s, cap);
    __shared__ float red[UPD_THREADS / 64];
    __shared__ __attribute__((aligned(16))) int32_t li[CHAIN_MAXB + 4];  // the draws' slots, padded to a multiple of 4
    __shared__ int32_t lsz;                              // leaf size[s], row `batch` of the partner table
    __shared__ float uni[CHAIN_MAXB];                    // the draws' uniforms
    __shared__ int32_t later[CHAIN_MAXB];                // a later duplicate of the draw's slot exists
    __shared__ int32_t partner[CHAIN_MAXG * CHAIN_ROW];  // [lv][b]: the draw below b's level-lv sibling, or -1
    __shared__ float chain[2][CHAIN_MAXB];
    __shared__ float lowval[CHAIN_MAXG];                 // the prefix addends below the staged top, final
    __shared__ float top[TOPN_US];
    __shared__ int32_t pick[CHAIN_MAXB];
    const int G = lap_chain::global_levels(levels, TOPN_US);
    const int lim = min(TOPN_US, 2 * cap);
    const bool draw = t < batch;
    const long d = (long)s * batch + (draw ? t : 0);
    // ---- trip 1: nothing here depends on a load (addresses clamped, not
    // branched around: every load is issued before the first wait)
    const unsigned long long call = *rng.counter;  // read before any workgroup can take the ticket
    const int sz = size[s];
    const int me = idx_in[d];
    const float *pp = tp.td ? tp.td + 2 * d : prio + d;
    const float p0 = pp[0], p1 = pp[tp.td ? 1 : 0];  // the priority, or the |td| pair
    constexpr int PER = TOPN_US / UPD_THREADS;
    float stage[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) stage[j] = T[min(t + j * UPD_THREADS, lim - 1)];
    for (int i = t; i < G * CHAIN_ROW; i += UPD_THREADS) partner[i] = -1;
    if (t < CHAIN_MAXB + 4) li[t] = draw ? me : CHAIN_PAD;
    if (draw) later[t] = 0;
    if (t >= CHAIN_RNG0 && t < CHAIN_RNG0 + batch) {  // draw t - CHAIN_RNG0's uniform, off the draws' waves
        uint32_t r[4];
        philox_block(rng.seed, rng.tag, call, (uint32_t)(s * batch + t - CHAIN_RNG0), r);
        uni[t - CHAIN_RNG0] = u01_open_hi(r[0]);
    }
    const int szl = min(sz, cap - 1);  // the prefix walk's leaf (sz >= cap: the root is the total)
    // thread `batch` stands for leaf sz: its siblings are the prefix walk's addends
    const int leaf = t == batch ? szl : me;
    if (t == batch) lsz = szl;
    // ---- trip 2: the siblings of the leaf's global ancestors
    float sib[CHAIN_MAXG];
#pragma unroll
    for (int lv = 0; lv < CHAIN_MAXG; ++lv) sib[lv] = 0.0f;
    if (t <= batch) {
#pragma unroll
        for (int lv = 0; lv < CHAIN_MAXG; ++lv) sib[lv] = T[lap_chain::sibling_of(cap, leaf, min(lv, max(G - 1, 0)))];
    }
    lds_barrier();
    {   // superseded duplicates and partners: table row b scanned by 2^lp threads, four slots per read;
        // a slot is a duplicate (xor 0), a partner (xor below 2^G) or, nearly always, neither
        int lp = 0;
        while (((batch + 1) << (lp + 1)) <= UPD_THREADS) ++lp;
        const int b = t >> lp, part = t & ((1 << lp) - 1);
        const int chunk = (((batch + 3) >> 2) + (1 << lp) - 1) >> lp;  // reads of four slots per thread
        if (b <= batch) {
            const int mine = b < batch ? li[b] : lsz;
            const unsigned near = 1u << G;
            bool sup = false;
            for (int q = part * chunk; q < (part + 1) * chunk && 4 * q < batch; ++q) {
                const int4 o = *reinterpret_cast<const int4 *>(&li[4 * q]);
                const int other[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = 4 * q + j;
                    if ((unsigned)(mine ^ other[j]) >= near) continue;
                    const int lv = lap_chain::partner_level(mine, other[j]);
                    if (lv < 0) sup |= b < batch && lap_chain::superseded_by(b, mine, k, other[j]);
                    else atomicMax(&partner[lv * CHAIN_ROW + b], k);
                }
            }
            if (sup) later[b] = 1;
        }
    }
    const float pb = !draw ? 0.0f : tp.td ? powf(fmaxf(fmaxf(p0, p1), tp.minp), tp.alpha) : p0;
    float mx = pb;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((t & 63) == 0) red[t >> 6] = mx;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = t + j * UPD_THREADS;
        if (i < lim) top[i] = stage[j];
    }
    lds_barrier();
    const bool carry = draw && !later[t];  // the last duplicate of its slot: it writes the leaf and runs the chain
    if (draw && tp.td && tp.out) tp.out[d] = pb;
    float cur = pb;
    if (carry) {
        T[cap + me] = pb;
        chain[0][t] = pb;
    }
    if (t == batch) {  // the prefix addends no draw changes: as loaded
#pragma unroll
        for (int lv = 0; lv < CHAIN_MAXG; ++lv)
            if (lv < G && partner[lv * CHAIN_ROW + batch] < 0) lowval[lv] = sib[lv];
    }
#pragma unroll
    for (int lv = 0; lv < CHAIN_MAXG; ++lv) {
        if (lv < G) lds_barrier();
        if (lv < G && carry) {
            if (partner[lv * CHAIN_ROW + batch] == t) lowval[lv] = cur;
            const int node = lap_chain::node_of(cap, me, lv), k = partner[lv * CHAIN_ROW + t];
            cur = lap_chain::chain_step(node, cur, k >= 0 ? chain[lv & 1][k] : sib[lv]);
            T[node >> 1] = cur;
            chain[(lv + 1) & 1][t] = cur;
        }
    }
    if (carry) top[lap_chain::node_of(cap, me, G)] = cur;  // the staged value was loaded before this update
    for (int lv = G + 1; lv <= levels; ++lv) {
        lds_barrier();
        if (draw) {
            const int node = lap_chain::node_of(cap, me, lv);
            top[node] = top[2 * node] + top[2 * node + 1];
        }
    }
    __syncthreads();  // the tree's global levels are final for every thread of the workgroup
    const int wb = min(TOPN_US / 2, cap);
    for (int i = 1 + t; i < wb; i += UPD_THREADS) T[i] = top[i];
    if (t >= UPD_THREADS - 64) {  // the last wave (no draws there): the batch's largest priority
        float m = red[t & (UPD_THREADS / 64 - 1)];
        for (int o = UPD_THREADS / 128; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        // priorities are >= min_priority^alpha > 0: int order == float order
        if (t == UPD_THREADS - 64) atomicMax(reinterpret_cast<int *>(maxp), __float_as_int(m));
    }
    // ---- the next batch of this stratum
    if (draw) {
        const int ltop = levels - G;  // the levels of the staged top
        float tot;
        if (sz >= cap) {
            tot = top[1];
        } else {  // prefix_sum's additions in its order: the staged steps (read together), then the global ones
            float x[CHAIN_TOPLV];
#pragma unroll
            for (int j = 0; j < CHAIN_TOPLV; ++j) {
                const int lv = levels - 1 - j;
                x[j] = j < ltop ? top[2 * ((1 << j) | (sz >> (lv + 1)))] : 0.0f;
            }
            tot = 0.0f;
#pragma unroll
            for (int j = 0; j < CHAIN_TOPLV; ++j)
                if (j < ltop) tot += ((sz >> (levels - 1 - j)) & 1) ? x[j] : 0.0f;
#pragma unroll
            for (int lv = CHAIN_MAXG - 1; lv >= 0; --lv) {
                if (lv >= G) continue;
                tot += ((sz >> lv) & 1) ? lowval[lv] : 0.0f;
            }
        }
        float val = uni[t] * tot;
        // the staged levels from LDS one at a time, then (trips 3, 4) the global ones, three per trip
        int node = 1;
        for (int lv = 0; lv < ltop; ++lv) {
            const float left = top[2 * node], right = top[2 * node + 1];
            if ((val <= left && left > 0.0f) || right <= 0.0f) {
                node = 2 * node;
            } else {
                val -= left;
                node = 2 * node + 1;
            }
        }
        node = descend_from([T](int n) { return T[n]; }, val, node, ltop, levels);
        int i = node - cap;
        if (i >= sz) i = sz > 0 ? sz - 1 : 0;
        idx_out[d] = i;
        pick[t] = i;
    }
    __syncthreads();
    if (gather) {
        gather_picked(st, o, capacity, s, batch, pick);
        __syncthreads();
    }
    // ---- trip 5; `call` was read (and used) before this add: no fence needed
    if (t == 0) rng_ticket(rng, call);
}

// ---------------------------------------------------------------- behaviour-policy column, views
// source[n_strata][capacity + 1] (int32, -1 = untagged) names the behaviour
// policy of every stored row; it is laid out like reward / not_done, so the
// storage row index r = s (capacity + 1) + slot addresses it.

// lap_store_copy_kernel that also writes the row's source (src == nullptr: -1).
// Inactive rows land in the trash row `capacity`, rows without a stratum
// (row_of < 0) write nothing.
__global__ __launch_bounds__(256) void lap_store_copy_src_kernel(lap_storage_desc st, Rows in, int n,
                                                                 const int32_t *row_of, const int32_t *src,
                                                                 int32_t *source) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const long r = row_of[i];
    if (r < 0) return;
    store_row_wave(st, in, r, i, lane);
    if (lane == 0) source[r] = src ? src[i] : -1;
}

// Rows per source id of every stratum, slots < size[s] only: out[s][id] for
// 0 <= id < K, out[s][K] the untagged rows (ids >= K are not counted).  The
// workgroups of a stratum (blockIdx.x) each count COUNT_SLOTS slots in an LDS
// histogram and add their non-zero bins to `out` (zeroed by the launcher).
// A thread loads COUNT_U slots before it counts any of them: one slot per
// round trip left the launch waiting for memory 64 times in a row.
constexpr int COUNT_THREADS = 256;
constexpr int COUNT_MAXK = 4096;
constexpr int COUNT_SLOTS = 16384;  // slots per workgroup
constexpr int COUNT_U = 8;          // loads in flight per thread
__global__ __launch_bounds__(COUNT_THREADS) void lap_source_counts_kernel(const int32_t *source, int capacity,
                                                                          const int32_t *size, int K,
                                                                          unsigned long long *out) {
    __shared__ int hist[COUNT_MAXK + 1];
    const int s = blockIdx.y, t = threadIdx.x;
    const int sz = min(size[s], capacity);
    const int32_t *col = source + (size_t)s * (capacity + 1);
    for (int k = t; k <= K; k += COUNT_THREADS) hist[k] = 0;
    __syncthreads();
    const int lo = blockIdx.x * COUNT_SLOTS, hi = min(sz, lo + COUNT_SLOTS);
    for (int i0 = lo + t; i0 < hi; i0 += COUNT_U * COUNT_THREADS) {
        int v[COUNT_U];
#pragma unroll
        for (int u = 0; u < COUNT_U; ++u) {
            const int i = i0 + u * COUNT_THREADS;
            v[u] = i < hi ? col[i] : K;  // K: not counted
        }
#pragma unroll
        for (int u = 0; u < COUNT_U; ++u)
            if (v[u] < K) atomicAdd(&hist[v[u] < 0 ? K : v[u]], 1);
    }
    __syncthreads();
    for (int k = t; k <= K; k += COUNT_THREADS)
        if (hist[k]) atomicAdd(&out[(size_t)s * (K + 1) + k], (unsigned long long)hist[k]);
}

// lap_view_build: the trees of a view over the same rows.  Leaf i of stratum
// s is base leaf i (inherit) or 1 when i < size[s], source >= 0 and
// keep[source], else 0; every internal node is T[2n] + T[2n + 1] of its final
// children -- the sums propagate / propagate_span compute, so a view that
// keeps every row and inherits is the base's tree bit for bit.
// Pass 1 (grid: leaf blocks x strata): a workgroup owns VIEW_LEAVES
// consecutive leaves (the whole stratum when cap is smaller): the kept mask
// from coalesced source loads into LDS, the leaves as float4 stores, then the
// block's own subtree level by level in LDS -- local node n at depth d (w =
// 2^d nodes) is node root * w + (n - w) of the tree.  With inherit the block's
// largest kept leaf goes to max_priority (zeroed by the launcher) with one
// atomic; without, max_priority = 1.
// Pass 2 (one workgroup per stratum, only when cap > VIEW_LEAVES, a later
// launch): the cap / VIEW_LEAVES subtree roots pass 1 wrote, reduced to node
// 1 in LDS.  No workgroup reads what another wrote in the same launch.
constexpr int VIEW_LEAVES = 4096;
constexpr int VIEW_THREADS = 512;
static_assert((1 << MAXLV) / VIEW_LEAVES <= VIEW_LEAVES, "pass 2 holds the subtree roots in 2 VIEW_LEAVES floats");
__global__ __launch_bounds__(VIEW_THREADS) void lap_view_leaves_kernel(float *tree, float *maxp, const float *base,
                                                                       int cap, int capacity, const int32_t *size,
                                                                       const int32_t *source, const uint8_t *keep,
                                                                       int n_keep, bool inherit) {
    __shared__ __attribute__((aligned(16))) float lt[2 * VIEW_LEAVES];
    __shared__ float red[VIEW_THREADS / 64];
    const int s = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
    const int nl = min(VIEW_LEAVES, cap);  // this block's leaves [i0, i0 + nl)
    const int i0 = b * nl, root = cap / nl + b;
    float *T = stratum_tree(tree, s, cap);
    const float *B = base + (size_t)s * 2 * cap + cap;
    const int sz = min(size[s], capacity);
    const int32_t *col = source + (size_t)s * (capacity + 1);
    for (int j = t; j < nl; j += VIEW_THREADS) {
        const int i = i0 + j;
        const int v = i < sz ? col[i] : -1;
        lt[nl + j] = (v >= 0 && v < n_keep && keep[v]) ? 1.0f : 0.0f;
    }
    __syncthreads();
    float mx = 0.0f;
    if ((nl & 3) == 0) {
        for (int q = t; q < nl / 4; q += VIEW_THREADS) {
            float4 v = *reinterpret_cast<const float4 *>(&lt[nl + 4 * q]);
            if (inherit) {
                const float4 p = ld4(B + i0 + 4 * q);
                v.x = v.x != 0.0f ? p.x : 0.0f;
                v.y = v.y != 0.0f ? p.y : 0.0f;
                v.z = v.z != 0.0f ? p.z : 0.0f;
                v.w = v.w != 0.0f ? p.w : 0.0f;
                *reinterpret_cast<float4 *>(&lt[nl + 4 * q]) = v;
                mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
            }
            st4(T + cap + i0 + 4 * q, v);
        }
    } else {  // cap 1 or 2
        for (int j = t; j < nl; j += VIEW_THREADS) {
            float v = lt[nl + j];
            if (inherit) {
                v = v != 0.0f ? B[i0 + j] : 0.0f;
                lt[nl + j] = v;
                mx = fmaxf(mx, v);
            }
            T[cap + i0 + j] = v;
        }
    }
    for (int w = nl / 2; w >= 1; w >>= 1) {
        __syncthreads();
        for (int j = t; j < w; j += VIEW_THREADS) {
            const int n = w + j;
            const float v = lt[2 * n] + lt[2 * n + 1];
            lt[n] = v;
            T[(size_t)root * w + j] = v;
        }
    }
    if (inherit) {
        mx = wave_max_to(red, mx);
        __syncthreads();
        block_max_to(maxp, mx, red);  // leaves >= 0: int order == float order
    } else if (s == 0 && b == 0 && t == 0) {
        *maxp = 1.0f;
    }
}

__global__ __launch_bounds__(UPD_THREADS) void lap_view_top_kernel(float *tree, int cap) {
    __shared__ float top[2 * VIEW_LEAVES];
    float *T = stratum_tree(tree, blockIdx.x, cap);
    const int nb = cap / VIEW_LEAVES, t = threadIdx.x;  // the subtree roots are nodes [nb, 2 nb)
    for (int j = t; j < nb; j += UPD_THREADS) top[nb + j] = T[nb + j];
    for (int w = nb / 2; w >= 1; w >>= 1) {
        __syncthreads();
        for (int j = t; j < w; j += UPD_THREADS) {
            const int n = w + j;
            const float v = top[2 * n] + top[2 * n + 1];
            top[n] = v;
            T[n] = v;
        }
    }
}

// lap_views_follow: the live views of a buffer after one lap_store_batch(_src).
// Workgroup (s, v) scans the insert's row_of: every row that landed in a real
// slot of stratum s (not the trash row, not -1) gets view v's leaf -- the
// view's max_priority when the row's source is kept (LAP.add's rule, on the
// view's own maximum), else 0, which also takes an evicted kept row out of the
// view.  The slots of one insert in one stratum are distinct (one add_batch
// must not wrap a ring onto itself), so every leaf has one writer, and they
// are the `cnt` ring slots that end at the ring pointer the rank kernel left:
// their ancestors are recomputed by propagate_span, the same sums as the
// insert's own.  kept[s] follows the change in positive leaves.
__global__ __launch_bounds__(UPD_THREADS) void lap_views_follow_kernel(const lap_view_entry *views, int cap,
                                                                       int levels, int capacity,
                                                                       const int32_t *ring_ptr, const int32_t *row_of,
                                                                       const int32_t *src, int n) {
    const int s = blockIdx.x, t = threadIdx.x;
    const lap_view_entry V = views[blockIdx.y];
    // an entry cleared since the launch was recorded (a view detached, the captured
    // insert replayed with the old n_views): nothing to follow, the whole workgroup
    if (!V.tree || !V.max_priority || !V.kept) return;
    float *T = stratum_tree(V.tree, s, cap);
    __shared__ int wcnt[UPD_THREADS / 64], wdelta[UPD_THREADS / 64];
    const float p = *V.max_priority;
    const int row0 = s * (capacity + 1);
    int cnt = 0, delta = 0;  // rows written, change in positive leaves
    for (int i = t; i < n; i += UPD_THREADS) {
        const int r = row_of[i];
        if (r < row0 || r >= row0 + capacity) continue;
        const int id = src ? src[i] : -1;
        const bool kept = id >= 0 && id < V.n_keep && V.keep[id];
        const float leaf = kept ? p : 0.0f;
        float *L = T + cap + (r - row0);
        delta += (leaf > 0.0f) - (*L > 0.0f);
        *L = leaf;
        ++cnt;
    }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        delta += __shfl_xor(delta, o, 64);
    }
    if ((t & 63) == 0) {
        wcnt[t >> 6] = cnt;
        wdelta[t >> 6] = delta;
    }
    __syncthreads();
    cnt = delta = 0;
    for (int w = 0; w < UPD_THREADS / 64; ++w) {
        cnt += wcnt[w];
        delta += wdelta[w];
    }
    if (cnt == 0) return;  // the whole workgroup: nothing of this insert in stratum s
    const int first = ((ring_ptr[s] - cnt) % capacity + capacity) % capacity;
    propagate_span(T, cap, levels, capacity, first, cnt);
    if (t == 0) V.kept[s] += delta;
}

int rc(hipError_t e) { return e == hipSuccess ? EXO_OK : EXO_EDEVICE; }

int levels_of(const lap_tree_desc *t) {
    int lv = 0;
    while ((1 << lv) < t->cap) ++lv;
    return lv;
}

// lap_update_sample's rows gathered by lap_gather_kernel (EXO_LAP_GATHER_SPLIT=0:
// by the update's own stratum workgroups, the r04 layout)
bool env_not_zero(const char *name) {  // unset, or not "0..."
    const char *e = getenv(name);
    return !(e && e[0] == '0');
}
bool gather_split() {
    static const bool on = env_not_zero("EXO_LAP_GATHER_SPLIT");
    return on;
}

// lap_update_sample's launch: the sibling-chain kernel up to CHAIN_MAXB draws per
// stratum (EXO_LAP_CHAIN=0: always lap_update_sample_kernel, the level sweeps;
// read per call, the parity test switches it).  Both compute the same bits.
void launch_update_sample(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *idx_in, const float *prio,
                          int batch, SampleRng rng, int32_t *idx_out, const Outs &o, TdPrio tp, bool gather,
                          void *stream) {
    const int levels = levels_of(t);
    const bool chain = env_not_zero("EXO_LAP_CHAIN") && batch <= CHAIN_MAXB && levels >= 1 &&
                       lap_chain::global_levels(levels, TOPN_US) <= CHAIN_MAXG;
    if (chain)
        hipLaunchKernelGGL(lap_update_sample_chain_kernel, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream,
                           t->tree, t->max_priority, t->cap, levels, t->capacity, idx_in, prio, batch, st->size, *st,
                           rng, idx_out, o, tp, gather);
    else
        hipLaunchKernelGGL(lap_update_sample_kernel, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream,
                           t->tree, t->max_priority, t->cap, levels, t->capacity, idx_in, prio, batch, st->size, *st,
                           rng, idx_out, o, tp, gather);
}

int launch_gather(const lap_tree_desc *t, const lap_storage_desc *st, int batch, const int32_t *idx, const Outs &o,
                  void *stream) {
    const int total = t->n_strata * batch;
    hipLaunchKernelGGL(lap_gather_kernel, dim3((total + GATHER_DRAWS - 1) / GATHER_DRAWS), dim3(256), 0,
                       (hipStream_t)stream, *st, t->capacity, idx, batch, total, o);
    return rc(hipGetLastError());
}

int gather_after(const lap_tree_desc *t, const lap_storage_desc *st, int batch, const int32_t *idx, const Outs &o,
                 void *stream) {
    if (hipGetLastError() != hipSuccess) return EXO_EDEVICE;
    if (!gather_split()) return EXO_OK;
    return launch_gather(t, st, batch, idx, o, stream);
}

bool valid(const lap_tree_desc *t) {
    // cap <= 2^MAXLV: prefix_sum unrolls MAXLV levels
    return t && t->tree && t->max_priority && t->n_strata > 0 && t->capacity > 0 && t->cap >= t->capacity &&
           (t->cap & (t->cap - 1)) == 0 && t->cap <= (1 << MAXLV);
}

bool storage_ok(const lap_storage_desc *st) {  // the five row arrays
    return st && st->state && st->action && st->next_state && st->reward && st->not_done;
}
bool rows_ok(const Rows &in) {
    return in.state && in.action && in.next_state && in.reward && in.done && in.action_scale != 0.0f;
}
// what the three inserts (lap_store_batch, lap_store_batch_ref, the fused ref insert) all require
bool store_args_ok(const lap_tree_desc *t, const lap_storage_desc *st, const Rows &in, const int32_t *strata, int n) {
    return valid(t) && storage_ok(st) && st->size && st->state_dim > 0 && st->action_dim > 0 && rows_ok(in) &&
           strata && n >= 0;
}
bool outs_ok(const Outs &o) { return o.state && o.action && o.next_state && o.reward && o.not_done; }

} // namespace

extern "C" {

int32_t lap_tree_floats(int32_t n_strata, int32_t capacity) {
    int cap = 1;
    while (cap < capacity) cap <<= 1;
    return n_strata * 2 * cap;
}

int lap_init(const lap_tree_desc *t, void *stream) {
    if (!valid(t)) return EXO_EINVAL;
    hipError_t e = hipMemsetAsync(t->tree, 0, (size_t)t->n_strata * 2 * t->cap * sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t->max_priority);
    return rc(hipGetLastError());
}

int lap_add(const lap_tree_desc *t, const int32_t *stratum, const int32_t *slot, int32_t n, void *stream) {
    if (!valid(t) || !stratum || !slot || n < 0) return EXO_EINVAL;
    if (n == 0) return EXO_OK;
    hipLaunchKernelGGL(lap_add_kernel, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream, t->tree,
                       t->max_priority, t->cap, levels_of(t), t->capacity, stratum, slot, n);
    return rc(hipGetLastError());
}

int lap_sample(const lap_tree_desc *t, const float *u, const int32_t *size, int32_t batch, int32_t *idx, void *stream) {
    if (!valid(t) || !u || !size || !idx || batch <= 0) return EXO_EINVAL;
    const int th = 128;
    hipLaunchKernelGGL(lap_sample_kernel, dim3((batch + th - 1) / th, t->n_strata), dim3(th), 0, (hipStream_t)stream,
                       t->tree, t->cap, levels_of(t), u, size, batch, idx);
    return rc(hipGetLastError());
}

int lap_update(const lap_tree_desc *t, const int32_t *idx, const float *prio, int32_t batch, void *stream) {
    if (!valid(t) || !idx || !prio || batch <= 0) return EXO_EINVAL;
    hipLaunchKernelGGL(lap_update_kernel, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream, t->tree,
                       t->max_priority, t->cap, levels_of(t), idx, prio, batch);
    return rc(hipGetLastError());
}

int lap_reset_max(const lap_tree_desc *t, void *stream) {
    if (!valid(t)) return EXO_EINVAL;
    hipError_t e = hipMemsetAsync(t->max_priority, 0, sizeof(float), (hipStream_t)stream);
    if (e != hipSuccess) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_reset_max_kernel, dim3(256), dim3(1024), 0, (hipStream_t)stream, t->tree, t->max_priority,
                       t->cap, t->n_strata);
    return rc(hipGetLastError());
}

int lap_totals(const lap_tree_desc *t, float *out, void *stream) {
    if (!valid(t) || !out) return EXO_EINVAL;
    hipLaunchKernelGGL(lap_totals_kernel, dim3((t->n_strata + 63) / 64), dim3(64), 0, (hipStream_t)stream, t->tree,
                       t->cap, t->n_strata, out);
    return rc(hipGetLastError());
}

// lap_store_batch's first launch: the slots, leaves, span and ring state
static int launch_store_rank(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *strata,
                             const uint8_t *active, int32_t n, int32_t *row_ws, void *stream) {
    if (n > 4 * STORE_CHUNK)
        hipLaunchKernelGGL(lap_store_rank_kernel<16>, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream,
                           t->tree, t->max_priority, t->cap, levels_of(t), t->capacity, st->ptr, st->size, strata,
                           active, n, row_ws);
    else
        hipLaunchKernelGGL(lap_store_rank_kernel<4>, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream,
                           t->tree, t->max_priority, t->cap, levels_of(t), t->capacity, st->ptr, st->size, strata,
                           active, n, row_ws);
    return rc(hipGetLastError());
}

int lap_store_batch_src(const lap_tree_desc *t, const lap_storage_desc *st, const float *state, const float *action,
                        const float *next_state, const float *reward, const uint8_t *done, const int32_t *strata,
                        const uint8_t *active, float action_scale, int32_t n, int32_t *row_ws, const int32_t *src,
                        int32_t *source, void *stream) {
    const Rows in{state, action, next_state, reward, done, action_scale};
    if (!store_args_ok(t, st, in, strata, n) || !st->ptr || !row_ws || !source) return EXO_EINVAL;
    if (n == 0) return EXO_OK;
    if (launch_store_rank(t, st, strata, active, n, row_ws, stream) != EXO_OK) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_store_copy_src_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *st, in, n,
                       row_ws, src, source);
    return rc(hipGetLastError());
}

int lap_source_counts(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *source, int32_t n_sources,
                      int64_t *out, void *stream) {
    if (!valid(t) || !st || !st->size || !source || !out || n_sources < 0 || n_sources > COUNT_MAXK)
        return EXO_EINVAL;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)t->n_strata * (n_sources + 1) * sizeof(int64_t),
                                  (hipStream_t)stream);
    if (e != hipSuccess) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_source_counts_kernel, dim3((t->capacity + COUNT_SLOTS - 1) / COUNT_SLOTS, t->n_strata),
                       dim3(COUNT_THREADS), 0, (hipStream_t)stream, source, t->capacity, st->size, n_sources,
                       (unsigned long long *)out);
    return rc(hipGetLastError());
}

int lap_view_build(const lap_tree_desc *view, const lap_tree_desc *base, const lap_storage_desc *st,
                   const int32_t *source, const uint8_t *keep, int32_t n_keep, int32_t inherit, void *stream) {
    if (!valid(view) || !valid(base) || view->tree == base->tree || view->max_priority == base->max_priority ||
        view->n_strata != base->n_strata || view->capacity != base->capacity || view->cap != base->cap || !st ||
        !st->size || !source || !keep || n_keep <= 0)
        return EXO_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (inherit && hipMemsetAsync(view->max_priority, 0, sizeof(float), s) != hipSuccess) return EXO_EDEVICE;
    const int cap = view->cap, nl = std::min(VIEW_LEAVES, cap);
    hipLaunchKernelGGL(lap_view_leaves_kernel, dim3(cap / nl, view->n_strata), dim3(VIEW_THREADS), 0, s, view->tree,
                       view->max_priority, base->tree, cap, view->capacity, st->size, source, keep, n_keep,
                       inherit != 0);
    if (hipGetLastError() != hipSuccess) return EXO_EDEVICE;
    if (cap > VIEW_LEAVES)
        hipLaunchKernelGGL(lap_view_top_kernel, dim3(view->n_strata), dim3(UPD_THREADS), 0, s, view->tree, cap);
    return rc(hipGetLastError());
}

int lap_views_follow(const lap_tree_desc *base, const lap_storage_desc *st, const int32_t *row_ws, const int32_t *src,
                     int32_t n, const lap_view_entry *views, int32_t n_views, void *stream) {
    if (!valid(base) || !st || !st->ptr || !st->size || !row_ws || !views || n_views <= 0 || n < 0) return EXO_EINVAL;
    if (n == 0) return EXO_OK;
    hipLaunchKernelGGL(lap_views_follow_kernel, dim3(base->n_strata, n_views), dim3(UPD_THREADS), 0,
                       (hipStream_t)stream, views, base->cap, levels_of(base), base->capacity, st->ptr, row_ws, src, n);
    return rc(hipGetLastError());
}

int lap_store_batch(const lap_tree_desc *t, const lap_storage_desc *st, const float *state, const float *action,
                    const float *next_state, const float *reward, const uint8_t *done, const int32_t *strata,
                    const uint8_t *active, float action_scale, int32_t n, int32_t *row_ws, void *stream) {
    const Rows in{state, action, next_state, reward, done, action_scale};
    if (!store_args_ok(t, st, in, strata, n) || !st->ptr || !row_ws) return EXO_EINVAL;
    if (n == 0) return EXO_OK;
    if (launch_store_rank(t, st, strata, active, n, row_ws, stream) != EXO_OK) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_store_copy_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *st, in, n,
                       row_ws);
    return rc(hipGetLastError());
}

int lap_store_batch_ref(const lap_tree_desc *t, const lap_storage_desc *st, int64_t *ref_dev, const float *state,
                        const float *action, const float *next_state, const float *reward, const uint8_t *done,
                        const int32_t *strata, const uint8_t *active, float action_scale, int32_t n,
                        int32_t *ws_dev, void *stream) {
    const Rows in{state, action, next_state, reward, done, action_scale};
    if (!store_args_ok(t, st, in, strata, n) || !ref_dev || !ws_dev) return EXO_EINVAL;
    if (n == 0) return EXO_OK;
    int32_t *rank_row = ws_dev, *slot_of = ws_dev + n, *row_of = ws_dev + 2 * n;
    hipLaunchKernelGGL(lap_store_ref_slots_kernel, dim3(1), dim3(UPD_THREADS), 0, (hipStream_t)stream, t->capacity,
                       t->n_strata, (long long *)ref_dev, st->size, strata, active, n, rank_row, slot_of, row_of);
    if (hipGetLastError() != hipSuccess) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_add_kernel, dim3(t->n_strata), dim3(UPD_THREADS), 0, (hipStream_t)stream, t->tree,
                       t->max_priority, t->cap, levels_of(t), t->capacity, strata, slot_of, n);
    if (hipGetLastError() != hipSuccess) return EXO_EDEVICE;
    hipLaunchKernelGGL(lap_store_copy_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *st, in, n,
                       row_of);
    return rc(hipGetLastError());
}

static int store_ref_fused(const lap_tree_desc *t, const lap_storage_desc *st, int64_t *ref_dev, const Rows &in,
                           const int32_t *strata, const uint8_t *active, int32_t n, uint32_t *ticket_dev,
                           const MaskAdvance &adv, void *stream) {
    if (!store_args_ok(t, st, in, strata, n) || !ref_dev || !ticket_dev) return EXO_EINVAL;
    if (n == 0) return EXO_OK;
    const int E = t->n_strata;
    // part 0 of a stratum: leaves + ancestors; parts 1..K-1: ~64 rows of the copy each
    const int K = 1 + std::max(1, std::min(15, (n + E * 64 - 1) / (E * 64)));
    if (rows_vec(*st, in.state, in.next_state))
        hipLaunchKernelGGL(lap_store_ref_fused_kernel<true>, dim3(E, K), dim3(UPD_THREADS), 0, (hipStream_t)stream,
                           t->tree, t->max_priority, t->cap, levels_of(t), t->capacity, E, (long long *)ref_dev,
                           st->size, *st, in, strata, active, n, ticket_dev, adv);
    else
        hipLaunchKernelGGL(lap_store_ref_fused_kernel<false>, dim3(E, K), dim3(UPD_THREADS), 0, (hipStream_t)stream,
                           t->tree, t->max_priority, t->cap, levels_of(t), t->capacity, E, (long long *)ref_dev,
                           st->size, *st, in, strata, active, n, ticket_dev, adv);
    return rc(hipGetLastError());
}

int lap_store_batch_ref_fused(const lap_tree_desc *t, const lap_storage_desc *st, int64_t *ref_dev,
                              const float *state, const float *action, const float *next_state, const float *reward,
                              const uint8_t *done, const int32_t *strata, const uint8_t *active, float action_scale,
                              int32_t n, uint32_t *ticket_dev, void *stream) {
    return store_ref_fused(t, st, ref_dev, Rows{state, action, next_state, reward, done, action_scale}, strata, active,
                           n, ticket_dev, MaskAdvance{}, stream);
}

int lap_store_batch_ref_fused_adv(const lap_tree_desc *t, const lap_storage_desc *st, int64_t *ref_dev,
                                  const float *state, const float *action, const float *next_state,
                                  const float *reward, const uint8_t *done, const int32_t *strata, uint8_t *active,
                                  float action_scale, int32_t n, uint32_t *ticket_dev, const uint8_t *table,
                                  int32_t rows, int64_t *k_dev, int32_t *count_dev, double *score_dev, void *stream) {
    if (!table || rows <= 0 || !k_dev || !active) return EXO_EINVAL;
    return store_ref_fused(t, st, ref_dev, Rows{state, action, next_state, reward, done, action_scale}, strata, active,
                           n, ticket_dev, MaskAdvance{table, rows, (long long *)k_dev, active, count_dev, score_dev},
                           stream);
}

int lap_sample_gather(const lap_tree_desc *t, const lap_storage_desc *st, const float *u, int32_t batch,
                      int32_t *idx, float *out_state, float *out_action, float *out_next_state, float *out_reward,
                      float *out_not_done, void *stream) {
    const Outs o{out_state, out_action, out_next_state, out_reward, out_not_done};
    if (!valid(t) || !st || !st->size || !u || !idx || batch <= 0 || !outs_ok(o)) return EXO_EINVAL;
    const int total = t->n_strata * batch;
    hipLaunchKernelGGL(lap_sample_gather_kernel, dim3((total + 3) / 4), dim3(256), 0, (hipStream_t)stream, t->tree,
                       t->cap, levels_of(t), t->capacity, u, st->size, batch, total, idx, *st, o,
                       SampleRng{0, 0, nullptr, nullptr});
    return rc(hipGetLastError());
}

int lap_update_sample_rng(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *idx_in,
                          const float *prio, int32_t batch, uint64_t seed, uint32_t tag, unsigned long long *counter,
                          uint32_t *ticket, int32_t *idx_out, float *out_state, float *out_action,
                          float *out_next_state, float *out_reward, float *out_not_done, void *stream) {
    const Outs o{out_state, out_action, out_next_state, out_reward, out_not_done};
    if (!valid(t) || !st || !st->size || !idx_in || !prio || !counter || !ticket || !idx_out || batch <= 0 ||
        batch > UPD_THREADS || !outs_ok(o))
        return EXO_EINVAL;
    launch_update_sample(t, st, idx_in, prio, batch, SampleRng{seed, tag, counter, ticket}, idx_out, o,
                         TdPrio{nullptr, 0.f, 0.f, nullptr}, !gather_split(), stream);
    return gather_after(t, st, batch, idx_out, o, stream);
}

int lap_update_sample_idx(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *idx_in,
                          const float *prio, int32_t batch, uint64_t seed, uint32_t tag, unsigned long long *counter,
                          uint32_t *ticket, int32_t *idx_out, void *stream) {
    if (!valid(t) || !st || !st->size || !idx_in || !prio || !counter || !ticket || !idx_out || batch <= 0 ||
        batch > UPD_THREADS)
        return EXO_EINVAL;
    launch_update_sample(t, st, idx_in, prio, batch, SampleRng{seed, tag, counter, ticket}, idx_out, Outs{},
                         TdPrio{nullptr, 0.f, 0.f, nullptr}, false, stream);
    return rc(hipGetLastError());
}

int lap_gather_rows(const lap_tree_desc *t, const lap_storage_desc *st, int32_t batch, const int32_t *idx,
                    float *out_state, float *out_action, float *out_next_state, float *out_reward,
                    float *out_not_done, void *stream) {
    const Outs o{out_state, out_action, out_next_state, out_reward, out_not_done};
    if (!valid(t) || !storage_ok(st) || !idx || batch <= 0 || !outs_ok(o)) return EXO_EINVAL;
    return launch_gather(t, st, batch, idx, o, stream);
}

int lap_update_sample_td(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *idx_in, const float *td,
                         float alpha, float min_priority, float *prio_out, int32_t batch, uint64_t seed, uint32_t tag,
                         unsigned long long *counter, uint32_t *ticket, int32_t *idx_out, float *out_state,
                         float *out_action, float *out_next_state, float *out_reward, float *out_not_done,
                         void *stream) {
    const Outs o{out_state, out_action, out_next_state, out_reward, out_not_done};
    if (!valid(t) || !st || !st->size || !idx_in || !td || !counter || !ticket || !idx_out || batch <= 0 ||
        batch > UPD_THREADS || !outs_ok(o))
        return EXO_EINVAL;
    launch_update_sample(t, st, idx_in, nullptr, batch, SampleRng{seed, tag, counter, ticket}, idx_out, o,
                         TdPrio{td, alpha, min_priority, prio_out}, !gather_split(), stream);
    return gather_after(t, st, batch, idx_out, o, stream);
}

int lap_sample_gather_rng(const lap_tree_desc *t, const lap_storage_desc *st, uint64_t seed, uint32_t tag,
                          unsigned long long *counter, uint32_t *ticket, int32_t batch, int32_t *idx,
                          float *out_state, float *out_action, float *out_next_state, float *out_reward,
                          float *out_not_done, void *stream) {
    const Outs o{out_state, out_action, out_next_state, out_reward, out_not_done};
    if (!valid(t) || !st || !st->size || !counter || !ticket || !idx || batch <= 0 || !outs_ok(o)) return EXO_EINVAL;
    const int total = t->n_strata * batch;
    hipLaunchKernelGGL(lap_sample_gather_kernel, dim3((total + 3) / 4), dim3(256), 0, (hipStream_t)stream, t->tree,
                       t->cap, levels_of(t), t->capacity, nullptr, st->size, batch, total, idx, *st, o,
                       SampleRng{seed, tag, counter, ticket});
    return rc(hipGetLastError());
}


// ---------------------------------------------------------------- planned reference inserts (C ABI)
int lap_ref_plan(const lap_tree_desc *t, const int64_t *ref_dev, const uint8_t *table_dev, int32_t rows, int32_t n,
                 const int32_t *strata_dev, const int64_t *offs_dev, int64_t total, int32_t *add_ws_dev,
                 int32_t *plan_dev, void *stream) {
    if (!valid(t) || !ref_dev || !table_dev || rows <= 0 || n <= 0 || !strata_dev || !offs_dev || total < 0 ||
        (total > 0 && !add_ws_dev) || !plan_dev)
        return EXO_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lap_ref_plan_scan_kernel, dim3(rows), dim3(UPD_THREADS), 0, s, table_dev, n, strata_dev,
                       t->n_strata, (const long long *)offs_dev, add_ws_dev, plan_dev);
    if (hipGetLastError() != hipSuccess) return EXO_EDEVICE;
    const long long entries = (long long)rows * n;
    hipLaunchKernelGGL(lap_ref_plan_slots_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, plan_dev,
                       entries, add_ws_dev, (long long)total, (const long long *)ref_dev, t->n_strata, t->capacity);
    return rc(hipGetLastError());
}

int lap_ref_step(const lap_tree_desc *t, const lap_storage_desc *st, const int32_t *plan_dev, int32_t rows,
                 int32_t n, int64_t *kk_dev, int32_t par, int64_t *k_dev, const int32_t *strata_dev,
                 const float *state, const float *action, const float *next_state, const float *reward,
                 const uint8_t *done, float action_scale, const uint8_t *table_dev, uint8_t *active_dev,
                 int32_t *count_dev, const int32_t *counts_table_dev, double *score_dev, void *stream) {
    const Rows in{state, action, next_state, reward, done, action_scale};
    if (!valid(t) || !storage_ok(st) || !plan_dev || rows <= 0 || n <= 0 || !kk_dev || (par != 0 && par != 1) ||
        !strata_dev || !rows_ok(in) || !table_dev || !active_dev || (count_dev && !counts_table_dev))
        return EXO_EINVAL;
    hipLaunchKernelGGL(lap_ref_step_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, *st, plan_dev,
                       rows, n, (long long *)kk_dev, par, (long long *)k_dev, strata_dev, t->capacity, in, table_dev,
                       active_dev, count_dev, counts_table_dev, score_dev);
    return rc(hipGetLastError());
}

int lap_ref_commit(const lap_tree_desc *t, const lap_storage_desc *st, int64_t *ref_dev, const int32_t *plan_dev,
                   int32_t rows, int32_t n, const int32_t *strata_dev, int64_t total, void *stream) {
    if (!valid(t) || !st || !st->size || !ref_dev || !plan_dev || rows <= 0 || n <= 0 || !strata_dev || total < 0)
        return EXO_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long entries = (long long)rows * n;
    hipLaunchKernelGGL(lap_ref_commit_leaves_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s,
                       plan_dev, entries, n, strata_dev, t->tree, t->cap, t->max_priority);
    hipLaunchKernelGGL(lap_ref_commit_tree_kernel, dim3(t->n_strata), dim3(UPD_THREADS), 0, s, t->tree, t->cap,
                       levels_of(t), t->capacity, (const long long *)ref_dev, (long long)total, t->n_strata);
    hipLaunchKernelGGL(lap_ref_commit_ref_kernel, dim3(1), dim3(1), 0, s, (long long *)ref_dev, (long long)total,
                       t->n_strata, t->capacity, st->size);
    return rc(hipGetLastError());
}

} // extern "C"
