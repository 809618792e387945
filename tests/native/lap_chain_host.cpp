// Host build of csrc/lap_chain.h for tests/test_lap_chain_host.py: the update
// of lap_update_sample_chain_kernel (csrc/lap.hip) replayed on the CPU in the
// kernel's order -- every load the kernel issues before its first store reads
// the tree as it was before the update.
#include <cmath>
#include <cstdint>
#include <vector>

#include "lap_chain.h"

extern "C" {

int lc_global_levels(int levels, int ntop) { return lap_chain::global_levels(levels, ntop); }
int lc_partner_level(int me, int other) { return lap_chain::partner_level(me, other); }

// One stratum's update.  T: the 2 cap nodes, updated in place; idx, prio: the
// n draws.  poison != 0: a preloaded sibling or prefix addend that a partner's
// chain value must replace is NaN instead of the stale tree value.  low_out:
// the G prefix addends below the staged top for sampling size sz (level 0
// first), as the kernel's draws read them.  Returns G.
int lc_update(float *T, int levels, int ntop, const int32_t *idx, const float *prio, int n, int sz, int poison,
              float *low_out) {
    const int cap = 1 << levels;
    const int G = lap_chain::global_levels(levels, ntop);
    const int lim = ntop < 2 * cap ? ntop : 2 * cap;
    const int rows = n + 1;  // the draws and leaf sz
    const int szl = sz < cap - 1 ? sz : cap - 1;
    std::vector<int32_t> li(idx, idx + n);
    li.push_back(szl);
    // trip 1: the staged top
    std::vector<float> top(T, T + lim);
    // trip 2: the siblings
    std::vector<float> sib((size_t)(G > 0 ? G : 1) * rows);
    for (int lv = 0; lv < G; ++lv)
        for (int b = 0; b < rows; ++b) sib[(size_t)lv * rows + b] = T[lap_chain::sibling_of(cap, li[b], lv)];
    // superseded duplicates and partners (the highest draw below each sibling)
    std::vector<char> later(n, 0);
    std::vector<int32_t> partner((size_t)(G > 0 ? G : 1) * rows, -1);
    for (int b = 0; b < rows; ++b)
        for (int k = 0; k < n; ++k) {
            const int lv = lap_chain::partner_level(li[b], li[k]);
            if (b < n && lap_chain::superseded_by(b, li[b], k, li[k])) later[b] = 1;
            else if (lv >= 0 && lv < G && k > partner[(size_t)lv * rows + b]) partner[(size_t)lv * rows + b] = k;
        }
    if (poison)
        for (int lv = 0; lv < G; ++lv)
            for (int b = 0; b < rows; ++b)
                if (partner[(size_t)lv * rows + b] >= 0) sib[(size_t)lv * rows + b] = NAN;
    // leaves, then the chain, one level at a time
    std::vector<float> cur(n, 0.0f), nxt(n, 0.0f), low(G > 0 ? G : 1, 0.0f);
    for (int b = 0; b < n; ++b)
        if (!later[b]) T[cap + li[b]] = cur[b] = prio[b];
    for (int lv = 0; lv < G; ++lv) {
        const int ks = partner[(size_t)lv * rows + n];
        low[lv] = ks >= 0 ? cur[ks] : sib[(size_t)lv * rows + n];
        for (int b = 0; b < n; ++b) {
            if (later[b]) continue;
            const int node = lap_chain::node_of(cap, li[b], lv), k = partner[(size_t)lv * rows + b];
            nxt[b] = lap_chain::chain_step(node, cur[b], k >= 0 ? cur[k] : sib[(size_t)lv * rows + b]);
            T[node >> 1] = nxt[b];
        }
        cur.swap(nxt);
    }
    for (int lv = 0; lv < G; ++lv) low_out[lv] = low[lv];
    // the level-G values patch the staged top; the remaining levels there
    for (int b = 0; b < n; ++b)
        if (!later[b]) top[lap_chain::node_of(cap, li[b], G)] = cur[b];
    for (int lv = G + 1; lv <= levels; ++lv)
        for (int b = 0; b < n; ++b) {
            const int node = lap_chain::node_of(cap, li[b], lv);
            top[node] = top[2 * node] + top[2 * node + 1];
        }
    const int wb = ntop / 2 < cap ? ntop / 2 : cap;
    for (int i = 1; i < wb; ++i) T[i] = top[i];
    return G;
}
}
