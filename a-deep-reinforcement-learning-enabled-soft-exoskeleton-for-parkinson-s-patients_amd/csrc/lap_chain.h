// lap_chain.h -- the index logic of lap_update_sample's sibling chain
// (csrc/lap.hip, lap_update_sample_chain_kernel), host-compilable: the same
// functions run in the kernel and in tests/native/lap_chain_host.cpp.
//
// A stratum tree over cap = 2^levels leaves keeps its nodes [1, ntop) in LDS
// during the update; the G levels below them are "global".  The level-
// synchronous update recomputes, level by level, T[n] = T[2n] + T[2n + 1] for
// every ancestor n of an updated leaf, one dependent memory round trip per
// level.  The chain computes the same sums from values it already holds:
//   * draw b (leaf slot me) carries the new value of its own ancestor at
//     level lv, chain[lv][b] (chain[0][b] = the new priority);
//   * the other child of the next ancestor is the SIBLING node_of(me, lv) ^ 1.
//     Its value is chain[lv][k] if some draw k updates a leaf below it, else
//     the tree's value, which this launch does not change and which was
//     therefore loaded -- for all G levels at once -- before anything else;
//   * slot o lies below the sibling of me's level-lv ancestor exactly when
//     the highest set bit of (me ^ o) is bit lv: every other draw is a partner
//     at one level (partner_level) or none;
//   * of several draws below one sibling any one serves (they hold the same
//     bits), provided it carries a value: a draw superseded by a later
//     duplicate of its slot (last duplicate wins) does not.  The partner is
//     the HIGHEST such draw, which no later duplicate can follow;
//   * left and right follow the node's low bit (chain_step), so every sum is
//     the level-synchronous T[2n] + T[2n + 1] with the same operands: the
//     same bits.
#pragma once

#if defined(__HIPCC__)
#define LAP_CHAIN_HD __host__ __device__ __forceinline__
#else
#define LAP_CHAIN_HD inline
#endif

namespace lap_chain {

// The number of levels lv in [1, levels] whose nodes lie outside the staged
// top: (2 cap >> lv) > ntop / 2 (propagate_top's first loop).
LAP_CHAIN_HD int global_levels(int levels, int ntop) {
    int g = 0;
    for (int lv = 1; lv <= levels; ++lv)
        if (((2ll << levels) >> lv) > ntop / 2) ++g;
    return g;
}

// The ancestor of leaf `slot` at level lv (0: the leaf itself) and its sibling.
LAP_CHAIN_HD int node_of(int cap, int slot, int lv) { return (cap + slot) >> lv; }
LAP_CHAIN_HD int sibling_of(int cap, int slot, int lv) { return node_of(cap, slot, lv) ^ 1; }

// The level at which slot `other` lies below the sibling of `me`'s ancestor:
// node_of(other, lv) == sibling_of(me, lv)  <=>  (me ^ other) >> lv == 1.
// -1: the same slot.
LAP_CHAIN_HD int partner_level(int me, int other) {
    const unsigned d = (unsigned)(me ^ other);
    return d ? 31 - __builtin_clz(d) : -1;
}

// Draw b (slot me) is superseded by draw k (slot other): a later duplicate.
LAP_CHAIN_HD bool superseded_by(int b, int me, int k, int other) { return k > b && other == me; }

// The parent of `node` from its own value and its sibling's: left + right.
LAP_CHAIN_HD float chain_step(int node, float mine, float sibling) {
    return (node & 1) ? sibling + mine : mine + sibling;
}

}  // namespace lap_chain
