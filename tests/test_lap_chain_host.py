"""csrc/lap_chain.h on the host: lap_update_sample's sibling chain replayed on the
CPU (tests/native/lap_chain_host.cpp) against a level-synchronous numpy float32
recomputation -- leaves (last duplicate wins), then level by level every
touched node once, T[n] = T[2n] + T[2n + 1].  Every node of the tree and the
prefix walk's addends below the staged top must match bit for bit, also when
every preloaded value a partner's chain value must replace is NaN."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import PKG, REPO
from lap_chain_cases import NTOP, global_levels, pattern, pattern_names

SO = os.path.join(REPO, "tests", "native", "_build", "liblap_chain_host.so")
F32P, I32P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


def _lib():
    src = os.path.join(REPO, "tests", "native", "lap_chain_host.cpp")
    hdr = os.path.join(PKG, "csrc", "lap_chain.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(PKG, "csrc"), "-o", SO, src],
                       check=True)
    L = ctypes.CDLL(SO)
    L.lc_update.argtypes = [F32P, ctypes.c_int, ctypes.c_int, I32P, F32P, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                            F32P]
    return L


def _tree(prio):
    """The stratum tree of float32 leaves `prio` (cap of them)."""
    cap = prio.shape[0]
    T = np.zeros(2 * cap, dtype=np.float32)
    T[cap:] = prio
    n = cap
    while n > 1:
        T[n // 2:n] = T[n:2 * n:2] + T[n + 1:2 * n:2]
        n //= 2
    return T


def _reference(T, idx, p):
    cap = T.shape[0] // 2
    T = T.copy()
    for b in range(idx.shape[0]):  # the last duplicate wins
        T[cap + idx[b]] = p[b]
    nodes = np.unique(cap + idx.astype(np.int64))
    while nodes[0] > 1:
        nodes = np.unique(nodes >> 1)
        T[nodes] = T[2 * nodes] + T[2 * nodes + 1]
    return T


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_global_levels_and_partner_level():
    L = _lib()
    for levels in range(0, 25):
        assert L.lc_global_levels(levels, NTOP) == max(0, levels - 12) == global_levels(1 << levels)
    rng = np.random.default_rng(3)
    for me, other in rng.integers(0, 1 << 24, (2000, 2)):
        lv = L.lc_partner_level(int(me), int(other))
        if me == other:
            assert lv == -1
        else:  # other lies below the sibling of me's level-lv ancestor, and at no other level
            assert [q for q in range(25) if (int(other) >> q) == ((int(me) >> q) ^ 1)] == [lv]
    assert L.lc_partner_level(5, 5) == -1 and L.lc_partner_level(4, 5) == 0 and L.lc_partner_level(0, 1 << 17) == 17


@pytest.mark.parametrize("cap", [1 << 13, 1 << 14, 1 << 18])
def test_chain_equals_the_level_synchronous_update(cap):
    L = _lib()
    levels = cap.bit_length() - 1
    G = global_levels(cap)
    rng = np.random.default_rng(cap)
    prio = (rng.gamma(0.7, 2.0, cap) + 1e-3).astype(np.float32)
    T0 = _tree(prio)
    low = np.zeros(max(G, 1), dtype=np.float32)
    for B in (1, 2, 16, 128, 256):
        for size in (cap, cap - 3, cap // 2 + 77, 65):
            for name in pattern_names(cap):
                for poison in (0, 1):
                    T, want = T0.copy(), T0
                    prng = np.random.default_rng([cap, B, size])
                    for call in range(4):  # consecutive updates: the tree evolves
                        idx = pattern(name, prng, B, size)
                        p = prng.uniform(0.1, 9.0, B).astype(np.float32)
                        want = _reference(want, idx, p)
                        g = L.lc_update(T.ctypes.data_as(F32P), levels, NTOP, idx.ctypes.data_as(I32P),
                                        p.ctypes.data_as(F32P), B, size, poison, low.ctypes.data_as(F32P))
                        assert g == G
                        tag = (cap, B, size, name, poison, call)
                        assert _same_bits(T, want), tag
                        if size < cap:  # the prefix walk's addends: the siblings of leaf `size`'s ancestors
                            sib = np.array([want[((cap + size) >> lv) ^ 1] for lv in range(G)], dtype=np.float32)
                            assert _same_bits(low[:G], sib), tag


def test_reference_keeps_every_node_the_sum_of_its_children():
    """The numpy reference itself: after its update every internal node is
    exactly left + right (the tree's invariant)."""
    cap = 1 << 14
    rng = np.random.default_rng(1)
    T = _tree((rng.gamma(0.7, 2.0, cap) + 1e-3).astype(np.float32))
    idx = pattern("dups", rng, 128, cap)
    T = _reference(T, idx, rng.uniform(0.1, 9.0, 128).astype(np.float32))
    assert _same_bits(T[1:cap], T[2:2 * cap:2] + T[3:2 * cap:2])
