"""csrc/td7_xcd_map.h on the host: the workgroup order td7f::wgrad_kernel takes
its tiles in.  For every grid size the map must be a permutation (every tile
computed exactly once) and the workgroups of one XCD (equal b % 8) must take
one contiguous range of the tile order."""
import ctypes
import os
import subprocess

import numpy as np

from helpers import PKG, REPO

SO = os.path.join(REPO, "tests", "native", "_build", "libxcd_map_host.so")


def _lib():
    src = os.path.join(REPO, "tests", "native", "xcd_map_host.cpp")
    hdr = os.path.join(PKG, "csrc", "td7_xcd_map.h")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(PKG, "csrc"), "-o", SO, src],
                       check=True)
    L = ctypes.CDLL(SO)
    L.xm_map.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return L


def _map(L, total):
    out = np.empty(total, dtype=np.int32)
    L.xm_map(total, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return out


def test_map_is_a_permutation_for_every_total():
    L = _lib()
    for total in range(1, 601):
        m = _map(L, total)
        assert np.array_equal(np.sort(m), np.arange(total)), total


def test_each_xcd_takes_one_contiguous_range():
    L = _lib()
    nx = L.xm_num_xcd()
    assert nx == 8
    for total in range(1, 601):
        m = _map(L, total)
        start = 0
        for x in range(nx):
            mine = m[x::nx]  # workgroups x, x + 8, ...: in dispatch order
            # consecutive tiles, ascending with the dispatch order, the ranges
            # of XCD 0, 1, ... following each other
            assert np.array_equal(mine, np.arange(start, start + len(mine))), (total, x)
            start += len(mine)
        assert start == total


def test_bench_totals_are_covered():
    """The bench's launches (actor 90, encoder 135, critic 230 tiles): no
    multiple of 8, the first total % 8 XCDs take one tile more."""
    L = _lib()
    for total in (5, 90, 135, 230):
        m = _map(L, total)
        sizes = [len(m[x::8]) for x in range(8)]
        assert sizes == [total // 8 + (1 if x < total % 8 else 0) for x in range(8)]
