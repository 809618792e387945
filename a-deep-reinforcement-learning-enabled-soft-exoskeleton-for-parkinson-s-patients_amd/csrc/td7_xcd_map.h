// XCD-contiguous order of a 1-D grid's workgroups (device and host).
//
// The hardware deals consecutive workgroups round-robin over the 8 XCDs, each
// with its own L2.  xcd_contiguous(b, total) sends workgroup b of a grid of
// `total` to a work item such that the workgroups with equal b % 8 (one XCD)
// take one contiguous range of 0 .. total-1: neighbours in the work order,
// which share operand panels, then meet in one L2.  The map is a bijection
// for every total >= 1 (total < 8 and total % 8 != 0 included); placement is a
// speed assumption only, nothing may depend on it for correctness.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EXO_XCD_HD __host__ __device__ __forceinline__
#else
#define EXO_XCD_HD inline
#endif

constexpr int EXO_NUM_XCD = 8;

EXO_XCD_HD int xcd_contiguous(int b, int total) {
    const int q = total / EXO_NUM_XCD, r = total % EXO_NUM_XCD, x = b % EXO_NUM_XCD;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / EXO_NUM_XCD;
}
