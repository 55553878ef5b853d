// What the molecule kernels share (molecule.hip: perception and SDF text; molset.hip: keys, fingerprints, diversity): the size
// limits of one ligand, the status bits of kpd_mol_perceive and the segment check.
#pragma once
#include "common.h"

namespace kpd {

constexpr int MOL_MAX = 256;            // atoms of one ligand
constexpr int MOL_W = MOL_MAX / 32;     // words of one row of a bit matrix
constexpr int MOL_K = MOL_MAX / 64;     // atoms per lane

enum : int { MOL_EMPTY = 1, MOL_CAPACITY = 2, MOL_BAD_ATOM = 4, MOL_BAD_SEGMENT = 8 };

__device__ __forceinline__ bool mol_segment(const int *__restrict__ ptr, int b, int n, int &a0, int &a1) {
    a0 = ptr[b];
    a1 = ptr[b + 1];
    return a0 >= 0 && a1 >= a0 && a1 <= n;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

}  // namespace kpd
