// What the molecule kernels share (molecule.hip: perception and SDF text; molset.hip: keys, fingerprints, diversity): the size
// limits of one ligand, the element table, the status bits of kpd_mol_perceive and the segment check.
// relax.hip reads the same table for its rest lengths; vina.hip types pocket atoms by the same distance recipe and step-1 / step-3 tests.
#pragma once
#include "common.h"

namespace kpd {

constexpr int MOL_MAX = 256;            // atoms of one ligand
constexpr int MOL_W = MOL_MAX / 32;     // words of one row of a bit matrix
constexpr int MOL_K = MOL_MAX / 64;     // atoms per lane

enum : int { MOL_EMPTY = 1, MOL_CAPACITY = 2, MOL_BAD_ATOM = 4, MOL_BAD_SEGMENT = 8 };

// the element table: r1 | r2 << 8 | r3 << 16 | cap << 24 (covalent radii after Pyykko & Atsumi 2009 in pm, 0 = no bond of that
// order; cap = chemical valence cap); 0 for every other atomic number
__device__ __forceinline__ unsigned element_row(int z) {
#define KPD_EL(r1, r2, r3, cap) ((unsigned)(r1) | (unsigned)(r2) << 8 | (unsigned)(r3) << 16 | (unsigned)(cap) << 24)
    switch (z) {
    case 1: return KPD_EL(32, 0, 0, 1);         // H
    case 5: return KPD_EL(85, 78, 0, 3);        // B
    case 6: return KPD_EL(75, 67, 60, 4);       // C
    case 7: return KPD_EL(71, 60, 54, 3);       // N
    case 8: return KPD_EL(63, 57, 0, 2);        // O
    case 9: return KPD_EL(64, 0, 0, 1);         // F
    case 14: return KPD_EL(116, 0, 0, 4);       // Si
    case 15: return KPD_EL(111, 102, 0, 5);     // P
    case 16: return KPD_EL(103, 94, 0, 6);      // S
    case 17: return KPD_EL(99, 0, 0, 1);        // Cl
    case 33: return KPD_EL(121, 0, 0, 3);       // As
    case 35: return KPD_EL(114, 0, 0, 1);       // Br
    case 53: return KPD_EL(133, 0, 0, 1);       // I
    default: return 0u;
    }
#undef KPD_EL
}

// fp64 sum of squares of the exact differences; every product and sum is rounded on its own (no fused multiply-add)
__device__ __forceinline__ double sum_sq(double dx, double dy, double dz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
__device__ __forceinline__ double mol_d2(const float *p, int i, int j) {
    return sum_sq((double)p[i * 3] - (double)p[j * 3], (double)p[i * 3 + 1] - (double)p[j * 3 + 1],
                  (double)p[i * 3 + 2] - (double)p[j * 3 + 2]);
}

// d2 <= ((r_k(i) + r_k(j) + margin) pm)^2; false if either radius is 0
__device__ __forceinline__ bool within(double d2, unsigned ri, unsigned rj, int margin) {
    if (!ri || !rj) return false;
    const int T = (int)ri + (int)rj + margin;
    return d2 <= (double)(T * T) * 1e-4;
}

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
