// The atom invariant of kpd_mol_keys (include/kpd.h: inv_0 .. inv_n) as device functions: the splitmix64 finaliser, the three
// constants, the distance term of the seed (a BFS from one source atom over bitset frontiers, a lane per source) and one
// refinement step.  k_pose_rmsd (pose_rmsd.hip) takes them from here.  k_mol_keys (molset.hip) and k_smiles_build (smiles.hip)
// carry the same text written out, from before this header; they are left as they are, object code included, and can move here
// in a change of their own.  Everything is __device__ __forceinline__ and takes plain pointers, as molgraph_core.h does: an LDS
// array stays in its address space after inlining.  Integer arithmetic modulo 2^64 only.
#pragma once
#include "molgraph_core.h"

namespace kpd {

typedef unsigned long long mr_u64;

constexpr mr_u64 MR_K1 = 0x9E3779B97F4A7C15ull, MR_K2 = 0xC2B2AE3D27D4EB4Full, MR_K3 = 0x165667B19E3779F9ull;
constexpr int MR_ROW = MOL_W + 1;       // padded adjacency row: in the BFS every lane walks rows of its own
constexpr int MR_FAR = 65535;           // d(a, b) of an atom that cannot be reached

__device__ __forceinline__ mr_u64 mr_mix(mr_u64 x) {            // the splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// one refinement step of atom a: mix(K1 x[a] + sum over its bonds of mix(x[b] + l K2)); a neighbour entry is b | l << 8
__device__ __forceinline__ mr_u64 mr_refine(const mr_u64 *x, const unsigned short *nb, int deg, int a) {
    mr_u64 s = MR_K1 * x[a];
    for (int k = 0; k < deg; ++k) {
        const unsigned e = nb[a * MOL_DEG + k];
        s += mr_mix(x[e & 0xffu] + (mr_u64)(e >> 8) * MR_K2);
    }
    return mr_mix(s);
}

// the distance term of the seed of atom a: sum over b in S, b != a, of mix(zk[b] + d(a,b)).  adj: the bit matrix of the bonds
// inside S (MR_ROW words per row), zk[b] = (the atom's label) K2, inS: the MOL_W words of the scope.
__device__ __forceinline__ mr_u64 mr_seed_sum(const unsigned *adj, const mr_u64 *zk, const unsigned *inS, int a) {
    unsigned seen[MOL_W], front[MOL_W], next[MOL_W];
#pragma unroll
    for (int w = 0; w < MOL_W; ++w) seen[w] = front[w] = (w == (a >> 5)) ? 1u << (a & 31) : 0u;
    mr_u64 sum = 0;
    for (int d = 1;; ++d) {
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) next[w] = 0;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            unsigned bits = front[w];
            while (bits) {
                const int j = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1;
#pragma unroll
                for (int v = 0; v < MOL_W; ++v) next[v] |= adj[j * MR_ROW + v];
            }
        }
        unsigned any = 0;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            next[w] &= ~seen[w];
            any |= next[w];
        }
        if (!any) break;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            unsigned bits = next[w];
            while (bits) {
                sum += mr_mix(zk[32 * w + __ffs(bits) - 1] + (mr_u64)d);
                bits &= bits - 1;
            }
            seen[w] |= next[w];
            front[w] = next[w];
        }
    }
#pragma unroll
    for (int w = 0; w < MOL_W; ++w) {
        unsigned bits = inS[w] & ~seen[w];
        while (bits) {
            sum += mr_mix(zk[32 * w + __ffs(bits) - 1] + (mr_u64)MR_FAR);
            bits &= bits - 1;
        }
    }
    return sum;
}

}  // namespace kpd
