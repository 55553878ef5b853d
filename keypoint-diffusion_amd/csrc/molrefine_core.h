// The atom invariant of kpd_mol_keys (include/kpd.h: inv_0 .. inv_n), stated once for k_mol_keys (molset.hip), k_smiles_build
// (smiles.hip) and k_pose_rmsd (pose_rmsd.hip): the splitmix64 finaliser, the three constants, the distance term of the seed (a BFS
// from one source atom over bitset frontiers, a lane per source), one refinement step and the double-buffered loop of n of them.
// Each kernel adds its own atom term to the seed: keys Z + deg K3, smiles also hl K2, pose_rmsd A(a) for Z.  Also here, for the two
// kernels that order atoms by the invariant: the rank "atoms of S with a smaller value" and the sort of a neighbour row.
// k_pose_rmsd has the loop of n steps (mr_refine_steps) written out around mr_refine: the call cost it time, profiles/molrefine_core.md.
// Everything is __device__ __forceinline__ and takes plain pointers, as molgraph_core.h does: an LDS array stays in its address
// space after inlining, and the __shared__ declarations stay in the kernels' files.  Integer arithmetic modulo 2^64 only.
#pragma once
#include "molgraph_core.h"

namespace kpd {

typedef unsigned long long u64;

constexpr u64 MR_K1 = 0x9E3779B97F4A7C15ull, MR_K2 = 0xC2B2AE3D27D4EB4Full, MR_K3 = 0x165667B19E3779F9ull;
constexpr int MR_ROW = MOL_W + 1;       // padded adjacency row: in the BFS every lane walks rows of its own
constexpr int MR_FAR = 65535;           // d(a, b) of an atom that cannot be reached

__device__ __forceinline__ u64 mr_mix(u64 x) {            // the splitmix64 finaliser
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// one refinement step of atom a: mix(K1 x[a] + sum over its bonds of mix(x[b] + l K2)); a neighbour entry is b | l << 8
__device__ __forceinline__ u64 mr_refine(const u64 *x, const unsigned short *nb, int deg, int a) {
    u64 s = MR_K1 * x[a];
    for (int k = 0; k < deg; ++k) {
        const unsigned e = nb[a * MOL_DEG + k];
        s += mr_mix(x[e & 0xffu] + (u64)(e >> 8) * MR_K2);
    }
    return mr_mix(s);
}

// the distance term of the seed of atom a: sum over b in S, b != a, of mix(zk[b] + d(a,b)).  adj: the bit matrix of the bonds
// inside S (MR_ROW words per row), zk[b] = (the atom's label) K2, inS: the MOL_W words of the scope.
__device__ __forceinline__ u64 mr_seed_sum(const unsigned *adj, const u64 *zk, const unsigned *inS, int a) {
    unsigned seen[MOL_W], front[MOL_W], next[MOL_W];
#pragma unroll
    for (int w = 0; w < MOL_W; ++w) seen[w] = front[w] = (w == (a >> 5)) ? 1u << (a & 31) : 0u;
    u64 sum = 0;
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
                sum += mr_mix(zk[32 * w + __ffs(bits) - 1] + (u64)d);
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
            sum += mr_mix(zk[32 * w + __ffs(bits) - 1] + (u64)MR_FAR);
            bits &= bits - 1;
        }
    }
    return sum;
}

// `steps` refinement steps over x [2][MOL_MAX], from the buffer cur: lane takes the atoms lane + 64 k that are in S (in[k], degree
// dg[k]), a barrier per step.  Returns the buffer that holds the result.
__device__ __forceinline__ int mr_refine_steps(u64 *x, const unsigned short *nb, const bool (&in)[MOL_K], const int (&dg)[MOL_K], int lane,
                                               int cur, int steps) {
    for (int r = 0; r < steps; ++r) {
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (in[k]) x[(cur ^ 1) * MOL_MAX + a] = mr_refine(x + cur * MOL_MAX, nb, dg[k], a);
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// less[k]: how many atoms of S have a smaller value than the atom lane + 64 k (0 outside S).  INDEX_BREAKS_TIES: of two equal
// values the one of the lower atom counts as smaller, so the ranks are a permutation; without it equal values share a rank.
template <bool INDEX_BREAKS_TIES>
__device__ __forceinline__ void mr_rank(const u64 *x, const unsigned *inS, const bool (&in)[MOL_K], int n, int lane, int (&less)[MOL_K]) {
    u64 xa[MOL_K];
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        xa[k] = in[k] ? x[lane + 64 * k] : 0;
        less[k] = 0;
    }
    for (int c = 0; c < n; ++c) {
        if (!in_scope(inS, c)) continue;            // wave-uniform
        const u64 xc = x[c];
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) less[k] += xc < xa[k] || (INDEX_BREAKS_TIES && xc == xa[k] && c < lane + 64 * k);
    }
}

// the `deg` entries of one neighbour row in ascending key(entry): an insertion sort, equal keys keep their order
template <class Key>
__device__ __forceinline__ void mr_sort_row(unsigned short *row, int deg, Key key) {
    for (int s = 1; s < deg; ++s) {
        const unsigned short e = row[s];
        int t = s;
        for (; t > 0 && key(row[t - 1]) > key(e); --t) row[t] = row[t - 1];
        row[t] = e;
    }
}

}  // namespace kpd
