// What the molecule kernels share (molecule.hip: perception and SDF text; molset.hip: keys, fingerprints, diversity): the size
// limits of one ligand, the element table, the status bits of kpd_mol_perceive, the segment and bond-range checks.
// relax.hip reads the same table for its rest lengths; vina.hip types pocket atoms by the same distance recipe and step-1 / step-3 tests.
// relax.hip and vina.hip also share everything that means "one workgroup takes one perceived ligand and its pocket" (the second
// half of this file): the device front end with status bits 0 and 1, the two-vote epilogue of the staging loops, the LDS carving,
// and on the host the argument check and the number of staged pocket rows.  pocket.hip takes the segment check alone.
// vina_min.hip takes the same front end; what vina.hip and vina_min.hip share beyond it (typing, pair terms, staging, bond graph,
// graph walk) is in vina_core.h.  The wave butterflies (wave_sum, the fp64 wave_max) serve relax.hip and both of them.
// molset.hip, sanitize.hip and hydrogens.hip share "one wave takes one perceived ligand and builds its graph in the scope S"
// through molgraph_core.h, which stands on this file; the int wave_max, the 64-bit wave_sum and wave_exclusive serve them and molecule.hip,
// the two wave minima smiles.hip.
#pragma once
#include <algorithm>

#include "common.h"

namespace kpd {

constexpr int MOL_MAX = 256;            // atoms of one ligand
constexpr int MOL_W = MOL_MAX / 32;     // words of one row of a bit matrix
constexpr int MOL_K = MOL_MAX / 64;     // atoms per lane
constexpr int MOL_DEG = 6;              // neighbours of one atom: the largest valence cap of the bond rule

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

// rows [a0, a1) of entry b, or false if the segment table is malformed (nothing of that entry is then touched)
__device__ __forceinline__ bool mol_segment(const int *__restrict__ ptr, int b, int n, int &a0, int &a1) {
    a0 = ptr[b];
    a1 = ptr[b + 1];
    return a0 >= 0 && a1 >= a0 && a1 <= n;
}

// bonds [p0, p1) of ligand b, or false if the range is malformed, ends beyond cap_bonds or holds more bonds than MOL_MAX atoms can have
__device__ __forceinline__ bool mol_bond_range(const int *__restrict__ bond_ptr, int b, int cap_bonds, int &p0, int &p1) {
    p0 = bond_ptr[b];
    p1 = bond_ptr[b + 1];
    return p0 >= 0 && p1 >= p0 && p1 <= cap_bonds && p1 - p0 <= 3 * MOL_MAX;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {      // modulo 2^64
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) { return -wave_max(-v); }
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long t = __shfl_xor(v, off);
        v = t < v ? t : v;
    }
    return v;
}
// exclusive prefix of v over the lanes of the wave; total = the wave's sum
__device__ __forceinline__ int wave_exclusive(int v, int lane, int &total) {
    int s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(s, off);
        if (lane >= off) s += t;
    }
    total = __shfl(s, 63);
    return s - v;
}
__device__ __forceinline__ double wave_sum(double v) {      // a butterfly: the same bits on every lane
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {      // a maximum has no order
#pragma unroll
    for (int off = 32; off; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }      // false for NaN too

// ---- steps 5 and 6 of kpd_mol_perceive, for a wave that holds a ligand's bond graph as bit matrices (k_mol_perceive; k_sdf_records
// of structure_io.hip, whose bonds come from a file) ----------------------------------------------------------------------------------
// A1 / A2 / A3 [n x MOL_W words]: bonded / order >= 2 / order >= 3, symmetric; label, fsize [MOL_MAX]: LDS scratch.
// Writes valence and frag of the atoms a0 .. a0 + n - 1 and, unless ij_dst is null, the bonds in (i, j) order (global rows) to
// ij_dst / order_dst.  invalid_atom(k, valence) is step 6 for the lane's k-th atom.  Out, on every lane: fragments, atoms of the
// largest one, invalid atoms, bonds.
template <class Invalid>
__device__ __forceinline__ void mol_fragments_out(const unsigned *A1, const unsigned *A2, const unsigned *A3, int *label, int *fsize, int n,
                                                  int lane, int a0, Invalid invalid_atom, int *__restrict__ valence, int *__restrict__ frag,
                                                  int *__restrict__ ij_dst, int *__restrict__ order_dst, int &n_frags, int &largest,
                                                  int &invalid, int &total) {
    // step 5: fragments by label propagation (the fixed point is the lowest atom of every component)
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        label[lane + 64 * k] = lane + 64 * k;
        fsize[lane + 64 * k] = 0;
    }
    __syncthreads();
    for (;;) {
        bool changed = false;
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int i = lane + 64 * k;
            if (i >= n) continue;
            int l = label[i];
            const int before = l;
            for (int w = 0; w < MOL_W; ++w) {
                unsigned bits = A1[i * MOL_W + w];
                while (bits) {
                    l = min(l, label[32 * w + __ffs(bits) - 1]);
                    bits &= bits - 1;
                }
            }
            l = min(l, label[l]);                   // pointer jump
            if (l != before) {
                label[i] = l;
                changed = true;
            }
        }
        __syncthreads();
        if (!__any(changed)) break;                 // wave-uniform
    }
    unsigned long long roots[MOL_K];
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int i = lane + 64 * k;
        roots[k] = __ballot(i < n && label[i] == i);
        if (i < n) atomicAdd(&fsize[label[i]], 1);
    }
    __syncthreads();
    n_frags = 0;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) n_frags += __popcll(roots[k]);
    // largest fragment: most atoms, then the lowest rank (= the lowest root)
    int best = 0;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int i = lane + 64 * k;
        if (i < n && label[i] == i) best = max(best, fsize[i] * (MOL_MAX + 1) + (MOL_MAX - i));
    }
    largest = wave_max(best) / (MOL_MAX + 1);
    // per-atom outputs, step 6
    int mine[MOL_K];
    invalid = 0;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int i = lane + 64 * k;
        mine[k] = 0;
        if (i < n) {
            int val = 0;
            for (int w = 0; w < MOL_W; ++w) {
                val += __popc(A1[i * MOL_W + w]) + __popc(A2[i * MOL_W + w]) + __popc(A3[i * MOL_W + w]);
                unsigned up = A1[i * MOL_W + w];
                if (32 * w + 31 <= i) up = 0;
                else if (32 * w <= i) up &= ~((2u << (i & 31)) - 1u);
                mine[k] += __popc(up);
            }
            const int root = label[i];
            int rank = 0;
#pragma unroll
            for (int q = 0; q < MOL_K; ++q) {
                const int below = root - 64 * q;    // roots of chunk q below `root`
                if (below >= 64) rank += __popcll(roots[q]);
                else if (below > 0) rank += __popcll(roots[q] & ((1ull << below) - 1ull));
            }
            valence[a0 + i] = val;
            frag[a0 + i] = rank;
            invalid += invalid_atom(k, val) ? 1 : 0;
        }
    }
    invalid = wave_sum(invalid);
    // bonds in (i, j) order
    int base = 0;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        int chunk;
        int at = base + wave_exclusive(mine[k], lane, chunk);
        base += chunk;
        const int i = lane + 64 * k;
        if (i >= n || !ij_dst) continue;
        for (int w = i >> 5; w < MOL_W; ++w) {
            unsigned bits = A1[i * MOL_W + w];
            if (32 * w <= i) bits &= (i & 31) == 31 ? 0u : ~((2u << (i & 31)) - 1u);
            while (bits) {
                const int t = __ffs(bits) - 1, j = 32 * w + t;
                bits &= bits - 1;
                const size_t r = (size_t)at++;
                ij_dst[r * 2] = a0 + i;
                ij_dst[r * 2 + 1] = a0 + j;
                order_dst[r] = 1 + (int)((A2[i * MOL_W + w] >> t) & 1u) + (int)((A3[i * MOL_W + w] >> t) & 1u);
            }
        }
    }
    total = base;
}

// ---- one workgroup takes one perceived ligand and its pocket (kpd_relax, kpd_vina_score, kpd_vina_minimize) ---------------------------------
enum : int { LP_NO_MOLECULE = 1, LP_BAD_INPUT = 2 };     // bits 0 and 1 of both status words

// the ligand's n atoms [a0, a1) (to be used only where seg: lig_ptr was well-formed), its bonds [p0, p1), the np atoms of its pocket from q0
struct LigandInPocket {
    int a0, a1, n, p0, p1, q0, np;
    bool seg;
};

// Fills s for ligand b; returns 0, LP_NO_MOLECULE (bad or empty segment, more than nm atoms, left out by perception, bad bond
// range) or LP_BAD_INPUT (pocket_of or its pocket_ptr range out of bounds).  Block-uniform; nothing is read behind a failed check.
__device__ __forceinline__ int ligand_in_pocket(const int *__restrict__ lig_ptr, int b, int n_atoms, int nm,
                                                const int *__restrict__ bond_ptr, int cap_bonds, const int *__restrict__ mol_status,
                                                const int *__restrict__ pocket_of, const int *__restrict__ pocket_ptr, int n_pocket,
                                                int n_pockets, LigandInPocket &s) {
    s.seg = mol_segment(lig_ptr, b, n_atoms, s.a0, s.a1);
    s.n = s.a1 - s.a0;
    s.p0 = s.p1 = s.q0 = s.np = 0;
    if (!s.seg || s.n <= 0 || s.n > MOL_MAX || s.n > nm || (mol_status[b] & (MOL_EMPTY | MOL_CAPACITY | MOL_BAD_SEGMENT))) return LP_NO_MOLECULE;
    if (!mol_bond_range(bond_ptr, b, cap_bonds, s.p0, s.p1)) return LP_NO_MOLECULE;
    const int po = pocket_of[b];
    if (po < -1 || po >= n_pockets) return LP_BAD_INPUT;
    if (po >= 0) {
        s.q0 = pocket_ptr[po];
        const int q1 = pocket_ptr[po + 1];
        if (s.q0 < 0 || q1 < s.q0 || q1 > n_pocket) return LP_BAD_INPUT;
        s.np = q1 - s.q0;
    }
    return 0;
}

// what the threads of a workgroup found while staging atoms and pocket -> its status: two votes, not a sum (and a barrier)
__device__ __forceinline__ int lp_votes(int bad) {
    const int no_mol = __syncthreads_or(bad & LP_NO_MOLECULE), bad_in = __syncthreads_or(bad & LP_BAD_INPUT);
    return no_mol ? LP_NO_MOLECULE : bad_in ? LP_BAD_INPUT : 0;
}

// carves `bytes`, rounded up to `align` (a power of two), off an LDS layout that has grown to o; returns where they start
__host__ __device__ inline size_t lds_take(size_t &o, size_t bytes, size_t align) {
    const size_t at = o;
    o += (bytes + align - 1) & ~(align - 1);
    return at;
}

// ---- the host side: the arguments kpd_relax and kpd_vina_score share; every *_ok is the caller's "none of these is null"
static inline kpd_status ligand_pocket_args(int n_atoms, int B, int max_atoms, int F, int cap_bonds, int n_pocket, int P, int max_pocket,
                                            bool tables_ok, bool atoms_ok, bool ligands_ok, bool bonds_ok, bool pocket_ptr_ok,
                                            bool pocket_ok) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0 && n_pocket >= 0 && P >= 0 && max_pocket >= 0, KPD_ERR_INVALID,
                "n_atoms=%d B=%d F=%d cap_bonds=%d n_pocket=%d P=%d max_pocket=%d", n_atoms, B, F, cap_bonds, n_pocket, P, max_pocket);
    KPD_REQUIRE(max_atoms >= 1 && max_atoms <= MOL_MAX, KPD_ERR_INVALID, "max_atoms=%d (1 .. %d)", max_atoms, MOL_MAX);
    KPD_REQUIRE(tables_ok && (!n_atoms || atoms_ok) && (!B || ligands_ok), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || bonds_ok, KPD_ERR_INVALID, "null bond buffer");
    KPD_REQUIRE(!P || pocket_ptr_ok, KPD_ERR_INVALID, "null pocket_ptr");
    KPD_REQUIRE(!n_pocket || pocket_ok, KPD_ERR_INVALID, "null pocket buffer");
    return KPD_OK;
}

// as much of the largest pocket as fits beside the `fixed` bytes of a max_atoms ligand, in rows; -1 if that ligand does not fit
static inline int stage_rows(size_t fixed, size_t lds_budget, size_t row_bytes, int max_pocket) {
    if (fixed + 64 > lds_budget) return -1;
    return (int)std::min<size_t>((size_t)max_pocket, (lds_budget - 64 - fixed) / row_bytes);
}

}  // namespace kpd
