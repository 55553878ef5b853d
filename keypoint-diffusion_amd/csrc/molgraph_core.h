// "One wave takes one perceived ligand and builds its bond graph in the scope S", stated once for k_mol_keys (molset.hip),
// k_mol_sanitize (sanitize.hip), k_mol_add_hs (hydrogens.hip), k_smiles_build (smiles.hip) and k_pose_rmsd (pose_rmsd.hip; the last
// two under the unordered row contract, pose_rmsd with its labels for the orders): the entry check, the atom staging, the scope, the bond
// loop with its two row contracts, and the membership test.  include/kpd.h states the rule (kpd_mol_keys: which ligands have no
// molecule, which atoms count).  The pattern is that of vina_core.h: everything is __device__ __forceinline__, arrays come in as
// plain pointers (an LDS array stays in its address space after inlining), the __shared__ declarations and the kernels stay in
// their files, and what one kernel alone does with an atom or a bond comes in as a callable that is inlined at the call site.
// Also here: the bits of kpd_mol_sanitize's outputs that kpd_mol_add_hs reads, the fragment key that k_sdf_size (molecule.hip)
// shares with the scope, and the once-rounded fp64 vectors of sanitize.hip and hydrogens.hip (last section; molset.hip and
// molecule.hip use none of them).
#pragma once
#include "molecule_core.h"

namespace kpd {

// ---- kpd_mol_sanitize's outputs, as kpd_mol_add_hs reads them: the status bits and the six atom flags that are written out
enum : int { SAN_NO_MOLECULE = 1, SAN_TOO_MANY_RINGS = 2, SAN_COMPONENT_TOO_LARGE = 4 };
enum : unsigned { AT_RING = 1, AT_AROMATIC = 2, AT_DONOR = 4, AT_ACCEPTOR = 8, AT_UNSATISFIED = 16, AT_OVERVALENT = 32 };

// ---- the entry check -------------------------------------------------------------------------------------------------------------
// atoms [a0, a0 + n) (to be used only where seg: lig_ptr was well-formed), bonds [p0, p1) (only where range_ok); ok: the ligand
// has 1 .. MOL_MAX atoms, perception did not leave it out and both ranges are well-formed.  Wave-uniform.
struct MolEntry {
    int a0, n, p0, p1;
    bool seg, range_ok, ok;
};
__device__ __forceinline__ MolEntry mol_entry(const int *__restrict__ lig_ptr, int b, int n_atoms, const int *__restrict__ bond_ptr,
                                              int cap_bonds, const int *__restrict__ mol_status) {
    MolEntry e;
    int a1;
    e.seg = mol_segment(lig_ptr, b, n_atoms, e.a0, a1);
    e.n = a1 - e.a0;
    e.range_ok = mol_bond_range(bond_ptr, b, cap_bonds, e.p0, e.p1);
    e.ok = e.seg && e.n > 0 && e.n <= MOL_MAX && !(mol_status[b] & (MOL_EMPTY | MOL_CAPACITY | MOL_BAD_SEGMENT)) && e.range_ok;
    return e;
}

// ---- the atom staging ------------------------------------------------------------------------------------------------------------
// Z as a byte: 0 for a Z outside 0 .. 255, which no rule of sanitize.hip or hydrogens.hip knows either
__device__ __forceinline__ unsigned char mol_z_byte(int z) { return (unsigned char)(z >= 0 && z <= 255 ? z : 0); }

// Lane `lane` takes the atoms lane + 64 k.  An atom whose class is in 0 .. F-1 and whose fragment label is in 0 .. n-1 goes to
// accept(k, a, a0 + a, Z of its class): what the kernel keeps of it, and false if the kernel refuses it after all.  An accepted atom
// is counted in fsize (zeroed by the caller, a barrier before and after this) and has its label in fr_of[k]; every other atom of
// the ligand raises *bad and leaves fr_of[k] = -1.
template <class Accept>
__device__ __forceinline__ void mol_stage_atoms(const int *__restrict__ elem, int F, const int *__restrict__ zs, const int *__restrict__ frag,
                                                int a0, int n, int lane, int *fsize, int *bad, int (&fr_of)[MOL_K], Accept accept) {
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        fr_of[k] = -1;
        if (a < n) {
            const size_t g = (size_t)(a0 + a);
            const int e = elem[g], f = frag[g];
            if (e < 0 || e >= F || f < 0 || f >= n || !accept(k, a, g, zs[e])) {
                atomicOr(bad, 1);
            } else {
                fr_of[k] = f;
                atomicAdd(&fsize[f], 1);
            }
        }
    }
}

// ---- the scope S: the largest fragment (most atoms, then the lowest rank), or every atom -----------------------------------------
// the key of fragment f with `size` atoms: its maximum is the largest fragment; and the rank back out of a key
__device__ __forceinline__ int frag_key(int size, int f) { return size * MOL_MAX + (MOL_MAX - 1 - f); }
__device__ __forceinline__ int frag_key_rank(int key) { return MOL_MAX - 1 - key % MOL_MAX; }

__device__ __forceinline__ bool in_scope(const unsigned *inS, int a) { return (inS[a >> 5] >> (a & 31)) & 1u; }
__device__ __forceinline__ bool both_in_scope(const unsigned *inS, int i, int j) {
    return (inS[i >> 5] >> (i & 31)) & (inS[j >> 5] >> (j & 31)) & 1u;
}

struct MolScope {
    int rank, nS, n_frag;       // the fragment S is (-1: every atom), atoms in S, fragments of the ligand
};
// From the fsize and fr_of of mol_stage_atoms; writes the MOL_W words of inS and ends in a barrier.
__device__ __forceinline__ MolScope mol_scope(const int *fsize, const int (&fr_of)[MOL_K], int n, int lane, int largest_only,
                                              unsigned *inS) {
    MolScope s = {-1, 0, 0};
    if (largest_only) {
        int best = 0;
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int f = lane + 64 * k;
            if (f < n && fsize[f]) best = max(best, frag_key(fsize[f], f));
        }
        s.rank = frag_key_rank(wave_max(best));
    }
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        s.n_frag += __popcll(__ballot(lane + 64 * k < n && fsize[lane + 64 * k] > 0));
        const unsigned long long m = __ballot(fr_of[k] >= 0 && (s.rank < 0 || fr_of[k] == s.rank));
        s.nS += __popcll(m);
        if (lane == 0) {
            inS[2 * k] = (unsigned)m;
            inS[2 * k + 1] = (unsigned)(m >> 32);
        }
    }
    __syncthreads();
    return s;
}

// ---- the bond loop ---------------------------------------------------------------------------------------------------------------
// Bonds [p0, p1), a lane per row: both ends inside the ligand, label(row) in 1 .. max_label (the order, 1 .. 3; k_pose_rmsd: the
// caller's label, 1 .. 15, or 1 without any); a bond with both ends in S takes a slot in each end's neighbour list,
// nb[i * MOL_DEG + slot] = (NB)(j | common(local row, label)), and a seventh neighbour is refused.  Whatever
// is refused raises *bad.  deg zeroed by the caller, a barrier before and after this.  The two row contracts:
// ORDERED = false (sanitize, smiles, pose_rmsd; keys has this form written out in molset.hip, where the call cost time:
//   profiles/molgraph_core.md):
//   i != j, and a bond listed twice is found through the bit matrix adj (`stride` words per row, zeroed by the caller).  The first
//   mark goes on the (low, high) word whichever way round the bond is listed, so two lanes that meet (i, j) and (j, i) in the same
//   pass cannot both read "not yet"; upto is not touched.
// ORDERED = true (add_hs): i < j and the rows strictly ascending in (i, j), so none comes twice and adj is not touched; upto[i]
//   (zeroed by the caller) counts the rows that start at i, in S or not.
template <bool ORDERED, class NB, class Label, class Common>
__device__ __forceinline__ void mol_bond_graph(const int *__restrict__ bond_ij, int p0, int p1, int a0, int n, int lane, const unsigned *inS,
                                               unsigned *adj, int stride, int *deg, int *upto, NB *nb, int *bad, Label label, int max_label,
                                               Common common) {
    for (int k = p0 + lane; k < p1; k += 64) {
        const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0, o = label(k);
        bool good = (ORDERED ? i >= 0 && i < j && j < n : i >= 0 && i < n && j >= 0 && j < n && i != j) && o >= 1 && o <= max_label;
        if (ORDERED && good && k > p0) {
            const int pi = bond_ij[(size_t)(k - 1) * 2] - a0, pj = bond_ij[(size_t)(k - 1) * 2 + 1] - a0;
            good = pi < i || (pi == i && pj < j);
        }
        if (!good) {
            atomicOr(bad, 1);
            continue;
        }
        if (ORDERED) atomicAdd(&upto[i], 1);
        if (!both_in_scope(inS, i, j)) continue;
        bool twice = false;
        if (!ORDERED) {
            const int lo = min(i, j), hi = max(i, j);
            const unsigned was = atomicOr(&adj[lo * stride + (hi >> 5)], 1u << (hi & 31));
            atomicOr(&adj[hi * stride + (lo >> 5)], 1u << (lo & 31));
            twice = (was >> (hi & 31)) & 1u;
        }
        const int si = atomicAdd(&deg[i], 1), sj = atomicAdd(&deg[j], 1);
        if (twice || si >= MOL_DEG || sj >= MOL_DEG) {
            atomicOr(bad, 1);
            continue;
        }
        const unsigned c = common(k - p0, o);
        nb[i * MOL_DEG + si] = (NB)((unsigned)j | c);
        nb[j * MOL_DEG + sj] = (NB)((unsigned)i | c);
    }
}

// ---- fp64 vectors, every product, sum and quotient rounded once ------------------------------------------------------------------
// Exact only in files the Makefile compiles with -ffp-contract=off (sanitize.hip, hydrogens.hip): the __d*_rn functions of the HIP
// headers are plain operators, which the default setting may fuse after inlining.
struct V3 {
    double x, y, z;
};
__device__ __forceinline__ double vdot(V3 a, V3 b) { return __dadd_rn(__dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)), __dmul_rn(a.z, b.z)); }
__device__ __forceinline__ V3 vcross(V3 a, V3 b) {
    return {__dsub_rn(__dmul_rn(a.y, b.z), __dmul_rn(a.z, b.y)), __dsub_rn(__dmul_rn(a.z, b.x), __dmul_rn(a.x, b.z)),
            __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x))};
}
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return {__dadd_rn(a.x, b.x), __dadd_rn(a.y, b.y), __dadd_rn(a.z, b.z)}; }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return {__dsub_rn(a.x, b.x), __dsub_rn(a.y, b.y), __dsub_rn(a.z, b.z)}; }
__device__ __forceinline__ V3 vover(V3 a, double s) { return {__ddiv_rn(a.x, s), __ddiv_rn(a.y, s), __ddiv_rn(a.z, s)}; }
__device__ __forceinline__ V3 vneg(V3 a) { return {-a.x, -a.y, -a.z}; }
// x a + y b, component by component: (x a_c) + (y b_c)
__device__ __forceinline__ V3 vcomb(double x, V3 a, double y, V3 b) {
    return {__dadd_rn(__dmul_rn(x, a.x), __dmul_rn(y, b.x)), __dadd_rn(__dmul_rn(x, a.y), __dmul_rn(y, b.y)),
            __dadd_rn(__dmul_rn(x, a.z), __dmul_rn(y, b.z))};
}
__device__ __forceinline__ V3 vat(const float *p, int a) { return {(double)p[a * 3], (double)p[a * 3 + 1], (double)p[a * 3 + 2]}; }

}  // namespace kpd
