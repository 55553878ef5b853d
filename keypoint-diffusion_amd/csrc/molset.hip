// Properties of the SET of sampled ligands on the device: a key per molecule that is equal for isomorphic bond graphs
// (uniqueness, novelty: analysis/metrics.py:135-147 compares canonical SMILES) and a substructure fingerprint per molecule with
// the pairwise Tanimoto distances inside a pocket's samples (MoleculeProperties.calculate_diversity, :263-277, over RDKit
// fingerprints).  Both are read off the bond graph kpd_mol_perceive left on the device; include/kpd.h states the rule.
// Everything but the final Tanimoto ratio is integer arithmetic modulo 2^64 with commutative sums, so neither the order of the
// atoms nor that of the bonds (nor of the LDS atomics that build the neighbour lists) can show in a result.
// k_mol_keys: one wave per ligand, as k_mol_perceive.  Adjacency bit rows and neighbour lists in LDS, all-pairs BFS with a
// lane per source atom and the frontier as a bitset in registers, the invariants double-buffered, lanes stride over the atoms
// in passes of 64.  k_fp_diversity: one workgroup per group, a thread per pair, fp64 partial sums reduced by a fixed tree.
// The front end of k_mol_keys (entry check, atom staging, the scope S, the membership test) is that of molgraph_core.h, shared
// with k_mol_sanitize and k_mol_add_hs; the bond loop is the header's unordered form written out here, the one piece whose call
// cost time.  The invariant (mix, the constants, the seed's BFS, the refinement step and its loop) is that of molrefine_core.h,
// shared with k_smiles_build and k_pose_rmsd.  The header's fp64 vectors are not used here (no -ffp-contract=off).
#include "common.h"
#include "molgraph_core.h"
#include "molrefine_core.h"

namespace kpd {

constexpr int MS_FP_WORDS = 128;        // nbits <= 4096

enum : int { KEY_NO_MOLECULE = 1 };
enum : int { DIV_BAD_SEGMENT = 1 };

__device__ __forceinline__ void set_fp_bit(unsigned *row, u64 h, int nwords) {
    const unsigned bit = (unsigned)h & (unsigned)(nwords * 32 - 1);
    atomicOr(&row[bit >> 5], 1u << (bit & 31));
}

// ---- 1. keys and fingerprints: one wave per ligand -----------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_mol_keys(const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F, const int *__restrict__ zs,
           const int *__restrict__ frag, const int *__restrict__ bond_ij, const int *__restrict__ bond_order,
           const int *__restrict__ bond_ptr, int cap_bonds, const int *__restrict__ mol_status, int largest_only, int with_orders,
           int radius, int nwords, long long *__restrict__ key, unsigned *__restrict__ fp, long long *__restrict__ atom_inv,
           int *__restrict__ status) {
    __shared__ unsigned A[MOL_MAX * MR_ROW];        // bonded, both ends in S
    __shared__ u64 inv[2][MOL_MAX];
    __shared__ u64 zk[MOL_MAX];                     // Z K2
    __shared__ int zv[MOL_MAX];                     // Z
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];
    __shared__ unsigned short nbr[MOL_MAX * MOL_DEG];
    __shared__ unsigned inS[MOL_W];
    __shared__ unsigned row[MS_FP_WORDS];
    __shared__ int bad;
    const int b = blockIdx.x, lane = threadIdx.x;
    const MolEntry en = mol_entry(lig_ptr, b, n_atoms, bond_ptr, cap_bonds, mol_status);
    const int a0 = en.a0, n = en.n;
    bool ok = en.ok;
    unsigned *out_row = fp + (size_t)b * nwords;
    if (ok) {                                       // wave-uniform, as every `ok` below
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            deg[a] = 0;
            fsize[a] = 0;
            for (int w = 0; w < MR_ROW; ++w) A[a * MR_ROW + w] = 0;
        }
        for (int w = lane; w < MS_FP_WORDS; w += 64) row[w] = 0;
        if (lane == 0) bad = 0;
        __syncthreads();
        // atoms: atomic number of the class (the full int), sizes of the fragments
        int fr_of[MOL_K];
        mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int, int a, size_t, int z) {
            zv[a] = z;
            zk[a] = (u64)(long long)z * MR_K2;
            return true;
        });
        __syncthreads();
        ok = !bad;
        int nS = 0;
        if (ok) {
            nS = mol_scope(fsize, fr_of, n, lane, largest_only, inS).nS;
            // bonds with both ends in S: adjacency bits and neighbour lists (the order of a list does not matter).  This is
            // mol_bond_graph<false> of molgraph_core.h written out: calling it here costs 1.7 % (profiles/molgraph_core.md)
            for (int k = en.p0 + lane; k < en.p1; k += 64) {
                const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0, o = bond_order[k];
                if (i < 0 || i >= n || j < 0 || j >= n || i == j || o < 1 || o > 3) {
                    atomicOr(&bad, 1);
                    continue;
                }
                if (!both_in_scope(inS, i, j)) continue;
                const unsigned l = with_orders ? (unsigned)o : 1u;
                const int lo = min(i, j), hi = max(i, j);   // the first mark is on one word whichever way round the bond is listed
                const unsigned was = atomicOr(&A[lo * MR_ROW + (hi >> 5)], 1u << (hi & 31));
                atomicOr(&A[hi * MR_ROW + (lo >> 5)], 1u << (lo & 31));
                const int si = atomicAdd(&deg[i], 1), sj = atomicAdd(&deg[j], 1);
                if (((was >> (hi & 31)) & 1u) || si >= MOL_DEG || sj >= MOL_DEG) {          // a bond twice, or a seventh neighbour
                    atomicOr(&bad, 1);
                    continue;
                }
                nbr[i * MOL_DEG + si] = (unsigned short)((unsigned)j | l << 8);
                nbr[j * MOL_DEG + sj] = (unsigned short)((unsigned)i | l << 8);
            }
            __syncthreads();
            ok = !bad && nS > 0;
        }
        if (ok) {
            bool in[MOL_K];
            int dg[MOL_K], m2 = 0;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                in[k] = in_scope(inS, a);
                dg[k] = in[k] ? deg[a] : 0;
                m2 += dg[k];
            }
            const int m = wave_sum(m2) / 2;
            // fingerprint: local seeds, `radius` steps, a bit per atom and step
            int cur = 0;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                if (!in[k]) continue;
                const u64 f0 = mr_mix((u64)(long long)zv[a] + (u64)dg[k] * MR_K3);
                inv[0][a] = f0;
                set_fp_bit(row, f0, nwords);
            }
            __syncthreads();
            for (int r = 1; r <= radius; ++r) {
#pragma unroll
                for (int k = 0; k < MOL_K; ++k) {
                    const int a = lane + 64 * k;
                    if (!in[k]) continue;
                    const u64 f = mr_refine(inv[cur], nbr, dg[k], a);
                    inv[cur ^ 1][a] = f;
                    set_fp_bit(row, f, nwords);
                }
                __syncthreads();
                cur ^= 1;
            }
            for (int w = lane; w < nwords; w += 64) out_row[w] = row[w];
            // key seeds: every other atom of S by element and distance (mr_seed_sum), then |S| steps: a difference has reached every
            // atom it can reach (inv is free: the barrier after the last fingerprint step is behind every lane, and the BFS reads none of it)
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                if (in[k]) inv[0][a] = mr_mix((u64)(long long)zv[a] + (u64)dg[k] * MR_K3 + MR_K1 * mr_seed_sum(A, zk, inS, a));
            }
            __syncthreads();
            cur = mr_refine_steps(&inv[0][0], nbr, in, dg, lane, 0, nS);
            u64 total = 0;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                if (!in[k]) continue;
                total += mr_mix(inv[cur][a]);
                if (atom_inv) atom_inv[a0 + a] = (long long)inv[cur][a];
            }
            total = wave_sum(total);
            if (lane == 0) {
                key[b] = (long long)mr_mix((u64)nS + (u64)m * MR_K3 + MR_K1 * total);
                status[b] = 0;
            }
            return;
        }
    }
    for (int w = lane; w < nwords; w += 64) out_row[w] = 0;
    if (lane == 0) {
        key[b] = 0;
        status[b] = KEY_NO_MOLECULE;
    }
}

// ---- 2. Tanimoto distances inside groups: one workgroup per group ------------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ double tanimoto_distance(const unsigned *__restrict__ a, const unsigned *__restrict__ b, int W) {
    int c = 0, u = 0;
    if (VEC) {
        const uint4 *a4 = reinterpret_cast<const uint4 *>(a), *b4 = reinterpret_cast<const uint4 *>(b);
        for (int w = 0; w < W / 4; ++w) {
            const uint4 x = a4[w], y = b4[w];
            c += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
            u += __popc(x.x | y.x) + __popc(x.y | y.y) + __popc(x.z | y.z) + __popc(x.w | y.w);
        }
    } else {
        for (int w = 0; w < W; ++w) {
            c += __popc(a[w] & b[w]);
            u += __popc(a[w] | b[w]);
        }
    }
    return u ? 1.0 - (double)c / (double)u : 0.0;
}

// Thread t takes the pairs (i, i + 1 + t + 256 q) of every used i in ascending order; the partial sums meet in a fixed tree.
// Nothing depends on where the group stands in the batch.
template <bool VEC>
__global__ void __launch_bounds__(256)
k_fp_diversity(const unsigned *__restrict__ fp, const unsigned char *__restrict__ use, const int *__restrict__ group_ptr, int B, int W,
               double *__restrict__ div_sum, long long *__restrict__ n_pairs, int *__restrict__ status) {
    __shared__ double part[256];
    __shared__ long long count[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int g0 = group_ptr[g], g1 = group_ptr[g + 1];
    if (g0 < 0 || g1 < g0 || g1 > B) {              // block-uniform
        if (tid == 0) {
            div_sum[g] = 0.0;
            n_pairs[g] = 0;
            status[g] = DIV_BAD_SEGMENT;
        }
        return;
    }
    double s = 0.0;
    long long c = 0;
    for (int i = g0; i < g1; ++i) {
        if (!use[i]) continue;                      // block-uniform
        const unsigned *a = fp + (size_t)i * W;
        for (long long j = (long long)i + 1 + tid; j < g1; j += 256) {
            if (!use[j]) continue;
            s += tanimoto_distance<VEC>(a, fp + (size_t)j * W, W);
            ++c;
        }
    }
    part[tid] = s;
    count[tid] = c;
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
        if (tid < off) {
            part[tid] += part[tid + off];
            count[tid] += count[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        div_sum[g] = part[0];
        n_pairs[g] = count[0];
        status[g] = 0;
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_mol_keys(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                                   const int32_t *frag, const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr,
                                   int32_t cap_bonds, const int32_t *mol_status, int32_t largest_only, int32_t with_orders,
                                   int32_t radius, int32_t nbits, int64_t *key, uint32_t *fp, int64_t *atom_inv, int32_t *status,
                                   void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0, KPD_ERR_INVALID, "n_atoms=%d B=%d F=%d cap_bonds=%d", n_atoms, B, F,
                cap_bonds);
    KPD_REQUIRE(radius >= 0 && radius <= 4 && nbits >= 64 && nbits <= 32 * MS_FP_WORDS && !(nbits & (nbits - 1)), KPD_ERR_INVALID,
                "radius=%d (0 .. 4) nbits=%d (a power of two, 64 .. 4096)", radius, nbits);
    KPD_REQUIRE(lig_ptr && z && bond_ptr, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (elem && frag), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (mol_status && key && fp && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || (bond_ij && bond_order), KPD_ERR_INVALID, "null bond buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (atom_inv && n_atoms) KPD_HIP(hipMemsetAsync(atom_inv, 0, (size_t)n_atoms * 8, st));      // 0 outside S
    if (B) {
        hipLaunchKernelGGL(k_mol_keys, dim3(B), dim3(64), 0, st, lig_ptr, n_atoms, elem, F, z, frag, bond_ij, bond_order, bond_ptr, cap_bonds,
                           mol_status, largest_only, with_orders, radius, nbits / 32, reinterpret_cast<long long *>(key), fp,
                           reinterpret_cast<long long *>(atom_inv), status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}

extern "C" kpd_status kpd_fp_diversity(const uint32_t *fp, const uint8_t *use, int32_t B, int32_t W, const int32_t *group_ptr, int32_t G,
                                       double *div_sum, int64_t *n_pairs, int32_t *status, void *stream) {
    KPD_REQUIRE(B >= 0 && W >= 1 && G >= 0, KPD_ERR_INVALID, "B=%d W=%d G=%d", B, W, G);
    KPD_REQUIRE(group_ptr && (!B || (fp && use)) && (!G || (div_sum && n_pairs && status)), KPD_ERR_INVALID, "null argument");
    if (!G) return KPD_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long *np = reinterpret_cast<long long *>(n_pairs);
    if (W % 4 == 0 && reinterpret_cast<uintptr_t>(fp) % 16 == 0)       // rows of whole 16-byte pieces
        hipLaunchKernelGGL(k_fp_diversity<true>, dim3(G), dim3(256), 0, st, fp, use, group_ptr, B, W, div_sum, np, status);
    else
        hipLaunchKernelGGL(k_fp_diversity<false>, dim3(G), dim3(256), 0, st, fp, use, group_ptr, B, W, div_sum, np, status);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}
