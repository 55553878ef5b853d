// Symmetry-corrected RMSD between poses of one molecule (kpd_pose_rmsd): the minimum over the automorphisms of the labelled bond
// graph of the unaligned RMSD, what upstream reads off Chem.CalcRMS(mol1, mol2) (analysis/pocket_minimization.py:21).  RDKit's
// substructure matcher cannot be restated: include/kpd.h defines the search down to the order of every candidate, and
// tests/pose_rmsd_ref.py restates it.  No agreement with RDKit's numbers is claimed.
// k_pose_rmsd: one wave per ligand.  The front end (entry check, atom staging, the scope S, the unordered bond loop with the
// caller's labels, 1 .. 15 or none, in place of the orders 1 .. 3) is that of molgraph_core.h.  The seed sum, the refinement step, the
// classes (a rank without tie-break) and the sort of the neighbour lists are those of molrefine_core.h and run across the lanes;
// only the loop of |S| steps around the refinement step is written out here, the one piece whose call cost time.  The source
// order is one breadth-first walk on lane 0.  Then every lane takes searches of its own, strided over the K poses (or the
// K (K - 1) / 2 pairs): the graph, the classes and the source order are shared in LDS, the images of a lane's search and its
// 256-bit "taken" mask lie in LDS over the dead arrays of the refinement, its running sums s_t in the scratch buffer (see
// 64 stacks of 256 fp64 do not fit in LDS), and the poses are read from global memory.  fp64, every product and sum
// rounded once: this file is compiled with -ffp-contract=off.
#include "common.h"
#include "engine.h"
#include "molgraph_core.h"
#include "molrefine_core.h"

namespace kpd {

enum : int { PR_NO_MOLECULE = 1, PR_MAX_NODES = 2, PR_NONFINITE = 4 };
constexpr unsigned short PR_NONE = 0xffff;
constexpr int PR_MAX_ATOM_LABEL = (1 << 20) - 1, PR_MAX_BOND_LABEL = 15, PR_MAX_PAIR_POSES = 64;

// d2(u, v): the fp64 squared distance of X[u] and Y[v] in the arithmetic of kpd_mol_perceive
__device__ __forceinline__ double pr_d2(const float *__restrict__ X, int u, const float *__restrict__ Y, int v) {
    return sum_sq((double)X[u * 3] - (double)Y[v * 3], (double)X[u * 3 + 1] - (double)Y[v * 3 + 1],
                  (double)X[u * 3 + 2] - (double)Y[v * 3 + 2]);
}

__global__ void __launch_bounds__(64)
k_pose_rmsd(const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F, const int *__restrict__ zs,
            const int *__restrict__ frag, const int *__restrict__ bond_ij, const int *__restrict__ bond_ptr, int cap_bonds,
            const int *__restrict__ mol_status, const int *__restrict__ bond_label, const int *__restrict__ atom_label, int largest_only,
            int skip_h, const float *__restrict__ ref_pos, const float *__restrict__ pos, int K, int pairs, long long max_nodes, int LU,
            double *__restrict__ rmsd, double *__restrict__ plain, int *__restrict__ map, long long *__restrict__ nodes,
            int *__restrict__ status, double *__restrict__ stack) {
    // buf, first life: x [2][MOL_MAX] and zk [MOL_MAX] (64-bit), the bit matrix A [MOL_MAX * MR_ROW]; second life, behind the
    // barrier after the source order: img [MOL_MAX][64] bytes (the image of u_t in the search of a lane) and taken [MOL_W][64]
    __shared__ u64 buf[MOL_MAX * 8 + MOL_W * 32];
    __shared__ long long av[MOL_MAX];               // A(a) = Z + 256 atom_label
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];
    __shared__ unsigned short nb[MOL_MAX * MOL_DEG];        // partner | L << 8, ascending partner once sorted
    __shared__ unsigned short cls[MOL_MAX];         // c(a) as the number of atoms of S with a smaller value: equal iff the values are
    __shared__ unsigned short at[MOL_MAX];          // the place of atom a in the source order
    __shared__ unsigned short par[MOL_MAX];         // the place of p(u_t), PR_NONE for a start atom
    __shared__ unsigned char ord[MOL_MAX];          // u_t
    __shared__ unsigned inS[MOL_W];
    __shared__ int bad;
    u64 *const x = buf, *const zk = buf + 2 * MOL_MAX;
    unsigned *const A = reinterpret_cast<unsigned *>(buf + 3 * MOL_MAX);
    unsigned char *const img = reinterpret_cast<unsigned char *>(buf);
    unsigned *const taken = reinterpret_cast<unsigned *>(buf + MOL_MAX * 8);
    static_assert(3 * MOL_MAX * 8 + MOL_MAX * MR_ROW * 4 <= sizeof(u64) * (MOL_MAX * 8 + MOL_W * 32), "the first life fits in buf");

    const int b = blockIdx.x, lane = threadIdx.x;
    const MolEntry en = mol_entry(lig_ptr, b, n_atoms, bond_ptr, cap_bonds, mol_status);
    const int a0 = en.a0, n = en.n;
    bool ok = en.ok;
    int nS = 0;
    if (ok) {                                       // wave-uniform, as every `ok` below
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            deg[a] = 0;
            fsize[a] = 0;
            at[a] = PR_NONE;
            for (int w = 0; w < MR_ROW; ++w) A[a * MR_ROW + w] = 0;
        }
        if (lane == 0) bad = 0;
        __syncthreads();
        int fr_of[MOL_K];
        bool is_h[MOL_K] = {false, false, false, false};
        mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int k, int a, size_t g, int z) {
            const int l = atom_label ? atom_label[g] : 0;
            if (l < 0 || l > PR_MAX_ATOM_LABEL) return false;
            av[a] = (long long)z + 256ll * l;
            zk[a] = (u64)av[a] * MR_K2;
            is_h[k] = z == 1;
            return true;
        });
        __syncthreads();
        ok = !bad;
        if (ok) {
            nS = mol_scope(fsize, fr_of, n, lane, largest_only, inS).nS;
            if (skip_h) {                           // Z = 1 leaves S after the scope is chosen: the fragment sizes count it
                nS = 0;
#pragma unroll
                for (int k = 0; k < MOL_K; ++k) {
                    const unsigned long long m = __ballot(in_scope(inS, lane + 64 * k) && !is_h[k]);
                    nS += __popcll(m);
                    __syncthreads();                // every lane has read the words of this k
                    if (lane == 0) {
                        inS[2 * k] = (unsigned)m;
                        inS[2 * k + 1] = (unsigned)(m >> 32);
                    }
                }
                __syncthreads();
            }
            // bonds with both ends in S: the unordered row contract with L in 1 .. 15 (1 without bond_label) for the order
            mol_bond_graph<false>(bond_ij, en.p0, en.p1, a0, n, lane, inS, A, MR_ROW, deg, (int *)nullptr, nb, &bad,
                                  [bond_label](int k) { return bond_label ? bond_label[k] : 1; }, PR_MAX_BOND_LABEL,
                                  [](int, int l) { return (unsigned)l << 8; });
            __syncthreads();
            ok = !bad && nS > 0;
        }
    }
    if (!ok) {                                      // the fills of the host are this ligand's outputs
        if (lane == 0) status[b] = PR_NO_MOLECULE;
        return;
    }
    // ---- the class c(a): inv_n of kpd_mol_keys on the labels A and L, across the lanes ------------------------------------------
    bool in[MOL_K];
    int dg[MOL_K];
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        in[k] = in_scope(inS, a);
        dg[k] = in[k] ? deg[a] : 0;
        if (in[k]) x[a] = mr_mix((u64)av[a] + (u64)dg[k] * MR_K3 + MR_K1 * mr_seed_sum(A, zk, inS, a));
    }
    __syncthreads();
    // |S| steps: a difference has reached every atom it can reach.  This is mr_refine_steps of molrefine_core.h written out: calling
    // it here put the kernel outside its time bound (profiles/molrefine_core.md)
    int cur = 0;
    for (int r = 1; r <= nS; ++r) {
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (in[k]) x[(cur ^ 1) * MOL_MAX + a] = mr_refine(x + cur * MOL_MAX, nb, dg[k], a);
        }
        __syncthreads();
        cur ^= 1;
    }
    {
        int less[MOL_K];
        mr_rank<false>(x + cur * MOL_MAX, inS, in, n, lane, less);
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            if (!in[k]) continue;
            cls[lane + 64 * k] = (unsigned short)less[k];
            mr_sort_row(nb + (lane + 64 * k) * MOL_DEG, dg[k], [](unsigned e) { return e & 0xffu; });        // neighbours in ascending index
        }
    }
    __syncthreads();
    // ---- the source order: breadth-first from the lowest atom not yet listed, neighbours in ascending index -------------------------
    if (lane == 0) {
        int t = 0, head = 0;
        for (int s = 0; s < n; ++s) {
            if (!in_scope(inS, s) || at[s] != PR_NONE) continue;
            ord[t] = (unsigned char)s;
            par[t] = PR_NONE;
            at[s] = (unsigned short)t++;
            for (; head < t; ++head) {
                const int u = ord[head];
                for (int q = 0; q < deg[u]; ++q) {
                    const int w = nb[u * MOL_DEG + q] & 0xffu;
                    if (at[w] != PR_NONE) continue;
                    ord[t] = (unsigned char)w;
                    par[t] = (unsigned short)head;
                    at[w] = (unsigned short)t++;
                }
            }
        }
    }
    __syncthreads();                                // x, zk and A are dead behind this barrier: img and taken lie over them
    // ---- the searches: lane takes the searches lane, lane + 64, .. ----------------------------------------------------------------
    const int n_search = pairs ? K * (K - 1) / 2 : K;
    const double inf = __builtin_inf();
    int flags = 0;
    for (int q = lane; q < n_search; q += 64) {
        int pi = 0, pj = q;
        if (pairs) {                                // the pairs i < j in row order
            int rem = q;
            while (rem >= K - 1 - pi) {
                rem -= K - 1 - pi;
                ++pi;
            }
            pj = pi + 1 + rem;
        }
        const float *X = (pairs ? pos + (size_t)pi * n_atoms * 3 : ref_pos) + (size_t)a0 * 3;
        const float *Y = pos + ((size_t)pj * n_atoms + a0) * 3;
        bool finite = true;
        double s_id = 0.0;
        for (int t = 0; t < nS; ++t) {
            const int u = ord[t];
            for (int c = 0; c < 3; ++c) finite = finite && finite_f(X[u * 3 + c]) && finite_f(Y[u * 3 + c]);
            s_id = __dadd_rn(s_id, pr_d2(X, u, Y, u));
        }
        if (!finite) {                              // zeros, nodes 0, map -1: the fills
            flags |= PR_NONFINITE;
            continue;
        }
        int *const map_row = !pairs && map ? map + (size_t)pj * n_atoms + a0 : nullptr;
        if (map_row)
            for (int t = 0; t < nS; ++t) map_row[ord[t]] = a0 + ord[t];
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) taken[w * 64 + lane] = 0;
        double *const st = stack + (size_t)a0 * LU + lane;         // s_t at st[t * LU], t = 1 .. nS - 1
        double best = s_id, s_t = 0.0, last_d = -1.0;              // candidates behind (last_d, last_v) at this depth are still to try
        int t = 0, last_v = -1;
        long long count = 0;
        for (;;) {
            const int u = ord[t], du = deg[u];
            const long long au = av[u];
            const unsigned short cu = cls[u];
            double bd = inf;
            int bv = -1;
            auto consider = [&](int v) {
                if (((taken[(v >> 5) * 64 + lane] >> (v & 31)) & 1u) || av[v] != au || deg[v] != du || cls[v] != cu) return;
                for (int s = 0; s < du; ++s) {      // every bond of u to an atom listed before it has its image at v
                    const unsigned e = nb[u * MOL_DEG + s];
                    const int tw = at[e & 0xffu];
                    if (tw >= t) continue;
                    const unsigned want = (unsigned)img[tw * 64 + lane] | (e & 0xff00u);
                    bool found = false;
                    for (int r = 0; r < du; ++r) found = found || nb[v * MOL_DEG + r] == want;
                    if (!found) return;
                }
                const double d = pr_d2(X, u, Y, v);
                if ((d > last_d || (d == last_d && v > last_v)) && (d < bd || (d == bd && v < bv))) {
                    bd = d;
                    bv = v;
                }
            };
            if (par[t] != PR_NONE) {
                const int pv = img[par[t] * 64 + lane];
                for (int s = 0; s < deg[pv]; ++s) consider(nb[pv * MOL_DEG + s] & 0xffu);
            } else {
                for (int v = 0; v < n; ++v)
                    if (in_scope(inS, v)) consider(v);
            }
            if (bv >= 0) {
                if (++count > max_nodes) {
                    flags |= PR_MAX_NODES;
                    break;
                }
                const double s = __dadd_rn(s_t, bd);
                if (s < best) {
                    if (t == nS - 1) {              // a whole automorphism, strictly better
                        best = s;
                        if (map_row) {
                            for (int k = 0; k < t; ++k) map_row[ord[k]] = a0 + img[k * 64 + lane];
                            map_row[u] = a0 + bv;
                        }
                        last_d = bd;
                        last_v = bv;
                    } else {
                        img[t * 64 + lane] = (unsigned char)bv;
                        taken[(bv >> 5) * 64 + lane] |= 1u << (bv & 31);
                        ++t;
                        st[(size_t)t * LU] = s;
                        s_t = s;
                        last_d = -1.0;
                        last_v = -1;
                    }
                    continue;
                }
            }
            // no candidate left at this depth, or none that can be smaller: back to the one above
            if (t == 0) break;
            --t;
            last_v = img[t * 64 + lane];
            taken[(last_v >> 5) * 64 + lane] &= ~(1u << (last_v & 31));
            last_d = pr_d2(X, ord[t], Y, last_v);
            s_t = t ? st[(size_t)t * LU] : 0.0;
        }
        const double r_best = __dsqrt_rn(__ddiv_rn(best, (double)nS)), r_id = __dsqrt_rn(__ddiv_rn(s_id, (double)nS));
        if (pairs) {                                // the upper triangle is computed, the lower one is its mirror
            const size_t ij = ((size_t)b * K + pi) * K + pj, ji = ((size_t)b * K + pj) * K + pi;
            rmsd[ij] = rmsd[ji] = r_best;
            plain[ij] = plain[ji] = r_id;
            nodes[ij] = nodes[ji] = count;
        } else {
            const size_t o = (size_t)b * K + pj;
            rmsd[o] = r_best;
            plain[o] = r_id;
            nodes[o] = count;
        }
    }
    const bool hit = __ballot(flags & PR_MAX_NODES) != 0, nonfinite = __ballot(flags & PR_NONFINITE) != 0;
    if (lane == 0) status[b] = (hit ? PR_MAX_NODES : 0) | (nonfinite ? PR_NONFINITE : 0);
}

}  // namespace kpd

using namespace kpd;

// how many lanes of a wave have a search: the stacks of s_t are sized by it
static int pose_rmsd_lanes(int K, int pairs) { return std::min(64, pairs ? K * (K - 1) / 2 : K); }

struct PoseRmsdScratch {
    int n_atoms, lanes;
    double *stack = nullptr;
    void operator()(Carve &c) { c(stack, (size_t)n_atoms * (size_t)lanes); }
};

extern "C" int64_t kpd_pose_rmsd_scratch_bytes(int32_t n_atoms, int32_t K, int32_t pairs) {
    if (n_atoms < 0 || K < 1 || (pairs != 0 && pairs != 1) || (pairs && K > PR_MAX_PAIR_POSES)) return -1;
    PoseRmsdScratch s{n_atoms, pose_rmsd_lanes(K, pairs)};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_pose_rmsd(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                                    const int32_t *frag, const int32_t *bond_ij, const int32_t *bond_ptr, int32_t cap_bonds,
                                    const int32_t *mol_status, const int32_t *bond_label, const int32_t *atom_label, int32_t largest_only,
                                    int32_t skip_h, const float *ref_pos, const float *pos, int32_t K, int32_t pairs, int64_t max_nodes,
                                    double *rmsd, double *plain, int32_t *map, int64_t *nodes, int32_t *status, void *scratch,
                                    void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0, KPD_ERR_INVALID, "n_atoms=%d B=%d F=%d cap_bonds=%d", n_atoms, B, F,
                cap_bonds);
    KPD_REQUIRE((pairs == 0 || pairs == 1) && K >= 1 && (!pairs || K <= PR_MAX_PAIR_POSES) && max_nodes >= 1, KPD_ERR_INVALID,
                "K=%d (>= 1; <= %d with pairs) pairs=%d (0 or 1) max_nodes=%lld (>= 1)", K, PR_MAX_PAIR_POSES, pairs, (long long)max_nodes);
    KPD_REQUIRE(lig_ptr && z && bond_ptr && scratch, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (elem && frag && pos && (pairs || ref_pos)), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (mol_status && rmsd && plain && nodes && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || bond_ij, KPD_ERR_INVALID, "null bond buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PoseRmsdScratch s{n_atoms, pose_rmsd_lanes(K, pairs)};
    carve_raw(static_cast<char *>(scratch), s);
    const size_t per = pairs ? (size_t)K * K : (size_t)K;
    if (B) {                                        // what a ligand without a molecule, a diagonal and a search left out read
        KPD_HIP(hipMemsetAsync(rmsd, 0, (size_t)B * per * 8, st));
        KPD_HIP(hipMemsetAsync(plain, 0, (size_t)B * per * 8, st));
        KPD_HIP(hipMemsetAsync(nodes, 0, (size_t)B * per * 8, st));
    }
    if (!pairs && map && n_atoms) KPD_HIP(hipMemsetAsync(map, 0xff, (size_t)K * n_atoms * 4, st));      // -1 outside S
    if (B) {
        hipLaunchKernelGGL(k_pose_rmsd, dim3(B), dim3(64), 0, st, lig_ptr, n_atoms, elem, F, z, frag, bond_ij, bond_ptr, cap_bonds, mol_status,
                           bond_label, atom_label, largest_only, skip_h, ref_pos, pos, K, pairs, (long long)max_nodes, s.lanes, rmsd, plain,
                           map, reinterpret_cast<long long *>(nodes), status, s.stack);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
