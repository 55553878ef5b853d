// Canonical SMILES of sanitised ligands (kpd_mol_smiles): one line of text per molecule from what kpd_mol_perceive and
// kpd_mol_sanitize left on the device.  Stands where upstream calls Chem.MolToSmiles(largest_mol) (analysis/metrics.py:102-147).
// RDKit's canonicalisation cannot be restated: include/kpd.h defines the rule down to the order of every choice, and
// tests/smiles_ref.py restates it.  NOT RDKit's canonical SMILES.
// k_smiles_build: one wave per ligand, everything in LDS.  The front end (entry check, atom staging, the scope S, the unordered
// bond loop) is that of molgraph_core.h, shared with k_mol_keys, k_mol_sanitize, k_mol_add_hs and k_pose_rmsd.  Seeds,
// refinement, the census of equal values and the tie-breaking loop run across the lanes, as do the ranks, the sort of
// the neighbour lists, the start atom of every fragment and the formatting of the tokens; the depth-first walk and the numbering
// of the ring closures are serial and stay on lane 0, with nothing but the order, the branch marks and the closure numbers on it.
// The bytes of a ligand go to scratch (at most SM_BYTES per atom, at its first atom's row), its length to the library's one
// exclusive scan, and k_smiles_copy moves the bytes to their place: three launches whatever B is, nothing is computed twice.
// The seed and refinement steps are those of k_mol_keys with the labels of the sanitised graph: molrefine_core.h states them once
// (with the loop of n steps, the rank and the sort of a neighbour row), shared with k_mol_keys and k_pose_rmsd.  Integer arithmetic only.
#include "common.h"
#include "engine.h"
#include "molgraph_core.h"
#include "molrefine_core.h"
#include "scan_core.h"

namespace kpd {

constexpr int SM_BYTES = 36;            // of text per atom of S, at most: '.' or '(', a bond, "[XxxxHn]", six closures "=%nn", ')'
constexpr int SM_MAX_H = 9, SM_MAX_CLOSURE = 99;
constexpr unsigned short SM_NONE = 0xffff;

enum : int { SMI_NO_MOLECULE = 1, SMI_EXHAUSTED = 2, SMI_CAPACITY = 4 };

// the smallest normal valence of the organic subset, 0 for every other element; v: the next ones (0 = none)
__device__ __forceinline__ int sm_valences(int z, int &v1, int &v2) {
    v1 = v2 = 0;
    switch (z) {
    case 5: return 3;
    case 6: return 4;
    case 7: v1 = 5; return 3;
    case 8: return 2;
    case 15: v1 = 5; return 3;
    case 16: v1 = 4; v2 = 6; return 2;
    case 9: case 17: case 35: case 53: return 1;
    default: return 0;
    }
}

// the hydrogens a SMILES reader gives a bare atom: total = the sum of its bond labels, an aromatic bond counting 1
__device__ __forceinline__ int sm_implied_h(int z, bool ar, int total) {
    int v1, v2;
    const int v0 = sm_valences(z, v1, v2);
    if (ar) return max(0, v0 - (total + 1));
    if (v0 >= total) return v0 - total;
    if (v1 >= total) return v1 - total;
    if (v2 >= total) return v2 - total;
    return 0;
}

// 0 nothing, 1 '-', 2 '=', 3 '#': label 1 is written only between two aromatic atoms, label 4 never
__device__ __forceinline__ unsigned sm_bond_code(unsigned label, bool ar_a, bool ar_b) {
    return label == 1 ? (ar_a && ar_b ? 1u : 0u) : label == 4 ? 0u : label;
}
__device__ __forceinline__ char sm_bond_char(unsigned code) { return code == 1 ? '-' : code == 2 ? '=' : '#'; }

// values of x equal over atoms of S: how many distinct ones, and the smallest that two atoms share (~0 if none)
__device__ __forceinline__ void sm_census(const u64 *x, const unsigned *inS, const bool (&in)[MOL_K], int n, int lane, int &n_distinct,
                                          u64 &shared) {
    u64 xa[MOL_K];
    int before[MOL_K], other[MOL_K];
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        xa[k] = in[k] ? x[lane + 64 * k] : 0;
        before[k] = other[k] = 0;
    }
    for (int b = 0; b < n; ++b) {
        if (!in_scope(inS, b)) continue;            // wave-uniform
        const u64 xb = x[b];
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            before[k] += xb == xa[k] && b < a;
            other[k] += xb == xa[k] && b != a;
        }
    }
    int d = 0;
    u64 s = ~0ull;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        if (!in[k]) continue;
        d += before[k] == 0;
        if (other[k] && xa[k] < s) s = xa[k];
    }
    n_distinct = wave_sum(d);
    shared = wave_min_u64(s);
}

// ---- one wave per ligand: the bytes of its string into scratch, their number and the status bits 0 and 1 ---------------------------
__global__ void __launch_bounds__(64)
k_smiles_build(const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F, const int *__restrict__ zs,
               const unsigned *__restrict__ symbols, const int *__restrict__ frag, const int *__restrict__ bond_ij,
               const int *__restrict__ order_k, const int *__restrict__ bond_flags, const int *__restrict__ bond_ptr, int cap_bonds,
               const int *__restrict__ mol_status, const int *__restrict__ san_status, const int *__restrict__ atom_h,
               const int *__restrict__ atom_flags, int largest_only, int aromatic, char *__restrict__ bytes, long long *__restrict__ len,
               int *__restrict__ st_out) {
    // A serves the BFS of the seeds and is dead after them: the arrays of the ranking, the walk and the tokens lie over it
    // (MR_ROW * 4 = 36 bytes per atom, exactly what they take), so the workgroup stays at 22 KB and seven fit a CU
    __shared__ unsigned A[MOL_MAX * MR_ROW];        // bonded, both ends in S
    __shared__ u64 x[2][MOL_MAX];
    __shared__ u64 zk[MOL_MAX];                     // Z K2
    __shared__ int zv[MOL_MAX];                     // Z
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];                  // atoms per fragment; later the start key of every fragment
    __shared__ unsigned short nb[MOL_MAX * MOL_DEG];        // partner | label << 8, after the ranking sorted by the partner's rank
    __shared__ unsigned short rank[MOL_MAX];
    __shared__ unsigned char hl[MOL_MAX];           // h << 1 | ar
    __shared__ unsigned char frl[MOL_MAX];          // fragment label
    unsigned short *const ent = reinterpret_cast<unsigned short *>(A);      // closures at the atom in written order: number | bond code << 8
    unsigned short *const vis = ent + MOL_MAX * MOL_DEG, *const par = vis + MOL_MAX, *const lastc = par + MOL_MAX;
    short *const closes = reinterpret_cast<short *>(lastc + MOL_MAX);       // ')' behind the atom
    int *const off = reinterpret_cast<int *>(closes + MOL_MAX);             // where the tokens of the t-th atom of the walk start
    unsigned char *const number = reinterpret_cast<unsigned char *>(off + MOL_MAX);    // the closure number a bond took where it opened
    unsigned char *const by_rank = number + MOL_MAX * MOL_DEG, *const ord = by_rank + MOL_MAX, *const cursor = ord + MOL_MAX,
                        *const paren = cursor + MOL_MAX, *const psym = paren + MOL_MAX, *const nent = psym + MOL_MAX;
    static_assert(MOL_DEG * 2 + 3 * 2 + 2 + 4 + MOL_DEG + 6 == MR_ROW * 4, "the arrays over A fill it exactly");
    __shared__ unsigned inS[MOL_W];
    __shared__ int bad, walk_flags;
    const int b = blockIdx.x, lane = threadIdx.x;
    const MolEntry en = mol_entry(lig_ptr, b, n_atoms, bond_ptr, cap_bonds, mol_status);
    const int a0 = en.a0, n = en.n;
    bool ok = en.ok && !(san_status[b] & SAN_NO_MOLECULE);
    int nS = 0, status = 0;
    long long total_len = 0;
    int fr_of[MOL_K] = {-1, -1, -1, -1};
    if (ok) {                                       // wave-uniform, as every `ok` below
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            deg[a] = 0;
            fsize[a] = 0;
            for (int w = 0; w < MR_ROW; ++w) A[a * MR_ROW + w] = 0;
        }
        if (lane == 0) bad = walk_flags = 0;
        __syncthreads();
        mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int, int a, size_t g, int z) {
            const int h = atom_h[g];
            if (h < 0 || h > SM_MAX_H) return false;
            zv[a] = z;
            zk[a] = (u64)(long long)z * MR_K2;
            hl[a] = (unsigned char)(h << 1 | (aromatic && (atom_flags[g] & AT_AROMATIC) ? 1 : 0));
            frl[a] = (unsigned char)frag[g];        // 0 .. n - 1: checked by the caller of this
            return true;
        });
        __syncthreads();
        ok = !bad;
    }
    if (ok) {
        nS = mol_scope(fsize, fr_of, n, lane, largest_only, inS).nS;
        mol_bond_graph<false>(bond_ij, en.p0, en.p1, a0, n, lane, inS, A, MR_ROW, deg, (int *)nullptr, nb, &bad,
                              [order_k](int k) { return order_k[k]; }, 3,
                              [&](int r, int o) { return (unsigned)(aromatic && (bond_flags[en.p0 + r] & 4) ? 4 : o) << 8; });
        __syncthreads();
        ok = !bad && nS > 0;
    }
    bool in[MOL_K];
    int dg[MOL_K];
    if (ok) {
        // a fragment label is a connected component: no bond of S joins two labels (and the walk below reaches every atom)
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            in[k] = in_scope(inS, a);
            dg[k] = in[k] ? deg[a] : 0;
            for (int s = 0; s < dg[k]; ++s)
                if (frl[nb[a * MOL_DEG + s] & 0xffu] != frl[a]) atomicOr(&bad, 1);
            fsize[a] = 0x7fffffff;                  // free since mol_scope's barrier: the start keys
        }
        __syncthreads();
        ok = !bad;
    }
    if (ok) {
        // seeds: every other atom of S by element and distance (mr_seed_sum, as k_mol_keys), with the hydrogens and the aromatic flag
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (a >= n || !in_scope(inS, a)) continue;
            x[0][a] = mr_mix((u64)(long long)zv[a] + (u64)deg[a] * MR_K3 + (u64)hl[a] * MR_K2 + MR_K1 * mr_seed_sum(A, zk, inS, a));
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {           // A is dead behind this barrier: the walk's arrays over it
            const int a = lane + 64 * k;
            vis[a] = par[a] = lastc[a] = SM_NONE;
            closes[a] = 0;
            cursor[a] = paren[a] = psym[a] = nent[a] = 0;
        }
        int cur = mr_refine_steps(&x[0][0], nb, in, dg, lane, 0, nS);       // |S| steps: a difference has reached every atom it can reach
        // ties: perturb the lowest-numbered atom of the smallest shared value, refine until no new value appears
        int n_distinct;
        u64 shared;
        sm_census(x[cur], inS, in, n, lane, n_distinct, shared);
        for (int round = 0; n_distinct < nS && round < nS; ++round) {       // wave-uniform
            int first = MOL_MAX;
#pragma unroll
            for (int k = MOL_K - 1; k >= 0; --k)
                if (in[k] && x[cur][lane + 64 * k] == shared) first = lane + 64 * k;
            first = wave_min_int(first);
            if (first < MOL_MAX && lane == (first & 63)) x[cur][first] = mr_mix(x[cur][first] + MR_K3);
            __syncthreads();
            int count = n_distinct + 1;
            for (int r = 0; r < nS; ++r) {
                cur = mr_refine_steps(&x[0][0], nb, in, dg, lane, cur, 1);
                sm_census(x[cur], inS, in, n, lane, n_distinct, shared);
                if (n_distinct == count) break;
                count = n_distinct;
            }
        }
        // ranks (equal values, which 64 bits make unheard of, in atom order: the ranks are a permutation whatever happens)
        {
            int less[MOL_K];
            mr_rank<true>(x[cur], inS, in, n, lane, less);
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                if (!in[k]) continue;
                const int a = lane + 64 * k;
                rank[a] = (unsigned short)less[k];
                by_rank[less[k]] = (unsigned char)a;
                atomicMin(&fsize[frl[a]], dg[k] << 16 | less[k]);       // the start atom: the lowest degree, then the lowest rank
            }
        }
        __syncthreads();
        // neighbour lists in ascending rank of the partner
#pragma unroll
        for (int k = 0; k < MOL_K; ++k)
            if (in[k]) mr_sort_row(nb + (lane + 64 * k) * MOL_DEG, dg[k], [&](unsigned e) { return rank[e & 0xffu]; });
        __syncthreads();
        // the serial part: the walk (order, parents, branch marks), then the closure numbers in written order
        if (lane == 0) {
            int t = 0, flags = 0;
            for (int r = 0; r < nS; ++r) {
                const int s = by_rank[r];
                if (fsize[frl[s]] != (deg[s] << 16 | r)) continue;
                if (vis[s] != SM_NONE) {            // a label with two start atoms cannot be; a start atom reached from another label neither
                    flags |= SMI_NO_MOLECULE;
                    break;
                }
                ord[t] = (unsigned char)s;
                vis[s] = (unsigned short)t++;
                int at = s;
                for (;;) {
                    const int slot = cursor[at];
                    if (slot < deg[at]) {
                        cursor[at] = (unsigned char)(slot + 1);
                        const unsigned e = nb[at * MOL_DEG + slot];
                        const int c = (int)(e & 0xffu);
                        if (vis[c] != SM_NONE) continue;        // the parent, or a ring closure: numbered below
                        par[c] = (unsigned short)at;
                        psym[c] = (unsigned char)sm_bond_code(e >> 8, hl[at] & 1, hl[c] & 1);
                        ord[t] = (unsigned char)c;
                        vis[c] = (unsigned short)t++;
                        at = c;
                        continue;
                    }
                    // every neighbour seen: the last child loses its parentheses
                    if (lastc[at] != SM_NONE) {
                        paren[lastc[at]] = 0;
                        --closes[ord[t - 1]];
                    }
                    const int p = par[at];
                    if (p == SM_NONE) break;
                    paren[at] = 1;
                    ++closes[ord[t - 1]];
                    lastc[p] = (unsigned short)at;
                    at = p;
                }
            }
            if (t != nS) flags |= SMI_NO_MOLECULE;  // a fragment label of more than one component
            u64 used_lo = 0, used_hi = 0;           // numbers 1 .. 64 and 65 .. 99 that are open
            for (int i = 0; i < t && !flags; ++i) {
                const int a = ord[i], pa = par[a], da = deg[a];
                unsigned short *mine = ent + a * MOL_DEG;
                int ne = 0;
                for (int s = 0; s < da; ++s) {      // closures that end here, ascending number
                    const int c = (int)(nb[a * MOL_DEG + s] & 0xffu);
                    if (vis[c] >= i || c == pa) continue;
                    int d = 0;
                    for (int q = 0; q < deg[c]; ++q)
                        if ((nb[c * MOL_DEG + q] & 0xffu) == (unsigned)a) d = number[c * MOL_DEG + q];
                    int w = ne++;
                    for (; w > 0 && mine[w - 1] > d; --w) mine[w] = mine[w - 1];
                    mine[w] = (unsigned short)d;
                }
                for (int q = 0; q < ne; ++q) {
                    const int d = mine[q];
                    if (d < 1) flags |= SMI_NO_MOLECULE;        // cannot be: the bond was numbered where it opened
                    else if (d <= 64) used_lo &= ~(1ull << (d - 1));
                    else used_hi &= ~(1ull << (d - 65));
                }
                for (int s = 0; s < da; ++s) {      // closures that open here, ascending rank of the partner
                    const unsigned e = nb[a * MOL_DEG + s];
                    const int c = (int)(e & 0xffu);
                    if (vis[c] <= i || par[c] == a) continue;
                    int d;
                    if (~used_lo) {
                        d = __ffsll((long long)~used_lo);
                        used_lo |= 1ull << (d - 1);
                    } else {
                        d = 64 + __ffsll((long long)~used_hi);
                        if (d > SM_MAX_CLOSURE) {
                            flags |= SMI_EXHAUSTED;
                            break;
                        }
                        used_hi |= 1ull << (d - 65);
                    }
                    number[a * MOL_DEG + s] = (unsigned char)d;
                    mine[ne++] = (unsigned short)(d | sm_bond_code(e >> 8, hl[a] & 1, hl[c] & 1) << 8);
                }
                nent[a] = (unsigned char)ne;
            }
            walk_flags = flags;
        }
        __syncthreads();
        status = walk_flags;
        ok = !status;
    } else {
        status = SMI_NO_MOLECULE;
    }
    if (ok) {
        // tokens in parallel: lane takes the atoms lane, lane + 64, .. of the walk; lengths, their prefix sums, then the bytes
        char *out = bytes + (size_t)a0 * SM_BYTES;
        int base = 0;
        for (int pass = 0; pass < 2; ++pass) {
            base = 0;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int t = lane + 64 * k;
                int l = 0;
                if (t < nS) {
                    const int a = ord[t];
                    const bool ar = hl[a] & 1;
                    const int h = hl[a] >> 1, z = zv[a];
                    char *dst = out + (pass ? off[t] : 0);
                    auto put = [&](char ch) {
                        if (pass) dst[l] = ch;
                        ++l;
                    };
                    if (par[a] == SM_NONE) {
                        if (t > 0) put('.');
                    } else {
                        if (paren[a]) put('(');
                        if (psym[a]) put(sm_bond_char(psym[a]));
                    }
                    int total = 0;
                    for (int s = 0; s < deg[a]; ++s) {
                        const int lb = nb[a * MOL_DEG + s] >> 8;
                        total += lb == 4 ? 1 : lb;
                    }
                    int v1, v2;
                    const bool organic = sm_valences(z, v1, v2) != 0 && (!ar || z == 5 || z == 6 || z == 7 || z == 8 || z == 15 || z == 16);
                    const bool bare = organic && sm_implied_h(z, ar, total) == h;
                    const unsigned sym = symbols[elem[a0 + a]];
                    if (!bare) put('[');
                    for (int q = 0; q < 4; ++q) {
                        char ch = (char)((sym >> (8 * q)) & 0xffu);
                        if (!ch) break;
                        if (q == 0 && ar && ch >= 'A' && ch <= 'Z') ch = (char)(ch + 32);
                        put(ch);
                    }
                    if (!bare) {
                        if (h >= 1) put('H');
                        if (h >= 2) put((char)('0' + h));
                        put(']');
                    }
                    for (int q = 0; q < nent[a]; ++q) {
                        const unsigned e = ent[a * MOL_DEG + q], d = e & 0xffu;
                        if (e >> 8) put(sm_bond_char(e >> 8));
                        if (d >= 10) {
                            put('%');
                            put((char)('0' + d / 10));
                        }
                        put((char)('0' + d % 10));
                    }
                    for (int q = 0; q < closes[a]; ++q) put(')');
                }
                if (pass == 0) {
                    int tot;
                    const int ex = wave_exclusive(l, lane, tot);
                    if (t < nS) off[t] = base + ex;
                    base += tot;
                }
            }
            if (pass == 0) {
                total_len = base;
                if (base > SM_BYTES * nS) {         // cannot be (the bound of SM_BYTES counts every byte an atom can bring)
                    status = SMI_NO_MOLECULE;
                    total_len = 0;
                    break;
                }
                __syncthreads();
            }
        }
    }
    if (lane == 0) {
        len[b] = total_len;
        st_out[b] = status;
    }
}

// ---- the bytes to their place: one workgroup per ligand; a ligand that ends beyond the capacity is not written ---------------------
__global__ void __launch_bounds__(256)
k_smiles_copy(const char *__restrict__ bytes, const int *__restrict__ lig_ptr, const int *__restrict__ st, const long long *__restrict__ text_ptr,
              long long capacity, char *__restrict__ text, int *__restrict__ status) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long t0 = text_ptr[b], t1 = text_ptr[b + 1];
    const int s = st[b];
    if (s || t1 > capacity) {                       // block-uniform
        if (tid == 0) status[b] = s ? s : SMI_CAPACITY;
        return;
    }
    if (tid == 0) status[b] = 0;
    const char *src = bytes + (size_t)lig_ptr[b] * SM_BYTES;   // checked by k_smiles_build: s would be set otherwise
    for (long long k = tid; k < t1 - t0; k += 256) text[t0 + k] = src[k];
}

}  // namespace kpd

using namespace kpd;

// the bytes of every ligand's string before they are packed, their number and the status of the build per ligand
struct SmilesScratch {
    int n_atoms, B;
    long long *len = nullptr;
    int *st = nullptr;
    char *bytes = nullptr;
    void operator()(Carve &c) { c(len, (size_t)B); c(st, (size_t)B); c(bytes, (size_t)n_atoms * SM_BYTES); }
};

extern "C" int64_t kpd_smiles_scratch_bytes(int32_t n_atoms, int32_t B) {
    if (n_atoms < 0 || B < 0) return -1;
    SmilesScratch s{n_atoms, B};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_mol_smiles(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                                     const uint32_t *symbols, const int32_t *frag, const int32_t *bond_ij, const int32_t *order_k,
                                     const int32_t *bond_flags, const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status,
                                     const int32_t *san_status, const int32_t *atom_h, const int32_t *atom_flags, int32_t largest_only,
                                     int32_t aromatic, uint8_t *text, int64_t capacity, int64_t *text_ptr, int32_t *status, void *scratch,
                                     void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0 && capacity >= 0, KPD_ERR_INVALID,
                "n_atoms=%d B=%d F=%d cap_bonds=%d capacity=%lld", n_atoms, B, F, cap_bonds, (long long)capacity);
    KPD_REQUIRE(aromatic == 0 || aromatic == 1, KPD_ERR_INVALID, "aromatic=%d (0: Kekule form, 1: aromatic form)", aromatic);
    KPD_REQUIRE(lig_ptr && z && symbols && bond_ptr && text_ptr && scratch, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (elem && frag && atom_h && atom_flags), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (mol_status && san_status && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || (bond_ij && order_k && bond_flags), KPD_ERR_INVALID, "null bond buffer");
    KPD_REQUIRE(!capacity || text, KPD_ERR_INVALID, "null text buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SmilesScratch s{n_atoms, B};
    carve_raw(static_cast<char *>(scratch), s);
    long long *len = s.len;
    int *build_status = s.st;
    char *bytes = s.bytes;
    if (B) {
        hipLaunchKernelGGL(k_smiles_build, dim3(B), dim3(64), 0, st, lig_ptr, n_atoms, elem, F, z, symbols, frag, bond_ij, order_k, bond_flags,
                           bond_ptr, cap_bonds, mol_status, san_status, atom_h, atom_flags, largest_only, aromatic, bytes, len, build_status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, len, B, reinterpret_cast<long long *>(text_ptr)));
    if (B) {
        hipLaunchKernelGGL(k_smiles_copy, dim3(B), dim3(256), 0, st, bytes, lig_ptr, build_status, reinterpret_cast<const long long *>(text_ptr),
                           (long long)capacity, reinterpret_cast<char *>(text), status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
