// Molecules from sampled ligands on the device: atoms -> bond graph -> valences, fragments, validity counts, SDF text.
// Replaces, for the array-level part, make_mol_openbabel (analysis/molecule_builder.py:38-60: a per-ligand XYZ string round
// trip through openbabel), check_atom_valency / compute_avg_frag_size (analysis/metrics.py:156-206) and the SDF writing of
// sample.py.  The rule is the lookup-table builder of the EDM / DiffSBDD lineage, stated in include/kpd.h: connectivity from
// covalent radii, bond orders as length classes, both under valence caps.  Every decision compares an fp64 squared distance
// (exact differences of the fp32 coordinates, products and sums rounded once each, no contraction) with an integer threshold,
// so a float64 restatement reproduces it bit for bit.
// One wave per ligand: positions, the adjacency and the two order bit matrices (256 x 256 bits each) live in LDS; the serial
// steps (degree pruning, valence repair) walk the atoms in order with a wave-wide argmax inside; trip counts are wave-uniform.
// Small latency-bound kernels; nothing is shared between ligands, no float atomics, bitwise independent of batch composition.
#include "common.h"
#include "emit_core.h"
#include "engine.h"
#include "molgraph_core.h"
#include "scan_core.h"

namespace kpd {

enum : int { SDF_NONFINITE = 1, SDF_WIDE = 2, SDF_NO_MOLECULE = 4, SDF_CAPACITY = 8 };

// the bond of the wave's candidates with the highest (order, d2, partner), on every lane
__device__ __forceinline__ void wave_argmax(int &o, double &d, int &j) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const int oo = __shfl_xor(o, off), oj = __shfl_xor(j, off);
        const double od = __shfl_xor(d, off);
        if (oo > o || (oo == o && (od > d || (od == d && oj > j)))) {
            o = oo;
            d = od;
            j = oj;
        }
    }
}

__device__ __forceinline__ void clear_pair(unsigned *M, int i, int j) {
    M[i * MOL_W + (j >> 5)] &= ~(1u << (j & 31));
    M[j * MOL_W + (i >> 5)] &= ~(1u << (i & 31));
}

// ---- 1. perceive: one wave per ligand --------------------------------------------------------------------------------
// Bonds go to the ligand's own part of the scratch list (rows [3 a0, 3 a1): degree <= 6 bounds them by 3 n), in (i, j) order.
__global__ void __launch_bounds__(64)
k_mol_perceive(const float *__restrict__ pos, const float *__restrict__ feat, const int *__restrict__ lig_ptr, int n_atoms, int F,
               const int *__restrict__ zs, const int *__restrict__ allowed, int *__restrict__ elem, int *__restrict__ valence,
               int *__restrict__ frag, int *__restrict__ tmp_ij, int *__restrict__ tmp_order, int *__restrict__ n_bonds,
               int *__restrict__ summary, int *__restrict__ status) {
    __shared__ float p[MOL_MAX * 3];
    __shared__ unsigned A1[MOL_MAX * MOL_W];        // bonded
    __shared__ unsigned A2[MOL_MAX * MOL_W];        // order >= 2
    __shared__ unsigned A3[MOL_MAX * MOL_W];        // order >= 3
    __shared__ unsigned el[MOL_MAX];                // element_row of the atom; radii zeroed for an atom that is never bonded
    __shared__ int label[MOL_MAX];
    __shared__ int fsize[MOL_MAX];
    const int b = blockIdx.x, lane = threadIdx.x;
    int a0, a1;
    const bool ok = mol_segment(lig_ptr, b, n_atoms, a0, a1);
    const int n = a1 - a0;
    if (!ok || n > MOL_MAX || n == 0) {
        if (lane == 0) {
            status[b] = (!ok || n > MOL_MAX) ? MOL_BAD_SEGMENT : MOL_EMPTY;
            n_bonds[b] = 0;
            summary[b * 4] = summary[b * 4 + 1] = summary[b * 4 + 2] = summary[b * 4 + 3] = 0;
        }
        return;
    }
    // atoms: coordinates, element decode, table row
    int st = 0;
    int cls[MOL_K];
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        cls[k] = 0;
        if (a < n) {
            const size_t g = (size_t)(a0 + a);
            const float x = pos[g * 3], y = pos[g * 3 + 1], z = pos[g * 3 + 2];
            p[a * 3] = x;
            p[a * 3 + 1] = y;
            p[a * 3 + 2] = z;
            const int c = argmax_first(feat + g * F, F);
            cls[k] = c;
            elem[g] = c;
            unsigned row = element_row(zs[c]);
            const bool finite = finite_f(x) && finite_f(y) && finite_f(z);
            if (!row || !finite) st = MOL_BAD_ATOM;
            if (!finite) row &= 0xff000000u;
            el[a] = row;
        }
    }
    __syncthreads();
    // step 1: candidates, every row on its own lane (d2 and the threshold are symmetric in i and j)
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int i = lane + 64 * k;
        if (i >= n) continue;
        const unsigned ri = el[i] & 0xffu;
        for (int w = 0; w < MOL_W; ++w) {
            unsigned bits = 0;
            const int j1 = min(n, 32 * w + 32);
            for (int j = 32 * w; j < j1; ++j) {
                if (j == i) continue;
                const double d2 = mol_d2(p, i, j);
                if (d2 > 0.16 && within(d2, ri, el[j] & 0xffu, 45)) bits |= 1u << (j & 31);
            }
            A1[i * MOL_W + w] = bits;
        }
    }
    __syncthreads();
    // step 2: degree pruning, atoms in order; the lane holds d2 of the partners lane, lane + 64, ...
    for (int i = 0; i < n; ++i) {
        int deg = 0;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) deg += __popc(A1[i * MOL_W + w]);
        const int cap = (int)(el[i] >> 24);
        if (deg <= cap) continue;                   // wave-uniform
        double key[MOL_K];
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int j = lane + 64 * k;
            key[k] = ((A1[i * MOL_W + (j >> 5)] >> (j & 31)) & 1u) ? mol_d2(p, i, j) : -1.0;
        }
        while (deg > cap) {
            int o = 0, bj = -1;
            double bd = -1.0;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k)
                if (key[k] >= bd && key[k] >= 0.0) {     // later k = larger partner wins a tie
                    bd = key[k];
                    bj = lane + 64 * k;
                }
            wave_argmax(o, bd, bj);
#pragma unroll
            for (int k = 0; k < MOL_K; ++k)
                if (bj == lane + 64 * k) key[k] = -1.0;
            if (lane == 0) clear_pair(A1, i, bj);
            --deg;
        }
        __syncthreads();
    }
    // step 3: order by length, every row on its own lane
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int i = lane + 64 * k;
        if (i >= n) continue;
        const unsigned ei = el[i];
        for (int w = 0; w < MOL_W; ++w) {
            unsigned bits = A1[i * MOL_W + w], b2 = 0, b3 = 0;
            while (bits) {
                const int t = __ffs(bits) - 1, j = 32 * w + t;
                bits &= bits - 1;
                const unsigned ej = el[j];
                const double d2 = mol_d2(p, i, j);
                if (within(d2, (ei >> 16) & 0xffu, (ej >> 16) & 0xffu, 3)) {
                    b3 |= 1u << t;
                    b2 |= 1u << t;
                } else if (within(d2, (ei >> 8) & 0xffu, (ej >> 8) & 0xffu, 5)) {
                    b2 |= 1u << t;
                }
            }
            A2[i * MOL_W + w] = b2;
            A3[i * MOL_W + w] = b3;
        }
    }
    __syncthreads();
    // step 4: valence repair, atoms in order
    for (int i = 0; i < n; ++i) {
        int val = 0;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) val += __popc(A1[i * MOL_W + w]) + __popc(A2[i * MOL_W + w]) + __popc(A3[i * MOL_W + w]);
        const int cap = (int)(el[i] >> 24);
        if (val <= cap) continue;                   // wave-uniform
        double key[MOL_K];
        int ord[MOL_K];
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int j = lane + 64 * k, w = i * MOL_W + (j >> 5), s = j & 31;
            ord[k] = (int)((A1[w] >> s) & 1u) + (int)((A2[w] >> s) & 1u) + (int)((A3[w] >> s) & 1u);
            key[k] = ord[k] ? mol_d2(p, i, j) : -1.0;
        }
        while (val > cap) {
            int o = 0, bj = -1;
            double bd = -1.0;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k)
                if (ord[k] > o || (ord[k] == o && ord[k] && key[k] >= bd)) {
                    o = ord[k];
                    bd = key[k];
                    bj = lane + 64 * k;
                }
            wave_argmax(o, bd, bj);
            if (o < 2) break;                       // cannot happen: step 2 left degree <= cap
#pragma unroll
            for (int k = 0; k < MOL_K; ++k)
                if (bj == lane + 64 * k) --ord[k];
            if (lane == 0) clear_pair(o == 3 ? A3 : A2, i, bj);
            --val;
        }
        __syncthreads();
    }
    // steps 5 and 6, the per-atom outputs, and the bonds in (i, j) order into the ligand's part of the scratch list
    int n_frags, lo, invalid, total;
    mol_fragments_out(A1, A2, A3, label, fsize, n, lane, a0, [&](int k, int val) { return val == 0 || val > allowed[cls[k]]; }, valence, frag,
                      tmp_ij + (size_t)6 * a0, tmp_order + (size_t)3 * a0, n_frags, lo, invalid, total);
    st = __any(st != 0) ? MOL_BAD_ATOM : 0;
    if (lane == 0) {
        n_bonds[b] = total;
        summary[b * 4] = total;
        summary[b * 4 + 1] = n_frags;
        summary[b * 4 + 2] = lo;
        summary[b * 4 + 3] = invalid;
        status[b] = st;
    }
}

// one wave per ligand: its bonds from the scratch list to bond_ptr
__global__ void __launch_bounds__(64)
k_mol_gather(const int *__restrict__ lig_ptr, const int *__restrict__ tmp_ij, const int *__restrict__ tmp_order,
             const int *__restrict__ bond_ptr, int cap_bonds, int *__restrict__ bond_ij, int *__restrict__ bond_order,
             int *__restrict__ status) {
    const int b = blockIdx.x;
    const int p0 = bond_ptr[b], p1 = bond_ptr[b + 1];
    if (p1 == p0) return;                           // also every ligand that was left out: its a0 is never used
    if (p1 > cap_bonds) {
        if (threadIdx.x == 0) status[b] |= MOL_CAPACITY;
        return;
    }
    const size_t src = (size_t)3 * lig_ptr[b];
    for (int k = threadIdx.x; k < p1 - p0; k += 64) {
        bond_ij[(size_t)(p0 + k) * 2] = tmp_ij[(src + k) * 2];
        bond_ij[(size_t)(p0 + k) * 2 + 1] = tmp_ij[(src + k) * 2 + 1];
        bond_order[p0 + k] = tmp_order[src + k];
    }
}

// ---- 2. SDF text ---------------------------------------------------------------------------------------------------------
// Every line of a MOL V2000 block has a fixed width once the coordinates fit "%10.4f", so a block's size follows from its atom
// and bond counts: sizes, scan, then every line is written straight to its place (no line slots to compact).
constexpr int SDF_HEAD = 25, SDF_COUNTS = 40, SDF_ATOM = 70, SDF_BOND = 13, SDF_TAIL = 12;

// width of "%.4f" of a finite value, or 99 if it cannot be printed here
__device__ __forceinline__ int width_f4(float v) {
    const unsigned bits = __float_as_uint(v);
    unsigned long long N;
    if (!fixed_scaled<4>(bits, N)) return 99;
    int w = (bits >> 31) + 6;
    for (unsigned long long ip = N / 10000ull; ip >= 10ull; ip /= 10ull) ++w;
    return w;
}

__device__ __forceinline__ void put_int3(char *dst, int v) {     // "%3d" of 0 .. 999
    dst[0] = v >= 100 ? (char)('0' + v / 100) : ' ';
    dst[1] = v >= 10 ? (char)('0' + (v / 10) % 10) : ' ';
    dst[2] = (char)('0' + v % 10);
}

__device__ __forceinline__ void put_text(char *dst, const char *s, int n) {
    for (int k = 0; k < n; ++k) dst[k] = s[k];
}

// one workgroup per ligand: flags, the largest fragment, atoms and bonds of the block -> info [b] = {flags, atoms, bonds, rank}
__global__ void __launch_bounds__(256)
k_sdf_size(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F,
           const int *__restrict__ frag, const int *__restrict__ bond_ij, const int *__restrict__ bond_ptr, int cap_bonds,
           const int *__restrict__ mol_status, int largest_only, int *__restrict__ info, long long *__restrict__ lig_len) {
    __shared__ int fsize[MOL_MAX];
    __shared__ int red[4];
    __shared__ int best;
    const int b = blockIdx.x, tid = threadIdx.x;
    int a0, a1;
    const bool ok = mol_segment(lig_ptr, b, n_atoms, a0, a1);
    const int n = a1 - a0;
    int flags = 0;
    if (!ok || n > MOL_MAX || (mol_status[b] & (MOL_CAPACITY | MOL_BAD_SEGMENT))) flags = SDF_NO_MOLECULE;
    int p0 = 0, p1 = 0;
    if (!flags) {
        p0 = bond_ptr[b];
        p1 = bond_ptr[b + 1];
        // not mol_bond_range: a ligand without bonds has a block (atoms only) even where its empty range lies beyond cap_bonds
        if (p0 < 0 || p1 < p0 || (p1 > p0 && p1 > cap_bonds) || p1 - p0 > 3 * MOL_MAX) flags = SDF_NO_MOLECULE;
    }
    if (flags) {                                    // block-uniform
        if (tid == 0) {
            info[b * 4] = flags;
            info[b * 4 + 1] = info[b * 4 + 2] = info[b * 4 + 3] = 0;
            lig_len[b] = 0;
        }
        return;
    }
    fsize[tid] = 0;
    if (tid < 4) red[tid] = 0;
    if (tid == 0) best = 0;
    __syncthreads();
    int f = -1;
    if (tid < n) {
        const size_t g = (size_t)(a0 + tid);
        for (int c = 0; c < 3; ++c) {
            const float v = pos[g * 3 + c];
            if (!finite_f(v)) flags |= SDF_NONFINITE;
            else if (width_f4(v) > 10) flags |= SDF_WIDE;
        }
        f = frag[g];
        const int e = elem[g];
        if (f < 0 || f >= n || e < 0 || e >= F) flags |= SDF_NO_MOLECULE;
        else atomicAdd(&fsize[f], 1);
        if (flags) atomicOr(&red[0], flags);
    }
    __syncthreads();
    flags = red[0];
    if (largest_only && !flags) {                   // most atoms, then the lowest rank
        const int key = tid < n && fsize[tid] ? frag_key(fsize[tid], tid) : 0;
        atomicMax(&best, key);
        __syncthreads();
        const int rank = frag_key_rank(best);
        int nb = 0;
        for (int k = p0 + tid; k < p1; k += 256) {
            const int i = bond_ij[(size_t)k * 2] - a0;
            nb += i >= 0 && i < n && frag[a0 + i] == rank;
        }
        if (nb) atomicAdd(&red[1], nb);
        __syncthreads();
        if (tid == 0) {
            const int na = best / MOL_MAX;
            info[b * 4] = 0;
            info[b * 4 + 1] = na;
            info[b * 4 + 2] = red[1];
            info[b * 4 + 3] = rank;
            lig_len[b] = SDF_HEAD + SDF_COUNTS + SDF_TAIL + (long long)SDF_ATOM * na + (long long)SDF_BOND * red[1];
        }
        return;
    }
    if (tid == 0) {
        info[b * 4] = flags;
        info[b * 4 + 1] = flags ? 0 : n;
        info[b * 4 + 2] = flags ? 0 : p1 - p0;
        info[b * 4 + 3] = -1;                       // every fragment
        lig_len[b] = flags ? 0 : SDF_HEAD + SDF_COUNTS + SDF_TAIL + (long long)SDF_ATOM * n + (long long)SDF_BOND * (p1 - p0);
    }
}

// one workgroup per ligand: the block, every line at its place
__global__ void __launch_bounds__(256)
k_sdf_write(const float *__restrict__ pos, const int *__restrict__ lig_ptr, const int *__restrict__ elem,
            const unsigned *__restrict__ symbols, const int *__restrict__ frag, const int *__restrict__ bond_ij,
            const int *__restrict__ bond_order, const int *__restrict__ bond_ptr, const int *__restrict__ info,
            const long long *__restrict__ text_ptr, long long capacity, char *__restrict__ text, int *__restrict__ status) {
    __shared__ int newidx[MOL_MAX];                 // 1-based number of the atom in the block, 0 = not in it
    __shared__ int part[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int flags = info[b * 4], na = info[b * 4 + 1], nb = info[b * 4 + 2], rank = info[b * 4 + 3];
    const long long t0 = text_ptr[b], t1 = text_ptr[b + 1];
    if (flags || t1 > capacity) {                   // block-uniform
        if (tid == 0) status[b] = flags | (!flags && t1 > capacity ? SDF_CAPACITY : 0);
        return;
    }
    if (tid == 0) status[b] = 0;
    const int a0 = lig_ptr[b], n = lig_ptr[b + 1] - a0;        // checked by k_sdf_size: flags would be set otherwise
    const bool keep = tid < n && (rank < 0 || frag[a0 + tid] == rank);
    int total;
    int ex = wave_exclusive(keep ? 1 : 0, lane, total);
    if (lane == 0) part[w] = total;
    __syncthreads();
    for (int k = 0; k < w; ++k) ex += part[k];
    newidx[tid] = keep ? ex + 1 : 0;
    __syncthreads();
    char *blk = text + t0;
    if (tid == 0) {
        put_text(blk, "\n  kpd_hip           3D\n\n", SDF_HEAD);
        char *c = blk + SDF_HEAD;
        put_int3(c, na);
        put_int3(c + 3, nb);
        put_text(c + 6, "  0  0  0  0  0  0  0  0999 V2000\n", SDF_COUNTS - 6);
        put_text(blk + SDF_HEAD + SDF_COUNTS + (long long)SDF_ATOM * na + (long long)SDF_BOND * nb, "M  END\n$$$$\n", SDF_TAIL);
    }
    if (keep) {
        char *line = blk + SDF_HEAD + SDF_COUNTS + (long long)SDF_ATOM * ex;
        const size_t g = (size_t)(a0 + tid);
        for (int c = 0; c < 3; ++c) {
            char num[32];
            const int len = format_fixed<4>(pos[g * 3 + c], num);      // 6 .. 10: k_sdf_size saw to it
            for (int k = 0; k < 10; ++k) line[c * 10 + k] = k < 10 - len ? ' ' : num[k - (10 - len)];
        }
        line[30] = ' ';
        const unsigned sym = symbols[elem[g]];       // "%-3s": at most three bytes of the symbol, blank padded
        bool end = false;
        for (int k = 0; k < 3; ++k) {
            const char ch = (char)((sym >> (8 * k)) & 0xff);
            end = end || !ch;
            line[31 + k] = end ? ' ' : ch;
        }
        put_text(line + 34, " 0  0  0  0  0  0  0  0  0  0  0  0\n", SDF_ATOM - 34);
    }
    const int p0 = bond_ptr[b], p1 = bond_ptr[b + 1];
    if (rank < 0) {                                 // every bond, in place
        for (int k = tid; k < p1 - p0; k += 256) {
            char *line = blk + SDF_HEAD + SDF_COUNTS + (long long)SDF_ATOM * na + (long long)SDF_BOND * k;
            const int i = bond_ij[(size_t)(p0 + k) * 2] - a0, j = bond_ij[(size_t)(p0 + k) * 2 + 1] - a0;
            put_int3(line, i >= 0 && i < n ? newidx[i] : 0);
            put_int3(line + 3, j >= 0 && j < n ? newidx[j] : 0);
            put_int3(line + 6, bond_order[p0 + k] & 7);
            put_text(line + 9, "  0\n", 4);
        }
        return;
    }
    int done = 0;                                   // bonds of the fragment, in order; trip count block-uniform
    for (int base = p0; base < p1; base += 256) {
        const int k = base + tid;
        int i = -1, j = -1;
        if (k < p1) {
            i = bond_ij[(size_t)k * 2] - a0;
            j = bond_ij[(size_t)k * 2 + 1] - a0;
        }
        const bool in = i >= 0 && i < n && j >= 0 && j < n && newidx[i] && newidx[j];
        int at = wave_exclusive(in ? 1 : 0, lane, total);
        __syncthreads();
        if (lane == 0) part[w] = total;
        __syncthreads();
        int all = 0;
        for (int q = 0; q < 4; ++q) {
            if (q < w) at += part[q];
            all += part[q];
        }
        if (in && done + at < nb) {
            char *line = blk + SDF_HEAD + SDF_COUNTS + (long long)SDF_ATOM * na + (long long)SDF_BOND * (done + at);
            put_int3(line, newidx[i]);
            put_int3(line + 3, newidx[j]);
            put_int3(line + 6, bond_order[k] & 7);
            put_text(line + 9, "  0\n", 4);
        }
        done += all;
    }
}

}  // namespace kpd

using namespace kpd;

// the bond list before compaction (3 n rows of (i, j) and of the order), bonds per ligand
struct MolScratch {
    int n_atoms, B;
    int *tmp_ij = nullptr, *tmp_order = nullptr, *n_bonds = nullptr;
    void operator()(Carve &c) { c(tmp_ij, (size_t)n_atoms * 6); c(tmp_order, (size_t)n_atoms * 3); c(n_bonds, B); }
};

extern "C" int64_t kpd_mol_scratch_bytes(int32_t n_atoms, int32_t B) {
    if (n_atoms < 0 || B < 0) return -1;
    MolScratch s{n_atoms, B};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_mol_perceive(const float *pos, const float *feat, const int32_t *lig_ptr, int32_t n_atoms, int32_t B,
                                       int32_t F, const int32_t *z, const int32_t *allowed, int32_t cap_bonds, int32_t *elem,
                                       int32_t *valence, int32_t *frag, int32_t *bond_ij, int32_t *bond_order, int32_t *bond_ptr,
                                       int32_t *summary, int32_t *status, void *scratch, void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0, KPD_ERR_INVALID, "n_atoms=%d B=%d F=%d cap_bonds=%d", n_atoms, B, F,
                cap_bonds);
    KPD_REQUIRE(lig_ptr && z && allowed && bond_ptr && scratch, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (pos && feat && elem && valence && frag), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (summary && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || (bond_ij && bond_order), KPD_ERR_INVALID, "null bond buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    MolScratch s{n_atoms, B};
    carve_raw(static_cast<char *>(scratch), s);
    int *tmp_ij = s.tmp_ij, *tmp_order = s.tmp_order, *n_bonds = s.n_bonds;
    if (n_atoms) {                                  // atoms of a ligand that is left out (and of none) read -1
        KPD_HIP(hipMemsetAsync(elem, 0xff, (size_t)n_atoms * 4, st));
        KPD_HIP(hipMemsetAsync(valence, 0xff, (size_t)n_atoms * 4, st));
        KPD_HIP(hipMemsetAsync(frag, 0xff, (size_t)n_atoms * 4, st));
    }
    if (B) {
        hipLaunchKernelGGL(k_mol_perceive, dim3(B), dim3(64), 0, st, pos, feat, lig_ptr, n_atoms, F, z, allowed, elem, valence, frag, tmp_ij,
                           tmp_order, n_bonds, summary, status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, n_bonds, B, bond_ptr));
    if (B) {
        hipLaunchKernelGGL(k_mol_gather, dim3(B), dim3(64), 0, st, lig_ptr, tmp_ij, tmp_order, bond_ptr, cap_bonds, bond_ij, bond_order,
                           status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}

// {flags, atoms, bonds, rank} and the bytes of every ligand's block
struct SdfScratch {
    int B;
    int *info = nullptr;
    long long *lig_len = nullptr;
    void operator()(Carve &c) { c(info, (size_t)B * 4); c(lig_len, B); }
};

extern "C" int64_t kpd_sdf_scratch_bytes(int32_t n_atoms, int32_t B) {
    if (n_atoms < 0 || B < 0) return -1;
    SdfScratch s{B};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_sdf_emit(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem,
                                   int32_t F, const uint32_t *symbols, const int32_t *frag, const int32_t *bond_ij,
                                   const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status,
                                   int32_t largest_only, uint8_t *text, int64_t capacity, int64_t *text_ptr, int32_t *status,
                                   void *scratch, void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0 && capacity >= 0, KPD_ERR_INVALID,
                "n_atoms=%d B=%d F=%d cap_bonds=%d capacity=%lld", n_atoms, B, F, cap_bonds, (long long)capacity);
    KPD_REQUIRE(lig_ptr && symbols && bond_ptr && text_ptr && scratch, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (pos && elem && frag), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (mol_status && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || (bond_ij && bond_order), KPD_ERR_INVALID, "null bond buffer");
    KPD_REQUIRE(!capacity || text, KPD_ERR_INVALID, "null text buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SdfScratch s{B};
    carve_raw(static_cast<char *>(scratch), s);
    int *info = s.info;
    long long *lig_len = s.lig_len;
    if (B) {
        hipLaunchKernelGGL(k_sdf_size, dim3(B), dim3(256), 0, st, pos, lig_ptr, n_atoms, elem, F, frag, bond_ij, bond_ptr, cap_bonds,
                           mol_status, largest_only, info, lig_len);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, lig_len, B, reinterpret_cast<long long *>(text_ptr)));
    if (B) {
        hipLaunchKernelGGL(k_sdf_write, dim3(B), dim3(256), 0, st, pos, lig_ptr, elem, symbols, frag, bond_ij, bond_order, bond_ptr, info,
                           reinterpret_cast<const long long *>(text_ptr), (long long)capacity, reinterpret_cast<char *>(text), status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
