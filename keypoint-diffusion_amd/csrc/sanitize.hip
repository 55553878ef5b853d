// Sanitisation of perceived ligands on the device: ring bonds, planar rings, a Kekule assignment, aromatic rings, implicit
// hydrogens, donor / acceptor flags, validity and the per-molecule descriptors.  Stands where upstream calls Chem.SanitizeMol
// and MoleculeProperties on every sample (analysis/metrics.py).  RDKit's rules cannot be restated: include/kpd.h defines the rule.
// It reads the bond graph kpd_mol_perceive left on the device and writes a second set of bond orders next to it.
// One wave per ligand, as k_mol_perceive and k_mol_keys: positions, the adjacency bit matrix and the neighbour lists live in
// LDS.  A neighbour entry is one word: the partner, the length-class order, the row of the bond and the flags the steps add.
// Parallel over lanes: bond validation, the ring test of every bond (vina_walk of vina_core.h), the cycles by start atom (a
// depth-first walk whose path and iterators are packed into two registers), the planarity windows and the aromatic count by
// cycle, everything per atom.  The matching of one component of the candidate graph is serial inside the lane that owns the
// component's lowest atom: at most 24 atoms, renumbered, so that every set is a 32-bit mask and the stack of the alternating-
// path search packs into two 64-bit registers.  Integer LDS atomics only (all of them commutative), no float atomics, no
// scratch memory.  All geometry is fp64 with every product and sum rounded once: the Makefile compiles this file with
// -ffp-contract=off (the __d*_rn functions of the HIP headers are plain operators, which the default setting may fuse).
// The front end (entry check, atom staging, the scope S, the bond loop with its unordered row contract), the status bits, the six
// atom flags that are written out and the fp64 vectors are those of molgraph_core.h, shared with k_mol_keys and k_mol_add_hs.
#include "common.h"
#include "molgraph_core.h"
#include "vina_core.h"

namespace kpd {

typedef unsigned long long u64;

enum : int { SAN_MAX_CYCLES = 64, SAN_MAX_COMPONENT = 24 };
// a neighbour entry: partner | order << 8 | local bond row << 10 | flags
enum : unsigned { NB_RING = 1u << 20, NB_PLANAR = 1u << 21, NB_GEDGE = 1u << 22, NB_MATCHED = 1u << 23, NB_AROMATIC = 1u << 24 };
// the working atom flags, above the six of molgraph_core.h that are written out
enum : unsigned { AT_PLANAR = 1u << 8, AT_ING = 1u << 9, AT_MATCHED = 1u << 10, AT_LONE_PAIR = 1u << 11, AT_TOO_LARGE = 1u << 12 };

__device__ __forceinline__ int normal_valence(int z, int val) {
    switch (z) {
    case 6:
    case 14: return 4;
    case 7:
    case 5:
    case 33: return 3;
    case 8: return 2;
    case 1:
    case 9:
    case 17:
    case 35:
    case 53: return 1;
    case 16: return val <= 2 ? 2 : val <= 4 ? 4 : 6;
    case 15: return val <= 3 ? 3 : 5;
    default: return 0;
    }
}

__device__ __forceinline__ int find_slot(const unsigned *nb, int dg, int i, int j) {
    int at = -1;
#pragma unroll
    for (int s = 0; s < MOL_DEG; ++s)
        if (s < dg && (int)(nb[i * MOL_DEG + s] & 0xffu) == j) at = s;
    return at;
}

// order_k of a neighbour entry between atoms with the flags fi and fj
__device__ __forceinline__ int order_k_of(unsigned e, unsigned fi, unsigned fj) {
    if ((e & NB_PLANAR) && !((fi | fj) & AT_TOO_LARGE)) return (e & NB_MATCHED) ? 2 : 1;
    return (int)((e >> 8) & 3u);
}

// step 2: all windows of four consecutive atoms of the cycle (atom t in byte t of `path`) pass the 20 degree test
__device__ bool cycle_planar(const float *p, u64 path, int len) {
    for (int t = 0; t < len; ++t) {
        V3 q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int at = t + k;
            if (at >= len) at -= len;
            q[k] = vat(p, (int)((path >> (8 * at)) & 0xffull));
        }
        const V3 u = vsub(q[1], q[0]), v = vsub(q[2], q[1]), w = vsub(q[3], q[2]);
        const V3 n1 = vcross(u, v), n2 = vcross(v, w);
        const double qq = __dmul_rn(vdot(n1, n1), vdot(n2, n2));
        if (!(qq >= 1e-12 && vdot(n1, n2) >= __dmul_rn(0.9396926207859084, __dsqrt_rn(qq)))) return false;
    }
    return true;
}

// ---- the matching of one component, in local numbers 0 .. 23; lg / mate are the lane's own rows in LDS, ladj is by atom ----------
// Is there a simple alternating path from the free atom v that ends at a free atom, or after an even number of bonds at a
// matched atom that is not in `taken`?  If so the matching is turned over along it.  Walks every simple alternating path (exact
// with odd rings); x_d of the stack in bits 5 d of xs, one more than the last partner tried there in bits 5 d of lasts.
__device__ bool alternating_path(int v, unsigned avail, unsigned taken, const unsigned *ladj, const unsigned char *lg, signed char *mate) {
    unsigned visited = 1u << v;
    u64 xs = (u64)v, lasts = 0;
    int depth = 0;
    for (;;) {
        const int sh = 5 * depth;
        const int x = (int)((xs >> sh) & 31ull), last = (int)((lasts >> sh) & 31ull);
        const unsigned cand = ladj[lg[x]] & avail & ~visited & ~((1u << last) - 1u);
        if (!cand) {
            if (depth == 0) return false;
            visited &= ~((1u << x) | (1u << mate[x]));
            xs &= ~(31ull << sh);
            lasts &= ~(31ull << sh);
            --depth;
            continue;
        }
        const int y = __ffs(cand) - 1;
        lasts = (lasts & ~(31ull << sh)) | ((u64)(y + 1) << sh);
        const int m = mate[y];
        if (m >= 0 && ((visited >> m) & 1u)) continue;
        if (m < 0 || !((taken >> m) & 1u)) {
            if (m >= 0) mate[m] = -1;
            int yd = y;
            for (int d = depth; d >= 0; --d) {
                const int xd = (int)((xs >> (5 * d)) & 31ull), old = mate[xd];
                mate[xd] = (signed char)yd;
                mate[yd] = (signed char)xd;
                yd = old;
            }
            return true;
        }
        visited |= (1u << y) | (1u << m);
        ++depth;
        xs = (xs & ~(31ull << (sh + 5))) | ((u64)m << (sh + 5));
        lasts &= ~(31ull << (sh + 5));
    }
}

// (matched carbons, matched atoms) of an optimal matching of the graph on `avail`: atoms in order, carbons (cm) first
__device__ void greedy_value(unsigned avail, unsigned cm, const unsigned *ladj, const unsigned char *lg, signed char *mate, int &nc, int &na) {
    for (unsigned bits = avail; bits; bits &= bits - 1) mate[__ffs(bits) - 1] = -1;
    unsigned taken = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (unsigned todo = avail & (pass ? ~cm : cm); todo; todo &= todo - 1) {
            const int v = __ffs(todo) - 1;
            if (mate[v] >= 0 || alternating_path(v, avail, taken, ladj, lg, mate)) taken |= 1u << v;
        }
    nc = __popc(taken & cm);
    na = __popc(taken);
}

// ---- one wave per ligand -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_mol_sanitize(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F,
               const int *__restrict__ zs, const int *__restrict__ allowed, const double *__restrict__ mass, double mass_h,
               const int *__restrict__ frag, const int *__restrict__ bond_ij, const int *__restrict__ bond_order,
               const int *__restrict__ bond_ptr, int cap_bonds, const int *__restrict__ mol_status, int largest_only,
               int *__restrict__ order_k, int *__restrict__ bond_flags, int *__restrict__ valence_k, int *__restrict__ atom_h,
               int *__restrict__ atom_flags, int *__restrict__ desc_i, double *__restrict__ desc_f, int *__restrict__ valid,
               int *__restrict__ status) {
    __shared__ float p[MOL_MAX * 3];
    __shared__ unsigned adj[MOL_MAX * MOL_W];       // bonded, both ends in S
    __shared__ unsigned nb[MOL_MAX * MOL_DEG];
    __shared__ unsigned aflag[MOL_MAX];
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];                  // atoms per fragment; later atoms per component of G, at its lowest atom
    __shared__ unsigned char label[MOL_MAX];
    __shared__ unsigned char zv[MOL_MAX];           // Z; 0 for a Z outside 0 .. 255, which no rule here knows either
    __shared__ unsigned char vk[MOL_MAX];           // valence_k
    __shared__ unsigned char hd[MOL_MAX];           // heavy degree
    __shared__ u64 cyc[SAN_MAX_CYCLES];             // atom t in byte t, the length in byte 7
    __shared__ unsigned ladj[MOL_MAX];                          // the G neighbours of an atom as a mask of local numbers
    __shared__ __align__(8) signed char mate[64 * SAN_MAX_COMPONENT];
    __shared__ unsigned char lg[64 * SAN_MAX_COMPONENT];        // local -> atom, of the component a lane works on
    __shared__ unsigned char gl[MOL_MAX];                       // atom -> local
    __shared__ unsigned inS[MOL_W];
    __shared__ int bad, ncyc, stat;
    const int b = blockIdx.x, lane = threadIdx.x;
    const MolEntry en = mol_entry(lig_ptr, b, n_atoms, bond_ptr, cap_bonds, mol_status);
    const int a0 = en.a0, n = en.n, p0 = en.p0, p1 = en.p1;
    bool ok = en.ok;
    int fr_of[MOL_K] = {-1, -1, -1, -1};
    if (ok) {                                       // wave-uniform, as every `ok` below
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            deg[a] = 0;
            fsize[a] = 0;
            aflag[a] = 0;
            label[a] = (unsigned char)a;
            for (int w = 0; w < MOL_W; ++w) adj[a * MOL_W + w] = 0;
        }
        if (lane == 0) bad = ncyc = stat = 0;
        __syncthreads();
        mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int, int a, size_t g, int z) {
            zv[a] = mol_z_byte(z);
            p[a * 3] = pos[g * 3];
            p[a * 3 + 1] = pos[g * 3 + 1];
            p[a * 3 + 2] = pos[g * 3 + 2];
            return true;
        });
        __syncthreads();
        ok = !bad;
    }
    int nS = 0, n_frag = 1;
    if (ok) {
        const MolScope sc = mol_scope(fsize, fr_of, n, lane, largest_only, inS);
        nS = sc.nS;
        if (!largest_only) n_frag = sc.n_frag;
        // bonds with both ends in S: adjacency bits and neighbour entries
        mol_bond_graph<false>(bond_ij, p0, p1, a0, n, lane, inS, adj, MOL_W, deg, (int *)nullptr, nb, &bad,
                              [bond_order](int k) { return bond_order[k]; }, 3, [](int row, int o) { return (unsigned)o << 8 | (unsigned)row << 10; });
        __syncthreads();
        ok = !bad && nS > 0;
    }
    if (!ok) {                                      // no molecule: the rows keep the orders they came with
        if (en.range_ok)
            for (int k = p0 + lane; k < p1; k += 64) order_k[k] = bond_order[k];
        if (lane < 10) desc_i[b * 10 + lane] = 0;
        if (lane < 2) desc_f[b * 2 + lane] = 0.0;
        if (lane == 0) {
            valid[b] = 0;
            status[b] = SAN_NO_MOLECULE;
        }
        return;
    }
    bool in[MOL_K];
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        in[k] = in_scope(inS, a);
    }
    // ---- step 1: ring bonds (the ends stay connected without the bond), the 5- and 6-cycles by start atom
    for (int k = p0 + lane; k < p1; k += 64) {
        const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0;
        if (!both_in_scope(inS, i, j)) continue;
        unsigned vis[MOL_W];
        if (!vina_walk<true>(adj, MOL_W, i, j, vis)) continue;
        atomicOr(&nb[i * MOL_DEG + find_slot(nb, deg[i], i, j)], NB_RING);
        atomicOr(&nb[j * MOL_DEG + find_slot(nb, deg[j], j, i)], NB_RING);
        atomicOr(&aflag[i], AT_RING);
        atomicOr(&aflag[j], AT_RING);
    }
    for (int k = 0; k < MOL_K; ++k) {
        const int s = lane + 64 * k;
        if (s >= n || !in_scope(inS, s)) continue;
        u64 path = (u64)s;
        unsigned it = 0;                            // the next neighbour slot of the atom at place d in bits 3 d
        int depth = 1;
        for (;;) {
            const int cur = (int)((path >> (8 * (depth - 1))) & 0xffull), slot = (int)((it >> (3 * (depth - 1))) & 7u);
            if (slot >= deg[cur]) {
                if (--depth == 0) break;
                path &= ~(0xffull << (8 * depth));
                continue;
            }
            it += 1u << (3 * (depth - 1));
            const int v = (int)(nb[cur * MOL_DEG + slot] & 0xffu);
            if (v <= s) continue;
            bool on = false;
#pragma unroll
            for (int d = 1; d < 6; ++d) on = on || (d < depth && (int)((path >> (8 * d)) & 0xffull) == v);
            if (on) continue;
            path |= (u64)v << (8 * depth);
            ++depth;
            if (depth >= 5 && ((adj[v * MOL_W + (s >> 5)] >> (s & 31)) & 1u) && (int)((path >> 8) & 0xffull) < v) {
                const int at = atomicAdd(&ncyc, 1);
                if (at < SAN_MAX_CYCLES) cyc[at] = path | (u64)depth << 56;
            }
            if (depth < 6) {
                it &= ~(7u << (3 * (depth - 1)));
            } else {
                --depth;
                path &= ~(0xffull << (8 * depth));
            }
        }
    }
    __syncthreads();
    const int n_cycles = ncyc;
    const bool many = n_cycles > SAN_MAX_CYCLES;
    int n_arom_rings = 0, len = 0;
    u64 mine = 0;                                   // the lane's cycle: lane c owns cycle c in steps 2 and 4
    bool flat = false;
    if (!many) {                                    // wave-uniform
        // ---- step 2: planar cycles, a lane per cycle (the order of the cycles in the list shows in no output)
        mine = lane < n_cycles ? cyc[lane] : 0ull;
        len = (int)(mine >> 56);
        flat = lane < n_cycles && cycle_planar(p, mine, len);
        if (flat)
            for (int t = 0; t < len; ++t) {
                const int x = (int)((mine >> (8 * t)) & 0xffull), y = (int)((mine >> (8 * (t + 1 == len ? 0 : t + 1))) & 0xffull);
                atomicOr(&nb[x * MOL_DEG + find_slot(nb, deg[x], x, y)], NB_PLANAR);
                atomicOr(&nb[y * MOL_DEG + find_slot(nb, deg[y], y, x)], NB_PLANAR);
                atomicOr(&aflag[x], AT_PLANAR);
            }
        __syncthreads();
        // ---- step 3: the atoms and edges of G, its components, the matching of every component
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            fsize[a] = 0;                           // from here on the sizes of the components of G
            if (a >= n || !(aflag[a] & AT_PLANAR) || (zv[a] != 6 && zv[a] != 7)) continue;
            int room = zv[a] == 6 ? 4 : 3;
            for (int s = 0; s < deg[a]; ++s) {
                const unsigned e = nb[a * MOL_DEG + s];
                room -= (e & NB_PLANAR) ? 1 : (int)((e >> 8) & 3u);
            }
            if (room >= 1) aflag[a] |= AT_ING;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (a >= n || !(aflag[a] & AT_ING)) continue;
            const unsigned ra = element_row(zv[a]) & 0xffu;
            for (int s = 0; s < deg[a]; ++s) {
                const unsigned e = nb[a * MOL_DEG + s];
                const int j = (int)(e & 0xffu);
                if ((e & NB_PLANAR) && (aflag[j] & AT_ING) && within(mol_d2(p, a, j), ra, element_row(zv[j]) & 0xffu, -3))
                    nb[a * MOL_DEG + s] = e | NB_GEDGE;
            }
        }
        __syncthreads();
        for (;;) {                                  // labels: the lowest atom of every component of G
            bool changed = false;
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                if (a >= n || !(aflag[a] & AT_ING)) continue;
                int l = label[a];
                const int before = l;
                for (int s = 0; s < deg[a]; ++s) {
                    const unsigned e = nb[a * MOL_DEG + s];
                    if (e & NB_GEDGE) l = min(l, label[e & 0xffu]);
                }
                l = min(l, label[l]);
                if (l != before) {
                    label[a] = (unsigned char)l;
                    changed = true;
                }
            }
            __syncthreads();
            if (!__any(changed)) break;             // wave-uniform
        }
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (a < n && (aflag[a] & AT_ING)) atomicAdd(&fsize[label[a]], 1);
        }
        __syncthreads();
        signed char *my_mate = mate + lane * SAN_MAX_COMPONENT;
        unsigned char *my_lg = lg + lane * SAN_MAX_COMPONENT;
        for (int k = 0; k < MOL_K; ++k) {
            const int root = lane + 64 * k;
            if (root >= n || !(aflag[root] & AT_ING) || label[root] != root || fsize[root] < 2) continue;
            const int size = fsize[root];
            if (size > SAN_MAX_COMPONENT) {         // the component keeps its length-class orders; its carbons are unsatisfied
                atomicOr(&stat, SAN_COMPONENT_TOO_LARGE);
                for (int a = root; a < n; ++a)
                    if ((aflag[a] & AT_ING) && label[a] == root) atomicOr(&aflag[a], AT_TOO_LARGE | (zv[a] == 6 ? AT_UNSATISFIED : 0u));
                continue;
            }
            unsigned cm = 0;
            for (int a = root, c = 0; a < n && c < size; ++a)
                if ((aflag[a] & AT_ING) && label[a] == root) {
                    my_lg[c] = (unsigned char)a;
                    gl[a] = (unsigned char)c;
                    if (zv[a] == 6) cm |= 1u << c;
                    ++c;
                }
            for (int u = 0; u < size; ++u) {
                const int g = my_lg[u];
                unsigned m = 0;
                for (int s = 0; s < deg[g]; ++s) {
                    const unsigned e = nb[g * MOL_DEG + s];
                    if (e & NB_GEDGE) m |= 1u << gl[e & 0xffu];
                }
                ladj[g] = m;
            }
            const unsigned all = size == 32 ? ~0u : (1u << size) - 1u;
            int opt_c, opt_a;
            greedy_value(all, cm, ladj, my_lg, my_mate, opt_c, opt_a);
            // the lexicographic choice: the bonds in row order; one is taken iff an optimal matching holds it and those taken before.
            // `mate` always holds such an optimal matching, so a bond that is in it needs no search
            unsigned avail = all;
            int have_c = 0, have_a = 0, last = -1;
            while (have_a < opt_a) {
                int best = 1 << 20, bu = -1, bv = -1;
                for (unsigned bits = avail; bits; bits &= bits - 1) {
                    const int u = __ffs(bits) - 1, g = my_lg[u];
                    for (int s = 0; s < deg[g]; ++s) {
                        const unsigned e = nb[g * MOL_DEG + s];
                        if (!(e & NB_GEDGE)) continue;
                        const int v = gl[e & 0xffu], row = (int)((e >> 10) & 0x3ffu);
                        if (v > u && ((avail >> v) & 1u) && row > last && row < best) {
                            best = row;
                            bu = u;
                            bv = v;
                        }
                    }
                }
                if (bu < 0) break;
                last = best;
                const unsigned rest = avail & ~((1u << bu) | (1u << bv));
                const int add_c = (int)((cm >> bu) & 1u) + (int)((cm >> bv) & 1u);
                if (my_mate[bu] != bv) {
                    u64 keep0, keep1, keep2;        // the 24 mates of the matching at hand
                    __builtin_memcpy(&keep0, my_mate, 8);
                    __builtin_memcpy(&keep1, my_mate + 8, 8);
                    __builtin_memcpy(&keep2, my_mate + 16, 8);
                    int c, a;
                    greedy_value(rest, cm, ladj, my_lg, my_mate, c, a);
                    if (c + have_c + add_c != opt_c || a + have_a + 2 != opt_a) {
                        __builtin_memcpy(my_mate, &keep0, 8);
                        __builtin_memcpy(my_mate + 8, &keep1, 8);
                        __builtin_memcpy(my_mate + 16, &keep2, 8);
                        continue;
                    }
                    my_mate[bu] = (signed char)bv;
                    my_mate[bv] = (signed char)bu;
                }
                have_c += add_c;
                have_a += 2;
                avail = rest;
                const int gu = my_lg[bu], gv = my_lg[bv];
                nb[gu * MOL_DEG + find_slot(nb, deg[gu], gu, gv)] |= NB_MATCHED;
                nb[gv * MOL_DEG + find_slot(nb, deg[gv], gv, gu)] |= NB_MATCHED;
                atomicOr(&aflag[gu], AT_MATCHED);
                atomicOr(&aflag[gv], AT_MATCHED);
            }
            for (int u = 0; u < size; ++u) {
                const int g = my_lg[u];
                if (zv[g] == 6 && !(aflag[g] & AT_MATCHED)) atomicOr(&aflag[g], AT_UNSATISFIED);
            }
        }
        __syncthreads();
    }
    // ---- step 5 first (step 4 reads the valences): valence_k, the heavy degree, the lone-pair nitrogens of planar rings
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        if (a >= n || !in[k]) continue;
        const unsigned fa = aflag[a];
        int v = 0, n_heavy_nb = 0;
        for (int s = 0; s < deg[a]; ++s) {
            const unsigned e = nb[a * MOL_DEG + s];
            const int j = (int)(e & 0xffu);
            v += order_k_of(e, fa, aflag[j]);
            n_heavy_nb += zv[j] != 1;
        }
        vk[a] = (unsigned char)v;
        hd[a] = (unsigned char)n_heavy_nb;
        if ((fa & AT_PLANAR) && !(fa & AT_MATCHED) && zv[a] == 7 && (deg[a] == 2 || deg[a] == 3) && v == deg[a]) atomicOr(&aflag[a], AT_LONE_PAIR);
    }
    __syncthreads();
    // ---- step 4: aromatic cycles, a lane per planar cycle
    if (!many) {
        bool arom = false;
        if (lane < n_cycles) {
            int sum = 0;
            bool all = flat;
            for (int t = 0; t < len && all; ++t) {
                const int a = (int)((mine >> (8 * t)) & 0xffull);
                const unsigned fa = aflag[a];
                if (fa & AT_MATCHED) {
                    sum += 1;
                } else if ((zv[a] == 8 || zv[a] == 16) && deg[a] == 2) {
                    sum += 2;
                } else if (fa & AT_LONE_PAIR) {
                    sum += 2;
                } else {
                    bool exo = false;
                    if (zv[a] == 6)
                        for (int s = 0; s < deg[a]; ++s) {
                            const unsigned e = nb[a * MOL_DEG + s];
                            const int j = (int)(e & 0xffu);
                            exo = exo || (!(e & NB_PLANAR) && order_k_of(e, fa, aflag[j]) == 2 && (zv[j] == 7 || zv[j] == 8 || zv[j] == 16));
                        }
                    all = exo;
                }
            }
            arom = all && sum == 6;
        }
        if (arom)
            for (int t = 0; t < len; ++t) {
                const int x = (int)((mine >> (8 * t)) & 0xffull), y = (int)((mine >> (8 * (t + 1 == len ? 0 : t + 1))) & 0xffull);
                atomicOr(&nb[x * MOL_DEG + find_slot(nb, deg[x], x, y)], NB_AROMATIC);
                atomicOr(&nb[y * MOL_DEG + find_slot(nb, deg[y], y, x)], NB_AROMATIC);
                atomicOr(&aflag[x], AT_AROMATIC);
            }
        n_arom_rings = __popcll(__ballot(arom));
        __syncthreads();
    }
    // ---- steps 5 and 6 per atom
    int n_heavy = 0, n_h = 0, hbd = 0, hba = 0, n_arom_atoms = 0, n_bad = 0, deg_sum = 0;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        if (a >= n || !in[k]) continue;
        const int z = zv[a], v = vk[a];
        unsigned fa = aflag[a];
        const int h = max(0, normal_valence(z, v) - v);
        const bool donor = (z == 7 || z == 8) && h >= 1;
        const bool acceptor = z == 8 || (z == 7 && !donor && deg[a] <= 2 && !(fa & AT_LONE_PAIR));
        fa = (fa & (AT_RING | AT_AROMATIC | AT_UNSATISFIED)) | (donor ? AT_DONOR : 0u) | (acceptor ? AT_ACCEPTOR : 0u) |
             (v > allowed[elem[a0 + a]] ? AT_OVERVALENT : 0u);
        valence_k[a0 + a] = v;
        atom_h[a0 + a] = h;
        atom_flags[a0 + a] = (int)fa;
        n_heavy += z != 1;
        n_h += h;
        hbd += donor;
        hba += acceptor;
        n_arom_atoms += (fa & AT_AROMATIC) != 0;
        n_bad += (fa & (AT_UNSATISFIED | AT_OVERVALENT)) != 0;
        deg_sum += deg[a];
    }
    // ---- the bond rows, and the rotors on order_k
    int n_rot = 0;
    for (int k = p0 + lane; k < p1; k += 64) {
        const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0;
        if (!both_in_scope(inS, i, j)) {
            order_k[k] = bond_order[k];
            continue;
        }
        const unsigned e = nb[i * MOL_DEG + find_slot(nb, deg[i], i, j)];
        const int o = order_k_of(e, aflag[i], aflag[j]);
        order_k[k] = o;
        bond_flags[k] = ((e & NB_RING) ? 1 : 0) | ((e & NB_PLANAR) ? 2 : 0) | ((e & NB_AROMATIC) ? 4 : 0);
        n_rot += o == 1 && !(e & NB_RING) && hd[i] >= 2 && hd[j] >= 2;
    }
    n_heavy = wave_sum(n_heavy);
    n_h = wave_sum(n_h);
    hbd = wave_sum(hbd);
    hba = wave_sum(hba);
    n_arom_atoms = wave_sum(n_arom_atoms);
    n_bad = wave_sum(n_bad);
    n_rot = wave_sum(n_rot);
    const int m = wave_sum(deg_sum) / 2;
    // ---- step 8: the mass, class by class (integer counts: no order in the sums)
    double mw = 0.0;
    for (int c = 0; c < F; ++c) {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            cnt += a < n && in[k] && elem[a0 + a] == c;
        }
        mw = __dadd_rn(mw, __dmul_rn((double)wave_sum(cnt), mass[c]));
    }
    mw = __dadd_rn(mw, __dmul_rn((double)n_h, mass_h));
    if (lane == 0) {
        const int st = stat | (many ? SAN_TOO_MANY_RINGS : 0);
        int *d = desc_i + (size_t)b * 10;
        d[0] = n_heavy;
        d[1] = n_h;
        d[2] = hbd;
        d[3] = hba;
        d[4] = n_rot;
        d[5] = m - nS + n_frag;
        d[6] = n_arom_rings;
        d[7] = n_arom_atoms;
        d[8] = (mw < 500.0) + (hbd <= 5) + (hba <= 10) + (n_rot <= 10);
        d[9] = n_cycles;
        desc_f[(size_t)b * 2] = mw;
        desc_f[(size_t)b * 2 + 1] = 0.0;
        valid[b] = !st && !n_bad;
        status[b] = st;
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_mol_sanitize(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem,
                                       int32_t F, const int32_t *z, const int32_t *allowed, const double *mass, double mass_h,
                                       const int32_t *frag, const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr,
                                       int32_t cap_bonds, const int32_t *mol_status, int32_t largest_only, int32_t *order_k,
                                       int32_t *bond_flags, int32_t *valence_k, int32_t *atom_h, int32_t *atom_flags, int32_t *desc_i,
                                       double *desc_f, int32_t *valid, int32_t *status, void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0, KPD_ERR_INVALID, "n_atoms=%d B=%d F=%d cap_bonds=%d", n_atoms, B, F,
                cap_bonds);
    KPD_REQUIRE(mass_h >= 0.0 && mass_h < 1e6, KPD_ERR_INVALID, "mass_h=%g (finite, >= 0)", mass_h);
    KPD_REQUIRE(lig_ptr && z && allowed && mass && bond_ptr, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (pos && elem && frag && valence_k && atom_h && atom_flags), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (mol_status && desc_i && desc_f && valid && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds || (bond_ij && bond_order && order_k && bond_flags), KPD_ERR_INVALID, "null bond buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_atoms) {                                  // atoms outside S and of a ligand without a molecule read -1, 0, 0
        KPD_HIP(hipMemsetAsync(valence_k, 0xff, (size_t)n_atoms * 4, st));
        KPD_HIP(hipMemsetAsync(atom_h, 0, (size_t)n_atoms * 4, st));
        KPD_HIP(hipMemsetAsync(atom_flags, 0, (size_t)n_atoms * 4, st));
    }
    if (cap_bonds) {                                // rows of no ligand read 0
        KPD_HIP(hipMemsetAsync(order_k, 0, (size_t)cap_bonds * 4, st));
        KPD_HIP(hipMemsetAsync(bond_flags, 0, (size_t)cap_bonds * 4, st));
    }
    if (B) {
        hipLaunchKernelGGL(k_mol_sanitize, dim3(B), dim3(64), 0, st, pos, lig_ptr, n_atoms, elem, F, z, allowed, mass, mass_h, frag, bond_ij,
                           bond_order, bond_ptr, cap_bonds, mol_status, largest_only, order_k, bond_flags, valence_k, atom_h, atom_flags,
                           desc_i, desc_f, valid, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
