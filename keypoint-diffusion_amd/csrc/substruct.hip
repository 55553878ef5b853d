// Substructure search on the sanitised molecules (kpd_mol_match): which ligands contain a query graph, and at which atoms.  The
// query text never reaches the device: smarts.py compiles it into the int32 table that include/kpd.h defines row by row, and that
// header states the search down to the order of every candidate (tests/match_ref.py restates it).  This is NOT RDKit's matcher.
// k_mol_match: one wave per ligand.  The front end (entry check, atom staging, the scope S, the unordered bond loop on order_k) is
// that of molgraph_core.h.  Every atom then gets one word of labels (Z, aromatic, ring, and D, H, X, v, x clamped at 15) and every
// neighbour entry the bit number of its bond in a query bond's mask.  The rows of the table are visited in ascending order, the
// same row on every lane (a row is staged into LDS, over the dead bit matrix of the bond loop); lane takes the anchors lane + 64 k
// and runs one depth-first search each, its images and cursors in LDS columns of its own.  The anchor bits of every row stay in
// LDS while the ligand is processed ($(...) references read them; the barrier at the head of the next row completes them), the
// cover bits next to them, and both are written out once at the end, followed by the typing epilogue.
#include "common.h"
#include "engine.h"
#include "molgraph_core.h"

namespace kpd {

enum : int { MM_NO_MOLECULE = 1, MM_MAX_NODES = 2 };
constexpr int Q_ATOMS = 16, Q_BONDS = 24, Q_ALT = 8, Q_PATTERNS = 512, Q_MAGIC = 0x4b505101;
constexpr int Q_HEAD = 4, Q_ROW_HEAD = 4, Q_ATOM_WORDS = 4, Q_CLOSE_WORDS = 4, Q_ALT_WORDS = 16;
constexpr int Q_ROW_MAX = Q_ROW_HEAD + Q_ATOMS * Q_ATOM_WORDS + Q_BONDS * Q_CLOSE_WORDS + Q_ATOMS * Q_ALT * Q_ALT_WORDS;
constexpr int MM_TOP = 15, MM_MAX_H = 9;
// one word of labels per atom: Z | aromatic << 8 | ring << 9 | D << 12 | H << 16 | X << 20 | v << 24 | x << 28
constexpr int PR_AROM = 8, PR_RING = 9, PR_D = 12;
static_assert(Q_ROW_MAX >= MOL_MAX * MOL_W, "the bit matrix of the bond loop fits where the rows are staged");

__global__ void __launch_bounds__(64)
k_mol_match(const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F, const int *__restrict__ zs,
            const int *__restrict__ frag, const int *__restrict__ bond_ij, const int *__restrict__ order_k, const int *__restrict__ bond_flags,
            const int *__restrict__ bond_ptr, int cap_bonds, const int *__restrict__ mol_status, const int *__restrict__ san_status,
            const int *__restrict__ valence_k, const int *__restrict__ atom_h, const int *__restrict__ atom_flags, int largest_only,
            const int *__restrict__ table, int P, int W, int all, long long max_nodes, const int *__restrict__ type_group,
            const double *__restrict__ value, int G, unsigned *__restrict__ anchor, int *__restrict__ hits, int *__restrict__ first_map,
            long long *__restrict__ n_embed, unsigned *__restrict__ cover, int *atom_type, double *__restrict__ type_sum,
            int *__restrict__ untyped, int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned dyn[];      // anc [MOL_MAX][W]; with `all` cov [MOL_MAX][W] behind it
    __shared__ unsigned rowbuf[Q_ROW_MAX];          // first life: the bit matrix of the bond loop; then the row in hand
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];
    __shared__ unsigned short nb[MOL_MAX * MOL_DEG];        // partner | (kind + 4 ring) << 8, ascending partner once sorted
    __shared__ unsigned prop[MOL_MAX];
    __shared__ unsigned char img[Q_ATOMS * 64];     // the image of query atom t in the search of a lane
    __shared__ unsigned char cur[Q_ATOMS * 64];     // the next slot of f(p(t))'s neighbour list to try at depth t
    __shared__ unsigned char map1[Q_ATOMS * 64];    // the first embedding of the lane's search in hand
    __shared__ unsigned inS[MOL_W];
    __shared__ int bad;
    unsigned *const anc = dyn, *const cov = dyn + MOL_MAX * W;

    const int b = blockIdx.x, lane = threadIdx.x;
    const MolEntry en = mol_entry(lig_ptr, b, n_atoms, bond_ptr, cap_bonds, mol_status);
    const int a0 = en.a0, n = en.n;
    bool ok = en.ok && !(san_status[b] & SAN_NO_MOLECULE);
    if (ok) {                                       // wave-uniform, as every `ok` below
        int hk[MOL_K], vk[MOL_K];
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            deg[a] = 0;
            fsize[a] = 0;
            for (int w = 0; w < MOL_W; ++w) rowbuf[a * MOL_W + w] = 0;
            hk[k] = vk[k] = 0;
        }
        for (int i = lane; i < n * W; i += 64) {
            anc[i] = 0;
            if (all) cov[i] = 0;
        }
        if (lane == 0) bad = 0;
        __syncthreads();
        int fr_of[MOL_K];
        mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int k, int a, size_t g, int z) {
            const unsigned fl = (unsigned)atom_flags[g];
            prop[a] = (unsigned)mol_z_byte(z) | ((fl >> 1) & 1u) << PR_AROM | (fl & 1u) << PR_RING;
            hk[k] = atom_h[g];
            vk[k] = valence_k[g];
            return true;
        });
        __syncthreads();
        ok = !bad;
        if (ok) {
            const int nS = mol_scope(fsize, fr_of, n, lane, largest_only, inS).nS;
            const int p0 = en.p0;
            mol_bond_graph<false>(bond_ij, p0, en.p1, a0, n, lane, inS, rowbuf, MOL_W, deg, (int *)nullptr, nb, &bad,
                                  [order_k](int k) { return order_k[k]; }, 3, [bond_flags, p0](int row, int o) {
                                      const int fl = bond_flags[p0 + row];
                                      return (unsigned)(((fl & 4) ? 3 : o - 1) | (fl & 1) << 2) << 8;
                                  });
#pragma unroll
            for (int k = 0; k < MOL_K; ++k)             // the labels of an atom of S are outputs of kpd_mol_sanitize
                if (in_scope(inS, lane + 64 * k) && (hk[k] < 0 || hk[k] > MM_MAX_H || vk[k] < 0)) atomicOr(&bad, 1);
            __syncthreads();
            ok = !bad && nS > 0;
        }
        if (ok) {
            unsigned pr[MOL_K];
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                pr[k] = 0;
                if (!in_scope(inS, a)) continue;
                unsigned short *row = nb + a * MOL_DEG;
                const int d = deg[a];
                for (int i = 1; i < d; ++i) {           // neighbours in ascending index
                    const unsigned short e = row[i];
                    int j = i;
                    for (; j > 0 && (row[j - 1] & 0xffu) > (e & 0xffu); --j) row[j] = row[j - 1];
                    row[j] = e;
                }
                int heavy = 0, ringb = 0;
                for (int i = 0; i < d; ++i) {
                    heavy += (prop[row[i] & 0xffu] & 0xffu) != 1u;
                    ringb += (row[i] >> 10) & 1;
                }
                const int D = heavy, H = hk[k] + (d - heavy), X = d + hk[k], v = vk[k] + hk[k];
                pr[k] = prop[a] | (unsigned)min(D, MM_TOP) << PR_D | (unsigned)min(H, MM_TOP) << (PR_D + 4) | (unsigned)min(X, MM_TOP) << (PR_D + 8) |
                        (unsigned)min(v, MM_TOP) << (PR_D + 12) | (unsigned)min(ringb, MM_TOP) << (PR_D + 16);
            }
            __syncthreads();                        // every Z of a neighbour has been read
#pragma unroll
            for (int k = 0; k < MOL_K; ++k)
                if (in_scope(inS, lane + 64 * k)) prop[lane + 64 * k] = pr[k];
        }
    }
    if (!ok) {                                      // the fills of the host are this ligand's outputs
        if (lane == 0) status[b] = MM_NO_MOLECULE;
        return;
    }
    // ---- the rows in ascending order, the same row on every lane ---------------------------------------------------------------------
    int flags = 0;
    for (int p = 0; p < P; ++p) {
        const int o = table[Q_HEAD + p], len = (p + 1 < P ? table[Q_HEAD + p + 1] : table[2]) - o;
        __syncthreads();                            // the row before is done: its anchor bits are complete, rowbuf is free
        for (int i = lane; i < len; i += 64) rowbuf[i] = (unsigned)table[o + i];
        __syncthreads();
        const int na = (int)rowbuf[0], nc = (int)rowbuf[1];
        const unsigned *const qa = rowbuf + Q_ROW_HEAD, *const qc = qa + Q_ATOM_WORDS * na, *const ql = qc + Q_CLOSE_WORDS * nc;
        const int pw = p >> 5;
        const unsigned pbit = 1u << (p & 31);
        auto pred = [&](int t, int v) {             // some alternative of query atom t holds at atom v
            const unsigned x = prop[v], z = (x & 0xffu) < 128u ? x & 0xffu : 0u;
            const unsigned *al = ql + Q_ALT_WORDS * qa[Q_ATOM_WORDS * t + 2];
            for (int i = (int)qa[Q_ATOM_WORDS * t + 3]; i > 0; --i, al += Q_ALT_WORDS) {
                if (!((al[z >> 5] >> (z & 31)) & (al[4] >> ((x >> PR_AROM) & 1u)) & (al[4] >> (2 + ((x >> PR_RING) & 1u))) & 1u)) continue;
                if (!((al[5] >> ((x >> PR_D) & 15u)) & (al[6] >> ((x >> (PR_D + 4)) & 15u)) & (al[7] >> ((x >> (PR_D + 8)) & 15u)) &
                      (al[8] >> ((x >> (PR_D + 12)) & 15u)) & (al[9] >> ((x >> (PR_D + 16)) & 15u)) & 1u))
                    continue;
                bool good = true;
                for (int r = 0; r < 4; ++r) {       // two rows it needs, two it forbids: all lower than p
                    const int ref = (int)al[10 + r];
                    if (ref >= 0 && (((anc[v * W + (ref >> 5)] >> (ref & 31)) & 1u) != 0) != (r < 2)) good = false;
                }
                if (good) return true;
            }
            return false;
        };
        int n_hit = 0;
        long long embeds = 0;
        bool map_done = first_map == nullptr;       // wave-uniform
        for (int k = 0; k < MOL_K && 64 * k < n; ++k) {
            const int a = lane + 64 * k;
            bool hit = false;
            if (a < n && in_scope(inS, a) && pred(0, a)) {
                img[lane] = (unsigned char)a;
                auto embedding = [&]() {
                    if (!hit)
                        for (int t = 0; t < na; ++t) map1[t * 64 + lane] = img[t * 64 + lane];
                    hit = true;
                    if (all) {
                        ++embeds;
                        for (int t = 0; t < na; ++t) atomicOr(&cov[img[t * 64 + lane] * W + pw], pbit);
                    }
                };
                if (na == 1) {
                    embedding();
                } else {
                    int t = 1;
                    long long count = 0;
                    cur[64 + lane] = 0;
                    for (;;) {
                        const int pv = img[qa[Q_ATOM_WORDS * t] * 64 + lane], dp = deg[pv];
                        const unsigned pm = qa[Q_ATOM_WORDS * t + 1];
                        int s = cur[t * 64 + lane], found = -1;
                        for (; s < dp && found < 0; ++s) {
                            const unsigned e = nb[pv * MOL_DEG + s];
                            const int v = e & 0xffu;
                            if (!((pm >> (e >> 8)) & 1u)) continue;
                            bool used = false;
                            for (int u = 0; u < t; ++u) used = used || img[u * 64 + lane] == v;
                            if (used || !pred(t, v)) continue;
                            bool closed = true;
                            for (int c = 0; c < nc && closed; ++c) {        // every closure bond to an earlier atom
                                if ((int)qc[Q_CLOSE_WORDS * c + 1] != t) continue;
                                const unsigned w = img[qc[Q_CLOSE_WORDS * c] * 64 + lane], cm = qc[Q_CLOSE_WORDS * c + 2];
                                bool there = false;
                                for (int r = 0; r < deg[v]; ++r) {
                                    const unsigned e2 = nb[v * MOL_DEG + r];
                                    there = there || ((e2 & 0xffu) == w && ((cm >> (e2 >> 8)) & 1u));
                                }
                                closed = there;
                            }
                            if (closed) found = v;
                        }
                        if (found >= 0) {
                            if (++count > max_nodes) {
                                flags |= MM_MAX_NODES;
                                break;
                            }
                            img[t * 64 + lane] = (unsigned char)found;
                            cur[t * 64 + lane] = (unsigned char)s;
                            if (t == na - 1) {
                                embedding();
                                if (!all) break;
                            } else {
                                ++t;
                                cur[t * 64 + lane] = 0;
                            }
                        } else if (--t == 0) {
                            break;
                        }
                    }
                }
            }
            const unsigned long long hm = __ballot(hit);
            n_hit += __popcll(hm);
            if (hit) anc[a * W + pw] |= pbit;       // the word of atom a is this lane's alone
            if (hm && !map_done) {                  // the embedding found from the lowest anchor
                map_done = true;
                if (lane == __ffsll(hm) - 1)
                    for (int t = 0; t < na; ++t) first_map[((size_t)b * P + p) * Q_ATOMS + t] = a0 + map1[t * 64 + lane];
            }
        }
        const unsigned long long total = all ? wave_sum((unsigned long long)embeds) : 0ull;
        if (lane == 0) {
            hits[(size_t)b * P + p] = n_hit;
            if (all) n_embed[(size_t)b * P + p] = (long long)total;
        }
    }
    __syncthreads();
    for (int i = lane; i < n * W; i += 64) {
        anchor[(size_t)a0 * W + i] = anc[i];
        if (all) cover[(size_t)a0 * W + i] = cov[i];
    }
    const bool capped = __ballot(flags & MM_MAX_NODES) != 0;
    if (lane == 0) status[b] = capped ? MM_MAX_NODES : 0;
    // ---- typing: the lowest row of every group whose anchor bit an atom has, then the sums in ascending atom index ------------------
    if (G <= 0) return;
    for (int k = 0; k < MOL_K && 64 * k < n; ++k) {
        const int a = lane + 64 * k;
        if (a >= n || !in_scope(inS, a)) continue;
        for (int w = 0; w < W; ++w) {
            unsigned bits = anc[a * W + w];
            while (bits) {
                const int p = 32 * w + __ffs(bits) - 1, g = type_group[p];
                bits &= bits - 1;
                if (g < 0 || g >= G) continue;
                int *const slot = atom_type + (size_t)g * n_atoms + a0 + a;        // -1 from the host's fill
                if (*slot < 0) *slot = p;
            }
        }
    }
    __syncthreads();                                // the types are in memory for the lanes that sum them
    for (int g = lane; g < G; g += 64) {
        double s = 0.0;
        int none = 0;
        for (int a = 0; a < n; ++a) {
            if (!in_scope(inS, a)) continue;
            const int t = atom_type[(size_t)g * n_atoms + a0 + a];
            if (t < 0) ++none;
            else s = __dadd_rn(s, value[t]);
        }
        type_sum[(size_t)b * G + g] = s;
        untyped[(size_t)b * G + g] = none;
    }
}

}  // namespace kpd

using namespace kpd;

// The table as include/kpd.h defines it, checked word by word: what the kernel indexes with is in range behind this.
static kpd_status match_table_check(const int32_t *t, int32_t words) {
    KPD_REQUIRE(words >= Q_HEAD + 1 && t[0] == Q_MAGIC && t[2] == words && t[3] == 0 && t[1] >= 1 && t[1] <= Q_PATTERNS &&
                    words > Q_HEAD + t[1] && t[Q_HEAD] == Q_HEAD + t[1],
                KPD_ERR_INVALID, "match table: bad head (magic, 1 .. %d rows, its length in words, 0, row 0 right behind the offsets)", Q_PATTERNS);
    const int P = t[1];
    for (int p = 0; p < P; ++p) {
        const int64_t o = t[Q_HEAD + p], end = p + 1 < P ? t[Q_HEAD + p + 1] : words;
        KPD_REQUIRE(o >= Q_HEAD + P && end <= words && end - o >= Q_ROW_HEAD && end - o <= Q_ROW_MAX, KPD_ERR_INVALID,
                    "match table: row %d lies at words %lld .. %lld", p, (long long)o, (long long)end);
        const int32_t *r = t + o;
        const int na = r[0], nc = r[1], nalt = r[2];
        KPD_REQUIRE(r[3] == 0, KPD_ERR_INVALID, "match table: row %d: the fourth word of its head is %d, not 0", p, r[3]);
        KPD_REQUIRE(na >= 1 && na <= Q_ATOMS && nc >= 0 && na - 1 + nc <= Q_BONDS && nalt >= 1 && nalt <= Q_ATOMS * Q_ALT, KPD_ERR_INVALID,
                    "match table: row %d has %d atoms (1 .. %d), %d closures (at most %d bonds), %d alternatives", p, na, Q_ATOMS, nc, Q_BONDS,
                    nalt);
        KPD_REQUIRE(end - o == Q_ROW_HEAD + Q_ATOM_WORDS * na + Q_CLOSE_WORDS * nc + Q_ALT_WORDS * nalt, KPD_ERR_INVALID,
                    "match table: row %d has %lld words, its counts need another number", p, (long long)(end - o));
        const int32_t *qa = r + Q_ROW_HEAD, *qc = qa + Q_ATOM_WORDS * na, *ql = qc + Q_CLOSE_WORDS * nc;
        for (int a = 0; a < na; ++a) {
            const int32_t *q = qa + Q_ATOM_WORDS * a;
            KPD_REQUIRE(a ? q[0] >= 0 && q[0] < a : q[0] == -1, KPD_ERR_INVALID, "match table: row %d, atom %d: parent %d is not lower", p, a,
                        q[0]);
            KPD_REQUIRE(q[1] >= 0 && q[1] <= 0xff && q[3] >= 1 && q[3] <= Q_ALT && q[2] >= 0 && q[2] + q[3] <= nalt, KPD_ERR_INVALID,
                        "match table: row %d, atom %d: bond mask %d, alternatives %d .. +%d of %d", p, a, q[1], q[2], q[3], nalt);
        }
        for (int c = 0; c < nc; ++c) {
            const int32_t *q = qc + Q_CLOSE_WORDS * c;
            KPD_REQUIRE(q[0] >= 0 && q[0] < q[1] && q[1] < na && q[2] >= 0 && q[2] <= 0xff && q[3] == 0, KPD_ERR_INVALID,
                        "match table: row %d, closure %d: atoms %d, %d of %d, mask %d", p, c, q[0], q[1], na, q[2]);
        }
        for (int a = 0; a < nalt; ++a) {
            const int32_t *q = ql + Q_ALT_WORDS * a;
            KPD_REQUIRE(q[4] >= 0 && q[4] <= 15 && q[14] == 0 && q[15] == 0, KPD_ERR_INVALID,
                        "match table: row %d, alternative %d: class mask %d, last words %d, %d (0, 0)", p, a, q[4], q[14], q[15]);
            for (int m = 5; m < 10; ++m)
                KPD_REQUIRE(q[m] >= 0 && q[m] <= 0xffff, KPD_ERR_INVALID, "match table: row %d, alternative %d: mask %d", p, a, q[m]);
            for (int m = 10; m < 14; ++m)
                KPD_REQUIRE(q[m] >= -1 && q[m] < p, KPD_ERR_INVALID, "match table: row %d references row %d, which is not lower", p, q[m]);
        }
    }
    return KPD_OK;
}

extern "C" kpd_status kpd_mol_match(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                                    const int32_t *frag, const int32_t *bond_ij, const int32_t *order_k, const int32_t *bond_flags,
                                    const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status, const int32_t *san_status,
                                    const int32_t *valence_k, const int32_t *atom_h, const int32_t *atom_flags, int32_t largest_only,
                                    const int32_t *table_host, const int32_t *table, int32_t table_words, int32_t mode, int64_t max_nodes,
                                    const int32_t *type_group, const double *value, int32_t G, uint32_t *anchor, int32_t *hits,
                                    int32_t *first_map, int64_t *n_embed, uint32_t *cover, int32_t *atom_type, double *type_sum,
                                    int32_t *untyped, int32_t *status, void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds >= 0 && G >= 0, KPD_ERR_INVALID, "n_atoms=%d B=%d F=%d cap_bonds=%d G=%d", n_atoms,
                B, F, cap_bonds, G);
    KPD_REQUIRE((mode == 0 || mode == 1) && max_nodes >= 1, KPD_ERR_INVALID, "mode=%d (0 or 1) max_nodes=%lld (>= 1)", mode, (long long)max_nodes);
    KPD_REQUIRE(table_host && table && lig_ptr && z && bond_ptr, KPD_ERR_INVALID, "null argument");
    KPD_TRY(match_table_check(table_host, table_words));
    const int P = table_host[1], W = (P + 31) / 32;
    KPD_REQUIRE(!n_atoms || (elem && frag && valence_k && atom_h && atom_flags && anchor && (!mode || cover) && (!G || atom_type)), KPD_ERR_INVALID,
                "null argument");
    KPD_REQUIRE(!B || (mol_status && san_status && hits && status && (!mode || n_embed) && (!G || (type_sum && untyped))), KPD_ERR_INVALID,
                "null argument");
    KPD_REQUIRE(!G || (type_group && value), KPD_ERR_INVALID, "null typing table");
    KPD_REQUIRE(!cap_bonds || (bond_ij && order_k && bond_flags), KPD_ERR_INVALID, "null bond buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_atoms) {                                  // what an atom of no ligand, and of a ligand without a molecule, reads
        KPD_HIP(hipMemsetAsync(anchor, 0, (size_t)n_atoms * W * 4, st));
        if (mode) KPD_HIP(hipMemsetAsync(cover, 0, (size_t)n_atoms * W * 4, st));
        if (G) KPD_HIP(hipMemsetAsync(atom_type, 0xff, (size_t)G * n_atoms * 4, st));
    }
    if (B) {
        KPD_HIP(hipMemsetAsync(hits, 0, (size_t)B * P * 4, st));
        if (first_map) KPD_HIP(hipMemsetAsync(first_map, 0xff, (size_t)B * P * Q_ATOMS * 4, st));
        if (mode) KPD_HIP(hipMemsetAsync(n_embed, 0, (size_t)B * P * 8, st));
        if (G) {
            KPD_HIP(hipMemsetAsync(type_sum, 0, (size_t)B * G * 8, st));
            KPD_HIP(hipMemsetAsync(untyped, 0, (size_t)B * G * 4, st));
        }
        hipLaunchKernelGGL(k_mol_match, dim3(B), dim3(64), (size_t)MOL_MAX * W * 4 * (mode ? 2 : 1), st, lig_ptr, n_atoms, elem, F, z, frag, bond_ij,
                           order_k, bond_flags, bond_ptr, cap_bonds, mol_status, san_status, valence_k, atom_h, atom_flags, largest_only, table, P,
                           W, mode, (long long)max_nodes, type_group, value, G, anchor, hits, first_map, reinterpret_cast<long long *>(n_embed),
                           cover, atom_type, type_sum, untyped, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
