// Explicit hydrogens on sanitised ligands (kpd_mol_add_hs): turns the hydrogen counts of kpd_mol_sanitize into coordinates and a
// grown bond graph, a second molecule batch in the layout of kpd_mol_perceive.  Stands where upstream calls
// Chem.AddHs(lig, addCoords=True) before every force-field step.  RDKit's coordinates cannot be restated: include/kpd.h defines
// the placement rule down to the order of every operation, and tests/hydrogens_ref.py restates it.
// One wave per ligand, as k_mol_sanitize: positions and the neighbour lists (sorted by partner) live in LDS, a lane owns the
// atoms lane, lane + 64, ..., and in-wave prefix sums of the hydrogen counts give every new atom and bond its row.  The same
// kernel runs twice: a size pass that only counts, the shared exclusive scan (atoms and bonds of a ligand packed into one
// 64-bit count), and the write pass, which also blanks the rows no ligand fills.  Integer LDS atomics only (all commutative), no float atomics, no scratch memory.
// All geometry is fp64 with every product and sum rounded once: the Makefile compiles this file with -ffp-contract=off.
// The front end (entry check, atom staging, the scope S, the bond loop with its ordered row contract), the bits of
// kpd_mol_sanitize's outputs that are read here and the fp64 vectors are those of molgraph_core.h, shared with k_mol_keys and
// k_mol_sanitize.
#include "common.h"
#include "engine.h"
#include "molgraph_core.h"
#include "scan_core.h"

namespace kpd {

enum : int { HS_NO_MOLECULE = 1, HS_TOO_MANY_ATOMS = 2, HS_NO_ROOM = 4, HS_GENERAL = 8, HS_NONFINITE = 16 };
enum : int { HS_LINEAR = 0, HS_PLANAR = 1, HS_TET = 2 };
// what the class of an atom is read from: its own bonds and the aromatic flag
enum : unsigned { HI_TRIPLE = 1, HI_TWO_DOUBLES = 2, HI_DOUBLE = 4, HI_AROMATIC = 8 };
constexpr double HS_THIRD = 0.3333333333333333, HS_TET1 = 0.9428090415820634, HS_S3 = 0.5773502691896258, HS_TET2 = 0.816496580927726,
                 HS_H3 = 0.8660254037844386;

__device__ __forceinline__ V3 vperp(V3 u) {
    int e = 0;
    double ue = u.x;
    if (fabs(u.y) < fabs(ue)) {
        e = 1;
        ue = u.y;
    }
    if (fabs(u.z) < fabs(ue)) {
        e = 2;
        ue = u.z;
    }
    const V3 q = {__dsub_rn(e == 0 ? 1.0 : 0.0, __dmul_rn(ue, u.x)), __dsub_rn(e == 1 ? 1.0 : 0.0, __dmul_rn(ue, u.y)),
                  __dsub_rn(e == 2 ? 1.0 : 0.0, __dmul_rn(ue, u.z))};
    return vover(q, __dsqrt_rn(vdot(q, q)));
}

// where the hydrogens of one atom go: rows of the output batch, or nowhere (a ligand that does not fit is not written)
struct HsSink {
    float *pos;
    int *elem, *valence, *frag, *parent, *source, *bond_ij, *order;
    long long atom_row, bond_row, parent_row;       // of the atom's first hydrogen, of its first H bond, of the atom itself
    int h_class, frag_of;
    double L;
    V3 at;
    bool store;
};
__device__ __forceinline__ void hs_emit(const HsSink &o, int t, V3 d) {
    if (!o.store) return;
    const size_t r = (size_t)(o.atom_row + t), k = (size_t)(o.bond_row + t);
    o.pos[r * 3] = (float)__dadd_rn(o.at.x, __dmul_rn(o.L, d.x));
    o.pos[r * 3 + 1] = (float)__dadd_rn(o.at.y, __dmul_rn(o.L, d.y));
    o.pos[r * 3 + 2] = (float)__dadd_rn(o.at.z, __dmul_rn(o.L, d.z));
    o.elem[r] = o.h_class;
    o.valence[r] = 1;
    o.frag[r] = o.frag_of;
    o.parent[r] = (int)o.parent_row;
    o.source[r] = -1;
    o.bond_ij[k * 2] = (int)o.parent_row;
    o.bond_ij[k * 2 + 1] = (int)r;
    o.order[k] = 1;
}

// rows [lo, hi) as nothing was written to them: coordinates and orders 0, everything else -1
__device__ __forceinline__ void hs_blank_atoms(float *pos, int *elem, int *valence, int *frag, int *parent, int *source, long long lo,
                                               long long hi, int lane) {
    for (long long r = lo + lane; r < hi; r += 64) {
        pos[r * 3] = pos[r * 3 + 1] = pos[r * 3 + 2] = 0.0f;
        elem[r] = valence[r] = frag[r] = parent[r] = source[r] = -1;
    }
}
__device__ __forceinline__ void hs_blank_bonds(int *bond_ij, int *order, long long lo, long long hi, int lane) {
    for (long long k = lo + lane; k < hi; k += 64) {
        bond_ij[k * 2] = bond_ij[k * 2 + 1] = -1;
        order[k] = 0;
    }
}

// the h hydrogens of atom a (the placement rule of include/kpd.h); returns HS_GENERAL if the general rule was used or a
// coincident neighbour ignored, else 0.  nb: the neighbour lists sorted by partner, partner in the low byte.
__device__ int hs_place(const float *p, const unsigned *nb, const int *deg, const unsigned char *info, const unsigned char *zv, int a, int h,
                        const HsSink &o) {
    const V3 pa = vat(p, a);
    V3 u0 = {0, 0, 0}, u1 = u0, u2 = u0, sum = u0;
    int k = 0, first = -1, flag = 0;
    bool nbr_unsat = false;
    const int dg = deg[a];
    for (int s = 0; s < dg; ++s) {
        const int b = (int)(nb[a * MOL_DEG + s] & 0xffu);
        nbr_unsat = nbr_unsat || (info[b] & (HI_TRIPLE | HI_DOUBLE | HI_AROMATIC));
        const V3 v = vsub(vat(p, b), pa);
        const double n2 = vdot(v, v);
        if (n2 < 1e-12) {
            flag = HS_GENERAL;
            continue;
        }
        const V3 u = vover(v, __dsqrt_rn(n2));
        if (k == 0) {
            u0 = u;
            first = b;
        } else if (k == 1) {
            u1 = u;
        } else if (k == 2) {
            u2 = u;
        }
        sum = vadd(sum, u);
        ++k;
    }
    const unsigned ia = info[a];
    const int cls = (ia & (HI_TRIPLE | HI_TWO_DOUBLES)) ? HS_LINEAR
                    : ((ia & (HI_DOUBLE | HI_AROMATIC)) || (zv[a] == 7 && nbr_unsat)) ? HS_PLANAR : HS_TET;
    // the azimuth of a one-neighbour centre: anti to the lowest other neighbour of that neighbour
    V3 p0 = {0, 0, 0};
    if (k == 1 && cls != HS_LINEAR) {
        int c = -1;
        for (int s = deg[first] - 1; s >= 0; --s) {
            const int x = (int)(nb[first * MOL_DEG + s] & 0xffu);
            if (x != a) c = x;
        }
        bool have = false;
        if (c >= 0) {
            const V3 w = vsub(vat(p, c), vat(p, first));
            const double wu = vdot(w, u0);
            const V3 q = {__dsub_rn(w.x, __dmul_rn(wu, u0.x)), __dsub_rn(w.y, __dmul_rn(wu, u0.y)), __dsub_rn(w.z, __dmul_rn(wu, u0.z))};
            const double qq = vdot(q, q);
            if (qq >= 1e-12) {
                p0 = vover(vneg(q), __dsqrt_rn(qq));
                have = true;
            }
        }
        if (!have) p0 = vperp(u0);
    }
    if (cls == HS_TET && k == 0 && h <= 4) {
        for (int t = 0; t < h; ++t) {
            const double sy = (t == 1 || t == 3) ? -1.0 : 1.0, sx = (t >= 2) ? -1.0 : 1.0, sz = (t == 1 || t == 2) ? -1.0 : 1.0;
            hs_emit(o, t, {__dmul_rn(HS_S3, sx), __dmul_rn(HS_S3, sy), __dmul_rn(HS_S3, sz)});
        }
        return flag;
    }
    if (cls == HS_TET && k == 1 && h <= 3) {
        const V3 t = vcross(u0, p0);
        hs_emit(o, 0, vcomb(-HS_THIRD, u0, HS_TET1, p0));
        if (h >= 2) hs_emit(o, 1, vcomb(-HS_THIRD, u0, HS_TET1, vcomb(-0.5, p0, HS_H3, t)));
        if (h >= 3) hs_emit(o, 2, vcomb(-HS_THIRD, u0, HS_TET1, vcomb(-0.5, p0, -HS_H3, t)));
        return flag;
    }
    if (cls == HS_TET && k == 2 && h <= 2) {
        const V3 s = vadd(u0, u1), x = vcross(u0, u1);
        const double ss = vdot(s, s), xx = vdot(x, x);
        if (ss >= 1e-12 && xx >= 1e-12) {
            const V3 w = vover(vneg(s), __dsqrt_rn(ss)), n = vover(x, __dsqrt_rn(xx));
            hs_emit(o, 0, vcomb(HS_S3, w, HS_TET2, n));
            if (h >= 2) hs_emit(o, 1, vcomb(HS_S3, w, -HS_TET2, n));
            return flag;
        }
    } else if (cls == HS_TET && k == 3 && h == 1) {
        const V3 s = vadd(vadd(u0, u1), u2), x = vcross(vsub(u1, u0), vsub(u2, u0));
        const double ss = vdot(s, s), xx = vdot(x, x);
        if (xx >= 1e-12) {
            const V3 n = vover(x, __dsqrt_rn(xx));
            hs_emit(o, 0, vdot(n, s) > 0.0 ? vneg(n) : n);
            return flag;
        }
        if (ss >= 1e-4) {
            hs_emit(o, 0, vover(vneg(s), __dsqrt_rn(ss)));
            return flag;
        }
    } else if (cls == HS_PLANAR && k == 1 && h <= 2) {
        hs_emit(o, 0, vcomb(-0.5, u0, HS_H3, p0));
        if (h >= 2) hs_emit(o, 1, vcomb(-0.5, u0, -HS_H3, p0));
        return flag;
    } else if (cls == HS_PLANAR && k == 2 && h == 1) {
        const V3 s = vadd(u0, u1);
        const double ss = vdot(s, s);
        if (ss >= 1e-4) {
            hs_emit(o, 0, vover(vneg(s), __dsqrt_rn(ss)));
            return flag;
        }
    } else if (cls == HS_LINEAR && k == 1 && h == 1) {
        hs_emit(o, 0, vneg(u0));
        return flag;
    }
    // the general rule: one hydrogen after another, each opposite the sum of the unit vectors so far
    V3 lead = u0;                                   // the first unit vector: of a neighbour, else of the first hydrogen
    for (int t = 0; t < h; ++t) {
        const double ss = vdot(sum, sum);
        V3 d;
        if (k + t > 0 && ss >= 1e-4) d = vover(vneg(sum), __dsqrt_rn(ss));
        else if (k + t > 0) d = vperp(lead);
        else d = {__dmul_rn(HS_S3, 1.0), __dmul_rn(HS_S3, 1.0), __dmul_rn(HS_S3, 1.0)};
        if (k + t == 0) lead = d;
        hs_emit(o, t, d);
        sum = vadd(sum, d);
    }
    return HS_GENERAL;
}

// ---- one wave per ligand; WRITE = false: the size pass (cnt[b] = atoms << 32 | bonds of the output), true: the write pass ------------
template <bool WRITE>
__global__ void __launch_bounds__(64)
k_mol_add_hs(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, int B, const int *__restrict__ elem, int F,
             const int *__restrict__ zs, const int *__restrict__ allowed, const int *__restrict__ frag, const int *__restrict__ bond_ij,
             const int *__restrict__ order_k, const int *__restrict__ bond_ptr, int cap_in, const int *__restrict__ mol_status,
             const int *__restrict__ san_status, const int *__restrict__ valence_k, const int *__restrict__ atom_h,
             const int *__restrict__ atom_flags, int largest_only, int h_class, long long *__restrict__ cnt,
             const long long *__restrict__ packed, int cap_atoms, int cap_bonds, int *__restrict__ out_ptr, float *__restrict__ out_pos,
             int *__restrict__ out_elem, int *__restrict__ out_valence, int *__restrict__ out_frag, int *__restrict__ out_bond_ij,
             int *__restrict__ out_order, int *__restrict__ out_bond_ptr, int *__restrict__ out_summary, int *__restrict__ parent,
             int *__restrict__ source, int *__restrict__ n_h, int *__restrict__ status) {
    __shared__ float p[MOL_MAX * 3];
    __shared__ unsigned nb[MOL_MAX * MOL_DEG];      // partner | order_k << 8
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];                  // atoms per fragment, later with their hydrogens
    __shared__ int upto[MOL_MAX];                   // bond rows whose first atom is this one, later: is <= this one
    __shared__ int before[MOL_MAX];                 // hydrogens of the atoms below this one
    __shared__ unsigned char hs[MOL_MAX];           // hydrogens of the atom (0 outside S)
    __shared__ unsigned char zv[MOL_MAX];
    __shared__ unsigned char info[MOL_MAX];
    __shared__ unsigned inS[MOL_W];
    __shared__ int bad, stat;
    const int b = blockIdx.x, lane = threadIdx.x;
    const MolEntry en = mol_entry(lig_ptr, b, n_atoms, bond_ptr, cap_in, mol_status);
    const int a0 = en.a0, n = en.seg ? en.n : 0, p0 = en.p0;
    const int m = en.seg && en.range_ok ? en.p1 - p0 : 0;
    bool ok = en.ok && !(san_status[b] & SAN_NO_MOLECULE) && zs[h_class] == 1;
    bool finite = true;
    int fr_of[MOL_K] = {-1, -1, -1, -1}, h_raw[MOL_K] = {0, 0, 0, 0};
    if (ok) {                                       // wave-uniform, as every `ok` below
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            deg[a] = 0;
            fsize[a] = 0;
            upto[a] = 0;
            before[a] = 0;
            hs[a] = 0;
            info[a] = 0;
        }
        if (lane == 0) bad = stat = 0;
        __syncthreads();
        mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int k, int a, size_t g, int z) {
            const int h = atom_h[g];
            if (h < 0 || h > 4) return false;
            zv[a] = mol_z_byte(z);
            h_raw[k] = h;
            if (atom_flags[g] & AT_AROMATIC) info[a] = HI_AROMATIC;
            const float x = pos[g * 3], y = pos[g * 3 + 1], w = pos[g * 3 + 2];
            p[a * 3] = x;
            p[a * 3 + 1] = y;
            p[a * 3 + 2] = w;
            if (!(finite_f(x) && finite_f(y) && finite_f(w))) finite = false;
            return true;
        });
        __syncthreads();
        ok = !bad;
        finite = !__any(!finite);
    }
    int nS = 0, n_frags = 0;
    if (ok) {
        const MolScope sc = mol_scope(fsize, fr_of, n, lane, largest_only, inS);
        nS = sc.nS;
        n_frags = sc.n_frag;
        // the bond rows: i < j inside the ligand, order_k 1 .. 3, in (i, j) order (so none twice); neighbour entries inside S
        mol_bond_graph<true>(bond_ij, p0, en.p1, a0, n, lane, inS, (unsigned *)nullptr, 0, deg, upto, nb, &bad,
                             [order_k](int k) { return order_k[k]; }, 3, [](int, int o) { return (unsigned)o << 8; });
        __syncthreads();
        ok = !bad && nS > 0;
    }
    int H = 0;
    if (ok) {
        // the lists in partner order (they were filled in the order the atomics fell), what the class rule reads, the prefix sums
        int base_h = 0, base_r = 0;
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            int h = 0;
            if (a < n) {
                const int dg = deg[a];
                unsigned *row = nb + a * MOL_DEG;
                for (int s = 1; s < dg; ++s) {
                    const unsigned e = row[s];
                    int t = s;
                    for (; t > 0 && (row[t - 1] & 0xffu) > (e & 0xffu); --t) row[t] = row[t - 1];
                    row[t] = e;
                }
                int doubles = 0;
                unsigned inf = info[a];
                for (int s = 0; s < dg; ++s) {
                    const unsigned o = (row[s] >> 8) & 3u;
                    if (o == 3) inf |= HI_TRIPLE;
                    doubles += o == 2;
                }
                if (doubles >= 1) inf |= HI_DOUBLE;
                if (doubles >= 2) inf |= HI_TWO_DOUBLES;
                info[a] = (unsigned char)inf;
                if (in_scope(inS, a)) h = h_raw[k];
                hs[a] = (unsigned char)h;
            }
            int tot_h, tot_r;
            const int rows = a < n ? upto[a] : 0;
            const int eh = wave_exclusive(h, lane, tot_h), er = wave_exclusive(rows, lane, tot_r);
            if (a < n) {
                before[a] = base_h + eh;
                upto[a] = base_r + er + rows;
            }
            base_h += tot_h;
            base_r += tot_r;
        }
        H = base_h;
        __syncthreads();
    }
    // what becomes of the ligand: left out (a malformed segment), copied through, or hydrogenated
    int st = 0;
    if (!ok) st = HS_NO_MOLECULE;
    else if (!finite) st = HS_NONFINITE;
    else if (n + H > MOL_MAX) st = HS_TOO_MANY_ATOMS;
    const bool grow = !st && H > 0;
    const int add = st ? 0 : H;
    if (!WRITE) {
        if (lane == 0) cnt[b] = (long long)((unsigned long long)(unsigned)(n + add) << 32 | (unsigned)(m + add));
        return;
    }
    const unsigned long long at0 = (unsigned long long)packed[b], at1 = (unsigned long long)packed[b + 1];
    const long long o0 = (long long)(at0 >> 32), o1 = (long long)(at1 >> 32), q0 = (long long)(at0 & 0xffffffffull),
                    q1 = (long long)(at1 & 0xffffffffull);
    const bool fits = o1 <= (long long)cap_atoms && q1 <= (long long)cap_bonds;
    if (lane == 0) {
        out_ptr[b] = (int)o0;
        out_bond_ptr[b] = (int)q0;
        if (b == B - 1) {
            out_ptr[B] = (int)o1;
            out_bond_ptr[B] = (int)q1;
        }
    }
    // Rows nothing else writes read 0 / -1: those of this ligand if it does not fit, and this workgroup's share of the rows behind
    // the last ligand (the segments of the ligands tile the rows below out_ptr[B], so every row of the buffers is written once).
    {
        const unsigned long long end = (unsigned long long)packed[B];
        const long long cap_a = cap_atoms, cap_b = cap_bonds;
        const long long tail_a = min((long long)(end >> 32), cap_a), tail_b = min((long long)(end & 0xffffffffull), cap_b);
        const long long share_a = (cap_a - tail_a + B - 1) / B, share_b = (cap_b - tail_b + B - 1) / B;
        hs_blank_atoms(out_pos, out_elem, out_valence, out_frag, parent, source, min(tail_a + b * share_a, cap_a),
                       min(tail_a + (b + 1) * share_a, cap_a), lane);
        hs_blank_bonds(out_bond_ij, out_order, min(tail_b + b * share_b, cap_b), min(tail_b + (b + 1) * share_b, cap_b), lane);
        if (!fits) {
            hs_blank_atoms(out_pos, out_elem, out_valence, out_frag, parent, source, min(o0, cap_a), min(o1, cap_a), lane);
            hs_blank_bonds(out_bond_ij, out_order, min(q0, cap_b), min(q1, cap_b), lane);
        }
    }
    // the atoms and bonds that were there
    if (fits) {
        for (int a = lane; a < n; a += 64) {
            const size_t g = (size_t)(a0 + a), r = (size_t)(o0 + a);
            out_pos[r * 3] = pos[g * 3];
            out_pos[r * 3 + 1] = pos[g * 3 + 1];
            out_pos[r * 3 + 2] = pos[g * 3 + 2];
            out_elem[r] = elem[g];
            out_valence[r] = valence_k[g] + (grow ? (int)hs[a] : 0);
            out_frag[r] = frag[g];
            parent[r] = (int)r;
            source[r] = (int)g;
        }
        for (int k = lane; k < m; k += 64) {
            const int i = bond_ij[(size_t)(p0 + k) * 2] - a0, j = bond_ij[(size_t)(p0 + k) * 2 + 1] - a0;
            const size_t r = (size_t)(q0 + k + (grow ? before[i] : 0));
            out_bond_ij[r * 2] = (int)(o0 + i);
            out_bond_ij[r * 2 + 1] = (int)(o0 + j);
            out_order[r] = order_k[p0 + k];
        }
    }
    int invalid = 0, largest = 0;
    if (ok) {
        if (grow) {
#pragma unroll
            for (int k = 0; k < MOL_K; ++k) {
                const int a = lane + 64 * k;
                if (a < n && hs[a]) atomicAdd(&fsize[fr_of[k]], (int)hs[a]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (a >= n) continue;
            largest = max(largest, fsize[a]);
            const int e = elem[a0 + a], v = valence_k[a0 + a] + (grow ? (int)hs[a] : 0);
            invalid += v == 0 || v > allowed[e] || !element_row(zs[e]);
        }
        largest = wave_max(largest);
        invalid = wave_sum(invalid);
        if (grow && (allowed[h_class] < 1 || !element_row(zs[h_class]))) invalid += H;
    }
    if (grow) {
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (a >= n || !hs[a]) continue;
            HsSink o;
            o.pos = out_pos, o.elem = out_elem, o.valence = out_valence, o.frag = out_frag, o.parent = parent, o.source = source;
            o.bond_ij = out_bond_ij, o.order = out_order;
            o.atom_row = o0 + n + before[a];
            o.bond_row = q0 + upto[a] + before[a];
            o.parent_row = o0 + a;
            o.h_class = h_class;
            o.frag_of = fr_of[k];
            o.L = __dmul_rn((double)(int)((element_row(zv[a]) & 0xffu) + 32u), 0.01);
            o.at = vat(p, a);
            o.store = fits;
            const int fl = hs_place(p, nb, deg, info, zv, a, (int)hs[a], o);
            if (fl) atomicOr(&stat, fl);
        }
        __syncthreads();
        st |= stat;
    }
    if (lane == 0) {
        status[b] = st | (fits ? 0 : HS_NO_ROOM);
        n_h[b] = add;
        int *s = out_summary + (size_t)b * 4;
        s[0] = m + add;
        s[1] = ok ? n_frags : 0;
        s[2] = ok ? largest : 0;
        s[3] = ok ? invalid : 0;
    }
}

}  // namespace kpd

using namespace kpd;

// atoms << 32 | bonds of every ligand's output, and their exclusive prefix
struct HsScratch {
    int B;
    long long *cnt = nullptr, *packed = nullptr;
    void operator()(Carve &c) { c(cnt, (size_t)B); c(packed, (size_t)B + 1); }
};

extern "C" int64_t kpd_mol_add_hs_scratch_bytes(int32_t n_atoms, int32_t B) {
    if (n_atoms < 0 || B < 0) return -1;
    HsScratch s{B};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_mol_add_hs(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F,
                                     const int32_t *z, const int32_t *allowed, const int32_t *frag, const int32_t *bond_ij,
                                     const int32_t *order_k, const int32_t *bond_ptr, int32_t cap_bonds_in, const int32_t *mol_status,
                                     const int32_t *san_status, const int32_t *valence_k, const int32_t *atom_h, const int32_t *atom_flags,
                                     int32_t largest_only, int32_t h_class, int32_t cap_atoms, int32_t cap_bonds,
                                     int32_t *out_ptr, float *out_pos, int32_t *out_elem, int32_t *out_valence, int32_t *out_frag,
                                     int32_t *out_bond_ij, int32_t *out_order, int32_t *out_bond_ptr, int32_t *out_summary,
                                     int32_t *parent, int32_t *source, int32_t *n_h, int32_t *status, void *scratch, void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && cap_bonds_in >= 0 && cap_atoms >= 0 && cap_bonds >= 0, KPD_ERR_INVALID,
                "n_atoms=%d B=%d F=%d cap_bonds_in=%d cap_atoms=%d cap_bonds=%d", n_atoms, B, F, cap_bonds_in, cap_atoms, cap_bonds);
    KPD_REQUIRE(h_class >= 0 && h_class < F, KPD_ERR_INVALID, "h_class=%d must name one of the F=%d classes", h_class, F);
    KPD_REQUIRE((long long)n_atoms + (long long)MOL_MAX * B <= 0x7fffffffLL && B <= (1 << 21), KPD_ERR_CAPACITY,
                "n_atoms=%d B=%d: the output offsets would not fit 32 bits", n_atoms, B);
    KPD_REQUIRE(lig_ptr && z && allowed && bond_ptr && out_ptr && out_bond_ptr && scratch, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (pos && elem && frag && valence_k && atom_h && atom_flags), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!B || (mol_status && san_status && out_summary && n_h && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!cap_bonds_in || (bond_ij && order_k), KPD_ERR_INVALID, "null bond buffer");
    KPD_REQUIRE(!cap_atoms || (out_pos && out_elem && out_valence && out_frag && parent && source), KPD_ERR_INVALID, "null output buffer");
    KPD_REQUIRE(!cap_bonds || (out_bond_ij && out_order), KPD_ERR_INVALID, "null output bond buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HsScratch s{B};
    carve_raw(static_cast<char *>(scratch), s);
    long long *cnt = s.cnt, *packed = s.packed;
    if (!B) {                                       // no write pass: every row reads 0 / -1
        if (cap_atoms) {
            KPD_HIP(hipMemsetAsync(out_pos, 0, (size_t)cap_atoms * 12, st));
            KPD_HIP(hipMemsetAsync(out_elem, 0xff, (size_t)cap_atoms * 4, st));
            KPD_HIP(hipMemsetAsync(out_valence, 0xff, (size_t)cap_atoms * 4, st));
            KPD_HIP(hipMemsetAsync(out_frag, 0xff, (size_t)cap_atoms * 4, st));
            KPD_HIP(hipMemsetAsync(parent, 0xff, (size_t)cap_atoms * 4, st));
            KPD_HIP(hipMemsetAsync(source, 0xff, (size_t)cap_atoms * 4, st));
        }
        if (cap_bonds) {
            KPD_HIP(hipMemsetAsync(out_bond_ij, 0xff, (size_t)cap_bonds * 8, st));
            KPD_HIP(hipMemsetAsync(out_order, 0, (size_t)cap_bonds * 4, st));
        }
        KPD_HIP(hipMemsetAsync(out_ptr, 0, 4, st));
        KPD_HIP(hipMemsetAsync(out_bond_ptr, 0, 4, st));
        return KPD_OK;
    }
#define KPD_HS_ARGS                                                                                                                         \
    pos, lig_ptr, n_atoms, B, elem, F, z, allowed, frag, bond_ij, order_k, bond_ptr, cap_bonds_in, mol_status, san_status, valence_k, atom_h, \
        atom_flags, largest_only, h_class, cnt, packed, cap_atoms, cap_bonds, out_ptr, out_pos, out_elem, out_valence, out_frag,            \
        out_bond_ij, out_order, out_bond_ptr, out_summary, parent, source, n_h, status
    hipLaunchKernelGGL(k_mol_add_hs<false>, dim3(B), dim3(64), 0, st, KPD_HS_ARGS);
    KPD_LAUNCH_CHECK();
    KPD_TRY(exclusive_scan(st, cnt, B, packed));
    hipLaunchKernelGGL(k_mol_add_hs<true>, dim3(B), dim3(64), 0, st, KPD_HS_ARGS);
    KPD_LAUNCH_CHECK();
#undef KPD_HS_ARGS
    return KPD_OK;
}
