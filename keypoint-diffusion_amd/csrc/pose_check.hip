// Plausibility checks of poses (kpd_pose_check): bond lengths, 1-3 distances, internal clash, flat aromatic rings, flat planar
// centres, untwisted double bonds, clash with the pocket and volume overlap with it, in the spirit of PoseBusters' list.  NOT
// PoseBusters' numbers: the reference lengths and angles are this library's own (the radii table and the centre classes of
// kpd_mol_add_hs), there is no energy check and no stereo.  include/kpd.h defines every check down to the order of every
// operation, and tests/pose_check_ref.py restates it.
// k_pose_check: one wave per (ligand, pose).  The front end (atom staging, the scope S, the unordered bond loop) is that of
// molgraph_core.h, the entry check and the pocket lookup those of the relax / Vina front end (molecule_core.h).  A lane owns the atoms
// lane, lane + 64, ..: its bonds to higher atoms (check 1, twist), the angles it is the centre of (check 2), the pairs with higher
// atoms (check 3), the aromatic cycles it is the lowest atom of, its own flatness.  Check 5 strides the pocket over the lanes.
// Check 6 walks the ligand atoms one after another, the lattice points in an atom's box strided over the lanes; the pocket atoms
// that can hold a point of the ligand at all are listed once per pose (a box test), those whose sphere meets the sphere of the atom
// at hand, and the lower ligand atoms that do, once per atom (margins far above any rounding), and a list that does not fit is
// replaced by the list it was drawn from: the counts cannot move.  The first pocket atoms are staged in LDS, the rest is read from
// global memory: the same floats either way.
// Every per-pose reduction is a minimum, a maximum or an integer count (butterflies over the wave): no summation order exists.
// fp64, every product and sum rounded once: this file is compiled with -ffp-contract=off.  Integer LDS atomics only.
#include "common.h"
#include "engine.h"
#include "molgraph_core.h"
#include "molrefine_core.h"

namespace kpd {

enum : int { PC_NO_MOLECULE = 1, PC_BAD_INPUT = 2, PC_ATOM_OUT = 4 };
enum : unsigned {
    PC_F_BOND = 1, PC_F_ANGLE = 2, PC_F_CLASH = 4, PC_F_RING = 8, PC_F_CENTRE = 16, PC_F_TWIST = 32, PC_F_POCKET = 64, PC_F_OVERLAP = 128,
    PC_OWNS_OVERLAP = 1u << 31      // in the LDS copy of atom_fail only: the atom owns a point inside the pocket
};
enum : unsigned { PC_E_AROM = 1u << 10, PC_E_RING = 1u << 11 };        // a neighbour entry: partner | order_k << 8 | these
enum : unsigned { PI_TRIPLE = 1, PI_TWO_DOUBLES = 2, PI_DOUBLE = 4, PI_AROMATIC = 8 };      // as HI_* of hydrogens.hip
enum : int { PC_LINEAR = 0, PC_PLANAR = 1, PC_TET = 2 };
constexpr int PC_NR = 10, PC_NC = 17, PC_MAX_H = 9, PC_NEAR = 1024, PC_MAX_STAGE = 2048;
constexpr double PC_MAX_COORD = 1048576.0, PC_MAX_RADIUS = 8.0, PC_THIRD = 0.3333333333333333, PC_TINY = 1e-12;
enum : int {
    C_BOND, C_BOND_F, C_ANGLE, C_ANGLE_F, C_PAIR, C_PAIR_F, C_RING, C_RING_F, C_CENTRE, C_CENTRE_F, C_TORSION, C_TORSION_F, C_TORSION_SKIP,
    C_POCKET, C_POCKET_F, C_LIG_POINTS, C_OVERLAP_POINTS
};
enum : int { R_BOND_MIN, R_BOND_MAX, R_ANGLE_MIN, R_ANGLE_MAX, R_CLASH_MIN, R_RING_MAX, R_CENTRE_MAX, R_TWIST_MIN, R_POCKET_MIN, R_OVERLAP };

struct PoseCheckParams {
    double bond_lo, bond_hi, angle_lo, angle_hi, clash_min, ring_max, centre_max, twist_min, pocket_min, pocket_scale, overlap_max, h;
};

// the rest length of a bond in half picometres from the element rows of its ends and its neighbour entry; 0: no radius
__device__ __forceinline__ int pc_r0_half(unsigned ri, unsigned rj, unsigned e) {
    const int a1 = ri & 0xffu, b1 = rj & 0xffu;
    if (!a1 || !b1) return 0;
    const int a2 = (ri >> 8) & 0xffu, b2 = (rj >> 8) & 0xffu, a3 = (ri >> 16) & 0xffu, b3 = (rj >> 16) & 0xffu;
    const int L1 = 2 * (a1 + b1), L2 = a2 && b2 ? 2 * (a2 + b2) : 0, L3 = a3 && b3 ? 2 * (a3 + b3) : 0;
    if (e & PC_E_AROM) return L2 ? (L1 + L2) / 2 : L1;
    const unsigned o = (e >> 8) & 3u;
    if (o == 3) return L3 ? L3 : L1;
    if (o == 2) return L2 ? L2 : L1;
    return L1;
}

__device__ __forceinline__ double wave_min_f64(double v) { return -wave_max(-v); }

__global__ void __launch_bounds__(64)
k_pose_check(const int *__restrict__ lig_ptr, int n_atoms, const int *__restrict__ elem, int F, const int *__restrict__ zs,
             const int *__restrict__ frag, const int *__restrict__ bond_ij, const int *__restrict__ order_k, const int *__restrict__ bond_flags,
             const int *__restrict__ bond_ptr, int cap_bonds, const int *__restrict__ mol_status, const int *__restrict__ san_status,
             const int *__restrict__ atom_h, const int *__restrict__ atom_flags, int largest_only, const float *__restrict__ pos, int K,
             int max_atoms, const float *__restrict__ lig_radius, const float *__restrict__ pocket_x, const float *__restrict__ pocket_radius,
             const int *__restrict__ pocket_ptr, int n_pocket, int P, int n_stage, const int *__restrict__ pocket_of, PoseCheckParams prm,
             int *__restrict__ fail_out, double *__restrict__ report, int *__restrict__ counts, int *__restrict__ atom_fail,
             int *__restrict__ status) {
    extern __shared__ float4 stage[];               // x, y, z, radius of the first n_stage atoms of the pocket
    __shared__ float p[MOL_MAX * 3];
    __shared__ float rad[MOL_MAX];
    __shared__ unsigned nb[MOL_MAX * MOL_DEG];      // partner | order_k << 8 | aromatic bond << 10 | ring bond << 11, ascending partner
    __shared__ unsigned A[MOL_MAX * MR_ROW];        // bonded, both ends in S
    __shared__ int deg[MOL_MAX];
    __shared__ int fsize[MOL_MAX];
    __shared__ unsigned afail[MOL_MAX];
    __shared__ int near[PC_NEAR];                   // the pocket atoms (local rows) that can hold a lattice point of the ligand
    __shared__ int near_a[PC_NEAR];                 // those of them that can hold a point of the atom at hand
    __shared__ unsigned char low_a[MOL_MAX];        // the lower ligand atoms that can
    __shared__ unsigned char zv[MOL_MAX];
    __shared__ unsigned char info[MOL_MAX];
    __shared__ unsigned char frl[MOL_MAX];
    __shared__ unsigned inS[MOL_W];
    __shared__ unsigned part[MOL_W];                // atoms of S whose radius is > 0
    __shared__ int bad;

    const int b = blockIdx.x / K, pose = blockIdx.x - b * K, lane = threadIdx.x;
    const size_t row = (size_t)blockIdx.x;
    LigandInPocket lp;
    const int entry = ligand_in_pocket(lig_ptr, b, n_atoms, max_atoms, bond_ptr, cap_bonds, mol_status, pocket_of, pocket_ptr, n_pocket, P, lp);
    if (entry || (san_status[b] & SAN_NO_MOLECULE)) {       // block-uniform; the fills of the host are this pose's rows
        if (lane == 0) status[row] = entry ? entry : PC_NO_MOLECULE;
        return;
    }
    const int a0 = lp.a0, n = lp.n, np = pocket_of[b] >= 0 ? lp.np : 0;
    const bool has_pocket = pocket_of[b] >= 0;
    const float *const P0 = pos + ((size_t)pose * n_atoms + a0) * 3;
    const float *const QX = pocket_x + (size_t)lp.q0 * 3, *const QR = pocket_radius + lp.q0;
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        deg[a] = 0;
        fsize[a] = 0;
        afail[a] = 0;
        info[a] = 0;
        rad[a] = 0.0f;
        for (int w = 0; w < MR_ROW; ++w) A[a * MR_ROW + w] = 0;
    }
    if (lane == 0) bad = 0;
    __syncthreads();
    int fr_of[MOL_K];
    bool input_ok = true;
    mol_stage_atoms(elem, F, zs, frag, a0, n, lane, fsize, &bad, fr_of, [&](int, int a, size_t g, int z) {
        const int h = atom_h[g];
        if (h < 0 || h > PC_MAX_H) return false;
        zv[a] = mol_z_byte(z);
        if (atom_flags[g] & AT_AROMATIC) info[a] = PI_AROMATIC;
        frl[a] = (unsigned char)frag[g];
        const float r = lig_radius[elem[g]];
        rad[a] = r;
        if (!finite_f(r) || r > (float)PC_MAX_RADIUS) input_ok = false;
        for (int c = 0; c < 3; ++c) {
            const float x = P0[a * 3 + c];
            p[a * 3 + c] = x;
            if (!(fabsf(x) < (float)PC_MAX_COORD)) input_ok = false;       // false for NaN too
        }
        return true;
    });
    __syncthreads();
    bool ok = !bad;
    int nS = 0;
    if (ok) {                                       // wave-uniform, as every `ok` below
        nS = mol_scope(fsize, fr_of, n, lane, largest_only, inS).nS;
        mol_bond_graph<false>(bond_ij, lp.p0, lp.p1, a0, n, lane, inS, A, MR_ROW, deg, (int *)nullptr, nb, &bad,
                              [order_k](int k) { return order_k[k]; }, 3, [&](int r, int o) {
                                  const int f = bond_flags[lp.p0 + r];
                                  return (unsigned)o << 8 | (f & 4 ? PC_E_AROM : 0u) | (f & 1 ? PC_E_RING : 0u);
                              });
        __syncthreads();
        ok = !bad && nS > 0;
    }
    if (ok) {                                       // no bond of S joins two fragment labels; the rows in partner order; the class bits
#pragma unroll
        for (int k = 0; k < MOL_K; ++k) {
            const int a = lane + 64 * k;
            if (a >= n || !in_scope(inS, a)) continue;
            const int dg = deg[a];
            unsigned *const r = nb + a * MOL_DEG;
            for (int s = 1; s < dg; ++s) {
                const unsigned e = r[s];
                int t = s;
                for (; t > 0 && (r[t - 1] & 0xffu) > (e & 0xffu); --t) r[t] = r[t - 1];
                r[t] = e;
            }
            int doubles = 0;
            unsigned inf = info[a];
            for (int s = 0; s < dg; ++s) {
                if (frl[r[s] & 0xffu] != frl[a]) atomicOr(&bad, 1);
                const unsigned o = (r[s] >> 8) & 3u;
                if (o == 3) inf |= PI_TRIPLE;
                doubles += o == 2;
            }
            if (doubles >= 1) inf |= PI_DOUBLE;
            if (doubles >= 2) inf |= PI_TWO_DOUBLES;
            info[a] = (unsigned char)inf;
        }
        __syncthreads();
        ok = !bad;
    }
    if (!ok) {
        if (lane == 0) status[row] = PC_NO_MOLECULE;
        return;
    }
    // ---- who takes part in checks 3, 5 and 6, and the box of the ligand's spheres ------------------------------------------------------
    const double inf = __builtin_inf();
    int st = 0;
    double box_lo[3] = {inf, inf, inf}, box_hi[3] = {-inf, -inf, -inf};
#pragma unroll
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        const bool in = a < n && in_scope(inS, a), takes = in && rad[a] > 0.0f;
        if (in && !takes) st |= PC_ATOM_OUT;
        const unsigned long long m = __ballot(takes);
        if (lane == 0) {
            part[2 * k] = (unsigned)m;
            part[2 * k + 1] = (unsigned)(m >> 32);
        }
        if (takes)
            for (int c = 0; c < 3; ++c) {
                box_lo[c] = fmin(box_lo[c], (double)p[a * 3 + c] - (double)rad[a]);
                box_hi[c] = fmax(box_hi[c], (double)p[a * 3 + c] + (double)rad[a]);
            }
    }
    for (int c = 0; c < 3; ++c) {
        box_lo[c] = wave_min_f64(box_lo[c]);
        box_hi[c] = wave_max(box_hi[c]);
    }
    // ---- the pocket: its first rows into LDS, every row examined, the list of those near the ligand ---------------------------------
    const int staged = min(np, n_stage);
    int n_near = 0;
    for (int base = 0; base < np; base += 64) {
        const int j = base + lane;
        bool is_near = false;
        if (j < np) {
            const float x = QX[(size_t)j * 3], y = QX[(size_t)j * 3 + 1], z = QX[(size_t)j * 3 + 2], r = QR[j];
            if (j < staged) stage[j] = make_float4(x, y, z, r);
            if (!(fabsf(x) < (float)PC_MAX_COORD && fabsf(y) < (float)PC_MAX_COORD && fabsf(z) < (float)PC_MAX_COORD) || !finite_f(r) ||
                r > (float)PC_MAX_RADIUS)
                input_ok = false;
            else if (!(r > 0.0f))
                st |= PC_ATOM_OUT;
            else {
                const double reach = (double)r * prm.pocket_scale + 1e-3;
                is_near = (double)x >= box_lo[0] - reach && (double)x <= box_hi[0] + reach && (double)y >= box_lo[1] - reach &&
                          (double)y <= box_hi[1] + reach && (double)z >= box_lo[2] - reach && (double)z <= box_hi[2] + reach;
            }
        }
        const unsigned long long m = __ballot(is_near);
        if (is_near) {
            const int slot = n_near + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < PC_NEAR) near[slot] = j;
        }
        n_near += __popcll(m);
    }
    const bool bad_input = __syncthreads_or(!input_ok);     // also the barrier behind stage, near and part
    if (bad_input) {
        if (lane == 0) status[row] = PC_BAD_INPUT;
        return;
    }
    const bool whole_pocket = n_near > PC_NEAR;
    auto pocket_atom = [&](int j) -> float4 {
        if (j < staged) return stage[j];
        return make_float4(QX[(size_t)j * 3], QX[(size_t)j * 3 + 1], QX[(size_t)j * 3 + 2], QR[j]);
    };
    auto at = [&](int a) -> V3 { return vat(p, a); };

    int cnt[PC_NC];
#pragma unroll
    for (int c = 0; c < PC_NC; ++c) cnt[c] = 0;
    double bond_min = inf, bond_max = -inf, angle_min = inf, angle_max = -inf, clash_min = inf, ring_max = -inf, centre_max = -inf,
           twist_min = inf, pocket_min = inf;

    // ---- checks 1, 2, 3, 4 on the atoms of this lane -------------------------------------------------------------------------------------
#pragma unroll 1
    for (int k = 0; k < MOL_K; ++k) {
        const int a = lane + 64 * k;
        if (a >= n || !in_scope(inS, a)) continue;
        const int dg = deg[a];
        const unsigned *const ra = nb + a * MOL_DEG;
        const unsigned row_a = element_row(zv[a]);
        const V3 pa = at(a);
        // check 1: the bonds to higher atoms; and the torsions around those of order_k 2 outside rings
        for (int s = 0; s < dg; ++s) {
            const unsigned e = ra[s];
            const int j = (int)(e & 0xffu);
            if (j < a) continue;
            const int L = pc_r0_half(row_a, element_row(zv[j]), e);
            if (L) {
                const double ratio = __ddiv_rn(__dsqrt_rn(mol_d2(p, a, j)), __dmul_rn((double)L, 0.005));
                ++cnt[C_BOND];
                bond_min = fmin(bond_min, ratio);
                bond_max = fmax(bond_max, ratio);
                if (ratio < prm.bond_lo || ratio > prm.bond_hi) {
                    ++cnt[C_BOND_F];
                    atomicOr(&afail[a], PC_F_BOND);
                    atomicOr(&afail[j], PC_F_BOND);
                }
            }
            if (((e >> 8) & 3u) != 2 || (e & PC_E_RING)) continue;
            const V3 pb = at(j), b2 = vsub(pb, pa);
            for (int s1 = 0; s1 < dg; ++s1) {
                const int c = (int)(ra[s1] & 0xffu);
                if (c == j) continue;
                const V3 n1 = vcross(vsub(pa, at(c)), b2);
                const double n11 = vdot(n1, n1);
                for (int s2 = 0; s2 < deg[j]; ++s2) {
                    const int d = (int)(nb[j * MOL_DEG + s2] & 0xffu);
                    if (d == a) continue;
                    const V3 n2 = vcross(b2, vsub(at(d), pb));
                    const double n22 = vdot(n2, n2);
                    if (n11 < PC_TINY || n22 < PC_TINY) {
                        ++cnt[C_TORSION_SKIP];
                        continue;
                    }
                    const double dd = vdot(n1, n2), c2 = __ddiv_rn(__dmul_rn(dd, dd), __dmul_rn(n11, n22));
                    ++cnt[C_TORSION];
                    twist_min = fmin(twist_min, c2);
                    if (c2 < prm.twist_min) {
                        ++cnt[C_TORSION_F];
                        atomicOr(&afail[a], PC_F_TWIST);
                        atomicOr(&afail[j], PC_F_TWIST);
                        atomicOr(&afail[c], PC_F_TWIST);
                        atomicOr(&afail[d], PC_F_TWIST);
                    }
                }
            }
        }
        // check 2: the angles this atom is the centre of
        if (dg >= 2) {
            const unsigned ia = info[a];
            bool nbr_unsat = false;
            for (int s = 0; s < dg; ++s) nbr_unsat = nbr_unsat || (info[ra[s] & 0xffu] & (PI_TRIPLE | PI_DOUBLE | PI_AROMATIC));
            const int cls = (ia & (PI_TRIPLE | PI_TWO_DOUBLES)) ? PC_LINEAR
                            : ((ia & (PI_DOUBLE | PI_AROMATIC)) || (zv[a] == 7 && nbr_unsat)) ? PC_PLANAR : PC_TET;
            const double cos0 = dg >= 4 ? -PC_THIRD : dg == 3 ? (cls == PC_TET ? -PC_THIRD : -0.5)
                                : cls == PC_LINEAR ? -1.0 : cls == PC_PLANAR ? -0.5 : -PC_THIRD;
            for (int s = 0; s < dg; ++s) {
                const int i = (int)(ra[s] & 0xffu);
                const int Li = pc_r0_half(row_a, element_row(zv[i]), ra[s]);
                for (int t = s + 1; t < dg; ++t) {
                    const int q = (int)(ra[t] & 0xffu);
                    const int Lq = pc_r0_half(row_a, element_row(zv[q]), ra[t]);
                    if (!Li || !Lq || ((A[i * MR_ROW + (q >> 5)] >> (q & 31)) & 1u)) continue;
                    const double x = __dmul_rn((double)Li, 0.005), y = __dmul_rn((double)Lq, 0.005);
                    const double d0sq = __dsub_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(__dmul_rn(__dmul_rn(2.0, x), y), cos0));
                    const double ratio = __ddiv_rn(__dsqrt_rn(mol_d2(p, i, q)), __dsqrt_rn(d0sq));
                    ++cnt[C_ANGLE];
                    angle_min = fmin(angle_min, ratio);
                    angle_max = fmax(angle_max, ratio);
                    if (ratio < prm.angle_lo || ratio > prm.angle_hi) {
                        ++cnt[C_ANGLE_F];
                        atomicOr(&afail[a], PC_F_ANGLE);
                        atomicOr(&afail[i], PC_F_ANGLE);
                        atomicOr(&afail[q], PC_F_ANGLE);
                    }
                }
            }
        }
        // check 3: the pairs with higher atoms that lie four or more bonds away, or in another component
        if (rad[a] > 0.0f) {
            unsigned ball[MOL_W], grown[MOL_W];
#pragma unroll
            for (int w = 0; w < MOL_W; ++w) ball[w] = A[a * MR_ROW + w] | (w == (a >> 5) ? 1u << (a & 31) : 0u);
            for (int step = 0; step < 2; ++step) {
#pragma unroll
                for (int w = 0; w < MOL_W; ++w) grown[w] = ball[w];
#pragma unroll
                for (int w = 0; w < MOL_W; ++w) {
                    unsigned bits = ball[w];
                    while (bits) {
                        const int j = 32 * w + __ffs(bits) - 1;
                        bits &= bits - 1;
#pragma unroll
                        for (int v = 0; v < MOL_W; ++v) grown[v] |= A[j * MR_ROW + v];
                    }
                }
#pragma unroll
                for (int w = 0; w < MOL_W; ++w) ball[w] = grown[w];
            }
            const double Ra = (double)rad[a];
#pragma unroll
            for (int w = 0; w < MOL_W; ++w) {
                unsigned bits = part[w] & ~ball[w];
                if (w == (a >> 5)) bits &= ~((2u << (a & 31)) - 1u);
                else if (w < (a >> 5)) bits = 0;
                while (bits) {
                    const int j = 32 * w + __ffs(bits) - 1;
                    bits &= bits - 1;
                    const double ratio = __ddiv_rn(__dsqrt_rn(mol_d2(p, a, j)), __dadd_rn(Ra, (double)rad[j]));
                    ++cnt[C_PAIR];
                    clash_min = fmin(clash_min, ratio);
                    if (ratio < prm.clash_min) {
                        ++cnt[C_PAIR_F];
                        atomicOr(&afail[a], PC_F_CLASH);
                        atomicOr(&afail[j], PC_F_CLASH);
                    }
                }
            }
        }
        // check 4, planar centres
        if (dg == 3 && (info[a] & (PI_DOUBLE | PI_AROMATIC))) {
            const V3 q0 = at((int)(ra[0] & 0xffu));
            const V3 nn = vcross(vsub(at((int)(ra[1] & 0xffu)), q0), vsub(at((int)(ra[2] & 0xffu)), q0));
            const double n2 = vdot(nn, nn);
            ++cnt[C_CENTRE];
            bool fails = true;
            if (n2 >= PC_TINY) {
                const double v = fabs(vdot(vsub(pa, q0), vover(nn, __dsqrt_rn(n2))));
                centre_max = fmax(centre_max, v);
                fails = v > prm.centre_max;
            }
            if (fails) {
                ++cnt[C_CENTRE_F];
                atomicOr(&afail[a], PC_F_CENTRE);
            }
        }
        // check 4, aromatic rings: the simple 5- and 6-cycles of the aromatic bonds whose lowest atom this is
        {
            int path[6], slot[6];
            int depth = 0;
            path[0] = a;
            slot[0] = 0;
            while (depth >= 0) {
                const int u = path[depth];
                if (slot[depth] >= deg[u]) {
                    --depth;
                    continue;
                }
                const unsigned e = nb[u * MOL_DEG + slot[depth]++];
                if (!(e & PC_E_AROM)) continue;
                const int v = (int)(e & 0xffu);
                if (v == a && depth >= 4 && path[1] < path[depth]) {
                    const int m = depth + 1;
                    V3 c = at(path[0]);
                    for (int t = 1; t < m; ++t) c = vadd(c, at(path[t]));
                    c = vover(c, (double)m);
                    V3 nn = {0.0, 0.0, 0.0};
                    for (int t = 0; t < m; ++t) nn = vadd(nn, vcross(vsub(at(path[t]), c), vsub(at(path[t + 1 == m ? 0 : t + 1]), c)));
                    const double n2 = vdot(nn, nn);
                    ++cnt[C_RING];
                    bool fails = true;
                    if (n2 >= PC_TINY) {
                        const V3 un = vover(nn, __dsqrt_rn(n2));
                        double v_ring = 0.0;
                        for (int t = 0; t < m; ++t) v_ring = fmax(v_ring, fabs(vdot(vsub(at(path[t]), c), un)));
                        ring_max = fmax(ring_max, v_ring);
                        fails = v_ring > prm.ring_max;
                    }
                    if (fails) {
                        ++cnt[C_RING_F];
                        for (int t = 0; t < m; ++t) atomicOr(&afail[path[t]], PC_F_RING);
                    }
                }
                if (v <= a || depth == 5) continue;
                bool seen = false;
                for (int t = 1; t <= depth; ++t) seen = seen || path[t] == v;
                if (seen) continue;
                path[++depth] = v;
                slot[depth] = 0;
            }
        }
    }
    // ---- check 5: every participating ligand atom x every participating atom of the pocket ------------------------------------------
    if (has_pocket) {
        for (int j = lane; j < np; j += 64) {
            const float4 q = pocket_atom(j);
            if (!(q.w > 0.0f)) continue;
            const double Rj = (double)q.w;
            for (int a = 0; a < n; ++a) {
                if (!in_scope(part, a)) continue;
                const double d2 = sum_sq((double)p[a * 3] - (double)q.x, (double)p[a * 3 + 1] - (double)q.y, (double)p[a * 3 + 2] - (double)q.z);
                const double ratio = __ddiv_rn(__dsqrt_rn(d2), __dadd_rn((double)rad[a], Rj));
                ++cnt[C_POCKET];
                pocket_min = fmin(pocket_min, ratio);
                if (ratio < prm.pocket_min) {
                    ++cnt[C_POCKET_F];
                    atomicOr(&afail[a], PC_F_POCKET);
                }
            }
        }
        // ---- check 6: the lattice points inside the ligand, each at its lowest atom, and those of them inside the scaled pocket -----
        const double h = prm.h;
        const int n_list = whole_pocket ? np : n_near;
        const unsigned long long below = (1ull << lane) - 1ull;
        for (int a = 0; a < n; ++a) {
            if (!in_scope(part, a)) continue;       // wave-uniform
            const double R = (double)rad[a], R2 = __dmul_rn(R, R);
            const double c[3] = {(double)p[a * 3], (double)p[a * 3 + 1], (double)p[a * 3 + 2]};
            // the pocket atoms and the lower ligand atoms whose spheres meet the sphere of a at all: a point of a can lie in no other
            // (triangle inequality; the margin of 1e-3 is far above any rounding, so no count can move).  A pocket list that does not
            // fit is replaced by the list it was drawn from.
            __syncthreads();                        // the lists of the atom before are no longer read
            int n_pa = 0, n_low = 0;
            for (int base = 0; base < n_list; base += 64) {
                const int s = base + lane;
                bool hit = false;
                int j = -1;
                if (s < n_list) {
                    j = whole_pocket ? s : near[s];
                    const float4 q = pocket_atom(j);
                    if (q.w > 0.0f) {
                        const double reach = R + prm.pocket_scale * (double)q.w + 1e-3;
                        hit = sum_sq(c[0] - (double)q.x, c[1] - (double)q.y, c[2] - (double)q.z) <= reach * reach;
                    }
                }
                const unsigned long long m = __ballot(hit);
                if (hit) {
                    const int slot = n_pa + __popcll(m & below);
                    if (slot < PC_NEAR) near_a[slot] = j;
                }
                n_pa += __popcll(m);
            }
            for (int base = 0; base < a; base += 64) {
                const int a2 = base + lane;
                bool hit = false;
                if (a2 < a && in_scope(part, a2)) {
                    const double reach = R + (double)rad[a2] + 1e-3;
                    hit = sum_sq(c[0] - (double)p[a2 * 3], c[1] - (double)p[a2 * 3 + 1], c[2] - (double)p[a2 * 3 + 2]) <= reach * reach;
                }
                const unsigned long long m = __ballot(hit);
                if (hit) low_a[n_low + __popcll(m & below)] = (unsigned char)a2;
                n_low += __popcll(m);
            }
            __syncthreads();
            const bool listed = n_pa <= PC_NEAR;
            const int n_walk = listed ? n_pa : n_list;
            int lo[3], ext[3];
            for (int d = 0; d < 3; ++d) {
                lo[d] = (int)floor(__ddiv_rn(__dsub_rn(c[d], R), h) - 1e-3);
                ext[d] = (int)floor(__ddiv_rn(__dadd_rn(c[d], R), h) + 1e-3) - lo[d] + 1;
            }
            const int total = ext[0] * ext[1] * ext[2];
            for (int t = lane; t < total; t += 64) {
                const int ix = lo[0] + t % ext[0], iy = lo[1] + (t / ext[0]) % ext[1], iz = lo[2] + t / (ext[0] * ext[1]);
                const double x = __dmul_rn(h, (double)ix), y = __dmul_rn(h, (double)iy), z = __dmul_rn(h, (double)iz);
                if (!(sum_sq(x - c[0], y - c[1], z - c[2]) <= R2)) continue;
                bool lower = false;
                for (int s = 0; s < n_low && !lower; ++s) {
                    const int a2 = low_a[s];
                    const double r2 = (double)rad[a2];
                    lower = sum_sq(x - (double)p[a2 * 3], y - (double)p[a2 * 3 + 1], z - (double)p[a2 * 3 + 2]) <= __dmul_rn(r2, r2);
                }
                if (lower) continue;
                ++cnt[C_LIG_POINTS];
                bool inside = false;
                for (int s = 0; s < n_walk && !inside; ++s) {
                    const float4 q = pocket_atom(listed ? near_a[s] : whole_pocket ? s : near[s]);
                    if (!(q.w > 0.0f)) continue;
                    const double sr = __dmul_rn(prm.pocket_scale, (double)q.w);
                    inside = sum_sq(x - (double)q.x, y - (double)q.y, z - (double)q.z) <= __dmul_rn(sr, sr);
                }
                if (inside) {
                    ++cnt[C_OVERLAP_POINTS];
                    atomicOr(&afail[a], PC_OWNS_OVERLAP);
                }
            }
        }
    }
    // ---- the pose's rows -------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < PC_NC; ++c) cnt[c] = wave_sum(cnt[c]);
    bond_min = wave_min_f64(bond_min), bond_max = wave_max(bond_max), angle_min = wave_min_f64(angle_min), angle_max = wave_max(angle_max);
    clash_min = wave_min_f64(clash_min), ring_max = wave_max(ring_max), centre_max = wave_max(centre_max);
    twist_min = wave_min_f64(twist_min), pocket_min = wave_min_f64(pocket_min);
    st = __any(st & PC_ATOM_OUT) ? PC_ATOM_OUT : 0;
    const double overlap = cnt[C_LIG_POINTS] ? __ddiv_rn((double)cnt[C_OVERLAP_POINTS], (double)cnt[C_LIG_POINTS]) : 0.0;
    const bool overlap_fails = overlap > prm.overlap_max;
    __syncthreads();                                // afail is complete
    for (int a = lane; a < n; a += 64) {
        const unsigned f = afail[a];
        atom_fail[(size_t)pose * n_atoms + a0 + a] = (int)((f & ~PC_OWNS_OVERLAP) | ((f & PC_OWNS_OVERLAP) && overlap_fails ? PC_F_OVERLAP : 0u));
    }
    if (lane == 0) {
        double *const r = report + row * PC_NR;
        r[R_BOND_MIN] = cnt[C_BOND] ? bond_min : 0.0;
        r[R_BOND_MAX] = cnt[C_BOND] ? bond_max : 0.0;
        r[R_ANGLE_MIN] = cnt[C_ANGLE] ? angle_min : 0.0;
        r[R_ANGLE_MAX] = cnt[C_ANGLE] ? angle_max : 0.0;
        r[R_CLASH_MIN] = cnt[C_PAIR] ? clash_min : 0.0;
        r[R_RING_MAX] = ring_max >= 0.0 ? ring_max : 0.0;
        r[R_CENTRE_MAX] = centre_max >= 0.0 ? centre_max : 0.0;
        r[R_TWIST_MIN] = cnt[C_TORSION] ? twist_min : 0.0;
        r[R_POCKET_MIN] = cnt[C_POCKET] ? pocket_min : 0.0;
        r[R_OVERLAP] = overlap;
        int *const c = counts + row * PC_NC;
#pragma unroll
        for (int q = 0; q < PC_NC; ++q) c[q] = cnt[q];
        fail_out[row] = (cnt[C_BOND_F] ? PC_F_BOND : 0) | (cnt[C_ANGLE_F] ? PC_F_ANGLE : 0) | (cnt[C_PAIR_F] ? PC_F_CLASH : 0) |
                        (cnt[C_RING_F] ? PC_F_RING : 0) | (cnt[C_CENTRE_F] ? PC_F_CENTRE : 0) | (cnt[C_TORSION_F] ? PC_F_TWIST : 0) |
                        (cnt[C_POCKET_F] ? PC_F_POCKET : 0) | (overlap_fails ? PC_F_OVERLAP : 0);
        status[row] = st;
    }
}

}  // namespace kpd

using namespace kpd;

static_assert(sizeof(kpd_pose_check_params) == sizeof(PoseCheckParams), "the device copy of the parameters");

extern "C" void kpd_pose_check_defaults(kpd_pose_check_params *q) {
    if (!q) return;
    q->bond_lo = 0.75, q->bond_hi = 1.25, q->angle_lo = 0.75, q->angle_hi = 1.25, q->clash_min = 0.7, q->ring_max = 0.25, q->centre_max = 0.25;
    q->twist_min = 0.75, q->pocket_min = 0.75, q->pocket_scale = 0.8, q->overlap_max = 0.075, q->h = 0.5;
}

extern "C" kpd_status kpd_pose_check(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms, const int32_t *elem, int32_t F,
                                     const int32_t *z, const int32_t *frag, const int32_t *bond_ij, const int32_t *order_k,
                                     const int32_t *bond_flags, const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status,
                                     const int32_t *san_status, const int32_t *atom_h, const int32_t *atom_flags, int32_t largest_only,
                                     const float *pos, int32_t K, const float *lig_radius, const float *pocket_x, const float *pocket_radius,
                                     const int32_t *pocket_ptr, int32_t n_pocket, int32_t P, int32_t max_pocket, const int32_t *pocket_of,
                                     const kpd_pose_check_params *params, int32_t *fail, double *report, int32_t *counts, int32_t *atom_fail,
                                     int32_t *status, void *stream) {
    KPD_TRY(ligand_pocket_args(n_atoms, B, max_atoms, F, cap_bonds, n_pocket, P, max_pocket, lig_ptr && z && bond_ptr && lig_radius,
                               elem && frag && pos && atom_h && atom_flags && atom_fail,
                               mol_status && san_status && pocket_of && fail && report && counts && status, bond_ij && order_k && bond_flags,
                               pocket_ptr != nullptr, pocket_x && pocket_radius));
    KPD_REQUIRE(K >= 1 && (long long)B * K <= 0x7fffffffLL / PC_NC && n_pocket <= (1 << 22), KPD_ERR_INVALID,
                "K=%d (>= 1) B=%d n_pocket=%d: B K must stay below 2^31 / %d and n_pocket at most 2^22", K, B, n_pocket, PC_NC);
    kpd_pose_check_params q;
    kpd_pose_check_defaults(&q);
    if (params) q = *params;
    const double *v = &q.bond_lo;
    for (int k = 0; k < 12; ++k) KPD_REQUIRE(v[k] >= 0.0 && v[k] <= 1e6, KPD_ERR_INVALID, "parameter %d = %g must be in 0 .. 1e6", k, v[k]);
    KPD_REQUIRE(q.h >= 0.1 && q.h <= 4.0 && q.pocket_scale <= 4.0, KPD_ERR_INVALID, "h=%g (0.1 .. 4) pocket_scale=%g (0 .. 4)", q.h, q.pocket_scale);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t rows = (size_t)B * K;
    if (rows) {                                     // what a pose that is left out reads
        KPD_HIP(hipMemsetAsync(fail, 0, rows * 4, st));
        KPD_HIP(hipMemsetAsync(report, 0, rows * PC_NR * 8, st));
        KPD_HIP(hipMemsetAsync(counts, 0, rows * PC_NC * 4, st));
        KPD_HIP(hipMemsetAsync(status, 0, rows * 4, st));
    }
    if (n_atoms) KPD_HIP(hipMemsetAsync(atom_fail, 0, (size_t)K * n_atoms * 4, st));
    if (rows) {
        const PoseCheckParams d = {q.bond_lo, q.bond_hi, q.angle_lo, q.angle_hi, q.clash_min, q.ring_max, q.centre_max, q.twist_min,
                                   q.pocket_min, q.pocket_scale, q.overlap_max, q.h};
        const int n_stage = std::min(max_pocket, PC_MAX_STAGE);
        hipLaunchKernelGGL(k_pose_check, dim3((unsigned)rows), dim3(64), (size_t)n_stage * sizeof(float4), st, lig_ptr, n_atoms, elem, F, z, frag,
                           bond_ij, order_k, bond_flags, bond_ptr, cap_bonds, mol_status, san_status, atom_h, atom_flags, largest_only, pos, K,
                           max_atoms, lig_radius, pocket_x, pocket_radius, pocket_ptr, n_pocket, P, n_stage, pocket_of, d, fail, report, counts,
                           atom_fail, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
