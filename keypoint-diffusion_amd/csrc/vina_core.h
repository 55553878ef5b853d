// What "the Vina form on one perceived ligand in its pocket" means, stated once for vina.hip (kpd_vina_score) and vina_min.hip
// (kpd_vina_minimize): the flags and the typing rule of include/kpd.h, the five terms of one pair, the pocket pair sums of one
// ligand atom, the staging of the pocket, the bond graph as a bit matrix, the type loop, the graph walk without one bond, and on
// the host the check of the weights.  Everything here is inlined into its caller and takes its arrays as plain pointers, so every
// load keeps its address space.  The LDS layouts and the kernels stay with their files, and so does the staging loop of the ligand's
// atoms: shared, it cost k_vina_minimize 1.7 % of a one-evaluation call by moving unchanged code (profiles/vina_core.md).
#pragma once
#include "common.h"
#include "molecule_core.h"

namespace kpd {

constexpr int VN_T = 256;                 // threads of a workgroup
constexpr int VN_POCKET_ROW = 20;         // staged pocket atom: 3 floats, radius, type

enum : int { VN_ATOM_OUT = 4 };           // status bit 2; bits 0 and 1 are LP_NO_MOLECULE and LP_BAD_INPUT
enum : int { VN_H = 1, VN_D = 2, VN_A = 4 };
enum : unsigned { VN_HETERO = 1u };       // neighbour flags: bit 0 = a neighbour that is neither C nor H, bit k = a bond of order k

struct VinaP {
    double w[5], w_rot, rc2;
};

// the flags of include/kpd.h from the atomic number, the heavy degree and the neighbour flags
__device__ __forceinline__ int vina_flags(int z, int deg, unsigned nf) {
    switch (z) {
    case 6: return (nf & VN_HETERO) ? 0 : VN_H;
    case 9:
    case 17:
    case 35:
    case 53: return VN_H;
    case 7:
        if (deg > 2) return 0;
        return (deg == 1 && (nf & (1u << 3))) ? VN_A : VN_D;
    case 8: return VN_A | ((deg == 0 || (deg == 1 && (nf & (1u << 1)))) ? VN_D : 0);
    case 12:
    case 20:
    case 25:
    case 26:
    case 27:
    case 28:
    case 29:
    case 30: return VN_D;
    default: return 0;
    }
}

// the five terms of one pair at surface distance d (added to t) and dd = sum over the terms of w_term * dterm/dd
__device__ __forceinline__ double vina_pair(double d, int ti, int tj, const VinaP &P, double (&t)[5]) {
    const double u = d / 0.5, v = (d - 3.0) / 2.0;
    const double g1 = exp(-(u * u)), g2 = exp(-(v * v));
    t[0] += g1;
    t[1] += g2;
    double dd = P.w[0] * (-4.0 * u * g1) + P.w[1] * (-v * g2);
    if (d < 0.0) {
        t[2] += d * d;
        dd += P.w[2] * (2.0 * d);
    }
    if (ti & tj & VN_H) {
        if (d < 0.5) {
            t[3] += 1.0;
        } else if (d < 1.5) {
            t[3] += 1.5 - d;
            dd -= P.w[3];
        }
    }
    if (((ti & VN_D) && (tj & VN_A)) || ((ti & VN_A) && (tj & VN_D))) {
        if (d < -0.7) {
            t[4] += 1.0;
        } else if (d < 0.0) {
            t[4] += d / -0.7;
            dd += P.w[4] / -0.7;
        }
    }
    return dd;
}

// The pocket pair sums of the ligand atom of type ti >= 0 and radius Ri at (xi, yi, zi), on one wavefront: lane l takes the pocket
// atoms l, l + 64, ..., the first `stage` of them from LDS (px, prad, ptyp), the rest from global memory (gpx, gpr, gpt) with the
// same bits.  Adds the lane's share of the five terms to t and of the unnormalised gradient to (gx, gy, gz).
__device__ __forceinline__ void vina_pocket_sums(double xi, double yi, double zi, double Ri, int ti, int lane, int np, int stage,
                                                 const float *px, const float *prad, const int *ptyp, const float *gpx, const float *gpr,
                                                 const int *gpt, const VinaP &P, double (&t)[5], double &gx, double &gy, double &gz) {
    for (int j = lane; j < np; j += 64) {
        float qx, qy, qz, rj;
        int tj;
        if (j < stage) {
            qx = px[3 * j];
            qy = px[3 * j + 1];
            qz = px[3 * j + 2];
            rj = prad[j];
            tj = ptyp[j];
        } else {
            const float *r = gpx + (size_t)j * 3;
            qx = r[0];
            qy = r[1];
            qz = r[2];
            rj = gpr[j];
            tj = gpt[j];
        }
        if (tj < 0 || !(rj > 0.0f)) continue;
        const double dx = xi - (double)qx, dy = yi - (double)qy, dz = zi - (double)qz;
        const double d2 = sum_sq(dx, dy, dz);
        if (!(d2 < P.rc2)) continue;
        const double r = __dsqrt_rn(d2), d = (r - Ri) - (double)rj;
        const double dd = vina_pair(d, ti, tj & 7, P, t);
        if (r >= 1e-6) {
            const double k = dd / r;
            gx += k * dx;
            gy += k * dy;
            gz += k * dz;
        }
    }
}

// Stages the pocket's np atoms from q0: every one of them is checked (LP_BAD_INPUT into bad, atom_out), the first `stage` are kept.
__device__ __forceinline__ void vina_stage_pocket(const float *__restrict__ pocket_x, const float *__restrict__ pocket_radius,
                                                  const int *__restrict__ pocket_type, int q0, int np, int stage, int tid, float *px,
                                                  float *prad, int *ptyp, int &bad, int &atom_out) {
    for (int j = tid; j < np; j += VN_T) {
        const float *r = pocket_x + (size_t)(q0 + j) * 3;
        const float rv = pocket_radius[q0 + j];
        const int tj = pocket_type[q0 + j];
        if (!(finite_f(r[0]) && finite_f(r[1]) && finite_f(r[2]) && finite_f(rv))) bad |= LP_BAD_INPUT;
        if (tj < 0 || !(rv > 0.0f)) atom_out = 1;
        if (j < stage) {
            px[3 * j] = r[0];
            px[3 * j + 1] = r[1];
            px[3 * j + 2] = r[2];
            prad[j] = rv;
            ptyp[j] = tj;
        }
    }
}

// The bond graph of bonds [p0, p1) over the staged atoms: the bit matrix adj, per atom the packed count cnt (all neighbours |
// heavy neighbours << 4) and the neighbour flags flg (integer atomics: no order).  Returns whether this thread met a bond that
// leaves the ligand out: an end beyond the ligand, a loop, an order outside 1 .. 3, an element the bond rule never bonds, a bond
// twice, a seventh neighbour.  ORDERED: bond_ij must hold i < j, so that a bond listed both ways round cannot hide from `was`;
// without it (j, i) is accepted.  FRAG: a bond across two labels of frg is refused as well.
template <bool ORDERED, bool FRAG>
__device__ __forceinline__ int vina_bond_graph(const int *__restrict__ bond_ij, const int *__restrict__ bond_order, int p0, int p1, int a0,
                                               int n, int W, int tid, const int *zat, const int *frg, unsigned *adj, unsigned *cnt,
                                               unsigned *flg) {
    int bad = 0;
    for (int k = p0 + tid; k < p1; k += VN_T) {
        const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0, o = bond_order[k];
        if (i < 0 || i >= n || j < 0 || j >= n || (ORDERED ? i >= j : i == j) || o < 1 || o > 3) {
            bad = 1;
            continue;
        }
        const int zi = zat[i], zj = zat[j];
        if (!(element_row(zi) & 0xffu) || !(element_row(zj) & 0xffu) || (FRAG && frg[i] != frg[j])) {
            bad = 1;
            continue;
        }
        const unsigned was = atomicOr(&adj[i * W + (j >> 5)], 1u << (j & 31));
        atomicOr(&adj[j * W + (i >> 5)], 1u << (i & 31));
        if (was & (1u << (j & 31))) bad = 1;     // a bond twice
        const unsigned ci = atomicAdd(&cnt[i], 1u + (zj != 1 ? 16u : 0u)), cj = atomicAdd(&cnt[j], 1u + (zi != 1 ? 16u : 0u));
        if ((ci & 15u) >= (unsigned)MOL_DEG || (cj & 15u) >= (unsigned)MOL_DEG) bad = 1;      // a seventh neighbour
        if (zj != 1) atomicOr(&flg[i], (zj != 6 ? VN_HETERO : 0u) | (1u << o));
        if (zi != 1) atomicOr(&flg[j], (zi != 6 ? VN_HETERO : 0u) | (1u << o));
    }
    return bad;
}

// The types of the n staged atoms into typ (and lig_type from a0, unless NULL): the flags of the graph, or lig_type_in's where it
// is given and >= 0; -1 and atom_out for a hydrogen or a radius that is not > 0.
__device__ __forceinline__ void vina_type_atoms(int n, int a0, int tid, const int *zat, const unsigned *cnt, const unsigned *flg,
                                                const float *rad, const int *__restrict__ lig_type_in, int *typ,
                                                int *__restrict__ lig_type, int &atom_out) {
    for (int a = tid; a < n; a += VN_T) {
        const int z = zat[a];
        int f = vina_flags(z, (int)((cnt[a] >> 4) & 15u), flg[a]);
        if (lig_type_in) {
            const int over = lig_type_in[a0 + a];
            if (over >= 0) f = over & 7;
        }
        const int t = (z == 1 || !(rad[a] > 0.0f)) ? -1 : f;
        if (t < 0) atom_out = 1;
        typ[a] = t;
        if (lig_type) lig_type[a0 + a] = t;
    }
}

// The walk from `from` through the graph without its bond to `other`; visited (vis) / frontier are bit sets in registers.  With
// STOP it ends as soon as `other` is reached and returns true (the bond is in a ring), false if the walk ends without it; without
// STOP it runs to its end and vis is the set reached.
template <bool STOP>
__device__ bool vina_walk(const unsigned *adj, int W, int from, int other, unsigned (&vis)[MOL_W]) {
    unsigned fr[MOL_W];
#pragma unroll
    for (int w = 0; w < MOL_W; ++w) vis[w] = fr[w] = (w == (from >> 5)) ? 1u << (from & 31) : 0u;
    const int ow = other >> 5;
    const unsigned ob = 1u << (other & 31);
    for (;;) {
        int a = -1;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w)
            if (a < 0 && fr[w]) {
                a = 32 * w + __ffs(fr[w]) - 1;
                fr[w] &= fr[w] - 1;
            }
        if (a < 0) return false;
        const unsigned *row = adj + a * W;
        bool found = false;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            if (w >= W) continue;
            unsigned r = row[w];
            if (a == from && w == ow) r &= ~ob;      // the bond itself
            const unsigned nw = r & ~vis[w];
            vis[w] |= nw;
            fr[w] |= nw;
            if (STOP && w == ow && (vis[w] & ob)) found = true;
        }
        if (STOP && found) return true;
    }
}

// ---- the host side: the five weights, w_rot and r_c of either parameter struct, checked and turned into a VinaP
static inline kpd_status vina_fill_params(const kpd_vina_params &d, VinaP &vp) {
    const double ws[5] = {d.w_gauss1, d.w_gauss2, d.w_repulsion, d.w_hydrophobic, d.w_hbond};
    bool ok = d.r_c > 0.0 && d.r_c < 1e6 && d.w_rot >= 0.0 && d.w_rot < 1e12;
    for (double w : ws) ok = ok && w > -1e12 && w < 1e12;
    KPD_REQUIRE(ok, KPD_ERR_INVALID, "weights %g %g %g %g %g (finite) w_rot=%g (>= 0) r_c=%g (> 0)", ws[0], ws[1], ws[2], ws[3], ws[4],
                d.w_rot, d.r_c);
    for (int k = 0; k < 5; ++k) vp.w[k] = ws[k];
    vp.w_rot = d.w_rot;
    vp.rc2 = d.r_c * d.r_c;
    return KPD_OK;
}

}  // namespace kpd
