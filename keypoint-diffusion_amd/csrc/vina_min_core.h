// What vina_min.hip (kpd_vina_minimize) and vina_dock.hip (kpd_vina_dock) share, stated once: the LDS layout of one ligand's state,
// the context of one evaluation, the evaluation itself (energy and Cartesian gradient), its projection on the pose coordinates, the
// two-loop recursion, the first-order speed bound and the chart move(x, delta) of include/kpd.h.  Moved here from vina_min.hip
// unchanged; the set-up of a ligand and the iteration loop stay in each kernel (profiles/vina_dock.md says why).
#pragma once
#include "common.h"
#include "molecule_core.h"
#include "vina_core.h"

namespace kpd {

constexpr int VM_M = 8;                   // stored correction pairs
constexpr int VM_LDS = 160 * 1024 - 512;  // LDS of one CU, less the few static bytes the compiler adds for the block-wide votes
constexpr int VM_FRAGS = 8;               // bodies of one ligand
constexpr int VM_ROTORS = 64;             // active rotors of one ligand

enum : int { VM_LINE_SEARCH = 8, VM_FROZEN = 16, VM_FRAGMENTS = 32, VM_ITER_CAP = 64 };      // status bits 3 .. 6, above VN_ATOM_OUT
// slots of `scal`
enum : int { VS_INTER = 0, VS_INTRA, VS_E, VS_GNORM, VS_GP, VS_SY, VS_YY, VS_GG, VS_RESET, VS_COUNT = 16 };

struct VinaMinP : VinaP {
    double w_intra, gtol, max_step;
    int max_iters;
};

// byte offsets of the dynamic LDS of a workgroup for ligands of at most nm atoms, mr active rotors and `stage` staged pocket atoms
struct VinaMinLayout {
    size_t x, xt, g, part, vec, rho, scal, red, cen, axu, trig, body, x0, rad, zat, typ, cnt, flg, frg, piece, adj, adjp, imask, mset, fset,
        ra, rb, depth, ord, flow, fcnt, rflag, px, prad, ptyp, bytes;
    int W, DS;
};

__host__ __device__ inline VinaMinLayout vina_min_layout(int nm, int mr, int stage) {
    VinaMinLayout L;
    L.W = (nm + 31) / 32;
    L.DS = 6 * VM_FRAGS + mr;             // stride of the pose vectors
    size_t o = 0;
    auto take = [&o](size_t bytes) { return lds_take(o, bytes, 16); };
    L.x = take((size_t)nm * 3 * 8);
    L.xt = take((size_t)nm * 3 * 8);
    L.g = take((size_t)nm * 3 * 8);
    L.part = take((size_t)nm * 10 * 8);
    L.vec = take((size_t)(3 + 2 * VM_M) * L.DS * 8);          // g_delta, its trial, p, S[8], Y[8]
    L.rho = take(VM_M * 8);
    L.scal = take(VS_COUNT * 8);
    L.red = take(8 * 8);
    L.cen = take(VM_FRAGS * 3 * 8);
    L.axu = take((size_t)(mr + 1) * 3 * 8);
    L.trig = take((size_t)(mr + 1) * 2 * 8);
    L.body = take(VM_FRAGS * 8 * 8);
    L.x0 = take((size_t)nm * 3 * 4);
    L.rad = take((size_t)nm * 4);
    L.zat = take((size_t)nm * 4);
    L.typ = take((size_t)nm * 4);
    L.cnt = take((size_t)nm * 4);
    L.flg = take((size_t)nm * 4);
    L.frg = take((size_t)nm * 4);
    L.piece = take((size_t)nm * 4);
    L.adj = take((size_t)nm * L.W * 4);
    L.adjp = take((size_t)nm * L.W * 4);
    L.imask = take((size_t)nm * L.W * 4);
    L.mset = take((size_t)(mr + 1) * L.W * 4);
    L.fset = take((size_t)VM_FRAGS * L.W * 4);
    L.ra = take((size_t)(mr + 1) * 4);
    L.rb = take((size_t)(mr + 1) * 4);
    L.depth = take((size_t)(mr + 1) * 4);
    L.ord = take((size_t)(mr + 1) * 4);
    L.flow = take(VM_FRAGS * 4);
    L.fcnt = take(VM_FRAGS * 4);
    L.rflag = take((size_t)nm * 3);
    L.px = take((size_t)stage * 3 * 4);
    L.prad = take((size_t)stage * 4);
    L.ptyp = take((size_t)stage * 4);
    L.bytes = o;
    return L;
}

struct VinaMinCtx {
    int n, np, stage, W, F, T, D;
    const float *rad, *px, *prad, *gpx, *gpr;
    const int *typ, *ptyp, *gpt, *frg, *ra, *rb, *ord, *fcnt;
    const unsigned *imask, *mset;
    double *part, *scal, *red, *cen, *axu, *trig, *body;
    VinaMinP P;
};

__device__ __forceinline__ bool vm_bit(const unsigned *row, int j) { return (row[j >> 5] >> (j & 31)) & 1u; }

// r turned about the unit axis u by the angle whose cosine and sine are c, s (Rodrigues)
__device__ __forceinline__ void vm_rot(double &rx, double &ry, double &rz, double ux, double uy, double uz, double c, double s) {
    const double cx = uy * rz - uz * ry, cy = uz * rx - ux * rz, cz = ux * ry - uy * rx;
    const double k = ((ux * rx + uy * ry) + uz * rz) * (1.0 - c);
    rx = (rx * c + cx * s) + ux * k;
    ry = (ry * c + cy * s) + uy * k;
    rz = (rz * c + cz * s) + uz * k;
}

// Energy and Cartesian gradient at xq.  Wave w takes the atoms w, w + 4, ...; afterwards scal = {inter, intra, E, ...}.
__device__ void vm_eval(const VinaMinCtx &C, const double *xq, double *gq, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    for (int i = wv; i < C.n; i += 4) {
        const int ti = C.typ[i];
        double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, u[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, gx = 0.0, gy = 0.0, gz = 0.0;
        if (ti >= 0) {                               // wave-uniform
            const double xi = xq[3 * i], yi = xq[3 * i + 1], zi = xq[3 * i + 2], Ri = (double)C.rad[i];
            vina_pocket_sums(xi, yi, zi, Ri, ti, lane, C.np, C.stage, C.px, C.prad, C.ptyp, C.gpx, C.gpr, C.gpt, C.P, t, gx, gy, gz);
            const unsigned *row = C.imask + i * C.W;
            for (int j = lane; j < C.n; j += 64) {   // the ligand's own atoms: every pair is seen from both of its atoms
                if (!vm_bit(row, j)) continue;
                const double dx = xi - xq[3 * j], dy = yi - xq[3 * j + 1], dz = zi - xq[3 * j + 2];
                const double d2 = sum_sq(dx, dy, dz);
                if (!(d2 < C.P.rc2)) continue;
                const double r = __dsqrt_rn(d2), d = (r - Ri) - (double)C.rad[j];
                const double dd = vina_pair(d, ti, C.typ[j] & 7, C.P, u);
                if (r >= 1e-6) {
                    const double k = C.P.w_intra * dd / r;
                    gx += k * dx;
                    gy += k * dy;
                    gz += k * dz;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            t[k] = wave_sum(t[k]);
            u[k] = wave_sum(u[k]);
        }
        gx = wave_sum(gx);
        gy = wave_sum(gy);
        gz = wave_sum(gz);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                C.part[10 * i + k] = t[k];
                C.part[10 * i + 5 + k] = u[k];
            }
            gq[3 * i] = gx;
            gq[3 * i + 1] = gy;
            gq[3 * i + 2] = gz;
        }
    }
    __syncthreads();
    if (wv == 0) {
        double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = lane; i < C.n; i += 64) {
#pragma unroll
            for (int k = 0; k < 10; ++k) s[k] += C.part[10 * i + k];
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) s[k] = wave_sum(s[k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 10; ++k) s[k] *= C.P.w[k % 5];
            const double inter = (((s[0] + s[1]) + s[2]) + s[3]) + s[4];
            const double intra = 0.5 * ((((s[5] + s[6]) + s[7]) + s[8]) + s[9]);
            C.scal[VS_INTER] = inter;
            C.scal[VS_INTRA] = intra;
            C.scal[VS_E] = inter + C.P.w_intra * intra;
        }
    }
    __syncthreads();
}

// The gradient at delta = 0 in the chart at xq, from the Cartesian gradient gq: the centres and axes of xq are left in cen / axu,
// the largest |entry| in scal[VS_GNORM].
__device__ void vm_project(const VinaMinCtx &C, const double *xq, const double *gq, double *gd, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    if (tid < 3 * C.F) {                             // a centre's component: its fragment's atoms in index order
        const int f = tid / 3, c = tid % 3;
        double s = 0.0;
        for (int i = 0; i < C.n; ++i)
            if (C.frg[i] == f) s += xq[3 * i + c];
        C.cen[tid] = s / (double)C.fcnt[f];
    }
    __syncthreads();
    for (int q = wv; q < C.F + C.T; q += 4) {        // wave-uniform
        if (q < C.F) {
            const double cx = C.cen[3 * q], cy = C.cen[3 * q + 1], cz = C.cen[3 * q + 2];
            double tx = 0.0, ty = 0.0, tz = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;
            for (int i = lane; i < C.n; i += 64) {
                if (C.frg[i] != q) continue;
                const double gx = gq[3 * i], gy = gq[3 * i + 1], gz = gq[3 * i + 2];
                const double rx = xq[3 * i] - cx, ry = xq[3 * i + 1] - cy, rz = xq[3 * i + 2] - cz;
                tx += gx;
                ty += gy;
                tz += gz;
                ox += ry * gz - rz * gy;
                oy += rz * gx - rx * gz;
                oz += rx * gy - ry * gx;
            }
            tx = wave_sum(tx);
            ty = wave_sum(ty);
            tz = wave_sum(tz);
            ox = wave_sum(ox);
            oy = wave_sum(oy);
            oz = wave_sum(oz);
            if (lane == 0) {
                double *o = gd + 6 * q;
                o[0] = tx;
                o[1] = ty;
                o[2] = tz;
                o[3] = ox;
                o[4] = oy;
                o[5] = oz;
            }
        } else {
            const int k = q - C.F, a = C.ra[k], b = C.rb[k];
            const double bx = xq[3 * b], by = xq[3 * b + 1], bz = xq[3 * b + 2];
            const double ax = bx - xq[3 * a], ay = by - xq[3 * a + 1], az = bz - xq[3 * a + 2];
            const double len = sqrt((ax * ax + ay * ay) + az * az);
            const bool ok = len >= 1e-6;             // an axis that cannot be measured turns nothing
            const double ux = ok ? ax / len : 0.0, uy = ok ? ay / len : 0.0, uz = ok ? az / len : 0.0;
            const unsigned *M = C.mset + k * C.W;
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int i = lane; i < C.n; i += 64) {
                if (!vm_bit(M, i)) continue;
                const double gx = gq[3 * i], gy = gq[3 * i + 1], gz = gq[3 * i + 2];
                const double rx = xq[3 * i] - bx, ry = xq[3 * i + 1] - by, rz = xq[3 * i + 2] - bz;
                sx += ry * gz - rz * gy;
                sy += rz * gx - rx * gz;
                sz += rx * gy - ry * gx;
            }
            sx = wave_sum(sx);
            sy = wave_sum(sy);
            sz = wave_sum(sz);
            if (lane == 0) {
                C.axu[3 * k] = ux;
                C.axu[3 * k + 1] = uy;
                C.axu[3 * k + 2] = uz;
                gd[6 * C.F + k] = (ux * sx + uy * sy) + uz * sz;
            }
        }
    }
    __syncthreads();
    if (wv == 0) {
        double m = 0.0;
        for (int d = lane; d < C.D; d += 64) m = fmax(m, fabs(gd[d]));
        m = wave_max(m);
        if (lane == 0) C.scal[VS_GNORM] = m;
    }
    __syncthreads();
}

// a . b over the D entries of two pose vectors on one wavefront: lane l takes the entries l and l + 64
__device__ __forceinline__ double vm_dot(const double *a, const double *b, int D, int lane) {
    double v = 0.0;
    if (lane < D) v = a[lane] * b[lane];
    if (lane + 64 < D) v += a[lane + 64] * b[lane + 64];
    return wave_sum(v);
}

// The direction p = -H g_delta by the two-loop recursion over the m newest pairs, on wave 0 alone; scal[VS_GP] = g.p; should that
// not be negative, p = -g and scal[VS_RESET] = 1 (the pairs are to be dropped).
__device__ void vm_direction(const double *gd, const double *S, const double *Y, const double *rho, int DS, int D, int m, int head,
                             double gamma, double *p, double *scal, int lane) {
    const int d0 = lane, d1 = lane + 64;
    const bool in0 = d0 < D, in1 = d1 < D;
    const double g0 = in0 ? gd[d0] : 0.0, g1 = in1 ? gd[d1] : 0.0;
    double q0 = g0, q1 = g1, al[VM_M];
#pragma unroll
    for (int k = 0; k < VM_M; ++k) {                 // newest first
        al[k] = 0.0;
        if (k < m) {
            const int slot = (head + VM_M - 1 - k) & (VM_M - 1);
            const double s0 = in0 ? S[slot * DS + d0] : 0.0, s1 = in1 ? S[slot * DS + d1] : 0.0;
            const double y0 = in0 ? Y[slot * DS + d0] : 0.0, y1 = in1 ? Y[slot * DS + d1] : 0.0;
            al[k] = rho[slot] * wave_sum(s0 * q0 + s1 * q1);
            q0 -= al[k] * y0;
            q1 -= al[k] * y1;
        }
    }
    if (m) {
        q0 *= gamma;
        q1 *= gamma;
    }
#pragma unroll
    for (int k = VM_M - 1; k >= 0; --k) {            // oldest first
        if (k < m) {
            const int slot = (head + VM_M - 1 - k) & (VM_M - 1);
            const double s0 = in0 ? S[slot * DS + d0] : 0.0, s1 = in1 ? S[slot * DS + d1] : 0.0;
            const double y0 = in0 ? Y[slot * DS + d0] : 0.0, y1 = in1 ? Y[slot * DS + d1] : 0.0;
            const double be = rho[slot] * wave_sum(y0 * q0 + y1 * q1);
            q0 += (al[k] - be) * s0;
            q1 += (al[k] - be) * s1;
        }
    }
    q0 = -q0;
    q1 = -q1;
    double gp = wave_sum(g0 * q0 + g1 * q1), reset = 0.0;
    if (!(gp < 0.0)) {                               // no descent direction: forget the pairs
        reset = 1.0;
        q0 = -g0;
        q1 = -g1;
        gp = -wave_sum(g0 * g0 + g1 * g1);
    }
    if (in0) p[d0] = q0;
    if (in1) p[d1] = q1;
    if (lane == 0) {
        scal[VS_GP] = gp;
        scal[VS_RESET] = reset;
    }
}

// the largest first-order speed of an atom under the pose velocity p (a maximum has no order); cen and axu are those of x
__device__ double vm_vmax(const VinaMinCtx &C, const double *x, const double *p, int tid) {
    double m = 0.0;
    for (int i = tid; i < C.n; i += VN_T) {
        const int f = C.frg[i];
        const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
        const double *pf = p + 6 * f;
        const double rx = xi - C.cen[3 * f], ry = yi - C.cen[3 * f + 1], rz = zi - C.cen[3 * f + 2];
        double vx = pf[0] + (pf[4] * rz - pf[5] * ry), vy = pf[1] + (pf[5] * rx - pf[3] * rz), vz = pf[2] + (pf[3] * ry - pf[4] * rx);
        for (int k = 0; k < C.T; ++k) {
            if (!vm_bit(C.mset + k * C.W, i)) continue;
            const int b = C.rb[k];
            const double pk = p[6 * C.F + k], ux = C.axu[3 * k], uy = C.axu[3 * k + 1], uz = C.axu[3 * k + 2];
            const double sx = xi - x[3 * b], sy = yi - x[3 * b + 1], sz = zi - x[3 * b + 2];
            vx += pk * (uy * sz - uz * sy);
            vy += pk * (uz * sx - ux * sz);
            vz += pk * (ux * sy - uy * sx);
        }
        m = fmax(m, sqrt((vx * vx + vy * vy) + vz * vz));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) C.red[tid >> 6] = m;
    __syncthreads();
    const double r = fmax(fmax(C.red[0], C.red[1]), fmax(C.red[2], C.red[3]));
    __syncthreads();
    return r;
}

// xt = move(x, alpha p): torsions from the deepest to the shallowest about the axes of x, then the bodies about the centres of x
__device__ void vm_move(const VinaMinCtx &C, const double *x, const double *p, double alpha, double *xt, int tid) {
    if (tid < C.T) {
        double s, c;
        sincos(alpha * p[6 * C.F + tid], &s, &c);
        C.trig[2 * tid] = c;
        C.trig[2 * tid + 1] = s;
    } else if (tid >= 64 && tid < 64 + C.F) {
        const int f = tid - 64;
        const double *pf = p + 6 * f;
        const double ox = alpha * pf[3], oy = alpha * pf[4], oz = alpha * pf[5];
        const double th = sqrt((ox * ox + oy * oy) + oz * oz);
        double *o = C.body + 8 * f;
        double s = 0.0, c = 1.0;
        const bool turn = th >= 1e-12;
        if (turn) sincos(th, &s, &c);
        o[0] = turn ? ox / th : 0.0;
        o[1] = turn ? oy / th : 0.0;
        o[2] = turn ? oz / th : 0.0;
        o[3] = c;
        o[4] = s;
        o[5] = alpha * pf[0];
        o[6] = alpha * pf[1];
        o[7] = alpha * pf[2];
    }
    __syncthreads();
    for (int i = tid; i < C.n; i += VN_T) {
        double px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
        for (int kk = 0; kk < C.T; ++kk) {
            const int k = C.ord[kk];
            if (!vm_bit(C.mset + k * C.W, i)) continue;
            const int b = C.rb[k];
            const double bx = x[3 * b], by = x[3 * b + 1], bz = x[3 * b + 2];
            double rx = px - bx, ry = py - by, rz = pz - bz;
            vm_rot(rx, ry, rz, C.axu[3 * k], C.axu[3 * k + 1], C.axu[3 * k + 2], C.trig[2 * k], C.trig[2 * k + 1]);
            px = bx + rx;
            py = by + ry;
            pz = bz + rz;
        }
        const int f = C.frg[i];
        const double *o = C.body + 8 * f;
        const double cx = C.cen[3 * f], cy = C.cen[3 * f + 1], cz = C.cen[3 * f + 2];
        double rx = px - cx, ry = py - cy, rz = pz - cz;
        vm_rot(rx, ry, rz, o[0], o[1], o[2], o[3], o[4]);
        xt[3 * i] = (cx + rx) + o[5];
        xt[3 * i + 1] = (cy + ry) + o[6];
        xt[3 * i + 2] = (cz + rz) + o[7];
    }
    __syncthreads();
}

}  // namespace kpd
