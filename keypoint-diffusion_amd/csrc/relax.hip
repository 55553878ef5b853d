// Relaxation of sampled ligands inside their rigid pockets on the device: the step upstream runs after building molecules
// (analysis/pocket_minimization.py: RDKit's UFF on ligand + receptor with every receptor atom fixed, up to 400 iterations, then
// `CalcRMS` and the energies before and after).  RDKit's UFF cannot be restated here (it needs hydrogens, atom typing, torsions and
// inversions), so include/kpd.h DEFINES the force field and the minimiser used instead: harmonic bonds and cosine-harmonic angles
// around the ideal values nearest to the sampled geometry, a cut, shifted, soft-core Lennard-Jones term inside the ligand and
// against the pocket, L-BFGS with Armijo backtracking.  NOT UFF: its energies compare samples relaxed here with each other only.
// One workgroup (4 waves) per ligand and ONE launch for the whole minimisation of every ligand.  The state (x, g, p, the trial
// point, 8 correction pairs) lives in LDS in fp64, beside the ligand's topology and as much of its pocket as fits; the rest of
// the pocket is read from global memory (L2: consecutive ligands share a pocket).  An atom's gradient is summed by one wavefront:
// its lanes stride the pocket atoms, then the ligand atoms, take one bond or angle each, and meet in a butterfly; every dot product
// meets in the same fixed tree.  Nothing is shared between ligands, no atomics on floats, no host synchronisation: a ligand's result
// is bitwise independent of the batch, of what was staged, and of the repeat.
#include "common.h"
#include "molecule_core.h"

namespace kpd {

constexpr int RX_T = 256;                // threads of a workgroup
constexpr int RX_M = 8;                  // stored correction pairs
constexpr int RX_LDS = 160 * 1024 - 512;  // LDS of one CU, less the few static bytes the compiler adds for the block-wide votes
constexpr int RX_POCKET_ROW = 28;        // staged pocket atom: 3 floats, 2 doubles
constexpr double RX_COS100 = -0.1736481776669303, RX_COS150 = -0.8660254037844387, RX_COS114 = -0.4184314830435483;
constexpr double RX_COS_TET = -0.3333333228927115;        // cos 109.47122 deg

enum : int { RX_ITER_CAP = 4, RX_LINE_SEARCH = 8 };      // status bits 2 and 3; bits 0 and 1 are LP_NO_MOLECULE and LP_BAD_INPUT

struct RelaxP {
    double k_b, k_a, rc2, inv_rc2, s, ce, cf, w_intra, gtol, max_step;
    int max_iters;
};

// byte offsets of the dynamic LDS of a workgroup for ligands of at most nm atoms and `stage` staged pocket atoms
struct RelaxLayout {
    size_t vec, sx, sD, epart, red, scal, rho, psx, psD, x0, px, excl, acls, deg, r0h, nbr, bytes;
    int W;
};

__host__ __device__ inline RelaxLayout relax_layout(int nm, int stage) {
    RelaxLayout L;
    L.W = (nm + 31) / 32;
    size_t o = 0;
    auto take = [&o](size_t bytes) { return lds_take(o, bytes, 8); };
    L.vec = take((size_t)(5 + 2 * RX_M) * 3 * nm * 8);       // x, g, p, xt, gt, S[8], Y[8]
    L.sx = take((size_t)nm * 8);
    L.sD = take((size_t)nm * 8);
    L.epart = take((size_t)nm * 4 * 8);
    L.red = take(8 * 8);
    L.scal = take(8 * 8);
    L.rho = take(RX_M * 8);
    L.psx = take((size_t)stage * 8);
    L.psD = take((size_t)stage * 8);
    L.x0 = take((size_t)nm * 3 * 4);
    L.px = take((size_t)stage * 3 * 4);
    L.excl = take((size_t)nm * L.W * 4);
    L.acls = take((size_t)nm * 4);
    L.deg = take((size_t)nm * 4);
    L.r0h = take((size_t)nm * MOL_DEG * 2);
    L.nbr = take((size_t)nm * MOL_DEG);
    L.bytes = o;
    return L;
}

struct RelaxCtx {
    int n, np, stage, W;
    const double *sx, *sD, *psx, *psD;
    const float *x0, *px;
    const float *gpx, *gpv;              // this pocket's rows in global memory: coordinates [np,3], {x, D} [np,2]
    const unsigned *excl, *acls;
    const int *deg;
    const unsigned short *r0h;
    const unsigned char *nbr;
    double *epart, *red, *scal;
    RelaxP P;
};

// a . b over N3 elements: thread t takes t, t + 256, ...; butterfly inside each wave; the four waves in order.  Same value on every
// thread.
__device__ __forceinline__ double block_dot(const double *a, const double *b, int N3, double *red, int tid) {
    double v = 0.0;
    for (int k = tid; k < N3; k += RX_T) v += a[k] * b[k];
    v = wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

// the largest |v_i| over the n atoms (a maximum has no order)
__device__ __forceinline__ double block_max_norm(const double *v, int n, double *red, int tid) {
    double m = 0.0;
    for (int i = tid; i < n; i += RX_T) m = fmax(m, sqrt(v[3 * i] * v[3 * i] + v[3 * i + 1] * v[3 * i + 1] + v[3 * i + 2] * v[3 * i + 2]));
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r;
}

// the non-bonded pair of include/kpd.h at squared distance d2: energy e and k with dE/dx_i = k (x_i - x_j)
__device__ __forceinline__ void lj_pair(double d2, double xij, double Dij, const RelaxP &P, double &e, double &k) {
    e = 0.0;
    k = 0.0;
    if (!(d2 < P.rc2)) return;
    const double x2 = xij * xij, q = x2 * P.inv_rc2, q3 = q * q * q, shift = Dij * (q3 * q3 - 2.0 * q3), d0 = P.s * xij;
    if (d2 < d0 * d0) {                              // soft core: the tangent line of e at d0
        const double d = sqrt(d2), slope = -12.0 * Dij * P.cf / d0;
        e = Dij * P.ce + slope * (d - d0) - shift;
        k = d >= 1e-6 ? slope / d : 0.0;
    } else {
        const double u = x2 / d2, u3 = u * u * u;
        e = Dij * (u3 * u3 - 2.0 * u3) - shift;
        k = -12.0 * Dij * (u3 * u3 - u3) / d2;
    }
}

// slots (a, b), a < b < 6, of pair q = 0 .. 14 of a neighbour list, and back
__device__ __forceinline__ void pair_slots(int q, int &a, int &b) {
    a = 0;
    while (q >= MOL_DEG - 1 - a) {
        q -= MOL_DEG - 1 - a;
        ++a;
    }
    b = a + 1 + q;
}
__device__ __forceinline__ int pair_index(int a, int b) { return a * (2 * MOL_DEG - 1 - a) / 2 + b - a - 1; }

// cosine of the angle a - c - b in the coordinates v (double or the fp32 input); false if an arm is shorter than 1e-6
template <typename T>
__device__ __forceinline__ bool angle_cos(const T *v, int a, int c, int b, double (&u)[3], double (&w)[3], double &uu, double &ww,
                                          double &inv, double &cs) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = (double)v[3 * a + k] - (double)v[3 * c + k];
        w[k] = (double)v[3 * b + k] - (double)v[3 * c + k];
    }
    uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
    ww = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (uu < 1e-12 || ww < 1e-12) return false;
    inv = 1.0 / sqrt(uu * ww);
    cs = (u[0] * w[0] + u[1] * w[1] + u[2] * w[2]) * inv;
    return true;
}

// the angle a - c - b with rest class cls: its energy and, into (gx, gy, gz), its gradient with respect to c (centre) or to a
__device__ __forceinline__ double angle_term(const RelaxCtx &C, const double *xq, int a, int c, int b, unsigned cls, bool centre,
                                             double &gx, double &gy, double &gz) {
    double u[3], w[3], uu, ww, inv, cs, cos0 = cls == 1 ? RX_COS_TET : cls == 2 ? -0.5 : -1.0;
    if (cls == 0 && !angle_cos(C.x0, a, c, b, u, w, uu, ww, inv, cos0)) return 0.0;
    if (!angle_cos(xq, a, c, b, u, w, uu, ww, inv, cs)) return 0.0;
    const double dl = cs - cos0, f = C.P.k_a * dl;
    double ga[3], gb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ga[k] = f * (w[k] * inv - cs * u[k] / uu);
        gb[k] = f * (u[k] * inv - cs * w[k] / ww);
    }
    if (centre) {
        gx -= ga[0] + gb[0];
        gy -= ga[1] + gb[1];
        gz -= ga[2] + gb[2];
    } else {
        gx += ga[0];
        gy += ga[1];
        gz += ga[2];
    }
    return 0.5 * C.P.k_a * dl * dl;
}

// Energy and gradient at xq.  Wave w takes the atoms w, w + 4, ...; afterwards scal = {bond, angle, intra, pocket, E, gmax}.
__device__ void relax_eval(const RelaxCtx &C, const double *xq, double *gq, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    for (int i = wv; i < C.n; i += 4) {
        const double xi = xq[3 * i], yi = xq[3 * i + 1], zi = xq[3 * i + 2], sxi = C.sx[i], sDi = C.sD[i];
        double gx = 0.0, gy = 0.0, gz = 0.0, eb = 0.0, ea = 0.0, ei = 0.0, ep = 0.0;
        for (int j = lane; j < C.np; j += 64) {     // the pocket
            double qx, qy, qz, sxj, sDj;
            if (j < C.stage) {
                qx = (double)C.px[3 * j];
                qy = (double)C.px[3 * j + 1];
                qz = (double)C.px[3 * j + 2];
                sxj = C.psx[j];
                sDj = C.psD[j];
            } else {
                const float *r = C.gpx + (size_t)j * 3, *v = C.gpv + (size_t)j * 2;
                qx = (double)r[0];
                qy = (double)r[1];
                qz = (double)r[2];
                sxj = sqrt((double)v[0]);
                sDj = sqrt((double)v[1]);
            }
            const double dx = xi - qx, dy = yi - qy, dz = zi - qz;
            double e, k;
            lj_pair(dx * dx + dy * dy + dz * dz, sxi * sxj, sDi * sDj, C.P, e, k);
            ep += e;
            gx += k * dx;
            gy += k * dy;
            gz += k * dz;
        }
        for (int j = lane; j < C.n; j += 64) {      // the ligand's own atoms three or more bonds away
            if ((C.excl[i * C.W + (j >> 5)] >> (j & 31)) & 1u) continue;
            const double dx = xi - xq[3 * j], dy = yi - xq[3 * j + 1], dz = zi - xq[3 * j + 2];
            double e, k;
            lj_pair(dx * dx + dy * dy + dz * dz, sxi * C.sx[j], sDi * C.sD[j], C.P, e, k);
            ei += 0.5 * C.P.w_intra * e;            // every pair is seen from both of its atoms
            k *= C.P.w_intra;
            gx += k * dx;
            gy += k * dy;
            gz += k * dz;
        }
        const int di = C.deg[i];
        if (lane < di) {                            // one bond per lane
            const int j = C.nbr[i * MOL_DEG + lane];
            const double dx = xi - xq[3 * j], dy = yi - xq[3 * j + 1], dz = zi - xq[3 * j + 2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz), dl = d - 0.005 * (double)C.r0h[i * MOL_DEG + lane];
            if (i < j) eb += 0.5 * C.P.k_b * dl * dl;
            if (d >= 1e-6) {
                const double k = C.P.k_b * dl / d;
                gx += k * dx;
                gy += k * dy;
                gz += k * dz;
            }
        }
        if (lane < 15) {                            // the angles at i
            int a, b;
            pair_slots(lane, a, b);
            if (b < di)
                ea += angle_term(C, xq, C.nbr[i * MOL_DEG + a], i, C.nbr[i * MOL_DEG + b], (C.acls[i] >> (2 * lane)) & 3u, true, gx, gy, gz);
        } else if (lane < 45) {                     // the angles i is an end of: neighbour s of i, its t-th other neighbour
            const int s = (lane - 15) / 5, t = (lane - 15) % 5;
            if (s < di) {
                const int c = C.nbr[i * MOL_DEG + s], dc = C.deg[c];
                int at = 0;
                while (at < dc && C.nbr[c * MOL_DEG + at] != i) ++at;
                const int o = t < at ? t : t + 1;
                if (at < dc && o < dc) {
                    const unsigned cls = (C.acls[c] >> (2 * pair_index(min(at, o), max(at, o)))) & 3u;
                    double unused = angle_term(C, xq, i, c, C.nbr[c * MOL_DEG + o], cls, false, gx, gy, gz);
                    (void)unused;
                }
            }
        }
        gx = wave_sum(gx);
        gy = wave_sum(gy);
        gz = wave_sum(gz);
        eb = wave_sum(eb);
        ea = wave_sum(ea);
        ei = wave_sum(ei);
        ep = wave_sum(ep);
        if (lane == 0) {
            gq[3 * i] = gx;
            gq[3 * i + 1] = gy;
            gq[3 * i + 2] = gz;
            C.epart[4 * i] = eb;
            C.epart[4 * i + 1] = ea;
            C.epart[4 * i + 2] = ei;
            C.epart[4 * i + 3] = ep;
        }
    }
    __syncthreads();
    if (wv == 0) {
        double part[4] = {0.0, 0.0, 0.0, 0.0}, gm = 0.0;
        for (int i = lane; i < C.n; i += 64) {
#pragma unroll
            for (int k = 0; k < 4; ++k) part[k] += C.epart[4 * i + k];
            gm = fmax(gm, sqrt(gq[3 * i] * gq[3 * i] + gq[3 * i + 1] * gq[3 * i + 1] + gq[3 * i + 2] * gq[3 * i + 2]));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) part[k] = wave_sum(part[k]);
        gm = wave_max(gm);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) C.scal[k] = part[k];
            C.scal[4] = ((part[0] + part[1]) + part[2]) + part[3];
            C.scal[5] = gm;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(RX_T)
k_relax(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, int nm, const int *__restrict__ elem, int F,
        const int *__restrict__ zs, const float *__restrict__ lig_vdw, const int *__restrict__ bond_ij, const int *__restrict__ bond_ptr,
        int cap_bonds, const int *__restrict__ mol_status, const float *__restrict__ pocket_x, const float *__restrict__ pocket_vdw,
        const int *__restrict__ pocket_ptr, int n_pocket, int n_pockets, int stage_cap, const int *__restrict__ pocket_of, RelaxP P,
        float *__restrict__ pos_out, double *__restrict__ report, int *__restrict__ status) {
    extern __shared__ double lds_d[];
    char *lds = reinterpret_cast<char *>(lds_d);
    const RelaxLayout L = relax_layout(nm, stage_cap);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int V = 3 * nm;                            // stride of the state vectors
    double *x = reinterpret_cast<double *>(lds + L.vec), *g = x + V, *p = g + V, *xt = p + V, *gt = xt + V, *S = gt + V,
           *Y = S + RX_M * V;
    double *sx = reinterpret_cast<double *>(lds + L.sx), *sD = reinterpret_cast<double *>(lds + L.sD);
    double *red = reinterpret_cast<double *>(lds + L.red), *scal = reinterpret_cast<double *>(lds + L.scal);
    double *rho = reinterpret_cast<double *>(lds + L.rho);
    double *psx = reinterpret_cast<double *>(lds + L.psx), *psD = reinterpret_cast<double *>(lds + L.psD);
    float *x0 = reinterpret_cast<float *>(lds + L.x0), *px = reinterpret_cast<float *>(lds + L.px);
    unsigned *excl = reinterpret_cast<unsigned *>(lds + L.excl), *acls = reinterpret_cast<unsigned *>(lds + L.acls);
    int *deg = reinterpret_cast<int *>(lds + L.deg);
    unsigned short *r0h = reinterpret_cast<unsigned short *>(lds + L.r0h);
    unsigned char *nbr = reinterpret_cast<unsigned char *>(lds + L.nbr);

    // ---- is there a molecule (bit 0), and its pocket (bit 1)?  Every `st` below is block-uniform.
    LigandInPocket lp;
    int st = ligand_in_pocket(lig_ptr, b, n_atoms, nm, bond_ptr, cap_bonds, mol_status, pocket_of, pocket_ptr, n_pocket, n_pockets, lp);
    const int a0 = lp.a0, n = lp.n, p0 = lp.p0, p1 = lp.p1, q0 = lp.q0, np = lp.np;
    if (!st) {
        int bad = 0;
        for (int a = tid; a < n; a += RX_T) {
            deg[a] = 0;
            acls[a] = 0;
            const size_t ga = (size_t)(a0 + a);
            const int e = elem[ga];
            if (e < 0 || e >= F) {
                bad |= LP_NO_MOLECULE;
                continue;
            }
            const float vx = lig_vdw[2 * e], vD = lig_vdw[2 * e + 1];
            if (!(finite_f(vx) && finite_f(vD) && vx > 0.0f && vD >= 0.0f)) bad |= LP_BAD_INPUT;
            sx[a] = sqrt((double)vx);
            sD[a] = sqrt((double)vD);
            for (int k = 0; k < 3; ++k) {
                const float v = pos[ga * 3 + k];
                if (!finite_f(v)) bad |= LP_BAD_INPUT;
                x0[3 * a + k] = v;
                x[3 * a + k] = (double)v;
            }
        }
        const int stage = min(np, stage_cap);
        for (int j = tid; j < np; j += RX_T) {       // every pocket atom is checked, the first `stage` are kept
            const float *r = pocket_x + (size_t)(q0 + j) * 3, *v = pocket_vdw + (size_t)(q0 + j) * 2;
            if (!(finite_f(r[0]) && finite_f(r[1]) && finite_f(r[2]) && finite_f(v[0]) && finite_f(v[1]) && v[0] > 0.0f && v[1] >= 0.0f))
                bad |= LP_BAD_INPUT;
            if (j < stage) {
                px[3 * j] = r[0];
                px[3 * j + 1] = r[1];
                px[3 * j + 2] = r[2];
                psx[j] = sqrt((double)v[0]);
                psD[j] = sqrt((double)v[1]);
            }
        }
        st = lp_votes(bad);
    }
    if (!st) {                                       // neighbour lists from the bond list
        int bad = 0;
        for (int k = p0 + tid; k < p1; k += RX_T) {
            const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0;
            if (i < 0 || i >= n || j < 0 || j >= n || i == j) {
                bad = 1;
                continue;
            }
            const int si = atomicAdd(&deg[i], 1), sj = atomicAdd(&deg[j], 1);
            if (si >= MOL_DEG || sj >= MOL_DEG) {      // a seventh neighbour
                bad = 1;
                continue;
            }
            nbr[i * MOL_DEG + si] = (unsigned char)j;
            nbr[j * MOL_DEG + sj] = (unsigned char)i;
        }
        st = __syncthreads_or(bad) ? LP_NO_MOLECULE : 0;
    }
    if (!st) {                                       // sorted lists (the atomics above have no order), rest lengths
        int bad = 0;
        for (int i = tid; i < n; i += RX_T) {
            const int di = deg[i];
            unsigned char *l = nbr + i * MOL_DEG;
            for (int a = 1; a < di; ++a)
                for (int c = a; c > 0 && l[c - 1] > l[c]; --c) {
                    const unsigned char t = l[c];
                    l[c] = l[c - 1];
                    l[c - 1] = t;
                }
            const unsigned ri = element_row(zs[elem[a0 + i]]);
            for (int a = 0; a < di; ++a) {
                const int j = l[a];
                if (a && l[a - 1] == l[a]) bad = 1;  // a bond twice
                const unsigned rj = element_row(zs[elem[a0 + j]]);
                const int s1 = (int)(ri & 0xffu), t1 = (int)(rj & 0xffu), s2 = (int)((ri >> 8) & 0xffu), t2 = (int)((rj >> 8) & 0xffu),
                          s3 = (int)((ri >> 16) & 0xffu), t3 = (int)((rj >> 16) & 0xffu);
                if (!s1 || !t1) {                    // an element the bond rule never bonds
                    bad = 1;
                    continue;
                }
                const double dx = (double)x0[3 * i] - (double)x0[3 * j], dy = (double)x0[3 * i + 1] - (double)x0[3 * j + 1],
                             dz = (double)x0[3 * i + 2] - (double)x0[3 * j + 2];
                const double d = sqrt(dx * dx + dy * dy + dz * dz);
                // candidates in half picometres, ascending: L3, L2, L15, L1; the nearest wins, the longer one on a tie
                const int h1 = 2 * (s1 + t1), h2 = (s2 && t2) ? 2 * (s2 + t2) : 0, h3 = (s3 && t3) ? 2 * (s3 + t3) : 0;
                const int cand[4] = {h3, h2, h2 ? (h1 + h2) / 2 : 0, h1};
                int best = 0;
                double bd = 0.0;
                for (int c = 0; c < 4; ++c) {
                    if (!cand[c]) continue;
                    const double off = fabs(d - 0.005 * (double)cand[c]);
                    if (!best || off < bd || (off == bd && cand[c] > best)) {
                        best = cand[c];
                        bd = off;
                    }
                }
                r0h[i * MOL_DEG + a] = (unsigned short)best;
            }
        }
        st = __syncthreads_or(bad) ? LP_NO_MOLECULE : 0;
    }
    if (st) {                                        // left out: pos_out keeps the input rows the host copied
        if (tid < 12) report[(size_t)b * 12 + tid] = 0.0;
        if (tid == 0) status[b] = st;
        return;
    }
    RelaxCtx C;
    C.n = n;
    C.np = np;
    C.stage = min(np, stage_cap);
    C.W = L.W;
    C.sx = sx;
    C.sD = sD;
    C.psx = psx;
    C.psD = psD;
    C.x0 = x0;
    C.px = px;
    C.gpx = pocket_x + (size_t)q0 * 3;
    C.gpv = pocket_vdw + (size_t)q0 * 2;
    C.excl = excl;
    C.acls = acls;
    C.deg = deg;
    C.r0h = r0h;
    C.nbr = nbr;
    C.epart = reinterpret_cast<double *>(lds + L.epart);
    C.red = red;
    C.scal = scal;
    C.P = P;
    // pairs one or two bonds apart (and i itself) are no non-bonded pairs; the rest class of every angle
    for (int i = tid; i < n; i += RX_T) {
        unsigned *row = excl + i * L.W;
        for (int w = 0; w < L.W; ++w) row[w] = 0;
        row[i >> 5] |= 1u << (i & 31);
        const int di = deg[i];
        unsigned cls = 0;
        for (int a = 0; a < di; ++a) {
            const int j = nbr[i * MOL_DEG + a];
            row[j >> 5] |= 1u << (j & 31);
            for (int c = 0; c < deg[j]; ++c) {
                const int k = nbr[j * MOL_DEG + c];
                row[k >> 5] |= 1u << (k & 31);
            }
            for (int c = a + 1; c < di; ++c) {
                double u[3], w[3], uu, ww, inv, cs = 0.0;
                unsigned code = 0;                   // keep the sampled angle (also when it cannot be measured)
                if (angle_cos(x0, j, i, (int)nbr[i * MOL_DEG + c], u, w, uu, ww, inv, cs) && !(cs > RX_COS100))
                    code = di >= 4 ? 1u : cs <= RX_COS150 ? 3u : cs <= RX_COS114 ? 2u : 1u;
                cls |= code << (2 * pair_index(a, c));
            }
        }
        acls[i] = cls;
    }
    __syncthreads();

    const int N3 = 3 * n;
    relax_eval(C, x, g, tid);
    double part[4] = {scal[0], scal[1], scal[2], scal[3]}, E = scal[4], gmax = scal[5];
    const double E_before = E, pocket_before = part[3], gmax_before = gmax, part0[4] = {part[0], part[1], part[2], part[3]};
    int m = 0, head = 0, iters = 0, evals = 1;
    double gamma = 1.0;
    for (int it = 0; it < P.max_iters; ++it) {
        if (gmax <= P.gtol) break;
        ++iters;
        // direction: the two-loop recursion over the m newest pairs, p = -H g
        for (int k = tid; k < N3; k += RX_T) p[k] = g[k];
        __syncthreads();
        double al[RX_M];
#pragma unroll
        for (int k = 0; k < RX_M; ++k) {             // newest first
            al[k] = 0.0;
            if (k < m) {
                const int slot = (head + RX_M - 1 - k) & (RX_M - 1);
                al[k] = rho[slot] * block_dot(S + slot * V, p, N3, red, tid);
                for (int e = tid; e < N3; e += RX_T) p[e] -= al[k] * Y[slot * V + e];
                __syncthreads();
            }
        }
        if (m) {
            for (int e = tid; e < N3; e += RX_T) p[e] *= gamma;
            __syncthreads();
        }
#pragma unroll
        for (int k = RX_M - 1; k >= 0; --k) {        // oldest first
            if (k < m) {
                const int slot = (head + RX_M - 1 - k) & (RX_M - 1);
                const double be = rho[slot] * block_dot(Y + slot * V, p, N3, red, tid);
                for (int e = tid; e < N3; e += RX_T) p[e] += (al[k] - be) * S[slot * V + e];
                __syncthreads();
            }
        }
        for (int k = tid; k < N3; k += RX_T) p[k] = -p[k];
        __syncthreads();
        double gp = block_dot(g, p, N3, red, tid);
        if (!(gp < 0.0)) {                           // no descent direction: forget the pairs
            m = 0;
            for (int k = tid; k < N3; k += RX_T) p[k] = -g[k];
            __syncthreads();
            gp = -block_dot(g, g, N3, red, tid);
        }
        const double pmax = block_max_norm(p, n, red, tid);
        double alpha = fmin(1.0, P.max_step / pmax);
        bool accepted = false;
        for (int ls = 0; ls <= 20; ++ls) {
            for (int k = tid; k < N3; k += RX_T) xt[k] = x[k] + alpha * p[k];
            __syncthreads();
            relax_eval(C, xt, gt, tid);
            ++evals;
            const double Et = scal[4];
            if (fabs(Et) < __builtin_inf() && Et <= E + 1e-4 * alpha * gp) {
                accepted = true;
                break;
            }
            alpha *= 0.5;
        }
        if (!accepted) {
            if (m) {                                 // try again along -g
                m = 0;
                continue;
            }
            st |= RX_LINE_SEARCH;
            break;
        }
        double *s_new = S + head * V, *y_new = Y + head * V;
        for (int k = tid; k < N3; k += RX_T) {
            s_new[k] = xt[k] - x[k];
            y_new[k] = gt[k] - g[k];
            x[k] = xt[k];
            g[k] = gt[k];
        }
        __syncthreads();
        const double sy = block_dot(s_new, y_new, N3, red, tid), yy = block_dot(y_new, y_new, N3, red, tid),
                     gg = block_dot(g, g, N3, red, tid);
        if (sy > 1e-10 * yy && yy > 1e-20 * gg) {       // the second test: where the energy is linear, y is rounding noise
            if (tid == 0) rho[head] = 1.0 / sy;
            gamma = sy / yy;
            head = (head + 1) & (RX_M - 1);
            m = min(m + 1, RX_M);
        }
        E = scal[4];
        gmax = scal[5];
#pragma unroll
        for (int k = 0; k < 4; ++k) part[k] = scal[k];
        __syncthreads();                             // rho is read, and scal written again, only behind this
    }
    // The report describes the rows written: where the ligand moved, the energy is evaluated once more at the fp32-rounded
    // positions.  Should that rounding alone turn the (then tiny) gain into a rise, the ligand keeps its input rows.
    if (iters) {
        for (int k = tid; k < N3; k += RX_T) xt[k] = (double)(float)x[k];
        __syncthreads();
        relax_eval(C, xt, gt, tid);
        ++evals;
        const bool keep = scal[4] <= E_before;
        E = keep ? scal[4] : E_before;
        gmax = keep ? scal[5] : gmax_before;
#pragma unroll
        for (int k = 0; k < 4; ++k) part[k] = keep ? scal[k] : part0[k];
        for (int k = tid; k < N3; k += RX_T) x[k] = keep ? xt[k] : (double)x0[k];
        __syncthreads();
    }
    if (gmax > P.gtol && !(st & RX_LINE_SEARCH)) st |= RX_ITER_CAP;

    double sq = 0.0;
    for (int k = tid; k < N3; k += RX_T) {
        const float v = (float)x[k];
        pos_out[(size_t)a0 * 3 + k] = v;
        const double d = (double)v - (double)x0[k];
        sq += d * d;
    }
    sq = wave_sum(sq);
    if ((tid & 63) == 0) red[tid >> 6] = sq;
    __syncthreads();
    if (tid == 0) {
        double *r = report + (size_t)b * 12;
        r[0] = E_before;
        r[1] = E;
        r[2] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)n);
        r[3] = gmax;
        r[4] = (double)iters;
        r[5] = (double)evals;
        r[6] = part[0];
        r[7] = part[1];
        r[8] = part[2];
        r[9] = part[3];
        r[10] = pocket_before;
        r[11] = gmax_before;
        status[b] = st;
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_relax(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms,
                                const int32_t *elem, int32_t F, const int32_t *z, const float *lig_vdw, const int32_t *bond_ij,
                                const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status, const float *pocket_x,
                                const float *pocket_vdw, const int32_t *pocket_ptr, int32_t n_pocket, int32_t P, int32_t max_pocket,
                                const int32_t *pocket_of, const kpd_relax_params *params, float *pos_out, double *report,
                                int32_t *status, void *stream) {
    KPD_TRY(ligand_pocket_args(n_atoms, B, max_atoms, F, cap_bonds, n_pocket, P, max_pocket, lig_ptr && z && lig_vdw && bond_ptr,
                               pos && elem && pos_out, mol_status && pocket_of && report && status, bond_ij, pocket_ptr,
                               pocket_x && pocket_vdw));
    kpd_relax_params d;
    kpd_relax_defaults(&d);
    if (params) d = *params;
    KPD_REQUIRE(d.k_b >= 0.0 && d.k_a >= 0.0 && d.r_c > 0.0 && d.s > 0.0 && d.s < 1.0 && d.w_intra >= 0.0 && d.gtol >= 0.0 &&
                    d.max_step > 0.0 && d.max_iters >= 0 && d.r_c < 1e6 && d.k_b < 1e12 && d.k_a < 1e12 && d.w_intra < 1e12,
                KPD_ERR_INVALID, "k_b=%g k_a=%g r_c=%g s=%g (0 .. 1) w_intra=%g gtol=%g max_step=%g max_iters=%d", d.k_b, d.k_a, d.r_c, d.s,
                d.w_intra, d.gtol, d.max_step, d.max_iters);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_atoms && pos_out != pos) KPD_HIP(hipMemcpyAsync(pos_out, pos, (size_t)n_atoms * 12, hipMemcpyDeviceToDevice, st));
    if (!B) return KPD_OK;
    const double s6 = 1.0 / (d.s * d.s * d.s * d.s * d.s * d.s);
    RelaxP rp;
    rp.k_b = d.k_b;
    rp.k_a = d.k_a;
    rp.rc2 = d.r_c * d.r_c;
    rp.inv_rc2 = 1.0 / rp.rc2;
    rp.s = d.s;
    rp.ce = s6 * s6 - 2.0 * s6;
    rp.cf = s6 * s6 - s6;
    rp.w_intra = d.w_intra;
    rp.gtol = d.gtol;
    rp.max_step = d.max_step;
    rp.max_iters = d.max_iters;
    // as much of the largest pocket as fits beside the state of a max_atoms ligand
    const int stage = stage_rows(relax_layout(max_atoms, 0).bytes, RX_LDS, RX_POCKET_ROW, max_pocket);
    KPD_REQUIRE(stage >= 0, KPD_ERR_INVALID, "no LDS for %d atoms", max_atoms);
    const RelaxLayout L = relax_layout(max_atoms, stage);
    KPD_REQUIRE(L.bytes <= (size_t)RX_LDS, KPD_ERR_INVALID, "LDS layout of %zu bytes", L.bytes);
    KPD_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(k_relax), (int)L.bytes));
    hipLaunchKernelGGL(k_relax, dim3(B), dim3(RX_T), L.bytes, st, pos, lig_ptr, n_atoms, max_atoms, elem, F, z, lig_vdw, bond_ij, bond_ptr,
                       cap_bonds, mol_status, pocket_x, pocket_vdw, pocket_ptr, n_pocket, P, stage, pocket_of, rp, pos_out, report, status);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" void kpd_relax_defaults(kpd_relax_params *p) {
    if (!p) return;
    p->k_b = 700.0;
    p->k_a = 200.0;
    p->r_c = 10.0;
    p->s = 0.6;
    p->w_intra = 1.0;
    p->gtol = 1e-3;
    p->max_step = 0.2;
    p->max_iters = 400;
}
