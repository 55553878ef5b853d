// Local minimisation of sampled ligands under the Vina-form score of vina.hip, over rigid-body and torsional degrees of freedom:
// the step upstream runs as `gnina --minimize` (analysis/docking/gen_docking_cmds.py --minimize).  include/kpd.h DEFINES the torsion
// tree, the chart, the intramolecular term and the minimiser; typing, rotor rule, pair terms and constants are those of
// kpd_vina_score.  NOT gnina's or Vina's numbers.
// k_vina_minimize: one workgroup (4 waves) per ligand and ONE launch for the whole minimisation of every ligand.  Once per ligand:
// the bond graph as a bit matrix in LDS, typing, the rotor list in bond order, the moved set of every active rotor as a bit set
// (one thread per rotor walks the graph without its bond), piece labels by label propagation, the mask of intramolecular pairs.
// One evaluation: an atom's pocket and intramolecular terms and its Cartesian gradient are summed by one wavefront (lanes stride the
// pocket atoms, then the ligand's own, and meet in a butterfly); the projection on the pose coordinates takes one wavefront per
// body or rotor over its atom set.  The pose vectors have at most 112 entries, so the two-loop recursion and every dot product of
// the L-BFGS run on one wavefront, two entries per lane.  Nothing is shared between ligands, no atomics on floats, no host
// synchronisation: a ligand's result is bitwise independent of the batch, of what was staged, of the bounds, and of the repeat.
// The layout, the evaluation, the projection, the recursion and the chart are in vina_min_core.h, which vina_dock.hip shares.
#include "vina_min_core.h"

namespace kpd {

// Three waves per SIMD: the compiler's own choice is 173 VGPRs, one short of that; bounded to 168 it spills four of them (20 B of
// scratch per lane) and the third workgroup on a compute unit more than pays for it (profiles/vina_min.md).
__global__ void __launch_bounds__(VN_T) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_vina_minimize(const float *pos, const int *__restrict__ lig_ptr, int n_atoms, int nm, const int *__restrict__ elem, int F,
                const int *__restrict__ zs, const float *__restrict__ lig_radius, const int *__restrict__ frag,
                const int *__restrict__ bond_ij, const int *__restrict__ bond_order, const int *__restrict__ bond_ptr, int cap_bonds,
                const int *__restrict__ mol_status, const int *__restrict__ lig_type_in, const float *__restrict__ pocket_x,
                const float *__restrict__ pocket_radius, const int *__restrict__ pocket_type, const int *__restrict__ pocket_ptr,
                int n_pocket, int n_pockets, int stage_cap, const int *__restrict__ pocket_of, int max_rotors, VinaMinP P,
                float *pos_out, double *__restrict__ report, int *__restrict__ status) {      // pos_out may be pos: no __restrict__ on the two
    extern __shared__ double lds_d[];
    char *lds = reinterpret_cast<char *>(lds_d);
    const VinaMinLayout L = vina_min_layout(nm, max_rotors, stage_cap);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, W = L.W, DS = L.DS;
    double *x = reinterpret_cast<double *>(lds + L.x), *xt = reinterpret_cast<double *>(lds + L.xt);
    double *g = reinterpret_cast<double *>(lds + L.g);
    double *gd = reinterpret_cast<double *>(lds + L.vec), *gdt = gd + DS, *p = gdt + DS, *S = p + DS, *Y = S + VM_M * DS;
    double *rho = reinterpret_cast<double *>(lds + L.rho), *scal = reinterpret_cast<double *>(lds + L.scal);
    double *red = reinterpret_cast<double *>(lds + L.red);
    float *x0 = reinterpret_cast<float *>(lds + L.x0), *rad = reinterpret_cast<float *>(lds + L.rad);
    int *zat = reinterpret_cast<int *>(lds + L.zat), *typ = reinterpret_cast<int *>(lds + L.typ);
    unsigned *cnt = reinterpret_cast<unsigned *>(lds + L.cnt), *flg = reinterpret_cast<unsigned *>(lds + L.flg);
    int *frg = reinterpret_cast<int *>(lds + L.frg), *piece = reinterpret_cast<int *>(lds + L.piece);
    unsigned *adj = reinterpret_cast<unsigned *>(lds + L.adj), *adjp = reinterpret_cast<unsigned *>(lds + L.adjp);
    unsigned *imask = reinterpret_cast<unsigned *>(lds + L.imask), *mset = reinterpret_cast<unsigned *>(lds + L.mset);
    unsigned *fset = reinterpret_cast<unsigned *>(lds + L.fset);
    int *ra = reinterpret_cast<int *>(lds + L.ra), *rb = reinterpret_cast<int *>(lds + L.rb);
    int *depth = reinterpret_cast<int *>(lds + L.depth), *ord = reinterpret_cast<int *>(lds + L.ord);
    int *flow = reinterpret_cast<int *>(lds + L.flow), *fcnt = reinterpret_cast<int *>(lds + L.fcnt);
    unsigned char *rflag = reinterpret_cast<unsigned char *>(lds + L.rflag);
    float *px = reinterpret_cast<float *>(lds + L.px), *prad = reinterpret_cast<float *>(lds + L.prad);
    int *ptyp = reinterpret_cast<int *>(lds + L.ptyp);

    // ---- is there a molecule (bit 0), and its pocket (bit 1)?  Every `st` below is block-uniform.
    LigandInPocket lp;
    int st = ligand_in_pocket(lig_ptr, b, n_atoms, nm, bond_ptr, cap_bonds, mol_status, pocket_of, pocket_ptr, n_pocket, n_pockets, lp);
    const int a0 = lp.a0, n = lp.n, p0 = lp.p0, p1 = lp.p1, q0 = lp.q0, np = lp.np;
    const int stage = min(np, stage_cap);
    int atom_out = 0;
    if (!st) {
        if (tid < VM_FRAGS) {
            flow[tid] = MOL_MAX;
            fcnt[tid] = 0;
        }
        for (int k = tid; k < VM_FRAGS * W; k += VN_T) fset[k] = 0;
        int bad = 0;
        for (int a = tid; a < n; a += VN_T) {        // k_vina_score's atom staging, plus the fragment label and the fp64 copy
            cnt[a] = 0;
            flg[a] = 0;
            zat[a] = 0;
            rad[a] = 0.f;
            frg[a] = 0;
            for (int w = 0; w < W; ++w) adj[a * W + w] = 0;
            const size_t ga = (size_t)(a0 + a);
            const int e = elem[ga], fl = frag[ga];
            if (e < 0 || e >= F || fl < 0 || fl >= n) {
                bad |= LP_NO_MOLECULE;
                continue;
            }
            frg[a] = fl;
            const float rv = lig_radius[e];
            if (!finite_f(rv)) bad |= LP_BAD_INPUT;
            rad[a] = rv;
            zat[a] = zs[e];
            for (int k = 0; k < 3; ++k) {
                const float v = pos[ga * 3 + k];
                if (!finite_f(v)) bad |= LP_BAD_INPUT;
                x0[3 * a + k] = v;
                x[3 * a + k] = (double)v;
            }
        }
        vina_stage_pocket(pocket_x, pocket_radius, pocket_type, q0, np, stage, tid, px, prad, ptyp, bad, atom_out);
        st = lp_votes(bad);
    }
    int n_frag = 0;
    if (!st) {                                       // the bond graph: bond_ij holds i < j inside one fragment; then the fragments
        const int bad = vina_bond_graph<true, true>(bond_ij, bond_order, p0, p1, a0, n, W, tid, zat, frg, adj, cnt, flg);
        int top = 0;
        for (int a = tid; a < n; a += VN_T) {
            const int fl = frg[a];
            top = max(top, fl);
            if (fl < VM_FRAGS) {
                atomicMin(&flow[fl], a);
                atomicAdd(&fcnt[fl], 1);
                atomicOr(&fset[fl * W + (a >> 5)], 1u << (a & 31));
            }
        }
        st = __syncthreads_or(bad) ? LP_NO_MOLECULE : 0;
        const int many = __syncthreads_or(top >= VM_FRAGS);
        if (!st && many) st = VM_FRAGMENTS;
        if (!st) {                                   // labels 0 .. n_frag - 1, every one of them used
            int hole = 0;
            for (int f = 0; f < VM_FRAGS; ++f) {
                if (fcnt[f]) {
                    if (f != n_frag) hole = 1;
                    ++n_frag;
                }
            }
            if (hole) st = LP_NO_MOLECULE;
        }
    }
    if (st) {                                        // left out: pos_out keeps the input rows the host copied
        if (tid < 16) report[(size_t)b * 16 + tid] = 0.0;
        if (tid == 0) status[b] = st;
        return;
    }
    // ---- types
    vina_type_atoms(n, a0, tid, zat, cnt, flg, rad, lig_type_in, typ, nullptr, atom_out);
    // ---- rotors in bond order: single bonds between atoms of heavy degree >= 2 that are in no ring
    const int nb = min(p1 - p0, 3 * nm);             // a graph that passed the checks has at most 3 n bonds
    for (int k = tid; k < nb; k += VN_T) {
        int is = 0;
        if (bond_order[p0 + k] == 1) {
            const int i = bond_ij[(size_t)(p0 + k) * 2] - a0, j = bond_ij[(size_t)(p0 + k) * 2 + 1] - a0;
            if (((cnt[i] >> 4) & 15u) >= 2u && ((cnt[j] >> 4) & 15u) >= 2u) {
                unsigned vis[MOL_W];
                vina_walk<false>(adj, W, j, i, vis);
                unsigned hit = 0;
#pragma unroll
                for (int w = 0; w < MOL_W; ++w)
                    if (w == (i >> 5)) hit = vis[w] & (1u << (i & 31));
                is = hit ? 0 : 1;
            }
        }
        rflag[k] = (unsigned char)is;
    }
    if (__syncthreads_or(atom_out)) st |= VN_ATOM_OUT;   // also orders typ and rflag before their readers
    int *redi = reinterpret_cast<int *>(red);
    if (wv == 0) {                                   // the first max_rotors of them are active
        int base = 0;
        for (int c = 0; c < nb; c += 64) {
            const int k = c + lane;
            const int is = k < nb ? rflag[k] : 0;
            const unsigned long long m = __ballot(is);
            const int rank = base + __popcll(m & ((1ull << lane) - 1ull));
            if (is && rank < max_rotors) {
                ra[rank] = bond_ij[(size_t)(p0 + k) * 2] - a0;
                rb[rank] = bond_ij[(size_t)(p0 + k) * 2 + 1] - a0;
            }
            base += __popcll(m);
        }
        if (lane == 0) redi[0] = base;
    }
    __syncthreads();
    const int n_rot = redi[0], T = min(n_rot, max_rotors), D = 6 * n_frag + T;
    if (n_rot > T) st |= VM_FROZEN;
    const double inv_norm = 1.0 / (1.0 + P.w_rot * (double)n_rot);
    // ---- the moved set of every active rotor (i, j): the side of j, or the rest of the fragment when that side holds its lowest atom
    for (int a = tid; a < n; a += VN_T)
        for (int w = 0; w < W; ++w) adjp[a * W + w] = adj[a * W + w];
    if (tid < T) {
        const int i = ra[tid], j = rb[tid], low = flow[frg[j]];
        unsigned vis[MOL_W];
        vina_walk<false>(adj, W, j, i, vis);
        unsigned hit = 0;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w)
            if (w == (low >> 5)) hit = vis[w] & (1u << (low & 31));
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            if (w >= W) continue;
            mset[tid * W + w] = hit ? fset[frg[j] * W + w] & ~vis[w] : vis[w];
        }
        if (hit) {                                   // b is the end that moves, a the other one
            ra[tid] = j;
            rb[tid] = i;
        }
    }
    __syncthreads();
    if (tid < T) {                                   // pieces: the graph without the active rotor bonds
        const int i = ra[tid], j = rb[tid];
        atomicAnd(&adjp[i * W + (j >> 5)], ~(1u << (j & 31)));
        atomicAnd(&adjp[j * W + (i >> 5)], ~(1u << (i & 31)));
        int d = 0;
        for (int k = 0; k < T; ++k) d += vm_bit(mset + k * W, rb[tid]) ? 1 : 0;
        depth[tid] = d;
    }
    for (int a = tid; a < n; a += VN_T) piece[a] = a;
    __syncthreads();
    if (tid == 0) {                                  // rotors from the deepest to the shallowest, by index within one depth
        for (int k = 0; k < T; ++k) {
            int c = k;
            while (c > 0 && depth[ord[c - 1]] < depth[k]) {
                ord[c] = ord[c - 1];
                --c;
            }
            ord[c] = k;
        }
    }
    // Label propagation: the fixed point is the lowest atom of every piece.  A sweep reads labels that other threads are lowering in
    // the same sweep (aligned 32-bit words, no barrier between): a label only ever decreases and always names an atom of the same
    // piece, so a stale read merely delays the descent, and the loop ends on a sweep in which nobody wrote, which has no race.  The
    // result does not depend on the interleaving.
    for (;;) {
        int changed = 0;
        for (int a = tid; a < n; a += VN_T) {
            int l = piece[a];
            const int before = l;
            for (int w = 0; w < W; ++w) {
                unsigned bits = adjp[a * W + w];
                while (bits) {
                    l = min(l, piece[32 * w + __ffs(bits) - 1]);
                    bits &= bits - 1;
                }
            }
            l = min(l, piece[l]);
            if (l != before) {
                piece[a] = l;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // ---- intramolecular pairs: both atoms take part, different pieces, four or more bonds apart or not connected
    for (int a = tid; a < n; a += VN_T) {
        unsigned e1[MOL_W], e2[MOL_W], e3[MOL_W];
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            e1[w] = w < W ? adj[a * W + w] : 0u;
            if (w == (a >> 5)) e1[w] |= 1u << (a & 31);
            e2[w] = e1[w];
        }
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            unsigned bits = e1[w];
            while (bits) {
                const int j = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1;
#pragma unroll
                for (int v = 0; v < MOL_W; ++v)
                    if (v < W) e2[v] |= adj[j * W + v];
            }
        }
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) e3[w] = e2[w];
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            unsigned bits = e2[w];
            while (bits) {
                const int j = 32 * w + __ffs(bits) - 1;
                bits &= bits - 1;
#pragma unroll
                for (int v = 0; v < MOL_W; ++v)
                    if (v < W) e3[v] |= adj[j * W + v];
            }
        }
        const int pa = piece[a];
        const bool on = typ[a] >= 0;
#pragma unroll
        for (int w = 0; w < MOL_W; ++w) {
            if (w >= W) continue;
            unsigned m = 0;
            for (int j = 32 * w; j < min(n, 32 * w + 32); ++j)
                if (on && typ[j] >= 0 && piece[j] != pa) m |= 1u << (j & 31);
            imask[a * W + w] = m & ~e3[w];
        }
    }
    __syncthreads();

    VinaMinCtx C;
    C.n = n;
    C.np = np;
    C.stage = stage;
    C.W = W;
    C.F = n_frag;
    C.T = T;
    C.D = D;
    C.rad = rad;
    C.px = px;
    C.prad = prad;
    C.gpx = pocket_x + (size_t)q0 * 3;
    C.gpr = pocket_radius + q0;
    C.typ = typ;
    C.ptyp = ptyp;
    C.gpt = pocket_type + q0;
    C.frg = frg;
    C.ra = ra;
    C.rb = rb;
    C.ord = ord;
    C.fcnt = fcnt;
    C.imask = imask;
    C.mset = mset;
    C.part = reinterpret_cast<double *>(lds + L.part);
    C.scal = scal;
    C.red = red;
    C.cen = reinterpret_cast<double *>(lds + L.cen);
    C.axu = reinterpret_cast<double *>(lds + L.axu);
    C.trig = reinterpret_cast<double *>(lds + L.trig);
    C.body = reinterpret_cast<double *>(lds + L.body);
    C.P = P;

    const int N3 = 3 * n;
    vm_eval(C, x, g, tid);
    double inter = scal[VS_INTER], intra = scal[VS_INTRA], E = scal[VS_E];
    vm_project(C, x, g, gd, tid);
    double gnorm = scal[VS_GNORM];
    const double E_before = E, inter_before = inter, intra_before = intra, gnorm_before = gnorm;
    int m = 0, head = 0, iters = 0, evals = 1;
    double gamma = 1.0;
    for (int it = 0; it < P.max_iters; ++it) {
        if (gnorm <= P.gtol) break;
        ++iters;
        if (wv == 0) vm_direction(gd, S, Y, rho, DS, D, m, head, gamma, p, scal, lane);
        __syncthreads();
        if (scal[VS_RESET] != 0.0) m = 0;
        const double gp = scal[VS_GP];
        const double vmax = vm_vmax(C, x, p, tid);
        double alpha = fmin(1.0, P.max_step / vmax);
        bool accepted = false;
        for (int ls = 0; ls <= 20; ++ls) {
            vm_move(C, x, p, alpha, xt, tid);
            vm_eval(C, xt, g, tid);
            ++evals;
            const double Et = scal[VS_E];
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
            st |= VM_LINE_SEARCH;
            break;
        }
        E = scal[VS_E];
        inter = scal[VS_INTER];
        intra = scal[VS_INTRA];
        vm_project(C, xt, g, gdt, tid);              // the new point's own chart
        gnorm = scal[VS_GNORM];
        for (int d = tid; d < D; d += VN_T) {
            S[head * DS + d] = alpha * p[d];
            Y[head * DS + d] = gdt[d] - gd[d];
        }
        __syncthreads();
        if (wv == 0) {
            const double sy = vm_dot(S + head * DS, Y + head * DS, D, lane), yy = vm_dot(Y + head * DS, Y + head * DS, D, lane),
                         gg = vm_dot(gdt, gdt, D, lane);
            if (lane == 0) {
                scal[VS_SY] = sy;
                scal[VS_YY] = yy;
                scal[VS_GG] = gg;
            }
        }
        __syncthreads();
        const double sy = scal[VS_SY], yy = scal[VS_YY], gg = scal[VS_GG];
        if (sy > 1e-10 * yy && yy > 1e-20 * gg) {       // the second test: where the energy is linear, y is rounding noise
            if (tid == 0) rho[head] = 1.0 / sy;
            gamma = sy / yy;
            head = (head + 1) & (VM_M - 1);
            m = min(m + 1, VM_M);
        }
        double *sw = x;
        x = xt;
        xt = sw;
        sw = gd;
        gd = gdt;
        gdt = sw;
        __syncthreads();                             // rho is read, and scal written again, only behind this
    }
    // The report describes the rows written: where the ligand moved, the score is evaluated once more at the fp32-rounded
    // positions.  Should that rounding alone turn the (then tiny) gain into a rise, the ligand keeps its input rows.
    bool keep = false;
    if (iters) {
        for (int k = tid; k < N3; k += VN_T) xt[k] = (double)(float)x[k];
        __syncthreads();
        vm_eval(C, xt, g, tid);
        ++evals;
        keep = scal[VS_E] <= E_before;
        E = keep ? scal[VS_E] : E_before;
        inter = keep ? scal[VS_INTER] : inter_before;
        intra = keep ? scal[VS_INTRA] : intra_before;
        vm_project(C, xt, g, gdt, tid);
        gnorm = keep ? scal[VS_GNORM] : gnorm_before;
    }
    if (gnorm > P.gtol && !(st & VM_LINE_SEARCH)) st |= VM_ITER_CAP;

    double sq = 0.0;
    for (int k = tid; k < N3; k += VN_T) {
        const float v = keep ? (float)xt[k] : x0[k];
        pos_out[(size_t)a0 * 3 + k] = v;
        const double d = (double)v - (double)x0[k];
        sq += d * d;
    }
    sq = wave_sum(sq);
    if (lane == 0) red[wv] = sq;
    __syncthreads();
    if (tid == 0) {
        double *r = report + (size_t)b * 16;
        r[0] = inter_before * inv_norm;
        r[1] = inter * inv_norm;
        r[2] = E_before;
        r[3] = E;
        r[4] = inter_before;
        r[5] = inter;
        r[6] = intra_before;
        r[7] = intra;
        r[8] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)n);
        r[9] = gnorm_before;
        r[10] = gnorm;
        r[11] = (double)iters;
        r[12] = (double)evals;
        r[13] = (double)n_rot;
        r[14] = (double)T;
        r[15] = (double)n_frag;
        status[b] = st;
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_vina_minimize(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms,
                                        const int32_t *elem, int32_t F, const int32_t *z, const float *lig_radius, const int32_t *frag,
                                        const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds,
                                        const int32_t *mol_status, const int32_t *lig_type_in, const float *pocket_x,
                                        const float *pocket_radius, const int32_t *pocket_type, const int32_t *pocket_ptr,
                                        int32_t n_pocket, int32_t P, int32_t max_pocket, const int32_t *pocket_of, int32_t max_rotors,
                                        const kpd_vina_min_params *params, float *pos_out, double *report, int32_t *status,
                                        void *stream) {
    KPD_TRY(ligand_pocket_args(n_atoms, B, max_atoms, F, cap_bonds, n_pocket, P, max_pocket, lig_ptr && z && lig_radius && bond_ptr,
                               pos && elem && frag && pos_out, mol_status && pocket_of && report && status, bond_ij && bond_order,
                               pocket_ptr, pocket_x && pocket_radius && pocket_type));
    KPD_REQUIRE(max_rotors >= 0 && max_rotors <= VM_ROTORS, KPD_ERR_INVALID, "max_rotors=%d (0 .. %d)", max_rotors, VM_ROTORS);
    kpd_vina_min_params d;
    kpd_vina_min_defaults(&d);
    if (params) d = *params;
    VinaMinP vp;
    KPD_TRY(vina_fill_params({d.w_gauss1, d.w_gauss2, d.w_repulsion, d.w_hydrophobic, d.w_hbond, d.w_rot, d.r_c}, vp));
    KPD_REQUIRE(d.w_intra >= 0.0 && d.w_intra < 1e12 && d.gtol >= 0.0 && d.max_step > 0.0 && d.max_iters >= 0, KPD_ERR_INVALID,
                "w_intra=%g gtol=%g (>= 0) max_step=%g (> 0) max_iters=%d", d.w_intra, d.gtol, d.max_step, d.max_iters);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_atoms && pos_out != pos) KPD_HIP(hipMemcpyAsync(pos_out, pos, (size_t)n_atoms * 12, hipMemcpyDeviceToDevice, st));
    if (!B) return KPD_OK;
    vp.w_intra = d.w_intra;
    vp.gtol = d.gtol;
    vp.max_step = d.max_step;
    vp.max_iters = d.max_iters;
    // as much of the largest pocket as fits beside the state of a max_atoms ligand
    const int stage = stage_rows(vina_min_layout(max_atoms, max_rotors, 0).bytes, VM_LDS, VN_POCKET_ROW, max_pocket);
    KPD_REQUIRE(stage >= 0, KPD_ERR_INVALID, "no LDS for %d atoms", max_atoms);
    const VinaMinLayout L = vina_min_layout(max_atoms, max_rotors, stage);
    KPD_REQUIRE(L.bytes <= (size_t)VM_LDS, KPD_ERR_INVALID, "LDS layout of %zu bytes", L.bytes);
    KPD_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(k_vina_minimize), (int)L.bytes));
    hipLaunchKernelGGL(k_vina_minimize, dim3(B), dim3(VN_T), L.bytes, st, pos, lig_ptr, n_atoms, max_atoms, elem, F, z, lig_radius, frag,
                       bond_ij, bond_order, bond_ptr, cap_bonds, mol_status, lig_type_in, pocket_x, pocket_radius, pocket_type, pocket_ptr,
                       n_pocket, P, stage, pocket_of, max_rotors, vp, pos_out, report, status);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" void kpd_vina_min_defaults(kpd_vina_min_params *p) {
    if (!p) return;
    kpd_vina_params v;
    kpd_vina_defaults(&v);
    p->w_gauss1 = v.w_gauss1;
    p->w_gauss2 = v.w_gauss2;
    p->w_repulsion = v.w_repulsion;
    p->w_hydrophobic = v.w_hydrophobic;
    p->w_hbond = v.w_hbond;
    p->w_rot = v.w_rot;
    p->r_c = v.r_c;
    p->w_intra = 1.0;
    p->gtol = 1e-3;
    p->max_step = 0.2;
    p->max_iters = 200;
}
