// Monte-Carlo search of sampled ligands in their pockets under the Vina-form score: the step upstream runs as gnina docking inside
// --autobox_ligand (analysis/docking/gen_docking_cmds.py without --minimize).  include/kpd.h DEFINES the search: the random
// streams, the start of a chain, a mutation, the box, the Metropolis rule, the refinement and the modes; typing, tree, chart,
// objective and minimiser are those of kpd_vina_minimize.  NOT gnina's or Vina's docking and not their numbers.
// k_vina_dock: one workgroup (4 waves) per (ligand, chain) and ONE launch for the whole search of every chain.  The set-up of
// k_vina_minimize runs once; then every turn of one outer loop (the start, the n_steps Monte-Carlo steps, the refinement) prepares a
// point and hands it to the ONE instance of the minimiser loop, with the turn's own iteration cap.  The current and the best pose
// live in LDS beside the minimiser's state; Philox words are drawn where they are used.  Evaluation, projection, recursion and chart
// are vina_min_core.h's; the set-up and the loop are restated from vina_min.hip, whose code object must not move
// (profiles/vina_dock.md).  k_vina_dock_modes: one workgroup per ligand ranks the chains' poses, takes their pairwise RMSDs and
// keeps the modes.  Nothing is shared between chains, no atomics on floats, no host synchronisation.
#include "vina_min_core.h"

namespace kpd {

constexpr int VD_CHAINS = 64;             // chains of one ligand
constexpr int VD_REPORT = 8;              // columns of report
constexpr int VD_CHAIN_REPORT = 10;       // columns of chain_report
enum : int { VD_BOX = 128, VD_START_OUT = 256, VD_FEW_MODES = 512 };                          // status bits 7 .. 9
constexpr int VD_LEFT_OUT = LP_NO_MOLECULE | LP_BAD_INPUT | VM_FRAGMENTS | VD_BOX;
// Philox blocks (the counter word q): a step's mutation, its Metropolis draw; of the random start, rotation and place of fragment f,
// and the angles of the rotors 4 j .. 4 j + 3
enum : unsigned { VD_Q_MUTATION = 0, VD_Q_METROPOLIS = 1, VD_Q_FRAGMENT = 2, VD_Q_ROTORS = VD_Q_FRAGMENT + 2 * VM_FRAGS };
constexpr double VD_PI = 3.141592653589793;

struct VinaDockP : VinaMinP {
    double temperature, amplitude;
    int step_iters;
};

// the minimiser's layout, then the current and the best pose, the fragments' radii of gyration and the ligand's centre
struct VinaDockLayout {
    VinaMinLayout M;
    size_t cur, best, rg, ctr, bytes;
};

__host__ __device__ inline VinaDockLayout vina_dock_layout(int nm, int mr, int stage) {
    VinaDockLayout L;
    L.M = vina_min_layout(nm, mr, stage);
    size_t o = L.M.bytes;
    L.cur = lds_take(o, (size_t)nm * 3 * 8, 16);
    L.best = lds_take(o, (size_t)nm * 3 * 8, 16);
    L.rg = lds_take(o, VM_FRAGS * 8, 16);
    L.ctr = lds_take(o, 4 * 8, 16);
    L.bytes = o;
    return L;
}

// the four uniforms u = (w + 0.5) 2^-32 of the Philox block (q, s, c, id)
__device__ __forceinline__ void vd_uniforms(unsigned q, unsigned s, unsigned c, unsigned id, unsigned k0, unsigned k1, double (&u)[4]) {
    unsigned w[4] = {q, s, c, id};
    philox4x32_10(w, k0, k1);
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = ((double)w[j] + 0.5) * 0x1p-32;
}

// a vector of the unit ball from three uniforms
__device__ __forceinline__ void vd_ball(double u1, double u2, double u3, double (&v)[3]) {
    const double z = 2.0 * u1 - 1.0, phi = (2.0 * VD_PI) * u2, rho = cbrt(u3);
    const double sq = sqrt(1.0 - z * z);
    double s, c;
    sincos(phi, &s, &c);
    v[0] = rho * (sq * c);
    v[1] = rho * (sq * s);
    v[2] = rho * z;
}

// centres and axes of x as vm_project leaves them, and the radius of gyration of every fragment about its centre (index order)
__device__ void vd_frame(const VinaMinCtx &C, const double *x, double *rg, int tid) {
    if (tid < 3 * C.F) {
        const int f = tid / 3, c = tid % 3;
        double s = 0.0;
        for (int i = 0; i < C.n; ++i)
            if (C.frg[i] == f) s += x[3 * i + c];
        C.cen[tid] = s / (double)C.fcnt[f];
    }
    __syncthreads();
    if (tid < C.T) {
        const int a = C.ra[tid], b = C.rb[tid];
        const double ax = x[3 * b] - x[3 * a], ay = x[3 * b + 1] - x[3 * a + 1], az = x[3 * b + 2] - x[3 * a + 2];
        const double len = sqrt((ax * ax + ay * ay) + az * az);
        const bool ok = len >= 1e-6;
        C.axu[3 * tid] = ok ? ax / len : 0.0;
        C.axu[3 * tid + 1] = ok ? ay / len : 0.0;
        C.axu[3 * tid + 2] = ok ? az / len : 0.0;
    } else if (tid >= 64 && tid < 64 + C.F) {
        const int f = tid - 64;
        const double cx = C.cen[3 * f], cy = C.cen[3 * f + 1], cz = C.cen[3 * f + 2];
        double s = 0.0;
        for (int i = 0; i < C.n; ++i) {
            if (C.frg[i] != f) continue;
            const double dx = x[3 * i] - cx, dy = x[3 * i + 1] - cy, dz = x[3 * i + 2] - cz;
            s += (dx * dx + dy * dy) + dz * dz;
        }
        rg[f] = sqrt(s / (double)C.fcnt[f]);
    }
    __syncthreads();
}

// is the mean of the atoms of x (index order) outside [lo, hi] in any coordinate?  Block-uniform.
__device__ bool vd_outside(const double *x, int n, const double (&lo)[3], const double (&hi)[3], double *ctr, int tid) {
    if (tid < 3) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += x[3 * i + tid];
        ctr[tid] = s / (double)n;
    }
    __syncthreads();
    bool out = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) out = out || ctr[k] < lo[k] || ctr[k] > hi[k];
    __syncthreads();
    return out;
}

// Waves per SIMD: profiles/vina_dock.md has the code-object figures of this kernel at two and at three, and the measurement.
#ifndef VD_WAVES
#define VD_WAVES 3
#endif
__global__ void __launch_bounds__(VN_T) __attribute__((amdgpu_waves_per_eu(VD_WAVES, VD_WAVES)))
k_vina_dock(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, int nm, const int *__restrict__ elem, int F,
            const int *__restrict__ zs, const float *__restrict__ lig_radius, const int *__restrict__ frag,
            const int *__restrict__ bond_ij, const int *__restrict__ bond_order, const int *__restrict__ bond_ptr, int cap_bonds,
            const int *__restrict__ mol_status, const int *__restrict__ lig_type_in, const float *__restrict__ pocket_x,
            const float *__restrict__ pocket_radius, const int *__restrict__ pocket_type, const int *__restrict__ pocket_ptr,
            int n_pocket, int n_pockets, int stage_cap, const int *__restrict__ pocket_of, int max_rotors,
            const float *__restrict__ box_lo, const float *__restrict__ box_hi, const int *__restrict__ lig_id, unsigned key0,
            unsigned key1, int n_chains, int n_steps, VinaDockP P, float *__restrict__ chain_pos, double *__restrict__ chain_report,
            int *__restrict__ status) {
    extern __shared__ double lds_d[];
    char *lds = reinterpret_cast<char *>(lds_d);
    const VinaDockLayout LD = vina_dock_layout(nm, max_rotors, stage_cap);
    const VinaMinLayout &L = LD.M;
    const int b = blockIdx.x, chain = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, W = L.W, DS = L.DS;
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
    double *cur = reinterpret_cast<double *>(lds + LD.cur), *best = reinterpret_cast<double *>(lds + LD.best);
    double *rg = reinterpret_cast<double *>(lds + LD.rg), *ctr = reinterpret_cast<double *>(lds + LD.ctr);
    double *crep = chain_report + ((size_t)b * n_chains + chain) * VD_CHAIN_REPORT;

    // ---- the box (bit 7), then k_vina_minimize's set-up: is there a molecule (bit 0), and its pocket (bit 1)?  Every `st` below is
    // block-uniform.
    double lo[3], hi[3];
    int box_bad = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float l = box_lo[(size_t)b * 3 + k], h = box_hi[(size_t)b * 3 + k];
        if (!finite_f(l) || !finite_f(h) || l > h) box_bad = VD_BOX;
        lo[k] = (double)l;
        hi[k] = (double)h;
    }
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
        for (int a = tid; a < n; a += VN_T) {
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
    st |= box_bad;
    if (st) {                                        // left out: chain_pos keeps the input rows the host copied
        if (tid < VD_CHAIN_REPORT) crep[tid] = 0.0;
        if (tid == 0 && chain == 0) status[b] = st;
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
    // Label propagation, as in k_vina_minimize: a label only ever decreases and always names an atom of the same piece, so a stale
    // read merely delays the descent; the loop ends on a sweep in which nobody wrote.
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

    // ---- the search
    const int N3 = 3 * n;
    const unsigned lid = lig_id ? (unsigned)lig_id[b] : (unsigned)b;
    if (vd_outside(x, n, lo, hi, ctr, tid)) st |= VD_START_OUT;
    int found = 0, best_step = -1, n_acc = 0, n_box = 0, evals = 0;
    double E_cur = 0.0, E_best = 0.0, E = 0.0, inter = 0.0, intra = 0.0, gnorm = 0.0;
    for (int turn = 0; turn <= n_steps + 1; ++turn) {
        const bool refine = turn == n_steps + 1;
        const int K = refine ? P.max_iters : P.step_iters;
        // -- the turn's starting point, in x
        if (turn == 0) {
            if (chain > 0) {                         // a random start: every rotor turned, every fragment turned and placed in the box
                vd_frame(C, x, rg, tid);
                for (int d = tid; d < D; d += VN_T) {
                    double u[4], val;
                    if (d < 6 * n_frag) {
                        const int f = d / 6, j = d % 6;
                        if (j >= 3) {
                            double v[3];
                            vd_uniforms(VD_Q_FRAGMENT + 2 * f, 0u, (unsigned)chain, lid, key0, key1, u);
                            vd_ball(u[0], u[1], u[2], v);
                            val = VD_PI * (j == 3 ? v[0] : j == 4 ? v[1] : v[2]);
                        } else {
                            vd_uniforms(VD_Q_FRAGMENT + 2 * f + 1, 0u, (unsigned)chain, lid, key0, key1, u);
                            const double uj = j == 0 ? u[0] : j == 1 ? u[1] : u[2];
                            const double l = j == 0 ? lo[0] : j == 1 ? lo[1] : lo[2], h = j == 0 ? hi[0] : j == 1 ? hi[1] : hi[2];
                            val = (l + uj * (h - l)) - C.cen[3 * f + j];
                        }
                    } else {
                        const int k = d - 6 * n_frag;
                        vd_uniforms(VD_Q_ROTORS + (unsigned)(k >> 2), 0u, (unsigned)chain, lid, key0, key1, u);
                        const int j = k & 3;
                        const double uj = j == 0 ? u[0] : j == 1 ? u[1] : j == 2 ? u[2] : u[3];
                        val = VD_PI * (2.0 * uj - 1.0);
                    }
                    p[d] = val;
                }
                __syncthreads();
                vm_move(C, x, p, 1.0, xt, tid);
                double *sw = x;
                x = xt;
                xt = sw;
            }
        } else if (!refine) {                        // a mutation of the current pose: one slot group of a delta that is zero elsewhere
            vd_frame(C, cur, rg, tid);
            double u[4], v[3];
            vd_uniforms(VD_Q_MUTATION, (unsigned)turn, (unsigned)chain, lid, key0, key1, u);
            vd_ball(u[1], u[2], u[3], v);
            const int n_ent = 2 * n_frag + T;
            const int e = min((int)floor(u[0] * (double)n_ent), n_ent - 1);
            for (int d = tid; d < D; d += VN_T) {
                double val = 0.0;
                const int f = d / 6, j = d % 6;
                const double vj = (j % 3) == 0 ? v[0] : (j % 3) == 1 ? v[1] : v[2];
                if (e < n_frag) {
                    if (d < 6 * n_frag && f == e && j < 3) val = P.amplitude * vj;
                } else if (e < 2 * n_frag) {
                    if (d < 6 * n_frag && f == e - n_frag && j >= 3 && rg[f] >= 1e-6) val = (P.amplitude / rg[f]) * vj;
                } else if (d == 6 * n_frag + (e - 2 * n_frag)) {
                    val = VD_PI * (2.0 * u[1] - 1.0);
                }
                p[d] = val;
            }
            __syncthreads();
            vm_move(C, cur, p, 1.0, x, tid);
            if (vd_outside(x, n, lo, hi, ctr, tid)) {    // box-rejected before minimising
                ++n_box;
                continue;
            }
        } else {
            if (!found) break;
            for (int k = tid; k < N3; k += VN_T) x[k] = best[k];
            __syncthreads();
        }
        // -- minimise(x, K): the iteration loop of k_vina_minimize with fresh memory
        vm_eval(C, x, g, tid);
        ++evals;
        E = scal[VS_E];
        inter = scal[VS_INTER];
        intra = scal[VS_INTRA];
        vm_project(C, x, g, gd, tid);
        gnorm = scal[VS_GNORM];
        int m = 0, head = 0;
        double gamma = 1.0;
        for (int it = 0; it < K; ++it) {
            if (gnorm <= P.gtol) break;
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
                if (m) {                             // try again along -g
                    m = 0;
                    continue;
                }
                break;                               // the line search is exhausted: this minimisation ends here
            }
            E = scal[VS_E];
            inter = scal[VS_INTER];
            intra = scal[VS_INTRA];
            vm_project(C, xt, g, gdt, tid);          // the new point's own chart
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
            if (sy > 1e-10 * yy && yy > 1e-20 * gg) {
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
            __syncthreads();                         // rho is read, and scal written again, only behind this
        }
        // -- what the turn does with the minimised point
        const bool fin = fabs(E) < __builtin_inf();
        if (refine) {
            // the closing step: the fp32 rounding of the refined point if its E does not exceed the best's, else that of the best itself
            for (int pass = 0; pass < 2; ++pass) {
                const double *src = pass ? best : x;
                for (int k = tid; k < N3; k += VN_T) xt[k] = (double)(float)src[k];
                __syncthreads();
                vm_eval(C, xt, g, tid);
                ++evals;
                if (pass) break;
                const bool lower = scal[VS_E] <= E_best;
                if (lower && !(chain > 0 && vd_outside(xt, n, lo, hi, ctr, tid))) break;     // chain 0 is the minimiser: no box
            }
            E = scal[VS_E];
            inter = scal[VS_INTER];
            intra = scal[VS_INTRA];
            vm_project(C, xt, g, gdt, tid);
            gnorm = scal[VS_GNORM];
        } else if (turn == 0) {
            if (!fin) break;                         // the chain ends with nothing found
            if (chain > 0 && vd_outside(x, n, lo, hi, ctr, tid)) {     // so does a random start that left the box
                ++n_box;
                break;
            }
            for (int k = tid; k < N3; k += VN_T) cur[k] = best[k] = x[k];
            E_cur = E_best = E;
            found = 1;
            best_step = 0;
            __syncthreads();
        } else if (vd_outside(x, n, lo, hi, ctr, tid)) {
            ++n_box;                                 // box-rejected after minimising
        } else {
            if (fin && E < E_best) {                 // the chain's best, accepted or not; a tie stays with the earlier step
                for (int k = tid; k < N3; k += VN_T) best[k] = x[k];
                E_best = E;
                best_step = turn;
            }
            double u[4];
            vd_uniforms(VD_Q_METROPOLIS, (unsigned)turn, (unsigned)chain, lid, key0, key1, u);
            if (fin && (E < E_cur || u[0] < exp((E_cur - E) / P.temperature))) {
                for (int k = tid; k < N3; k += VN_T) cur[k] = x[k];
                E_cur = E;
                ++n_acc;
            }
            __syncthreads();
        }
    }
    if (found) {                                     // xt holds the fp32-valued rows of the closing step
        float *rows = chain_pos + ((size_t)chain * n_atoms + a0) * 3;
        for (int k = tid; k < N3; k += VN_T) rows[k] = (float)xt[k];
    }
    if (tid == 0) {
        crep[0] = found ? E : 0.0;
        crep[1] = found ? inter : 0.0;
        crep[2] = found ? intra : 0.0;
        crep[3] = (double)best_step;
        crep[4] = (double)n_acc;
        crep[5] = (double)n_box;
        crep[6] = (double)evals;
        crep[7] = (double)found;
        crep[8] = found ? gnorm : 0.0;
        crep[9] = found ? inter * inv_norm : 0.0;
        if (chain == 0) status[b] = st;
    }
}

// Ranks the chains of one ligand that found a pose by (E, chain), keeps a pose iff it lies min_rmsd or more from every kept one, and
// writes the modes.  RMSDs between poses: over all atoms of the fp32 rows, in fp64, summed in index order by one thread per pair.
__global__ void __launch_bounds__(VN_T)
k_vina_dock_modes(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, const float *__restrict__ chain_pos,
                  const double *__restrict__ chain_report, int n_chains, int n_modes, double min_rmsd, float *__restrict__ pos_out,
                  int *__restrict__ n_found, double *__restrict__ report, int *__restrict__ status) {
    __shared__ double dist[VD_CHAINS * VD_CHAINS];
    __shared__ double red[4];
    __shared__ int kept[VD_CHAINS], s_kept;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int st = status[b];
    double *rep = report + (size_t)b * n_modes * VD_REPORT;
    const double *crep = chain_report + (size_t)b * n_chains * VD_CHAIN_REPORT;
    for (int k = tid; k < n_modes * VD_REPORT; k += VN_T) rep[k] = 0.0;
    if (st & VD_LEFT_OUT) {
        if (tid == 0) n_found[b] = 0;
        return;
    }
    int a0, a1;
    mol_segment(lig_ptr, b, n_atoms, a0, a1);        // well-formed: the ligand was not left out
    const int n = a1 - a0, N3 = 3 * n;
    for (int pr = tid; pr < n_chains * n_chains; pr += VN_T) {
        const int i = pr / n_chains, j = pr % n_chains;
        if (i >= j || crep[i * VD_CHAIN_REPORT + 7] == 0.0 || crep[j * VD_CHAIN_REPORT + 7] == 0.0) continue;
        const float *xi = chain_pos + ((size_t)i * n_atoms + a0) * 3, *xj = chain_pos + ((size_t)j * n_atoms + a0) * 3;
        double s = 0.0;
        for (int a = 0; a < n; ++a) {
            const double dx = (double)xi[3 * a] - (double)xj[3 * a], dy = (double)xi[3 * a + 1] - (double)xj[3 * a + 1],
                         dz = (double)xi[3 * a + 2] - (double)xj[3 * a + 2];
            s += (dx * dx + dy * dy) + dz * dz;
        }
        dist[i * VD_CHAINS + j] = dist[j * VD_CHAINS + i] = sqrt(s / (double)n);
    }
    __syncthreads();
    if (tid == 0) {
        int order[VD_CHAINS], cnt = 0;
        for (int c = 0; c < n_chains; ++c) {         // insertion by (E, chain): a later chain goes behind an equal E
            if (crep[c * VD_CHAIN_REPORT + 7] == 0.0) continue;
            const double Ec = crep[c * VD_CHAIN_REPORT];
            int at = cnt;
            while (at > 0 && Ec < crep[order[at - 1] * VD_CHAIN_REPORT]) {
                order[at] = order[at - 1];
                --at;
            }
            order[at] = c;
            ++cnt;
        }
        int nk = 0;
        for (int r = 0; r < cnt && nk < n_modes; ++r) {
            const int c = order[r];
            bool ok = true;
            for (int k = 0; k < nk; ++k) ok = ok && dist[c * VD_CHAINS + kept[k]] >= min_rmsd;
            if (ok) kept[nk++] = c;
        }
        s_kept = nk;
        n_found[b] = nk;
        status[b] = st | (nk < n_modes ? VD_FEW_MODES : 0);
    }
    __syncthreads();
    const int nk = s_kept;
    for (int m = 0; m < nk; ++m) {
        const int c = kept[m];
        const float *src = chain_pos + ((size_t)c * n_atoms + a0) * 3;
        float *dst = pos_out + ((size_t)m * n_atoms + a0) * 3;
        double sq = 0.0;                             // the rmsd to the input pose, reduced as kpd_vina_minimize reduces its own
        for (int k = tid; k < N3; k += VN_T) {
            const float v = src[k];
            dst[k] = v;
            const double d = (double)v - (double)pos[(size_t)a0 * 3 + k];
            sq += d * d;
        }
        sq = wave_sum(sq);
        if (lane == 0) red[wv] = sq;
        __syncthreads();
        if (tid == 0) {
            const double *cr = crep + c * VD_CHAIN_REPORT;
            double *r = rep + m * VD_REPORT;
            r[0] = cr[9];
            r[1] = cr[0];
            r[2] = cr[1];
            r[3] = cr[2];
            r[4] = sqrt((((red[0] + red[1]) + red[2]) + red[3]) / (double)n);
            r[5] = m ? dist[c * VD_CHAINS + kept[0]] : 0.0;
            r[6] = (double)c;
            r[7] = cr[8];
        }
        __syncthreads();
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_vina_dock(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms,
                                    const int32_t *elem, int32_t F, const int32_t *z, const float *lig_radius, const int32_t *frag,
                                    const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds,
                                    const int32_t *mol_status, const int32_t *lig_type_in, const float *pocket_x,
                                    const float *pocket_radius, const int32_t *pocket_type, const int32_t *pocket_ptr,
                                    int32_t n_pocket, int32_t P, int32_t max_pocket, const int32_t *pocket_of, int32_t max_rotors,
                                    const float *box_lo, const float *box_hi, const int32_t *lig_id, uint64_t seed, int32_t n_chains,
                                    int32_t n_steps, int32_t n_modes, const kpd_vina_dock_params *params, float *pos_out,
                                    int32_t *n_found, double *report, float *chain_pos, double *chain_report, int32_t *status,
                                    void *stream) {
    KPD_TRY(ligand_pocket_args(n_atoms, B, max_atoms, F, cap_bonds, n_pocket, P, max_pocket, lig_ptr && z && lig_radius && bond_ptr,
                               pos && elem && frag && pos_out && chain_pos,
                               mol_status && pocket_of && report && status && box_lo && box_hi && n_found && chain_report,
                               bond_ij && bond_order, pocket_ptr, pocket_x && pocket_radius && pocket_type));
    KPD_REQUIRE(max_rotors >= 0 && max_rotors <= VM_ROTORS, KPD_ERR_INVALID, "max_rotors=%d (0 .. %d)", max_rotors, VM_ROTORS);
    KPD_REQUIRE(n_chains >= 1 && n_chains <= VD_CHAINS && n_modes >= 1 && n_modes <= n_chains && n_steps >= 0, KPD_ERR_INVALID,
                "n_chains=%d (1 .. %d) n_modes=%d (1 .. n_chains) n_steps=%d (>= 0)", n_chains, VD_CHAINS, n_modes, n_steps);
    KPD_REQUIRE(!n_atoms || (pos_out != pos && chain_pos != pos), KPD_ERR_INVALID, "pos_out and chain_pos must not be pos");
    kpd_vina_dock_params d;
    kpd_vina_dock_defaults(&d);
    if (params) d = *params;
    VinaDockP vp;
    KPD_TRY(vina_fill_params({d.w_gauss1, d.w_gauss2, d.w_repulsion, d.w_hydrophobic, d.w_hbond, d.w_rot, d.r_c}, vp));
    KPD_REQUIRE(d.w_intra >= 0.0 && d.w_intra < 1e12 && d.gtol >= 0.0 && d.max_step > 0.0 && d.max_iters >= 0 && d.step_iters >= 0,
                KPD_ERR_INVALID, "w_intra=%g gtol=%g (>= 0) max_step=%g (> 0) max_iters=%d step_iters=%d", d.w_intra, d.gtol, d.max_step,
                d.max_iters, d.step_iters);
    KPD_REQUIRE(d.temperature > 0.0 && d.temperature < 1e12 && d.amplitude > 0.0 && d.amplitude < 1e12 && d.min_rmsd > 0.0 &&
                    d.min_rmsd < 1e12,
                KPD_ERR_INVALID, "temperature=%g amplitude=%g min_rmsd=%g (> 0)", d.temperature, d.amplitude, d.min_rmsd);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_atoms) {                                   // every mode and every chain starts as the input rows
        for (int m = 0; m < n_modes; ++m)
            KPD_HIP(hipMemcpyAsync(pos_out + (size_t)m * n_atoms * 3, pos, (size_t)n_atoms * 12, hipMemcpyDeviceToDevice, st));
        for (int c = 0; c < n_chains; ++c)
            KPD_HIP(hipMemcpyAsync(chain_pos + (size_t)c * n_atoms * 3, pos, (size_t)n_atoms * 12, hipMemcpyDeviceToDevice, st));
    }
    if (!B) return KPD_OK;
    vp.w_intra = d.w_intra;
    vp.gtol = d.gtol;
    vp.max_step = d.max_step;
    vp.max_iters = d.max_iters;
    vp.temperature = d.temperature;
    vp.amplitude = d.amplitude;
    vp.step_iters = d.step_iters;
    // as much of the largest pocket as fits beside the state of a max_atoms ligand
    const int stage = stage_rows(vina_dock_layout(max_atoms, max_rotors, 0).bytes, VM_LDS, VN_POCKET_ROW, max_pocket);
    KPD_REQUIRE(stage >= 0, KPD_ERR_INVALID, "no LDS for %d atoms", max_atoms);
    const VinaDockLayout L = vina_dock_layout(max_atoms, max_rotors, stage);
    KPD_REQUIRE(L.bytes <= (size_t)VM_LDS, KPD_ERR_INVALID, "LDS layout of %zu bytes", L.bytes);
    KPD_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(k_vina_dock), (int)L.bytes));
    hipLaunchKernelGGL(k_vina_dock, dim3(B, n_chains), dim3(VN_T), L.bytes, st, pos, lig_ptr, n_atoms, max_atoms, elem, F, z, lig_radius,
                       frag, bond_ij, bond_order, bond_ptr, cap_bonds, mol_status, lig_type_in, pocket_x, pocket_radius, pocket_type,
                       pocket_ptr, n_pocket, P, stage, pocket_of, max_rotors, box_lo, box_hi, lig_id, (unsigned)seed,
                       (unsigned)(seed >> 32), n_chains, n_steps, vp, chain_pos, chain_report, status);
    KPD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vina_dock_modes, dim3(B), dim3(VN_T), 0, st, pos, lig_ptr, n_atoms, chain_pos, chain_report, n_chains, n_modes,
                       d.min_rmsd, pos_out, n_found, report, status);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" void kpd_vina_dock_defaults(kpd_vina_dock_params *p) {
    if (!p) return;
    kpd_vina_min_params v;
    kpd_vina_min_defaults(&v);
    p->w_gauss1 = v.w_gauss1;
    p->w_gauss2 = v.w_gauss2;
    p->w_repulsion = v.w_repulsion;
    p->w_hydrophobic = v.w_hydrophobic;
    p->w_hbond = v.w_hbond;
    p->w_rot = v.w_rot;
    p->r_c = v.r_c;
    p->w_intra = v.w_intra;
    p->gtol = v.gtol;
    p->max_step = v.max_step;
    p->temperature = 1.2;
    p->amplitude = 2.0;
    p->min_rmsd = 1.0;
    p->max_iters = v.max_iters;
    p->step_iters = 20;
}
