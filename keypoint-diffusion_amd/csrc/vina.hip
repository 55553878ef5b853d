// Scores of sampled ligands in their rigid pockets on the device: the AutoDock Vina FUNCTIONAL FORM (five pair terms over ligand x
// pocket heavy atoms, divided by 1 + w_rot N_rot), where upstream hands pocket_minimized_ligands.sdf to gnina
// (analysis/docking: gen_docking_cmds.py).  Vina's own typing reads hydrogens and AutoDock atom types from PDBQT; ligands and
// pockets here carry heavy atoms and element classes, so include/kpd.h DEFINES the typing (three flags per atom from the element,
// the heavy degree and the neighbours' elements and length-class bond orders) and the rotor count.  NOT gnina's numbers: the
// scores rank samples scored here against each other.  No intramolecular term; minimisation and search under this function are vina_min.hip and vina_dock.hip.
// k_vina_pocket_types: one thread per pocket atom, the atoms of its pocket tiled through LDS 256 at a time (quadratic per pocket,
// which is right for pockets of hundreds of atoms); done once per pocket set.
// k_vina_score: one workgroup (4 waves) per ligand and ONE launch: the ligand's bond graph as a bit matrix in LDS, typing, the
// rotor count (one thread per bond walks the graph without it), then the pair sums: an atom's five terms and its gradient are
// summed by one wavefront whose lanes stride the pocket atoms (the first of them staged in LDS, the rest read from global memory
// with the same bits) and meet in a butterfly.  Nothing is shared between ligands, no atomics on floats, no host synchronisation:
// a ligand's result is bitwise independent of the batch, of what was staged, and of the repeat.
#include "common.h"
#include "molecule_core.h"
#include "vina_core.h"

namespace kpd {

constexpr int VN_LDS = 64 * 1024 - 512;   // dynamic LDS of a workgroup: what needs no opt-in, less the static bytes of the votes

// byte offsets of the dynamic LDS of a workgroup for ligands of at most nm atoms and `stage` staged pocket atoms
struct VinaLayout {
    size_t part, red, x0, rad, zat, typ, cnt, flg, adj, px, prad, ptyp, bytes;
    int W;
};

__host__ __device__ inline VinaLayout vina_layout(int nm, int stage) {
    VinaLayout L;
    L.W = (nm + 31) / 32;
    size_t o = 0;
    auto take = [&o](size_t bytes) { return lds_take(o, bytes, 16); };
    L.part = take((size_t)nm * 5 * 8);
    L.red = take(8 * 8);
    L.x0 = take((size_t)nm * 3 * 4);
    L.rad = take((size_t)nm * 4);
    L.zat = take((size_t)nm * 4);
    L.typ = take((size_t)nm * 4);
    L.cnt = take((size_t)nm * 4);
    L.flg = take((size_t)nm * 4);
    L.adj = take((size_t)nm * L.W * 4);
    L.px = take((size_t)stage * 3 * 4);
    L.prad = take((size_t)stage * 4);
    L.ptyp = take((size_t)stage * 4);
    L.bytes = o;
    return L;
}

// ---- pocket typing: block (q, t) types the atoms [256 t, 256 t + 256) of pocket q ------------------------------------------
__global__ void __launch_bounds__(VN_T)
k_vina_pocket_types(const float *__restrict__ pocket_x, const int *__restrict__ pocket_z, const int *__restrict__ pocket_ptr, int n_pocket,
                    int tiles, int *__restrict__ pocket_type, int *__restrict__ status) {
    __shared__ float sx[VN_T * 3];
    __shared__ unsigned srow[VN_T];      // element_row, radii zeroed for an atom that has no neighbours
    __shared__ int sz[VN_T];
    const int q = blockIdx.x / tiles, t = blockIdx.x % tiles, tid = threadIdx.x;
    const int q0 = pocket_ptr[q], q1 = pocket_ptr[q + 1];
    if (q0 < 0 || q1 < q0 || q1 > n_pocket) {        // malformed: no atom is touched
        if (t == 0 && tid == 0) status[q] = 1;
        return;
    }
    const int np = q1 - q0;
    if (t && t * VN_T >= np) return;
    const int i = t * VN_T + tid;
    float xi = 0.f, yi = 0.f, zi = 0.f;
    unsigned ri = 0;
    int Zi = 0;
    bool fin_i = false;
    if (i < np) {
        const float *r = pocket_x + (size_t)(q0 + i) * 3;
        xi = r[0];
        yi = r[1];
        zi = r[2];
        Zi = pocket_z[q0 + i];
        fin_i = finite_f(xi) && finite_f(yi) && finite_f(zi);
        ri = fin_i ? element_row(Zi) : 0u;
    }
    int deg = 0, bad = 0;
    unsigned nf = 0;
    for (int j0 = 0; j0 < np; j0 += VN_T) {
        __syncthreads();
        const int jl = j0 + tid;
        if (jl < np) {
            const float *r = pocket_x + (size_t)(q0 + jl) * 3;
            const float x = r[0], y = r[1], z = r[2];
            const int Z = pocket_z[q0 + jl];
            const bool fin = finite_f(x) && finite_f(y) && finite_f(z);
            if (!fin) bad = 1;
            sx[3 * tid] = x;
            sx[3 * tid + 1] = y;
            sx[3 * tid + 2] = z;
            srow[tid] = fin ? element_row(Z) : 0u;
            sz[tid] = Z;
        }
        __syncthreads();
        if (!(ri & 0xffu)) continue;                 // block-uniform barriers stay above; this atom has no neighbours
        const int cnt = min(VN_T, np - j0);
        for (int j = 0; j < cnt; ++j) {
            if (j0 + j == i) continue;
            const unsigned rj = srow[j];
            const double d2 = sum_sq((double)xi - (double)sx[3 * j], (double)yi - (double)sx[3 * j + 1], (double)zi - (double)sx[3 * j + 2]);
            if (!(d2 > 0.16 && within(d2, ri & 0xffu, rj & 0xffu, 45))) continue;
            const int Zj = sz[j];
            if (Zj == 1) continue;                   // hydrogens are no neighbours for the typing
            ++deg;
            if (Zj != 6) nf |= VN_HETERO;
            const int order = within(d2, (ri >> 16) & 0xffu, (rj >> 16) & 0xffu, 3) ? 3 : within(d2, (ri >> 8) & 0xffu, (rj >> 8) & 0xffu, 5) ? 2 : 1;
            nf |= 1u << order;
        }
    }
    if (i < np) pocket_type[q0 + i] = (!fin_i || Zi == 1) ? -1 : vina_flags(Zi, deg, nf);
    const int any_bad = __syncthreads_or(bad);
    if (t == 0 && tid == 0) status[q] = any_bad ? 2 : 0;      // the vote is a predicate, not the OR of the values
}

__global__ void __launch_bounds__(VN_T)
k_vina_score(const float *__restrict__ pos, const int *__restrict__ lig_ptr, int n_atoms, int nm, const int *__restrict__ elem, int F,
             const int *__restrict__ zs, const float *__restrict__ lig_radius, const int *__restrict__ bond_ij,
             const int *__restrict__ bond_order, const int *__restrict__ bond_ptr, int cap_bonds, const int *__restrict__ mol_status,
             const int *__restrict__ lig_type_in, const float *__restrict__ pocket_x, const float *__restrict__ pocket_radius,
             const int *__restrict__ pocket_type, const int *__restrict__ pocket_ptr, int n_pocket, int n_pockets, int stage_cap,
             const int *__restrict__ pocket_of, VinaP P, double *__restrict__ report, double *__restrict__ grad,
             double *__restrict__ atom_score, int *__restrict__ lig_type, int *__restrict__ status) {
    extern __shared__ double lds_d[];
    char *lds = reinterpret_cast<char *>(lds_d);
    const VinaLayout L = vina_layout(nm, stage_cap);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, W = L.W;
    double *part = reinterpret_cast<double *>(lds + L.part), *red = reinterpret_cast<double *>(lds + L.red);
    float *x0 = reinterpret_cast<float *>(lds + L.x0), *rad = reinterpret_cast<float *>(lds + L.rad);
    int *zat = reinterpret_cast<int *>(lds + L.zat), *typ = reinterpret_cast<int *>(lds + L.typ);
    unsigned *cnt = reinterpret_cast<unsigned *>(lds + L.cnt), *flg = reinterpret_cast<unsigned *>(lds + L.flg);
    unsigned *adj = reinterpret_cast<unsigned *>(lds + L.adj);
    float *px = reinterpret_cast<float *>(lds + L.px), *prad = reinterpret_cast<float *>(lds + L.prad);
    int *ptyp = reinterpret_cast<int *>(lds + L.ptyp);

    // ---- is there a molecule (bit 0), and its pocket (bit 1)?  Every `st` below is block-uniform.
    LigandInPocket lp;
    int st = ligand_in_pocket(lig_ptr, b, n_atoms, nm, bond_ptr, cap_bonds, mol_status, pocket_of, pocket_ptr, n_pocket, n_pockets, lp);
    const int a0 = lp.a0, a1 = lp.a1, n = lp.n, p0 = lp.p0, p1 = lp.p1, q0 = lp.q0, np = lp.np;
    const int stage = min(np, stage_cap);
    int atom_out = 0;
    if (!st) {
        int bad = 0;
        for (int a = tid; a < n; a += VN_T) {        // k_vina_minimize stages its atoms the same way
            cnt[a] = 0;
            flg[a] = 0;
            zat[a] = 0;
            rad[a] = 0.f;
            for (int w = 0; w < W; ++w) adj[a * W + w] = 0;
            const size_t ga = (size_t)(a0 + a);
            const int e = elem[ga];
            if (e < 0 || e >= F) {
                bad |= LP_NO_MOLECULE;
                continue;
            }
            const float rv = lig_radius[e];
            if (!finite_f(rv)) bad |= LP_BAD_INPUT;
            rad[a] = rv;
            zat[a] = zs[e];
            for (int k = 0; k < 3; ++k) {
                const float v = pos[ga * 3 + k];
                if (!finite_f(v)) bad |= LP_BAD_INPUT;
                x0[3 * a + k] = v;
            }
        }
        vina_stage_pocket(pocket_x, pocket_radius, pocket_type, q0, np, stage, tid, px, prad, ptyp, bad, atom_out);
        st = lp_votes(bad);
    }
    if (!st) {                                       // the bond graph: a bond may be listed as (j, i), there are no fragment labels
        const int bad = vina_bond_graph<false, false>(bond_ij, bond_order, p0, p1, a0, n, W, tid, zat, nullptr, adj, cnt, flg);
        st = __syncthreads_or(bad) ? LP_NO_MOLECULE : 0;
    }
    if (st) {                                        // left out: zero rows, types -1
        if (tid < 8) report[(size_t)b * 8 + tid] = 0.0;
        if (tid == 0) status[b] = st;
        if (lp.seg)
            for (int a = a0 + tid; a < a1; a += VN_T) {
                if (grad) grad[(size_t)a * 3] = grad[(size_t)a * 3 + 1] = grad[(size_t)a * 3 + 2] = 0.0;
                if (atom_score) atom_score[a] = 0.0;
                if (lig_type) lig_type[a] = -1;
            }
        return;
    }
    // ---- types
    vina_type_atoms(n, a0, tid, zat, cnt, flg, rad, lig_type_in, typ, lig_type, atom_out);
    // ---- rotors: single bonds between atoms of heavy degree >= 2 that are in no ring
    int rot = 0;
    for (int k = p0 + tid; k < p1; k += VN_T) {
        if (bond_order[k] != 1) continue;
        const int i = bond_ij[(size_t)k * 2] - a0, j = bond_ij[(size_t)k * 2 + 1] - a0;
        if (((cnt[i] >> 4) & 15u) < 2u || ((cnt[j] >> 4) & 15u) < 2u) continue;
        unsigned vis[MOL_W];
        if (!vina_walk<true>(adj, W, i, j, vis)) ++rot;      // in no ring: j is not reached from i without the bond
    }
    rot = wave_sum(rot);
    int *redi = reinterpret_cast<int *>(red);
    if (lane == 0) redi[wv] = rot;
    if (__syncthreads_or(atom_out)) st |= VN_ATOM_OUT;   // also orders typ and redi before their readers
    const int n_rot = (redi[0] + redi[1]) + (redi[2] + redi[3]);
    const double inv_norm = 1.0 / (1.0 + P.w_rot * (double)n_rot);

    // ---- pair sums: wave w takes the atoms w, w + 4, ...
    const float *gpx = pocket_x + (size_t)q0 * 3, *gpr = pocket_radius + q0;
    const int *gpt = pocket_type + q0;
    for (int i = wv; i < n; i += 4) {
        const int ti = typ[i];
        double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, gx = 0.0, gy = 0.0, gz = 0.0;
        if (ti >= 0) {                               // wave-uniform
            const double xi = (double)x0[3 * i], yi = (double)x0[3 * i + 1], zi = (double)x0[3 * i + 2], Ri = (double)rad[i];
            vina_pocket_sums(xi, yi, zi, Ri, ti, lane, np, stage, px, prad, ptyp, gpx, gpr, gpt, P, t, gx, gy, gz);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] = wave_sum(t[k]);
        gx = wave_sum(gx);
        gy = wave_sum(gy);
        gz = wave_sum(gz);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) part[5 * i + k] = t[k];
            if (grad) {
                double *g = grad + (size_t)(a0 + i) * 3;
                g[0] = gx * inv_norm;
                g[1] = gy * inv_norm;
                g[2] = gz * inv_norm;
            }
            if (atom_score) atom_score[a0 + i] = (((P.w[0] * t[0] + P.w[1] * t[1]) + P.w[2] * t[2]) + P.w[3] * t[3]) + P.w[4] * t[4];
        }
    }
    __syncthreads();
    if (wv == 0) {
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = lane; i < n; i += 64) {
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] += part[5 * i + k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = wave_sum(s[k]);
        if (lane == 0) {
            double *r = report + (size_t)b * 8;
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] *= P.w[k];
            const double inter = (((s[0] + s[1]) + s[2]) + s[3]) + s[4];
            r[0] = inter * inv_norm;
            r[1] = inter;
#pragma unroll
            for (int k = 0; k < 5; ++k) r[2 + k] = s[k];
            r[7] = (double)n_rot;
            status[b] = st;
        }
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_vina_pocket_types(const float *pocket_x, const int32_t *pocket_z, const int32_t *pocket_ptr, int32_t n_pocket,
                                            int32_t P, int32_t *pocket_type, int32_t *status, void *stream) {
    KPD_REQUIRE(n_pocket >= 0 && P >= 0, KPD_ERR_INVALID, "n_pocket=%d P=%d", n_pocket, P);
    KPD_REQUIRE(!P || (pocket_ptr && status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_pocket || (pocket_x && pocket_z && pocket_type), KPD_ERR_INVALID, "null pocket buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // atoms outside every well-formed segment read -1
    if (n_pocket) KPD_HIP(hipMemsetAsync(pocket_type, 0xff, (size_t)n_pocket * 4, st));
    if (!P) return KPD_OK;
    const int tiles = std::max(1, cdiv(n_pocket, VN_T));
    KPD_REQUIRE((int64_t)P * tiles <= 0x7fffffffLL, KPD_ERR_INVALID, "P=%d pockets x %d tiles exceed the grid", P, tiles);
    hipLaunchKernelGGL(k_vina_pocket_types, dim3((unsigned)(P * tiles)), dim3(VN_T), 0, st, pocket_x, pocket_z, pocket_ptr, n_pocket, tiles,
                       pocket_type, status);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_vina_score(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms,
                                     const int32_t *elem, int32_t F, const int32_t *z, const float *lig_radius, const int32_t *bond_ij,
                                     const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status,
                                     const int32_t *lig_type_in, const float *pocket_x, const float *pocket_radius,
                                     const int32_t *pocket_type, const int32_t *pocket_ptr, int32_t n_pocket, int32_t P,
                                     int32_t max_pocket, const int32_t *pocket_of, const kpd_vina_params *params, double *report,
                                     double *grad, double *atom_score, int32_t *lig_type, int32_t *status, void *stream) {
    KPD_TRY(ligand_pocket_args(n_atoms, B, max_atoms, F, cap_bonds, n_pocket, P, max_pocket, lig_ptr && z && lig_radius && bond_ptr,
                               pos && elem, mol_status && pocket_of && report && status, bond_ij && bond_order, pocket_ptr,
                               pocket_x && pocket_radius && pocket_type));
    kpd_vina_params d;
    kpd_vina_defaults(&d);
    if (params) d = *params;
    VinaP vp;
    KPD_TRY(vina_fill_params(d, vp));
    if (!B) return KPD_OK;
    // as much of the largest pocket as fits beside a max_atoms ligand
    const int stage = stage_rows(vina_layout(max_atoms, 0).bytes, VN_LDS, VN_POCKET_ROW, max_pocket);
    KPD_REQUIRE(stage >= 0, KPD_ERR_INVALID, "no LDS for %d atoms", max_atoms);
    const VinaLayout L = vina_layout(max_atoms, stage);
    KPD_REQUIRE(L.bytes <= (size_t)VN_LDS, KPD_ERR_INVALID, "LDS layout of %zu bytes", L.bytes);
    hipLaunchKernelGGL(k_vina_score, dim3(B), dim3(VN_T), L.bytes, static_cast<hipStream_t>(stream), pos, lig_ptr, n_atoms, max_atoms, elem,
                       F, z, lig_radius, bond_ij, bond_order, bond_ptr, cap_bonds, mol_status, lig_type_in, pocket_x, pocket_radius,
                       pocket_type, pocket_ptr, n_pocket, P, stage, pocket_of, vp, report, grad, atom_score, lig_type, status);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" void kpd_vina_defaults(kpd_vina_params *p) {
    if (!p) return;
    p->w_gauss1 = -0.035579;
    p->w_gauss2 = -0.005156;
    p->w_repulsion = 0.840245;
    p->w_hydrophobic = -0.035069;
    p->w_hbond = -0.587439;
    p->w_rot = 0.05846;
    p->r_c = 8.0;
}
