// The GVP denoiser at n_hidden_scalars 257 .. 1024 (inference): LigRecDynamicsGVP.forward (models/dynamics_gvp.py:149-199,
// models/gvp.py:459-551; oracle/gvp.py) composed one GVP at a time from the trainer's GVP forward (gvp_train_core.h gvp_fwd: its
// vector-channel kernels and its scalar products on the library's fp32 MFMA GEMM, sgemm.hip) and five kernels of its own.
//
// S = n_hidden_scalars, V = vector_size (1 .. 16), Sw = S rounded up to a multiple of 4: scalar rows are Sw floats, the pad columns hold
// zeros (zero weight rows / columns, zero biases: SiLU(0) = 0), vectors are [rows, 3, V] (the trainer's layout).  Per conv:
//   1. per active edge type (ll, kl, then lk, kk when update_kp and not the last conv):
//        sgemm          P = s_src Wsrc^T: the s_src block of the head GVP's to_feats_out, once per SOURCE node
//        k_gw_edge_in   pre[e] = P[src[e]] + rbf(d_e) Wrbf^T, vin[e] = [x_diff / d_e | v_src[src[e]]]  (gvp.py:472-480, 545-547)
//        gvp_fwd        the head GVP on the rest (the |Vh| block, bias, SiLU, gate), then the n_message_gvps - 1 others (S -> S)
//        k_gw_agg       node-parallel sum over the dst-sorted CSR into agg_s / agg_v: edges in CSR order, edge types in the order
//                       ll, kl, lk, kk, 'mean' per edge type, the last type into a node type divides by the norm -- no atomics;
//   2. per updated node type: k_gw_norm (residual + GVPLayerNorm over the S true columns and V channels), the n_update_gvps chain,
//      k_gw_norm again.  The last conv runs ll + kl and the ligand update only (dynamics_gvp.py:67-72).
// Encoders: sgemm over [h | t] with the bias + SiLU epilogue, then k_gw_norm (LayerNorm only).  Noise head: the n_noise_gvps chain (the
// last to 64 scalars and one vector, identity vector activation), then k_gw_out (to_scalar_output, eps_x).
// Every scalar product is an A B^T product with M a multiple of 4 and a device live-row count (edge counts stay on the device; node
// counts are lig_ptr[B] / kp_ptr[B]), no split along K: each output element is one MFMA chain over K in slab order, whatever M or the
// row's position (sgemm.h), so a complex's bits do not depend on its batch.  The forward makes no host synchronisation.
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "gvp_host.h"
#include "gvp_kernels.h"
#include "gvp_train_core.h"
#include "gvp_wide.h"
#include "sgemm.h"

namespace kpd {

namespace {

const int kSrcNtW[4] = {0, 1, 0, 1};     // ll, kl, lk, kk  (0 = lig, 1 = kp)
const int kDstNtW[4] = {0, 0, 1, 1};
const char *kCanonW[4] = {"lig_ll_lig", "kp_kl_lig", "lig_lk_kp", "kp_kk_kp"};
const char *kNtNameW[2] = {"lig", "kp"};

typedef float gf4 __attribute__((ext_vector_type(4)));

inline int up4(int v) { return (v + 3) & ~3; }

// encoder input rows [h | t[graph] | 0 ..] (dynamics_gvp.py:161-169), ldx columns
__global__ void k_gw_cat_time(const float *__restrict__ h, int F, const float *__restrict__ t, const int *__restrict__ bidx, int n, int ldx,
                              float *__restrict__ X) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)n * ldx) return;
    const int r = (int)(i / ldx), c = (int)(i - (long long)r * ldx);
    X[i] = c < F ? h[(size_t)r * F + c] : (c == F ? t[bidx[r]] : 0.0f);
}

// reference [n, V, 3] -> [n, 3, V]
__global__ void k_gw_v_in(const float *__restrict__ in, int n, int V, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 3 * V) return;
    const int r = i / (3 * V), k = i - r * 3 * V, c = k / V, ch = k - c * V;
    out[i] = in[(size_t)r * 3 * V + ch * 3 + c];
}

__device__ __forceinline__ float gw_block_sum(float v, float *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// s = LayerNorm(s + ds) over the St true columns (pads 0); v = v' / (sqrt(mean_ch max(|v'_ch|^2, 1e-8) + 1e-5) + 1e-5), v' = v + dv
// (GVPLayerNorm, gvp.py:159-166).  ds / dv may be null; v null: the scalar LayerNorm alone (the encoders).  One workgroup per node.
constexpr int GW_PER = GVP_WIDE_MAX_S / 256;     // columns per thread
__global__ __launch_bounds__(256) void k_gw_norm(float *__restrict__ s, const float *__restrict__ ds, int St, int Sw,
                                                 const float *__restrict__ lnw, const float *__restrict__ lnb, float *__restrict__ v,
                                                 const float *__restrict__ dv, int V) {
    __shared__ float red[256];
    __shared__ float sv[3 * 16];
    __shared__ float s_inv;
    const int node = blockIdx.x, tid = threadIdx.x;
    float *sr = s + (size_t)node * Sw;
    const float *dr = ds ? ds + (size_t)node * Sw : nullptr;
    float x[GW_PER];
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < GW_PER; ++i) {
        const int c = tid + 256 * i;
        x[i] = c < St ? sr[c] + (dr ? dr[c] : 0.0f) : 0.0f;
        sum += x[i];
    }
    const float mean = gw_block_sum(sum, red) / (float)St;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < GW_PER; ++i) {
        const int c = tid + 256 * i;
        x[i] = c < St ? x[i] - mean : 0.0f;
        q += x[i] * x[i];
    }
    const float rstd = 1.0f / sqrtf(gw_block_sum(q, red) / (float)St + 1e-5f);
#pragma unroll
    for (int i = 0; i < GW_PER; ++i) {
        const int c = tid + 256 * i;
        if (c < Sw) sr[c] = c < St ? x[i] * rstd * lnw[c] + lnb[c] : 0.0f;
    }
    if (!v) return;
    float *vr = v + (size_t)node * 3 * V;
    const float *dvr = dv ? dv + (size_t)node * 3 * V : nullptr;
    if (tid < 3 * V) sv[tid] = vr[tid] + (dvr ? dvr[tid] : 0.0f);
    __syncthreads();
    if (tid == 0) {                    // channels in order: one fixed sum
        float m = 0.0f;
        for (int ch = 0; ch < V; ++ch) m += fmaxf(sv[ch] * sv[ch] + sv[V + ch] * sv[V + ch] + sv[2 * V + ch] * sv[2 * V + ch], 1e-8f);
        s_inv = sqrtf(m / (float)V + 1e-5f) + 1e-5f;
    }
    __syncthreads();
    if (tid < 3 * V) vr[tid] = sv[tid] / s_inv;
}

// head GVP inputs, one thread per (edge, 4 columns): pre[e] = P[src[e]] + sum_k rbf_k(d_e) WrbfT[k]; thread 0 of an edge also writes
// vin[e] = [unit edge vector | v_src[src[e]]] ([3][V + 1]).  x_diff = x_src - x_dst, d = sqrt(max(|x_diff|^2, 1e-8)) + 1e-8,
// rbf_k = exp(-((d - mu_k) / sigma)^2), mu_k = k dmax / 15, sigma = dmax / 16 (gvp.py:26-41, 474-480)
__global__ __launch_bounds__(256) void k_gw_edge_in(const int *__restrict__ e_live, int e_cap, const int *__restrict__ src,
                                                    const int *__restrict__ dst, const float *__restrict__ xs, const float *__restrict__ xd,
                                                    const float *__restrict__ vsrc, int V, const float *__restrict__ P, int Sw,
                                                    const float *__restrict__ WrbfT, float dmax, float *__restrict__ pre,
                                                    float *__restrict__ vin) {
    const int q4 = Sw >> 2;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int e = (int)(gid / q4), q = (int)(gid - (long long)e * q4);
    if (e >= min(*e_live, e_cap)) return;
    const int s = src[e], d = dst[e];
    float dx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) dx[k] = xs[(size_t)s * 3 + k] - xd[(size_t)d * 3 + k];
    const float dist = sqrtf(fmaxf(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2], 1e-8f)) + 1e-8f;
    const float sigma = dmax / 16.0f;
    float rb[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float z = (dist - dmax * (float)k / 15.0f) / sigma;
        rb[k] = expf(-z * z);
    }
    gf4 o = *reinterpret_cast<const gf4 *>(P + (size_t)s * Sw + 4 * q);
#pragma unroll
    for (int k = 0; k < 16; ++k) {             // Wrbf^T rows: the lanes of a wave read one contiguous piece
        const gf4 w = *reinterpret_cast<const gf4 *>(WrbfT + (size_t)k * Sw + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = fmaf(rb[k], w[i], o[i]);
    }
    *reinterpret_cast<gf4 *>(pre + (size_t)e * Sw + 4 * q) = o;
    if (q != 0) return;
    const int vi = V + 1;
    float *out = vin + (size_t)e * 3 * vi;
    const float *vs = vsrc + (size_t)s * 3 * V;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c * vi] = dx[c] / dist;
        for (int ch = 0; ch < V; ++ch) out[c * vi + 1 + ch] = vs[c * V + ch];
    }
}

// segmented sums over the dst-sorted CSR: two nodes per workgroup, 128 threads per node.  agg_s [n][Sw] / agg_v [n][3V] continue from
// what the previous edge type into this node type left (first: from zero).  mode 1 ('mean'): this type's sums / max(in-degree, 1);
// modes 0 / 2: the last type divides the total by norm / z[graph] (gvp.py:486-507)
__global__ __launch_bounds__(256) void k_gw_agg(const int *__restrict__ rowptr, int n, const float *__restrict__ ms, int Sw,
                                                const float *__restrict__ mv, int V, float *__restrict__ agg_s, float *__restrict__ agg_v,
                                                int first, int last, int mode, float norm, const float *__restrict__ z,
                                                const int *__restrict__ bidx) {
    const int t = threadIdx.x & 127, node = blockIdx.x * 2 + (threadIdx.x >> 7);
    if (node >= n) return;
    const int e0 = rowptr[node], e1 = rowptr[node + 1];
    const float deg = (float)max(e1 - e0, 1);
    const bool div = last && mode != 1;
    const float nv = div ? (mode == 2 ? z[bidx[node]] : norm) : 1.0f;
    for (int q = t; q < (Sw >> 2); q += 128) {
        gf4 acc = gf4(0.0f);
        for (int e = e0; e < e1; ++e) acc += *reinterpret_cast<const gf4 *>(ms + (size_t)e * Sw + 4 * q);
        if (mode == 1) acc = acc / deg;
        if (!first) acc = *reinterpret_cast<const gf4 *>(agg_s + (size_t)node * Sw + 4 * q) + acc;
        if (div) acc = acc / nv;
        *reinterpret_cast<gf4 *>(agg_s + (size_t)node * Sw + 4 * q) = acc;
    }
    const int vw = 3 * V;
    for (int k = t; k < vw; k += 128) {
        float acc = 0.0f;
        for (int e = e0; e < e1; ++e) acc += mv[(size_t)e * vw + k];
        if (mode == 1) acc = acc / deg;
        if (!first) acc = agg_v[(size_t)node * vw + k] + acc;
        if (div) acc = acc / nv;
        agg_v[(size_t)node * vw + k] = acc;
    }
}

// noise-head outputs (dynamics_gvp.py:38-44): eps_h[r] = W s[r] + b (s: the last GVP's 64 scalars), eps_x[r] = its single vector
__global__ void k_gw_out(const float *__restrict__ s, const float *__restrict__ vout, int n, const float *__restrict__ W,
                         const float *__restrict__ b, int F, float *__restrict__ eps_h, float *__restrict__ eps_x) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * (F + 3)) return;
    const int r = i / (F + 3), c = i - r * (F + 3);
    if (c < F) {
        float a = b[c];
        for (int k = 0; k < 64; ++k) a = fmaf(s[(size_t)r * 64 + k], W[(size_t)c * 64 + k], a);
        eps_h[(size_t)r * F + c] = a;
    } else {
        eps_x[(size_t)r * 3 + (c - F)] = vout[(size_t)r * 3 + (c - F)];
    }
}

}  // namespace

// the stream and the (unused: no 256 x 256 products here) scratch members gvp_fwd refers to
struct GvpWideCtx : TrainCtx {
    float *dgate = nullptr, *wsg_pack = nullptr;
};

// one GVP with zero-padded weights in gvp_fwd's form (GvpP: Ws [so][si + h], the |Vh| block after si columns)
struct WideGvp {
    GvpP p;
    int si_t = 0, so_t = 0;                  // true scalar widths (head: si_t = S, the s_src block, which lives in Wsrc)
    bool head = false;
    float *Wsrc = nullptr, *WrbfT = nullptr; // head: to_feats_out's s_src block [Sw][Sw] and rbf block, transposed [16][Sw]
};

struct GvpWide {
    kpd_gvp_config cfg;
    int St, Sw, V, fin4[2];
    Arena warena, ws;
    std::vector<std::vector<std::vector<WideGvp>>> msg, upd;     // [conv][et | nt][j]
    std::vector<std::vector<float *>> ln1w, ln1b, ln2w, ln2b;    // [conv][nt]
    std::vector<WideGvp> noise;
    float *enc_W[2], *enc_b[2], *enc_lw[2], *enc_lb[2];          // encoder Linear [Sw][fin4], LayerNorm [Sw]
    float *out_W, *out_b;
    std::set<std::string> expected, loaded;
    bool committed = false;
    int debug_convs = -1;
    GvpWideCtx T;
    // workspace (valid after reserve)
    int cap_B = 0, cap_lig = 0, cap_kp = 0, cap_kk = 0, cap_maxlig = 0, cap_maxkp = 0, rows = 0;
    float *s[2], *v[2], *agg_s[2], *agg_v[2], *z[2], *X, *P;
    float *es[2], *ev[2], *vin, *Vh, *Vu, *sh, *gate;
    int *bidx[2];
    int *meta4, *ll_deg, *ll_off, *kl_off, *kl_pg;
    kpd_lig_graph lg;

    int n_et(int conv) const { return (cfg.update_kp && conv != cfg.n_convs - 1) ? 4 : 2; }
};

namespace {

// carve one GVP's weights: vi / vo vector channels, si_w / so_w scalar columns of the engine layout (head: si_w = 0)
void carve_gvp(Carve &A, WideGvp &g, int vi, int vo, int si_t, int so_t, int si_w, int so_w, bool head, int Sw, std::set<std::string> &expected,
               const std::string &prefix) {
    GvpP &p = g.p;
    p.vi = vi; p.vo = vo; p.h = std::max(vi, vo); p.si = si_w; p.so = so_w;
    g.si_t = si_t; g.so_t = so_t; g.head = head;
    float *Wh, *Wu, *Ws, *bs, *Wg, *bg;
    A(Wh, (size_t)vi * p.h); A(Wu, (size_t)p.h * vo);
    A(Ws, (size_t)so_w * (si_w + p.h)); A(bs, so_w);
    A(Wg, (size_t)vo * so_w); A(bg, vo);
    if (head) { A(g.Wsrc, (size_t)Sw * Sw); A(g.WrbfT, (size_t)16 * Sw); }
    p.Wh.w = Wh; p.Wu.w = Wu; p.Ws.w = Ws; p.bs.w = bs; p.Wg.w = Wg; p.bg.w = bg;
    for (const char *s : {".Wh", ".Wu", ".to_feats_out.0.weight", ".to_feats_out.0.bias", ".scalar_to_vector_gates.weight",
                          ".scalar_to_vector_gates.bias"})
        expected.insert(prefix + s);
}

// rows x cols of a row-major source (row stride lds) into dst (row stride ldd); everything else of dst keeps its zeros
kpd_status place(const float *dst, size_t ldd, const float *src, size_t lds, size_t rows, size_t cols, hipStream_t st) {
    KPD_HIP(hipMemcpy2DAsync(const_cast<float *>(dst), ldd * 4, src, lds * 4, cols * 4, rows, hipMemcpyDeviceToDevice, st));
    return KPD_OK;
}

kpd_status load_gvp(WideGvp &g, const std::string &tail, const char *name, const float *w, const int64_t *shape, int ndim, int St,
                    hipStream_t st) {
    const GvpP &p = g.p;
    const int h = p.h;
    if (tail == "Wh") {
        KPD_TRY(want_shape(name, shape, ndim, {p.vi, h}));
        return place(p.Wh.w, h, w, h, p.vi, h, st);
    }
    if (tail == "Wu") {
        KPD_TRY(want_shape(name, shape, ndim, {h, p.vo}));
        return place(p.Wu.w, p.vo, w, p.vo, h, p.vo, st);
    }
    if (tail == "to_feats_out.0.weight") {
        if (g.head) {                 // [S, S + 16 + h]: s_src | rbf | |Vh|
            const int k = St + 16 + h;
            KPD_TRY(want_shape(name, shape, ndim, {g.so_t, k}));
            KPD_TRY(place(g.Wsrc, p.so, w, k, g.so_t, St, st));
            for (int j = 0; j < 16; ++j) KPD_TRY(place(g.WrbfT + (size_t)j * p.so, 1, w + St + j, k, g.so_t, 1, st));   // column j -> row j
            return place(p.Ws.w, h, w + St + 16, k, g.so_t, h, st);
        }
        const int k = g.si_t + h;
        KPD_TRY(want_shape(name, shape, ndim, {g.so_t, k}));
        KPD_TRY(place(p.Ws.w, p.si + h, w, k, g.so_t, g.si_t, st));
        return place(p.Ws.w + p.si, p.si + h, w + g.si_t, k, g.so_t, h, st);
    }
    if (tail == "to_feats_out.0.bias") {
        KPD_TRY(want_shape(name, shape, ndim, {g.so_t}));
        return place(p.bs.w, g.so_t, w, g.so_t, 1, g.so_t, st);
    }
    if (tail == "scalar_to_vector_gates.weight") {
        KPD_TRY(want_shape(name, shape, ndim, {p.vo, g.so_t}));
        return place(p.Wg.w, p.so, w, g.so_t, p.vo, g.so_t, st);
    }
    KPD_TRY(want_shape(name, shape, ndim, {p.vo}));        // scalar_to_vector_gates.bias
    return place(p.bg.w, p.vo, w, p.vo, 1, p.vo, st);
}

}  // namespace

kpd_status gvp_wide_create(const kpd_gvp_config &c, GvpWide **out) {
    KPD_REQUIRE(c.n_hidden_scalars > 256 && c.n_hidden_scalars <= GVP_WIDE_MAX_S, KPD_ERR_INVALID,
                "n_hidden_scalars=%d: the wide path covers 257 .. %d", c.n_hidden_scalars, GVP_WIDE_MAX_S);
    GvpWide *m = new GvpWide();
    m->cfg = c;
    m->St = c.n_hidden_scalars;
    m->Sw = up4(m->St);
    m->V = c.vector_size;
    m->fin4[0] = up4(c.n_lig_scalars + 1);
    m->fin4[1] = up4(c.n_kp_scalars + 1);
    const int S = m->St, Sw = m->Sw, V = m->V, C = c.n_convs;
    m->msg.resize(C); m->upd.resize(C); m->ln1w.resize(C); m->ln1b.resize(C); m->ln2w.resize(C); m->ln2b.resize(C);
    for (int i = 0; i < C; ++i) {
        m->msg[i].resize(4); m->upd[i].resize(2);
        m->ln1w[i].assign(2, nullptr); m->ln1b[i].assign(2, nullptr); m->ln2w[i].assign(2, nullptr); m->ln2b[i].assign(2, nullptr);
    }
    m->noise.resize(c.n_noise_gvps);
    m->warena.poison_at = 1 << 30;             // pads are zeros by contract (never poisoned)
    const kpd_status st = carve(m->warena, ARENA_TAIL, [&](Carve &A) {
        for (int i = 0; i < C; ++i) {
            const std::string pre = "noise_predictor.conv_layers." + std::to_string(i) + ".";
            const int net = m->n_et(i), nnt = net == 4 ? 2 : 1;
            for (int et = 0; et < net; ++et) {
                m->msg[i][et].resize(c.n_message_gvps);
                for (int j = 0; j < c.n_message_gvps; ++j)
                    carve_gvp(A, m->msg[i][et][j], j == 0 ? V + 1 : V, V, S, S, j == 0 ? 0 : Sw, Sw, j == 0, Sw, m->expected,
                              pre + "edge_message_fns." + kCanonW[et] + "." + std::to_string(j));
            }
            for (int nt = 0; nt < nnt; ++nt) {
                m->upd[i][nt].resize(c.n_update_gvps);
                for (int j = 0; j < c.n_update_gvps; ++j)
                    carve_gvp(A, m->upd[i][nt][j], V, V, S, S, Sw, Sw, false, Sw, m->expected,
                              pre + "node_update_fns." + kNtNameW[nt] + "." + std::to_string(j));
                A(m->ln1w[i][nt], Sw); A(m->ln1b[i][nt], Sw);
                A(m->ln2w[i][nt], Sw); A(m->ln2b[i][nt], Sw);
                for (const char *s : {".feat_norm.weight", ".feat_norm.bias"}) {
                    m->expected.insert(pre + "message_layer_norms." + kNtNameW[nt] + s);
                    m->expected.insert(pre + "update_layer_norms." + kNtNameW[nt] + s);
                }
            }
        }
        for (int j = 0; j < c.n_noise_gvps; ++j) {
            const bool last = j == c.n_noise_gvps - 1;
            carve_gvp(A, m->noise[j], V, last ? 1 : V, S, last ? 64 : S, Sw, last ? 64 : Sw, false, Sw, m->expected,
                      "noise_predictor.noise_predictor.gvps." + std::to_string(j));
        }
        for (int nt = 0; nt < 2; ++nt) {
            A(m->enc_W[nt], (size_t)Sw * m->fin4[nt]); A(m->enc_b[nt], Sw);
            A(m->enc_lw[nt], Sw); A(m->enc_lb[nt], Sw);
            const std::string e = std::string(kNtNameW[nt]) + "_encoder.";
            for (const char *s : {"0.weight", "0.bias", "2.weight", "2.bias"}) m->expected.insert(e + s);
        }
        A(m->out_W, (size_t)c.n_lig_scalars * 64);
        A(m->out_b, c.n_lig_scalars);
        m->expected.insert("noise_predictor.noise_predictor.to_scalar_output.weight");
        m->expected.insert("noise_predictor.noise_predictor.to_scalar_output.bias");
    });
    if (st != KPD_OK) {
        gvp_wide_destroy(m);
        return st;
    }
    *out = m;
    return KPD_OK;
}

void gvp_wide_destroy(GvpWide *m) {
    if (!m) return;
    m->warena.release();
    m->ws.release();
    delete m;
}

kpd_status gvp_wide_load_weight(GvpWide *m, const char *name, const float *w, const int64_t *shape, int ndim, hipStream_t st) {
    const std::string nm(name);
    KPD_REQUIRE(m->expected.count(nm), KPD_ERR_WEIGHTS, "unknown or unused weight name '%s' for this configuration", name);
    const int St = m->St;
    const std::vector<std::string> tk = split_dots(nm);
    auto tail_from = [&](size_t i) {
        std::string t;
        for (size_t k = i; k < tk.size(); ++k) t += (k > i ? "." : "") + tk[k];
        return t;
    };
    if (tk[0] == "lig_encoder" || tk[0] == "kp_encoder") {
        const int nt = tk[0] == "lig_encoder" ? 0 : 1;
        const int fin = (nt == 0 ? m->cfg.n_lig_scalars : m->cfg.n_kp_scalars) + 1;
        const bool is_w = tk[2] == "weight";
        if (tk[1] == "0") {
            if (is_w) { KPD_TRY(want_shape(name, shape, ndim, {St, fin})); KPD_TRY(place(m->enc_W[nt], m->fin4[nt], w, fin, St, fin, st)); }
            else { KPD_TRY(want_shape(name, shape, ndim, {St})); KPD_TRY(place(m->enc_b[nt], St, w, St, 1, St, st)); }
        } else {
            KPD_TRY(want_shape(name, shape, ndim, {St}));
            KPD_TRY(place(is_w ? m->enc_lw[nt] : m->enc_lb[nt], St, w, St, 1, St, st));
        }
    } else if (tk[1] == "noise_predictor") {
        if (tk[2] == "to_scalar_output") {
            const int F = m->cfg.n_lig_scalars;
            if (tk[3] == "weight") { KPD_TRY(want_shape(name, shape, ndim, {F, 64})); KPD_TRY(place(m->out_W, 64, w, 64, F, 64, st)); }
            else { KPD_TRY(want_shape(name, shape, ndim, {F})); KPD_TRY(place(m->out_b, F, w, F, 1, F, st)); }
        } else {   // noise_predictor.noise_predictor.gvps.<j>.<param>
            KPD_TRY(load_gvp(m->noise[atoi(tk[3].c_str())], tail_from(4), name, w, shape, ndim, St, st));
        }
    } else {       // noise_predictor.conv_layers.<i>.<block>.<key>...
        const int i = atoi(tk[2].c_str());
        const std::string &blk = tk[3];
        if (blk == "edge_message_fns") {
            int et = -1;
            for (int e = 0; e < 4; ++e)
                if (tk[4] == kCanonW[e]) et = e;
            KPD_TRY(load_gvp(m->msg[i][et][atoi(tk[5].c_str())], tail_from(6), name, w, shape, ndim, St, st));
        } else if (blk == "node_update_fns") {
            const int nt = tk[4] == "lig" ? 0 : 1;
            KPD_TRY(load_gvp(m->upd[i][nt][atoi(tk[5].c_str())], tail_from(6), name, w, shape, ndim, St, st));
        } else {   // message_layer_norms / update_layer_norms .<nt>.feat_norm.<param>
            const int nt = tk[4] == "lig" ? 0 : 1;
            const bool is_w = tk[6] == "weight";
            KPD_TRY(want_shape(name, shape, ndim, {St}));
            float *dst = blk == "message_layer_norms" ? (is_w ? m->ln1w[i][nt] : m->ln1b[i][nt]) : (is_w ? m->ln2w[i][nt] : m->ln2b[i][nt]);
            KPD_TRY(place(dst, St, w, St, 1, St, st));
        }
    }
    m->loaded.insert(nm);
    m->committed = false;
    return KPD_OK;
}

kpd_status gvp_wide_commit(GvpWide *m) {
    for (const std::string &n : m->expected)
        KPD_REQUIRE(m->loaded.count(n), KPD_ERR_WEIGHTS, "weight '%s' was never loaded (%zu of %zu loaded)", n.c_str(), m->loaded.size(),
                    m->expected.size());
    KPD_HIP(hipDeviceSynchronize());
    m->committed = true;
    return KPD_OK;
}

kpd_status gvp_wide_reserve(GvpWide *m, int max_B, int max_n_lig, int max_n_kp, int max_n_kk, int max_lig_pg, int max_kp_pg) {
    if (max_B <= m->cap_B && max_n_lig <= m->cap_lig && max_n_kp <= m->cap_kp && max_n_kk <= m->cap_kk && max_lig_pg <= m->cap_maxlig &&
        max_kp_pg <= m->cap_maxkp)
        return KPD_OK;
    max_B = std::max(max_B, m->cap_B); max_n_lig = std::max(max_n_lig, m->cap_lig); max_n_kp = std::max(max_n_kp, m->cap_kp);
    max_n_kk = std::max(max_n_kk, m->cap_kk); max_lig_pg = std::max(max_lig_pg, m->cap_maxlig); max_kp_pg = std::max(max_kp_pg, m->cap_maxkp);
    kpd_lig_graph &g = m->lg;
    KPD_TRY(lig_graph_caps(m->cfg.ll_k, m->cfg.kl_k, max_n_lig, max_n_kp, max_lig_pg, g));
    const size_t Sw = m->Sw, V = m->V;
    const int nmax = std::max(max_n_lig, max_n_kp);
    // rows of the per-edge (and node-chain) scratch: every edge type's capacity and the node counts, + 4 (the products' M is a count
    // rounded up to 4)
    const int rows = up4(std::max(std::max(g.cap_ll, g.cap_kl), std::max(max_n_kk, nmax)) + 4);
    KPD_REQUIRE((long long)rows * (long long)Sw < (1ll << 31), KPD_ERR_CAPACITY,
                "%d edges x %zu columns of edge scratch exceed 2^31 floats (split the batch)", rows, Sw);
    const int n[2] = {max_n_lig, max_n_kp};
    const size_t fin4 = std::max(m->fin4[0], m->fin4[1]);
    KPD_TRY(carve(m->ws, ARENA_TAIL, [&](Carve &C) {
        for (int nt = 0; nt < 2; ++nt) {
            C(m->s[nt], ((size_t)n[nt] + 4) * Sw);
            C(m->v[nt], ((size_t)n[nt] + 4) * 3 * V);
            C(m->agg_s[nt], (size_t)n[nt] * Sw);
            C(m->agg_v[nt], (size_t)n[nt] * 3 * V);
            C(m->bidx[nt], n[nt]);
            C(m->z[nt], max_B);
        }
        C(m->X, ((size_t)nmax + 4) * fin4);
        C(m->P, ((size_t)nmax + 4) * Sw);
        for (int k = 0; k < 2; ++k) { C(m->es[k], (size_t)rows * Sw); C(m->ev[k], (size_t)rows * 3 * V); }
        C(m->vin, (size_t)rows * 3 * (V + 1));
        C(m->Vh, (size_t)rows * 3 * (V + 1));
        C(m->Vu, (size_t)rows * 3 * V);
        C(m->sh, (size_t)rows * (V + 1));
        C(m->gate, (size_t)rows * V);
        carve_lig_graph(C, m->meta4, m->ll_deg, m->ll_off, m->kl_off, m->kl_pg, g, max_B, max_n_lig, max_n_kp);
    }));
    m->cap_B = max_B; m->cap_lig = max_n_lig; m->cap_kp = max_n_kp; m->cap_kk = max_n_kk;
    m->cap_maxlig = max_lig_pg; m->cap_maxkp = max_kp_pg; m->rows = rows;
    return KPD_OK;
}

kpd_status gvp_wide_forward(GvpWide *m, const kpd_batch *bt, const float *t_dev, float *eps_h, float *eps_x, hipStream_t st) {
    KPD_REQUIRE(m->committed, KPD_ERR_STATE, "kpd_gvp_forward before kpd_gvp_commit");
    KPD_REQUIRE(bt->B <= m->cap_B && bt->n_lig <= m->cap_lig && bt->n_kp <= m->cap_kp && bt->n_kk <= m->cap_kk &&
                    bt->max_lig <= m->cap_maxlig && bt->max_kp <= m->cap_maxkp,
                KPD_ERR_CAPACITY, "batch (B=%d lig=%d kp=%d kk=%d maxlig=%d maxkp=%d) exceeds reserved workspace (%d %d %d %d %d %d)",
                bt->B, bt->n_lig, bt->n_kp, bt->n_kk, bt->max_lig, bt->max_kp, m->cap_B, m->cap_lig, m->cap_kp, m->cap_kk,
                m->cap_maxlig, m->cap_maxkp);
    const kpd_gvp_config &c = m->cfg;
    const int St = m->St, Sw = m->Sw, V = m->V;
    const int n[2] = {bt->n_lig, bt->n_kp};
    const int *n_live[2] = {bt->lig_ptr + bt->B, bt->kp_ptr + bt->B};       // the node counts on the device
    GvpWideCtx *T = &m->T;
    T->st = st;

    KPD_TRY(launch_node_graph_index(bt->lig_ptr, bt->B, bt->n_lig, m->bidx[0], st));
    KPD_TRY(launch_node_graph_index(bt->kp_ptr, bt->B, bt->n_kp, m->bidx[1], st));
    KPD_TRY(launch_lig_graph(bt, c.ll_cutoff, c.ll_k, c.kl_cutoff, c.kl_k, &m->lg, m->ll_deg, m->ll_off, m->kl_off, m->kl_pg, st));
    // edge counts of all four types (meta4[0 .. 3]); z for message_norm == 0
    const float mn = c.message_norm_mode == 2 ? 0.0f : 1.0f;
    KPD_TRY(launch_egnn_meta(m->lg.counts, bt->n_kk, 0xF, 0x3, bt->lig_ptr, bt->kp_ptr, m->lg.ll_per_graph, bt->kk_rowptr, bt->B,
                             m->kl_off, mn, 1, m->meta4, m->z[0], m->z[1], st));
    // encoders: LayerNorm(SiLU(Linear([h | t])))
    const float *h_in[2] = {bt->lig_h, bt->kp_h};
    const int F_in[2] = {c.n_lig_scalars, c.n_kp_scalars};
    for (int nt = 0; nt < 2; ++nt) {
        const int f4 = m->fin4[nt];
        hipLaunchKernelGGL(k_gw_cat_time, grid1((long long)n[nt] * f4), dim3(256), 0, st, h_in[nt], F_in[nt], t_dev, m->bidx[nt], n[nt], f4,
                           m->X);
        KPD_LAUNCH_CHECK();
        KPD_TRY(sgemm(false, true, up4(n[nt]), Sw, f4, 1.0f, m->X, f4, m->enc_W[nt], f4, 0.0f, m->s[nt], Sw, st, nullptr, 0, nullptr, nullptr,
                      m->enc_b[nt], m->s[nt], n_live[nt]));
        hipLaunchKernelGGL(k_gw_norm, dim3(n[nt]), dim3(256), 0, st, m->s[nt], nullptr, St, Sw, m->enc_lw[nt], m->enc_lb[nt], nullptr, nullptr, V);
        KPD_LAUNCH_CHECK();
    }
    KPD_HIP(hipMemsetAsync(m->v[0], 0, (size_t)bt->n_lig * 3 * V * 4, st));                   // dynamics_gvp.py:179-184
    hipLaunchKernelGGL(k_gw_v_in, grid1((long long)bt->n_kp * 3 * V), dim3(256), 0, st, bt->kp_v, bt->n_kp, V, m->v[1]);
    KPD_LAUNCH_CHECK();

    // host bounds of the edge counts (kpd.h, kpd_build_lig_graph); the device counts (meta4) are the live rows
    const int e_kl = std::min(bt->n_kp * (c.kl_k > 0 ? c.kl_k : std::min(bt->max_lig, 100)), m->lg.cap_kl);
    const int e_ll = std::min(std::max(bt->n_lig * std::min(bt->max_lig - 1, c.ll_k > 0 ? c.ll_k : 200), 1), m->lg.cap_ll);
    const int E_cap[4] = {e_ll, e_kl, e_kl, bt->n_kk};
    const int *esrc[4] = {m->lg.ll_src, m->lg.kl_src, m->lg.lk_src, bt->kk_src};
    const int *edst[4] = {m->lg.ll_dst, m->lg.kl_dst, m->lg.lk_dst, bt->kk_dst};
    const int *rowptr[4] = {m->lg.ll_rowptr, m->lg.kl_rowptr, m->lg.lk_rowptr, bt->kk_rowptr};
    const float *x[2] = {bt->lig_x, bt->kp_x};
    const int n_convs = m->debug_convs >= 0 ? std::min(m->debug_convs, c.n_convs) : c.n_convs;

    // a chain of GVPs over M rows from (s_in, v_in) (s_in null: the head, its pre-activation already in es[0]); the output ends in
    // es[*cur] / ev[*cur]
    auto chain = [&](const std::vector<WideGvp> &gs, int M, const int *live, const float *s_in, const float *v_in, bool last_identity,
                     int *cur) -> kpd_status {
        int o = 0;
        for (size_t j = 0; j < gs.size(); ++j) {
            GvpBuf b;
            b.Vh = m->Vh; b.Vu = m->Vu; b.sh = m->sh; b.gate = m->gate;
            b.pre = b.s = m->es[o]; b.V = m->ev[o];
            const bool ident = last_identity && j + 1 == gs.size();
            KPD_TRY(gvp_fwd(T, gs[j].p, M, s_in, Sw, v_in, b, ident, live));
            s_in = m->es[o]; v_in = m->ev[o];
            o ^= 1;
        }
        *cur = o ^ 1;
        return KPD_OK;
    };

    for (int ci = 0; ci < n_convs; ++ci) {
        const int net = m->n_et(ci), nnt = net == 4 ? 2 : 1;
        int into_last[2] = {-1, -1};
        for (int et = 0; et < net; ++et) into_last[kDstNtW[et]] = et;
        bool first[2] = {true, true};
        for (int et = 0; et < net; ++et) {
            const int snt = kSrcNtW[et], dnt = kDstNtW[et], E = E_cap[et];
            int cur = 0;
            if (E > 0) {
                const std::vector<WideGvp> &gs = m->msg[ci][et];
                KPD_TRY(sgemm(false, true, up4(n[snt]), Sw, Sw, 1.0f, m->s[snt], Sw, gs[0].Wsrc, Sw, 0.0f, m->P, Sw, st, nullptr, 0, nullptr,
                              nullptr, nullptr, nullptr, n_live[snt]));
                hipLaunchKernelGGL(k_gw_edge_in, dim3((unsigned)(((long long)E * (Sw / 4) + 255) / 256)), dim3(256), 0, st, m->meta4 + et, E,
                                   esrc[et], edst[et], x[snt], x[dnt], m->v[snt], V, m->P, Sw, gs[0].WrbfT, 15.0f, m->es[0], m->vin);
                KPD_LAUNCH_CHECK();
                KPD_TRY(chain(gs, up4(E), m->meta4 + et, nullptr, m->vin, false, &cur));
            }
            hipLaunchKernelGGL(k_gw_agg, dim3(cdiv(n[dnt], 2)), dim3(256), 0, st, rowptr[et], n[dnt], m->es[cur], Sw, m->ev[cur], V,
                               m->agg_s[dnt], m->agg_v[dnt], first[dnt] ? 1 : 0, into_last[dnt] == et ? 1 : 0, c.message_norm_mode,
                               c.message_norm, m->z[dnt], m->bidx[dnt]);
            KPD_LAUNCH_CHECK();
            first[dnt] = false;
        }
        for (int nt = 0; nt < nnt; ++nt) {
            hipLaunchKernelGGL(k_gw_norm, dim3(n[nt]), dim3(256), 0, st, m->s[nt], m->agg_s[nt], St, Sw, m->ln1w[ci][nt], m->ln1b[ci][nt],
                               m->v[nt], m->agg_v[nt], V);
            KPD_LAUNCH_CHECK();
            int cur = 0;
            KPD_TRY(chain(m->upd[ci][nt], up4(n[nt]), n_live[nt], m->s[nt], m->v[nt], false, &cur));
            hipLaunchKernelGGL(k_gw_norm, dim3(n[nt]), dim3(256), 0, st, m->s[nt], m->es[cur], St, Sw, m->ln2w[ci][nt], m->ln2b[ci][nt],
                               m->v[nt], m->ev[cur], V);
            KPD_LAUNCH_CHECK();
        }
    }
    int cur = 0;
    KPD_TRY(chain(m->noise, up4(bt->n_lig), n_live[0], m->s[0], m->v[0], true, &cur));
    hipLaunchKernelGGL(k_gw_out, grid1((long long)bt->n_lig * (c.n_lig_scalars + 3)), dim3(256), 0, st, m->es[cur], m->ev[cur], bt->n_lig,
                       m->out_W, m->out_b, c.n_lig_scalars, eps_h, eps_x);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

kpd_status gvp_wide_debug_state(GvpWide *m, const char *what, float *out, int64_t n_floats, hipStream_t st) {
    const std::string w(what);
    if (w.rfind("convs=", 0) == 0) {
        m->debug_convs = atoi(w.c_str() + 6);
        return KPD_OK;
    }
    if (w == "gemm=f32") return KPD_OK;
    KPD_REQUIRE(w != "gemm=f16x2", KPD_ERR_INVALID,
                "gemm=f16x2: the f16x2 mode covers n_hidden_scalars = 256; n_hidden_scalars = %d runs the exact fp32 path only", m->St);
    if (w == "ws_bytes") {          // bytes of the reserved workspace, as one float (diagnostics)
        const float b = (float)m->ws.cap;
        KPD_REQUIRE(out && n_floats >= 1, KPD_ERR_INVALID, "ws_bytes needs one float");
        KPD_HIP(hipMemcpyAsync(out, &b, 4, hipMemcpyHostToDevice, st));
        KPD_HIP(hipStreamSynchronize(st));
        return KPD_OK;
    }
    set_error("debug tap '%s' is not available for n_hidden_scalars = %d (the wide path offers convs=, gemm=f32, ws_bytes)", what, m->St);
    return KPD_ERR_INVALID;
}

kpd_status gvp_wide_last_counts(GvpWide *m, int32_t out[8], hipStream_t st) {
    for (int i = 0; i < 8; ++i) out[i] = 0;                          // out[7] = 0: exact fp32
    if (!m->ws.base) return KPD_OK;
    int host[25];
    KPD_HIP(hipMemcpyAsync(host, m->meta4, sizeof(host), hipMemcpyDeviceToHost, st));
    KPD_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) out[i] = host[i];
    out[4] = host[8];
    out[5] = host[16 + 8];
    out[6] = host[16] + host[17];
    return KPD_OK;
}

}  // namespace kpd
