// The EGNN denoiser at hidden_nf 257 .. 1024 (inference): a composed layer on the library's fp32 MFMA GEMM (sgemm.hip).
//
// Width W = hidden_nf + 1 (features, then the timestep: upstream's own [h, t] order, dynamics.py:359-363), row stride LDW = W rounded
// up to a multiple of 4; the pad columns hold zeros (zero weight rows / columns, zero biases).  Per layer (LigRecConv.forward,
// dynamics.py:124-207; oracle/egnn.py egnn_conv):
//   1. P[nt] = h[nt] Wp[nt]^T (+ b1 on the dst slots): the first Linear of every (edge, coord) x (src, dst) slot, once per NODE
//      (DESIGN section 2.2), one GEMM per node type over the prefix of slots the layer's edge types use;
//   2. per active edge type, coordinate branch then edge branch:
//        k_wide_gather  A1[e] = SiLU(P_src[src] + P_dst[dst] + d_e w_r)
//        sgemm          A2 = SiLU(A1 W2^T + b2)  (bias + SiLU epilogue, activated output only; live rows = the device edge count)
//        k_wide_head    coord: xm[e] = (tanh(A2[e] . w3) coords_range | A2[e] . w3) x_diff / (d_e + 1);  edge: att[e] = sigmoid(A2[e] . wa + ba)
//        k_wide_agg     node-parallel sum over the dst-sorted CSR into [h | agg] (and x_agg): edges in CSR order, edge types in the
//                       order ll, kl, lk, kk, the last one into a node type divides by z -- no atomics, a node's bits do not depend on
//                       the batch;
//   3. per updated node type: U1 = SiLU([h | agg / z] Wa^T + b0), U2 = U1 Wb^T + b2, then k_wide_finish: h = LN(h + U2) over the
//      W true columns, x += x_agg / z.
// The final layer runs ll + kl and the ligand update only.  Every GEMM is an A B^T product with M a multiple of 4
// (never a fringe row), N and K multiples of 4 (never a fringe column) and no split along K: each output element is one MFMA chain
// over K in slab order, whatever M, the row's position or the tile shape (sgemm.h).
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "egnn_wide.h"
#include "sgemm.h"

namespace kpd {

namespace {

const int kSrcNt[4] = {NT_LIG, NT_KP, NT_LIG, NT_KP};
const int kDstNt[4] = {NT_LIG, NT_LIG, NT_KP, NT_KP};
const int kSrcSlot[4] = {0, 0, 6, 4};
const int kDstSlot[4] = {2, 4, 2, 6};
const char *kEtName[4] = {"ll", "kl", "lk", "kk"};
const char *kNtName[2] = {"lig", "kp"};

typedef float wf4 __attribute__((ext_vector_type(4)));

inline int round4(int v) { return (v + 3) & ~3; }

__device__ __forceinline__ float wsilu(float v) { return v / (1.0f + __expf(-v)); }

// ---- encoders (dynamics.py:313-318, 355-363): out[node][0 .. H-1] = SiLU(W1 SiLU(W0 in + b0) + b1), [H] = t[graph], pads 0 ----
constexpr int WE_NODES = 8;
__global__ __launch_bounds__(256) void k_wide_embed(const float *__restrict__ in, int n, int fin, const float *__restrict__ W0,
                                                    const float *__restrict__ b0, int hid, const float *__restrict__ W1,
                                                    const float *__restrict__ b1, int H, int ldw, const float *__restrict__ t,
                                                    const int *__restrict__ bidx, float *__restrict__ out, int ldo) {
    __shared__ float s_in[WE_NODES][256];
    __shared__ float s_hid[WE_NODES][512];
    const int node0 = blockIdx.x * WE_NODES, tid = threadIdx.x;
    for (int i = tid; i < WE_NODES * fin; i += 256) {
        const int j = i / fin, k = i - j * fin;
        s_in[j][k] = node0 + j < n ? in[(size_t)(node0 + j) * fin + k] : 0.0f;
    }
    __syncthreads();
    for (int u = tid; u < hid; u += 256) {
        float a[WE_NODES];
#pragma unroll
        for (int j = 0; j < WE_NODES; ++j) a[j] = b0[u];
        for (int k = 0; k < fin; ++k) {
            const float w = W0[(size_t)u * fin + k];
#pragma unroll
            for (int j = 0; j < WE_NODES; ++j) a[j] = fmaf(w, s_in[j][k], a[j]);
        }
#pragma unroll
        for (int j = 0; j < WE_NODES; ++j) s_hid[j][u] = wsilu(a[j]);
    }
    __syncthreads();
    for (int c = tid; c < ldw; c += 256) {
        float a[WE_NODES];
#pragma unroll
        for (int j = 0; j < WE_NODES; ++j) a[j] = c < H ? b1[c] : 0.0f;
        if (c < H) {
            for (int u = 0; u < hid; ++u) {
                const float w = W1[(size_t)c * hid + u];
#pragma unroll
                for (int j = 0; j < WE_NODES; ++j) a[j] = fmaf(w, s_hid[j][u], a[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < WE_NODES; ++j)
            if (node0 + j < n) out[(size_t)(node0 + j) * ldo + c] = c < H ? wsilu(a[j]) : (c == H ? t[bidx[node0 + j]] : 0.0f);
    }
}

// ---- decoder (dynamics.py:320-324, 376-381): one wave per ligand atom; eps_h = W1 SiLU(W0 h[:H] + b0) + b1, eps_x = x - x_0 ----
// HMAX bounds the hidden layer 2 atom_nf: 64 (atom_nf <= 32, one output per lane) or 512 (atom_nf <= 256, outputs 64 apart per lane)
template <int HMAX>
__global__ __launch_bounds__(64) void k_wide_decode(const float *__restrict__ h, int ldh, int H, const float *__restrict__ x,
                                                    const float *__restrict__ x0, int n, int atom_nf, const float *__restrict__ W0,
                                                    const float *__restrict__ b0, const float *__restrict__ W1,
                                                    const float *__restrict__ b1, float *__restrict__ eps_h, float *__restrict__ eps_x) {
    __shared__ float s_hid[HMAX];
    const int v = blockIdx.x, lane = threadIdx.x, hid = 2 * atom_nf;
    if (v >= n) return;
    const float *hr = h + (size_t)v * ldh;
    for (int u = 0; u < hid; ++u) {
        float s = 0.0f;
        for (int c = lane; c < H; c += 64) s = fmaf(hr[c], W0[(size_t)u * H + c], s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) s_hid[u] = wsilu(s + b0[u]);
    }
    __syncthreads();
    if constexpr (HMAX <= 64) {
        if (lane < atom_nf) {
            float s = b1[lane];
            for (int u = 0; u < hid; ++u) s = fmaf(W1[(size_t)lane * hid + u], s_hid[u], s);
            eps_h[(size_t)v * atom_nf + lane] = s;
        }
    } else {
        for (int o = lane; o < atom_nf; o += 64) {
            float s = b1[o];
            for (int u = 0; u < hid; ++u) s = fmaf(W1[(size_t)o * hid + u], s_hid[u], s);
            eps_h[(size_t)v * atom_nf + o] = s;
        }
    }
    if (lane < 3) eps_x[(size_t)v * 3 + lane] = x[(size_t)v * 3 + lane] - x0[(size_t)v * 3 + lane];
}

__device__ __forceinline__ float edge_dist(const float *xs, const float *xd, int s, int d, float *dx) {
#pragma unroll
    for (int k = 0; k < 3; ++k) dx[k] = xs[(size_t)s * 3 + k] - xd[(size_t)d * 3 + k];
    return sqrtf(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
}

// ---- A1[e] = SiLU(P_src[src[e]] + P_dst[dst[e]] + d_e w_r): one thread per (edge, 4 columns) ----
__global__ __launch_bounds__(256) void k_wide_gather(const int *__restrict__ e_live, int e_cap, const int *__restrict__ src,
                                                     const int *__restrict__ dst, const float *__restrict__ xs, const float *__restrict__ xd,
                                                     const float *__restrict__ Ps, const float *__restrict__ Pd, int ldp,
                                                     const float *__restrict__ wr, int q4, float *__restrict__ A1) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int e = (int)(gid / q4), q = (int)(gid - (long long)e * q4);
    if (e >= min(*e_live, e_cap)) return;
    const int s = src[e], d = dst[e];
    float dx[3];
    const float dist = edge_dist(xs, xd, s, d, dx);
    const wf4 ps = *reinterpret_cast<const wf4 *>(Ps + (size_t)s * ldp + 4 * q);
    const wf4 pd = *reinterpret_cast<const wf4 *>(Pd + (size_t)d * ldp + 4 * q);
    const wf4 w = *reinterpret_cast<const wf4 *>(wr + 4 * q);
    wf4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = wsilu(fmaf(dist, w[k], ps[k] + pd[k]));
    *reinterpret_cast<wf4 *>(A1 + (size_t)e * (4 * q4) + 4 * q) = o;
}

// ---- heads: one wave per edge.  bias != null (edge branch): att[e] = sigmoid(A2[e] . w + *bias); else (coordinate branch)
// xm[e][0..2] = c x_diff / (d_e + 1), c = tanh(A2[e] . w) coords_range (use_tanh) or A2[e] . w ----
__global__ __launch_bounds__(256) void k_wide_head(const int *__restrict__ e_live, int e_cap, const float *__restrict__ A2, int q4,
                                                   const float *__restrict__ w, const float *__restrict__ bias, const int *__restrict__ src,
                                                   const int *__restrict__ dst, const float *__restrict__ xs, const float *__restrict__ xd,
                                                   int use_tanh, float coords_range, float *__restrict__ att, float *__restrict__ xm) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= min(*e_live, e_cap)) return;
    const float *row = A2 + (size_t)e * (4 * q4);
    float s = 0.0f;
    for (int q = lane; q < q4; q += 64) {
        const wf4 a = *reinterpret_cast<const wf4 *>(row + 4 * q), b = *reinterpret_cast<const wf4 *>(w + 4 * q);
        s = fmaf(a[0], b[0], s); s = fmaf(a[1], b[1], s); s = fmaf(a[2], b[2], s); s = fmaf(a[3], b[3], s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane != 0) return;
    if (bias) {
        att[e] = 1.0f / (1.0f + __expf(-(s + *bias)));
        return;
    }
    float dx[3];
    const float dist = edge_dist(xs, xd, src[e], dst[e], dx);
    const float c = use_tanh ? tanhf(s) * coords_range : s;
#pragma unroll
    for (int k = 0; k < 3; ++k) xm[(size_t)e * 4 + k] = c * (dx[k] / (dist + 1.0f));
}

// ---- segmented sums over the dst-sorted CSR: two nodes per workgroup, 128 threads per node.  agg (row stride ldh) and x_agg [n][4]
// continue from what the previous edge type into this node type left (first: from zero); last: divided by z[graph] ----
__global__ __launch_bounds__(256) void k_wide_agg(const int *__restrict__ rowptr, int n, const float *__restrict__ A2, int q4,
                                                  const float *__restrict__ att, const float *__restrict__ xm, float *__restrict__ agg, int ldh,
                                                  float *__restrict__ xagg, int first, int last, const float *__restrict__ z,
                                                  const int *__restrict__ bidx) {
    const int t = threadIdx.x & 127, node = blockIdx.x * 2 + (threadIdx.x >> 7);
    if (node >= n) return;
    const int e0 = rowptr[node], e1 = rowptr[node + 1];
    const float zz = last ? z[bidx[node]] : 1.0f;
    for (int q = t; q < q4; q += 128) {
        wf4 acc = first ? wf4(0.0f) : *reinterpret_cast<const wf4 *>(agg + (size_t)node * ldh + 4 * q);
        for (int e = e0; e < e1; ++e) {
            const float a = att[e];
            const wf4 v = *reinterpret_cast<const wf4 *>(A2 + (size_t)e * (4 * q4) + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += v[k] * a;
        }
        if (last) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = acc[k] / zz;
        }
        *reinterpret_cast<wf4 *>(agg + (size_t)node * ldh + 4 * q) = acc;
    }
    if (t < 3) {
        float acc = first ? 0.0f : xagg[(size_t)node * 4 + t];
        for (int e = e0; e < e1; ++e) acc += xm[(size_t)e * 4 + t];
        xagg[(size_t)node * 4 + t] = last ? acc / zz : acc;
    }
}

// ---- h = LN(h + U2) over the W true columns (norm; else h + U2), pads 0; x += x_agg (already / z).  One workgroup per node ----
constexpr int WF_PER = 5;          // columns per thread: 5 x 256 >= 1028 = LDW at hidden_nf 1024
__device__ __forceinline__ float block_sum(float v, float *red) {
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
__global__ __launch_bounds__(256) void k_wide_finish(float *__restrict__ h, int ldh, const float *__restrict__ U2, int W, int ldw, int norm,
                                                     const float *__restrict__ lnw, const float *__restrict__ lnb, float *__restrict__ x,
                                                     const float *__restrict__ xagg) {
    __shared__ float red[256];
    const int node = blockIdx.x, tid = threadIdx.x;
    float *hr = h + (size_t)node * ldh;
    const float *ur = U2 + (size_t)node * ldw;
    float v[WF_PER];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < WF_PER; ++i) {
        const int c = tid + 256 * i;
        v[i] = c < W ? hr[c] + ur[c] : 0.0f;
        s += v[i];
    }
    if (norm) {
        const float mean = block_sum(s, red) / (float)W;
        float s2 = 0.0f;
#pragma unroll
        for (int i = 0; i < WF_PER; ++i) {
            const int c = tid + 256 * i;
            v[i] = c < W ? v[i] - mean : 0.0f;
            s2 += v[i] * v[i];
        }
        const float rstd = 1.0f / sqrtf(block_sum(s2, red) / (float)W + 1e-5f);
#pragma unroll
        for (int i = 0; i < WF_PER; ++i) {
            const int c = tid + 256 * i;
            if (c < W) v[i] = v[i] * rstd * lnw[c] + lnb[c];
        }
    }
#pragma unroll
    for (int i = 0; i < WF_PER; ++i) {
        const int c = tid + 256 * i;
        if (c < ldw) hr[c] = c < W ? v[i] : 0.0f;
    }
    if (tid < 3) x[(size_t)node * 3 + tid] += xagg[(size_t)node * 4 + tid];
}

std::vector<std::string> split(const std::string &s, char c) {
    std::vector<std::string> out;
    size_t p = 0;
    while (true) {
        size_t q = s.find(c, p);
        out.push_back(s.substr(p, q == std::string::npos ? q : q - p));
        if (q == std::string::npos) break;
        p = q + 1;
    }
    return out;
}

int index_of(const char *const *names, int n, const std::string &s) {
    for (int i = 0; i < n; ++i)
        if (s == names[i]) return i;
    return -1;
}

}  // namespace

struct WideLayer {
    float *Wp[2], *bp[2];              // per node type: the first Linears of all 8 slots [8 LDW][LDW], their biases [8 LDW] (dst slots)
    float *wr[4][2];                   // per (et, branch): the d_ij column of the first Linear [LDW]
    float *W2[4][2], *b2[4][2];        //                   second Linear [LDW][LDW], [LDW]
    float *watt[4], *w3[4];            // per et: soft-attention row [LDW] with its bias at [LDW]; coordinate head row [LDW]
    float *Wa[2], *b0[2], *Wb[2], *bb[2], *lnw[2], *lnb[2];      // node MLP [LDW][2 LDW], [LDW][LDW]; LayerNorm
};

struct EgnnWide {
    kpd_egnn_config cfg;
    int H, W, LDW, n_et, n_upd;
    Arena warena, ws;
    std::vector<WideLayer> L;
    float *le_W0, *le_b0, *le_W1, *le_b1, *re_W0, *re_b0, *re_W1, *re_b1, *de_W0, *de_b0, *de_W1, *de_b1;
    std::set<std::string> expected, loaded;
    bool committed = false;
    int debug_layers = -1, prune_last = 1;
    // workspace (valid after reserve)
    int cap_B = 0, cap_lig = 0, cap_kp = 0, cap_kk = 0, cap_maxlig = 0, cap_maxkp = 0, cap_rows = 0;
    float *hA[2], *x[2], *P[2], *z[2], *xagg[2];
    int *bidx[2];
    float *A1, *A2, *att, *xm, *U1, *U2;
    int *meta, *ll_deg, *ll_off, *kl_off, *kl_pg;
    kpd_lig_graph lg;
};

kpd_status wide_create(const kpd_egnn_config &c, EgnnWide **out) {
    KPD_REQUIRE(c.hidden_nf > HID && c.hidden_nf <= WIDE_MAX_HID, KPD_ERR_INVALID, "hidden_nf=%d: the HIP path covers 1 .. %d", c.hidden_nf,
                WIDE_MAX_HID);
    KPD_REQUIRE(c.rec_nf != c.hidden_nf, KPD_ERR_INVALID,
                "rec_nf == hidden_nf = %d (identity keypoint encoder, dynamics.py:326-334) is implemented for hidden_nf = 256 only", c.hidden_nf);
    KPD_REQUIRE(c.rec_nf <= 256, KPD_ERR_INVALID, "rec_nf=%d: the wide path's keypoint encoder takes at most 256 inputs", c.rec_nf);
    KPD_REQUIRE(c.atom_nf >= 1 && c.atom_nf <= 256, KPD_ERR_INVALID, "atom_nf=%d outside 1 .. 256", c.atom_nf);
    EgnnWide *m = new EgnnWide();
    m->cfg = c;
    m->H = c.hidden_nf;
    m->W = c.hidden_nf + 1;
    m->LDW = round4(m->W);
    m->n_et = c.update_kp_feat ? 4 : 2;
    m->n_upd = c.update_kp_feat ? 2 : 1;
    m->L.assign(c.n_layers, WideLayer());
    const size_t LDW = m->LDW, H = m->H;
    const int a = c.atom_nf, r = c.rec_nf;
    m->warena.poison_at = 1 << 30;             // pads are zeros by contract (never poisoned)
    kpd_status st = carve(m->warena, ARENA_TAIL, [&](Carve &A) {
        for (int i = 0; i < c.n_layers; ++i) {
            WideLayer &w = m->L[i];
            const std::string pre = "egnn.conv_layers." + std::to_string(i) + ".";
            for (int nt = 0; nt < 2; ++nt) { A(w.Wp[nt], 8 * LDW * LDW); A(w.bp[nt], 8 * LDW); }
            for (int et = 0; et < m->n_et; ++et) {
                for (int br = 0; br < 2; ++br) { A(w.wr[et][br], LDW); A(w.W2[et][br], LDW * LDW); A(w.b2[et][br], LDW); }
                A(w.watt[et], LDW + 4); A(w.w3[et], LDW);
                const std::string e = kEtName[et];
                for (const char *blk : {"edge_mlp.", "coord_mlp."})
                    for (const char *s : {".0.weight", ".0.bias", ".2.weight", ".2.bias"}) m->expected.insert(pre + blk + e + s);
                m->expected.insert(pre + "coord_mlp." + e + ".4.weight");
                m->expected.insert(pre + "soft_attention." + e + ".0.weight");
                m->expected.insert(pre + "soft_attention." + e + ".0.bias");
            }
            for (int nt = 0; nt < m->n_upd; ++nt) {
                A(w.Wa[nt], 2 * LDW * LDW); A(w.b0[nt], LDW); A(w.Wb[nt], LDW * LDW); A(w.bb[nt], LDW);
                A(w.lnw[nt], LDW); A(w.lnb[nt], LDW);
                const std::string n = kNtName[nt];
                for (const char *s : {".0.weight", ".0.bias", ".2.weight", ".2.bias"}) m->expected.insert(pre + "node_mlp." + n + s);
                if (c.norm) {
                    m->expected.insert(pre + "layer_norm." + n + ".weight");
                    m->expected.insert(pre + "layer_norm." + n + ".bias");
                }
            }
        }
        A(m->le_W0, 64 * a); A(m->le_b0, 64); A(m->le_W1, H * 64); A(m->le_b1, H);
        A(m->re_W0, 2 * r * r); A(m->re_b0, 2 * r); A(m->re_W1, H * 2 * r); A(m->re_b1, H);
        A(m->de_W0, 2 * a * H); A(m->de_b0, 2 * a); A(m->de_W1, 2 * a * a); A(m->de_b1, a);
        for (const char *s : {"lig_encoder.0.weight", "lig_encoder.0.bias", "lig_encoder.2.weight", "lig_encoder.2.bias", "rec_encoder.0.weight",
                              "rec_encoder.0.bias", "rec_encoder.2.weight", "rec_encoder.2.bias", "lig_decoder.0.weight", "lig_decoder.0.bias",
                              "lig_decoder.2.weight", "lig_decoder.2.bias"})
            m->expected.insert(s);
    });
    if (st != KPD_OK) {
        wide_destroy(m);
        return st;
    }
    *out = m;
    return KPD_OK;
}

void wide_destroy(EgnnWide *m) {
    if (!m) return;
    m->warena.release();
    m->ws.release();
    delete m;
}

// rows x cols of a row-major source (row stride lds) into dst (row stride ldd); everything else of dst keeps its zeros
static kpd_status place(float *dst, size_t ldd, const float *src, size_t lds, size_t rows, size_t cols, hipStream_t st) {
    KPD_HIP(hipMemcpy2DAsync(dst, ldd * 4, src, lds * 4, cols * 4, rows, hipMemcpyDeviceToDevice, st));
    return KPD_OK;
}

kpd_status wide_load_weight(EgnnWide *m, const char *name, const float *w, const int64_t *shape, int ndim, hipStream_t st) {
    const kpd_egnn_config &c = m->cfg;
    const std::string nm(name);
    KPD_REQUIRE(m->expected.count(nm), KPD_ERR_WEIGHTS, "unknown or unused weight name '%s' for this configuration", name);
    const std::vector<std::string> tk = split(nm, '.');
    const bool is_w = tk.back() == "weight";
    const int H = m->H, W = m->W, LDW = m->LDW, a = c.atom_nf, r = c.rec_nf;
    auto want = [&](std::initializer_list<int64_t> dims) -> kpd_status {
        bool ok = ndim == (int)dims.size();
        int i = 0;
        for (int64_t d : dims) {
            if (ok && shape[i] != d) ok = false;
            ++i;
        }
        if (!ok) {
            std::string got, exp;
            for (int j = 0; j < ndim; ++j) got += std::to_string(shape[j]) + (j + 1 < ndim ? "," : "");
            for (int64_t d : dims) exp += std::to_string(d) + ",";
            set_error("weight %s has shape [%s], expected [%s] (hidden_nf=%d)", name, got.c_str(), exp.c_str(), H);
            return KPD_ERR_WEIGHTS;
        }
        return KPD_OK;
    };
    auto flat = [&](float *dst, std::initializer_list<int64_t> dims) -> kpd_status {
        KPD_TRY(want(dims));
        size_t n = 1;
        for (int64_t d : dims) n *= (size_t)d;
        KPD_HIP(hipMemcpyAsync(dst, w, n * 4, hipMemcpyDeviceToDevice, st));
        return KPD_OK;
    };
    if (tk[0] == "lig_encoder" || tk[0] == "rec_encoder" || tk[0] == "lig_decoder") {
        const bool lig = tk[0] == "lig_encoder", dec = tk[0] == "lig_decoder";
        const int in0 = dec ? H : lig ? a : r, hid = dec ? 2 * a : lig ? 64 : 2 * r, out1 = dec ? a : H;
        float *W0 = dec ? m->de_W0 : lig ? m->le_W0 : m->re_W0, *B0 = dec ? m->de_b0 : lig ? m->le_b0 : m->re_b0;
        float *W1 = dec ? m->de_W1 : lig ? m->le_W1 : m->re_W1, *B1 = dec ? m->de_b1 : lig ? m->le_b1 : m->re_b1;
        if (tk[1] == "0") KPD_TRY(is_w ? flat(W0, {hid, in0}) : flat(B0, {hid}));
        else KPD_TRY(is_w ? flat(W1, {out1, hid}) : flat(B1, {out1}));
    } else {
        // egnn.conv_layers.<i>.<block>.<et|nt>.<idx>.<param>  |  egnn.conv_layers.<i>.layer_norm.<nt>.<param>
        WideLayer &L = m->L[atoi(tk[2].c_str())];
        const std::string &blk = tk[3];
        if (blk == "layer_norm") {
            const int nt = index_of(kNtName, 2, tk[4]);
            KPD_TRY(flat(is_w ? L.lnw[nt] : L.lnb[nt], {W}));
        } else if (blk == "node_mlp") {
            const int nt = index_of(kNtName, 2, tk[4]);
            if (tk[5] == "0") {
                if (is_w) {
                    KPD_TRY(want({W, 2 * W}));
                    KPD_TRY(place(L.Wa[nt], 2 * LDW, w, 2 * W, W, W, st));                 // [h | agg / z]: h in columns 0 .., agg in LDW ..
                    KPD_TRY(place(L.Wa[nt] + LDW, 2 * LDW, w + W, 2 * W, W, W, st));
                } else {
                    KPD_TRY(flat(L.b0[nt], {W}));
                }
            } else {
                if (is_w) { KPD_TRY(want({W, W})); KPD_TRY(place(L.Wb[nt], LDW, w, W, W, W, st)); }
                else KPD_TRY(flat(L.bb[nt], {W}));
            }
        } else if (blk == "soft_attention") {
            const int et = index_of(kEtName, 4, tk[4]);
            KPD_TRY(is_w ? flat(L.watt[et], {1, W}) : flat(L.watt[et] + LDW, {1}));
        } else {   // edge_mlp / coord_mlp
            const int br = blk == "coord_mlp" ? 1 : 0;
            const int et = index_of(kEtName, 4, tk[4]);
            const int snt = kSrcNt[et], dnt = kDstNt[et], ss = kSrcSlot[et] + br, ds = kDstSlot[et] + br;
            if (tk[5] == "0") {
                if (is_w) {
                    KPD_TRY(want({W, 2 * W + 1}));
                    KPD_TRY(place(L.Wp[snt] + (size_t)ss * LDW * LDW, LDW, w, 2 * W + 1, W, W, st));
                    KPD_TRY(place(L.Wp[dnt] + (size_t)ds * LDW * LDW, LDW, w + W, 2 * W + 1, W, W, st));
                    KPD_TRY(place(L.wr[et][br], 1, w + 2 * W, 2 * W + 1, W, 1, st));
                } else {
                    KPD_TRY(flat(L.bp[dnt] + (size_t)ds * LDW, {W}));
                }
            } else if (tk[5] == "2") {
                if (is_w) { KPD_TRY(want({W, W})); KPD_TRY(place(L.W2[et][br], LDW, w, W, W, W, st)); }
                else KPD_TRY(flat(L.b2[et][br], {W}));
            } else {   // coord_mlp.<et>.4.weight
                KPD_TRY(flat(L.w3[et], {1, W}));
            }
        }
    }
    m->loaded.insert(nm);
    m->committed = false;
    return KPD_OK;
}

kpd_status wide_commit(EgnnWide *m) {
    for (const std::string &n : m->expected)
        KPD_REQUIRE(m->loaded.count(n), KPD_ERR_WEIGHTS, "weight '%s' was never loaded (%zu of %zu loaded)", n.c_str(), m->loaded.size(),
                    m->expected.size());
    KPD_HIP(hipDeviceSynchronize());
    m->committed = true;
    return KPD_OK;
}

kpd_status wide_reserve(EgnnWide *m, int max_B, int max_n_lig, int max_n_kp, int max_n_kk, int max_lig_pg, int max_kp_pg) {
    if (max_B <= m->cap_B && max_n_lig <= m->cap_lig && max_n_kp <= m->cap_kp && max_n_kk <= m->cap_kk && max_lig_pg <= m->cap_maxlig &&
        max_kp_pg <= m->cap_maxkp)
        return KPD_OK;
    max_B = std::max(max_B, m->cap_B); max_n_lig = std::max(max_n_lig, m->cap_lig); max_n_kp = std::max(max_n_kp, m->cap_kp);
    max_n_kk = std::max(max_n_kk, m->cap_kk); max_lig_pg = std::max(max_lig_pg, m->cap_maxlig); max_kp_pg = std::max(max_kp_pg, m->cap_maxkp);
    kpd_lig_graph &g = m->lg;
    KPD_TRY(lig_graph_caps(m->cfg.ll_k, m->cfg.kl_k, max_n_lig, max_n_kp, max_lig_pg, g));
    const size_t LDW = m->LDW;
    // rows of the per-edge scratch: every edge type's capacity rounded up to 4 (the edge GEMMs' M)
    const int rows = round4(std::max(std::max(g.cap_ll, g.cap_kl), std::max(max_n_kk, 1)));
    KPD_REQUIRE((long long)rows * (long long)LDW < (1ll << 31), KPD_ERR_CAPACITY,
                "%d edges x %zu columns of edge scratch exceed 2^31 floats (split the batch)", rows, LDW);
    const int n[2] = {max_n_lig, max_n_kp};
    const int nmax = std::max(max_n_lig, max_n_kp);
    KPD_TRY(carve(m->ws, ARENA_TAIL, [&](Carve &C) {
        for (int nt = 0; nt < 2; ++nt) {
            C.rows(m->hA[nt], (size_t)n[nt] + 4, 2 * LDW, 2 * LDW);      // [h | agg]; + 4: the GEMMs' M is the count rounded up to 4
            C(m->x[nt], (size_t)n[nt] * 3);
            C(m->P[nt], ((size_t)n[nt] + 4) * 8 * LDW);
            C(m->bidx[nt], n[nt]);
            C(m->z[nt], max_B);
            C(m->xagg[nt], (size_t)n[nt] * 4);
        }
        C(m->A1, (size_t)rows * LDW);
        C(m->A2, (size_t)rows * LDW);
        C(m->att, rows);
        C(m->xm, (size_t)rows * 4);
        C(m->U1, ((size_t)nmax + 4) * LDW);
        C(m->U2, ((size_t)nmax + 4) * LDW);
        carve_lig_graph(C, m->meta, m->ll_deg, m->ll_off, m->kl_off, m->kl_pg, g, max_B, max_n_lig, max_n_kp);
    }));
    m->cap_B = max_B; m->cap_lig = max_n_lig; m->cap_kp = max_n_kp; m->cap_kk = max_n_kk;
    m->cap_maxlig = max_lig_pg; m->cap_maxkp = max_kp_pg; m->cap_rows = rows;
    return KPD_OK;
}

kpd_status wide_forward(EgnnWide *m, const kpd_batch *bt, const float *t_dev, float *eps_h, float *eps_x, hipStream_t st) {
    KPD_REQUIRE(m->committed, KPD_ERR_STATE, "kpd_egnn_forward before kpd_egnn_commit");
    KPD_REQUIRE(bt->B <= m->cap_B && bt->n_lig <= m->cap_lig && bt->n_kp <= m->cap_kp && bt->n_kk <= m->cap_kk &&
                    bt->max_lig <= m->cap_maxlig && bt->max_kp <= m->cap_maxkp,
                KPD_ERR_CAPACITY, "batch (B=%d lig=%d kp=%d kk=%d maxlig=%d maxkp=%d) exceeds reserved workspace (%d %d %d %d %d %d)",
                bt->B, bt->n_lig, bt->n_kp, bt->n_kk, bt->max_lig, bt->max_kp, m->cap_B, m->cap_lig, m->cap_kp, m->cap_kk,
                m->cap_maxlig, m->cap_maxkp);
    const kpd_egnn_config &c = m->cfg;
    const int LDW = m->LDW, q4 = LDW / 4, ldh = 2 * LDW, ldp = 8 * LDW;

    KPD_HIP(hipMemcpyAsync(m->x[NT_LIG], bt->lig_x, (size_t)bt->n_lig * 12, hipMemcpyDeviceToDevice, st));
    KPD_HIP(hipMemcpyAsync(m->x[NT_KP], bt->kp_x, (size_t)bt->n_kp * 12, hipMemcpyDeviceToDevice, st));
    KPD_TRY(launch_node_graph_index(bt->lig_ptr, bt->B, bt->n_lig, m->bidx[NT_LIG], st));
    KPD_TRY(launch_node_graph_index(bt->kp_ptr, bt->B, bt->n_kp, m->bidx[NT_KP], st));
    KPD_TRY(launch_lig_graph(bt, c.ll_cutoff, c.ll_k, c.kl_cutoff, c.kl_k, &m->lg, m->ll_deg, m->ll_off, m->kl_off, m->kl_pg, st));
    const int active = c.update_kp_feat ? 0xF : 0x3;
    const bool prune = c.update_kp_feat && m->prune_last;
    const int active_last = prune ? 0x3 : active;
    KPD_TRY(launch_egnn_meta(m->lg.counts, bt->n_kk, active, active_last, bt->lig_ptr, bt->kp_ptr, m->lg.ll_per_graph, bt->kk_rowptr, bt->B,
                             m->kl_off, c.message_norm, c.update_kp_feat, m->meta, m->z[NT_LIG], m->z[NT_KP], st, TM));
    hipLaunchKernelGGL(k_wide_embed, dim3(cdiv(bt->n_lig, WE_NODES)), dim3(256), 0, st, bt->lig_h, bt->n_lig, c.atom_nf, m->le_W0, m->le_b0, 64,
                       m->le_W1, m->le_b1, m->H, LDW, t_dev, m->bidx[NT_LIG], m->hA[NT_LIG], ldh);
    KPD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_wide_embed, dim3(cdiv(bt->n_kp, WE_NODES)), dim3(256), 0, st, bt->kp_h, bt->n_kp, c.rec_nf, m->re_W0, m->re_b0,
                       2 * c.rec_nf, m->re_W1, m->re_b1, m->H, LDW, t_dev, m->bidx[NT_KP], m->hA[NT_KP], ldh);
    KPD_LAUNCH_CHECK();

    // host bounds of the edge counts (kpd.h, kpd_build_lig_graph); the device counts (meta) are the live rows
    const int e_kl = std::min(bt->n_kp * (c.kl_k > 0 ? c.kl_k : std::min(bt->max_lig, 100)), m->lg.cap_kl);
    const int e_ll = std::min(std::max(bt->n_lig * std::min(bt->max_lig - 1, c.ll_k > 0 ? c.ll_k : 200), 1), m->lg.cap_ll);
    const int E_cap[4] = {e_ll, e_kl, e_kl, bt->n_kk};
    const int n[2] = {bt->n_lig, bt->n_kp};
    const int *esrc[4] = {m->lg.ll_src, m->lg.kl_src, m->lg.lk_src, bt->kk_src};
    const int *edst[4] = {m->lg.ll_dst, m->lg.kl_dst, m->lg.lk_dst, bt->kk_dst};
    const int *rowptr[4] = {m->lg.ll_rowptr, m->lg.kl_rowptr, m->lg.lk_rowptr, bt->kk_rowptr};
    const int n_layers = m->debug_layers >= 0 ? std::min(m->debug_layers, c.n_layers) : c.n_layers;

    for (int li = 0; li < n_layers; ++li) {
        const WideLayer &L = m->L[li];
        const bool last = li == n_layers - 1;
        const int etmask = last ? active_last : active;
        const int *meta = last ? m->meta + 16 : m->meta;
        // 1. projections: the slots a layer uses are a prefix of the 8 (lig: ll 0-3, kl 4-5, lk 6-7; kp: kl 0-1, lk 2-3, kk 4-7)
        int slots[2] = {0, 0}, into_last[2] = {-1, -1};
        for (int et = 0; et < 4; ++et)
            if ((etmask >> et) & 1) {
                slots[kSrcNt[et]] = std::max(slots[kSrcNt[et]], kSrcSlot[et] + 2);
                slots[kDstNt[et]] = std::max(slots[kDstNt[et]], kDstSlot[et] + 2);
                into_last[kDstNt[et]] = et;
            }
        for (int nt = 0; nt < 2; ++nt)
            KPD_TRY(sgemm(false, true, round4(n[nt]), slots[nt] * LDW, LDW, 1.0f, m->hA[nt], ldh, L.Wp[nt], LDW, 0.0f, m->P[nt], ldp, st,
                          nullptr, 0, nullptr, nullptr, L.bp[nt]));
        // 2. edge types in the order ll, kl, lk, kk
        bool first[2] = {true, true};
        for (int et = 0; et < 4; ++et) {
            if (!((etmask >> et) & 1)) continue;
            const int snt = kSrcNt[et], dnt = kDstNt[et], E = E_cap[et];
            for (int br = 1; br >= 0; --br) {          // coordinate branch, then the edge branch (its A2 stays for the sum)
                if (E > 0) {
                    const long long threads = (long long)E * q4;
                    hipLaunchKernelGGL(k_wide_gather, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, meta + et, E, esrc[et], edst[et],
                                       m->x[snt], m->x[dnt], m->P[snt] + (size_t)(kSrcSlot[et] + br) * LDW,
                                       m->P[dnt] + (size_t)(kDstSlot[et] + br) * LDW, ldp, L.wr[et][br], q4, m->A1);
                    KPD_LAUNCH_CHECK();
                    KPD_TRY(sgemm(false, true, round4(E), LDW, LDW, 1.0f, m->A1, LDW, L.W2[et][br], LDW, 0.0f, m->A2, LDW, st, nullptr, 0,
                                  nullptr, nullptr, L.b2[et][br], m->A2, meta + et));
                    hipLaunchKernelGGL(k_wide_head, dim3(cdiv(E, 4)), dim3(256), 0, st, meta + et, E, m->A2, q4, br ? L.w3[et] : L.watt[et],
                                       br ? nullptr : L.watt[et] + LDW, esrc[et], edst[et], m->x[snt], m->x[dnt], c.use_tanh, c.coords_range,
                                       m->att, m->xm);
                    KPD_LAUNCH_CHECK();
                }
            }
            hipLaunchKernelGGL(k_wide_agg, dim3(cdiv(n[dnt], 2)), dim3(256), 0, st, rowptr[et], n[dnt], m->A2, q4, m->att, m->xm,
                               m->hA[dnt] + LDW, ldh, m->xagg[dnt], first[dnt] ? 1 : 0, into_last[dnt] == et ? 1 : 0, m->z[dnt],
                               m->bidx[dnt]);
            KPD_LAUNCH_CHECK();
            first[dnt] = false;
        }
        // 3. node updates
        for (int nt = 0; nt < m->n_upd; ++nt) {
            if (nt == NT_KP && last && prune) continue;
            const int M = round4(n[nt]);
            KPD_TRY(sgemm(false, true, M, LDW, ldh, 1.0f, m->hA[nt], ldh, L.Wa[nt], ldh, 0.0f, m->U1, LDW, st, nullptr, 0, nullptr, nullptr,
                          L.b0[nt], m->U1));
            KPD_TRY(sgemm(false, true, M, LDW, LDW, 1.0f, m->U1, LDW, L.Wb[nt], LDW, 0.0f, m->U2, LDW, st, nullptr, 0, nullptr, nullptr,
                          L.bb[nt]));
            hipLaunchKernelGGL(k_wide_finish, dim3(n[nt]), dim3(256), 0, st, m->hA[nt], ldh, m->U2, m->W, LDW, c.norm, L.lnw[nt], L.lnb[nt],
                               m->x[nt], m->xagg[nt]);
            KPD_LAUNCH_CHECK();
        }
    }
    if (c.atom_nf <= 32)
        hipLaunchKernelGGL(k_wide_decode<64>, dim3(bt->n_lig), dim3(64), 0, st, m->hA[NT_LIG], ldh, m->H, m->x[NT_LIG], bt->lig_x, bt->n_lig,
                           c.atom_nf, m->de_W0, m->de_b0, m->de_W1, m->de_b1, eps_h, eps_x);
    else
        hipLaunchKernelGGL(k_wide_decode<512>, dim3(bt->n_lig), dim3(64), 0, st, m->hA[NT_LIG], ldh, m->H, m->x[NT_LIG], bt->lig_x, bt->n_lig,
                           c.atom_nf, m->de_W0, m->de_b0, m->de_W1, m->de_b1, eps_h, eps_x);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

kpd_status wide_debug_state(EgnnWide *m, const char *what, float *out, int64_t n_floats, hipStream_t st) {
    const std::string w(what);
    if (w.rfind("layers=", 0) == 0) {
        m->debug_layers = atoi(w.c_str() + 7);
        return KPD_OK;
    }
    if (w.rfind("prune=", 0) == 0) {
        m->prune_last = atoi(w.c_str() + 6);
        return KPD_OK;
    }
    if (w == "gemm=f32") return KPD_OK;
    KPD_REQUIRE(w != "gemm=f16x2", KPD_ERR_INVALID,
                "gemm=f16x2: the f16x2 mode covers hidden_nf <= 256; hidden_nf = %d runs the exact fp32 path only", m->H);
    if (w == "ws_bytes") {          // bytes of the reserved workspace, as one float (diagnostics)
        const float b = (float)m->ws.cap;
        KPD_REQUIRE(n_floats >= 1, KPD_ERR_INVALID, "ws_bytes needs one float");
        KPD_HIP(hipMemcpyAsync(out, &b, 4, hipMemcpyHostToDevice, st));
        KPD_HIP(hipStreamSynchronize(st));
        return KPD_OK;
    }
    set_error("debug tap '%s' is not available for hidden_nf = %d (the wide path offers layers=, prune=, gemm=f32, ws_bytes)", what, m->H);
    return KPD_ERR_INVALID;
}

kpd_status wide_last_counts(EgnnWide *m, int32_t out[8], hipStream_t st) {
    for (int i = 0; i < 8; ++i) out[i] = 0;                          // out[7] = 0: exact fp32
    if (!m->ws.base) return KPD_OK;
    int host[25];
    KPD_HIP(hipMemcpyAsync(host, m->meta, sizeof(host), hipMemcpyDeviceToHost, st));
    KPD_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 4; ++i) out[i] = host[i];
    out[4] = host[8];
    out[5] = host[16 + 8];
    out[6] = host[16] + host[17] + host[18] + host[19];
    return KPD_OK;
}

}  // namespace kpd
