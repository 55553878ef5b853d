// Small kernels shared by the two keypoint receptor encoders (defined in rec_encoder.hip).
#pragma once
#include "engine.h"

namespace kpd {

// out[i] = i * scale, i < n
kpd_status launch_iota_scaled(int *out, int n, int scale, hipStream_t st);
// per-graph mean of node rows [n][S] -> [B][S]   (dgl.readout_nodes mean)
kpd_status launch_graph_mean(const float *s, const int *ptr, int B, int S, float *out, hipStream_t st);
// out[node][:] = Wt^T in[node][:], Wt = square weight stored transposed [in][out], S <= 256
kpd_status launch_linear_rows(const float *in, int n, int S, const float *Wt, float *out, hipStream_t st);
// attention-pooled keypoint positions: softmax over all receptor atoms of the keypoint's graph of <ft_src, ft_dst> / sqrt(S),
// exponentiated without max-subtraction as upstream; kp_x = sum_r softmax * rec_x[r]
kpd_status launch_kp_attention(const float *ft_src, const float *ft_dst, const float *rec_x, const int *rec_ptr, int n_kp, int K,
                               int S, float *kp_x, hipStream_t st);
// message_norm == 0: z[b] = edges into graph b's destination nodes (rowptr: CSR over them) / its destination nodes (ptr)
kpd_status launch_indegree_ratio(const int *rowptr, const int *ptr, int B, float *z, hipStream_t st);
// g[r][:] += dmean[graph(r)][:] / n_graph, r < n   (backward of launch_graph_mean)
kpd_status launch_graph_mean_bwd(const float *dmean, const int *bidx, const int *ptr, int n, int S, float *g, hipStream_t st);
// the training engines' attention pooling, S <= 256: as launch_kp_attention over the positions rec_x, and keeps the softmax weights
// w[r * K + k]
kpd_status launch_att_fwd(const float *ft_src, const float *ft_dst, const float *rec_x, const int *rec_ptr, int n_kp, int K, int S,
                          float *w, float *kp_x, hipStream_t st);
// its backward, given dkp_x: w <- the gradient G of the logits <ft_src[r], ft_dst[kp]>; then dft_dst [n_kp][S] and dft_src [n_rec][S]
kpd_status launch_att_bwd_logits(float *w, const float *rec_x, const int *rec_ptr, int n_kp, int K, int S, const float *dkp_x,
                                 const float *kp_x, hipStream_t st);
kpd_status launch_att_bwd_dst(const float *G, const float *ft_src, const int *rec_ptr, int n_kp, int K, int S, float *dft_dst,
                              hipStream_t st);
kpd_status launch_att_bwd_src(const float *G, const float *ft_dst, const int *bidx, int n_rec, int K, int S, float *dft_src,
                              hipStream_t st);

}  // namespace kpd
