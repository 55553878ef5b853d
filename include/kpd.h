/*
 * kpd.h -- C ABI of libkpd_hip.so: the MI355X (gfx950) denoising hot path of
 * Dunni3/keypoint-diffusion behind plain pointers and sizes.
 *
 * The reference is pure Python; its "FFI" for this path is the set of third-party native
 * ops it calls every reverse-diffusion step (torch_cluster.radius_graph / knn,
 * DGL apply_edges / multi_update_all, torch.nn.Linear / LayerNorm) from
 *   models/dynamics.py:342-441        LigRecDynamics.forward  (+ LigRecEGNN, LigRecConv)
 *   models/dynamics_gvp.py:149-255    LigRecDynamicsGVP.forward (+ gvp.py GVPMultiEdgeConv)
 *   models/receptor_encoder_gvp.py:212-321  ReceptorEncoderGVP.forward
 *   models/ligand_diffuser.py:497-538 KeypointDiffusion.sample_p_zs_given_zt
 * Each entry point below replaces one of those call sites as a whole and cites it.
 *
 * Conventions
 *   - every pointer named *_dev / marked [dev] is a device (HBM) pointer, fp32 or int32,
 *     contiguous, row-major; everything else is host memory;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no hidden
 *     synchronisation, no allocation inside forward calls (kpd_*_reserve allocates);
 *   - node arrays are flat and graph-major: complex b owns rows [ptr[b], ptr[b+1]);
 *   - every call returns KPD_OK or a negative kpd_status; kpd_last_error() gives text.
 */
#ifndef KPD_H
#define KPD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum kpd_status {
    KPD_OK = 0,
    KPD_ERR_INVALID = -1,      /* bad argument / unsupported configuration              */
    KPD_ERR_CAPACITY = -2,     /* batch larger than the reserved workspace               */
    KPD_ERR_WEIGHTS = -3,      /* unknown weight name, wrong shape, or weights missing   */
    KPD_ERR_HIP = -4,          /* a HIP runtime call failed                              */
    KPD_ERR_STATE = -5         /* call order violated (e.g. forward before commit)       */
} kpd_status;

const char *kpd_last_error(void);
int kpd_version(void);
/* Always 0: the library has one build, and no environment switch of it can make a kernel skip work.  bench.py refuses to print a
 * contract line from a library whose flags are not 0.  (No reference counterpart: the reference has no build variants.) */
int kpd_build_flags(void);

/* ---------------------------------------------------------------------------------------
 * Batch of complexes (the tensors the reference keeps in a batched DGL heterograph).
 * kk edges are static during sampling (ligand_diffuser.py:201-202 translates keypoints
 * rigidly) and are passed dst-sorted with their CSR row pointer.
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_batch {
    int32_t B;                 /* complexes                                              */
    int32_t n_lig, n_kp;       /* total ligand atoms / keypoints                         */
    int32_t max_lig, max_kp;   /* largest per-complex counts (host-known)                */
    const int32_t *lig_ptr;    /* [dev] [B+1]                                            */
    const int32_t *kp_ptr;     /* [dev] [B+1]                                            */
    const float *lig_x;        /* [dev] [n_lig,3]        g.nodes['lig'].data['x_0']      */
    const float *lig_h;        /* [dev] [n_lig,atom_nf]  g.nodes['lig'].data['h_0']      */
    const float *kp_x;         /* [dev] [n_kp,3]                                         */
    const float *kp_h;         /* [dev] [n_kp,rec_nf]                                    */
    const float *kp_v;         /* [dev] [n_kp,V,3] (GVP only, else NULL)                 */
    int32_t n_kk;              /* kk edges                                               */
    const int32_t *kk_src;     /* [dev] [n_kk] sorted by (dst, src)                      */
    const int32_t *kk_dst;     /* [dev] [n_kk]                                           */
    const int32_t *kk_rowptr;  /* [dev] [n_kp+1]                                         */
} kpd_batch;

/* ---------------------------------------------------------------------------------------
 * Per-step ligand graph build.  Replaces add_lig_edges (models/dynamics.py:387-420,
 * models/dynamics_gvp.py:201-234): torch_cluster.radius_graph(lig, r=ll) and
 * torch_cluster.knn(x=lig, y=kp, k) plus the DGL add_edges / batch bookkeeping.
 * Output: dst-sorted COO + CSR row pointers for ll (dst lig), kl (src kp -> dst lig) and
 * lk (src lig -> dst kp), in caller buffers of the stated capacity.
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_lig_graph {
    int32_t cap_ll, cap_kl;    /* capacities (edges) of the arrays below                 */
    int32_t *ll_src, *ll_dst, *ll_rowptr;   /* [dev] [cap_ll],[cap_ll],[n_lig+1]         */
    int32_t *kl_src, *kl_dst, *kl_rowptr;   /* [dev] [cap_kl],[cap_kl],[n_lig+1]         */
    int32_t *lk_src, *lk_dst, *lk_rowptr;   /* [dev] [cap_kl],[cap_kl],[n_kp+1]          */
    int32_t *ll_per_graph;     /* [dev] [B] ll edges per complex                          */
    int32_t *counts;           /* [dev] [2]: {E_ll, E_kl}                                 */
} kpd_lig_graph;

/* ll: radius graph of radius ll_cutoff (ll_k == 0, at most 200 neighbours) or kNN graph (ll_k in 1..16);
 * kl / lk: for every keypoint its kl_k nearest ligand atoms (kl_k in 1..16) or all ligand atoms within kl_cutoff
 * (kl_k == 0, at most 100).  Capacities: cap_ll >= n_lig * min(max_lig - 1, ll_k or 200),
 * cap_kl >= n_kp * (kl_k or min(max_lig, 100)). */
kpd_status kpd_build_lig_graph(const kpd_batch *batch, float ll_cutoff, int32_t ll_k, float kl_cutoff,
                               int32_t kl_k, const kpd_lig_graph *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * EGNN denoiser.  Replaces LigRecDynamics.forward (models/dynamics.py:342-385) including
 * lig/rec encoders, edge build, the LigRecEGNN stack (:266-294, LigRecConv :89-217) and
 * the decoder.  Constructor fields mirror LigRecDynamics.__init__ (:300-340).
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_egnn_config {
    int32_t atom_nf, rec_nf;           /* atom_nf 1 .. 256, rec_nf 1 .. 256 (rec_nf == hidden_nf: identity keypoint encoder, any
                                          hidden_nf <= 256); the same ranges as the trainer.  atom_nf > 32, rec_nf 129 .. 255 and the
                                          identity encoder below hidden_nf 256 run exact fp32 only ("gemm=f16x2" is refused) */
    int32_t n_layers, hidden_nf;       /* hidden_nf 1 .. 256 (the kernels are 256 + 1 wide; narrower models run zero padded: the reference's
                                          default ctor is 255); 257 .. 1024 for inference on the composed wide path (csrc/egnn_wide.hip:
                                          fp32 only, debug taps layers= / prune= only, no kpd_egnn_profile); the trainer takes <= 256;
                                          > 1024 is refused (INTEGRATION.md section 1 lists the limits) */
    int32_t use_tanh, norm, update_kp_feat;
    float message_norm;                /* 0 => per-graph average in-degree + 1           */
    int32_t ll_k, kl_k;                /* 0 = radius graph (the cutoffs below), else kNN, <= 16 */
    float ll_cutoff, kl_cutoff;
    float coords_range;                /* 10 in the reference (dynamics.py:15)           */
} kpd_egnn_config;

typedef struct kpd_egnn kpd_egnn;

kpd_status kpd_egnn_create(const kpd_egnn_config *cfg, kpd_egnn **out);
void kpd_egnn_destroy(kpd_egnn *m);
/* One state-dict tensor of the reference `dynamics` module, by its reference name
 * (e.g. "egnn.conv_layers.3.edge_mlp.kl.2.weight"); repacked on device for the kernels. */
kpd_status kpd_egnn_load_weight(kpd_egnn *m, const char *name, const float *w_dev,
                                const int64_t *shape, int32_t ndim, void *stream);
kpd_status kpd_egnn_commit(kpd_egnn *m);          /* checks every tensor was loaded        */
/* Allocate workspace for batches up to these sizes (grow-only; not stream-ordered). */
kpd_status kpd_egnn_reserve(kpd_egnn *m, int32_t max_B, int32_t max_n_lig, int32_t max_n_kp,
                            int32_t max_n_kk, int32_t max_lig_per_graph, int32_t max_kp_per_graph);
/* eps_h [n_lig, atom_nf], eps_x [n_lig, 3];  t [B] in (0,1]. */
kpd_status kpd_egnn_forward(kpd_egnn *m, const kpd_batch *batch, const float *t_dev,
                            float *eps_h_dev, float *eps_x_dev, void *stream);
/* Debug/test taps and switches.  Taps copy engine state to out_dev: "h_lig" / "h_kp" (node state, row stride 264), "x_lig" /
 * "x_kp", "z_lig" / "z_kp", "xnm<et>" / "xnc<et>" / "hnm<et>" / "hnc<et>" (segment-sum pieces of edge type et as the last layer
 * left them), "kp_table_ok" (n_floats = 1: 1.0 when layer 0 of the last forward took its keypoint projections from the per-class
 * table, 0.0 when it ran per atom).  One-hot kp_h (fixed receptor encoder) is detected on the device at every forward: layer 0 then
 * embeds and projects the B * rec_nf class rows instead of every keypoint, bit-identical to the per-atom path, which any other kp_h
 * falls back to inside the same stream ("kp_table=0" forces it; fp32 mode, rec_nf != hidden_nf and B * rec_nf <= n_kp / 2 only).
 * Switches (n_floats = 0, out_dev ignored but non-null): "layers=N" (run only the first N layers), "prune=0|1", "kp_table=0|1", and
 *   "gemm=f32"   exact fp32 MFMA in every GEMM -- the default and the contract path;
 *   "gemm=f16x2" EXPERIMENTAL, opt-in, never the default and never part of the benchmark's `value`: every fp32 product of the
 *                edge / projection / node-update GEMMs as three f16 MFMA products of hi / lo operand planes with fp32
 *                accumulation (the parity suite holds at the same 1e-4 in this mode, ~2x the step rate).  Status (round 4,
 *                DESIGN.md "f16x2 mode"): a build VARIANT of its edge kernel (batched distance read) showed a first-launch
 *                deviation of one LDS row in rounds 2 - 3; the shipped per-row form has never shown it in any detector, and a
 *                standalone kernel with the suspected ingredients (profiles/tools/f16_lds_row_probe.hip: 20 fresh processes,
 *                80 launches clean) does not reproduce it; in round 4 the variant build itself -- of today's sources and of the
 *                round-3 sources -- is clean in 24 fresh processes on 10 GPUs (profiles/r04_f16_variant_resample.txt), so it is
 *                neither explained nor reproducible any more, nor shown to be a hardware erratum.
 *                Until it is, the mode is frozen as experimental: use it for throughput experiments, not for results you keep.
 *                The environment variable KPD_GEMM=f16x2 selects it at kpd_egnn_create time. */
kpd_status kpd_egnn_debug_state(kpd_egnn *m, const char *what, float *out_dev, int64_t n_floats,
                                void *stream);
/* HIP-event timing of the dominant kernel (the fused edge kernel), recorded on the caller's
 * stream around each of its launches while enabled (up to 8192 launches per enable). */
kpd_status kpd_egnn_profile(kpd_egnn *m, int32_t enable);
kpd_status kpd_egnn_profile_read(kpd_egnn *m, double *total_ms, int32_t *launches);
/* Launch geometry of the last forward: {E_ll, E_kl, E_lk, E_kk, edge tiles of a full layer, edge tiles and edges of the
 * final layer, and in out[7] the GEMM mode in effect (0 exact fp32, 1 f16x2)} -- the final layer runs ll + kl only, since
 * LigRecEGNN.forward returns (h_lig, x_lig) alone (models/dynamics.py:288-294).  Before the first forward only out[7] is set. */
kpd_status kpd_egnn_last_counts(kpd_egnn *m, int32_t out[8], void *stream);

/* ---------------------------------------------------------------------------------------
 * EGNN denoiser, training path: forward that keeps the layer states and the backward pass of
 * LigRecDynamics.forward (models/dynamics.py:342-385), i.e. what torch autograd derives for the loss of
 * KeypointDiffusion.forward (models/ligand_diffuser.py:89-175) in train.py:423-524.  Parameters are bound once by their
 * reference state-dict names and read in place in the reference [out, in] layout (no repacking: they change every
 * optimizer step); each parameter's gradient is ACCUMULATED (+=) into the bound buffer of the same shape, the way
 * autograd accumulates into .grad.  grad may be NULL for a frozen parameter.
 *   forward : eps_h [n_lig, atom_nf], eps_x [n_lig, 3]; the batch tensors and `t` must stay alive until backward.
 *             One host read-back of the edge counts per call (they size the GEMMs).
 *   backward: d_eps_h / d_eps_x = dL/d(eps); any of d_lig_h [n_lig, atom_nf], d_lig_x [n_lig, 3], d_kp_h [n_kp, rec_nf],
 *             d_kp_x [n_kp, 3] may be NULL (written, not accumulated, when given).  Consumes the forward.
 * Memory: reserve() tries to keep the edge activations of every layer (13.5 GB at B = 64 x (300-atom pocket, 25-atom ligand)); if that
 * allocation fails it keeps one layer's worth and recomputes layer by layer in backward (same results, bit for bit).
 * Environment: KPD_TRAIN_STORE=0 (read once per process) selects the recompute mode.
 * profile / profile_read: HIP-event time of the two per-layer edge kernels of a training step on their launch stream, as
 * kpd_egnn_profile does for the inference kernel: index 0 = forward (k_egnn_edge_train), 1 = backward (k_egnn_edge_bwd); `edges` =
 * edges those launches processed (for a FLOP count).  No reference counterpart (bench.py's roofline of the training lines).
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_egnn_trainer kpd_egnn_trainer;
kpd_status kpd_egnn_trainer_create(const kpd_egnn_config *cfg, kpd_egnn_trainer **out);
void kpd_egnn_trainer_destroy(kpd_egnn_trainer *t);
kpd_status kpd_egnn_trainer_bind(kpd_egnn_trainer *t, const char *name, const float *weight_dev, float *grad_dev,
                                 const int64_t *shape, int32_t ndim);
kpd_status kpd_egnn_trainer_reserve(kpd_egnn_trainer *t, int32_t max_B, int32_t max_n_lig, int32_t max_n_kp,
                                    int32_t max_n_kk, int32_t max_lig_per_graph, int32_t max_kp_per_graph);
kpd_status kpd_egnn_trainer_forward(kpd_egnn_trainer *t, const kpd_batch *batch, const float *t_dev, float *eps_h_dev,
                                    float *eps_x_dev, void *stream);
kpd_status kpd_egnn_trainer_backward(kpd_egnn_trainer *t, const float *d_eps_h, const float *d_eps_x, float *d_lig_h,
                                     float *d_lig_x, float *d_kp_h, float *d_kp_x, void *stream);
kpd_status kpd_egnn_trainer_profile(kpd_egnn_trainer *t, int32_t enable);
kpd_status kpd_egnn_trainer_profile_read(kpd_egnn_trainer *t, double total_ms[2], int32_t launches[2], double edges[2]);

/* ---------------------------------------------------------------------------------------
 * GVP denoiser.  Replaces LigRecDynamicsGVP.forward (models/dynamics_gvp.py:149-199): encoders
 * (:124-134), edge build (:201-234), the GVPMultiEdgeConv stack (models/gvp.py:343-551; GVP :43-116,
 * GVPLayerNorm :152-166) and the NoisePredictionBlock (:10-44).  Fields mirror
 * LigRecDynamicsGVP.__init__ (:106-147).  kpd_batch.kp_v carries the keypoint vector features v_0.
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_gvp_config {
    int32_t n_lig_scalars, n_kp_scalars; /* n_lig_scalars 1 .. 255 (> 64: exact fp32 only), n_kp_scalars 1 .. 256 (the */
                                         /* trainer takes n_kp_scalars 1 .. 255)                                        */
    int32_t vector_size;               /* 1 .. 16 (kernels are 16 channels wide; fewer are zero padded)           */
    int32_t n_convs, n_hidden_scalars; /* n_hidden_scalars 1 .. 256 (kernels are 128 / 256 wide, likewise); the   */
                                       /* training engine kpd_gvp_trainer_* takes the same ranges (narrower models */
                                       /* through zero-padded wide parameter copies); 257 .. 1024 for inference on */
                                       /* the composed wide path (csrc/gvp_wide.hip: fp32 only; debug taps convs=, */
                                       /* gemm=f32, ws_bytes only; no kpd_gvp_profile); > 1024 is refused          */
    int32_t update_kp;
    int32_t message_norm_mode;         /* 0: constant message_norm, 1: 'mean', 2: message_norm == 0
                                          (per-graph average in-degree + 1, gvp.py:504-507)  */
    float message_norm;
    int32_t ll_k, kl_k;                /* ll_k must be 0; kl_k in 1..16                    */
    float ll_cutoff, kl_cutoff;
    int32_t n_message_gvps, n_update_gvps, n_noise_gvps;   /* each in 1..4                 */
} kpd_gvp_config;

typedef struct kpd_gvp kpd_gvp;

kpd_status kpd_gvp_create(const kpd_gvp_config *cfg, kpd_gvp **out);
void kpd_gvp_destroy(kpd_gvp *m);
/* Reference state-dict names of the `dynamics` module, e.g.
 * "noise_predictor.conv_layers.2.edge_message_fns.kp_kl_lig.0.to_feats_out.0.weight". */
kpd_status kpd_gvp_load_weight(kpd_gvp *m, const char *name, const float *w_dev,
                               const int64_t *shape, int32_t ndim, void *stream);
kpd_status kpd_gvp_commit(kpd_gvp *m);
kpd_status kpd_gvp_reserve(kpd_gvp *m, int32_t max_B, int32_t max_n_lig, int32_t max_n_kp,
                           int32_t max_n_kk, int32_t max_lig_per_graph, int32_t max_kp_per_graph);
kpd_status kpd_gvp_forward(kpd_gvp *m, const kpd_batch *batch, const float *t_dev,
                           float *eps_h_dev, float *eps_x_dev, void *stream);
/* Debug/test taps: "convs=<n>" limits the conv stack; "s_lig", "s_kp", "v_lig", "v_kp" copy state; "gemm=f32" | "gemm=f16x2" as for
 * kpd_egnn_debug_state (the 256 x 256 products of the message / update chains; KPD_GEMM=f16x2 at create time; 256 scalars only). */
kpd_status kpd_gvp_debug_state(kpd_gvp *m, const char *what, float *out_dev, int64_t n_floats,
                               void *stream);
/* HIP-event timing of the dominant kernel (k_gvp_chain: the message chain of GVPMultiEdgeConv.message,
 * models/gvp.py:459-497, 545-549) around each of its launches while enabled, and the launch geometry of the last
 * forward {E_ll, E_kl, E_lk, E_kk, tiles of a four-edge-type conv, tiles of the final conv, edges of the final conv}
 * (the final conv runs ll + kl only, models/dynamics_gvp.py:67-72), out[7] = the GEMM mode in effect (0 exact fp32, 1 f16x2). */
kpd_status kpd_gvp_profile(kpd_gvp *m, int32_t enable);
kpd_status kpd_gvp_profile_read(kpd_gvp *m, double *total_ms, int32_t *launches);
kpd_status kpd_gvp_last_counts(kpd_gvp *m, int32_t out[8], void *stream);

/* Training path of the GVP denoiser: same contract as kpd_egnn_trainer_* above for
 * LigRecDynamicsGVP.forward (models/dynamics_gvp.py:149-199).  Gradients flow to every parameter and to the scalar and
 * vector input features: d_lig_h [n_lig, n_lig_scalars], d_kp_h [n_kp, n_kp_scalars], d_kp_v [n_kp, vector_size, 3] (each may be
 * NULL); positions receive no gradient (they enter through the unit edge vector and the rbf code only and are data in
 * every training configuration served). */
typedef struct kpd_gvp_trainer kpd_gvp_trainer;
kpd_status kpd_gvp_trainer_create(const kpd_gvp_config *cfg, kpd_gvp_trainer **out);
void kpd_gvp_trainer_destroy(kpd_gvp_trainer *t);
kpd_status kpd_gvp_trainer_bind(kpd_gvp_trainer *t, const char *name, const float *weight_dev, float *grad_dev,
                                const int64_t *shape, int32_t ndim);
/* GVPDropout of training mode (gvp.py:119-149): rate in [0, 1) and the seed of this step's masks; call before forward
 * (0 = identity, the default).  Feature dropout is per element, vector dropout per channel, kept entries scale by
 * 1 / (1 - rate); the masks are Philox streams keyed by (seed; conv, node type, position, kind) and are regenerated in
 * backward.  kpd_dropout_mask writes one such stream ({0, 1 / (1 - rate)} per entry; node_type 0 = lig, 1 = kp;
 * position 0 = aggregated messages, 1 = update residual; kind 0 = scalars [n, S] row-major, 1 = vector channels
 * [n, 16]) so that tests can replay a step on the oracle. */
kpd_status kpd_gvp_trainer_set_dropout(kpd_gvp_trainer *t, float rate, uint64_t seed);
kpd_status kpd_dropout_mask(uint64_t seed, int32_t conv, int32_t node_type, int32_t position, int32_t kind, int64_t n,
                            float rate, float *out_dev, void *stream);
kpd_status kpd_gvp_trainer_reserve(kpd_gvp_trainer *t, int32_t max_B, int32_t max_n_lig, int32_t max_n_kp,
                                   int32_t max_n_kk, int32_t max_lig_per_graph, int32_t max_kp_per_graph);
kpd_status kpd_gvp_trainer_forward(kpd_gvp_trainer *t, const kpd_batch *batch, const float *t_dev, float *eps_h_dev,
                                   float *eps_x_dev, void *stream);
/* d_lig_x [n_lig, 3] / d_kp_x [n_kp, 3] (either may be null): gradients with respect to the positions, which enter through the
 * unit edge vector and the rbf code of every edge (models/gvp.py:472-480); the edge lists themselves are not differentiable. */
/* E_ll, E_kl, E_lk, E_kk of the last forward (host values the forward already read back: no synchronisation).  No reference counterpart
 * (bench.py's FLOP count of the training lines). */
kpd_status kpd_gvp_trainer_last_counts(kpd_gvp_trainer *t, int32_t out[4]);
/* Which form the edge messages of the convs run in with the current reservation: 1 = the register-chained kernels (one forward, one
 * backward and two batched weight-gradient launches per conv: n_hidden_scalars = 256 and the kept-activation memory was granted),
 * 0 = one GVP at a time through the GEMM kernels (any width; recomputation when memory is short).  Same gradients to rounding.  No
 * reference counterpart (tests assert that the path they mean to cover is the one that ran). */
kpd_status kpd_gvp_trainer_message_path(kpd_gvp_trainer *t, int32_t *path);
kpd_status kpd_gvp_trainer_backward(kpd_gvp_trainer *t, const float *d_eps_h, const float *d_eps_x, float *d_lig_h,
                                    float *d_kp_h, float *d_kp_v, float *d_lig_x, float *d_kp_x, void *stream);

/* ---------------------------------------------------------------------------------------
 * GVP keypoint receptor encoder (once per pocket).  Replaces ReceptorEncoderGVP.forward
 * (models/receptor_encoder_gvp.py:212-294): scalar embedding, rec-rec GVPEdgeConv stack
 * (models/gvp.py:170-341), KeypointInitializer (:15-93), kNN rec->kp edges (update_rk_edges
 * :297-321), rec-kp GVPEdgeConv stack, keypoint radius graph.  Fields mirror
 * ReceptorEncoderGVP.__init__ (:99-114) + graph_cutoffs.
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_recenc_config {
    int32_t in_scalar_size, out_scalar_size;   /* each 1 .. 256 (kernels are 128 / 256 wide; narrower models run zero
                                                  padded, the LayerNorms and the attention scale take the true width) */
    int32_t vector_size;                       /* 1 .. 16 (16-channel kernels, fewer are zero padded); kp_v of kpd_rec_out is [n_kp][vector_size][3] */
    int32_t n_rr_convs, n_rk_convs, n_message_gvps, n_update_gvps;
    int32_t message_norm_mode;                 /* 0 constant, 1 'mean', 2 message_norm == 0 */
    float message_norm;
    int32_t k_closest;                         /* kNN rec->kp, 1..16, or 0 with kp_rad > 0 */
    int32_t n_keypoints;
    float rr_cutoff, rk_cutoff, kk_cutoff;     /* graph_cutoffs['rr'|'rk'|'kk'] (rbf D_max, kk radius) */
    float kp_rad;                              /* > 0 (with k_closest == 0): radius rec->kp graph, at most 10 receptor atoms per
                                                * keypoint in index order (receptor_encoder_gvp.py:304-306) */
} kpd_recenc_config;

typedef struct kpd_rec_batch {
    int32_t B, n_rec, max_rec;
    const int32_t *rec_ptr;     /* [dev] [B+1]                                             */
    const float *rec_x;         /* [dev] [n_rec,3]                                         */
    const float *rec_h;         /* [dev] [n_rec,in_scalar_size]                            */
    int32_t n_rr;
    const int32_t *rr_src;      /* [dev] [n_rr] sorted by (dst, src)                       */
    const int32_t *rr_dst;
    const int32_t *rr_rowptr;   /* [dev] [n_rec+1]                                         */
} kpd_rec_batch;

typedef struct kpd_rec_out {
    float *kp_x;                /* [dev] [B*K,3]    keypoint positions                     */
    float *kp_h;                /* [dev] [B*K,out_scalar_size] keypoint scalars            */
    float *kp_v;                /* [dev] [B*K][vector_size][3] keypoint vectors            */
    int32_t *rk_src, *rk_dst;   /* [dev] [B*K*k_closest] rec->kp edges, kp-major           */
    int32_t cap_kk;             /* capacity of kk_src / kk_dst (>= B*K*min(K-1,100))       */
    int32_t *kk_src, *kk_dst;   /* [dev] kp-kp radius graph, dst-sorted                    */
    int32_t *kk_per_graph;      /* [dev] [B]                                               */
    int32_t *counts;            /* [dev] [2]: {E_kk, E_rk}                                 */
} kpd_rec_out;

typedef struct kpd_recenc kpd_recenc;

kpd_status kpd_recenc_create(const kpd_recenc_config *cfg, kpd_recenc **out);
void kpd_recenc_destroy(kpd_recenc *m);
/* Reference state-dict names of the `rec_encoder` module, e.g.
 * "rk_conv_layers.1.edge_message.0.to_feats_out.0.weight". */
kpd_status kpd_recenc_load_weight(kpd_recenc *m, const char *name, const float *w_dev,
                                  const int64_t *shape, int32_t ndim, void *stream);
kpd_status kpd_recenc_commit(kpd_recenc *m);
kpd_status kpd_recenc_reserve(kpd_recenc *m, int32_t max_B, int32_t max_n_rec, int32_t max_n_rr,
                              int32_t max_rec_per_graph);
kpd_status kpd_recenc_forward(kpd_recenc *m, const kpd_rec_batch *batch, const kpd_rec_out *out,
                              void *stream);

/* Training engine of the same encoder (SURVEY.md 8(f) item 2 for row a8): forward with saved node states, backward with
 * respect to every parameter given the gradients of the three outputs (keypoint positions, scalars, vectors -- what the GVP
 * denoiser's backward pass and the optimal-transport encoder loss, losses/rec_encoder_loss.py:49-82, hand back).  Parameters are
 * bound by reference state-dict name to live storage (read in place, gradients accumulated in place: bind zero-filled buffers);
 * dropout as in kpd_gvp_trainer_set_dropout (GVPDropout on the aggregated messages and on the update residual of every
 * GVPEdgeConv, models/gvp.py:316, 327).  Forward fills the same kpd_rec_out as kpd_recenc_forward; any of the three gradient
 * pointers of backward may be null (= zero). */
typedef struct kpd_recenc_trainer kpd_recenc_trainer;
kpd_status kpd_recenc_trainer_create(const kpd_recenc_config *cfg, kpd_recenc_trainer **out);
void kpd_recenc_trainer_destroy(kpd_recenc_trainer *t);
kpd_status kpd_recenc_trainer_bind(kpd_recenc_trainer *t, const char *name, const float *weight_dev, float *grad_dev,
                                   const int64_t *shape, int32_t ndim);
kpd_status kpd_recenc_trainer_set_dropout(kpd_recenc_trainer *t, float rate, uint64_t seed);
kpd_status kpd_recenc_trainer_reserve(kpd_recenc_trainer *t, int32_t max_B, int32_t max_n_rec, int32_t max_n_rr,
                                      int32_t max_rec_per_graph);
kpd_status kpd_recenc_trainer_forward(kpd_recenc_trainer *t, const kpd_rec_batch *batch, const kpd_rec_out *out, void *stream);
kpd_status kpd_recenc_trainer_backward(kpd_recenc_trainer *t, const float *d_kp_x, const float *d_kp_h, const float *d_kp_v,
                                       void *stream);

/* ---------------------------------------------------------------------------------------
 * EGNN keypoint receptor encoder (once per pocket; the encoder of the egnn_20kp / egnn_40kp models).  Replaces
 * ReceptorEncoder.forward (models/receptor_encoder.py:483-555): the ReceptorConv stack on the rr graph (:14-154),
 * keypoint_embedding of the mean receptor feature (:526-530), RecKeyConv (:182-297, k_closest features) and the
 * keypoint radius graph (:541).  Fields mirror ReceptorEncoder.__init__ (:383-400) + graph_cutoffs['kk'].
 * Batch and outputs reuse kpd_rec_batch / kpd_rec_out (rec_h width = in_n_node_feat, kp_h width =
 * out_n_node_feat, kp_v unused); rr_same_res [n_rr] is the rr `same_res` column as floats, in the order of the
 * sorted rr edges (null without use_sameres_feat); rec_h_out [n_rec,out] / rec_x_out [n_rec,3] (optional) receive
 * the learned receptor features / positions the reference stores as rec 'h' / 'x' (:516-517).
 * ------------------------------------------------------------------------------------- */
typedef struct kpd_recegnn_config {
    int32_t n_convs, n_keypoints;
    int32_t in_n_node_feat, hidden_n_node_feat, out_n_node_feat;   /* each in 1..256                        */
    int32_t use_sameres_feat, use_tanh, norm, fix_pos;
    float coords_range;
    float message_norm;          /* 0: z = rr edges / receptor nodes per graph (no +1, :505-509)          */
    int32_t k_closest;           /* kNN rec->kp features, 1..16, or 0 with kp_rad > 0                     */
    float kk_cutoff;             /* graph_cutoffs['kk']                                                   */
    float kp_rad;                /* > 0 (with k_closest == 0): keypoint features = sum of the receptor features within kp_rad (at most
                                  * 100 atoms, index order) / (rk edges per keypoint of the complex + 1) (receptor_encoder.py:238-262) */
} kpd_recegnn_config;

typedef struct kpd_recegnn kpd_recegnn;

kpd_status kpd_recegnn_create(const kpd_recegnn_config *cfg, kpd_recegnn **out);
void kpd_recegnn_destroy(kpd_recegnn *m);
/* Reference state-dict names of the `rec_encoder` module, e.g. "rec_convs.2.edge_mlp.0.weight",
 * "rec_kp_conv.kp_feature_mlp.0.bias" ("rec_kp_conv.fc_dst.weight" is accepted and ignored, as upstream never applies it). */
kpd_status kpd_recegnn_load_weight(kpd_recegnn *m, const char *name, const float *w_dev,
                                   const int64_t *shape, int32_t ndim, void *stream);
kpd_status kpd_recegnn_commit(kpd_recegnn *m);
kpd_status kpd_recegnn_reserve(kpd_recegnn *m, int32_t max_B, int32_t max_n_rec, int32_t max_n_rr,
                               int32_t max_rec_per_graph);
kpd_status kpd_recegnn_forward(kpd_recegnn *m, const kpd_rec_batch *batch, const float *rr_same_res,
                               const kpd_rec_out *out, float *rec_h_out, float *rec_x_out, void *stream);

/* Training engine of the same encoder (SURVEY.md 8(f) item 2 for row f1): forward with saved layer states, backward with respect
 * to every parameter given the gradients of the keypoint positions and keypoint features (either may be null = zero).  The
 * k_closest keypoint features only (every shipped config; create refuses kp_rad > 0).  Parameters are bound as in
 * kpd_recenc_trainer_bind.  Forward fills the same outputs as kpd_recegnn_forward. */
typedef struct kpd_recegnn_trainer kpd_recegnn_trainer;
kpd_status kpd_recegnn_trainer_create(const kpd_recegnn_config *cfg, kpd_recegnn_trainer **out);
void kpd_recegnn_trainer_destroy(kpd_recegnn_trainer *t);
kpd_status kpd_recegnn_trainer_bind(kpd_recegnn_trainer *t, const char *name, const float *weight_dev, float *grad_dev,
                                    const int64_t *shape, int32_t ndim);
kpd_status kpd_recegnn_trainer_reserve(kpd_recegnn_trainer *t, int32_t max_B, int32_t max_n_rec, int32_t max_n_rr,
                                       int32_t max_rec_per_graph);
kpd_status kpd_recegnn_trainer_forward(kpd_recegnn_trainer *t, const kpd_rec_batch *batch, const float *rr_same_res,
                                       const kpd_rec_out *out, float *rec_h_out, float *rec_x_out, void *stream);
kpd_status kpd_recegnn_trainer_backward(kpd_recegnn_trainer *t, const float *d_kp_x, const float *d_kp_h, void *stream);

/* ---------------------------------------------------------------------------------------
 * Exact optimal-transport plans between small uniform point clouds, on the HOST (no device work): what the reference gets from
 * POT's `ot.emd` in losses/rec_encoder_loss.py:11-18 (keypoints vs receptor atoms / interface points, once per complex and
 * training batch).  n_problems independent problems; problem p: cost matrix at cost + offsets[p] (row-major [n[p], m[p]],
 * doubles), masses 1 / n[p] and 1 / m[p]; the optimal plan is written to plan + offsets[p].  Up to n_threads host threads.
 * ------------------------------------------------------------------------------------- */
kpd_status kpd_ot_emd_uniform(int32_t n_problems, const int32_t *n, const int32_t *m, const int64_t *offsets,
                              const double *cost_host, double *plan_host, int32_t n_threads);

/* ---------------------------------------------------------------------------------------
 * The fp32 GEMM the training engines run their dense products on (csrc/sgemm.hip, v_mfma_f32_32x32x2_f32; no vendor BLAS in the
 * library): row-major C[M,N] = alpha op(A) op(B) + beta C on device pointers, any sizes, leading dimensions and alignments.  What the
 * reference gets from torch.nn.Linear / autograd inside models/dynamics.py:37-79, models/gvp.py:166-222 during train.py; exported so
 * that its parity against a plain fp32 product can be tested on its own.  `workspace` (device floats, may be NULL): scratch for the
 * partial products of a K-dominated shape (a weight gradient, K = edge count), which is then cut along K over the grid and summed in a
 * fixed order -- never with atomics.  `colsum` (may be NULL; A^T B products only): colsum[m] += sum_k A[k][m] in the same pass over A
 * -- the bias gradient of the Linear whose weight gradient the product is.
 * ------------------------------------------------------------------------------------- */
kpd_status kpd_sgemm(int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K, float alpha, const float *A, int32_t lda,
                     const float *B, int32_t ldb, float beta, float *C, int32_t ldc, float *colsum, float *workspace,
                     int64_t workspace_floats, void *stream);

/* The batched weight gradients of the training engines (csrc/sgemm.hip: k_wgrad_tnx, k_sgemm_tn256_batch), exported like kpd_sgemm so that
 * their parity against plain fp32 products can be tested on their own.  Up to eight products of one kind per call, every output ACCUMULATED
 * (+=), split along K over the CUs in proportion to the products' K and summed in a fixed order (no atomics).  A, B: [K, >= 256] device
 * arrays with 16-byte aligned rows (lda, ldb multiples of 4).
 *   kind 0 (GVP message / update chains: autograd of models/gvp.py:100-111 with respect to to_feats_out and scalar_to_vector_gates):
 *       C [256, 256] += A^T B;  Cx1 [256, nb2] += A^T B2 (nb2 <= 31);  colsum [256] += column sums of A;
 *       Cx2 [na2, 256] += A2^T B (na2 <= 32);  colsum2 [na2] += column sums of A2;
 *       C == NULL for all products of the call: no 256 x 256 block, and Cx3 [256, nb3] += A^T B3 (nb3 <= 32) as a second narrow block.
 *       Unused narrow operands: widths 0 and NULL pointers.
 *   kind 1 (EGNN second Linears, models/dynamics.py:37-79): C [257, 257] += A[:, :257]^T B[:, :257], colsum [257] += column sums of A (or
 *       NULL); the narrow fields are ignored. */
typedef struct {
    const float *A, *B;
    int32_t lda, ldb, K;
    float *C;
    int32_t ldc;
    const float *B2;
    int32_t ldb2, nb2;
    float *Cx1;
    int32_t ldx1;
    float *colsum;
    const float *A2;
    int32_t lda2, na2;
    float *Cx2;
    int32_t ldx2;
    float *colsum2;
    const float *B3;
    int32_t ldb3, nb3;
    float *Cx3;
    int32_t ldx3;
} kpd_wgrad_item;
kpd_status kpd_wgrad_batch(int32_t kind, int32_t n, const kpd_wgrad_item *items, float *workspace, int64_t workspace_floats, void *stream);

/* ---------------------------------------------------------------------------------------
 * The optimizer step of the training loop.  Replaces torch.nn.utils.clip_grad_value_(model.parameters(), clip_value) +
 * torch.optim.Adam(...).step() of train.py:430-433, 541-543 (torch/optim/adam.py, default flags: no amsgrad, no maximize) for every
 * parameter tensor in ONE launch; same arithmetic element for element (csrc/optim.hip).  `params_dev`: DEVICE array of n_params entries
 * -- device pointers to a parameter, its gradient, exp_avg, exp_avg_sq (fp32, contiguous) and the element count -- that the caller
 * keeps current (gradient tensors may move from step to step); max_numel = the largest count.  mode 0: Adam step number `step` (>= 1),
 * with the gradients clamped to +- clip_value first when clip_value > 0 (written back, as clip_grad_value_ does); mode 1: the clamp
 * alone.  No host synchronisation.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    float *p;
    const float *g;
    float *m, *v;
    int64_t n;
} kpd_adam_param;
kpd_status kpd_adam_step(const kpd_adam_param *params_dev, int32_t n_params, int64_t max_numel, int32_t mode, double lr, double beta1, double beta2,
                         double eps, double weight_decay, int64_t step, double clip_value, void *stream);

/* ---------------------------------------------------------------------------------------
 * Receptor-ligand distance hinge of the training loss.  Replaces the per-complex loop of KeypointDiffusion.forward
 * (models/ligand_diffuser.py:149-154: dgl.unbatch, then DistanceHingeLoss = torch.cdist + max(thr - d, 0) + sum per complex,
 * losses/dist_hinge_loss.py) with one segmented launch (csrc/dist_hinge.hip).
 *   a [n_a,3], a_ptr [S+1]; b [n_b,3], b_ptr [S+1] (all device; segment s = rows [ptr[s], ptr[s+1]) of each side);
 *   b_ptr == NULL: self mode (B = A, pairs i < j, upstream's DistanceHingeLoss(pos_a) without pos_b; b and grad_b must be NULL).
 *   Pointers of empty arrays may be NULL (a side with no rows, seg_loss when S == 0).
 *   Out (device): seg_loss [S] = sum over the segment's pairs of max(threshold - ||a_i - b_j||, 0), total [1] = their sum;
 *   grad_a [n_a,3] / grad_b [n_b,3] (optional, NULL = not computed) = d total / d a, d total / d b, with torch's subgradients
 *   (weight 1/2 at d == threshold, 0 at d == 0).  Rows outside every segment are not written.  Fixed-order reductions, no atomics:
 *   a segment's loss and gradient rows are bitwise independent of the other segments.  No host synchronisation.
 * ------------------------------------------------------------------------------------- */
kpd_status kpd_dist_hinge(const float *a, const int32_t *a_ptr, int32_t n_a, const float *b, const int32_t *b_ptr, int32_t n_b, int32_t S,
                          float threshold, float *seg_loss, float *total, float *grad_a, float *grad_b, void *stream);

/* ---------------------------------------------------------------------------------------
 * Reverse-diffusion update around the denoiser.  Replaces the elementwise part of
 * KeypointDiffusion.sample_p_zs_given_zt (models/ligand_diffuser.py:515-536):
 *   z_s = z_t / alpha_ts - var_terms * eps + sigma * noise, then ligand-COM removal from
 *   ligand and keypoints (remove_com :185-203).  coef [B,3] = {1/alpha_ts, var_terms, sigma}.
 * Updates lig_x, lig_h, kp_x in place.
 * ------------------------------------------------------------------------------------- */
kpd_status kpd_sample_update(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr,
                             int32_t atom_nf, float *lig_x, float *lig_h, float *kp_x,
                             const float *eps_x, const float *eps_h,
                             const float *noise_x, const float *noise_h,
                             const float *coef, int32_t max_lig, void *stream);

/* Coefficients of that update for every complex of the batch, from the noise-schedule table.
 * Replaces PredefinedNoiseSchedule.forward (models/ligand_diffuser.py:654-690) and the gamma / sigma / alpha
 * arithmetic of sample_p_zs_given_zt (:505-526, sigma_and_alpha_t_given_s :552-566):
 *   gamma [n_gamma] device table (n_gamma = timesteps + 1), s, t [B] device, coef [B,3] device out =
 *   {alpha_t|s, sigma^2_t|s / alpha_t|s / sigma_t, sigma_t|s sigma_s / sigma_t}. */
kpd_status kpd_step_coefficients(const float *gamma, int32_t n_gamma, const float *s, const float *t,
                                 int32_t B, float *coef, void *stream);

/* ---------------------------------------------------------------------------------------
 * Inpainting: the reverse step around fixed atoms (RePaint-style replacement conditioning; no upstream counterpart, this
 * comment is the specification).  Some ligand atoms are given (a scaffold, a hinge binder, a warhead); they are held at
 * their known positions and features while the other atoms are generated around them.
 *
 * The sampler's state lives in a ligand-COM-free frame, and the keypoints translate rigidly with it.  The input (receptor)
 * frame is therefore recovered at every step from the keypoints alone: with kp_com0 [B,3] = per-complex mean of the keypoint
 * positions in the input frame and m_b = the mean of complex b's rows of kp_x on entry to the step (lane-strided partial sums
 * and a butterfly over one wavefront: a fixed order that depends on nothing but that complex), a position X given in the input
 * frame sits at k0 = (X - kp_com0_b) + m_b in the state frame -- evaluated in that order, the first difference removes the
 * large input-frame magnitudes.  Nothing is accumulated from step to step, so the frame cannot drift and a captured step replays.
 *
 * One step t -> s for complex b (coef6 [B,6] = {alpha_t|s, var, sigma_step, alpha_s, sigma_s, sigma_t|s}):
 *   1. candidate for every atom, the arithmetic of kpd_sample_update:  u = z_t / alpha_t|s - var eps + sigma_step n   (x and h)
 *   2. frame: m_b, k0 as above
 *   3. noised known part:  k = alpha_s k0 + sigma_s n',  kh = alpha_s Hn + sigma_s n'_h   (n', n'_h: a second pair of draws)
 *   4. merge:  z_s = fixed ? (k, kh) : u
 *   5. COM removal: the mean of the merged ligand positions (staged in LDS, summed in a fixed order) is subtracted from the
 *      ligand and from the keypoints, as kpd_sample_update does.
 * kpd_sample_update, kpd_sample_update_inpaint and kpd_sample_renoise are instances of one device function, so a complex with
 * no fixed atom leaves kpd_sample_update_inpaint with exactly the bits kpd_sample_update gives, and a complex's result is
 * bitwise independent of the other complexes in the batch.
 *   fixed [n_lig] bytes (1 = given); known_x [n_lig,3] input frame, known_h [n_lig,atom_nf] already divided by the feature
 *   normalisation constant, known_noise_x / known_noise_h like noise_x / noise_h: all four are read on fixed rows only.
 * One workgroup per complex, max_lig <= 4096 (positions staged in LDS), larger ligands and keypoint sets than the workgroup
 * are strided over; no atomics, no host synchronisation, counts come from device memory (capturable).
 *
 * kpd_sample_renoise moves the state back from s to t between two repetitions of a resampled step:
 *   z_t = alpha_t|s z_s + sigma_t|s n'' for x and h, then the same COM removal (reads columns 0 and 5 of coef6).
 * kpd_inpaint_coefficients fills coef6; its first three columns are the bits of kpd_step_coefficients.
 * ------------------------------------------------------------------------------------- */
kpd_status kpd_inpaint_coefficients(const float *gamma, int32_t n_gamma, const float *s, const float *t,
                                    int32_t B, float *coef6, void *stream);
kpd_status kpd_sample_update_inpaint(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr,
                                     int32_t atom_nf, float *lig_x, float *lig_h, float *kp_x,
                                     const float *eps_x, const float *eps_h,
                                     const float *noise_x, const float *noise_h, const float *coef6,
                                     const uint8_t *fixed, const float *known_x, const float *known_h,
                                     const float *kp_com0, const float *known_noise_x, const float *known_noise_h,
                                     int32_t max_lig, void *stream);
kpd_status kpd_sample_renoise(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr, int32_t atom_nf,
                              float *lig_x, float *lig_h, float *kp_x, const float *noise_x, const float *noise_h,
                              const float *coef6, int32_t max_lig, void *stream);

/* ---------------------------------------------------------------------------------------
 * Clash guidance: the reverse step that keeps the ligand out of a set of atoms (no upstream counterpart, this comment is the
 * specification).  Upstream knows steric clashes only as a training loss (rl_dist_threshold, models/ligand_diffuser.py:137-156,
 * here kpd_dist_hinge); this imposes the same constraint at sampling time, on the same quantity -- the denoised estimate x-hat --
 * without retraining and without a gradient through the denoiser.
 *
 * Inputs per batch beyond those of kpd_sample_update: wall_x [n_wall,3], the atoms to stay away from, in the input (receptor)
 * frame; wall_ptr [B+1] int32 offsets, complex b owns rows [wall_ptr[b], wall_ptr[b+1]) and may own none; kp_com0 [B,3], the
 * keypoint mean in the input frame (as in inpainting); threshold > 0 in Angstrom; coef9 [B,9] from kpd_guided_coefficients:
 *   columns 0-5 = the bits of kpd_inpaint_coefficients (so 0-2 = the bits of kpd_step_coefficients),
 *   6 = alpha_t = sqrt(sigmoid(-gamma_t)),  7 = sigma_t = sqrt(sigmoid(gamma_t)),
 *   8 = w = scale alpha_s sigma^2_t|s / sigma_t^2  when round(t T) <= round(t_max T), else 0.
 * alpha_s sigma^2_t|s / sigma_t^2 is the weight of x_0 in the mean of q(z_s | z_t, x_0); upstream's mu is that mean evaluated at
 * x-hat, so moving x-hat by D moves mu by exactly this weight times D.  It lies in [0.19, 0.9995] for T = 10 and in
 * [3.9e-4, 0.36] for T = 1000 (polynomial_2, precision 1e-4 and 1e-5): nothing blows up at t ~ 1, where 1 / alpha_t ~ 300.
 *
 * One step t -> s for complex b:
 *   1. candidate for every atom, the arithmetic of kpd_sample_update:  u = z_t / alpha_t|s - var eps + sigma_step n   (x and h)
 *   2. denoised positions:  xh_i = (z_t,i - sigma_t eps_x,i) / alpha_t          (denoised_representation, :221-230)
 *   3. frame, as in inpainting: m_b = ordered mean of this complex's kp_x rows on entry; a wall atom r sits at
 *      r' = (r - kp_com0_b) + m_b, evaluated in that order
 *   4. force:  F_i = sum_r max(threshold - d, 0) (xh_i - r') / d,  d = |xh_i - r'|, over the wall atoms of complex b.  A pair with
 *      d < 1e-6 has no direction and adds nothing.  F_i is minus the gradient of the squared hinge 1/2 sum (threshold - d)+^2; the
 *      square is deliberate: the gradient of upstream's linear hinge jumps by a unit vector at d = threshold, where a last-bit
 *      difference would flip a whole contact.  With scale = 1 an atom with one contact has its x-hat moved onto the threshold sphere.
 *   5. shift:  u_x,i += w F_i.  Features are not guided.
 *   6. inpainting merge, if a mask is given: fixed rows are replaced as kpd_sample_update_inpaint does.  Fixed atoms are not
 *      pushed and are not part of the wall.
 *   7. COM removal, as in every other instance.
 * The guided step is a fourth instance of the device function behind kpd_sample_update, kpd_sample_update_inpaint and
 * kpd_sample_renoise, whose bits it does not change.  A neutral complex -- no wall atoms, or w = 0, or no pair under the threshold --
 * leaves with exactly the bits of kpd_sample_update (with a mask: of kpd_sample_update_inpaint).  An atom's force is summed by one
 * wavefront, lanes striding the wall atoms, then a butterfly: a fixed order that depends only on its complex, so a complex's result
 * is bitwise independent of the batch and of the repeat.  No atomics, no host synchronisation, counts come from device memory
 * (capturable); one workgroup per complex; max_lig <= 4096 (x-hat is staged in LDS beside the new positions, 96 KB at most); wall
 * atoms are read from global memory, any number per complex.  wall_ptr must be ascending within [0, n_wall]: the kernel reads
 * what it says.  fixed, known_x, known_h, known_noise_x, known_noise_h: all NULL (no mask) or all given.
 *
 * kpd_clash_score is the report to rank or filter finished samples by: out [B,3] = per complex {1/2 sum (threshold - d)+^2, the
 * number of pairs with d < threshold (exact up to 2^24), the smallest such d or +inf}, ligand and wall in one frame, through the
 * same pair loop (coincident pairs count here), summed in a fixed order.
 * ------------------------------------------------------------------------------------- */
kpd_status kpd_guided_coefficients(const float *gamma, int32_t n_gamma, const float *s, const float *t,
                                   int32_t B, float scale, float t_max, float *coef9, void *stream);
kpd_status kpd_sample_update_guided(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr,
                                    int32_t atom_nf, float *lig_x, float *lig_h, float *kp_x,
                                    const float *eps_x, const float *eps_h,
                                    const float *noise_x, const float *noise_h, const float *coef9,
                                    const uint8_t *fixed, const float *known_x, const float *known_h,
                                    const float *kp_com0, const float *known_noise_x, const float *known_noise_h,
                                    const int32_t *wall_ptr, const float *wall_x,
                                    float threshold, int32_t max_lig, void *stream);
kpd_status kpd_clash_score(int32_t B, const int32_t *lig_ptr, const float *lig_x, const int32_t *wall_ptr,
                           const float *wall_x, float threshold, float *out, void *stream);

/* Sharding-invariant N(0,1) noise for the ligand rows of a batch (opt-in replacement of the global torch.randn draws of
 * ligand_diffuser.py:367, 530-531): out [n_nodes, width] with rows of complex b =
 * [node_ptr[b], node_ptr[b+1]).  Philox4x32-10 keyed by (seed, complex_id[b]), counter (element, step, tag): the values do
 * not depend on batch composition or rank.  complex_id [B] device int64 (global index of the complex in the job). */
kpd_status kpd_complex_noise(int32_t B, const int32_t *node_ptr, int32_t width, const int64_t *complex_id,
                             uint64_t seed, int32_t step, int32_t tag, float *out, void *stream);

/* Input side: the receptor part of build_initial_complex_graph
 * (data_processing/pdbbind_processing.py:221-274) for a whole batch of pockets taken from the flat dataset arrays
 * (data_processing/crossdocked/dataset.py:62-76, 135-145): rr = torch_cluster.radius_graph(rec, r = cutoffs['rr'],
 * max_num_neighbors = 100) per pocket (:245) and same_res = res_idx[src] == res_idx[dst] per edge (:248).
 *   rec_x [n_rec,3], rec_ptr [B+1] (device; pocket b = rows [rec_ptr[b], rec_ptr[b+1]), at most max_rec <= 2048 each),
 *   res_idx [n_rec] or NULL.  Out: src/dst [cap] dst-major with src ascending (global row numbers), rowptr [n_rec+1],
 *   per_graph [B], same_res [cap] bytes or NULL, counts [2] = {n_edges, 0} (edges beyond cap are counted, not written);
 *   scratch: kpd_rec_graph_scratch_bytes(n_rec, B) device bytes.  The complete rec -> kp edge list (:251-253) is
 *   implicit (dst-major, every receptor atom of the pocket) and is never materialised by this library. */
int64_t kpd_rec_graph_scratch_bytes(int32_t n_rec, int32_t B);
kpd_status kpd_build_rec_graph(const float *rec_x, const int32_t *rec_ptr, int32_t B, int32_t n_rec, int32_t max_rec,
                               float r, int32_t max_nn, const int32_t *res_idx, int32_t cap, int32_t *src, int32_t *dst,
                               int32_t *rowptr, int32_t *per_graph, uint8_t *same_res, int32_t *counts, void *scratch,
                               void *stream);

/* Output side of sampling: element decode and XYZ text for a batch of sampled ligands.
 * Replaces the tensor -> text part of write_sampled_ligands (sample.py:66-90: torch.argmax over the feature columns,
 * dataset.lig_atom_idx_to_element) and write_xyz_file (utils.py:11-21: "<n>\n\n" + "<el> <x:.3f> <y:.3f> <z:.3f>\n"
 * per atom), as analysis/molecule_builder.py:47-48 calls it per ligand; bonds, fragments and SDF text: kpd_mol_perceive and
 * kpd_sdf_emit below.  The bytes equal Python's: "%.3f" of the exact fp32 value, round-half-even, '-0.000', 'nan', 'inf'.
 *   pos [n_atoms,3], feat [n_atoms,F], lig_ptr [B+1] (device); symbols [F] device, each element symbol as up to four
 *   NUL-padded bytes packed little-endian; elem [n_atoms] out (argmax, first maximum); text [capacity] out; text_ptr
 *   [B+1] int64 out (ligand b's block = text[text_ptr[b] : text_ptr[b+1]]; text_ptr[B] is the size needed, also when it
 *   exceeds capacity); status [1] out: bit 0 = a coordinate with |x| >= 2^53 was printed as '?', bit 1 = capacity too
 *   small (nothing written for the ligands that do not fit); scratch: kpd_xyz_scratch_bytes(n_atoms, B) device bytes. */
int64_t kpd_xyz_scratch_bytes(int32_t n_atoms, int32_t B);
kpd_status kpd_xyz_emit(const float *pos, const float *feat, const int32_t *lig_ptr, int32_t n_atoms, int32_t B,
                        int32_t F, const uint32_t *symbols, int32_t *elem, uint8_t *text, int64_t capacity,
                        int64_t *text_ptr, int32_t *status, void *scratch, void *stream);

/* Pocket extraction: the array-level part of dataset construction, for a batch of whole receptors + ligands
 * (csrc/pocket.hip).  Replaces get_pocket_atoms (data_processing/pdbbind_processing.py:85-149, called by
 * process_crossdocked.py:112-119) and the residue-wise selection of process_bindingmoad.py:124-161 / byop.py:119-157:
 * ligand bounding box + padding (:92-97, :114-117), atoms closer than pocket_cutoff to a ligand atom (:124-128), expansion to
 * whole residues (torch.isin, :131-134), compaction (:137-138).  The arrays come from files through kpd_pdb_parse / kpd_sdf_parse (end of this file).
 *   rec_x [n_rec,3], rec_ptr [B+1] (complex b = rows [rec_ptr[b], rec_ptr[b+1]), at most max_rec each), res_idx [n_rec]
 *   (per complex in [0, atoms of that complex), as prody's getResindices; need not be contiguous or sorted), probe [n_rec]
 *   bytes (atoms that count for the distance test), emit [n_rec] bytes (atoms that may appear in the pocket), lig_x [n_lig,3],
 *   lig_ptr [B+1] (at most 1024 ligand atoms per complex); box_padding < 0: no box; all device pointers.
 *   A residue is selected if one of its probe atoms lies inside the box and closer than pocket_cutoff to a ligand atom.
 *   Out (device): in_box [n_rec] bytes (geometric box test of every atom, upstream's >= lower, <= upper on fp32 corners),
 *   pocket_mask [n_rec] bytes (emit and residue selected: upstream's byres_pocket_atom_mask), rows [cap_rows] (selected atoms,
 *   global row numbers ascending), pocket_res [cap_rows] (rank of the atom's residue among the selected residues of its complex
 *   in order of first appearance), pocket_ptr [B+1] (pocket_ptr[B] is the size needed, also when it exceeds cap_rows; the rows of
 *   a complex that does not fit are not written), status [B]: bit 0 = no pocket atom, bit 1 = cap_rows too small for this
 *   complex, bit 2 = a res_idx outside its range (that atom is never selected), bit 3 = malformed segment, more than max_rec
 *   atoms or more than 1024 ligand atoms (complex left out).  Nothing is read or written out of bounds in any of these cases.
 *   scratch: kpd_pocket_scratch_bytes(n_rec, B) device bytes.  Four kernel launches (and five memsets) whatever B is; no host synchronisation.
 * Arithmetic: every threshold test compares the squared distance, computed in fp64 from direct differences of the fp32
 * coordinates (the differences are exact), with the squared threshold; a NaN coordinate is never selected.  Upstream's own
 * decisions (scipy float64 / torch.cdist's fp32 matmul form) agree with this wherever they are stable.
 * Deterministic and bitwise independent of batch composition (no float atomics; flags are same-value byte stores).
 * ------------------------------------------------------------------------------------- */
int64_t kpd_pocket_scratch_bytes(int32_t n_rec, int32_t B);
kpd_status kpd_pocket_select(const float *rec_x, const int32_t *rec_ptr, const int32_t *res_idx, const uint8_t *probe,
                             const uint8_t *emit, int32_t n_rec, int32_t max_rec, const float *lig_x, const int32_t *lig_ptr,
                             int32_t n_lig, int32_t B, float box_padding, float pocket_cutoff, int32_t cap_rows, uint8_t *in_box,
                             uint8_t *pocket_mask, int32_t *rows, int32_t *pocket_res, int32_t *pocket_ptr, int32_t *status,
                             void *scratch, void *stream);

/* Interface points, the targets of the optimal-transport encoder loss (losses/rec_encoder_loss.py:71-82).  Replaces
 * get_interface_points (data_processing/pdbbind_processing.py:295-325; called at :142-145 with the box atoms and at
 * process_bindingmoad.py:200 with the pocket atoms): midpoints (lig + rec) / 2 of all pairs closer than dist_thr in
 * torch.where order (ligand atom ascending, then receptor atom ascending, :306-308), thinned by the sequential greedy rule
 * (:312-321: the first candidate is kept, a later one if it is >= excl_thr from every point kept so far).
 *   rec_x, rec_ptr, lig_x, lig_ptr as above; cand_mask [n_rec] bytes = the candidate receptor set (in_box & probe for the
 *   CrossDocked form, pocket_mask for the BindingMOAD / byop form); cap_cand = candidate capacity per complex, cap_points =
 *   capacity of points (all complexes together).
 *   Out (device): points [cap_points,3], ip_ptr [B+1] (ip_ptr[B] is the size needed; the points of a complex that does not fit
 *   are not written), n_cand [B] (exact, also beyond cap_cand), status [B]: bit 0 = no candidate (upstream raises
 *   InterfacePointException), bit 1 = more candidates than cap_cand (the points are then those of the first cap_cand
 *   candidates, a prefix of the full answer), more than 4096 points in one complex, or cap_points too small for this complex,
 *   bit 3 = malformed segment or more than 1024 ligand atoms.  scratch: kpd_interface_points_scratch_bytes(n_rec, B, cap_cand).
 *   Three launches whatever B is; no host synchronisation.  Arithmetic and determinism as for kpd_pocket_select; midpoints are
 *   (a + b) * 0.5f in fp32, bitwise upstream's. */
int64_t kpd_interface_points_scratch_bytes(int32_t n_rec, int32_t B, int32_t cap_cand);
kpd_status kpd_interface_points(const float *rec_x, const int32_t *rec_ptr, const uint8_t *cand_mask, int32_t n_rec,
                                const float *lig_x, const int32_t *lig_ptr, int32_t n_lig, int32_t B, float dist_thr,
                                float excl_thr, int32_t cap_cand, int32_t cap_points, float *points, int32_t *ip_ptr,
                                int32_t *n_cand, int32_t *status, void *scratch, void *stream);

/* Molecules from sampled ligands (csrc/molecule.hip): atoms -> bond graph -> valences, fragments, validity counts, SDF text.
 * Replaces, for the array-level part, make_mol_openbabel (analysis/molecule_builder.py:38-60, a per-ligand XYZ string round trip
 * through openbabel), check_atom_valency and compute_avg_frag_size (analysis/metrics.py:156-206) and the SDF writing of
 * sample.py.  openbabel's rules cannot be restated here, so THIS COMMENT IS THE DEFINITION: the lookup-table builder of the
 * EDM / DiffSBDD lineage that upstream's molecule_builder.py was adapted from.  Connectivity comes from covalent radii, bond
 * orders from length classes, both under valence caps.  Sanitisation (rings, Kekule orders, hydrogen counts, validity) is
 * kpd_mol_sanitize below; RDKit's force fields stay with the caller;
 * what upstream compares SMILES for (uniqueness, novelty) is kpd_mol_keys below, and the relaxation of the samples inside their
 * pockets (by a force field of this library's own, not UFF) is kpd_relax at the end of this file.
 *
 * Ligands carry heavy atoms only; no hydrogens are added here (kpd_mol_sanitize counts them per atom, kpd_mol_add_hs places them).
 * Everything below is per ligand (at most 256 atoms).
 * Element table, by atomic number (radii after Pyykko & Atsumi 2009 in integer picometres, single / double / triple, 0 = no
 * bond of that order; cap = chemical valence cap):
 *     H  1:  32   0   0  1      B  5:  85  78   0  3      C  6:  75  67  60  4      N  7:  71  60  54  3      O  8:  63  57   0  2
 *     F  9:  64   0   0  1      Si 14: 116  0   0  4      P 15: 111 102   0  5      S 16: 103  94   0  6      Cl 17: 99   0   0  1
 *     As 33: 121  0   0  3      Br 35: 114  0   0  1      I 53: 133   0   0  1
 *   Any other atomic number is "unknown": such an atom is never bonded and sets status bit 2.
 * Arithmetic (as kpd_pocket_select): d2(i,j) = fp64 sum of squares of the differences of the fp32 coordinates (differences
 *   exact, each product and sum rounded once, (dx^2 + dy^2) + dz^2).  The test of order k with margin m is
 *   d2 <= (double)(T * T) * 1e-4 with the integer T = r_k(i) + r_k(j) + m (pm); false if either radius is 0.  A NaN or Inf
 *   coordinate makes every test false: such an atom is never bonded and sets status bit 2.
 * Steps:
 *   1. candidates: i < j bonded if d2 > 0.16 (0.4 A) and the order-1 test holds with m = 45;
 *   2. degree pruning: atoms i in ascending order; while degree(i) > cap(i), remove i's bond with the largest d2 (tie: the
 *      larger partner index).  A removal lowers the partner's degree too, which is why the order of the atoms matters;
 *   3. order by length: a surviving bond gets order 3 if the order-3 test holds with m = 3, else 2 if the order-2 test holds
 *      with m = 5, else 1;
 *   4. valence repair: atoms i in ascending order; while the sum of i's orders > cap(i), lower by one the order of i's bond
 *      with the highest order (among equals: the largest d2, then the larger partner index).  Terminates: degree <= cap;
 *   5. fragments: frag[a] = rank of a's connected component in order of first atom (0, 1, ...); the largest fragment has the
 *      most atoms, the lowest rank on a tie;
 *   6. validity (upstream's check_atom_valency): an atom is invalid if valence == 0, valence > allowed[class], or its element
 *      is unknown.  `allowed` comes from the caller (upstream's allowed_bonds maxima) and is deliberately another table than
 *      `cap`: a sulfone S (valence 6 > 4) counts as invalid, as it would upstream.
 * Limits: the orders are LENGTH CLASSES.  No aromaticity or Kekule perception in this call (an ideal benzene, 1.397 A, gets six
 *   single bonds; kpd_mol_sanitize writes Kekule orders next to them), no formal charges (nitro groups are demoted to single bonds).  Connectivity, fragments and the counts of step 5 do
 *   not depend on the orders.
 *
 * kpd_mol_perceive: pos [n_atoms,3], feat [n_atoms,F], lig_ptr [B+1], z [F] (atomic number of every feature class), allowed
 *   [F]; all device pointers.  Out (device): elem [n_atoms] (argmax of the feature row, first maximum, the routine of
 *   kpd_xyz_emit), valence [n_atoms], frag [n_atoms] (all three -1 for the atoms of a ligand that is left out), bond_ij
 *   [cap_bonds,2] (global row numbers, i < j; per ligand sorted by i, then j), bond_order [cap_bonds], bond_ptr [B+1]
 *   (bond_ptr[B] is the size needed, also when it exceeds cap_bonds; the bonds of a ligand that does not fit are not written;
 *   cap_bonds = 3 n_atoms always suffices, degree <= 6), summary [B,4] = {n_bonds, n_frags, largest_frag_atoms,
 *   n_invalid_atoms}, status [B]: bit 0 = empty ligand, bit 1 = cap_bonds too small for this ligand, bit 2 = a non-finite
 *   coordinate or an unknown element, bit 3 = malformed segment or more than 256 atoms (ligand left out: summary 0, no bonds;
 *   nothing is read or written out of bounds).  scratch: kpd_mol_scratch_bytes(n_atoms, B) device bytes.
 *   One wave per ligand; three launches (and three memsets) whatever B is; no host synchronisation, no float atomics;
 *   deterministic and bitwise independent of batch composition.
 *
 * kpd_sdf_emit: MOL V2000 blocks from those outputs.  symbols [F] as for kpd_xyz_emit (at most three bytes are printed).
 *   Block: an empty title line, "  kpd_hip " + 10 blanks + "3D", an empty comment line, the counts line
 *   "%3d%3d  0  0  0  0  0  0  0  0999 V2000", atom lines "%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0", bond
 *   lines "%3d%3d%3d  0" (1-based numbers local to the block), "M  END", "$$$$"; every line ends in '\n'.  Coordinates are
 *   Python's "%10.4f" of the exact fp32 value (round-half-even on the binary value, "-0.0000").  largest_only != 0: only the
 *   atoms and bonds of the largest fragment, renumbered in atom order (upstream's largest_frag).
 *   text [capacity], text_ptr [B+1] int64 as for kpd_xyz_emit (text_ptr[B] = size needed); status [B]: bit 0 = a non-finite
 *   coordinate, bit 1 = a coordinate whose text is wider than 10 characters, bit 2 = no molecule (mol_status bits 1 or 3, or
 *   inconsistent inputs), bit 3 = capacity too small for this ligand (nothing written for it).  With bits 0-2 the block is
 *   empty.  scratch: kpd_sdf_scratch_bytes(n_atoms, B).  Three launches whatever B is; no host synchronisation. */
int64_t kpd_mol_scratch_bytes(int32_t n_atoms, int32_t B);
kpd_status kpd_mol_perceive(const float *pos, const float *feat, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t F,
                            const int32_t *z, const int32_t *allowed, int32_t cap_bonds, int32_t *elem, int32_t *valence,
                            int32_t *frag, int32_t *bond_ij, int32_t *bond_order, int32_t *bond_ptr, int32_t *summary,
                            int32_t *status, void *scratch, void *stream);
int64_t kpd_sdf_scratch_bytes(int32_t n_atoms, int32_t B);
kpd_status kpd_sdf_emit(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F,
                        const uint32_t *symbols, const int32_t *frag, const int32_t *bond_ij, const int32_t *bond_order,
                        const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status, int32_t largest_only,
                        uint8_t *text, int64_t capacity, int64_t *text_ptr, int32_t *status, void *scratch, void *stream);

/* Properties of the SET of sampled ligands (csrc/molset.hip): uniqueness and novelty (analysis/metrics.py:135-147) and the
 * Tanimoto diversity of a pocket's samples (MoleculeProperties.calculate_diversity, analysis/metrics.py:263-277).  Upstream
 * compares canonical SMILES and RDKit path fingerprints, which cannot be restated here, so THIS COMMENT IS THE DEFINITION:
 * a key that is equal for isomorphic bond graphs, and a bit vector of the substructures around every atom, both read off the
 * bond graph kpd_mol_perceive left on the device.  All arithmetic is on unsigned 64-bit integers, modulo 2^64, except the
 * final Tanimoto ratio.
 *   mix(x):  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31  (splitmix64's finaliser)
 *   K1 = 0x9E3779B97F4A7C15, K2 = 0xC2B2AE3D27D4EB4F, K3 = 0x165667B19E3779F9.
 * Scope S of a ligand: with largest_only its largest fragment (frag of kpd_mol_perceive: most atoms, the lowest rank on a
 *   tie), else all of its atoms.  Only bonds with both ends in S count.  n, m = atoms and bonds in S; deg(a) = degree of a in
 *   S; d(a,b) = length in bonds of the shortest path inside S, 65535 if there is none; Z(a) = z[elem[a]], the atomic number
 *   of a's class (as a two's-complement integer); l = bond_order with with_orders, else 1.
 * Key:  inv_0[a] = mix(Z(a) + deg(a) K3 + K1 * sum over b in S, b != a, of mix(Z(b) K2 + d(a,b)));
 *       inv_r[a] = mix(K1 inv_{r-1}[a] + sum over the bonds (a,b) of mix(inv_{r-1}[b] + l K2)),   r = 1 .. n;
 *       key      = mix(n + m K3 + K1 * sum over a in S of mix(inv_n[a])).
 *   Every sum is commutative: neither the order of the atoms nor that of the bonds matters.  The distance term of inv_0 is
 *   what tells ring sizes apart (plain neighbourhood refinement gives decalin and bicyclopentyl one key).
 * Fingerprint: f_0[a] = mix(Z(a) + deg(a) K3), f_r from f_{r-1} by the step of inv_r; for r = 0 .. radius every atom a of S
 *   sets bit (f_r[a] mod nbits) of the ligand's row: bit k is bit (k & 31) of word (k >> 5).  The seeds are local on purpose:
 *   molecules that share a substructure share its bits.
 * Limits: a key describes the CONSTITUTION only: no stereo (enantiomers and E/Z isomers share a key), no hydrogens, no
 *   charges.  With with_orders it inherits the bond orders it is given: the length classes of kpd_mol_perceive know no
 *   aromaticity (two Kekule-like geometries of one ring can differ), order_k of kpd_mol_sanitize does; with_orders = 0 makes it
 *   independent of them.  It is a hash: equal keys of
 *   non-isomorphic graphs are possible in principle (none among the 1 136 pairs of equal size, composition and bond count,
 *   27 of them isomorphic, of the 700 seeded random molecule-like graphs of tests/test_molset_config.py: there key equality
 *   and labelled-graph isomorphism coincide).
 *
 * kpd_mol_keys: lig_ptr [B+1], elem / frag [n_atoms], bond_ij [cap_bonds,2], bond_order [cap_bonds], bond_ptr [B+1],
 *   mol_status [B] as kpd_mol_perceive wrote them, z [F]; radius 0 .. 4, nbits a power of two in 64 .. 4096.  Out (device):
 *   key [B] (the uint64 bit pattern), fp [B, nbits / 32], atom_inv [n_atoms] (inv_n of every atom of S, 0 elsewhere; may be
 *   NULL), status [B]: bit 0 = no molecule (mol_status bits 0, 1 or 3, an empty S, or inputs that are no output of
 *   kpd_mol_perceive: an element or fragment out of range, a bond outside the ligand, twice, of an order outside 1 .. 3, or a
 *   seventh neighbour); such a ligand gets key 0 and an all-zero row, and nothing is read or written out of bounds.
 *   One wave per ligand, one launch (and a memset for atom_inv) whatever B is; no scratch, no host synchronisation, no float
 *   arithmetic; a ligand's results are bitwise independent of the rest of the batch.
 *
 * kpd_fp_diversity: fp [B, W] (W >= 1 words per row), use [B] (0 = leave the ligand out), group_ptr [G+1]: group g is the
 *   ligands group_ptr[g] .. group_ptr[g+1] - 1 (a pocket's samples).  For every pair i < j of used ligands of a group:
 *   c = popcount(a & b), u = popcount(a | b), T = (double)c / (double)u, T = 1 if u == 0.  Out (device): div_sum [G] =
 *   sum of (1 - T) in fp64, n_pairs [G] int64, status [G]: bit 0 = malformed segment (not 0 <= group_ptr[g] <=
 *   group_ptr[g+1] <= B: div_sum 0, n_pairs 0, nothing read).  One workgroup per group, one launch; the partial sums of its
 *   256 threads meet in a fixed tree: no float atomics, deterministic, and bitwise the same whether a group is alone or in a
 *   batch.  The mean Tanimoto distance upstream reports is div_sum / n_pairs (0 for fewer than two ligands). */
kpd_status kpd_mol_keys(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                        const int32_t *frag, const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr,
                        int32_t cap_bonds, const int32_t *mol_status, int32_t largest_only, int32_t with_orders, int32_t radius,
                        int32_t nbits, int64_t *key, uint32_t *fp, int64_t *atom_inv, int32_t *status, void *stream);
kpd_status kpd_fp_diversity(const uint32_t *fp, const uint8_t *use, int32_t B, int32_t W, const int32_t *group_ptr, int32_t G,
                            double *div_sum, int64_t *n_pairs, int32_t *status, void *stream);

/* Sanitisation of the perceived molecules (csrc/sanitize.hip): ring bonds, planar rings, a Kekule assignment, aromatic rings,
 * implicit hydrogens, donor / acceptor flags, validity and the per-molecule descriptors.  Stands where upstream calls
 * Chem.SanitizeMol on every sample (`validity` of ModelAnalyzer.sample_and_analyze, analysis/metrics.py) and reads molecular
 * weight, donors, acceptors, rotatable bonds and the Lipinski count off the RDKit molecule (MoleculeProperties).  RDKit's rules
 * cannot be restated here, so THIS COMMENT IS THE DEFINITION; no agreement with RDKit or openbabel is claimed.  The inputs are
 * what kpd_mol_perceive left on the device and are never written; a second set of bond orders (order_k) is written next to the
 * length classes.  Scope S, Z(a), deg(a) and "both ends in S" are those of kpd_mol_keys; n, m = atoms and bonds in S.
 * Arithmetic: all geometry is fp64 on the differences of the fp32 coordinates; every product and sum is rounded once (no fused
 *   multiply-add); d2 and the length tests are those of kpd_mol_perceive.  A NaN or Inf coordinate makes every test it enters false.
 * Steps:
 *   1. ring bonds and rings: a bond is a ring bond iff its ends stay connected without it (the rule of N_rot below); ring atoms are
 *      their ends.  n_rings = m - n + (the number of distinct `frag` labels in S).  The simple cycles of 5 and of 6 atoms in S are
 *      listed, each once (from its smallest atom, the second atom smaller than the last; ordered by start atom, then
 *      lexicographically -- no output depends on that order).  More than 64 of them: status bit 1 (TOO_MANY_RINGS), steps 2 - 4 are
 *      skipped (order_k = bond_order, nothing planar or aromatic) and the ligand is not valid.
 *   2. planar rings: a cycle p_0 .. p_{k-1} is planar iff each of its k cyclic windows a, b, c, d of four consecutive atoms passes:
 *      u = b - a, v = c - b, w = d - c, n1 = u x v, n2 = v x w (a component is (x y) - (x' y')), dot products ((.) + (.)) + (.),
 *      q = |n1|^2 |n2|^2; pass iff q >= 1e-12 and n1.n2 >= 0.9396926207859084 * sqrt(q) (cos 20 deg).  Planar ring bonds and atoms
 *      are those of planar cycles.
 *   3. Kekule assignment on the candidate graph G.  Atoms of G: planar ring atoms with Z in {6, 7} and cap(Z) - (number of the
 *      atom's planar ring bonds) - (sum of bond_order over its other bonds) >= 1, cap from the table above.  Edges of G: planar
 *      ring bonds between two such atoms that pass the order-1 length test with margin -3 pm (C-C <= 1.47 A, C-N <= 1.43 A;
 *      this keeps the CH2 of cyclopentadiene out).  Per connected component of G with an edge: the matching M that maximises
 *      first the number of matched carbons, then the number of matched atoms, and among those has the lexicographically smallest
 *      ascending list of bond_ij row numbers.  This is an optimum: it does not depend on how it is found.  A component of more
 *      than 24 atoms sets status bit 2 (COMPONENT_TOO_LARGE): nothing in it is matched, every planar ring bond with an end in it
 *      keeps bond_order, and its carbons count as unsatisfied.  order_k = 2 on matched bonds, 1 on the other planar ring bonds,
 *      bond_order on every other bond.  A carbon of G with an edge that M leaves unmatched is UNSATISFIED ("cannot kekulise").
 *   4. aromatic rings: valence_k(a) = sum of order_k over a's bonds in S.  A planar cycle is aromatic iff every atom contributes
 *      and the contributions sum to 6: 1 for a matched atom; else 2 for O or S with deg 2; else 2 for an unmatched planar ring N
 *      with deg 2 or 3 and valence_k = deg (a "lone-pair N": pyrrole N-H, N-alkyl); else 0 for a C with a bond of order_k 2, not a
 *      planar ring bond, to N, O or S; anything else does not contribute.  Aromatic atoms and bonds are those of aromatic cycles.
 *   5. hydrogens: h = max(0, normal(Z, valence_k) - valence_k); normal = 4 for C and Si, 3 for N, B and As, 2 for O, 1 for H and
 *      the halogens, for S the smallest of 2, 4, 6 that is >= valence_k (6 beyond), for P of 3, 5 (5 beyond), 0 otherwise.
 *      No hydrogen positions are produced here: kpd_mol_add_hs below turns the counts into atoms.
 *   6. flags: donor = N or O with h >= 1; acceptor = every O, and every N that is no donor, has deg <= 2 and is no lone-pair N;
 *      over-valent = valence_k > allowed[class] (the table of kpd_mol_perceive's step 6).
 *   7. valid iff there is a molecule, no atom of S is over-valent or unsatisfied and neither cap bit is set.  An isolated atom
 *      is valid (its valence 0 is atom_validity's business).
 *   8. descriptors over S: desc_i = {n_heavy (Z != 1), n_h (sum of h), hbd (donors), hba (acceptors), n_rot (the rotor rule of
 *      kpd_vina_score below on order_k: order_k 1, both ends of heavy degree >= 2, no ring bond), n_rings, n_arom_rings (aromatic
 *      cycles), n_arom_atoms, lipinski4, n_cycles (the cycles of step 1)}; mw = sum over the classes c in class order of
 *      (double)count_c * mass[c], then + (double)n_h * mass_h (each product and sum rounded once; the counts are integers);
 *      lipinski4 = how many of mw < 500, hbd <= 5, hba <= 10, n_rot <= 10 hold.  Upstream's fifth rule (Crippen logP <= 5) is
 *      deliberately NOT counted: logP, QED and SA need RDKit's parameter files and stay with the caller.
 * Limits: no formal charges (a nitro group stays demoted, its O read as hydroxyls; pyridinium or an N-oxide ends up over-valent or
 *   non-aromatic); no 7-membered aromatic rings; no tautomer canonicalisation (which N of an imidazole carries the H follows
 *   from the lexicographic choice, so per-atom h and the Kekule pattern may move under renumbering; the aromatic sets, valid and
 *   every descriptor do not); no stereo.
 *
 * kpd_mol_sanitize: pos [n_atoms,3], lig_ptr [B+1], elem / frag [n_atoms], bond_ij [cap_bonds,2], bond_order [cap_bonds], bond_ptr
 *   [B+1], mol_status [B] as kpd_mol_perceive wrote them, z / allowed [F], mass [F] fp64 and mass_h (the mass of every class and
 *   of hydrogen, from the caller); all device pointers.  Out (device): order_k [cap_bonds], bond_flags [cap_bonds] (bit 0 ring,
 *   1 planar ring, 2 aromatic), valence_k / atom_h / atom_flags [n_atoms] (bit 0 ring, 1 aromatic, 2 donor, 3 acceptor, 4
 *   unsatisfied, 5 over-valent; -1, 0, 0 for atoms outside S or of a ligand without a molecule), desc_i [B,10], desc_f [B,2] =
 *   {mw, 0 (reserved)}, valid [B], status [B]: bit 0 = no molecule (the conditions of kpd_mol_keys: mol_status bits 0, 1 or 3, an
 *   empty S, an element or fragment out of range, a bond outside the ligand, twice (whichever way round it is listed), of an order
 *   outside 1 .. 3, or a seventh neighbour): desc 0, valid 0, its bond rows read bond_order and flags 0 (rows of a malformed bond range, and rows of no ligand,
 *   read 0); bits 1 and 2 as above.  A bond of S's ligand with an end outside S reads bond_order and flags 0.
 *   One wave per ligand, one launch (and five memsets) whatever B is; no scratch, no host synchronisation, no float atomics;
 *   nothing is read or written out of bounds; a ligand's results are bitwise independent of the rest of the batch and of the repeat.
 *   Two well-formed lig_ptr segments that share atoms (or bond_ptr ranges that share rows) are both processed, each workgroup
 *   writing the rows it sees: the per-atom and per-bond outputs of the shared rows are then UNSPECIFIED (whichever stores last);
 *   the per-ligand outputs (desc_i, desc_f, valid, status) are not affected.  kpd_mol_perceive never produces such input. */
kpd_status kpd_mol_sanitize(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F,
                            const int32_t *z, const int32_t *allowed, const double *mass, double mass_h, const int32_t *frag,
                            const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds,
                            const int32_t *mol_status, int32_t largest_only, int32_t *order_k, int32_t *bond_flags,
                            int32_t *valence_k, int32_t *atom_h, int32_t *atom_flags, int32_t *desc_i, double *desc_f,
                            int32_t *valid, int32_t *status, void *stream);

/* Explicit hydrogens on the sanitised molecules (csrc/hydrogens.hip): the hydrogen counts of kpd_mol_sanitize become atoms with
 * coordinates and bonds.  Stands where upstream calls Chem.AddHs(lig, addCoords=True) before every force-field step
 * (analysis/pocket_minimization.py, process_molecule(add_hydrogens=True)).  RDKit's coordinates cannot be restated here, so THIS
 * COMMENT IS THE DEFINITION; the coordinates are not RDKit's and are not compared with them.  The inputs are what kpd_mol_perceive
 * and kpd_mol_sanitize left on the device and are never written; the output is a second molecule batch in the layout of
 * kpd_mol_perceive, which every call of this file takes unchanged (its bond orders are order_k).
 * Scope S, Z(a) (0 for an atomic number outside 0 .. 255) and "both ends in S" are those of kpd_mol_sanitize.  An atom a of S gets
 *   h = atom_h[a] hydrogens, an atom outside S none.  a's neighbours are its partners over bonds with both ends in S.
 * Atom order of a ligand: its input atoms in input order, then the hydrogens grouped by parent in ascending order, by site
 *   t = 0 .. h-1 within a parent (the append convention of AddHs).  Bond rows: the input rows are sorted by (i, j) with i < j, so
 *   the H bonds of atom i sort right after its rows (i, .): the input row r (local) with first atom i moves to local row
 *   r + (hydrogens of the atoms < i), and the H bond of site t of atom i is local row
 *   (input rows whose first atom is <= i) + (hydrogens of the atoms < i) + t.
 * Arithmetic: fp64 on the fp32 coordinates; every product, sum and difference is rounded once (no fused multiply-add), sqrt and
 *   / are correctly rounded.  a.b = (ax bx + ay by) + az bz; a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx); a vector over
 *   a scalar, a sum or difference of vectors, and "x a + y b" = (x a_c) + (y b_c) are taken component by component; -a is exact.
 *   Constants: T3 = 0.3333333333333333, T1 = 0.9428090415820634, S3 = 0.5773502691896258, T2 = 0.816496580927726,
 *   H3 = 0.8660254037844386.
 * Neighbours of a in ascending row order; for neighbour b: v = P_b - P_a, n2 = v.v.  n2 < 1e-12: b is ignored for directions
 *   (status bit 3).  Else u = v / sqrt(n2).  The k remaining are u_1 .. u_k, b_1 the first of them.
 * Bond length: L = (double)(r1(Z(a)) + 32) * 0.01 with r1 from the element table above (C-H 1.07, N-H 1.03, O-H 0.95, S-H 1.35 A:
 *   the rest lengths kpd_relax picks for those bonds).
 * Class of a, the first that holds (over all of a's neighbours, ignored ones too): LINEAR if a has a bond of order_k 3 or two or
 *   more of order_k 2; PLANAR if a has a bond of order_k 2, or a is aromatic (atom_flags bit 1), or Z(a) = 7 and a neighbour is
 *   aromatic or has a bond of order_k >= 2 (amide, aniline, enamine and pyrrole-type N); TET otherwise.
 * perp(u): e = the coordinate axis with the smallest |u_c| (the first on a tie), q_c = e_c - (u_e u_c), perp = q / sqrt(q.q).
 * azimuth (k = 1, u = u_1, b = b_1): c = the lowest-row neighbour of b other than a; w = P_c - P_b, q_c = w_c - ((w.u) u_c);
 *   if c exists and q.q >= 1e-12: p0 = (-q) / sqrt(q.q) (the first hydrogen is anti to c), else p0 = perp(u).  t = u x p0,
 *   p1 = -0.5 p0 + H3 t, p2 = -0.5 p0 + (-H3) t.
 * Directions d_0 .. d_{h-1}:
 *   TET, k = 0, h <= 4: the first h of (S3, S3, S3), (S3, -S3, -S3), (-S3, S3, -S3), (-S3, -S3, S3);
 *   TET, k = 1, h <= 3: d_i = (-T3) u + T1 p_i;
 *   TET, k = 2, h <= 2: s = u_1 + u_2, x = u_1 x u_2; if s.s >= 1e-12 and x.x >= 1e-12: w = (-s) / sqrt(s.s), n = x / sqrt(x.x),
 *     d_0 = S3 w + T2 n, d_1 = S3 w + (-T2) n;
 *   TET, k = 3, h = 1: s = (u_1 + u_2) + u_3, x = (u_2 - u_1) x (u_3 - u_1); if x.x >= 1e-12: n = x / sqrt(x.x), d = -n if
 *     n.s > 0 else n (the normal, not the sum, keeps a flat three-neighbour centre from putting its H onto a neighbour);
 *     else if s.s >= 1e-4: d = (-s) / sqrt(s.s);
 *   PLANAR, k = 1, h <= 2: d_0 = -0.5 u + H3 p0 (trans to c), d_1 = -0.5 u + (-H3) p0;
 *   PLANAR, k = 2, h = 1: s = u_1 + u_2; if s.s >= 1e-4: d = (-s) / sqrt(s.s);
 *   LINEAR, k = 1, h = 1: d = -u;
 *   the general rule, for every other (class, k, h) and whenever a condition above fails (status bit 3): s = ((0 + u_1) + u_2) ..
 *     + u_k; for t = 0 .. h-1: if k + t > 0 and s.s >= 1e-4: d_t = (-s) / sqrt(s.s); else if k + t > 0: d_t = perp(the first of
 *     u_1 .. u_k, d_0 ..); else d_t = (S3, S3, S3); then s = s + d_t.
 * Position of a hydrogen: each component is (float)(P_a.c + L * d.c).
 * Limits: no clash avoidance between hydrogens of different atoms; no orientation of hydroxyl or amine hydrogens towards a
 *   pocket; no formal charges; no tautomer choice beyond atom_h; NOT RDKit's coordinates.
 *
 * kpd_mol_add_hs: pos [n_atoms,3], lig_ptr [B+1], elem / frag [n_atoms], bond_ij [cap_bonds_in,2], bond_ptr [B+1], mol_status [B] as
 *   kpd_mol_perceive wrote them; order_k [cap_bonds_in], valence_k / atom_h / atom_flags [n_atoms] and san_status [B] (its `status`)
 *   as kpd_mol_sanitize wrote them with the same largest_only; z / allowed [F]; h_class: the class the new atoms get,
 *   z[h_class] must be 1 (else every ligand has status bit 0); all device pointers.  Out (device): out_ptr [B+1], out_pos
 *   [cap_atoms,3], out_elem / out_valence / out_frag [cap_atoms], out_bond_ij [cap_bonds,2] (global output rows, i < j, per
 *   ligand sorted by i, then j), out_order [cap_bonds], out_bond_ptr [B+1], out_summary [B,4] = {n_bonds, n_frags,
 *   largest_frag_atoms (its hydrogens counted), n_invalid_atoms (step 6 of kpd_mol_perceive on out_valence and allowed, the
 *   hydrogens included)}, parent [cap_atoms] (for an H the output row of its heavy atom, else the atom's own row), source
 *   [cap_atoms] (-1 for an H, else the input row), n_h [B] (hydrogens added), status [B].  out_valence = valence_k + h for an
 *   input atom, 1 for an H; out_order = order_k, 1 for an H bond; out_frag is the parent's.  out_ptr[B] and out_bond_ptr[B] are
 *   the sizes needed, also when they exceed cap_atoms / cap_bonds (the convention of kpd_sdf_emit's text_ptr); a ligand that
 *   does not fit either capacity is not written and gets status bit 2.  Rows nothing is written to read 0 (out_pos, out_order)
 *   or -1.  The number and order of the ligands never change.  A ligand that gets no hydrogens is copied through (its rows,
 *   its bonds with order_k, no H): bit 0 = no molecule (san_status bit 0, mol_status bits 0, 1 or 3, more than 256 atoms, a
 *   malformed bond range (then no bonds are copied), an element or fragment out of range, atom_h outside 0 .. 4, an empty S, a
 *   bond row that is not i < j inside the ligand with order_k 1 .. 3, rows not ascending in (i, j), a seventh neighbour;
 *   out_summary is {n_bonds, 0, 0, 0}); bit 1 = more than 256 atoms after the addition; bit 4 = a non-finite coordinate.  A
 *   malformed lig_ptr segment contributes no rows (bit 0).  Bit 3 is informational: some atom used the general rule or ignored a
 *   coincident neighbour.  scratch: kpd_mol_add_hs_scratch_bytes(n_atoms, B) device bytes.  n_atoms + 256 B must stay below 2^31
 *   and B at most 2^21 (KPD_ERR_CAPACITY).
 *   One wave per ligand; a size pass, one exclusive scan (atoms and bonds packed into one 64-bit count) and a write pass: three
 *   launches and no fills whatever B >= 1 is (the write pass blanks the rows no ligand fills; B = 0: fills only); no host synchronisation, no float atomics; nothing is read or written out of
 *   bounds; a ligand's results are bitwise independent of the rest of the batch and of the repeat. */
int64_t kpd_mol_add_hs_scratch_bytes(int32_t n_atoms, int32_t B);
kpd_status kpd_mol_add_hs(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F,
                          const int32_t *z, const int32_t *allowed, const int32_t *frag, const int32_t *bond_ij,
                          const int32_t *order_k, const int32_t *bond_ptr, int32_t cap_bonds_in, const int32_t *mol_status,
                          const int32_t *san_status, const int32_t *valence_k, const int32_t *atom_h, const int32_t *atom_flags,
                          int32_t largest_only, int32_t h_class, int32_t cap_atoms, int32_t cap_bonds, int32_t *out_ptr,
                          float *out_pos, int32_t *out_elem, int32_t *out_valence, int32_t *out_frag, int32_t *out_bond_ij,
                          int32_t *out_order, int32_t *out_bond_ptr, int32_t *out_summary, int32_t *parent, int32_t *source,
                          int32_t *n_h, int32_t *status, void *scratch, void *stream);

/* Canonical SMILES of the sanitised molecules (csrc/smiles.hip): one string per ligand, the form every downstream tool reads.
 * Stands where upstream calls Chem.MolToSmiles(largest_mol) to compare samples (`uniqueness`, `novelty`, analysis/metrics.py:102-147).
 * RDKit's canonicalisation cannot be restated here, so THIS COMMENT IS THE DEFINITION.  The strings are valid SMILES of the same
 * molecule and canonical under THIS rule: NOT RDKit's canonical SMILES and not openbabel's; they cannot be compared as text with
 * strings from either (nor with upstream's train_smiles.pkl), only with strings of this call.  The inputs are what kpd_mol_perceive
 * and kpd_mol_sanitize left on the device and are never written.  Integer arithmetic only, modulo 2^64 where it hashes.
 * Scope S, Z(a), deg(a), "both ends in S" and mix, K1, K2, K3 are those of kpd_mol_keys; n = atoms in S.
 * Labelled graph: atom a carries (Z(a), h(a) = atom_h[a], ar(a)) and a bond the label L.  aromatic = 1: ar = bit 1 of atom_flags, L = 4 if
 *   bond_flags has bit 2 (aromatic), else order_k.  aromatic = 0 (the Kekule form): ar = 0 everywhere and L = order_k.
 * Ranks:  x_0[a] = mix(Z(a) + deg(a) K3 + (2 h(a) + ar(a)) K2 + K1 * sum over b in S, b != a, of mix(Z(b) K2 + d(a,b)))  (inv_0 of
 *   kpd_mol_keys with the atom's labels added);  step: x'[a] = mix(K1 x[a] + sum over the bonds (a,b) of mix(x[b] + L K2)); n steps.
 *   Then, while two atoms of S share a value (compared as unsigned 64-bit integers): v = the smallest shared value, a = the atom
 *   with the LOWEST INDEX among those with x[a] = v; x[a] = mix(x[a] + K3); c = (the number of distinct values before) + 1; then at
 *   most n times: step, c' = the number of distinct values; stop if c' = c, else c = c'.  rank(a) = the number of atoms of S with a
 *   smaller value.  The lowest index is the only place where the numbering of the atoms enters: the ranks, and so the string, are
 *   independent of the numbering whenever the atoms tied at each stage are equivalent under an automorphism of the labelled graph
 *   (and, as for the key, up to the 64 bits of a hash).  On the 821 inputs of tests/test_smiles_config.py (18 named molecules and
 *   8 ring templates in both modes, 48 generated ligands, 700 seeded random molecule-like graphs, 21 graphs written by hand), 8
 *   renumberings each, no string moved.
 * String: the fragments of S (the `frag` labels, which must be the connected components of S: else no molecule) in ascending rank
 *   of their start atom, joined by '.'.  The start atom of a fragment: among its atoms of minimal degree the one of lowest rank.
 *   Depth-first walk from the start atom; at an atom the neighbours are tried in ascending rank; a neighbour not yet visited becomes
 *   a child and is walked at once.  Every child but the last is written in parentheses.  A bond to a visited atom that is not the
 *   parent is a ring closure: it OPENS at the end visited first and ENDS at the other.  Behind the atom's token come the closures
 *   that end here in ascending number (each number is free again from then on), then the closures that open here in ascending rank
 *   of the partner; each opening takes the lowest free number from 1; 10 .. 99 are written %nn; no free number among 1 .. 99:
 *   status bit 1 and an empty string.
 *   Bond symbol (before the child's token, inside its parenthesis; for a closure before the number where it opens, nothing where it
 *   ends): nothing for L = 1 unless both atoms are aromatic, then '-' (biphenyl); nothing for L = 4; '=' for 2, '#' for 3.
 *   Atom token: the element symbol is symbols[elem[a]] (up to four bytes, as kpd_xyz_emit reads it), its first letter in lower case
 *   when ar = 1.  The token is the bare symbol iff Z is in the organic subset B C N O P S F Cl Br I (by atomic number; when ar = 1
 *   only b c n o p s) and the hydrogens a reader implies equal h: t = the sum of the atom's labels with L = 4 counted 1; ar = 0:
 *   (the smallest of the normal valences -- B 3, C 4, N 3 5, O 2, P 3 5, S 2 4 6, halogens 1 -- that is >= t) - t, 0 if none is;
 *   ar = 1: max(0, (the smallest normal valence) - (t + 1)).  Otherwise it is [X], [XH] or [XHn] (n = h, 2 .. 9): [nH], an
 *   over-valent [N], [Si], the [H] atoms of a hydrogenated batch.
 * Limits: no charges, no stereo, no isotopes, no atom classes (the limits of kpd_mol_sanitize: a nitro group reads ON(O)..); no
 *   tautomer canonicalisation (which N of an imidazole carries the H follows kpd_mol_sanitize, and the string follows it); a label
 *   4 between atoms that are not both aromatic (no output of kpd_mol_sanitize) is written as nothing.
 *
 * kpd_mol_smiles: lig_ptr [B+1], elem / frag [n_atoms], bond_ij [cap_bonds,2], bond_ptr [B+1], mol_status [B] as kpd_mol_perceive
 *   wrote them; order_k / bond_flags [cap_bonds], atom_h / atom_flags [n_atoms] and san_status [B] (its `status`) as
 *   kpd_mol_sanitize wrote them with the same largest_only, or with largest_only = 0 (its per-atom and per-bond outputs cover
 *   every fragment, the largest one included; only atoms and bonds of S are read here); z [F]; symbols [F] as for kpd_xyz_emit; aromatic 0 or 1; all device
 *   pointers.  Out (device): text [capacity], text_ptr [B+1] int64 (ligand b's string = text[text_ptr[b] : text_ptr[b+1]], no
 *   newline, no terminator; text_ptr[B] is the size needed, also when it exceeds capacity), status [B]: bit 0 = no molecule (san_status
 *   bit 0, the conditions of kpd_mol_keys -- mol_status bits 0, 1 or 3, more than 256 atoms, an empty S, an element or fragment out
 *   of range, a bond outside the ligand, twice, of an order_k outside 1 .. 3, a seventh neighbour --, atom_h outside 0 .. 9, or
 *   `frag` labels that are not the connected components of S), bit 1 = closure numbers exhausted, bit 2 = capacity too small for
 *   this ligand (nothing is written for it, as kpd_sdf_emit).  With bits 0 or 1 the string is empty.  Nothing is read or written
 *   out of bounds.  scratch: kpd_smiles_scratch_bytes(n_atoms, B) device bytes (36 per atom: the bound on the text of one atom).
 *   One wave per ligand builds the bytes in scratch, the library's exclusive scan turns the lengths into text_ptr, a third kernel
 *   moves the bytes: three launches whatever B >= 1 is (B = 0: the scan alone), no host synchronisation.  A ligand's bytes are
 *   independent of the rest of the batch, of cap_bonds, of capacity and of the repeat. */
int64_t kpd_smiles_scratch_bytes(int32_t n_atoms, int32_t B);
kpd_status kpd_mol_smiles(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                          const uint32_t *symbols, const int32_t *frag, const int32_t *bond_ij, const int32_t *order_k,
                          const int32_t *bond_flags, const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status,
                          const int32_t *san_status, const int32_t *atom_h, const int32_t *atom_flags, int32_t largest_only,
                          int32_t aromatic, uint8_t *text, int64_t capacity, int64_t *text_ptr, int32_t *status, void *scratch,
                          void *stream);

/* Symmetry-corrected RMSD between poses of one molecule (csrc/pose_rmsd.hip): the minimum over the automorphisms of the labelled
 * bond graph of the unaligned RMSD.  Stands where upstream calls Chem.CalcRMS(mol1, mol2) (analysis/pocket_minimization.py:21),
 * the number behind its strain table and behind redocking RMSDs: a phenyl ring flipped by 180 degrees, or a carboxylate, CF3 or
 * tert-butyl turned by one step, is the same pose, and the atom-by-atom number sqrt(sum_i |x_i - y_i|^2 / n) that kpd_relax,
 * kpd_vina_minimize and kpd_vina_dock report calls it 1 - 2.5 A away.  RDKit's matcher cannot be restated here, so THIS COMMENT IS
 * THE DEFINITION, down to the order of every choice (tests/pose_rmsd_ref.py restates it bit for bit); no agreement with RDKit's
 * numbers is claimed.  The inputs are what kpd_mol_perceive (and, for labels, kpd_mol_sanitize) left on the device and are never
 * written.  mix, K1, K2, K3, Z(a) and the scope of kpd_mol_keys are those stated there.
 * Scope S: that of kpd_mol_keys (largest_only); with skip_h != 0 the atoms with Z(a) = 1 then leave S as well (the largest
 *   fragment is chosen with them counted).  n = atoms in S; only bonds with both ends in S count; deg(a), d(a,b) inside S.
 * Labels: A(a) = Z(a) + 256 atom_label[a] (atom_label = 0 everywhere when the pointer is NULL; allowed 0 .. 2^20 - 1) and
 *   L(bond) = bond_label[row] (1 everywhere when NULL; allowed 1 .. 15).  Every atom and every bond row of the ligand is range-
 *   checked, in S or not.  NULL, NULL is elements and connectivity only: Kekule orders as labels would make the two Kekule
 *   patterns of one benzene ring different graphs.  The labelled graph of kpd_mol_smiles (atom_label = 2 h + ar, bond_label = 4 on
 *   an aromatic bond, else order_k) does not depend on the pattern either.
 * Class c(a): inv_n[a] of kpd_mol_keys with Z replaced by A and l by L, deg and d(a,b) inside S, n refinement steps.  c only
 *   prunes: it cannot change which bijections are automorphisms (an automorphism keeps it), but it decides how many candidates
 *   are tried, so it is part of the rule.
 * Automorphism: a bijection pi of S with A(pi(a)) = A(a) that maps every bond (a,b) onto a bond (pi(a), pi(b)) of the same L.
 * Source order u_0 .. u_{n-1}: repeat: the lowest-index atom of S not yet listed starts a breadth-first traversal, the
 *   neighbours of an atom in ascending index.  p(u) = the atom from whose list u was enqueued; a start atom has none.
 * Cost: a search takes a source pose X and a target pose Y (fp32 rows).  d2(u,v) = the fp64 squared distance of X[u] and Y[v]
 *   in the arithmetic of kpd_mol_perceive: the differences of the fp32 values in fp64, every product and sum rounded once,
 *   (dx^2 + dy^2) + dz^2.  cost(pi) = ((d2(u_0, pi u_0) + d2(u_1, pi u_1)) + ..) in source order; s_id = cost(identity).
 * Search: best = s_id, map = identity, nodes = 0.  At depth t, u = u_t, the candidates are the atoms v of S that are no image
 *   yet, have A(v) = A(u), deg(v) = deg(u) and c(v) = c(u), are neighbours of pi(p(u)) if u has a p(u), and have a bond
 *   (v, pi(w)) of label L(u,w) for every neighbour w of u listed before u.  They are tried in ascending (d2(u,v), index of v).
 *   For each: nodes += 1; if nodes > max_nodes the whole search stops with what it has (status bit 1); s = s_t + d2(u,v) (s_0 =
 *   0); if s >= best this candidate and all later ones of this depth are dropped; else at t = n - 1: best = s and the map is
 *   recorded (strict improvement only: the first optimum in this order wins); else descend with s_{t+1} = s.
 *   Rounded addition of non-negative terms is monotone (x <= y implies x + d <= y + d after rounding, and s + d >= s), so a
 *   dropped candidate cannot lead below best, nor can a later one of its depth: the pruning is exact, and best is the minimum of
 *   cost(pi) over ALL automorphisms whatever the order of the candidates.  The order decides nodes and which of several optimal
 *   maps is reported.
 * Results: rmsd = sqrt(best / n), plain = sqrt(s_id / n) (division and square root correctly rounded); rmsd <= plain always; a
 *   search that stopped at max_nodes still gives an upper bound of the minimum.
 * Out of scope: the RMSD after alignment (GetBestRMS), stereo (a mirror image that is a graph automorphism counts), matching
 *   two different molecules, and kpd_vina_dock's own clustering, which keeps the atom-by-atom number.
 *
 * kpd_pose_rmsd: lig_ptr [B+1], elem / frag [n_atoms], bond_ij [cap_bonds,2], bond_ptr [B+1], mol_status [B] as kpd_mol_perceive
 *   wrote them (the bond orders are not read), z [F]; bond_label [cap_bonds] / atom_label [n_atoms] int32 or NULL; ref_pos
 *   [n_atoms,3] and pos [K,n_atoms,3] fp32, pose-major, the layout of kpd_vina_dock's pos_out; all device pointers.
 *   pairs = 0: X = ref_pos, Y = pose k, K >= 1; rmsd, plain [B,K] fp64, nodes [B,K] int64; map [K,n_atoms] int32 or NULL:
 *     map[k][a] = the global row pi(a) of the recorded map, -1 outside S.
 *   pairs = 1: X = pose i, Y = pose j for i < j only, K <= 64; outputs [B,K,K]: the UPPER triangle is computed (cost is not
 *     bitwise symmetric in X and Y: the source order sums other terms), the lower one is its mirror, the diagonal 0; ref_pos and
 *     map are not used.
 *   max_nodes >= 1.  KPD_ERR_INVALID for K, pairs or max_nodes out of range.
 *   status [B]: bit 0 = no molecule (the conditions of kpd_mol_keys without its test of the orders -- mol_status bits 0, 1 or 3,
 *   more than 256 atoms, an element or fragment out of range, a bond outside the ligand, twice, a seventh neighbour --, a label
 *   out of range, or an empty S): zeros everywhere and map -1.  bit 1 = some search of this ligand stopped at max_nodes (its
 *   nodes reads max_nodes + 1), informational.  bit 2 = a non-finite coordinate of an atom of S in a pose used: every search that
 *   reads it gives zeros, nodes 0 and map -1.
 *   scratch: kpd_pose_rmsd_scratch_bytes(n_atoms, K, pairs) device bytes (-1 for arguments out of range): the running sums s_t of
 *   the searches in flight, 8 n_atoms min(64, searches per ligand).
 *   One wave per ligand, each lane a search of its own, strided over the K poses (or the K (K - 1) / 2 pairs): one launch
 *   whatever B and K are, and the fills of the outputs; no host synchronisation, no atomics on floats.  Nothing is read or
 *   written out of bounds.  A ligand's results are bitwise independent of the rest of the batch, of cap_bonds, of K (per pose)
 *   and of the repeat. */
enum { KPD_POSE_NO_MOLECULE = 1, KPD_POSE_MAX_NODES = 2, KPD_POSE_NONFINITE = 4 };
int64_t kpd_pose_rmsd_scratch_bytes(int32_t n_atoms, int32_t K, int32_t pairs);
kpd_status kpd_pose_rmsd(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                         const int32_t *frag, const int32_t *bond_ij, const int32_t *bond_ptr, int32_t cap_bonds,
                         const int32_t *mol_status, const int32_t *bond_label, const int32_t *atom_label, int32_t largest_only,
                         int32_t skip_h, const float *ref_pos, const float *pos, int32_t K, int32_t pairs, int64_t max_nodes,
                         double *rmsd, double *plain, int32_t *map, int64_t *nodes, int32_t *status, void *scratch, void *stream);

/* Substructure search on the sanitised molecules (csrc/substruct.hip): which ligands contain a query graph, at which atoms, and
 * (for typing tables) which row of a first-match-wins list an atom falls under.  Stands where upstream's users call
 * mol.HasSubstructMatch / GetSubstructMatches with a SMARTS pattern one molecule at a time, and under what rests on that: functional
 * group counts, structural alerts, Crippen-style atom typing.  RDKit's matcher cannot be restated here, so THIS COMMENT IS THE
 * DEFINITION, down to the order of every choice (tests/match_ref.py restates it); it is NOT RDKit's matcher and is not compared with
 * it.  The labels are those kpd_mol_sanitize wrote: its aromaticity applies, not RDKit's; there are no charges, no stereo and no
 * ring sizes.  No query text reaches the device: a query is compiled on the host (smarts.py, a SMARTS subset) into the int32 table
 * below, and that table is the interface.  The library ships no Crippen, QED or PAINS table.  Inputs are never written.
 * Scope S, Z(a), "both ends in S" and the conditions of "no molecule" are those of kpd_mol_keys / kpd_mol_sanitize (below, at the
 *   status).  The neighbours of an atom are its partners over bonds with both ends in S, in ascending index; deg(a) their number.
 * Labels of an atom a of S: z = Z(a) if it is in 0 .. 127, else 0; aromatic = atom_flags bit 1; ring = atom_flags bit 0;
 *   D = the neighbours with Z != 1; H = atom_h[a] + the neighbours with Z = 1; X = deg(a) + atom_h[a]; v = valence_k[a] +
 *   atom_h[a]; x = the bonds of a (in S) with bond_flags bit 0.  D, H, X, v and x are clamped at 15 (KPD_Q_TOP): 15 means 15 or more.
 * Labels of a bond: kind = 3 (aromatic) if bond_flags bit 2 is set, whatever order_k says, else order_k - 1 (0, 1, 2); ring =
 *   bond_flags bit 0; its bit number in a bond mask is kind + 4 ring.
 * The table, int32 words:
 *   [0] = KPD_Q_MAGIC, [1] = P, the rows (1 .. KPD_Q_PATTERNS), [2] = the length of the table in words, [3] = 0;
 *   [4 + p], p < P: the word at which row p starts; the rows follow each other without gaps in ascending p, the last ends the table.
 *   A row: {na (atoms, 1 .. KPD_Q_ATOMS), nc (closure bonds; na - 1 + nc <= KPD_Q_BONDS), nalt (alternatives, 1 .. 128), 0},
 *     then na atom records {parent p(t) (-1 for t = 0, else 0 .. t - 1), the mask of the bond to the parent (0 for t = 0), the
 *       first alternative of the atom, their number (1 .. KPD_Q_ALT)}: the atoms are in depth-first order;
 *     then nc closure records {s, t, mask, 0} with s < t < na: the bonds of the query that are no parent bond;
 *     then nalt alternatives of 16 words {Z[4], cls, D, H, X, v, x, need[2], forbid[2], 0, 0}: Z is a set of 128 bits (bit z of
 *       word z >> 5); cls bit 0 / 1 = an aliphatic / aromatic atom is allowed, bit 2 / 3 = an atom outside / inside a ring is
 *       allowed; D .. x are sets of 16 bits, bit k for the label k; need and forbid name LOWER rows of the table, -1 = none.
 *   An alternative holds at atom a iff a's z is in Z, its aromatic and ring labels are allowed by cls, each of D .. x has the bit
 *   of a's label, the anchor bit (below) of a is set for every row it needs and for no row it forbids.  The predicate of a query
 *   atom holds iff one of its alternatives does.  (A SMARTS "$(...)" is a `need` of the row compiled from its inside, "!$(...)"
 *   a `forbid`; negation of everything else is in the sets.)
 * Embedding of row q in a ligand: an injective map f of q's atoms into S such that the predicate of every t holds at f(t) and every
 *   bond (s, t) of the query (parent bonds and closures) lands on a bond (f(s), f(t)) whose bit is in its mask.  Non-induced: bonds
 *   between images that the query does not mention are allowed.
 * Search, per (ligand, row, anchor a in S): nothing to do unless the predicate of atom 0 holds at a; then f(0) = a, nodes = 0.  At
 *   depth t = 1 .. na - 1 the candidates are the neighbours v of f(p(t)), in ascending index, that are no image yet, whose bond to
 *   f(p(t)) is in the parent mask, at which the predicate of t holds, and that have, for every closure (s, t), a bond to f(s) in
 *   its mask.  For each candidate: nodes += 1; if nodes > max_nodes this search stops with what it has found (status bit 1);
 *   else f(t) = v, and at t = na - 1 this is an embedding, otherwise the search descends; when the candidates of a depth are
 *   used up it returns to the depth above, and ends when those of depth 1 are.  A query of one atom has its one embedding at
 *   every anchor whose predicate holds, and no nodes.
 *   Mode KPD_MATCH_ANCHORS: a search stops at its first embedding.  Mode KPD_MATCH_ALL: it enumerates all of them.
 *   Anchor bit (a, p): some embedding of row p with f(0) = a was found.  The rows are processed in ascending order; the bits of a
 *   row are complete before a higher row reads them.
 * Typing: type_group [P] (-1 or anything outside 0 .. G-1: the row takes no part; else its group g) and value [P] fp64.  For a
 *   group g and an atom of S: type = the lowest row of g whose anchor bit the atom has, -1 if none.  type_sum[b][g] = the sum of
 *   value[type] over the typed atoms of S in ascending atom index, from 0.0, one rounded fp64 addition at a time; untyped[b][g] =
 *   the atoms of S without a type.
 *
 * kpd_mol_match: lig_ptr [B+1], elem / frag [n_atoms], bond_ij [cap_bonds,2], bond_ptr [B+1], mol_status [B] as kpd_mol_perceive
 *   wrote them; order_k / bond_flags [cap_bonds], valence_k / atom_h / atom_flags [n_atoms] and san_status [B] (its `status`) as
 *   kpd_mol_sanitize wrote them with the same largest_only, or with largest_only = 0; z [F]; type_group, value as above or NULL
 *   with G = 0; all device pointers.  The table comes twice: table_host, the table_words words in HOST memory, which are checked
 *   before anything is launched, and table, the same words in device memory, which the kernel reads (the caller keeps the two
 *   equal).  KPD_ERR_INVALID, and no launch, for a malformed table: a bad head, counts beyond the limits, a row whose length is
 *   not what its counts need, a parent that is not lower, a closure that is not s < t < na, alternatives out of range, a
 *   mask with bits it cannot have, a reference to a row that is not lower; also for a mode other than 0 / 1 and max_nodes < 1.
 *   Out (device), W = ceil(P / 32): anchor [n_atoms, W] uint32 (bit p & 31 of word p >> 5 of row a = the anchor bit (a, p));
 *   hits [B, P] = the anchors of row p in ligand b; first_map [B, P, KPD_Q_ATOMS] int32 or NULL: the first embedding found
 *   from the lowest anchor that has one, as global atom rows, -1 beyond the row's atoms and without a hit; with KPD_MATCH_ALL
 *   also n_embed [B, P] int64, the embeddings (as maps: a benzene ring holds c1ccccc1 twelve times), and cover [n_atoms, W]
 *   uint32: bit p of atom a = a is the image of some query atom in some embedding of row p (both may be NULL otherwise).  Where a
 *   search stopped at max_nodes, hits, anchor, n_embed and cover are LOWER BOUNDS, and what rows that reference such a row
 *   report follows the bits that were found.  With G > 0: atom_type [G, n_atoms] int32, type_sum [B, G] fp64, untyped [B, G].
 *   status [B]: bit 0 = no molecule (san_status bit 0, mol_status bits 0, 1 or 3, more than 256 atoms, an empty S, an element or
 *   fragment out of range, a bond outside the ligand, twice, of an order_k outside 1 .. 3, a seventh neighbour, or, on an atom
 *   of S, atom_h outside 0 .. 9 or a negative valence_k): zeros everywhere, first_map -1, atom_type -1; atoms of no ligand and
 *   atoms outside S read the same.  bit 1 = some search of this ligand stopped at max_nodes, informational.
 *   One wave per ligand, lane l runs the searches of the anchors l, l + 64, ..; the rows in ascending order, one barrier between
 *   rows: one launch whatever B and P are, and the fills of the outputs (three to eight); no scratch, no host synchronisation,
 *   no float atomics.  Nothing is read or written out of bounds.  A ligand's results are bitwise independent of the rest of the
 *   batch, of cap_bonds and of the repeat; what row p reports is independent of the rows it does not reference (through any
 *   chain), type_sum included. */
#define KPD_Q_ATOMS 16
#define KPD_Q_BONDS 24
#define KPD_Q_ALT 8
#define KPD_Q_PATTERNS 512
#define KPD_Q_TOP 15
#define KPD_Q_MAGIC 0x4b505101
enum { KPD_MATCH_ANCHORS = 0, KPD_MATCH_ALL = 1 };
enum { KPD_MATCH_NO_MOLECULE = 1, KPD_MATCH_MAX_NODES = 2 };
kpd_status kpd_mol_match(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, const int32_t *elem, int32_t F, const int32_t *z,
                         const int32_t *frag, const int32_t *bond_ij, const int32_t *order_k, const int32_t *bond_flags,
                         const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status, const int32_t *san_status,
                         const int32_t *valence_k, const int32_t *atom_h, const int32_t *atom_flags, int32_t largest_only,
                         const int32_t *table_host, const int32_t *table, int32_t table_words, int32_t mode, int64_t max_nodes,
                         const int32_t *type_group, const double *value, int32_t G, uint32_t *anchor, int32_t *hits,
                         int32_t *first_map, int64_t *n_embed, uint32_t *cover, int32_t *atom_type, double *type_sum,
                         int32_t *untyped, int32_t *status, void *stream);

/* Plausibility checks of poses (csrc/pose_check.hip): whether a pose is physically plausible, which no energy, score or RMSD of the
 * calls around it says.  The list follows PoseBusters (Buttenschoen, Morris & Deane 2024): bond lengths and angles in range, no
 * internal clash, flat aromatic rings and double bonds, no clash with the protein, little volume overlap with it.  PoseBusters
 * runs on RDKit and cannot be restated here, so THIS COMMENT IS THE DEFINITION, down to the order of every operation
 * (tests/pose_check_ref.py restates it bit for bit).  THESE ARE NOT PoseBusters' NUMBERS: the reference lengths and angles are
 * this library's own (the radii table above and the centre classes of kpd_mol_add_hs), not RDKit's distance-geometry bounds;
 * there is no energy-ratio check; there is no stereo.  The default thresholds are PoseBusters' published ones AS RECALLED, NOT
 * CHECKED AGAINST THE PAPER OR ITS SOURCE: nothing may rely on them being its values.  All of them are fields of the params.
 * The graph is what kpd_mol_perceive and kpd_mol_sanitize left on the device; the poses need not be the pose it was perceived
 * from (relaxed, minimised and docked poses are the main customers).  Inputs are never written.
 * Scope S, Z(a) (0 for an atomic number outside 0 .. 255), deg(a) and "both ends in S" are those of kpd_mol_sanitize; the
 *   neighbours of an atom are its partners over bonds with both ends in S, in ascending index.
 * Arithmetic: fp64 on the fp32 values; every product, sum, difference and quotient is rounded once (no fused multiply-add), sqrt
 *   and / are correctly rounded; only + - x / sqrt (and floor, for lattice indices) are used.  d2(a,b) = (dx^2 + dy^2) + dz^2 on
 *   the differences of the fp32 coordinates, d = sqrt(d2); a.b, a x b, a / s and sums of vectors as for kpd_mol_add_hs.  R_a =
 *   lig_radius[elem[a]], R_j = pocket_radius[j] as fp64.  Every per-pose result is a minimum, a maximum or an integer count: no
 *   order of summation exists.  "Takes part": an atom of S (a pocket atom) whose radius is > 0; checks 3, 5 and 6 see no other.
 * r0 of a bond (a,b): from the radii table, in half picometres: L1 = 2 (r1(a) + r1(b)); L2, L3 the same sums of the double and
 *   triple radii where both are non-zero; L15 = (L1 + L2) / 2.  L = L15 (L1 without an L2) if the bond is aromatic (bond_flags bit
 *   2); else L3 (L1 without) for order_k 3; else L2 (L1 without) for order_k 2; else L1.  r0 = (double)L * 0.005.  A bond with
 *   r1 = 0 at either end has no r0 and is examined by neither check 1 nor check 2.
 * Check 1, bond lengths (fail bit 0): every bond of S with an r0: v = d / r0; fails iff v < bond_lo or v > bond_hi.
 * Check 2, 1-3 distances (bit 1): every centre j of S and every pair i < k of its neighbours that are not bonded to each other and
 *   whose bonds to j have an r0: x = r0(i,j), y = r0(j,k), d0sq = ((x x) + (y y)) - (((2 x) y) c), v = d(i,k) / sqrt(d0sq); fails
 *   iff v < angle_lo or v > angle_hi.  c = cos t0 from deg(j) and the class kpd_mol_add_hs gives j (LINEAR / PLANAR / TET, the
 *   conjugated-N clause included): deg >= 4: -T3; deg 3: -0.5 if PLANAR or LINEAR, else -T3; deg 2: -1 if LINEAR, -0.5 if PLANAR,
 *   else -T3.  T3 = 0.3333333333333333.
 * Check 3, internal clash (bit 2): every pair a < b of atoms that take part whose shortest path in S has four or more bonds, or
 *   that are not connected: v = d / (R_a + R_b); fails iff v < clash_min.
 * Check 4, flatness, three sub-checks.  A squared norm below 1e-12 is DEGENERATE.
 *   aromatic rings (bit 3): every simple cycle of 5 or of 6 atoms in the graph of the aromatic bonds of S, each once: listed from
 *     its lowest atom p_0 towards the lower of that atom's two ring neighbours, p_0 .. p_{m-1}.  c = (((P_0 + P_1) + ..) + P_{m-1})
 *     / m; v_k = P_k - c; N = ((0 + v_0 x v_1) + v_1 x v_2) + .. + v_{m-1} x v_0; degenerate N.N: the ring fails and has no value;
 *     else u = N / sqrt(N.N), value = max_k |v_k . u|; fails iff value > ring_max.
 *   planar centres (bit 4): every atom a of S with deg 3 that has a bond of order_k 2 or is aromatic (atom_flags bit 1); the
 *     conjugated-N clause does NOT count here.  Neighbours q_0 < q_1 < q_2: N = (Q_1 - Q_0) x (Q_2 - Q_0); degenerate: fails, no
 *     value; else value = |(P_a - Q_0) . (N / sqrt(N.N))|; fails iff value > centre_max.
 *   double-bond twist (bit 5): every bond (a,b), a < b, of order_k 2 that is no ring bond (bond_flags bit 0), every neighbour c of
 *     a other than b and every neighbour d of b other than a: n1 = (P_a - P_c) x (P_b - P_a), n2 = (P_b - P_a) x (P_d - P_b); a
 *     degenerate n1.n1 or n2.n2: skipped and counted; else value = ((n1.n2) (n1.n2)) / ((n1.n1) (n2.n2)), the squared cosine of
 *     the torsion; fails iff value < twist_min.
 * Check 5, pocket clash (bit 6): every ligand atom a x every atom j of its pocket, both taking part: v = d / (R_a + R_j); fails
 *   iff v < pocket_min.
 * Check 6, volume overlap (bit 7): the lattice of the points (h ix, h iy, h iz) over ALL integers (each coordinate one rounded
 *   product; the lattice is fixed in space, not per ligand).  A point is in the ligand iff d2(point, P_a) <= R_a R_a for some
 *   ligand atom a that takes part; it is counted once and belongs to the lowest such a.  A ligand point is in the pocket iff
 *   d2(point, Q_j) <= (s R_j) (s R_j) for some atom j of the pocket that takes part, s = pocket_scale.  n_lig_points, n_overlap_points;
 *   value = (double)n_overlap_points / (double)n_lig_points, 0 without points; fails iff value > overlap_max.
 *   pocket_of = -1: checks 5 and 6 examine nothing (no points are counted) and pass.
 * kpd_pose_check_defaults: bond_lo 0.75, bond_hi 1.25, angle_lo 0.75, angle_hi 1.25, clash_min 0.7, ring_max 0.25, centre_max
 *   0.25, twist_min 0.75, pocket_min 0.75, pocket_scale 0.8, overlap_max 0.075, h 0.5 (RECALLED, see above).  Every field must be
 *   in 0 .. 1e6, h in 0.1 .. 4 and pocket_scale at most 4 (KPD_ERR_INVALID).
 *
 * kpd_pose_check: lig_ptr, elem, z, frag, bond_ij, order_k, bond_flags, bond_ptr, mol_status, san_status, atom_h, atom_flags and
 *   largest_only as for kpd_mol_smiles; pos [K,n_atoms,3] fp32, pose-major, K >= 1; lig_radius [F], pocket_radius [n_pocket]
 *   (van der Waals radii from the caller); pocket_x, pocket_ptr, pocket_of, max_atoms and max_pocket as for kpd_vina_score
 *   (n_pocket at most 2^22); params: NULL for the defaults; all device pointers but params.
 *   Out (device), per (ligand, pose), row b K + k: fail [B,K] (the bits above); report [B,K,10] fp64 = {bond min, bond max, angle
 *   min, angle max, internal clash min, ring max, centre max, twist min, pocket clash min, overlap value}, 0 where nothing was
 *   examined (or nothing had a value); counts [B,K,17] int32 = {bonds examined, failing, angles, failing, internal pairs, failing,
 *   rings, failing, centres, failing, torsions, failing, torsions skipped, pocket pairs, failing, n_lig_points, n_overlap_points};
 *   atom_fail [K,n_atoms]: per atom the bits of the checks it took part in failing (both ends of a bond or pair, the three atoms
 *   of an angle, the atoms of a ring, the centre, the four atoms of a torsion, the ligand atom of a pocket pair; bit 7 on the
 *   owners of overlapping points when check 6 fails); status [B,K]:
 *   bit 0 = no molecule (san_status bit 0, mol_status bits 0, 1 or 3, more than max_atoms atoms, an empty S, an element or
 *   fragment out of range, a bond outside the ligand, twice, of an order_k outside 1 .. 3, a seventh neighbour, atom_h outside
 *   0 .. 9, or a bond of S that joins two `frag` labels); bit 1 = bad input: a coordinate of the pose or of its pocket that is not
 *   finite or not below 2^20 in magnitude (the lattice indices must fit), a radius of an atom of the ligand or of its pocket that
 *   is not finite or above 8, a pocket_of outside [-1, P) or a malformed pocket segment; bit 2 (informational) = some atom of S or
 *   of the pocket took no part.  Of bits 0 and 1 one is reported, the first that is met in this order: the ligand's segment, size,
 *   mol_status and bond range (bit 0); pocket_of and the pocket segment (bit 1); san_status and the graph (bit 0); coordinates and
 *   radii (bit 1).  With bit 0 or 1 the pose's rows are zeros and fail is 0 (rows of a malformed ligand segment are
 *   zeros as well); nothing is read or written out of bounds.
 *   One wave per (ligand, pose): one launch and five fills whatever B and K are; no scratch, no host synchronisation, no float
 *   atomics.  Of a pocket the first atoms are staged in LDS (as many as max_pocket asks for, at most 2048) and the rest is read
 *   from global memory with the same result to the bit; the pocket atoms that can reach the ligand's lattice points are culled by
 *   a box test per pose and a sphere test per ligand atom, whose margins cannot change a count.  A pose's results are bitwise independent of the rest of the batch, of the
 *   ligand's place in it, of K, of max_atoms / max_pocket, of cap_bonds and of the repeat. */
enum { KPD_CHECK_NO_MOLECULE = 1, KPD_CHECK_BAD_INPUT = 2, KPD_CHECK_ATOM_OUT = 4 };
enum { KPD_CHECK_REPORT = 10, KPD_CHECK_COUNTS = 17 };
typedef struct kpd_pose_check_params {
    double bond_lo, bond_hi, angle_lo, angle_hi, clash_min, ring_max, centre_max, twist_min, pocket_min, pocket_scale, overlap_max, h;
} kpd_pose_check_params;
void kpd_pose_check_defaults(kpd_pose_check_params *params);
kpd_status kpd_pose_check(const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms, const int32_t *elem, int32_t F,
                          const int32_t *z, const int32_t *frag, const int32_t *bond_ij, const int32_t *order_k,
                          const int32_t *bond_flags, const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status,
                          const int32_t *san_status, const int32_t *atom_h, const int32_t *atom_flags, int32_t largest_only,
                          const float *pos, int32_t K, const float *lig_radius, const float *pocket_x, const float *pocket_radius,
                          const int32_t *pocket_ptr, int32_t n_pocket, int32_t P, int32_t max_pocket, const int32_t *pocket_of,
                          const kpd_pose_check_params *params, int32_t *fail, double *report, int32_t *counts, int32_t *atom_fail,
                          int32_t *status, void *stream);

/* Relaxation of sampled ligands inside their rigid pockets (csrc/relax.hip).  Stands where upstream runs
 * analysis/pocket_minimization.py: RDKit's UFF on ligand + receptor with every receptor atom fixed, maxIts = 400, then the plain
 * (unaligned) CalcRMS and the energies before and after.  RDKit's UFF cannot be restated here -- it needs hydrogens, atom typing,
 * torsions and inversions -- so THIS COMMENT IS THE DEFINITION of the force field and of the minimiser.  IT IS NOT UFF: heavy
 * atoms only, no torsions or inversions, no electrostatics, a rigid pocket.  Its energies are comparable between samples relaxed
 * by this function and with nothing else, RDKit's numbers least of all.
 *
 * Ligand and pocket are in one frame, as for kpd_clash_score.  All arithmetic is fp64 on values read from the fp32 inputs;
 * energies in kcal/mol, lengths in Angstrom.  Only the connectivity of kpd_mol_perceive is used, not bond_order (the length
 * classes know no aromaticity): rest values are the ideal values nearest to the sampled geometry, so a benzene ring stays one.
 * Bond (i,j):  E = 1/2 k_b (d - r0)^2.  Candidates for r0 from the radii table above, in half picometres: L1 = 2 (r1(i) + r1(j)),
 *   L2 and L3 the same sums of the double and triple radii where both are non-zero, L15 = (L1 + L2) / 2 where L2 exists;
 *   r0 = 0.005 L of the candidate nearest to the sampled length, the longer one on a tie.  d < 1e-6: energy, no force.
 * Angle (i,j,k) at centre j, for i < k among j's neighbours:  E = 1/2 k_a (cos t - cos t0)^2, with c the sampled cosine:
 *   c > cos 100 deg (-0.1736481776669303): t0 = the sampled angle (small rings are not reshaped); else a centre with four or more
 *   neighbours: 109.47122 deg (cos t0 = -0.3333333228927115); else c <= cos 150 deg (-0.8660254037844387): 180 deg (cos t0 = -1);
 *   else c <= cos 114.7356 deg (-0.4184314830435483): 120 deg (-1/2); else 109.47122 deg.  cos = (u.v) * (1 / sqrt(|u|^2 |v|^2));
 *   an angle with an arm shorter than 1e-6 adds nothing, and one that cannot be measured in the sample keeps "the sampled angle".
 * Non-bonded pair:  Lennard-Jones in UFF's form, e(d) = D_ij [(x_ij / d)^12 - 2 (x_ij / d)^6], x_ij = sqrt(x_i) sqrt(x_j),
 *   D_ij = sqrt(D_i) sqrt(D_j) (fp64 roots of the fp32 parameters).  The pair energy is e(d) - e(r_c) for d < r_c and 0 beyond.
 *   Soft core: for d < s x_ij it is the tangent line of e at s x_ij (minus e(r_c)), which keeps the energy and the force of a
 *   clashing sample finite and well scaled.  d < 1e-6: energy, no force.  It applies, with weight w_intra, to the pairs of ligand
 *   atoms whose shortest path has three or more bonds or that are not connected, and, with weight 1, to every ligand atom x every
 *   atom of its pocket.  The vdW parameters {x, D} come from the caller: lig_vdw [F,2] per ligand class, pocket_vdw [n_pocket,2].
 * E = ((bond + angle) + intra) + pocket.  gmax = the largest norm of an atom's gradient.
 *
 * Minimiser: L-BFGS on the 3n ligand coordinates, 8 stored pairs (s, y), two-loop recursion with the initial scaling
 *   gamma = s.y / y.y of the newest pair; a pair with s.y <= 1e-10 y.y, or with y.y <= 1e-20 g'.g' (g' the gradient at the new
 *   point: where the energy is linear in the step, as inside the soft core, y is rounding noise), is not stored.  One iteration, while gmax > gtol and fewer
 *   than max_iters were run: p = -H g; if not g.p < 0, drop the pairs and take p = -g.  First trial step
 *   alpha = min(1, max_step / max_i |p_i|) (no atom moves more than max_step in a trial: none tunnels through another); accept if
 *   E' is finite and E' <= E + 1e-4 alpha g.p, else halve alpha, at most 20 times.  If no step is accepted and pairs are stored,
 *   drop them (the iteration is spent); if none are stored, stop with status bit 3.  Every dot product and every energy and
 *   gradient sum is reduced in a fixed order that depends on the ligand and its pocket only.
 *   The report describes the rows written: after at least one iteration the positions are rounded to fp32 and the energy, its
 *   parts and gmax are evaluated once more there (that evaluation is counted).  Should the rounding alone turn a gain into a rise
 *   (E > E_before), the ligand keeps its input rows and the numbers of the first evaluation.  Hence E_after <= E_before always.
 *
 * kpd_relax: pos [n_atoms,3], lig_ptr [B+1], elem [n_atoms], bond_ij [cap_bonds,2], bond_ptr [B+1], mol_status [B] as
 *   kpd_mol_perceive wrote them, z [F], lig_vdw [F,2]; pocket_x [n_pocket,3], pocket_vdw [n_pocket,2], pocket_ptr [P+1] (pocket q
 *   = rows [pocket_ptr[q], pocket_ptr[q+1]), any number of atoms), pocket_of [B] (the pocket of every ligand, -1 = none; many
 *   ligands share one pocket without copies of it); all device pointers.  max_atoms (1 .. 256) and max_pocket are host-known
 *   upper bounds that size the workgroup's LDS: a ligand with more than max_atoms atoms is left out (bit 0); of a pocket, the
 *   first atoms are staged in LDS, as many as max_pocket asks for and fit, and the rest is read from global memory with the
 *   same result to the bit.  params: NULL for kpd_relax_defaults (k_b 700, k_a 200, r_c 10, s 0.6, w_intra 1, gtol 1e-3, max_step
 *   0.2, max_iters 400).
 *   Out (device): pos_out [n_atoms,3] fp32 (may be pos itself); report [B,12] fp64 = {E_before, E_after, rmsd (plain RMSD of
 *   the rows written against the input rows, in atom order, no alignment, no symmetry), gmax_after, iterations, energy
 *   evaluations, bond / angle / intra / pocket part of E_after, pocket part of E_before, gmax_before}; status [B]:
 *   bit 0 = no molecule (mol_status bits 0, 1 or 3, more than max_atoms atoms, or inputs that are no output of kpd_mol_perceive:
 *   an element out of range, a bond outside the ligand, twice, between elements the bond rule never bonds, or a seventh
 *   neighbour), bit 1 = a non-finite coordinate in the ligand or its pocket, a vdW parameter that is not finite, x <= 0 or D < 0,
 *   a pocket_of outside [-1, P) or a malformed pocket segment, bit 2 = gmax_after > gtol without bit 3: max_iters came first, or the fp32
 *   rounding of pos_out alone lifts the gradient over gtol (k_b times half an ulp of a coordinate of 10 A is 3e-4; informational), bit 3 = the
 *   line search could not lower the energy further (informational; the result stands).  With bit 0 or 1 the ligand's rows of
 *   pos_out are its input rows and its report is zeros; nothing is read or written out of bounds.
 *   One workgroup per ligand, one launch (and one copy pos -> pos_out) for the whole minimisation of every ligand whatever B is;
 *   no scratch, no host synchronisation, no atomics on floats; a ligand's result is bitwise independent of the rest of the batch,
 *   of max_atoms / max_pocket, and of the repeat. */
typedef struct kpd_relax_params {
    double k_b, k_a, r_c, s, w_intra, gtol, max_step;
    int32_t max_iters;
} kpd_relax_params;
void kpd_relax_defaults(kpd_relax_params *params);
kpd_status kpd_relax(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms, const int32_t *elem,
                     int32_t F, const int32_t *z, const float *lig_vdw, const int32_t *bond_ij, const int32_t *bond_ptr,
                     int32_t cap_bonds, const int32_t *mol_status, const float *pocket_x, const float *pocket_vdw,
                     const int32_t *pocket_ptr, int32_t n_pocket, int32_t P, int32_t max_pocket, const int32_t *pocket_of,
                     const kpd_relax_params *params, float *pos_out, double *report, int32_t *status, void *stream);

/* Scores of sampled ligands in their rigid pockets (csrc/vina.hip).  Stands where upstream hands pocket_minimized_ligands.sdf to
 * gnina (analysis/docking/gen_docking_cmds.py), which docks or minimises under the AutoDock Vina scoring function.  This is the
 * Vina FUNCTIONAL FORM: five pair terms over ligand x pocket heavy atoms, the sum divided by 1 + w_rot N_rot, with its analytic
 * gradient.  The typing cannot be Vina's own (Vina reads hydrogens and AutoDock atom types from PDBQT; ligands and pockets here
 * carry heavy atoms and element classes only), so THIS COMMENT IS THE DEFINITION.  THE SCORES ARE NOT gnina's OR Vina's NUMBERS:
 * they rank samples scored by this function against each other.  Out of scope here: no intramolecular
 * term in the score, no hydrogens, no aromaticity; this call scores the poses it is given.  The torsional and rigid-body
 * minimisation under this function (gnina's --minimize) is kpd_vina_minimize below, built on the gradient delivered here, and
 * the search for poses (gnina's docking) is kpd_vina_dock below it.
 *
 * Ligand and pocket are in one frame, as for kpd_relax.  All arithmetic is fp64 on values read from the fp32 inputs.
 * Distances: d2(i,j) by the recipe of kpd_mol_perceive and kpd_pocket_select (differences of the fp32 coordinates in fp64, each
 *   product and sum rounded once, (dx^2 + dy^2) + dz^2, no fused multiply-add).  A pair takes part iff d2 < r_c * r_c; then
 *   r = sqrt(d2) and the surface distance is d = (r - R_i) - R_j, in that order, R the fp64 values of the fp32 radii.
 * Types: three flags per atom, H = 1 (hydrophobic), D = 2 (hydrogen-bond donor), A = 4 (acceptor), from the atomic number Z, the
 *   heavy degree deg and the neighbours.  A neighbour with Z = 1 is ignored throughout (it neither counts in deg nor matters below).
 *   Ligand: neighbours and orders are those of kpd_mol_perceive (bond_ij, bond_order).  Pocket: a pair i < j of one pocket is a
 *   neighbour pair iff it passes step 1 of the bond rule above (d2 > 0.16 and the order-1 test with m = 45, radii table above);
 *   its order comes from step 3; there is no degree pruning and no valence repair; an atomic number outside the table has no
 *   neighbours.
 *     Z = 6 (C):                   H iff no neighbour has Z outside {1, 6}, else 0
 *     Z = 9, 17, 35, 53:           H
 *     Z = 7 (N):                   D iff deg <= 2 and not (deg == 1 and that bond has order 3); A iff not D and deg <= 2; else 0
 *     Z = 8 (O):                   A always; also D iff deg == 0, or deg == 1 and that bond has order 1
 *     Z = 12, 20, 25 .. 30 (metals): D
 *     anything else:               0
 *   An atom with Z = 1, or whose radius is not > 0, takes no part in any term; its reported type is -1.
 *   Limits: an aromatic or imine N of degree 2 counts as a donor (no aromaticity, no hydrogens), so a histidine's two ring N
 *   are both donors (for the ligand, flags recomputed from the hydrogen counts of kpd_mol_sanitize can be passed as lig_type_in); the O rule leans on the length classes (C=O 1.23 A is a double, C-O 1.36 .. 1.43 A a single).  The caller
 *   may override any atom's flags (lig_type_in, and whatever it writes into pocket_type; bits above 4 are ignored).
 * Rotors: N_rot = the number of ligand bonds of order 1 with both ends of heavy degree >= 2 that are in no ring (a bond is in a
 *   ring iff its ends stay connected when it is removed).  Limits: an amide C-N counts; rotors that would move only hydrogens
 *   (hydroxyl, amine) do not count, where Vina counts them half.
 * Pair terms, for u = d / 0.5 and v = (d - 3) / 2:
 *     gauss1 = exp(-(u u)), gauss2 = exp(-(v v)), repulsion = d < 0 ? d d : 0,
 *     hydrophobic, only when both atoms carry H: 1 for d < 0.5, 1.5 - d for d < 1.5, else 0,
 *     hbond, only when one atom carries D and the other A (either way round, once per pair): 1 for d < -0.7, d / -0.7 for d < 0,
 *     else 0.
 *   inter = sum over the five terms of w_term * (sum over the pairs of term); score = inter / (1 + w_rot N_rot).
 *   kpd_vina_defaults: w_gauss1 -0.035579, w_gauss2 -0.005156, w_repulsion 0.840245, w_hydrophobic -0.035069, w_hbond -0.587439,
 *   w_rot 0.05846, r_c 8.  RECALLED, NOT CHECKED AGAINST TROTT & OLSON 2010 OR VINA'S SOURCE: nothing may rely on these being
 *   Vina's values.  The radii come from the caller (lig_radius [F] per ligand class, pocket_radius [n_pocket]).
 *   grad[i] = (1 / (1 + w_rot N_rot)) sum_j (sum over the terms of w_term dterm/dd) (x_i - x_j) / r; a pair with r < 1e-6
 *   contributes energy and no force.  atom_score[i] = the un-normalised weighted pair sum of ligand atom i.
 *   Every sum is reduced in a fixed order that depends on the ligand and its pocket only.
 *
 * kpd_vina_pocket_types: pocket_x [n_pocket,3], pocket_z [n_pocket] (atomic numbers), pocket_ptr [P+1]; all device pointers.
 *   Out (device): pocket_type [n_pocket] (flags, or -1; -1 also for the atoms outside every well-formed segment), status [P]:
 *   bit 0 = malformed segment (not 0 <= pocket_ptr[q] <= pocket_ptr[q+1] <= n_pocket; none of its atoms is typed), bit 1 = a
 *   non-finite coordinate (that atom has no neighbours and type -1).  One launch (and a memset) whatever P is; one thread per
 *   atom, the atoms of its pocket tiled through LDS: quadratic per pocket, which is right for pockets of hundreds of atoms.
 *   Done once per pocket set and reused for raw and relaxed poses.
 *
 * kpd_vina_score: pos, lig_ptr, elem, z, bond_ij, bond_ptr, mol_status, pocket_x, pocket_ptr, pocket_of, max_atoms and
 *   max_pocket as for kpd_relax; bond_order [cap_bonds] as kpd_mol_perceive wrote it; lig_radius [F]; lig_type_in NULL, or
 *   [n_atoms] whose entries >= 0 replace the perceived flags; pocket_radius, pocket_type [n_pocket]; params: NULL for
 *   kpd_vina_defaults.  Out (device): report [B,8] fp64 = {score, inter, weighted gauss1, gauss2, repulsion, hydrophobic, hbond,
 *   N_rot}; grad [n_atoms,3] fp64 or NULL; atom_score [n_atoms] fp64 or NULL; lig_type [n_atoms] or NULL; status [B]:
 *   bit 0 = no molecule (the conditions of kpd_relax, or a bond order outside 1 .. 3), bit 1 = a non-finite coordinate or radius
 *   in the ligand or its pocket, a pocket_of outside [-1, P) or a malformed pocket segment, bit 2 (informational) = some atom of
 *   the ligand or of its pocket took no part (type -1, or a radius that is not > 0).  With bit 0 or 1 the ligand's report, grad
 *   and atom_score rows are zeros and its types are -1 (rows of a malformed ligand segment are not written); nothing is read or
 *   written out of bounds.  pocket_of = -1: all terms are 0 and N_rot is still reported.  Inputs are never written.
 *   One workgroup per ligand, one launch whatever B is; no scratch, no host synchronisation, no atomics on floats; a ligand's
 *   results are bitwise independent of the rest of the batch, of max_atoms / max_pocket, and of the repeat. */
typedef struct kpd_vina_params {
    double w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond, w_rot, r_c;
} kpd_vina_params;
void kpd_vina_defaults(kpd_vina_params *params);
kpd_status kpd_vina_pocket_types(const float *pocket_x, const int32_t *pocket_z, const int32_t *pocket_ptr, int32_t n_pocket, int32_t P,
                                 int32_t *pocket_type, int32_t *status, void *stream);
kpd_status kpd_vina_score(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms, const int32_t *elem,
                          int32_t F, const int32_t *z, const float *lig_radius, const int32_t *bond_ij, const int32_t *bond_order,
                          const int32_t *bond_ptr, int32_t cap_bonds, const int32_t *mol_status, const int32_t *lig_type_in,
                          const float *pocket_x, const float *pocket_radius, const int32_t *pocket_type, const int32_t *pocket_ptr,
                          int32_t n_pocket, int32_t P, int32_t max_pocket, const int32_t *pocket_of, const kpd_vina_params *params,
                          double *report, double *grad, double *atom_score, int32_t *lig_type, int32_t *status, void *stream);

/* Local minimisation of sampled ligands under that score, over rigid-body and torsional degrees of freedom (csrc/vina_min.hip).
 * Stands where upstream runs gen_docking_cmds.py --minimize: gnina --minimize on pocket_minimized_ligands.sdf, written out as
 * gen_ligands_gnina_minimized.sdf.  gnina's minimiser, its torsion tree (which reads hydrogens) and its numbers cannot be restated
 * here, so THIS COMMENT IS THE DEFINITION.  THE POSES AND SCORES ARE NOT gnina's OR Vina's: typing, rotor rule, pair terms, weights
 * and the recalled constants are those of kpd_vina_score, and what is reported is the score at the nearest local minimum of THIS
 * function.  No search in this call (kpd_vina_dock below searches), a rigid pocket, no hydrogens.
 *
 * All arithmetic is fp64 on values read from the fp32 inputs.  The distance recipe, the types, the rotor rule, the pair terms,
 * the weights, r_c and the r < 1e-6 rule are those of kpd_vina_score, word for word.
 * Active rotors: the bonds the N_rot rule counts (order 1, both ends of heavy degree >= 2, in no ring), in bond_ij order; the
 *   first max_rotors of them are active, the rest are frozen (status bit 4, informational).  max_rotors = 0: rigid bodies only.
 *   T = the number of active rotors.
 * Rigid pieces: the connected components of the bond graph without the active rotor bonds.
 * Bodies: each fragment (the labels of `frag`, as kpd_mol_perceive wrote them: connected components ranked by their lowest atom)
 *   is one body with 6 coordinates, translation t_f and rotation vector w_f.  A ligand with more than 8 fragments is left out
 *   (status bit 5).  F = the number of fragments; D = 6 F + T <= 112.
 * Orientation of rotor k = (i, j), i < j as in bond_ij: walk the graph from j without the bond.  If the walk reaches the lowest
 *   atom of the fragment, the moved set M_k is the fragment minus the reached set and b_k = i; else M_k is the reached set and
 *   b_k = j.  a_k is the other end.  depth(k) = the number of active rotors k' with b_k in M_k'.
 * The chart.  The state is the Cartesian x (rigid by construction); a step delta in R^D acts as move(x, delta) in two stages:
 *   1. torsions: for atom i, the active rotors with i in M_k from the deepest to the shallowest (no ties on a path); each turns
 *      the atom about the line through the PRE-STEP x_a, x_b by delta_theta_k: with u_k = (x_b - x_a) / |x_b - x_a| (0 if that
 *      length is below 1e-6) and r = x - x_b, x' = x_b + (r cos + (u x r) sin) + u (u.r)(1 - cos) (Rodrigues).  Deeper turns
 *      never move a shallower axis, so this is the exact tree kinematics.
 *   2. bodies: x'' = (c_f + R(delta_w_f)(x' - c_f)) + delta_t_f, c_f the mean of the fragment's pre-step atoms summed in index
 *      order, R the Rodrigues rotation about delta_w_f / |delta_w_f| by |delta_w_f|, the identity for |delta_w_f| < 1e-12.
 *   Gradient at delta = 0 from the Cartesian gradient g:  dE/dt_f = sum_{i in f} g_i;  dE/dw_f = sum_{i in f} (x_i - c_f) x g_i;
 *   dE/dtheta_k = u_k . sum_{i in M_k} (x_i - x_b) x g_i.  Order in the vector: (t, w) per fragment in label order, then the
 *   rotors in active order.  First-order velocity of atom i under p:  v_i = p_t + p_w x (x_i - c_f) + sum_{k: i in M_k}
 *   p_theta_k u_k x (x_i - x_b).
 * Objective: E = inter + w_intra intra, un-normalised.  inter is kpd_vina_score's weighted five-term sum.  intra is the same pair
 *   function (same weights, radii, types, cutoff) over the ligand pairs i < j of which both atoms take part, that lie in
 *   different rigid pieces, and whose shortest bond path has four or more bonds or that are not connected.
 *   score = inter / (1 + w_rot N_rot); N_rot counts all rotors, the frozen ones included.
 * Minimiser: L-BFGS on delta with the rules of kpd_relax: 8 stored pairs, gamma = s.y / y.y of the newest pair, a pair with
 *   s.y <= 1e-10 y.y or y.y <= 1e-20 g'.g' is not stored; one iteration, while gnorm > gtol and fewer than max_iters were run:
 *   p = -H g; if not g.p < 0, drop the pairs and take p = -g.  First trial alpha = min(1, max_step / max_i |v_i|); accept if E'
 *   is finite and E' <= E + 1e-4 alpha g.p, else halve alpha, at most 20 times.  If no step is accepted and pairs are stored,
 *   drop them (the iteration is spent); if none are stored, stop with status bit 3.  A pair is s = alpha p and y = g'_delta -
 *   g_delta, each gradient taken in the chart of its own point.  gnorm = max_d |g_delta,d|.
 *   After at least one iteration x is rounded to fp32 and evaluated once more there (that evaluation is counted); should E have
 *   risen above E_before, the ligand keeps its input rows and the numbers of the first evaluation.  Hence E_after <= E_before.
 *   Every sum is reduced in a fixed order that depends on the ligand and its pocket only.
 *
 * kpd_vina_minimize: the inputs of kpd_vina_score, and frag [n_atoms] as kpd_mol_perceive wrote it; max_rotors (0 .. 64) is a
 *   host-known bound like max_atoms; params: NULL for kpd_vina_min_defaults (kpd_vina_defaults, w_intra 1, gtol 1e-3, max_step
 *   0.2, max_iters 200).  Out (device): pos_out [n_atoms,3] fp32 (may be pos itself); report [B,16] fp64 = {score_before,
 *   score_after, E_before, E_after, inter_before, inter_after, intra_before, intra_after, rmsd (plain, as kpd_relax),
 *   gnorm_before, gnorm_after, iterations, evaluations, N_rot, T, F}; status [B]: bits 0, 1, 2 as for kpd_vina_score (bit 0 also
 *   for a bond whose ends are not i < j, a frag entry outside [0, n), a bond between two labels, or a label below the largest
 *   that no atom carries), bit 3 = the
 *   line search could not lower E further (informational), bit 4 = rotors were frozen (informational), bit 5 = more than 8
 *   fragments, bit 6 = gnorm_after > gtol without bit 3 (max_iters came first; informational).  With bit 0, 1 or 5 the ligand's
 *   rows of pos_out are its input rows and its report is zeros; nothing is read or written out of bounds.
 *   One workgroup per ligand, one launch (and one copy pos -> pos_out) whatever B is; no scratch, no host synchronisation, no
 *   atomics on floats; a ligand's result is bitwise independent of the rest of the batch, of max_atoms / max_pocket, of
 *   max_rotors once it is at least the ligand's rotor count, and of the repeat. */
enum {
    KPD_VINA_MIN_NO_MOLECULE = 1,
    KPD_VINA_MIN_BAD_INPUT = 2,
    KPD_VINA_MIN_ATOM_OUT = 4,
    KPD_VINA_MIN_LINE_SEARCH = 8,
    KPD_VINA_MIN_FROZEN_ROTORS = 16,
    KPD_VINA_MIN_FRAGMENTS = 32,
    KPD_VINA_MIN_ITER_CAP = 64
};
typedef struct kpd_vina_min_params {
    double w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond, w_rot, r_c, w_intra, gtol, max_step;
    int32_t max_iters;
} kpd_vina_min_params;
void kpd_vina_min_defaults(kpd_vina_min_params *params);
kpd_status kpd_vina_minimize(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms,
                             const int32_t *elem, int32_t F, const int32_t *z, const float *lig_radius, const int32_t *frag,
                             const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds,
                             const int32_t *mol_status, const int32_t *lig_type_in, const float *pocket_x, const float *pocket_radius,
                             const int32_t *pocket_type, const int32_t *pocket_ptr, int32_t n_pocket, int32_t P, int32_t max_pocket,
                             const int32_t *pocket_of, int32_t max_rotors, const kpd_vina_min_params *params, float *pos_out,
                             double *report, int32_t *status, void *stream);

/* Monte-Carlo search of sampled ligands in their pockets under that score (csrc/vina_dock.hip).  Stands where upstream runs
 * gen_docking_cmds.py without --minimize: full gnina docking inside --autobox_ligand <reference ligand>, written out as
 * gen_ligands_docked.sdf.  gnina's search, its torsion tree and its numbers cannot be restated here, so THIS COMMENT IS THE
 * DEFINITION.  THE POSES AND SCORES ARE NOT gnina's OR Vina's: typing, rotor rule, pair terms, weights and the recalled constants
 * are those of kpd_vina_score, and the search is the one written down here.  A rigid pocket, no hydrogens.
 *
 * All arithmetic is fp64.  Everything not restated here is that of kpd_vina_minimize, word for word: types, rotors, pieces,
 * bodies, the chart move(x, delta), the objective E = inter + w_intra intra, and the minimiser's rules.
 * Random numbers: Philox4x32-10, key = (low, high) half of seed, counter = (q, s, c, id): block q, step s, chain c, and id =
 *   lig_id[b] (b itself when lig_id is NULL), so a ligand's result does not depend on its place in the batch.  Word j of a block
 *   becomes u_j = (w_j + 0.5) 2^-32, in (0, 1).  ball(u1, u2, u3), a vector of the unit ball: z = 2 u1 - 1, phi = 2 pi u2, rho =
 *   cbrt(u3), v = rho (sqrt(1 - z z) cos phi, sqrt(1 - z z) sin phi, z).  Blocks: q = 0, the mutation of step s; q = 1, word 0:
 *   the Metropolis draw of step s; of the random start (s = 0): q = 2 + 2 f, the rotation of fragment f; q = 3 + 2 f, its place;
 *   q = 18 + j, word k - 4 j: the angle of active rotor k in 4 j .. 4 j + 3.
 * minimise(x, K): the iteration loop of kpd_vina_minimize from x with max_iters = K and fresh L-BFGS memory, in fp64 throughout:
 *   the closing fp32 step is not taken.  K = 0 is one evaluation.  A line search that is exhausted ends that minimisation only.
 * The box test: a pose is outside iff the mean of all the ligand's atoms (summed in index order) is below box_lo or above box_hi
 *   in any coordinate.
 * Chain c of a ligand:
 *   Step 0.  Chain 0 starts at the input pose.  A chain c >= 1 starts at move(input, delta): theta_k = pi (2 u - 1) for every
 *     active rotor; w_f = pi ball(u0, u1, u2) of block 2 + 2 f and t_f = (lo + u (hi - lo)) - c_f, coordinate j from word j of
 *     block 3 + 2 f, for every fragment f (c_f its centre in the input pose).  The start is minimised with step_iters and becomes
 *     the chain's current pose, and its best if E is finite; if E is not finite, or if the minimised start of a chain c >= 1 is
 *     outside the box (counted as a box rejection), the chain ends with nothing found.
 *   Step s = 1 .. n_steps.  With u0 .. u3 of block 0: e = min(floor(u0 (2 F + T)), 2 F + T - 1) selects one slot group of a delta
 *     that is zero elsewhere.  e < F: t_e = amplitude ball(u1, u2, u3).  F <= e < 2 F, f = e - F: w_f = (amplitude / r_f) ball(u1,
 *     u2, u3), r_f = sqrt(sum_{i in f} |x_i - c_f|^2 / n_f) summed in index order, each |.|^2 as (dx^2 + dy^2) + dz^2; delta stays
 *     0 where r_f < 1e-6.  e >= 2 F, k = e - 2 F: theta_k = pi (2 u1 - 1).  candidate = minimise(move(current, delta), step_iters).
 *     It is box-rejected, before minimising (then nothing is evaluated) and again after, if it is outside the box.  Otherwise it is
 *     accepted iff E_cand is finite and (E_cand < E_cur or u_M < exp((E_cur - E_cand) / temperature)), and then becomes the
 *     current pose.  The chain's best is the lowest-E candidate with a finite E that was not box-rejected, accepted or not; a tie
 *     stays with the earlier step.
 *   Refinement.  x = minimise(best, max_iters), then the closing step of kpd_vina_minimize: x is rounded to fp32 and evaluated
 *     there; the rounded point is kept iff its E does not exceed the best's E and, for a chain c >= 1, it is inside the box, else
 *     the fp32 rounding of the best itself is kept and evaluated.  What is reported is always the evaluation at the fp32 rows
 *     written.  So a pose of a chain c >= 1 lies in the box (to the fp32 rounding of its rows); chain 0, which starts at the input
 *     pose wherever that is, is box-tested in its steps only.
 * Modes: the chains that found a pose are ranked by (E, chain index) and walked in that order; a pose is kept iff its RMSD to
 *   every pose kept before is >= min_rmsd, until n_modes are kept.  That RMSD is sqrt(sum_i |x_i - y_i|^2 / n) over all atoms of
 *   the fp32 rows, in fp64, summed in index order.
 *
 * kpd_vina_dock: the inputs of kpd_vina_minimize, and box_lo, box_hi [B,3] fp32 (the search box of every ligand), lig_id [B] or
 *   NULL, seed, n_chains (1 .. 64), n_steps (>= 0), n_modes (1 .. n_chains); params: NULL for kpd_vina_dock_defaults
 *   (kpd_vina_min_defaults, temperature 1.2, amplitude 2 A (Vina's, RECALLED, NOT CHECKED), min_rmsd 1 A, step_iters 20; max_iters
 *   200 is the refinement's).  KPD_ERR_INVALID for counts out of range and for temperature, amplitude or min_rmsd that are not
 *   > 0.  Out (device): pos_out [n_modes,n_atoms,3] fp32, mode-major, so mode 0 is a drop-in pos; rows of a mode that does not
 *   exist are the input rows (pos_out and chain_pos must not be pos).  n_found [B].  report [B,n_modes,8] fp64 = {score, E,
 *   inter, intra, rmsd to the input pose (as kpd_vina_minimize's), rmsd to mode 0, chain, gnorm}, zeros for a mode that does not
 *   exist.  chain_pos [n_chains,n_atoms,3] fp32 and chain_report [B,n_chains,10] fp64 = {E, inter, intra, step of the best (-1:
 *   none), accepted steps, box rejections, evaluations, found, gnorm, score} are caller-allocated, the search's only global
 *   intermediate, and double as diagnostics; the rows of a chain that found nothing are the input rows, its first three and last
 *   two columns zeros.  status [B]: bits 0, 1, 2, 4, 5 as for kpd_vina_minimize, bit 7 = a box bound that is not finite or lo >
 *   hi, bit 8 = the input pose is outside the box (informational), bit 9 = fewer than n_modes were found (informational).  With
 *   bit 0, 1, 5 or 7 the ligand is left out: n_found 0, zero reports, its input rows in every mode and chain.
 *   k_vina_dock runs one workgroup per (ligand, chain), k_vina_dock_modes one per ligand: two launches, and n_modes + n_chains
 *   copies pos -> rows, whatever B is; no host synchronisation, no atomics on floats.  A ligand's result is bitwise independent
 *   of the rest of the batch and of its place in it (given lig_id), of max_atoms / max_pocket, of max_rotors once it is at least
 *   the ligand's rotor count, and of the repeat; chain c's chain_pos and chain_report do not depend on n_chains.  With n_chains =
 *   1, n_steps = 0 and step_iters = 0, mode 0 is kpd_vina_minimize's result to the bit. */
enum {
    KPD_VINA_DOCK_NO_MOLECULE = 1,
    KPD_VINA_DOCK_BAD_INPUT = 2,
    KPD_VINA_DOCK_ATOM_OUT = 4,
    KPD_VINA_DOCK_FROZEN_ROTORS = 16,
    KPD_VINA_DOCK_FRAGMENTS = 32,
    KPD_VINA_DOCK_BAD_BOX = 128,
    KPD_VINA_DOCK_START_OUTSIDE = 256,
    KPD_VINA_DOCK_FEW_MODES = 512
};
typedef struct kpd_vina_dock_params {
    double w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond, w_rot, r_c, w_intra, gtol, max_step;
    int32_t max_iters;
    double temperature, amplitude, min_rmsd;
    int32_t step_iters;
} kpd_vina_dock_params;
void kpd_vina_dock_defaults(kpd_vina_dock_params *params);
kpd_status kpd_vina_dock(const float *pos, const int32_t *lig_ptr, int32_t n_atoms, int32_t B, int32_t max_atoms,
                         const int32_t *elem, int32_t F, const int32_t *z, const float *lig_radius, const int32_t *frag,
                         const int32_t *bond_ij, const int32_t *bond_order, const int32_t *bond_ptr, int32_t cap_bonds,
                         const int32_t *mol_status, const int32_t *lig_type_in, const float *pocket_x, const float *pocket_radius,
                         const int32_t *pocket_type, const int32_t *pocket_ptr, int32_t n_pocket, int32_t P, int32_t max_pocket,
                         const int32_t *pocket_of, int32_t max_rotors, const float *box_lo, const float *box_hi,
                         const int32_t *lig_id, uint64_t seed, int32_t n_chains, int32_t n_steps, int32_t n_modes,
                         const kpd_vina_dock_params *params, float *pos_out, int32_t *n_found, double *report, float *chain_pos,
                         double *chain_report, int32_t *status, void *stream);

/* Structure files (csrc/structure_io.hip): PDB text -> the arrays kpd_pocket_select takes, for a batch of files.  Replaces the
 * parsing upstream leaves to prody / BioPython (byop.py:101-117, process_crossdocked.py:96-111, process_bindingmoad.py:124-135):
 * per-file Python work that this library does on the device.  None of those packages is restated here, so THIS COMMENT IS THE
 * DEFINITION; where it departs from them is listed at the end.  SDF / MOL input: kpd_sdf_parse below.
 *
 * Input: text [n_bytes] bytes and file_ptr [B+1] int64, both device: file b is text[file_ptr[b] : file_ptr[b+1]].  `text` needs no
 *   alignment.  file_ptr must ascend within [0, n_bytes]; a file whose own segment does not (file_ptr[b] < 0, file_ptr[b+1] <
 *   file_ptr[b] or > n_bytes) gets status bit 4 and no atoms, and what the other files of such a table read as is unspecified
 *   (still nothing is read or written out of bounds).  n_bytes + B < 2^31 - 1 (KPD_ERR_CAPACITY).
 * Lines: a line starts at file_ptr[b] of a non-empty file and behind every '\n' inside a file; it ends in front of the next line
 *   start or at the end of its file, so a file boundary ends a line even without '\n'.  The line's content is its bytes without
 *   that '\n' and then without one '\r' at the end; of the content only the first 80 bytes (columns 1 .. 80) are read, and
 *   columns beyond the content read as blanks (0x20).  Tabs and bytes >= 0x80 are ordinary bytes: they are no blanks, digits or
 *   letters, so they make a number they fall in unparsable.
 * Real field (columns a .. b): blanks, one optional '+' or '-', digits with at most one '.', blanks; at least one digit ('1.' and
 *   '.5' are real, '.', '+', '' are not); nothing else: no exponent, no 'nan' / 'inf', no blank inside.  With m the integer its
 *   digits spell and k the number of digits behind the '.', the value is fp32(fp64(m) / fp64(10^k)), negated after the division
 *   for '-': one IEEE fp64 division and one rounding to fp32, exact operands, hence numpy.float32(float(field)); '-0.000' is -0.0.
 *   More than 15 digits (leading zeros not counted) or k > 15: unparsable.
 * Integer field: blanks, optional sign, 1 .. 9 digits, blanks.  Anything else (hybrid-36, 'A000', '****') is unparsable.
 * Records: a line whose columns 1-6 are 'ATOM  ' or 'HETATM' and lie inside the content is a record; one whose columns 1-6 are
 *   'ENDMDL' ends the first model.  Kept are the records in front of the first ENDMDL line of their file, in file order: they are
 *   the atoms, atom_ptr[b] .. atom_ptr[b+1] of file b.  Columns (wwPDB format 3.3, 1-based): name 13-16, altLoc 17, resName 18-20,
 *   chainID 22, resSeq 23-26 (integer), iCode 27, x / y / z 31-38 / 39-46 / 47-54 (real), occupancy 55-60, tempFactor 61-66 (real),
 *   element 77-78.  The serial (7-11) and everything else is not read ('*****' is fine).
 * Out per atom (capacity cap_atoms rows; atom_ptr [B+1], atom_ptr[B] = the size needed, also when it exceeds cap_atoms; the atoms
 *   of a file that does not fit are not written), all device:
 *   pos [.,3]      x, y, z; all three NaN for a bad record (below)
 *   occ_b [.,2]    occupancy, tempFactor; NaN where the field is blank, beyond the line or unparsable (no error)
 *   sym            element symbol, up to two bytes NUL-padded little-endian as kpd_xyz_emit's `symbols`, 0 for none.  From the
 *                  non-blank bytes of columns 77-78 in order, a letter in first place in upper and in second place in lower case,
 *                  other bytes as they are.  If both columns are blank, from columns 13-14 = (a, b) by the first rule that applies
 *                  (flag bit 6 says so): a is blank or a digit: b.  a is a letter and resName is a standard amino acid: a
 *                  ('HD11', 'HH11' are hydrogens).  a and b are letters and a b, in that case form, is one of
 *                    Li Be Ne Na Mg Al Si Cl Ar Ca Sc Ti Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Zr Mo Ru Rh Pd Ag Cd In Sn
 *                    Sb Te Xe Cs Ba Pt Au Pb
 *                  : that symbol.  Otherwise a.  A heuristic, as BioPython's is.
 *   elem           index of sym in the caller's symbols [F] (first match), or F: upstream's "other" column
 *   name, resname  columns 13-16 / 18-20 as they are, packed little-endian (column 13 / 18 in the low byte)
 *   res_class      index of resname in the caller's resnames [R] (packed the same way), or R: upstream's aa_to_idx for ca_only
 *   resseq         the integer of columns 23-26, 0 when unparsable
 *   tags           chainID | iCode << 8 | altLoc << 16
 *   line_off       int64: offset of the record's first byte in text (slice the lines of selected atoms back out as pocket.pdb)
 *   res_idx        a kept record starts a residue if it is the first of its file or if its columns 18-20 and 22-27 (resName,
 *                  chainID, resSeq, iCode; compared as bytes) differ from those of the kept record before it.  res_idx = the
 *                  number of starts up to and including the record, minus 1, per file.  The run-length reading of a PDB file
 *                  (BioPython's); equal to prody's getResindices when the atoms of every residue are contiguous.
 *                  kpd_pocket_select uses only equality of these labels.
 *   flags          bit 0 HETATM, bit 1 hydrogen (sym is H or D), bit 2 water (resName one of HOH DOD WAT H2O OH2 TIP SOL), bit 3
 *                  altLoc neither blank nor 'A', bit 4 standard amino acid (resName one of ALA ARG ASN ASP CYS GLN GLU GLY HIS ILE
 *                  LEU LYS MET PHE PRO SER THR TRP TYR VAL), bit 5 C-alpha (name ' CA ' and bit 4), bit 6 element guessed from
 *                  the name, bit 7 bad record: content shorter than 54 columns, or x, y, z or resSeq unparsable.
 *   No filtering happens here: the flags become the probe / emit masks of kpd_pocket_select.
 * Out per file: n_res [B] (residue starts), status [B]: bit 0 = no atom, bit 1 = cap_atoms too small for this file, bit 2 = a bad
 *   record, bit 3 = records behind the first ENDMDL were ignored, bit 4 = malformed segment, bit 5 = cap_lines too small (no file
 *   is parsed then).  n_lines [1] = lines of the whole buffer, the cap_lines needed.
 * scratch: kpd_pdb_scratch_bytes(n_bytes, B, cap_lines) device bytes; it holds the table of line starts.  Six launches whatever B
 *   is; no host synchronisation; no float atomics; bitwise independent of batch composition.  The line scan reads the buffer in
 *   tiles of KPD_STRUCT_TILE bytes with aligned 16-byte loads (the partial 16 bytes at either end byte by byte).
 * Nothing is read or written out of bounds for any bytes of text whatsoever.
 * Known deviations: no hybrid-36, no exponents (Python's float takes them); altloc choice is the caller's (flag bit 3 is prody's
 *   default, not BioPython's highest occupancy); water is the list above, not prody's selection grammar; CONECT, TER, MODEL,
 *   ANISOU and SEQRES are not read; mmCIF, PDBQT and gzip are not supported. */
#define KPD_STRUCT_TILE 4096
int64_t kpd_pdb_scratch_bytes(int64_t n_bytes, int32_t B, int32_t cap_lines);
kpd_status kpd_pdb_parse(const uint8_t *text, int64_t n_bytes, const int64_t *file_ptr, int32_t B, const uint32_t *symbols, int32_t F,
                         const uint32_t *resnames, int32_t R, int32_t cap_lines, int32_t cap_atoms, float *pos, float *occ_b,
                         uint32_t *sym, int32_t *elem, uint32_t *name, uint32_t *resname, int32_t *res_class, int32_t *resseq,
                         uint32_t *tags, int64_t *line_off, int32_t *res_idx, int32_t *flags, int32_t *atom_ptr, int32_t *n_res,
                         int32_t *status, int32_t *n_lines, void *scratch, void *stream);

/* kpd_sdf_parse: SDF / MOL V2000 text -> molecules in exactly the layout kpd_mol_perceive writes, so that every consumer of that
 * layout (kpd_sdf_emit, kpd_mol_keys, kpd_mol_sanitize, kpd_pose_rmsd, kpd_vina_score, kpd_relax, ...) takes a file's ligand
 * unchanged, with the bonds the file states instead of perceived ones.  Replaces parse_ligand (data_processing/
 * pdbbind_processing.py:45-83: rdkit's SDMolSupplier(sanitize=False) and RemoveAllHs).  THIS COMMENT IS THE DEFINITION.
 * text, file_ptr, lines, real and integer fields: as for kpd_pdb_parse.
 * Records: a line whose first four bytes are '$$$$' closes a record; the lines of a file behind its last '$$$$' line (all of them
 *   if it has none: one bare MOL block) are one more record unless every one of them is without content.  mol_ptr [B+1]: file b
 *   holds the records mol_ptr[b] .. mol_ptr[b+1]; mol_ptr[B] = M, the records of the call, is the cap_mols needed.  The records of
 *   a file whose records do not all fit cap_mols are not parsed (file_status bit 1).
 * A record, by line: title, program, comment, counts, n_a atom lines, n_b bond lines, property lines up to 'M  END'; what follows
 *   (data items) is not read.  Counts line: n_a = integer of columns 1-3, n_b = integer of columns 4-6, columns 35-39 'V2000'.
 *   Atom line: x / y / z = reals of columns 1-10 / 11-20 / 21-30; symbol = the non-blank bytes of columns 32-34 up to the first
 *   blank behind them, the first in upper and the others in lower case, packed as kpd_xyz_emit's `symbols`; columns 35-36 (mass
 *   difference) and 37-39 (charge): an integer other than 0 sets status bit 5.  Bond line: i, j, type = integers of columns 1-3,
 *   4-6, 7-9 (1-based atoms of the block).  Type 1 / 2 / 3 is the order; type 4 is written as order 1 and sets status bit 4
 *   ("aromatic bond type: call kpd_mol_sanitize").  A property line 'M  CHG' or 'M  ISO' sets status bit 5 ("charges / isotopes
 *   present, ignored": the library carries none).
 * remove_h != 0: atoms whose symbol is H or D are dropped with their bonds and the others renumbered in order (RemoveAllHs, :66-67).
 * Out per record (all device; capacity cap_mols records, cap_atoms atoms, cap_bonds bonds):
 *   lig_ptr [cap_mols+1] (record m's atoms are rows lig_ptr[m] .. lig_ptr[m+1]; lig_ptr[M] = atoms needed; entries behind M repeat
 *   it), pos [.,3], sym, elem (index of sym in symbols [F], or F for "other": such an atom sets status bit 2, is invalid in step 6,
 *   and upstream raises Unparsable for its ligand), valence (sum of its bonds' orders), frag; bond_ij [cap_bonds,2] (global rows,
 *   i < j, per record sorted by i then j whatever the file's order), bond_order, bond_ptr [cap_mols+1]; summary [cap_mols,4] and
 *   frag by steps 5-6 of kpd_mol_perceive with the caller's z and allowed [F] (an atom whose class is F or whose z the element
 *   table does not know is invalid); title_off [cap_mols,2] int64 = begin and end of the title line's content in text;
 *   status [cap_mols]: bits 0-3 are kpd_mol_perceive's (0 = no atom, 1 = cap_atoms or cap_bonds too small for this record: nothing
 *   but lig_ptr / bond_ptr is written for it, 2 = an "other" or unknown element, 3 = record left out), 4 and 5 as above, and why it
 *   was left out: 6 = 'V3000' in columns 35-39, 7 = unparsable (count, version, coordinate, blank symbol, bond index or type; a bond
 *   to atom 0 or beyond n_a; types 5-8), 8 = truncated (fewer lines than 4 + n_a + n_b, or no 'M  END' behind them), 9 = a self
 *   bond, a repeated bond, or after hydrogen removal more than 256 atoms, more than 3 n bonds or an atom with more than 6 bonds.
 *   A record that is left out has no atoms and no bonds (lig_ptr[m+1] = lig_ptr[m]) and summary 0.
 * Out per file: mol_ptr, file_status [B]: bit 1 = cap_mols too small, bit 4 = malformed segment, bit 5 = cap_lines too small.
 *   n_lines [1] as for kpd_pdb_parse.  scratch: kpd_sdf_parse_scratch_bytes(n_bytes, B, cap_lines, cap_mols).
 * One wave per record.  Ten launches and one memset whatever B is; no host synchronisation; no float atomics; bitwise independent
 *   of batch composition.  Nothing is read or written out of bounds for any bytes of text whatsoever.
 * Not read: V3000 blocks, formal charges, isotopes, stereo flags, atom lists, SGroups; MOL2 and PDBQT are not supported. */
int64_t kpd_sdf_parse_scratch_bytes(int64_t n_bytes, int32_t B, int32_t cap_lines, int32_t cap_mols);
kpd_status kpd_sdf_parse(const uint8_t *text, int64_t n_bytes, const int64_t *file_ptr, int32_t B, const uint32_t *symbols, int32_t F,
                         const int32_t *z, const int32_t *allowed, int32_t remove_h, int32_t cap_lines, int32_t cap_mols,
                         int32_t cap_atoms, int32_t cap_bonds, int32_t *mol_ptr, int32_t *file_status, int32_t *lig_ptr, float *pos,
                         uint32_t *sym, int32_t *elem, int32_t *valence, int32_t *frag, int32_t *bond_ij, int32_t *bond_order,
                         int32_t *bond_ptr, int32_t *summary, int64_t *title_off, int32_t *status, int32_t *n_lines, void *scratch,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* KPD_H */
