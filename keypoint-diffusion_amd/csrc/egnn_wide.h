// The wide EGNN denoiser (egnn_wide.hip): hidden_nf 257 .. 1024, inference only, behind the kpd_egnn handle (egnn.hip dispatches).
#pragma once
#include "egnn_kernels.h"

namespace kpd {

constexpr int WIDE_MAX_HID = 1024;

struct EgnnWide;
kpd_status wide_create(const kpd_egnn_config &c, EgnnWide **out);
void wide_destroy(EgnnWide *w);
kpd_status wide_load_weight(EgnnWide *w, const char *name, const float *src, const int64_t *shape, int ndim, hipStream_t st);
kpd_status wide_commit(EgnnWide *w);
kpd_status wide_reserve(EgnnWide *w, int max_B, int max_n_lig, int max_n_kp, int max_n_kk, int max_lig_pg, int max_kp_pg);
kpd_status wide_forward(EgnnWide *w, const kpd_batch *bt, const float *t_dev, float *eps_h, float *eps_x, hipStream_t st);
kpd_status wide_debug_state(EgnnWide *w, const char *what, float *out, int64_t n_floats, hipStream_t st);
kpd_status wide_last_counts(EgnnWide *w, int32_t out[8], hipStream_t st);

}  // namespace kpd
