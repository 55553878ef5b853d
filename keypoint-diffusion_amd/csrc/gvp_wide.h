// The wide GVP denoiser (gvp_wide.hip): n_hidden_scalars 257 .. 1024, inference only, behind the kpd_gvp handle (gvp.hip dispatches).
#pragma once
#include "common.h"

namespace kpd {

constexpr int GVP_WIDE_MAX_S = 1024;

struct GvpWide;
kpd_status gvp_wide_create(const kpd_gvp_config &c, GvpWide **out);
void gvp_wide_destroy(GvpWide *w);
kpd_status gvp_wide_load_weight(GvpWide *w, const char *name, const float *src, const int64_t *shape, int ndim, hipStream_t st);
kpd_status gvp_wide_commit(GvpWide *w);
kpd_status gvp_wide_reserve(GvpWide *w, int max_B, int max_n_lig, int max_n_kp, int max_n_kk, int max_lig_pg, int max_kp_pg);
kpd_status gvp_wide_forward(GvpWide *w, const kpd_batch *bt, const float *t_dev, float *eps_h, float *eps_x, hipStream_t st);
kpd_status gvp_wide_debug_state(GvpWide *w, const char *what, float *out, int64_t n_floats, hipStream_t st);
kpd_status gvp_wide_last_counts(GvpWide *w, int32_t out[8], hipStream_t st);

}  // namespace kpd
