// Reverse-diffusion state update around the denoiser: the elementwise part of
// KeypointDiffusion.sample_p_zs_given_zt (models/ligand_diffuser.py:515-536) fused with the
// ligand-COM removal (remove_com :185-203).  One workgroup per complex; the new ligand
// coordinates are staged in LDS so the COM is a fixed-order sum (deterministic).
#include "engine.h"

namespace kpd {

// The three state updates of the sampler share this body, so the candidate expression and the COM removal are the same
// instructions in every one of them (FMA contraction cannot differ) and a complex without fixed atoms leaves the inpainting
// kernel with the bits of the plain one.  One workgroup per complex; sx [3 * n_lig of this complex] stages the new positions.
enum { UPD_PLAIN = 0, UPD_INPAINT = 1, UPD_RENOISE = 2, UPD_GUIDED = 3 };

struct InpaintArgs {                        // UPD_INPAINT only (include/kpd.h has the algorithm)
    const unsigned char *fixed;             // [n_lig] 1 = this atom is given
    const float *known_x, *known_h;         // [n_lig,3] input frame, [n_lig,atom_nf] normalised; read on fixed rows only
    const float *kp_com0;                   // [B,3] keypoint mean in the input frame
    const float *known_noise_x, *known_noise_h;
};

struct GuideArgs {                          // UPD_GUIDED only (include/kpd.h, "Clash guidance")
    const int *wall_ptr;                    // [B+1] wall atoms of complex b = rows [wall_ptr[b], wall_ptr[b+1])
    const float *wall_x;                    // [n_wall,3] input frame
    const float *kp_com0;                   // [B,3] keypoint mean in the input frame
    float threshold;
};

// The squared-hinge pair loop of the guided update and of k_clash_score.  One wavefront holds the point p; lane l takes the wall
// atoms l, l + 64, ... of [wlo, wlo + nw) in that order, then a butterfly over the 64 lanes: a fixed order that depends on nothing
// but the point and its complex's wall, and every lane returns the same sums.  A wall atom r sits at (r - o0) + o1.
//   f = sum (threshold - d)+ (p - r') / d   (pairs with d < 1e-6 have no direction and add nothing to f)
//   e = 1/2 sum (threshold - d)+^2,  n = pairs with d < threshold,  dmin = smallest such d (+inf without one)
struct PairSums { float f[3], e, dmin; int n; };

__device__ __forceinline__ PairSums hinge_pairs(float px, float py, float pz, const float *__restrict__ wall_x, int wlo, int nw,
                                                const float (&o0)[3], const float (&o1)[3], float threshold, int lane) {
    PairSums a{{0.0f, 0.0f, 0.0f}, 0.0f, __builtin_inff(), 0};
    for (int j = lane; j < nw; j += 64) {
        const float *r = wall_x + (size_t)(wlo + j) * 3;
        const float dx = px - ((r[0] - o0[0]) + o1[0]), dy = py - ((r[1] - o0[1]) + o1[1]), dz = pz - ((r[2] - o0[2]) + o1[2]);
        const float d = sqrtf(dx * dx + dy * dy + dz * dz);
        if (d < threshold) {
            const float h = threshold - d;
            a.e += 0.5f * h * h;
            a.n += 1;
            a.dmin = fminf(a.dmin, d);
            if (d >= 1e-6f) {
                const float k = h / d;
                a.f[0] += k * dx;
                a.f[1] += k * dy;
                a.f[2] += k * dz;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.f[0] += __shfl_xor(a.f[0], off, 64);
        a.f[1] += __shfl_xor(a.f[1], off, 64);
        a.f[2] += __shfl_xor(a.f[2], off, 64);
        a.e += __shfl_xor(a.e, off, 64);
        a.n += __shfl_xor(a.n, off, 64);
        a.dmin = fminf(a.dmin, __shfl_xor(a.dmin, off, 64));
    }
    return a;
}

// c = the coefficient row of this complex: {alpha_t|s, var, sigma_step} and, beyond UPD_PLAIN, {alpha_s, sigma_s, sigma_t|s};
// UPD_GUIDED adds {alpha_t, sigma_t, w}.  UPD_GUIDED: ia.fixed may be null (no inpainting mask); sxh [3 * n_lig] stages x-hat.
template <int MODE>
__device__ __forceinline__ void update_and_center(const int *__restrict__ lig_ptr, const int *__restrict__ kp_ptr, int atom_nf,
                                                  float *__restrict__ lig_x, float *__restrict__ lig_h, float *__restrict__ kp_x,
                                                  const float *__restrict__ eps_x, const float *__restrict__ eps_h,
                                                  const float *__restrict__ noise_x, const float *__restrict__ noise_h,
                                                  const float *__restrict__ c, const InpaintArgs &ia, float *sx, float *s_com,
                                                  float *s_frame, const GuideArgs &ga = GuideArgs{}, float *sxh = nullptr) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int llo = lig_ptr[b], nl = lig_ptr[b + 1] - llo;
    const int klo = kp_ptr[b], nk = kp_ptr[b + 1] - klo;
    const float alpha = c[0], var = c[1], sigma = c[2];

    if constexpr (MODE == UPD_INPAINT || MODE == UPD_GUIDED) {
        // frame: mean of this complex's keypoint rows as they are on entry.  Wave w < 3 sums component w: lane-strided partial
        // sums, then a butterfly over the 64 lanes -- a fixed order that depends on nothing but this complex.
        const int w = tid >> 6, lane = tid & 63;
        if (w < 3) {
            float p = 0.0f;
            for (int j = lane; j < nk; j += 64) p += kp_x[(size_t)(klo + j) * 3 + w];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) p += __shfl_xor(p, off, 64);
            if (lane == 0) s_frame[w] = p / (float)nk;
        }
        __syncthreads();
    }

    for (int i = tid; i < nl * 3; i += blockDim.x) {
        const size_t g = (size_t)llo * 3 + i;
        if constexpr (MODE == UPD_RENOISE) {
            sx[i] = alpha * lig_x[g] + c[5] * noise_x[g];
        } else {
            float u = lig_x[g] / alpha - var * eps_x[g] + sigma * noise_x[g];
            if constexpr (MODE == UPD_GUIDED) sxh[i] = (lig_x[g] - c[7] * eps_x[g]) / c[6];          // denoised position
            if constexpr (MODE == UPD_INPAINT || MODE == UPD_GUIDED) {
                if ((MODE == UPD_INPAINT || ia.fixed) && ia.fixed[llo + i / 3]) {
                    const float k0 = (ia.known_x[g] - ia.kp_com0[3 * b + i % 3]) + s_frame[i % 3];   // this order: see kpd.h
                    u = c[3] * k0 + c[4] * ia.known_noise_x[g];
                }
            }
            sx[i] = u;
        }
    }
    for (int i = tid; i < nl * atom_nf; i += blockDim.x) {
        const size_t g = (size_t)llo * atom_nf + i;
        if constexpr (MODE == UPD_RENOISE) {
            lig_h[g] = alpha * lig_h[g] + c[5] * noise_h[g];
        } else {
            float u = lig_h[g] / alpha - var * eps_h[g] + sigma * noise_h[g];
            if constexpr (MODE == UPD_INPAINT || MODE == UPD_GUIDED) {
                if ((MODE == UPD_INPAINT || ia.fixed) && ia.fixed[llo + i / atom_nf]) u = c[3] * ia.known_h[g] + c[4] * ia.known_noise_h[g];
            }
            lig_h[g] = u;
        }
    }
    __syncthreads();
    if constexpr (MODE == UPD_GUIDED) {
        // shift: one wavefront per free ligand atom against this complex's wall.  A complex without wall atoms or with w = 0
        // skips the loop, a component on which no pair pushes is not written: both keep the bits of the candidate.
        const int wlo = ga.wall_ptr[b], nw = ga.wall_ptr[b + 1] - wlo;
        const float wgt = c[8];
        if (nw > 0 && wgt != 0.0f) {
            const int w = tid >> 6, lane = tid & 63;
            const float o0[3] = {ga.kp_com0[3 * b], ga.kp_com0[3 * b + 1], ga.kp_com0[3 * b + 2]};
            const float o1[3] = {s_frame[0], s_frame[1], s_frame[2]};
            for (int i = w; i < nl; i += (int)(blockDim.x >> 6)) {
                if (ia.fixed && ia.fixed[llo + i]) continue;
                const PairSums p = hinge_pairs(sxh[3 * i], sxh[3 * i + 1], sxh[3 * i + 2], ga.wall_x, wlo, nw, o0, o1, ga.threshold, lane);
                if (lane == 0) {                     // a component without force keeps its bits (p.n also counts coincident pairs)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (p.f[k] != 0.0f) sx[3 * i + k] += wgt * p.f[k];
                }
            }
        }
        __syncthreads();
    }
    if (tid < 3) {
        float s = 0.0f;
        for (int i = 0; i < nl; ++i) s += sx[3 * i + tid];
        s_com[tid] = s / (float)nl;
    }
    __syncthreads();
    for (int i = tid; i < nl * 3; i += blockDim.x) lig_x[(size_t)llo * 3 + i] = sx[i] - s_com[i % 3];
    for (int i = tid; i < nk * 3; i += blockDim.x) kp_x[(size_t)klo * 3 + i] -= s_com[i % 3];
}

// coef[b] = {alpha_t_given_s, var_terms, sigma}
__global__ __launch_bounds__(256) void k_sample_update(const int *__restrict__ lig_ptr, const int *__restrict__ kp_ptr,
                                                       int atom_nf, float *__restrict__ lig_x, float *__restrict__ lig_h,
                                                       float *__restrict__ kp_x, const float *__restrict__ eps_x,
                                                       const float *__restrict__ eps_h, const float *__restrict__ noise_x,
                                                       const float *__restrict__ noise_h, const float *__restrict__ coef) {
    extern __shared__ float sx[];          // [3 * n_lig of this complex]
    __shared__ float s_com[3];
    update_and_center<UPD_PLAIN>(lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h,
                                 coef + 3 * blockIdx.x, InpaintArgs{}, sx, s_com, nullptr);
}

// Replacement conditioning: fixed atoms take the noised known part instead of the candidate.  coef6[b] = {alpha_t|s, var_terms,
// sigma, alpha_s, sigma_s, sigma_t|s} (k_inpaint_coef).
__global__ __launch_bounds__(256) void k_sample_update_inpaint(const int *__restrict__ lig_ptr, const int *__restrict__ kp_ptr,
                                                               int atom_nf, float *__restrict__ lig_x, float *__restrict__ lig_h,
                                                               float *__restrict__ kp_x, const float *__restrict__ eps_x,
                                                               const float *__restrict__ eps_h, const float *__restrict__ noise_x,
                                                               const float *__restrict__ noise_h, const float *__restrict__ coef6,
                                                               InpaintArgs ia) {
    extern __shared__ float sx[];
    __shared__ float s_com[3], s_frame[3];
    update_and_center<UPD_INPAINT>(lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h,
                                   coef6 + 6 * blockIdx.x, ia, sx, s_com, s_frame);
}

// Clash guidance: the candidate's positions are shifted by w F, F = the squared-hinge force of the wall atoms on the denoised
// positions (include/kpd.h, "Clash guidance").  coef9[b] = the six of k_sample_update_inpaint, then {alpha_t, sigma_t, w}
// (k_guided_coef).  ia.fixed == nullptr: no inpainting mask.  Dynamic LDS: [3 * max_lig] new positions, [3 * max_lig] x-hat.
__global__ __launch_bounds__(256) void k_sample_update_guided(const int *__restrict__ lig_ptr, const int *__restrict__ kp_ptr,
                                                              int atom_nf, float *__restrict__ lig_x, float *__restrict__ lig_h,
                                                              float *__restrict__ kp_x, const float *__restrict__ eps_x,
                                                              const float *__restrict__ eps_h, const float *__restrict__ noise_x,
                                                              const float *__restrict__ noise_h, const float *__restrict__ coef9,
                                                              InpaintArgs ia, GuideArgs ga, int max_lig) {
    extern __shared__ float sx[];
    __shared__ float s_com[3], s_frame[3];
    update_and_center<UPD_GUIDED>(lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h,
                                  coef9 + 9 * blockIdx.x, ia, sx, s_com, s_frame, ga, sx + (size_t)3 * max_lig);
}

// The report on finished samples: per complex {1/2 sum (threshold - d)+^2, pairs under the threshold, smallest distance}.  Wave w
// takes the ligand atoms w, w + 4, ... in that order, each through hinge_pairs; the four wave sums are added in wave order.
__global__ __launch_bounds__(256) void k_clash_score(const int *__restrict__ lig_ptr, const float *__restrict__ lig_x,
                                                     const int *__restrict__ wall_ptr, const float *__restrict__ wall_x,
                                                     float threshold, float *__restrict__ out) {
    __shared__ float s_e[4], s_d[4];
    __shared__ int s_n[4];
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int llo = lig_ptr[b], nl = lig_ptr[b + 1] - llo;
    const int wlo = wall_ptr[b], nw = wall_ptr[b + 1] - wlo;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float e = 0.0f, dmin = __builtin_inff();
    int n = 0;
    for (int i = w; i < nl; i += 4) {
        const float *p = lig_x + (size_t)(llo + i) * 3;
        const PairSums a = hinge_pairs(p[0], p[1], p[2], wall_x, wlo, nw, zero, zero, threshold, lane);
        e += a.e;
        n += a.n;
        dmin = fminf(dmin, a.dmin);
    }
    if (lane == 0) s_e[w] = e, s_n[w] = n, s_d[w] = dmin;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[3 * b] = ((s_e[0] + s_e[1]) + s_e[2]) + s_e[3];
        out[3 * b + 1] = (float)(s_n[0] + s_n[1] + s_n[2] + s_n[3]);
        out[3 * b + 2] = fminf(fminf(s_d[0], s_d[1]), fminf(s_d[2], s_d[3]));
    }
}

// Back from s to t between two repetitions of a resampled step: z_t = alpha_t|s z_s + sigma_t|s n, then the COM removal.
__global__ __launch_bounds__(256) void k_sample_renoise(const int *__restrict__ lig_ptr, const int *__restrict__ kp_ptr, int atom_nf,
                                                        float *__restrict__ lig_x, float *__restrict__ lig_h, float *__restrict__ kp_x,
                                                        const float *__restrict__ noise_x, const float *__restrict__ noise_h,
                                                        const float *__restrict__ coef6) {
    extern __shared__ float sx[];
    __shared__ float s_com[3];
    update_and_center<UPD_RENOISE>(lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, nullptr, nullptr, noise_x, noise_h,
                                   coef6 + 6 * blockIdx.x, InpaintArgs{}, sx, s_com, nullptr);
}

// Per-complex coefficients of one reverse step from the noise-schedule table (ligand_diffuser.py:505-526, 654-690):
// gamma lookup at round(t T), sigma^2_t|s = -expm1(softplus(g_s) - softplus(g_t)), alpha_t|s = exp((softplus(g_s) -
// softplus(g_t)) / 2), sigma = sqrt(sigmoid(gamma)).  Replaces ~30 elementwise launches on B-element tensors.
__device__ __forceinline__ float softplusf_(float x) { return x > 20.0f ? x : log1pf(expf(x)); }   // torch default threshold

// {alpha_t|s, var_terms, sigma_step, alpha_s, sigma_s, sigma_t|s}: one body for both coefficient kernels, so the first three are the same bits
__device__ __forceinline__ void step_coef_row(const float *__restrict__ gamma, int n_gamma, float s, float t, float (&o)[6]) {
    const float T = (float)(n_gamma - 1);
    const int is = min(max((int)rintf(s * T), 0), n_gamma - 1), it = min(max((int)rintf(t * T), 0), n_gamma - 1);
    const float gs = gamma[is], gt = gamma[it];
    const float dsp = softplusf_(gs) - softplusf_(gt);
    const float sigma2_ts = -expm1f(dsp);
    const float alpha_ts = expf(0.5f * dsp);
    const float sig_s = sqrtf(1.0f / (1.0f + expf(-gs))), sig_t = sqrtf(1.0f / (1.0f + expf(-gt)));
    o[0] = alpha_ts;
    o[1] = sigma2_ts / alpha_ts / sig_t;
    o[2] = sqrtf(sigma2_ts) * sig_s / sig_t;
    o[3] = sqrtf(1.0f / (1.0f + expf(gs)));            // alpha_s = sqrt(sigmoid(-gamma_s))
    o[4] = sig_s;
    o[5] = sqrtf(sigma2_ts);
}

template <int W>
__global__ void k_step_coef(const float *__restrict__ gamma, int n_gamma, const float *__restrict__ s,
                            const float *__restrict__ t, int B, float *__restrict__ coef) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float o[6];
    step_coef_row(gamma, n_gamma, s[b], t[b], o);
#pragma unroll
    for (int i = 0; i < W; ++i) coef[W * b + i] = o[i];
}

// coef9[b] = the row of k_step_coef<6> (the same body, so the same bits), then alpha_t, sigma_t and the guidance weight
// w = scale alpha_s sigma^2_t|s / sigma_t^2 (the weight of x-hat in the posterior mean) for round(t T) <= round(t_max T), else 0.
__global__ void k_guided_coef(const float *__restrict__ gamma, int n_gamma, const float *__restrict__ s, const float *__restrict__ t,
                              int B, float scale, float t_max, float *__restrict__ coef9) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float o[6];
    step_coef_row(gamma, n_gamma, s[b], t[b], o);
#pragma unroll
    for (int i = 0; i < 6; ++i) coef9[9 * b + i] = o[i];
    const float T = (float)(n_gamma - 1);
    const int is = min(max((int)rintf(s[b] * T), 0), n_gamma - 1), it = min(max((int)rintf(t[b] * T), 0), n_gamma - 1);
    const float gs = gamma[is], gt = gamma[it];
    const float sigma2_ts = -expm1f(softplusf_(gs) - softplusf_(gt));
    const float sig2_t = 1.0f / (1.0f + expf(-gt));
    coef9[9 * b + 6] = sqrtf(1.0f / (1.0f + expf(gt)));
    coef9[9 * b + 7] = sqrtf(sig2_t);
    coef9[9 * b + 8] = it <= (int)rintf(t_max * T) ? scale * o[3] * sigma2_ts / sig2_t : 0.0f;
}

// ---- per-complex counter-based noise ------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11) keyed by (seed, complex id), counter = (element quad within the complex, step,
// tag); Box-Muller on the four 32-bit outputs.  The value of an element depends only on (seed, complex id, step, tag,
// position inside the complex), never on which batch or rank the complex was placed in, so a sharded run reproduces the
// single-process run.  The reference draws one global torch.randn over the batch (ligand_diffuser.py:367,
// 530-531); this is the opt-in replacement, torch.randn stays the default.

__global__ void k_complex_noise(const int *__restrict__ ptr, int B, int width, const long long *__restrict__ complex_id,
                                unsigned long long seed, int step, int tag, float *__restrict__ out) {
    const int b = blockIdx.x;
    const int lo = ptr[b], n = (ptr[b + 1] - lo) * width;
    const unsigned long long cid = (unsigned long long)complex_id[b];
    const unsigned k0 = (unsigned)seed ^ (unsigned)cid, k1 = (unsigned)(seed >> 32) ^ (unsigned)(cid >> 32) ^ 0x5bd1e995u;
    float *o = out + (size_t)lo * width;
    for (int quad = threadIdx.x; 4 * quad < n; quad += blockDim.x) {
        unsigned c[4] = {(unsigned)quad, (unsigned)step, (unsigned)tag, 0u};
        philox4x32_10(c, k0, k1);
        float z[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);        // (0, 1)
            const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            const float r = sqrtf(-2.0f * logf(u1));
            float sn, cs;
            sincosf(6.283185307179586f * u2, &sn, &cs);
            z[2 * h] = r * cs;
            z[2 * h + 1] = r * sn;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * quad + i < n) o[4 * quad + i] = z[i];
    }
}

}  // namespace kpd

using namespace kpd;

extern "C" kpd_status kpd_complex_noise(int32_t B, const int32_t *node_ptr, int32_t width, const int64_t *complex_id, uint64_t seed,
                                        int32_t step, int32_t tag, float *out, void *stream) {
    KPD_REQUIRE(node_ptr && complex_id && out, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(B >= 1 && width >= 1, KPD_ERR_INVALID, "B=%d width=%d", B, width);
    hipLaunchKernelGGL(k_complex_noise, dim3(B), dim3(128), 0, static_cast<hipStream_t>(stream), node_ptr, B, width,
                       reinterpret_cast<const long long *>(complex_id), (unsigned long long)seed, step, tag, out);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_step_coefficients(const float *gamma, int32_t n_gamma, const float *s, const float *t, int32_t B,
                                            float *coef, void *stream) {
    KPD_REQUIRE(gamma && s && t && coef, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(n_gamma >= 2 && B >= 1, KPD_ERR_INVALID, "n_gamma=%d B=%d", n_gamma, B);
    hipLaunchKernelGGL(k_step_coef<3>, dim3(cdiv(B, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gamma, n_gamma, s, t, B,
                       coef);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_sample_update(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr, int32_t atom_nf,
                                        float *lig_x, float *lig_h, float *kp_x, const float *eps_x, const float *eps_h,
                                        const float *noise_x, const float *noise_h, const float *coef, int32_t max_lig,
                                        void *stream) {
    KPD_REQUIRE(lig_ptr && kp_ptr && lig_x && lig_h && kp_x && eps_x && eps_h && noise_x && noise_h && coef,
                KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(B >= 1 && max_lig >= 1 && max_lig <= 4096, KPD_ERR_INVALID, "B=%d max_lig=%d", B, max_lig);
    hipLaunchKernelGGL(k_sample_update, dim3(B), dim3(256), (size_t)max_lig * 3 * sizeof(float),
                       static_cast<hipStream_t>(stream), lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h,
                       noise_x, noise_h, coef);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_inpaint_coefficients(const float *gamma, int32_t n_gamma, const float *s, const float *t, int32_t B,
                                               float *coef, void *stream) {
    KPD_REQUIRE(gamma && s && t && coef, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(n_gamma >= 2 && B >= 1, KPD_ERR_INVALID, "n_gamma=%d B=%d", n_gamma, B);
    hipLaunchKernelGGL(k_step_coef<6>, dim3(cdiv(B, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gamma, n_gamma, s, t, B,
                       coef);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_sample_update_inpaint(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr, int32_t atom_nf,
                                                float *lig_x, float *lig_h, float *kp_x, const float *eps_x, const float *eps_h,
                                                const float *noise_x, const float *noise_h, const float *coef6,
                                                const uint8_t *fixed, const float *known_x, const float *known_h,
                                                const float *kp_com0, const float *known_noise_x, const float *known_noise_h,
                                                int32_t max_lig, void *stream) {
    KPD_REQUIRE(lig_ptr && kp_ptr && lig_x && lig_h && kp_x && eps_x && eps_h && noise_x && noise_h && coef6 && fixed && known_x &&
                    known_h && kp_com0 && known_noise_x && known_noise_h,
                KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(B >= 1 && atom_nf >= 1 && max_lig >= 1 && max_lig <= 4096, KPD_ERR_INVALID, "B=%d atom_nf=%d max_lig=%d", B, atom_nf,
                max_lig);
    const InpaintArgs ia{fixed, known_x, known_h, kp_com0, known_noise_x, known_noise_h};
    hipLaunchKernelGGL(k_sample_update_inpaint, dim3(B), dim3(256), (size_t)max_lig * 3 * sizeof(float),
                       static_cast<hipStream_t>(stream), lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h,
                       coef6, ia);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_sample_renoise(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr, int32_t atom_nf, float *lig_x,
                                         float *lig_h, float *kp_x, const float *noise_x, const float *noise_h, const float *coef6,
                                         int32_t max_lig, void *stream) {
    KPD_REQUIRE(lig_ptr && kp_ptr && lig_x && lig_h && kp_x && noise_x && noise_h && coef6, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(B >= 1 && atom_nf >= 1 && max_lig >= 1 && max_lig <= 4096, KPD_ERR_INVALID, "B=%d atom_nf=%d max_lig=%d", B, atom_nf,
                max_lig);
    hipLaunchKernelGGL(k_sample_renoise, dim3(B), dim3(256), (size_t)max_lig * 3 * sizeof(float), static_cast<hipStream_t>(stream),
                       lig_ptr, kp_ptr, atom_nf, lig_x, lig_h, kp_x, noise_x, noise_h, coef6);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_guided_coefficients(const float *gamma, int32_t n_gamma, const float *s, const float *t, int32_t B,
                                              float scale, float t_max, float *coef9, void *stream) {
    KPD_REQUIRE(gamma && s && t && coef9, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(n_gamma >= 2 && B >= 1, KPD_ERR_INVALID, "n_gamma=%d B=%d", n_gamma, B);
    KPD_REQUIRE(scale >= 0.0f && t_max > 0.0f && t_max <= 1.0f, KPD_ERR_INVALID, "scale=%g (>= 0) t_max=%g (in (0, 1])", scale, t_max);
    hipLaunchKernelGGL(k_guided_coef, dim3(cdiv(B, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gamma, n_gamma, s, t, B,
                       scale, t_max, coef9);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_sample_update_guided(int32_t B, const int32_t *lig_ptr, const int32_t *kp_ptr, int32_t atom_nf,
                                               float *lig_x, float *lig_h, float *kp_x, const float *eps_x, const float *eps_h,
                                               const float *noise_x, const float *noise_h, const float *coef9,
                                               const uint8_t *fixed, const float *known_x, const float *known_h,
                                               const float *kp_com0, const float *known_noise_x, const float *known_noise_h,
                                               const int32_t *wall_ptr, const float *wall_x, float threshold, int32_t max_lig,
                                               void *stream) {
    KPD_REQUIRE(lig_ptr && kp_ptr && lig_x && lig_h && kp_x && eps_x && eps_h && noise_x && noise_h && coef9 && wall_ptr && kp_com0,
                KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!fixed || (known_x && known_h && known_noise_x && known_noise_h), KPD_ERR_INVALID,
                "a mask needs known_x, known_h, known_noise_x and known_noise_h");
    KPD_REQUIRE(B >= 1 && atom_nf >= 1 && max_lig >= 1 && max_lig <= 4096, KPD_ERR_INVALID, "B=%d atom_nf=%d max_lig=%d", B, atom_nf,
                max_lig);
    KPD_REQUIRE(threshold > 0.0f, KPD_ERR_INVALID, "threshold=%g must be positive", threshold);
    const InpaintArgs ia{fixed, known_x, known_h, kp_com0, known_noise_x, known_noise_h};
    const GuideArgs ga{wall_ptr, wall_x, kp_com0, threshold};
    const size_t lds = (size_t)max_lig * 6 * sizeof(float);
    if (lds > 65536) KPD_TRY(ensure_dynamic_lds(reinterpret_cast<const void *>(k_sample_update_guided), (int)lds));
    hipLaunchKernelGGL(k_sample_update_guided, dim3(B), dim3(256), lds, static_cast<hipStream_t>(stream), lig_ptr, kp_ptr, atom_nf,
                       lig_x, lig_h, kp_x, eps_x, eps_h, noise_x, noise_h, coef9, ia, ga, max_lig);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

extern "C" kpd_status kpd_clash_score(int32_t B, const int32_t *lig_ptr, const float *lig_x, const int32_t *wall_ptr, const float *wall_x,
                                      float threshold, float *out, void *stream) {
    KPD_REQUIRE(lig_ptr && lig_x && wall_ptr && out, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(B >= 1 && threshold > 0.0f, KPD_ERR_INVALID, "B=%d threshold=%g", B, threshold);
    hipLaunchKernelGGL(k_clash_score, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), lig_ptr, lig_x, wall_ptr, wall_x,
                       threshold, out);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}
