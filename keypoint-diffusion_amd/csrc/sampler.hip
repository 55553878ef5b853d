// Reverse-diffusion state update around the denoiser: the elementwise part of
// KeypointDiffusion.sample_p_zs_given_zt (models/ligand_diffuser.py:515-536) fused with the
// ligand-COM removal (remove_com :185-203).  One workgroup per complex; the new ligand
// coordinates are staged in LDS so the COM is a fixed-order sum (deterministic).
#include "engine.h"

namespace kpd {

// The three state updates of the sampler share this body, so the candidate expression and the COM removal are the same
// instructions in every one of them (FMA contraction cannot differ) and a complex without fixed atoms leaves the inpainting
// kernel with the bits of the plain one.  One workgroup per complex; sx [3 * n_lig of this complex] stages the new positions.
enum { UPD_PLAIN = 0, UPD_INPAINT = 1, UPD_RENOISE = 2 };

struct InpaintArgs {                        // UPD_INPAINT only (include/kpd.h has the algorithm)
    const unsigned char *fixed;             // [n_lig] 1 = this atom is given
    const float *known_x, *known_h;         // [n_lig,3] input frame, [n_lig,atom_nf] normalised; read on fixed rows only
    const float *kp_com0;                   // [B,3] keypoint mean in the input frame
    const float *known_noise_x, *known_noise_h;
};

// c = the coefficient row of this complex: {alpha_t|s, var, sigma_step} and, beyond UPD_PLAIN, {alpha_s, sigma_s, sigma_t|s}
template <int MODE>
__device__ __forceinline__ void update_and_center(const int *__restrict__ lig_ptr, const int *__restrict__ kp_ptr, int atom_nf,
                                                  float *__restrict__ lig_x, float *__restrict__ lig_h, float *__restrict__ kp_x,
                                                  const float *__restrict__ eps_x, const float *__restrict__ eps_h,
                                                  const float *__restrict__ noise_x, const float *__restrict__ noise_h,
                                                  const float *__restrict__ c, const InpaintArgs &ia, float *sx, float *s_com,
                                                  float *s_frame) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int llo = lig_ptr[b], nl = lig_ptr[b + 1] - llo;
    const int klo = kp_ptr[b], nk = kp_ptr[b + 1] - klo;
    const float alpha = c[0], var = c[1], sigma = c[2];

    if constexpr (MODE == UPD_INPAINT) {
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
            if constexpr (MODE == UPD_INPAINT) {
                if (ia.fixed[llo + i / 3]) {
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
            if constexpr (MODE == UPD_INPAINT) {
                if (ia.fixed[llo + i / atom_nf]) u = c[3] * ia.known_h[g] + c[4] * ia.known_noise_h[g];
            }
            lig_h[g] = u;
        }
    }
    __syncthreads();
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
