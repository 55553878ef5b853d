// Receptor-ligand distance hinge (losses/dist_hinge_loss.py, called per complex by models/ligand_diffuser.py:137-156) for a whole batch:
//   loss_s = sum_{i in A_s, j in B_s} max(thr - ||a_i - b_j||, 0)          (cross mode)
//   loss_s = sum_{i < j in A_s}       max(thr - ||a_i - a_j||, 0)          (self mode, B = A)
// and its gradients with respect to A and B.  Upstream runs one torch.cdist + an elementwise chain per complex behind a Python loop.
//
// VALU work.  One workgroup (256 lanes) per segment; every row of the segment's "row side" X is owned by a group of L consecutive lanes
// (L = 16 when the other side Y has more than 64 points, else 4; chosen from the segment's own sizes), lane l of the group takes
// Y points l, l + L, l + 2L, ...  Y is staged through LDS in chunks of HINGE_CH points.  Per pair the exact difference form is used:
// d = sqrt(dx^2 + dy^2 + dz^2), h = thr - d, weight w = 1 for h > 0 and 0.5 for h == 0 (torch.max splits the gradient at a tie), no
// gradient at d == 0.  The gradient of X row i, sum_j w (y_j - x_i) / d, is reduced over its L lanes with a fixed xor butterfly; the
// segment's loss is a per-lane running sum reduced over the workgroup in a fixed tree.  Nothing depends on the other segments or on
// the launch's shapes, so a segment's bits are the same alone or in any batch.  No atomics.
//
// Pass A: X = A, Y = B; writes the per-segment loss and (optionally) grad_a.  Pass B (cross mode, when grad_b is asked for): X = B, Y = A,
// gradient only -- the same pairs with the roles swapped, so each output row is written by exactly one lane.  A last one-block kernel
// sums the per-segment losses in index order into the total.
#include "common.h"

namespace kpd {

namespace {

constexpr int HINGE_BLOCK = 256;
constexpr int HINGE_CH = 1024;      // Y points per LDS chunk (12 KB)

__device__ __forceinline__ float block_sum_fixed(float v, float *red) {
    // fixed order: xor butterfly inside each wave64, then the four wave partials in wave order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// x / y: [n,3]; x_ptr / y_ptr: [S+1] (offsets are clamped into [0, n] so a bad offset array cannot read out of bounds).
// self_mode: Y = X and the loss counts pairs j > i only.
__global__ __launch_bounds__(HINGE_BLOCK) void k_hinge_rows(const float *__restrict__ x, const int32_t *__restrict__ x_ptr, int32_t n_x,
                                                            const float *__restrict__ y, const int32_t *__restrict__ y_ptr, int32_t n_y,
                                                            float thr, int self_mode, float *__restrict__ seg_loss,
                                                            float *__restrict__ grad_x) {
    __shared__ float sy[3][HINGE_CH];
    __shared__ float red[HINGE_BLOCK / 64];
    const int s = blockIdx.x;
    const int xa = min(max(x_ptr[s], 0), n_x), xb = min(max(x_ptr[s + 1], xa), n_x);
    const int ya = min(max(y_ptr[s], 0), n_y), yb = min(max(y_ptr[s + 1], ya), n_y);
    const int nx = xb - xa, ny = yb - ya;
    const int L = ny > 64 ? 16 : 4, groups = HINGE_BLOCK / L;
    const int grp = threadIdx.x / L, lane = threadIdx.x % L;
    const int npass = (nx + groups - 1) / groups, nchunk = (ny + HINGE_CH - 1) / HINGE_CH;
    float lsum = 0.0f;
    for (int p = 0; p < npass; ++p) {
        const int i = p * groups + grp;
        const bool valid = i < nx;
        float xi0 = 0.0f, xi1 = 0.0f, xi2 = 0.0f;
        if (valid) {
            xi0 = x[3 * (xa + i)];
            xi1 = x[3 * (xa + i) + 1];
            xi2 = x[3 * (xa + i) + 2];
        }
        float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
        for (int c = 0; c < nchunk; ++c) {
            const int c0 = c * HINGE_CH, cn = min(HINGE_CH, ny - c0);
            if (nchunk > 1 || p == 0) {          // block-uniform: every lane runs the same pass and chunk counts
                __syncthreads();
                for (int k = threadIdx.x; k < cn; k += HINGE_BLOCK) {
                    const float *q = y + 3 * (size_t)(ya + c0 + k);
                    sy[0][k] = q[0];
                    sy[1][k] = q[1];
                    sy[2][k] = q[2];
                }
                __syncthreads();
            }
            if (valid) {
                for (int k = lane; k < cn; k += L) {
                    const float dx = sy[0][k] - xi0, dy = sy[1][k] - xi1, dz = sy[2][k] - xi2;
                    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
                    const float h = thr - d;
                    if (!(h < 0.0f)) {                       // h >= 0, or NaN (propagated as upstream does)
                        if (!self_mode || c0 + k > i) lsum += h;
                        if (d > 0.0f) {
                            const float sc = (h > 0.0f ? 1.0f : 0.5f) / d;
                            g0 += sc * dx;
                            g1 += sc * dy;
                            g2 += sc * dz;
                        }
                    }
                }
            }
        }
        for (int o = L >> 1; o >= 1; o >>= 1) {            // the L lanes of a group are consecutive inside one wave
            g0 += __shfl_xor(g0, o);
            g1 += __shfl_xor(g1, o);
            g2 += __shfl_xor(g2, o);
        }
        if (valid && lane == 0 && grad_x) {
            float *q = grad_x + 3 * (size_t)(xa + i);
            q[0] = g0;
            q[1] = g1;
            q[2] = g2;
        }
    }
    if (seg_loss) {
        const float tot = block_sum_fixed(lsum, red);
        if (threadIdx.x == 0) seg_loss[s] = tot;
    }
}

__global__ __launch_bounds__(HINGE_BLOCK) void k_hinge_total(const float *__restrict__ seg_loss, int32_t S, float *__restrict__ total) {
    __shared__ float red[HINGE_BLOCK / 64];
    float v = 0.0f;
    for (int k = threadIdx.x; k < S; k += HINGE_BLOCK) v += seg_loss[k];
    const float tot = block_sum_fixed(v, red);
    if (threadIdx.x == 0) total[0] = tot;
}

}  // namespace

// include/kpd.h
extern "C" kpd_status kpd_dist_hinge(const float *a, const int32_t *a_ptr, int32_t n_a, const float *b, const int32_t *b_ptr, int32_t n_b, int32_t S,
                                     float threshold, float *seg_loss, float *total, float *grad_a, float *grad_b, void *stream) {
    const bool self_mode = b_ptr == nullptr;
    KPD_REQUIRE(S >= 0 && n_a >= 0 && n_b >= 0 && total && (S == 0 || seg_loss), KPD_ERR_INVALID,
                "kpd_dist_hinge: bad arguments (S=%d n_a=%d n_b=%d, seg_loss and total are required)", S, n_a, n_b);
    KPD_REQUIRE(S == 0 || (a_ptr && (n_a == 0 || a)), KPD_ERR_INVALID, "kpd_dist_hinge: a / a_ptr missing");
    KPD_REQUIRE(!self_mode || (b == nullptr && grad_b == nullptr), KPD_ERR_INVALID,
                "kpd_dist_hinge: self mode (b_ptr == NULL) takes no b and no grad_b");
    KPD_REQUIRE(self_mode || n_b == 0 || b, KPD_ERR_INVALID, "kpd_dist_hinge: b missing");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S > 0) {
        if (self_mode)
            hipLaunchKernelGGL(k_hinge_rows, dim3(S), dim3(HINGE_BLOCK), 0, st, a, a_ptr, n_a, a, a_ptr, n_a, threshold, 1, seg_loss, grad_a);
        else
            hipLaunchKernelGGL(k_hinge_rows, dim3(S), dim3(HINGE_BLOCK), 0, st, a, a_ptr, n_a, b, b_ptr, n_b, threshold, 0, seg_loss, grad_a);
        KPD_LAUNCH_CHECK();
        if (!self_mode && grad_b) {
            hipLaunchKernelGGL(k_hinge_rows, dim3(S), dim3(HINGE_BLOCK), 0, st, b, b_ptr, n_b, a, a_ptr, n_a, threshold, 0,
                               static_cast<float *>(nullptr), grad_b);
            KPD_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(k_hinge_total, dim3(1), dim3(HINGE_BLOCK), 0, st, seg_loss, S, total);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

}  // namespace kpd
