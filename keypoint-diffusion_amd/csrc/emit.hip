// Output side of sampling: element decode and XYZ text of a batch of sampled ligands, on the device.
// Replaces, for the tensor -> text part, sample.py:66-90 (argmax over the feature columns, index -> element symbol) and
// utils.py:11-21 (write_xyz_file: "<n>\n\n" then one "<el> <x:.3f> <y:.3f> <z:.3f>\n" line per atom).  The text is
// byte-identical to what Python's float formatting prints: "%.3f" of the exact value of the fp32 coordinate, rounded
// half-to-even on the exact binary value (integer arithmetic below, no floating-point rounding involved).
// Byte work, HBM-bound and tiny: three launches per batch (lines, ligand offsets, compaction).
#include "common.h"
#include "emit_core.h"
#include "engine.h"
#include "scan_core.h"

namespace kpd {

constexpr int LINE_SLOT = 80;       // 2 symbol bytes + 3 x (space, sign, <= 16 integer digits, '.', 3 digits) + '\n' <= 72

// one thread per atom: argmax of the feature row (first maximum, torch.argmax on CPU), the atom's line into its slot
__global__ void k_emit_lines(const float *__restrict__ pos, const float *__restrict__ feat, int N, int F,
                             const unsigned *__restrict__ symbols, int *__restrict__ elem, char *__restrict__ slots,
                             int *__restrict__ len, int *__restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int best = argmax_first(feat + (size_t)i * F, F);
    elem[i] = best;
    char line[LINE_SLOT];
    int n = 0;
    const unsigned sym = symbols[best];             // up to 4 bytes, NUL-padded, little-endian
    for (int b = 0; b < 4; ++b) {
        const char c = (char)((sym >> (8 * b)) & 0xff);
        if (!c) break;
        line[n++] = c;
    }
    for (int c = 0; c < 3; ++c) {
        line[n++] = ' ';
        const int w = format_fixed<3>(pos[(size_t)i * 3 + c], line + n);
        if (w < 0) {
            atomicOr(status, 1);
            line[n++] = '?';
        } else {
            n += w;
        }
    }
    line[n++] = '\n';
    len[i] = n;
    char *dst = slots + (size_t)i * LINE_SLOT;
    for (int b = 0; b < n; ++b) dst[b] = line[b];
}

__device__ __forceinline__ int header_len(int n) {
    int d = 1;
    for (int v = n; v >= 10; v /= 10) ++d;
    return d + 2;
}

// one wave per ligand: bytes of its block = header + lines
__global__ void k_emit_ligand_len(const int *__restrict__ lig_ptr, int B, const int *__restrict__ len, long long *__restrict__ lig_len) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const int a0 = lig_ptr[b], a1 = lig_ptr[b + 1];
    long long s = 0;
    for (int i = a0 + lane; i < a1; i += 64) s += len[i];
    for (int off = 32; off; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) lig_len[b] = s + header_len(a1 - a0);
}

// one workgroup per ligand: header, then every line at its offset (in-block scan of the line lengths)
__global__ void k_emit_compact(const int *__restrict__ lig_ptr, const int *__restrict__ len, const char *__restrict__ slots,
                               const long long *__restrict__ text_ptr, long long capacity, char *__restrict__ text,
                               int *__restrict__ status) {
    __shared__ int part[256 / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int a0 = lig_ptr[b], a1 = lig_ptr[b + 1], n = a1 - a0;
    const long long t0 = text_ptr[b];
    if (text_ptr[b + 1] > capacity) {
        if (tid == 0) atomicOr(status, 2);
        return;
    }
    const int hl = header_len(n);
    if (tid == 0) {
        int v = n;
        for (int d = hl - 3; d >= 0; --d) {
            text[t0 + d] = (char)('0' + v % 10);
            v /= 10;
        }
        text[t0 + hl - 2] = '\n';
        text[t0 + hl - 1] = '\n';
    }
    int carry = hl;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const int v = i < n ? len[a0 + i] : 0;
        int total;
        const int at = carry + block_exclusive<256>(v, part, total);
        if (i < n) {
            char *dst = text + t0 + at;
            const char *src = slots + (size_t)(a0 + i) * LINE_SLOT;
            for (int k = 0; k < v; ++k) dst[k] = src[k];
        }
        carry += total;
    }
}

}  // namespace kpd

using namespace kpd;

// a line slot and its length for every atom, the bytes of every ligand's block
struct XyzScratch {
    int n_atoms, B;
    char *slots = nullptr;
    int *len = nullptr;
    long long *lig_len = nullptr;
    void operator()(Carve &c) { c(slots, (size_t)n_atoms * LINE_SLOT); c(len, n_atoms); c(lig_len, B); }
};

extern "C" int64_t kpd_xyz_scratch_bytes(int32_t n_atoms, int32_t B) {
    if (n_atoms < 0 || B < 0) return -1;
    XyzScratch s{n_atoms, B};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_xyz_emit(const float *pos, const float *feat, const int32_t *lig_ptr, int32_t n_atoms, int32_t B,
                                   int32_t F, const uint32_t *symbols, int32_t *elem, uint8_t *text, int64_t capacity,
                                   int64_t *text_ptr, int32_t *status, void *scratch, void *stream) {
    KPD_REQUIRE(n_atoms >= 0 && B >= 0 && F >= 1 && capacity >= 0, KPD_ERR_INVALID, "n_atoms=%d B=%d F=%d capacity=%lld", n_atoms, B,
                F, (long long)capacity);
    KPD_REQUIRE(lig_ptr && text_ptr && status && scratch, KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_atoms || (pos && feat && symbols && elem), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!capacity || text, KPD_ERR_INVALID, "null text buffer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    KPD_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    XyzScratch s{n_atoms, B};
    carve_raw(static_cast<char *>(scratch), s);
    char *slots = s.slots;
    int *len = s.len;
    long long *lig_len = s.lig_len;
    if (n_atoms) {
        hipLaunchKernelGGL(k_emit_lines, dim3(cdiv(n_atoms, 256)), dim3(256), 0, st, pos, feat, n_atoms, F, symbols, elem, slots, len,
                           status);
        KPD_LAUNCH_CHECK();
    }
    if (B) {
        hipLaunchKernelGGL(k_emit_ligand_len, dim3(cdiv(B, 4)), dim3(256), 0, st, lig_ptr, B, len, lig_len);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, lig_len, B, reinterpret_cast<long long *>(text_ptr)));
    if (B) {
        hipLaunchKernelGGL(k_emit_compact, dim3(B), dim3(256), 0, st, lig_ptr, len, slots,
                           reinterpret_cast<const long long *>(text_ptr), (long long)capacity, reinterpret_cast<char *>(text), status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
