// Pocket extraction on the device: from whole receptors + ligands to pocket atoms and interface points, for a batch.
// Replaces, for the array-level part, get_pocket_atoms (data_processing/pdbbind_processing.py:85-149), get_interface_points
// (:295-325) and the residue-wise selection of process_bindingmoad.py:124-204 / byop.py:119-197.  File parsing is
// structure_io.hip.  Every decision (d < cutoff, d < dist_thr, d >= excl_thr) is taken on squared distances computed in fp64 from
// direct differences of the fp32 coordinates: exact differences, no matmul form, so no wobble at the thresholds.
// Small latency-bound kernels: a complex is one workgroup (or one row of tiles in k_pocket_mark); nothing is shared between
// complexes, there are no float atomics, and results are bitwise independent of batch composition.
#include "common.h"
#include "engine.h"
#include "molecule_core.h"
#include "scan_core.h"

namespace kpd {

constexpr int PK_THREADS = 256;
constexpr int PK_MAX_LIG = 1024;        // ligand atoms held in LDS (the library's max_lig)
constexpr int IP_ITEMS = 4;             // (ligand, receptor) pairs per thread and enumeration step
constexpr int IP_MAX_POINTS = 4096;     // interface points of one complex held in LDS while thinning

enum : int { PK_EMPTY = 1, PK_CAPACITY = 2, PK_BAD_RES = 4, PK_BAD_SEGMENT = 8 };

// ligand of the complex into LDS; returns its size, or -1 if it does not fit
__device__ __forceinline__ int load_ligand(const float *__restrict__ lig_x, int l0, int l1, float *lig) {
    const int m = l1 - l0;
    if (m > PK_MAX_LIG) return -1;
    for (int i = threadIdx.x; i < m * 3; i += PK_THREADS) lig[i] = lig_x[(size_t)l0 * 3 + i];
    __syncthreads();
    return m;
}

// threshold^2 for "d < t" (never true for t <= 0) and "d >= t" (always true for t <= 0) on squared distances
__device__ __forceinline__ double below2(float t) { return t > 0.f ? (double)t * (double)t : -1.0; }
__device__ __forceinline__ double atleast2(float t) { return t > 0.f ? (double)t * (double)t : 0.0; }

__device__ __forceinline__ double dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by, dz = (double)az - (double)bz;
    return dx * dx + dy * dy + dz * dz;
}

// ---- 1. mark: box test, minimum ligand distance, residue flags ---------------------------------------------------
// grid (B, tiles of PK_THREADS receptor atoms).  in_box is written for every atom of a well-formed complex.
__global__ void __launch_bounds__(PK_THREADS)
k_pocket_mark(const float *__restrict__ rec_x, const int *__restrict__ rec_ptr, int n_rec, const int *__restrict__ res_idx,
              const uint8_t *__restrict__ probe, const float *__restrict__ lig_x, const int *__restrict__ lig_ptr, int n_lig,
              float box_padding, float pocket_cutoff, uint8_t *__restrict__ in_box, uint8_t *__restrict__ res_flag,
              int *__restrict__ status) {
    __shared__ float lig[PK_MAX_LIG * 3];
    __shared__ float red[PK_THREADS / 64][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    int a0, a1, l0, l1;
    const bool ok = mol_segment(rec_ptr, b, n_rec, a0, a1) && mol_segment(lig_ptr, b, n_lig, l0, l1);
    if (!ok || l1 - l0 > PK_MAX_LIG) {
        if (tid == 0 && blockIdx.y == 0) atomicOr(status + b, PK_BAD_SEGMENT);
        return;
    }
    if (a1 - a0 > (int)gridDim.y * PK_THREADS) {        // max_rec understated: the complex is left out, not half marked
        if (tid == 0 && blockIdx.y == 0) atomicOr(status + b, PK_BAD_SEGMENT);
        return;
    }
    if ((int)blockIdx.y * PK_THREADS >= a1 - a0) return;
    const int m = load_ligand(lig_x, l0, l1, lig);
    // padded bounding box, corners = fp32 min / max -+ padding (:92-97); a NaN ligand coordinate poisons its corner, as torch.min
    float lo[3], hi[3];
    const bool use_box = box_padding >= 0.f;
    if (use_box) {
        const float inf = __builtin_inff();
        float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
        bool nan[3] = {false, false, false};
        for (int j = tid; j < m; j += PK_THREADS)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = lig[j * 3 + c];
                mn[c] = fminf(mn[c], v);
                mx[c] = fmaxf(mx[c], v);
                nan[c] |= v != v;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (nan[c]) mn[c] = mx[c] = __builtin_nanf("");
            for (int off = 32; off; off >>= 1) {
                const float o1 = __shfl_xor(mn[c], off), o2 = __shfl_xor(mx[c], off);
                mn[c] = (mn[c] != mn[c] || o1 != o1) ? __builtin_nanf("") : fminf(mn[c], o1);
                mx[c] = (mx[c] != mx[c] || o2 != o2) ? __builtin_nanf("") : fmaxf(mx[c], o2);
            }
            if ((tid & 63) == 0) {
                red[tid >> 6][c] = mn[c];
                red[tid >> 6][3 + c] = mx[c];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float l = red[0][c], h = red[0][3 + c];
            for (int w = 1; w < PK_THREADS / 64; ++w) {
                const float o1 = red[w][c], o2 = red[w][3 + c];
                l = (l != l || o1 != o1) ? __builtin_nanf("") : fminf(l, o1);
                h = (h != h || o2 != o2) ? __builtin_nanf("") : fmaxf(h, o2);
            }
            lo[c] = l - box_padding;
            hi[c] = h + box_padding;
        }
    }
    const int i = a0 + (int)blockIdx.y * PK_THREADS + tid;
    if (i >= a1) return;
    const float x = rec_x[(size_t)i * 3], y = rec_x[(size_t)i * 3 + 1], z = rec_x[(size_t)i * 3 + 2];
    const bool inside = !use_box || (x >= lo[0] && y >= lo[1] && z >= lo[2] && x <= hi[0] && y <= hi[1] && z <= hi[2]);   // :114-117
    in_box[i] = inside;
    const int r = res_idx[i];
    if (r < 0 || r >= a1 - a0) {
        atomicOr(status + b, PK_BAD_RES);
        return;
    }
    if (!inside || !probe[i]) return;
    const double c2 = below2(pocket_cutoff);
    bool near = false;
    for (int j = 0; j < m && !near; ++j) near = dist2(x, y, z, lig[j * 3], lig[j * 3 + 1], lig[j * 3 + 2]) < c2;   // min d < cutoff (:127-128)
    if (near) res_flag[a0 + r] = 1;     // same-value race between the atoms of a residue: benign
}

__device__ __forceinline__ bool emitted(int i, int a0, int a1, const int *__restrict__ res_idx, const uint8_t *__restrict__ emit,
                                        const uint8_t *__restrict__ res_flag) {
    const int r = res_idx[i];
    return emit[i] && r >= 0 && r < a1 - a0 && res_flag[a0 + r];
}

// ---- 2a. count: by-residue mask, atoms emitted per complex, first emitted atom of every residue -----------------
__global__ void __launch_bounds__(PK_THREADS)
k_pocket_count(const int *__restrict__ rec_ptr, int n_rec, const int *__restrict__ res_idx, const uint8_t *__restrict__ emit,
               const uint8_t *__restrict__ res_flag, uint8_t *__restrict__ mask, int *__restrict__ first_atom,
               int *__restrict__ cnt, int *__restrict__ status) {
    __shared__ int part[PK_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int a0, a1;
    if (!mol_segment(rec_ptr, b, n_rec, a0, a1) || (status[b] & PK_BAD_SEGMENT)) {
        if (tid == 0) cnt[b] = 0;
        return;
    }
    int mine = 0;
    for (int i = a0 + tid; i < a1; i += PK_THREADS) {
        const bool e = emitted(i, a0, a1, res_idx, emit, res_flag);
        mask[i] = e;
        if (e) {
            atomicMin(first_atom + a0 + res_idx[i], i);         // integer minimum: the result does not depend on the order
            ++mine;
        }
    }
    int total;
    block_exclusive<PK_THREADS>(mine, part, total);
    if (tid == 0) {
        cnt[b] = total;
        if (!total) atomicOr(status + b, PK_EMPTY);
    }
}

// ---- 2b. compact: rows in ascending order, residue labels in order of first appearance ---------------------------
__global__ void __launch_bounds__(PK_THREADS)
k_pocket_compact(const int *__restrict__ rec_ptr, int n_rec, const int *__restrict__ res_idx, const uint8_t *__restrict__ emit,
                 const uint8_t *__restrict__ res_flag, const int *__restrict__ first_atom, int *__restrict__ res_rank,
                 const int *__restrict__ pocket_ptr, int cap_rows, int *__restrict__ rows, int *__restrict__ pocket_res,
                 int *__restrict__ status) {
    __shared__ int part[PK_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int a0, a1;
    if (!mol_segment(rec_ptr, b, n_rec, a0, a1) || (status[b] & PK_BAD_SEGMENT)) return;
    const int p0 = pocket_ptr[b], p1 = pocket_ptr[b + 1];
    if (p1 > cap_rows) {
        if (tid == 0 && p1 > p0) atomicOr(status + b, PK_CAPACITY);
        return;
    }
    int n_out = 0, n_res = 0;
    for (int base = a0; base < a1; base += PK_THREADS) {
        const int i = base + tid;
        const bool e = i < a1 && emitted(i, a0, a1, res_idx, emit, res_flag);
        const bool first = e && first_atom[a0 + res_idx[i]] == i;
        int total;
        const int packed = block_exclusive<PK_THREADS>((int)e | ((int)first << 16), part, total);     // both counts are <= 256 per step
        if (e) rows[p0 + n_out + (packed & 0xffff)] = i;
        if (first) res_rank[a0 + res_idx[i]] = n_res + (packed >> 16);
        n_out += total & 0xffff;
        n_res += total >> 16;
    }
    __syncthreads();                    // rows and res_rank of this complex were written by this workgroup
    for (int k = tid; k < p1 - p0; k += PK_THREADS) pocket_res[p0 + k] = res_rank[a0 + res_idx[rows[p0 + k]]];
}

// ---- 3. interface points ---------------------------------------------------------------------------------------
// One workgroup per complex: candidate receptor atoms in order -> candidate midpoints in torch.where order (ligand atom
// ascending, then receptor atom ascending) -> greedy thinning (:312-321), a chunk of PK_THREADS candidates at a time.
// The kept points are left at the front of the complex's candidate buffer; k_ip_gather places them at ip_ptr.
__global__ void __launch_bounds__(PK_THREADS)
k_ip_select(const float *__restrict__ rec_x, const int *__restrict__ rec_ptr, int n_rec, const uint8_t *__restrict__ cand_mask,
            const float *__restrict__ lig_x, const int *__restrict__ lig_ptr, int n_lig, float dist_thr, float excl_thr,
            int cap_cand, int *__restrict__ clist, float *__restrict__ cand, int *__restrict__ n_cand, int *__restrict__ n_pts,
            int *__restrict__ status) {
    __shared__ float lig[PK_MAX_LIG * 3];
    __shared__ float sel[IP_MAX_POINTS * 3];
    __shared__ float cm[PK_THREADS * 3];
    __shared__ int part[PK_THREADS / 64];
    __shared__ int wfirst[PK_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int a0, a1, l0, l1;
    const bool ok = mol_segment(rec_ptr, b, n_rec, a0, a1) && mol_segment(lig_ptr, b, n_lig, l0, l1);
    if (!ok || l1 - l0 > PK_MAX_LIG) {
        if (tid == 0) {
            status[b] = PK_BAD_SEGMENT;
            n_cand[b] = n_pts[b] = 0;
        }
        return;
    }
    const int m = load_ligand(lig_x, l0, l1, lig);
    int st = 0;
    // candidate receptor atoms, ascending
    int nc = 0;
    for (int base = a0; base < a1; base += PK_THREADS) {
        const int i = base + tid;
        const bool c = i < a1 && cand_mask[i];
        int total;
        const int ex = block_exclusive<PK_THREADS>((int)c, part, total);
        if (c) clist[a0 + nc + ex] = i;
        nc += total;
    }
    __syncthreads();
    // (a) candidate pairs: pair p = (ligand p / nc, candidate p % nc), IP_ITEMS consecutive pairs per thread
    float *mine = cand + (size_t)b * cap_cand * 3;
    const double t2 = below2(dist_thr);
    const long long n_pairs = (long long)m * nc;
    long long found = 0;
    for (long long base = 0; base < n_pairs; base += PK_THREADS * IP_ITEMS) {
        float mid[IP_ITEMS][3];
        bool hit[IP_ITEMS];
        int k = 0;
#pragma unroll
        for (int it = 0; it < IP_ITEMS; ++it) {
            const long long p = base + (long long)tid * IP_ITEMS + it;
            hit[it] = false;
            if (p < n_pairs) {
                const int l = (int)(p / nc), r = clist[a0 + (int)(p % nc)];
                const float lx = lig[l * 3], ly = lig[l * 3 + 1], lz = lig[l * 3 + 2];
                const float rx = rec_x[(size_t)r * 3], ry = rec_x[(size_t)r * 3 + 1], rz = rec_x[(size_t)r * 3 + 2];
                hit[it] = dist2(lx, ly, lz, rx, ry, rz) < t2;                    // :306
                mid[it][0] = (lx + rx) * 0.5f;                                   // :308, bitwise (a + b) / 2
                mid[it][1] = (ly + ry) * 0.5f;
                mid[it][2] = (lz + rz) * 0.5f;
                k += hit[it];
            }
        }
        int total;
        long long slot = found + block_exclusive<PK_THREADS>(k, part, total);
#pragma unroll
        for (int it = 0; it < IP_ITEMS; ++it) {
            if (!hit[it]) continue;
            if (slot < cap_cand) {
                mine[slot * 3] = mid[it][0];
                mine[slot * 3 + 1] = mid[it][1];
                mine[slot * 3 + 2] = mid[it][2];
            }
            ++slot;
        }
        found += total;
    }
    if (found == 0) st |= PK_EMPTY;
    if (found > cap_cand) st |= PK_CAPACITY;
    const int stored = (int)(found < cap_cand ? found : cap_cand);
    __syncthreads();                    // the candidate buffer of this complex was written by this workgroup
    // (b) greedy thinning
    const double e2 = atleast2(excl_thr);
    int ns = 0;
    bool full = false;
    for (int base = 0; base < stored && !full; base += PK_THREADS) {
        const int c = base + tid;
        bool alive = c < stored;
        float x = 0.f, y = 0.f, z = 0.f;
        if (alive) {
            x = mine[(size_t)c * 3];
            y = mine[(size_t)c * 3 + 1];
            z = mine[(size_t)c * 3 + 2];
            cm[tid * 3] = x;
            cm[tid * 3 + 1] = y;
            cm[tid * 3 + 2] = z;
            for (int j = 0; j < ns && alive; ++j) alive = dist2(x, y, z, sel[j * 3], sel[j * 3 + 1], sel[j * 3 + 2]) >= e2;   // :319-320
        }
        for (;;) {                      // resolve the chunk in order: the first survivor is kept, later survivors test against it
            const unsigned long long bal = __ballot(alive);
            __syncthreads();            // wfirst of the previous turn has been read; cm is complete
            if (lane == 0) wfirst[w] = bal ? w * 64 + __ffsll((long long)bal) - 1 : PK_THREADS;
            __syncthreads();
            int f = PK_THREADS;
#pragma unroll
            for (int k = 0; k < PK_THREADS / 64; ++k) f = min(f, wfirst[k]);
            if (f == PK_THREADS) break;
            if (ns == IP_MAX_POINTS) {
                full = true;
                break;
            }
            const float fx = cm[f * 3], fy = cm[f * 3 + 1], fz = cm[f * 3 + 2];
            if (tid == f) {
                sel[ns * 3] = fx;
                sel[ns * 3 + 1] = fy;
                sel[ns * 3 + 2] = fz;
                alive = false;
            } else if (alive && tid > f) {
                alive = dist2(x, y, z, fx, fy, fz) >= e2;
            }
            ++ns;
        }
        __syncthreads();                // sel is complete before the next chunk tests against it
    }
    if (full) st |= PK_CAPACITY;
    __syncthreads();
    for (int k = tid; k < ns * 3; k += PK_THREADS) mine[k] = sel[k];     // ns <= stored <= cap_cand
    if (tid == 0) {
        n_cand[b] = (int)(found < 0x7fffffff ? found : 0x7fffffff);
        n_pts[b] = ns;
        status[b] = st;
    }
}

__global__ void __launch_bounds__(PK_THREADS)
k_ip_gather(const float *__restrict__ cand, int cap_cand, const int *__restrict__ ip_ptr, int cap_points, float *__restrict__ points,
            int *__restrict__ status) {
    const int b = blockIdx.x;
    const int p0 = ip_ptr[b], p1 = ip_ptr[b + 1];
    if (p1 > cap_points) {
        if (threadIdx.x == 0 && p1 > p0) atomicOr(status + b, PK_CAPACITY);
        return;
    }
    const float *src = cand + (size_t)b * cap_cand * 3;
    for (int k = threadIdx.x; k < (p1 - p0) * 3; k += PK_THREADS) points[(size_t)p0 * 3 + k] = src[k];
}

}  // namespace kpd

using namespace kpd;

// residue flags, first emitted atom and rank of every residue, atoms emitted per complex
struct PocketScratch {
    int n_rec, B;
    uint8_t *res_flag = nullptr;
    int *first_atom = nullptr, *res_rank = nullptr, *cnt = nullptr;
    void operator()(Carve &c) { c(res_flag, n_rec); c(first_atom, n_rec); c(res_rank, n_rec); c(cnt, B); }
};

extern "C" int64_t kpd_pocket_scratch_bytes(int32_t n_rec, int32_t B) {
    if (n_rec < 0 || B < 0) return -1;
    PocketScratch s{n_rec, B};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_pocket_select(const float *rec_x, const int32_t *rec_ptr, const int32_t *res_idx, const uint8_t *probe,
                                        const uint8_t *emit, int32_t n_rec, int32_t max_rec, const float *lig_x,
                                        const int32_t *lig_ptr, int32_t n_lig, int32_t B, float box_padding, float pocket_cutoff,
                                        int32_t cap_rows, uint8_t *in_box, uint8_t *pocket_mask, int32_t *rows, int32_t *pocket_res,
                                        int32_t *pocket_ptr, int32_t *status, void *scratch, void *stream) {
    KPD_REQUIRE(n_rec >= 0 && max_rec >= 0 && max_rec <= n_rec && n_lig >= 0 && B >= 0 && cap_rows >= 0, KPD_ERR_INVALID,
                "n_rec=%d max_rec=%d n_lig=%d B=%d cap_rows=%d", n_rec, max_rec, n_lig, B, cap_rows);
    KPD_REQUIRE(rec_ptr && lig_ptr && pocket_ptr && scratch && (!B || status), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_rec || (rec_x && res_idx && probe && emit && in_box && pocket_mask), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_lig || lig_x, KPD_ERR_INVALID, "null ligand coordinates");
    KPD_REQUIRE(!cap_rows || (rows && pocket_res), KPD_ERR_INVALID, "null output");
    KPD_REQUIRE(pocket_cutoff == pocket_cutoff && box_padding == box_padding, KPD_ERR_INVALID, "NaN threshold");
    hipStream_t st = static_cast<hipStream_t>(stream);
    PocketScratch s{n_rec, B};
    carve_raw(static_cast<char *>(scratch), s);
    uint8_t *res_flag = s.res_flag;
    int *first_atom = s.first_atom, *res_rank = s.res_rank, *cnt = s.cnt;
    if (n_rec) {
        KPD_HIP(hipMemsetAsync(res_flag, 0, (size_t)n_rec, st));
        KPD_HIP(hipMemsetAsync(first_atom, 0x7f, (size_t)n_rec * 4, st));
        KPD_HIP(hipMemsetAsync(in_box, 0, (size_t)n_rec, st));           // rows outside every segment read as 0
        KPD_HIP(hipMemsetAsync(pocket_mask, 0, (size_t)n_rec, st));
    }
    if (B) {
        KPD_HIP(hipMemsetAsync(status, 0, (size_t)B * 4, st));
        if (max_rec) {
            hipLaunchKernelGGL(k_pocket_mark, dim3(B, cdiv(max_rec, PK_THREADS)), dim3(PK_THREADS), 0, st, rec_x, rec_ptr, n_rec, res_idx,
                               probe, lig_x, lig_ptr, n_lig, box_padding, pocket_cutoff, in_box, res_flag, status);
            KPD_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_pocket_count, dim3(B), dim3(PK_THREADS), 0, st, rec_ptr, n_rec, res_idx, emit, res_flag, pocket_mask,
                           first_atom, cnt, status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, cnt, B, pocket_ptr));
    if (B) {
        hipLaunchKernelGGL(k_pocket_compact, dim3(B), dim3(PK_THREADS), 0, st, rec_ptr, n_rec, res_idx, emit, res_flag, first_atom,
                           res_rank, pocket_ptr, cap_rows, rows, pocket_res, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}

// candidate receptor atoms, candidate midpoints of every complex, points kept per complex
struct InterfaceScratch {
    int n_rec, B, cap_cand;
    int *clist = nullptr, *n_pts = nullptr;
    float *cand = nullptr;
    void operator()(Carve &c) { c(clist, n_rec); c(cand, (size_t)B * cap_cand * 3); c(n_pts, B); }
};

extern "C" int64_t kpd_interface_points_scratch_bytes(int32_t n_rec, int32_t B, int32_t cap_cand) {
    if (n_rec < 0 || B < 0 || cap_cand < 0) return -1;
    InterfaceScratch s{n_rec, B, cap_cand};
    return scratch_bytes(s);
}

extern "C" kpd_status kpd_interface_points(const float *rec_x, const int32_t *rec_ptr, const uint8_t *cand_mask, int32_t n_rec,
                                           const float *lig_x, const int32_t *lig_ptr, int32_t n_lig, int32_t B, float dist_thr,
                                           float excl_thr, int32_t cap_cand, int32_t cap_points, float *points, int32_t *ip_ptr,
                                           int32_t *n_cand, int32_t *status, void *scratch, void *stream) {
    KPD_REQUIRE(n_rec >= 0 && n_lig >= 0 && B >= 0 && cap_cand >= 0 && cap_points >= 0, KPD_ERR_INVALID,
                "n_rec=%d n_lig=%d B=%d cap_cand=%d cap_points=%d", n_rec, n_lig, B, cap_cand, cap_points);
    KPD_REQUIRE((long long)B * cap_cand <= 0x7fffffffLL / 3, KPD_ERR_INVALID, "B * cap_cand = %lld candidates do not fit int32 indexing",
                (long long)B * cap_cand);
    KPD_REQUIRE(rec_ptr && lig_ptr && ip_ptr && scratch && (!B || (status && n_cand)), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_rec || (rec_x && cand_mask), KPD_ERR_INVALID, "null argument");
    KPD_REQUIRE(!n_lig || lig_x, KPD_ERR_INVALID, "null ligand coordinates");
    KPD_REQUIRE(!cap_points || points, KPD_ERR_INVALID, "null output");
    KPD_REQUIRE(dist_thr == dist_thr && excl_thr == excl_thr, KPD_ERR_INVALID, "NaN threshold");
    hipStream_t st = static_cast<hipStream_t>(stream);
    InterfaceScratch s{n_rec, B, cap_cand};
    carve_raw(static_cast<char *>(scratch), s);
    int *clist = s.clist, *n_pts = s.n_pts;
    float *cand = s.cand;
    if (B) {
        hipLaunchKernelGGL(k_ip_select, dim3(B), dim3(PK_THREADS), 0, st, rec_x, rec_ptr, n_rec, cand_mask, lig_x, lig_ptr, n_lig, dist_thr,
                           excl_thr, cap_cand, clist, cand, n_cand, n_pts, status);
        KPD_LAUNCH_CHECK();
    }
    KPD_TRY(exclusive_scan(st, n_pts, B, ip_ptr));
    if (B) {
        hipLaunchKernelGGL(k_ip_gather, dim3(B), dim3(PK_THREADS), 0, st, cand, cap_cand, ip_ptr, cap_points, points, status);
        KPD_LAUNCH_CHECK();
    }
    return KPD_OK;
}
