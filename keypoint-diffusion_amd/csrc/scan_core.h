// The library's exclusive scan: the workgroup-wide device function, and the single-workgroup kernel with its launcher that turn
// per-item counts into offsets (count, scan, fill: the graph builders, the trainers' source CSR, pockets, XYZ / SDF text, bonds).
// Integer sums only, so every result is exact whatever the block size.  Everything here is file-local to the including unit.
#pragma once
#include <type_traits>

#include "common.h"

namespace kpd {
namespace {

// exclusive prefix of v over a workgroup of THREADS threads, in thread order; total = sum over the workgroup.
// part: THREADS / 64 values of LDS.  Two barriers.  T: int or long long.
template <int THREADS, typename T>
__device__ __forceinline__ T block_exclusive(T v, T *part, T &total) {
    static_assert(THREADS % 64 == 0, "whole waves");
    static_assert(std::is_same<T, int>::value || std::is_same<T, long long>::value, "the shuffle must carry every bit of T");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(s, off);
        if (lane >= off) s += t;
    }
    __syncthreads();                    // part may still be read from the previous call
    if (lane == 63) part[w] = s;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) {
        const T p = part[k];
        if (k < w) base += p;
        total += p;
    }
    return base + s - v;
}

// The carry makes the chunks of the scan kernel a serial chain, and a chunk costs one global-load latency and two barriers whatever
// its width: the widest workgroup gives the fewest chunks (the trainers scan several thousand nodes), and its 16 partials are
// broadcast reads of LDS.  The tests place their batch sizes and node counts on the chunk edges of this value: change SCAN_T in
// tests/test_pocket_gpu.py and the 2070-atom batch of tests/test_recenc_train_gpu.py with it.
constexpr int SCAN_THREADS = 1024;

struct ScanNoEpilogue {
    template <typename T>
    __device__ void operator()(T) const {}
};

// single workgroup: ptr[i] = count[0] + .. + count[i - 1] for i <= n, summed in T_out; `also` (optional) receives ptr[0..n) too.
// A thread's count is loaded one chunk ahead (the first before anything else), so the load's latency runs beside the scan.
// count may alias also: every thread reads its own count[i], and nothing else, before it writes also[i], and no other thread
// touches entry i.  Thread 0 ends with epilogue(ptr[n]).
template <typename T_in, typename T_out, typename Epilogue>
__global__ void __launch_bounds__(SCAN_THREADS)
k_exclusive_scan(const T_in *count, int n, T_out *__restrict__ ptr, T_out *also, Epilogue epilogue) {
    __shared__ T_out part[SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    T_in next = tid < n ? count[tid] : T_in(0);
    T_out carry = 0;
    for (int base = 0; base < n; base += SCAN_THREADS) {
        const int i = base + tid;
        const T_out v = i < n ? (T_out)next : (T_out)0;
        if (i + SCAN_THREADS < n) next = count[i + SCAN_THREADS];
        T_out total;
        const T_out at = carry + block_exclusive<SCAN_THREADS>(v, part, total);
        if (i < n) {
            ptr[i] = at;
            if (also) also[i] = at;
        }
        carry += total;
    }
    if (tid == 0) {
        ptr[n] = carry;
        epilogue(carry);
    }
}

// one launch, for n == 0 too (ptr[0] = 0)
template <typename T_in, typename T_out, typename Epilogue = ScanNoEpilogue>
kpd_status exclusive_scan(hipStream_t st, const T_in *count, int n, T_out *ptr, T_out *also = nullptr, Epilogue epilogue = Epilogue()) {
    hipLaunchKernelGGL((k_exclusive_scan<T_in, T_out, Epilogue>), dim3(1), dim3(SCAN_THREADS), 0, st, count, n, ptr, also, epilogue);
    KPD_LAUNCH_CHECK();
    return KPD_OK;
}

}  // namespace
}  // namespace kpd
