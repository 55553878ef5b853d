// Device routines shared by the text writers (emit.hip: XYZ, molecule.hip: SDF): the element decode and Python's
// fixed-point float formatting by exact integer arithmetic on the fp32 bit pattern.
#pragma once
#include "common.h"

namespace kpd {

// torch.argmax over one feature row on the CPU: the first maximum; a NaN is a maximum
__device__ __forceinline__ int argmax_first(const float *__restrict__ f, int F) {
    int best = 0;
    float bv = f[0];
    bool has_nan = bv != bv;
    for (int k = 1; k < F && !has_nan; ++k) {
        const float x = f[k];
        if (x != x) {
            best = k;
            has_nan = true;
        } else if (x > bv) {
            bv = x;
            best = k;
        }
    }
    return best;
}

// round_half_even(|v| * 10^DEC) of a finite fp32 value, exact; false if it does not fit 64-bit integers here
template <int DEC>
__device__ __forceinline__ bool fixed_scaled(unsigned bits, unsigned long long &N) {
    static_assert(DEC == 3 || DEC == 4, "scale");
    constexpr unsigned long long SCALE = DEC == 3 ? 1000ull : 10000ull;
    constexpr int EMAX = DEC == 3 ? 29 : 25;        // m * SCALE < 2^34 (2^38): the shifted value stays below 2^63
    const int e8 = (bits >> 23) & 0xff;
    const unsigned frac = bits & 0x7fffffu;
    const unsigned long long m = e8 ? (frac | 0x800000u) : frac;
    const int e = (e8 ? e8 : 1) - 150;              // value = m * 2^e
    const unsigned long long M = m * SCALE;
    if (e >= 0) {
        if (e > EMAX) return false;
        N = M << e;
    } else {
        const int s = -e;
        if (s >= 64) {
            N = 0;
        } else {
            const unsigned long long q = M >> s, r = M & ((1ull << s) - 1ull), half = 1ull << (s - 1);
            N = q + ((r > half || (r == half && (q & 1ull))) ? 1ull : 0ull);
        }
    }
    return true;
}

// "%.<DEC>f" of an fp32 value into buf; returns the length, or -1 if |v| >= 2^53 (2^49 for DEC = 4)
template <int DEC>
__device__ __forceinline__ int format_fixed(float v, char *buf) {
    constexpr unsigned long long SCALE = DEC == 3 ? 1000ull : 10000ull;
    const unsigned bits = __float_as_uint(v);
    const bool neg = bits >> 31;
    int n = 0;
    if (((bits >> 23) & 0xff) == 255) {             // Python: 'nan' without sign, 'inf' / '-inf'
        if (bits & 0x7fffffu) {
            buf[0] = 'n'; buf[1] = 'a'; buf[2] = 'n';
            return 3;
        }
        if (neg) buf[n++] = '-';
        buf[n++] = 'i'; buf[n++] = 'n'; buf[n++] = 'f';
        return n;
    }
    unsigned long long N;
    if (!fixed_scaled<DEC>(bits, N)) return -1;
    if (neg) buf[n++] = '-';                        // the sign survives rounding to zero ('-0.000'), as in Python
    unsigned long long ip = N / SCALE;
    unsigned fp = (unsigned)(N % SCALE);
    char tmp[20];
    int nd = 0;
    do {
        tmp[nd++] = (char)('0' + (int)(ip % 10ull));
        ip /= 10ull;
    } while (ip);
    while (nd) buf[n++] = tmp[--nd];
    buf[n++] = '.';
#pragma unroll
    for (unsigned div = (unsigned)(SCALE / 10ull); div; div /= 10u) {
        buf[n++] = (char)('0' + fp / div);
        fp %= div;
    }
    return n;
}

}  // namespace kpd
