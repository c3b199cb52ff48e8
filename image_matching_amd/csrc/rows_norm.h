// image_matching_amd/csrc/rows_norm.h — the scalar arithmetic of templates that arrive in device memory: the exact widening of an
// f16 / bf16 / f32 bit pattern to a double and the L2 normalisation of a row (shared by k_rows_widen in client_kernels.hip, by
// normalize() in client.cpp and, on the host, by tests/csrc/rows_norm_check.cpp, which checks them against numpy and the oracle).
//
// The widenings work on the bit patterns with integer arithmetic only, so that host and device cannot differ (no conversion
// instruction, no denormal mode): a normal number is re-biased, a subnormal is its integer mantissa times a power of two (exact in
// a double), infinities and NaNs keep their sign and their mantissa bits.
// The normalisation is VectorUtils::plaintextNormalize as client.cpp has always computed it: m = 0; m += x[i] * x[i] in index order,
// product and sum rounded separately (the build uses -ffp-contract=off); m = sqrt(m); x[i] / m unless m == 0.  Square root and
// division are the correctly rounded IEEE operations on both sides.
#pragma once
#include <math.h>
#include <string.h>

#include "devmath.h"

HD double rn_from_bits(u64 b) {
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}
// IEEE binary32 bit pattern -> double
HD double rn_widen_f32_bits(unsigned b) {
    const u64 sign = (u64)(b >> 31) << 63;
    const unsigned e = (b >> 23) & 0xFFu, m = b & 0x7FFFFFu;
    if (e == 0) {  // zero or subnormal: m 2^-149
        const double v = (double)(int)m * 0x1p-149;
        return (b >> 31) ? -v : v;
    }
    if (e == 0xFFu) return rn_from_bits(sign | (0x7FFull << 52) | ((u64)m << 29));
    return rn_from_bits(sign | ((u64)(e - 127 + 1023) << 52) | ((u64)m << 29));
}
// bfloat16 = the upper half of a binary32
HD double rn_widen_bf16_bits(unsigned short b) { return rn_widen_f32_bits((unsigned)b << 16); }
// IEEE binary16 bit pattern -> double
HD double rn_widen_f16_bits(unsigned short b) {
    const u64 sign = (u64)(b >> 15) << 63;
    const unsigned e = (b >> 10) & 0x1Fu, m = b & 0x3FFu;
    if (e == 0) {  // zero or subnormal: m 2^-24
        const double v = (double)(int)m * 0x1p-24;
        return (b >> 15) ? -v : v;
    }
    if (e == 0x1Fu) return rn_from_bits(sign | (0x7FFull << 52) | ((u64)m << 42));
    return rn_from_bits(sign | ((u64)(e - 15 + 1023) << 52) | ((u64)m << 42));
}

// one step of the squared sum, the norm, one quotient: the three operations a row's owner performs, in this order
HD double rn_sq_step(double m, double x) { return m + x * x; }
HD double rn_norm(double m) { return sqrt(m); }
HD double rn_quot(double x, double m) { return m != 0 ? x / m : x; }

// a whole row in place: the host's normalize(), and what the kernel computes from the three steps above
HD void rn_normalise_row(double *x, int dim) {
    double m = 0.0;
    for (int i = 0; i < dim; i++) m = rn_sq_step(m, x[i]);
    m = rn_norm(m);
    if (m != 0)
        for (int i = 0; i < dim; i++) x[i] = rn_quot(x[i], m);
}
