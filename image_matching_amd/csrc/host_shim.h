// image_matching_amd/csrc/host_shim.h — the HIP vector types and device intrinsics ntt_arith.h uses, for a HOST build of that header
// (tests/csrc/ntt_arith_check.cpp checks the real butterfly structs against exact integer arithmetic).  Device code never includes
// this file: under __HIPCC__ ntt_arith.h takes the same names from hip_runtime.h.  Build the host program with -ffp-contract=off and
// without fast-math, so that every double operation is the single IEEE operation the device performs.
#pragma once
#if defined(__HIPCC__)
#error "host_shim.h is for host-only builds"
#endif
#include <cmath>
#include <cstring>
#include "devmath.h"

struct ulonglong2 {
    u64 x, y;
};
struct double2 {
    double x, y;
};
inline double2 make_double2(double x, double y) { return double2{x, y}; }
inline ulonglong2 make_ulonglong2(u64 x, u64 y) { return ulonglong2{x, y}; }
inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((u64)a * b) >> 32); }
inline u64 __umul64hi(u64 a, u64 b) { return (u64)(((u128)a * b) >> 64); }
inline double __fma_rn(double a, double b, double c) { return std::fma(a, b, c); }  // one rounding, as v_fma_f64
inline double __longlong_as_double(long long x) {
    double d;
    std::memcpy(&d, &x, sizeof d);
    return d;
}
inline long long __double_as_longlong(double d) {
    long long x;
    std::memcpy(&x, &d, sizeof x);
    return x;
}
// rint: std::rint in the default rounding mode (round to nearest, ties to even), as v_rndne_f64
using std::rint;
