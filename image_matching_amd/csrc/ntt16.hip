// image_matching_amd/csrc/ntt16.hip — plain negacyclic NTT / INTT for the ring N = 2^16 of approaches 1-3 on gfx950.
//
// N = 256 rows x 256 columns, tables and bit-reversed order as everywhere else.  Forward = pass 1 (stages 0-7, row strides 128..1: a
// workgroup owns 16 adjacent columns of all 256 rows) then pass 2 (stages 8-15 inside 256-coefficient blocks: a workgroup owns 2048
// consecutive coefficients); the inverse runs pass 2' then pass 1' with Gentleman-Sande butterflies and applies 1/N (times the
// caller's factor) in its last store.  Butterflies run in REGISTERS — radix 16 x radix 16 in pass 1 with one LDS exchange, radix
// 8 x 8 x 4 in pass 2 with two — with the three exact arithmetics of ntt_arith.h chosen per limb (FpA where NttTables::fp_mask is set,
// IntP where pm_mask is set, IntA otherwise), so results are bit-identical to the ring-size-generic kernels'.  FpA limbs travel
// between the passes as raw doubles in the (uint64) buffer; every limb leaves canonical.  No fused prologues or epilogues here.
//
// The schedule itself — stage order, twiddle indices, fold / re-centre points — lives in ntt16_sched.h, which the host check
// tests/csrc/ntt16_arith_check.cpp runs too.  Its bounds for 8 + 8 stages (q+ = fold's range 2^60 + 15c = q + 16c; 16q + 16c = 2^64):
//
//   IntA     Harvey: [0, 4q) forward, [0, 2q) inverse at every stage, any number of stages; the hooks are empty.
//   IntP fwd ct takes a < 12q + 16c (b any word) and adds 4q, so THREE stages run from a fold.
//            pass 1: canonical < q | st 0-2 -> 13q | fold -> q+ | st 3 -> 5q+ | LDS | st 4, 5 -> 13q+ | fold -> q+ | st 6, 7 -> 9q+, raw.
//            pass 2: fold on reading (from_raw) -> q+ | st 8-10 -> 13q+ | fold | st 11-13 -> 13q+ | fold (mid) | st 14, 15 -> 9q+ |
//            fin_fwd.  Two folds in pass 1, as in the seven-stage pass 1 of ntt15.hip; the largest value ever held is below 13q + 16c.
//   IntP inv gs takes a, b < 8q: sums below 16q, products below 4q, so bounds run 4, 8, 16 q over THREE stages from a fold.
//            pass 2': canonical | st 15, 14 -> 8q | fold | st 13-11 -> 16q | fold | st 10-8 -> 16q | fold -> q+, raw.
//            pass 1': q+ | st 7-5 -> 16q | fold (recentre) | st 4 -> 4q | LDS | st 3, 2 -> 16q | fold (recentre_wide) | st 1, 0 -> 8q |
//            fin_inv (an exact Shoup product of any 64-bit word).
//   FpA fwd  no reduction at all.  |r| <= q/2 + |v| (w/q) 2^-52 q per product (pair tables: the quotient w / q is precomputed), and
//            q 2^-52 < 1/32 for q < 2^47, so the magnitude in units of q obeys m' <= m + 1/2 + m / 32 from m = 1: below 11.9 q after
//            sixteen stages — under 2^50.6 for a 47-bit prime, under 2^48.7 for the lean ones — inside u2d / d2u's 2^52 window with a
//            factor 2.6 to spare (the fifteen stages of ntt15.hip reach 10.9 q).
//   FpA inv  sums double.  Non-lean primes reduce at every hook: runs of 2 | 3 | 3 | 3 | 1 + 2 | 2 stages from q, q/2, q/2, q/2, q/2, q/2:
//            at most 4 q < 2^49, and fin_inv takes 2 q.  Lean primes (32 q < 2^50.1) skip the recentre_wide hooks: runs of 5 (from q:
//            32 q), 3 + 3 (from q/2: 32 q) and 1 + 4 (from q/2: 16 q) stages; fin_inv takes 16 q < 2^49.1, where its product is still
//            within 0.75 q, so one conditional addition makes it canonical.  (Without the hook after stage 2 a 47-bit prime would hand
//            fin_inv 16 q = 2^51, where |r| can reach q: that hook is what the extra stage costs.)
//
// Pass 1, k_ntt16_p1: grid (16 column tiles, X * limbs), 256 threads, col = t & 15, g = t >> 4, 16 values per thread.  Phase A works
// on rows g + 16k with workgroup-uniform twiddles, phase B on rows 16g + l with twiddles 16..255 staged once per workgroup in LDS from
// the pair tables.  The LDS image is 16 groups of 16 rows x 16 columns, each group padded by 16 words (34 KiB): a half-wave's
// ds_read/write_b64 cover 256 consecutive bytes modulo the bank window in both phases.  A workgroup reads its whole tile before the
// exchange and writes after it, so src == dst is allowed.
// (src and dst are declared __restrict__ although the in-place calls — forward pass 2, inverse pass 1', and any caller's src == dst —
// pass the same pointer, as ntt15.hip does: every value a workgroup stores was computed from loads that went through an LDS exchange
// first, and no workgroup touches another's tile or chunk, so there is no load the qualifier could let the compiler move past a store
// to the same address.  A kernel that stored before its last load of the tile would break this.)
// Pass 2, k_ntt16_p2: grid (32 chunks of 2048, (X / NP) * limbs), 256 threads, 8 values per thread and polynomial; NP = 2 polynomials
// of one limb share every twiddle load in large launches.  Wave-synchronous as in ntt15.hip: a 256-block belongs to one half-wave in
// every phase, so the exchanges need no s_barrier.  Loads and stores of the canonical side are 16 bytes.
#include "kernels.h"
#include "ntt16_sched.h"

#include <cstdio>

namespace {

constexpr int N16 = 65536;

// ------------------------------------------------------------------------------------------------ pass 1 (strided)
DEV int p1_at(int row, int col) { return (row >> 4) * 272 + (row & 15) * 16 + col; }
constexpr int P1_LDS = 16 * 272;

template <class A, bool INV>
DEV void p1_body16(const A ar, const ulonglong2 *__restrict__ tw, const u64 *s, u64 *d, u64 *lds, const ulonglong2 *ltw, int t, u64 sc,
                   u64 scs) {
    typedef typename A::T T;
    const int col = t & 15, g = t >> 4;
    const auto gtw = [&](int i) { return A::tw(tw[i]); };
    const auto stw = [&](int i) { return A::tw(ltw[i]); };
    T v[16];
    if (!INV) {
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = ar.from_canon(s[(size_t)n16_p1_row_A(g, k) * 256 + col]);
        n16_p1_fwd_A(ar, v, gtw);
#pragma unroll
        for (int k = 0; k < 16; k++) lds[p1_at(n16_p1_row_A(g, k), col)] = A::to_bits(v[k]);
        __syncthreads();  // (also: ltw is in place)
#pragma unroll
        for (int l = 0; l < 16; l++) v[l] = A::from_bits(lds[p1_at(n16_p1_row_B(g, l), col)]);
        n16_p1_fwd_B(ar, v, g, stw);
#pragma unroll
        for (int l = 0; l < 16; l++) d[(size_t)n16_p1_row_B(g, l) * 256 + col] = A::to_bits(v[l]);  // raw: pass 2 finishes
    } else {
#pragma unroll
        for (int l = 0; l < 16; l++) v[l] = A::from_bits(s[(size_t)n16_p1_row_B(g, l) * 256 + col]);  // raw from pass 2'
        __syncthreads();  // ltw
        n16_p1_inv_B(ar, v, g, stw);
#pragma unroll
        for (int l = 0; l < 16; l++) lds[p1_at(n16_p1_row_B(g, l), col)] = A::to_bits(v[l]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = A::from_bits(lds[p1_at(n16_p1_row_A(g, k), col)]);
        n16_p1_inv_A(ar, v, gtw);
#pragma unroll
        for (int k = 0; k < 16; k++) d[(size_t)n16_p1_row_A(g, k) * 256 + col] = ar.fin_inv(v[k], sc, scs);
    }
}

template <bool INV>
__global__ __launch_bounds__(256) void k_ntt16_p1(NttTables T, const u64 *__restrict__ src, u64 *__restrict__ dst, size_t so, size_t dso,
                                                  LimbSel sel, ScaleSel scale) {
    __shared__ u64 lds[P1_LDS];
    __shared__ ulonglong2 ltw[256];
    const int y = blockIdx.y, x = y / sel.n, slot = y - x * sel.n, m = sel.mod[slot];
    const ModC M = T.mod[m];
    const bool fp = (T.fp_mask >> m) & 1u;
    const ulonglong2 *__restrict__ tw = (fp ? (INV ? T.itwf : T.twf) : (INV ? T.itwp : T.twp)) + (size_t)m * N16;
    const int c0 = blockIdx.x * 16;
    const u64 *s = src + (size_t)x * so + (size_t)slot * N16 + c0;
    u64 *d = dst + (size_t)x * dso + (size_t)slot * N16 + c0;
    const int t = threadIdx.x;
    ltw[t] = tw[t];
    const u64 sc = INV ? scale.s[slot] : 0, scs = INV ? scale.s_sh[slot] : 0;
    if (fp) p1_body16<FpA, INV>(FpA(M), tw, s, d, lds, ltw, t, sc, scs);
    else if ((T.pm_mask >> m) & 1u) p1_body16<IntP, INV>(IntP(M), tw, s, d, lds, ltw, t, sc, scs);
    else p1_body16<IntA, INV>(IntA(M), tw, s, d, lds, ltw, t, sc, scs);
}

// ------------------------------------------------------------------------------------------------ pass 2 (contiguous)
// The LDS image of a workgroup: 8 blocks x 8 rows x 32 coefficients per polynomial, rows padded to 36 so phase B's (row, 4k + b)
// accesses of a half-wave hit 32 distinct bank pairs (the image of ntt15.hip's pass 2).
constexpr int P2_LDS = 8 * 288;
DEV int p2_at(int blk, int row, int pos) { return blk * 288 + row * 36 + pos; }
DEV int p2_pos(int blk, int P) { return p2_at(blk, P >> 5, P & 31); }  // position P of the 256-block
// an exchange between lanes of ONE wave: the LDS executes a wave's instructions in order, so the compiler must keep the accesses on
// their side and nothing else is needed
DEV void p2_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class A, bool INV, int NP>
DEV void p2_body16(const A ar, const ulonglong2 *__restrict__ tw, const u64 *const *s, u64 *const *d, u64 (*lds)[P2_LDS], int t, int B0) {
    typedef typename A::T T;
    const int blk = t >> 5, w = t & 31;
    const int bg = (B0 >> 8) + blk;
    const int a = w >> 2;
    const auto gtw = [&](int i) { return A::tw(tw[i]); };
    T v[NP][8];
    if (!INV) {
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) v[p][k] = ar.from_raw(s[p][blk * 256 + n16_p2_pos_A(w, k)]);  // raw from pass 1
        n16_p2_fwd_A<A, NP>(ar, v, bg, gtw);
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) lds[p][p2_pos(blk, n16_p2_pos_A(w, k))] = A::to_bits(v[p][k]);
        p2_wave_sync();
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) v[p][k] = A::from_bits(lds[p][p2_pos(blk, n16_p2_pos_B(w, k))]);
        n16_p2_fwd_B<A, NP>(ar, v, 8 * bg + a, gtw);
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) lds[p][p2_pos(blk, n16_p2_pos_B(w, k))] = A::to_bits(v[p][k]);
        p2_wave_sync();
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int e = blk * 256 + n16_p2_pos_C(w, hh), u = e & 255, la = p2_at(blk, u >> 5, u & 31);  // four consecutive slots
            T c[NP][4];
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
                for (int k = 0; k < 4; k++) c[p][k] = A::from_bits(lds[p][la + k]);
            n16_p2_fwd_C<A, NP>(ar, c, (B0 + e) >> 2, gtw);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                *reinterpret_cast<ulonglong2 *>(d[p] + e) = make_ulonglong2(ar.fin_fwd(c[p][0]), ar.fin_fwd(c[p][1]));
                *reinterpret_cast<ulonglong2 *>(d[p] + e + 2) = make_ulonglong2(ar.fin_fwd(c[p][2]), ar.fin_fwd(c[p][3]));
            }
        }
    } else {
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int e = blk * 256 + n16_p2_pos_C(w, hh), u = e & 255, la = p2_at(blk, u >> 5, u & 31);
            T c[NP][4];
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const ulonglong2 i0 = *reinterpret_cast<const ulonglong2 *>(s[p] + e), i1 = *reinterpret_cast<const ulonglong2 *>(s[p] + e + 2);
                c[p][0] = ar.from_canon(i0.x); c[p][1] = ar.from_canon(i0.y);
                c[p][2] = ar.from_canon(i1.x); c[p][3] = ar.from_canon(i1.y);
            }
            n16_p2_inv_C<A, NP>(ar, c, (B0 + e) >> 2, gtw);
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
                for (int k = 0; k < 4; k++) lds[p][la + k] = A::to_bits(c[p][k]);
        }
        p2_wave_sync();
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) v[p][k] = A::from_bits(lds[p][p2_pos(blk, n16_p2_pos_B(w, k))]);
        n16_p2_inv_B<A, NP>(ar, v, 8 * bg + a, gtw);
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) lds[p][p2_pos(blk, n16_p2_pos_B(w, k))] = A::to_bits(v[p][k]);
        p2_wave_sync();
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) v[p][k] = A::from_bits(lds[p][p2_pos(blk, n16_p2_pos_A(w, k))]);
        n16_p2_inv_A<A, NP>(ar, v, bg, gtw);
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
            for (int k = 0; k < 8; k++) d[p][blk * 256 + n16_p2_pos_A(w, k)] = A::to_bits(v[p][k]);  // raw: pass 1' finishes
    }
}

template <bool INV, int NP>
__global__ __launch_bounds__(256) void k_ntt16_p2(NttTables T, const u64 *__restrict__ src, u64 *__restrict__ dst, size_t so, size_t dso,
                                                  LimbSel sel) {
    __shared__ u64 lds[NP][P2_LDS];
    const int y = blockIdx.y, xp = y / sel.n, slot = y - xp * sel.n, m = sel.mod[slot];
    const ModC M = T.mod[m];
    const bool fp = (T.fp_mask >> m) & 1u;
    const ulonglong2 *__restrict__ tw = (fp ? (INV ? T.itwf : T.twf) : (INV ? T.itwp : T.twp)) + (size_t)m * N16;
    const int B0 = blockIdx.x * 2048;
    const u64 *s[NP];
    u64 *d[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        s[p] = src + (size_t)(xp * NP + p) * so + (size_t)slot * N16 + B0;
        d[p] = dst + (size_t)(xp * NP + p) * dso + (size_t)slot * N16 + B0;
    }
    if (fp) p2_body16<FpA, INV, NP>(FpA(M), tw, s, d, lds, threadIdx.x, B0);
    else if ((T.pm_mask >> m) & 1u) p2_body16<IntP, INV, NP>(IntP(M), tw, s, d, lds, threadIdx.x, B0);
    else p2_body16<IntA, INV, NP>(IntA(M), tw, s, d, lds, threadIdx.x, B0);
}

}  // namespace

namespace hk {

// two polynomials per pass-2 workgroup share the twiddle loads; small launches (below 4 workgroups per CU when paired) run one
// polynomial per workgroup: twice the workgroups, half the serial work in each
static bool pair_polys16(int X, int nsl) { return X % 2 == 0 && (X / 2) * nsl * 32 >= 1024; }

template <bool INV>
static void launch_p2_16(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t so, size_t dso, int X, const LimbSel &sel) {
    const bool pair = pair_polys16(X, sel.n);
    char name[48];
    snprintf(name, sizeof name, "k_ntt16_p2<%s, %d>", INV ? "true" : "false", pair ? 2 : 1);
    ledger_add(name, 2.0 * X * sel.n * N16 * 8.0);
    if (pair) hipLaunchKernelGGL((k_ntt16_p2<INV, 2>), dim3(32, (X / 2) * sel.n), dim3(256), 0, st, T, src, dst, so, dso, sel);
    else hipLaunchKernelGGL((k_ntt16_p2<INV, 1>), dim3(32, X * sel.n), dim3(256), 0, st, T, src, dst, so, dso, sel);
}

// element (x, slot) at base + x*outer + slot*N; src == dst allowed
void ntt16_forward(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t so, size_t dso, int X, const LimbSel &sel) {
    ScaleSel dummy = {};
    ledger_add("k_ntt16_p1<false>", 2.0 * X * sel.n * N16 * 8.0);
    hipLaunchKernelGGL((k_ntt16_p1<false>), dim3(16, X * sel.n), dim3(256), 0, st, T, src, dst, so, dso, sel, dummy);
    launch_p2_16<false>(st, T, dst, dst, dso, dso, X, sel);
}
void ntt16_inverse(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t so, size_t dso, int X, const LimbSel &sel,
                   const ScaleSel &scale) {
    launch_p2_16<true>(st, T, src, dst, so, dso, X, sel);
    ledger_add("k_ntt16_p1<true>", 2.0 * X * sel.n * N16 * 8.0);
    hipLaunchKernelGGL((k_ntt16_p1<true>), dim3(16, X * sel.n), dim3(256), 0, st, T, dst, dst, dso, dso, sel, scale);
}

}  // namespace hk
