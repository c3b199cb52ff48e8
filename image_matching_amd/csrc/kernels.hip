// image_matching_amd/csrc/kernels.hip — hand-written gfx950 kernels of the HyDia sender hot path.
//
// What each kernel replaces (reference call sites; the arithmetic itself is OpenFHE's, un-vendored):
//   k_ntt_*               every NTT/INTT inside EvalFastRotation / Relinearize / Rescale
//                         (/root/reference/src/sender/sender_diag.cpp:22-26, :79-80)
//   k_base_convert        ModUp / ModDown fast base conversion of hybrid key switching (same call sites)
//   k_inner_product       <digits, evk> of EvalFastRotation (sender_diag.cpp:25) and RelinearizeInPlace (:79)
//   k_moddown_combine     ModDown's (acc - conv) / P, + c0, + the evaluation-form automorphism of EvalFastRotation
//   k_hydia_tensor        512 x EvalMultNoRelin + 511 x EvalAddInPlace per block (sender_diag.cpp:70-77, :93)
//   k_hydia_plain         the same sums against a PLAIN gallery (one encoded polynomial per diagonal; no counterpart in the reference)
//   k_hydia_pq            the same sums for a PLAIN query against the encrypted database (one encoded polynomial per rotation; no
//                         counterpart in the reference), k_automorph_batch: the rotations of that plaintext
//   k_hydia_pq_mq         the same for a BATCH of plain queries: QW probes per pass over the database
//   k_hydia_plain_mq      a BATCH of encrypted queries against a PLAIN gallery: QW queries per pass over the gallery
//   k_rescale_*           RescaleInPlace (sender_diag.cpp:80)
//   k_tensor, k_lincomb*  ct x ct products and Chebyshev/f4 leaves of chebyshevCompare (src/openFHE_wrapper.cpp:143-185)
//   k_batch_sum           HERS: sum of the per-dimension products (src/sender/sender_hers.cpp:60-87)
// No MFMA: this is 64-bit integer modular arithmetic.  HBM-streaming kernels read 16 B per lane (1 KiB per wave
// instruction) of one limb, so modulus constants are wave-uniform.
#include <stdexcept>

#include "kernels.h"
#include "db_accum.h"  // the per-granule arithmetic of k_db_accumulate / k_db_accumulate46 (host-checkable)
#include "ntt_arith.h"  // FpA: exact FP64 products for the limbs below 2^47

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>

namespace {

DEV unsigned brev_n(unsigned x, int bits) { return __brev(x) >> (32 - bits); }

// ------------------------------------------------------------------------------------------------ NTT
// N = 2^logN = R * 256.  Forward = strided pass (first logN-8 stages, stride >= 256, a workgroup owns 32 adjacent
// columns x all R rows in LDS) then contiguous pass (last 8 stages inside 256-blocks; a workgroup owns 2048
// consecutive coefficients).  Inverse runs the two passes in the opposite order with Gentleman-Sande butterflies.
template <bool INV>
__global__ __launch_bounds__(256) void k_ntt_strided(NttTables T, int logN, const u64 *__restrict__ src,
                                                     u64 *__restrict__ dst, size_t so, size_t dso, LimbSel sel,
                                                     ScaleSel scale) {
    extern __shared__ u64 lds[];
    const int N = 1 << logN, logR = logN - 8, R = 1 << logR;
    const int y = blockIdx.y, x = y / sel.n, slot = y - x * sel.n, m = sel.mod[slot];
    const u64 q = T.mod[m].q;
    const u64 *s = src + (size_t)x * so + (size_t)slot * N;
    u64 *d = dst + (size_t)x * dso + (size_t)slot * N;
    const int c0 = blockIdx.x * 32, tid = threadIdx.x;
    for (int e = tid; e < R * 32; e += 256) lds[e] = s[(size_t)(e >> 5) * 256 + c0 + (e & 31)];
    __syncthreads();
    const u64 *tw = (INV ? T.itw : T.tw) + (size_t)m * N;
    const u64 *tws = (INV ? T.itw_sh : T.tw_sh) + (size_t)m * N;
    for (int st = 0; st < logR; st++) {
        const int lt = INV ? st : logR - 1 - st;           // log2 of the row stride
        const int base = INV ? (R >> (st + 1)) : (1 << st);  // twiddle block of this stage
        for (int e = tid; e < (R >> 1) * 32; e += 256) {
            const int c = e & 31, k = e >> 5;
            const int i = k >> lt, o = k & ((1 << lt) - 1);
            const int r0 = (i << (lt + 1)) + o, r1 = r0 + (1 << lt);
            const u64 W = tw[base + i], Ws = tws[base + i];
            const u64 U = lds[r0 * 32 + c], V = lds[r1 * 32 + c];
            if (!INV) {
                const u64 Vw = mulmod_shoup(V, W, Ws, q);
                lds[r0 * 32 + c] = addmod(U, Vw, q);
                lds[r1 * 32 + c] = submod(U, Vw, q);
            } else {
                lds[r0 * 32 + c] = addmod(U, V, q);
                lds[r1 * 32 + c] = mulmod_shoup(submod(U, V, q), W, Ws, q);
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < R * 32; e += 256) {
        u64 v = lds[e];
        if (INV) v = mulmod_shoup(v, scale.s[slot], scale.s_sh[slot], q);
        d[(size_t)(e >> 5) * 256 + c0 + (e & 31)] = v;
    }
}

// CH: the coefficients a workgroup owns, 2048, or 1024 for the one ring that is smaller than that (N = 2^10: one workgroup per limb)
template <bool INV, int CH = 2048>
__global__ __launch_bounds__(256) void k_ntt_contig(NttTables T, int logN, const u64 *__restrict__ src,
                                                    u64 *__restrict__ dst, size_t so, size_t dso, LimbSel sel) {
    static_assert(CH == 2048 || CH == 1024, "a chunk is a whole number of 512-coefficient loads and holds 256-coefficient blocks");
    __shared__ u64 lds[CH];
    const int N = 1 << logN;
    const int y = blockIdx.y, x = y / sel.n, slot = y - x * sel.n, m = sel.mod[slot];
    const u64 q = T.mod[m].q;
    const int B0 = blockIdx.x * CH, tid = threadIdx.x;
    const u64 *s = src + (size_t)x * so + (size_t)slot * N + B0;
    u64 *d = dst + (size_t)x * dso + (size_t)slot * N + B0;
    for (int k = 0; k < CH / 512; k++) {
        const int idx = 2 * tid + 512 * k;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(s + idx);
        lds[idx] = v.x;
        lds[idx + 1] = v.y;
    }
    __syncthreads();
    const u64 *tw = (INV ? T.itw : T.tw) + (size_t)m * N;
    const u64 *tws = (INV ? T.itw_sh : T.tw_sh) + (size_t)m * N;
    for (int st = 0; st < 8; st++) {
        const int lt = INV ? st : 7 - st;  // log2 of the stride inside the chunk
        const int base = (INV ? (N >> (lt + 1)) : (N >> (lt + 1))) + (B0 >> (lt + 1));
        // forward stage with stride t uses block mm = N/(2t); inverse stage with stride t uses block h = N/(2t)
        for (int e = tid; e < CH / 2; e += 256) {
            const int i = e >> lt, o = e & ((1 << lt) - 1);
            const int l0 = (i << (lt + 1)) + o, l1 = l0 + (1 << lt);
            const u64 W = tw[base + i], Ws = tws[base + i];
            const u64 U = lds[l0], V = lds[l1];
            if (!INV) {
                const u64 Vw = mulmod_shoup(V, W, Ws, q);
                lds[l0] = addmod(U, Vw, q);
                lds[l1] = submod(U, Vw, q);
            } else {
                lds[l0] = addmod(U, V, q);
                lds[l1] = mulmod_shoup(submod(U, V, q), W, Ws, q);
            }
        }
        __syncthreads();
    }
    for (int k = 0; k < CH / 512; k++) {
        const int idx = 2 * tid + 512 * k;
        ulonglong2 v;
        v.x = lds[idx];
        v.y = lds[idx + 1];
        *reinterpret_cast<ulonglong2 *>(d + idx) = v;
    }
}

// ------------------------------------------------------------------------------------------------ element-wise
// grid: (N/512, XP*sel.n) over XP polynomials; each thread 2 coefficients (16 B).  Operands may be limb-strided views
// (a dropped ciphertext keeps its allocation): polynomial xp of operand t starts at xp * t_ls * N.
template <int OP>
__global__ __launch_bounds__(256) void k_addsub(const ModC *__restrict__ mod, int N, const u64 *a, const u64 *b, u64 *o,
                                                LimbSel sel, int a_ls, int b_ls, int o_ls) {  // a, b, o may alias
    const int y = blockIdx.y, xp = y / sel.n, slot = y - xp * sel.n;
    const u64 q = mod[sel.mod[slot]].q;
    const size_t i = (size_t)slot * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 va = *reinterpret_cast<const ulonglong2 *>(a + (size_t)xp * a_ls * N + i);
    const ulonglong2 vb = *reinterpret_cast<const ulonglong2 *>(b + (size_t)xp * b_ls * N + i);
    ulonglong2 r;
    // OP 2: plain integer sum (the cross-shard membership reduction keeps residues unreduced until k_mod_reduce)
    r.x = OP == 0 ? addmod(va.x, vb.x, q) : OP == 1 ? submod(va.x, vb.x, q) : va.x + vb.x;
    r.y = OP == 0 ? addmod(va.y, vb.y, q) : OP == 1 ? submod(va.y, vb.y, q) : va.y + vb.y;
    *reinterpret_cast<ulonglong2 *>(o + (size_t)xp * o_ls * N + i) = r;
}
// any 64-bit value -> canonical residue of its limb (after an integer all-reduce of at most 16 residues < 2^60)
__global__ __launch_bounds__(256) void k_mod_reduce(const ModC *__restrict__ mod, int N, u64 *a, LimbSel sel, int a_ls) {
    const int y = blockIdx.y, xp = y / sel.n, slot = y - xp * sel.n;
    const ModC M = mod[sel.mod[slot]];
    u64 *p = a + (size_t)xp * a_ls * N + (size_t)slot * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(p);
    *reinterpret_cast<ulonglong2 *>(p) = make_ulonglong2(reduce64(v.x, M), reduce64(v.y, M));
}
__global__ __launch_bounds__(256) void k_mul_scalar(const ModC *__restrict__ mod, int N, const u64 *__restrict__ a,
                                                    u64 *__restrict__ o, LimbSel sel, ScaleSel c, int a_ls, int o_ls) {
    const int y = blockIdx.y, xp = y / sel.n, slot = y - xp * sel.n;
    const u64 q = mod[sel.mod[slot]].q;
    const size_t i = (size_t)slot * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 va = *reinterpret_cast<const ulonglong2 *>(a + (size_t)xp * a_ls * N + i);
    ulonglong2 r;
    r.x = mulmod_shoup(va.x, c.s[slot], c.s_sh[slot], q);
    r.y = mulmod_shoup(va.y, c.s[slot], c.s_sh[slot], q);
    *reinterpret_cast<ulonglong2 *>(o + (size_t)xp * o_ls * N + i) = r;
}
// grid (N/512, nl, X*npoly)
__global__ __launch_bounds__(256) void k_lincomb(const ModC *__restrict__ mod, int N, LinComb lc, u64 *__restrict__ o,
                                                 int npoly, int nl) {
    const int j = blockIdx.y, xp = blockIdx.z, p = xp % npoly;
    const ModC M = mod[j];
    const size_t i = (size_t)j * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    u64 ax = 0, ay = 0;  // each term < q < 2^60 and at most 8 terms (+ c0): no overflow
#pragma unroll
    for (int t = 0; t < HY_LC_TERMS; t++)
        if (t < lc.nterms) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(lc.src[t] + (size_t)xp * lc.ls[t] * N + i);
            ax += mulmod_shoup(v.x, lc.c[t][j], lc.cs[t][j], M.q);
            ay += mulmod_shoup(v.y, lc.c[t][j], lc.cs[t][j], M.q);
        }
    if (p == 0) {
        ax += lc.c0[j];
        ay += lc.c0[j];
    }
    ulonglong2 r;
    r.x = reduce64(ax, M);
    r.y = reduce64(ay, M);
    *reinterpret_cast<ulonglong2 *>(o + (size_t)xp * nl * N + i) = r;
}
// grid (N/512, nl, X*npoly): the terms are loaded once into registers, then K outputs with wave-uniform constants
// (128-bit lazy sums: 8 terms * 2^120 + c0 < 2^124)
__global__ __launch_bounds__(256) void k_lincomb_multi(const ModC *__restrict__ mod, int N, LinCombMulti lc, u64 *__restrict__ o,
                                                       int XP, int npoly, int nl) {
    const int j = blockIdx.y, xp = blockIdx.z, p = xp % npoly;
    const ModC M = mod[j];
    const size_t i = (size_t)j * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    ulonglong2 v[HY_LC_TERMS];
#pragma unroll
    for (int t = 0; t < HY_LC_TERMS; t++)
        v[t] = t < lc.nterms ? *reinterpret_cast<const ulonglong2 *>(lc.src[t] + (size_t)xp * lc.ls[t] * N + i) : make_ulonglong2(0, 0);
    if (lc.fp && M.ks + 2 <= 47) {
        // limbs below 2^47 (round 4): exact FP64 products, v c - rint(v c / q) q (six instructions, no carries) instead of 128-bit
        // multiply-accumulates and a Barrett reduction — the same canonical residues (|sum| < 8 x 0.8 q + q, exact in a double)
        const FpA ar(M);
        double vx[HY_LC_TERMS], vy[HY_LC_TERMS];
#pragma unroll
        for (int t = 0; t < HY_LC_TERMS; t++) {
            vx[t] = FpA::u2d(v[t].x);
            vy[t] = FpA::u2d(v[t].y);
        }
        for (int k = 0; k < lc.K; k++) {
            const u64 *tb = lc.tab + (size_t)k * HY_LCM_BLOCK;
            double ax = 0, ay = 0;
#pragma unroll
            for (int t = 0; t < HY_LC_TERMS; t++)
                if (t < lc.nterms) {
                    const FpA::TW W = ar.tw8(FpA::u2d(tb[t * HY_LC_LIMBS + j]));
                    ax += ar.mulmod(vx[t], W);
                    ay += ar.mulmod(vy[t], W);
                }
            if (p == 0) {
                const double c0 = FpA::u2d(tb[HY_LC_TERMS * HY_LC_LIMBS + j]);
                ax += c0;
                ay += c0;
            }
            *reinterpret_cast<ulonglong2 *>(o + ((size_t)k * XP + xp) * nl * N + i) = make_ulonglong2(ar.fin_fwd(ax), ar.fin_fwd(ay));
        }
        return;
    }
    for (int k = 0; k < lc.K; k++) {
        const u64 *tb = lc.tab + (size_t)k * HY_LCM_BLOCK;
        u128 ax = 0, ay = 0;
#pragma unroll
        for (int t = 0; t < HY_LC_TERMS; t++)
            if (t < lc.nterms) {
                const u64 c = tb[t * HY_LC_LIMBS + j];
                ax += (u128)v[t].x * c;
                ay += (u128)v[t].y * c;
            }
        if (p == 0) {
            const u64 c0 = tb[HY_LC_TERMS * HY_LC_LIMBS + j];
            ax += c0;
            ay += c0;
        }
        ulonglong2 r;
        r.x = reduce_lazy(ax, M, lc.nterms + 1);
        r.y = reduce_lazy(ay, M, lc.nterms + 1);
        *reinterpret_cast<ulonglong2 *>(o + ((size_t)k * XP + xp) * nl * N + i) = r;
    }
}
// grid (N/512, nl, npoly): serial sum over the batch with 128-bit accumulators (X * 2^60 fits)
// output m (grid.z = npoly * nout) = sum over x of ciphertext m + x * stride of `in` (stride 1, nout 1: a plain batch sum)
__global__ __launch_bounds__(256) void k_batch_sum(const ModC *__restrict__ mod, int N, const u64 *__restrict__ in,
                                                   u64 *__restrict__ o, int X, int npoly, int nl, int stride) {
    const int j = blockIdx.y, p = blockIdx.z % npoly, m = blockIdx.z / npoly;
    const ModC M = mod[j];
    const size_t i = ((size_t)p * nl + j) * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t cs = (size_t)npoly * nl * N, xs = cs * (size_t)stride;
    u128 ax = 0, ay = 0;
    for (int x = 0; x < X; x++) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(in + (size_t)m * cs + (size_t)x * xs + i);
        ax += v.x;
        ay += v.y;
    }
    ulonglong2 r;
    r.x = reduce128(ax, M);
    r.y = reduce128(ay, M);
    *reinterpret_cast<ulonglong2 *>(o + (size_t)m * cs + i) = r;
}
__global__ __launch_bounds__(256) void k_add_scalar(const ModC *__restrict__ mod, int N, u64 *__restrict__ a,
                                                    size_t outer, LimbSel sel, ScaleSel c) {
    const int y = blockIdx.y, x = y / sel.n, slot = y - x * sel.n;
    const u64 q = mod[sel.mod[slot]].q;
    u64 *p = a + (size_t)x * outer + (size_t)slot * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    ulonglong2 v = *reinterpret_cast<ulonglong2 *>(p);
    v.x = addmod(v.x, c.s[slot], q);
    v.y = addmod(v.y, c.s[slot], q);
    *reinterpret_cast<ulonglong2 *>(p) = v;
}
__global__ __launch_bounds__(256) void k_copy_limbs(int N, const u64 *__restrict__ src, u64 *__restrict__ dst,
                                                    size_t so, size_t dso, int nlimbs) {
    const int y = blockIdx.y, x = y / nlimbs, slot = y - x * nlimbs;
    const size_t i = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    *reinterpret_cast<ulonglong2 *>(dst + (size_t)x * dso + (size_t)slot * N + i) =
        *reinterpret_cast<const ulonglong2 *>(src + (size_t)x * so + (size_t)slot * N + i);
}
// EvalMultNoRelin on X pairs: grid (N/512, nl, X); inputs may be limb-strided views, output compact.
// SUB: d0 -= kap_j*c0, d1 -= kap_j*c1 for a 2-component c (the comparator's  2ab - K*c  with kap = K/2 mod q_j, applied
// ahead of the doubling relinearisation)
template <bool SUB>
__global__ __launch_bounds__(256) void k_tensor(const ModC *__restrict__ mod, int N, const u64 *__restrict__ a,
                                                const u64 *__restrict__ b, u64 *__restrict__ o, int nl, int a_ls, int b_ls,
                                                const u64 *__restrict__ c, int c_ls, ScaleSel kap) {
    const int j = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[j];
    const size_t i = (size_t)j * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t pa = (size_t)x * 2 * a_ls * N + i, pb = (size_t)x * 2 * b_ls * N + i, ps = (size_t)nl * N;
    const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(a + pa), a1 = *reinterpret_cast<const ulonglong2 *>(a + pa + (size_t)a_ls * N);
    const ulonglong2 b0 = *reinterpret_cast<const ulonglong2 *>(b + pb), b1 = *reinterpret_cast<const ulonglong2 *>(b + pb + (size_t)b_ls * N);
    ulonglong2 d0, d1, d2;
    d0.x = mulmod(a0.x, b0.x, M);
    d0.y = mulmod(a0.y, b0.y, M);
    d1.x = reduce128k((u128)a0.x * b1.x + (u128)a1.x * b0.x, M);
    d1.y = reduce128k((u128)a0.y * b1.y + (u128)a1.y * b0.y, M);
    d2.x = mulmod(a1.x, b1.x, M);
    d2.y = mulmod(a1.y, b1.y, M);
    if (SUB) {
        const size_t pc = (size_t)x * 2 * c_ls * N + i;
        const ulonglong2 c0 = *reinterpret_cast<const ulonglong2 *>(c + pc), c1 = *reinterpret_cast<const ulonglong2 *>(c + pc + (size_t)c_ls * N);
        const u64 k = kap.s[j], ks = kap.s_sh[j];
        d0.x = submod(d0.x, mulmod_shoup(c0.x, k, ks, M.q), M.q);
        d0.y = submod(d0.y, mulmod_shoup(c0.y, k, ks, M.q), M.q);
        d1.x = submod(d1.x, mulmod_shoup(c1.x, k, ks, M.q), M.q);
        d1.y = submod(d1.y, mulmod_shoup(c1.y, k, ks, M.q), M.q);
    }
    const size_t po = (size_t)x * 3 * ps + i;
    *reinterpret_cast<ulonglong2 *>(o + po) = d0;
    *reinterpret_cast<ulonglong2 *>(o + po + ps) = d1;
    *reinterpret_cast<ulonglong2 *>(o + po + 2 * ps) = d2;
}
// EvalSquare on X ciphertexts (approach 2's alpha norm, sender_hers.cpp:124 / :153): d0 = c0^2, d1 = 2 c0 c1, d2 = c1^2.  Grid and limb
// stride as k_tensor<false>; two 16-byte loads and three stores per coefficient pair where k_tensor on (a, a) loads four, three products
// instead of four.  Canonical residues, so the bits are k_tensor<false>(a, a)'s.
__global__ __launch_bounds__(256) void k_tensor_sq(const ModC *__restrict__ mod, int N, const u64 *__restrict__ a, u64 *__restrict__ o,
                                                   int nl, int a_ls) {
    const int j = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[j];
    const size_t i = (size_t)j * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t pa = (size_t)x * 2 * a_ls * N + i, ps = (size_t)nl * N;
    const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(a + pa), a1 = *reinterpret_cast<const ulonglong2 *>(a + pa + (size_t)a_ls * N);
    ulonglong2 d0, d1, d2;
    d0.x = mulmod(a0.x, a0.x, M);
    d0.y = mulmod(a0.y, a0.y, M);
    d1.x = mulmod(a0.x, a1.x, M);
    d1.y = mulmod(a0.y, a1.y, M);
    d1.x = addmod(d1.x, d1.x, M.q);
    d1.y = addmod(d1.y, d1.y, M.q);
    d2.x = mulmod(a1.x, a1.x, M);
    d2.y = mulmod(a1.y, a1.y, M);
    const size_t po = (size_t)x * 3 * ps + i;
    *reinterpret_cast<ulonglong2 *>(o + po) = d0;
    *reinterpret_cast<ulonglong2 *>(o + po + ps) = d1;
    *reinterpret_cast<ulonglong2 *>(o + po + 2 * ps) = d2;
}
// Approach 1's product of ONE query ciphertext with X database ciphertexts (EvalInnerProduct's EvalMult, sender_base.cpp:93).
// grid (N/512, nl, ceil(X / HY_BCAST_X)): a thread keeps its two coefficients of q0, q1 in registers and walks HY_BCAST_X database
// ciphertexts, so the query is fetched once per HY_BCAST_X products from its single copy; b is read where it lies (the row-packed
// resident database, [X][2][b_ls][N] plain residues), streamed once: non-temporal 16-byte loads.  Residues = k_tensor<false>'s.
#define HY_BCAST_X 4
__global__ __launch_bounds__(256) void k_tensor_bcast(const ModC *__restrict__ mod, int N, const u64 *__restrict__ qc, int q_ls,
                                                      const u64 *__restrict__ b, int b_ls, u64 *__restrict__ o, int nl, int X) {
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    const int j = blockIdx.y;
    const ModC M = mod[j];
    const size_t i = (size_t)j * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2, ps = (size_t)nl * N;
    const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(qc + i), a1 = *reinterpret_cast<const ulonglong2 *>(qc + (size_t)q_ls * N + i);
    const int x0 = blockIdx.z * HY_BCAST_X, x1 = min(X, x0 + HY_BCAST_X);
    for (int x = x0; x < x1; x++) {
        const size_t pb = (size_t)x * 2 * b_ls * N + i;
        const ull2 b0 = __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(b + pb));
        const ull2 b1 = __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(b + pb + (size_t)b_ls * N));
        ulonglong2 d0, d1, d2;
        d0.x = mulmod(a0.x, b0.x, M);
        d0.y = mulmod(a0.y, b0.y, M);
        d1.x = reduce128k((u128)a0.x * b1.x + (u128)a1.x * b0.x, M);
        d1.y = reduce128k((u128)a0.y * b1.y + (u128)a1.y * b0.y, M);
        d2.x = mulmod(a1.x, b1.x, M);
        d2.y = mulmod(a1.y, b1.y, M);
        const size_t po = (size_t)x * 3 * ps + i;
        *reinterpret_cast<ulonglong2 *>(o + po) = d0;
        *reinterpret_cast<ulonglong2 *>(o + po + ps) = d1;
        *reinterpret_cast<ulonglong2 *>(o + po + 2 * ps) = d2;
    }
}
// Approach 3's sum of K unrelinearised products (BlindSender::computeSimilarityMatrix, sender_blind.cpp:65-71): K query ciphertexts
// qc [K][2][q_ls][N] times the K chunk ciphertexts of each of X matrices, b [X][K][2][b_ls][N] (the resident database read where it
// lies: non-temporal 16-byte loads, streamed once) -> o [X][3][nl][N].  grid (N/512, nl, ceil(X / HY_DOT_X)): a thread owns two
// coefficients of HY_DOT_X matrices and walks the chunks, so a query chunk is fetched once per HY_DOT_X matrices (K small ciphertexts:
// they stay in cache).  d0, d1, d2 are 128-bit lazy sums reduced once: d0 and d2 hold K products, d1 holds 2K, each below 2^120 on the
// 60-bit limb, so 64 of them fit 128 bits (K <= 32, checked by the caller); reduce_lazy takes the true product count, because
// reduce128k's range ends at four products on that limb.  Operands are canonical residues, so the bits are those of K k_tensor<false>
// products added with k_addsub.  A ragged last group re-reads the last matrix and does not store it.
#define HY_DOT_X 2
__global__ __launch_bounds__(256) void k_tensor_dot(const ModC *__restrict__ mod, int N, const u64 *__restrict__ qc, int q_ls,
                                                    const u64 *__restrict__ b, int b_ls, u64 *__restrict__ o, int nl, int X, int K) {
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    const int j = blockIdx.y;
    const ModC M = mod[j];
    const size_t i = (size_t)j * N + (size_t)(blockIdx.x * 256 + threadIdx.x) * 2, ps = (size_t)nl * N;
    const size_t qp = (size_t)q_ls * N, bp = (size_t)b_ls * N;
    const int x0 = blockIdx.z * HY_DOT_X;
    const u64 *bg[HY_DOT_X];
#pragma unroll
    for (int g = 0; g < HY_DOT_X; g++) bg[g] = b + (size_t)min(x0 + g, X - 1) * K * 2 * bp + i;
    u128 s0x[HY_DOT_X], s0y[HY_DOT_X], s1x[HY_DOT_X], s1y[HY_DOT_X], s2x[HY_DOT_X], s2y[HY_DOT_X];
#pragma unroll
    for (int g = 0; g < HY_DOT_X; g++) s0x[g] = s0y[g] = s1x[g] = s1y[g] = s2x[g] = s2y[g] = 0;
    for (int c = 0; c < K; c++) {
        const u64 *qa = qc + (size_t)c * 2 * qp + i;
        const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(qa), a1 = *reinterpret_cast<const ulonglong2 *>(qa + qp);
#pragma unroll
        for (int g = 0; g < HY_DOT_X; g++) {
            const u64 *pb = bg[g] + (size_t)c * 2 * bp;
            const ull2 b0 = __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(pb));
            const ull2 b1 = __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(pb + bp));
            s0x[g] += (u128)a0.x * b0.x;
            s0y[g] += (u128)a0.y * b0.y;
            s1x[g] += (u128)a0.x * b1.x + (u128)a1.x * b0.x;
            s1y[g] += (u128)a0.y * b1.y + (u128)a1.y * b0.y;
            s2x[g] += (u128)a1.x * b1.x;
            s2y[g] += (u128)a1.y * b1.y;
        }
    }
#pragma unroll
    for (int g = 0; g < HY_DOT_X; g++) {
        if (x0 + g >= X) break;
        ulonglong2 d0, d1, d2;
        d0.x = reduce_lazy(s0x[g], M, K);
        d0.y = reduce_lazy(s0y[g], M, K);
        d1.x = reduce_lazy(s1x[g], M, 2 * K);
        d1.y = reduce_lazy(s1y[g], M, 2 * K);
        d2.x = reduce_lazy(s2x[g], M, K);
        d2.y = reduce_lazy(s2y[g], M, K);
        const size_t po = (size_t)(x0 + g) * 3 * ps + i;
        *reinterpret_cast<ulonglong2 *>(o + po) = d0;
        *reinterpret_cast<ulonglong2 *>(o + po + ps) = d1;
        *reinterpret_cast<ulonglong2 *>(o + po + 2 * ps) = d2;
    }
}

// ------------------------------------------------------------------------------------------------ key switching
// grid (N/512, X): each thread reads its ns source residues ONCE (2 coefficients, 16 B loads) and produces all nt
// targets — (ns + nt) limb-polys of traffic instead of nt*(ns + 1)
__global__ __launch_bounds__(256) void k_base_convert(const ModC *__restrict__ mod, int N, const u64 *__restrict__ y,
                                                      size_t yo, u64 *__restrict__ out, size_t oo, ConvTab tab,
                                                      LimbSel dsel, int tz) {
    // grid.z > 1 (few polynomials: a query's fixed-cost tail): targets [z*tz, (z+1)*tz) per slice, sources re-read from L2
    const int x = blockIdx.y;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    ulonglong2 v[HY_MAX_DIGIT];
#pragma unroll
    for (int s = 0; s < HY_MAX_DIGIT; s++)
        if (s < tab.ns) v[s] = *reinterpret_cast<const ulonglong2 *>(y + (size_t)x * yo + (size_t)s * N + c);
    const int t_lo = blockIdx.z * tz, t_hi = min(tab.nt, t_lo + tz);
    for (int t = t_lo; t < t_hi; t++) {
        if (t >= tab.skip_lo && t < tab.skip_hi) continue;
        const ModC M = mod[dsel.mod[t]];
        u128 ax = 0, ay = 0;
#pragma unroll
        for (int s = 0; s < HY_MAX_DIGIT; s++)
            if (s < tab.ns) {
                ax += (u128)v[s].x * tab.f[s][t];
                ay += (u128)v[s].y * tab.f[s][t];
            }
        // sources are residues of OTHER moduli (< 2^60), constants < q_t: up to four terms stay below 2^(k+62)
        ulonglong2 r;
        r.x = tab.ns <= 4 ? reduce128k(ax, M) : reduce128(ax, M);
        r.y = tab.ns <= 4 ? reduce128k(ay, M) : reduce128(ay, M);
        *reinterpret_cast<ulonglong2 *>(out + (size_t)x * oo + (size_t)t * N + c) = r;
    }
}
// ModUp of ALL digits of a key switch in one launch: grid (N/512, X, nd * slices).  Digit d = z / slices converts its own limbs
// (rows [skip_lo, skip_hi) of y [X][nl][N], coefficient form) into rows of out [X][nd][nE][N]; tabs[d] lives in device memory
__global__ __launch_bounds__(256) void k_base_convert_digits(const ModC *__restrict__ mod, int N, const u64 *__restrict__ y, size_t yo,
                                                             u64 *__restrict__ out, size_t oo, const ConvTab *__restrict__ tabs,
                                                             LimbSel dsel, int slices, int tz, int nE) {
    const int x = blockIdx.y, d = blockIdx.z / slices, zs = blockIdx.z - d * slices;
    const ConvTab &tab = tabs[d];
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const int ns = tab.ns, lo = tab.skip_lo, hi = tab.skip_hi;
    ulonglong2 v[HY_MAX_DIGIT];
#pragma unroll
    for (int s = 0; s < HY_MAX_DIGIT; s++)
        if (s < ns) v[s] = *reinterpret_cast<const ulonglong2 *>(y + (size_t)x * yo + (size_t)(lo + s) * N + c);
    u64 *o = out + (size_t)x * oo + (size_t)d * nE * N;
    const int t_lo = zs * tz, t_hi = min(tab.nt, t_lo + tz);
    for (int t = t_lo; t < t_hi; t++) {
        if (t >= lo && t < hi) continue;
        const ModC M = mod[dsel.mod[t]];
        u128 ax = 0, ay = 0;
#pragma unroll
        for (int s = 0; s < HY_MAX_DIGIT; s++)
            if (s < ns) {
                const u64 f = tab.f[s][t];
                ax += (u128)v[s].x * f;
                ay += (u128)v[s].y * f;
            }
        ulonglong2 r;
        r.x = ns <= 4 ? reduce128k(ax, M) : reduce128(ax, M);
        r.y = ns <= 4 ? reduce128k(ay, M) : reduce128(ay, M);
        *reinterpret_cast<ulonglong2 *>(o + (size_t)t * N + c) = r;
    }
}
// two consecutive residues of an 8-byte (PK = false) or 6-byte (PK = true) row; NT: non-temporal load
// grid (N/512, nE, X); 2 coefficients per thread, both key polys.  PK: keys[x] points at a packed key (see above)
template <bool PK>
__global__ __launch_bounds__(256) void k_inner_product(const ModC *__restrict__ mod, int N, const u64 *__restrict__ dig,
                                                       size_t dxs, int nd, const u64 *const *__restrict__ keys,
                                                       int same_key, int nT, u64 *__restrict__ acc, LimbSel esel,
                                                       const u64 *__restrict__ own, size_t own_xs, int alpha, int nl, int acc_rows,
                                                       int nQ, int dig_rows, int dig_t0) {
    // acc row t <-> modulus esel.mod[t] <-> digit row dig_t0 + t (dig_t0 > 0: only the special-prime limbs are accumulated here,
    // the Q limbs' inner product lives in the ModDown transform's epilogue — NttStore mode 5)
    const int t = blockIdx.y, x = blockIdx.z, nE = acc_rows, m = esel.mod[t];
    const ModC M = mod[m];
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const u64 *key = keys[same_key ? 0 : x];
    const bool six = PK && m > 0 && m < nQ;
    const unsigned char *kbytes = reinterpret_cast<const unsigned char *>(key) + (PK ? key_limb_offset(N, nQ, m) : 0) + c * (six ? 6 : 8);
    const size_t set_bytes = PK ? key_set_bytes(N, nQ, nT) : 0;
    u128 a0x = 0, a0y = 0, a1x = 0, a1y = 0;
    for (int d = 0; d < nd; d++) {
        // a digit's own limbs are the input itself (evaluation form): read them in place when the caller did not copy them
        const u64 *src = (own && t < nl && t / alpha == d) ? own + (size_t)x * own_xs + (size_t)t * N + c
                                                           : dig + (size_t)x * dxs + ((size_t)d * dig_rows + dig_t0 + t) * N + c;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(src);
        ulonglong2 kb, ka;
        if (PK) {
            const unsigned char *pb = kbytes + (size_t)(d * 2) * set_bytes, *pa = pb + set_bytes;
            if (six) {
                kb = db_load2<true, false>(pb);
                ka = db_load2<true, false>(pa);
            } else {
                kb = db_load2<false, false>(pb);
                ka = db_load2<false, false>(pa);
            }
        } else {
            kb = *reinterpret_cast<const ulonglong2 *>(key + (((size_t)d * 2 + 0) * nT + m) * N + c);
            ka = *reinterpret_cast<const ulonglong2 *>(key + (((size_t)d * 2 + 1) * nT + m) * N + c);
        }
        a0x += (u128)v.x * kb.x;
        a0y += (u128)v.y * kb.y;
        a1x += (u128)v.x * ka.x;
        a1y += (u128)v.y * ka.y;
    }
    ulonglong2 r0, r1;
    r0.x = reduce_lazy(a0x, M, nd);
    r0.y = reduce_lazy(a0y, M, nd);
    r1.x = reduce_lazy(a1x, M, nd);
    r1.y = reduce_lazy(a1y, M, nd);
    *reinterpret_cast<ulonglong2 *>(acc + (((size_t)x * 2 + 0) * nE + t) * N + c) = r0;
    *reinterpret_cast<ulonglong2 *>(acc + (((size_t)x * 2 + 1) * nE + t) * N + c) = r1;
}
// [nd][2][nT][N] u64 -> packed key.  grid (N/512, nT, nd*2)
// premul: the Q-limb rows are stored multiplied by P^{-1} mod q_j (mul.s[j]) — loop A's fused ModDown epilogue then needs no
// multiplication at all: (acc - conv) P^{-1} = acc' - conv' with both operands pre-scaled (NttStore mode 5, LoopAIp::premul)
__global__ __launch_bounds__(256) void k_key_pack(const ModC *__restrict__ mod, int N, int nQ, int nT, const u64 *__restrict__ key,
                                                  unsigned char *__restrict__ out, int premul, ScaleSel mul) {
    const int m = blockIdx.y, dp = blockIdx.z;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(key + ((size_t)dp * nT + m) * N + c);
    if (premul && m < nQ) {
        const u64 q = mod[m].q;
        v.x = mulmod_shoup(v.x, mul.s[m], mul.s_sh[m], q);
        v.y = mulmod_shoup(v.y, mul.s[m], mul.s_sh[m], q);
    }
    const bool six = m > 0 && m < nQ;
    unsigned char *d = out + (size_t)dp * key_set_bytes(N, nQ, nT) + key_limb_offset(N, nQ, m) + c * (six ? 6 : 8);
    typedef unsigned int u3 __attribute__((ext_vector_type(3), aligned(4)));
    if (six) {
        u3 w;
        w.x = (unsigned)v.x;
        w.y = (unsigned)(v.x >> 32) | ((unsigned)v.y << 16);
        w.z = (unsigned)(v.y >> 16);
        *reinterpret_cast<u3 *>(d) = w;
    } else {
        *reinterpret_cast<ulonglong2 *>(d) = v;
    }
}
// grid (N/256, nl, X*2)
__global__ __launch_bounds__(256) void k_moddown_combine(const ModC *__restrict__ mod, int logN,
                                                         const u64 *__restrict__ acc, int acc_limbs,
                                                         const u64 *__restrict__ conv, const u64 *__restrict__ addend,
                                                         size_t axs, size_t aps, int add_polys, u64 *__restrict__ out, int nl,
                                                         ScaleSel pinv, const unsigned *__restrict__ galois,
                                                         int same_g, const u64 *__restrict__ self, size_t sxs, size_t sps) {
    const int N = 1 << logN;
    const int j = blockIdx.y, xp = blockIdx.z, x = xp >> 1, p = xp & 1;
    const u64 q = mod[j].q;
    const unsigned co = blockIdx.x * 256 + threadIdx.x;
    unsigned c = co;
    if (galois) {
        const unsigned g = galois[same_g ? 0 : x];
        if (g != 1u) {
            const unsigned e = ((2u * brev_n(co, logN) + 1u) * g) & (2u * N - 1u);
            c = brev_n((e - 1u) >> 1, logN);
        }
    }
    u64 v = submod(acc[((size_t)xp * acc_limbs + j) * N + c], conv[((size_t)xp * nl + j) * N + c], q);
    v = mulmod_shoup(v, pinv.s[j], pinv.s_sh[j], q);
    if (addend && p < add_polys) v = addmod(v, addend[(size_t)x * axs + (size_t)p * aps + (size_t)j * N + c], q);
    // rotate-and-accumulate (approach 1's EvalSum and merge steps): self + Rot(t) leaves in this store, self read at the OUTPUT index
    if (self) v = addmod(v, self[(size_t)x * sxs + (size_t)p * sps + (size_t)j * N + co], q);
    out[((size_t)xp * nl + j) * N + co] = v;
}
// grid (N/512, XP): see moddown_rescale_conv in kernels.h.  Two coefficients per thread.  (Sources are P-limb residues < 2^60:
// up to four terms stay below 2^(k+62), the range of reduce128k.)  The conversion constants arrive with
// P^{-1} (and the doubling) already folded in: tab.f[s][j] = (P/p_s mod q_j) * P^{-1} (* 2) mod q_j, so a target costs nP lazy
// multiply-accumulates and ONE reduction.
__global__ __launch_bounds__(256) void k_moddown_rescale_conv(const ModC *__restrict__ mod, int N, const u64 *__restrict__ y,
                                                              size_t yo, const u64 *__restrict__ u, size_t uo, u64 *__restrict__ w,
                                                              int l, int nP, ConvTab tab, int tz) {
    const int xp = blockIdx.y;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    ulonglong2 v[HY_MAX_DIGIT];
#pragma unroll
    for (int s = 0; s < HY_MAX_DIGIT; s++)
        if (s < nP) v[s] = *reinterpret_cast<const ulonglong2 *>(y + (size_t)xp * yo + (size_t)s * N + c);
    // the dropped limb of the ModDown output, coefficient form: y_l = u - conv_l P^{-1} (doubled when dbl)
    const ModC Ml = mod[l];
    u128 ax = 0, ay = 0;
#pragma unroll
    for (int s = 0; s < HY_MAX_DIGIT; s++)
        if (s < nP) {
            ax += (u128)v[s].x * tab.f[s][l];
            ay += (u128)v[s].y * tab.f[s][l];
        }
    const ulonglong2 uu = *reinterpret_cast<const ulonglong2 *>(u + (size_t)xp * uo + c);
    const u64 ylx = submod(uu.x, (nP <= 4 ? reduce128k(ax, Ml) : reduce128(ax, Ml)), Ml.q), yly = submod(uu.y, (nP <= 4 ? reduce128k(ay, Ml) : reduce128(ay, Ml)), Ml.q);
    const u64 half = Ml.q >> 1;
    const bool negx = ylx > half, negy = yly > half;
    const u64 magx = negx ? Ml.q - ylx : ylx, magy = negy ? Ml.q - yly : yly;  // |centred residue|
    const int j_lo = blockIdx.z * tz, j_hi = min(l, j_lo + tz);  // grid.z slices the targets of small launches
    for (int j = j_lo; j < j_hi; j++) {
        const ModC M = mod[j];
        u128 bx = 0, by = 0;
#pragma unroll
        for (int s = 0; s < HY_MAX_DIGIT; s++)
            if (s < nP) {
                bx += (u128)v[s].x * tab.f[s][j];
                by += (u128)v[s].y * tab.f[s][j];
            }
        const u64 rx = reduce64(magx, M), ry = reduce64(magy, M);
        ulonglong2 o;
        o.x = addmod((nP <= 4 ? reduce128k(bx, M) : reduce128(bx, M)), negx ? negmod(rx, M.q) : rx, M.q);
        o.y = addmod((nP <= 4 ? reduce128k(by, M) : reduce128(by, M)), negy ? negmod(ry, M.q) : ry, M.q);
        *reinterpret_cast<ulonglong2 *>(w + ((size_t)xp * l + j) * N + c) = o;
    }
}
// grid (N/512, XP)
__global__ __launch_bounds__(256) void k_moddown_last_limb(const ModC *__restrict__ mod, int N, const u64 *acc,  // u may be acc's row l
                                                           int acc_limbs, const u64 *__restrict__ addend, size_t add_x,
                                                           size_t add_p, u64 *u, size_t uo, int l, u64 pinv, u64 pinv_sh,
                                                           int dbl) {
    const int xp = blockIdx.y, x = xp >> 1, p = xp & 1;
    const u64 q = mod[l].q;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(acc + ((size_t)xp * acc_limbs + l) * N + c);
    const ulonglong2 d = *reinterpret_cast<const ulonglong2 *>(addend + (size_t)x * add_x + (size_t)p * add_p + (size_t)l * N + c);
    ulonglong2 r;
    r.x = addmod(mulmod_shoup(a.x, pinv, pinv_sh, q), d.x, q);
    r.y = addmod(mulmod_shoup(a.y, pinv, pinv_sh, q), d.y, q);
    if (dbl) {
        r.x = addmod(r.x, r.x, q);
        r.y = addmod(r.y, r.y, q);
    }
    *reinterpret_cast<ulonglong2 *>(u + (size_t)xp * uo + c) = r;
}
// grid (N/256, l, X)
__global__ __launch_bounds__(256) void k_rescale_spread(const ModC *__restrict__ mod, int N, const u64 *__restrict__ t,
                                                        u64 *__restrict__ tmp, int l) {
    const int j = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[j];
    const u64 ql = mod[l].q, half = ql >> 1;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u64 v = t[(size_t)x * N + c];
    tmp[((size_t)x * l + j) * N + c] = v > half ? negmod(reduce64(ql - v, M), M.q) : reduce64(v, M);
}
__global__ __launch_bounds__(256) void k_rescale_combine(const ModC *__restrict__ mod, int N, const u64 *__restrict__ in,
                                                         const u64 *__restrict__ tmp, u64 *__restrict__ out, int l,
                                                         ScaleSel qlinv, int in_ls) {
    const int j = blockIdx.y, x = blockIdx.z;
    const u64 q = mod[j].q;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u64 v = submod(in[((size_t)x * in_ls + j) * N + c], tmp[((size_t)x * l + j) * N + c], q);
    out[((size_t)x * l + j) * N + c] = mulmod_shoup(v, qlinv.s[j], qlinv.s_sh[j], q);
}

// ------------------------------------------------------------------------------------------------ loop B
// acc[g][{d0,d1,d2}][j][c] = sum_{i<dim} rot[i] (x) db[g][i] with 128-bit lazy accumulation: one double-word
// Barrett per output instead of 4*dim reductions.  45/46-bit limbs never overflow (dim * 2^93 < 2^128); the 60-bit
// limb folds its accumulators every 32 diagonals (Sums128::chunk).  16 B per lane per operand (1 KiB per wave instruction).
//
// Work split (HBM must see the 3 GiB of rotated queries ONCE, not once per block): a workgroup owns one 128-coefficient
// tile of one limb and NW*BPP database blocks — each of its NW waves serves BPP blocks with one register copy of the
// rot operands, and the NW waves read the SAME rot addresses in step (one barrier per diagonal), so the per-CU vector
// cache serves NW-1 of them.  The database operands are streamed with non-temporal loads so they do not evict rot.
// grid (256 tiles * G/(NW*BPP), nl), block group fastest.
// Database residues of the 45/46-bit limbs are stored as 48-bit integers (two per 12-byte load): -23 % HBM bytes on the
// operand that dominates loop B.  Limb 0 (60 bit) and the rotated queries stay 8-byte.
// what a loop-B wave adds to its operand pointer: first byte of (block g0, diagonal 0, polynomial 0, its two residues) and the strides
// to the next block of the wave, the next diagonal, the other polynomial.  g0 = first block of the wave, grp = its workgroup's group
struct DbWalk {
    size_t base, su, si, sp;
};
DEV DbWalk db_walk(const DbLayout &L, int N, int dim, int j, int tile, int lane, int g0, int grp, int u0) {
    const size_t es = (L.packed && j > 0) ? 6 : 8;
    DbWalk w;
    if (!L.seq) {
        w.base = (size_t)g0 * dim * L.ct_bytes + db_limb_offset(L, N, j) + ((size_t)tile * 128 + lane * 2) * es;
        w.su = (size_t)dim * L.ct_bytes;
        w.si = L.ct_bytes;
        w.sp = L.poly_bytes;
    } else {
        const size_t groups = L.blocks / L.seq, ub = db_unit_bytes(L, j), np = db_polys(L);
        // (bits46: the lane's two residues start at bit 92 lane of the unit; it loads 16 bytes from the dword that holds that bit)
        const size_t in_unit = (L.bits46 && j > 0) ? db_lane_load46(lane) : (size_t)lane * 2 * es;
        w.base = (size_t)L.blocks * L.bd * np * db_limb_offset(L, N, j) + ((((size_t)tile * groups + grp) * L.bd) * L.seq + u0) * np * ub + in_unit;
        w.su = np * ub;
        w.si = (size_t)L.seq * np * ub;
        w.sp = ub;
    }
    return w;
}
// One Karatsuba step per coefficient: d0 += a0 b0, d2 += a1 b1, dk += (a0+a1)(b0+b1); d1 = dk - d0 - d2 at the end.
// Three products per coefficient instead of four — loop B is co-bound by the integer multiplier, not only by HBM.
//
// Two arithmetics (policies of k_hydia_tensor), same sums, one reduction per output:
// - Sums128: 64x64->128 products in 128-bit lazy sums (gfx950 builds one from four v_mad_u64_u32).  A Karatsuba product of a k-bit
//   limb is budgeted at 2^(2k+2) and a sum folded every chunk = 2^(125 - 2k) diagonals, q + chunk 2^(2k+2) < 2^128: every 32 on a
//   60-bit limb, 128 on a 59-bit one, never from 47 bits down (chunk = dim) nor, in effect, at 48 (2^29).  The budget is one bit
//   above what residues below q reach — 64 (2q - 2)^2 + q < 256 q^2 < 2^128, so 64 would hold too; 65 would not
//   (tests/test_loop_b_model_cpu.py; the kernels on saturated residues: tests/test_gpu_loop_b_edges.py).
// - Halves24, on the packed limbs of a group-sequential database (residues and rotated-query residues below 2^48).  There HBM
//   delivers 7 TB/s and the 128-bit multiply-accumulates (94 % of the vector issue slots at 6 TB/s) would be the limit, so the
//   products are taken on 24-bit halves, a = ah 2^24 + al, b = bh 2^24 + bl: the partial sums  ll = sum al bl,
//   mid = sum (al bh + ah bl),  hh = sum ah bh  stay below 2^63 for up to 4096 diagonals (Karatsuba's operand sums included:
//   halves below 2^25), so every multiply-accumulate is ONE v_mad_u64_u32 with no carry — 12 per coefficient instead of three
//   128-bit ones of ~9 instructions each; the 6-byte (48-bit) or 46-bit residues are cut into halves straight from the loaded dwords.
// (The halves pass through an empty asm statement: knowing an operand has 24 bits the compiler (ROCm 7.2) forms 24-bit multiplies,
// drops the masks they make redundant, and then fuses some of them back into v_mad_u64_u32 on the UNMASKED registers — wrong
// products; tools/ubench/tensor_check.cpp found it.)
DEV unsigned hide24(unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
}
struct Acc24 {
    u64 ll, mid, hh;
    DEV void mac(unsigned al, unsigned ah, unsigned bl, unsigned bh) {
        ll += (u64)al * bl;
        mid += (u64)al * bh;
        mid += (u64)ah * bl;
        hh += (u64)ah * bh;
    }
    DEV u128 wide() const { return (u128)ll + ((u128)mid << 24) + ((u128)hh << 48); }
};
// two 46-bit residues at bit `s` (a multiple of 4 below 32) of four dwords (bits46 layout): fetched as one 4-byte-aligned 16-byte load
struct DbRaw46 {
    typedef unsigned int u4a __attribute__((ext_vector_type(4), aligned(4)));
    u4a w;
    template <bool NT>
    DEV void load(const unsigned char *p) {
        w = NT ? __builtin_nontemporal_load(reinterpret_cast<const u4a *>(p)) : *reinterpret_cast<const u4a *>(p);
    }
};
// A policy turns a rotated-query residue (rot) and a loaded database operand (cut: one polynomial's two residues) into operands of
// type T, multiply-accumulates them into a Sum (mac) and reduces it (reduce; fold: mid-way, every `chunk` diagonals).
template <bool PK>  // PK: 6-byte database residues
struct Sums128 {
    typedef u64 T;
    typedef u128 Sum;
    typedef DbRaw<PK> Raw;
    static constexpr int depth = 2;  // operand sets in flight
    static constexpr const char *name = PK ? "Sums128<true>" : "Sums128<false>";
    int chunk;  // products a lazy 128-bit sum can take
    DEV Sums128(const ModC &M, int dim, int) {
        const int kbits = M.ks + 2;
        chunk = (125 - 2 * kbits >= 30) ? dim : (1 << (125 - 2 * kbits));
    }
    DEV static T rot(u64 v) { return v; }
    DEV void cut(const Raw &r, T (&b)[2]) const {
        const ulonglong2 v = r.get();
        b[0] = v.x;
        b[1] = v.y;
    }
    DEV static void mac(Sum &s, T a, T b) { s += (u128)a * b; }
    DEV static void fold(Sum &s, const ModC &M) { s = reduce128(s, M); }
    DEV static u64 reduce(const Sum &s, const ModC &M) { return reduce128(s, M); }
};
struct Half24 {
    unsigned l, h;
    DEV Half24 operator+(Half24 o) const { return {l + o.l, h + o.h}; }
};
template <bool B46>  // B46: 46-bit residues in 736-byte units, else 6-byte residues
struct Halves24 {
    typedef Half24 T;
    typedef Acc24 Sum;
    typedef typename std::conditional<B46, DbRaw46, DbRaw<true>>::type Raw;
    // 46-bit units: 4 % fewer bytes per diagonal, and with one diagonal in flight per wave the launch did not get shorter — it is
    // bound by what a CU keeps in flight (3 workgroups x one diagonal = 35 KB; 1.4 us of latency), not by HBM.  So the database
    // operands run TWO diagonals ahead there (three rotating sets), the rotated-query lines (L2) one ahead as before.
    static constexpr int depth = B46 ? 3 : 2;
    static constexpr const char *name = B46 ? "Halves24<true>" : "Halves24<false>";
    int chunk;  // = dim: the sums hold 4096 diagonals, the launcher's limit
    unsigned s46;  // B46: bit of the lane's first residue inside its first dword
    DEV Halves24(const ModC &, int dim, int lane) : chunk(dim), s46((unsigned)(lane * 92) & 31u) {}
    DEV static T rot(u64 v) {  // below 2^48
        return {hide24((unsigned)v & 0xFFFFFFu), __builtin_amdgcn_alignbit((unsigned)(v >> 32), (unsigned)v, 24)};
    }
    DEV void cut(const Raw &r, T (&b)[2]) const {
        const auto w = r.w;
        if constexpr (B46) {  // T = (w3:w2:w1:w0) >> s: residue 0 = T[0, 46), residue 1 = T[46, 92); halves of 24 and 22 bits
            const unsigned t0 = __builtin_amdgcn_alignbit(w[1], w[0], s46), t1 = __builtin_amdgcn_alignbit(w[2], w[1], s46),
                           t2 = __builtin_amdgcn_alignbit(w[3], w[2], s46);
            b[0] = {hide24(t0 & 0xFFFFFFu), hide24(__builtin_amdgcn_alignbit(t1, t0, 24) & 0x3FFFFFu)};
            b[1] = {hide24(__builtin_amdgcn_alignbit(t2, t1, 14) & 0xFFFFFFu), hide24((t2 >> 6) & 0x3FFFFFu)};
        } else {  // two 48-bit integers in three dwords
            b[0] = {hide24(w[0] & 0xFFFFFFu), hide24(__builtin_amdgcn_alignbit(w[1], w[0], 24) & 0xFFFFFFu)};
            b[1] = {hide24(__builtin_amdgcn_alignbit(w[2], w[1], 16) & 0xFFFFFFu), hide24(w[2] >> 8)};
        }
    }
    DEV static void mac(Sum &s, T a, T b) { s.mac(a.l, a.h, b.l, b.h); }
    DEV static void fold(Sum &, const ModC &) {}  // never reached (chunk = dim)
    DEV static u64 reduce(const Sum &s, const ModC &M) { return reduce128(s.wide(), M); }
};
// one Karatsuba step on a lane's coefficient pair: a, b = [polynomial][coefficient] operands of the query and the database;
// s = [d0, d2, dk][coefficient].  (The operand sums are formed here: the compiler forms each once per diagonal)
template <class A>
DEV void kara_mac(typename A::Sum (&s)[3][2], const typename A::T (&a)[2][2], const typename A::T (&b)[2][2]) {
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int e = 0; e < 2; e++) A::mac(s[k][e], a[k][e], b[k][e]);
#pragma unroll
    for (int e = 0; e < 2; e++) A::mac(s[2][e], a[0][e] + a[1][e], b[0][e] + b[1][e]);
}
// Output slot of (query q of the batch of Qt, block gi): ng == 0: q G + gi; ng > 0 (baby-step / giant-step split, gi = (database
// block, giant)): giant-major over the WHOLE batch, (g Qt + q) nblk + block — one giant step's partial sums over every query and
// block are one contiguous batch.  A single query is q = 0 of Qt = 1.
DEV size_t mq_slot(int q, int gi, int G, int ng, int nblk, int Qt) {
    return ng > 0 ? ((size_t)(gi % ng) * Qt + q) * nblk + gi / ng : (size_t)q * G + gi;
}
// the three reduced sums (d0, dk, d2 of the lane's two coefficients) -> components d0, d1 = dk - d0 - d2, d2 of the accumulator
DEV void store_karatsuba(u64 *o, size_t ps, ulonglong2 r0, ulonglong2 rk, ulonglong2 r2, u64 q) {
    *reinterpret_cast<ulonglong2 *>(o) = r0;
    *reinterpret_cast<ulonglong2 *>(o + ps) = make_ulonglong2(submod(submod(rk.x, r0.x, q), r2.x, q), submod(submod(rk.y, r0.y, q), r2.y, q));
    *reinterpret_cast<ulonglong2 *>(o + 2 * ps) = r2;
}
// ------------------------------------------------------------------------------------------------ loop B: the three products
// The product-form policy beside the arithmetic policy.  A form F states what one diagonal multiplies:
//   qp     polynomials per rotated-query entry (so one rotation is qp limb-polynomial sets: the rot stride per rotation)
//   dp     polynomials per database entry
//   sums   lazy sums per block, query and coefficient;  comps  components stored per accumulator slot
//   mac    feeds the sums of a lane's coefficient pair from the prepared operands a[polynomial][coefficient], b[polynomial][coefficient]
//   store  writes the reduced sums r[sum] (one coefficient pair each) as the slot's components, ps elements apart
//   name   of the kernel family (k_hydia_<name>, k_hydia_<name>_sk);  batch: the launcher serves batches of queries with it (QW = 2
//          passes, NW = 8 workgroups), and its instantiation names carry QW
// The split-diagonal body and the launcher are written over F.  The three streaming kernels spell the same products out (below).
// Ciphertext x ciphertext (database kinds 5 / 6): acc[slot][{d0,d1,d2}][j][c] = sum_{i<dim} rot[q][i] (x) db[g][i], Karatsuba
struct FormCtCt {
    static constexpr int qp = 2, dp = 2, sums = 3, comps = 3;  // sums: d0, d2, dk
    static constexpr const char *name = "tensor";
    static constexpr bool batch = true, bpp_arg = true;  // bpp_arg: the streaming kernel's template list names BPP
    static constexpr int max_qw = 2;                     // widest QW instantiated
    template <class A>
    DEV static void mac(typename A::Sum (&s)[3][2], const typename A::T (&a)[2][2], const typename A::T (&b)[2][2]) {
        kara_mac<A>(s, a, b);
    }
    DEV static void store(u64 *o, size_t ps, const ulonglong2 (&r)[3], u64 q) { store_karatsuba(o, ps, r[0], r[2], r[1], q); }
};
// The two plain forms: one side is NOT encrypted and has ONE encoded polynomial m per entry, so there are two sums instead of
// Karatsuba's three, four multiply-accumulates per lane pair against six with operand sums, and a 2-component accumulator that needs no
// relinearisation.  Bounds (tests/test_plain_gallery_model_cpu.py): every product is one canonical residue times one canonical
// residue, with no operand sums.
// - Halves24: every half is below 2^24 and every product below 2^48; ll and hh take one product per diagonal, mid two: 4096 diagonals
//   (the launcher's limit) x 2 x 2^48 = 2^61 < 2^63.
// - Sums128: the fold chunk of the encrypted form is kept.  It budgets a product at 2^(2k+2) (Karatsuba's operand sums); a plain
//   product of residues below q < 2^k is below 2^(2k), so the chunk is conservative by two bits: q + chunk 2^(2k) < 2^126.  The fold
//   path stays exercised on 59/60-bit limbs (every 128 / 32 diagonals).
struct FormPlain {
    static constexpr int sums = 2, comps = 2;
    static constexpr bool batch = false, bpp_arg = true;
    static constexpr int max_qw = 1;
    DEV static void store(u64 *o, size_t ps, const ulonglong2 (&r)[2], u64) {
        *reinterpret_cast<ulonglong2 *>(o) = r[0];
        *reinterpret_cast<ulonglong2 *>(o + ps) = r[1];
    }
};
// Ciphertext query x plain gallery (database kinds 7 / 8, DbLayout::plain; no counterpart in the reference):
//   acc[slot][p][j][c] = sum_{i<dim} rot[i].c_p[j][c] * m[g][i][j][c] mod q_j,  p = 0, 1
struct FormCtPlain : FormPlain {
    static constexpr int qp = 2, dp = 1;
    static constexpr const char *name = "plain";
    template <class A>
    DEV static void mac(typename A::Sum (&s)[2][2], const typename A::T (&a)[2][2], const typename A::T (&b)[1][2]) {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int e = 0; e < 2; e++) A::mac(s[p][e], a[p][e], b[0][e]);
    }
};
// Plain query x ciphertext database (kinds 5 / 6), the mirror image: rot holds the R evaluation-form rotations sigma_i(m) of the known
// probe as [R][nl][N] (k_automorph_batch), ONE polynomial each:
//   acc[slot][p][j][c] = sum_{i<R} rot[i][j][c] * db[g][i].c_p[j][c] mod q_j,  p = 0, 1
struct FormPlainCt : FormPlain {
    static constexpr int qp = 1, dp = 2;
    static constexpr const char *name = "pq";
    template <class A>
    DEV static void mac(typename A::Sum (&s)[2][2], const typename A::T (&a)[1][2], const typename A::T (&b)[2][2]) {
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int e = 0; e < 2; e++) A::mac(s[p][e], a[0][e], b[p][e]);
    }
};

// A BATCH of plain queries (k_hydia_pq_mq, k_hydia_pq_mq_sk): the same products for QW probes per pass, every probe with its own rotation
// set (rqs elements apart) and its OWN sums, so the bounds stated at FormPlain are unchanged — a sum still takes one product of two
// canonical residues per diagonal, whatever the number of queries beside it.  The batch has a tag of its own so that FormPlainCt (batch =
// false) and with it k_hydia_pq / k_hydia_pq_sk, their names and their code stay what they are; its streaming kernel serves one block
// per wave and has no BPP in its template list (bpp_arg)
struct FormPlainCtMq : FormPlainCt {
    static constexpr const char *name = "pq_mq";
    static constexpr bool batch = true, bpp_arg = false;
    static constexpr int max_qw = 4;
};

// A BATCH of encrypted queries against a plain gallery (k_hydia_plain_mq, k_hydia_plain_mq_sk): FormCtPlain's products for QW queries per
// pass, every query with its own rotation set (rqs elements apart) and its OWN two sums.  The bounds are FormPlain's, unchanged: a sum
// still takes one product of two canonical residues per diagonal, however many queries sit beside it.  A tag of its own, as
// FormPlainCtMq is, so that FormCtPlain (batch = false), k_hydia_plain / k_hydia_plain_sk, their names and their code stay what they
// are; one block per wave, no BPP in the streaming kernel's template list
struct FormCtPlainMq : FormCtPlain {
    static constexpr const char *name = "plain_mq";
    static constexpr bool batch = true, bpp_arg = false;
    static constexpr int max_qw = 4;
};

// The streaming kernels.  k_hydia_tensor, k_hydia_plain, k_hydia_pq, k_hydia_pq_mq and k_hydia_plain_mq hold the SAME pipeline (tile map,
// db_walk, rotating operand sets with the clamped re-fetch, one s_barrier per diagonal, fold, reduction, mq_slot store): a change to
// it is made in all five.
// It is written out in each entry point on purpose.  Called as one device function the pipeline is optimised twice, alone and again
// after inlining, and the second pass orders the multiply-accumulates differently: k_hydia_tensor<Halves24<true>, 1, 2, *> took 186 /
// 188 VGPRs instead of 164 (2 waves per SIMD instead of 3), k_hydia_pq<Halves24<true>, 2, *> 151 instead of 120 (3 instead of 4),
// k_hydia_plain / k_hydia_pq<Sums128<false>, 1, *> 77 / 78 instead of 70 / 72 (6 instead of 7) — profiles/loop_b_forms/README.md.
// Moving k_hydia_tensor's body into a function unchanged does the same to it.
//
// acc[slot][{d0,d1,d2}][j][c] = sum_{i<dim} rot[q][i] (x) db[g][i] for BPP database blocks x QW queries per wave (rot: the queries'
// rotation sets, rqs elements apart, from query q0 on).  One pass reads a database operand ONCE per diagonal for its QW queries.
//
// Work split (HBM must see the 3 GiB of rotated queries ONCE, not once per block): a workgroup owns one 128-coefficient tile of one
// limb and NW*BPP database blocks — each of its NW waves serves BPP blocks with one register copy of the rot operands, and the NW
// waves read the SAME rot addresses in step (one barrier per diagonal), so the per-CU vector cache serves NW-1 of them.  The
// database operands are streamed with non-temporal loads so they do not evict rot.  In the group-sequential layout a workgroup
// walks one group, one contiguous run.  grid (256 tiles * Gq, limbs j0..), Gq = G/(NW*BPP) block groups per tile.
// Registers: a wave holds BPP x QW accumulator sets; single queries take BPP = 2, batches QW = 2 (QW = 4 spilled).
// The operands of the next diagonal(s) are fetched while the current one's products run (A::depth sets: 2 + 4 BPP loads in flight
// instead of none during the multiply-accumulates; 27.2 -> 26.65 ms at 64 blocks for the 128-bit sums).
template <class A, int BPP, int QW, int NW>
__global__ __launch_bounds__(64 * NW, 2) void k_hydia_tensor(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot, size_t rqs,
                                                             const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                             int Gq, int xcd_map, DbLayout L, int j0, int G, int ng, int nblk, int q0, int Qt) {
    typedef typename A::T T;
    const int j = blockIdx.y + j0;
    // consecutive workgroup ids are dealt round-robin over the 8 XCDs: give every XCD its own tiles and let the Gq block
    // groups of one tile follow each other ON THAT XCD, so they find the tile's rot lines in its L2
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int gq = xcd_map ? k % Gq : blockIdx.x % Gq;
    const int tile = xcd_map ? xcd + 8 * (k / Gq) : blockIdx.x / Gq;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ModC M = mod[j];
    const size_t c = (size_t)tile * 128 + lane * 2;
    const size_t ps = (size_t)nl * N, cs = 2 * ps;  // rot / acc poly stride, ciphertext stride (elements)
    const int g0 = (gq * NW + wv) * BPP;
    const u64 *ra = rot + (size_t)q0 * rqs + (size_t)j * N + c;
    const DbWalk dw = db_walk(L, N, dim, j, tile, lane, g0, gq, wv * BPP);
    const unsigned char *da = db + dw.base;
    const A ar(M, dim, lane);
    typename A::Sum s[BPP][QW][3][2];  // [block][query][d0, d2, dk][coefficient of the lane's pair]
#pragma unroll
    for (int u = 0; u < BPP; u++)
#pragma unroll
        for (int q = 0; q < QW; q++)
#pragma unroll
            for (int k3 = 0; k3 < 3; k3++) s[u][q][k3][0] = s[u][q][k3][1] = typename A::Sum{};
    struct Operands {
        ulonglong2 a0[QW], a1[QW];
        typename A::Raw b0[BPP], b1[BPP];
    };
    auto fetch = [&](Operands &o, int i) {
#pragma unroll
        for (int q = 0; q < QW; q++) {
            o.a0[q] = *reinterpret_cast<const ulonglong2 *>(ra + q * rqs + (size_t)i * cs);
            o.a1[q] = *reinterpret_cast<const ulonglong2 *>(ra + q * rqs + (size_t)i * cs + ps);
        }
#pragma unroll
        for (int u = 0; u < BPP; u++) {
            o.b0[u].template load<true>(da + u * dw.su + (size_t)i * dw.si);
            o.b1[u].template load<true>(da + u * dw.su + (size_t)i * dw.si + dw.sp);
        }
    };
    auto accumulate = [&](const Operands &o) {
        // each query's operands once per diagonal, shared by the BPP blocks; each block's once (with the first query), shared by the QW
        // queries.  (This nesting keeps the 24-bit kernels at 164 VGPRs for BPP = 2 and for QW = 2; others took up to 206)
        T b[BPP][2][2];
#pragma unroll
        for (int q = 0; q < QW; q++) {
            const T a[2][2] = {{A::rot(o.a0[q].x), A::rot(o.a0[q].y)}, {A::rot(o.a1[q].x), A::rot(o.a1[q].y)}};
#pragma unroll
            for (int u = 0; u < BPP; u++) {
                if (q == 0) {
                    ar.cut(o.b0[u], b[u][0]);
                    ar.cut(o.b1[u], b[u][1]);
                }
                kara_mac<A>(s[u][q], a, b[u]);
            }
        }
    };
    if constexpr (A::depth == 3) {
        Operands S0, S1, S2;
        fetch(S0, 0);
        fetch(S1, 1);
        int i = 0;
        for (; i + 2 < dim; i += 3) {  // branch-free inside: clamped re-fetches of the last diagonal are never accumulated
            fetch(S2, i + 2);
            accumulate(S0);
            if (NW > 1) __builtin_amdgcn_s_barrier();  // keep the waves on the same diagonal (no memory wait implied)
            fetch(S0, i + 3 < dim ? i + 3 : dim - 1);
            accumulate(S1);
            if (NW > 1) __builtin_amdgcn_s_barrier();
            fetch(S1, i + 4 < dim ? i + 4 : dim - 1);
            accumulate(S2);
            if (NW > 1) __builtin_amdgcn_s_barrier();
        }
        if (i < dim) accumulate(S0);  // the one or two diagonals the groups of three leave over (workgroup-uniform)
        if (i + 1 < dim) accumulate(S1);
    } else {
        Operands cur, nxt;
        fetch(cur, 0);
        for (int i0 = 0; i0 < dim; i0 += ar.chunk) {
            const int i1 = i0 + ar.chunk < dim ? i0 + ar.chunk : dim;
            // dim (>= 2, checked at context creation) and every chunk are powers of two: even.  No branch inside the loop: at a join the
            // compiler waits for every outstanding load, the prefetched ones included
            for (int i = i0; i < i1; i += 2) {
                fetch(nxt, i + 1);
                accumulate(cur);
                if (NW > 1) __builtin_amdgcn_s_barrier();
                fetch(cur, i + 2 < dim ? i + 2 : i + 1);  // the last one re-reads a line that is in flight: never used
                accumulate(nxt);
                if (NW > 1) __builtin_amdgcn_s_barrier();
            }
            if (i1 < dim) {
#pragma unroll
                for (int u = 0; u < BPP; u++)
#pragma unroll
                    for (int q = 0; q < QW; q++)
#pragma unroll
                        for (int k3 = 0; k3 < 3; k3++) {
                            A::fold(s[u][q][k3][0], M);
                            A::fold(s[u][q][k3][1], M);
                        }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < BPP; u++)
#pragma unroll
        for (int q = 0; q < QW; q++) {
            ulonglong2 r[3];
#pragma unroll
            for (int k3 = 0; k3 < 3; k3++) r[k3] = make_ulonglong2(A::reduce(s[u][q][k3][0], M), A::reduce(s[u][q][k3][1], M));
            store_karatsuba(acc + (mq_slot(q0 + q, g0 + u, G, ng, nblk, Qt) * 3 * nl + j) * N + c, ps, r[0], r[2], r[1], M.q);
        }
}

// The split-diagonal body of every form, for limb 0 of SMALL ciphertext-major databases (at most 8 blocks on this GPU): the streaming
// kernel's limb-0 launch has only 256 x G waves, each walking all `dim` diagonals — latency-bound (0.6 ms at G = 1 for 0.5 GB).  Here
// KS waves of a workgroup share one (block, tile) and take every KS-th diagonal for QW queries; the partial sums are reduced modulo
// q_0 through LDS, one query at a time.  Same residues as the one-wave kernel (a sum modulo q does not depend on how it is split).
// grid (N/128 * G, 1)
template <class F, int KS, int QW>
DEV void loop_b_split(const ModC *mod, int N, const u64 *rot, size_t rqs, const unsigned char *db,
                      u64 *acc, int dim, int nl, const DbLayout &L, int G, int ng, int nblk, int q0, int Qt) {
    typedef Sums128<false> A;
    constexpr int NS = 2 * F::sums;  // sums of a lane: [sum of the form][coefficient of its pair]
    __shared__ u64 part[KS][NS][64];
    static_assert(sizeof(part) == (F::sums == 3 ? 3072 : 2048) * KS, "24 / 12 KiB of LDS for the encrypted form, 16 / 8 KiB for the plain ones");
    const int tiles = N / 128;
    const int tile = blockIdx.x % tiles, g = blockIdx.x / tiles;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ModC M = mod[0];
    const size_t c = (size_t)tile * 128 + lane * 2;
    const size_t ps = (size_t)nl * N, cs = F::qp * ps;
    const u64 *ra = rot + (size_t)q0 * rqs + c;
    const unsigned char *da = db + (size_t)g * dim * L.ct_bytes + c * 8;
    const A ar(M, dim, lane);
    u128 s[QW][F::sums][2] = {};
    int since = 0;
    for (int i = wv; i < dim; i += KS) {
        A::Raw r[F::dp];
#pragma unroll
        for (int p = 0; p < F::dp; p++) r[p].template load<true>(da + (size_t)i * L.ct_bytes + p * L.poly_bytes);
        u64 b[F::dp][2];
#pragma unroll
        for (int p = 0; p < F::dp; p++) ar.cut(r[p], b[p]);
#pragma unroll
        for (int q = 0; q < QW; q++) {
            u64 a[F::qp][2];
#pragma unroll
            for (int p = 0; p < F::qp; p++) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(ra + q * rqs + (size_t)i * cs + p * ps);
                a[p][0] = v.x;
                a[p][1] = v.y;
            }
            F::template mac<A>(s[q], a, b);
        }
        if (++since == ar.chunk) {  // the fold interval counts this wave's diagonals
            since = 0;
#pragma unroll
            for (int q = 0; q < QW; q++)
#pragma unroll
                for (int k = 0; k < NS; k++) A::fold(s[q][k / 2][k % 2], M);
        }
    }
#pragma unroll
    for (int q = 0; q < QW; q++) {
#pragma unroll
        for (int k = 0; k < NS; k++) part[wv][k][lane] = A::reduce(s[q][k / 2][k % 2], M);
        __syncthreads();
        if (wv == 0) {
            ulonglong2 r[F::sums];
#pragma unroll
            for (int k = 0; k < F::sums; k++) {
                u64 t0 = part[0][2 * k][lane], t1 = part[0][2 * k + 1][lane];
                for (int w = 1; w < KS; w++) {
                    t0 = addmod(t0, part[w][2 * k][lane], M.q);
                    t1 = addmod(t1, part[w][2 * k + 1][lane], M.q);
                }
                r[k] = make_ulonglong2(t0, t1);
            }
            F::store(acc + mq_slot(q0 + q, g, G, ng, nblk, Qt) * F::comps * nl * N + c, ps, r, M.q);
        }
        if (q + 1 < QW) __syncthreads();  // the next query reuses part
    }
}


// The three split-diagonal entry points: the names rocprofv3 prints and the byte ledger records
template <int KS, int QW>
__global__ __launch_bounds__(64 * KS) void k_hydia_tensor_sk(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot, size_t rqs,
                                                             const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                             DbLayout L, int G, int ng, int nblk, int q0, int Qt) {
    loop_b_split<FormCtCt, KS, QW>(mod, N, rot, rqs, db, acc, dim, nl, L, G, ng, nblk, q0, Qt);
}
template <int KS>
__global__ __launch_bounds__(64 * KS) void k_hydia_plain_sk(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot,
                                                            const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                            DbLayout L, int G, int ng, int nblk) {
    loop_b_split<FormCtPlain, KS, 1>(mod, N, rot, 0, db, acc, dim, nl, L, G, ng, nblk, 0, 1);
}
template <int KS>
__global__ __launch_bounds__(64 * KS) void k_hydia_pq_sk(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot,
                                                         const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                         DbLayout L, int G, int ng, int nblk) {
    loop_b_split<FormPlainCt, KS, 1>(mod, N, rot, 0, db, acc, dim, nl, L, G, ng, nblk, 0, 1);
}

// ------------------------------------------------------------------------------------------------ loop B for a plain gallery
// FormCtPlain as a streaming kernel: k_hydia_tensor's pipeline with one database operand per diagonal, two sums and a 2-component
// accumulator; the arithmetic policies are used as they are (bounds: at the forms)
template <class A, int BPP, int NW>
__global__ __launch_bounds__(64 * NW, 2) void k_hydia_plain(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot,
                                                            const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                            int Gq, int xcd_map, DbLayout L, int j0, int G, int ng, int nblk) {
    typedef typename A::T T;
    const int j = blockIdx.y + j0;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int gq = xcd_map ? k % Gq : blockIdx.x % Gq;
    const int tile = xcd_map ? xcd + 8 * (k / Gq) : blockIdx.x / Gq;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ModC M = mod[j];
    const size_t c = (size_t)tile * 128 + lane * 2;
    const size_t ps = (size_t)nl * N, cs = 2 * ps;  // rot / acc poly stride, ciphertext stride (elements)
    const int g0 = (gq * NW + wv) * BPP;
    const u64 *ra = rot + (size_t)j * N + c;
    const DbWalk dw = db_walk(L, N, dim, j, tile, lane, g0, gq, wv * BPP);
    const unsigned char *da = db + dw.base;
    const A ar(M, dim, lane);
    typename A::Sum s[BPP][2][2];  // [block][component][coefficient of the lane's pair]
#pragma unroll
    for (int u = 0; u < BPP; u++)
#pragma unroll
        for (int p = 0; p < 2; p++) s[u][p][0] = s[u][p][1] = typename A::Sum{};
    struct Operands {
        ulonglong2 a0, a1;
        typename A::Raw b[BPP];
    };
    auto fetch = [&](Operands &o, int i) {
        o.a0 = *reinterpret_cast<const ulonglong2 *>(ra + (size_t)i * cs);
        o.a1 = *reinterpret_cast<const ulonglong2 *>(ra + (size_t)i * cs + ps);
#pragma unroll
        for (int u = 0; u < BPP; u++) o.b[u].template load<true>(da + u * dw.su + (size_t)i * dw.si);
    };
    auto accumulate = [&](const Operands &o) {
        const T a[2][2] = {{A::rot(o.a0.x), A::rot(o.a0.y)}, {A::rot(o.a1.x), A::rot(o.a1.y)}};
#pragma unroll
        for (int u = 0; u < BPP; u++) {
            T b[2];
            ar.cut(o.b[u], b);
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int e = 0; e < 2; e++) A::mac(s[u][p][e], a[p][e], b[e]);
        }
    };
    if constexpr (A::depth == 3) {
        Operands S0, S1, S2;
        fetch(S0, 0);
        fetch(S1, 1);
        int i = 0;
        for (; i + 2 < dim; i += 3) {  // branch-free inside: clamped re-fetches of the last diagonal are never accumulated
            fetch(S2, i + 2);
            accumulate(S0);
            if (NW > 1) __builtin_amdgcn_s_barrier();  // keep the waves on the same diagonal (no memory wait implied)
            fetch(S0, i + 3 < dim ? i + 3 : dim - 1);
            accumulate(S1);
            if (NW > 1) __builtin_amdgcn_s_barrier();
            fetch(S1, i + 4 < dim ? i + 4 : dim - 1);
            accumulate(S2);
            if (NW > 1) __builtin_amdgcn_s_barrier();
        }
        if (i < dim) accumulate(S0);
        if (i + 1 < dim) accumulate(S1);
    } else {
        Operands cur, nxt;
        fetch(cur, 0);
        for (int i0 = 0; i0 < dim; i0 += ar.chunk) {
            const int i1 = i0 + ar.chunk < dim ? i0 + ar.chunk : dim;
            for (int i = i0; i < i1; i += 2) {  // dim and every chunk are even (k_hydia_tensor)
                fetch(nxt, i + 1);
                accumulate(cur);
                if (NW > 1) __builtin_amdgcn_s_barrier();
                fetch(cur, i + 2 < dim ? i + 2 : i + 1);
                accumulate(nxt);
                if (NW > 1) __builtin_amdgcn_s_barrier();
            }
            if (i1 < dim) {
#pragma unroll
                for (int u = 0; u < BPP; u++)
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        A::fold(s[u][p][0], M);
                        A::fold(s[u][p][1], M);
                    }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < BPP; u++) {
        u64 *o = acc + (mq_slot(0, g0 + u, G, ng, nblk, 1) * 2 * nl + j) * N + c;
#pragma unroll
        for (int p = 0; p < 2; p++)
            *reinterpret_cast<ulonglong2 *>(o + p * ps) = make_ulonglong2(A::reduce(s[u][p][0], M), A::reduce(s[u][p][1], M));
    }
}
// ------------------------------------------------------------------------------------------------ loop B for a plain query
// FormPlainCt as a streaming kernel: k_hydia_tensor's pipeline with ONE query operand (rot is [R][nl][N]) and two database operands per
// diagonal and block, two sums and a 2-component accumulator; the arithmetic policies are used as they are (bounds: at the forms)
template <class A, int BPP, int NW>
__global__ __launch_bounds__(64 * NW, 2) void k_hydia_pq(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot,
                                                         const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                         int Gq, int xcd_map, DbLayout L, int j0, int G, int ng, int nblk) {
    typedef typename A::T T;
    const int j = blockIdx.y + j0;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int gq = xcd_map ? k % Gq : blockIdx.x % Gq;
    const int tile = xcd_map ? xcd + 8 * (k / Gq) : blockIdx.x / Gq;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ModC M = mod[j];
    const size_t c = (size_t)tile * 128 + lane * 2;
    const size_t ps = (size_t)nl * N;  // rot stride per rotation = acc poly stride (elements)
    const int g0 = (gq * NW + wv) * BPP;
    const u64 *ra = rot + (size_t)j * N + c;
    const DbWalk dw = db_walk(L, N, dim, j, tile, lane, g0, gq, wv * BPP);
    const unsigned char *da = db + dw.base;
    const A ar(M, dim, lane);
    typename A::Sum s[BPP][2][2];  // [block][component][coefficient of the lane's pair]
#pragma unroll
    for (int u = 0; u < BPP; u++)
#pragma unroll
        for (int p = 0; p < 2; p++) s[u][p][0] = s[u][p][1] = typename A::Sum{};
    struct Operands {
        ulonglong2 a;
        typename A::Raw b0[BPP], b1[BPP];
    };
    auto fetch = [&](Operands &o, int i) {
        o.a = *reinterpret_cast<const ulonglong2 *>(ra + (size_t)i * ps);
#pragma unroll
        for (int u = 0; u < BPP; u++) {
            o.b0[u].template load<true>(da + u * dw.su + (size_t)i * dw.si);
            o.b1[u].template load<true>(da + u * dw.su + (size_t)i * dw.si + dw.sp);
        }
    };
    auto accumulate = [&](const Operands &o) {
        const T a[2] = {A::rot(o.a.x), A::rot(o.a.y)};
#pragma unroll
        for (int u = 0; u < BPP; u++) {
            T b[2][2];
            ar.cut(o.b0[u], b[0]);
            ar.cut(o.b1[u], b[1]);
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int e = 0; e < 2; e++) A::mac(s[u][p][e], a[e], b[p][e]);
        }
    };
    if constexpr (A::depth == 3) {
        Operands S0, S1, S2;
        fetch(S0, 0);
        fetch(S1, 1);
        int i = 0;
        for (; i + 2 < dim; i += 3) {  // branch-free inside: clamped re-fetches of the last diagonal are never accumulated
            fetch(S2, i + 2);
            accumulate(S0);
            if (NW > 1) __builtin_amdgcn_s_barrier();  // keep the waves on the same diagonal (no memory wait implied)
            fetch(S0, i + 3 < dim ? i + 3 : dim - 1);
            accumulate(S1);
            if (NW > 1) __builtin_amdgcn_s_barrier();
            fetch(S1, i + 4 < dim ? i + 4 : dim - 1);
            accumulate(S2);
            if (NW > 1) __builtin_amdgcn_s_barrier();
        }
        if (i < dim) accumulate(S0);
        if (i + 1 < dim) accumulate(S1);
    } else {
        Operands cur, nxt;
        fetch(cur, 0);
        for (int i0 = 0; i0 < dim; i0 += ar.chunk) {
            const int i1 = i0 + ar.chunk < dim ? i0 + ar.chunk : dim;
            for (int i = i0; i < i1; i += 2) {  // dim and every chunk are even (k_hydia_tensor)
                fetch(nxt, i + 1);
                accumulate(cur);
                if (NW > 1) __builtin_amdgcn_s_barrier();
                fetch(cur, i + 2 < dim ? i + 2 : i + 1);
                accumulate(nxt);
                if (NW > 1) __builtin_amdgcn_s_barrier();
            }
            if (i1 < dim) {
#pragma unroll
                for (int u = 0; u < BPP; u++)
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        A::fold(s[u][p][0], M);
                        A::fold(s[u][p][1], M);
                    }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < BPP; u++) {
        u64 *o = acc + (mq_slot(0, g0 + u, G, ng, nblk, 1) * 2 * nl + j) * N + c;
#pragma unroll
        for (int p = 0; p < 2; p++)
            *reinterpret_cast<ulonglong2 *>(o + p * ps) = make_ulonglong2(A::reduce(s[u][p][0], M), A::reduce(s[u][p][1], M));
    }
}
// ------------------------------------------------------------------------------------------------ loop B for a batch of plain queries
// k_hydia_pq's pipeline with a query dimension added the way k_hydia_tensor has one, at ONE block per wave: rot holds the queries'
// rotation sets [R][nl][N], rqs elements apart, from query q0 on.  A database operand is loaded and cut once per diagonal and shared by
// the QW queries; each query's operand is loaded once.  Every query has its own two sums, so the bounds are FormPlain's, unchanged.
// The store goes through mq_slot into [slot][2][nl][N] (Qt = queries of the whole batch).  QW = 4 on eight-wave workgroups asks for one
// workgroup per CU: at two the 128 registers a lane may then hold do not take four queries' sums
template <class A, int QW, int NW>
__global__ __launch_bounds__(64 * NW, (QW >= 4 && NW >= 8) ? 1 : 2) void k_hydia_pq_mq(
    const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot, size_t rqs, const unsigned char *__restrict__ db, u64 *__restrict__ acc,
    int dim, int nl, int Gq, int xcd_map, DbLayout L, int j0, int G, int ng, int nblk, int q0, int Qt) {
    typedef typename A::T T;
    const int j = blockIdx.y + j0;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int gq = xcd_map ? k % Gq : blockIdx.x % Gq;
    const int tile = xcd_map ? xcd + 8 * (k / Gq) : blockIdx.x / Gq;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ModC M = mod[j];
    const size_t c = (size_t)tile * 128 + lane * 2;
    const size_t ps = (size_t)nl * N;  // rot stride per rotation = acc poly stride (elements)
    const int g = gq * NW + wv;        // the wave's block
    const u64 *ra = rot + (size_t)q0 * rqs + (size_t)j * N + c;
    const DbWalk dw = db_walk(L, N, dim, j, tile, lane, g, gq, wv);
    const unsigned char *da = db + dw.base;
    const A ar(M, dim, lane);
    typename A::Sum s[QW][2][2];  // [query][component][coefficient of the lane's pair]
#pragma unroll
    for (int q = 0; q < QW; q++)
#pragma unroll
        for (int p = 0; p < 2; p++) s[q][p][0] = s[q][p][1] = typename A::Sum{};
    struct Operands {
        ulonglong2 a[QW];
        typename A::Raw b0, b1;
    };
    auto fetch = [&](Operands &o, int i) {
#pragma unroll
        for (int q = 0; q < QW; q++) o.a[q] = *reinterpret_cast<const ulonglong2 *>(ra + q * rqs + (size_t)i * ps);
        o.b0.template load<true>(da + (size_t)i * dw.si);
        o.b1.template load<true>(da + (size_t)i * dw.si + dw.sp);
    };
    auto accumulate = [&](const Operands &o) {
        T b[2][2];
#pragma unroll
        for (int q = 0; q < QW; q++) {
            const T a[2] = {A::rot(o.a[q].x), A::rot(o.a[q].y)};
            if (q == 0) {  // (k_hydia_tensor's nesting: the block's operands are cut with the first query)
                ar.cut(o.b0, b[0]);
                ar.cut(o.b1, b[1]);
            }
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int e = 0; e < 2; e++) A::mac(s[q][p][e], a[e], b[p][e]);
        }
    };
    if constexpr (A::depth == 3) {
        Operands S0, S1, S2;
        fetch(S0, 0);
        fetch(S1, 1);
        int i = 0;
        for (; i + 2 < dim; i += 3) {  // branch-free inside: clamped re-fetches of the last diagonal are never accumulated
            fetch(S2, i + 2);
            accumulate(S0);
            if (NW > 1) __builtin_amdgcn_s_barrier();  // keep the waves on the same diagonal (no memory wait implied)
            fetch(S0, i + 3 < dim ? i + 3 : dim - 1);
            accumulate(S1);
            if (NW > 1) __builtin_amdgcn_s_barrier();
            fetch(S1, i + 4 < dim ? i + 4 : dim - 1);
            accumulate(S2);
            if (NW > 1) __builtin_amdgcn_s_barrier();
        }
        if (i < dim) accumulate(S0);
        if (i + 1 < dim) accumulate(S1);
    } else {
        Operands cur, nxt;
        fetch(cur, 0);
        for (int i0 = 0; i0 < dim; i0 += ar.chunk) {
            const int i1 = i0 + ar.chunk < dim ? i0 + ar.chunk : dim;
            for (int i = i0; i < i1; i += 2) {  // dim and every chunk are even (k_hydia_tensor)
                fetch(nxt, i + 1);
                accumulate(cur);
                if (NW > 1) __builtin_amdgcn_s_barrier();
                fetch(cur, i + 2 < dim ? i + 2 : i + 1);
                accumulate(nxt);
                if (NW > 1) __builtin_amdgcn_s_barrier();
            }
            if (i1 < dim) {
#pragma unroll
                for (int q = 0; q < QW; q++)
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        A::fold(s[q][p][0], M);
                        A::fold(s[q][p][1], M);
                    }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < QW; q++) {
        u64 *o = acc + (mq_slot(q0 + q, g, G, ng, nblk, Qt) * 2 * nl + j) * N + c;
#pragma unroll
        for (int p = 0; p < 2; p++)
            *reinterpret_cast<ulonglong2 *>(o + p * ps) = make_ulonglong2(A::reduce(s[q][p][0], M), A::reduce(s[q][p][1], M));
    }
}
// its split-diagonal entry (limb 0 of small ciphertext-major databases).  The body is instantiated on the batch's own tag, which is
// FormPlainCt in everything the body reads, so that loop_b_split<FormPlainCt, KS, 1> keeps k_hydia_pq_sk as its only caller and that
// kernel's code stays what it is
template <int KS, int QW>
__global__ __launch_bounds__(64 * KS) void k_hydia_pq_mq_sk(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot, size_t rqs,
                                                            const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                            DbLayout L, int G, int ng, int nblk, int q0, int Qt) {
    loop_b_split<FormPlainCtMq, KS, QW>(mod, N, rot, rqs, db, acc, dim, nl, L, G, ng, nblk, q0, Qt);
}
// ------------------------------------------------------------------------------------------------ loop B for a batch on a plain gallery
// k_hydia_plain's pipeline with the query dimension k_hydia_pq_mq has, at ONE block per wave: rot holds the queries' rotation sets
// [R][2][nl][N], rqs elements apart, from query q0 on.  The gallery operand (one polynomial) is loaded and cut once per diagonal, with
// the first query, and shared by the QW queries; each query's two operands are loaded once.  Every query has its own two sums, so the
// bounds are FormPlain's, unchanged.  The store goes through mq_slot into [slot][2][nl][N] (Qt = queries of the whole batch).  QW = 4
// on eight-wave workgroups asks for one workgroup per CU, as k_hydia_pq_mq does
template <class A, int QW, int NW>
__global__ __launch_bounds__(64 * NW, (QW >= 4 && NW >= 8) ? 1 : 2) void k_hydia_plain_mq(
    const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot, size_t rqs, const unsigned char *__restrict__ db, u64 *__restrict__ acc,
    int dim, int nl, int Gq, int xcd_map, DbLayout L, int j0, int G, int ng, int nblk, int q0, int Qt) {
    typedef typename A::T T;
    const int j = blockIdx.y + j0;
    const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
    const int gq = xcd_map ? k % Gq : blockIdx.x % Gq;
    const int tile = xcd_map ? xcd + 8 * (k / Gq) : blockIdx.x / Gq;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ModC M = mod[j];
    const size_t c = (size_t)tile * 128 + lane * 2;
    const size_t ps = (size_t)nl * N, cs = 2 * ps;  // rot / acc poly stride, ciphertext stride (elements)
    const int g = gq * NW + wv;                     // the wave's block
    const u64 *ra = rot + (size_t)q0 * rqs + (size_t)j * N + c;
    const DbWalk dw = db_walk(L, N, dim, j, tile, lane, g, gq, wv);
    const unsigned char *da = db + dw.base;
    const A ar(M, dim, lane);
    typename A::Sum s[QW][2][2];  // [query][component][coefficient of the lane's pair]
#pragma unroll
    for (int q = 0; q < QW; q++)
#pragma unroll
        for (int p = 0; p < 2; p++) s[q][p][0] = s[q][p][1] = typename A::Sum{};
    struct Operands {
        ulonglong2 a0[QW], a1[QW];
        typename A::Raw b;
    };
    auto fetch = [&](Operands &o, int i) {
#pragma unroll
        for (int q = 0; q < QW; q++) {
            o.a0[q] = *reinterpret_cast<const ulonglong2 *>(ra + q * rqs + (size_t)i * cs);
            o.a1[q] = *reinterpret_cast<const ulonglong2 *>(ra + q * rqs + (size_t)i * cs + ps);
        }
        o.b.template load<true>(da + (size_t)i * dw.si);
    };
    auto accumulate = [&](const Operands &o) {
        T b[2];
#pragma unroll
        for (int q = 0; q < QW; q++) {
            const T a[2][2] = {{A::rot(o.a0[q].x), A::rot(o.a0[q].y)}, {A::rot(o.a1[q].x), A::rot(o.a1[q].y)}};
            if (q == 0) ar.cut(o.b, b);  // (k_hydia_tensor's nesting: the block's operand is cut with the first query)
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int e = 0; e < 2; e++) A::mac(s[q][p][e], a[p][e], b[e]);
        }
    };
    if constexpr (A::depth == 3) {
        Operands S0, S1, S2;
        fetch(S0, 0);
        fetch(S1, 1);
        int i = 0;
        for (; i + 2 < dim; i += 3) {  // branch-free inside: clamped re-fetches of the last diagonal are never accumulated
            fetch(S2, i + 2);
            accumulate(S0);
            if (NW > 1) __builtin_amdgcn_s_barrier();  // keep the waves on the same diagonal (no memory wait implied)
            fetch(S0, i + 3 < dim ? i + 3 : dim - 1);
            accumulate(S1);
            if (NW > 1) __builtin_amdgcn_s_barrier();
            fetch(S1, i + 4 < dim ? i + 4 : dim - 1);
            accumulate(S2);
            if (NW > 1) __builtin_amdgcn_s_barrier();
        }
        if (i < dim) accumulate(S0);
        if (i + 1 < dim) accumulate(S1);
    } else {
        Operands cur, nxt;
        fetch(cur, 0);
        for (int i0 = 0; i0 < dim; i0 += ar.chunk) {
            const int i1 = i0 + ar.chunk < dim ? i0 + ar.chunk : dim;
            for (int i = i0; i < i1; i += 2) {  // dim and every chunk are even (k_hydia_tensor)
                fetch(nxt, i + 1);
                accumulate(cur);
                if (NW > 1) __builtin_amdgcn_s_barrier();
                fetch(cur, i + 2 < dim ? i + 2 : i + 1);
                accumulate(nxt);
                if (NW > 1) __builtin_amdgcn_s_barrier();
            }
            if (i1 < dim) {
#pragma unroll
                for (int q = 0; q < QW; q++)
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        A::fold(s[q][p][0], M);
                        A::fold(s[q][p][1], M);
                    }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < QW; q++) {
        u64 *o = acc + (mq_slot(q0 + q, g, G, ng, nblk, Qt) * 2 * nl + j) * N + c;
#pragma unroll
        for (int p = 0; p < 2; p++)
            *reinterpret_cast<ulonglong2 *>(o + p * ps) = make_ulonglong2(A::reduce(s[q][p][0], M), A::reduce(s[q][p][1], M));
    }
}
// its split-diagonal entry (limb 0 of small ciphertext-major galleries), on the batch's own tag, so that loop_b_split<FormCtPlain, KS, 1>
// keeps k_hydia_plain_sk as its only caller and that kernel's code stays what it is
template <int KS, int QW>
__global__ __launch_bounds__(64 * KS) void k_hydia_plain_mq_sk(const ModC *__restrict__ mod, int N, const u64 *__restrict__ rot, size_t rqs,
                                                               const unsigned char *__restrict__ db, u64 *__restrict__ acc, int dim, int nl,
                                                               DbLayout L, int G, int ng, int nblk, int q0, int Qt) {
    loop_b_split<FormCtPlainMq, KS, QW>(mod, N, rot, rqs, db, acc, dim, nl, L, G, ng, nblk, q0, Qt);
}
// The R rotations of a plaintext in ONE launch: out[i][j][co] = m[j][perm_{g_i}(co)] (the gather form of the evaluation-form
// automorphism, k_moddown_combine's index map), galois[i] = 5^i mod 2N, identity for g = 1 (rotation 0).  grid (N/256, nl, R)
__global__ __launch_bounds__(256) void k_automorph_batch(int logN, const u64 *__restrict__ m, u64 *__restrict__ out, int nl,
                                                         const unsigned *__restrict__ galois) {
    const unsigned N = 1u << logN;
    const int j = blockIdx.y, i = blockIdx.z;
    const unsigned co = blockIdx.x * 256 + threadIdx.x, g = galois[i];
    unsigned c = co;
    if (g != 1u) {
        const unsigned e = ((2u * brev_n(co, logN) + 1u) * g) & (2u * N - 1u);
        c = brev_n((e - 1u) >> 1, logN);
    }
    out[((size_t)i * nl + j) * N + co] = m[(size_t)j * N + c];
}

// unpacked [X][np][nQ][N] u64  <->  database layout (np = db_polys(L): 2, or 1 for a plain gallery).  grid (N/512, nQ, X*np)
template <bool PACK>
__global__ __launch_bounds__(256) void k_db_repack(int N, int nQ, u64 *__restrict__ plain, unsigned char *__restrict__ db,
                                                   DbLayout L, size_t t0) {
    const int j = blockIdx.y, xp = blockIdx.z, x = L.plain ? xp : xp >> 1, p = L.plain ? 0 : xp & 1;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    u64 *pl = plain + ((size_t)xp * nQ + j) * N + c;
    const bool pk = L.packed && j > 0;
    unsigned char *d = db + db_offset(L, N, t0 + x, p, j, c);
    typedef unsigned int u3 __attribute__((ext_vector_type(3), aligned(4)));
    if (PACK) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(pl);
        if (pk) {
            u3 w;
            w.x = (unsigned)v.x;
            w.y = (unsigned)(v.x >> 32) | ((unsigned)v.y << 16);
            w.z = (unsigned)(v.y >> 16);
            *reinterpret_cast<u3 *>(d) = w;
        } else {
            *reinterpret_cast<ulonglong2 *>(d) = v;
        }
    } else {
        *reinterpret_cast<ulonglong2 *>(pl) = pk ? db_load2<true, false>(d) : db_load2<false, false>(d);
    }
}

// the 46-bit limbs of a bits46 layout: a thread moves SIXTEEN residues = 23 dwords (the granule that starts on a dword).
// grid (N/4096, nQ - 1, X*np): limb j = blockIdx.y + 1
template <bool PACK>
__global__ __launch_bounds__(256) void k_db_repack46(int N, int nQ, u64 *__restrict__ plain, unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y + 1, xp = blockIdx.z, x = L.plain ? xp : xp >> 1, p = L.plain ? 0 : xp & 1;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 16;
    if (c >= (size_t)N) return;
    u64 *pl = plain + ((size_t)xp * nQ + j) * N + c;
    unsigned *d = reinterpret_cast<unsigned *>(db + db_offset(L, N, t0 + x, p, j, c));
    unsigned w[24];
    if (PACK) {
#pragma unroll
        for (int k = 0; k < 24; k++) w[k] = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const u64 v = pl[r] & ((1ull << 46) - 1);
            const int bit = 46 * r, di = bit >> 5, sh = bit & 31;
            w[di] |= (unsigned)(v << sh);
            w[di + 1] |= (unsigned)(sh ? v >> (32 - sh) : v >> 32);
            if (sh > 18) w[di + 2] |= (unsigned)(v >> (64 - sh));  // 46 + sh > 64: the field reaches a third dword
        }
#pragma unroll
        for (int k = 0; k < 23; k++) d[k] = w[k];
    } else {
#pragma unroll
        for (int k = 0; k < 23; k++) w[k] = d[k];
        w[23] = 0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int bit = 46 * r, di = bit >> 5, sh = bit & 31;
            u64 v = ((u64)w[di] >> sh) | ((u64)w[di + 1] << (32 - sh));
            if (sh > 18) v |= (u64)w[di + 2] << (64 - sh);
            pl[r] = v & ((1ull << 46) - 1);
        }
    }
}

// In-place update of the resident database: ciphertexts t0 .. t0+X-1 += fresh [X][2][nQ][N] residues, mod q_j.  Fused
// read-add-reduce-write on k_db_repack's thread-to-bytes map (a residue pair per thread): every resident byte is read and written
// once by the one thread that owns it, so no atomics and no unpacked copy of the block in HBM.  grid (N/512, nQ or 1, X*2)
__global__ __launch_bounds__(256) void k_db_accumulate(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ plain,
                                                       unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y, xp = blockIdx.z, x = xp >> 1, p = xp & 1;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(plain + ((size_t)xp * nQ + j) * N + c);
    db_accumulate_pair(db + db_offset(L, N, t0 + x, p, j, c), L.packed && j > 0, a.x, a.y, mod[j].q);
}
// ... the 46-bit limbs of a bits46 layout on k_db_repack46's map: a thread owns SIXTEEN residues = 23 whole dwords.  The sums are
// reduced before they are packed (two residues below a prime above 2^45 can add up to more than 2^46).
// grid (N/4096, nQ - 1, X*2): limb j = blockIdx.y + 1
__global__ __launch_bounds__(256) void k_db_accumulate46(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ plain,
                                                         unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y + 1, xp = blockIdx.z, x = xp >> 1, p = xp & 1;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 16;
    if (c >= (size_t)N) return;
    const u64 *pl = plain + ((size_t)xp * nQ + j) * N + c;
    u64 a[16];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(pl + r);
        a[r] = v.x;
        a[r + 1] = v.y;
    }
    db_accumulate_granule46(reinterpret_cast<unsigned *>(db + db_offset(L, N, t0 + x, p, j, c)), a, mod[j].q);
}
// In-place update of a PLAIN gallery (one polynomial per entry): plaintexts t0 .. t0+X-1 += fresh [X][nQ][N] residues, mod q_j, on the
// same thread-to-bytes map and with the same arithmetic (db_accum.h).  Kernels of their own, so the ciphertext kernels above keep their
// code.  grid (N/512, nQ or 1, X)
__global__ __launch_bounds__(256) void k_plain_db_accumulate(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ plain,
                                                             unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y, x = blockIdx.z;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(plain + ((size_t)x * nQ + j) * N + c);
    db_accumulate_pair(db + db_offset(L, N, t0 + x, 0, j, c), L.packed && j > 0, a.x, a.y, mod[j].q);
}
// ... the 46-bit limbs of a bits46 gallery.  grid (N/4096, nQ - 1, X): limb j = blockIdx.y + 1
__global__ __launch_bounds__(256) void k_plain_db_accumulate46(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ plain,
                                                               unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y + 1, x = blockIdx.z;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 16;
    if (c >= (size_t)N) return;
    const u64 *pl = plain + ((size_t)x * nQ + j) * N + c;
    u64 a[16];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(pl + r);
        a[r] = v.x;
        a[r + 1] = v.y;
    }
    db_accumulate_granule46(reinterpret_cast<unsigned *>(db + db_offset(L, N, t0 + x, 0, j, c)), a, mod[j].q);
}
// Loading a plain gallery from an untrusted file: are the unpacked residues plain [X][nQ][N] canonical (< q_j)?  A flag reduction: a
// workgroup that saw a residue at or above its modulus sets *flag (never cleared here).  grid (N/512, nQ, X)
__global__ __launch_bounds__(256) void k_db_check_canonical(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ plain,
                                                            unsigned *__restrict__ flag) {
    const int j = blockIdx.y, x = blockIdx.z;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(plain + ((size_t)x * nQ + j) * N + c);
    const u64 q = mod[j].q;
    if (__syncthreads_or(a.x >= q || a.y >= q) && threadIdx.x == 0) *flag = 1u;
}

// Re-keying the resident database (Context::db_rekey): polynomial 1 ALONE of ciphertexts t0 .. t0+X-1 out of the resident layout into
// out [X][nQ][N] u64 — the key switch's c1 operand — on k_db_repack<false>'s thread-to-bytes map; polynomial 0 is never unpacked (the
// store below adds to it where it lies).  grid (N/512, nQ or 1, X)
__global__ __launch_bounds__(256) void k_db_gather_poly(int N, int nQ, u64 *__restrict__ out, const unsigned char *__restrict__ db,
                                                        DbLayout L, size_t t0) {
    const int j = blockIdx.y, x = blockIdx.z;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const unsigned char *d = db + db_offset(L, N, t0 + x, 1, j, c);
    *reinterpret_cast<ulonglong2 *>(out + ((size_t)x * nQ + j) * N + c) = (L.packed && j > 0) ? db_load2<true, false>(d) : db_load2<false, false>(d);
}
// ... the 46-bit limbs of a bits46 layout on k_db_repack46<false>'s map (sixteen residues = 23 dwords per thread).
// grid (N/4096, nQ - 1, X): limb j = blockIdx.y + 1
__global__ __launch_bounds__(256) void k_db_gather_poly46(int N, int nQ, u64 *__restrict__ out, const unsigned char *__restrict__ db,
                                                          DbLayout L, size_t t0) {
    const int j = blockIdx.y + 1, x = blockIdx.z;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 16;
    if (c >= (size_t)N) return;
    const unsigned *d = reinterpret_cast<const unsigned *>(db + db_offset(L, N, t0 + x, 1, j, c));
    unsigned w[23];
    u64 v[16];
#pragma unroll
    for (int k = 0; k < 23; k++) w[k] = d[k];
    db_unpack_granule46(w, v);
    u64 *o = out + ((size_t)x * nQ + j) * N + c;
#pragma unroll
    for (int r = 0; r < 16; r += 2) *reinterpret_cast<ulonglong2 *>(o + r) = make_ulonglong2(v[r], v[r + 1]);
}
// The key switch's output ks [X][2][nQ][N] (canonical residues, no addend) back into ciphertexts t0 .. t0+X-1: (c0, c1) := (c0 + ks0, ks1).
// Polynomial 0 is k_db_accumulate's fused read-add-reduce-write (the sum is reduced before it is packed), polynomial 1 an overwrite
// on the same map: one thread owns every dword it touches, no atomics, no unpacked copy of c0 in HBM.  grid (N/512, nQ or 1, X*2)
__global__ __launch_bounds__(256) void k_db_rekey_store(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ ks,
                                                        unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y, xp = blockIdx.z, x = xp >> 1, p = xp & 1;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2;
    const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(ks + ((size_t)xp * nQ + j) * N + c);
    unsigned char *d = db + db_offset(L, N, t0 + x, p, j, c);
    const bool pk = L.packed && j > 0;
    if (p == 0) {
        db_accumulate_pair(d, pk, a.x, a.y, mod[j].q);
    } else if (pk) {
        unsigned w[3];
        db_pack_pair48(a.x, a.y, w);
        unsigned *o = reinterpret_cast<unsigned *>(d);
        o[0] = w[0];
        o[1] = w[1];
        o[2] = w[2];
    } else {
        *reinterpret_cast<ulonglong2 *>(d) = a;
    }
}
// ... the 46-bit limbs of a bits46 layout on k_db_repack46's map.  grid (N/4096, nQ - 1, X*2): limb j = blockIdx.y + 1
__global__ __launch_bounds__(256) void k_db_rekey_store46(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ ks,
                                                          unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    const int j = blockIdx.y + 1, xp = blockIdx.z, x = xp >> 1, p = xp & 1;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 16;
    if (c >= (size_t)N) return;
    const u64 *pl = ks + ((size_t)xp * nQ + j) * N + c;
    u64 a[16];
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(pl + r);
        a[r] = v.x;
        a[r + 1] = v.y;
    }
    unsigned *d = reinterpret_cast<unsigned *>(db + db_offset(L, N, t0 + x, p, j, c));
    if (p == 0) {
        db_accumulate_granule46(d, a, mod[j].q);
    } else {
        unsigned w[23];
        db_pack_granule46(a, w);
#pragma unroll
        for (int k = 0; k < 23; k++) d[k] = w[k];
    }
}

__global__ __launch_bounds__(256) void k_fill_uniform_hash(const ModC *__restrict__ mod, int N, u64 *__restrict__ dst,
                                                           int nl, u64 seed) {
    const size_t lp = blockIdx.y + (size_t)blockIdx.z * gridDim.y;
    const ModC M = mod[lp % nl];
    const size_t idx = lp * N + (size_t)blockIdx.x * 256 + threadIdx.x;
    u64 z = seed + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    dst[idx] = reduce64(z, M);
}

}  // namespace

// ================================================================================================ launchers
namespace hk {

// ---- byte ledger
namespace {
bool g_ledger_on = false;
std::mutex g_ledger_mu;
std::map<std::string, std::pair<long, double>> g_ledger;
}  // namespace
void ledger_enable(bool on) {
    std::lock_guard<std::mutex> lk(g_ledger_mu);
    g_ledger_on = on;
    g_ledger.clear();
}
void ledger_add(const char *kernel, double bytes) {
    if (!g_ledger_on) return;
    std::lock_guard<std::mutex> lk(g_ledger_mu);
    auto &e = g_ledger[kernel];
    e.first++;
    e.second += bytes;
}
size_t ledger_dump(char *out, size_t cap) {
    std::lock_guard<std::mutex> lk(g_ledger_mu);
    std::string t;
    char line[256];
    for (auto &kv : g_ledger) {
        snprintf(line, sizeof line, "%s\t%ld\t%.0f\n", kv.first.c_str(), kv.second.first, kv.second.second);
        t += line;
    }
    if (out && cap) {
        const size_t n = std::min(cap - 1, t.size());
        memcpy(out, t.data(), n);
        out[n] = 0;
    }
    return t.size() + 1;
}
#define LP_BYTES(N) ((double)(N) * 8.0)

void ntt_forward(hipStream_t st, const NttTables &T, int logN, const u64 *src, u64 *dst, size_t so, size_t dso, int X,
                 const LimbSel &sel) {
    if (logN == 15 && !T.generic) return ntt15_forward(st, T, src, dst, so, dso, X, sel);
    if (logN == 16 && T.ntt16 && !T.generic) return ntt16_forward(st, T, src, dst, so, dso, X, sel);
    const int N = 1 << logN, R = N >> 8;
    ScaleSel dummy = {};
    hipLaunchKernelGGL(k_ntt_strided<false>, dim3(8, X * sel.n), dim3(256), (size_t)R * 32 * 8, st, T, logN, src, dst, so,
                       dso, sel, dummy);
    if (N < 2048) hipLaunchKernelGGL((k_ntt_contig<false, 1024>), dim3(N / 1024, X * sel.n), dim3(256), 0, st, T, logN, dst, dst, dso, dso, sel);
    else hipLaunchKernelGGL(k_ntt_contig<false>, dim3(N / 2048, X * sel.n), dim3(256), 0, st, T, logN, dst, dst, dso, dso, sel);
}
void ntt_inverse(hipStream_t st, const NttTables &T, int logN, const u64 *src, u64 *dst, size_t so, size_t dso, int X,
                 const LimbSel &sel, const ScaleSel &scale) {
    if (logN == 15 && !T.generic) return ntt15_inverse(st, T, src, dst, so, dso, X, sel, scale);
    if (logN == 16 && T.ntt16 && !T.generic) return ntt16_inverse(st, T, src, dst, so, dso, X, sel, scale);
    const int N = 1 << logN, R = N >> 8;
    if (N < 2048) hipLaunchKernelGGL((k_ntt_contig<true, 1024>), dim3(N / 1024, X * sel.n), dim3(256), 0, st, T, logN, src, dst, so, dso, sel);
    else hipLaunchKernelGGL(k_ntt_contig<true>, dim3(N / 2048, X * sel.n), dim3(256), 0, st, T, logN, src, dst, so, dso, sel);
    hipLaunchKernelGGL(k_ntt_strided<true>, dim3(8, X * sel.n), dim3(256), (size_t)R * 32 * 8, st, T, logN, dst, dst, dso,
                       dso, sel, scale);
}
void add(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int XP, const LimbSel &sel, int a_ls,
         int b_ls, int o_ls) {
    ledger_add("k_addsub", 3.0 * XP * sel.n * LP_BYTES(N));
    hipLaunchKernelGGL(k_addsub<0>, dim3(N / 512, XP * sel.n), dim3(256), 0, st, mod, N, a, b, o, sel, a_ls, b_ls, o_ls);
}
void sub(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int XP, const LimbSel &sel, int a_ls,
         int b_ls, int o_ls) {
    ledger_add("k_addsub", 3.0 * XP * sel.n * LP_BYTES(N));
    hipLaunchKernelGGL(k_addsub<1>, dim3(N / 512, XP * sel.n), dim3(256), 0, st, mod, N, a, b, o, sel, a_ls, b_ls, o_ls);
}
void add_raw(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int XP, const LimbSel &sel, int a_ls,
             int b_ls, int o_ls) {
    ledger_add("k_addsub", 3.0 * XP * sel.n * LP_BYTES(N));
    hipLaunchKernelGGL(k_addsub<2>, dim3(N / 512, XP * sel.n), dim3(256), 0, st, mod, N, a, b, o, sel, a_ls, b_ls, o_ls);
}
void mod_reduce(hipStream_t st, const ModC *mod, int N, u64 *a, int XP, const LimbSel &sel, int a_ls) {
    ledger_add("k_mod_reduce", 2.0 * XP * sel.n * LP_BYTES(N));
    hipLaunchKernelGGL(k_mod_reduce, dim3(N / 512, XP * sel.n), dim3(256), 0, st, mod, N, a, sel, a_ls);
}
void mul_scalar(hipStream_t st, const ModC *mod, int N, const u64 *a, u64 *o, int XP, const LimbSel &sel,
                const ScaleSel &c, int a_ls, int o_ls) {
    ledger_add("k_mul_scalar", 2.0 * XP * sel.n * LP_BYTES(N));
    hipLaunchKernelGGL(k_mul_scalar, dim3(N / 512, XP * sel.n), dim3(256), 0, st, mod, N, a, o, sel, c, a_ls, o_ls);
}
void lincomb(hipStream_t st, const ModC *mod, int N, const LinComb &lc, u64 *o, int X, int npoly, int nl) {
    ledger_add("k_lincomb", (lc.nterms + 1.0) * X * npoly * nl * LP_BYTES(N));
    hipLaunchKernelGGL(k_lincomb, dim3(N / 512, nl, X * npoly), dim3(256), 0, st, mod, N, lc, o, npoly, nl);
}
void lincomb_multi(hipStream_t st, const ModC *mod, int N, const LinCombMulti &lc, u64 *o, int X, int npoly, int nl) {
    ledger_add("k_lincomb_multi", (lc.nterms + (double)lc.K) * X * npoly * nl * LP_BYTES(N));
    hipLaunchKernelGGL(k_lincomb_multi, dim3(N / 512, nl, X * npoly), dim3(256), 0, st, mod, N, lc, o, X * npoly, npoly, nl);
}
void batch_sum(hipStream_t st, const ModC *mod, int N, const u64 *in, u64 *o, int X, int npoly, int nl, int stride, int nout) {
    ledger_add("k_batch_sum", (X + 1.0) * nout * npoly * nl * LP_BYTES(N));
    hipLaunchKernelGGL(k_batch_sum, dim3(N / 512, nl, npoly * nout), dim3(256), 0, st, mod, N, in, o, X, npoly, nl, stride);
}
void add_scalar(hipStream_t st, const ModC *mod, int N, u64 *a, size_t outer, int X, const LimbSel &sel,
                const ScaleSel &c) {
    ledger_add("k_add_scalar", 2.0 * X * sel.n * LP_BYTES(N));
    hipLaunchKernelGGL(k_add_scalar, dim3(N / 512, X * sel.n), dim3(256), 0, st, mod, N, a, outer, sel, c);
}
void copy_limbs(hipStream_t st, int N, const u64 *src, u64 *dst, size_t so, size_t dso, int X, int nlimbs) {
    ledger_add("k_copy_limbs", 2.0 * X * nlimbs * LP_BYTES(N));
    hipLaunchKernelGGL(k_copy_limbs, dim3(N / 512, X * nlimbs), dim3(256), 0, st, N, src, dst, so, dso, nlimbs);
}
void tensor(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int X, int nl, int a_ls, int b_ls,
            const u64 *c, int c_ls, const ScaleSel *kap) {
    ledger_add(c ? "k_tensor<true>" : "k_tensor<false>", (c ? 9.0 : 7.0) * X * nl * LP_BYTES(N));  // a0 a1 b0 b1 (c0 c1) in, d0 d1 d2 out
    if (c)
        hipLaunchKernelGGL(k_tensor<true>, dim3(N / 512, nl, X), dim3(256), 0, st, mod, N, a, b, o, nl, a_ls, b_ls, c, c_ls, *kap);
    else
        hipLaunchKernelGGL(k_tensor<false>, dim3(N / 512, nl, X), dim3(256), 0, st, mod, N, a, b, o, nl, a_ls, b_ls,
                           (const u64 *)nullptr, 0, ScaleSel{});
}
// conversion kernels let one thread produce every target limb (sources read once).  With few polynomials that is N/512 * X
// workgroups, each a long serial chain: below ~2 workgroups per CU the targets are sliced over grid.z instead (sources come from L2)
static int small_launch_targets(int N, int X, int nt) {
    const int wgs = (N / 512) * X;
    if (nt <= 1 || wgs >= 512) return nt > 0 ? nt : 1;
    const int slices = std::min(nt, (512 + wgs - 1) / wgs);
    return (nt + slices - 1) / slices;
}
void tensor_sq(hipStream_t st, const ModC *mod, int N, const u64 *a, u64 *o, int X, int nl, int a_ls) {
    ledger_add("k_tensor_sq", 5.0 * X * nl * LP_BYTES(N));  // a0 a1 in, d0 d1 d2 out
    hipLaunchKernelGGL(k_tensor_sq, dim3(N / 512, nl, X), dim3(256), 0, st, mod, N, a, o, nl, a_ls);
}
void tensor_bcast(hipStream_t st, const ModC *mod, int N, const u64 *q, int q_ls, const u64 *b, int b_ls, u64 *o, int X, int nl) {
    ledger_add("k_tensor_bcast", (2.0 + 5.0 * X) * nl * LP_BYTES(N));  // q0 q1 once, b0 b1 in and d0 d1 d2 out per ciphertext
    hipLaunchKernelGGL(k_tensor_bcast, dim3(N / 512, nl, (X + HY_BCAST_X - 1) / HY_BCAST_X), dim3(256), 0, st, mod, N, q, q_ls, b, b_ls, o, nl, X);
}
void tensor_dot(hipStream_t st, const ModC *mod, int N, const u64 *q, int q_ls, const u64 *b, int b_ls, u64 *o, int X, int K, int nl) {
    ledger_add("k_tensor_dot", (2.0 * K + (2.0 * K + 3.0) * X) * nl * LP_BYTES(N));  // the K query chunks once; per matrix 2K operands in, d0 d1 d2 out
    hipLaunchKernelGGL(k_tensor_dot, dim3(N / 512, nl, (X + HY_DOT_X - 1) / HY_DOT_X), dim3(256), 0, st, mod, N, q, q_ls, b, b_ls, o, nl, X, K);
}
void base_convert(hipStream_t st, const ModC *mod, int N, const u64 *y, size_t yo, u64 *out, size_t oo, int X,
                  const ConvTab &tab, const LimbSel &dsel) {
    ledger_add("k_base_convert", (double)X * (tab.ns + tab.nt - (tab.skip_hi - tab.skip_lo)) * LP_BYTES(N));  // sources once, every target once
    const int tz = small_launch_targets(N, X, tab.nt);
    hipLaunchKernelGGL(k_base_convert, dim3(N / 512, X, (tab.nt + tz - 1) / tz), dim3(256), 0, st, mod, N, y, yo, out, oo, tab, dsel, tz);
}
void base_convert_digits(hipStream_t st, const ModC *mod, int N, const u64 *y, size_t yo, u64 *out, size_t oo, int X,
                          const ConvTab *d_tabs, int nd, int nl, int nE, const LimbSel &esel) {
    ledger_add("k_base_convert_digits", (double)X * nd * nE * LP_BYTES(N));  // nl sources once + (nd nE - nl) targets once
    const int tz = small_launch_targets(N, X * nd, nE);
    const int slices = (nE + tz - 1) / tz;
    hipLaunchKernelGGL(k_base_convert_digits, dim3(N / 512, X, nd * slices), dim3(256), 0, st, mod, N, y, yo, out, oo, d_tabs, esel, slices, tz, nE);
}
void inner_product(hipStream_t st, const ModC *mod, int N, const u64 *dig, size_t dxs, int nd, const u64 *const *keys,
                   int same_key, int nT, u64 *acc, int X, const LimbSel &esel, const u64 *own, size_t own_xs, int alpha, int nl,
                   int acc_rows, int packed_nQ, int dig_rows, int dig_t0) {
    const int rows = acc_rows > 0 ? acc_rows : esel.n, drows = dig_rows > 0 ? dig_rows : rows;
    {   // keys of X rotations streamed once (one shared key: once in all), digits / own limbs once per x unless shared (dxs == 0), acc out
        double rowb = 0;  // bytes of one (digit, poly) key row set restricted to the limbs of esel
        for (int t = 0; t < esel.n; t++) rowb += (packed_nQ > 0 && esel.mod[t] > 0 && esel.mod[t] < packed_nQ) ? N * 6.0 : N * 8.0;
        const double keyb = nd * 2 * rowb;
        const double digb = (double)nd * esel.n * LP_BYTES(N);
        ledger_add(packed_nQ > 0 ? "k_inner_product<true>" : "k_inner_product<false>",
                   (same_key ? keyb : keyb * X) + (dxs ? digb * X : digb) + 2.0 * X * esel.n * LP_BYTES(N));
    }
    if (packed_nQ > 0)
        hipLaunchKernelGGL(k_inner_product<true>, dim3(N / 512, esel.n, X), dim3(256), 0, st, mod, N, dig, dxs, nd, keys, same_key,
                           nT, acc, esel, own, own_xs, alpha, nl, rows, packed_nQ, drows, dig_t0);
    else
        hipLaunchKernelGGL(k_inner_product<false>, dim3(N / 512, esel.n, X), dim3(256), 0, st, mod, N, dig, dxs, nd, keys, same_key,
                           nT, acc, esel, own, own_xs, alpha, nl, rows, 0, drows, dig_t0);
}
size_t key_packed_bytes(int N, int nQ, int nT, int nd) { return (size_t)nd * 2 * key_set_bytes(N, nQ, nT); }
void key_pack(hipStream_t st, const ModC *mod, int N, int nQ, int nT, int nd, const u64 *key, void *out, const ScaleSel *premul) {
    ledger_add("k_key_pack", (double)nd * 2 * nT * LP_BYTES(N) + (double)key_packed_bytes(N, nQ, nT, nd));
    hipLaunchKernelGGL(k_key_pack, dim3(N / 512, nT, nd * 2), dim3(256), 0, st, mod, N, nQ, nT, key, (unsigned char *)out, premul ? 1 : 0,
                       premul ? *premul : ScaleSel{});
}
void moddown_combine(hipStream_t st, const ModC *mod, int logN, const u64 *acc, int acc_limbs, const u64 *conv,
                     const u64 *addend, size_t axs, size_t aps, int add_polys, u64 *out, int X, int nl,
                     const ScaleSel &pinv, const unsigned *galois, int same_g, const u64 *self, size_t sxs, size_t sps) {
    ledger_add("k_moddown_combine", (3.0 + (addend ? 0.5 * add_polys : 0.0) + (self ? 1.0 : 0.0)) * X * 2 * nl * LP_BYTES(1 << logN));
    hipLaunchKernelGGL(k_moddown_combine, dim3((1 << logN) / 256, nl, X * 2), dim3(256), 0, st, mod, logN, acc, acc_limbs,
                       conv, addend, axs, aps, add_polys, out, nl, pinv, galois, same_g, self, sxs, sps);
}
void moddown_rescale_conv(hipStream_t st, const ModC *mod, int N, const u64 *y, size_t yo, const u64 *u, size_t uo, u64 *w, int XP, int l,
                          int nP, const ConvTab &tab) {
    ledger_add("k_moddown_rescale_conv", (double)XP * (nP + 1 + l) * LP_BYTES(N));  // y (nP limbs) + u in, l limbs out
    const int tz = small_launch_targets(N, XP, l);
    hipLaunchKernelGGL(k_moddown_rescale_conv, dim3(N / 512, XP, (l + tz - 1) / tz), dim3(256), 0, st, mod, N, y, yo, u, uo, w, l, nP, tab, tz);
}
void moddown_last_limb(hipStream_t st, const ModC *mod, int N, const u64 *acc, int acc_limbs, const u64 *addend, size_t add_x,
                       size_t add_p, u64 *u, size_t uo, int XP, int l, u64 pinv, u64 pinv_sh, int dbl) {
    ledger_add("k_moddown_last_limb", 3.0 * XP * LP_BYTES(N));
    hipLaunchKernelGGL(k_moddown_last_limb, dim3(N / 512, XP), dim3(256), 0, st, mod, N, acc, acc_limbs, addend, add_x, add_p, u, uo, l,
                       pinv, pinv_sh, dbl);
}
void rescale_spread(hipStream_t st, const ModC *mod, int N, const u64 *t, u64 *tmp, int X, int l) {
    ledger_add("k_rescale_spread", (1.0 + l) * X * LP_BYTES(N));
    hipLaunchKernelGGL(k_rescale_spread, dim3(N / 256, l, X), dim3(256), 0, st, mod, N, t, tmp, l);
}
void rescale_combine(hipStream_t st, const ModC *mod, int N, const u64 *in, const u64 *tmp, u64 *out, int X, int l,
                     const ScaleSel &qlinv, int in_ls) {
    ledger_add("k_rescale_combine", 3.0 * X * l * LP_BYTES(N));
    hipLaunchKernelGGL(k_rescale_combine, dim3(N / 256, l, X), dim3(256), 0, st, mod, N, in, tmp, out, l, qlinv, in_ls);
}
// bpp = database blocks per wave (1 or 2), nw = max waves per workgroup (1, 2 or 4; 0 = 4); both must divide G.  Round 5: four blocks
// per wave and eight / sixteen waves per workgroup are gone — they spilled (863 registers at <4,16>, 237 at <4,8>) and were never
// faster (profiles/r04/experiments.txt: BPP=4 140.5 ms, NW=8 inside the run-to-run spread); larger values are clamped.
void tensor_split(int G, int bpp, int nw, int *Bo, int *Wo) {
    const int B = (bpp >= 2 && G % 2 == 0) ? 2 : 1;
    const int rest = G / B;
    if (nw == 0 || nw > 4) nw = 4;
    int W = 1;
    for (int cand : {4, 2})
        if ((nw == 0 || cand <= nw) && rest % cand == 0) {
            W = cand;
            break;
        }
    *Bo = B;
    *Wo = W;
}
// ---- loop B.  Batches: QW = 2.  At QW = 4 every instantiation takes 256 VGPRs (one wave per SIMD) and the 512-thread ones spill; at
// QW = 2 the kernels keep what the single-query kernels at BPP = 2 take (three waves per SIMD)
constexpr int MQ_QW = 2;
int hydia_tensor_mq_width(const DbLayout &) { return MQ_QW; }
// A batch of plain queries: two sums per query instead of three leave room for QW = 4 without scratch, and batches of
// four or more take it — the measured choice (profiles/plain_query_batch/README.md).  Two or three queries take QW = 2 (and 1): the
// launcher serves what is left with the narrower widths
constexpr int PQ_MQ_QW = 4;
int hydia_pq_mq_width(const DbLayout &) { return PQ_MQ_QW; }
// A batch on a plain gallery: both widths build without scratch, and batches of four or more take QW = 4 — the measured
// choice: at 2^20 vectors it beats QW = 2 by more than the repeats spread, 10.1 against 10.7 ms of loop B per query
// (profiles/plain_gallery_batch/README.md).  Two or three queries take QW = 2 (and 1): the launcher serves what is left with the
// narrower widths
constexpr int PLAIN_MQ_QW = 4;
int hydia_plain_mq_width(const DbLayout &) { return PLAIN_MQ_QW; }
// what every loop-B entry point takes, in the launcher's words (a plain form ignores rqs, q0 and Qt)
struct LoopB {
    const ModC *mod;
    int N;
    const u64 *rot;
    size_t rqs;
    const unsigned char *db;
    u64 *acc;
    int dim, nl, Gq, xm;
    DbLayout L;
    int G, ng, nblk, q0, Qt;
};
// a form's two entry points with the argument lists they have: streaming <A, BPP, QW, NW> from limb j0 on, split-diagonal <KS, QW>
template <class A, int BPP, int QW, int NW>
static void launch_stream(FormCtCt, hipStream_t st, dim3 grid, const LoopB &p, int j0) {
    hipLaunchKernelGGL((k_hydia_tensor<A, BPP, QW, NW>), grid, dim3(64 * NW), 0, st, p.mod, p.N, p.rot, p.rqs, p.db, p.acc, p.dim, p.nl, p.Gq,
                       p.xm, p.L, j0, p.G, p.ng, p.nblk, p.q0, p.Qt);
}
template <class A, int BPP, int QW, int NW>
static void launch_stream(FormCtPlain, hipStream_t st, dim3 grid, const LoopB &p, int j0) {
    hipLaunchKernelGGL((k_hydia_plain<A, BPP, NW>), grid, dim3(64 * NW), 0, st, p.mod, p.N, p.rot, p.db, p.acc, p.dim, p.nl, p.Gq, p.xm, p.L, j0,
                       p.G, p.ng, p.nblk);
}
template <class A, int BPP, int QW, int NW>
static void launch_stream(FormPlainCt, hipStream_t st, dim3 grid, const LoopB &p, int j0) {
    hipLaunchKernelGGL((k_hydia_pq<A, BPP, NW>), grid, dim3(64 * NW), 0, st, p.mod, p.N, p.rot, p.db, p.acc, p.dim, p.nl, p.Gq, p.xm, p.L, j0,
                       p.G, p.ng, p.nblk);
}
template <int KS, int QW>
static void launch_split(FormCtCt, hipStream_t st, dim3 grid, const LoopB &p) {
    hipLaunchKernelGGL((k_hydia_tensor_sk<KS, QW>), grid, dim3(64 * KS), 0, st, p.mod, p.N, p.rot, p.rqs, p.db, p.acc, p.dim, p.nl, p.L, p.G,
                       p.ng, p.nblk, p.q0, p.Qt);
}
template <int KS, int QW>
static void launch_split(FormCtPlain, hipStream_t st, dim3 grid, const LoopB &p) {
    hipLaunchKernelGGL((k_hydia_plain_sk<KS>), grid, dim3(64 * KS), 0, st, p.mod, p.N, p.rot, p.db, p.acc, p.dim, p.nl, p.L, p.G, p.ng, p.nblk);
}
template <int KS, int QW>
static void launch_split(FormPlainCt, hipStream_t st, dim3 grid, const LoopB &p) {
    hipLaunchKernelGGL((k_hydia_pq_sk<KS>), grid, dim3(64 * KS), 0, st, p.mod, p.N, p.rot, p.db, p.acc, p.dim, p.nl, p.L, p.G, p.ng, p.nblk);
}
template <class A, int BPP, int QW, int NW>
static void launch_stream(FormPlainCtMq, hipStream_t st, dim3 grid, const LoopB &p, int j0) {
    // (Halves24<false> is not instantiated for this family: a batch keeps the 128-bit sums where a single query takes it, see loop_b)
    if constexpr (BPP == 1 && !std::is_same<A, Halves24<false>>::value)
        hipLaunchKernelGGL((k_hydia_pq_mq<A, QW, NW>), grid, dim3(64 * NW), 0, st, p.mod, p.N, p.rot, p.rqs, p.db, p.acc, p.dim, p.nl, p.Gq,
                           p.xm, p.L, j0, p.G, p.ng, p.nblk, p.q0, p.Qt);
    else throw std::logic_error("hydia: no such kernel for a batch of plain queries (one block per wave; 128-bit sums or 46-bit halves)");
}
template <int KS, int QW>
static void launch_split(FormPlainCtMq, hipStream_t st, dim3 grid, const LoopB &p) {
    hipLaunchKernelGGL((k_hydia_pq_mq_sk<KS, QW>), grid, dim3(64 * KS), 0, st, p.mod, p.N, p.rot, p.rqs, p.db, p.acc, p.dim, p.nl, p.L, p.G,
                       p.ng, p.nblk, p.q0, p.Qt);
}
template <class A, int BPP, int QW, int NW>
static void launch_stream(FormCtPlainMq, hipStream_t st, dim3 grid, const LoopB &p, int j0) {
    // (Halves24<false> is not instantiated for this family either: a batch keeps the 128-bit sums there, see loop_b)
    if constexpr (BPP == 1 && !std::is_same<A, Halves24<false>>::value)
        hipLaunchKernelGGL((k_hydia_plain_mq<A, QW, NW>), grid, dim3(64 * NW), 0, st, p.mod, p.N, p.rot, p.rqs, p.db, p.acc, p.dim, p.nl, p.Gq,
                           p.xm, p.L, j0, p.G, p.ng, p.nblk, p.q0, p.Qt);
    else throw std::logic_error("hydia: no such kernel for a batch on a plain gallery (one block per wave; 128-bit sums or 46-bit halves)");
}
template <int KS, int QW>
static void launch_split(FormCtPlainMq, hipStream_t st, dim3 grid, const LoopB &p) {
    hipLaunchKernelGGL((k_hydia_plain_mq_sk<KS, QW>), grid, dim3(64 * KS), 0, st, p.mod, p.N, p.rot, p.rqs, p.db, p.acc, p.dim, p.nl, p.L, p.G,
                       p.ng, p.nblk, p.q0, p.Qt);
}
// an instantiation's name as rocprofv3 prints it (namespaces dropped), which is what the byte ledger records; QW only where the form
// has batches
template <class F>
static std::string stream_name(const char *policy, int bpp, int qw, int nw) {
    char n[96];
    if (!F::bpp_arg) snprintf(n, sizeof n, "k_hydia_%s<%s, %d, %d>", F::name, policy, qw, nw);
    else if (F::batch) snprintf(n, sizeof n, "k_hydia_%s<%s, %d, %d, %d>", F::name, policy, bpp, qw, nw);
    else snprintf(n, sizeof n, "k_hydia_%s<%s, %d, %d>", F::name, policy, bpp, nw);
    return n;
}
template <class F>
static std::string split_name(int ks, int qw) {
    char n[96];
    if (F::batch) snprintf(n, sizeof n, "k_hydia_%s_sk<%d, %d>", F::name, ks, qw);
    else snprintf(n, sizeof n, "k_hydia_%s_sk<%d>", F::name, ks);
    return n;
}
// the streaming kernel <A, BPP, QW, nw> of form F with its ledger entry.  NW = 8 is a batch over a group-sequential layout of
// eight-block groups
template <class F, class A, int BPP, int QW>
static void stream_nw(hipStream_t st, int nw, dim3 grid, const LoopB &p, int j0, double bytes) {
    ledger_add(stream_name<F>(A::name, BPP, QW, nw).c_str(), bytes);
    switch (nw) {
    case 1: launch_stream<A, BPP, QW, 1>(F{}, st, grid, p, j0); return;
    case 2: launch_stream<A, BPP, QW, 2>(F{}, st, grid, p, j0); return;
    case 4: launch_stream<A, BPP, QW, 4>(F{}, st, grid, p, j0); return;
    case 8:
        if constexpr (F::batch && BPP == 1) {
            launch_stream<A, BPP, QW, 8>(F{}, st, grid, p, j0);
            return;
        }
    }
    throw std::logic_error("hydia: no loop B kernel for this split");
}
// the split-diagonal kernel <KS, qw> of form F with its ledger entry
template <class F, int KS>
static void split_qw(hipStream_t st, int qw, dim3 grid, const LoopB &p, double bytes) {
    ledger_add(split_name<F>(KS, qw).c_str(), bytes);
    if constexpr (F::max_qw >= 4)
        if (qw == 4) return launch_split<KS, 4>(F{}, st, grid, p);
    if constexpr (F::batch)
        if (qw == 2) return launch_split<KS, 2>(F{}, st, grid, p);
    if (qw != 1) throw std::logic_error("hydia: no loop B kernel for this batch width");
    launch_split<KS, 1>(F{}, st, grid, p);
}
// Loop B of every form: Q queries (one unless the form has batches and bpp = TENSOR_BATCH) against G blocks of dim diagonals; width =
// queries per pass of a batch (a power of two up to F::max_qw; what is left over takes the narrower widths, a last odd query QW = 1)
template <class F>
static void loop_b(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G, int dim,
                   int nl, const DbLayout &L, int ng, int bpp, int nw, int width = MQ_QW) {
    const bool batch = F::batch && bpp == TENSOR_BATCH;
    if (Q < 1 || (!batch && Q != 1) || G < 1 || dim < 2 || (ng > 0 && G % ng)) throw std::logic_error("hydia: loop B with a bad shape");
    if (!batch) width = 1;
    if (width < 1 || width > F::max_qw || (width & (width - 1))) throw std::logic_error("hydia: loop B with a batch width that is not instantiated");
    if (L.bits46 && !(L.packed && L.seq && dim <= 4096)) throw std::logic_error("hydia: 46-bit database outside the 24-bit-halves loop B");
    if (L.seq && (G != L.blocks || dim != L.bd || G % L.seq || G <= 8 || L.seq % L.seq_bpp || (L.seq & (L.seq - 1)) || L.seq > 8))
        throw std::logic_error("hydia: loop B launched against a group-sequential database with another shape");
    // B blocks per wave, W waves per workgroup.  The group-sequential layout fixes the workgroup's share: a group of the database is
    // what one workgroup walks.  A batch takes one block per wave (its QW accumulator sets take the registers of BPP blocks)
    int B = 1, W;
    if (batch) {
        W = L.seq ? L.seq : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
    } else if (L.seq) {
        B = L.seq_bpp;
        W = L.seq / L.seq_bpp;
    } else {
        tensor_split(G, bpp, nw, &B, &W);
    }
    LoopB p{mod, N, rot, rqs, (const unsigned char *)db, acc, dim, nl, G / (B * W), (N / 128) % 8 == 0 ? 1 : 0 /* XCD-aware tile map */,
            L, G, ng, ng > 0 ? G / ng : 0, 0, Q};
    // ledger bytes per limb: the resident database (dp polynomials per entry; 6- or 8-byte residues, 5.75 for 46-bit) + the QW rotation
    // sets (qp polynomials per rotation) once + QW x G accumulators of `comps` components
    const double per_lp8 = LP_BYTES(N), per_lp6 = (double)N * (L.bits46 ? 5.75 : 6.0);
    int QW = 1;
    for (p.q0 = 0; p.q0 < Q; p.q0 += QW) {  // one pass over the database per QW queries (an odd last one alone)
        for (QW = width; QW > Q - p.q0; QW >>= 1) {}
        auto bytes = [&](int limbs, double per_lp) {
            return limbs * ((double)G * dim * F::dp * per_lp + QW * ((double)dim * F::qp + (double)G * F::comps) * per_lp8);
        };
        auto stream = [&](auto *policy, int j0, int limbs) {  // policy: a null pointer of the arithmetic's type
            typedef typename std::remove_pointer<decltype(policy)>::type A;
            const dim3 grid((N / 128) * p.Gq, limbs);
            const double by = bytes(limbs, j0 ? per_lp6 : per_lp8);
            if constexpr (F::max_qw >= 4)
                if (QW == 4) return stream_nw<F, A, 1, 4>(st, W, grid, p, j0, by);
            if constexpr (F::batch)
                if (QW == 2) return stream_nw<F, A, 1, 2>(st, W, grid, p, j0, by);  // (a batch has B = 1)
            if (B == 2) stream_nw<F, A, 2, 1>(st, W, grid, p, j0, by);
            else stream_nw<F, A, 1, 1>(st, W, grid, p, j0, by);
        };
        if (!L.packed) {  // 8-byte residues everywhere: one launch over all limbs
            stream((Sums128<false> *)nullptr, 0, nl);
            continue;
        }
        // limb 0 (8-byte residues) and limbs 1.. (6-byte or 46-bit residues) as two launches: no shared register budget
        if (!L.seq && G <= 8) {  // few blocks: 256 x G one-wave workgroups cannot hide the latency of dim dependent steps -> split the
            // diagonals (eight waves: sixteen hold a lane to 128 registers and the kernel spilled 69 of them — round 5)
            const dim3 grid((N / 128) * G, 1);
            if (G <= 2) split_qw<F, 8>(st, QW, grid, p, bytes(1, per_lp8));
            else split_qw<F, 4>(st, QW, grid, p, bytes(1, per_lp8));
        } else {
            stream((Sums128<false> *)nullptr, 0, 1);
        }
        if (nl == 1) continue;
        if (L.bits46) stream((Halves24<true> *)nullptr, 1, nl - 1);
        else if (!batch && L.seq && dim <= 4096) stream((Halves24<false> *)nullptr, 1, nl - 1);  // (a batch keeps the 128-bit sums here)
        else stream((Sums128<true> *)nullptr, 1, nl - 1);
    }
}
void hydia_tensor_accumulate(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G,
                             int dim, int nl, const DbLayout &L, int ng, int bpp, int nw) {
    loop_b<FormCtCt>(st, mod, N, rot, rqs, db, acc, Q, G, dim, nl, L, ng, bpp, nw);
}
// The split of a plain gallery is tensor_split's with the gallery's own cap of blocks per wave (PLAIN_BPP = 2): at two blocks per wave
// the 46-bit kernel takes 125 VGPRs (four waves per SIMD, the encrypted one two); four blocks per wave compiled to 231 (two waves per
// SIMD: the same blocks in flight per SIMD, half the waves to hide latency with) and is not instantiated
void hydia_plain_accumulate(hipStream_t st, const ModC *mod, int N, const u64 *rot, const void *db, u64 *acc, int G, int dim, int nl,
                            const DbLayout &L, int ng, int bpp, int nw) {
    if (!L.plain) throw std::logic_error("hydia: plain loop B launched against a ciphertext database");
    loop_b<FormCtPlain>(st, mod, N, rot, 0, db, acc, 1, G, dim, nl, L, ng, bpp, nw);
}
// A plain query reads every layout an encrypted query reads, unchanged, with the encrypted loop B's split
void hydia_pq_accumulate(hipStream_t st, const ModC *mod, int N, const u64 *rot, const void *db, u64 *acc, int G, int dim, int nl,
                         const DbLayout &L, int ng, int bpp, int nw) {
    if (L.plain) throw std::logic_error("hydia: plain-query loop B launched against a plain gallery");
    loop_b<FormPlainCt>(st, mod, N, rot, 0, db, acc, 1, G, dim, nl, L, ng, bpp, nw);
}
// A batch of plain queries over the same routine, with the encrypted batch's choices (workgroup = the layout's group or 4 / 2 / 1 waves
// by divisibility of G, limb 0 on the split kernel for few ciphertext-major blocks, its arithmetic per layout)
void hydia_pq_accumulate_multi(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G,
                               int dim, int nl, const DbLayout &L, int ng, int width) {
    if (L.plain) throw std::logic_error("hydia: plain-query loop B launched against a plain gallery");
    loop_b<FormPlainCtMq>(st, mod, N, rot, rqs, db, acc, Q, G, dim, nl, L, ng, TENSOR_BATCH, 0, width > 0 ? width : hydia_pq_mq_width(L));
}
// A batch of encrypted queries on a plain gallery over the same routine, with the other batches' choices (workgroup = the layout's group
// or 4 / 2 / 1 waves by divisibility of G, limb 0 on the split kernel for few ciphertext-major blocks, the arithmetic per layout)
void hydia_plain_accumulate_multi(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G,
                                  int dim, int nl, const DbLayout &L, int ng, int width) {
    if (!L.plain) throw std::logic_error("hydia: plain loop B launched against a ciphertext database");
    loop_b<FormCtPlainMq>(st, mod, N, rot, rqs, db, acc, Q, G, dim, nl, L, ng, TENSOR_BATCH, 0, width > 0 ? width : hydia_plain_mq_width(L));
}
void automorph_batch(hipStream_t st, int logN, const u64 *m, u64 *out, int nl, int R, const unsigned *galois) {
    ledger_add("k_automorph_batch", (1.0 + R) * nl * LP_BYTES(1 << logN));
    hipLaunchKernelGGL(k_automorph_batch, dim3((1u << logN) / 256, nl, R), dim3(256), 0, st, logN, m, out, nl, galois);
}
DbLayout db_layout(int N, int nQ, int packed, bool plain) {
    DbLayout L{};
    L.packed = packed;
    L.plain = plain ? 1 : 0;
    L.poly_bytes = packed ? (unsigned long long)N * 8 + (unsigned long long)(nQ - 1) * N * 6 : (unsigned long long)nQ * N * 8;
    L.ct_bytes = db_polys(L) * L.poly_bytes;
    return L;
}
// group-sequential for `blocks` blocks of bd ciphertexts: only where loop B is a stream worth shaping (more than 8 blocks, whole
// 128-residue tiles) — otherwise the ciphertext-major layout comes back
DbLayout db_layout_seq(int N, int nQ, int packed, int bd, int blocks, int bpp, int nw, bool bits46, bool plain) {
    DbLayout L = db_layout(N, nQ, packed, plain);
    if (blocks <= 8 || N % 128) return L;
    int B, W;
    tensor_split(blocks, bpp, nw, &B, &W);
    L.seq = B * W;
    L.seq_bpp = B;
    L.bd = bd;
    L.blocks = blocks;
    if (bits46 && packed && bd <= 4096) {  // 46-bit residues for the packed limbs (the caller vouches for the moduli)
        L.bits46 = 1;
        L.poly_bytes = (unsigned long long)N * 8 + (unsigned long long)(nQ - 1) * (N / 128) * 736;
        L.ct_bytes = db_polys(L) * L.poly_bytes;
    }
    return L;
}
void db_pack(hipStream_t st, int N, int nQ, const u64 *plain, void *db, size_t t0, int X, const DbLayout &L) {
    const int np = (int)db_polys(L);
    const bool b46 = L.bits46 && L.seq && L.packed && nQ > 1;  // limb 0 through the pair kernel, the 46-bit limbs through the granule kernel
    hipLaunchKernelGGL(k_db_repack<true>, dim3(N / 512, b46 ? 1 : nQ, X * np), dim3(256), 0, st, N, nQ, const_cast<u64 *>(plain),
                       (unsigned char *)db, L, t0);
    if (b46)
        hipLaunchKernelGGL(k_db_repack46<true>, dim3((N / 16 + 255) / 256, nQ - 1, X * np), dim3(256), 0, st, N, nQ, const_cast<u64 *>(plain), (unsigned char *)db, L, t0);
}
void db_unpack(hipStream_t st, int N, int nQ, u64 *plain, const void *db, size_t t0, int X, const DbLayout &L) {
    const int np = (int)db_polys(L);
    const bool b46 = L.bits46 && L.seq && L.packed && nQ > 1;
    hipLaunchKernelGGL(k_db_repack<false>, dim3(N / 512, b46 ? 1 : nQ, X * np), dim3(256), 0, st, N, nQ, plain, (unsigned char *)db, L, t0);
    if (b46) hipLaunchKernelGGL(k_db_repack46<false>, dim3((N / 16 + 255) / 256, nQ - 1, X * np), dim3(256), 0, st, N, nQ, plain, (unsigned char *)db, L, t0);
}
// ciphertexts t0 .. t0+X-1 of the database at `db` += plain [X][2][nQ][N] residues (mod q_j): the launch shapes of db_pack
void db_accumulate(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *plain, void *db, size_t t0, int X, const DbLayout &L) {
    const bool b46 = L.bits46 && L.seq && L.packed && nQ > 1;
    if (L.plain) {  // a plain gallery: plain [X][nQ][N], one polynomial read and written + nQ N 8 fresh bytes read per entry
        ledger_add("k_plain_db_accumulate", (double)X * (2.0 * L.ct_bytes + 1.0 * nQ * N * 8));
        hipLaunchKernelGGL(k_plain_db_accumulate, dim3(N / 512, b46 ? 1 : nQ, X), dim3(256), 0, st, mod, N, nQ, plain, (unsigned char *)db, L, t0);
        if (b46)
            hipLaunchKernelGGL(k_plain_db_accumulate46, dim3((N / 16 + 255) / 256, nQ - 1, X), dim3(256), 0, st, mod, N, nQ, plain, (unsigned char *)db, L, t0);
        return;
    }
    ledger_add("k_db_accumulate", (double)X * (2.0 * L.ct_bytes + 2.0 * nQ * N * 8));  // resident bytes read and written + the fresh ones read
    hipLaunchKernelGGL(k_db_accumulate, dim3(N / 512, b46 ? 1 : nQ, X * 2), dim3(256), 0, st, mod, N, nQ, plain, (unsigned char *)db, L, t0);
    if (b46)
        hipLaunchKernelGGL(k_db_accumulate46, dim3((N / 16 + 255) / 256, nQ - 1, X * 2), dim3(256), 0, st, mod, N, nQ, plain, (unsigned char *)db, L, t0);
}
// *flag |= (some residue of plain [X][nQ][N] is at or above its modulus); the caller clears the flag and reads it back
void db_check_canonical(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *plain, int X, unsigned *flag) {
    ledger_add("k_db_check_canonical", (double)X * nQ * N * 8);
    hipLaunchKernelGGL(k_db_check_canonical, dim3(N / 512, nQ, X), dim3(256), 0, st, mod, N, nQ, plain, flag);
}
// polynomial 1 of ciphertexts t0 .. t0+X-1 -> out [X][nQ][N] residues: the launch shapes of db_unpack, one polynomial per ciphertext
void db_gather_poly(hipStream_t st, int N, int nQ, u64 *out, const void *db, size_t t0, int X, const DbLayout &L) {
    const bool b46 = L.bits46 && L.seq && L.packed && nQ > 1;
    ledger_add("k_db_gather_poly", (double)X * (1.0 * L.poly_bytes + 1.0 * nQ * N * 8));  // one resident polynomial read, its residues written
    hipLaunchKernelGGL(k_db_gather_poly, dim3(N / 512, b46 ? 1 : nQ, X), dim3(256), 0, st, N, nQ, out, (const unsigned char *)db, L, t0);
    if (b46)
        hipLaunchKernelGGL(k_db_gather_poly46, dim3((N / 16 + 255) / 256, nQ - 1, X), dim3(256), 0, st, N, nQ, out, (const unsigned char *)db, L, t0);
}
// ciphertexts t0 .. t0+X-1 := (c0 + ks0, ks1), ks [X][2][nQ][N] residues (mod q_j): the launch shapes of db_accumulate
void db_rekey_store(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *ks, void *db, size_t t0, int X, const DbLayout &L) {
    const bool b46 = L.bits46 && L.seq && L.packed && nQ > 1;
    ledger_add("k_db_rekey_store", (double)X * (1.5 * L.ct_bytes + 2.0 * nQ * N * 8));  // c0 read and written, c1 written + the key switch's output read
    hipLaunchKernelGGL(k_db_rekey_store, dim3(N / 512, b46 ? 1 : nQ, X * 2), dim3(256), 0, st, mod, N, nQ, ks, (unsigned char *)db, L, t0);
    if (b46)
        hipLaunchKernelGGL(k_db_rekey_store46, dim3((N / 16 + 255) / 256, nQ - 1, X * 2), dim3(256), 0, st, mod, N, nQ, ks, (unsigned char *)db, L, t0);
}
// grid (N/512, nl, XP): two coefficients per thread, the plaintext's residues and Shoup companions read beside the operand's
__global__ __launch_bounds__(256) void k_mul_plain(const ModC *__restrict__ mod, int N, const u64 *__restrict__ a, int a_ls,
                                                   const u64 *__restrict__ m, const u64 *__restrict__ ms, u64 *__restrict__ o, int nl) {
    const int j = blockIdx.y, xp = blockIdx.z;
    const u64 q = mod[j].q;
    const size_t c = (size_t)(blockIdx.x * 256 + threadIdx.x) * 2, i = (size_t)j * N + c;
    const ulonglong2 va = *reinterpret_cast<const ulonglong2 *>(a + (size_t)xp * a_ls * N + i);
    const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(m + i), ws = *reinterpret_cast<const ulonglong2 *>(ms + i);
    *reinterpret_cast<ulonglong2 *>(o + (size_t)xp * nl * N + i) = make_ulonglong2(mulmod_shoup(va.x, w.x, ws.x, q), mulmod_shoup(va.y, w.y, ws.y, q));
}
void mul_plain(hipStream_t st, const ModC *mod, int N, const u64 *a, int a_ls, const u64 *m, const u64 *ms, u64 *o, int XP, int nl) {
    ledger_add("k_mul_plain", (2.0 * XP + 2.0) * nl * LP_BYTES(N));
    hipLaunchKernelGGL(k_mul_plain, dim3(N / 512, nl, XP), dim3(256), 0, st, mod, N, a, a_ls, m, ms, o, nl);
}
void fill_uniform_hash(hipStream_t st, const ModC *mod, int N, u64 *dst, size_t n_limbpolys, int nl,
                       unsigned long long seed) {
    // slabs of at most 32768 limb-polys (grid.y limit), each starting on a limb-0 boundary
    const size_t slab = 32768 - 32768 % nl;
    for (size_t done = 0; done < n_limbpolys; done += slab) {
        const size_t cnt = n_limbpolys - done < slab ? n_limbpolys - done : slab;
        hipLaunchKernelGGL(k_fill_uniform_hash, dim3(N / 256, (unsigned)cnt, 1), dim3(256), 0, st, mod, N,
                           dst + done * N, nl, seed + done * 0x51ED27ull);
    }
}

}  // namespace hk
