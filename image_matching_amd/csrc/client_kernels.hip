// image_matching_amd/csrc/client_kernels.hip — gfx950 kernels of the receiver / enroller / key-generation side:
// ChaCha20-addressed samplers, the canonical-embedding FFT (CKKS encode/decode), public-key encryption, decryption
// the diagonal packing of DiagonalEnroller, and the widening / normalisation of templates that arrive in device memory.
//
// Replaces, on the GPU: MakeCKKSPackedPlaintext + Encrypt (/root/reference/src/openFHE_wrapper.cpp:74-77), Decrypt +
// GetRealPackedValue (:81-85), KeyGen/EvalMultKeyGen/EvalRotateKeyGen (/root/reference/src/main.cpp:184-206) and the
// packing loops of /root/reference/src/enroller/enroller_diag.cpp:57-156.
// Floating point here is compiled with -ffp-contract=off and uses the same operation order as the specification in
// DESIGN.md, so encodings are reproducible bit for bit.
#include "client_kernels.h"

#include <stdexcept>

#include "gauss_cdt.h"
#include "rows_norm.h"

namespace {

__device__ __constant__ u64 d_gauss_cdt[HYDIA_GAUSS_CDT_LEN] = HYDIA_GAUSS_CDT_VALUES;

// uniform residues: thread = one ChaCha block = 4 coefficients (128 random bits each, reduced mod q).
// grid (N/4/256 rounded up, ny, nz): stream = base + y*step_y + z*step_z ; out = dst + y*stride_y + z*stride_z
__global__ __launch_bounds__(256) void k_sample_uniform(ChaChaKey key, const ModC *__restrict__ mod, int N, u64 sbase,
                                                        u64 step_y, u64 step_z, u64 *__restrict__ dst, size_t stride_y,
                                                        size_t stride_z, LimbSel ysel) {
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk * 4 >= N) return;
    const int y = blockIdx.y, z = blockIdx.z;
    const ModC M = mod[ysel.mod[y]];
    u64 a[4];
    chacha_uniform4(key, sbase + (u64)y * step_y + (u64)z * step_z, (u64)blk, M, a);
    u64 *o = dst + (size_t)y * stride_y + (size_t)z * stride_z + (size_t)blk * 4;
#pragma unroll
    for (int t = 0; t < 4; t++) o[t] = a[t];
}
// small signed polynomials: MODE 0 ternary (16 per block), MODE 1 discrete Gaussian sigma 3.19 (8 per block).
// grid (ceil(N/per/256), X): stream = base + x*step ; out int32 [X][N]
template <int MODE>
__global__ __launch_bounds__(256) void k_sample_small(ChaChaKey key, int N, u64 sbase, u64 step, int *__restrict__ dst) {
    constexpr int PER = MODE == 0 ? 16 : 8;
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk * PER >= N) return;
    const int x = blockIdx.y;
    unsigned w[16];
    chacha_block(key, sbase + (u64)x * step, (u64)blk, w);
    int *o = dst + (size_t)x * N + (size_t)blk * PER;
    if (MODE == 0) {
#pragma unroll
        for (int t = 0; t < 16; t++) o[t] = (int)(((u64)w[t] * 3ull) >> 32) - 1;
    } else {
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const u64 r = (u64)w[2 * t] | ((u64)w[2 * t + 1] << 32);
            const u64 u = r >> 1;
            int k = 0;
            while (u >= d_gauss_cdt[k]) k++;
            o[t] = (r & 1) ? -k : k;
        }
    }
}
// out[x][slot][c] = (a[x][c] (+ m[x][c])) mod q_slot ; a int32, m int64 (optional). grid (N/256, sel.n, X)
__global__ __launch_bounds__(256) void k_small_to_limbs(const ModC *__restrict__ mod, int N, const int *__restrict__ a,
                                                        const long long *__restrict__ m, u64 *__restrict__ out,
                                                        size_t out_x_stride, LimbSel sel) {
    const int slot = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[sel.mod[slot]];
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const long long e = a ? (long long)a[(size_t)x * N + c] : 0;
    u64 r;
    if (m) {
        const long long mv = m[(size_t)x * N + c];
        const u64 rm = mv >= 0 ? reduce64((u64)mv, M) : negmod(reduce64((u64)(-(mv + 1)) + 1ull, M), M.q);
        const u64 re = e >= 0 ? (u64)e : M.q - (u64)(-e);
        r = addmod(rm, re, M.q);
    } else {
        r = e >= 0 ? (u64)e : M.q - (u64)(-e);
    }
    out[(size_t)x * out_x_stride + (size_t)slot * N + c] = r;
}
// evaluation-form automorphism on [n limbs][N]: out[j] = in[perm_g(j)]. grid (N/256, n)
__global__ __launch_bounds__(256) void k_automorph(int logN, const u64 *__restrict__ in, u64 *__restrict__ out, unsigned g) {
    const unsigned N = 1u << logN, co = blockIdx.x * 256 + threadIdx.x;
    const unsigned e = ((2u * (__brev(co) >> (32 - logN)) + 1u) * g) & (2u * N - 1u);
    const unsigned c = __brev((e - 1u) >> 1) >> (32 - logN);
    out[(size_t)blockIdx.y * N + co] = in[(size_t)blockIdx.y * N + c];
}
// o = a (*) b over [n limbs][N] with per-slot modulus. grid (N/256, n)
__global__ __launch_bounds__(256) void k_mul(const ModC *__restrict__ mod, int N, const u64 *__restrict__ a,
                                             const u64 *__restrict__ b, u64 *__restrict__ o, LimbSel sel) {
    const ModC M = mod[sel.mod[blockIdx.y]];
    const size_t i = (size_t)blockIdx.y * N + (size_t)blockIdx.x * 256 + threadIdx.x;
    o[i] = mulmod(a[i], b[i], M);
}
// public key: b[j] = e[j] - a[j] s[j]. grid (N/256, nQ)
__global__ __launch_bounds__(256) void k_pk_combine(const ModC *__restrict__ mod, int N, u64 *__restrict__ b,
                                                    const u64 *__restrict__ a, const u64 *__restrict__ s) {
    const ModC M = mod[blockIdx.y];
    const size_t i = (size_t)blockIdx.y * N + (size_t)blockIdx.x * 256 + threadIdx.x;
    b[i] = submod(b[i], mulmod(a[i], s[i], M), M.q);
}
// switching key: b[d][m] = e[d][m] - a[d][m] s_enc[m] + [m in digit d] P s_from[m].  key [dnum][2][nT][N], e [dnum][nT][N]
// grid (N/256, nT, dnum)
__global__ __launch_bounds__(256) void k_evk_combine(const ModC *__restrict__ mod, int N, int nT, int nQ, int alpha,
                                                     u64 *__restrict__ key, const u64 *__restrict__ e,
                                                     const u64 *__restrict__ s_enc, const u64 *__restrict__ s_from,
                                                     ScaleSel pmodq) {
    const int m = blockIdx.y, d = blockIdx.z;
    const ModC M = mod[m];
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u64 a = key[(((size_t)d * 2 + 1) * nT + m) * N + c];
    u64 v = submod(e[((size_t)d * nT + m) * N + c], mulmod(a, s_enc[(size_t)m * N + c], M), M.q);
    if (m < nQ && m / alpha == d) v = addmod(v, mulmod(pmodq.s[m], s_from[(size_t)m * N + c], M), M.q);
    key[(((size_t)d * 2 + 0) * nT + m) * N + c] = v;
}
// c0 = b u + t0 ; c1 = a u + t1.  ct [X][2][nQ][N]; u,t0,t1 [X][nQ][N]; pk [2][nQ][N]. grid (N/256, nQ, X)
__global__ __launch_bounds__(256) void k_enc_combine(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ pk,
                                                     const u64 *__restrict__ u, const u64 *__restrict__ t0,
                                                     const u64 *__restrict__ t1, u64 *__restrict__ ct) {
    const int j = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[j];
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t i = ((size_t)x * nQ + j) * N + c;
    const u64 uu = u[i];
    ct[(((size_t)x * 2 + 0) * nQ + j) * N + c] = addmod(mulmod(pk[(size_t)j * N + c], uu, M), t0[i], M.q);
    ct[(((size_t)x * 2 + 1) * nQ + j) * N + c] = addmod(mulmod(pk[((size_t)nQ + j) * N + c], uu, M), t1[i], M.q);
}
// seeded secret-key encryption: c0[x][j] = t0[x][j] - a s[j], a = the uniform residues of stream sbase + j + (x << 16) under the PUBLIC
// key `akey` — k_sample_uniform's thread (one ChaCha block = 4 residues, the same reduce128) fused with the combine, so `a` reaches
// memory only when c1 is given.  t0, c0, c1 [X][nQ][N]; s [>= nQ][N].  16-byte loads and stores.  grid (N/4/256 rounded up, nQ, X)
__global__ __launch_bounds__(256) void k_enc_sym(ChaChaKey akey, const ModC *__restrict__ mod, int N, int nQ, u64 sbase,
                                                 const u64 *__restrict__ t0, const u64 *__restrict__ s, u64 *__restrict__ c0,
                                                 u64 *__restrict__ c1) {
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk * 4 >= N) return;
    const int j = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[j];
    u64 a[4];
    chacha_uniform4(akey, sbase + (u64)j + ((u64)x << 16), (u64)blk, M, a);
    const size_t is = (size_t)j * N + (size_t)blk * 4, i = (size_t)x * nQ * N + is;
    const ulonglong2 *tp = (const ulonglong2 *)(t0 + i), *sp = (const ulonglong2 *)(s + is);
    ulonglong2 *op = (ulonglong2 *)(c0 + i);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const ulonglong2 tv = tp[h], sv = sp[h];
        op[h] = make_ulonglong2(submod(tv.x, mulmod(a[2 * h], sv.x, M), M.q), submod(tv.y, mulmod(a[2 * h + 1], sv.y, M), M.q));
    }
    if (c1) {
        ulonglong2 *ap = (ulonglong2 *)(c1 + i);
        ap[0] = make_ulonglong2(a[0], a[1]);
        ap[1] = make_ulonglong2(a[2], a[3]);
    }
}
// decryption dot product on the first nu limbs: t[x][j] = c0 + s (c1 + s c2 ...). grid (N/256, nu, X)
__global__ __launch_bounds__(256) void k_dec_dot(const ModC *__restrict__ mod, int N, int npoly, int nl,
                                                 const u64 *__restrict__ ct, const u64 *__restrict__ s, u64 *__restrict__ t,
                                                 int nu) {
    const int j = blockIdx.y, x = blockIdx.z;
    const ModC M = mod[j];
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const u64 sv = s[(size_t)j * N + c];
    u64 acc = ct[(((size_t)x * npoly + (npoly - 1)) * nl + j) * N + c];
    for (int p = npoly - 2; p >= 0; p--) acc = addmod(mulmod(acc, sv, M), ct[(((size_t)x * npoly + p) * nl + j) * N + c], M.q);
    t[((size_t)x * nu + j) * N + c] = acc;
}

// ------------------------------------------------------------------------------------------------ canonical embedding
// one radix-2 stage of the slots->coefficients transform ("fftSpecialInv"); v [X][Nh] complex. grid (Nh/2/256, X)
__global__ __launch_bounds__(256) void k_fft_inv_stage(double2 *__restrict__ v, int Nh, int len, int M,
                                                       const unsigned *__restrict__ rot_group,
                                                       const double2 *__restrict__ ksi) {
    const int b = blockIdx.x * 256 + threadIdx.x;  // butterfly id < Nh/2
    const int lenh = len >> 1, lenq = len << 2, gap = M / lenq;
    const int j = b % lenh, i = (b / lenh) * len;
    double2 *p = v + (size_t)blockIdx.y * Nh;
    const int idx = (lenq - (int)(rot_group[j] % (unsigned)lenq)) * gap;
    const double2 w = ksi[idx];
    const double2 A = p[i + j], B = p[i + j + lenh];
    const double ur = A.x + B.x, ui = A.y + B.y, dr = A.x - B.x, di = A.y - B.y;
    const double m0 = dr * w.x, m1 = di * w.y, m2 = dr * w.y, m3 = di * w.x;
    p[i + j] = make_double2(ur, ui);
    p[i + j + lenh] = make_double2(m0 - m1, m2 + m3);
}
// one stage of the coefficients->slots transform ("fftSpecial")
__global__ __launch_bounds__(256) void k_fft_fwd_stage(double2 *__restrict__ v, int Nh, int len, int M,
                                                       const unsigned *__restrict__ rot_group,
                                                       const double2 *__restrict__ ksi) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int lenh = len >> 1, lenq = len << 2, gap = M / lenq;
    const int j = b % lenh, i = (b / lenh) * len;
    double2 *p = v + (size_t)blockIdx.y * Nh;
    const int idx = (int)(rot_group[j] % (unsigned)lenq) * gap;
    const double2 w = ksi[idx];
    const double2 A = p[i + j], B = p[i + j + lenh];
    const double m0 = B.x * w.x, m1 = B.y * w.y, m2 = B.x * w.y, m3 = B.y * w.x;
    const double tr = m0 - m1, ti = m2 + m3;
    p[i + j] = make_double2(A.x + tr, A.y + ti);
    p[i + j + lenh] = make_double2(A.x - tr, A.y - ti);
}
// real slot values -> complex work array. grid (Nh/256, X)
__global__ __launch_bounds__(256) void k_slots_to_complex(const double *__restrict__ slots, double2 *__restrict__ v, int Nh) {
    const size_t i = (size_t)blockIdx.y * Nh + (size_t)blockIdx.x * 256 + threadIdx.x;
    v[i] = make_double2(slots[i], 0.0);
}
// after the last inverse stage: bit-reverse, scale by 1/Nh, then round(re*scale), round(im*scale) -> int64 coeffs [X][N]
__global__ __launch_bounds__(256) void k_encode_finish(const double2 *__restrict__ v, long long *__restrict__ coeffs, int Nh,
                                                       int logNh, double scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int r = (int)(__brev((unsigned)i) >> (32 - logNh));
    const double2 a = v[(size_t)blockIdx.y * Nh + r];
    const double inv = 1.0 / (double)Nh;
    const double re = a.x * inv, im = a.y * inv;
    long long *o = coeffs + (size_t)blockIdx.y * 2 * Nh;
    o[i] = __double2ll_rn(re * scale);
    o[i + Nh] = __double2ll_rn(im * scale);
}
// decode front: centred CRT of the first nu (1 or 2) limbs (coefficient form, t [X][nu][N]) -> value/scale, written in
// BIT-REVERSED complex order ready for the forward stages. grid (Nh/256, X)
__global__ __launch_bounds__(256) void k_decode_front(const ModC *__restrict__ mod, const u64 *__restrict__ t, int nu, int N,
                                                      int logNh, double scale, u64 q0inv_mod_q1, double2 *__restrict__ v) {
    const int Nh = N >> 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const u64 *p = t + (size_t)blockIdx.y * nu * N;
    double val[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int c = i + h * Nh;
        double r;
        if (nu >= 2) {
            const ModC M0 = mod[0], M1 = mod[1];
            const u64 r0 = p[c], r1 = p[(size_t)N + c];
            const u64 d = submod(r1, reduce64(r0, M1), M1.q);
            const u64 tt = mulmod(d, q0inv_mod_q1, M1);
            const u128 Q = (u128)M0.q * M1.q, x = (u128)r0 + (u128)M0.q * tt;
            const bool neg = x > (Q >> 1);
            const u128 mag = neg ? Q - x : x;
            const double vv = (double)(u64)(mag >> 64) * 18446744073709551616.0 + (double)(u64)mag;
            r = (neg ? -vv : vv) / scale;
        } else {
            const u64 q0 = mod[0].q, r0 = p[c];
            const bool neg = r0 > (q0 >> 1);
            const double vv = (double)(neg ? q0 - r0 : r0);
            r = (neg ? -vv : vv) / scale;
        }
        val[h] = r;
    }
    const int rr = (int)(__brev((unsigned)i) >> (32 - logNh));
    v[(size_t)blockIdx.y * Nh + rr] = make_double2(val[0], val[1]);
}
__global__ __launch_bounds__(256) void k_complex_real(const double2 *__restrict__ v, double *__restrict__ out, int Nh) {
    const size_t i = (size_t)blockIdx.y * Nh + (size_t)blockIdx.x * 256 + threadIdx.x;
    out[i] = v[i].x;
}

// ------------------------------------------------------------------------------------------------ enroller packing
// DiagonalEnroller's splitIntoSquareMatrices + preprocessToDiagonalForm + concatenateRows for ONE ciphertext group g:
// slots[i][j*dim + r] = db[(g*per + j)*dim + r][(r + i) mod dim] (0 beyond n).  dbg points at row g*per*dim.
// grid (slots/256, dim)
// babies > 0 (baby-step / giant-step form of the mat-vec): diagonal i is rotated by -babies * (i / babies) slots in the clear, i.e. output
// slot s takes what the plain layout has in slot s - babies * (i / babies) (mod Nh)
// row0 > 0 (an in-place update: the sparse image of a block whose only non-zero rows are the given ones): dbg's rows go to slots
// [row0, row0 + rows_left) of the plain layout and zeros go everywhere else, in both forms
__global__ __launch_bounds__(256) void k_diag_pack(const double *__restrict__ dbg, long long rows_left, int dim, int Nh,
                                                   double *__restrict__ slots, int babies, int row0) {
    const int so = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    const int s = babies > 0 ? (so + Nh - (babies * (i / babies)) % Nh) % Nh : so;
    const int r = s % dim;
    const long long v = (long long)s - row0;  // row inside this group = j*dim + r = s; row of dbg = s - row0
    slots[(size_t)i * Nh + so] = (v >= 0 && v < rows_left) ? dbg[(size_t)v * dim + (r + i) % dim] : 0.0;
}

// HersEnroller::serializeDBThread (/root/reference/src/enroller/enroller_hers.cpp:108-113): slots[j][k] = db[m*S + k][j].
// grid (Nh/256, dim)
__global__ __launch_bounds__(256) void k_hers_pack(const double *__restrict__ dbg, long long rows_left, int dim, int Nh,
                                                   double *__restrict__ slots) {
    const int k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    slots[(size_t)j * Nh + k] = k < rows_left ? dbg[(size_t)k * dim + j] : 0.0;
}
// BaseEnroller::serializeDB's packing (/root/reference/src/enroller/enroller_base.cpp:28-44): database ciphertext x holds vectors
// x vpc .. x vpc + vpc - 1 back to back, i.e. slot s of vector x is element x Nh + s of the row-major normalised rows; zeros past the
// last row.  grid (Nh/256, X)
__global__ __launch_bounds__(256) void k_row_pack(const double *__restrict__ dbg, long long elems_left, int Nh, double *__restrict__ slots) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const long long e = (long long)blockIdx.y * Nh + s;
    slots[e] = e < elems_left ? dbg[e] : 0.0;
}
// BlindEnroller::serializeDBThread's packing (/root/reference/src/enroller/enroller_blind.cpp:66-80) for ONE matrix: slot image c holds
// coordinates [c chunk, (c + 1) chunk) of vector v at slots [v chunk, (v + 1) chunk), zeros past the last row.  rows points at the
// matrix's first vector (row-major, dim values each).  grid (Nh/256, dim / chunk)
__global__ __launch_bounds__(256) void k_chunk_pack(const double *__restrict__ rows, long long rows_left, int dim, int chunk, int Nh,
                                                    double *__restrict__ slots) {
    const int s = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    const long long v = s / chunk;
    slots[(size_t)c * Nh + s] = v < rows_left ? rows[(size_t)v * dim + (size_t)c * chunk + s % chunk] : 0.0;
}
// BlindReceiver::encryptQueryThread (/root/reference/src/receiver/receiver_blind.cpp:58-67): slot image c = chunk c of the query tiled
// over all slots.  grid (Nh/256, dim / chunk)
__global__ __launch_bounds__(256) void k_chunk_tile(const double *__restrict__ q, int chunk, int Nh, double *__restrict__ slots) {
    const int s = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    slots[(size_t)c * Nh + s] = q[(size_t)c * chunk + s % chunk];
}
// HersReceiver::encryptQueryThread (/root/reference/src/receiver/receiver_hers.cpp:58-63): every slot = coordinate i
__global__ __launch_bounds__(256) void k_broadcast_rows(const double *__restrict__ vals, int Nh, double *__restrict__ slots) {
    slots[(size_t)blockIdx.y * Nh + blockIdx.x * 256 + threadIdx.x] = vals[blockIdx.y];
}

// ---- templates that are already in device memory (f64 / f32 / f16 / bf16 rows, `stride` elements apart): dense double rows
// dst[n][dim], the d_rows buffer k_diag_pack reads — widened exactly and, with normalise != 0, divided by their L2 norm bit for bit
// as normalize() in client.cpp does it on the host (rows_norm.h: the squared sum runs in index order, so ONE thread owns a row's
// sum).  src is only ever read, element by element: nothing but the element's own alignment is assumed.
// A workgroup takes a tile of RW_ROWS rows.  Pass 1 (normalise only): RW_COLS columns at a time are loaded by all 256 threads —
// consecutive threads take consecutive elements of a row, so a wave reads whole runs of a row — widened and parked in LDS; lane r of
// wave 0 then walks row r there.  The row pitch is odd in doubles: at one column the 32 lanes of a ds_read_b64 group hit the 32
// different even banks.  Pass 2: all threads read the tile again (from cache), divide by the row's norm and write dst coalesced.
// dim is a power of two.  grid ((n + RW_ROWS - 1) / RW_ROWS), 256 threads
#define RW_ROWS 64
#define RW_COLS 64
#define RW_PITCH (RW_COLS + 1)
struct bf16_bits {
    unsigned short b;
};
DEV double rw_widen(double v) { return v; }
DEV double rw_widen(float v) { return rn_widen_f32_bits(__builtin_bit_cast(unsigned, v)); }
DEV double rw_widen(_Float16 v) { return rn_widen_f16_bits(__builtin_bit_cast(unsigned short, v)); }
DEV double rw_widen(bf16_bits v) { return rn_widen_bf16_bits(v.b); }

template <typename T>
__global__ __launch_bounds__(256) void k_rows_widen(const T *__restrict__ src, long long n, int log_dim, long long stride, int normalise,
                                                    double *__restrict__ dst) {
    __shared__ double tile[RW_ROWS * RW_PITCH];
    __shared__ double norm[RW_ROWS];
    const int t = threadIdx.x, dim = 1 << log_dim;
    const long long row0 = (long long)blockIdx.x * RW_ROWS;
    const int rows = (int)(n - row0 < RW_ROWS ? n - row0 : RW_ROWS);
    if (normalise) {
        const int log_cols = log_dim < 6 ? log_dim : 6, cols = 1 << log_cols;  // min(dim, RW_COLS)
        double m = 0.0;
        for (int c0 = 0; c0 < dim; c0 += cols) {
            for (int e = t; e < rows << log_cols; e += 256) {
                const int r = e >> log_cols, c = e & (cols - 1);
                tile[r * RW_PITCH + c] = rw_widen(src[(row0 + r) * stride + c0 + c]);
            }
            __syncthreads();
            if (t < rows)
                for (int c = 0; c < cols; c++) m = rn_sq_step(m, tile[t * RW_PITCH + c]);
            __syncthreads();
        }
        if (t < RW_ROWS) norm[t] = rn_norm(m);
        __syncthreads();
    }
    for (int e = t; e < rows << log_dim; e += 256) {
        const int r = e >> log_dim, c = e & (dim - 1);
        double v = rw_widen(src[(row0 + r) * stride + c]);
        if (normalise) v = rn_quot(v, norm[r]);
        dst[((row0 + r) << log_dim) + c] = v;
    }
}
// DiagonalReceiver::encryptQuery's tiling (/root/reference/src/receiver/receiver_diag.cpp:18-21) for Q probes at once: slot image q =
// row q of rows[Q][dim] (k_rows_widen's output) repeated over all slots.  dim is a power of two.  grid (Nh/256, Q)
__global__ __launch_bounds__(256) void k_query_tile(const double *__restrict__ rows, int dim, int Nh, double *__restrict__ slots) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    slots[(size_t)blockIdx.y * Nh + s] = rows[(size_t)blockIdx.y * dim + (s & (dim - 1))];
}

}  // namespace

namespace hc {

void sample_uniform(hipStream_t st, const ChaChaKey &key, const ModC *mod, int N, u64 sbase, u64 step_y, u64 step_z,
                    u64 *dst, size_t stride_y, size_t stride_z, const LimbSel &ysel, int nz) {
    const int blocks = (N / 4 + 255) / 256;
    hipLaunchKernelGGL(k_sample_uniform, dim3(blocks, ysel.n, nz), dim3(256), 0, st, key, mod, N, sbase, step_y, step_z, dst,
                       stride_y, stride_z, ysel);
}
void sample_ternary(hipStream_t st, const ChaChaKey &key, int N, u64 sbase, u64 step, int *dst, int X) {
    hipLaunchKernelGGL(k_sample_small<0>, dim3((N / 16 + 255) / 256, X), dim3(256), 0, st, key, N, sbase, step, dst);
}
void sample_gauss(hipStream_t st, const ChaChaKey &key, int N, u64 sbase, u64 step, int *dst, int X) {
    hipLaunchKernelGGL(k_sample_small<1>, dim3((N / 8 + 255) / 256, X), dim3(256), 0, st, key, N, sbase, step, dst);
}
void small_to_limbs(hipStream_t st, const ModC *mod, int N, const int *a, const long long *m, u64 *out,
                    size_t out_x_stride, int X, const LimbSel &sel) {
    hipLaunchKernelGGL(k_small_to_limbs, dim3(N / 256, sel.n, X), dim3(256), 0, st, mod, N, a, m, out, out_x_stride, sel);
}
void automorph(hipStream_t st, int logN, const u64 *in, u64 *out, unsigned g, int nlimbs) {
    hipLaunchKernelGGL(k_automorph, dim3((1 << logN) / 256, nlimbs), dim3(256), 0, st, logN, in, out, g);
}
void mul(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, const LimbSel &sel) {
    hipLaunchKernelGGL(k_mul, dim3(N / 256, sel.n), dim3(256), 0, st, mod, N, a, b, o, sel);
}
void pk_combine(hipStream_t st, const ModC *mod, int N, int nQ, u64 *b, const u64 *a, const u64 *s) {
    hipLaunchKernelGGL(k_pk_combine, dim3(N / 256, nQ), dim3(256), 0, st, mod, N, b, a, s);
}
void evk_combine(hipStream_t st, const ModC *mod, int N, int nT, int nQ, int alpha, int dnum, u64 *key, const u64 *e,
                 const u64 *s_enc, const u64 *s_from, const ScaleSel &pmodq) {
    hipLaunchKernelGGL(k_evk_combine, dim3(N / 256, nT, dnum), dim3(256), 0, st, mod, N, nT, nQ, alpha, key, e, s_enc, s_from,
                       pmodq);
}
void enc_combine(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *pk, const u64 *u, const u64 *t0, const u64 *t1,
                 u64 *ct, int X) {
    hipLaunchKernelGGL(k_enc_combine, dim3(N / 256, nQ, X), dim3(256), 0, st, mod, N, nQ, pk, u, t0, t1, ct);
}
void enc_sym(hipStream_t st, const ChaChaKey &akey, const ModC *mod, int N, int nQ, u64 sbase, const u64 *t0, const u64 *s, u64 *c0,
             u64 *c1, int X) {
    if (X < 1 || X > 65535) throw std::runtime_error("hydia: enc_sym takes 1 .. 65535 polynomials per launch");
    hipLaunchKernelGGL(k_enc_sym, dim3((N / 4 + 255) / 256, nQ, X), dim3(256), 0, st, akey, mod, N, nQ, sbase, t0, s, c0, c1);
}
void dec_dot(hipStream_t st, const ModC *mod, int N, int npoly, int nl, const u64 *ct, const u64 *s, u64 *t, int nu, int X) {
    hipLaunchKernelGGL(k_dec_dot, dim3(N / 256, nu, X), dim3(256), 0, st, mod, N, npoly, nl, ct, s, t, nu);
}
void encode(hipStream_t st, const double *slots, double2 *work, long long *coeffs, int N, int X, double scale,
            const unsigned *rot_group, const double2 *ksi) {
    const int Nh = N / 2, M = 2 * N;
    int logNh = 0;
    while ((1 << logNh) < Nh) logNh++;
    hipLaunchKernelGGL(k_slots_to_complex, dim3(Nh / 256, X), dim3(256), 0, st, slots, work, Nh);
    for (int len = Nh; len >= 2; len >>= 1)
        hipLaunchKernelGGL(k_fft_inv_stage, dim3(Nh / 2 / 256, X), dim3(256), 0, st, work, Nh, len, M, rot_group, ksi);
    hipLaunchKernelGGL(k_encode_finish, dim3(Nh / 256, X), dim3(256), 0, st, work, coeffs, Nh, logNh, scale);
}
void decode(hipStream_t st, const ModC *mod, const u64 *t, int nu, int N, int X, double scale, u64 q0inv_mod_q1,
            double2 *work, double *out, const unsigned *rot_group, const double2 *ksi) {
    const int Nh = N / 2, M = 2 * N;
    int logNh = 0;
    while ((1 << logNh) < Nh) logNh++;
    hipLaunchKernelGGL(k_decode_front, dim3(Nh / 256, X), dim3(256), 0, st, mod, t, nu, N, logNh, scale, q0inv_mod_q1, work);
    for (int len = 2; len <= Nh; len <<= 1)
        hipLaunchKernelGGL(k_fft_fwd_stage, dim3(Nh / 2 / 256, X), dim3(256), 0, st, work, Nh, len, M, rot_group, ksi);
    hipLaunchKernelGGL(k_complex_real, dim3(Nh / 256, X), dim3(256), 0, st, work, out, Nh);
}
void hers_pack(hipStream_t st, const double *dbg, long long rows_left, int dim, int Nh, double *slots) {
    hipLaunchKernelGGL(k_hers_pack, dim3(Nh / 256, dim), dim3(256), 0, st, dbg, rows_left, dim, Nh, slots);
}
void chunk_pack(hipStream_t st, const double *rows, long long rows_left, int dim, int chunk, int Nh, double *slots) {
    hipLaunchKernelGGL(k_chunk_pack, dim3(Nh / 256, dim / chunk), dim3(256), 0, st, rows, rows_left, dim, chunk, Nh, slots);
}
void chunk_tile(hipStream_t st, const double *q, int dim, int chunk, int Nh, double *slots) {
    hipLaunchKernelGGL(k_chunk_tile, dim3(Nh / 256, dim / chunk), dim3(256), 0, st, q, chunk, Nh, slots);
}
void row_pack(hipStream_t st, const double *dbg, long long elems_left, int Nh, double *slots, int X) {
    hipLaunchKernelGGL(k_row_pack, dim3(Nh / 256, X), dim3(256), 0, st, dbg, elems_left, Nh, slots);
}
void broadcast_rows(hipStream_t st, const double *vals, int dim, int Nh, double *slots) {
    hipLaunchKernelGGL(k_broadcast_rows, dim3(Nh / 256, dim), dim3(256), 0, st, vals, Nh, slots);
}
void diag_pack(hipStream_t st, const double *dbg, long long rows_left, int dim, int Nh, double *slots, int babies, int row0) {
    hipLaunchKernelGGL(k_diag_pack, dim3(Nh / 256, dim), dim3(256), 0, st, dbg, rows_left, dim, Nh, slots, babies, row0);
}
size_t rows_elem_size(int dtype) { return dtype == HC_ROWS_F64 ? 8 : dtype == HC_ROWS_F32 ? 4 : 2; }
void rows_widen(hipStream_t st, const void *src, int dtype, size_t n, int dim, size_t stride, int normalise, double *dst) {
    if (n == 0) return;
    int log_dim = 0;
    while ((1 << log_dim) < dim) log_dim++;
    if ((1 << log_dim) != dim || stride < (size_t)dim || n > (size_t)0x7FFFFFFF * RW_ROWS)
        throw std::runtime_error("hydia: rows_widen takes a power-of-two dimension, a row stride of at least it and fewer than 2^37 rows");
    const dim3 grid((unsigned)((n + RW_ROWS - 1) / RW_ROWS)), block(256);
    const long long nn = (long long)n, ss = (long long)stride;
    switch (dtype) {
        case HC_ROWS_F64: hipLaunchKernelGGL(k_rows_widen<double>, grid, block, 0, st, (const double *)src, nn, log_dim, ss, normalise, dst); break;
        case HC_ROWS_F32: hipLaunchKernelGGL(k_rows_widen<float>, grid, block, 0, st, (const float *)src, nn, log_dim, ss, normalise, dst); break;
        case HC_ROWS_F16: hipLaunchKernelGGL(k_rows_widen<_Float16>, grid, block, 0, st, (const _Float16 *)src, nn, log_dim, ss, normalise, dst); break;
        case HC_ROWS_BF16: hipLaunchKernelGGL(k_rows_widen<bf16_bits>, grid, block, 0, st, (const bf16_bits *)src, nn, log_dim, ss, normalise, dst); break;
        default: throw std::runtime_error("hydia: rows_widen: element type outside f64 / f32 / f16 / bf16");
    }
}
void query_tile(hipStream_t st, const double *rows, int Q, int dim, int Nh, double *slots) {
    hipLaunchKernelGGL(k_query_tile, dim3(Nh / 256, Q), dim3(256), 0, st, rows, dim, Nh, slots);
}

}  // namespace hc
