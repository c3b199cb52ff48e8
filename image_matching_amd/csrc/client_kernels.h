// image_matching_amd/csrc/client_kernels.h — launch interface of client_kernels.hip
#pragma once
#include "kernels.h"

#include "chacha_dev.h"  // ChaChaKey, the ChaCha20 block and the uniform residues drawn from it (after kernels.h: it needs the HIP runtime's attributes)

// stream ids of the deterministic sampler specification (DESIGN.md §"Randomness")
#define HY_DOM_SK 1ull
#define HY_DOM_PK_A 2ull
#define HY_DOM_PK_E 3ull
#define HY_DOM_EVK_A 4ull
#define HY_DOM_EVK_E 5ull
#define HY_DOM_ENC_U 6ull
#define HY_DOM_ENC_E0 7ull
#define HY_DOM_ENC_E1 8ull
#define HY_DOM_SYM_A 9ull  // c1 = a of a seeded secret-key query, under the PUBLIC expansion seed: (9, nonce, 0, limb)
#define HY_STREAM(dom, a, b, c) (((u64)(dom) << 56) | ((u64)(a) << 16) | ((u64)(b) << 8) | (u64)(c))

namespace hc {
void sample_uniform(hipStream_t st, const ChaChaKey &key, const ModC *mod, int N, u64 sbase, u64 step_y, u64 step_z,
                    u64 *dst, size_t stride_y, size_t stride_z, const LimbSel &ysel, int nz);
void sample_ternary(hipStream_t st, const ChaChaKey &key, int N, u64 sbase, u64 step, int *dst, int X);
void sample_gauss(hipStream_t st, const ChaChaKey &key, int N, u64 sbase, u64 step, int *dst, int X);
void small_to_limbs(hipStream_t st, const ModC *mod, int N, const int *a, const long long *m, u64 *out,
                    size_t out_x_stride, int X, const LimbSel &sel);
void automorph(hipStream_t st, int logN, const u64 *in, u64 *out, unsigned g, int nlimbs);
void mul(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, const LimbSel &sel);
void pk_combine(hipStream_t st, const ModC *mod, int N, int nQ, u64 *b, const u64 *a, const u64 *s);
void evk_combine(hipStream_t st, const ModC *mod, int N, int nT, int nQ, int alpha, int dnum, u64 *key, const u64 *e,
                 const u64 *s_enc, const u64 *s_from, const ScaleSel &pmodq);
void enc_combine(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *pk, const u64 *u, const u64 *t0, const u64 *t1,
                 u64 *ct, int X);
// seeded secret-key encryption of X polynomials (X <= 65535): c0[x][j] = t0[x][j] - a s[j] with a = sample_uniform(akey, sbase, step_y
// 1, step_z 1 << 16) limb j of element x, drawn inside the kernel; a is also written to c1 [X][nQ][N] when c1 != nullptr
void enc_sym(hipStream_t st, const ChaChaKey &akey, const ModC *mod, int N, int nQ, u64 sbase, const u64 *t0, const u64 *s, u64 *c0,
             u64 *c1, int X);
void dec_dot(hipStream_t st, const ModC *mod, int N, int npoly, int nl, const u64 *ct, const u64 *s, u64 *t, int nu, int X);
void encode(hipStream_t st, const double *slots, double2 *work, long long *coeffs, int N, int X, double scale,
            const unsigned *rot_group, const double2 *ksi);
void decode(hipStream_t st, const ModC *mod, const u64 *t, int nu, int N, int X, double scale, u64 q0inv_mod_q1,
            double2 *work, double *out, const unsigned *rot_group, const double2 *ksi);
void diag_pack(hipStream_t st, const double *dbg, long long rows_left, int dim, int Nh, double *slots, int babies = 0, int row0 = 0);
// HERS (approach 4): slots[j][k] = dbg[k][j] (column packing); query coordinate i broadcast to every slot of vector i
void hers_pack(hipStream_t st, const double *dbg, long long rows_left, int dim, int Nh, double *slots);
// BaseEnroller (approach 1): slot vector x = rows x vpc .. x vpc + vpc - 1 back to back (vpc = Nh / dim), zeros past the last row
void row_pack(hipStream_t st, const double *dbg, long long elems_left, int Nh, double *slots, int X);
// approach 3: the dim / chunk slot images of one matrix of Nh / chunk vectors, and the dim / chunk tiled images of a query
void chunk_pack(hipStream_t st, const double *rows, long long rows_left, int dim, int chunk, int Nh, double *slots);
void chunk_tile(hipStream_t st, const double *q, int dim, int chunk, int Nh, double *slots);
void broadcast_rows(hipStream_t st, const double *vals, int dim, int Nh, double *slots);
// templates in device memory: n rows of dim elements of type `dtype` (the values of hydia_dtype), `stride` elements apart (>= dim, dim
// a power of two), widened exactly to dense doubles dst[n][dim] — diag_pack's input — and with normalise != 0 divided by their L2
// norm bit for bit as the host normalises (rows_norm.h).  src is never written and needs only its element's alignment
#define HC_ROWS_F64 0
#define HC_ROWS_F32 1
#define HC_ROWS_F16 2
#define HC_ROWS_BF16 3
size_t rows_elem_size(int dtype);
void rows_widen(hipStream_t st, const void *src, int dtype, size_t n, int dim, size_t stride, int normalise, double *dst);
// slots[q][i] = rows[q][i mod dim] for Q probes (Q <= 65535): the tiling of DiagonalReceiver::encryptQuery
void query_tile(hipStream_t st, const double *rows, int Q, int dim, int Nh, double *slots);
}  // namespace hc

// ---- wire_kernels.hip: the wire format's rows (wire_format.h).  off[j] = the 64-bit word at which limb j's packed row starts inside one
// polynomial's run of rows, off[limbs] = the words of one polynomial: N / 64 granules of w_j words each
struct WireRows {
    unsigned off[HY_MAX_MODS + 1];
};
namespace hc {
WireRows wire_rows(const u64 *moduli, int N, int nl);  // limb j <-> moduli[j] (the context's chain: limb j is modulus j of `mod` below)
// rows [items][npoly][nl] of N u64 residues at src + item * item_stride + poly * poly_stride + limb * N <-> packed rows back to back,
// dst [items][npoly][R.off[nl]] words.  unpack: *flag := 1 when a residue is >= its modulus (the caller clears it beforehand)
void wire_pack(hipStream_t st, const ModC *mod, int N, const u64 *src, size_t item_stride, size_t poly_stride, size_t items, int npoly,
               int nl, const WireRows &R, u64 *dst);
void wire_unpack_check(hipStream_t st, const ModC *mod, int N, const u64 *src, u64 *dst, size_t item_stride, size_t poly_stride, size_t items,
                       int npoly, int nl, const WireRows &R, unsigned *flag);
// the range check of wire_unpack_check alone: packed rows [items][npoly][R.off[nl]] words are read, nothing is written but *flag
void wire_check(hipStream_t st, const ModC *mod, int N, const u64 *src, size_t items, int npoly, int nl, const WireRows &R, unsigned *flag);
// one block of a database delta: resident ciphertexts t0 .. t0 + X - 1 += (store: :=) the packed rows [X][2][R.off[nQ]] words at src,
// mod q_j, in one pass (k_db_accumulate_wire / k_db_store_wire, and their 46-bit forms for the packed limbs of a bits46 layout).  The
// rows are canonical (wire_check) and L describes a ciphertext database
void db_wire(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *src, const WireRows &R, void *db, size_t t0, int X, const DbLayout &L,
             bool store);
// one block of a SEEDED database delta: the same for ciphertexts (c0_x, a_x), c0 from the packed rows [X][R.off[nQ]] words at src and
// a_x limb j = the uniform stream (SYM_A, nonce0 + x, 0, j) under akey, generated inside the kernel (k_db_accumulate_seeded /
// k_db_store_seeded and their 46-bit forms).  X <= 65535, nonce0 + X < 2^40
void db_wire_seeded(hipStream_t st, const ChaChaKey &akey, u64 nonce0, const ModC *mod, int N, int nQ, const u64 *src, const WireRows &R, void *db,
                    size_t t0, int X, const DbLayout &L, bool store);
}  // namespace hc
