// image_matching_amd/csrc/wire_kernels.hip — gfx950 kernels of the wire format (wire_format.h, include/hydia.h "wire messages"): residues
// packed into the bit length of their modulus on the way out, unpacked and range-checked on the way in.
//
// Further down: the range check alone (k_wire_check) and the kernels that take the packed rows of a database delta straight to the
// resident database (k_db_accumulate_wire, k_db_store_wire; include/hydia.h "database deltas"), and their seeded forms, which take
// the c0 halves alone and regenerate a where it is stored (k_db_accumulate_seeded, k_db_store_seeded).
//
// Pack and unpack are pure data movement.  The unit of both kernels is the GRANULE: 64 consecutive residues of one limb = exactly
// w 64-bit words of the packed row (w = the bit length of q_j, wave-uniform, read from ModC at run time — one kernel serves every width).  One wave owns one
// granule, so no two waves ever write one word and the pack needs no atomics.  Both sides of a granule are coalesced: lane c loads /
// stores residue c (512 contiguous bytes per wave), lane k < w stores / loads word k (8 w contiguous bytes); the bit gather between
// the two goes through a 512-byte LDS tile per wave.  A word holds pieces of at most ceil(64 / w) + 1 residues (three for the 45 .. 60
// bit limbs of this library's chains); the gather loop is general in w.
#include "client_kernels.h"
#include "db_accum.h"  // the per-granule arithmetic of an in-place update (host-checkable), shared with k_db_accumulate / k_db_accumulate46

#include <stdexcept>
#include <string>

namespace {

// rows [item][poly][limb] of N residues at src + item * item_stride + poly * poly_stride + limb * N (a limb-prefix view keeps its
// limb stride inside poly_stride; the b halves of a key skip the a halves through item_stride) -> packed rows, back to back.
// grid (N / 256, limbs, items * npoly), 4 granules per workgroup
__global__ __launch_bounds__(256) void k_wire_pack(const ModC *__restrict__ mod, int N, const u64 *__restrict__ src, size_t item_stride,
                                                   size_t poly_stride, int npoly, WireRows R, u64 *__restrict__ dst) {
    __shared__ u64 tile[4][64];
    const int j = blockIdx.y, z = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * 4 + wave;
    const int w = 64 - __clzll((long long)mod[j].q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;  // a residue wider than its field must not reach its neighbour's bits
    tile[wave][lane] = src[(size_t)(z / npoly) * item_stride + (size_t)(z % npoly) * poly_stride + (size_t)j * N + g * 64 + lane] & mask;
    __syncthreads();
    if (lane < w) {
        int c = (64 * lane) / w;            // the residue bit 64 * lane of the granule belongs to
        const int off = 64 * lane - c * w;  // its bits below that one went into the word before
        u64 word = tile[wave][c] >> off;
        for (int filled = w - off; filled < 64; filled += w) word |= tile[wave][++c] << filled;
        dst[(size_t)z * R.off[gridDim.y] + R.off[j] + g * w + lane] = word;
    }
}
// residue r of a run of whole granules held in LDS from its first word on: bits [r w, (r + 1) w) of the run (the run ends with a
// residue, so tile[k + 1] exists whenever the field crosses a word)
__device__ __forceinline__ u64 wire_field(const u64 *tile, int r, int w, u64 mask) {
    const int bit = r * w, k = bit >> 6, off = bit & 63;
    u64 v = tile[k] >> off;
    if (off + w > 64) v |= tile[k + 1] << (64 - off);
    return v & mask;
}
// the inverse, and the range check: *flag := 1 when any residue is at or above its modulus (never cleared here), in the style of
// k_db_check_canonical.  Same grid
__global__ __launch_bounds__(256) void k_wire_unpack_check(const ModC *__restrict__ mod, int N, const u64 *__restrict__ src, WireRows R,
                                                           u64 *__restrict__ dst, size_t item_stride, size_t poly_stride, int npoly,
                                                           unsigned *__restrict__ flag) {
    __shared__ u64 tile[4][64];
    const int j = blockIdx.y, z = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * 4 + wave;
    const u64 q = mod[j].q;
    const int w = 64 - __clzll((long long)q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;
    if (lane < w) tile[wave][lane] = src[(size_t)z * R.off[gridDim.y] + R.off[j] + g * w + lane];
    __syncthreads();
    const u64 v = wire_field(tile[wave], lane, w, mask);
    dst[(size_t)(z / npoly) * item_stride + (size_t)(z % npoly) * poly_stride + (size_t)j * N + g * 64 + lane] = v;
    if (__syncthreads_or(v >= q) && threadIdx.x == 0) *flag = 1u;
}

// the range check alone, for a message that is applied only after ALL of it passed (a database delta): same grid, same granule, same
// flag as k_wire_unpack_check; no destination is written
__global__ __launch_bounds__(256) void k_wire_check(const ModC *__restrict__ mod, const u64 *__restrict__ src, WireRows R,
                                                    unsigned *__restrict__ flag) {
    __shared__ u64 tile[4][64];
    const int j = blockIdx.y, z = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t g = (size_t)blockIdx.x * 4 + wave;
    const u64 q = mod[j].q;
    const int w = 64 - __clzll((long long)q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;
    if (lane < w) tile[wave][lane] = src[(size_t)z * R.off[gridDim.y] + R.off[j] + g * w + lane];
    __syncthreads();
    const u64 v = wire_field(tile[wave], lane, w, mask);
    if (__syncthreads_or(v >= q) && threadIdx.x == 0) *flag = 1u;
}

// ---- what the block bodies of a delta and of a seeded delta share
// the residues a thread owns += (STORE: :=) into the resident database: a residue pair (16 bytes, or pk: 12), or db_layout.h's 92-byte
// granule of sixteen 46-bit residues
template <bool STORE>
__device__ __forceinline__ void db_put_pair(unsigned char *d, bool pk, u64 ax, u64 ay, u64 q) {
    if (!STORE) {
        db_accumulate_pair(d, pk, ax, ay, q);
    } else if (pk) {
        unsigned v[3];
        db_pack_pair48(ax, ay, v);
        unsigned *o = reinterpret_cast<unsigned *>(d);
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
    } else {
        reinterpret_cast<u64 *>(d)[0] = ax;
        reinterpret_cast<u64 *>(d)[1] = ay;
    }
}
template <bool STORE>
__device__ __forceinline__ void db_put_granule46(unsigned char *d, const u64 a[16], u64 q) {
    unsigned *o = reinterpret_cast<unsigned *>(d);
    if (!STORE) {
        db_accumulate_granule46(o, a, q);
    } else {
        unsigned v[23];
        db_pack_granule46(a, v);
#pragma unroll
        for (int k = 0; k < 23; k++) o[k] = v[k];
    }
}
// the workgroup's PER * 256 residues of one limb's packed row, from residue c0 (a multiple of 64) on: whole granules, contiguous and
// coalesced, into LDS; returns how many residues that is (N is a multiple of 512)
template <int PER>
__device__ __forceinline__ int db_load_tile(u64 *tile, const u64 *__restrict__ row, int N, size_t c0, int w) {
    const int span = (int)((size_t)N - c0 < (size_t)(PER * 256) ? (size_t)N - c0 : (size_t)(PER * 256));
    row += (c0 >> 6) * w;
    for (int k = threadIdx.x; k < (span >> 6) * w; k += 256) tile[k] = row[k];
    __syncthreads();
    return span;
}

// Packed wire rows of ONE block -> the resident database, in one pass: ciphertexts t0 .. t0 + X - 1 += (STORE: :=) the rows
// [X][2][nQ] of a CT_BATCH payload, mod q_j.  No unpacked copy of the block in HBM: a workgroup loads the packed words of its PER * 256
// residues (whole granules, contiguous, coalesced) into LDS, and every thread gathers the residues of the database granule it OWNS —
// k_db_repack's map, a residue pair (PER = 2; 16 or 12 bytes), or k_db_repack46's, sixteen 46-bit residues = 23 dwords (PER = 16) —
// and runs db_accum.h's read-add-reduce-write on it (db_offset: either placement).  One thread owns every dword of the database it
// reads and writes: no atomics.  The residues were range-checked beforehand (k_wire_check): both operands are reduced.
// grid (ceil(N / (PER 256)), limbs, X * 2); limb j = blockIdx.y + j0
template <bool STORE, int PER>
__device__ __forceinline__ void db_wire_body(u64 *tile, const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ src, WireRows R,
                                             unsigned char *__restrict__ db, const DbLayout &L, size_t t0, int j0) {
    const int j = blockIdx.y + j0, xp = blockIdx.z, x = xp >> 1, p = xp & 1;
    const u64 q = mod[j].q;
    const int w = 64 - __clzll((long long)q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;
    const size_t c0 = (size_t)blockIdx.x * (PER * 256);  // first residue of the workgroup
    const int span = db_load_tile<PER>(tile, src + (size_t)xp * R.off[nQ] + R.off[j], N, c0, w), r0 = threadIdx.x * PER;
    if (r0 >= span) return;
    unsigned char *d = db + db_offset(L, N, t0 + x, p, j, c0 + r0);
    u64 v[PER];
#pragma unroll
    for (int r = 0; r < PER; r++) v[r] = wire_field(tile, r0 + r, w, mask);
    if constexpr (PER == 2) db_put_pair<STORE>(d, L.packed && j > 0, v[0], v[1], q);
    else db_put_granule46<STORE>(d, v, q);
}
// the 8-byte and 6-byte residues (limb 0, every limb of a 48-bit or unpacked layout): 512 residues = 8 granules <= 512 words per workgroup
__global__ __launch_bounds__(256) void k_db_accumulate_wire(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ src, WireRows R,
                                                            unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    __shared__ u64 tile[512];
    db_wire_body<false, 2>(tile, mod, N, nQ, src, R, db, L, t0, 0);
}
__global__ __launch_bounds__(256) void k_db_store_wire(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ src, WireRows R,
                                                       unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    __shared__ u64 tile[512];
    db_wire_body<true, 2>(tile, mod, N, nQ, src, R, db, L, t0, 0);
}
// the 46-bit limbs of a bits46 layout (q_j < 2^46, so w <= 46): 4096 residues = 64 granules <= 2944 words per workgroup; limb j =
// blockIdx.y + 1
__global__ __launch_bounds__(256) void k_db_accumulate_wire46(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ src, WireRows R,
                                                              unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    __shared__ u64 tile[64 * 46];
    db_wire_body<false, 16>(tile, mod, N, nQ, src, R, db, L, t0, 1);
}
__global__ __launch_bounds__(256) void k_db_store_wire46(const ModC *__restrict__ mod, int N, int nQ, const u64 *__restrict__ src, WireRows R,
                                                         unsigned char *__restrict__ db, DbLayout L, size_t t0) {
    __shared__ u64 tile[64 * 46];
    db_wire_body<true, 16>(tile, mod, N, nQ, src, R, db, L, t0, 1);
}

// ---- a SEEDED database delta (include/hydia.h "seeded database deltas"): one block's packed c0 rows [X][R.off[nQ]] words -> BOTH
// components of resident ciphertexts t0 .. t0 + X - 1 in one pass.  A workgroup takes a tile of PER * 256 residues of limb j of
// ciphertext x: component 0 += (STORE: :=) the c0 residues gathered from the packed words in LDS, exactly as db_wire_body does, and
// component 1 += (:=) the matching residues of a, REGENERATED here — stream (SYM_A, nonce0 + x, 0, j) under the public akey, ChaCha
// block = coefficient / 4, chacha_dev.h's chacha_uniform4, the thread of k_enc_sym and k_sample_uniform — so neither component has a
// 64-bit image in HBM and a is never read from anywhere.  A thread owns PER consecutive residues of both components: two residue pairs
// = ONE ChaCha block (PER = 4; 2 x 16 or 2 x 12 bytes, the pairs adjacent in either placement because 4 divides 128), or db_layout.h's
// 92-byte granule of sixteen 46-bit residues = FOUR blocks (PER = 16).  One thread owns every dword it reads and writes: no atomics.
// c0 was range-checked beforehand (k_wire_check) and a is reduced by construction: both operands of the add are canonical.
// grid (ceil(N / (PER 256)), limbs, X); limb j = blockIdx.y + j0
template <bool STORE, int PER>
__device__ __forceinline__ void db_seeded_body(u64 *tile, const ChaChaKey &akey, u64 nonce0, const ModC *__restrict__ mod, int N, int nQ,
                                               const u64 *__restrict__ src, WireRows R, unsigned char *__restrict__ db, const DbLayout &L,
                                               size_t t0, int j0) {
    const int j = blockIdx.y + j0, x = blockIdx.z;
    const ModC M = mod[j];
    const int w = 64 - __clzll((long long)M.q);
    const u64 mask = w == 64 ? ~0ull : (1ull << w) - 1;
    const size_t c0 = (size_t)blockIdx.x * (PER * 256);  // first residue of the workgroup
    const int span = db_load_tile<PER>(tile, src + (size_t)x * R.off[nQ] + R.off[j], N, c0, w), r0 = threadIdx.x * PER;
    if (r0 >= span) return;
    const u64 stream = HY_STREAM(HY_DOM_SYM_A, nonce0 + (u64)x, 0, j), blk0 = (u64)((c0 + r0) >> 2);
    unsigned char *d0 = db + db_offset(L, N, t0 + x, 0, j, c0 + r0), *d1 = db + db_offset(L, N, t0 + x, 1, j, c0 + r0);
    u64 v[PER];
#pragma unroll
    for (int r = 0; r < PER; r++) v[r] = wire_field(tile, r0 + r, w, mask);
    if constexpr (PER == 4) {
        const bool pk = L.packed && j > 0;
        const int pair_bytes = pk ? 12 : 16;
        db_put_pair<STORE>(d0, pk, v[0], v[1], M.q);
        db_put_pair<STORE>(d0 + pair_bytes, pk, v[2], v[3], M.q);
        chacha_uniform4(akey, stream, blk0, M, v);
        db_put_pair<STORE>(d1, pk, v[0], v[1], M.q);
        db_put_pair<STORE>(d1 + pair_bytes, pk, v[2], v[3], M.q);
    } else {
        db_put_granule46<STORE>(d0, v, M.q);
#pragma unroll
        for (int b = 0; b < PER / 4; b++) chacha_uniform4(akey, stream, blk0 + b, M, v + 4 * b);
        db_put_granule46<STORE>(d1, v, M.q);
    }
}
// the 8-byte and 6-byte residues (limb 0, every limb of a 48-bit or unpacked layout): 1024 residues = 16 granules <= 1024 words per workgroup
__global__ __launch_bounds__(256) void k_db_accumulate_seeded(ChaChaKey akey, u64 nonce0, const ModC *__restrict__ mod, int N, int nQ,
                                                              const u64 *__restrict__ src, WireRows R, unsigned char *__restrict__ db,
                                                              DbLayout L, size_t t0) {
    __shared__ u64 tile[1024];
    db_seeded_body<false, 4>(tile, akey, nonce0, mod, N, nQ, src, R, db, L, t0, 0);
}
__global__ __launch_bounds__(256) void k_db_store_seeded(ChaChaKey akey, u64 nonce0, const ModC *__restrict__ mod, int N, int nQ,
                                                         const u64 *__restrict__ src, WireRows R, unsigned char *__restrict__ db, DbLayout L,
                                                         size_t t0) {
    __shared__ u64 tile[1024];
    db_seeded_body<true, 4>(tile, akey, nonce0, mod, N, nQ, src, R, db, L, t0, 0);
}
// the 46-bit limbs of a bits46 layout (w <= 46): 4096 residues = 64 granules <= 2944 words per workgroup; limb j = blockIdx.y + 1
__global__ __launch_bounds__(256) void k_db_accumulate_seeded46(ChaChaKey akey, u64 nonce0, const ModC *__restrict__ mod, int N, int nQ,
                                                                const u64 *__restrict__ src, WireRows R, unsigned char *__restrict__ db,
                                                                DbLayout L, size_t t0) {
    __shared__ u64 tile[64 * 46];
    db_seeded_body<false, 16>(tile, akey, nonce0, mod, N, nQ, src, R, db, L, t0, 1);
}
__global__ __launch_bounds__(256) void k_db_store_seeded46(ChaChaKey akey, u64 nonce0, const ModC *__restrict__ mod, int N, int nQ,
                                                           const u64 *__restrict__ src, WireRows R, unsigned char *__restrict__ db,
                                                           DbLayout L, size_t t0) {
    __shared__ u64 tile[64 * 46];
    db_seeded_body<true, 16>(tile, akey, nonce0, mod, N, nQ, src, R, db, L, t0, 1);
}

}  // namespace

namespace hc {

WireRows wire_rows(const u64 *moduli, int N, int nl) {
    WireRows R{};
    if (nl < 1 || nl > HY_MAX_MODS || N < 256 || N % 256) throw std::runtime_error("hydia: wire rows: bad shape");
    for (int j = 0; j < nl; j++) R.off[j + 1] = R.off[j] + (unsigned)(N / 64) * (unsigned)(64 - __builtin_clzll(moduli[j]));
    return R;
}
// the launches take at most 65535 (item, poly) pairs each
void wire_pack(hipStream_t st, const ModC *mod, int N, const u64 *src, size_t item_stride, size_t poly_stride, size_t items, int npoly,
               int nl, const WireRows &R, u64 *dst) {
    hk::ledger_add("k_wire_pack", (double)items * npoly * ((double)nl * N * 8 + (double)R.off[nl] * 8));
    const size_t per = 65535 / (size_t)npoly;
    for (size_t i0 = 0; i0 < items; i0 += per) {
        const size_t n = items - i0 < per ? items - i0 : per;
        hipLaunchKernelGGL(k_wire_pack, dim3(N / 256, nl, (unsigned)(n * npoly)), dim3(256), 0, st, mod, N, src + i0 * item_stride, item_stride,
                           poly_stride, npoly, R, dst + i0 * npoly * R.off[nl]);
    }
}
void wire_unpack_check(hipStream_t st, const ModC *mod, int N, const u64 *src, u64 *dst, size_t item_stride, size_t poly_stride, size_t items,
                       int npoly, int nl, const WireRows &R, unsigned *flag) {
    hk::ledger_add("k_wire_unpack_check", (double)items * npoly * ((double)nl * N * 8 + (double)R.off[nl] * 8));
    const size_t per = 65535 / (size_t)npoly;
    for (size_t i0 = 0; i0 < items; i0 += per) {
        const size_t n = items - i0 < per ? items - i0 : per;
        hipLaunchKernelGGL(k_wire_unpack_check, dim3(N / 256, nl, (unsigned)(n * npoly)), dim3(256), 0, st, mod, N,
                           src + i0 * npoly * R.off[nl], R, dst + i0 * item_stride, item_stride, poly_stride, npoly, flag);
    }
}

void wire_check(hipStream_t st, const ModC *mod, int N, const u64 *src, size_t items, int npoly, int nl, const WireRows &R, unsigned *flag) {
    hk::ledger_add("k_wire_check", (double)items * npoly * (double)R.off[nl] * 8);
    const size_t per = 65535 / (size_t)npoly;
    for (size_t i0 = 0; i0 < items; i0 += per) {
        const size_t n = items - i0 < per ? items - i0 : per;
        hipLaunchKernelGGL(k_wire_check, dim3(N / 256, nl, (unsigned)(n * npoly)), dim3(256), 0, st, mod, src + i0 * npoly * R.off[nl], R, flag);
    }
}
// what both delta launchers require of a block: a ciphertext layout, at least one ciphertext and no more than the launch's grid takes
// (fits, the caller's bound), whole 512-residue tiles, and in a 46-bit layout no packed limb wider than 46 bits.  Returns whether the
// 46-bit kernels serve limbs 1 .. nQ - 1
static bool db_wire_shape(const char *who, bool fits, int N, int nQ, const WireRows &R, int X, const DbLayout &L) {
    if (L.plain || X < 1 || !fits || N < 512 || N % 512) throw std::runtime_error(std::string("hydia: ") + who + ": bad shape");
    const bool b46 = L.bits46 && L.packed;
    if (b46)
        for (int j = 1; j < nQ; j++)
            if (R.off[j + 1] - R.off[j] > (unsigned)(N / 64) * 46u)
                throw std::runtime_error(std::string("hydia: ") + who + ": a limb wider than 46 bits in a 46-bit layout");
    return b46;
}
// X <= 32767 ciphertexts of two polynomials on all nQ limbs (one block of a database: X = vector_dim)
void db_wire(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *src, const WireRows &R, void *db, size_t t0, int X, const DbLayout &L,
             bool store) {
    const bool b46 = db_wire_shape("db_wire", X <= 32767, N, nQ, R, X, L);
    // resident bytes (read and) written + the packed bytes read
    hk::ledger_add(store ? "k_db_store_wire" : "k_db_accumulate_wire", (double)X * ((store ? 1.0 : 2.0) * L.ct_bytes + 2.0 * R.off[nQ] * 8));
    const dim3 g2(N / 512, b46 ? 1 : nQ, X * 2), g16((N + 4095) / 4096, nQ - 1, X * 2);
    unsigned char *d = (unsigned char *)db;
    if (store) {
        hipLaunchKernelGGL(k_db_store_wire, g2, dim3(256), 0, st, mod, N, nQ, src, R, d, L, t0);
        if (b46 && nQ > 1) hipLaunchKernelGGL(k_db_store_wire46, g16, dim3(256), 0, st, mod, N, nQ, src, R, d, L, t0);
    } else {
        hipLaunchKernelGGL(k_db_accumulate_wire, g2, dim3(256), 0, st, mod, N, nQ, src, R, d, L, t0);
        if (b46 && nQ > 1) hipLaunchKernelGGL(k_db_accumulate_wire46, g16, dim3(256), 0, st, mod, N, nQ, src, R, d, L, t0);
    }
}

// X <= 65535 ciphertexts: c0 from the packed rows [X][R.off[nQ]] words at src, a from (akey, nonce0 + x)
void db_wire_seeded(hipStream_t st, const ChaChaKey &akey, u64 nonce0, const ModC *mod, int N, int nQ, const u64 *src, const WireRows &R, void *db,
                    size_t t0, int X, const DbLayout &L, bool store) {
    const bool b46 = db_wire_shape("db_wire_seeded", X <= 65535 && nonce0 + (u64)X < (1ull << 40), N, nQ, R, X, L);
    // resident bytes (read and) written + the packed bytes read; a costs no memory traffic
    hk::ledger_add(store ? "k_db_store_seeded" : "k_db_accumulate_seeded", (double)X * ((store ? 1.0 : 2.0) * L.ct_bytes + 1.0 * R.off[nQ] * 8));
    const dim3 g4((N + 1023) / 1024, b46 ? 1 : nQ, X), g16((N + 4095) / 4096, nQ - 1, X);
    unsigned char *d = (unsigned char *)db;
    if (store) {
        hipLaunchKernelGGL(k_db_store_seeded, g4, dim3(256), 0, st, akey, nonce0, mod, N, nQ, src, R, d, L, t0);
        if (b46 && nQ > 1) hipLaunchKernelGGL(k_db_store_seeded46, g16, dim3(256), 0, st, akey, nonce0, mod, N, nQ, src, R, d, L, t0);
    } else {
        hipLaunchKernelGGL(k_db_accumulate_seeded, g4, dim3(256), 0, st, akey, nonce0, mod, N, nQ, src, R, d, L, t0);
        if (b46 && nQ > 1) hipLaunchKernelGGL(k_db_accumulate_seeded46, g16, dim3(256), 0, st, akey, nonce0, mod, N, nQ, src, R, d, L, t0);
    }
}

}  // namespace hc
