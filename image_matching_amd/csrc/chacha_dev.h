// image_matching_amd/csrc/chacha_dev.h — the ChaCha20 block of the deterministic sampler specification (DESIGN.md §"Randomness") and the
// uniform residues drawn from it, as device functions: ONE text for every kernel that samples (client_kernels.hip: k_sample_uniform,
// k_sample_small, k_enc_sym) or regenerates a seeded half where it is consumed (wire_kernels.hip: k_db_accumulate_seeded /
// k_db_store_seeded), so the bits cannot diverge.
#pragma once
#include "devmath.h"

struct ChaChaKey {
    unsigned k[8];
};

#if defined(__HIPCC__)
DEV unsigned rotl32(unsigned v, int n) { return (v << n) | (v >> (32 - n)); }
#define CHACHA_QR(a, b, c, d) \
    a += b; d ^= a; d = rotl32(d, 16); \
    c += d; b ^= c; b = rotl32(b, 12); \
    a += b; d ^= a; d = rotl32(d, 8);  \
    c += d; b ^= c; b = rotl32(b, 7);

// ChaCha20 block with a 64-bit block counter (words 12,13) and a 64-bit stream id (words 14,15)
DEV void chacha_block(const ChaChaKey &key, u64 stream, u64 block, unsigned out[16]) {
    unsigned s[16], x[16];
    s[0] = 0x61707865u; s[1] = 0x3320646eu; s[2] = 0x79622d32u; s[3] = 0x6b206574u;
#pragma unroll
    for (int i = 0; i < 8; i++) s[4 + i] = key.k[i];
    s[12] = (unsigned)block; s[13] = (unsigned)(block >> 32);
    s[14] = (unsigned)stream; s[15] = (unsigned)(stream >> 32);
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        CHACHA_QR(x[0], x[4], x[8], x[12]) CHACHA_QR(x[1], x[5], x[9], x[13]) CHACHA_QR(x[2], x[6], x[10], x[14]) CHACHA_QR(x[3], x[7], x[11], x[15])
        CHACHA_QR(x[0], x[5], x[10], x[15]) CHACHA_QR(x[1], x[6], x[11], x[12]) CHACHA_QR(x[2], x[7], x[8], x[13]) CHACHA_QR(x[3], x[4], x[9], x[14])
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}
// uniform residues: block `block` of `stream` = coefficients 4 block .. 4 block + 3 (128 random bits each, reduced mod q)
DEV void chacha_uniform4(const ChaChaKey &key, u64 stream, u64 block, const ModC &M, u64 a[4]) {
    unsigned w[16];
    chacha_block(key, stream, block, w);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const u64 lo = (u64)w[4 * t] | ((u64)w[4 * t + 1] << 32);
        const u64 hi = (u64)w[4 * t + 2] | ((u64)w[4 * t + 3] << 32);
        a[t] = reduce128(((u128)hi << 64) | lo, M);
    }
}
#endif
