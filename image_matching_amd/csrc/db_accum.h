// image_matching_amd/csrc/db_accum.h — the per-granule arithmetic of an in-place database update: unpack the resident residues, add
// the fresh ones mod q, pack them back (shared by k_db_accumulate / k_db_accumulate46 and, on the host, by
// tests/csrc/db_accumulate_check.cpp, which checks them against plain unsigned __int128 arithmetic).
//
// The granules are the ones k_db_repack / k_db_repack46 move, so that one thread owns every dword it reads and writes:
//   a residue PAIR:   16 bytes (8-byte residues: limb 0, or every limb of an unpacked database) or 12 bytes = 3 dwords (48-bit residues)
//   SIXTEEN residues: 92 bytes = 23 dwords (the 46-bit residues of a bits46 layout; the granule starts and ends on a dword)
// Both operands are reduced (< q), and q > 2^45 for a 46-bit limb: the sum can exceed 2^46 and is reduced BEFORE it is packed — an
// unreduced sum would carry into the neighbouring field.
#pragma once
#include "devmath.h"

#if defined(__clang__)
#define HY_UNROLL _Pragma("unroll")  // the dword and field indices must be compile-time constants on the device (registers, no scratch)
#else
#define HY_UNROLL
#endif

HD void db_unpack_pair48(const unsigned w[3], u64 &x, u64 &y) {
    x = (u64)w[0] | ((u64)(w[1] & 0xFFFFu) << 32);
    y = (u64)(w[1] >> 16) | ((u64)w[2] << 16);
}
HD void db_pack_pair48(u64 x, u64 y, unsigned w[3]) {
    w[0] = (unsigned)x;
    w[1] = ((unsigned)(x >> 32) & 0xFFFFu) | ((unsigned)y << 16);
    w[2] = (unsigned)(y >> 16);
}
// the pair at d (12 bytes when pk, else 16; 4- resp. 8-byte aligned) += (ax, ay) mod q
HD void db_accumulate_pair(unsigned char *d, bool pk, u64 ax, u64 ay, u64 q) {
    if (pk) {
        unsigned *p = reinterpret_cast<unsigned *>(d);
        unsigned w[3] = {p[0], p[1], p[2]};
        u64 x, y;
        db_unpack_pair48(w, x, y);
        db_pack_pair48(addmod(x, ax, q), addmod(y, ay, q), w);
        p[0] = w[0];
        p[1] = w[1];
        p[2] = w[2];
    } else {
        u64 *p = reinterpret_cast<u64 *>(d);
        p[0] = addmod(p[0], ax, q);
        p[1] = addmod(p[1], ay, q);
    }
}

// field r of a 46-bit granule starts at bit 46 r: dword (46 r) >> 5, shift (46 r) & 31; it reaches a third dword when 46 + shift > 64
HD void db_unpack_granule46(const unsigned w[23], u64 v[16]) {
    HY_UNROLL
    for (int r = 0; r < 16; r++) {
        const int bit = 46 * r, di = bit >> 5, sh = bit & 31;
        u64 x = ((u64)w[di] >> sh) | ((u64)w[di + 1] << (32 - sh));
        if (sh > 18) x |= (u64)w[di + 2] << (64 - sh);
        v[r] = x & ((1ull << 46) - 1);
    }
}
HD void db_pack_granule46(const u64 v[16], unsigned w[23]) {
    HY_UNROLL
    for (int k = 0; k < 23; k++) w[k] = 0;
    HY_UNROLL
    for (int r = 0; r < 16; r++) {
        const u64 x = v[r] & ((1ull << 46) - 1);
        const int bit = 46 * r, di = bit >> 5, sh = bit & 31;
        w[di] |= (unsigned)(x << sh);
        w[di + 1] |= (unsigned)(sh ? x >> (32 - sh) : x >> 32);
        if (sh > 18) w[di + 2] |= (unsigned)(x >> (64 - sh));
    }
}
// the sixteen residues in the 23 dwords at d += add[0..15] mod q
HD void db_accumulate_granule46(unsigned *d, const u64 add[16], u64 q) {
    unsigned w[23];
    u64 v[16];
    HY_UNROLL
    for (int k = 0; k < 23; k++) w[k] = d[k];
    db_unpack_granule46(w, v);
    HY_UNROLL
    for (int r = 0; r < 16; r++) v[r] = addmod(v[r], add[r], q);
    db_pack_granule46(v, w);
    HY_UNROLL
    for (int k = 0; k < 23; k++) d[k] = w[k];
}
