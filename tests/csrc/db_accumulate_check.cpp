// tests/csrc/db_accumulate_check.cpp — host check of image_matching_amd/csrc/db_accum.h, the per-granule arithmetic of the in-place
// database update (k_db_accumulate / k_db_accumulate46), against plain unsigned __int128 arithmetic on bit strings:
//   - a 46-bit granule (16 residues in 23 dwords): pack / unpack round trip; adding to ONE field position r (every r = 0 .. 15) changes
//     that field to (old + add) mod q and leaves every other field, every neighbouring granule of the 736-byte unit and the bytes after
//     the unit as they were; adding to all sixteen at once; inputs all-zero, all q - 1 (the sum exceeds 2^46: a missing reduction
//     carries into the neighbour) and random
//   - a 48-bit pair (3 dwords) and an 8-byte pair (limb 0, 60 bits), same inputs, neighbours on both sides untouched
// Stand-alone: g++ -O2 -std=c++17 -I image_matching_amd/csrc tests/csrc/db_accumulate_check.cpp (also built with
// -fsanitize=address,undefined by tests/test_db_update_cpu.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "db_accum.h"

static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static int fails = 0;
#define CHECK(c, ...)                      \
    do {                                   \
        if (!(c)) {                        \
            if (fails++ < 20) {            \
                printf("FAIL %s: ", #c);   \
                printf(__VA_ARGS__);       \
                printf("\n");              \
            }                              \
        }                                  \
    } while (0)

// field of `bits` bits at bit position `pos` of a little-endian byte string, by plain 128-bit arithmetic
static u64 get_bits(const unsigned char *b, size_t pos, int bits) {
    u128 v = 0;
    for (int k = 0; k < 16; k++) v |= (u128)b[(pos >> 3) + k] << (8 * k);  // (callers keep 16 readable bytes from pos / 8)
    return (u64)((v >> (pos & 7)) & (((u128)1 << bits) - 1));
}
static void put_bits(unsigned char *b, size_t pos, int bits, u64 x) {
    for (int k = 0; k < bits; k++) {
        const size_t p = pos + k;
        b[p >> 3] = (unsigned char)((b[p >> 3] & ~(1u << (p & 7))) | (((x >> k) & 1) << (p & 7)));
    }
}
enum Fill { ZERO, SAT, RANDOM };
static u64 pick(Fill f, u64 q) { return f == ZERO ? 0 : (f == SAT ? q - 1 : rnd() % q); }

// one 736-byte unit of 8 granules + guard bytes; the granule functions see dword pointers into it
static void check_unit46(u64 q, Fill fold, Fill fadd) {
    const size_t UNIT = 736, GUARD = 32;
    std::vector<unsigned> store((UNIT + GUARD) / 4);
    unsigned char *buf = reinterpret_cast<unsigned char *>(store.data());
    u64 res[128];
    for (int c = 0; c < 128; c++) res[c] = pick(fold, q);
    // fill through the pack function, check the bit string it makes by plain arithmetic
    for (int g = 0; g < 8; g++) db_pack_granule46(res + 16 * g, store.data() + 23 * g);
    for (size_t k = 0; k < GUARD; k++) buf[UNIT + k] = (unsigned char)(0xA5 ^ k);
    for (int c = 0; c < 128; c++)
        CHECK(get_bits(buf, (size_t)(c >> 4) * 92 * 8 + (size_t)(c & 15) * 46, 46) == res[c], "pack46 q=%llu c=%d", q, c);
    for (int g = 0; g < 8; g++) {
        u64 back[16];
        db_unpack_granule46(store.data() + 23 * g, back);
        CHECK(memcmp(back, res + 16 * g, sizeof back) == 0, "unpack46 q=%llu g=%d", q, g);
    }
    // one field position at a time (granule g = r mod 8 so that every granule of the unit is hit too), then all sixteen
    for (int r = 0; r <= 16; r++) {
        const int g = r & 7;
        u64 add[16];
        for (int k = 0; k < 16; k++) add[k] = (r == 16 || k == r) ? pick(fadd, q) : 0;
        std::vector<unsigned> before(store);
        db_accumulate_granule46(store.data() + 23 * g, add, q);
        for (int c = 0; c < 128; c++) {
            const u64 old = res[c];
            if ((c >> 4) == g) res[c] = (u64)(((u128)old + add[c & 15]) % q);
            const u64 got = get_bits(buf, (size_t)(c >> 4) * 92 * 8 + (size_t)(c & 15) * 46, 46);
            CHECK(got == res[c], "acc46 q=%llu r=%d c=%d old=%llu add=%llu got=%llu want=%llu", q, r, c, old, add[c & 15], got, res[c]);
        }
        for (size_t w = 0; w < store.size(); w++)
            if (w < (size_t)23 * g || w >= (size_t)23 * (g + 1)) CHECK(store[w] == before[w], "acc46 touched dword %zu outside granule %d", w, g);
    }
    for (size_t k = 0; k < GUARD; k++) CHECK(buf[UNIT + k] == (unsigned char)(0xA5 ^ k), "acc46 wrote past the unit (+%zu)", k);
}

// five pairs side by side; the middle one is updated
static void check_pairs(u64 q, bool pk, Fill fold, Fill fadd) {
    const size_t es = pk ? 6 : 8, GUARD = 16;
    std::vector<u64> store((10 * es + GUARD + 7) / 8 + 2);
    unsigned char *buf = reinterpret_cast<unsigned char *>(store.data());
    u64 res[10];
    for (int c = 0; c < 10; c++) {
        res[c] = pick(fold, q);
        put_bits(buf, c * es * 8, (int)es * 8, res[c]);
    }
    if (pk) {
        unsigned w[3];
        u64 x, y;
        db_pack_pair48(res[0], res[1], w);
        CHECK(memcmp(w, buf, 12) == 0, "pack48 q=%llu", q);
        db_unpack_pair48(reinterpret_cast<unsigned *>(buf) + 3, x, y);
        CHECK(x == res[2] && y == res[3], "unpack48 q=%llu", q);
    }
    for (int pair = 0; pair < 5; pair++) {
        const u64 ax = pick(fadd, q), ay = pick(fadd, q);
        std::vector<u64> before(store);
        db_accumulate_pair(buf + pair * 2 * es, pk, ax, ay, q);
        res[2 * pair] = (u64)(((u128)res[2 * pair] + ax) % q);
        res[2 * pair + 1] = (u64)(((u128)res[2 * pair + 1] + ay) % q);
        for (int c = 0; c < 10; c++) CHECK(get_bits(buf, c * es * 8, (int)es * 8) == res[c], "pair q=%llu pk=%d pair=%d c=%d", q, (int)pk, pair, c);
        const unsigned char *b0 = reinterpret_cast<const unsigned char *>(before.data());
        for (size_t k = 0; k < store.size() * 8; k++)
            if (k < pair * 2 * es || k >= (pair + 1) * 2 * es) CHECK(buf[k] == b0[k], "pair pk=%d touched byte %zu outside pair %d", (int)pk, k, pair);
    }
}

int main() {
    // 46-bit limbs: primes of the default chain's shape (just above / below 2^45), the largest value below 2^46, the smallest above 2^45
    const u64 q46[] = {35184372121601ull, 35184371892225ull, (1ull << 46) - 1, (1ull << 45) + 1, 35184372744193ull};
    // 48-bit residues: the same and values up to 2^48 - 1; 8-byte residues: 60-bit moduli (limb 0) and a 45-bit one (unpacked databases)
    const u64 q48[] = {35184372121601ull, (1ull << 48) - 1, (1ull << 47) + 5, (1ull << 45) + 1};
    const u64 q64[] = {1152921504606584833ull, (1ull << 60) - 1, (1ull << 59) + 1, 35184372121601ull, (1ull << 62) - 57};
    const Fill fills[] = {ZERO, SAT, RANDOM};
    for (u64 q : q46)
        for (Fill a : fills)
            for (Fill b : fills)
                for (int rep = 0; rep < (a == RANDOM || b == RANDOM ? 50 : 1); rep++) check_unit46(q, a, b);
    for (Fill a : fills)
        for (Fill b : fills)
            for (int rep = 0; rep < (a == RANDOM || b == RANDOM ? 200 : 1); rep++) {
                for (u64 q : q48) check_pairs(q, true, a, b);
                for (u64 q : q64) check_pairs(q, false, a, b);
            }
    if (fails) {
        printf("db accumulate: %d failures\n", fails);
        return 1;
    }
    printf("db accumulate ok\n");
    return 0;
}
