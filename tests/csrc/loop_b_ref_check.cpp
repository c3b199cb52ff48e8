// tests/csrc/loop_b_ref_check.cpp — tests/csrc/loop_b_ref.h checked on the CPU (tests/test_loop_b_model_cpu.py compiles it with g++,
// plain and with the host sanitizers).  It pins the residue patterns, the recomputation and the slot map that tests/csrc/loop_b_check.cpp
// holds the loop-B kernels against, and the range premises that decide what that comparison can and cannot see — in exact integers
// wider than the sums they are about.
// Usage: loop_b_ref_check <name>:<logN>:<q_0,q_1,...,q_{nl-1}> ...   (the ciphertext limbs of each chain; "default*" names take the
//        premises of the 60-bit first limb)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "loop_b_ref.h"
using namespace loop_b_ref;

static int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            failures++;                  \
            printf("FAILED: " __VA_ARGS__); \
            printf("\n");                \
        }                                \
    } while (0)

// 192-bit unsigned sum of 128-bit terms: wide enough for every sum below (at most 2^13 terms below 2^128)
struct U192 {
    u128 lo = 0;
    u64 hi = 0;
    void add(u128 x) {
        lo += x;
        if (lo < x) hi++;
    }
    bool below_2p128() const { return hi == 0; }
};
static int bit_length(u128 v) {
    int n = 0;
    while (v) {
        n++;
        v >>= 1;
    }
    return n;
}

struct Chain {
    std::string name;
    int logN;
    std::vector<u64> q;
};

// sat on both sides: every residue is -1, every product 1: d0 = d2 = dim, d1 = 2 dim (mod q)
static void closed_forms(const Chain &ch) {
    const int dims[2] = {64, 512};
    for (int dim : dims)
        for (size_t j = 0; j < ch.q.size(); j++) {
            const u64 q = ch.q[j];
            const int nl = (int)ch.q.size(), N = 1 << ch.logN;
            auto rot = [&](int, int i, int p) { return residue(SAT, 11, operand_index(i, p, (int)j, 5, nl, N), q); };
            auto db = [&](int g, int i, int p) { return residue(SAT, 1200 + g, operand_index(i, p, (int)j, 5, nl, N), q); };
            const Triple t = triple(0, 3, dim, q, rot, db);
            CHECK(t.d0 == (u64)dim % q && t.d2 == (u64)dim % q && t.d1 == (u64)(2 * dim) % q, "closed form, chain %s limb %zu dim %d: %llu %llu %llu",
                  ch.name.c_str(), j, dim, t.d0, t.d1, t.d2);
            // the two branches of the recomputation (one-by-one and lazy) agree where both are in range: a 2-diagonal sum
            auto ru = [&](int, int i, int p) { return residue(HOLES, 7, operand_index(i, p, (int)j, 9, nl, N), q); };
            auto du = [&](int, int i, int p) { return residue(UNIFORM, 8, operand_index(i, p, (int)j, 9, nl, N), q); };
            const Triple w = triple(0, 0, 2, q, ru, du);
            u64 e0 = 0, e1 = 0, e2 = 0;
            for (int i = 0; i < 2; i++) {
                const u64 a0 = ru(0, i, 0), a1 = ru(0, i, 1), b0 = du(0, i, 0), b1 = du(0, i, 1);
                e0 = (u64)((e0 + (u128)a0 * b0 % q) % q);
                e1 = (u64)((e1 + (u128)a0 * b1 % q + (u128)a1 * b0 % q) % q);
                e2 = (u64)((e2 + (u128)a1 * b1 % q) % q);
            }
            CHECK(w.d0 == e0 && w.d1 == e1 && w.d2 == e2, "recomputation branches, chain %s limb %zu", ch.name.c_str(), j);
        }
}

static void patterns(const Chain &ch) {
    for (size_t j = 0; j < ch.q.size(); j++) {
        const u64 q = ch.q[j];
        for (size_t k = 0; k < 300; k++) {  // uniform IS the device fill's hash, restated here independently
            const size_t idx = k * 7919 + j;
            u64 z = 1200 + idx * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            CHECK(residue(UNIFORM, 1200, idx, q) == z % q && hash_residue(1200, idx, q) == z % q, "uniform differs from the fill hash at %zu", idx);
        }
        const size_t n = 1 << 16;
        size_t holes = 0, seen[4] = {0, 0, 0, 0}, hole_special = 0, hole_other = 0;
        for (size_t idx = 0; idx < n; idx++) {
            const u64 h = residue(HOLES, 21 + j, idx, q), e = residue(EDGE, 21 + j, idx, q);
            CHECK(h < q && e < q && residue(SAT, 0, idx, q) == q - 1, "residue out of range at %zu", idx);
            if (h != q - 1) {
                holes++;
                if (h == 0 || h == 1 || h == q - 2 || h == q / 2) hole_special++;
                else hole_other++;
            }
            if (e == 0) seen[0]++;
            else if (e == 1) seen[1]++;
            else if (e == q - 2) seen[2]++;
            else if (e == q - 1) seen[3]++;
            else CHECK(false, "edge residue %llu outside its set", e);
        }
        CHECK(holes * 32 > n && holes * 8 < n, "holes: %zu of %zu positions differ from q - 1 (wanted between 1/32 and 1/8)", holes, n);
        CHECK(hole_special > 0 && hole_other > 0, "holes: special %zu, hashed %zu", hole_special, hole_other);
        for (int k = 0; k < 4; k++) CHECK(seen[k] * 8 > n, "edge: value %d drawn %zu times of %zu", k, seen[k], n);
        // two queries (or blocks) with different seeds never share a holes / uniform / edge operand
        size_t same = 0;
        for (size_t idx = 0; idx < 4096; idx++) same += residue(HOLES, 11, idx, q) == residue(HOLES, 111, idx, q);
        CHECK(same < 4096, "holes does not depend on the seed");
    }
}

// Sums128 on a 60-bit limb, in exact integers.  The kernel folds a sum of Karatsuba products (a0 + a1)(b0 + b1) <= (2q - 2)^2 every
// chunk = 2^(125 - 2k) = 32 diagonals (k = 60); a folded sum is below q.
static void sums128_premises(const Chain &ch) {
    const u64 q = ch.q[0];
    if (bit_length(q) != 60) {
        CHECK(false, "chain %s: q_0 has %d bits, the premises are about a 60-bit limb", ch.name.c_str(), bit_length(q));
        return;
    }
    const u128 sat = (u128)(2 * q - 2) * (2 * q - 2);
    auto fits = [&](int n) {
        U192 s;
        s.add(q - 1);  // what a fold leaves
        for (int i = 0; i < n; i++) s.add(sat);
        return s.below_2p128();
    };
    // what the code does (32) is in range.  So is twice that: 64 (2q - 2)^2 + q < 256 q^2 < 2^128 for every q < 2^60 — the interval
    // the comments used to quote would not have wrapped, the code is conservative by one bit.  From 65 saturated products on (and so
    // at 128, the next power of two) the sum wraps.
    CHECK(fits(32), "32 saturated Karatsuba products + q do not fit 128 bits");
    CHECK(fits(64), "64 saturated Karatsuba products + q do not fit 128 bits");
    CHECK(!fits(65), "65 saturated Karatsuba products + q fit 128 bits");
    CHECK(!fits(128), "128 saturated Karatsuba products + q fit 128 bits");
    // uniform residues of the existing test's own seeds (rotations 11, blocks 1200 + g): every aligned run of 128 diagonals — and
    // every stride-4 run of a split-diagonal wave — stays below 2^128, so a fold interval FOUR times too long passes
    // the uniform comparison; only residues near q - 1 separate 32 or 64 from 128.
    const int N = 1 << ch.logN, nl = (int)ch.q.size(), dim = 512, step = N > 4096 ? 16 : 1;
    int worst = 0;
    for (int g = 0; g < 2; g++)
        for (int c = 0; c < N; c += step) {
            U192 run[4], strided4[4];
            for (int i = 0; i < dim; i++) {
                const u64 a0 = hash_residue(11, operand_index(i, 0, 0, c, nl, N), q), a1 = hash_residue(11, operand_index(i, 1, 0, c, nl, N), q);
                const u64 b0 = hash_residue(1200 + g, operand_index(i, 0, 0, c, nl, N), q), b1 = hash_residue(1200 + g, operand_index(i, 1, 0, c, nl, N), q);
                const u128 k = (u128)(a0 + a1) * (b0 + b1);
                run[i / 128].add(k);
                strided4[i % 4].add(k);  // k_hydia_tensor_sk<4, .>: 128 diagonals per wave at dim 512
            }
            for (int r = 0; r < 4; r++) {
                run[r].add(q - 1);
                strided4[r].add(q - 1);
                CHECK(run[r].below_2p128() && strided4[r].below_2p128(), "a uniform run of 128 diagonals wraps at block %d coefficient %d", g, c);
                if (bit_length(run[r].lo) > worst) worst = bit_length(run[r].lo);
                if (bit_length(strided4[r].lo) > worst) worst = bit_length(strided4[r].lo);
            }
        }
    printf("chain %s: 128 uniform Karatsuba products + q on q_0 = %llu take at most %d bits\n", ch.name.c_str(), q, worst);
}

// Halves24: operands cut at 24 bits, a = ah 2^24 + al; per coefficient three 64-bit sums ll = sum al bl, mid = sum (al bh + ah bl),
// hh = sum ah bh over the diagonals, never folded.  The largest are the Karatsuba term's, whose operands are sums of two residues'
// halves: low halves up to 2 (2^24 - 1), high halves up to 2 (2^hb - 1) with hb = 24 (48-bit residues) or 22 (46-bit ones).
static void halves24_premises() {
    const int hbs[2] = {24, 22};
    for (int hb : hbs) {
        const u128 lo = 2 * ((1ull << 24) - 1), hi = 2 * ((1ull << hb) - 1);
        auto sums = [&](int dim, u128 *ll, u128 *mid, u128 *hh) {
            *ll = *mid = *hh = 0;
            for (int i = 0; i < dim; i++) {
                *ll += lo * lo;
                *mid += lo * hi;
                *mid += hi * lo;
                *hh += hi * hi;
            }
        };
        const u128 lim = (u128)1 << 63;
        u128 ll, mid, hh;
        sums(512, &ll, &mid, &hh);
        CHECK(ll < lim && mid < lim && hh < lim, "Halves24 24+%d at dim 512 passes 2^63", hb);
        printf("Halves24 24+%d bits at dim 512: ll %d bits, mid %d bits, hh %d bits (of 63)\n", hb, bit_length(ll), bit_length(mid), bit_length(hh));
        if (hb == 24) CHECK(bit_length(mid) == 60, "Halves24 24+24 at dim 512: mid takes %d bits, expected 60 (three bits of margin)", bit_length(mid));
        sums(4096, &ll, &mid, &hh);
        CHECK(ll < lim && mid < lim && hh < lim, "Halves24 24+%d at dim 4096 passes 2^63", hb);
        printf("Halves24 24+%d bits at dim 4096: ll %d bits, mid %d bits, hh %d bits (of 63)\n", hb, bit_length(ll), bit_length(mid), bit_length(hh));
        if (hb == 24) {
            CHECK(bit_length(mid) == 63, "Halves24 24+24 at dim 4096: mid takes %d bits, expected all 63", bit_length(mid));
            sums(4097, &ll, &mid, &hh);  // the launcher's limit is the arithmetic's: one more diagonal of all-ones halves passes 2^63
            CHECK(mid >= lim, "Halves24 24+24: 4097 diagonals stay below 2^63");
        }
    }
}

static void slots() {
    const int shapes[][3] = {{1, 1, 0}, {1, 2, 0}, {1, 16, 0}, {2, 2, 0}, {3, 2, 0}, {2, 8, 0}, {3, 8, 0}, {2, 16, 0}, {3, 16, 0},
                             {1, 16, 2}, {3, 16, 2}, {1, 16, 4}, {3, 16, 4}};
    for (auto &s : shapes) {
        const int Q = s[0], G = s[1], ng = s[2];
        std::vector<int> hit((size_t)Q * G, 0);
        for (int q = 0; q < Q; q++)
            for (int gi = 0; gi < G; gi++) {
                const size_t t = slot(q, gi, Q, G, ng);
                CHECK(t < hit.size(), "slot (%d, %d) of Q %d G %d ng %d = %zu is out of range", q, gi, Q, G, ng, t);
                if (t < hit.size()) hit[t]++;
                // giant-major: all of one giant step's slots are one contiguous run of Q (G / ng), query-major inside
                if (ng > 0) CHECK(t / ((size_t)Q * (G / ng)) == (size_t)(gi % ng) && (t / (G / ng)) % Q == (size_t)q && t % (G / ng) == (size_t)(gi / ng), "slot (%d, %d) is not giant-major", q, gi);
            }
        for (size_t t = 0; t < hit.size(); t++) CHECK(hit[t] == 1, "slot %zu of Q %d G %d ng %d is hit %d times", t, Q, G, ng, hit[t]);
    }
}

int main(int argc, char **argv) {
    std::vector<Chain> chains;
    for (int a = 1; a < argc; a++) {
        std::string s = argv[a];
        const size_t c1 = s.find(':'), c2 = s.find(':', c1 + 1);
        if (c1 == std::string::npos || c2 == std::string::npos) {
            printf("bad chain argument %s\n", argv[a]);
            return 2;
        }
        Chain ch;
        ch.name = s.substr(0, c1);
        ch.logN = atoi(s.substr(c1 + 1, c2 - c1 - 1).c_str());
        const char *p = s.c_str() + c2 + 1;
        while (*p) {
            char *end;
            ch.q.push_back(strtoull(p, &end, 10));
            p = *end ? end + 1 : end;
        }
        if (ch.q.empty() || ch.logN < 7 || ch.logN > 16) {
            printf("bad chain argument %s\n", argv[a]);
            return 2;
        }
        chains.push_back(ch);
    }
    if (chains.empty()) {
        printf("usage: loop_b_ref_check <name>:<logN>:<q_0,q_1,...> ...\n");
        return 2;
    }
    for (const Chain &ch : chains) {
        closed_forms(ch);
        patterns(ch);
        if (ch.name.compare(0, 7, "default") == 0) sums128_premises(ch);
    }
    halves24_premises();
    slots();
    if (failures) {
        printf("loop B reference: %d checks FAILED\n", failures);
        return 1;
    }
    printf("loop B reference ok (%zu chains)\n", chains.size());
    return 0;
}
