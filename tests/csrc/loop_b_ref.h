// tests/csrc/loop_b_ref.h — the host side of the loop-B checks, with no HIP in it: the residue patterns the operands are filled with,
// the recomputation of one accumulator triple with unsigned __int128, and the output-slot map documented in kernels.h.  Shared by
// tests/csrc/loop_b_check.cpp (which runs the kernels) and tests/csrc/loop_b_ref_check.cpp (which checks THIS file on the CPU, also
// under the host sanitizers).  Test infrastructure, never part of the product.
#pragma once
#include <cstddef>
#include <cstring>

namespace loop_b_ref {
typedef unsigned long long u64;
typedef unsigned __int128 u128;

// The counter hash of k_fill_uniform_hash (kernels.hip) before its reduction.
inline u64 mix(u64 seed, size_t idx) {
    u64 z = seed + (u64)idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
inline u64 hash_residue(u64 seed, size_t idx, u64 q) { return mix(seed, idx) % q; }  // k_fill_uniform_hash on the host

// uniform: hash_residue.  sat: q - 1 everywhere (every lazy sum at its bound).  holes: q - 1 except at about one index in 16, picked by
// a hash of (seed, idx); there a hashed residue or one of 0, 1, q - 2, floor(q / 2) — the sums stay at the bound and every (block,
// diagonal, polynomial, limb, coefficient) still decides the result.  edge: every residue drawn from {0, 1, q - 2, q - 1}.
enum Pattern { UNIFORM = 0, SAT = 1, HOLES = 2, EDGE = 3 };
inline const char *pattern_name(Pattern p) {
    static const char *const n[] = {"uniform", "sat", "holes", "edge"};
    return n[p];
}
inline bool parse_pattern(const char *s, size_t len, Pattern *out) {
    for (int p = 0; p < 4; p++)
        if (strlen(pattern_name((Pattern)p)) == len && !strncmp(s, pattern_name((Pattern)p), len)) {
            *out = (Pattern)p;
            return true;
        }
    return false;
}
inline u64 residue(Pattern p, u64 seed, size_t idx, u64 q) {
    switch (p) {
    case UNIFORM: return hash_residue(seed, idx, q);
    case SAT: return q - 1;
    case HOLES: {
        const u64 h = mix(seed ^ 0x5851F42D4C957F2Dull, idx);  // its own stream: independent of the uniform fill of the same seed
        if (h & 15) return q - 1;
        switch ((h >> 4) & 7) {
        case 4: return 0;
        case 5: return 1;
        case 6: return q - 2;
        case 7: return q / 2;
        default: return mix(h, idx) % q;
        }
    }
    default: {
        const u64 h = mix(seed ^ 0xD1342543DE82EF95ull, idx);
        const u64 v[4] = {0, 1, q - 2, q - 1};
        return v[h >> 62];
    }
    }
}

// index of (diagonal i, polynomial p, limb j, coefficient c) inside one rotation set or one database block: [i][p][j][c]
inline size_t operand_index(int i, int p, int j, int c, int nl, int N) { return (((size_t)i * 2 + p) * nl + j) * N + c; }

// One accumulator triple of loop B: d0 = sum a0 b0, d1 = sum (a0 b1 + a1 b0), d2 = sum a1 b1 over the dim diagonals, modulo q.
// rot(query, i, p) and db(block, i, p) give the two operands' residues (of the limb and coefficient the caller has fixed).  Products
// are reduced one by one when q >= 2^50 (a lazy 128-bit sum of 2 dim of them would pass 2^128), summed lazily otherwise
// (2 * 4096 * 2^100 < 2^128).
struct Triple {
    u64 d0, d1, d2;
};
template <class Rot, class Db>
inline Triple triple(int query, int block, int dim, u64 q, Rot rot, Db db) {
    const bool wide = (q >> 50) != 0;
    u128 d0 = 0, d1 = 0, d2 = 0;
    for (int i = 0; i < dim; i++) {
        const u64 a0 = rot(query, i, 0), a1 = rot(query, i, 1), b0 = db(block, i, 0), b1 = db(block, i, 1);
        if (wide) {
            d0 += (u128)a0 * b0 % q;
            d1 += (u128)a0 * b1 % q + (u128)a1 * b0 % q;
            d2 += (u128)a1 * b1 % q;
        } else {
            d0 += (u128)a0 * b0;
            d1 += (u128)a0 * b1 + (u128)a1 * b0;
            d2 += (u128)a1 * b1;
        }
    }
    return {(u64)(d0 % q), (u64)(d1 % q), (u64)(d2 % q)};
}

// Output slot of (query q of Q, block gi of G) — kernels.h: q G + gi; with ng > 0 giant steps the G blocks are (database block, giant)
// pairs and the slots are giant-major over the whole batch, ((gi % ng) Q + q) (G / ng) + gi / ng.
inline size_t slot(int q, int gi, int Q, int G, int ng) {
    return ng > 0 ? ((size_t)(gi % ng) * Q + q) * (size_t)(G / ng) + gi / ng : (size_t)q * G + gi;
}
}  // namespace loop_b_ref
