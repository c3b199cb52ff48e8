// tests/csrc/loop_b_check.cpp — loop B exactly as a query runs it (Context::similarity_accumulate_rot: the production layout choice,
// kernel choice and launch shape) against a host recomputation with unsigned __int128, on pseudo-random residues at the FULL ring.
// Test infrastructure (tests/test_gpu_full_ring.py builds and runs it; never part of the product).  Why it exists: ROCm 7.2 once
// miscompiled the 24-bit-halves kernel (k_hydia_tensor24) — it dropped the operand masks and fused unmasked registers back into
// v_mad_u64_u32 — and only a host recomputation shows that; a compiler bump could bring it back at dim 512.  What it replaces:
// 512 x EvalMultNoRelin + 511 x EvalAddInPlace per block, /root/reference/src/sender/sender_diag.cpp:70-77,:93.
// Usage: loop_b_check <blocks> <dim> <logN> <0 = ciphertext-major | 1 = the layout the context picks (group-sequential above 8 blocks,
//        46-bit residues) | 2 = group-sequential with 48-bit residues>
//
// With any of the flags below (tests/test_gpu_loop_b_edges.py) both operands are built on the HOST from the patterns of loop_b_ref.h —
// saturated residues reach the lazy sums' bounds, which uniform ones miss by two bits — and every (query, block) slot is compared:
//   --patterns a/b,...   rotation / database pattern pairs (uniform, sat, holes, edge), one result line per pair, prefixed with the pair
//   --moduli q0,q1,... --np n   a caller's chain: the ciphertext primes, then n special primes (roots left to the context)
//   --queries Q          Q > 1: hk::hydia_tensor_accumulate as a batch (bpp = TENSOR_BATCH), query q with its own seed and the pattern
//                        (given, holes, uniform)[q % 3]
//   --giants NG          ng = NG: the blocks are (database block, giant step) pairs, the slots giant-major
// and the loop-B launches the byte ledger recorded are printed ("ledger <pair>: <kernel> x<launches>").  Exit status 1 on any mismatch.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hydia_core.h"
#include "loop_b_ref.h"
using namespace hydia;
namespace ref = loop_b_ref;

static const u64 seed_rot = 11, seed_db = 1200;

// every (query, block, limb) of `ha` [slot][{d0, d1, d2}][limb][coefficient] against ref::triple, on T threads; returns the mismatches
template <class Rot, class Db>
static long compare(const Context &cx, const std::vector<u64> &ha, int Q, int G, int ng, int dim, unsigned T, Rot rot, Db db) {
    const int N = cx.N, nl = cx.nQ;
    std::atomic<long> bad{0};
    std::atomic<int> next{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; t++)
        th.emplace_back([&] {
            for (;;) {
                const int w = next.fetch_add(1);  // one (query, block, limb) at a time
                if (w >= Q * G * nl) break;
                const int qi = w / (G * nl), g = w / nl % G, j = w % nl;
                const u64 q = cx.q[j];
                const size_t s = ref::slot(qi, g, Q, G, ng);
                for (int c = 0; c < N; c++) {
                    const ref::Triple want = ref::triple(qi, g, dim, q, [&](int x, int i, int p) { return rot(x, i, p, j, c); },
                                                         [&](int x, int i, int p) { return db(x, i, p, j, c); });
                    const u64 g0 = ha[(s * 3 + 0) * nl * N + (size_t)j * N + c], g1 = ha[(s * 3 + 1) * nl * N + (size_t)j * N + c],
                              g2 = ha[(s * 3 + 2) * nl * N + (size_t)j * N + c];
                    if (g0 != want.d0 || g1 != want.d1 || g2 != want.d2) {
                        if (bad.fetch_add(1) < 6) {
                            if (Q > 1) printf("query %d ", qi);
                            printf("mismatch block %d limb %d coefficient %d: got %llu %llu %llu want %llu %llu %llu\n", g, j, c, (unsigned long long)g0,
                                   (unsigned long long)g1, (unsigned long long)g2, (unsigned long long)want.d0, (unsigned long long)want.d1,
                                   (unsigned long long)want.d2);
                        }
                    }
                }
            }
        });
    for (auto &x : th) x.join();
    return bad.load();
}

// the four-argument call: device-filled uniform residues, one query, the context's own chain
static int uniform_main(int G, int dim, int logN, int mode) {
    const bool pick = mode != 0;
    Params p;
    p.logN = logN;
    p.dim = dim;
    Context cx(p, 0);
    const int N = cx.N, nl = cx.nQ;
    if (!pick) cx.db_seq_ok = false;
    if (mode == 2) cx.db_bits46_ok = false;
    const size_t cts = (size_t)G * dim, e = (size_t)2 * nl * N;
    if ((size_t)dim * 2 * nl > 32768 - 32768 % (size_t)nl) {
        printf("block too large for one fill launch\n");
        return 2;
    }
    cx.db_resize((size_t)G * cx.slots, cts, dim);
    cx.db_kind = 5;
    cx.db_babies = dim;
    printf("N = 2^%d, dim %d, %d blocks: %s layout (groups of %d blocks, %d-bit packed residues), %.2f GiB resident\n", logN, dim, G,
           cx.db_lay.seq ? "group-sequential" : "ciphertext-major", cx.db_lay.seq, cx.db_lay.bits46 ? 46 : 48, (double)cts * cx.db_lay.ct_bytes / (1 << 30));
    Ct rot(&cx, dim, 2, nl, cx.delta);
    hk::fill_uniform_hash(cx.stream, cx.d_mod, N, rot.d, (size_t)dim * 2 * nl, nl, seed_rot);
    u64 *tmp = cx.pool.get((size_t)dim * e * sizeof(u64));
    std::vector<u64> probe(4096);
    for (int g = 0; g < G; g++) {
        hk::fill_uniform_hash(cx.stream, cx.d_mod, N, tmp, (size_t)dim * 2 * nl, nl, seed_db + g);
        cx.db_store((size_t)g * dim, tmp, dim);
        if (g == G - 1) {  // the host mirror of the fill must be the device's: a stretch of the last block's last ciphertext, limb nl - 1
            cx.sync();
            const size_t off = (size_t)dim * e - probe.size();
            HIP_CHECK(hipMemcpy(probe.data(), tmp + off, probe.size() * 8, hipMemcpyDeviceToHost));
            for (size_t k = 0; k < probe.size(); k++)
                if (probe[k] != ref::hash_residue(seed_db + g, off + k, cx.q[nl - 1])) {
                    printf("host mirror of the fill differs from the device at %zu\n", k);
                    return 2;
                }
        }
    }
    cx.sync();
    cx.pool.put(tmp);
    Ct acc = cx.similarity_accumulate_rot(rot);
    cx.sync();
    std::vector<u64> ha((size_t)G * 3 * nl * N);
    HIP_CHECK(hipMemcpy(ha.data(), acc.d, ha.size() * 8, hipMemcpyDeviceToHost));
    // rotated queries on the host, once: [i][poly][limb][c]
    std::vector<u64> hr((size_t)dim * e);
    const unsigned T = std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < T; t++)
            th.emplace_back([&, t] {
                for (size_t lp = t; lp < (size_t)dim * 2 * nl; lp += T)
                    for (int c = 0; c < N; c++) hr[lp * N + c] = ref::hash_residue(seed_rot, lp * N + c, cx.q[lp % nl]);
            });
        for (auto &x : th) x.join();
    }
    const long bad = compare(
        cx, ha, 1, G, 0, dim, T, [&](int, int i, int pl, int j, int c) { return hr[ref::operand_index(i, pl, j, c, nl, N)]; },
        [&](int g, int i, int pl, int j, int c) { return ref::hash_residue(seed_db + g, ref::operand_index(i, pl, j, c, nl, N), cx.q[j]); });
    printf("loop B, %d blocks x %d diagonals at N = 2^%d: %ld mismatches of %ld (block, limb, coefficient) triples\n", G, dim, logN, bad,
           (long)G * nl * N);
    return bad != 0;
}

struct Options {
    std::vector<u64> moduli;
    int np = 0, Q = 1, ng = 0;
    std::vector<std::pair<ref::Pattern, ref::Pattern>> pairs;
};

static bool parse_pairs(const char *s, Options &o) {
    while (*s) {
        const char *end = strchr(s, ',');
        const size_t len = end ? (size_t)(end - s) : strlen(s);
        const char *slash = (const char *)memchr(s, '/', len);
        ref::Pattern a, b;
        if (!slash || !ref::parse_pattern(s, slash - s, &a) || !ref::parse_pattern(slash + 1, len - (slash + 1 - s), &b)) return false;
        o.pairs.emplace_back(a, b);
        s += len + (end ? 1 : 0);
    }
    return !o.pairs.empty();
}

// the flagged call: host-built operands, pattern pairs, a caller's chain, a batch of queries, giant-major slots
static int pattern_main(int G, int dim, int logN, int mode, const Options &o) {
    const int Q = o.Q, ng = o.ng;
    if (Q < 1 || ng < 0 || (ng > 0 && G % ng)) {
        printf("bad shape: %d queries, %d blocks, %d giant steps\n", Q, G, ng);
        return 2;
    }
    Params p;
    p.logN = logN;
    p.dim = dim;
    if (!o.moduli.empty()) {
        p.custom_q = o.moduli;
        p.custom_nP = o.np;
        p.mult_depth = (int)o.moduli.size() - o.np - 1;
    }
    Context cx(p, 0);
    const int N = cx.N, nl = cx.nQ;
    if (mode == 0) cx.db_seq_ok = false;
    if (mode == 2) cx.db_bits46_ok = false;
    const size_t cts = (size_t)G * dim, e = (size_t)2 * nl * N, blk = (size_t)dim * e;
    cx.db_resize((size_t)G * cx.slots, cts, dim);  // (as for kind 6: the form is the number of ciphertexts loop B walks per block)
    cx.db_kind = 5;
    cx.db_babies = dim;
    const DbLayout &L = cx.db_lay;
    char width[48];
    if (L.packed) snprintf(width, sizeof width, "%d-bit packed residues", L.bits46 ? 46 : 48);
    else snprintf(width, sizeof width, "unpacked 8-byte residues");
    printf("N = 2^%d, dim %d, %d blocks, %d queries, %d giant steps: %s layout (groups of %d blocks, %s), %.2f GiB resident\n", logN, dim, G, Q, ng,
           L.seq ? "group-sequential" : "ciphertext-major", L.seq, width, (double)cts * L.ct_bytes / (1 << 30));
    const unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    auto fill = [&](u64 *dst, ref::Pattern pat, u64 seed) {  // one rotation set or block, [i][poly][limb][c]
        std::vector<std::thread> th;
        for (unsigned t = 0; t < T; t++)
            th.emplace_back([&, t] {
                for (size_t lp = t; lp < (size_t)dim * 2 * nl; lp += T)
                    for (int c = 0; c < N; c++) dst[lp * N + c] = ref::residue(pat, seed, lp * N + c, cx.q[lp % nl]);
            });
        for (auto &x : th) x.join();
    };
    Ct rot(&cx, Q * dim, 2, nl, cx.delta);
    Ct direct(&cx, Q * G, 3, nl, cx.delta * cx.delta);  // the accumulators of a direct launcher call
    u64 *tmp = cx.pool.get(blk * sizeof(u64));
    std::vector<u64> hr((size_t)Q * blk), hb(blk), ha((size_t)Q * G * 3 * nl * N);
    long total_bad = 0;
    for (const auto &pr : o.pairs) {
        const std::string name = std::string(ref::pattern_name(pr.first)) + "/" + ref::pattern_name(pr.second);
        // query q: its own seed; the given pattern, holes, uniform in turn, so that no two queries' accumulators can be equal
        auto rot_pattern = [&](int q) { return q % 3 == 0 ? pr.first : q % 3 == 1 ? ref::HOLES : ref::UNIFORM; };
        auto rot_seed = [&](int q) { return seed_rot + 100 * (u64)q; };
        for (int q = 0; q < Q; q++) fill(hr.data() + (size_t)q * blk, rot_pattern(q), rot_seed(q));
        cx.sync();
        HIP_CHECK(hipMemcpy(rot.d, hr.data(), hr.size() * 8, hipMemcpyHostToDevice));
        for (int g = 0; g < G; g++) {
            fill(hb.data(), pr.second, seed_db + g);
            HIP_CHECK(hipMemcpy(tmp, hb.data(), blk * 8, hipMemcpyHostToDevice));
            cx.db_store((size_t)g * dim, tmp, dim);
            cx.sync();
        }
        hk::ledger_enable(true);
        if (Q == 1 && ng == 0) {
            Ct acc = cx.similarity_accumulate_rot(rot);
            cx.sync();
            HIP_CHECK(hipMemcpy(ha.data(), acc.d, ha.size() * 8, hipMemcpyDeviceToHost));
        } else {
            HIP_CHECK(hipMemsetAsync(direct.d, 0xFF, ha.size() * 8, cx.stream));  // a slot the launch misses is no residue
            if (Q == 1) hk::hydia_tensor_accumulate(cx.stream, cx.d_mod, N, rot.d, 0, cx.d_db, direct.d, 1, G, dim, nl, L, ng, cx.tensor_bpp, cx.tensor_nw);
            else hk::hydia_tensor_accumulate(cx.stream, cx.d_mod, N, rot.d, blk, cx.d_db, direct.d, Q, G, dim, nl, L, ng, hk::TENSOR_BATCH, 0);
            cx.sync();
            HIP_CHECK(hipMemcpy(ha.data(), direct.d, ha.size() * 8, hipMemcpyDeviceToHost));
        }
        std::vector<char> led(hk::ledger_dump(nullptr, 0));
        hk::ledger_dump(led.data(), led.size());
        hk::ledger_enable(false);
        for (char *line = strtok(led.data(), "\n"); line; line = strtok(nullptr, "\n"))
            if (!strncmp(line, "k_hydia_tensor", 14)) {
                char *tab = strchr(line, '\t');
                if (!tab) continue;
                *tab = 0;
                printf("ledger %s: %s x%d\n", name.c_str(), line, atoi(tab + 1));
            }
        const long bad = compare(
            cx, ha, Q, G, ng, dim, T, [&](int q, int i, int pl, int j, int c) { return hr[(size_t)q * blk + ref::operand_index(i, pl, j, c, nl, N)]; },
            [&](int g, int i, int pl, int j, int c) { return ref::residue(pr.second, seed_db + g, ref::operand_index(i, pl, j, c, nl, N), cx.q[j]); });
        printf("%s: loop B, %d queries x %d blocks x %d diagonals at N = 2^%d: %ld mismatches of %ld (query, block, limb, coefficient) triples\n",
               name.c_str(), Q, G, dim, logN, bad, (long)Q * G * nl * N);
        fflush(stdout);
        total_bad += bad;
    }
    cx.sync();
    cx.pool.put(tmp);
    return total_bad != 0;
}

int main(int argc, char **argv) {
    std::vector<const char *> pos;
    Options o;
    bool flagged = false;
    for (int a = 1; a < argc; a++) {
        if (strncmp(argv[a], "--", 2)) {
            pos.push_back(argv[a]);
            continue;
        }
        flagged = true;
        const char *v = a + 1 < argc ? argv[a + 1] : nullptr;
        if (!v) {
            printf("%s needs a value\n", argv[a]);
            return 2;
        }
        if (!strcmp(argv[a], "--moduli")) {
            for (const char *s = v; *s;) {
                char *end;
                o.moduli.push_back(strtoull(s, &end, 10));
                s = *end ? end + 1 : end;
            }
        } else if (!strcmp(argv[a], "--np")) o.np = atoi(v);
        else if (!strcmp(argv[a], "--queries")) o.Q = atoi(v);
        else if (!strcmp(argv[a], "--giants")) o.ng = atoi(v);
        else if (!strcmp(argv[a], "--patterns")) {
            if (!parse_pairs(v, o)) {
                printf("bad pattern pairs %s\n", v);
                return 2;
            }
        } else {
            printf("unknown flag %s\n", argv[a]);
            return 2;
        }
        a++;
    }
    const int G = pos.size() > 0 ? atoi(pos[0]) : 2, dim = pos.size() > 1 ? atoi(pos[1]) : 8, logN = pos.size() > 2 ? atoi(pos[2]) : 11;
    const int mode = pos.size() > 3 ? atoi(pos[3]) : 1;
    if (!flagged) return uniform_main(G, dim, logN, mode);
    if (o.pairs.empty()) o.pairs.emplace_back(ref::UNIFORM, ref::UNIFORM);
    try {
        return pattern_main(G, dim, logN, mode, o);
    } catch (const std::exception &ex) {
        printf("refused: %s\n", ex.what());
        return 3;
    }
}
