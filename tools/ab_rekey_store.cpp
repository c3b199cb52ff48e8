// tools/ab_rekey_store.cpp — the fused store of a re-key (hk::db_rekey_store: c0 read-add-reduce-write where it lies, c1 overwritten)
// against the unfused form it replaces: hk::db_unpack of the chunk, hk::add on polynomial 0, hk::db_pack.  Measurement only: the
// unfused form exists here and nowhere in the library.  Reads the engine's internal structures directly, like tests/csrc/loop_b_check.
// Full ring, uniform residues (the kernels' cost is data independent), the layout the context picks for <blocks> hoisted blocks.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I image_matching_amd/csrc -I include tools/ab_rekey_store.cpp -L image_matching_amd
//         -lhydia -lpthread -Wl,-rpath,'$ORIGIN/../image_matching_amd' -o tools/ab_rekey_store          (tools/bench_db_rekey.py --build)
// Usage: ab_rekey_store <blocks> <dim> <chunk> <reps>: alternates the two forms on the chunks of the database, `reps` passes each after
// one warm-up pass of each; one JSON line with the per-pass device-event times.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hydia_core.h"
using namespace hydia;

int main(int argc, char **argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s <blocks> <dim> <chunk> <reps>\n", argv[0]);
        return 2;
    }
    const int G = atoi(argv[1]), dim = atoi(argv[2]), C = atoi(argv[3]), reps = atoi(argv[4]);
    if (G < 1 || dim < 2 || C < 1 || C > 256 || reps < 1) return 2;
    Params p;
    p.dim = dim;
    Context cx(p, 0);
    const int N = cx.N, nQ = cx.nQ;
    const size_t cts = (size_t)G * dim, pe = (size_t)nQ * N;
    cx.db_resize((size_t)G * cx.slots, cts, dim);
    cx.db_kind = 5;
    cx.db_babies = dim;
    u64 *ks = cx.pool.get((size_t)C * 2 * pe * sizeof(u64)), *tmp = cx.pool.get((size_t)C * 2 * pe * sizeof(u64));
    for (size_t t0 = 0; t0 < cts; t0 += (size_t)C) {
        const int X = (int)std::min((size_t)C, cts - t0);
        hk::fill_uniform_hash(cx.stream, cx.d_mod, N, tmp, (size_t)X * 2 * nQ, nQ, 77 + t0);
        cx.db_store(t0, tmp, X);
    }
    hk::fill_uniform_hash(cx.stream, cx.d_mod, N, ks, (size_t)C * 2 * nQ, nQ, 5);
    cx.sync();
    const LimbSel qsel = cx.sel_q(nQ);
    auto pass = [&](bool fused) {
        hipEvent_t a, b;
        HIP_CHECK(hipEventCreate(&a));
        HIP_CHECK(hipEventCreate(&b));
        HIP_CHECK(hipEventRecord(a, cx.stream));
        for (size_t t0 = 0; t0 < cts; t0 += (size_t)C) {
            const int X = (int)std::min((size_t)C, cts - t0);
            if (fused) {
                hk::db_rekey_store(cx.stream, cx.d_mod, N, nQ, ks, cx.d_db, t0, X, cx.db_lay);
            } else {
                hk::db_unpack(cx.stream, N, nQ, tmp, cx.d_db, t0, X, cx.db_lay);
                hk::add(cx.stream, cx.d_mod, N, tmp, ks, tmp, X, qsel, 2 * nQ, 2 * nQ, 2 * nQ);  // c0 += ks0
                hk::copy_limbs(cx.stream, N, ks + pe, tmp + pe, 2 * pe, 2 * pe, X, nQ);                   // c1 = ks1
                hk::db_pack(cx.stream, N, nQ, tmp, cx.d_db, t0, X, cx.db_lay);
            }
        }
        HIP_CHECK(hipEventRecord(b, cx.stream));
        HIP_CHECK(hipEventSynchronize(b));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, a, b));
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        return (double)ms;
    };
    pass(true);
    pass(false);
    std::vector<double> f, u;
    for (int r = 0; r < reps; r++) {
        f.push_back(pass(true));
        u.push_back(pass(false));
    }
    printf("{\"ab\": \"rekey_store\", \"blocks\": %d, \"dim\": %d, \"chunk\": %d, \"cts\": %zu, \"db_group\": %d, \"bits46\": %d, \"ct_bytes\": %llu, \"fused_ms\": [", G,
           dim, C, cts, cx.db_lay.seq, cx.db_lay.bits46, (unsigned long long)cx.db_lay.ct_bytes);
    for (size_t i = 0; i < f.size(); i++) printf("%s%.3f", i ? ", " : "", f[i]);
    printf("], \"unfused_ms\": [");
    for (size_t i = 0; i < u.size(); i++) printf("%s%.3f", i ? ", " : "", u[i]);
    printf("]}\n");
    cx.pool.put(tmp);
    cx.pool.put(ks);
    return 0;
}
