// Host check of the ONE-polynomial address map of a plain gallery (image_matching_amd/csrc/db_layout.h with DbLayout::plain set; the
// two-polynomial map is checked by db_layout_check.cpp): in both layouts every residue pair of every (plaintext, limb) gets its own
// bytes, the map is a bijection onto entries * ct_bytes with ct_bytes = poly_bytes, the widest access — lane 63's 16-byte load of the
// last 46-bit unit — ends inside db_alloc_size, and in the group-sequential layout the bytes a loop-B workgroup reads (one 128-residue
// tile of one limb of one group of blocks, every diagonal, ONE polynomial) are one contiguous run.  The walk the kernels use
// (base + u su + i si, restated here from kernels.hip's db_walk) lands on db_offset.
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "db_layout.h"

static DbLayout make(int N, int nQ, int packed, int bd, int blocks, int gs, int bpp, int bits46) {
    DbLayout L{};
    L.plain = 1;
    L.packed = packed;
    L.bits46 = (bits46 && gs && packed) ? 1 : 0;
    L.poly_bytes = packed ? (unsigned long long)N * 8 + (unsigned long long)(nQ - 1) * (L.bits46 ? (N / 128) * 736 : N * 6) : (unsigned long long)nQ * N * 8;
    L.ct_bytes = db_polys(L) * L.poly_bytes;
    L.seq = gs;
    L.seq_bpp = bpp;
    L.bd = bd;
    L.blocks = blocks;
    return L;
}

static int check(int N, int nQ, int packed, int bd, int blocks, int gs, int bits46 = 0) {
    const DbLayout L = make(N, nQ, packed, bd, blocks, gs, 1, bits46);
    if (db_polys(L) != 1 || L.ct_bytes != L.poly_bytes) return printf("a plain layout holds one polynomial per entry\n"), 1;
    DbLayout two = L;
    two.plain = 0;
    if (db_polys(two) != 2 || db_polys(DbLayout{}) != 2) return printf("the zero value means two polynomials\n"), 1;
    const size_t pts = (size_t)bd * blocks, total = pts * L.ct_bytes;
    std::vector<unsigned char> used(total, 0);
    for (size_t t = 0; t < pts; t++)
        for (int j = 0; j < nQ; j++)
            for (size_t c = 0; c < (size_t)N; c += (L.bits46 && j > 0) ? 16 : 2) {
                const size_t es = (L.bits46 && j > 0) ? 46 : (packed && j > 0) ? 6 : 8, o = db_offset(L, N, t, 0, j, c);
                if (o + 2 * es > total) return printf("out of range: t %zu j %d c %zu\n", t, j, c), 1;
                if (o % 4) return printf("granule not on a dword: t %zu j %d c %zu\n", t, j, c), 1;
                for (size_t k = 0; k < 2 * es; k++) {
                    if (used[o + k]) return printf("overlap at byte %zu (t %zu j %d c %zu)\n", o + k, t, j, c), 1;
                    used[o + k] = 1;
                }
            }
    for (size_t k = 0; k < total; k++)
        if (!used[k]) return printf("hole at byte %zu\n", k), 1;
    if (db_alloc_size(L, pts) != total + DB_ALLOC_TAIL) return printf("allocation is not the layout's bytes plus the tail\n"), 1;
    if (L.bits46) {
        size_t last = 0;
        for (size_t t = 0; t < pts; t++)
            for (int j = 1; j < nQ; j++)
                for (size_t c = 0; c < (size_t)N; c += 128) last = std::max(last, db_offset(L, N, t, 0, j, c));
        if (last + 736 != total) return printf("the last 46-bit unit does not end the layout\n"), 1;
        if (last + db_lane_load46(63) + 16 <= total) return printf("lane 63 stays inside the unit: the tail would be dead weight\n"), 1;
        if (last + db_lane_load46(63) + 16 > db_alloc_size(L, pts)) return printf("lane 63's load ends past the allocation\n"), 1;
    }
    if (gs) {
        for (int j = 0; j < nQ; j++)
            for (int tile = 0; tile < N / 128; tile++)
                for (int grp = 0; grp < blocks / gs; grp++) {
                    size_t expect = db_offset(L, N, (size_t)grp * gs * bd, 0, j, (size_t)tile * 128);
                    // the kernels' walk: first byte of the group, then + u su + i si with su = one unit, si = gs units
                    const size_t base = expect, su = db_unit_bytes(L, j), si = (size_t)gs * su;
                    for (int i = 0; i < bd; i++)
                        for (int u = 0; u < gs; u++) {
                            const size_t o = db_offset(L, N, ((size_t)grp * gs + u) * bd + i, 0, j, (size_t)tile * 128);
                            if (o != expect) return printf("run broken: j %d tile %d grp %d i %d u %d\n", j, tile, grp, i, u), 1;
                            if (o != base + u * su + i * si) return printf("walk off the map: j %d tile %d grp %d i %d u %d\n", j, tile, grp, i, u), 1;
                            expect += db_unit_bytes(L, j);
                        }
                }
    } else {  // ciphertext-major: entry after entry, poly_bytes apart
        for (size_t t = 0; t < pts; t++)
            if (db_offset(L, N, t, 0, 0, 0) != t * L.poly_bytes) return printf("entry %zu is not at t * poly_bytes\n", t), 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    bad |= check(256, 3, 1, 4, 12, 0);  // ciphertext-major, packed
    bad |= check(256, 3, 0, 4, 12, 0);  // ciphertext-major, 8-byte
    bad |= check(256, 3, 1, 4, 12, 4);  // group-sequential, groups of 4
    bad |= check(256, 4, 1, 8, 16, 8);
    bad |= check(512, 2, 1, 2, 9, 1);   // degenerate groups of one block
    bad |= check(256, 3, 1, 4, 20, 2);
    bad |= check(256, 3, 1, 4, 12, 4, 1);  // group-sequential with 46-bit residues in 736-byte units
    bad |= check(512, 4, 1, 8, 16, 8, 1);
    bad |= check(256, 2, 1, 2, 10, 2, 1);
    bad |= check(256, 3, 1, 3, 10, 2, 1);  // an odd count of diagonals: the units of a limb do not pair up
    if (!bad) printf("plain db layout ok\n");
    return bad;
}
