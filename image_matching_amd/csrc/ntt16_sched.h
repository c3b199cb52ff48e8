// image_matching_amd/csrc/ntt16_sched.h — the butterfly schedule of the N = 2^16 two-pass transforms: which stage runs where, with which
// twiddle, and where the lazy arithmetics fold / re-centre.  Included by the kernels (ntt16.hip) AND by the host check
// (tests/csrc/ntt16_arith_check.cpp), so the schedule whose bounds are checked on the CPU is the schedule the GPU runs.  The bounds are
// derived in the file header of ntt16.hip.
//
// Every function takes the values of ONE register phase of one lane (A::T, the arithmetic's own representation) and a twiddle accessor
// tw(i) -> A::TW for entry i of the limb's table (forward table for the n16_*_fwd_* functions, inverse table for n16_*_inv_*).  A stage
// with stride t reads entry N/(2t) + i, i the index of the butterfly's 2t-block — the indices of the ring-size-generic kernels.
#pragma once
#include "ntt_arith.h"

namespace {

// which coefficients a lane holds in each register phase.  Pass 1 (one column of the 256 x 256 matrix): value k of row group g in phase
// A, value l of row group h in phase B.  Pass 2 (position inside the 256-block of half-wave lane w < 32): value k in phases A and B,
// the first of four consecutive positions of group hh in phase C.
DEV int n16_p1_row_A(int g, int k) { return g + 16 * k; }
DEV int n16_p1_row_B(int h, int l) { return 16 * h + l; }
DEV int n16_p2_pos_A(int w, int k) { return 32 * k + w; }
DEV int n16_p2_pos_B(int w, int k) { return 32 * (w >> 2) + 4 * k + (w & 3); }
DEV int n16_p2_pos_C(int w, int hh) { return 4 * w + 128 * hh; }

// ------------------------------------------------------------------------------------------------ pass 1: rows (stages 0-7)
// phase A: v[k] = row n16_p1_row_A(g, k) (any g < 16, any column); stages 0-3, row strides 128, 64, 32, 16.  Workgroup-uniform twiddles 1 .. 15.
template <class A, class TWF>
DEV void n16_p1_fwd_A(const A &ar, typename A::T (&v)[16], TWF tw) {
#pragma unroll
    for (int st = 0; st < 4; st++) {
        const int h = 8 >> st;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (!(k & h)) ar.ct(v[k], v[k + h], tw((1 << st) + (k >> (4 - st))));
        if (st == 2) {  // IntP: three stages from canonical input, fold, the fourth leaves 5+ q
#pragma unroll
            for (int k = 0; k < 16; k++) ar.fwd_fold(v[k]);
        }
    }
}
// phase B: w[l] = row n16_p1_row_B(h, l); stages 4-7, row strides 8, 4, 2, 1.  Twiddles 16 .. 255.
template <class A, class TWF>
DEV void n16_p1_fwd_B(const A &ar, typename A::T (&w)[16], int h, TWF tw) {
#pragma unroll
    for (int st = 0; st < 4; st++) {
        const int hh = 8 >> st;
#pragma unroll
        for (int l = 0; l < 16; l++)
            if (!(l & hh)) ar.ct(w[l], w[l + hh], tw((16 << st) + (h << st) + (l >> (4 - st))));
        if (st == 1) {  // IntP: 5+ -> 9+ -> 13+ q, fold, two more stages leave 9+ q for pass 2 (which folds on reading)
#pragma unroll
            for (int l = 0; l < 16; l++) ar.fwd_fold(w[l]);
        }
    }
}
// inverse phase B': strides 1, 2, 4 | reduction | 8
template <class A, class TWF>
DEV void n16_p1_inv_B(const A &ar, typename A::T (&w)[16], int h, TWF tw) {
#pragma unroll
    for (int st = 3; st >= 0; st--) {
        const int hh = 8 >> st;
#pragma unroll
        for (int l = 0; l < 16; l++)
            if (!(l & hh)) ar.gs(w[l], w[l + hh], tw((16 << st) + (h << st) + (l >> (4 - st))));
        if (st == 1) {
#pragma unroll
            for (int l = 0; l < 16; l++) ar.recentre(w[l]);
        }
    }
}
// inverse phase A': strides 16, 32 | reduction (IntP, non-lean FpA) | 64, 128; the caller finishes with fin_inv
template <class A, class TWF>
DEV void n16_p1_inv_A(const A &ar, typename A::T (&v)[16], TWF tw) {
#pragma unroll
    for (int st = 3; st >= 0; st--) {
        const int h = 8 >> st;
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (!(k & h)) ar.gs(v[k], v[k + h], tw((1 << st) + (k >> (4 - st))));
        if (st == 2) {
#pragma unroll
            for (int k = 0; k < 16; k++) ar.recentre_wide(v[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ pass 2: inside 256-blocks (stages 8-15)
// NP polynomials of one limb share the twiddles.  bg = index of the 256-block in the limb-polynomial.
// phase A: v[p][k] = coefficient 32k + w of the block (caller: from_raw on loading); stages 8, 9, 10 (strides 128, 64, 32)
template <class A, int NP, class TWF>
DEV void n16_p2_fwd_A(const A &ar, typename A::T (&v)[NP][8], int bg, TWF tw) {
    const typename A::TW W8 = tw(256 + bg), W9a = tw(512 + 2 * bg), W9b = tw(512 + 2 * bg + 1);
    typename A::TW W10[4];
#pragma unroll
    for (int i = 0; i < 4; i++) W10[i] = tw(1024 + 4 * bg + i);
#pragma unroll
    for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int k = 0; k < 4; k++) ar.ct(v[p][k], v[p][k + 4], W8);
        ar.ct(v[p][0], v[p][2], W9a);
        ar.ct(v[p][1], v[p][3], W9a);
        ar.ct(v[p][4], v[p][6], W9b);
        ar.ct(v[p][5], v[p][7], W9b);
#pragma unroll
        for (int k = 0; k < 8; k += 2) ar.ct(v[p][k], v[p][k + 1], W10[k >> 1]);
#pragma unroll
        for (int k = 0; k < 8; k++) ar.fwd_fold(v[p][k]);
    }
}
// phase B: v[p][k] = coefficient n16_p2_pos_B(w, k) = 32a + 4k + b of the block, ib = 8 bg + a; stages 11, 12, 13 (strides 16, 8, 4)
template <class A, int NP, class TWF>
DEV void n16_p2_fwd_B(const A &ar, typename A::T (&v)[NP][8], int ib, TWF tw) {
    const typename A::TW W11 = tw(2048 + ib), W12a = tw(4096 + 2 * ib), W12b = tw(4096 + 2 * ib + 1);
    typename A::TW W13[4];
#pragma unroll
    for (int i = 0; i < 4; i++) W13[i] = tw(8192 + 4 * ib + i);
#pragma unroll
    for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int k = 0; k < 4; k++) ar.ct(v[p][k], v[p][k + 4], W11);
        ar.ct(v[p][0], v[p][2], W12a);
        ar.ct(v[p][1], v[p][3], W12a);
        ar.ct(v[p][4], v[p][6], W12b);
        ar.ct(v[p][5], v[p][7], W12b);
#pragma unroll
        for (int k = 0; k < 8; k += 2) ar.ct(v[p][k], v[p][k + 1], W13[k >> 1]);
    }
}
// phase C: c[p][0..3] = four consecutive coefficients 4 gi .. 4 gi + 3 of the limb-polynomial; stages 14, 15 (strides 2, 1); the caller
// finishes with fin_fwd
template <class A, int NP, class TWF>
DEV void n16_p2_fwd_C(const A &ar, typename A::T (&c)[NP][4], int gi, TWF tw) {
    const typename A::TW W14 = tw(16384 + gi), W15a = tw(32768 + 2 * gi), W15b = tw(32768 + 2 * gi + 1);
#pragma unroll
    for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int k = 0; k < 4; k++) ar.mid(c[p][k]);
        ar.ct(c[p][0], c[p][2], W14);
        ar.ct(c[p][1], c[p][3], W14);
        ar.ct(c[p][0], c[p][1], W15a);
        ar.ct(c[p][2], c[p][3], W15b);
    }
}
// inverse phase C' (caller: from_canon on loading): strides 1, 2
template <class A, int NP, class TWF>
DEV void n16_p2_inv_C(const A &ar, typename A::T (&c)[NP][4], int gi, TWF tw) {
    const typename A::TW W14 = tw(16384 + gi), W15a = tw(32768 + 2 * gi), W15b = tw(32768 + 2 * gi + 1);
#pragma unroll
    for (int p = 0; p < NP; p++) {
        ar.gs(c[p][0], c[p][1], W15a);
        ar.gs(c[p][2], c[p][3], W15b);
        ar.gs(c[p][0], c[p][2], W14);
        ar.gs(c[p][1], c[p][3], W14);
#pragma unroll
        for (int k = 0; k < 4; k++) ar.recentre_wide(c[p][k]);
    }
}
// inverse phase B': strides 4, 8, 16
template <class A, int NP, class TWF>
DEV void n16_p2_inv_B(const A &ar, typename A::T (&v)[NP][8], int ib, TWF tw) {
    const typename A::TW W11 = tw(2048 + ib), W12a = tw(4096 + 2 * ib), W12b = tw(4096 + 2 * ib + 1);
    typename A::TW W13[4];
#pragma unroll
    for (int i = 0; i < 4; i++) W13[i] = tw(8192 + 4 * ib + i);
#pragma unroll
    for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int k = 0; k < 8; k += 2) ar.gs(v[p][k], v[p][k + 1], W13[k >> 1]);
        ar.gs(v[p][0], v[p][2], W12a);
        ar.gs(v[p][1], v[p][3], W12a);
        ar.gs(v[p][4], v[p][6], W12b);
        ar.gs(v[p][5], v[p][7], W12b);
#pragma unroll
        for (int k = 0; k < 4; k++) ar.gs(v[p][k], v[p][k + 4], W11);
#pragma unroll
        for (int k = 0; k < 8; k++) ar.recentre(v[p][k]);
    }
}
// inverse phase A': strides 32, 64, 128; leaves the raw image pass 1' reads
template <class A, int NP, class TWF>
DEV void n16_p2_inv_A(const A &ar, typename A::T (&v)[NP][8], int bg, TWF tw) {
    const typename A::TW W8 = tw(256 + bg), W9a = tw(512 + 2 * bg), W9b = tw(512 + 2 * bg + 1);
    typename A::TW W10[4];
#pragma unroll
    for (int i = 0; i < 4; i++) W10[i] = tw(1024 + 4 * bg + i);
#pragma unroll
    for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int k = 0; k < 8; k += 2) ar.gs(v[p][k], v[p][k + 1], W10[k >> 1]);
        ar.gs(v[p][0], v[p][2], W9a);
        ar.gs(v[p][1], v[p][3], W9a);
        ar.gs(v[p][4], v[p][6], W9b);
        ar.gs(v[p][5], v[p][7], W9b);
#pragma unroll
        for (int k = 0; k < 4; k++) ar.gs(v[p][k], v[p][k + 4], W8);
#pragma unroll
        for (int k = 0; k < 8; k++) ar.recentre_wide(v[p][k]);
    }
}

}  // namespace
