// Host check of image_matching_amd/csrc/ntt_arith.h — the three butterfly arithmetics of the N = 2^15 transforms (IntA, IntP, FpA) —
// against exact integer arithmetic (unsigned / signed __int128).  The header itself is compiled here (host_shim.h supplies the HIP
// names), so this checks the real structs.  Build with -O2 -std=c++17 -ffp-contract=off and no fast-math: every double operation is
// then the single IEEE operation the device performs.  Run by tests/test_devmath_host.py.
//
// usage: ntt_arith_check [q ...]   — extra moduli (the default chain, passed by the test); the edge moduli are derived below from the
// context's selection rule (context.cpp: FP64 for <= 47 bits; IntP for q = 2^60 - c, c < 2^24; IntA otherwise).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
#include "ntt_arith.h"

typedef __int128 i128;

static u64 rng_state = 0x2545F4914F6CDD1Dull;
static u64 rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static u64 rnd_below(u64 n) { return (u64)(((u128)rnd() * n) >> 64); }

static long g_checks = 0;
#define REQUIRE(cond, ...)                                  \
    do {                                                    \
        g_checks++;                                         \
        if (!(cond)) {                                      \
            printf("FAIL %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
            exit(1);                                        \
        }                                                   \
    } while (0)

static u64 mulm(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
static u64 powm(u64 a, u64 e, u64 q) {
    u64 r = 1 % q;
    for (a %= q; e; e >>= 1, a = mulm(a, a, q))
        if (e & 1) r = mulm(r, a, q);
    return r;
}
static bool is_prime(u64 n) {  // deterministic Miller-Rabin for 64-bit n
    if (n < 2) return false;
    for (u64 p : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull})
        if (n % p == 0) return n == p;
    u64 d = n - 1;
    int s = 0;
    while (!(d & 1)) d >>= 1, s++;
    for (u64 a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
        u64 x = powm(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int r = 1; r < s && comp; r++) {
            x = mulm(x, x, n);
            if (x == n - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}
static u64 modinv(u64 a, u64 q) { return powm(a, q - 2, q); }
static ModC make(u64 q) {  // as context.cpp fills ModC (only q is read by the structs)
    ModC m{};
    m.q = q;
    const int k = 64 - __builtin_clzll(q);
    m.ks = k - 2;
    m.mu = (u64)((((u128)1) << (k + 62)) / q);
    m.r64 = (u64)((((u128)1) << 64) / q);
    return m;
}
static int bits(u64 q) { return 64 - __builtin_clzll(q); }
// the context's per-modulus rule (context.cpp): 0 FpA, 1 IntP, 2 IntA
static int arith_of(u64 q) {
    if (bits(q) <= 47) return 0;
    if (q < (1ull << 60) && (1ull << 60) - q < (1ull << 24)) return 1;
    return 2;
}
static const char *kName[3] = {"FpA", "IntP", "IntA"};
// every 2N-th root of unity (powers of a primitive one), N = 2^logn
static std::vector<u64> roots_of(u64 q, int logn) {
    const u64 n2 = 2ull << logn;
    REQUIRE((q - 1) % n2 == 0, "q=%llu is not 1 mod 2N", q);
    u64 psi = 0;
    for (u64 g = 2;; g++) {
        psi = powm(g, (q - 1) / n2, q);
        if (powm(psi, n2 >> 1, q) == q - 1) break;
    }
    std::vector<u64> r(n2);
    r[0] = 1;
    for (u64 k = 1; k < n2; k++) r[k] = mulm(r[k - 1], psi, q);
    return r;
}
// twiddles to use: 1, q - 1 (= psi^N), the largest and smallest roots other than 1, and random ones
static std::vector<u64> pick_twiddles(u64 q, int logn, int nrand) {
    const std::vector<u64> r = roots_of(q, logn);
    u64 hi = 0, lo = q;
    for (u64 w : r) {
        if (w != q - 1 && w > hi) hi = w;
        if (w != 1 && w < lo) lo = w;
    }
    std::vector<u64> t = {1, q - 1, hi, lo, r[1], r[r.size() - 1]};
    for (int i = 0; i < nrand; i++) t.push_back(r[rnd_below(r.size())]);
    return t;
}
static ulonglong2 shoup_pair(u64 w, u64 q) { return ulonglong2{w, (u64)((((u128)w) << 64) / q)}; }
static u64 modq(i128 v, u64 q) {
    i128 r = v % (i128)q;
    return (u64)(r < 0 ? r + q : r);
}

struct Worst {  // largest observed output / q per class and method
    double v = 0;
    void see(double x) { v = x > v ? x : v; }
};

// ------------------------------------------------------------------------------------------------------------------------- IntA
static void check_inta(u64 q, int logn, Worst &w_ct, Worst &w_gs) {
    const IntA ar(make(q));
    const u64 q2 = 2 * q, q4 = 4 * q;
    const u64 e4[] = {0, 1, q - 1, q, q + 1, q2 - 1, q2, q2 + 1, 3 * q, q4 - 2, q4 - 1};
    const u64 e2[] = {0, 1, q - 1, q, q + 1, q2 - 2, q2 - 1};
    for (u64 w : pick_twiddles(q, logn, 24)) {
        const ulonglong2 W = IntA::tw(shoup_pair(w, q));
        auto ct = [&](u64 a, u64 b) {
            u64 x = a, y = b;
            ar.ct(x, y, W);
            REQUIRE(x < q4 && y < q4, "IntA::ct q=%llu a=%llu b=%llu -> %llu %llu", q, a, b, x, y);
            const u64 bw = mulm(b % q, w, q);
            REQUIRE(x % q == (a % q + bw) % q && y % q == (a % q + q - bw) % q, "IntA::ct residue q=%llu a=%llu b=%llu", q, a, b);
            w_ct.see((double)(x > y ? x : y) / q);
        };
        auto gs = [&](u64 a, u64 b) {
            u64 x = a, y = b;
            ar.gs(x, y, W);
            REQUIRE(x < q2 && y < q2, "IntA::gs q=%llu a=%llu b=%llu -> %llu %llu", q, a, b, x, y);
            REQUIRE(x % q == (a + b) % q && y % q == mulm((a % q + q - b % q) % q, w, q), "IntA::gs residue q=%llu a=%llu b=%llu", q, a, b);
            w_gs.see((double)(x > y ? x : y) / q);
        };
        for (u64 a : e4) for (u64 b : e4) ct(a, b);
        for (u64 a : e2) for (u64 b : e2) gs(a, b);
        for (int i = 0; i < 20000; i++) {
            ct(rnd_below(q4), rnd_below(q4));
            gs(rnd_below(q2), rnd_below(q2));
        }
    }
    for (u64 x : {0ull, 1ull, q - 1, q, 2 * q - 1, 2 * q, 3 * q, 4 * q - 1}) REQUIRE(ar.fin_fwd(x) == x % q, "IntA::fin_fwd q=%llu x=%llu", q, x);
    for (int i = 0; i < 100000; i++) {
        const u64 x = rnd_below(q4);
        REQUIRE(ar.fin_fwd(x) == x % q, "IntA::fin_fwd q=%llu x=%llu", q, x);
    }
}

// ------------------------------------------------------------------------------------------------------------------------- IntP
// The conversion sums of colfuse.hip (cf_macN), reproduced to derive fold_lh's input range from its call sites: NS sources y < 2^60
// and constants f < 2^60, both cut at 30 bits.  With yl, yh, fl, fh < 2^30:  ll, hh <= NS (2^30 - 1)^2,  mid <= 2 NS (2^30 - 1)^2,
// L = ll + (mid mod 2^32) 2^30,  H = hh + 4 (mid >> 32).  For NS = 4 (the widest call with 60-bit sources): L < 2^62 + 2^62 = 2^63
// and H < 2^62 + 2^33.  For NS = 5 (sources below 2^48, yh < 2^18): ll < 5 2^60, so L < 5 2^60 + 2^62 = 9 2^60 (not 2^63: still
// one 64-bit word, and fold_lh takes any L), and H < 5 2^48 + 2^20 < 2^51.  Every call site (cf_convert and the two
// column-fused conversions) then adds at most one residue below q (the dropped limb's), and the first forward stage takes the sum.
static void cf_sum(const u64 *y, const u64 *f, int ns, u64 &L, u64 &H) {
    u64 pll = 0, pmid = 0, phh = 0;
    for (int s = 0; s < ns; s++) {
        const u64 yl = y[s] & 0x3FFFFFFFull, yh = y[s] >> 30, fl = f[s] & 0x3FFFFFFFull, fh = f[s] >> 30;
        pll += yl * fl;
        pmid += yl * fh;
        pmid += yh * fl;
        phh += yh * fh;
    }
    L = pll + ((pmid & 0xFFFFFFFFull) << 30);
    H = phh + ((pmid >> 32) << 2);
}
static const u128 kTwo60 = ((u128)1) << 60;
static Worst w_L[2];  // largest conversion-sum L / 2^60 for NS = 4, 5
static void check_intp(u64 q, int logn, Worst &w_sh, Worst &w_ct, Worst &w_gs, Worst &w_lh, Worst &w_128, long &deficit2) {
    const IntP ar(make(q));
    const u64 c = (1ull << 60) - q;
    REQUIRE(ar.c == c, "IntP c");
    const u64 q4 = 4 * q, q8 = 8 * q, q12 = 12 * q, q16 = 16 * q;
    const u64 fold_max = (1ull << 60) - 1 + 15 * c;
    // fold: ANY 64-bit x -> [0, 2^60 + 15c), same residue
    auto fold = [&](u64 x) {
        const u64 r = ar.fold(x);
        REQUIRE(r <= fold_max && r % q == x % q, "IntP::fold q=%llu x=%llu -> %llu", q, x, r);
        REQUIRE(ar.fin_fwd(x) == x % q, "IntP::fin_fwd q=%llu x=%llu", q, x);
    };
    const u64 e64[] = {0, 1, q - 1, q, q + 1, 2 * q - 1, 4 * q - 1, 12 * q, q16 - 1, q16, q16 + 1, 1ull << 63, (1ull << 63) - 1,
                       ~0ull, ~0ull - 1, (1ull << 60) - 1, 1ull << 60, ~0ull - ((1ull << 60) - 1)};
    for (u64 x : e64) fold(x);
    for (int i = 0; i < 200000; i++) fold(rnd());
    for (u64 w : pick_twiddles(q, logn, 24)) {
        const ulonglong2 W = IntP::tw(shoup_pair(w, q));
        // shoup: ANY 64-bit x -> [0, 4q), x w mod q
        auto shoup = [&](u64 x) {
            const u64 r = ar.shoup(x, W);
            REQUIRE(r < q4 && r % q == mulm(x % q, w, q), "IntP::shoup q=%llu w=%llu x=%llu -> %llu", q, w, x, r);
            w_sh.see((double)r / q);
            const u64 hi = __umul64hi(x, W.y);
            const u64 hi2 = (u64)(x >> 32) * (W.y >> 32) + ((u64)__umulhi((unsigned)x, (unsigned)(W.y >> 32)) + (u64)__umulhi((unsigned)(x >> 32), (unsigned)W.y));
            if (hi - hi2 == 2) deficit2++;
        };
        for (u64 x : e64) shoup(x);
        // adversarial: low words that maximise the dropped terms lo32(xl wh) 2^32, lo32(xh wl) 2^32 and xl wl
        const unsigned wl = (unsigned)W.y, wh = (unsigned)(W.y >> 32);
        std::vector<unsigned> xls = {0xFFFFFFFFu, 0xFFFFFFFEu, 0x80000000u}, xhs = {0xFFFFFFFFu, 0x0FFFFFFFu, 0x7FFFFFFFu};
        auto inv32 = [](unsigned a) {  // inverse of an odd a mod 2^32
            unsigned x = a;
            for (int i = 0; i < 5; i++) x *= 2 - a * x;
            return x;
        };
        for (unsigned t : {0xFFFFFFFFu, 0xFFFFFFF0u, 0xF0000000u}) {
            if (wh & 1) xls.push_back(t * inv32(wh));
            if (wl & 1) xhs.push_back(t * inv32(wl));
            if (wh & 1) xls.push_back((t * inv32(wh)) | 0x80000000u);
        }
        for (unsigned xl : xls)
            for (unsigned xh : xhs) shoup(((u64)xh << 32) | xl);
        for (int i = 0; i < 20000; i++) shoup(rnd());
        // ct: a < 12q (the largest pre-stage value: three stages of +4q from a fold below 2^60 + 15c, and the column-fused
        // conversions' 3.1q), b any 64-bit -> both below 16q = 2^64 - 16c
        auto ct = [&](u64 a, u64 b) {
            u64 x = a, y = b;
            ar.ct(x, y, W);
            REQUIRE(x < q16 && y < q16, "IntP::ct q=%llu a=%llu b=%llu -> %llu %llu", q, a, b, x, y);
            const u64 bw = mulm(b % q, w, q);
            REQUIRE(x % q == (a % q + bw) % q && y % q == (a % q + q - bw) % q, "IntP::ct residue q=%llu a=%llu b=%llu", q, a, b);
            w_ct.see((double)(x > y ? x : y) / q);
        };
        const u64 ea[] = {0, 1, q - 1, q, fold_max, 4 * q, 8 * q - 1, q12 - 2, q12 - 1};
        for (u64 a : ea) for (u64 b : e64) ct(a, b);
        for (int i = 0; i < 20000; i++) ct(rnd_below(q12), rnd());
        // gs: a, b < 8q -> a < 16q, b < 4q
        auto gs = [&](u64 a, u64 b) {
            u64 x = a, y = b;
            ar.gs(x, y, W);
            REQUIRE(x < q16 && y < q4, "IntP::gs q=%llu a=%llu b=%llu -> %llu %llu", q, a, b, x, y);
            REQUIRE(x % q == (u64)(((u128)a + b) % q) && y % q == mulm((a % q + q - b % q) % q, w, q), "IntP::gs residue q=%llu a=%llu b=%llu", q, a, b);
            w_gs.see((double)x / q);
        };
        const u64 eg[] = {0, 1, q - 1, q, q + 1, fold_max, 4 * q, q8 - 2, q8 - 1};
        for (u64 a : eg) for (u64 b : eg) gs(a, b);
        for (int i = 0; i < 20000; i++) gs(rnd_below(q8), rnd_below(q8));
    }
    // fold_lh over the call sites' range (cf_sum above) and, as the struct's own contract, over L < 2^64, H < 2^63: result
    // below 2.07 2^60, the residue of L + H 2^60; plus the dropped limb's residue (< q) it is below 3.1 q, which three forward
    // stages take to 15.1 q < 16 q
    auto lh = [&](u64 L, u64 H) {
        const u64 r = ar.fold_lh(L, H);
        const u128 z = (u128)L + ((u128)H << 60);
        REQUIRE((u128)r * 100 < kTwo60 * 207 && r % q == (u64)(z % q), "IntP::fold_lh q=%llu L=%llu H=%llu -> %llu", q, L, H, r);
        REQUIRE((double)(r + (q - 1)) < 3.1 * (double)q, "IntP::fold_lh + q q=%llu", q);
        w_lh.see((double)r / q);
    };
    const u64 eL[] = {0, 1, q, (1ull << 60) - 1, 1ull << 60, (1ull << 63) - 1, 1ull << 63, ~0ull};
    const u64 Hmax_call = (1ull << 62) + (1ull << 33) - 1;
    std::vector<u64> eH = {0, 1, 0xFFFFFFFFull, 1ull << 32, Hmax_call, (1ull << 62) - 1, (1ull << 51) - 1, (1ull << 63) - 1};
    // H whose high word makes m1 mod 2^28 maximal (c is odd), with the low word all ones
    {
        const unsigned cinv = [&] { unsigned a = (unsigned)c, x = a; for (int i = 0; i < 5; i++) x *= 2 - a * x; return x; }();
        const u64 hw = (u64)((0x0FFFFFFFu * cinv) & 0x0FFFFFFFu);  // (hw c) mod 2^28 = 2^28 - 1
        for (u64 top : {0ull, 1ull << 28, 3ull << 28, 7ull << 28})
            if (((hw | top) << 32) < (1ull << 63)) eH.push_back(((hw | top) << 32) | 0xFFFFFFFFull);
    }
    for (u64 L : eL) for (u64 H : eH) lh(L, H);
    for (int i = 0; i < 200000; i++) lh(rnd(), rnd() >> 1);
    for (int ns : {4, 5}) {  // call-site sums
        const int ybits = ns == 5 ? 48 : 60;
        for (int i = 0; i < 100000; i++) {
            u64 y[5], f[5], L, H;
            for (int s = 0; s < ns; s++) {
                y[s] = i < 8 ? (1ull << ybits) - 1 - (u64)(i & 1) : rnd() >> (64 - ybits);
                f[s] = i < 8 ? q - 1 : rnd_below(q);
            }
            cf_sum(y, f, ns, L, H);
            REQUIRE((ns == 5 ? L < 9ull << 60 && H < (1ull << 51) : L < (1ull << 63) && H <= Hmax_call), "cf_sum range ns=%d L=%llu H=%llu", ns, L, H);
            w_L[ns - 4].see((double)L / (double)(1ull << 60));
            lh(L, H);
        }
    }
    // fold128 / canon128: ANY 128-bit z -> below 3.07 2^60 / canonical
    auto f128 = [&](u128 z) {
        const u64 r = ar.fold128(z);
        REQUIRE((u128)r * 100 < kTwo60 * 307 && r % q == (u64)(z % q), "IntP::fold128 q=%llu z=%llx%016llx -> %llu", q, (u64)(z >> 64), (u64)z, r);
        REQUIRE(ar.canon128(z) == (u64)(z % q), "IntP::canon128 q=%llu", q);
        w_128.see((double)r / q);
    };
    const u128 all = ~(u128)0;
    f128(0); f128(1); f128(q); f128(all); f128(all - 1); f128(all >> 1); f128((u128)1 << 127); f128(((u128)1 << 64) - 1);
    f128((u128)q * q); f128((u128)(q16 - 1) * (q - 1) * 4);
    {  // z >> 96 making t1 mod 2^28 maximal, every other bit set
        const unsigned c16 = (unsigned)c << 4;  // even: solve (z96 * (c16 >> 4)) mod 2^24 = 2^24 - 1 so t1 mod 2^28 = 2^28 - 16
        unsigned a = (unsigned)c, x = a;
        for (int i = 0; i < 5; i++) x *= 2 - a * x;
        const u64 z96 = (u64)((0x00FFFFFFu * x) & 0x00FFFFFFu);
        for (u64 top : {0ull, 0xFF000000ull})
            f128((((u128)(z96 | top)) << 96) | (((u128)0xFFFFFFFFull) << 64) | ~0ull);
        (void)c16;
    }
    for (int i = 0; i < 200000; i++) {
        u128 z = ((u128)rnd() << 64) | rnd();
        if (i < 128) z >>= i;
        f128(z);
    }
}

// -------------------------------------------------------------------------------------------------------------------------- FpA
static bool is_int(double x) { return std::rint(x) == x; }
// Largest |v| mulmod is fed, from the recentre placement of the two-pass transforms (ntt15.hip):
//   inverse (Gentleman-Sande: sums double, differences go through mulmod) runs 2 | 3 | 3 | 4 stages between the four reductions
//   (recentre_wide, recentre, recentre_wide, recentre) from canonical input, then fin_inv.  A run of k stages from magnitude m feeds
//   mulmod at most 2^k m.  Non-lean: max(2^2 q, 2^3 q/2, 2^4 q/2) = 8 q, and fin_inv 8 q.  Lean (both recentre_wide skipped): runs of
//   5 (from q) and 6 (from q/2) stages, 32 q; fin_inv 8 q.
//   forward (Cooley-Tukey, no reduction in 15 stages): b at stage k is below m0 + r_1 + ... + r_(k-1), m0 = 1.9 q (the column-fused
//   conversions' cf_fold plus the dropped limb), r_i the bound below at the magnitude reached — about 12 q for 45/46-bit primes and
//   14 q for the largest 47-bit ones.
// The quotient estimate rint(v y), y = fl(w / q) (or fl(w fl(1/q)) for tw8), is within |v| (w/q) 2u (3u) of v w / q, u = 2^-53, so
// |r| <= q/2 + |v| w 2u (3u).  That is <= 0.75 q (1.3 q) up to 32 q on the lean primes — the documented bound — but on a 47-bit
// prime v = 21 q already allows 0.83 q (0.99 q): the bound the comment states is the lean one.  Checked here: exactness always, the
// q/2 + |v| w k u bound for every prime, 0.75 q / 1.3 q for the lean ones, and that the forward magnitudes stay below 2^52.
static double rbound(double v_abs, double wq, bool t8) { return 0.5 + v_abs * wq * (t8 ? 3 : 2) * 0x1p-53; }  // |r| / q, wq = w / q
static void check_fpa(u64 q, int logn, Worst &w_mm, Worst &w_mm8, Worst &w_mm2, Worst &w_rc) {
    const ModC M = make(q);
    const FpA ar(M);
    const bool lean = ar.lean;  // the struct's own choice: a lean prime must meet the lean bounds at 32 q
    const double qd = (double)q;
    double mf = 1.9;  // forward magnitudes in units of q, tw8 bound at the largest twiddle (w < q)
    for (int st = 1; st < 15; st++) mf += rbound(mf * qd, 1.0, true);
    REQUIRE(mf * qd + rbound(mf * qd, 1.0, true) * qd < 0x1p52, "FpA forward headroom q=%llu (%.1f q)", q, mf);
    const double vq = lean ? 32.0 : std::max(8.0, std::ceil(mf));
    const i128 V = (i128)(vq * qd);
    REQUIRE(V < ((i128)1 << 52), "V");
    auto mm = [&](i128 v, u64 w, const FpA::TW W, bool t8) {
        const double vd = (double)v;
        REQUIRE((i128)vd == v, "v exact");
        const double r = ar.mulmod(vd, W);
        REQUIRE(is_int(r) && std::fabs(r) < 9007199254740992.0, "FpA::mulmod not an integer q=%llu v=%lld w=%llu", q, (long long)v, w);
        const i128 d = v * (i128)w - (i128)r;
        REQUIRE(d % (i128)q == 0, "FpA::mulmod residue q=%llu v=%lld w=%llu r=%.0f", q, (long long)v, w, r);
        const double rq = std::fabs(r) / qd, vabs = std::fabs(vd);
        REQUIRE(std::fabs(r) <= 0.5 * qd + vabs * ((double)w / qd) * (t8 ? 3 : 2) * 0x1p-53 * qd * (1 + 0x1p-40) + 1,
                "FpA::mulmod bound q=%llu v=%lld w=%llu%s r=%.0f (%.4f q)", q, (long long)v, w, t8 ? " tw8" : "", r, rq);
        REQUIRE(!lean || rq <= (t8 ? 1.3 : 0.75), "FpA::mulmod lean bound q=%llu v=%lld w=%llu%s r=%.0f (%.4f q)", q, (long long)v, w, t8 ? " tw8" : "", r, rq);
        (t8 ? w_mm8 : w_mm).see(rq);
    };
    for (u64 w : pick_twiddles(q, logn, 12)) {
        const FpA::TW W = make_double2((double)w, (double)w / qd), W8 = ar.tw8((double)w);
        auto both = [&](i128 v) {
            mm(v, w, W, false);
            mm(v, w, W8, true);
        };
        const i128 Q = q;
        for (i128 v : {(i128)0, (i128)1, Q - 1, Q, Q + 1, 2 * Q - 1, 2 * Q + 1, 8 * Q - 1, 8 * Q + 1, V - 1, V, V - Q + 1})
            both(v), both(-v);
        for (int i = 0; i < 4000; i++) {
            const i128 v = (i128)rnd_below((u64)(2 * V + 1)) - V;
            both(v);
        }
        // near-ties: v w / q within a few units of 1/q from k + 1/2 (and a little further out, where the estimate's error can reach),
        // at the largest magnitudes
        if (w > 1) {
            const u64 wi = modinv(w, q);
            for (int j = -24; j <= 24; j++) {
                const i128 num = (i128)(q / 2) + j * (i128)(q >> 8 > 0 ? 1 : 1) + (j > 4 ? (j - 4) * (i128)(q >> 10) : 0) - (j < -4 ? (-j - 4) * (i128)(q >> 10) : 0);
                const u64 vr = mulm(modq(num, q), wi, q);  // v w = num (mod q)
                for (i128 k = V / Q; k >= V / Q - 3; k--)
                    for (int sg : {1, -1}) {
                        const i128 v = (i128)vr + (sg > 0 ? (k - 1) : -k) * Q;
                        if (v <= V && v >= -V) both(v);
                    }
            }
        }
    }
    // mulmod2: canonical a, b -> |r| <= 0.55 q
    auto mm2 = [&](u64 a, u64 b) {
        const double r = ar.mulmod2((double)a, (double)b);
        REQUIRE(is_int(r) && ((i128)a * b - (i128)r) % (i128)q == 0, "FpA::mulmod2 residue q=%llu a=%llu b=%llu", q, a, b);
        REQUIRE(std::fabs(r) <= 0.55 * qd, "FpA::mulmod2 bound q=%llu a=%llu b=%llu r=%.0f", q, a, b, r);
        w_mm2.see(std::fabs(r) / qd);
    };
    const u64 ec[] = {0, 1, 2, q / 2, q / 2 + 1, q - 2, q - 1};
    for (u64 a : ec) for (u64 b : ec) mm2(a, b);
    for (int i = 0; i < 200000; i++) mm2(rnd_below(q), rnd_below(q));
    for (int i = 0; i < 20000; i++) {  // near-ties of a b / q
        const u64 b = q - 1 - rnd_below(q / 4), tgt = (q / 2 + rnd_below(64)) % q;
        mm2(mulm(tgt, modinv(b, q), q), b);
    }
    // recentre: integer |x| < 2^52 -> x - k q in [-(q+1)/2, (q+1)/2] (the quotient estimate may miss a near-tie by one)
    auto rc = [&](i128 x) {
        double v = (double)x;
        ar.recentre(v);
        REQUIRE(is_int(v) && (x - (i128)v) % (i128)q == 0 && std::fabs(v) <= (qd + 1) / 2, "FpA::recentre q=%llu x=%lld -> %.0f", q, (long long)x, v);
        w_rc.see(std::fabs(v) / qd);
    };
    const i128 X = ((i128)1 << 52) - 1, Q = q;
    for (i128 x : {(i128)0, (i128)1, Q / 2, Q / 2 + 1, Q - 1, Q, Q + 1, X, X - 1, (X / Q) * Q, (X / Q) * Q - 1, (X / Q) * Q + Q / 2, (X / Q) * Q - Q / 2 - 1})
        rc(x), rc(-x);
    for (int i = 0; i < 200000; i++) rc((i128)rnd_below((u64)(2 * X + 1)) - X);
    for (i128 k = X / Q; k > X / Q - 64 && k > 0; k--)
        for (int d = -3; d <= 3; d++) rc(k * Q + Q / 2 + d), rc(-(k * Q + Q / 2 + d));
    REQUIRE(lean == (q < (1ull << 45) + (1ull << 41)), "FpA::lean selection q=%llu", q);
    // u2d / d2u round trip on [0, 2^52)
    for (u64 x : {0ull, 1ull, q - 1, q, (1ull << 52) - 1, (1ull << 52) - 2, 1ull << 51})
        REQUIRE(FpA::d2u(FpA::u2d(x)) == x && FpA::u2d(x) == (double)x, "u2d/d2u x=%llu", x);
    for (int i = 0; i < 200000; i++) {
        const u64 x = rnd() >> 12;
        REQUIRE(FpA::d2u(FpA::u2d(x)) == x && FpA::u2d(x) == (double)x && ar.from_canon(x) == (double)x, "u2d/d2u x=%llu", x);
    }
    // fin_fwd: any integer |x| < 2^52 -> canonical residue; fin_inv: |x| <= 8 q (the last inverse run) times (sc, Shoup companion)
    for (int i = 0; i < 200000; i++) {
        const i128 x = i < 64 ? (i & 1 ? X : -X) - i / 2 : (i128)rnd_below((u64)(2 * X + 1)) - X;
        REQUIRE(ar.fin_fwd((double)x) == modq(x, q), "FpA::fin_fwd q=%llu x=%lld", q, (long long)x);
    }
    for (u64 sc : {1ull, q - 1, (u64)rnd_below(q), modinv(1ull << logn, q)}) {
        const u64 scs = (u64)((((u128)sc) << 64) / q);
        for (int i = 0; i < 50000; i++) {
            const i128 x = i < 16 ? (i & 1 ? 8 * Q : -8 * Q) - i / 2 : (i128)rnd_below((u64)(16 * Q + 1)) - 8 * Q;
            REQUIRE(ar.fin_inv((double)x, sc, scs) == mulm(modq(x, q), sc, q), "FpA::fin_inv q=%llu x=%lld sc=%llu", q, (long long)x, sc);
        }
    }
}

int main(int argc, char **argv) {
    struct Mod {
        u64 q;
        int logn;
        const char *why;
    };
    std::vector<Mod> mods;
    // IntP: every q = 2^60 - c, c < 2^24, prime and 1 mod 2N — at N = 2^15 all of them, at N = 2^11 the smallest and largest c
    for (int logn : {15, 11}) {
        std::vector<u64> ps;
        for (u64 c = (2ull << logn) - 1; c < (1ull << 24); c += 2ull << logn)
            if (is_prime((1ull << 60) - c)) ps.push_back((1ull << 60) - c);
        if (logn == 15) {
            REQUIRE(ps.size() == 8, "expected eight IntP primes at N = 2^15, found %zu", ps.size());
            for (u64 q : ps) mods.push_back({q, 15, "IntP 2^60-c"});
        } else {
            mods.push_back({ps.front(), 11, "IntP smallest c, N=2^11"});
            mods.push_back({ps.back(), 11, "IntP largest c, N=2^11"});
        }
    }
    const u64 step = 1ull << 16;  // N = 2^15: q = 1 mod 2^16
    auto prime_below = [&](u64 x) { u64 q = ((x - 2) / step) * step + 1; while (!is_prime(q)) q -= step; return q; };
    auto prime_above = [&](u64 x) { u64 q = (x / step + 1) * step + 1; while (!is_prime(q)) q += step; return q; };
    const u64 lean_edge = (1ull << 45) + (1ull << 41);
    mods.push_back({prime_below(lean_edge), 15, "FpA largest lean"});
    mods.push_back({prime_above(lean_edge), 15, "FpA smallest non-lean"});
    mods.push_back({prime_below(1ull << 46), 15, "FpA largest 46-bit"});
    mods.push_back({prime_below(1ull << 47), 15, "FpA largest 47-bit"});
    mods.push_back({prime_above(1ull << 30), 15, "FpA ~2^30"});
    mods.push_back({prime_above(1ull << 47), 15, "IntA smallest 48-bit"});
    mods.push_back({prime_below(1ull << 59), 15, "IntA largest 59-bit"});
    {
        u64 c = (1ull << 24) + step - 1;  // first 60-bit prime past the IntP rule
        while (!is_prime((1ull << 60) - c)) c += step;
        mods.push_back({(1ull << 60) - c, 15, "IntA 60-bit, c >= 2^24"});
    }
    for (int i = 1; i < argc; i++) mods.push_back({strtoull(argv[i], nullptr, 0), 15, "default chain"});

    Worst a_ct, a_gs, p_sh, p_ct, p_gs, p_lh, p_128, f_mm[2], f_mm8[2], f_mm2, f_rc;  // f_*[0] lean, [1] non-lean
    long deficit2 = 0;
    for (const Mod &m : mods) {
        REQUIRE(is_prime(m.q) && (m.q - 1) % (2ull << m.logn) == 0, "modulus %llu", m.q);
        const int k = arith_of(m.q);
        const bool lean = k == 0 && m.q < (1ull << 45) + (1ull << 41);
        if (k == 0) check_fpa(m.q, m.logn, f_mm[!lean], f_mm8[!lean], f_mm2, f_rc);
        if (k == 1) check_intp(m.q, m.logn, p_sh, p_ct, p_gs, p_lh, p_128, deficit2);
        if (k == 2) check_inta(m.q, m.logn, a_ct, a_gs);
        printf("%-5s q=%llu (%d bits", kName[k], m.q, bits(m.q));
        if (bits(m.q) == 60) printf(", c=0x%llx", (1ull << 60) - m.q);
        printf(") N=2^%d%s  [%s]\n", m.logn, k == 0 ? (lean ? " lean" : " non-lean") : "", m.why);
    }
    printf("worst IntA: ct max/q %.6f (< 4), gs max/q %.6f (< 2)\n", a_ct.v, a_gs.v);
    printf("worst IntP: shoup/q %.6f (< 4), ct/q %.6f (< 16), gs a/q %.6f (< 16), fold_lh/2^60 %.4f (< 2.07), fold128/2^60 %.4f (< 3.07); "
           "quotient two below exact in %ld shoup products\n",
           p_sh.v, p_ct.v, p_gs.v, p_lh.v, p_128.v, deficit2);
    printf("worst IntP conversion sums: L/2^60 %.4f (NS = 4, < 8), %.4f (NS = 5, < 9)\n", w_L[0].v, w_L[1].v);
    printf("worst FpA: mulmod |r|/q lean %.4f non-lean %.4f (<= 0.75), tw8 lean %.4f non-lean %.4f (<= 1.3), mulmod2 %.4f (<= 0.55), "
           "recentre %.4f (<= (q+1)/2)\n", f_mm[0].v, f_mm[1].v, f_mm8[0].v, f_mm8[1].v, f_mm2.v, f_rc.v);
    printf("ntt_arith ok (%ld checks, %zu moduli)\n", g_checks, mods.size());
    return 0;
}
