// image_matching_amd/csrc/kernels.h — launch interface of the gfx950 kernels (kernels.hip, client_kernels.hip).
//
// Data layout everywhere: limb-major uint64 residues, [batch][poly][limb][N] contiguous, evaluation form in
// bit-reversed order (out[j] = a(psi^{2*bitrev(j)+1})) unless a comment says "coefficient form".  One wave reads 64
// (or 128) consecutive coefficients of ONE limb, so the modulus constants are wave-uniform (SGPRs).
#pragma once
#include <hip/hip_runtime.h>
#include "devmath.h"

// which modulus each limb slot of a buffer uses
struct LimbSel {
    int n;
    int mod[HY_MAX_MODS];
};

struct NttTables {
    const u64 *tw, *tw_sh;    // [nT][N] psi^{bitrev(k)} and Shoup companions
    const u64 *itw, *itw_sh;  // [nT][N] psi^{-bitrev(k)}
    const ModC *mod;          // [nT]
    const ulonglong2 *twp, *itwp;  // the same tables interleaved as (w, w_shoup) pairs: one 16-byte load per twiddle
    const ulonglong2 *twf, *itwf;  // bit patterns of double pairs (w, w / q) for the FP64 path of the <= 47-bit primes
    const double *twd, *itwd;      // [nT][N] the twiddles alone as doubles (8 bytes each): the one-pass kernel's per-lane twiddle loads
    unsigned fp_mask;              // host copy of the kernels' own rule: bit m set <=> modulus m takes the FP64 path
    unsigned pm_mask;              // bit m set <=> modulus m = 2^60 - c with c < 2^24 takes the lazy pseudo-Mersenne integer path (IntP)
    // launch-shape switches, read from the environment ONCE per context (host side only; the parity tests build one context per variant)
    int one_pass;                  // HYDIA_NTT_1PASS: 0 off (default), 1 every FP64 transform, 2 ("plain") only transforms without fused prologue / epilogue
    int one_pass_min;              // HYDIA_NTT_1PASS_MIN: smallest launch (limb-polynomials) that takes the one-pass kernel (default 1024)
    int two_ip_launches;           // HYDIA_RELIN_TWO_IP_LAUNCHES: Q and special-prime halves of the fused inner product as two launches
    int ip_group;                  // HYDIA_IP_GROUP: ciphertexts per interleaving group of the merged inner-product kernel (default 8)
    int int_epilogue;              // HYDIA_INT_EPILOGUE: merged ModDown + Rescale epilogue in integers for every limb (round 3's form)
    int no_drop_in_ip;             // HYDIA_NO_DROP_IN_IP: the dropped limb's inverse pass 2 as its own launch (round 3's form)
    int no_tw_lds;                 // HYDIA_NO_TW_LDS: pass 2's phase A / B twiddles of the FP64 limbs as per-lane vector loads (round 4's form) instead of a wave-local LDS table
    int p2_wg_sync;                // HYDIA_P2_WG_SYNC: the plain N = 2^15 transforms through round 4's workgroup-synchronous pass 2 (parity variant)
    int cf_wide;                   // HYDIA_COLFUSE_WIDE: round 4's column-fused kernel (32-column tiles, 16 rows per lane, two workgroups per CU)
    int generic;                   // HYDIA_NTT_GENERIC: the ring-size-generic transform kernels also at N = 2^15 and 2^16 (parity variant)
    int ntt16;                     // HYDIA_NTT16=1: the plain transforms at N = 2^16 through k_ntt16_p1 / p2 (ntt16.hip) — opt-in until measured
};

// base conversion table: out[t] = sum_s y[s] * f[s][t] mod q_{dst t}
struct ConvTab {
    int ns, nt;
    int skip_lo, skip_hi;  // target slots in [skip_lo, skip_hi) are left untouched (the digit's own limbs)
    u64 f[HY_MAX_DIGIT][HY_MAX_MODS];
};

struct ScaleSel {  // per-limb multiplier applied by the inverse NTT's last pass (N^{-1} * extra)
    u64 s[HY_MAX_MODS], s_sh[HY_MAX_MODS];
};

#define HY_LC_TERMS 8
#define HY_LC_LIMBS 16
// linear combination of up to 8 ciphertext batches with per-limb constants (Chebyshev / f4 leaves)
struct LinComb {
    int nterms;
    const u64 *src[HY_LC_TERMS];
    int ls[HY_LC_TERMS];                   // limb stride of each source
    u64 c[HY_LC_TERMS][HY_LC_LIMBS];       // constant residues per (term, limb)
    u64 cs[HY_LC_TERMS][HY_LC_LIMBS];      // Shoup companions
    u64 c0[HY_LC_LIMBS];                   // constant added to polynomial 0
};

// K linear combinations of the SAME terms in one pass (the Paterson-Stockmeyer leaves share T_1..T_7): every term is read
// once, K outputs are written.  tab (device): K blocks of [HY_LC_TERMS][HY_LC_LIMBS] constants followed by [HY_LC_LIMBS] c0.
struct LinCombMulti {
    int nterms, K;
    int fp;               // limbs below 2^47 on the FP64 pipe (HYDIA_NTT_INT turns it off: 128-bit integer sums everywhere)
    const u64 *src[HY_LC_TERMS];
    int ls[HY_LC_TERMS];
    const u64 *tab;
};
#define HY_LCM_BLOCK (HY_LC_TERMS * HY_LC_LIMBS + HY_LC_LIMBS)

// Fused prologue of the N = 2^15 forward NTT's first pass: where the coefficient-form input comes from
struct NttLoad {
    int mode;             // 0 plain (src), 2 rescale spread from `y`
    const u64 *y;         // mode 2: [x][N] last limb, coefficient form
    size_t y_outer;       // elements between consecutive x
    int l;                // mode 2: index of the dropped modulus q_l
};
// Fused epilogue of its second pass: what is done with the evaluation-form value v of limb j
// store mode 4: the forward transform's results are consumed by the key-switching inner product instead of being stored —
// a workgroup transforms limb t of EVERY digit that has to be extended to it, multiplies by the key and writes acc only
// A ct x ct product whose tensor is formed where it is consumed (round 4) instead of by k_tensor: d0 = a0 b0, d1 = a0 b1 + a1 b0 go into
// the merged ModDown + Rescale epilogue (and the dropped limb's tail), d2 = a1 b1 into the load of the relinearisation's inverse
// transform — the degree-2 ciphertext [x][3][nl][N] never exists in HBM (7 limb-polynomials of traffic per limb and ciphertext and
// one launch less per product).  a, b: [x][2][..][N] views, limb j of polynomial p of ciphertext x at a + x a_x + p a_p + j N.
// Optionally minus kap c on d0, d1 (a Chebyshev step 2ab - K c: kap = K/2 mod q_j — per limb in NttStore::kap, at the dropped limb here).
struct ProdSrc {
    const u64 *a, *b;
    size_t a_x, a_p, b_x, b_p;
    const u64 *c;  // null: a plain product
    size_t c_x, c_p;
    u64 kap_l, kap_l_sh;  // kap at the limb the rescale drops (the tail's addend)
};
struct IpArgs {
    const u64 *key;   // [nd][2][nT][N]
    const u64 *const *keys;  // non-null (device array): ciphertext x takes keys[x] instead (giant-step rotations: one key per giant step)
    int nT, nE, nl, alpha;
    int own;          // 1: limbs t < nl also take their own digit's residues (evaluation form) from c2
    const u64 *c2;    // [x][..][N] the polynomial being key-switched, limb t at c2 + x*c2_xs + t*N
    size_t c2_xs;
    u64 *acc;         // [x][2][nE][N]
    // special-prime limbs only (kernel variant TAIL): the two sums do not go to acc but straight through the first pass of their
    // inverse transform; its raw image lands in row inv_row0 + (t - nl) of polynomial 2x + {0,1} of inv_out
    u64 *inv_out;
    size_t inv_outer;  // elements per polynomial of inv_out
    int inv_row0;
    // merged ModDown + Rescale (round 4): the Q limb drop_l (the limb the rescale drops; -1 = none) takes the tail as well — its two
    // sums become the dropped limb of the would-be ModDown output, (sum drop_mul + drop_add[x, p, drop_l])(x2), and go through the first
    // pass of the inverse transform into row inv_row0 - 1; nothing of that limb reaches acc (nobody reads it)
    int drop_l, drop_dbl;
    u64 drop_mul, drop_mul_sh;
    const u64 *drop_add;  // [x][p][..][N]: + drop_add[x*drop_add_x + p*drop_add_p + drop_l*N + c]
    size_t drop_add_x, drop_add_p;
    int drop_has_prod;    // the addend is the product's d_p at that limb, formed from drop_prod (drop_add unused)
    ProdSrc drop_prod;
};
struct DropLimb {  // host side of the same (ntt15_p2_inner_product)
    int l, dbl;
    u64 mul, mul_sh;
    const u64 *add;
    size_t add_x, add_p;
    const ProdSrc *prod;  // non-null: the addend is a product's d_p (add unused)
};
// store mode 5 = mode 1 whose `in` operand (the key-switching accumulator of the Q limbs) is never materialised: the epilogue forms
// sum_d dig[d][j][c] * key_x[d][p][j][c] itself from the shared digits (L2-resident) and rotation x's key (loop A)
struct LoopAIp {
    const u64 *const *keys;  // device array: key of rotation x (packed when packed_nQ > 0, else [nd][2][nT][N] u64)
    const u64 *dig;          // [nd][dig_rows][N], shared by every x
    int nd, dig_rows, nT, packed_nQ;
    int key_row0, dig_row0;  // limb slot s of the launch <-> key row key_row0 + s, digit row dig_row0 + s (0, 0 for the Q limbs;
                             // nQ, nl for the special-prime limbs whose sums enter the ModDown inverse transform directly)
    int fp;                  // primes below 2^47: products on the FP64 pipe (bit-identical; HYDIA_LOOPA_INT_IP turns it off)
    int premul;              // keys (Q-limb rows) and the converted rows already carry P^{-1}: the combine is a plain subtraction
    int limb_fastest;        // HYDIA_LOOPA_LIMB_FASTEST: round 4's workgroup order in the last pass (limbs fastest instead of rotations)
    int raw_fp;              // (set at launch) fp && premul: the epilogue takes the FP64 sums unreduced and reduces once (p2_finish5_fp)
};
struct NttStore {
    int mode;             // 0 plain (dst in place), 1 ModDown combine, 2 rescale combine, 3 merged ModDown + rescale, 4 inner product, 5 see LoopAIp
    u64 *out;             // modes 1,2: destination, compact [xp][nl][N]
    int nl;               // limbs of `out`
    const u64 *in;        // mode 1: acc [xp][in_ls][N] (Q limbs first); mode 2: ciphertext being rescaled [xp][in_ls][N]
    int in_ls;
    ScaleSel mul;         // mode 1: P^{-1} mod q_j; mode 2: q_l^{-1} mod q_j   -> out = (in - v) * mul
    ScaleSel mul2;        // mode 3: q_l^{-1} mod q_j:  out = ((in * mul + addend)(x2) - v) * mul2 (- sub)(+ addc)
    const u64 *addend;    // mode 1: + addend[x*add_x + p*add_p + j*N + c] for p < add_polys (xp = 2x + p)
    size_t add_x, add_p;
    int add_polys;
    int dbl;              // mode 1: result doubled (Chebyshev recurrences 2ab - c)
    const unsigned *ginv; // mode 1: scatter through the automorphism: out index = perm_{ginv[x]}(c); null = identity
    int same_g;
    const u64 *sub;       // mode 2: - sub[xp*sub_ls*N + j*N + c]
    int sub_ls;
    int sub_add;          // mode 3: the `sub` operand is ADDED instead (Paterson-Stockmeyer  Q*T_g + R)
    int has_addc;         // mode 2: + addc[j] on polynomials with xp % npoly == 0
    int npoly;
    u64 addc[HY_LC_LIMBS];
    int has_prod;         // mode 3: the addend is d_p of the product `prod` (addend unused); inverse load mode 8: the input is d2 = a1 b1 of `prod`
    ScaleSel kap;         //         prod.c != null: d_p -= kap[j] c_p
    ProdSrc prod;         //         (mode 8 also writes d2 to `out`, compact [x][nl][N], for the inner product's own-digit rows)
    int int_epilogue;     // mode 3: integer (Shoup) epilogue for every limb (HYDIA_INT_EPILOGUE; default: FP64 for the limbs below 2^47)
    IpArgs ip;            // mode 4
    LoopAIp la;           // mode 5
};


// Column-fused conversion (k_ntt15_colfuse, N = 2^15): inverse pass 1' of up to 4 source limbs (+ the dropped limb of a merged
// ModDown + Rescale), fast base conversion, forward pass 1 of up to 16 target limbs — all on ONE 32-column tile of the 128 x 256
// coefficient matrix, sources held in registers, so the coefficient-form rows never exist in HBM.  One entry describes one
// (sources -> targets) map: a ModDown, or one digit of a ModUp.
#define HY_CF_SRC 4       // conversion sources of the default kernels (a digit of alpha = 4 limbs; the reference's four special primes)
#define HY_CF_SRC_MAX 5   // round 5: a FIFTH source for ModDown maps over five special primes below 2^48 (k_ntt15_colfuse8<*, 5>; secondary figure)
#define HY_CF_TGT 16
struct ColFuse {
    int nk, nt;                  // conversion sources, targets
    int mdr;                     // 1: merged ModDown + Rescale — an extra source `u` (modulus l) whose centred residue is added to every target
    int l;                       // mdr: modulus id of the dropped limb
    int smod[HY_CF_SRC_MAX], srow[HY_CF_SRC_MAX];  // modulus id / row (in src, per polynomial) of each conversion source
    int umod, urow;                        // mdr: the same for u
    u64 ssc[HY_CF_SRC_MAX], ssc_sh[HY_CF_SRC_MAX]; // final multiplier of each source's inverse transform (N^{-1} x conversion factor)
    u64 usc, usc_sh;
    int tmod[HY_CF_TGT], trow[HY_CF_TGT];  // modulus id / row (in dst, per polynomial) of each target
    u64 f[HY_CF_SRC_MAX][HY_CF_TGT];           // conversion constants: target t = sum_k y_k f[k][t] mod q_tmod[t]
    u64 fl[HY_CF_SRC_MAX];                     // mdr: constants of the dropped limb, y_l = u - sum_k y_k fl[k] mod q_l
    u64 t60[HY_CF_TGT];                    // 2^60 mod q_tmod[t] (the FP64 fold of the conversion sums; filled by cf_plan_store)
    ModC sM[HY_CF_SRC_MAX], uM, lM;            // the same for the sources, u and the dropped limb
    ModC tM[HY_CF_TGT];                    // the targets' modulus constants (a copy of NttTables::mod[tmod[t]], filled by cf_plan_store): a
                                           // target's constants then come with ONE batch of scalar loads off the map instead of a chain of
                                           // dependent ones (tmod -> mod[] -> kind -> tables) at the head of every target
};

#include "db_layout.h"  // DbLayout, db_limb_offset, db_offset (host-checkable: tests/csrc/db_layout_check.cpp)

// ---- device helpers shared by kernels.hip and ntt15.hip: 48-bit packed residues (database, rotation keys of loop A)
#if defined(__HIPCC__)
template <bool PK, bool NT>
DEV ulonglong2 db_load2(const unsigned char *p) {  // two consecutive residues
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u3 __attribute__((ext_vector_type(3), aligned(4)));
    if (!PK) {
        const ull2 v = NT ? __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(p)) : *reinterpret_cast<const ull2 *>(p);
        ulonglong2 r;
        r.x = v.x;
        r.y = v.y;
        return r;
    }
    const u3 w = NT ? __builtin_nontemporal_load(reinterpret_cast<const u3 *>(p)) : *reinterpret_cast<const u3 *>(p);
    ulonglong2 r;
    r.x = (u64)w.x | ((u64)(w.y & 0xFFFFu) << 32);
    r.y = (u64)(w.y >> 16) | ((u64)w.z << 16);
    return r;
}

// the same in two steps — the raw load (what stays in flight) and the unpacking (where the value is used).  (Two explicit
// specialisations: a typedef's alignment does not survive being a template argument, and the 12-byte loads are only 4-byte aligned.)
template <bool PK>
struct DbRaw;
template <>
struct DbRaw<true> {
    typedef unsigned int u3 __attribute__((ext_vector_type(3), aligned(4)));
    u3 w;
    template <bool NT>
    DEV void load(const unsigned char *p) {
        w = NT ? __builtin_nontemporal_load(reinterpret_cast<const u3 *>(p)) : *reinterpret_cast<const u3 *>(p);
    }
    DEV ulonglong2 get() const {
        ulonglong2 r;
        r.x = (u64)w.x | ((u64)(w.y & 0xFFFFu) << 32);
        r.y = (u64)(w.y >> 16) | ((u64)w.z << 16);
        return r;
    }
};
template <>
struct DbRaw<false> {
    typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
    ull2 w;
    template <bool NT>
    DEV void load(const unsigned char *p) {
        w = NT ? __builtin_nontemporal_load(reinterpret_cast<const ull2 *>(p)) : *reinterpret_cast<const ull2 *>(p);
    }
    DEV ulonglong2 get() const {
        ulonglong2 r;
        r.x = w.x;
        r.y = w.y;
        return r;
    }
};

// packed key layout (loop A's rotation keys): per (digit, poly) one row set — modulus 0 as N 8-byte residues, the nQ-1 scaling
// moduli (< 2^48) as N 6-byte residues each, then the nP special moduli as N 8-byte residues.  -17 % of the 12 GiB key stream.
HD size_t key_limb_offset(int N, int nQ, int m) {
    return m == 0 ? 0 : (m < nQ ? (size_t)N * 8 + (size_t)(m - 1) * N * 6 : (size_t)N * 8 + (size_t)(nQ - 1) * N * 6 + (size_t)(m - nQ) * N * 8);
}
HD size_t key_set_bytes(int N, int nQ, int nT) { return key_limb_offset(N, nQ, nT); }
#endif

namespace hk {
// ---- byte ledger (measurement): when enabled, every launcher below records the bytes its launch has to move (operands read +
// results written, each once; shared operands that stay in L2 — key tiles, twiddles, digits of loop A — are not counted) under the
// kernel's name, so that tools/kernel_rooflines.py can put a GB/s figure next to EVERY kernel of a query
void ledger_enable(bool on);
void ledger_add(const char *kernel, double bytes);
size_t ledger_dump(char *out, size_t cap);  // "kernel\tlaunches\tbytes\n" per line; returns the size needed

// plain: a plain gallery, one polynomial per entry (DbLayout::plain)
DbLayout db_layout(int N, int nQ, int packed, bool plain = false);                                 // ciphertext-major
DbLayout db_layout_seq(int N, int nQ, int packed, int bd, int blocks, int bpp, int nw, bool bits46 = false, bool plain = false);  // group-sequential when it applies
// ciphertexts t0 .. t0+X-1 of the database at `db` <-> plain [X][np][nQ][N] residues, np = db_polys(L)
void db_pack(hipStream_t st, int N, int nQ, const u64 *plain, void *db, size_t t0, int X, const DbLayout &L);
void db_unpack(hipStream_t st, int N, int nQ, u64 *plain, const void *db, size_t t0, int X, const DbLayout &L);
// ciphertexts t0 .. t0+X-1 of the database += plain [X][2][nQ][N] residues mod q_j, in place (db_accum.h; mod = the context's table);
// a plain gallery (L.plain): plaintexts t0 .. t0+X-1 += plain [X][nQ][N], through k_plain_db_accumulate / k_plain_db_accumulate46
void db_accumulate(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *plain, void *db, size_t t0, int X, const DbLayout &L);
// loading a plain gallery: *flag := 1 when a residue of plain [X][nQ][N] is at or above its modulus (never cleared here)
void db_check_canonical(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *plain, int X, unsigned *flag);
// re-keying (Context::db_rekey): polynomial 1 of ciphertexts t0 .. t0+X-1 -> out [X][nQ][N] residues (the key switch's operand), and the
// key switch's output ks [X][2][nQ][N] back in place: (c0, c1) := (c0 + ks0 mod q_j, ks1)
void db_gather_poly(hipStream_t st, int N, int nQ, u64 *out, const void *db, size_t t0, int X, const DbLayout &L);
void db_rekey_store(hipStream_t st, const ModC *mod, int N, int nQ, const u64 *ks, void *db, size_t t0, int X, const DbLayout &L);
// blocks per wave / waves per workgroup loop B uses for G blocks (bpp, nw = the context's caps)
void tensor_split(int G, int bpp, int nw, int *B, int *W);

// ---- NTT: X limb-polys of N coefficients; element (x, slot) lives at base + x*outer + slot*N, slot < sel.n
void ntt_forward(hipStream_t st, const NttTables &T, int logN, const u64 *src, u64 *dst, size_t src_outer,
                 size_t dst_outer, int X, const LimbSel &sel);
void ntt_inverse(hipStream_t st, const NttTables &T, int logN, const u64 *src, u64 *dst, size_t src_outer,
                 size_t dst_outer, int X, const LimbSel &sel, const ScaleSel &scale);

// N = 2^16 register-radix plain transforms (ntt16.hip); ntt_forward / ntt_inverse dispatch to them when logN == 16 and NttTables::ntt16 is set
void ntt16_forward(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer, int X,
                   const LimbSel &sel);
void ntt16_inverse(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer, int X,
                   const LimbSel &sel, const ScaleSel &scale);
// N = 2^15 register-radix fast path (ntt15.hip); ntt_forward / ntt_inverse dispatch to it when logN == 15
void ntt15_forward(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer, int X,
                   const LimbSel &sel);
// inverse transform whose INPUT is loop A's inner product over the limbs of sel (formed in the first pass's load, never in HBM)
void ntt15_inverse_loop_a(hipStream_t st, const NttTables &T, u64 *dst, size_t dst_outer, int X, const LimbSel &sel,
                          const ScaleSel &scale, const LoopAIp &la, bool p1 = true);
void ntt15_inverse(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer, int X,
                   const LimbSel &sel, const ScaleSel &scale);
// forward transform with fused prologue / epilogue; dst is the [X][sel.n][N] scratch between the passes
void ntt15_forward_fused(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer,
                         int X, const LimbSel &sel, const NttLoad &ld, const NttStore &stp);

// ---- element-wise over [X][sel.n][N]
// XP polynomials; operand t's polynomial xp starts at xp * t_ls * N (limb-strided views of dropped ciphertexts)
void add(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int XP, const LimbSel &sel, int a_ls,
         int b_ls, int o_ls);
void sub(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int XP, const LimbSel &sel, int a_ls,
         int b_ls, int o_ls);
// cross-shard membership reduction (multi-GPU): o = a + b as plain 64-bit integers, then every value -> its canonical residue
void add_raw(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int XP, const LimbSel &sel, int a_ls,
             int b_ls, int o_ls);
void mod_reduce(hipStream_t st, const ModC *mod, int N, u64 *a, int XP, const LimbSel &sel, int a_ls);
void mul_scalar(hipStream_t st, const ModC *mod, int N, const u64 *a, u64 *o, int XP, const LimbSel &sel,
                const ScaleSel &c, int a_ls, int o_ls);  // o = a * c[slot]
void add_scalar(hipStream_t st, const ModC *mod, int N, u64 *a, size_t outer, int X, const LimbSel &sel,
                const ScaleSel &c);  // a[x][slot] += c[slot]  (first sel.n slots of each outer block)
void copy_limbs(hipStream_t st, int N, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer, int X,
                int nlimbs);
// o[x][p][j] = sum_t src_t[x][p][j] * c[t][j] (+ c0[j] on p = 0): X cts of npoly polys, nl limbs, compact output
void lincomb(hipStream_t st, const ModC *mod, int N, const LinComb &lc, u64 *o, int X, int npoly, int nl);
// o[p][j] = sum_x in[x][p][j] mod q_j: EvalAdd chain over a batch (HERS sums its 512 per-dimension products); o compact
// out[k][x][p][j][c] = sum_t tab[k][t][j] * src_t[x][p][j][c] (+ c0[k][j] on polynomial 0)
void lincomb_multi(hipStream_t st, const ModC *mod, int N, const LinCombMulti &lc, u64 *o, int X, int npoly, int nl);
// stride / nout: output m (m < nout) = sum over x of ciphertext m + x * stride (the giant-major partial sums of the BSGS mat-vec)
void batch_sum(hipStream_t st, const ModC *mod, int N, const u64 *in, u64 *o, int X, int npoly, int nl, int stride = 1, int nout = 1);
// (a0 b0, a0 b1 + a1 b0, a1 b1) for X ciphertext pairs at nl limbs; o: [X][3][nl][N]
void tensor(hipStream_t st, const ModC *mod, int N, const u64 *a, const u64 *b, u64 *o, int X, int nl, int a_ls, int b_ls,
            const u64 *c = nullptr, int c_ls = 0, const ScaleSel *kap = nullptr);
// EvalSquare (approach 2's alpha norm): (a0^2, 2 a0 a1, a1^2) for X ciphertexts at nl limbs, a a limb-strided view; o: [X][3][nl][N].
// The residues tensor(a, a) gives, with half the loads
void tensor_sq(hipStream_t st, const ModC *mod, int N, const u64 *a, u64 *o, int X, int nl, int a_ls);
// approach 1's query-broadcast product: ONE 2-component ciphertext q ([2][q_ls][N]) times X ciphertexts b ([X][2][b_ls][N], e.g. the
// row-packed resident database read in place) -> o [X][3][nl][N]; the residues k_tensor gives for X copies of q
void tensor_bcast(hipStream_t st, const ModC *mod, int N, const u64 *q, int q_ls, const u64 *b, int b_ls, u64 *o, int X, int nl);
// approach 3's fused sum of products: K query ciphertexts q ([K][2][q_ls][N]) times the K chunk ciphertexts of each of X matrices b
// ([X][K][2][b_ls][N], e.g. the chunk-packed resident database read in place) -> o [X][3][nl][N], o[x] = sum_c q[c] (x) b[x][c]; the
// residues K tensor products summed with add give.  K <= 32 (the 128-bit lazy sums hold 64 products on the 60-bit limb)
void tensor_dot(hipStream_t st, const ModC *mod, int N, const u64 *q, int q_ls, const u64 *b, int b_ls, u64 *o, int X, int K, int nl);

// ---- key switching
// out[x][t][c] = sum_s y[x][s][c] * tab.f[s][t] mod q_{dsel.mod[t]} ; y coefficient form, residues < 2^60
void base_convert(hipStream_t st, const ModC *mod, int N, const u64 *y, size_t y_outer, u64 *out, size_t out_outer,
                  int X, const ConvTab &tab, const LimbSel &dsel);
// ModUp of every digit in one launch: y [X][nl][N] (coefficient form, digit d = rows [d_tabs[d].skip_lo, skip_hi)) ->
// out [X][nd][nE][N], rows of a digit's own limbs untouched; d_tabs: nd tables in device memory
void base_convert_digits(hipStream_t st, const ModC *mod, int N, const u64 *y, size_t y_outer, u64 *out, size_t out_outer, int X,
                          const ConvTab *d_tabs, int nd, int nl, int nE, const LimbSel &esel);
// acc[x][p][t][c] = sum_d dig[(x*dig_x_stride) + d][t][c] * key_x[d][p][mod(t)][c];  keys[x] -> [dnum][2][nT][N]
// (same_key: every x uses keys[0])
void inner_product(hipStream_t st, const ModC *mod, int N, const u64 *dig, size_t dig_x_stride, int nd,
                   const u64 *const *keys, int same_key, int nT, u64 *acc, int X, const LimbSel &esel,
                   const u64 *own = nullptr, size_t own_x_stride = 0, int alpha = 1, int nl = 0, int acc_rows = 0, int packed_nQ = 0,
                   int dig_rows = 0 /* rows per digit in dig; default acc_rows */, int dig_t0 = 0 /* digit row of acc row 0 */);
// packed evaluation keys (loop A): 45/46-bit limbs as 6-byte residues; packed_nQ > 0 tells inner_product that keys[] are packed
size_t key_packed_bytes(int N, int nQ, int nT, int nd);
// premul (optional): per-modulus factor applied to the Q-limb rows while packing (P^{-1} mod q_j for the fused loop A)
void key_pack(hipStream_t st, const ModC *mod, int N, int nQ, int nT, int nd, const u64 *key, void *out, const ScaleSel *premul = nullptr);
// the two halves of ntt15_inverse on their own (the fused key-switching tail runs the first pass of some rows elsewhere)
void ntt15_inverse_p2(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t src_outer, size_t dst_outer, int X, const LimbSel &sel);
void ntt15_inverse_p1(hipStream_t st, const NttTables &T, u64 *dst, size_t dst_outer, int X, const LimbSel &sel, const ScaleSel &scale);
// inverse pass 2 of d2 = a1 b1 of a product (formed in the load; also stored to d2_out, compact [X][sel.n][N])
void ntt15_inverse_p2_prod(hipStream_t st, const NttTables &T, const ProdSrc &ps, u64 *dst, size_t dst_outer, int X, const LimbSel &sel, u64 *d2_out);
void ntt15_inverse_p2_last_limb(hipStream_t st, const NttTables &T, const u64 *acc_l, u64 *dst, size_t src_outer, size_t dst_outer, int XP, int l,
                                u64 pinv, u64 pinv_sh, const u64 *addend, size_t add_x, size_t add_p, int dbl);
// second pass of the ModUp forward transforms fused with the inner product (N = 2^15): dig holds pass-1 output of every
// extended limb [x][nd][nE][N]; acc[x][2][nE][N] = sum_d NTT(dig[x][d][t]) * key[d][.][t]  (+ own-digit limbs from c2).
// inv_out != nullptr: the special-prime rows skip acc (see IpArgs)
// returns true when the launch also produced the dropped limb's inverse-pass-2 image (`drop` given and the merged kernel ran)
bool ntt15_p2_inner_product(hipStream_t st, const NttTables &T, const ModC *mod, const u64 *dig, size_t dig_x_stride, int nd, int X,
                            int nl, int nP, int nT, int alpha, const u64 *const *keys, const u64 *key, const u64 *c2, size_t c2_xs, u64 *acc,
                            u64 *inv_out = nullptr, size_t inv_outer = 0, int inv_row0 = 0, const DropLimb *drop = nullptr, bool per_x_keys = false);
void ntt15_forward_p1(hipStream_t st, const NttTables &T, const u64 *src, u64 *dst, size_t so, size_t dso, int X, const LimbSel &sel);
// second pass alone, in place on pass-1 output (plain store)
void ntt15_forward_p2(hipStream_t st, const NttTables &T, u64 *dst, size_t dso, int X, const LimbSel &sel);
void ntt15_forward_p2_fused(hipStream_t st, const NttTables &T, u64 *dst, size_t dso, int X, const LimbSel &sel, const NttStore &stp);
// column-fused conversion: src [XP][..][N] holds the raw image of the sources' inverse pass 2', dst [XP][..][N] receives the raw
// pass-1 image of the targets (pass 2 finishes it).  d_cf: ncf maps in device memory (h_cf: host copy), map z serves every polynomial
// pre: src holds the sources' canonical coefficient-form residues (inverse transform already complete) — the form small launches
// take (ntt15_colfuse_small): their inverse transform runs as its own, wider launch and the fused kernel keeps a short serial chain
void ntt15_colfuse(hipStream_t st, const NttTables &T, const u64 *src, size_t so, u64 *dst, size_t dso, int XP, const ColFuse *d_cf,
                   const ColFuse *h_cf, int ncf, bool pre = false);
bool ntt15_colfuse_small(int XP, int ncf);
// inverse pass 1' of a small launch on 16-column tiles (colfuse.hip k_ntt15_p1inv8), in place on dst; returns false when the launch is large
// (or HYDIA_COLFUSE_WIDE): the caller then launches the 32-column kernel
bool ntt15_inverse_p1_narrow(hipStream_t st, const NttTables &T, u64 *dst, size_t dso, int X, const LimbSel &sel, int slot0, int nsl, const ScaleSel &scale);
// out[x][p][j][c'] = ((acc[x][p][j][c] - conv[x][p][j][c]) * pinv[j] + (addend ? addend[x*add_x + p*add_ps + j*N + c] : 0)),
// c = perm_g(c') when galois[x] != 1 (evaluation-form automorphism), acc rows have stride acc_limbs*N
void moddown_combine(hipStream_t st, const ModC *mod, int logN, const u64 *acc, int acc_limbs, const u64 *conv,
                     const u64 *addend, size_t add_x_stride, size_t add_poly_stride, int add_polys, u64 *out, int X, int nl,
                     const ScaleSel &pinv, const unsigned *galois /* device [X] (or [1] with same_g) or null */,
                     int same_g, const u64 *self = nullptr, size_t self_x_stride = 0, size_t self_poly_stride = 0);
// merged ModDown + Rescale (bit-identical to doing them in sequence), coefficient-domain part.
// u  [xp][N]      : INTT of (acc_l P^{-1} + d_l)(x2), the dropped limb q_l of the would-be ModDown output
// y  [xp][nP][N]  : INTT of acc's P limbs times (P/p_k)^{-1}
// w  [xp][l][N]   : (conv_j P^{-1})(x2) + centred(y_l) mod q_j, whose NTT is subtracted in the pass-2 epilogue (mode 3)
void moddown_rescale_conv(hipStream_t st, const ModC *mod, int N, const u64 *y, size_t y_outer, const u64 *u, size_t u_outer, u64 *w, int XP,
                          int l, int nP, const ConvTab &tab /* f[s][j] = (P/p_s) P^{-1} (x2) mod q_j, j <= l */);
// u[xp*u_outer + c] = (acc[xp][l][c] * pinv_l + addend[x*add_x + p*add_p + l*N + c])(x2)   (evaluation form, limb l; u may be acc's row l)
void moddown_last_limb(hipStream_t st, const ModC *mod, int N, const u64 *acc, int acc_limbs, const u64 *addend, size_t add_x,
                       size_t add_p, u64 *u, size_t u_outer, int XP, int l, u64 pinv, u64 pinv_sh, int dbl);
// rescale: t = last limb in coefficient form [X][N]; tmp[x][j][c] = centred t mod q_j (coefficient form)
void rescale_spread(hipStream_t st, const ModC *mod, int N, const u64 *t, u64 *tmp, int X, int l);
// out[x][j][c] = (in[x][j][c] - tmp[x][j][c]) * qlinv[j]; in has nl=l+1 limbs per x, out has l
void rescale_combine(hipStream_t st, const ModC *mod, int N, const u64 *in, const u64 *tmp, u64 *out, int X, int l,
                     const ScaleSel &qlinv, int in_ls);

// The three hydia_*_accumulate functions are one routine over the product form (kernels.hip: FormCtCt, FormCtPlain, FormPlainCt): the
// shape checks, the block / wave split, the limb schedule, the choice of arithmetic and the ledger bytes are shared, so every layout
// one of them reads the others read the same way.
//
// ---- loop B of the HyDia sender: acc[q][g][3][nl][N] = sum_i rot[q][i] (x) db[g][i], fully reduced, for Q queries whose rotation sets
// lie rqs elements apart.  bpp, nw: a single query's launch (Q = 1) with the context's split caps (tensor_split); bpp = TENSOR_BATCH:
// a batch, ceil(Q / QW) passes over the database (QW = hydia_tensor_mq_width), one block per wave.  Every accumulator equals the
// single-query launch's for that query, bit for bit.  Slot of (query q, block gi): q * G + gi; ng > 0: the G "blocks" are (database
// block, giant step) pairs, block-major in the database, and the slots are giant-major over the whole batch,
// ((gi % ng) * Q + q) * (G / ng) + gi / ng, so that one giant step's partial sums over all queries and blocks are one contiguous batch
constexpr int TENSOR_BATCH = 0;
void hydia_tensor_accumulate(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G,
                             int dim, int nl, const DbLayout &L, int ng, int bpp, int nw);
int hydia_tensor_mq_width(const DbLayout &L);  // queries one pass over the database serves
// passes over the database a batch of Q queries takes at `width` queries per pass — the launcher's schedule: every pass takes the
// widest power of two up to width that still fits what is left (5 queries at width 4: 4 + 1; at width 2: 2 + 2 + 1)
inline int loop_b_passes(int Q, int width) {
    int passes = 0;
    for (int left = Q, qw = width; left > 0; left -= qw, passes++)
        while (qw > left) qw >>= 1;
    return passes;
}
// Loop B over a plain gallery (database kinds 7 / 8, L.plain): acc [G][2][nl][N] (slot map as above with a batch of one),
// acc[slot][p] = sum_i rot[i].c_p * m[g][i] mod q_j — no third component, nothing to relinearise.  bpp, nw: split caps (tensor_split)
void hydia_plain_accumulate(hipStream_t st, const ModC *mod, int N, const u64 *rot, const void *db, u64 *acc, int G, int dim, int nl,
                            const DbLayout &L, int ng, int bpp, int nw);
constexpr int PLAIN_BPP = 2;  // blocks per wave of a plain gallery's loop B (resources of every instantiation)
// Loop B for a PLAIN QUERY against an encrypted database (kinds 5 / 6; L.plain is refused): rot [dim][nl][N] = the rotations of the
// known probe's plaintext, ONE polynomial each (automorph_batch); acc [G][2][nl][N] (slot map as above with a batch of one),
// acc[slot][p] = sum_i rot[i] * db[g][i].c_p mod q_j — no third component, nothing to relinearise.  bpp, nw: split caps (tensor_split)
void hydia_pq_accumulate(hipStream_t st, const ModC *mod, int N, const u64 *rot, const void *db, u64 *acc, int G, int dim, int nl,
                         const DbLayout &L, int ng, int bpp, int nw);
// The same for a BATCH of Q plain queries whose rotation sets [dim][nl][N] lie rqs elements apart: ceil over hydia_pq_mq_width passes
// over the database (what is left over takes the narrower widths, a last odd query one of its own), one block per wave; acc
// [Q G][2][nl][N] with the batch slot map of hydia_tensor_accumulate.  Every accumulator equals hydia_pq_accumulate's for that query,
// bit for bit.  width: queries per pass (1, 2 or 4); 0 = hydia_pq_mq_width(L), the measured choice
void hydia_pq_accumulate_multi(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G,
                               int dim, int nl, const DbLayout &L, int ng, int width = 0);
int hydia_pq_mq_width(const DbLayout &L);  // queries one pass serves for this form
// A BATCH of Q encrypted queries against a PLAIN gallery (L.plain): rot holds the queries' rotation sets [dim][2][nl][N], rqs elements
// apart; acc [Q G][2][nl][N] with the batch slot map of hydia_tensor_accumulate.  Every accumulator equals hydia_plain_accumulate's for
// that query, bit for bit.  width: queries per pass (1, 2 or 4); 0 = hydia_plain_mq_width(L)
void hydia_plain_accumulate_multi(hipStream_t st, const ModC *mod, int N, const u64 *rot, size_t rqs, const void *db, u64 *acc, int Q, int G,
                                  int dim, int nl, const DbLayout &L, int ng, int width = 0);
int hydia_plain_mq_width(const DbLayout &L);  // queries one pass serves for this form
// out[i][j][c] = m[j][perm_{galois[i]}(c)], i < R, in one launch (m [nl][N], out [R][nl][N]; galois: device [R], 1 = identity)
void automorph_batch(hipStream_t st, int logN, const u64 *m, u64 *out, int nl, int R, const unsigned *galois);

// EvalMult(ct, plaintext) residue-wise (approach 1's merge masks): o[xp][j] = a[xp][j] * m[j] mod q_j with the Shoup companions ms;
// XP polynomials of nl limbs (a at limb stride a_ls, o compact), m / ms [nl][N]
void mul_plain(hipStream_t st, const ModC *mod, int N, const u64 *a, int a_ls, const u64 *m, const u64 *ms, u64 *o, int XP, int nl);

// ---- misc
void fill_uniform_hash(hipStream_t st, const ModC *mod, int N, u64 *dst, size_t n_limbpolys, int nl,
                       unsigned long long seed);  // bench filler: residues < q_limb from a counter hash
}  // namespace hk
