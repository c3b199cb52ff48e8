"""Helpers of the column-fused conversion tests (tests/test_colfuse_edges_cpu.py, tests/test_gpu_colfuse_edges.py): residue patterns laid
on the SOURCES of a fast base conversion, the inputs that make a ModUp, a ModDown and the merged ModDown + Rescale read them, and a
Python-integer restatement of the conversion sums of image_matching_amd/csrc/colfuse.hip (cf_macN / CfSum) with their three reductions
(cf_fold, IntP::fold_lh, reduce128k) that returns the intermediate words.  TEST INFRASTRUCTURE ONLY; no tests in here.

A conversion source is y_s = coeff_s (D / q_s)^-1 mod q_s in COEFFICIENT form (D the product of the source moduli).  A pattern laid in
the evaluation domain reaches the conversion as something uniform-looking, so here the pattern is laid on y itself, multiplied by
D / q_s and carried to the evaluation domain with the oracle's P.ntt_fwd.

A map (Map) is one (sources -> targets) conversion with the constants as evaluator.cpp's cf_plan_* form them from the moduli:
  modup_maps(P, nl)          one map per digit: sources the digit's limbs, targets every other limb of Q_l u P, f = D_d / q_s mod q_t
  moddown_map(P, nl)         sources the special primes, targets limbs 0 .. nl-1, f = P / p_k mod q_j; premul: times P^-1 mod q_j (loop A)
  mdr_map(P, nl)             merged ModDown + Rescale: the constants with P^-1 folded in, targets 0 .. l-1, fl = the dropped limb's

Source patterns, per source limb with modulus q (phase moves holes / edge / tie so that two keys or two digits differ):
  sat       q - 1
  holes     q - 1, one value in 16 replaced by a uniform one below q - 1 (keyswitch_ref.fill_row)
  edge      the cycle 0, 1, q - 2, q - 1
  lo30      the largest value below q whose low 30 bits are all ones: the low half of the 30 + 30 split at its maximum, the high half
            at or one below its maximum
  hi30      the largest value below q whose low 30 bits are zero: the high half alone
  uniform   the control
  tie       a table per (map, target) of source tuples chosen among TIE_TRIES random candidates: for an FP64 target the two whose
            quotient estimates in cf_fold (H c60 qinv, hi32(L) 2^32 qinv) lie closest to a rounding tie, the one with the largest
            operand and the one with the largest H; for an integer target the two whose exact sum lies closest below and above a
            multiple of q_t, the largest L and the largest H.  Coefficient i serves target i mod nt with variant (i div nt) mod 4."""
import numpy as np

import batch_ref as B
import keyswitch_ref as KR

SOURCE_PATTERNS = ("sat", "holes", "edge", "lo30", "hi30", "uniform", "tie")
TIE_TRIES = 3000
TIE_VARIANTS = 4
M30 = (1 << 30) - 1
M32 = (1 << 32) - 1
M60 = (1 << 60) - 1
_ints, _u64, _prod = KR._ints, KR._u64, KR._prod


def kind_of(q):
    """the arithmetic a modulus takes in the N = 2^15 kernels (context.cpp): FP64 up to 47 bits, the lazy pseudo-Mersenne integers for
    2^60 - c with c < 2^24, the general integers otherwise"""
    q = int(q)
    if q.bit_length() <= 47:
        return "fp"
    if q < (1 << 60) and (1 << 60) - q < (1 << 24):
        return "pm"
    return "int"


def lo30_value(q):
    v = (int(q) >> 30 << 30) | M30
    return v if v < int(q) else v - (1 << 30)


def hi30_value(q):
    return (int(q) - 1) >> 30 << 30


# ------------------------------------------------------------------ maps
class Map:
    """src / tgt: modulus indices; f[s][t] the conversion constants; hat[s] = D / q_s mod q_s and inv[s] its inverse (the factor that
    rides on the inverse transform); fl[s] / l: the dropped limb's constants and index (merged ModDown + Rescale only)"""

    def __init__(self, P, src, tgt, scale=None, l=None):
        q = [int(v) for v in P.moduli]
        self.src, self.tgt, self.l = list(src), list(tgt), l
        self.qs, self.qt = [q[s] for s in self.src], [q[t] for t in self.tgt]
        D = _prod(self.qs)
        self.hat = [D // qs % qs for qs in self.qs]
        self.inv = [pow(h, -1, qs) for h, qs in zip(self.hat, self.qs)]
        mul = (lambda t: 1) if scale is None else scale
        self.f = [[D // qs % q[t] * mul(t) % q[t] for t in self.tgt] for qs in self.qs]
        self.fl = None if l is None else [D // qs % q[l] * mul(l) % q[l] for qs in self.qs]
        self.key = (tuple(self.qs), tuple(self.qt), tuple(tuple(r) for r in self.f))


def modup_maps(P, nl):
    ext = list(range(nl)) + list(range(P.nQ, P.nT))
    out = []
    for d in range(KR.digits_in_use(P, nl)):
        lo, hi = d * P.alpha, min(d * P.alpha + P.alpha, nl)
        out.append(Map(P, range(lo, hi), [m for m in ext if not lo <= m < hi]))
    return out


def _pinv(P):
    PP = _prod(P.moduli[P.nQ:])
    return lambda t: pow(PP % int(P.moduli[t]), -1, int(P.moduli[t]))


def moddown_map(P, nl, premul=False):
    return Map(P, range(P.nQ, P.nT), range(nl), scale=_pinv(P) if premul else None)


def mdr_map(P, nl):
    return Map(P, range(P.nQ, P.nT), range(nl - 1), scale=_pinv(P), l=nl - 1)


# ------------------------------------------------------------------ the conversion sums, word by word
def cf_mac(y, f):
    """cf_macN: y a list of arrays of source residues (object arrays of Python ints for exact words, uint64 where the caller knows the
    ranges hold), f the constants.  Returns the words {pll, pmid, phh, L, H}; L is NOT wrapped at 2^64 (the premise tests bound it)."""
    pll = pmid = phh = 0
    for ys, fs in zip(y, f):
        yl, yh = ys & M30, ys >> 30
        fl, fh = int(fs) & M30, int(fs) >> 30
        pll = pll + yl * fl
        pmid = pmid + yl * fh + yh * fl
        phh = phh + yh * fh
    return {"pll": pll, "pmid": pmid, "phh": phh, "L": pll + ((pmid & M32) << 30), "H": phh + ((pmid >> 32) << 2)}


def fold_lh(L, H, q):
    """IntP::fold_lh: L + H 2^60 folded with 2^60 = c (mod q) to a lazy representative"""
    c = (1 << 60) - int(q)
    m1 = (H >> 32) * c
    acc = (L & M60) + (L >> 60) * c
    acc = acc + (H & M32) * c
    acc = acc + (m1 >> 28) * c
    return acc + ((m1 & 0x0FFFFFFF) << 32)


def _rint_times(a, b):
    """rint(fl(a) * fl(b)) of doubles, elementwise, as Python ints (numpy multiplies and rounds as IEEE binary64 does)"""
    return _ints(np.rint(np.asarray(a, dtype=np.float64) * np.float64(b)).astype(np.int64))


def cf_fold(L, H, q):
    """cf_fold: the FP64 fold.  Every step of the kernel is exact apart from the two quotient estimates, which are taken in doubles
    here too; the rest is integers.  Returns (operand, c1, c0): the operand handed to the forward butterflies and the quotients."""
    q = int(q)
    c60 = (1 << 60) % q
    qinv = 1.0 / float(q)
    Hf = np.array([float(v) for v in H])  # H < 2^50 (asserted by the caller): exact
    h1 = Hf * np.float64(c60)  # the rounded product whose quotient mulmod2 estimates
    c1 = _rint_times(h1, qinv)
    t1 = H * c60 - c1 * q
    hw = (L >> 32 & M32) << 32
    c0 = _rint_times(np.array([float(v) for v in hw]), qinv)
    t0 = hw - c0 * q
    return t1 + t0 + (L & M32), c1, c0


def tie_distance(L, H, q):
    """how far the two quotient estimates of cf_fold are from a rounding tie (0 = on it), for uint64 arrays L, H"""
    q = int(q)
    qinv = 1.0 / float(q)
    e1 = (H.astype(np.float64) * np.float64((1 << 60) % q)) * qinv
    e0 = ((L >> np.uint64(32)).astype(np.float64) * 4294967296.0) * qinv
    return np.abs(np.abs(e1 - np.floor(e1)) - 0.5), np.abs(np.abs(e0 - np.floor(e0)) - 0.5)


def fp_wide(qt, ql):
    """cf_fp_wide: the FP64 targets whose operands colfuse.hip re-centres after the conversion — a target below 2^40 (the low dword of L
    is not small against it) or one more than 1 / 32 smaller than the dropped limb (whose centred residue is up to q_l / 2); ql = 0
    without one"""
    return int(qt) < (1 << 40) or int(ql) > int(qt) + (int(qt) >> 5)


def reduce128k(z, q):
    """reduce128k: single-word Barrett on the top bits; returns (residue, the value before the two conditional subtractions, x)"""
    q = int(q)
    k = q.bit_length()
    mu = (1 << (k + 62)) // q
    x = z >> (k - 2)
    qh = (x * mu) >> 64
    r = z - qh * q  # (the kernel forms it modulo 2^64; the caller asserts 0 <= r < 3 q, where both agree)
    return r % q, r, x


def convert(cmap, y, stats=None, mutation=None, dropped=None):
    """One conversion through the word model: y [ns][n] object array of source residues -> [nt][n] canonical target residues in
    coefficient form.  dropped: (u [n] the dropped limb before the correction, as residues modulo q_l) for the merged ModDown +
    Rescale; the centred y_l = u - sum y_k fl[k] joins every target.  stats: a dict that collects the largest fraction of each bound
    of the colfuse.hip comments that was reached (and asserts nothing).  mutation: one of MUTATIONS, the deliberately wrong forms."""
    ns, nt = len(cmap.src), len(cmap.tgt)
    y = [y[s] for s in range(ns)]

    def note(name, value, bound):
        if stats is not None:
            stats[name] = max(stats.get(name, 0.0), float(max(int(v) for v in np.ravel(value))) / float(bound))

    def sums(f, t):
        use = list(range(ns))
        if mutation == "drop_source":
            use = use[:-1]
        f = list(f)
        if mutation == "neighbour_constant" and t is not None and nt > 1:
            f[0] = cmap.f[0][(t + 1) % nt]
        zero = np.zeros(len(y[0]), dtype=object)  # (keeps the words arrays where a mutation leaves no source at all)
        w = cf_mac([zero] + [y[s] for s in use], [0] + [f[s] for s in use])
        if mutation == "pmid_top":
            w["H"] = w["phh"]
        for name in ("pll", "pmid", "phh"):
            note(name + " / 2^63", w[name], 1 << 63)
        if ns <= 4:
            note("L / 2^63 (four sources)", w["L"], 1 << 63)
        else:
            note("L / (9 2^60) (five sources)", w["L"], 9 << 60)
            note("H / 2^51 (five sources)", w["H"], 1 << 51)
        return w

    cen = neg = None
    if dropped is not None:
        ql = int(dropped[1])
        w = sums(cmap.fl, None)
        yl = (dropped[0] - reduce128k(w["L"] + (w["H"] << 60), ql)[0]) % ql
        half = ql >> 1
        neg = (yl >= half) if mutation == "centre_ge" else (yl > half)
        cen = np.where(neg, ql - yl, yl)
        if mutation == "sign_flip":
            neg = ~neg
        note("centred dropped limb / 2^52", cen, 1 << 52)
    out = np.zeros((nt, len(y[0])), dtype=object)
    for t in range(nt):
        qt = cmap.qt[t]
        w = sums([cmap.f[s][t] for s in range(ns)], t)
        kind = kind_of(qt)
        if kind == "fp":
            note("H / 2^50 (FP64 target)", w["H"], 1 << 50)
            r, _, _ = cf_fold(w["L"], w["H"], qt)
            if cen is not None:
                r = r + np.where(neg, -cen, cen)
            raw = r
            if fp_wide(qt, 0 if cen is None else ql):  # cf_fp_wide: the operands of such a target are re-centred
                r = r - _rint_times(np.array([float(v) for v in r]), 1.0 / float(qt)) * qt
                note("|operand before the re-centring| / 2^52 (cf_fp_wide targets)", abs(raw), 1 << 52)
            if cen is not None:
                note("|cf_fold operand| / 1.9 q (with the dropped limb)", abs(r), 1.9 * qt)
            else:
                note("|cf_fold operand| / 1.4 q", abs(r), 1.4 * qt)
        elif kind == "pm":
            r = fold_lh(w["L"], w["H"], qt)
            note("fold_lh / (2.07 2^60)", r, 2.07 * 2.0 ** 60)
            if cen is not None:
                c = cen % qt
                r = r + np.where(neg, qt - c, c)
        else:
            r, raw, x = reduce128k(w["L"] + (w["H"] << 60), qt)
            note("reduce128k: x / 2^64", x, 1 << 64)
            note("reduce128k: remainder before the subtractions / 3 q", raw, 3 * qt)
            if cen is not None:
                r = r + np.where(neg, -(cen % qt), cen % qt)
        out[t] = r % qt
    return out


MUTATIONS = ("drop_source", "neighbour_constant", "pmid_top", "centre_ge", "sign_flip")


# ------------------------------------------------------------------ source patterns
_TIE = {}


def tie_table(cmap, seed=0):
    """[TIE_VARIANTS * nt][ns] uint64: row v * nt + t holds variant v of target t (see the module docstring)"""
    if cmap.key in _TIE:
        return _TIE[cmap.key]
    ns, nt = len(cmap.src), len(cmap.tgt)
    rng = np.random.default_rng([20260412, seed, ns, nt])
    cand = np.stack([rng.integers(0, qs, size=TIE_TRIES, dtype=np.uint64) for qs in cmap.qs])  # [ns][tries]
    tab = np.zeros((TIE_VARIANTS * nt, ns), dtype=np.uint64)
    for t in range(nt):
        qt = cmap.qt[t]
        w = cf_mac(list(cand), [cmap.f[s][t] for s in range(ns)])  # (uint64: every word stays below 2^64 for <= 5 sources)
        L, H = w["L"], w["H"]
        if kind_of(qt) == "fp":
            d1, d0 = tie_distance(L, H, qt)
            op = np.abs(np.array([float(v) for v in cf_fold(_ints(L), _ints(H), qt)[0]]))
            pick = [int(np.argmin(d1)), int(np.argmin(d0)), int(np.argmax(op)), int(np.argmax(H))]
        else:
            rem = [(a + (b << 60)) % qt for a, b in zip(L.tolist(), H.tolist())]
            pick = [rem.index(max(rem)), rem.index(min(rem)), int(np.argmax(L)), int(np.argmax(H))]
        for v in range(TIE_VARIANTS):
            tab[v * nt + t] = cand[:, pick[v]]
    _TIE[cmap.key] = tab
    return tab


def source_values(P, cmap, pattern, rng, phase=0):
    """[ns][N] uint64: the pattern on every source of the map"""
    ns = len(cmap.src)
    out = np.zeros((ns, P.N), dtype=np.uint64)
    if pattern == "tie":
        tab = tie_table(cmap)
        return np.ascontiguousarray(tab[(np.arange(P.N) + phase * len(cmap.tgt)) % len(tab)].T)
    for s, qs in enumerate(cmap.qs):
        if pattern == "lo30":
            out[s] = lo30_value(qs)
        elif pattern == "hi30":
            out[s] = hi30_value(qs)
        else:
            KR.fill_row(out[s], qs, pattern, rng, cmap.src[s] + phase)
    return out


def expected_sources(P, cmap, pattern, seed, phase=0):
    """what source_values returned for a generator seeded the same way (the premise tests compare recomputed sources with it)"""
    return source_values(P, cmap, pattern, np.random.default_rng(seed), phase)


def _mulmod(a, k, q):
    """(uint64 array a) * (int k) mod q through Python integers: uint64 [n]"""
    return _u64(_ints(a) * int(k) % int(q))


# ------------------------------------------------------------------ ModUp
def modup_input(P, nl, pattern, rng, phase=0):
    """[nl][N] evaluation form: the ModUp sources of every digit at nl limbs equal the pattern in every coefficient (one generator
    serves the digits in order, as modup_sources' caller re-creates them)"""
    c = np.zeros((nl, P.N), dtype=np.uint64)
    for d, cmap in enumerate(modup_maps(P, nl)):
        y = source_values(P, cmap, pattern, rng, phase + d)
        for s, j in enumerate(cmap.src):
            c[j] = P.ntt_fwd(_mulmod(y[s], cmap.hat[s], cmap.qs[s]), j)
    return c


def modup_sources(P, c, nl):
    """per digit [sz][N] uint64: ntt_inv(c_j) (D_d / q_j)^-1 mod q_j, recomputed from an evaluation-form polynomial"""
    return [np.stack([_mulmod(P.ntt_inv(c[j], j), cmap.inv[s], cmap.qs[s]) for s, j in enumerate(cmap.src)]) for cmap in modup_maps(P, nl)]


# ------------------------------------------------------------------ ModDown
def constant_extension(P, nl):
    """kappa[d][m]: the value, in every evaluation slot, of limb m of digit d's extension of the constant polynomial 1 (evaluation form
    all ones; coefficient form 1 at index 0 — the conversion acts on that one coefficient).  1 on the digit's own limbs."""
    q = [int(v) for v in P.moduli]
    out = []
    for cmap in modup_maps(P, nl):
        kap = {m: 1 for m in cmap.src}
        for t, m in enumerate(cmap.tgt):
            kap[m] = sum(cmap.inv[s] * cmap.f[s][t] for s in range(len(cmap.src))) % q[m]
        out.append(kap)
    return out


def moddown_key(P, nl, pattern, rng, phase=0, cmap=None):
    """(key [dnum][2][nT][N], polynomial [nl][N]): switching the constant polynomial with this key makes the ModDown's sources
    ntt_inv(acc_{nQ+k}) (P / p_k)^-1 equal the pattern, for both output polynomials (polynomial p with phase + p).  Only digit 0 of the
    key is non-zero; its Q-limb rows hold holes, so the combine after the conversion is decided in every slot.  cmap: the map the tie
    table is searched for (the ModDown's own by default; the pre-scaled and the merged forms have other constants)."""
    cmap = moddown_map(P, nl) if cmap is None else cmap
    kap = constant_extension(P, nl)[0]
    key = np.zeros((P.dnum, 2, P.nT, P.N), dtype=np.uint64)
    for p in range(2):
        y = source_values(P, cmap, pattern, rng, phase + p)
        for k, m in enumerate(cmap.src):
            assert kap[m] != 0
            w = _mulmod(y[k], cmap.hat[k], cmap.qs[k])
            key[0, p, m] = _mulmod(P.ntt_fwd(w, m), pow(kap[m], -1, cmap.qs[k]), cmap.qs[k])
        for m in range(P.nQ):
            KR.fill_row(key[0, p, m], P.moduli[m], "holes", rng, KR.row_shift(0, p, m, P.nT, phase))
    return key, np.ones((nl, P.N), dtype=np.uint64)


def extended_digits(P, c, nl, mutation=None, stats=None):
    """[nd][nE][N] object: every digit of c [nl][N] on the limbs of Q_l u P in evaluation form (own limbs: the input itself), the
    conversions through the word model"""
    ext = list(range(nl)) + list(range(P.nQ, P.nT))
    maps = modup_maps(P, nl)
    src = modup_sources(P, c, nl)
    out = np.zeros((len(maps), len(ext), P.N), dtype=object)
    for d, cmap in enumerate(maps):
        conv = convert(cmap, _ints(src[d]), stats=stats, mutation=mutation)
        for e, m in enumerate(ext):
            out[d, e] = _ints(c[m]) if m in cmap.src else _ints(P.ntt_fwd(_u64(conv[cmap.tgt.index(m)]), m))
    return out


def accumulate(P, dig, nl, key):
    """[2][nE][N] object: sum over the digits of digit * key row, reduced once"""
    ext = list(range(nl)) + list(range(P.nQ, P.nT))
    acc = np.zeros((2, len(ext), P.N), dtype=object)
    for p in range(2):
        for e, m in enumerate(ext):
            s = 0
            for d in range(dig.shape[0]):
                s = s + dig[d, e] * _ints(key[d, p, m])
            acc[p, e] = s % int(P.moduli[m])
    return acc


def moddown_sources(P, acc, nl):
    """[2][nP][N] uint64: ntt_inv(acc_{nQ+k}) (P / p_k)^-1 mod p_k of both accumulated polynomials"""
    cmap = moddown_map(P, nl)
    return np.stack([np.stack([_mulmod(P.ntt_inv(_u64(acc[p, nl + k]), m), cmap.inv[k], cmap.qs[k]) for k, m in enumerate(cmap.src)])
                     for p in range(2)])


def switch_model(P, c, nl, key, up=None, down=None, stats_up=None, stats_down=None, product=None):
    """Hybrid key switching of c [nl][N] with key [dnum][2][nT][N], every conversion through the word model.  up / down: a mutation of
    MUTATIONS applied to the ModUp's / the ModDown's conversions.  Without `product`: (out0, out1), each [nl][N] uint64 — what
    keyswitch_ref.keyswitch_model returns.  With product = (d0, d1), each [nl][N] (the product's first two polynomials): the merged
    ModDown + Rescale, [2][nl - 1][N] — relinearised and rescaled."""
    q = [int(v) for v in P.moduli]
    pinv = _pinv(P)
    acc = accumulate(P, extended_digits(P, c, nl, mutation=up, stats=stats_up), nl, key)
    y = moddown_sources(P, acc, nl)
    if product is None:
        cmap = moddown_map(P, nl)
        out = np.zeros((2, nl, P.N), dtype=np.uint64)
        for p in range(2):
            conv = convert(cmap, _ints(y[p]), stats=stats_down, mutation=down)
            for j in range(nl):
                out[p, j] = _u64((acc[p, j] - _ints(P.ntt_fwd(_u64(conv[j]), j))) * pinv(j) % q[j])
        return out[0], out[1]
    l = nl - 1
    cmap = mdr_map(P, nl)
    out = np.zeros((2, l, P.N), dtype=np.uint64)
    for p in range(2):
        u = _ints(P.ntt_inv(_u64((acc[p, l] * pinv(l) + _ints(product[p][l])) % q[l]), l))
        w = convert(cmap, _ints(y[p]), stats=stats_down, mutation=down, dropped=(u, q[l]))
        for j in range(l):
            x = acc[p, j] * pinv(j) + _ints(product[p][j]) - _ints(P.ntt_fwd(_u64(w[j]), j))
            out[p, j] = _u64(x * pow(q[l], -1, q[j]) % q[j])
    return out


def tensor(P, a, b):
    """the three polynomials of the product of two 2-component ciphertexts [2][nl][N] in evaluation form: [3][nl][N] uint64"""
    nl = a.shape[1]
    out = np.zeros((3, nl, P.N), dtype=np.uint64)
    for j in range(nl):
        qj = int(P.moduli[j])
        a0, a1, b0, b1 = (_ints(v[j]) for v in (a[0], a[1], b[0], b[1]))
        out[0, j], out[1, j], out[2, j] = _u64(a0 * b0 % qj), _u64((a0 * b1 + a1 * b0) % qj), _u64(a1 * b1 % qj)
    return out


# ------------------------------------------------------------------ merged ModDown + Rescale
def mdr_input(P, nl, pattern, rng, phase=0):
    """(key, a [2][2][nl][N], b [2][nl][N], targets [2][N]): eval_mult(a[i], b) under the relinearisation key `key` runs the merged
    ModDown + Rescale on special-prime sources equal to the pattern AND with the dropped limb's value before centring,
    y_l = u - sum y_k fl[k] mod q_l, equal to batch_ref.boundary_targets (0, 1, half - 1 .. half + 2, q_l - 2, q_l - 1 around the
    ring; polynomial 0 ascending, polynomial 1 descending) for both distinct ciphertexts a[0] (other limbs uniform) and a[1]
    (saturated).  b = (1, 1) and a1 = 1 in evaluation form: d2 = 1 (the constant polynomial of moddown_key), d0 = a0, d1 = a0 + 1.
    Polynomial 0's target is reached through a0's limb l, the free addend; polynomial 1 shares that addend, so its target is reached
    through the key's own row of limb l."""
    assert nl >= 2
    l = nl - 1
    ql = int(P.moduli[l])
    cmap = mdr_map(P, nl)
    key, _ = moddown_key(P, nl, pattern, rng, phase, cmap=cmap)
    kap = constant_extension(P, nl)[0]
    pinv_l = _pinv(P)(l)
    PP = _prod(cmap.qs)
    t = _ints(B.boundary_targets(ql, P.N))
    delta = np.zeros(P.N, dtype=object)
    delta[0] = 1  # the constant polynomial 1 in coefficient form: a1 b0 on limb l

    def correction(p):  # sum_k y_k fl[k]: the conversion's share of y_l (fl carries P^-1)
        y = [_ints(_mulmod(P.ntt_inv(_mulmod(key[0, p, m], kap[m], cmap.qs[k]), m), cmap.inv[k], cmap.qs[k])) for k, m in enumerate(cmap.src)]
        return sum(y[k] * cmap.fl[k] for k in range(len(y))) % ql

    # rest_p = y_l(p) - coeff(a0_l) [- delta]: the key's share.  Polynomial 1's row of limb l := what makes rest_1 = rest_0 - delta + t_1 - t_0
    rest0 = (_ints(P.ntt_inv(_mulmod(key[0, 0, l], kap[l], ql), l)) * pinv_l - correction(0)) % ql
    want_acc1 = (rest0 - delta + t[1] - t[0] + correction(1)) * (PP % ql) % ql
    key[0, 1, l] = _mulmod(P.ntt_fwd(_u64(want_acc1), l), pow(kap[l], -1, ql), ql)
    a = np.zeros((2, 2, nl, P.N), dtype=np.uint64)
    for i in range(2):
        for j in range(l):
            KR.fill_row(a[i, 0, j], P.moduli[j], "uniform" if i == 0 else "sat", rng, 0)
        a[i, 0, l] = P.ntt_fwd(_u64((t[0] - rest0) % ql), l)
        a[i, 1] = 1
    return key, a, np.ones((2, nl, P.N), dtype=np.uint64), _u64(t)


def dropped_limb(P, relinearised, nl):
    """[2][N]: the dropped limb of a relinearised ciphertext [2][nl][N] in coefficient form — the value the rescale centres"""
    return np.stack([P.ntt_inv(relinearised[p][nl - 1], nl - 1) for p in range(2)])
