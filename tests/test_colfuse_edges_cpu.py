"""The host side of the column-fused conversion tests (tests/test_gpu_colfuse_edges.py), without a GPU, at N = 2^11 where a
big-integer model runs over every coefficient:

  premises   the inputs of tests/colfuse_ref.py are what they claim: the conversion sources recomputed from modup_input (12, 9 and 5
             limbs: digits of 4/4/4, 4/4/1, 4/1), from moddown_key and from mdr_input with P.ntt_inv and Python integers equal the
             pattern in every coefficient, and the dropped limb of the relinearised product sits on the centring boundary list
  oracle     on those inputs the oracle (hyo_keyswitch, Or.relin, Or.rotate, Or.mult) equals the word model of colfuse_ref
             (switch_model: cf_macN's words, cf_fold, fold_lh, reduce128k, the merged ModDown + Rescale) and keyswitch_ref's
             keyswitch_model bit for bit
  ranges     the bounds the comments of colfuse.hip argue from hold on every crafted pattern with the real constants of the default
             chain, evaluator_chain, transform_chain and the five-special chain, at 12 / 10 / 9 / 5 / 4 / 2 limbs, for the ModUp maps,
             the ModDown (plain and pre-scaled) and the merged ModDown + Rescale wherever the fused path is taken ((q_l >> 50) == 0)
  reach      per pattern family, the largest fraction of each bound that was reached is printed (pytest -s); recorded below
  sensitive  five deliberately wrong forms of the model change the compared output on every family that claims to cover them

Reach, measured: the largest fraction of each bound reached over the four chains (N = 2^11 forms), all limb counts and maps; a
record, not a threshold (test_reach_report prints it).      sat   holes    edge    lo30    hi30 uniform     tie
  pll / 2^63                                              0.500   0.500   0.331   0.500   0.000   0.461   0.462
  pmid / 2^63                                             0.998   0.998   0.499   0.998   0.500   0.800   0.845
  phh / 2^63                                              0.498   0.498   0.249   0.498   0.498   0.453   0.484
  L / 2^63 (four sources)                                 0.787   0.992   0.716   0.870   0.500   0.908   0.957
  L / (9 2^60) (five sources below 2^48)                  0.790   0.857   0.636   0.755   0.434   0.779   0.762
  H / 2^51 (five sources below 2^48)                      0.202   0.202   0.138   0.202   0.202   0.182   0.188
  H / 2^50 (FP64 target)                                  0.244   0.244   0.189   0.244   0.244   0.228   0.239
  |cf_fold operand| / 1.4 q         default chain         0.608   0.705   0.662   0.630   0.630   0.710   0.713
                                    evaluator_chain       0.711   0.711   0.704   0.588   0.642   0.713   0.714
                                    transform_chain       0.611   0.711   0.674   0.543   0.588   0.714   0.715
                                    five special primes   0.531   0.711   0.696   0.670   0.687   0.712   0.713
  ... / 1.9 q with the dropped limb default chain         0.693   0.758   0.683   0.674   0.708   0.769   0.786
                                    evaluator_chain       0.569   0.709   0.641   0.637   0.736   0.772   0.789
                                    transform_chain       0.462   0.616   0.511   0.497   0.470   0.740   0.760
                                    five special primes   0.652   0.751   0.688   0.757   0.687   0.780   0.787
  |operand before the re-centring| / 2^52 (cf_fp_wide)    0.019   0.024   0.022   0.022   0.021   0.024   0.024
  fold_lh / (2.07 2^60)                                   0.925   0.974   0.966   0.824   0.873   0.982   0.966
  centred dropped limb / 2^52                             0.016 in every family (half of a 48-bit dropped limb)
  reduce128k: x / 2^64                                    0.500   0.500   0.500   0.500   0.500   0.475   0.497
  reduce128k: remainder before the subtractions / 3 q     0.458   0.489   0.469   0.432   0.390   0.498   0.500
So the one-word partial sums come within 0.2 % of 2^63 (pmid: saturated 60-bit sources against a 60-bit constant), L within 1 %
(holes), the lazy pseudo-Mersenne fold within 2 % of its 2.07 2^60 (uniform) — uniform sources reach 0.80 / 0.91 / 0.98 of those
three, the crafted ones what is left.  H of an FP64 target stays at a quarter of 2^50: no chain here puts four 60-bit sources
against a 47-bit target.  cf_fold's operand reaches 0.71 of 1.4 q and 0.79 of 1.9 q on every chain.  Before the kernels re-centred
the operands of the targets that cf_fp_wide names, these two rows read up to 3.5 on transform_chain (4.9 q beside its 31-bit
target) and 8625 with the dropped limb, and 1.51 on evaluator_chain with the dropped limb (the 48-bit limb beside 45-bit targets):
the one finding of this file that changed a kernel (test_fold_operand_as_the_comment_states_it).

Which family sees which wrong form (asserted in test_mutations_are_seen): a dropped source, a neighbouring target's constant and the
lost top bits of pmid move the output on EVERY family, in the ModUp, in the ModDown and in the merged form — except that a
neighbour's constant does not exist where a map has one target (the merged form at 2 limbs: asserted blind there; the 5-limb cases
carry it).  The centring rule and the dropped limb's sign are seen on every family of mdr_input, because its dropped limb runs
through half and half + 1; with an uncrafted (uniform) dropped limb `>=` for `>` is NOT seen (asserted as the control) — that is
the one the boundary list carries alone."""
import numpy as np
import pytest

import batch_ref as B
import colfuse_ref as CF
import keyswitch_ref as KR
import oracle_lib as O

SEED = 20260412
LIMBS = (12, 9, 5)
RANGE_LIMBS = (12, 10, 9, 5, 4, 2)
CHAINS = ("default", "evaluator", "transform", "five")
RANGE_COEFFS = 256  # every pattern repeats within 16 coefficients, the tie table within 4 * 15
REACH = {}  # bound -> pattern -> largest fraction reached


def rng_for(*ints):
    return np.random.default_rng([SEED] + [int(i) for i in ints])


def params_of(chain):
    import test_gpu_keyswitch_edges as KE  # (functions of that GPU module; importing it runs nothing)
    moduli, n_p = KE.chain_moduli(chain, 11)
    kw = {} if moduli is None else {"moduli": moduli, "n_p": n_p}
    P = O.Params(log_n=11, depth=11, dim=16, **kw)
    assert (P.nQ, P.dnum, P.alpha, P.nP) == (12, 3, 4, n_p)
    return P


class Ring:
    def __init__(self, chain):
        self.chain, self.P = chain, params_of(chain)
        self.K = O.Keys(self.P, SEED, rotations=[1])
        self.Or = O.Oracle(self.P, self.K)
        self.genuine = {0: self.K.relin().copy(), 1: self.K.rot_key(1).copy()}

    def view(self, slot):
        return self.K.relin() if slot == 0 else self.K.rot_key(slot)

    def restore(self):
        for slot, data in self.genuine.items():
            self.view(slot)[...] = data

    def ct(self, data, scale):
        c = B.new_ct(self.P, data.shape[0], data.shape[1], scale)
        c.data()[...] = data
        return c


@pytest.fixture(scope="module", params=["default", "transform"])
def ring(request):
    R = Ring(request.param)
    yield R
    R.restore()


@pytest.fixture(scope="module")
def default_ring():
    R = Ring("default")
    yield R
    R.restore()


def same(got, want, tag):
    diff = KR.first_difference(got, want)
    assert diff is None, "%s: %d residues differ; first at %s: got %d, want %d" % ((tag,) + diff)


# ---------------------------------------------------------------- the patterns
def test_source_patterns_are_what_they_claim(default_ring):
    P = default_ring.P
    for cmap in CF.modup_maps(P, 12) + [CF.moddown_map(P, 12)]:
        for pattern in CF.SOURCE_PATTERNS:
            y = CF.source_values(P, cmap, pattern, rng_for(1), phase=2)
            q = np.array(cmap.qs, dtype=np.uint64)[:, None]
            assert y.shape == (len(cmap.src), P.N) and (y < q).all(), pattern
            if pattern == "sat":
                assert (y == q - np.uint64(1)).all()
            elif pattern == "holes":
                assert ((y == q - np.uint64(1)).sum(axis=1) == P.N - P.N // KR.HOLE_EVERY).all()
            elif pattern == "edge":
                for v in (0, 1):
                    assert ((y == np.uint64(v)).sum(axis=1) == P.N // 4).all() and ((y == q - np.uint64(1 + v)).sum(axis=1) == P.N // 4).all()
            elif pattern == "lo30":
                assert ((y & np.uint64(CF.M30)) == np.uint64(CF.M30)).all() and (y + np.uint64(1 << 30) >= q).all()
            elif pattern == "hi30":
                assert ((y & np.uint64(CF.M30)) == 0).all() and (y + np.uint64(1 << 30) >= q).all()
            elif pattern == "tie":
                tab = CF.tie_table(cmap)
                nt = len(cmap.tgt)
                assert tab.shape == (CF.TIE_VARIANTS * nt, len(cmap.src)) and len(np.unique(tab, axis=0)) > nt
                for i in (0, 1, nt, 3 * nt + 2, P.N - 1):  # coefficient i serves target i mod nt
                    row = (i + 2 * nt) % len(tab)
                    assert row % nt == i % nt and np.array_equal(y[:, i], tab[row])
    # the tie table does what it was searched for: on an FP64 target its first two variants sit closer to a rounding tie than the
    # median candidate by orders of magnitude; on an integer target the exact sum is within q / 200 of a multiple of q from below / above
    cmap = CF.moddown_map(P, 12)
    tab = CF.tie_table(cmap)
    for t, qt in enumerate(cmap.qt):
        f = [cmap.f[s][t] for s in range(len(cmap.src))]
        w = [CF.cf_mac(list(tab[v * len(cmap.tgt) + t][:, None]), f) for v in range(2)]
        if CF.kind_of(qt) == "fp":
            assert CF.tie_distance(w[0]["L"], w[0]["H"], qt)[0][0] < 2e-3 and CF.tie_distance(w[1]["L"], w[1]["H"], qt)[1][0] < 2e-3
        else:
            rem = [(int(x["L"][0]) + (int(x["H"][0]) << 60)) % qt for x in w]
            assert qt - rem[0] < qt // 200 and rem[1] < qt // 200


# ---------------------------------------------------------------- premises and the oracle
@pytest.mark.parametrize("pattern", CF.SOURCE_PATTERNS)
@pytest.mark.parametrize("nl", LIMBS)
def test_modup_input(ring, nl, pattern):
    """the ModUp sources of every digit equal the pattern; hyo_keyswitch with the genuine key equals the word model"""
    P = ring.P
    ring.restore()
    c = CF.modup_input(P, nl, pattern, rng_for(2, nl), phase=3)
    src = CF.modup_sources(P, c, nl)
    again = rng_for(2, nl)
    for d, cmap in enumerate(CF.modup_maps(P, nl)):
        same(src[d], CF.source_values(P, cmap, pattern, again, 3 + d), ("ModUp sources", ring.chain, nl, pattern, d))
    key = ring.genuine[0]
    got = KR.oracle_keyswitch(P, c, nl, key)
    want = CF.switch_model(P, c, nl, key)
    for p in range(2):
        same(got[p], want[p], ("hyo_keyswitch on modup_input", ring.chain, nl, pattern, p))


@pytest.mark.parametrize("pattern", CF.SOURCE_PATTERNS)
@pytest.mark.parametrize("nl", LIMBS)
def test_moddown_key(ring, nl, pattern):
    """the ModDown sources of both output polynomials equal the pattern; hyo_keyswitch equals the word model"""
    P = ring.P
    key, c = CF.moddown_key(P, nl, pattern, rng_for(3, nl), phase=2)
    assert not key[1:].any()
    y = CF.moddown_sources(P, CF.accumulate(P, CF.extended_digits(P, c, nl), nl, key), nl)
    again = rng_for(3, nl)
    cmap = CF.moddown_map(P, nl)
    for p in range(2):
        same(y[p], CF.source_values(P, cmap, pattern, again, 2 + p), ("ModDown sources", ring.chain, nl, pattern, p))
        for m in range(P.nQ):  # (the generator also served the Q-limb rows of polynomial p)
            KR.fill_row(np.zeros(P.N, dtype=np.uint64), P.moduli[m], "holes", again, 0)
    got = KR.oracle_keyswitch(P, c, nl, key)
    want = CF.switch_model(P, c, nl, key)
    for p in range(2):
        same(got[p], want[p], ("hyo_keyswitch with moddown_key", ring.chain, nl, pattern, p))
        assert got[p].any()


@pytest.mark.parametrize("pattern", ["sat", "lo30", "tie"])
@pytest.mark.parametrize("nl", LIMBS)
def test_oracle_callers(ring, nl, pattern):
    """the callers the GPU file compares with, reading the crafted keys through the edited views: Or.relin and Or.rotate against
    keyswitch_ref's models (and those against the word model), on modup_input with the genuine keys and on moddown_key"""
    P, Or = ring.P, ring.Or
    ring.restore()
    c = CF.modup_input(P, nl, pattern, rng_for(4, nl), phase=1)
    data = KR.craft_ct(P, B.new_ct(P, 3, nl, P.delta ** 2), "uniform", rng_for(5, nl)).data().copy()
    data[2] = c
    d = ring.ct(data, P.delta ** 2)
    Or.relin(d)
    same(d.data(), KR.relin_model(P, data, ring.genuine[0]), ("Or.relin on modup_input", ring.chain, nl, pattern))
    data[1] = c
    rot = Or.rotate(ring.ct(data[:2], P.delta), 1)  # (kept alive while its residues are read)
    same(rot.data(), KR.rotate_model(P, data[:2], ring.genuine[1], 1), ("Or.rotate on modup_input", ring.chain, nl, pattern))
    key, one = CF.moddown_key(P, nl, pattern, rng_for(6, nl), phase=1)
    k0, k1 = KR.keyswitch_model(P, one, nl, key)
    w0, w1 = CF.switch_model(P, one, nl, key)
    same(w0, k0, ("the word model against keyswitch_model", 0))
    same(w1, k1, ("the word model against keyswitch_model", 1))
    for slot in (0, 1):
        ring.view(slot)[...] = key
    data[2] = one
    data[1] = one
    d = ring.ct(data, P.delta ** 2)
    Or.relin(d)
    relin = d.data().copy()
    rot = Or.rotate(ring.ct(data[:2], P.delta), 1)
    rotated = rot.data().copy()
    ring.restore()
    same(relin, KR.relin_model(P, data, key), ("Or.relin with moddown_key", ring.chain, nl, pattern))
    same(rotated, KR.rotate_model(P, data[:2], key, 1), ("Or.rotate with moddown_key", ring.chain, nl, pattern))


@pytest.mark.parametrize("pattern", CF.SOURCE_PATTERNS)
@pytest.mark.parametrize("nl", (12, 5, 2))
def test_mdr_input(default_ring, nl, pattern):
    """the relinearised product's dropped limb is the boundary list in both polynomials of both ciphertexts, the special-prime sources
    are the pattern, and Or.mult equals the word model extended by the rescale"""
    R, P, Or = default_ring, default_ring.P, default_ring.Or
    key, a, b, t = CF.mdr_input(P, nl, pattern, rng_for(7, nl), phase=1)
    half = int(P.moduli[nl - 1]) >> 1
    assert [int(v) for v in t[0, :8]] == [0, 1, half - 1, half, half + 1, half + 2, 2 * half - 1, 2 * half]
    assert np.array_equal(t[1, :8], t[0, 7::-1])
    y = CF.moddown_sources(P, CF.accumulate(P, CF.extended_digits(P, b[1], nl), nl, key), nl)
    again = rng_for(7, nl)
    for p in range(2):
        same(y[p], CF.source_values(P, CF.mdr_map(P, nl), pattern, again, 1 + p), ("merged form's sources", nl, pattern, p))
        for m in range(P.nQ):
            KR.fill_row(np.zeros(P.N, dtype=np.uint64), P.moduli[m], "holes", again, 0)
    R.view(0)[...] = key
    try:
        for i in range(2):
            ca, cb = R.ct(a[i], P.delta), R.ct(b, P.delta)
            d = Or.mult_norelin(ca, cb)
            prod = d.data().copy()
            same(prod, CF.tensor(P, a[i], b), ("mult_norelin", i))
            assert (prod[2] == 1).all()
            Or.relin(d)
            same(CF.dropped_limb(P, d.data(), nl), t, ("the dropped limb before centring", nl, pattern, i))
            m = Or.mult(ca, cb)
            same(m.data(), CF.switch_model(P, prod[2], nl, key, product=(prod[0], prod[1])), ("Or.mult on mdr_input", nl, pattern, i))
    finally:
        R.restore()


# ---------------------------------------------------------------- ranges and reach
AS_STATED = ("|cf_fold operand| / 1.4 q", "|cf_fold operand| / 1.9 q (with the dropped limb)")
BOUNDS_BELOW_ONE = ("pll / 2^63", "pmid / 2^63", "phh / 2^63", "L / 2^63 (four sources)", "L / (9 2^60) (five sources)",
                    "H / 2^51 (five sources)", "H / 2^50 (FP64 target)") + AS_STATED + (
                    "|operand before the re-centring| / 2^52 (cf_fp_wide targets)", "fold_lh / (2.07 2^60)", "centred dropped limb / 2^52",
                    "reduce128k: x / 2^64", "reduce128k: remainder before the subtractions / 3 q")
RANGE_STATS = {}


def range_stats(chain):
    """{(nl, map kind, pattern): the fractions convert() noted} over every map of the chain; the words are checked against the sums
    they stand for on the way.  The merged form is taken only where the evaluator takes the fused kernel ((q_l >> 50) == 0); there
    the dropped limb runs through the boundary list."""
    if chain in RANGE_STATS:
        return RANGE_STATS[chain]
    P = params_of(chain)
    n = RANGE_COEFFS
    five = P.nP == 5
    if five:
        assert all(int(q) < (1 << 48) for q in P.moduli[P.nQ:])  # (what Context::cf_ok demands of five sources)
    found = {}
    for nl in RANGE_LIMBS:
        maps = [("up", m) for m in CF.modup_maps(P, nl)] + [("down", CF.moddown_map(P, nl)), ("down-premul", CF.moddown_map(P, nl, premul=True))]
        if int(P.moduli[nl - 1]) >> 50 == 0:
            maps.append(("mdr", CF.mdr_map(P, nl)))
        for what, cmap in maps:
            assert len(cmap.src) <= (5 if five and what != "up" else 4)
            for pattern in CF.SOURCE_PATTERNS:
                y = KR._ints(CF.source_values(P, cmap, pattern, rng_for(8, nl), phase=nl)[:, :n])
                stats, dropped = found.setdefault((nl, what, pattern), {}), None
                if what == "mdr":
                    ql = int(P.moduli[nl - 1])
                    yl = KR._ints(B.boundary_targets(ql, n)[0])
                    corr = sum(y[k] * cmap.fl[k] for k in range(len(cmap.src))) % ql
                    dropped = ((yl + corr) % ql, ql)
                out = CF.convert(cmap, y, stats=stats, dropped=dropped)
                for t, qt in enumerate(cmap.qt):  # the words mean the sum they claim to
                    want = sum(y[k] * cmap.f[k][t] for k in range(len(cmap.src)))
                    if dropped is not None:
                        want = want + np.where(yl > (ql >> 1), yl - ql, yl)
                    assert (out[t] == want % qt).all(), (chain, nl, what, pattern, t)
    P.close()
    RANGE_STATS[chain] = found
    return found


@pytest.mark.parametrize("chain", CHAINS)
def test_range_premises(chain):
    """every bound of the colfuse.hip comments, on every crafted pattern, with the chain's real constants"""
    found = range_stats(chain)
    assert sum(1 for (nl, what, pattern) in found if what == "mdr" and pattern == "sat") >= 4
    for (nl, what, pattern), stats in found.items():
        for name, frac in stats.items():
            assert name in BOUNDS_BELOW_ONE and frac < 1.0, (chain, nl, what, pattern, name, frac)


@pytest.mark.parametrize("chain", CHAINS)
def test_fold_operand_as_the_comment_states_it(chain):
    """colfuse.hip on cf_fold: "|operand| <= 1.4 q (... the first term stays below 0.875 q; the second below 0.5 q; 1.9 q with the
    dropped limb's centred residue)".  The sum alone keeps that only where the low dword of L, which enters as it is, is small
    against q, and where the dropped limb is no larger than the FP64 target.  This test found both premises broken on the edge
    chains: without more, the operand reaches 4.9 q beside transform_chain's 31-bit target (the low dword is up to 4 q), 2^14 q
    where a 45-bit limb is dropped beside it, and 2.9 q where evaluator_chain's 48-bit limb is dropped beside 45-bit targets —
    exact all the same, but outside what the transform's own argument takes for granted.  The kernels now re-centre the operands
    of exactly those targets (cf_fp_wide: q < 2^40 or q_l > (1 + 1/32) q, one workgroup-uniform branch, never taken on a chain
    of like primes: asserted below for the default and the five-special chain), the model follows (colfuse_ref.fp_wide), and the bound holds on all four chains as stated.  The re-centring step itself
    needs its input below 2^52: asserted in test_range_premises (0.016 of it reached)."""
    seen = 0
    for (nl, what, pattern), stats in range_stats(chain).items():
        for name in AS_STATED:
            if name in stats:
                seen += 1
                assert stats[name] < 1.0, (chain, nl, what, pattern, name, stats[name])
    assert seen
    P = params_of(chain)
    wide = {(int(P.moduli[t]).bit_length(), nl) for nl in RANGE_LIMBS for t in range(nl - 1) if CF.kind_of(P.moduli[t]) == "fp"
            and CF.fp_wide(P.moduli[t], P.moduli[nl - 1] if int(P.moduli[nl - 1]) >> 50 == 0 else 0)}
    assert bool(wide) == (chain in ("evaluator", "transform")), (chain, sorted(wide))  # the default and five-special chains never branch
    P.close()


def test_reach_report():
    """prints (pytest -s) the largest fraction of each bound reached, per pattern family and over the four chains — the figures of
    this file's docstring — and, for the operand with the dropped limb, per chain.  Every family reached every quantity."""
    print()
    print("%-56s %s" % ("largest fraction reached", " ".join("%9s" % p for p in CF.SOURCE_PATTERNS)))
    for name in BOUNDS_BELOW_ONE:
        for chains in ((CHAINS,) if name not in AS_STATED else tuple((c,) for c in CHAINS)):
            row = {}
            for chain in chains:
                for (nl, what, pattern), stats in range_stats(chain).items():
                    if name in stats:
                        row[pattern] = max(row.get(pattern, 0.0), stats[name])
            print("%-56s %s" % (name if len(chains) > 1 else "  on " + chains[0], " ".join("%9.3f" % row.get(p, float("nan")) for p in CF.SOURCE_PATTERNS)))
            assert set(row) == set(CF.SOURCE_PATTERNS), name


# ---------------------------------------------------------------- sensitivity
@pytest.fixture(scope="module")
def mutation_cases(default_ring):
    """per pattern, at 5 limbs (digits of 4 / 1; four targets in the merged form): the three inputs and the oracle's outputs on them"""
    R, P, Or = default_ring, default_ring.P, default_ring.Or
    nl, cases = 5, {}
    for i, pattern in enumerate(CF.SOURCE_PATTERNS):
        R.restore()
        c = CF.modup_input(P, nl, pattern, rng_for(9, i), phase=1)
        up = np.stack(KR.oracle_keyswitch(P, c, nl, R.genuine[0]))
        key, one = CF.moddown_key(P, nl, pattern, rng_for(10, i), phase=1)
        down = np.stack(KR.oracle_keyswitch(P, one, nl, key))
        mkey, a, b, _ = CF.mdr_input(P, nl, pattern, rng_for(11, i), phase=1)
        R.view(0)[...] = mkey
        m = Or.mult(R.ct(a[0], P.delta), R.ct(b, P.delta))
        cases[pattern] = {"c": c, "up": up, "key": key, "one": one, "down": down, "mkey": mkey, "prod": CF.tensor(P, a[0], b),
                          "mdr": m.data().copy()}
    R.restore()
    return cases


@pytest.mark.parametrize("pattern", CF.SOURCE_PATTERNS)
@pytest.mark.parametrize("mutation", CF.MUTATIONS)
def test_mutations_are_seen(default_ring, mutation_cases, mutation, pattern):
    """the comparisons of this file and of the GPU file are not vacuous: each wrong form of the model differs from the oracle on
    every family.  The unmutated model equals it (test_modup_input, test_moddown_key, test_mdr_input)."""
    P, nl, k = default_ring.P, 5, mutation_cases[pattern]
    prod = k["prod"]
    if mutation in ("centre_ge", "sign_flip"):
        wrong = CF.switch_model(P, prod[2], nl, k["mkey"], down=mutation, product=(prod[0], prod[1]))
        assert (wrong != k["mdr"]).any(axis=2).all(), "not every limb of both polynomials moves"
        return
    up = np.stack(CF.switch_model(P, k["c"], nl, default_ring.genuine[0], up=mutation))
    assert (up != k["up"]).any(axis=2).all(), "ModUp"
    down = np.stack(CF.switch_model(P, k["one"], nl, k["key"], down=mutation))
    assert (down != k["down"]).any(axis=2).all(), "ModDown"
    mdr = CF.switch_model(P, prod[2], nl, k["mkey"], down=mutation, product=(prod[0], prod[1]))
    assert (mdr != k["mdr"]).any(axis=2).all(), "merged ModDown + Rescale"


def test_what_a_family_cannot_see(default_ring):
    """the blind spots, stated: a map with one target has no neighbouring constant (the merged form at 2 limbs), and with an
    uncrafted dropped limb the centring rule `>=` for `>` moves nothing — only mdr_input's boundary list holds half itself"""
    R, P, Or = default_ring, default_ring.P, default_ring.Or
    key, a, b, _ = CF.mdr_input(P, 2, "sat", rng_for(12), phase=1)
    prod = CF.tensor(P, a[0], b)
    right = CF.switch_model(P, prod[2], 2, key, product=(prod[0], prod[1]))
    assert np.array_equal(right, CF.switch_model(P, prod[2], 2, key, down="neighbour_constant", product=(prod[0], prod[1])))
    assert not np.array_equal(right, CF.switch_model(P, prod[2], 2, key, down="centre_ge", product=(prod[0], prod[1])))
    a[0, 0, 1] = rng_for(13).integers(0, int(P.moduli[1]), size=P.N, dtype=np.uint64)  # the addend uncrafted: a uniform dropped limb
    prod = CF.tensor(P, a[0], b)
    right = CF.switch_model(P, prod[2], 2, key, product=(prod[0], prod[1]))
    assert np.array_equal(right, CF.switch_model(P, prod[2], 2, key, down="centre_ge", product=(prod[0], prod[1])))
    assert not np.array_equal(right, CF.switch_model(P, prod[2], 2, key, down="sign_flip", product=(prod[0], prod[1])))
