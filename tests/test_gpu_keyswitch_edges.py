"""Key switching on CRAFTED evaluation keys, BIT-EXACT against the CPU oracle holding the same key (tests/keyswitch_ref.py for the
patterns; tests/test_keyswitch_edges_cpu.py pins the oracle on them against a Python-integer model).  Every other GPU test feeds
the kernels keys from a key generator — uniform below q — so the lazy sums of <digits, key> never come near the ranges their
comments argue from.  Here the key operand is saturated (q - 1), saturated with holes, on the cycle 0, 1, q - 2, q - 1, one digit
alone, or uniform (the control), against a switched polynomial with the matching pattern and a uniform one.  Keys enter the context
through import_eval_key only; the public, secret and remaining keys are keygen_rotations' with the oracle's seed.  Every comparison
is np.array_equal on exported residues; a mismatch names (ciphertext, polynomial, limb, index, got, want).  A key that differs per
rotation (holes, edge, uniform: phase and seed = the rotation) stands in every list next to the rotation-independent ones (sat,
digit-d), so a kernel that reads rotation x's key for rotation x' is caught.

Both rings use vector_dim 16 (the context and the oracle accept it): at N = 2^15 loop A is still the fused fifteen-rotation launch.

  a  relinearize on imported 3-component ciphertexts (d2 itself patterned: a product of saturated pairs only gives d2 = 1), N = 2^15,
     12 / 9 / 5 / 4 / 2 limbs (full digits, a partial last digit, one digit, the 60-bit limb nearly alone), batches of 3 and 17
     (ntt15_p2_inner_product: IpAcc<IntP> on q_0 and the special primes — four lazy-output products below 2^124, fold128 — IpAcc<FpA>
     and the raw_fp hand-off into p2_finish5_fp on the 45-bit limbs).  At 5 / 4 / 2 limbs again with the unused digits' key rows
     saturated; the expectation is the oracle's with those rows as the pattern left them.  digit-d with d not in use is the same
     check from the other side: the only non-zero rows are rows nobody may read.  eval_mult with a1 = q - 1, b1 = 1 and the saturated
     key: the fused product path and the merged ModDown + Rescale on a saturated d2
  b  eval_rotate by 1 and 512 at 12 / 5 / 1 limbs, batches of 3 and 17, the same pairs on c1 (a saturated c1 stays saturated under
     the automorphism: own-digit products (q - 1)^2 in every slot); at 5 limbs and at 1 also with the unused digits' rows saturated
  c  loop A (DiagonalSender.rotateQuery), all 15 rotation keys crafted, the pattern in both polynomials of the query, every rotation
     against Or.rotate_query: default engine and HYDIA_LOOPA_INT_IP, HYDIA_KEYS_UNPACKED, HYDIA_NO_FUSE_LOOPA,
     HYDIA_LOOPA_SEPARATE_IP, HYDIA_LOOPA_LIMB_FASTEST, each in a context of its own (loop_a_ip_fp / loop_a_ip_int<SIX, RED> on six-
     and eight-byte rows, pre-multiplied by P^-1 (k_key_pack) and plain, both workgroup orders, k_inner_product<true / false>).  Also
     at 5 and 4 limbs on every engine, where LoopAOperands::fetch re-reads the last digit for d >= nd and the sums mask it (keys
     holes, sat, and the one whose only non-zero rows belong to a digit not in use).  The byte ledger says
     which form ran: the fused launch by default, k_inner_product under HYDIA_NO_FUSE_LOOPA
  d  giant-step keys: one block enrolled with 4 babies (giant keys 4, 8, 12), computeSimilarity with crafted giant-step keys that
     differ per key — the per-ciphertext key selection (IpArgs::keys) of the merged inner product; holes and sat
  e  a (12 limbs, 3 ciphertexts) and c (default engine) on evaluator_chain(15), transform_chain(15) and the chain with five 47-bit
     special primes, keys sat / holes / edge: the largest-c IntP limbs, 47 / 48-bit primes at the FpA / IntA boundary (and unpacked
     eight-byte key rows where a scaling prime has 48 bits or more), the fifth conversion source
  f  the generic kernels at N = 2^11: a, b and c at 12 / 5 / 2 limbs, batches of 1 and 5, default chain and transform_chain(11)
     (hk::inner_product; reduce_lazy on the 60-bit limbs with three saturated products)
  g  re-key: after crafted imports and a query served with them, the genuine keys are imported back; rotateQuery and relinearize on
     real ciphertexts equal the oracle with the genuine keys, and the ledger shows the packed shadow being rebuilt

What a compared residue depends on, from the inputs: with holes / edge / uniform keys every key residue of a digit in use enters
one output slot's sum with a non-zero, slot-dependent digit value, so one wrong key bit, one digit dropped or doubled, or another
rotation's row moves that residue.  sat / sat is the bound case but a blunt one: every digit's term is the same small negative
constant in every slot, the ModDown rounds any number of them to -1, so it detects a wrong FOLD (the sum's high bits) and not a
missing term — sat / uniform and uniform / sat carry that.

NOT reached: the extended limbs of a digit are base-conversion outputs; their joint worst case with a saturated key (every extended
residue at q - 1 together with the key) is not constructed — only the own-digit terms are (q - 1)^2 by construction.  The
conversions' own inputs are the business of the column-fused tests: tests/test_gpu_colfuse_edges.py lays the patterns on the
conversion SOURCES, in coefficient form, for the ModUp, the ModDown and the merged ModDown + Rescale (helpers in tests/colfuse_ref.py,
the host side in tests/test_colfuse_edges_cpu.py).  The sharded contexts' borrowed keys are not re-keyed here.

Nothing of the issue's list was dropped.  Measured on one MI355X: the whole file (about 200 cases) takes a quarter of a minute.  A
relinearize or eval_rotate case (both batches) 0.07 s, a loop A case on the default engine 0.3 s (it computes the oracle's fifteen
rotations of two queries; the switched engines reuse them: 0.07 - 0.10 s), a giant-step case 0.4 s, an edge-chain case 0.3 - 0.45 s
plus 0.3 - 0.9 s once per chain for keys and context, a generic-ring case about 0.1 s."""
import os
import re

import numpy as np
import pytest

import batch_ref as B
import keyswitch_ref as KR
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 20260412
DIM = 16
LOOP_A_ROTATIONS = tuple(range(1, DIM))
ROTATIONS = LOOP_A_ROTATIONS + (512,)
GIANT_KEYS = (4, 8, 12)
GENUINE = ("genuine", 0)
KEY_PATTERNS = KR.key_patterns(3)  # sat, holes, edge, uniform, digit-0 .. digit-2
PATTERN_ID = {p: i for i, p in enumerate(KEY_PATTERNS)}
# key pattern -> the patterns of the switched polynomial it meets (the issue's pairs; a uniform polynomial joins every key so that a
# batch holds two distinct ciphertexts)
PAIRED = {"sat": ("sat", "uniform"), "holes": ("holes", "uniform"), "uniform": ("sat", "uniform"), "edge": ("edge", "uniform"),
          "digit-0": ("sat", "uniform"), "digit-1": ("sat", "uniform"), "digit-2": ("sat", "uniform")}
PER_ROTATION = ("holes", "edge", "uniform")  # the key patterns that differ from one rotation to the next
LOOP_A_SWITCHES = ("HYDIA_LOOPA_INT_IP", "HYDIA_KEYS_UNPACKED", "HYDIA_NO_FUSE_LOOPA", "HYDIA_LOOPA_SEPARATE_IP", "HYDIA_LOOPA_LIMB_FASTEST")
FUSED_LOOP_A = re.compile(r"^k_ntt15_p2<true, [12], 5>$")


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def rng_for(*ints):
    return np.random.default_rng([SEED] + [int(i) for i in ints])


def owned(ct):
    """a copy of an oracle ciphertext's residues, taken while the ciphertext is alive (data() is a view into it)"""
    return ct.data().copy()


def check(got, want, src, tag):
    """every ciphertext of the batch against the oracle's result on the distinct input it was tiled from"""
    assert got.shape == (len(src),) + want.shape[1:], (tag, got.shape, want.shape)
    for i, s in enumerate(src):
        diff = KR.first_difference(got[i], want[s])
        if diff is not None:
            n, (p, j, c), g, w = diff
            raise AssertionError("%s: ciphertext %d of %d (distinct input %d) differs from the oracle at %d residues; first: polynomial %d "
                                 "limb %d index %d: got %d, want %d" % (tag, i, len(src), s, n, p, j, c, g, w))


def five_special_chain():
    """the chain of test_gpu_full_ring.py::test_five_special_primes_below_2p48_full_ring: the default Q limbs, five 47-bit special primes"""
    from sympy import isprime
    base = O.Params()
    M = 2 << 15
    c, p5 = (1 << 47) - ((1 << 47) % M) + 1, []
    while len(p5) < 5:
        c -= M
        if isprime(c):
            p5.append(c)
    moduli = np.array([int(x) for x in base.moduli[:base.nQ]] + p5, dtype=np.uint64)
    base.close()
    return moduli


def chain_moduli(name, log_n):
    from test_gpu_edge_primes import evaluator_chain, transform_chain
    if name == "default":
        return None, 4
    if name == "five":
        return five_special_chain(), 5
    return {"evaluator": evaluator_chain, "transform": transform_chain}[name](log_n), 4


class Rig:
    """One ring and chain: the oracle with its (edited) keys, the GPU contexts (one per engine switch), and which key contents each of
    them holds.  A key's contents are a function of its spec (pattern, limb count whose unused digits are saturated or 0) and its
    slot, so equal specs mean equal bytes and nothing is imported twice.  Expectations are computed once and never edited."""

    def __init__(self, im, log_n, chain="default"):
        self.im, self.chain = im, chain
        self.moduli, self.n_p = chain_moduli(chain, log_n)
        kw = {} if self.moduli is None else {"moduli": self.moduli, "n_p": self.n_p}
        self.P = P = O.Params(log_n=log_n, depth=11, dim=DIM, **kw)
        assert (P.nQ, P.dnum, P.alpha, P.dim) == (12, 3, 4, DIM) and 512 < P.slots
        self.K = O.Keys(P, SEED, rotations=list(ROTATIONS))
        self.Or = O.Oracle(P, self.K)
        self.slots = (0,) + ROTATIONS
        self.genuine = {s: self.view(s).copy() for s in self.slots}
        self.now = {s: GENUINE for s in self.slots}
        self.ctx, self.memo = {}, {}

    def close(self):
        for cc, _ in self.ctx.values():
            cc.close()
        self.ctx = {}

    # ---- keys
    def view(self, slot):
        return self.K.relin() if slot == 0 else self.K.rot_key(slot)

    def set_key(self, slot, spec):
        """the oracle's key `slot` := the contents of spec = (pattern, nl whose unused digits are saturated, or 0)"""
        if self.now[slot] == spec:
            return
        pattern, poison_nl = spec
        if pattern == "genuine":
            self.view(slot)[...] = self.genuine[slot]
        else:
            KR.craft_key(self.P, self.view(slot), pattern, rng_for(slot, PATTERN_ID[pattern]), phase=slot)
            if poison_nl:
                KR.poison_unused_digits(self.P, self.view(slot), poison_nl)
        self.now[slot] = spec

    def context(self, engine="default"):
        if engine not in self.ctx:
            saved = {k: os.environ.pop(k) for k in LOOP_A_SWITCHES if k in os.environ}
            if engine != "default":
                os.environ[engine] = "1"
            try:  # the switch is read when the context is created
                prm = self.im.default_params(log_n=self.P.log_n, vector_dim=DIM)
                if self.moduli is None:
                    cc = self.im.Context(prm, 0)
                else:
                    cc = self.im.Context(prm, 0, moduli=self.moduli, roots=self.P.roots, n_p=self.n_p)
            finally:
                os.environ.pop(engine, None)
                os.environ.update(saved)
            assert np.array_equal(cc.moduli, self.P.moduli) and np.array_equal(cc.roots, self.P.roots) and cc.dim == DIM
            cc.keygen_rotations(ROTATIONS, SEED)
            for s in (0, 1, 512):
                assert np.array_equal(cc.export_eval_key(s), self.genuine[s]), (engine, s)
            self.ctx[engine] = (cc, {s: GENUINE for s in self.slots})
        return self.ctx[engine][0]

    def push(self, engine, slots):
        """import into the engine's context every key of `slots` whose contents there differ from the oracle's"""
        cc = self.context(engine)
        held = self.ctx[engine][1]
        for s in slots:
            if held[s] != self.now[s]:
                cc.import_eval_key(s, self.view(s))
                held[s] = self.now[s]
        return cc

    # ---- inputs and expectations
    def _memo(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def inputs(self, npoly, nl, key_pattern):
        """(data [2][npoly][nl][N] of the two distinct ciphertexts a key pattern meets, their scale)"""
        scale = self.P.delta ** (npoly - 1)

        def one(pattern):
            def make():
                ct = B.new_ct(self.P, npoly, nl, scale)
                return owned(KR.craft_ct(self.P, ct, pattern, rng_for(100 + npoly, nl, PATTERN_ID[pattern])))
            return self._memo(("in", npoly, nl, pattern), make)
        return np.stack([one(p) for p in PAIRED[key_pattern]]), scale

    def oracle_ct(self, data, scale):
        ct = B.new_ct(self.P, data.shape[0], data.shape[1], scale)
        ct.data()[...] = data
        return ct

    def relin_want(self, nl, key_pattern):
        def make():
            self.set_key(0, (key_pattern, 0))
            data, scale = self.inputs(3, nl, key_pattern)
            out = []
            for d in data:
                ct = self.oracle_ct(d, scale)
                self.Or.relin(ct)
                out.append(owned(ct))
            return np.stack(out)
        return self._memo(("relin", nl, key_pattern), make)

    def rotate_want(self, nl, r, key_pattern):
        def make():
            self.set_key(r, (key_pattern, 0))
            data, scale = self.inputs(2, nl, key_pattern)
            return np.stack([owned(self.Or.rotate(self.oracle_ct(d, scale), r)) for d in data])
        return self._memo(("rot", nl, r, key_pattern), make)

    def loop_a_want(self, nl, key_pattern):
        """[2 queries][DIM][2][nl][N]: Or.rotate_query of the two queries the key pattern meets, all 15 keys crafted"""
        def make():
            for r in LOOP_A_ROTATIONS:
                self.set_key(r, (key_pattern, 0))
            data, scale = self.inputs(2, nl, key_pattern)
            out = []
            for d in data:
                rot = self.Or.rotate_query(self.oracle_ct(d, scale))
                out.append(np.stack([rot[i].data() for i in range(DIM)]))
            return np.stack(out)
        return self._memo(("loop_a", nl, key_pattern), make)


def run_relin(R, nl, key_pattern, batches, poisoned=False, engine="default"):
    want = R.relin_want(nl, key_pattern)  # (the oracle's with the unused digits' rows as the pattern left them)
    R.set_key(0, (key_pattern, nl if poisoned else 0))
    cc = R.push(engine, [0])
    data, scale = R.inputs(3, nl, key_pattern)
    for X in batches:
        batch, _, src = B.tile(data, X)
        g = cc.import_ct(batch, scale)
        cc.relinearize(g)
        assert g.shape()[:3] == (X, 2, nl)
        got = g.export()
        del g
        check(got, want, src, ("relinearize", R.chain, key_pattern, "poisoned" if poisoned else "", nl, X))


def run_rotate(R, nl, r, key_pattern, batches, poisoned=False, engine="default"):
    want = R.rotate_want(nl, r, key_pattern)
    R.set_key(r, (key_pattern, nl if poisoned else 0))
    cc = R.push(engine, [r])
    data, scale = R.inputs(2, nl, key_pattern)
    for X in batches:
        batch, _, src = B.tile(data, X)
        ga = cc.import_ct(batch, scale)
        g = cc.eval_rotate(ga, r)
        got = g.export()
        del ga, g
        check(got, want, src, ("rotate", R.chain, key_pattern, "poisoned" if poisoned else "", nl, X, r))


def run_loop_a(R, nl, key_pattern, engine="default"):
    want = R.loop_a_want(nl, key_pattern)
    for r in LOOP_A_ROTATIONS:
        R.set_key(r, (key_pattern, 0))
    cc = R.push(engine, LOOP_A_ROTATIONS)
    data, scale = R.inputs(2, nl, key_pattern)
    sender = R.im.DiagonalSender(cc, 1)
    for k in range(len(data)):
        gq = cc.import_ct(data[k], scale)
        got = sender.rotateQuery(gq).export()
        del gq
        check(got, want[k], list(range(DIM)), ("rotateQuery", R.chain, engine, key_pattern, PAIRED[key_pattern][k], nl))


# ---------------------------------------------------------------- N = 2^15, the default chain
@pytest.fixture(scope="module")
def full(im):
    R = Rig(im, 15)
    yield R
    R.close()


@pytest.mark.parametrize("nl", (12, 9, 5, 4, 2))
@pytest.mark.parametrize("key_pattern", KEY_PATTERNS)
def test_relinearize(full, key_pattern, nl):
    """group a"""
    run_relin(full, nl, key_pattern, (3, 17))


@pytest.mark.parametrize("nl", (5, 4, 2))
@pytest.mark.parametrize("key_pattern", ("holes", "edge", "uniform", "digit-0"))
def test_relinearize_with_poisoned_unused_digits(full, key_pattern, nl):
    """group a: the key rows of the digits >= ceil(nl / 4) saturated on the GPU; expected: as if they were not"""
    assert KR.digits_in_use(full.P, nl) < full.P.dnum
    run_relin(full, nl, key_pattern, (3, 17), poisoned=True)


@pytest.mark.parametrize("nl", (12, 9, 5, 4, 2))
def test_eval_mult_on_a_saturated_d2(full, nl):
    """group a: a1 = q - 1, b1 = 1 (d2 = q - 1 in every slot), a0 and b0 uniform, the saturated key: fused product, ModUp, inner
    product, merged ModDown + Rescale"""
    R, P = full, full.P
    R.set_key(0, ("sat", 0))
    cc = R.push("default", [0])

    def make():
        A, Bm, want = [], [], []
        for k in range(2):
            a = B.randomise(P, B.new_ct(P, 2, nl, P.delta), rng_for(200, nl, k))
            b = B.randomise(P, B.new_ct(P, 2, nl, P.delta), rng_for(201, nl, k))
            a.data()[1] = (P.moduli[:nl] - np.uint64(1))[:, None]
            b.data()[1] = 1
            A.append(owned(a))
            Bm.append(owned(b))
            want.append(owned(R.Or.mult(a, b)))
        return np.stack(A), np.stack(Bm), np.stack(want)
    A, Bm, want = R._memo(("mult", nl), make)
    for X in (3, 17):
        ba, _, src = B.tile(A, X)
        bb, _, _ = B.tile(Bm, X)
        ga, gb = cc.import_ct(ba, P.delta), cc.import_ct(bb, P.delta)
        g = cc.eval_mult(ga, gb)
        assert g.shape()[:3] == (X, 2, nl - 1)
        got = g.export()
        del ga, gb, g
        check(got, want, src, ("eval_mult, saturated d2", nl, X))


@pytest.mark.parametrize("nl", (12, 5, 1))
@pytest.mark.parametrize("r", (1, 512))
@pytest.mark.parametrize("key_pattern", KEY_PATTERNS)
def test_rotate(full, key_pattern, r, nl):
    """group b; at 5 limbs and at 1 also with the unused digits' key rows saturated"""
    run_rotate(full, nl, r, key_pattern, (3, 17))
    if KR.digits_in_use(full.P, nl) < full.P.dnum:
        run_rotate(full, nl, r, key_pattern, (3, 17), poisoned=True)


LOOP_A_CASES = [(e, k, 12) for k in ("sat",) + PER_ROTATION for e in ("default",) + LOOP_A_SWITCHES]
# (digit-2 at 5 limbs, digit-1 at 4: the only non-zero key rows belong to digits that are not in use — the rotation is the automorphism alone)
LOOP_A_CASES += [(e, k, nl) for nl, ks in ((5, ("holes", "sat", "digit-2")), (4, ("holes", "sat", "digit-1"))) for k in ks
                 for e in ("default",) + LOOP_A_SWITCHES]


@pytest.mark.parametrize("engine,key_pattern,nl", LOOP_A_CASES)
def test_loop_a(full, engine, key_pattern, nl):
    """group c"""
    run_loop_a(full, nl, key_pattern, engine)


def test_loop_a_forms_by_the_ledger(full, im):
    """group c: the default engine takes the fused loop A (the inner product inside the ModDown transforms), HYDIA_NO_FUSE_LOOPA the
    separate k_inner_product over packed rows, HYDIA_KEYS_UNPACKED never packs"""
    seen = {}
    for engine in ("default", "HYDIA_NO_FUSE_LOOPA", "HYDIA_KEYS_UNPACKED"):
        full.context(engine)
        im.byte_ledger(1)
        try:
            run_loop_a(full, 12, "holes", engine)
        finally:
            seen[engine] = set(im.byte_ledger(0))
    fused = {e: sorted(k for k in names if FUSED_LOOP_A.match(k)) for e, names in seen.items()}
    assert fused["default"] and not any(k.startswith("k_inner_product") for k in seen["default"]), sorted(seen["default"])
    assert not fused["HYDIA_NO_FUSE_LOOPA"] and "k_inner_product<true>" in seen["HYDIA_NO_FUSE_LOOPA"], sorted(seen["HYDIA_NO_FUSE_LOOPA"])
    assert fused["HYDIA_KEYS_UNPACKED"] and "k_key_pack" not in seen["HYDIA_KEYS_UNPACKED"], sorted(seen["HYDIA_KEYS_UNPACKED"])


@pytest.mark.parametrize("key_pattern", ("holes", "sat"))
def test_giant_step_keys(full, im, key_pattern):
    """group d: 4 babies x 4 giants at vector_dim 16; the three giant-step key switches of the block run as ONE batch that picks its
    key per ciphertext.  The baby keys 1..3 and the relinearisation key are the genuine ones."""
    R, P, Or = full, full.P, full.Or
    for s in (0, 1, 2, 3):
        R.set_key(s, GENUINE)
    for s in GIANT_KEYS:
        R.set_key(s, (key_pattern, 0))
    cc = R.push("default", R.slots)
    n = 3000
    db = rng_for(300).integers(-99, 100, size=(n, DIM)).astype(np.float64)
    query = np.ones(DIM)
    dbc = Or.enroll(db.copy(), 8, matvec=4)
    im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=8, matvec=4)
    assert cc.db_kind() == 6 and cc.db_babies() == 4 == dbc.babies
    q = Or.encrypt_query(query, 2, 9)
    gq = im.DiagonalReceiver(cc, n).encryptQuery(query, seed=2, nonce=9)
    assert np.array_equal(gq.export()[0], q.data())
    sim = Or.compute_similarity(q, dbc, n)
    assert len(sim) == 1
    got = im.DiagonalSender(cc, n).computeSimilarity(gq).export()
    check(got, sim[0].data()[None], [0], ("computeSimilarity, crafted giant-step keys", key_pattern))
    if key_pattern in PER_ROTATION:  # the three keys differ, so does what each contributes
        assert not np.array_equal(R.view(4), R.view(8)) and not np.array_equal(R.view(8), R.view(12))


def test_rekey_with_the_genuine_keys(full, im):
    """group g: crafted keys served a query (the packed shadow and the giant-step table were built from them); the genuine keys come
    back through the same import and everything follows them"""
    R, P, Or = full, full.P, full.Or
    run_loop_a(R, 12, "holes", "default")
    run_relin(R, 12, "holes", (3,))
    for s in R.slots:
        R.set_key(s, GENUINE)
    im.byte_ledger(1)
    try:
        cc = R.push("default", R.slots)
        rng = rng_for(400)
        query = rng.uniform(-1, 1, DIM)
        q = Or.encrypt_query(query, 2, 9)
        gq = im.DiagonalReceiver(cc, 1).encryptQuery(query, seed=2, nonce=9)
        assert np.array_equal(gq.export()[0], q.data())
        rot = Or.rotate_query(q)
        want = np.stack([rot[i].data() for i in range(DIM)])
        check(im.DiagonalSender(cc, 1).rotateQuery(gq).export(), want, list(range(DIM)), ("rotateQuery after the re-key",))
    finally:
        led = im.byte_ledger(0)
    assert led["k_key_pack"][0] == len(LOOP_A_ROTATIONS), led.get("k_key_pack")  # the shadow was packed again, every key of it
    a, b = Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 1), Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 2)
    d = Or.mult_norelin(a, b)
    g = cc.import_ct(d.data(), d.scale)
    Or.relin(d)
    cc.relinearize(g)
    check(g.export(), d.data()[None], [0], ("relinearize after the re-key",))


# ---------------------------------------------------------------- N = 2^15, edge chains
@pytest.fixture(scope="module", params=["evaluator", "transform", "five"])
def edge(request, im):
    R = Rig(im, 15, request.param)
    yield R
    R.close()


@pytest.mark.parametrize("key_pattern", ("sat", "holes", "edge"))
def test_edge_chains(edge, key_pattern):
    """group e"""
    run_relin(edge, 12, key_pattern, (3,))
    run_loop_a(edge, 12, key_pattern)


# ---------------------------------------------------------------- N = 2^11, the generic kernels
@pytest.fixture(scope="module", params=["default", "transform"])
def small(request, im):
    R = Rig(im, 11, request.param)
    yield R
    R.close()


@pytest.mark.parametrize("nl", (12, 5, 2))
@pytest.mark.parametrize("key_pattern", KEY_PATTERNS)
def test_generic_ring(small, key_pattern, nl):
    """group f: relinearize (also with the unused digits' rows saturated), eval_rotate by 1 and 512, rotateQuery"""
    run_relin(small, nl, key_pattern, (1, 5))
    if KR.digits_in_use(small.P, nl) < small.P.dnum:
        run_relin(small, nl, key_pattern, (1, 5), poisoned=True)
    for r in (1, 512):
        run_rotate(small, nl, r, key_pattern, (1, 5))
        if KR.digits_in_use(small.P, nl) < small.P.dnum:
            run_rotate(small, nl, r, key_pattern, (1, 5), poisoned=True)
    run_loop_a(small, nl, key_pattern)
