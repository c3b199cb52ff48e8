"""The small element-wise kernels under the scenarios, on caller-supplied residues at the ends of every limb's range (q_j - 1, 0, their
alternation, 1, and uniform rows that are all different), at N = 2^11 on two chains: the default one (a 60-bit q_0, eleven 45-bit
limbs) and test_gpu_edge_primes.evaluator_chain (the IntP prime with the largest c, the lean-edge pair, the top 47-bit and the smallest
48-bit prime).  Every expectation is an exact integer formula (tests/additive_ref.py, pinned by tests/test_additive_model_cpu.py) or the
CPU oracle on the same residues; every comparison is np.array_equal on exported residues.

  add_many            k_batch_sum (compact input, more than two ciphertexts: 128-bit sums, one reduce128) and the X - 1 k_addsub<0>
                      launches on aliases, against the model; the byte ledger says which form ran.  129 saturated ciphertexts pass
                      2^64 on q_0, the only size here that separates a 64-bit accumulator from a 128-bit one.
  ct_add_raw /        k_addsub<2>, k_mod_reduce, reduce64: 16 saturated addends land within 16 (c + 1) of 2^64 on q_0 = 2^60 - c; sums
  ct_mod_reduce       that are an exact multiple of q_j are where reduce64's conditional subtraction is needed (the model file shows
                      that 16 (q_j - 1) is not); an accumulator that is a limb-prefix view has a limb stride (12) that differs from its
                      limb count (5).  hydia_level_reduce copies, so a level-reduced accumulator is compact: that case runs too.
  eval_sum /          rotate_acc at N = 2^11 against the oracle's rotate and add in the engine's order (r = 1, 2, 4, .., slots / 2).
  sum_and_evalsum
  chebyshev_compare   depth 7 and 10 against the oracle on the same residues, under the default engine (k_lincomb_multi's FP64 form on
                      the limbs below 2^47, the 128-bit form on the others) and under HYDIA_NTT_INT, the switch Context::lincomb_multi
                      reads (getenv_int_arith, context.cpp) to clear lc.fp, which sends every limb through the 128-bit form.

What the comparator cases do NOT pin: only the first layer sees the crafted values: the first leaves (k_lincomb_multi on T_1),
k_add_scalar's constants and the first products (k_tensor on T_1 x T_1, k_tensor<SUB>'s subtrahend T_1).  After one relinearisation
the residues are pseudo-random again, so the later leaves, k_lincomb and k_mul_scalar run on uniform data as in every other test.  The
scale is meaningless on such inputs; residues are the requirement, not decryption.  The column-fused kernels and the base conversions
are not this file's business."""
import os

import numpy as np
import pytest

import additive_ref as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 20260312
INT_SWITCH = "HYDIA_NTT_INT"  # context.cpp: getenv_int_arith; evaluator.cpp Context::lincomb_multi: lc.fp = ... && !getenv_int_arith


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


class Rig:
    """One chain: oracle, GPU context built from the oracle's moduli and roots, and the oracle's results (computed once, never edited)."""

    def __init__(self, im, name):
        self.im, self.name = im, name
        self.P = P = A.CHAINS[name]()
        self.rots = A.powers_of_two(P.slots) if name == "default" else []  # only the default chain's cases rotate
        self.K = O.Keys(P, SEED, rotations=self.rots)
        self.Or = O.Oracle(P, self.K)
        self.cc = self.context()
        self.cache = {}
        self._int = None

    def context(self):
        P = self.P
        cc = self.im.Context(self.im.default_params(log_n=P.log_n, vector_dim=P.dim), 0, moduli=P.moduli, roots=P.roots, n_p=P.nP)
        assert np.array_equal(cc.moduli, P.moduli) and np.array_equal(cc.roots, P.roots)
        cc.keygen_rotations(self.rots, SEED)
        assert np.array_equal(cc.export_eval_key(0), self.K.relin())
        return cc

    def int_context(self):
        """a second context created under the switch that clears lc.fp (read when the context is created)"""
        if self._int is None:
            saved = os.environ.pop(INT_SWITCH, None)
            os.environ[INT_SWITCH] = "1"
            try:
                self._int = self.context()
            finally:
                del os.environ[INT_SWITCH]
                if saved is not None:
                    os.environ[INT_SWITCH] = saved
        return self._int

    def memo(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def batch(self, kind, X, npoly, nl, seed=0):
        P = self.P
        if kind == "distinct":
            return A.distinct(P.moduli, X, npoly, nl, P.N, seed=seed)
        return A.BUILDERS[kind](P.moduli, X, npoly, nl, P.N)

    def close(self):
        self.cc.close()
        if self._int is not None:
            self._int.close()


@pytest.fixture(scope="module")
def rigs(im):
    """one context per chain for the whole module, built when first asked for"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(im, name)
        return made[name]
    yield get
    for R in made.values():
        R.close()


@pytest.fixture(scope="module", params=("default", "edge"))
def rig(request, rigs):
    return rigs(request.param)


@pytest.fixture(scope="module")
def default_rig(rigs):
    return rigs("default")


def same(got, want, tag):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d residues differ; first at %s: got %d, want %d" % (tag, len(bad), at, got[at], want[at]))


class ledger:
    """the kernel names (and launch counts) the byte ledger records around one call"""

    def __init__(self, im):
        self.im, self.seen = im, {}

    def __enter__(self):
        self.im.byte_ledger(1)
        return self

    def __exit__(self, *exc):
        self.seen = {k: n for k, (n, _) in self.im.byte_ledger(0).items()}


# ---------------------------------------------------------------- add_many
def add_many_shapes(X):
    """(npoly, nl): the whole cross product for the small batches; the one large batch (50 MB at 12 limbs) on two components only"""
    return [(2, 12), (2, 1)] if X == 129 else [(npoly, nl) for npoly in (2, 3) for nl in (12, 5, 1)]


@pytest.mark.parametrize("kind", ("saturated", "alternating", "distinct"))
@pytest.mark.parametrize("X", (1, 2, 3, 4, 129))
def test_add_many_equals_the_integer_model(rig, X, kind):
    """sizes 1 and 2 take the modular-add form, 3 is the first k_batch_sum launch, 129 is past a 64-bit accumulator on q_0"""
    P, cc = rig.P, rig.cc
    for npoly, nl in add_many_shapes(X):
        tag = (rig.name, kind, X, npoly, nl)
        data = rig.batch(kind, X, npoly, nl, seed=X)
        want = A.sum_mod(data, P.moduli)
        g = cc.import_ct(data, P.delta)
        with ledger(rig.im) as led:
            out = cc.add_many(g)
        assert out.shape()[:3] == (1, npoly, nl), tag
        same(out.export()[0], want, tag)
        if X >= 3:  # compact, more than two ciphertexts: one k_batch_sum launch and no modular add
            assert led.seen.get("k_batch_sum") == 1 and "k_addsub" not in led.seen, (tag, led.seen)
        else:
            assert "k_batch_sum" not in led.seen and led.seen.get("k_addsub", 0) == X - 1, (tag, led.seen)
        del g, out


@pytest.mark.parametrize("npoly", (2, 3))
def test_add_many_on_a_limb_prefix_view_takes_the_fallback(rig, npoly):
    """three ciphertexts read through ct_limb_prefix (limb stride 12, 5 limbs in use) are not compact: X - 1 modular adds on aliases,
    and the result equals the model on the prefix limbs"""
    P, cc = rig.P, rig.cc
    for kind in ("saturated", "distinct"):
        tag = (rig.name, kind, npoly)
        data = rig.batch(kind, 3, npoly, 12, seed=7)
        base = cc.import_ct(data, P.delta)
        view = cc.ct_limb_prefix(base, 5)
        with ledger(rig.im) as led:
            out = cc.add_many(view)
        assert out.shape()[:3] == (1, npoly, 5), tag
        same(out.export()[0], A.sum_mod(data[:, :, :5], P.moduli), tag)
        assert "k_batch_sum" not in led.seen and led.seen.get("k_addsub") == 2, (tag, led.seen)
        same(base.export(), data, tag + ("the viewed batch is unchanged",))
        del out, view, base


# ---------------------------------------------------------------- ct_add_raw / ct_mod_reduce
def model(addends):
    """equal-shaped [X][npoly][nl][N] addends as one [n][X npoly][nl][N] batch for the integer model, and the accumulator's shape"""
    s = np.stack(addends)
    n, X, npoly, nl, N = s.shape
    return s.reshape(n, X * npoly, nl, N), (X, npoly, nl, N)


def accumulate(cc, acc, sources):
    """acc += every source, as the sharded membership reduction does: by device pointer"""
    for src in sources:
        ptr, nbytes = src.device_ptr()
        assert nbytes == acc.shape()[0] * acc.shape()[1] * acc.shape()[2] * cc.N * 8  # the source is compact and of the accumulator's shape
        cc.ct_add_raw(acc, ptr)


def check_raw_then_reduced(rig, addends, acc, sources, tag, read=None):
    """the accumulator holds the plain 64-bit sum, then its canonical residues, and a second reduction changes nothing"""
    P, cc = rig.P, rig.cc
    read = read or (lambda: acc.export())
    stack, shape = model(addends)
    accumulate(cc, acc, sources)
    same(read(), A.raw_sum(stack).reshape(shape), tag + ("plain sum",))
    want = A.sum_mod(stack, P.moduli).reshape(shape)
    cc.ct_mod_reduce(acc)
    same(read(), want, tag + ("reduced",))
    cc.ct_mod_reduce(acc)
    same(read(), want, tag + ("reduced twice",))
    return want


@pytest.mark.parametrize("npoly", (2, 3))
def test_sixteen_saturated_addends_reach_the_top_of_64_bits(rig, npoly):
    """accumulator and source q_j - 1 everywhere, the source added 15 times: 16 (q_j - 1) as plain uint64, without a wrap, then
    16 (q_j - 1) mod q_j"""
    P, cc = rig.P, rig.cc
    sat = rig.batch("saturated", 1, npoly, P.nQ)
    acc, src = cc.import_ct(sat, P.delta), cc.import_ct(sat, P.delta)
    want = check_raw_then_reduced(rig, [sat] * 16, acc, [src] * 15, (rig.name, npoly, "saturated x 16"))
    for j in range(P.nQ):
        q = int(P.moduli[j])
        assert np.all(want[:, :, j] == np.uint64(16 * (q - 1) % q))


@pytest.mark.parametrize("npoly", (2, 3))
def test_sums_that_are_a_multiple_of_the_modulus_reduce_to_zero(rig, npoly):
    """15 + 15 (q_j - 1) = 15 q_j and 1 + (q_j - 1) = q_j: reduce64's quotient estimate is one short there (see the model file), so
    the residue 0 needs its conditional subtraction"""
    P, cc = rig.P, rig.cc
    sat = rig.batch("saturated", 1, npoly, P.nQ)
    src = cc.import_ct(sat, P.delta)
    for first, times in ((15, 15), (1, 1)):
        start = A.constant(P.moduli, 1, npoly, P.nQ, P.N, first)
        acc = cc.import_ct(start, P.delta)
        want = check_raw_then_reduced(rig, [start] + [sat] * times, acc, [src] * times, (rig.name, npoly, "multiple of q", first))
        assert not want.any()


@pytest.mark.parametrize("total", (1, 2, 16))
@pytest.mark.parametrize("npoly", (2, 3))
def test_distinct_addends(rig, npoly, total):
    """batches of two ciphertexts, every addend drawn on its own; one addend in total = the reduction of canonical residues (identity)"""
    P, cc = rig.P, rig.cc
    addends = [rig.batch("distinct", 2, npoly, P.nQ, seed=100 + i) for i in range(total)]
    acc = cc.import_ct(addends[0], P.delta)
    sources = [cc.import_ct(a, P.delta) for a in addends[1:]]
    check_raw_then_reduced(rig, addends, acc, sources, (rig.name, npoly, "distinct", total))


@pytest.mark.parametrize("kind", ("saturated", "distinct"))
def test_accumulator_whose_limb_stride_differs_from_its_limb_count(rig, kind):
    """the accumulator is the 5-limb prefix view of a 12-limb ciphertext (limb stride 12), the sources are compact 5-limb ciphertexts:
    16 addends in total.  The view is read through its parent: limbs 0 .. 4 hold the model's sums, limbs 5 .. 11 stay what they were"""
    P, cc = rig.P, rig.cc
    for npoly in (2, 3):
        full = rig.batch(kind, 2, npoly, P.nQ, seed=50)
        if kind == "saturated":
            adds = [rig.batch(kind, 2, npoly, 5)] * 15
            handles = [cc.import_ct(adds[0], P.delta)] * 15
        else:
            adds = [rig.batch(kind, 2, npoly, 5, seed=60 + i) for i in range(15)]
            handles = [cc.import_ct(a, P.delta) for a in adds]
        parent = cc.import_ct(full, P.delta)
        acc = cc.ct_limb_prefix(parent, 5)
        assert acc.shape()[:3] == (2, npoly, 5) and acc.device_ptr()[1] == parent.device_ptr()[1]  # 5 limbs in use, 12 allocated
        tag = (rig.name, kind, npoly, "prefix view")
        check_raw_then_reduced(rig, [full[:, :, :5]] + adds, acc, handles, tag, read=lambda: parent.export()[:, :, :5])
        same(parent.export()[:, :, 5:], full[:, :, 5:], tag + ("limbs past the prefix",))
        del acc, parent


def test_level_reduced_accumulator(rig):
    """hydia_level_reduce from 12 to 5 limbs (a compact copy) and a compact 5-limb source, 16 addends: the model on those 5 limbs"""
    P, cc = rig.P, rig.cc
    for npoly in (2, 3):
        full = rig.batch("distinct", 1, npoly, P.nQ, seed=70)
        adds = [rig.batch("distinct", 1, npoly, 5, seed=80 + i) for i in range(15)]
        acc = cc.import_ct(full, P.delta)
        cc.level_reduce(acc, 5)
        assert acc.shape()[:3] == (1, npoly, 5)
        check_raw_then_reduced(rig, [full[:, :, :5]] + adds, acc, [cc.import_ct(a, P.delta) for a in adds], (rig.name, npoly, "level-reduced"))


# ---------------------------------------------------------------- eval_sum / sum_and_evalsum (the default chain: the only cases that rotate)
@pytest.mark.parametrize("nl", (12, 2))
@pytest.mark.parametrize("X", (1, 3))
def test_eval_sum_and_sum_and_evalsum(default_rig, X, nl):
    R = default_rig
    P, Or, cc = R.P, R.Or, R.cc
    for kind in ("distinct", "saturated"):
        tag = (kind, X, nl)
        data = R.batch(kind, X, 2, nl, seed=nl)
        g = cc.import_ct(data, P.delta)
        want = np.stack([A.eval_sum_ref(Or, A.oracle_ct(P, data[x], P.delta)) for x in range(X)])
        same(cc.eval_sum(g).export(), want, tag + ("eval_sum",))
        want = A.eval_sum_ref(Or, A.oracle_ct(P, A.sum_mod(data, P.moduli), P.delta))
        same(cc.sum_and_evalsum(g).export()[0], want, tag + ("sum_and_evalsum",))


# ---------------------------------------------------------------- the comparator's leaves
COMPARE_INPUTS = ("saturated", "zeros", "alternating", "ones", "distinct")
COMPARE_BATCHES = [(k,) for k in COMPARE_INPUTS] + [("saturated", "alternating", "distinct"), ("zeros", "ones", "distinct")]


def compare_reference(R, depth):
    """{input: (residues, the oracle's chebyshev_compare on them)} and the scale, on crafted full-level encryptions"""
    def make():
        P, Or = R.P, R.Or
        out, scale = {}, None
        for i, kind in enumerate(COMPARE_INPUTS):
            ct = A.crafted_encryption(Or, R.batch(kind, 1, 2, P.nQ, seed=9)[0], 17, 40 + i)
            res = Or.chebyshev_compare(ct, 0.44, depth)
            out[kind] = (ct.data().copy(), res.data().copy())  # (data() is a view: copied while ct and res are alive)
            scale = ct.scale
        return out, scale
    return R.memo(("compare", depth), make)


@pytest.mark.parametrize("engine", ("default", INT_SWITCH))
@pytest.mark.parametrize("depth", (7, 10))
def test_comparator_on_crafted_residues(rig, depth, engine):
    """a batch of 1 of every input and two batches of 3 with different rows, bit for bit against the oracle on the same residues"""
    ref, scale = compare_reference(rig, depth)
    cc = rig.cc if engine == "default" else rig.int_context()
    for kinds in COMPARE_BATCHES:
        tag = (rig.name, depth, engine, kinds)
        g = cc.import_ct(np.stack([ref[k][0] for k in kinds]), scale)
        with ledger(rig.im) as led:
            got = cc.chebyshev_compare(g, 0.44, depth).export()
        assert led.seen.get("k_lincomb_multi", 0) >= 1, (tag, sorted(led.seen))
        same(got, np.stack([ref[k][1] for k in kinds]), tag)
