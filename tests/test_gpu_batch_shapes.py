"""The evaluator's batch-size-dependent kernels at N = 2^15, BIT-EXACT against the CPU oracle, on both sides of every selection rule
(image_matching_amd/csrc: ntt15_colfuse_small, ntt15_inverse_p1_narrow, the merged / per-digit second pass, pair_polys, Rescale's
column-fused form from 128 ciphertexts), on inputs that sit on the rescale's centring boundary.

Every expectation is the oracle's result on a few DISTINCT inputs; a batch of X ciphertexts is tiled from them (batch_ref.tile: first,
last, odd and even positions hold different data) and every ciphertext of the GPU result is compared with np.array_equal on exported
residues.  The distinct operand pairs per limb count: (i) two real ciphertexts of the oracle's own product chain, (ii) the same through
batch_ref.craft_product_pair (the relinearised dropped limb is 0, 1, half - 1, half, half + 1, half + 2, q - 2, q - 1 around the
ring), (iii) every residue q_j - 1 in both operands, (iv) q_j - 1 against uniform residues.

The byte ledger records which kernel form each launch took: over the mult sweep both forms of each column-fused family must appear,
over the rescale sweep the column-fused launch must appear from 128 ciphertexts and not at 3 — asserted over the sweep, so a threshold
may move inside the swept range but not out of it."""
import os

import numpy as np
import pytest

import batch_ref as B
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 20260117
ROTATIONS = (1, 512)
MULT_X = (2, 3, 10, 11, 15, 16, 17, 128, 129)
RESCALE_X = (3, 127, 128, 129)
SWITCHES = ("HYDIA_COLFUSE_WIDE", "HYDIA_INT_EPILOGUE", "HYDIA_NO_RESCALE_CF", "HYDIA_NO_MERGE_RESCALE", "HYDIA_NO_PROD_FUSE",
            "HYDIA_NO_KS_FUSE", "HYDIA_NO_COLFUSE", "HYDIA_P2_WG_SYNC", "HYDIA_NTT_INT")
SEEN = {"mult": {}, "rescale": {}}  # sweep -> X -> kernel names the byte ledger recorded


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def owned(ct):
    """a copy of an oracle ciphertext's residues, taken while the ciphertext is alive (data() is a view into it)"""
    return ct.data().copy()


class Rig:
    """One ring: oracle, GPU context, the distinct inputs per limb count and the oracle's results on them (computed once, never edited)."""

    def __init__(self, im, P, K, cc, limb_counts):
        self.im, self.P, self.K, self.Or, self.cc = im, P, K, O.Oracle(P, K), cc
        rng = np.random.default_rng(P.log_n)
        a = self.Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 1)
        b = self.Or.encrypt(rng.uniform(-1, 1, P.slots), 3, 2)
        self.chain = B.mult_chain(self.Or, a, b, limb_counts)
        self.rng = np.random.default_rng(P.log_n + 1)
        self.cache = {}

    def _memo(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def pairs(self, nl):
        """the oracle ciphertexts of the four operand pairs at nl limbs"""
        def make():
            P, Or = self.P, self.Or
            a, b = self.chain[nl]
            a2, b2 = a.clone(), b.clone()
            B.craft_product_pair(P, Or, a2, b2)
            a3, b3 = B.saturate(P, a.clone()), B.saturate(P, b.clone())
            a4, b4 = B.saturate(P, a.clone()), B.randomise(P, b.clone(), self.rng)
            return [(a, b), (a2, b2), (a3, b3), (a4, b4)]
        return self._memo(("pairs", nl), make)

    def pair_data(self, nl):
        """(A [4][2][nl][N], B likewise, scale of a, scale of b)"""
        def make():
            ps = self.pairs(nl)
            return np.stack([x.data() for x, _ in ps]), np.stack([y.data() for _, y in ps]), ps[0][0].scale, ps[0][1].scale
        return self._memo(("pair_data", nl), make)

    def mult_want(self, nl):
        return self._memo(("mult", nl), lambda: np.stack([owned(self.Or.mult(x, y)) for x, y in self.pairs(nl)]))

    def steps_want(self, nl):
        def make():
            w = {"norelin": [], "relin": [], "rescale": []}
            for x, y in self.pairs(nl):
                d = self.Or.mult_norelin(x, y)
                w["norelin"].append(owned(d))
                self.Or.relin(d)
                w["relin"].append(owned(d))
                self.Or.rescale(d)
                w["rescale"].append(owned(d))
            return {k: np.stack(v) for k, v in w.items()}
        return self._memo(("steps", nl), make)

    def rot_inputs(self, nl):
        """pairs (i), (iii), (iv): a real ciphertext, a saturated one, a uniform one (no product: nothing to craft)"""
        def make():
            a = self.chain[nl][0]
            cts = [a, B.saturate(self.P, a.clone()), B.randomise(self.P, a.clone(), self.rng)]
            return cts, np.stack([c.data() for c in cts]), a.scale
        return self._memo(("rot_in", nl), make)

    def rot_want(self, nl, r):
        return self._memo(("rot", nl, r), lambda: np.stack([owned(self.Or.rotate(c, r)) for c in self.rot_inputs(nl)[0]]))

    def rescale_inputs(self, nl):
        """the dropped limb = the boundary targets; the other limbs: one uniform ciphertext, one saturated"""
        def make():
            a = self.chain[nl][0]
            cts = [B.randomise(self.P, a.clone(), self.rng), B.saturate(self.P, a.clone())]
            for c in cts:
                B.craft_rescale_input(self.P, c)
            return cts, np.stack([c.data() for c in cts]), a.scale
        return self._memo(("resc_in", nl), make)

    def rescale_want(self, nl):
        def make():
            out = []
            for c in self.rescale_inputs(nl)[0]:
                d = c.clone()
                self.Or.rescale(d)
                out.append(owned(d))
            return np.stack(out)
        return self._memo(("resc", nl), make)


def check(got, want, src, tag):
    """every ciphertext of the batch against the oracle's result on the distinct input it was tiled from"""
    assert got.shape == (len(src),) + want.shape[1:], (tag, got.shape, want.shape)
    for i, s in enumerate(src):
        if not np.array_equal(got[i], want[s]):
            bad = np.argwhere(got[i] != want[s])
            p, j, c = (int(v) for v in bad[0])
            raise AssertionError("%s: ciphertext %d of %d (distinct input %d) differs from the oracle at %d residues; first: polynomial %d "
                                 "limb %d index %d: got %d, want %d" % (tag, i, len(src), s, len(bad), p, j, c, got[i][p, j, c], want[s][p, j, c]))


class ledger:
    """restart the byte ledger around one case of a sweep and note the kernel names it recorded"""

    def __init__(self, im, sweep, X):
        self.im, self.sweep, self.X = im, sweep, X

    def __enter__(self):
        self.im.byte_ledger(1)

    def __exit__(self, *exc):
        led = self.im.byte_ledger(0)
        if exc[0] is None:
            SEEN[self.sweep][self.X] = set(led)


def run_mult(R, cc, nl, X, tag):
    A, Bm, sa, sb = R.pair_data(nl)
    want = R.mult_want(nl)
    ba, _, src = B.tile(A, X)
    bb, _, _ = B.tile(Bm, X)
    ga, gb = cc.import_ct(ba, sa), cc.import_ct(bb, sb)
    del ba, bb
    g = cc.eval_mult(ga, gb)
    assert g.shape()[:3] == (X, 2, nl - 1)
    got = g.export()
    del ga, gb, g  # (the batch is freed before the next one is built)
    check(got, want, src, ("mult", tag, nl, X))


def run_steps(R, cc, nl, X, tag):
    A, Bm, sa, sb = R.pair_data(nl)
    want = R.steps_want(nl)
    ba, _, src = B.tile(A, X)
    bb, _, _ = B.tile(Bm, X)
    ga, gb = cc.import_ct(ba, sa), cc.import_ct(bb, sb)
    del ba, bb
    g = cc.eval_mult_no_relin(ga, gb)
    del ga, gb
    check(g.export(), want["norelin"], src, ("mult_no_relin", tag, nl, X))
    cc.relinearize(g)
    check(g.export(), want["relin"], src, ("relinearize", tag, nl, X))
    cc.rescale(g)
    check(g.export(), want["rescale"], src, ("rescale of the product", tag, nl, X))
    del g


def run_rotate(R, cc, nl, X, r, tag):
    _, data, scale = R.rot_inputs(nl)
    want = R.rot_want(nl, r)
    batch, _, src = B.tile(data, X)
    ga = cc.import_ct(batch, scale)
    del batch
    g = cc.eval_rotate(ga, r)
    got = g.export()
    del ga, g
    check(got, want, src, ("rotate", tag, nl, X, r))


def run_rescale(R, cc, nl, X, tag):
    _, data, scale = R.rescale_inputs(nl)
    want = R.rescale_want(nl)
    batch, _, src = B.tile(data, X)
    g = cc.import_ct(batch, scale)
    del batch
    cc.rescale(g)
    assert g.shape()[:3] == (X, 2, nl - 1)
    got = g.export()
    del g
    check(got, want, src, ("rescale", tag, nl, X))


@pytest.fixture(scope="module")
def full(im):
    P = O.Params()
    K = O.Keys(P, SEED, rotations=list(ROTATIONS))
    cc = im.Context()
    assert np.array_equal(cc.moduli, P.moduli) and np.array_equal(cc.roots, P.roots)
    cc.keygen_rotations(ROTATIONS, SEED)
    assert np.array_equal(cc.export_eval_key(0), K.relin()) and np.array_equal(cc.export_eval_key(1), K.rot_key(1))
    R = Rig(im, P, K, cc, (12, 9, 8, 7, 5, 4, 2, 1))
    yield R
    cc.close()


# ---------------------------------------------------------------- the default engine
@pytest.mark.parametrize("X", MULT_X)
def test_mult_12_limbs(full, X):
    """eval_mult (fused product, ModUp, inner product, merged ModDown + Rescale) at every X around the selection rules"""
    with ledger(full.im, "mult", X):
        run_mult(full, full.cc, 12, X, "default")


def test_mult_sweep_launches_both_forms_of_each_family(full):
    for X in MULT_X:  # (cases that did not run in this session, e.g. under -k, run here)
        if X not in SEEN["mult"]:
            with ledger(full.im, "mult", X):
                run_mult(full, full.cc, 12, X, "default")
    seen = set().union(*SEEN["mult"].values())
    for name in ("k_ntt15_colfuse8<true, 4>", "k_ntt15_conv_p1_8<true>", "k_ntt15_colfuse8<false, 4>", "k_ntt15_conv_p1_8<false>",
                 "k_ntt15_p1inv8"):
        assert name in seen, "%s was never launched by eval_mult at 12 limbs for X in %s (recorded: %s)" % (name, MULT_X, sorted(seen))


@pytest.mark.parametrize("X", (3, 16, 17))
def test_three_steps_12_limbs(full, X):
    """eval_mult_no_relin -> relinearize -> rescale, each step compared"""
    run_steps(full, full.cc, 12, X, "default")


@pytest.mark.parametrize("X", (3, 16, 17))
@pytest.mark.parametrize("nl", (9, 8, 5, 4, 2))
def test_mult_lower_limb_counts(full, nl, X):
    """9 and 5 limbs end on a partial digit, 4 is one digit (the unfused product), 2 rescales onto the 60-bit limb alone"""
    run_mult(full, full.cc, nl, X, "default")


@pytest.mark.parametrize("X", (3, 10, 11, 16, 17))
@pytest.mark.parametrize("nl", (12, 9, 5, 1))
@pytest.mark.parametrize("r", ROTATIONS)
def test_rotate(full, r, nl, X):
    run_rotate(full, full.cc, nl, X, r, "default")


@pytest.mark.parametrize("X", RESCALE_X)
@pytest.mark.parametrize("nl", (12, 7, 2))
def test_rescale_on_the_centring_boundary(full, nl, X):
    if nl == 12:
        with ledger(full.im, "rescale", X):
            run_rescale(full, full.cc, nl, X, "default")
    else:
        run_rescale(full, full.cc, nl, X, "default")


def test_rescale_sweep_takes_the_column_fused_form_from_128_ciphertexts(full):
    for X in RESCALE_X:
        if X not in SEEN["rescale"]:
            with ledger(full.im, "rescale", X):
                run_rescale(full, full.cc, 12, X, "default")
    cf = {X: sorted(k for k in names if k.startswith("k_ntt15_colfuse")) for X, names in SEEN["rescale"].items()}
    assert any(cf[X] for X in RESCALE_X if X >= 128), "no column-fused Rescale launch at X >= 128: %s" % SEEN["rescale"]
    assert not cf[3], "a column-fused Rescale launch at X = 3: %s" % cf[3]


@pytest.fixture(scope="module")
def scores(full):
    """two score-like ciphertexts at n_q - 1 limbs (slots over [-1, 1] with a dense stretch around the threshold 0.44) and the oracle's
    comparator on them — about 22 products each, shared by the batch sizes"""
    P, Or = full.P, full.Or
    h = P.slots // 2
    x0 = np.concatenate([np.linspace(-1, 1, h), np.linspace(0.40, 0.48, P.slots - h)])
    x1 = np.concatenate([np.linspace(0.47, 0.41, h), np.linspace(1, -1, P.slots - h)])
    data, want, scale = [], [], None
    for k, x in enumerate((x0, x1)):
        ct = Or.encrypt(x, 9, 70 + k)
        P.L.hyo_drop_to(P.h, ct.h, P.nQ - 1)
        data.append(owned(ct))
        want.append(owned(Or.chebyshev_compare(ct, 0.44, 10)))
        scale = ct.scale
    return np.stack(data), np.stack(want), scale


@pytest.mark.parametrize("X", (17, 32))
def test_comparator(full, scores, X):
    """chebyshev_compare on a batch: the doubling, subtrahend and added-constant epilogues of the merged tail in large launches"""
    data, want, scale = scores
    batch, _, src = B.tile(data, X)
    g = full.cc.import_ct(batch, scale)
    out = full.cc.chebyshev_compare(g, 0.44, 10)
    got = out.export()
    del g, out
    check(got, want, src, ("chebyshev_compare", X))


# ---------------------------------------------------------------- the engine switches, each in a fresh context
@pytest.fixture(scope="module", params=SWITCHES)
def switched(request, im, full):
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    os.environ[request.param] = "1"
    try:  # the switch is read when the context is created
        cc = im.Context()
    finally:
        del os.environ[request.param]
        os.environ.update(saved)
    cc.keygen_rotations(ROTATIONS, SEED)
    yield request.param, cc
    cc.close()


@pytest.mark.parametrize("X", (3, 16, 17, 129))
@pytest.mark.parametrize("nl", (12, 9))
@pytest.mark.parametrize("op", ("mult", "rotate", "rescale"))
def test_switches(full, switched, op, nl, X):
    name, cc = switched
    if op == "mult":
        run_mult(full, cc, nl, X, name)
    elif op == "rotate":
        for r in ROTATIONS:
            run_rotate(full, cc, nl, X, r, name)
    else:
        run_rescale(full, cc, nl, X, name)


# ---------------------------------------------------------------- the generic kernels (N = 2^11)
@pytest.fixture(scope="module")
def small(im):
    P = O.Params(log_n=11, depth=11, dim=64)
    K = O.Keys(P, SEED, rotations=[1])
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    cc.keygen_rotations([1], SEED)
    assert np.array_equal(cc.export_eval_key(0), K.relin())
    R = Rig(im, P, K, cc, (12, 2))
    yield R
    cc.close()


@pytest.mark.parametrize("X", (1, 5))
@pytest.mark.parametrize("nl", (12, 2))
def test_generic_ring(small, nl, X):
    """k_rescale_spread and the sequential relinearise + rescale on the crafted and saturated pairs"""
    run_mult(small, small.cc, nl, X, "2^11")
    run_steps(small, small.cc, nl, X, "2^11")
    run_rescale(small, small.cc, nl, X, "2^11")
