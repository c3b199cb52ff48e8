"""GPU parity on prime chains at the edges of the three butterfly arithmetics (image_matching_amd/csrc/ntt_arith.h; host contract check:
tests/csrc/ntt_arith_check.cpp).  The context picks FpA for primes of at most 47 bits (lean below 2^45 + 2^41), IntP for q = 2^60 - c
with c < 2^24 and IntA otherwise; a caller-supplied chain (hydia_ctx_create_custom) reaches every edge.  Transforms and the evaluator
are compared BIT-EXACTLY with the CPU oracle on the same chain, through the engine switches that change which arithmetic or which
kernel shape a limb takes.  The odd scaling primes distort the CKKS scale, so bit-exactness is the requirement, not decryption."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SWITCHES = ("HYDIA_NTT_1PASS", "HYDIA_NTT_1PASS_MIN", "HYDIA_P2_WG_SYNC", "HYDIA_NTT_GENERIC", "HYDIA_NO_TW_LDS", "HYDIA_NTT_NO_PM",
            "HYDIA_NTT_INT", "HYDIA_NO_COLFUSE", "HYDIA_COLFUSE_WIDE", "HYDIA_INT_EPILOGUE", "HYDIA_NO_FUSE_IP",
            "HYDIA_RELIN_TWO_IP_LAUNCHES")
NTT_VARIANTS = [{}, {"HYDIA_NTT_1PASS": "1", "HYDIA_NTT_1PASS_MIN": "1"}, {"HYDIA_P2_WG_SYNC": "1"}, {"HYDIA_NTT_GENERIC": "1"},
                {"HYDIA_NO_TW_LDS": "1"}, {"HYDIA_NTT_NO_PM": "1"}, {"HYDIA_NTT_INT": "1"}]
EVAL_VARIANTS = [{}, {"HYDIA_NO_COLFUSE": "1"}, {"HYDIA_COLFUSE_WIDE": "1"}, {"HYDIA_INT_EPILOGUE": "1"}, {"HYDIA_NO_FUSE_IP": "1"},
                 {"HYDIA_NTT_NO_PM": "1"}, {"HYDIA_RELIN_TWO_IP_LAUNCHES": "1"}]
LEAN_EDGE = (1 << 45) + (1 << 41)


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _prime_below(x, M):
    from sympy import isprime
    c = (x - 2) // M * M + 1
    while not isprime(c):
        c -= M
    return c


def _prime_above(x, M):
    from sympy import isprime
    c = (x // M + 1) * M + 1
    while not isprime(c):
        c += M
    return c


def intp_primes(log_n):
    """Every q = 2^60 - c, c < 2^24, prime and 1 mod 2N — the IntP rule of context.cpp — in increasing c."""
    from sympy import isprime
    M = 2 << log_n
    return [(1 << 60) - c for c in range(M - 1, 1 << 24, M) if isprime((1 << 60) - c)]


def edge_primes(log_n):
    """The edge moduli of each class at ring 2^log_n (as in the host check): lean-threshold pair, top 47-bit, ~2^30 (FpA); smallest
    48-bit, largest 59-bit, first 60-bit prime outside the IntP rule (IntA)."""
    M = 2 << log_n
    c = (1 << 24) + M - 1
    from sympy import isprime
    while not isprime((1 << 60) - c):
        c += M
    return {"lean_lo": _prime_below(LEAN_EDGE, M), "lean_hi": _prime_above(LEAN_EDGE, M), "top47": _prime_below(1 << 47, M),
            "p30": _prime_above(1 << 30, M), "p48": _prime_above(1 << 47, M), "p59": _prime_below(1 << 59, M), "intA60": (1 << 60) - c}


def test_edge_prime_selection_matches_the_issue_values():
    e = edge_primes(15)
    assert e["lean_lo"] == 37383394754561 and e["lean_hi"] == 37383395868673 and e["top47"] == 140737487306753
    assert e["p48"] == 140737488486401 and e["intA60"] == (1 << 60) - 0x101ffff
    assert [(1 << 60) - q for q in intp_primes(15)] == [0x3ffff, 0x7bffff, 0x95ffff, 0xa5ffff, 0xaaffff, 0xccffff, 0xd5ffff, 0xdbffff]


def transform_chain(log_n):
    """12 Q + 4 P limbs covering every edge prime of the ring: at N = 2^15 all eight IntP primes; at N = 2^11 the IntP extremes."""
    base = O.Params(log_n=log_n, depth=11, dim=64)
    default45 = [int(q) for q in base.moduli[1:12]]
    base.close()
    e = edge_primes(log_n)
    ip = intp_primes(log_n)
    if log_n == 11:
        ip = [ip[0], ip[1], ip[-2], ip[-1]]
    edge = [e["lean_lo"], e["lean_hi"], e["top47"], e["p30"], e["p48"], e["p59"], e["intA60"]]
    chain = [ip[-1]] + edge + ip[:-1]
    chain += [q for q in default45 if q not in chain][:16 - len(chain)]
    return np.array(chain, dtype=np.uint64)


@pytest.mark.parametrize("log_n", [15, 11])
def test_edge_prime_transforms_bit_exact(im, log_n, monkeypatch):
    """cc.ntt forward, inverse and round trip on every limb of an edge chain against the oracle, through every transform variant; odd
    (3) and even (6) polynomial counts so the pair path runs too.  Rows: random, all q - 1, alternating 0 / q - 1, impulses at 0 and
    N - 1, a constant."""
    moduli = transform_chain(log_n)
    P = O.Params(log_n=log_n, depth=11, dim=64, moduli=moduli, n_p=4)
    N = P.N
    rng = np.random.default_rng(log_n + 100)
    cases = []
    for m in range(P.nT):
        q = int(P.moduli[m])
        a = rng.integers(0, q, size=(6, N), dtype=np.uint64)
        a[1] = q - 1
        a[2] = 0
        a[2, 1::2] = q - 1
        a[3] = 0
        a[3, 0] = q - 1
        a[4] = 0
        a[4, N - 1] = 1
        a[5] = q // 3
        fwd = np.stack([P.ntt_fwd(r, m) for r in a])
        inv = np.stack([P.ntt_inv(r, m) for r in a])
        cases.append((m, a, fwd, inv))
    for env in NTT_VARIANTS:
        _set_env(monkeypatch, env)
        cc = im.Context(im.default_params(log_n=log_n, vector_dim=64), 0, moduli=moduli, roots=P.roots, n_p=4)
        _set_env(monkeypatch, {})
        assert np.array_equal(cc.moduli, P.moduli)
        for m, a, fwd, inv in cases:
            for rows in (slice(0, 3), slice(0, 6)):
                got = cc.ntt(a[rows], m)
                assert np.array_equal(got, fwd[rows]), (env, m, int(P.moduli[m]))
                assert np.array_equal(cc.ntt(got, m, inverse=True), a[rows]), (env, m)
                assert np.array_equal(cc.ntt(a[rows], m, inverse=True), inv[rows]), (env, m)
        cc.close()
    P.close()


def evaluator_chain(log_n):
    """12 Q + 4 P limbs (dnum stays 3): q_0 the IntP prime with the largest c; scaling primes the lean-edge pair, the top 47-bit prime,
    the smallest 48-bit (IntA) prime and default 45-bit primes; special primes the two next-largest-c IntP primes, the first IntA
    60-bit prime and one default special prime."""
    base = O.Params(log_n=log_n, depth=11, dim=64)
    default = [int(q) for q in base.moduli]
    base.close()
    e = edge_primes(log_n)
    ip = intp_primes(log_n)
    scal = [e["lean_lo"], e["lean_hi"], e["top47"], e["p48"]]
    scal += [q for q in default[1:12] if q not in scal][:11 - len(scal)]
    special = [ip[-3], ip[-2], e["intA60"]] + [q for q in default[12:] if q not in ip[-3:]][:1]
    return np.array([ip[-1]] + scal + special, dtype=np.uint64)


def _owned(ct):
    """A copy of an oracle ciphertext's residues, taken while the ciphertext is alive (data() is a view into it)."""
    return ct.data().copy()


def _evaluator_reference(P, Or, rng):
    z, w = rng.uniform(-1, 1, P.slots), rng.uniform(-1, 1, P.slots)
    a, b = Or.encrypt(z, 1, 1), Or.encrypt(w, 1, 2)
    d = Or.mult_norelin(a, b)
    want = {"norelin": d.data().copy()}
    Or.relin(d)
    want["relin"] = d.data().copy()
    Or.rescale(d)
    want["rescale"] = d.data().copy()
    want["rot"] = {r: _owned(Or.rotate(a, r)) for r in (1, 5, P.slots // 2)}
    chain, cur = [], a
    while cur.nl > 1:
        cur = Or.mult(cur, cur)
        chain.append(cur.data().copy())
    want["chain"] = chain
    want["rot_low"] = _owned(Or.rotate(cur, 3))
    return a, b, want


def _evaluator_check(cc, P, a, b, want, tag):
    ga, gb = cc.import_ct(a.data(), a.scale), cc.import_ct(b.data(), b.scale)
    gd = cc.eval_mult_no_relin(ga, gb)
    assert np.array_equal(gd.export()[0], want["norelin"]), tag
    cc.relinearize(gd)
    assert np.array_equal(gd.export()[0], want["relin"]), tag
    cc.rescale(gd)
    assert np.array_equal(gd.export()[0], want["rescale"]), tag
    for r, v in want["rot"].items():
        assert np.array_equal(cc.eval_rotate(ga, r).export()[0], v), (tag, r)
    g = ga
    for lvl, v in enumerate(want["chain"]):  # multiply (relinearise, rescale) down to one limb
        g = cc.eval_mult(g, g)
        assert np.array_equal(g.export()[0], v), (tag, lvl)
    assert np.array_equal(cc.eval_rotate(g, 3).export()[0], want["rot_low"]), tag  # a partial digit at the last level


def test_edge_chain_evaluator_and_sender_full_ring(im, monkeypatch):
    """N = 2^15 edge chain: mult-no-relin, relinearise, rescale, rotations at every level down to one limb, and a one-block
    computeSimilarity / indexScenario (hoisted rotations of the query, ModDown conversions into the largest-c IntP limbs) equal the
    oracle's on the same chain, bit for bit, through the default engine and each arithmetic-relevant switch."""
    moduli = evaluator_chain(15)
    P = O.Params(moduli=moduli, n_p=4)
    assert (P.nQ, P.nP, P.dnum) == (12, 4, 3)
    K = O.Keys(P, 21)
    Or = O.Oracle(P, K)
    a, b, want = _evaluator_reference(P, Or, np.random.default_rng(15))
    n = 3000
    rng = np.random.default_rng(16)
    db = rng.integers(-99, 100, size=(n, 512)).astype(np.float64)
    db[11] = rng.integers(1, 4, size=512)
    query = np.ones(512)
    dbc = Or.enroll(db.copy(), 8, matvec="hoisted")
    q = Or.encrypt_query(query, 2, 9)
    sim_arr, idx_arr = Or.compute_similarity(q, dbc, n), Or.index_scenario(q, dbc, n)  # (the arrays own the ciphertexts)
    sim, idx = sim_arr[0].data().copy(), idx_arr[0].data().copy()
    for env in EVAL_VARIANTS:
        _set_env(monkeypatch, env)
        cc = im.Context(im.default_params(), 0, moduli=moduli, roots=P.roots, n_p=4)
        _set_env(monkeypatch, {})
        assert np.array_equal(cc.moduli, P.moduli)
        cc.keygen(21)
        assert np.array_equal(cc.export_eval_key(0), K.relin()) and np.array_equal(cc.export_eval_key(1), K.rot_key(1)), env
        _evaluator_check(cc, P, a, b, want, env)
        cc.set_matvec("hoisted")
        im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=8)
        gq = im.DiagonalReceiver(cc, n).encryptQuery(query, seed=2, nonce=9)
        assert np.array_equal(gq.export()[0], q.data()), env
        sender = im.DiagonalSender(cc, n)
        assert np.array_equal(sender.computeSimilarity(gq).export()[0], sim), env
        assert np.array_equal(sender.indexScenario(gq).export()[0], idx), env
        cc.close()
    P.close()


def test_edge_chain_multi_block_small_ring(im, monkeypatch):
    """The same chain shape at N = 2^11, dim 64: evaluator primitives, every hoisted rotation of the query, and a 10-block
    group-sequential database (which takes the residue-width fallback: a scaling prime is 2^46 or wider) through the multi-block
    sender, bit for bit against the oracle, for the default engine and each arithmetic-relevant switch."""
    moduli = evaluator_chain(11)
    P = O.Params(log_n=11, depth=11, dim=64, moduli=moduli, n_p=4)
    assert (P.nQ, P.nP, P.dnum) == (12, 4, 3)
    K = O.Keys(P, 5)
    Or = O.Oracle(P, K)
    a, b, want = _evaluator_reference(P, Or, np.random.default_rng(11))
    blocks = 10
    n = blocks * P.slots - 3
    rng = np.random.default_rng(12)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    db[n // 3] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    dbc = Or.enroll(db.copy(), 4, matvec="hoisted")
    q = Or.encrypt_query(query, 6, 1)
    rot_arr = Or.rotate_query(q)
    rot = [rot_arr[i].data().copy() for i in range(P.dim)]
    sim, idx = Or.compute_similarity(q, dbc, n), Or.index_scenario(q, dbc, n)
    assert len(sim) == blocks
    for env in EVAL_VARIANTS:
        _set_env(monkeypatch, env)
        cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0, moduli=moduli, roots=P.roots, n_p=4)
        _set_env(monkeypatch, {})
        cc.keygen(5)
        _evaluator_check(cc, P, a, b, want, env)
        cc.set_matvec("hoisted")
        im.DiagonalEnroller(cc, n).serializeDB(db.copy(), seed=4)
        assert cc.db_kind() == 5 and cc.db_residue_bits() == 48, env  # group-sequential, 48-bit residue fallback
        gq = im.DiagonalReceiver(cc, n).encryptQuery(query, seed=6, nonce=1)
        assert np.array_equal(gq.export()[0], q.data()), env
        sender = im.DiagonalSender(cc, n)
        grot = sender.rotateQuery(gq).export()
        for i in range(P.dim):
            assert np.array_equal(grot[i], rot[i]), (env, i)
        gsim, gidx = sender.computeSimilarity(gq).export(), sender.indexScenario(gq).export()
        for g in range(blocks):
            assert np.array_equal(gsim[g], sim[g].data()) and np.array_equal(gidx[g], idx[g].data()), (env, g)
        cc.close()
    P.close()
