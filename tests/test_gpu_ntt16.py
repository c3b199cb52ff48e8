"""GPU (run with -m gpu): the two-pass register-radix transforms of the N = 2^16 ring (image_matching_amd/csrc/ntt16.hip; host check of
their schedule and lazy bounds: tests/test_ntt16_host.py).  They are opt-in (HYDIA_NTT16=1 when the context is created; the default on
that ring stays the ring-size-generic kernels until the new ones are measured).  With the switch every
transform of the generic pipeline goes through them, so they are compared BIT-EXACTLY with the CPU oracle on an edge-prime chain,
through the arithmetic switches and against the generic kernels, and through the evaluator, which reaches what hydia_ntt alone does
not: limb selections, separate source and destination strides, limb-prefix views, in-place use."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_edge_primes import _set_env, transform_chain

pytestmark = pytest.mark.gpu

ON = {"HYDIA_NTT16": "1"}
VARIANTS = [ON, dict(ON, HYDIA_NTT_INT="1"), dict(ON, HYDIA_NTT_NO_PM="1"), dict(ON, HYDIA_NTT_GENERIC="1"), {}]
PAIR_ROWS = np.arange(64) % 6  # the six reference rows, repeated: 64 polynomials of one limb


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def _env(monkeypatch, env):
    """test_gpu_edge_primes' switches cleared, then env (which may hold HYDIA_NTT16, a switch that module does not know)"""
    monkeypatch.delenv("HYDIA_NTT16", raising=False)
    _set_env(monkeypatch, env)


def test_engine_reports_the_ring(im, monkeypatch):
    """ntt_engine follows what actually runs: the 2^16 transforms only under HYDIA_NTT16=1 (read when the context is created), never
    under HYDIA_NTT_GENERIC=1, and on no other ring."""
    def engine(params, env):
        _env(monkeypatch, env)
        cc = im.Context(params, 0)
        _env(monkeypatch, {})
        e, n = cc.ntt_engine, cc.N
        cc.close()
        return e, n

    p16 = im.params_for_approach(3)
    assert engine(p16, ON) == (16, 1 << 16)
    assert engine(p16, {}) == (0, 1 << 16)
    assert engine(p16, dict(ON, HYDIA_NTT_GENERIC="1")) == (0, 1 << 16)
    assert engine(im.default_params(), {}) == (15, 1 << 15)
    assert engine(im.default_params(), ON) == (15, 1 << 15)
    assert engine(im.default_params(log_n=11, vector_dim=64), ON) == (0, 1 << 11)


def test_edge_prime_transforms_bit_exact_2p16(im, monkeypatch):
    """cc.ntt forward, inverse and round trip on every limb of the 2^16 edge chain against the oracle: the six IntP primes 2^60 - c, the
    lean-edge pair, the top 47-bit prime, ~2^30, the three IntA edges and three default 45-bit primes.  Rows: random, all q - 1,
    alternating 0 / q - 1, impulses at 0 and N - 1, a constant; HYDIA_NTT16=1 alone, with HYDIA_NTT_INT, HYDIA_NTT_NO_PM and
    HYDIA_NTT_GENERIC, and the default (generic) engine; 1, 3 and 6 rows per call, and 64 (the six repeated), where pass 2 pairs
    polynomials.  Under HYDIA_NTT16=1 alone the launches are
    k_ntt16_p1 / k_ntt16_p2 and no other transform kernel."""
    moduli = transform_chain(16)
    assert len(moduli) == 16
    chain = [int(q) for q in moduli]
    assert sorted((1 << 60) - q for q in chain if q > (1 << 60) - (1 << 24)) == [0x3ffff, 0x7bffff, 0x95ffff, 0xa5ffff, 0xd5ffff, 0xdbffff]
    for q in (37383392985089, 37383395868673, 140737487306753, 1073872897, 140737488486401, 576460752300015617, (1 << 60) - 0x101ffff):
        assert q in chain, q
    # (the remaining three are default 45-bit scaling primes)
    P = O.Params(log_n=16, depth=11, dim=64, moduli=moduli, n_p=4)
    N = P.N
    rng = np.random.default_rng(116)
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
    for env in VARIANTS:
        _env(monkeypatch, env)
        cc = im.Context(im.default_params(log_n=16, vector_dim=64), 0, moduli=moduli, roots=P.roots, n_p=4)
        _env(monkeypatch, {})
        assert np.array_equal(cc.moduli, P.moduli)
        assert cc.ntt_engine == (16 if "HYDIA_NTT16" in env and "HYDIA_NTT_GENERIC" not in env else 0)
        im.byte_ledger(1)
        for m, a, fwd, inv in cases:
            for rows in (slice(0, 1), slice(0, 3), slice(0, 6)):
                got = cc.ntt(a[rows], m)
                assert np.array_equal(got, fwd[rows]), (env, m, int(P.moduli[m]))
                assert np.array_equal(cc.ntt(got, m, inverse=True), a[rows]), (env, m)
                assert np.array_equal(cc.ntt(a[rows], m, inverse=True), inv[rows]), (env, m)
            # 64 rows on one limb: the smallest even count at which pass 2 takes two polynomials per workgroup (k_ntt16_p2<*, 2>)
            got = cc.ntt(a[PAIR_ROWS], m)
            assert np.array_equal(got, fwd[PAIR_ROWS]), (env, m, "paired")
            assert np.array_equal(cc.ntt(got, m, inverse=True), a[PAIR_ROWS]), (env, m, "paired")
            assert np.array_equal(cc.ntt(a[PAIR_ROWS], m, inverse=True), inv[PAIR_ROWS]), (env, m, "paired")
        led = im.byte_ledger(0)
        if env == ON:
            names = [k for k in led if k.startswith("k_ntt")]
            assert any(k.startswith("k_ntt16_p1<false") for k in names) and any(k.startswith("k_ntt16_p1<true") for k in names), led
            assert any(k.startswith("k_ntt16_p2<false") for k in names) and any(k.startswith("k_ntt16_p2<true") for k in names), led
            # no transform of the 2^15 family ran.  (The ring-size-generic kernels record no ledger lines, so a quiet fall-back to them
            # would not show as a name here: the launch and byte counts below are what pins every transform to k_ntt16_*.)
            assert all(k.startswith("k_ntt16_p1") or k.startswith("k_ntt16_p2") for k in names), names
            launches = 3 * 4 * P.nT  # three transforms per call, four calls per limb
            nbytes = 3 * (1 + 3 + 6 + 64) * P.nT * 2 * N * 8
            for kern in ("k_ntt16_p1", "k_ntt16_p2"):
                assert sum(led[k][0] for k in names if k.startswith(kern)) == launches, (kern, led)
                assert sum(led[k][1] for k in names if k.startswith(kern)) == nbytes, (kern, led)
            # one polynomial per workgroup below 64 rows, two at 64
            # (one forward and two inverse transforms per row count)
            assert led["k_ntt16_p2<false, 1>"][0] == 3 * P.nT and led["k_ntt16_p2<true, 1>"][0] == 2 * 3 * P.nT, led
            assert led["k_ntt16_p2<false, 2>"][0] == P.nT and led["k_ntt16_p2<true, 2>"][0] == 2 * P.nT, led
        cc.close()
    P.close()


def test_evaluator_on_the_2p16_ring_through_both_engines(im, monkeypatch):
    """approach 3's chain (13 + 5 limbs): eval_mult, eval_rotate(., 1) and rescale of two encryptions at full level and at 2 limbs, and
    eval_mult with one operand a limb-prefix view of the full ciphertext, equal the oracle's bit for bit under HYDIA_NTT16=1 and
    under the default (generic) engine — hence identical bytes between the two."""
    p = im.params_for_approach(3)
    P = O.Params(log_n=16, depth=12, dim=512)
    rots = [1, P.slots - 1]
    K = O.Keys(P, 33, rotations=rots)
    Or = O.Oracle(P, K)
    rng = np.random.default_rng(316)
    a, b = Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 10), Or.encrypt(rng.uniform(-1, 1, P.slots), 4, 11)
    a2, b2 = a.clone(), b.clone()
    P.L.hyo_drop_to(P.h, a2.h, 2)
    P.L.hyo_drop_to(P.h, b2.h, 2)
    want = {}
    for tag, x, y in (("full", a, b), ("two", a2, b2)):
        m, r = Or.mult(x, y), Or.rotate(x, 1)  # (kept alive while copied: data() is a view into the ciphertext)
        want[tag, "mult"] = m.data().copy()
        want[tag, "rot"] = r.data().copy()
        s = x.clone()
        Or.rescale(s)
        want[tag, "rescale"] = s.data().copy()
    got = {}
    for env in (ON, {}):
        _env(monkeypatch, env)
        cc = im.Context(p, 0)
        _env(monkeypatch, {})
        assert np.array_equal(cc.moduli, P.moduli) and cc.ntt_engine == (16 if env else 0)
        cc.keygen_rotations(rots, seed=33)
        res = {}
        for tag, x, y in (("full", a, b), ("two", a2, b2)):
            gx, gy = cc.import_ct(x.data(), x.scale), cc.import_ct(y.data(), y.scale)
            res[tag, "mult"] = cc.eval_mult(gx, gy).export()[0]
            res[tag, "rot"] = cc.eval_rotate(gx, 1).export()[0]
            gs = cc.import_ct(x.data(), x.scale)
            cc.rescale(gs)
            res[tag, "rescale"] = gs.export()[0]
        full = cc.import_ct(a.data(), a.scale)
        view = cc.ct_limb_prefix(full, 2)  # two limbs in use, the full ciphertext's limb stride
        res["two", "mult_view"] = cc.eval_mult(view, cc.import_ct(b2.data(), b2.scale)).export()[0]
        for key, v in res.items():
            ref = want[key[0], "mult" if key[1] == "mult_view" else key[1]]
            assert v.shape == ref.shape and np.array_equal(v, ref), (env, key)
        got[bool(env)] = res
        del view, full
        cc.close()
    for key in got[False]:
        assert got[False][key].tobytes() == got[True][key].tobytes(), key
    P.close()
