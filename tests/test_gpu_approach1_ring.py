"""GPU (run with -m gpu): the pieces of approach 1 (literature baseline) that exist so far, bit exact against the CPU oracle —
hydia_keygen_rotations, the plaintext-mask multiply (new kernel k_mul_plain), binaryRotate — and the first run of the N = 2^16 ring
approach 1 needs (hydia_params_for_approach): key generation, encryption, decryption, mult, rotate, rescale and the comparator."""
import math

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def approach1_rotations(slots):
    """{2^k} u {slots - 2^k}: every rotation approach 1's EvalSum, merge and placement steps decompose into."""
    s, k = set(), 1
    while k < slots:
        s.update((k, slots - k))
        k *= 2
    return sorted(s)


def binary_rotations(factor, slots):
    """OpenFHEWrapper::binaryRotate's greedy signed decomposition (src/openFHE_wrapper.cpp:111-121), each step mod slots."""
    out = []
    while factor != 0:
        sign = 1 if factor > 0 else -1
        bc = int(2 ** math.floor(math.log2(abs(factor)) + 0.5))  # C round(): half away from zero
        if (bc * sign) % slots:
            out.append((bc * sign) % slots)
        factor -= bc * sign
    return out


def oracle_mult_plain(P, Or, ct, v):
    """EvalMult(ct, MakeCKKSPackedPlaintext(v)) + rescale: v encoded at 2^scale_bits on ct's limbs, residue-wise product."""
    m = P.encode(v, scale=P.delta, nl=ct.nl).astype(object)
    out = O.Ct(P, P.L.hyo_ct_alloc(P.h, 2, ct.nl, ct.scale * P.delta))
    src, dst = ct.data(), out.data()
    for j in range(ct.nl):
        q = int(P.moduli[j])
        for p in range(2):
            dst[p, j] = np.array((src[p, j].astype(object) * m[j]) % q, dtype=np.uint64)
    Or.rescale(out)
    return out


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module")
def small(im):
    """2^11 ring with approach 1's chain (depth 13), 64-dim vectors, the approach-1 key set."""
    P = O.Params(log_n=11, depth=13, dim=64)
    rots = approach1_rotations(P.slots)
    K = O.Keys(P, 7, rotations=rots)
    cc = im.Context(im.default_params(log_n=11, mult_depth=13, vector_dim=64), 0)
    cc.keygen_rotations(rots, seed=7)
    yield P, K, O.Oracle(P, K), cc, rots
    cc.close()


def test_keygen_rotations_bit_exact(im, small):
    P, K, Or, cc, rots = small
    assert np.array_equal(cc.export_secret_key(), K.s_ntt())
    assert np.array_equal(cc.export_public_key(), K.pk())
    assert np.array_equal(cc.export_eval_key(0), K.relin())
    for r in rots:
        assert np.array_equal(cc.export_eval_key(r), K.rot_key(r)), r
    assert not cc.has_eval_key(3) and not cc.has_eval_key(P.slots - 3)
    # a key in hydia_keygen's set too is bit-identical to it; negative rotations name slots + r; keys outside a new set are released
    other = im.Context(im.default_params(log_n=11, mult_depth=13, vector_dim=64), 0)
    other.keygen(7)
    for r in (1, 2, 64, 512):
        assert np.array_equal(other.export_eval_key(r), K.rot_key(r)), r
    other.keygen_rotations([-1, 3], seed=7)
    assert np.array_equal(other.export_eval_key(P.slots - 1), K.rot_key(P.slots - 1))
    assert other.has_eval_key(3) and not other.has_eval_key(1) and not other.has_eval_key(64)
    with pytest.raises(im.HydiaError):
        other.keygen_rotations([P.slots], seed=7)
    other.close()


@pytest.mark.parametrize("f", [1, -1, 3, -3, 511, -192, 1023])
def test_binary_rotate_bit_exact(small, f):
    P, K, Or, cc, rots = small
    rng = np.random.default_rng(1000 + f)
    z = rng.uniform(-1, 1, P.slots)
    ct = Or.encrypt(z, 3, 9)
    want = ct
    for r in binary_rotations(f, P.slots):
        want = Or.rotate(want, r)
    got = cc.binary_rotate(cc.import_ct(ct.data(), ct.scale), f)
    assert np.array_equal(got.export()[0], want.data())
    assert np.abs(cc.decrypt(got)[0] - np.roll(z, -f)).max() < 1e-6


def test_eval_mult_plain_bit_exact(small):
    """the merge mask multiply, twice in a row (each product rescaled: one limb less every time)"""
    P, K, Or, cc, rots = small
    rng = np.random.default_rng(5)
    z = rng.uniform(-1, 1, P.slots)
    mask = np.zeros(P.slots)
    mask[::P.dim] = 1.0  # generateMergeMask(dim, 1)
    ct = Or.encrypt(z, 4, 2)
    for _ in range(2):
        g = cc.eval_mult_plain(cc.import_ct(ct.data(), ct.scale), mask)
        want = oracle_mult_plain(P, Or, ct, mask)
        assert g.shape()[2:] == (want.nl, want.scale)
        assert np.array_equal(g.export()[0], want.data())
        assert np.abs(cc.decrypt(g)[0] - z * mask).max() < 1e-6
        ct = want


def test_ring_2p16_bring_up(im):
    """approach 1's context (hydia_params_for_approach(1): N = 2^16, 14 + 5 limbs) against the oracle, bit for bit."""
    p = im.params_for_approach(1)
    assert p.log_n == 16 and p.mult_depth == 13
    P = O.Params(log_n=16, depth=13, dim=512)
    cc = im.Context(p, 0)
    assert (cc.N, cc.nQ, cc.nP) == (P.N, P.nQ, P.nP) and np.array_equal(cc.moduli, P.moduli)
    rots = [1, 256, P.slots - 1]
    K = O.Keys(P, 21, rotations=rots)
    Or = O.Oracle(P, K)
    cc.keygen_rotations(rots, seed=21)
    assert np.array_equal(cc.export_secret_key(), K.s_ntt())
    assert np.array_equal(cc.export_public_key(), K.pk())
    assert np.array_equal(cc.export_eval_key(0), K.relin())
    for r in rots:
        assert np.array_equal(cc.export_eval_key(r), K.rot_key(r)), r
    rng = np.random.default_rng(16)
    za, zb = rng.uniform(-1, 1, P.slots), rng.uniform(-1, 1, P.slots)
    ga = cc.encrypt(np.stack([za, zb]), 8, 30)
    a, b = Or.encrypt(za, 8, 30), Or.encrypt(zb, 8, 31)
    data = ga.export()
    assert np.array_equal(data[0], a.data()) and np.array_equal(data[1], b.data())
    dec = cc.decrypt(ga)
    assert np.array_equal(dec[0], Or.decrypt(a)) and np.abs(dec[0] - za).max() < 1e-7
    gA, gB = cc.import_ct(a.data(), a.scale), cc.import_ct(b.data(), b.scale)
    m = Or.mult(a, b)
    gm = cc.eval_mult(gA, gB)
    assert np.array_equal(gm.export()[0], m.data())
    assert np.abs(cc.decrypt(gm)[0] - za * zb).max() < 1e-6
    for r in (1, P.slots - 1):
        assert np.array_equal(cc.eval_rotate(gA, r).export()[0], Or.rotate(a, r).data()), r
    gs = cc.import_ct(a.data(), a.scale)
    cc.rescale(gs)
    s = a.clone()
    Or.rescale(s)
    assert np.array_equal(gs.export()[0], s.data())
    # the comparator at the level approach 1 reaches it (1 + 2 rescales: 11 limbs, scale 2^45)
    x = Or.encrypt(0.8 * za, 8, 40)
    P.L.hyo_drop_to(P.h, x.h, P.nQ - 3)
    gc = cc.chebyshev_compare(cc.import_ct(x.data(), x.scale))
    c = Or.chebyshev_compare(x)
    assert np.array_equal(gc.export()[0], c.data())
    cc.close()
