"""CPU-only: the ring rule of hydia_params_for_approach (include/hydia.h) — the context ./ImageMatching <file> <approach> needs."""
import math

import pytest


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


def log_qp(im, p):
    _, moduli, _ = im.describe_params(p)
    return sum(math.log2(int(m)) for m in moduli)


def test_params_for_approach_picks_the_ring(im):
    """HEStd_128_classic: depth 11 (approaches 4, 5) fits 2^15 (881 bits); depth 13 (approach 1: 14 Q limbs, 5 special primes) does
    not, so approach 1 runs on 2^16 (1772 bits)."""
    d = im.default_params()
    for approach, log_n, depth in ((5, 15, 11), (4, 15, 11), (1, 16, 13)):
        p = im.params_for_approach(approach)
        assert (p.log_n, p.mult_depth) == (log_n, depth), approach
        assert (p.scale_bits, p.first_mod_bits, p.dnum, p.vector_dim) == (d.scale_bits, d.first_mod_bits, d.dnum, d.vector_dim)
    assert im.params_for_approach(5).log_n == d.log_n  # the default context is approach 5's
    p1 = im.params_for_approach(1)
    info, _, _ = im.describe_params(p1)
    assert (info["n_q"], info["n_p"], info["alpha"]) == (14, 5, 5)
    assert 881 < log_qp(im, im.default_params(mult_depth=13)) <= 1772
    assert log_qp(im, im.default_params()) <= 881


def test_params_for_approach_rejects_unknown(im):
    for a in (0, 6):
        with pytest.raises(im.HydiaError):
            im.params_for_approach(a)
