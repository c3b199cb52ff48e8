"""GPU test of the one piece of arithmetic the three batch modes share on the host: the number of passes over the database that the
`op:loop_b_*multi` entry of the byte ledger charges.  The launcher serves a batch of Q queries `width` at a time and what is left over
with the narrower widths (a last odd query alone), so 5 queries take 4+1, 2+2+1 or five passes at widths 4, 2, 1, and the encrypted
batch (width 2) takes 2+1 for 3 queries.  The pass counts below are written out by hand, not computed by the code under test.

Smallest shapes that tell the schedules apart: ring 2^11, vector_dim 64, two database blocks; Q = 5 is the smallest batch where the
three widths give three different schedules, Q = 3 the smallest where the encrypted batch has a leftover pass.  Results are not
looked at (random evaluation keys, random or zero database): the batch suites compare them bit for bit with the single calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N_VECTORS, BLOCKS = 64, 2048, 2  # 1024 slots per block at ring 2^11


@pytest.fixture(scope="module")
def cc():
    import image_matching_amd as im
    c = im.Context(im.default_params(log_n=11, vector_dim=DIM), 0)
    c.fill_eval_keys_random(1)
    yield c
    c.close()


def _residues(cc, polys, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, int(m), size=(polys, cc.N), dtype=np.uint64) for m in cc.moduli[:cc.nQ]], axis=1)


def _op_entry(cc, op, call):
    import image_matching_amd as im
    im.byte_ledger(1)
    out = call()
    cc.sync()
    led = im.byte_ledger(0)
    del out
    return led[op]


def _expected(cc, passes, Q, R, qp, comps):
    """passes * db_cts * ct_bytes + (Q R qp + Q G NG comps) n_q N 8, with R babies and NG = DIM / R giants per block"""
    NG = DIM // R
    return passes * cc.db_stats()[2] + (Q * R * qp + Q * BLOCKS * NG * comps) * cc.nQ * cc.N * 8


# (babies R): 64 = hoisted (kinds 5 / 7), 16 = a BSGS split with four giants per block (kinds 6 / 8)
@pytest.mark.parametrize("babies", [64, 16])
def test_encrypted_batch_charges_two_passes_for_three_queries(cc, babies):
    import image_matching_amd as im
    cc.set_matvec("hoisted" if babies == DIM else babies)
    cc.db_fill_random(N_VECTORS, 2)
    assert cc.db_kind() == (5 if babies == DIM else 6) and cc.db_babies() == babies and cc.db_stats()[1] == BLOCKS * DIM
    sender = im.DiagonalSender(cc, N_VECTORS)
    qs = [cc.import_ct(_residues(cc, 2, 10 + i), cc.delta) for i in range(3)]
    launches, nbytes = _op_entry(cc, "op:loop_b_multi", lambda: sender.computeSimilarityMulti(qs))
    print("op:loop_b_multi babies", babies, "launches", launches, "bytes", nbytes, "expected", _expected(cc, 2, 3, babies, 2, 3))
    assert launches == 1  # the batch was not cut by free memory: the formula applies
    assert nbytes == _expected(cc, 2, 3, babies, 2, 3)  # width 2: 2 + 1


WIDTH_PASSES = [(4, 2), (2, 3), (1, 5)]  # 5 queries: 4 + 1, 2 + 2 + 1, five 1s


@pytest.mark.parametrize("babies", [64, 16])
def test_plain_query_batch_charges_the_schedule_of_its_width(cc, babies):
    import image_matching_amd as im
    cc.set_matvec("hoisted" if babies == DIM else babies)
    cc.db_fill_random(N_VECTORS, 3)
    assert cc.db_kind() == (5 if babies == DIM else 6) and cc.db_stats()[1] == BLOCKS * DIM
    sender = im.DiagonalSender(cc, N_VECTORS)
    pts = [cc.pt_import(_residues(cc, 1, 20 + i)[0]) for i in range(5)]
    try:
        for width, passes in WIDTH_PASSES:
            cc.set_pq_batch_width(width)
            launches, nbytes = _op_entry(cc, "op:loop_b_pq_multi", lambda: sender.computeSimilarityPlainMulti(pts))
            print("op:loop_b_pq_multi babies", babies, "width", width, "launches", launches, "bytes", nbytes, "expected",
                  _expected(cc, passes, 5, babies, 1, 2))
            assert launches == 1
            assert nbytes == _expected(cc, passes, 5, babies, 1, 2), width
    finally:
        cc.set_pq_batch_width(0)


@pytest.mark.parametrize("babies", [64, 16])
def test_gallery_batch_charges_the_schedule_of_its_width(cc, babies):
    import image_matching_amd as im
    cc.plain_db_alloc(N_VECTORS, babies)  # a zero gallery
    assert cc.db_kind() == (7 if babies == DIM else 8) and cc.db_stats()[1] == BLOCKS * DIM
    sender = im.DiagonalSender(cc, N_VECTORS)
    qs = [cc.import_ct(_residues(cc, 2, 30 + i), cc.delta) for i in range(5)]
    try:
        for width, passes in WIDTH_PASSES:
            cc.set_gallery_batch_width(width)
            launches, nbytes = _op_entry(cc, "op:loop_b_plain_multi", lambda: sender.computeSimilarityGalleryMulti(qs))
            print("op:loop_b_plain_multi babies", babies, "width", width, "launches", launches, "bytes", nbytes, "expected",
                  _expected(cc, passes, 5, babies, 2, 2))
            assert launches == 1
            assert nbytes == _expected(cc, passes, 5, babies, 2, 2), width
    finally:
        cc.set_gallery_batch_width(0)
