"""CPU-only checks of approach 2 (GROTE group testing): the host-only entries, the plain model's decoding, and the oracle restatement
of tests/approach2_ref.py decrypted against the plain model.  Only the parts that need no product entry pass without approach 2."""
import numpy as np
import pytest

import approach1_ref as A
import approach2_ref as G
import oracle_lib as O

TOL = 1e-4  # src/main_accuracy.cpp:359-360


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module")
def small():
    """2^11 ring with approach 2's chain (depth 18: 19 limbs), 64-dim vectors: vpc 16, rowLength 32, colLength 32"""
    P = O.Params(log_n=11, depth=18, dim=64)
    K = O.Keys(P, 7, rotations=A.approach1_rotations(P.slots))
    return P, K, O.Oracle(P, K)


def test_row_length(im):
    assert [im.grote_row_length(s) for s in (1024, 2048, 32768)] == [32, 64, 256]
    assert [G.row_length(s) for s in (1024, 2048, 32768)] == [32, 64, 256]
    assert im.load_library().hydia_grote_row_length(48) == 0


def test_params_for_approach_2(im):
    info, moduli, _ = im.describe_params(im.params_for_approach(2))
    assert (info["log_n"], info["n_q"], info["n_p"], info["alpha"]) == (16, 19, 6, 7) and len(moduli) == 25


def cosines(n, planted, seed, dim=64):
    rng = np.random.default_rng(seed)
    db = rng.integers(-99, 100, size=(n, dim)).astype(np.float64)
    for i in planted:
        db[i] = rng.integers(1, 4, size=dim)
    query = np.ones(dim)
    return db, query, (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (query / np.linalg.norm(query))


@pytest.mark.parametrize("n,seed,planted,want", [(40, 3, [23], [23]), (40, 3, [], []), (1100, 11, [2, 1061], [2, 1061]),
                                                 (1100, 11, [2, 1061, 1099], [2, 1061, 1067, 1093, 1099])])
def test_plain_model_decoding(n, seed, planted, want):
    """the sums the group test compares: non-matching at most 0.012, matching at least 0.63 (so inside the comparator's [-1, 1] and far
    from the threshold 0.44^4 on either side); three matches of one matrix on two rows and two columns decode to all four crossings"""
    slots = 1024
    assert G.no_shared_line(planted, slots)
    _, _, cos = cosines(n, planted, seed)
    scores = G.score_vectors(cos, slots)
    rl = G.row_length(slots)
    rows, cols = G.plain_rows(scores, rl), G.plain_cols(scores, rl)
    hit_r = {i // rl for i in planted}
    hit_c = {(i // slots) * rl + i % rl for i in planted}
    for vals, hit in ((rows, hit_r), (cols, hit_c)):
        for k, v in enumerate(vals):
            assert (0.63 <= v <= 1.0) if k in hit else abs(v) <= 0.012, (k, v)
    assert G.plain_index(scores) == want


def test_decode_pairs_rows_and_columns_of_one_matrix_only():
    slots, rl, cl = 1024, 32, 32
    rows, cols = np.zeros(2 * cl * 1), np.zeros(2 * rl)
    rows[3], rows[cl + 5] = 2.0, 1.0   # row 3 of matrix 0, row 5 of matrix 1
    cols[7], cols[rl + 9] = 1.5, 2.0   # column 7 of matrix 0, column 9 of matrix 1
    assert G.decode(rows, cols, slots) == [3 * rl + 7, (cl + 5) * rl + 9]
    cols[8] = 0.999
    assert G.decode(rows, cols, slots) == [3 * rl + 7, (cl + 5) * rl + 9]


@pytest.mark.parametrize("count,rl", [(1, 32), (3, 512)])
def test_restatement_rows_and_columns_against_plain_model(small, count, rl):
    """uniform inputs in [-0.8, 0.8] on n_q - 3 limbs through the restatement, decrypted against the sums of x^5"""
    P, K, Or = small
    z = np.random.default_rng(count + rl).uniform(-0.8, 0.8, (count, P.slots))
    cts = G.fresh_scores(P, Or, z, 4)
    rows = G.oracle_rows(P, Or, cts, G.ALPHA_DEPTH, rl)
    cols = G.oracle_cols(P, Or, cts, G.ALPHA_DEPTH, rl)
    masks = sum(1 for what, _ in A.merge_schedule(P.slots, rl) if what == "mask")
    assert [c.nl for c in rows] == [P.nQ - 3 - G.ALPHA_DEPTH - 1 - masks] * (-(-(count * (P.slots // rl)) // P.slots))
    assert [c.nl for c in cols] == [P.nQ - 3 - G.ALPHA_DEPTH - 2] * (-(-(count * rl) // P.slots))
    got_r = np.concatenate([Or.decrypt(c) for c in rows])
    got_c = np.concatenate([Or.decrypt(c) for c in cols])
    err = max(np.abs(got_r - G.plain_rows(list(z), rl)).max(), np.abs(got_c - G.plain_cols(list(z), rl)).max())
    print("approach 2 restatement, rows / columns against the plain model: max error %.3e" % err)
    assert err < TOL


def test_restatement_index_scenario_against_plain_model(small):
    """n = 40, planted [23]: computeSimilarity (approach 1's restatement), the group test, the comparator and the receiver's decoding"""
    P, K, Or = small
    db, query, cos = cosines(40, [23], 3)
    dbcts = A.oracle_enroll(P, Or, db, 99)
    scores = A.oracle_compute_similarity(P, Or, Or.encrypt_query(query, 5, 1), dbcts)
    assert len(scores) == 1 and scores[0].nl == P.nQ - 3
    rows, cols = G.oracle_index_scenario(P, Or, scores)
    assert (len(rows), len(cols)) == (1, 1) and rows[0].nl == 1 and cols[0].nl == 2
    assert G.oracle_decrypt_index(P, Or, rows, cols) == G.plain_index(G.score_vectors(cos, P.slots)) == [23]
