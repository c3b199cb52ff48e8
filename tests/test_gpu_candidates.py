"""Candidate lists and matches on the GPU (run with -m gpu): the selection stage behind the decoder
(image_matching_amd/csrc/select_kernels.hip) through hydia_slots_select_device / hydia_slots_topk_device on crafted arrays, and through
the decrypt entries, the Python roles and the wire.  The model is tests/candidates_ref.py (pinned by tests/test_candidates_cpu.py, which
also shows for each wrong form of a kernel a crafted input here that it changes).  Every comparison is bit for bit: indices equal, values
viewed as uint64.

Device arrays.  The count / scatter kernels own tiles of TILE = 1024 elements (4 rounds of 256 lanes); the scan kernel takes 1024 tile
counts per trip of its loop, so one trip covers 2^20 elements and BIG = 2^20 + 1025 (1026 tiles) is the size that needs a second trip.
  sizes      1, 63, 64, 65, 1023, 1024, 1025, BIG
  contents   candidates_ref.contents: normal random, all equal, a +-0.0 mix, +-inf and NaN sprinkled in, four distinct values (heavy
             ties), negatives only, subnormals, bit patterns that differ only in the lowest byte and only in the highest
  select     thresholds: a value that is present and nextafter above it; capacities 0 with null outputs, below / equal to / above the count
  top-k      k = 1, 2, the top tie group's size - 1 / that size / + 1 (case "head"), n - 1, n, n + 5 (case "tail")
Decrypt entries at N = 2^10 (512 slots; such a context serves exactly the receiver's side) and 2^11: random and crafted ciphertexts,
n_vectors, batches of results, refusals; end to end at 2^11 with planted matches; scoresToWire / resultFromWire.
Measured on one MI355X: the 228 cases take 7.0 s together; the slowest call is a BIG top-k "tail" case at 0.36 s (k = n: a million
survivors sorted on the host), the slowest step of all the first context's set-up at 1.8 s."""
import ctypes as C

import numpy as np
import pytest

import candidates_ref as CR
import client_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 20261021
BIG = CR.ONE_TRIP + CR.TILE + 1
SIZES = [1, 63, 64, 65, CR.TILE - 1, CR.TILE, CR.TILE + 1, BIG]
NAMES = ["normal", "equal", "zeros", "specials", "four", "negatives", "subnormals", "low_byte", "high_byte"]
ERR_ARG = -1


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module")
def torch():
    """(every context fixture below asks for this one first: torch is imported before the library opens the GPU, as in
    tests/test_gpu_device_rows.py — imported after it, torch finds no device in this process)"""
    import torch
    return torch


@pytest.fixture(scope="module", params=[10, 11])
def recv(torch, im, request):
    """a receiver-side context (no rotation keys) on the default chain of that ring, dimension 64"""
    cc = im.Context(im.default_params(log_n=request.param, vector_dim=64), 0)
    cc.keygen_rotations([], SEED)
    yield cc
    cc.close()


@pytest.fixture(scope="module")
def cc11(torch, im):
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    cc.keygen_rotations([], SEED)
    yield cc
    cc.close()


# ---- device arrays: one input, its device copy and the model's full order per (size, content), computed once and left unchanged
_CONTENTS, _CASES = {}, {}


def case(torch, n, name):
    if n not in _CONTENTS:
        _CONTENTS[n] = CR.contents(n, np.random.default_rng([SEED, n]))
    if (n, name) not in _CASES:
        v = _CONTENTS[n][name]
        v.setflags(write=False)
        order = CR.topk(v, n)[0]
        order.setflags(write=False)
        _CASES[(n, name)] = (v, torch.from_numpy(v.copy()).cuda(), order)
    return _CASES[(n, name)]


def same(got_idx, got_val, want_idx, v, what):
    assert np.array_equal(got_idx, want_idx), (what, got_idx[:8], want_idx[:8])
    assert np.array_equal(CR.bits(got_val), CR.bits(v[want_idx])), what


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", SIZES)
def test_select_on_crafted_arrays(cc11, torch, n, name):
    v, d, _ = case(torch, n, name)
    numbers = np.flatnonzero(~np.isnan(v))
    present = v[numbers[numbers.size // 2]] if numbers.size else 0.0
    for t in (present, np.nextafter(present, np.inf)):
        want, _, count = CR.select(v, t)
        assert numbers.size == 0 or t != present or count >= 1  # a value that is present is included
        idx, val, total = cc11.slots_select(d, t, cap=0)  # null outputs: count only
        assert total == count and idx.size == 0 and val.size == 0, (t, total, count)
        for cap in sorted({c for c in (count // 2, count - 1, count, count + 3, None) if c is None or c >= 1}, key=lambda c: (c is None, c)):
            idx, val, total = cc11.slots_select(d, t, cap=cap)
            assert total == count, (t, cap, total, count)
            same(idx, val, want[:cap], v, ("select", t, cap))


@pytest.mark.parametrize("part", ["head", "tail"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", SIZES)
def test_topk_on_crafted_arrays(cc11, torch, n, name, part):
    v, d, order = case(torch, n, name)
    g = CR.top_group(v)
    ks = {1, 2, g - 1, g, g + 1} if part == "head" else {n - 1, n, n + 5}
    for k in sorted(k for k in ks if k >= 1):
        idx, val = cc11.slots_topk(d, k)
        assert idx.size == min(k, n)
        same(idx, val, order[:k], v, ("topk", k))


def test_same_input_same_output(cc11, torch):
    v, d, order = case(torch, BIG, "four")
    runs = [cc11.slots_topk(d, 1000) for _ in range(3)]
    for idx, val in runs:
        same(idx, val, order[:1000], v, "repeat")


def test_device_array_refusals(cc11, torch, im):
    """k = 0, n = 0, a host pointer and a tensor on the CPU answer HYDIA_ERR_ARG and leave the outputs untouched"""
    L = cc11.L
    v, d, _ = case(torch, 65, "normal")
    sentinel = np.uint64(0xDEADBEEF)
    idx, val, n = np.full(8, sentinel, dtype=np.uint64), np.full(8, 7.5), C.c_size_t(99)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dev = C.c_void_p(d.data_ptr())
    host = np.ascontiguousarray(v)
    calls = [lambda: L.hydia_slots_topk_device(cc11.h, dev, 65, 0, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_slots_topk_device(cc11.h, dev, 0, 3, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_slots_topk_device(cc11.h, dev, 1 << 31, 3, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_slots_topk_device(cc11.h, dev, 65, 3, p(idx), p(val), None),
             lambda: L.hydia_slots_topk_device(cc11.h, p(host), 65, 3, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_slots_select_device(cc11.h, p(host), 65, 0.0, p(idx), p(val), 8, C.byref(n)),
             lambda: L.hydia_slots_select_device(cc11.h, dev, 0, 0.0, p(idx), p(val), 8, C.byref(n)),
             lambda: L.hydia_slots_select_device(cc11.h, dev, 65, 0.0, p(idx), p(val), 8, None),
             lambda: L.hydia_decrypt_device(cc11.h, cc11.encrypt(np.zeros(cc11.slots), seed=1).h, p(np.zeros(cc11.slots)))]
    for i, call in enumerate(calls):
        assert call() == ERR_ARG, i
        assert (idx == sentinel).all() and (val == 7.5).all() and n.value == 99, i
    with pytest.raises(im.HydiaError) as e:
        cc11.slots_topk(torch.from_numpy(host.copy()), 3)
    assert e.value.code == ERR_ARG
    with pytest.raises(im.HydiaError) as e:
        cc11.slots_select(torch.from_numpy(host.copy()), 0.0)
    assert e.value.code == ERR_ARG
    # the context still works
    assert cc11.slots_topk(d, 1)[0].tolist() == [int(np.argmax(v))]


# ---- decrypt entries
def test_random_ciphertexts(recv, im):
    cc, S = recv, recv.slots
    rng = np.random.default_rng([SEED, S])
    ct = cc.encrypt(rng.uniform(-1.5, 1.5, (3, S)), seed=11, nonce0=3)
    truth = cc.decrypt(ct).reshape(-1)
    dev = cc.decrypt_device(ct)
    assert tuple(dev.shape) == (3, S) and np.array_equal(CR.bits(dev.cpu().numpy().reshape(-1)), CR.bits(truth))
    r = im.DiagonalReceiver(cc, 3 * S)
    for nv in (None, 1, S, S + 1, 3 * S - 7):
        part = truth[:nv]
        for t in (part[part.size // 2], np.nextafter(part[part.size // 2], np.inf), 1.0):
            want, _, count = CR.select(part, t)
            idx, val, total = r.decryptMatches(ct, t, nv)
            assert total == count
            same(idx, val, want, part, ("matches", nv, t))
            idx, val, total = r.decryptMatches(ct, t, nv, cap=2)
            assert total == count
            same(idx, val, want[:2], part, ("matches cap 2", nv, t))
        order = CR.topk(part, part.size)[0]
        for k in (1, 5, part.size, part.size + 5):
            idx, val = r.decryptTopK(ct, k, nv)
            same(idx, val, order[:k], part, ("topk", nv, k))
    hits = np.flatnonzero(truth >= 1.0)
    assert hits.size > 20 and r.decryptIndex(ct) == hits.tolist()
    cap, sentinel = 10, np.uint64(0xDEADBEEF)
    out, n = np.full(3 * S, sentinel, dtype=np.uint64), C.c_size_t()
    assert cc.L.hydia_decrypt_index(cc.h, ct.h, out.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == hits.size and np.array_equal(out[:cap], hits[:cap].astype(np.uint64)) and (out[cap:] == sentinel).all()
    assert cc.L.hydia_decrypt_index(cc.h, ct.h, None, 0, C.byref(n)) == 0 and n.value == hits.size


def test_crafted_ciphertexts(recv, im):
    """(NTT(t), 0) with a constant t decrypts to the same exact double in every slot of that ciphertext"""
    cc, S = recv, recv.slots
    d = int(cc.delta)
    r = im.DiagonalReceiver(cc, 3 * S)
    make = lambda vals: cc.import_ct(R.single_batch(vals, cc.moduli, 2, cc.N), cc.delta)
    a, b = 3 * d // 4, d // 4
    aba = make([a, b, a])
    assert np.array_equal(CR.bits(cc.decrypt(aba)), CR.bits(np.repeat([0.75, 0.25, 0.75], S).reshape(3, S)))
    walk = list(range(S)) + list(range(2 * S, 3 * S)) + list(range(S, 2 * S))
    for k in (1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S):
        idx, val = r.decryptTopK(aba, k)
        assert idx.tolist() == walk[:k], k
        assert np.array_equal(CR.bits(val), CR.bits([0.75] * min(k, 2 * S) + [0.25] * max(0, k - 2 * S)))
    # exactly 1.0 is included, the double below it (at scale 2^90: 2^90 - 2^37) is not
    scale = cc.delta * cc.delta
    mixed = cc.import_ct(R.single_batch([(1 << 90) - (1 << 37), 1 << 90, (1 << 90) - (1 << 37)], cc.moduli, 2, cc.N), scale)
    truth = cc.decrypt(mixed)
    assert np.array_equal(CR.bits(truth), CR.bits(np.repeat([np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 0.0)], S).reshape(3, S)))
    idx, val, total = r.decryptMatches(mixed, 1.0)
    assert total == S and idx.tolist() == list(range(S, 2 * S)) and np.array_equal(CR.bits(val), CR.bits(np.ones(S)))
    assert r.decryptMatches(mixed, np.nextafter(1.0, 0.0))[2] == 3 * S
    assert r.decryptIndex(mixed) == list(range(S, 2 * S))
    assert r.decryptMembership(mixed) is False and r.decryptMembership(make([d, 0])) is True


def test_batches_of_results(recv, im):
    cc, S = recv, recv.slots
    rng = np.random.default_rng([SEED, S, 2])
    results = [cc.encrypt(rng.uniform(-1.5, 1.5, (x, S)), seed=12, nonce0=10 * x) for x in (1, 3, 2)]
    r = im.DiagonalReceiver(cc, 3 * S)
    for nv in (None, S - 3):
        for k in (1, 7, S + 9):
            rows = r.decryptTopKMulti(results, k, nv)
            assert len(rows) == 3
            for ct, (idx, val) in zip(results, rows):
                one = r.decryptTopK(ct, k, nv)
                assert idx.size == min(k, nv or len(ct) * S)
                assert np.array_equal(idx, one[0]) and np.array_equal(CR.bits(val), CR.bits(one[1])), (nv, k)
        for cap in (None, 4):
            rows = r.decryptMatchesMulti(results, 1.0, nv, cap)
            totals = []
            for ct, (idx, val, total) in zip(results, rows):
                one = r.decryptMatches(ct, 1.0, nv, cap)
                truth = cc.decrypt(ct).reshape(-1)[:nv]
                assert total == one[2] == int((truth >= 1.0).sum())
                assert np.array_equal(idx, one[0]) and np.array_equal(CR.bits(val), CR.bits(one[1])), (nv, cap)
                totals.append(total)
            assert nv is not None or len(set(totals)) == 3  # the counts are per result


def test_decrypt_refusals(recv, im):
    cc, S = recv, recv.slots
    ct = cc.encrypt(np.linspace(-1, 1, 2 * S).reshape(2, S), seed=13)
    sentinel = np.uint64(0xDEADBEEF)
    idx, val, n = np.full(8, sentinel, dtype=np.uint64), np.full(8, 7.5), C.c_size_t(99)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    hs = (C.c_void_p * 1)(ct.h)
    L = cc.L
    calls = [lambda: L.hydia_decrypt_topk(cc.h, ct.h, 0, 0, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_decrypt_topk(cc.h, ct.h, 2 * S + 1, 3, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_decrypt_topk(cc.h, ct.h, 0, 3, p(idx), p(val), None),
             lambda: L.hydia_decrypt_matches(cc.h, ct.h, 2 * S + 1, 0.0, p(idx), p(val), 8, C.byref(n)),
             lambda: L.hydia_decrypt_matches(cc.h, ct.h, 0, 0.0, p(idx), p(val), 8, None),
             lambda: L.hydia_decrypt_topk_multi(cc.h, hs, 1, 2 * S + 1, 3, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_decrypt_topk_multi(cc.h, hs, 1, 0, 0, p(idx), p(val), C.byref(n)),
             lambda: L.hydia_decrypt_matches_multi(cc.h, hs, 1, 2 * S + 1, 0.0, p(idx), p(val), 8, C.byref(n))]
    for i, call in enumerate(calls):
        assert call() == ERR_ARG, i
        assert (idx == sentinel).all() and (val == 7.5).all() and n.value == 99, i
    r = im.DiagonalReceiver(cc, 2 * S)
    for bad in (lambda: r.decryptTopK(ct, 0), lambda: r.decryptTopK(ct, 3, 2 * S + 1), lambda: r.decryptMatches(ct, 0.0, 2 * S + 1)):
        with pytest.raises(im.HydiaError) as e:
            bad()
        assert e.value.code == ERR_ARG
    assert r.decryptTopK(ct, 1)[0].tolist() == [2 * S - 1]


# ---- end to end at 2^11: dimension 64, 2500 vectors (three blocks), two planted matches
N_VEC, DIM, PLANTED = 2500, 64, (777, 2311)


def planted_database():
    """rows whose cosine with the query is >= 0.9 (the two planted rows) or outside (0.30, 0.60): a random row inside a margin around
    that band has its component along the query removed"""
    rng = np.random.default_rng([SEED, 5])
    q = rng.standard_normal(DIM)
    u = q / np.linalg.norm(q)
    db = rng.standard_normal((N_VEC, DIM))
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ u
    mid = (cos > 0.25) & (cos < 0.65)
    db[mid] -= np.outer(db[mid] @ u, u)
    for i in PLANTED:
        db[i] = q + 0.2 * rng.standard_normal(DIM)
    return q, db


@pytest.fixture(scope="module")
def served(torch, im):
    q, db = planted_database()
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (q / np.linalg.norm(q))
    assert not ((cos > 0.30) & (cos < 0.60)).any() and (cos[list(PLANTED)] >= 0.9).all() and (cos >= 0.9).sum() == 2
    cc = im.Context(im.default_params(log_n=11, vector_dim=DIM), 0)
    cc.keygen(SEED)
    im.DiagonalEnroller(cc, N_VEC).serializeDB(db.copy(), seed=99)
    receiver, sender = im.DiagonalReceiver(cc, N_VEC), im.DiagonalSender(cc, N_VEC)
    qc = receiver.encryptQuery(q, seed=5, nonce=1)
    scores = sender.computeSimilarity(qc)
    yield cc, receiver, sender, qc, scores, cos
    cc.close()


def test_end_to_end_candidate_list(served):
    cc, receiver, sender, qc, scores, cos = served
    assert len(scores) == 3
    truth = cc.decrypt(scores).reshape(-1)[:N_VEC]
    assert np.abs(truth - cos).max() < 1e-4
    idx, val = receiver.decryptTopK(scores, 5, N_VEC)
    same(idx, val, CR.topk(truth, 5)[0], truth, "end to end")
    assert sorted(idx[:2].tolist()) == sorted(PLANTED)
    hits, _, total = receiver.decryptMatches(scores, 0.44, N_VEC)
    assert total == 2 and sorted(hits.tolist()) == sorted(receiver.decryptIndex(sender.indexScenario(qc))) == sorted(PLANTED)


def test_scores_over_the_wire(served, im):
    cc, receiver, sender, qc, scores, cos = served
    X, _, nl, scale = scores.shape()
    assert nl == 11
    truth = cc.decrypt(scores)
    width = [int(m).bit_length() for m in cc.moduli]
    two, one = sender.scoresToWire(scores), sender.scoresToWire(scores, limbs=1)
    for message, limbs in ((two, 2), (one, 1)):
        assert len(message) == 360 + X * 2 * sum(cc.N * w // 8 for w in width[:limbs])  # wire_format.h: header + [count][poly][limb] rows
    assert len(two) == cc.wire_ct_bytes(X, 2, 2) and len(one) == cc.wire_ct_bytes(X, 2, 1)
    got2 = receiver.resultFromWire(two)
    assert got2.shape() == (X, 2, 2, scale)
    assert np.array_equal(CR.bits(cc.decrypt(got2)), CR.bits(truth))
    idx, val = receiver.decryptTopK(got2, 5, N_VEC)
    want = receiver.decryptTopK(scores, 5, N_VEC)
    assert np.array_equal(idx, want[0]) and np.array_equal(CR.bits(val), CR.bits(want[1]))
    # one limb: the oracle's transforms and decode of t = c0 + c1 s on q_0 alone
    P = O.Params(log_n=11, depth=11, dim=DIM)
    assert np.array_equal(P.moduli, cc.moduli)
    q0 = int(cc.moduli[0])
    s = cc.export_secret_key()[0].astype(object)
    data = scores.export()
    want1 = np.stack([P.decode(P.ntt_inv(((data[x, 0, 0].astype(object) + data[x, 1, 0].astype(object) * s) % q0).astype(np.uint64), 0)[None], scale)
                      for x in range(X)])
    got1 = receiver.resultFromWire(one)
    assert got1.shape() == (X, 2, 1, scale)
    assert np.array_equal(CR.bits(cc.decrypt(got1)), CR.bits(want1))
    assert np.abs(cc.decrypt(got1).reshape(-1)[:N_VEC] - cos).max() < 1e-4
    with pytest.raises(im.HydiaError):
        sender.scoresToWire(scores, limbs=3)
    P.close()
