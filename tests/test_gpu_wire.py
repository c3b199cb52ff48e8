"""Wire messages on the GPU (include/hydia.h, "wire messages"; run with -m gpu): k_wire_pack and k_wire_unpack_check bit for bit, the
range check, the header refusals against a context, seeded queries and keys as messages, the key-set file, and two contexts end to end
with nothing but bytes between them.  Every comparison is np.array_equal or bytes == against the numpy restatement tests/wire_ref.py
(over the oracle's / tests/seeded_ref.py's residues), never against the product's own output.
Ring: N = 2^11, 64-dim vectors (n_q 12, n_p 4, dnum 3) unless said."""
import os

import numpy as np
import pytest

import oracle_lib as O
import seeded_ref as SR
import wire_ref as WR

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2
SEED, A_SEED = 7, 1007


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module")
def torch():
    try:
        import torch
    except ImportError:
        return None
    return torch


def new_ctx(im, log_n=11, dim=64):
    return im.Context(im.default_params(log_n=log_n, vector_dim=dim), 0)


@pytest.fixture(scope="module")
def small(im, torch):
    """the oracle's parameters and key set under SEED, the restated seeded keys (computed once, never modified), the receiver's context R
    after keygen_seeded(SEED, A_SEED) — never re-keyed — and a second context S without any key for everything that only moves residues"""
    P = O.Params(log_n=11, depth=11, dim=64)
    K0, K = O.Keys(P, SEED), O.Keys(P, SEED)
    keys, pk = SR.install(K, P, SEED, A_SEED)
    R, S = new_ctx(im), new_ctx(im)
    R.keygen_seeded(SEED, A_SEED)
    mods = [int(q) for q in P.moduli]
    yield P, K0, keys, pk, R, S, mods
    R.close()
    S.close()
    P.close()


def raises(im, code, fn, *args, **kw):
    with pytest.raises(im.HydiaError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def probe(P, seed):
    return np.random.default_rng(seed).integers(-99, 100, size=P.dim).astype(np.float64)


def crafted(mods, count, n_polys, n_limbs, n, seed):
    """[count][poly][limb][N] canonical residues: random, with the first rows of every limb 0, 1, q - 1, (q - 1, 0, ..), (0, q - 1, ..)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, n_polys, n_limbs, n), dtype=np.uint64)
    for j in range(n_limbs):
        q = mods[j]
        out[:, :, j] = rng.integers(0, q, size=(count, n_polys, n), dtype=np.uint64)
        flat = out[:, :, j].reshape(count * n_polys, n)
        alt = np.zeros(n, dtype=np.uint64)
        alt[0::2] = q - 1
        for i, row in enumerate((np.full(n, q - 1, dtype=np.uint64), alt, np.uint64(q - 1) - alt, np.zeros(n, dtype=np.uint64), np.ones(n, dtype=np.uint64))):
            if i < len(flat):
                flat[(i + j) % len(flat)] = row
        out[:, :, j] = flat.reshape(count, n_polys, n)
    return out


# ------------------------------------------------------------------------------------------------ 1. pack and unpack, bit for bit
@pytest.mark.parametrize("count,n_polys,n_limbs", [(1, 2, 12), (3, 3, 12), (3, 2, 5), (1, 3, 1), (3, 2, 1)])
def test_pack_bit_for_bit(im, small, count, n_polys, n_limbs):
    P, K0, keys, pk, R, S, mods = small
    data = crafted(mods, count, n_polys, n_limbs, P.N, 100 * count + 10 * n_polys + n_limbs)
    scale = 2.0 ** 45 * (1 + n_limbs / 16)
    ct = S.import_ct(data, scale)
    want = WR.ct_message(data, mods, scale)
    assert S.wire_ct_bytes(count, n_polys, n_limbs) == len(want)
    got = ct.to_wire()
    assert got == want
    back = S.ct_from_wire(want)
    assert back.shape() == (count, n_polys, n_limbs, scale)
    assert np.array_equal(back.export(), data)
    info = im.wire_peek(got)
    assert (info["type"], info["count"], info["n_polys"], info["n_limbs"], info["scale"]) == (1, count, n_polys, n_limbs, scale)


def test_pack_a_limb_prefix_view(im, small):
    """a hydia_ct_limb_prefix view of 5 limbs over a 12-limb batch: the pack honours the limb stride"""
    P, K0, keys, pk, R, S, mods = small
    data = crafted(mods, 3, 2, 12, P.N, 77)
    big = S.import_ct(data, 2.0 ** 45)
    view = S.ct_limb_prefix(big, 5)
    assert view.to_wire() == WR.ct_message(data[:, :, :5], mods, 2.0 ** 45)
    assert big.to_wire() == WR.ct_message(data, mods, 2.0 ** 45)


def test_pack_on_widths_outside_the_default_chain(im):
    """a custom chain with 31-, 46-, 47-, 48-, 59- and 60-bit limbs (tests/test_gpu_edge_primes.py's constructor)"""
    from test_gpu_edge_primes import transform_chain
    moduli = transform_chain(11)
    widths = {int(q).bit_length() for q in moduli[:12]}
    assert {47, 48, 59} <= widths
    P = O.Params(log_n=11, depth=11, dim=64, moduli=moduli, n_p=4)
    cc = im.Context(im.default_params(log_n=11, vector_dim=64), 0, moduli=moduli, roots=P.roots, n_p=4)
    try:
        mods = [int(q) for q in moduli]
        data = crafted(mods, 2, 2, 12, P.N, 5)
        ct = cc.import_ct(data, 2.0 ** 45)
        want = WR.ct_message(data, mods, 2.0 ** 45)
        assert ct.to_wire() == want
        assert np.array_equal(cc.ct_from_wire(want).export(), data)
        # the range check follows the limb's own modulus
        bad = data.copy()
        bad[1, 1, 7, P.N - 1] = mods[7]
        raises(im, ERR_ARG, cc.ct_from_wire, WR.ct_message(bad, mods, 2.0 ** 45))
    finally:
        cc.close()
        P.close()


# ------------------------------------------------------------------------------------------------ 2. the range check
def test_range_check(im, small):
    P, K0, keys, pk, R, S, mods = small
    base = crafted(mods, 3, 2, 12, P.N, 9)
    S.ct_from_wire(WR.ct_message(base, mods, 2.0 ** 45))  # (the pool is warm: what a refusal leaves is compared with this state)
    live = S.memory_stats()[0]
    places = (((0, 0, 0, 0), mods[0]), ((2, 1, 11, P.N - 1), mods[11]))
    for at, q in places:
        w = q.bit_length()
        for value, ok in ((q, False), (q - 1, True), ((1 << w) - 1, False)):
            data = base.copy()
            data[at] = value
            msg = WR.ct_message(data, mods, 2.0 ** 45)
            if ok:
                got = S.ct_from_wire(msg)
                assert np.array_equal(got.export(), data)
                del got
            else:
                text = raises(im, ERR_ARG, S.ct_from_wire, msg)
                assert "modulus" in text
            assert S.memory_stats()[0] == live, (at, value)
    # a seeded query message is checked the same way, and makes no handle
    c0 = base[:, 0]
    c0[2, 11, P.N - 1] = mods[11]
    raises(im, ERR_ARG, S.ct_from_wire, WR.query_message(c0, mods, P.delta, O.seed_bytes(A_SEED).tobytes(), 1))
    assert S.memory_stats()[0] == live


# ------------------------------------------------------------------------------------------------ 3. header refusals with a context
def test_header_refusals_with_a_context(im, small):
    P, K0, keys, pk, R, S, mods = small
    data = crafted(mods, 1, 2, 12, P.N, 3)
    good = WR.ct_message(data, mods, 2.0 ** 45)
    body = good[WR.HEADER_BYTES:]
    other = list(mods)
    other[3] = mods[3] - 2  # the same width, another modulus
    ring10 = crafted(mods, 1, 2, 12, 1024, 4)
    key2 = np.zeros((2, 2, P.nT, P.N), dtype=np.uint64)  # two digits where the context has three
    bad = {
        "log_n": WR.ct_message(ring10, mods, 2.0 ** 45),
        "modulus": WR.header(1, 11, 1, 2, other[:12], scale=2.0 ** 45) + body,
        "n_limbs": WR.ct_message(crafted(mods, 1, 2, 13, P.N, 5), mods, 2.0 ** 45),
        "one byte short": good[:-1],
        "one byte over": good + b"\0",
    }
    for name, msg in bad.items():
        text = raises(im, ERR_ARG, S.ct_from_wire, msg)
        assert name.split()[0] in text or "len" in text, (name, text)
    text = raises(im, ERR_ARG, S.key_from_wire, WR.eval_key_message(key2, mods, 1))
    assert "dnum" in text and not S.has_eval_key(1)
    # keys go to key_from_wire and ciphertexts to ct_from_wire
    raises(im, ERR_ARG, S.key_from_wire, good)
    raises(im, ERR_ARG, S.ct_from_wire, WR.public_key_message(pk, mods))
    # and the context still works
    assert np.array_equal(S.ct_from_wire(good).export(), data)


# ------------------------------------------------------------------------------------------------ 4. seeded queries
def test_seeded_queries_as_messages(im, small, torch):
    P, K0, keys, pk, R, S, mods = small
    rec, snd = im.DiagonalReceiver(R, 1), im.DiagonalSender(S, 1)
    a_seed = O.seed_bytes(A_SEED).tobytes()
    rows = np.stack([probe(P, s) for s in (2, 3, 4)])
    want_c0, want_a = zip(*[SR.seeded_query(P, K0, rows[i], SEED, A_SEED, 5 + i) for i in range(3)])
    want = WR.query_message(np.stack(want_c0), mods, P.delta, a_seed, 5)
    got = rec.encryptQueriesWire(rows, seed=SEED, a_seed=A_SEED, nonce0=5)
    assert got == want
    assert R.wire_ct_bytes(3, 1, P.nQ, seeded=True) == len(want)
    info = im.wire_peek(got)
    assert (info["type"], info["count"], info["nonce0"], info["a_seed"], info["scale"]) == (2, 3, 5, a_seed, P.delta)
    one = rec.encryptQueryWire(rows[1], seed=SEED, a_seed=A_SEED, nonce=6)
    assert one == WR.query_message(np.stack(want_c0[1:2]), mods, P.delta, a_seed, 6)
    # the sender's handles: (c0, a) bit for bit, ordinary fresh ciphertexts
    handles = snd.queryFromWire(want)
    assert len(handles) == 3
    for i, h in enumerate(handles):
        assert h.shape() == (1, 2, P.nQ, P.delta)
        e = h.export()[0]
        assert np.array_equal(e[0], want_c0[i]) and np.array_equal(e[1], want_a[i]), i
    single = snd.queryFromWire(one)
    assert np.array_equal(single.export()[0, 0], want_c0[1])
    # refusals as hydia_encrypt_queries_seeded's: a_seed == seed, the nonce space, no secret key
    raises(im, ERR_ARG, rec.encryptQueriesWire, rows, seed=5, a_seed=5)
    raises(im, ERR_ARG, rec.encryptQueriesWire, rows, seed=SEED, a_seed=A_SEED, nonce0=(1 << 40) - 2)
    raises(im, ERR_STATE, im.DiagonalReceiver(S, 1).encryptQueryWire, rows[0], seed=SEED, a_seed=A_SEED)


def test_seeded_queries_from_device_rows(im, small, torch):
    """the _device twin from an f32 tensor on the context's GPU: the same bytes as the host entry on the widened rows"""
    if torch is None:
        pytest.skip("torch is not installed")
    P, K0, keys, pk, R, S, mods = small
    rec, a_seed = im.DiagonalReceiver(R, 1), O.seed_bytes(A_SEED).tobytes()
    rows32 = (np.stack([probe(P, s) for s in (2, 3, 4)]) / 7).astype(np.float32)
    t = torch.from_numpy(rows32).to("cuda:0")
    c0d = np.stack([SR.seeded_query(P, K0, rows32[i].astype(np.float64), SEED, A_SEED, 20 + i)[0] for i in range(3)])
    assert rec.encryptQueriesWire(t, seed=SEED, a_seed=A_SEED, nonce0=20) == WR.query_message(c0d, mods, P.delta, a_seed, 20)


# ------------------------------------------------------------------------------------------------ 5. keys
def test_keys_as_messages(im, small):
    P, K0, keys, pk, R, S, mods = small
    a_seed = O.seed_bytes(A_SEED).tobytes()
    ids = (0, 1, P.slots // 2)
    whole = {r: WR.eval_key_message(keys[r], mods, r) for r in ids}
    half = {r: WR.eval_key_message(keys[r], mods, r, a_seed) for r in ids}
    for r in ids:
        assert R.key_to_wire(r) == whole[r], r
        assert R.key_to_wire(r, seeded=True) == half[r], r
    pk_whole, pk_half = WR.public_key_message(pk, mods), WR.public_key_message(pk, mods, a_seed)
    assert R.key_to_wire(-1) == pk_whole and R.key_to_wire(-1, seeded=True) == pk_half
    assert (R.wire_eval_key_bytes(), R.wire_eval_key_bytes(True)) == (len(whole[1]), len(half[1]))
    assert (R.wire_public_key_bytes(), R.wire_public_key_bytes(True)) == (len(pk_whole), len(pk_half))
    for messages, pkm in ((whole, pk_whole), (half, pk_half)):
        cc = new_ctx(im)
        try:
            for r in ids:
                assert cc.key_from_wire(messages[r]) == r
                assert np.array_equal(cc.export_eval_key(r), keys[r]), r
            assert cc.key_from_wire(pkm) == -1
            assert np.array_equal(cc.export_public_key(), pk)
            # an installed key is whatever the message carried: not marked seeded here
            raises(im, ERR_STATE, cc.key_to_wire, 1, seeded=True)
            raises(im, ERR_STATE, cc.key_to_wire, -1, seeded=True)
            raises(im, ERR_STATE, cc.key_to_wire, 2)
            # one bad residue: refused, and the key installed before still exports unchanged
            bad = np.array(keys[1], dtype=np.uint64)
            bad[2, 0, P.nT - 1, P.N - 1] = mods[P.nT - 1]
            raises(im, ERR_ARG, cc.key_from_wire, WR.eval_key_message(bad, mods, 1))
            raises(im, ERR_ARG, cc.key_from_wire, WR.eval_key_message(bad, mods, 1, a_seed))
            assert np.array_equal(cc.export_eval_key(1), keys[1])
        finally:
            cc.close()
    # ... and keeps its seeded mark (on the receiver, whose keys are marked): refused, unchanged, still exported as a half
    bad = np.array(keys[1], dtype=np.uint64)
    bad[0, 0, 0, 0] = mods[0]
    raises(im, ERR_ARG, R.key_from_wire, WR.eval_key_message(bad, mods, 1))
    badpk = np.array(pk, dtype=np.uint64)
    badpk[0, 3, 5] = mods[3] + 1
    raises(im, ERR_ARG, R.key_from_wire, WR.public_key_message(badpk, mods))
    assert np.array_equal(R.export_eval_key(1), keys[1]) and np.array_equal(R.export_public_key(), pk)
    assert R.key_to_wire(1, seeded=True) == half[1] and R.key_to_wire(-1, seeded=True) == pk_half


# ------------------------------------------------------------------------------------------------ 6. the key-set file
def test_key_set_file(im, small, tmp_path):
    P, K0, keys, pk, R, S, mods = small
    a_seed = O.seed_bytes(A_SEED).tobytes()
    rots = [1, P.dim - 1, P.slots // 2]
    path = str(tmp_path / "keys.bin")
    im.DiagonalReceiver(R, 1).exportKeysWire(path, seeded=True, rotations=rots)
    messages = [WR.public_key_message(pk, mods, a_seed)] + [WR.eval_key_message(keys[r], mods, r, a_seed) for r in [0] + rots]
    data = open(path, "rb").read()
    assert len(data) == WR.FILE_HEADER_BYTES + sum(len(m) for m in messages)
    assert data == WR.file_header(5) + b"".join(messages)
    cc = new_ctx(im)
    try:
        im.DiagonalSender(cc, 1).importKeysWire(path)
        assert [r for r in range(P.slots) if cc.has_eval_key(r)] == [0] + rots
        for r in [0] + rots:
            assert np.array_equal(cc.export_eval_key(r), keys[r]), r
        assert np.array_equal(cc.export_public_key(), pk)
        # hydia_keys_save: every key the context holds, whole, in ascending id
        whole = str(tmp_path / "whole.bin")
        cc.keys_save(whole)
        assert open(whole, "rb").read() == WR.file_header(5) + WR.public_key_message(pk, mods) + b"".join(
            WR.eval_key_message(keys[r], mods, r) for r in [0] + rots)
        raises(im, ERR_STATE, cc.keys_save, str(tmp_path / "no.bin"), True)  # its keys are not marked seeded
    finally:
        cc.close()
    # a file cut in its last message: refused naming that message; the load is not transactional
    cut = str(tmp_path / "cut.bin")
    open(cut, "wb").write(data[:-100])
    cc = new_ctx(im)
    try:
        text = raises(im, ERR_ARG, cc.keys_load, cut)
        assert "message 4" in text and "truncated" in text
        assert cc.has_eval_key(P.dim - 1) and not cc.has_eval_key(P.slots // 2)
        open(cut, "wb").write(data + b"\0")
        assert "after the last message" in raises(im, ERR_ARG, cc.keys_load, cut)
        open(cut, "wb").write(b"HYDKEYS2" + data[8:])
        raises(im, ERR_ARG, cc.keys_load, cut)
    finally:
        cc.close()


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_end_to_end_nothing_but_bytes(im, small, tmp_path):
    """receiver R and a sender of its own: keys by file, one seeded query by message through indexScenario on a one-block database, the
    result back by message — bit for bit the result of the same query moved with expandQuery on the existing path"""
    P, K0, keys, pk, R, S, mods = small
    n, planted = 300, 123
    rng = np.random.default_rng(31)
    db = rng.integers(-99, 100, size=(n, P.dim)).astype(np.float64)
    db[planted] = rng.integers(1, 4, size=P.dim)
    query = np.ones(P.dim)
    receiver = im.DiagonalReceiver(R, n)
    path = str(tmp_path / "keys.bin")
    receiver.exportKeysWire(path)  # the whole seeded set
    assert os.path.getsize(path) == WR.FILE_HEADER_BYTES + R.wire_public_key_bytes(True) + (1 + len(O.default_rotations(P))) * R.wire_eval_key_bytes(True)
    T = new_ctx(im)
    try:
        sender = im.DiagonalSender(T, n)
        sender.importKeysWire(path)
        raises(im, ERR_STATE, T.export_secret_key)
        im.DiagonalEnroller(T, n).serializeDB(db.copy(), seed=41)
        message = receiver.encryptQueryWire(query, seed=SEED, a_seed=A_SEED, nonce=1)
        q = sender.queryFromWire(message)
        result = sender.indexScenario(q)
        shipped = sender.resultToWire(result)
        assert shipped == WR.ct_message(result.export(), mods, result.shape()[3])
        back = receiver.resultFromWire(shipped)
        # the existing path: the same query as a SeededQuery record, expanded
        q2 = sender.expandQuery(receiver.encryptQuerySeeded(query, seed=SEED, a_seed=A_SEED, nonce=1))
        want = sender.indexScenario(q2).export()
        assert np.array_equal(q.export(), q2.export())
        assert np.array_equal(result.export(), want) and np.array_equal(back.export(), want)
        assert back.shape() == result.shape()
        assert receiver.decryptIndex(back) == [planted]
    finally:
        T.close()


def test_kernels_are_timed_and_in_the_ledger(im, small):
    P, K0, keys, pk, R, S, mods = small
    data = crafted(mods, 2, 2, 12, P.N, 8)
    im.byte_ledger(1)
    S.kernel_time_reset()
    try:
        ct = S.import_ct(data, 2.0 ** 45)
        msg = ct.to_wire()
        S.ct_from_wire(msg)
        ledger = im.byte_ledger(0)
    finally:
        im.byte_ledger(0)
    packed, raw = len(msg) - WR.HEADER_BYTES, data.nbytes
    assert ledger["k_wire_pack"] == (1, float(packed + raw)) and ledger["k_wire_unpack_check"] == (1, float(packed + raw))
    assert S.kernel_time("k_wire_pack")[1] == 1 and S.kernel_time("k_wire_unpack_check")[1] == 1
