"""Templates already in device memory (hydia_dev_rows; run with -m gpu): the widening / normalising kernel through
hydia_rows_widen_device, enrolment, in-place updates and queries from f64 / f32 / f16 / bf16 tensors, the ordering against the
producer stream and the refused calls.  Every comparison is bit for bit: the kernel against numpy's widening and the oracle's
hyo_normalize (tests/device_rows_ref.py), everything behind it against the HOST entry point on a twin context (same key seed) that is
handed the rows widened on the host.  Ring: N = 2^11 (1024 slots), 64-dim vectors; contexts at dim 8 and 512 for the kernel alone."""
import ctypes as C
import functools

import numpy as np
import pytest

from device_rows_ref import BF16_NANS, F16_NANS, edge_bits, hyo_normalize_rows, same_bits, same_bits_nan_as_nan, widen_bits

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2
DTYPES = ["f64", "f32", "f16", "bf16"]
CODE = {"f64": 0, "f32": 1, "f16": 2, "bf16": 3}
KEY_SEED, DIM, SLOTS = 7, 64, 1024


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_CTX = {}


def ctx(im, dim=DIM, twin=0, keys=True):
    """contexts shared by the module: (dim, twin) -> Context; the two twins at one dim hold the same keys"""
    key = (dim, twin)
    if key not in _CTX:
        cc = im.Context(im.default_params(log_n=11, vector_dim=dim), 0)
        if keys:
            cc.keygen(KEY_SEED)
        _CTX[key] = cc
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for cc in _CTX.values():
        cc.close()
    _CTX.clear()


# ---- rows as bit patterns (numpy) and as tensors
def to_bits(values, dtype):
    """float64 values -> bit patterns of `dtype` (bf16: the upper half of the float32 pattern — any pattern is a legitimate input)"""
    v = np.asarray(values, dtype=np.float64)
    if dtype == "f64":
        return v.view(np.uint64).copy()
    if dtype == "f32":
        return v.astype(np.float32).view(np.uint32).copy()
    if dtype == "f16":
        return v.astype(np.float16).view(np.uint16).copy()
    return (v.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def tensor(torch, bits, dtype):
    """a contiguous tensor [n][dim] of `dtype` on the GPU holding exactly these bit patterns"""
    signed = {"f64": np.int64, "f32": np.int32, "f16": np.int16, "bf16": np.int16}[dtype]
    tt = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    return torch.from_numpy(np.ascontiguousarray(bits).view(signed).copy()).cuda().view(tt)


def raw(torch, t):
    """the tensor's bits on the host"""
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().copy()


LAYOUTS = ["dense", "stride+8", "offset1"]


def laid_out(torch, t, layout):
    """the same rows as a slice of a wider tensor: (the slice, the wider tensor).  stride+8: row_stride = dim + 8; offset1: the slice
    t[:, 1:1+dim] of that, so the base pointer is aligned to one element only"""
    if layout == "dense":
        return t, t
    n, dim = t.shape
    wide = torch.full((n, dim + 8), 3.0, dtype=t.dtype, device=t.device)
    a = 0 if layout == "stride+8" else 1
    wide[:, a:a + dim] = t
    return wide[:, a:a + dim], wide


@functools.lru_cache(maxsize=None)
def random_rows(dtype, dim, n=1027):
    """(bit patterns [n][dim], the rows widened on the host, their normalisation by the oracle): computed once, never modified"""
    rng = np.random.default_rng(1000 + dim + CODE[dtype])
    v = rng.standard_normal((n, dim)) * rng.choice([1e-3, 1.0, 40.0], size=(n, 1))
    bits = to_bits(v, dtype)
    D = widen_bits(bits, dtype)
    want = hyo_normalize_rows(D)
    for a in (bits, D, want):
        a.setflags(write=False)
    return bits, D, want


# ------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("dtype,nans", [("f16", F16_NANS), ("bf16", BF16_NANS)])
def test_every_half_precision_pattern_is_widened_exactly(im, torch, dtype, nans):
    cc = ctx(im)
    bits = np.arange(65536, dtype=np.uint16).reshape(1024, 64)
    t = tensor(torch, bits, dtype)
    got = cc.rows_widen_device(t, normalise=False).cpu().numpy()
    assert same_bits_nan_as_nan(got, widen_bits(bits, dtype), nans)
    assert np.array_equal(raw(torch, t), bits.view(np.int16))


@pytest.mark.parametrize("dim", [8, 64, 512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_widened_and_normalised_bit_for_bit(im, torch, dtype, dim):
    """n = 1, 63, 64, 65 (around the 64-row tile) and 1027 (many tiles, a ragged last one), in the three layouts"""
    cc = ctx(im, dim, keys=False)
    bits, D, want = random_rows(dtype, dim)
    for n in (1, 63, 64, 65, 1027):
        for layout in LAYOUTS:
            t, wide = laid_out(torch, tensor(torch, bits[:n], dtype), layout)
            before = raw(torch, wide)
            assert same_bits(cc.rows_widen_device(t, normalise=False).cpu().numpy(), D[:n]), (n, layout)
            assert same_bits(cc.rows_widen_device(t, normalise=True).cpu().numpy(), want[:n]), (n, layout)
            assert np.array_equal(raw(torch, wide), before), (n, layout)  # the source is never written


@pytest.mark.parametrize("dim", [8, 64, 512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_rows(im, torch, dtype, dim):
    """zero row, one non-zero element, subnormals, f16 maxima, an overflowing squared sum (f64), a negative zero"""
    cc = ctx(im, dim, keys=False)
    bits = edge_bits(dim, dtype)
    D = widen_bits(bits, dtype)
    for layout in ("dense", "offset1"):
        t, wide = laid_out(torch, tensor(torch, bits, dtype), layout)
        before = raw(torch, wide)
        assert same_bits(cc.rows_widen_device(t, normalise=False).cpu().numpy(), D), layout
        got = cc.rows_widen_device(t, normalise=True).cpu().numpy()
        assert same_bits(got, hyo_normalize_rows(D)), layout
        assert same_bits(got[0], D[0]) and not np.isnan(got).any()  # the zero row passes through
        assert np.array_equal(raw(torch, wide), before)


# ------------------------------------------------------------------ 2. enrolment
def gallery_rows(dtype, n):
    bits, D, _ = random_rows(dtype, DIM, 1027)
    return bits[:n], D[:n].copy()


def all_cts(cc):
    return [cc.db_export_ct(t) for t in range(cc.db_stats()[1])]


def all_pts(cc):
    return [cc.plain_db_export_pt(t) for t in range(cc.db_stats()[1])]


def same_lists(a, b):
    return len(a) == len(b) and len(a) > 0 and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("matvec", ["hoisted", "bsgs"])
@pytest.mark.parametrize("n", [1, 1024, 1027])
@pytest.mark.parametrize("dtype", DTYPES)
def test_enrolment_equals_the_host_enrolment(im, torch, dtype, n, matvec):
    dev, host = ctx(im, DIM, 0), ctx(im, DIM, 1)
    bits, D = gallery_rows(dtype, n)
    t = tensor(torch, bits, dtype)
    for cc in (dev, host):
        cc.set_matvec(matvec)
    try:
        im.DiagonalEnroller(dev, n).serializeDB(t, seed=3)
        im.DiagonalEnroller(host, n).serializeDB(D.copy(), seed=3)  # (a copy: the host entry point normalises in place)
        assert dev.db_kind() == host.db_kind() == (5 if matvec == "hoisted" else 6) and dev.db_babies() == host.db_babies()
        assert dev.db_stats() == host.db_stats() and dev.db_stats()[:2] == (n, DIM * ((n + SLOTS - 1) // SLOTS))
        assert same_lists(all_cts(dev), all_cts(host))
        im.PlainEnroller(dev, n).serializeDB(t)
        im.PlainEnroller(host, n).serializeDB(D.copy())
        assert dev.db_kind() == host.db_kind() == (7 if matvec == "hoisted" else 8) and dev.db_stats() == host.db_stats()
        assert same_lists(all_pts(dev), all_pts(host))
    finally:
        for cc in (dev, host):
            cc.set_matvec("auto")
    assert np.array_equal(raw(torch, t), bits.view(raw(torch, t).dtype))


# ------------------------------------------------------------------ 3. updates
@pytest.mark.parametrize("plain", [False, True], ids=["ciphertexts", "plain-gallery"])
@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_updates_equal_the_host_updates(im, torch, dtype, plain):
    """an append across a block edge (1020 + 7 rows, given with row_stride = dim + 8), a replace with normalise = 0 (new - old) and
    a remove by the negated rows; after each, every ciphertext / plaintext equals the host call's on the twin context"""
    dev, host = ctx(im, DIM, 0), ctx(im, DIM, 1)
    n0 = 1020
    bits, D = gallery_rows(dtype, 1027)
    export = all_pts if plain else all_cts
    if plain:
        enr_d, enr_h = im.PlainEnroller(dev, n0), im.PlainEnroller(host, n0)
        enr_d.serializeDB(tensor(torch, bits[:n0], dtype))
        enr_h.serializeDB(D[:n0].copy())
        kw = lambda s: {}  # noqa: E731
    else:
        enr_d, enr_h = im.DiagonalEnroller(dev, n0), im.DiagonalEnroller(host, n0)
        enr_d.serializeDB(tensor(torch, bits[:n0], dtype), seed=11)
        enr_h.serializeDB(D[:n0].copy(), seed=11)
        kw = lambda s: {"seed": s}  # noqa: E731
    # append across the block edge
    t, _ = laid_out(torch, tensor(torch, bits[n0:n0 + 7], dtype), "stride+8")
    enr_d.appendDB(t, **kw(12))
    enr_h.appendDB(D[n0:n0 + 7].copy(), **kw(12))
    assert enr_d.numVectors == enr_h.numVectors == n0 + 7 and dev.db_stats() == host.db_stats() and dev.db_stats()[1] == 2 * DIM
    assert same_lists(export(dev), export(host))
    # replace rows 500 .. 502: new - old of values that exist in the type, as given
    rng = np.random.default_rng(8)
    delta_bits = to_bits(rng.standard_normal((3, DIM)) * 0.1, dtype)
    enr_d.updateRows(500, tensor(torch, delta_bits, dtype), False, **kw(13))
    enr_h.updateRows(500, widen_bits(delta_bits, dtype), False, **kw(13))
    assert same_lists(export(dev), export(host))
    # remove rows 1022 .. 1026 (across the edge again): the negated rows, normalised
    neg_bits = to_bits(-D[1022:1027], dtype)
    enr_d.updateRows(1022, tensor(torch, neg_bits, dtype), True, **kw(14))
    enr_h.updateRows(1022, widen_bits(neg_bits, dtype), True, **kw(14))
    assert dev.db_stats() == host.db_stats()
    assert same_lists(export(dev), export(host))


# ------------------------------------------------------------------ 4. queries
@pytest.mark.parametrize("dtype", DTYPES)
def test_queries_equal_the_single_host_queries(im, torch, dtype):
    cc = ctx(im)
    bits, D, _ = random_rows(dtype, DIM)
    receiver, sender = im.DiagonalReceiver(cc, 100), im.DiagonalSender(cc, 100)
    singles_ct = [np.asarray(receiver.encryptQuery(D[i].copy(), seed=21, nonce=40 + i).export()) for i in range(9)]
    singles_pt = [np.asarray(sender.encodeQuery(D[i].copy()).export()) for i in range(9)]
    for k in (1, 3, 9):
        t, _ = laid_out(torch, tensor(torch, bits[:k], dtype), "offset1")
        cts = receiver.encryptQueries(t, seed=21, nonce0=40)
        pts = sender.encodeQueries(t)
        assert len(cts) == len(pts) == k
        for i in range(k):
            assert np.array_equal(np.asarray(cts[i].export()), singles_ct[i]), (k, i)
            assert np.array_equal(np.asarray(pts[i].export()), singles_pt[i]), (k, i)
    # a 1-D tensor is one probe
    one = tensor(torch, bits[:1], dtype)[0]
    assert np.array_equal(np.asarray(receiver.encryptQuery(one, seed=21, nonce=40).export()), singles_ct[0])
    assert np.array_equal(np.asarray(sender.encodeQuery(one).export()), singles_pt[0])


def test_the_nonce_limit_applies_to_the_whole_batch(im, torch):
    cc = ctx(im)
    bits, D, _ = random_rows("f32", DIM)
    receiver = im.DiagonalReceiver(cc, 100)
    t = tensor(torch, bits[:3], "f32")
    with pytest.raises(im.HydiaError) as e:
        receiver.encryptQueries(t, seed=1, nonce0=2 ** 40 - 2)  # the third probe would take nonce 2^40
    assert e.value.code == ERR_ARG and "2^40" in str(e.value)
    got = receiver.encryptQueries(t, seed=1, nonce0=2 ** 40 - 3)  # the last three nonces
    want = receiver.encryptQuery(D[2].copy(), seed=1, nonce=2 ** 40 - 1)
    assert np.array_equal(np.asarray(got[2].export()), np.asarray(want.export()))
    with pytest.raises(im.HydiaError) as e:  # an empty batch
        receiver.encryptQueries(t[:0], seed=1, nonce0=1)
    assert e.value.code == ERR_ARG
    with pytest.raises(im.HydiaError) as e:
        im.DiagonalSender(cc, 100).encodeQueries(t[:0])
    assert e.value.code == ERR_ARG


# ------------------------------------------------------------------ 5. end to end
def test_end_to_end_from_tensors(im, torch):
    """small integers are exact in every type: a gallery enrolled from f16, probes encoded from f16 (a plain-query batch); a plain
    gallery enrolled from f32, probes encrypted from bf16 (a gallery batch); decryptIndex returns the planted rows"""
    cc = ctx(im)
    n = 300
    rng = np.random.default_rng(0)
    db = rng.integers(-99, 100, size=(n, DIM)).astype(np.float64)
    db[123] = rng.integers(1, 4, size=DIM)
    db[207] = -db[123]
    probes = np.stack([np.ones(DIM), -np.ones(DIM), db[5]])
    cos = (db / np.linalg.norm(db, axis=1, keepdims=True)) @ (probes / np.linalg.norm(probes, axis=1, keepdims=True)).T
    planted = [123, 207, 5]
    assert all(cos[planted[k], k] > 0.8 for k in range(3))
    receiver, sender = im.DiagonalReceiver(cc, n), im.DiagonalSender(cc, n)
    im.DiagonalEnroller(cc, n).serializeDB(torch.from_numpy(db).cuda().to(torch.float16), seed=31)
    pts = sender.encodeQueries(torch.from_numpy(probes).cuda().to(torch.float16))
    for k, res in enumerate(sender.indexScenarioPlainMulti(pts)):
        assert planted[k] in receiver.decryptIndex(res), k
    im.PlainEnroller(cc, n).serializeDB(torch.from_numpy(db).cuda().to(torch.float32))
    cts = receiver.encryptQueries(torch.from_numpy(probes).cuda().to(torch.bfloat16), seed=32, nonce0=1)
    for k, res in enumerate(sender.indexScenarioGalleryMulti(cts)):
        assert planted[k] in receiver.decryptIndex(res), k


# ------------------------------------------------------------------ 6. ordering
def test_rows_produced_on_another_stream_are_waited_for(im, torch):
    """the rows are the output of kernels enqueued on a non-default stream and not synchronised; that stream is the producer stream
    of the descriptor.  One case: the result is what the synchronised rows give"""
    cc = ctx(im)
    bits, D, _ = random_rows("f32", DIM)
    base = tensor(torch, bits[:9], "f32")
    work = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(20):  # something for the producer to be busy with before the rows exist
            work = (work @ work) * (1.0 / 2048)
        rows = base * 2.0 + work[:9, :DIM]  # (work stays all ones: exact)
        pts = im.DiagonalSender(cc, 100).encodeQueries(rows)
    torch.cuda.synchronize()
    want = im.DiagonalSender(cc, 100).encodeQueries(rows)
    assert np.array_equal(raw(torch, rows), raw(torch, base * 2.0 + 1.0))
    for a, b in zip(pts, want):
        assert np.array_equal(np.asarray(a.export()), np.asarray(b.export()))


# ------------------------------------------------------------------ 7. refusals
def test_refused_calls_leave_the_database_alone(im, torch):
    import image_matching_amd.hydia as H
    cc = ctx(im)
    L = cc.L
    n = 100
    bits, D, _ = random_rows("f32", DIM)
    good = tensor(torch, bits[:n], "f32")
    wide = torch.zeros((n, DIM + 8), dtype=torch.float32, device="cuda")
    seed = H._p(H._seed(3))
    im.DiagonalEnroller(cc, n).serializeDB(D[:n].copy(), seed=3)
    stats, before = cc.db_stats(), cc.db_export_ct(1)

    def desc(ptr=None, dtype=1, rows=n, stride=DIM):
        return H._DevRows(good.data_ptr() if ptr is None else ptr, dtype, rows, stride, None)

    def every_entry(d, c=cc):
        out = (C.c_void_p * 128)()
        dst = torch.empty((n, DIM), dtype=torch.float64, device="cuda")
        codes = [L.hydia_rows_widen_device(c.h, C.byref(d), 1, C.c_void_p(dst.data_ptr())),
                 L.hydia_db_enroll_device(c.h, C.byref(d), seed),
                 L.hydia_plain_db_enroll_device(c.h, C.byref(d)),
                 L.hydia_db_update_device(c.h, 0, C.byref(d), 1, seed),
                 L.hydia_plain_db_update_device(c.h, 0, C.byref(d), 1),
                 L.hydia_encrypt_queries_device(c.h, C.byref(d), seed, 1, out),
                 L.hydia_encode_queries_device(c.h, C.byref(d), out)]
        assert not any(out[i] for i in range(128))
        return codes

    host_rows = D[:n].copy()
    bad = {"a host pointer": desc(ptr=host_rows.ctypes.data, dtype=0),
           "row_stride < dim": desc(stride=DIM - 1),
           "dtype 7": desc(dtype=7),
           "a misaligned pointer": desc(ptr=wide.data_ptr() + 2, stride=DIM + 8)}
    for what, d in bad.items():
        assert every_entry(d) == [ERR_ARG] * 7, what
        assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(1), before), what
    assert np.array_equal(host_rows, D[:n])
    # the Python layer: another dtype, a last dimension that is not contiguous, a tensor that is not on a GPU
    for t in (good.to(torch.int32), good.t().contiguous().t(), good.cpu(), good[:, :DIM // 2]):
        with pytest.raises(im.HydiaError) as e:
            im.DiagonalSender(cc, n).encodeQueries(t)
        assert e.value.code == ERR_ARG
    # hydia_db_update_device on a plain gallery and the converse, each naming the other's entry point; then the right one works
    d = desc()
    assert L.hydia_plain_db_update_device(cc.h, 0, C.byref(d), 1) == ERR_STATE and "hydia_db_update" in L.hydia_last_error().decode()
    assert cc.db_stats() == stats and np.array_equal(cc.db_export_ct(1), before)
    im.PlainEnroller(cc, n).serializeDB(good)
    pstats, pbefore = cc.db_stats(), cc.plain_db_export_pt(1)
    assert L.hydia_db_update_device(cc.h, 0, C.byref(d), 1, seed) == ERR_STATE and "hydia_plain_db_update" in L.hydia_last_error().decode()
    assert cc.db_stats() == pstats and np.array_equal(cc.plain_db_export_pt(1), pbefore)
    hole = desc(rows=2)
    assert L.hydia_plain_db_update_device(cc.h, n + 1, C.byref(hole), 1) == ERR_ARG  # a hole
    empty = desc(rows=0)
    assert L.hydia_plain_db_update_device(cc.h, 0, C.byref(empty), 1) == 0 and L.hydia_plain_db_enroll_device(cc.h, C.byref(empty)) == ERR_ARG
    assert cc.db_stats() == pstats and np.array_equal(cc.plain_db_export_pt(1), pbefore)
    # no database resident; another kind resident (approach 4's); no public key
    fresh = im.Context(im.default_params(log_n=11, vector_dim=DIM), 0)
    try:
        assert L.hydia_db_update_device(fresh.h, 0, C.byref(d), 1, seed) == ERR_STATE
        assert L.hydia_plain_db_update_device(fresh.h, 0, C.byref(d), 1) == ERR_STATE
        out = (C.c_void_p * 128)()
        assert L.hydia_db_enroll_device(fresh.h, C.byref(d), seed) == ERR_STATE and "public key" in L.hydia_last_error().decode()
        assert L.hydia_encrypt_queries_device(fresh.h, C.byref(d), seed, 1, out) == ERR_STATE and "public key" in L.hydia_last_error().decode()
        assert fresh.db_kind() == 0 and fresh.db_stats() == (0, 0, 0) and not any(out[i] for i in range(128))
        # (no key is needed to encode)
        assert len(im.DiagonalSender(fresh, n).encodeQueries(good[:2])) == 2
        fresh.import_public_key(cc.export_public_key())
        im.HersEnroller(fresh, 10).serializeDB(D[:10].copy(), seed=4)
        kind, hstats, hbefore = fresh.db_kind(), fresh.db_stats(), fresh.db_export_ct(1)
        assert kind not in (5, 6, 7, 8)
        assert L.hydia_db_update_device(fresh.h, 0, C.byref(d), 1, seed) == ERR_STATE
        assert L.hydia_plain_db_update_device(fresh.h, 0, C.byref(d), 1) == ERR_STATE
        assert (fresh.db_kind(), fresh.db_stats()) == (kind, hstats) and np.array_equal(fresh.db_export_ct(1), hbefore)
    finally:
        fresh.close()
    # a shard context of a group
    grp = im.ShardGroup([0, 0], im.default_params(log_n=11, vector_dim=DIM))
    try:
        sc = grp.shard_ctx(0)
        sc.db_fill_random(n, 5)
        sstats, sbefore = sc.db_stats(), sc.db_export_ct(1)
        assert every_entry(d, sc) == [ERR_STATE] * 7
        assert "group" in L.hydia_last_error().decode()
        assert sc.db_stats() == sstats and np.array_equal(sc.db_export_ct(1), sbefore)
        with pytest.raises(im.HydiaError) as e:
            im.DiagonalEnroller(grp, n).serializeDB(good)
        assert e.value.code == ERR_STATE
    finally:
        grp.close()
