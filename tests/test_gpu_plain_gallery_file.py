"""A plain gallery's file on the GPU (hydia_plain_db_save / hydia_plain_db_load; run with -m gpu): round trips through every resident
layout and form, the file's independence of the resident layout, bad headers and sizes, residues at or above their modulus (checked on
the device while the file streams in) and the two loaders refusing each other's files.  The header is the restatement of
tests/test_plain_gallery_update_cpu.py; ring, contexts and rows are those of tests/test_gpu_plain_gallery.py."""
import numpy as np
import pytest

import test_gpu_plain_gallery as base
from test_gpu_plain_gallery import enrol_plain, raw_rows, world
from test_plain_gallery_update_cpu import HEADER, poly_bytes, read_header, residue_offset, write_header

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def im():
    import image_matching_amd as im
    return im


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for P, K, Or, cc in base._CTX.values():
        cc.close()
    base._CTX.clear()


def shared(P, n):
    return raw_rows(P.dim, 16, P.slots)[:n].copy()


def state(cc):
    return cc.db_kind(), cc.db_babies(), cc.db_group(), cc.db_residue_bits(), cc.db_stats()


def all_plaintexts(cc):
    return [cc.plain_db_export_pt(t) for t in range(cc.db_stats()[1])]


def make_gallery(im, P, cc, case):
    """-> the vector count"""
    if case == "ct-major":
        n = 2 * P.slots - 3
        enrol_plain(im, cc, shared(P, n), "hoisted")
    elif case == "group-seq":
        n = 10 * P.slots - 3
        enrol_plain(im, cc, shared(P, n), "hoisted")
    elif case == "B8":
        n = 2 * P.slots - 3
        enrol_plain(im, cc, shared(P, n), 8)
    else:  # "updated": 2 blocks, a removal and an append that opens a third
        n0, n = 2 * P.slots - 3, 2 * P.slots + 9
        enrol_plain(im, cc, shared(P, n0), "hoisted")
        enr = im.PlainEnroller(cc, n0)
        enr.updateRows(17, -shared(P, 18)[17:18])
        enr.appendDB(shared(P, n)[n0:].copy())
        assert enr.numVectors == n
    return n


WANT = {"ct-major": (7, 64, 0, 48), "group-seq": (7, 64, 2, 46), "B8": (8, 8, 4, 46), "updated": (7, 64, 0, 48)}


# ------------------------------------------------------------------ 1. round trips
@pytest.mark.parametrize("case", ["ct-major", "group-seq", "B8", "updated"])
def test_round_trip(im, case, tmp_path):
    P, K, Or, cc = world(im)
    n = make_gallery(im, P, cc, case)
    st = state(cc)
    assert st[:2] == WANT[case][:2] and st[3] == WANT[case][3] and (st[2] > 0) == (WANT[case][2] > 0) and st[4][0] == n
    pts = all_plaintexts(cc)
    sender, receiver = im.DiagonalSender(cc, n), im.DiagonalReceiver(cc, n)
    qc = receiver.encryptQuery(np.ones(P.dim), seed=5, nonce=1)
    idx = np.asarray(sender.indexScenario(qc).export())
    path = tmp_path / "gallery.db"
    cc.plain_db_save(path)
    h = read_header(path.read_bytes()[:HEADER.size])
    assert h["magic"] == b"HYDIADB1" and (h["logN"], h["nQ"], h["dim"], h["packed"]) == (11, P.nQ, P.dim, 1)
    assert (h["kind"], h["babies"], h["n_vectors"], h["n_cts"]) == (st[0], st[1], n, st[4][1])
    assert h["ct_bytes"] == poly_bytes(P.N, P.nQ, True) and h["moduli"][:P.nQ] == [int(x) for x in P.moduli[:P.nQ]]
    assert path.stat().st_size == HEADER.size + h["n_cts"] * h["ct_bytes"]
    im.DiagonalEnroller(cc, 300).serializeDB(shared(P, 300), seed=1)  # something else resident in between
    assert cc.db_kind() in (5, 6)
    cc.set_matvec(4 if case != "B8" else "hoisted")  # a loaded gallery takes the form the file declares, whatever the policy says
    try:
        cc.plain_db_load(path)
    finally:
        cc.set_matvec("auto")
    assert state(cc) == st
    for t, want in enumerate(pts):
        assert np.array_equal(cc.plain_db_export_pt(t), want), t
    assert np.array_equal(np.asarray(im.DiagonalSender(cc, n).indexScenario(qc).export()), idx)


# ------------------------------------------------------------------ 2. the file does not depend on the resident layout
def test_file_is_the_same_from_either_layout(im, tmp_path, monkeypatch):
    P, K, Or, cc = world(im)
    n = make_gallery(im, P, cc, "group-seq")
    assert cc.db_group() == 2 and cc.db_residue_bits() == 46
    first, second = tmp_path / "seq.db", tmp_path / "ctm.db"
    cc.plain_db_save(first)
    monkeypatch.setenv("HYDIA_DB_CT_MAJOR", "1")
    other = im.Context(im.default_params(log_n=11, vector_dim=P.dim), 0)
    monkeypatch.delenv("HYDIA_DB_CT_MAJOR")
    try:
        other.plain_db_load(first)
        assert other.db_group() == 0 and other.db_residue_bits() == 48 and other.db_kind() == 7 and other.db_stats()[:2] == (n, 10 * P.dim)
        for t in (0, 3 * P.dim + 7, 10 * P.dim - 1):
            assert np.array_equal(other.plain_db_export_pt(t), cc.plain_db_export_pt(t)), t
        other.plain_db_save(second)
    finally:
        other.close()
    assert first.read_bytes() == second.read_bytes()


# ------------------------------------------------------------------ 3. bad files
@pytest.fixture(scope="module")
def saved(im, tmp_path_factory):
    """the files the bad ones are crafted from: 2 blocks hoisted, 2 blocks at B = 8, 10 blocks — and a ciphertext database's"""
    P, K, Or, cc = world(im)
    d = tmp_path_factory.mktemp("plain_files")
    out = {}
    for case in ("ct-major", "B8", "group-seq"):
        make_gallery(im, P, cc, case)
        cc.plain_db_save(d / (case + ".db"))
        out[case] = (d / (case + ".db")).read_bytes()
    cc.set_matvec("hoisted")
    try:
        im.DiagonalEnroller(cc, 300).serializeDB(shared(P, 300), seed=9)
    finally:
        cc.set_matvec("auto")
    cc.db_save(d / "enc.db")
    out["enc"] = (d / "enc.db").read_bytes()
    return out


def edited(raw, **fields):
    h = read_header(raw[:HEADER.size])
    for k, v in fields.items():
        if k == "prime":
            h["moduli"][v] += 2
        else:
            h[k] = v
    return write_header(h) + raw[HEADER.size:]


def resident_sample(im, P, cc):
    """a small plain gallery resident, and what must still be there after a refused load"""
    enrol_plain(im, cc, shared(P, 500), "hoisted")
    return state(cc), {t: cc.plain_db_export_pt(t) for t in (0, 31, P.dim - 1)}


def check_untouched(cc, st, sample):
    assert state(cc) == st
    for t, want in sample.items():
        assert np.array_equal(cc.plain_db_export_pt(t), want), t


def test_bad_files_are_refused_with_the_resident_gallery_untouched(im, saved, tmp_path):
    P, K, Or, cc = world(im)
    raw, raw8 = saved["ct-major"], saved["B8"]
    h = read_header(raw[:HEADER.size])
    bad = {
        "truncated by one byte": raw[:-1],
        "one trailing byte": raw + b"\0",
        "other dim": edited(raw, dim=32),
        "another prime": edited(raw, prime=3),
        "n_cts off by dim": edited(raw, n_cts=h["n_cts"] + P.dim),
        "n_cts short by dim": edited(raw, n_cts=h["n_cts"] - P.dim),
        "kind 8 with a baby count of 3": edited(raw8, babies=3),
        "an unknown kind": edited(raw, kind=9),
        "not a database file": b"HYDIADB2" + raw[8:],
    }
    st, sample = resident_sample(im, P, cc)
    for name, data in bad.items():
        path = tmp_path / "bad.db"
        path.write_bytes(data)
        with pytest.raises(im.HydiaError) as e:
            cc.plain_db_load(path)
        assert e.value.code == ERR_ARG, (name, str(e.value))
        check_untouched(cc, st, sample)
    path = tmp_path / "good.db"  # and the file they were made from loads
    path.write_bytes(raw)
    cc.plain_db_load(path)
    assert cc.db_stats()[:2] == (h["n_vectors"], h["n_cts"]) and cc.db_kind() == 7


# ------------------------------------------------------------------ 4. a residue at or above its modulus
@pytest.mark.parametrize("case,t,j,c,value", [("ct-major", 70, 0, 1001, "q"), ("group-seq", 5 * 64 + 3, 4, 777, 2 ** 46 - 1),
                                              ("group-seq", 10 * 64 - 1, 11, 2047, "q")],
                         ids=["q0-in-limb0", "2^46-1-in-a-packed-limb", "q-in-the-last-residue"])
def test_a_residue_at_or_above_its_modulus_leaves_no_database(im, saved, tmp_path, case, t, j, c, value):
    """the default chain's scaling primes are below 2^46 (a 10-block gallery is resident in 46-bit fields), the file carries 48-bit
    ones: the check is made on the unpacked residues of every chunk, on the device, before they are stored"""
    P, K, Or, cc = world(im)
    raw = bytearray(saved[case])
    v = int(P.moduli[j]) if value == "q" else value
    assert v >= int(P.moduli[j])
    off, width = residue_offset(P.N, P.nQ, True, t, j, c)
    assert int.from_bytes(raw[off:off + width], "little") < int(P.moduli[j])
    raw[off:off + width] = v.to_bytes(width, "little")
    path = tmp_path / "bad.db"
    path.write_bytes(bytes(raw))
    resident_sample(im, P, cc)
    with pytest.raises(im.HydiaError) as e:
        cc.plain_db_load(path)
    assert e.value.code == ERR_ARG and "modulus" in str(e.value)
    assert cc.db_kind() == 0 and cc.db_stats() == (0, 0, 0)
    raw[off:off + width] = (int(P.moduli[j]) - 1).to_bytes(width, "little")  # the largest canonical residue is served
    path.write_bytes(bytes(raw))
    cc.plain_db_load(path)
    assert cc.db_kind() == 7 and int(cc.plain_db_export_pt(t)[j, c]) == int(P.moduli[j]) - 1


# ------------------------------------------------------------------ 5. the two kinds of file, and the other states
def test_each_loader_refuses_the_other_kind_of_file(im, saved, tmp_path):
    P, K, Or, cc = world(im)
    plain, enc = tmp_path / "plain.db", tmp_path / "enc.db"
    plain.write_bytes(saved["ct-major"])
    enc.write_bytes(saved["enc"])
    st, sample = resident_sample(im, P, cc)
    with pytest.raises(im.HydiaError) as e:
        cc.db_load(plain)
    assert e.value.code == ERR_ARG and "plain gallery" in str(e.value) and "hydia_plain_db_load" in str(e.value)
    check_untouched(cc, st, sample)
    with pytest.raises(im.HydiaError) as e:
        cc.plain_db_load(enc)
    assert e.value.code == ERR_ARG and "hydia_db_load" in str(e.value)
    check_untouched(cc, st, sample)
    # a ciphertext database resident: the same refusals, and no plain file is written of it
    cc.db_load(enc)
    assert cc.db_kind() == 5
    ct = cc.db_export_ct(7)
    with pytest.raises(im.HydiaError) as e:
        cc.db_load(plain)
    assert e.value.code == ERR_ARG and cc.db_kind() == 5 and np.array_equal(cc.db_export_ct(7), ct)
    out = tmp_path / "out.db"
    with pytest.raises(im.HydiaError) as e:
        cc.plain_db_save(out)
    assert e.value.code == ERR_STATE and not out.exists()
    assert np.array_equal(cc.db_export_ct(7), ct)
    # no database at all; and a shard of a group
    fresh = im.Context(im.default_params(log_n=11, vector_dim=64), 0)
    try:
        with pytest.raises(im.HydiaError) as e:
            fresh.plain_db_save(out)
        assert e.value.code == ERR_STATE and not out.exists()
    finally:
        fresh.close()
    grp = im.ShardGroup([0, 0], im.default_params(log_n=11, vector_dim=64))
    try:
        sc = grp.shard_ctx(0)
        with pytest.raises(im.HydiaError) as e:
            sc.plain_db_load(plain)
        assert e.value.code == ERR_STATE and "plain gallery" in str(e.value)
        assert sc.db_kind() == 0 and sc.db_stats() == (0, 0, 0)
    finally:
        grp.close()
