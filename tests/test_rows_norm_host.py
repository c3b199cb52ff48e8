"""Host checks of image_matching_amd/csrc/rows_norm.h (tests/csrc/rows_norm_check.cpp, g++ -O2 -ffp-contract=off): the widening of
every f16 and bf16 bit pattern against numpy, the row normalisation against the oracle's hyo_normalize — bit for bit — and a -Werror
compile of every C++ role overload that takes rows in device memory.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from device_rows_ref import BF16_NANS, F16_NANS, edge_rows, hyo_normalize_rows, same_bits, same_bits_nan_as_nan, widen_bits


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rows_norm") / "rows_norm_check"
    src = os.path.join(ROOT, "tests", "csrc", "rows_norm_check.cpp")
    inc = os.path.join(ROOT, "image_matching_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", inc, src, "-o", str(exe)], check=True)

    def run(*args):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (args, out.returncode, out.stdout + out.stderr)
    return run


@pytest.mark.parametrize("dtype,nans", [("f16", F16_NANS), ("bf16", BF16_NANS)])
def test_every_half_precision_pattern_widens_as_numpy_does(check, tmp_path, dtype, nans):
    check(dtype, tmp_path / "out.bin")
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    assert got.shape == (65536,)
    assert same_bits_nan_as_nan(got, widen_bits(np.arange(65536), dtype), nans)


def test_f32_patterns_widen_as_numpy_does(check, tmp_path):
    """every exponent with mantissas 0, 1, all ones and random ones, both signs (subnormals, infinities and NaNs among them)"""
    rng = np.random.default_rng(5)
    e = np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)
    m = np.concatenate([np.array([0, 1, 0x7FFFFF, 0x400000], dtype=np.uint32), rng.integers(0, 1 << 23, size=60, dtype=np.uint32)])[None, :]
    bits = np.concatenate([(e | m).ravel(), (e | m).ravel() | np.uint32(1 << 31)]).astype(np.uint32)
    bits.tofile(tmp_path / "in.bin")
    check("f32", tmp_path / "in.bin", tmp_path / "out.bin")
    want = widen_bits(bits, "f32")
    assert same_bits_nan_as_nan(np.fromfile(tmp_path / "out.bin", dtype=np.float64), want, int(np.isnan(want).sum()))


def normalised(check, tmp_path, rows):
    rows.tofile(tmp_path / "in.bin")
    check("norm", rows.shape[1], tmp_path / "in.bin", tmp_path / "out.bin")
    return np.fromfile(tmp_path / "out.bin", dtype=np.float64).reshape(rows.shape)


@pytest.mark.parametrize("dim", [8, 64, 512])
def test_normalisation_matches_the_oracle(check, tmp_path, dim):
    rng = np.random.default_rng(dim)
    rows = np.concatenate([rng.standard_normal((40, dim)), rng.integers(-99, 100, size=(40, dim)).astype(np.float64),
                           rng.standard_normal((8, dim)).astype(np.float16).astype(np.float64),
                           rng.standard_normal((8, dim)) * 1e-160, rng.standard_normal((8, dim)) * 1e150])
    assert same_bits(normalised(check, tmp_path, rows), hyo_normalize_rows(rows))


@pytest.mark.parametrize("dim", [8, 64, 512])
def test_normalisation_at_the_edges(check, tmp_path, dim):
    rows = edge_rows(dim).copy()
    got, want = normalised(check, tmp_path, rows), hyo_normalize_rows(rows)
    assert same_bits(got, want)
    # what the edges are there for: the zero row and the f64 subnormals pass through, the overflowing row becomes zeros
    assert same_bits(got[0], rows[0]) and same_bits(got[3], rows[3]) and not got[5].any() and np.count_nonzero(got[1]) == 1 and got[1][dim // 3] == -1.0
    assert not np.isnan(got).any()


ROLES_DEVICE_ROWS = r"""
#include "hydia_roles.hpp"
using namespace hydia;
int drive(CryptoContext cc, const void *dev, void *stream) {
    DeviceRows gallery(dev, HYDIA_F16, 1000, 512, stream), more(dev, HYDIA_BF16, 3, 520), probes(dev, HYDIA_F32, 8, 512, stream);
    DiagonalEnroller enroller(cc, gallery.size());
    enroller.serializeDB(gallery);
    bool ok = enroller.updateRows(5, more, false) && enroller.updateRows(5, more) && enroller.appendDB(more);
    PlainEnroller plain(cc, gallery.size());
    plain.serializeDB(gallery);
    ok = ok && plain.updateRows(5, more, false) && plain.updateRows(5, more) && plain.appendDB(more);
    DiagonalReceiver receiver(cc, enroller.size());
    std::vector<std::vector<Ciphertext>> queries = receiver.encryptQueries(probes);
    DiagonalSender sender(cc, plain.size());
    std::vector<Plaintext> known = sender.encodeQueries(probes);
    auto a = sender.indexScenarioGalleryMulti(queries);
    auto b = sender.indexScenarioPlainMulti(known);
    hydia_dev_rows raw = gallery.d;
    return (ok ? 0 : 1) + (int)a.size() + (int)b.size() + (int)raw.n + (int)(HYDIA_F64 + HYDIA_F32 + HYDIA_F16 + HYDIA_BF16);
}
int main() { return 0; }
"""


def test_roles_header_compiles_with_every_device_rows_overload(tmp_path):
    src = tmp_path / "roles_device_rows.cpp"
    src.write_text(ROLES_DEVICE_ROWS)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # and hydia.h alone, as C
    c = tmp_path / "abi.c"
    c.write_text('#include "hydia.h"\nint f(hydia_ctx *c, const hydia_dev_rows *r, double *d) { return hydia_rows_widen_device(c, r, 1, d); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
