"""The specification of a plain gallery (include/hydia.h, hydia_plain_db_enroll; database kinds 7 / 8) restated on the CPU oracle.
TEST INFRASTRUCTURE ONLY: nothing here touches the product.

A plain gallery is, bit for bit, the oracle's existing sender path run on a database of TRIVIAL ciphertexts
(c0, c1) = (hyo_encode(image_t), 0):
  - image_t = the slot image hyo_enroll_layout_row (hoisted form) or hyo_enroll_layout_row_bsgs (pre-rotated form, B babies) makes
    of the normalised rows for ciphertext t = block * vector_dim + diagonal;
  - plaintext t = P.encode(image_t): scale 2^scale_bits, all n_q limbs, evaluation form, one polynomial;
  - hyo_mult_norelin with a trivial ciphertext gives d0, d1 = the plain residue products and d2 = 0, and hyo_relin_inplace leaves
    d0, d1 as they are (tests/test_plain_gallery_cpu.py), so hyo_compute_similarity[_bsgs], hyo_index_scenario[_bsgs] and
    hyo_membership_scenario[_bsgs] over the trivial ciphertexts are what the product must return.
"""
import ctypes as C

import numpy as np

import oracle_lib as O


class _CtList:
    """what Oracle.compute_similarity / index_scenario / membership_scenario take for a database: .h = hy_ct **, len(), .bsgs, .babies"""

    def __init__(self, cts, dim, babies):
        self.keep = cts
        self.h = (C.c_void_p * len(cts))(*[c.h for c in cts])
        self.babies, self.bsgs = babies, babies < dim

    def __len__(self):
        return len(self.keep)


def trivial_ct(P, m):
    """the ciphertext (m, 0) at scale 2^scale_bits on all n_q limbs; m = [n_q][N] residues in evaluation form"""
    c = O.Ct(P, P.L.hyo_ct_alloc(P.h, 2, P.nQ, P.delta))
    d = c.data()
    d[0] = m
    d[1] = 0
    return c


def pattern_poly(P, name):
    """[n_q][N] residues of one of the operand patterns of tests/test_gpu_loop_b_edges.py: "sat" (q - 1 everywhere), "holes" (q - 1 with
    one residue in 16 replaced by a small value that depends on its position), "uniform" (canonical residues from a seeded generator),
    "edge" (0, 1, q - 2, q - 1 in turn)"""
    out = np.zeros((P.nQ, P.N), dtype=np.uint64)
    c = np.arange(P.N, dtype=np.uint64)
    for j in range(P.nQ):
        q = P.moduli[j]
        if name == "sat":
            out[j] = q - np.uint64(1)
        elif name == "holes":
            out[j] = np.where(c % np.uint64(16) == np.uint64((5 * j + 3) % 16), c + np.uint64(j + 2), q - np.uint64(1))
        elif name == "uniform":
            out[j] = np.random.default_rng(1000 + j).integers(0, int(q), size=P.N, dtype=np.uint64)
        elif name == "edge":
            out[j] = np.choose(((c + np.uint64(j)) % np.uint64(4)).astype(np.int64), [np.uint64(0), np.uint64(1), q - np.uint64(2), q - np.uint64(1)])
        else:
            raise ValueError(name)
    return out


def pattern_ct(P, name):
    """a 2-component ciphertext whose two polynomials both carry the pattern (a stand-in for a query: any residues are a ciphertext)"""
    c = O.Ct(P, P.L.hyo_ct_alloc(P.h, 2, P.nQ, P.delta))
    d = c.data()
    d[0] = d[1] = pattern_poly(P, name)
    return c


_BLOCKS = {}  # (moduli, dim, babies, the block's normalised rows) -> its plaintexts and trivial ciphertexts, made on demand


class PlainRef:
    """The expected gallery of `rows` (normalised in place, like the product's enroller) in the form of `babies` hoisted rotations
    (None = vector_dim, the hoisted form).  A block's plaintexts depend on that block's `slots` rows alone (the enroller packs block
    by block: image(t) below against image_whole(t), tests/test_plain_gallery_cpu.py), so they are made once per distinct block and
    shared between the galleries of a test module — an encoding on the oracle takes milliseconds, a gallery has thousands."""

    def __init__(self, P, Or, rows, babies=None):
        assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.shape[1] == P.dim
        self.P, self.Or = P, Or
        self.B = P.dim if babies is None else int(babies)
        for v in range(rows.shape[0]):
            P.L.hyo_normalize(O._ptr(rows[v]), P.dim)
        self.rows, self.n = rows, rows.shape[0]
        self.n_pts = -(-self.n // P.slots) * P.dim
        self._blk, self._arr = {}, None

    def _layout(self, rows, t):
        P = self.P
        slots = np.zeros(P.slots, dtype=np.float64)
        if self.B < P.dim:
            P.L.hyo_enroll_layout_row_bsgs(P.h, O._ptr(rows), rows.shape[0], t, O._ptr(slots), self.B)
        else:
            P.L.hyo_enroll_layout_row(P.h, O._ptr(rows), rows.shape[0], t, O._ptr(slots))
        return slots

    def image_whole(self, t):
        """the enroller's slot image of ciphertext t, from the whole database"""
        return self._layout(self.rows, t)

    def _block(self, g):
        if g not in self._blk:
            P = self.P
            rows = np.ascontiguousarray(self.rows[g * P.slots:(g + 1) * P.slots])
            key = (P.moduli.tobytes(), P.dim, self.B, rows.tobytes())
            if key not in _BLOCKS:
                _BLOCKS[key] = {"rows": rows, "pt": {}, "ct": {}}
            self._blk[g] = _BLOCKS[key]
        return self._blk[g]

    def image(self, t):
        g, i = divmod(t, self.P.dim)
        return self._layout(self._block(g)["rows"], i)

    def encode(self, t):
        g, i = divmod(t, self.P.dim)
        b = self._block(g)
        if i not in b["pt"]:
            b["pt"][i] = self.P.encode(self._layout(b["rows"], i))
        return b["pt"][i]

    def trivial(self, t):
        g, i = divmod(t, self.P.dim)
        b = self._block(g)
        if i not in b["ct"]:
            b["ct"][i] = trivial_ct(self.P, self.encode(t))
        return b["ct"][i]

    def array(self):
        """the database of trivial ciphertexts the oracle's sender methods take (identical blocks share their ciphertexts: read-only)"""
        if self._arr is None:
            self._arr = _CtList([self.trivial(t) for t in range(self.n_pts)], self.P.dim, self.B)
        return self._arr


def pattern_array(P, name, n_pts, babies=None):
    """a database of n_pts identical trivial ciphertexts carrying the pattern (one oracle ciphertext, shared: the sender only reads)"""
    c = trivial_ct(P, pattern_poly(P, name))
    return _CtList([c] * n_pts, P.dim, P.dim if babies is None else int(babies))
