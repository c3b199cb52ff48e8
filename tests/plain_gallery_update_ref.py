"""The semantics of the in-place update of a plain gallery (include/hydia.h, hydia_plain_db_update) restated on the CPU oracle.
TEST INFRASTRUCTURE ONLY: nothing here touches the product.

An update adds the ENCODING of a sparse diagonal image to the resident block plaintexts:
  - a block's rows that are zero everywhere except the updated slots;
  - plaintext t = g dim + i of every touched block g: the slot image hyo_enroll_layout_row (hoisted form) or
    hyo_enroll_layout_row_bsgs (pre-rotated form, B babies) makes of those rows for diagonal i;
  - E = P.encode(image): scale 2^scale_bits, all n_q limbs, evaluation form, one polynomial — no seed, no nonce;
  - block that existed: (old + E) mod q_j, residue by residue; block the update creates: E.
The oracle's scenarios take the gallery as TRIVIAL ciphertexts (m, 0), as tests/plain_gallery_ref.py makes them.
"""
import numpy as np

import oracle_lib as O
from plain_gallery_ref import _CtList, trivial_ct


def add_mod(P, a, b):
    """(a + b) mod q_j per limb; a, b [n_q][N] canonical residues (below 2^63, so the sum does not wrap)"""
    q = P.moduli[:P.nQ].astype(np.uint64)[:, None]
    s = a + b
    return np.where(s >= q, s - q, s)


class PlainUpdateRef:
    """The expected gallery, one [n_q][N] array per resident plaintext (None = not known, never read).  Arrays are never modified
    in place: an update REPLACES the entries it touches."""

    def __init__(self, P, babies=None):
        self.P = P
        self.B = P.dim if babies is None else int(babies)
        self.pts, self.n = [], 0

    # ---- construction
    def enroll(self, ref, blocks=None):
        """from tests/plain_gallery_ref.PlainRef (an enrolment of the same form); blocks: the only ones a test will look at"""
        assert ref.B == self.B
        dim = self.P.dim
        self.pts = [ref.encode(t) if blocks is None or t // dim in blocks else None for t in range(ref.n_pts)]
        self.n = ref.n
        return self

    def planted(self, n, pts):
        self.pts, self.n = list(pts), n
        return self

    def fork(self):
        r = PlainUpdateRef(self.P, self.B)
        r.pts, r.n = list(self.pts), self.n
        return r

    # ---- the specification
    def blocks(self):
        return len(self.pts) // self.P.dim

    def image(self, Z, i):
        """diagonal i of ONE block whose rows are Z (slots x dim)"""
        P = self.P
        slots = np.zeros(P.slots, dtype=np.float64)
        if self.B < P.dim:
            P.L.hyo_enroll_layout_row_bsgs(P.h, O._ptr(Z), Z.shape[0], i, O._ptr(slots), self.B)
        else:
            P.L.hyo_enroll_layout_row(P.h, O._ptr(Z), Z.shape[0], i, O._ptr(slots))
        return slots

    def encodings(self, first_vector, rows):
        """{t: E_t} for every plaintext of the blocks that rows placed at first_vector .. touch (rows as given)"""
        P = self.P
        n, out = rows.shape[0], {}
        for g in range(first_vector // P.slots, (first_vector + n - 1) // P.slots + 1):
            Z = np.zeros((P.slots, P.dim), dtype=np.float64)  # the block, zero except the updated slots
            lo, hi = max(first_vector, g * P.slots), min(first_vector + n, (g + 1) * P.slots)
            Z[lo - g * P.slots:hi - g * P.slots] = rows[lo - first_vector:hi - first_vector]
            for i in range(P.dim):
                out[g * P.dim + i] = P.encode(self.image(Z, i))
        return out

    def update(self, first_vector, rows, normalise):
        """returns the indices of the plaintexts the update touches"""
        P = self.P
        assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.shape[1] == P.dim
        n = rows.shape[0]
        if n == 0:
            return []
        assert first_vector <= self.n  # no holes
        if normalise:
            for v in range(n):
                P.L.hyo_normalize(O._ptr(rows[v]), P.dim)
        G_old = self.blocks()
        touched = []
        for t, E in sorted(self.encodings(first_vector, rows).items()):
            if t // P.dim < G_old:
                self.pts[t] = add_mod(P, self.pts[t], E)
            else:
                assert t == len(self.pts)
                self.pts.append(E)
            touched.append(t)
        self.n = max(self.n, first_vector + n)
        return touched

    # ---- what the sender methods of the oracle take
    def array(self):
        """a list of trivial ciphertexts made from the expected polynomials"""
        return trivial_array(self.P, self.pts, self.B)


def trivial_array(P, polys, babies=None):
    return _CtList([trivial_ct(P, m) for m in polys], P.dim, P.dim if babies is None else int(babies))
