"""The semantics of the in-place database update (include/hydia.h, hydia_db_update) restated on the CPU oracle.  TEST
INFRASTRUCTURE ONLY: nothing here touches the product.

An update adds a FRESH encryption of a sparse diagonal image to the resident block ciphertexts:
  - a zero matrix with the given rows placed at their vector indices;
  - ciphertext t = g dim + i of every touched block g: the slot image hyo_enroll_layout_row (hoisted form) or
    hyo_enroll_layout_row_bsgs (pre-rotated form, B babies) makes of that matrix;
  - E = hyo_encrypt(image; seed, nonce = 2^36 + first_block dim + t);
  - block that existed: old + E (hyo_add_inplace); block the update creates: E.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

DB_NONCE_BASE = 1 << 36


class _CtList:
    """what Oracle.compute_similarity / index_scenario take for a database: .h = hy_ct **, len(), .bsgs, .babies"""

    def __init__(self, cts, dim, babies):
        self.keep = cts
        self.h = (C.c_void_p * len(cts))(*[c.h for c in cts])
        self.babies, self.bsgs = babies, babies < dim

    def __len__(self):
        return len(self.keep)


class UpdateRef:
    """The expected database, one oracle ciphertext per resident ciphertext.  Ciphertexts are never modified in place: an update
    REPLACES the entries it touches, so a fork() of an enrolment can be shared between tests."""

    def __init__(self, P, Or, babies=None):
        self.P, self.Or = P, Or
        self.B = P.dim if babies is None else int(babies)
        self.cts, self.n, self._keep = [], 0, []

    # ---- construction
    def enroll(self, db, seed):
        """the oracle's own enrolment (normalises db in place)"""
        arr = self.Or.enroll(db, seed, matvec=self.B)
        self._keep.append(arr)
        self.cts = [arr[t] for t in range(len(arr))]
        self.n = db.shape[0]
        return self

    def planted(self, n, cts):
        """a database whose ciphertexts were put there one by one (None = not known, never read)"""
        self.cts, self.n = list(cts), n
        return self

    def fork(self):
        r = UpdateRef(self.P, self.Or, self.B)
        r.cts, r.n, r._keep = list(self.cts), self.n, list(self._keep)
        return r

    # ---- the specification
    def blocks(self):
        return len(self.cts) // self.P.dim

    def image(self, Z, t):
        P = self.P
        slots = np.zeros(P.slots, dtype=np.float64)
        if self.B < P.dim:
            P.L.hyo_enroll_layout_row_bsgs(P.h, O._ptr(Z), Z.shape[0], t, O._ptr(slots), self.B)
        else:
            P.L.hyo_enroll_layout_row(P.h, O._ptr(Z), Z.shape[0], t, O._ptr(slots))
        return slots

    def update(self, first_vector, rows, normalise, seed, first_block=0):
        """returns the indices of the ciphertexts the update touches"""
        P = self.P
        assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.shape[1] == P.dim
        n = rows.shape[0]
        if n == 0:
            return []
        assert first_vector <= self.n  # no holes
        if normalise:
            for v in range(n):
                P.L.hyo_normalize(O._ptr(rows[v]), P.dim)
        n_new = max(self.n, first_vector + n)
        G_old, G_new = self.blocks(), -(-n_new // P.slots)
        Z = np.zeros((G_new * P.slots, P.dim), dtype=np.float64)  # a zero matrix with the rows placed
        Z[first_vector:first_vector + n] = rows
        touched = []
        for g in range(first_vector // P.slots, (first_vector + n - 1) // P.slots + 1):
            for i in range(P.dim):
                t = g * P.dim + i
                E = self.Or.encrypt(self.image(Z, t), seed, DB_NONCE_BASE + first_block * P.dim + t)
                if g < G_old:
                    s = self.cts[t].clone()
                    self.Or.add(s, E)
                    self.cts[t] = s
                else:
                    assert t == len(self.cts)
                    self.cts.append(E)
                touched.append(t)
        self.n = n_new
        return touched

    # ---- what the sender methods of the oracle take
    def array(self):
        return _CtList(self.cts, self.P.dim, self.B)


def saturated_ct(P, Or):
    """a ciphertext whose every residue is q_j - 1"""
    c = Or.encrypt(np.zeros(P.slots), 1, 1)
    d = c.data()
    for j in range(P.nQ):
        d[:, j, :] = P.moduli[j] - np.uint64(1)
    return c
