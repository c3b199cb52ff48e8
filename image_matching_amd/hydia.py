"""ctypes host layer over libhydia.so (include/hydia.h).

Mirrors the reference's class surface for approach 5 so parity tests read like the reference's driver
(/root/reference/src/main.cpp:302-374):
    DiagonalEnroller(cc, n).serializeDB(db)            include/enroller_diag.h:7-27
    DiagonalReceiver(cc, n).encryptQuery(q) / decryptMembership(ct) / decryptIndex(cts)   include/receiver.h:17-43
    DiagonalSender(cc, n).computeSimilarity / membershipScenario / indexScenario          include/sender.h:19-43
`cc` is a Context (replaces CryptoContext + keys).  There is no CPU fallback: a missing library or GPU raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class HydiaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hydia error %d: %s" % (code, msg))
        self.code = code


class _Params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("log_n", "mult_depth", "scale_bits", "first_mod_bits", "dnum", "vector_dim")]


class _DevRows(C.Structure):  # hydia_dev_rows
    _fields_ = [("ptr", C.c_void_p), ("dtype", C.c_int), ("n", C.c_size_t), ("row_stride", C.c_size_t), ("stream", C.c_void_p)]


class _Info(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("log_n", "n", "slots", "n_q", "n_p", "dnum", "alpha", "vector_dim")] + [
        ("delta", C.c_double)]


class _DeltaInfo(C.Structure):  # hydia_db_delta_info
    _fields_ = [("version", C.c_uint32), ("vector_dim", C.c_uint32)] + [
        (n, C.c_uint64) for n in ("babies", "first_vector", "n_rows", "first_block", "n_blocks", "total_bytes")]


class _WireInfo(C.Structure):  # hydia_wire_info
    _fields_ = [(n, C.c_uint32) for n in ("type", "log_n", "n_polys", "n_limbs", "rot", "reserved")] + [
        ("count", C.c_uint64), ("scale", C.c_double), ("a_seed", C.c_uint8 * 32), ("nonce0", C.c_uint64), ("header_bytes", C.c_uint64),
        ("payload_bytes", C.c_uint64)]


def lib_path():
    # HYDIA_LIBPATH: an alternative build of the same library (kernel A/B experiments, tools/ubench)
    return os.environ.get("HYDIA_LIBPATH") or os.path.join(_HERE, "libhydia.so")


def build_library():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")])


def load_library():
    """Load libhydia.so; raises if it has not been built (no fallback of any kind)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise HydiaError(-3, "libhydia.so is not built (%s missing): run __graft_entry__.build() or "
                             "make -C image_matching_amd/csrc" % path)
    L = C.CDLL(path)
    vp, u64, sz, dbl, i32, u32 = C.c_void_p, C.c_uint64, C.c_size_t, C.c_double, C.c_int, C.c_uint32
    pp = C.POINTER(C.c_void_p)
    sig = {
        "hydia_last_error": (C.c_char_p, []),
        "hydia_version": (C.c_char_p, []),
        "hydia_default_params": (None, [C.POINTER(_Params)]),
        "hydia_params_describe": (i32, [C.POINTER(_Params), C.POINTER(_Info), vp, vp]),
        "hydia_compute_required_depth": (sz, [sz]),
        "hydia_ctx_create": (i32, [C.POINTER(_Params), i32, pp]),
        "hydia_ctx_create_custom": (i32, [C.POINTER(_Params), vp, vp, u32, u32, i32, pp]),
        "hydia_ctx_destroy": (None, [vp]),
        "hydia_get_info": (i32, [vp, C.POINTER(_Info)]),
        "hydia_get_moduli": (i32, [vp, vp, vp]),
        "hydia_sync": (i32, [vp]),
        "hydia_memory_stats": (i32, [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
        "hydia_keygen": (i32, [vp, vp]),
        "hydia_import_eval_key": (i32, [vp, i32, vp]),
        "hydia_export_eval_key": (i32, [vp, i32, vp]),
        "hydia_import_public_key": (i32, [vp, vp]),
        "hydia_import_secret_key": (i32, [vp, vp]),
        "hydia_export_public_key": (i32, [vp, vp]),
        "hydia_export_secret_key": (i32, [vp, vp]),
        "hydia_has_eval_key": (i32, [vp, i32]),
        "hydia_fill_eval_keys_random": (i32, [vp, u64]),
        "hydia_ct_import": (i32, [vp, vp, u32, u32, u32, dbl, pp]),
        "hydia_ct_export": (i32, [vp, vp, vp]),
        "hydia_ct_shape": (i32, [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(dbl)]),
        "hydia_ct_device_ptr": (i32, [vp, pp, C.POINTER(sz)]),
        "hydia_ct_from_device": (i32, [vp, vp, u32, u32, u32, dbl, pp]),
        "hydia_ct_copy_to_device": (i32, [vp, vp, vp]),
        "hydia_ct_view_device": (i32, [vp, vp, u32, u32, u32, dbl, pp]),
        "hydia_rotate_query_range_into": (i32, [vp, vp, u32, u32, vp]),
        "hydia_rotate_query_range": (i32, [vp, vp, u32, u32, pp]),
        "hydia_compute_similarity_rotated": (i32, [vp, vp, pp]),
        "hydia_index_scenario_rotated": (i32, [vp, vp, pp]),
        "hydia_group_set_rotation_split": (i32, [vp, i32]),
        "hydia_ct_free": (None, [vp]),
        "hydia_encrypt_query": (i32, [vp, vp, vp, u64, pp]),
        "hydia_encrypt": (i32, [vp, vp, u32, vp, u64, pp]),
        "hydia_decrypt": (i32, [vp, vp, vp]),
        "hydia_decrypt_membership": (i32, [vp, vp, C.POINTER(i32)]),
        "hydia_decrypt_index": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
        "hydia_decrypt_device": (i32, [vp, vp, vp]),
        "hydia_slots_select_device": (i32, [vp, vp, sz, dbl, vp, vp, sz, vp]),
        "hydia_slots_topk_device": (i32, [vp, vp, sz, sz, vp, vp, vp]),
        "hydia_decrypt_matches": (i32, [vp, vp, sz, dbl, vp, vp, sz, vp]),
        "hydia_decrypt_topk": (i32, [vp, vp, sz, sz, vp, vp, vp]),
        "hydia_decrypt_matches_multi": (i32, [vp, vp, u32, sz, dbl, vp, vp, sz, vp]),
        "hydia_decrypt_topk_multi": (i32, [vp, vp, u32, sz, sz, vp, vp, vp]),
        "hydia_db_num_cts": (sz, [vp, sz]),
        "hydia_db_enroll": (i32, [vp, vp, sz, vp]),
        "hydia_db_alloc": (i32, [vp, sz]),
        "hydia_plain_db_enroll": (i32, [vp, vp, sz]),
        "hydia_plain_db_alloc": (i32, [vp, sz, i32]),
        "hydia_plain_db_import_pt": (i32, [vp, sz, vp]),
        "hydia_plain_db_export_pt": (i32, [vp, sz, vp]),
        "hydia_plain_db_update": (i32, [vp, sz, vp, sz, i32]),
        "hydia_plain_db_save": (i32, [vp, C.c_char_p]),
        "hydia_plain_db_load": (i32, [vp, C.c_char_p]),
        "hydia_encode_query": (i32, [vp, vp, pp]),
        "hydia_pt_import": (i32, [vp, vp, dbl, pp]),
        "hydia_pt_export": (i32, [vp, vp, vp]),
        "hydia_pt_free": (None, [vp]),
        "hydia_compute_similarity_pq": (i32, [vp, vp, pp]),
        "hydia_index_scenario_pq": (i32, [vp, vp, pp]),
        "hydia_membership_scenario_pq": (i32, [vp, vp, pp]),
        "hydia_compute_similarity_pq_multi": (i32, [vp, vp, u32, vp]),
        "hydia_index_scenario_pq_multi": (i32, [vp, vp, u32, vp]),
        "hydia_membership_scenario_pq_multi": (i32, [vp, vp, u32, vp]),
        "hydia_set_pq_batch_width": (i32, [vp, u32]),
        "hydia_rows_widen_device": (i32, [vp, C.POINTER(_DevRows), i32, vp]),
        "hydia_db_enroll_device": (i32, [vp, C.POINTER(_DevRows), vp]),
        "hydia_plain_db_enroll_device": (i32, [vp, C.POINTER(_DevRows)]),
        "hydia_db_update_device": (i32, [vp, sz, C.POINTER(_DevRows), i32, vp]),
        "hydia_plain_db_update_device": (i32, [vp, sz, C.POINTER(_DevRows), i32]),
        "hydia_encrypt_queries_device": (i32, [vp, C.POINTER(_DevRows), vp, u64, vp]),
        "hydia_encode_queries_device": (i32, [vp, C.POINTER(_DevRows), vp]),
        "hydia_keygen_seeded": (i32, [vp, vp, vp]),
        "hydia_keygen_rotations_seeded": (i32, [vp, vp, vp, vp, u32]),
        "hydia_get_key_seed": (i32, [vp, vp]),
        "hydia_eval_key_seeded_words": (sz, [vp]),
        "hydia_export_eval_key_seeded": (i32, [vp, i32, vp]),
        "hydia_export_public_key_seeded": (i32, [vp, vp]),
        "hydia_import_eval_key_seeded": (i32, [vp, i32, vp, vp]),
        "hydia_import_public_key_seeded": (i32, [vp, vp, vp]),
        "hydia_encrypt_query_seeded": (i32, [vp, vp, vp, vp, u64, vp]),
        "hydia_encrypt_queries_seeded": (i32, [vp, vp, sz, vp, vp, u64, vp]),
        "hydia_encrypt_queries_seeded_device": (i32, [vp, C.POINTER(_DevRows), vp, vp, u64, vp]),
        "hydia_ct_expand_seeded": (i32, [vp, vp, sz, vp, u64, vp]),
        "hydia_wire_peek": (i32, [vp, sz, C.POINTER(_WireInfo)]),
        "hydia_wire_ct_bytes": (sz, [vp, u64, u32, u32, i32]),
        "hydia_wire_eval_key_bytes": (sz, [vp, i32]),
        "hydia_wire_public_key_bytes": (sz, [vp, i32]),
        "hydia_ct_to_wire": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
        "hydia_ct_from_wire": (i32, [vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "hydia_encrypt_queries_seeded_wire": (i32, [vp, vp, sz, vp, vp, u64, vp, sz, C.POINTER(sz)]),
        "hydia_encrypt_queries_seeded_wire_device": (i32, [vp, C.POINTER(_DevRows), vp, vp, u64, vp, sz, C.POINTER(sz)]),
        "hydia_key_to_wire": (i32, [vp, i32, i32, vp, sz, C.POINTER(sz)]),
        "hydia_key_from_wire": (i32, [vp, vp, sz, C.POINTER(i32)]),
        "hydia_keys_save": (i32, [vp, C.c_char_p, i32]),
        "hydia_keys_load": (i32, [vp, C.c_char_p]),
        "hydia_db_delta_bytes": (i32, [vp, sz, sz, C.POINTER(sz)]),
        "hydia_db_delta_peek": (i32, [vp, sz, C.POINTER(_DeltaInfo)]),
        "hydia_db_delta_make": (i32, [vp, sz, vp, sz, i32, vp, i32, sz, vp, sz, C.POINTER(sz)]),
        "hydia_db_delta_make_device": (i32, [vp, sz, C.POINTER(_DevRows), i32, vp, i32, sz, vp, sz, C.POINTER(sz)]),
        "hydia_db_delta_apply": (i32, [vp, vp, sz]),
        "hydia_db_delta_seeded_bytes": (i32, [vp, sz, sz, C.POINTER(sz)]),
        "hydia_db_delta_seeded_peek": (i32, [vp, sz, C.POINTER(_DeltaInfo)]),
        "hydia_db_delta_make_seeded": (i32, [vp, sz, vp, sz, i32, vp, vp, i32, sz, vp, sz, C.POINTER(sz)]),
        "hydia_db_delta_make_seeded_device": (i32, [vp, sz, C.POINTER(_DevRows), i32, vp, vp, i32, sz, vp, sz, C.POINTER(sz)]),
        "hydia_db_delta_apply_seeded": (i32, [vp, vp, sz]),
        "hydia_compute_similarity_gallery_multi": (i32, [vp, vp, u32, vp]),
        "hydia_index_scenario_gallery_multi": (i32, [vp, vp, u32, vp]),
        "hydia_membership_scenario_gallery_multi": (i32, [vp, vp, u32, vp]),
        "hydia_set_gallery_batch_width": (i32, [vp, u32]),
        "hydia_db_import_ct": (i32, [vp, sz, vp]),
        "hydia_db_export_ct": (i32, [vp, sz, vp]),
        "hydia_db_fill_random": (i32, [vp, sz, u64]),
        "hydia_db_save": (i32, [vp, C.c_char_p]),
        "hydia_db_load": (i32, [vp, C.c_char_p]),
        "hydia_db_stats": (i32, [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "hydia_rotate_query": (i32, [vp, vp, pp]),
        "hydia_compute_similarity": (i32, [vp, vp, pp]),
        "hydia_index_scenario": (i32, [vp, vp, pp]),
        "hydia_membership_scenario": (i32, [vp, vp, pp]),
        "hydia_compute_similarity_multi": (i32, [vp, vp, u32, vp]),
        "hydia_index_scenario_multi": (i32, [vp, vp, u32, vp]),
        "hydia_membership_scenario_multi": (i32, [vp, vp, u32, vp]),
        "hydia_chebyshev_compare": (i32, [vp, vp, dbl, sz, pp]),
        "hydia_sum_and_evalsum": (i32, [vp, vp, pp]),
        "hydia_add_many": (i32, [vp, vp, pp]),
        "hydia_eval_sum": (i32, [vp, vp, pp]),
        "hydia_ct_add_raw": (i32, [vp, vp, vp, i32]),
        "hydia_ct_mod_reduce": (i32, [vp, vp]),
        "hydia_db_enroll_shard": (i32, [vp, vp, sz, vp, sz]),
        "hydia_db_update": (i32, [vp, sz, vp, sz, i32, vp]),
        "hydia_db_update_shard": (i32, [vp, sz, vp, sz, i32, vp, sz]),
        "hydia_keygen_switch": (i32, [vp, vp, vp, vp]),
        "hydia_db_rekey": (i32, [vp, vp]),
        "hydia_db_rekey_chunked": (i32, [vp, vp, i32]),
        "hydia_switch_key_words": (sz, [vp]),
        "hydia_db_enroll_shard_ex": (i32, [vp, vp, sz, vp, sz, i32]),
        "hydia_set_matvec": (i32, [vp, i32]),
        "hydia_get_matvec": (i32, [vp]),
        "hydia_db_kind": (i32, [vp]),
        "hydia_db_group": (i32, [vp]),
        "hydia_db_babies": (i32, [vp]),
        "hydia_db_set_babies": (i32, [vp, i32]),
        "hydia_auto_babies": (i32, [vp, sz]),
        "hydia_random_seed": (i32, [vp]),
        "hydia_shard_blocks": (None, [sz, u32, u32, C.POINTER(sz), C.POINTER(sz)]),
        "hydia_group_create": (i32, [C.POINTER(_Params), C.POINTER(i32), u32, pp]),
        "hydia_group_destroy": (None, [vp]),
        "hydia_group_size": (u32, [vp]),
        "hydia_group_ctx": (vp, [vp, u32]),
        "hydia_group_keygen": (i32, [vp, vp]),
        "hydia_group_db_enroll": (i32, [vp, vp, sz, vp]),
        "hydia_group_shard_range": (i32, [vp, u32, C.POINTER(sz), C.POINTER(sz)]),
        "hydia_group_compute_similarity": (i32, [vp, vp, pp]),
        "hydia_group_index_scenario": (i32, [vp, vp, pp]),
        "hydia_group_membership_scenario": (i32, [vp, vp, pp]),
        "hydia_hers_db_enroll": (i32, [vp, vp, sz, vp]),
        "hydia_hers_encrypt_query": (i32, [vp, vp, vp, u64, pp]),
        "hydia_hers_compute_similarity": (i32, [vp, vp, pp]),
        "hydia_hers_index_scenario": (i32, [vp, vp, pp]),
        "hydia_hers_membership_scenario": (i32, [vp, vp, pp]),
        "hydia_ntt": (i32, [vp, vp, u32, u32, i32]),
        "hydia_ntt_engine": (i32, [vp]),
        "hydia_eval_rotate": (i32, [vp, vp, i32, pp]),
        "hydia_eval_mult": (i32, [vp, vp, vp, pp]),
        "hydia_eval_mult_no_relin": (i32, [vp, vp, vp, pp]),
        "hydia_relinearize": (i32, [vp, vp]),
        "hydia_rescale": (i32, [vp, vp]),
        "hydia_eval_add": (i32, [vp, vp, vp]),
        "hydia_level_reduce": (i32, [vp, vp, u32]),
        "hydia_params_for_approach": (i32, [sz, vp]),
        "hydia_keygen_rotations": (i32, [vp, vp, vp, u32]),
        "hydia_eval_mult_plain": (i32, [vp, vp, vp, pp]),
        "hydia_binary_rotate": (i32, [vp, vp, i32, pp]),
        "hydia_base_db_num_cts": (sz, [vp, sz]),
        "hydia_base_db_enroll": (i32, [vp, vp, sz, vp]),
        "hydia_base_compute_similarity": (i32, [vp, vp, pp]),
        "hydia_base_index_scenario": (i32, [vp, vp, pp]),
        "hydia_base_membership_scenario": (i32, [vp, vp, pp]),
        "hydia_merge_ciphers": (i32, [vp, vp, sz, pp]),
        "hydia_base_rotations": (i32, [u32, vp, sz, C.POINTER(sz)]),
        "hydia_grote_row_length": (u32, [u32]),
        "hydia_alpha_norm_rows": (i32, [vp, vp, sz, sz, pp]),
        "hydia_alpha_norm_columns": (i32, [vp, vp, sz, sz, pp]),
        "hydia_grote_index_scenario": (i32, [vp, vp, pp, pp]),
        "hydia_grote_membership_scenario": (i32, [vp, vp, pp]),
        "hydia_grote_decrypt_index": (i32, [vp, vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "hydia_eval_square_no_relin": (i32, [vp, vp, u32, pp]),
        "hydia_ct_limb_prefix": (i32, [vp, vp, u32, pp]),
        "hydia_blind_db_num_cts": (sz, [vp, sz, sz]),
        "hydia_blind_db_enroll": (i32, [vp, vp, sz, sz, vp]),
        "hydia_blind_encrypt_query": (i32, [vp, vp, sz, vp, u64, pp]),
        "hydia_blind_compute_similarity": (i32, [vp, vp, pp]),
        "hydia_blind_index_scenario": (i32, [vp, vp, pp]),
        "hydia_blind_membership_scenario": (i32, [vp, vp, pp]),
        "hydia_compress_ciphers": (i32, [vp, vp, sz, pp]),
        "hydia_blind_decrypt_index": (i32, [vp, vp, sz, vp, sz, C.POINTER(sz)]),
        "hydia_eval_dot_no_relin": (i32, [vp, vp, vp, pp]),
        "hydia_kernel_time": (i32, [vp, C.c_char_p, C.POINTER(dbl), C.POINTER(u64)]),
        "hydia_kernel_time_reset": (i32, [vp]),
        "hydia_byte_ledger": (i32, [i32, C.c_char_p, sz, C.POINTER(sz)]),
        "hydia_db_residue_bits": (i32, [vp]),
        "hydia_bench_ntt": (i32, [vp, u32, u32, u32, i32, u32, C.POINTER(dbl)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    L._hydia_symbols = sorted(sig)
    _LIB = L
    return L


BLIND_CHUNK_LEN = 128  # CHUNK_LEN, include/config.h:34 (HYDIA_BLIND_CHUNK_LEN)


def _chk(code):
    if code != 0:
        raise HydiaError(code, load_library().hydia_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _seed(x):
    """32-byte sampler key.  None = fresh OS entropy (what every role method defaults to: the reference seeds OpenFHE's PRNG
    from the OS); an int or 32 bytes = a reproducible key for tests — a (seed, nonce) pair must never encrypt two plaintexts."""
    if x is None:
        return np.frombuffer(os.urandom(32), dtype=np.uint8).copy()
    if isinstance(x, (bytes, bytearray)):
        b = bytes(x)
        assert len(b) == 32
    else:
        b = int(x).to_bytes(32, "little")
    return np.frombuffer(b, dtype=np.uint8).copy()


def _is_device_tensor(x):
    """a tensor in device memory, by duck typing: torch is not imported unless the caller already hands one in"""
    return all(hasattr(x, a) for a in ("data_ptr", "is_cuda", "dtype", "stride"))


_DTYPES = {"torch.float64": 0, "torch.float32": 1, "torch.float16": 2, "torch.bfloat16": 3}  # hydia_dtype


def _dev_rows(cc, t):
    """hydia_dev_rows of a 2-D tensor (1-D: one row) of f64 / f32 / f16 / bf16 on the context's GPU whose last dimension has stride 1;
    the producer stream is torch's current stream of the tensor's device.  The tensor is only read.  That the memory lies on the
    context's GPU is checked by the library (HydiaError(-1))."""
    import torch
    if t.dim() == 1:
        t = t[None]
    code = _DTYPES.get(str(t.dtype))
    if not t.is_cuda or code is None or t.dim() != 2 or t.shape[1] != cc.dim or (t.shape[1] > 1 and t.stride(1) != 1):
        raise HydiaError(-1, "hydia: device rows are a tensor [n][vector_dim] of float64 / float32 / float16 / bfloat16 in device "
                             "memory whose last dimension has stride 1")
    n = t.shape[0]
    stream = torch.cuda.current_stream(t.device)
    handle = stream.cuda_stream or None
    if handle is None:
        stream.synchronize()  # the null stream: nothing to record an event on that the context's non-blocking stream would wait for
    return _DevRows(t.data_ptr() or None, code, n, t.stride(0) if n > 1 else cc.dim, handle)


def byte_ledger(enable=-1):
    """Read the process-wide byte ledger {kernel: (launches, bytes)}, then apply `enable` (1 restart, 0 stop, -1 keep)."""
    L = load_library()
    buf = C.create_string_buffer(1 << 16)
    need = C.c_size_t()
    _chk(L.hydia_byte_ledger(enable, buf, len(buf), C.byref(need)))
    out = {}
    for line in buf.value.decode().splitlines():
        k, n, b = line.split("\t")
        out[k] = (int(n), float(b))
    return out


def default_params(**over):
    p = _Params()
    load_library().hydia_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def compute_required_depth(approach):
    """OpenFHEWrapper::computeRequiredDepth (src/openFHE_wrapper.cpp:6-44)."""
    return int(load_library().hydia_compute_required_depth(approach))


def params_for_approach(approach):
    """Host-only: the context ./ImageMatching <file> <approach> needs — depth computeRequiredDepth(approach), the smallest ring whose
    log2(QP) fits HEStd_128_classic (log_n 15 for approaches 4 and 5, 16 for approach 1; include/hydia.h)."""
    p = _Params()
    _chk(load_library().hydia_params_for_approach(approach, C.byref(p)))
    return p


def base_rotations(slots):
    """Host-only: the rotation keys approach 1 needs on a ring of `slots` slots, {2^k} u {slots - 2^k} (hydia_base_rotations)."""
    L = load_library()
    n = C.c_size_t()
    _chk(L.hydia_base_rotations(slots, None, 0, C.byref(n)))
    out = np.zeros(n.value, dtype=np.int32)
    _chk(L.hydia_base_rotations(slots, _p(out), n.value, C.byref(n)))
    return [int(r) for r in out]


def grote_row_length(slots):
    """Host-only: approach 2's row length 2^ceil(log2(slots) / 2) (hydia_grote_row_length)."""
    r = int(load_library().hydia_grote_row_length(slots))
    if r == 0:
        raise HydiaError(-1, "hydia: slots must be a power of two >= 2")
    return r


def describe_params(params=None):
    """Host-only: (info dict, moduli, roots) of a parameter set — works without a GPU."""
    L = load_library()
    p = params or default_params()
    info = _Info()
    mod = np.zeros(64, dtype=np.uint64)
    roots = np.zeros(64, dtype=np.uint64)
    _chk(L.hydia_params_describe(C.byref(p), C.byref(info), _p(mod), _p(roots)))
    nt = info.n_q + info.n_p
    d = {k: getattr(info, k) for k, _ in _Info._fields_}
    return d, mod[:nt].copy(), roots[:nt].copy()


def wire_peek(message):
    """Host-only (hydia_wire_peek): the context-free validation of a wire message and what its header says — a dict of type, log_n,
    count, n_polys, n_limbs, rot, scale, a_seed (32 bytes), nonce0, header_bytes, payload_bytes.  A malformed message: HydiaError(-1)
    naming the field."""
    raw = np.frombuffer(bytes(message), dtype=np.uint8)
    info = _WireInfo()
    _chk(load_library().hydia_wire_peek(_p(raw) if raw.size else None, raw.size, C.byref(info)))
    d = {k: getattr(info, k) for k, _ in _WireInfo._fields_}
    d["a_seed"] = bytes(info.a_seed)
    return d


def _delta_peek(message, peek):
    raw = np.frombuffer(bytes(message), dtype=np.uint8)
    info = _DeltaInfo()
    _chk(peek(_p(raw) if raw.size else None, raw.size, C.byref(info)))
    return {k: int(getattr(info, k)) for k, _ in _DeltaInfo._fields_}


def db_delta_peek(message):
    """Host-only (hydia_db_delta_peek): the context-free validation of a database delta and what its header says — a dict of version,
    vector_dim, babies, first_vector, n_rows, first_block, n_blocks, total_bytes.  A malformed delta: HydiaError(-1) naming the field."""
    return _delta_peek(message, load_library().hydia_db_delta_peek)


def db_delta_seeded_peek(message):
    """Host-only (hydia_db_delta_seeded_peek): db_delta_peek for a SEEDED database delta (magic HYDDELS1, type 2 messages); the same
    dict.  A malformed delta, an unseeded one included: HydiaError(-1) naming the field."""
    return _delta_peek(message, load_library().hydia_db_delta_seeded_peek)


def _public_seed(x):
    """a PUBLIC expansion seed: None = a fresh hydia_random_seed, otherwise as _seed"""
    if x is not None:
        return _seed(x)
    out = np.zeros(32, dtype=np.uint8)
    _chk(load_library().hydia_random_seed(_p(out)))
    return out


def _wire_out(call):
    """call(buf, cap, written) -> bytes: the size first (a NULL buffer answers HYDIA_ERR_ARG with the need), then the message"""
    n = C.c_size_t()
    code = call(None, 0, C.byref(n))
    if code != 0 and n.value == 0:
        _chk(code)
    if n.value == 0:
        return b""
    buf = np.empty(n.value, dtype=np.uint8)
    _chk(call(_p(buf), buf.size, C.byref(n)))
    return buf[:n.value].tobytes()


class Ciphertext:
    """Handle of a batch of ciphertexts resident in HBM (Ciphertext<DCRTPoly> / vector<Ciphertext<DCRTPoly>>)."""

    def to_wire(self):
        """the batch as one wire message (hydia_ct_to_wire): packed on the GPU, residues in the bit length of their modulus"""
        return _wire_out(lambda buf, cap, n: self.cc.L.hydia_ct_to_wire(self.cc.h, self.h, buf, cap, n))

    def __init__(self, cc, h):
        self.cc, self.h = cc, h

    def __del__(self):
        # a handle pins its context inside the library (hydia_ctx_destroy defers until the last handle is gone), so it can
        # always be released, also after Context.close()
        if getattr(self, "h", None):
            self.cc.L.hydia_ct_free(self.h)
            self.h = None

    def shape(self):
        c, p, l, s = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double()
        _chk(self.cc.L.hydia_ct_shape(self.h, C.byref(c), C.byref(p), C.byref(l), C.byref(s)))
        return c.value, p.value, l.value, s.value

    def __len__(self):
        return self.shape()[0]

    size = __len__

    def export(self):
        c, p, l, _ = self.shape()
        out = np.zeros((c, p, l, self.cc.N), dtype=np.uint64)
        _chk(self.cc.L.hydia_ct_export(self.cc.h, self.h, _p(out)))
        return out

    def copy_to_device(self, dev_ptr):
        _chk(self.cc.L.hydia_ct_copy_to_device(self.cc.h, self.h, C.c_void_p(dev_ptr)))

    def device_ptr(self):
        ptr, n = C.c_void_p(), C.c_size_t()
        _chk(self.cc.L.hydia_ct_device_ptr(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value


class Plaintext:
    """Handle of a plain query (include/hydia.h, hydia_pt): ONE encoded polynomial [n_q][N] resident in HBM — a probe the sender
    knows.  A type of its own: the ciphertext methods do not take it."""

    def __init__(self, cc, h):
        self.cc, self.h = cc, h

    def __del__(self):
        if getattr(self, "h", None):  # pins its context inside the library like a Ciphertext
            self.cc.L.hydia_pt_free(self.h)
            self.h = None

    def export(self):
        out = np.zeros((self.cc.nQ, self.cc.N), dtype=np.uint64)
        _chk(self.cc.L.hydia_pt_export(self.cc.h, self.h, _p(out)))
        return out


class Context:
    """CKKS context + keys + resident database on one GPU (replaces CryptoContext<DCRTPoly>, src/main.cpp:169-206)."""

    def __init__(self, params=None, device=0, moduli=None, roots=None, n_p=None):
        """moduli (optional): a caller-supplied prime chain, n_q ciphertext primes then n_p special primes, with optional
        2N-th roots — the OpenFHE-adapter path (hydia_ctx_create_custom)."""
        self.L = load_library()
        self.params = params or default_params()
        h = C.c_void_p()
        if moduli is None:
            _chk(self.L.hydia_ctx_create(C.byref(self.params), device, C.byref(h)))
        else:
            moduli = np.ascontiguousarray(moduli, dtype=np.uint64)
            roots = None if roots is None else np.ascontiguousarray(roots, dtype=np.uint64)
            _chk(self.L.hydia_ctx_create_custom(C.byref(self.params), _p(moduli), None if roots is None else _p(roots),
                                                len(moduli) - n_p, n_p, device, C.byref(h)))
        self.h = h
        self.owned = True
        self.device = device
        self._read_info()

    def _read_info(self):
        info = _Info()
        _chk(self.L.hydia_get_info(self.h, C.byref(info)))
        self.info = info
        self.N, self.slots, self.nQ, self.nP, self.dnum, self.dim = info.n, info.slots, info.n_q, info.n_p, info.dnum, info.vector_dim
        self.nT = self.nQ + self.nP
        self.delta = info.delta
        self.moduli = np.zeros(self.nT, dtype=np.uint64)
        self.roots = np.zeros(self.nT, dtype=np.uint64)
        _chk(self.L.hydia_get_moduli(self.h, _p(self.moduli), _p(self.roots)))

    @classmethod
    def _borrowed(cls, L, params, h):
        """A view of a context owned by a shard group (never destroyed through this object)."""
        self = cls.__new__(cls)
        self.L, self.params, self.h, self.owned, self.device = L, params, C.c_void_p(h), False, None
        self._read_info()
        return self

    def close(self):
        if self.h and getattr(self, "owned", True):
            self.L.hydia_ctx_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _chk(self.L.hydia_sync(self.h))

    # ---- keys
    def keygen(self, seed=None):
        _chk(self.L.hydia_keygen(self.h, _p(_seed(seed))))

    def keygen_rotations(self, rotations, seed=None):
        """keygen with rotation keys for exactly `rotations` (each taken mod slots; include/hydia.h hydia_keygen_rotations)."""
        rots = np.ascontiguousarray(list(rotations), dtype=np.int32)
        _chk(self.L.hydia_keygen_rotations(self.h, _p(_seed(seed)), _p(rots) if rots.size else None, rots.size))

    # ---- seeded keys (include/hydia.h): the uniform halves are the expansion of the PUBLIC a_seed; only the b halves travel
    def keygen_seeded(self, seed=None, a_seed=None):
        """hydia_keygen_seeded: keygen(seed) with every uniform half under the public `a_seed` (None: fresh OS entropy; read it back
        with key_seed()).  a_seed == seed is refused (HydiaError -1)."""
        _chk(self.L.hydia_keygen_seeded(self.h, _p(_seed(seed)), _p(_seed(a_seed))))

    def keygen_rotations_seeded(self, rotations, seed=None, a_seed=None):
        rots = np.ascontiguousarray(list(rotations), dtype=np.int32)
        _chk(self.L.hydia_keygen_rotations_seeded(self.h, _p(_seed(seed)), _p(_seed(a_seed)), _p(rots) if rots.size else None, rots.size))

    def key_seed(self):
        """the 32 bytes of the public seed the context's seeded keys were made under (HydiaError -2 when there is none)"""
        out = np.zeros(32, dtype=np.uint8)
        _chk(self.L.hydia_get_key_seed(self.h, _p(out)))
        return out.tobytes()

    def export_eval_key_seeded(self, rot):
        """the b halves [dnum][n_q+n_p][N] of a key key_seed() covers (HydiaError -2 for any other key)"""
        out = np.zeros((self.dnum, self.nT, self.N), dtype=np.uint64)
        assert out.size == self.L.hydia_eval_key_seeded_words(self.h)
        _chk(self.L.hydia_export_eval_key_seeded(self.h, rot, _p(out)))
        return out

    def import_eval_key_seeded(self, rot, b, a_seed):
        b = np.ascontiguousarray(b, dtype=np.uint64)
        assert b.size == self.dnum * self.nT * self.N
        _chk(self.L.hydia_import_eval_key_seeded(self.h, rot, _p(b), _p(_seed(a_seed))))

    def export_public_key_seeded(self):
        out = np.zeros((self.nQ, self.N), dtype=np.uint64)
        _chk(self.L.hydia_export_public_key_seeded(self.h, _p(out)))
        return out

    def import_public_key_seeded(self, b, a_seed):
        b = np.ascontiguousarray(b, dtype=np.uint64)
        assert b.size == self.nQ * self.N
        _chk(self.L.hydia_import_public_key_seeded(self.h, _p(b), _p(_seed(a_seed))))

    def import_eval_key(self, rot, data):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.size == self.dnum * 2 * self.nT * self.N
        _chk(self.L.hydia_import_eval_key(self.h, rot, _p(data)))

    def export_eval_key(self, rot):
        out = np.zeros((self.dnum, 2, self.nT, self.N), dtype=np.uint64)
        _chk(self.L.hydia_export_eval_key(self.h, rot, _p(out)))
        return out

    def import_public_key(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.size == 2 * self.nQ * self.N
        _chk(self.L.hydia_import_public_key(self.h, _p(data)))

    def import_secret_key(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.size == self.nT * self.N
        _chk(self.L.hydia_import_secret_key(self.h, _p(data)))

    def export_public_key(self):
        out = np.zeros((2, self.nQ, self.N), dtype=np.uint64)
        _chk(self.L.hydia_export_public_key(self.h, _p(out)))
        return out

    def export_secret_key(self):
        out = np.zeros((self.nT, self.N), dtype=np.uint64)
        _chk(self.L.hydia_export_secret_key(self.h, _p(out)))
        return out

    def keygen_switch(self, old_secret, seed=None):
        """hydia_keygen_switch, on the NEW receiver's context: the switching key [dnum][2][n_q+n_p][N] from `old_secret` (the old
        receiver's export_secret_key()) to this context's secret — what Context.db_rekey on the sender takes.  Treat it like an
        evaluation key; seed=None draws a fresh one from the OS (use a fresh seed per switching key: include/hydia.h)."""
        if old_secret is not None:
            old_secret = np.ascontiguousarray(old_secret, dtype=np.uint64)
            assert old_secret.size == self.nT * self.N
        out = np.zeros((self.dnum, 2, self.nT, self.N), dtype=np.uint64)
        assert out.size == self.L.hydia_switch_key_words(self.h)
        _chk(self.L.hydia_keygen_switch(self.h, None if old_secret is None else _p(old_secret), _p(_seed(seed)), _p(out)))
        return out

    def fill_eval_keys_random(self, seed=1):
        _chk(self.L.hydia_fill_eval_keys_random(self.h, seed))

    def has_eval_key(self, rot):
        return bool(self.L.hydia_has_eval_key(self.h, rot))

    # ---- wire messages (include/hydia.h): packed, range-checked, self-describing; the checked path for data from outside
    def ct_from_wire(self, message):
        """a type 1 message -> ONE Ciphertext batch; a type 2 message (seeded queries) -> a list of single-ciphertext handles, exactly
        those hydia_ct_expand_seeded makes.  A malformed or non-canonical message: HydiaError(-1), nothing stays allocated."""
        raw = np.frombuffer(bytes(message), dtype=np.uint8)
        info = wire_peek(message)
        cap = 1 if info["type"] == 1 else info["count"]
        out = (C.c_void_p * cap)()
        n = C.c_size_t()
        _chk(self.L.hydia_ct_from_wire(self.h, _p(raw), raw.size, out, cap, C.byref(n)))
        cts = [Ciphertext(self, C.c_void_p(out[i])) for i in range(n.value)]
        return cts[0] if info["type"] == 1 else cts

    def key_to_wire(self, rot, seeded=False):
        """key `rot` (-1: the public key, 0: relinearisation, r: rotation r) as one wire message; seeded: the b halves and the context's
        public key seed (HydiaError(-2) for a key hydia_keygen_seeded did not make)"""
        return _wire_out(lambda buf, cap, n: self.L.hydia_key_to_wire(self.h, rot, int(bool(seeded)), buf, cap, n))

    def key_from_wire(self, message):
        """installs the key a message carries after its residues passed the range check; returns its id (-1: the public key)"""
        raw = np.frombuffer(bytes(message), dtype=np.uint8)
        rot = C.c_int()
        _chk(self.L.hydia_key_from_wire(self.h, _p(raw) if raw.size else None, raw.size, C.byref(rot)))
        return rot.value

    def keys_save(self, path, seeded=False):
        """the public key and every evaluation key the context holds as a key-set file of wire messages"""
        _chk(self.L.hydia_keys_save(self.h, os.fsencode(path), int(bool(seeded))))

    def keys_load(self, path):
        """NOT transactional: a refused file (HydiaError(-1) naming the message) leaves the keys of earlier messages installed"""
        _chk(self.L.hydia_keys_load(self.h, os.fsencode(path)))

    def wire_ct_bytes(self, count, n_polys, n_limbs, seeded=False):
        return int(self.L.hydia_wire_ct_bytes(self.h, count, n_polys, n_limbs, int(bool(seeded))))

    def wire_eval_key_bytes(self, seeded=False):
        return int(self.L.hydia_wire_eval_key_bytes(self.h, int(bool(seeded))))

    def wire_public_key_bytes(self, seeded=False):
        return int(self.L.hydia_wire_public_key_bytes(self.h, int(bool(seeded))))

    # ---- ciphertexts
    def import_ct(self, data, scale):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        if data.ndim == 3:
            data = data[None]
        c, p, l, n = data.shape
        assert n == self.N
        h = C.c_void_p()
        _chk(self.L.hydia_ct_import(self.h, _p(data), c, p, l, scale, C.byref(h)))
        return Ciphertext(self, h)

    def ct_from_device(self, ptr, count, n_polys, n_limbs, scale):
        h = C.c_void_p()
        _chk(self.L.hydia_ct_from_device(self.h, C.c_void_p(ptr), count, n_polys, n_limbs, scale, C.byref(h)))
        return Ciphertext(self, h)

    def ct_view_device(self, ptr, count, n_polys, n_limbs, scale, keepalive=None):
        """A handle over ciphertexts that stay in the caller's device memory (no copy).  `keepalive` (e.g. the torch tensor that owns
        the memory) is referenced by the handle."""
        h = C.c_void_p()
        _chk(self.L.hydia_ct_view_device(self.h, C.c_void_p(ptr), count, n_polys, n_limbs, scale, C.byref(h)))
        ct = Ciphertext(self, h)
        ct._keepalive = keepalive
        return ct

    def ct_limb_prefix(self, ct, n_limbs):
        """A handle over the first n_limbs limbs of ct, read in place (no copy, ct's limb stride); it keeps ct alive."""
        v = self._out(self.L.hydia_ct_limb_prefix, ct.h, int(n_limbs))
        v._keepalive = ct
        return v

    def _out(self, fn, *args):
        h = C.c_void_p()
        _chk(fn(self.h, *args, C.byref(h)))
        return Ciphertext(self, h)

    def pt_import(self, data, scale=None):
        """a plain query from its residues [n_q][N] (canonical, evaluation form); scale defaults to 2^scale_bits"""
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.size == self.nQ * self.N
        h = C.c_void_p()
        _chk(self.L.hydia_pt_import(self.h, _p(data), float(self.delta if scale is None else scale), C.byref(h)))
        return Plaintext(self, h)

    def encrypt(self, slots, seed=None, nonce0=0):
        slots = np.ascontiguousarray(slots, dtype=np.float64)
        if slots.ndim == 1:
            slots = slots[None]
        assert slots.shape[1] == self.slots
        return self._out(self.L.hydia_encrypt, _p(slots), slots.shape[0], _p(_seed(seed)), nonce0)

    def decrypt(self, ct):
        out = np.zeros((len(ct), self.slots), dtype=np.float64)
        _chk(self.L.hydia_decrypt(self.h, ct.h, _p(out)))
        return out

    # ---- candidate lists and matches (include/hydia.h): the decoded slots stay on the GPU, only what was asked for comes back
    def decrypt_device(self, ct):
        """hydia_decrypt_device: the slots of decrypt(ct), bit for bit, as a float64 tensor [count, slots] on the context's GPU.
        (A process that uses torch beside this library imports torch before it creates a context.)"""
        import torch
        if self.device is None:
            raise HydiaError(-2, "hydia: decrypt_device is not served on a shard of a group")
        out = torch.empty((len(ct), self.slots), dtype=torch.float64, device="cuda:%d" % self.device)
        _chk(self.L.hydia_decrypt_device(self.h, ct.h, C.c_void_p(out.data_ptr() or None)))
        return out

    def _dev_values(self, values):
        """(pointer, n) of a contiguous float64 tensor, after torch's current stream has finished with it; that the memory lies on
        the context's GPU is checked by the library (HydiaError(-1))"""
        import torch
        if not _is_device_tensor(values) or str(values.dtype) != "torch.float64" or not values.is_contiguous():
            raise HydiaError(-1, "hydia: the values are a contiguous float64 tensor in the memory of the context's GPU")
        if values.is_cuda:
            torch.cuda.current_stream(values.device).synchronize()
        return C.c_void_p(values.data_ptr() or None), values.numel()

    def slots_select(self, values, threshold, cap=None):
        """hydia_slots_select_device: (idx, val, total) — the indices i with values[i] >= threshold ascending (at most cap of them,
        default all), their values, and how many there are"""
        ptr, n = self._dev_values(values)
        cap = n if cap is None else int(cap)
        idx, val, total = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.float64), C.c_size_t()
        _chk(self.L.hydia_slots_select_device(self.h, ptr, n, float(threshold), _p(idx) if cap else None, _p(val) if cap else None, cap,
                                              C.byref(total)))
        w = min(cap, total.value)
        return idx[:w].astype(np.int64), val[:w], total.value

    def slots_topk(self, values, k):
        """hydia_slots_topk_device: (idx, val) — the min(k, n) largest by value descending, ties by ascending index, NaN last"""
        ptr, n = self._dev_values(values)
        k = int(k)
        room = max(1, min(k, n))
        idx, val, got = np.zeros(room, dtype=np.uint64), np.zeros(room, dtype=np.float64), C.c_size_t()
        _chk(self.L.hydia_slots_topk_device(self.h, ptr, n, k, _p(idx), _p(val), C.byref(got)))
        return idx[:got.value].astype(np.int64), val[:got.value]

    # ---- primitives
    def ntt(self, data, modulus_index, inverse=False):
        a = np.ascontiguousarray(data, dtype=np.uint64).copy()
        a2 = a.reshape(-1, self.N)
        _chk(self.L.hydia_ntt(self.h, _p(a2), a2.shape[0], modulus_index, int(inverse)))
        return a

    @property
    def ntt_engine(self):
        """15 or 16: the ring whose specialised two-pass transform the plain transforms run on; 0: the ring-size-generic kernels
        (another ring, HYDIA_NTT_GENERIC=1, or N = 2^16 without HYDIA_NTT16=1 when the context was created)."""
        return int(self.L.hydia_ntt_engine(self.h))

    def eval_rotate(self, ct, rot):
        return self._out(self.L.hydia_eval_rotate, ct.h, rot)

    def eval_mult(self, a, b):
        return self._out(self.L.hydia_eval_mult, a.h, b.h)

    def eval_mult_no_relin(self, a, b):
        return self._out(self.L.hydia_eval_mult_no_relin, a.h, b.h)

    def relinearize(self, ct):
        _chk(self.L.hydia_relinearize(self.h, ct.h))

    def rescale(self, ct):
        _chk(self.L.hydia_rescale(self.h, ct.h))

    def eval_add(self, a, b):
        _chk(self.L.hydia_eval_add(self.h, a.h, b.h))

    def level_reduce(self, ct, n_limbs):
        _chk(self.L.hydia_level_reduce(self.h, ct.h, n_limbs))

    def eval_mult_plain(self, ct, slots):
        """EvalMult(ct, MakeCKKSPackedPlaintext(slots)) + RescaleInPlace on every ciphertext of the batch."""
        v = np.ascontiguousarray(slots, dtype=np.float64)
        assert v.shape == (self.slots,)
        return self._out(self.L.hydia_eval_mult_plain, ct.h, _p(v))

    def binary_rotate(self, ct, factor):
        """OpenFHEWrapper::binaryRotate (src/openFHE_wrapper.cpp:103-128)."""
        return self._out(self.L.hydia_binary_rotate, ct.h, int(factor))

    def merge_ciphers(self, ct, dimension):
        """OpenFHEWrapper::mergeCiphers (src/openFHE_wrapper.cpp:191-218) on a batch: every dimension-th slot, packed in order."""
        return self._out(self.L.hydia_merge_ciphers, ct.h, int(dimension))

    def alpha_norm_rows(self, ct, alpha, row_length):
        """HersSender::alphaNormRows (src/sender/sender_hers.cpp:118-132) on a batch."""
        return self._out(self.L.hydia_alpha_norm_rows, ct.h, int(alpha), int(row_length))

    def alpha_norm_columns(self, ct, alpha, row_length):
        """HersSender::alphaNormColumns (src/sender/sender_hers.cpp:136-178) on a batch."""
        return self._out(self.L.hydia_alpha_norm_columns, ct.h, int(alpha), int(row_length))

    def grote_row_length(self):
        """approach 2's row length for this context's slot count"""
        return grote_row_length(self.slots)

    def eval_square_no_relin(self, ct, n_limbs=0):
        """(c0^2, 2 c0 c1, c1^2) on the first n_limbs limbs of ct read in place (0 = all)"""
        return self._out(self.L.hydia_eval_square_no_relin, ct.h, int(n_limbs))

    def compress_ciphers(self, ct, dimension):
        """OpenFHEWrapper::compressCiphers (src/openFHE_wrapper.cpp:273-312) on a batch: the slots = 0 mod dimension of `dimension`
        ciphertexts interleaved into one."""
        return self._out(self.L.hydia_compress_ciphers, ct.h, int(dimension))

    def eval_dot_no_relin(self, q, b):
        """sum_c q[c] (x) b[m K + c] without relinearisation: q a batch of K ciphertexts, b of M K -> M 3-component ciphertexts"""
        return self._out(self.L.hydia_eval_dot_no_relin, q.h, b.h)

    def blind_db_num_cts(self, n, chunk_len=BLIND_CHUNK_LEN):
        return int(self.L.hydia_blind_db_num_cts(self.h, n, chunk_len))

    def base_rotations(self):
        """the key set of approach 1 for this context's slot count (pass it to keygen_rotations)"""
        return base_rotations(self.slots)

    def base_db_num_cts(self, n):
        return int(self.L.hydia_base_db_num_cts(self.h, n))

    def chebyshev_compare(self, ct, delta=0.44, depth=10):
        """OpenFHEWrapper::chebyshevCompare (src/openFHE_wrapper.cpp:143-185)."""
        return self._out(self.L.hydia_chebyshev_compare, ct.h, delta, depth)

    def sum_and_evalsum(self, ct):
        return self._out(self.L.hydia_sum_and_evalsum, ct.h)

    def add_many(self, ct):
        """EvalAddManyInPlace (sender_diag.cpp:46): the batch summed into one ciphertext."""
        return self._out(self.L.hydia_add_many, ct.h)

    def eval_sum(self, ct):
        """EvalSum(ct, batchSize) (sender_diag.cpp:47)."""
        return self._out(self.L.hydia_eval_sum, ct.h)

    def ct_add_raw(self, acc, dev_ptr, src_device=-1):
        _chk(self.L.hydia_ct_add_raw(self.h, acc.h, C.c_void_p(dev_ptr), src_device))

    def ct_mod_reduce(self, ct):
        _chk(self.L.hydia_ct_mod_reduce(self.h, ct.h))

    # ---- database
    def db_num_cts(self, n):
        return int(self.L.hydia_db_num_cts(self.h, n))

    def db_alloc(self, n):
        _chk(self.L.hydia_db_alloc(self.h, n))

    def db_import_ct(self, t, data):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.size == 2 * self.nQ * self.N
        _chk(self.L.hydia_db_import_ct(self.h, t, _p(data)))

    def db_export_ct(self, t):
        out = np.zeros((2, self.nQ, self.N), dtype=np.uint64)
        _chk(self.L.hydia_db_export_ct(self.h, t, _p(out)))
        return out

    # ---- plain gallery (kinds 7 / 8, include/hydia.h): unencrypted templates, one encoded polynomial [n_q][N] per diagonal
    def plain_db_alloc(self, n, babies=None):
        """room for n vectors in a declared form: babies = vector_dim (hoisted, the default) or a power of two >= 2 dividing it"""
        _chk(self.L.hydia_plain_db_alloc(self.h, n, self.dim if babies is None else int(babies)))

    def plain_db_import_pt(self, t, data):
        data = np.ascontiguousarray(data, dtype=np.uint64)
        assert data.size == self.nQ * self.N
        _chk(self.L.hydia_plain_db_import_pt(self.h, t, _p(data)))

    def plain_db_export_pt(self, t):
        out = np.zeros((self.nQ, self.N), dtype=np.uint64)
        _chk(self.L.hydia_plain_db_export_pt(self.h, t, _p(out)))
        return out

    def plain_db_update(self, first_vector, rows, normalise=True):
        """hydia_plain_db_update: add the ENCODED sparse image of `rows` (k x vector_dim float64, normalised IN PLACE when `normalise`),
        placed at vectors first_vector .., to the resident plain gallery — db_update without a seed.  Append: first_vector =
        db_stats()[0]; remove: the negated template (the same rows negated restore an existing block bit for bit); replace:
        new_normalised - old_normalised with normalise=False."""
        assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.ndim == 2 and rows.shape[1] == self.dim
        _chk(self.L.hydia_plain_db_update(self.h, first_vector, _p(rows), rows.shape[0], 1 if normalise else 0))

    def plain_db_save(self, path):
        """write the resident plain gallery to `path` (db_save's format, one polynomial per entry)"""
        _chk(self.L.hydia_plain_db_save(self.h, str(path).encode()))

    def plain_db_load(self, path):
        """load a plain gallery file; every residue is checked on the device, and a bad one leaves no database resident"""
        _chk(self.L.hydia_plain_db_load(self.h, str(path).encode()))

    def db_update(self, first_vector, rows, normalise=True, seed=None, first_block=0):
        """hydia_db_update[_shard]: add a FRESH encryption of `rows` (k x vector_dim float64, normalised IN PLACE when `normalise`),
        placed at vectors first_vector .., to the resident kind-5 / kind-6 database.  Append: first_vector = db_stats()[0]; remove:
        the negated template; replace: new_normalised - old_normalised with normalise=False.  seed=None draws a fresh key from the OS
        — a seed must NEVER be used twice on one database (include/hydia.h)."""
        assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.ndim == 2 and rows.shape[1] == self.dim
        _chk(self.L.hydia_db_update_shard(self.h, first_vector, _p(rows), rows.shape[0], 1 if normalise else 0, _p(_seed(seed)), first_block))

    # ---- database deltas and seeded database deltas (include/hydia.h): the enroller's context makes the message, the sender's applies
    # it.  Seeded: the maker holds the SECRET key; only the c0 halves travel
    def _delta_bytes(self, entry, first_vector, n):
        b = C.c_size_t()
        _chk(entry(self.h, first_vector, n, C.byref(b)))
        return b.value

    def _delta_make(self, host_entry, device_entry, first_vector, rows, normalise, seeds, babies, first_block):
        """seeds: the seed arrays the entries take — ONE set for the sizing call and the making call"""
        B = self.dim if babies is None else int(babies)
        if _is_device_tensor(rows):
            d = _dev_rows(self, rows)
            call, src = device_entry, (C.byref(d),)
        else:
            assert rows.dtype == np.float64 and rows.flags.c_contiguous and rows.ndim == 2 and rows.shape[1] == self.dim
            call, src = host_entry, (_p(rows), rows.shape[0])
        sp = [_p(x) for x in seeds]
        return _wire_out(lambda buf, cap, n: call(self.h, first_vector, *src, 1 if normalise else 0, *sp, B, first_block, buf, cap, n))

    def _delta_apply(self, entry, message):
        raw = np.frombuffer(bytes(message), dtype=np.uint8)
        _chk(entry(self.h, _p(raw) if raw.size else None, raw.size))

    def db_delta_bytes(self, first_vector, n):
        """the size of the delta of rows first_vector .. first_vector + n - 1 on this context (host arithmetic only)"""
        return self._delta_bytes(self.L.hydia_db_delta_bytes, first_vector, n)

    def db_delta_peek(self, message):
        """the module's db_delta_peek (context-free, host only)"""
        return db_delta_peek(message)

    def db_delta_make(self, first_vector, rows, normalise=True, seed=None, babies=None, first_block=0):
        """hydia_db_delta_make[_device]: the FRESH encryption of `rows` (k x vector_dim float64, normalised IN PLACE when `normalise`; or
        a tensor on the context's GPU, never written) that db_update would add at vectors first_vector .., as one message (bytes) for
        the db_delta_apply of the context that holds the database.  Needs the public key alone.  babies: the form of the TARGET
        database (None = vector_dim, hoisted).  seed=None draws a fresh key from the OS — a seed must NEVER be used twice on one
        database (include/hydia.h)."""
        return self._delta_make(self.L.hydia_db_delta_make, self.L.hydia_db_delta_make_device, first_vector, rows, normalise, [_seed(seed)],
                                babies, first_block)

    def db_delta_apply(self, message):
        """hydia_db_delta_apply: add the delta's ciphertexts to the resident kind-5 / kind-6 database (bit for bit what db_update with
        the maker's arguments leaves), or enrol from it when nothing is resident and it starts at vector 0.  Every header and residue
        is checked first: a refused delta (HydiaError) changes nothing."""
        self._delta_apply(self.L.hydia_db_delta_apply, message)

    def db_delta_seeded_bytes(self, first_vector, n):
        """the size of the seeded delta of rows first_vector .. first_vector + n - 1 on this context (host arithmetic only)"""
        return self._delta_bytes(self.L.hydia_db_delta_seeded_bytes, first_vector, n)

    def db_delta_seeded_peek(self, message):
        """the module's db_delta_seeded_peek (context-free, host only)"""
        return db_delta_seeded_peek(message)

    def db_delta_make_seeded(self, first_vector, rows, normalise=True, seed=None, a_seed=None, babies=None, first_block=0):
        """hydia_db_delta_make_seeded[_device]: db_delta_make on a context that holds the SECRET key — the c0 halves alone, half the
        bytes, for db_delta_apply_seeded.  seed (secret, the noise) as in db_delta_make; a_seed (PUBLIC, travels in the message):
        None = a fresh hydia_random_seed — it must never have served a query under this key or another delta on that database, and
        must differ from seed (include/hydia.h)."""
        return self._delta_make(self.L.hydia_db_delta_make_seeded, self.L.hydia_db_delta_make_seeded_device, first_vector, rows, normalise,
                                [_seed(seed), _public_seed(a_seed)], babies, first_block)

    def db_delta_apply_seeded(self, message):
        """hydia_db_delta_apply_seeded: db_delta_apply for a seeded delta — c0 from the message, a regenerated on the GPU straight into
        the resident layout.  Needs no key.  Every header and c0 residue is checked first: a refused delta (HydiaError) changes nothing."""
        self._delta_apply(self.L.hydia_db_delta_apply_seeded, message)

    # ---- templates already in device memory (include/hydia.h, hydia_dev_rows): `rows` is a tensor on this context's GPU, only read
    def rows_widen_device(self, rows, normalise=True):
        """hydia_rows_widen_device: the rows widened exactly to float64 (and divided by their L2 norm), as a new tensor [n][vector_dim]"""
        import torch
        d = _dev_rows(self, rows)
        out = torch.empty((d.n, self.dim), dtype=torch.float64, device=rows.device)
        _chk(self.L.hydia_rows_widen_device(self.h, C.byref(d), 1 if normalise else 0, C.c_void_p(out.data_ptr() or None)))
        return out

    def db_update_device(self, first_vector, rows, normalise=True, seed=None):
        """db_update from rows in device memory (normalised on the device, never written)"""
        d = _dev_rows(self, rows)
        _chk(self.L.hydia_db_update_device(self.h, first_vector, C.byref(d), 1 if normalise else 0, _p(_seed(seed))))

    def plain_db_update_device(self, first_vector, rows, normalise=True):
        """plain_db_update from rows in device memory (normalised on the device, never written)"""
        d = _dev_rows(self, rows)
        _chk(self.L.hydia_plain_db_update_device(self.h, first_vector, C.byref(d), 1 if normalise else 0))

    def _queries_device(self, fn, cls, rows, *args):
        d = _dev_rows(self, rows)
        out = (C.c_void_p * max(d.n, 1))()
        _chk(fn(self.h, C.byref(d), *args, out))
        return [cls(self, C.c_void_p(out[i])) for i in range(d.n)]

    def db_rekey(self, key, chunk=0):
        """hydia_db_rekey: key-switch every ciphertext of the resident kind-4 / 5 / 6 database in place with `key` (keygen_switch of
        the NEW receiver's context).  Layout, form, kind and order stay; afterwards import the new receiver's evaluation and public
        keys, and encrypt later updates under the new public key.  chunk > 0 (tests only) caps the ciphertexts per pass."""
        if key is not None:
            key = np.ascontiguousarray(key, dtype=np.uint64)
            assert key.size == self.dnum * 2 * self.nT * self.N
        _chk(self.L.hydia_db_rekey_chunked(self.h, None if key is None else _p(key), int(chunk)))

    def db_fill_random(self, n, seed=1):
        _chk(self.L.hydia_db_fill_random(self.h, n, seed))

    def db_save(self, path):
        """write the resident database (packed layout) to `path` — restart without re-enrolling"""
        _chk(self.L.hydia_db_save(self.h, str(path).encode()))

    def db_load(self, path):
        _chk(self.L.hydia_db_load(self.h, str(path).encode()))

    # ---- the split of the diagonal mat-vec (include/hydia.h): "auto" | "hoisted" | "bsgs" | a baby count; takes effect at the next enrolment
    def _matvec_code(self, mode):
        if isinstance(mode, str):
            return {"auto": 0, "hoisted": 1, "bsgs": self.bsgs_babies()}[mode]
        return int(mode)

    def set_matvec(self, mode):
        _chk(self.L.hydia_set_matvec(self.h, self._matvec_code(mode)))

    def get_matvec(self):
        m = self.L.hydia_get_matvec(self.h)
        return {0: "auto", 1: "hoisted"}.get(m, m)

    def db_kind(self):
        """0 none, 5 hoisted diagonals, 6 pre-rotated diagonals (baby-step / giant-step), 4 HERS columns, 1 rows (approach 1),
        7 / 8 a plain gallery in the form of 5 / 6"""
        return int(self.L.hydia_db_kind(self.h))

    def db_babies(self):
        """hoisted rotations per query the resident diagonal database is laid out for (vector_dim = the reference's form)"""
        return int(self.L.hydia_db_babies(self.h))

    def db_set_babies(self, babies):
        _chk(self.L.hydia_db_set_babies(self.h, int(babies)))

    def bsgs_babies(self):
        B = 1
        while B * B < self.dim:
            B *= 2
        return B

    def auto_babies(self, blocks):
        """what an enrolment of `blocks` 16384-vector blocks on this context would pick (its policy applied)"""
        return int(self.L.hydia_auto_babies(self.h, blocks))

    def db_residue_bits(self):
        """bits per stored residue of the 45/46-bit limbs of the resident database (46, 48 or 64; 0 = none)"""
        return int(self.L.hydia_db_residue_bits(self.h))

    def db_group(self):
        """0: the resident database is ciphertext-major; g > 0: group-sequential with groups of g blocks (hydia_db_group)"""
        return int(self.L.hydia_db_group(self.h))

    def db_stats(self):
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _chk(self.L.hydia_db_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- measurement
    def set_pq_batch_width(self, width):
        """UNSTABLE (hydia_set_pq_batch_width: measurements and tests only).  Queries one database pass of a plain-query batch serves
        on this context: 1, 2 or 4; 0 = the library's measured choice.  No result depends on it (tools/bench_plain_query.py --batch
        compares the widths with it)"""
        _chk(self.L.hydia_set_pq_batch_width(self.h, int(width)))

    def set_gallery_batch_width(self, width):
        """UNSTABLE (hydia_set_gallery_batch_width: measurements and tests only).  Queries one pass over a plain gallery serves in a
        *GalleryMulti batch on this context: 1, 2 or 4; 0 = the library's choice.  No result depends on it
        (tools/bench_plain_gallery.py --batch compares the widths with it)"""
        _chk(self.L.hydia_set_gallery_batch_width(self.h, int(width)))

    def kernel_time(self, name):
        ms, n = C.c_double(), C.c_uint64()
        _chk(self.L.hydia_kernel_time(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_time_reset(self):
        _chk(self.L.hydia_kernel_time_reset(self.h))

    def bench_ntt(self, polys, first_mod, n_mods, inverse=False, iters=10):
        ms = C.c_double()
        _chk(self.L.hydia_bench_ntt(self.h, polys, first_mod, n_mods, int(inverse), iters, C.byref(ms)))
        return ms.value

    def memory_stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(self.L.hydia_memory_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value


class DiagonalEnroller:
    """include/enroller_diag.h:7-27 — ctor (cc, pk, numVectors); pk lives inside the Context here."""

    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    def serializeDB(self, database, seed=None, first_block=0, matvec=None):
        """DiagonalEnroller::serializeDB (src/enroller/enroller_diag.cpp:12-53).  Normalises `database` IN PLACE like
        the reference; the ciphertexts go straight into HBM instead of serial/db_diagonal/index<t>.bin.  first_block > 0:
        `database` is one shard (a contiguous range of 16384-vector blocks) of a larger database.  matvec: None = the context's
        policy (Context.set_matvec), or "hoisted" / "bsgs" / a baby count (a sharded enrolment passes one decision to every shard).
        A tensor on the context's GPU (f64 / f32 / f16 / bf16) is enrolled where it lies (hydia_db_enroll_device): normalised on the
        device and never written; the form follows Context.set_matvec."""
        if _is_device_tensor(database):
            if not isinstance(self.cc, Context):
                raise HydiaError(-2, "hydia: rows in device memory are not taken on a sharded context")
            if first_block or matvec is not None:
                raise HydiaError(-1, "hydia: rows in device memory are enrolled whole, in the form of Context.set_matvec")
            d = _dev_rows(self.cc, database)
            if d.n != self.numVectors:
                raise HydiaError(-1, "hydia: the tensor holds another number of rows than the enroller was built for")
            _chk(self.cc.L.hydia_db_enroll_device(self.cc.h, C.byref(d), _p(_seed(seed))))
            return
        assert database.dtype == np.float64 and database.flags.c_contiguous
        assert database.shape == (self.numVectors, self.cc.dim)
        mv = 0 if matvec is None else self.cc._matvec_code(matvec)
        _chk(self.cc.L.hydia_db_enroll_shard_ex(self.cc.h, _p(database), self.numVectors, _p(_seed(seed)), first_block, mv))

    def updateRows(self, first_vector, rows, normalise=True, seed=None):
        """In-place update (Context.db_update): a fresh encryption of `rows` at vectors first_vector .. is added to the blocks they
        touch.  numVectors follows the database; a DiagonalSender / DiagonalReceiver built for the old count is rebuilt by the caller.
        `rows` may be a tensor on the context's GPU (Context.db_update_device)."""
        if _is_device_tensor(rows):
            self.cc.db_update_device(first_vector, rows, normalise, seed)
        else:
            self.cc.db_update(first_vector, rows, normalise, seed)
        self.numVectors = max(self.numVectors, first_vector + rows.shape[0])

    def appendDB(self, rows, seed=None):
        """append `rows` (normalised in place) after the last enrolled vector"""
        self.updateRows(self.numVectors, rows, True, seed)

    # ---- database deltas (include/hydia.h): this enroller holds the public key only; the database lies on the sender's machine
    def _one_context(self):
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: database deltas are not made on a sharded context (make one per shard context, with its first_block)")

    def _delta_to_wire(self, make, first_vector, rows, *args):
        """make: the name of the Context method (looked up only once the context is known to be one)"""
        self._one_context()
        m = getattr(self.cc, make)(first_vector, rows, *args)
        self.numVectors = max(self.numVectors, first_vector + rows.shape[0])
        return m

    def _db_to_wire(self, make, database, seeds, babies, first_block):
        """seeds: (draw, given) per seed the maker takes — each drawn ONCE here, for every block"""
        self._one_context()
        n, slots = database.shape[0], self.cc.N // 2
        drawn = [bytes(draw(given)) for draw, given in seeds]
        for lo in range(0, n, slots):
            yield getattr(self.cc, make)(lo, database[lo:lo + slots], True, *drawn, babies, first_block)
        self.numVectors = n

    def updateToWire(self, first_vector, rows, normalise=True, seed=None, babies=None, first_block=0):
        """updateRows for a database on ANOTHER machine: the update as one delta message (Context.db_delta_make) for
        DiagonalSender.applyDBWire.  Nothing resident on this context is touched; numVectors follows as in updateRows."""
        return self._delta_to_wire("db_delta_make", first_vector, rows, normalise, seed, babies, first_block)

    def appendToWire(self, rows, n_resident, seed=None, babies=None, first_block=0):
        """append `rows` (normalised in place) after the n_resident vectors the sender's database holds"""
        return self.updateToWire(n_resident, rows, True, seed, babies, first_block)

    def serializeDBToWire(self, database, seed=None, babies=None, first_block=0):
        """serializeDB for a sender on another machine: yields one delta message per 'slots'-vector block, in order; the first enrols
        on an empty sender context, every later one appends.  ONE seed for the whole database (None: drawn once from the OS), as
        an enrolment uses — the blocks differ in their nonces.  `database` is normalised IN PLACE (a tensor is never written)."""
        return self._db_to_wire("db_delta_make", database, [(_seed, seed)], babies, first_block)

    # ---- seeded database deltas (include/hydia.h): this enroller is the owner — it holds the SECRET key; half the bytes travel
    def updateToWireSeeded(self, first_vector, rows, normalise=True, seed=None, a_seed=None, babies=None, first_block=0):
        """updateToWire on a key-holding context: one SEEDED delta message (Context.db_delta_make_seeded) for
        DiagonalSender.applyDBWireSeeded.  a_seed=None draws a fresh hydia_random_seed."""
        return self._delta_to_wire("db_delta_make_seeded", first_vector, rows, normalise, seed, a_seed, babies, first_block)

    def appendToWireSeeded(self, rows, n_resident, seed=None, a_seed=None, babies=None, first_block=0):
        """append `rows` (normalised in place) after the n_resident vectors the sender's database holds, as a seeded delta"""
        return self.updateToWireSeeded(n_resident, rows, True, seed, a_seed, babies, first_block)

    def serializeDBToWireSeeded(self, database, seed=None, a_seed=None, babies=None, first_block=0):
        """serializeDBToWire as seeded deltas: one message per 'slots'-vector block, in order.  ONE seed and ONE a_seed for the whole
        database (None: each drawn once), as an enrolment uses one seed — the blocks differ in their nonces."""
        return self._db_to_wire("db_delta_make_seeded", database, [(_seed, seed), (_public_seed, a_seed)], babies, first_block)

    def rekeyDB(self, key):
        """Re-key the enrolled database in place (Context.db_rekey) with the switching key DiagonalReceiver.genSwitchKey of the NEW
        receiver made.  A sharded database is re-keyed shard by shard (db_rekey on every shard context, same key)."""
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: a sharded database is re-keyed shard by shard (Context.db_rekey on every shard context)")
        self.cc.db_rekey(key)


class PlainEnroller:
    """A gallery the sender may see (database kinds 7 / 8; no counterpart in the reference): DiagonalEnroller's constructor shape,
    serializeDB without a seed — the diagonals are encoded, not encrypted.  DiagonalSender and DiagonalReceiver are used unchanged.
    Trust model (include/hydia.h): the sender sees the gallery; the query and the result stay encrypted under the receiver's key."""

    def __init__(self, cc, num_vectors):
        if not isinstance(cc, Context):  # a ShardGroup: the sharded senders do not serve a plain gallery (its shard contexts refuse too)
            raise HydiaError(-2, "hydia: a plain gallery (kind 7 / 8) is not enrolled on a sharded context")
        self.cc, self.numVectors = cc, num_vectors

    def serializeDB(self, database):
        """normalises `database` IN PLACE like DiagonalEnroller.serializeDB; the form follows Context.set_matvec.  A tensor on the
        context's GPU is enrolled where it lies (hydia_plain_db_enroll_device): normalised on the device and never written"""
        if _is_device_tensor(database):
            d = _dev_rows(self.cc, database)
            if d.n != self.numVectors:
                raise HydiaError(-1, "hydia: the tensor holds another number of rows than the enroller was built for")
            _chk(self.cc.L.hydia_plain_db_enroll_device(self.cc.h, C.byref(d)))
            return
        assert database.dtype == np.float64 and database.flags.c_contiguous
        assert database.shape == (self.numVectors, self.cc.dim)
        _chk(self.cc.L.hydia_plain_db_enroll(self.cc.h, _p(database), self.numVectors))

    def updateRows(self, first_vector, rows, normalise=True):
        """In-place update (Context.plain_db_update): the encoded image of `rows` at vectors first_vector .. is added to the blocks
        they touch.  numVectors follows the gallery; a DiagonalSender / DiagonalReceiver built for the old count is rebuilt by the caller.
        `rows` may be a tensor on the context's GPU (Context.plain_db_update_device)."""
        if _is_device_tensor(rows):
            self.cc.plain_db_update_device(first_vector, rows, normalise)
        else:
            self.cc.plain_db_update(first_vector, rows, normalise)
        self.numVectors = max(self.numVectors, first_vector + rows.shape[0])

    def appendDB(self, rows):
        """append `rows` (normalised in place) after the last enrolled vector"""
        self.updateRows(self.numVectors, rows, True)


class SeededQuery:
    """What the receiver sends for `count` seeded queries (include/hydia.h): c0 [count][n_q][N] uint64, the PUBLIC a_seed (32 bytes)
    and nonce0 (query i was made with nonce0 + i).  The sender expands c1 (DiagonalSender.expandQueries)."""

    def __init__(self, c0, a_seed, nonce0):
        self.c0, self.a_seed, self.nonce0 = c0, bytes(a_seed), int(nonce0)

    def __len__(self):
        return self.c0.shape[0]

    @property
    def nbytes(self):
        """bytes on the wire: the c0 halves, the seed and the nonce"""
        return int(self.c0.nbytes) + 32 + 8


class SeededKeys:
    """The receiver's seeded key set as it travels: a_seed (32 bytes, public), the public key's b half [n_q][N] and, per key id (0 = the
    relinearisation key), the b halves [dnum][n_q+n_p][N]."""

    def __init__(self, a_seed, public_key, eval_keys):
        self.a_seed, self.public_key, self.eval_keys = bytes(a_seed), public_key, eval_keys

    @property
    def nbytes(self):
        return 32 + int(self.public_key.nbytes) + sum(int(b.nbytes) for b in self.eval_keys.values())


class DiagonalReceiver:
    """include/receiver_diag.h:7-16 + inherited HersReceiver::decrypt* (src/receiver/receiver_hers.cpp:26-54)."""

    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    # ---- seeded secret-key queries (include/hydia.h): half the bytes of encryptQuery's ciphertext; needs the secret key
    def encryptQuerySeeded(self, query, seed=None, a_seed=None, nonce=1):
        """one probe (a host vector, or a 1-D tensor on the context's GPU) -> SeededQuery of count 1"""
        if _is_device_tensor(query):
            if query.dim() != 1:
                raise HydiaError(-1, "hydia: encryptQuerySeeded takes one probe (encryptQueriesSeeded takes a matrix)")
            return self.encryptQueriesSeeded(query, seed, a_seed, nonce)
        query = np.ascontiguousarray(query, dtype=np.float64)
        assert query.shape == (self.cc.dim,)
        return self.encryptQueriesSeeded(query[None], seed, a_seed, nonce)

    def encryptQueriesSeeded(self, matrix, seed=None, a_seed=None, nonce0=1):
        """k probes (k x vector_dim host array, or a tensor on the context's GPU) -> ONE SeededQuery; probe i takes nonce0 + i.
        seed=None and a_seed=None each draw fresh OS entropy per call; a pair (a_seed, nonce) must never encrypt two queries."""
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: seeded queries are not made on a sharded context")
        L, key, akey = self.cc.L, _seed(seed), _seed(a_seed)
        if _is_device_tensor(matrix):
            d = _dev_rows(self.cc, matrix)
            c0 = np.zeros((d.n, self.cc.nQ, self.cc.N), dtype=np.uint64)
            _chk(L.hydia_encrypt_queries_seeded_device(self.cc.h, C.byref(d), _p(key), _p(akey), nonce0, _p(c0)))
        else:
            matrix = np.ascontiguousarray(matrix, dtype=np.float64)
            assert matrix.ndim == 2 and matrix.shape[1] == self.cc.dim
            c0 = np.zeros((matrix.shape[0], self.cc.nQ, self.cc.N), dtype=np.uint64)
            _chk(L.hydia_encrypt_queries_seeded(self.cc.h, _p(matrix), matrix.shape[0], _p(key), _p(akey), nonce0, _p(c0)))
        return SeededQuery(c0, akey.tobytes(), nonce0)

    # ---- wire messages (include/hydia.h): what crosses to the sender as bytes — packed on the GPU, range-checked on arrival
    def encryptQueryWire(self, query, seed=None, a_seed=None, nonce=1):
        """one probe (a host vector, or a 1-D tensor on the context's GPU) -> a type 2 wire message of count 1 (bytes)"""
        if _is_device_tensor(query):
            if query.dim() != 1:
                raise HydiaError(-1, "hydia: encryptQueryWire takes one probe (encryptQueriesWire takes a matrix)")
            return self.encryptQueriesWire(query, seed, a_seed, nonce)
        query = np.ascontiguousarray(query, dtype=np.float64)
        assert query.shape == (self.cc.dim,)
        return self.encryptQueriesWire(query[None], seed, a_seed, nonce)

    def encryptQueriesWire(self, matrix, seed=None, a_seed=None, nonce0=1):
        """encryptQueriesSeeded with c0 leaving the GPU packed: ONE type 2 message (bytes) that carries a_seed and nonce0 itself"""
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: seeded queries are not made on a sharded context")
        L, h, key, akey = self.cc.L, self.cc.h, _seed(seed), _seed(a_seed)
        if _is_device_tensor(matrix):
            d = _dev_rows(self.cc, matrix)
            return _wire_out(lambda buf, cap, n: L.hydia_encrypt_queries_seeded_wire_device(h, C.byref(d), _p(key), _p(akey), nonce0, buf, cap, n))
        matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        assert matrix.ndim == 2 and matrix.shape[1] == self.cc.dim
        return _wire_out(lambda buf, cap, n: L.hydia_encrypt_queries_seeded_wire(h, _p(matrix), matrix.shape[0], _p(key), _p(akey), nonce0, buf, cap, n))

    def exportKeysWire(self, path, seeded=True, rotations=None):
        """the key-set file: the public key, then the evaluation keys in ascending id — every key the context holds, or the
        relinearisation key and `rotations`.  seeded: half keys under the context's public key seed (Context.keygen_seeded)."""
        cc = self.cc
        if rotations is None:
            return cc.keys_save(path, seeded)
        ids = sorted({0} | {int(r) % cc.slots for r in rotations})
        with open(path, "wb") as f:
            f.write(b"HYDKEYS1" + np.array([1, 1 + len(ids)], dtype="<u4").tobytes())
            for r in [-1] + ids:
                f.write(cc.key_to_wire(r, seeded))

    def resultFromWire(self, message):
        """a scenario's result that the sender shipped with resultToWire -> the Ciphertext decryptIndex / decryptMembership take"""
        return self.cc.ct_from_wire(message)

    def exportKeysSeeded(self, rotations=None):
        """the seeded key set of Context.keygen_seeded as SeededKeys: the public key and every evaluation key the context holds (or
        the relinearisation key and `rotations`).  At the default parameters the full set is 6.5 GB of host memory in place of
        13 GB; a caller short of it loops over Context.export_eval_key_seeded key by key."""
        cc = self.cc
        if rotations is None:
            ids = [r for r in range(cc.slots) if cc.has_eval_key(r)]
        else:
            ids = [0] + [int(r) % cc.slots for r in rotations]
        return SeededKeys(cc.key_seed(), cc.export_public_key_seeded(), {r: cc.export_eval_key_seeded(r) for r in ids})

    def encryptQuery(self, query, seed=None, nonce=1):
        """a 1-D tensor on the context's GPU is encrypted where it lies (the one-row case of encryptQueries)"""
        if _is_device_tensor(query):
            if query.dim() != 1:
                raise HydiaError(-1, "hydia: encryptQuery takes one probe (encryptQueries takes a matrix)")
            return self.encryptQueries(query, seed, nonce)[0]
        query = np.ascontiguousarray(query, dtype=np.float64)
        assert query.shape == (self.cc.dim,)
        return self.cc._out(self.cc.L.hydia_encrypt_query, _p(query), _p(_seed(seed)), nonce)

    def encryptQueries(self, matrix, seed=None, nonce0=1):
        """one Ciphertext per row of `matrix` (k x vector_dim): row i is what encryptQuery(row i, seed, nonce0 + i) makes.  A tensor on
        the context's GPU is ONE library call (hydia_encrypt_queries_device): normalised, tiled, encoded and encrypted as a batch"""
        if _is_device_tensor(matrix):
            if not isinstance(self.cc, Context):
                raise HydiaError(-2, "hydia: rows in device memory are not taken on a sharded context")
            return self.cc._queries_device(self.cc.L.hydia_encrypt_queries_device, Ciphertext, matrix, _p(_seed(seed)), nonce0)
        matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        assert matrix.ndim == 2 and matrix.shape[1] == self.cc.dim
        key = _seed(seed)  # ONE key for the batch: the nonces tell the probes apart
        return [self.encryptQuery(row, bytes(key), nonce0 + i) for i, row in enumerate(matrix)]

    def genSwitchKey(self, old_secret, seed=None):
        """the switching key from the OLD receiver's secret (its Context.export_secret_key()) to this receiver's
        (Context.keygen_switch): hand it to the enroller / sender for DiagonalEnroller.rekeyDB"""
        return self.cc.keygen_switch(old_secret, seed)

    def decryptMembership(self, membership_cipher):
        r = C.c_int()
        _chk(self.cc.L.hydia_decrypt_membership(self.cc.h, membership_cipher.h, C.byref(r)))
        return bool(r.value)

    def decryptIndex(self, index_cipher):
        cap = len(index_cipher) * self.cc.slots
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        _chk(self.cc.L.hydia_decrypt_index(self.cc.h, index_cipher.h, _p(out), cap, C.byref(n)))
        return [int(v) for v in out[:n.value]]

    # ---- candidate lists and matches (include/hydia.h) from computeSimilarity's scores: selected on the GPU behind the decoder.  The
    # receiver sees every score here, as with Context.decrypt; indexScenario + decryptIndex stays the path that reveals only matches
    def _handles(self, results):
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: candidate lists are decrypted on one context")
        results = list(results)
        if not results:
            raise HydiaError(-1, "hydia: an empty list of results")
        return results, (C.c_void_p * len(results))(*[r.h for r in results])

    def decryptMatchesMulti(self, results, threshold, n_vectors=None, cap=None):
        """one (idx, val, total) per result: the indices of the slots >= threshold among the first n_vectors (default all), ascending,
        at most cap of them (default all), with their scores; total counts them all.  One library call and one synchronisation"""
        results, hs = self._handles(results)
        R, nv = len(results), int(n_vectors or 0)
        cap = (nv or max(len(r) for r in results) * self.cc.slots) if cap is None else int(cap)
        idx, val = np.zeros((R, max(cap, 1)), dtype=np.uint64), np.zeros((R, max(cap, 1)), dtype=np.float64)
        total = np.zeros(R, dtype=np.uint64)
        _chk(self.cc.L.hydia_decrypt_matches_multi(self.cc.h, hs, R, nv, float(threshold), _p(idx) if cap else None, _p(val) if cap else None,
                                                   cap, _p(total)))
        return [(idx[r, :min(cap, int(total[r]))].astype(np.int64), val[r, :min(cap, int(total[r]))].copy(), int(total[r])) for r in range(R)]

    def decryptTopKMulti(self, results, k, n_vectors=None):
        """one (idx, val) per result: its min(k, n) best slots among the first n_vectors (default all) by score descending, ties by
        ascending index.  One library call and one synchronisation"""
        results, hs = self._handles(results)
        R, nv, k = len(results), int(n_vectors or 0), int(k)
        room = max(1, min(k, nv or max(len(r) for r in results) * self.cc.slots))
        # (rows are k entries apart in the library's layout; a k beyond every result's slots is clamped here, where it changes nothing)
        kk = min(k, room) if k >= 1 else k
        idx, val, got = np.zeros((R, room), dtype=np.uint64), np.zeros((R, room), dtype=np.float64), np.zeros(R, dtype=np.uint64)
        _chk(self.cc.L.hydia_decrypt_topk_multi(self.cc.h, hs, R, nv, kk, _p(idx), _p(val), _p(got)))
        return [(idx[r, :int(got[r])].astype(np.int64), val[r, :int(got[r])].copy()) for r in range(R)]

    def decryptMatches(self, cts, threshold, n_vectors=None, cap=None):
        """(idx, val, total) of one result (decryptMatchesMulti of one)"""
        return self.decryptMatchesMulti([cts], threshold, n_vectors, cap)[0]

    def decryptTopK(self, cts, k, n_vectors=None):
        """(idx, val) of one result (decryptTopKMulti of one)"""
        return self.decryptTopKMulti([cts], k, n_vectors)[0]


class DiagonalSender:
    """include/sender_diag.h:5-28 — the three virtuals of include/sender.h:28-35."""

    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    # ---- plain query (include/hydia.h: the sender knows the probe, the database stays encrypted; kinds 5 / 6 only)
    def encodeQuery(self, query):
        """exactly the plaintext DiagonalReceiver.encryptQuery encrypts, encoded and not encrypted: no seed, no nonce, no public key"""
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: a plain query is not served on a sharded context")
        if _is_device_tensor(query):  # a 1-D tensor on the context's GPU: the one-row case of encodeQueries
            if query.dim() != 1:
                raise HydiaError(-1, "hydia: encodeQuery takes one probe (encodeQueries takes a matrix)")
            return self.encodeQueries(query)[0]
        query = np.ascontiguousarray(query, dtype=np.float64)
        assert query.shape == (self.cc.dim,)
        h = C.c_void_p()
        _chk(self.cc.L.hydia_encode_query(self.cc.h, _p(query), C.byref(h)))
        return Plaintext(self.cc, h)

    # ---- seeded keys and queries (include/hydia.h): the sender regenerates the uniform halves on its GPU from the public seed
    def importKeysSeeded(self, keys):
        """DiagonalReceiver.exportKeysSeeded's SeededKeys into this context: the full public key and evaluation keys, bit for bit"""
        self.cc.import_public_key_seeded(keys.public_key, keys.a_seed)
        for r, b in keys.eval_keys.items():
            self.cc.import_eval_key_seeded(r, b, keys.a_seed)

    def expandQueries(self, seeded):
        """a SeededQuery -> one ordinary Ciphertext per probe (hydia_ct_expand_seeded): what every method below takes"""
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: seeded queries are expanded on one context (hand the handles to the sharded sender)")
        n = len(seeded)
        c0 = np.ascontiguousarray(seeded.c0, dtype=np.uint64)
        assert c0.shape == (n, self.cc.nQ, self.cc.N)
        out = (C.c_void_p * max(n, 1))()
        _chk(self.cc.L.hydia_ct_expand_seeded(self.cc.h, _p(c0), n, _p(_seed(seeded.a_seed)), seeded.nonce0, out))
        return [Ciphertext(self.cc, C.c_void_p(out[i])) for i in range(n)]

    def expandQuery(self, seeded):
        """a SeededQuery of one probe -> its Ciphertext"""
        if len(seeded) != 1:
            raise HydiaError(-1, "hydia: expandQuery takes one probe (expandQueries takes a batch)")
        return self.expandQueries(seeded)[0]

    # ---- wire messages (include/hydia.h): the checked path for what arrives from outside
    def importKeysWire(self, path):
        """DiagonalReceiver.exportKeysWire's file into this context (hydia_keys_load; not transactional)"""
        self.cc.keys_load(path)

    def _apply_db_wire(self, apply, message):
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: database deltas are not applied on a sharded context (apply one per shard context)")
        getattr(self.cc, apply)(message)
        self.numVectors = self.cc.db_stats()[0]
        return self.numVectors

    def applyDBWire(self, message):
        """a delta message of DiagonalEnroller.updateToWire / appendToWire / serializeDBToWire into this sender's database
        (Context.db_delta_apply: checked, transactional); returns the new vector count, which numVectors follows"""
        return self._apply_db_wire("db_delta_apply", message)

    def applyDBWireSeeded(self, message):
        """a SEEDED delta message of DiagonalEnroller.updateToWireSeeded / appendToWireSeeded / serializeDBToWireSeeded into this
        sender's database (Context.db_delta_apply_seeded: checked, transactional, no key needed); returns the new vector count"""
        return self._apply_db_wire("db_delta_apply_seeded", message)

    def queryFromWire(self, message):
        """a query message -> what expandQuery / Context.import_ct return, ready for every single, *Multi and *GalleryMulti method: a
        type 2 message of one probe or a type 1 message gives ONE Ciphertext, a type 2 message of several a list of them"""
        r = self.cc.ct_from_wire(message)
        return r[0] if isinstance(r, list) and len(r) == 1 else r

    def queriesFromWire(self, message):
        """always a list: one Ciphertext per probe of a type 2 message (the batch of a type 1 message as its only element)"""
        r = self.cc.ct_from_wire(message)
        return r if isinstance(r, list) else [r]

    def resultToWire(self, result_cipher):
        """a scenario's output as one wire message (bytes) for DiagonalReceiver.resultFromWire"""
        return result_cipher.to_wire()

    def scoresToWire(self, scores, limbs=2):
        """computeSimilarity's scores as one wire message of their first `limbs` limbs (1 or 2) for DiagonalReceiver.resultFromWire:
        the decoder reads at most the first two limbs, so nothing the receiver decrypts changes with limbs=2, and limbs=1 halves
        the message again at the precision of q_0 alone"""
        if limbs not in (1, 2):
            raise HydiaError(-1, "hydia: scoresToWire ships 1 or 2 limbs")
        return self.cc.ct_limb_prefix(scores, limbs).to_wire()

    @staticmethod
    def _no_plain(what, *queries):
        if any(isinstance(q, Plaintext) for q in queries):
            raise HydiaError(-1, "hydia: %s does not take a plain query (batches and caller-supplied rotations are not served for it)" % what)

    def rotateQuery(self, query_cipher):
        self._no_plain("rotateQuery", query_cipher)
        return self.cc._out(self.cc.L.hydia_rotate_query, query_cipher.h)

    def computeSimilarity(self, query_cipher):
        if isinstance(query_cipher, Plaintext):
            return self.cc._out(self.cc.L.hydia_compute_similarity_pq, query_cipher.h)
        return self.cc._out(self.cc.L.hydia_compute_similarity, query_cipher.h)

    def membershipScenario(self, query_cipher):
        if isinstance(query_cipher, Plaintext):
            return self.cc._out(self.cc.L.hydia_membership_scenario_pq, query_cipher.h)
        return self.cc._out(self.cc.L.hydia_membership_scenario, query_cipher.h)

    def indexScenario(self, query_cipher):
        if isinstance(query_cipher, Plaintext):
            return self.cc._out(self.cc.L.hydia_index_scenario_pq, query_cipher.h)
        return self.cc._out(self.cc.L.hydia_index_scenario, query_cipher.h)

    # ---- several queries in one pass over the database (an extension: the reference serves one query per call).  A list of query
    # ciphertexts in, a list out: per query exactly what the single-query method returns
    def _batch_call(self, fn, qs):
        """the C call of every batch method: the handles of `qs` in, one owning Ciphertext per query out"""
        n = len(qs)
        hs = (C.c_void_p * max(n, 1))(*[q.h for q in qs])
        out = (C.c_void_p * max(n, 1))()
        _chk(getattr(self.cc.L, fn)(self.cc.h, hs, n, out))
        return [Ciphertext(self.cc, C.c_void_p(out[i])) for i in range(n)]

    def _multi(self, fn, query_ciphers):
        qs = list(query_ciphers)
        self._no_plain("a *Multi method", *qs)
        return self._batch_call(fn, qs)

    def computeSimilarityMulti(self, query_ciphers):
        return self._multi("hydia_compute_similarity_multi", query_ciphers)

    def indexScenarioMulti(self, query_ciphers):
        return self._multi("hydia_index_scenario_multi", query_ciphers)

    def membershipScenarioMulti(self, query_ciphers):
        return self._multi("hydia_membership_scenario_multi", query_ciphers)

    # ---- several PLAIN queries in one pass over the database (names of their own: the *Multi methods above keep refusing a Plaintext).
    # A list of Plaintext in, a list out: per query exactly what the single-query method returns
    def encodeQueries(self, matrix):
        """one Plaintext per row of `matrix` (k x vector_dim), each what encodeQuery makes of that row.  A tensor on the context's GPU
        is ONE library call (hydia_encode_queries_device): the probes are normalised, tiled and encoded as a batch where they lie"""
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: a plain query is not served on a sharded context")
        if _is_device_tensor(matrix):
            return self.cc._queries_device(self.cc.L.hydia_encode_queries_device, Plaintext, matrix)
        matrix = np.ascontiguousarray(matrix, dtype=np.float64)
        assert matrix.ndim == 2 and matrix.shape[1] == self.cc.dim
        return [self.encodeQuery(row) for row in matrix]

    def _plain_multi(self, fn, plaintexts):
        qs = list(plaintexts)
        if any(not isinstance(q, Plaintext) for q in qs):
            raise HydiaError(-1, "hydia: a *PlainMulti method takes Plaintexts (encodeQuery); encrypted queries go to the *Multi methods")
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: a plain query is not served on a sharded context")
        return self._batch_call(fn, qs)

    def computeSimilarityPlainMulti(self, plaintexts):
        return self._plain_multi("hydia_compute_similarity_pq_multi", plaintexts)

    def indexScenarioPlainMulti(self, plaintexts):
        return self._plain_multi("hydia_index_scenario_pq_multi", plaintexts)

    def membershipScenarioPlainMulti(self, plaintexts):
        return self._plain_multi("hydia_membership_scenario_pq_multi", plaintexts)

    # ---- several ENCRYPTED queries against a PLAIN gallery (kinds 7 / 8) in shared passes over it (names of their own: the *Multi
    # methods keep refusing a plain gallery).  A list of Ciphertext in, a list out: per query exactly what the single method returns
    def _gallery_multi(self, fn, query_ciphers):
        qs = list(query_ciphers)
        if any(not isinstance(q, Ciphertext) or isinstance(q, Plaintext) for q in qs):
            raise HydiaError(-1, "hydia: a *GalleryMulti method takes encrypted queries (Ciphertext): a plain gallery under a plain query would keep nothing private")
        if not isinstance(self.cc, Context):
            raise HydiaError(-2, "hydia: a plain gallery (kind 7 / 8) is not served on a sharded context")
        return self._batch_call(fn, qs)

    def computeSimilarityGalleryMulti(self, query_ciphers):
        return self._gallery_multi("hydia_compute_similarity_gallery_multi", query_ciphers)

    def indexScenarioGalleryMulti(self, query_ciphers):
        return self._gallery_multi("hydia_index_scenario_gallery_multi", query_ciphers)

    def membershipScenarioGalleryMulti(self, query_ciphers):
        return self._gallery_multi("hydia_membership_scenario_gallery_multi", query_ciphers)

    # ---- loop A split over the GPUs of a node (sender_diag.cpp:23-26 cut into ranges; image_matching_amd.sharding)
    def rotateQueryRange(self, query_cipher, first, count):
        """rotations first .. first+count-1 of the query (0 = the query itself) as a batch of `count` ciphertexts"""
        self._no_plain("rotateQueryRange", query_cipher)
        return self.cc._out(self.cc.L.hydia_rotate_query_range, query_cipher.h, first, count)

    def rotateQueryRangeInto(self, query_cipher, first, count, dev_ptr):
        """rotations first .. first+count-1 of the query (0 = the query itself) into device memory [count][2][nQ][N]"""
        self._no_plain("rotateQueryRangeInto", query_cipher)
        _chk(self.cc.L.hydia_rotate_query_range_into(self.cc.h, query_cipher.h, first, count, C.c_void_p(dev_ptr)))

    def computeSimilarityRotated(self, rotations):
        self._no_plain("computeSimilarityRotated", rotations)
        return self.cc._out(self.cc.L.hydia_compute_similarity_rotated, rotations.h)

    def indexScenarioRotated(self, rotations):
        self._no_plain("indexScenarioRotated", rotations)
        return self.cc._out(self.cc.L.hydia_index_scenario_rotated, rotations.h)


# ---- HERS, approach 4: include/enroller_hers.h:16-37, include/receiver_hers.h:9-28, include/sender_hers.h:9-44
class HersEnroller:
    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    def serializeDB(self, database, seed=None):
        """HersEnroller::serializeDB (src/enroller/enroller_hers.cpp:40-93): index-batched packing, normalises in place."""
        assert database.dtype == np.float64 and database.flags.c_contiguous
        assert database.shape == (self.numVectors, self.cc.dim)
        _chk(self.cc.L.hydia_hers_db_enroll(self.cc.h, _p(database), self.numVectors, _p(_seed(seed))))


class HersReceiver(DiagonalReceiver):
    """HersReceiver::encryptQuery (src/receiver/receiver_hers.cpp:13-24); decrypt* are the shared ones (:26-54)."""

    def encryptQuery(self, query, seed=None, nonce=1000):
        query = np.ascontiguousarray(query, dtype=np.float64)
        assert query.shape == (self.cc.dim,)
        return self.cc._out(self.cc.L.hydia_hers_encrypt_query, _p(query), _p(_seed(seed)), nonce)


class HersSender:
    """include/sender_hers.h:9-44 — computeSimilarity / membershipScenario / indexScenario of approach 4."""

    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    def computeSimilarity(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_hers_compute_similarity, query_cipher.h)

    def membershipScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_hers_membership_scenario, query_cipher.h)

    def indexScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_hers_index_scenario, query_cipher.h)


# ---- the literature baseline, approach 1: include/enroller_base.h, include/receiver_base.h, include/sender_base.h
class BaseEnroller:
    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    def serializeDB(self, database, seed=None):
        """BaseEnroller::serializeDB (src/enroller/enroller_base.cpp:13-56): slots / vector_dim vectors back to back per
        ciphertext, normalises in place."""
        assert database.dtype == np.float64 and database.flags.c_contiguous
        assert database.shape == (self.numVectors, self.cc.dim)
        _chk(self.cc.L.hydia_base_db_enroll(self.cc.h, _p(database), self.numVectors, _p(_seed(seed))))


class BaseReceiver(HersReceiver):
    """BaseReceiver::encryptQuery (src/receiver/receiver_base.cpp:13-26) is the tiled single ciphertext of approach 5; decrypt* are
    HersReceiver's (include/receiver_base.h derives from it)."""

    def encryptQuery(self, query, seed=None, nonce=1):
        return DiagonalReceiver.encryptQuery(self, query, seed, nonce)


class BaseSender(HersSender):
    """include/sender_base.h (derives from HersSender) — computeSimilarity returns the merged score ciphertexts."""

    def computeSimilarity(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_base_compute_similarity, query_cipher.h)

    def membershipScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_base_membership_scenario, query_cipher.h)

    def indexScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_base_index_scenario, query_cipher.h)


# ---- GROTE group testing, approach 2: include/sender_grote.h (derives from BaseSender), include/receiver_grote.h (from BaseReceiver);
# the enroller is BaseEnroller (src/main.cpp:236-238)
class GroteSender(BaseSender):
    """computeSimilarity is BaseSender's.  indexScenario returns the pair (rows, columns): the reference's single vector holds the row
    ciphertexts followed by the column ciphertexts, which are two batches here (their limb counts differ by one)."""

    def membershipScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_grote_membership_scenario, query_cipher.h)

    def indexScenario(self, query_cipher):
        rows, cols = C.c_void_p(), C.c_void_p()
        _chk(self.cc.L.hydia_grote_index_scenario(self.cc.h, query_cipher.h, C.byref(rows), C.byref(cols)))
        return Ciphertext(self.cc, rows), Ciphertext(self.cc, cols)


class GroteReceiver(BaseReceiver):
    """GroteReceiver::decryptIndex (src/receiver/receiver_grote.cpp:12-65): rows x columns of one matrix -> indices."""

    def decryptIndex(self, index_cipher):
        rows, cols = index_cipher
        cap = max(1, len(rows) * len(cols) * self.cc.slots)
        while True:
            out = np.zeros(cap, dtype=np.uint64)
            n = C.c_size_t()
            _chk(self.cc.L.hydia_grote_decrypt_index(self.cc.h, rows.h, cols.h, self.numVectors, _p(out), cap, C.byref(n)))
            if n.value <= cap:
                return [int(v) for v in out[:n.value]]
            cap = n.value


# ---- the Blind-Match method, approach 3: include/enroller_blind.h, include/receiver_blind.h, include/sender_blind.h.  The reference fixes
# CHUNK_LEN = 128 at compile time; the roles here take it as a constructor argument with that default, so a small ring can be tested
class BlindEnroller:
    def __init__(self, cc, num_vectors):
        self.cc, self.numVectors = cc, num_vectors

    def serializeDB(self, database, chunk_length=BLIND_CHUNK_LEN, seed=None):
        """BlindEnroller::serializeDB (src/enroller/enroller_blind.cpp:13-90): per matrix of slots / chunk_length vectors one ciphertext
        per chunk of coordinates, normalises in place."""
        assert database.dtype == np.float64 and database.flags.c_contiguous
        assert database.shape == (self.numVectors, self.cc.dim)
        _chk(self.cc.L.hydia_blind_db_enroll(self.cc.h, _p(database), self.numVectors, int(chunk_length), _p(_seed(seed))))


class BlindReceiver(HersReceiver):
    """BlindReceiver (src/receiver/receiver_blind.cpp): the query is vector_dim / chunk_length tiled ciphertexts in one batch;
    decryptMembership is HersReceiver's."""

    def __init__(self, cc, num_vectors, chunk_length=BLIND_CHUNK_LEN):
        super().__init__(cc, num_vectors)
        self.chunkLength = int(chunk_length)

    def encryptQuery(self, query, seed=None, nonce=1):
        query = np.ascontiguousarray(query, dtype=np.float64)
        assert query.shape == (self.cc.dim,)
        return self.cc._out(self.cc.L.hydia_blind_encrypt_query, _p(query), self.chunkLength, _p(_seed(seed)), nonce)

    def decryptIndex(self, index_cipher):
        """receiver_blind.cpp:28-54: a value >= 1.0 at slot j of ciphertext i is vector i slots + j // chunk + (j % chunk) (slots // chunk).
        Like the reference, it does NOT filter indices that fall into the padding past numVectors."""
        cap = len(index_cipher) * self.cc.slots
        out = np.zeros(cap, dtype=np.uint64)
        n = C.c_size_t()
        _chk(self.cc.L.hydia_blind_decrypt_index(self.cc.h, index_cipher.h, self.chunkLength, _p(out), cap, C.byref(n)))
        return [int(v) for v in out[:n.value]]


class BlindSender(HersSender):
    """include/sender_blind.h (derives from HersSender) — computeSimilarity returns the compressed score ciphertexts; the chunk length
    is the resident database's."""

    def computeSimilarity(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_blind_compute_similarity, query_cipher.h)

    def membershipScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_blind_membership_scenario, query_cipher.h)

    def indexScenario(self, query_cipher):
        return self.cc._out(self.cc.L.hydia_blind_index_scenario, query_cipher.h)
