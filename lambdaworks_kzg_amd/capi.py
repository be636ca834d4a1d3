"""ctypes binding of liblambdaworks_kzg.so -- the C ABI declared in include/lambdaworks_kzg_amd.h.

This is the same stub a maintainer of a Python consumer of lambdaworks_kzg / c-kzg-4844 would write
(INTEGRATION.md shows the cgo / Rust FFI equivalents). Function names, argument order and error
behaviour mirror the reference's extern "C" surface (/root/reference/src/lib.rs:245-829).

There is NO CPU fallback: without the built HIP library the import of `lib()` raises, and without a
GPU every compute entry point returns C_KZG_ERROR.
"""
import ctypes as C
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LWKZG_LIBRARY") or os.path.join(_HERE, "lib", "liblambdaworks_kzg.so")  # override: A/B builds

C_KZG_OK, C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC = 0, 1, 2, 3
MODE_REFERENCE, MODE_CKZG, MODE_ETH = 0, 1, 2   # MODE_ETH: the consensus specs' encoding (big-endian evaluation form, c-kzg-4844 2.x)
FIELD_ELEMENTS_PER_BLOB = 4096
BYTES_PER_BLOB = 4096 * 32
BYTES_PER_COMMITMENT = 48
BYTES_PER_PROOF = 48
# EIP-7594
FIELD_ELEMENTS_PER_EXT_BLOB = 8192
FIELD_ELEMENTS_PER_CELL = 64
CELLS_PER_EXT_BLOB = 128
BYTES_PER_CELL = 2048


class KZGSettings(C.Structure):
    """#[repr(C)] KZGSettings, /root/reference/src/lib.rs:206-222."""
    _fields_ = [("fs", C.c_void_p), ("g1_values", C.c_void_p), ("g2_values", C.c_void_p)]


class FFTSettings(C.Structure):
    """#[repr(C)] FFTSettings, /root/reference/src/lib.rs:173-197."""
    _fields_ = [("max_width", C.c_uint64), ("expanded_roots_of_unity", C.c_void_p),
                ("reverse_roots_of_unity", C.c_void_p), ("roots_of_unity", C.c_void_p)]


VERIFIER_DEPTH = 4   # LWKZG_VERIFIER_DEPTH


class VerifyResult(C.Structure):
    """LwkzgVerifyResult: where an asynchronous verification answers. state is written last (0 = pending, 1 = complete)."""
    _fields_ = [("state", C.c_int32), ("rc", C.c_int32), ("ok", C.c_int32), ("first_bad", C.c_uint32),
                ("r", C.c_uint8 * 32), ("partial", C.c_uint8 * 328)]


class CellVerifyResult(C.Structure):
    """LwkzgCellVerifyResult: where an asynchronous cell verification answers. state is written last (0 = pending, 1 = complete)."""
    _fields_ = [("state", C.c_int32), ("rc", C.c_int32), ("ok", C.c_int32), ("first_bad", C.c_uint32), ("m", C.c_uint32),
                ("partials", C.c_uint8 * (32 + 4 * 97))]


# every symbol include/lambdaworks_kzg_amd.h declares
EXPORTED_SYMBOLS = [
    "load_trusted_setup", "load_trusted_setup_file", "free_trusted_setup", "blob_to_kzg_commitment",
    "compute_kzg_proof", "compute_blob_kzg_proof", "verify_kzg_proof", "verify_blob_kzg_proof",
    "verify_blob_kzg_proof_batch",
    "lwkzg_set_mode", "lwkzg_get_mode", "lwkzg_settings_set_mode", "lwkzg_settings_get_mode",
    "lwkzg_blob_to_kzg_commitment_batch",
    "lwkzg_compute_blob_kzg_proof_batch", "lwkzg_compute_kzg_proof_batch",
    "lwkzg_blob_to_kzg_commitment_batch_device", "lwkzg_compute_blob_kzg_proof_batch_device", "lwkzg_reserve", "lwkzg_reserve_streams",
    "lwkzg_g1_lincomb_setup_device", "lwkzg_fr_ntt4096_device",
    "lwkzg_setup_image_bytes", "lwkzg_setup_export_device", "lwkzg_setup_import_device",
    "lwkzg_device_count", "lwkzg_set_device", "lwkzg_version", "lwkzg_last_error",
    "lwkzg_profile_enable", "lwkzg_profile_reset", "lwkzg_profile_report", "lwkzg_profile_sources",
    "lwkzg_msm_window_bits", "lwkzg_msm_num_windows", "lwkzg_pairing_product_is_one",
    "lwkzg_challenge_digests_host", "lwkzg_challenge_digests_host_mode", "lwkzg_batch_challenge_host", "lwkzg_g1_msm_tiled_device", "lwkzg_g1_sum_compressed",
    "lwkzg_commit_and_prove_batch_device", "lwkzg_enable_direct_table", "lwkzg_direct_table_bits", "lwkzg_direct_table_forms", "lwkzg_enable_direct_table_forms", "lwkzg_direct_num_windows", "lwkzg_direct_row_bytes",
    "lwkzg_compute_challenges_device",
    "lwkzg_timing_report", "lwkzg_runtime_init", "lwkzg_knob_report", "lwkzg_last_proof_schedule",
    "lwkzg_multi_load", "lwkzg_multi_load_file", "lwkzg_multi_free", "lwkzg_multi_device_count", "lwkzg_multi_device", "lwkzg_multi_settings",
    "lwkzg_multi_set_mode", "lwkzg_multi_enable_direct_table", "lwkzg_multi_blob_to_kzg_commitment_batch",
    "lwkzg_multi_compute_blob_kzg_proof_batch", "lwkzg_multi_compute_kzg_proof_batch", "lwkzg_multi_verify_blob_kzg_proof_batch",
    "lwkzg_multi_g1_msm_tiled",
    "lwkzg_release_context", "lwkzg_verify_shard_begin", "lwkzg_verify_shard_partial", "lwkzg_verify_shard_free", "lwkzg_verify_shards_finish",
    "lwkzg_verify_blob_kzg_proof_batch_device", "lwkzg_verify_shard_begin_device", "lwkzg_shard_range",
    "lwkzg_multi_blob_to_kzg_commitment_batch_device", "lwkzg_multi_compute_blob_kzg_proof_batch_device",
    "lwkzg_multi_verify_blob_kzg_proof_batch_device", "lwkzg_clock_probe_mhz",
    "lwkzg_verify_blob_kzg_proof_each", "lwkzg_verify_blob_kzg_proof_each_device", "lwkzg_verify_kzg_proof_each",
    "lwkzg_pairing_line_table",
    "lwkzg_compute_cells_and_kzg_proofs", "lwkzg_compute_cells_and_kzg_proofs_batch", "lwkzg_compute_cells_and_kzg_proofs_batch_device",
    "lwkzg_compute_cells_and_kzg_proofs_columns", "lwkzg_compute_cells_and_kzg_proofs_columns_device",
    "lwkzg_recover_cells_and_kzg_proofs_columns", "lwkzg_recover_cells_and_kzg_proofs_columns_device",
    "lwkzg_verify_cell_kzg_proof_batch", "lwkzg_verify_cell_kzg_proof_batch_device", "lwkzg_cell_verify_partials",
    "lwkzg_cell_batch_challenge_host",
    "lwkzg_verify_cell_kzg_proof_each", "lwkzg_verify_cell_kzg_proof_each_device", "lwkzg_cell_verify_each_points",
    "lwkzg_verify_cell_kzg_proof_groups", "lwkzg_verify_cell_kzg_proof_groups_device", "lwkzg_cell_verify_groups_partials",
    "lwkzg_verify_blob_cell_kzg_proofs_batch", "lwkzg_verify_blob_cell_kzg_proofs_batch_device", "lwkzg_blob_cell_verify_partials",
    "lwkzg_verify_blob_cell_kzg_proofs_groups", "lwkzg_verify_blob_cell_kzg_proofs_groups_device", "lwkzg_blob_cell_verify_groups_partials",
    "lwkzg_recover_cells_and_kzg_proofs", "lwkzg_recover_cells_and_kzg_proofs_batch", "lwkzg_recover_cells_and_kzg_proofs_batch_device",
    "lwkzg_recover_cells_and_kzg_proofs_mixed", "lwkzg_recover_cells_and_kzg_proofs_mixed_device",
    "lwkzg_set_cell_proof_engine", "lwkzg_cell_proof_engine", "lwkzg_fk20_table_bytes", "lwkzg_fk20_chunk_blobs", "lwkzg_fk20_points",
    "lwkzg_load_trusted_setup_lagrange", "lwkzg_load_trusted_setup_ckzg", "lwkzg_load_trusted_setup_file_ckzg", "lwkzg_setup_g1_lagrange",
    "lwkzg_trusted_setup_check",
    "lwkzg_verifier_new", "lwkzg_verifier_enqueue", "lwkzg_verifier_pending", "lwkzg_verifier_wait", "lwkzg_verifier_free",
    "lwkzg_verifier_host_steps",
    "lwkzg_cell_verifier_new", "lwkzg_cell_verifier_enqueue", "lwkzg_cell_verifier_pending", "lwkzg_cell_verifier_wait",
    "lwkzg_cell_verifier_free", "lwkzg_cell_verifier_host_steps", "lwkzg_cell_group_device",
    "lwkzg_cell_verifier_new_groups", "lwkzg_cell_verifier_enqueue_groups", "lwkzg_cell_group_segmented_device",
    "lwkzg_cell_verifier_groups_host_steps",
    "lwkzg_cell_verifier_new_blobs", "lwkzg_cell_verifier_enqueue_blobs", "lwkzg_cell_verifier_enqueue_blobs_groups", "lwkzg_blob_group_device",
    "lwkzg_verify_kzg_proof_batch", "lwkzg_verify_kzg_proof_batch_device", "lwkzg_verify_kzg_proof_batch_partial",
    "lwkzg_verifier_enqueue_openings", "lwkzg_verify_kzg_proof_each_device",
]

_lib = None


def lib():
    """Load the HIP shared library; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C lambdaworks_kzg_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    l = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
    ps = C.POINTER(KZGSettings)
    l.load_trusted_setup.argtypes = [ps, C.c_char_p, sz, C.c_char_p, sz]
    l.load_trusted_setup_file.argtypes = [ps, vp]
    l.free_trusted_setup.argtypes = [ps]
    l.blob_to_kzg_commitment.argtypes = [C.c_char_p, C.c_char_p, ps]
    l.compute_kzg_proof.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, ps]
    l.compute_blob_kzg_proof.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, ps]
    l.verify_kzg_proof.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, ps]
    l.verify_blob_kzg_proof.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, C.c_char_p, ps]
    l.verify_blob_kzg_proof_batch.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_set_mode.argtypes = [ci]
    l.lwkzg_timing_report.argtypes = [ps, C.c_char_p, sz]
    l.lwkzg_timing_report.restype = sz
    l.lwkzg_knob_report.argtypes = [C.c_char_p, sz]
    l.lwkzg_knob_report.restype = sz
    l.lwkzg_settings_set_mode.argtypes = [ps, ci]
    l.lwkzg_settings_get_mode.argtypes = [ps]
    l.lwkzg_blob_to_kzg_commitment_batch.argtypes = [C.c_char_p, C.c_char_p, sz, ps, C.POINTER(sz)]
    l.lwkzg_compute_blob_kzg_proof_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, ps, C.POINTER(sz)]
    l.lwkzg_compute_kzg_proof_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps, C.POINTER(sz)]
    l.lwkzg_blob_to_kzg_commitment_batch_device.argtypes = [vp, vp, sz, ps, vp, vp]
    l.lwkzg_compute_blob_kzg_proof_batch_device.argtypes = [vp, vp, vp, sz, ps, vp, vp]
    l.lwkzg_compute_challenges_device.argtypes = [vp, vp, vp, sz, ps, vp]
    l.lwkzg_verify_blob_kzg_proof_batch_device.argtypes = [C.POINTER(C.c_bool), vp, vp, vp, sz, ps, vp]
    pu8, pi32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    l.lwkzg_verify_blob_kzg_proof_each.argtypes = [pu8, pi32, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_blob_kzg_proof_each_device.argtypes = [pu8, pi32, vp, vp, vp, sz, ps, vp]
    l.lwkzg_verify_kzg_proof_each.argtypes = [pu8, pi32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_kzg_proof_each_device.argtypes = [pu8, pi32, vp, vp, vp, vp, sz, ps, vp]
    l.lwkzg_verify_kzg_proof_batch.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_kzg_proof_batch_device.argtypes = [C.POINTER(C.c_bool), vp, vp, vp, vp, sz, ps, vp]
    l.lwkzg_verify_kzg_proof_batch_partial.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_pairing_line_table.argtypes = [C.c_char_p, C.c_char_p]
    l.lwkzg_compute_cells_and_kzg_proofs.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, ps]
    l.lwkzg_compute_cells_and_kzg_proofs_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, ps, C.POINTER(sz)]
    l.lwkzg_compute_cells_and_kzg_proofs_batch_device.argtypes = [vp, vp, vp, sz, ps, vp, vp]
    pu64 = C.POINTER(C.c_uint64)
    l.lwkzg_verify_cell_kzg_proof_batch.argtypes = [C.POINTER(C.c_bool), C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_cell_kzg_proof_batch_device.argtypes = [C.POINTER(C.c_bool), vp, vp, vp, vp, sz, ps, vp]
    l.lwkzg_cell_verify_partials.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_cell_batch_challenge_host.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, ci]
    l.lwkzg_verify_cell_kzg_proof_each.argtypes = [pu8, pi32, C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_cell_kzg_proof_each_device.argtypes = [pu8, pi32, vp, vp, vp, vp, sz, ps, vp]
    l.lwkzg_cell_verify_each_points.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_cell_kzg_proof_groups.argtypes = [pu8, pi32, C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, pu64, sz, ps]
    l.lwkzg_verify_cell_kzg_proof_groups_device.argtypes = [pu8, pi32, vp, vp, vp, vp, sz, pu64, sz, ps, vp]
    l.lwkzg_cell_verify_groups_partials.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, C.c_char_p, sz, pu64, sz, ps]
    l.lwkzg_verify_blob_cell_kzg_proofs_batch.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_blob_cell_kzg_proofs_batch_device.argtypes = [C.POINTER(C.c_bool), vp, vp, vp, sz, ps, vp]
    l.lwkzg_blob_cell_verify_partials.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_blob_cell_kzg_proofs_groups.argtypes = [pu8, pi32, C.c_char_p, C.c_char_p, C.c_char_p, sz, pu64, sz, ps]
    l.lwkzg_verify_blob_cell_kzg_proofs_groups_device.argtypes = [pu8, pi32, vp, vp, vp, sz, pu64, sz, ps, vp]
    l.lwkzg_blob_cell_verify_groups_partials.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, pu64, sz, ps]
    l.lwkzg_recover_cells_and_kzg_proofs.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, sz, ps]
    l.lwkzg_recover_cells_and_kzg_proofs_batch.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, sz, sz, ps, C.POINTER(sz)]
    l.lwkzg_recover_cells_and_kzg_proofs_batch_device.argtypes = [vp, vp, pu64, vp, sz, sz, ps, vp, vp]
    l.lwkzg_compute_cells_and_kzg_proofs_columns.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, pu64, sz, ps, C.POINTER(sz)]
    l.lwkzg_compute_cells_and_kzg_proofs_columns_device.argtypes = [vp, vp, vp, sz, pu64, sz, ps, vp, vp]
    l.lwkzg_recover_cells_and_kzg_proofs_columns.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, sz, sz, pu64, sz, ps, C.POINTER(sz)]
    l.lwkzg_recover_cells_and_kzg_proofs_columns_device.argtypes = [vp, vp, pu64, vp, sz, sz, pu64, sz, ps, vp, vp]
    l.lwkzg_recover_cells_and_kzg_proofs_mixed.argtypes = [C.c_char_p, C.c_char_p, pu64, C.c_char_p, C.POINTER(sz), sz, ps, C.POINTER(sz)]
    l.lwkzg_recover_cells_and_kzg_proofs_mixed_device.argtypes = [vp, vp, pu64, vp, C.POINTER(sz), sz, ps, vp, vp]
    l.lwkzg_set_cell_proof_engine.argtypes = [ps, ci, ci, sz]
    l.lwkzg_cell_proof_engine.argtypes = [ps]
    l.lwkzg_fk20_table_bytes.argtypes = [ps]
    l.lwkzg_fk20_table_bytes.restype = sz
    l.lwkzg_fk20_chunk_blobs.argtypes = []
    l.lwkzg_fk20_chunk_blobs.restype = sz
    l.lwkzg_fk20_points.argtypes = [C.c_char_p, ci, C.c_char_p, ps]
    l.lwkzg_shard_range.argtypes = [sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]
    pvp, psz = C.POINTER(vp), C.POINTER(sz)
    l.lwkzg_multi_blob_to_kzg_commitment_batch_device.argtypes = [pvp, pvp, psz, vp, psz]
    l.lwkzg_multi_compute_blob_kzg_proof_batch_device.argtypes = [pvp, pvp, pvp, psz, vp, psz]
    l.lwkzg_multi_verify_blob_kzg_proof_batch_device.argtypes = [C.POINTER(C.c_bool), pvp, pvp, pvp, psz, vp]
    l.lwkzg_verify_shard_begin_device.argtypes = [C.POINTER(vp), C.c_char_p, vp, vp, vp, sz, ps, vp]
    l.lwkzg_commit_and_prove_batch_device.argtypes = [vp, vp, vp, sz, ps, vp, vp]
    l.lwkzg_verify_shard_begin.argtypes = [C.POINTER(vp), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, ps]
    l.lwkzg_verify_shard_partial.argtypes = [C.c_char_p, vp, C.c_char_p, sz, sz]
    l.lwkzg_verify_shard_free.argtypes = [vp]
    l.lwkzg_verify_shard_free.restype = None
    l.lwkzg_verify_shards_finish.argtypes = [C.POINTER(C.c_bool), C.c_char_p, sz, sz, ps]
    l.lwkzg_verifier_new.argtypes = [C.POINTER(vp), ps, sz]
    l.lwkzg_verifier_enqueue.argtypes = [vp, C.POINTER(VerifyResult), vp, vp, vp, sz, vp]
    l.lwkzg_verifier_enqueue_openings.argtypes = [vp, C.POINTER(VerifyResult), vp, vp, vp, vp, sz, vp]
    l.lwkzg_verifier_pending.argtypes = [vp]
    l.lwkzg_verifier_wait.argtypes = [vp]
    l.lwkzg_verifier_free.argtypes = [vp]
    l.lwkzg_verifier_free.restype = None
    l.lwkzg_verifier_host_steps.argtypes = [C.POINTER(VerifyResult), C.c_char_p, sz, C.c_uint32, C.c_char_p, C.c_char_p, ps, ci]
    pu32 = C.POINTER(C.c_uint32)
    l.lwkzg_cell_verifier_new.argtypes = [C.POINTER(vp), ps, sz]
    l.lwkzg_cell_verifier_enqueue.argtypes = [vp, C.POINTER(CellVerifyResult), vp, vp, vp, vp, sz, vp]
    l.lwkzg_cell_verifier_pending.argtypes = [vp]
    l.lwkzg_cell_verifier_wait.argtypes = [vp]
    l.lwkzg_cell_verifier_free.argtypes = [vp]
    l.lwkzg_cell_verifier_free.restype = None
    l.lwkzg_cell_verifier_host_steps.argtypes = [C.POINTER(CellVerifyResult), C.c_char_p, sz, C.c_char_p, sz, C.c_uint32, pi32, pu32,
                                                 C.c_char_p, C.c_char_p, ps, ci]
    l.lwkzg_cell_group_device.argtypes = [pu32, pu32, C.c_char_p, pu32, pu32, pu32, pu32, pu32, pu32, vp, vp, sz, C.c_uint64, C.c_uint32, vp]
    l.lwkzg_cell_verifier_new_groups.argtypes = [C.POINTER(vp), ps, sz, sz]
    l.lwkzg_cell_verifier_enqueue_groups.argtypes = [vp, C.POINTER(CellVerifyResult), pu8, pi32, C.c_char_p, vp, vp, vp, vp, sz, pu64, sz, vp]
    l.lwkzg_cell_group_segmented_device.argtypes = [pu32, pu32, C.c_char_p, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu32, vp, vp,
                                                    sz, pu64, sz, C.c_uint64, C.c_uint32, vp]
    l.lwkzg_cell_verifier_groups_host_steps.argtypes = [C.POINTER(CellVerifyResult), pu8, pi32, C.c_char_p, pu64, sz, sz, pu32, pu32, pi32,
                                                        pu32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, ps, C.c_int]
    l.lwkzg_cell_verifier_new_blobs.argtypes = [C.POINTER(vp), ps, sz, sz]
    l.lwkzg_cell_verifier_enqueue_blobs.argtypes = [vp, C.POINTER(CellVerifyResult), vp, vp, vp, sz, vp]
    l.lwkzg_cell_verifier_enqueue_blobs_groups.argtypes = [vp, C.POINTER(CellVerifyResult), pu8, pi32, C.c_char_p, vp, vp, vp, sz, pu64, sz, vp]
    l.lwkzg_blob_group_device.argtypes = [pu32, pu32, C.c_char_p, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu32, pu64, vp, sz, pu64,
                                          sz, C.c_uint64, C.c_uint32, vp]
    l.lwkzg_release_context.argtypes = [ps]
    l.lwkzg_reserve.argtypes = [ps, sz]
    l.lwkzg_reserve_streams.argtypes = [ps, sz, ci]
    l.lwkzg_enable_direct_table.argtypes = [ps, ci]
    l.lwkzg_direct_table_bits.argtypes = [ps]
    l.lwkzg_direct_table_forms.argtypes = [ps]
    l.lwkzg_enable_direct_table_forms.argtypes = [ps, ci, ci]
    l.lwkzg_direct_num_windows.argtypes = [ci]
    l.lwkzg_direct_row_bytes.argtypes = [ps]
    l.lwkzg_g1_lincomb_setup_device.argtypes = [vp, vp, sz, ps, vp]
    l.lwkzg_fr_ntt4096_device.argtypes = [vp, vp, sz, ci, ps, vp]
    l.lwkzg_setup_image_bytes.restype = sz
    l.lwkzg_setup_export_device.argtypes = [ps, vp, vp]
    l.lwkzg_setup_import_device.argtypes = [ps, vp]
    l.lwkzg_load_trusted_setup_lagrange.argtypes = [ps, C.c_char_p, sz, C.c_char_p, sz]
    l.lwkzg_load_trusted_setup_ckzg.argtypes = [ps, C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, sz, C.c_uint64]
    l.lwkzg_load_trusted_setup_file_ckzg.argtypes = [ps, vp]
    l.lwkzg_setup_g1_lagrange.argtypes = [C.c_char_p, ps]
    l.lwkzg_trusted_setup_check.argtypes = [C.POINTER(C.c_bool), ps]
    l.lwkzg_set_device.argtypes = [ci]
    l.lwkzg_version.restype = C.c_char_p
    l.lwkzg_last_error.restype = C.c_char_p
    l.lwkzg_profile_enable.argtypes = [ci]
    l.lwkzg_profile_enable.restype = None
    l.lwkzg_profile_reset.restype = None
    l.lwkzg_profile_report.argtypes = [C.c_char_p, sz]
    l.lwkzg_profile_report.restype = sz
    l.lwkzg_profile_sources.argtypes = [C.c_char_p, sz]
    l.lwkzg_profile_sources.restype = sz
    l.lwkzg_pairing_product_is_one.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, sz]
    l.lwkzg_challenge_digests_host.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz]
    l.lwkzg_challenge_digests_host_mode.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, ci]
    l.lwkzg_batch_challenge_host.argtypes = [C.c_char_p, C.c_char_p, sz, ci]
    l.lwkzg_g1_msm_tiled_device.argtypes = [vp, vp, sz, ps, vp]
    l.lwkzg_g1_sum_compressed.argtypes = [C.c_char_p, C.c_char_p, sz]
    pi = C.POINTER(C.c_int)
    l.lwkzg_multi_load.argtypes = [C.POINTER(vp), C.c_char_p, sz, C.c_char_p, sz, pi, sz]
    l.lwkzg_multi_load_file.argtypes = [C.POINTER(vp), vp, pi, sz]
    l.lwkzg_multi_free.argtypes = [vp]
    l.lwkzg_multi_free.restype = None
    l.lwkzg_multi_device_count.argtypes = [vp]
    l.lwkzg_multi_device_count.restype = sz
    l.lwkzg_multi_device.argtypes = [vp, sz]
    l.lwkzg_multi_settings.argtypes = [vp, sz]
    l.lwkzg_multi_settings.restype = ps
    l.lwkzg_multi_set_mode.argtypes = [vp, ci]
    l.lwkzg_multi_enable_direct_table.argtypes = [vp, ci]
    l.lwkzg_multi_blob_to_kzg_commitment_batch.argtypes = [C.c_char_p, C.c_char_p, sz, vp, C.POINTER(sz)]
    l.lwkzg_multi_compute_blob_kzg_proof_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, vp, C.POINTER(sz)]
    l.lwkzg_multi_compute_kzg_proof_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, vp, C.POINTER(sz)]
    l.lwkzg_multi_verify_blob_kzg_proof_batch.argtypes = [C.POINTER(C.c_bool), C.c_char_p, C.c_char_p, C.c_char_p, sz, vp]
    l.lwkzg_multi_g1_msm_tiled.argtypes = [C.c_char_p, C.c_char_p, sz, vp]
    _lib = l
    return l


class KzgError(RuntimeError):
    def __init__(self, fn, rc):
        self.rc = rc
        msg = lib().lwkzg_last_error().decode(errors="replace")
        super().__init__("%s returned %s%s" % (fn, {1: "C_KZG_BADARGS", 2: "C_KZG_ERROR", 3: "C_KZG_MALLOC"}.get(rc, rc),
                                               (": " + msg) if msg else ""))


def _check(fn, rc):
    if rc != C_KZG_OK:
        raise KzgError(fn, rc)


_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]


def direct_table_bytes(window_bits, row_bytes=112):
    """HBM footprint of the direct table of that width with packed (112-byte) or line-aligned (128-byte) rows."""
    nw = lib().lwkzg_direct_num_windows(window_bits)
    if nw == 0:
        return 0
    top = 255 - window_bits * (nw - 1)
    return ((nw - 1) * 4096 * (1 << (window_bits - 1)) + 4096 * (1 << top)) * row_bytes


def shard_range(n_items, parts, k):
    """(first, count) of part k: the library's one shard rule (lwkzg_shard_range; csrc/multi.hip and dist.py both go through it)"""
    first, count = C.c_size_t(0), C.c_size_t(0)
    _check("lwkzg_shard_range", lib().lwkzg_shard_range(n_items, parts, k, C.byref(first), C.byref(count)))
    return first.value, count.value


def set_mode(mode):
    return lib().lwkzg_set_mode(mode)


def get_mode():
    return lib().lwkzg_get_mode()


def last_proof_schedule():
    """the schedule (csrc/plan.h: ProofSchedule) the last device-resident blob-proof call of this process took; -1 before the first"""
    return int(lib().lwkzg_last_proof_schedule())


def knob_report():
    """the environment knobs in effect for this process (lwkzg_knob_report; csrc/knobs.h reads them once, in one place)"""
    n = lib().lwkzg_knob_report(None, 0)
    buf = C.create_string_buffer(n)
    lib().lwkzg_knob_report(buf, n)
    return json.loads(buf.value.decode())


def clock_probe_mhz():
    """the shader clock the current device holds under a short dense multiply-add stream (lwkzg_clock_probe_mhz)"""
    mhz = C.c_double(0.0)
    lib().lwkzg_clock_probe_mhz.argtypes = [C.POINTER(C.c_double)]
    _check("lwkzg_clock_probe_mhz", lib().lwkzg_clock_probe_mhz(C.byref(mhz)))
    return mhz.value


def runtime_init():
    """first use of the HIP runtime by this process (device context, code object load): timed apart from the first real call"""
    if lib().lwkzg_runtime_init() != 0:
        raise KzgError("lwkzg_runtime_init", C_KZG_ERROR)


def set_device(ordinal):
    if lib().lwkzg_set_device(ordinal) != 0:
        raise KzgError("lwkzg_set_device", C_KZG_ERROR)


class TrustedSetup:
    """A loaded KZGSettings. Mirrors load_trusted_setup* / free_trusted_setup."""

    def __init__(self):
        self.s = KZGSettings()
        self._loaded = False

    @classmethod
    def from_file(cls, path):
        """load_trusted_setup_file(KZGSettings*, FILE*), /root/reference/src/lib.rs:779."""
        self = cls()
        fp = _libc.fopen(os.fsencode(path), b"r")
        if not fp:
            raise FileNotFoundError(path)
        try:
            _check("load_trusted_setup_file", lib().load_trusted_setup_file(C.byref(self.s), fp))
        finally:
            _libc.fclose(fp)
        self._loaded = True
        return self

    @classmethod
    def from_bytes(cls, g1_bytes, g2_bytes):
        """load_trusted_setup(out, g1_bytes, n1, g2_bytes, n2), /root/reference/src/lib.rs:709."""
        self = cls()
        _check("load_trusted_setup", lib().load_trusted_setup(C.byref(self.s), g1_bytes, len(g1_bytes) // 48,
                                                              g2_bytes, len(g2_bytes) // 96))
        self._loaded = True
        return self

    @classmethod
    def from_lagrange_bytes(cls, g1_lagrange_bytes, g2_bytes):
        """c-kzg-4844 1.x's load_trusted_setup (lwkzg_load_trusted_setup_lagrange): 4096 LAGRANGE G1 points, natural order, and 65 G2
        points; the monomial points are derived on the device. The settings answer in c-kzg mode."""
        self = cls()
        _check("lwkzg_load_trusted_setup_lagrange", lib().lwkzg_load_trusted_setup_lagrange(
            C.byref(self.s), g1_lagrange_bytes, len(g1_lagrange_bytes) // 48, g2_bytes, len(g2_bytes) // 96))
        self._loaded = True
        return self

    @classmethod
    def from_ckzg_bytes(cls, g1_monomial_bytes, g1_lagrange_bytes, g2_monomial_bytes, precompute=0):
        """c-kzg-4844 2.x's load_trusted_setup, its argument order (lwkzg_load_trusted_setup_ckzg): both G1 sections are validated and
        held against each other. The settings answer in c-kzg mode."""
        self = cls()
        _check("lwkzg_load_trusted_setup_ckzg", lib().lwkzg_load_trusted_setup_ckzg(
            C.byref(self.s), g1_monomial_bytes, len(g1_monomial_bytes) // 48, g1_lagrange_bytes, len(g1_lagrange_bytes) // 48,
            g2_monomial_bytes, len(g2_monomial_bytes) // 96, precompute))
        self._loaded = True
        return self

    @classmethod
    def from_ckzg_file(cls, path):
        """a c-kzg-4844 trusted_setup.txt of either layout (lwkzg_load_trusted_setup_file_ckzg); from_file is for the reference's
        monomial text"""
        self = cls()
        fp = _libc.fopen(os.fsencode(path), b"r")
        if not fp:
            raise FileNotFoundError(path)
        try:
            _check("lwkzg_load_trusted_setup_file_ckzg", lib().lwkzg_load_trusted_setup_file_ckzg(C.byref(self.s), fp))
        finally:
            _libc.fclose(fp)
        self._loaded = True
        return self

    @classmethod
    def from_device_image(cls, image_dev_ptr):
        self = cls()
        _check("lwkzg_setup_import_device", lib().lwkzg_setup_import_device(C.byref(self.s), image_dev_ptr))
        self._loaded = True
        return self

    def export_device_image(self, image_dev_ptr, stream=None):
        _check("lwkzg_setup_export_device", lib().lwkzg_setup_export_device(C.byref(self.s), image_dev_ptr, stream))

    def g1_values_bytes(self):
        return C.string_at(self.s.g1_values, 4096 * 144)

    def g2_values_bytes(self):
        return C.string_at(self.s.g2_values, 65 * 288)

    def g1_lagrange(self):
        """the Lagrange form of the setup as a c-kzg 1.x file holds it: 4096 x 48 bytes compressed, natural order (derived if absent)"""
        out = C.create_string_buffer(4096 * 48)
        _check("lwkzg_setup_g1_lagrange", lib().lwkzg_setup_g1_lagrange(out, self.ref()))
        return out.raw

    def check(self):
        """is this a powers-of-tau setup? (lwkzg_trusted_setup_check: False for a Lagrange file loaded as monomial, among others)"""
        ok = C.c_bool(False)
        _check("lwkzg_trusted_setup_check", lib().lwkzg_trusted_setup_check(C.byref(ok), self.ref()))
        return bool(ok.value)

    def fft_settings(self):
        return FFTSettings.from_address(self.s.fs)

    def ref(self):
        return C.byref(self.s)

    def reserve(self, n, caller_streams=1):
        _check("lwkzg_reserve_streams", lib().lwkzg_reserve_streams(self.ref(), n, caller_streams))

    def set_mode(self, mode):
        """This settings object's own semantics (MODE_REFERENCE / MODE_CKZG / MODE_ETH; -1 = follow the process-wide default)."""
        prev = lib().lwkzg_settings_set_mode(self.ref(), mode)
        if prev < 0:
            raise KzgError("lwkzg_settings_set_mode", C_KZG_BADARGS)
        return prev

    def get_mode(self):
        return lib().lwkzg_settings_get_mode(self.ref())

    def enable_direct_table(self, window_bits):
        """Select the direct-table MSM of that width (10 .. 16) or the bucket engine (0); raises KzgError(C_KZG_MALLOC) if
        the table does not fit."""
        _check("lwkzg_enable_direct_table", lib().lwkzg_enable_direct_table(self.ref(), window_bits))

    def direct_table_bits(self):
        return lib().lwkzg_direct_table_bits(self.ref())

    def enable_direct_table_forms(self, window_bits, forms):
        """forms: 1 = monomial only, 2 = Lagrange only, 3 = both"""
        _check("lwkzg_enable_direct_table_forms", lib().lwkzg_enable_direct_table_forms(self.ref(), window_bits, forms))

    def direct_table_forms(self):
        """bit 0: a monomial-form direct table is live, bit 1: a Lagrange-form one (c-kzg commitments without the transform)"""
        return lib().lwkzg_direct_table_forms(self.ref())

    def set_cell_proof_engine(self, engine, window_bits=0, min_blobs=0):
        """The engine behind the cell proofs of the compute and recover calls: CELL_PROOFS_MSM (the default) or CELL_PROOFS_FK20, which
        builds the settings' FK20 table (window_bits 0 = the default width) and serves calls of at least min_blobs blobs (0 = the
        library's threshold); raises KzgError(C_KZG_MALLOC) if the table does not fit, the engine staying as it was."""
        _check("lwkzg_set_cell_proof_engine", lib().lwkzg_set_cell_proof_engine(self.ref(), engine, window_bits, min_blobs))

    def cell_proof_engine(self):
        return lib().lwkzg_cell_proof_engine(self.ref())

    def fk20_table_bytes(self):
        return lib().lwkzg_fk20_table_bytes(self.ref())

    def fk20_points(self, what, blob=None):
        """test hook (lwkzg_fk20_points): what 0 = the 8192 bases, 1 = E[0..127] of the blob, 2 = h_0 .. h_63; a list of 97-byte
        records flag | x | y"""
        n = {0: 8192, 1: 128, 2: 64}[what]
        out = C.create_string_buffer(n * FK20_POINT_BYTES)
        _check("lwkzg_fk20_points", lib().lwkzg_fk20_points(out, what, blob, self.ref()))
        return [out.raw[FK20_POINT_BYTES * i:FK20_POINT_BYTES * (i + 1)] for i in range(n)]

    def direct_row_bytes(self):
        """128 = table rows aligned to 128-byte lines, 112 = packed, 0 = bucket engine."""
        return lib().lwkzg_direct_row_bytes(self.ref())

    def timing_report(self):
        """where the milliseconds of the load and of the last table build went (lwkzg_timing_report)"""
        n = lib().lwkzg_timing_report(self.ref(), None, 0)
        buf = C.create_string_buffer(n)
        lib().lwkzg_timing_report(self.ref(), buf, n)
        return json.loads(buf.value.decode())

    def free(self):
        if self._loaded:
            lib().free_trusted_setup(C.byref(self.s))
            self._loaded = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceSettings:
    """the k-th device's KZGSettings of a MultiSetup, usable wherever a TrustedSetup is (the MultiSetup owns it)"""

    def __init__(self, ptr):
        self._p = ptr

    def ref(self):
        return self._p


class MultiSetup:
    """One process, several GPUs (lwkzg_multi_*, csrc/multi.hip): the setup loaded once and delivered device-to-device, batches cut
    into contiguous shards, one host thread per device, no reduction. `devices` may name a device more than once."""

    def __init__(self, h):
        self.h = h

    @classmethod
    def from_file(cls, path, devices):
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        fp = _libc.fopen(os.fsencode(path), b"r")
        if not fp:
            raise FileNotFoundError(path)
        try:
            _check("lwkzg_multi_load_file", lib().lwkzg_multi_load_file(C.byref(h), fp, arr, len(devices)))
        finally:
            _libc.fclose(fp)
        return cls(h)

    @classmethod
    def from_bytes(cls, g1_bytes, g2_bytes, devices):
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        _check("lwkzg_multi_load", lib().lwkzg_multi_load(C.byref(h), g1_bytes, len(g1_bytes) // 48, g2_bytes, len(g2_bytes) // 96, arr, len(devices)))
        return cls(h)

    def device_count(self):
        return lib().lwkzg_multi_device_count(self.h)

    def devices(self):
        return [lib().lwkzg_multi_device(self.h, k) for k in range(self.device_count())]

    def settings(self, k):
        p = lib().lwkzg_multi_settings(self.h, k)
        if not p:
            raise IndexError(k)
        return _DeviceSettings(p)

    def set_mode(self, mode):
        _check("lwkzg_multi_set_mode", lib().lwkzg_multi_set_mode(self.h, mode))

    def enable_direct_table(self, window_bits):
        _check("lwkzg_multi_enable_direct_table", lib().lwkzg_multi_enable_direct_table(self.h, window_bits))

    def blob_to_kzg_commitment_batch(self, blobs):
        n = len(blobs) // BYTES_PER_BLOB
        assert len(blobs) == n * BYTES_PER_BLOB
        out = C.create_string_buffer(48 * max(n, 1))
        self.first_bad = C.c_size_t(0)
        _check("lwkzg_multi_blob_to_kzg_commitment_batch", lib().lwkzg_multi_blob_to_kzg_commitment_batch(out, blobs, n, self.h, C.byref(self.first_bad)))
        raw = out.raw      # (ONE copy of the buffer: `.raw` inside the comprehension copied all 48 n bytes per element -- 6 ms of Python per 4096 results)
        return [raw[48 * i:48 * i + 48] for i in range(n)]

    def compute_blob_kzg_proof_batch(self, blobs, commitments):
        n = len(blobs) // BYTES_PER_BLOB
        assert len(blobs) == n * BYTES_PER_BLOB and len(commitments) == 48 * n
        out = C.create_string_buffer(48 * max(n, 1))
        self.first_bad = C.c_size_t(0)
        _check("lwkzg_multi_compute_blob_kzg_proof_batch",
               lib().lwkzg_multi_compute_blob_kzg_proof_batch(out, blobs, commitments, n, self.h, C.byref(self.first_bad)))
        raw = out.raw      # (ONE copy of the buffer: `.raw` inside the comprehension copied all 48 n bytes per element -- 6 ms of Python per 4096 results)
        return [raw[48 * i:48 * i + 48] for i in range(n)]

    def compute_kzg_proof_batch(self, blobs, zs):
        n = len(blobs) // BYTES_PER_BLOB
        assert len(blobs) == n * BYTES_PER_BLOB and len(zs) == 32 * n
        out, ys = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(32 * max(n, 1))
        self.first_bad = C.c_size_t(0)
        _check("lwkzg_multi_compute_kzg_proof_batch",
               lib().lwkzg_multi_compute_kzg_proof_batch(out, ys, blobs, zs, n, self.h, C.byref(self.first_bad)))
        raw, yraw = out.raw, ys.raw
        return [(raw[48 * i:48 * i + 48], yraw[32 * i:32 * i + 32]) for i in range(n)]

    # ---- shards already in HBM: lists of per-device device pointers and counts (device k's shard on device k)
    @staticmethod
    def _ptrs(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def blob_to_kzg_commitment_batch_device(self, out_ptrs, blob_ptrs, counts):
        cnt = (C.c_size_t * len(counts))(*counts)
        self.first_bad = C.c_size_t(0)
        _check("lwkzg_multi_blob_to_kzg_commitment_batch_device",
               lib().lwkzg_multi_blob_to_kzg_commitment_batch_device(self._ptrs(out_ptrs), self._ptrs(blob_ptrs), cnt, self.h, C.byref(self.first_bad)))

    def compute_blob_kzg_proof_batch_device(self, out_ptrs, blob_ptrs, comm_ptrs, counts):
        cnt = (C.c_size_t * len(counts))(*counts)
        self.first_bad = C.c_size_t(0)
        _check("lwkzg_multi_compute_blob_kzg_proof_batch_device",
               lib().lwkzg_multi_compute_blob_kzg_proof_batch_device(self._ptrs(out_ptrs), self._ptrs(blob_ptrs), self._ptrs(comm_ptrs), cnt, self.h,
                                                                     C.byref(self.first_bad)))

    def verify_blob_kzg_proof_batch_device(self, blob_ptrs, comm_ptrs, proof_ptrs, counts):
        cnt = (C.c_size_t * len(counts))(*counts)
        ok = C.c_bool(False)
        _check("lwkzg_multi_verify_blob_kzg_proof_batch_device",
               lib().lwkzg_multi_verify_blob_kzg_proof_batch_device(C.byref(ok), self._ptrs(blob_ptrs), self._ptrs(comm_ptrs), self._ptrs(proof_ptrs), cnt,
                                                                    self.h))
        return bool(ok.value)

    def verify_blob_kzg_proof_batch(self, blobs, commitments, proofs, n):
        ok = C.c_bool(False)
        _check("lwkzg_multi_verify_blob_kzg_proof_batch",
               lib().lwkzg_multi_verify_blob_kzg_proof_batch(C.byref(ok), blobs, commitments, proofs, n, self.h))
        return bool(ok.value)

    def g1_msm_tiled(self, scalars_be):
        out = C.create_string_buffer(48)
        _check("lwkzg_multi_g1_msm_tiled", lib().lwkzg_multi_g1_msm_tiled(out, scalars_be, len(scalars_be) // 32, self.h))
        return out.raw

    def free(self):
        if self.h:
            lib().lwkzg_multi_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the reference's functions, same names and argument meaning ---------------------------------

def blob_to_kzg_commitment(blob, ts):
    assert len(blob) == BYTES_PER_BLOB
    out = C.create_string_buffer(48)
    _check("blob_to_kzg_commitment", lib().blob_to_kzg_commitment(out, blob, ts.ref()))
    return out.raw


def compute_kzg_proof(blob, z_bytes, ts):
    assert len(blob) == BYTES_PER_BLOB and len(z_bytes) == 32
    proof, y = C.create_string_buffer(48), C.create_string_buffer(32)
    _check("compute_kzg_proof", lib().compute_kzg_proof(proof, y, blob, z_bytes, ts.ref()))
    return proof.raw, y.raw


def compute_blob_kzg_proof(blob, commitment_bytes, ts):
    assert len(blob) == BYTES_PER_BLOB and len(commitment_bytes) == 48
    out = C.create_string_buffer(48)
    _check("compute_blob_kzg_proof", lib().compute_blob_kzg_proof(out, blob, commitment_bytes, ts.ref()))
    return out.raw


def verify_kzg_proof(commitment_bytes, z_bytes, y_bytes, proof_bytes, ts):
    ok = C.c_bool(False)
    _check("verify_kzg_proof", lib().verify_kzg_proof(C.byref(ok), commitment_bytes, z_bytes, y_bytes, proof_bytes, ts.ref()))
    return bool(ok.value)


def verify_blob_kzg_proof(blob, commitment_bytes, proof_bytes, ts):
    ok = C.c_bool(False)
    _check("verify_blob_kzg_proof", lib().verify_blob_kzg_proof(C.byref(ok), blob, commitment_bytes, proof_bytes, ts.ref()))
    return bool(ok.value)


def verify_blob_kzg_proof_batch(blobs, commitments_bytes, proofs_bytes, n, ts):
    ok = C.c_bool(False)
    _check("verify_blob_kzg_proof_batch",
           lib().verify_blob_kzg_proof_batch(C.byref(ok), blobs, commitments_bytes, proofs_bytes, n, ts.ref()))
    return bool(ok.value)


def verify_blob_kzg_proof_batch_device(blobs_ptr, comm_ptr, proofs_ptr, n, ts, stream=None):
    """verify_blob_kzg_proof_batch on DEVICE pointers (produced on `stream`); the verdict is a host bool, the call synchronous"""
    ok = C.c_bool(False)
    _check("lwkzg_verify_blob_kzg_proof_batch_device",
           lib().lwkzg_verify_blob_kzg_proof_batch_device(C.byref(ok), blobs_ptr, comm_ptr, proofs_ptr, n, ts.ref(), stream))
    return bool(ok.value)


def _each(fn, n, call):
    ok = (C.c_uint8 * max(n, 1))()
    rc = (C.c_int32 * max(n, 1))()
    _check(fn, call(ok, rc))
    return [(rc[i], bool(ok[i])) for i in range(n)]


def verify_blob_kzg_proof_each(blobs, commitments, proofs, ts):
    """n independent verify_blob_kzg_proof calls in one (lwkzg_verify_blob_kzg_proof_each): a list of (rc, ok), item i exactly what
    the single call on item i answers. Inputs: the concatenated blobs, commitments and proofs (bytes)."""
    n = len(commitments) // 48
    assert len(commitments) == 48 * n and len(proofs) == 48 * n and len(blobs) == BYTES_PER_BLOB * n
    return _each("lwkzg_verify_blob_kzg_proof_each", n,
                 lambda ok, rc: lib().lwkzg_verify_blob_kzg_proof_each(ok, rc, blobs, commitments, proofs, n, ts.ref()))


def verify_blob_kzg_proof_each_device(blobs_ptr, comm_ptr, proofs_ptr, n, ts, stream=None):
    """the same on DEVICE pointers (produced on `stream`); the verdicts come to the host, the call is synchronous"""
    return _each("lwkzg_verify_blob_kzg_proof_each_device", n,
                 lambda ok, rc: lib().lwkzg_verify_blob_kzg_proof_each_device(ok, rc, blobs_ptr, comm_ptr, proofs_ptr, n, ts.ref(), stream))


def verify_kzg_proof_each(commitments, zs, ys, proofs, ts):
    """n independent verify_kzg_proof calls in one (lwkzg_verify_kzg_proof_each): a list of (rc, ok)"""
    n = len(commitments) // 48
    assert len(commitments) == 48 * n and len(proofs) == 48 * n and len(zs) == 32 * n and len(ys) == 32 * n
    return _each("lwkzg_verify_kzg_proof_each", n,
                 lambda ok, rc: lib().lwkzg_verify_kzg_proof_each(ok, rc, commitments, zs, ys, proofs, n, ts.ref()))


def verify_kzg_proof_each_device(comm_ptr, zs_ptr, ys_ptr, proofs_ptr, n, ts, stream=None):
    """the same on DEVICE pointers (produced on `stream`); the verdicts come to the host, the call is synchronous"""
    return _each("lwkzg_verify_kzg_proof_each_device", n,
                 lambda ok, rc: lib().lwkzg_verify_kzg_proof_each_device(ok, rc, comm_ptr, zs_ptr, ys_ptr, proofs_ptr, n, ts.ref(), stream))


def verify_kzg_proof_batch(commitments, zs, ys, proofs, ts):
    """n openings (C_i, z_i, y_i, pi_i) with one pairing check (lwkzg_verify_kzg_proof_batch): the consensus specs'
    verify_kzg_proof_batch. Inputs: the concatenated commitments, zs, ys and proofs (bytes). Raises KzgError when an item is invalid."""
    n = len(commitments) // 48
    assert len(commitments) == 48 * n and len(proofs) == 48 * n and len(zs) == 32 * n and len(ys) == 32 * n
    ok = C.c_bool(False)
    _check("lwkzg_verify_kzg_proof_batch", lib().lwkzg_verify_kzg_proof_batch(C.byref(ok), commitments, zs, ys, proofs, n, ts.ref()))
    return bool(ok.value)


def verify_kzg_proof_batch_device(comm_ptr, zs_ptr, ys_ptr, proofs_ptr, n, ts, stream=None):
    """the same on DEVICE pointers (16-byte aligned, produced on `stream`); the verdict is a host bool, the call synchronous"""
    ok = C.c_bool(False)
    _check("lwkzg_verify_kzg_proof_batch_device",
           lib().lwkzg_verify_kzg_proof_batch_device(C.byref(ok), comm_ptr, zs_ptr, ys_ptr, proofs_ptr, n, ts.ref(), stream))
    return bool(ok.value)


def verify_kzg_proof_batch_partial(commitments, zs, ys, proofs, ts):
    """test hook: (r, partial) of the batch call up to its pairing -- r as batch_challenge_host writes it, the partial as
    VerifyShard.partial(records, n, 0) writes it"""
    n = len(commitments) // 48
    assert len(commitments) == 48 * n and len(proofs) == 48 * n and len(zs) == 32 * n and len(ys) == 32 * n
    r, partial = C.create_string_buffer(32), C.create_string_buffer(VERIFY_PARTIAL_BYTES)
    _check("lwkzg_verify_kzg_proof_batch_partial",
           lib().lwkzg_verify_kzg_proof_batch_partial(r, partial, commitments, zs, ys, proofs, n, ts.ref()))
    return r.raw, partial.raw


def _cells_split(cells_raw, proofs_raw, n):
    """n x 128 cells / proofs as returned by the library -> [(cells, proofs)] per blob, each a list of 128 bytes objects (or None)"""
    out = []
    for b in range(n):
        cs = None if cells_raw is None else [cells_raw[(128 * b + k) * BYTES_PER_CELL:(128 * b + k + 1) * BYTES_PER_CELL] for k in range(128)]
        ps = None if proofs_raw is None else [proofs_raw[(128 * b + k) * 48:(128 * b + k + 1) * 48] for k in range(128)]
        out.append((cs, ps))
    return out


def compute_cells_and_kzg_proofs(blob, ts, cells=True, proofs=True):
    """EIP-7594 compute_cells_and_kzg_proofs (lwkzg_compute_cells_and_kzg_proofs): (cells, proofs), 128 cells of 2048 bytes and
    128 compressed proofs, in the settings' mode; cells=False / proofs=False leave that output out (None)."""
    assert len(blob) == BYTES_PER_BLOB
    cb = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if cells else None
    pb = C.create_string_buffer(CELLS_PER_EXT_BLOB * 48) if proofs else None
    _check("lwkzg_compute_cells_and_kzg_proofs", lib().lwkzg_compute_cells_and_kzg_proofs(cb, pb, blob, ts.ref()))
    return _cells_split(cb.raw if cells else None, pb.raw if proofs else None, 1)[0]


def compute_cells_and_kzg_proofs_batch(blobs, ts, cells=True, proofs=True):
    """the same for n concatenated blobs in one call: a list of (cells, proofs) per blob"""
    n = len(blobs) // BYTES_PER_BLOB
    assert len(blobs) == n * BYTES_PER_BLOB
    cb = C.create_string_buffer(max(n, 1) * CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if cells else None
    pb = C.create_string_buffer(max(n, 1) * CELLS_PER_EXT_BLOB * 48) if proofs else None
    bad = C.c_size_t(0)
    _check("lwkzg_compute_cells_and_kzg_proofs_batch",
           lib().lwkzg_compute_cells_and_kzg_proofs_batch(cb, pb, blobs, n, ts.ref(), C.byref(bad)))
    return _cells_split(cb.raw if cells else None, pb.raw if proofs else None, n)


def compute_cells_and_kzg_proofs_batch_device(cells_ptr, proofs_ptr, blobs_ptr, n, ts, stream=None, status_ptr=None):
    """cells (n x 128 x 2048 bytes) and proofs (n x 128 x 48 bytes) of n device-resident blobs, asynchronous on `stream`; either output
    pointer may be None"""
    _check("lwkzg_compute_cells_and_kzg_proofs_batch_device",
           lib().lwkzg_compute_cells_and_kzg_proofs_batch_device(cells_ptr, proofs_ptr, blobs_ptr, n, ts.ref(), stream, status_ptr))


def _recover_args(cell_indices, cells, n):
    """the indices as a C array and the cells (a list per blob or concatenated bytes, n x num_cells x 2048, blob-major) as bytes"""
    num = len(cell_indices)
    ce = cells if isinstance(cells, (bytes, bytearray)) else b"".join(cells)
    if len(ce) != n * num * BYTES_PER_CELL:
        raise ValueError("cells must hold one cell per index and blob")
    return (C.c_uint64 * max(num, 1))(*cell_indices), bytes(ce), num


def recover_cells_and_kzg_proofs(cell_indices, cells, ts, cells_out=True, proofs=True):
    """EIP-7594 recover_cells_and_kzg_proofs (lwkzg_recover_cells_and_kzg_proofs): all 128 cells and 128 proofs of a blob from 64 .. 128
    of its cells (cells[i] = cell cell_indices[i], indices strictly ascending), in the settings' mode; (cells, proofs) as
    compute_cells_and_kzg_proofs returns them. cells_out=False / proofs=False leave that output out (None)."""
    idx, ce, num = _recover_args(cell_indices, cells, 1)
    cb = C.create_string_buffer(CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if cells_out else None
    pb = C.create_string_buffer(CELLS_PER_EXT_BLOB * 48) if proofs else None
    _check("lwkzg_recover_cells_and_kzg_proofs", lib().lwkzg_recover_cells_and_kzg_proofs(cb, pb, idx, ce, num, ts.ref()))
    return _cells_split(cb.raw if cells_out else None, pb.raw if proofs else None, 1)[0]


def recover_cells_and_kzg_proofs_batch(cell_indices, cells, n, ts, cells_out=True, proofs=True):
    """the same for n blobs that share one index set (cells: n x len(cell_indices) cells, blob-major): a list of (cells, proofs) per blob"""
    idx, ce, num = _recover_args(cell_indices, cells, n)
    cb = C.create_string_buffer(max(n, 1) * CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if cells_out else None
    pb = C.create_string_buffer(max(n, 1) * CELLS_PER_EXT_BLOB * 48) if proofs else None
    bad = C.c_size_t(0)
    _check("lwkzg_recover_cells_and_kzg_proofs_batch",
           lib().lwkzg_recover_cells_and_kzg_proofs_batch(cb, pb, idx, ce, num, n, ts.ref(), C.byref(bad)))
    return _cells_split(cb.raw if cells_out else None, pb.raw if proofs else None, n)


def recover_cells_and_kzg_proofs_batch_device(cells_out_ptr, proofs_ptr, cell_indices, cells_ptr, n, ts, stream=None, status_ptr=None):
    """cells (n x 128 x 2048 bytes) and proofs (n x 128 x 48 bytes) of n blobs from their device-resident cells (n x len(cell_indices) x
    2048 bytes, blob-major; cell_indices a host list), asynchronous on `stream`; either output pointer may be None"""
    num = len(cell_indices)
    idx = (C.c_uint64 * max(num, 1))(*cell_indices)
    _check("lwkzg_recover_cells_and_kzg_proofs_batch_device",
           lib().lwkzg_recover_cells_and_kzg_proofs_batch_device(cells_out_ptr, proofs_ptr, idx, cells_ptr, num, n, ts.ref(), stream, status_ptr))


def _columns_split(cells_raw, proofs_raw, n, c):
    """n x c cells / proofs as a column call returns them -> [(cells, proofs)] per blob, each a list of c bytes objects (or None)"""
    out = []
    for b in range(n):
        cs = None if cells_raw is None else [cells_raw[(c * b + i) * BYTES_PER_CELL:(c * b + i + 1) * BYTES_PER_CELL] for i in range(c)]
        ps = None if proofs_raw is None else [proofs_raw[(c * b + i) * 48:(c * b + i + 1) * 48] for i in range(c)]
        out.append((cs, ps))
    return out


def compute_cells_and_kzg_proofs_columns(blobs, columns, ts, cells=True, proofs=True):
    """the cells and proofs of the chosen columns alone (lwkzg_compute_cells_and_kzg_proofs_columns; columns: 1 .. 128 strictly ascending
    indices below 128) of n concatenated blobs: a list of (cells, proofs) per blob, each len(columns) long and equal to entries
    columns[i] of what compute_cells_and_kzg_proofs_batch returns"""
    n, c = len(blobs) // BYTES_PER_BLOB, len(columns)
    assert len(blobs) == n * BYTES_PER_BLOB
    cb = C.create_string_buffer(max(n * c, 1) * BYTES_PER_CELL) if cells else None
    pb = C.create_string_buffer(max(n * c, 1) * 48) if proofs else None
    bad = C.c_size_t(0)
    _check("lwkzg_compute_cells_and_kzg_proofs_columns",
           lib().lwkzg_compute_cells_and_kzg_proofs_columns(cb, pb, blobs, n, (C.c_uint64 * max(c, 1))(*columns), c, ts.ref(), C.byref(bad)))
    return _columns_split(cb.raw if cells else None, pb.raw if proofs else None, n, c)


def compute_cells_and_kzg_proofs_columns_device(cells_ptr, proofs_ptr, blobs_ptr, n, columns, ts, stream=None, status_ptr=None):
    """cells (n x len(columns) x 2048 bytes) and proofs (n x len(columns) x 48 bytes) of the chosen columns of n device-resident blobs
    (columns a host list), asynchronous on `stream`; either output pointer may be None"""
    c = len(columns)
    _check("lwkzg_compute_cells_and_kzg_proofs_columns_device",
           lib().lwkzg_compute_cells_and_kzg_proofs_columns_device(cells_ptr, proofs_ptr, blobs_ptr, n, (C.c_uint64 * max(c, 1))(*columns), c,
                                                                   ts.ref(), stream, status_ptr))


def recover_cells_and_kzg_proofs_columns(cell_indices, cells, n, columns, ts, cells_out=True, proofs=True):
    """the chosen columns alone of n blobs recovered through one index set (lwkzg_recover_cells_and_kzg_proofs_columns): a list of
    (cells, proofs) per blob, each len(columns) long and equal to entries columns[i] of what recover_cells_and_kzg_proofs_batch returns"""
    idx, ce, num = _recover_args(cell_indices, cells, n)
    c = len(columns)
    cb = C.create_string_buffer(max(n * c, 1) * BYTES_PER_CELL) if cells_out else None
    pb = C.create_string_buffer(max(n * c, 1) * 48) if proofs else None
    bad = C.c_size_t(0)
    _check("lwkzg_recover_cells_and_kzg_proofs_columns",
           lib().lwkzg_recover_cells_and_kzg_proofs_columns(cb, pb, idx, ce, num, n, (C.c_uint64 * max(c, 1))(*columns), c, ts.ref(),
                                                            C.byref(bad)))
    return _columns_split(cb.raw if cells_out else None, pb.raw if proofs else None, n, c)


def recover_cells_and_kzg_proofs_columns_device(cells_out_ptr, proofs_ptr, cell_indices, cells_ptr, n, columns, ts, stream=None,
                                                status_ptr=None):
    """cells (n x len(columns) x 2048 bytes) and proofs (n x len(columns) x 48 bytes) of the chosen columns of n blobs from their
    device-resident cells (n x len(cell_indices) x 2048 bytes, blob-major; both lists stay on the host), asynchronous on `stream`;
    either output pointer may be None"""
    num, c = len(cell_indices), len(columns)
    _check("lwkzg_recover_cells_and_kzg_proofs_columns_device",
           lib().lwkzg_recover_cells_and_kzg_proofs_columns_device(cells_out_ptr, proofs_ptr, (C.c_uint64 * max(num, 1))(*cell_indices),
                                                                   cells_ptr, num, n, (C.c_uint64 * max(c, 1))(*columns), c, ts.ref(),
                                                                   stream, status_ptr))


def _mixed_lists(index_lists):
    """one index list per blob -> the lists one after the other and the counts, as C arrays"""
    flat = [k for lst in index_lists for k in lst]
    return (C.c_uint64 * max(len(flat), 1))(*flat), (C.c_size_t * max(len(index_lists), 1))(*[len(lst) for lst in index_lists]), len(flat)


def recover_cells_and_kzg_proofs_mixed(index_lists, cells_per_blob, ts, cells_out=True, proofs=True):
    """n blobs, each through an index set of its own, in one call (lwkzg_recover_cells_and_kzg_proofs_mixed): index_lists[b] is blob b's
    list of 64 .. 128 ascending indices and cells_per_blob[b] its cells (a list of cells or their concatenation), one per index. A list
    of (cells, proofs) per blob, each what recover_cells_and_kzg_proofs gives for that blob alone."""
    n = len(index_lists)
    idx, num, total = _mixed_lists(index_lists)
    ce = b"".join(c if isinstance(c, (bytes, bytearray)) else b"".join(c) for c in cells_per_blob)
    if len(cells_per_blob) != n or len(ce) != total * BYTES_PER_CELL:
        raise ValueError("cells_per_blob must hold one cell per index of every blob")
    cb = C.create_string_buffer(max(n, 1) * CELLS_PER_EXT_BLOB * BYTES_PER_CELL) if cells_out else None
    pb = C.create_string_buffer(max(n, 1) * CELLS_PER_EXT_BLOB * 48) if proofs else None
    bad = C.c_size_t(0)
    _check("lwkzg_recover_cells_and_kzg_proofs_mixed",
           lib().lwkzg_recover_cells_and_kzg_proofs_mixed(cb, pb, idx, bytes(ce), num, n, ts.ref(), C.byref(bad)))
    return _cells_split(cb.raw if cells_out else None, pb.raw if proofs else None, n)


def recover_cells_and_kzg_proofs_mixed_device(cells_out_ptr, proofs_ptr, index_lists, cells_ptr, ts, stream=None, status_ptr=None):
    """cells (n x 128 x 2048 bytes) and proofs (n x 128 x 48 bytes) of the n = len(index_lists) blobs from their device-resident cells
    (the blobs' cells one after the other, blob b's in the order of index_lists[b]; the lists stay on the host), asynchronous on `stream`;
    either output pointer may be None"""
    idx, num, _ = _mixed_lists(index_lists)
    _check("lwkzg_recover_cells_and_kzg_proofs_mixed_device",
           lib().lwkzg_recover_cells_and_kzg_proofs_mixed_device(cells_out_ptr, proofs_ptr, idx, cells_ptr, num, len(index_lists), ts.ref(),
                                                                 stream, status_ptr))


CELL_VERIFY_PARTIAL_BYTES = 32 + 4 * 97


def _cell_items(commitments, cell_indices, cells, proofs):
    """lists (or concatenated bytes) of n commitments, cells and proofs and n indices -> the C arguments"""
    n = len(cell_indices)
    cm = commitments if isinstance(commitments, (bytes, bytearray)) else b"".join(commitments)
    ce = cells if isinstance(cells, (bytes, bytearray)) else b"".join(cells)
    pf = proofs if isinstance(proofs, (bytes, bytearray)) else b"".join(proofs)
    if len(cm) != 48 * n or len(ce) != BYTES_PER_CELL * n or len(pf) != 48 * n:
        raise ValueError("commitments, cells and proofs must hold one entry per cell index")
    return bytes(cm), (C.c_uint64 * max(n, 1))(*cell_indices), bytes(ce), bytes(pf), n


def verify_cell_kzg_proof_batch(commitments, cell_indices, cells, proofs, ts):
    """EIP-7594 verify_cell_kzg_proof_batch (lwkzg_verify_cell_kzg_proof_batch): do the cells belong to the commitments? Item i is
    (commitments[i], cell_indices[i], cells[i], proofs[i]); cells in the settings' mode's byte order. The empty batch answers True."""
    cm, idx, ce, pf, n = _cell_items(commitments, cell_indices, cells, proofs)
    ok = C.c_bool(False)
    _check("lwkzg_verify_cell_kzg_proof_batch", lib().lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), cm, idx, ce, pf, n, ts.ref()))
    return bool(ok.value)


def verify_cell_kzg_proof_batch_device(comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, ts, stream=None):
    """the same on DEVICE pointers (48 n commitment bytes, n uint64 indices, 2048 n cell bytes, 48 n proof bytes, produced on
    `stream`); the verdict is a host bool, the call synchronous"""
    ok = C.c_bool(False)
    _check("lwkzg_verify_cell_kzg_proof_batch_device",
           lib().lwkzg_verify_cell_kzg_proof_batch_device(C.byref(ok), comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, ts.ref(), stream))
    return bool(ok.value)


def cell_verify_partials(commitments, cell_indices, cells, proofs, ts):
    """r (32 bytes, the mode's byte order) and the four sums P, RLC, RLI, RLP of the check (97 bytes each: flag | x | y), by the
    verdict call's own code path up to the pairing"""
    cm, idx, ce, pf, n = _cell_items(commitments, cell_indices, cells, proofs)
    out = C.create_string_buffer(CELL_VERIFY_PARTIAL_BYTES)
    _check("lwkzg_cell_verify_partials", lib().lwkzg_cell_verify_partials(out, cm, idx, ce, pf, n, ts.ref()))
    return out.raw


CELL_EACH_POINT_BYTES = 97
CELL_PROOFS_MSM, CELL_PROOFS_FK20 = 0, 1     # lwkzg_set_cell_proof_engine
FK20_POINT_BYTES = 97
FK20_DEFAULT_MIN_BLOBS = 64                   # LWKZG_FK20_DEFAULT_MIN_BLOBS: the measured crossing of profiles/fk20_timing.txt


def fk20_chunk_blobs():
    """blobs per chunk of the FK20 cell proof engine"""
    return lib().lwkzg_fk20_chunk_blobs()


def verify_cell_kzg_proof_each(commitments, cell_indices, cells, proofs, ts):
    """n independent one-item verify_cell_kzg_proof_batch calls in one (lwkzg_verify_cell_kzg_proof_each): a list of (rc, ok), item i
    exactly what the batch call on item i alone answers. Arguments as verify_cell_kzg_proof_batch."""
    cm, idx, ce, pf, n = _cell_items(commitments, cell_indices, cells, proofs)
    return _each("lwkzg_verify_cell_kzg_proof_each", n,
                 lambda ok, rc: lib().lwkzg_verify_cell_kzg_proof_each(ok, rc, cm, idx, ce, pf, n, ts.ref()))


def verify_cell_kzg_proof_each_device(comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, ts, stream=None):
    """the same on DEVICE pointers (48 n commitment bytes, n uint64 indices, 2048 n cell bytes, 48 n proof bytes, produced on
    `stream`); the verdicts come to the host, the call is synchronous"""
    return _each("lwkzg_verify_cell_kzg_proof_each_device", n,
                 lambda ok, rc: lib().lwkzg_verify_cell_kzg_proof_each_device(ok, rc, comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n,
                                                                              ts.ref(), stream))


def cell_verify_each_points(commitments, cell_indices, cells, proofs, ts):
    """the G1 point each item's pairing is taken of (97 bytes each: flag | x | y; flag 1 = infinity, 2 = a bad item), by the per-item
    verdict call's own code path: a list of n bytes objects"""
    cm, idx, ce, pf, n = _cell_items(commitments, cell_indices, cells, proofs)
    out = C.create_string_buffer(CELL_EACH_POINT_BYTES * max(n, 1))
    _check("lwkzg_cell_verify_each_points", lib().lwkzg_cell_verify_each_points(out, cm, idx, ce, pf, n, ts.ref()))
    return [out.raw[CELL_EACH_POINT_BYTES * i:CELL_EACH_POINT_BYTES * (i + 1)] for i in range(n)]


def _group_offsets(sizes):
    """the g + 1 offsets of groups of these sizes, as the C calls take them"""
    off = [0]
    for m in sizes:
        off.append(off[-1] + m)
    return (C.c_uint64 * len(off))(*off)


def _cell_groups(groups):
    """a list of item lists (an item: (commitment, cell index, cell, proof)) -> the C arguments of the grouped calls"""
    items = [it for grp in groups for it in grp]
    cm, idx, ce, pf, n = _cell_items([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items])
    return cm, idx, ce, pf, n, _group_offsets([len(grp) for grp in groups]), len(groups)


def verify_cell_kzg_proof_groups(groups, ts):
    """one verify_cell_kzg_proof_batch answer per group in one call (lwkzg_verify_cell_kzg_proof_groups): groups is a list of item
    lists, an item (commitment, cell index, cell, proof); returns a list of (rc, ok), group j exactly what the batch call on its
    items alone answers. An empty group answers (C_KZG_OK, True)."""
    cm, idx, ce, pf, n, off, g = _cell_groups(groups)
    return _each("lwkzg_verify_cell_kzg_proof_groups", g,
                 lambda ok, rc: lib().lwkzg_verify_cell_kzg_proof_groups(ok, rc, cm, idx, ce, pf, n, off, g, ts.ref()))


def verify_cell_kzg_proof_groups_device(comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, group_sizes, ts, stream=None):
    """the same on DEVICE pointers (48 n commitment bytes, n uint64 indices, 2048 n cell bytes, 48 n proof bytes, produced on
    `stream`); group_sizes (a host list) cuts the n items into consecutive groups; the answers come to the host, the call is
    synchronous"""
    if sum(group_sizes) != n:
        raise ValueError("group_sizes must add up to n")
    off, g = _group_offsets(group_sizes), len(group_sizes)
    return _each("lwkzg_verify_cell_kzg_proof_groups_device", g,
                 lambda ok, rc: lib().lwkzg_verify_cell_kzg_proof_groups_device(ok, rc, comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n,
                                                                                off, g, ts.ref(), stream))


def cell_verify_groups_partials(groups, ts):
    """per group what cell_verify_partials writes for the group alone (CELL_VERIFY_PARTIAL_BYTES each), by the grouped verdict call's
    own code path up to the pairings; all zero for an empty group and for a group the call answers with an error code: a list of g
    bytes objects"""
    cm, idx, ce, pf, n, off, g = _cell_groups(groups)
    out = C.create_string_buffer(CELL_VERIFY_PARTIAL_BYTES * max(g, 1))
    _check("lwkzg_cell_verify_groups_partials", lib().lwkzg_cell_verify_groups_partials(out, cm, idx, ce, pf, n, off, g, ts.ref()))
    return [out.raw[CELL_VERIFY_PARTIAL_BYTES * j:CELL_VERIFY_PARTIAL_BYTES * (j + 1)] for j in range(g)]


def _blob_items(blobs, commitments, cell_proofs):
    """lists (or concatenated bytes) of n blobs, n commitments and n x 128 cell proofs -> the C arguments"""
    bl = blobs if isinstance(blobs, (bytes, bytearray)) else b"".join(blobs)
    cm = commitments if isinstance(commitments, (bytes, bytearray)) else b"".join(commitments)
    pf = cell_proofs if isinstance(cell_proofs, (bytes, bytearray)) else b"".join(cell_proofs)
    n = len(cm) // 48
    if len(cm) != 48 * n or len(bl) != BYTES_PER_BLOB * n or len(pf) != 48 * CELLS_PER_EXT_BLOB * n:
        raise ValueError("blobs, commitments and cell proofs must hold one blob, one commitment and 128 proofs per blob")
    return bytes(bl), bytes(cm), bytes(pf), n


def verify_blob_cell_kzg_proofs_batch(blobs, commitments, cell_proofs, ts):
    """do the 128 cell proofs of every blob belong to the blob and its commitment (lwkzg_verify_blob_cell_kzg_proofs_batch)? The
    answer of verify_cell_kzg_proof_batch on the 128 n items (commitments[b], k, cell k of blob b, cell_proofs[128 b + k]), without
    the cells ever being passed. The empty call answers True."""
    bl, cm, pf, n = _blob_items(blobs, commitments, cell_proofs)
    ok = C.c_bool(False)
    _check("lwkzg_verify_blob_cell_kzg_proofs_batch", lib().lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), bl, cm, pf, n, ts.ref()))
    return bool(ok.value)


def verify_blob_cell_kzg_proofs_batch_device(blobs_ptr, comm_ptr, cell_proofs_ptr, n, ts, stream=None):
    """the same on DEVICE pointers (n blobs, 48 n commitment bytes, 128 x 48 n proof bytes, produced on `stream`); the verdict is a
    host bool, the call synchronous"""
    ok = C.c_bool(False)
    _check("lwkzg_verify_blob_cell_kzg_proofs_batch_device",
           lib().lwkzg_verify_blob_cell_kzg_proofs_batch_device(C.byref(ok), blobs_ptr, comm_ptr, cell_proofs_ptr, n, ts.ref(), stream))
    return bool(ok.value)


def blob_cell_verify_partials(blobs, commitments, cell_proofs, ts):
    """what cell_verify_partials gives for the 128 n items of these blobs, by the verdict call's own code path up to the pairing"""
    bl, cm, pf, n = _blob_items(blobs, commitments, cell_proofs)
    out = C.create_string_buffer(CELL_VERIFY_PARTIAL_BYTES)
    _check("lwkzg_blob_cell_verify_partials", lib().lwkzg_blob_cell_verify_partials(out, bl, cm, pf, n, ts.ref()))
    return out.raw


def verify_blob_cell_kzg_proofs_groups(blobs, commitments, cell_proofs, group_sizes, ts):
    """one verify_blob_cell_kzg_proofs_batch answer per group of blobs in one call (lwkzg_verify_blob_cell_kzg_proofs_groups):
    group_sizes (in blobs) cuts the n blobs into consecutive groups -- the blobs of a transaction each; a list of (rc, ok)"""
    bl, cm, pf, n = _blob_items(blobs, commitments, cell_proofs)
    if sum(group_sizes) != n:
        raise ValueError("group_sizes must add up to the number of blobs")
    off, g = _group_offsets(group_sizes), len(group_sizes)
    return _each("lwkzg_verify_blob_cell_kzg_proofs_groups", g,
                 lambda ok, rc: lib().lwkzg_verify_blob_cell_kzg_proofs_groups(ok, rc, bl, cm, pf, n, off, g, ts.ref()))


def verify_blob_cell_kzg_proofs_groups_device(blobs_ptr, comm_ptr, cell_proofs_ptr, n, group_sizes, ts, stream=None):
    """the same on DEVICE pointers; group_sizes stays a host list; the answers come to the host, the call is synchronous"""
    if sum(group_sizes) != n:
        raise ValueError("group_sizes must add up to n")
    off, g = _group_offsets(group_sizes), len(group_sizes)
    return _each("lwkzg_verify_blob_cell_kzg_proofs_groups_device", g,
                 lambda ok, rc: lib().lwkzg_verify_blob_cell_kzg_proofs_groups_device(ok, rc, blobs_ptr, comm_ptr, cell_proofs_ptr, n, off, g,
                                                                                      ts.ref(), stream))


def blob_cell_verify_groups_partials(blobs, commitments, cell_proofs, group_sizes, ts):
    """per group of blobs what cell_verify_groups_partials gives for the group's 128-per-blob items: a list of g bytes objects"""
    bl, cm, pf, n = _blob_items(blobs, commitments, cell_proofs)
    if sum(group_sizes) != n:
        raise ValueError("group_sizes must add up to the number of blobs")
    off, g = _group_offsets(group_sizes), len(group_sizes)
    out = C.create_string_buffer(CELL_VERIFY_PARTIAL_BYTES * max(g, 1))
    _check("lwkzg_blob_cell_verify_groups_partials", lib().lwkzg_blob_cell_verify_groups_partials(out, bl, cm, pf, n, off, g, ts.ref()))
    return [out.raw[CELL_VERIFY_PARTIAL_BYTES * j:CELL_VERIFY_PARTIAL_BYTES * (j + 1)] for j in range(g)]


def cell_batch_challenge_host(commitments, cell_indices, cells, proofs, mode):
    """the two-level transcript of the cell batch alone (host only): r, 32 bytes in `mode`'s byte order"""
    cm, idx, ce, pf, n = _cell_items(commitments, cell_indices, cells, proofs)
    out = C.create_string_buffer(32)
    _check("lwkzg_cell_batch_challenge_host", lib().lwkzg_cell_batch_challenge_host(out, cm, idx, ce, pf, n, mode))
    return out.raw


def pairing_line_table(g2_compressed):
    """the 68 Miller-loop lines of a compressed G2 point as the device takes them (host-only test hook): 68 x 192 bytes"""
    out = C.create_string_buffer(68 * 192)
    _check("lwkzg_pairing_line_table", lib().lwkzg_pairing_line_table(out, g2_compressed))
    return out.raw


# ---- sharded batch verification (one batch, one r, one pairing check; include/lambdaworks_kzg_amd.h) ---------

VERIFY_RECORD_BYTES = 160
VERIFY_PARTIAL_BYTES = 328


class VerifyShard:
    """This process's shard of a sharded verify_blob_kzg_proof_batch (lwkzg_verify_shard_*)."""

    def __init__(self, blobs, commitments_bytes, proofs_bytes, n_local, ts):
        assert len(blobs) == n_local * BYTES_PER_BLOB and len(commitments_bytes) == len(proofs_bytes) == 48 * n_local
        self.n = n_local
        self.ts = ts  # the shard's device buffers belong to the setup's context: keep it alive as long as the shard
        self.h = C.c_void_p()
        rec = C.create_string_buffer(VERIFY_RECORD_BYTES * max(n_local, 1))
        _check("lwkzg_verify_shard_begin",
               lib().lwkzg_verify_shard_begin(C.byref(self.h), rec, blobs, commitments_bytes, proofs_bytes, n_local, ts.ref()))
        self.records = rec.raw[:VERIFY_RECORD_BYTES * n_local]

    @classmethod
    def from_device(cls, blobs_ptr, comm_ptr, proofs_ptr, n_local, ts, stream=None):
        """the shard's inputs as device pointers (lwkzg_verify_shard_begin_device); the records come back to the host"""
        self = cls.__new__(cls)
        self.n = n_local
        self.ts = ts
        self.h = C.c_void_p()
        rec = C.create_string_buffer(VERIFY_RECORD_BYTES * max(n_local, 1))
        _check("lwkzg_verify_shard_begin_device",
               lib().lwkzg_verify_shard_begin_device(C.byref(self.h), rec, blobs_ptr, comm_ptr, proofs_ptr, n_local, ts.ref(), stream))
        self.records = rec.raw[:VERIFY_RECORD_BYTES * n_local]
        return self

    def partial(self, records_all, n_total, first_index):
        assert len(records_all) == VERIFY_RECORD_BYTES * n_total
        out = C.create_string_buffer(VERIFY_PARTIAL_BYTES)
        _check("lwkzg_verify_shard_partial", lib().lwkzg_verify_shard_partial(out, self.h, records_all, n_total, first_index))
        return out.raw

    def free(self):
        if self.h:
            lib().lwkzg_verify_shard_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _AsyncVerifier:
    """what Verifier and CellVerifier share; a kind names the prefix of its C symbols (_PREFIX) and its result type (_RESULT)"""

    def __init__(self, ts, max_items):
        self.ts = ts   # the verifier's device scratch belongs to the setup's context
        self.h = C.c_void_p()
        self._results = []
        _check(self._PREFIX + "new", self._fn("new")(C.byref(self.h), ts.ref(), max_items))

    def _fn(self, name):
        return getattr(lib(), self._PREFIX + name)

    def _enqueue(self, *args, call="enqueue", keep=None):
        res = self._RESULT()
        res._keep = keep   # what else the call writes lives as long as its result
        self._results = [r for r in self._results if r.state != 1][-4 * VERIFIER_DEPTH:] + [res]
        rc = self._fn(call)(self.h, C.byref(res), *args)
        if rc != C_KZG_OK:
            err = KzgError(self._PREFIX + call, rc)
            err.result = res
            raise err
        return res

    def pending(self):
        return self._fn("pending")(self.h)

    def wait(self):
        _check(self._PREFIX + "wait", self._fn("wait")(self.h))

    def free(self):
        if self.h:
            self._fn("free")(self.h)   # waits for the calls in flight first
            self.h = C.c_void_p()
            self._results = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Verifier(_AsyncVerifier):
    """lwkzg_verifier_*: device-resident batch verifications that do not block the calling thread. enqueue returns a VerifyResult
    whose state turns 1 once rc / ok / first_bad / r / partial are final; the verifier keeps every result it handed out alive."""
    _PREFIX, _RESULT = "lwkzg_verifier_", VerifyResult

    def __init__(self, ts, max_blobs):
        super().__init__(ts, max_blobs)

    def enqueue(self, blobs_ptr, comm_ptr, proofs_ptr, n, stream=None):
        """returns at once; raises KzgError (its .result is the completed VerifyResult) for what the call itself refuses"""
        return self._enqueue(blobs_ptr, comm_ptr, proofs_ptr, n, stream)

    def enqueue_openings(self, comm_ptr, zs_ptr, ys_ptr, proofs_ptr, n, stream=None):
        """the same for n openings (lwkzg_verifier_enqueue_openings): verify_kzg_proof_batch_device without the wait; the verifier's
        capacity counts openings here. Blob and opening calls may be mixed and complete in order."""
        return self._enqueue(comm_ptr, zs_ptr, ys_ptr, proofs_ptr, n, stream, call="enqueue_openings")


def verifier_host_steps(records, n, first_bad, sums3x97, ysum32, settings_ref, mode):
    """test hook (host only): the two host steps of Verifier.enqueue on caller-supplied blocks; returns the completed VerifyResult"""
    res = VerifyResult()
    _check("lwkzg_verifier_host_steps",
           lib().lwkzg_verifier_host_steps(C.byref(res), records, n, first_bad, sums3x97, ysum32, settings_ref, mode))
    return res


class CellVerifier(_AsyncVerifier):
    """lwkzg_cell_verifier_*: device-resident cell proof batch verifications that do not block the calling thread. enqueue returns a
    CellVerifyResult whose state turns 1 once rc / ok / first_bad / m / partials are final; the verifier keeps every result it handed
    out alive."""
    _PREFIX, _RESULT = "lwkzg_cell_verifier_", CellVerifyResult

    def __init__(self, ts, max_cells, max_groups=0):
        """max_groups > 0: lwkzg_cell_verifier_new_groups -- the verifier also takes enqueue_groups"""
        if not max_groups:
            super().__init__(ts, max_cells)
            return
        self.ts = ts
        self.h = C.c_void_p()
        self._results = []
        _check(self._PREFIX + "new_groups", self._fn("new_groups")(C.byref(self.h), ts.ref(), max_cells, max_groups))

    @classmethod
    def for_blobs(cls, ts, max_blobs, max_groups=0):
        """lwkzg_cell_verifier_new_blobs: a verifier of 128 max_blobs items (and max_groups groups) that also takes WHOLE BLOBS --
        enqueue_blobs and, with max_groups > 0, enqueue_blobs_groups; max_blobs is 1 .. 512"""
        self = cls.__new__(cls)
        self.ts = ts
        self.h = C.c_void_p()
        self._results = []
        _check(cls._PREFIX + "new_blobs", self._fn("new_blobs")(C.byref(self.h), ts.ref(), max_blobs, max_groups))
        return self

    def enqueue_blobs(self, blobs_ptr, comm_ptr, proofs_ptr, n, stream=None):
        """verify_blob_cell_kzg_proofs_batch_device without the wait (lwkzg_cell_verifier_enqueue_blobs): n device-resident blobs, n
        commitments, 128 n cell proofs. Returns at once with a CellVerifyResult; first_bad counts the 128 n expanded items. Raises
        KzgError (its .result is the completed CellVerifyResult) for what the call itself refuses"""
        return self._enqueue(blobs_ptr, comm_ptr, proofs_ptr, n, stream, call="enqueue_blobs")

    def enqueue_blobs_groups(self, blobs_ptr, comm_ptr, proofs_ptr, n, group_sizes, stream=None, partials=True):
        """one answer per group of blobs (lwkzg_cell_verifier_enqueue_blobs_groups): group_sizes (a host list, in BLOBS) cuts the n
        blobs into consecutive groups -- the blobs of a transaction each. Returns at once with a GroupedCellAnswers, as enqueue_groups"""
        ans = GroupedCellAnswers(len(group_sizes), partials)
        off = _group_offsets(group_sizes)
        ans.result = self._enqueue(ans._ok, ans._rc, ans._partials, blobs_ptr, comm_ptr, proofs_ptr, n, off, len(group_sizes), stream,
                                   call="enqueue_blobs_groups", keep=ans)
        return ans

    def enqueue(self, comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, stream=None):
        """returns at once; raises KzgError (its .result is the completed CellVerifyResult) for what the call itself refuses"""
        return self._enqueue(comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, stream)

    def enqueue_groups(self, comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, group_sizes, stream=None, partials=True):
        """one answer per group (lwkzg_cell_verifier_enqueue_groups): group_sizes (a host list) cuts the n device-resident items into
        consecutive groups. Returns at once with a GroupedCellAnswers, whose arrays stay the library's until its result.state reads 1;
        raises KzgError (its .result is the completed CellVerifyResult) for what the call itself refuses"""
        ans = GroupedCellAnswers(len(group_sizes), partials)
        off = _group_offsets(group_sizes)
        ans.result = self._enqueue(ans._ok, ans._rc, ans._partials, comm_ptr, indices_ptr, cells_ptr, proofs_ptr, n, off, len(group_sizes),
                                   stream, call="enqueue_groups", keep=ans)
        return ans


class GroupedCellAnswers:
    """where CellVerifier.enqueue_groups answers: result (a CellVerifyResult) and, once result.state == 1, answers() / partials()"""

    def __init__(self, g, partials=True):
        self.g = g
        self._ok, self._rc = (C.c_uint8 * max(g, 1))(*([0xee] * max(g, 1))), (C.c_int32 * max(g, 1))(*([-1] * max(g, 1)))
        self._partials = C.create_string_buffer(b"\xee" * (CELL_VERIFY_PARTIAL_BYTES * max(g, 1))) if partials else None
        self.result = None

    def answers(self):
        """[(rc, ok)] per group, as verify_cell_kzg_proof_groups returns them"""
        assert self.result is not None and self.result.state == 1
        return [(self._rc[j], bool(self._ok[j])) for j in range(self.g)]

    def partials(self):
        assert self.result is not None and self.result.state == 1 and self._partials is not None
        raw = self._partials.raw
        return [raw[CELL_VERIFY_PARTIAL_BYTES * j:CELL_VERIFY_PARTIAL_BYTES * (j + 1)] for j in range(self.g)]


def cell_verifier_host_steps(distinct48, m, digests32, n, bad_index, status, first_item, sums3x97, rli48, settings_ref, mode):
    """test hook (host only): the two host steps of CellVerifier.enqueue on caller-supplied blocks; status: 2 n fault words (items, then
    distinct commitments) or None, first_item: m indices or None. Returns the completed CellVerifyResult"""
    res = CellVerifyResult()
    st = (C.c_int32 * len(status))(*status) if status is not None else None
    fi = (C.c_uint32 * len(first_item))(*first_item) if first_item is not None else None
    _check("lwkzg_cell_verifier_host_steps",
           lib().lwkzg_cell_verifier_host_steps(C.byref(res), distinct48, m, digests32, n, bad_index, st, fi, sums3x97, rli48, settings_ref,
                                                mode))
    return res


def cell_group_device(comm_ptr, indices_ptr, n, seed, hash_mask=0xffffffff, stream=None):
    """test hook: the grouping kernels of a cell verifier on DEVICE inputs (48 n commitment bytes, n uint64 indices). Returns a dict:
    rows, m, distinct (48 n bytes, padded with infinity encodings), first_item (m), perm_row, row_off (m + 1), perm_col, col_off (129),
    bad_index. The order inside a group of perm_row / perm_col is not defined."""
    u32 = C.c_uint32
    rows, first, perm_row, row_off, perm_col = (u32 * n)(), (u32 * n)(), (u32 * n)(), (u32 * (n + 1))(), (u32 * n)()
    col_off, m, bad = (u32 * 129)(), u32(0), u32(0)
    distinct = C.create_string_buffer(48 * n)
    _check("lwkzg_cell_group_device",
           lib().lwkzg_cell_group_device(rows, C.byref(m), distinct, first, perm_row, row_off, perm_col, col_off, C.byref(bad), comm_ptr,
                                         indices_ptr, n, seed, hash_mask, stream))
    return {"rows": list(rows), "m": m.value, "distinct": distinct.raw, "first_item": list(first)[:m.value], "perm_row": list(perm_row),
            "row_off": list(row_off)[:m.value + 1], "perm_col": list(perm_col), "col_off": list(col_off), "bad_index": bad.value}


def cell_group_segmented_device(comm_ptr, indices_ptr, n, group_sizes, seed, hash_mask=0xffffffff, stream=None, gflag=None, slices=True):
    """test hook: the segmented grouping kernels of a grouped cell verifier on DEVICE inputs, and the slice table cut with the groups
    flagged by gflag (a list of g words; None: the groups with a bad index). Returns a dict: rows (group-local), m (the total), distinct
    (48 n bytes), first_item (m), perm_row, row_off (m + 1), perm_col, col_off (128 g + 1), row_base (g + 1), bad_words (g), slice_off
    (3 g + 1), slices ((group, sum, first, count) each). The order inside a list of perm_row / perm_col is not defined."""
    u32, g = C.c_uint32, len(group_sizes)
    rows, first, perm_row, row_off, perm_col = (u32 * n)(), (u32 * n)(), (u32 * n)(), (u32 * (n + 1))(), (u32 * n)()
    col_off, row_base, bad, m = (u32 * (128 * g + 1))(), (u32 * (g + 1))(), (u32 * max(g, 1))(), u32(0)
    max_slices = 3 * (n // 64 + g)
    sl, sl_off = ((u32 * (4 * max_slices))(), (u32 * (3 * g + 1))()) if slices else (None, None)
    flags = (u32 * g)(*gflag) if gflag is not None else None
    distinct = C.create_string_buffer(48 * max(n, 1))
    _check("lwkzg_cell_group_segmented_device",
           lib().lwkzg_cell_group_segmented_device(rows, C.byref(m), distinct, first, perm_row, row_off, perm_col, col_off, row_base, bad, sl,
                                                   sl_off, flags, comm_ptr, indices_ptr, n, _group_offsets(group_sizes), g, seed, hash_mask,
                                                   stream))
    out = {"rows": list(rows), "m": m.value, "distinct": distinct.raw[:48 * n], "first_item": list(first)[:m.value],
           "perm_row": list(perm_row), "row_off": list(row_off)[:m.value + 1], "perm_col": list(perm_col), "col_off": list(col_off),
           "row_base": list(row_base), "bad_words": list(bad)[:g]}
    if slices:
        out["slice_off"] = list(sl_off)
        out["slices"] = [tuple(sl[4 * k:4 * k + 4]) for k in range(sl_off[3 * g])]
    return out


def blob_group_device(comm_ptr, n_blobs, group_sizes, seed, hash_mask=0xffffffff, stream=None, slices=True):
    """test hook: the blob-level grouping and the expansion kernels of a cell verifier's blob calls on n_blobs DEVICE commitments
    (group_sizes in blobs). Returns cell_group_segmented_device's dict for the n = 128 n_blobs expanded items, and item_group (n) and
    idx (n). The order inside a list of perm_row / perm_col is not defined."""
    u32, g, n = C.c_uint32, len(group_sizes), 128 * n_blobs
    rows, first, perm_row, row_off, perm_col = (u32 * n)(), (u32 * n)(), (u32 * n)(), (u32 * (n + 1))(), (u32 * n)()
    col_off, row_base, bad, m = (u32 * (128 * g + 1))(), (u32 * (g + 1))(), (u32 * max(g, 1))(), u32(0)
    item_group, idx = (u32 * n)(), (C.c_uint64 * n)()
    max_slices = 3 * (n // 64 + g)
    sl, sl_off = ((u32 * (4 * max_slices))(), (u32 * (3 * g + 1))()) if slices else (None, None)
    distinct = C.create_string_buffer(48 * max(n, 1))
    _check("lwkzg_blob_group_device",
           lib().lwkzg_blob_group_device(rows, C.byref(m), distinct, first, perm_row, row_off, perm_col, col_off, row_base, bad, sl, sl_off,
                                         item_group, idx, comm_ptr, n_blobs, _group_offsets(group_sizes), g, seed, hash_mask, stream))
    out = {"rows": list(rows), "m": m.value, "distinct": distinct.raw[:48 * n], "first_item": list(first)[:m.value],
           "perm_row": list(perm_row), "row_off": list(row_off)[:m.value + 1], "perm_col": list(perm_col), "col_off": list(col_off),
           "row_base": list(row_base), "bad_words": list(bad)[:g], "item_group": list(item_group), "idx": list(idx)}
    if slices:
        out["slice_off"] = list(sl_off)
        out["slices"] = [tuple(sl[4 * k:4 * k + 4]) for k in range(sl_off[3 * g])]
    return out


def cell_verifier_groups_host_steps(group_sizes, row_base, bad_words, status, first_item, digests32, distinct48, sums3x97, rli48,
                                    settings_ref, mode, partials=True):
    """test hook (host only): the two host steps of CellVerifier.enqueue_groups on caller-supplied blocks (None where a block is not to
    be read). Returns (the completed CellVerifyResult, [(rc, ok)] per group, the partials per group or None)"""
    g, n = len(group_sizes), sum(group_sizes)
    res, ans = CellVerifyResult(), GroupedCellAnswers(g, partials)
    st = (C.c_int32 * len(status))(*status) if status is not None else None
    fi = (C.c_uint32 * max(len(first_item), 1))(*first_item) if first_item is not None else None
    _check("lwkzg_cell_verifier_groups_host_steps",
           lib().lwkzg_cell_verifier_groups_host_steps(C.byref(res), ans._ok, ans._rc, ans._partials, _group_offsets(group_sizes), g, n,
                                                       (C.c_uint32 * (g + 1))(*row_base), (C.c_uint32 * g)(*bad_words), st, fi, digests32,
                                                       distinct48, sums3x97, rli48, settings_ref, mode))
    ans.result = res
    return res, ans.answers(), ans.partials() if partials else None


def verify_shards_finish(partials, n_shards, n_total, ts):
    assert len(partials) == VERIFY_PARTIAL_BYTES * n_shards
    ok = C.c_bool(False)
    _check("lwkzg_verify_shards_finish", lib().lwkzg_verify_shards_finish(C.byref(ok), partials, n_shards, n_total, ts.ref()))
    return bool(ok.value)


# ---- batched host-pointer extensions --------------------------------------------------------------

def blob_to_kzg_commitment_batch(blobs, ts):
    n = len(blobs) // BYTES_PER_BLOB
    assert len(blobs) == n * BYTES_PER_BLOB
    out = C.create_string_buffer(48 * max(n, 1))
    bad = C.c_size_t(0)
    _check("lwkzg_blob_to_kzg_commitment_batch",
           lib().lwkzg_blob_to_kzg_commitment_batch(out, blobs, n, ts.ref(), C.byref(bad)))
    raw = out.raw      # (ONE copy of the buffer: `.raw` inside the comprehension copied all 48 n bytes per element -- 6 ms of Python per 4096 results)
    return [raw[48 * i:48 * i + 48] for i in range(n)]


def compute_blob_kzg_proof_batch(blobs, commitments, ts):
    n = len(blobs) // BYTES_PER_BLOB
    assert len(blobs) == n * BYTES_PER_BLOB and len(commitments) == 48 * n
    out = C.create_string_buffer(48 * max(n, 1))
    bad = C.c_size_t(0)
    _check("lwkzg_compute_blob_kzg_proof_batch",
           lib().lwkzg_compute_blob_kzg_proof_batch(out, blobs, commitments, n, ts.ref(), C.byref(bad)))
    raw = out.raw      # (ONE copy of the buffer: `.raw` inside the comprehension copied all 48 n bytes per element -- 6 ms of Python per 4096 results)
    return [raw[48 * i:48 * i + 48] for i in range(n)]


def compute_kzg_proof_batch(blobs, zs, ts):
    n = len(blobs) // BYTES_PER_BLOB
    assert len(blobs) == n * BYTES_PER_BLOB and len(zs) == 32 * n
    out, ys = C.create_string_buffer(48 * max(n, 1)), C.create_string_buffer(32 * max(n, 1))
    bad = C.c_size_t(0)
    _check("lwkzg_compute_kzg_proof_batch",
           lib().lwkzg_compute_kzg_proof_batch(out, ys, blobs, zs, n, ts.ref(), C.byref(bad)))
    raw, yraw = out.raw, ys.raw
    return [(raw[48 * i:48 * i + 48], yraw[32 * i:32 * i + 32]) for i in range(n)]


# ---- device-resident extensions (pointers are ints: torch tensor .data_ptr()) -----------------------

def blob_to_kzg_commitment_batch_device(out_ptr, blobs_ptr, n, ts, stream=None, status_ptr=None):
    _check("lwkzg_blob_to_kzg_commitment_batch_device",
           lib().lwkzg_blob_to_kzg_commitment_batch_device(out_ptr, blobs_ptr, n, ts.ref(), stream, status_ptr))


def compute_blob_kzg_proof_batch_device(out_ptr, blobs_ptr, comm_ptr, n, ts, stream=None, status_ptr=None):
    _check("lwkzg_compute_blob_kzg_proof_batch_device",
           lib().lwkzg_compute_blob_kzg_proof_batch_device(out_ptr, blobs_ptr, comm_ptr, n, ts.ref(), stream, status_ptr))


def commit_and_prove_batch_device(comm_ptr, proof_ptr, blobs_ptr, n, ts, stream=None, status_ptr=None):
    """Commitments and blob proofs of n device-resident blobs in one pass (the hash's commitment-independent part runs
    beside the commitment MSM); the same bytes as the two separate calls."""
    _check("lwkzg_commit_and_prove_batch_device",
           lib().lwkzg_commit_and_prove_batch_device(comm_ptr, proof_ptr, blobs_ptr, n, ts.ref(), stream, status_ptr))


def compute_challenges_device(z_ptr, blobs_ptr, comm_ptr, n, ts, stream=None):
    """z_i = compute_challenge(blob_i, commitment_i) for device-resident inputs (n x 32 bytes, mode's byte order)."""
    _check("lwkzg_compute_challenges_device",
           lib().lwkzg_compute_challenges_device(z_ptr, blobs_ptr, comm_ptr, n, ts.ref(), stream))


def g1_lincomb_setup_device(out_ptr, scalars_be_ptr, n_msm, ts, stream=None):
    _check("lwkzg_g1_lincomb_setup_device", lib().lwkzg_g1_lincomb_setup_device(out_ptr, scalars_be_ptr, n_msm, ts.ref(), stream))


def g1_msm_tiled_device(out_ptr, scalars_be_ptr, n_terms, ts, stream=None):
    _check("lwkzg_g1_msm_tiled_device", lib().lwkzg_g1_msm_tiled_device(out_ptr, scalars_be_ptr, n_terms, ts.ref(), stream))


def g1_sum_compressed(points48):
    n = len(points48) // 48
    out = C.create_string_buffer(48)
    _check("lwkzg_g1_sum_compressed", lib().lwkzg_g1_sum_compressed(out, points48, n))
    return out.raw


def fr_ntt4096_device(out_ptr, in_ptr, n, inverse, ts, stream=None):
    _check("lwkzg_fr_ntt4096_device", lib().lwkzg_fr_ntt4096_device(out_ptr, in_ptr, n, 1 if inverse else 0, ts.ref(), stream))


def pairing_product_is_one(g1_compressed, g2_compressed):
    """prod e(P_i, Q_i) == 1 for concatenated compressed points (host-only test hook)."""
    n = len(g1_compressed) // 48
    assert len(g1_compressed) == 48 * n and len(g2_compressed) == 96 * n
    ok = C.c_bool(False)
    _check("lwkzg_pairing_product_is_one", lib().lwkzg_pairing_product_is_one(C.byref(ok), g1_compressed, g2_compressed, n))
    return bool(ok.value)


def batch_challenge_host(records_all, n_total, mode):
    """r of verify_blob_kzg_proof_batch over a transcript of 160-byte records, canonical 32 bytes big-endian (lwkzg_batch_challenge_host)"""
    assert len(records_all) == VERIFY_RECORD_BYTES * n_total
    out = C.create_string_buffer(32)
    _check("lwkzg_batch_challenge_host", lib().lwkzg_batch_challenge_host(out, records_all, n_total, mode))
    return out.raw


def challenge_digests_host(blobs, commitments):
    n = len(commitments) // 48
    assert len(blobs) == n * BYTES_PER_BLOB
    out = C.create_string_buffer(32 * max(n, 1))
    _check("lwkzg_challenge_digests_host", lib().lwkzg_challenge_digests_host(out, blobs, commitments, n))
    raw = out.raw
    return [raw[32 * i:32 * i + 32] for i in range(n)]


def challenge_digests_host_mode(blobs, commitments, mode):
    """the compute_challenge digests of `mode`'s message (host only); MODE_ETH: the consensus specs' be128(4096) degree field"""
    n = len(commitments) // 48
    assert len(blobs) == n * BYTES_PER_BLOB
    out = C.create_string_buffer(32 * max(n, 1))
    _check("lwkzg_challenge_digests_host_mode", lib().lwkzg_challenge_digests_host_mode(out, blobs, commitments, n, mode))
    raw = out.raw
    return [raw[32 * i:32 * i + 32] for i in range(n)]


def setup_image_bytes():
    return lib().lwkzg_setup_image_bytes()


def profile_enable(on=True):
    lib().lwkzg_profile_enable(1 if on else 0)


def profile_reset():
    lib().lwkzg_profile_reset()


def profile_sources():
    """what the profile has been made of since the last reset (lwkzg_profile_sources: dispatch-bound pairs, marker pairs, shared markers)"""
    n = lib().lwkzg_profile_sources(None, 0)
    buf = C.create_string_buffer(n)
    lib().lwkzg_profile_sources(buf, n)
    return json.loads(buf.value.decode())


def profile_report():
    n = lib().lwkzg_profile_report(None, 0)
    buf = C.create_string_buffer(n)
    lib().lwkzg_profile_report(buf, n)
    return json.loads(buf.value.decode())
