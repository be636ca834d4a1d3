"""lambdaworks_kzg_amd -- MI355X-native KZG / EIP-4844 blob-commitment engine.

Host-side mirror of lambdaclass/lambdaworks_kzg's C ABI for the blob-commitment hot path
(blob_to_kzg_commitment / compute_kzg_proof / compute_blob_kzg_proof + trusted-setup load) over
hand-written HIP kernels for gfx950. See DESIGN.md; the C header is include/lambdaworks_kzg_amd.h.
"""
from .capi import (  # noqa: F401
    BYTES_PER_BLOB, BYTES_PER_COMMITMENT, BYTES_PER_PROOF, C_KZG_BADARGS, C_KZG_ERROR, C_KZG_MALLOC, C_KZG_OK,
    FIELD_ELEMENTS_PER_BLOB, MODE_CKZG, MODE_ETH, MODE_REFERENCE, KzgError, KZGSettings, TrustedSetup,
    blob_to_kzg_commitment, blob_to_kzg_commitment_batch, blob_to_kzg_commitment_batch_device, commit_and_prove_batch_device,
    compute_blob_kzg_proof, compute_blob_kzg_proof_batch, compute_blob_kzg_proof_batch_device,
    compute_kzg_proof, compute_kzg_proof_batch, get_mode, knob_report, lib, set_device, set_mode,
    VerifyShard, verify_shards_finish, Verifier, VerifyResult, VERIFIER_DEPTH, verifier_host_steps, batch_challenge_host,
    verify_blob_kzg_proof, verify_blob_kzg_proof_batch, verify_blob_kzg_proof_batch_device, verify_kzg_proof,
    verify_blob_kzg_proof_each, verify_blob_kzg_proof_each_device, verify_kzg_proof_each, verify_kzg_proof_each_device,
    verify_kzg_proof_batch, verify_kzg_proof_batch_device, verify_kzg_proof_batch_partial,
    BYTES_PER_CELL, CELLS_PER_EXT_BLOB, FIELD_ELEMENTS_PER_CELL, FIELD_ELEMENTS_PER_EXT_BLOB,
    compute_cells_and_kzg_proofs, compute_cells_and_kzg_proofs_batch, compute_cells_and_kzg_proofs_batch_device,
    verify_cell_kzg_proof_batch, verify_cell_kzg_proof_batch_device, cell_verify_partials, cell_batch_challenge_host,
    verify_cell_kzg_proof_each, verify_cell_kzg_proof_each_device, cell_verify_each_points,
    verify_cell_kzg_proof_groups, verify_cell_kzg_proof_groups_device, cell_verify_groups_partials,
    verify_blob_cell_kzg_proofs_batch, verify_blob_cell_kzg_proofs_batch_device, blob_cell_verify_partials,
    verify_blob_cell_kzg_proofs_groups, verify_blob_cell_kzg_proofs_groups_device, blob_cell_verify_groups_partials,
    CellVerifier, CellVerifyResult, cell_verifier_host_steps, cell_group_device,
    GroupedCellAnswers, cell_group_segmented_device, cell_verifier_groups_host_steps, blob_group_device,
    recover_cells_and_kzg_proofs, recover_cells_and_kzg_proofs_batch, recover_cells_and_kzg_proofs_batch_device,
    recover_cells_and_kzg_proofs_mixed, recover_cells_and_kzg_proofs_mixed_device,
    compute_cells_and_kzg_proofs_columns, compute_cells_and_kzg_proofs_columns_device,
    recover_cells_and_kzg_proofs_columns, recover_cells_and_kzg_proofs_columns_device,
    CELL_PROOFS_FK20, CELL_PROOFS_MSM, fk20_chunk_blobs,
)

__all__ = [n for n in dir() if not n.startswith("_")]
