"""Helpers of the consensus-specs ("eth") mode tests: the byte reversal the identities rest on and the two Fiat-Shamir transcripts of the
consensus specs, restated with hashlib. With B' = rev32(B): commit_eth(B) = commit_ckzg(B'); (pi, y)_eth(B, z) = (pi', rev(y')) where
(pi', y') = ckzg(B', rev(z)); blob_proof_eth(B, C) = pi' of ckzg.compute_kzg_proof(B', rev(challenge_eth(B, C)))."""
import hashlib

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
RECORD = 160   # C 48 | z 32 | y 32 | proof 48


def rev32(data):
    """every 32-byte element reversed (big-endian <-> little-endian view of the same integers)"""
    assert len(data) % 32 == 0
    if len(data) > (1 << 20):   # (whole batches: the same reversal as one array operation)
        import numpy as np
        return np.frombuffer(data, dtype=np.uint8).reshape(-1, 32)[:, ::-1].tobytes()
    return b"".join(data[i:i + 32][::-1] for i in range(0, len(data), 32))


def challenge_eth(blob, commitment):
    """compute_challenge of the consensus specs: 32 big-endian canonical bytes"""
    digest = hashlib.sha256(b"FSBLOBVERIFY_V1_" + (4096).to_bytes(16, "big") + blob + commitment).digest()
    return (int.from_bytes(digest, "big") % R).to_bytes(32, "big")


def batch_r_eth(records):
    """the batch challenge over n 160-byte records (C | z | y | proof, z and y big-endian): 32 big-endian canonical bytes"""
    assert len(records) % RECORD == 0
    n = len(records) // RECORD
    digest = hashlib.sha256(b"RCKZGBATCH___V1_" + (4096).to_bytes(8, "big") + n.to_bytes(8, "big") + records).digest()
    return (int.from_bytes(digest, "big") % R).to_bytes(32, "big")
