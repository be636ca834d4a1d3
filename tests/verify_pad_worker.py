"""Run by tests/test_gpu_verify_msm.py in fresh processes (the library reads its environment once): the device-resident batch
verification of 65 blobs -- k_decompress_points on two workgroups, the second with one live lane; k_subgroup_coop_asm on two, the second
with one live quad; every validation launch with its LDS footprint (csrc/lds_pad.h) -- for (a) honest triples, (b) the last proof
replaced by a point of E(Fp) outside G1, (c) the first commitment (the zero blob's: infinity) in a valid non-canonical encoding. Prints
the pads in effect, the (return code, verdict) of each call and what lwkzg_verify_blob_kzg_proof_each answers item by item, as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402
import blobs as B  # noqa: E402
import lambdaworks_kzg_amd as K  # noqa: E402

N = 65


def main():
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    blobs = [bytes(B.BYTES_PER_BLOB)] + [B.synthetic_blob(91000 + i) for i in range(1, N)]
    data = b"".join(blobs)
    cj = b"".join(K.blob_to_kzg_commitment_batch(data, ts))
    pj = b"".join(K.compute_blob_kzg_proof_batch(data, cj, ts))
    inf = bytes([0xc0]) + bytes(47)
    assert cj[:48] == inf and pj[:48] == inf
    not_in_g1 = bytes([0x80]) + bytes(47)                      # (0, 2): on the curve, outside the subgroup
    stray = bytes([0xc0]) + bytes(46) + b"\x01"                 # infinity with a stray bit: valid, not canonical
    cases = {"a": (cj, pj), "b": (cj, pj[:48 * (N - 1)] + not_in_g1), "c": (stray + cj[48:], pj)}
    db = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = {"verify_pad_kb": K.knob_report()["verify_pad_kb"]}
    for name, (c, p) in cases.items():
        dc = torch.frombuffer(bytearray(c), dtype=torch.uint8).cuda()
        dp = torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        try:
            got = [0, K.verify_blob_kzg_proof_batch_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), N, ts)]
        except K.KzgError as e:
            got = [e.rc, False]
        out[name] = {"batch": got, "each": [[rc, ok] for rc, ok in K.verify_blob_kzg_proof_each(data, c, p, ts)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
