"""Run by tests/test_gpu_commit_tail.py in fresh processes (the library reads its environment once), one per arm of LWKZG_COMMIT_TAIL:
commitments and proofs of fixed batches that take one workgroup per blob on the direct table (n >= 512), printed as JSON. The arms --
k_commit_tail behind the second pass with the clears riding on the parse kernel (shipped; any value but 0), and fold / second pass /
finalize as launches of their own behind two fill launches (0) -- compute the same group elements and must print the same bytes.
The flags_* legs (tests/test_gpu_full_chunk_flags.py reads them) run tests/flag_cases.py's batches, whose special blobs raise the redo flag
in the accumulation or in the fold, on the launch sets a FULL chunk takes: a fresh process has no second context, so nothing is ever
"busy beside us" and 1024 blobs take the one-wave-per-SIMD builds (k_commit_tail<true>, k_direct_fold_lanes_asm_alone)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402
import blobs as B  # noqa: E402
import lambdaworks_kzg_amd as K  # noqa: E402
from lambdaworks_kzg_amd import capi  # noqa: E402
from flag_cases import fold_collision_scalars, full_chunk_batch  # noqa: E402

R = B.R
SIZES = (512, 513, 1024, 1500)
# scalar sets that make lanes meet P = +-Q on a setup whose 4096 points are all the generator (tests/test_gpu_setups_unstructured.py)
ADVERSARIAL = [[1] * 4096, [1, R - 1] * 2048, [3] * 4096, [(1 << 16) + 1] * 4096, list(range(1, 4097)), [R - 1] * 4096, [0] * 4095 + [5],
               [2, 2, R - 4, 7] * 1024]


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _commit_device(ts_ref, data, n):
    """device-resident commitments; the status words start out as garbage and must come back zero"""
    d_blobs = _dev(data)
    d_out = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = K.lib().lwkzg_blob_to_kzg_commitment_batch_device(d_out.data_ptr(), d_blobs.data_ptr(), n, ts_ref, None, d_status.data_ptr())
    assert rc == K.C_KZG_OK, rc
    torch.cuda.synchronize()
    return bytes(d_out.cpu().numpy().tobytes()), int(d_status.abs().sum())


def _profiled(fn):
    capi.profile_reset()
    capi.profile_enable(True)
    try:
        r = fn()
    finally:
        capi.profile_enable(False)
    return r, capi.profile_report()


FLAG_SEED = 1   # tests/test_flag_cases_cpu.py proves the special blobs of this seed


def _flag_legs(ts, tag, out):
    """flagged blobs on the launch sets of 1024 blobs (the ALONE builds) and of 1023 (the shareable ones; uneven shares of the second
    pass), each with the library's profile of the call; then an honest batch on the same settings"""
    for n in (1024, 1023):
        data, _ = full_chunk_batch(n, FLAG_SEED)
        (got, bad), prof = _profiled(lambda: _commit_device(ts.ref(), data, n))
        out["%s_flags_%d" % (tag, n)] = {"commitments": got.hex(), "status_sum": bad, "profile": prof}
        if n == 1024:
            honest = B.synthetic_batch(52000 + n, n)
            (got, bad), prof = _profiled(lambda: _commit_device(ts.ref(), honest, n))
            out["%s_honest_after_flags_1024" % tag] = {"commitments": got.hex(), "status_sum": bad, "profile": prof}
    if tag != "default":
        return
    # the same scalars as 1024 MSMs over the setup (no parse kernel of the commitment call in front: the flags are cleared by a memset),
    # and as ONE MSM of 2^22 terms over the tiled setup: no compressed output per tile, so the lane fold is a launch of its own
    n = 1024
    data, _ = full_chunk_batch(n, FLAG_SEED)
    d_in = _dev(data)
    d_out = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def lincomb():
        capi.g1_lincomb_setup_device(d_out.data_ptr(), d_in.data_ptr(), n, ts)
        torch.cuda.synchronize()
        return bytes(d_out.cpu().numpy().tobytes())
    got, prof = _profiled(lincomb)
    out["lincomb_flags_1024"] = {"commitments": got.hex(), "status_sum": 0, "profile": prof}
    d_one = torch.zeros(48, dtype=torch.uint8, device="cuda")

    def tiled():
        capi.g1_msm_tiled_device(d_one.data_ptr(), d_in.data_ptr(), n * 4096, ts)
        torch.cuda.synchronize()
        return bytes(d_one.cpu().numpy().tobytes())
    got, prof = _profiled(tiled)
    out["tiled_flags_1024"] = {"commitments": got.hex(), "status_sum": 0, "profile": prof}


def main():
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    out = {"knob": K.knob_report()["commit_tail"], "bits": ts.direct_table_bits()}

    # reference mode on the table a plain load selects (13 bits on an empty MI355X), then on a wider one
    for tag, bits, sizes in (("default", None, SIZES), ("wide", 14, (512, 1024))):
        if bits is not None:
            ts.enable_direct_table(bits)
        for n in sizes:
            data = B.synthetic_batch(52000 + n, n)
            got, bad = _commit_device(ts.ref(), data, n)
            out["%s_%d" % (tag, n)] = {"commitments": got.hex(), "status_sum": bad}
        if bits is None:
            # the launches of ONE call at 1024 blobs, by the library's own events
            n = 1024
            data = B.synthetic_batch(52000 + n, n)
            (got, bad), prof = _profiled(lambda: _commit_device(ts.ref(), data, n))
            assert got.hex() == out["default_1024"]["commitments"]
            out["profile_1024"] = prof
            # blob proofs of the same batch
            d_blobs, d_comm = _dev(data), _dev(got)
            d_proof = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            K.compute_blob_kzg_proof_batch_device(d_proof.data_ptr(), d_blobs.data_ptr(), d_comm.data_ptr(), n, ts)
            torch.cuda.synchronize()
            out["proofs_1024"] = bytes(d_proof.cpu().numpy().tobytes()).hex()
        _flag_legs(ts, tag, out)

    # equal and opposite lane sums inside the fold (the flag is raised behind the second pass), on the 14-bit table
    n = 512
    data = b"".join(b"".join(v.to_bytes(32, "big") for v in fold_collision_scalars(b)) for b in range(n))
    (got, bad), prof = _profiled(lambda: _commit_device(ts.ref(), data, n))
    out["fold_collisions_512"] = {"commitments": got.hex(), "status_sum": bad, "profile": prof}

    # adversarial scalars on the all-generator setup (hand-built KZGSettings), 512 blobs: every blob but the [0 .. 0 5] ones is flagged
    # and recomputed by the second pass; then an honest batch on the same settings, whose flags and status words the first call left set
    ts.enable_direct_table(10)   # (the wide table makes room for the table of the second settings object)
    g_blst = C.create_string_buffer(ts.g1_values_bytes()[:144] * 4096)
    s = K.KZGSettings()
    s.fs, s.g1_values, s.g2_values = None, C.cast(g_blst, C.c_void_p), ts.s.g2_values
    try:
        n = 512
        sets = ADVERSARIAL * (n // len(ADVERSARIAL))
        data = b"".join(b"".join(v.to_bytes(32, "big") for v in ss) for ss in sets)
        (got, bad), prof = _profiled(lambda: _commit_device(C.byref(s), data, n))
        out["adversarial_512"] = {"commitments": got.hex(), "status_sum": bad, "profile": prof}
        host = C.create_string_buffer(48 * n)
        first_bad = C.c_size_t(0)
        assert K.lib().lwkzg_blob_to_kzg_commitment_batch(host, data, n, C.byref(s), C.byref(first_bad)) == K.C_KZG_OK
        out["adversarial_512_host_pointers"] = host.raw.hex()
        # one non-zero scalar per blob: no lane adds anything, nothing can collide
        honest = b"".join(b"".join((b + 2 if i == (37 * b) % 4096 else 0).to_bytes(32, "big") for i in range(4096)) for b in range(n))
        (got, bad), prof = _profiled(lambda: _commit_device(C.byref(s), honest, n))
        out["honest_after_adversarial_512"] = {"commitments": got.hex(), "status_sum": bad, "profile": prof}
    finally:
        K.lib().lwkzg_release_context(C.byref(s))

    # c-kzg semantics on the Lagrange form of the setup: the copy + range check is in front of the MSM, not the parse kernel
    ts.enable_direct_table(10)
    ts.set_mode(K.MODE_CKZG)
    assert ts.direct_table_forms() & 2, "no Lagrange-form table"
    n = 512
    data = B.synthetic_batch(53000, n, big_endian=False)
    got, bad = _commit_device(ts.ref(), data, n)
    out["ckzg_lagrange_512"] = {"commitments": got.hex(), "status_sum": bad}
    # the Lagrange-form twins of the flagged batch: the same collisions among the points [l_i(tau)]G (the clears are memsets here)
    n = 1024
    data, _ = full_chunk_batch(n, FLAG_SEED, lagrange=True)
    (got, bad), prof = _profiled(lambda: _commit_device(ts.ref(), data, n))
    out["ckzg_lagrange_flags_1024"] = {"commitments": got.hex(), "status_sum": bad, "profile": prof}
    ts.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
