"""Run by tests/test_gpu_dispatch_events.py in fresh processes (the library reads its environment once), one per arm of
LWKZG_PROF_MARKERS: the library's profile of fixed calls, taken from the dispatch packets' own start and stop times (shipped, 0) or from a
pair of marker packets around every launch (1), with the results of the same calls profiled and unprofiled, printed as JSON. What a call
computes and which launches it makes do not depend on how those launches are timed: every byte, name and launch count must agree."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402
import blobs as B  # noqa: E402
import lambdaworks_kzg_amd as K  # noqa: E402
from lambdaworks_kzg_amd import capi  # noqa: E402


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


class Call:
    """one device-resident call on fixed inputs, its buffers allocated once"""

    def __init__(self, ts, n, proofs=False):
        self.ts, self.n, self.proofs = ts, n, proofs
        self.d_blobs = _dev(B.synthetic_batch(61000 + n, n))
        self.d_out = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
        self.d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.d_comm = None
        if proofs:
            self.d_comm = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
            K.blob_to_kzg_commitment_batch_device(self.d_comm.data_ptr(), self.d_blobs.data_ptr(), n, ts, None, self.d_status.data_ptr())
        torch.cuda.synchronize()

    def run(self):
        """(result bytes, sum of the status words, host wall clock in ms from synchronize to synchronize)"""
        self.d_out.zero_()
        self.d_status.fill_(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.proofs:
            K.compute_blob_kzg_proof_batch_device(self.d_out.data_ptr(), self.d_blobs.data_ptr(), self.d_comm.data_ptr(), self.n, self.ts, None,
                                                  self.d_status.data_ptr())
        else:
            K.blob_to_kzg_commitment_batch_device(self.d_out.data_ptr(), self.d_blobs.data_ptr(), self.n, self.ts, None, self.d_status.data_ptr())
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return bytes(self.d_out.cpu().numpy().tobytes()).hex(), int(self.d_status.abs().sum()), wall


def main():
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    out = {"knob": K.knob_report()["prof_markers"], "bits": ts.direct_table_bits()}
    capi.profile_enable(False)
    capi.profile_reset()
    assert capi.profile_report() == {}

    # 512 commitments take parse, accumulate, second pass and tail; 1 the cooperative kernel; 9 the hand-scheduled accumulation with the lane
    # fold as a launch of its own and finalize; 16 proofs the proof pipeline with its scopes on the library's side streams
    for tag, n, proofs in (("commit_512", 512, False), ("commit_1", 1, False), ("commit_9", 9, False), ("proofs_16", 16, True)):
        call = Call(ts, n, proofs)
        capi.profile_reset()
        off = call.run()                       # profile off (and the call's warm-up: workspace, host threads)
        report_off = capi.profile_report()
        capi.profile_enable(True)
        try:
            on = call.run()
        finally:
            capi.profile_enable(False)
        out[tag] = {"off": {"bytes": off[0], "status_sum": off[1]}, "report_after_off": report_off,
                    "on": {"bytes": on[0], "status_sum": on[1], "wall_ms": on[2]}, "profile": capi.profile_report(),
                    "sources": capi.profile_sources()}

    # a per-item verification of four openings: its two padded validation launches keep their marker scopes, back to back on one stream
    n = 4
    blobs = B.synthetic_batch(61500, n)
    zs = b"".join((5 + i).to_bytes(32, "big") for i in range(n))
    comms = b"".join(capi.blob_to_kzg_commitment_batch(blobs, ts))
    opened = capi.compute_kzg_proof_batch(blobs, zs, ts)
    d = [_dev(x) for x in (comms, zs, b"".join(y for _, y in opened), b"".join(p for p, _ in opened))]
    torch.cuda.synchronize()
    verdicts = []
    for prof in (False, True):
        capi.profile_reset()
        capi.profile_enable(prof)
        try:
            verdicts.append([list(v) for v in capi.verify_kzg_proof_each_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, ts)])
        finally:
            capi.profile_enable(False)
    out["openings_4"] = {"verdicts": verdicts, "profile": capi.profile_report(), "sources": capi.profile_sources()}

    # the pool: a reset while pairs are pending, then a report; then two profiled calls in a row, whose second takes its events from the pool
    call = Call(ts, 9)
    capi.profile_reset()
    capi.profile_enable(True)
    try:
        K.blob_to_kzg_commitment_batch_device(call.d_out.data_ptr(), call.d_blobs.data_ptr(), 9, ts, None, call.d_status.data_ptr())
        capi.profile_reset()                   # (the call's pairs are pending: nothing has read them yet)
        out["report_after_pending_reset"] = capi.profile_report()
        first = call.run()
        second = call.run()
    finally:
        capi.profile_enable(False)
    out["twice"] = {"first": first[0], "second": second[0], "profile": capi.profile_report()}
    ts.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
