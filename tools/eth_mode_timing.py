#!/usr/bin/env python3
"""Consensus-specs (eth) mode against c-kzg mode, the yardstick, in ONE process on ONE settings object with the 13-bit Lagrange-form
table: the two modes alternate call by call within each workload of a round, so that both see the same clocks and
the same neighbours.
Per round and mode: 1024 device-resident commitments, 1024 blob proofs, one 4096-blob device-resident batch verification, 8 blobs of
cells + cell proofs. Every call is followed by a device synchronisation; one untimed round warms every shape. Reported: median (min,
max) per mode over --rounds rounds, the ratio of the medians eth / c-kzg, and c-kzg mode's own run-to-run range (max / min) beside it.
The eth blobs are the c-kzg blobs with every 32-byte element reversed: the same field elements, so both modes do the same arithmetic
behind their fronts. --profile: one more round per mode under lwkzg_profile_enable, the kernel totals appended (where a ratio comes from).
Writes profiles/eth_mode_timing.txt (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eth_mode_timing.txt"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--bits", type=int, default=13)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds"
    import numpy as np
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    from lambdaworks_kzg_amd import capi
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    CKZG, ETH = K.MODE_CKZG, K.MODE_ETH
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    ts.enable_direct_table_forms(a.bits, 2)
    n_commit, n_verify, n_cells = 1024, 4096, 8
    le = B.synthetic_batch(0, n_verify, big_endian=False)
    be = np.frombuffer(le, dtype=np.uint8).reshape(-1, 32)[:, ::-1].tobytes()
    blobs = {CKZG: torch.frombuffer(bytearray(le), dtype=torch.uint8).cuda(), ETH: torch.frombuffer(bytearray(be), dtype=torch.uint8).cuda()}
    comms = {m: torch.zeros(48 * n_verify, dtype=torch.uint8, device="cuda") for m in (CKZG, ETH)}
    proofs = {m: torch.zeros(48 * n_verify, dtype=torch.uint8, device="cuda") for m in (CKZG, ETH)}
    out48 = torch.zeros(48 * n_commit, dtype=torch.uint8, device="cuda")
    cells = torch.zeros(n_cells * 128 * 2048, dtype=torch.uint8, device="cuda")
    cproofs = torch.zeros(n_cells * 128 * 48, dtype=torch.uint8, device="cuda")
    ts.reserve(n_verify)
    for m in (CKZG, ETH):          # the honest triples of each mode's verification (the commitments are the same points, the proofs are not)
        ts.set_mode(m)
        capi.commit_and_prove_batch_device(comms[m].data_ptr(), proofs[m].data_ptr(), blobs[m].data_ptr(), n_verify, ts)
        torch.cuda.synchronize()
    assert torch.equal(comms[CKZG], comms[ETH]) and not torch.equal(proofs[CKZG], proofs[ETH])

    def commit(m):
        K.blob_to_kzg_commitment_batch_device(out48.data_ptr(), blobs[m].data_ptr(), n_commit, ts)

    def prove(m):
        K.compute_blob_kzg_proof_batch_device(out48.data_ptr(), blobs[m].data_ptr(), comms[m].data_ptr(), n_commit, ts)

    def verify(m):
        assert K.verify_blob_kzg_proof_batch_device(blobs[m].data_ptr(), comms[m].data_ptr(), proofs[m].data_ptr(), n_verify, ts)

    def cells_and_proofs(m):
        K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), cproofs.data_ptr(), blobs[m].data_ptr(), n_cells, ts)

    work = [("commitments, 1024 device-resident", commit), ("blob proofs, 1024 device-resident", prove),
            ("batch verification, 4096 device-resident", verify), ("cells + cell proofs, 8 blobs", cells_and_proofs)]
    times = {(name, m): [] for name, _ in work for m in (CKZG, ETH)}

    def one_round(record):
        for name, fn in work:
            for m in (CKZG, ETH):
                ts.set_mode(m)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(m)
                torch.cuda.synchronize()
                if record:
                    times[(name, m)].append((time.perf_counter() - t0) * 1e3)

    one_round(False)
    for _ in range(a.rounds):
        one_round(True)
    lines = ["# eth mode against c-kzg mode, one process, one settings object, %d-bit Lagrange-form table; the modes alternate call by call; "
             "%d rounds after one warm-up round; ms per call, median (min, max); every call followed by a device synchronisation" % (a.bits, a.rounds)]
    for name, _ in work:
        c, e = times[(name, CKZG)], times[(name, ETH)]
        mc, me = statistics.median(c), statistics.median(e)
        lines.append("%-42s c-kzg %8.3f (%.3f, %.3f)   eth %8.3f (%.3f, %.3f)   eth / c-kzg %.3f   c-kzg's own range max / min %.3f"
                     % (name, mc, min(c), max(c), me, min(e), max(e), me / mc, max(c) / min(c)))
    if a.profile:
        for m, label in ((CKZG, "c-kzg"), (ETH, "eth")):
            ts.set_mode(m)
            capi.profile_reset()
            capi.profile_enable(True)
            for _, fn in work:
                fn(m)
                torch.cuda.synchronize()
            capi.profile_enable(False)
            rep = capi.profile_report()
            rep = rep if isinstance(rep, dict) else json.loads(rep)
            lines.append("## kernel totals of one round, %s mode (ms; launches)" % label)
            for k in sorted(rep, key=lambda k: -rep[k]["total_ms"]):
                lines.append("%-44s %9.3f  %d" % (k, rep[k]["total_ms"], rep[k]["launches"]))
    ts.set_mode(-1)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ts.free()


if __name__ == "__main__":
    main()
