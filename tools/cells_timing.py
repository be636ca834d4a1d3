#!/usr/bin/env python3
"""EIP-7594 cells timing, on the default engine and on the 16-bit direct table, reference mode, device-resident
synthetic blobs: the per-blob time of lwkzg_compute_cells_and_kzg_proofs_batch_device at n = 64; in the same process the per-MSM time of
lwkzg_g1_lincomb_setup_device at 1024 MSMs and the ratio per-blob / (128 x per-MSM); the cells-only call (no proofs) for 1024 blobs;
the latency of the single host call lwkzg_compute_cells_and_kzg_proofs. Median of --reps calls after one warm-up, each call followed by a
device synchronisation. Writes profiles/cells_timing.txt (or --out). --prof N: only N device calls at n = 64 and N cells-only calls at
n = 1024 on the default engine (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_timing.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prof", type=int, default=0)
    a = ap.parse_args()
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    n_big = 1024
    data = b"".join(B.synthetic_blob(i) for i in range(n_big))
    db = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cells = torch.empty(n_big * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs = torch.empty(64 * 128 * 48, dtype=torch.uint8, device="cuda")
    msm_out = torch.empty(1024 * 48, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def dev_call(n, with_cells=True, with_proofs=True):
        K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr() if with_cells else None, proofs.data_ptr() if with_proofs else None,
                                                    db.data_ptr(), n, ts)
        torch.cuda.synchronize()

    def lincomb():
        K.capi.g1_lincomb_setup_device(msm_out.data_ptr(), db.data_ptr(), 1024, ts)
        torch.cuda.synchronize()

    if a.prof:
        for _ in range(a.prof):
            dev_call(64)
            dev_call(n_big, with_proofs=False)
        ts.free()
        return

    def med(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t), min(t), max(t)

    lines = ["# compute_cells_and_kzg_proofs, reference mode, device-resident synthetic blobs; median of %d calls after one warm-up "
             "(min, max), each call followed by a device synchronisation" % a.reps]
    blob0 = data[:B.BYTES_PER_BLOB]
    for name, bits in (("default", None), ("16-bit", 16)):
        if bits is not None:
            ts.enable_direct_table(bits)
        lines.append("## engine: %s (direct_bits=%d)" % (name, ts.direct_table_bits()))
        md, lo, hi = med(lambda: dev_call(64))
        per_blob = md / 64
        lines.append("cells+proofs device n=64     %8.2f ms per call  (min %.2f, max %.2f)  %.3f ms per blob  %.0f blobs/s"
                     % (md, lo, hi, per_blob, 1e3 / per_blob))
        mm, mlo, mhi = med(lincomb)
        per_msm = mm / 1024
        lines.append("g1_lincomb_setup_device 1024 %8.2f ms per call  (min %.2f, max %.2f)  %.4f ms per MSM  %.0f MSMs/s"
                     % (mm, mlo, mhi, per_msm, 1e3 / per_msm))
        lines.append("ratio per-blob / (128 x per-MSM): %.3f  (target <= 1.10)" % (per_blob / (128 * per_msm)))
        md, lo, hi = med(lambda: dev_call(n_big, with_proofs=False))
        lines.append("cells only device n=1024     %8.2f ms per call  (min %.2f, max %.2f)  (target <= 2 ms)" % (md, lo, hi))
        md, lo, hi = med(lambda: K.compute_cells_and_kzg_proofs(blob0, ts))
        lines.append("single host call (1 blob)    %8.2f ms per call  (min %.2f, max %.2f)  (target <= 2.5 ms)" % (md, lo, hi))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ts.free()


if __name__ == "__main__":
    main()
