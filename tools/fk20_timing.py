#!/usr/bin/env python3
"""FK20 against the MSM path for the cell proofs: lwkzg_compute_cells_and_kzg_proofs_batch_device (cells and
proofs), reference mode, default table, device-resident synthetic blobs, n = 1, 2, 4, 8, 16, 32, 64, 256, 1024. Both engines run in the
same process on two settings objects over the same setup, alternating call by call; the median of --reps calls each after one warm-up,
each call followed by a device synchronisation. The last lines name the smallest n from which FK20's median stays below the MSM path's:
the library's default min_blobs (LWKZG_FK20_DEFAULT_MIN_BLOBS). Writes profiles/fk20_timing.txt (or --out). --prof N: only N FK20 calls at
n = 64 (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SIZES = (1, 2, 4, 8, 16, 32, 64, 256, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk20_timing.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prof", type=int, default=0)
    ap.add_argument("--window-bits", type=int, default=0)
    a = ap.parse_args()
    assert a.reps >= 7 or a.prof
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    K.set_mode(K.MODE_REFERENCE)
    path = os.path.join(ROOT, "tests", "golden", "trusted_setup.txt")
    n_big = max(SIZES)
    data = b"".join(B.synthetic_blob(i) for i in range(n_big))
    db = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cells = torch.empty(n_big * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs = {name: torch.zeros(n_big * 128 * 48, dtype=torch.uint8, device="cuda") for name in ("msm", "fk20")}
    ts = {"msm": K.TrustedSetup.from_file(path), "fk20": K.TrustedSetup.from_file(path)}
    t0 = time.perf_counter()
    ts["fk20"].set_cell_proof_engine(K.CELL_PROOFS_FK20, a.window_bits, 1)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3

    def call(name, n):
        K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs[name].data_ptr(), db.data_ptr(), n, ts[name])
        torch.cuda.synchronize()

    if a.prof:
        for _ in range(a.prof):
            call("fk20", 64)
        for t in ts.values():
            t.free()
        return

    lines = ["# compute_cells_and_kzg_proofs_batch_device (cells + proofs), reference mode, default table (direct_bits=%d), device-resident "
             "synthetic blobs" % ts["msm"].direct_table_bits(),
             "# both engines in one process, alternating call by call; median of %d calls after one warm-up (min, max), each call followed "
             "by a device synchronisation" % a.reps,
             "# FK20 table: %d bytes, built in %.0f ms (bases, table and scratch)" % (ts["fk20"].fk20_table_bytes(), build_ms),
             "#    n   MSM ms/call (min, max)          FK20 ms/call (min, max)         MSM ms/blob  FK20 ms/blob  MSM / FK20"]
    med = {}
    for n in SIZES:
        t = {"msm": [], "fk20": []}
        for name in t:
            call(name, n)
        for _ in range(a.reps):
            for name in ("msm", "fk20"):
                t0 = time.perf_counter()
                call(name, n)
                t[name].append((time.perf_counter() - t0) * 1e3)
        same = bool(torch.equal(proofs["msm"][:n * 6144], proofs["fk20"][:n * 6144]))
        m, f = statistics.median(t["msm"]), statistics.median(t["fk20"])
        med[n] = (m, f)
        lines.append("%6d  %10.3f (%9.3f, %9.3f)  %10.3f (%9.3f, %9.3f)  %10.4f  %10.4f  %8.2f%s"
                     % (n, m, min(t["msm"]), max(t["msm"]), f, min(t["fk20"]), max(t["fk20"]), m / n, f / n, m / f,
                        "" if same else "   PROOFS DIFFER"))
    wins = [n for n in SIZES if all(med[k][1] < med[k][0] for k in SIZES if k >= n)]
    lines.append("smallest measured n from which FK20's median stays below the MSM path's: %s" % (wins[0] if wins else "none"))
    for n in (64, 1024):
        lines.append("per-blob ratio MSM / FK20 at n = %d: %.2f" % (n, med[n][0] / med[n][1]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    for t in ts.values():
        t.free()


if __name__ == "__main__":
    main()
