#!/usr/bin/env python3
"""EIP-7594 recovery timing, default engine, reference mode, device-resident inputs: a random half of the cells
of synthetic blobs. In one fresh process, after a warm-up call each, the two calls of a pair alternating: lwkzg_recover_cells_and_kzg_proofs_batch_device with proofs at
n = 8 and n = 64 and, as the yardstick, lwkzg_compute_cells_and_kzg_proofs_batch_device at the same n; both calls without proofs at
n = 1024; the ratio of each pair. Median, minimum and maximum of --reps calls, each followed by a device synchronisation. Then one
profiled recovery call at n = 8 with proofs and one at n = 1024 without: the per-kernel figures lwkzg_profile_report returns. Writes
profiles/recover_timing.txt (or --out)."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_timing.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    n_big = 1024
    db = torch.frombuffer(bytearray(b"".join(B.synthetic_blob(i) for i in range(n_big))), dtype=torch.uint8).cuda()
    cells = torch.empty(n_big * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs = torch.empty(64 * 128 * 48, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n_big, dtype=torch.int32, device="cuda")
    K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), None, db.data_ptr(), n_big, ts)
    torch.cuda.synchronize()
    idx = sorted(random.Random(7594).sample(range(128), 64))
    given = cells.view(n_big, 128, 2048)[:, idx, :].contiguous()
    want = cells.clone()
    torch.cuda.synchronize()

    def compute(n, with_proofs):
        K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs.data_ptr() if with_proofs else None, db.data_ptr(), n, ts)
        torch.cuda.synchronize()

    def recover(n, with_proofs):
        K.recover_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs.data_ptr() if with_proofs else None, idx, given.data_ptr(), n, ts,
                                                    None, status.data_ptr())
        torch.cuda.synchronize()

    def med_pair(f, g):
        """the two calls alternating, so that whatever else the machine does meets both alike"""
        f()
        g()
        tf, tg = [], []
        for _ in range(a.reps):
            for fn, t in ((f, tf), (g, tg)):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
        return (statistics.median(tf), min(tf), max(tf)), (statistics.median(tg), min(tg), max(tg))

    lines = ["# recover_cells_and_kzg_proofs against compute_cells_and_kzg_proofs, reference mode, engine direct_bits=%d, device-resident, "
             "64 random cells of 128 per blob; median of %d calls after one warm-up (min, max), the two calls of a pair alternating, each "
             "followed by a device synchronisation" % (ts.direct_table_bits(), a.reps)]
    for n, with_proofs in ((8, True), (64, True), (n_big, False)):
        what = "cells+proofs" if with_proofs else "cells only  "
        (rm, rlo, rhi), (cm, clo, chi) = med_pair(lambda: recover(n, with_proofs), lambda: compute(n, with_proofs))
        lines.append("recover %s n=%-4d %8.3f ms per call  (min %.3f, max %.3f)" % (what, n, rm, rlo, rhi))
        lines.append("compute %s n=%-4d %8.3f ms per call  (min %.3f, max %.3f)" % (what, n, cm, clo, chi))
        lines.append("ratio recover / compute n=%-4d %.3f  (the yardstick's own range: %.3f .. %.3f of its median)" % (n, rm / cm, clo / cm, chi / cm))
    recover(n_big, False)
    assert not status.any().item() and torch.equal(cells, want), "the recovered cells differ from the computed ones"
    lines.append("# the cells recovered at n=%d equal the computed ones" % n_big)
    for n, with_proofs in ((8, True), (n_big, False)):
        K.capi.profile_reset()
        K.capi.profile_enable(True)
        recover(n, with_proofs)
        K.capi.profile_enable(False)
        rep = K.capi.profile_report()
        lines.append("## per kernel, one recovery call, n=%d, %s (launches, total ms)" % (n, "with proofs" if with_proofs else "cells only"))
        for name in sorted(rep, key=lambda k: -rep[k]["total_ms"]):
            lines.append("%-32s %4d %9.4f" % (name, rep[name]["launches"], rep[name]["total_ms"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ts.free()


if __name__ == "__main__":
    main()
