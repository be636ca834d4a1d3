#!/usr/bin/env python3
"""Mixed recovery timing, reference mode, default engine, device-resident inputs: 64 synthetic blobs in 8
distinct random sets of 64 cells, 8 blocks of 8 blobs. In one fresh process, after a warm-up call each, the two arms alternating:
  arm A  one lwkzg_recover_cells_and_kzg_proofs_mixed_device call of 64 blobs
  arm B  eight lwkzg_recover_cells_and_kzg_proofs_batch_device calls of 8 blobs, one per block, enqueued one after the other
each arm followed by one device synchronisation; cells and proofs. Median, minimum and maximum of --reps rounds, first on the MSM
engine, then with the FK20 engine on at min_blobs = 64 (the documented threshold), where arm B's calls of 8 stay on the MSM path by
construction. Then one profiled mixed call of each kind: the per-kernel figures lwkzg_profile_report returns. Writes
profiles/recover_mixed_timing.txt (or --out)."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

BLOCKS, PER_BLOCK, GIVEN = 8, 8, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_mixed_timing.txt"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    n = BLOCKS * PER_BLOCK
    db = torch.frombuffer(bytearray(b"".join(B.synthetic_blob(i) for i in range(n))), dtype=torch.uint8).cuda()
    want_cells = torch.empty(n * 128 * 2048, dtype=torch.uint8, device="cuda")
    want_proofs = torch.empty(n * 128 * 48, dtype=torch.uint8, device="cuda")
    K.compute_cells_and_kzg_proofs_batch_device(want_cells.data_ptr(), want_proofs.data_ptr(), db.data_ptr(), n, ts)
    torch.cuda.synchronize()
    rnd = random.Random(7594)
    sets = [sorted(rnd.sample(range(128), GIVEN)) for _ in range(BLOCKS)]
    assert len(set(map(tuple, sets))) == BLOCKS
    lists = [sets[b // PER_BLOCK] for b in range(n)]
    full = want_cells.view(n, 128, 2048)
    # the blobs' given cells one after the other: with one count for all, arm B's block j is a slice of arm A's input
    given = torch.cat([full[b, lists[b], :] for b in range(n)]).contiguous()
    cells = torch.empty_like(want_cells)
    proofs = torch.empty_like(want_proofs)
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    per_block_in, per_block_cells, per_block_proofs = PER_BLOCK * GIVEN * 2048, PER_BLOCK * 128 * 2048, PER_BLOCK * 128 * 48

    def arm_a():
        K.recover_cells_and_kzg_proofs_mixed_device(cells.data_ptr(), proofs.data_ptr(), lists, given.data_ptr(), ts, None, status.data_ptr())
        torch.cuda.synchronize()

    def arm_b():
        for j in range(BLOCKS):
            K.recover_cells_and_kzg_proofs_batch_device(cells.data_ptr() + j * per_block_cells, proofs.data_ptr() + j * per_block_proofs, sets[j],
                                                        given.data_ptr() + j * per_block_in, PER_BLOCK, ts, None,
                                                        status.data_ptr() + 4 * j * PER_BLOCK)
        torch.cuda.synchronize()

    def checked(arm, name):
        cells.zero_()
        proofs.zero_()
        arm()
        assert not status.any().item() and torch.equal(cells, want_cells) and torch.equal(proofs, want_proofs), name

    def med_pair(f, g):
        """the two arms alternating, so that whatever else the machine does meets both alike"""
        f()
        g()
        tf, tg = [], []
        for _ in range(a.reps):
            for fn, t in ((f, tf), (g, tg)):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
        return (statistics.median(tf), min(tf), max(tf)), (statistics.median(tg), min(tg), max(tg))

    def profiled(title):
        K.capi.profile_reset()
        K.capi.profile_enable(True)
        arm_a()
        K.capi.profile_enable(False)
        rep = K.capi.profile_report()
        out = ["## per kernel, one mixed call of %d blobs, %s (launches, total ms)" % (n, title)]
        for name in sorted(rep, key=lambda k: -rep[k]["total_ms"]):
            out.append("%-32s %4d %9.4f" % (name, rep[name]["launches"], rep[name]["total_ms"]))
        return out

    lines = ["# recovery of %d blobs in %d distinct random sets of %d cells (%d blocks of %d), cells + proofs, reference mode, engine "
             "direct_bits=%d, device-resident" % (n, BLOCKS, GIVEN, BLOCKS, PER_BLOCK, ts.direct_table_bits()),
             "# arm A: one mixed call; arm B: %d shared-set calls of %d. Median of %d rounds after one warm-up (min, max), the arms "
             "alternating, each arm followed by one device synchronisation" % (BLOCKS, PER_BLOCK, a.reps)]
    kernels = []
    for engine in ("MSM", "FK20 at min_blobs = 64"):
        if engine != "MSM":
            t0 = time.perf_counter()
            ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 64)
            lines.append("# FK20 table: %d bytes, built in %.0f ms" % (ts.fk20_table_bytes(), (time.perf_counter() - t0) * 1e3))
        checked(arm_a, "arm A, " + engine)
        checked(arm_b, "arm B, " + engine)
        (am, alo, ahi), (bm, blo, bhi) = med_pair(arm_a, arm_b)
        lines.append("%-22s arm A (1 mixed call)       %8.3f ms  (min %.3f, max %.3f)" % (engine, am, alo, ahi))
        lines.append("%-22s arm B (%d shared-set calls) %8.3f ms  (min %.3f, max %.3f)" % (engine, BLOCKS, bm, blo, bhi))
        lines.append("%-22s ratio A / B %.3f  (arm B's own range: %.3f .. %.3f of its median)" % (engine, am / bm, blo / bm, bhi / bm))
        kernels += profiled("engine " + engine)
    lines.append("# both arms' outputs equal compute_cells_and_kzg_proofs_batch_device's on the original blobs, on both engines")
    ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)
    text = "\n".join(lines + kernels) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ts.free()


if __name__ == "__main__":
    main()
