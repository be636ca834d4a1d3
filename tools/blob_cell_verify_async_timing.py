#!/usr/bin/env python3
"""Cell proofs of whole blobs on the verifier that does not block: lwkzg_cell_verifier_enqueue_blobs /
_enqueue_blobs_groups against the synchronous device forms (section 4s). One MI355X, one process, default engine, device-resident
honest inputs; per mode (reference, eth), kind (batch; groups, one group per blob) and shape (1, 6 and 48 blobs) the median (min, max)
of --reps calls after a warm-up call of both routes, the routes taking turns inside each repetition:
  (a) the wall time the calling thread spends inside the enqueue call, against the synchronous call's whole time (which its thread is
      parked for);
  (b) enqueue + wait (until the result's state reads 1) against the synchronous call: "level" unless the medians differ by more than
      the synchronous route's own min-max range, then "ahead" or "behind";
  (c) the device time of the blob-level grouping and the expansion (k_blob_group + k_blob_items_dev, the library's per-kernel report
      around lwkzg_blob_group_device) against the item-level segmented grouping on the 128 n expanded commitments and indices (the
      k_seg_* kernels but the slice table, around lwkzg_cell_group_segmented_device).
Writes profiles/blob_cell_verify_async_timing.txt (or --out)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.blob_cell_verify_timing import SHAPES, random_blobs   # noqa: E402

BLOB_KERNELS = ("k_blob_group", "k_blob_items_dev")
ITEM_KERNELS = ("k_seg_mark", "k_seg_insert", "k_seg_scan", "k_seg_rows", "k_seg_offsets", "k_seg_scatter")


def stats(t):
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_cell_verify_async_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    import lambdaworks_kzg_amd as K
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    n_max = max(SHAPES)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    v = K.CellVerifier.for_blobs(ts, n_max, n_max)
    fmt = "%-44s %9.3f  (min %.3f, max %.3f)"
    lines = ["# cell proofs of whole blobs: the cell verifier's blob calls against the synchronous device forms; engine direct_bits=%d; one "
             "process, device-resident honest inputs on one stream of the caller's; median of %d calls after a warm-up call, the routes "
             "taking turns (min, max); ms per call" % (ts.direct_table_bits(), a.reps)]
    for mode, mode_name in ((K.MODE_REFERENCE, "reference"), (K.MODE_ETH, "eth")):
        ts.set_mode(mode)
        blobs = random_blobs(torch, n_max, 5 + mode)
        comms = torch.empty(n_max * 48, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(n_max * 128 * 48, dtype=torch.uint8, device="cuda")
        K.blob_to_kzg_commitment_batch_device(comms.data_ptr(), blobs.data_ptr(), n_max, ts)
        K.compute_cells_and_kzg_proofs_batch_device(None, proofs.data_ptr(), blobs.data_ptr(), n_max, ts)
        torch.cuda.synchronize()
        p = (blobs.data_ptr(), comms.data_ptr(), proofs.data_ptr())
        for n in SHAPES:
            ones, good = [1] * n, [(0, True)] * n

            def sync_batch():
                assert K.verify_blob_cell_kzg_proofs_batch_device(*p, n, ts, st)

            def sync_groups():
                assert K.verify_blob_cell_kzg_proofs_groups_device(*p, n, ones, ts, st) == good

            def async_batch():
                t0 = time.perf_counter()
                res = v.enqueue_blobs(*p, n, st)
                t1 = time.perf_counter()
                v.wait()
                t2 = time.perf_counter()
                assert (res.state, res.rc, res.ok) == (1, 0, 1)
                return (t1 - t0) * 1e3, (t2 - t0) * 1e3

            def async_groups():
                t0 = time.perf_counter()
                ans = v.enqueue_blobs_groups(*p, n, ones, st, partials=False)
                t1 = time.perf_counter()
                v.wait()
                t2 = time.perf_counter()
                assert ans.result.state == 1 and ans.answers() == good
                return (t1 - t0) * 1e3, (t2 - t0) * 1e3

            for kind, sync_call, async_call in (("batch", sync_batch, async_batch), ("groups", sync_groups, async_groups)):
                async_call()
                sync_call()
                inside, total, sync = [], [], []
                for _ in range(a.reps):
                    e, t = async_call()
                    inside.append(e)
                    total.append(t)
                    t0 = time.perf_counter()
                    sync_call()
                    sync.append((time.perf_counter() - t0) * 1e3)
                inside, total, sync = stats(inside), stats(total), stats(sync)
                gap, spread = sync[0] - total[0], sync[2] - sync[1]
                lines.append("## %s mode, %s, %d blob%s" % (mode_name, kind, n, "" if n == 1 else "s"))
                lines.append(fmt % (("(a) the calling thread inside the enqueue",) + inside))
                lines.append(fmt % (("(b) enqueue + wait",) + total))
                lines.append(fmt % (("    the synchronous device form",) + sync))
                lines.append("(b): synchronous median minus enqueue + wait's %.3f ms; the synchronous route's own min-max range %.3f ms -> %s"
                             % (gap, spread, "level" if abs(gap) <= spread else "ahead" if gap > 0 else "behind"))
    v.free()
    # (c): the two hooks under the library's per-kernel report, a call each per repetition
    lines.append("## (c) device time of the grouping: the blob-level kernels (%s) against the item-level segmented grouping on the expanded "
                 "arrays (%s); one group per blob; the sum of the kernels' device times per call" % (" + ".join(BLOB_KERNELS), ", ".join(ITEM_KERNELS)))
    for n in SHAPES:
        ones = [1] * n
        items = comms[:48 * n].reshape(n, 1, 48).expand(n, 128, 48).contiguous()
        idx = torch.arange(128, dtype=torch.int64, device="cuda").repeat(n)
        torch.cuda.synchronize()
        routes = {"blob-level": (lambda: K.blob_group_device(comms.data_ptr(), n, ones, 0x5eed, slices=False), BLOB_KERNELS),
                  "item-level": (lambda: K.cell_group_segmented_device(items.data_ptr(), idx.data_ptr(), 128 * n, [128] * n, 0x5eed, slices=False),
                                 ITEM_KERNELS)}
        times = {k: [] for k in routes}
        for fn, _ in routes.values():
            fn()
        K.capi.profile_enable(True)
        for _ in range(a.reps):
            for k, (fn, kernels) in routes.items():
                K.capi.profile_reset()
                fn()
                rep = K.capi.profile_report()
                times[k].append(sum(rep[name]["total_ms"] for name in kernels))
        K.capi.profile_enable(False)
        for k in routes:
            lines.append(fmt % (("%d blob%s, %s" % (n, "" if n == 1 else "s", k),) + stats(times[k])))
    ts.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
