#!/usr/bin/env python3
"""Per-item verification timing: ms per call of lwkzg_verify_blob_kzg_proof_each_device at n = 1, 64, 1024, 4096
on device-resident honest items; the batch verification of the same 4096 blobs (the floor the shared front sets); 16 host threads
calling verify_blob_kzg_proof over the same 4096 items. Writes profiles/verify_each_timing.txt (or --out). --prof N: only N calls at
n = 4096 (for a rocprofv3 --kernel-trace --stats run of its own: front / combine / pairing)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_each_timing.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prof", type=int, default=0)
    a = ap.parse_args()
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    n = 4096
    data = b"".join(B.synthetic_blob(i) for i in range(n))
    cms = b"".join(K.blob_to_kzg_commitment_batch(data, ts))
    prs = b"".join(K.compute_blob_kzg_proof_batch(data, cms, ts))
    dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()   # noqa: E731
    db, dc, dp = dev(data), dev(cms), dev(prs)
    torch.cuda.synchronize()
    each = lambda m: K.verify_blob_kzg_proof_each_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), m, ts)   # noqa: E731
    assert each(n) == [(0, True)] * n
    if a.prof:
        for _ in range(a.prof):
            each(n)
        return
    lines = ["# lwkzg_verify_blob_kzg_proof_each_device, honest device-resident items, reference mode, default engine; "
             "median of %d calls after one warm-up" % a.reps]

    def med(fn):
        fn()
        t = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t), min(t), max(t)
    for m in (1, 64, 1024, 4096):
        md, lo, hi = med(lambda: each(m))
        lines.append("each_device n=%-5d %8.2f ms per call  (min %.2f, max %.2f)" % (m, md, lo, hi))
    md, lo, hi = med(lambda: K.verify_blob_kzg_proof_batch_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, ts))
    lines.append("batch_device n=4096    %8.2f ms per call  (min %.2f, max %.2f)" % (md, lo, hi))
    l = K.lib()
    ok_all = [True]

    def loop(lo_, hi_):
        ok = C.c_bool(False)
        for i in range(lo_, hi_):
            rc = l.verify_blob_kzg_proof(C.byref(ok), data[i * B.BYTES_PER_BLOB:(i + 1) * B.BYTES_PER_BLOB], cms[48 * i:48 * i + 48],
                                         prs[48 * i:48 * i + 48], ts.ref())
            if rc != 0 or not ok.value:
                ok_all[0] = False
    nt = 16
    t0 = time.perf_counter()
    th = [threading.Thread(target=loop, args=(n * k // nt, n * (k + 1) // nt)) for k in range(nt)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    ms = (time.perf_counter() - t0) * 1e3
    assert ok_all[0]
    lines.append("16 host threads x verify_blob_kzg_proof over the 4096 items: %.1f ms" % ms)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    ts.free()


if __name__ == "__main__":
    main()
