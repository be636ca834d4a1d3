#!/usr/bin/env python3
"""Per-item EIP-7594 cell proof verification timing, reference mode, default engine. Every measurement runs in
a fresh process of its own (this script starts itself with --worker): median (min, max) of --reps calls after a warm-up call, each
call synchronous (the verdicts are host bytes).
  * lwkzg_verify_cell_kzg_proof_each_device and the host-pointer call at n = 64, 1024 and 4096 cells (the cells of whole blobs, made by
    lwkzg_compute_cells_and_kzg_proofs_batch_device);
  * the yardstick, what a caller without this call does: n calls of lwkzg_verify_cell_kzg_proof_batch with one item each (host
    pointers) at n = 64 and 1024, and the ratio loop / each at equal n;
  * one lwkzg_verify_cell_kzg_proof_batch_device call at equal n (one verdict for the whole batch);
  * the per-kernel figures of lwkzg_profile_report for one per-item call of each size.
Writes profiles/cell_verify_each_timing.txt (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SIZES = (64, 1024, 4096)
LOOP_SIZES = (64, 1024)


def random_blobs(torch, n, seed):
    """n reference-mode blobs on the device: random big-endian elements with the top two bits clear (below r)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    b = torch.randint(0, 256, (n, 4096, 32), dtype=torch.uint8, device="cuda", generator=g)
    b[:, :, 0] &= 0x3f
    return b.reshape(-1)


def med(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(t), min(t), max(t)]


def worker(a):
    import ctypes as C
    import torch
    import lambdaworks_kzg_amd as K
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    out = {"direct_bits": ts.direct_table_bits()}
    n_blobs = max(SIZES) // 128
    blobs = random_blobs(torch, n_blobs, 2)
    comm1 = torch.empty(n_blobs * 48, dtype=torch.uint8, device="cuda")
    K.blob_to_kzg_commitment_batch_device(comm1.data_ptr(), blobs.data_ptr(), n_blobs, ts)
    cells = torch.empty(n_blobs * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs = torch.empty(n_blobs * 128 * 48, dtype=torch.uint8, device="cuda")
    K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs.data_ptr(), blobs.data_ptr(), n_blobs, ts)
    torch.cuda.synchronize()
    comm = comm1.reshape(n_blobs, 1, 48).expand(n_blobs, 128, 48).contiguous().reshape(-1)
    idx = torch.arange(128, dtype=torch.int64, device="cuda").repeat(n_blobs)
    torch.cuda.synchronize()

    def host_args(m):
        h_comm, h_cells, h_proofs = bytes(comm[:48 * m].cpu().numpy()), bytes(cells[:2048 * m].cpu().numpy()), bytes(proofs[:48 * m].cpu().numpy())
        return h_comm, [i % 128 for i in range(m)], h_cells, h_proofs

    def each_device(m):
        got = K.verify_cell_kzg_proof_each_device(comm.data_ptr(), idx.data_ptr(), cells.data_ptr(), proofs.data_ptr(), m, ts)
        assert got == [(0, True)] * m

    if a.worker == "each_device":
        for m in SIZES:
            out["each_device_%d" % m] = med(lambda: each_device(m), a.reps)
    elif a.worker == "each_host":
        for m in SIZES:
            cm, ix, ce, pf, _ = K.capi._cell_items(*host_args(m))
            ok, rc = (C.c_uint8 * m)(), (C.c_int32 * m)()

            def host():
                assert K.lib().lwkzg_verify_cell_kzg_proof_each(ok, rc, cm, ix, ce, pf, m, ts.ref()) == 0 and all(ok) and not any(rc)
            out["each_host_%d" % m] = med(host, a.reps)
    elif a.worker == "loop":
        for m in LOOP_SIZES:
            h_comm, h_idx, h_cells, h_proofs = host_args(m)
            items = [(h_comm[48 * i:48 * i + 48], (C.c_uint64 * 1)(h_idx[i]), h_cells[2048 * i:2048 * i + 2048], h_proofs[48 * i:48 * i + 48])
                     for i in range(m)]
            ok = C.c_bool(False)
            fn = K.lib().lwkzg_verify_cell_kzg_proof_batch

            def loop():
                for c, k, ce, pf in items:
                    assert fn(C.byref(ok), c, k, ce, pf, 1, ts.ref()) == 0 and ok.value
            out["loop_%d" % m] = med(loop, max(1, a.reps // 3))
    elif a.worker == "batch":
        for m in SIZES:
            def batch():
                assert K.verify_cell_kzg_proof_batch_device(comm.data_ptr(), idx.data_ptr(), cells.data_ptr(), proofs.data_ptr(), m, ts)
            out["batch_device_%d" % m] = med(batch, a.reps)
    elif a.worker == "kernels":
        for m in SIZES:
            each_device(m)
            K.capi.profile_enable(True)
            K.capi.profile_reset()
            each_device(m)
            out["kernels_%d" % m] = K.capi.profile_report()
            K.capi.profile_enable(False)
    ts.free()
    print("RESULT " + json.dumps(out))


def run_worker(kind, reps):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--reps", str(reps)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("worker %s failed with status %d" % (kind, p.returncode))
    res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(res[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_verify_each_timing.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    dev = run_worker("each_device", a.reps)
    host = run_worker("each_host", a.reps)
    loop = run_worker("loop", a.reps)
    batch = run_worker("batch", a.reps)
    kern = run_worker("kernels", 1)
    fmt = "%-58s %9.3f ms per call  (min %.3f, max %.3f)"
    lines = ["# verify_cell_kzg_proof_each, reference mode, engine direct_bits=%d; every group in a fresh process; median of %d calls "
             "(the loops: %d) after one warm-up (min, max); the cells of n / 128 whole blobs, every item honest"
             % (dev["direct_bits"], a.reps, max(1, a.reps // 3))]
    for m in SIZES:
        lines.append(fmt % (("each, device-resident n=%d" % m,) + tuple(dev["each_device_%d" % m])))
    for m in SIZES:
        lines.append(fmt % (("each, host pointers   n=%d" % m,) + tuple(host["each_host_%d" % m])))
    for m in LOOP_SIZES:
        lines.append(fmt % (("n one-item batch calls, host pointers n=%d (yardstick)" % m,) + tuple(loop["loop_%d" % m])))
    for m in SIZES:
        lines.append(fmt % (("one batch call, device-resident n=%d (one verdict)" % m,) + tuple(batch["batch_device_%d" % m])))
    for m in LOOP_SIZES:
        lines.append("ratio loop of one-item batch calls / each (host pointers), n=%d: %.2f" % (m, loop["loop_%d" % m][0] / host["each_host_%d" % m][0]))
    for m in SIZES:
        lines.append("ratio each / one batch call (device-resident), n=%d: %.2f" % (m, dev["each_device_%d" % m][0] / batch["batch_device_%d" % m][0]))
    lines.append("## per kernel (lwkzg_profile_report), one device-resident per-item call of each size after a warm-up call")
    for m in SIZES:
        rep = kern["kernels_%d" % m]
        lines.append("n=%d: " % m + ", ".join("%s %.3f ms" % (k, v["total_ms"]) for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["total_ms"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
