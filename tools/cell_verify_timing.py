#!/usr/bin/env python3
"""EIP-7594 cell proof batch verification timing, reference mode, default engine. Every measurement runs in a
fresh process of its own (this script starts itself with --worker): median (min, max) of --reps calls after a warm-up call, each call
synchronous (the verdict is a host bool).
  * lwkzg_verify_cell_kzg_proof_batch_device and the host-pointer call at n = 128, 1024, 4096 and 8192 cells (whole blobs: 128 cells
    each, made by lwkzg_compute_cells_and_kzg_proofs_batch_device);
  * the yardstick: lwkzg_verify_blob_kzg_proof_batch_device at n = 1024 and 4096 blobs, and the ratio cell / blob at equal n;
  * the library's phase clock (LWKZG_TIMING=1) of one device-resident call per size.
Writes profiles/cell_verify_timing.txt (or --out). --prof N: only N device-resident calls at n = 8192 (for a
rocprofv3 --kernel-trace --stats run of its own)."""
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

CELL_SIZES = (128, 1024, 4096, 8192)
BLOB_SIZES = (1024, 4096)


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
    import torch
    import lambdaworks_kzg_amd as K
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    out = {"direct_bits": ts.direct_table_bits()}
    if a.worker == "blobs":
        n = max(BLOB_SIZES)
        blobs = random_blobs(torch, n, 1)
        comm = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(n * 48, dtype=torch.uint8, device="cuda")
        K.commit_and_prove_batch_device(comm.data_ptr(), proofs.data_ptr(), blobs.data_ptr(), n, ts)
        torch.cuda.synchronize()
        for m in BLOB_SIZES:
            def call():
                assert K.verify_blob_kzg_proof_batch_device(blobs.data_ptr(), comm.data_ptr(), proofs.data_ptr(), m, ts)
            out["blob_device_%d" % m] = med(call, a.reps)
    else:
        n_blobs = max(CELL_SIZES) // 128
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
        sizes = [max(CELL_SIZES)] if a.worker == "prof" else CELL_SIZES
        for m in sizes:
            def dev():
                assert K.verify_cell_kzg_proof_batch_device(comm.data_ptr(), idx.data_ptr(), cells.data_ptr(), proofs.data_ptr(), m, ts)
            if a.worker == "prof":
                for _ in range(a.reps):
                    dev()
            elif a.worker == "phases":
                for _ in range(3):
                    dev()
            elif a.worker == "device":
                out["cell_device_%d" % m] = med(dev, a.reps)
            else:
                h_comm, h_cells, h_proofs = bytes(comm[:48 * m].cpu().numpy()), bytes(cells[:2048 * m].cpu().numpy()), bytes(proofs[:48 * m].cpu().numpy())
                h_idx = list(range(128)) * (m // 128)
                cm, ix, ce, pf, _ = K.capi._cell_items(h_comm, h_idx, h_cells, h_proofs)
                ok = K.capi.C.c_bool(False)

                def host():
                    assert K.lib().lwkzg_verify_cell_kzg_proof_batch(K.capi.C.byref(ok), cm, ix, ce, pf, m, ts.ref()) == 0 and ok.value
                out["cell_host_%d" % m] = med(host, a.reps)
    ts.free()
    print("RESULT " + json.dumps(out))


def run_worker(kind, reps, env=None):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, "--reps", str(reps)], env=dict(os.environ, **(env or {})),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("worker %s failed with status %d" % (kind, p.returncode))
    res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(res[-1][7:]), p.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_verify_timing.txt"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--prof", type=int, default=0)
    ap.add_argument("--worker", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.prof:
        a.worker, a.reps = "prof", a.prof
        return worker(a)
    dev, _ = run_worker("device", a.reps)
    host, _ = run_worker("host", a.reps)
    blob, _ = run_worker("blobs", a.reps)
    _, phases = run_worker("phases", 1, {"LWKZG_TIMING": "1"})
    fmt = "%-44s %8.3f ms per call  (min %.3f, max %.3f)"
    lines = ["# verify_cell_kzg_proof_batch, reference mode, engine direct_bits=%d; every group in a fresh process; median of %d calls after "
             "one warm-up (min, max); n cells = n / 128 whole blobs" % (dev["direct_bits"], a.reps)]
    for m in CELL_SIZES:
        lines.append(fmt % (("cells device-resident n=%d" % m,) + tuple(dev["cell_device_%d" % m])))
    for m in CELL_SIZES:
        lines.append(fmt % (("cells host pointers   n=%d" % m,) + tuple(host["cell_host_%d" % m])))
    for m in BLOB_SIZES:
        lines.append(fmt % (("blobs device-resident n=%d (yardstick)" % m,) + tuple(blob["blob_device_%d" % m])))
    for m in BLOB_SIZES:
        lines.append("ratio cells(n=%d) / blobs(n=%d), device-resident: %.3f" % (m, m, dev["cell_device_%d" % m][0] / blob["blob_device_%d" % m][0]))
    lines.append("## phase clock (LWKZG_TIMING=1), the third device-resident call of each size in a process of its own")
    seen = {}
    for l in phases.splitlines():
        if "verify cells n=" in l:
            seen.setdefault(l.split("verify cells n=")[1].split(":")[0].split()[0], []).append(l.strip())
    for m in CELL_SIZES:
        calls = seen.get(str(m), [])
        lines += [x for x in calls[-2:]]     # the sums' line and the pairing's line of the last call
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
