#!/usr/bin/env python3
"""Per-group EIP-7594 cell proof verification timing, reference mode, default engine, device-resident inputs.
One process measures, per shape, median (min, max) of --reps calls after a warm-up call, each call synchronous:
  * lwkzg_verify_cell_kzg_proof_groups_device, one call for the g groups;
  * the two routes to the same per-group answers without it: g calls of lwkzg_verify_cell_kzg_proof_batch_device, one per group, and
    one lwkzg_verify_cell_kzg_proof_each_device over all items with the verdicts ANDed per group;
  * the floor: one lwkzg_verify_cell_kzg_proof_batch_device over everything (one verdict).
Shapes: 128 groups x 48 cells (the column sidecars of a 48-blob block), 6 x 128 (the blobs of a transaction), 1024 x 1. Every item is
honest (made by lwkzg_compute_cells_and_kzg_proofs_batch_device). The claim under test: at 128 x 48 the grouped call's median lies
below the lower of the two routes' medians by more than that route's own min-max range. A second process with LWKZG_TIMING=1 gives the
grouped call's phase split. Writes profiles/cell_verify_groups_timing.txt (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((128, 48), (6, 128), (1024, 1))
N_BLOBS = 48


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
    blobs = random_blobs(torch, N_BLOBS, 2)
    comm1 = torch.empty(N_BLOBS * 48, dtype=torch.uint8, device="cuda")
    K.blob_to_kzg_commitment_batch_device(comm1.data_ptr(), blobs.data_ptr(), N_BLOBS, ts)
    cells = torch.empty(N_BLOBS * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs = torch.empty(N_BLOBS * 128 * 48, dtype=torch.uint8, device="cuda")
    K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs.data_ptr(), blobs.data_ptr(), N_BLOBS, ts)
    torch.cuda.synchronize()
    # by blob: item 128 b + k; by column: item 48 k + b
    by_blob = (comm1.reshape(N_BLOBS, 1, 48).expand(N_BLOBS, 128, 48).contiguous(), torch.arange(128, dtype=torch.int64, device="cuda").repeat(N_BLOBS),
               cells.reshape(N_BLOBS, 128, 2048), proofs.reshape(N_BLOBS, 128, 48))
    by_col = (by_blob[0].permute(1, 0, 2).contiguous(), by_blob[1].reshape(N_BLOBS, 128).permute(1, 0).contiguous(),
              by_blob[2].permute(1, 0, 2).contiguous(), by_blob[3].permute(1, 0, 2).contiguous())
    torch.cuda.synchronize()
    for g, m in SHAPES:
        if a.only and a.only != "%dx%d" % (g, m):
            continue
        cm, ix, ce, pf = [t.reshape(-1) for t in (by_col if m == 48 else by_blob)]
        n, sizes = g * m, [m] * g
        p = (cm.data_ptr(), ix.data_ptr(), ce.data_ptr(), pf.data_ptr())

        def groups():
            assert K.verify_cell_kzg_proof_groups_device(p[0], p[1], p[2], p[3], n, sizes, ts) == [(0, True)] * g

        def batch_per_group():
            for j in range(g):
                o = j * m
                assert K.verify_cell_kzg_proof_batch_device(p[0] + 48 * o, p[1] + 8 * o, p[2] + 2048 * o, p[3] + 48 * o, m, ts)

        def each_anded():
            got = K.verify_cell_kzg_proof_each_device(p[0], p[1], p[2], p[3], n, ts)
            assert [all(rc == 0 and ok for rc, ok in got[j * m:(j + 1) * m]) for j in range(g)] == [True] * g

        def one_batch():
            assert K.verify_cell_kzg_proof_batch_device(p[0], p[1], p[2], p[3], n, ts)

        key = "%dx%d" % (g, m)
        if a.phases:
            groups()
            sys.stderr.write("PHASES %s\n" % key)
            groups()
            continue
        out[key] = {"groups": med(groups, a.reps), "batch_per_group": med(batch_per_group, a.reps), "each_anded": med(each_anded, a.reps),
                    "one_batch": med(one_batch, a.reps)}
    ts.free()
    print("RESULT " + json.dumps(out))


def run_worker(reps, phases, only):
    env = dict(os.environ)
    if phases:
        env["LWKZG_TIMING"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(reps)] + (["--phases"] if phases else []) + (["--only", only] if only else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % p.returncode)
    if phases:
        lines, keep = [], False
        for l in p.stderr.splitlines():
            if l.startswith("PHASES "):
                keep = True
                lines.append("# " + l[7:])
            elif keep and "verify cell groups" in l:
                lines.append(l)
                keep = False
        return lines
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_verify_groups_timing.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="one shape, as 128x48")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--phases", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = run_worker(a.reps, False, a.only)
    fmt = "%-64s %10.3f ms per call  (min %.3f, max %.3f)"
    lines = ["# verify_cell_kzg_proof_groups, reference mode, engine direct_bits=%d, device-resident inputs, every item honest; one process; "
             "median of %d calls after one warm-up (min, max)" % (res["direct_bits"], a.reps)]
    names = [("groups", "one grouped call"), ("batch_per_group", "g batch calls, one per group"), ("each_anded", "one per-item call, ANDed per group"),
             ("one_batch", "one batch call over everything (one verdict: the floor)")]
    for g, m in SHAPES:
        r = res.get("%dx%d" % (g, m))
        if not r:
            continue
        lines.append("## %d groups x %d cells" % (g, m))
        for k, label in names:
            lines.append(fmt % ((label,) + tuple(r[k])))
        route = min(("batch_per_group", "each_anded"), key=lambda k: r[k][0])
        gap, spread = r[route][0] - r["groups"][0], r[route][2] - r[route][1]
        lines.append("the lower route: %s; its median minus the grouped call's: %.3f ms; its own min-max range: %.3f ms; ratio %.2f -> the claim %s"
                     % (route, gap, spread, r[route][0] / r["groups"][0], "HOLDS" if gap > spread else "FAILS"))
    lines.append("## the grouped call's phases (LWKZG_TIMING=1, a process of its own, the call after a warm-up call)")
    lines += run_worker(1, True, a.only)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
