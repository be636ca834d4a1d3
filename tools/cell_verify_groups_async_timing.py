#!/usr/bin/env python3
"""Per-group cell proof verdicts that do not block the caller: timing, reference mode, default engine,
device-resident honest inputs. One process measures, per shape, median (min, max) of --reps calls after a warm-up call:
  * the time the calling thread spends inside lwkzg_cell_verifier_enqueue_groups;
  * enqueue + wait (until the result's state reads 1);
  * the synchronous lwkzg_verify_cell_kzg_proof_groups_device on the same inputs.
Shapes: section 4q's three -- 128 groups x 48 cells, 6 x 128, 1024 x 1. The claim under test: at every shape enqueue + wait's median is
not above the synchronous call's median by more than the synchronous call's own min-max range. A second process gives the kernels'
share: the library's per-kernel profile (lwkzg_profile_*) of one grouped enqueue -- the segmented grouping (k_seg_*) and the slice table
(k_seg_slice_table) -- beside the "host plan" the synchronous call reports under LWKZG_TIMING=1, which they replace. Writes
profiles/cell_verify_groups_async_timing.txt (or --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cell_verify_groups_timing import N_BLOBS, SHAPES, random_blobs   # noqa: E402


def stats(t):
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
    by_blob = (comm1.reshape(N_BLOBS, 1, 48).expand(N_BLOBS, 128, 48).contiguous(), torch.arange(128, dtype=torch.int64, device="cuda").repeat(N_BLOBS),
               cells.reshape(N_BLOBS, 128, 2048), proofs.reshape(N_BLOBS, 128, 48))
    by_col = (by_blob[0].permute(1, 0, 2).contiguous(), by_blob[1].reshape(N_BLOBS, 128).permute(1, 0).contiguous(),
              by_blob[2].permute(1, 0, 2).contiguous(), by_blob[3].permute(1, 0, 2).contiguous())
    torch.cuda.synchronize()
    v = K.CellVerifier(ts, max(g * m for g, m in SHAPES), max(g for g, _ in SHAPES))
    for g, m in SHAPES:
        if a.only and a.only != "%dx%d" % (g, m):
            continue
        cm, ix, ce, pf = [t.reshape(-1) for t in (by_col if m == 48 else by_blob)]
        n, sizes = g * m, [m] * g
        p = (cm.data_ptr(), ix.data_ptr(), ce.data_ptr(), pf.data_ptr())
        key = "%dx%d" % (g, m)

        def sync_call():
            assert K.verify_cell_kzg_proof_groups_device(p[0], p[1], p[2], p[3], n, sizes, ts) == [(0, True)] * g

        def async_call():
            t0 = time.perf_counter()
            ans = v.enqueue_groups(p[0], p[1], p[2], p[3], n, sizes, partials=False)
            t1 = time.perf_counter()
            v.wait()
            t2 = time.perf_counter()
            assert ans.result.state == 1 and ans.answers() == [(0, True)] * g
            return (t1 - t0) * 1e3, (t2 - t0) * 1e3

        if a.kernels:
            async_call()
            sync_call()
            K.capi.profile_enable(True)
            K.capi.profile_reset()
            async_call()
            torch.cuda.synchronize()
            rep = K.capi.profile_report()
            K.capi.profile_enable(False)
            sys.stderr.write("KERNELS %s %s\n" % (key, json.dumps(rep)))
            sys.stderr.write("PHASES %s\n" % key)
            sync_call()
            continue
        async_call()
        sync_call()
        inside, total, sync = [], [], []
        for _ in range(a.reps):      # the two forms in turn: the same state of the machine for both
            e, t = async_call()
            inside.append(e)
            total.append(t)
            t0 = time.perf_counter()
            sync_call()
            sync.append((time.perf_counter() - t0) * 1e3)
        out[key] = {"inside_enqueue": stats(inside), "enqueue_and_wait": stats(total), "synchronous": stats(sync)}
    v.free()
    ts.free()
    print("RESULT " + json.dumps(out))


def run_worker(reps, kernels, only):
    env = dict(os.environ)
    if kernels:
        env["LWKZG_TIMING"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(reps)] + (["--kernels"] if kernels else []) + (["--only", only] if only else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit("worker failed with status %d" % p.returncode)
    if not kernels:
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    lines, keep = [], False
    for l in p.stderr.splitlines():
        if l.startswith("KERNELS "):
            _, key, rep = l.split(" ", 2)
            lines.append("# %s: the library's profile of one grouped enqueue, kernels of the grouping and the slice table" % key)
            lines.append(json.dumps({k: val for k, val in json.loads(rep).items() if k.startswith("k_seg_")}, sort_keys=True))
        elif l.startswith("PHASES "):
            keep = True
        elif keep and "verify cell groups" in l:
            lines.append("# the synchronous call's own account (its 'host plan' is what the kernels above replace):")
            lines.append(l)
            keep = False
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_verify_groups_async_timing.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="one shape, as 128x48")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    res = run_worker(a.reps, False, a.only)
    fmt = "%-64s %10.3f ms per call  (min %.3f, max %.3f)"
    lines = ["# lwkzg_cell_verifier_enqueue_groups against lwkzg_verify_cell_kzg_proof_groups_device, reference mode, engine direct_bits=%d, "
             "device-resident inputs, every item honest; one process, the two forms in turn; median of %d calls after one warm-up (min, max)"
             % (res["direct_bits"], a.reps)]
    names = [("inside_enqueue", "the calling thread inside enqueue_groups"), ("enqueue_and_wait", "enqueue_groups + wait"),
             ("synchronous", "the synchronous grouped call")]
    for g, m in SHAPES:
        r = res.get("%dx%d" % (g, m))
        if not r:
            continue
        lines.append("## %d groups x %d cells" % (g, m))
        for k, label in names:
            lines.append(fmt % ((label,) + tuple(r[k])))
        over, spread = r["enqueue_and_wait"][0] - r["synchronous"][0], r["synchronous"][2] - r["synchronous"][1]
        lines.append("enqueue + wait's median minus the synchronous call's: %.3f ms; the synchronous call's own min-max range: %.3f ms -> the claim %s"
                     % (over, spread, "HOLDS" if over <= spread else "FAILS"))
    lines.append("## kernels (a process of its own, the call after a warm-up call)")
    lines += run_worker(1, True, a.only)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
