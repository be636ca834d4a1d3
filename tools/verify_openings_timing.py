#!/usr/bin/env python3
"""Batch verification of openings (lwkzg_verify_kzg_proof_batch_device) timed in ONE process, under a time limit, on
device-resident openings of n = 64, 1024, 4096 and 16384 items (64 blobs opened at n / 64 distinct points each; reference mode, the
engine a plain load selects). After every shape has been warmed, median and range over the repeated calls of:

    batch    lwkzg_verify_kzg_proof_batch_device                       (one pairing on the host; the calling thread waits)
    each     lwkzg_verify_kzg_proof_each on the same items             (one pairing per item on the GPU; host pointers)
    enqueue  lwkzg_verifier_enqueue_openings + wait, and the time the calling thread spends inside the enqueue
    blobs    at n = 4096, lwkzg_verify_blob_kzg_proof_batch_device on 4096 device-resident blobs (64 distinct, repeated)

then the library's per-kernel report (lwkzg_profile_report) of one batch call per shape.

    python tools/verify_openings_timing.py [--calls 12] [--time-limit 480] [--out profiles/verify_openings_timing.txt]"""
import argparse, os, signal, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch
import blobs as B
import lambdaworks_kzg_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=12)
ap.add_argument("--sizes", default="64,1024,4096,16384")
ap.add_argument("--time-limit", type=int, default=480, help="seconds; the process ends itself when they run out")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_openings_timing.txt"))
a = ap.parse_args()
signal.alarm(a.time_limit)
sizes = [int(x) for x in a.sizes.split(",")]
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
N_BLOBS = 64
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def to_dev(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)


def stats(ms):
    return "%9.3f [%9.3f .. %9.3f] ms" % (statistics.median(ms), min(ms), max(ms))


def timed(fn, calls):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
blobs = [B.synthetic_blob(9700 + i) for i in range(N_BLOBS)]
comms = K.blob_to_kzg_commitment_batch(b"".join(blobs), ts)
nmax = max(sizes)
cols = [[], [], [], []]
for lo in range(0, nmax, 1024):   # item i opens blob i mod 64 at a point of its own
    m = min(1024, nmax - lo)
    zs = [((lo + k + 1) * 0x9e3779b97f4a7c15f39cc0605cedc835 % R).to_bytes(32, "big") for k in range(m)]
    res = K.compute_kzg_proof_batch(b"".join(blobs[(lo + k) % N_BLOBS] for k in range(m)), b"".join(zs), ts)
    cols[0] += [comms[(lo + k) % N_BLOBS] for k in range(m)]
    cols[1] += zs
    cols[2] += [y for _, y in res]
    cols[3] += [p for p, _ in res]
host = [b"".join(c) for c in cols]
width = (48, 32, 32, 48)
keep = [to_dev(h) for h in host]
ptrs = [t.data_ptr() for t in keep]
v = K.Verifier(ts, nmax)
st = torch.cuda.Stream(dev)
torch.cuda.synchronize(dev)


def batch(n):
    assert K.verify_kzg_proof_batch_device(*ptrs, n, ts) is True


def each(n):
    got = K.verify_kzg_proof_each(*[h[:w * n] for h, w in zip(host, width)], ts)
    assert got[0] == (0, True) and got[-1] == (0, True)


inside = {}


def enqueue(n):
    t0 = time.perf_counter()
    r = v.enqueue_openings(*ptrs, n, st.cuda_stream)
    inside.setdefault(n, []).append((time.perf_counter() - t0) * 1e3)
    v.wait()
    assert (r.state, r.rc, r.ok) == (1, 0, 1)


for n in sizes:   # warm every shape: the scratch, the pinned blocks, the host-function machinery, the line tables
    for fn in (batch, each, enqueue):
        fn(n)
        fn(n)
inside.clear()
torch.cuda.synchronize(dev)
say("default engine (direct table, %d bits), reference mode, %d calls per figure (each: %d) after two warm-up calls; wall clock of the "
    "calling thread per call: median [min .. max]" % (ts.direct_table_bits(), a.calls, max(3, a.calls // 4)))
for n in sizes:
    say("n = %d openings" % n)
    say("  batch    lwkzg_verify_kzg_proof_batch_device      %s" % stats(timed(lambda: batch(n), a.calls)))
    say("  each     lwkzg_verify_kzg_proof_each              %s" % stats(timed(lambda: each(n), max(3, a.calls // 4))))
    say("  enqueue  lwkzg_verifier_enqueue_openings + wait   %s" % stats(timed(lambda: enqueue(n), a.calls)))
    say("           inside the enqueue                       %s" % stats(inside[n]))
    if n == 4096:
        db = to_dev(b"".join(blobs)).repeat(n // N_BLOBS)
        dc = torch.empty(48 * n, dtype=torch.uint8, device=dev)
        dp = torch.empty(48 * n, dtype=torch.uint8, device=dev)
        K.capi.commit_and_prove_batch_device(dc.data_ptr(), dp.data_ptr(), db.data_ptr(), n, ts)
        torch.cuda.synchronize(dev)

        def blob_batch():
            assert K.verify_blob_kzg_proof_batch_device(db.data_ptr(), dc.data_ptr(), dp.data_ptr(), n, ts) is True

        blob_batch()
        blob_batch()
        say("  blobs    lwkzg_verify_blob_kzg_proof_batch_device %s   (4096 blobs: the same sums and pairing behind the blob hash "
            "and the evaluation)" % stats(timed(blob_batch, a.calls)))
        del db, dc, dp
say()
say("per kernel: one profiled lwkzg_verify_kzg_proof_batch_device call per shape (lwkzg_profile_report; device time of each launch, "
    "which overlap across streams)")
for n in sizes:
    K.capi.profile_reset()
    K.capi.profile_enable(True)
    batch(n)
    torch.cuda.synchronize(dev)
    rep = K.capi.profile_report()
    K.capi.profile_enable(False)
    say("  n = %5d: " % n + ", ".join("%s %.3f" % (name, rep[name]["total_ms"]) for name in sorted(rep, key=lambda k: -rep[k]["total_ms"])))
say()
say("not measured here: c-kzg and eth mode (the byte order of z and y is the only difference on this path); the host-pointer form "
    "(160 bytes per item of upload in front of the same work)")
v.free()
ts.free()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
