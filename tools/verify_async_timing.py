#!/usr/bin/env python3
"""The asynchronous batch verifier (lwkzg_verifier_*) against the synchronous device call, in ONE process, on N
device-resident blobs, on the 16-bit direct table and on the engine a plain load selects. Three arms, alternated round by round after
every shape has been warmed, the profiler off:

    (a) lwkzg_verify_blob_kzg_proof_batch_device in a loop                       (the calling thread waits inside every call)
    (b) one verifier: enqueue, then wait, per call                               (the same work, two host-function hand-overs more)
    (c) two verifiers on two streams, each kept LWKZG_VERIFIER_DEPTH deep        (the two contexts of the settings overlap)

    python tools/verify_async_timing.py [--n 4096] [--rounds 8] [--calls 8] [--out profiles/verify_async_timing.txt]

Per arm: median and range over the rounds of ms per call and blobs/s; for (b) and (c) also what the calling thread spent inside
enqueue per call. The text goes to stdout and to --out.
"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch
import blobs as B
import lambdaworks_kzg_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--calls", type=int, default=8, help="calls per round and arm (arm (c): per verifier)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_async_timing.txt"))
a = ap.parse_args()
assert a.rounds >= 6
dev = torch.device("cuda:0")
n = a.n
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def measure(ts, label):
    h_blobs = B.synthetic_batch(9000, n)
    h_comms = b"".join(K.blob_to_kzg_commitment_batch(h_blobs, ts))
    h_proofs = b"".join(K.compute_blob_kzg_proof_batch(h_blobs, h_comms, ts))
    to_dev = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
    d_b, d_c, d_p = to_dev(h_blobs), to_dev(h_comms), to_dev(h_proofs)
    ptrs = (d_b.data_ptr(), d_c.data_ptr(), d_p.data_ptr())
    ts.reserve(n, caller_streams=2)
    v = [K.Verifier(ts, n), K.Verifier(ts, n)]
    st = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize(dev)

    def arm_a():
        t0 = time.perf_counter()
        for _ in range(a.calls):
            assert K.verify_blob_kzg_proof_batch_device(*ptrs, n, ts, st[0].cuda_stream)
        return (time.perf_counter() - t0) / a.calls, 0.0, a.calls

    def arm_b():
        inside = 0.0
        t0 = time.perf_counter()
        for _ in range(a.calls):
            t1 = time.perf_counter()
            r = v[0].enqueue(*ptrs, n, st[0].cuda_stream)
            inside += time.perf_counter() - t1
            v[0].wait()
            assert r.state == 1 and r.rc == 0 and r.ok == 1
        return (time.perf_counter() - t0) / a.calls, inside / a.calls, a.calls

    def arm_c():
        # (an enqueue beyond the depth waits inside the library for the verifier's oldest call: that wait is part of `inside`)
        inside, res = 0.0, []
        t0 = time.perf_counter()
        for _ in range(a.calls):
            for k in (0, 1):
                t1 = time.perf_counter()
                res.append(v[k].enqueue(*ptrs, n, st[k].cuda_stream))
                inside += time.perf_counter() - t1
        v[0].wait(); v[1].wait()
        dt = time.perf_counter() - t0
        assert all(r.state == 1 and r.rc == 0 and r.ok == 1 for r in res)
        return dt / len(res), inside / len(res), len(res)

    arms = (("a", "synchronous device call, loop", arm_a), ("b", "one verifier, enqueue + wait", arm_b),
            ("c", "two verifiers, two streams, depth %d" % K.VERIFIER_DEPTH, arm_c))
    for _ in range(2):           # warm every shape: the scratch, the twin context, the host-function machinery of both streams
        for _, _, fn in arms:
            fn()
    torch.cuda.synchronize(dev)
    per = {k: [] for k, _, _ in arms}
    inside = {k: [] for k, _, _ in arms}
    for _ in range(a.rounds):    # the arms alternate within a round
        for k, _, fn in arms:
            dt, ins, _ = fn()
            per[k].append(dt * 1e3)
            inside[k].append(ins * 1e3)
        torch.cuda.synchronize(dev)
    say("%s, %d blobs, %d rounds of %d calls per arm (ms per call: median [min .. max]; blobs/s at the median)" % (label, n, a.rounds, a.calls))
    for k, what, _ in arms:
        med = statistics.median(per[k])
        line = "  (%s) %-44s %7.3f [%7.3f .. %7.3f] ms   %9.0f blobs/s" % (k, what, med, min(per[k]), max(per[k]), n / med * 1e3)
        if k != "a":
            line += "   inside enqueue: %.3f [%.3f .. %.3f] ms per call (%.1f %%)" % (
                statistics.median(inside[k]), min(inside[k]), max(inside[k]), 100 * statistics.median(inside[k]) / med)
        say(line)
    rate = {k: n / statistics.median(per[k]) * 1e3 for k in per}
    spread = {k: n / min(per[k]) * 1e3 - n / max(per[k]) * 1e3 for k in per}
    say("  (b) against (a): %+.3f ms per call; (a)'s own range is %.3f ms" % (statistics.median(per["b"]) - statistics.median(per["a"]),
                                                                            max(per["a"]) - min(per["a"])))
    say("  (c) against (a): %+.0f blobs/s; the larger of the two arms' ranges is %.0f blobs/s -> overlap %s" % (
        rate["c"] - rate["a"], max(spread["a"], spread["c"]), "achieved" if rate["c"] - rate["a"] > max(spread["a"], spread["c"]) else "NOT achieved"))
    say()
    for x in v:
        x.free()


ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
measure(ts, "default engine (direct table, %d bits)" % ts.direct_table_bits())
try:
    ts.enable_direct_table(16)
    measure(ts, "16-bit direct table")
except K.KzgError as e:
    say("16-bit direct table: not measured (%s)" % e)
ts.free()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
