#!/usr/bin/env python3
"""The asynchronous cell verifier (lwkzg_cell_verifier_*) against the synchronous device call, in ONE process, on
device-resident cell batches of n = 128, 1024, 4096 and 8192 items with m = n / 128 and with m = n distinct commitments. Three arms,
alternated round by round after every shape has been warmed, the profiler off:

    (a) lwkzg_verify_cell_kzg_proof_batch_device in a loop        (the calling thread waits inside every call, and groups on the host)
    (b) one cell verifier: enqueue, then wait, per call           (the same device work, the grouping as kernels, two host functions)
    (c) one cell verifier kept four deep                          (LWKZG_VERIFIER_DEPTH calls in flight)

    python tools/cell_verify_async_timing.py [--rounds 8] [--calls 6] [--out profiles/cell_verify_async_timing.txt]

Per shape and arm: median and range over the rounds of ms per call; for (b) and (c) what the calling thread spent inside enqueue. Then,
per shape, the device time of the grouping kernels (one profiled enqueue, lwkzg_profile_report) beside the "host grouping" figure of the
synchronous call's phase clock, which a child process with LWKZG_TIMING=1 prints (the knobs are read once per process).

The m = n / 128 batches are honest (cells and proofs of n / 128 blobs, made by the library). The m = n batches keep those cells and
proofs and take the commitments of n OTHER blobs: valid points, so nothing is rejected and the device work is that of an honest batch
with n rows; their verdict is false. (n honest one-cell items would need the 128 proofs of n blobs each to be computed first.)"""
import argparse, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch
import blobs as B
import lambdaworks_kzg_amd as K

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--calls", type=int, default=6)
ap.add_argument("--sizes", default="128,1024,4096,8192")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_verify_async_timing.txt"))
ap.add_argument("--phase-clock", action="store_true", help="child mode: one synchronous call per shape, the phase clock on stderr")
a = ap.parse_args()
sizes = [int(x) for x in a.sizes.split(",")]
dev = torch.device("cuda:0")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def to_dev(b):
    return torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)


class Shape:
    def __init__(self, n, m, comm, idx, cells, proofs, honest):
        self.n, self.m, self.honest = n, m, honest
        self.keep = (to_dev(comm), torch.tensor(idx, dtype=torch.int64).to(dev), to_dev(cells), to_dev(proofs))
        self.ptrs = tuple(t.data_ptr() for t in self.keep)


def make_shapes(ts):
    nb = max(sizes) // 128
    blobs = B.synthetic_batch(9400, nb)
    comms = K.blob_to_kzg_commitment_batch(blobs, ts)
    made = K.compute_cells_and_kzg_proofs_batch(blobs, ts)
    cells = b"".join(b"".join(c) for c, _ in made)
    proofs = b"".join(b"".join(p) for _, p in made)
    others = K.blob_to_kzg_commitment_batch(B.synthetic_batch(9500, max(sizes)), ts)
    assert len(set(others)) == max(sizes)
    out = []
    for n in sizes:
        idx = list(range(128)) * (n // 128)
        out.append(Shape(n, n // 128, b"".join(c * 128 for c in comms[:n // 128]), idx, cells[:2048 * n], proofs[:48 * n], True))
        if n > 128:
            out.append(Shape(n, n, b"".join(others[:n]), idx, cells[:2048 * n], proofs[:48 * n], False))
    torch.cuda.synchronize(dev)
    return out


ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
shapes = make_shapes(ts)

if a.phase_clock:
    for s in shapes:
        for _ in range(2):   # (the second call's line is the warm one)
            K.verify_cell_kzg_proof_batch_device(*s.ptrs, s.n, ts)
    ts.free()
    sys.exit(0)

v = K.CellVerifier(ts, max(sizes))
st = torch.cuda.Stream(dev)
torch.cuda.synchronize(dev)


def arm_a(s):
    t0 = time.perf_counter()
    for _ in range(a.calls):
        assert K.verify_cell_kzg_proof_batch_device(*s.ptrs, s.n, ts, st.cuda_stream) is s.honest
    return (time.perf_counter() - t0) / a.calls, 0.0


def arm_b(s):
    inside = 0.0
    t0 = time.perf_counter()
    for _ in range(a.calls):
        t1 = time.perf_counter()
        r = v.enqueue(*s.ptrs, s.n, st.cuda_stream)
        inside += time.perf_counter() - t1
        v.wait()
        assert (r.state, r.rc, bool(r.ok), r.m) == (1, 0, s.honest, s.m)
    return (time.perf_counter() - t0) / a.calls, inside / a.calls


def arm_c(s):
    # (an enqueue beyond the depth waits inside the library for the verifier's oldest call: that wait is part of `inside`)
    inside, res = 0.0, []
    t0 = time.perf_counter()
    for _ in range(2 * a.calls):
        t1 = time.perf_counter()
        res.append(v.enqueue(*s.ptrs, s.n, st.cuda_stream))
        inside += time.perf_counter() - t1
    v.wait()
    dt = time.perf_counter() - t0
    assert all((r.state, r.rc, bool(r.ok)) == (1, 0, s.honest) for r in res)
    return dt / len(res), inside / len(res)


arms = (("a", "synchronous device call, loop", arm_a), ("b", "one cell verifier, enqueue + wait", arm_b),
        ("c", "one cell verifier kept %d deep" % K.VERIFIER_DEPTH, arm_c))
for s in shapes:             # warm every shape: the scratch, the pinned blocks, the host-function machinery
    for _ in range(2):
        for _, _, fn in arms:
            fn(s)
torch.cuda.synchronize(dev)
per = {(s, k): [] for s in shapes for k, _, _ in arms}
inside = {(s, k): [] for s in shapes for k, _, _ in arms}
for _ in range(a.rounds):    # the arms alternate within a round
    for s in shapes:
        for k, _, fn in arms:
            dt, ins = fn(s)
            per[(s, k)].append(dt * 1e3)
            inside[(s, k)].append(ins * 1e3)
    torch.cuda.synchronize(dev)

say("default engine (direct table, %d bits), reference mode, %d rounds of %d calls per arm and shape ((c): %d); ms per call: median "
    "[min .. max]" % (ts.direct_table_bits(), a.rounds, a.calls, 2 * a.calls))
for s in shapes:
    say("n = %d, m = %d%s" % (s.n, s.m, "" if s.honest else "  (foreign commitments: verdict false, same work)"))
    for k, what, _ in arms:
        p = per[(s, k)]
        line = "  (%s) %-36s %8.3f [%8.3f .. %8.3f] ms" % (k, what, statistics.median(p), min(p), max(p))
        if k != "a":
            q = inside[(s, k)]
            line += "   inside enqueue: %.3f [%.3f .. %.3f] ms per call" % (statistics.median(q), min(q), max(q))
        say(line)
    pa, pb = per[(s, "a")], per[(s, "b")]
    diff, rng = statistics.median(pb) - statistics.median(pa), max(pa) - min(pa)
    say("  (b) against (a): %+.3f ms per call; (a)'s own range is %.3f ms -> %s" % (
        diff, rng, "within it" if diff <= rng else "SLOWER by more than it: see the per-kernel figures below"))
say()

# the grouping's device time: one profiled enqueue per shape
phase = {}
try:
    env = dict(os.environ, LWKZG_TIMING="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--phase-clock", "--sizes", a.sizes], env=env, capture_output=True, text=True,
                           timeout=600)
    for mt in re.finditer(r"verify cells n=(\d+) m=(\d+): host grouping ([0-9.]+) ms", child.stderr):
        phase[(int(mt.group(1)), int(mt.group(2)))] = float(mt.group(3))   # (the last line of a shape wins: the warm call)
except Exception as e:   # noqa: BLE001
    say("phase clock of the synchronous call: not measured (%s)" % e)
say("grouping: device time of the six k_group_* launches of one profiled enqueue (their fills not included), beside the synchronous "
    "call's host grouping (its phase clock, LWKZG_TIMING=1, a process of its own)")
for s in shapes:
    K.capi.profile_reset()
    K.capi.profile_enable(True)
    r = v.enqueue(*s.ptrs, s.n, st.cuda_stream)
    v.wait()
    torch.cuda.synchronize(dev)
    rep = K.capi.profile_report()
    K.capi.profile_enable(False)
    group = sum(x["total_ms"] for name, x in rep.items() if name.startswith("k_group_"))
    total = sum(x["total_ms"] for x in rep.values())
    host = phase.get((s.n, s.m))
    say("  n = %5d m = %5d: k_group_* %.3f ms of %.3f ms of profiled launches (%.1f %%); host grouping %s" % (
        s.n, s.m, group, total, 100 * group / total if total else 0.0, "%.3f ms" % host if host is not None else "not measured"))
    say("      " + ", ".join("%s %.3f" % (name, rep[name]["total_ms"]) for name in sorted(rep) if name.startswith("k_group_")))
say()
say("not measured here: two cell verifiers on two streams; c-kzg mode; the 16-bit table (the 64-term MSM is a fixed cost in every arm)")
v.free()
ts.free()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
