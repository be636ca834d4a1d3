#!/usr/bin/env python3
"""The column calls against the full calls: lwkzg_compute_cells_and_kzg_proofs_columns_device and
lwkzg_recover_cells_and_kzg_proofs_columns_device (cells and proofs), device-resident synthetic blobs, reference and eth mode, default
table. Compute: n in {6, 21, 48} x c in {8, 64, 128}; recover: 64 even columns given, the 64 odd ones wanted, n in {6, 48}; one
host-pointer row (n = 48, c = 8); with the FK20 engine on (the library's default threshold), n = 64 x c in {8, 64, 128}.

Every row times three routes, alternating call by call: the full call of the baseline library (--baseline: the library built from the
parent commit in a directory of its own; without it the column says "-"), this build's full call, and this build's column call. This
build's two routes run in ONE process; the baseline's library lives in a child process of its own on the same GPU (two builds of one
library do not share a process), which holds its settings and buffers, runs one call when told to and reports the call's time. The median of --reps calls each after one warm-up, with minimum and maximum; each call is followed
by a device synchronisation. "ahead" says whether the column call's median is below the baseline's by more than the baseline's own
min-max range, "inside" whether it lies within that range (what c = 128 should show). ms/slot: per (blob, column), beside the full
call's. Writes profiles/cells_columns_timing.txt (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SETUP = os.path.join(ROOT, "tests", "golden", "trusted_setup.txt")
EVEN, ODD = list(range(0, 128, 2)), list(range(1, 128, 2))
N_MAX = 64


class KZGSettings(C.Structure):
    _fields_ = [("fs", C.c_void_p), ("g1_values", C.c_void_p), ("g2_values", C.c_void_p)]


class Baseline:
    """the few full calls of another build of the library, through ctypes alone (it may lack symbols the package binds)"""

    def __init__(self, path):
        self.l = C.CDLL(path)
        vp, sz, ps, pu64 = C.c_void_p, C.c_size_t, C.POINTER(KZGSettings), C.POINTER(C.c_uint64)
        l = self.l
        l.load_trusted_setup_file.argtypes = [ps, vp]
        l.free_trusted_setup.argtypes = [ps]
        l.lwkzg_settings_set_mode.argtypes = [ps, C.c_int]
        l.lwkzg_set_cell_proof_engine.argtypes = [ps, C.c_int, C.c_int, sz]
        l.lwkzg_compute_cells_and_kzg_proofs_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, sz, ps, C.POINTER(sz)]
        l.lwkzg_compute_cells_and_kzg_proofs_batch_device.argtypes = [vp, vp, vp, sz, ps, vp, vp]
        l.lwkzg_recover_cells_and_kzg_proofs_batch_device.argtypes = [vp, vp, pu64, vp, sz, sz, ps, vp, vp]
        self.libc = C.CDLL(None)
        self.libc.fopen.restype = vp
        self.libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        self.libc.fclose.argtypes = [vp]

    def settings(self, mode, fk20):
        s = KZGSettings()
        fp = self.libc.fopen(os.fsencode(SETUP), b"r")
        assert fp and self.l.load_trusted_setup_file(C.byref(s), fp) == 0
        self.libc.fclose(fp)
        self.l.lwkzg_settings_set_mode(C.byref(s), mode)
        if fk20:
            assert self.l.lwkzg_set_cell_proof_engine(C.byref(s), 1, 0, 0) == 0
        return s


def worker(path):
    """the baseline's process: one command per line on stdin -- "setup MODE FK20", "compute N", "recover N", "host N", "free" --, one
    line back: the call's milliseconds (device synchronisation included), or "ok"""
    import torch
    import blobs as B
    base = Baseline(path)
    sync = torch.cuda.synchronize
    cells = torch.empty(N_MAX * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs = torch.empty(N_MAX * 128 * 48, dtype=torch.uint8, device="cuda")
    data = b"".join(B.synthetic_blob(3000 + i) for i in range(N_MAX))
    db = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    idx_even = (C.c_uint64 * 64)(*EVEN)
    hc, hp = C.create_string_buffer(48 * 128 * 2048), C.create_string_buffer(48 * 128 * 48)
    bs, given = None, {}
    for line in sys.stdin:
        cmd = line.split()
        if not cmd:
            continue
        ms = None
        if cmd[0] == "setup":
            bs, given = base.settings(int(cmd[1]), cmd[2] == "1"), {}
        elif cmd[0] == "free":
            base.l.free_trusted_setup(C.byref(bs))
        else:
            n = int(cmd[1])
            if cmd[0] == "recover" and n not in given:
                assert base.l.lwkzg_compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), None, db.data_ptr(), n, C.byref(bs), None, None) == 0
                sync()
                given[n] = cells[:n * 262144].view(n, 128, 2048)[:, EVEN].reshape(-1).clone()
            sync()
            t0 = time.perf_counter()
            if cmd[0] == "compute":
                rc = base.l.lwkzg_compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs.data_ptr(), db.data_ptr(), n, C.byref(bs), None, None)
            elif cmd[0] == "recover":
                rc = base.l.lwkzg_recover_cells_and_kzg_proofs_batch_device(cells.data_ptr(), proofs.data_ptr(), idx_even, given[n].data_ptr(), 64, n,
                                                                            C.byref(bs), None, None)
            else:
                rc = base.l.lwkzg_compute_cells_and_kzg_proofs_batch(hc, hp, data[:n * 131072], n, C.byref(bs), None)
            sync()
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0
        print("ok" if ms is None else "%.6f" % ms, flush=True)


class Worker:
    def __init__(self, path):
        import subprocess
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", path], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True)

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        while True:   # (a line that is neither is the runtime's own chatter)
            answer = self.p.stdout.readline()
            assert answer, "the baseline's process ended"
            answer = answer.strip()
            if answer == "ok":
                return None
            try:
                return float(answer)
            except ValueError:
                pass

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells_columns_timing.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline", default="", help="the library built from the parent commit (a .so in a directory of its own)")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    assert a.reps >= 7
    import torch
    import lambdaworks_kzg_amd as K
    import blobs as B
    base = Worker(a.baseline) if a.baseline else None

    sync = torch.cuda.synchronize
    cells_full = torch.empty(N_MAX * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs_full = torch.empty(N_MAX * 128 * 48, dtype=torch.uint8, device="cuda")
    cells_cols = torch.empty(N_MAX * 128 * 2048, dtype=torch.uint8, device="cuda")
    proofs_cols = torch.empty(N_MAX * 128 * 48, dtype=torch.uint8, device="cuda")
    data = b"".join(B.synthetic_blob(3000 + i) for i in range(N_MAX))   # big-endian canonical elements: a blob in either mode
    db = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    lines = ["# column calls against full calls (cells + proofs), device-resident synthetic blobs, default table; one process, the routes "
             "alternating call by call",
             "# median of %d calls after one warm-up (min, max), ms per call, each call followed by a device synchronisation" % a.reps,
             "# baseline: %s" % ("the full call of the library built from the parent commit, in a process of its own, taking turns" if base else
                                 "none given (--baseline)"),
             "# ahead: the column call's median is below the baseline's by more than the baseline's min-max range; inside: within that range",
             "# ms/slot: median / (n c) of the column call, and median / (128 n) of the baseline's (this build's without one) full call",
             "# %-26s %4s %4s  %-30s %-30s %-30s %8s %-7s %9s %9s %6s"
             % ("call", "n", "c", "baseline full (min, max)", "this build full (min, max)", "columns (min, max)", "col/full", "verdict", "ms/slot", "full's", "ratio")]

    print("\n".join(lines), flush=True)

    def row(label, n, c, routes, same):
        """routes: [(name, fn)] in the order baseline, full, columns (baseline may be None); fn returns its own time, or None: timed here"""
        t = {name: [] for name, fn in routes if fn}
        for name, fn in routes:
            if fn:
                fn()
        for _ in range(a.reps):
            for name, fn in routes:
                if fn:
                    t0 = time.perf_counter()
                    own = fn()
                    t[name].append((time.perf_counter() - t0) * 1e3 if own is None else own)

        def cell(name):
            if name not in t:
                return "%-30s" % "-"
            return "%-30s" % ("%9.3f (%8.3f, %8.3f)" % (statistics.median(t[name]), min(t[name]), max(t[name])))

        ref = "baseline" if "baseline" in t else "full"
        m_ref, m_col = statistics.median(t[ref]), statistics.median(t["columns"])
        spread = max(t[ref]) - min(t[ref])
        verdict = "ahead" if m_ref - m_col > spread else "inside" if min(t[ref]) <= m_col <= max(t[ref]) else "behind" if m_col > max(t[ref]) else "below"
        slot, full_slot = m_col / (n * c), m_ref / (n * 128)
        lines.append("  %-26s %4d %4d  %s %s %s %8.3f %-7s %9.5f %9.5f %6.2f%s"
                     % (label, n, c, cell("baseline"), cell("full"), cell("columns"), m_col / m_ref, verdict, slot, full_slot, slot / full_slot,
                        "" if same() else "   OUTPUTS DIFFER"))
        print(lines[-1], flush=True)

    for mode, mode_name in ((K.MODE_REFERENCE, "reference"), (K.MODE_ETH, "eth")):
        for fk20 in (False, True):
            ts = K.TrustedSetup.from_file(SETUP)
            ts.set_mode(mode)
            if base:
                base.ask("setup %d %d" % (mode, fk20))
            if fk20:
                ts.set_cell_proof_engine(K.CELL_PROOFS_FK20, 0, 0)
            shapes = [(64, c) for c in (8, 64, 128)] if fk20 else [(n, c) for n in (6, 21, 48) for c in (8, 64, 128)]
            for n, c in shapes:
                cols = sorted(range(0, 128, 128 // c))[:c]

                def full():
                    K.compute_cells_and_kzg_proofs_batch_device(cells_full.data_ptr(), proofs_full.data_ptr(), db.data_ptr(), n, ts)
                    sync()

                def baseline():
                    return base.ask("compute %d" % n)

                def columns():
                    K.compute_cells_and_kzg_proofs_columns_device(cells_cols.data_ptr(), proofs_cols.data_ptr(), db.data_ptr(), n, cols, ts)
                    sync()

                def same():
                    pf = proofs_full[:n * 6144].view(n, 128, 48)[:, cols].reshape(-1)
                    cf = cells_full[:n * 262144].view(n, 128, 2048)[:, cols].reshape(-1)
                    return bool(torch.equal(pf, proofs_cols[:n * c * 48]) and torch.equal(cf, cells_cols[:n * c * 2048]))

                row("compute %s%s" % (mode_name, " FK20 on" if fk20 else ""), n, c, [("baseline", baseline if base else None), ("full", full), ("columns", columns)], same)
            if not fk20:
                for n in (6, 48):
                    K.compute_cells_and_kzg_proofs_batch_device(cells_full.data_ptr(), None, db.data_ptr(), n, ts)
                    sync()
                    given = cells_full[:n * 262144].view(n, 128, 2048)[:, EVEN].reshape(-1).clone()

                    def full():
                        K.recover_cells_and_kzg_proofs_batch_device(cells_full.data_ptr(), proofs_full.data_ptr(), EVEN, given.data_ptr(), n, ts)
                        sync()

                    def baseline():
                        return base.ask("recover %d" % n)

                    def columns():
                        K.recover_cells_and_kzg_proofs_columns_device(cells_cols.data_ptr(), proofs_cols.data_ptr(), EVEN, given.data_ptr(), n, ODD, ts)
                        sync()

                    def same():
                        pf = proofs_full[:n * 6144].view(n, 128, 48)[:, ODD].reshape(-1)
                        cf = cells_full[:n * 262144].view(n, 128, 2048)[:, ODD].reshape(-1)
                        return bool(torch.equal(pf, proofs_cols[:n * 64 * 48]) and torch.equal(cf, cells_cols[:n * 64 * 2048]))

                    row("recover 64 -> 64 %s" % mode_name, n, 64, [("baseline", baseline if base else None), ("full", full), ("columns", columns)], same)
                if mode == K.MODE_REFERENCE:
                    n, cols = 48, list(range(0, 128, 16))
                    blobs = data[:n * 131072]
                    hc, hp = C.create_string_buffer(n * 128 * 2048), C.create_string_buffer(n * 128 * 48)
                    cc, cp = C.create_string_buffer(n * 8 * 2048), C.create_string_buffer(n * 8 * 48)
                    arr = (C.c_uint64 * 8)(*cols)

                    def full():
                        assert K.lib().lwkzg_compute_cells_and_kzg_proofs_batch(hc, hp, blobs, n, ts.ref(), None) == 0

                    def baseline():
                        return base.ask("host %d" % n)

                    def columns():
                        assert K.lib().lwkzg_compute_cells_and_kzg_proofs_columns(cc, cp, blobs, n, arr, 8, ts.ref(), None) == 0

                    def same():
                        fc, fp, gc, gp = hc.raw, hp.raw, cc.raw, cp.raw
                        return all(fc[(128 * b + k) * 2048:(128 * b + k + 1) * 2048] == gc[(8 * b + i) * 2048:(8 * b + i + 1) * 2048] and
                                   fp[(128 * b + k) * 48:(128 * b + k + 1) * 48] == gp[(8 * b + i) * 48:(8 * b + i + 1) * 48]
                                   for b in range(n) for i, k in enumerate(cols))

                    row("compute host form %s" % mode_name, n, 8, [("baseline", baseline if base else None), ("full", full), ("columns", columns)], same)
            if fk20:
                ts.set_cell_proof_engine(K.CELL_PROOFS_MSM)
            ts.free()
            if base:
                base.ask("free")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if base:
        base.close()


if __name__ == "__main__":
    main()
