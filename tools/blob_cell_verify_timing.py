#!/usr/bin/env python3
"""Cell proof verification of whole blobs: the calls that take blobs against the route a caller had without
them. One MI355X, one process, default engine; per mode (reference, eth), form (host pointers, device pointers) and shape (1, 6 and 48
blobs, every input honest) the median (min, max) of --reps calls after a warm-up call of every route, the routes taking turns inside
each repetition. Every call is synchronous: the clock stops on the host result.
  new batch    lwkzg_verify_blob_cell_kzg_proofs_batch(_device)
  new groups   lwkzg_verify_blob_cell_kzg_proofs_groups(_device), one group per blob
  old batch    lwkzg_compute_cells_and_kzg_proofs_batch(_device)(cells, NULL), the commitments replicated 128 times and the indices
               0 .. 127 written out (numpy on the host, torch on the device: part of the route), lwkzg_verify_cell_kzg_proof_batch(_device)
  old groups   the same in front of lwkzg_verify_cell_kzg_proof_groups(_device) with 128 items per group
The device forms run on one stream of the caller's; the old device route's 256 KiB of cells per blob are allocated once, outside the
clock. Writes profiles/blob_cell_verify_timing.txt (or --out)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (1, 6, 48)
ROUTES = ("new batch", "old batch", "new groups", "old groups")


def random_blobs(torch, n, seed):
    """n blobs on the device: random big-endian elements with the top two bits clear (below r), good in reference and eth mode"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    b = torch.randint(0, 256, (n, 4096, 32), dtype=torch.uint8, device="cuda", generator=g)
    b[:, :, 0] &= 0x3f
    return b.reshape(-1)


def offsets(sizes):
    off = [0]
    for m in sizes:
        off.append(off[-1] + m)
    return (C.c_uint64 * len(off))(*off)


def take_turns(routes, reps):
    for fn in routes.values():
        fn()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(t), min(t), max(t)) for k, t in times.items()}


def host_routes(K, np, ts, blobs, comms, proofs, n):
    l, s = K.lib(), ts.ref()
    pu64 = C.POINTER(C.c_uint64)
    cells = C.create_string_buffer(n * 128 * 2048)
    okb, rcb = (C.c_uint8 * n)(), (C.c_int32 * n)()
    off_blobs, off_items = offsets([1] * n), offsets([128] * n)
    comm_rows = np.frombuffer(comms, dtype=np.uint8).reshape(n, 48)

    def answers():
        assert list(okb) == [1] * n and list(rcb) == [0] * n

    def new_batch():
        ok = C.c_bool(False)
        assert l.lwkzg_verify_blob_cell_kzg_proofs_batch(C.byref(ok), blobs, comms, proofs, n, s) == 0 and ok.value

    def new_groups():
        assert l.lwkzg_verify_blob_cell_kzg_proofs_groups(okb, rcb, blobs, comms, proofs, n, off_blobs, n, s) == 0
        answers()

    def old_front():
        assert l.lwkzg_compute_cells_and_kzg_proofs_batch(cells, None, blobs, n, s, None) == 0
        cm = np.repeat(comm_rows, 128, axis=0).tobytes()
        idx = np.tile(np.arange(128, dtype=np.uint64), n)
        return cm, idx

    def old_batch():
        cm, idx = old_front()
        ok = C.c_bool(False)
        assert l.lwkzg_verify_cell_kzg_proof_batch(C.byref(ok), cm, idx.ctypes.data_as(pu64), cells, proofs, 128 * n, s) == 0 and ok.value

    def old_groups():
        cm, idx = old_front()
        assert l.lwkzg_verify_cell_kzg_proof_groups(okb, rcb, cm, idx.ctypes.data_as(pu64), cells, proofs, 128 * n, off_items, n, s) == 0
        answers()

    return {"new batch": new_batch, "old batch": old_batch, "new groups": new_groups, "old groups": old_groups}


def device_routes(K, torch, ts, blobs, comms, proofs, n, stream):
    st = stream.cuda_stream
    cells = torch.empty(n * 128 * 2048, dtype=torch.uint8, device="cuda")
    ones, per_blob = [1] * n, [128] * n
    good = [(0, True)] * n

    def new_batch():
        assert K.verify_blob_cell_kzg_proofs_batch_device(blobs.data_ptr(), comms.data_ptr(), proofs.data_ptr(), n, ts, st)

    def new_groups():
        assert K.verify_blob_cell_kzg_proofs_groups_device(blobs.data_ptr(), comms.data_ptr(), proofs.data_ptr(), n, ones, ts, st) == good

    def old_front():
        with torch.cuda.stream(stream):
            K.compute_cells_and_kzg_proofs_batch_device(cells.data_ptr(), None, blobs.data_ptr(), n, ts, st)
            cm = comms[:48 * n].reshape(n, 1, 48).expand(n, 128, 48).contiguous()
            idx = torch.arange(128, dtype=torch.int64, device="cuda").repeat(n)
        return cm, idx

    def old_batch():
        cm, idx = old_front()
        assert K.verify_cell_kzg_proof_batch_device(cm.data_ptr(), idx.data_ptr(), cells.data_ptr(), proofs.data_ptr(), 128 * n, ts, st)

    def old_groups():
        cm, idx = old_front()
        assert K.verify_cell_kzg_proof_groups_device(cm.data_ptr(), idx.data_ptr(), cells.data_ptr(), proofs.data_ptr(), 128 * n, per_blob, ts,
                                                     st) == good

    return {"new batch": new_batch, "old batch": old_batch, "new groups": new_groups, "old groups": old_groups}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blob_cell_verify_timing.txt"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import lambdaworks_kzg_amd as K
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    ts = K.TrustedSetup.from_file(os.path.join(ROOT, "tests", "golden", "trusted_setup.txt"))
    n_max = max(SHAPES)
    stream = torch.cuda.Stream()
    lines = ["# cell proofs of whole blobs: the calls over blobs against compute-cells + arrays + the calls over items; engine direct_bits=%d; "
             "one process; median of %d calls after a warm-up call, the routes taking turns (min, max); ms per call"
             % (ts.direct_table_bits(), a.reps)]
    for mode, mode_name in ((K.MODE_REFERENCE, "reference"), (K.MODE_ETH, "eth")):
        ts.set_mode(mode)
        blobs = random_blobs(torch, n_max, 5 + mode)
        comms = torch.empty(n_max * 48, dtype=torch.uint8, device="cuda")
        proofs = torch.empty(n_max * 128 * 48, dtype=torch.uint8, device="cuda")
        K.blob_to_kzg_commitment_batch_device(comms.data_ptr(), blobs.data_ptr(), n_max, ts)
        K.compute_cells_and_kzg_proofs_batch_device(None, proofs.data_ptr(), blobs.data_ptr(), n_max, ts)
        torch.cuda.synchronize()
        h_blobs, h_comms, h_proofs = (bytes(t.cpu().numpy().tobytes()) for t in (blobs, comms, proofs))
        for form in ("host", "device"):
            for n in SHAPES:
                if form == "host":
                    routes = host_routes(K, np, ts, h_blobs[:n * 4096 * 32], h_comms[:48 * n], h_proofs[:n * 128 * 48], n)
                else:
                    routes = device_routes(K, torch, ts, blobs, comms, proofs, n, stream)
                res = take_turns(routes, a.reps)
                lines.append("## %s mode, %s form, %d blob%s" % (mode_name, form, n, "" if n == 1 else "s"))
                for k in ROUTES:
                    lines.append("%-12s %9.3f  (min %.3f, max %.3f)" % ((k,) + res[k]))
                for kind in ("batch", "groups"):
                    new, old = res["new " + kind], res["old " + kind]
                    gap, spread = old[0] - new[0], old[2] - old[1]
                    lines.append("%s: old median minus new median %.3f ms; the old route's own min-max range %.3f ms -> the new call is %s"
                                 % (kind, gap, spread, "ahead by more than that range" if gap > spread else
                                    "ahead, within that range" if gap > 0 else "not ahead"))
    ts.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
