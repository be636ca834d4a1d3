"""GPU: the piece boundaries of the EIP-7594 calls' host code -- what feeds the kernels of tests/test_gpu_cells.py, test_gpu_recover.py and
test_gpu_cell_verify.py in slices and chunks. A: the host-pointer forms across the 64-blob slice (64 | 65), first_bad and the untouched
outputs of a rejection from the second slice, a good call after it. B: the device forms across the 512-blob cells-only chunk (512 | 513),
the status words of blobs beyond the first chunk, one bad blob in each 8-blob proof chunk. C: two caller streams with no host
synchronisation between the calls, and a workspace that grows in between. D: the capacity steps of the cell verification's grow-only
buffers (256 | 257, and smaller calls after larger ones). E: where the altered element of an inconsistent recovery sits.

Expected values never come from the call under test: (1) the restatement of tests/cells_spec.py and the closed form over the known tau
for the blobs next to a boundary; (2) calls of at most 8 blobs, which the neighbouring files hold against the restatement, for every
blob of a large batch; (3) in c-kzg mode the first 64 cells of a blob are the blob's own bytes, for every blob."""
import ctypes as C

import pytest

import blobs as B
import cell_verify_spec as V
import cells_spec as S
import recover_spec as RS
import test_gpu_cell_verify as TV
import test_gpu_cells as TC
import test_gpu_recover as TR
from conftest import R, SETUP_PATH, TAU, tau_closed_form

pytestmark = pytest.mark.gpu

REF, CKZG = S.MODE_REFERENCE, S.MODE_CKZG
MODES = [REF, CKZG]
CELL = 2048
BLOB = 4096 * 32
CELLS = 128 * CELL      # the 128 cells of one blob
PROOFS = 128 * 48       # its 128 proofs
FILL = 0x5a
_mode = TC._mode
_cache = {}


def teardown_module(module):
    """the shared batches (a few hundred MiB of host bytes) go when the module is done"""
    _cache.clear()


def _batch(first, count, mode):
    return B.synthetic_batch(first, count, big_endian=mode == REF)


def _blob_of(data, b):
    return data[BLOB * b:BLOB * (b + 1)]


def _cells_of(flat):
    """256 KiB -> the 128 cells"""
    return [flat[CELL * k:CELL * (k + 1)] for k in range(128)]


def _flat(per_blob):
    """[(cells, proofs)] as the wrappers split them -> [(256 KiB, 6 KiB)], either None where it was left out"""
    return [(None if c is None else b"".join(c), None if p is None else b"".join(p)) for c, p in per_blob]


def _in_groups_of_8(K, ts, data, proofs=True):
    """source 2: every blob of `data` through host-form calls of at most 8 blobs"""
    n = len(data) // BLOB
    out = []
    for off in range(0, n, 8):
        out += _flat(K.compute_cells_and_kzg_proofs_batch(data[BLOB * off:BLOB * min(off + 8, n)], ts, proofs=proofs))
    return out


def _restated_cells(blob, mode):
    """source 1, the 128 cells concatenated"""
    return b"".join(S.cells_bytes(S.poly_from_blob(blob, mode), mode))


def _restated_proofs(oracle, blob, mode, ks=(0, 63, 64, 127)):
    p = S.poly_from_blob(blob, mode)
    return {k: tau_closed_form(oracle, S.quotient(p, k)) for k in ks}


def _per_blob(buf, size):
    """a host form's output buffer -> `size` bytes per blob"""
    raw = buf.raw
    assert len(raw) % size == 0
    return [raw[size * b:size * (b + 1)] for b in range(len(raw) // size)]


def _joined_cells(got):
    """the device helpers' split result -> 256 KiB per blob"""
    return [b"".join(c) for c, _ in got]


def _wrong_blobs(got, want, skip=()):
    """the blobs whose piece of `got` is not want[b]: a failure names the blob and renders no 128 MiB diff"""
    assert len(got) == len(want)
    return [b for b in range(len(want)) if b not in skip and got[b] != want[b]]


def _not_their_own_bytes(got, data, skip=()):
    """source 3 (c-kzg mode), on 256 KiB of cells per blob: cells 0 .. 63, concatenated, are the blob's bytes"""
    return [b for b in range(len(got)) if b not in skip and got[b][:BLOB] != _blob_of(data, b)]


def _out_buffers(n, cells=True, proofs=True):
    oc = C.create_string_buffer(bytes([FILL]) * (n * CELLS), n * CELLS) if cells else None
    op = C.create_string_buffer(bytes([FILL]) * (n * PROOFS), n * PROOFS) if proofs else None
    return oc, op


def _untouched(oc, op):
    return (oc is None or oc.raw == bytes([FILL]) * len(oc.raw)) and (op is None or op.raw == bytes([FILL]) * len(op.raw))


def _host_compute(K, ts, data, cells=True, proofs=True):
    """lwkzg_compute_cells_and_kzg_proofs_batch on prefilled outputs: (rc, first_bad, cells buffer, proofs buffer)"""
    n = len(data) // BLOB
    oc, op = _out_buffers(n, cells, proofs)
    first_bad = C.c_size_t(12345)
    rc = K.lib().lwkzg_compute_cells_and_kzg_proofs_batch(oc, op, data, n, ts.ref(), C.byref(first_bad))
    return rc, first_bad.value, oc, op


def _host_recover(K, ts, idx, given, n, cells=True, proofs=True):
    """lwkzg_recover_cells_and_kzg_proofs_batch on prefilled outputs: (rc, first_bad, cells buffer, proofs buffer)"""
    assert len(given) == n * len(idx) * CELL
    oc, op = _out_buffers(n, cells, proofs)
    first_bad = C.c_size_t(12345)
    arr = (C.c_uint64 * len(idx))(*idx)
    rc = K.lib().lwkzg_recover_cells_and_kzg_proofs_batch(oc, op, arr, given, len(idx), n, ts.ref(), C.byref(first_bad))
    return rc, first_bad.value, oc, op


def _given_of(want_cells, idx):
    """the given cells of every blob (want_cells: 256 KiB per blob), blob-major"""
    return b"".join(TR._given(_cells_of(w), idx) for w in want_cells)


def _spoil(given, num, b, i, t, mode, value=None):
    """element t of the i-th given cell of blob b replaced (TR._alter), in the blob-major cells of a batch with num cells per blob"""
    at = num * CELL * b
    return given[:at] + TR._alter(given[at:at + num * CELL], i, t, mode, value=value) + given[at + num * CELL:]


def _with_element_r(data, b, elem=100):
    """c-kzg blob b of `data` with element `elem` equal to r"""
    at = BLOB * b + 32 * elem
    return data[:at] + R.to_bytes(32, "little") + data[at + 32:]


# ------------------------------------------------------------------------------------------------ A. the 64-blob slice of the host forms

def _batch65(K, ts, mode):
    """70 blobs, and (cells, proofs) of the first 65 by calls of at most 8: made once per mode"""
    if ("65", mode) not in _cache:
        data = _batch(2000, 70, mode)
        with _mode(K, ts, mode):
            _cache[("65", mode)] = (data, _in_groups_of_8(K, ts, data[:65 * BLOB]))
    return _cache[("65", mode)]


@pytest.mark.parametrize("mode", MODES)
def test_compute_host_form_across_the_slice(K, gpu_setup, oracle, mode):
    """n = 65 is a slice of 64 and a slice of one: the second upload, download and h_status + off; n = 64 is one full slice"""
    data70, want = _batch65(K, gpu_setup, mode)
    data = data70[:65 * BLOB]
    with _mode(K, gpu_setup, mode):
        rc, _, oc, op = _host_compute(K, gpu_setup, data)
        assert rc == K.C_KZG_OK
        cells, proofs = _per_blob(oc, CELLS), _per_blob(op, PROOFS)
        assert _wrong_blobs(cells, [w[0] for w in want]) == []
        assert _wrong_blobs(proofs, [w[1] for w in want]) == []
        rc, _, oc, op = _host_compute(K, gpu_setup, data[:64 * BLOB])
        assert rc == K.C_KZG_OK
        assert _wrong_blobs(_per_blob(oc, CELLS), [w[0] for w in want[:64]]) == []
        assert _wrong_blobs(_per_blob(op, PROOFS), [w[1] for w in want[:64]]) == []
    for b in (63, 64):   # the last blob of the first slice and the only one of the second against the restatement
        assert cells[b] == _restated_cells(_blob_of(data, b), mode), b
        for k, pi in _restated_proofs(oracle, _blob_of(data, b), mode).items():
            assert proofs[b][48 * k:48 * (k + 1)] == pi, (b, k)
    if mode == CKZG:
        assert _not_their_own_bytes(cells, data) == []


@pytest.mark.parametrize("mode", MODES)
def test_recover_host_form_across_the_slice(K, gpu_setup, mode):
    """n = 65 through recover_host: both outputs, the proofs left out, and 100 given cells (the staging's in_bytes goes by num_cells)"""
    _, want = _batch65(K, gpu_setup, mode)
    want_c, want_p = [w[0] for w in want], [w[1] for w in want]
    with _mode(K, gpu_setup, mode):
        for count, seed, proofs in [(64, 200, True), (64, 201, False), (100, 202, True)]:
            idx = TR._pick(count, seed)
            rc, _, oc, op = _host_recover(K, gpu_setup, idx, _given_of(want_c, idx), 65, proofs=proofs)
            assert rc == K.C_KZG_OK, (count, proofs)
            assert _wrong_blobs(_per_blob(oc, CELLS), want_c) == [], (count, proofs)
            if proofs:
                assert _wrong_blobs(_per_blob(op, PROOFS), want_p) == [], count


def test_compute_rejection_from_the_second_slice(K, gpu_setup):
    """c-kzg mode, n = 70: an element equal to r in blobs 64 and 69 (positions 0 and 5 of the second slice), then in blob 3 as well; a
    good call right after each rejected one (status words and staging are per call)"""
    data70, want = _batch65(K, gpu_setup, CKZG)
    bad = _with_element_r(_with_element_r(data70, 64), 69, elem=4095)
    with _mode(K, gpu_setup, CKZG):
        for spoilt, first in [(bad, 64), (_with_element_r(bad, 3, elem=0), 3)]:
            rc, first_bad, oc, op = _host_compute(K, gpu_setup, spoilt)
            assert rc == K.C_KZG_BADARGS and first_bad == first
            assert _untouched(oc, op)
            rc, _, oc, op = _host_compute(K, gpu_setup, data70[:65 * BLOB])
            assert rc == K.C_KZG_OK
            assert _wrong_blobs(_per_blob(oc, CELLS), [w[0] for w in want]) == []
            assert _wrong_blobs(_per_blob(op, PROOFS), [w[1] for w in want]) == []
            assert _not_their_own_bytes(_per_blob(oc, CELLS), data70) == []


@pytest.mark.parametrize("mode", MODES)
def test_recover_rejection_from_the_second_slice(K, gpu_setup, mode):
    """n = 67, 65 given cells: an element not below r in blob 64 and inconsistent cells in blob 66; then a good call"""
    data70, want = _batch65(K, gpu_setup, mode)
    idx = TR._pick(65, 210)
    with _mode(K, gpu_setup, mode):
        extra = _in_groups_of_8(K, gpu_setup, data70[65 * BLOB:67 * BLOB], proofs=False)
        good = _given_of([w[0] for w in want] + [e[0] for e in extra], idx)
        bad = _spoil(_spoil(good, 65, 64, 0, 0, mode, value=R), 65, 66, 64, 63, mode)
        rc, first_bad, oc, op = _host_recover(K, gpu_setup, idx, bad, 67)
        assert rc == TR._bad_code(K, mode) and first_bad == 64
        assert _untouched(oc, op)
        rc, _, oc, op = _host_recover(K, gpu_setup, idx, good[:65 * 65 * CELL], 65)
        assert rc == K.C_KZG_OK
        assert _wrong_blobs(_per_blob(oc, CELLS), [w[0] for w in want]) == []
        assert _wrong_blobs(_per_blob(op, PROOFS), [w[1] for w in want]) == []


# ------------------------------------------------------------------------------------------------ B. the 512-blob chunk of the device forms

def _batch513(K, ts, mode):
    """513 blobs and their cells by cells-only calls of at most 8: made once per mode"""
    if ("513", mode) not in _cache:
        data = _batch(3000, 513, mode)
        with _mode(K, ts, mode):
            _cache[("513", mode)] = (data, [w[0] for w in _in_groups_of_8(K, ts, data, proofs=False)])
    return _cache[("513", mode)]


@pytest.mark.parametrize("mode", MODES)
def test_compute_device_form_across_the_cells_chunk(K, gpu_setup, mode):
    """proofs48_dev = NULL: chunks of 512 blobs, so n = 513 is a chunk of 512 and a chunk of one (status + off, blobs + off * ..., cells
    + off * ...), and n = 512 puts 1024 transforms into the workspace's 1024 slots: the last slot"""
    import torch
    data, want = _batch513(K, gpu_setup, mode)
    with _mode(K, gpu_setup, mode):
        for n in (513, 512):
            got, status = TC._device(K, torch, data[:n * BLOB], gpu_setup, proofs=False)
            got = _joined_cells(got)
            assert status == [0] * n
            assert _wrong_blobs(got, want[:n]) == [], n
            if mode == CKZG:
                assert _not_their_own_bytes(got, data) == [], n
    for b in (0, 511, 512):   # the restatement at the start and on both sides of the boundary (both calls have been held equal to `want`)
        assert want[b] == _restated_cells(_blob_of(data, b), mode), b


def test_recover_device_form_across_the_cells_chunk(K, gpu_setup):
    """recovered_proofs48_dev = NULL, n = 513, c-kzg mode, 64 given cells (random_64): the cells are those of the original blobs, which
    the test above pins; blob 512 also against the restated spec's reconstruction"""
    import torch
    data, want = _batch513(K, gpu_setup, CKZG)
    idx = dict(TR.PATTERNS)["random_64"]
    given = _given_of(want, idx)
    with _mode(K, gpu_setup, CKZG):
        got, status = TR._device(K, torch, idx, given, 513, gpu_setup, proofs=False)
    got = _joined_cells(got)
    assert status == [0] * 513
    assert _wrong_blobs(got, want) == []
    assert _not_their_own_bytes(got, data) == []
    last = given[512 * 64 * CELL:]
    values = [[S.element(last[CELL * i + 32 * t:CELL * i + 32 * t + 32], CKZG) for t in range(64)] for i in range(64)]
    coeffs = RS.recover_polynomialcoeff(idx, values)
    assert not any(coeffs[4096:])
    assert got[512] == b"".join(S.cells_bytes(coeffs[:4096], CKZG))


def test_status_across_the_cells_chunk_compute(K, gpu_setup):
    """c-kzg mode, n = 513, an element equal to r in blobs 511 and 512: the last word of the first chunk and the only one of the second"""
    import torch
    data, want = _batch513(K, gpu_setup, CKZG)
    bad = _with_element_r(_with_element_r(data, 511, elem=4095), 512, elem=0)
    with _mode(K, gpu_setup, CKZG):
        got, status = TC._device(K, torch, bad, gpu_setup, proofs=False)
    assert [b for b, s in enumerate(status) if s != 0] == [511, 512]
    assert status[511] == status[512] == K.C_KZG_BADARGS
    got = _joined_cells(got)
    assert got[0] == want[0] and got[510] == want[510]
    assert _wrong_blobs(got, want, skip=(511, 512)) == []
    assert _not_their_own_bytes(got, data, skip=(511, 512)) == []


def test_status_across_the_cells_chunk_recover(K, gpu_setup):
    """reference mode, n = 513, 65 given cells: a non-canonical element in blob 0 and inconsistent cells in blob 512"""
    import torch
    _, want = _batch513(K, gpu_setup, REF)
    idx = TR._pick(65, 220)
    given = _spoil(_spoil(_given_of(want, idx), 65, 0, 64, 63, REF, value=2 ** 256 - 1), 65, 512, 0, 0, REF)
    with _mode(K, gpu_setup, REF):
        got, status = TR._device(K, torch, idx, given, 513, gpu_setup, proofs=False)
    assert [b for b, s in enumerate(status) if s != 0] == [0, 512]
    assert status[0] == status[512] == K.C_KZG_ERROR
    assert _wrong_blobs(_joined_cells(got), want, skip=(0, 512)) == []


def test_compute_host_form_cells_only_n513(K, gpu_setup):
    """the same batch through the host form, cells only: nine slices, the last of one blob"""
    data, want = _batch513(K, gpu_setup, CKZG)
    with _mode(K, gpu_setup, CKZG):
        rc, _, oc, _ = _host_compute(K, gpu_setup, data, proofs=False)
    assert rc == K.C_KZG_OK
    cells = _per_blob(oc, CELLS)
    assert _wrong_blobs(cells, want) == []
    assert _not_their_own_bytes(cells, data) == []


def test_proof_chunks_with_bad_blobs_compute(K, gpu_setup):
    """c-kzg mode, n = 17 with proofs through the device form: one bad blob in each chunk of 8 (0, 8, 16)"""
    import torch
    data = _batch(3600, 17, CKZG)
    bad = data
    for b in (0, 8, 16):
        bad = _with_element_r(bad, b, elem=17 * b)
    with _mode(K, gpu_setup, CKZG):
        singles = [K.compute_cells_and_kzg_proofs(_blob_of(data, b), gpu_setup) for b in range(17)]
        got, status = TC._device(K, torch, bad, gpu_setup)
    assert [b for b, s in enumerate(status) if s != 0] == [0, 8, 16]
    assert [b for b in range(17) if b not in (0, 8, 16) and got[b] != singles[b]] == []
    assert _not_their_own_bytes(_joined_cells(got), data, skip=(0, 8, 16)) == []


def test_proof_chunks_with_bad_blobs_recover(K, gpu_setup):
    """reference mode, n = 17 with proofs through the device form, 65 given cells: an element not below r in blob 0, inconsistent cells in
    blobs 8 and 16"""
    import torch
    data = _batch(3700, 17, REF)
    idx = TR._pick(65, 230)
    with _mode(K, gpu_setup, REF):
        singles = [K.compute_cells_and_kzg_proofs(_blob_of(data, b), gpu_setup) for b in range(17)]
        given = b"".join(TR._given(c, idx) for c, _ in singles)
        given = _spoil(_spoil(_spoil(given, 65, 0, 7, 7, REF, value=R), 65, 8, 0, 63, REF), 65, 16, 64, 0, REF)
        got, status = TR._device(K, torch, idx, given, 17, gpu_setup)
    assert [b for b, s in enumerate(status) if s != 0] == [0, 8, 16]
    assert [status[b] for b in (0, 8, 16)] == [K.C_KZG_ERROR] * 3
    assert [b for b in range(17) if b not in (0, 8, 16) and got[b] != singles[b]] == []


# ------------------------------------------------------------------------------------------------ C. two caller streams

class _Pending:
    """a device-form call's buffers: allocated and filled before the calls are issued, read after the streams are synchronised"""

    def __init__(self, torch, n, inputs, cells=True, proofs=True):
        self.n = n
        self.din = TC._dev(torch, inputs)
        self.dc = torch.zeros(n * CELLS, dtype=torch.uint8, device="cuda") if cells else None
        self.dp = torch.zeros(n * PROOFS, dtype=torch.uint8, device="cuda") if proofs else None
        self.ds = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def ptrs(self):
        return self.dc.data_ptr() if self.dc is not None else None, self.dp.data_ptr() if self.dp is not None else None

    def compute(self, K, ts, stream):
        oc, op = self.ptrs()
        K.compute_cells_and_kzg_proofs_batch_device(oc, op, self.din.data_ptr(), self.n, ts, stream.cuda_stream, self.ds.data_ptr())

    def recover(self, K, ts, stream, idx):
        oc, op = self.ptrs()
        K.recover_cells_and_kzg_proofs_batch_device(oc, op, idx, self.din.data_ptr(), self.n, ts, stream.cuda_stream, self.ds.data_ptr())

    def result(self, K):
        cr = bytes(self.dc.cpu().numpy()) if self.dc is not None else None
        pr = bytes(self.dp.cpu().numpy()) if self.dp is not None else None
        return K.capi._cells_split(cr, pr, self.n), self.ds.cpu().tolist()


def _both(torch, first, second):
    """issue two calls on two streams with no host synchronisation between them; then wait for both"""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()   # the buffers are ready before either stream starts
    first(s1)
    second(s2)
    s1.synchronize()
    s2.synchronize()


def test_two_recover_calls_on_two_streams(K, gpu_setup):
    """Two recover_..._batch_device calls with different index sets and blobs, back to back on two streams: k_recover_setup rewrites
    the context's recover_tab at every call, and the table and the workspace pass from stream to stream only through WsUse. Passing once
    on an idle machine proves nothing: the test is here to fail when the WsUse hand-over is removed. Not looped to hunt for a race."""
    import torch
    pats = dict(TR.PATTERNS)
    ia, ib = pats["cells_0_to_63"], pats["odd"]
    with _mode(K, gpu_setup, CKZG):
        wa = K.compute_cells_and_kzg_proofs_batch(_batch(4000, 3, CKZG), gpu_setup)
        wb = K.compute_cells_and_kzg_proofs_batch(_batch(4010, 3, CKZG), gpu_setup)
    ga, gb = b"".join(TR._given(c, ia) for c, _ in wa), b"".join(TR._given(c, ib) for c, _ in wb)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        with _mode(K, ts, CKZG):
            for swapped in (False, True):
                pa, pb = _Pending(torch, 3, ga), _Pending(torch, 3, gb)
                calls = [lambda s: pa.recover(K, ts, s, ia), lambda s: pb.recover(K, ts, s, ib)]
                _both(torch, *(calls[::-1] if swapped else calls))
                assert pa.result(K) == (wa, [0, 0, 0]), swapped
                assert pb.result(K) == (wb, [0, 0, 0]), swapped
    finally:
        ts.free()


def test_cells_only_call_then_a_proofs_call_on_another_stream(K, gpu_setup):
    """On a new settings object a cells-only call of 2 blobs reserves 4 workspace slots; the call with proofs that follows at once on
    another stream reserves 256, and ctx_reserve frees and reallocates while the first call may be in flight, behind its device-wide
    synchronisation. The test is here to fail when that synchronisation (or the WsUse hand-over) is removed; passing once on an idle
    machine proves nothing. Not looped."""
    import torch
    da, db = _batch(4020, 2, REF), _batch(4030, 2, REF)
    with _mode(K, gpu_setup, REF):
        wa = K.compute_cells_and_kzg_proofs_batch(da, gpu_setup, proofs=False)
        wb = K.compute_cells_and_kzg_proofs_batch(db, gpu_setup)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        with _mode(K, ts, REF):
            pa, pb = _Pending(torch, 2, da, proofs=False), _Pending(torch, 2, db)
            _both(torch, lambda s: pa.compute(K, ts, s), lambda s: pb.compute(K, ts, s))
            assert pa.result(K) == (wa, [0, 0])
            assert pb.result(K) == (wb, [0, 0])
    finally:
        ts.free()


def test_recover_and_compute_interleaved_on_two_streams(K, gpu_setup):
    """recover, compute, recover, compute on alternating streams without a host synchronisation in between: the two pipelines share
    ws.scalars, ws.scalars2 and ws.fr. Here to fail when the WsUse hand-over is removed; passing once proves nothing. Not looped."""
    import torch
    idx = dict(TR.PATTERNS)["even"]
    datas = [_batch(4040 + 10 * j, 3, REF) for j in range(4)]
    with _mode(K, gpu_setup, REF):
        wants = [K.compute_cells_and_kzg_proofs_batch(d, gpu_setup) for d in datas]
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        with _mode(K, ts, REF):
            pend = [_Pending(torch, 3, b"".join(TR._given(c, idx) for c, _ in wants[j]) if j % 2 == 0 else datas[j]) for j in range(4)]
            s = [torch.cuda.Stream(), torch.cuda.Stream()]
            torch.cuda.synchronize()
            for j, p in enumerate(pend):
                if j % 2 == 0:
                    p.recover(K, ts, s[0], idx)
                else:
                    p.compute(K, ts, s[1])
            s[0].synchronize()
            s[1].synchronize()
            for j, p in enumerate(pend):
                assert p.result(K) == (wants[j], [0, 0, 0]), j
    finally:
        ts.free()


# ------------------------------------------------------------------------------------------------ D. cell verification: capacity steps

def _items384(K, ts, mode):
    """the 384 (commitment, index, cell, proof) of three blobs, made by the library as test_large_batch_made_by_the_library makes them"""
    if ("items", mode) not in _cache:
        data = _batch(5000, 3, mode)
        with _mode(K, ts, mode):
            comms = K.blob_to_kzg_commitment_batch(data, ts)
            made = K.compute_cells_and_kzg_proofs_batch(data, ts)
        _cache[("items", mode)] = ([(comms[b], k, made[b][0][k], made[b][1][k]) for b in range(3) for k in range(128)], comms)
    return _cache[("items", mode)]


def _challenge_host(K, items, mode):
    return K.cell_batch_challenge_host([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], mode)


def _device_rc(K, torch, ts, items):
    """lwkzg_verify_cell_kzg_proof_batch_device: (rc, *ok)"""
    dc, dcell, dp = TC._dev(torch, b"".join(i[0] for i in items)), TC._dev(torch, b"".join(i[2] for i in items)), TC._dev(torch, b"".join(i[3] for i in items))
    di = torch.tensor([i[1] for i in items], dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    ok = C.c_bool(True)
    rc = K.lib().lwkzg_verify_cell_kzg_proof_batch_device(C.byref(ok), dc.data_ptr(), di.data_ptr(), dcell.data_ptr(), dp.data_ptr(), len(items),
                                                          ts.ref(), None)
    return rc, bool(ok.value)


@pytest.mark.parametrize("mode", MODES)
def test_cell_verification_across_the_capacity_steps(K, gpu_setup, mode):
    """On a new settings object, in this order: n = 1, 255, 256 (the first capacity), 257 (the buffers double; the pinned block is laid
    out by capacity: digests at 0, status words at 32 * cap, tail at 36 * cap), 300, then 256 and 1 again in the larger buffers. Every
    n: the honest verdict, r against the host-only transcript (a check on the digests that came down), three corruptions of the last
    item. A non-canonical element in the last item at the first 256 (capacity 256: the status words at 32 * 256), at 257 and at the
    second 256 (capacity 512: at 32 * 512). Last, the device form with an index of 128."""
    import torch
    all_items, comms = _items384(K, gpu_setup, mode)
    bad_code = K.C_KZG_BADARGS if mode == CKZG else K.C_KZG_ERROR
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        with _mode(K, ts, mode):
            for n in (1, 255, 256, 257, 300, 256, 1):
                items = all_items[:n]
                c, k, cell, proof = items[-1]
                assert TV._verify(K, ts, items) is True, n
                assert TV._partials(K, ts, items)[:32] == _challenge_host(K, items, mode), n
                at = 32 * 21 + (31 if mode == REF else 0)   # the low byte of an element
                flipped = cell[:at] + bytes([cell[at] ^ 1]) + cell[at + 1:]
                other_proof = all_items[0 if n > 1 else 1][3]   # the first item's (at n = 1 the last item is the first: the next one's)
                other_comm = comms[(comms.index(c) + 1) % 3]
                for name, bad in [("cell byte", (c, k, flipped, proof)), ("proof", (c, k, cell, other_proof)),
                                  ("commitment", (other_comm, k, cell, proof))]:
                    assert TV._rc(K, ts, items[:-1] + [bad]) == (K.C_KZG_OK, False), (n, name)
                if n in (256, 257):   # capacity 256 (the status words at 32 * 256 of the pinned block), then 512 twice
                    big = cell[:32 * 63] + S.to_bytes(R, mode)
                    assert TV._rc(K, ts, items[:-1] + [(c, k, big, proof)]) == (bad_code, False), n
                    assert TV._rc(K, ts, items) == (K.C_KZG_OK, True), n
            items = all_items[:300]
            assert _device_rc(K, torch, ts, items) == (K.C_KZG_OK, True)
            c, k, cell, proof = items[150]
            assert _device_rc(K, torch, ts, items[:150] + [(c, 128, cell, proof)] + items[151:]) == (K.C_KZG_BADARGS, False)
            assert _device_rc(K, torch, ts, items) == (K.C_KZG_OK, True)
    finally:
        ts.free()


def test_the_four_sums_at_257_items(K, gpu_setup, oracle):
    """r and the four sums of a batch one item above the first capacity, as the first call on a new settings object (the buffers go
    straight to 512 items), against the restatement of tests/cell_verify_spec.py. At n = 257, not at the fallback of 65: measured at 1.5 s on an MI355X,
    in a run where the slowest tests of test_gpu_cells.py and test_gpu_recover.py took 5.7 s and 2.8 s."""
    items = _items384(K, gpu_setup, REF)[0][:257]
    want = V.partials_bytes(oracle, items, REF, TAU)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    try:
        with _mode(K, ts, REF):
            got = TV._partials(K, ts, items)
    finally:
        ts.free()
    assert got == want


# ------------------------------------------------------------------------------------------------ E. recovery: where the altered element sits

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", [65, 127, 128])
def test_inconsistent_cells_wherever_the_altered_element_sits(K, gpu_setup, mode, count):
    """the first and the last given cell, element 0 and element 63, in the middle blob of three: the mode's code, nothing written. At
    127 cells Zs has one factor, at 128 none."""
    idx = TR._pick(count, 240 + count)
    with _mode(K, gpu_setup, mode):
        full = _in_groups_of_8(K, gpu_setup, _batch(6000 + count, 3, mode), proofs=False)
        good = _given_of([f[0] for f in full], idx)
        for i in (0, count - 1):
            for t in (0, 63):
                rc, first_bad, oc, op = _host_recover(K, gpu_setup, idx, _spoil(good, count, 1, i, t, mode), 3)
                assert rc == TR._bad_code(K, mode) and first_bad == 1, (i, t)
                assert _untouched(oc, op), (i, t)
        rc, _, oc, _ = _host_recover(K, gpu_setup, idx, good, 3, proofs=False)
        assert rc == K.C_KZG_OK
        assert _wrong_blobs(_per_blob(oc, CELLS), [f[0] for f in full]) == []


@pytest.mark.parametrize("mode", MODES)
def test_a_cell_of_the_same_blob_under_the_wrong_index(K, gpu_setup, mode):
    """cell idx[5]'s bytes delivered at position 6 as well. With 65 cells that is inconsistent; with exactly 64 it is the polynomial
    through what was given."""
    with _mode(K, gpu_setup, mode):
        full, _ = K.compute_cells_and_kzg_proofs(TR._blob(6500, mode), gpu_setup, proofs=False)
        for count in (65, 64):
            idx = TR._pick(count, 250 + count)
            given = TR._given(full, idx)
            given = given[:6 * CELL] + given[5 * CELL:6 * CELL] + given[7 * CELL:]
            assert given[6 * CELL:7 * CELL] == full[idx[5]] != full[idx[6]]
            if count == 65:
                rc, _, oc, op = _host_recover(K, gpu_setup, idx, given, 1)
                assert rc == TR._bad_code(K, mode)
                assert _untouched(oc, op)
            else:
                cells, _ = K.recover_cells_and_kzg_proofs(idx, given, gpu_setup, proofs=False)
                assert b"".join(cells[k] for k in idx) == given
                assert cells != full


@pytest.mark.parametrize("mode", MODES)
def test_an_element_equal_to_r_minus_1_is_a_value(K, gpu_setup, mode):
    """With 64 cells the call answers and the given cells come back unchanged; with 65, on a blob that did not have r - 1 there, the
    cells are inconsistent. That rejection and the one of an element not below r share the code and the wrapper's error text, so
    which of the two it was is not checked."""
    with _mode(K, gpu_setup, mode):
        full, _ = K.compute_cells_and_kzg_proofs(TR._blob(6600, mode), gpu_setup, proofs=False)
        idx = TR._pick(64, 260)
        given = TR._alter(TR._given(full, idx), 63, 63, mode, value=R - 1)
        assert given != TR._given(full, idx)
        cells, _ = K.recover_cells_and_kzg_proofs(idx, given, gpu_setup, proofs=False)
        assert b"".join(cells[k] for k in idx) == given
        idx = TR._pick(65, 261)
        given = TR._alter(TR._given(full, idx), 64, 63, mode, value=R - 1)
        rc, _, oc, op = _host_recover(K, gpu_setup, idx, given, 1)
        assert rc == TR._bad_code(K, mode)
        assert _untouched(oc, op)
