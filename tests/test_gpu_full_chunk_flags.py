"""GPU: blobs that raise the redo flag (P = +-Q in the hand-scheduled accumulation or in the fold stream) on the launch sets a FULL chunk
of 1024 blobs takes -- k_commit_tail<true> with its skip-fold and repair branches, four flags to a row of the second pass, the lane
fold as a launch of its own over 1024 and over 2048 units, a flag in the second chunk of a long call, c-kzg mode on the Lagrange form.
Below a full chunk tests/test_gpu_commit_tail.py and tests/test_gpu_parity.py pin the same repair; every test at 1024 blobs or more
ran honest blobs until this file. tests/flag_cases.py builds the batches and tests/test_flag_cases_cpu.py proves, without a GPU, that
their special blobs collide where they say. Byte equality throughout: closed forms from the setup's secret, the bucket engine (an
independent algorithm), and the other arm of LWKZG_COMMIT_TAIL.

The worker legs (tests/commit_tail_worker.py) run in fresh processes, where a settings object has one context: nothing is ever "busy
beside" a call and 1024 blobs take the one-wave-per-SIMD builds. The legs in this process use a settings object of their own for the
same reason (the session's may have grown a second context in the two-stream tests).
Which instantiation a launch took does not show in the library's profile (both are "k_commit_tail"); a kernel trace of the worker
confirmed k_commit_tail<true> for flags_1024 and k_commit_tail<false> for flags_1023 when this file was written, and the condition in
direct.hip (launch_direct_t) names this file."""
import pytest

import blobs as B
import flag_cases as F
from conftest import SETUP_PATH
from test_gpu_commit_tail import run_arm

pytestmark = pytest.mark.gpu

SEED = 1   # commit_tail_worker.FLAG_SEED
SHIPPED = ["k_commit_tail", "k_direct_accumulate_asm", "k_direct_redo", "k_parse_be_reduce"]


@pytest.fixture(autouse=True)
def _reference_mode(K):
    K.set_mode(K.MODE_REFERENCE)
    yield
    K.set_mode(K.MODE_REFERENCE)


@pytest.fixture(scope="module")
def arms():
    return {arm: run_arm(arm) for arm in (0, 1)}


@pytest.fixture(scope="module")
def own_setup(K):
    """a settings object no other test has used: one context, so the library never picks the two-stream geometry by itself"""
    K.set_mode(K.MODE_REFERENCE)
    ts = K.TrustedSetup.from_file(SETUP_PATH)
    assert ts.direct_table_bits() >= 10
    yield ts
    ts.free()


def _dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


def _one_launch_each(prof, names):
    assert sorted(prof) == sorted(names), prof
    assert all(prof[k]["launches"] == 1 for k in names), prof


@pytest.mark.parametrize("n", [1024, 1023])
@pytest.mark.parametrize("table", ["default", "wide"])
def test_flags(arms, oracle, table, n):
    """device-resident commitments of the flagged batch on the 13- and the 14-bit table: every special blob, both neighbours of each,
    every 61st honest blob and the last one against the closed form; no status word left set (they started as garbage); the call
    is parse, accumulate, second pass, tail and nothing else; the arm with the fold and the finalize as launches of their own
    (k_direct_fold_lanes_asm_alone at 1024) gives the same bytes. 1024: k_commit_tail<true>. 1023: <false>, and rows 0 .. 254 of
    the second pass walk four flags where row 255 walks three."""
    data, specials = F.full_chunk_batch(n, SEED)
    r = arms[1]["%s_flags_%d" % (table, n)]
    bad = F.wrong_blobs(oracle, data, specials, bytes.fromhex(r["commitments"]))
    assert not bad, (len(bad), bad[:8])
    assert r["status_sum"] == 0
    _one_launch_each(r["profile"], SHIPPED)
    old = arms[0]["%s_flags_%d" % (table, n)]
    assert old["commitments"] == r["commitments"] and old["status_sum"] == 0
    assert "k_commit_tail" not in old["profile"] and old["profile"]["k_direct_fold_lanes"]["launches"] == 1, old["profile"]


@pytest.mark.parametrize("table", ["default", "wide"])
def test_honest_after_flags_1024(arms, oracle, table):
    """an honest batch on the settings the flagged one just used: the flags and the sums it left behind are not seen again"""
    n = 1024
    r = arms[1]["%s_honest_after_flags_1024" % table]
    assert r["commitments"] == arms[1]["%s_1024" % table]["commitments"]     # (the same blobs, before any flag was ever raised)
    got = bytes.fromhex(r["commitments"])
    data = B.synthetic_batch(52000 + n, n)
    for i in sorted(set(range(0, n, 61)) | {n - 1}):
        assert got[48 * i:48 * i + 48] == F.closed_form(oracle, F.blob_scalars_at(data, i)), (table, i)
    assert r["status_sum"] == 0
    _one_launch_each(r["profile"], SHIPPED)
    assert arms[0]["%s_honest_after_flags_1024" % table]["commitments"] == r["commitments"]


def test_lincomb_flags_1024(arms):
    """the flagged batch's scalars as 1024 MSMs over the setup (lwkzg_g1_lincomb_setup_device): the commitments' bytes. The call ends in
    a compressed output per MSM, so on the shipped arm it takes the tail kernel as a commitment call does -- behind its own parse
    launch, the flags cleared by a memset --; with LWKZG_COMMIT_TAIL=0 the fold is k_direct_fold_lanes_asm_alone over 1024 units and
    the second pass behind it repairs the pairs that met in it."""
    want = arms[1]["default_flags_1024"]["commitments"]
    for arm in (0, 1):
        assert arms[arm]["lincomb_flags_1024"]["commitments"] == want, arm
    _one_launch_each(arms[1]["lincomb_flags_1024"]["profile"], SHIPPED)
    old = arms[0]["lincomb_flags_1024"]["profile"]
    assert old["k_direct_fold_lanes"]["launches"] == 1 and old["k_direct_redo"]["launches"] == 1 and "k_commit_tail" not in old, old


def test_tiled_msm_flags_1024(arms, oracle):
    """the same scalars as ONE 2^22-term MSM over the tiled setup: 1024 sums and no compressed output per tile, so on BOTH arms the lane
    fold is a launch of its own -- k_direct_fold_lanes_asm_alone over 1024 units -- and a pair that meets in it is repaired by the
    second pass behind it. The result is the sum of the 1024 commitments (added by the CPU oracle)."""
    comm = bytes.fromhex(arms[1]["default_flags_1024"]["commitments"])
    acc, acc_inf = None, True
    for i in range(1024):
        point = oracle.g1_decompress(comm[48 * i:48 * i + 48])
        assert point is not None, i
        xy, inf = point
        if inf:
            continue
        acc, acc_inf = (xy, False) if acc_inf else oracle.g1_add_affine(acc, False, xy, False)
    want = oracle.g1_compress(acc, acc_inf).hex()
    for arm in (0, 1):
        r = arms[arm]["tiled_flags_1024"]
        assert r["commitments"] == want, arm
        prof = r["profile"]
        assert prof["k_direct_fold_lanes"]["launches"] == 1 and prof["k_direct_redo"]["launches"] == 1 and "k_commit_tail" not in prof, prof


def test_ckzg_lagrange_flags_1024(arms, oracle):
    """c-kzg mode on the Lagrange form: the twins of the flagged batch (the same collisions among the points [l_i(tau)]G, little-endian
    elements below r) against their closed form [sum s_i l_i(tau)]G. The copy + range check stands where the parse kernel stood and
    the clears are memsets; the rest of the launch set is the same."""
    n = 1024
    data, specials = F.full_chunk_batch(n, SEED, lagrange=True)
    r = arms[1]["ckzg_lagrange_flags_1024"]
    bad = F.wrong_blobs(oracle, data, specials, bytes.fromhex(r["commitments"]), lagrange=True)
    assert not bad, (len(bad), bad[:8])
    assert r["status_sum"] == 0
    prof = r["profile"]
    assert all(prof[k]["launches"] == 1 for k in ("k_direct_accumulate_asm", "k_direct_redo", "k_commit_tail")), prof
    assert "k_direct_fold_lanes" not in prof and "k_finalize_compress" not in prof and "k_parse_be_reduce" not in prof, prof
    assert arms[0]["ckzg_lagrange_flags_1024"]["commitments"] == r["commitments"]


def test_commit_and_prove_flags_1024(K, own_setup, bucket_setup, arms, oracle):
    """lwkzg_commit_and_prove_batch_device at a full chunk: the hash runs beside the commitment MSM, which therefore spreads every blob
    over two workgroups -- k_direct_fold_lanes_asm over 2048 units, the second pass, k_direct_fold over two partial sums. The
    commitments: the closed forms, the worker's bytes and the bucket engine's; the proofs: the proof call's on those commitments."""
    import torch
    from lambdaworks_kzg_amd import capi
    n = 1024
    data, specials = F.full_chunk_batch(n, SEED)
    d_in = _dev(data)
    comm = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    proof = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    want_c = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    want_p = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    capi.profile_reset()
    capi.profile_enable(True)
    try:
        K.commit_and_prove_batch_device(comm.data_ptr(), proof.data_ptr(), d_in.data_ptr(), n, own_setup, None, st.data_ptr())
        torch.cuda.synchronize()
    finally:
        capi.profile_enable(False)
    prof = capi.profile_report()
    assert int(st.abs().sum()) == 0
    got = _host(comm)
    bad = F.wrong_blobs(oracle, data, specials, got)
    assert not bad, (len(bad), bad[:8])
    assert got.hex() == arms[1]["default_flags_1024"]["commitments"]
    K.blob_to_kzg_commitment_batch_device(want_c.data_ptr(), d_in.data_ptr(), n, bucket_setup, None, None)
    K.compute_blob_kzg_proof_batch_device(want_p.data_ptr(), d_in.data_ptr(), comm.data_ptr(), n, own_setup, None, st.data_ptr())
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    assert torch.equal(comm, want_c), "commitments differ from the bucket engine's"
    assert torch.equal(proof, want_p), "proofs differ from the proof call's"
    # the commitment MSM took the two-workgroups-per-blob launch set (its fold of partial sums), the proof MSM the tail kernel
    assert prof["k_direct_fold"]["launches"] == 1 and prof["k_direct_fold_lanes"]["launches"] == 1, prof
    assert prof["k_direct_redo"]["launches"] == 2 and prof["k_commit_tail"]["launches"] == 1, prof


@pytest.mark.parametrize("n", [1536, 2049])
def test_flags_in_every_chunk_of_a_long_call(K, own_setup, bucket_setup, oracle, n):
    """device-resident calls of more than one chunk: special blobs at each chunk's first and last index (1023, 1024, 1535; 2047, 2048)
    besides those of the first chunk. ALL blobs against the bucket engine on the device, the specials and a sample against the
    closed form. (2049: the third chunk is one blob, and that blob is flagged.)"""
    import torch
    data, specials = F.full_chunk_batch(n, SEED)
    assert {1023, 1024, n - 1} <= {s.index for s in specials}
    d_in = _dev(data)
    got = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    want = torch.zeros(48 * n, dtype=torch.uint8, device="cuda")
    st = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
    K.blob_to_kzg_commitment_batch_device(got.data_ptr(), d_in.data_ptr(), n, own_setup, None, st.data_ptr())
    K.blob_to_kzg_commitment_batch_device(want.data_ptr(), d_in.data_ptr(), n, bucket_setup, None, st[n:].data_ptr())
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0
    bad = F.wrong_blobs(oracle, data, specials, _host(got))
    assert not bad, (len(bad), bad[:8])
    assert torch.equal(got, want), torch.nonzero((got != want).view(n, 48).any(dim=1)).flatten()[:8].tolist()
