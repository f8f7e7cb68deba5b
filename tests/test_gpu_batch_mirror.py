"""batch_commit / batch_open through the host mirror (zinc_amd/pcs.py -> libzinc_zip.so -> libzip_hip.so) at the shape
of the reference's test_zip_batch_evaluation (tests.rs:148: n = 8, m = 10): the batched device path against the loop
over commit / open, byte for byte and transcript state for transcript state."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODULUS = 57316695564490278656402085503
FL = 4
N, M = 8, 10


@pytest.fixture(scope="module")
def pcs():
    from zinc_amd import cabi, pcs as m

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


@pytest.fixture(scope="module")
def case(pcs):
    t = pcs.KeccakTranscript()
    pp = pcs.MultilinearZip.setup(1 << N, pcs.RaaCode(1 << N, t))
    rng = np.random.default_rng(5)
    mles = [rng.integers(-128, 128, size=1 << N, dtype=np.int64) for _ in range(M)]
    field = pcs.FieldConfig(MODULUS, FL)
    points_int = [rng.integers(-128, 128, size=N, dtype=np.int64) for _ in range(M)]  # a different point per polynomial
    points = [field.map_to_field(p) for p in points_int]
    return pp, mles, field, points_int, points


def _int_mle_eval(evals, point):
    cur = [int(x) for x in evals]
    for p in point:
        cur = [cur[2 * b] + int(p) * (cur[2 * b + 1] - cur[2 * b]) for b in range(len(cur) // 2)]
    return cur[0]


def _run(pcs, case, order=None, split=None):
    """batch_commit + batch_open on a fresh PcsTranscript -> (stream bytes, probe, commitments)"""
    pp, mles, field, _, points = case
    if split:  # the datas of two different batches
        outs = pcs.MultilinearZip.batch_commit(pp, mles[:split]) + pcs.MultilinearZip.batch_commit(pp, mles[split:])
    else:
        outs = pcs.MultilinearZip.batch_commit(pp, mles)
    idx = list(order) if order is not None else list(range(M))
    transcript = pcs.PcsTranscript()
    pcs.MultilinearZip.batch_open(pp, [mles[i] for i in idx], [outs[i][0] for i in idx], [points[i] for i in idx], field, transcript)
    return transcript.into_proof(), transcript.probe(), [outs[i][1] for i in idx]


def test_batched_path_equals_the_loop(pcs, case, monkeypatch):
    pp, mles, field, points_int, points = case
    proof, probe, comms = _run(pcs, case)
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    proof_l, probe_l, comms_l = _run(pcs, case)
    monkeypatch.delenv("ZIP_HIP_BATCH")
    assert proof.size == proof_l.size and proof.size % M == 0
    assert np.array_equal(proof, proof_l)
    assert probe == probe_l
    assert all(np.array_equal(a, b) for a, b in zip(comms, comms_l))
    # and the loop is the per-polynomial calls
    t = pcs.PcsTranscript()
    for mle, pt in zip(mles, points):
        data, _ = pcs.MultilinearZip.commit(pp, mle)
        pcs.MultilinearZip.open(pp, mle, data, pt, field, t)
    assert np.array_equal(proof, t.into_proof()) and probe == t.probe()
    # batch_verify_z accepts
    q = MODULUS
    evals = [np.array([(_int_mle_eval(m, p) % q * (1 << 256) % q >> (64 * i)) & (2**64 - 1) for i in range(FL)], dtype=np.uint64)
             for m, p in zip(mles, points_int)]
    vt = pcs.PcsTranscript.from_proof(proof)
    pcs.MultilinearZip.batch_verify_z(pp, comms, points, evals, vt, field)
    assert vt.position() == proof.size


def test_datas_of_two_batches_fall_back_to_the_loop(pcs, case):
    proof, probe, _ = _run(pcs, case)
    proof_s, probe_s, _ = _run(pcs, case, split=4)
    assert np.array_equal(proof, proof_s) and probe == probe_s


def test_datas_out_of_order_fall_back_to_the_loop(pcs, case, monkeypatch):
    order = [3, 0, 1, 2, 9, 8, 7, 6, 5, 4]
    proof, probe, _ = _run(pcs, case, order=order)
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    proof_l, probe_l, _ = _run(pcs, case, order=order)
    assert np.array_equal(proof, proof_l) and probe == probe_l
    # a different stream from the in-order one: the transcript is shared, the order matters
    assert not np.array_equal(proof, _run(pcs, case)[0])


def test_empty_batches_make_no_call(pcs, case):
    pp, _, field, _, _ = case
    assert pcs.MultilinearZip.batch_commit(pp, []) == []
    t = pcs.PcsTranscript()
    pcs.MultilinearZip.batch_open(pp, [], [], [], field, t)
    assert t.into_proof().size == 0
