"""batch_verify_z through the host mirror (zinc_amd/pcs.py -> libzinc_zip.so -> libzip_hip.so) at the shape of the
reference's test_zip_batch_evaluation (tests.rs:148: n = 8, m = 10): the batched path (one host walk of the shared
transcript, one zip_batch_verify call) against the loop over verify (ZIP_HIP_BATCH=0) -- same result, same exception,
same cursor, same transcript state."""
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


def _int_mle_eval(evals, point):
    cur = [int(x) for x in evals]
    for p in point:
        cur = [cur[2 * b] + int(p) * (cur[2 * b + 1] - cur[2 * b]) for b in range(len(cur) // 2)]
    return cur[0]


@pytest.fixture(scope="module")
def case(pcs):
    """pp, field, points, claimed evaluations, commitments and the stream batch_open left: built once, never modified"""
    t = pcs.KeccakTranscript()
    pp = pcs.MultilinearZip.setup(1 << N, pcs.RaaCode(1 << N, t))
    rng = np.random.default_rng(5)
    mles = [rng.integers(-128, 128, size=1 << N, dtype=np.int64) for _ in range(M)]
    field = pcs.FieldConfig(MODULUS, FL)
    points_int = [rng.integers(-128, 128, size=N, dtype=np.int64) for _ in range(M)]  # a different point per polynomial
    points = [field.map_to_field(p) for p in points_int]
    outs = pcs.MultilinearZip.batch_commit(pp, mles)
    transcript = pcs.PcsTranscript()
    pcs.MultilinearZip.batch_open(pp, mles, [o[0] for o in outs], points, field, transcript)
    proof = transcript.into_proof()
    q = MODULUS
    evals = [np.array([(_int_mle_eval(m, p) % q * (1 << 256) % q >> (64 * i)) & (2**64 - 1) for i in range(FL)], dtype=np.uint64)
             for m, p in zip(mles, points_int)]
    proof.setflags(write=False)
    return pp, field, points, evals, [o[1] for o in outs], proof


def _verify(pcs, case, proof, n=M, points=None):
    """batch_verify_z on a fresh reading transcript -> (exception type or None, message, position, probe, device calls made)"""
    from zinc_amd import cabi

    pp, field, pts, evals, comms, _ = case
    pts = pts if points is None else points
    vt = pcs.PcsTranscript.from_proof(proof)
    before = cabi.batch_verify_calls()
    err = (None, "")
    try:
        pcs.MultilinearZip.batch_verify_z(pp, comms[:n], pts[:n], evals[:n], vt, field)
    except Exception as e:  # noqa: BLE001  (the type is what is compared)
        err = (type(e), str(e))
    return err + (vt.position(), vt.probe(), cabi.batch_verify_calls() - before)


def _both(pcs, case, monkeypatch, proof, **kw):
    batched = _verify(pcs, case, proof, **kw)
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    loop = _verify(pcs, case, proof, **kw)
    monkeypatch.delenv("ZIP_HIP_BATCH")
    return batched, loop


def test_honest_proof_takes_the_batched_path(pcs, case, monkeypatch):
    proof = case[-1]
    batched, loop = _both(pcs, case, monkeypatch, proof)
    assert batched[:3] == (None, "", proof.size) and batched[4] == 1
    assert loop[:3] == (None, "", proof.size) and loop[4] == 0
    assert batched[3] == loop[3]


def test_tampered_proof_fails_as_the_loop_does(pcs, case, monkeypatch):
    pp, proof = case[0], case[-1]
    stream_len = proof.size // M
    bad = proof.copy()
    u_bytes = pp.row_len * 64
    col_bytes = pp.num_rows * (32 + 8 + 32 * (pp.codeword_len.bit_length() - 1))
    bad[6 * stream_len + u_bytes + 321 * col_bytes + 32 * 3 + 1] ^= 0x20  # stream 6, opening 321, row 3: a column value
    batched, loop = _both(pcs, case, monkeypatch, bad)
    assert batched[:4] == loop[:4]
    assert batched[0] is pcs.InvalidPcsOpen and batched[1] == "Proximity failure" and batched[2] == 6 * stream_len
    assert (batched[4], loop[4]) == (1, 0)
    assert batched[3] != _verify(pcs, case, proof)[3]  # (the transcript stopped inside polynomial 6)


def test_stream_truncated_inside_stream_8(pcs, case, monkeypatch):
    proof = case[-1]
    stream_len = proof.size // M
    batched, loop = _both(pcs, case, monkeypatch, proof[: 8 * stream_len + 1000])
    assert batched[:4] == loop[:4]
    assert batched[0] is pcs.InvalidPcsOpen and batched[2] == 8 * stream_len
    assert (batched[4], loop[4]) == (1, 0)  # the eight whole streams went to the device in one call


def test_one_polynomial_or_a_short_point_take_the_loop(pcs, case, monkeypatch):
    pp, field, points, evals, comms, proof = case
    stream_len = proof.size // M
    one = _verify(pcs, case, proof, n=1)
    assert one[:3] == (None, "", stream_len) and one[4] == 0
    short = list(points)
    short[3] = points[3][:-1]
    batched, loop = _both(pcs, case, monkeypatch, proof, points=short)
    assert batched == loop and batched[0] is pcs.InvalidPcsParam and batched[2] == 3 * stream_len and batched[4] == 0
