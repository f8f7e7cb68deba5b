"""ZincProver::pcs_step_batch inside prove_batch: the PCS step of B proofs of one circuit -- every proof with the RAA code
of its own transcript and its own field -- as ONE zip_batch_commit_codes and one pair of _fields opens.  Byte for byte
the loop over the one-proof step (ZIP_HIP_BATCH=0): ZipProofs and final transcripts; zip_batch_codes_counts says which
path ran; every proof passes the unchanged ZincVerifier, one at a time."""
import numpy as np
import pytest

from test_gpu_spartan_batch import KEYS, _batch, _boolean_instances, _moduli, _random_instances, _transcripts, _xw

pytestmark = pytest.mark.gpu

ZIP_KEYS = ("z_comm", "v", "pcs_proof")


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _both_legs(mods, monkeypatch, insts, moduli, fl):
    """prove_batch with the PCS step batched from two proofs on, then as the loop -> (batch, its transcripts, loop, its
    transcripts); the counters are checked on the way"""
    cabi, pcs = mods
    B = len(insts)
    monkeypatch.setenv("ZIP_HIP_PCS_MIN_BATCH", "2")
    before = cabi.batch_codes_counts()
    got, ts = _batch(pcs, insts, moduli, fl, with_pcs=True)
    after = cabi.batch_codes_counts()
    assert after == (before[0] + 1, before[1] + B, before[2] + 2), "one commit of B members, two field opens"
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    loop, ts_loop = _batch(pcs, insts, moduli, fl, with_pcs=True)
    assert cabi.batch_codes_counts() == after, "the loop does not come near the batch entry points"
    monkeypatch.delenv("ZIP_HIP_BATCH")
    monkeypatch.delenv("ZIP_HIP_PCS_MIN_BATCH")
    return got, ts, loop, ts_loop


def _assert_same_bytes(got, ts, loop, ts_loop):
    assert len(got) == len(loop)
    for i in range(len(got)):
        for key in KEYS:
            assert np.array_equal(got[i][key], loop[i][key]), (i, key)
        for key in ZIP_KEYS:
            assert got[i]["zip_proof"][key].shape == loop[i]["zip_proof"][key].shape, (i, key)
            assert np.array_equal(got[i]["zip_proof"][key], loop[i]["zip_proof"][key]), (i, key)
        st, buf = ts[i].state()
        st_loop, buf_loop = ts_loop[i].state()
        assert np.array_equal(st, st_loop) and buf == buf_loop, i
        assert ts[i].get_u64() == ts_loop[i].get_u64(), i


# one row of two entries, a 4 x 4 matrix, 32 x 32; five members: every label of the transcripts (one longer than a Keccak
# block), the moduli _moduli gives (2^256 - 189 among them at 4 limbs)
@pytest.mark.parametrize("s,fl", [(1, 4), (4, 4), (10, 4), (4, 2)])
def test_same_bytes_as_the_loop_and_the_verifier_accepts(mods, monkeypatch, s, fl):
    _, pcs = mods
    B = 5
    insts, moduli = _boolean_instances(s, B), _moduli(fl, B)
    got, ts, loop, ts_loop = _both_legs(mods, monkeypatch, insts, moduli, fl)
    _assert_same_bytes(got, ts, loop, ts_loop)
    if s == 1:  # a one-column matrix: the reference's verifier accepts only a zero evaluation (verify_z.rs:145-149)
        return
    def accepts(proof, i):  # the unchanged verifier, one proof at a time; it raises on a reject
        inst, t = insts[i], _transcripts(pcs, B)[i]
        try:
            pcs.ZincVerifier().verify(inst.matrices, inst.s, inst.d, inst.S, inst.c, proof, t, pcs.FieldConfig(moduli[i], fl))
        except pcs.InvalidPcsOpen:
            return False
        return True

    for i, q in enumerate(moduli):
        if (1 << (64 * fl)) - q < 1 << 64:
            # 2^256 - 189 and its like are a negative Int inside the reference's `%=` (field.rs:550-557): its FieldMap is
            # not additive there and the reference rejects its own proofs once the values outgrow the modulus' distance
            # to 2^(64 limbs) (tests/test_gpu_verify.py).  What holds is that the batch's proof fares as the loop's does.
            assert accepts(got[i], i) == accepts(loop[i], i), i
        else:
            assert accepts(got[i], i), i


@pytest.mark.parametrize("s", [4, 10])
def test_same_bytes_on_full_width_witnesses(mods, monkeypatch, s):
    """the random circuit (7 matrices) with 64-bit witnesses, members 0 and 1 the same z in different fields"""
    insts, moduli = _random_instances(s, 5), _moduli(4, 5)
    got, ts, loop, ts_loop = _both_legs(mods, monkeypatch, insts, moduli, 4)
    _assert_same_bytes(got, ts, loop, ts_loop)
    assert not np.array_equal(got[0]["zip_proof"]["z_comm"], got[1]["zip_proof"]["z_comm"])  # their codes differ


def test_two_proximity_tests_take_the_loop(mods, monkeypatch):
    cabi, pcs = mods
    s, fl, B = 4, 4, 3
    insts, moduli = _boolean_instances(s, B), _moduli(fl, B)
    spec = pcs.LinearCodeSpec(num_proximity_testing=2)
    fields = [pcs.FieldConfig(q, fl) for q in moduli]
    xs, ws = [_xw(i.z)[0] for i in insts], [_xw(i.z)[1] for i in insts]
    base = insts[0]
    monkeypatch.setenv("ZIP_HIP_PCS_MIN_BATCH", "2")
    before = cabi.batch_codes_counts()
    ts = _transcripts(pcs, B)
    got = pcs.ZincProver(spec=spec).prove_batch(base.matrices, base.s, base.d, base.S, base.c, xs, ws, ts, fields)
    assert cabi.batch_codes_counts() == before
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    ts_loop = _transcripts(pcs, B)
    loop = pcs.ZincProver(spec=spec).prove_batch(base.matrices, base.s, base.d, base.S, base.c, xs, ws, ts_loop, fields)
    assert cabi.batch_codes_counts() == before
    _assert_same_bytes(got, ts, loop, ts_loop)
    # one instance takes the loop as well
    monkeypatch.delenv("ZIP_HIP_BATCH")
    pcs.ZincProver().prove_batch(base.matrices, base.s, base.d, base.S, base.c, xs[:1], ws[:1], _transcripts(pcs, 1), fields[:1])
    assert cabi.batch_codes_counts() == before
