"""ZincVerifier::verify_batch on the device: B proofs of one circuit (what prove_batch makes), each with its own transcript,
code and field -- the PCS part ONE zip_batch_verify_codes, the matrix MLEs ONE zip_ccs_batch_eval_matrices.  Outcome for
outcome and transcript for transcript the loop over the unchanged `verify` (ZIP_HIP_BATCH=0 inside the call, and `verify`
itself called proof after proof), for rejected proofs as well; zip_batch_verify_codes_counts says which path ran."""
import copy

import numpy as np
import pytest

import _ccs
import _ccs_random
from test_gpu_spartan_batch import _batch, _boolean_instances, _moduli, _random_instances, _transcripts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _verify_batch(pcs, insts, moduli, fl, proofs, spec=None):
    base = insts[0]
    ts = _transcripts(pcs, len(proofs))
    fields = [pcs.FieldConfig(q, fl) for q in moduli]
    got = pcs.ZincVerifier(spec=spec).verify_batch(base.matrices, base.s, base.d, base.S, base.c, proofs, ts, fields)
    return got, ts


def _verify_one_by_one(pcs, insts, moduli, fl, proofs, spec=None):
    """the unchanged verify, proof after proof: the exception it raises, or None"""
    ts = _transcripts(pcs, len(proofs))
    out = []
    for inst, q, proof, t in zip(insts, moduli, proofs, ts):
        try:
            pcs.ZincVerifier(spec=spec).verify(inst.matrices, inst.s, inst.d, inst.S, inst.c, proof, t, pcs.FieldConfig(q, fl))
            out.append(None)
        except (pcs.SpartanError, pcs.InvalidPcsOpen) as e:
            out.append(e)
    return out, ts


def _same_outcomes(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert type(x) is type(y) and str(x) == str(y), (i, x, y)


def _same_transcripts(*legs):
    """member for member the same sponge in every leg: the state, then the next squeeze (which moves it: call once)"""
    for i, ts in enumerate(zip(*legs)):
        states = [t.state() for t in ts]
        for st, buf in states[1:]:
            assert np.array_equal(st, states[0][0]) and buf == states[0][1], i
        assert len({t.get_u64() for t in ts}) == 1, i


def _three_legs(mods, monkeypatch, insts, moduli, fl, proofs, survivors):
    """verify_batch batched from two proofs on, verify_batch as the loop, and verify itself proof after proof: identical
    outcomes and transcripts; the counters say which path ran.  -> the outcomes"""
    cabi, pcs = mods
    monkeypatch.setenv("ZIP_HIP_VERIFY_MIN_BATCH", "2")
    before = cabi.batch_verify_codes_counts()
    launches = cabi.ccs_batch_counts()[0]
    got, ts = _verify_batch(pcs, insts, moduli, fl, proofs)
    after = cabi.batch_verify_codes_counts()
    assert after == (before[0] + 1, before[1] + survivors), "one call, the survivors of the Spartan part"
    assert cabi.ccs_batch_counts()[0] == launches + 3, "one zip_ccs_batch_eval_matrices"
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    loop, ts_loop = _verify_batch(pcs, insts, moduli, fl, proofs)
    assert cabi.batch_verify_codes_counts() == after, "the loop does not come near the batch entry point"
    monkeypatch.delenv("ZIP_HIP_BATCH")
    monkeypatch.delenv("ZIP_HIP_VERIFY_MIN_BATCH")
    one, ts_one = _verify_one_by_one(pcs, insts, moduli, fl, proofs)
    _same_outcomes(got, loop)
    _same_outcomes(got, one)
    _same_transcripts(ts, ts_loop, ts_one)
    return got


# one row of two entries, a 4 x 4 matrix, 32 x 32; five members: every label of the transcripts, the moduli _moduli gives
@pytest.mark.parametrize("s,fl", [(1, 4), (4, 4), (10, 4), (4, 2)])
def test_honest_proofs_fare_as_in_the_loop(mods, monkeypatch, s, fl):
    _, pcs = mods
    B = 5
    insts, moduli = _boolean_instances(s, B), _moduli(fl, B)
    proofs, _ = _batch(pcs, insts, moduli, fl, with_pcs=True)
    got = _three_legs(mods, monkeypatch, insts, moduli, fl, proofs, survivors=B)
    if s == 1:  # a one-column matrix: the reference's verifier accepts only a zero evaluation (verify_z.rs:145-149)
        return
    for i, q in enumerate(moduli):
        # 2^256 - 189 and its like: the reference rejects its own proofs there (tests/test_gpu_pcs_step_batch.py); what
        # holds is that the batch fares as the loop does, which _three_legs has asserted
        if (1 << (64 * fl)) - q >= 1 << 64:
            assert got[i] is None, (i, got[i])


def test_a_batch_with_every_kind_of_reject(mods, monkeypatch):
    _, pcs = mods
    s, fl, B = 4, 4, 5
    insts = _boolean_instances(s, B)
    moduli = [m for m in _moduli(fl, 2 * B) if (1 << (64 * fl)) - m >= 1 << 64][:1] * B  # a field every honest proof passes in
    honest, _ = _batch(pcs, insts, moduli, fl, with_pcs=True)
    proofs = copy.deepcopy(honest)
    proofs[1]["zip_proof"]["pcs_proof"][len(proofs[1]["zip_proof"]["pcs_proof"]) // 2] ^= 0x10  # a bit of an opening
    proofs[2]["zip_proof"]["v"][0] ^= 1                                                          # a wrong v
    proofs[3]["msgs1"][1, 0, 0] ^= 1                                                             # a sumcheck message
    proofs[4]["V_s"][0, 0] ^= 1                                                                  # a wrong V_s[0]
    got = _three_legs(mods, monkeypatch, insts, moduli, fl, proofs, survivors=B - 2)  # 3 and 4 fall in the Spartan part
    print(got)
    assert got[0] is None
    assert isinstance(got[1], pcs.InvalidPcsOpen)
    assert isinstance(got[2], (pcs.InvalidPcsOpen, pcs.SpartanError))
    assert isinstance(got[3], pcs.SpartanError)
    assert isinstance(got[4], pcs.SpartanError)


def test_the_seven_matrix_random_circuit(mods, monkeypatch):
    """the random circuit of tests/_ccs_random.py is satisfied by nothing: every proof is rejected, by the batch exactly
    as by the loop and by verify; members 0 and 1 hold the same z in different fields"""
    cabi, pcs = mods
    s, fl, B = 4, 4, 5
    insts, moduli = _random_instances(s, B), _moduli(fl, B)
    proofs, _ = _batch(pcs, insts, moduli, fl, with_pcs=True)
    one, ts_one = _verify_one_by_one(pcs, insts, moduli, fl, proofs)
    assert all(e is not None for e in one)
    monkeypatch.setenv("ZIP_HIP_VERIFY_MIN_BATCH", "2")
    got, ts = _verify_batch(pcs, insts, moduli, fl, proofs)
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    loop, ts_loop = _verify_batch(pcs, insts, moduli, fl, proofs)
    _same_outcomes(got, loop)
    _same_outcomes(got, one)
    _same_transcripts(ts, ts_loop, ts_one)


def test_a_satisfied_seven_matrix_circuit(mods, monkeypatch):
    """t = 7 through the device: I, I, I, I, I, I, 5 I with the S and c of the random circuit's shape --
    z z - z z + 5 z z - 5 z = 0 for every 0/1 vector -- so all seven V_xy enter the last check"""
    _, pcs = mods
    s, fl, B = 4, 4, 5
    m = 1 << s
    ident = _ccs.CsrMatrix.diagonal(np.ones(m, dtype=np.int64))
    five = _ccs.CsrMatrix.diagonal(np.full(m, 5, dtype=np.int64))
    S, c, d = _ccs_random._shape(7)
    assert S == [[0, 1], [2, 3], [4, 5], [6]] and c == [1, -1, 5, -1]
    insts = [_ccs.CcsInstance(m, m, s, s, d, [ident] * 6 + [five], S, c, b.z) for b in _boolean_instances(s, B)]
    moduli = _moduli(fl, B)
    proofs, _ = _batch(pcs, insts, moduli, fl, with_pcs=True)
    got = _three_legs(mods, monkeypatch, insts, moduli, fl, proofs, survivors=B)
    for i, q in enumerate(moduli):
        if (1 << (64 * fl)) - q >= 1 << 64:
            assert got[i] is None, (i, got[i])
    wrong = copy.deepcopy(proofs)
    wrong[2]["V_s"][6, 0] ^= 1  # the seventh matrix's claim
    got = _three_legs(mods, monkeypatch, insts, moduli, fl, wrong, survivors=B - 1)
    assert isinstance(got[2], pcs.SpartanError)


def test_two_proximity_tests_and_one_instance_take_the_loop(mods, monkeypatch):
    cabi, pcs = mods
    s, fl, B = 4, 4, 3
    insts, moduli = _boolean_instances(s, B), [_moduli(fl, 2)[1]] * B
    spec = pcs.LinearCodeSpec(num_proximity_testing=2)
    base = insts[0]
    fields = [pcs.FieldConfig(q, fl) for q in moduli]
    xs, ws = [i.z[:1] for i in insts], [i.z[2:] for i in insts]
    proofs = pcs.ZincProver(spec=spec).prove_batch(base.matrices, base.s, base.d, base.S, base.c, xs, ws, _transcripts(pcs, B), fields)
    monkeypatch.setenv("ZIP_HIP_VERIFY_MIN_BATCH", "2")
    before = cabi.batch_verify_codes_counts()
    got, ts = _verify_batch(pcs, insts, moduli, fl, proofs, spec=spec)
    assert cabi.batch_verify_codes_counts() == before
    one, ts_one = _verify_one_by_one(pcs, insts, moduli, fl, proofs, spec=spec)
    _same_outcomes(got, one)
    _same_transcripts(ts, ts_one)
    assert got == [None] * B
    # one instance
    honest, _ = _batch(pcs, insts[:1], moduli[:1], fl, with_pcs=True)
    got, _ = _verify_batch(pcs, insts[:1], moduli[:1], fl, honest)
    assert got == [None] and cabi.batch_verify_codes_counts() == before
    # without the hook the measured line holds (profiles/verify_batch.md): up to 2^10 rows two proofs are a batch already
    monkeypatch.delenv("ZIP_HIP_VERIFY_MIN_BATCH")
    honest, _ = _batch(pcs, insts, moduli, fl, with_pcs=True)
    got, _ = _verify_batch(pcs, insts, moduli, fl, honest)
    assert got == [None] * B and cabi.batch_verify_codes_counts() == (before[0] + 1, before[1] + B)
