"""ZincProver::spartan_prove_batch / prove_batch on the device: B proofs of ONE circuit, each with its own z, transcript
and field -- the circuit on the device once as integers (zip_ccs_batch), both sumchecks one zip_sumcheck_prove_batch each.
Bit for bit against the oracle's SpartanProver::prove (orc.Ccs(inst).spartan_prove) and against the device's own loop
over spartan_prove (ZIP_HIP_BATCH=0), the transcript afterwards included."""
import numpy as np
import pytest

import _ccs
import _ccs_random
import _oracle as orc

pytestmark = pytest.mark.gpu

KEYS = ("msgs1", "msgs2", "V_s", "r_y")
LABELS = (b"", b"zinc", b"a transcript that has seen more than one hundred and thirty-six bytes before the proof begins: " * 2, b"\x00")


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _moduli(fl, n):
    ms = _ccs_random.MODULI[fl]
    return [ms[(0, 1, 1, 2, 3)[i % 5]] for i in range(n)]


def _xw(z):
    """z = (x, 1, w) with one public input"""
    assert len(z) >= 2 and z[1] == 1
    return z[:1], z[2:]


def _random_instances(s, n):
    zs = _ccs_random.witnesses(s, n)
    zs = [z if len(z) >= 2 else np.array([z[0], 1], dtype=np.int64) for z in zs]
    zs[1] = zs[0]  # members 0 and 1 differ only in field and transcript
    return _ccs_random.instances(s, 7, zs)


def _boolean_instances(s, n):
    """A = B = C = I with S = [[0, 1], [2]], c = [1, -1]: z_i * z_i = z_i, satisfied by every 0/1 vector"""
    m = 1 << s
    ident = _ccs.CsrMatrix.diagonal(np.ones(m, dtype=np.int64))
    rng = np.random.default_rng(s)
    out = []
    for i in range(n):
        z = rng.integers(0, 2, size=m if i % 2 == 0 else max(2, m - m // 4), dtype=np.int64)
        z[1] = 1
        out.append(_ccs.CcsInstance(m, m, s, s, 2, [ident, ident, ident], [[0, 1], [2]], [1, -1], z))
    return out


def _transcripts(pcs, n):
    ts = []
    for i in range(n):
        t = pcs.KeccakTranscript()
        if LABELS[i % len(LABELS)]:
            t.absorb(LABELS[i % len(LABELS)])
        ts.append(t)
    return ts


def _oracle_transcript(i):
    k = orc.new_transcript()
    if LABELS[i % len(LABELS)]:
        orc.absorb(k, LABELS[i % len(LABELS)])
    return k


def _batch(pcs, insts, moduli, fl, with_pcs=False):
    base = insts[0]
    ts = _transcripts(pcs, len(insts))
    fields = [pcs.FieldConfig(q, fl) for q in moduli]
    fn = pcs.ZincProver().prove_batch if with_pcs else pcs.ZincProver().spartan_prove_batch
    got = fn(base.matrices, base.s, base.d, base.S, base.c, [_xw(i.z)[0] for i in insts], [_xw(i.z)[1] for i in insts], ts, fields)
    return got, ts


@pytest.mark.parametrize("fl", [2, 3, 4])
@pytest.mark.parametrize("s", [1, 3, 10, 13])
def test_spartan_prove_batch_equals_the_oracle_and_the_loop(mods, monkeypatch, s, fl):
    """four proofs of the random circuit, transcripts primed with different labels, four moduli: every round message of
    both sumchecks, V_s and r_y are the oracle's; the device's own loop gives the same; so is every transcript afterwards"""
    cabi, pcs = mods
    B = 4
    insts, moduli = _random_instances(s, B), _moduli(fl, B)
    before, before_rounds = cabi.sumcheck_batch_counts(), cabi.sumcheck_launch_counts()
    got, ts = _batch(pcs, insts, moduli, fl)
    after = cabi.sumcheck_batch_counts()
    # the batched path: two launches of the batch sumcheck kernel for the whole call, no round kernel, no tail kernel
    assert after[0] - before[0] == 2 and after[1] - before[1] == 2 * B
    assert cabi.sumcheck_launch_counts() == before_rounds
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    loop, ts_loop = _batch(pcs, insts, moduli, fl)
    assert cabi.sumcheck_batch_counts() == after  # the loop does not come near the batch kernel
    monkeypatch.delenv("ZIP_HIP_BATCH")
    for i, (inst, q) in enumerate(zip(insts, moduli)):
        ko = _oracle_transcript(i)
        want = orc.Ccs(inst).spartan_prove(orc.make_field(q, fl), ko)
        for key in KEYS:
            assert np.array_equal(got[i][key], want[key]), (i, key)
            assert np.array_equal(loop[i][key], want[key]), (i, key, "loop")
        st, buf = ts[i].state()
        st_loop, buf_loop = ts_loop[i].state()
        assert np.array_equal(st, st_loop) and buf == buf_loop, i
        assert ts[i].get_u64() == orc.lib().orc_tr_get_u64(orc.C.byref(ko)), i


@pytest.mark.parametrize("s", [1, 3, 10, 13])
def test_the_oracle_verifier_accepts_every_proof_of_a_batch(mods, s):
    _, pcs = mods
    fl, B = 3, 4
    insts, moduli = _boolean_instances(s, B), _moduli(fl, B)
    got, _ = _batch(pcs, insts, moduli, fl)
    for i, (inst, q) in enumerate(zip(insts, moduli)):
        f = orc.make_field(q, fl)
        want = orc.Ccs(inst).spartan_prove(f, _oracle_transcript(i))
        for key in KEYS:
            assert np.array_equal(got[i][key], want[key]), (i, key)
        rc, pts = orc.Ccs(inst).spartan_verify(f, got[i], _oracle_transcript(i))
        assert rc == 0 and np.array_equal(pts["r_y"], got[i]["r_y"]), i


def test_a_broken_witness_inside_a_batch(mods):
    """zinc/tests.rs:159-209 in a batch: the prover still succeeds on w_ccs[3] = 0, the verifier rejects that proof and
    accepts its neighbours"""
    _, pcs = mods
    fl = 4
    insts = [_ccs.vitalik_ccs(3), _ccs.vitalik_ccs(5), _ccs.vitalik_ccs(3, break_witness=True), _ccs.vitalik_ccs(-7)]
    moduli = _moduli(fl, 4)
    got, _ = _batch(pcs, insts, moduli, fl)
    for i, (inst, q) in enumerate(zip(insts, moduli)):
        f = orc.make_field(q, fl)
        want = orc.Ccs(inst).spartan_prove(f, _oracle_transcript(i))
        for key in KEYS:
            assert np.array_equal(got[i][key], want[key]), (i, key)
        rc, _ = orc.Ccs(inst).spartan_verify(f, got[i], _oracle_transcript(i))
        assert rc == (orc.ORC_ERR_PROOF if i == 2 else 0), i


@pytest.mark.parametrize("batch_env", [None, "0"])
def test_a_shape_error_leaves_every_transcript_as_it_was(mods, monkeypatch, batch_env):
    """instance 2 has a z longer than the matrices are wide (LengthsNotEqual, ccs/utils.rs:52-59): refused before any
    transcript is touched, on the batched path and on the loop"""
    _, pcs = mods
    if batch_env is not None:
        monkeypatch.setenv("ZIP_HIP_BATCH", batch_env)
    fl, B = 3, 4
    insts = _random_instances(3, B)
    ts = _transcripts(pcs, B)
    before = [t.state() for t in ts]
    fields = [pcs.FieldConfig(q, fl) for q in _moduli(fl, B)]
    xs, ws = [_xw(i.z)[0] for i in insts], [_xw(i.z)[1] for i in insts]
    ws[2] = np.ones(20, dtype=np.int64)
    base = insts[0]
    with pytest.raises(pcs.ReferencePanic):
        pcs.ZincProver().spartan_prove_batch(base.matrices, base.s, base.d, base.S, base.c, xs, ws, ts, fields)
    for t, (st, buf) in zip(ts, before):
        st2, buf2 = t.state()
        assert np.array_equal(st, st2) and buf == buf2
    with pytest.raises(pcs.InvalidPcsParam):  # a zero coefficient: refused for the whole batch
        pcs.ZincProver().spartan_prove_batch(base.matrices, base.s, base.d, base.S, [1, 0, 5, -1], xs[:2], [ws[0], ws[1]], ts[:2], fields[:2])
    for t, (st, buf) in zip(ts, before):
        st2, buf2 = t.state()
        assert np.array_equal(st, st2) and buf == buf2


def test_one_instance_and_mixed_limb_counts_take_the_loop(mods):
    cabi, pcs = mods
    insts = _random_instances(3, 3)
    base = insts[0]
    xs, ws = [_xw(i.z)[0] for i in insts], [_xw(i.z)[1] for i in insts]
    before = cabi.sumcheck_batch_counts()
    mixed = [(_ccs_random.Q192, 3), (_ccs_random.QSTARK, 4), (_ccs_random.Q128, 2)]
    for sel in ([0], [0, 1, 2]):
        ts = _transcripts(pcs, len(sel))
        fields = [pcs.FieldConfig(*mixed[i]) for i in sel]
        got = pcs.ZincProver().spartan_prove_batch(base.matrices, base.s, base.d, base.S, base.c, [xs[i] for i in sel],
                                                   [ws[i] for i in sel], ts, fields)
        for j, i in enumerate(sel):
            want = orc.Ccs(insts[i]).spartan_prove(orc.make_field(*mixed[i]), _oracle_transcript(j))
            for key in KEYS:
                assert np.array_equal(got[j][key], want[key]), (sel, i, key)
    assert cabi.sumcheck_batch_counts() == before
    assert pcs.ZincProver().spartan_prove_batch(base.matrices, base.s, base.d, base.S, base.c, [], [], [], []) == []


@pytest.mark.parametrize("s", [4, 10])
def test_prove_batch_equals_prove_one_at_a_time(mods, s):
    """Prover::prove for three proofs: the Spartan part batched, the PCS step per proof with the code each proof draws
    from its own transcript -- commitment, v and the PCS proof bytes are those of prove"""
    _, pcs = mods
    fl, B = 4, 3
    insts, moduli = _boolean_instances(s, B), _moduli(fl, B)
    got, ts = _batch(pcs, insts, moduli, fl, with_pcs=True)
    ts_one = _transcripts(pcs, B)
    for i, (inst, q) in enumerate(zip(insts, moduli)):
        x, w = _xw(inst.z)
        want = pcs.ZincProver().prove(inst.matrices, inst.s, inst.d, inst.S, inst.c, x, w, ts_one[i], pcs.FieldConfig(q, fl))
        for key in KEYS:
            assert np.array_equal(got[i][key], want[key]), (i, key)
        for key in ("z_comm", "v", "pcs_proof"):
            assert np.array_equal(got[i]["zip_proof"][key], want["zip_proof"][key]), (i, key)
        assert ts[i].get_u64() == ts_one[i].get_u64(), i
        rc, _ = orc.Ccs(inst).spartan_verify(orc.make_field(q, fl), got[i], _oracle_transcript(i))
        assert rc == 0
