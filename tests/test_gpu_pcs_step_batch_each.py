"""ZincProver::pcs_step_batch delivers every proof stream straight into its ZipProof: the batched PCS step is one
zip_batch_commit_codes, one zip_batch_open_eval_fields and ONE zip_batch_open_each, and returns the ZipProofs of the loop
over the one-proof step (ZIP_HIP_BATCH=0) byte for byte.  Needs a real MI355X."""
import numpy as np
import pytest

from test_gpu_spartan_batch import _boolean_instances, _moduli, _transcripts, _xw

pytestmark = pytest.mark.gpu

ZIP_KEYS = ("z_comm", "v", "pcs_proof")


def test_pcs_step_batch_is_one_open_each_and_returns_the_loops_proofs(monkeypatch):
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    s, fl, B = 1, 4, 3  # the smallest circuit of tests/test_gpu_pcs_step_batch.py: one row of two entries
    insts, moduli = _boolean_instances(s, B), _moduli(fl, B)
    fields = [pcs.FieldConfig(q, fl) for q in moduli]
    base = insts[0]
    prover = pcs.ZincProver()
    # the state the PCS step starts from: the points and transcripts the Spartan part leaves
    ts = _transcripts(pcs, B)
    sp = prover.spartan_prove_batch(base.matrices, base.s, base.d, base.S, base.c, [_xw(i.z)[0] for i in insts],
                                    [_xw(i.z)[1] for i in insts], ts, fields)
    r_y, states = [p["r_y"] for p in sp], [t.state() for t in ts]
    m = 1 << s
    zs = [np.concatenate([i.z, np.zeros(m - len(i.z), dtype=np.int64)]) for i in insts]

    def step():
        legs = _transcripts(pcs, B)
        for t, st in zip(legs, states):
            t.set_state(st)
        return prover.pcs_step_batch(s, zs, r_y, legs, fields), legs

    monkeypatch.setenv("ZIP_HIP_PCS_MIN_BATCH", "2")
    before, before_codes = cabi.batch_open_each_counts(), cabi.batch_codes_counts()
    got, ts_got = step()
    after = cabi.batch_open_each_counts()
    assert after[:2] == (before[0] + 1, before[1] + B), "one zip_batch_open_each for the three proofs"
    assert after[2] == before[2] + 1 and after[3] == B * got[0]["pcs_proof"].size, "64 MiB windows: one, of three streams"
    assert cabi.batch_codes_counts() == (before_codes[0] + 1, before_codes[1] + B, before_codes[2] + 2)
    monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    loop, ts_loop = step()
    assert cabi.batch_open_each_counts() == after, "the loop does not come near the batch entry points"
    assert len(got) == len(loop) == B
    for i in range(B):
        for key in ZIP_KEYS:
            assert got[i][key].shape == loop[i][key].shape, (i, key)
            assert np.array_equal(got[i][key], loop[i][key]), (i, key)
        st, buf = ts_got[i].state()
        st_loop, buf_loop = ts_loop[i].state()
        assert np.array_equal(st, st_loop) and buf == buf_loop, i
    assert len({p["pcs_proof"].tobytes() for p in got}) == B, "three proofs, three streams"
