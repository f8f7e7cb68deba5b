"""The verifier shapes of tests/test_gpu_two_limb_regimes.py without a device: at 2048 rows and at codewords of 2048, 4096
and 65536 the CPU oracle accepts its own two-limb proof, the Python-int model of tests/_two_limb.py says ACCEPT for it,
and for every tampered stream the GPU file feeds zip_verify the model names a failure and the oracle rejects -- with
ORC_ERR_OVERFLOW where the model says OVERFLOW.  So the model is held to the oracle at these shapes before any kernel is
compared with it."""
import pytest

import _oracle as orc
import _two_limb as tl


def _model_against_oracle(inst, cases):
    assert inst.oracle_rc(inst.proof, inst.roots, inst.ev) == 0
    assert inst.expect(inst.proof, inst.roots, inst.ev) == dict(verdict=tl.ACCEPT, column=0, bad_merkle_paths=0, malformed_paths=0)
    names = [name for name, _, _ in cases]
    assert len(set(names)) == len(names), names
    for name, mutate, claim in cases:
        proof, roots, ev = mutate(inst.proof, inst.roots, inst.ev)
        want = inst.expect(proof, roots, ev)
        for key, value in claim.items():
            assert want[key] == value, (name, want, claim)
        assert want["verdict"] != tl.ACCEPT, name
        rc = inst.oracle_rc(proof, roots, ev)
        assert rc != 0, f"{name}: the oracle accepts"
        assert (rc == orc.ORC_ERR_OVERFLOW) == (want["verdict"] == tl.OVERFLOW), (name, rc, want)


@pytest.mark.parametrize("shape", tl.REGIME_MANY_ROWS, ids=lambda s: f"nv{s[0]}-R{s[3][1]}-fl{s[2]}")
def test_model_and_oracle_at_eight_rows_per_thread(shape):
    inst = tl.regime_instance(*shape)
    cases = tl.many_rows_cases(inst)
    # the rows that only a repeat iteration of the column kernel reads are among them
    assert {"value[5,2047] bit 0", "value[7,256] bit 0", "path[9,1300] level 1", "entries that fill all 512 bits"} <= {c[0] for c in cases}
    _model_against_oracle(inst, cases)


@pytest.mark.parametrize("shape", tl.REGIME_WIDE_CODEWORDS, ids=lambda s: f"nv{s[0]}-cw{s[3][2]}-fl{s[2]}")
def test_model_and_oracle_at_wide_codewords(shape):
    inst = tl.regime_instance(*shape)
    assert inst.cw >= 1024
    cases = tl.wide_codeword_cases(inst)
    verdicts = {inst.expect(*mutate(inst.proof, inst.roots, inst.ev))["verdict"] for _, mutate, _ in cases}
    assert verdicts == {tl.OVERFLOW, tl.PROXIMITY_TESTING, tl.EVAL_CONSISTENCY}
    _model_against_oracle(inst, cases)
