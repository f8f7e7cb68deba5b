"""CPU: every expectation tests/test_gpu_verify_soundness.py holds the device to is the reference's.

The model in _verify_cases.py predicts zip_verify's whole report; here its verdict class is compared with what the CPU
oracle (check_merkle on) returns for the same tampered proof, and with what each tamper promises by construction."""
import numpy as np
import pytest

import _oracle as orc
import _verify_cases as vc


def test_python_raa_is_the_oracles():
    """The Python-int encoder the model and wide_proof rest on, against orc_raa_encode_row on an honest u'."""
    for geometry, q, fl in (("base", vc.BENCH_MODULUS, 4), ("wide", vc.MOD_3LIMB, 3)):
        inst = vc.instance(geometry, q, fl)
        u = inst.u_prime(inst.proof)
        rc, want = inst.z.encode_row(np.array([orc.int_to_limbs(x, 8) for x in u], dtype=np.uint64), 8, 8)
        got, lo, hi = vc.raa_encode(inst.z, u)
        assert rc == 0 and vc.INT8_MIN <= lo and hi <= vc.INT8_MAX
        assert [orc.limbs_to_int(w, signed=True) for w in want] == got


@pytest.mark.parametrize("key", sorted({k for k, _ in vc.PLAN}, key=str), ids=lambda k: f"{k[0]}-fl{k[2]}-{'wide' if k[3] else 'honest'}")
def test_untampered_proofs_are_accepted_by_model_and_oracle(key):
    inst = vc.instance(*key)
    want = vc.expected_report(inst, inst.proof, inst.roots, inst.ev)
    assert want.report == {"verdict": vc.ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    assert inst.oracle_rc(inst.proof, inst.roots, inst.ev) == 0
    if key[3]:  # wide entries: they do fill Int<4>, with both signs
        vals = [inst.value(inst.proof, k, r) for k in range(0, inst.n_cols, 97) for r in range(0, inst.R, 3)]
        assert max(abs(v) for v in vals).bit_length() > 236 and sum(v < 0 for v in vals) > len(vals) // 4


@pytest.mark.parametrize("entry", vc.PLAN, ids=vc.plan_id)
def test_model_agrees_with_the_oracle(entry):
    key, group = entry
    inst, cases = vc.cases(key, group)
    assert cases
    for case, want in cases:
        for field, value in case.claim.items():
            assert want.report[field] == value, (inst.name, case.name, field, want)
        rc = inst.oracle_rc(*case.mutate(inst.proof, inst.roots, inst.ev))
        print(f"{inst.name}: {case.name}: model {want}, oracle {rc}")
        if want.oracle == "accept":
            assert rc == 0, (case.name, want, rc)
        elif want.oracle == "overflow":
            assert rc == orc.ORC_ERR_OVERFLOW, (case.name, want, rc)
        elif want.oracle == "transcript":
            assert rc == orc.ORC_ERR_TRANSCRIPT, (case.name, want, rc)
        elif want.oracle == "noncanonical":
            # The device is stricter on purpose (include/zip_hip.h): the reference does not range-check the elements,
            # and whether its sequential modular additions in encode_f still reach the honest codeword depends on
            # where x + q enters them -- on both fields the oracle accepts one of the two elements tried and rejects
            # the other.  Either is fine here; only the device's MALFORMED is pinned, in the GPU test.
            assert rc in (0, orc.ORC_ERR_PROOF), (case.name, want, rc)
        else:
            assert want.oracle == "reject" and rc != 0, (case.name, want, rc)
