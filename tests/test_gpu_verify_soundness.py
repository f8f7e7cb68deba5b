"""GPU: zip_verify's verdict, failing opening and counts on tampered proofs, through cabi.ZipContext.verify.

Every expectation is the whole report dict predicted by the Python-int model of _verify_cases.py, which
tests/test_verify_cases_host.py confirms against the CPU oracle case by case.  The catalogue reaches what an honest
proof never does: row blocks past the first (tall), full-width signed column entries (wide entries), the overflow flag
at its exact boundary with one and with two codeword positions per thread (wide), non-canonical evaluation-row
elements, and two faults at once."""
import numpy as np
import pytest

import _oracle as orc
import _verify_cases as vc

pytestmark = pytest.mark.gpu

ACCEPTED = {"verdict": vc.ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    assert [m.VERIFY_ACCEPT, m.VERIFY_PROXIMITY_TESTING, m.VERIFY_EVAL_CONSISTENCY, m.VERIFY_PROXIMITY_Q0,
            m.VERIFY_MERKLE, m.VERIFY_MALFORMED, m.VERIFY_OVERFLOW] == list(range(7))
    return m


@pytest.fixture(scope="module")
def contexts():
    return {}


def _device(cabi, contexts, inst, proof, roots, ev):
    z = inst.z
    geo = (z.row_len, z.num_rows, z.codeword_len)
    if geo not in contexts:
        contexts[geo] = cabi.ZipContext(z.num_vars, z.perm1, z.perm2, geometry_override=geo)
    return contexts[geo].verify(roots, proof, inst.coeffs, inst.cols, inst.q0, inst.q1,
                                np.array(orc.int_to_limbs(ev, inst.fl), dtype=np.uint64),
                                cabi.make_field(inst.modulus, inst.fl))


@pytest.mark.parametrize("entry", vc.PLAN, ids=vc.plan_id)
def test_report_is_the_models(cabi, contexts, entry):
    """(a) positions, (b) counts, (c) combination-preserving tampers, (d) full-width entries, (e) the overflow
    boundary, (f) precedence: one instance and one group of the catalogue per case."""
    key, group = entry
    inst, cases = vc.cases(key, group)
    assert _device(cabi, contexts, inst, inst.proof, inst.roots, inst.ev) == ACCEPTED, inst.name
    wrong = []
    for case, want in cases:
        got = _device(cabi, contexts, inst, *case.mutate(inst.proof, inst.roots, inst.ev))
        print(f"{inst.name}: {case.name}: device {got}, model {want}")
        if got != want.report:
            wrong.append((case.name, got, want.report))
    assert not wrong, wrong


@pytest.mark.parametrize("geometry", ["base", "tall"])
def test_full_width_entries_from_device_memory(cabi, contexts, geometry):
    """(d) with the stream resident in HBM: accepted, then one sign bit flipped in place and flipped back."""
    torch = pytest.importorskip("torch")
    inst = vc.instance(geometry, vc.BENCH_MODULUS, 4, True)
    dev = torch.from_numpy(inst.proof.copy()).cuda()
    assert _device(cabi, contexts, inst, dev, inst.roots, inst.ev) == ACCEPTED
    k, r = inst.n_cols - 2, inst.R - 1
    dev[inst.val_at(k, r) + 31] ^= 0x80
    assert _device(cabi, contexts, inst, dev, inst.roots, inst.ev) == {
        "verdict": vc.PROXIMITY_TESTING, "column": k, "bad_merkle_paths": 1, "malformed_paths": 0}
    dev[inst.val_at(k, r) + 31] ^= 0x80
    assert _device(cabi, contexts, inst, dev, inst.roots, inst.ev) == ACCEPTED
