"""zip_verify on a two-limb ctx: honest proofs are accepted (and the reference's verifier, with Merkle paths checked,
accepts the same bytes), and every tampered stream gets the verdict, the failing column and the counts that the
Python-int model of tests/_two_limb.py derives in the reference's order of checks -- the order tests/_verify_cases.py
defines for one limb.  Needs a real MI355X."""
import numpy as np
import pytest

import _oracle as orc
import _two_limb as tl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _verify(cabi, ctx, inst, proof, roots, ev):
    return ctx.verify(roots, proof, inst.coeffs, inst.cols, inst.q0, inst.q1, np.array(orc.int_to_limbs(ev, inst.fl), dtype=np.uint64),
                      cabi.make_field(inst.modulus, inst.fl))


@pytest.mark.parametrize("modulus,fl", tl.VERIFY_MODULI)
@pytest.mark.parametrize("num_vars", [4, 8, 12])
def test_honest_proofs_are_accepted(cabi, num_vars, modulus, fl):
    inst = tl.instance(num_vars, modulus, fl)
    ctx = inst.z.ctx(cabi)
    # the device's own proof is the oracle's, byte for byte, and both verifiers accept it
    proof, roots, _ = ctx.commit_open(inst.evals, inst.coeffs, inst.cols, inst.q0, cabi.make_field(modulus, fl))
    assert np.array_equal(proof, inst.proof) and np.array_equal(roots, inst.roots)
    assert inst.z.verify(inst.f, roots, inst.point, inst.ev, proof, check_merkle=True) == 0
    rep = _verify(cabi, ctx, inst, proof, roots, inst.ev)
    assert rep == dict(verdict=cabi.VERIFY_ACCEPT, column=0, bad_merkle_paths=0, malformed_paths=0)
    # a longer buffer is allowed
    longer = np.concatenate([proof, np.arange(40, dtype=np.uint8)])
    assert _verify(cabi, ctx, inst, longer, roots, inst.ev)["verdict"] == cabi.VERIFY_ACCEPT


@pytest.mark.parametrize("num_vars", [0, 1])
def test_one_column_matrices(cabi, num_vars):
    """row_len == 1 leaves q_1 empty (pcs/utils.rs:253-276): <row, q1> is 0 in both verifiers, so the claimed evaluation 0
    passes the consistency check and the true evaluation of a non-zero witness does not (verify_z.rs:146-151).
    num_vars 0 is also the one-row matrix: no u', no proximity test over Z."""
    modulus, fl = tl.BENCH_MODULUS, 4
    z = tl.Zip2(num_vars)
    assert z.row_len == 1 and z.num_rows == 1 << num_vars
    f = orc.make_field(modulus, fl)
    zf = cabi.make_field(modulus, fl)
    evals = tl.witness(z) if num_vars else tl.to_limbs([tl.INT2_MIN])
    point = tl.make_point(f, num_vars)
    rows, layers, roots = z.commit(evals)
    proof, cols, coeffs = z.open(f, evals, rows, layers, point)
    q0, q1 = z.tensors(f, point)
    assert q1 is None
    ctx = z.ctx(cabi)
    single = z.num_rows == 1
    got, roots_d, _ = ctx.commit_open(evals, None if single else coeffs, cols, q0, zf)
    assert np.array_equal(got, proof) and np.array_equal(roots_d, roots)
    true_ev = z.mle_eval(f, evals, point)
    assert true_ev != 0
    for ev, verdict in ((0, cabi.VERIFY_ACCEPT), (true_ev, cabi.VERIFY_EVAL_CONSISTENCY)):
        assert (z.verify(f, roots, point, ev, proof) == 0) == (verdict == cabi.VERIFY_ACCEPT)
        rep = ctx.verify(roots, proof, None if single else coeffs, cols, q0, None, np.array(orc.int_to_limbs(ev, fl), dtype=np.uint64), zf)
        assert rep == dict(verdict=verdict, column=0, bad_merkle_paths=0, malformed_paths=0)
    tampered = proof.copy()
    tampered[(0 if single else 128) + 3] ^= 1  # a column value of the first opening
    rep = ctx.verify(roots, tampered, None if single else coeffs, cols, q0, None, np.zeros(fl, dtype=np.uint64), zf)
    assert z.verify(f, roots, point, 0, tampered) != 0
    assert rep["verdict"] == (cabi.VERIFY_MERKLE if single else cabi.VERIFY_PROXIMITY_TESTING) and rep["column"] == 0


def test_a_proof_on_the_device_is_verified_in_place(cabi):
    import torch

    inst = tl.instance(8, tl.MOD_3LIMB, 3)
    ctx = inst.z.ctx(cabi)
    proof_d = torch.from_numpy(inst.proof.copy()).cuda()
    assert _verify(cabi, ctx, inst, proof_d, inst.roots, inst.ev)["verdict"] == cabi.VERIFY_ACCEPT


@pytest.mark.parametrize("modulus,fl", [(tl.BENCH_MODULUS, 4), (tl.TEST_MODULUS_2, 2)])
@pytest.mark.parametrize("num_vars", [8, 12])
def test_tamper_catalogue(cabi, num_vars, modulus, fl):
    inst = tl.instance(num_vars, modulus, fl)
    ctx = inst.z.ctx(cabi)
    failures = []
    for name, mutate, claim in tl.tamper_cases(inst):
        proof, roots, ev = mutate(inst.proof, inst.roots, inst.ev)
        want = inst.expect(proof, roots, ev)
        for key, value in claim.items():
            assert want[key] == value, (name, want, claim)  # what the one-limb catalogue defines for the section
        assert want["verdict"] != tl.ACCEPT, name
        rc = inst.oracle_rc(proof, roots, ev)
        assert rc != 0, f"{name}: the oracle accepts"
        got = _verify(cabi, ctx, inst, proof, roots, ev)
        if got != want:
            failures.append((name, got, want))
    assert not failures, failures
    # the ctx still accepts the honest proof afterwards
    assert _verify(cabi, ctx, inst, inst.proof, inst.roots, inst.ev)["verdict"] == cabi.VERIFY_ACCEPT


@pytest.mark.parametrize("modulus,fl", [(tl.BENCH_MODULUS, 4), (tl.MOD_M127, 2)])
@pytest.mark.parametrize("num_vars", [8, 12])
def test_an_encoding_that_leaves_int16_is_overflow(cabi, num_vars, modulus, fl):
    inst = tl.instance(num_vars, modulus, fl)
    ctx = inst.z.ctx(cabi)
    name, mutate, claim = tl.overflow_case(inst)
    proof, roots, ev = mutate(inst.proof, inst.roots, inst.ev)
    want = inst.expect(proof, roots, ev)
    assert want["verdict"] == tl.OVERFLOW == cabi.VERIFY_OVERFLOW
    assert inst.oracle_rc(proof, roots, ev) == orc.ORC_ERR_OVERFLOW
    assert _verify(cabi, ctx, inst, proof, roots, ev) == want
    # the same element one bit lower fits: a proximity failure, not an overflow, unless a prefix sum still leaves Int<16>
    lower = inst.with_u_prime(inst.proof, [(1 << 1000) if j == inst.C - 1 else 0 for j in range(inst.C)])
    want = inst.expect(lower, inst.roots, inst.ev)
    assert want["verdict"] == tl.PROXIMITY_TESTING
    assert _verify(cabi, ctx, inst, lower, inst.roots, inst.ev) == want


def test_entries_that_fill_all_512_bits(cabi):
    """A dishonest stream may fill Int<8>: the sums of 128 x 512-bit products and the 512-bit reduction are the model's"""
    inst = tl.instance(8, tl.MOD_3LIMB, 3)
    ctx = inst.z.ctx(cabi)
    proof = inst.proof.copy()
    rng = np.random.default_rng(9)
    for k in range(inst.n_cols):
        for r in range(inst.R):
            proof[inst.val_at(k, r): inst.val_at(k, r) + 64] = np.frombuffer(rng.bytes(64), dtype=np.uint8)
    inst.set_value(proof, 0, 0, -(1 << 511))
    inst.set_value(proof, 0, 1, (1 << 511) - 1)
    want = inst.expect(proof, inst.roots, inst.ev)
    assert want["verdict"] == tl.PROXIMITY_TESTING and want["bad_merkle_paths"] == inst.n_cols * inst.R
    assert _verify(cabi, ctx, inst, proof, inst.roots, inst.ev) == want
