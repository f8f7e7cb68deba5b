"""ZincProver and ZincVerifier on the device for CCS with four to seven matrices (tests/_ccs_wide.py: the plain Plonk
gate among them): the first sumcheck runs over t + 1 = 5..8 tables on sumcheck_round_wide_kernel.  Against the oracle's
restatement of src/zinc/prover.rs and src/zinc/verifier.rs, as tests/test_gpu_spartan.py does for R1CS-shaped CCS.

On the 256-bit modulus with the top bit set the oracle (like the reference) rejects even its own proof of these
instances: FieldMap reads such a modulus as a signed number and does not keep an integer identity that has negative
entries.  There the tests compare verdicts; they demand acceptance on the other three fields."""
import functools

import numpy as np
import pytest

import _ccs
import _ccs_wide
import _oracle as orc

pytestmark = pytest.mark.gpu

Q192 = 312829638388039969874974628075306023441          # zinc/tests.rs:28
Q256 = 115792089237316195423570985008687907853269984665640564039457584007913129639747  # spartan_benches.rs:152 (top bit set)
QSTARK = 3618502788666131213697322783095070105623107215331596699973092056135872020481  # spartan_benches.rs:161
Q128 = 57316695564490278656402085503
FIELDS = [(Q192, 3), (Q256, 4), (QSTARK, 4), (Q128, 2)]
SIZES = [1, 3, 6, 10]
NAMES = list(_ccs_wide.SHAPES)
KEYS = ("msgs1", "msgs2", "V_s", "r_y")


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


@functools.lru_cache(maxsize=None)
def _oracle_proof(name, s, q, fl, label=b""):
    """(the oracle's proof, its verifier's verdict on it) -- computed once, read by several tests"""
    f = orc.make_field(q, fl)
    o = orc.Ccs(_ccs_wide.instance(name, s))
    t = orc.new_transcript()
    if label:
        orc.absorb(t, label)
    proof = o.spartan_prove(f, t)
    v = orc.new_transcript()
    if label:
        orc.absorb(v, label)
    return proof, o.spartan_verify(f, proof, v)[0]


def _args(inst):
    return inst.matrices, inst.s, inst.d, inst.S, inst.c


def _device_spartan(pcs, inst, q, fl, label=b"", with_pcs=False):
    t = pcs.KeccakTranscript()
    if label:
        t.absorb(label)
    prover = pcs.ZincProver()
    fn = prover.prove if with_pcs else prover.spartan_prove
    return fn(*_args(inst), inst.z[:1], inst.z[2:], t, pcs.FieldConfig(q, fl)), t  # z = (x, 1, w), pub_io_len = 1


@pytest.mark.parametrize("q,fl", FIELDS)
@pytest.mark.parametrize("s", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_ccs_tables_equal_the_oracle(mods, name, s, q, fl):
    """M_k z for all t matrices, the second sumcheck's table and V_s."""
    cabi, _ = mods
    inst = _ccs_wide.instance(name, s)
    f = orc.make_field(q, fl)
    o = orc.Ccs(inst)
    d = cabi.Ccs(inst.matrices, inst.s, cabi.make_field(q, fl))
    d.set_z(inst.z)
    mz_o = o.mz(f)
    for k in range(inst.t):
        assert np.array_equal(d.download(cabi.CCS_MZ, k), mz_o[k]), k
    rng = np.random.default_rng(inst.s + inst.t)
    r = orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=inst.s)], fl)
    gamma = orc.field_elems([orc.field_from_i64(f, 0x1234567890ABCDEF)], fl)[0]
    eq_o = orc.build_eq_x_r(f, r)
    vs = d.second_table(r, gamma)
    assert np.array_equal(d.download(cabi.CCS_SECOND), o.second_table(f, eq_o, gamma))
    R_inv = pow(1 << (64 * fl), -1, q)
    for k in range(inst.t):  # V_s[k] = <Mz_k, eq(r_x)>, in Python integers (Montgomery: a*b*R^-1)
        acc = sum(orc.limbs_to_int(a) * orc.limbs_to_int(b) for a, b in zip(mz_o[k], eq_o)) * R_inv % q
        assert orc.limbs_to_int(vs[k]) == acc, k
    d.free()


@pytest.mark.parametrize("q,fl", FIELDS)
@pytest.mark.parametrize("s", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_spartan_prove_equals_the_oracle(mods, name, s, q, fl):
    """SpartanProver::prove: every round message of both sumchecks, V_s and r_y; the oracle's verifier gives the device's
    proof the verdict it gives its own; a wrong witness is rejected."""
    _, pcs = mods
    inst = _ccs_wide.instance(name, s)
    f = orc.make_field(q, fl)
    want, verdict = _oracle_proof(name, s, q, fl)
    got, _ = _device_spartan(pcs, inst, q, fl)
    assert got["msgs1"].shape == (s, inst.d + 2, fl)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    rc, pts = orc.Ccs(inst).spartan_verify(f, got, orc.new_transcript())
    assert rc == verdict
    if rc == 0:  # (a rejecting verifier stops before it has the second sumcheck's point)
        assert np.array_equal(pts["r_y"], got["r_y"])
    if q != Q256:
        assert rc == 0
    elif s >= 3:
        assert rc == orc.ORC_ERR_PROOF  # (see the module's docstring; s = 1 has no constraint row and passes)
    if s >= 3:
        bad = _ccs_wide.bumped(inst)
        got, _ = _device_spartan(pcs, bad, q, fl)  # the prover still succeeds (zinc/tests.rs:184-193)
        assert np.array_equal(got["msgs1"], orc.Ccs(bad).spartan_prove(f, orc.new_transcript())["msgs1"])
        assert orc.Ccs(bad).spartan_verify(f, got, orc.new_transcript())[0] == orc.ORC_ERR_PROOF


@pytest.mark.parametrize("q,fl", FIELDS)
@pytest.mark.parametrize("s", [3, 10])
@pytest.mark.parametrize("name", ["plonk6", "t7d3"])
def test_verifier_mirror_and_matrix_evaluations(mods, name, s, q, fl):
    """zip_ccs_eval_matrices (V_xy of verify_pcs_proof, verifier.rs:248-261) for all t matrices; SpartanVerifier::verify in
    the host mirror: the oracle's points, verdicts and transcript afterwards."""
    cabi, pcs = mods
    inst = _ccs_wide.instance(name, s)
    f = orc.make_field(q, fl)
    field = pcs.FieldConfig(q, fl)
    o = orc.Ccs(inst)
    rng = np.random.default_rng(s + 40)
    rx = orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=s)], fl)
    ry = orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=s)], fl)
    d = cabi.Ccs(inst.matrices, s, cabi.make_field(q, fl))
    assert np.array_equal(d.eval_matrices(rx, ry), o.eval_matrices(f, rx, ry))
    d.free()

    proof, verdict = _oracle_proof(name, s, q, fl)
    vt = pcs.KeccakTranscript()
    if verdict != 0:
        assert q == Q256
        with pytest.raises(pcs.SpartanError):
            pcs.ZincVerifier().spartan_verify(*_args(inst), proof, vt, field)
        return
    kv = orc.new_transcript()
    rc, want = o.spartan_verify(f, proof, kv)
    got = pcs.ZincVerifier().spartan_verify(*_args(inst), proof, vt, field)
    assert rc == 0 and np.array_equal(got["rx_ry"], np.concatenate([want["r_x"], want["r_y"]]))
    assert np.array_equal(got["e_y"], want["e_y"]) and np.array_equal(got["gamma"], want["gamma"])
    assert vt.get_u64() == orc.lib().orc_tr_get_u64(orc.C.byref(kv))
    for key, idx in (("msgs1", (0, 1, 0)), ("msgs1", (s - 1, inst.d + 1, 0)), ("msgs2", (0, 0, 0)), ("V_s", (inst.t - 1, 0))):
        bad = {k: v.copy() for k, v in proof.items()}
        bad[key][idx] ^= np.uint64(2)
        assert o.spartan_verify(f, bad, orc.new_transcript())[0] == orc.ORC_ERR_PROOF
        with pytest.raises(pcs.SpartanError):
            pcs.ZincVerifier().spartan_verify(*_args(inst), bad, pcs.KeccakTranscript(), field)


@pytest.mark.parametrize("onecall", ["0", "1"])
@pytest.mark.parametrize("q,fl,s", [(Q192, 3, 6), (QSTARK, 4, 10)])
def test_plonk_gate_prove_then_verify_end_to_end(mods, monkeypatch, q, fl, s, onecall):
    """Prover::prove (Spartan, then commit / evaluate / open from the same transcript) and Verifier::verify through the
    mirror on the Plonk gate, with the per-round sumcheck loop and with zip_sumcheck_prove: the oracle's Spartan proof,
    its verdicts, and the same Fiat-Shamir state after verification."""
    _, pcs = mods
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_ONECALL", onecall)
    inst = _ccs_wide.instance("plonk6", s)
    f = orc.make_field(q, fl)
    field = pcs.FieldConfig(q, fl)
    want, verdict = _oracle_proof("plonk6", s, q, fl, b"zv")
    assert verdict == 0
    proof, _ = _device_spartan(pcs, inst, q, fl, label=b"zv", with_pcs=True)
    for key in KEYS:
        assert np.array_equal(proof[key], want[key]), key
    o = orc.Ccs(inst)
    kv = orc.new_transcript()
    orc.absorb(kv, b"zv")
    rc, pts = o.spartan_verify(f, proof, kv)
    assert rc == 0
    s1 = orc.lib().orc_tr_get_u64(orc.C.byref(kv))
    s2 = orc.lib().orc_tr_get_u64(orc.C.byref(kv))
    zp = proof["zip_proof"]
    assert orc.Zip(s, seeds=(s1, s2)).verify(f, zp["z_comm"], pts["r_y"], orc.limbs_to_int(zp["v"]), zp["pcs_proof"]) == 0
    assert o.final_check(f, pts, zp["v"]) == 0

    def fresh():
        t = pcs.KeccakTranscript()
        t.absorb(b"zv")
        return t

    vt = fresh()
    got = pcs.ZincVerifier().verify(*_args(inst), proof, vt, field)
    assert np.array_equal(got["rx_ry"][s:], pts["r_y"])
    assert vt.get_u64() == orc.lib().orc_tr_get_u64(orc.C.byref(kv))
    # another circuit (one selector entry changed): the sumchecks and the PCS pass, the final equation does not
    other = _ccs.CcsInstance(inst.m, inst.n, inst.s, inst.s_prime, inst.d, list(inst.matrices), inst.S, inst.c, inst.z)
    m3 = inst.matrices[3]
    changed = _ccs.CsrMatrix.__new__(_ccs.CsrMatrix)
    changed.n_rows, changed.n_cols, changed.row_ptr, changed.col_idx = m3.n_rows, m3.n_cols, m3.row_ptr, m3.col_idx
    changed.values = m3.values.copy()
    changed.values[0] += 1
    other.matrices[3] = changed
    with pytest.raises(pcs.SpartanError, match="e_y"):
        pcs.ZincVerifier().verify(*_args(other), proof, fresh(), field)
    wrong_v = zp["v"].copy()
    wrong_v[0] ^= np.uint64(1)
    with pytest.raises(pcs.InvalidPcsOpen):
        pcs.ZincVerifier().verify(*_args(inst), dict(proof, zip_proof=dict(zp, v=wrong_v)), fresh(), field)


def test_shapes_beyond_the_limits_stay_refused(mods):
    """d = 4 (a round polynomial of degree 5), nine terms and an S out of order give the errors they gave before."""
    _, pcs = mods
    field = pcs.FieldConfig(Q192, 3)
    prover = pcs.ZincProver()

    def run(S, c, s=3, d=None):
        inst = _ccs_wide.wide_ccs(s, S, c, seed=5)
        return prover.spartan_prove(inst.matrices, inst.s, inst.d if d is None else d, inst.S, inst.c, inst.z[:1], inst.z[2:],
                                    pcs.KeccakTranscript(), field)

    run([[0, 1, 2], [3]], [1, -1])  # d = 3 works
    with pytest.raises(pcs.InvalidPcsParam):
        run([[0, 1, 2, 3], [4]], [1, -1], s=2)  # d = 4
    with pytest.raises(pcs.InvalidPcsParam):
        run([[0, 1, 2], [3]], [1, -1], d=4)
    inst = _ccs_wide.instance("t4", 3)
    with pytest.raises(pcs.InvalidPcsParam, match="more than 8"):  # nine terms (six of them empty products)
        prover.spartan_prove(inst.matrices, inst.s, inst.d, inst.S + [[]] * 6, inst.c + [1] * 6, inst.z[:1], inst.z[2:],
                             pcs.KeccakTranscript(), field)
    with pytest.raises(pcs.InvalidPcsParam):  # S must enumerate the matrices in order
        prover.spartan_prove(inst.matrices, inst.s, inst.d, [[2], [0, 1], [3]], [1, -1, -1], inst.z[:1], inst.z[2:],
                             pcs.KeccakTranscript(), field)
