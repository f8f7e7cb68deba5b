"""GPU: a LinearCodeSpec with num_proximity_testing = 2 through the host mirror -- MultilinearZip::{open, verify}, the
batch entry points (which take the loop), ZincProver and ZincVerifier -- against the oracle's loop over the tests."""
import numpy as np
import pytest

import _ccs
import _oracle as orc
import _proximity as px

pytestmark = pytest.mark.gpu

Q192 = 312829638388039969874974628075306023441  # zinc/tests.rs:28
N_COLS = 10


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _spec(pcs, T=2):
    return pcs.LinearCodeSpec(num_column_opening=N_COLS, num_proximity_testing=T)


def _oracle_zip(nv, T, seeds=(1, 2)):
    z = orc.Zip(nv, seeds=seeds)
    z.p.num_proximity_testing = T
    z.p.num_column_opening = N_COLS
    return z


@pytest.mark.parametrize("nv,modulus,fl", [(9, px.BENCH_MODULUS, 4), (13, px.TEST_MODULUS_2, 2)])
def test_open_verify_round_trip_with_two_tests(mods, nv, modulus, fl):
    _, pcs = mods
    T = 2
    i = px.instance(nv, T, modulus, fl, n_cols=N_COLS)
    field = pcs.FieldConfig(modulus, fl)
    pp = pcs.MultilinearZip.setup(1 << nv, pcs.RaaCode(1 << nv, spec=_spec(pcs)))
    data, roots = pcs.MultilinearZip.commit(pp, i.evals)
    assert np.array_equal(roots, i.roots)
    t = pcs.PcsTranscript()
    pcs.MultilinearZip.open(pp, i.evals, data, i.point, field, t)
    proof = t.into_proof()
    assert np.array_equal(proof, i.proof)
    after = orc.lib().orc_tr_get_u64(orc.C.byref(px.copy_transcript(i.fs_after)))
    assert t.probe() == after
    v = np.array(orc.int_to_limbs(i.ev, fl), dtype=np.uint64)
    vt = pcs.PcsTranscript.from_proof(proof)
    pcs.MultilinearZip.verify(pp, roots, i.point, v, field, vt)
    assert vt.position() == proof.size and vt.probe() == after  # the verifier's transcript equals the prover's
    # a one-test verifier squeezes other columns and reads a shorter stream: it rejects
    one = pcs.MultilinearZip.setup(1 << nv, pcs.RaaCode(1 << nv, spec=_spec(pcs, 1)))
    with pytest.raises(pcs.InvalidPcsOpen):
        pcs.MultilinearZip.verify(one, roots, i.point, v, field, pcs.PcsTranscript.from_proof(proof))
    bad = proof.copy()
    bad[i.C * 64 + 3] ^= 1  # u'_1
    with pytest.raises(pcs.InvalidPcsOpen, match="Proximity failure"):
        pcs.MultilinearZip.verify(pp, roots, i.point, v, field, pcs.PcsTranscript.from_proof(bad))


@pytest.mark.parametrize("T", [0, 9])
def test_counts_outside_the_range_are_invalid_param(mods, T):
    _, pcs = mods
    nv = 9
    field = pcs.FieldConfig(px.BENCH_MODULUS, 4)
    evals = px.witness(nv)
    pp = pcs.MultilinearZip.setup(1 << nv, pcs.RaaCode(1 << nv, spec=_spec(pcs, T)))
    data, _ = pcs.MultilinearZip.commit(pp, evals)
    with pytest.raises(pcs.InvalidPcsParam, match=r"1 \.\. 8"):
        pcs.MultilinearZip.open(pp, evals, data, field.map_to_field([1] * nv), field, pcs.PcsTranscript())


def test_batches_take_the_loop_and_agree_with_it(mods):
    cabi, pcs = mods
    nv, B = 9, 3
    field = pcs.FieldConfig(px.BENCH_MODULUS, 4)
    pp = pcs.MultilinearZip.setup(1 << nv, pcs.RaaCode(1 << nv, spec=_spec(pcs)))
    polys = [px.witness(nv, seed=20 + k) for k in range(B)]
    points = [field.map_to_field(np.random.default_rng(k).integers(-50, 50, size=nv)) for k in range(B)]
    committed = pcs.MultilinearZip.batch_commit(pp, polys)
    datas, roots = [d for d, _ in committed], [r for _, r in committed]
    t = pcs.PcsTranscript()
    pcs.MultilinearZip.batch_open(pp, polys, datas, points, field, t)
    loop = pcs.PcsTranscript()
    for k in range(B):
        d, r = pcs.MultilinearZip.commit(pp, polys[k])
        assert np.array_equal(r, roots[k])
        pcs.MultilinearZip.open(pp, polys[k], d, points[k], field, loop)
    proofs = t.into_proof()
    assert np.array_equal(proofs, loop.into_proof()) and t.probe() == loop.probe()
    # each stream is the oracle's two-test stream of that polynomial on the shared transcript
    z, f, fs = _oracle_zip(nv, 2), orc.make_field(px.BENCH_MODULUS, 4), orc.new_transcript()
    want = [z.open(f, polys[k], *z.commit(polys[k])[:2], points[k], fs)[0] for k in range(B)]
    assert np.array_equal(proofs, np.concatenate(want))
    evs = [pcs.MultilinearZip.evaluate(pp, polys[k], points[k], field) for k in range(B)]
    calls = cabi.batch_verify_calls()
    vt = pcs.PcsTranscript.from_proof(proofs)
    pcs.MultilinearZip.batch_verify_z(pp, roots, points, evs, vt, field)
    assert cabi.batch_verify_calls() == calls  # the loop over verify, not zip_batch_verify
    assert vt.position() == proofs.size and vt.probe() == t.probe()
    lt = pcs.PcsTranscript.from_proof(proofs)
    for k in range(B):
        pcs.MultilinearZip.verify(pp, roots[k], points[k], evs[k], field, lt)
    assert lt.probe() == vt.probe()
    bad = proofs.copy()
    bad[want[0].size + z.row_len * 64 + 1] ^= 1  # u'_1 of polynomial 1
    with pytest.raises(pcs.InvalidPcsOpen, match="Proximity failure"):
        pcs.MultilinearZip.batch_verify_z(pp, roots, points, evs, pcs.PcsTranscript.from_proof(bad), field)


@pytest.mark.parametrize("name", ["vitalik", "dummy1k"])
def test_zinc_prover_and_verifier_with_two_tests(mods, name):
    """Prover::prove with spec.num_proximity_testing = 2: the PCS proof bytes equal the oracle's, as
    tests/test_gpu_spartan.py checks them for the default spec; the verifier accepts, and rejects a proof made under the
    default spec."""
    _, pcs = mods
    inst = _ccs.vitalik_ccs(3) if name == "vitalik" else _ccs.dummy_ccs_from_len(1 << 10, seed=10)
    q, fl = Q192, 3
    f, field = orc.make_field(q, fl), pcs.FieldConfig(q, fl)
    ko = orc.new_transcript()
    orc.absorb(ko, b"zinc")
    want = orc.Ccs(inst).spartan_prove(f, ko)
    s1 = orc.lib().orc_tr_get_u64(orc.C.byref(ko))
    s2 = orc.lib().orc_tr_get_u64(orc.C.byref(ko))
    z = _oracle_zip(inst.s, 2, seeds=(s1, s2))
    z_ccs = np.zeros(1 << inst.s, dtype=np.int64)  # x || 1 || w, zero-extended to m (prover.rs:230-232)
    z_ccs[: len(inst.z)] = inst.z
    rows, layers, roots_o = z.commit(z_ccs)
    proof_o, _, _ = z.open(f, z_ccs, rows, layers, want["r_y"], orc.new_transcript())
    assert proof_o.size == px.stream_len(z, 2, N_COLS, fl)

    def prove(spec):
        t = pcs.KeccakTranscript()
        t.absorb(b"zinc")
        return pcs.ZincProver(spec=spec).prove(inst.matrices, inst.s, inst.d, inst.S, inst.c, inst.z[:1], inst.z[2:], t, field)

    def verify(spec, proof):
        t = pcs.KeccakTranscript()
        t.absorb(b"zinc")
        return pcs.ZincVerifier(spec=spec).verify(inst.matrices, inst.s, inst.d, inst.S, inst.c, proof, t, field)

    got = prove(_spec(pcs))
    for key in ("msgs1", "msgs2", "V_s", "r_y"):
        assert np.array_equal(got[key], want[key]), key
    zp = got["zip_proof"]
    assert np.array_equal(zp["z_comm"], roots_o)
    assert np.array_equal(zp["pcs_proof"], proof_o)
    verify(_spec(pcs), got)
    default = prove(_spec(pcs, 1))
    assert default["zip_proof"]["pcs_proof"].size == proof_o.size - z.row_len * 64
    verify(_spec(pcs, 1), default)
    with pytest.raises(pcs.InvalidPcsOpen):
        verify(_spec(pcs), default)
