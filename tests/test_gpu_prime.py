"""The random field on the device: zip_prime_test_base2 (one candidate per lane) against Python's pow, zip_get_prime
against the reference's loop on the oracle's transcript -- prime, candidates tried, the whole returned sponge and the
launches it took --, pcs.draw_random_field, and the draw_random_field check of Verifier::verify
(src/zinc/verifier.rs:53-57) on the instance of the reference's examples/simple_r1cs.rs."""
import numpy as np
import pytest

import _ccs
import _oracle as orc
import _prime

pytestmark = pytest.mark.gpu

QSTARK = 3618502788666131213697322783095070105623107215331596699973092056135872020481


@pytest.fixture(scope="module")
def mods():
    orc.build()  # before the first HIP call
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


@pytest.mark.parametrize("fl", _prime.FLS)
def test_prime_test_base2_equals_python(mods, fl):
    cabi, _ = mods
    pool = _prime.adversarial(fl) + _prime.random_odd(fl, 300, seed=2)
    want = [int(_prime.sprp2(n)) for n in pool]
    assert 0 < sum(want) < len(want)
    launches0, tested0 = cabi.prime_launch_counts()
    calls = tested = 0
    for b in (63, 64, 65, 257, len(pool)):
        got = cabi.prime_test_base2(pool[:b], fl)
        assert [int(x) for x in got] == want[:b], b
        calls, tested = calls + 1, tested + b
    for i in (0, 5, len(_prime.adversarial(fl)) - 1):  # batches of one
        assert int(cabi.prime_test_base2([pool[i]], fl)[0]) == want[i], hex(pool[i])
        calls, tested = calls + 1, tested + 1
    # the same candidates as a limb array, the tail of the pool first (another split into waves)
    got = cabi.prime_test_base2(_prime.limbs(pool[::-1][:257], fl), fl)
    assert [int(x) for x in got] == want[::-1][:257]
    assert cabi.prime_launch_counts() == (launches0 + calls + 1, tested0 + tested + 257)


def test_prime_test_base2_above_one_launch(mods):
    """more candidates than one launch takes (4096): split inside the call, same verdicts"""
    cabi, _ = mods
    pool = _prime.random_odd(2, 4096 + 65, seed=3)
    launches0, _ = cabi.prime_launch_counts()
    got = cabi.prime_test_base2(pool, 2)
    assert [int(x) for x in got] == [int(_prime.sprp2(n)) for n in pool]
    assert cabi.prime_launch_counts()[0] == launches0 + 2


@pytest.mark.parametrize("batch", [None, 64, 7])
@pytest.mark.parametrize("fl", _prime.FLS)
def test_get_prime_equals_the_references_loop(mods, monkeypatch, fl, batch):
    cabi, _ = mods
    if batch is None:
        monkeypatch.delenv("ZIP_HIP_PRIME_BATCH", raising=False)
    else:
        monkeypatch.setenv("ZIP_HIP_PRIME_BATCH", str(batch))
    width = batch or 128  # the default (include/zip_hip.h, profiles/prime_gen.md)
    counts = []
    for seed_k in range(12):
        prime, tried, st_w, pending_w = _prime.reference_get_prime(seed_k, fl)
        counts.append(tried)
        st0, pending0 = _prime.sponge(_prime.transcript(seed_k))
        state = cabi.KeccakState.make(st0, pending0)
        launches0, tested0 = cabi.prime_launch_counts()
        got, got_tried = cabi.get_prime(state, fl)
        assert (got, got_tried) == (prime, tried), seed_k
        assert tuple(int(w) for w in state.st) == st_w, seed_k
        assert state.buflen == len(pending_w) and state.pending() == pending_w, seed_k
        assert not any(state.buf[state.buflen:]), seed_k
        launches, tested = cabi.prime_launch_counts()
        assert launches - launches0 == -(-tried // width), (seed_k, tried)
        assert tested - tested0 == (launches - launches0) * width
    # what the twelve transcripts cover: a first-candidate prime, an exact multiple of 64, several batches
    if fl == 2:
        assert 1 in counts and any(c % 64 == 0 for c in counts)
    assert max(counts) > 64


@pytest.mark.parametrize("fl", _prime.FLS)
def test_draw_random_field_and_get_prime_through_the_mirror(mods, fl):
    _, pcs = mods
    for x in ([3], [-5, 0, 7], [-(2 ** 63), 2 ** 63 - 1, 0, 0], []):
        prime, tried, st_w, pending_w = _prime.reference_get_prime(0, fl, _prime.public_input_bytes(x))
        t = pcs.KeccakTranscript()
        field = pcs.draw_random_field(x, t, fl)
        assert (field.modulus, field.limbs) == (prime, fl), x
        st, pending = t.state()
        assert tuple(int(w) for w in st) == st_w and pending == pending_w, x
    for seed_k in (0, 9):
        prime, tried, st_w, pending_w = _prime.reference_get_prime(seed_k, fl)
        t = pcs.KeccakTranscript()
        t.absorb(bytes([seed_k]) * seed_k)
        assert pcs.get_prime(t, fl, want_tried=True) == (prime, tried)
        st, pending = t.state()
        assert tuple(int(w) for w in st) == st_w and pending == pending_w
    with pytest.raises(pcs.InvalidPcsParam):
        pcs.get_prime(pcs.KeccakTranscript(), 1)


def test_verifier_checks_the_drawn_field(mods):
    """examples/simple_r1cs.rs: the field is drawn from the public input on the prover's transcript, the proof made on
    that transcript; Verifier::verify draws it again on its own and compares (verifier.rs:53-57)."""
    _, pcs = mods
    inst = _ccs.vitalik_ccs(3)
    x, w = inst.z[:1], inst.z[2:]
    args = (inst.matrices, inst.s, inst.d, inst.S, inst.c)
    pt = pcs.KeccakTranscript()
    field = pcs.draw_random_field(x, pt, 4)
    assert field.modulus == _prime.reference_get_prime(0, 4, _prime.public_input_bytes(x))[0]
    # (253 bits: the reference rejects its own PCS proofs for a modulus with the top bit of its limbs set)
    assert field.modulus.bit_length() < 256
    proof = pcs.ZincProver().prove(*args, x, w, pt, field)
    verifier = pcs.ZincVerifier()
    pts = verifier.verify(*args, proof, pcs.KeccakTranscript(), field, public_input=x)
    # a different prime as config, a changed public input: the reference's first verdict, before any other work
    other = pcs.FieldConfig(QSTARK, 4)
    vt = pcs.KeccakTranscript()
    with pytest.raises(pcs.FieldConfigError):
        verifier.verify(*args, proof, vt, other, public_input=x)
    after_draw = pcs.KeccakTranscript()
    pcs.draw_random_field(x, after_draw, 4)
    assert vt.state()[0].tolist() == after_draw.state()[0].tolist() and vt.state()[1] == after_draw.state()[1]
    for changed in ([4], [3, 0], []):
        with pytest.raises(pcs.FieldConfigError):
            verifier.verify(*args, proof, pcs.KeccakTranscript(), field, public_input=changed)
    # without public_input: today's verifier, which takes the field and the transcript as handed
    got = verifier.verify(*args, proof, after_draw, field)
    assert all(np.array_equal(got[k], pts[k]) for k in ("rx_ry", "e_y", "gamma"))
    with pytest.raises((pcs.SpartanError, pcs.InvalidPcsOpen)):  # the draw not replayed: another transcript
        verifier.verify(*args, proof, pcs.KeccakTranscript(), field)
    with pytest.raises((pcs.SpartanError, pcs.InvalidPcsOpen)):  # no field check: a wrong field fails later, as today
        t = pcs.KeccakTranscript()
        pcs.draw_random_field(x, t, 4)
        verifier.verify(*args, proof, t, other)
