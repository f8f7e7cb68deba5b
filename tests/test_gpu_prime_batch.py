"""The fields of a whole batch on the device: zip_get_prime_batch -- the candidate chains one member per lane
(prime_chain_batch_kernel), the tests, the per-member reduction and the replay of the winner's sponge -- against the
reference's loop on the oracle's transcript (tests/_prime.py), member for member: prime, candidates tried, the whole
returned sponge.  Then the loop of zip_get_prime on the same states, the launch counters, and the host mirror:
draw_random_field_batch, check_field_batch, verify_batch_checked.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
import _prime
from test_gpu_spartan_batch import _boolean_instances, _xw

pytestmark = pytest.mark.gpu

QSTARK = 3618502788666131213697322783095070105623107215331596699973092056135872020481
DEFAULT_WINDOW = 64  # include/zip_hip.h
LAUNCHES_PER_ROUND = 4  # chain, test, reduce, replay


@pytest.fixture(scope="module")
def mods():
    orc.build()  # before the first HIP call
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _member(seed_k, prefix=b""):
    """(st, pending) of the transcript reference_get_prime(seed_k, fl, prefix) starts from"""
    k = _prime.transcript(seed_k)
    if prefix:
        orc.absorb(k, prefix)
    return _prime.sponge(k)


def _states(cabi, members):
    return [cabi.KeccakState.make(*_member(*m)) for m in members]


def _check_against_reference(cabi, members, fl, primes, tried, states):
    assert primes.shape == (len(members), fl) and tried.shape == (len(members),)
    for i, m in enumerate(members):
        prime, n, st_w, pending_w = _prime.reference_get_prime(m[0], fl, *m[1:])
        assert (orc.limbs_to_int(primes[i]), int(tried[i])) == (prime, n), (i, m)
        s = states[i]
        assert tuple(int(w) for w in s.st) == st_w, (i, m)
        assert s.buflen == len(pending_w) and s.pending() == pending_w, (i, m)
        assert not any(s.buf[s.buflen:]), (i, m)


def _rounds(members, fl, window):
    longest = max(_prime.reference_get_prime(m[0], fl, *m[1:])[1] for m in members)
    return -(-longest // window)


TWELVE = [(k,) for k in range(12)]


@pytest.mark.parametrize("fl", _prime.FLS)
def test_the_twelve_transcripts_as_one_batch(mods, monkeypatch, fl):
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_PRIME_BATCH_WINDOW", raising=False)
    counts = [_prime.reference_get_prime(k, fl)[1] for k in range(12)]
    # several rounds, and members that finish in different ones
    assert len({-(-c // DEFAULT_WINDOW) for c in counts}) >= 2 and max(counts) > DEFAULT_WINDOW
    states = _states(cabi, TWELVE)
    calls0, members0, launches0 = cabi.prime_batch_counts()
    primes, tried = cabi.get_prime_batch(states, fl)
    _check_against_reference(cabi, TWELVE, fl, primes, tried, states)
    assert cabi.prime_batch_counts() == (calls0 + 1, members0 + 12,
                                         launches0 + LAUNCHES_PER_ROUND * _rounds(TWELVE, fl, DEFAULT_WINDOW))


@pytest.mark.parametrize("window", [1, 7, 1024])
def test_window_edges_and_launches_that_follow_the_rounds_not_the_members(mods, monkeypatch, window):
    cabi, _ = mods
    fl = 2
    counts = [_prime.reference_get_prime(k, fl)[1] for k in range(12)]
    # with 7 candidates per round: a winner in the last slot of a round, the first of the next, the last of the second
    assert {7, 8, 14} <= set(counts)
    monkeypatch.setenv("ZIP_HIP_PRIME_BATCH_WINDOW", str(window))
    grown = []
    for members in (TWELVE, [m for m in TWELVE for _ in range(5)]):
        states = _states(cabi, members)
        launches0 = cabi.prime_batch_counts()[2]
        primes, tried = cabi.get_prime_batch(states, fl)
        _check_against_reference(cabi, members, fl, primes, tried, states)
        grown.append(cabi.prime_batch_counts()[2] - launches0)
    assert grown[0] == LAUNCHES_PER_ROUND * _rounds(TWELVE, fl, window)
    assert grown[1] == grown[0], "five times the members, the same launches"


@pytest.mark.parametrize("n", [1, 65, 130])
def test_partial_waves_beside_full_ones(mods, monkeypatch, n):
    cabi, _ = mods
    fl = 4
    monkeypatch.delenv("ZIP_HIP_PRIME_BATCH_WINDOW", raising=False)
    members = [(i % 12, _prime.public_input_bytes([i])) for i in range(n)]
    if n > 1:
        members[n - 1] = members[0]  # one identical pair
    states = _states(cabi, members)
    primes, tried = cabi.get_prime_batch(states, fl)
    _check_against_reference(cabi, members, fl, primes, tried, states)
    if n > 1:
        assert np.array_equal(primes[0], primes[n - 1]) and tried[0] == tried[n - 1]
        assert bytes(states[0]) == bytes(states[n - 1])


@pytest.mark.parametrize("fl", _prime.FLS)
def test_equals_the_loop_of_get_prime_and_leaves_its_counters(mods, monkeypatch, fl):
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_PRIME_BATCH_WINDOW", raising=False)
    monkeypatch.delenv("ZIP_HIP_PRIME_BATCH", raising=False)
    members = TWELVE + [(3, b"abc")]
    states, copies = _states(cabi, members), _states(cabi, members)
    single0 = cabi.prime_launch_counts()
    primes, tried = cabi.get_prime_batch(states, fl)
    assert cabi.prime_launch_counts() == single0, "the batch call moves its own counters only"
    batch0 = cabi.prime_batch_counts()
    for i, s in enumerate(copies):
        assert cabi.get_prime(s, fl) == (orc.limbs_to_int(primes[i]), int(tried[i])), i
        assert bytes(s) == bytes(states[i]), i
    assert cabi.prime_batch_counts() == batch0 and cabi.prime_launch_counts()[0] > single0[0]


PUBLIC_INPUTS = ([3], [-5, 0, 7], [-(2 ** 63), 2 ** 63 - 1, 0, 0], [], [1])


def _sponges(ts):
    return [(t.state()[0].tolist(), t.state()[1]) for t in ts]


@pytest.mark.parametrize("setting", ["loop", "batch", "default"])
@pytest.mark.parametrize("fl", _prime.FLS)
def test_draw_random_field_batch_equals_the_loop_of_draw_random_field(mods, monkeypatch, fl, setting):
    cabi, pcs = mods
    monkeypatch.delenv("ZIP_HIP_BATCH", raising=False)
    monkeypatch.delenv("ZIP_HIP_PRIME_MIN_BATCH", raising=False)
    one_by_one = [pcs.KeccakTranscript() for _ in PUBLIC_INPUTS]
    want = [pcs.draw_random_field(x, t, fl) for x, t in zip(PUBLIC_INPUTS, one_by_one)]
    if setting == "loop":
        monkeypatch.setenv("ZIP_HIP_BATCH", "0")
    elif setting == "batch":
        monkeypatch.setenv("ZIP_HIP_PRIME_MIN_BATCH", "2")
    ts = [pcs.KeccakTranscript() for _ in PUBLIC_INPUTS]
    calls0 = cabi.prime_batch_counts()[0]
    got = pcs.draw_random_field_batch(PUBLIC_INPUTS, ts, fl)
    calls = cabi.prime_batch_counts()[0] - calls0
    if setting != "default":
        assert calls == (1 if setting == "batch" else 0)
    assert [(f.modulus, f.limbs) for f in got] == [(f.modulus, f.limbs) for f in want]
    assert _sponges(ts) == _sponges(one_by_one)
    for x, f, t in zip(PUBLIC_INPUTS, got, ts):  # and the reference's
        prime, _, st_w, pending_w = _prime.reference_get_prime(0, fl, _prime.public_input_bytes(x))
        assert f.modulus == prime and (tuple(t.state()[0].tolist()), t.state()[1]) == (st_w, pending_w)
    # get_prime_batch alone, on transcripts that absorbed something
    ts = [pcs.KeccakTranscript() for _ in range(3)]
    for k, t in zip((9, 0, 11), ts):
        t.absorb(bytes([k]) * k)
    primes, tried = pcs.get_prime_batch(ts, fl, want_tried=True)
    assert list(zip(primes, tried)) == [_prime.reference_get_prime(k, fl)[:2] for k in (9, 0, 11)]


def test_check_field_batch_names_the_members_whose_field_is_not_the_drawn_one(mods, monkeypatch):
    cabi, pcs = mods
    monkeypatch.setenv("ZIP_HIP_PRIME_MIN_BATCH", "2")
    fl = 4
    drawn = [_prime.reference_get_prime(0, fl, _prime.public_input_bytes(x))[0] for x in PUBLIC_INPUTS]
    fields = [pcs.FieldConfig(q, fl) for q in drawn]
    fields[1] = pcs.FieldConfig(QSTARK, fl)  # a wrong modulus
    # the right modulus of ANOTHER limb count: the prime this input draws at 3 limbs, handed over as a 4-limb field
    fields[3] = pcs.FieldConfig(_prime.reference_get_prime(0, 3, _prime.public_input_bytes(PUBLIC_INPUTS[3]))[0], fl)
    ts = [pcs.KeccakTranscript() for _ in PUBLIC_INPUTS]
    calls0 = cabi.prime_batch_counts()[0]
    assert pcs.ZincVerifier().check_field_batch(PUBLIC_INPUTS, ts, fields) == [True, False, True, False, True]
    assert cabi.prime_batch_counts()[0] == calls0 + 1
    for x, t in zip(PUBLIC_INPUTS, ts):  # where check_field leaves it: after the draw at the field's limb count
        _, _, st_w, pending_w = _prime.reference_get_prime(0, fl, _prime.public_input_bytes(x))
        assert (tuple(t.state()[0].tolist()), t.state()[1]) == (st_w, pending_w)
    # members of two limb counts: one draw per limb count, each transcript after the draw at its own
    mixed = [pcs.FieldConfig(drawn[0], 4), pcs.FieldConfig(_prime.reference_get_prime(0, 3, _prime.public_input_bytes(PUBLIC_INPUTS[1]))[0], 3),
             pcs.FieldConfig(drawn[2], 4), pcs.FieldConfig(QSTARK, 4)]
    ts = [pcs.KeccakTranscript() for _ in mixed]
    assert pcs.ZincVerifier().check_field_batch(PUBLIC_INPUTS[:4], ts, mixed) == [True, True, True, False]
    for x, f, t in zip(PUBLIC_INPUTS, mixed, ts):
        _, _, st_w, pending_w = _prime.reference_get_prime(0, f.limbs, _prime.public_input_bytes(x))
        assert (tuple(t.state()[0].tolist()), t.state()[1]) == (st_w, pending_w)


def test_verify_batch_checked_reports_the_member_with_the_wrong_field(mods, monkeypatch):
    """three proofs of the instance of tests/test_gpu_verify_batch.py (A = B = C = I, 16 rows), each in the field drawn
    from its own public input on its own labelled transcript, as examples/simple_r1cs.rs draws it"""
    cabi, pcs = mods
    monkeypatch.setenv("ZIP_HIP_PRIME_MIN_BATCH", "2")
    fl, s = 4, 4
    insts = _boolean_instances(s, 3)
    xs = [_xw(i.z)[0] for i in insts]
    # labels whose drawn prime leaves the top bit of its limbs clear (the reference rejects its own PCS proofs otherwise:
    # tests/test_gpu_prime.py) -- chosen by the reference's loop, not by the code under test
    labels = []
    for k in range(64):
        label = b"prime-batch-%d" % k
        if len(labels) < 3 and _prime.reference_get_prime(0, fl, label + _prime.public_input_bytes(xs[len(labels)]))[0].bit_length() < 256:
            labels.append(label)
    assert len(labels) == 3

    def transcripts():
        ts = [pcs.KeccakTranscript() for _ in labels]
        for t, label in zip(ts, labels):
            t.absorb(label)
        return ts

    pts = transcripts()
    fields = pcs.draw_random_field_batch(xs, pts, fl)
    base = insts[0]
    proofs = pcs.ZincProver().prove_batch(base.matrices, base.s, base.d, base.S, base.c, xs, [_xw(i.z)[1] for i in insts], pts, fields)
    handed = list(fields)
    handed[2] = pcs.FieldConfig(QSTARK, fl)
    vts = transcripts()
    got = pcs.ZincVerifier().verify_batch_checked(base.matrices, base.s, base.d, base.S, base.c, proofs, vts, handed, xs)
    assert got[0] is None and got[1] is None, got
    assert isinstance(got[2], pcs.FieldConfigError), got[2]
    after_check = transcripts()
    pcs.draw_random_field(xs[2], after_check[2], fl)
    assert _sponges(vts[2:]) == _sponges(after_check[2:])
    # the members that passed: where `verify` with the field check leaves them
    for i in (0, 1):
        t = transcripts()[i]
        pcs.ZincVerifier().verify(base.matrices, base.s, base.d, base.S, base.c, proofs[i], t, fields[i], public_input=xs[i])
        assert _sponges([vts[i]]) == _sponges([t]), i
