"""CPU: the Keccak sponge of the host mirror's KeccakTranscript in transit (state() / set_state()), the form in which
zip_sumcheck_prove borrows the transcript for one sumcheck (zip_keccak_state)."""
import numpy as np
import pytest

import _oracle as orc

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383


@pytest.fixture(scope="module")
def pcs():
    from zinc_amd import pcs as p

    return p


def test_state_equals_the_oracles_sponge_at_every_length(pcs):
    data = bytes(range(256)) * 2
    for n in range(301):
        t = pcs.KeccakTranscript()
        t.absorb(data[:n])
        k = orc.new_transcript()
        orc.absorb(k, data[:n])
        st, buf = t.state()
        assert [int(w) for w in st] == [int(w) for w in k.st], n
        assert len(buf) == k.buflen == n % 136, n
        assert buf == bytes(k.buf[: k.buflen]), n


def test_set_state_continues_like_the_original(pcs):
    data = bytes(range(256)) * 2
    field = pcs.FieldConfig(BENCH_MODULUS, 4)
    for n in (0, 1, 135, 136, 137, 271, 272, 300):
        a = pcs.KeccakTranscript()
        a.absorb(data[:n])
        b = pcs.KeccakTranscript()
        b.absorb(b"something else entirely")
        b.set_state(a.state())
        assert b.get_u64() == a.get_u64(), n
        assert np.array_equal(b.get_challenge(field), a.get_challenge(field)), n
        a.absorb(data[:n])
        b.absorb(data[:n])
        sa, sb = a.state(), b.state()
        assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1], n


def test_set_state_rejects_a_full_buffer(pcs):
    t = pcs.KeccakTranscript()
    st, _ = t.state()
    with pytest.raises(pcs.InvalidPcsParam):
        t.set_state((st, bytes(136)))
    with pytest.raises(ValueError):
        t.set_state((st[:24], b""))


def test_cabi_keccak_state_layout():
    """cabi.KeccakState is zip_keccak_state: 25 words, 136 bytes, the length -- the oracle's sponge has the same layout"""
    from zinc_amd import cabi

    assert cabi.C.sizeof(cabi.KeccakState) == cabi.C.sizeof(orc.Keccak) == 25 * 8 + 136 + 4 + 4
    k = cabi.KeccakState.make(st=range(25), buf=b"abc")
    assert k.buflen == 3 and k.pending() == b"abc" and [int(w) for w in k.st] == list(range(25))
    assert "zip_sumcheck_prove" in cabi.EXPORTED_SYMBOLS and "zip_sumcheck_launch_counts" in cabi.EXPORTED_SYMBOLS
    assert "zip_sumcheck_grid_counts" in cabi.EXPORTED_SYMBOLS
