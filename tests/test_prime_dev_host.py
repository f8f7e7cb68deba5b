"""CPU: zinc_amd/csrc/prime_dev.cuh -- the lane function of prime_test_base2_kernel, the candidate chain of zip_get_prime
and the knob parser -- compiled for the host and held to Python's pow and to the oracle's KeccakTranscript; and the
admission checks of the three zip_prime_* / zip_get_prime entry points, which need no device."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
import _prime


@pytest.fixture(scope="module")
def pd(tmp_path_factory):
    return _prime.build_host_check(str(tmp_path_factory.mktemp("prime_dev")))


def _verdicts(pd, values, fl):
    c = _prime.limbs(values, fl)
    out = np.zeros(len(values), np.uint8)
    assert pd.pd_test_base2(fl, C.c_void_p(c.ctypes.data), len(values), C.c_void_p(out.ctypes.data)) == 0
    return [int(x) for x in out]


@pytest.mark.parametrize("fl", _prime.FLS)
def test_lane_function_on_the_adversarial_list(pd, fl):
    values = _prime.adversarial(fl)
    got = _verdicts(pd, values, fl)
    for n, g in zip(values, got):
        assert g == int(_prime.sprp2(n)), hex(n)
    # composite, and accepted because the reference accepts them
    for n in (2047, (1 << 64) + 1, (1 << 128) + 1, (1 << 67) - 1, (1 << 137) - 1, (1 << 211) - 1):
        if n < 1 << (64 * fl):
            assert _verdicts(pd, [n], fl) == [1], hex(n)


@pytest.mark.parametrize("fl", _prime.FLS)
def test_lane_function_on_random_values_and_semiprimes(pd, fl):
    values = _prime.random_odd(fl, 2000) + _prime.semiprimes(fl, 200)
    got = _verdicts(pd, values, fl)
    want = [int(_prime.sprp2(n)) for n in values]
    assert got == want
    assert sum(want[:2000]) > 0, "no prime among the random values: the test shows one side only"


@pytest.mark.parametrize("fl", _prime.FLS)
def test_outside_the_contract_is_composite_and_terminates(pd, fl):
    assert _verdicts(pd, [0, 1, 2, 4, 6, (1 << (64 * fl)) - 2, 1 << 64], fl) == [0] * 7


@pytest.mark.parametrize("fl", _prime.FLS)
def test_candidate_chain_and_restored_sponge_at_every_buflen(pd, fl):
    orc.build()
    count = 8
    for p in range(136):
        k = orc.new_transcript()
        orc.absorb(k, bytes((7 * i + p) & 0xFF for i in range(136 + p)))  # one full block, then p pending bytes
        assert k.buflen == p
        st0, pending0 = _prime.sponge(k)
        st = np.array(st0, np.uint64)
        buf = np.zeros(136, np.uint8)
        buf[:p] = np.frombuffer(pending0, np.uint8)
        cands = np.zeros((count, fl), np.uint64)
        st_out, buf_out, len_out = np.zeros((count, 25), np.uint64), np.ones((count, 136), np.uint8), np.zeros(count, np.uint32)
        assert pd.pd_chain(fl, C.c_void_p(st.ctypes.data), C.c_void_p(buf.ctypes.data), p, count, C.c_void_p(cands.ctypes.data),
                           C.c_void_p(st_out.ctypes.data), C.c_void_p(buf_out.ctypes.data), C.c_void_p(len_out.ctypes.data)) == 0
        for i in range(count):
            want = _prime.next_candidate(k, fl)
            assert orc.limbs_to_int(cands[i]) == want, (p, i)
            st_w, pending_w = _prime.sponge(k)
            assert [int(x) for x in st_out[i]] == st_w, (p, i)
            assert int(len_out[i]) == len(pending_w) and bytes(buf_out[i, : len(pending_w)]) == pending_w, (p, i)
            assert not buf_out[i, len(pending_w):].any(), (p, i)


@pytest.mark.parametrize("fl", _prime.FLS)
def test_sequential_restatement_finds_the_references_prime(pd, fl):
    """the reference's loop with the host build of the lane function (the CPU restatement tools/prime_times.py times)"""
    for seed_k in (0, 9):
        prime, tried, st_w, pending_w = _prime.reference_get_prime(seed_k, fl)
        st0, pending0 = _prime.sponge(_prime.transcript(seed_k))
        st = np.array(st0, np.uint64)
        buf = np.zeros(136, np.uint8)
        buf[: len(pending0)] = np.frombuffer(pending0, np.uint8)
        n = C.c_uint32(len(pending0))
        out = np.zeros(fl, np.uint64)
        got = pd.pd_get_prime(fl, C.c_void_p(st.ctypes.data), C.c_void_p(buf.ctypes.data), C.byref(n), C.c_void_p(out.ctypes.data), 65536)
        assert (got, orc.limbs_to_int(out)) == (tried, prime)
        assert tuple(int(x) for x in st) == st_w and bytes(buf[: n.value]) == pending_w and not buf[n.value:].any()


def test_knob_parser_keeps_the_default_for_garbage_and_out_of_range(pd):
    for text, want in ((None, 256), (b"", 256), (b"64", 64), (b"1", 1), (b"4096", 4096), (b"0", 256), (b"4097", 256),
                       (b"-3", 256), (b"abc", 256), (b"12abc", 256), (b" 7", 256), (b"7 ", 256), (b"1e3", 256),
                       (b"99999999999999999999", 256), (b"0x40", 256), (b"007", 7)):
        assert pd.pd_batch_knob(text, 256, 4096) == want, text


def test_admission_needs_no_device():
    from zinc_amd import cabi

    L = cabi.lib()
    before = cabi.prime_launch_counts()
    good = _prime.limbs([7, 11], 2)
    out = np.zeros(2, np.uint8)
    assert L.zip_prime_test_base2(0, None, 2, 2, out.ctypes.data) == cabi.ZIP_ERR_NULL
    assert L.zip_prime_test_base2(0, good.ctypes.data, 2, 2, None) == cabi.ZIP_ERR_NULL
    for fl in (0, 1, 5, 8):
        assert L.zip_prime_test_base2(0, good.ctypes.data, 1, fl, out.ctypes.data) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_prime_test_base2(0, good.ctypes.data, 0, 2, out.ctypes.data) == cabi.ZIP_ERR_INVALID_PARAM
    for bad in ([7, 10], [1, 7], [7, 0], [2, 3], [1 << 64, 7]):
        b = _prime.limbs(bad, 2)
        assert L.zip_prime_test_base2(0, b.ctypes.data, 2, 2, out.ctypes.data) == cabi.ZIP_ERR_INVALID_PARAM, bad
    st = cabi.KeccakState.make()
    prime = np.zeros(4, np.uint64)
    assert L.zip_get_prime(0, None, 4, prime.ctypes.data, None) == cabi.ZIP_ERR_NULL
    assert L.zip_get_prime(0, C.byref(st), 4, None, None) == cabi.ZIP_ERR_NULL
    for fl in (0, 1, 5):
        assert L.zip_get_prime(0, C.byref(st), fl, prime.ctypes.data, None) == cabi.ZIP_ERR_INVALID_PARAM
    st.buflen = 136
    assert L.zip_get_prime(0, C.byref(st), 4, prime.ctypes.data, None) == cabi.ZIP_ERR_INVALID_PARAM
    st.buflen = 0
    assert L.zip_get_prime(-1, C.byref(st), 4, prime.ctypes.data, None) == cabi.ZIP_ERR_NO_DEVICE
    assert cabi.prime_launch_counts() == before
    assert not prime.any() and st.buflen == 0 and not any(st.st)
    L.zip_prime_launch_counts(None, None)  # either pointer may be NULL
