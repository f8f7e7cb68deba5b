"""zip_get_prime_batch without a device: the symbols are exported and declared as the headers state them, every usage
error gets its code in the documented order before any device is looked for -- transcripts and counters unchanged --, and
the window knob goes through prime_batch_knob (garbage keeps the default)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _prime
from zinc_amd import cabi, pcs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ZIP_SIGNATURES = {
    "zip_get_prime_batch": ("int32_t", "int32_t device, zip_keccak_state *transcripts, uint32_t n, uint32_t limbs, "
                                       "uint64_t *primes_out, uint32_t *candidates_tried_out"),
    "zip_prime_batch_counts": ("void", "uint64_t *calls, uint64_t *members, uint64_t *kernel_launches"),
}
ZINC_SIGNATURES = {
    "zinc_get_prime_batch": ("int32_t", "zinc_transcript *const *transcripts, uint32_t n, uint32_t limbs, int32_t device, "
                                        "uint64_t *primes_out, uint32_t *candidates_tried_out"),
    "zinc_draw_random_field_batch": ("int32_t", "const int64_t *const *public_inputs, const size_t *lens, "
                                                "zinc_transcript *const *transcripts, uint32_t n, uint32_t limbs, int32_t device, "
                                                "uint64_t *moduli_out"),
    "zinc_verifier_check_field_batch": ("int32_t", "const int64_t *const *public_inputs, const size_t *lens, "
                                                   "zinc_transcript *const *transcripts, uint32_t n, const uint64_t *moduli, "
                                                   "const uint32_t *limbs, int32_t device, uint8_t *same_out"),
}


def _declared(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^;]*)\);", text, re.M)
    assert m, name
    return m.group(1), " ".join(m.group(2).split())


def test_symbols_exported_and_declared_with_the_headers_signatures():
    for name, want in ZIP_SIGNATURES.items():
        assert name in cabi.EXPORTED_SYMBOLS, name
        assert hasattr(cabi.lib(), name), name
        assert _declared("zip_hip.h", name) == want, name
    for name, want in ZINC_SIGNATURES.items():
        assert name in pcs.EXPORTED_SYMBOLS, name
        assert hasattr(pcs.lib(), name), name
        assert _declared("zinc_zip_host.h", name) == want, name
    assert hasattr(pcs.lib(), "zinc_verifier_verify_batch_checked")
    assert cabi.lib().zip_abi_version() == 3
    assert callable(cabi.get_prime_batch) and callable(cabi.prime_batch_counts)
    assert callable(pcs.get_prime_batch) and callable(pcs.draw_random_field_batch)
    assert callable(pcs.ZincVerifier.check_field_batch) and callable(pcs.ZincVerifier.verify_batch_checked)
    cabi.lib().zip_prime_batch_counts(None, None, None)  # any pointer may be NULL
    a = C.c_uint64(7)
    cabi.lib().zip_prime_batch_counts(None, C.byref(a), None)
    assert a.value == cabi.prime_batch_counts()[1]


def _three_states():
    arr = (cabi.KeccakState * 3)()
    for i in range(3):
        for w in range(25):
            arr[i].st[w] = 1000 * i + w + 1
        for b in range(136):
            arr[i].buf[b] = (7 * i + b) & 0xFF
        arr[i].buflen = 10 * i + 3
    return arr


def test_usage_errors_in_the_stated_order_with_no_device():
    L = cabi.lib()
    arr = _three_states()
    before = bytes(arr)
    counts = cabi.prime_batch_counts()
    single = cabi.prime_launch_counts()
    primes = np.zeros((3, 4), np.uint64)
    tried = (C.c_uint32 * 3)()
    call = L.zip_get_prime_batch
    NULL, INVALID = cabi.ZIP_ERR_NULL, cabi.ZIP_ERR_INVALID_PARAM
    # 1. NULL comes first, whatever else is wrong
    assert call(0, None, 3, 4, primes.ctypes.data, tried) == NULL
    assert call(0, arr, 3, 4, None, tried) == NULL
    assert call(-1, None, 0, 9, None, None) == NULL
    assert call(0, arr, 0, 9, None, None) == NULL
    # 2. limbs, before n and before the members
    for fl in (0, 1, 5, 8):
        assert call(0, arr, 3, fl, primes.ctypes.data, tried) == INVALID
        assert call(-1, arr, 0, fl, primes.ctypes.data, None) == INVALID
    # 3. n
    for n in (0, 65536, 1 << 31):
        assert call(0, arr, n, 4, primes.ctypes.data, None) == INVALID, n
        assert call(-1, arr, n, 4, primes.ctypes.data, None) == INVALID, n
    # 4. a member's buflen: any member, the last one included
    for bad in (0, 1, 2):
        for buflen in (136, 137, 0xFFFFFFFF):
            keep = arr[bad].buflen
            arr[bad].buflen = buflen
            assert call(0, arr, 3, 4, primes.ctypes.data, tried) == INVALID, (bad, buflen)
            assert call(-1, arr, 3, 4, primes.ctypes.data, tried) == INVALID, "before any device is looked for"
            arr[bad].buflen = keep
    # only now the device: an ordinal that cannot exist
    assert call(-1, arr, 3, 4, primes.ctypes.data, tried) == cabi.ZIP_ERR_NO_DEVICE
    assert call(1 << 20, arr, 3, 2, primes.ctypes.data, None) == cabi.ZIP_ERR_NO_DEVICE
    assert bytes(arr) == before, "on every non-zero return the transcripts are byte-for-byte unchanged"
    assert not primes.any() and not any(tried)
    assert cabi.prime_batch_counts() == counts and cabi.prime_launch_counts() == single


def test_the_python_wrapper_raises_what_the_library_answers():
    states = [cabi.KeccakState.make() for _ in range(2)]
    with pytest.raises(cabi.ZipError) as e:
        cabi.get_prime_batch(states, 5)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError) as e:
        cabi.get_prime_batch([], 4)
    assert e.value.code == cabi.ZIP_ERR_NULL  # no members: no primes to point at
    with pytest.raises(pcs.InvalidPcsParam):
        pcs.get_prime_batch([pcs.KeccakTranscript(), pcs.KeccakTranscript()], 1)
    with pytest.raises(pcs.InvalidPcsParam):
        pcs.draw_random_field_batch([[1], [2]], [pcs.KeccakTranscript(), pcs.KeccakTranscript()], 5)
    assert pcs.get_prime_batch([], 4) == [] and pcs.draw_random_field_batch([], [], 4) == []


def test_window_knob_keeps_the_default_for_garbage_and_out_of_range(tmp_path):
    """ZIP_HIP_PRIME_BATCH_WINDOW is read through prime_batch_knob with (default 64, max 1024): the parser's own test, at
    those bounds"""
    pd = _prime.build_host_check(str(tmp_path))
    for text, want in ((None, 64), (b"", 64), (b"1", 1), (b"7", 7), (b"1024", 1024), (b"0", 64), (b"1025", 64), (b"-3", 64),
                       (b"abc", 64), (b"12abc", 64), (b" 7", 64), (b"7 ", 64), (b"1e3", 64), (b"99999999999999999999", 64),
                       (b"0x40", 64), (b"007", 7)):
        assert pd.pd_batch_knob(text, 64, 1024) == want, text
    src = open(os.path.join(ROOT, "zinc_amd", "csrc", "zip_hip.hip")).read()
    assert re.search(r'prime_batch_knob\(getenv\("ZIP_HIP_PRIME_BATCH_WINDOW"\), kPrimeBatchDefaultWindow, kPrimeBatchMaxWindow\)', src)
    assert "kPrimeBatchDefaultWindow = 64, kPrimeBatchMaxWindow = 1024" in src
    for doc in ("README.md", os.path.join("include", "zip_hip.h")):
        assert "ZIP_HIP_PRIME_BATCH_WINDOW" in open(os.path.join(ROOT, doc)).read(), doc
    assert "ZIP_HIP_PRIME_MIN_BATCH" in open(os.path.join(ROOT, "README.md")).read()
