"""zip_sumcheck_prove_batch without a device: the symbols, the ABI version, and every usage error -- answered with its
code, in the documented order, before anything reaches a device, and with every transcript left byte for byte as it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from zinc_amd import cabi, pcs

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503


def test_symbols_exported_and_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "zip_hip.h")).read()
    for name in ("zip_sumcheck_prove_batch", "zip_sumcheck_batch_counts"):
        assert name in cabi.EXPORTED_SYMBOLS
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(cabi.lib(), name)
    assert "zinc_sumcheck_prove_batch" in pcs.EXPORTED_SYMBOLS
    assert hasattr(pcs.lib(), "zinc_sumcheck_prove_batch")
    assert cabi.lib().zip_abi_version() == 3
    # any pointer of the counters may be NULL; they are monotonic and nothing here moves them
    a = C.c_uint64(7)
    cabi.lib().zip_sumcheck_batch_counts(None, None, None)
    cabi.lib().zip_sumcheck_batch_counts(C.byref(a), None, None)
    assert a.value == cabi.sumcheck_batch_counts()[0]


class _Batch:
    """B instances of K tables of 2^nv elements (host), their fields and primed transcripts, as the C structures"""

    def __init__(self, B=3, K=2, nv=3, fl=4, modulus=BENCH_MODULUS):
        self.B, self.K, self.nv, self.fl = B, K, nv, fl
        rng = np.random.default_rng(5)
        self.tables = rng.integers(0, 1 << 60, size=(B, K, 1 << nv, fl), dtype=np.uint64)
        self.ptrs = [(C.c_void_p * 8)(*([self.tables[i, k].ctypes.data for k in range(K)] + [None] * (8 - K))) for i in range(B)]
        self.fields = [cabi.make_field(modulus, fl) for _ in range(B)]
        self.states = [cabi.KeccakState.make(st=range(i, i + 25), buf=bytes(range(10 * i + 1))) for i in range(B)]
        self.arr = (cabi.SumcheckInstance * B)()
        for i in range(B):
            self.arr[i].mles = C.cast(self.ptrs[i], C.c_void_p)
            self.arr[i].comb = None
            self.arr[i].field = C.pointer(self.fields[i])
            self.arr[i].transcript = C.pointer(self.states[i])
        self.msgs = np.zeros((B, nv, 5, fl), np.uint64)
        self.rand = np.zeros((B, nv, fl), np.uint64)
        self.before = [bytes(s) for s in self.states]

    def call(self, inst="arr", B=None, K=None, nv=None, degree=2, msgs="m", rand="r"):
        rc = cabi.lib().zip_sumcheck_prove_batch(
            0, self.arr if inst == "arr" else inst, self.B if B is None else B, cabi.MEM_HOST, self.K if K is None else K,
            self.nv if nv is None else nv, degree, self.msgs.ctypes.data if msgs == "m" else msgs,
            self.rand.ctypes.data if rand == "r" else rand)
        assert [bytes(s) for s in self.states] == self.before, "a refused call touched a transcript"
        return rc


def test_null_arguments():
    b = _Batch()
    assert b.call(inst=None) == cabi.ZIP_ERR_NULL
    assert b.call(msgs=None) == cabi.ZIP_ERR_NULL
    assert b.call(rand=None) == cabi.ZIP_ERR_NULL
    for member in ("mles", "field", "transcript"):
        b = _Batch()
        setattr(b.arr[1], member, None)
        assert b.call() == cabi.ZIP_ERR_NULL, member
    b = _Batch()
    b.ptrs[2][1] = None  # a table pointer of the last instance
    assert b.call() == cabi.ZIP_ERR_NULL


def test_null_comes_before_invalid_parameters():
    b = _Batch()
    b.arr[2].field = None
    b.states[0].buflen = 136
    b.before = [bytes(s) for s in b.states]
    assert b.call(degree=9) == cabi.ZIP_ERR_NULL
    assert b.call(nv=17) == cabi.ZIP_ERR_NULL


def test_invalid_parameters():
    b = _Batch()
    assert b.call(B=0) == cabi.ZIP_ERR_INVALID_PARAM
    for kw in ({"K": 0}, {"degree": 0}, {"degree": 5}, {"nv": 0}, {"nv": 31}):
        assert b.call(**kw) == cabi.ZIP_ERR_INVALID_PARAM, kw
    assert _Batch(K=8).call(K=9) == cabi.ZIP_ERR_INVALID_PARAM  # (eight tables that exist: no NULL comes first)
    # limbs: not in {2, 3, 4}; differing between instances
    for limbs in (1, 5):
        b = _Batch()
        b.fields[0].limbs = limbs
        assert b.call() == cabi.ZIP_ERR_INVALID_PARAM, limbs
    b = _Batch()
    b.fields[2] = cabi.make_field(TEST_MODULUS_2, 2)
    b.arr[2].field = C.pointer(b.fields[2])
    assert b.call() == cabi.ZIP_ERR_INVALID_PARAM
    # a comb with n_terms outside 1..8, or a mask bit at or above n_mles
    for n_terms, mask in ((0, 1), (9, 1), (1, 0b100)):
        b = _Batch()
        comb = cabi.make_comb([mask], np.ones((1, 4), np.uint64))
        comb.n_terms = n_terms
        b.arr[1].comb = C.pointer(comb)
        assert b.call() == cabi.ZIP_ERR_INVALID_PARAM, (n_terms, mask)
    # buflen >= 136
    for buflen in (136, 200):
        b = _Batch()
        b.states[1].buflen = buflen
        b.before = [bytes(s) for s in b.states]
        assert b.call() == cabi.ZIP_ERR_INVALID_PARAM, buflen


def test_more_than_65535_instances():
    """n_instances one above the range"""
    b = _Batch(B=1)
    big = (cabi.SumcheckInstance * 65536)()
    for i in range(65536):
        big[i] = b.arr[0]
    assert b.call(inst=big, B=65536) == cabi.ZIP_ERR_INVALID_PARAM


def test_num_vars_above_16_is_unsupported_and_comes_last():
    b = _Batch()
    assert b.call(nv=17) == cabi.ZIP_ERR_UNSUPPORTED  # (nothing reads the tables: their size does not matter)
    assert b.call(nv=30) == cabi.ZIP_ERR_UNSUPPORTED
    assert b.call(nv=17, degree=5) == cabi.ZIP_ERR_INVALID_PARAM
    b.states[2].buflen = 136
    b.before = [bytes(s) for s in b.states]
    assert b.call(nv=17) == cabi.ZIP_ERR_INVALID_PARAM


def test_python_wrapper_reports_the_code():
    b = _Batch()
    with pytest.raises(cabi.ZipError) as e:
        cabi.sumcheck_prove_batch([(b.tables[i], b.fields[i], b.states[i]) for i in range(b.B)], b.K, 17, 2)
    assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED
    assert [bytes(s) for s in b.states] == b.before
