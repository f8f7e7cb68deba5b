"""zip_ccs_batch without a device: the symbols, the ABI version, and every usage error a call can answer without a
handle -- with its code, in the order include/zip_hip.h documents, before a device is looked for (on a machine without
one a call that passes them all ends in ZIP_ERR_NO_DEVICE; that is how the order is read here).  The usage errors of the
calls that need a handle are in tests/test_gpu_ccs_batch.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _ccs
import _ccs_random
from zinc_amd import cabi

NAMES = ("zip_ccs_batch_create", "zip_ccs_batch_free", "zip_ccs_batch_last_error", "zip_ccs_batch_set_z",
         "zip_ccs_batch_eq_tables", "zip_ccs_batch_second_tables", "zip_ccs_batch_table", "zip_ccs_batch_download",
         "zip_ccs_batch_counts")


def test_symbols_exported_and_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "zip_hip.h")).read()
    for name in NAMES:
        assert name in cabi.EXPORTED_SYMBOLS
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(cabi.lib(), name)
    assert cabi.lib().zip_abi_version() == 3
    # any pointer of the counters may be NULL; they are monotonic and nothing here moves them
    a = C.c_uint64(7)
    cabi.lib().zip_ccs_batch_counts(None, None)
    cabi.lib().zip_ccs_batch_counts(C.byref(a), None)
    assert a.value == cabi.ccs_batch_counts()[0]


class _Create:
    """the arguments of zip_ccs_batch_create over CSR arrays that can be edited in place"""

    def __init__(self, s=3, t=3):
        self.s, self.t = s, t
        mats = _ccs_random.circuit(s, t)[0]
        self.keep = [(M.row_ptr.copy(), M.col_idx.copy(), M.values.copy()) for M in mats]
        self.arr = (cabi.SparseMatrix * 8)()
        for k, (M, (rp, ci, va)) in enumerate(zip(mats, self.keep)):
            self.arr[k] = cabi.SparseMatrix(M.n_rows, M.n_cols, rp.ctypes.data, ci.ctypes.data, va.ctypes.data)
        self.out = C.c_void_p(0xDEAD)

    def call(self, mats="arr", t=None, s=None, limbs=4, capacity=4, out="out"):
        rc = cabi.lib().zip_ccs_batch_create(0, self.arr if mats == "arr" else mats, self.t if t is None else t,
                                             self.s if s is None else s, limbs, capacity,
                                             C.byref(self.out) if out == "out" else out)
        assert rc != cabi.ZIP_OK or cabi.device_count() > 0
        if rc == cabi.ZIP_OK:  # a machine with a device: the call was valid
            cabi.lib().zip_ccs_batch_free(self.out)
            return "valid"
        if out == "out" and mats == "arr":
            assert not self.out.value, "a refused create must leave *out NULL"
        return "valid" if rc == cabi.ZIP_ERR_NO_DEVICE else rc


def test_a_valid_create_passes_every_usage_check():
    assert _Create().call() == "valid"
    assert _Create(s=1, t=1).call(limbs=2, capacity=1) == "valid"
    assert _Create(s=4, t=7).call(limbs=3, capacity=65535) == "valid"  # (65535 * 11 tables of 384 bytes)


def test_create_null_arguments():
    c = _Create()
    assert c.call(mats=None) == cabi.ZIP_ERR_NULL
    assert c.call(out=None) == cabi.ZIP_ERR_NULL
    assert c.call(mats=None, t=0, limbs=9) == cabi.ZIP_ERR_NULL  # NULL comes before the ranges


def test_create_ranges():
    c = _Create()
    for kw in ({"t": 0}, {"t": 8}, {"s": 0}, {"s": 29}, {"limbs": 1}, {"limbs": 5}, {"capacity": 0}, {"capacity": 65536}):
        assert c.call(**kw) == cabi.ZIP_ERR_INVALID_PARAM, kw
    # the ranges come before the matrices are looked at
    c.arr[1].row_ptr = None
    assert c.call(limbs=5) == cabi.ZIP_ERR_INVALID_PARAM
    assert c.call() == cabi.ZIP_ERR_NULL


def test_create_matrix_rules_are_those_of_zip_ccs_create():
    for member in ("row_ptr", "col_idx", "values"):
        c = _Create()
        setattr(c.arr[2], member, None)
        assert c.call() == cabi.ZIP_ERR_NULL, member
    c = _Create()
    assert c.call(s=2) == cabi.ZIP_ERR_SHAPE            # n_cols != 2^s
    c = _Create()
    c.arr[0].n_cols = 4
    assert c.call() == cabi.ZIP_ERR_SHAPE
    c = _Create()
    c.keep[1][0][0] = 1                                # row_ptr[0] != 0
    assert c.call() == cabi.ZIP_ERR_INVALID_PARAM
    c = _Create()
    rp = c.keep[2][0]
    rp[3] = rp[4] + 1                                  # a decreasing row_ptr
    assert c.call() == cabi.ZIP_ERR_INVALID_PARAM
    c = _Create()
    c.keep[0][1][0] = 8                                # a column index >= 2^s
    assert c.call() == cabi.ZIP_ERR_SHAPE
    # more rows than 2^s
    wide = _ccs.CsrMatrix(9, 8, [[(1, 1)]])
    c = _Create()
    c.arr[1] = cabi.SparseMatrix(9, 8, wide.row_ptr.ctypes.data, wide.col_idx.ctypes.data, wide.values.ctypes.data)
    assert c.call() == cabi.ZIP_ERR_SHAPE
    # the matrices are answered one after the other: the first offender decides
    c = _Create()
    c.keep[0][1][0] = 8
    c.arr[1].row_ptr = None
    assert c.call() == cabi.ZIP_ERR_SHAPE


def test_s_above_16_is_unsupported_and_comes_last():
    m = 1 << 17
    ident = _ccs.CsrMatrix.diagonal(np.ones(m, dtype=np.int64))
    c = _Create()
    for k in range(3):
        c.arr[k] = cabi.SparseMatrix(m, m, ident.row_ptr.ctypes.data, ident.col_idx.ctypes.data, ident.values.ctypes.data)
    assert c.call(s=17) == cabi.ZIP_ERR_UNSUPPORTED
    assert c.call(s=17, limbs=5) == cabi.ZIP_ERR_INVALID_PARAM
    assert c.call(s=17, capacity=0) == cabi.ZIP_ERR_INVALID_PARAM
    assert c.call(s=18) == cabi.ZIP_ERR_SHAPE           # the matrices of 2^17 columns against s = 18
    c.arr[2].values = None
    assert c.call(s=17) == cabi.ZIP_ERR_NULL


def test_calls_on_a_null_handle():
    L = cabi.lib()
    L.zip_ccs_batch_free(None)  # a no-op
    assert L.zip_ccs_batch_last_error(None) == b""
    x = np.zeros(8, np.uint64)
    p = C.c_void_p()
    assert L.zip_ccs_batch_set_z(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, 1, cabi.MEM_HOST) == cabi.ZIP_ERR_NULL
    assert L.zip_ccs_batch_eq_tables(None, x.ctypes.data, 0) == cabi.ZIP_ERR_NULL
    assert L.zip_ccs_batch_second_tables(None, x.ctypes.data, x.ctypes.data, x.ctypes.data) == cabi.ZIP_ERR_NULL
    assert L.zip_ccs_batch_table(None, 0, cabi.CCS_MZ, 0, C.byref(p)) == cabi.ZIP_ERR_NULL
    assert L.zip_ccs_batch_download(None, 0, cabi.CCS_MZ, 0, x.ctypes.data) == cabi.ZIP_ERR_NULL


def test_python_wrapper_reports_the_code():
    mats = _ccs_random.circuit(3, 3)[0]
    with pytest.raises(cabi.ZipError) as e:
        cabi.CcsBatch(mats, 3, 7, 4)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError) as e:
        cabi.CcsBatch(mats, 2, 4, 4)
    assert e.value.code == cabi.ZIP_ERR_SHAPE


def test_the_random_circuit_has_what_it_promises():
    for s, t in ((3, 7), (10, 7), (13, 7)):
        mats = _ccs_random.circuit(s, t)[0]
        f = _ccs_random.features(mats)
        assert f["full_column"] and f["short_matrix"] and f["empty_row"] and f["empty_column"] and f["specials"], (s, f)
        assert 3 <= f["max_row"] <= 4, (s, f)
    for s in (1, 2):  # what fits
        f = _ccs_random.features(_ccs_random.circuit(s, 7)[0])
        assert f["full_column"] and f["short_matrix"] and f["empty_column"], (s, f)
    zs = _ccs_random.witnesses(10, 5)
    assert any(len(z) < 1 << 10 for z in zs) and any(len(z) == 1 << 10 for z in zs)
