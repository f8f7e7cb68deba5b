"""CPU: zip_sumcheck_init_products -- the symbol is exported and declared, and every usage error is answered with its
code and *out == NULL before the device is touched (so: on a machine without one)."""
import os
import re

import numpy as np
import pytest

from zinc_amd import cabi

C = cabi.C
BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV, FL = 2, 4


def test_symbol_is_exported_and_declared():
    assert "zip_sumcheck_init_products" in cabi.EXPORTED_SYMBOLS
    assert hasattr(cabi.lib(), "zip_sumcheck_init_products")
    header = open(os.path.join(ROOT, "include", "zip_hip.h")).read()
    assert re.search(r"\bint32_t\s+zip_sumcheck_init_products\s*\(", header)
    assert cabi.lib().zip_abi_version() == 3  # additive


class _Call:
    """One zip_sumcheck_init_products call with valid arguments; the tests replace one of them."""

    def __init__(self, n_mles=3, masks=(0b011, 0b110), num_vars=NV, degree=2):
        self.tables = np.zeros((32, 1 << NV, FL), dtype=np.uint64)
        self.n_mles, self.num_vars, self.degree = n_mles, num_vars, degree
        self.arr = (C.c_void_p * 33)(*[self.tables[min(k, 31)].ctypes.data for k in range(33)])
        self.comb = cabi.make_comb(list(masks), np.ones((len(masks), FL), dtype=np.uint64))
        self.field = cabi.make_field(BENCH_MODULUS, FL)
        self.mles, self.products, self.fieldp = self.arr, C.byref(self.comb), C.byref(self.field)
        self.out = C.c_void_p(0xDEAD)  # a usage error must reset it
        self.outp = C.byref(self.out)

    def run(self):
        return cabi.lib().zip_sumcheck_init_products(0, self.mles, cabi.MEM_HOST, self.n_mles, self.num_vars, self.degree,
                                                     self.products, self.fieldp, self.outp)


@pytest.mark.parametrize("which", ["mles", "field", "products"])
def test_null_arguments(which):
    c = _Call()
    setattr(c, {"mles": "mles", "field": "fieldp", "products": "products"}[which], None)
    assert c.run() == cabi.ZIP_ERR_NULL
    if which == "products":  # (out itself was fine: it has been reset)
        assert c.out.value is None


def test_null_out():
    c = _Call()
    c.outp = None
    assert c.run() == cabi.ZIP_ERR_NULL


def _invalid(**kw):
    c = _Call(**kw)
    assert c.run() == cabi.ZIP_ERR_INVALID_PARAM, kw
    assert c.out.value is None, kw


@pytest.mark.parametrize("n_mles", [0, 33])
def test_n_mles_out_of_range(n_mles):
    _invalid(n_mles=n_mles, masks=(0b1,))


@pytest.mark.parametrize("n_terms", [0, 9])
def test_n_terms_out_of_range(n_terms):
    c = _Call()
    c.comb.n_terms = n_terms
    for t in range(8):
        c.comb.term_mask[t] = 0b11
    assert c.run() == cabi.ZIP_ERR_INVALID_PARAM
    assert c.out.value is None


@pytest.mark.parametrize("mask", [0, 0b11111])
def test_mask_with_no_bit_or_five(mask):
    _invalid(n_mles=8, masks=(0b11, mask))


def _valid(**kw):
    """Valid arguments: ZIP_ERR_NO_DEVICE where there is none (the CPU box this file is for), a handle where there is"""
    c = _Call(**kw)
    rc = c.run()
    if cabi.device_count() > 0:
        assert rc == cabi.ZIP_OK and c.out.value, kw
        cabi.lib().zip_sumcheck_free(c.out)
    else:
        assert rc == cabi.ZIP_ERR_NO_DEVICE, kw
        assert c.out.value is None, kw


@pytest.mark.parametrize("n_mles", [3, 31])
def test_mask_bit_at_n_mles(n_mles):
    _invalid(n_mles=n_mles, masks=(0b11, 1 << n_mles))


def test_mask_bit_31_of_32_tables_is_valid():
    _valid(n_mles=32, masks=(0b11, 1 << 31))


@pytest.mark.parametrize("degree", [0, 5])
def test_degree_out_of_range(degree):
    _invalid(degree=degree)


@pytest.mark.parametrize("num_vars", [0, 31])
def test_num_vars_out_of_range(num_vars):
    _invalid(num_vars=num_vars)


def test_order_of_the_checks_is_that_of_zip_sumcheck_init():
    """NULL before everything, then n_terms, then n_mles / degree / num_vars, then the masks"""
    c = _Call(n_mles=0, masks=(0,))
    c.comb.n_terms = 9
    c.fieldp = None
    assert c.run() == cabi.ZIP_ERR_NULL
    c = _Call(n_mles=0, masks=(0,))  # a bad n_mles and a bad mask: both INVALID_PARAM, *out reset
    assert c.run() == cabi.ZIP_ERR_INVALID_PARAM and c.out.value is None


@pytest.mark.parametrize("kw", [dict(), dict(n_mles=32, masks=tuple(0xF << (4 * t) for t in range(8)), degree=4),
                                dict(n_mles=4, masks=(0b0011, 0b0110, 0b0001, 0b0011), degree=4),
                                dict(n_mles=1, masks=(1,), degree=1, num_vars=1)])
def test_valid_arguments_need_a_device(kw):
    _valid(**kw)
