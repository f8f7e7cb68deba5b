"""CPU: which (n_limbs, k_limbs, m_limbs) triples and codeword lengths zip_ctx_create admits, decided before a device is
looked for, and the declaration of zip_field_map_int."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _oracle as orc
from zinc_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(num_vars, limbs, geometry=None, rep=2, **kw):
    """zip_ctx_create's return code for the reference's geometry of num_vars (or the given slice); a ctx that was made
    (a machine with a GPU) is destroyed again."""
    row_len, num_rows, cw = geometry or cabi.geometry(num_vars, rep)
    perm1, perm2 = orc.shuffle_perm(1, cw), orc.shuffle_perm(2, cw)
    p = cabi.ZipParams(num_vars, row_len, num_rows, cw, rep, *limbs, perm1.ctypes.data_as(C.POINTER(C.c_uint32)),
                       perm2.ctypes.data_as(C.POINTER(C.c_uint32)), 0, kw.get("row_begin", 0), kw.get("row_count", 0))
    h = C.c_void_p()
    rc = cabi.lib().zip_ctx_create(C.byref(p), C.byref(h))
    if rc == cabi.ZIP_OK:
        cabi.lib().zip_ctx_destroy(h)
    else:
        assert not h.value
    return rc


def test_the_two_limb_triple_is_admitted():
    assert _create(8, (2, 8, 16)) in (cabi.ZIP_OK, cabi.ZIP_ERR_NO_DEVICE)
    assert _create(8, (1, 4, 8)) in (cabi.ZIP_OK, cabi.ZIP_ERR_NO_DEVICE)


@pytest.mark.parametrize("limbs", [(2, 4, 8), (2, 8, 8), (1, 8, 16), (3, 12, 24), (2, 4, 16), (1, 4, 16)])
def test_every_other_triple_is_unsupported(limbs):
    assert _create(8, limbs) == cabi.ZIP_ERR_UNSUPPORTED


@pytest.mark.parametrize("num_vars,geometry,rep", [(1, None, 2), (7, None, 2), (14, (8192, 2, 16384), 2), (15, (16384, 2, 32768), 2),
                                                   (15, (16384, 2, 65536), 4)])
def test_codewords_up_to_65536_are_admitted(num_vars, geometry, rep):
    """the bound the header states for a two-limb ctx: every power of two up to 65536, as for one limb"""
    assert _create(num_vars, (2, 8, 16), geometry, rep) in (cabi.ZIP_OK, cabi.ZIP_ERR_NO_DEVICE)


def test_a_codeword_above_65536_is_unsupported():
    assert _create(16, (2, 8, 16), (32768, 2, 131072), 4) == cabi.ZIP_ERR_UNSUPPORTED
    assert "up to 65536" in open(os.path.join(ROOT, "include", "zip_hip.h")).read()


def test_an_inconsistent_two_limb_geometry_is_a_parameter_error():
    """The geometry checks come after the triple's admission and hold for two limbs as for one.  (RaaCode::new's width
    assertion, code_raa.rs:68-72, is kept with 64 * n_limbs, but it cannot decide here: 128 + num_vars + 2 log2(rep) is
    at most 128 + 40 + 62 for the num_vars and the 32-bit rep the ABI takes, below the 512 bits of Int<8>.)"""
    assert _create(9, (2, 8, 16), (16, 16, 32)) == cabi.ZIP_ERR_INVALID_PARAM   # row_len * num_rows != 2^num_vars
    assert _create(8, (2, 8, 16), (16, 16, 64)) == cabi.ZIP_ERR_INVALID_PARAM   # codeword_len != row_len * rep
    assert _create(8, (2, 8, 16), (8, 32, 24), rep=3) == cabi.ZIP_ERR_INVALID_PARAM  # rep not a power of two


def test_row_shards_of_a_two_limb_ctx_are_unsupported():
    assert _create(8, (2, 8, 16), row_begin=0, row_count=8) == cabi.ZIP_ERR_UNSUPPORTED
    assert _create(8, (2, 8, 16), row_begin=8, row_count=8) == cabi.ZIP_ERR_UNSUPPORTED
    assert _create(8, (2, 8, 16), row_begin=0, row_count=16) in (cabi.ZIP_OK, cabi.ZIP_ERR_NO_DEVICE)  # all 16 rows: no shard
    # one limb: unchanged
    assert _create(8, (1, 4, 8), row_begin=8, row_count=8) in (cabi.ZIP_OK, cabi.ZIP_ERR_NO_DEVICE)


def test_field_map_int_is_exported_and_declared():
    assert "zip_field_map_int" in cabi.EXPORTED_SYMBOLS
    assert hasattr(cabi.lib(), "zip_field_map_int")
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "zip_hip.h")).read())
    assert ("int32_t zip_field_map_int(zip_ctx *ctx, const uint64_t *values, uint32_t n, uint32_t value_limbs, "
            "const zip_field *field, uint64_t *out);") in text
    assert "#define ZIP_HIP_ABI_VERSION 3" in text and cabi.lib().zip_abi_version() == 3
    # NULL arguments are refused before anything else is looked at
    out = np.zeros(4, dtype=np.uint64)
    assert cabi.lib().zip_field_map_int(None, out.ctypes.data, 1, 2, None, out.ctypes.data) == cabi.ZIP_ERR_NULL


def test_the_binding_sizes_two_limb_arrays():
    """ZipContext counts coefficients, not limbs, and hands uint64 limbs over as they are"""
    a = np.array([[1, 2], [(1 << 64) - 1, 1 << 63]], dtype=np.uint64)
    assert cabi._ints(a).dtype == np.int64 and cabi._ints(a).tobytes() == a.tobytes()
    assert cabi._ints(np.array([3, -4], dtype=np.int64)).tolist() == [3, -4]
    assert cabi._ints([5, -6]).dtype == np.int64
