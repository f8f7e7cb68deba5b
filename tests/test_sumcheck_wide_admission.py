"""Admission of sumchecks over five to eight MLEs (CCS with four to seven matrices): zip_sumcheck_init accepts them and
only then looks for the device; nine tables, degree 5 and a term that names a table beyond n_mles stay refused.
CPU only."""
import numpy as np
import pytest

from zinc_amd import cabi

NO_SUCH_DEVICE = 1 << 20  # an ordinal no box has: the device check fails after the parameter checks, GPU or not
MODULUS = 312829638388039969874974628075306023441  # zinc/tests.rs:28, 3 limbs


def _init(n_mles, degree, masks=None, nv=3):
    field = cabi.make_field(MODULUS, 3)
    tables = np.zeros((n_mles, 1 << nv, 3), dtype=np.uint64)
    comb = None
    if masks is not None:
        comb = cabi.make_comb(masks, np.ones((len(masks), 3), dtype=np.uint64))
    return cabi.Sumcheck(tables, nv, degree, field, device=NO_SUCH_DEVICE, comb=comb)


@pytest.mark.parametrize("n_mles", [5, 6, 7, 8])
@pytest.mark.parametrize("degree", [1, 3, 4])
def test_five_to_eight_tables_pass_the_parameter_checks(n_mles, degree):
    with pytest.raises(cabi.ZipError) as e:
        _init(n_mles, degree)
    assert e.value.code == cabi.ZIP_ERR_NO_DEVICE
    with pytest.raises(cabi.ZipError) as e:  # the CCS form: a term over all matrices and one over the last alone
        _init(n_mles, degree, masks=[(1 << (n_mles - 1)) - 1, 1 << (n_mles - 2)])
    assert e.value.code == cabi.ZIP_ERR_NO_DEVICE


def test_up_to_four_tables_are_admitted_as_before():
    for n_mles in (1, 4):
        with pytest.raises(cabi.ZipError) as e:
            _init(n_mles, 2)
        assert e.value.code == cabi.ZIP_ERR_NO_DEVICE


def test_nine_tables_no_table_and_degree_5_stay_refused():
    with pytest.raises(cabi.ZipError) as e:
        _init(9, 3)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    for n_mles in (4, 5, 8):
        with pytest.raises(cabi.ZipError) as e:
            _init(n_mles, 5)
        assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError) as e:
        _init(0, 2)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM


@pytest.mark.parametrize("n_mles", [3, 5, 8])
def test_a_term_beyond_n_mles_is_refused(n_mles):
    with pytest.raises(cabi.ZipError) as e:
        _init(n_mles, 3, masks=[1, 1 << n_mles])
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError) as e:  # the highest table there is
        _init(n_mles, 3, masks=[1, 1 << (n_mles - 1)])
    assert e.value.code == cabi.ZIP_ERR_NO_DEVICE
