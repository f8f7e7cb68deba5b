"""Admission of the geometries above 2^26 evaluations (codewords of 32768 and 65536): zip_ctx_create accepts them and
only then looks for the device; codewords of 131072 exceed the 96-bit lanes and stay unsupported.  CPU only."""
import numpy as np
import pytest

import _oracle as orc
from zinc_amd import cabi

NO_SUCH_DEVICE = 1 << 20  # an ordinal no box has: the device check fails after the geometry checks, GPU or not

ACCEPTED = [(nv, 2) for nv in (27, 28, 29, 30)] + [(nv, 4) for nv in (25, 26, 27, 28)]


def _ctx(nv, rep):
    _, _, cw = cabi.geometry(nv, rep)
    perm = np.arange(cw, dtype=np.uint32)
    return cabi.ZipContext(nv, perm, perm, device=NO_SUCH_DEVICE, rep=rep)


@pytest.mark.parametrize("nv,rep", ACCEPTED)
def test_codewords_up_to_65536_pass_the_geometry_checks(nv, rep):
    _, _, cw = cabi.geometry(nv, rep)
    assert cw in (32768, 65536)
    with pytest.raises(cabi.ZipError) as e:
        _ctx(nv, rep)
    assert e.value.code == cabi.ZIP_ERR_NO_DEVICE


@pytest.mark.parametrize("nv,rep", [(31, 2), (29, 4)])
def test_codewords_of_131072_stay_unsupported(nv, rep):
    assert cabi.geometry(nv, rep)[2] == 131072
    with pytest.raises(cabi.ZipError) as e:
        _ctx(nv, rep)
    assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED


@pytest.mark.parametrize("nv,rep", ACCEPTED)
def test_geometry_matches_the_oracle(nv, rep):
    p = orc.Params()
    assert orc.lib().orc_params_init(orc.C.byref(p), nv, 1, rep, None, None) == 0
    assert cabi.geometry(nv, rep) == (p.row_len, p.num_rows, p.codeword_len)
    assert p.row_len * p.num_rows == 1 << nv
