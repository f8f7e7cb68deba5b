"""The host mirror's walk for num_proximity_testing = T: MultilinearZip::open_challenges (zinc_zip_open_challenges) is
the squeezes of prove_testing_phase / verify_testing and nothing else -- held to a replay on the oracle's transcript.
Host only: no device is touched."""
import numpy as np
import pytest

import _oracle as orc
import _proximity as px


@pytest.fixture(scope="module")
def pcs():
    from zinc_amd import pcs as m

    m.lib()
    return m


@pytest.mark.parametrize("modulus,fl", [(px.BENCH_MODULUS, 4), (px.TEST_MODULUS_2, 2)])
@pytest.mark.parametrize("T", [1, 2, 8])
def test_open_challenges_against_the_oracle_replay(pcs, T, modulus, fl):
    R, cw, n_cols = 16, 64, 7
    field = pcs.FieldConfig(modulus, fl)
    t = pcs.PcsTranscript()
    coeffs, cols = pcs.MultilinearZip.open_challenges(R, cw, n_cols, T, field, t)
    k = orc.new_transcript()
    f = orc.make_field(modulus, fl)
    want = px.squeeze_coeffs(k, T * R).reshape(T, R)  # test 0 .. test T-1 ...
    want_cols = px.squeeze_cols(k, f, cw, n_cols)     # ... then the columns
    assert coeffs.shape == (T, R) and np.array_equal(coeffs, want)
    assert np.array_equal(cols, want_cols)
    assert t.probe() == orc.lib().orc_tr_get_u64(orc.C.byref(k))


@pytest.mark.parametrize("T", [0, 9])
def test_open_challenges_refuses_counts_outside_the_range(pcs, T):
    field = pcs.FieldConfig(px.BENCH_MODULUS, 4)
    t = pcs.PcsTranscript()
    before = t.probe()
    with pytest.raises(pcs.InvalidPcsParam, match=r"1 \.\. 8"):
        pcs.MultilinearZip.open_challenges(16, 64, 5, T, field, t)
    assert t.probe() == before  # nothing was squeezed


@pytest.mark.parametrize("T", [0, 1, 3, 9])
def test_one_row_matrix_squeezes_no_coefficient(pcs, T):
    """num_rows == 1: no test at all, whatever T is (open_z.rs:100) -- only the columns are squeezed."""
    field = pcs.FieldConfig(px.BENCH_MODULUS, 4)
    t = pcs.PcsTranscript()
    coeffs, cols = pcs.MultilinearZip.open_challenges(1, 32, 5, T, field, t)
    k = orc.new_transcript()
    assert coeffs is None
    assert np.array_equal(cols, px.squeeze_cols(k, orc.make_field(px.BENCH_MODULUS, 4), 32, 5))
    assert t.probe() == orc.lib().orc_tr_get_u64(orc.C.byref(k))


def test_linear_code_spec_reaches_raa_code(pcs):
    spec = pcs.LinearCodeSpec(num_column_opening=12, num_proximity_testing=3)
    code = pcs.RaaCode(1 << 9, spec=spec)
    assert (code.s.num_column_opening, code.s.repetition_factor, code.s.num_proximity_testing) == (12, 2, 3)
    default = pcs.RaaCode(1 << 9)
    assert (default.s.num_column_opening, default.s.repetition_factor, default.s.num_proximity_testing) == (1000, 2, 1)
    assert (code.row_len, code.perm_1_seed, code.perm_2_seed) == (default.row_len, default.perm_1_seed, default.perm_2_seed)
