"""Pins the oracle's loop over num_proximity_testing (oracle/zip_oracle.c, orc_open / orc_proof_len) before the device
is held to it: every u'_t in Python integers, the stream length of commit.rs:726, and that the column section and the
evaluation row do not depend on T beyond the transcript state they are squeezed from."""
import numpy as np
import pytest

import _oracle as orc
import _proximity as px

N_COLS = 6


@pytest.mark.parametrize("T", [1, 2, 3, 8])
@pytest.mark.parametrize("num_vars", [6, 9])
def test_oracle_stream_with_T_proximity_tests(num_vars, T):
    i = px.instance(num_vars, T, n_cols=N_COLS, seed=num_vars)
    z = i.z
    assert i.R > 1
    # the stream length (commit.rs:712-737)
    assert i.proof.size == px.stream_len(z, T, N_COLS, i.fl) == z.proof_len(i.fl)
    # every u'_t = sum_r coeffs_t[r] * w[r][c] in Python integers (open_z.rs:103-112)
    got = px.u_primes(i.proof, z, T)
    for t in range(T):
        assert got[t] == px.combine_int(i.coeffs[t], i.evals, i.R, i.C), t
    # the T = 1 stream made from the transcript state after the first (T - 1) * num_rows squeezes: its own proximity row
    # is u'_{T-1}, and its column section and evaluation row are those of the T-test stream
    fs = orc.new_transcript()
    px.squeeze_coeffs(fs, (T - 1) * i.R)
    one = px.make(num_vars, 1, n_cols=N_COLS, seed=num_vars, fs=fs)
    assert np.array_equal(one.cols, i.cols)
    assert np.array_equal(one.proof, i.proof[(T - 1) * i.C * 64:])
    # ... and both provers leave the transcript in the same state
    assert orc.lib().orc_tr_get_u64(orc.C.byref(px.copy_transcript(one.fs_after))) == \
        orc.lib().orc_tr_get_u64(orc.C.byref(px.copy_transcript(i.fs_after)))


@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_oracle_verifier_runs_every_proximity_test(T):
    """orc_verify reads T proximity rows and holds every opened column to every one of them (verify_z.rs:66-103): its
    own proof passes; a bit in any single u'_t, a T - 1 test stream and a T + 1 test stream do not."""
    i = px.instance(9, T, n_cols=N_COLS, seed=9)
    check = lambda z, proof: z.verify(i.f, i.roots, i.point, i.ev, proof)
    assert check(i.z, i.proof) == 0
    for t in range(T):
        bad = i.proof.copy()
        bad[(t * i.C + i.C - 1) * 64 + 9] ^= 1
        assert check(i.z, bad) == orc.ORC_ERR_PROOF, t
    for other in (T - 1, T + 1):
        if other >= 1:
            assert check(px.instance(9, other, n_cols=N_COLS, seed=9).z, i.proof) != 0, other


@pytest.mark.parametrize("T", [1, 3])
def test_oracle_one_row_matrix_has_no_test(T):
    """num_rows == 1 (open_z.rs:100): no proximity row, no coefficient squeezed, whatever T is."""
    i = px.make(4, T, n_cols=3, geometry=(16, 1, 32))
    assert i.R == 1 and i.coeffs is None
    assert i.proof.size == px.stream_len(i.z, T, 3, i.fl) == 3 * i.col_bytes + i.C * 8 * i.fl
    fs = orc.new_transcript()
    assert np.array_equal(px.squeeze_cols(fs, i.f, i.cw, 3), i.cols)
