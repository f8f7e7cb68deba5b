"""The host-only pieces of the batch path, no GPU: the Fiat-Shamir walk of batch_open
(zinc_zip_batch_open_challenges, what a Rust shim runs between zip_batch_open_eval and zip_batch_open) against the
oracle's `open` looped on one transcript, and the NULL handling of the batch entry points of libzip_hip.so."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
from zinc_amd import cabi, pcs

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2)])
def test_batch_open_challenges_match_the_oracle(modulus, fl):
    num_vars, B = 8, 4
    z = orc.Zip(num_vars)
    f = orc.make_field(modulus, fl)
    rng = np.random.default_rng(11)
    fs = orc.new_transcript()
    want, rows = [], []
    for i in range(B):
        evals = rng.integers(-128, 128, size=1 << num_vars, dtype=np.int64)
        point = orc.point_to_field(f, rng.integers(-100, 100, size=num_vars, dtype=np.int64))
        rows_o, layers_o, _ = z.commit(evals)
        proof, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, fs)
        want.append((cols.copy(), coeffs.copy()))
        # the evaluation row: big-endian bytes of the Montgomery value at the end of the proof (pcs_transcript.rs:107-113)
        be = proof[-z.row_len * 8 * fl:].reshape(z.row_len, fl, 8)
        rows.append(be[:, ::-1, ::-1].copy().view("<u8").reshape(z.row_len, fl))
    rows = np.ascontiguousarray(np.stack(rows), dtype=np.uint64)

    t = pcs.PcsTranscript()
    field = pcs.FieldConfig(modulus, fl)
    coeffs = np.zeros((B, z.num_rows), np.int64)
    cols = np.zeros((B, 1000), np.uint32)
    rc = pcs.lib().zinc_zip_batch_open_challenges(z.num_rows, z.row_len, z.codeword_len, 1000, field._m.ctypes.data, fl, t._h,
                                                 rows.ctypes.data, B, coeffs.ctypes.data, cols.ctypes.data)
    assert rc == 0, pcs.lib().zinc_last_error()
    for i in range(B):
        assert np.array_equal(cols[i], want[i][0]), i
        assert np.array_equal(coeffs[i], want[i][1]), i
    assert not np.array_equal(cols[0], cols[1]) and not np.array_equal(coeffs[0], coeffs[1])
    assert t.probe() == orc.lib().orc_tr_get_u64(orc.C.byref(fs))  # the transcript afterwards


def test_batch_entry_points_handle_null():
    L = cabi.lib()
    assert L.zip_batch_size(None) == 0
    L.zip_batch_free(None)  # a no-op
    h = C.c_void_p()
    evals = np.zeros(4, np.int64)
    assert L.zip_batch_commit(None, evals.ctypes.data, 4, 1, cabi.MEM_HOST, None, C.byref(h)) == cabi.ZIP_ERR_NULL
    assert not h.value
    assert L.zip_batch_member(None, 0, C.byref(h)) == cabi.ZIP_ERR_NULL
    f = cabi.make_field(BENCH_MODULUS, 4)
    assert L.zip_batch_open_eval(None, None, C.byref(f), evals.ctypes.data, cabi.MEM_HOST) == cabi.ZIP_ERR_NULL
    assert L.zip_batch_open(None, None, None, 0, None, C.byref(f), evals.ctypes.data, cabi.MEM_HOST) == cabi.ZIP_ERR_NULL
