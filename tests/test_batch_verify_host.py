"""The host-only pieces of the batched verifier, no GPU: the Fiat-Shamir walk of batch_verify_z
(zinc_zip_batch_verify_challenges, what a Rust shim runs in front of the one zip_batch_verify call) against the oracle's
`open` and `verify` looped on one transcript, and the NULL handling of the new entry points of libzip_hip.so."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
from zinc_amd import cabi, pcs

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2)])
def test_batch_verify_challenges_match_the_oracle(modulus, fl):
    num_vars, B = 8, 4
    z = orc.Zip(num_vars)
    f = orc.make_field(modulus, fl)
    rng = np.random.default_rng(11)
    fs = orc.new_transcript()
    want, proofs, verify_args = [], [], []
    for i in range(B):  # the prover's side: open looped on one transcript
        evals = rng.integers(-128, 128, size=1 << num_vars, dtype=np.int64)
        point = orc.point_to_field(f, rng.integers(-100, 100, size=num_vars, dtype=np.int64))
        rows_o, layers_o, roots_o = z.commit(evals)
        proof, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, fs)
        want.append((cols.copy(), coeffs.copy()))
        proofs.append(proof)
        verify_args.append((roots_o, point, z.mle_eval(f, evals, point)))
    stream = np.concatenate(proofs)
    assert stream.size == B * z.proof_len(fl)

    t = pcs.PcsTranscript()
    field = pcs.FieldConfig(modulus, fl)
    coeffs = np.zeros((B, z.num_rows), np.int64)
    cols = np.zeros((B, 1000), np.uint32)
    rc = pcs.lib().zinc_zip_batch_verify_challenges(z.num_rows, z.row_len, z.codeword_len, 1000, field._m.ctypes.data, fl, t._h,
                                                   stream.ctypes.data, z.proof_len(fl), B, coeffs.ctypes.data, cols.ctypes.data)
    assert rc == 0, pcs.lib().zinc_last_error()
    for i in range(B):  # the verifier draws what the prover drew
        assert np.array_equal(cols[i], want[i][0]), i
        assert np.array_equal(coeffs[i], want[i][1]), i
    assert not np.array_equal(cols[0], cols[1]) and not np.array_equal(coeffs[0], coeffs[1])
    assert t.position() == 0  # the walk reads the rows where they lie; the cursor is the caller's
    # the transcript afterwards: the oracle's verifier looped over the four polynomials on one transcript
    vfs = orc.new_transcript()
    for (roots_o, point, ev), proof in zip(verify_args, proofs):
        assert z.verify(f, roots_o, point, ev, proof, fs=vfs) == 0
    assert t.probe() == orc.lib().orc_tr_get_u64(orc.C.byref(vfs))
    assert t.probe() == orc.lib().orc_tr_get_u64(orc.C.byref(fs))  # ... which is where the prover's ended up


def test_batch_verify_challenges_usage_errors():
    field = pcs.FieldConfig(BENCH_MODULUS, 4)
    t = pcs.PcsTranscript()
    L = pcs.lib()
    buf = np.zeros(64, np.uint8)
    cols = np.zeros(4, np.uint32)
    assert L.zinc_zip_batch_verify_challenges(1, 2, 4, 4, field._m.ctypes.data, 4, None, buf.ctypes.data, 64, 1, None,
                                              cols.ctypes.data) == pcs.ERR_NULL
    assert L.zinc_zip_batch_verify_challenges(1, 2, 4, 4, field._m.ctypes.data, 4, t._h, None, 64, 1, None,
                                              cols.ctypes.data) == pcs.ERR_NULL
    assert L.zinc_zip_batch_verify_challenges(2, 2, 4, 4, field._m.ctypes.data, 4, t._h, buf.ctypes.data, 64, 1, None,
                                              cols.ctypes.data) == pcs.ERR_NULL  # num_rows > 1 needs coeffs_out
    # a stream shorter than its own evaluation row (2 elements of 32 bytes)
    assert L.zinc_zip_batch_verify_challenges(1, 2, 4, 4, field._m.ctypes.data, 4, t._h, buf.ctypes.data, 63, 1, None,
                                              cols.ctypes.data) == pcs.ERR_INVALID_PARAM
    assert L.zinc_zip_batch_verify(None, buf.ctypes.data, None, None, buf.ctypes.data, 0, field._m.ctypes.data, 4, t._h) == pcs.ERR_NULL


def test_batch_verify_entry_points_need_no_gpu():
    L = cabi.lib()
    before = L.zip_batch_verify_calls()
    f = cabi.make_field(BENCH_MODULUS, 4)
    buf = np.zeros(64, np.uint8)
    cols = np.zeros(4, np.uint32)
    ev = np.zeros(4, np.uint64)
    reps = (cabi.VerifyReport * 2)()

    def call(ctx, roots, proofs, evals, reports):
        return L.zip_batch_verify(ctx, 2, roots, proofs, cabi.MEM_HOST, 64, None, cols.ctypes.data, 2, None, None, evals,
                                  C.byref(f), reports)

    assert call(None, buf.ctypes.data, buf.ctypes.data, ev.ctypes.data, reps) == cabi.ZIP_ERR_NULL
    # (the other NULL arguments are refused before the ctx is looked at: any non-NULL value stands in for one)
    fake = C.c_void_p(buf.ctypes.data)
    assert call(fake, None, buf.ctypes.data, ev.ctypes.data, reps) == cabi.ZIP_ERR_NULL
    assert call(fake, buf.ctypes.data, None, ev.ctypes.data, reps) == cabi.ZIP_ERR_NULL
    assert call(fake, buf.ctypes.data, buf.ctypes.data, None, reps) == cabi.ZIP_ERR_NULL
    assert call(fake, buf.ctypes.data, buf.ctypes.data, ev.ctypes.data, None) == cabi.ZIP_ERR_NULL
    assert L.zip_batch_verify(fake, 2, buf.ctypes.data, buf.ctypes.data, cabi.MEM_HOST, 64, None, None, 2, None, None,
                              ev.ctypes.data, C.byref(f), reps) == cabi.ZIP_ERR_NULL  # cols with n_cols != 0
    assert L.zip_batch_verify_calls() == before  # nothing reached a device
