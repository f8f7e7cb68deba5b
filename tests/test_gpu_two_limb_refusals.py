"""What a live two-limb ctx refuses: every entry point of the header's list answers ZIP_ERR_UNSUPPORTED with a
zip_ctx_last_error text that says "two-limb", launches nothing and leaves the ctx usable; and a one-limb ctx made beside
it in the same process still produces the oracle's proof.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc
import _two_limb as tl

pytestmark = pytest.mark.gpu

BENCH_MODULUS = tl.BENCH_MODULUS


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _refused(cabi, ctx, rc, what):
    assert rc == cabi.ZIP_ERR_UNSUPPORTED, (what, rc)
    text = cabi.lib().zip_ctx_last_error(ctx._h).decode()
    assert "two-limb" in text, (what, text)


def test_every_refusal_on_a_live_ctx_and_the_ctx_stays_usable(cabi):
    import torch

    L = cabi.lib()
    z = tl.Zip2(8)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = tl.witness(z)
    rows_o, layers_o, roots_o = z.commit(evals)
    point = tl.make_point(f, 8)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point)
    q0, q1 = z.tensors(f, point)
    ctx = z.ctx(cabi)
    com, roots = ctx.commit(evals)
    assert np.array_equal(roots, roots_o)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.profile_read()

    R, Cn, cw = z.num_rows, z.row_len, z.codeword_len
    ev_d = torch.from_numpy(evals.view(np.int64).copy()).cuda()
    out_d = torch.zeros(proof_o.size, dtype=torch.uint8, device="cuda")
    u64_d = torch.zeros(Cn * 16, dtype=torch.int64, device="cuda")
    cols_c = np.ascontiguousarray(cols, dtype=np.uint32)
    coeffs_c = np.ascontiguousarray(coeffs)
    q0_c, q1_c = np.ascontiguousarray(q0), np.ascontiguousarray(q1)
    h = C.c_void_p()

    # proximity tests above one (one is what the ctx has)
    _refused(cabi, ctx, L.zip_ctx_set_proximity_tests(ctx._h, 2), "zip_ctx_set_proximity_tests(2)")
    assert L.zip_ctx_set_proximity_tests(ctx._h, 1) == cabi.ZIP_OK and ctx.proximity_tests == 1
    # the row-shard open and the fold of shard partials
    _refused(cabi, ctx, L.zip_open_shard(com._h, ev_d.data_ptr(), coeffs_c.ctypes.data, cols_c.ctypes.data, cols_c.size, q0_c.ctypes.data,
                                         C.byref(zf), u64_d.data_ptr(), u64_d.data_ptr(), out_d.data_ptr()), "zip_open_shard")
    _refused(cabi, ctx, L.zip_sum_partials(ctx._h, u64_d.data_ptr(), None, 1, C.byref(zf), u64_d.data_ptr(), None), "zip_sum_partials")
    # jobs
    _refused(cabi, ctx, L.zip_commit_open_begin(ctx._h, ev_d.data_ptr(), R * Cn, coeffs_c.ctypes.data, cols_c.ctypes.data, cols_c.size,
                                                q0_c.ctypes.data, C.byref(zf), out_d.data_ptr(), C.byref(h)), "zip_commit_open_begin")
    assert not h.value
    # the streaming writer
    pieces = []
    sink = cabi.PROOF_SINK(lambda user, p, n: pieces.append(n) or 0)
    _refused(cabi, ctx, L.zip_open_stream(com._h, evals.ctypes.data, cabi.MEM_HOST, coeffs_c.ctypes.data, cols_c.ctypes.data, cols_c.size,
                                          q0_c.ctypes.data, C.byref(zf), sink, None, 0), "zip_open_stream")
    assert not pieces
    # batches
    _refused(cabi, ctx, L.zip_batch_commit(ctx._h, evals.ctypes.data, R * Cn, 1, cabi.MEM_HOST, None, C.byref(h)), "zip_batch_commit")
    p1, p2 = np.ascontiguousarray(z.perm1), np.ascontiguousarray(z.perm2)
    _refused(cabi, ctx, L.zip_batch_commit_codes(ctx._h, evals.ctypes.data, R * Cn, 1, cabi.MEM_HOST, p1.ctypes.data, p2.ctypes.data, None,
                                                 C.byref(h)), "zip_batch_commit_codes")
    assert not h.value
    rep = cabi.VerifyReport()
    ev_m = np.array(orc.int_to_limbs(0, 4), dtype=np.uint64)
    proof_c = np.ascontiguousarray(proof_o)
    _refused(cabi, ctx, L.zip_batch_verify(ctx._h, 1, roots_o.ctypes.data, proof_c.ctypes.data, cabi.MEM_HOST, proof_c.size,
                                           coeffs_c.ctypes.data, cols_c.ctypes.data, cols_c.size, q0_c.ctypes.data, q1_c.ctypes.data,
                                           ev_m.ctypes.data, C.byref(zf), C.byref(rep)), "zip_batch_verify")
    proofs = (C.c_void_p * 1)(proof_c.ctypes.data)
    lens = (C.c_size_t * 1)(proof_c.size)
    fields = (C.c_void_p * 1)(C.addressof(zf))
    _refused(cabi, ctx, L.zip_batch_verify_codes(ctx._h, 1, p1.ctypes.data, p2.ctypes.data, roots_o.ctypes.data, proofs, lens, cabi.MEM_HOST,
                                                 coeffs_c.ctypes.data, cols_c.ctypes.data, cols_c.size, q0_c.ctypes.data, q1_c.ctypes.data,
                                                 ev_m.ctypes.data, fields, C.byref(rep)), "zip_batch_verify_codes")
    # speculation stays off whatever it is set to: the call succeeds and changes nothing
    ctx.set_speculation(True)
    # nothing was launched by any of them
    assert ctx.profile_read() == {}
    ctx.set_profiling(False)

    # zip_mctx_create and row shards: refused where the ctx would be made
    p = cabi.ZipParams(8, Cn, R, cw, 2, 2, 8, 16, p1.ctypes.data_as(C.POINTER(C.c_uint32)), p2.ctypes.data_as(C.POINTER(C.c_uint32)),
                       0, 0, 0)
    devices = (C.c_int32 * 1)(0)
    m = C.c_void_p()
    assert L.zip_mctx_create(C.byref(p), 1, devices, C.byref(m)) == cabi.ZIP_ERR_UNSUPPORTED and not m.value
    with pytest.raises(cabi.ZipError) as e:
        cabi.ZipContext(8, p1, p2, n_limbs=2, k_limbs=8, m_limbs=16, row_begin=0, row_count=R // 2)
    assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED

    # the ctx is as usable as before: commit + open still match, with and without the handle made before the refusals
    assert np.array_equal(com.open(evals, coeffs, cols, q0, zf), proof_o)
    com2, roots2 = ctx.commit(ev_d)
    assert np.array_equal(roots2, roots_o)
    assert np.array_equal(com2.open(ev_d, coeffs, cols, q0, zf), proof_o)
    proof3, roots3, _ = ctx.commit_open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(proof3, proof_o) and np.array_equal(roots3, roots_o)
    ev = z.mle_eval(f, evals, point)
    got = ctx.verify(roots_o, proof3, coeffs, cols, q0, q1, np.array(orc.int_to_limbs(ev, 4), dtype=np.uint64), zf)
    assert got["verdict"] == cabi.VERIFY_ACCEPT


def test_a_one_limb_ctx_beside_a_two_limb_ctx_is_unchanged(cabi):
    z2 = tl.Zip2(10)
    ctx2 = z2.ctx(cabi)
    evals2 = tl.witness(z2)
    com2, roots2 = ctx2.commit(evals2)

    z = orc.Zip(10)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = orc.splitmix64(0x5A494E43, 1 << 10).copy()
    evals[:4] = np.array([-(2**63), 2**63 - 1, -1, 0], dtype=np.int64)
    point = orc.point_to_field(f, np.random.default_rng(3).integers(-100, 100, size=10, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    ctx = cabi.ZipContext(10, z.perm1, z.perm2)
    q0 = orc.build_eq_x_r(f, point[5:])
    for _ in range(2):  # the second commit hints itself with the first opening's columns, as it always has
        com, roots = ctx.commit(evals)
        assert np.array_equal(roots, roots_o)
        assert np.array_equal(com.open(evals, coeffs, cols, q0, zf), proof_o)
    proof, roots, _ = ctx.commit_open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(proof, proof_o) and np.array_equal(roots, roots_o)
    r, l, t = com.download()
    assert np.array_equal(r, rows_o) and np.array_equal(l, layers_o[:, :-1, :]) and np.array_equal(t, roots_o)
    # ... and the two-limb ctx beside it still matches its own oracle
    rows2_o, _, roots2_o = z2.commit(evals2)
    assert np.array_equal(roots2, roots2_o) and np.array_equal(com2.download(layers=False, roots=False)[0], rows2_o)
