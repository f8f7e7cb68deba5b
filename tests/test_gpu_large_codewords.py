"""Polynomials above 2^26 evaluations (codewords 32768 and 65536: raa_commit_slab_kernel) on the GPU against the
oracle: row shards of 2^27 .. 2^30 at rep 2 and 2^25 at rep 4 (every row entry, tree node and root), the whole 2^27
on one device (all roots, 64 whole opening blocks, every commit / open path byte-identical, the verifiers, zip_mctx),
and the whole 2^28 (sampled roots, zip_verify on the whole stream)."""
import os

import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    from zinc_amd import cabi

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, torch


def _witness(seed, rows, row_len):
    """splitmix rows, the first three replaced by the extremes: all i64::MIN, all i64::MAX, alternating (at cw 65536
    these reach the 96-bit bound of the lanes)."""
    w = orc.splitmix64(seed, rows * row_len).reshape(rows, row_len)
    w[0] = I64_MIN
    w[1] = I64_MAX
    w[2, 0::2] = I64_MIN
    w[2, 1::2] = I64_MAX
    return w.reshape(-1)


@pytest.mark.parametrize("nv,rep,rows,begin", [
    (27, 2, 24, 1000), (28, 2, 24, 3000), (29, 2, 16, 5000), (30, 2, 16, 7777), (25, 4, 24, 100),
    # more rows than resident workgroups: the persistent loop runs a second round, and the upper levels of the first
    # chunk go the deferred way (ChunkFinisher::after_hash of the next row) -- at both entry counts, E = 32 and 64
    (27, 2, 300, 4000), (29, 2, 300, 2000),
])
def test_commit_row_shard_matches_oracle(env, nv, rep, rows, begin):
    cabi, torch = env
    row_len, num_rows, cw = cabi.geometry(nv, rep)
    assert cw in (32768, 65536)
    z = orc.Zip(nv, rep=rep, geometry=(row_len, rows, cw), seeds=(nv, nv + 100))
    evals = _witness(nv * 7 + rep, rows, row_len)
    rows_o, layers_o, roots_o = z.commit(evals)
    ctx = cabi.ZipContext(nv, z.perm1, z.perm2, rep=rep, row_begin=begin, row_count=rows)
    d_evals = torch.from_numpy(evals).cuda()
    com, roots = ctx.commit(d_evals)
    assert np.array_equal(roots, roots_o)
    rows_a, layers_a, roots_a = com.download()
    assert np.array_equal(rows_a, rows_o)
    assert np.array_equal(layers_a, layers_o[:, : 2 * cw - 2])
    assert np.array_equal(roots_a, layers_o[:, 2 * cw - 2])
    com.free()
    enc, _ = ctx.commit(d_evals, with_merkle=False)  # encode_rows / commit_no_merkle: Int<4> rows
    rows_b, _, _ = enc.download()
    assert np.array_equal(rows_b, rows_o)
    enc.free()
    ctx.close()


def _squeeze_open_inputs(z, f, nv):
    fs = orc.new_transcript()
    coeffs = np.zeros(z.num_rows, dtype=np.int64)
    for r in range(z.num_rows):
        orc.lib().orc_tr_get_integer_challenge(orc.C.byref(fs), 1, coeffs[r:].ctypes.data_as(orc.C.POINTER(orc.C.c_uint64)))
    cols = np.array([orc.get_challenge(fs, f) % (1 << 32) % z.codeword_len for _ in range(1000)], dtype=np.uint32)
    point = orc.point_to_field(f, [1] * nv)
    lr = z.num_rows.bit_length() - 1
    return coeffs, cols, point, orc.build_eq_x_r(f, point[nv - lr:]), orc.build_eq_x_r(f, point[: nv - lr])


def _check_roots(z, evals, roots, sample):
    for r in sample:
        rc, enc = z.encode_row(evals[r * z.row_len:(r + 1) * z.row_len])
        assert rc == 0
        assert np.array_equal(roots[r], orc.merkle_tree(z.depth, enc)[-1]), r


def test_commit_open_2pow27_full_on_one_gpu(env, monkeypatch):
    """2^27 = 8192 rows x 16384, codeword 32768, depth 15 on ONE device: all 8192 roots and 64 whole opening blocks
    against the oracle's row-by-row pass, the exact proof length, and byte-identical proofs from the plain commit +
    open, zip_commit_open, the hinted commit (its hint is ignored above cw 16384), zip_open_stream and two jobs in
    flight; zip_verify accepts (and rejects one flipped bit), the oracle's verifier accepts, zip_mle_eval equals the
    oracle's, no gather ran into its wait timeout; zip_mctx with 2 and 4 shards on device 0 gives the same bytes."""
    cabi, torch = env
    nv = 27
    z = orc.Zip(nv)
    assert (z.row_len, z.num_rows, z.codeword_len, z.depth) == (16384, 8192, 32768, 15)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = orc.splitmix64(0x5A494E43 + 27, 1 << nv)
    coeffs, cols, point, q0, q1 = _squeeze_open_inputs(z, f, nv)
    pick = np.unique(np.concatenate([[0, 1, 2, 499, 500, 997, 998, 999], np.arange(7, 1000, 17)]))[:64]
    roots_o, blocks_o = z.commit_open_columns(evals, cols[pick])
    d_blocks = torch.from_numpy(blocks_o).cuda()
    del blocks_o
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    ulen = z.row_len * 64

    def check_blocks(proof_t, what):
        for k, i in enumerate(pick):
            o = ulen + int(i) * per_col
            assert torch.equal(proof_t[o:o + per_col], d_blocks[k]), (what, int(i), int(cols[i]))

    ctx = cabi.ZipContext(nv, z.perm1, z.perm2)
    ctx.set_speculation(False)
    d_evals = torch.from_numpy(evals).cuda()
    plen = ctx.proof_len(1000, 4)
    assert plen == z.proof_len(4) == 16384 * 64 + 1000 * 8192 * (32 + 8 + 32 * 15) + 16384 * 32

    # plain zip_commit + zip_open, profiled: no gather may have waited into its 0.25 s timeout (and been redone)
    ctx.set_profiling(True)
    com, roots = ctx.commit(d_evals)
    assert np.array_equal(roots, roots_o)  # all 8192
    proof = torch.full((plen,), 0x33, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    com.open(d_evals, coeffs, cols, q0, zf, out=proof)
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.set_profiling(False)
    launches, wait_ms = prof.get("wait_counter_kernel", (0, 0.0))
    assert wait_ms < 250.0, prof
    check_blocks(proof, "plain")

    def same(other, what):
        assert torch.equal(other, proof), what

    # zip_commit_open (one call), the hinted commit, the self-hinted plain commit
    one = torch.full_like(proof, 0x44)
    torch.cuda.synchronize()
    _, roots1, _ = ctx.commit_open(d_evals, coeffs, cols, q0, zf, out=one)
    ctx.synchronize()
    assert np.array_equal(roots1, roots_o)
    same(one, "commit_open")
    for how in ("hinted", "self_hinted"):
        one.fill_(0x55)
        torch.cuda.synchronize()
        ctx.set_speculation(how == "self_hinted")
        c3, r3 = ctx.commit(d_evals, hint_cols=cols if how == "hinted" else None)
        c3.open(d_evals, coeffs, cols, q0, zf, out=one)
        ctx.synchronize()
        c3.free()
        assert np.array_equal(r3, roots_o), how
        same(one, how)
    ctx.set_speculation(False)

    # zip_open_stream: every piece against the device proof at its offset (no host copy of the stream)
    at = [0]

    def sink(mv):
        n = len(mv)
        piece = torch.from_numpy(np.frombuffer(mv, dtype=np.uint8).copy()).cuda()
        ok = torch.equal(piece, proof[at[0]:at[0] + n])
        at[0] += n
        return not ok

    com.open_stream(d_evals, coeffs, cols, q0, zf, sink, chunk_bytes=256 << 20)
    assert at[0] == plen
    com.free()

    # two jobs in flight
    outs = [torch.full_like(proof, 0x66), one]
    one.fill_(0x77)
    torch.cuda.synchronize()
    jobs = [ctx.commit_open_begin(d_evals, coeffs, cols, q0, zf, o) for o in outs]
    for j in jobs:
        j.wait()
    ctx.synchronize()
    same(outs[0], "job 0")
    same(outs[1], "job 1")
    del outs, one

    # the verifiers and the MLE evaluation
    ev = z.mle_eval(f, evals, point)
    ev_limbs = np.array(orc.int_to_limbs(ev, 4), dtype=np.uint64)
    assert orc.limbs_to_int(ctx.mle_eval(d_evals, q0, q1, zf)) == ev
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, ev_limbs, zf)
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    proof_h = proof.cpu().numpy()  # a host copy of the stream, for the oracle's verifier
    assert z.verify(f, roots, point, ev, proof_h, check_merkle=False) == 0
    del proof_h
    proof[plen // 2] ^= 1
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, ev_limbs, zf)
    assert rep["verdict"] != cabi.VERIFY_ACCEPT
    proof[plen // 2] ^= 1
    ctx.close()
    del d_evals

    # zip_mctx: 2 and 4 shards on device 0, compared with the device proof in slabs (one host copy at a time).
    # (Repeated ordinals never take the RCCL path -- it needs distinct devices -- so ZIP_HIP_MCTX_FORCE_NO_RCCL repeats
    # the two-shard run under the knob; the roots travel as device copies either way.)
    slab = 256 << 20
    for shards, knob in ((2, None), (4, None), (2, "ZIP_HIP_MCTX_FORCE_NO_RCCL")):
        if knob:
            monkeypatch.setenv(knob, "1")
        m = cabi.ZipMultiContext(nv, z.perm1, z.perm2, [0] * shards)
        pm, rm = m.commit_open(evals, coeffs, cols, q0, zf)
        m.close()
        assert np.array_equal(rm, roots_o), (shards, knob)
        assert pm.size == plen, (shards, knob)
        for o in range(0, plen, slab):
            assert torch.equal(torch.from_numpy(pm[o:o + slab]).cuda(), proof[o:o + slab]), (shards, knob, o)
        del pm


def test_commit_2pow28_whole_on_one_gpu(env):
    """2^28 = 16384 rows x 16384, codeword 32768 (8 GiB of row entries, 32 GiB of trees, an 8.5 GB proof) on one
    device: sampled roots against the oracle, and zip_verify accepts the whole stream."""
    cabi, torch = env
    nv = 28
    z = orc.Zip(nv)
    assert (z.row_len, z.num_rows, z.codeword_len) == (16384, 16384, 32768)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = orc.splitmix64(0x5A494E43 + 28, 1 << nv)
    coeffs, cols, point, q0, q1 = _squeeze_open_inputs(z, f, nv)
    ctx = cabi.ZipContext(nv, z.perm1, z.perm2)
    d_evals = torch.from_numpy(evals).cuda()
    proof = torch.empty(ctx.proof_len(1000, 4), dtype=torch.uint8, device="cuda")
    _, roots, _ = ctx.commit_open(d_evals, coeffs, cols, q0, zf, out=proof)
    ctx.synchronize()
    _check_roots(z, evals, roots, [0, 1, 255, 256, 8191, 8192, 16383])
    ev_limbs = ctx.mle_eval(d_evals, q0, q1, zf)
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, np.asarray(ev_limbs, dtype=np.uint64), zf)
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    ctx.close()


def _mle_from_row(f, row, q1):
    """sum_c row[c] q1[c]: the MLE evaluation from the evaluation row (eq(point) = q0 (x) q1 over rows x columns)."""
    acc = 0
    for c in range(row.shape[0]):
        acc = orc.field_add(f, acc, orc.field_mul(f, orc.limbs_to_int(row[c]), orc.limbs_to_int(q1[c])))
    return acc


def test_commit_open_2pow29_full_on_one_gpu(env):
    """2^29 = 16384 rows x 32768, codeword 65536, depth 16 on ONE device (open_columns_kernel<64>: 2 depth + 1 > 32):
    all 16384 roots and 8 whole opening blocks against the oracle's row-by-row pass, the exact proof length, the
    evaluation row (zip_open_eval) and the proximity row (zip_open_testing) against the oracle's row combinations,
    zip_mle_eval, zip_verify accepting the proof and rejecting one flipped bit, and one zip_commit_open_begin job
    giving the same bytes."""
    cabi, torch = env
    nv = 29
    z = orc.Zip(nv)
    assert (z.row_len, z.num_rows, z.codeword_len, z.depth) == (32768, 16384, 65536, 16)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = orc.splitmix64(0x5A494E43 + 29, 1 << nv)
    coeffs, cols, _, _, _ = _squeeze_open_inputs(z, f, nv)
    point = orc.point_to_field(f, np.arange(2, nv + 2, dtype=np.int64))
    lr = z.num_rows.bit_length() - 1
    q0, q1 = orc.build_eq_x_r(f, point[nv - lr:]), orc.build_eq_x_r(f, point[: nv - lr])
    pick = np.array([0, 1, 123, 333, 500, 777, 998, 999])
    roots_o, blocks_o = z.commit_open_columns(evals, cols[pick])
    d_blocks = torch.from_numpy(blocks_o).cuda()
    del blocks_o
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)

    ctx = cabi.ZipContext(nv, z.perm1, z.perm2)
    ctx.set_speculation(False)
    d_evals = torch.from_numpy(evals).cuda()
    plen = ctx.proof_len(1000, 4)
    assert plen == z.proof_len(4) == 32768 * 64 + 1000 * 16384 * (32 + 8 + 32 * 16) + 32768 * 32
    com, roots = ctx.commit(d_evals)
    assert np.array_equal(roots, roots_o)  # all 16384
    proof = torch.full((plen,), 0x33, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    com.open(d_evals, coeffs, cols, q0, zf, out=proof)
    ctx.synchronize()
    com.free()
    for k, i in enumerate(pick):
        o = z.row_len * 64 + int(i) * per_col
        assert torch.equal(proof[o:o + per_col], d_blocks[k]), (int(i), int(cols[i]))
    del d_blocks

    # the row combinations at row_len 32768, and the MLE evaluation
    row_o = z.combine_rows_field(f, q0, evals)
    assert np.array_equal(ctx.open_eval(d_evals, q0, zf), row_o)
    rc, u_o = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    assert np.array_equal(ctx.open_testing(d_evals, coeffs), u_o)
    ev = _mle_from_row(f, row_o, q1)
    assert orc.limbs_to_int(ctx.mle_eval(d_evals, q0, q1, zf)) == ev
    ev_limbs = np.array(orc.int_to_limbs(ev, 4), dtype=np.uint64)
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, ev_limbs, zf)
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    proof[plen // 2] ^= 1
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, ev_limbs, zf)
    assert rep["verdict"] != cabi.VERIFY_ACCEPT
    proof[plen // 2] ^= 1

    # one job
    out = torch.full_like(proof, 0x66)
    torch.cuda.synchronize()
    roots_j = ctx.commit_open_begin(d_evals, coeffs, cols, q0, zf, out).wait(want_roots=True)
    ctx.synchronize()
    assert np.array_equal(roots_j, roots_o)
    assert torch.equal(out, proof)
    ctx.close()


def test_commit_open_job_2pow30_whole_on_one_gpu(env):
    """2^30 = 32768 rows x 32768, codeword 65536 (32 GiB of row entries, 128 GiB of trees, an 18 GB proof) as ONE
    zip_commit_open_begin job with the 4-limb field -- its small inputs (1.3 MB) exceed the 1 MiB a job's staging block
    held before -- sampled roots against the oracle, zip_verify accepting the whole stream, and every chunk's gather
    launched once (a wait that ran into its 0.25 s timeout would add a re-gather)."""
    cabi, torch = env
    nv = 30
    z = orc.Zip(nv)
    assert (z.row_len, z.num_rows, z.codeword_len) == (32768, 32768, 65536)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = orc.splitmix64(0x5A494E43 + 30, 1 << nv)
    coeffs, cols, point, q0, q1 = _squeeze_open_inputs(z, f, nv)
    ctx = cabi.ZipContext(nv, z.perm1, z.perm2)
    d_evals = torch.from_numpy(evals).cuda()
    proof = torch.empty(ctx.proof_len(1000, 4), dtype=torch.uint8, device="cuda")
    ctx.set_profiling(True)
    roots = ctx.commit_open_begin(d_evals, coeffs, cols, q0, zf, proof).wait(want_roots=True)
    ctx.synchronize()
    prof = ctx.profile_read()
    ctx.set_profiling(False)
    waits, gathers = prof["wait_counter_kernel"][0], prof["open_columns_kernel"][0]
    assert waits >= 2 and gathers == waits, prof
    _check_roots(z, evals, roots, [0, 1, 255, 256, 16383, 16384, 32767])
    ev_limbs = ctx.mle_eval(d_evals, q0, q1, zf)
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, np.asarray(ev_limbs, dtype=np.uint64), zf)
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    ctx.close()


def test_job_stages_the_inputs_of_many_rows(env):
    """A job's small inputs grow with the rows and the field limbs: 32768 rows (codeword 128, so that the test stays
    small) with a 4-limb field stage 1.3 MB of coefficients and q0.  The job's proof equals the plain commit + open's
    byte for byte and zip_verify accepts it; two jobs in flight (both staging blocks)."""
    cabi, torch = env
    nv, geo = 21, (64, 32768, 128)
    z = orc.Zip(nv, geometry=geo)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = orc.splitmix64(21, 1 << nv)
    _, _, roots_o = z.commit(evals)
    coeffs = orc.splitmix64(22, z.num_rows)
    cols = np.array([0, 5, 77, 127], dtype=np.uint32)
    point = orc.point_to_field(f, np.arange(2, nv + 2, dtype=np.int64))
    lr = z.num_rows.bit_length() - 1
    q0, q1 = orc.build_eq_x_r(f, point[nv - lr:]), orc.build_eq_x_r(f, point[: nv - lr])
    ctx = cabi.ZipContext(nv, z.perm1, z.perm2, geometry_override=geo)
    d_evals = torch.from_numpy(evals).cuda()
    plen = ctx.proof_len(cols.size, 4)
    ref = torch.full((plen,), 0x11, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    com, roots = ctx.commit(d_evals)
    assert np.array_equal(roots, roots_o)
    com.open(d_evals, coeffs, cols, q0, zf, out=ref)
    ctx.synchronize()
    com.free()
    ev_limbs = ctx.mle_eval(d_evals, q0, q1, zf)
    rep = ctx.verify(roots, ref, coeffs, cols, q0, q1, np.asarray(ev_limbs, dtype=np.uint64), zf)
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    outs = [torch.full_like(ref, 0x22), torch.full_like(ref, 0x44)]
    torch.cuda.synchronize()
    jobs = [ctx.commit_open_begin(d_evals, coeffs, cols, q0, zf, o) for o in outs]
    for j in jobs:
        assert np.array_equal(j.wait(want_roots=True), roots_o)
    ctx.synchronize()
    for o in outs:
        assert torch.equal(o, ref)
    ctx.close()
