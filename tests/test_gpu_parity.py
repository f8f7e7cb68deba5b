"""GPU parity: the HIP path, called through the C ABI, against the CPU oracle on
identical inputs -- bit-exact (integer / byte work).  Needs a real MI355X."""
import numpy as np
import pytest

import _oracle as orc
from _openings import _expected_openings

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189  # benches/spartan_benches.rs:134-137
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59  # not necessarily prime; arithmetic is ring arithmetic either way


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _ctx(cabi, z, **kw):
    return cabi.ZipContext(z.num_vars, z.perm1, z.perm2, geometry_override=(z.row_len, z.num_rows, z.codeword_len), **kw)


def _witness(num_vars, seed=0, small=False):
    n = 1 << num_vars
    if small:
        return np.random.default_rng(seed).integers(-128, 128, size=n, dtype=np.int64)
    w = orc.splitmix64(0x5A494E43 + seed, n).copy()
    # force the extremes in (sign handling, carries)
    w[: min(n, 4)] = np.array([-(2**63), 2**63 - 1, -1, 0], dtype=np.int64)[: min(n, 4)]
    return w


# every kernel variant: E=1 (cw<=64), E=2 (128), E=4 (256), E=8 (>=512); odd num_vars; single row
@pytest.mark.parametrize("num_vars", [0, 1, 2, 3, 5, 6, 9, 10, 12, 13, 14, 16, 18])
def test_commit_bit_exact(cabi, num_vars):
    z = orc.Zip(num_vars)
    evals = _witness(num_vars)
    rows_o, layers_o, roots_o = z.commit(evals)
    ctx = _ctx(cabi, z)
    com, roots = ctx.commit(evals)
    rows, layers, roots_d = com.download()
    assert np.array_equal(rows, rows_o)
    assert np.array_equal(roots, roots_o) and np.array_equal(roots_d, roots_o)
    assert np.array_equal(layers, layers_o[:, :-1, :])  # reference layers have the root popped
    # commit_no_merkle / encode_rows (commit.rs:104-119)
    com2, r2 = ctx.commit(evals, with_merkle=False)
    assert r2 is None
    assert np.array_equal(com2.download()[0], rows_o)
    # deterministic (commit.rs:253-283)
    com3, roots3 = ctx.commit(evals)
    assert np.array_equal(roots3, roots_o)


def test_commit_2pow20_bit_exact(cabi):
    """BASELINE config 2: commit at 2^20 coefficients, every byte against the oracle."""
    z = orc.Zip(20)
    evals = _witness(20)
    rows_o, layers_o, roots_o = z.commit(evals)
    ctx = _ctx(cabi, z)
    com, roots = ctx.commit(evals)
    rows, layers, _ = com.download()
    assert np.array_equal(roots, roots_o)
    assert np.array_equal(rows, rows_o)
    assert np.array_equal(layers, layers_o[:, :-1, :])


def test_commit_device_resident_input(cabi):
    torch = pytest.importorskip("torch")
    z = orc.Zip(12)
    evals = _witness(12)
    ctx = _ctx(cabi, z)
    d = torch.from_numpy(evals).cuda()
    com, roots = ctx.commit(d)
    assert np.array_equal(roots, z.commit(evals)[2])


def test_commit_large_codeword_global_t2_path(cabi):
    """cw = 16384 (the 2^26 geometry): raa_commit16_kernel -- t2 compacted into LDS, the output through an 8x8
    transpose inside every 8-lane group, its second half parked in the dead t2 planes."""
    z = orc.Zip(16, geometry=(8192, 8, 16384))
    evals = _witness(16)
    rows_o, layers_o, roots_o = z.commit(evals)
    ctx = _ctx(cabi, z)
    com, roots = ctx.commit(evals)
    rows, layers, _ = com.download()
    assert np.array_equal(rows, rows_o)
    assert np.array_equal(layers, layers_o[:, :-1, :])
    assert np.array_equal(roots, roots_o)


def test_commit_shape_and_param_errors(cabi):
    z = orc.Zip(8)
    ctx = _ctx(cabi, z)
    with pytest.raises(cabi.ZipError) as e:  # commit.rs:56-63 panics; the ABI reports ZIP_ERR_SHAPE
        ctx.commit(np.zeros(100, dtype=np.int64))
    assert e.value.code == cabi.ZIP_ERR_SHAPE
    bad = z.perm1.copy()
    bad[0] = bad[1]
    with pytest.raises(cabi.ZipError) as e:
        cabi.ZipContext(8, bad, z.perm2)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError) as e:  # K must be Int<4N>
        cabi.ZipContext(8, z.perm1, z.perm2, k_limbs=2)
    assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED


@pytest.mark.parametrize("num_vars", [2, 3, 8, 9, 12, 16])
def test_open_testing_bit_exact(cabi, num_vars):
    z = orc.Zip(num_vars)
    evals = _witness(num_vars)
    coeffs = orc.splitmix64(77, z.num_rows).copy()
    coeffs[:2] = [-(2**63), 2**63 - 1][: min(2, z.num_rows)]
    rc, expect = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    ctx = _ctx(cabi, z)
    got = ctx.open_testing(evals, coeffs)
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2), (MOD_NO_SPARE, 4), (MOD_3LIMB, 3)])
@pytest.mark.parametrize("num_vars", [3, 8, 9, 14])
def test_open_eval_bit_exact(cabi, num_vars, modulus, fl):
    z = orc.Zip(num_vars)
    f = orc.make_field(modulus, fl)
    evals = _witness(num_vars)
    rng = np.random.default_rng(num_vars)
    q0_vals = [int.from_bytes(rng.bytes(8 * fl), "little") % modulus for _ in range(z.num_rows)]
    q0_vals[0] = modulus - 1
    q0 = orc.field_elems(q0_vals, fl)
    expect = z.combine_rows_field(f, q0, evals)
    ctx = _ctx(cabi, z)
    got = ctx.open_eval(evals, q0, cabi.make_field(modulus, fl))
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("num_vars", [16, 20, 22])
@pytest.mark.parametrize("signs", ["same", "opposite", "mixed"])
def test_row_combinations_at_their_accumulator_bounds(cabi, num_vars, signs):
    """Every product of the proximity row at its extreme (|coeff * w| = 2^126, zip/utils.rs:94-127 over Int<8>), summed
    over up to 2048 rows with one sign -- the 192-bit accumulators of combine_rows_kernel and the fold of the partial
    sums must carry it -- and every q_0 entry at q - 1 beside witnesses of -2^63 / 2^63 - 1 for the evaluation row (no
    spare bit in the modulus: the carry branch of the reduction, field/config.rs:68-76)."""
    z = orc.Zip(num_vars)
    n, R = 1 << num_vars, z.num_rows
    lo, hi = -(2**63), 2**63 - 1
    if signs == "same":
        evals, coeffs = np.full(n, lo, dtype=np.int64), np.full(R, lo, dtype=np.int64)
    elif signs == "opposite":
        evals, coeffs = np.full(n, hi, dtype=np.int64), np.full(R, lo, dtype=np.int64)
    else:
        evals = np.where(np.arange(n) % 3 == 0, lo, hi).astype(np.int64)
        coeffs = np.where(np.arange(R) % 5 < 2, lo, hi).astype(np.int64)
    rc, expect = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    ctx = _ctx(cabi, z)
    assert np.array_equal(ctx.open_testing(evals, coeffs), expect)
    for modulus in (MOD_NO_SPARE, BENCH_MODULUS):
        f = orc.make_field(modulus, 4)
        q0 = orc.field_elems([modulus - 1 - (i % 2) for i in range(R)], 4)
        assert np.array_equal(ctx.open_eval(evals, q0, cabi.make_field(modulus, 4)), z.combine_rows_field(f, q0, evals))


def test_open_eval_single_row_is_map_to_field(cabi):
    z = orc.Zip(0)
    f = orc.make_field(BENCH_MODULUS, 4)
    ctx = _ctx(cabi, z)
    for w in (-5, 0, 2**63 - 1, -(2**63)):
        got = ctx.open_eval(np.array([w], dtype=np.int64), None, cabi.make_field(BENCH_MODULUS, 4))
        assert orc.limbs_to_int(got[0]) == orc.field_from_i64(f, w)


@pytest.mark.parametrize("num_vars", [3, 8, 12, 16])
def test_open_columns_wire_format(cabi, num_vars):
    z = orc.Zip(num_vars)
    evals = _witness(num_vars)
    rows_o, layers_o, roots_o = z.commit(evals)
    ctx = _ctx(cabi, z)
    com, _ = ctx.commit(evals)
    rng = np.random.default_rng(1)
    cols = rng.integers(0, z.codeword_len, size=37, dtype=np.uint32)
    cols[:3] = [0, z.codeword_len - 1, cols[3]]  # edges + a duplicate
    wire = com.open_columns(cols)
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    assert wire.size == cols.size * per_col
    rows3 = rows_o.reshape(z.num_rows, z.codeword_len, 4)
    for i, c in enumerate(cols):
        blk = wire[i * per_col:(i + 1) * per_col]
        assert blk[: z.num_rows * 32].tobytes() == rows3[:, c, :].astype("<u8").tobytes()
        rec = blk[z.num_rows * 32:].reshape(z.num_rows, 8 + 32 * z.depth)
        for r in range(z.num_rows):
            assert int.from_bytes(rec[r, :8].tobytes(), "big") == z.depth
            assert rec[r, 8:].tobytes() == orc.merkle_path(z.depth, layers_o[r], int(c)).tobytes()


@pytest.mark.parametrize("num_vars,modulus,fl", [(8, BENCH_MODULUS, 4), (8, TEST_MODULUS_2, 2), (9, BENCH_MODULUS, 4),
                                                 (3, TEST_MODULUS_2, 2), (0, BENCH_MODULUS, 4), (14, BENCH_MODULUS, 4),
                                                 (10, MOD_NO_SPARE, 4)])
def test_full_open_proof_equals_oracle_and_verifies(cabi, num_vars, modulus, fl):
    """The proof bytes of MultilinearZip::open on identical transcripts, then the
    oracle's verifier (src/zip/pcs/verify_z.rs) accepts the GPU proof."""
    z = orc.Zip(num_vars)
    f = orc.make_field(modulus, fl)
    evals = _witness(num_vars, small=(fl == 2))
    rng = np.random.default_rng(3)
    point_i = rng.integers(-100, 100, size=num_vars, dtype=np.int64)
    point = orc.point_to_field(f, point_i) if num_vars else np.zeros((0, fl), dtype=np.uint64)
    rows_o, layers_o, roots_o = z.commit(evals)
    fs = orc.new_transcript()
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, fs)

    ctx = _ctx(cabi, z)
    com, roots = ctx.commit(evals)
    assert np.array_equal(roots, roots_o)
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:]) if lr else None
    proof = com.open(evals, coeffs if z.num_rows > 1 else None, cols, q0, cabi.make_field(modulus, fl))
    assert proof.size == proof_o.size == z.proof_len(fl)
    assert np.array_equal(proof, proof_o)
    # row_len == 1 leaves q_1 empty: the reference's own verifier cannot accept (verify_z.rs:146-151); nor does it accept
    # its own proofs for a modulus with the top bit set -- that case is here for the BYTES: both row
    # combinations in one pass, the field half seeing |w| mod (2^256 - q), the integer half the entry as it is
    if num_vars > 0 and modulus != MOD_NO_SPARE:
        ev = z.mle_eval(f, evals, point)
        assert z.verify(f, roots, point, ev, proof) == 0


def test_open_from_uploaded_and_mutated_commitment(cabi):
    """The reference's tests mutate MultilinearZipData before opening (open_z.rs:230-241)."""
    z = orc.Zip(8)
    evals = _witness(8)
    rows_o, layers_o, roots_o = z.commit(evals)
    rows_m = rows_o.copy()
    rows_m[5, 0] ^= np.uint64(1)
    ctx = _ctx(cabi, z)
    com = ctx.upload_commitment(rows_m, layers_o[:, :-1, :], roots_o)
    cols = np.array([5, 6], dtype=np.uint32)
    wire = com.open_columns(cols)
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    assert wire[:32].tobytes() == rows_m[5].astype("<u8").tobytes()
    assert wire[per_col:per_col + 32].tobytes() == rows_o[6].astype("<u8").tobytes()
    r, l, t = com.download()
    assert np.array_equal(r, rows_m) and np.array_equal(l, layers_o[:, :-1, :]) and np.array_equal(t, roots_o)


def test_row_sharded_commit_and_open_match_unsharded(cabi):
    """rows shard across GPUs; partial row combinations add exactly."""
    torch = pytest.importorskip("torch")
    nv, G = 10, 4
    z = orc.Zip(nv)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv)
    rows_o, layers_o, roots_o = z.commit(evals)
    coeffs = orc.splitmix64(5, z.num_rows)
    q0 = orc.field_elems([int(x) * 0xDEADBEEFCAFEBABE1234567 % BENCH_MODULUS for x in orc.splitmix64(6, z.num_rows).view(np.uint64)], 4)
    _, u_full = z.combine_rows_int(coeffs, evals)
    row_full = z.combine_rows_field(f, q0, evals)
    per = z.num_rows // G
    uparts = torch.zeros((G, z.row_len, 8), dtype=torch.int64, device="cuda")
    fparts = torch.zeros((G, z.row_len, 4), dtype=torch.int64, device="cuda")
    cols = np.array([1, 7, 63], dtype=np.uint32)
    ctxs = []
    for g in range(G):
        ctx = cabi.ZipContext(nv, z.perm1, z.perm2, row_begin=g * per, row_count=per)
        ctxs.append(ctx)
        sl = slice(g * per * z.row_len, (g + 1) * per * z.row_len)
        com, roots = ctx.commit(evals[sl])
        assert np.array_equal(roots, roots_o[g * per:(g + 1) * per])
        ctx.open_testing(evals[sl], coeffs[g * per:(g + 1) * per], out=uparts[g])
        ctx.open_eval(evals[sl], q0[g * per:(g + 1) * per], zf, out=fparts[g])
        wire = com.open_columns(cols)
        rows3 = rows_o.reshape(z.num_rows, z.codeword_len, 4)[g * per:(g + 1) * per]
        assert wire[: per * 32].tobytes() == rows3[:, 1, :].astype("<u8").tobytes()
        ctx.synchronize()
    torch.cuda.synchronize()
    u_out = torch.zeros((z.row_len, 8), dtype=torch.int64, device="cuda")
    r_out = torch.zeros((z.row_len, 4), dtype=torch.int64, device="cuda")
    ctxs[0].sum_partials(uparts, fparts, G, zf, u_out, r_out)
    ctxs[0].synchronize()
    assert np.array_equal(u_out.cpu().numpy().view(np.uint64), u_full)
    assert np.array_equal(r_out.cpu().numpy().view(np.uint64), row_full)


def test_standalone_merkle_trees(cabi):
    """MerkleTree::new on random full-width leaves (benches/zip_benches.rs:80-98; pcs/utils.rs:340 uses Int<3>)."""
    rng = np.random.default_rng(8)
    for limbs, depth in ((4, 10), (3, 6), (1, 0), (8, 4)):
        leaves = rng.integers(0, 2**64, size=(3, 1 << depth, limbs), dtype=np.uint64)
        got = cabi.merkle_trees(leaves, depth)
        for t in range(3):
            assert np.array_equal(got[t], orc.merkle_tree(depth, leaves[t]))


def test_profiling_hooks_report_kernels(cabi):
    z = orc.Zip(10)
    ctx = _ctx(cabi, z)
    ctx.set_profiling(True)
    ctx.commit(_witness(10))
    times = ctx.profile_read()
    assert "raa_commit_kernel" in times and times["raa_commit_kernel"][0] == 1
    assert times["raa_commit_kernel"][1] > 0


@pytest.mark.parametrize("num_vars,chunk", [(0, 0), (3, 1), (8, 4096), (12, 1 << 16), (14, 0)])
def test_open_stream_pieces_concatenate_to_the_proof(cabi, num_vars, chunk):
    """zip_open_stream: u', column groups, evaluation row, in order, byte-identical
    to the contiguous proof of zip_open -- whatever the group size."""
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    evals = _witness(num_vars, seed=9)
    point = orc.point_to_field(f, np.arange(num_vars, dtype=np.int64) - 3) if num_vars else np.zeros((0, 4), dtype=np.uint64)
    rows_o, layers_o, _ = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:]) if lr else None
    cf = coeffs if z.num_rows > 1 else None
    ctx = _ctx(cabi, z)
    com, _ = ctx.commit(evals)
    pieces = []
    com.open_stream(evals, cf, cols, q0, cabi.make_field(BENCH_MODULUS, 4), lambda mv: pieces.append(bytes(mv)) and None,
                    chunk_bytes=chunk)
    assert b"".join(pieces) == proof_o.tobytes()
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    assert all(len(p) % per_col == 0 for p in pieces[(1 if z.num_rows > 1 else 0):-1])  # whole columns per piece
    if chunk == 1:
        assert len(pieces) == (1 if z.num_rows > 1 else 0) + len(cols) + 1
    # a sink that refuses the stream aborts the call
    seen = []
    with pytest.raises(cabi.ZipError):
        com.open_stream(evals, cf, cols, q0, cabi.make_field(BENCH_MODULUS, 4),
                        lambda mv: seen.append(len(mv)) or len(seen) >= 2, chunk_bytes=chunk)
    assert len(seen) == 2
    # the handle is still usable afterwards
    assert com.open(evals, cf, cols, q0, cabi.make_field(BENCH_MODULUS, 4)).tobytes() == proof_o.tobytes()


@pytest.mark.parametrize("how", ["hinted", "commit_open"])
def test_open_stream_on_a_packed_handle(cabi, how):
    """A packed hinted handle (zip_commit_hinted / zip_commit_open(out=&h), the default from codeword 512 up) opened
    through zip_open_stream in SEVERAL column groups: group g > 0 must use the ranks of ITS openings (round-2 advisor
    finding: every group read the ranks of group 0)."""
    num_vars = 16  # 256 x 256, cw = 512: the smallest geometry with packed openings
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(num_vars, seed=21)
    point = orc.point_to_field(f, np.arange(num_vars, dtype=np.int64) + 2)
    rows_o, layers_o, _ = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    ctx = _ctx(cabi, z)
    if how == "hinted":
        com, _ = ctx.commit(evals, hint_cols=cols)
    else:
        proof1, _, com = ctx.commit_open(evals, coeffs, cols, q0, zf, keep=True)
        assert np.asarray(proof1).tobytes() == proof_o.tobytes()
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    for chunk in (7 * per_col, per_col, 0):  # 143 groups of 7 columns; one column per group; one group
        pieces = []
        com.open_stream(evals, coeffs, cols, q0, zf, lambda mv: pieces.append(bytes(mv)) and None, chunk_bytes=chunk)
        assert b"".join(pieces) == proof_o.tobytes(), chunk
    com.free()


def test_pipelined_gather_recovers_from_a_timed_out_wait(cabi, monkeypatch):
    """The gather of a chunk is gated on a counter of the still running commit kernel; when that wait
    gives up (kernel dispatch serialised by a profiler, say) the gather is redone after the commit."""
    torch = pytest.importorskip("torch")
    nv = 22  # 2048 rows in 4 rounds of 512 workgroups
    z = orc.Zip(nv)
    evals = _witness(nv, seed=4)
    cols = np.array([0, 5, 4095, 1024, 77], dtype=np.uint32)
    monkeypatch.setenv("ZIP_HIP_CHUNKS", "4")  # one chunk per round: the open below is pipelined
    ctx = _ctx(cabi, z)
    d = torch.from_numpy(evals).cuda()
    want = ctx.commit(d)[0].open_columns(cols)
    monkeypatch.setenv("ZIP_HIP_FORCE_WAIT_TIMEOUT", "1")
    com, _ = ctx.commit(d)
    got = com.open_columns(cols)  # enqueued right behind the commit: the waits give up after 1 ms
    monkeypatch.delenv("ZIP_HIP_FORCE_WAIT_TIMEOUT")
    assert np.array_equal(got, want)
    # and both equal the oracle on sampled rows of a column
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    vals = got[per_col:per_col + z.num_rows * 32].reshape(z.num_rows, 32)
    for r in (0, 511, 512, 2047):
        rc, enc = z.encode_row(evals[r * z.row_len:(r + 1) * z.row_len])
        assert rc == 0 and vals[r].tobytes() == enc[5].astype("<u8").tobytes(), r


def test_open_and_verify_on_the_2pow26_geometry(cabi):
    """cw = 16384, depth 14 (raa_commit16_kernel's trees): the whole proof against the oracle, then the
    device verifier, on a 16-row slice of the geometry."""
    z = orc.Zip(17, geometry=(8192, 16, 16384))
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(17, seed=12)
    point = orc.point_to_field(f, np.arange(3, 20, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    ctx = _ctx(cabi, z)
    com, roots = ctx.commit(evals)
    assert np.array_equal(roots, roots_o)
    lr = 4  # log2(16 rows)
    q0 = orc.build_eq_x_r(f, point[17 - lr:])
    q1 = orc.build_eq_x_r(f, point[: 17 - lr])
    proof = com.open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(proof, proof_o)
    ev = z.mle_eval(f, evals, point)
    assert z.verify(f, roots, point, ev, proof) == 0
    rep = ctx.verify(roots, proof, coeffs, cols, q0, q1, np.array(orc.int_to_limbs(ev, 4), dtype=np.uint64), zf)
    assert rep["verdict"] == cabi.VERIFY_ACCEPT and rep["bad_merkle_paths"] == 0


@pytest.mark.parametrize("geometry", [(16, None), (17, None), (20, None), (17, (8192, 16, 16384)), (12, None)])
def test_hinted_commit_opens_bit_exact_and_completes_itself(cabi, geometry):
    """zip_commit_hinted: the commit kernel skips every store the hinted openings cannot read (the columns are known
    before the commit in the prover flow, src/zinc/prover.rs:316).  Roots and the proof of the hinted columns are the
    oracle's byte for byte; asking for anything else (other columns, a download) completes the handle first and is
    again the oracle's.  (2^12: codeword 128 < 512, the hint is ignored.)"""
    nv, geo = geometry
    z = orc.Zip(nv, geometry=geo) if geo else orc.Zip(nv)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv, seed=21)
    point = orc.point_to_field(f, np.arange(-4, nv - 4, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[nv - lr:])
    ctx = _ctx(cabi, z)
    # a poisoned pool: stale bytes of an earlier commit must never reach the proof
    junk, _ = ctx.commit(_witness(nv, seed=99))
    ctx.synchronize()
    junk.free()
    com, roots = ctx.commit(evals, hint_cols=cols)
    assert np.array_equal(roots, roots_o)
    proof = com.open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(proof, proof_o)
    # different columns: not covered by the hint
    other = ((cols.astype(np.int64) * 7 + 3) % z.codeword_len).astype(np.uint32)
    wire = com.open_columns(other)
    per_col = z.num_rows * (32 + 8 + 32 * z.depth)
    for i in (0, 1, len(other) // 2, len(other) - 1):
        c = int(other[i])
        got = wire[i * per_col:(i + 1) * per_col]
        vals = got[: z.num_rows * 32].reshape(z.num_rows, 32)
        rec = got[z.num_rows * 32:].reshape(z.num_rows, 8 + 32 * z.depth)
        for r in (0, z.num_rows - 1):
            assert vals[r].tobytes() == rows_o[r * z.codeword_len + c].astype("<u8").tobytes()
            assert rec[r, 8:].tobytes() == orc.merkle_path(z.depth, layers_o[r], c).tobytes()
    rows, layers, roots2 = com.download()
    assert np.array_equal(rows, rows_o) and np.array_equal(roots2, roots_o)
    assert np.array_equal(layers, layers_o[:, : 2 * z.codeword_len - 2])
    com.free()
    # a hinted handle that is downloaded straight away
    com, _ = ctx.commit(evals, hint_cols=cols[:3])
    rows, layers, _ = com.download()
    assert np.array_equal(rows, rows_o) and np.array_equal(layers, layers_o[:, : 2 * z.codeword_len - 2])


@pytest.mark.parametrize("geometry", [(16, None), (17, None), (18, None), (20, None), (17, (8192, 16, 16384)), (12, None), (9, None)])
@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("packed", ["1", "0"])
def test_commit_open_in_one_call_is_byte_identical(cabi, geometry, device_out, packed, monkeypatch):
    """zip_commit_open (the binding for commit_z_mle_and_prove_evaluation, prover.rs:305-328).  Default: what the
    openings read of the row entries and of tree levels 0..2 is stored packed and gathered from there (codeword >= 512,
    both commit kernels; the repeated columns of codeword 512, neighbours that are each other's sibling, nodes that
    serve four columns all go through the rank tables).  ZIP_HIP_PACKED=0: the same stores at their natural places.
    Roots and every proof byte equal the oracle's; the output buffer is poisoned first, so a byte nobody wrote shows."""
    monkeypatch.setenv("ZIP_HIP_PACKED", packed)
    nv, geo = geometry
    z = orc.Zip(nv, geometry=geo) if geo else orc.Zip(nv)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv, seed=31)
    point = orc.point_to_field(f, np.arange(-7, nv - 7, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[nv - lr:])
    ctx = _ctx(cabi, z)
    if device_out:
        torch = pytest.importorskip("torch")
        out = torch.full((proof_o.size,), 0xAA, dtype=torch.uint8, device="cuda")
        d_evals = torch.from_numpy(evals).cuda()
        torch.cuda.synchronize()  # the fill runs on torch's stream, the library on its own
        proof, roots, com = ctx.commit_open(d_evals, coeffs, cols, q0, zf, out=out, keep=True)
        ctx.synchronize()
        got = proof.cpu().numpy()
    else:
        proof, roots, com = ctx.commit_open(evals, coeffs, cols, q0, zf, keep=True)
        got = proof
    assert np.array_equal(roots, roots_o)
    bad = np.flatnonzero(got != proof_o)
    assert bad.size == 0, f"{bad.size} proof bytes differ, first at {bad[:8]}"
    # the handle completes itself when asked for what went into the proof instead of into rows / layers
    rows, layers, roots2 = com.download()
    assert np.array_equal(rows, rows_o) and np.array_equal(roots2, roots_o)
    assert np.array_equal(layers, layers_o[:, : 2 * z.codeword_len - 2])
    again = com.open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(again, proof_o)
    com.free()
    # without keeping the handle
    proof2, _, none = ctx.commit_open(evals, coeffs, cols, q0, zf, want_roots=False)
    assert none is None and np.array_equal(proof2, proof_o)


@pytest.mark.parametrize("num_vars", [12, 18])
def test_prepared_one_call_writes_the_same_proof_every_time(cabi, num_vars):
    """cabi.commit_open_prepared: the zip_commit_open call with its arguments marshalled once (what bench.py's step is).
    Called three times into a poisoned device buffer, with the witness replaced IN PLACE before the third call: the
    oracle's proof bytes every time."""
    torch = pytest.importorskip("torch")
    nv = num_vars
    z = orc.Zip(nv)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    point = orc.point_to_field(f, np.arange(-7, nv - 7, dtype=np.int64))
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[nv - lr:])
    ctx = _ctx(cabi, z)
    want = []
    for seed in (31, 32):
        evals = _witness(nv, seed=seed)
        rows_o, layers_o, _ = z.commit(evals)
        proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
        want.append((evals, proof_o, cols, coeffs))
    assert np.array_equal(want[0][2], want[1][2]) and np.array_equal(want[0][3], want[1][3])  # (transcript-only inputs)
    d_evals = torch.from_numpy(want[0][0].copy()).cuda()
    out = torch.full((want[0][1].size,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call = ctx.commit_open_prepared(d_evals, want[0][3], want[0][2], q0, zf, out)
    for k in range(3):
        if k == 2:
            d_evals.copy_(torch.from_numpy(want[1][0]))
        out.fill_(0xAA)
        torch.cuda.synchronize()
        call()
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[1 if k == 2 else 0][1]), k


@pytest.mark.parametrize("num_vars", [16, 18, 20])
@pytest.mark.parametrize("classes", ["1", "2", "4"])
def test_single_round_commit_in_priority_classes(cabi, num_vars, classes, monkeypatch):
    """A commit of ONE round whose workgroups share their CUs (2^16: 8 per CU, 2^18: 8, 2^20: 4) is published in classes
    of workgroups at different wave priorities (CommitArgs.classes; ZIP_HIP_CLASSES = 1: off, 2, 4), each class a chunk
    of consecutive rows gathered on its own.  Same roots, same proof bytes as the oracle, device witness, poisoned output."""
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("ZIP_HIP_CLASSES", classes)
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(num_vars, seed=131)
    point = orc.point_to_field(f, np.arange(2, num_vars + 2, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    ctx = _ctx(cabi, z)
    d = torch.from_numpy(evals).cuda()
    for _ in range(2):
        out = torch.full((proof_o.size,), 0x5C, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _, roots, com = ctx.commit_open(d, coeffs, cols, q0, zf, out=out, keep=True)
        ctx.synchronize()
        assert np.array_equal(roots, roots_o)
        bad = np.flatnonzero(out.cpu().numpy() != proof_o)
        assert bad.size == 0, f"{bad.size} proof bytes differ, first at {bad[:8]}"
        rows, _, _ = com.download()  # the handle completes itself (full re-run with the same row mapping)
        assert np.array_equal(rows, rows_o)
        com.free()


@pytest.mark.parametrize("geometry", [(16, None), (20, None), (17, (8192, 16, 16384))])
@pytest.mark.parametrize("pattern", ["min", "max", "alternating", "runs"])
def test_commit_extreme_witnesses(cabi, geometry, pattern):
    """The widest prefix sums the lanes can meet (code_raa.rs:53-72 sizes K for exactly these): every coefficient
    -2^63, every coefficient 2^63 - 1, alternating signs, long runs of each.  The 16-entry kernel keeps the
    intermediate codeword as 64 low bits + a one-byte difference of the high word to its thread's prefix
    (kernels_commit.cuh): these inputs are where that difference is largest.  Rows, every tree layer and the roots
    equal the oracle's."""
    nv, geo = geometry
    z = orc.Zip(nv, geometry=geo) if geo else orc.Zip(nv)
    n = 1 << nv
    lo, hi = -(2**63), 2**63 - 1
    if pattern == "min":
        evals = np.full(n, lo, dtype=np.int64)
    elif pattern == "max":
        evals = np.full(n, hi, dtype=np.int64)
    elif pattern == "alternating":
        evals = np.where(np.arange(n) & 1, lo, hi).astype(np.int64)
    else:
        evals = np.where((np.arange(n) // 97) & 1, lo, hi).astype(np.int64)
    rows_o, layers_o, roots_o = z.commit(evals)
    ctx = _ctx(cabi, z)
    com, roots = ctx.commit(evals)
    rows, layers, _ = com.download()
    com.free()
    assert np.array_equal(roots, roots_o)
    assert np.array_equal(rows, rows_o)
    assert np.array_equal(layers, layers_o[:, : 2 * z.codeword_len - 2])


_COLUMN_LISTS = {
    "one": lambda cw: [0],
    "last": lambda cw: [cw - 1],
    "same-40": lambda cw: [5] * 40,
    "siblings": lambda cw: [6, 7, 7, 6],
    "quad": lambda cw: [8, 9, 10, 11, cw - 4, cw - 3, cw - 2, cw - 1],
    "every-column": lambda cw: list(range(cw)),
    "descending-even": lambda cw: list(range(cw - 2, -1, -2))[:700],
    "low-half-twice": lambda cw: (list(range(0, cw // 2, 3)) * 2)[:900],
    "one-wave": lambda cw: list(range(64, 128)),
}


@pytest.mark.parametrize("geometry", [(16, None), (18, None), (17, (8192, 16, 16384))])
@pytest.mark.parametrize("which", sorted(_COLUMN_LISTS))
def test_hinted_and_packed_openings_for_hand_made_column_lists(cabi, geometry, which):
    """The rank tables of the packed openings and the hint bitmaps under column lists a transcript never squeezes: a
    single opening, one column forty times, sibling pairs, aligned groups of four (a level-2 node that serves four
    openings), EVERY column (all bits set: nothing may be skipped), only one wave's columns (every other wave stores
    nothing), more openings than distinct columns.  Both commit kernels (8 and 16 entries per lane).  The column section
    equals the oracle's rows and trees byte for byte, the whole proof equals the plain commit + open of the same ctx."""
    nv, geo = geometry
    z = orc.Zip(nv, geometry=geo) if geo else orc.Zip(nv)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    f = orc.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv, seed=77)
    rows_o, layers_o, roots_o = z.commit(evals)
    cols = np.array(_COLUMN_LISTS[which](z.codeword_len), dtype=np.uint32)
    coeffs = orc.splitmix64(5, z.num_rows).copy()
    point = orc.point_to_field(f, np.arange(3, nv + 3, dtype=np.int64))
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[nv - lr:])
    ctx = _ctx(cabi, z)
    ctx.set_speculation(False)
    plain, roots_p = ctx.commit(evals)
    ref = plain.open(evals, coeffs, cols, q0, zf)
    plain.free()
    assert np.array_equal(roots_p, roots_o)
    expect = _expected_openings(z, rows_o, layers_o, cols)
    u_bytes = z.row_len * 64
    assert np.array_equal(ref[u_bytes: u_bytes + expect.size], expect)
    proof, roots, _ = ctx.commit_open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(roots, roots_o)
    bad = np.flatnonzero(proof != ref)
    assert bad.size == 0, f"{which}: {bad.size} proof bytes differ, first at {bad[:8]}"
    com, _ = ctx.commit(evals, hint_cols=cols)
    again = com.open(evals, coeffs, cols, q0, zf)
    com.free()
    assert np.array_equal(again, ref)


@pytest.mark.parametrize("num_vars", [12, 18, 22])
def test_jobs_in_flight_produce_the_same_proofs(cabi, num_vars):
    """zip_commit_open_begin / zip_job_wait: four different polynomials, two jobs in flight at any time (the second
    commit kernel queued behind the first, beside the first one's last openings).  Every proof and every root equals
    what the one-call zip_commit_open gives for that polynomial (itself diffed against the oracle above); a third
    begin while two jobs are in flight is refused; 2^22 has two chunks, so the overlap is the real one."""
    torch = pytest.importorskip("torch")
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    point = orc.point_to_field(f, np.arange(-7, num_vars - 7, dtype=np.int64))
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    rng = np.random.default_rng(5)
    coeffs = rng.integers(-(1 << 62), 1 << 62, size=z.num_rows, dtype=np.int64)
    cols = rng.integers(0, z.codeword_len, size=1000, dtype=np.uint32)
    ctx = _ctx(cabi, z)
    witnesses = [torch.from_numpy(_witness(num_vars, seed=40 + i)).cuda() for i in range(4)]
    want = []
    for w in witnesses:
        proof, roots, _ = ctx.commit_open(w, coeffs, cols, q0, zf)
        want.append((proof.copy() if isinstance(proof, np.ndarray) else proof.cpu().numpy(), roots))
    outs = [torch.full((want[0][0].size,), 0xA5, dtype=torch.uint8, device="cuda") for _ in witnesses]
    torch.cuda.synchronize()  # the fills run on torch's stream, the library on its own
    jobs = [ctx.commit_open_begin(witnesses[0], coeffs, cols, q0, zf, outs[0]),
            ctx.commit_open_begin(witnesses[1], coeffs, cols, q0, zf, outs[1])]
    with pytest.raises(cabi.ZipError):
        ctx.commit_open_begin(witnesses[2], coeffs, cols, q0, zf, outs[2])
    got_roots = [jobs[0].wait(want_roots=True)]
    jobs.append(ctx.commit_open_begin(witnesses[2], coeffs, cols, q0, zf, outs[2]))
    got_roots.append(jobs[1].wait(want_roots=True))
    jobs.append(ctx.commit_open_begin(witnesses[3], coeffs, cols, q0, zf, outs[3]))
    got_roots.append(jobs[2].wait(want_roots=True))
    got_roots.append(jobs[3].wait(want_roots=True))
    ctx.synchronize()
    for i in range(4):
        assert np.array_equal(got_roots[i], want[i][1]), i
        bad = np.flatnonzero(outs[i].cpu().numpy() != want[i][0])
        assert bad.size == 0, f"job {i}: {bad.size} proof bytes differ, first at {bad[:8]}"


def test_two_jobs_in_flight_recover_from_timed_out_waits(cabi, monkeypatch):
    """Both jobs' pipeline waits give up (ZIP_HIP_FORCE_WAIT_TIMEOUT): the first zip_job_wait drains the streams and
    clears the flag, the SECOND job must still re-gather (round-2 advisor finding: it returned a proof whose gathers
    had run before the commit kernel published their rows)."""
    torch = pytest.importorskip("torch")
    num_vars = 22
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    point = orc.point_to_field(f, np.arange(-7, num_vars - 7, dtype=np.int64))
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    rng = np.random.default_rng(6)
    coeffs = rng.integers(-(1 << 62), 1 << 62, size=z.num_rows, dtype=np.int64)
    cols = rng.integers(0, z.codeword_len, size=200, dtype=np.uint32)
    monkeypatch.setenv("ZIP_HIP_CHUNKS", "4")
    ctx = _ctx(cabi, z)
    witnesses = [torch.from_numpy(_witness(num_vars, seed=60 + i)).cuda() for i in range(2)]
    want = [ctx.commit_open(w, coeffs, cols, q0, zf)[0] for w in witnesses]
    outs = [torch.full((want[0].size,), 0x5A, dtype=torch.uint8, device="cuda") for _ in witnesses]
    torch.cuda.synchronize()
    monkeypatch.setenv("ZIP_HIP_FORCE_WAIT_TIMEOUT", "200")  # 2 us: the gathers run long before their rows exist
    jobs = [ctx.commit_open_begin(witnesses[i], coeffs, cols, q0, zf, outs[i]) for i in range(2)]
    monkeypatch.delenv("ZIP_HIP_FORCE_WAIT_TIMEOUT")
    for j in jobs:
        j.wait()
    ctx.synchronize()
    for i in range(2):
        bad = np.flatnonzero(outs[i].cpu().numpy() != np.asarray(want[i]))
        assert bad.size == 0, f"job {i}: {bad.size} proof bytes differ, first at {bad[:8]}"
    # and the ctx is back to normal: a plain job afterwards
    j = ctx.commit_open_begin(witnesses[0], coeffs, cols, q0, zf, outs[1])
    j.wait()
    ctx.synchronize()
    assert np.array_equal(outs[1].cpu().numpy(), np.asarray(want[0]))


@pytest.mark.parametrize("num_vars", [16, 20])
def test_plain_commit_speculates_with_the_last_columns(cabi, num_vars):
    """The two UNCHANGED calls of ZincProver (commit, then open on a fresh transcript: prover.rs:315-320): after a first
    opening the ctx hints its plain zip_commit with that column list.  Byte-identical proofs for commit -> open (same
    columns: the fast path), commit -> open (OTHER columns: transparent re-run from the witness zip_open is handed),
    commit -> download (re-run from the device witness, digest intact); a DEVICE witness overwritten in between is
    refused, not silently re-read."""
    torch = pytest.importorskip("torch")
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(num_vars, seed=77)
    point = orc.point_to_field(f, np.arange(num_vars, dtype=np.int64) + 9)
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    ctx = _ctx(cabi, z)
    d = torch.from_numpy(evals).cuda()
    ctx.set_profiling(True)
    # 0. the default: a DEVICE witness is never speculated on (the caller was not asked to keep it) ...
    com, _ = ctx.commit(d)
    assert np.array_equal(com.open(d, coeffs, cols, q0, zf), proof_o)
    com.free()
    ctx.profile_read()
    com, _ = ctx.commit(d)  # (the ctx has seen the columns by now)
    rows, _, _ = com.download()
    assert np.array_equal(rows, rows_o) and ctx.profile_read()["raa_commit_kernel"][0] == 1  # everything was stored
    com.free()
    # ... a HOST witness is (the library owns the copy a re-run reads): one launch for commit + open, the same bytes
    com, roots = ctx.commit(evals)
    assert np.array_equal(roots, roots_o)
    assert np.array_equal(com.open(evals, coeffs, cols, q0, zf), proof_o)
    assert ctx.profile_read()["raa_commit_kernel"][0] == 1
    rows, _, _ = com.download()  # completes itself from the library's copy: a second launch
    assert np.array_equal(rows, rows_o) and ctx.profile_read()["raa_commit_kernel"][0] == 1
    com.free()
    ctx = _ctx(cabi, z)
    ctx.set_profiling(True)
    ctx.set_speculation(True)  # opt in: device witnesses too, from here on
    # 1. nothing seen yet: a full commit; its opening names the columns
    com, roots = ctx.commit(d)
    assert np.array_equal(roots, roots_o)
    assert np.array_equal(com.open(d, coeffs, cols, q0, zf), proof_o)
    com.free()
    ctx.profile_read()
    # 2. the fast path: ONE commit launch, the same bytes
    com, roots = ctx.commit(d)
    assert np.array_equal(roots, roots_o)
    assert np.array_equal(com.open(d, coeffs, cols, q0, zf), proof_o)
    assert ctx.profile_read()["raa_commit_kernel"][0] == 1
    # ... and the same handle opened with OTHER columns completes itself first (second launch) -- right bytes again
    cols2 = ((cols[::-1].astype(np.int64) + 3) % z.codeword_len).astype(np.uint32)
    plain = _ctx(cabi, z)
    plain.set_speculation(False)  # (a fully materialised commitment opened with cols2: checked against the oracle elsewhere)
    c_full, _ = plain.commit(d)
    want2 = c_full.open(d, coeffs, cols2, q0, zf)
    c_full.free()
    assert not np.array_equal(want2, proof_o)
    assert np.array_equal(com.open(d, coeffs, cols2, q0, zf), want2)
    assert ctx.profile_read()["raa_commit_kernel"][0] == 1
    com.free()
    # 3. commit -> download: everything the reference's MultilinearZipData holds
    com, _ = ctx.commit(d)  # (hinted with cols2 now: the last opening's list)
    rows, layers, roots3 = com.download()
    assert np.array_equal(rows, rows_o) and np.array_equal(roots3, roots_o)
    assert np.array_equal(layers, layers_o[:, : 2 * z.codeword_len - 2])
    com.free()
    # 4. a device witness overwritten between the commit and the completion: refused
    com, _ = ctx.commit(d)
    ctx.synchronize()
    d2 = d.clone()
    d[5] += 1
    torch.cuda.synchronize()
    with pytest.raises(cabi.ZipError):
        com.download()
    com.free()
    # 5. a HOST witness is copied by the commit: completing its handle never looks at the caller's array again
    host = evals.copy()
    com, _ = ctx.commit(host)
    host[:] = 0
    rows, _, _ = com.download()
    assert np.array_equal(rows, rows_o)
    com.free()
    # 6. switched off: a plain commit stores everything again
    ctx.set_speculation(False)
    ctx.profile_read()
    com, _ = ctx.commit(d2)
    rows, _, _ = com.download()
    assert np.array_equal(rows, rows_o) and ctx.profile_read()["raa_commit_kernel"][0] == 1
    com.free()


def _device_bytes(ptr, n):
    """n bytes at device address ptr (device 0) -> numpy, through a zero-copy torch view"""
    import torch

    holder = type("_H", (), {})()
    holder.__cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(holder, device="cuda:0").cpu().numpy()


@pytest.mark.parametrize("shards", [1, 2, 4])
def test_multi_device_context_on_the_2pow26_geometry(cabi, shards):
    """zip_mctx over cw = 16384 (raa_commit16_kernel, packed openings, the image-free gather): a 16-row slice of the
    BASELINE configs[3] geometry, sharded by rows; proof, roots and the gathered commitment equal the oracle's."""
    nv, geo = 17, (8192, 16, 16384)
    z = orc.Zip(nv, geometry=geo)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(nv, seed=43)
    point = orc.point_to_field(f, np.arange(5, nv + 5, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[nv - lr:])
    m = cabi.ZipMultiContext(nv, z.perm1, z.perm2, [0] * shards, geometry_override=geo)
    for evals_arg in (evals, None):  # host witness, then the slices it left on the devices
        proof, roots = m.commit_open(evals_arg, coeffs, cols, q0, zf)
        assert np.array_equal(roots, roots_o)
        bad = np.flatnonzero(proof != proof_o)
        assert bad.size == 0, f"{bad.size} proof bytes differ, first at {bad[:8]}"
        for sh in range(shards):
            assert np.array_equal(_device_bytes(m.roots_ptr(sh), z.num_rows * 32).reshape(z.num_rows, 32), roots_o), sh
    m.close()


@pytest.mark.parametrize("knob", ["ZIP_HIP_MCTX_FORCE_NO_RCCL", "ZIP_HIP_MCTX_FORCE_NO_PEER", "both"])
@pytest.mark.parametrize("shards", [1, 3, 4])
def test_multi_device_context_without_rccl_or_peer_access(cabi, shards, knob, monkeypatch):
    """What zip_mctx does on a box whose librccl is missing / refuses (ZIP_HIP_MCTX_FORCE_NO_RCCL: the roots travel as
    device copies -- also for ONE shard, which otherwise takes the real one-rank RCCL path) or whose devices cannot map
    each other (ZIP_HIP_MCTX_FORCE_NO_PEER: no hipDeviceEnablePeerAccess; hipMemcpyPeerAsync stages): the same bytes.
    (Round-3 verdict: the first real 8-GPU run must not be the first time these branches execute.)"""
    for k in (["ZIP_HIP_MCTX_FORCE_NO_RCCL", "ZIP_HIP_MCTX_FORCE_NO_PEER"] if knob == "both" else [knob]):
        monkeypatch.setenv(k, "1")
    num_vars = 16
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(num_vars, seed=47)
    point = orc.point_to_field(f, np.arange(2, num_vars + 2, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    m = cabi.ZipMultiContext(num_vars, z.perm1, z.perm2, [0] * shards)
    proof, roots = m.commit_open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(roots, roots_o) and np.array_equal(proof, proof_o)
    want_path = "copies" if (shards > 1 or knob != "ZIP_HIP_MCTX_FORCE_NO_PEER") else "rccl"
    assert m.roots_path() == want_path, m.roots_path()
    for sh in range(shards):
        assert np.array_equal(_device_bytes(m.roots_ptr(sh), z.num_rows * 32).reshape(z.num_rows, 32), roots_o), sh
    m.close()


@pytest.mark.parametrize("num_vars", [12, 16, 18])
@pytest.mark.parametrize("shards", [1, 2, 3, 4, 8])
def test_multi_device_context_proof_equals_unsharded(cabi, num_vars, shards):
    """zip_mctx (SURVEY 8e behind the C ABI, one process): rows split over `shards` contexts -- here all on device 0,
    which is what a one-GPU box can run -- every shard commits and opens its rows, the partial row combinations are
    added on the lead shard, every shard delivers its row slice of every column to the host proof.  Roots and every
    proof byte equal the oracle's unsharded ones (3 shards: uneven blocks of rows)."""
    z = orc.Zip(num_vars)
    f = orc.make_field(BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    evals = _witness(num_vars, seed=41)
    point = orc.point_to_field(f, np.arange(2, num_vars + 2, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    m = cabi.ZipMultiContext(num_vars, z.perm1, z.perm2, [0] * shards)
    assert m.shards() == shards
    proof, roots = m.commit_open(evals, coeffs, cols, q0, zf)
    assert np.array_equal(roots, roots_o)
    bad = np.flatnonzero(proof != proof_o)
    assert bad.size == 0, f"{bad.size} proof bytes differ, first at {bad[:8]}"
    # the one exchange of the commit: every shard's device holds the roots of ALL rows (commit.rs:78-81).  One shard
    # on device 0 is a one-rank in-process RCCL communicator (the real ncclAllGather path); repeated ordinals copy.
    assert m.roots_path() == ("rccl" if shards == 1 else "copies"), m.roots_path()
    for sh in range(shards):
        assert np.array_equal(_device_bytes(m.roots_ptr(sh), z.num_rows * 32).reshape(z.num_rows, 32), roots_o), sh
    # witness resident on the devices, second call through the same context (buffers reused)
    m.set_witness(evals)
    proof2, roots2 = m.commit_open(None, coeffs, cols, q0, zf)
    assert np.array_equal(roots2, roots_o) and np.array_equal(proof2, proof_o)
    # a different field width through the same context
    f2 = orc.make_field(TEST_MODULUS_2, 2)
    pt2 = orc.point_to_field(f2, np.arange(2, num_vars + 2, dtype=np.int64))
    proof_o2, cols2, coeffs2 = z.open(f2, evals, rows_o, layers_o, pt2, orc.new_transcript())
    q02 = orc.build_eq_x_r(f2, pt2[num_vars - lr:])
    proof3, _ = m.commit_open(None, coeffs2, cols2, q02, cabi.make_field(TEST_MODULUS_2, 2), want_roots=False)
    assert np.array_equal(proof3, proof_o2)
    m.close()
