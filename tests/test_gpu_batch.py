"""GPU parity of the batch path (zip_batch_commit / _member / _open_eval / _open): many polynomials of one geometry in
one launch set, against the CPU oracle and against the per-polynomial calls.  Bit-exact.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189  # benches/spartan_benches.rs:134-137
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59


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


def _batch_witness(num_vars, n_polys, seed=0, small=False):
    """[n_polys, 2^num_vars]: a different seed per polynomial, the extremes in every one"""
    return np.stack([_witness(num_vars, seed=seed + 101 * i + 1, small=small) for i in range(n_polys)])


# ---------------------------------------------------------------------------------------------- commit
# a single row, R = 2, the four E variants of commit_geom (E = 1, 2, 4 and E = 8 with 64 threads), odd sizes
@pytest.mark.parametrize("num_vars,n_polys", [(0, 3), (1, 3), (3, 3), (8, 3), (12, 3), (13, 3), (15, 3), (8, 1)])
def test_batch_commit_equals_oracle(cabi, num_vars, n_polys):
    z = orc.Zip(num_vars)
    evals = _batch_witness(num_vars, n_polys)
    ctx = _ctx(cabi, z)
    batch = ctx.batch_commit(evals)
    assert len(batch) == n_polys and batch.roots.shape == (n_polys, z.num_rows, 32)
    for i in range(n_polys):
        rows_o, layers_o, roots_o = z.commit(evals[i])
        assert np.array_equal(batch.roots[i], roots_o), i
        rows, layers, roots = batch.member(i).download()
        assert np.array_equal(rows, rows_o), i
        assert np.array_equal(layers, layers_o[:, :-1, :]), i  # reference layers have the root popped
        assert np.array_equal(roots, roots_o), i
    batch.free()


# ------------------------------------------------------------------------------------------------ open
def _oracle_batch_open(z, f, evals, points):
    """z.open of every polynomial on ONE Keccak -> [(proof, cols, coeffs, roots)], what batch_open leaves behind"""
    fs = orc.new_transcript()
    out = []
    for ev, pt in zip(evals, points):
        rows_o, layers_o, roots_o = z.commit(ev)
        proof, cols, coeffs = z.open(f, ev, rows_o, layers_o, pt, fs)
        out.append((proof, cols.copy(), coeffs.copy(), roots_o))
    return out


OPEN_CASES = [(8, BENCH_MODULUS, 4), (8, TEST_MODULUS_2, 2), (3, TEST_MODULUS_2, 2), (0, BENCH_MODULUS, 4),
              (1, BENCH_MODULUS, 4), (9, MOD_3LIMB, 3), (10, MOD_NO_SPARE, 4), (12, BENCH_MODULUS, 4)]
DEVICE_OUT_CASES = {(8, BENCH_MODULUS, 4), (1, BENCH_MODULUS, 4)}


@pytest.mark.parametrize("num_vars,modulus,fl", OPEN_CASES)
def test_batch_open_equals_oracle_on_one_shared_transcript(cabi, num_vars, modulus, fl):
    B = 5
    z = orc.Zip(num_vars)
    f, zf = orc.make_field(modulus, fl), cabi.make_field(modulus, fl)
    evals = _batch_witness(num_vars, B, seed=7, small=(fl == 2))
    rng = np.random.default_rng(3 + num_vars)
    points_i = rng.integers(-100, 100, size=(B, num_vars), dtype=np.int64)  # a different point per polynomial
    points = [orc.point_to_field(f, p) if num_vars else np.zeros((0, fl), dtype=np.uint64) for p in points_i]
    want = _oracle_batch_open(z, f, evals, points)
    cols = np.stack([w[1] for w in want])
    coeffs = np.stack([w[2] for w in want])
    assert cols.shape == (B, 1000)
    if num_vars >= 3:  # (the challenges differ between the polynomials: a kernel reading slice 0 for everyone fails)
        assert not np.array_equal(cols[0], cols[1])
        assert z.num_rows == 1 or not np.array_equal(coeffs[0], coeffs[1])
    lr = z.num_rows.bit_length() - 1
    q0 = np.stack([orc.build_eq_x_r(f, pt[num_vars - lr:]) for pt in points]) if lr else None

    ctx = _ctx(cabi, z)
    batch = ctx.batch_commit(evals)
    assert np.array_equal(batch.roots, np.stack([w[3] for w in want]))
    # the evaluation rows
    rows = batch.open_eval(q0, zf)
    for i in range(B):
        q0_i = q0[i] if lr else orc.field_elems([(1 << (64 * fl)) % modulus], fl)
        assert np.array_equal(rows[i], z.combine_rows_field(f, q0_i, evals[i])), i
        be = want[i][0][-z.row_len * 8 * fl:].reshape(z.row_len, fl, 8)  # the same row at the end of the oracle's proof
        assert np.array_equal(rows[i], be[:, ::-1, ::-1].copy().view("<u8").reshape(z.row_len, fl)), i
    # the proof streams: the concatenation of the oracle's
    expect = np.concatenate([w[0] for w in want])
    cf = coeffs if z.num_rows > 1 else None
    proofs = batch.open(cf, cols, q0, zf)
    assert proofs.shape == (B, z.proof_len(fl)) and z.proof_len(fl) % 8 == 0
    assert np.array_equal(proofs.reshape(-1), expect)
    if (num_vars, modulus, fl) in DEVICE_OUT_CASES:
        torch = pytest.importorskip("torch")
        out = torch.zeros(expect.size, dtype=torch.uint8, device="cuda")
        batch.open(cf, cols, q0, zf, out=out)
        assert np.array_equal(out.cpu().numpy(), expect)
    # the oracle's verifier, looped on one fresh transcript, accepts all five (where the single-proof test verifies)
    if z.row_len > 1 and modulus != MOD_NO_SPARE:
        fs = orc.new_transcript()
        for i in range(B):
            ev = z.mle_eval(f, evals[i], points[i])
            assert z.verify(f, batch.roots[i], points[i], ev, proofs[i], fs=fs) == 0, i


# ----------------------------------------------------------------------- batch == loop, across commit rounds
def _hand_made_cols(cw, n_polys):
    """8 columns per polynomial: 0, cw - 1, a duplicate and a sibling pair in every list, the rest different per polynomial"""
    out = np.zeros((n_polys, 8), dtype=np.uint32)
    for i in range(n_polys):
        a = (7 * i + 3) % cw
        s = (2 * ((5 * i + 1) % (cw // 2)))
        out[i] = [0, cw - 1, a, a, s, s + 1, (11 * i + cw // 2) % cw, (13 * i + 5) % cw]
    return out


# 2^12 x 40: 2560 one-wave workgroups against at most 2048 resident -- a second, partial round of the persistent kernel
@pytest.mark.parametrize("num_vars,n_polys", [(12, 40), (15, 20)])
@pytest.mark.parametrize("where", ["host", "device"])
def test_batch_equals_the_loop_across_commit_rounds(cabi, num_vars, n_polys, where):
    z = orc.Zip(num_vars)
    f, zf = orc.make_field(BENCH_MODULUS, 4), cabi.make_field(BENCH_MODULUS, 4)
    evals = _batch_witness(num_vars, n_polys, seed=31)
    cols = _hand_made_cols(z.codeword_len, n_polys)
    coeffs = np.stack([orc.splitmix64(1000 + i, z.num_rows).copy() for i in range(n_polys)]).astype(np.int64)
    coeffs[:, 0], coeffs[:, 1] = -(2**63), 2**63 - 1
    lr = z.num_rows.bit_length() - 1
    rng = np.random.default_rng(num_vars)
    q0 = np.stack([orc.build_eq_x_r(f, orc.point_to_field(f, rng.integers(-50, 50, size=lr, dtype=np.int64)))
                   for _ in range(n_polys)])
    ctx = _ctx(cabi, z)
    if where == "device":
        torch = pytest.importorskip("torch")
        witness = torch.from_numpy(evals).cuda()
    else:
        witness = evals
    batch = ctx.batch_commit(witness)
    proofs = batch.open(coeffs, cols, q0, zf)
    rows = batch.open_eval(q0, zf)
    for i in range(n_polys):  # the per-polynomial calls, which the existing suite pins to the oracle
        com, roots = ctx.commit(evals[i])
        assert np.array_equal(batch.roots[i], roots), i
        assert np.array_equal(proofs[i], com.open(evals[i], coeffs[i], cols[i], q0[i], zf)), i
        assert np.array_equal(rows[i], ctx.open_eval(evals[i], q0[i], zf)), i
        com.free()


# proof_len is a multiple of 8, not of 16: one row and an odd number of openings (72 bytes each), or a one-element
# evaluation row of a 3-limb field (24 bytes) -- every second stream then starts at 8 mod 16
@pytest.mark.parametrize("num_vars,modulus,fl,n_cols", [(0, BENCH_MODULUS, 4, 3), (1, MOD_3LIMB, 3, 5), (2, MOD_3LIMB, 3, 7)])
def test_streams_that_start_at_8_mod_16(cabi, num_vars, modulus, fl, n_cols):
    B = 4
    z = orc.Zip(num_vars)
    f, zf = orc.make_field(modulus, fl), cabi.make_field(modulus, fl)
    ctx = _ctx(cabi, z)
    if num_vars < 2:
        assert ctx.proof_len(n_cols, fl) % 16 == 8
    evals = _batch_witness(num_vars, B, seed=77)
    rng = np.random.default_rng(num_vars)
    cols = rng.integers(0, z.codeword_len, size=(B, n_cols), dtype=np.uint32)
    lr = z.num_rows.bit_length() - 1
    coeffs = rng.integers(-(2**63), 2**63 - 1, size=(B, z.num_rows), dtype=np.int64) if lr else None
    q0 = np.stack([orc.build_eq_x_r(f, orc.point_to_field(f, rng.integers(-9, 9, size=lr, dtype=np.int64))) for _ in range(B)]) if lr else None
    batch = ctx.batch_commit(evals)
    proofs = batch.open(coeffs, cols, q0, zf)
    for i in range(B):
        com, _ = ctx.commit(evals[i])
        want = com.open(evals[i], coeffs[i] if lr else None, cols[i], q0[i] if lr else None, zf)
        assert np.array_equal(proofs[i], want), i
    torch = pytest.importorskip("torch")
    out = torch.zeros(proofs.size, dtype=torch.uint8, device="cuda")
    batch.open(coeffs, cols, q0, zf, out=out)
    assert np.array_equal(out.cpu().numpy(), proofs.reshape(-1))


# --------------------------------------------------------------------------------------------- members
def test_members_are_plain_commitments_and_outlive_the_batch(cabi):
    num_vars, B = 8, 4
    z = orc.Zip(num_vars)
    f, zf = orc.make_field(BENCH_MODULUS, 4), cabi.make_field(BENCH_MODULUS, 4)
    evals = _batch_witness(num_vars, B, seed=5)
    ctx = _ctx(cabi, z)
    batch = ctx.batch_commit(evals)
    lr = z.num_rows.bit_length() - 1
    point = orc.point_to_field(f, np.arange(num_vars, dtype=np.int64) - 4)
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    coeffs = orc.splitmix64(9, z.num_rows).copy()
    batch_cols = np.tile(np.arange(8, dtype=np.uint32), (B, 1))
    batch.open(np.tile(coeffs, (B, 1)), batch_cols, np.stack([q0] * B), zf)
    other_cols = np.array([z.codeword_len - 1, 17, 17, 0, 5, 4, z.codeword_len // 2 + 3], dtype=np.uint32)  # not the batch's list
    kept = batch.member(2)
    for i in (0, B - 1):
        m = batch.member(i)
        ref, _ = ctx.commit(evals[i])
        assert np.array_equal(m.open(evals[i], coeffs, other_cols, q0, zf), ref.open(evals[i], coeffs, other_cols, q0, zf)), i
        assert np.array_equal(m.open(None, coeffs, other_cols, q0, zf), ref.open(evals[i], coeffs, other_cols, q0, zf)), i
        assert np.array_equal(m.open_columns(other_cols), ref.open_columns(other_cols)), i
        rows_o, layers_o, roots_o = z.commit(evals[i])
        rows, layers, roots = m.download()
        assert np.array_equal(rows, rows_o) and np.array_equal(layers, layers_o[:, :-1, :]) and np.array_equal(roots, roots_o)
        r, l, t = m.device_ptrs()
        assert r and l and t
        m.free()
        ref.free()
    # (a member that materialised its rows left the batch's own storage as it was)
    assert np.array_equal(batch.member(0).open_columns(other_cols), ctx.commit(evals[0])[0].open_columns(other_cols))
    batch.free()
    ref, _ = ctx.commit(evals[2])
    assert np.array_equal(kept.open(evals[2], coeffs, other_cols, q0, zf), ref.open(evals[2], coeffs, other_cols, q0, zf))
    assert np.array_equal(kept.download()[0], z.commit(evals[2])[0])
    kept.free()


# ---------------------------------------------------------------------------------------- launch count
def test_launch_count_does_not_depend_on_the_batch_size(cabi):
    num_vars = 8
    z = orc.Zip(num_vars)
    f, zf = orc.make_field(BENCH_MODULUS, 4), cabi.make_field(BENCH_MODULUS, 4)
    ctx = _ctx(cabi, z)
    ctx.set_profiling(True)
    counts = {}
    for B in (2, 12):
        evals = _batch_witness(num_vars, B, seed=B)
        q0 = np.stack([orc.build_eq_x_r(f, orc.point_to_field(f, [i, 2, 3, 4])) for i in range(B)])
        coeffs = np.arange(B * z.num_rows, dtype=np.int64).reshape(B, -1) - 7
        cols = (np.arange(B * 16, dtype=np.uint32).reshape(B, 16) * 3) % z.codeword_len
        ctx.profile_read()
        batch = ctx.batch_commit(evals)
        batch.open_eval(q0, zf)
        batch.open(coeffs, cols, q0, zf)
        times = ctx.profile_read()
        counts[B] = sum(v[0] for v in times.values())
        assert times["raa_commit_kernel"][0] == 1 and times["batch_open_columns_kernel"][0] == 1, times
        batch.free()
    assert counts[2] == counts[12] and counts[2] > 0, counts


# ---------------------------------------------------------------------------------------- usage errors
def _raw_batch_commit(cabi, ctx, evals, n_evals, n_polys):
    h = C.c_void_p()
    rc = cabi.lib().zip_batch_commit(ctx._h, evals.ctypes.data, n_evals, n_polys, cabi.MEM_HOST, None, C.byref(h))
    assert rc != 0 and not h.value
    return rc


def test_batch_usage_errors(cabi):
    z = orc.Zip(8)
    ctx = _ctx(cabi, z)
    evals = _batch_witness(8, 3)
    assert _raw_batch_commit(cabi, ctx, evals, evals.size - 1, 3) == cabi.ZIP_ERR_SHAPE
    assert _raw_batch_commit(cabi, ctx, evals, evals.size, 2) == cabi.ZIP_ERR_SHAPE
    assert _raw_batch_commit(cabi, ctx, evals, 0, 0) == cabi.ZIP_ERR_INVALID_PARAM
    assert _raw_batch_commit(cabi, ctx, evals, evals.size, 65536) == cabi.ZIP_ERR_INVALID_PARAM
    assert cabi.lib().zip_batch_commit(ctx._h, None, 0, 1, cabi.MEM_HOST, None, C.byref(C.c_void_p())) == cabi.ZIP_ERR_NULL
    # a row-sharded ctx
    shard = _ctx(cabi, z, row_begin=0, row_count=z.num_rows // 2)
    assert _raw_batch_commit(cabi, shard, evals, evals.size, 3) == cabi.ZIP_ERR_INVALID_PARAM
    # codewords above 16384 are not launch-bound: refused, and nothing is launched
    zb = orc.Zip(15, geometry=(16384, 2, 32768))
    big = _ctx(cabi, zb)
    big.set_profiling(True)
    w = np.zeros((2, 2 * 16384), dtype=np.int64)
    assert _raw_batch_commit(cabi, big, w, w.size, 2) == cabi.ZIP_ERR_UNSUPPORTED
    assert sum(v[0] for v in big.profile_read().values()) == 0
    # members and columns
    batch = ctx.batch_commit(evals)
    with pytest.raises(cabi.ZipError) as e:
        batch.member(3)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    f, zf = orc.make_field(BENCH_MODULUS, 4), cabi.make_field(BENCH_MODULUS, 4)
    q0 = np.stack([orc.build_eq_x_r(f, orc.point_to_field(f, [1, 2, 3, 4]))] * 3)
    coeffs = np.ones((3, z.num_rows), dtype=np.int64)
    cols = np.zeros((3, 4), dtype=np.uint32)
    cols[2, 3] = z.codeword_len
    with pytest.raises(cabi.ZipError) as e:
        batch.open(coeffs, cols, q0, zf)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    cols[2, 3] = z.codeword_len - 1
    assert batch.open(coeffs, cols, q0, zf).shape[0] == 3  # the handle is still usable
