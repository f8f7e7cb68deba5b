"""GPU parity at INT_LIMBS = 2: commit, row combinations, column gather, whole proofs, the witness MLE and both field maps
of a two-limb ctx, called through the C ABI, against the CPU oracle at n_limbs = 2 on identical inputs.  Bit-exact:
there are no tolerances.  Needs a real MI355X."""
import functools

import numpy as np
import pytest

import _oracle as orc
import _two_limb as tl

pytestmark = pytest.mark.gpu

WHOLE = [1, 2, 3, 4, 7, 8, 10, 12, 13, 16]
# slices (num_vars, (row_len, num_rows, codeword_len), rep) of the real geometries: the smallest shapes in which a thread of
# the scan owns more than one codeword position (8 / 32 / 64 / 128 / 256) and the lanes reach their last limb
SLICES = {"cw2048": (12, (1024, 4, 2048), 2), "cw8192": (14, (4096, 4, 8192), 2), "cw16384": (14, (8192, 2, 16384), 2),
          "cw32768": (15, (16384, 2, 32768), 2), "cw65536": (15, (16384, 2, 65536), 4)}


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


@functools.lru_cache(maxsize=None)
def _committed(num_vars, kind="random", geometry=None, rep=2, n_cols=tl.N_COLS):
    """(z, evals, rows, layers, roots): the oracle's commit, computed once per shape and witness and never modified"""
    z = tl.Zip2(num_vars, geometry=geometry, rep=rep, n_cols=n_cols)
    evals = tl.witness(z, kind)
    rows, layers, roots = z.commit(evals)
    for a in (evals, rows, layers, roots):
        a.setflags(write=False)
    return z, evals, rows, layers, roots


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(np.asarray(got).reshape(-1) != np.asarray(want).reshape(-1))
        pytest.fail(f"{what}: {bad.size} of {np.asarray(want).size} words differ, first at {bad[:8].tolist()}")


def _check_commit(cabi, z, evals, rows_o, layers_o, roots_o):
    ctx = z.ctx(cabi)
    com, roots = ctx.commit(evals)
    rows, layers, roots_d = com.download()
    assert rows.shape == (z.num_rows * z.codeword_len, 8)
    _same(rows, rows_o, "rows")
    _same(roots, roots_o, "roots")
    _same(roots_d, roots_o, "downloaded roots")
    _same(layers, layers_o[:, :-1, :], "tree layers")  # the reference's layers have the root popped
    com2, r2 = ctx.commit(evals, with_merkle=False)
    assert r2 is None
    _same(com2.download(layers=False, roots=False)[0], rows_o, "rows of commit_no_merkle")
    return ctx, com


@pytest.mark.parametrize("num_vars", WHOLE)
def test_commit_bit_exact(cabi, num_vars):
    _check_commit(cabi, *_committed(num_vars))


@pytest.mark.parametrize("kind", ["max", "min", "lowtop"])
@pytest.mark.parametrize("num_vars", [7, 12])
def test_commit_of_the_extreme_witnesses(cabi, num_vars, kind):
    _check_commit(cabi, *_committed(num_vars, kind))


def test_commit_from_device_memory_and_device_views(cabi):
    import torch

    z, evals, rows_o, layers_o, roots_o = _committed(10)
    ctx = z.ctx(cabi)
    ev_d = torch.from_numpy(evals.view(np.int64).copy()).cuda()
    assert tuple(ev_d.shape) == (1 << 10, 2)
    com, roots = ctx.commit(ev_d)
    _same(roots, roots_o, "roots")
    rows_p, layers_p, roots_p = com.device_ptrs()
    ctx.synchronize()
    # row_count * cw * 8 u64 behind the pointer, through a zero-copy torch view
    holder = type("_H", (), {})()
    holder.__cuda_array_interface__ = {"shape": (rows_o.size * 8,), "typestr": "|u1", "data": (int(rows_p), False), "version": 2}
    got = torch.as_tensor(holder, device="cuda:0").cpu().numpy()
    _same(got.view(np.uint64).reshape(rows_o.shape), rows_o, "rows behind the device pointer")
    holder.__cuda_array_interface__ = {"shape": (roots_o.size,), "typestr": "|u1", "data": (int(roots_p), False), "version": 2}
    _same(torch.as_tensor(holder, device="cuda:0").cpu().numpy().reshape(roots_o.shape), roots_o, "roots behind the device pointer")
    assert layers_p
    with pytest.raises(cabi.ZipError) as e:  # n_evals counts coefficients
        ctx.commit(evals[:-1])
    assert e.value.code == cabi.ZIP_ERR_SHAPE


@pytest.mark.parametrize("num_vars", WHOLE)
def test_open_testing_bit_exact(cabi, num_vars):
    z, evals, *_ = _committed(num_vars)
    coeffs = tl.challenge_like(z.num_rows, 77)
    rc, expect = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    got = z.ctx(cabi).open_testing(evals, coeffs)
    assert got.shape == (z.row_len, 16)
    _same(got, expect, "u'")


@pytest.mark.parametrize("kind", ["max", "min", "lowtop"])
def test_row_combinations_at_their_bounds(cabi, kind):
    """every product at +-2^254 with one sign over the rows of 2^12 / 2^16, and the low-limb top bits"""
    for num_vars in (12, 16):
        z, evals, *_ = _committed(num_vars, kind)
        for coeffs in (np.tile(tl.to_limbs([tl.INT2_MIN]), (z.num_rows, 1)), np.tile(tl.to_limbs([tl.INT2_MAX]), (z.num_rows, 1))):
            rc, expect = z.combine_rows_int(coeffs, evals)
            assert rc == 0
            _same(z.ctx(cabi).open_testing(evals, coeffs), expect, "u'")


def _q0(z, modulus, fl, seed):
    rng = np.random.default_rng(seed)
    vals = [int.from_bytes(rng.bytes(8 * fl), "little") % modulus for _ in range(z.num_rows)]
    vals[0] = modulus - 1
    return orc.field_elems(vals, fl)


@pytest.mark.parametrize("modulus,fl", tl.MODULI)
@pytest.mark.parametrize("num_vars", [3, 8])
def test_open_eval_bit_exact_for_every_modulus(cabi, num_vars, modulus, fl):
    f = orc.make_field(modulus, fl)
    for kind in ("random", "lowtop", "max", "min"):
        z, evals, *_ = _committed(num_vars, kind)
        q0 = _q0(z, modulus, fl, num_vars)
        _same(z.ctx(cabi).open_eval(evals, q0, cabi.make_field(modulus, fl)), z.combine_rows_field(f, q0, evals), f"row ({kind})")


@pytest.mark.parametrize("num_vars", WHOLE)
def test_open_eval_bit_exact_at_every_size(cabi, num_vars):
    f = orc.make_field(tl.BENCH_MODULUS, 4)
    z, evals, *_ = _committed(num_vars)
    q0 = _q0(z, tl.BENCH_MODULUS, 4, num_vars)
    _same(z.ctx(cabi).open_eval(evals, q0, cabi.make_field(tl.BENCH_MODULUS, 4)), z.combine_rows_field(f, q0, evals), "row")


@pytest.mark.parametrize("modulus,fl", tl.MODULI)
def test_one_row_matrix_is_map_to_field(cabi, modulus, fl):
    """num_rows == 1: q0 is ignored, the row is phi(evals), the stream has no u'"""
    z = tl.Zip2(0)
    assert z.num_rows == 1 and z.row_len == 1
    f = orc.make_field(modulus, fl)
    ctx = z.ctx(cabi)
    for v in (tl.INT2_MIN, tl.INT2_MAX, 0, -1, (1 << 100) + 2, -(modulus % (1 << 126)) - 1):
        evals = tl.to_limbs([v])
        got = ctx.open_eval(evals, None, cabi.make_field(modulus, fl))
        _same(got, z.map_to_field(f, evals), f"phi({v})")
    evals = tl.to_limbs([tl.INT2_MIN])
    rows, layers, roots = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows, layers, np.zeros((0, fl), dtype=np.uint64))
    com, roots_d = ctx.commit(evals)
    _same(roots_d, roots, "roots")
    proof = com.open(evals, None, cols, None, cabi.make_field(modulus, fl))
    assert proof.size == z.proof_len(fl) == tl.N_COLS * (64 + 8 + 32 * z.depth) + 8 * fl  # no u' in front
    _same(proof, proof_o, "proof")


def _open_all_ways(cabi, z, evals, rows_o, layers_o, roots_o, modulus, fl):
    f = orc.make_field(modulus, fl)
    zf = cabi.make_field(modulus, fl)
    point = tl.make_point(f, z.num_vars)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point)
    q0, q1 = z.tensors(f, point)
    ctx = z.ctx(cabi)
    com, roots = ctx.commit(evals)
    _same(roots, roots_o, "roots")
    single = z.num_rows == 1
    proof = com.open(evals, None if single else coeffs, cols, q0, zf)
    assert proof.size == proof_o.size == z.proof_len(fl)
    _same(proof, proof_o, "zip_open")
    _same(com.open(None, None if single else coeffs, cols, q0, zf), proof_o, "zip_open from the retained witness")
    proof2, roots2, kept = ctx.commit_open(evals, None if single else coeffs, cols, q0, zf, keep=True)
    _same(proof2, proof_o, "zip_commit_open")
    _same(roots2, roots_o, "zip_commit_open roots")
    _same(kept.open_columns(cols), proof_o[z.row_len * 128 * (not single): proof_o.size - z.row_len * 8 * fl], "zip_open_columns")
    hinted, roots3 = ctx.commit(evals, hint_cols=cols[:5])
    _same(roots3, roots_o, "zip_commit_hinted roots")
    _same(hinted.open(evals, None if single else coeffs, cols, q0, zf), proof_o, "zip_open on a hinted handle")
    up = ctx.upload_commitment(rows_o, layers_o[:, :-1, :], roots_o)
    _same(up.open(evals, None if single else coeffs, cols, q0, zf), proof_o, "zip_open on an uploaded handle")
    r, l, t = up.download()
    _same(r, rows_o, "uploaded rows")
    _same(l, layers_o[:, :-1, :], "uploaded layers")
    _same(t, roots_o, "uploaded roots")
    # the witness MLE at the point
    want = z.mle_eval(f, evals, point)
    assert orc.limbs_to_int(ctx.mle_eval(evals, q0, q1, zf)) == want
    # ... and over the witness a host-side commit left on the device with its handle
    value = np.zeros(fl, dtype=np.uint64)
    rc = cabi.lib().zip_commitment_mle_eval(com._h, None if q0 is None else q0.ctypes.data, None if q1 is None else q1.ctypes.data,
                                            zf, value.ctypes.data)
    assert rc == cabi.ZIP_OK and orc.limbs_to_int(value) == want
    return ctx, proof_o, cols, coeffs, q0, q1, want


@pytest.mark.parametrize("num_vars", WHOLE)
def test_open_commit_open_upload_and_mle_eval(cabi, num_vars):
    _open_all_ways(cabi, *_committed(num_vars), tl.BENCH_MODULUS, 4)


@pytest.mark.parametrize("modulus,fl", tl.MODULI[1:])
def test_whole_proofs_for_the_other_moduli(cabi, modulus, fl):
    _open_all_ways(cabi, *_committed(8), modulus, fl)
    _open_all_ways(cabi, *_committed(7, "lowtop"), modulus, fl)


def test_the_default_thousand_openings(cabi):
    z, evals, rows_o, layers_o, roots_o = _committed(10, n_cols=1000)
    f = orc.make_field(tl.BENCH_MODULUS, 4)
    zf = cabi.make_field(tl.BENCH_MODULUS, 4)
    point = tl.make_point(f, 10)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point)
    assert cols.size == 1000 and len(set(cols.tolist())) < 1000  # duplicates among them
    q0, _ = z.tensors(f, point)
    ctx = z.ctx(cabi)
    com, _ = ctx.commit(evals)
    _same(com.open(evals, coeffs, cols, q0, zf), proof_o, "zip_open, 1000 openings")
    _same(ctx.commit_open(evals, coeffs, cols, q0, zf)[0], proof_o, "zip_commit_open, 1000 openings")


def test_device_resident_witness_and_proof(cabi):
    import torch

    z, evals, rows_o, layers_o, roots_o = _committed(12)
    f = orc.make_field(tl.MOD_3LIMB, 3)
    zf = cabi.make_field(tl.MOD_3LIMB, 3)
    point = tl.make_point(f, 12)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point)
    q0, q1 = z.tensors(f, point)
    ctx = z.ctx(cabi)
    ev_d = torch.from_numpy(evals.view(np.int64).copy()).cuda()
    out_d = torch.zeros(proof_o.size, dtype=torch.uint8, device="cuda")
    ctx.commit_open(ev_d, coeffs, cols, q0, zf, out=out_d)
    ctx.synchronize()
    _same(out_d.cpu().numpy(), proof_o, "zip_commit_open, device to device")
    u_d = torch.zeros((z.row_len, 16), dtype=torch.int64, device="cuda")
    ctx.open_testing(ev_d, coeffs, out=u_d)
    ctx.synchronize()
    _same(u_d.cpu().numpy().view(np.uint64), z.combine_rows_int(coeffs, evals)[1], "u' on the device")
    assert orc.limbs_to_int(ctx.mle_eval(ev_d, q0, q1, zf)) == z.mle_eval(f, evals, point)


@pytest.mark.parametrize("kind", ["random", "max", "min"])
@pytest.mark.parametrize("which", sorted(SLICES))
def test_slices_of_the_real_geometries(cabi, which, kind):
    num_vars, geometry, rep = SLICES[which]
    z, evals, rows_o, layers_o, roots_o = _committed(num_vars, kind, geometry, rep)
    assert (z.row_len, z.num_rows, z.codeword_len) == geometry
    ctx, com = _check_commit(cabi, z, evals, rows_o, layers_o, roots_o)
    f = orc.make_field(tl.BENCH_MODULUS, 4)
    zf = cabi.make_field(tl.BENCH_MODULUS, 4)
    point = tl.make_point(f, num_vars)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point)
    q0, _ = z.tensors(f, point)
    _same(com.open(evals, coeffs, cols, q0, zf), proof_o, "zip_open")
    _same(ctx.commit_open(evals, coeffs, cols, q0, zf)[0], proof_o, "zip_commit_open")


@pytest.mark.parametrize("modulus,fl", tl.MODULI + [(tl.MOD_M127, 2)])
def test_field_map_int_equals_the_oracle(cabi, modulus, fl):
    f = orc.make_field(modulus, fl)
    ctx = tl.Zip2(2).ctx(cabi)
    one_limb = cabi.ZipContext(2, *[orc.shuffle_perm(s, 4) for s in (1, 2)])  # the diagnostic works on any ctx
    for width in (2, 8):
        vals = tl.field_map_values(modulus, fl, width)
        assert vals.shape == (512, width)
        want = np.stack([orc.field_from_int(f, v) for v in vals])
        _same(ctx.field_map_int(vals, width, cabi.make_field(modulus, fl)), want, f"phi of Int<{width}>")
        _same(one_limb.field_map_int(vals[:64], width, cabi.make_field(modulus, fl)), want[:64], f"phi of Int<{width}>, one-limb ctx")
    with pytest.raises(cabi.ZipError) as e:
        ctx.field_map_int(np.zeros((2, 4), dtype=np.uint64), 4, cabi.make_field(modulus, fl))
    assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED
