"""GPU: the prover side of num_proximity_testing = T > 1 (zip_ctx_set_proximity_tests) through the C ABI, bit-exact
against orc_open: u'_0 .. u'_{T-1} head the stream, the column section and the evaluation row follow unchanged.

Sizes: the smallest at which combine_rows_extra_kernel takes each of its paths.  num_rows is a power of two, so the rows
per chunk are 1 (2^3, 2^9), 2 (2^13: the remainder loop only -- not a multiple of the 4-row unroll), 8 (2^16: two
unrolled passes, one full workgroup of 256 columns) and 16 (2^18: two column workgroups, 32 chunks)."""
import numpy as np
import pytest

import _oracle as orc
import _proximity as px

pytestmark = pytest.mark.gpu

N_COLS = 8
SIZES = [3, 9, 13, 16, 18]
NEW_PASS = "combine_rows_extra_kernel"


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _ctx(cabi, i, T=None):
    ctx = cabi.ZipContext(i.z.num_vars, i.z.perm1, i.z.perm2)
    if T is not None:
        ctx.set_proximity_tests(T)
    return ctx


@pytest.mark.parametrize("T", [2, 3, 8])
@pytest.mark.parametrize("num_vars", SIZES)
def test_open_on_a_plain_handle(cabi, num_vars, T):
    i = px.instance(num_vars, T, n_cols=N_COLS)
    ctx = _ctx(cabi, i, T)
    assert ctx.proximity_tests == T and ctx.proof_len(N_COLS, i.fl) == i.proof.size
    com, roots = ctx.commit(i.evals)
    assert np.array_equal(roots, i.roots)
    proof = com.open(i.evals, i.coeffs, i.cols, i.q0, cabi.make_field(i.modulus, i.fl))
    assert np.array_equal(proof[: i.u_bytes], i.proof[: i.u_bytes]), "proximity rows"
    assert np.array_equal(proof, i.proof)


@pytest.mark.parametrize("num_vars,T", [(9, 2), (9, 8), (18, 3), (18, 8)])
def test_commit_open_unpacked_and_packed(cabi, num_vars, T):
    """cw 64 stores everything; cw 1024 takes the hinted, packed commit."""
    i = px.instance(num_vars, T, n_cols=N_COLS)
    proof, roots, _ = _ctx(cabi, i, T).commit_open(i.evals, i.coeffs, i.cols, i.q0, cabi.make_field(i.modulus, i.fl))
    assert np.array_equal(roots, i.roots)
    assert np.array_equal(proof, i.proof)


@pytest.mark.parametrize("T", [2, 8])
def test_open_stream_one_column_per_group(cabi, T):
    i = px.instance(13, T, n_cols=N_COLS)
    ctx = _ctx(cabi, i, T)
    com, _ = ctx.commit(i.evals)
    pieces = []
    com.open_stream(i.evals, i.coeffs, i.cols, i.q0, cabi.make_field(i.modulus, i.fl),
                    lambda mv: pieces.append(bytes(mv)) and None, chunk_bytes=1)
    assert len(pieces[0]) == i.u_bytes, "the first piece carries all T proximity rows"
    assert [len(p) for p in pieces[1:-1]] == [i.col_bytes] * N_COLS
    assert np.array_equal(np.frombuffer(b"".join(pieces), dtype=np.uint8), i.proof)


@pytest.mark.parametrize("num_vars,T", [(9, 3), (16, 2), (16, 8)])
def test_open_testing_alone(cabi, num_vars, T):
    i = px.instance(num_vars, T, n_cols=N_COLS)
    u = _ctx(cabi, i, T).open_testing(i.evals, i.coeffs)
    assert u.shape == (T, i.C, 8)
    assert np.array_equal(u.view(np.uint8).reshape(-1), i.proof[: i.u_bytes])


def test_two_jobs_in_flight(cabi):
    torch = pytest.importorskip("torch")
    T = 3
    a, b = px.instance(13, T, n_cols=N_COLS), px.instance(13, T, n_cols=N_COLS, seed=7)
    ctx = _ctx(cabi, a, T)
    zf = cabi.make_field(a.modulus, a.fl)
    ev = [torch.from_numpy(np.array(x.evals)).cuda() for x in (a, b)]
    out = [torch.empty(a.proof.size, dtype=torch.uint8, device="cuda") for _ in range(2)]
    jobs = [ctx.commit_open_begin(ev[k], x.coeffs, x.cols, x.q0, zf, out[k]) for k, x in enumerate((a, b))]
    for k, x in enumerate((a, b)):
        roots = jobs[k].wait(want_roots=True)
        assert np.array_equal(roots, x.roots)
        assert np.array_equal(out[k].cpu().numpy(), x.proof), k


@pytest.mark.parametrize("modulus,fl", [(px.TEST_MODULUS_2, 2), (px.MOD_3LIMB, 3), (px.BENCH_MODULUS, 4)])
def test_field_width_does_not_matter_to_the_new_pass(cabi, modulus, fl):
    i = px.instance(9, 3, modulus, fl, n_cols=N_COLS)
    com, _ = (ctx := _ctx(cabi, i, 3)).commit(i.evals)
    assert ctx.proof_len(N_COLS, fl) == i.proof.size
    assert np.array_equal(com.open(i.evals, i.coeffs, i.cols, i.q0, cabi.make_field(modulus, fl)), i.proof)


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.mark.parametrize("kind", ["min", "max", "mixed"])
def test_accumulator_bound_at_2pow16(cabi, kind):
    """Every coefficient of every test and every witness entry at the ends of i64: |u'| reaches 256 * 2^126, the most
    the 192-bit partial sums are asked to hold.  Compared with Python integers."""
    nv, T = 16, 8
    R = C = 256
    if kind == "mixed":
        rng = np.random.default_rng(3)
        evals = np.where(rng.integers(0, 2, size=R * C) == 1, INT64_MIN, INT64_MAX).astype(np.int64)
        coeffs = np.where(rng.integers(0, 2, size=(T, R)) == 1, INT64_MIN, INT64_MAX).astype(np.int64)
    else:
        v = INT64_MIN if kind == "min" else INT64_MAX
        evals = np.full(R * C, v, dtype=np.int64)
        coeffs = np.full((T, R), v, dtype=np.int64)
    ctx = cabi.ZipContext(nv, orc.shuffle_perm(1, 2 * C), orc.shuffle_perm(2, 2 * C))
    ctx.set_proximity_tests(T)
    u = ctx.open_testing(evals, coeffs)
    for t in range(T):
        want = px.combine_int(coeffs[t], evals, R, C)
        got = [orc.limbs_to_int(u[t, c], signed=True) for c in range(C)]
        assert got == want, (kind, t)


def _profiled_open(cabi, i, ctx):
    com, _ = ctx.commit(i.evals)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.profile_read()
    proof = com.open(i.evals, i.coeffs, i.cols, i.q0, cabi.make_field(i.modulus, i.fl))
    launches = {name: n for name, (n, _ms) in ctx.profile_read().items()}
    ctx.set_profiling(False)
    return proof, launches


def test_one_test_launches_what_it_launched_before(cabi):
    """set_proximity_tests(1) changes nothing: the same bytes and the same launches as a ctx that never called it; with
    T in {2, 8} exactly one launch of the new pass is added (and one fold per further test)."""
    one = px.instance(13, 1, n_cols=N_COLS)
    proof0, base = _profiled_open(cabi, one, _ctx(cabi, one))
    proof1, same = _profiled_open(cabi, one, _ctx(cabi, one, 1))
    assert np.array_equal(proof0, one.proof) and np.array_equal(proof1, proof0)
    assert same == base and NEW_PASS not in base and base["combine_finalize_kernel"] == 1
    for T in (2, 8):
        i = px.instance(13, T, n_cols=N_COLS)
        proof, got = _profiled_open(cabi, i, _ctx(cabi, i, T))
        assert np.array_equal(proof, i.proof)
        want = dict(base)
        want[NEW_PASS] = 1
        want["combine_finalize_kernel"] += T - 1
        assert got == want, T


# ---- usage errors ------------------------------------------------------------------------------------------------------
def test_setter_ranges(cabi):
    i = px.instance(9, 1, n_cols=N_COLS)
    ctx = _ctx(cabi, i)
    assert ctx.proximity_tests == 1
    for bad in (0, 9, 1000):
        with pytest.raises(cabi.ZipError) as e:
            ctx.set_proximity_tests(bad)
        assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED and "1 .. 8" in str(e.value)
        assert ctx.proximity_tests == 1
    for ok in (8, 1, 2):
        ctx.set_proximity_tests(ok)
        assert ctx.proximity_tests == ok


def test_row_sharded_ctx_stays_a_one_test_ctx(cabi):
    i = px.instance(9, 1, n_cols=N_COLS)
    shard = cabi.ZipContext(9, i.z.perm1, i.z.perm2, row_begin=4, row_count=8)
    shard.set_proximity_tests(1)
    with pytest.raises(cabi.ZipError) as e:
        shard.set_proximity_tests(2)
    assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED and shard.proximity_tests == 1


def test_one_test_paths_refuse_without_a_launch(cabi):
    torch = pytest.importorskip("torch")
    i = px.instance(9, 2, n_cols=N_COLS)
    ctx = _ctx(cabi, i)
    zf = cabi.make_field(i.modulus, i.fl)
    batch = ctx.batch_commit(np.stack([i.evals, i.evals]))
    com, _ = ctx.commit(i.evals)
    ev_d = torch.from_numpy(np.array(i.evals)).cuda()
    up, rp = (torch.zeros(i.C * n, dtype=torch.int64, device="cuda") for n in (8, i.fl))
    wire = torch.zeros(N_COLS * i.col_bytes, dtype=torch.uint8, device="cuda")
    ctx.set_proximity_tests(2)
    ctx.synchronize()
    ctx.set_profiling(True)
    ctx.profile_read()
    calls = cabi.batch_verify_calls()
    two = lambda a: np.stack([a, a])
    refused = [
        lambda: batch.open(two(i.coeffs[0]), two(i.cols), two(i.q0), zf),
        lambda: ctx.batch_verify(two(i.roots), np.concatenate([i.proof, i.proof]), two(i.coeffs[0]), two(i.cols), two(i.q0),
                                 two(i.q1), two(np.array(orc.int_to_limbs(i.ev, i.fl), dtype=np.uint64)), zf),
        lambda: com.open_shard(ev_d, i.coeffs[0], i.cols, i.q0, zf, up, rp, wire),
    ]
    for call in refused:
        with pytest.raises(cabi.ZipError) as e:
            call()
        assert e.value.code == cabi.ZIP_ERR_UNSUPPORTED
    assert ctx.profile_read() == {} and cabi.batch_verify_calls() == calls
