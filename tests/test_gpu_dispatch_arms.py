"""GPU: the template instances that a public entry point can select but no other test ran (tests/_dispatch_arms.py is
the inventory; tests/test_dispatch_census.py holds it to the dispatchers).  Everything is bit-exact against the CPU
oracle or Python integers: there are no tolerances here.  Needs a real MI355X.

  (a) 4 .. 7 proximity tests: combine_rows_extra_kernel<3..6>, verify_extra_tests_kernel with 3 .. 6 tests
  (b) moduli 2^128 - 159 and 2^192 - 237 (top bit set, 2^(64 FL) - q fits a limb) on the one-polynomial paths: the QUIRK
      instances of combine_rows_kernel<2|3>, field_map_i64_kernel<2|3> with quirk_mod, field_from_int256 on zip_verify
  (c) sumcheck_round_kernel<FL, K, DEG> for every K, DEG in 1..4 and sumcheck_round_quad_kernel for DEG 2, 3
  (d) merkle_leaves_kernel<1..8> and every first pass of merkle_upper_levels
  (f) sum_partials_kernel<2|3|4>: the 512-bit carries and the modular add's carry out of the top limb; three row shards
      with a 3-limb field and with a 4-limb quirk modulus
((e), open_columns_ilv_scalar_kernel<2, 14>, is two more cases of tests/test_gpu_gather_walk.py.)"""
import functools

import numpy as np
import pytest

import _ccs
import _ccs_random
import _oracle as orc
import _proximity as px
from test_gpu_sumcheck import _tables
from test_gpu_sumcheck_onecall import _assert_state_equal, _state_of

pytestmark = pytest.mark.gpu

N_COLS = 8
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
MOD_NO_SPARE = (1 << 256) - 189
Q128_QUIRK = (1 << 128) - 159  # 2 limbs, quirk_mod 159
Q192_QUIRK = (1 << 192) - 237  # 3 limbs, quirk_mod 237
QUIRK_FIELDS = [(Q128_QUIRK, 2), (Q192_QUIRK, 3)]


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _ctx(cabi, z, T=None):
    ctx = cabi.ZipContext(z.num_vars, z.perm1, z.perm2, geometry_override=(z.row_len, z.num_rows, z.codeword_len))
    if T is not None:
        ctx.set_proximity_tests(T)
    return ctx


def _ev_limbs(i):
    return np.array(orc.int_to_limbs(i.ev, i.fl), dtype=np.uint64)


# ------------------------------------------------------------------------------------------- (a) 4 .. 7 proximity tests
@pytest.mark.parametrize("T", [4, 5, 6, 7])
@pytest.mark.parametrize("num_vars", [13, 16])
def test_open_with_four_to_seven_proximity_tests(cabi, num_vars, T):
    """2^13: two rows per chunk, the remainder loop of combine_rows_extra_kernel<T - 1> only; 2^16: eight rows per chunk
    (two unrolled passes) and a full workgroup of 256 columns."""
    i = px.instance(num_vars, T, n_cols=N_COLS)
    ctx = _ctx(cabi, i.z, T)
    assert ctx.proximity_tests == T and ctx.proof_len(N_COLS, i.fl) == i.proof.size
    com, roots = ctx.commit(i.evals)
    assert np.array_equal(roots, i.roots)
    proof = com.open(i.evals, i.coeffs, i.cols, i.q0, cabi.make_field(i.modulus, i.fl))
    assert np.array_equal(proof[: i.u_bytes], i.proof[: i.u_bytes]), "proximity rows"
    assert np.array_equal(proof, i.proof)


@functools.lru_cache(maxsize=None)
def _bound_case(kind):
    """The construction of test_gpu_proximity_open.py::test_accumulator_bound_at_2pow16 for seven tests: (evals,
    coeffs [7, R], u'_t in Python integers); T tests take the first T coefficient vectors."""
    R = C = 256
    if kind == "mixed":
        rng = np.random.default_rng(3)
        evals = np.where(rng.integers(0, 2, size=R * C) == 1, INT64_MIN, INT64_MAX).astype(np.int64)
        coeffs = np.where(rng.integers(0, 2, size=(7, R)) == 1, INT64_MIN, INT64_MAX).astype(np.int64)
    else:
        v = INT64_MIN if kind == "min" else INT64_MAX
        evals = np.full(R * C, v, dtype=np.int64)
        coeffs = np.full((7, R), v, dtype=np.int64)
    return evals, coeffs, [px.combine_int(coeffs[t], evals, R, C) for t in range(7)]


@pytest.mark.parametrize("kind", ["min", "max", "mixed"])
@pytest.mark.parametrize("T", [4, 5, 6, 7])
def test_open_testing_at_the_accumulator_bound(cabi, T, kind):
    """Every coefficient and every witness entry at the ends of i64: |u'| reaches 256 * 2^126, the most the 192-bit
    partial sums of combine_rows_extra_kernel<T - 1> are asked to hold."""
    C = 256
    evals, coeffs, want = _bound_case(kind)
    ctx = cabi.ZipContext(16, orc.shuffle_perm(1, 2 * C), orc.shuffle_perm(2, 2 * C))
    ctx.set_proximity_tests(T)
    u = ctx.open_testing(evals, np.ascontiguousarray(coeffs[:T]))
    assert u.shape == (T, C, 8)
    for t in range(T):
        assert [orc.limbs_to_int(u[t, c], signed=True) for c in range(C)] == want[t], (kind, t)


@pytest.mark.parametrize("T", [4, 5, 6, 7])
def test_verify_with_four_to_seven_proximity_tests(cabi, T):
    """zip_verify on a ctx set to T gives the oracle's honest proof and the same stream with one bit flipped in
    u'_{T-1} the verdicts the oracle's verifier gives (verify_z.rs:66-103): accepted; rejected, at the first opened column
    whose entry of the re-encoded row moved."""
    i = px.instance(13, T, n_cols=N_COLS)
    ctx = _ctx(cabi, i.z, T)
    zf, ev = cabi.make_field(i.modulus, i.fl), _ev_limbs(i)
    assert i.z.verify(i.f, i.roots, i.point, i.ev, i.proof) == 0
    rep = ctx.verify(i.roots, i.proof, i.coeffs, i.cols, i.q0, i.q1, ev, zf)
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    bad = i.proof.copy()
    bad[(T - 1) * i.C * 64 + 64 * (i.C - 1) + 9] ^= 1  # (test_gpu_proximity_verify.py: "bit in u'_{T-1} only")
    assert i.z.verify(i.f, i.roots, i.point, i.ev, bad) == orc.ORC_ERR_PROOF
    enc = []
    for p in (i.proof, bad):
        limbs = np.array([orc.int_to_limbs(x, 8) for x in px.u_primes(p, i.z, T)[T - 1]], dtype=np.uint64)
        rc, e = i.z.encode_row(limbs, in_limbs=8, out_limbs=8)
        assert rc == 0
        enc.append(e)
    moved = [k for k in range(N_COLS) if not np.array_equal(enc[0][i.cols[k]], enc[1][i.cols[k]])]
    assert moved, "the flipped position reaches none of the opened columns"
    rep = ctx.verify(i.roots, bad, i.coeffs, i.cols, i.q0, i.q1, ev, zf)
    assert rep == {"verdict": cabi.VERIFY_PROXIMITY_TESTING, "column": moved[0], "bad_merkle_paths": 0, "malformed_paths": 0}


# ------------------------------------------------------------------- (b) quirk moduli at 2 and 3 limbs, one polynomial
@functools.lru_cache(maxsize=None)
def _quirk_instance(modulus, fl, num_vars):
    """An honest oracle commit + open (one proximity test) whose witness has entries of both signs beyond quirk_mod and
    the ends of i64: splitmix64 with the first four entries replaced."""
    evals = orc.splitmix64(0x51524B + num_vars, 1 << num_vars).copy()
    evals[:4] = np.array([INT64_MIN, INT64_MAX, -1, 0], dtype=np.int64)
    quirk_mod = (1 << (64 * fl)) - modulus
    assert 0 < quirk_mod < 1 << 64 and (evals[4:] >= quirk_mod).any() and (evals[4:] <= -quirk_mod).any()
    i = px.make(num_vars, 1, modulus, fl, n_cols=N_COLS, evals=evals)
    # the modulus does have the quirk: map_to_field(i64::MAX) is (i64::MAX mod quirk_mod), not i64::MAX
    assert orc.field_from_i64(i.f, INT64_MAX) == (INT64_MAX % quirk_mod << (64 * fl)) % modulus != (INT64_MAX << (64 * fl)) % modulus
    for a in (i.evals, i.proof):
        a.setflags(write=False)
    return i


def _row_be(row):
    """write_field_element of every entry (pcs_transcript.rs:107-113): big-endian bytes of the Montgomery value"""
    return np.ascontiguousarray(row[:, ::-1].astype(">u8")).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("modulus,fl", QUIRK_FIELDS)
@pytest.mark.parametrize("num_vars", [8, 9])
def test_quirk_open_eval_alone(cabi, num_vars, modulus, fl):
    """zip_open_eval: combine_rows_kernel<FL, false, true, /*QUIRK*/true>"""
    i = _quirk_instance(modulus, fl, num_vars)
    row = _ctx(cabi, i.z).open_eval(i.evals, i.q0, cabi.make_field(modulus, fl))
    assert np.array_equal(row, i.z.combine_rows_field(i.f, i.q0, i.evals))


@pytest.mark.parametrize("modulus,fl", QUIRK_FIELDS)
@pytest.mark.parametrize("num_vars", [8, 9])
def test_quirk_open_runs_both_row_combinations(cabi, num_vars, modulus, fl):
    """zip_open: combine_rows_kernel<FL, true, true, /*QUIRK*/true> -- one pass, the field half seeing |w| mod quirk_mod,
    the integer half the entry as it is."""
    i = _quirk_instance(modulus, fl, num_vars)
    ctx = _ctx(cabi, i.z)
    zf = cabi.make_field(modulus, fl)
    com, roots = ctx.commit(i.evals)
    assert np.array_equal(roots, i.roots)
    proof = com.open(i.evals, i.coeffs[0], i.cols, i.q0, zf)
    rc, u = i.z.combine_rows_int(i.coeffs[0], i.evals)
    assert rc == 0
    assert np.array_equal(proof[: i.u_bytes], np.ascontiguousarray(u.astype("<u8")).view(np.uint8).reshape(-1)), "u'"
    assert np.array_equal(proof[proof.size - i.C * 8 * fl:], _row_be(i.z.combine_rows_field(i.f, i.q0, i.evals))), "evaluation row"
    assert np.array_equal(proof, i.proof)
    u_alone = ctx.open_testing(i.evals, i.coeffs[0])
    assert np.array_equal(u_alone, u)


@pytest.mark.parametrize("modulus,fl", QUIRK_FIELDS)
def test_quirk_proof_mle_eval_and_verdict(cabi, modulus, fl):
    """zip_open and zip_commit_open write the oracle's proof, zip_mle_eval gives the oracle's evaluation, and zip_verify
    gives that proof the oracle verifier's verdict -- which is a rejection, as for 2^256 - 189 in
    test_gpu_verify.py::test_verify_agrees_with_the_oracle_on_honest_proofs.  The witness entries are Int<1>: their FieldMap
    takes `modulus: F::I` (field.rs:557-559), an Int<FL> that is negative when q has its top bit set, and `%=` then
    reduces |w| by 2^(64 FL) - q.  The column entries are Int<4>, wider than the field: field.rs:550-555 widens the modulus
    to an Int<4> with zero limbs on top (biginteger.rs:824-834), which is positive, and `%=` reduces honestly.  So the
    evaluation row is not the q_0 combination of the mapped column entries, and verify_proximity_q_0
    (verify_z.rs:165-188) fails; the proximity test, the paths and the evaluation-consistency check
    (both sides take the Int<1> map) pass before it."""
    i = _quirk_instance(modulus, fl, 9)
    ctx = _ctx(cabi, i.z)
    zf = cabi.make_field(modulus, fl)
    com, roots = ctx.commit(i.evals)
    assert np.array_equal(roots, i.roots)
    assert np.array_equal(com.open(i.evals, i.coeffs[0], i.cols, i.q0, zf), i.proof)
    proof, roots, _ = _ctx(cabi, i.z).commit_open(i.evals, i.coeffs[0], i.cols, i.q0, zf)
    assert np.array_equal(roots, i.roots) and np.array_equal(proof, i.proof)
    assert orc.limbs_to_int(ctx.mle_eval(i.evals, i.q0, i.q1, zf)) == i.ev
    orc_rc = i.z.verify(i.f, i.roots, i.point, i.ev, i.proof)
    rep = ctx.verify(i.roots, i.proof, i.coeffs[0], i.cols, i.q0, i.q1, _ev_limbs(i), zf)
    assert (orc_rc == 0) == (rep["verdict"] == cabi.VERIFY_ACCEPT), (orc_rc, rep)
    assert orc_rc == orc.ORC_ERR_PROOF
    assert rep["verdict"] == cabi.VERIFY_PROXIMITY_Q0 and rep["bad_merkle_paths"] == 0 and rep["malformed_paths"] == 0


_CCS_INSTANCES = {
    "random6": lambda: _ccs_random.instances(6, 7, _ccs_random.witnesses(6, 1))[0],  # INT64_MIN among matrix values and z
    "vitalik": lambda: _ccs.vitalik_ccs(3),
}


@pytest.mark.parametrize("modulus,fl", QUIRK_FIELDS)
@pytest.mark.parametrize("name", sorted(_CCS_INSTANCES))
def test_quirk_ccs_tables_equal_the_oracle(cabi, name, modulus, fl):
    """A single zip_ccs: z_ccs in F_q (field_map_i64_kernel<FL> with quirk_mod), M_k z (field_from_i64 on the matrix
    values), eq(), the second sumcheck's table, V_s and mle[M_k](r_x, r_y) -- the comparisons of
    test_gpu_spartan.py::test_ccs_tables_equal_the_oracle and ::test_matrix_mles_at_a_point_equal_the_oracle."""
    inst = _CCS_INSTANCES[name]()
    if name == "random6":
        assert _ccs_random.features(inst.matrices)["specials"] and INT64_MIN in inst.z
    f = orc.make_field(modulus, fl)
    o = orc.Ccs(inst)
    d = cabi.Ccs(inst.matrices, inst.s, cabi.make_field(modulus, fl))
    d.set_z(inst.z)
    zf = d.download(cabi.CCS_Z_FIELD)
    for k in range(inst.m):
        want = orc.field_from_i64(f, int(inst.z[k])) if k < len(inst.z) else 0
        assert orc.limbs_to_int(zf[k]) == want, k
    mz_o = o.mz(f)
    for k in range(inst.t):
        assert np.array_equal(d.download(cabi.CCS_MZ, k), mz_o[k]), k
    rng = np.random.default_rng(inst.s)
    r = orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=inst.s)], fl)
    ry = orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=inst.s)], fl)
    gamma = orc.field_elems([orc.field_from_i64(f, 0x1234567890ABCDEF)], fl)[0]
    eq_o = orc.build_eq_x_r(f, r)
    d.eq_table(r, 0)
    assert np.array_equal(d.download(cabi.CCS_EQ, 0), eq_o)
    vs = d.second_table(r, gamma)
    assert np.array_equal(d.download(cabi.CCS_EQ, 1), eq_o)
    assert np.array_equal(d.download(cabi.CCS_SECOND), o.second_table(f, eq_o, gamma))
    R_inv = pow(1 << (64 * fl), -1, modulus)
    for k in range(inst.t):  # V_s[k] = <Mz_k, eq(r_x)>, in Python integers (Montgomery: a*b*R^-1)
        acc = sum(orc.limbs_to_int(a) * orc.limbs_to_int(b) for a, b in zip(mz_o[k], eq_o)) * R_inv % modulus
        assert orc.limbs_to_int(vs[k]) == acc, k
    assert np.array_equal(d.eval_matrices(r, ry), o.eval_matrices(f, r, ry))
    d.free()


# ------------------------------------------------------------------------------------------- (c) sumcheck K x degree
SUMCHECK_FIELDS = [(TEST_MODULUS_2, 2), (MOD_3LIMB, 3), (MOD_NO_SPARE, 4)]
SUMCHECK_NV = 10  # round 1: 512 points = two workgroups of the one-thread kernel; nine folding rounds follow


@functools.lru_cache(maxsize=None)
def _sumcheck_tables(modulus, fl, K):
    t = _tables(orc.make_field(modulus, fl), fl, modulus, K, SUMCHECK_NV, seed=SUMCHECK_NV * 7 + K)
    t.setflags(write=False)
    return t


def _prove_on_the_round_kernels(cabi, monkeypatch, quad, modulus, fl, K, degree):
    """zip_sumcheck_prove with every round on the round kernels (no tail kernel): messages, challenges and the
    transcript afterwards against orc.sumcheck_prove_product from the same primed transcript."""
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_QUAD", quad)
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_TAIL", "0")
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_GRID", raising=False)
    mles = _sumcheck_tables(modulus, fl, K)
    to = orc.new_transcript()
    orc.absorb(to, b"dispatch-arms")
    state = _state_of(cabi, to)
    msgs_o, rand_o = orc.sumcheck_prove_product(orc.make_field(modulus, fl), mles, degree, to)
    sc = cabi.Sumcheck(mles, SUMCHECK_NV, degree, cabi.make_field(modulus, fl))
    rounds0, tails0 = cabi.sumcheck_launch_counts()
    msgs, rand = sc.prove(state)
    rounds1, tails1 = cabi.sumcheck_launch_counts()
    sc.free()
    assert (rounds1 - rounds0, tails1 - tails0) == (SUMCHECK_NV, 0), "every round through the round kernels"
    for rnd in range(SUMCHECK_NV):
        assert np.array_equal(msgs[rnd], msgs_o[rnd]), f"message of round {rnd + 1}"
        assert np.array_equal(rand[rnd], rand_o[rnd]), f"challenge of round {rnd + 1}"
    _assert_state_equal(state, to)


@pytest.mark.parametrize("modulus,fl", SUMCHECK_FIELDS)
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sumcheck_one_thread_arms(cabi, monkeypatch, K, degree, modulus, fl):
    """sumcheck_round_kernel<FL, K, degree> in every round (ZIP_HIP_SUMCHECK_QUAD=0)"""
    _prove_on_the_round_kernels(cabi, monkeypatch, "0", modulus, fl, K, degree)


@pytest.mark.parametrize("modulus,fl", SUMCHECK_FIELDS)
@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sumcheck_quad_arms(cabi, monkeypatch, K, degree, modulus, fl):
    """sumcheck_round_quad_kernel<FL, K, degree> in every round, the first included (ZIP_HIP_SUMCHECK_QUAD=2)"""
    _prove_on_the_round_kernels(cabi, monkeypatch, "2", modulus, fl, K, degree)


# ------------------------------------------------------------------------------------------- (d) stand-alone Merkle trees
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 5, 7, 9])
@pytest.mark.parametrize("limbs", [1, 2, 3, 4, 5, 6, 7, 8])
def test_merkle_trees_every_leaf_width_and_split(cabi, limbs, depth):
    """merkle_leaves_kernel<limbs>, then merkle_upper_levels from level 0: depth 1 / 2 / 3 are one launch_upper<1> / <2> /
    <3>, 5 = 4 + 1, 7 = 4 + 3, 9 = 4 + 4 + 1, 0 copies the leaf hashes.  Five trees of 2^depth <= 32 leaves leave the
    last workgroup of the leaf grid partly idle."""
    rng = np.random.default_rng(100 * limbs + depth)
    for num_trees in (1, 5):
        leaves = rng.integers(0, 2**64, size=(num_trees, 1 << depth, limbs), dtype=np.uint64)
        got = cabi.merkle_trees(leaves, depth)
        assert got.shape == (num_trees, (2 << depth) - 1, 32)
        for t in range(num_trees):
            assert np.array_equal(got[t], orc.merkle_tree(depth, leaves[t])), (num_trees, t)


# ------------------------------------------------------------------------------------------- (f) the row-sharded fold
SUM_ROW_LEN = 512  # two workgroups of sum_partials_kernel
INT8_MAX = (1 << 511) - 1


@functools.lru_cache(maxsize=None)
def _u_parts(G):
    """[G][512] 512-bit two's-complement parts as Python integers and their column sums mod 2^512"""
    rng = np.random.default_rng(7 + G)
    parts = [[0] * SUM_ROW_LEN for _ in range(G)]
    for c in range(SUM_ROW_LEN):
        for g in range(G):
            if c == 0:
                v = (-1, 1)[g] if g < 2 else 0              # -1 + 1: a carry through all eight limbs and out
            elif c == 1:
                v = (INT8_MAX, 1)[g] if g < 2 else 0        # the largest positive + 1: a carry into the top limb's sign bit
            elif c == 2:
                v = -1                                       # every limb sums to G * (2^64 - 1): carries of G - 1
            elif c == 3:
                v = ((1 << 64) - 1, 1)[g] if g < 2 else -1  # a carry out of the low limb only, then borrows
            else:
                v = int.from_bytes(rng.bytes(63), "little") * (1 if rng.integers(0, 2) else -1)
            parts[g][c] = v
    sums = [sum(parts[g][c] for g in range(G)) & ((1 << 512) - 1) for c in range(SUM_ROW_LEN)]
    return parts, sums


def _limb_array(values, limbs):
    return np.array([[orc.int_to_limbs(v, limbs) for v in row] for row in values], dtype=np.uint64)


@pytest.fixture(scope="module")
def sum_ctx(cabi):
    return cabi.ZipContext(18, orc.shuffle_perm(1, 2 * SUM_ROW_LEN), orc.shuffle_perm(2, 2 * SUM_ROW_LEN))


@pytest.mark.parametrize("G", [1, 3, 4])
def test_sum_partials_integer_halves(cabi, sum_ctx, G):
    torch = pytest.importorskip("torch")
    assert sum_ctx.row_len == SUM_ROW_LEN
    parts, sums = _u_parts(G)
    uparts = torch.from_numpy(_limb_array(parts, 8).view(np.int64)).cuda()
    u_out = torch.full((SUM_ROW_LEN, 8), 0x55, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sum_ctx.sum_partials(uparts, None, G, None, u_out, None)
    sum_ctx.synchronize()
    got = u_out.cpu().numpy().view(np.uint64)
    for c in range(SUM_ROW_LEN):
        assert orc.limbs_to_int(got[c]) == sums[c], c


@pytest.mark.parametrize("modulus,fl", [(MOD_3LIMB, 3), (MOD_NO_SPARE, 4), (Q128_QUIRK, 2)])
@pytest.mark.parametrize("G", [1, 3, 4])
def test_sum_partials_field_halves(cabi, sum_ctx, G, modulus, fl):
    """sum_partials_kernel<FL>: canonical residues in, the canonical sum out.  The first columns hold q - 1 in every
    part; without a spare bit (2^256 - 189, 2^128 - 159) q - 1 + q - 1 carries out of the top limb.  The integer halves
    ride along, as they do in zip_mctx."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(fl * 10 + G)
    res = [[modulus - 1 if c < 8 else int.from_bytes(rng.bytes(40), "little") % modulus for c in range(SUM_ROW_LEN)] for _ in range(G)]
    res[0][8] = 0
    if G > 1:
        res[0][9], res[1][9] = modulus - 1, 1  # the sum is q itself
    parts, sums = _u_parts(G)
    uparts = torch.from_numpy(_limb_array(parts, 8).view(np.int64)).cuda()
    fparts = torch.from_numpy(_limb_array(res, fl).view(np.int64)).cuda()
    u_out = torch.full((SUM_ROW_LEN, 8), 0x55, dtype=torch.int64, device="cuda")
    r_out = torch.full((SUM_ROW_LEN, fl), 0x55, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sum_ctx.sum_partials(uparts, fparts, G, cabi.make_field(modulus, fl), u_out, r_out)
    sum_ctx.synchronize()
    got_r, got_u = r_out.cpu().numpy().view(np.uint64), u_out.cpu().numpy().view(np.uint64)
    for c in range(SUM_ROW_LEN):
        assert orc.limbs_to_int(got_r[c]) == sum(res[g][c] for g in range(G)) % modulus, c
        assert orc.limbs_to_int(got_u[c]) == sums[c], c


@pytest.mark.parametrize("modulus,fl", [(MOD_3LIMB, 3), (MOD_NO_SPARE, 4)])
def test_three_shards_on_one_device(cabi, modulus, fl):
    """ZipMultiContext, 64 rows over three shards (uneven blocks) on device 0: sum_partials_kernel<3>, and with
    2^256 - 189 the QUIRK instance of combine_rows_kernel on every shard and the fold's carry branch.  Roots and proof
    equal the oracle's unsharded ones (the pattern of test_gpu_parity.py::test_multi_device_context_proof_equals_unsharded)."""
    num_vars = 12
    z = orc.Zip(num_vars)
    f = orc.make_field(modulus, fl)
    zf = cabi.make_field(modulus, fl)
    evals = orc.splitmix64(0x5A494E43 + 43, 1 << num_vars).copy()
    evals[:4] = np.array([INT64_MIN, INT64_MAX, -1, 0], dtype=np.int64)
    point = orc.point_to_field(f, np.arange(2, num_vars + 2, dtype=np.int64))
    rows_o, layers_o, roots_o = z.commit(evals)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point, orc.new_transcript())
    lr = z.num_rows.bit_length() - 1
    q0 = orc.build_eq_x_r(f, point[num_vars - lr:])
    m = cabi.ZipMultiContext(num_vars, z.perm1, z.perm2, [0, 0, 0])
    assert m.shards() == 3
    proof, roots = m.commit_open(evals, coeffs, cols, q0, zf)
    m.close()
    assert np.array_equal(roots, roots_o)
    bad = np.flatnonzero(proof != proof_o)
    assert bad.size == 0, f"{bad.size} proof bytes differ, first at {bad[:8]}"
