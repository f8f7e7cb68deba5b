"""The loops of the two-limb kernels that only real sizes enter, each at the smallest shape that enters it, bit-exact
against the CPU oracle at n_limbs = 2 or the Python-int model tests/_two_limb.py Instance.expect: no tolerances.
tests/test_two_limb_regimes_host.py holds that model to the oracle on the same shapes and tampers.  Needs a real MI355X.

Every test first asserts, from the device's compute-unit count and the host formula of zinc_amd/csrc/zip_hip.hip that
it mirrors below, that its shape does enter the regime on the device at hand; one that cannot fails.

The census (kernel, loop, what enters it, who does):

    tl_encode_rows_kernel<HASH>   row += gridDim.x                G < num_rows, G = min(num_rows, 4 CUs, scratch cap)
        G = 4 CUs       (13, (4, 2048, 8), 2)         test_commit_second_rows_of_a_workgroup, test_whole_proofs_over_second_rows
        G = scratch cap (21, (16384, 128, 65536), 4)  test_commit_under_the_scratch_cap_roots_and_openings
    tl_verify_columns_kernel<FL>  r += 256                        num_rows > 256
        (13, (4, 2048, 8), 2), FL 4 and 2             test_verifier_accepts_at_eight_rows_per_thread, test_verifier_reports_at_eight_rows_per_thread
    encode_row_kernel<16, false>  j in [j0, j1), j1 - j0 > 1      cw > 1024 (and 1024 x 136 bytes of dynamic LDS from cw 1024)
        cw 2048 (FL 4, 3), 4096, 65536                test_encode_wide_int16_accepts_the_honest_proof, test_encode_wide_int16_reports
    tl_combine_kernel<FL, ., .>   r += 4 gridDim.y                num_rows > 4 by, by = min(ceil(R / 4), 2048 / ceil(C / 64))
        (20, (1024, 1024, 2048), 2)                   test_open_testing_two_rows_per_thread, test_open_testing_at_its_bounds_two_rows_per_thread,
                                                      test_open_eval_two_rows_per_thread
    tl_open_columns_kernel        g += gridDim.x * 256            n_cols num_rows (depth + 2) > 64 CUs 256
        (16, (32, 2048, 64), 2), 300 openings         test_column_gather_grid_stride
"""
import functools

import numpy as np
import pytest

import _oracle as orc
import _two_limb as tl
from test_gpu_two_limb_parity import _check_commit, _committed, _open_all_ways, _q0, _same

pytestmark = pytest.mark.gpu

SECOND_ROWS = (13, (4, 2048, 8), 2)
SCRATCH_CAP = (21, (16384, 128, 65536), 4)
COMBINE = (20, (1024, 1024, 2048), 2)
GATHER = (16, (32, 2048, 64), 2)


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the host formulas, restated ------------------------------------------------------------------------------------
def _commit_grid(num_rows, cw, cus):
    """tl_commit, zip_hip.hip:3056-3057 -> (G, scratch cap): the workgroups of tl_encode_rows_kernel"""
    cap = (128 << 20) // (cw * 3 * 8)
    return max(1, min(num_rows, 4 * cus, cap)), cap


def _combine_row_blocks(num_rows, row_len):
    """tl_run_combine_fl, zip_hip.hip:3105-3106 -> gridDim.y of tl_combine_kernel; a thread strides by 4 gridDim.y rows"""
    bx = (row_len + 63) // 64
    return max(1, min((num_rows + 3) // 4, 2048 // min(bx, 2048)))


def _gather_threads(n_cols, num_rows, depth, cus):
    """tl_launch_open_columns, zip_hip.hip:3238-3239 -> (pieces, threads of the launch)"""
    total = n_cols * num_rows * (depth + 2)
    return total, 256 * min((total + 255) // 256, cus * 64)


def _encode_wide_shape(cw):
    """encode_shape<16, false>, zip_hip.hip:1710-1711 -> (threads, bytes of dynamic LDS, positions per thread);
    EncElem<16, false> is 17 limbs (kernels_verify.cuh:42-45)"""
    threads = (64 if cw < 64 else cw) if cw < 1024 else 1024
    return threads, threads * 17 * 8, (cw + threads - 1) // threads


def _verify(cabi, ctx, inst, proof, roots, ev):
    return ctx.verify(roots, proof, inst.coeffs, inst.cols, inst.q0, inst.q1, np.array(orc.int_to_limbs(ev, inst.fl), dtype=np.uint64),
                      cabi.make_field(inst.modulus, inst.fl))


def _accepts_the_honest_proof(cabi, inst):
    """both verifiers accept the same bytes, the oracle with its Merkle paths checked.  (The oracle's proof, not one the
    device made: what a test of the verifier's loops reports does not depend on the commit and open kernels.)"""
    ctx = inst.z.ctx(cabi)
    assert inst.z.verify(inst.f, inst.roots, inst.point, inst.ev, inst.proof, check_merkle=True) == 0
    rep = _verify(cabi, ctx, inst, inst.proof, inst.roots, inst.ev)
    assert rep == dict(verdict=cabi.VERIFY_ACCEPT, column=0, bad_merkle_paths=0, malformed_paths=0)


def _reports_equal_the_model(cabi, ctx, inst, cases):
    failures = []
    for name, mutate, claim in cases:
        proof, roots, ev = mutate(inst.proof, inst.roots, inst.ev)
        want = inst.expect(proof, roots, ev)
        for key, value in claim.items():
            assert want[key] == value, (name, want, claim)
        assert want["verdict"] != tl.ACCEPT, name
        got = _verify(cabi, ctx, inst, proof, roots, ev)
        if got != want:
            failures.append((name, got, want))
    assert not failures, failures
    # the ctx still accepts the honest proof afterwards
    assert _verify(cabi, ctx, inst, inst.proof, inst.roots, inst.ev)["verdict"] == cabi.VERIFY_ACCEPT


# ---- A: tl_encode_rows_kernel, a workgroup encodes a second row; G = 4 CUs ------------------------------------------
def _enters_second_rows(z):
    G, cap = _commit_grid(z.num_rows, z.codeword_len, _cus())
    assert G == 4 * _cus() < min(z.num_rows, cap), f"{G} workgroups for {z.num_rows} rows (cap {cap}): no workgroup takes a second row"


@pytest.mark.parametrize("kind", ["random", "max", "min"])
def test_commit_second_rows_of_a_workgroup(cabi, kind):
    """rows, tree layers and roots of both instances of the kernel (with and without leaf hashes): the t1 scratch row
    and the wave totals of a workgroup are reused by its second row"""
    num_vars, geometry, rep = SECOND_ROWS
    z, evals, rows_o, layers_o, roots_o = _committed(num_vars, kind, geometry, rep)
    assert (z.row_len, z.num_rows, z.codeword_len) == geometry
    _enters_second_rows(z)
    _check_commit(cabi, z, evals, rows_o, layers_o, roots_o)


def test_whole_proofs_over_second_rows(cabi):
    """zip_open, zip_commit_open, a hinted and an uploaded handle against the oracle's proof (4 MB)"""
    num_vars, geometry, rep = SECOND_ROWS
    committed = _committed(num_vars, "random", geometry, rep)
    _enters_second_rows(committed[0])
    _open_all_ways(cabi, *committed, tl.BENCH_MODULUS, 4)


# ---- B: tl_encode_rows_kernel, G = the scratch cap, 256 positions per thread ----------------------------------------
def test_commit_under_the_scratch_cap_roots_and_openings(cabi):
    """128 rows of cw 65536 by 85 workgroups: rows 85 .. 127 are second rows.  The 128 roots pin every entry and every
    leaf hash; 12 opened columns are compared besides.  The 512 MB row matrix stays on the device.  (Not cached: about
    1 GiB of oracle output, used here only.)"""
    num_vars, geometry, rep = SCRATCH_CAP
    z = tl.Zip2(num_vars, geometry=geometry, rep=rep)
    assert (z.row_len, z.num_rows, z.codeword_len) == geometry
    G, cap = _commit_grid(z.num_rows, z.codeword_len, _cus())
    assert G == cap < min(z.num_rows, 4 * _cus()), f"{G} workgroups for {z.num_rows} rows (cap {cap}): the scratch cap does not bind"
    assert (z.codeword_len + 255) // 256 == 256  # kernels_two_limb.cuh:153, positions per thread
    evals = tl.witness(z, "random")
    rows_o, layers_o, roots_o = z.commit(evals)
    f = orc.make_field(tl.BENCH_MODULUS, 4)
    proof_o, cols, _ = z.open(f, evals, rows_o, layers_o, tl.make_point(f, num_vars))
    del rows_o, layers_o
    assert cols.size == tl.N_COLS == 12
    com, roots = z.ctx(cabi).commit(evals)
    try:
        _same(roots, roots_o, "roots")
        _same(com.open_columns(cols), proof_o[z.row_len * 128: proof_o.size - z.row_len * 8 * 4], "zip_open_columns")
    finally:
        com.free()
        cabi.lib().zip_release_cached_memory()


# ---- C: tl_verify_columns_kernel, 8 rows per thread ------------------------------------------------------------------
_MANY_ROWS_IDS = [f"fl{s[2]}" for s in tl.REGIME_MANY_ROWS]


def _many_rows_instance(shape):
    inst = tl.regime_instance(*shape)
    # kernels_two_limb.cuh:523: thread t walks rows t, t + 256, ...; one workgroup of 256 per opening (zip_hip.hip:3412)
    assert inst.R // 256 == 8 and inst.R % 256 == 0
    return inst


@pytest.mark.parametrize("shape", tl.REGIME_MANY_ROWS, ids=_MANY_ROWS_IDS)
def test_verifier_accepts_at_eight_rows_per_thread(cabi, shape):
    _accepts_the_honest_proof(cabi, _many_rows_instance(shape))


@pytest.mark.parametrize("shape", tl.REGIME_MANY_ROWS, ids=_MANY_ROWS_IDS)
def test_verifier_reports_at_eight_rows_per_thread(cabi, shape):
    """the whole catalogue, the overflow, the tampers at rows 256, 1300 and 2047 that only a repeat iteration reads, and
    12 x 2048 entries that fill all 512 bits (the 704-bit integer sum and the field sum carry across the iterations)"""
    inst = _many_rows_instance(shape)
    _reports_equal_the_model(cabi, inst.z.ctx(cabi), inst, tl.many_rows_cases(inst))


# ---- D: encode_row_kernel<16, false>, 1024 threads, 139264 bytes of dynamic LDS, several positions per thread --------
def _wide_instance(shape):
    inst = tl.regime_instance(*shape)
    threads, lds, per = _encode_wide_shape(inst.cw)
    assert threads == 1024 and lds == 139264 > 65536 and per == inst.cw // 1024 >= 2
    return inst


_WIDE_IDS = [f"cw{s[3][2]}-fl{s[2]}" for s in tl.REGIME_WIDE_CODEWORDS]


@pytest.mark.parametrize("shape", tl.REGIME_WIDE_CODEWORDS, ids=_WIDE_IDS)
def test_encode_wide_int16_accepts_the_honest_proof(cabi, shape):
    _accepts_the_honest_proof(cabi, _wide_instance(shape))


@pytest.mark.parametrize("shape", tl.REGIME_WIDE_CODEWORDS, ids=_WIDE_IDS)
def test_encode_wide_int16_reports(cabi, shape):
    """u' bit 0 and bit 1023, 2^1022 at the last element (OVERFLOW, found by a thread that owns several positions) and
    2^1000 there (formed: PROXIMITY_TESTING), a value and an evaluation-row tamper"""
    inst = _wide_instance(shape)
    cases = tl.wide_codeword_cases(inst)
    assert [c[2]["verdict"] for c in cases if c[0].startswith("u' = 2^")] == [tl.OVERFLOW, tl.PROXIMITY_TESTING]
    assert tl.OVERFLOW == cabi.VERIFY_OVERFLOW
    _reports_equal_the_model(cabi, inst.z.ctx(cabi), inst, cases)


# ---- E: tl_combine_kernel, two rows per thread -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _combine_witness(kind):
    """(z, evals) at COMBINE, never committed (16 MB of witness)"""
    num_vars, geometry, rep = COMBINE
    z = tl.Zip2(num_vars, geometry=geometry, rep=rep)
    assert (z.row_len, z.num_rows, z.codeword_len) == geometry
    by = _combine_row_blocks(z.num_rows, z.row_len)
    assert z.num_rows == 2 * 4 * by, f"gridDim.y = {by} for {z.num_rows} rows: no thread takes a second row"
    evals = tl.witness(z, kind)
    evals.setflags(write=False)
    return z, evals


def test_open_testing_two_rows_per_thread(cabi):
    z, evals = _combine_witness("random")
    coeffs = tl.challenge_like(z.num_rows, 77)
    rc, expect = z.combine_rows_int(coeffs, evals)
    assert rc == 0
    _same(z.ctx(cabi).open_testing(evals, coeffs), expect, "u'")


@pytest.mark.parametrize("kind", ["max", "min", "lowtop"])
def test_open_testing_at_its_bounds_two_rows_per_thread(cabi, kind):
    """1024 products at +-2^254 of one sign per column: a thread's 320-bit accumulator leaves 256 bits with its second
    row, the folded sum reaches 2^264"""
    z, evals = _combine_witness(kind)
    ctx = z.ctx(cabi)
    for c in (tl.INT2_MIN, tl.INT2_MAX):
        coeffs = np.tile(tl.to_limbs([c]), (z.num_rows, 1))
        rc, expect = z.combine_rows_int(coeffs, evals)
        assert rc == 0
        if kind != "lowtop":
            assert abs(orc.limbs_to_int(expect[0], signed=True)) >= 1 << 263
        _same(ctx.open_testing(evals, coeffs), expect, "u'")


@pytest.mark.parametrize("modulus,fl", [(tl.BENCH_MODULUS, 4), (tl.MOD_3LIMB, 3), (tl.TEST_MODULUS_2, 2), (tl.MOD_QUIRK_2LIMB, 2)])
def test_open_eval_two_rows_per_thread(cabi, modulus, fl):
    z, evals = _combine_witness("random")
    f = orc.make_field(modulus, fl)
    q0 = _q0(z, modulus, fl, 20)
    _same(z.ctx(cabi).open_eval(evals, q0, cabi.make_field(modulus, fl)), z.combine_rows_field(f, q0, evals), "row")


# ---- F: tl_open_columns_kernel, the grid-stride loop ---------------------------------------------------------------
@pytest.mark.parametrize("handle", ["uploaded", "committed"])
def test_column_gather_grid_stride(cabi, handle):
    """more (opening, row, piece) triples than the capped grid has threads: 300 openings on 256 compute units, more on a
    larger device; duplicates among them.  zip_open_columns and the whole proof (155 MB) against the oracle's: from a
    handle that holds the oracle's own rows and trees (nothing but the gather between them and the stream), and from the
    handle zip_commit_open keeps (its 2048 rows are also second rows of the commit kernel on 256 compute units)"""
    num_vars, geometry, rep = GATHER
    row_len, num_rows, cw = geometry
    depth = cw.bit_length() - 1
    cus = _cus()
    # a sixth more pieces than threads; 300 where 256 compute units cap the grid at 4,194,304 threads
    n_cols = max(300, -(-(64 * cus * 256 * 7 // 6) // (num_rows * (depth + 2))))
    z, evals, rows_o, layers_o, roots_o = _committed(num_vars, "random", geometry, rep, n_cols)
    assert (z.row_len, z.num_rows, z.codeword_len, z.depth) == (row_len, num_rows, cw, depth)
    total, threads = _gather_threads(n_cols, z.num_rows, z.depth, cus)
    assert threads == 64 * cus * 256 < total, f"{total} pieces for {threads} threads: no thread takes a second piece"
    proof_o, cols, coeffs, q0 = _gather_proof(n_cols)
    assert cols.size == n_cols and len(set(cols.tolist())) < n_cols
    zf = cabi.make_field(tl.BENCH_MODULUS, 4)
    ctx = z.ctx(cabi)
    if handle == "uploaded":
        com = ctx.upload_commitment(rows_o, layers_o[:, :-1, :], roots_o)
        _same(com.open(evals, coeffs, cols, q0, zf), proof_o, "zip_open")
    else:
        proof, roots, com = ctx.commit_open(evals, coeffs, cols, q0, zf, keep=True)
        _same(roots, roots_o, "roots")
        _same(proof, proof_o, "zip_commit_open")
    _same(com.open_columns(cols), proof_o[z.row_len * 128: proof_o.size - z.row_len * 8 * 4], "zip_open_columns")
    com.free()


@functools.lru_cache(maxsize=None)
def _gather_proof(n_cols):
    """(proof, cols, coeffs, q0) of the oracle at GATHER, opened once"""
    num_vars, geometry, rep = GATHER
    z, evals, rows_o, layers_o, _ = _committed(num_vars, "random", geometry, rep, n_cols)
    f = orc.make_field(tl.BENCH_MODULUS, 4)
    point = tl.make_point(f, num_vars)
    proof_o, cols, coeffs = z.open(f, evals, rows_o, layers_o, point)
    proof_o.setflags(write=False)
    return proof_o, cols, coeffs, z.tensors(f, point)[0]
