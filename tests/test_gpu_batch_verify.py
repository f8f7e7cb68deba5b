"""GPU parity of the batched verifier (zip_batch_verify): many proofs of one geometry in one launch set, report for report
against zip_verify on each member's slices (which tests/test_gpu_verify*.py pin to the oracle) and against the tamper
catalogue and model of tests/_verify_cases.py (which tests/test_verify_cases_host.py confirms on the oracle).
Needs a real MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as orc
import _verify_cases as vc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189  # benches/spartan_benches.rs:134-137
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
ACCEPTED = {"verdict": vc.ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
SHORT = {"verdict": vc.MALFORMED, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
NEW_KERNELS = ("batch_encode_wide_kernel", "batch_encode_field_kernel", "batch_verify_columns_kernel",
               "batch_verify_report_kernel")


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _ctx(cabi, z, **kw):
    return cabi.ZipContext(z.num_vars, z.perm1, z.perm2, geometry_override=(z.row_len, z.num_rows, z.codeword_len), **kw)


def _witness(num_vars, seed, small):
    n = 1 << num_vars
    if small:
        return np.random.default_rng(seed).integers(-128, 128, size=n, dtype=np.int64)
    w = orc.splitmix64(0x5A494E43 + seed, n).copy()
    w[: min(n, 4)] = np.array([-(2**63), 2**63 - 1, -1, 0], dtype=np.int64)[: min(n, 4)]
    return w


class Batch:
    """B honest proofs on ONE shared transcript (the oracle's open, looped) with everything both verifiers take,
    polynomial-major.  Built once per shape and never modified."""

    def __init__(self, num_vars, modulus, fl, B=5):
        z = orc.Zip(num_vars)
        f = orc.make_field(modulus, fl)
        self.z, self.f, self.modulus, self.fl, self.B = z, f, modulus, fl, B
        rng = np.random.default_rng(3 + num_vars)
        lr = z.num_rows.bit_length() - 1
        fs = orc.new_transcript()
        roots, proofs, cols, coeffs, q0, q1, evs = [], [], [], [], [], [], []
        for i in range(B):
            ev = _witness(num_vars, seed=7 + 101 * i + 1, small=(fl == 2))
            pt_i = rng.integers(-100, 100, size=num_vars, dtype=np.int64)  # a different point per polynomial
            pt = orc.point_to_field(f, pt_i) if num_vars else np.zeros((0, fl), dtype=np.uint64)
            rows_o, layers_o, roots_o = z.commit(ev)
            proof, c, k = z.open(f, ev, rows_o, layers_o, pt, fs)
            roots.append(roots_o)
            proofs.append(proof)
            cols.append(c.copy())
            coeffs.append(k.copy())
            if lr:
                q0.append(orc.build_eq_x_r(f, pt[num_vars - lr:]))
            if num_vars - lr:
                q1.append(orc.build_eq_x_r(f, pt[: num_vars - lr]))
            evs.append(z.mle_eval(f, ev, pt))
        self.len = z.proof_len(fl)
        self.roots = np.stack(roots)
        self.proofs = np.concatenate(proofs)
        self.cols = np.stack(cols)
        self.coeffs = np.stack(coeffs) if lr else None
        self.q0 = np.stack(q0) if lr else None
        self.q1 = np.stack(q1) if num_vars - lr else None
        self.evs = list(evs)  # Montgomery values as Python ints
        for a in (self.roots, self.proofs, self.cols):
            a.setflags(write=False)

    def ev_limbs(self, evs=None):
        return np.array([orc.int_to_limbs(e, self.fl) for e in (self.evs if evs is None else evs)], dtype=np.uint64)

    def take(self, idx):
        """(roots, coeffs, cols, q0, q1) of the members idx"""
        pick = lambda a: None if a is None else np.ascontiguousarray(a[idx])
        return pick(self.roots), pick(self.coeffs), pick(self.cols), pick(self.q0), pick(self.q1)


@functools.lru_cache(maxsize=None)
def _batch(num_vars, modulus, fl):
    return Batch(num_vars, modulus, fl)


def _loop(ctx, zf, roots, proofs, stream_len, coeffs, cols, q0, q1, evs):
    """zip_verify of every member's slices: the yardstick"""
    out = []
    for i in range(len(cols)):
        out.append(ctx.verify(roots[i], proofs[i * stream_len: (i + 1) * stream_len], None if coeffs is None else coeffs[i],
                              cols[i], None if q0 is None else q0[i], None if q1 is None else q1[i], evs[i], zf))
    return out


# R = 1 with row_len 1, R = 2 (row_len 1), R = 4, R = 16, R = 32, R = 64; every limb count; the quirk modulus
HONEST = [(0, BENCH_MODULUS, 4), (1, BENCH_MODULUS, 4), (3, BENCH_MODULUS, 4), (8, BENCH_MODULUS, 4), (12, BENCH_MODULUS, 4),
          (8, TEST_MODULUS_2, 2), (3, TEST_MODULUS_2, 2), (9, MOD_3LIMB, 3), (10, MOD_NO_SPARE, 4)]


@pytest.mark.parametrize("num_vars,modulus,fl", HONEST)
def test_honest_batches_equal_zip_verify_per_member(cabi, num_vars, modulus, fl):
    import torch

    b = _batch(num_vars, modulus, fl)
    z, zf = b.z, cabi.make_field(modulus, fl)
    if num_vars >= 3:  # the challenges differ between the members: a kernel reading slice 0 for everyone fails
        assert not np.array_equal(b.cols[0], b.cols[1])
        assert z.num_rows == 1 or not np.array_equal(b.coeffs[0], b.coeffs[1])
    ctx = _ctx(cabi, z)
    evs = b.ev_limbs()
    want = _loop(ctx, zf, b.roots, b.proofs, b.len, b.coeffs, b.cols, b.q0, b.q1, evs)
    got = ctx.batch_verify(b.roots, b.proofs, b.coeffs, b.cols, b.q0, b.q1, evs, zf)
    print(num_vars, fl, got)
    assert got == want
    if z.row_len > 1 and modulus != MOD_NO_SPARE:  # the cases the oracle's verifier accepts (tests/test_gpu_batch.py)
        assert got == [ACCEPTED] * b.B
    dev = torch.from_numpy(b.proofs.copy()).cuda()
    assert ctx.batch_verify(b.roots, dev, b.coeffs, b.cols, b.q0, b.q1, evs, zf) == want


def _chunks(n, size):
    return [range(i, min(i + size, n)) for i in range(0, n, size)]


@pytest.mark.parametrize("entry", vc.PLAN, ids=vc.plan_id)
def test_tamper_catalogue_as_a_batch(cabi, entry):
    key, group = entry
    inst, cases = vc.cases(key, group)
    members = []
    for c, want in cases:
        proof, roots, ev = c.mutate(inst.proof, inst.roots, inst.ev)
        if proof.size == inst.need:  # (a batch has one stream length: "one byte short" and "trailing garbage" stay out)
            members.append((c, want, proof, roots, ev))
    assert len(members) >= len(cases) - 2 and members
    ctx = _ctx(cabi, inst.z)
    zf = cabi.make_field(inst.modulus, inst.fl)
    for chunk in _chunks(len(members), 8 if key[0] == "tall" else 32):
        part = [members[j] for j in chunk]
        n = len(part)
        got = ctx.batch_verify(np.stack([m[3] for m in part]), np.concatenate([m[2] for m in part]),
                               np.tile(inst.coeffs, (n, 1)), np.tile(inst.cols, (n, 1)), np.stack([inst.q0] * n),
                               np.stack([inst.q1] * n),
                               np.array([orc.int_to_limbs(m[4], inst.fl) for m in part], dtype=np.uint64), zf)
        for (c, want, *_), rep in zip(part, got):
            print(inst.name, c.name, rep)
            assert rep == want.report, (inst.name, c.name, want)


def test_mixed_batch_neighbouring_openings_of_one_workgroup(cabi):
    b = _batch(8, BENCH_MODULUS, 4)
    z, zf = b.z, cabi.make_field(BENCH_MODULUS, 4)
    assert z.num_rows == 16  # 16 openings per workgroup: openings 16 and 17 share one
    R, d = z.num_rows, z.depth
    u_bytes, rec_bytes = z.row_len * 64, 8 + 32 * d
    col_bytes = R * (32 + rec_bytes)
    proofs = b.proofs.copy()
    proofs[1 * b.len + u_bytes + 17 * col_bytes + 32 * 5 + 2] ^= 0x08                      # member 1: a value bit, opening 17, row 5
    proofs[3 * b.len + u_bytes + 16 * col_bytes + 32 * R + 0 * rec_bytes + 8 + 3] ^= 0x01  # member 3: a path node, opening 16, row 0
    evs = list(b.evs)
    evs[4] = (evs[4] + 1) % BENCH_MODULUS                                                  # member 4: a wrong claimed evaluation
    ev = b.ev_limbs(evs)
    ctx = _ctx(cabi, z)
    want = _loop(ctx, zf, b.roots, proofs, b.len, b.coeffs, b.cols, b.q0, b.q1, ev)
    got = ctx.batch_verify(b.roots, proofs, b.coeffs, b.cols, b.q0, b.q1, ev, zf)
    print(got)
    assert got == want
    assert got[0] == ACCEPTED and got[2] == ACCEPTED
    assert got[1] == {"verdict": vc.PROXIMITY_TESTING, "column": 17, "bad_merkle_paths": 1, "malformed_paths": 0}
    assert got[3] == {"verdict": vc.MERKLE, "column": 16, "bad_merkle_paths": 1, "malformed_paths": 0}
    assert got[4] == {"verdict": vc.EVAL_CONSISTENCY, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}


# proof_len is a multiple of 8, not of 16 (tests/test_gpu_batch.py): every second stream starts at 8 mod 16
@pytest.mark.parametrize("num_vars,modulus,fl,n_cols", [(0, BENCH_MODULUS, 4, 3), (1, MOD_3LIMB, 3, 5), (2, MOD_3LIMB, 3, 7)])
def test_streams_that_start_at_8_mod_16(cabi, num_vars, modulus, fl, n_cols):
    import torch

    B = 4
    z = orc.Zip(num_vars)
    f, zf = orc.make_field(modulus, fl), cabi.make_field(modulus, fl)
    ctx = _ctx(cabi, z)
    if num_vars < 2:
        assert ctx.proof_len(n_cols, fl) % 16 == 8
    evals = np.stack([_witness(num_vars, seed=77 + 101 * i + 1, small=False) for i in range(B)])
    rng = np.random.default_rng(num_vars)
    cols = rng.integers(0, z.codeword_len, size=(B, n_cols), dtype=np.uint32)
    lr = z.num_rows.bit_length() - 1
    points = [orc.point_to_field(f, rng.integers(-9, 9, size=num_vars, dtype=np.int64)) if num_vars else np.zeros((0, fl), np.uint64)
              for _ in range(B)]
    coeffs = rng.integers(-(2**63), 2**63 - 1, size=(B, z.num_rows), dtype=np.int64) if lr else None
    q0 = np.stack([orc.build_eq_x_r(f, pt[num_vars - lr:]) for pt in points]) if lr else None
    q1 = np.stack([orc.build_eq_x_r(f, pt[: num_vars - lr]) for pt in points]) if num_vars - lr else None
    ev = np.array([orc.int_to_limbs(z.mle_eval(f, evals[i], points[i]), fl) for i in range(B)], dtype=np.uint64)
    if z.row_len == 1:
        ev[::2] = 0  # (a one-column matrix only verifies a zero evaluation: both kinds in one batch)
    batch = ctx.batch_commit(evals)
    stream_len = ctx.proof_len(n_cols, fl)
    out = torch.zeros(B * stream_len, dtype=torch.uint8, device="cuda")
    batch.open(coeffs, cols, q0, zf, out=out)
    want = _loop(ctx, zf, batch.roots, out, stream_len, coeffs, cols, q0, q1, ev)
    got = ctx.batch_verify(batch.roots, out, coeffs, cols, q0, q1, ev, zf)
    print(got)
    assert got == want
    assert any(r == ACCEPTED for r in got)


def test_short_proofs_len(cabi):
    b = _batch(8, BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    idx = [0, 1, 2, 3]
    roots, coeffs, cols, q0, q1 = b.take(idx)
    ev = b.ev_limbs()[idx]
    ctx = _ctx(cabi, b.z)
    want = _loop(ctx, zf, roots[:2], b.proofs, b.len, coeffs, cols[:2], q0, q1, ev)
    before = cabi.batch_verify_calls()
    got = ctx.batch_verify(roots, b.proofs, coeffs, cols, q0, q1, ev, zf, proofs_len=2 * b.len + 1)
    assert cabi.batch_verify_calls() == before + 1
    assert got[:2] == want and want == [ACCEPTED] * 2
    assert got[2:] == [SHORT] * 2
    # no whole stream at all: nothing reaches the device
    assert ctx.batch_verify(roots, b.proofs, coeffs, cols, q0, q1, ev, zf, proofs_len=b.len - 1) == [SHORT] * 4
    assert cabi.batch_verify_calls() == before + 1


def test_launch_count_does_not_depend_on_the_batch_size(cabi):
    b = _batch(8, BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    ctx = _ctx(cabi, b.z)
    ctx.set_profiling(True)
    counts = {}
    for B in (2, 12):
        idx = [i % b.B for i in range(B)]
        roots, coeffs, cols, q0, q1 = b.take(idx)
        proofs = np.concatenate([b.proofs[i * b.len: (i + 1) * b.len] for i in idx])
        ctx.profile_read()
        got = ctx.batch_verify(roots, proofs, coeffs, cols, q0, q1, b.ev_limbs()[idx], zf)
        times = ctx.profile_read()
        assert got == [ACCEPTED] * B
        counts[B] = sum(v[0] for v in times.values())
        assert all(times[k][0] == 1 for k in NEW_KERNELS), times
    assert counts[2] == counts[12] == len(NEW_KERNELS), counts


def _raw(cabi, ctx, b, n_polys, zf, roots=True, proofs=True, coeffs=True, cols=True, q0=True, q1=True, evs=True, reports=True,
         cols_arr=None, n_cols=None):
    idx = [i % b.B for i in range(min(n_polys, 2) or 1)]
    r, k, c, a0, a1 = b.take(idx)
    if cols_arr is not None:
        c = cols_arr
    ev = b.ev_limbs()[idx]
    reps = (cabi.VerifyReport * max(n_polys if n_polys <= 2 else 2, 1))()
    p = lambda on, a: a.ctypes.data if on and a is not None else None
    return cabi.lib().zip_batch_verify(ctx._h, n_polys, p(roots, r), p(proofs, b.proofs), cabi.MEM_HOST, b.proofs.size,
                                       p(coeffs, k), p(cols, c), c.shape[1] if n_cols is None else n_cols, p(q0, a0), p(q1, a1),
                                       p(evs, ev), C.byref(zf), reps if reports else None)


def test_batch_verify_usage_errors(cabi):
    b = _batch(8, BENCH_MODULUS, 4)
    zf = cabi.make_field(BENCH_MODULUS, 4)
    ctx = _ctx(cabi, b.z)
    ctx.set_profiling(True)
    before = cabi.batch_verify_calls()
    for missing in ("roots", "proofs", "evs", "reports", "cols", "coeffs", "q0", "q1"):
        assert _raw(cabi, ctx, b, 2, zf, **{missing: False}) == cabi.ZIP_ERR_NULL, missing
    assert _raw(cabi, ctx, b, 0, zf) == cabi.ZIP_ERR_INVALID_PARAM
    assert _raw(cabi, ctx, b, 65536, zf) == cabi.ZIP_ERR_INVALID_PARAM  # (refused before any array is read)
    for limbs in (1, 5):
        assert _raw(cabi, ctx, b, 2, cabi.make_field(BENCH_MODULUS if limbs > 4 else (1 << 61) - 1, limbs)) == cabi.ZIP_ERR_UNSUPPORTED
    # 65535 x 65538 openings do not fit 32 bits (65535 x 65537 = 2^32 - 1 still would); refused before cols is read
    assert _raw(cabi, ctx, b, 65535, zf, n_cols=65538) == cabi.ZIP_ERR_UNSUPPORTED
    # a column index equal to codeword_len
    bad_cols = np.ascontiguousarray(b.cols[:2]).copy()
    bad_cols[1, 999] = b.z.codeword_len
    assert _raw(cabi, ctx, b, 2, zf, cols_arr=bad_cols) == cabi.ZIP_ERR_INVALID_PARAM
    # a row-sharded ctx
    shard = _ctx(cabi, b.z, row_begin=0, row_count=b.z.num_rows // 2)
    assert _raw(cabi, shard, b, 2, zf) == cabi.ZIP_ERR_INVALID_PARAM
    # codewords above 16384 are not launch-bound: refused, and nothing is launched
    zb = orc.Zip(15, geometry=(16384, 2, 32768))
    big = _ctx(cabi, zb)
    big.set_profiling(True)
    assert _raw(cabi, big, b, 2, zf) == cabi.ZIP_ERR_UNSUPPORTED
    assert sum(v[0] for v in big.profile_read().values()) == 0
    assert sum(v[0] for v in ctx.profile_read().values()) == 0 and cabi.batch_verify_calls() == before
    # the ctx is still usable
    roots, coeffs, cols, q0, q1 = b.take([0, 1])
    assert ctx.batch_verify(roots, b.proofs, coeffs, cols, q0, q1, b.ev_limbs()[:2], zf) == [ACCEPTED] * 2
