"""GPU parity of a batch whose members have their own RAA code and their own field (zip_batch_commit_codes,
zip_batch_open_eval_fields, zip_batch_open_fields, zip_batch_codes_counts): every member against the CPU oracle with THAT
member's permutations and field, bit-exact, and through the unchanged zip_verify.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
MOD_NO_SPARE = (1 << 256) - 189          # quirk_mod 189 (make_field): read as a negative Int by the reference
MOD_SECP = (1 << 256) - (1 << 32) - 977  # another modulus with the quirk, quirk_mod 2^32 + 977
MOD_25519 = (1 << 255) - 19              # top bit clear: no quirk
# five odd moduli per limb count, every member its own; the 4-limb list mixes quirk and no quirk
MODULI = {
    4: [MOD_NO_SPARE, BENCH_MODULUS, MOD_SECP, MOD_25519, BENCH_MODULUS - 2],
    3: [(1 << 190) - 11 * (1 << 64) - 59, (1 << 191) - 19, (1 << 190) - 11, (1 << 189) - 25, (1 << 188) - 125],
    2: [57316695564490278656402085503, (1 << 127) - 1, (1 << 128) - 159, (1 << 126) - 137, (1 << 100) - 15],
}
SEEDS = [(1, 2), (3, 4), (0x5EED, 0xC0DE), (7, 1), (2, 1)]


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
    w[: min(n, 4)] = np.array([-(2**63), 2**63 - 1, -1, 0], dtype=np.int64)[: min(n, 4)]
    return w


def _perms(zs):
    return np.stack([z.perm1 for z in zs]), np.stack([z.perm2 for z in zs])


def _assert_member_equals_oracle(batch, i, z, evals):
    rows_o, layers_o, roots_o = z.commit(evals)
    assert np.array_equal(batch.roots[i], roots_o), i
    rows, layers, roots = batch.member(i).download()
    assert np.array_equal(rows, rows_o), i
    assert np.array_equal(layers, layers_o[:, :-1, :]), i  # reference layers have the root popped
    assert np.array_equal(roots, roots_o), i


# ---------------------------------------------------------------------------------------------- commit
# a single row, R = 2, every E of commit_geom (1, 2, 4 and 8), as tests/test_gpu_batch.py
@pytest.mark.parametrize("num_vars", [0, 1, 3, 8, 12, 13, 15])
def test_commit_codes_equals_oracle_per_member(cabi, num_vars):
    zs = [orc.Zip(num_vars, seeds=s) for s in SEEDS[:3]]
    w = _witness(num_vars, seed=1)
    evals = np.stack([w, w, _witness(num_vars, seed=2)])  # members 0 and 1: the same witness under different codes
    ctx = _ctx(cabi, orc.Zip(num_vars, seeds=(9, 9)))    # the ctx's own permutations are nobody's
    before = cabi.batch_codes_counts()
    batch = ctx.batch_commit_codes(evals, *_perms(zs))
    assert cabi.batch_codes_counts() == (before[0] + 1, before[1] + 3, before[2])
    assert len(batch) == 3 and batch.roots.shape == (3, zs[0].num_rows, 32)
    for i in range(3):
        _assert_member_equals_oracle(batch, i, zs[i], evals[i])
    if zs[0].codeword_len > 2:  # (the two permutations of two entries hardly differ)
        assert not np.array_equal(batch.roots[0], batch.roots[1]), "a kernel that reads slice 0 for every member"
    batch.free()


@pytest.mark.parametrize("num_vars", [3, 12])
def test_commit_codes_with_the_ctx_permutations_equals_batch_commit(cabi, num_vars):
    z = orc.Zip(num_vars)
    evals = np.stack([_witness(num_vars, seed=10 + i) for i in range(4)])
    ctx = _ctx(cabi, z)
    plain = ctx.batch_commit(evals)
    codes = ctx.batch_commit_codes(evals, *_perms([z] * 4))
    assert np.array_equal(plain.roots, codes.roots)
    for i in range(4):
        for a, b in zip(plain.member(i).download(), codes.member(i).download()):
            assert np.array_equal(a, b), i


def _workgroups(cabi, num_vars):
    """the commit launch's workgroup count for the small geometries (one wave, little LDS): 8 resident per CU"""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 8


# 64 and 4 rows per member, more rows than the persistent launch has workgroups: a workgroup's second row belongs to
# another member WITH ANOTHER CODE, and it must reload its permutation indices -- a kernel that loads them on its first
# row only fails here.  Three seed pairs in turn: a second row is G rows after the first, G / R members on, and G / R
# (32 and 512 with 8 x 256 workgroups) is no multiple of 3.  (n_polys * rows - workgroups is asked to be no multiple of
# 64; at 64 rows per member it is one whenever the workgroup count is a multiple of 64 -- 8 x 256 is -- so what is
# asserted is what that stands for: second rows exist, and every one is of a member whose code differs from the first's.)
@pytest.mark.parametrize("num_vars", [12, 3])
def test_member_changes_inside_a_workgroup(cabi, num_vars):
    zs3 = [orc.Zip(num_vars, seeds=s) for s in SEEDS[:3]]
    R = zs3[0].num_rows
    G = _workgroups(cabi, num_vars)
    n_polys = G // R + 3
    total = n_polys * R
    assert total > G
    assert (total - G) % 64 != 0 or (R == 64 and G % 64 == 0)

    def code(i):
        return i % 3

    def wit(i):
        return (i // 3) % 2

    # (round_slot only permutes the slots inside one round: the rows a workgroup plays are G apart)
    assert all(code(g // R) != code((g + G) // R) for g in range(total - G))
    for c in range(3):
        for d in range(c):
            assert not (np.array_equal(zs3[c].perm1, zs3[d].perm1) and np.array_equal(zs3[c].perm2, zs3[d].perm2))
    zs = [zs3[code(i)] for i in range(n_polys)]
    base = [_witness(num_vars, seed=40 + k) for k in range(2)]
    evals = np.stack([base[wit(i)] for i in range(n_polys)])
    want = {(c, k): zs3[c].commit(base[k]) for c in range(3) for k in range(2)}  # computed once, shared
    for k in range(2):  # the codes tell in the roots: a stale code cannot pass by coincidence
        assert len({want[(c, k)][2].tobytes() for c in range(3)}) == 3
    ctx = _ctx(cabi, zs3[0])
    batch = ctx.batch_commit_codes(evals, *_perms(zs))
    for i in range(n_polys):
        assert np.array_equal(batch.roots[i], want[(code(i), wit(i))][2]), i
    for i in (0, 1, n_polys // 2, n_polys - 2, n_polys - 1):  # rows and trees, first and second rounds
        rows_o, layers_o, _ = want[(code(i), wit(i))]
        rows, layers, _ = batch.member(i).download()
        assert np.array_equal(rows, rows_o) and np.array_equal(layers, layers_o[:, :-1, :]), i
    batch.free()


# ------------------------------------------------------------------------------------------------ open
def _open_case(cabi, num_vars, fl, B=5, codes=True):
    """B members, each with its own code (unless not `codes`), field, witness (0 and 1 share one), point and transcript"""
    mods = MODULI[fl]
    zs = [orc.Zip(num_vars, seeds=SEEDS[i] if codes else SEEDS[0]) for i in range(B)]
    fs = [orc.make_field(m, fl) for m in mods]
    zfs = [cabi.make_field(m, fl) for m in mods]
    w = _witness(num_vars, seed=7, small=(fl == 2))
    evals = np.stack([w, w] + [_witness(num_vars, seed=8 + i, small=(fl == 2)) for i in range(B - 2)])
    rng = np.random.default_rng(3 + num_vars)
    pt0 = rng.integers(-100, 100, size=num_vars, dtype=np.int64)
    points_i = [pt0, pt0] + [rng.integers(-100, 100, size=num_vars, dtype=np.int64) for _ in range(B - 2)]
    points = [orc.point_to_field(f, p) if num_vars else np.zeros((0, fl), dtype=np.uint64) for f, p in zip(fs, points_i)]
    want = []
    for z, f, ev, pt in zip(zs, fs, evals, points):
        rows_o, layers_o, roots_o = z.commit(ev)
        proof, cols, coeffs = z.open(f, ev, rows_o, layers_o, pt, orc.new_transcript())  # its own fresh transcript
        want.append((proof, cols.copy(), coeffs.copy(), roots_o))
    lr = zs[0].num_rows.bit_length() - 1
    q0 = np.stack([orc.build_eq_x_r(f, pt[num_vars - lr:]) for f, pt in zip(fs, points)]) if lr else None
    return zs, fs, zfs, mods, evals, points, want, q0


OPEN_CASES = [(8, 4), (8, 2), (3, 2), (0, 4), (1, 4), (9, 3), (10, 4), (12, 4)]


@pytest.mark.parametrize("num_vars,fl", OPEN_CASES)
def test_open_fields_equals_oracle_per_member(cabi, num_vars, fl):
    B = 5
    zs, fs, zfs, mods, evals, points, want, q0 = _open_case(cabi, num_vars, fl)
    z = zs[0]
    cols = np.stack([w[1] for w in want])
    coeffs = np.stack([w[2] for w in want]) if z.num_rows > 1 else None
    ctx = _ctx(cabi, z)
    batch = ctx.batch_commit_codes(evals, *_perms(zs))
    assert np.array_equal(batch.roots, np.stack([w[3] for w in want]))
    before = cabi.batch_codes_counts()
    rows = batch.open_eval_fields(q0, zfs)
    for i in range(B):
        q0_i = q0[i] if q0 is not None else orc.field_elems([(1 << (64 * fl)) % mods[i]], fl)
        assert np.array_equal(rows[i], zs[i].combine_rows_field(fs[i], q0_i, evals[i])), i
    assert not np.array_equal(rows[0], rows[1]), "equal witnesses and points in different fields give different rows"
    proofs = batch.open_fields(coeffs, cols, q0, zfs)
    assert proofs.shape == (B, z.proof_len(fl))
    for i in range(B):
        assert np.array_equal(proofs[i], want[i][0]), i
    assert cabi.batch_codes_counts() == (before[0], before[1], before[2] + 2)
    if (num_vars, fl) in ((8, 4), (1, 4)):
        import torch

        out = torch.zeros(proofs.size, dtype=torch.uint8, device="cuda")
        rows_d = torch.zeros(rows.size, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()  # torch fills on its own stream; the library writes on the ctx's, which does not wait for it
        batch.open_fields(coeffs, cols, q0, zfs, out=out)
        assert np.array_equal(out.cpu().numpy(), proofs.reshape(-1))
        batch.open_eval_fields(q0, zfs, out=rows_d)
        assert np.array_equal(rows_d.cpu().numpy().view(np.uint64), rows.reshape(-1))
    batch.free()


def test_fields_on_a_batch_of_plain_batch_commit(cabi):
    num_vars, fl, B = 8, 4, 5
    zs, fs, zfs, mods, evals, points, want, q0 = _open_case(cabi, num_vars, fl, codes=False)
    ctx = _ctx(cabi, zs[0])
    batch = ctx.batch_commit(evals)
    proofs = batch.open_fields(np.stack([w[2] for w in want]), np.stack([w[1] for w in want]), q0, zfs)
    for i in range(B):
        assert np.array_equal(proofs[i], want[i][0]), i
    # and the one-field calls on a batch of zip_batch_commit_codes: they never read a permutation
    zs, fs, zfs, mods, evals, points, want, q0 = _open_case(cabi, num_vars, fl)
    batch = ctx.batch_commit_codes(evals, *_perms(zs))
    cols, coeffs = np.stack([w[1] for w in want]), np.stack([w[2] for w in want])
    q0_1 = np.stack([orc.build_eq_x_r(fs[1], orc.point_to_field(fs[1], np.arange(4) + i)) for i in range(B)])
    one = batch.open(coeffs, cols, q0_1, zfs[1])
    for i in range(B):
        m = batch.member(i)
        assert np.array_equal(one[i], m.open(evals[i], coeffs[i], cols[i], q0_1[i], zfs[1])), i
        m.free()


# ------------------------------------------------------------------------- through the unchanged verifier
def test_streams_pass_zip_verify_on_each_members_own_ctx(cabi):
    num_vars, fl, B = 9, 3, 5
    zs, fs, zfs, mods, evals, points, want, q0 = _open_case(cabi, num_vars, fl)
    z = zs[0]
    cols, coeffs = np.stack([w[1] for w in want]), np.stack([w[2] for w in want])
    ctx = _ctx(cabi, z)
    batch = ctx.batch_commit_codes(evals, *_perms(zs))
    proofs = batch.open_fields(coeffs, cols, q0, zfs)
    lr = z.num_rows.bit_length() - 1
    row_at = z.proof_len(fl) - z.row_len * 8 * fl
    bad = proofs.copy()
    bad[2, row_at + 5] ^= 1  # one byte of member 2's evaluation row
    for i in range(B):
        own = _ctx(cabi, zs[i])  # created with member i's permutations
        q1 = orc.build_eq_x_r(fs[i], points[i][: num_vars - lr])
        ev = np.array(orc.int_to_limbs(zs[i].mle_eval(fs[i], evals[i], points[i]), fl), dtype=np.uint64)
        rep = own.verify(batch.roots[i], proofs[i], coeffs[i], cols[i], q0[i], q1, ev, zfs[i])
        assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}, i
        rep = own.verify(batch.roots[i], bad[i], coeffs[i], cols[i], q0[i], q1, ev, zfs[i])
        assert (rep["verdict"] == cabi.VERIFY_ACCEPT) == (i != 2), (i, rep)
        own.close()


# ---------------------------------------------------------------------------------------- usage errors
def test_usage_errors_reach_no_device(cabi):
    nv = 8
    z = orc.Zip(nv)
    cw = z.codeword_len
    ctx = _ctx(cabi, z)
    evals = np.stack([_witness(nv, seed=i) for i in range(3)])
    p1, p2 = _perms([orc.Zip(nv, seeds=s) for s in SEEDS[:3]])
    before = cabi.batch_codes_counts()
    L = cabi.lib()

    def commit(ctx_, ev, n_evals, n_polys, a, b):
        h = C.c_void_p()
        rc = L.zip_batch_commit_codes(ctx_._h, ev.ctypes.data, n_evals, n_polys, cabi.MEM_HOST,
                                      None if a is None else a.ctypes.data, None if b is None else b.ctypes.data, None, C.byref(h))
        assert rc != 0 and not h.value
        return rc

    assert commit(ctx, evals, evals.size, 3, None, p2) == cabi.ZIP_ERR_NULL
    assert commit(ctx, evals, evals.size, 3, p1, None) == cabi.ZIP_ERR_NULL
    assert commit(ctx, evals, 0, 0, None, None) == cabi.ZIP_ERR_NULL  # NULL comes before the ranges
    assert commit(ctx, evals, 0, 0, p1, p2) == cabi.ZIP_ERR_INVALID_PARAM
    assert commit(ctx, evals, evals.size, 65536, p1, p2) == cabi.ZIP_ERR_INVALID_PARAM
    assert commit(ctx, evals, evals.size - 1, 3, p1, p2) == cabi.ZIP_ERR_SHAPE
    rep = p1.copy()
    rep[2, 5] = rep[2, 6]  # a repeated index, in the last member
    assert commit(ctx, evals, evals.size, 3, rep, p2) == cabi.ZIP_ERR_INVALID_PARAM
    big = p2.copy()
    big[1, 0] = cw
    assert commit(ctx, evals, evals.size, 3, p1, big) == cabi.ZIP_ERR_INVALID_PARAM
    assert commit(ctx, evals, evals.size - 1, 3, rep, p2) == cabi.ZIP_ERR_SHAPE  # the permutations are looked at last
    shard = _ctx(cabi, z, row_begin=0, row_count=z.num_rows // 2)
    assert commit(shard, evals, evals.size, 3, p1, p2) == cabi.ZIP_ERR_INVALID_PARAM
    # a codeword of 16384: zip_batch_commit serves it, the geometry with a code per member is not built
    zb = orc.Zip(14, geometry=(8192, 2, 16384))
    cb = _ctx(cabi, zb)
    wb = np.zeros((2, 2 * 8192), dtype=np.int64)
    pb1, pb2 = _perms([zb, zb])
    assert commit(cb, wb, wb.size, 2, pb1, pb2) == cabi.ZIP_ERR_UNSUPPORTED
    assert b"not built" in L.zip_ctx_last_error(cb._h)
    assert cabi.batch_codes_counts() == before

    # the fields of the two opens
    batch = ctx.batch_commit_codes(evals, p1, p2)
    assert cabi.batch_codes_counts() == (before[0] + 1, before[1] + 3, before[2])
    f = orc.make_field(BENCH_MODULUS, 4)
    q0 = np.stack([orc.build_eq_x_r(f, orc.point_to_field(f, [1, 2, 3, 4]))] * 3)
    coeffs = np.ones((3, z.num_rows), dtype=np.int64)
    cols = np.zeros((3, 4), dtype=np.uint32)
    ok = [cabi.make_field(m, 4) for m in MODULI[4][:3]]
    cases = [([ok[0], ok[1], cabi.make_field(MODULI[3][0], 3)], cabi.ZIP_ERR_INVALID_PARAM),   # differing limb counts
             ([ok[0], cabi.make_field(BENCH_MODULUS - 1, 4), ok[2]], cabi.ZIP_ERR_INVALID_PARAM),  # an even modulus
             ([ok[0], ok[1], cabi.make_field(1, 4)], cabi.ZIP_ERR_INVALID_PARAM),
             ([cabi.make_field(3, 1)] * 3, cabi.ZIP_ERR_INVALID_PARAM),
             ([ok[0], None, ok[2]], cabi.ZIP_ERR_NULL)]
    for fields, code in cases:
        with pytest.raises(cabi.ZipError) as e:
            batch.open_eval_fields(q0, fields)
        assert e.value.code == code, fields
        with pytest.raises(cabi.ZipError) as e:
            batch.open_fields(coeffs, cols, q0, fields)
        assert e.value.code == code, fields
    rows = np.zeros((3, z.row_len, 4), dtype=np.uint64)
    assert L.zip_batch_open_eval_fields(batch._h, q0.ctypes.data, None, rows.ctypes.data, cabi.MEM_HOST) == cabi.ZIP_ERR_NULL
    cols[2, 3] = cw
    with pytest.raises(cabi.ZipError) as e:
        batch.open_fields(coeffs, cols, q0, ok)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    assert cabi.batch_codes_counts() == (before[0] + 1, before[1] + 3, before[2])
    cols[2, 3] = cw - 1
    assert batch.open_fields(coeffs, cols, q0, ok).shape[0] == 3  # the handle is still usable
    assert cabi.batch_codes_counts() == (before[0] + 1, before[1] + 3, before[2] + 1)
