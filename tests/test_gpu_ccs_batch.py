"""zip_ccs_batch on the device: the Spartan tables of several proofs of ONE circuit, each proof in its own field, built
with a launch count that does not depend on the number of proofs.  Every table of every instance -- z in F_q, every
M_k z, eq(beta), eq(r_x), the second sumcheck's table -- and V_s is compared bit for bit with the oracle's
(orc.Ccs(inst).mz / second_table, orc.build_eq_x_r); there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import _ccs
import _ccs_random
import _oracle as orc

pytestmark = pytest.mark.gpu

MODULI, Q256, QSTARK = _ccs_random.MODULI, _ccs_random.Q256, _ccs_random.QSTARK
Q192 = _ccs_random.Q192


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _moduli(fl, n, shift=0):
    """n moduli of fl limbs; members 1 and 2 share one (with equal z they differ in nothing, with other z only in z)"""
    ms = MODULI[fl]
    order = [0, 1, 1, 2, 3, 0, 2]
    return [ms[(order[i % len(order)] + shift) % len(ms)] for i in range(n)]


def _witnesses(s, n):
    """n z vectors; members 0 and 1 share one (with _moduli: they differ only in their field)"""
    zs = _ccs_random.witnesses(s, n)
    if n > 1:
        zs[1] = zs[0]
    return zs


def _to_ints(a):
    """[n, fl] limbs -> object array of Python ints"""
    out = np.zeros(a.shape[0], dtype=object)
    for j in range(a.shape[1]):
        out += a[:, j].astype(object) << (64 * j)
    return out


def _challenges(f, fl, rng, n):
    return orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=n)], fl)


def _run_and_compare(cabi, batch, insts, moduli, fl, seed, second=True):
    """set_z, eq_tables(0), second_tables on `batch`; every table and V_s of every instance against the oracle"""
    n, s, t, m = len(insts), insts[0].s, insts[0].t, insts[0].m
    fields = [orc.make_field(q, fl) for q in moduli]
    rng = np.random.default_rng(seed)
    beta = np.stack([_challenges(f, fl, rng, s) for f in fields])
    r_x = np.stack([_challenges(f, fl, rng, s) for f in fields])
    gamma = np.stack([_challenges(f, fl, rng, 1)[0] for f in fields])
    batch.set_z([cabi.make_field(q, fl) for q in moduli], [i.z for i in insts])
    assert batch.n == n
    batch.eq_tables(beta, 0)
    vs = batch.second_tables(r_x, gamma) if second else None
    for i, (inst, f, q) in enumerate(zip(insts, fields, moduli)):
        o = orc.Ccs(inst)
        zf = batch.download(i, cabi.CCS_Z_FIELD)
        want_z = orc.field_elems([orc.field_from_i64(f, int(v)) for v in inst.z], fl)
        assert np.array_equal(zf[: len(inst.z)], want_z), (i, "z_f")
        assert not zf[len(inst.z):].any(), (i, "z_f beyond z_len")
        mz_o = o.mz(f)
        for k in range(t):
            assert np.array_equal(batch.download(i, cabi.CCS_MZ, k), mz_o[k]), (i, "mz", k)
        assert np.array_equal(batch.download(i, cabi.CCS_EQ, 0), orc.build_eq_x_r(f, beta[i])), (i, "eq slot 0")
        if not second:
            continue
        eq1 = orc.build_eq_x_r(f, r_x[i])
        assert np.array_equal(batch.download(i, cabi.CCS_EQ, 1), eq1), (i, "eq slot 1")
        assert np.array_equal(batch.download(i, cabi.CCS_SECOND), o.second_table(f, eq1, gamma[i])), (i, "second")
        R_inv = pow(1 << (64 * fl), -1, q)
        e = _to_ints(eq1)
        for k in range(t):  # V_s[k] = <Mz_k, eq(r_x)>, in Python integers (Montgomery: a*b*R^-1)
            assert orc.limbs_to_int(vs[i, k]) == int((_to_ints(mz_o[k]) * e).sum()) * R_inv % q, (i, "V_s", k)


@pytest.mark.parametrize("fl", [2, 3, 4])
@pytest.mark.parametrize("s,B", [(1, 5), (2, 5), (3, 5), (10, 5), (13, 5)])
def test_random_circuit_tables_equal_the_oracle(cabi, s, B, fl):
    """t = 7 on the random circuit: empty rows and columns, one column hit by every row, a matrix with fewer rows, an
    explicit zero, INT64_MIN / INT64_MAX among the values and the witnesses; five fields in one call; members 0 / 1
    differ only in their field, members 1 / 2 only in z.  n = capacity at even s, n < capacity at odd s."""
    moduli, zs = _moduli(fl, B), _witnesses(s, B)
    assert moduli[0] != moduli[1] and zs[0] is zs[1] and moduli[1] == moduli[2] and zs[1] is not zs[2]
    insts = _ccs_random.instances(s, 7, zs)
    batch = cabi.CcsBatch(insts[0].matrices, s, fl, B + s % 2)
    _run_and_compare(cabi, batch, insts, moduli, fl, seed=100 * s + fl)
    batch.free()


def test_2_pow_16_rows_two_proofs(cabi):
    """the largest size: 16 workgroups per instance in the eq kernel, 256 row blocks, a CSC column of 2^16 entries"""
    s, fl = 16, 4
    insts = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, 2))
    batch = cabi.CcsBatch(insts[0].matrices, s, fl, 2)
    _run_and_compare(cabi, batch, insts, [Q256, QSTARK], fl, seed=16)
    batch.free()


@pytest.mark.parametrize("fl", [2, 3, 4])
def test_vitalik_circuit_five_statements(cabi, fl):
    """t = 3: x^3 + x + 5 = y for five x, one of them negative, each proof in its own field"""
    insts = [_ccs.vitalik_ccs(x) for x in (3, 5, -7, 2, 11)]
    batch = cabi.CcsBatch(insts[0].matrices, 3, fl, 5)
    _run_and_compare(cabi, batch, insts, _moduli(fl, 5), fl, seed=fl)
    batch.free()


@pytest.mark.parametrize("s", [3, 10])
def test_a_handle_is_reusable_with_another_n_and_other_fields(cabi, s):
    """n = capacity, then n = 1, then n < capacity with other fields and other z on the SAME handle: stale arguments or
    tables of the earlier call would show"""
    fl, cap = 4, 5
    batch = None
    for n, shift in ((cap, 0), (1, 1), (3, 2), (cap, 3)):
        zs = _ccs_random.witnesses(s, n, seed=0x5EED + shift)
        insts = _ccs_random.instances(s, 7, zs)
        batch = batch or cabi.CcsBatch(insts[0].matrices, s, fl, cap)
        _run_and_compare(cabi, batch, insts, _moduli(fl, n, shift), fl, seed=s + shift)
    # after a set_z the tables of the calls before it are gone: nothing stale is handed out
    batch.set_z([cabi.make_field(QSTARK, fl)], [np.ones(3, np.int64)])
    for which, index in ((cabi.CCS_EQ, 0), (cabi.CCS_EQ, 1), (cabi.CCS_SECOND, 0)):
        with pytest.raises(cabi.ZipError) as e:
            batch.table(0, which, index)
        assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    batch.free()


def test_z_on_the_device_is_read_in_place(cabi):
    import torch

    s, fl, n = 3, 3, 4
    insts = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, n))
    moduli = _moduli(fl, n)
    batch = cabi.CcsBatch(insts[0].matrices, s, fl, n)
    zs_d = [torch.from_numpy(i.z).cuda() for i in insts]
    batch.set_z([cabi.make_field(q, fl) for q in moduli], zs_d)
    for i, (inst, q) in enumerate(zip(insts, moduli)):
        mz_o = orc.Ccs(inst).mz(orc.make_field(q, fl))
        for k in range(inst.t):
            assert np.array_equal(batch.download(i, cabi.CCS_MZ, k), mz_o[k]), (i, k)
    batch.free()


def test_launches_do_not_depend_on_the_number_of_proofs(cabi):
    s, fl = 10, 4
    moved = {}
    for B in (2, 7):
        insts = _ccs_random.instances(s, 7, _witnesses(s, B))
        batch = cabi.CcsBatch(insts[0].matrices, s, fl, B)
        before = cabi.ccs_batch_counts()
        _run_and_compare(cabi, batch, insts, _moduli(fl, B), fl, seed=B)
        after = cabi.ccs_batch_counts()
        moved[B] = after[0] - before[0]
        assert after[1] - before[1] == B
        batch.free()
    assert moved[2] == moved[7] == 6  # set_z: map + M z; eq_tables: 1; second_tables: eq, the table, V_s


def test_usage_errors_on_a_handle(cabi):
    """with their codes and in the documented order; a refused call leaves the handle as it was"""
    s, fl, cap = 3, 4, 3
    L = cabi.lib()
    insts = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, cap))
    batch = cabi.CcsBatch(insts[0].matrices, s, fl, cap)
    h = batch._h
    x = np.zeros((cap, s + 1, fl), np.uint64)
    p = C.c_void_p()
    # before set_z
    assert L.zip_ccs_batch_eq_tables(h, x.ctypes.data, 0) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_second_tables(h, x.ctypes.data, x.ctypes.data, x.ctypes.data) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_table(h, 0, cabi.CCS_MZ, 0, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_eq_tables(h, None, 0) == cabi.ZIP_ERR_NULL  # NULL first
    assert b"set_z" in L.zip_ccs_batch_last_error(h)

    good = [cabi.make_field(q, fl) for q in _moduli(fl, cap)]
    zs = [i.z for i in insts]

    def set_z(fields=good, zs=zs, n=None, lens=None, null_field=None, null_z=None):
        n = len(zs) if n is None else n
        k = max(len(zs), 1)
        fa = (C.POINTER(cabi.ZipField) * k)(*[C.pointer(f) for f in fields[:k]])
        za = (C.c_void_p * k)(*[z.ctypes.data for z in zs])
        la = (C.c_size_t * k)(*(lens or [z.size for z in zs]))
        if null_field is not None:
            fa[null_field] = None
        if null_z is not None:
            za[null_z] = None
        return L.zip_ccs_batch_set_z(h, C.cast(fa, C.c_void_p), C.cast(za, C.c_void_p), C.cast(la, C.c_void_p), n, cabi.MEM_HOST)

    even, one, short = cabi.make_field(QSTARK - 1, fl), cabi.make_field(1, fl), cabi.make_field(Q192, 3)
    assert set_z(null_field=1) == cabi.ZIP_ERR_NULL
    assert set_z(null_z=2) == cabi.ZIP_ERR_NULL
    assert set_z(null_z=2, lens=[zs[0].size, zs[1].size, 0]) == cabi.ZIP_OK  # an empty z needs no pointer
    assert set_z(null_field=1, n=0) == cabi.ZIP_ERR_INVALID_PARAM  # (nothing of the arrays is read at n = 0)
    assert set_z(n=0) == cabi.ZIP_ERR_INVALID_PARAM
    four = zs + [zs[0]]
    assert set_z(fields=good + [good[0]], zs=four) == cabi.ZIP_ERR_INVALID_PARAM  # n above the capacity
    assert set_z(fields=[good[0], short, good[2]]) == cabi.ZIP_ERR_INVALID_PARAM
    assert set_z(fields=[good[0], good[1], even]) == cabi.ZIP_ERR_INVALID_PARAM
    assert set_z(fields=[one, good[1], good[2]]) == cabi.ZIP_ERR_INVALID_PARAM
    assert set_z(lens=[8, 9, 8]) == cabi.ZIP_ERR_SHAPE
    # the order: NULL, then INVALID_PARAM, then SHAPE
    assert set_z(fields=[good[0], good[1], even], null_z=0) == cabi.ZIP_ERR_NULL
    assert set_z(fields=[good[0], good[1], even], lens=[9, 8, 8]) == cabi.ZIP_ERR_INVALID_PARAM

    # a handle with tables: refused calls leave them as they were
    moduli = _moduli(fl, cap)
    _run_and_compare(cabi, batch, insts, moduli, fl, seed=1, second=False)
    want = batch.download(1, cabi.CCS_MZ, 2)
    assert set_z(fields=[good[0], good[1], even]) == cabi.ZIP_ERR_INVALID_PARAM
    assert set_z(lens=[8, 9, 8]) == cabi.ZIP_ERR_SHAPE
    assert L.zip_ccs_batch_eq_tables(h, x.ctypes.data, 2) == cabi.ZIP_ERR_INVALID_PARAM
    assert np.array_equal(batch.download(1, cabi.CCS_MZ, 2), want)
    assert L.zip_ccs_batch_table(h, cap, cabi.CCS_MZ, 0, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM  # instance >= n
    assert L.zip_ccs_batch_table(h, 0, cabi.CCS_MZ, 7, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_table(h, 0, cabi.CCS_EQ, 1, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM      # slot 1 not built
    assert L.zip_ccs_batch_table(h, 0, cabi.CCS_SECOND, 0, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_table(h, 0, 9, 0, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_table(h, 0, cabi.CCS_MZ, 0, None) == cabi.ZIP_ERR_NULL
    assert L.zip_ccs_batch_table(h, 0, cabi.CCS_EQ, 0, C.byref(p)) == cabi.ZIP_OK and p.value
    batch.free()


def test_tables_that_cannot_fit_are_refused(cabi):
    """65535 proofs at 2^16 rows: 1.5 PB of tables"""
    ident = _ccs.CsrMatrix.diagonal(np.ones(1 << 16, dtype=np.int64))
    with pytest.raises(cabi.ZipError) as e:
        cabi.CcsBatch([ident] * 3, 16, 4, 65535)
    assert e.value.code == cabi.ZIP_ERR_ALLOC
