"""zip_ccs_batch_eval_matrices on the device: the verifier's V_xy = mle[M_k](r_x, r_y) of several proofs of ONE circuit,
each proof in its own field, in three launches whatever their number.  Bit for bit against the oracle per instance
(orc.Ccs(inst).eval_matrices) and against zip_ccs_eval_matrices on a one-field zip_ccs; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import _ccs
import _ccs_random
import _oracle as orc
from test_gpu_spartan_batch import _boolean_instances

pytestmark = pytest.mark.gpu

MODULI = _ccs_random.MODULI
INT64_MIN, INT64_MAX = _ccs_random.INT64_MIN, _ccs_random.INT64_MAX
LAUNCHES = 3  # eq(r_x), eq(r_y), the sums: what include/zip_hip.h documents


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


def _moduli(fl, n):
    """n moduli of fl limbs, five different in turn where the list has them; members 1 and 2 share one"""
    ms = MODULI[fl]
    return [ms[(0, 1, 1, 2, 3)[i % 5]] for i in range(n)]


def _challenges(f, fl, rng, n):
    return orc.field_elems([orc.field_from_i64(f, int(v)) for v in rng.integers(-2**62, 2**62, size=n)], fl)


def _points(moduli, fl, s, seed):
    fields = [orc.make_field(q, fl) for q in moduli]
    rng = np.random.default_rng(seed)
    r_x = np.stack([_challenges(f, fl, rng, s) for f in fields])
    r_y = np.stack([_challenges(f, fl, rng, s) for f in fields])
    return fields, r_x, r_y


def _compare(cabi, batch, inst, moduli, fl, seed, one_field=True):
    """eval_matrices of len(moduli) instances against the oracle and (one_field) against zip_ccs_eval_matrices"""
    fields, r_x, r_y = _points(moduli, fl, inst.s, seed)
    got = batch.eval_matrices([cabi.make_field(q, fl) for q in moduli], r_x, r_y)
    assert got.shape == (len(moduli), inst.t, fl)
    o = orc.Ccs(inst)
    for i, (f, q) in enumerate(zip(fields, moduli)):
        assert np.array_equal(got[i], o.eval_matrices(f, r_x[i], r_y[i])), (i, "oracle")
        if one_field:
            one = cabi.Ccs(inst.matrices, inst.s, cabi.make_field(q, fl))
            assert np.array_equal(got[i], one.eval_matrices(r_x[i], r_y[i])), (i, "zip_ccs_eval_matrices")
            one.free()
    return got


@pytest.mark.parametrize("fl", [2, 3, 4])
@pytest.mark.parametrize("s", [1, 4, 10])
@pytest.mark.parametrize("circuit", ["boolean", "random"])
def test_v_xy_of_five_instances_equals_the_oracle_and_zip_ccs(cabi, circuit, s, fl):
    """boolean: t = 3, three identities.  random: t = 7 with a matrix of fewer than 2^s rows, empty rows and columns, one
    column hit by every row, and -1, INT64_MIN, INT64_MAX among the values; every modulus list holds one that the
    reference reads as a small negative integer (quirk_mod)."""
    n = 5
    inst = (_boolean_instances(s, 1) if circuit == "boolean" else _ccs_random.instances(s, 7, _ccs_random.witnesses(s, 1)))[0]
    if circuit == "random" and s >= 4:
        feats = _ccs_random.features(inst.matrices)
        assert feats["short_matrix"] and feats["specials"], feats
    moduli = _moduli(fl, n)
    assert any((1 << (64 * fl)) - q < 1 << 64 for q in moduli)
    batch = cabi.CcsBatch(inst.matrices, s, fl, n + s % 2)  # n = capacity at even s, n < capacity at odd s
    _compare(cabi, batch, inst, moduli, fl, seed=100 * s + fl)
    batch.free()


@pytest.mark.parametrize("fl", [2, 3, 4])
def test_extreme_values_under_a_quirk_modulus(cabi, fl):
    """-1, INT64_MIN and INT64_MAX on the diagonals of a matrix with fewer than 2^s rows, every instance in a field whose
    modulus is 2^(64 fl) minus less than a limb: the signed-modulus path of the value map"""
    s, m = 3, 8
    quirk = {2: (1 << 128) - 159, 3: (1 << 192) - 237, 4: _ccs_random.Q256}[fl]
    assert (1 << (64 * fl)) - quirk < 1 << 64
    vals = np.array([-1, INT64_MIN, INT64_MAX, 1, -1, INT64_MAX, INT64_MIN, 5], dtype=np.int64)
    short = _ccs.CsrMatrix(5, m, [sorted([(int(vals[r]), (r + 3) % m), (int(vals[(r + 1) % m]), r)], key=lambda e: e[1])
                                  for r in range(5)])
    mats = [_ccs.CsrMatrix.diagonal(vals), short, _ccs.CsrMatrix.diagonal(vals[::-1].copy())]
    inst = _ccs.CcsInstance(m, m, s, s, 2, mats, [[0, 1], [2]], [1, -1], np.ones(m, dtype=np.int64))
    batch = cabi.CcsBatch(mats, s, fl, 3)
    _compare(cabi, batch, inst, [quirk, MODULI[fl][1], quirk], fl, seed=fl)
    batch.free()


def test_the_same_points_in_different_fields_give_different_values(cabi):
    s, fl = 4, 4
    inst = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, 1))[0]
    moduli = [MODULI[fl][0], MODULI[fl][1]]
    ints = np.random.default_rng(5).integers(-100, 100, size=(2, s))
    fields = [orc.make_field(q, fl) for q in moduli]
    r_x = np.stack([orc.point_to_field(f, ints[0]) for f in fields])
    r_y = np.stack([orc.point_to_field(f, ints[1]) for f in fields])
    batch = cabi.CcsBatch(inst.matrices, s, fl, 2)
    got = batch.eval_matrices([cabi.make_field(q, fl) for q in moduli], r_x, r_y)
    o = orc.Ccs(inst)
    for i, f in enumerate(fields):
        assert np.array_equal(got[i], o.eval_matrices(f, r_x[i], r_y[i])), i
    assert not np.array_equal(got[0], got[1]), "a kernel that reads entry 0 for every instance"
    batch.free()


def test_launches_do_not_depend_on_the_number_of_instances(cabi):
    s, fl = 10, 4
    inst = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, 1))[0]
    batch = cabi.CcsBatch(inst.matrices, s, fl, 5)
    for n in (1, 5):
        before = cabi.ccs_batch_counts()
        _compare(cabi, batch, inst, _moduli(fl, n), fl, seed=n, one_field=False)
        after = cabi.ccs_batch_counts()
        assert after[0] - before[0] == LAUNCHES, n
        assert after[1] == before[1]  # (no set_z ran)
    batch.free()


def test_the_call_replaces_the_tables_and_set_z_brings_them_back(cabi):
    s, fl, n = 4, 3, 3
    insts = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, n))
    moduli = _moduli(fl, n)
    zfs = [cabi.make_field(q, fl) for q in moduli]
    batch = cabi.CcsBatch(insts[0].matrices, s, fl, n)
    _compare(cabi, batch, insts[0], moduli, fl, seed=1, one_field=False)  # needs no set_z
    batch.set_z(zfs, [i.z for i in insts])
    want = batch.download(1, cabi.CCS_MZ, 2)
    _compare(cabi, batch, insts[0], moduli[:2], fl, seed=2, one_field=False)
    L, p = cabi.lib(), C.c_void_p()
    x = np.zeros((n, s + 1, fl), np.uint64)
    assert L.zip_ccs_batch_table(batch._h, 0, cabi.CCS_MZ, 0, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_table(batch._h, 0, cabi.CCS_EQ, 0, C.byref(p)) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_eq_tables(batch._h, x.ctypes.data, 0) == cabi.ZIP_ERR_INVALID_PARAM
    assert L.zip_ccs_batch_second_tables(batch._h, x.ctypes.data, x.ctypes.data, x.ctypes.data) == cabi.ZIP_ERR_INVALID_PARAM
    batch.set_z(zfs, [i.z for i in insts])
    assert np.array_equal(batch.download(1, cabi.CCS_MZ, 2), want)
    f = orc.make_field(moduli[0], fl)
    r = np.stack([_challenges(orc.make_field(q, fl), fl, np.random.default_rng(9), s) for q in moduli])
    batch.eq_tables(r, 0)
    assert np.array_equal(batch.download(0, cabi.CCS_EQ, 0), orc.build_eq_x_r(f, r[0]))
    batch.free()


def test_usage_errors_in_the_order_of_set_z(cabi):
    s, fl, cap = 3, 4, 3
    L = cabi.lib()
    inst = _ccs_random.instances(s, 7, _ccs_random.witnesses(s, 1))[0]
    batch = cabi.CcsBatch(inst.matrices, s, fl, cap)
    h = batch._h
    good = [cabi.make_field(q, fl) for q in _moduli(fl, cap)]
    x = np.zeros((cap + 1, s, fl), np.uint64)
    out = np.zeros((cap + 1, 7, fl), np.uint64)

    def call(fields=good, n=None, r_x=x, r_y=x, v=out, null_field=None, handle=h):
        k = max(len(fields), 1)
        fa = (C.POINTER(cabi.ZipField) * k)(*[C.pointer(f) for f in fields])
        if null_field is not None:
            fa[null_field] = None
        p = lambda a: None if a is None else a.ctypes.data
        return L.zip_ccs_batch_eval_matrices(handle, C.cast(fa, C.c_void_p), len(fields) if n is None else n, p(r_x), p(r_y), p(v))

    before = cabi.ccs_batch_counts()
    even, one, short = cabi.make_field(_ccs_random.QSTARK - 1, fl), cabi.make_field(1, fl), cabi.make_field(_ccs_random.Q192, 3)
    assert call(handle=None) == cabi.ZIP_ERR_NULL
    assert L.zip_ccs_batch_eval_matrices(h, None, 1, x.ctypes.data, x.ctypes.data, out.ctypes.data) == cabi.ZIP_ERR_NULL
    assert call(r_x=None) == cabi.ZIP_ERR_NULL
    assert call(r_y=None) == cabi.ZIP_ERR_NULL
    assert call(v=None) == cabi.ZIP_ERR_NULL
    assert call(null_field=1) == cabi.ZIP_ERR_NULL
    assert call(n=0) == cabi.ZIP_ERR_INVALID_PARAM
    assert call(fields=good + [good[0]]) == cabi.ZIP_ERR_INVALID_PARAM  # n above the capacity
    assert call(fields=[good[0], short, good[2]]) == cabi.ZIP_ERR_INVALID_PARAM
    assert call(fields=[good[0], good[1], even]) == cabi.ZIP_ERR_INVALID_PARAM
    assert call(fields=[one, good[1], good[2]]) == cabi.ZIP_ERR_INVALID_PARAM
    assert call(fields=[good[0], good[1], even], null_field=0) == cabi.ZIP_ERR_NULL  # NULL first
    assert cabi.ccs_batch_counts() == before
    assert call() == cabi.ZIP_OK
    batch.free()
