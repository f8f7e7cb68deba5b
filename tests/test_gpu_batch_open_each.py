"""GPU parity of zip_batch_open_each: the batch open of zip_batch_open_fields with every member's stream delivered to a
destination of its own -- HOST destinations window by window through two staging slots, DEVICE destinations through a
device table of pointers.  Five members throughout, each with its own witness, RAA code, columns, coefficients and
modulus, so a stale member offset cannot pass; 12 openings per member, one column of each list a duplicate.  Every stream
against the CPU oracle's `open` of that member, bit-exact, and against the slice of zip_batch_open_fields.  Needs a real
MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as orc
from test_gpu_batch_codes import MODULI, SEEDS, _ctx, _perms, _witness

pytestmark = pytest.mark.gpu

B, N_COLS = 5, 12
GUARD = 0xA5
# what zip_batch_open_fields launches on the parent commit, and what the new call launches instead
FIELDS_KERNELS = {"batch_combine_fields_kernel", "batch_open_columns_kernel"}
EACH_KERNELS = {"batch_combine_each_kernel", "batch_open_columns_each_kernel"}


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


class Case:
    """Five honest members of one geometry; the oracle's streams, computed once and never modified.  The oracle squeezes
    its 12 columns from the member's transcript; the last of them is then replaced by a copy of the third, and the
    expected stream gets the oracle's own bytes of that column's opening in the last place (an opening depends on its
    column alone)."""

    def __init__(self, num_vars, fl):
        self.num_vars, self.fl, self.mods = num_vars, fl, MODULI[fl]
        self.zs = [orc.Zip(num_vars, seeds=SEEDS[i]) for i in range(B)]
        for z in self.zs:
            z.p.num_column_opening = N_COLS
        z = self.zs[0]
        self.fs = [orc.make_field(m, fl) for m in self.mods]
        small = fl == 2
        self.evals = np.stack([_witness(num_vars, seed=20 + i, small=small) for i in range(B)])
        rng = np.random.default_rng(11 + num_vars)
        pts = [rng.integers(-100, 100, size=num_vars, dtype=np.int64) for _ in range(B)]
        self.points = [orc.point_to_field(f, p) if num_vars else np.zeros((0, fl), dtype=np.uint64) for f, p in zip(self.fs, pts)]
        self.lr = z.num_rows.bit_length() - 1
        self.len = z.proof_len(fl)
        self.u_bytes = z.row_len * z.m_limbs * 8 if z.num_rows > 1 else 0
        self.col_bytes = z.num_rows * (8 * z.k_limbs + 8 + 32 * z.depth)
        self.row_bytes = z.row_len * 8 * fl
        assert self.len == self.u_bytes + N_COLS * self.col_bytes + self.row_bytes
        want, cols, coeffs, roots = [], [], [], []
        for z_i, f, ev, pt in zip(self.zs, self.fs, self.evals, self.points):
            rows_o, layers_o, roots_o = z_i.commit(ev)
            proof, c, k = z_i.open(f, ev, rows_o, layers_o, pt, orc.new_transcript())
            c, proof = c.copy(), proof.copy()
            c[N_COLS - 1] = c[2]
            at = lambda j: self.u_bytes + j * self.col_bytes
            proof[at(N_COLS - 1): at(N_COLS)] = proof[at(2): at(3)]
            proof.setflags(write=False)
            want.append(proof)
            cols.append(c)
            coeffs.append(k.copy())
            roots.append(roots_o)
        self.want, self.cols, self.roots = want, np.stack(cols), np.stack(roots)
        self.coeffs = np.stack(coeffs) if self.lr else None
        self.q0 = np.stack([orc.build_eq_x_r(f, pt[num_vars - self.lr:]) for f, pt in zip(self.fs, self.points)]) if self.lr else None

    def zfields(self, cabi):
        return [cabi.make_field(m, self.fl) for m in self.mods]

    def batch(self, cabi):
        """-> (ctx, batch): committed under the members' codes on a ctx whose own permutations are nobody's"""
        ctx = _ctx(cabi, orc.Zip(self.num_vars, seeds=(9, 9)))
        batch = ctx.batch_commit_codes(self.evals, *_perms(self.zs))
        assert np.array_equal(batch.roots, self.roots)
        return ctx, batch


@functools.lru_cache(maxsize=None)
def _case(num_vars, fl):
    return Case(num_vars, fl)


def _assert_streams(case, outs):
    assert len(outs) == B
    for i in range(B):
        got = outs[i] if isinstance(outs[i], np.ndarray) else outs[i].cpu().numpy()
        assert got.shape == (case.len,), i
        assert np.array_equal(got, case.want[i]), f"stream {i} differs from the oracle's"


# ------------------------------------------------------------------------------------------- oracle parity
# one row (no u', coeffs NULL) at 0; two rows of one entry at 1; 2^3 and 2^8; 2^12 has 64 rows: two row blocks per
# opening; every limb count
@pytest.mark.parametrize("num_vars,fl", [(0, 4), (1, 4), (3, 4), (8, 4), (12, 4), (8, 2), (8, 3)])
def test_every_stream_equals_the_oracle_and_the_slice_of_open_fields(cabi, num_vars, fl):
    case = _case(num_vars, fl)
    if num_vars == 0:
        assert case.coeffs is None and case.q0 is None and case.u_bytes == 0
    if num_vars == 1:
        assert (case.zs[0].num_rows, case.zs[0].row_len) == (2, 1)
    if num_vars == 12:
        assert case.zs[0].num_rows == 64
    ctx, batch = case.batch(cabi)
    zfs = case.zfields(cabi)
    before, before_codes = cabi.batch_open_each_counts(), cabi.batch_codes_counts()
    outs = batch.open_each(case.coeffs, case.cols, case.q0, zfs)
    after = cabi.batch_open_each_counts()
    assert after[:3] == (before[0] + 1, before[1] + B, before[2] + 1)
    assert after[3] == B * case.len, "one window of five streams, one slot"
    assert cabi.batch_codes_counts() == (before_codes[0], before_codes[1], before_codes[2] + 1)
    _assert_streams(case, outs)
    block = batch.open_fields(case.coeffs, case.cols, case.q0, zfs)
    for i in range(B):
        assert np.array_equal(outs[i], block[i]), i
    batch.free()
    ctx.close()


def test_a_stream_passes_the_unchanged_zip_verify(cabi):
    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    outs = batch.open_each(case.coeffs, case.cols, case.q0, case.zfields(cabi), window_bytes=2 * case.len)
    i = 3  # 2^255 - 19: no quirk, so the reference's verifier accepts its own proofs
    z, f = case.zs[i], case.fs[i]
    own = _ctx(cabi, z)
    q1 = orc.build_eq_x_r(f, case.points[i][: case.num_vars - case.lr])
    ev = np.array(orc.int_to_limbs(z.mle_eval(f, case.evals[i], case.points[i]), case.fl), dtype=np.uint64)
    rep = own.verify(case.roots[i], outs[i], case.coeffs[i], case.cols[i], case.q0[i], q1, ev, case.zfields(cabi)[i])
    assert rep == {"verdict": cabi.VERIFY_ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    bad = outs[i].copy()
    bad[case.u_bytes + 5 * case.col_bytes + 3] ^= 1
    assert own.verify(case.roots[i], bad, case.coeffs[i], case.cols[i], case.q0[i], q1, ev, case.zfields(cabi)[i])["verdict"] != cabi.VERIFY_ACCEPT
    own.close()
    batch.free()
    ctx.close()


# ------------------------------------------------------------------------------------------------ windows
# 2 * len: windows of 2, 2, 1; len - 1: W = 1, five windows; 0: 64 MiB, one window; 3 * len + 1: windows of 3, 2
@pytest.mark.parametrize("setting", ["2len", "len-1", "0", "3len+1"])
def test_windows(cabi, setting):
    case = _case(8, 4)
    n = case.len
    window_bytes = {"2len": 2 * n, "len-1": n - 1, "0": 0, "3len+1": 3 * n + 1}[setting]
    W = min(B, max(1, (window_bytes or (64 << 20)) // n))
    assert W == {"2len": 2, "len-1": 1, "0": 5, "3len+1": 3}[setting]
    ctx, batch = case.batch(cabi)
    ctx.set_profiling(True)
    before = cabi.batch_open_each_counts()
    outs = batch.open_each(case.coeffs, case.cols, case.q0, case.zfields(cabi), window_bytes=window_bytes)
    after = cabi.batch_open_each_counts()
    n_windows = -(-B // W)
    assert after[:3] == (before[0] + 1, before[1] + B, before[2] + n_windows)
    assert after[3] == (2 if n_windows > 1 else 1) * W * n
    if setting == "2len":
        assert after[3] <= 4 * n < 5 * n
    _assert_streams(case, outs)
    prof = ctx.profile_read()
    assert set(prof) == EACH_KERNELS and all(v[0] == n_windows for v in prof.values()), prof
    batch.free()
    ctx.close()


def test_no_columns(cabi):
    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    zfs = case.zfields(cabi)
    outs = batch.open_each(case.coeffs, None, case.q0, zfs, window_bytes=2 * ctx.proof_len(0, case.fl))
    block = batch.open_fields(case.coeffs, np.zeros((B, 0), dtype=np.uint32), case.q0, zfs)
    for i in range(B):
        assert outs[i].size == case.u_bytes + case.row_bytes
        assert np.array_equal(outs[i], block[i]), i
        assert np.array_equal(outs[i], np.concatenate([case.want[i][: case.u_bytes], case.want[i][case.len - case.row_bytes:]])), i
    batch.free()
    ctx.close()


# -------------------------------------------------------------------------------------- HOST destinations
def _guarded(case):
    """five buffers filled with the guard byte, the destination at an odd address some 37 bytes inside each"""
    bufs = [np.full(case.len + 80, GUARD, dtype=np.uint8) for _ in range(B)]
    dsts = []
    for b in bufs:
        lo = 37 if (b.ctypes.data + 37) % 2 else 38
        dsts.append(b[lo: lo + case.len])
    assert all(d.ctypes.data % 2 == 1 for d in dsts)
    return bufs, dsts


@pytest.mark.parametrize("registered", [False, True], ids=["pageable", "registered"])
def test_host_destinations_at_odd_offsets_inside_guards(cabi, registered):
    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    bufs, dsts = _guarded(case)
    if registered:
        for b in bufs:
            assert cabi.lib().zip_host_register(b.ctypes.data, b.nbytes) == 0
    try:
        outs = batch.open_each(case.coeffs, case.cols, case.q0, case.zfields(cabi), outs=dsts, window_bytes=2 * case.len)
    finally:
        if registered:
            for b in bufs:
                cabi.lib().zip_host_unregister(b.ctypes.data)
    _assert_streams(case, outs)
    for b, d in zip(bufs, dsts):
        lo = d.ctypes.data - b.ctypes.data
        assert (b[:lo] == GUARD).all() and (b[lo + case.len:] == GUARD).all()
    batch.free()
    ctx.close()


def test_host_destinations_in_reverse_order(cabi):
    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    whole = np.full(B * (case.len + 16) + 16, GUARD, dtype=np.uint8)
    # member i's destination is the (B - 1 - i)-th slice: the addresses fall as the members rise
    dsts = [whole[16 + (B - 1 - i) * (case.len + 16):][: case.len] for i in range(B)]
    assert all(dsts[i].ctypes.data > dsts[i + 1].ctypes.data for i in range(B - 1))
    batch.open_each(case.coeffs, case.cols, case.q0, case.zfields(cabi), outs=dsts, window_bytes=2 * case.len)
    _assert_streams(case, dsts)
    keep = np.ones(whole.size, dtype=bool)
    for i in range(B):
        lo = 16 + i * (case.len + 16)
        keep[lo: lo + case.len] = False
    assert (whole[keep] == GUARD).all()
    batch.free()
    ctx.close()


# ------------------------------------------------------------------------------------ DEVICE destinations
def test_device_destinations_shuffled_at_8_mod_16_with_guards(cabi):
    import torch

    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    stride = (case.len + 16 + 15) // 16 * 16  # a multiple of 16: every slice starts at 8 mod 16
    whole = torch.full((8 + B * stride + 16,), GUARD, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    place = [3, 0, 4, 1, 2]  # member i -> slice place[i]
    dsts = [whole[8 + place[i] * stride: 8 + place[i] * stride + case.len] for i in range(B)]
    assert all(d.data_ptr() % 16 == 8 for d in dsts)
    torch.cuda.synchronize()  # torch fills on its own stream; the library writes on the ctx's, which does not wait for it
    ctx.set_profiling(True)
    before = cabi.batch_open_each_counts()
    batch.open_each(case.coeffs, case.cols, case.q0, case.zfields(cabi), outs=dsts, out_kind=cabi.MEM_DEVICE, window_bytes=case.len)
    after = cabi.batch_open_each_counts()
    assert after == (before[0] + 1, before[1] + B, before[2] + 1, 0), "no staging, one window whatever window_bytes says"
    prof = ctx.profile_read()
    assert set(prof) == EACH_KERNELS and all(v[0] == 1 for v in prof.values()), prof
    host = whole.cpu().numpy()
    keep = np.ones(host.size, dtype=bool)
    for i in range(B):
        lo = 8 + place[i] * stride
        assert np.array_equal(host[lo: lo + case.len], case.want[i]), i
        keep[lo: lo + case.len] = False
    assert (host[keep] == GUARD).all(), "the guard bytes between the slices"
    # fresh device buffers when none are given
    outs = batch.open_each(case.coeffs, case.cols, case.q0, case.zfields(cabi), out_kind=cabi.MEM_DEVICE)
    _assert_streams(case, outs)
    batch.free()
    ctx.close()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_reach_no_device_and_leave_the_batch_usable(cabi):
    import torch

    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    zfs = case.zfields(cabi)
    cw = case.zs[0].codeword_len
    ctx.set_profiling(True)
    ctx.profile_read()
    before, before_codes = cabi.batch_open_each_counts(), cabi.batch_codes_counts()

    def refused(code, cols=case.cols, **kw):
        with pytest.raises(cabi.ZipError) as e:
            batch.open_each(case.coeffs, cols, case.q0, zfs, **kw)
        assert e.value.code == code, kw
        assert ctx.profile_read() == {}, "a launch"
        assert cabi.batch_open_each_counts() == before and cabi.batch_codes_counts() == before_codes

    host = [np.full(case.len, GUARD, dtype=np.uint8) for _ in range(B)]
    refused(cabi.ZIP_ERR_NULL, outs=host[:2] + [None] + host[3:])
    dev = torch.full((B * (case.len + 8) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    slices = [dev[i * (case.len + 8):][: case.len] for i in range(B)]
    assert all(s.data_ptr() % 8 == 0 for s in slices)
    refused(cabi.ZIP_ERR_INVALID_PARAM, outs=slices[:4] + [slices[4].data_ptr() + 4], out_kind=cabi.MEM_DEVICE)
    # overlap: member 4's range begins inside member 1's, on the device and on the host
    refused(cabi.ZIP_ERR_INVALID_PARAM, outs=slices[:4] + [slices[1].data_ptr() + case.len - 8], out_kind=cabi.MEM_DEVICE)
    refused(cabi.ZIP_ERR_INVALID_PARAM, outs=host[:4] + [host[1].ctypes.data + case.len - 1])
    refused(cabi.ZIP_ERR_INVALID_PARAM, outs=host[:4] + [host[0]])
    bad_cols = case.cols.copy()
    bad_cols[4, N_COLS - 1] = cw
    refused(cabi.ZIP_ERR_INVALID_PARAM, cols=bad_cols, outs=host)
    ctx.set_proximity_tests(2)
    refused(cabi.ZIP_ERR_UNSUPPORTED, outs=host)
    ctx.set_proximity_tests(1)
    # the raw call: no table at all
    arr = cabi.Batch._field_ptrs(zfs)
    rc = cabi.lib().zip_batch_open_each(batch._h, case.coeffs.ctypes.data, case.cols.ctypes.data, N_COLS, case.q0.ctypes.data,
                                        C.cast(arr, C.c_void_p), None, cabi.MEM_HOST, 0)
    assert rc == cabi.ZIP_ERR_NULL
    assert all((h == GUARD).all() for h in host) and (dev.cpu().numpy() == GUARD).all(), "a refused call wrote"
    assert cabi.batch_open_each_counts() == before
    # the same batch then opens correctly
    outs = batch.open_each(case.coeffs, case.cols, case.q0, zfs, outs=host, window_bytes=2 * case.len)
    _assert_streams(case, outs)
    assert cabi.batch_open_each_counts()[:3] == (before[0] + 1, before[1] + B, before[2] + 3)
    batch.free()
    ctx.close()


# ------------------------------------------------------------------------------------- unchanged launches
def test_open_fields_still_launches_what_it_launched(cabi):
    case = _case(8, 4)
    ctx, batch = case.batch(cabi)
    zfs = case.zfields(cabi)
    ctx.set_profiling(True)
    ctx.profile_read()
    before = cabi.batch_open_each_counts()
    block = batch.open_fields(case.coeffs, case.cols, case.q0, zfs)
    prof = ctx.profile_read()
    assert set(prof) == FIELDS_KERNELS and all(v[0] == 1 for v in prof.values()), prof
    assert cabi.batch_open_each_counts() == before
    for i in range(B):
        assert np.array_equal(block[i], case.want[i]), i
    batch.free()
    ctx.close()
