"""GPU parity of the batched verifier with a code, a field and a stream buffer per member (zip_batch_verify_codes): report
for report against zip_verify on a ctx created with THAT member's permutations and field (which tests/test_gpu_verify*.py
pin to the oracle).  The honest proofs are the oracle's own commit + open, per member in its own field.  The C ABI takes
`cols` directly, so the column counts are small: 7, and 300 where the report kernel's strided loop takes a second pass.
Needs a real MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import _oracle as orc
import _verify_cases as vc
from test_gpu_batch_codes import BENCH_MODULUS, MOD_NO_SPARE, MODULI, SEEDS

pytestmark = pytest.mark.gpu

ACCEPTED = {"verdict": vc.ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
SHORT = {"verdict": vc.MALFORMED, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
B = 5
# name -> (num_vars, geometry or None for the reference's own, openings)
SHAPES = {"one-row": (0, None, 7), "2^3": (3, None, 7), "2^8": (8, None, 300), "2^12": (12, None, 7),
          "tall": (*vc.GEOMETRIES["tall"], 7), "wide": (*vc.GEOMETRIES["wide"], 300)}


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


class Members:
    """B honest proofs, member i under its own code (SEEDS[i]) and in its own field (MODULI[fl][i]), each on a fresh
    transcript.  Members 0 and 1 share the witness and the point.  Built once per shape and never modified."""

    def __init__(self, shape, fl):
        num_vars, geometry, n_cols = SHAPES[shape]
        self.fl, self.n_cols, self.mods = fl, n_cols, MODULI[fl]
        self.zs = [orc.Zip(num_vars, seeds=SEEDS[i], geometry=geometry) for i in range(B)]
        for z in self.zs:
            z.p.num_column_opening = n_cols
        z = self.zs[0]
        self.fs = [orc.make_field(m, fl) for m in self.mods]
        lr = z.num_rows.bit_length() - 1
        rng = np.random.default_rng(3 + num_vars)
        w = _witness(num_vars, 7, fl == 2)
        self.evals = [w, w] + [_witness(num_vars, 8 + i, fl == 2) for i in range(B - 2)]
        p0 = rng.integers(-100, 100, size=num_vars, dtype=np.int64)
        pts = [p0, p0] + [rng.integers(-100, 100, size=num_vars, dtype=np.int64) for _ in range(B - 2)]
        self.points = [orc.point_to_field(f, p) if num_vars else np.zeros((0, fl), dtype=np.uint64) for f, p in zip(self.fs, pts)]
        roots, self.proofs, cols, coeffs, q0, q1, self.evs = [], [], [], [], [], [], []
        for z_i, f, ev, pt in zip(self.zs, self.fs, self.evals, self.points):
            rows_o, layers_o, roots_o = z_i.commit(ev)
            proof, c, k = z_i.open(f, ev, rows_o, layers_o, pt, orc.new_transcript())
            assert proof.size == z_i.proof_len(fl)
            proof.setflags(write=False)
            roots.append(roots_o)
            self.proofs.append(proof)
            cols.append(c.copy())
            coeffs.append(k.copy())
            if lr:
                q0.append(orc.build_eq_x_r(f, pt[num_vars - lr:]))
            if num_vars - lr:
                q1.append(orc.build_eq_x_r(f, pt[: num_vars - lr]))
            self.evs.append(z_i.mle_eval(f, ev, pt))
        self.len = z.proof_len(fl)
        self.roots, self.cols = np.stack(roots), np.stack(cols)
        self.coeffs = np.stack(coeffs) if lr else None
        self.q0 = np.stack(q0) if lr else None
        self.q1 = np.stack(q1) if num_vars - lr else None
        self.perms1, self.perms2 = np.stack([z.perm1 for z in self.zs]), np.stack([z.perm2 for z in self.zs])
        self.shared_ctx_code = orc.Zip(num_vars, seeds=(9, 9), geometry=geometry)  # the ctx's own permutations are nobody's
        self._want = None

    def ev_limbs(self, evs=None):
        return np.array([orc.int_to_limbs(e, self.fl) for e in (self.evs if evs is None else evs)], dtype=np.uint64)

    def zfields(self, cabi):
        return [cabi.make_field(m, self.fl) for m in self.mods]

    def verify_one(self, cabi, i, proof=None, roots=None, ev=None, code=None, field=None):
        """zip_verify of member i's slices on a ctx created with its (or `code`'s) permutations: the yardstick"""
        own = _ctx(cabi, self.zs[i if code is None else code])
        zf = cabi.make_field(self.mods[i if field is None else field], self.fl)
        pick = lambda a: None if a is None else a[i]
        rep = own.verify(self.roots[i] if roots is None else roots, self.proofs[i] if proof is None else proof, pick(self.coeffs),
                         self.cols[i], pick(self.q0), pick(self.q1), self.ev_limbs()[i] if ev is None else ev, zf)
        own.close()
        return rep

    def want(self, cabi):
        """zip_verify's reports of the honest members: computed once, shared"""
        if self._want is None:
            self._want = [self.verify_one(cabi, i) for i in range(B)]
        return [dict(r) for r in self._want]

    def run(self, cabi, ctx=None, proofs=None, roots=None, evs=None, perms=None, fields=None, proof_lens=None):
        ctx = ctx or _ctx(cabi, self.shared_ctx_code)
        p1, p2 = perms or (self.perms1, self.perms2)
        return ctx.batch_verify_codes(p1, p2, self.roots if roots is None else roots, self.proofs if proofs is None else proofs,
                                      self.coeffs, self.cols, self.q0, self.q1, self.ev_limbs(evs),
                                      fields or self.zfields(cabi), proof_lens=proof_lens)


@functools.lru_cache(maxsize=None)
def _members(shape, fl):
    return Members(shape, fl)


# ------------------------------------------------------------------------------------------------ honest proofs
@pytest.mark.parametrize("fl", [2, 3, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_honest_members_equal_zip_verify_on_their_own_ctx(cabi, shape, fl):
    m = _members(shape, fl)
    z = m.zs[0]
    want = m.want(cabi)
    before = cabi.batch_verify_codes_counts()
    got = m.run(cabi)
    print(shape, fl, got)
    assert cabi.batch_verify_codes_counts() == (before[0] + 1, before[1] + B)
    assert got == want
    for i in range(B):  # what zip_verify accepts of the reference's own proofs: more than one column, and no modulus
        # that the reference reads as a small negative integer (2^256 - 189 and its like: tests/test_gpu_batch_verify.py)
        if z.row_len > 1 and (1 << (64 * fl)) - m.mods[i] >= 1 << 64:
            assert got[i] == ACCEPTED, i
    if fl == 4:
        assert m.mods[0] == MOD_NO_SPARE and m.mods[1] == BENCH_MODULUS  # a batch that mixes quirk and no quirk


@pytest.mark.parametrize("shape,fl", [("2^8", 4), ("2^3", 3), ("wide", 2)])
def test_device_streams_give_the_same_reports(cabi, shape, fl):
    import torch

    m = _members(shape, fl)
    dev = [torch.from_numpy(p.copy()).cuda() for p in m.proofs]
    torch.cuda.synchronize()
    assert m.run(cabi, proofs=dev) == m.want(cabi)
    # a stream one byte off an 8-byte boundary is refused before anything runs
    pad = torch.zeros(m.len + 8, dtype=torch.uint8, device="cuda")
    before = cabi.batch_verify_codes_counts()
    with pytest.raises(cabi.ZipError) as e:
        m.run(cabi, proofs=dev[:3] + [pad[1: 1 + m.len]] + dev[4:])
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    assert cabi.batch_verify_codes_counts() == before


def test_the_ctx_own_permutations_change_nothing(cabi):
    m = _members("2^8", 4)
    for code in (m.zs[0], m.zs[3], m.shared_ctx_code):
        assert m.run(cabi, ctx=_ctx(cabi, code)) == m.want(cabi)


# ------------------------------------------------------------- a kernel that reads slice 0 for everyone must fail
@pytest.mark.parametrize("shape,fl", [("2^8", 4), ("2^12", 3), ("tall", 2), ("wide", 4)])
def test_swapped_codes_and_swapped_fields_reject_both_members(cabi, shape, fl):
    m = _members(shape, fl)
    want = m.want(cabi)
    assert np.array_equal(m.evals[0], m.evals[1])      # the same witness
    assert not np.array_equal(m.roots[0], m.roots[1])  # under different codes
    swap = [1, 0, 2, 3, 4]
    got = m.run(cabi, perms=(m.perms1[swap], m.perms2[swap]))
    print("codes", got)
    assert got[0]["verdict"] != vc.ACCEPT and got[1]["verdict"] != vc.ACCEPT
    assert got[2:] == want[2:]
    assert got[0] == m.verify_one(cabi, 0, code=1) and got[1] == m.verify_one(cabi, 1, code=0)
    zf = m.zfields(cabi)
    got = m.run(cabi, fields=[zf[j] for j in swap])  # q0, q1 and the evaluations stay in the members' own fields
    print("fields", got)
    assert got[0]["verdict"] != vc.ACCEPT and got[1]["verdict"] != vc.ACCEPT
    assert got[2:] == want[2:]
    assert got[0] == m.verify_one(cabi, 0, field=1) and got[1] == m.verify_one(cabi, 1, field=0)


# ------------------------------------------------------------------------------------------------ tampered members
# a member whose modulus has no quirk for every limb count, and whose opened columns are of both parities (the
# catalogue's path cases want an even and an odd one; under 2^127 - 1 every squeezed column is even)
TAMPERED = 3


@functools.lru_cache(maxsize=None)
def _tamper_cases(shape, fl):
    """One case of tests/_verify_cases.py's catalogue per verdict, built on member TAMPERED's own proof"""
    m = _members(shape, fl)
    i = TAMPERED
    inst = vc.Instance(m.zs[i], m.mods[i], fl, m.fs[i], m.points[i], m.roots[i], m.proofs[i], m.cols[i], m.coeffs[i], m.q0[i],
                       m.q1[i], m.evs[i])
    pool = vc.value_cases(inst) + vc.position_cases(inst) + vc.overflow_cases(inst)
    pool.append(vc.Case("evaluation row consistent with its claim, rows are not", vc._q0_only(inst, 1), verdict=vc.PROXIMITY_Q0,
                        bad_merkle_paths=0, malformed_paths=0))
    out = {}
    for c in pool:
        proof, roots, ev = c.mutate(inst.proof, inst.roots, inst.ev)
        if proof.size == inst.need and c.claim["verdict"] not in out:
            out[c.claim["verdict"]] = (c, proof, roots, ev)
    return out


@pytest.mark.parametrize("verdict", [vc.PROXIMITY_TESTING, vc.EVAL_CONSISTENCY, vc.PROXIMITY_Q0, vc.MERKLE, vc.MALFORMED, vc.OVERFLOW],
                         ids=lambda v: vc.VERDICT_NAMES[v])
@pytest.mark.parametrize("shape,fl", [("2^8", 4), ("2^8", 2), ("tall", 3)])
def test_one_tampered_member_among_honest_ones(cabi, shape, fl, verdict):
    m = _members(shape, fl)
    c, proof, roots, ev = _tamper_cases(shape, fl)[verdict]
    i = TAMPERED
    proofs = list(m.proofs)
    proofs[i] = proof
    all_roots = m.roots.copy()
    all_roots[i] = roots
    evs = list(m.evs)
    evs[i] = ev
    got = m.run(cabi, proofs=proofs, roots=all_roots, evs=evs)
    print(shape, fl, c.name, got[i])
    want = m.want(cabi)
    assert got[:i] == want[:i] and got[i + 1:] == want[i + 1:]  # the neighbours' reports do not change
    assert got[i] == m.verify_one(cabi, i, proof=proof, roots=roots, ev=np.array(orc.int_to_limbs(ev, fl), dtype=np.uint64))
    assert got[i]["verdict"] == verdict
    for k, v in c.claim.items():
        assert got[i][k] == v, (c.name, k)


# ------------------------------------------------------------------------------------------------ short members
def test_a_short_member_is_malformed_and_the_others_are_verified(cabi):
    m = _members("2^8", 4)
    want = m.want(cabi)
    lens = [m.len] * B
    lens[0] = m.len - 1
    lens[3] = 0
    before = cabi.batch_verify_codes_counts()
    got = m.run(cabi, proof_lens=lens)
    assert cabi.batch_verify_codes_counts() == (before[0] + 1, before[1] + 3)
    assert got[0] == SHORT and got[3] == SHORT
    assert [got[i] for i in (1, 2, 4)] == [want[i] for i in (1, 2, 4)]
    # nobody long enough: nothing reaches the device
    assert m.run(cabi, proof_lens=[m.len - 1] * B) == [SHORT] * B
    assert cabi.batch_verify_codes_counts() == (before[0] + 1, before[1] + 3)
    # longer than needed is allowed, as for zip_verify
    longer = [np.concatenate([p, np.arange(7, 47, dtype=np.uint8)]) for p in m.proofs]
    assert m.run(cabi, proofs=longer) == want


# ------------------------------------------------------------------------------------------------ usage errors
def test_usage_errors_reach_no_device(cabi):
    m = _members("2^8", 4)
    z = m.zs[0]
    ctx = _ctx(cabi, m.shared_ctx_code)
    before = cabi.batch_verify_codes_counts()

    def code_of(**kw):
        with pytest.raises(cabi.ZipError) as e:
            m.run(cabi, ctx=ctx, **kw)
        return e.value.code

    rep = m.perms1.copy()
    rep[4, 5] = rep[4, 6]  # a repeated index, in the last member
    assert code_of(perms=(rep, m.perms2)) == cabi.ZIP_ERR_INVALID_PARAM
    big = m.perms2.copy()
    big[2, 0] = z.codeword_len
    assert code_of(perms=(m.perms1, big)) == cabi.ZIP_ERR_INVALID_PARAM
    zf = m.zfields(cabi)
    assert code_of(fields=zf[:4] + [cabi.make_field(MODULI[3][0], 3)]) == cabi.ZIP_ERR_INVALID_PARAM  # differing limb counts
    assert code_of(fields=zf[:4] + [cabi.make_field(BENCH_MODULUS - 1, 4)]) == cabi.ZIP_ERR_INVALID_PARAM  # an even modulus
    assert code_of(fields=zf[:4] + [None]) == cabi.ZIP_ERR_NULL
    assert code_of(fields=zf[:4] + [None], perms=(rep, m.perms2)) == cabi.ZIP_ERR_NULL  # the permutations are looked at last
    shard = _ctx(cabi, z, row_begin=0, row_count=z.num_rows // 2)
    with pytest.raises(cabi.ZipError) as e:
        m.run(cabi, ctx=shard)
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    L = cabi.lib()
    reps = (cabi.VerifyReport * B)()
    assert L.zip_batch_verify_codes(ctx._h, B, None, m.perms2.ctypes.data, m.roots.ctypes.data, None, None, cabi.MEM_HOST, None, None, 0,
                                    None, None, None, None, reps) == cabi.ZIP_ERR_NULL
    assert cabi.batch_verify_codes_counts() == before
    assert m.run(cabi, ctx=ctx) == m.want(cabi)  # the ctx is still usable
