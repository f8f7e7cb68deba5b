"""GPU: zip_verify on a ctx set to T > 1 proximity tests (verify_z.rs:66-103), held to a model written here.

The model.  Per test t, enc_t = Zip.encode_row(u'_t) on the oracle, whose return code is the overflow fact; the proximity
fact of opening i is whether sum_r coeffs_t[r] * v[r], in Python integers, differs from enc_t[col_i] for ANY t.  Every
fact that does not depend on T -- evaluation consistency, q0 proximity, Merkle, malformed, non-canonical -- comes from
zip_verify on a ONE-test ctx, which the existing suite holds to the oracle: it gets the stream with u'_1 .. u'_{T-1} cut
out, test 0's coefficients and the same columns.  Its counts do not depend on its verdict, so called on one opening at
a time it also tells which openings have a wrong prefix or a wrong path.  The facts then go through the cascade of
verify_verdict.h: overflow; per opening in order proximity, prefix, path; evaluation; non-canonical; q0.  Whatever test
0's proximity failure hides in the one-test run is hidden by the any-test failure at the same opening here too."""
import numpy as np
import pytest

import _oracle as orc
import _proximity as px

pytestmark = pytest.mark.gpu

N_COLS = 8
ACCEPT, PROXIMITY_TESTING, EVAL_CONSISTENCY, PROXIMITY_Q0, MERKLE, MALFORMED, OVERFLOW = range(7)
INT8_MAX = (1 << 511) - 1


@pytest.fixture(scope="module")
def cabi():
    from zinc_amd import cabi as m

    if m.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return m


class Verifier:
    """The T-test ctx under test and the one-test ctx the model asks, for one instance."""

    def __init__(self, cabi, i):
        self.cabi, self.i = cabi, i
        geo = (i.C, i.R, i.cw)
        self.ctx = cabi.ZipContext(i.z.num_vars, i.z.perm1, i.z.perm2, geometry_override=geo)
        self.ctx.set_proximity_tests(i.T)
        self.one = cabi.ZipContext(i.z.num_vars, i.z.perm1, i.z.perm2, geometry_override=geo)
        self.zf = cabi.make_field(i.modulus, i.fl)
        self.ev = np.array(orc.int_to_limbs(i.ev, i.fl), dtype=np.uint64)

    def run(self, proof, coeffs=None, ctx=None):
        i = self.i
        coeffs = i.coeffs if coeffs is None else coeffs
        return (ctx or self.ctx).verify(i.roots, proof, coeffs if i.R > 1 else None, i.cols, i.q0, i.q1, self.ev, self.zf)

    def _one(self, stream, coeffs0, cols):
        i = self.i
        return self.one.verify(i.roots, stream, coeffs0, cols, i.q0, i.q1, self.ev, self.zf)

    def expect(self, proof, coeffs=None):
        i, T, C = self.i, self.i.T, self.i.C
        coeffs = i.coeffs if coeffs is None else coeffs
        if proof.size < i.proof.size:  # the reference runs out of stream
            return {"verdict": MALFORMED, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
        u1 = C * 64
        cut = np.concatenate([proof[:u1], proof[T * u1:]])  # u'_0 | columns | row
        rep1 = self._one(cut, coeffs[0], i.cols)
        want = dict(rep1)  # the counts never depend on T
        # ---- the facts that do: overflow and proximity, every test
        us = px.u_primes(proof, i.z, T)
        encs, overflow = [], False
        for t in range(T):
            limbs = np.array([orc.int_to_limbs(x, 8) for x in us[t]], dtype=np.uint64)
            rc, enc = i.z.encode_row(limbs, in_limbs=8, out_limbs=8)
            overflow |= rc != 0
            encs.append(enc)
        if overflow:
            want.update(verdict=OVERFLOW, column=0)
            return want
        cf = [[int(c) for c in coeffs[t]] for t in range(T)]
        first = None
        for k in range(i.n_cols):
            at = i.u_bytes + k * i.col_bytes
            raw = proof[at: at + 32 * i.R].tobytes()
            v = [int.from_bytes(raw[32 * r: 32 * r + 32], "little", signed=True) for r in range(i.R)]
            col = int(i.cols[k])
            prox = any(sum(c * x for c, x in zip(cf[t], v)) != orc.limbs_to_int(encs[t][col], signed=True) for t in range(T))
            mal = bad = 0
            if rep1["bad_merkle_paths"] or rep1["malformed_paths"]:  # where: the one-test verifier, one opening at a time
                blk = proof[at: at + i.col_bytes]
                r = self._one(np.concatenate([proof[:u1], blk, proof[T * u1 + i.n_cols * i.col_bytes:]]), coeffs[0], i.cols[k: k + 1])
                mal, bad = r["malformed_paths"], r["bad_merkle_paths"]
            if prox or mal or bad:
                first = (k, PROXIMITY_TESTING if prox else MALFORMED if mal else MERKLE)
                break
        if first is not None:
            want.update(verdict=first[1], column=first[0])
        # else: no opening fails here, so none fails in the one-test run either, and its verdict is one of the later
        # checks (evaluation, non-canonical, q0) or ACCEPT: rep1's own
        else:
            assert rep1["verdict"] in (ACCEPT, EVAL_CONSISTENCY, MALFORMED, PROXIMITY_Q0)
        return want


@pytest.mark.parametrize("T", [2, 3, 8])
@pytest.mark.parametrize("num_vars", [13, 16, 18])
def test_honest_oracle_proofs_are_accepted(cabi, num_vars, T):
    """64, 256 and 512 rows: one pass of the rows, exactly one, and two per thread of verify_extra_tests_kernel."""
    i = px.instance(num_vars, T, n_cols=N_COLS)
    v = Verifier(cabi, i)
    assert v.run(i.proof) == {"verdict": ACCEPT, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    assert v.expect(i.proof)["verdict"] == ACCEPT


@pytest.mark.parametrize("T", [2, 8])
def test_one_row_matrix_has_no_test(cabi, T):
    i = px.make(4, T, n_cols=3, geometry=(16, 1, 32))
    assert i.R == 1 and i.u_bytes == 0
    v = Verifier(cabi, i)
    assert v.ctx.proof_len(3, i.fl) == i.proof.size == v.one.proof_len(3, i.fl)
    assert v.run(i.proof)["verdict"] == ACCEPT


@pytest.mark.parametrize("num_vars,T", [(13, 2), (16, 3), (18, 8)])
def test_the_devices_own_proofs_are_accepted_from_device_memory(cabi, num_vars, T):
    torch = pytest.importorskip("torch")
    i = px.instance(num_vars, T, n_cols=N_COLS)
    v = Verifier(cabi, i)
    out = torch.empty(i.proof.size, dtype=torch.uint8, device="cuda")
    _, roots, _ = v.ctx.commit_open(i.evals, i.coeffs, i.cols, i.q0, v.zf, out=out)
    assert np.array_equal(roots, i.roots)
    assert v.run(out)["verdict"] == ACCEPT


def _flip(proof, at, xor=1):
    p = proof.copy()
    p[at] ^= xor
    return p


def _with_u(i, proof, t, c, value):
    p = proof.copy()
    at = (t * i.C + c) * 64
    p[at: at + 64] = np.frombuffer(int(value).to_bytes(64, "little", signed=True), dtype=np.uint8)
    return p


@pytest.mark.parametrize("num_vars,T", [(13, 3), (18, 3), (13, 8)])
def test_rejections_follow_the_model(cabi, num_vars, T):
    i = px.instance(num_vars, T, n_cols=N_COLS)
    v = Verifier(cabi, i)
    u1 = i.C * 64
    node = lambda k, r, lvl: i.u_bytes + k * i.col_bytes + 32 * i.R + r * (8 + 32 * i.d) + 8 + 32 * lvl + 3
    val = lambda k, r: i.u_bytes + k * i.col_bytes + 32 * r
    wrong = i.coeffs.copy()
    wrong[1, 5] ^= 1
    flipped = _flip(i.proof, val(3, i.R - 1))
    cases = {
        "bit in u'_0 only": (_flip(i.proof, 5 * 64 + 1), None, PROXIMITY_TESTING),
        "bit in u'_1 only": (_flip(i.proof, u1 + 2 * 64), None, PROXIMITY_TESTING),
        "bit in u'_{T-1} only": (_flip(i.proof, (T - 1) * u1 + 64 * (i.C - 1) + 9), None, PROXIMITY_TESTING),
        "wrong coefficient in one vector": (i.proof, wrong, PROXIMITY_TESTING),
        "encode_wide overflow in the last test only": (_with_u(i, i.proof, T - 1, 0, INT8_MAX), None, OVERFLOW),
        "flipped column value": (flipped, None, PROXIMITY_TESTING),
        "bad path before the first proximity failure": (_flip(flipped, node(1, 2, 4)), None, MERKLE),
        "bad path after the first proximity failure": (_flip(flipped, node(5, i.R - 2, 0)), None, PROXIMITY_TESTING),
        "wrong prefix before the first proximity failure": (_flip(flipped, node(1, 2, 0) - 8 - 3 + 7), None, MALFORMED),
        "evaluation row": (_flip(i.proof, i.proof.size - 9), None, EVAL_CONSISTENCY),
        "stream short by one u' row": (i.proof[: i.proof.size - u1], None, MALFORMED),
        "untouched": (i.proof, None, ACCEPT),
    }
    for name, (proof, coeffs, verdict) in cases.items():
        want = v.expect(proof, coeffs)
        got = v.run(proof, coeffs)
        assert want["verdict"] == verdict, (name, want)  # the model says what the case was built to provoke
        assert got == want, name
    assert v.run(cases["flipped column value"][0])["column"] == 3
    assert v.run(cases["bad path before the first proximity failure"][0])["column"] == 1
    rep = v.run(cases["bad path after the first proximity failure"][0])
    assert rep["column"] == 3 and rep["bad_merkle_paths"] == 2  # the flipped value's own path, and the flipped node


def test_a_proof_made_with_two_tests_checked_with_three(cabi):
    two, three = px.instance(13, 2, n_cols=N_COLS), px.instance(13, 3, n_cols=N_COLS)
    v = Verifier(cabi, three)
    assert two.proof.size == three.proof.size - two.C * 64
    assert not np.array_equal(two.cols, three.cols)  # one more squeeze of num_rows coefficients moves the columns
    rep = v.run(two.proof)  # the stream ends one proximity row early
    assert rep == {"verdict": MALFORMED, "column": 0, "bad_merkle_paths": 0, "malformed_paths": 0}
    # ... and with room to read past its end, the columns the three-test verifier squeezes are not the ones opened
    padded = np.concatenate([two.proof, np.zeros(two.C * 64, dtype=np.uint8)])
    assert v.run(padded)["verdict"] != ACCEPT

