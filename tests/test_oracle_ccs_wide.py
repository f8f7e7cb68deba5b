"""CPU: the oracle on CCS with four to seven matrices and on sumchecks over eight MLEs -- shapes the yardstick had not
been run on before the device prover took them.  The instances hold in Python integers; the oracle's Spartan verifier
accepts its own proofs on the fields whose FieldMap keeps the integer identity and rejects a wrong witness; the
oracle's sumcheck prover over eight tables equals a restatement in Python big integers."""
import numpy as np
import pytest

import _ccs_wide
import _oracle as orc

Q192 = 312829638388039969874974628075306023441          # zinc/tests.rs:28
QSTARK = 3618502788666131213697322783095070105623107215331596699973092056135872020481  # spartan_benches.rs:161
Q128 = 57316695564490278656402085503
ACCEPTING_FIELDS = [(Q192, 3), (Q128, 2), (QSTARK, 4)]
BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
MOD_NO_SPARE = (1 << 256) - 189


@pytest.mark.parametrize("s", [1, 3, 6])
@pytest.mark.parametrize("name", list(_ccs_wide.SHAPES))
def test_instances_hold_in_integers(name, s):
    inst = _ccs_wide.instance(name, s)
    S, _ = _ccs_wide.SHAPES[name]
    assert inst.t == sum(len(Si) for Si in S) and inst.q == len(S) and inst.d == max(len(Si) for Si in S)
    assert inst.m == inst.n == 1 << s and int(inst.z[0]) == 3 and int(inst.z[1]) == 1
    assert _ccs_wide.row_identity_holds(inst)
    if s >= 3:
        assert not _ccs_wide.row_identity_holds(_ccs_wide.bumped(inst))


@pytest.mark.parametrize("q,fl", ACCEPTING_FIELDS)
@pytest.mark.parametrize("s", [1, 3, 6])
@pytest.mark.parametrize("name", list(_ccs_wide.SHAPES))
def test_oracle_verifier_accepts_and_rejects(name, s, q, fl):
    f = orc.make_field(q, fl)
    inst = _ccs_wide.instance(name, s)
    o = orc.Ccs(inst)
    proof = o.spartan_prove(f, orc.new_transcript())
    assert proof["msgs1"].shape == (s, inst.d + 2, fl) and proof["V_s"].shape == (inst.t, fl)
    rc, pts = o.spartan_verify(f, proof, orc.new_transcript())
    assert rc == 0 and np.array_equal(pts["r_y"], proof["r_y"])
    if s >= 3:
        bad = orc.Ccs(_ccs_wide.bumped(inst))
        assert bad.spartan_verify(f, bad.spartan_prove(f, orc.new_transcript()), orc.new_transcript())[0] == orc.ORC_ERR_PROOF


def _interp(ys, x, q):
    """value at x of the polynomial through (0, ys[0]), (1, ys[1]), ...  (interpolate_uni_poly, verifier.rs:161-)"""
    acc = 0
    for i, yi in enumerate(ys):
        num, den = 1, 1
        for j in range(len(ys)):
            if j != i:
                num = num * (x - j) % q
                den = den * (i - j) % q
        acc = (acc + yi * num * pow(den, -1, q)) % q
    return acc


MASKS_8 = [0b0000111, 0b0011000, 0b0100000, 0b1000000]


@pytest.mark.parametrize("modulus,fl", [(BENCH_MODULUS, 4), (Q128, 2), (Q192, 3), (MOD_NO_SPARE, 4)])
@pytest.mark.parametrize("nv", [1, 2, 4])
def test_eight_mle_sumcheck_equals_python_integers(modulus, fl, nv):
    """comb = (c0 v0 v1 v2 + c1 v3 v4 + c2 v5 + c3 v6) * v7, degree 4: every round message is the sum over the cube of
    comb at t = 0..4 of the tables folded with the challenges so far (prover.rs:62-180), and continues the round before."""
    q, K, degree = modulus, 8, 4
    f = orc.make_field(q, fl)
    R = 1 << (64 * fl)
    R_inv = pow(R, -1, q)
    rng = np.random.default_rng(80 + nv)
    n = 1 << nv
    std = [[int.from_bytes(rng.bytes(40), "little") % q for _ in range(n)] for _ in range(K)]
    c = [5, q - 1, int.from_bytes(rng.bytes(40), "little") % q, q - 7]
    mles = np.stack([orc.field_elems([v * R % q for v in t], fl) for t in std])
    msgs, rand = orc.sumcheck_prove(f, mles, degree, MASKS_8, [x * R % q for x in c], orc.new_transcript())
    g = [[orc.limbs_to_int(msgs[i, e]) * R_inv % q for e in range(degree + 1)] for i in range(nv)]
    r = [orc.limbs_to_int(rand[i]) * R_inv % q for i in range(nv)]

    def comb(v):
        total = 0
        for ct, m in zip(c, MASKS_8):
            p = ct
            for j in range(K):
                if (m >> j) & 1:
                    p = p * v[j] % q
            total += p
        return total * v[K - 1] % q

    cur = [t[:] for t in std]
    for i in range(nv):
        half = len(cur[0]) // 2
        for e in range(degree + 1):
            want = sum(comb([(t[2 * b] + e * (t[2 * b + 1] - t[2 * b])) % q for t in cur]) for b in range(half)) % q
            assert g[i][e] == want, (i, e)
        if i:
            assert (g[i][0] + g[i][1]) % q == _interp(g[i - 1], r[i - 1], q)
        cur = [[(t[2 * b] + r[i] * (t[2 * b + 1] - t[2 * b])) % q for b in range(half)] for t in cur]
    assert comb([t[0] for t in cur]) == _interp(g[-1], r[-1], q)
    # the challenges are the transcript's (sumcheck.rs:64-106)
    replay = orc.new_transcript()
    orc.absorb_field(replay, f, orc.field_from_u128(f, nv))
    orc.absorb_field(replay, f, orc.field_from_u128(f, degree))
    for i in range(nv):
        for e in range(degree + 1):
            orc.absorb_field(replay, f, orc.limbs_to_int(msgs[i, e]))
        ri = orc.get_challenge(replay, f)
        assert ri == orc.limbs_to_int(rand[i])
        orc.absorb_field(replay, f, ri)
