"""GPU: sumchecks over five to eight MLEs (sumcheck_round_wide_kernel: eight lanes per hypercube point) against the
oracle's MLSumcheck::prove_as_subprotocol -- every round message, every challenge and the transcript afterwards, bit
for bit; round by round through the host mirror and in one call (zip_sumcheck_prove, whose tail kernel takes the last
rounds)."""
import functools
import os

import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

TEST_MODULUS_2 = 57316695564490278656402085503
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
MOD_NO_SPARE = (1 << 256) - 189
FIELDS = [(TEST_MODULUS_2, 2), (MOD_3LIMB, 3), (MOD_NO_SPARE, 4)]
GENERAL = 0x1234567890ABCDEF0FEDCBA987654321  # a coefficient that is neither 1 nor -1

# (K, degree) -> (S, c): the first sumcheck of the CCS shapes of tests/_ccs_wide.py (K = t + 1 tables, eq() last) and
# their like for the pairs those leave out; 1, -1 and general coefficients meet in plonk6 and in (8, 4)
COMBS = {
    (5, 1): ([[0], [1], [2], [3]], [1, -1, GENERAL, 1]),
    (5, 2): ([[0], [1], [2], [3]], [-1, 1, 1, GENERAL]),
    (5, 3): ([[0, 1], [2], [3]], [1, -1, -1]),                          # t4
    (5, 4): ([[0, 1, 2], [3]], [2, -1]),
    (6, 3): ([[0, 1], [2, 3], [4]], [1, GENERAL, -1]),
    (6, 4): ([[0, 1, 2], [3], [4]], [1, -1, 1]),                        # t5d3
    (7, 3): ([[0], [1], [2], [3, 4], [5]], [2, 1, -1, 1, -1]),          # plonk6
    (7, 4): ([[0, 1, 2], [3, 4], [5]], [1, 2, -1]),
    (8, 3): ([[0, 1], [2, 3], [4, 5], [6]], [1, -1, 5, -1]),            # t7d2
    (8, 4): ([[0, 1, 2], [3, 4], [5], [6]], [1, GENERAL, -3, -1]),      # t7d3's masks
}
GRID = sorted(COMBS)
NVS = [1, 2, 6, 13]  # one round without a fold; the smallest fold; one-launch rounds; 4096 points = 128 workgroups + reduce


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


@functools.lru_cache(maxsize=None)
def _tables8(modulus, fl, nv):
    """eight tables of 2^nv canonical field elements (Montgomery limbs): the last from i64 (an eq()-less stand-in that
    has small and negative values), the rest random; tests take the first K - 1 and the last"""
    f = orc.make_field(modulus, fl)
    rng = np.random.default_rng(nv * 17 + fl)
    n = 1 << nv
    out = np.zeros((8, n, fl), dtype=np.uint64)
    for k in range(7):
        raw = rng.bytes(40 * n)
        out[k] = orc.field_elems([int.from_bytes(raw[40 * i: 40 * i + 40], "little") % modulus for i in range(n)], fl)
    w = orc.splitmix64(nv + 7, n)
    out[7] = orc.field_elems([orc.field_from_i64(f, int(v)) for v in w.view(np.int64)], fl)
    out.setflags(write=False)
    return out


def _tables(modulus, fl, K, nv):
    t = _tables8(modulus, fl, nv)
    return np.ascontiguousarray(np.concatenate([t[: K - 1], t[7:]]))


def _comb(modulus, fl, K, degree):
    S, c = COMBS[(K, degree)]
    R = 1 << (64 * fl)
    return S, [sum(1 << j for j in Si) for Si in S], [ci % modulus * R % modulus for ci in c]


@functools.lru_cache(maxsize=None)
def _oracle(modulus, fl, K, degree, nv, form, prime):
    """(msgs, rand, transcript afterwards) of the oracle's prover from a transcript primed with `prime`"""
    f = orc.make_field(modulus, fl)
    to = orc.new_transcript()
    if prime:
        orc.absorb(to, prime)
    mles = _tables(modulus, fl, K, nv)
    if form == "product":
        msgs, rand = orc.sumcheck_prove_product(f, mles, degree, to)
    else:
        _, masks, c = _comb(modulus, fl, K, degree)
        msgs, rand = orc.sumcheck_prove(f, mles, degree, masks, c, to)
    return msgs, rand, to


@pytest.mark.parametrize("modulus,fl", FIELDS)
@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("K,degree", GRID)
def test_rounds_equal_the_oracle(mods, modulus, fl, nv, K, degree):
    """Round by round through the host mirror (transcript on the host): the CCS form and the plain product."""
    _, pcs = mods
    field = pcs.FieldConfig(modulus, fl)
    mles = _tables(modulus, fl, K, nv)
    S, _, c = _comb(modulus, fl, K, degree)
    for form in ("ccs", "product"):
        msgs_o, rand_o, to = _oracle(modulus, fl, K, degree, nv, form, b"wide")
        t = pcs.KeccakTranscript()
        t.absorb(b"wide")
        if form == "ccs":
            msgs, rand = pcs.sumcheck_prove_ccs(t, mles, degree, orc.field_elems(c, fl), S, field)
        else:
            msgs, rand = pcs.sumcheck_prove_product(t, mles, degree, field)
        assert np.array_equal(msgs, msgs_o), form
        assert np.array_equal(rand, rand_o), form
        after = orc.Keccak.from_buffer_copy(to)  # get_u64 squeezes: leave the shared reference as it is
        assert t.get_u64() == orc.lib().orc_tr_get_u64(orc.C.byref(after)), form


# ---------------------------------------------------------------------------------------------- zip_sumcheck_prove
def _lds_tail_bound(K, fl):
    """The default of ZIP_HIP_SUMCHECK_TAIL: K tables of 2^n entries beside the tail kernel's own 4920 bytes in the
    160 KiB of LDS of one workgroup (kernels_sumcheck_tail.cuh), n <= 13"""
    n = 0
    while n < 13 and (K << (n + 1)) * fl * 8 + 4920 <= 160 * 1024:
        n += 1
    return n


def _state_of(cabi, to):
    return cabi.KeccakState.make(st=[int(w) for w in to.st], buf=bytes(to.buf[: to.buflen]))


def _prove_and_check(cabi, modulus, fl, K, degree, nv, form, prime, tables=None, what=""):
    msgs_o, rand_o, to = _oracle(modulus, fl, K, degree, nv, form, prime)
    before = orc.new_transcript()
    if prime:
        orc.absorb(before, prime)
    state = _state_of(cabi, before)
    comb = None
    if form == "ccs":
        _, masks, c = _comb(modulus, fl, K, degree)
        comb = cabi.make_comb(masks, orc.field_elems(c, fl))
    mles = _tables(modulus, fl, K, nv) if tables is None else tables
    sc = cabi.Sumcheck(mles, nv, degree, cabi.make_field(modulus, fl), comb=comb)
    rounds0, tails0 = cabi.sumcheck_launch_counts()
    msgs, rand = sc.prove(state)
    rounds1, tails1 = cabi.sumcheck_launch_counts()
    bound = _lds_tail_bound(K, fl)
    knob = os.environ.get("ZIP_HIP_SUMCHECK_TAIL")
    n_tail = min(bound if knob is None else int(knob), bound, nv)
    assert tails1 - tails0 == (1 if n_tail else 0), what  # every path gives the same bytes: the counts tell which ran
    assert rounds1 - rounds0 == nv - n_tail, what
    assert np.array_equal(msgs, msgs_o), what
    assert np.array_equal(rand, rand_o), what
    assert [int(w) for w in state.st] == [int(w) for w in to.st], what
    assert state.buflen == to.buflen and state.pending() == bytes(to.buf[: to.buflen]), what
    assert not any(state.buf[state.buflen:]), what
    with pytest.raises(cabi.ZipError, match="not active"):
        sc.round(rand_o[-1])
    sc.free()


@pytest.mark.parametrize("modulus,fl", FIELDS)
@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("K,degree", GRID)
def test_prove_in_one_call_equals_the_oracle(mods, monkeypatch, modulus, fl, nv, K, degree):
    """The default tail: as many rounds as fit the LDS (all of them up to nv = 9; at nv = 13 the wide round kernel plays
    the rounds before).  The sponge starts at offset 0, 135 or in between."""
    cabi, _ = mods
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)
    prime = (b"", bytes(range(135)), bytes(range(71)))[(K + degree + nv) % 3]
    for form in ("ccs", "product"):
        _prove_and_check(cabi, modulus, fl, K, degree, nv, form, prime, what=form)


@pytest.mark.parametrize("tail", ["0", "1", "bound"])
@pytest.mark.parametrize("offset", [0, 71, 135])
@pytest.mark.parametrize("modulus,fl,K,degree", [(TEST_MODULUS_2, 2, 5, 3), (MOD_3LIMB, 3, 7, 3), (MOD_NO_SPARE, 4, 8, 4)])
def test_prove_with_the_tail_knob(mods, monkeypatch, modulus, fl, K, degree, offset, tail):
    """ZIP_HIP_SUMCHECK_TAIL: no tail kernel (every round on the wide kernel), a one-round tail, the bound itself."""
    cabi, _ = mods
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_TAIL", str(_lds_tail_bound(K, fl)) if tail == "bound" else tail)
    for form in ("ccs", "product"):
        _prove_and_check(cabi, modulus, fl, K, degree, 13, form, bytes(range(offset)), what=form)


# ---------------------------------------------------------------------------------------------- large, device-resident
def test_2pow18_device_tables_take_several_passes_and_are_only_read(mods):
    """K = 5, two limbs, degree 3 at 2^18 (20 MiB): round 1 has 2^17 points = 4096 workgroups' worth, more than the
    grid ever has (at most 8 per CU), so the grid-stride loop runs more than once."""
    import torch

    cabi, _ = mods
    nv, fl, K, degree, modulus = 18, 2, 5, 3, TEST_MODULUS_2
    assert (1 << (nv - 1)) // 32 > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    f = orc.make_field(modulus, fl)
    rng = np.random.default_rng(18)
    mles = rng.integers(0, 1 << 62, size=(K, 1 << nv, fl), dtype=np.uint64)
    mles[..., fl - 1] >>= np.uint64(34)  # canonical: below 2^92 < q (95 bits)
    _, masks, c = _comb(modulus, fl, K, degree)
    msgs_o, rand_o = orc.sumcheck_prove(f, mles, degree, masks, c, orc.new_transcript())
    dev = [torch.from_numpy(mles[k].view(np.int64)).cuda() for k in range(K)]
    before = [d.clone() for d in dev]
    sc = cabi.Sumcheck(dev, nv, degree, cabi.make_field(modulus, fl), comb=cabi.make_comb(masks, orc.field_elems(c, fl)))
    r = None
    for i in range(nv):
        assert np.array_equal(sc.round(r), msgs_o[i]), i
        r = rand_o[i]
    with pytest.raises(cabi.ZipError):  # "Prover is not active" (prover.rs:91-93)
        sc.round(r)
    sc.free()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


def test_usage_errors(mods):
    cabi, _ = mods
    zf = cabi.make_field(MOD_NO_SPARE, 4)
    one = np.ones((1, 4), dtype=np.uint64)
    for n_mles, degree, comb in ((9, 3, None), (5, 5, None), (8, 5, None), (5, 3, cabi.make_comb([1 << 5], one)),
                                 (8, 4, cabi.make_comb([1 << 8], one))):
        with pytest.raises(cabi.ZipError) as e:
            cabi.Sumcheck(np.zeros((n_mles, 8, 4), dtype=np.uint64), 3, degree, zf, comb=comb)
        assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM, (n_mles, degree)
    sc = cabi.Sumcheck(np.zeros((8, 8, 4), dtype=np.uint64), 3, 4, zf, comb=cabi.make_comb([1 << 7], one))
    with pytest.raises(cabi.ZipError):
        sc.round(np.ones(4, dtype=np.uint64))  # "first round should be prover first." (prover.rs:69-71)
    assert not sc.round().any()  # all-zero tables: the zero polynomial
    with pytest.raises(cabi.ZipError):
        sc.round()                             # "verifier message is empty" (prover.rs:87-89)
    sc.free()
