"""GPU: zip_sumcheck_init_products -- a sum of products sum_p c_p * prod_{j in S_p} v_j over up to 32 MLEs in ONE handle
(sumcheck_round_products_kernel: one pass per round over all tables) against the oracle's prove_as_subprotocol with
rand_poly_comb_fn, bit for bit: every round message, every challenge, and the transcript afterwards."""
import functools

import numpy as np
import pytest

import _oracle as orc

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
Q192 = 312829638388039969874974628075306023441  # 3-limb prime 1 of the benchmark (sumcheck_benches.rs:43)
FIELDS = [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2), (MOD_3LIMB, 3), (MOD_NO_SPARE, 4)]

BENCH_SHAPE = (2, 3, 4, 2, 3, 4, 3)
OVERLAP = "overlap"  # masks [0b0011, 0b0110, 0b0001, 0b0011] over 4 MLEs: a shared MLE, a single factor, a repeated mask,
#                      and MLE 3 in no product
SHAPES = [(2,), (1, 2), (2, 3, 4), BENCH_SHAPE, (4,) * 8, OVERLAP]
NUM_VARS = [1, 2, 3, 6, 10, 13]


@pytest.fixture(scope="module")
def mods():
    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return cabi, pcs


def _masks(shape):
    if shape == OVERLAP:
        return [0b0011, 0b0110, 0b0001, 0b0011], 4
    masks, k = [], 0
    for m in shape:
        masks.append(sum(1 << (k + i) for i in range(m)))
        k += m
    return masks, k


def _residues(rng, modulus, fl, shape):
    """canonical residues as raw Montgomery limbs: random below the modulus' top limb, that one below the modulus' own"""
    top = (modulus.bit_length() - 1) // 64
    a = np.zeros(shape + (fl,), dtype=np.uint64)
    a[..., :top] = rng.integers(0, 2**64, size=shape + (top,), dtype=np.uint64)
    a[..., top] = rng.integers(0, modulus >> (64 * top), size=shape, dtype=np.uint64)
    return a


def _coeffs(rng, modulus, fl, n):
    """random coefficients with 1, q - 1 and 0 (Montgomery: R, q - R, 0) among them where there is room"""
    R = (1 << (64 * fl)) % modulus
    c = [orc.limbs_to_int(x) for x in _residues(rng, modulus, fl, (n,))]
    special = [R, modulus - R, 0]
    for i, v in enumerate(special[: max(n - 1, 0)]):  # (at least one random coefficient stays)
        c[(i + 1) % n] = v
    return c


@functools.lru_cache(maxsize=None)
def _case(modulus, fl, nv, shape, degree=None, carry=False, prime=b""):
    """(tables, masks, coeffs as ints, degree, oracle msgs, oracle rand, oracle transcript afterwards); computed once
    and shared, never written"""
    masks, K = _masks(shape)
    rng = np.random.default_rng(nv * 1000 + K * 10 + fl)
    if carry:  # every entry q - 1: the largest products, the accumulator's carries run all the way
        tables = np.tile(orc.field_elems([modulus - 1], fl)[0], (K, 1 << nv, 1))
    else:
        tables = _residues(rng, modulus, fl, (K, 1 << nv))
    coeffs = [modulus - 1] * len(masks) if carry else _coeffs(rng, modulus, fl, len(masks))
    if degree is None:
        degree = max(bin(m).count("1") for m in masks)
    to = orc.new_transcript()
    if prime:
        orc.absorb(to, prime)
    msgs, rand = orc.sumcheck_prove_products(orc.make_field(modulus, fl), tables, degree, masks, coeffs, to)
    for a in (tables, msgs, rand):
        a.setflags(write=False)
    return tables, masks, coeffs, degree, msgs, rand, to


def _handle(cabi, modulus, fl, nv, tables, masks, coeffs, degree):
    comb = cabi.make_comb(masks, orc.field_elems(coeffs, fl))
    return cabi.Sumcheck(tables, nv, degree, cabi.make_field(modulus, fl), comb=comb, products=True)


def _play(sc, nv, msgs_o, rand_o, what=""):
    r = None
    for i in range(nv):
        assert np.array_equal(sc.round(r), msgs_o[i]), (what, i)
        r = rand_o[i]


@pytest.mark.parametrize("modulus,fl", FIELDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
@pytest.mark.parametrize("nv", NUM_VARS)
def test_rounds_equal_the_oracle(mods, modulus, fl, nv, shape):
    """nv = 1: no fold, one point; 2, 3: the first fold and both ping-pong buffers; 10: 32 workgroups (the last one folds
    the partials); 13: 256 workgroups (sumcheck_reduce_kernel folds them)"""
    cabi, _ = mods
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(modulus, fl, nv, shape)
    sc = _handle(cabi, modulus, fl, nv, tables, masks, coeffs, degree)
    _play(sc, nv, msgs_o, rand_o)
    with pytest.raises(cabi.ZipError, match="not active"):
        sc.round(rand_o[-1])
    sc.free()


@pytest.mark.parametrize("modulus,fl", FIELDS)
@pytest.mark.parametrize("nv", [1, 3, 10])
def test_degree_above_the_largest_product(mods, modulus, fl, nv):
    """rand_poly hands over the maximum it could have drawn: degree 4 with one product of two"""
    cabi, _ = mods
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(modulus, fl, nv, (2,), degree=4)
    assert degree == 4 and msgs_o.shape[1] == 5
    sc = _handle(cabi, modulus, fl, nv, tables, masks, coeffs, degree)
    _play(sc, nv, msgs_o, rand_o)
    sc.free()


@pytest.mark.parametrize("modulus,fl", FIELDS)
def test_carry_stress_every_entry_q_minus_1(mods, modulus, fl):
    cabi, _ = mods
    nv = 10
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(modulus, fl, nv, BENCH_SHAPE, carry=True)
    sc = _handle(cabi, modulus, fl, nv, tables, masks, coeffs, degree)
    _play(sc, nv, msgs_o, rand_o)
    sc.free()


def test_device_resident_tables_2pow16_are_only_read(mods):
    import torch

    cabi, _ = mods
    nv = 16
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(Q192, 3, nv, BENCH_SHAPE)
    dev = [torch.from_numpy(np.array(tables[k]).view(np.int64)).cuda() for k in range(tables.shape[0])]
    before = [d.clone() for d in dev]
    sc = _handle(cabi, Q192, 3, nv, dev, masks, coeffs, degree)
    _play(sc, nv, msgs_o, rand_o)
    sc.free()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


# ------------------------------------------------------------------ zip_sumcheck_prove on the handle
def _state_of(cabi, to):
    return cabi.KeccakState.make(st=[int(w) for w in to.st], buf=bytes(to.buf[: to.buflen]))


def _assert_state_equal(state, to, what=""):
    assert [int(w) for w in state.st] == [int(w) for w in to.st], what
    assert state.buflen == to.buflen, what
    assert state.pending() == bytes(to.buf[: to.buflen]), what
    assert not any(state.buf[state.buflen:]), what


@pytest.mark.parametrize("primed", [0, 1, 135, 136])
@pytest.mark.parametrize("modulus,fl,nv,shape", [(Q192, 3, 10, BENCH_SHAPE), (BENCH_MODULUS, 4, 13, OVERLAP), (TEST_MODULUS_2, 2, 1, (2,)),
                                                 (MOD_NO_SPARE, 4, 6, (4,) * 8)])
def test_prove_in_one_call(mods, modulus, fl, nv, shape, primed):
    """messages, challenges and the sponge afterwards; every round through the round kernel, no tail kernel"""
    cabi, _ = mods
    prime = bytes(range(primed))
    tables, masks, coeffs, degree, msgs_o, rand_o, to_after = _case(modulus, fl, nv, shape, prime=prime)
    to = orc.new_transcript()
    if prime:
        orc.absorb(to, prime)
    state = _state_of(cabi, to)
    sc = _handle(cabi, modulus, fl, nv, tables, masks, coeffs, degree)
    rounds0, tails0 = cabi.sumcheck_launch_counts()
    msgs, rand = sc.prove(state)
    rounds1, tails1 = cabi.sumcheck_launch_counts()
    assert (rounds1 - rounds0, tails1 - tails0) == (nv, 0)
    assert np.array_equal(msgs, msgs_o) and np.array_equal(rand, rand_o)
    _assert_state_equal(state, to_after)
    with pytest.raises(cabi.ZipError, match="already") as e:  # a second zip_sumcheck_prove
        sc.prove(cabi.KeccakState.make())
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    with pytest.raises(cabi.ZipError, match="not active"):
        sc.round(rand_o[-1])
    sc.free()


def test_prove_after_a_round_is_refused(mods):
    cabi, _ = mods
    nv = 6
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(Q192, 3, nv, (2, 3, 4))
    sc = _handle(cabi, Q192, 3, nv, tables, masks, coeffs, degree)
    assert np.array_equal(sc.round(), msgs_o[0])
    with pytest.raises(cabi.ZipError, match="fresh") as e:
        sc.prove(cabi.KeccakState.make())
    assert e.value.code == cabi.ZIP_ERR_INVALID_PARAM
    for i in range(1, nv):  # and the handle still finishes its rounds one by one
        assert np.array_equal(sc.round(rand_o[i - 1]), msgs_o[i]), i
    sc.free()


# ------------------------------------------------------------------ round_begin / round_end
def test_two_handles_in_flight(mods):
    cabi, _ = mods
    L = cabi.lib()
    nv = 10
    ca = _case(Q192, 3, nv, BENCH_SHAPE)
    cb = _case(BENCH_MODULUS, 4, nv, OVERLAP)
    a = _handle(cabi, Q192, 3, nv, *ca[:4])
    b = _handle(cabi, BENCH_MODULUS, 4, nv, *cb[:4])
    out_a = np.zeros((ca[3] + 1, 3), dtype=np.uint64)
    out_b = np.zeros((cb[3] + 1, 4), dtype=np.uint64)
    for i in range(nv):
        ra = None if i == 0 else np.ascontiguousarray(ca[5][i - 1])
        rb = None if i == 0 else np.ascontiguousarray(cb[5][i - 1])
        assert L.zip_sumcheck_round_begin(a._h, None if ra is None else ra.ctypes.data) == 0
        assert L.zip_sumcheck_round_begin(b._h, None if rb is None else rb.ctypes.data) == 0
        assert L.zip_sumcheck_round_end(b._h, out_b.ctypes.data) == 0
        assert L.zip_sumcheck_round_end(a._h, out_a.ctypes.data) == 0
        assert np.array_equal(out_a, ca[4][i]) and np.array_equal(out_b, cb[4][i]), i
    a.free()
    b.free()


def test_round_begin_end_protocol(mods):
    cabi, _ = mods
    L = cabi.lib()
    nv = 6
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(Q192, 3, nv, (2, 3, 4))
    a = _handle(cabi, Q192, 3, nv, tables, masks, coeffs, degree)
    out = np.zeros((degree + 1, 3), dtype=np.uint64)
    assert L.zip_sumcheck_round_end(a._h, out.ctypes.data) == cabi.ZIP_ERR_INVALID_PARAM     # nothing in flight
    assert L.zip_sumcheck_round_begin(a._h, None) == 0
    assert L.zip_sumcheck_round_begin(a._h, None) == cabi.ZIP_ERR_INVALID_PARAM               # not collected yet
    assert L.zip_sumcheck_round_end(a._h, out.ctypes.data) == 0
    assert np.array_equal(out, msgs_o[0])
    r = np.ascontiguousarray(rand_o[0])
    assert L.zip_sumcheck_round_begin(a._h, r.ctypes.data) == 0
    assert L.zip_sumcheck_round_end(a._h, out.ctypes.data) == 0
    assert np.array_equal(out, msgs_o[1])
    a.free()


# ------------------------------------------------------------------ the host mirror
def _mirror(pcs, cabi, monkeypatch, fused, onecall, modulus, fl, tables, masks, coeffs, degree, prime=b"mirror"):
    for name, v in (("ZIP_HIP_SUMCHECK_FUSED", fused), ("ZIP_HIP_SUMCHECK_ONECALL", onecall)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    t = pcs.KeccakTranscript()
    t.absorb(prime)
    rounds0, tails0 = cabi.sumcheck_launch_counts()
    msgs, rand = pcs.sumcheck_prove_products(t, np.array(tables), degree, np.array(masks, dtype=np.uint32),
                                             orc.field_elems(coeffs, fl), pcs.FieldConfig(modulus, fl))
    rounds1, tails1 = cabi.sumcheck_launch_counts()
    assert tails1 == tails0  # neither path launches the tail kernel
    return msgs, rand, t.get_u64(), rounds1 - rounds0


@pytest.mark.parametrize("modulus,fl,nv,shape", [(Q192, 3, 10, BENCH_SHAPE), (BENCH_MODULUS, 4, 6, OVERLAP), (TEST_MODULUS_2, 2, 3, (1, 2))])
@pytest.mark.parametrize("fused,onecall", [("0", None), ("1", None), ("1", "1"), ("0", "1")])
def test_mirror_equals_the_oracle_on_both_paths(mods, monkeypatch, modulus, fl, nv, shape, fused, onecall):
    cabi, pcs = mods
    tables, masks, coeffs, degree, msgs_o, rand_o, to = _case(modulus, fl, nv, shape, prime=b"mirror")
    msgs, rand, u64, rounds = _mirror(pcs, cabi, monkeypatch, fused, onecall, modulus, fl, tables, masks, coeffs, degree)
    assert np.array_equal(msgs, msgs_o) and np.array_equal(rand, rand_o)
    to2 = orc.Keccak.from_buffer_copy(to)  # (get_u64 moves the sponge: the shared case stays as it is)
    assert u64 == orc.lib().orc_tr_get_u64(orc.C.byref(to2))
    # the path taken: one round kernel per round, or one per product and round
    assert rounds == (nv if fused == "1" else len(masks) * nv)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_nine_products_take_the_loop(mods, monkeypatch, fused):
    cabi, pcs = mods
    modulus, fl, nv, shape = Q192, 3, 6, (2,) * 9
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _case(modulus, fl, nv, shape, prime=b"mirror")
    msgs, rand, _, rounds = _mirror(pcs, cabi, monkeypatch, fused, None, modulus, fl, tables, masks, coeffs, degree)
    assert np.array_equal(msgs, msgs_o) and np.array_equal(rand, rand_o)
    assert rounds == 9 * nv


@pytest.mark.parametrize("fused", ["0", "1"])
def test_bad_shapes_raise_the_same_exceptions(mods, monkeypatch, fused):
    """the two bad shapes of tests/test_gpu_sumcheck.py: checked before a path is chosen"""
    cabi, pcs = mods
    monkeypatch.setenv("ZIP_HIP_SUMCHECK_FUSED", fused)
    field = pcs.FieldConfig(BENCH_MODULUS, 4)
    rng = np.random.default_rng(1)
    tables = _residues(rng, BENCH_MODULUS, 4, (4, 8))
    coeffs = _residues(rng, BENCH_MODULUS, 4, (2,))
    big = _residues(rng, BENCH_MODULUS, 4, (5, 8))
    rounds0 = cabi.sumcheck_launch_counts()[0]
    with pytest.raises(pcs.InvalidPcsParam):  # five multiplicands in one product
        pcs.sumcheck_prove_products(pcs.KeccakTranscript(), big, 5, np.array([31], dtype=np.uint32), coeffs[:1], field)
    with pytest.raises(pcs.ReferencePanic):   # a product refers to an MLE that does not exist
        pcs.sumcheck_prove_products(pcs.KeccakTranscript(), tables, 2, np.array([3, 1 << 7], dtype=np.uint32), coeffs, field)
    with pytest.raises(pcs.InvalidPcsParam):  # the count is checked first, in product order
        pcs.sumcheck_prove_products(pcs.KeccakTranscript(), tables, 2, np.array([0b11111 << 3, 3], dtype=np.uint32), coeffs, field)
    assert cabi.sumcheck_launch_counts()[0] == rounds0  # nothing was played
